"""The per-call plane set of the two engines (HipPredictor, PrecisePredictor): one device buffer at a fixed address that every forward - and a
captured graph - reads, holding the model's fixed planes until a call brings its own (the plane-adjustment network's output for its image)."""
from .._tensors import check_devices, check_tensor


class PerCallPlanes:
    def _init_planes(self, model, dev):
        import torch
        self._plane_disp = model.plane_disparities(torch.zeros(1, device=dev))[0].contiguous()      # linspace(1, 0.001, S+2)[1:-1]
        self._planes, self._planes_are_fixed = self._plane_disp.clone(), True

    def _set_planes(self, plane_disp):
        """plane_disp: None = the fixed planes, or a device [S] float32 tensor, copied on the current stream into the buffer the forward reads.
        The fixed planes are written back only after a call that changed them, so a caller that never passes a plane set pays no copy."""
        if plane_disp is None:
            if not self._planes_are_fixed:
                self._planes.copy_(self._plane_disp)
                self._planes_are_fixed = True
            return
        who = type(self).__name__
        S = self._planes.numel()
        check_tensor(plane_disp, "plane_disp", who, (S,), "[S] with the model's S = %d" % S)
        check_devices(who, dict(planes=self._planes, plane_disp=plane_disp))
        self._planes.copy_(plane_disp)
        self._planes_are_fixed = False
