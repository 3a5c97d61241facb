"""The per-image front end shared by the generator CLI (gen_3dphoto_dynamic.py) and the online pair source (online.py): the draw schedule,
the intrinsics, the model and its engine, and a Lane that turns one decoded image into rendered pairs.  One copy, so that both callers
render the same pairs for the same seed and producer flags."""
import contextlib
import os
import random

import numpy as np
import torch

from . import _lib, host_math, ops, pipeline, synth

PRECISE_DTYPES = {"fp32": torch.float32, "fp32-mfma": torch.float32, "fp64": torch.float64}     # model_dtype -> PrecisePredictor's dtype


def intrinsics(W, H):
    """K [1,3,3] float32 as gen_3dphoto_dynamic_v2.py:42-49 computes it (rows scaled in float32: not synth.intrinsics, which rounds
    differently)."""
    K = torch.tensor([[0.58, 0, 0.5], [0, 0.58, 0.5], [0, 0, 1]])
    K[0, :] *= W
    K[1, :] *= H
    return K.unsqueeze(0)


def parse_disp_filter(disp_filter):
    """disp_filter= of Lane / OnlinePairs and --disp-filter of the CLI: None, "5,5" or a sequence of windows -> None or a tuple of odd
    windows in 3..9 (ops.sparse_bilateral_filter runs one iteration per window)."""
    if disp_filter is None or disp_filter == "" or disp_filter is False:
        return None
    try:
        sizes = tuple(int(s) for s in (disp_filter.split(",") if isinstance(disp_filter, str) else disp_filter))
    except (TypeError, ValueError):
        raise ValueError("disp_filter must be windows such as 5,5 (got %r)" % (disp_filter,)) from None
    if not sizes or any(s not in (3, 5, 7, 9) for s in sizes) or len(sizes) > _lib.BILATERAL_MAX_ITER:
        raise ValueError("disp_filter must be 1..%d windows, each 3, 5, 7 or 9 (got %r)" % (_lib.BILATERAL_MAX_ITER, disp_filter))
    return sizes


def mpi_from_disparity(image_3HW, disp_HW, S):
    """Stand-in MPI producer (--mpi-from disparity): colours on every plane, sigma = 1e-4 except 50 on the plane nearest to the pixel's
    disparity (a hard depth assignment).  Returns (mpi [S,4,H,W], disparity [S])."""
    planes = torch.from_numpy(synth.plane_disparities(S)).to(disp_HW.device)
    idx = (disp_HW.unsqueeze(0) - planes.view(S, 1, 1)).abs().argmin(0)
    sigma = torch.full((S,) + tuple(disp_HW.shape), 1e-4, dtype=torch.float32, device=disp_HW.device)
    sigma.scatter_(0, idx.unsqueeze(0), 50.0)
    mpi = torch.cat([image_3HW.unsqueeze(0).expand(S, -1, -1, -1), sigma.unsqueeze(1)], dim=1).contiguous()
    return mpi, planes


class PlaneRefused(ValueError):
    """An image whose adjusted planes cannot be rendered: a plane with a disparity of 0 or below (or NaN) has no depth"""


def check_planes(name, planes_host):
    """planes_host [S] on the host, the plane-adjustment network's output for image `name`: unbounded, handed on as it is - and refused here,
    before anything renders on it, where a plane has no depth"""
    bad = ~(planes_host > 0)
    if bool(bad.any()):
        k = int(torch.nonzero(bad)[0])
        raise PlaneRefused("image %s: plane %d of %d has disparity %g after plane adjustment; a plane needs a disparity above 0 to have a depth. "
                           "The network's output is handed on as it is (not clamped, not re-sorted), so this image is not rendered"
                           % (name, k, planes_host.numel(), float(planes_host[k])))


def load_model(ckpt_path, W, H, planes, device, adjust_planes=False):
    """The MPIPredictor of a checkpoint (which carries its own num_planes) or of "random:SEED" (deterministic random weights, `planes` planes),
    on `device`; adjust_planes: MPIPredictor's.  Leaves torch's global RNG as it was: module construction draws default initialisations from it."""
    from .model import MPIPredictor
    ckpt_path = str(ckpt_path)
    with torch.random.fork_rng(devices=[]):
        if ckpt_path.startswith("random:"):
            return MPIPredictor(W, H, planes, adjust_planes=adjust_planes).randomize_(int(ckpt_path.split(":")[1])).eval().to(device)
        if not os.path.exists(ckpt_path):
            raise FileNotFoundError("checkpoint %r not found" % (ckpt_path,))
        return MPIPredictor.from_checkpoint(ckpt_path, W, H, adjust_planes=adjust_planes).to(device)


def make_predictor(model, model_dtype):
    """The HIP engine for `model_dtype`: fp32 | fp32-mfma | fp64 = PrecisePredictor (parity grade, eager), auto | fp16 = HipPredictor (fp16
    storage, one graph per image)."""
    if model_dtype in PRECISE_DTYPES:
        from .model.precise import PrecisePredictor
        return PrecisePredictor(model, dtype=PRECISE_DTYPES[model_dtype], x3=model_dtype == "fp32")
    if model_dtype in ("auto", "fp16"):
        from .model.engine import HipPredictor
        return HipPredictor(model, graph=True)
    raise ValueError("model_dtype must be auto, fp16, fp32, fp32-mfma or fp64")


class Schedule:
    """The CLI's draw schedule on private streams: random.Random(seed) / np.random.RandomState(seed) replay what the reference draws from the
    global `random` / `np.random` seeded with `seed`.  draw(mask_max) -> (obj_indices, pose_params), or None (no instance: no draws)."""

    def __init__(self, seed, ext_cz, pairs_per_image, poses="v2"):
        self.rng = random.Random(seed)
        self.nrs = np.random.RandomState(seed)
        self.ext_cz, self.R, self.poses = ext_cz, pairs_per_image, poses

    def draw(self, mask_max):
        if mask_max <= 0:
            return None
        obj_indices, pose_params = [], []
        for _ in range(self.R):
            obj_indices.append(int(self.nrs.randint(mask_max)) + 1)                                                         # :101
            pose_params.append(host_math.draw_pose_parameters(self.ext_cz, rng=self.rng, profile=self.poses))                 # utils.py:207
            pose_params.append(host_math.draw_pose_parameters(self.ext_cz, base_motions=[0, 0, 0], rng=self.rng, profile=self.poses))   # :208
        return obj_indices, pose_params

    def state(self):
        return dict(rng=self.rng.getstate(), nrs=self.nrs.get_state())

    def set_state(self, st):
        self.rng.setstate(st["rng"])
        self.nrs.set_state(st["nrs"])


class Lane:
    """Everything one in-flight image owns: its render stream and tail stream, the blended plane stack (PairRenderer), the input buffers,
    the hole-fill workspace and the network engine.  Built ON the lane's stream, so that the zero-fill of the stack and the packed weights
    are ordered before its first use.

    model_dtype: the HIP engine make_predictor builds for `model`; None runs `model` as torch modules under autocast `amp`.  lap(label): a
    context factory timing the stages (no-op by default).  streams: (render, tail) streams the caller created, default two new ones.
    disp_filter: None, or the windows of ops.sparse_bilateral_filter (such as (5, 5)), run on the uploaded disparity bytes at file
    resolution before the input stage.  A model built with adjust_planes=True moves the planes per image: front() runs the plane-adjustment
    network once, copies its S values to the host once (the renderer's homographies are built there), refuses an image with a plane at or
    below 0 (PlaneRefused, before anything renders) and hands the same values to the engine and to the renderer.  front() and pairs() enqueue on the current stream: call them inside torch.cuda.stream(lane.stream)."""

    def __init__(self, device, H, W, planes, model=None, model_dtype=None, amp=None, lap=contextlib.nullcontext, streams=None, disp_filter=None):
        self.device, self.H, self.W, self.planes, self.K = device, H, W, planes, intrinsics(W, H)
        self.model, self.amp, self.lap = model, amp, lap
        self.disp_filter = parse_disp_filter(disp_filter)
        self.stream, self.tail_stream = streams or (torch.cuda.Stream(device=device), torch.cuda.Stream(device=device))
        self.stream.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(self.stream):
            self.renderer = pipeline.PairRenderer(planes, H, W, device)
            self.fill_ws = torch.empty(int(_lib.load().mpf_fill_holes_workspace(H, W)), dtype=torch.uint8, device=device)
            self.ns_ws = None                                     # fill "ns-hip": sized by its first use (ns_workspace)
            self.inputs = dict(image=torch.empty((3, H, W), device=device), disp=torch.empty((H, W), device=device))
            self.predictor = make_predictor(model, model_dtype) if model is not None and model_dtype is not None else None
        self.adjust_planes = bool(getattr(model, "adjust_planes", False))
        self.tail_stream.wait_stream(self.stream)

    def ns_workspace(self, B):
        """The workspace of fill "ns-hip" (ops.inpaint_ns) for B frames: allocated on the current stream at first use, grown when short."""
        need = ops.inpaint_ns_workspace(B, self.H, self.W)
        if self.ns_ws is None or self.ns_ws.numel() < need:
            self.ns_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self.ns_ws

    def front(self, item, npz=None):
        """item (io_formats.InputPrefetcher's): upload, input stage (:82-89), MPI producer - the stack in the file `npz` if given, else the
        network, else mpi_from_disparity - and the blend into renderer.src_u8 (:122).  -> what pairs() needs."""
        dev, H, W = self.device, self.H, self.W
        with self.lap("upload + resize image, disparity"):
            rgb8 = item["rgb_u8"].to(dev, non_blocking=True)
            dsp8 = item["disp_u8"].to(dev, non_blocking=True)
            ids = item["ids_u8"].to(dev, non_blocking=True)
            if self.disp_filter is not None:
                dsp8 = ops.sparse_bilateral_filter(dsp8.contiguous(), self.disp_filter)
            if rgb8.shape[:2] == dsp8.shape[:2]:
                pre = ops.prepare_inputs(rgb_u8=rgb8, disp_u8=dsp8, size=(H, W), out=self.inputs)     # :82-89 in one launch
            else:                                                          # files of different sizes: each resized on its own, as :86-89 does
                pre = dict(image=ops.prepare_inputs(rgb_u8=rgb8, size=(H, W), out=self.inputs)["image"],
                           disp=ops.prepare_inputs(disp_u8=dsp8, size=(H, W), out=self.inputs)["disp"])
            image, disp = pre["image"][None], pre["disp"][None, None]
        cum_mask = None
        with self.lap("MPI producer + blend"):
            if npz is not None:
                z = np.load(npz)
                mpi, planes = torch.from_numpy(z["mpi"]).to(dev), torch.from_numpy(z["disparity"]).to(dev)
            elif self.predictor is not None and self.adjust_planes:
                with torch.no_grad():
                    pd = self.model.render_disparities(image, disp)[0].float().contiguous()
                # the image's one device-to-host copy of its S planes (256 bytes at S = 64): the host waits here for the upload and the
                # plane-adjustment network, BEFORE the engine's forward is enqueued, so the wait does not include it
                planes = pd.cpu()
                check_planes(item.get("name", item.get("i")), planes)
                mpi, cum_mask, _ = self.predictor(image, disp, plane_disp=pd)       # the engine reads the device values, the renderer the host's
            elif self.predictor is not None:
                mpi, cum_mask, planes = self.predictor(image, disp)        # static buffers: consumed by blend() below
            elif self.model is not None:
                with torch.no_grad(), torch.autocast("cuda", dtype=self.amp, enabled=self.amp is not None):      # :92-93
                    raw, cm, pd = self.model(image, disp, raw=True)
                mpi, cum_mask, planes = raw[0].float().contiguous(), cm[0].float().contiguous(), pd[0].float()
                if self.adjust_planes:                                     # the torch modules ran the network inside their forward: the same copy and check
                    planes = planes.cpu()
                    check_planes(item.get("name", item.get("i")), planes)
            else:
                mpi, planes = mpi_from_disparity(image[0], disp[0, 0], self.planes)
            self.renderer.blend(mpi, image[0], self.K, planes, cum_mask=cum_mask)      # once per image; its pairs reuse it
        return image[0], ids, mpi, planes, cum_mask

    def pairs(self, front, obj_indices, pose_params):
        """The image's pairs from front()'s result and its schedule draws: instance masks (:102-105) and run_pairs.  -> run_pairs' results."""
        image, ids, mpi, planes, cum_mask = front
        poses = host_math.poses_from_parameters(pose_params)               # the image's 2 x repeat poses in one batched evaluation
        with self.lap("instance masks"):
            obj_masks = [ops.prepare_inputs(ids_u8=ids, obj_index=k, size=(self.H, self.W))["mask"] for k in obj_indices]
        with self.lap("render pairs"):
            # utils.py:207-208 draws the dynamic pose first; the camera pose renders with obj_mask, the dynamic one with 1 - obj_mask
            return self.renderer.run_pairs(mpi, image, self.K, planes, obj_masks, [(poses[2 * r + 1], poses[2 * r]) for r in range(len(obj_indices))],
                                           cum_mask=cum_mask)
