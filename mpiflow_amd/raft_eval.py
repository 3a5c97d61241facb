"""RAFT evaluation (RAFT/evaluate.py) on frames of any size: upstream's InputPadder, and the numbers of validate_chairs / validate_sintel /
validate_kitti accumulated on the device.

    from mpiflow_amd.raft import RAFT
    from mpiflow_amd.raft_eval import FlowMetrics, InputPadder
    model = RAFT(args).cuda().eval()
    metrics = FlowMetrics()
    for image1, image2, flow_gt, valid_gt in dataset:                    # [3,H,W], [3,H,W], [2,H,W], [H,W]: any H, W
        flow_low, flow_pr = model.predict(image1[None].cuda(), image2[None].cuda(), iters=24, mode="kitti")
        metrics.update(flow_pr, flow_gt[None].cuda(), valid_gt[None].cuda())     # no host copy, no synchronisation
    print(metrics.result("kitti"))                                       # one device-to-host copy: {'kitti-epe': ..., 'kitti-f1': ...}

InputPadder is RAFT/core/utils/utils.py's class: the same constructor, `_pad = [left, right, top, bottom]`, pad() and unpad(), plus pair():
the scaled and padded [2N,3,Hp,Wp] batch RAFT's feature network takes, in one launch (ops.raft_images_padded), which RAFT.predict uses.

FlowMetrics.update launches mpf_flow_metrics (ops.flow_metrics): per frame six float64 sums stay on the device.  A pixel counts when
valid >= 0.5 (every pixel without valid); sequence_loss's max_flow rule is NOT applied: evaluate.py has none.  result() copies them once.

forward_interpolate is RAFT/core/utils/utils.py's function, the warm start of create_sintel_submission, on the device
(ops.forward_interpolate: an exact nearest-source search); upstream's line keeps working:

    flow_low, flow_pr = model.predict(image1, image2, iters=32, flow_init=flow_prev)
    flow_prev = forward_interpolate(flow_low[0])[None].cuda()            # already on the device: .cuda() is a no-op

or, without the line: model.predict(image1, image2, iters=32, warm_start=flow_low_of_the_previous_pair), or the whole loop:

    for flow_low, flow_pr in predict_sequence(model, frames, iters=32):  # frames: an iterable of [N,3,H,W] batches

What upstream does with a prediction: flow_to_image is flow_viz.flow_to_image on the device, save_flow_image
demo.py's picture as a PNG, write_flow_kitti / read_flow_kitti frame_utils' KITTI pair without OpenCV; .flo is io_formats.write_flo.

    picture = flow_to_image(flow_pr, image=image1)                       # uint8 [N,2H,W,3] on the device: the frame above its colour-coded flow
    write_flow_kitti("000000_10.png", flow_pr[0])                        # create_kitti_submission's file

Not here: the dataset readers, mixed_precision.
"""
import torch
import torch.nn.functional as F

from . import io_formats, ops
from ._lib import MpiFlowHipError


class InputPadder:
    """Pads images such that dimensions are divisible by 8 (upstream's class).  dims: a shape whose last two entries are H, W; mode 'sintel'
    splits both pads, any other mode (upstream passes 'kitti') puts the whole height pad at the bottom."""

    def __init__(self, dims, mode="sintel"):
        self.ht, self.wd = dims[-2:]
        pad_ht = (((self.ht // 8) + 1) * 8 - self.ht) % 8
        pad_wd = (((self.wd // 8) + 1) * 8 - self.wd) % 8
        if mode == "sintel":
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, pad_ht // 2, pad_ht - pad_ht // 2]
        else:
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, 0, pad_ht]

    def pad(self, *inputs):
        return [F.pad(x, self._pad, mode="replicate") for x in inputs]

    def unpad(self, x):
        ht, wd = x.shape[-2:]
        c = [self._pad[2], ht - self._pad[3], self._pad[0], wd - self._pad[1]]
        return x[..., c[0]:c[1], c[2]:c[3]]

    def pair(self, image1, image2):
        """image1, image2 [N,3,H,W] float32 in 0..255 on the GPU -> [2N,3,Hp,Wp]: 2 * (x / 255) - 1 of both padded images, image1 first, without
        the padded images (ops.raft_images_padded).  The tensors are taken as they are or refused (MpiFlowHipError)."""
        if isinstance(image1, torch.Tensor) and image1.dim() == 4 and tuple(image1.shape[-2:]) != (self.ht, self.wd):
            raise MpiFlowHipError("InputPadder.pair: the padder was made for %d x %d frames (got image1 of shape %s)" % (self.ht, self.wd, tuple(image1.shape)))
        return ops.raft_images_padded(image1, image2, self._pad)


class FlowMetrics:
    """The accumulators of evaluate.py's validation loops, kept on the device.  update() per batch; result(kind) once at the end."""

    def __init__(self):
        self._acc = []                                       # per update a float64 device tensor [N,6]

    def update(self, flow_pr, flow_gt, valid=None):
        """flow_pr, flow_gt [N,2,H,W], valid [N,H,W] or None, float32 on the GPU; frames of different sizes may be mixed across updates"""
        self._acc.append(ops.flow_metrics(flow_pr, flow_gt, valid))

    def result(self, kind="sintel"):
        """kind 'sintel' (also chairs): {'epe', '1px', '3px', '5px'} over all counted pixels of all frames, np.mean(np.concatenate(epe_list)) and
        its companions.  kind 'kitti': {'kitti-epe': the mean over frames of each frame's mean epe over its valid pixels, 'kitti-f1': 100 *
        outliers / valid pixels over all frames} (validate_kitti).  A frame without a counted pixel has the mean nan, as upstream's empty
        .mean().  Python floats; one device-to-host copy."""
        if kind not in ("sintel", "kitti"):
            raise MpiFlowHipError("FlowMetrics.result: kind must be 'sintel' or 'kitti' (got %r)" % (kind,))
        if not self._acc:
            raise MpiFlowHipError("FlowMetrics.result: no frame has been added (call update first)")
        devices = {a.device for a in self._acc}
        if len(devices) > 1:
            raise MpiFlowHipError("FlowMetrics.result: the updates ran on %d devices; keep one FlowMetrics per device" % len(devices))
        rows = torch.cat(self._acc, dim=0).cpu().tolist()
        ratio = lambda num, den: num / den if den else float("nan")
        total = [sum(r[q] for r in rows) for q in range(6)]
        if kind == "sintel":
            return {"epe": ratio(total[0], total[1]), "1px": ratio(total[2], total[1]), "3px": ratio(total[3], total[1]), "5px": ratio(total[4], total[1])}
        return {"kitti-epe": sum(ratio(r[0], r[1]) for r in rows) / len(rows), "kitti-f1": 100.0 * ratio(total[5], total[1])}


def forward_interpolate(flow):
    """upstream's utils.forward_interpolate: flow [2,h,w] -> [2,h,w] (also [N,2,h,w] -> [N,2,h,w], samples independent): every pixel takes the
    flow vector of the nearest pixel pushed forward along its own flow (ops.forward_interpolate has the exact rule).  float32 on the GPU; the
    result STAYS on the device (upstream returns a CPU tensor and calls .cuda() on it).  A flow without a valid source gives zeros, not NaN."""
    if isinstance(flow, torch.Tensor) and flow.dim() == 3:
        return ops.forward_interpolate(flow[None])[0]
    return ops.forward_interpolate(flow)


def flow_to_image(flow, image=None, clip_flow=None, convert_to_bgr=False):
    """upstream's flow_viz.flow_to_image on the device (ops.flow_to_image has the arithmetic): flow [N,2,H,W] (what RAFT.predict returns) ->
    uint8 [N,H,W,3], every image normalised by its own largest vector, as upstream, which is called per image; or upstream's own layout, one
    [H,W,2] tensor -> [H,W,3] (re-laid as [1,2,H,W] by a device copy).  image [N,3,H,W] ([3,H,W] beside an [H,W,2] flow) in 0..255: demo.py's
    stack, uint8 [N,2H,W,3] with the frame on top.  float32 on the GPU; the result stays there."""
    if isinstance(flow, torch.Tensor) and flow.dim() == 3:
        if flow.shape[2] != 2:
            raise MpiFlowHipError("flow_to_image: flow must be [N,2,H,W] or [H,W,2] (got shape %s)" % (tuple(flow.shape),))
        if isinstance(image, torch.Tensor) and image.dim() == 3:
            image = image[None]
        return ops.flow_to_image(flow.permute(2, 0, 1).contiguous()[None], image, clip_flow, convert_to_bgr)[0]
    return ops.flow_to_image(flow, image, clip_flow, convert_to_bgr)


def _single(t, name, who, rank):
    """one sample of a batch argument, for the writers of one file: [1, ...] or its unbatched form -> the batched form"""
    if isinstance(t, torch.Tensor) and t.dim() == rank - 1:
        return t[None]
    if isinstance(t, torch.Tensor) and t.dim() == rank and t.shape[0] != 1:
        raise MpiFlowHipError("%s: one file holds one image: %s must be a single sample (got shape %s)" % (who, name, tuple(t.shape)))
    return t


def save_flow_image(path, flow, image=None):
    """demo.py's picture as an 8-bit PNG: the colour-coded flow [2,H,W] (or [1,2,H,W]), under the frame [3,H,W] if one is given.  Colours and
    PNG row filter on the device (ops.flow_to_image, ops.png_scanlines); the host deflates 3 bytes per pixel.  Synchronises: it writes a file."""
    who = "save_flow_image"
    bgr = ops.flow_to_image(_single(flow, "flow", who, 4), None if image is None else _single(image, "image", who, 4), convert_to_bgr=True)
    io_formats.write_bytes(path, io_formats.png_from_scanlines(ops.png_scanlines(bgr[0]).cpu().numpy()))


def write_flow_kitti(path, flow, valid=None):
    """frame_utils.writeFlowKITTI without OpenCV: flow [2,H,W] (or [1,2,H,W]), valid [H,W] or None (all ones, as upstream) -> KITTI's 16-bit RGB
    PNG, R = 64 * u + 2^15, G = 64 * v + 2^15, B = valid, encoded on the device (ops.flow_encode_kitti: |flow| >= 512 px clamps).  Synchronises."""
    who = "write_flow_kitti"
    code = ops.flow_encode_kitti(_single(flow, "flow", who, 4), None if valid is None else _single(valid, "valid", who, 3))
    io_formats.write_bytes(path, io_formats.png16_from_rgb(code[0].cpu().numpy()))


def read_flow_kitti(path):
    """frame_utils.readFlowKITTI without OpenCV: -> (flow [H,W,2] float32 = (code - 2^15) / 64, valid [H,W] float32), numpy arrays on the host"""
    code = io_formats.read_png_rgb(path)
    if code.dtype != "uint16":
        raise MpiFlowHipError("read_flow_kitti: %s is no 16-bit PNG" % (path,))
    code = code.astype("float32")
    return (code[:, :, :2] - 2 ** 15) / 64.0, code[:, :, 2]


def predict_sequence(model, frames, iters=32, mode="sintel", warm_start=True):
    """create_sintel_submission's loop over one video: `frames` an iterable of [N,3,H,W] batches; yields (flow_low, flow_up) of
    model.predict(frames[t], frames[t+1], iters, mode=mode, warm_start=prev) per consecutive pair, prev the previous pair's flow_low (None for
    the first pair, and always with warm_start=False).  Nothing but prev is kept; no host copy."""
    prev = last = None
    for frame in frames:
        if last is not None:
            flow_low, flow_up = model.predict(last, frame, iters=iters, mode=mode, warm_start=prev)
            prev = flow_low if warm_start else None
            yield flow_low, flow_up
        last = frame
