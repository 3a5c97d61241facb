"""Drop-in for the reference's bilateral_filter.py (3d-photo-inpainting's bilateral_filtering.py) on MI355X: sparse_bilateral_filtering,
vis_depth_discontinuity and bilateral_filter under the reference's signatures.

The reference's body is a Python loop over every pixel with an argsort and a cumsum each; here an iteration is two HIP launches
(ops.sparse_bilateral_filter, mpf_bilateral.hip) and the result is the reference's bit for bit.  A numpy array
in gives a numpy array of the same dtype out, by upload and download; a GPU tensor in gives a tensor out.  There is no CPU path.

Not supported, and refused: vis_depth_discontinuity(label=True), and bilateral_filter without a discontinuity map - the range-weighted
branch, which sparse_bilateral_filtering never reaches and whose exp weights cannot be pinned bit for bit."""
import numpy as np
import torch

from . import ops
from ._lib import MpiFlowHipError

__all__ = ["sparse_bilateral_filtering"]


def _device():
    if not torch.cuda.is_available():
        raise MpiFlowHipError("bilateral_filter: a numpy array needs a GPU to be filtered on; mpiflow_amd has no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _up(a, name):
    """numpy or tensor -> (GPU tensor, was numpy)"""
    if isinstance(a, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(a)).to(_device()), True
    if isinstance(a, torch.Tensor):
        return a, False
    raise MpiFlowHipError("bilateral_filter: %s must be a numpy array or a torch.Tensor (got %s)" % (name, type(a).__name__))


def _mask(mask, like):
    if mask is None:
        return None
    m, _ = _up(mask, "mask")
    if m.dtype not in (torch.bool, torch.uint8, torch.float32):       # the reference multiplies by it: any numeric array of 0 / 1
        m = m != 0
    return m.to(like.device)


def sparse_bilateral_filtering(depth, filter_size, sigma_r=0.5, sigma_s=4.0, depth_threshold=0.04, HR=False, mask=None, gsHR=True,
                               edge_id=None, num_iter=None, num_gs_iter=None):
    """The reference's sparse_bilateral_filtering (bilateral_filter.py:13-53): depth [h,w] float32, float64 or uint8 (value u / 255.0) ->
    the filtered depth, same type.  sigma_r, sigma_s, HR, gsHR, edge_id and num_gs_iter are accepted and ignored, as the reference never
    reads them on this path.  num_iter=None: len(filter_size) (the reference raises there)."""
    d, was_numpy = _up(depth, "depth")
    out = ops.sparse_bilateral_filter(d, filter_size, depth_threshold=depth_threshold, mask=_mask(mask, d), num_iter=num_iter)
    return out.cpu().numpy() if was_numpy else out


def vis_depth_discontinuity(depth, depth_threshold, vis_diff=False, label=False, mask=None):
    """The reference's vis_depth_discontinuity (:56-109) with label=False: [u_over, b_over, l_over, r_over], float32 0 / 1 maps of the four
    differences of 1 / depth that exceed depth_threshold, the border ring 0 (and with vis_diff the four differences as well).  A few
    elementwise operations in depth's own dtype, on the array's own side: numpy on the host, torch on the GPU; the filter does not call it
    (its map is mpf_bilateral.hip's k_bil_map)."""
    if label:
        raise MpiFlowHipError("vis_depth_discontinuity: label=True (the label-map branch) is not supported (got label=%r)" % (label,))
    if isinstance(depth, np.ndarray):
        xp_abs, pad = np.abs, lambda a: np.pad(a, 1, mode="constant")
        over = lambda a: (xp_abs(a) > depth_threshold).astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            disp = 1.0 / depth
    elif isinstance(depth, torch.Tensor):
        xp_abs, pad = torch.abs, lambda a: torch.nn.functional.pad(a, (1, 1, 1, 1))
        over = lambda a: (xp_abs(a) > depth_threshold).float()
        disp = 1.0 / depth
    else:
        raise MpiFlowHipError("vis_depth_discontinuity: depth must be a numpy array or a torch.Tensor (got %s)" % type(depth).__name__)
    inner = (slice(1, -1), slice(1, -1))
    around = ((slice(0, -2), slice(1, -1)), (slice(2, None), slice(1, -1)), (slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None)))   # up, below, left, right
    diffs = [disp[inner] - disp[nb] for nb in around]                  # an interior pixel minus its neighbour
    if mask is not None:
        diffs = [d * (mask[inner] * mask[nb]) for d, nb in zip(diffs, around)]
    overs = [pad(over(d)) for d in diffs]
    return (overs, [pad(d) for d in diffs]) if vis_diff else overs


def bilateral_filter(depth, sigma_s, sigma_r, window_size, discontinuity_map=None, HR=False, mask=None):
    """The reference's bilateral_filter (:112-228).  Only what sparse_bilateral_filtering reaches is a product here, and that is reached
    through sparse_bilateral_filtering, which forms the map itself; a map handed in would have to be trusted instead of computed, and without
    one the reference takes its range-weighted branch (exp weights, not a selection pinned bit for bit).  Both are refused."""
    if discontinuity_map is None:
        raise MpiFlowHipError("bilateral_filter: discontinuity_map=None selects the range-weighted branch, which is not supported; "
                              "call sparse_bilateral_filtering(depth, filter_size=[%r], num_iter=1)" % (window_size,))
    raise MpiFlowHipError("bilateral_filter: a caller-supplied discontinuity_map is not supported (the kernel computes the map of its own "
                          "input); call sparse_bilateral_filtering(depth, filter_size=[%r], num_iter=1)" % (window_size,))
