"""The one contract of every tensor the RAFT modules hand to a kernel (ops' RAFT half, raft_corr, raft_upsample, raft_update, raft_extractor):
a tensor is taken as it is - float32, the expected shape, contiguous, on the GPU, all tensors of a call on one device - or MpiFlowHipError.
Nothing is copied, cast or moved.  The C ABI sees bare pointers: these checks are what ties a tensor's real size to what a kernel indexes.

The order is fixed: per tensor its type, dtype, shape, contiguity (check_tensor); then whatever the call itself requires;
the device LAST (check_devices, once per call), so that every other fault is named as such wherever the tensors live.
"""
import torch

from ._lib import CORR_MAX_LEVELS, MpiFlowHipError


def check_tensor(t, name, who, shape, layout=None, dtypes=None):
    """`shape`: a tuple whose None entries are free, or just a rank; `layout`: a word for the message, such as "[N,C,H,W]"; `dtypes`: the
    dtypes a call with kernels for several takes (default: float32 alone).  Returns t itself."""
    if not isinstance(t, torch.Tensor):
        raise MpiFlowHipError("%s: %s must be a torch.Tensor (got %s)" % (who, name, type(t).__name__))
    if dtypes is not None:
        if t.dtype not in dtypes:
            raise MpiFlowHipError("%s: %s must be %s (got %s)" % (who, name, " or ".join(str(d).replace("torch.", "") for d in dtypes), t.dtype))
    elif t.dtype != torch.float32:
        raise MpiFlowHipError("%s: %s must be float32 (got %s); call .float() on it (the kernels are float32 only)" % (who, name, t.dtype))
    rank, shape = (shape, ()) if isinstance(shape, int) else (len(shape), shape)
    if t.dim() != rank or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        what = layout or (list(shape) if shape else None)
        raise MpiFlowHipError("%s: %s must be %sa contiguous tensor of %d dimensions (got shape %s)"
                              % (who, name, "%s, " % what if what else "", rank, tuple(t.shape)))
    if not t.is_contiguous():
        raise MpiFlowHipError("%s: %s must be contiguous (got shape %s with strides %s)" % (who, name, tuple(t.shape), t.stride()))
    return t


def check_devices(who, tensors):
    """`tensors`: {name: tensor}, every tensor of one call after its own checks: all on the GPU, all on the device of the first"""
    first = None
    for name, t in tensors.items():
        if not t.is_cuda:
            raise MpiFlowHipError("%s: %s must live on the GPU (got %s); mpiflow_amd has no CPU path" % (who, name, t.device))
        first = (name, t.device) if first is None else first
        if t.device != first[1]:
            raise MpiFlowHipError("%s: %s is on %s, %s on %s: the tensors of a call must share one device" % (who, name, t.device, first[0], first[1]))


def check_pyramid(who, H, W, num_levels, radius=None):
    """a correlation pyramid over an H x W frame: every level at least 2 x 2.  radius=None: a call without a lookup window.  H=None: the
    on-demand lookup, whose caller hands in the levels' own sizes (the library judges those)"""
    if not 1 <= int(num_levels) <= CORR_MAX_LEVELS:
        raise MpiFlowHipError("%s: num_levels must be 1..%d (got %s)" % (who, CORR_MAX_LEVELS, num_levels))
    if radius is not None and not 1 <= int(radius) <= 8:
        raise MpiFlowHipError("%s: radius must be 1..8 (got %s)" % (who, radius))
    if H is not None and min(H, W) < 2 ** int(num_levels):
        raise MpiFlowHipError("%s: H, W = %d, %d must be at least 2^num_levels = %d (every level at least 2 x 2)" % (who, H, W, 2 ** int(num_levels)))
