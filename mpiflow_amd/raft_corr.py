"""RAFT's two correlation blocks on the GPU.  CorrBlock (the class of that name below): the all-pairs default of RAFT/core/corr.py, its
per-iteration work fused in HIP.  The rest of this module is RAFT's on-demand correlation lookup: a drop-in for RAFT/core/corr.py's AlternateCorrBlock and for the `alt_cuda_corr`
extension it calls (RAFT/alt_cuda_corr), which has no ROCm build.

Two ways in:

    from mpiflow_amd.raft_corr import AlternateCorrBlock            # corr_fn = AlternateCorrBlock(fmap1, fmap2, radius=r); corr_fn(coords1)

    import sys, mpiflow_amd.raft_corr                               # or: leave RAFT's own corr.py as it is
    sys.modules["alt_cuda_corr"] = mpiflow_amd.raft_corr            # before `import corr`

The class holds the two feature maps channel-last (fmap1 once, fmap2 as its avg_pool2d pyramid) - nothing quadratic in H * W - and every
lookup is ONE launch of mpf_corr_lookup for all levels.  It is differentiable with respect to fmap1 and fmap2 (the kernel's gradient,
mpf_corr_lookup_backward, then torch's own backward of the permutes and of avg_pool2d); coords get NO gradient: the function returns None for
them, as RAFT detaches coords1 before every lookup (RAFT/core/raft.py:123) and upstream's backward returns zeros there.

What differs from upstream: one launch for all levels instead of one per level plus two permutes per level and lookup; gradients are wired
(upstream's AlternateCorrBlock calls the extension's forward outside autograd: it is inference-only); coordinates may hold any value - NaN,
+-inf and far-out values give exactly 0 and no gradient; levels smaller than 2 x 2 (H or W < 2^num_levels) are refused, where the
reference's sampler divides by zero.  Tensors are held to the contract of _tensors.py (the device is judged last): nothing
runs on the CPU and there is no eager fallback: MpiFlowHipError.
"""
import torch
import torch.nn.functional as F

from . import ops
from ._lib import MpiFlowHipError
from ._tensors import check_devices, check_pyramid, check_tensor


class _CorrLookup(torch.autograd.Function):
    """out = corr_lookup(fmap1_nhwc, levels, coords); gradients for fmap1_nhwc and every level, None for coords and radius."""

    @staticmethod
    def forward(ctx, coords, radius, fmap1_nhwc, *levels):
        ctx.radius = radius
        ctx.save_for_backward(coords, fmap1_nhwc, *levels)
        return ops.corr_lookup(fmap1_nhwc, levels, coords, radius)

    @staticmethod
    def backward(ctx, grad_out):
        coords, fmap1_nhwc, *levels = ctx.saved_tensors
        g1, g2 = ops.corr_lookup_backward(fmap1_nhwc, levels, coords, grad_out.contiguous(), ctx.radius)
        return (None, None, g1) + tuple(g2)


def _check_maps(who, fmap1, fmap2, num_levels, radius):
    """what both blocks ask of their maps (the contract of _tensors), except the device, which the block judges last: -> (B, C, H, W)"""
    for t, name in ((fmap1, "fmap1"), (fmap2, "fmap2")):
        check_tensor(t, name, who, 4, "[B,C,H,W]")
    if fmap1.shape != fmap2.shape:
        raise MpiFlowHipError("%s: fmap1 %s and fmap2 %s must agree" % (who, tuple(fmap1.shape), tuple(fmap2.shape)))
    check_pyramid(who, fmap1.shape[2], fmap1.shape[3], num_levels, radius)
    return fmap1.shape


class AlternateCorrBlock:
    """RAFT/core/corr.py's AlternateCorrBlock: AlternateCorrBlock(fmap1, fmap2, num_levels=4, radius=4)(coords) -> [B, L*(2r+1)^2, H, W],
    CorrBlock's result (same channel order: the first window index moves x) without the all-pairs volume.  fmap1, fmap2 [B,C,H,W] float32,
    contiguous, on the GPU, C a multiple of 32, H and W at least 2^num_levels; coords [B,2,H,W] (x, y), any values.  Usable as `corr_fn` in
    RAFT/core/raft.py:104-107 unchanged.  No gradient flows to coords (None)."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        B, C, H, W = _check_maps("AlternateCorrBlock", fmap1, fmap2, num_levels, radius)
        if C < 32 or C % 32:
            raise MpiFlowHipError("AlternateCorrBlock: C must be a multiple of 32 (got %d)" % C)
        check_devices("AlternateCorrBlock", dict(fmap1=fmap1, fmap2=fmap2))
        self.num_levels, self.radius = int(num_levels), int(radius)
        # the layout change happens here, once per pair, not per lookup; autograd carries the levels' gradients back through avg_pool2d
        self.fmap1_nhwc = fmap1.permute(0, 2, 3, 1).contiguous()
        self.f2_levels_nhwc = []
        for i in range(self.num_levels):
            if i:
                fmap2 = F.avg_pool2d(fmap2, 2, stride=2)
            self.f2_levels_nhwc.append(fmap2.permute(0, 2, 3, 1).contiguous())

    def __call__(self, coords):
        return _CorrLookup.apply(coords, self.radius, self.fmap1_nhwc, *self.f2_levels_nhwc)


class _GradPyramid:
    """What the autograd nodes of one CorrBlock share: the gradient pyramid every lookup's backward adds into.  Allocated and zeroed at the
    first backward call of a lookup, handed over (and forgotten) when the pyramid's own backward folds it."""

    def __init__(self):
        self.levels = None


class _CorrPyramid(torch.autograd.Function):
    """(fmap1, fmap2) -> the levels of the all-pairs pyramid.  Its cotangents do not arrive as arguments (the lookups return None for the
    levels) but in `shared`, complete when autograd runs this node: a node runs after every node that depends on it has run."""

    @staticmethod
    def forward(ctx, shared, num_levels, fmap1, fmap2):
        B, C, H, W = fmap1.shape
        ctx.shared, ctx.norm = shared, float(torch.sqrt(torch.tensor(C).float()))          # RAFT divides by the fp32 sqrt(C)
        ctx.save_for_backward(fmap1, fmap2)
        ctx.set_materialize_grads(False)
        raw = torch.matmul(fmap1.view(B, C, H * W).transpose(1, 2), fmap2.view(B, C, H * W))
        levels = ops.corr_pyramid(raw.view(B * H * W, H, W), num_levels, ctx.norm)        # level 0 is raw itself, scaled in place
        return tuple(t.unsqueeze(1) for t in levels)

    @staticmethod
    def backward(ctx, *unused):
        grad, ctx.shared.levels = ctx.shared.levels, None
        if grad is None:                                         # no lookup of this block reached the loss
            return None, None, None, None
        fmap1, fmap2 = ctx.saved_tensors
        B, C, H, W = fmap1.shape
        g = ops.corr_pyramid_backward(grad, ctx.norm).view(B, H * W, H * W)
        del grad
        g1 = torch.matmul(fmap2.view(B, C, H * W), g.transpose(1, 2)).view(B, C, H, W) if ctx.needs_input_grad[2] else None
        g2 = torch.matmul(fmap1.view(B, C, H * W), g).view(B, C, H, W) if ctx.needs_input_grad[3] else None
        return None, None, g1, g2


class _CorrVolumeLookup(torch.autograd.Function):
    """out = corr_volume_lookup(levels, coords).  Its backward adds into the block's shared gradient pyramid and returns None for every input."""

    @staticmethod
    def forward(ctx, shared, radius, coords, *levels):
        ctx.shared, ctx.radius, ctx.shapes = shared, radius, [t.shape for t in levels]
        ctx.save_for_backward(coords)
        return ops.corr_volume_lookup([t.squeeze(1) for t in levels], coords, radius)

    @staticmethod
    def backward(ctx, grad_out):
        coords, = ctx.saved_tensors
        if ctx.shared.levels is None:
            ctx.shared.levels = [torch.zeros((s[0], s[2], s[3]), dtype=torch.float32, device=coords.device) for s in ctx.shapes]
        ops.corr_volume_lookup_backward(ctx.shared.levels, coords, grad_out.contiguous(), ctx.radius)
        return (None,) * (3 + len(ctx.shapes))


class CorrBlock:
    """RAFT/core/corr.py's CorrBlock: CorrBlock(fmap1, fmap2, num_levels=4, radius=4)(coords) -> [B, L*(2r+1)^2, H, W], the reference's values
    and channel order (the first window index moves x).  fmap1, fmap2 [B,C,H,W] float32, contiguous, on the GPU, H and W at least
    2^num_levels; coords [B,2,H,W] (x, y), any values: NaN, +-inf and far-out ones give exactly 0.  Usable as `corr_fn` in
    RAFT/core/raft.py:104-107 unchanged.  `corr_pyramid` is upstream's list of [B*H*W, 1, H_l, W_l] tensors.

    Construction is one torch.matmul and one launch (mpf_corr_pyramid: 1/sqrt(C) applied to the product in place, the other levels written in
    the same pass); a lookup is one launch for all levels (mpf_corr_volume_lookup).  Differentiable with respect to fmap1 and fmap2; coords get
    no gradient (None), as in AlternateCorrBlock.  The backward pass of every lookup ADDS into one gradient pyramid owned by the block
    (mpf_corr_volume_lookup_backward: no atomics, nothing zero-filled per lookup), allocated and zeroed at the first such call; the node that
    produced the pyramid runs last, folds it (mpf_corr_pyramid_backward), does the two GEMMs and releases it.  Every kernel result is
    bit-identical from run to run.  Under torch.no_grad(), or when neither map requires a gradient, none of this is allocated.  A lookup's
    backward needs the coordinates and the levels' shapes, not the pyramid: a block dropped before backward() (RAFT.forward's on return) frees it.

    Not supported: torch.autograd.grad with respect to `corr_pyramid` itself (its levels receive no cotangent: the gradient travels in the
    shared buffer), double backward, and backward passes of two lookups of ONE block running at the same time on different streams (they add
    into the same buffer).  A backward pass that reaches some lookups but not fmap1 / fmap2 leaves the buffer allocated until the block dies."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        _check_maps("CorrBlock", fmap1, fmap2, num_levels, radius)
        check_devices("CorrBlock", dict(fmap1=fmap1, fmap2=fmap2))
        self.num_levels, self.radius = int(num_levels), int(radius)
        self._shared = _GradPyramid()
        self.corr_pyramid = list(_CorrPyramid.apply(self._shared, self.num_levels, fmap1, fmap2))

    def __call__(self, coords):
        return _CorrVolumeLookup.apply(self._shared, self.radius, coords, *self.corr_pyramid)


def _ext_coords(coords, fmap1):
    if not isinstance(coords, torch.Tensor) or coords.dim() != 5 or coords.shape[-1] != 2 or tuple(coords.shape[2:4]) != tuple(fmap1.shape[1:3]):
        raise MpiFlowHipError("alt_cuda_corr: coords must be [B,N,H,W,2] for fmap1 [B,H,W,C] (got %s)"
                              % (tuple(coords.shape) if isinstance(coords, torch.Tensor) else type(coords).__name__,))
    return [coords[:, n].permute(0, 3, 1, 2).contiguous() for n in range(coords.shape[1])]


def forward(fmap1, fmap2, coords, r):
    """alt_cuda_corr.forward (RAFT/alt_cuda_corr/correlation.cpp:51-54): fmap1 [B,H,W,C], fmap2 [B,H2,W2,C] (one pyramid level, channel-last),
    coords [B,N,H,W,2] in pixels of fmap2 -> [corr [B,N,(2r+1)^2,H,W]], NOT scaled by 1/sqrt(C)."""
    return [torch.stack([ops.corr_lookup(fmap1, [fmap2], c, r, scale=1.0) for c in _ext_coords(coords, fmap1)], dim=1)]


def backward(fmap1, fmap2, coords, corr_grad, r):
    """alt_cuda_corr.backward: -> [fmap1_grad [B,H,W,C], fmap2_grad [B,H2,W2,C], coords_grad [B,N,H,W,2] (zeros, as upstream)]."""
    g1, g2 = None, None
    for n, c in enumerate(_ext_coords(coords, fmap1)):
        a, b = ops.corr_lookup_backward(fmap1, [fmap2], c, corr_grad[:, n].contiguous(), r, scale=1.0)
        g1, g2 = (a, b[0]) if g1 is None else (g1 + a, g2 + b[0])
    return [g1, g2, torch.zeros_like(coords)]
