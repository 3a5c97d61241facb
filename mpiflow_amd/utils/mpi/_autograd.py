"""Autograd for the utils/mpi renderer: three torch.autograd.Functions over the HIP backward kernels (mpf_render_bwd.hip).

Gradients flow to the per-plane VALUES only - colour, density, the "extra" channels (flow, object mask) and the sampler's source tensor.  Geometry is
constant: an xyz tensor, a disparity, a pose or an intrinsic matrix that requires grad while grad mode is on is refused with MpiFlowHipError naming the
argument (refuse_geometry), and so are is_bg_depth_inf=True, anything but float32 on one GPU (check_values) and double backward (once_differentiable).

mpi_rendering.py / homography_sampler.py come here only when wants_grad() says that an eligible input requires grad; otherwise they take the code path
they always took.  Each Function's forward IS that path - the same ops calls with the same arguments - so the values are the same bits.

The two sampling adjoints (homography_sample_backward, warp_composite_split_backward) scatter with float atomic adds: the order in which the adds arrive
decides the last bits of each gradient, so two runs of one backward may differ there.  A deterministic gather form is not provided."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ... import _lib, host_math, ops


def wants_grad(*tensors):
    """True when grad mode is on and one of the tensors (None entries allowed) requires grad."""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def refuse_geometry(who, **named):
    """Geometry is constant here: raise if grad mode is on and one of the named tensors requires grad."""
    if not torch.is_grad_enabled():
        return
    for name, t in named.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise _lib.MpiFlowHipError("%s: %s requires grad, but the HIP renderer is differentiable with respect to the plane colours, densities and extra "
                                       "values only - geometry (xyz, disparities, poses, intrinsics) is constant; detach %s" % (who, name, name))


def check_values(who, **named):
    """The differentiable path is float32 on one GPU: every named value tensor (None allowed) must be a float32 CUDA tensor, all on one device."""
    dev = None
    for name, t in named.items():
        if t is None:
            continue
        if not t.is_cuda or t.dtype != torch.float32:
            raise _lib.MpiFlowHipError("%s: gradients are provided for float32 tensors on one GPU only; %s is %s on %s" % (who, name, t.dtype, t.device))
        if dev is not None and t.device != dev:
            raise _lib.MpiFlowHipError("%s: gradients are provided on one GPU only; %s lives on %s, another argument on %s" % (who, name, t.device, dev))
        dev = t.device


def refuse_bg_depth_inf(who, is_bg_depth_inf):
    if is_bg_depth_inf:
        raise _lib.MpiFlowHipError("%s: is_bg_depth_inf=True is not differentiable here (only the normalised depth has a backward kernel); "
                                   "run it under torch.no_grad() or with is_bg_depth_inf=False" % who)


class HomographySampleFn(Function):
    """ops.homography_sample with the gradient of src_BCHW.  ranges: the channel ranges [(c0, c1), ...] whose gradient is wanted (None: all) -
    render_tgt_rgb_depth's concatenation carries constant xyz channels in the middle.  valid and flowB2A carry no gradient."""

    @staticmethod
    def forward(ctx, src_BCHW, H_src_tgt, ranges):
        ctx.H_src_tgt = H_src_tgt
        ctx.ranges = ranges if ranges is not None else [(0, src_BCHW.size(1))]
        tgt, valid, flow = ops.homography_sample(src_BCHW, H_src_tgt)
        ctx.mark_non_differentiable(valid, flow)
        return tgt, valid, flow

    @staticmethod
    @once_differentiable
    def backward(ctx, g_tgt, _g_valid, _g_flow):
        grad_src = None
        for c0, c1 in ctx.ranges:
            grad_src = ops.homography_sample_backward(g_tgt, ctx.H_src_tgt, c0, c1, grad_src=grad_src)
        return grad_src, None, None


class VolumeRenderFn(Function):
    """ops.volume_render for one batch item with the gradients of rgb, sigma and the extras; all five outputs are connected.
    -> (rgb | None, depth, tacc | None, weights | None, extra | None)"""

    @staticmethod
    def forward(ctx, rgb_S3N, sigma_SN, xyz_S3N, extra_SEN, hard, want_tacc, want_weights):
        r = ops.volume_render(rgb_S3N, sigma_SN, xyz_S3N, extra_SEN=extra_SEN, hard=hard, want_tacc=want_tacc, want_weights=want_weights)
        ctx.save_for_backward(rgb_S3N, sigma_SN, xyz_S3N, extra_SEN)
        ctx.hard = bool(hard)
        ctx.set_materialize_grads(False)
        return r["rgb"], r["depth"], r["tacc"], r["weights"], r["extra"]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_rgb, g_depth, g_tacc, g_weights, g_extra):
        rgb, sigma, xyz, extra = ctx.saved_tensors
        if ctx.hard:                       # the flow form: only the extras' gradient exists (depth, tacc and weights are not handed out there)
            g_depth = g_tacc = g_weights = None
        g = ops.volume_render_backward(rgb, sigma, xyz, extra, hard=ctx.hard, g_rgb=g_rgb, g_depth=g_depth, g_extra=g_extra, g_weights=g_weights,
                                       g_tacc=g_tacc, want_rgb=rgb is not None and ctx.needs_input_grad[0],
                                       want_extra=extra is not None and ctx.needs_input_grad[3])
        return (g["rgb"].reshape(rgb.shape) if g["rgb"] is not None else None, g["sigma"].reshape(sigma.shape), None,
                g["extra"].reshape(extra.shape) if g["extra"] is not None else None, None, None, None)


def volume_render(rgb_S3N, sigma_SN, xyz_S3N, extra_SEN=None, hard=False, want_tacc=True, want_weights=True):
    """ops.volume_render's dict, differentiable."""
    rgb, depth, tacc, weights, extra = VolumeRenderFn.apply(rgb_S3N, sigma_SN, xyz_S3N, extra_SEN, hard, want_tacc, want_weights)
    return dict(rgb=rgb, depth=depth, tacc=tacc, weights=weights, extra=extra)


class WarpCompositeFn(Function):
    """The fused standard call of render_tgt_rgb_depth (mpf_warp_composite_split per batch item) with the gradients of the rgb and sigma stacks
    (mpf_warp_composite_bwd): no [S,C,H,W] intermediate in either direction.  obj_mask is a constant here; tgt_mask carries no gradient.
    -> (rgb Bx3xHxW, depth Bx1xHxW, tgt_mask Bx1xHxW, objmask Bx1xHxW | None)"""

    @staticmethod
    def forward(ctx, mpi_rgb_src, mpi_sigma_src, mpi_disparity_src, G_tgt_src, K_src_inv, K_tgt, obj_mask):
        B, S, _, H, W = mpi_rgb_src.size()
        dev = mpi_rgb_src.device
        rgbs, depths, tms, oms, ctx.quads, ctx.dparams = [], [], [], [], [], []
        for b in range(B):
            d = host_math.plane_depths(mpi_disparity_src[b])
            _, H_st = host_math.homographies(G_tgt_src[b], K_src_inv[b], K_tgt[b], d)
            quads = ops.mask_quads(obj_mask[b, 0, 0].to(dev, torch.float32).contiguous(), False) if obj_mask is not None else None
            dparams = ops.upload_params(ops.warp_params(H_st, K_src_inv[b], G_tgt_src[b], d), dev)
            v = ops.warp_composite_split(mpi_rgb_src[b], mpi_sigma_src[b], quads, dparams=dparams)
            rgbs.append(v["rgb"]); depths.append(v["depth"].reshape(1, H, W)); tms.append(v["tgt_mask"].reshape(1, H, W))
            if obj_mask is not None:
                oms.append(v["objmask"].reshape(1, H, W))
            ctx.quads.append(quads); ctx.dparams.append(dparams)
        ctx.save_for_backward(mpi_rgb_src, mpi_sigma_src)
        ctx.set_materialize_grads(False)
        tgt_mask = torch.stack(tms)
        ctx.mark_non_differentiable(tgt_mask)
        return torch.stack(rgbs), torch.stack(depths), tgt_mask, (torch.stack(oms) if oms else None)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_rgb, g_depth, _g_tgt_mask, g_om):
        mpi_rgb_src, mpi_sigma_src = ctx.saved_tensors
        B, S, _, H, W = mpi_rgb_src.size()
        grad_rgb = torch.zeros_like(mpi_rgb_src, memory_format=torch.contiguous_format)
        grad_sigma = torch.zeros_like(mpi_sigma_src, memory_format=torch.contiguous_format)
        if g_rgb is None:
            g_rgb = torch.zeros((B, 3, H, W), dtype=torch.float32, device=mpi_rgb_src.device)
        for b in range(B):
            ops.warp_composite_split_backward(mpi_rgb_src[b], mpi_sigma_src[b], ctx.quads[b], ctx.dparams[b], g_rgb[b],
                                              g_depth[b] if g_depth is not None else None,
                                              g_om[b] if (g_om is not None and ctx.quads[b] is not None) else None,
                                              grad_rgb=grad_rgb[b], grad_sigma=grad_sigma[b].view(S, H, W))
        return grad_rgb, grad_sigma, None, None, None, None, None
