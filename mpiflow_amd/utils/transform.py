"""Drop-in for the reference's utils/transform.py: the backward warps by a flow field, warp(x, flo) and warp_rife(tenInput, tenFlow), as one HIP
pass each way (mpf_flow_warp.hip), and its numpy helpers gen_random_perspective / get_flow as they stand there.

warp        (output, mask) = x sampled at (x + u, y + v), bilinear, zero padding.  The reference normalises the coordinate for align_corners=True
            and samples with grid_sample's default align_corners=False; that is its behaviour and it is reproduced:
            ix = ((2 (x + u) / max(W - 1, 1) - 1 + 1) W - 1) / 2.  Differentiable with respect to x and flo.
warp_rife   tenInput sampled at lin_W[x] + u / ((W - 1) / 2), align_corners=True, border padding; differentiable with respect to both arguments.
            The linspace grids are made by torch once per (device, size) and kept (ops.flow_warp_linspace), as the reference keeps them.

A pixel's four taps are built once and used for every channel and for the mask.  The gradient of the image is a float-atomic scatter (the order of
the adds decides its last bits); the gradient of the flow is one store per pixel, atomic-free and identical on every run.  Both functions are
once-differentiable (double backward raises).  float32 tensors of one GPU, [B,C,H,W] and [B,2,H,W]; a non-contiguous tensor is made contiguous;
half, double, CPU tensors and mismatched shapes raise MpiFlowHipError before anything is launched.

transform(img, flow) is cv2.remap on uint8, whose fixed-point interpolation cannot be pinned without an OpenCV: it raises NotImplementedError.
This module imports without cv2."""
import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib, ops


class FlowWarpFn(Function):
    """ops.flow_warp with the gradients of x (float-atomic scatter) and flow (one store per pixel) through mpf_flow_warp_bwd.  The mask is an
    output that carries no gradient."""

    @staticmethod
    def forward(ctx, x, flow, mode, want_mask):
        out, mask = ops.flow_warp(x, flow, mode, want_mask)
        ctx.save_for_backward(x, flow)
        ctx.mode = mode
        if not want_mask:
            return out
        ctx.mark_non_differentiable(mask)
        return out, mask

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        x, flow = ctx.saved_tensors
        want_x, want_flow = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gx, gf = ops.flow_warp_backward(x, flow, g.contiguous(), ctx.mode, want_x=want_x, want_flow=want_flow)
        return gx, gf, None, None


def _run(x, flow, mode, want_mask):
    if isinstance(x, torch.Tensor):
        x = x.contiguous()
    if isinstance(flow, torch.Tensor):
        flow = flow.contiguous()
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (x, flow)):
        return FlowWarpFn.apply(x, flow, mode, want_mask)
    out, mask = ops.flow_warp(x, flow, mode, want_mask)
    return (out, mask) if want_mask else out


def warp(x, flo):
    """warp an image/tensor (im2) back to im1, according to the optical flow

    x: [B, C, H, W] (im2)
    flo: [B, 2, H, W] flow

    -> (output, mask), both [B, C, H, W].  mask is the sum of the bilinear weights of the taps inside the image (1 where all four are, 0 where
    none is); it is the same in every channel, so it is computed once per pixel as [B,1,H,W] and returned as an .expand()ed view of that: reading it
    is free, an in-place write to it raises in torch (clone it first).  It never requires grad, as the reference detaches it."""
    out, mask = _run(x, flo, _lib.FLOW_WARP_WARP, True)
    return out, mask.expand(-1, out.shape[1], -1, -1)


def warp_rife(tenInput, tenFlow):
    return _run(tenInput, tenFlow, _lib.FLOW_WARP_RIFE, False)


def gen_random_perspective():
    '''
    generate a random 3x3 perspective matrix
    '''
    init_M = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]])
    noise = np.random.normal(0, 0.0001, 9)
    noise = np.reshape(noise, [3, 3])
    noise[2, 2] = 0
    return init_M + noise


def get_flow(img, M):
    '''
    use img shape and M  to calculate flow
    return flow
    '''
    x = np.linspace(0, img.shape[1] - 1, img.shape[1])
    y = np.linspace(0, img.shape[0] - 1, img.shape[0])
    xx, yy = np.meshgrid(x, y)
    coords = np.stack([xx, yy, np.ones_like(xx)], axis=0)
    new_coords = np.einsum('ij,jkl->ikl', M, coords)
    xx2 = new_coords[0, :, :] / new_coords[2, :, :]
    yy2 = new_coords[1, :, :] / new_coords[2, :, :]
    xx2 = xx2.astype(np.float32)
    yy2 = yy2.astype(np.float32)
    flow_x = xx2 - xx
    flow_y = yy2 - yy
    flow_x = flow_x.astype(np.float32)
    flow_y = flow_y.astype(np.float32)
    return np.stack([flow_x, flow_y], axis=2)


def transform(img, flow):
    '''
    remap image according to the flow (the reference: cv2.remap, INTER_LINEAR, BORDER_REFLECT_101, on uint8)
    '''
    raise NotImplementedError("transform(img, flow) is cv2.remap on uint8: its fixed-point interpolation tables cannot be pinned without an OpenCV "
                              "to record them from, so it is not provided; for float tensors use warp() or warp_rife()")
