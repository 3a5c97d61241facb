"""Drop-in for the on-path functions of the reference's utils/mpi/mpi_rendering.py - same names, argument order and
return tuples - with the per-pixel arithmetic in HIP kernels (libmpiflow_hip.so).

These are the *generic* forms: they accept and return the same materialised [B,S,C,H,W] tensors as the reference, so
each function is a drop-in on its own and reproduces the reference's semantics exactly (incl. sampling the xyz
channels rather than recomputing them).  The fused fast path that never materialises an [S,...] intermediate lives in
mpiflow_amd.pipeline / utils.utils.render_3dphoto_dynamic.

Also provided although MPI-Flow's generation never takes them: alpha_composition / use_alpha=True (:42-59),
get_xyz_from_depth (:157-177) and disparity_consistency_src_to_tgt (:180-210), the training loss of the MINE code base this module was
taken from: one fused pass (mpf_disp_consistency), differentiable with respect to both disparity maps under default grad mode
(INTEGRATION.md section 21).

Differentiable (HIP backward kernels, mpf_render_bwd.hip, behind the Functions of _autograd.py): plane_volume_rendering,
plane_volume_rendering_flow, render and render_tgt_rgb_depth, with respect to the plane colours, densities and extra values (rgb_BS3HW, sigma_BS1HW,
src_sigma_BS1HW, src_flow_BS2HW, obj_mask, mpi_rgb_src, mpi_sigma_src).  Geometry - every xyz tensor, mpi_disparity_src, G_tgt_src, K_src_inv,
K_tgt - is constant: one that requires grad while grad mode is on raises MpiFlowHipError naming it; so do is_bg_depth_inf=True with gradients,
tensors that are not float32 on one GPU, and double backward.  With no input requiring grad, or under torch.no_grad(), every function takes the
path it took before.  Forward only: alpha_composition, weighted_sum_mpi, get_xyz_from_depth.

Inside mpiflow_amd.utils.mpi.plane_geometry_grad() the geometry that a plane disparity reaches is differentiable too:
xyz_BS3HW, src_xyz_BS3HW, xyz_tgt_BS3HW, xyz_src_BS3HW and mpi_disparity_src (of render_tgt_rgb_depth: through sample_inverse's flow; of
get_src_xyz_from_plane_disparity: through the xyz field), and xyz_src_BS3HW of get_tgt_xyz_from_plane_disparity.  The sampling grid gives no gradient,
as in the reference.  G_tgt_src, K_src_inv, K_tgt, is_bg_depth_inf=True, non-float32 tensors and double backward stay refused there.
"""
import torch

from ... import _lib, host_math, ops
from . import _autograd
from .homography_sampler import HomographySample
from .rendering_utils import transform_G_xyz, sample_pdf, gather_pixel_by_pxpy  # noqa: F401  (re-exported like the reference module does)


# ---- provenance tags: which tensors are "the standard ones" ---------------------------------------------------------------------------
# render_tgt_rgb_depth receives xyz_src / xyz_tgt as materialised tensors.  When they are what get_src_xyz_from_plane_disparity /
# get_tgt_xyz_from_plane_disparity of THIS module returned for the same (K_src_inv, disparities, G_tgt_src) - the reference's only call site
# builds them exactly so (utils/utils.py:303-310) - the fused kernels, which evaluate those affine fields in registers, apply.  The tag is a
# Python attribute on the returned tensor: (what, bytes of the small host matrices it was built from, tensor version at tagging time).  A
# tensor that was modified in place, sliced, copied or built any other way carries no valid tag and takes the generic kernels.

def _key(*small):
    return tuple(host_math._cpu32(t).contiguous().numpy().tobytes() for t in small)


def _tag(t, what, key, leaf=None):
    """leaf: the disparity tensor t was built from, when it requires grad inside plane_geometry_grad() - the fused backward sends its gradient there"""
    t._mpf_std = (what, key, t._version, leaf)
    return t


def _tag_leaf(t):
    tag = getattr(t, "_mpf_std", None)
    return tag[3] if tag is not None and tag[2] == t._version else None


def _tagged(t, what):
    tag = getattr(t, "_mpf_std", None)
    return tag[1] if tag is not None and tag[0] == what and tag[2] == t._version else None


def _flat(t):                      # [B,S,C,H,W] -> per-batch [S,C,H*W] views
    B, S, C, H, W = t.shape
    return t.reshape(B, S, C, H * W)


def render(rgb_BS3HW, sigma_BS1HW, xyz_BS3HW, src_sigma_BS1HW=None, src_flow_BS2HW=None, src_xyz_BS3HW=None,
           use_alpha=False, is_bg_depth_inf=False, hard_flow=False, obj_mask=None):
    """reference utils/mpi/mpi_rendering.py:7-39 -> (imgs_syn, depth_syn, blend_weights, weights, flowA2B, obj_mask)"""
    if use_alpha:
        # The reference's use_alpha branch (:33-38) computes alpha_composition results and then fails at its return statement
        # (`flowA2B` is only bound in the other branch): same exception here.  alpha_composition() itself is provided below.
        raise UnboundLocalError("local variable 'flowA2B' referenced before assignment (reference utils/mpi/mpi_rendering.py:39, use_alpha=True)")
    imgs_syn, depth_syn, blend_weights, weights, flowB2A, obj_mask = plane_volume_rendering(
        rgb_BS3HW, sigma_BS1HW, xyz_BS3HW, src_sigma_BS1HW, src_flow_BS2HW, src_xyz_BS3HW, is_bg_depth_inf,
        hard_flow=hard_flow, obj_mask=obj_mask)
    flowA2B = None
    if src_sigma_BS1HW is not None:
        flowA2B = plane_volume_rendering_flow(src_sigma_BS1HW, src_flow_BS2HW, src_xyz_BS3HW, is_bg_depth_inf,
                                              hard_flow=hard_flow)
    return imgs_syn, depth_syn, blend_weights, weights, flowA2B, obj_mask


def alpha_composition(alpha_BK1HW, value_BKCHW):
    """reference :42-59 ("Single-View View Synthesis with Multiplane Images") -> (value_composed BxCxHxW, weights BxKx1xHxW)"""
    B, K, _, H, W = alpha_BK1HW.size()
    C = value_BKCHW.size(2)
    vals, wts = [], []
    for b in range(B):
        r = ops.alpha_composite(alpha_BK1HW[b, :, 0], value_BKCHW[b])
        vals.append(r["out"].reshape(C, H, W))
        wts.append(r["weights"].reshape(K, 1, H, W))
    return torch.stack(vals), torch.stack(wts)


def get_xyz_from_depth(meshgrid_homo, depth, K_inv):
    """xyz = (K^-1 . (x,y,1)) * depth   (reference :157-177): meshgrid 3xHxW (only its size is read), depth Bx1xHxW,
    K_inv Bx3x3 -> Bx3xHxW"""
    H, W = meshgrid_homo.size(1), meshgrid_homo.size(2)
    B, _, H_d, W_d = depth.size()
    assert H == H_d and W == W_d
    return torch.stack([ops.backproject(depth[b, 0], K_inv[b])[:3].reshape(3, H, W) for b in range(B)])


def _require_standard_meshgrid(who, meshgrid_homo, H, W):
    """meshgrid_homo must be HomographySample's 3xHxW grid of (x, y, 1) for this frame: the kernel generates the coordinates itself.  A grid on the host is
    compared there; one on the GPU by its size alone, so that nothing synchronises."""
    if not isinstance(meshgrid_homo, torch.Tensor) or tuple(meshgrid_homo.shape) != (3, H, W):
        raise _lib.MpiFlowHipError("%s: meshgrid_homo must be the standard 3xHxW grid of (x, y, 1) for the %dx%d frame of disparity_src (got %s)"
                                   % (who, H, W, tuple(meshgrid_homo.shape) if isinstance(meshgrid_homo, torch.Tensor) else type(meshgrid_homo).__name__))
    if not meshgrid_homo.is_cuda:
        std = HomographySample.grid_generation(H, W, meshgrid_homo.device).permute(2, 0, 1)
        if not torch.equal(meshgrid_homo.to(torch.float32), std):
            raise _lib.MpiFlowHipError("%s: meshgrid_homo must be the standard grid of (x, y, 1), x = 0..W-1, y = 0..H-1 (HomographySample(H, W).meshgrid): "
                                       "the kernel generates the coordinates itself" % who)


def disparity_consistency_src_to_tgt(meshgrid_homo, K_src_inv, disparity_src, G_tgt_src, K_tgt, disparity_tgt):
    """mean over the source pixels that project into the target frame of |1 / z_tgt - disparity_tgt[rounded target pixel]|   (reference :180-210)

    :param meshgrid_homo: 3xHxW - the standard (x, y, 1) grid of HomographySample for the frame's size (the kernel generates the coordinates)
    :param K_src_inv: Bx3x3
    :param disparity_src: Bx1xHxW float32 on the GPU
    :param G_tgt_src: Bx4x4
    :param K_tgt: Bx3x3
    :param disparity_tgt: Bx1xHxW float32 on the GPU, the size of disparity_src
    :return: a 0-dim float32 tensor on the GPU; NaN when no source pixel lands in the target frame (the mean of an empty selection)

    One fused pass (mpf_disp_consistency) with the matrices on the device: loss and count stay there, nothing synchronises with the host.  Differentiable
    with respect to disparity_src (one store per pixel, the same bits on every run) and disparity_tgt (a float-atomic scatter: source pixels that land on
    one target pixel decide its last bits by their order) under default grad mode - plane_geometry_grad() is not needed.  K_src_inv, G_tgt_src or K_tgt
    requiring grad is refused."""
    who = "disparity_consistency_src_to_tgt"
    _autograd.refuse_geometry(who, (), K_src_inv=K_src_inv, G_tgt_src=G_tgt_src, K_tgt=K_tgt)
    if isinstance(disparity_src, torch.Tensor) and disparity_src.dim() == 4:
        _require_standard_meshgrid(who, meshgrid_homo, disparity_src.size(2), disparity_src.size(3))
    dev = disparity_src.device if isinstance(disparity_src, torch.Tensor) else None
    mats = [m.detach().to(dev, torch.float32).contiguous() if isinstance(m, torch.Tensor) else m for m in (K_src_inv, G_tgt_src, K_tgt)]
    if _autograd.wants_grad(disparity_src, disparity_tgt):
        _autograd.check_values(who, disparity_src=disparity_src, disparity_tgt=disparity_tgt)
        return _autograd.DisparityConsistencyFn.apply(disparity_src, disparity_tgt, *mats)
    return ops.disparity_consistency(mats[0], disparity_src.detach(), mats[1], mats[2], disparity_tgt.detach())[0]


def plane_volume_rendering(rgb_BS3HW, sigma_BS1HW, xyz_BS3HW, src_sigma_BS1HW, src_flow_BS2HW, src_xyz_BS3HW,
                           is_bg_depth_inf, hard_flow=False, obj_mask=None):
    """reference :62-99 -> (rgb_out Bx3xHxW, depth_out Bx1xHxW, transparency_acc BxSx1xHxW, weights BxSx1xHxW,
    flow_out Bx2xHxW | None, obj_mask Bx1xHxW | as passed)"""
    B, S, _, H, W = sigma_BS1HW.size()
    _autograd.refuse_geometry("plane_volume_rendering", ("xyz_BS3HW", "src_xyz_BS3HW"), xyz_BS3HW=xyz_BS3HW, src_xyz_BS3HW=src_xyz_BS3HW)
    with_extra = src_sigma_BS1HW is not None
    grad = _autograd.wants_grad(rgb_BS3HW, sigma_BS1HW, src_flow_BS2HW if with_extra else None, obj_mask if with_extra else None) \
        or _autograd.wants_geometry_grad(xyz_BS3HW)
    if grad:
        _autograd.refuse_bg_depth_inf("plane_volume_rendering", is_bg_depth_inf)
        _autograd.check_values("plane_volume_rendering", rgb_BS3HW=rgb_BS3HW, sigma_BS1HW=sigma_BS1HW, xyz_BS3HW=xyz_BS3HW,
                               src_flow_BS2HW=src_flow_BS2HW if with_extra else None, obj_mask=obj_mask if with_extra else None)
    volume_render = _autograd.volume_render if grad else ops.volume_render
    rgbs, depths, taccs, wts, flows, oms = [], [], [], [], [], []
    for b in range(B):
        extra = None
        if src_sigma_BS1HW is not None:
            parts = [src_flow_BS2HW[b].to(torch.float32)]
            if obj_mask is not None:
                parts.append(obj_mask[b].to(torch.float32))
            extra = torch.cat(parts, dim=1).contiguous()
        r = volume_render(rgb_BS3HW[b], sigma_BS1HW[b, :, 0], xyz_BS3HW[b], extra_SEN=extra)
        depth = r["depth"]
        if is_bg_depth_inf:      # :146-149 (DTU option): sum(w z) + (1 - sum w) * 1000 instead of the normalised depth
            wsum = ops.weighted_sum(r["weights"])[0]
            wz = ops.weighted_sum(r["weights"], xyz_BS3HW[b][:, 2:3].contiguous())[0]
            depth = wz + (1 - wsum) * 1000
        rgbs.append(r["rgb"]); depths.append(depth.unsqueeze(0)); taccs.append(r["tacc"].unsqueeze(1)); wts.append(r["weights"].unsqueeze(1))
        if extra is not None:
            flows.append(r["extra"][0:2])
            if obj_mask is not None:
                oms.append(r["extra"][2:3])
    flow_out = torch.stack(flows) if flows else None
    om_out = torch.stack(oms) if oms else obj_mask
    return torch.stack(rgbs), torch.stack(depths), torch.stack(taccs), torch.stack(wts), flow_out, om_out


def plane_volume_rendering_flow(src_sigma_BS1HW, src_flow_BS2HW, src_xyz_BS3HW, is_bg_depth_inf, hard_flow=False):
    """reference :102-139 -> flow_out Bx2xHxW (hard_flow: the arg-max-weight plane's flow)"""
    B = src_sigma_BS1HW.size(0)
    _autograd.refuse_geometry("plane_volume_rendering_flow", ("src_xyz_BS3HW",), src_xyz_BS3HW=src_xyz_BS3HW)
    grad = _autograd.wants_grad(src_sigma_BS1HW, src_flow_BS2HW) or _autograd.wants_geometry_grad(src_xyz_BS3HW)
    if grad:
        _autograd.refuse_bg_depth_inf("plane_volume_rendering_flow", is_bg_depth_inf)
        _autograd.check_values("plane_volume_rendering_flow", src_sigma_BS1HW=src_sigma_BS1HW, src_flow_BS2HW=src_flow_BS2HW,
                               src_xyz_BS3HW=src_xyz_BS3HW)
    volume_render = _autograd.volume_render if grad else ops.volume_render
    out = []
    for b in range(B):
        r = volume_render(None, src_sigma_BS1HW[b, :, 0], src_xyz_BS3HW[b], extra_SEN=src_flow_BS2HW[b], hard=hard_flow,
                          want_tacc=False, want_weights=False)
        out.append(r["extra"])
    return torch.stack(out)


def weighted_sum_mpi(rgb_BS3HW, xyz_BS3HW, weights, is_bg_depth_inf):
    """reference :142-154 -> (rgb_out Bx3xHxW, depth_out Bx1xHxW)"""
    B = rgb_BS3HW.size(0)
    rgbs, depths = [], []
    for b in range(B):
        w = weights[b, :, 0]
        wsum = ops.weighted_sum(w)
        rgbs.append(ops.weighted_sum(w, rgb_BS3HW[b]))
        wz = ops.weighted_sum(w, xyz_BS3HW[b][:, 2:3].contiguous())
        depths.append(wz + (1 - wsum) * 1000 if is_bg_depth_inf else wz / (wsum + 1e-5))
    return torch.stack(rgbs), torch.stack(depths)


def get_src_xyz_from_plane_disparity(meshgrid_src_homo, mpi_disparity_src, K_src_inv):
    """xyz_src[b,s] = (K^-1 . (x,y,1)) / disparity[b,s]   (reference :213-239)

    :param meshgrid_src_homo: 3xHxW - must be the standard (x, y, 1) grid of HomographySample (its values are
                              regenerated from pixel indices in the kernel; only H and W are read from it)
    :param mpi_disparity_src: BxS
    :param K_src_inv: Bx3x3
    :return: BxSx3xHxW

    Inside plane_geometry_grad() a mpi_disparity_src that requires grad (float32, on the GPU) receives
    dL/ddisparity_s = -depth_s^2 sum_p <g_s(p), K^-1 (x, y, 1)> (mpf_src_xyz_bwd), and the returned tensor's tag remembers it for the fused backward.
    K_src_inv stays a constant."""
    B, S = mpi_disparity_src.size()
    H, W = meshgrid_src_homo.size(1), meshgrid_src_homo.size(2)
    dev = mpi_disparity_src.device if mpi_disparity_src.is_cuda else meshgrid_src_homo.device
    if _autograd.geometry_grad_enabled():              # outside, the helper is forward only whatever requires grad, as it always was
        _autograd.refuse_geometry("get_src_xyz_from_plane_disparity", ("mpi_disparity_src",), mpi_disparity_src=mpi_disparity_src, K_src_inv=K_src_inv)
    if _autograd.wants_geometry_grad(mpi_disparity_src):
        _autograd.check_values("get_src_xyz_from_plane_disparity", mpi_disparity_src=mpi_disparity_src)
        return _tag(_autograd.SrcXyzFn.apply(mpi_disparity_src, K_src_inv, H, W), "src", _key(K_src_inv, mpi_disparity_src), mpi_disparity_src)
    out = [ops.src_xyz(K_src_inv[b], host_math.plane_depths(mpi_disparity_src[b]), H, W, dev) for b in range(B)]
    return _tag(torch.stack(out), "src", _key(K_src_inv, mpi_disparity_src))


def get_tgt_xyz_from_plane_disparity(xyz_src_BS3HW, G_tgt_src):
    """xyz_tgt = G . [xyz_src; 1]   (reference :242-256) -> BxSx3xHxW

    Inside plane_geometry_grad() an xyz_src_BS3HW that requires grad (float32, on the GPU) receives R^T g (mpf_transform_xyz with [R^T | 0]); the tag of
    the result carries on the disparity tensor that xyz_src_BS3HW's tag remembers.  G_tgt_src stays a constant."""
    B, S, _, H, W = xyz_src_BS3HW.size()
    if _autograd.geometry_grad_enabled():
        _autograd.refuse_geometry("get_tgt_xyz_from_plane_disparity", ("xyz_src_BS3HW",), xyz_src_BS3HW=xyz_src_BS3HW, G_tgt_src=G_tgt_src)
    src_key = _tagged(xyz_src_BS3HW, "src")
    if _autograd.wants_geometry_grad(xyz_src_BS3HW):
        _autograd.check_values("get_tgt_xyz_from_plane_disparity", xyz_src_BS3HW=xyz_src_BS3HW)
        res = _autograd.TransformXyzFn.apply(xyz_src_BS3HW, G_tgt_src)
        return _tag(res, "tgt", src_key + _key(G_tgt_src), _tag_leaf(xyz_src_BS3HW)) if src_key is not None else res
    out = [ops.transform_xyz(G_tgt_src[b], xyz_src_BS3HW[b].reshape(S, 3, H * W)).reshape(S, 3, H, W) for b in range(B)]
    res = torch.stack(out)
    return _tag(res, "tgt", src_key + _key(G_tgt_src)) if src_key is not None else res


def _same_mask_on_every_plane(obj_mask_BS1HW):
    """The reference hands over S copies of ONE mask (utils/utils.py:323: obj_mask.unsqueeze(1).repeat(B, S, 1, 1, 1)); the fused kernel takes
    the mask once.  An expanded view is recognised by its stride, a materialised repeat by comparing the planes (one pass over the tensor)."""
    if obj_mask_BS1HW.size(1) == 1 or obj_mask_BS1HW.stride(1) == 0:
        return True
    return bool((obj_mask_BS1HW[:, 1:] == obj_mask_BS1HW[:, :1]).all())


def fused_render_applies(mpi_disparity_src, xyz_tgt_BS3HW, xyz_src_BS3HW, G_tgt_src, K_src_inv, K_tgt, use_alpha=False, is_bg_depth_inf=False,
                         hard_flow=False, obj_mask=None):
    """True when render_tgt_rgb_depth may dispatch to the fused kernels: default options, xyz tensors that carry this module's tag for exactly
    these (K_src_inv, disparities, G_tgt_src), and one mask on every plane.  (K_tgt is free: it only enters the homographies.)"""
    if use_alpha or is_bg_depth_inf or hard_flow:
        return False
    src_key, tgt_key = _tagged(xyz_src_BS3HW, "src"), _tagged(xyz_tgt_BS3HW, "tgt")
    if src_key is None or tgt_key is None:
        return False
    want_src = _key(K_src_inv, mpi_disparity_src)
    if src_key != want_src or tgt_key != want_src + _key(G_tgt_src):
        return False
    return obj_mask is None or _same_mask_on_every_plane(obj_mask)


def _render_tgt_fused(mpi_rgb_src, mpi_sigma_src, mpi_disparity_src, G_tgt_src, K_src_inv, K_tgt, obj_mask):
    """The fused form of render_tgt_rgb_depth: Stage B on the two channel-planar tensors in place (mpf_warp_composite_split: homography warp,
    analytic xyz_tgt, front-to-back composite, depth, validity count, rendered mask) + the source-frame flow of the sigma tensor
    (mpf_src_flow) - two launches per batch item instead of the reference-shaped chain (8-channel concatenation, generic sampling of every
    channel, S-deep intermediates)."""
    B, S, _, H, W = mpi_rgb_src.size()
    dev = mpi_rgb_src.device
    rgbs, depths, tms, flows, oms = [], [], [], [], []
    for b in range(B):
        d = host_math.plane_depths(mpi_disparity_src[b])
        H_ts, H_st = host_math.homographies(G_tgt_src[b], K_src_inv[b], K_tgt[b], d)
        quads = ops.mask_quads(obj_mask[b, 0, 0].to(dev, torch.float32).contiguous(), False) if obj_mask is not None else None
        v = ops.warp_composite_split(mpi_rgb_src[b].to(torch.float32), mpi_sigma_src[b].to(torch.float32), quads, H_st, K_src_inv[b], G_tgt_src[b], d)
        rgbs.append(v["rgb"]); depths.append(v["depth"].reshape(1, H, W)); tms.append(v["tgt_mask"].reshape(1, H, W))
        flows.append(ops.src_flow(mpi_sigma_src[b].to(torch.float32), K_src_inv[b], d, H_ts.unsqueeze(0), flow_clip=0.0)[0])
        if obj_mask is not None:
            oms.append(v["objmask"].reshape(1, H, W))
    return torch.stack(rgbs), torch.stack(depths), torch.stack(tms), torch.stack(flows), (torch.stack(oms) if oms else None)


def _render_tgt_fused_grad(mpi_rgb_src, mpi_sigma_src, mpi_disparity_src, G_tgt_src, K_src_inv, K_tgt, obj_mask, disparity_leaf=None):
    """_render_tgt_fused when mpi_rgb_src or mpi_sigma_src requires grad: the same launches (same values, bit for bit), with rgb, depth and the rendered
    mask connected to the two stacks through mpf_warp_composite_bwd.  flowA2B is computed as in _render_tgt_fused, from the detached sigma: it is
    returned with requires_grad == False (its gradient needs fused=False).  tgt_mask never carries gradient.  disparity_leaf: the disparity tensor
    that the xyz tensors were built from, which receives the gradient the reference sends through xyz_tgt (mpf_warp_composite_bwd_disp)."""
    B = mpi_rgb_src.size(0)
    rgb, depth, tgt_mask, om = _autograd.WarpCompositeFn.apply(mpi_rgb_src, mpi_sigma_src, mpi_disparity_src.detach(), G_tgt_src, K_src_inv, K_tgt, obj_mask,
                                                               disparity_leaf)
    flows = []
    with torch.no_grad():
        for b in range(B):
            d = host_math.plane_depths(mpi_disparity_src[b])
            H_ts, _ = host_math.homographies(G_tgt_src[b], K_src_inv[b], K_tgt[b], d)
            flows.append(ops.src_flow(mpi_sigma_src[b].to(torch.float32), K_src_inv[b], d, H_ts.unsqueeze(0), flow_clip=0.0)[0])
    return rgb, depth, tgt_mask, torch.stack(flows), om


def render_tgt_rgb_depth(H_sampler: HomographySample, mpi_rgb_src, mpi_sigma_src, mpi_disparity_src, xyz_tgt_BS3HW,
                         xyz_src_BS3HW, G_tgt_src, K_src_inv, K_tgt, mpi_flow_src=None, use_alpha=False,
                         is_bg_depth_inf=False, hard_flow=False, obj_mask=None, fused=None):
    """reference :259-349 -> (tgt_rgb_syn Bx3xHxW, tgt_depth_syn Bx1xHxW, tgt_mask Bx1xHxW, flowA2B Bx2xHxW,
    tgt_obj_mask_sync Bx1xHxW).  `mpi_flow_src` is accepted and ignored exactly as in the reference (:267).

    fused (not a reference argument): None = dispatch to the fused kernels when fused_render_applies(...) - the standard call of
    utils/utils.py:291-349 -, else the generic kernels that work on the materialised tensors; False = always generic; True = fused, raising
    if it does not apply.  The two forms differ by fp32 rounding only (the generic one interpolates the xyz_tgt channels bilinearly, the fused
    one evaluates the same affine field at the interpolated coordinate): both sit inside the parity bars against the reference's outputs
    (tests/test_dropin_api.py), tgt_mask is identical.

    Gradients: when mpi_rgb_src, mpi_sigma_src or obj_mask requires grad (float32, one GPU) the outputs carry them.  The generic form is then the
    differentiable sampler followed by the differentiable render(), with torch's own cat / slice / where in between: every output but tgt_mask is
    connected.  The fused form (taken with fused=None exactly when it would be taken without gradients, unless obj_mask itself requires grad) runs
    mpf_warp_composite_bwd, which holds no S-deep intermediate: rgb, depth and the rendered mask get gradients to mpi_rgb_src and mpi_sigma_src;
    flowA2B is returned with requires_grad == False - pass fused=False for its gradient.  Disparities, xyz tensors, pose and intrinsics are
    constants (one that requires grad is refused), is_bg_depth_inf=True is refused, and both sampling adjoints add with float atomics, so the last
    bits of a gradient depend on the order of the adds.

    Inside plane_geometry_grad(): xyz_tgt_BS3HW, xyz_src_BS3HW and mpi_disparity_src may require grad.  Generic form: the sampled xyz_tgt stays on the
    graph (the z >= 0 gate is a constant condition), and mpi_disparity_src reaches flowA2B through sample_inverse.  Fused form: the gradient that the
    reference sends through xyz_tgt goes to the disparity tensor the xyz tensors were built from - which their tag remembers - through
    mpf_warp_composite_bwd_disp, without an [S,3,H,W] gradient; flowA2B stays detached there, so its gradient to a disparity (the xyz_src path and
    the mpi_disparity_src argument's) needs fused=False.  Poses and intrinsics stay refused."""
    _autograd.refuse_geometry("render_tgt_rgb_depth", ("mpi_disparity_src", "xyz_tgt_BS3HW", "xyz_src_BS3HW"), mpi_disparity_src=mpi_disparity_src,
                              xyz_tgt_BS3HW=xyz_tgt_BS3HW, xyz_src_BS3HW=xyz_src_BS3HW, G_tgt_src=G_tgt_src, K_src_inv=K_src_inv, K_tgt=K_tgt)
    geom = _autograd.wants_geometry_grad(mpi_disparity_src, xyz_tgt_BS3HW, xyz_src_BS3HW)
    grad = _autograd.wants_grad(mpi_rgb_src, mpi_sigma_src, obj_mask) or geom
    if grad:
        _autograd.refuse_bg_depth_inf("render_tgt_rgb_depth", is_bg_depth_inf)
        _autograd.check_values("render_tgt_rgb_depth", mpi_rgb_src=mpi_rgb_src, mpi_sigma_src=mpi_sigma_src, xyz_tgt_BS3HW=xyz_tgt_BS3HW,
                               xyz_src_BS3HW=xyz_src_BS3HW, obj_mask=obj_mask if _autograd.wants_grad(obj_mask) else None,
                               mpi_disparity_src=mpi_disparity_src if _autograd.wants_geometry_grad(mpi_disparity_src) else None)
    if fused is None or fused:
        ok = fused_render_applies(mpi_disparity_src, xyz_tgt_BS3HW, xyz_src_BS3HW, G_tgt_src, K_src_inv, K_tgt, use_alpha, is_bg_depth_inf,
                                  hard_flow, obj_mask)
        if fused and not ok:
            raise ValueError("render_tgt_rgb_depth(fused=True): the fused kernels need default options, one mask on every plane and xyz tensors built by "
                             "this module's get_src_xyz_from_plane_disparity / get_tgt_xyz_from_plane_disparity for the same K, disparities and pose")
        if ok and _autograd.wants_grad(obj_mask):      # the fused backward treats the mask as a constant: its gradient needs the generic form
            if fused:
                raise _lib.MpiFlowHipError("render_tgt_rgb_depth(fused=True): obj_mask requires grad, and the fused backward gives gradients to mpi_rgb_src "
                                           "and mpi_sigma_src only; pass fused=False (or None) for the gradient of obj_mask")
            ok = False
        leaf = None
        if ok and _autograd.wants_geometry_grad(xyz_tgt_BS3HW):
            # the fused kernels never read xyz_tgt: its gradient goes straight to the disparity tensor it was built from, which its tag remembers
            leaf = _tag_leaf(xyz_tgt_BS3HW)
            if leaf is None or not leaf.requires_grad:
                if fused:
                    raise _lib.MpiFlowHipError("render_tgt_rgb_depth(fused=True): xyz_tgt_BS3HW requires grad but was not built from a disparity tensor "
                                               "that requires grad by this module's helpers inside plane_geometry_grad(); pass fused=False (or None)")
                ok = False
        if ok and grad:
            return _render_tgt_fused_grad(mpi_rgb_src, mpi_sigma_src, mpi_disparity_src, G_tgt_src, K_src_inv, K_tgt, obj_mask, leaf)
        if ok:
            return _render_tgt_fused(mpi_rgb_src, mpi_sigma_src, mpi_disparity_src, G_tgt_src, K_src_inv, K_tgt, obj_mask)
    B, S, _, H, W = mpi_rgb_src.size()
    mpi_depth_src = torch.reciprocal(mpi_disparity_src.detach().to("cpu", torch.float32))          # :284
    # the host copy above is what the homographies are built from; with a disparity gradient the reciprocal is also taken on the graph, for sample_inverse
    depth_graph = torch.reciprocal(mpi_disparity_src).view(B * S) if _autograd.wants_geometry_grad(mpi_disparity_src) else None
    xyz_grad = _autograd.wants_geometry_grad(xyz_tgt_BS3HW)
    mpi_xyz_src = torch.cat((mpi_rgb_src.to(torch.float32), mpi_sigma_src.to(torch.float32), xyz_tgt_BS3HW.to(torch.float32)), dim=2)
    if obj_mask is not None:
        mpi_xyz_src = torch.cat((mpi_xyz_src, obj_mask.to(torch.float32)), dim=2)
    G_Bs44 = G_tgt_src.unsqueeze(1).repeat(1, S, 1, 1).contiguous().reshape(B * S, 4, 4)
    Kinv_Bs33 = K_src_inv.unsqueeze(1).repeat(1, S, 1, 1).contiguous().reshape(B * S, 3, 3)
    Kt_Bs33 = K_tgt.unsqueeze(1).repeat(1, S, 1, 1).contiguous().reshape(B * S, 3, 3)
    # channels 4..6 are xyz_tgt, a constant unless it requires grad inside plane_geometry_grad(): under autograd only the colour / density channels (and
    # the mask's) get the sampler's scatter
    grad_ranges = ([(0, mpi_xyz_src.size(2))] if xyz_grad else [(0, 4)] + ([(7, mpi_xyz_src.size(2))] if obj_mask is not None else []))
    tgt, tgt_mask_BsHW, _ = H_sampler.sample(mpi_xyz_src.view(B * S, -1, H, W), mpi_depth_src.view(B * S), G_Bs44, Kinv_Bs33, Kt_Bs33,
                                             _grad_ranges=grad_ranges)
    if depth_graph is not None:
        flowB2A = H_sampler.sample_inverse(mpi_xyz_src.view(B * S, -1, H, W), depth_graph, G_Bs44, Kinv_Bs33, Kt_Bs33, _d_host=mpi_depth_src.view(B * S))
    else:
        flowB2A = H_sampler.sample_inverse(mpi_xyz_src.view(B * S, -1, H, W), mpi_depth_src.view(B * S), G_Bs44, Kinv_Bs33, Kt_Bs33)
    flowB2A = flowB2A.permute(0, 3, 1, 2).reshape(B, S, 2, H, W)                                     # :316
    tgt = tgt.view(B, S, -1, H, W)
    tgt_rgb, tgt_sigma, tgt_xyz = tgt[:, :, 0:3], tgt[:, :, 3:4], tgt[:, :, 4:7]
    if not xyz_grad:
        tgt_xyz = tgt_xyz.detach()                                                                  # the sampled xyz_tgt is geometry: a constant
    tgt_om = tgt[:, :, 7:] if obj_mask is not None else None
    tgt_sigma = torch.where(tgt_xyz[:, :, -1:] >= 0, tgt_sigma, torch.zeros_like(tgt_sigma))        # :336-338
    rgb_syn, depth_syn, _, _, flowA2B, om_sync = render(tgt_rgb.contiguous(), tgt_sigma.contiguous(), tgt_xyz.contiguous(),
                                                        mpi_sigma_src, flowB2A, xyz_src_BS3HW, use_alpha=use_alpha,
                                                        is_bg_depth_inf=is_bg_depth_inf, hard_flow=hard_flow,
                                                        obj_mask=tgt_om.contiguous() if tgt_om is not None else None)
    tgt_mask = torch.sum(tgt_mask_BsHW.view(B, S, H, W).to(torch.float32), dim=1, keepdim=True)      # :347 (exact integers)
    return rgb_syn, depth_syn, tgt_mask, flowA2B, om_sync
