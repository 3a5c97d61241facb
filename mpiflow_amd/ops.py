"""Tensor-level wrappers over the C ABI (include/mpiflow_hip.h): torch CUDA tensors in, torch CUDA tensors out.

PyTorch is plumbing here (device memory, current stream); all arithmetic on tensors happens in the HIP kernels of
libmpiflow_hip.so.  Every function launches asynchronously on torch's current stream and raises MpiFlowHipError if
the library is missing or a launch fails - there is no eager/CPU fallback.
"""
import ctypes
import operator

import torch

from . import _lib, host_math
from ._tensors import check_devices, check_pyramid, check_tensor

_f32 = torch.float32


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _on_device(fn):
    """Run `fn` with the device of its first CUDA tensor (or torch.device) argument current, so that the HIP launch and
    torch's "current stream" both refer to the GPU that owns the buffers, whatever device the caller had selected."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        dev = None
        flat = []
        for a in list(args) + list(kwargs.values()):                 # a list of tensors (a pyramid) counts as its tensors
            flat.extend(a if isinstance(a, (list, tuple)) else [a])
        for a in flat:
            if isinstance(a, torch.Tensor) and a.is_cuda:
                dev = a.device
                break
            if isinstance(a, torch.device) and a.type == "cuda":
                dev = a
                break
        if dev is None or dev.index is None:
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapped


def _dev(t, name, dtype=_f32):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise _lib.MpiFlowHipError("%s must live on the GPU (got %s); mpiflow_amd has no CPU path" % (name, t.device))
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def upload_params(host_buf, device):
    """Small per-call matrices -> device (one async H2D copy of a few KB on the current stream)."""
    return host_buf.pin_memory().to(device=device, non_blocking=True)


# ---- fused hot path ---------------------------------------------------------------------------------------------

def blend_flow_params(K_inv, depth_S, homs_tgt_src=None):
    """Host image of d_params for mpf_src_blend_flow.  homs_tgt_src: None or [P,S,3,3] (P <= 2).  -> (buf, P)"""
    d = host_math._cpu32(depth_S).reshape(-1)
    S = d.numel()
    if homs_tgt_src is None:
        return host_math.pack_params(K_inv=K_inv, depths=d), 0
    hts = host_math._cpu32(homs_tgt_src).reshape(-1, S, 3, 3)
    P = hts.shape[0]
    homs = hts.permute(1, 0, 2, 3).reshape(S * P, 3, 3)               # record = s*P + p
    return host_math.pack_params(K_inv=K_inv, homs=homs, depths=d.repeat_interleave(P)), P


def warp_params(H_src_tgt, K_inv, G, depth_S):
    """Host image of d_params for mpf_warp_composite."""
    d = host_math._cpu32(depth_S).reshape(-1)
    return host_math.pack_params(K_inv=K_inv, G=G, homs=host_math._cpu32(H_src_tgt).reshape(d.numel(), 3, 3), depths=d)


@_on_device
def src_blend_flow(mpi_S4HW, img_3HW, K_inv=None, depth_S=None, homs_tgt_src=None, flow_clip=200.0,
                   want_rgba=True, want_planar=False, want_tacc=False, out_rgba=None, out_flows=None,
                   dparams=None, P=None, src_u8=None, obj_mask=None, quads=None, quads_complement=None, cum_mask=None,
                   support=None, support_complement=None, tag=0):
    """Stage A + C.  homs_tgt_src: None or [P,S,3,3] CPU (P <= 2), or pass a pre-uploaded `dparams` + P.
    Fused by-products (preallocated outputs, optional): src_u8 [H,W,3] u8 BGR source frame; quads / quads_complement
    [H,W,4] = mask_quads(obj_mask, False / True).  cum_mask [S,H,W]: `mpi` is the RAW decoder output and the network's
    activation epilogue (sigmoid / relu(x*cum_mask)+1e-4) is fused into this pass.  support / support_complement: the mask support maps of
    quads / quads_complement (alloc_support_map) - their live cells get `tag` (mpf_src_blend_flow_support).  Returns dict(rgba, rgb_planar, tacc, flows)."""
    lib = _lib.load()
    mpi = _dev(mpi_S4HW, "mpi")
    S, C, H, W = mpi.shape
    assert C == 4
    img = _dev(img_3HW, "img").reshape(3, H, W)
    if dparams is None:
        params, P = blend_flow_params(K_inv, depth_S, homs_tgt_src)
        dparams = upload_params(params, mpi.device)
    rgba = out_rgba if out_rgba is not None else (torch.empty((S, H, W, 4), dtype=_f32, device=mpi.device) if want_rgba else None)
    planar = torch.empty((S, 3, H, W), dtype=_f32, device=mpi.device) if want_planar else None
    tacc = torch.empty((S, H, W), dtype=_f32, device=mpi.device) if want_tacc else None
    flows = out_flows if out_flows is not None else (torch.empty((P, 2, H, W), dtype=_f32, device=mpi.device) if P else None)
    args = [_ptr(mpi), _ptr(img), _ptr(dparams), P, S, H, W, float(flow_clip), _ptr(rgba), _ptr(planar), _ptr(tacc), _ptr(flows), _ptr(src_u8),
            _ptr(_dev(obj_mask, "obj_mask").reshape(H, W)) if obj_mask is not None else None, _ptr(quads), _ptr(quads_complement),
            _ptr(_dev(cum_mask, "cum_mask")) if cum_mask is not None else None]
    _check_support_map(support, H, W, mpi.device)
    _check_support_map(support_complement, H, W, mpi.device)
    _lib.check(lib.mpf_src_blend_flow_support(*args, _ptr(support), _ptr(support_complement), int(tag), _stream()), "mpf_src_blend_flow_support")
    return dict(rgba=rgba, rgb_planar=planar, tacc=tacc, flows=flows)


@_on_device
def alloc_rgba_stack(S, H, W, device):
    """Interleaved [S,H,W,4] stack followed by (W+2) zeroed texels: lets Stage B read the east/south bilinear taps at fixed
    +16 / +row-byte offsets (`interleaved=2`); taps that fall outside the image carry weight exactly 0."""
    n = S * H * W * 4
    store = torch.zeros(n + (W + 2) * 4, dtype=_f32, device=device)
    return store[:n].view(S, H, W, 4)


def support_cells(H, W):
    """(rows, columns) of a mask support map over an H x W frame (MPF_SUPPORT_CELLS)."""
    return (H + _lib.SUPPORT_CELL_H - 1) // _lib.SUPPORT_CELL_H, (W + _lib.SUPPORT_CELL_W - 1) // _lib.SUPPORT_CELL_W


@_on_device
def alloc_support_map(H, W, device):
    """A zeroed mask support map (include/mpiflow_hip.h, "mask support maps"): int32 [rows, columns], to be used with tags 1, 2, ..."""
    return torch.zeros(support_cells(H, W), dtype=torch.int32, device=device)


def _check_support_map(t, H, W, device):
    assert t is None or (t.is_cuda and t.device == device and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == support_cells(H, W)), \
        "a support map is a contiguous int32 tensor of shape support_cells(H, W) on the stack's device"


def _support_array(views, H, W, device):
    """views' optional `support` = (map, tag, thresh) -> MpfViewSupport array, or None when no view carries one"""
    if not any(v.get("support") is not None for v in views):
        return None
    arr = (_lib.MpfViewSupport * len(views))()
    for i, v in enumerate(views):
        if v.get("support") is not None:
            cells, tag, thresh = v["support"]
            _check_support_map(cells, H, W, device)
            arr[i] = _lib.MpfViewSupport(cells.data_ptr(), int(tag), float(thresh))
    return arr


@_on_device
def support_dead_tiles(views, S, H, W):
    """The device's own skip decision (mpf_support_dead_tiles): uint8 [len(views), ceil(H/8), ceil(W/32)], 1 = the tile is not rendered.
    views as for warp_composite_views, each with `support` = (map, tag, thresh) or without."""
    lib = _lib.load()
    dev = views[0]["dparams"].device
    sup = _support_array(views, H, W, dev) or (_lib.MpfViewSupport * len(views))()
    dead = torch.empty((len(views), (H + 7) // 8, (W + 31) // 32), dtype=torch.uint8, device=dev)
    _lib.check(lib.mpf_support_dead_tiles(_view_array(views, dev), sup, len(views), S, H, W, _ptr(dead), _stream()), "mpf_support_dead_tiles")
    return dead


@_on_device
def mask_quads(obj_mask_HW, complement=False):
    lib = _lib.load()
    m = _dev(obj_mask_HW, "obj_mask")
    H, W = m.shape[-2:]
    m = m.reshape(H, W)
    q = torch.empty((H, W, 4), dtype=_f32, device=m.device)
    _lib.check(lib.mpf_build_mask_quads(_ptr(m), int(bool(complement)), H, W, _ptr(q), _stream()), "mpf_build_mask_quads")
    return q


@_on_device
def warp_composite(rgba, quads, H_src_tgt=None, K_inv=None, G=None, depth_S=None, interleaved=True, want_depth=True,
                   want_tgt_mask=True, dparams=None, out=None):
    """Stage B.  rgba [S,H,W,4] (interleaved) or [S,4,H,W]; quads from mask_quads() or None.  Either pass the small
    matrices or a pre-uploaded `dparams`.  `out`: optional dict of preallocated outputs to reuse.
    Returns dict(rgb [3,H,W], depth [H,W], objmask [H,W] | None, tgt_mask [H,W])."""
    lib = _lib.load()
    a = _dev(rgba, "rgba")
    if interleaved == 2:      # caller guarantees >= (W+1) texels of finite padding after the last plane (alloc_rgba_stack)
        assert a.untyped_storage().nbytes() - a.storage_offset() * 4 >= a.numel() * 4 + (a.shape[2] + 1) * 16
    if interleaved:
        S, H, W, C = a.shape
    else:
        S, C, H, W = a.shape
    assert C == 4
    if dparams is None:
        dparams = upload_params(warp_params(H_src_tgt, K_inv, G, depth_S), a.device)
    q = _dev(quads, "mask quads") if quads is not None else None
    u8 = out.get("rgb_u8") if out is not None else None
    if out is not None:
        rgb, depth, om, tm = out["rgb"], out.get("depth"), out.get("objmask"), out.get("tgt_mask")
    else:
        rgb = torch.empty((3, H, W), dtype=_f32, device=a.device)
        depth = torch.empty((H, W), dtype=_f32, device=a.device) if want_depth else None
        om = torch.empty((H, W), dtype=_f32, device=a.device) if q is not None else None
        tm = torch.empty((H, W), dtype=_f32, device=a.device) if want_tgt_mask else None
    _lib.check(lib.mpf_warp_composite(_ptr(a), int(interleaved), _ptr(q), _ptr(dparams), S, H, W, _ptr(rgb),
                                      _ptr(depth), _ptr(om), _ptr(tm), _ptr(u8), _stream()), "mpf_warp_composite")
    return dict(rgb=rgb, depth=depth, objmask=om, tgt_mask=tm, rgb_u8=u8)


@_on_device
def warp_composite_split(rgb_S3HW, sigma_S1HW, quads, H_src_tgt=None, K_inv=None, G=None, depth_S=None, want_depth=True, want_tgt_mask=True,
                         dparams=None, out=None):
    """Stage B on the two channel-planar tensors render_novel_view_dynamic receives (mpi_all_rgb_src [S,3,H,W], mpi_all_sigma_src
    [S,1,H,W] | [S,H,W]), read in place: no concatenation, no repack (mpf_warp_composite_split).  Returns warp_composite's dict."""
    lib = _lib.load()
    rgb_in = _dev(rgb_S3HW, "rgb stack")
    S, C, H, W = rgb_in.shape
    assert C == 3
    sig = _dev(sigma_S1HW, "sigma stack").reshape(S, H, W)
    if dparams is None:
        dparams = upload_params(warp_params(H_src_tgt, K_inv, G, depth_S), rgb_in.device)
    q = _dev(quads, "mask quads") if quads is not None else None
    u8 = out.get("rgb_u8") if out is not None else None
    if out is not None:
        rgb, depth, om, tm = out["rgb"], out.get("depth"), out.get("objmask"), out.get("tgt_mask")
    else:
        rgb = torch.empty((3, H, W), dtype=_f32, device=rgb_in.device)
        depth = torch.empty((H, W), dtype=_f32, device=rgb_in.device) if want_depth else None
        om = torch.empty((H, W), dtype=_f32, device=rgb_in.device) if q is not None else None
        tm = torch.empty((H, W), dtype=_f32, device=rgb_in.device) if want_tgt_mask else None
    _lib.check(lib.mpf_warp_composite_split(_ptr(rgb_in), _ptr(sig), _ptr(q), _ptr(dparams), S, H, W, _ptr(rgb), _ptr(depth), _ptr(om), _ptr(tm),
                                            _ptr(u8), _stream()), "mpf_warp_composite_split")
    return dict(rgb=rgb, depth=depth, objmask=om, tgt_mask=tm, rgb_u8=u8)


def _grad_buffer(t, name, shape, device, zero):
    """A gradient tensor the backward kernels write in place: the caller's (fp32, contiguous, of this shape, on this device) or a new one."""
    if t is None:
        return (torch.zeros if zero else torch.empty)(shape, dtype=_f32, device=device)
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == device and t.dtype == _f32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise _lib.MpiFlowHipError("%s must be a contiguous float32 tensor of shape %s on %s" % (name, tuple(shape), device))
    return t


@_on_device
def warp_composite_split_backward(rgb_S3HW, sigma_S1HW, quads, dparams, g_rgb, g_depth=None, g_objmask=None, grad_rgb=None, grad_sigma=None,
                                  want_disparity=False):
    """Adjoint of warp_composite_split with respect to the two stacks (mpf_warp_composite_bwd): the same rgb, sigma, quads and dparams as the forward
    call, the upstream gradients of rgb [3,H,W], depth [H,W] | None and objmask [H,W] | None.  -> (grad_rgb [S,3,H,W], grad_sigma [S,H,W]).  The kernel
    ADDS into grad_rgb / grad_sigma with float atomics: pass zero-initialised buffers (or none: they are allocated zeroed).  The order in which the adds
    arrive decides the last bits of each sum, so two runs may differ there.

    want_disparity: -> (grad_rgb, grad_sigma, grad_disparity [S]) through mpf_warp_composite_bwd_disp; the [tiles, S] workspace of its per-plane sums is
    allocated here.  That gradient uses no atomics: two runs give the same bits."""
    lib = _lib.load()
    rgb_in = _dev(rgb_S3HW, "rgb stack")
    S, C, H, W = rgb_in.shape
    assert C == 3
    sig = _dev(sigma_S1HW, "sigma stack").reshape(S, H, W)
    q = _dev(quads, "mask quads") if quads is not None else None
    gr = _dev(g_rgb, "g_rgb").reshape(3, H, W)
    gd = _dev(g_depth, "g_depth").reshape(H, W) if g_depth is not None else None
    gm = _dev(g_objmask, "g_objmask").reshape(H, W) if g_objmask is not None else None
    grad_rgb = _grad_buffer(grad_rgb, "grad_rgb", (S, 3, H, W), rgb_in.device, True)
    grad_sigma = _grad_buffer(grad_sigma, "grad_sigma", (S, H, W), rgb_in.device, True)
    if want_disparity:
        tiles = ((W + 31) // 32) * ((H + 7) // 8)
        partial = torch.empty((tiles, S), dtype=_f32, device=rgb_in.device)
        grad_disp = torch.empty((S,), dtype=_f32, device=rgb_in.device)
        _lib.check(lib.mpf_warp_composite_bwd_disp(_ptr(rgb_in), _ptr(sig), _ptr(q), _ptr(dparams), S, H, W, _ptr(gr), _ptr(gd), _ptr(gm), _ptr(grad_rgb),
                                                   _ptr(grad_sigma), _ptr(partial), tiles, _ptr(grad_disp), _stream()), "mpf_warp_composite_bwd_disp")
        return grad_rgb, grad_sigma, grad_disp
    _lib.check(lib.mpf_warp_composite_bwd(_ptr(rgb_in), _ptr(sig), _ptr(q), _ptr(dparams), S, H, W, _ptr(gr), _ptr(gd), _ptr(gm), _ptr(grad_rgb),
                                          _ptr(grad_sigma), _stream()), "mpf_warp_composite_bwd")
    return grad_rgb, grad_sigma


@_on_device
def src_flow(sigma_S1HW, K_inv, depth_S, homs_tgt_src, flow_clip=200.0):
    """Stage C alone (mpf_src_flow): volume-rendered flows [P,2,H,W] of P <= 2 poses from a bare sigma tensor [S,1,H,W] | [S,H,W]."""
    lib = _lib.load()
    sig = _dev(sigma_S1HW, "sigma stack")
    S, H, W = sig.shape[0], sig.shape[-2], sig.shape[-1]
    sig = sig.reshape(S, H, W)
    params, P = blend_flow_params(K_inv, depth_S, homs_tgt_src)
    dparams = upload_params(params, sig.device)
    flows = torch.empty((P, 2, H, W), dtype=_f32, device=sig.device)
    _lib.check(lib.mpf_src_flow(_ptr(sig), _ptr(dparams), P, S, H, W, float(flow_clip), _ptr(flows), _stream()), "mpf_src_flow")
    return flows


@_on_device
def src_flow_hard(sigma_or_stack, K_inv, depth_S, homs_tgt_src, flow_clip=200.0):
    """hard_flow=True in one pass (mpf_src_flow_hard): [P,2,H,W] flows of the arg-max-weight plane.  sigma_or_stack: a bare sigma tensor [S,1,H,W] | [S,H,W],
    or the [S,4,H,W] stack (its sigma planes are read in place)."""
    lib = _lib.load()
    t = _dev(sigma_or_stack, "sigma stack")
    S, H, W = t.shape[0], t.shape[-2], t.shape[-1]
    N = H * W
    if t.dim() == 4 and t.shape[1] == 4:
        ptr, stride = t.data_ptr() + 3 * N * 4, 4 * N
    else:
        t = t.reshape(S, H, W)
        ptr, stride = t.data_ptr(), N
    params, P = blend_flow_params(K_inv, depth_S, homs_tgt_src)
    dparams = upload_params(params, t.device)
    flows = torch.empty((P, 2, H, W), dtype=_f32, device=t.device)
    _lib.check(lib.mpf_src_flow_hard(ctypes.c_void_p(ptr), stride, _ptr(dparams), P, S, H, W, float(flow_clip), _ptr(flows), _stream()), "mpf_src_flow_hard")
    return flows


@_on_device
def warp_composite_views(rgba, views, interleaved=2):
    """Stage B for several views of one interleaved stack in ONE launch (mpf_warp_composite_views): the stack crosses the HBM
    interface once instead of once per view.  views: list of dicts(dparams=, quads= | None, out=dict(rgb, objmask?, depth?,
    tgt_mask?, rgb_u8?)) - every buffer preallocated.  Bit-identical to len(views) warp_composite calls.  A view with
    support=(map, tag, thresh) skips the tiles whose mask taps are all zero (mpf_warp_composite_views_support; output contract: include/mpiflow_hip.h)."""
    lib = _lib.load()
    a = _dev(rgba, "rgba")
    S, H, W, C = a.shape
    assert C == 4 and interleaved in (1, 2) and 1 <= len(views) <= _lib.MAX_VIEWS
    if interleaved == 2:
        assert a.untyped_storage().nbytes() - a.storage_offset() * 4 >= a.numel() * 4 + (W + 1) * 16
    _lib.check(lib.mpf_warp_composite_views_support(_ptr(a), int(interleaved), _view_array(views, a.device), _support_array(views, H, W, a.device), len(views),
                                                    S, H, W, _stream()), "mpf_warp_composite_views_support")
    return [v["out"] for v in views]


def _view_array(views, device):
    arr = (_lib.MpfWarpView * len(views))()
    for i, v in enumerate(views):
        o = v["out"]
        q = v.get("quads")
        for t in [v["dparams"], q] + [o.get(k) for k in ("rgb", "depth", "objmask", "tgt_mask", "rgb_u8")]:
            assert t is None or (t.is_cuda and t.is_contiguous() and t.device == device)
        arr[i] = _lib.MpfWarpView(v["dparams"].data_ptr(), q.data_ptr() if q is not None else None, o["rgb"].data_ptr(),
                                  *[(o[k].data_ptr() if o.get(k) is not None else None) for k in ("depth", "objmask", "tgt_mask", "rgb_u8")])
    return arr


@_on_device
def warp_views_and_blend_next(rgba, views, mpi_next, img_next, dparams_next, P, out_rgba_next, out_flows_next=None, flow_clip=200.0,
                              src_u8_next=None, obj_mask_next=None, quads_next=None, quads_complement_next=None, cum_mask_next=None,
                              merge_prev=None, support_next=None, support_complement_next=None, tag_next=0):
    """Stage B of one image (all `views` of the tail-padded stack `rgba`, as warp_composite_views) and Stage A+C of the NEXT image
    (as src_blend_flow with preallocated outputs) in ONE launch whose grid interleaves the two kinds of workgroups
    (mpf_warp_views_and_blend_next).  Bit-identical to the two separate calls; every *_next buffer must be distinct from what the
    views read or write.  merge_prev: merge_args(...) of an EARLIER pair, merged by the Stage A+C role as a per-pixel prologue
    (mpf_warp_views_blend_next_merge_prev); its flows may be `out_flows_next` itself.  Views with support=(map, tag, thresh) skip their dead
    tiles; support_next / support_complement_next are the next pair's maps, written with tag_next (mpf_warp_views_blend_next_merge_prev_support)."""
    lib = _lib.load()
    a = _dev(rgba, "rgba")
    S, H, W, C = a.shape
    assert C == 4 and 1 <= len(views) <= _lib.MAX_VIEWS
    assert a.untyped_storage().nbytes() - a.storage_offset() * 4 >= a.numel() * 4 + (W + 1) * 16
    mpi = _dev(mpi_next, "mpi_next")
    assert tuple(mpi.shape) == (S, 4, H, W) and out_rgba_next.is_contiguous() and tuple(out_rgba_next.shape) == (S, H, W, 4)
    assert out_rgba_next.data_ptr() != a.data_ptr()
    img = _dev(img_next, "img_next").reshape(3, H, W)
    arr = _view_array(views, a.device)
    om = _dev(obj_mask_next, "obj_mask_next").reshape(H, W) if obj_mask_next is not None else None
    cm = _dev(cum_mask_next, "cum_mask_next") if cum_mask_next is not None else None
    sup = _support_array(views, H, W, a.device)
    mp = ctypes.byref(merge_prev) if merge_prev is not None else None
    _check_support_map(support_next, H, W, a.device)
    _check_support_map(support_complement_next, H, W, a.device)
    _lib.check(lib.mpf_warp_views_blend_next_merge_prev_support(
        _ptr(a), arr, sup, len(views), _ptr(mpi), _ptr(img), _ptr(dparams_next), int(P), float(flow_clip), _ptr(out_rgba_next), _ptr(out_flows_next),
        _ptr(src_u8_next), _ptr(om), _ptr(quads_next), _ptr(quads_complement_next), _ptr(cm), _ptr(support_next), _ptr(support_complement_next),
        int(tag_next), S, H, W, mp, _stream()), "mpf_warp_views_blend_next_merge_prev_support")
    return [v["out"] for v in views]


def merge_args(frame, frame_dyn, mask, mask_dyn, flow, flow_dyn, obj_mask, thresh, out, obj_mask_stride=1):
    """mpf_merge's arguments as the struct a pair launch takes (warp_views_and_blend_next(merge_prev=...)) or mpf_merge_ex.  All tensors fp32
    contiguous on the device, out = (flow_mix [H,W,2] f32, frame_mix [H,W,3] u8, fill_mask [H,W] u8) on the same device; the caller keeps them
    alive until the launch was issued.  obj_mask_stride = 4: `obj_mask` is a mask-quad buffer [H,W,4] whose .x is the object mask."""
    import numpy as np
    for t in (frame, frame_dyn, mask, mask_dyn, flow, flow_dyn, obj_mask):
        assert t.is_cuda and t.dtype == _f32 and t.is_contiguous()
    _, H, W = frame.shape
    assert obj_mask_stride in (1, 4) and obj_mask.numel() == H * W * obj_mask_stride, (obj_mask_stride, tuple(obj_mask.shape))
    fm, fr, fi = out
    assert fm.is_cuda and fm.dtype == _f32 and fm.is_contiguous() and tuple(fm.shape) == (H, W, 2), "flow_mix must be f32 [H,W,2], contiguous"
    assert fr.is_cuda and fr.dtype == torch.uint8 and fr.is_contiguous() and tuple(fr.shape) == (H, W, 3), "frame_mix must be u8 [H,W,3], contiguous"
    assert fi.is_cuda and fi.dtype == torch.uint8 and fi.is_contiguous() and tuple(fi.shape) == (H, W), "fill_mask must be u8 [H,W], contiguous"
    assert fm.device == fr.device == fi.device == frame.device, "merge outputs must live on the device of the views"
    return _lib.MpfMergeArgs(frame.data_ptr(), frame_dyn.data_ptr(), mask.data_ptr(), mask_dyn.data_ptr(), flow.data_ptr(), flow_dyn.data_ptr(),
                             obj_mask.data_ptr(), float(np.float32(thresh)), fm.data_ptr(), fr.data_ptr(), fi.data_ptr(), int(obj_mask_stride))


def pair_slab(H, W, device):
    """One contiguous device buffer holding a pair's three products - flow_mix [H,W,2] f32 | frame_mix [H,W,3] u8 | fill_mask [H,W] u8 (12 H W bytes) -
    so that they leave the GPU in ONE device-to-host copy (io_formats.OutputRing.submit_pair_fill(slab=...)).  -> (slab u8 [12 H W], (flow_mix, frame_mix, fill_mask) views)"""
    n = H * W
    slab = torch.empty(12 * n, dtype=torch.uint8, device=device)
    return slab, slab_views(slab, H, W)


def slab_views(slab, H, W):
    n = H * W
    return (slab[:8 * n].view(torch.float32).view(H, W, 2), slab[8 * n:11 * n].view(H, W, 3), slab[11 * n:12 * n].view(H, W))


@_on_device
def merge(frame, frame_dyn, mask, mask_dyn, flow, flow_dyn, obj_mask, thresh=0.99, out=None, obj_mask_stride=1):
    """Stage D.  out: optional preallocated (flow_mix [H,W,2] f32, frame_mix [H,W,3] u8, fill_mask [H,W] u8); default: views of one pair_slab.
    obj_mask_stride = 4: `obj_mask` is a mask-quad buffer [H,W,4] whose .x is the object mask (mpf_merge_ex)."""
    lib = _lib.load()
    frame = _dev(frame, "frame")
    _, H, W = frame.shape
    dev = frame.device
    if out is not None:
        flow_mix, frame_mix, fill = out
    else:
        _, (flow_mix, frame_mix, fill) = pair_slab(H, W, dev)
    if obj_mask_stride != 1:
        import ctypes
        a = merge_args(frame, _dev(frame_dyn, "frame_dyn").reshape(3, H, W), _dev(mask, "mask").reshape(H, W), _dev(mask_dyn, "mask_dyn").reshape(H, W),
                       _dev(flow, "flow").reshape(2, H, W), _dev(flow_dyn, "flow_dyn").reshape(2, H, W), _dev(obj_mask, "obj_mask"), thresh,
                       (flow_mix, frame_mix, fill), obj_mask_stride=obj_mask_stride)
        _lib.check(lib.mpf_merge_ex(ctypes.byref(a), H, W, _stream()), "mpf_merge_ex")
        return flow_mix, frame_mix, fill
    args = [_dev(frame_dyn, "frame_dyn").reshape(3, H, W), _dev(mask, "mask").reshape(H, W),
            _dev(mask_dyn, "mask_dyn").reshape(H, W), _dev(flow, "flow").reshape(2, H, W),
            _dev(flow_dyn, "flow_dyn").reshape(2, H, W), _dev(obj_mask, "obj_mask").reshape(H, W)]
    import numpy as np
    _lib.check(lib.mpf_merge(_ptr(frame), *[_ptr(a) for a in args], float(np.float32(thresh)), H, W, _ptr(flow_mix),
                             _ptr(frame_mix), _ptr(fill), _stream()), "mpf_merge")
    return flow_mix, frame_mix, fill


@_on_device
def merge_depth_ordered(frame, frame_dyn, mask, mask_dyn, depth, depth_dyn, thresh=0.99, out=None, want_depth_mask=False):
    """The depth-ordered frame of the reference's older module ("utils/utils copy.py":278-303): Stage D's frame_mix, except that where both
    layers cover the pixel (both masks non-zero) and depth > depth_dyn the dynamic layer's pixel is taken.
    -> frame_mix_depth [H,W,3] u8 BGR (, depth_mask [H,W] u8 when want_depth_mask)."""
    import numpy as np
    lib = _lib.load()
    frame = _dev(frame, "frame")
    _, H, W = frame.shape
    dev = frame.device
    fmd = out if out is not None else torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    dm = torch.empty((H, W), dtype=torch.uint8, device=dev) if want_depth_mask else None
    args = [_dev(frame_dyn, "frame_dyn").reshape(3, H, W), _dev(mask, "mask").reshape(H, W), _dev(mask_dyn, "mask_dyn").reshape(H, W),
            _dev(depth, "depth").reshape(H, W), _dev(depth_dyn, "depth_dyn").reshape(H, W)]
    _lib.check(lib.mpf_merge_depth_ordered(_ptr(frame), *[_ptr(a) for a in args], float(np.float32(thresh)), H, W, _ptr(fmd), _ptr(dm),
                                           _stream()), "mpf_merge_depth_ordered")
    return (fmd, dm) if want_depth_mask else fmd


@_on_device
def fill_holes(img_HW3_u8, hole_HW_u8, out=None, hole_out=None, workspace=None):
    """Built-in deterministic hole fill (onion peel; NOT OpenCV's algorithm - see DESIGN.md, row A13).  Stream-ordered, no
    host synchronisation.  Returns the filled copy (`out`); `hole_out` (optional) receives the holes still open."""
    lib = _lib.load()
    src = _dev(img_HW3_u8, "img", torch.uint8)
    H, W, _ = src.shape
    out = torch.empty_like(src) if out is None else out
    out.copy_(src)
    hole = torch.empty((H, W), dtype=torch.uint8, device=src.device) if hole_out is None else hole_out
    hole.copy_(_dev(hole_HW_u8, "hole", torch.uint8))
    need = int(lib.mpf_fill_holes_workspace(H, W))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=src.device)
    _lib.check(lib.mpf_fill_holes(_ptr(out), _ptr(hole), H, W, _ptr(workspace), need, _stream()), "mpf_fill_holes")
    return out


@_on_device
def prepare_inputs(rgb_u8=None, disp_u8=None, ids_u8=None, obj_index=0, size=None, out=None):
    """Input stage in one launch (mpf_prepare_inputs): uploaded u8 buffers -> resized float tensors, bit-identical to the
    reference's ToTensor / `/255` / (ids == k).float() followed by F.interpolate(bilinear, align_corners=True).
    rgb_u8 [h,w,3], disp_u8 [h,w], ids_u8 [h,w] on the device (any subset); size = (H, W).
    Returns dict(image [3,H,W], disp [H,W], mask [H,W]) (None for absent inputs); `out` may carry preallocated tensors."""
    lib = _lib.load()
    H, W = size
    first = next(t for t in (rgb_u8, disp_u8, ids_u8) if t is not None)
    h, w = first.shape[:2]
    dev = first.device
    out = dict(out or {})
    rgb = _dev(rgb_u8, "rgb", torch.uint8) if rgb_u8 is not None else None
    dsp = _dev(disp_u8, "disp", torch.uint8) if disp_u8 is not None else None
    ids = _dev(ids_u8, "ids", torch.uint8) if ids_u8 is not None else None
    for t in (rgb, dsp, ids):
        assert t is None or tuple(t.shape[:2]) == (h, w)
    image = (out.get("image") if out.get("image") is not None else torch.empty((3, H, W), dtype=_f32, device=dev)) if rgb is not None else None
    disp = (out.get("disp") if out.get("disp") is not None else torch.empty((H, W), dtype=_f32, device=dev)) if dsp is not None else None
    mask = (out.get("mask") if out.get("mask") is not None else torch.empty((H, W), dtype=_f32, device=dev)) if ids is not None else None
    _lib.check(lib.mpf_prepare_inputs(_ptr(rgb), _ptr(dsp), _ptr(ids), int(obj_index), h, w, H, W, _ptr(image), _ptr(disp), _ptr(mask), _stream()),
               "mpf_prepare_inputs")
    return dict(image=image, disp=disp, mask=mask)


INPAINT_NS, INPAINT_TELEA = 0, 1          # cv2.INPAINT_NS / cv2.INPAINT_TELEA (MPF_INPAINT_*)


def inpaint_host(img_u8, mask_u8, radius=3, method=INPAINT_NS, out=None):
    """The reference's hole filling, cv2.inpaint(img, mask, radius, method) (utils/utils.py:284-286 NS, moving_obj.py:162 TELEA),
    as restated in libmpiflow_hip.so (mpf_inpaint_host): HOST numpy arrays in and out, like the reference's call; synchronous;
    ctypes releases the GIL, so frames fill in parallel on the generator's writer threads.  img u8 [H,W,3] | [H,W], mask u8 [H,W]."""
    import numpy as np
    lib = _lib.load()
    img = np.ascontiguousarray(img_u8, dtype=np.uint8)
    H, W = img.shape[:2]
    C = 1 if img.ndim == 2 else img.shape[2]
    mask = np.ascontiguousarray(mask_u8, dtype=np.uint8).reshape(H, W)
    if out is None:
        out = np.empty_like(img)
    assert out.shape == img.shape and out.dtype == np.uint8 and out.flags.c_contiguous and out is not img
    _lib.check(lib.mpf_inpaint_host(img.ctypes.data, mask.ctypes.data, H, W, C, float(radius), int(method), out.ctypes.data), "mpf_inpaint_host")
    return out


@_on_device
def inpaint_ns(img, mask, radius=3, out=None, workspace=None):
    """inpaint_host(img, mask, radius, INPAINT_NS) on the GPU, byte for byte (mpf_inpaint_ns): the reference's
    cv2.inpaint(frame_mix, fill_mask, 3, cv2.INPAINT_NS) (utils/utils.py:284-286), as restated by mpf_inpaint_host; parity with
    cv2 itself is as unpinned as the host restatement's.  img u8 [H,W,3] or [B,H,W,3] (BGR), mask [H,W] or [B,H,W] (non-zero = fill),
    both on the device; radius 1 - 4 (after cvInpaint's rounding); H, W >= 2.  Stream-ordered on the current stream, no host
    synchronisation.  Returns `out` (a new tensor unless given; it may not alias `img`).  `workspace`: u8 device tensor of at least
    inpaint_ns_workspace(B, H, W) bytes, allocated per call when absent or short."""
    lib = _lib.load()
    src = _dev(img, "img", torch.uint8)
    if src.dim() not in (3, 4) or src.shape[-1] != 3:
        raise ValueError("inpaint_ns: img must be [H,W,3] or [B,H,W,3] (got %s)" % (tuple(src.shape),))
    B, H, W = (1,) + tuple(src.shape[:2]) if src.dim() == 3 else tuple(src.shape[:3])
    m = _dev(mask, "mask", torch.uint8)
    if m.numel() != B * H * W:
        raise ValueError("inpaint_ns: mask of %s for images of %s" % (tuple(m.shape), tuple(src.shape)))
    if out is None:
        out = torch.empty_like(src)
    elif out.shape != src.shape or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != src.device:
        raise ValueError("inpaint_ns: out must be a contiguous u8 tensor of %s on %s" % (tuple(src.shape), src.device))
    need = inpaint_ns_workspace(B, H, W, radius)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=src.device)
    _lib.check(lib.mpf_inpaint_ns(_ptr(src), _ptr(m), B, H, W, float(radius), _ptr(out), _ptr(workspace), int(workspace.numel()), _stream()),
               "mpf_inpaint_ns")
    return out


def inpaint_ns_workspace(B, H, W, radius=3):
    """bytes of workspace mpf_inpaint_ns needs for B frames of H x W (about 45 per pixel: include/mpiflow_hip.h)"""
    return int(_lib.load().mpf_inpaint_ns_workspace(int(B), int(H), int(W), float(radius)))


def inpaint_ns_counters(workspace):
    """What the last inpaint_ns call with this workspace did, read from its first words once it has completed (synchronises with the
    current stream): clusters, heap pool items, clusters whose heap started in / moved to the pool, and `failed` - clusters left
    unfilled because a bound the fill relies on broke (0 unless the kernel is wrong)."""
    w = workspace[:24].view(torch.int32).cpu().tolist()
    return dict(clusters=w[0], pool_items=w[2], spilled_at_start=w[3], spilled_running=w[4], failed=w[5])


PAIR_STATS_SLICES = 64          # MPF_PAIR_STATS_SLICES


@_on_device
def pair_stats(flow_mix_HW2, fill_mask_HW, out4):
    """mpf_pair_stats: per-slice {sum |flow|, hole px, max |flow|, max(-flow)} of one pair into out4 ([64,4] float64 on the device),
    stream-ordered"""
    lib = _lib.load()
    flow = _dev(flow_mix_HW2, "flow_mix")
    fill = _dev(fill_mask_HW, "fill_mask", torch.uint8)
    H, W = fill.shape
    assert out4.dtype == torch.float64 and out4.numel() == 4 * PAIR_STATS_SLICES and out4.is_contiguous()
    _lib.check(lib.mpf_pair_stats(_ptr(flow), _ptr(fill), H, W, _ptr(out4), _stream()), "mpf_pair_stats")
    return out4


@_on_device
def png_scanlines(img_HW3_bgr_u8, out=None):
    """[H,W,3] u8 BGR on the device -> PNG scanlines u8 [H, 1+3W] (filter "Up", RGB order) for io_formats.png_from_scanlines"""
    lib = _lib.load()
    img = _dev(img_HW3_bgr_u8, "img", torch.uint8)
    H, W, _ = img.shape
    out = torch.empty((H, 3 * W + 1), dtype=torch.uint8, device=img.device) if out is None else out
    _lib.check(lib.mpf_png_filter_up(_ptr(img), H, W, _ptr(out), _stream()), "mpf_png_filter_up")
    return out


def _augment_out(name, B, H, W, dev, out, size):
    """The four output tensors of the augmentation launchers: `out`'s (checked), else new ones of crop `size`, else of the frame's size."""
    if out is not None:
        h, w = out["valid"].shape[-2:]
    else:
        h, w = size if size is not None else (H, W)
        out = dict(image1=torch.empty((B, 3, h, w), dtype=_f32, device=dev), image2=torch.empty((B, 3, h, w), dtype=_f32, device=dev),
                   flow=torch.empty((B, 2, h, w), dtype=_f32, device=dev), valid=torch.empty((B, h, w), dtype=_f32, device=dev))
    for k, shape in (("image1", (B, 3, h, w)), ("image2", (B, 3, h, w)), ("flow", (B, 2, h, w)), ("valid", (B, h, w))):
        t = out[k]
        if tuple(t.shape) != shape or t.dtype != _f32 or not t.is_contiguous() or t.device != dev:
            raise ValueError("%s: out[%r] must be a contiguous fp32 %s tensor on %s" % (name, k, shape, dev))
    return out, h, w


def augment_pairs(samples, out=None, size=None):
    """RAFT's spatial augmentation + tensor packing of a batch of pairs in one launch (mpf_augment_pairs), on the current stream.
    samples: B dicts with src / dst (u8 [H,W,3] BGR) and flow (f32 [H,W,2]) on the device, and resize, scale_x, scale_y, Hr, Wr, flip_h, flip_v,
    y0, x0 (missing keys: identity - no resize, no flips, origin 0).  The crop size is out's, else `size` = (h, w), else the frame's.
    -> dict(image1, image2 [B,3,h,w] RGB 0..255, flow [B,2,h,w], valid [B,h,w]), all fp32; `out` may carry these four tensors."""
    lib = _lib.load()
    B = len(samples)
    if B < 1:
        raise ValueError("augment_pairs: no samples")
    src0 = _dev(samples[0]["src"], "src", torch.uint8)
    H, W, _ = src0.shape
    dev = src0.device
    out, h, w = _augment_out("augment_pairs", B, H, W, dev, out, size)
    arr = (_lib.MpfAugmentSample * B)()
    keep = []
    with torch.cuda.device(dev):
        for b, s in enumerate(samples):
            src, dst, flow = _dev(s["src"], "src", torch.uint8), _dev(s["dst"], "dst", torch.uint8), _dev(s["flow"], "flow")
            if tuple(src.shape) != (H, W, 3) or tuple(dst.shape) != (H, W, 3) or tuple(flow.shape) != (H, W, 2):
                raise ValueError("augment_pairs: sample %d: src / dst must be [%d,%d,3], flow [%d,%d,2]" % (b, H, W, H, W))
            keep += [src, dst, flow]
            a = arr[b]
            a.src, a.dst, a.flow = src.data_ptr(), dst.data_ptr(), flow.data_ptr()
            a.resize = int(s.get("resize", 0))
            a.scale_x, a.scale_y = float(s.get("scale_x", 1.0)), float(s.get("scale_y", 1.0))
            a.Hr, a.Wr = int(s.get("Hr", H)), int(s.get("Wr", W))
            a.flip_h, a.flip_v = int(bool(s.get("flip_h", 0))), int(bool(s.get("flip_v", 0)))
            a.y0, a.x0 = int(s.get("y0", 0)), int(s.get("x0", 0))
        _lib.check(lib.mpf_augment_pairs(arr, B, H, W, h, w, _ptr(out["image1"]), _ptr(out["image2"]), _ptr(out["flow"]), _ptr(out["valid"]), _stream()),
                   "mpf_augment_pairs")
    return out


def augment_sparse_pairs(samples, out=None, size=None):
    """RAFT's sparse (KITTI-stage) spatial augmentation + tensor packing of a batch of pairs in one launch (mpf_augment_sparse_pairs), on the
    current stream: KITTI's 16-bit flow code, cv2 INTER_LINEAR images, resize_sparse_flow_map's nearest-pixel flow scatter, h-flip, crop.
    samples: B dicts with src / dst (u8 [H,W,3] BGR) and flow (f32 [H,W,2]) on the device, optionally valid (u8 or bool [H,W]; missing: every
    pixel valid), and quantize, resize, scale_x, scale_y, Hr, Wr, flip_h, y0, x0 (missing keys: identity - no KITTI code, no resize, no flip,
    origin 0).  The crop size is out's, else `size` = (h, w), else the frame's.
    -> dict(image1, image2 [B,3,h,w] RGB 0..255, flow [B,2,h,w], valid [B,h,w] 0 / 1), all fp32; `out` may carry these four tensors."""
    lib = _lib.load()
    B = len(samples)
    if B < 1:
        raise ValueError("augment_sparse_pairs: no samples")
    src0 = _dev(samples[0]["src"], "src", torch.uint8)
    H, W, _ = src0.shape
    dev = src0.device
    out, h, w = _augment_out("augment_sparse_pairs", B, H, W, dev, out, size)
    arr = (_lib.MpfSparseAugmentSample * B)()
    keep = []
    with torch.cuda.device(dev):
        for b, s in enumerate(samples):
            src, dst, flow = _dev(s["src"], "src", torch.uint8), _dev(s["dst"], "dst", torch.uint8), _dev(s["flow"], "flow")
            valid = None if s.get("valid") is None else _dev(s["valid"], "valid", torch.uint8)
            if tuple(src.shape) != (H, W, 3) or tuple(dst.shape) != (H, W, 3) or tuple(flow.shape) != (H, W, 2):
                raise ValueError("augment_sparse_pairs: sample %d: src / dst must be [%d,%d,3], flow [%d,%d,2]" % (b, H, W, H, W))
            if valid is not None and tuple(valid.shape) != (H, W):
                raise ValueError("augment_sparse_pairs: sample %d: valid must be [%d,%d]" % (b, H, W))
            keep += [src, dst, flow, valid]
            a = arr[b]
            a.src, a.dst, a.flow = src.data_ptr(), dst.data_ptr(), flow.data_ptr()
            a.valid = None if valid is None else valid.data_ptr()
            a.quantize, a.resize = int(bool(s.get("quantize", 0))), int(s.get("resize", 0))
            a.scale_x, a.scale_y = float(s.get("scale_x", 1.0)), float(s.get("scale_y", 1.0))
            a.Hr, a.Wr = int(s.get("Hr", H)), int(s.get("Wr", W))
            a.flip_h = int(bool(s.get("flip_h", 0)))
            a.y0, a.x0 = int(s.get("y0", 0)), int(s.get("x0", 0))
        _lib.check(lib.mpf_augment_sparse_pairs(arr, B, H, W, h, w, _ptr(out["image1"]), _ptr(out["image2"]), _ptr(out["flow"]), _ptr(out["valid"]),
                                                _stream()), "mpf_augment_sparse_pairs")
    return out


PHOTO_OPS = ("brightness", "contrast", "saturation", "hue")     # op codes 0..3 of MpfPhotoJitter.order


def photometric_pairs(samples, out=None):
    """RAFT's photometric augmentation (ColorJitter, then the eraser on image 2) of a batch of u8 pairs (mpf_photometric_pairs), on the current
    stream.  samples: B dicts with src / dst (u8 [H,W,3] BGR on the device), joint (1: one jitter for both frames, one contrast mean over
    both), jitter (one dict per parameter set - two when joint is 0: order (op names or codes 0..3, applied in that order), brightness,
    contrast, saturation (factors, default 1), hue_shift (int, default 0)) and rects (up to two (x0, y0, dx, dy)).
    -> dict(src, dst) u8 [B,H,W,3] BGR; `out` may carry these two tensors."""
    lib = _lib.load()
    B = len(samples)
    if B < 1:
        raise ValueError("photometric_pairs: no samples")
    src0 = _dev(samples[0]["src"], "src", torch.uint8)
    H, W, _ = src0.shape
    dev = src0.device
    if out is None:
        out = dict(src=torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev), dst=torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev))
    for k in ("src", "dst"):
        t = out[k]
        if tuple(t.shape) != (B, H, W, 3) or t.dtype != torch.uint8 or not t.is_contiguous() or t.device != dev:
            raise ValueError("photometric_pairs: out[%r] must be a contiguous u8 (%d, %d, %d, 3) tensor on %s" % (k, B, H, W, dev))
    arr = (_lib.MpfPhotoSample * B)()
    keep = []
    with torch.cuda.device(dev):
        for b, s in enumerate(samples):
            src, dst = _dev(s["src"], "src", torch.uint8), _dev(s["dst"], "dst", torch.uint8)
            if tuple(src.shape) != (H, W, 3) or tuple(dst.shape) != (H, W, 3):
                raise ValueError("photometric_pairs: sample %d: src / dst must be [%d,%d,3]" % (b, H, W))
            keep += [src, dst]
            a = arr[b]
            a.src, a.dst, a.src_out, a.dst_out = src.data_ptr(), dst.data_ptr(), out["src"][b].data_ptr(), out["dst"][b].data_ptr()
            a.joint = int(s.get("joint", 1))
            jit = list(s.get("jitter", ()))
            if len(jit) > 2:
                raise ValueError("photometric_pairs: sample %d: at most two jitter parameter sets" % b)
            for j, p in enumerate(jit):
                t = a.jitter[j]
                order = [PHOTO_OPS.index(o) if isinstance(o, str) else int(o) for o in p.get("order", ())]
                if len(order) > 4:
                    raise ValueError("photometric_pairs: sample %d: more than four ops" % b)
                t.n_ops = len(order)
                for k, o in enumerate(order):
                    t.order[k] = o
                t.brightness, t.contrast, t.saturation = (float(p.get(n, 1.0)) for n in PHOTO_OPS[:3])
                t.hue_shift = int(p.get("hue_shift", 0))
            for j in range(len(jit), 2):
                a.jitter[j].brightness = a.jitter[j].contrast = a.jitter[j].saturation = 1.0
            rects = list(s.get("rects", ()))
            if len(rects) > 2:
                raise ValueError("photometric_pairs: sample %d: at most two rectangles" % b)
            a.n_rect = len(rects)
            for k, r in enumerate(rects):
                for c in range(4):
                    a.rect[k][c] = int(r[c])
        ws = torch.empty(int(lib.mpf_photometric_workspace(B)), dtype=torch.uint8, device=dev)
        _lib.check(lib.mpf_photometric_pairs(arr, B, H, W, _ptr(ws), ws.numel(), _stream()), "mpf_photometric_pairs")
    return out


def _corr_args(fmap1_nhwc, f2_levels_nhwc, coords, radius, scale, who, plain=False, out=None, out_name="out"):
    """MpfCorrArgs of an on-demand lookup, with `out` (or grad_out) if the caller has one, and the levels as a list"""
    f1 = check_tensor(fmap1_nhwc, "fmap1_nhwc", who, 4, "[B,H,W,C]")
    B, H, W, C = f1.shape
    levels = list(f2_levels_nhwc)
    check_pyramid(who, None, None, len(levels))
    co = check_tensor(coords, "coords", who, (B, 2, H, W), "[B,2,H,W] = %s" % ((B, 2, H, W),))
    a = _lib.MpfCorrArgs()
    a.fmap1, a.coords = f1.data_ptr(), co.data_ptr()
    a.B, a.C, a.H, a.W = B, C, H, W
    tensors = dict(fmap1_nhwc=f1, coords=co)
    for i, t in enumerate(levels):
        tensors["f2_levels_nhwc[%d]" % i] = check_tensor(t, "f2_levels_nhwc[%d]" % i, who, (B, None, None, C), "[B,H_i,W_i,C] for fmap1_nhwc %s" % (tuple(f1.shape),))
        a.f2[i], a.Hl[i], a.Wl[i] = t.data_ptr(), t.shape[1], t.shape[2]
    a.radius, a.levels = int(radius), len(levels)
    a.scale = 1.0 / float(torch.sqrt(torch.tensor(C).float())) if scale is None else float(scale)       # RAFT divides by the fp32 sqrt(C)
    a.plain = int(bool(plain))
    if out is not None:
        rd = 2 * a.radius + 1
        tensors[out_name] = check_tensor(out, out_name, who, (B, len(levels) * rd * rd, H, W))
        a.out = out.data_ptr()
    check_devices(who, tensors)
    return a, levels


@_on_device
def corr_lookup(fmap1_nhwc, f2_levels_nhwc, coords, radius, out=None, scale=None, plain=False):
    """mpf_corr_lookup: RAFT's on-demand correlation lookup (AlternateCorrBlock / alt_cuda_corr), every level in one launch.
    fmap1_nhwc [B,H,W,C], f2_levels_nhwc: level i of fmap2's avg_pool2d pyramid as [B,H_i,W_i,C], coords [B,2,H,W] (x, y; any value is
    legal, non-finite ones give 0) -> [B, L*(2r+1)^2, H, W], scaled by `scale` (default 1/sqrt(C)).  float32, contiguous, on the GPU, or
    MpiFlowHipError.  `plain`: the one-thread-per-entry form of the kernel (yardstick of tools/bench_corr.py).  Asynchronous on the current stream."""
    a, levels = _corr_args(fmap1_nhwc, f2_levels_nhwc, coords, radius, scale, "corr_lookup", plain, out)
    lib = _lib.load()
    if out is None:
        rd = 2 * a.radius + 1
        out = torch.empty((a.B, len(levels) * rd * rd, a.H, a.W), dtype=_f32, device=fmap1_nhwc.device)
        a.out = out.data_ptr()
    _lib.check(lib.mpf_corr_lookup(ctypes.byref(a), _stream()), "mpf_corr_lookup")
    return out


@_on_device
def corr_lookup_backward(fmap1_nhwc, f2_levels_nhwc, coords, grad_out, radius, scale=None):
    """mpf_corr_lookup_backward: the cotangent grad_out [B, L*(2r+1)^2, H, W] of corr_lookup -> (grad_fmap1_nhwc, [grad_f2_i_nhwc per level]).
    grad_fmap1 is a per-pixel sum (bit-identical from run to run); the levels' gradients are scattered with fp32 atomics (last bits vary).
    There is no gradient for coords.  Asynchronous on the current stream."""
    if grad_out is None:
        raise _lib.MpiFlowHipError("corr_lookup_backward: grad_out must be a torch.Tensor (got NoneType)")
    a, levels = _corr_args(fmap1_nhwc, f2_levels_nhwc, coords, radius, scale, "corr_lookup_backward", out=grad_out, out_name="grad_out")
    lib = _lib.load()
    g1 = torch.empty_like(fmap1_nhwc)
    g2 = [torch.zeros_like(t) for t in levels]
    a.grad_fmap1 = g1.data_ptr()
    for i, t in enumerate(g2):
        a.grad_f2[i] = t.data_ptr()
    _lib.check(lib.mpf_corr_lookup_backward(ctypes.byref(a), _stream()), "mpf_corr_lookup_backward")
    return g1, g2


def _corr_volume_rows(who, N, H, W):
    """level 0 [N, H, W] of an all-pairs pyramid holds N = B * H * W rows"""
    if N == 0 or N % (H * W):
        raise _lib.MpiFlowHipError("%s: level 0 %s must hold B * H * W rows of H x W" % (who, (N, H, W)))


def _corr_volume_args(levels, who, norm=None, coords=None, radius=None, out=None, out_name="out"):
    """MpfCorrVolumeArgs for a pyramid (or its gradient): levels[i] [N, H >> i, W >> i] with N = B*H*W rows, for a pyramid call (norm) or a
    lookup call (coords [B,2,H,W], radius, and out / grad_out [B, L*(2r+1)^2, H, W] if the caller has one)."""
    levels = list(levels)
    N, H, W = check_tensor(levels[0], "levels[0]", who, 3).shape if levels else (0, 0, 0)
    check_pyramid(who, H, W, len(levels), radius)               # an empty list is refused here
    _corr_volume_rows(who, N, H, W)
    a = _lib.MpfCorrVolumeArgs()
    tensors = {}
    for i, t in enumerate(levels):
        tensors["levels[%d]" % i] = check_tensor(t, "levels[%d]" % i, who, (N, H >> i, W >> i),
                                                 "%s, level %d of a pooled pyramid of %d rows of %d x %d" % ((N, H >> i, W >> i), i, N, H, W))
        a.level[i], a.Hl[i], a.Wl[i] = t.data_ptr(), H >> i, W >> i
    a.B, a.H, a.W, a.levels = N // (H * W), H, W, len(levels)
    if coords is None:
        a.norm = float(norm)
    else:
        co = tensors["coords"] = check_tensor(coords, "coords", who, (a.B, 2, H, W), "[B,2,H,W] = %s for %d rows of %d x %d" % ((a.B, 2, H, W), N, H, W))
        a.coords, a.radius = co.data_ptr(), int(radius)
        if out is not None:
            rd = 2 * a.radius + 1
            tensors[out_name] = check_tensor(out, out_name, who, (a.B, len(levels) * rd * rd, H, W))
            a.out = out.data_ptr()
    check_devices(who, tensors)
    return a, levels


@_on_device
def corr_pyramid(raw, num_levels, norm):
    """mpf_corr_pyramid: raw [B*H*W, H, W], the product fmap1^T fmap2 (row p: query pixel p against all of frame 2) -> the list of num_levels
    levels [B*H*W, H >> i, W >> i] of CorrBlock's pyramid.  Level 0 IS raw, divided by `norm` (RAFT: sqrt(C) in float32) in place; the other
    levels are new.  float32, contiguous, on the GPU, or MpiFlowHipError.  Asynchronous on the current stream."""
    who = "corr_pyramid"
    N, H, W = check_tensor(raw, "raw", who, 3).shape
    check_pyramid(who, H, W, num_levels)
    _corr_volume_rows(who, N, H, W)
    check_devices(who, dict(raw=raw))
    levels = [raw] + [torch.empty((N, H >> i, W >> i), dtype=_f32, device=raw.device) for i in range(1, int(num_levels))]
    a, levels = _corr_volume_args(levels, who, norm=norm)
    _lib.check(_lib.load().mpf_corr_pyramid(ctypes.byref(a), _stream()), "mpf_corr_pyramid")
    return levels


@_on_device
def corr_volume_lookup(levels, coords, radius, out=None):
    """mpf_corr_volume_lookup: CorrBlock's lookup, every level in one launch.  levels: corr_pyramid's result, coords [B,2,H,W] (x, y; any value
    is legal, non-finite ones give 0) -> [B, L*(2r+1)^2, H, W].  Asynchronous on the current stream."""
    a, levels = _corr_volume_args(levels, "corr_volume_lookup", coords=coords, radius=radius, out=out)
    if out is None:
        rd = 2 * int(radius) + 1
        out = torch.empty((a.B, len(levels) * rd * rd, a.H, a.W), dtype=_f32, device=coords.device)
        a.out = out.data_ptr()
    _lib.check(_lib.load().mpf_corr_volume_lookup(ctypes.byref(a), _stream()), "mpf_corr_volume_lookup")
    return out


@_on_device
def corr_volume_lookup_backward(grad_levels, coords, grad_out, radius):
    """mpf_corr_volume_lookup_backward: ADDS the gradient of one lookup with the cotangent grad_out [B, L*(2r+1)^2, H, W] into grad_levels, a
    gradient pyramid shaped like corr_pyramid's result that the caller zeroed once and may share between lookups.  No atomics: bit-identical
    from run to run.  Returns grad_levels.  Asynchronous on the current stream."""
    if grad_out is None:
        raise _lib.MpiFlowHipError("corr_volume_lookup_backward: grad_out must be a torch.Tensor (got NoneType)")
    a, grad_levels = _corr_volume_args(grad_levels, "corr_volume_lookup_backward", coords=coords, radius=radius, out=grad_out, out_name="grad_out")
    _lib.check(_lib.load().mpf_corr_volume_lookup_backward(ctypes.byref(a), _stream()), "mpf_corr_volume_lookup_backward")
    return grad_levels


@_on_device
def corr_pyramid_backward(grad_levels, norm):
    """mpf_corr_pyramid_backward: folds a gradient pyramid into the gradient of the raw product, in place in grad_levels[0], which it returns
    ([B*H*W, H, W]); the other levels are only read.  Asynchronous on the current stream."""
    a, grad_levels = _corr_volume_args(grad_levels, "corr_pyramid_backward", norm=norm)
    _lib.check(_lib.load().mpf_corr_pyramid_backward(ctypes.byref(a), _stream()), "mpf_corr_pyramid_backward")
    return grad_levels[0]


def _up_args(flow, mask, who):
    """MpfUpsampleArgs with flow [N,2,H,W] and mask [N,576,H,W]; the caller checks its other tensors against N, H, W, then the devices"""
    f = check_tensor(flow, "flow", who, (None, 2, None, None))
    N, _, H, W = f.shape
    m = check_tensor(mask, "mask", who, (N, 576, H, W))
    a = _lib.MpfUpsampleArgs()
    a.flow, a.mask, a.N, a.H, a.W = f.data_ptr(), m.data_ptr(), N, H, W
    return a


def _up_loss_args(flow, mask, flow_gt, valid, max_flow, who, **more):
    a = _up_args(flow, mask, who)
    gt = check_tensor(flow_gt, "flow_gt", who, (a.N, 2, 8 * a.H, 8 * a.W))
    va = check_tensor(valid, "valid", who, (a.N, 8 * a.H, 8 * a.W))
    check_devices(who, dict(flow=flow, mask=mask, flow_gt=gt, valid=va, **more))
    a.flow_gt, a.valid, a.max_flow = gt.data_ptr(), va.data_ptr(), float(max_flow)
    return a


def _up_workspace(lib, a, backward, dev):
    ws = torch.empty(int(lib.mpf_upsample_workspace(a.N, a.H, a.W, backward)) // 8, dtype=torch.float64, device=dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    return ws


@_on_device
def upsample_flow(flow, mask):
    """mpf_upsample_flow: RAFT's convex upsampling.  flow [N,2,H,W], mask [N,576,H,W] -> [N,2,8H,8W]: per fine pixel the softmax over the mask's
    9 taps blends the 3 x 3 neighbourhood of 8 * flow.  float32, contiguous, on the GPU, or MpiFlowHipError.  Asynchronous on the current stream."""
    a = _up_args(flow, mask, "upsample_flow")
    check_devices("upsample_flow", dict(flow=flow, mask=mask))
    out = torch.empty((a.N, 2, 8 * a.H, 8 * a.W), dtype=_f32, device=flow.device)
    a.out = out.data_ptr()
    _lib.check(_lib.load().mpf_upsample_flow(ctypes.byref(a), _stream()), "mpf_upsample_flow")
    return out


@_on_device
def upsample_flow_backward(flow, mask, grad_out):
    """mpf_upsample_flow_backward: the cotangent grad_out [N,2,8H,8W] of upsample_flow -> (grad_flow, grad_mask); the softmax is recomputed, no
    atomics: bit-identical from run to run.  Asynchronous on the current stream."""
    who = "upsample_flow_backward"
    a = _up_args(flow, mask, who)
    g = check_tensor(grad_out, "grad_out", who, (a.N, 2, 8 * a.H, 8 * a.W))
    check_devices(who, dict(flow=flow, mask=mask, grad_out=g))
    lib = _lib.load()
    gf, gm = torch.empty_like(flow), torch.empty_like(mask)
    ws = _up_workspace(lib, a, 1, flow.device)
    a.out, a.grad_flow, a.grad_mask = g.data_ptr(), gf.data_ptr(), gm.data_ptr()
    _lib.check(lib.mpf_upsample_flow_backward(ctypes.byref(a), _stream()), "mpf_upsample_flow_backward")
    del ws
    return gf, gm


@_on_device
def flow_loss_term(flow, mask, flow_gt, valid, max_flow=400, metrics=False):
    """mpf_flow_loss_term: (v * |upsample_flow(flow, mask) - flow_gt|).mean() as a 0-d device tensor without forming the prediction;
    v = (valid >= 0.5) & (|flow_gt| < max_flow).  flow_gt [N,2,8H,8W], valid [N,8H,8W].  With metrics=True also a float64 device tensor of five
    accumulators of this prediction: sum of epe over v, counts of epe < 1, < 3, < 5, count of v.  -> (term, accumulators or None).  Asynchronous."""
    a = _up_loss_args(flow, mask, flow_gt, valid, max_flow, "flow_loss_term")
    lib = _lib.load()
    term = torch.empty((), dtype=_f32, device=flow.device)
    acc = torch.empty(5, dtype=torch.float64, device=flow.device) if metrics else None
    ws = _up_workspace(lib, a, 0, flow.device)
    a.term, a.metrics = term.data_ptr(), (acc.data_ptr() if metrics else None)
    _lib.check(lib.mpf_flow_loss_term(ctypes.byref(a), _stream()), "mpf_flow_loss_term")
    del ws
    return term, acc


@_on_device
def flow_loss_term_backward(flow, mask, flow_gt, valid, g, max_flow=400):
    """mpf_flow_loss_term_backward: g, a float32 scalar ON THE DEVICE (the gradient reaching the term; the kernel reads it, the host does not)
    -> (grad_flow, grad_mask) of flow_loss_term.  Bit-identical from run to run.  Asynchronous on the current stream."""
    g = check_tensor(g, "g", "flow_loss_term_backward", ())
    a = _up_loss_args(flow, mask, flow_gt, valid, max_flow, "flow_loss_term_backward", g=g)
    lib = _lib.load()
    gf, gm = torch.empty_like(flow), torch.empty_like(mask)
    ws = _up_workspace(lib, a, 1, flow.device)
    a.g, a.grad_flow, a.grad_mask = g.data_ptr(), gf.data_ptr(), gm.data_ptr()
    _lib.check(lib.mpf_flow_loss_term_backward(ctypes.byref(a), _stream()), "mpf_flow_loss_term_backward")
    del ws
    return gf, gm


def _up8_loss_args(flow, flow_gt, valid, max_flow, who, **more):
    """MpfUpsampleArgs of the bilinear loss calls: flow [N,2,H,W], flow_gt [N,2,8H,8W], valid [N,8H,8W]; mask and grad_mask stay NULL"""
    f = check_tensor(flow, "flow", who, (None, 2, None, None))
    N, _, H, W = f.shape
    gt = check_tensor(flow_gt, "flow_gt", who, (N, 2, 8 * H, 8 * W))
    va = check_tensor(valid, "valid", who, (N, 8 * H, 8 * W))
    check_devices(who, dict(flow=f, flow_gt=gt, valid=va, **more))
    a = _lib.MpfUpsampleArgs()
    a.flow, a.N, a.H, a.W = f.data_ptr(), N, H, W
    a.flow_gt, a.valid, a.max_flow = gt.data_ptr(), va.data_ptr(), float(max_flow)
    return a


@_on_device
def upflow8_loss_term(flow, flow_gt, valid, max_flow=400, metrics=False):
    """mpf_upflow8_loss_term: (v * |upflow8(flow) - flow_gt|).mean() as a 0-d device tensor without forming the prediction (the small model's
    loss term); v = (valid >= 0.5) & (|flow_gt| < max_flow).  flow [N,2,H,W], flow_gt [N,2,8H,8W], valid [N,8H,8W].  With metrics=True also the
    five float64 accumulators of flow_loss_term.  -> (term, accumulators or None).  Asynchronous on the current stream."""
    a = _up8_loss_args(flow, flow_gt, valid, max_flow, "upflow8_loss_term")
    lib = _lib.load()
    term = torch.empty((), dtype=_f32, device=flow.device)
    acc = torch.empty(5, dtype=torch.float64, device=flow.device) if metrics else None
    ws = torch.empty(int(lib.mpf_upflow8_loss_workspace(a.N, a.H, a.W, 0)) // 8, dtype=torch.float64, device=flow.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    a.term, a.metrics = term.data_ptr(), (acc.data_ptr() if metrics else None)
    _lib.check(lib.mpf_upflow8_loss_term(ctypes.byref(a), _stream()), "mpf_upflow8_loss_term")
    del ws
    return term, acc


@_on_device
def upflow8_loss_term_backward(flow, flow_gt, valid, g, max_flow=400):
    """mpf_upflow8_loss_term_backward: g, a float32 scalar ON THE DEVICE (the gradient reaching the term; the kernel reads it, the host does
    not) -> grad_flow [N,2,H,W] of upflow8_loss_term.  The prediction is recomputed; a gather, no atomics, no workspace: bit-identical from
    run to run.  Asynchronous on the current stream."""
    g = check_tensor(g, "g", "upflow8_loss_term_backward", ())
    a = _up8_loss_args(flow, flow_gt, valid, max_flow, "upflow8_loss_term_backward", g=g)
    gf = torch.empty_like(flow)
    a.g, a.grad_flow = g.data_ptr(), gf.data_ptr()
    _lib.check(_lib.load().mpf_upflow8_loss_term_backward(ctypes.byref(a), _stream()), "mpf_upflow8_loss_term_backward")
    return gf


def _gru_slices(dst, terms, name, who, h, limit, tensors):
    """terms: (tensor [B,channels,H,W], channel offset) pairs or None (absent) -> fills the MpfGruTerm array `dst`, adds the tensors by name
    to `tensors` (for the device check that ends the call), returns the count"""
    terms = list(terms)
    if not 1 <= len(terms) <= limit:
        raise _lib.MpiFlowHipError("%s: %s takes 1..%d slices (got %d)" % (who, name, limit, len(terms)))
    B, C, H, W = h.shape
    for k, term in enumerate(terms):
        if term is None:
            continue
        t, off = term
        t = tensors["%s[%d]" % (name, k)] = check_tensor(t, "%s[%d]" % (name, k), who, (B, None, H, W))
        if off < 0 or off + C > t.shape[1]:
            raise _lib.MpiFlowHipError("%s: %s[%d]: channels [%d, %d) are not inside its %d channels" % (who, name, k, off, off + C, t.shape[1]))
        dst[k].p, dst[k].channels, dst[k].offset = t.data_ptr(), t.shape[1], int(off)
    return len(terms)


def _gru_args(h, who):
    """(MpfGruArgs, {name: tensor} of the call so far)"""
    h = check_tensor(h, "h", who, 4, "[B,C,H,W]")
    a = _lib.MpfGruArgs()
    a.h = h.data_ptr()
    a.B, a.C, a.H, a.W = h.shape
    return a, dict(h=h)


@_on_device
def gru_reset(h, r_terms):
    """mpf_gru_reset: rh = sigmoid(sum of r_terms) * h.  h [B,C,H,W]; a term is (tensor [B,channels,H,W], channel offset) - the slice
    [offset, offset + C) read in place - or None.  float32, contiguous, on the GPU, or MpiFlowHipError.  Asynchronous on the current stream."""
    who = "gru_reset"
    a, tensors = _gru_args(h, who)
    a.nr = _gru_slices(a.r, r_terms, "r_terms", who, h, _lib.GRU_MAX_TERMS, tensors)
    check_devices(who, tensors)
    out = torch.empty_like(h)
    a.out = out.data_ptr()
    _lib.check(_lib.load().mpf_gru_reset(ctypes.byref(a), _stream()), "mpf_gru_reset")
    return out


@_on_device
def gru_update(h, z_terms, q_terms):
    """mpf_gru_update: h' = (1 - z) * h + z * q with z = sigmoid(sum of z_terms), q = tanh(sum of q_terms); terms as in gru_reset."""
    who = "gru_update"
    a, tensors = _gru_args(h, who)
    a.nz = _gru_slices(a.z, z_terms, "z_terms", who, h, _lib.GRU_MAX_TERMS, tensors)
    a.nq = _gru_slices(a.q, q_terms, "q_terms", who, h, _lib.GRU_MAX_TERMS, tensors)
    check_devices(who, tensors)
    out = torch.empty_like(h)
    a.out = out.data_ptr()
    _lib.check(_lib.load().mpf_gru_update(ctypes.byref(a), _stream()), "mpf_gru_update")
    return out


@_on_device
def gru_update_backward(grad_out, h, z_terms, q_terms, dz, dq):
    """mpf_gru_update_backward: the cotangent grad_out of gru_update's h' -> d h = grad_out * (1 - z), returned; d pre_z and d pre_q are WRITTEN
    into the slices dz and dq: one or two (tensor, channel offset) destinations each.  z and q are recomputed from the terms."""
    who = "gru_update_backward"
    a, tensors = _gru_args(h, who)
    g = tensors["grad_out"] = check_tensor(grad_out, "grad_out", who, tuple(h.shape))
    a.nz = _gru_slices(a.z, z_terms, "z_terms", who, h, _lib.GRU_MAX_TERMS, tensors)
    a.nq = _gru_slices(a.q, q_terms, "q_terms", who, h, _lib.GRU_MAX_TERMS, tensors)
    _gru_slices(a.dz, dz, "dz", who, h, 2, tensors)
    _gru_slices(a.dq, dq, "dq", who, h, 2, tensors)
    check_devices(who, tensors)
    dh = torch.empty_like(h)
    a.g, a.dh = g.data_ptr(), dh.data_ptr()
    _lib.check(_lib.load().mpf_gru_update_backward(ctypes.byref(a), _stream()), "mpf_gru_update_backward")
    return dh


@_on_device
def gru_reset_backward(grad_out, h, r_terms, dr, dh=None):
    """mpf_gru_reset_backward: the cotangent grad_out of gru_reset's rh -> d pre_r WRITTEN into the slices dr (one or two destinations);
    d h = grad_out * r is ADDED into `dh` when one is given, otherwise written to a fresh tensor.  Returns dh."""
    who = "gru_reset_backward"
    a, tensors = _gru_args(h, who)
    g = tensors["grad_out"] = check_tensor(grad_out, "grad_out", who, tuple(h.shape))
    a.nr = _gru_slices(a.r, r_terms, "r_terms", who, h, _lib.GRU_MAX_TERMS, tensors)
    _gru_slices(a.dr, dr, "dr", who, h, 2, tensors)
    a.accumulate = int(dh is not None)
    if dh is not None:
        tensors["dh"] = check_tensor(dh, "dh", who, tuple(h.shape))
    check_devices(who, tensors)
    dh = torch.empty_like(h) if dh is None else dh
    a.g, a.dh = g.data_ptr(), dh.data_ptr()
    _lib.check(_lib.load().mpf_gru_reset_backward(ctypes.byref(a), _stream()), "mpf_gru_reset_backward")
    return dh


NORM_MODES = {"none": _lib.NORM_NONE, "instance": _lib.NORM_INSTANCE, "batch_train": _lib.NORM_BATCH_TRAIN, "batch_eval": _lib.NORM_BATCH_EVAL,
              "group": _lib.NORM_GROUP}
_NORM_STATS = ("instance", "batch_train", "group")


class NormTerm:
    """One term of the encoders' norm / ReLU chain: a convolution output x [N,C,H,W] with a norm mode ('none', 'instance', 'batch_train',
    'batch_eval', 'group'), optional weight / bias [C], `groups` for 'group', running_mean / running_var [C] for 'batch_eval'.
    norm_act fills mean, rstd and var (one entry per statistic set; None for 'none' and 'batch_eval'), which norm_act_backward reads;
    `partials` may hold what norm_stats returned for x (otherwise norm_act computes it)."""

    def __init__(self, x, mode, weight=None, bias=None, groups=1, running_mean=None, running_var=None, partials=None):
        self.x, self.mode, self.weight, self.bias, self.groups = x, mode, weight, bias, groups
        self.running_mean, self.running_var, self.partials = running_mean, running_var, partials
        self.mean = self.rstd = self.var = None

    def sets(self):
        N, C = self.x.shape[:2]
        return {"instance": N * C, "batch_train": C, "group": N * self.groups}.get(self.mode, 0)


def norm_default_chunks(planes, hw):
    """how many workgroups share a plane: enough for about 2048 workgroups in all, none with fewer than 4096 elements, 64 at the most"""
    return max(1, min(-(-2048 // planes), hw // 4096, 64))


def _norm_check(term, name, who, shape=4):
    """a term's own checks: type, x, mode, parameters, more than a single element per statistic set"""
    if not isinstance(term, NormTerm):
        raise _lib.MpiFlowHipError("%s: %s must be an ops.NormTerm (got %s)" % (who, name, type(term).__name__))
    x = check_tensor(term.x, name + ".x", who, shape)
    if term.mode not in NORM_MODES:
        raise _lib.MpiFlowHipError("%s: %s.mode must be one of %s (got %r)" % (who, name, ", ".join(sorted(NORM_MODES)), term.mode))
    N, C, H, W = x.shape
    if term.mode == "group" and (not isinstance(term.groups, int) or term.groups < 1 or C % term.groups):
        raise _lib.MpiFlowHipError("%s: %s.groups must divide the %d channels (got %r)" % (who, name, C, term.groups))
    per_set = {"instance": H * W, "batch_train": N * H * W}.get(term.mode)
    if per_set == 1:
        raise _lib.MpiFlowHipError("%s: %s: '%s' statistics over a single value per %s (shape %s) have no variance; use a larger input or "
                                   "put the module in eval mode with running statistics" % (who, name, term.mode, "plane" if term.mode == "instance" else "channel", tuple(x.shape)))
    vecs = [("weight", term.weight), ("bias", term.bias)]
    if term.mode == "batch_eval":
        if term.running_mean is None or term.running_var is None:
            raise _lib.MpiFlowHipError("%s: %s: 'batch_eval' needs running_mean and running_var" % (who, name))
        vecs += [("running_mean", term.running_mean), ("running_var", term.running_var)]
    for vname, v in vecs:
        if v is None:
            continue
        if not isinstance(v, torch.Tensor) or v.dtype != _f32 or tuple(v.shape) != (C,) or not v.is_contiguous() or v.device != x.device:
            raise _lib.MpiFlowHipError("%s: %s.%s must be a contiguous float32 tensor [%d] on %s" % (who, name, vname, C, x.device))
    return x


def _norm_fill(ct, term):
    ct.x, ct.mode, ct.groups = term.x.data_ptr(), NORM_MODES[term.mode], int(term.groups)
    if term.mode != "none":
        for cname, v in (("weight", term.weight), ("bias", term.bias), ("running_mean", term.running_mean), ("running_var", term.running_var),
                         ("partials", term.partials), ("mean", term.mean), ("rstd", term.rstd), ("var", term.var)):
            setattr(ct, cname, None if v is None else v.data_ptr())


def _norm_args(term, residual, who, chunks, **like):
    """(MpfNormArgs, x, residual term or None, residual tensor or None): everything checked - `like`: further tensors of term.x's shape, by
    name - nothing allocated"""
    x = _norm_check(term, "term", who)
    N, C, H, W = x.shape
    a = _lib.MpfNormArgs()
    a.N, a.C, a.H, a.W = N, C, H, W
    tensors = {"term.x": x}
    rt = res = None
    if isinstance(residual, NormTerm):
        rt = residual
        tensors["residual.x"] = _norm_check(rt, "residual", who, tuple(x.shape))
    elif residual is not None:
        res = tensors["residual"] = check_tensor(residual, "residual", who, tuple(x.shape))
        a.res = res.data_ptr()
    for name, t in like.items():
        tensors[name] = check_tensor(t, name, who, tuple(x.shape))
    if chunks is None:
        chunks = norm_default_chunks(N * C, H * W)
    if not isinstance(chunks, int) or not 1 <= chunks <= _lib.NORM_MAX_CHUNKS:
        raise _lib.MpiFlowHipError("%s: chunks must be an integer in 1..%d (got %r)" % (who, _lib.NORM_MAX_CHUNKS, chunks))
    a.chunks = chunks
    check_devices(who, tensors)
    return a, x, rt, res


@_on_device
def norm_stats(x, mode, groups=1, chunks=None):
    """mpf_norm_stats: float64 partials [N,C,chunks,2] = (mean, centred sum of squares) of every chunk of every plane of x, for a mode with statistics
    ('instance', 'batch_train', 'group').  chunks=None: norm_default_chunks.  Hand it to NormTerm(partials=...); norm_act then uses its chunks."""
    who = "norm_stats"
    if mode in NORM_MODES and mode not in _NORM_STATS:
        raise _lib.MpiFlowHipError("%s: mode '%s' has no statistics to compute" % (who, mode))
    term = NormTerm(x, mode, groups=groups)
    a, x, _, _ = _norm_args(term, None, who, chunks)
    lib = _lib.load()
    term.partials = torch.empty((x.shape[0], x.shape[1], a.chunks, 2), dtype=torch.float64, device=x.device)
    _norm_fill(a.y, term)
    _lib.check(lib.mpf_norm_stats(ctypes.byref(a), _stream()), "mpf_norm_stats")
    return term.partials


def _term_device(term):
    """the device argument that makes _on_device select a NormTerm's GPU (it looks at tensors and devices, not into terms)"""
    x = getattr(term, "x", None)
    return x.device if isinstance(x, torch.Tensor) and x.is_cuda else None


def norm_act(term, residual=None, chunks=None):
    """mpf_norm_act: out = relu(norm(term.x)), or with a residual - a tensor, or a NormTerm, normalised without a ReLU - out =
    relu(residual + relu(norm(term.x))).  Statistics a term lacks are computed first (one mpf_norm_stats launch for both terms); term.mean,
    .rstd and .var are filled, .partials dropped.  float32, contiguous, on the GPU, or MpiFlowHipError.  Asynchronous on the current stream."""
    return _norm_act(_term_device(term), term, residual, chunks)


@_on_device
def _norm_act(device, term, residual, chunks):
    who = "norm_act"
    given = [t.partials for t in (term, residual) if isinstance(t, NormTerm) and t.mode in _NORM_STATS and t.partials is not None]
    if given:
        if chunks is not None and chunks != given[0].shape[2]:
            raise _lib.MpiFlowHipError("%s: chunks=%r but the partials handed in were computed with %d" % (who, chunks, given[0].shape[2]))
        chunks = int(given[0].shape[2])
    a, x, rt, res = _norm_args(term, residual, who, chunks)
    lib = _lib.load()
    N, C = x.shape[:2]
    fresh = []
    for t in (term, rt):
        if t is None or t.mode not in _NORM_STATS:
            continue
        if t.partials is None:
            t.partials = torch.empty((N, C, a.chunks, 2), dtype=torch.float64, device=x.device)
            fresh.append(t)
        elif tuple(t.partials.shape) != (N, C, a.chunks, 2) or t.partials.dtype != torch.float64 or not t.partials.is_contiguous() or t.partials.device != x.device:
            raise _lib.MpiFlowHipError("%s: partials must be what norm_stats returned for this x with chunks=%d: float64 %s (got %s)"
                                       % (who, a.chunks, [N, C, a.chunks, 2], tuple(t.partials.shape)))
        stat = torch.empty((3, t.sets()), dtype=_f32, device=x.device)
        t.mean, t.rstd, t.var = stat[0], stat[1], stat[2]
    out = torch.empty_like(x)
    a.out = out.data_ptr()
    if fresh:
        s = _lib.MpfNormArgs()
        s.N, s.C, s.H, s.W, s.chunks = a.N, a.C, a.H, a.W, a.chunks
        _norm_fill(s.y, fresh[0])
        if len(fresh) > 1:
            _norm_fill(s.r, fresh[1])
        _lib.check(lib.mpf_norm_stats(ctypes.byref(s), _stream()), "mpf_norm_stats")
    _norm_fill(a.y, term)
    if rt is not None:
        _norm_fill(a.r, rt)
    _lib.check(lib.mpf_norm_act(ctypes.byref(a), _stream()), "mpf_norm_act")
    for t in (term, rt):
        if t is not None:
            t.partials = None
    return out


def norm_act_backward(grad_out, term, residual=None, chunks=None, dres=None, param_grads=True):
    """mpf_norm_act_backward_reduce + mpf_norm_act_backward: the cotangent of norm_act's out -> (dx, dweight, dbias, dresidual) for the same
    term and residual, whose mean / rstd norm_act filled.  dresidual: the shortcut's gradient for a tensor residual - ADDED into `dres` when one
    is given, otherwise written to a fresh tensor - or (dx, dweight, dbias) of a NormTerm residual, or None.  dweight / dbias are None where the
    term has no weight / bias or param_grads is False ('batch_eval' then needs no reduce launch, like 'none').  Bit-identical from call to call."""
    return _norm_act_backward(_term_device(term), grad_out, term, residual, chunks, dres, param_grads)


@_on_device
def _norm_act_backward(device, grad_out, term, residual, chunks, dres, param_grads):
    who = "norm_act_backward"
    like = dict(grad_out=grad_out)
    if dres is not None and residual is not None and not isinstance(residual, NormTerm):
        like["dres"] = dres
    a, x, rt, res = _norm_args(term, residual, who, chunks, **like)
    lib = _lib.load()
    N, C = x.shape[:2]
    a.g = grad_out.data_ptr()
    keep, results = [], []
    for t, ct in ((term, a.y), (rt, a.r)):
        if t is None:
            continue
        if t.mode in _NORM_STATS and (t.mean is None or t.rstd is None):
            raise _lib.MpiFlowHipError("%s: the term has no mean / rstd: norm_act fills them in the forward pass" % who)
        _norm_fill(ct, t)
        dx = torch.empty_like(x)
        dw = torch.empty_like(t.weight) if param_grads and t.mode != "none" and t.weight is not None else None
        db = torch.empty_like(t.bias) if param_grads and t.mode != "none" and t.bias is not None else None
        ct.dx = dx.data_ptr()
        ct.dweight, ct.dbias = (None if dw is None else dw.data_ptr()), (None if db is None else db.data_ptr())
        if t.mode in _NORM_STATS or dw is not None or db is not None:
            gp = torch.empty((N, C, a.chunks, 2), dtype=torch.float64, device=x.device)
            ct.grad_partials = gp.data_ptr()
            keep.append(gp)
        results.append((dx, dw, db))
    if res is not None:
        a.accumulate = int(dres is not None)
        dres = torch.empty_like(x) if dres is None else dres
        a.dres = dres.data_ptr()
    if keep:
        _lib.check(lib.mpf_norm_act_backward_reduce(ctypes.byref(a), _stream()), "mpf_norm_act_backward_reduce")
    _lib.check(lib.mpf_norm_act_backward(ctypes.byref(a), _stream()), "mpf_norm_act_backward")
    del keep
    return results[0] + ((results[1] if rt is not None else dres),)


@_on_device
def raft_images(image1, image2):
    """mpf_raft_images: 2 * (x / 255) - 1 of both [N,3,H,W] image batches in one launch -> the [2N,3,H,W] batch RAFT's feature network takes
    (image1 first); its first N samples are what the context network takes.  A true fp32 division.  float32, contiguous, on the GPU, or
    MpiFlowHipError.  Asynchronous on the current stream."""
    who = "raft_images"
    im1 = check_tensor(image1, "image1", who, (None, 3, None, None))
    im2 = check_tensor(image2, "image2", who, tuple(im1.shape))
    check_devices(who, dict(image1=im1, image2=im2))
    N, _, H, W = im1.shape
    pair = torch.empty((2 * N, 3, H, W), dtype=_f32, device=im1.device)
    a = _lib.MpfRaftGlueArgs()
    a.image1, a.image2, a.pair, a.N, a.H, a.W = im1.data_ptr(), im2.data_ptr(), pair.data_ptr(), N, H, W
    _lib.check(_lib.load().mpf_raft_images(ctypes.byref(a), _stream()), "mpf_raft_images")
    return pair


def _split_args(net, inp, who):
    """MpfRaftGlueArgs with net [N,hdim,H,W] and inp [N,cdim,H,W]"""
    net = check_tensor(net, "net", who, 4, "[N,hdim,H,W]")
    N, hdim, H, W = net.shape
    inp = check_tensor(inp, "inp", who, (N, None, H, W))
    a = _lib.MpfRaftGlueArgs()
    a.net, a.inp, a.N, a.H, a.W, a.hdim, a.cdim = net.data_ptr(), inp.data_ptr(), N, H, W, hdim, inp.shape[1]
    return a


@_on_device
def context_split(cnet, hdim):
    """mpf_context_split: cnet [N,hdim+cdim,H,W] -> (tanh(cnet[:, :hdim]), relu(cnet[:, hdim:])), both contiguous, one launch."""
    who = "context_split"
    cnet = check_tensor(cnet, "cnet", who, 4, "[N,hdim+cdim,H,W]")
    N, C, H, W = cnet.shape
    if not 1 <= int(hdim) < C:
        raise _lib.MpiFlowHipError("%s: hdim must be 1..%d, fewer than cnet's channels (got %s for shape %s)" % (who, C - 1, hdim, tuple(cnet.shape)))
    check_devices(who, dict(cnet=cnet))
    net = torch.empty((N, int(hdim), H, W), dtype=_f32, device=cnet.device)
    inp = torch.empty((N, C - int(hdim), H, W), dtype=_f32, device=cnet.device)
    a = _split_args(net, inp, who)
    a.cnet = cnet.data_ptr()
    _lib.check(_lib.load().mpf_context_split(ctypes.byref(a), _stream()), "mpf_context_split")
    return net, inp


@_on_device
def context_split_backward(net, inp, g_net, g_inp):
    """mpf_context_split_backward: the cotangents of context_split's outputs -> grad_cnet [N,hdim+cdim,H,W], recomputed from the outputs
    themselves (1 - net^2; inp > 0) and written as one tensor."""
    who = "context_split_backward"
    a = _split_args(net, inp, who)
    g_net = check_tensor(g_net, "g_net", who, tuple(net.shape))
    g_inp = check_tensor(g_inp, "g_inp", who, tuple(inp.shape))
    check_devices(who, dict(net=net, inp=inp, g_net=g_net, g_inp=g_inp))
    grad = torch.empty((a.N, a.hdim + a.cdim, a.H, a.W), dtype=_f32, device=net.device)
    a.g_net, a.g_inp, a.grad_cnet = g_net.data_ptr(), g_inp.data_ptr(), grad.data_ptr()
    _lib.check(_lib.load().mpf_context_split_backward(ctypes.byref(a), _stream()), "mpf_context_split_backward")
    return grad


@_on_device
def upflow8(flow):
    """mpf_upflow8: RAFT's upflow8 (the small model's upsampling): flow [N,2,H,W] -> 8 * F.interpolate(flow, (8H, 8W), mode='bilinear',
    align_corners=True).  float32, contiguous, on the GPU, or MpiFlowHipError.  Asynchronous on the current stream."""
    who = "upflow8"
    flow = check_tensor(flow, "flow", who, (None, 2, None, None))
    check_devices(who, dict(flow=flow))
    N, _, H, W = flow.shape
    out = torch.empty((N, 2, 8 * H, 8 * W), dtype=_f32, device=flow.device)
    a = _lib.MpfRaftGlueArgs()
    a.flow, a.flow_up, a.N, a.H, a.W = flow.data_ptr(), out.data_ptr(), N, H, W
    _lib.check(_lib.load().mpf_upflow8(ctypes.byref(a), _stream()), "mpf_upflow8")
    return out


@_on_device
def upflow8_backward(grad_out):
    """mpf_upflow8_backward: the cotangent grad_out [N,2,8H,8W] of upflow8 -> grad_flow [N,2,H,W]; a gather, no atomics: bit-identical from
    run to run."""
    who = "upflow8_backward"
    g = check_tensor(grad_out, "grad_out", who, (None, 2, None, None))
    N, _, H8, W8 = g.shape
    if H8 % 8 or W8 % 8:
        raise _lib.MpiFlowHipError("%s: grad_out must be [N,2,8H,8W] (got shape %s)" % (who, tuple(g.shape)))
    check_devices(who, dict(grad_out=g))
    grad = torch.empty((N, 2, H8 // 8, W8 // 8), dtype=_f32, device=g.device)
    a = _lib.MpfRaftGlueArgs()
    a.g_up, a.grad_flow, a.N, a.H, a.W = g.data_ptr(), grad.data_ptr(), N, H8 // 8, W8 // 8
    _lib.check(_lib.load().mpf_upflow8_backward(ctypes.byref(a), _stream()), "mpf_upflow8_backward")
    return grad


def _eval_pad(a, pad, who):
    """InputPadder._pad = (left, right, top, bottom), each 0..7, into an MpfRaftEvalArgs"""
    try:
        sides = [operator.index(p) for p in pad]
    except TypeError:
        sides = []
    if len(sides) != 4 or not all(0 <= p <= 7 for p in sides):
        raise _lib.MpiFlowHipError("%s: pad must be (left, right, top, bottom), four integers 0..7, as InputPadder._pad (got %r)" % (who, pad))
    a.pad_left, a.pad_right, a.pad_top, a.pad_bottom = sides


@_on_device
def raft_images_padded(image1, image2, pad):
    """mpf_raft_images_padded: raft_images(F.pad(image1, pad, mode='replicate'), F.pad(image2, ...)) in one launch, bit for bit, without the
    padded images: [N,3,H,W] twice -> the [2N,3,Hp,Wp] batch RAFT's feature network takes (image1 first).  pad = (left, right, top, bottom),
    each 0..7 (InputPadder._pad); Hp = H + top + bottom and Wp = W + left + right must be multiples of 8.  float32, contiguous, on the GPU, or
    MpiFlowHipError.  Asynchronous on the current stream."""
    who = "raft_images_padded"
    im1 = check_tensor(image1, "image1", who, (None, 3, None, None))
    im2 = check_tensor(image2, "image2", who, tuple(im1.shape))
    a = _lib.MpfRaftEvalArgs()
    _eval_pad(a, pad, who)
    N, _, H, W = im1.shape
    Hp, Wp = H + a.pad_top + a.pad_bottom, W + a.pad_left + a.pad_right
    if Hp % 8 or Wp % 8:
        raise _lib.MpiFlowHipError("%s: the padded frame's H and W must be multiples of 8 (%d x %d with pad %s is %d x %d)" % (who, H, W, tuple(pad), Hp, Wp))
    check_devices(who, dict(image1=im1, image2=im2))
    pair = torch.empty((2 * N, 3, Hp, Wp), dtype=_f32, device=im1.device)
    a.image1, a.image2, a.pair, a.N, a.H, a.W = im1.data_ptr(), im2.data_ptr(), pair.data_ptr(), N, H, W
    _lib.check(_lib.load().mpf_raft_images_padded(ctypes.byref(a), _stream()), "mpf_raft_images_padded")
    return pair


def _crop_args(flow, mask, pad, out, who):
    """MpfRaftEvalArgs of the two cropped upsamplings and the window they write (`out`, or a new tensor); mask None: the bilinear one"""
    f = check_tensor(flow, "flow", who, (None, 2, None, None))
    N, _, H, W = f.shape
    tensors = dict(flow=f)
    if mask is not None:
        tensors["mask"] = check_tensor(mask, "mask", who, (N, 576, H, W))
    a = _lib.MpfRaftEvalArgs()
    _eval_pad(a, pad, who)
    Ho, Wo = 8 * H - a.pad_top - a.pad_bottom, 8 * W - a.pad_left - a.pad_right
    if Ho < 1 or Wo < 1:
        raise _lib.MpiFlowHipError("%s: pad %s leaves no window of the %d x %d prediction" % (who, tuple(pad), 8 * H, 8 * W))
    if out is not None:
        tensors["out"] = check_tensor(out, "out", who, (N, 2, Ho, Wo), "[N,2,8H-top-bottom,8W-left-right]")
    check_devices(who, tensors)
    if out is None:
        out = torch.empty((N, 2, Ho, Wo), dtype=_f32, device=f.device)
    a.flow, a.mask, a.flow_up, a.N, a.H, a.W = f.data_ptr(), (mask.data_ptr() if mask is not None else None), out.data_ptr(), N, H, W
    return a, out


@_on_device
def upsample_flow_crop(flow, mask, pad, out=None):
    """mpf_upsample_flow_crop: InputPadder.unpad(upsample_flow(flow, mask)) without the padded prediction, bit for bit: flow [N,2,H,W], mask
    [N,576,H,W], pad = (left, right, top, bottom), each 0..7 -> [N,2,8H-top-bottom,8W-left-right].  Mask channels of sub-positions outside the
    window are not read.  `out`: a contiguous tensor of that shape to write (any alignment).  Asynchronous on the current stream."""
    a, out = _crop_args(flow, mask, pad, out, "upsample_flow_crop")
    _lib.check(_lib.load().mpf_upsample_flow_crop(ctypes.byref(a), _stream()), "mpf_upsample_flow_crop")
    return out


@_on_device
def upflow8_crop(flow, pad, out=None):
    """mpf_upflow8_crop: InputPadder.unpad(upflow8(flow)) without the padded prediction, bit for bit (the small model's upsampling): flow
    [N,2,H,W], pad = (left, right, top, bottom), each 0..7 -> [N,2,8H-top-bottom,8W-left-right].  Asynchronous on the current stream."""
    a, out = _crop_args(flow, None, pad, out, "upflow8_crop")
    _lib.check(_lib.load().mpf_upflow8_crop(ctypes.byref(a), _stream()), "mpf_upflow8_crop")
    return out


@_on_device
def flow_metrics(flow_pr, flow_gt, valid=None):
    """mpf_flow_metrics: evaluate.py's per-frame sums in one launch pair: flow_pr, flow_gt [N,2,H,W], valid [N,H,W] or None (every pixel counts)
    -> a float64 device tensor [N,6]: per frame, over the pixels with valid >= 0.5, the sum of epe, their number, the numbers with epe < 1, < 3,
    < 5 and the number of outliers (epe > 3 and epe / |flow_gt| > 0.05).  No max_flow rule.  Bit-identical from run to run.  Asynchronous on the
    current stream: no host copy, no synchronisation."""
    who = "flow_metrics"
    pr = check_tensor(flow_pr, "flow_pr", who, (None, 2, None, None))
    N, _, H, W = pr.shape
    gt = check_tensor(flow_gt, "flow_gt", who, (N, 2, H, W))
    tensors = dict(flow_pr=pr, flow_gt=gt)
    if valid is not None:
        tensors["valid"] = check_tensor(valid, "valid", who, (N, H, W))
    check_devices(who, tensors)
    lib = _lib.load()
    acc = torch.empty((N, 6), dtype=torch.float64, device=pr.device)
    ws = torch.empty(int(lib.mpf_flow_metrics_workspace(N, H, W)) // 8, dtype=torch.float64, device=pr.device)
    a = _lib.MpfRaftEvalArgs()
    a.flow_pr, a.flow_gt, a.valid, a.metrics, a.N, a.H, a.W = pr.data_ptr(), gt.data_ptr(), (valid.data_ptr() if valid is not None else None), acc.data_ptr(), N, H, W
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    _lib.check(lib.mpf_flow_metrics(ctypes.byref(a), _stream()), "mpf_flow_metrics")
    del ws
    return acc


@_on_device
def forward_interpolate(flow, out=None):
    """mpf_forward_interpolate: RAFT's warm start (utils.forward_interpolate) per sample of flow [N,2,h,w] -> [N,2,h,w]: every pixel takes the
    flow vector of the nearest VALID source, a pixel pushed along its own flow to x1 = x0 + dx, y1 = y0 + dy with 0 < x1 < w and 0 < y1 < h
    (strict; NaN and inf drop out); squared distances in float64 without fused multiply-add, ties to the lowest flat index y0 * w + x0; a
    sample without a valid source gives zeros.  The selected vectors are copied, so the result is scipy's griddata(method='nearest') bit for
    bit wherever the nearest source is unique.  Brute force: h * w <= 65536 and N * h * w <= 2^22.  `out`: a contiguous tensor of flow's shape
    to write; it must not overlap flow.  Bit-identical from run to run.  Asynchronous on the current stream: no host copy, no synchronisation."""
    who = "forward_interpolate"
    f = check_tensor(flow, "flow", who, (None, 2, None, None), "[N,2,h,w]")
    N, _, h, w = f.shape
    tensors = dict(flow=f)
    if out is not None:
        tensors["out"] = check_tensor(out, "out", who, (N, 2, h, w), "[N,2,h,w] like flow")
    if N < 1 or h < 1 or w < 1:
        raise _lib.MpiFlowHipError("%s: flow must have at least one sample and one pixel (got shape %s)" % (who, tuple(f.shape)))
    if h * w > _lib.WARM_MAX_HW or N > 65535 or N * h * w > _lib.WARM_MAX_NHW:
        raise _lib.MpiFlowHipError("%s: the search is brute force: h * w must be at most %d, N at most 65535 and N * h * w at most %d (got shape %s)"
                                   % (who, _lib.WARM_MAX_HW, _lib.WARM_MAX_NHW, tuple(f.shape)))
    check_devices(who, tensors)
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(f)
    ws = torch.empty(int(lib.mpf_forward_interpolate_workspace(N, h, w)) // 8, dtype=torch.float64, device=f.device)
    a = _lib.MpfWarmStartArgs()
    a.flow, a.out, a.N, a.h, a.w = f.data_ptr(), out.data_ptr(), N, h, w
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    _lib.check(lib.mpf_forward_interpolate(ctypes.byref(a), _stream()), "mpf_forward_interpolate")
    del ws
    return out


def _mesh_limits(who, B, h, w):
    if B < 1 or h < 2 or w < 2:
        raise _lib.MpiFlowHipError("%s: a grid mesh needs at least one sample and h, w >= 2 (got B, h, w = %d, %d, %d)" % (who, B, h, w))
    if B > 65535 or B * h * w > _lib.MESH_MAX_BHW:
        raise _lib.MpiFlowHipError("%s: B must be at most 65535 and B * h * w at most %d (got B, h, w = %d, %d, %d)" % (who, _lib.MESH_MAX_BHW, B, h, w))


@_on_device
def rgbd_mesh_vertices(rgbd, cam_int, cam_ext):
    """mpf_rgbd_mesh_vertices: RGBDRenderer.construct_mesh and the first half of render_mesh (warpback/utils.py) in one launch: rgbd [B,4,h,w]
    (r, g, b, disparity), cam_int [B,3,3], cam_ext [B,3,4] -> (verts_ndc [B,h*w,3], attrs [B,h*w,5]).  verts_ndc: unprojected with depth =
    1 / (disp + 1e-4), moved by the extrinsic, through the near / far perspective matrix, divided, x and y negated, x scaled by w / h.  attrs:
    r, g, b, the Sobel visibility bit exp(-10 |grad disp|) > 0.3, the depth after the extrinsic.  cam_int is inverted in float64 by the
    adjugate.  float32, contiguous, on the GPU, or MpiFlowHipError.  Asynchronous on the current stream: no host copy, no synchronisation."""
    who = "rgbd_mesh_vertices"
    x = check_tensor(rgbd, "rgbd", who, (None, 4, None, None), "[B,4,h,w]")
    B, _, h, w = x.shape
    K = check_tensor(cam_int, "cam_int", who, (B, 3, 3), "[B,3,3]")
    E = check_tensor(cam_ext, "cam_ext", who, (B, 3, 4), "[B,3,4]")
    _mesh_limits(who, B, h, w)
    check_devices(who, dict(rgbd=x, cam_int=K, cam_ext=E))
    verts = torch.empty((B, h * w, 3), dtype=_f32, device=x.device)
    attrs = torch.empty((B, h * w, 5), dtype=_f32, device=x.device)
    a = _lib.MpfMeshVertexArgs()
    a.rgbd, a.cam_int, a.cam_ext, a.verts_ndc, a.attrs, a.B, a.h, a.w = x.data_ptr(), K.data_ptr(), E.data_ptr(), verts.data_ptr(), attrs.data_ptr(), B, h, w
    _lib.check(_lib.load().mpf_rgbd_mesh_vertices(ctypes.byref(a), _stream()), "mpf_rgbd_mesh_vertices")
    return verts, attrs


@_on_device
def rasterize_grid(verts_ndc, attrs, h, w, blur_radius=1e-6):
    """mpf_rasterize_grid: pytorch3d's rasterize_meshes(faces_per_pixel=1, blur_radius) and interpolate_face_attributes on the regular grid mesh
    of h x w vertices (RGBDRenderer.get_faces' faces, implicit): verts_ndc [B,h*w,3], attrs [B,h*w,C], C <= 8 -> (pix_to_face int64 [B,h,w],
    packed b * F + f; zbuf [B,h,w]; bary [B,h,w,3], unclipped; out [B,C,h,w]).  A pixel no face covers holds -1, -1, -1 and +0.  The winner of
    a pixel is the covering face of the least depth, the lowest face index on equal depth; a face with a non-finite coordinate is skipped;
    blur_radius is a SQUARED distance in NDC units.  INTEGRATION.md section 16 has the definition operation by operation.  No gradients.
    float32, contiguous, on the GPU, or MpiFlowHipError.  Identical bytes on every run.  Asynchronous on the current stream."""
    who = "rasterize_grid"
    v = check_tensor(verts_ndc, "verts_ndc", who, (None, None, 3), "[B,h*w,3]")
    B, n, _ = v.shape
    at = check_tensor(attrs, "attrs", who, (B, n, None), "[B,h*w,C] like verts_ndc")
    C = at.shape[2]
    try:
        h, w = operator.index(h), operator.index(w)
    except TypeError:
        raise _lib.MpiFlowHipError("%s: h and w must be integers (got %r, %r)" % (who, h, w)) from None
    if h < 2 or w < 2 or h * w != n:
        raise _lib.MpiFlowHipError("%s: h, w must be at least 2 with h * w = %d, the vertices of verts_ndc (got h, w = %d, %d)" % (who, n, h, w))
    if not 1 <= C <= _lib.MESH_MAX_ATTRS:
        raise _lib.MpiFlowHipError("%s: attrs must have 1..%d channels (got %d)" % (who, _lib.MESH_MAX_ATTRS, C))
    try:
        blur = float(blur_radius)
    except (TypeError, ValueError):
        blur = float("nan")
    if not 0.0 <= blur < float("inf"):
        raise _lib.MpiFlowHipError("%s: blur_radius must be a finite number >= 0 (got %r)" % (who, blur_radius))
    _mesh_limits(who, B, h, w)
    check_devices(who, dict(verts_ndc=v, attrs=at))
    lib = _lib.load()
    dev = v.device
    pix = torch.empty((B, h, w), dtype=torch.int64, device=dev)
    zbuf = torch.empty((B, h, w), dtype=_f32, device=dev)
    bary = torch.empty((B, h, w, 3), dtype=_f32, device=dev)
    out = torch.empty((B, C, h, w), dtype=_f32, device=dev)
    ws = torch.empty(int(lib.mpf_rasterize_grid_workspace(B, h, w)) // 8, dtype=torch.int64, device=dev)
    a = _lib.MpfMeshRasterArgs()
    a.verts_ndc, a.attrs, a.pix_to_face, a.zbuf, a.bary, a.out = v.data_ptr(), at.data_ptr(), pix.data_ptr(), zbuf.data_ptr(), bary.data_ptr(), out.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    a.B, a.h, a.w, a.C, a.blur_radius = B, h, w, C, blur
    _lib.check(lib.mpf_rasterize_grid(ctypes.byref(a), _stream()), "mpf_rasterize_grid")
    del ws
    return pix, zbuf, bary, out


CANNY_PASSES = {"all": _lib.CANNY_PASS_ALL, "smooth": _lib.CANNY_PASS_SMOOTH, "classify": _lib.CANNY_PASS_CLASSIFY, "hysteresis": _lib.CANNY_PASS_HYSTERESIS}


def canny_weights(sigma):
    """(radius, weights): the Gaussian taps of canny_masked, radius = int(4 sigma + 0.5) and w[radius + k] = exp(-0.5 / sigma^2 * k^2) over their
    sum, formed in float64 (math.fsum) and rounded to float32 once; a list of 2 radius + 1 Python floats holding float32 values"""
    import math
    import struct
    sigma = float(sigma)
    radius = int(4.0 * sigma + 0.5)
    phi = [math.exp(-0.5 / (sigma * sigma) * (k * k)) for k in range(-radius, radius + 1)]
    total = math.fsum(phi)
    return radius, [struct.unpack("f", struct.pack("f", p / total))[0] for p in phi]


def canny_workspace(B, h, w, device):
    """an uninitialised workspace for canny_masked on [B,1,h,w] (float32, mpf_canny_workspace bytes); canny_workspace_views names its parts"""
    n = int(_lib.load().mpf_canny_workspace(int(B), int(h), int(w)))
    if n == 0:
        raise _lib.MpiFlowHipError("canny_workspace: B must be 1..65535, h, w >= 1 and B * h * w at most %d (got %r, %r, %r)" % (_lib.CANNY_MAX_BHW, B, h, w))
    return torch.empty(n // 4, dtype=_f32, device=device)


def canny_workspace_views(workspace, B, h, w):
    """(smoothed float32 [B,1,h,w], classes uint8 [B,1,h,w]: 0, 1 weak, 2 strong): what the stages of canny_masked leave in a workspace, as views"""
    n = B * h * w
    return workspace[:n].view(B, 1, h, w), workspace.view(torch.uint8)[4 * n:5 * n].view(B, 1, h, w)


@_on_device
def canny_masked(gray, mask, sigma=2.0, low_threshold=0.1, high_threshold=0.2, out=None, workspace=None, passes="all"):
    """mpf_canny: skimage.feature.canny(gray[i, 0], sigma, low_threshold, high_threshold, mask=mask[i, 0] != 0) for every image of gray
    [b,1,h,w] with mask [b,1,h,w] (nonzero: inside) -> [b,1,h,w] float32 of 0.0 and 1.0, what the reference's get_edge returns.  Three
    stages - the masked, normalised Gaussian; Sobel, magnitude and interpolated non-maximum suppression into classes; hysteresis as a
    reachability fixpoint - in float32 exactly as INTEGRATION.md section 17 states them; identical bytes on every run.  `out`: a tensor to
    write; `workspace`: canny_workspace(b, h, w, device), reused between calls; `passes`: 'all', or one stage alone on what the stage before
    left in the workspace ('smooth' returns the smoothed view, 'classify' the class view of canny_workspace_views, 'hysteresis' out; the
    last two need `workspace`).  float32, contiguous, on the GPU, or MpiFlowHipError.  Asynchronous on the current stream: no host copy, no
    synchronisation."""
    who = "canny_masked"
    g = check_tensor(gray, "gray", who, (None, 1, None, None), "[b,1,h,w]")
    B, _, h, w = g.shape
    m = check_tensor(mask, "mask", who, (B, 1, h, w), "[b,1,h,w] like gray")
    tensors = dict(gray=g, mask=m)
    if out is not None:
        tensors["out"] = check_tensor(out, "out", who, (B, 1, h, w), "[b,1,h,w] like gray")
    if passes not in CANNY_PASSES:
        raise _lib.MpiFlowHipError("%s: passes must be one of %s (got %r)" % (who, ", ".join(CANNY_PASSES), passes))
    try:
        sigma, lo, hi = float(sigma), float(low_threshold), float(high_threshold)
    except (TypeError, ValueError):
        raise _lib.MpiFlowHipError("%s: sigma, low_threshold and high_threshold must be numbers (got %r, %r, %r)" % (who, sigma, low_threshold, high_threshold)) from None
    if not 0.0 < sigma < float("inf"):
        raise _lib.MpiFlowHipError("%s: sigma must be a finite number > 0 (got %r)" % (who, sigma))
    if int(4.0 * sigma + 0.5) > _lib.CANNY_MAX_RADIUS:
        raise _lib.MpiFlowHipError("%s: sigma = %r needs a radius of int(4 sigma + 0.5) = %d taps, more than the %d the kernel holds"
                                   % (who, sigma, int(4.0 * sigma + 0.5), _lib.CANNY_MAX_RADIUS))
    if not lo <= hi:
        raise _lib.MpiFlowHipError("%s: low_threshold must be at most high_threshold, neither NaN (got %r, %r)" % (who, low_threshold, high_threshold))
    if B < 1 or h < 1 or w < 1 or B > 65535 or B * h * w > _lib.CANNY_MAX_BHW:
        raise _lib.MpiFlowHipError("%s: gray must have 1..65535 images of at least one pixel and at most %d pixels in all (got shape %s)" % (who, _lib.CANNY_MAX_BHW, tuple(g.shape)))
    lib = _lib.load()
    need = int(lib.mpf_canny_workspace(B, h, w))
    if workspace is not None:
        ws = check_tensor(workspace, "workspace", who, 1)
        if ws.numel() * 4 < need:
            raise _lib.MpiFlowHipError("%s: workspace holds %d bytes, %d needed (ops.canny_workspace)" % (who, ws.numel() * 4, need))
        tensors["workspace"] = ws
    elif passes in ("classify", "hysteresis"):
        raise _lib.MpiFlowHipError("%s: passes=%r reads what the stage before left in `workspace`: hand one in" % (who, passes))
    check_devices(who, tensors)
    ws = torch.empty(need // 4, dtype=_f32, device=g.device) if workspace is None else workspace
    if out is None and passes in ("all", "hysteresis"):
        out = torch.empty_like(g)
    radius, weights = canny_weights(sigma)
    a = _lib.MpfCannyArgs()
    a.gray, a.mask, a.out = g.data_ptr(), m.data_ptr(), None if out is None else out.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    a.B, a.h, a.w, a.radius = B, h, w, radius
    for k, v in enumerate(weights):
        a.weights[k] = v
    a.low_threshold, a.high_threshold, a.passes = lo, hi, CANNY_PASSES[passes]
    _lib.check(lib.mpf_canny(ctypes.byref(a), _stream()), "mpf_canny")
    if passes == "smooth":
        return canny_workspace_views(ws, B, h, w)[0]
    if passes == "classify":
        return canny_workspace_views(ws, B, h, w)[1]
    return out


BILATERAL_DTYPES = {torch.float32: _lib.BILATERAL_F32, torch.float64: _lib.BILATERAL_F64, torch.uint8: _lib.BILATERAL_U8}


def sparse_bilateral_rank(n):
    """k*(n), the rank sparse_bilateral_filter takes among n valid samples: 1 + #{k <= n : S_k <= 0.5}, S_k the float32 sum of k copies of
    fl32(1 / n) added one at a time (the library's host arithmetic, the kernel's own function; no GPU)"""
    k = int(_lib.load().mpf_sparse_bilateral_rank(int(n)))
    if k == 0:
        raise _lib.MpiFlowHipError("sparse_bilateral_rank: n must be 1..%d (got %r)" % (_lib.BILATERAL_MAX_WINDOW ** 2, n))
    return k


def sparse_bilateral_workspace(dtype, B, h, w, device):
    """an uninitialised workspace for sparse_bilateral_filter on B images of h x w of `dtype` (uint8, mpf_sparse_bilateral_workspace bytes)"""
    n = int(_lib.load().mpf_sparse_bilateral_workspace(BILATERAL_DTYPES.get(dtype, -1), int(B), int(h), int(w)))
    if n == 0:
        raise _lib.MpiFlowHipError("sparse_bilateral_workspace: dtype must be float32, float64 or uint8, B 1..65535, h, w >= 3 and B * h * w at most %d "
                                   "(got %r, %r, %r, %r)" % (_lib.BILATERAL_MAX_BHW, dtype, B, h, w))
    return torch.empty(n, dtype=torch.uint8, device=device)


@_on_device
def sparse_bilateral_filter(depth, filter_size, depth_threshold=0.04, mask=None, num_iter=None, out=None, workspace=None):
    """mpf_sparse_bilateral: the reference's sparse_bilateral_filtering(depth, filter_size, depth_threshold=, mask=, num_iter=) per image of
    depth [h,w], [B,h,w] or [B,1,h,w] -> a tensor like depth.  A 0/1-weighted median around disparity discontinuities, num_iter times
    (None: len(filter_size)) with windows filter_size[i] in 3, 5, 7, 9, as INTEGRATION.md section 18 states it; the result is a selection of
    input values, equal to the reference's bit for bit, identical bytes on every run.  depth: float32 (arithmetic in float32), float64, or
    uint8, whose value is u / 255.0 in float64 (cv2.imread(path, 0) / 255) and whose result is the selected pixel's byte.  mask: bool, uint8
    or float32 of 0 / 1, shaped like depth or [h,w] for every image.  `out`: a tensor like depth to write (not depth itself); `workspace`:
    sparse_bilateral_workspace(...), reused between calls.  Contiguous, on the GPU, or MpiFlowHipError.  Asynchronous on the current stream."""
    who = "sparse_bilateral_filter"
    d = check_tensor(depth, "depth", who, depth.dim() if isinstance(depth, torch.Tensor) and depth.dim() in (2, 3, 4) else 3,
                     "[h,w], [B,h,w] or [B,1,h,w]", dtypes=tuple(BILATERAL_DTYPES))
    if d.dim() == 4 and d.shape[1] != 1:
        raise _lib.MpiFlowHipError("%s: depth must be [h,w], [B,h,w] or [B,1,h,w], a contiguous tensor (got shape %s)" % (who, tuple(d.shape)))
    B, (h, w) = (1 if d.dim() == 2 else d.shape[0]), d.shape[-2:]
    tensors = dict(depth=d)
    m = None
    if mask is not None:
        shared = isinstance(mask, torch.Tensor) and mask.dim() == 2 and d.dim() != 2
        m = check_tensor(mask, "mask", who, (h, w) if shared else tuple(d.shape), "[h,w] or shaped like depth", dtypes=(torch.bool, torch.uint8, torch.float32))
        tensors["mask"] = m
    if out is not None:
        tensors["out"] = check_tensor(out, "out", who, tuple(d.shape), "shaped like depth", dtypes=(d.dtype,))
    try:
        sizes = [operator.index(s) for s in filter_size]
    except TypeError:
        raise _lib.MpiFlowHipError("%s: filter_size must be a sequence of integers (got %r)" % (who, filter_size)) from None
    for s in sizes:
        if s % 2 == 0:
            raise _lib.MpiFlowHipError("%s: a window must be odd (got %d in filter_size %r)" % (who, s, list(sizes)))
        if not 3 <= s <= _lib.BILATERAL_MAX_WINDOW:
            raise _lib.MpiFlowHipError("%s: a window must be 3, 5, 7 or 9 (got %d in filter_size %r)" % (who, s, list(sizes)))
    if h < 3 or w < 3:
        raise _lib.MpiFlowHipError("%s: depth must have at least 3 rows and 3 columns (got h, w = %d, %d)" % (who, h, w))
    n_iter = len(sizes) if num_iter is None else operator.index(num_iter)
    if n_iter > len(sizes):
        raise _lib.MpiFlowHipError("%s: num_iter = %d needs %d windows, filter_size holds %d" % (who, n_iter, n_iter, len(sizes)))
    if not 1 <= n_iter <= _lib.BILATERAL_MAX_ITER:
        raise _lib.MpiFlowHipError("%s: num_iter must be 1..%d (got %d)" % (who, _lib.BILATERAL_MAX_ITER, n_iter))
    thr = float(depth_threshold)
    if thr != thr:
        raise _lib.MpiFlowHipError("%s: depth_threshold must not be NaN" % who)
    if B < 1 or B > 65535 or B * h * w > _lib.BILATERAL_MAX_BHW:
        raise _lib.MpiFlowHipError("%s: depth must have 1..65535 images and at most %d pixels in all (got shape %s)" % (who, _lib.BILATERAL_MAX_BHW, tuple(d.shape)))
    if out is not None and out.data_ptr() == d.data_ptr():
        raise _lib.MpiFlowHipError("%s: out must not be depth itself (a pixel reads its neighbours)" % who)
    lib = _lib.load()
    code = BILATERAL_DTYPES[d.dtype]
    need = int(lib.mpf_sparse_bilateral_workspace(code, B, h, w))
    if workspace is not None:
        ws = check_tensor(workspace, "workspace", who, 1, dtypes=(torch.uint8,))
        if ws.numel() < need:
            raise _lib.MpiFlowHipError("%s: workspace holds %d bytes, %d needed (ops.sparse_bilateral_workspace)" % (who, ws.numel(), need))
        tensors["workspace"] = ws
    check_devices(who, tensors)
    ws = torch.empty(need, dtype=torch.uint8, device=d.device) if workspace is None else workspace
    if out is None:
        out = torch.empty_like(d)
    if m is not None:                                                       # the kernel reads bytes: bool as it is, the others as != 0
        m8 = m.view(torch.uint8) if m.dtype == torch.bool else (m if m.dtype == torch.uint8 else (m != 0).view(torch.uint8))
    a = _lib.MpfBilateralArgs()
    a.depth, a.mask, a.out = d.data_ptr(), None if m is None else m8.data_ptr(), out.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    a.dtype, a.B, a.h, a.w = code, B, h, w
    a.mask_shared = 1 if m is not None and m.dim() == 2 else 0
    a.num_iter, a.depth_threshold = n_iter, thr
    for i in range(n_iter):
        a.filter_size[i] = sizes[i]
    _lib.check(lib.mpf_sparse_bilateral(ctypes.byref(a), _stream()), "mpf_sparse_bilateral")
    del ws
    return out


def _gather_pxpy_args(who, pxpy, B, C, H, W, tensors):
    """MpfGatherPxpyArgs with the shape and pxpy set: pxpy [B,2,N] float32 or int64, contiguous; the call's limits; the device last"""
    p = check_tensor(pxpy, "pxpy", who, (B, 2, None), "[B,2,N]", dtypes=(torch.float32, torch.int64))
    N = p.shape[2]
    if not 1 <= B <= 65535 or min(C, H, W, N) < 1 or B * C * H * W >= 1 << 31 or B * C * N >= 1 << 31:
        raise _lib.MpiFlowHipError("%s: 1..65535 images, at least one channel, pixel and point, and B * C * H * W and B * C * N below 2^31 "
                                   "(got B, C, H, W, N = %d, %d, %d, %d, %d)" % (who, B, C, H, W, N))
    tensors["pxpy"] = p
    check_devices(who, tensors)
    a = _lib.MpfGatherPxpyArgs()
    a.pxpy, a.pxpy_dtype = p.data_ptr(), _lib.PXPY_F32 if p.dtype == torch.float32 else _lib.PXPY_I64
    a.B, a.C, a.H, a.W, a.N = B, C, H, W, N
    return a


@_on_device
def gather_pixel_by_pxpy(img, pxpy, out=None):
    """mpf_gather_pxpy: out[b,c,i] = img[b,c,y_i,x_i] with (x_i, y_i) = pxpy[b,:,i] rounded (ties to even) and clamped to the frame - the reference's
    gather_pixel_by_pxpy (utils/mpi/rendering_utils.py:26-43).  img [B,C,H,W] float32, pxpy [B,2,N] float32 or int64 -> [B,C,N].  A coordinate that is
    NaN or -inf reads index 0, +inf the last index.  Contiguous, on the GPU, or MpiFlowHipError.  Asynchronous on the current stream."""
    who = "gather_pixel_by_pxpy"
    im = check_tensor(img, "img", who, 4, "[B,C,H,W]")
    B, C, H, W = im.shape
    tensors = dict(img=im)
    if out is not None:
        N = pxpy.shape[2] if isinstance(pxpy, torch.Tensor) and pxpy.dim() == 3 else None
        tensors["out"] = check_tensor(out, "out", who, (B, C, N), "[B,C,N]")
    a = _gather_pxpy_args(who, pxpy, B, C, H, W, tensors)
    if out is None:
        out = torch.empty((B, C, a.N), dtype=_f32, device=im.device)
    a.img, a.out = im.data_ptr(), out.data_ptr()
    _lib.check(_lib.load().mpf_gather_pxpy(ctypes.byref(a), _stream()), "mpf_gather_pxpy")
    return out


@_on_device
def gather_pixel_by_pxpy_backward(grad_out, pxpy, H, W, grad_img=None):
    """Adjoint of gather_pixel_by_pxpy with respect to img (mpf_gather_pxpy_bwd): grad_img[b,c,y_i,x_i] += grad_out[b,c,i].  grad_out [B,C,N] ->
    [B,C,H,W]; grad_img: a zero-initialised buffer to add into (allocated zeroed when None).  The adds are float atomics: where points share a pixel
    their arrival order decides the last bits of its sum.  pxpy has no gradient."""
    who = "gather_pixel_by_pxpy_backward"
    g = check_tensor(grad_out, "grad_out", who, 3, "[B,C,N]")
    B, C, N = g.shape
    H, W = operator.index(H), operator.index(W)
    tensors = dict(grad_out=g)
    if grad_img is not None:
        tensors["grad_img"] = check_tensor(grad_img, "grad_img", who, (B, C, H, W), "[B,C,H,W]")
    a = _gather_pxpy_args(who, pxpy, B, C, H, W, tensors)
    if a.N != N:
        raise _lib.MpiFlowHipError("%s: pxpy must be [B,2,N] with grad_out's N = %d (got shape %s)" % (who, N, tuple(pxpy.shape)))
    if grad_img is None:
        grad_img = torch.zeros((B, C, H, W), dtype=_f32, device=g.device)
    a.grad_out, a.grad_img = g.data_ptr(), grad_img.data_ptr()
    _lib.check(_lib.load().mpf_gather_pxpy_bwd(ctypes.byref(a), _stream()), "mpf_gather_pxpy_bwd")
    return grad_img


@_on_device
def sample_pdf(values, weights, u, out=None):
    """mpf_sample_pdf: the reference's sample_pdf (utils/mpi/rendering_utils.py:90-139) with its uniform draws handed in: values, weights [B,1,N,S] and
    u [B,1,N,n_samples] float32 -> samples [B,1,N,n_samples], as INTEGRATION.md section 21 states it, in one launch without a [B,1,N,S] temporary.
    1 <= S, n_samples <= 128 and B * N * max(S, n_samples) < 2^31.  weights, u (and out) are contiguous; values is contiguous or expanded over the rays
    (stride 0 in dim 2, unit stride in dim 3: a per-plane disparity broadcast with .expand), which is read in place.  Forward only.  On the GPU, or
    MpiFlowHipError.  Identical bytes on every run.  Asynchronous on the current stream."""
    who = "sample_pdf"
    w = check_tensor(weights, "weights", who, (None, 1, None, None), "[B,1,N,S]")
    B, _, N, S = w.shape
    if not isinstance(values, torch.Tensor):
        raise _lib.MpiFlowHipError("%s: values must be a torch.Tensor (got %s)" % (who, type(values).__name__))
    if values.dtype != torch.float32:
        raise _lib.MpiFlowHipError("%s: values must be float32 (got %s); call .float() on it (the kernels are float32 only)" % (who, values.dtype))
    if tuple(values.shape) != (B, 1, N, S):
        raise _lib.MpiFlowHipError("%s: values must be [B,1,N,S] like weights, %s (got shape %s)" % (who, tuple(w.shape), tuple(values.shape)))
    expanded = not values.is_contiguous() and values.stride(2) == 0 and (S == 1 or values.stride(3) == 1) and (B == 1 or values.stride(0) >= 0)
    if not values.is_contiguous() and not expanded:
        raise _lib.MpiFlowHipError("%s: values must be contiguous, or expanded over the rays with stride 0 in dim 2 and unit stride in dim 3 "
                                   "(got shape %s with strides %s)" % (who, tuple(values.shape), values.stride()))
    uu = check_tensor(u, "u", who, (B, 1, N, None), "[B,1,N,n_samples]")
    NS = uu.shape[3]
    tensors = dict(values=values, weights=w, u=uu)
    if out is not None:
        tensors["out"] = check_tensor(out, "out", who, (B, 1, N, NS), "[B,1,N,n_samples]")
    if not 1 <= S <= _lib.SAMPLE_PDF_MAX_S:
        raise _lib.MpiFlowHipError("%s: S must be 1..%d (got %d from weights of shape %s)" % (who, _lib.SAMPLE_PDF_MAX_S, S, tuple(w.shape)))
    if not 1 <= NS <= _lib.SAMPLE_PDF_MAX_SAMPLES:
        raise _lib.MpiFlowHipError("%s: n_samples must be 1..%d (got %d from u of shape %s)" % (who, _lib.SAMPLE_PDF_MAX_SAMPLES, NS, tuple(uu.shape)))
    if B < 1 or N < 1 or B * N * max(S, NS) >= 1 << 31:
        raise _lib.MpiFlowHipError("%s: at least one row, and B * N * max(S, n_samples) below 2^31 (got B, N, S, n_samples = %d, %d, %d, %d)" % (who, B, N, S, NS))
    check_devices(who, tensors)
    if out is None:
        out = torch.empty((B, 1, N, NS), dtype=_f32, device=w.device)
    a = _lib.MpfSamplePdfArgs()
    a.values, a.weights, a.u, a.out = values.data_ptr(), w.data_ptr(), uu.data_ptr(), out.data_ptr()
    a.values_batch_stride = (values.stride(0) if B > 1 else 0) if expanded else N * S
    a.values_row_stride = 0 if expanded else S
    a.B, a.N, a.S, a.n_samples = B, N, S, NS
    _lib.check(_lib.load().mpf_sample_pdf(ctypes.byref(a), _stream()), "mpf_sample_pdf")
    return out


def _disp_consistency_args(who, K_src_inv, disparity_src, G_tgt_src, K_tgt, disparity_tgt, tensors):
    """MpfDispConsistencyArgs with the five inputs set; `tensors`: the call's further tensors, already checked.  The device last."""
    ds = check_tensor(disparity_src, "disparity_src", who, (None, 1, None, None), "[B,1,H,W]")
    B, _, H, W = ds.shape
    dt = check_tensor(disparity_tgt, "disparity_tgt", who, 4, "[B,1,H,W]")
    if dt.shape != ds.shape:
        raise _lib.MpiFlowHipError("%s: disparity_tgt must have disparity_src's shape %s (got %s): frames of two sizes are not provided"
                                   % (who, tuple(ds.shape), tuple(dt.shape)))
    Ki = check_tensor(K_src_inv, "K_src_inv", who, (B, 3, 3), "[B,3,3]")
    G = check_tensor(G_tgt_src, "G_tgt_src", who, (B, 4, 4), "[B,4,4]")
    Kt = check_tensor(K_tgt, "K_tgt", who, (B, 3, 3), "[B,3,3]")
    if not 1 <= B <= 65535 or H < 1 or W < 1 or B * H * W >= 1 << 31:
        raise _lib.MpiFlowHipError("%s: 1..65535 frames of at least one pixel and B * H * W below 2^31 (got B, H, W = %d, %d, %d)" % (who, B, H, W))
    all_tensors = dict(disparity_src=ds, disparity_tgt=dt, K_src_inv=Ki, G_tgt_src=G, K_tgt=Kt)
    all_tensors.update(tensors)
    check_devices(who, all_tensors)
    a = _lib.MpfDispConsistencyArgs()
    a.K_src_inv, a.G_tgt_src, a.K_tgt, a.disparity_src, a.disparity_tgt = Ki.data_ptr(), G.data_ptr(), Kt.data_ptr(), ds.data_ptr(), dt.data_ptr()
    a.B, a.H, a.W = B, H, W
    return a


@_on_device
def disparity_consistency(K_src_inv, disparity_src, G_tgt_src, K_tgt, disparity_tgt):
    """mpf_disp_consistency: the reference's disparity_consistency_src_to_tgt (utils/mpi/mpi_rendering.py:180-210) on the standard (x, y, 1) grid:
    disparity_src, disparity_tgt [B,1,H,W], K_src_inv, K_tgt [B,3,3], G_tgt_src [B,4,4], all float32 on the GPU (the matrices too: nothing crosses
    to the host) -> (loss, state).  loss: a 0-dim tensor, the mean over the source pixels that project into the target frame of
    |1 / p.z - disparity_tgt[rounded pixel]|, NaN when there is none; its sum uses no atomics and gives the same bits on every run.  state: what
    disparity_consistency_backward needs (the call's workspace; its first 16 bytes hold the float64 sum and the int64 count)."""
    who = "disparity_consistency"
    a = _disp_consistency_args(who, K_src_inv, disparity_src, G_tgt_src, K_tgt, disparity_tgt, {})
    lib = _lib.load()
    dev = disparity_src.device
    state = torch.empty(int(lib.mpf_disp_consistency_workspace(a.B, a.H, a.W)), dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=_f32, device=dev)
    a.loss, a.workspace, a.workspace_bytes = loss.data_ptr(), state.data_ptr(), state.numel()
    _lib.check(lib.mpf_disp_consistency(ctypes.byref(a), _stream()), "mpf_disp_consistency")
    return loss, state


@_on_device
def disparity_consistency_backward(grad_loss, state, K_src_inv, disparity_src, G_tgt_src, K_tgt, disparity_tgt, want_src=True, want_tgt=True):
    """mpf_disp_consistency_bwd -> (grad_disparity_src | None, grad_disparity_tgt | None), each [B,1,H,W].  grad_loss: the upstream gradient, a float32
    tensor of one element on the GPU; state: disparity_consistency's, for the same inputs.  grad_disparity_src is one store per pixel (the same bits on
    every run); grad_disparity_tgt is scattered with float atomics, so source pixels that land on one target pixel decide its last bits by their order."""
    who = "disparity_consistency_backward"
    if not isinstance(grad_loss, torch.Tensor) or grad_loss.numel() != 1:
        raise _lib.MpiFlowHipError("%s: grad_loss must be a float32 tensor of one element (got %s)"
                                   % (who, tuple(grad_loss.shape) if isinstance(grad_loss, torch.Tensor) else type(grad_loss).__name__))
    g = check_tensor(grad_loss, "grad_loss", who, grad_loss.dim())
    st = check_tensor(state, "state", who, 1, dtypes=(torch.uint8,))
    if not (want_src or want_tgt):
        raise _lib.MpiFlowHipError("%s: want_src or want_tgt: one gradient at least" % who)
    a = _disp_consistency_args(who, K_src_inv, disparity_src, G_tgt_src, K_tgt, disparity_tgt, dict(grad_loss=g, state=st))
    lib = _lib.load()
    need = int(lib.mpf_disp_consistency_workspace(a.B, a.H, a.W))
    if st.numel() < need:
        raise _lib.MpiFlowHipError("%s: state holds %d bytes, %d needed: it is not disparity_consistency's for these shapes" % (who, st.numel(), need))
    grad_src = torch.empty_like(disparity_src) if want_src else None
    grad_tgt = torch.zeros_like(disparity_tgt) if want_tgt else None
    a.grad_loss, a.workspace, a.workspace_bytes = g.data_ptr(), st.data_ptr(), st.numel()
    a.grad_disparity_src = grad_src.data_ptr() if want_src else None
    a.grad_disparity_tgt = grad_tgt.data_ptr() if want_tgt else None
    _lib.check(lib.mpf_disp_consistency_bwd(ctypes.byref(a), _stream()), "mpf_disp_consistency_bwd")
    return grad_src, grad_tgt


_flow_warp_lin = {}


def flow_warp_linspace(device, H, W):
    """warp_rife's grids: (torch.linspace(-1, 1, W), torch.linspace(-1, 1, H)) on `device`, made by torch once per (device, H, W) and kept, as the
    reference keeps its backwarp_tenGrid.  The kernel reads them; it does not re-derive linspace."""
    key = (str(device), int(H), int(W))
    if key not in _flow_warp_lin:
        _flow_warp_lin[key] = (torch.linspace(-1.0, 1.0, int(W), dtype=_f32, device=device), torch.linspace(-1.0, 1.0, int(H), dtype=_f32, device=device))
    return _flow_warp_lin[key]


def _flow_warp_args(who, x, flow, mode, tensors, whole=False):
    """MpfFlowWarpArgs with x, flow, the mode, the shape and (warp_rife) the linspace grids set; `tensors`: the call's further [B,C,H,W] tensors by
    name.  x's own checks, flow's, the others', the mode's limits, the device last."""
    xx = check_tensor(x, "x", who, 4, "[B,C,H,W]")
    B, C, H, W = xx.shape
    if isinstance(flow, torch.Tensor) and flow.dim() == 4 and flow.shape[0] != B:
        raise _lib.MpiFlowHipError("%s: flow must have x's batch size %d (got shape %s)" % (who, B, tuple(flow.shape)))
    fl = check_tensor(flow, "flow", who, (B, 2, H, W), "[B,2,H,W] with x's B, H, W = %d, %d, %d" % (B, H, W))
    checked = dict(x=xx, flow=fl)
    for name, (t, shape, layout) in tensors.items():
        if t is not None:
            checked[name] = check_tensor(t, name, who, shape(B, C, H, W), layout)
    if mode not in (_lib.FLOW_WARP_WARP, _lib.FLOW_WARP_RIFE):
        raise _lib.MpiFlowHipError("%s: mode must be FLOW_WARP_WARP (0) or FLOW_WARP_RIFE (1) (got %r)" % (who, mode))
    if not 1 <= B <= 32767 or min(C, H, W) < 1 or H * W > 1 << 30 or B * C * H * W >= 1 << 31 or B * 2 * H * W >= 1 << 31:
        raise _lib.MpiFlowHipError("%s: 1..32767 images of at least one channel and pixel, H * W at most 2^30 and B * C * H * W and B * 2 * H * W below "
                                   "2^31 (got B, C, H, W = %d, %d, %d, %d)" % (who, B, C, H, W))
    if mode == _lib.FLOW_WARP_RIFE and (H < 2 or W < 2):
        raise _lib.MpiFlowHipError("%s: warp_rife needs H and W of at least 2 (got H, W = %d, %d): its scale (W - 1) / 2 is 0 at one pixel" % (who, H, W))
    check_devices(who, checked)
    a = _lib.MpfFlowWarpArgs()
    a.x, a.flow, a.mode, a.whole = xx.data_ptr(), fl.data_ptr(), mode, 1 if whole else 0
    a.B, a.C, a.H, a.W = B, C, H, W
    keep = None
    if mode == _lib.FLOW_WARP_RIFE:
        keep = flow_warp_linspace(xx.device, H, W)
        a.lin_w, a.lin_h = keep[0].data_ptr(), keep[1].data_ptr()
    return a, keep


_BCHW = (lambda B, C, H, W: (B, C, H, W), "[B,C,H,W] like x")


@_on_device
def flow_warp(x, flow, mode, want_mask, out=None, whole=False):
    """mpf_flow_warp: the reference's backward warp of x [B,C,H,W] by flow [B,2,H,W] (utils/transform.py:60-111) in one pass - a pixel's taps are
    built once and used for every channel and for the mask.  mode: _lib.FLOW_WARP_WARP (warp(): zero padding, the reference's mixed align_corners)
    or _lib.FLOW_WARP_RIFE (warp_rife(): border padding, align_corners=True).  -> (out [B,C,H,W], mask [B,1,H,W] or None); want_mask is for
    FLOW_WARP_WARP only: the sum of the weights of the taps inside the image.  float32, contiguous, on one GPU, or MpiFlowHipError before anything is
    launched.  whole: one thread per pixel walks every channel instead of 64-channel grid.z slices (a tuning knob; the same bytes).  Identical bytes
    on every run.  Asynchronous on the current stream."""
    who = "flow_warp"
    if want_mask and mode == _lib.FLOW_WARP_RIFE:
        raise _lib.MpiFlowHipError("%s: warp_rife has no mask (want_mask with FLOW_WARP_RIFE)" % who)
    a, keep = _flow_warp_args(who, x, flow, mode, dict(out=(out,) + _BCHW), whole)
    if out is None:
        out = torch.empty_like(x)
    mask = torch.empty((a.B, 1, a.H, a.W), dtype=_f32, device=x.device) if want_mask else None
    a.out, a.mask = out.data_ptr(), mask.data_ptr() if want_mask else None
    _lib.check(_lib.load().mpf_flow_warp(ctypes.byref(a), _stream()), "mpf_flow_warp")
    del keep
    return out, mask


@_on_device
def flow_warp_backward(x, flow, g_out, mode, want_x=True, want_flow=True, grad_x=None, whole=False):
    """mpf_flow_warp_bwd -> (grad_x [B,C,H,W] | None, grad_flow [B,2,H,W] | None) for the upstream gradient g_out [B,C,H,W] of flow_warp's out (the
    mask has no gradient).  grad_x is scattered with float atomic adds into a zeroed buffer (grad_x: a zero-initialised one to add into), so the order
    of the adds decides its last bits; grad_flow is one store per pixel, summed over the channels in a fixed order without atomics: identical bytes
    on every run, and with whole=True (one thread walks every channel; no workspace) as without."""
    who = "flow_warp_backward"
    if not (want_x or want_flow):
        raise _lib.MpiFlowHipError("%s: want_x or want_flow: one gradient at least" % who)
    a, keep = _flow_warp_args(who, x, flow, mode, dict(g_out=(g_out,) + _BCHW, grad_x=(grad_x if want_x else None,) + _BCHW), whole)
    lib = _lib.load()
    if want_x and grad_x is None:
        grad_x = torch.zeros_like(x)
    grad_flow = torch.empty_like(flow) if want_flow else None
    need = int(lib.mpf_flow_warp_workspace(a.B, a.C, a.H, a.W, a.whole)) if want_flow else 0
    ws = torch.empty(need, dtype=torch.uint8, device=x.device) if need else None
    a.grad_out = g_out.data_ptr()
    a.grad_x = grad_x.data_ptr() if want_x else None
    a.grad_flow = grad_flow.data_ptr() if want_flow else None
    a.workspace, a.workspace_bytes = (ws.data_ptr(), need) if need else (None, 0)
    _lib.check(lib.mpf_flow_warp_bwd(ctypes.byref(a), _stream()), "mpf_flow_warp_bwd")
    del ws, keep                                                # stream-ordered allocator: a later allocation on this stream queues behind the kernels
    return (grad_x if want_x else None), grad_flow


@_on_device
def pan_block1(rgb_low, disp_low, plane_disp, w1, b1, bn_scale, bn_shift, w2, b2, w3, b3, out=None):
    """mpf_pan_block1: the first residual block of the plane-adjustment network (model/PAN.py:18-46) with its 2 x 2 average pool over the S
    plane-images cat(rgb_low, disp_low, d_s) of each image, eval mode: conv1 and conv3 factorised into per-image maps built once, the rest fused per
    plane.  rgb_low [B,3,h,w], disp_low [B,1,h,w], plane_disp [B,S] (read on the device); w1 [8,5,3,3], b1 [8], w2
    [8,8,3,3], b2 [8], w3 [8,5,1,1], b3 [8] the block's parameters, bn_scale / bn_shift [8] its eval-mode BatchNorm folded.  -> out
    [B*S,8,h//2,w//2].  float32, contiguous, on one GPU, or MpiFlowHipError before anything is launched.  Identical bytes on every run.  Asynchronous
    on the current stream."""
    who = "pan_block1"
    C = _lib.PAN_C
    rgb = check_tensor(rgb_low, "rgb_low", who, (None, 3, None, None), "[B,3,h,w]")
    B, _, h, w = rgb.shape
    checked = dict(rgb_low=rgb)
    checked["disp_low"] = check_tensor(disp_low, "disp_low", who, (B, 1, h, w), "[B,1,h,w] with rgb_low's B, h, w = %d, %d, %d" % (B, h, w))
    checked["plane_disp"] = pd = check_tensor(plane_disp, "plane_disp", who, (B, None), "[B,S] with rgb_low's B = %d" % B)
    S = pd.shape[1]
    for name, t, shape in (("w1", w1, (C, 5, 3, 3)), ("b1", b1, (C,)), ("bn_scale", bn_scale, (C,)), ("bn_shift", bn_shift, (C,)), ("w2", w2, (C, C, 3, 3)),
                           ("b2", b2, (C,)), ("w3", w3, (C, 5, 1, 1)), ("b3", b3, (C,))):
        checked[name] = check_tensor(t, name, who, shape)
    if out is not None:
        checked["out"] = check_tensor(out, "out", who, (B * S, C, h // 2, w // 2), "[B*S,8,h//2,w//2]")
    if B < 1 or S < 1 or h < 2 or w < 2:
        raise _lib.MpiFlowHipError("%s: at least one image and one plane, h and w at least 2 (got B, S, h, w = %d, %d, %d, %d)" % (who, B, S, h, w))
    groups = (S + _lib.PAN_PLANES_PER_GROUP - 1) // _lib.PAN_PLANES_PER_GROUP
    if B * S * C * (h // 2) * (w // 2) >= 1 << 31 or B * C * h * w >= 1 << 31 or B * groups > 65535 or (h // 2 + 3) // 4 > 65535:
        raise _lib.MpiFlowHipError("%s: B * S * 8 * (h // 2) * (w // 2) and B * 8 * h * w below 2^31, at most 65535 (image, plane group) slices and row tiles "
                                   "(got B, S, h, w = %d, %d, %d, %d)" % (who, B, S, h, w))
    check_devices(who, checked)
    lib = _lib.load()
    if out is None:
        out = torch.empty((B * S, C, h // 2, w // 2), dtype=_f32, device=rgb.device)
    need = int(lib.mpf_pan_block1_workspace(B, h, w))
    ws = torch.empty(need, dtype=torch.uint8, device=rgb.device)
    a = _lib.MpfPanArgs()
    a.rgb_low, a.disp_low, a.plane_disp, a.out = rgb.data_ptr(), disp_low.data_ptr(), pd.data_ptr(), out.data_ptr()
    a.w1, a.b1, a.bn_scale, a.bn_shift, a.w2, a.b2, a.w3, a.b3 = (t.data_ptr() for t in (w1, b1, bn_scale, bn_shift, w2, b2, w3, b3))
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    a.B, a.S, a.h, a.w = B, S, h, w
    _lib.check(lib.mpf_pan_block1(ctypes.byref(a), _stream()), "mpf_pan_block1")
    del ws                                                      # stream-ordered allocator: a later allocation on this stream queues behind the kernels
    return out


def _stage2_args(who, B, h, w, **tensors):
    """MpfStage2Args with the named fields set; every tensor already checked"""
    if B < 1 or h < 1 or w < 1 or B > 65535 or B * h * w > (1 << 28):
        raise _lib.MpiFlowHipError("%s: 1..65535 images of at least one pixel and at most 2^28 pixels in all (got B, h, w = %d, %d, %d)" % (who, B, h, w))
    check_devices(who, tensors)
    a = _lib.MpfStage2Args()
    a.B, a.h, a.w = B, h, w
    for name, t in tensors.items():
        setattr(a, name, t.data_ptr())
    return a


def _stage2_out(t, name, who, shape, like):
    return torch.empty(shape, dtype=_f32, device=like.device) if t is None else check_tensor(t, name, who, shape)


@_on_device
def stage2_gray_hole(image, mask):
    """mpf_stage2_gray_hole: image [b,3,h,w], mask [b,1,h,w] -> (gray [b,1,h,w] = (0.2989 r + 0.587 g) + 0.114 b, torchvision's Grayscale;
    mask_hole = 1 - mask), one launch, equal to the torch expressions bit for bit.  float32, contiguous, on the GPU, or MpiFlowHipError."""
    who = "stage2_gray_hole"
    img = check_tensor(image, "image", who, (None, 3, None, None), "[b,3,h,w]")
    B, _, h, w = img.shape
    m = check_tensor(mask, "mask", who, (B, 1, h, w), "[b,1,h,w] like image")
    check_devices(who, dict(image=img, mask=m))
    gray, hole = torch.empty_like(m), torch.empty_like(m)
    a = _stage2_args(who, B, h, w, image=img, mask=m, gray=gray, mask_hole=hole)
    _lib.check(_lib.load().mpf_stage2_gray_hole(ctypes.byref(a), _stream()), "mpf_stage2_gray_hole")
    return gray, hole


@_on_device
def stage2_edge_input(gray, edge, mask_hole, out=None):
    """mpf_stage2_edge_input: the edge generator's input cat([gray, edge, mask_hole], 1) [b,3,h,w], written straight into one buffer"""
    who = "stage2_edge_input"
    g = check_tensor(gray, "gray", who, (None, 1, None, None), "[b,1,h,w]")
    B, _, h, w = g.shape
    e = check_tensor(edge, "edge", who, (B, 1, h, w), "[b,1,h,w] like gray")
    mh = check_tensor(mask_hole, "mask_hole", who, (B, 1, h, w), "[b,1,h,w] like gray")
    out = _stage2_out(out, "out", who, (B, 3, h, w), g)
    a = _stage2_args(who, B, h, w, gray=g, edge=e, mask_hole=mh, edge_input=out)
    _lib.check(_lib.load().mpf_stage2_edge_input(ctypes.byref(a), _stream()), "mpf_stage2_edge_input")
    return out


@_on_device
def stage2_gen_inputs(image, disp, mask_hole, edge_inpaint):
    """mpf_stage2_gen_inputs: both inpainting generators' inputs in one launch: (cat([image + mask_hole, edge_inpaint], 1) [b,4,h,w],
    cat([disp + mask_hole, edge_inpaint], 1) [b,2,h,w])"""
    who = "stage2_gen_inputs"
    img = check_tensor(image, "image", who, (None, 3, None, None), "[b,3,h,w]")
    B, _, h, w = img.shape
    d = check_tensor(disp, "disp", who, (B, 1, h, w), "[b,1,h,w] like image")
    mh = check_tensor(mask_hole, "mask_hole", who, (B, 1, h, w), "[b,1,h,w] like image")
    e = check_tensor(edge_inpaint, "edge_inpaint", who, (B, 1, h, w), "[b,1,h,w] like image")
    check_devices(who, dict(image=img, disp=d, mask_hole=mh, edge_inpaint=e))
    xi = torch.empty((B, 4, h, w), dtype=_f32, device=img.device)
    xd = torch.empty((B, 2, h, w), dtype=_f32, device=img.device)
    a = _stage2_args(who, B, h, w, image=img, disp=d, mask_hole=mh, edge_inpaint=e, image_input=xi, disp_input=xd)
    _lib.check(_lib.load().mpf_stage2_gen_inputs(ctypes.byref(a), _stream()), "mpf_stage2_gen_inputs")
    return xi, xd


@_on_device
def stage2_merge(image, image_inpaint, disp, disp_inpaint, mask_hole):
    """mpf_stage2_merge: (image * (1 - mask_hole) + image_inpaint * mask_hole, disp * (1 - mask_hole) + disp_inpaint * mask_hole) in one launch,
    in the reference's operation order: equal to the torch expressions bit for bit"""
    who = "stage2_merge"
    img = check_tensor(image, "image", who, (None, 3, None, None), "[b,3,h,w]")
    B, _, h, w = img.shape
    inp = check_tensor(image_inpaint, "image_inpaint", who, (B, 3, h, w), "[b,3,h,w] like image")
    d = check_tensor(disp, "disp", who, (B, 1, h, w), "[b,1,h,w] like image")
    dinp = check_tensor(disp_inpaint, "disp_inpaint", who, (B, 1, h, w), "[b,1,h,w] like image")
    mh = check_tensor(mask_hole, "mask_hole", who, (B, 1, h, w), "[b,1,h,w] like image")
    check_devices(who, dict(image=img, image_inpaint=inp, disp=d, disp_inpaint=dinp, mask_hole=mh))
    oi, od = torch.empty_like(img), torch.empty_like(d)
    a = _stage2_args(who, B, h, w, image=img, image_inpaint=inp, disp=d, disp_inpaint=dinp, mask_hole=mh, image_merged=oi, disp_merged=od)
    _lib.check(_lib.load().mpf_stage2_merge(ctypes.byref(a), _stream()), "mpf_stage2_merge")
    return oi, od


def _check_out_int(t, who, dtype, shape, layout):
    """check_tensor's rule for an integer `out` (the float32 test replaced by `dtype`): type, dtype, shape, contiguity; the 4-byte alignment
    the kernels' dword stores need.  Returns t itself."""
    if not isinstance(t, torch.Tensor):
        raise _lib.MpiFlowHipError("%s: out must be a torch.Tensor (got %s)" % (who, type(t).__name__))
    if t.dtype != dtype:
        raise _lib.MpiFlowHipError("%s: out must be %s (got %s)" % (who, str(dtype).replace("torch.", ""), t.dtype))
    if tuple(t.shape) != tuple(shape):
        raise _lib.MpiFlowHipError("%s: out must be %s, a contiguous tensor of %d dimensions (got shape %s)" % (who, layout, len(shape), tuple(t.shape)))
    if not t.is_contiguous():
        raise _lib.MpiFlowHipError("%s: out must be contiguous (got shape %s with strides %s)" % (who, tuple(t.shape), t.stride()))
    if t.data_ptr() % 4:
        raise _lib.MpiFlowHipError("%s: out must be 4-byte aligned (it is stored a dword at a time; got a view at offset %d)" % (who, t.storage_offset()))
    return t


@_on_device
def flow_to_image(flow, image=None, clip_flow=None, convert_to_bgr=False, out=None):
    """mpf_flow_to_image: RAFT/core/utils/flow_viz.py's flow_to_image per image of a batch, on the device: flow [N,2,H,W] -> uint8 [N,H,W,3], the
    colour wheel at upstream's precisions (float32 u, v, rad, atan2, fk; float64 wheel, blend and floor), normalised by each image's own
    rad_max + 1e-5.  clip_flow: upstream's np.clip(flow, 0, clip_flow) first (its lower bound is 0).  convert_to_bgr: channels B, G, R.
    image [N,3,H,W] in 0..255 (what RAFT.predict takes): the result is [N,2H,W,3], the frame truncated to uint8 on top and the colours below
    (demo.py:viz); convert_to_bgr reverses both halves, which is the layout ops.png_scanlines takes.  Against numpy a byte whose exact value
    lies within 0.01 of an integer may differ by 1 (the float32 atan2's last bits); every other byte is equal.  The colours of an image that
    holds a NaN or inf vector are unspecified.  `out`: a contiguous uint8 tensor of the result's shape to write.  float32, contiguous, on the
    GPU, or MpiFlowHipError.  Two launches, bit-identical from run to run, asynchronous on the current stream: no host copy, no
    synchronisation."""
    who = "flow_to_image"
    f = check_tensor(flow, "flow", who, (None, 2, None, None), "[N,2,H,W]")
    N, _, H, W = f.shape
    tensors = dict(flow=f)
    if image is not None:
        tensors["image"] = check_tensor(image, "image", who, (N, 3, H, W), "[N,3,H,W] like flow")
    rows = 2 * H if image is not None else H
    if out is not None:
        tensors["out"] = _check_out_int(out, who, torch.uint8, (N, rows, W, 3), "[N,2H,W,3]" if image is not None else "[N,H,W,3]")
    if N < 1 or H < 1 or W < 1:
        raise _lib.MpiFlowHipError("%s: flow must have at least one image and one pixel (got shape %s)" % (who, tuple(f.shape)))
    if clip_flow is not None:
        try:
            clip = float(clip_flow)
        except (TypeError, ValueError):
            clip = float("nan")
        if clip != clip:
            raise _lib.MpiFlowHipError("%s: clip_flow must be None or a number (got %r)" % (who, clip_flow))
        clip_flow = clip
    check_devices(who, tensors)
    lib = _lib.load()
    if out is None:
        out = torch.empty((N, rows, W, 3), dtype=torch.uint8, device=f.device)
    ws = torch.empty(int(lib.mpf_flow_to_image_workspace(N, H, W)) // 4, dtype=_f32, device=f.device)
    a = _lib.MpfFlowVizArgs()
    a.flow, a.image, a.out, a.N, a.H, a.W = f.data_ptr(), (image.data_ptr() if image is not None else None), out.data_ptr(), N, H, W
    a.clip, a.clip_flow, a.convert_to_bgr = int(clip_flow is not None), (clip_flow or 0.0), int(bool(convert_to_bgr))
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    _lib.check(lib.mpf_flow_to_image(ctypes.byref(a), _stream()), "mpf_flow_to_image")
    del ws
    return out


@_on_device
def flow_encode_kitti(flow, valid=None, out=None):
    """mpf_flow_encode_kitti: the array frame_utils.writeFlowKITTI hands to the PNG encoder, on the device: flow [N,2,H,W], valid [N,H,W] or None
    -> uint16 [N,H,W,3] = (64 * u + 2^15, 64 * v + 2^15, valid), the order the file holds as R, G, B (upstream passes cv2 the reverse, as B, G,
    R, and readFlowKITTI reverses what cv2 reads back).  Product and sum in float32, truncated toward zero, as upstream's astype(np.uint16).
    valid: 1 where valid >= 0.5, else 0; None: all ones, as upstream writes.  The one deviation: a code outside 0..65535 (|flow| >= 512 px),
    undefined in numpy, is clamped to 0 / 65535 (NaN: 0).  `out`: a contiguous uint16 tensor [N,H,W,3] to write.  float32, contiguous, on the
    GPU, or MpiFlowHipError.  One launch, asynchronous on the current stream."""
    who = "flow_encode_kitti"
    f = check_tensor(flow, "flow", who, (None, 2, None, None), "[N,2,H,W]")
    N, _, H, W = f.shape
    tensors = dict(flow=f)
    if valid is not None:
        tensors["valid"] = check_tensor(valid, "valid", who, (N, H, W), "[N,H,W] like flow")
    if out is not None:
        tensors["out"] = _check_out_int(out, who, torch.uint16, (N, H, W, 3), "[N,H,W,3]")
    if N < 1 or H < 1 or W < 1:
        raise _lib.MpiFlowHipError("%s: flow must have at least one image and one pixel (got shape %s)" % (who, tuple(f.shape)))
    check_devices(who, tensors)
    if out is None:
        out = torch.empty((N, H, W, 3), dtype=torch.uint16, device=f.device)
    a = _lib.MpfFlowVizArgs()
    a.flow, a.valid, a.out, a.N, a.H, a.W = f.data_ptr(), (valid.data_ptr() if valid is not None else None), out.data_ptr(), N, H, W
    _lib.check(_lib.load().mpf_flow_encode_kitti(ctypes.byref(a), _stream()), "mpf_flow_encode_kitti")
    return out


def _opt_table(who, columns, names):
    """The host table of mpf_grad_norm / mpf_adamw_clipped from parallel lists of tensors, `names` their names, the first column the one whose
    shape the others of a record must have and the LAST the gradients, where None skips the record.  Every tensor is held to the contract of
    _tensors.py in its order.  -> (MpfOptTensor array, device)"""
    n = len(columns[0])
    if n < 1 or any(len(c) != n for c in columns):
        raise _lib.MpiFlowHipError("%s: needs %s as lists of one length, at least 1 (got %s)" % (who, ", ".join(names), ", ".join(str(len(c)) for c in columns)))
    T = torch.Tensor
    dev = None
    fast = True
    for rec in zip(*columns):
        lead = rec[0] if rec[0] is not None else rec[-1]
        if lead is None:
            continue
        if not isinstance(lead, T):
            fast = False
            break
        shape = lead.shape
        dev = lead.device if dev is None else dev
        for t in rec:
            if t is None and t is rec[-1]:
                continue
            if not (isinstance(t, T) and t.dtype == _f32 and t.shape == shape and t.is_contiguous() and t.device == dev and t.is_cuda):
                fast = False
                break
        if not fast:
            break
    if not fast:                                                         # name the fault, in the contract's order
        tensors = {}
        for i, rec in enumerate(zip(*columns)):
            lead = rec[0] if rec[0] is not None else rec[-1]
            for name, t in zip(names, rec):
                if t is None and name == names[-1]:
                    continue
                if t is lead or not isinstance(lead, T):                 # its own shape is free; a lead that is no tensor is named first
                    shape, layout = (t.dim() if isinstance(t, T) else 0), None
                else:
                    shape, layout = tuple(lead.shape), "of the shape of its record's first tensor, %s" % (tuple(lead.shape),)
                tensors["%s[%d]" % (name, i)] = check_tensor(t, "%s[%d]" % (name, i), who, shape, layout)
        check_devices(who, tensors)
        raise AssertionError("unreachable: the fast check and the contract disagree")
    table = (_lib.MpfOptTensor * n)()
    fields = ("param", "exp_avg", "exp_avg_sq", "grad") if len(columns) == 4 else ("grad",)
    for i, rec in enumerate(zip(*columns)):
        r = table[i]
        lead = rec[0] if rec[0] is not None else rec[-1]
        r.numel = lead.numel() if lead is not None else 1
        if rec[-1] is None:
            continue                                                     # grad stays NULL: the library skips the record
        for f, t in zip(fields, rec):
            setattr(r, f, t.data_ptr())
    if dev is None:
        raise _lib.MpiFlowHipError("%s: every entry of %s is None: there is nothing to do and no device to do it on" % (who, names[-1]))
    return table, dev


def _opt_args(table, dev, workspace=None):
    """MpfAdamWArgs over `table` with total_norm [1] and the workspace (a new one, or the one an earlier grad_norm kept)"""
    lib = _lib.load()
    a = _lib.MpfAdamWArgs()
    a.tensors, a.count = table, len(table)
    total = torch.empty(1, dtype=_f32, device=dev)
    if workspace is None:
        need = int(lib.mpf_adamw_workspace(table, len(table)))
        if not need:
            raise _lib.MpiFlowHipError("mpf_adamw_workspace: %s" % lib.mpf_last_error().decode())
        workspace = torch.empty(need // 8, dtype=torch.float64, device=dev)
    a.total_norm, a.workspace, a.workspace_bytes = total.data_ptr(), workspace.data_ptr(), workspace.numel() * 8
    return a, total, workspace


@_on_device
def grad_norm(grads, keep_workspace=False):
    """mpf_grad_norm: what torch.nn.utils.clip_grad_norm_ returns, without touching a gradient: grads, a list of float32 tensors of any shapes on
    one GPU (None entries are skipped, as `p.grad is None`) -> the [1] float32 device tensor sqrt(sum of g * g), summed in float64 in a fixed
    order: bit-identical from run to run.  keep_workspace=True: -> (total_norm, workspace), the pair adamw_clipped's `norm` takes when several
    parameter groups share one global norm.  Asynchronous on the current stream: no host copy, no synchronisation."""
    who = "grad_norm"
    table, dev = _opt_table(who, [list(grads)], ("grads",))
    a, total, ws = _opt_args(table, dev)
    _lib.check(_lib.load().mpf_grad_norm(ctypes.byref(a), _stream()), "mpf_grad_norm")
    return (total, ws) if keep_workspace else total


@_on_device
def adamw_clipped(params, grads, exp_avgs, exp_avg_sqs, *, lr, betas, eps, weight_decay, step, max_norm, zero_grad=False, norm=None):
    """mpf_adamw_clipped: clip_grad_norm_(params, max_norm) and torch.optim.AdamW's update of step number `step` (1 for the first) over parallel
    lists of float32 tensors on one GPU, in place: params, exp_avgs, exp_avg_sqs are updated; grads are only read - NOT scaled, unlike
    clip_grad_norm_ - or, with zero_grad, overwritten by zeros.  A None in grads skips its record entirely.  Within a record the four tensors
    have one shape.  -> the [1] float32 device tensor total_norm, the norm before clipping.  max_norm=float('inf'): no clipping.
    norm: the (total_norm, workspace) of an earlier grad_norm(all_grads, keep_workspace=True) on this stream: the coefficient then comes from
    that norm (several parameter groups, one global norm) and the returned tensor is that norm again.
    Nothing is copied or cast; bit-identical from run to run.  Asynchronous on the current stream: no host copy, no synchronisation."""
    who = "adamw_clipped"
    table, dev = _opt_table(who, [list(params), list(exp_avgs), list(exp_avg_sqs), list(grads)], ("params", "exp_avgs", "exp_avg_sqs", "grads"))
    try:
        step = operator.index(step)
    except TypeError:
        step = 0
    if step < 1:
        raise _lib.MpiFlowHipError("%s: step must be an integer, 1 for the first update (got %r)" % (who, step))
    beta1, beta2 = (float(b) for b in betas)
    if norm is not None:
        if not (isinstance(norm, tuple) and len(norm) == 2 and isinstance(norm[1], torch.Tensor) and norm[1].dtype == torch.float64 and norm[1].dim() == 1
                and norm[1].is_contiguous()):
            raise _lib.MpiFlowHipError("%s: norm must be the (total_norm, workspace) pair of grad_norm(..., keep_workspace=True)" % who)
        if norm[1].device != dev:
            raise _lib.MpiFlowHipError("%s: norm was computed on %s, the tensors live on %s" % (who, norm[1].device, dev))
    a, total, ws = _opt_args(table, dev, None if norm is None else norm[1])
    a.norm_ready = 0 if norm is None else 1
    a.zero_grad = 1 if zero_grad else 0
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.max_norm = float(lr), beta1, beta2, float(eps), float(weight_decay), float(max_norm)
    a.bias_correction1 = 1.0 - beta1 ** step
    a.bias_correction2_sqrt = (1.0 - beta2 ** step) ** 0.5
    _lib.check(_lib.load().mpf_adamw_clipped(ctypes.byref(a), _stream()), "mpf_adamw_clipped")
    del ws
    return total


@_on_device
def to_u8_bgr(img_3HW):
    lib = _lib.load()
    img = _dev(img_3HW, "img")
    _, H, W = img.shape
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=img.device)
    _lib.check(lib.mpf_to_u8_bgr(_ptr(img), H, W, _ptr(out), _stream()), "mpf_to_u8_bgr")
    return out


# ---- generic ops ----------------------------------------------------------------------------------------------------

@_on_device
def src_xyz(K_inv, depth_S, H, W, device):
    lib = _lib.load()
    d = host_math._cpu32(depth_S).reshape(-1)
    S = d.numel()
    dparams = upload_params(host_math.pack_params(K_inv=K_inv, depths=d), device)
    out = torch.empty((S, 3, H, W), dtype=_f32, device=device)
    _lib.check(lib.mpf_src_xyz(_ptr(dparams), S, H, W, _ptr(out), _stream()), "mpf_src_xyz")
    return out


def _plane_sum_workspace(S, H, W, device):
    """the [blocks, S] partial sums of the per-plane reductions (one row per 256-pixel workgroup) and the [S] result"""
    blocks = (H * W + 255) // 256
    return torch.empty((blocks, S), dtype=_f32, device=device), blocks, torch.empty((S,), dtype=_f32, device=device)


@_on_device
def src_xyz_backward(g_xyz_S3HW, K_inv, depth_S):
    """Adjoint of src_xyz with respect to the plane disparities (mpf_src_xyz_bwd): g_xyz [S,3,H,W], the forward's K_inv and depths -> [S],
    dL/ddisparity_s = -depth_s^2 sum_p <g_s(p), K^-1 (x, y, 1)>.  No atomics: two runs give the same bits."""
    lib = _lib.load()
    g = _dev(g_xyz_S3HW, "g_xyz")
    S, C, H, W = g.shape
    assert C == 3
    d = host_math._cpu32(depth_S).reshape(-1)
    assert d.numel() == S
    dparams = upload_params(host_math.pack_params(K_inv=K_inv, depths=d), g.device)
    partial, blocks, out = _plane_sum_workspace(S, H, W, g.device)
    _lib.check(lib.mpf_src_xyz_bwd(_ptr(g), _ptr(dparams), S, H, W, _ptr(partial), blocks, _ptr(out), _stream()), "mpf_src_xyz_bwd")
    return out


@_on_device
def plane_flow_backward(g_flow_SHW2, H_tgt_src, depth_S, Kt_t_S3, Kinv_row3_S3):
    """Adjoint of homography_flow with respect to the plane depths d_s of H_s = K_tgt (R + t n^T / d_s) K_src^-1 (mpf_plane_flow_bwd): g_flow [S,H,W,2], the
    forward's H_tgt_src [S,3,3], the depths [S], K_tgt t [S,3] and the third row of K_src^-1 [S,3] -> [S].  No atomics: two runs give the same bits."""
    lib = _lib.load()
    g = _dev(g_flow_SHW2, "g_flow")
    S, H, W, two = g.shape
    assert two == 2
    buf = host_math.pack_params(homs=host_math._cpu32(H_tgt_src).reshape(S, 3, 3), depths=host_math._cpu32(depth_S).reshape(S))
    rec = buf[host_math.PARAMS_HEADER:].view(-1, host_math.PLANE_RECORD)
    rec[:S, 10:13] = host_math._cpu32(Kt_t_S3).reshape(S, 3)
    rec[:S, 13:16] = host_math._cpu32(Kinv_row3_S3).reshape(S, 3)
    dparams = upload_params(buf, g.device)
    partial, blocks, out = _plane_sum_workspace(S, H, W, g.device)
    _lib.check(lib.mpf_plane_flow_bwd(_ptr(g), _ptr(dparams), S, H, W, _ptr(partial), blocks, _ptr(out), _stream()), "mpf_plane_flow_bwd")
    return out


@_on_device
def transform_xyz(G, xyz_S3N):
    lib = _lib.load()
    xyz = _dev(xyz_S3N, "xyz")
    S = xyz.shape[0]
    N = xyz[0, 0].numel()
    dparams = upload_params(host_math.pack_params(G=G, records=1), xyz.device)
    out = torch.empty_like(xyz)
    _lib.check(lib.mpf_transform_xyz(_ptr(dparams), _ptr(xyz), S, N, _ptr(out), _stream()), "mpf_transform_xyz")
    return out


@_on_device
def homography_sample(src_SCHW, H_src_tgt, want_flow=True):
    lib = _lib.load()
    src = _dev(src_SCHW, "src")
    S, C, H, W = src.shape
    dparams = upload_params(host_math.pack_params(homs=host_math._cpu32(H_src_tgt).reshape(S, 3, 3)), src.device)
    tgt = torch.empty_like(src)
    valid = torch.empty((S, H, W), dtype=torch.uint8, device=src.device)
    flow = torch.empty((S, H, W, 2), dtype=_f32, device=src.device) if want_flow else None
    _lib.check(lib.mpf_homography_sample(_ptr(src), _ptr(dparams), S, C, H, W, _ptr(tgt), _ptr(valid), _ptr(flow), _stream()),
               "mpf_homography_sample")
    return tgt, valid.to(torch.bool), flow


@_on_device
def homography_sample_backward(g_tgt_SCHW, H_src_tgt, c0=0, c1=None, grad_src=None):
    """Adjoint of homography_sample with respect to src for the channels [c0, c1) (mpf_homography_sample_bwd): grad_src [S,C,H,W] += weight * g_tgt through
    the taps the forward read.  grad_src: a zero-initialised buffer to add into (allocated zeroed when None); channels outside the range stay as they
    are.  The adds are float atomics: their arrival order decides the last bits of each sum."""
    lib = _lib.load()
    g = _dev(g_tgt_SCHW, "g_tgt")
    S, C, H, W = g.shape
    c1 = C if c1 is None else c1
    dparams = upload_params(host_math.pack_params(homs=host_math._cpu32(H_src_tgt).reshape(S, 3, 3)), g.device)
    grad_src = _grad_buffer(grad_src, "grad_src", (S, C, H, W), g.device, True)
    _lib.check(lib.mpf_homography_sample_bwd(_ptr(g), _ptr(dparams), S, C, H, W, int(c0), int(c1), _ptr(grad_src), _stream()),
               "mpf_homography_sample_bwd")
    return grad_src


@_on_device
def homography_flow(H_tgt_src, H, W, device):
    lib = _lib.load()
    hts = host_math._cpu32(H_tgt_src).reshape(-1, 3, 3)
    S = hts.shape[0]
    dparams = upload_params(host_math.pack_params(homs=hts), device)
    flow = torch.empty((S, H, W, 2), dtype=_f32, device=device)
    _lib.check(lib.mpf_homography_flow(_ptr(dparams), S, H, W, _ptr(flow), _stream()), "mpf_homography_flow")
    return flow


@_on_device
def volume_render(rgb_S3N, sigma_SN, xyz_S3N, extra_SEN=None, hard=False, want_tacc=True, want_weights=True):
    """Generic plane_volume_rendering on materialised tensors.  Trailing dims are flattened to N."""
    lib = _lib.load()
    xyz = _dev(xyz_S3N, "xyz")
    S = xyz.shape[0]
    tail = tuple(xyz.shape[2:])
    N = xyz[0, 0].numel()
    sigma = _dev(sigma_SN, "sigma")
    rgb = _dev(rgb_S3N, "rgb") if rgb_S3N is not None else None
    extra = _dev(extra_SEN, "extra") if extra_SEN is not None else None
    E = 0 if extra is None else extra.shape[1]
    dev = xyz.device
    out = dict(rgb=torch.empty((3,) + tail, dtype=_f32, device=dev) if rgb is not None else None,
               depth=torch.empty(tail, dtype=_f32, device=dev),
               tacc=torch.empty((S,) + tail, dtype=_f32, device=dev) if want_tacc else None,
               weights=torch.empty((S,) + tail, dtype=_f32, device=dev) if want_weights else None,
               extra=torch.empty((E,) + tail, dtype=_f32, device=dev) if E else None)
    _lib.check(lib.mpf_volume_render(_ptr(rgb), _ptr(sigma), _ptr(xyz), S, N, _ptr(out["rgb"]), _ptr(out["depth"]),
                                     _ptr(out["tacc"]), _ptr(out["weights"]), _ptr(extra), E, _ptr(out["extra"]),
                                     int(bool(hard)), _stream()), "mpf_volume_render")
    return out


@_on_device
def volume_render_backward(rgb_S3N, sigma_SN, xyz_S3N, extra_SEN=None, hard=False, g_rgb=None, g_depth=None, g_extra=None, g_weights=None, g_tacc=None,
                           want_rgb=True, want_extra=True, want_xyz=False):
    """Adjoint of volume_render with respect to rgb, sigma and the extras (mpf_volume_render_bwd) and, with want_xyz, with respect to xyz
    (mpf_volume_render_bwd_xyz).  The same inputs as the forward call and the upstream gradient of each output that was used (None otherwise).
    -> dict(rgb [S,3,*tail] | None, sigma [S,*tail], extra [S,E,*tail] | None, xyz [S,3,*tail] | None)."""
    lib = _lib.load()
    xyz = _dev(xyz_S3N, "xyz")
    S = xyz.shape[0]
    tail = tuple(xyz.shape[2:])
    N = xyz[0, 0].numel()
    sigma = _dev(sigma_SN, "sigma")
    rgb = _dev(rgb_S3N, "rgb") if rgb_S3N is not None else None
    extra = _dev(extra_SEN, "extra") if extra_SEN is not None else None
    E = 0 if extra is None else extra.shape[1]
    dev = xyz.device

    def up(t, name, lead):
        if t is None:
            return None
        t = _dev(t, name)
        if t.numel() != lead * N:
            raise _lib.MpiFlowHipError("%s has %d elements, expected %d" % (name, t.numel(), lead * N))
        return t

    gr, gd, ge = up(g_rgb if rgb is not None else None, "g_rgb", 3), up(g_depth, "g_depth", 1), up(g_extra if E else None, "g_extra", E)
    gw, ga = up(g_weights, "g_weights", S), up(g_tacc, "g_tacc", S)
    out = dict(rgb=torch.empty((S, 3) + tail, dtype=_f32, device=dev) if (rgb is not None and want_rgb) else None,
               sigma=torch.empty((S,) + tail, dtype=_f32, device=dev),
               extra=torch.empty((S, E) + tail, dtype=_f32, device=dev) if (E and want_extra) else None,
               xyz=torch.empty((S, 3) + tail, dtype=_f32, device=dev) if want_xyz else None)
    if want_xyz:
        _lib.check(lib.mpf_volume_render_bwd_xyz(_ptr(rgb), _ptr(sigma), _ptr(xyz), _ptr(extra), S, N, E, int(bool(hard)), _ptr(gr), _ptr(gd), _ptr(ge),
                                                 _ptr(gw), _ptr(ga), _ptr(out["rgb"]), _ptr(out["sigma"]), _ptr(out["extra"]), _ptr(out["xyz"]), _stream()),
                   "mpf_volume_render_bwd_xyz")
        return out
    _lib.check(lib.mpf_volume_render_bwd(_ptr(rgb), _ptr(sigma), _ptr(xyz), _ptr(extra), S, N, E, int(bool(hard)), _ptr(gr), _ptr(gd), _ptr(ge), _ptr(gw),
                                         _ptr(ga), _ptr(out["rgb"]), _ptr(out["sigma"]), _ptr(out["extra"]), _stream()), "mpf_volume_render_bwd")
    return out


@_on_device
def weighted_sum(weights_SN, values_SCN=None):
    """cascade-sum over S of weights (* values).  weights [S,*tail], values [S,C,*tail] -> [C,*tail] ([1,*tail] if None)"""
    lib = _lib.load()
    w = _dev(weights_SN, "weights")
    S = w.shape[0]
    tail = tuple(w.shape[1:])
    N = w[0].numel()
    v = _dev(values_SCN, "values") if values_SCN is not None else None
    C = v.shape[1] if v is not None else 1
    out = torch.empty((C,) + tail, dtype=_f32, device=w.device)
    _lib.check(lib.mpf_weighted_sum(_ptr(w), _ptr(v), S, C, N, _ptr(out), _stream()), "mpf_weighted_sum")
    return out


# ---- depth -> flow, forward warp -----------------------------------------------------------------------------------

@_on_device
def alpha_composite(alpha_SN, values_SCN=None, want_weights=True, want_cumprod_eps=False):
    """alpha_composition (mpi_rendering.py:42-59) -> dict(out [C,N] | None, weights [S,N] | None, cumprod_eps [S,N] | None)"""
    lib = _lib.load()
    al = _dev(alpha_SN, "alpha")
    S, N = al.shape[0], al[0].numel()
    al = al.reshape(S, N)
    dev = al.device
    vals = out = None
    C = 1
    if values_SCN is not None:
        vals = _dev(values_SCN, "values")
        C = vals.shape[1]
        vals = vals.reshape(S, C, N)
        out = torch.empty((C, N), dtype=_f32, device=dev)
    w = torch.empty((S, N), dtype=_f32, device=dev) if want_weights else None
    ce = torch.empty((S, N), dtype=_f32, device=dev) if want_cumprod_eps else None
    _lib.check(lib.mpf_alpha_composite(_ptr(al), _ptr(vals), S, C, ctypes.c_int64(N), _ptr(out), _ptr(w), _ptr(ce), _stream()), "mpf_alpha_composite")
    return dict(out=out, weights=w, cumprod_eps=ce)


@_on_device
def disp_to_depth(disp):
    lib = _lib.load()
    d = _dev(disp, "disp")
    out = torch.empty_like(d)
    _lib.check(lib.mpf_disp_to_depth(_ptr(d), d.numel(), _ptr(out), _stream()), "mpf_disp_to_depth")
    return out


@_on_device
def backproject_project(depth_HW, inv_K33, P34):
    lib = _lib.load()
    depth = _dev(depth_HW, "depth")
    H, W = depth.shape[-2:]
    depth = depth.reshape(H, W)
    ik = host_math._cpu32(inv_K33).reshape(9).contiguous()
    P = host_math._cpu32(P34).reshape(12).contiguous()
    pix = torch.empty((H, W, 2), dtype=_f32, device=depth.device)
    z = torch.empty((H, W), dtype=_f32, device=depth.device)
    _lib.check(lib.mpf_backproject_project(_ptr(depth), ctypes.c_void_p(ik.data_ptr()), ctypes.c_void_p(P.data_ptr()), H, W,
                                           _ptr(pix), _ptr(z), _stream()), "mpf_backproject_project")
    return pix, z


@_on_device
def backproject(depth_HW, inv_K33):
    """BackprojectDepth.forward -> [4, H*W] camera points (rows X, Y, Z, 1)"""
    lib = _lib.load()
    depth = _dev(depth_HW, "depth")
    H, W = depth.shape[-2:]
    ik = host_math._cpu32(inv_K33).reshape(9).contiguous()
    cam = torch.empty((4, H * W), dtype=_f32, device=depth.device)
    _lib.check(lib.mpf_backproject(_ptr(depth.reshape(H, W)), ctypes.c_void_p(ik.data_ptr()), H, W, _ptr(cam), _stream()), "mpf_backproject")
    return cam


@_on_device
def project3d(points_4N, P34, H, W, eps=1e-7):
    """Project3D.forward on homogeneous points [4, H*W] -> (pix [H,W,2] normalised, z [H*W])"""
    lib = _lib.load()
    pts = _dev(points_4N, "points").reshape(4, H * W)
    P = host_math._cpu32(P34).reshape(12).contiguous()
    pix = torch.empty((H, W, 2), dtype=_f32, device=pts.device)
    z = torch.empty((H * W,), dtype=_f32, device=pts.device)
    _lib.check(lib.mpf_project3d(_ptr(pts), ctypes.c_void_p(P.data_ptr()), float(eps), H, W, _ptr(pix), _ptr(z), _stream()), "mpf_project3d")
    return pix, z


@_on_device
def select_truncate(p_static, z_static, p_obj, z_obj, inst_HW):
    lib = _lib.load()
    inst = _dev(inst_HW, "instance mask")
    H, W = inst.shape[-2:]
    dev = inst.device
    p1 = torch.empty((H, W, 2), dtype=_f32, device=dev)
    z1 = torch.empty((H, W), dtype=_f32, device=dev)
    sx = torch.empty((H, W), dtype=torch.int64, device=dev)
    sy = torch.empty((H, W), dtype=torch.int64, device=dev)
    fl = torch.empty((H, W, 2), dtype=_f32, device=dev)
    _lib.check(lib.mpf_select_truncate(_ptr(_dev(p_static, "p_static")), _ptr(_dev(z_static, "z_static")),
                                       _ptr(_dev(p_obj, "p_obj")), _ptr(_dev(z_obj, "z_obj")), _ptr(inst.reshape(H, W)), H, W,
                                       _ptr(p1), _ptr(z1), _ptr(sx), _ptr(sy), _ptr(fl), _stream()), "mpf_select_truncate")
    return p1, z1, sx, sy, fl


@_on_device
def moving_object_project(disp_HW, inv_K33, P_static34, P_obj34, inst_HW):
    """Fused moving_obj.py:29-124: -> (p1 [H,W,2], z1 [H,W], safe_x, safe_y int64 [H,W], flow01 [H,W,2])"""
    lib = _lib.load()
    disp = _dev(disp_HW, "disp")
    H, W = disp.shape[-2:]
    dev = disp.device
    inst = _dev(inst_HW, "instance mask").reshape(H, W)
    ik = host_math._cpu32(inv_K33).reshape(9).contiguous()
    Ps = host_math._cpu32(P_static34).reshape(12).contiguous()
    Po = host_math._cpu32(P_obj34).reshape(12).contiguous()
    p1 = torch.empty((H, W, 2), dtype=_f32, device=dev)
    z1 = torch.empty((H, W), dtype=_f32, device=dev)
    sx = torch.empty((H, W), dtype=torch.int64, device=dev)
    sy = torch.empty((H, W), dtype=torch.int64, device=dev)
    fl = torch.empty((H, W, 2), dtype=_f32, device=dev)
    _lib.check(lib.mpf_moving_object_project(_ptr(disp.reshape(H, W)), ctypes.c_void_p(ik.data_ptr()), ctypes.c_void_p(Ps.data_ptr()),
                                             ctypes.c_void_p(Po.data_ptr()), _ptr(inst), H, W, _ptr(p1), _ptr(z1), _ptr(sx), _ptr(sy),
                                             _ptr(fl), _stream()), "mpf_moving_object_project")
    return p1, z1, sx, sy, fl


@_on_device
def forward_warp(src_u8, idx_i64, idy_i64, z_f32, h, w):
    """Device-resident forward splat, byte-identical to the reference's serial C.  -> warped u8 [h,w,5]"""
    lib = _lib.load()
    src = _dev(src_u8, "src", torch.uint8).reshape(-1)
    idx = _dev(idx_i64, "idx", torch.int64).reshape(-1)
    idy = _dev(idy_i64, "idy", torch.int64).reshape(-1)
    z = _dev(z_f32, "z").reshape(-1)
    assert src.numel() == h * w * 3 and idx.numel() == h * w and idy.numel() == h * w and z.numel() == h * w
    ws_bytes = lib.mpf_forward_warp_workspace(h, w)
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=src.device)
    off = (-ws.data_ptr()) % 256
    warped = torch.empty((h, w, 5), dtype=torch.uint8, device=src.device)
    _lib.check(lib.mpf_forward_warp(_ptr(src), _ptr(idx), _ptr(idy), _ptr(z), _ptr(warped), h, w,
                                    ctypes.c_void_p(ws.data_ptr() + off), ws_bytes, _stream()), "mpf_forward_warp")
    return warped


@_on_device
def warp_masks(warped_HW5):
    lib = _lib.load()
    w5 = _dev(warped_HW5, "warped", torch.uint8)
    H, W, _ = w5.shape
    outs = [torch.empty((H, W), dtype=torch.uint8, device=w5.device) for _ in range(5)]
    _lib.check(lib.mpf_warp_masks(_ptr(w5), H, W, *[_ptr(o) for o in outs], _stream()), "mpf_warp_masks")
    return dict(zip(["H", "M", "M'", "P", "H'"], outs))


class MovingObjectBuffers:
    """Preallocated outputs + sort workspace of mpf_moving_object_chain for one (H, W) on one device (28 N bytes of results)."""

    def __init__(self, H, W, device):
        lib = _lib.load()
        dev = torch.device(device)
        u8 = torch.uint8
        self.H, self.W, self.device = H, W, dev
        self.p1 = torch.empty((H, W, 2), dtype=_f32, device=dev)
        self.z1 = torch.empty((H, W), dtype=_f32, device=dev)
        self.safe_x = torch.empty((H, W), dtype=torch.int64, device=dev)
        self.safe_y = torch.empty((H, W), dtype=torch.int64, device=dev)
        self.flow_01 = torch.empty((H, W, 2), dtype=_f32, device=dev)
        self.warped = torch.empty((H, W, 5), dtype=u8, device=dev)
        self.masks = {k: torch.empty((H, W), dtype=u8, device=dev) for k in ("H", "M", "M'", "P", "H'")}
        self.ws_bytes = lib.mpf_forward_warp_workspace(H, W)
        self._ws = torch.empty(self.ws_bytes + 256, dtype=u8, device=dev)
        self.ws_ptr = self._ws.data_ptr() + (-self._ws.data_ptr()) % 256
        m = self.masks
        self.ready = None        # set by pipeline.OverlappedPairRenderer (unordered chain): torch event recorded behind the launches that fill this set
        self.consumed = None     # optional, set by the consumer: torch event the side stream waits for before it rewrites this set
        self.c_out = _lib.MpfMovingObjectOut(self.p1.data_ptr(), self.z1.data_ptr(), self.safe_x.data_ptr(), self.safe_y.data_ptr(),
                                             self.flow_01.data_ptr(), self.warped.data_ptr(), m["H"].data_ptr(), m["M"].data_ptr(),
                                             m["M'"].data_ptr(), m["P"].data_ptr(), m["H'"].data_ptr())

    def as_dict(self):
        return dict(p1=self.p1, z1=self.z1, safe_x=self.safe_x, safe_y=self.safe_y, flow_01=self.flow_01, warped=self.warped, masks=self.masks)


@_on_device
def moving_object_chain(disp_HW, inv_K33, P_static34, P_obj34, inst_HW, src, bufs=None):
    """moving_obj.py:29-150 in one call (mpf_moving_object_chain): projection fused into the forward warp's first sort pass, splat, masks.
    src: the frame that is splatted - uint8 [H,W,3], or float32 [3,H,W] in 0..1 (its uint8 BGR form is splatted, converted on the fly).
    -> MovingObjectBuffers (bufs or a new one)"""
    lib = _lib.load()
    disp = _dev(disp_HW, "disp")
    H, W = disp.shape[-2:]
    inst = _dev(inst_HW, "instance mask")
    as_float = src.dtype != torch.uint8
    src = _dev(src, "src", _f32 if as_float else torch.uint8)
    assert inst.numel() == H * W and src.numel() == H * W * 3 and (not as_float or tuple(src.shape[-3:]) == (3, H, W))
    if bufs is None:
        bufs = MovingObjectBuffers(H, W, disp.device)
    assert (bufs.H, bufs.W) == (H, W) and bufs.device == disp.device
    ik = host_math._cpu32(inv_K33).reshape(9).contiguous()
    Ps = host_math._cpu32(P_static34).reshape(12).contiguous()
    Po = host_math._cpu32(P_obj34).reshape(12).contiguous()
    _lib.check(lib.mpf_moving_object_chain(_ptr(disp), ctypes.c_void_p(ik.data_ptr()), ctypes.c_void_p(Ps.data_ptr()), ctypes.c_void_p(Po.data_ptr()),
                                           _ptr(inst), None if as_float else _ptr(src), _ptr(src) if as_float else None, H, W, ctypes.byref(bufs.c_out), ctypes.c_void_p(bufs.ws_ptr), bufs.ws_bytes,
                                           _stream()), "mpf_moving_object_chain")
    return bufs
