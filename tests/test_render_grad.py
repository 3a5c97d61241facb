"""The differentiable utils/mpi renderer against the reference's own float64 autograd (tests/golden/render_grad.npz, written by
tests/golden/make_render_grad_golden.py): the three backward kernels through ops, every public function through .backward(), forward bits, the fused
form's memory, the refusals and the degenerate stacks.

Tolerance (per gradient tensor, nothing excluded): max|g_hip - g64| / max|g64| <= max(4 * e_ref, 1e-6), e_ref = max|g32_ref - g64| / max|g64| being
the reference's own float32 autograd against its float64, as the golden carries it.  The factor 4 covers what two float32 evaluations of the same sums
may legitimately differ by - the forward's cascade order over S and the order of the atomic adds -, the floor keeps a luckily tiny e_ref from becoming
a bit-exactness demand.  A gradient that is identically zero in float64 must be identically zero here."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, bits_equal, load_golden

sys.path.insert(0, GOLDEN)
import make_render_grad_golden as mk  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def gold():
    import __graft_entry__ as ge
    ge.build()
    return load_golden("render_grad")


def t(x, grad=False):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV).requires_grad_(grad)


def check(gold, prefix, name, g_hip, report):
    g64 = gold[prefix + "g64/" + name]
    e_ref = float(gold[prefix + "e_ref/" + name])
    g = g_hip.detach().cpu().numpy().astype(np.float64).reshape(g64.shape)
    assert np.isfinite(g).all(), (prefix, name)
    scale = np.abs(g64).max()
    if scale == 0.0:
        print("%s%s: identically zero in float64; max|g_hip| %.3e" % (prefix, name, np.abs(g).max()))
        assert np.abs(g).max() == 0.0, (prefix, name)
        return
    err, bar = np.abs(g - g64).max() / scale, max(4.0 * e_ref, 1e-6)
    print("%s%s: err %.3e  e_ref %.3e  bar %.3e" % (prefix, name, err, e_ref, bar))
    report.append((prefix + name, err, bar))


def settle(report):
    bad = [r for r in report if not r[1] <= r[2]]
    assert not bad, bad


def geometry(S, b=mk.B, h=mk.H, w=mk.W):
    """our sampler and tagged xyz tensors for the golden's poses"""
    from mpiflow_amd.utils.mpi import mpi_rendering as R
    from mpiflow_amd.utils.mpi.homography_sampler import HomographySample
    disp, G, K, Kinv = (torch.from_numpy(a) for a in mk.geometry(S, h, w, b))
    sampler = HomographySample(h, w, torch.device(DEV))
    xs = R.get_src_xyz_from_plane_disparity(sampler.meshgrid, disp.to(DEV), Kinv)
    xt = R.get_tgt_xyz_from_plane_disparity(xs, G)
    return R, sampler, xs, xt, disp, G, K, Kinv


def rep(m, S):
    return m.unsqueeze(1).repeat(1, S, 1, 1).reshape(m.shape[0] * S, m.shape[-2], m.shape[-1])


# ---- 1. kernels through ops, public functions through .backward() -------------------------------------------------------------------------

@pytest.mark.parametrize("name,S", [("s1", 1), ("s5", 5)])
def test_sample_backward_kernel_and_function(gold, name, S):
    from mpiflow_amd import ops
    p = "sample/%s/" % name
    d = mk.draw(int(gold[p + "seed"]), S, False)
    src = np.concatenate([d["rgb"], d["sigma"]], axis=2).reshape(mk.B * S, 4, mk.H, mk.W)
    assert abs(src.astype(np.float64).sum() + d["g_tgt"].astype(np.float64).sum() - float(gold[p + "input_sum"])) < 1e-6
    R, sampler, xs, xt, disp, G, K, Kinv = geometry(S)
    leaf = t(src, True)
    args = (torch.reciprocal(disp).view(-1), rep(G, S), rep(Kinv, S), rep(K, S))
    tgt, valid, flow = sampler.sample(leaf, *args)
    assert tgt.grad_fn is not None and not valid.requires_grad and not flow.requires_grad
    with torch.no_grad():
        tgt0, valid0, flow0 = sampler.sample(leaf, *args)
    assert tgt0.grad_fn is None
    assert bits_equal(tgt.detach().cpu().numpy(), tgt0.cpu().numpy()) == 0 and bits_equal(flow.cpu().numpy(), flow0.cpu().numpy()) == 0      # 2.
    tgt.backward(t(d["g_tgt"]))
    report = []
    check(gold, p, "src", leaf.grad, report)
    # the kernel itself: two channel ranges into one buffer == the whole range; the channels outside a range stay untouched
    H_ts = sampler._homographies(*args)
    from mpiflow_amd.utils.mpi.homography_sampler import inverse
    H_st = inverse(H_ts.to(torch.float64)).to(torch.float32)
    g = ops.homography_sample_backward(t(d["g_tgt"]), H_st, 0, 3)
    assert float(g[:, 3].abs().max()) == 0.0
    g = ops.homography_sample_backward(t(d["g_tgt"]), H_st, 3, 4, grad_src=g)
    check(gold, p, "src", g, report)
    if name == "s5":                         # 6. the plane no target pixel sees gets what the border-clamped taps dictate: finite, equal to the golden
        assert int(gold["coverage/s5/planes_all_invalid"]) >= 1
        dead = [i for i in range(mk.B * S) if not bool(valid[i].any())]
        assert dead and np.isfinite(leaf.grad[dead].cpu().numpy()).all() and float(leaf.grad[dead].abs().max()) > 0
    settle(report)


RENDER = {"s1_mask": (1, True, False, True), "s5_mask": (5, True, False, True), "s5_mask_hard": (5, True, True, True), "s5_plain": (5, False, False, False)}


@pytest.mark.parametrize("name", list(RENDER))
def test_render_backward(gold, name):
    S, with_mask, hard, with_src = RENDER[name]
    p = "render/%s/" % name
    base = "render/s5_mask/" if hard else p           # hard_flow shares its base case's draw; only src_sigma / src_flow differ
    assert list(gold[p + "settings"]) == [S, int(with_mask), int(hard), int(with_src)]
    d = mk.draw(int(gold[p + "seed"]), S, with_mask)
    assert abs(mk.input_sum(d) - float(gold[p + "input_sum"])) < 1e-6
    R, sampler, xs, xt, *_ = geometry(S)
    leaves = dict(rgb=t(d["rgb"], True), sigma=t(d["sigma"], True), src_sigma=t(d["src_sigma"], True) if with_src else None,
                  src_flow=t(d["src_flow"], True) if with_src else None, obj_mask=t(d["obj_mask"], True) if with_mask else None)
    call = lambda: R.render(leaves["rgb"], leaves["sigma"], xt, leaves["src_sigma"], leaves["src_flow"], xs if with_src else None, hard_flow=hard,
                            obj_mask=leaves["obj_mask"])
    out = call()
    with torch.no_grad():
        out0 = call()
    ups = [d["g_rgb"], d["g_depth"], d["g_tacc"], d["g_weights"], d["g_flow"], d["g_mask"]]
    for o, o0 in zip(out, out0):                                                                                                                     # 2., 5.
        if o is not None:
            assert o.grad_fn is not None and o0.grad_fn is None
            assert bits_equal(o.detach().cpu().numpy(), o0.cpu().numpy()) == 0
    torch.autograd.backward([o for o in out if o is not None], [t(u) for o, u in zip(out, ups) if o is not None])
    report = []
    for k, leaf in leaves.items():
        if leaf is not None:
            check(gold, p if (not hard or k in ("src_sigma", "src_flow")) else base, k, leaf.grad, report)
    settle(report)


def test_volume_render_backward_kernel(gold):
    """mpf_volume_render_bwd through ops on one batch item, all five upstream gradients, against the golden's render case"""
    from mpiflow_amd import ops
    p, S = "render/s5_mask/", 5
    d = mk.draw(int(gold[p + "seed"]), S, True)
    R, sampler, xs, xt, *_ = geometry(S)
    report = []
    g_rgb, g_sigma, g_mask, g_ssig, g_flow = [], [], [], [], []
    for b in range(mk.B):
        # render() keeps plane_volume_rendering's mask and drops its flow: the flow's upstream gradient is zero there ...
        extra = torch.cat([t(d["src_flow"][b]), t(d["obj_mask"][b])], dim=1).contiguous()
        g = ops.volume_render_backward(t(d["rgb"][b]), t(d["sigma"][b, :, 0]), xt[b], extra, g_rgb=t(d["g_rgb"][b]), g_depth=t(d["g_depth"][b, 0]),
                                       g_extra=torch.cat([torch.zeros_like(t(d["g_flow"][b])), t(d["g_mask"][b])]), g_weights=t(d["g_weights"][b, :, 0]),
                                       g_tacc=t(d["g_tacc"][b, :, 0]))
        g_rgb.append(g["rgb"]); g_sigma.append(g["sigma"]); g_mask.append(g["extra"][:, 2:3])
        # ... and flowA2B comes from the flow form (rgb == NULL) on the source-frame density
        f = ops.volume_render_backward(None, t(d["src_sigma"][b, :, 0]), xs[b], t(d["src_flow"][b]), g_extra=t(d["g_flow"][b]))
        assert f["rgb"] is None
        g_ssig.append(f["sigma"]); g_flow.append(f["extra"])
    check(gold, p, "rgb", torch.stack(g_rgb), report)
    check(gold, p, "sigma", torch.stack(g_sigma), report)
    check(gold, p, "obj_mask", torch.stack(g_mask), report)
    check(gold, p, "src_sigma", torch.stack(g_ssig), report)
    check(gold, p, "src_flow", torch.stack(g_flow), report)
    settle(report)


RTD = {"s1_mask": (1, False), "s5_mask": (5, False), "s5_mask_hard": (5, True)}


def rtd_call(gold, name, fused, with_mask=True, mask_grad=True):
    S, hard = RTD[name]
    p = "rtd/%s/" % name
    d = mk.draw(int(gold[p + "seed"]), S, True)
    assert abs(mk.input_sum(d) - float(gold[p + "input_sum"])) < 1e-6
    R, sampler, xs, xt, disp, G, K, Kinv = geometry(S)
    leaves = dict(mpi_rgb_src=t(d["rgb"], True), mpi_sigma_src=t(d["sigma"], True), obj_mask=t(d["obj_mask"], mask_grad) if with_mask else None)
    call = lambda: R.render_tgt_rgb_depth(sampler, leaves["mpi_rgb_src"], leaves["mpi_sigma_src"], disp.to(DEV), xt, xs, G, Kinv, K, hard_flow=hard,
                                          obj_mask=leaves["obj_mask"], fused=fused)
    return d, leaves, call


@pytest.mark.parametrize("name", list(RTD))
def test_render_tgt_rgb_depth_generic_backward(gold, name):
    d, leaves, call = rtd_call(gold, name, fused=False)
    rgb, depth, tgt_mask, flow, om = call()
    with torch.no_grad():
        out0 = call()
    for o, o0 in zip((rgb, depth, tgt_mask, flow, om), out0):
        assert bits_equal(o.detach().cpu().numpy(), o0.cpu().numpy()) == 0 and o0.grad_fn is None
    assert not tgt_mask.requires_grad and flow.grad_fn is not None
    torch.autograd.backward([rgb, depth, flow, om], [t(d["g_rgb"]), t(d["g_depth"]), t(d["g_flow2"]), t(d["g_mask"])])
    report = []
    hard = RTD[name][1]
    for k, leaf in leaves.items():
        check(gold, "rtd/%s/full/" % (name if (not hard or k == "mpi_sigma_src") else "s5_mask"), k, leaf.grad, report)
    settle(report)


# ---- 3. the fused backward ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,with_mask", [("s1_mask", True), ("s5_mask", True), ("s5_mask", False)])
def test_render_tgt_rgb_depth_fused_backward(gold, name, with_mask):
    from mpiflow_amd import ops
    d, leaves, call = rtd_call(gold, name, fused=None, with_mask=with_mask, mask_grad=False)
    called = []
    real = ops.warp_composite_split_backward
    ops.warp_composite_split_backward = lambda *a, **k: (called.append(1), real(*a, **k))[1]
    try:
        rgb, depth, tgt_mask, flow, om = call()
        with torch.no_grad():
            out0 = call()
        for o, o0 in zip((rgb, depth, tgt_mask, flow, om), out0):
            if o is not None:
                assert bits_equal(o.detach().cpu().numpy(), o0.cpu().numpy()) == 0 and o0.grad_fn is None
        assert rgb.grad_fn is not None and depth.grad_fn is not None
        assert flow.requires_grad is False and tgt_mask.requires_grad is False
        outs, ups = [rgb, depth], [t(d["g_rgb"]), t(d["g_depth"])]
        if with_mask:
            outs.append(om); ups.append(t(d["g_mask"]))
        torch.autograd.backward(outs, ups)
    finally:
        ops.warp_composite_split_backward = real
    assert len(called) == mk.B, "the fused backward kernel was not the one that ran"
    report = []
    check(gold, "rtd/%s/full/" % name, "mpi_rgb_src", leaves["mpi_rgb_src"].grad, report)
    check(gold, "rtd/%s/%s/" % (name, "noflow" if with_mask else "noflow_nomask"), "mpi_sigma_src", leaves["mpi_sigma_src"].grad, report)
    settle(report)


# ---- 4. memory ---------------------------------------------------------------------------------------------------------------------------------

def test_fused_backward_holds_no_plane_deep_intermediate(gold):
    b, S, h, w, seed = (int(gold["memory/" + k]) for k in ("B", "S", "H", "W", "seed"))
    assert (S, h, w) == (8, 64, 96)
    d = mk.draw(seed, S, False, h, w, b)
    R, sampler, xs, xt, disp, G, K, Kinv = geometry(S, b, h, w)
    disp = disp.to(DEV)
    peaks = {}
    for fused in (None, False):
        rgb_in, sig_in = t(d["rgb"], True), t(d["sigma"], True)
        g_rgb, g_depth = t(d["g_rgb"]), t(d["g_depth"])
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        rgb, depth, tgt_mask, flow, om = R.render_tgt_rgb_depth(sampler, rgb_in, sig_in, disp, xt, xs, G, Kinv, K, fused=fused)
        torch.autograd.backward([rgb, depth], [g_rgb, g_depth])
        torch.cuda.synchronize()
        peaks[fused] = torch.cuda.max_memory_allocated() - before
        assert rgb_in.grad is not None and sig_in.grad is not None
        del rgb, depth, tgt_mask, flow, om, rgb_in, sig_in
    bound = 1.5 * (d["rgb"].nbytes + d["sigma"].nbytes)
    print("peak over forward + backward: fused %d B, generic %d B, bound %d B" % (peaks[None], peaks[False], bound))
    assert peaks[None] <= bound, (peaks, bound)
    assert peaks[False] > bound, (peaks, bound)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_argument(gold):
    from mpiflow_amd._lib import MpiFlowHipError
    S = 5
    d = mk.draw(1, S, True)
    R, sampler, xs, xt, disp, G, K, Kinv = geometry(S)
    rgb, sig, om = t(d["rgb"], True), t(d["sigma"], True), t(d["obj_mask"])
    base = dict(mpi_disparity_src=disp.to(DEV), xyz_tgt_BS3HW=xt, xyz_src_BS3HW=xs, G_tgt_src=G, K_src_inv=Kinv, K_tgt=K)
    for bad in base:
        kw = dict(base)
        kw[bad] = base[bad].clone().requires_grad_(True)
        with pytest.raises(MpiFlowHipError, match=bad):
            R.render_tgt_rgb_depth(sampler, rgb, sig, obj_mask=om, **kw)
        with torch.no_grad():
            assert R.render_tgt_rgb_depth(sampler, rgb, sig, obj_mask=om, **kw)[0].grad_fn is None
    with pytest.raises(MpiFlowHipError, match="is_bg_depth_inf"):
        R.render_tgt_rgb_depth(sampler, rgb, sig, obj_mask=om, is_bg_depth_inf=True, **base)
    with pytest.raises(MpiFlowHipError, match="is_bg_depth_inf"):
        R.render(rgb, sig, xt, is_bg_depth_inf=True)
    with pytest.raises(MpiFlowHipError, match="xyz_BS3HW"):
        R.render(rgb, sig, xt.clone().requires_grad_(True))
    with pytest.raises(MpiFlowHipError, match="src_xyz_BS3HW"):
        R.plane_volume_rendering_flow(sig, t(d["src_flow"]), xs.clone().requires_grad_(True), False)
    with pytest.raises(MpiFlowHipError, match="mpi_rgb_src"):
        R.render_tgt_rgb_depth(sampler, t(d["rgb"]).double().requires_grad_(True), sig, obj_mask=om, **base)
    with pytest.raises(MpiFlowHipError, match="rgb_BS3HW"):
        R.render(t(d["rgb"]).double().requires_grad_(True), sig, xt)
    args = (torch.reciprocal(disp).view(-1), rep(G, S), rep(Kinv, S), rep(K, S))
    src = t(d["rgb"].reshape(mk.B * S, 3, mk.H, mk.W), True)
    for i, bad in enumerate(("d_src_B", "G_tgt_src", "K_src_inv", "K_tgt")):
        a = list(args)
        a[i] = a[i].clone().requires_grad_(True)
        with pytest.raises(MpiFlowHipError, match=bad):
            sampler.sample(src, *a)
    with pytest.raises(MpiFlowHipError, match="src_BCHW"):
        sampler.sample(src.detach().double().requires_grad_(True), *args)
    # double backward
    out = R.render(rgb, sig, xt)[0]
    w = torch.ones_like(out).requires_grad_(True)             # a first gradient that itself depends on something differentiable
    (g,) = torch.autograd.grad((out * w).sum(), sig, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    # nothing requires grad: no grad_fn anywhere
    for o in R.render_tgt_rgb_depth(sampler, rgb.detach(), sig.detach(), obj_mask=om, **base):
        assert o.grad_fn is None and not o.requires_grad
