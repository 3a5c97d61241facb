"""The renderer's opt-in geometry gradients (mpiflow_amd.utils.mpi.plane_geometry_grad) against the reference's own float64 autograd
(tests/golden/render_geom_grad.npz, written by tests/golden/make_render_geom_grad_golden.py).

Tolerance, per gradient tensor, nothing excluded: max|g - g64| / max|g64| <= max(4 * e_ref, 1e-6), e_ref being the reference's own float32 run against
its float64 (the bar of tests/test_render_grad.py).  A gradient that is identically zero in float64 must be identically zero here.  The shapes are the
golden's - B = 2, S in {1, 5}, 13 x 21 = 273 pixels: one full and one partial workgroup of 256, so the sums across workgroups and the tail guard both
run - plus one kernel-level case with S = 70, above a wave's 64 lanes, against the hand-written float64 formulas of tests/render_geom_grad_restated.py."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, bits_equal, load_golden

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_render_geom_grad_golden as mg  # noqa: E402
import make_render_grad_golden as mk  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H, W = mk.B, mk.H, mk.W


@pytest.fixture(scope="module")
def gold():
    import __graft_entry__ as ge
    ge.build()
    return load_golden("render_geom_grad")


def t(x, grad=False):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV).requires_grad_(grad)


def check(gold, key, g_hip, report, index=None):
    g64 = gold[key]
    e_ref = float(gold[key.replace("/g64/", "/e_ref/")])
    if index is not None:
        g64 = g64[index]
    g = g_hip.detach().cpu().numpy().astype(np.float64).reshape(g64.shape)
    assert np.isfinite(g).all(), key
    scale = np.abs(gold[key]).max()
    if scale == 0.0:
        print("%s: identically zero in float64; max|g_hip| %.3e" % (key, np.abs(g).max()))
        assert np.abs(g).max() == 0.0, key
        return
    scale = np.abs(g64).max()
    err, bar = np.abs(g - g64).max() / scale, max(4.0 * e_ref, 1e-6)
    print("%s%s: err %.3e  e_ref %.3e  bar %.3e" % (key, "" if index is None else "[%d]" % index, err, e_ref, bar))
    report.append((key, index, err, bar))


def settle(report):
    bad = [r for r in report if not r[2] <= r[3]]
    assert not bad, bad


def zeros_if_none(g, like):
    return torch.zeros_like(like) if g is None else g


def geometry(S, disp=None, grad=False):
    """our sampler and xyz tensors for the golden's poses, built inside the context manager when the disparity is a leaf"""
    from mpiflow_amd.utils import mpi
    from mpiflow_amd.utils.mpi import mpi_rendering as R
    from mpiflow_amd.utils.mpi.homography_sampler import HomographySample
    disp0, G, K, Kinv = (torch.from_numpy(a) for a in mk.geometry(S))
    disp = (disp0 if disp is None else torch.from_numpy(disp)).to(DEV).requires_grad_(grad)
    sampler = HomographySample(H, W, torch.device(DEV))
    with mpi.plane_geometry_grad():
        xs = R.get_src_xyz_from_plane_disparity(sampler.meshgrid, disp, Kinv)
        xt = R.get_tgt_xyz_from_plane_disparity(xs, G)
    return R, sampler, xs, xt, disp, G, K, Kinv


def rep(m, S):
    return m.unsqueeze(1).repeat(1, S, 1, 1).reshape(m.shape[0] * S, m.shape[-2], m.shape[-1])


def same_bits(outs, outs0):
    for o, o0 in zip(outs, outs0):
        if o is not None:
            assert bits_equal(o.detach().cpu().numpy(), o0.detach().cpu().numpy()) == 0


# ---- every golden case through the public functions ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,S,with_mask,hard,with_src,seed", mg.RENDER_CASES)
def test_render_xyz_gradients(gold, name, S, with_mask, hard, with_src, seed):
    from mpiflow_amd.utils import mpi
    d = mk.draw(seed, S, with_mask)
    R, sampler, xs, xt, *_ = geometry(S)
    leaves = dict(xyz_BS3HW=xt.detach().clone().requires_grad_(True), src_xyz_BS3HW=xs.detach().clone().requires_grad_(True) if with_src else None)
    call = lambda a, b: R.render(t(d["rgb"]), t(d["sigma"]), a, t(d["src_sigma"]) if with_src else None, t(d["src_flow"]) if with_src else None, b,
                                 hard_flow=hard, obj_mask=t(d["obj_mask"]))
    with mpi.plane_geometry_grad():
        out = call(leaves["xyz_BS3HW"], leaves["src_xyz_BS3HW"])
    out0 = call(xt.detach(), xs.detach() if with_src else None)                       # outside, nothing requires grad: the plain path
    same_bits(out, out0)
    ups = [d["g_rgb"], d["g_depth"], d["g_tacc"], d["g_weights"], d["g_flow"], d["g_mask"]]
    pairs = [(o, t(u)) for o, u in zip(out, ups) if o is not None and o.requires_grad]
    torch.autograd.backward([p[0] for p in pairs], [p[1] for p in pairs])
    report = []
    p = "render/%s/" % name
    check(gold, ("render/s5_mask/" if hard else p) + "g64/xyz_BS3HW", leaves["xyz_BS3HW"].grad, report)
    if with_src:
        check(gold, p + "g64/src_xyz_BS3HW", zeros_if_none(leaves["src_xyz_BS3HW"].grad, xs), report)
    settle(report)


def rtd_inputs(seed, S):
    d = mk.draw(seed, S, True)
    return d, [t(d["g_rgb"]), t(d["g_depth"]), t(d["g_flow2"]), t(d["g_mask"])]


def rtd_backward(out, ups, which):
    rgb, depth, tgt_mask, flow, om = out
    outs, gs = [rgb, depth, om], [ups[0], ups[1], ups[3]]
    if which == "full":
        outs.append(flow); gs.append(ups[2])
    torch.autograd.backward(outs, gs)


@pytest.mark.parametrize("which", ["full", "noflow"])
@pytest.mark.parametrize("name,S,seed", mg.RTD_CASES)
def test_render_tgt_rgb_depth_independent_leaves(gold, name, S, seed, which):
    from mpiflow_amd.utils import mpi
    d, ups = rtd_inputs(seed, S)
    R, sampler, xs, xt, disp, G, K, Kinv = geometry(S)
    leaves = dict(xyz_tgt_BS3HW=xt.detach().clone().requires_grad_(True), xyz_src_BS3HW=xs.detach().clone().requires_grad_(True),
                  mpi_disparity_src=disp.detach().clone().requires_grad_(True))
    call = lambda dd, a, b: R.render_tgt_rgb_depth(sampler, t(d["rgb"]), t(d["sigma"]), dd, a, b, G, Kinv, K, obj_mask=t(d["obj_mask"]), fused=False)
    with mpi.plane_geometry_grad():
        out = call(leaves["mpi_disparity_src"], leaves["xyz_tgt_BS3HW"], leaves["xyz_src_BS3HW"])
    same_bits(out, call(disp.detach(), xt.detach(), xs.detach()))
    assert not out[2].requires_grad
    rtd_backward(out, ups, which)
    report = []
    for k, leaf in leaves.items():
        check(gold, "rtd/%s/%s/g64/%s" % (name, which, k), zeros_if_none(leaf.grad, leaf), report)
    settle(report)


@pytest.mark.parametrize("name,dup,seed", mg.E2E_CASES)
def test_end_to_end_disparity_generic_and_fused(gold, name, dup, seed):
    """one disparity leaf through both helpers into render_tgt_rgb_depth: the generic form with and without the flow in the loss, the fused form (whose
    flowA2B stays detached) without; three draws of the upstream gradients"""
    from mpiflow_amd import ops
    from mpiflow_amd.utils import mpi
    S = 5
    d = mk.draw(seed, S, True)
    report = []
    for i, off in enumerate(mg.E2E_DRAWS):
        up = mk.draw(seed + off, S, True)
        ups = [t(up["g_rgb"]), t(up["g_depth"]), t(up["g_flow2"]), t(up["g_mask"])]
        for fused, which in ((False, "full"), (False, "noflow"), (True, "noflow")):
            R, sampler, xs, xt, disp, G, K, Kinv = geometry(S, mg.e2e_disparity(dup), grad=True)
            assert xs.grad_fn is not None and xt.grad_fn is not None
            called = []
            real = ops.warp_composite_split_backward
            ops.warp_composite_split_backward = lambda *a, **k: (called.append(k.get("want_disparity", False)), real(*a, **k))[1]
            try:
                with mpi.plane_geometry_grad():
                    out = R.render_tgt_rgb_depth(sampler, t(d["rgb"]), t(d["sigma"]), disp, xt, xs, G, Kinv, K, obj_mask=t(d["obj_mask"]), fused=fused)
                if i == 0:
                    with torch.no_grad():
                        same_bits(out, R.render_tgt_rgb_depth(sampler, t(d["rgb"]), t(d["sigma"]), disp, xt, xs, G, Kinv, K, obj_mask=t(d["obj_mask"]),
                                                              fused=fused))
                assert out[3].requires_grad is (not fused)
                rtd_backward(out, ups, which)
            finally:
                ops.warp_composite_split_backward = real
            assert called == ([True] * B if fused else []), "the fused form must run mpf_warp_composite_bwd_disp, the generic one must not"
            check(gold, "e2e/%s/%s/g64/disparity" % (name, which), disp.grad, report, index=i)
    settle(report)


def test_routing_the_leaf_behind_the_xyz_tensors_gets_the_gradient(gold):
    """the xyz tensors are built from a leaf, render_tgt_rgb_depth receives a detached copy of the disparity: as in the reference the gradient arrives
    at the leaf (through xyz), in both forms - everything the loss (without flowA2B) sends to a disparity"""
    from mpiflow_amd.utils import mpi
    name, dup, seed = mg.E2E_CASES[0]
    d, ups = rtd_inputs(seed, 5)
    report = []
    for fused in (False, True):
        R, sampler, xs, xt, disp, G, K, Kinv = geometry(5, mg.e2e_disparity(dup), grad=True)
        copy = disp.detach().clone()
        with mpi.plane_geometry_grad():
            out = R.render_tgt_rgb_depth(sampler, t(d["rgb"]), t(d["sigma"]), copy, xt, xs, G, Kinv, K, obj_mask=t(d["obj_mask"]), fused=fused)
        rtd_backward(out, ups, "noflow")
        assert copy.grad is None
        check(gold, "e2e/%s/noflow/g64/disparity" % name, disp.grad, report, index=0)
    settle(report)


def test_helpers_and_sample_inverse(gold):
    from mpiflow_amd.utils import mpi
    S = 5
    report = []
    R, sampler, xs, xt, disp, G, K, Kinv = geometry(S, grad=True)
    xs.backward(t(mg.helpers_upstream()))
    check(gold, "helpers/s5/g64/disparity", disp.grad, report)
    leaf = torch.reciprocal(disp.detach()).view(B * S).requires_grad_(True)
    args = (rep(G, S), rep(Kinv, S), rep(K, S))
    with mpi.plane_geometry_grad():
        flow = sampler.sample_inverse(xs.detach().reshape(B * S, 3, H, W), leaf, *args)
        # sample() accepts the same leaf and, as in the reference, gives it nothing
        tgt, _, _ = sampler.sample(t(mk.draw(1, S, False)["rgb"].reshape(B * S, 3, H, W), True), leaf, *args)
    flow0 = sampler.sample_inverse(xs.detach().reshape(B * S, 3, H, W), leaf, *args)                 # outside: forward only, as it always was
    assert flow0.grad_fn is None and bits_equal(flow.detach().cpu().numpy(), flow0.cpu().numpy()) == 0
    tgt.sum().backward()
    assert leaf.grad is None
    flow.backward(t(mg.sample_inverse_upstream()))
    check(gold, "sample_inverse/s5/g64/d_src_B", leaf.grad, report)
    settle(report)


# ---- S above a wave's 64 lanes, against the hand-written formulas ----------------------------------------------------------------------------

def test_kernels_with_seventy_planes():
    import __graft_entry__ as ge
    ge.build()
    import render_geom_grad_restated as gr
    from mpiflow_amd import host_math, ops
    S, h, w = 70, 5, 7
    rng = np.random.default_rng(9070)
    disp = np.linspace(1.9, 0.2, S).astype(np.float32)
    _, G, K, Kinv = (a[0] for a in mk.geometry(1, h, w, 1))
    rgb, sigma = rng.random((S, 3, h, w)).astype(np.float32), (2.5 * rng.random((S, 1, h, w))).astype(np.float32)
    g_rgb, g_depth = rng.standard_normal((3, h, w)).astype(np.float32), rng.standard_normal((1, h, w)).astype(np.float32)
    g_xyz, g_flow = rng.standard_normal((S, 3, h, w)).astype(np.float32), rng.standard_normal((S, h, w, 2)).astype(np.float32)
    rep = lambda m: m.unsqueeze(0).expand(S, *m.shape)

    depth = host_math.plane_depths(torch.from_numpy(disp))
    xt = ops.transform_xyz(torch.from_numpy(G), ops.src_xyz(torch.from_numpy(Kinv), depth, h, w, torch.device(DEV)).reshape(S, 3, h * w))
    xt_host = xt.cpu().numpy()                         # item 1 is checked on the very xyz tensor the kernel reads

    def restated(dt):
        c = lambda a: torch.from_numpy(a).to(dt)
        depth = torch.reciprocal(c(disp))
        return dict(src_xyz=gr.src_xyz_disparity_grad(c(g_xyz), c(disp), c(Kinv), h, w),
                    plane_flow=gr.plane_flow_depth_grad(c(g_flow), depth, rep(c(G)), rep(c(Kinv)), rep(c(K)), h, w),
                    fused=gr.fused_disparity_grad(c(rgb), c(sigma), c(disp), c(G), c(Kinv), c(K), c(g_rgb), c(g_depth)),
                    xyz=gr.composite_xyz_grad(c(sigma).reshape(S, -1), c(xt_host),
                                              rgb=c(rgb).reshape(S, 3, -1), g_rgb=c(g_rgb).reshape(3, -1), g_depth=c(g_depth).reshape(-1)))
    r64, r32 = restated(torch.float64), restated(torch.float32)
    H_ts, H_st = host_math.homographies(torch.from_numpy(G), torch.from_numpy(Kinv), torch.from_numpy(K), depth)
    Kt_t = (torch.from_numpy(K) @ torch.from_numpy(G)[:3, 3]).expand(S, 3)
    dparams = ops.upload_params(ops.warp_params(H_st, torch.from_numpy(Kinv), torch.from_numpy(G), depth), torch.device(DEV))
    got = dict(src_xyz=ops.src_xyz_backward(t(g_xyz), torch.from_numpy(Kinv), depth),
               plane_flow=ops.plane_flow_backward(t(g_flow), H_ts, depth, Kt_t, torch.from_numpy(Kinv)[2].expand(S, 3)),
               fused=ops.warp_composite_split_backward(t(rgb), t(sigma), None, dparams, t(g_rgb), t(g_depth), want_disparity=True)[2],
               xyz=ops.volume_render_backward(t(rgb).reshape(S, 3, -1), t(sigma).reshape(S, -1), xt, g_rgb=t(g_rgb).reshape(3, -1),
                                              g_depth=t(g_depth).reshape(-1), want_xyz=True)["xyz"])
    bad = []
    for k in got:
        g64 = r64[k].numpy()
        scale = np.abs(g64).max()
        e32 = np.abs(r32[k].numpy().astype(np.float64) - g64).max() / scale
        err, bar = np.abs(got[k].cpu().numpy().astype(np.float64).reshape(g64.shape) - g64).max() / scale, max(4 * e32, 1e-6)
        print("S = 70 %s: err %.3e  e32 %.3e  bar %.3e" % (k, err, e32, bar))
        assert scale > 0 and np.isfinite(err)
        if not err <= bar:
            bad.append((k, err, bar))
    assert not bad, bad


# ---- reproducibility, memory, refusals ---------------------------------------------------------------------------------------------------------

def test_two_backward_runs_give_the_same_bits(gold):
    from mpiflow_amd.utils import mpi
    name, dup, seed = mg.E2E_CASES[0]
    d, ups = rtd_inputs(seed, 5)
    runs = []
    for _ in range(2):
        got = {}
        R, sampler, xs, xt, disp, G, K, Kinv = geometry(5, mg.e2e_disparity(dup), grad=True)
        with mpi.plane_geometry_grad():                                                # item 5: the fused form
            out = R.render_tgt_rgb_depth(sampler, t(d["rgb"]), t(d["sigma"]), disp, xt, xs, G, Kinv, K, obj_mask=t(d["obj_mask"]), fused=True)
        rtd_backward(out, ups, "noflow")
        got["fused"] = disp.grad.clone()
        R, sampler, xs, xt, disp, G, K, Kinv = geometry(5, grad=True)                  # item 3
        xs.backward(t(mg.helpers_upstream()))
        got["helpers"] = disp.grad.clone()
        leaf = torch.reciprocal(disp.detach()).view(B * 5).requires_grad_(True)        # item 4
        with mpi.plane_geometry_grad():
            flow = sampler.sample_inverse(xs.detach().reshape(B * 5, 3, H, W), leaf, rep(G, 5), rep(Kinv, 5), rep(K, 5))
        flow.backward(t(mg.sample_inverse_upstream()))
        got["sample_inverse"] = leaf.grad.clone()
        x = xt.detach().clone().requires_grad_(True)                                   # item 1
        with mpi.plane_geometry_grad():
            o = R.render(t(d["rgb"]), t(d["sigma"]), x)
        torch.autograd.backward([o[0], o[1]], [ups[0], ups[1]])
        got["xyz"] = x.grad.clone()
        runs.append(got)
    for k in runs[0]:
        assert float(runs[0][k].abs().max()) > 0
        assert bits_equal(runs[0][k].cpu().numpy(), runs[1][k].cpu().numpy()) == 0, k


def test_fused_backward_with_the_disparity_gradient_holds_no_plane_deep_intermediate():
    """tests/test_render_grad.py's bound at its MEMORY_CASE, the [tiles, S] workspace of the per-plane sums included"""
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd.utils import mpi
    from mpiflow_amd.utils.mpi import mpi_rendering as R
    from mpiflow_amd.utils.mpi.homography_sampler import HomographySample
    c = mk.MEMORY_CASE
    b, S, h, w = c["B"], c["S"], c["H"], c["W"]
    assert (S, h, w) == (8, 64, 96)
    d = mk.draw(c["seed"], S, False, h, w, b)
    disp0, G, K, Kinv = (torch.from_numpy(a) for a in mk.geometry(S, h, w, b))
    sampler = HomographySample(h, w, torch.device(DEV))
    disp = disp0.to(DEV).requires_grad_(True)
    with mpi.plane_geometry_grad():
        xs = R.get_src_xyz_from_plane_disparity(sampler.meshgrid, disp, Kinv)
        xt = R.get_tgt_xyz_from_plane_disparity(xs, G)
    rgb_in, sig_in = t(d["rgb"], True), t(d["sigma"], True)
    g_rgb, g_depth = t(d["g_rgb"]), t(d["g_depth"])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with mpi.plane_geometry_grad():
        rgb, depth, tgt_mask, flow, om = R.render_tgt_rgb_depth(sampler, rgb_in, sig_in, disp, xt, xs, G, Kinv, K, fused=True)
    torch.autograd.backward([rgb, depth], [g_rgb, g_depth], inputs=[rgb_in, sig_in, disp])
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    bound = 1.5 * (d["rgb"].nbytes + d["sigma"].nbytes)
    print("peak over fused forward + backward with the disparity gradient: %d B, bound %d B" % (peak, bound))
    assert rgb_in.grad is not None and sig_in.grad is not None and disp.grad is not None and float(disp.grad.abs().max()) > 0
    assert peak <= bound, (peak, bound)


def test_refusals_inside_and_outside(gold):
    from mpiflow_amd._lib import MpiFlowHipError
    from mpiflow_amd.utils import mpi
    S = 5
    d = mk.draw(1, S, True)
    R, sampler, xs, xt, disp, G, K, Kinv = geometry(S)
    xs, xt = xs.detach(), xt.detach()
    rgb, sig, om = t(d["rgb"], True), t(d["sigma"], True), t(d["obj_mask"])
    base = dict(mpi_disparity_src=disp, xyz_tgt_BS3HW=xt, xyz_src_BS3HW=xs, G_tgt_src=G, K_src_inv=Kinv, K_tgt=K)
    with mpi.plane_geometry_grad():
        for bad in ("G_tgt_src", "K_src_inv", "K_tgt"):
            kw = dict(base)
            kw[bad] = base[bad].clone().requires_grad_(True)
            with pytest.raises(MpiFlowHipError, match=bad):
                R.render_tgt_rgb_depth(sampler, rgb, sig, obj_mask=om, **kw)
            with pytest.raises(MpiFlowHipError, match=bad):
                sampler.sample_inverse(xs.reshape(B * S, 3, H, W), torch.reciprocal(disp).view(-1),
                                       *[rep(kw[k], S) if kw[k] is base[k] else rep(base[k], S).requires_grad_(True) for k in ("G_tgt_src", "K_src_inv", "K_tgt")])
        with pytest.raises(MpiFlowHipError, match="K_src_inv"):
            R.get_src_xyz_from_plane_disparity(sampler.meshgrid, disp.clone().requires_grad_(True), Kinv.clone().requires_grad_(True))
        with pytest.raises(MpiFlowHipError, match="G_tgt_src"):
            R.get_tgt_xyz_from_plane_disparity(xs.clone().requires_grad_(True), G.clone().requires_grad_(True))
        geo = dict(base, mpi_disparity_src=disp.clone().requires_grad_(True))
        with pytest.raises(MpiFlowHipError, match="is_bg_depth_inf"):
            R.render_tgt_rgb_depth(sampler, rgb.detach(), sig.detach(), obj_mask=om, is_bg_depth_inf=True, fused=False, **geo)
        with pytest.raises(MpiFlowHipError, match="is_bg_depth_inf"):
            R.render(rgb.detach(), sig.detach(), xt.clone().requires_grad_(True), is_bg_depth_inf=True)
        with pytest.raises(MpiFlowHipError, match="xyz_BS3HW"):
            R.render(rgb.detach(), sig.detach(), xt.double().requires_grad_(True))
        with pytest.raises(MpiFlowHipError, match="mpi_disparity_src"):
            R.render_tgt_rgb_depth(sampler, rgb.detach(), sig.detach(), obj_mask=om, fused=False, **dict(base, mpi_disparity_src=disp.double().requires_grad_(True)))
        with pytest.raises(MpiFlowHipError, match="mpi_disparity_src"):
            R.get_src_xyz_from_plane_disparity(sampler.meshgrid, disp.double().requires_grad_(True), Kinv)
        with pytest.raises(MpiFlowHipError, match="d_src_B"):
            sampler.sample_inverse(xs.reshape(B * S, 3, H, W), torch.reciprocal(disp).double().view(-1).requires_grad_(True), rep(G, S), rep(Kinv, S), rep(K, S))
        # double backward
        x = xt.clone().requires_grad_(True)
        out = R.render(rgb.detach(), sig.detach(), x)[1]
        wgt = torch.ones_like(out).requires_grad_(True)
        (g,) = torch.autograd.grad((out * wgt).sum(), x, create_graph=True)
        with pytest.raises(RuntimeError, match="once_differentiable"):
            g.sum().backward()
    # outside: as today
    for bad in ("mpi_disparity_src", "xyz_tgt_BS3HW", "xyz_src_BS3HW"):
        kw = dict(base)
        kw[bad] = base[bad].clone().requires_grad_(True)
        with pytest.raises(MpiFlowHipError, match=bad):
            R.render_tgt_rgb_depth(sampler, rgb, sig, obj_mask=om, **kw)
    with pytest.raises(MpiFlowHipError, match="plane_geometry_grad"):
        R.render(rgb, sig, xt.clone().requires_grad_(True))
