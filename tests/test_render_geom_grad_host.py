"""Host-side checks of the renderer's geometry gradients: no GPU.  The golden (tests/golden/render_geom_grad.npz, the reference's own float64
autograd) is intact and covers what it must; the formulas that the HIP kernels implement - written out by hand in tests/render_geom_grad_restated.py,
no autograd - reproduce its float64 gradients to 1e-9; the context manager exists, is off by default, nests and is per thread; the header declares
the new launchers and the ctypes table mirrors them."""
import os
import re
import sys
import threading

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_render_geom_grad_golden as mg  # noqa: E402
import make_render_grad_golden as mk  # noqa: E402
import render_geom_grad_restated as gr  # noqa: E402
import render_grad_restated as rr  # noqa: E402

SYMBOLS = ("mpf_volume_render_bwd_xyz", "mpf_src_xyz_bwd", "mpf_plane_flow_bwd", "mpf_warp_composite_bwd_disp")
B, H, W = mk.B, mk.H, mk.W


@pytest.fixture(scope="module")
def gold():
    return load_golden("render_geom_grad")


def d64(x):
    return torch.from_numpy(np.asarray(x)).double()


def close(got, g64, what, rel=1e-9):
    g64 = np.asarray(g64)
    got = got.numpy().reshape(g64.shape)
    assert np.abs(got - g64).max() <= rel * np.abs(g64).max(), (what, np.abs(got - g64).max(), np.abs(g64).max())


def test_golden_integrity_and_coverage(gold):
    zero = set(str(z) for z in gold["zero_by_construction"])
    assert zero == set(mg.ZERO_BY_CONSTRUCTION)
    e = {k: float(v) for k, v in gold.items() if "/e_ref/" in k}
    assert len(e) >= 24
    for k, v in e.items():
        g64 = gold[k.replace("/e_ref/", "/g64/")]
        assert np.isfinite(g64).all() and 0.0 <= v < 1e-4, (k, v)
        assert (np.abs(g64).max() == 0) == (k.replace("/e_ref/", "/g64/") in zero), k
        assert max(4 * v, 1e-6) < 1e-3
    for k in ("s5_mask/invalid", "s5_mask/clamp_left", "s5_mask/clamp_right", "s5_mask/clamp_top", "s5_mask/clamp_bottom", "s5_mask/planes_all_invalid",
              "s5_mask/z_negative", "s1_mask/invalid"):
        assert int(gold["coverage/" + k]) > 0, k
    for name, S, with_mask, hard, with_src, seed in mg.RENDER_CASES:
        p = "render/%s/" % name
        assert int(gold[p + "seed"]) == seed and abs(mk.input_sum(mk.draw(seed, S, with_mask)) - float(gold[p + "input_sum"])) < 1e-6
    for name, S, seed in mg.RTD_CASES:
        p = "rtd/%s/" % name
        assert int(gold[p + "seed"]) == seed and abs(mk.input_sum(mk.draw(seed, S, True)) - float(gold[p + "input_sum"])) < 1e-6
    for name, dup, seed in mg.E2E_CASES:
        p = "e2e/%s/" % name
        total = mk.input_sum(mk.draw(seed, 5, True)) + sum(mk.input_sum({k: mk.draw(seed + o, 5, True)[k] for k in mg.UPSTREAM}) for o in mg.E2E_DRAWS)
        assert abs(total - float(gold[p + "input_sum"])) < 1e-6
        assert (gold[p + "disparity"] == mg.e2e_disparity(dup)).all() and gold[p + "full/g64/disparity"].shape == (3, B, 5)
    assert (gold["e2e/s5_dup/disparity"][:, 1] == gold["e2e/s5_dup/disparity"][:, 2]).all()             # the plane distance of exactly 0
    assert abs(mg.helpers_upstream().astype(np.float64).sum() - float(gold["helpers/s5/input_sum"])) < 1e-6
    assert abs(mg.sample_inverse_upstream().astype(np.float64).sum() - float(gold["sample_inverse/s5/input_sum"])) < 1e-6
    assert os.path.getsize(os.path.join(GOLDEN, "render_geom_grad.npz")) < 1000 * 1000


def test_context_manager_is_off_by_default_nests_and_is_per_thread():
    from mpiflow_amd.utils import mpi
    from mpiflow_amd.utils.mpi import _autograd
    assert mpi.plane_geometry_grad is _autograd.plane_geometry_grad
    assert not _autograd.geometry_grad_enabled()
    with mpi.plane_geometry_grad():
        assert _autograd.geometry_grad_enabled()
        with mpi.plane_geometry_grad():
            assert _autograd.geometry_grad_enabled()
        assert _autograd.geometry_grad_enabled()
        seen = []
        th = threading.Thread(target=lambda: seen.append(_autograd.geometry_grad_enabled()))
        th.start(); th.join()
        assert seen == [False]
    assert not _autograd.geometry_grad_enabled()
    with pytest.raises(ZeroDivisionError):
        with mpi.plane_geometry_grad():
            1 / 0
    assert not _autograd.geometry_grad_enabled()


def test_header_declares_the_new_launchers_and_ctypes_mirrors_them():
    from mpiflow_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    for name in ("src_xyz_backward", "plane_flow_backward"):
        assert callable(getattr(ops, name))


def test_launchers_refuse_bad_arguments_without_a_gpu():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    lib = _lib.load()
    one, bad = ctypes.c_void_p(256), 10001
    assert lib.mpf_src_xyz_bwd(None, one, 4, 8, 8, one, 1, one, None) == bad and b"null pointer" in lib.mpf_last_error()
    assert lib.mpf_src_xyz_bwd(one, one, 4096, 8, 8, one, 1, one, None) == bad and b"bad shape" in lib.mpf_last_error()
    assert lib.mpf_src_xyz_bwd(one, one, 4, 32, 32, one, 3, one, None) == bad and b"workspace" in lib.mpf_last_error()
    assert lib.mpf_plane_flow_bwd(one, one, 4, 8, 8, None, 1, one, None) == bad and b"null pointer" in lib.mpf_last_error()
    assert lib.mpf_plane_flow_bwd(one, one, 0, 8, 8, one, 1, one, None) == bad
    assert lib.mpf_plane_flow_bwd(one, one, 4, 32, 32, one, 3, one, None) == bad and b"workspace" in lib.mpf_last_error()
    assert lib.mpf_plane_flow_bwd(ctypes.c_void_p(260), one, 4, 8, 8, one, 1, one, None) == bad and b"aligned" in lib.mpf_last_error()
    assert lib.mpf_warp_composite_bwd_disp(one, one, None, one, 4, 8, 8, one, None, None, one, one, one, 1, None, None) == bad
    assert b"come together" in lib.mpf_last_error()
    assert lib.mpf_warp_composite_bwd_disp(one, one, None, one, 4, 64, 64, one, None, None, one, one, one, 15, one, None) == bad
    assert b"workspace" in lib.mpf_last_error()
    assert lib.mpf_volume_render_bwd_xyz(None, None, None, None, 4, 16, 0, 0, None, None, None, None, None, None, None, None, one, None) == bad


# ---- the formulas, by hand, in float64 ------------------------------------------------------------------------------------------------------

def planes(S, disp=None):
    disp0, G, K, Kinv = (d64(a) for a in mk.geometry(S))
    disp = disp0 if disp is None else d64(disp)
    xs, xt = rr.plane_xyz(disp, G, Kinv, H, W)
    return disp, G, K, Kinv, xs, xt


@pytest.mark.parametrize("name,S,with_mask,hard,with_src,seed", mg.RENDER_CASES)
def test_item1_composite_xyz_gradient(gold, name, S, with_mask, hard, with_src, seed):
    d = mk.draw(seed, S, with_mask)
    _, _, _, _, xs, xt = planes(S)
    p = "render/%s/" % name
    for b in range(B):
        flat = lambda k, c: d64(d[k][b]).reshape(*c, -1)
        if not hard:
            # render() keeps plane_volume_rendering's mask and drops its flow: the flow's upstream gradient is zero there
            extra = torch.cat((flat("src_flow", (S, 2)), flat("obj_mask", (S, 1))), 1) if with_src else None
            g_extra = torch.cat((torch.zeros(2, H * W, dtype=torch.float64), flat("g_mask", (1,)))) if with_src else None
            g = gr.composite_xyz_grad(flat("sigma", (S,)), xt[b].reshape(S, 3, -1), rgb=flat("rgb", (S, 3)), extra=extra, g_rgb=flat("g_rgb", (3,)),
                                      g_depth=flat("g_depth", ()), g_extra=g_extra, g_w=flat("g_weights", (S,)), g_tacc=flat("g_tacc", (S,)))
            close(g, gold[p + "g64/xyz_BS3HW"][b], (name, b, "xyz"))
        if with_src and not hard:
            g = gr.composite_xyz_grad(flat("src_sigma", (S,)), xs[b].reshape(S, 3, -1), extra=flat("src_flow", (S, 2)), g_extra=flat("g_flow", (2,)))
            if S == 1:
                assert float(g.abs().max()) == 0.0 and np.abs(gold[p + "g64/src_xyz_BS3HW"]).max() == 0.0
            else:
                close(g, gold[p + "g64/src_xyz_BS3HW"][b], (name, b, "src_xyz"))
        if hard:
            assert np.abs(gold[p + "g64/src_xyz_BS3HW"]).max() == 0.0            # the one-hot selection is constant: the kernel writes zeros


def test_item3_helpers(gold):
    disp, G, K, Kinv, xs, xt = planes(5)
    up = d64(mg.helpers_upstream())
    got = torch.stack([gr.src_xyz_disparity_grad(up[b], disp[b], Kinv[b], H, W) for b in range(B)])
    close(got, gold["helpers/s5/g64/disparity"], "helpers")
    # R^T g: against torch's own autograd of the affine map
    x = xs[0].reshape(5, 3, -1).clone().requires_grad_(True)
    y = G[0, :3, :3] @ x + G[0, :3, 3:4]
    (auto,) = torch.autograd.grad((y * up[0].reshape(5, 3, -1)).sum(), x)
    close(gr.rotate_back(up[0].reshape(5, 3, -1), G[0]), auto.numpy(), "rotate_back")


def test_item4_sample_inverse(gold):
    S = 5
    disp, G, K, Kinv, _, _ = planes(S)
    rep = lambda m: m.unsqueeze(1).expand(B, S, *m.shape[1:]).reshape(B * S, *m.shape[1:])
    got = gr.plane_flow_depth_grad(d64(mg.sample_inverse_upstream()), torch.reciprocal(disp).reshape(-1), rep(G), rep(Kinv), rep(K), H, W)
    close(got, gold["sample_inverse/s5/g64/d_src_B"], "sample_inverse")


@pytest.mark.parametrize("name,dup,seed", mg.E2E_CASES)
def test_item5_fused_disparity_gradient_and_the_flow_route(gold, name, dup, seed):
    S = 5
    d = mk.draw(seed, S, True)
    disp, G, K, Kinv, _, _ = planes(S, mg.e2e_disparity(dup))
    for i, off in enumerate(mg.E2E_DRAWS):
        up = mk.draw(seed + off, S, True)
        nof, full = [], []
        for b in range(B):
            g = gr.fused_disparity_grad(d64(d["rgb"][b]), d64(d["sigma"][b]), disp[b], G[b], Kinv[b], K[b], d64(up["g_rgb"][b]), d64(up["g_depth"][b]),
                                        obj_mask=d64(d["obj_mask"][b]), g_mask=d64(up["g_mask"][b]))
            nof.append(g)
            full.append(g + gr.flow_route_disparity_grad(d64(d["sigma"][b]), disp[b], G[b], Kinv[b], K[b], d64(up["g_flow2"][b]), H, W))
        close(torch.stack(nof), gold["e2e/%s/noflow/g64/disparity" % name][i], (name, "noflow", i))
        close(torch.stack(full), gold["e2e/%s/full/g64/disparity" % name][i], (name, "full", i))


@pytest.mark.parametrize("name,S,seed", mg.RTD_CASES)
def test_rtd_disparity_argument_gets_the_sample_inverse_route_only(gold, name, S, seed):
    """with independent leaves the mpi_disparity_src argument is reached through sample_inverse alone (item 4 times d depth / d disparity)"""
    d = mk.draw(seed, S, True)
    disp, G, K, Kinv, xs, _ = planes(S)
    rep = lambda m: m.unsqueeze(0).expand(S, *m.shape)
    got = []
    for b in range(B):
        depth = torch.reciprocal(disp[b])
        _, ws = rr.weights_of(d64(d["sigma"][b]).unsqueeze(0), xs[b:b + 1])
        g_fb = (ws[0] * d64(d["g_flow2"][b]).unsqueeze(0)).permute(0, 2, 3, 1)
        got.append(gr.plane_flow_depth_grad(g_fb, depth, rep(G[b]), rep(Kinv[b]), rep(K[b]), H, W) * (-depth ** 2))
    close(torch.stack(got), gold["rtd/%s/full/g64/mpi_disparity_src" % name], name)
