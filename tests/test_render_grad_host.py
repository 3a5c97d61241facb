"""Host-side checks of the differentiable renderer: no GPU.  The header declares the three backward launchers and the ctypes table mirrors them; the
golden's recorded coverage is what the issue asks for; the float32-vs-float64 reference error it carries yields the tests' tolerance; the launchers
refuse bad arguments before they launch anything (tools/render_bwd_args_check.cpp is the same probe as a stand-alone program for a sanitizer build);
and the restated torch baseline reproduces the golden's float64 gradients on the CPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden

sys.path.insert(0, GOLDEN)
import make_render_grad_golden as mk  # noqa: E402

SYMBOLS = ("mpf_volume_render_bwd", "mpf_homography_sample_bwd", "mpf_warp_composite_bwd")


def test_header_declares_the_backward_launchers_and_ctypes_mirrors_them():
    from mpiflow_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    for name in ("volume_render_backward", "homography_sample_backward", "warp_composite_split_backward"):
        from mpiflow_amd import ops
        assert callable(getattr(ops, name))


def test_golden_coverage_and_tolerance():
    g = load_golden("render_grad")
    c = {k.split("/", 1)[1]: int(v) for k, v in g.items() if k.startswith("coverage/")}
    for k in ("s5/invalid", "s5/clamp_left", "s5/clamp_right", "s5/clamp_top", "s5/clamp_bottom", "s5/planes_all_invalid", "s1/invalid",
              "rtd_s5_mask/z_negative"):
        assert c[k] > 0, (k, c)
    assert (int(g["memory/S"]), int(g["memory/H"]), int(g["memory/W"])) == (8, 64, 96)
    e = {k: float(v) for k, v in g.items() if "/e_ref/" in k}
    assert len(e) >= 25
    for k, v in e.items():
        g64 = g[k.replace("/e_ref/", "/g64/")]
        assert np.isfinite(g64).all() and 0.0 <= v < 1e-4, (k, v)          # float32 autograd of these sums: a few 1e-6 at the most
        assert max(4 * v, 1e-6) < 1e-3


def test_launchers_refuse_bad_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    bad = 10001
    assert lib.mpf_volume_render_bwd(None, None, None, None, 4, 16, 0, 0, None, None, None, None, None, None, None, None, None) == bad
    assert b"null pointer" in lib.mpf_last_error()
    assert lib.mpf_volume_render_bwd(None, one, one, None, 5000, 16, 0, 0, None, None, None, None, None, None, one, None, None) == bad
    assert lib.mpf_volume_render_bwd(None, one, one, None, 4, 0, 0, 0, None, None, None, None, None, None, one, None, None) == bad
    assert lib.mpf_volume_render_bwd(None, one, one, one, 4, 16, 5, 0, None, None, None, None, None, None, one, None, None) == bad
    assert lib.mpf_volume_render_bwd(None, one, one, None, 4, 16, 2, 0, None, None, None, None, None, None, one, None, None) == bad
    assert lib.mpf_volume_render_bwd(None, one, one, None, 4, 16, 0, 0, one, None, None, None, None, None, one, None, None) == bad
    assert lib.mpf_volume_render_bwd(one, one, one, one, 4, 16, 2, 1, None, None, one, None, None, None, one, one, None) == bad and b"hard" in lib.mpf_last_error()
    assert lib.mpf_homography_sample_bwd(None, None, 4, 3, 8, 8, 0, 3, None, None) == bad
    assert lib.mpf_homography_sample_bwd(one, one, 4, 3, 8, 8, 2, 2, one, None) == bad and b"channel range" in lib.mpf_last_error()
    assert lib.mpf_homography_sample_bwd(one, one, 4, 3, 8, 8, 0, 4, one, None) == bad
    assert lib.mpf_homography_sample_bwd(one, one, 70000, 3, 8, 8, 0, 3, one, None) == bad
    assert lib.mpf_homography_sample_bwd(one, one, 4, 3, 1 << 16, 1 << 16, 0, 3, one, None) == bad
    assert lib.mpf_warp_composite_bwd(None, None, None, None, 4, 8, 8, None, None, None, None, None, None) == bad
    assert lib.mpf_warp_composite_bwd(one, one, None, one, 5000, 8, 8, one, None, None, one, one, None) == bad and b"bad shape" in lib.mpf_last_error()
    assert lib.mpf_warp_composite_bwd(one, one, None, one, 4, 1 << 14, 1 << 14, one, None, None, one, one, None) == bad
    assert lib.mpf_warp_composite_bwd(one, one, None, one, 4, 8, 8, one, None, one, one, one, None) == bad and b"quads" in lib.mpf_last_error()
    assert lib.mpf_warp_composite_bwd(one, one, ctypes.c_void_p(260), one, 4, 8, 8, one, None, None, one, one, None) == bad


@pytest.mark.parametrize("name", ["s1_mask", "s5_mask"])
def test_restated_baseline_reproduces_the_reference_gradients(name):
    """tests/render_grad_restated.py - the torch baseline of tools/bench_render_grad.py - in float64 on the CPU against the golden"""
    import render_grad_restated as rr
    g = load_golden("render_grad")
    p = "rtd/%s/" % name
    S = int(g[p + "settings"][0])
    d = mk.draw(int(g[p + "seed"]), S, True)
    disp, G, K, Kinv = (torch.from_numpy(a).double() for a in mk.geometry(S))
    leaves = [torch.from_numpy(d[k]).double().requires_grad_(True) for k in ("rgb", "sigma", "obj_mask")]
    rgb, depth, tgt_mask, flow, om = rr.render_tgt_rgb_depth(leaves[0], leaves[1], disp, G, Kinv, K, obj_mask=leaves[2])
    up = lambda k: torch.from_numpy(d[k]).double()
    loss = (rgb * up("g_rgb")).sum() + (depth * up("g_depth")).sum() + (flow * up("g_flow2")).sum() + (om * up("g_mask")).sum()
    grads = torch.autograd.grad(loss, leaves)
    for k, out in (("rgb", rgb), ("depth", depth), ("tgt_mask", tgt_mask), ("flowA2B", flow), ("obj_mask", om)):
        assert np.abs(out.detach().numpy() - g[p + "full/out/" + k]).max() <= 1e-9 * max(1.0, np.abs(g[p + "full/out/" + k]).max()), k
    for k, gr in zip(("mpi_rgb_src", "mpi_sigma_src", "obj_mask"), grads):
        g64 = g[p + "full/g64/" + k]
        assert np.abs(gr.numpy() - g64).max() <= 1e-9 * np.abs(g64).max(), k
