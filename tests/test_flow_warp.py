"""GPU tests of the flow warps (mpiflow_amd.utils.transform.warp / warp_rife, ops.flow_warp / flow_warp_backward, mpf_flow_warp.hip) against
tests/golden/flow_warp.npz, recorded from the reference: every tensor within max(4 e_ref, 1e-6) of the reference's float64 run, relative to that
tensor's largest magnitude (the bar of tests/test_render_geom_grad.py, per tensor, nothing excluded).

Errors measured on an MI355X (err / e_ref of the reference's own float32 run), largest over the four shapes:
    warp       out 6.6e-06 / 6.6e-06   mask 5.5e-06 / 5.5e-06   grad_x 2.9e-06 / 2.9e-06   grad_flow 6.0e-06 / 6.0e-06
    warp_rife  out 5.2e-06 / 5.2e-06                            grad_x 8.4e-07 / 8.4e-07   grad_flow 2.1e-06 / 2.1e-06"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, bits_equal, load_golden

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flow_warp_restated as rs  # noqa: E402
import make_flow_warp_golden as mg  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def gold():
    import __graft_entry__ as ge
    ge.build()
    return load_golden("flow_warp")


@pytest.fixture(scope="module")
def mods(gold):
    from mpiflow_amd import _lib, ops
    from mpiflow_amd.utils import transform as T
    return _lib, ops, T


def t(x, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV).requires_grad_(grad)


def n(x):
    return x.detach().cpu().numpy()


def close(name, x, f64, e_ref):
    x = n(x).astype(np.float64).reshape(f64.shape)
    err, bar = float(np.abs(x - f64).max() / np.abs(f64).max()), max(4.0 * float(e_ref), 1e-6)
    print("%s: err %.3e  e_ref %.3e  bar %.3e" % (name, err, float(e_ref), bar))
    assert np.isfinite(x).all(), name
    return (name, err, bar)


def settle(report):
    bad = [r for r in report if not r[1] <= r[2]]
    assert not bad, bad


def run(T, mode, x, flow, g=None):
    """-> out, mask | None (and after backward the leaves' .grad)"""
    if mode == "warp":
        out, mask = T.warp(x, flow)
    else:
        out, mask = T.warp_rife(x, flow), None
    if g is not None:
        out.backward(g)
    return out, mask


@pytest.mark.parametrize("mode", list(mg.MODES))
@pytest.mark.parametrize("name", list(mg.CASES))
def test_values_and_gradients_against_the_reference(gold, mods, name, mode):
    _, _, T = mods
    x, flow, g = t(gold[name + "/x"], True), t(gold[name + "/flow"], True), t(gold[name + "/g"])
    out, mask = run(T, mode, x, flow, g)
    k = "%s/%s/" % (name, mode)
    got = dict(out=out, grad_x=x.grad, grad_flow=flow.grad)
    if mode == "warp":
        got["mask"] = mask[:, :1]
        assert mask.shape == out.shape
    assert out.shape == x.shape and out.dtype == torch.float32 and flow.grad.shape == flow.shape
    settle([close(k + f, v, rs.golden_f64(gold, name, mode, f), gold[k + "e_ref/" + f]) for f, v in got.items()])


def test_rife_zero_flow_returns_the_input(gold, mods):
    _, _, T = mods
    x = t(gold["rife/zero_flow/x"])
    out = T.warp_rife(x, torch.zeros((x.shape[0], 2) + tuple(x.shape[2:]), device=DEV))
    want = gold["rife/zero_flow/out"]
    err = float(np.abs(n(out) - want).max() / np.abs(want).max())
    print("rife/zero_flow: err %.3e" % err)
    assert err <= 1e-6                                           # against the reference's float32 output: the float32 rounding of (g + 1) / 2 * (W - 1)


def test_mask_is_expanded_detached_and_one_inside(gold, mods):
    _lib, ops, T = mods
    for name in mg.CASES:
        x, flow = t(gold[name + "/x"], True), t(gold[name + "/flow"], True)
        out, mask = T.warp(x, flow)
        assert out.requires_grad and not mask.requires_grad and mask.grad_fn is None
        assert mask.shape == x.shape and (mask.stride(1) == 0 or x.shape[1] == 1)               # [B,1,H,W] expanded, not copied
        _, m1 = ops.flow_warp(x.detach(), flow.detach(), _lib.FLOW_WARP_WARP, True)
        assert m1.shape == (x.shape[0], 1) + tuple(x.shape[2:])
        assert bits_equal(n(mask), np.broadcast_to(n(m1), tuple(x.shape)).copy()) == 0
        r = rs.flow_warp(gold[name + "/x"], gold[name + "/flow"], rs.WARP)
        inside = r["all_in"]
        assert inside.any() and np.abs(n(m1)[:, 0][inside] - 1.0).max() <= 1e-6
        assert (n(m1)[r["mask"] == 0] == 0).all()
        if x.shape[1] > 1:
            with pytest.raises(RuntimeError):
                mask.add_(1.0)


def test_reproducible_and_the_same_bytes_whole_or_split(gold, mods):
    _lib, ops, T = mods
    name = "b1_c70_9x11"
    x, flow, g = t(gold[name + "/x"]), t(gold[name + "/flow"]), t(gold[name + "/g"])
    for mode in (_lib.FLOW_WARP_WARP, _lib.FLOW_WARP_RIFE):
        o1, _ = ops.flow_warp(x, flow, mode, False)
        o2, _ = ops.flow_warp(x, flow, mode, False)
        ow, _ = ops.flow_warp(x, flow, mode, False, whole=True)
        assert bits_equal(n(o1), n(o2)) == 0 and bits_equal(n(o1), n(ow)) == 0
        _, f1 = ops.flow_warp_backward(x, flow, g, mode, want_x=False)
        _, f2 = ops.flow_warp_backward(x, flow, g, mode, want_x=False)
        gx, f3 = ops.flow_warp_backward(x, flow, g, mode)                                        # the kernel that also scatters grad_x
        _, fw = ops.flow_warp_backward(x, flow, g, mode, want_x=False, whole=True)               # one thread walks both chunks
        gxw, fw2 = ops.flow_warp_backward(x, flow, g, mode, whole=True)
        assert f1.abs().max() > 0
        for other in (f2, f3, fw, fw2):
            assert bits_equal(n(f1), n(other)) == 0
        assert float((gx - gxw).abs().max()) <= 1e-5 * float(gx.abs().max())
    for name in ("b2_c3_24x40", "b3_c2_33x65"):
        x, flow, g = t(gold[name + "/x"]), t(gold[name + "/flow"]), t(gold[name + "/g"])
        for mode in (_lib.FLOW_WARP_WARP, _lib.FLOW_WARP_RIFE):
            a = ops.flow_warp_backward(x, flow, g, mode)[1], ops.flow_warp(x, flow, mode, False)[0]
            b = ops.flow_warp_backward(x, flow, g, mode)[1], ops.flow_warp(x, flow, mode, False)[0]
            assert bits_equal(n(a[0]), n(b[0])) == 0 and bits_equal(n(a[1]), n(b[1])) == 0


@pytest.mark.parametrize("mode", list(mg.MODES))
def test_grad_x_with_integer_gradients_and_dyadic_weights(mods, mode):
    """flows whose sample positions have dyadic fractions (multiples of 1/8 for warp_rife; for warp the coordinate's own scale W / (W - 1) is
    made dyadic by W = 9, H = 5), small-integer upstream gradients: every product is exact and every sum of a few of them too, so the order of the
    atomic adds cannot show.  Compared with the restatement within the tolerance of the suite only: grad_x's bits are not promised."""
    _, _, T = mods
    rng = np.random.default_rng(11)
    B, C, H, W = 2, 3, 5, 9
    x = (rng.integers(-128, 129, (B, C, H, W)) / 64.0).astype(np.float32)
    g = rng.integers(-4, 5, (B, C, H, W)).astype(np.float32)
    flow = (rng.integers(-8 * 12, 8 * 12 + 1, (B, 2, H, W)) / 8.0).astype(np.float32)
    code = mg.MODES[mode]
    r = rs.flow_warp(x, flow, code, g)
    xt, ft = t(x, True), t(flow)
    run(T, mode, xt, ft, t(g))
    assert ft.grad is None
    err = float(np.abs(n(xt.grad) - r["grad_x"]).max() / np.abs(r["grad_x"]).max())
    print("grad_x %s: err %.3e" % (mode, err))
    assert err <= 1e-6


def test_gradient_routing(gold, mods):
    _, _, T = mods
    name = "b2_c3_24x40"
    for mode in mg.MODES:
        g = t(gold[name + "/g"])
        x, flow = t(gold[name + "/x"], True), t(gold[name + "/flow"], True)
        out, _ = run(T, mode, x, flow, g)
        gx, gf = x.grad, flow.grad
        with torch.no_grad():
            plain, _ = run(T, mode, x, flow)
        assert not plain.requires_grad and bits_equal(n(plain), n(out)) == 0
        plain2, m2 = run(T, mode, x.detach(), flow.detach())                                     # neither requires grad
        assert not plain2.requires_grad and plain2.grad_fn is None and bits_equal(n(plain2), n(out)) == 0
        # only x
        x1, f1 = t(gold[name + "/x"], True), t(gold[name + "/flow"])
        o1, _ = run(T, mode, x1, f1, g)
        assert f1.grad is None and bits_equal(n(o1), n(out)) == 0
        assert float((x1.grad - gx).abs().max()) <= 1e-5 * float(gx.abs().max())                 # atomics: the last bits may differ
        # only flo
        x2, f2 = t(gold[name + "/x"]), t(gold[name + "/flow"], True)
        run(T, mode, x2, f2, g)
        assert x2.grad is None and bits_equal(n(f2.grad), n(gf)) == 0
        # a non-leaf flow: flo = 2 p routes 2 grad_flow to p
        p = t(gold[name + "/flow"] * np.float32(0.5), True)
        run(T, mode, x2, 2 * p, g)
        assert bits_equal(n(p.grad), n(2 * gf)) == 0


def test_refusals_raise_before_launch(gold, mods):
    _lib, ops, T = mods
    E = _lib.MpiFlowHipError
    x, f = torch.zeros(2, 3, 4, 5, device=DEV), torch.zeros(2, 2, 4, 5, device=DEV)
    for fn in (T.warp, T.warp_rife):
        with pytest.raises(E, match=r"x must be float32.*\.float\(\)"):
            fn(x.half(), f)
        with pytest.raises(E, match=r"x must be float32.*\.float\(\)"):
            fn(x.double(), f)
        with pytest.raises(E, match=r"flow must be float32.*\.float\(\)"):
            fn(x, f.double())
        with pytest.raises(E, match="no CPU path"):
            fn(x.cpu(), f.cpu())
        with pytest.raises(E, match="flow must live on the GPU"):
            fn(x, f.cpu())
        with pytest.raises(E, match="flow must have x's batch size"):
            fn(x, f[:1])
        with pytest.raises(E, match=r"flow must be \[B,2,H,W\]"):
            fn(x, torch.zeros(2, 3, 4, 5, device=DEV))
        with pytest.raises(E, match=r"flow must be \[B,2,H,W\]"):
            fn(x, torch.zeros(2, 2, 4, 6, device=DEV))
    with pytest.raises(E, match="at least 2"):
        T.warp_rife(torch.zeros(2, 3, 4, 1, device=DEV), torch.zeros(2, 2, 4, 1, device=DEV))
    out, mask = T.warp(torch.ones(1, 2, 3, 1, device=DEV), torch.zeros(1, 2, 3, 1, device=DEV))  # warp takes W = 1: max(W - 1, 1)
    assert out.shape == (1, 2, 3, 1) and torch.isfinite(out).all()
    with pytest.raises(E, match="no mask"):
        ops.flow_warp(x, f, _lib.FLOW_WARP_RIFE, True)
    with pytest.raises(E, match="out must be"):
        ops.flow_warp(x, f, _lib.FLOW_WARP_WARP, False, out=torch.zeros(2, 3, 4, 6, device=DEV))
    # double backward
    xg, fg = x.clone().requires_grad_(True), f.clone().requires_grad_(True)
    o, _ = T.warp(xg, fg)
    (gx,) = torch.autograd.grad((o * o).sum(), xg, create_graph=True)                            # an upstream gradient that itself requires grad
    with pytest.raises(RuntimeError, match="once_differentiable|twice"):
        gx.sum().backward()


def test_non_contiguous_x_gives_the_contiguous_bits(gold, mods):
    _, _, T = mods
    name = "b2_c3_24x40"
    x, flow = t(gold[name + "/x"]), t(gold[name + "/flow"])
    xcl = x.contiguous(memory_format=torch.channels_last)
    assert not xcl.is_contiguous()
    for mode in mg.MODES:
        a, ma = run(T, mode, x, flow)
        b, mb = run(T, mode, xcl, flow)
        assert bits_equal(n(a), n(b)) == 0
        xg = xcl.clone(memory_format=torch.preserve_format).requires_grad_(True)
        c, _ = run(T, mode, xg, flow, t(gold[name + "/g"]))
        assert bits_equal(n(a), n(c)) == 0 and xg.grad.shape == x.shape


def test_transform_raises(mods):
    _, _, T = mods
    with pytest.raises(NotImplementedError, match="cv2.remap"):
        T.transform(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 2), np.float32))


def test_non_finite_flow_stays_in_bounds(mods):
    """a NaN or infinite flow samples outside the image (warp: 0, mask 0) or at the clamped border (warp_rife): finite outputs, no fault"""
    _, _, T = mods
    x = torch.ones(1, 2, 6, 7, device=DEV)
    f = torch.zeros(1, 2, 6, 7, device=DEV)
    f[0, 0, 0, 0], f[0, 1, 1, 1], f[0, 0, 2, 2], f[0, 0, 3, 3] = float("nan"), float("inf"), float("-inf"), 3e38
    out, mask = T.warp(x, f)
    assert torch.isfinite(out).all() and float(mask[0, 0, 0, 0]) == 0 and float(out[0, 0, 1, 1]) == 0 and float(out[0, 1, 2, 2]) == 0
    assert torch.isfinite(T.warp_rife(x, f)).all()
