"""The training-time half of utils/mpi on the GPU - gather_pixel_by_pxpy, the uniform disparity samplers, sample_pdf and
disparity_consistency_src_to_tgt - against tests/golden/mpi_training.npz (the reference's own runs and the float64 restatement, written by
tests/golden/make_mpi_training_golden.py).

Tolerance, per tensor, nothing excluded: max|x - f64| / max|f64| <= max(4 * e_ref, 1e-6), e_ref being the reference's own float32 run against float64
(the bar of tests/test_render_geom_grad.py).  The `empty` loss case must give the recorded NaN and zero gradients.  The gather is compared bit for bit:
its upstream gradients are small integers, so every order of the atomic adds gives the same float.  The shapes are the golden's: 5 x 7 (less than a
wave), 24 x 40, 33 x 65 (odd, 27 blocks of partials over three batch entries with their own matrices); sample_pdf at S = 1, at the limits S = N_samples =
128 (the 32-row tile) and at 260 rows of S = 70 (the 64-row tile would not fit: 32 rows, a partial last tile), 100 rows of S = 8 (64-row tiles, a
partial one)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, bits_equal, load_golden

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_mpi_training_golden as mg  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def gold():
    import __graft_entry__ as ge
    ge.build()
    return load_golden("mpi_training")


@pytest.fixture(scope="module")
def mods(gold):
    from mpiflow_amd import _lib, ops
    from mpiflow_amd.utils.mpi import mpi_rendering as R
    from mpiflow_amd.utils.mpi import rendering_utils as U
    from mpiflow_amd.utils.mpi.homography_sampler import HomographySample
    return _lib, ops, R, U, HomographySample


def t(x, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV).requires_grad_(grad)


def close(name, x, f64, e_ref):
    x = x.detach().cpu().numpy().astype(np.float64).reshape(f64.shape)
    err, bar = float(np.abs(x - f64).max() / np.abs(f64).max()), max(4.0 * float(e_ref), 1e-6)
    print("%s: err %.3e  e_ref %.3e  bar %.3e" % (name, err, float(e_ref), bar))
    assert np.isfinite(x).all(), name
    return (name, err, bar)


def settle(report):
    bad = [r for r in report if not r[1] <= r[2]]
    assert not bad, bad


def loss_case(gold, name, mods, grad=True):
    _, _, R, _, HomographySample = mods
    k = "loss/%s/" % name
    ds, dt = t(gold[k + "disparity_src"], grad), t(gold[k + "disparity_tgt"], grad)
    B, _, H, W = ds.shape
    mesh = HomographySample(H, W, torch.device(DEV)).meshgrid
    loss = R.disparity_consistency_src_to_tgt(mesh, t(gold[k + "K_src_inv"]), ds, t(gold[k + "G_tgt_src"]), t(gold[k + "K_tgt"]), dt)
    return k, loss, ds, dt


@pytest.mark.parametrize("name", mg.LOSS_CASES)
def test_loss_and_both_gradients(gold, mods, name):
    k, loss, ds, dt = loss_case(gold, name, mods)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
    loss.backward()
    if name == "empty":
        assert np.isnan(gold[k + "ref32/loss"]) and bool(torch.isnan(loss))
        assert not gold[k + "ref32/grad_src"].any() and not ds.grad.any() and not dt.grad.any()
        return
    report = [close(k + "loss", loss, gold[k + "f64/loss"], gold[k + "e_ref/loss"]),
              close(k + "grad_src", ds.grad, gold[k + "f64/grad_src"], gold[k + "e_ref/grad_src"]),
              close(k + "grad_tgt", dt.grad, gold[k + "f64/grad_tgt"], gold[k + "e_ref/grad_tgt"])]
    settle(report)


def test_loss_works_without_gradients_and_with_one_leaf(gold, mods):
    k, loss, ds, dt = loss_case(gold, "b2_24x40", mods)
    _, plain, _, _ = loss_case(gold, "b2_24x40", mods, grad=False)
    assert not plain.requires_grad and bits_equal(plain.cpu().numpy(), loss.detach().cpu().numpy()) == 0
    with torch.no_grad():
        assert not loss_case(gold, "b2_24x40", mods)[1].requires_grad
    g_src, = torch.autograd.grad(loss, [ds])
    settle([close(k + "grad_src alone", g_src, gold[k + "f64/grad_src"], gold[k + "e_ref/grad_src"])])
    # an upstream gradient other than 1 scales both
    _, loss2, ds2, dt2 = loss_case(gold, "b2_24x40", mods)
    (loss2 * 3.0).backward()
    settle([close(k + "3 x grad_src", ds2.grad, 3.0 * gold[k + "f64/grad_src"], gold[k + "e_ref/grad_src"]),
            close(k + "3 x grad_tgt", dt2.grad, 3.0 * gold[k + "f64/grad_tgt"], gold[k + "e_ref/grad_tgt"])])


def test_loss_and_source_gradient_are_reproducible(gold, mods):
    for name in ("b3_33x65", "collide"):
        runs = []
        for _ in range(2):
            _, loss, ds, _ = loss_case(gold, name, mods)
            loss.backward()
            runs.append((loss.detach().cpu().numpy(), ds.grad.cpu().numpy()))
        assert bits_equal(runs[0][0], runs[1][0]) == 0 and bits_equal(runs[0][1], runs[1][1]) == 0


@pytest.mark.parametrize("name,C,kind", mg.GATHER_CASES)
def test_gather_forward_and_backward_bit_for_bit(gold, mods, name, C, kind):
    _, _, _, U, _ = mods
    k = "gather/%s/" % name
    img, pxpy = t(gold[k + "img"], True), t(gold[k + "pxpy"])
    out = U.gather_pixel_by_pxpy(img, pxpy)
    assert bits_equal(out.detach().cpu().numpy(), gold[k + "out"]) == 0
    out.backward(t(gold[k + "grad_out"]))
    assert bits_equal(img.grad.cpu().numpy(), gold[k + "grad_img"]) == 0
    assert bits_equal(U.gather_pixel_by_pxpy(img.detach(), pxpy).cpu().numpy(), gold[k + "out"]) == 0
    if kind == "i64":                                             # any integer dtype, and the same numbers as float32
        assert bits_equal(U.gather_pixel_by_pxpy(img.detach(), pxpy.to(torch.int32)).cpu().numpy(), gold[k + "out"]) == 0
        assert bits_equal(U.gather_pixel_by_pxpy(img.detach(), pxpy.to(torch.float32)).cpu().numpy(), gold[k + "out"]) == 0


def test_gather_non_finite_coordinates_and_dtypes(gold, mods):
    _, _, _, U, _ = mods
    img = torch.arange(2 * 4 * 5, dtype=torch.float32, device=DEV).view(1, 2, 4, 5)
    pxpy = torch.tensor([[[float("nan"), float("-inf"), float("inf"), 1e30, 2.5, 3.5], [float("inf"), 1.0, float("nan"), -1e30, 0.5, 1.5]]], device=DEV)
    want = torch.tensor([15.0, 5.0, 4.0, 4.0, 2.0, 14.0], device=DEV)                # (0,3) (0,1) (4,0) (4,0) (2,0) (4,2)
    out = U.gather_pixel_by_pxpy(img, pxpy)
    assert torch.equal(out[0, 0], want) and torch.equal(out[0, 1], want + 20.0)
    for bad in (torch.float64, torch.float16):
        with pytest.raises(UnboundLocalError, match="pxpy_int"):
            U.gather_pixel_by_pxpy(img, pxpy.to(bad))
    pxpy.requires_grad_(True)
    img.requires_grad_(True)
    U.gather_pixel_by_pxpy(img, pxpy).sum().backward()
    assert pxpy.grad is None and float(img.grad.sum()) == 12.0


def pdf_case(gold, name):
    k = "pdf/%s/" % name
    values, weights, u = t(gold[k + "values"]), t(gold[k + "weights"]), t(gold[k + "u"])
    return k, values, weights, u


@pytest.mark.parametrize("name", mg.PDF_CASES)
def test_ops_sample_pdf(gold, mods, name):
    _, ops, _, _, _ = mods
    k, values, weights, u = pdf_case(gold, name)
    expanded = values.expand(weights.shape)
    contiguous = expanded.contiguous()
    out = ops.sample_pdf(contiguous, weights, u)
    assert out.shape == u.shape
    settle([close(k + "samples", out, gold[k + "f64"], gold[k + "e_ref"])])
    again = torch.empty_like(out)
    assert ops.sample_pdf(contiguous, weights, u, out=again) is again and bits_equal(out.cpu().numpy(), again.cpu().numpy()) == 0
    if values.shape[2] == 1:                                      # the expanded layout, read in place
        assert not expanded.is_contiguous() and expanded.stride(2) == 0
        assert bits_equal(ops.sample_pdf(expanded, weights, u).cpu().numpy(), out.cpu().numpy()) == 0
    else:                                                          # every case also with its first row expanded over the rays
        first = contiguous[:, :, 0:1, :].contiguous()
        a = ops.sample_pdf(first.expand(weights.shape), weights, u)
        b = ops.sample_pdf(first.expand(weights.shape).contiguous(), weights, u)
        assert bits_equal(a.cpu().numpy(), b.cpu().numpy()) == 0


def test_generator_replay(gold, mods):
    _, ops, _, U, _ = mods
    k, values, weights, u = pdf_case(gold, "n130_s70")
    values = values.expand(weights.shape)
    B, _, N, S = weights.shape
    torch.manual_seed(1234)
    got = U.sample_pdf(values, weights, 7)
    state = torch.cuda.get_rng_state()
    torch.manual_seed(1234)
    want = ops.sample_pdf(values, weights, torch.rand((B, 1, N, 7), dtype=torch.float32, device=weights.device))
    assert torch.equal(state, torch.cuda.get_rng_state()) and bits_equal(got.cpu().numpy(), want.cpu().numpy()) == 0
    edges = np.linspace(1.0, 0.01, 33).astype(np.float32)
    for fn, args in ((U.uniformly_sample_disparity_from_bins, (3, edges)), (U.uniformly_sample_disparity_from_linspace_bins, (3, 32, 1.0, 0.01))):
        torch.manual_seed(77)
        got = fn(*args, torch.device(DEV))
        state = torch.cuda.get_rng_state()
        torch.manual_seed(77)
        r = torch.rand((3, 32), dtype=torch.float32, device=DEV)
        assert torch.equal(state, torch.cuda.get_rng_state())
        e = torch.from_numpy(edges).to(DEV) if len(args) == 2 else torch.linspace(1.0, 0.01, 33, dtype=torch.float32, device=DEV)
        interval = (e[1:] - e[:-1]).unsqueeze(0).repeat(3, 1) if len(args) == 2 else e[1] - e[0]
        assert got.shape == (3, 32) and got.is_cuda and torch.equal(got, e[:-1].unsqueeze(0).repeat(3, 1) + interval * r)


def test_refusals_name_their_argument(gold, mods):
    _lib, ops, R, U, HomographySample = mods
    E = _lib.MpiFlowHipError
    k = "loss/b1_5x7/"
    Ki, G, Kt, ds, dt = (t(gold[k + n]) for n in ("K_src_inv", "G_tgt_src", "K_tgt", "disparity_src", "disparity_tgt"))
    mesh = HomographySample(5, 7, torch.device(DEV)).meshgrid
    for name, args in (("K_src_inv", (Ki.clone().requires_grad_(True), ds, G, Kt, dt)), ("G_tgt_src", (Ki, ds, G.clone().requires_grad_(True), Kt, dt)),
                       ("K_tgt", (Ki, ds, G, Kt.clone().requires_grad_(True), dt))):
        with pytest.raises(E, match="%s requires grad" % name):
            R.disparity_consistency_src_to_tgt(mesh, *args)
    with pytest.raises(E, match=r"disparity_tgt must have disparity_src's shape \(1, 1, 5, 7\) \(got \(1, 1, 5, 8\)\)"):
        R.disparity_consistency_src_to_tgt(mesh, Ki, ds, G, Kt, torch.ones(1, 1, 5, 8, device=DEV))
    with pytest.raises(E, match="meshgrid_homo"):
        R.disparity_consistency_src_to_tgt(HomographySample(5, 8, torch.device(DEV)).meshgrid, Ki, ds, G, Kt, dt)
    with pytest.raises(E, match="meshgrid_homo"):
        R.disparity_consistency_src_to_tgt(HomographySample(5, 7).meshgrid + 1.0, Ki, ds, G, Kt, dt)
    with pytest.raises(E, match="disparity_src must live on the GPU"):
        R.disparity_consistency_src_to_tgt(mesh, Ki.cpu(), ds.cpu(), G.cpu(), Kt.cpu(), dt.cpu())
    with pytest.raises(E, match="disparity_tgt must be float32"):
        R.disparity_consistency_src_to_tgt(mesh, Ki, ds, G, Kt, dt.double())
    with pytest.raises(E, match="disparity_src must be contiguous"):
        R.disparity_consistency_src_to_tgt(HomographySample(7, 5, torch.device(DEV)).meshgrid, Ki, ds.transpose(2, 3), G, Kt, dt.transpose(2, 3).contiguous())
    # the matrices may live on the host: they are moved, the loss is the same
    a = R.disparity_consistency_src_to_tgt(mesh.cpu(), Ki.cpu(), ds, G.cpu(), Kt.cpu(), dt)
    assert bits_equal(a.cpu().numpy(), R.disparity_consistency_src_to_tgt(mesh, Ki, ds, G, Kt, dt).cpu().numpy()) == 0

    _, values, weights, u = pdf_case(gold, "b2_n50_s8")
    for name, args in (("values", (values.clone().requires_grad_(True), weights)), ("weights", (values, weights.clone().requires_grad_(True)))):
        with pytest.raises(E, match="%s requires grad.*detach %s" % (name, name)):
            U.sample_pdf(*args, 4)
    with torch.no_grad():
        assert U.sample_pdf(values.clone().requires_grad_(True), weights, 4).shape == (2, 1, 50, 4)
    with pytest.raises(E, match="values must be contiguous, or expanded"):
        ops.sample_pdf(values.transpose(0, 2).contiguous().transpose(0, 2), weights, u)
    with pytest.raises(E, match="weights must be contiguous"):
        ops.sample_pdf(values, weights.transpose(0, 2).contiguous().transpose(0, 2), u)
    with pytest.raises(E, match="u must be float32"):
        ops.sample_pdf(values, weights, u.double())
    with pytest.raises(E, match="values must be float32"):
        ops.sample_pdf(values.half(), weights, u)
    with pytest.raises(E, match="values must live on the GPU"):
        ops.sample_pdf(values.cpu(), weights.cpu(), u.cpu())
    big = torch.rand(1, 1, 4, 129, device=DEV)
    with pytest.raises(E, match=r"S must be 1\.\.128 \(got 129"):
        ops.sample_pdf(big, big, torch.rand(1, 1, 4, 3, device=DEV))
    with pytest.raises(E, match=r"n_samples must be 1\.\.128 \(got 129"):
        ops.sample_pdf(values, weights, torch.rand(2, 1, 50, 129, device=DEV))
    with pytest.raises(E, match="S must be"):
        U.sample_pdf(big, big, 3)

    img = torch.zeros(1, 2, 4, 5, device=DEV)
    with pytest.raises(UnboundLocalError):
        U.gather_pixel_by_pxpy(img, torch.zeros(1, 2, 3, dtype=torch.float64, device=DEV))
    with pytest.raises(E, match="pxpy must be contiguous"):
        U.gather_pixel_by_pxpy(img, torch.zeros(1, 3, 2, device=DEV).transpose(1, 2))
    with pytest.raises(E, match="img must be float32"):
        U.gather_pixel_by_pxpy(img.double(), torch.zeros(1, 2, 3, device=DEV))
    with pytest.raises(E, match="img must live on the GPU"):
        U.gather_pixel_by_pxpy(img.cpu(), torch.zeros(1, 2, 3))
