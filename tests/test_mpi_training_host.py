"""CPU checks for the training-time half of utils/mpi (gather_pixel_by_pxpy, the uniform disparity samplers, sample_pdf,
disparity_consistency_src_to_tgt): the golden tests/golden/mpi_training.npz is intact and covers what tests/golden/make_mpi_training_golden.py
promises, tests/mpi_training_restated.py reproduces its float64 values, the C ABI declares the new calls, and the five names import from the two
drop-in modules."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_mpi_training_golden as mg  # noqa: E402
import mpi_training_restated as rs  # noqa: E402

NEW_SYMBOLS = ("mpf_gather_pxpy", "mpf_gather_pxpy_bwd", "mpf_sample_pdf", "mpf_disp_consistency", "mpf_disp_consistency_bwd",
               "mpf_disp_consistency_workspace")


@pytest.fixture(scope="module")
def gold():
    return load_golden("mpi_training")


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_golden_is_intact(gold):
    for name in mg.LOSS_CASES:
        k = "loss/%s/" % name
        for f in ("K_src_inv", "G_tgt_src", "K_tgt", "disparity_src", "disparity_tgt", "cov", "ref32/loss", "ref32/grad_src", "ref32/grad_tgt", "f64/loss",
                  "f64/grad_src", "f64/grad_tgt", "e_ref/loss", "e_ref/grad_src", "e_ref/grad_tgt"):
            assert k + f in gold, k + f
        assert gold[k + "disparity_src"].dtype == np.float32 and gold[k + "f64/grad_src"].dtype == np.float64
        assert gold[k + "disparity_src"].shape == gold[k + "disparity_tgt"].shape == gold[k + "f64/grad_tgt"].shape
    for name in mg.PDF_CASES:
        k = "pdf/%s/" % name
        assert gold[k + "f64"].shape == gold[k + "u"].shape == gold[k + "ref32"].shape and gold[k + "f64"].dtype == np.float64
    for name, C, kind in mg.GATHER_CASES:
        k = "gather/%s/" % name
        assert gold[k + "img"].shape[1] == C and gold[k + "pxpy"].dtype == (np.int64 if kind == "i64" else np.float32)
    assert os.path.getsize(os.path.join(GOLDEN, "mpi_training.npz")) < 1 << 20


def test_loss_cases_keep_clear_of_discrete_flips_and_cover_what_they_name(gold):
    shapes = {"b1_5x7": (1, 5, 7), "b2_24x40": (2, 24, 40), "b3_33x65": (3, 33, 65)}
    for name in mg.LOSS_CASES:
        k = "loss/%s/" % name
        cov = dict(zip(mg.COV, gold[k + "cov"].tolist()))
        r = rs.disparity_consistency(gold[k + "K_src_inv"], gold[k + "disparity_src"], gold[k + "G_tgt_src"], gold[k + "K_tgt"], gold[k + "disparity_tgt"])
        B, _, H, W = gold[k + "disparity_src"].shape
        assert mg.loss_coverage(r, H, W).tolist() == gold[k + "cov"].tolist(), name
        assert cov["near_boundary"] == 0, name
        assert (cov["count"] == 0) == (name == "empty"), name
        if name in shapes:
            assert (B, H, W) == shapes[name]
    cov = lambda name: dict(zip(mg.COV, gold["loss/%s/cov" % name].tolist()))          # noqa: E731
    assert min(cov("mostly_out")[s] for s in ("out_left", "out_right", "out_top", "out_bottom", "count")) > 0
    assert cov("collide")["max_collisions"] >= 4 and cov("behind")["behind_in_mask"] > 0
    assert np.isnan(gold["loss/empty/f64/loss"]) and np.isnan(gold["loss/empty/ref32/loss"])
    assert not gold["loss/empty/ref32/grad_src"].any() and not gold["loss/empty/ref32/grad_tgt"].any()
    # different matrices per batch entry
    assert (gold["loss/b2_24x40/G_tgt_src"][0] != gold["loss/b2_24x40/G_tgt_src"][1]).any() and (gold["loss/b2_24x40/K_tgt"][0] != gold["loss/b2_24x40/K_tgt"][1]).any()


def test_restatement_reproduces_the_float64_loss_and_gradients(gold):
    for name in mg.LOSS_CASES:
        k = "loss/%s/" % name
        r = rs.disparity_consistency(gold[k + "K_src_inv"], gold[k + "disparity_src"], gold[k + "G_tgt_src"], gold[k + "K_tgt"], gold[k + "disparity_tgt"])
        if name == "empty":
            assert np.isnan(r["loss"]) and not r["grad_src"].any() and not r["grad_tgt"].any()
            continue
        assert rel(np.float64(r["loss"]), gold[k + "f64/loss"]) <= 1e-9
        assert rel(r["grad_src"], gold[k + "f64/grad_src"]) <= 1e-9 and rel(r["grad_tgt"], gold[k + "f64/grad_tgt"]) <= 1e-9
        # the reference's own float32 run sits where e_ref says
        assert rel(gold[k + "ref32/grad_src"].astype(np.float64), gold[k + "f64/grad_src"]) == pytest.approx(float(gold[k + "e_ref/grad_src"]), rel=1e-6, abs=1e-12)


def test_sample_pdf_cases_keep_clear_of_flips_and_restate(gold):
    shapes = {"b2_n50_s8": (2, 50, 8, 6), "s1": (1, 20, 1, 4), "n3_s128": (1, 3, 128, 128), "n130_s70": (2, 130, 70, 5)}
    top = np.nextafter(np.float32(1), np.float32(0))
    for name in mg.PDF_CASES:
        k = "pdf/%s/" % name
        values, weights, u = gold[k + "values"], gold[k + "weights"], gold[k + "u"]
        B, _, N, S = weights.shape
        assert (B, N, S, u.shape[3]) == shapes[name]
        r = rs.sample_pdf(np.broadcast_to(values, weights.shape), weights, u)
        assert int(rs.pdf_near_flip(r["cdf"], u, r["cdf_interval"]).sum()) == 0 == int(gold[k + "cov"][0])
        assert rel(r["samples"], gold[k + "f64"]) <= 1e-9
        assert (weights.sum(axis=3) == 0).any() and ((weights != 0).sum(axis=3) == 1).any() and (u == 0).any() and (u == top).any()
        assert rel(gold[k + "ref32"].astype(np.float64), gold[k + "f64"]) == pytest.approx(float(gold[k + "e_ref"]), rel=1e-6, abs=1e-12)
    assert gold["pdf/n130_s70/values"].shape[2] == 1 and gold["pdf/n130_s70/cov"][6] == 1          # the expanded layout


def test_gather_cases_restate_bit_for_bit(gold):
    for name, C, kind in mg.GATHER_CASES:
        k = "gather/%s/" % name
        img, pxpy, g = gold[k + "img"], gold[k + "pxpy"], gold[k + "grad_out"]
        assert (rs.gather_pixel_by_pxpy(img, pxpy) == gold[k + "out"]).all()
        assert (rs.gather_pixel_by_pxpy_backward(g, pxpy, *img.shape[2:]) == gold[k + "grad_img"]).all()
        assert np.abs(g).max() <= 8 and (g == np.round(g)).all()
        if kind == "f32":
            for tie in (0.5, 1.5, 2.5):
                assert (pxpy == tie).any()
            assert (pxpy < 0).any() and (pxpy[:, 0] > img.shape[3]).any()
    assert rs.pixel_index(np.array([0.5, 1.5, 2.5, np.nan, -np.inf, np.inf, -0.5, 1e30]), 9).tolist() == [0, 2, 2, 0, 0, 8, 0, 8]


def test_header_declares_the_new_calls_and_the_ctypes_table_mirrors_them():
    import ctypes
    from mpiflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in _lib.SIGNATURES, n
    for struct, cls in (("MpfGatherPxpyArgs", _lib.MpfGatherPxpyArgs), ("MpfSamplePdfArgs", _lib.MpfSamplePdfArgs),
                        ("MpfDispConsistencyArgs", _lib.MpfDispConsistencyArgs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"[\s*]", "", part.split()[-1]) for part in decl.split(",")]
        assert names == [f[0] for f in cls._fields_], struct
    assert _lib.SAMPLE_PDF_MAX_S == int(re.search(r"#define MPF_SAMPLE_PDF_MAX_S (\d+)", hdr).group(1))
    assert _lib.SAMPLE_PDF_MAX_SAMPLES == int(re.search(r"#define MPF_SAMPLE_PDF_MAX_SAMPLES (\d+)", hdr).group(1))
    assert ctypes.sizeof(_lib.MpfSamplePdfArgs) == 4 * 8 + 2 * 8 + 4 * 4


def test_library_refuses_bad_arguments_without_a_gpu():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    lib = _lib.load()
    assert lib.mpf_sample_pdf(None, None) == 10001 and b"null argument block" in lib.mpf_last_error()
    a = _lib.MpfSamplePdfArgs()
    a.B, a.N, a.S, a.n_samples = 1, 4, 129, 4
    assert lib.mpf_sample_pdf(ctypes.byref(a), None) == 10001 and b"S must be 1..128" in lib.mpf_last_error()
    a.S, a.n_samples = 4, 129
    assert lib.mpf_sample_pdf(ctypes.byref(a), None) == 10001 and b"n_samples must be 1..128" in lib.mpf_last_error()
    a.N, a.S, a.n_samples, a.B = 1 << 24, 128, 4, 1
    assert lib.mpf_sample_pdf(ctypes.byref(a), None) == 10001 and b"2^31" in lib.mpf_last_error()
    assert lib.mpf_disp_consistency_workspace(0, 4, 4) == 0 and lib.mpf_disp_consistency_workspace(2, 33, 65) == 16 + 2 * 9 * 8
    assert lib.mpf_disp_consistency(None, None) == 10001 and lib.mpf_gather_pxpy(None, None) == 10001 and lib.mpf_gather_pxpy_bwd(None, None) == 10001
    d = _lib.MpfDispConsistencyArgs()
    d.B, d.H, d.W = 1, 4, 4
    assert lib.mpf_disp_consistency_bwd(ctypes.byref(d), None) == 10001 and b"null pointer" in lib.mpf_last_error()


def test_the_five_names_import_from_the_two_drop_in_modules():
    from mpiflow_amd.utils.mpi.rendering_utils import (gather_pixel_by_pxpy, sample_pdf, uniformly_sample_disparity_from_bins,  # noqa: F401
                                                       uniformly_sample_disparity_from_linspace_bins)
    from mpiflow_amd.utils.mpi.mpi_rendering import disparity_consistency_src_to_tgt  # noqa: F401
    import inspect
    assert list(inspect.signature(disparity_consistency_src_to_tgt).parameters) == ["meshgrid_homo", "K_src_inv", "disparity_src", "G_tgt_src", "K_tgt",
                                                                                     "disparity_tgt"]
    assert list(inspect.signature(sample_pdf).parameters) == ["values", "weights", "N_samples"]
    assert list(inspect.signature(uniformly_sample_disparity_from_linspace_bins).parameters) == ["batch_size", "num_bins", "start", "end", "device"]
    assert list(inspect.signature(uniformly_sample_disparity_from_bins).parameters) == ["batch_size", "disparity_np", "device"]


def test_the_uniform_samplers_follow_the_reference_on_the_cpu():
    """plain torch: they run wherever `device` says.  One torch.rand((B, S)) each; the asserts of the reference stay."""
    import torch
    from mpiflow_amd.utils.mpi import rendering_utils as U
    edges = np.linspace(1.0, 0.01, 9).astype(np.float32)
    torch.manual_seed(5)
    a = U.uniformly_sample_disparity_from_bins(3, edges, "cpu")
    b = U.uniformly_sample_disparity_from_linspace_bins(3, 8, 1.0, 0.01, "cpu")
    state = torch.get_rng_state()
    torch.manual_seed(5)
    r1, r2 = torch.rand((3, 8)), torch.rand((3, 8))
    assert torch.equal(state, torch.get_rng_state())
    e = torch.from_numpy(edges)
    assert torch.equal(a, e[:-1].unsqueeze(0).repeat(3, 1) + (e[1:] - e[:-1]).unsqueeze(0).repeat(3, 1) * r1)
    lin = torch.linspace(1.0, 0.01, 9, dtype=torch.float32)
    assert torch.equal(b, lin[:-1].unsqueeze(0).repeat(3, 1) + (lin[1] - lin[0]) * r2)
    assert a.shape == b.shape == (3, 8) and (a[:, :-1] > a[:, 1:]).all()
    with pytest.raises(AssertionError):
        U.uniformly_sample_disparity_from_bins(1, edges[::-1].copy(), "cpu")
    with pytest.raises(AssertionError):
        U.uniformly_sample_disparity_from_linspace_bins(1, 8, 0.01, 1.0, "cpu")
