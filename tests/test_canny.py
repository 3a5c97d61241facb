"""ops.canny_masked (mpf_canny.hip), the masked Canny of warp-back stage 2, against tests/canny_restated.py:

restated   INTEGRATION.md section 17 in numpy float32: the kernel must give its bytes - the edges, and each stage alone through `passes` its
           intermediate (smoothed, the class map).  No tolerance: the definition fixes every rounding.
witness    the same detector in float64 on scipy.ndimage, in the shape of skimage's implementation; the restatement must agree with it on
           every pixel of the committed random cases (CPU only).  skimage itself is installed nowhere: parity with it is unpinned.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import canny_restated as R  # noqa: E402
from conftest import bits_equal  # noqa: E402

F32 = np.float32


def same(a, b):
    return bits_equal(a, b) == 0


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def dev(built):
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---------------------------------------------------------------- cases: name -> (gray [b,1,h,w], mask, sigma, low, high)

def _blobs(h, w, seed=5):
    return R.random_case(seed, 1, h, w)[0]


def cases():
    out = {}
    for seed, b, h, w in R.RANDOM_CASES:
        out["random_%dx%dx%d" % (b, h, w)] = R.random_case(seed, b, h, w) + (2.0, 0.1, 0.2)
    h, w = 17, 19
    g = _blobs(h, w)
    ones = np.ones((1, 1, h, w), F32)
    out["mask_ones"] = (g, ones, 2.0, 0.1, 0.2)
    out["mask_zeros"] = (g, np.zeros_like(ones), 2.0, 0.1, 0.2)
    single = np.zeros_like(ones)
    single[0, 0, 8, 9] = 1
    out["single_inside_pixel"] = (g, single, 2.0, 0.1, 0.2)
    border = ones.copy()
    border[0, 0, :6, 12:] = 0
    border[0, 0, 10:, 0] = 0
    out["hole_touching_border"] = (g, border, 1.0, 0.1, 0.2)
    yy, xx = np.mgrid[0:h, 0:w]
    step = np.where(xx >= 9, 1.0, 0.0).astype(F32)[None, None]
    out["axis_step"] = (step, ones, 1.0, 0.1, 0.2)
    out["axis_step_rows"] = (np.where(yy >= 8, 0.0, 1.0).astype(F32)[None, None], ones, 1.0, 0.1, 0.2)
    cut = ones.copy()
    cut[0, 0, :, 10:] = 0                                   # the mask's edge runs along the step: the erosion removes what the cut creates
    out["mask_edge_through_gradient"] = (step + F32(0.3) * g, cut, 1.0, 0.05, 0.1)
    out["constant"] = (np.full((1, 1, h, w), 0.5, F32), ones, 2.0, 0.1, 0.2)
    out["ramp_45"] = (np.clip((xx + yy - 16) * 0.25, 0, 1).astype(F32)[None, None], ones, 1.0, 0.1, 0.2)
    out["ramp_135"] = (np.clip((xx - yy) * 0.25, 0, 1).astype(F32)[None, None], ones, 1.0, 0.1, 0.2)
    edge_max = np.zeros((1, 1, h, w), F32)
    edge_max[0, 0, 0, :] = 1                                # the gradient is largest on row 0 and on column w - 1
    edge_max[0, 0, :, w - 1] = 1
    out["maximum_on_border"] = (edge_max, ones, 1.0, 0.02, 0.05)
    out["thresholds"] = R.random_case(3, 2, 33, 70) + (2.0, 0.03, 0.31)
    out["equal_thresholds"] = R.random_case(2, 1, 17, 19) + (2.0, 0.15, 0.15)
    out["sigma_1"] = R.random_case(3, 2, 33, 70) + (1.0, 0.1, 0.2)
    out["sigma_1_small"] = R.random_case(1, 1, 5, 7) + (1.0, 0.05, 0.1)
    out["one_row"] = (_blobs(1, 40), np.ones((1, 1, 1, 40), F32), 1.0, 0.1, 0.2)
    return out


CASES = cases()
_expected = {}


def expected(name):
    """(edges, smoothed, classes) [b,1,h,w] of a case by the restatement: computed once, shared, never written"""
    if name not in _expected:
        gray, mask, sigma, lo, hi = CASES[name]
        wts = R.host_weights(sigma)[1]
        parts = [R.canny_restated(gray[i, 0], mask[i, 0], wts, lo, hi, parts=True) for i in range(gray.shape[0])]
        _expected[name] = tuple(np.stack([p[k] for p in parts])[:, None] for k in range(3))
        for a in _expected[name]:
            a.setflags(write=False)
    return _expected[name]


# ---------------------------------------------------------------- CPU: the restatement and its witness

def test_host_weights_are_the_ones_the_package_hands_the_kernel(built):
    from mpiflow_amd import ops
    for sigma in (2.0, 1.0, 0.3, 3.9):
        r, w = ops.canny_weights(sigma)
        rr, ww = R.host_weights(sigma)
        assert r == rr == int(4 * sigma + 0.5) and len(w) == 2 * r + 1
        assert same(np.array(w, F32), ww) and abs(float(np.sum(ww, dtype=np.float64)) - 1) < 1e-6
    assert R.host_weights(2.0)[0] == 8


@pytest.mark.parametrize("seed,b,h,w", R.RANDOM_CASES)
def test_restatement_agrees_with_the_float64_scipy_witness_on_every_pixel(seed, b, h, w):
    gray, mask = R.random_case(seed, b, h, w)
    edges = expected("random_%dx%dx%d" % (b, h, w))[0]
    for i in range(b):
        wit = R.canny_witness(gray[i, 0], mask[i, 0], 2.0, 0.1, 0.2)
        assert int((wit != (edges[i, 0] != 0)).sum()) == 0
    assert h * w < 100 or edges.sum() > 0                     # the case has edges to disagree on


def test_restatement_and_witness_agree_at_other_parameters():
    for name in ("sigma_1", "thresholds", "hole_touching_border"):
        gray, mask, sigma, lo, hi = CASES[name]
        edges = expected(name)[0]
        for i in range(gray.shape[0]):
            assert ((R.canny_witness(gray[i, 0], mask[i, 0], sigma, lo, hi)) == (edges[i, 0] != 0)).all(), name


def test_restated_special_cases_are_what_the_definition_says():
    assert expected("mask_zeros")[0].sum() == 0 and np.isfinite(expected("mask_zeros")[1]).all()
    assert expected("constant")[2].sum() == 0 and expected("constant")[0].sum() == 0
    e = expected("axis_step")[0][0, 0]
    assert e[1:-1, 8:10].sum() >= 15 and e[:, :7].sum() == 0 and e[0].sum() == 0 and e[-1].sum() == 0      # a vertical line, off the border ring
    assert expected("ramp_45")[0].sum() > 0 and expected("ramp_135")[0].sum() > 0
    em = expected("maximum_on_border")
    assert em[0][0, 0, 0].sum() == 0 and em[0][0, 0, :, -1].sum() == 0 and em[2][0, 0, 0].sum() == 0
    cut = expected("mask_edge_through_gradient")[2][0, 0]
    assert cut[:, 9:].sum() == 0                               # columns 9.. lie within one pixel of the outside: eroded


def test_refusals_name_the_argument(built):
    import torch
    from mpiflow_amd import ops
    from mpiflow_amd._lib import MpiFlowHipError
    g, m = torch.zeros(2, 1, 9, 11), torch.ones(2, 1, 9, 11)
    bad = [
        (dict(gray=g.double()), "gray must be float32"),
        (dict(gray=torch.zeros(2, 1, 9, 22)[..., ::2]), "gray must be contiguous"),
        (dict(gray=torch.zeros(2, 9, 11)), "gray must be"),
        (dict(mask=torch.ones(2, 1, 9, 12)), "mask must be"),
        (dict(mask=m.bool()), "mask must be float32"),
        (dict(sigma=0.0), "sigma"),
        (dict(sigma=-1.0), "sigma"),
        (dict(sigma=float("nan")), "sigma"),
        (dict(sigma=4.2), "radius"),
        (dict(low_threshold=0.3, high_threshold=0.2), "low_threshold"),
        (dict(low_threshold=float("nan")), "low_threshold"),
        (dict(out=torch.zeros(2, 1, 9, 12)), "out must be"),
        (dict(workspace=torch.zeros(10)), "workspace holds"),
        (dict(passes="classify"), "workspace"),
        (dict(passes="nms"), "passes"),
        (dict(), "gray must live on the GPU"),
    ]
    for kw, text in bad:
        args = dict(gray=g, mask=m)
        args.update(kw)
        with pytest.raises(MpiFlowHipError, match=text):
            ops.canny_masked(**args)
    assert ops.canny_weights(4.1)[0] == 16                     # the largest radius the kernel holds


def test_c_abi_refuses_before_launching(built):
    import ctypes
    lib = built.load()
    a = built.MpfCannyArgs()
    assert lib.mpf_canny(None, None) != 0 and lib.mpf_canny(ctypes.byref(a), None) != 0
    assert lib.mpf_canny_workspace(0, 4, 4) == 0 and lib.mpf_canny_workspace(1, 1 << 15, 1 << 14) == 0
    assert lib.mpf_canny_workspace(2, 33, 70) == 2 * 33 * 70 * 4 + 2 * 33 * 70 + 2 * 2 * 33 * 3 * 4
    a.B, a.h, a.w, a.radius = 1, 4, 4, 17
    assert lib.mpf_canny(ctypes.byref(a), None) != 0 and b"radius" in lib.mpf_last_error()
    s = built.MpfStage2Args()
    for fn in (lib.mpf_stage2_gray_hole, lib.mpf_stage2_edge_input, lib.mpf_stage2_gen_inputs, lib.mpf_stage2_merge):
        assert fn(None, None) != 0 and fn(ctypes.byref(s), None) != 0


# ---------------------------------------------------------------- GPU: the kernel against the restatement

def _run(dev, name, **kw):
    import torch
    from mpiflow_amd import ops
    gray, mask, sigma, lo, hi = CASES[name]
    return ops.canny_masked(torch.from_numpy(gray).to(dev), torch.from_numpy(mask).to(dev), sigma, lo, hi, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_canny_equals_the_restatement_on_every_pixel_and_stage_by_stage(built, dev, name):
    from mpiflow_amd import ops
    gray = CASES[name][0]
    b, _, h, w = gray.shape
    edges, smoothed, classes = expected(name)
    out = _run(dev, name).cpu().numpy()
    print(name, "edges", int(edges.sum()), "differing pixels", int((out != edges).sum()))
    assert out.dtype == F32 and same(out, edges)
    ws = ops.canny_workspace(b, h, w, dev)
    ws.fill_(float("nan"))
    sm = _run(dev, name, workspace=ws, passes="smooth")
    assert same(sm.cpu().numpy(), smoothed)
    cl = _run(dev, name, workspace=ws, passes="classify")
    assert (cl.cpu().numpy() == classes).all()
    out3 = _run(dev, name, workspace=ws, passes="hysteresis").cpu().numpy()
    assert same(out3, edges)


def _classify_alone(dev, smoothed, mask, lo, hi):
    import torch
    from mpiflow_amd import ops
    h, w = smoothed.shape
    ws = ops.canny_workspace(1, h, w, dev)
    ops.canny_workspace_views(ws, 1, h, w)[0].copy_(torch.from_numpy(smoothed).to(dev)[None, None])
    m = torch.from_numpy(mask).to(dev)[None, None]
    return ops.canny_masked(torch.zeros_like(m), m, 1.0, lo, hi, workspace=ws, passes="classify").cpu().numpy()[0, 0]


@pytest.mark.gpu
def test_classes_on_exact_gradients_zero_component_equal_components_and_border_maximum(built, dev):
    """smoothed maps handed to stage 2 alone, whose Sobel responses are exact: one component 0, |isobel| = |jsobel|, a maximum on the ring"""
    h, w = 19, 70
    yy, xx = np.mgrid[0:h, 0:w]
    bump = lambda t: (np.clip(t, 0, 6) ** 2 * 0.125).astype(F32)          # small dyadic values: every difference exact  # noqa: E731
    ones = np.ones((h, w), F32)
    maps = {"columns": bump(xx - 30), "rows": bump(yy - 6), "diagonal": bump(xx + yy - 40), "antidiagonal": bump(xx - yy - 20),
            "last_column": np.where(xx == w - 1, 3.0, np.where(xx == w - 2, -1.0, 0.0)).astype(F32),
            "row_0": np.where(yy == 0, 3.0, np.where(yy == 1, -1.0, 0.0)).astype(F32),
            "flat": np.zeros((h, w), F32), "diagonal_ramp": ((xx + yy) * 0.25).astype(F32)}
    for name, s in maps.items():
        want = R.restated_classes(s, ones, 0.1, 0.6)
        got = _classify_alone(dev, s, ones, 0.1, 0.6)
        assert (got == want).all(), name
        if name in ("columns", "rows", "diagonal", "antidiagonal", "diagonal_ramp"):
            assert want.max() == 2, name
        if name in ("last_column", "row_0", "flat"):
            assert want.sum() == 0, name                                  # the largest magnitude lies on the ring, which is skipped, and suppresses its neighbours
    hole = ones.copy()
    hole[8, 36] = 0
    assert (_classify_alone(dev, maps["diagonal"], hole, 0.1, 0.6) == R.restated_classes(maps["diagonal"], hole, 0.1, 0.6)).all()


def _serpentine(h, w):
    """a one-pixel-wide weak path over every other row, joined at alternating ends, its only strong pixel at the far end"""
    c = np.zeros((h, w), np.uint8)
    for y in range(0, h, 2):
        c[y, :] = 1
        if y + 1 < h:
            c[y + 1, w - 1 if (y // 2) % 2 == 0 else 0] = 1
    last = h - 1 if (h - 1) % 2 == 0 else h - 2
    c[last, 0 if (last // 2) % 2 == 0 else w - 1] = 2
    return c


def hysteresis_maps():
    h, w = 33, 70
    out = {"serpentine": _serpentine(h, w)}
    d = np.zeros((h, w), np.uint8)
    for k in range(33):
        d[k, k] = 1                                                       # diagonal steps only, down to (32, 32), through the word seam at column 32
        d[32 - k, 32 + k] = 1                                             # and up the other diagonal to (0, 64), through the seam at column 64
    d[0, 0] = 2
    out["diagonal_steps"] = d
    ring = np.zeros((h, w), np.uint8)
    ring[5, 5:40] = ring[25, 5:40] = 1
    ring[5:26, 5] = ring[5:26, 39] = 1
    out["weak_ring_without_strong"] = ring
    two = np.zeros((h, w), np.uint8)
    two[10, 3:31] = 1
    two[10, 3] = 2
    two[10, 32:66] = 1                                                    # one empty pixel (column 31) apart, and no strong pixel
    two[12, 0:70] = 1                                                     # one empty row apart
    out["two_components_one_pixel_apart"] = two
    rng = np.random.RandomState(7)
    out["random_classes"] = rng.choice(np.array([0, 0, 0, 1, 1, 2], np.uint8), size=(h, w), p=None)
    out["all_strong"] = np.full((h, w), 2, np.uint8)
    out["garbage_bytes_count_as_zero"] = rng.randint(0, 256, size=(h, w)).astype(np.uint8)
    return out


def _hysteresis_by_labels(cls):
    """restated_hysteresis by connected components (scipy), for maps on which growing ring by ring takes thousands of rounds"""
    import scipy.ndimage as ndi
    labels, count = ndi.label(cls > 0, np.ones((3, 3), bool))
    good = np.zeros(count + 1, bool)
    good[np.unique(labels[cls == 2])] = True
    good[0] = False
    return good[labels].astype(F32)


def _hysteresis_alone(dev, cls):
    import torch
    from mpiflow_amd import ops
    b, h, w = cls.shape
    ws = ops.canny_workspace(b, h, w, dev)
    ops.canny_workspace_views(ws, b, h, w)[1].copy_(torch.from_numpy(cls).to(dev)[:, None])
    z = torch.zeros((b, 1, h, w), device=dev)
    return ops.canny_masked(z, z, workspace=ws, passes="hysteresis").cpu().numpy()[:, 0]


@pytest.mark.gpu
def test_hysteresis_alone_on_hand_made_class_maps(built, dev):
    maps = hysteresis_maps()
    names = sorted(maps)
    got = _hysteresis_alone(dev, np.stack([maps[n] for n in names]))      # one launch, one workgroup per map
    for i, n in enumerate(names):
        clean = np.where(maps[n] <= 2, maps[n], 0)
        assert same(got[i], _hysteresis_by_labels(clean)), n
        assert n == "serpentine" or same(R.restated_hysteresis(clean), _hysteresis_by_labels(clean)), n
    on = dict(zip(names, got))
    s = maps["serpentine"]
    assert (s > 0).sum() > 33 * 70 // 2 and (on["serpentine"] == (s > 0)).all()          # the sweep-count worst case: fully on
    assert on["weak_ring_without_strong"].sum() == 0
    assert (on["diagonal_steps"] == (maps["diagonal_steps"] > 0)).all()
    t = on["two_components_one_pixel_apart"]
    assert t[10, 3:31].all() and t[10, 32:].sum() == 0 and t[12].sum() == 0


@pytest.mark.gpu
def test_hysteresis_past_the_lds_capacity_sweeps_in_the_workspace(built, dev):
    h, w = 100, 2017                                                      # 100 * 64 words per plane: over MPF_CANNY_LDS_WORDS
    assert h * ((w + 31) // 32) > built.CANNY_LDS_WORDS
    rng = np.random.RandomState(11)
    cls = np.zeros((h, w), np.uint8)
    cls[rng.rand(h, w) < 0.3] = 1
    cls[rng.rand(h, w) < 0.01] = 2
    cls[40:60, :] = 0
    cls[50, :] = 1                                                        # a weak line across every word of a row, lit from its end
    cls[50, w - 1] = 2
    got = _hysteresis_alone(dev, cls[None])[0]
    assert same(got, _hysteresis_by_labels(cls)) and got[50].all()


@pytest.mark.gpu
def test_two_runs_give_identical_bytes(built, dev):
    a = _run(dev, "random_2x33x70").cpu().numpy()
    b = _run(dev, "random_2x33x70").cpu().numpy()
    assert a.tobytes() == b.tobytes() and a.sum() > 0


@pytest.mark.gpu
def test_out_and_workspace_are_used_and_nothing_synchronises(built, dev):
    import torch
    from mpiflow_amd import ops
    gray, mask, sigma, lo, hi = CASES["random_2x33x70"]
    g, m = torch.from_numpy(gray).to(dev), torch.from_numpy(mask).to(dev)
    out = torch.full_like(g, 7.0)
    ws = ops.canny_workspace(2, 33, 70, dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        r = ops.canny_masked(g, m, sigma, lo, hi, out=out, workspace=ws)
    s.synchronize()
    assert r is out and same(out.cpu().numpy(), expected("random_2x33x70")[0])
    assert same(ops.canny_workspace_views(ws, 2, 33, 70)[0].cpu().numpy(), expected("random_2x33x70")[1])
    with pytest.raises(built.MpiFlowHipError, match="overlap"):
        ops.canny_masked(g, m, out=g)
