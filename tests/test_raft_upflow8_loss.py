"""The small RAFT model's sequence loss, fused (mpf_upflow8_loss_term / _backward of mpf_upsample.hip; raft_upsample.flow_loss_term and
sequence_loss with None in place of the mask(s); RAFT.forward(coarse="flow")).

The reference is the reference's own upflow8 followed by train.sequence_loss, recorded on the CPU by tests/golden/make_upflow8_loss_golden.py
into tests/golden/raft_upflow8_loss.npz: fp32 and double runs, err32 = max |fp32 run - double run| per array.  Every grad_flow is stored as
600 sampled entries, so it is compared twice: at the samples against the recorded double run and at EVERY entry against restated() below in
float64 (UP8-style matrices, none of the reference's code), which the host test ties to the samples at 1e-12.  The recorded flow_gt keeps
every |prediction - flow_gt| >= 1e-2 and every threshold quantity clear of its threshold, so no entry is left out of any comparison; the
host test re-asserts both conditions from restated().  A missing golden fails these tests; it does not skip them.

Bars.  Scalars (terms, loss, epe mean): relative, 3 x the largest relative err32 over the case's recorded terms - the rule of
tests/test_raft_upsample.py.  Counts: exact.  grad_flow, per array: the larger of 3 x its recorded err32 and the worst-case bound that
tests/test_raft_model.py derives for upflow8's backward pass, restated here (up8_backward_bar): the kernel rounds the scale once and the
product once, src <= n-1, so a coordinate is good to 2 u (n-1), u = 2^-24; with 1 - l and the factor 8 a tap's coefficient is good to
e = 8 u (2 (H-1) + 2 (W-1) + 6); a coarse pixel is read by at most Ky * Kx fine pixels, K = min(8n, floor(2 (8n-1)/(n-1)) + 1) (8 for n = 1);
the sums are fp64, so nothing else adds: bar = Ky Kx e max |cot|, cot = gamma^(n-1-i) / (N*2*8H*8W) * v * sign(pred - flow_gt) the loss's
cotangent with its gamma weight.  (The cotangent's own roundings - the weight in fp32, one division - are 2 u of it on a total tap weight of
8 * 64: 1024 u |cot|, under a twelfth of the bar's smallest value, 289 * 48 u |cot| in the interior.)

The model test reuses the recorded small/train_2x136x128 case of tests/golden/raft_model.npz and the helpers of tests/test_raft_model.py."""
import argparse
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "raft_upflow8_loss.npz")
SYMBOLS = ("mpf_upflow8_loss_term", "mpf_upflow8_loss_term_backward", "mpf_upflow8_loss_workspace")
U = 2.0 ** -24


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ the statement, in float64 (not code under test)


def up8_matrix(n):
    """[8n, n] float64: the weights with which fine index I reads the coarse ones, align_corners=True: src = I * (n-1)/(8n-1)"""
    A = np.zeros((8 * n, n))
    for I in range(8 * n):
        src = I * (n - 1) / (8 * n - 1) if n > 1 else 0.0
        i0 = min(int(np.floor(src)), n - 1)
        i1 = min(i0 + 1, n - 1)
        A[I, i0] += 1.0 - (src - i0)
        A[I, i1] += src - i0
    return A


def UP8(flow64):
    Ay, Ax = up8_matrix(flow64.shape[2]), up8_matrix(flow64.shape[3])
    return 8.0 * (Ay @ flow64 @ Ax.T)                                   # [8H,H] @ [N,2,H,W] @ [W,8W]


def UP8T(g64):
    Ay, Ax = up8_matrix(g64.shape[2] // 8), up8_matrix(g64.shape[3] // 8)
    return 8.0 * (Ay.T @ g64 @ Ax)                                       # the adjoint


def up8_backward_bar(H, W, cot_max):
    e = 8 * U * (2 * (H - 1) + 2 * (W - 1) + 6)
    K = lambda n: 8 if n == 1 else min(8 * n, (2 * (8 * n - 1)) // (n - 1) + 1)
    return K(H) * K(W) * e * cot_max


def validity(gt, valid, max_flow):
    return (valid >= 0.5) & (np.sqrt(gt[:, 0] ** 2 + gt[:, 1] ** 2) < max_flow)


def restated(flows, gt, valid, gamma, max_flow):
    """the loss of the issue on float64 copies of the inputs: dict of loss, terms, acc (five accumulators of the last prediction), per
    iteration grad_flow_i and the largest cotangent cot_i, and the quantities of the two no-tie conditions"""
    gt, valid = gt.astype(np.float64), valid.astype(np.float64)
    v = validity(gt, valid, max_flow)
    n, count = len(flows), gt.size
    res = dict(terms=np.zeros(n), loss=0.0, min_diff=np.inf)
    for i, f in enumerate(flows):
        pred = UP8(f.astype(np.float64))
        diff = pred - gt
        res["terms"][i] = (v[:, None] * np.abs(diff)).sum() / count
        weight = gamma ** (n - 1 - i)
        res["loss"] += weight * res["terms"][i]
        res["grad_flow_%d" % i] = UP8T(weight / count * v[:, None] * np.sign(diff))
        res["cot_%d" % i] = weight / count
        res["min_diff"] = min(res["min_diff"], float(np.abs(diff).min()))            # over ALL entries: none is left out
    epe = np.sqrt((diff ** 2).sum(axis=1))
    res["epe"] = epe
    res["acc"] = [float(epe[v].sum()), int((epe[v] < 1).sum()), int((epe[v] < 3).sum()), int((epe[v] < 5).sum()), int(v.sum())]
    return res


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN, allow_pickle=False)                  # a missing file is an error here, not a skip
    mk = _load("make_upflow8_loss_golden", "tests", "golden", "make_upflow8_loss_golden.py")
    cases = {}
    for name in [str(n) for n in z["names"]]:
        N, H, W, iters, seed = [int(v) for v in z[name + "/settings"]]
        flows, gt0, valid = mk.case_inputs(N, H, W, iters, seed)
        gt = mk.apply_fixes(gt0, z[name + "/gt_fix_idx"], z[name + "/gt_fix_val"])
        sums = [sum(f.astype(np.float64).sum() for f in flows), gt.astype(np.float64).sum(), valid.astype(np.float64).sum()]
        assert np.array_equal(np.array(sums), z[name + "/input_sums"]), "the seeded inputs of %s are not the recorded ones" % name
        c = dict(name=name, N=N, H=H, W=W, iters=iters, flows=flows, gt=gt, valid=valid, gamma=float(z["gamma"]), max_flow=float(z["max_flow"]),
                 tie=float(z["tie_margin"]), epe_margin=float(z["epe_margin"]))
        for key in ("loss", "terms", "metrics", "acc"):
            c[key] = dict(f32=z["%s/%s_f32" % (name, key)], f64=z["%s/%s_f64" % (name, key)])
        for i in range(iters):
            key = "grad_flow_%d" % i
            c[key] = dict(idx=mk.sample_index(N * 2 * H * W, seed), f32=z["%s/%s_f32" % (name, key)], f64=z["%s/%s_f64" % (name, key)],
                          err32=float(z["%s/%s_err32" % (name, key)]), absmax=float(z["%s/%s_absmax" % (name, key)]))
        t = c["terms"]
        c["rel_bar"] = 3 * float((np.abs(t["f32"] - t["f64"]) / np.abs(t["f64"])).max())
        c["want"] = restated(flows, gt, valid, c["gamma"], c["max_flow"])            # computed once, shared, left unchanged
        cases[name] = c
    assert [(c["N"], c["H"], c["W"], c["iters"]) for c in cases.values()] == [(1, 1, 1, 2), (2, 1, 9, 2), (2, 5, 1, 2), (1, 5, 7, 3), (1, 13, 83, 3), (2, 36, 120, 4)]
    return cases


# ---------------------------------------------------------------------------------------------------------------- host


def test_symbols_are_declared_bound_and_exported(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read(), flags=re.S)
    for path in (built.LIB_PATH, built.WITNESS_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        lib = ctypes.CDLL(path)
        for name in SYMBOLS:
            assert name in built.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name), (path, name)
            assert re.search(r"\b%s\b" % name, syms), (path, name)
        assert "k_up8_loss" in syms and "k_up8_loss_bwd" in syms, path


def _args(built, **kw):
    a = built.MpfUpsampleArgs()
    for k in ("flow", "flow_gt", "valid", "g", "term", "metrics", "grad_flow", "workspace"):
        setattr(a, k, 256)
    a.workspace_bytes, a.N, a.H, a.W, a.max_flow = 1 << 30, 2, 36, 120, 400.0        # mask, out, grad_mask stay NULL: ignored
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_c_abi_refuses_bad_arguments(built):
    """validated before anything is launched: no GPU is needed to be told so.  Status 10001 and a message that names the argument."""
    lib = built.load()
    fns = dict(loss=lib.mpf_upflow8_loss_term, lbwd=lib.mpf_upflow8_loss_term_backward)
    common = [(dict(flow=None), b"(flow)"), (dict(flow_gt=None), b"flow_gt"), (dict(valid=None), b"valid"), (dict(N=0), b"bad shape"), (dict(H=0), b"bad shape"),
              (dict(W=-3), b"bad shape"), (dict(N=1 << 12, H=1 << 10, W=1 << 10), b"2^31"), (dict(N=1, H=1 << 16, W=1 << 16), b"2^31"),
              (dict(N=2, H=2048, W=4096), b"2^31"), (dict(flow_gt=264), b"16-byte aligned"), (dict(valid=260), b"16-byte aligned")]
    blocks = (2 * 36 * 120 * 16 + 255) // 256
    only = dict(loss=[(dict(term=None), b"term"), (dict(workspace=None), b"workspace"), (dict(workspace_bytes=blocks * 48 - 1), b"workspace"),
                      (dict(workspace=260), b"8-byte")],
                lbwd=[(dict(g=None), b"(g)"), (dict(grad_flow=None), b"grad_flow")])
    for name, fn in fns.items():
        assert fn(None, None) == 10001 and b"null argument block" in lib.mpf_last_error()
        for kw, word in common + only[name]:
            assert fn(ctypes.byref(_args(built, **kw)), None) == 10001, (name, kw)
            assert word in lib.mpf_last_error() and name_of(fn) in lib.mpf_last_error(), (name, kw, lib.mpf_last_error())
    assert blocks == 540 and lib.mpf_upflow8_loss_workspace(2, 36, 120, 0) == blocks * 6 * 8 and lib.mpf_upflow8_loss_workspace(2, 36, 120, 1) == 0
    assert lib.mpf_upflow8_loss_workspace(8, 36, 120, 0) == 2160 * 6 * 8 and lib.mpf_upflow8_loss_workspace(32, 64, 64, 0) == 4096 * 6 * 8   # grid-stride beyond
    assert lib.mpf_upflow8_loss_workspace(1, 1, 1, 0) == 48
    assert lib.mpf_upflow8_loss_workspace(0, 36, 120, 0) == 0 and lib.mpf_upflow8_loss_workspace(1, 1 << 16, 1 << 16, 0) == 0
    assert lib.mpf_upflow8_loss_workspace(2, 2048, 4096, 0) == 0 and lib.mpf_upflow8_loss_workspace(1, 2048, 4096, 0) > 0


def name_of(fn):
    return fn.__name__.encode()


def test_public_functions_refuse_what_they_cannot_take(built):
    from mpiflow_amd import ops
    from mpiflow_amd import raft_upsample as ru
    E = built.MpiFlowHipError
    f = torch.zeros(1, 2, 4, 6)
    gt, va, g = torch.zeros(1, 2, 32, 48), torch.zeros(1, 32, 48), torch.ones(())
    with pytest.raises(E, match="no CPU path"):
        ru.flow_loss_term(f, None, gt, va)
    with pytest.raises(E, match="no CPU path"):
        ru.sequence_loss([f, f], None, gt, va)
    with pytest.raises(E, match="flow must live on the GPU.*no CPU path"):
        ops.upflow8_loss_term(f, gt, va, 400)
    with pytest.raises(E, match="flow must live on the GPU.*no CPU path"):
        ops.upflow8_loss_term_backward(f, gt, va, g, 400)
    for bad in (torch.float16, torch.bfloat16):
        with pytest.raises(E, match=r"flow must be float32.*\.float\(\)"):
            ru.flow_loss_term(f.to(bad), None, gt, va)
        with pytest.raises(E, match=r"flow must be float32.*\.float\(\)"):
            ru.sequence_loss([f.to(bad)], None, gt, va)
    with pytest.raises(E, match="flow must be a torch.Tensor"):
        ru.flow_loss_term(f.numpy(), None, gt, va)
    with pytest.raises(E, match="flow must be"):
        ru.flow_loss_term(torch.zeros(1, 3, 4, 6), None, gt, va)
    for wrong in (torch.zeros(1, 2, 32, 40), torch.zeros(2, 2, 32, 48), torch.zeros(1, 2, 4, 6), torch.zeros(2, 32, 48)):
        with pytest.raises(E, match="flow_gt must be"):
            ru.flow_loss_term(f, None, wrong, va)
    for wrong in (torch.zeros(1, 1, 32, 48), torch.zeros(1, 32, 40), torch.zeros(1, 4, 6)):
        with pytest.raises(E, match="valid must be"):
            ru.flow_loss_term(f, None, gt, wrong)
    with pytest.raises(E, match="valid must be"):
        ops.upflow8_loss_term_backward(f, gt, torch.zeros(1, 32, 40), g)
    with pytest.raises(E, match="flow must be contiguous"):
        ru.flow_loss_term(torch.zeros(1, 2, 6, 4).transpose(2, 3), None, gt, va)
    with pytest.raises(E, match="g must be"):
        ops.upflow8_loss_term_backward(f, gt, va, torch.ones(1))
    # the order of the contract: a wrong dtype before a wrong shape, both before the device
    with pytest.raises(E, match="flow_gt must be float32"):
        ru.flow_loss_term(f, None, torch.zeros(1, 2, 32, 40, dtype=torch.float64), va)
    with pytest.raises(E, match="as many masks as flows"):
        ru.sequence_loss([], None, gt, va)
    with pytest.raises(E, match="as many masks as flows"):
        ru.sequence_loss([f, f], [torch.zeros(1, 576, 4, 6)], gt, va)
    with pytest.raises(E, match="mask must be a torch.Tensor"):          # a None INSIDE a list of masks is what it was: a missing mask
        ru.sequence_loss([f], [None], gt, va)


def test_coarse_flow_is_the_small_models_and_other_values_are_refused(built):
    from mpiflow_amd import raft
    E = built.MpiFlowHipError
    basic = raft.RAFT(argparse.Namespace(small=False, mixed_precision=False))
    small = raft.RAFT(argparse.Namespace(small=True, mixed_precision=False))
    ok = torch.zeros(1, 3, 128, 136)
    with pytest.raises(E, match=r'coarse=True needs the basic model.*coarse="flow"'):
        small(ok, ok, coarse=True)
    with pytest.raises(E, match=r'coarse="flow" is the small model\'s.*coarse=True'):
        basic(ok, ok, coarse="flow")
    with pytest.raises(E, match=r'coarse="flow".*test_mode'):
        small(ok, ok, coarse="flow", test_mode=True)
    with pytest.raises(E, match="coarse=True.*test_mode"):
        basic(ok, ok, coarse=True, test_mode=True)
    for model in (basic, small):
        for bad in ("mask", "Flow", 1, 0, None, 2.0, ("flow",)):
            with pytest.raises(E, match="coarse must be False, True or \"flow\""):
                model(ok, ok, coarse=bad)
        # the tensors' own faults are named first, the device last
        with pytest.raises(E, match="image2 must be float32"):
            model(ok, ok.half(), coarse="flow")
    with pytest.raises(E, match="image1 must live on the GPU"):
        small(ok, ok, coarse="flow")
    with pytest.raises(E, match="image1 must live on the GPU"):
        small(ok, ok, coarse=False)


def test_restatement_equals_the_recorded_reference_and_no_entry_ties(golden):
    """restated() in float64 == the reference on double inputs: the sampled entries of every grad_flow to 1e-12 of the array's largest entry,
    the scalars to 1e-12 relative, the counts exactly.  Both no-tie conditions hold on EVERY entry (the cap on entries left out is zero)."""
    for c in golden.values():
        w = c["want"]
        for i in range(c["iters"]):
            s = c["grad_flow_%d" % i]
            full = w["grad_flow_%d" % i]
            assert full.shape == (c["N"], 2, c["H"], c["W"])
            d = np.abs(full.reshape(-1)[s["idx"]] - s["f64"]).max()
            assert d <= 1e-12 * s["absmax"], (c["name"], i, d, s["absmax"])
            assert abs(np.abs(full).max() - s["absmax"]) <= 1e-12 * s["absmax"]
            assert np.abs(s["f32"].astype(np.float64) - s["f64"]).max() <= s["err32"]
        assert np.abs(w["terms"] - c["terms"]["f64"]).max() <= 1e-12 * np.abs(c["terms"]["f64"]).max()
        assert abs(w["loss"] - float(c["loss"]["f64"])) <= 1e-12 * abs(float(c["loss"]["f64"]))
        acc = c["acc"]["f64"]
        assert w["acc"][1:] == [int(v) for v in acc[1:]] == [int(v) for v in c["acc"]["f32"][1:]]
        assert abs(w["acc"][0] - acc[0]) <= 1e-12 * acc[0]
        assert np.allclose(c["metrics"]["f64"], [acc[0] / acc[4], acc[1] / acc[4], acc[2] / acc[4], acc[3] / acc[4]], rtol=1e-6, atol=0)
        assert c["rel_bar"] > 0.0
        # the conditions on the inputs, from this file's own statement, on every entry
        assert w["min_diff"] >= c["tie"], (c["name"], w["min_diff"])
        mag = np.sqrt((c["gt"].astype(np.float64) ** 2).sum(axis=1))
        assert float(np.abs(mag - c["max_flow"]).min()) >= 1.0 and bool((mag > c["max_flow"]).any())
        for thr in (1.0, 3.0, 5.0):
            assert float(np.abs(w["epe"] - thr).min()) >= c["epe_margin"]
        assert 0 < w["acc"][1] < w["acc"][2] < w["acc"][3] < w["acc"][4] < mag.size
        print("%-16s rel bar of the scalars %.2e; smallest |pred64 - gt| %.3e" % (c["name"], c["rel_bar"], w["min_diff"]))


# ----------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ru(built):
    from mpiflow_amd import raft_upsample
    return raft_upsample


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(-1).view(torch.int32), b.contiguous().view(-1).view(torch.int32))


def tensors(c, dev, grad=False):
    t = lambda a: torch.from_numpy(a).to(dev)
    return [t(f).requires_grad_(grad) for f in c["flows"]], t(c["gt"]), t(c["valid"])


def check_rel(c, what, got, want):
    rel = abs(got - want) / abs(want)
    print("%-10s %-16s rel err %.2e = %.2f of the bar %.2e" % (what, c["name"], rel, rel / c["rel_bar"], c["rel_bar"]))
    assert rel <= c["rel_bar"], (c["name"], what, got, want, rel, c["rel_bar"])


def run_case(c, ru, dev):
    from mpiflow_amd import ops
    fl, gt, va = tensors(c, dev, grad=True)
    terms = [ru.flow_loss_term(f.detach(), None, gt, va, c["max_flow"]) for f in fl]
    loss, metrics = ru.sequence_loss(fl, None, gt, va, gamma=c["gamma"], max_flow=c["max_flow"])
    _, acc = ops.upflow8_loss_term(fl[-1].detach(), gt, va, c["max_flow"], metrics=True)
    loss.backward()
    return dict(terms=terms, loss=loss.detach(), metrics=metrics, acc=acc, grads=[f.grad for f in fl])


CASE_NAMES = ["one_1x1x1", "h1_2x1x9", "w1_2x5x1", "tiny_1x5x7", "mid_1x13x83", "real_2x36x120"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_loss_and_gradients_match_the_recorded_reference(name, golden, ru, dev):
    c = golden[name]
    w = c["want"]
    a, b = run_case(c, ru, dev), run_case(c, ru, dev)
    for x, y in zip(a["terms"] + [a["loss"], a["acc"]] + a["grads"], b["terms"] + [b["loss"], b["acc"]] + b["grads"]):
        assert same_bytes(x, y) if x.dtype == torch.float32 else torch.equal(x, y)
    assert a["metrics"] == b["metrics"]
    for i, term in enumerate(a["terms"]):
        assert term.dim() == 0 and term.is_cuda and term.dtype == torch.float32
        check_rel(c, "term %d" % i, float(term), float(c["terms"]["f64"][i]))
    loss, metrics = a["loss"], a["metrics"]
    assert loss.dim() == 0 and loss.is_cuda and sorted(metrics) == ["1px", "3px", "5px", "epe"] and all(type(v) is float for v in metrics.values())
    check_rel(c, "loss", float(loss), float(c["loss"]["f64"]))
    acc = c["acc"]["f64"]
    check_rel(c, "epe", metrics["epe"], acc[0] / acc[4])
    got = a["acc"].tolist()
    assert a["acc"].dtype == torch.float64 and [int(v) for v in got[1:]] == [int(v) for v in acc[1:]] == w["acc"][1:], (got, acc)
    for k, q in (("1px", 1), ("3px", 2), ("5px", 3)):
        assert metrics[k] == acc[q] / acc[4]
    for i, grad in enumerate(a["grads"]):
        s = c["grad_flow_%d" % i]
        bar = max(3 * s["err32"], up8_backward_bar(c["H"], c["W"], w["cot_%d" % i]))
        hip = grad.double().cpu().numpy()
        assert hip.shape == (c["N"], 2, c["H"], c["W"]) and grad.dtype == torch.float32
        d_s = float(np.abs(hip.reshape(-1)[s["idx"]] - s["f64"]).max())
        d_f = float(np.abs(hip - w["grad_flow_%d" % i]).max())
        print("loss bwd %-16s grad_flow_%d |hip - ref64| sampled %.2e, every entry vs the statement %.2e = %.3f of the bar %.2e (3 err32 %.2e, absmax %.2e)"
              % (c["name"], i, d_s, d_f, d_f / bar, bar, 3 * s["err32"], s["absmax"]))
        assert d_s <= bar and d_f <= bar, (c["name"], i, d_s, d_f, bar)


@pytest.mark.gpu
def test_gpu_the_prediction_in_registers_is_upflow8s(ru, dev):
    """flow_gt = upflow8(flow) bit for bit: every difference is exactly 0, so the term is exactly 0, epe is 0 on every valid pixel and no
    gradient flows - which holds only if the loss kernels form the prediction with mpf_upflow8's own arithmetic.  Widths and heights around
    the lane's 4 pixels and the group's 32 columns."""
    for N, H, W in ((1, 1, 1), (2, 3, 5), (1, 2, 2), (1, 9, 33)):
        gen = torch.Generator(device="cpu").manual_seed(5 + H * W)
        flow = (3.0 * torch.randn(N, 2, H, W, generator=gen)).to(dev).requires_grad_(True)
        gt = ru.upflow8(flow.detach())
        loss, metrics = ru.sequence_loss([flow], None, gt, torch.ones(N, 8 * H, 8 * W, device=dev))
        loss.backward()
        assert float(loss) == 0.0 and metrics == {"epe": 0.0, "1px": 1.0, "3px": 1.0, "5px": 1.0}, (N, H, W, float(loss), metrics)
        assert not flow.grad.any()


@pytest.mark.gpu
def test_gpu_sign_of_zero_and_masked_entries_give_no_gradient(ru, dev):
    """Per FINE pixel one of four kinds: 0 live, 1 flow_gt = the prediction exactly (sign 0), 2 valid = 0, 3 over max_flow.  Kinds 1-3 add
    exactly 0 to grad_flow: the gradient is the gradient, bit for bit, of the frame in which every such pixel is simply invalid, and it is the
    float64 statement's over the live pixels.  A frame made only of kinds 1-3 has grad_flow == 0 and term == 0; made only of kinds 2-3 (no
    valid pixel at all) its metrics are nan as well."""
    N, H, W = 2, 6, 37
    gen = torch.Generator(device="cpu").manual_seed(11)
    flow = (3.0 * torch.randn(N, 2, H, W, generator=gen)).to(dev)
    pred = ru.upflow8(flow).cpu()
    gt = pred + 2.0 * torch.randn(N, 2, 8 * H, 8 * W, generator=gen) + 0.5
    kind = torch.randint(0, 4, (N, 8 * H, 8 * W), generator=gen)

    def frame(kinds):
        g, v = gt.clone(), torch.ones(N, 8 * H, 8 * W)
        both = lambda m: m[:, None].expand_as(g)
        g[both(kinds == 1)] = pred[both(kinds == 1)]
        v[kinds == 2] = 0.0
        g[:, 0][kinds == 3] = 500.0
        return g.to(dev), v.to(dev)

    def run(kinds):
        g, v = frame(kinds)
        f = flow.clone().requires_grad_(True)
        loss, metrics = ru.sequence_loss([f], None, g, v)
        loss.backward()
        return float(loss), metrics, f.grad

    loss, _, grad = run(kind)
    loss2, _, grad2 = run(torch.where(kind == 0, 0, 2))                  # every dead pixel simply invalid
    assert grad.any() and loss > 0 and same_bytes(grad, grad2) and loss == loss2
    live = (kind == 0).numpy()
    diff = pred.double().numpy() - gt.double().numpy()
    want = UP8T(1.0 / diff.size * live[:, None] * np.sign(diff))
    bar = up8_backward_bar(H, W, 1.0 / diff.size)
    d = float(np.abs(grad.double().cpu().numpy() - want).max())
    print("kinds: |hip - statement| %.2e = %.3f of the bar %.2e" % (d, d / bar, bar))
    assert d <= bar
    dead = torch.where(kind == 0, 1, kind)
    loss, metrics, grad = run(dead)
    assert loss == 0.0 and not grad.any() and metrics["epe"] == 0.0 and metrics["1px"] == 1.0
    loss, metrics, grad = run(torch.where(dead == 1, 3, dead))
    assert loss == 0.0 and not grad.any() and all(np.isnan(v) for v in metrics.values())


@pytest.mark.gpu
def test_gpu_nan_and_inf_travel_as_in_torch(ru, dev):
    """a NaN prediction has sign 0 and poisons the term, as torch's (valid * |diff|).mean() does; an infinite flow_gt is over max_flow and
    masked out of the gradient; nothing stops the run and no other gradient entry changes"""
    N, H, W = 1, 4, 6
    gen = torch.Generator(device="cpu").manual_seed(3)
    flow = torch.randn(N, 2, H, W, generator=gen).to(dev)
    gt = (torch.randn(N, 2, 8 * H, 8 * W, generator=gen) + 20.0).to(dev)
    valid = torch.ones(N, 8 * H, 8 * W, device=dev)
    f = flow.clone().requires_grad_(True)
    ru.flow_loss_term(f, None, gt, valid).backward()
    clean = f.grad
    gt2 = gt.clone()
    gt2[0, 0, 3, 3] = float("inf")
    f = flow.clone().requires_grad_(True)
    term = ru.flow_loss_term(f, None, gt2, valid)
    term.backward()
    assert torch.isnan(term)                                                 # 0 * inf, as in torch
    changed = (f.grad != clean).nonzero()
    assert torch.isfinite(f.grad).all() and 0 < len(changed) <= 8 and int(changed[:, 2].max()) <= 1 and int(changed[:, 3].max()) <= 1
    flow2 = flow.clone()
    flow2[0, 1, 3, 5] = float("nan")
    f = flow2.requires_grad_(True)
    loss, metrics = ru.sequence_loss([f], None, gt, valid)
    loss.backward()
    assert torch.isnan(loss) and torch.isfinite(f.grad).all()
    assert same_bytes(f.grad[:, 0], clean[:, 0]) and same_bytes(f.grad[:, 1, :2], clean[:, 1, :2])


@pytest.mark.gpu
def test_gpu_no_prediction_is_materialised(golden, ru, dev):
    """4 terms at 2 x 36 x 120: forward allocates, beyond what was held before the call, less than ONE full-resolution prediction; so does
    backward (the gradients it returns included)."""
    c = golden["real_2x36x120"]
    fl, gt, va = tensors(c, dev, grad=True)
    ru.sequence_loss([f.detach() for f in fl], None, gt, va)                   # the library is loaded and warm
    one_field = c["N"] * 2 * 64 * c["H"] * c["W"] * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    loss, _ = ru.sequence_loss(fl, None, gt, va, gamma=c["gamma"])
    torch.cuda.synchronize()
    fwd = torch.cuda.max_memory_allocated(dev) - before
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    loss.backward()
    torch.cuda.synchronize()
    bwd = torch.cuda.max_memory_allocated(dev) - before
    print("forward allocates %.3f MB, backward %.3f MB (returned gradients included); one full-resolution prediction %.3f MB" % (fwd / 1e6, bwd / 1e6, one_field / 1e6))
    assert len(fl) == 4 and all(f.grad is not None for f in fl)
    assert fwd < one_field and bwd < one_field


@pytest.mark.gpu
def test_gpu_small_model_coarse_flows_feed_sequence_loss(built, ru, dev):
    """RAFT(small)(..., coarse="flow") -> iters coarse flows; sequence_loss(out, None, ...) against train.py's loss restated in torch (float64
    sums) on the coarse=False predictions, and the parameter gradients of the two calls under the model bar of the same array - what
    test_gpu_coarse_pairs_feed_sequence_loss asks of the basic model."""
    from mpiflow_amd import raft
    tm = _load("test_raft_model_helpers", "tests", "test_raft_model.py")
    mk = _load("make_raft_golden", "tests", "golden", "make_raft_golden.py")
    z = np.load(tm.GOLDEN, allow_pickle=False)
    name = "small/train_2x136x128"
    small, N, H, W, iters, train, seed = [int(v) for v in z[name + "/settings"]]
    d = mk.case_inputs(N, H, W, iters, bool(train), seed)
    c = dict(name=name, small=bool(small), N=N, H=H, W=W, iters=iters, train=bool(train), seed=seed, d=d, sums=z[name + "/input_sums"])
    assert c["small"] and c["train"] and sum(v.astype(np.float64).sum() for v in d.values()) == c["sums"][0]
    c["keys"] = [str(k) for k in z[name + "/keys"]]
    c["rec"] = {k: dict(f64=z["%s/%s_f64" % (name, k)], err32=float(z["%s/%s_err32" % (name, k)]), absmax=float(z["%s/%s_absmax" % (name, k)])) for k in c["keys"]}
    c["zero_grads"] = [str(k) for k in z[name + "/zero_grads"]]
    _, _, table = tm.runs_of(c, raft, dev, mk)
    rs = np.random.RandomState(seed + 3)
    t = lambda a: torch.from_numpy(a).to(dev)
    gt = t((10.0 * rs.standard_normal((N, 2, H, W))).astype(np.float32))
    valid = t((rs.rand(N, H, W) > 0.1).astype(np.float32))
    grads = []
    for coarse in ("flow", False):
        model = tm._prepare(c, raft.RAFT(mk.make_args(True)), dev, mk)
        out = model(t(d["image1"]), t(d["image2"]), iters=iters, coarse=coarse)
        assert isinstance(out, list) and len(out) == iters
        if coarse:
            for flow in out:
                assert isinstance(flow, torch.Tensor) and flow.shape == (N, 2, H // 8, W // 8) and flow.dtype == torch.float32
            loss, metrics = ru.sequence_loss(out, None, gt, valid, gamma=0.8)
            assert sorted(metrics) == ["1px", "3px", "5px", "epe"]
        else:
            assert out[0].shape == (N, 2, H, W)
            loss = tm.sequence_loss_restated(out, gt, valid, gamma=0.8)
        loss.backward()
        grads.append((float(loss), {k: p.grad for k, p in model.named_parameters()}))
    (fused, g_fused), (plain, g_plain) = grads
    rel = abs(fused - plain) / abs(plain)
    print("coarse=\"flow\": loss fused %.9g, restated %.9g, rel %.2e = %.3f of the bar" % (fused, plain, rel, rel / tm.LOSS_REL_BAR))
    top = max(float(g.abs().max()) for g in g_plain.values())
    diffs = {k: float((g_fused[k].double() - g_plain[k].double()).abs().max()) for k in g_fused}
    worst = max((dd / table["grad_" + k][2], k) for k, dd in diffs.items())
    worst_rel = max((dd / top, k) for k, dd in diffs.items())
    print("coarse=\"flow\": parameter gradients, worst %.2e of its bar (%s); worst difference %.2e of the largest gradient %.2e (%s)"
          % (worst[0], worst[1], worst_rel[0], top, worst_rel[1]))
    assert rel <= tm.LOSS_REL_BAR
    for k, dd in diffs.items():
        assert dd <= table["grad_" + k][2], (k, dd, table["grad_" + k])
