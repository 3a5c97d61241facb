"""RAFT's convex upsampling and sequence loss, fused (mpiflow_amd/raft_upsample.py; mpf_upsample_flow / _backward and mpf_flow_loss_term /
_backward of mpf_upsample.hip).

The reference is the reference's own RAFT.upsample_flow and train.sequence_loss, recorded on the CPU by tests/golden/make_upsample_golden.py
into tests/golden/raft_upsample.npz: fp32 and double runs and err32 = max |fp32 run - double run| per array - the yardstick: a kernel result
must stay within 3 * err32 of the DOUBLE run (the bar of tests/test_raft_corr.py).  Large arrays are stored as 600 sampled entries, so each
is compared twice: at the samples against the recorded double run, and at EVERY entry against formula() below in float64, which the host
test ties to the samples at 1e-12.  Scalars (terms, loss, epe mean) are held to a relative error of 3 x the largest relative err32 over the
case's recorded terms.  The recorded flow_gt keeps every |prediction - flow_gt| >= 1e-2 and every threshold quantity clear of its
threshold (the maker's docstring), so no entry is left out of any comparison; the host test re-asserts both conditions from formula().
A missing golden fails these tests; it does not skip them.

Measured on an MI355X (max |hip - ref64| / err32 per case; the bound is 3): see profiles/upsample/README.md."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "raft_upsample.npz")
BIG = ("pred_last", "up_grad_flow", "up_grad_mask")


def _maker():
    spec = importlib.util.spec_from_file_location("make_upsample_golden", os.path.join(ROOT, "tests", "golden", "make_upsample_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN, allow_pickle=False)                  # a missing file is an error here, not a skip
    mk = _maker()
    cases = {}
    for name in [str(n) for n in z["names"]]:
        N, H, W, iters, seed = [int(v) for v in z[name + "/settings"]]
        flows, masks, gt0, valid, cot = mk.case_inputs(N, H, W, iters, seed)
        gt = mk.apply_fixes(gt0, z[name + "/gt_fix_idx"], z[name + "/gt_fix_val"])
        sums = [sum(f.astype(np.float64).sum() for f in flows), sum(m.astype(np.float64).sum() for m in masks),
                gt.astype(np.float64).sum(), valid.astype(np.float64).sum(), cot.astype(np.float64).sum()]
        assert np.array_equal(np.array(sums), z[name + "/input_sums"]), "the seeded inputs of %s are not the recorded ones" % name
        c = dict(name=name, N=N, H=H, W=W, iters=iters, flows=flows, masks=masks, gt=gt, valid=valid, cot=cot,
                 gamma=float(z["gamma"]), max_flow=float(z["max_flow"]), tie=float(z["tie_margin"]), epe_margin=float(z["epe_margin"]))
        for key in ("loss", "terms", "metrics", "acc"):
            c[key] = dict(f32=z["%s/%s_f32" % (name, key)], f64=z["%s/%s_f64" % (name, key)])
        keys = list(BIG) + ["grad_%s_%d" % (w, i) for i in range(iters) for w in ("flow", "mask")]
        for key in keys:
            c[key] = dict(idx=mk.sample_index(int(np.prod(_shape(c, key))), seed), f32=z["%s/%s_f32" % (name, key)], f64=z["%s/%s_f64" % (name, key)],
                          err32=float(z["%s/%s_err32" % (name, key)]), absmax=float(z["%s/%s_absmax" % (name, key)]))
        t = c["terms"]
        c["rel_bar"] = 3 * float((np.abs(t["f32"] - t["f64"]) / np.abs(t["f64"])).max())
        cases[name] = c
    assert len(cases) == 5 and cases["real_2x36x120"]["iters"] == 12
    return cases


def _shape(c, key):
    N, H, W = c["N"], c["H"], c["W"]
    if key == "pred_last":
        return (N, 2, 8 * H, 8 * W)
    return (N, 576, H, W) if "mask" in key else (N, 2, H, W)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


def formula(flow, mask):
    """The op as the issue states it, in the dtype / on the device of its inputs, differentiable:
        p[k,i,j] = softmax over k of mask[n, k*64+i*8+j, h, w];   out[n,c,8h+i,8w+j] = sum_k p[k,i,j] * 8*flow[n,c,h+ky-1,w+kx-1], k = ky*3+kx,
    a neighbour outside the map = 0 (and keeps its weight).  No unfold, no code of the reference."""
    N, _, H, W = flow.shape
    m = mask.reshape(N, 9, 8, 8, H, W)
    e = torch.exp(m - m.max(dim=1, keepdim=True).values)
    p = e / e.sum(dim=1, keepdim=True)
    padded = F.pad(8 * flow, (1, 1, 1, 1))
    out = torch.zeros(N, 2, 8, 8, H, W, dtype=flow.dtype, device=flow.device)
    for k in range(9):
        ky, kx = divmod(k, 3)
        out = out + p[:, k][:, None] * padded[:, :, ky:ky + H, kx:kx + W][:, :, None, None]
    return out.permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * H, 8 * W)          # [N,2,H,i,W,j]


def validity(gt, valid, max_flow):
    return (valid >= 0.5) & (torch.sqrt(gt[:, 0] ** 2 + gt[:, 1] ** 2) < max_flow)


def term_formula(pred, gt, valid, max_flow):
    """S / count of the issue: the mean over ALL entries of v * |pred - gt|"""
    return (validity(gt, valid, max_flow)[:, None] * (pred - gt).abs()).mean()


def loss_formula(flows, masks, gt, valid, gamma, max_flow, up=formula):
    n = len(flows)
    terms = [term_formula(up(f, m), gt, valid, max_flow) for f, m in zip(flows, masks)]
    loss = 0.0
    for i, t in enumerate(terms):
        loss = loss + gamma ** (n - 1 - i) * t
    return loss, terms


def accumulators(pred, gt, valid, max_flow):
    v = validity(gt, valid, max_flow)
    epe = torch.sqrt(((pred - gt) ** 2).sum(dim=1))[v]
    return [float(epe.double().sum()), int((epe < 1).sum()), int((epe < 3).sum()), int((epe < 5).sum()), int(v.sum())]


def tensors(c, dtype, dev="cpu", grad=False):
    t = lambda a: torch.from_numpy(a).to(dtype).to(dev)
    fl, mk = [t(f).requires_grad_(grad) for f in c["flows"]], [t(m).requires_grad_(grad) for m in c["masks"]]
    return fl, mk, t(c["gt"]), t(c["valid"]), t(c["cot"])


def reference_run(c, dtype, dev="cpu"):
    """everything the golden records, from formula(): dict of full arrays and scalars"""
    fl, mk, gt, va, cot = tensors(c, dtype, dev, grad=True)
    loss, terms = loss_formula(fl, mk, gt, va, c["gamma"], c["max_flow"])
    loss.backward()
    res = dict(loss=float(loss.detach()), terms=np.array([float(t.detach()) for t in terms]))
    for i in range(c["iters"]):
        res["grad_flow_%d" % i], res["grad_mask_%d" % i] = fl[i].grad, mk[i].grad
    f, m = fl[-1].detach().clone().requires_grad_(True), mk[-1].detach().clone().requires_grad_(True)
    out = formula(f, m)
    out.backward(cot)
    res["pred_last"], res["up_grad_flow"], res["up_grad_mask"] = out.detach(), f.grad, m.grad
    res["acc"] = accumulators(out.detach(), gt, va, c["max_flow"])
    return res


def big_keys(c):
    return list(BIG) + ["grad_%s_%d" % (w, i) for i in range(c["iters"]) for w in ("flow", "mask")]


# ---------------------------------------------------------------------------------------------------------------- host


def test_formula_equals_the_recorded_reference(golden):
    """formula() in float64 == the reference on double inputs at the sampled entries to 1e-12 of the array's largest entry (prediction and all
    gradients), and its scalars to 1e-12 relative; formula() in float32 is within 3 * err32 of the double run.  The two input conditions hold."""
    for c in golden.values():
        r64, r32 = reference_run(c, torch.float64), reference_run(c, torch.float32)
        for key in big_keys(c):
            s = c[key]
            d64 = np.abs(r64[key].numpy().reshape(-1)[s["idx"]] - s["f64"]).max()
            d32 = np.abs(r32[key].numpy().astype(np.float64).reshape(-1)[s["idx"]] - s["f64"]).max()
            full32 = np.abs(r32[key].numpy().astype(np.float64) - r64[key].numpy()).max()
            assert d64 <= 1e-12 * s["absmax"], (c["name"], key, d64, s["absmax"])
            assert d32 <= 3 * s["err32"] and full32 <= 3 * s["err32"], (c["name"], key, d32, full32, s["err32"])
        assert np.abs(r64["terms"] - c["terms"]["f64"]).max() <= 1e-12 * np.abs(c["terms"]["f64"]).max()
        assert abs(r64["loss"] - float(c["loss"]["f64"])) <= 1e-12 * abs(float(c["loss"]["f64"]))
        assert r64["acc"][1:] == [int(v) for v in c["acc"]["f64"][1:]] == r32["acc"][1:]
        assert abs(r64["acc"][0] - c["acc"]["f64"][0]) <= 1e-12 * c["acc"]["f64"][0]
        # the conditions on the inputs, from this file's own formula
        fl, mk, gt, va, _ = tensors(c, torch.float64)
        v = validity(gt, va, c["max_flow"])
        for f, m in zip(fl, mk):
            assert float((formula(f, m) - gt).abs()[v[:, None].expand(-1, 2, -1, -1)].min()) >= c["tie"]
        mag = torch.sqrt(gt[:, 0] ** 2 + gt[:, 1] ** 2)
        assert float((mag - c["max_flow"]).abs().min()) >= 1.0 and bool((mag > c["max_flow"]).any())
        epe = torch.sqrt(((formula(fl[-1], mk[-1]) - gt) ** 2).sum(dim=1))
        for thr in (1.0, 3.0, 5.0):
            assert float((epe - thr).abs().min()) >= c["epe_margin"]
        assert 0 < r64["acc"][1] < r64["acc"][2] < r64["acc"][3] < r64["acc"][4]
        print("%-16s rel bar of the scalars %.2e" % (c["name"], c["rel_bar"]))


def _args(built, **kw):
    a = built.MpfUpsampleArgs()
    one = 256
    for k in ("flow", "mask", "out", "flow_gt", "valid", "g", "term", "metrics", "grad_flow", "grad_mask", "workspace"):
        setattr(a, k, one)
    a.workspace_bytes, a.N, a.H, a.W, a.max_flow = 1 << 30, 2, 36, 120, 400.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_c_abi_refuses_bad_arguments(built):
    """validated before anything is launched: no GPU is needed to be told so.  Status 10001 and a message that names the argument."""
    lib = built.load()
    fns = dict(fwd=lib.mpf_upsample_flow, bwd=lib.mpf_upsample_flow_backward, loss=lib.mpf_flow_loss_term, lbwd=lib.mpf_flow_loss_term_backward)
    common = [(dict(flow=None), b"flow"), (dict(mask=None), b"mask"), (dict(N=0), b"bad shape"), (dict(H=0), b"bad shape"), (dict(W=-3), b"bad shape"),
              (dict(N=1 << 12, H=1 << 10, W=1 << 10), b"2^31"), (dict(N=1, H=1 << 16, W=1 << 16), b"2^31"), (dict(N=2, H=1100, W=1700), b"2^31")]
    only = dict(fwd=[(dict(out=None), b"out"), (dict(out=260), b"16-byte aligned")],
                bwd=[(dict(out=None), b"out"), (dict(grad_flow=None), b"grad_flow"), (dict(grad_mask=None), b"grad_mask"), (dict(workspace=None), b"workspace"),
                     (dict(workspace_bytes=2 * 18 * 36 * 120 * 4 - 1), b"workspace"), (dict(workspace=260), b"8-byte")],
                loss=[(dict(flow_gt=None), b"flow_gt"), (dict(valid=None), b"valid"), (dict(term=None), b"term"), (dict(valid=264), b"16-byte aligned"),
                      (dict(workspace=None), b"workspace"), (dict(workspace_bytes=8), b"workspace")],
                lbwd=[(dict(flow_gt=None), b"flow_gt"), (dict(valid=None), b"valid"), (dict(g=None), b"(g)"), (dict(grad_flow=None), b"grad_flow"),
                      (dict(grad_mask=None), b"grad_mask"), (dict(workspace_bytes=100), b"workspace")])
    for name, fn in fns.items():
        assert fn(None, None) == 10001 and b"null argument block" in lib.mpf_last_error()
        for kw, word in common + only[name]:
            assert fn(ctypes.byref(_args(built, **kw)), None) == 10001, (name, kw)
            assert word in lib.mpf_last_error(), (name, kw, lib.mpf_last_error())
    assert lib.mpf_upsample_workspace(2, 36, 120, 1) == 2 * 18 * 36 * 120 * 4 and lib.mpf_upsample_workspace(2, 36, 120, 0) == 2 * 68 * 6 * 8
    assert lib.mpf_upsample_workspace(0, 36, 120, 0) == 0 and lib.mpf_upsample_workspace(1, 1 << 16, 1 << 16, 1) == 0


def test_both_libraries_export_the_symbols(built):
    for path in (built.LIB_PATH, built.WITNESS_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for n in ("mpf_upsample_flow", "mpf_upsample_flow_backward", "mpf_flow_loss_term", "mpf_flow_loss_term_backward", "mpf_upsample_workspace",
                  "k_upsample"):
            assert n in syms, (path, n)


def test_public_functions_refuse_what_they_cannot_take(built):
    from mpiflow_amd import raft_upsample as ru
    E = built.MpiFlowHipError
    f, m = torch.zeros(1, 2, 4, 6), torch.zeros(1, 576, 4, 6)
    gt, va = torch.zeros(1, 2, 32, 48), torch.zeros(1, 32, 48)
    with pytest.raises(E, match="no CPU path"):
        ru.upsample_flow(f, m)
    with pytest.raises(E, match="no CPU path"):
        ru.flow_loss_term(f, m, gt, va)
    with pytest.raises(E, match="no CPU path"):
        ru.sequence_loss([f], [m], gt, va)
    for bad in (torch.float16, torch.bfloat16):
        with pytest.raises(E, match=r"mask must be float32.*\.float\(\)"):
            ru.upsample_flow(f, m.to(bad))
        with pytest.raises(E, match=r"mask must be float32.*\.float\(\)"):
            ru.sequence_loss([f], [m.to(bad)], gt, va)
    with pytest.raises(E, match="flow must be float32"):
        ru.upsample_flow(f.double(), m)
    for wrong in (torch.zeros(1, 575, 4, 6), torch.zeros(1, 576, 4, 7), torch.zeros(2, 576, 4, 6), torch.zeros(576, 4, 6)):
        with pytest.raises(E, match="mask must be"):
            ru.upsample_flow(f, wrong)
    with pytest.raises(E, match="flow must be"):
        ru.upsample_flow(torch.zeros(1, 3, 4, 6), m)
    with pytest.raises(E, match="flow_gt must be"):
        ru.flow_loss_term(f, m, torch.zeros(1, 2, 32, 40), va)
    with pytest.raises(E, match="valid must be"):
        ru.flow_loss_term(f, m, gt, torch.zeros(1, 1, 32, 48))
    with pytest.raises(E, match="mask must be contiguous"):
        ru.upsample_flow(f, torch.zeros(1, 4, 6, 576).permute(0, 3, 1, 2))
    with pytest.raises(E, match="flow must be contiguous"):
        ru.flow_loss_term(torch.zeros(1, 2, 6, 4).transpose(2, 3), m, gt, va)
    with pytest.raises(E, match="as many masks as flows"):
        ru.sequence_loss([f, f], [m], gt, va)
    with pytest.raises(E, match="as many masks as flows"):
        ru.sequence_loss([], [], gt, va)


# ----------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ru(built):
    from mpiflow_amd import raft_upsample
    return raft_upsample


def check_big(c, key, hip, full64, what):
    """the rule of the issue, twice: sampled entries against the recorded double run, every entry against formula() in float64"""
    s = c[key]
    hip = hip.double().cpu().numpy()
    d_s = np.abs(hip.reshape(-1)[s["idx"]] - s["f64"]).max()
    d_f = np.abs(hip - full64.cpu().numpy()).max()
    print("%s %-16s %-13s |hip - ref64| sampled %.2e = %.2f err32, every entry vs formula64 %.2e = %.2f err32 (err32 %.2e)"
          % (what, c["name"], key, d_s, d_s / s["err32"], d_f, d_f / s["err32"], s["err32"]))
    assert d_s <= 3 * s["err32"] and d_f <= 3 * s["err32"], (c["name"], key, d_s, d_f, s["err32"])


def check_rel(c, what, got, want):
    rel = abs(got - want) / abs(want)
    print("%-10s %-16s rel err %.2e = %.2f of the bar %.2e" % (what, c["name"], rel, rel / c["rel_bar"], c["rel_bar"]))
    assert rel <= c["rel_bar"], (c["name"], what, got, want, rel, c["rel_bar"])


@pytest.mark.gpu
def test_gpu_upsample_flow_matches_the_recorded_reference(golden, ru, dev):
    for c in golden.values():
        want = reference_run(c, torch.float64, dev)
        fl, mk, _, _, cot = tensors(c, torch.float32, dev)
        f, m = fl[-1].requires_grad_(True), mk[-1].requires_grad_(True)
        out = ru.upsample_flow(f, m)
        assert out.shape == _shape(c, "pred_last") and out.dtype == torch.float32 and out.is_contiguous()
        out.backward(cot)
        check_big(c, "pred_last", out.detach(), want["pred_last"], "forward ")
        check_big(c, "up_grad_flow", f.grad, want["up_grad_flow"], "backward")
        check_big(c, "up_grad_mask", m.grad, want["up_grad_mask"], "backward")


@pytest.mark.gpu
def test_gpu_loss_matches_the_recorded_reference(golden, ru, dev):
    for c in golden.values():
        want = reference_run(c, torch.float64, dev)
        fl, mk, gt, va, _ = tensors(c, torch.float32, dev, grad=True)
        for i in range(c["iters"]):
            term = ru.flow_loss_term(fl[i].detach(), mk[i].detach(), gt, va, c["max_flow"])
            assert term.dim() == 0 and term.is_cuda and term.dtype == torch.float32
            check_rel(c, "term %d" % i, float(term), float(c["terms"]["f64"][i]))
        loss, metrics = ru.sequence_loss(fl, mk, gt, va, gamma=c["gamma"], max_flow=c["max_flow"])
        assert loss.dim() == 0 and loss.is_cuda and sorted(metrics) == ["1px", "3px", "5px", "epe"] and all(type(v) is float for v in metrics.values())
        check_rel(c, "loss", float(loss), float(c["loss"]["f64"]))
        acc = c["acc"]["f64"]
        check_rel(c, "epe", metrics["epe"], acc[0] / acc[4])
        from mpiflow_amd import ops
        _, got = ops.flow_loss_term(fl[-1].detach(), mk[-1].detach(), gt, va, c["max_flow"], metrics=True)
        assert [int(v) for v in got.tolist()[1:]] == [int(v) for v in acc[1:]] == want["acc"][1:]
        for k, q in (("1px", 1), ("3px", 2), ("5px", 3)):
            assert metrics[k] == acc[q] / acc[4]
        loss.backward()
        for i in range(c["iters"]):
            check_big(c, "grad_flow_%d" % i, fl[i].grad, want["grad_flow_%d" % i], "loss bwd")
            check_big(c, "grad_mask_%d" % i, mk[i].grad, want["grad_mask_%d" % i], "loss bwd")


@pytest.mark.gpu
def test_gpu_no_valid_pixel_gives_nan_metrics_and_zero_loss(golden, ru, dev):
    c = golden["tiny_1x5x7"]
    fl, mk, gt, va, _ = tensors(c, torch.float32, dev)
    loss, metrics = ru.sequence_loss(fl, mk, gt, torch.zeros_like(va), gamma=c["gamma"])
    assert float(loss) == 0.0 and all(np.isnan(v) for v in metrics.values())


@pytest.mark.gpu
def test_gpu_sign_of_zero_and_masked_entries_give_no_gradient(ru, dev):
    """flow = 0: the prediction is exactly 0.  Entries with flow_gt = 0 have sign 0; invalid and over-max_flow entries are masked: where ALL 64
    entries of a coarse pixel are of these kinds grad_mask is exactly 0, and with every entry so, grad_flow is exactly 0 as well."""
    N, H, W = 2, 6, 70
    gen = torch.Generator(device="cpu").manual_seed(11)
    mask = torch.randn(N, 576, H, W, generator=gen).to(dev)
    flow = torch.zeros(N, 2, H, W, device=dev)
    assert not ru.upsample_flow(flow, mask).any()
    gt = torch.randn(N, 2, 8 * H, 8 * W, generator=gen)
    valid = torch.ones(N, 8 * H, 8 * W)
    kind = torch.randint(0, 4, (N, H, W), generator=gen)                  # per coarse pixel: 0 live, 1 gt = 0, 2 invalid, 3 over max_flow
    fine = kind.repeat_interleave(8, 1).repeat_interleave(8, 2)
    gt[(fine == 1)[:, None].expand_as(gt)] = 0.0
    valid[fine == 2] = 0.0
    gt[:, 0][fine == 3] = 500.0
    for all_dead in (False, True):
        g2, v2 = gt.clone(), valid.clone()
        if all_dead:
            g2[(fine == 0)[:, None].expand_as(gt)] = 0.0
        f, m = flow.clone().requires_grad_(True), mask.clone().requires_grad_(True)
        term = ru.flow_loss_term(f, m, g2.to(dev), v2.to(dev))
        term.backward()
        dead = (kind != 0).to(dev) if not all_dead else torch.ones_like(kind, dtype=torch.bool).to(dev)
        assert not m.grad.permute(0, 2, 3, 1)[dead].any()
        if all_dead:
            assert not f.grad.any() and not m.grad.any()
        else:            # live entries count and dead ones add nothing: float64 autograd of the statement (grad_mask is 0 throughout: flow is 0)
            f64 = flow.double().requires_grad_(True)
            term_formula(formula(f64, mask.double()), g2.double().to(dev), v2.double().to(dev), 400.0).backward()
            assert f.grad.any() and float(term) > 0
            assert float((f.grad.double() - f64.grad).abs().max()) <= 1e-6 * float(f64.grad.abs().max())


@pytest.mark.gpu
def test_gpu_two_runs_are_bit_identical(golden, ru, dev):
    c = golden["real_2x36x120"]
    runs = []
    for _ in range(2):
        fl, mk, gt, va, cot = tensors(c, torch.float32, dev, grad=True)
        out = ru.upsample_flow(fl[0], mk[0])
        out.backward(cot)
        loss, metrics = ru.sequence_loss(fl[1:], mk[1:], gt, va, gamma=c["gamma"])
        loss.backward()
        runs.append([out.detach(), loss.detach()] + [t.grad for t in fl + mk] + [torch.tensor(sorted(metrics.values()))])
    for a, b in zip(*runs):
        assert torch.equal(a.cpu(), b.cpu())


@pytest.mark.gpu
def test_gpu_sequence_loss_equals_the_loss_of_its_own_upsampled_predictions(golden, ru, dev):
    """the same kernels' arithmetic up to summation order: plain-torch loss over upsample_flow's outputs, value and gradients"""
    c = golden["real_2x36x120"]
    fl, mk, gt, va, _ = tensors(c, torch.float32, dev, grad=True)
    loss, _ = ru.sequence_loss(fl, mk, gt, va, gamma=c["gamma"], max_flow=c["max_flow"])
    loss.backward()
    fl2, mk2, _, _, _ = tensors(c, torch.float32, dev, grad=True)
    loss2, _ = loss_formula(fl2, mk2, gt, va, c["gamma"], c["max_flow"], up=ru.upsample_flow)
    loss2.backward()
    check_rel(c, "composed", float(loss), float(loss2.double()))
    for i in range(c["iters"]):
        for a, b, key in ((fl[i], fl2[i], "grad_flow_%d" % i), (mk[i], mk2[i], "grad_mask_%d" % i)):
            assert float((a.grad.double() - b.grad.double()).abs().max()) <= 3 * c[key]["err32"], key


@pytest.mark.gpu
def test_gpu_no_prediction_is_materialised(golden, ru, dev):
    """12 iterations at 2 x 36 x 120: forward allocates, beyond its inputs, less than ONE full-resolution flow field; so does backward beyond the
    inputs and the gradients it returns."""
    c = golden["real_2x36x120"]
    fl, mk, gt, va, _ = tensors(c, torch.float32, dev, grad=True)
    one_field = c["N"] * 2 * 64 * c["H"] * c["W"] * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    loss, _ = ru.sequence_loss(fl, mk, gt, va, gamma=c["gamma"])
    torch.cuda.synchronize()
    fwd = torch.cuda.max_memory_allocated(dev) - before
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    loss.backward()
    torch.cuda.synchronize()
    grads = sum(t.grad.numel() * 4 for t in fl + mk)
    bwd = torch.cuda.max_memory_allocated(dev) - before - grads
    print("forward allocates %.3f MB, backward %.3f MB beyond the returned gradients; one full-resolution field %.3f MB" % (fwd / 1e6, bwd / 1e6, one_field / 1e6))
    assert fwd < one_field and bwd < one_field


@pytest.mark.gpu
def test_gpu_side_stream_and_interleaved_streams(golden, ru, dev):
    ca, cb = golden["mid_1x13x83"], golden["tiny_1x5x7"]

    def run(c):
        fl, mk, gt, va, cot = tensors(c, torch.float32, dev, grad=True)
        out = ru.upsample_flow(fl[0], mk[0])
        out.backward(cot)
        loss, _ = ru.sequence_loss(fl[1:], mk[1:], gt, va, gamma=c["gamma"])
        loss.backward()
        return [out.detach(), loss.detach()] + [t.grad for t in fl + mk]

    alone = {c["name"]: run(c) for c in (ca, cb)}
    torch.cuda.synchronize()
    busy, s1, s2 = [torch.cuda.Stream(device=dev) for _ in range(3)]
    big = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(busy):
        for _ in range(20):
            big = big @ big * 1e-3
    with torch.cuda.stream(s1):
        side = run(ca)
    s1.synchronize()
    for a, b in zip(side, alone[ca["name"]]):
        assert torch.equal(a, b)
    # two calls interleaved on two streams: forward of each, then backward of each
    got = {}
    state = {}
    for c, s in ((ca, s1), (cb, s2)):
        with torch.cuda.stream(s):
            fl, mk, gt, va, _ = tensors(c, torch.float32, dev, grad=True)
            state[c["name"]] = (fl, mk, ru.sequence_loss(fl[1:], mk[1:], gt, va, gamma=c["gamma"])[0])
    for c, s in ((ca, s1), (cb, s2)):
        with torch.cuda.stream(s):
            fl, mk, loss = state[c["name"]]
            loss.backward()
            got[c["name"]] = [loss.detach()] + [t.grad for t in fl[1:] + mk[1:]]
    s1.synchronize()
    s2.synchronize()
    busy.synchronize()
    for c in (ca, cb):
        n = c["iters"]
        want = alone[c["name"]]
        want = [want[1]] + want[3:2 + n] + want[3 + n:]
        assert len(want) == len(got[c["name"]])
        for a, b in zip(got[c["name"]], want):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_gpu_nan_in_the_mask_stays_where_it_is(ru, dev):
    """one NaN at mask[n, k*64 + i*8 + j, h, w] reaches out[n, :, 8h+i, 8w+j] and nothing else; inf in flow and flow_gt do not stop the run"""
    N, H, W = 2, 7, 67
    gen = torch.Generator(device="cpu").manual_seed(3)
    flow, mask = torch.randn(N, 2, H, W, generator=gen).to(dev), torch.randn(N, 576, H, W, generator=gen).to(dev)
    clean = ru.upsample_flow(flow, mask)
    n, k, i, j, h, w = 1, 4, 5, 2, 6, 66
    mask[n, k * 64 + i * 8 + j, h, w] = float("nan")
    out = ru.upsample_flow(flow, mask)
    bad = torch.isnan(out)
    want = torch.zeros_like(bad)
    want[n, :, 8 * h + i, 8 * w + j] = True
    assert torch.equal(bad, want) and torch.equal(out[~want], clean[~want])
    gt = torch.randn(N, 2, 8 * H, 8 * W, generator=gen).to(dev)
    gt[0, 0, 3, 3] = float("inf")
    flow[0, 1, 0, 0] = float("-inf")
    f, m = flow.requires_grad_(True), mask.requires_grad_(True)
    loss, metrics = ru.sequence_loss([f], [m], gt, torch.ones(N, 8 * H, 8 * W, device=dev))
    loss.backward()
    torch.cuda.synchronize()
    assert not torch.isfinite(loss) and f.grad.shape == flow.shape and m.grad.shape == mask.shape
