"""RAFT's training step (mpiflow_amd/raft_train.py): ClippedAdamW over mpf_grad_norm / mpf_adamw_clipped (mpf_optim.hip), fetch_optimizer, train_step.

Parity.  The reference is torch's clip_grad_norm_ + torch.optim.AdamW + OneCycleLR run in float64 on the CPU from the same float32 starting
values and gradients.  Per array (a parameter, exp_avg or exp_avg_sq after a step) the bar is absolute:
    max |hip - ref64| <= max(3 * err32, 2 * 2^-23 * absmax(ref64)),    err32 = max |torch's float32 CPU run - ref64| over that array,
computed here.  3 x the reference's own float32 error is the project's convention (profiles/raft/README.md); the floor of 2 ulp of the array's
largest magnitude covers arrays where err32 is zero.  total_norm: the same rule on the relative error.  Measured: profiles/train/README.md.

Tensor sets.  A: numels 1, 63, 64, 65 (a wave and its neighbours), CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3 (the vector path, the scalar tail,
more than one chunk), one parameter and gradient that are `buf[1:]` views (4-byte aligned only: whole chunks on the scalar path), one parameter
whose grad stays None, one with requires_grad=False.  B: TENSORS_PER_LAUNCH + 1 tensors of numels 1, 2, ...: two launches per pass.  CHUNK and
TENSORS_PER_LAUNCH are read from the library's Python mirror.  Three steps under OneCycleLR(max_lr=4e-4, total_steps=10, pct_start=0.3,
cycle_momentum=False, anneal_strategy='linear'), weight_decay=1e-4, eps=1e-8, clip=1.0; gradients N(0,1) in steps 1 and 3, 1e-3 N(0,1) in
step 2: set A's norms are about 157, 0.16, 156, so the clip and the coefficient-1 branch are both taken.
"""
import argparse
import copy
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mpf_adamw_workspace", "mpf_grad_norm", "mpf_adamw_clipped")
STRUCTS = ("MpfOptTensor", "MpfAdamWArgs")
ULP = 2.0 ** -23
HYPER = dict(weight_decay=1e-4, eps=1e-8)
STEPS = 3
GRAD_SCALE = (1.0, 1e-3, 1.0)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def rt(built):
    from mpiflow_amd import raft_train
    return raft_train


def _maker():
    spec = importlib.util.spec_from_file_location("make_raft_golden", os.path.join(ROOT, "tests", "golden", "make_raft_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------------------------ no GPU needed


def test_symbols_are_declared_bound_and_exported(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read(), flags=re.S)
    for path in (built.LIB_PATH, built.WITNESS_PATH):
        lib = ctypes.CDLL(path)
        for name in SYMBOLS:
            assert name in built.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name), name
    for name in STRUCTS:
        assert re.search(r"\}\s*%s\s*;" % name, hdr) and issubclass(getattr(built, name), ctypes.Structure), name
    assert built.load().mpf_version() == 601
    for define, mirror in (("MPF_OPT_CHUNK", built.OPT_CHUNK), ("MPF_OPT_TENSORS_PER_LAUNCH", built.OPT_TENSORS_PER_LAUNCH),
                           ("MPF_OPT_WORKSPACE_TAIL", built.OPT_WORKSPACE_TAIL), ("MPF_OPT_MAX_CHUNKS", built.OPT_MAX_CHUNKS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % define, hdr).group(1)) == mirror, define


def host_table(built, numels, ptr=256, grad=256):
    t = (built.MpfOptTensor * max(1, len(numels)))()
    for r, n in zip(t, numels):
        r.param, r.exp_avg, r.exp_avg_sq, r.grad, r.numel = ptr, ptr, ptr, grad, n
    return t


def test_workspace_of_a_host_table(built):
    lib = built.load()
    C = built.OPT_CHUNK
    # 1 + 1 + 2 chunks, one float64 partial each, behind the fixed tail (the sum of squares, the norm, the coefficient)
    assert lib.mpf_adamw_workspace(host_table(built, (1, C, C + 1)), 3) == built.OPT_WORKSPACE_TAIL + 4 * 8 == 48
    assert lib.mpf_adamw_workspace(host_table(built, (1, C, C + 1), grad=None), 3) == 48      # sized for every record, with a grad or not
    assert lib.mpf_adamw_workspace(host_table(built, (1,)), 0) == 0 and b"count" in lib.mpf_last_error()
    assert lib.mpf_adamw_workspace(host_table(built, (3, 0)), 2) == 0 and b"numel" in lib.mpf_last_error()
    assert lib.mpf_adamw_workspace(None, 1) == 0
    assert lib.mpf_adamw_workspace(host_table(built, (built.OPT_MAX_CHUNKS * C,)), 1) == built.OPT_WORKSPACE_TAIL + 8 * built.OPT_MAX_CHUNKS
    assert lib.mpf_adamw_workspace(host_table(built, (built.OPT_MAX_CHUNKS * C, 1)), 2) == 0 and b"too many chunks" in lib.mpf_last_error()


def good_args(built, numels=(5, 7)):
    a = built.MpfAdamWArgs()
    table = host_table(built, numels)
    a.tensors, a.count = table, len(numels)
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = 1e-3, 0.9, 0.999, 1e-8, 1e-2
    a.bias_correction1, a.bias_correction2_sqrt, a.max_norm = 0.1, math.sqrt(0.001), 1.0
    a.total_norm, a.workspace, a.workspace_bytes = 256, 256, 1 << 20
    return a, table


def test_every_refusal_is_an_error_code_before_any_launch(built):
    """dummy non-null pointers: a call that got past its checks would fault, so a returned code is also proof that nothing was launched"""
    lib = built.load()
    inf, nan = float("inf"), float("nan")

    def refused(fn, words, **change):
        a, table = good_args(built, change.pop("numels", (5, 7)))
        for k, v in change.items():
            if k.startswith("t0_"):
                setattr(table[0], k[3:], v)
            else:
                setattr(a, k, v)
        assert fn(ctypes.byref(a), None) == 10001, (fn.__name__, change)
        msg = lib.mpf_last_error()
        assert fn.__name__.encode() in msg and re.search(words, msg.decode()), (fn.__name__, change, msg)

    for fn in (lib.mpf_grad_norm, lib.mpf_adamw_clipped):
        assert fn(None, None) == 10001 and b"null argument block" in lib.mpf_last_error() and fn.__name__.encode() in lib.mpf_last_error()
        refused(fn, r"null pointer \(tensors\)", tensors=None)
        refused(fn, "count must be at least 1", count=0)
        refused(fn, "count must be at least 1", count=-3)
        refused(fn, r"tensors\[0\]\.numel must be at least 1", t0_numel=0)
        refused(fn, r"tensors\[0\]\.numel must be at least 1", t0_numel=-4)
        refused(fn, "too many chunks", numels=(built.OPT_MAX_CHUNKS * built.OPT_CHUNK, 1))
        refused(fn, "too many chunks", t0_numel=built.OPT_MAX_CHUNKS * built.OPT_CHUNK + 1)
        refused(fn, "4-byte aligned", t0_grad=258)
        refused(fn, r"null pointer \(total_norm\)", total_norm=None)
        refused(fn, r"null pointer \(workspace\)", workspace=None)
        refused(fn, "workspace must be 8-byte aligned", workspace=260)
        refused(fn, "workspace holds 31 bytes, 32 needed", workspace_bytes=31)
    fn = lib.mpf_adamw_clipped
    for field in ("param", "exp_avg", "exp_avg_sq"):
        refused(fn, r"null pointer \(param, exp_avg or exp_avg_sq of tensors\[0\]", **{"t0_" + field: None})
    refused(fn, "4-byte aligned", t0_exp_avg=257)
    refused(fn, "workspace holds 15 bytes, 16 needed", workspace_bytes=15, norm_ready=1)
    refused(fn, "lr must not be negative", lr=-1e-3)
    refused(fn, "eps must be positive", eps=0.0)
    refused(fn, "eps must be positive", eps=-1e-8)
    refused(fn, "eps must be positive", eps=1e-60)                        # zero in float32: the denominator would lose it
    refused(fn, "weight_decay must not be negative", weight_decay=-0.1)
    for beta in ("beta1", "beta2"):
        refused(fn, r"betas must lie in \[0, 1\)", **{beta: 1.0})
        refused(fn, r"betas must lie in \[0, 1\)", **{beta: -0.1})
    for bc in ("bias_correction1", "bias_correction2_sqrt"):
        refused(fn, r"bias corrections .* must lie in \(0, 1\]", **{bc: 0.0})
        refused(fn, r"bias corrections .* must lie in \(0, 1\]", **{bc: 1.5})
    refused(fn, "max_norm must be positive", max_norm=0.0)
    refused(fn, "max_norm must be positive", max_norm=-1.0)
    refused(fn, "max_norm must be positive", max_norm=nan)
    refused(fn, "max_norm must be positive", max_norm=-inf)
    for field in ("lr", "beta1", "beta2", "eps", "weight_decay", "bias_correction1", "bias_correction2_sqrt"):
        refused(fn, "non-finite hyperparameter", **{field: inf})
        refused(fn, "non-finite hyperparameter", **{field: nan})
    refused(fn, "zero_grad must be 0 or 1", zero_grad=2)
    refused(fn, "norm_ready must be 0 or 1", norm_ready=2)


KW = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, step=1, max_norm=1.0)


def test_ops_judge_type_dtype_shape_contiguity_and_the_device_last(built, monkeypatch):
    from mpiflow_amd import ops
    E = built.MpiFlowHipError

    def load():
        raise AssertionError("the library was asked for before the arguments were judged")
    monkeypatch.setattr(built, "load", load)
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    four = lambda: ([z(3, 4), z(5)], [z(3, 4), z(5)], [z(3, 4), z(5)], [z(3, 4), z(5)])           # params, grads, exp_avgs, exp_avg_sqs
    with pytest.raises(E, match=r"grad_norm: grads\[1\] must be a torch\.Tensor \(got ndarray\)"):
        ops.grad_norm([z(3), np.zeros(3, np.float32)])
    with pytest.raises(E, match=r"grad_norm: grads\[1\] must be float32 \(got torch\.float64\)"):
        ops.grad_norm([z(3), z(3, dtype=torch.float64)])
    with pytest.raises(E, match=r"grad_norm: grads\[0\] must be contiguous"):
        ops.grad_norm([z(3, 4).t(), z(3)])
    with pytest.raises(E, match=r"grad_norm: grads\[0\] must live on the GPU"):
        ops.grad_norm([z(3, 4), None, z(3)])
    with pytest.raises(E, match="at least 1"):
        ops.grad_norm([])
    with pytest.raises(E, match="every entry of grads is None"):
        ops.grad_norm([None, None])
    p, g, m, v = four()
    with pytest.raises(E, match="lists of one length"):
        ops.adamw_clipped(p, g[:1], m, v, **KW)
    p, g, m, v = four()
    g[1] = z(5, dtype=torch.float16)
    with pytest.raises(E, match=r"adamw_clipped: grads\[1\] must be float32 \(got torch\.float16\)"):
        ops.adamw_clipped(p, g, m, v, **KW)
    p, g, m, v = four()
    m[0] = z(4, 3)
    with pytest.raises(E, match=r"adamw_clipped: exp_avgs\[0\] must be of the shape of its record's first tensor, \(3, 4\), .*\(got shape \(4, 3\)\)"):
        ops.adamw_clipped(p, g, m, v, **KW)
    p, g, m, v = four()
    v[0] = z(4, 3).t()
    with pytest.raises(E, match=r"adamw_clipped: exp_avg_sqs\[0\] must be contiguous"):
        ops.adamw_clipped(p, g, m, v, **KW)
    p, g, m, v = four()
    v[1] = z(6)                                                          # a wrong shape further down is named before the device of the first
    with pytest.raises(E, match=r"exp_avg_sqs\[1\] must be of the shape"):
        ops.adamw_clipped(p, g, m, v, **KW)
    p, g, m, v = four()
    with pytest.raises(E, match=r"adamw_clipped: params\[0\] must live on the GPU .*no CPU path"):
        ops.adamw_clipped(p, g, m, v, **KW)
    g[0] = None                                                          # a skipped record is still judged: its parameter is on the CPU
    with pytest.raises(E, match=r"adamw_clipped: params\[0\] must live on the GPU"):
        ops.adamw_clipped(p, g, m, v, **KW)


def test_clipped_adamw_refuses_at_construction(rt, built):
    E = built.MpiFlowHipError
    P = lambda *s, dtype=torch.float32: torch.nn.Parameter(torch.zeros(*s, dtype=dtype))
    with pytest.raises(E, match="amsgrad=True is not supported"):
        rt.ClippedAdamW([P(3)], lr=1e-3, amsgrad=True)
    with pytest.raises(E, match="maximize=True is not supported"):
        rt.ClippedAdamW([P(3)], lr=1e-3, maximize=True)
    with pytest.raises(E, match=r"parameter 1 of group 0 must be float32 \(got torch\.float64\)"):
        rt.ClippedAdamW([P(3), P(3, dtype=torch.float64)], lr=1e-3)
    with pytest.raises(E, match="parameter 0 of group 0 must be contiguous"):
        rt.ClippedAdamW([torch.zeros(3, 4).t().requires_grad_()], lr=1e-3)
    with pytest.raises(E, match="parameter 0 of group 0 must live on the GPU"):
        rt.ClippedAdamW([P(3), P(4)], lr=1e-3)
    for bad, words in ((dict(lr=-1.0), "invalid learning rate"), (dict(eps=0.0), "eps must be positive"), (dict(betas=(0.9, 1.0)), "betas must lie"),
                       (dict(weight_decay=-1.0), "invalid weight_decay"), (dict(clip=0.0), "clip must be positive"), (dict(clip=float("nan")), "clip must be positive")):
        with pytest.raises(E, match=words):
            rt.ClippedAdamW([P(3)], **bad)
    with pytest.raises(E, match="optimizer must be a ClippedAdamW"):
        rt.train_step(None, torch.optim.AdamW([P(3)]), None, {})


# --------------------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def numels_of(built, which):
    C = built.OPT_CHUNK
    return [1, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3] if which == "A" else list(range(1, built.OPT_TENSORS_PER_LAUNCH + 2))


_DATA = {}


def data_of(built, which):
    """the float32 starting values and the gradients of the three steps, as numpy arrays, made once: a list of records
    dict(kind, p0, grads[3]); kind 'plain', 'view' (stored one element into a buffer), 'nograd', 'frozen'"""
    if which not in _DATA:
        rs = np.random.RandomState(17 if which == "A" else 23)
        recs = [dict(kind="plain", n=n) for n in numels_of(built, which)]
        if which == "A":
            recs += [dict(kind="view", n=built.OPT_CHUNK + 3), dict(kind="nograd", n=5), dict(kind="frozen", n=7)]
        for r in recs:
            r["p0"] = rs.standard_normal(r["n"]).astype(np.float32)
            r["grads"] = [(s * rs.standard_normal(r["n"])).astype(np.float32) for s in GRAD_SCALE]
        _DATA[which] = recs
    return _DATA[which]


def scheduler_for(opt):
    return torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=4e-4, total_steps=10, pct_start=0.3, cycle_momentum=False, anneal_strategy="linear")


def make_params(recs, device, dtype):
    """the records as leaf tensors; a 'view' parameter is buf[1:] of a buffer one element longer, so 4-byte aligned only"""
    out = []
    for r in recs:
        src = torch.from_numpy(r["p0"].copy()).to(device=device, dtype=dtype)
        if r["kind"] == "view":
            buf = torch.zeros(r["n"] + 1, device=device, dtype=dtype)
            buf[1:] = src
            p = buf[1:]
            assert p.data_ptr() % 16 == src.element_size() and p.is_contiguous()
        else:
            p = src.clone()
        out.append(p.requires_grad_(r["kind"] != "frozen"))
    return out


def make_grad(r, step, device, dtype):
    g = torch.from_numpy(r["grads"][step].copy()).to(device=device, dtype=dtype)          # a copy: clip_grad_norm_ scales a CPU gradient in place
    if r["kind"] != "view":
        return g
    buf = torch.zeros(r["n"] + 1, device=device, dtype=dtype)
    buf[1:] = g
    return buf[1:]


def has_grad(r):
    return r["kind"] in ("plain", "view")


def snapshot(opt, params):
    return [dict(param=p.detach().clone(), exp_avg=opt.state[p]["exp_avg"].clone() if p in opt.state else None,
                 exp_avg_sq=opt.state[p]["exp_avg_sq"].clone() if p in opt.state else None) for p in params]


_REF = {}


def reference_of(built, which):
    """torch's clip_grad_norm_ + AdamW + OneCycleLR on the CPU in float64 and in float32, once -> {dtype: (snapshots per step, norms per step)}"""
    if which not in _REF:
        recs = data_of(built, which)
        res = {}
        for dtype in (torch.float64, torch.float32):
            params = make_params(recs, "cpu", dtype)
            opt = torch.optim.AdamW(params, lr=4e-4, **HYPER)
            sched = scheduler_for(opt)
            snaps, norms = [], []
            for s in range(STEPS):
                for p, r in zip(params, recs):
                    p.grad = make_grad(r, s, "cpu", dtype) if has_grad(r) else None
                norms.append(float(torch.nn.utils.clip_grad_norm_(params, 1.0)))
                opt.step()
                sched.step()
                snaps.append(snapshot(opt, params))
            res[dtype] = (snaps, norms)
        _REF[which] = res
    return _REF[which]


def bar_of(ref64, ref32):
    err32 = float((ref32.double() - ref64).abs().max())
    return max(3.0 * err32, 2.0 * ULP * float(ref64.abs().max())), err32


def run_ours(rt, built, dev, which, clips=(1.0, 1.0, 1.0), zero_grad=False, fresh=False, steps=STEPS, probe_norm=False):
    """ClippedAdamW over set `which` -> dict(snaps, norms (device tensors), params, opt, sched, grads (the tensors of the last step), ...).
    fresh=False: every gradient is allocated once and refilled in place; fresh=True: zero_grad(set_to_none=True) and new tensors per step
    (the old ones are kept alive, so the new ones cannot land on their addresses)."""
    from mpiflow_amd import ops
    recs = data_of(built, which)
    params = make_params(recs, dev, torch.float32)
    opt = rt.ClippedAdamW(params, lr=4e-4, clip=clips[0], **HYPER)
    sched = scheduler_for(opt)
    out = dict(snaps=[], norms=[], probes=[], params=params, opt=opt, sched=sched, recs=recs, keep=[], ptrs=[])
    for s in range(steps):
        opt.param_groups[0]["clip"] = clips[s]
        if fresh and s:
            out["keep"].append([p.grad for p in params])
            opt.zero_grad(set_to_none=True)
        for p, r in zip(params, recs):
            if not has_grad(r):
                continue
            g = make_grad(r, s, dev, torch.float32)
            if p.grad is None:
                p.grad = g
            else:
                p.grad.copy_(g)
        out["ptrs"].append([None if p.grad is None else p.grad.data_ptr() for p in params])
        if probe_norm:
            out["probes"].append(ops.grad_norm([p.grad for p in params]))
        out["norms"].append(opt.step(zero_grad=zero_grad))
        sched.step()
        out["snaps"].append(snapshot(opt, params))
    return out


def same_bytes(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_snapshots(x, y):
    return all(same_bytes(a[k], b[k]) for sx, sy in zip(x, y) for a, b in zip(sx, sy) for k in ("param", "exp_avg", "exp_avg_sq")) and len(x) == len(y)


_RUNS = {}


def plain_run(rt, built, dev, which):
    if which not in _RUNS:
        _RUNS[which] = run_ours(rt, built, dev, which, probe_norm=True)
    return _RUNS[which]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["A", "B"])
def test_gpu_three_steps_match_torch_in_float64(which, rt, built, dev):
    ref = reference_of(built, which)
    (snap64, norm64), (snap32, norm32) = ref[torch.float64], ref[torch.float32]
    run = plain_run(rt, built, dev, which)
    recs = run["recs"]
    worst = (0.0, None)
    failures = []
    for s in range(STEPS):
        got = float(run["norms"][s].cpu()[0])
        rel, rel32 = abs(got - norm64[s]) / norm64[s], abs(norm32[s] - norm64[s]) / norm64[s]
        bar = max(3.0 * rel32, 2.0 * ULP)
        print("set %s step %d total_norm %.9g (ref64 %.9g): rel %.2e = %.3f of the bar %.2e (torch fp32 rel %.2e); lr %.3e"
              % (which, s + 1, got, norm64[s], rel, rel / bar, bar, rel32, run["sched"].get_last_lr()[0] if s == STEPS - 1 else float("nan")))
        worst = max(worst, (rel / bar, "total_norm step %d" % (s + 1)))
        if rel > bar:
            failures.append(("total_norm", s, rel, bar))
        by_key = {}
        for i, r in enumerate(recs):
            for k in ("param", "exp_avg", "exp_avg_sq"):
                r64, r32, hip = snap64[s][i][k], snap32[s][i][k], run["snaps"][s][i][k]
                assert (r64 is None) == (hip is None) == (k != "param" and not has_grad(r)), (i, k)
                if r64 is None:
                    continue
                bar, err32 = bar_of(r64, r32)
                d = float((hip.double().cpu() - r64).abs().max())
                by_key[k] = max(by_key.get(k, (0.0, 0.0, 0)), (d / bar, err32 / (ULP * float(r64.abs().max()) or 1.0), r["n"]))
                worst = max(worst, (d / bar, "%s of numel %d (%s) step %d" % (k, r["n"], r["kind"], s + 1)))
                if d > bar:
                    failures.append((k, r["n"], s, d, bar, err32))
        for k, (ratio, e32, n) in sorted(by_key.items()):
            print("set %s step %d %-10s worst |hip - ref64| = %.3f of its bar (numel %d; torch fp32's own error there %.2f ulp of absmax)" % (which, s + 1, k, ratio, n, e32))
    print("set %s worst: %.3f of its bar (%s)" % (which, worst[0], worst[1]))
    n = [float(t.cpu()[0]) for t in run["norms"]]
    assert n[0] > 1.0 and n[1] < 1.0 and n[2] > 1.0, n                    # the clip, the coefficient 1, the clip
    assert not failures, failures


@pytest.mark.gpu
def test_gpu_bit_identities(rt, built, dev):
    a = plain_run(rt, built, dev, "A")
    b = run_ours(rt, built, dev, "A")
    assert same_snapshots(a["snaps"], b["snaps"]), "two optimizers from identical bytes differ after three steps"
    assert all(same_bytes(x, y) for x, y in zip(a["norms"], b["norms"]))
    # ops.grad_norm is the total_norm that step returns, and last_grad_norm keeps it
    assert all(same_bytes(x, y) for x, y in zip(a["probes"], a["norms"]))
    assert a["opt"].last_grad_norm is a["norms"][-1] and a["norms"][0].shape == (1,) and a["norms"][0].dtype == torch.float32 and a["norms"][0].is_cuda
    # step 2 has a norm below the clip: coefficient exactly 1, the bytes of the same step without clipping
    c = run_ours(rt, built, dev, "A", clips=(1.0, float("inf"), 1.0), steps=2)
    assert float(a["norms"][1].cpu()[0]) < 1.0 and same_snapshots(a["snaps"][:2], c["snaps"]) and same_bytes(a["norms"][1], c["norms"][1])
    # and clipping does something: step 1 without it differs
    d = run_ours(rt, built, dev, "A", clips=(float("inf"),) * 3, steps=1)
    assert same_bytes(a["norms"][0], d["norms"][0]) and not same_snapshots(a["snaps"][:1], d["snaps"])
    # the gradients are read, not scaled
    for p, r in zip(a["params"], a["recs"]):
        if has_grad(r):
            assert same_bytes(p.grad, torch.from_numpy(r["grads"][STEPS - 1]).to(dev))
    # zero_grad=True: the same parameters and moments; every gradient all-zero where it was; the parameter without one stays without
    z = run_ours(rt, built, dev, "A", zero_grad=True)
    assert same_snapshots(a["snaps"], z["snaps"]) and all(same_bytes(x, y) for x, y in zip(a["norms"], z["norms"]))
    assert z["ptrs"][0] == z["ptrs"][1] == z["ptrs"][2] == [None if p.grad is None else p.grad.data_ptr() for p in z["params"]]
    for p, r in zip(z["params"], z["recs"]):
        if has_grad(r):
            assert p.grad is not None and not p.grad.any() and not torch.signbit(p.grad).any(), r["n"]
        else:
            assert p.grad is None
    # the parameter without a gradient and the frozen one: byte-unchanged, no state
    for run in (a, z):
        for p, r in zip(run["params"], run["recs"]):
            if not has_grad(r):
                assert same_bytes(p.detach(), torch.from_numpy(r["p0"]).to(dev)) and p not in run["opt"].state, r["kind"]
            else:
                assert not same_bytes(p.detach(), torch.from_numpy(r["p0"]).to(dev))
    # the state is torch.optim.AdamW's: a CPU float32 scalar step
    st = a["opt"].state[a["params"][0]]
    assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"] and st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == STEPS


@pytest.mark.gpu
def test_gpu_gradient_pointers_may_move(rt, built, dev):
    a = plain_run(rt, built, dev, "A")
    f = run_ours(rt, built, dev, "A", fresh=True)
    moved = sum(1 for x, y in zip(f["ptrs"][0], f["ptrs"][1]) if x is not None and x != y)
    assert moved == sum(1 for x in f["ptrs"][0] if x is not None), "the fresh gradients did not move"
    assert same_snapshots(a["snaps"], f["snaps"]) and all(same_bytes(x, y) for x, y in zip(a["norms"], f["norms"]))


@pytest.mark.gpu
def test_gpu_several_groups_share_one_global_norm(rt, built, dev):
    """two parameter groups with different weight decay: one norm over both, one update call per group; against one group per weight decay
    on its own, whose norm the other group's gradients do not enter, the clipped step must differ and the unclipped one must not"""
    recs = data_of(built, "A")
    plain = [i for i, r in enumerate(recs) if has_grad(r)]
    half = len(plain) // 2
    res = {}
    for clip in (1.0, float("inf")):
        params = make_params(recs, dev, torch.float32)
        both = rt.ClippedAdamW([dict(params=[params[i] for i in plain[:half]], weight_decay=0.0), dict(params=[params[i] for i in plain[half:]])],
                               lr=4e-4, clip=clip, **HYPER)
        alone = make_params(recs, dev, torch.float32)
        singles = [rt.ClippedAdamW([alone[i] for i in plain[:half]], lr=4e-4, clip=clip, eps=HYPER["eps"], weight_decay=0.0),
                   rt.ClippedAdamW([alone[i] for i in plain[half:]], lr=4e-4, clip=clip, **HYPER)]
        for ps in (params, alone):
            for p, r in zip(ps, recs):
                p.grad = make_grad(r, 0, dev, torch.float32) if has_grad(r) else None
        from mpiflow_amd import ops
        want = ops.grad_norm([p.grad for p in params])
        got = both.step()
        assert same_bytes(got, want) and got is both.last_grad_norm
        parts = [o.step() for o in singles]
        assert all(float(x.cpu()[0]) < float(got.cpu()[0]) for x in parts)
        res[clip] = all(same_bytes(params[i].detach(), alone[i].detach()) for i in plain)
        sd = both.state_dict()
        assert [g["weight_decay"] for g in sd["param_groups"]] == [0.0, HYPER["weight_decay"]] and all(g["clip"] == clip for g in sd["param_groups"])
    assert res[float("inf")] and not res[1.0]


def torch_twin(params, sd, dev):
    clones = [p.detach().clone().requires_grad_(p.requires_grad) for p in params]
    opt = torch.optim.AdamW(clones, lr=4e-4, **HYPER)
    opt.load_state_dict(copy.deepcopy(sd))                               # as a saved checkpoint: load_state_dict itself may keep the tensors it is given
    return clones, opt


@pytest.mark.gpu
def test_gpu_checkpoints_move_between_clipped_adamw_and_torch_adamw(rt, built, dev):
    ref = reference_of(built, "A")
    recs = data_of(built, "A")
    last = STEPS - 1

    def third_step(params, opt, clip_first):
        for p, r in zip(params, recs):
            p.grad = make_grad(r, last, dev, torch.float32) if has_grad(r) else None
        if clip_first:
            torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()

    def agree(pa, oa, pb, ob, what):
        worst = 0.0
        for i, r in enumerate(recs):
            if not has_grad(r):
                assert same_bytes(pa[i].detach(), pb[i].detach())
                continue
            for k in ("param", "exp_avg", "exp_avg_sq"):
                bar, _ = bar_of(ref[torch.float64][0][last][i][k], ref[torch.float32][0][last][i][k])
                x = pa[i].detach() if k == "param" else oa.state[pa[i]][k]
                y = pb[i].detach() if k == "param" else ob.state[pb[i]][k]
                d = float((x.double() - y.double()).abs().max())
                worst = max(worst, d / bar)
                assert d <= bar, (what, k, r["n"], d, bar)
            assert float(oa.state[pa[i]]["step"]) == float(ob.state[pb[i]]["step"]) == STEPS
        print("checkpoint %s: worst |ours - torch| after the third step = %.3f of the parity bar" % (what, worst))

    # ours -> torch
    run = run_ours(rt, built, dev, "A", steps=2)
    sd = run["opt"].state_dict()
    st0 = sd["state"][0]
    assert sorted(st0) == ["exp_avg", "exp_avg_sq", "step"] and st0["step"].device.type == "cpu" and st0["step"].dtype == torch.float32
    theirs = torch.optim.AdamW([torch.zeros(1)]).state_dict()["param_groups"][0]
    assert set(sd["param_groups"][0]) - {"initial_lr", "max_lr", "min_lr"} == set(theirs) | {"clip"}
    clones, topt = torch_twin(run["params"], sd, dev)
    assert topt.param_groups[0]["lr"] == run["opt"].param_groups[0]["lr"]
    third_step(clones, topt, True)
    third_step(run["params"], run["opt"], False)
    agree(run["params"], run["opt"], clones, topt, "ours -> torch")

    # torch -> ours
    tparams = make_params(recs, dev, torch.float32)
    topt = torch.optim.AdamW(tparams, lr=4e-4, **HYPER)
    tsched = scheduler_for(topt)
    for s in range(2):
        for p, r in zip(tparams, recs):
            p.grad = make_grad(r, s, dev, torch.float32) if has_grad(r) else None
        torch.nn.utils.clip_grad_norm_(tparams, 1.0)
        topt.step()
        tsched.step()
    mine = [p.detach().clone().requires_grad_(p.requires_grad) for p in tparams]
    opt = rt.ClippedAdamW(mine, lr=1.0, clip=1.0)
    opt.load_state_dict(copy.deepcopy(topt.state_dict()))
    g = opt.param_groups[0]
    assert g["clip"] == 1.0 and g["lr"] == topt.param_groups[0]["lr"] and g["weight_decay"] == HYPER["weight_decay"] and g["eps"] == HYPER["eps"]
    third_step(tparams, topt, True)
    third_step(mine, opt, False)
    agree(mine, opt, tparams, topt, "torch -> ours")


def synthetic_batch(dev, N=1, H=128, W=128, seed=5):
    rs = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    image1 = rs.randint(0, 256, (N, 3, H, W))
    return dict(image1=t(image1), image2=t(np.roll(image1, (2, -3), axis=(2, 3))), flow=t(3.0 * rs.standard_normal((N, 2, H, W))),
                valid=t(rs.rand(N, H, W) > 0.1))


_STEPS = {}


def train_runs(small, rt, dev):
    """the model through two train_step calls, a twin through the same two steps written out by hand, and a replay of the optimizer alone on
    the gradients train_step's backward passes produced (cloned by a step pre-hook); once per model kind"""
    if small in _STEPS:
        return _STEPS[small]
    from mpiflow_amd import raft, raft_upsample
    mk = _maker()
    args = argparse.Namespace(lr=4e-4, wdecay=1e-4, epsilon=1e-8, clip=1.0, num_steps=10)
    batch = synthetic_batch(dev)
    iters, gamma = 2, 0.8

    def new_model():
        model = raft.RAFT(mk.make_args(small))
        mk.fill_params(model, 11)
        return model.to(dev).train()

    def by_hand(model, opt, sched):
        out = model(batch["image1"], batch["image2"], iters=iters, coarse="flow" if small else True)
        if small:
            loss, metrics = raft_upsample.sequence_loss(out, None, batch["flow"], batch["valid"], gamma)
        else:
            loss, metrics = raft_upsample.sequence_loss([f for f, _ in out], [m for _, m in out], batch["flow"], batch["valid"], gamma)
        loss.backward()
        norm = opt.step(zero_grad=True)
        sched.step()
        return loss.detach(), metrics, norm

    # the library convolutions' backward is order-stable only when asked to be: both the model and its twin run under reproducible()
    with rt.reproducible():
        warm = new_model()                                                   # unmeasured: a convolution's first call in a process may pick another algorithm
        by_hand(warm, *rt.fetch_optimizer(args, warm))
        del warm

        model = new_model()
        r = dict(model=model, start={k: p.detach().clone() for k, p in model.named_parameters()}, seen=[])
        r["opt"], r["sched"] = opt, sched = rt.fetch_optimizer(args, model)
        r["no_grads_before"] = all(p.grad is None for p in model.parameters())
        hook = opt.register_step_pre_hook(lambda o, a, k: r["seen"].append([p.grad.clone() for p in model.parameters()]))
        r["got"] = [rt.train_step(model, opt, sched, batch, iters=iters, gamma=gamma) for _ in range(2)]
        hook.remove()
        r["ptrs"] = [p.grad.data_ptr() for p in model.parameters()]
        r["twin"] = twin = new_model()
        topt, tsched = rt.fetch_optimizer(args, twin)
        r["want"] = [by_hand(twin, topt, tsched) for _ in range(2)]
        # the optimizer alone, on the gradients the model's own backward passes made
        holder = torch.nn.ParameterList([torch.nn.Parameter(v.clone()) for v in r["start"].values()])
        ropt, rsched = rt.fetch_optimizer(args, holder)
        r["replay"] = replay = list(holder)
        r["replay_norms"] = []
        for grads in r["seen"]:
            for p, g in zip(replay, grads):
                p.grad = g.clone()
            r["replay_norms"].append(ropt.step(zero_grad=True))
            rsched.step()
    _STEPS[small] = r
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("small", [True, False], ids=["small", "basic"])
def test_gpu_train_step_updates_every_parameter(small, rt, built, dev):
    r = train_runs(small, rt, dev)
    model, opt, sched = r["model"], r["opt"], r["sched"]
    assert isinstance(opt, rt.ClippedAdamW) and isinstance(sched, torch.optim.lr_scheduler.OneCycleLR)
    g = opt.param_groups[0]
    assert (g["weight_decay"], g["eps"], g["clip"], g["max_lr"], sched.total_steps) == (1e-4, 1e-8, 1.0, 4e-4, 110)
    assert r["no_grads_before"]                                          # the first call found p.grad is None
    for loss, metrics, norm in r["got"]:
        assert loss.dim() == 0 and loss.is_cuda and not loss.requires_grad and norm.shape == (1,) and norm.is_cuda
        assert math.isfinite(float(loss)) and math.isfinite(float(norm)) and float(norm) > 0.0
        assert sorted(metrics) == ["1px", "3px", "5px", "epe"] and all(math.isfinite(v) for v in metrics.values())
    print("train_step %s: loss %.6f -> %.6f, total_norm %.4f -> %.4f, lr %.3e" % ("small" if small else "basic", float(r["got"][0][0]), float(r["got"][1][0]),
                                                                                  float(r["got"][0][2]), float(r["got"][1][2]), sched.get_last_lr()[0]))
    unchanged = [k for k, p in model.named_parameters() if same_bytes(p.detach(), r["start"][k])]
    assert not unchanged, unchanged
    # the gradients: zeroed in place, at the addresses the second backward accumulated into
    assert all(p.grad is not None and not p.grad.any() for p in model.parameters())
    assert r["ptrs"] == [p.grad.data_ptr() for p in model.parameters()]
    assert all(float(opt.state[p]["step"]) == 2.0 for p in model.parameters())
    # train_step's tail is the optimizer's step on the gradients its backward made: replayed alone on them, the same bytes
    assert all(same_bytes(x[2], y) for x, y in zip(r["got"], r["replay_norms"]))
    differ = [k for (k, p), q in zip(model.named_parameters(), r["replay"]) if not same_bytes(p.detach(), q.detach())]
    assert not differ, differ


@pytest.mark.gpu
@pytest.mark.parametrize("small", [True, False], ids=["small", "basic"])
def test_gpu_train_step_is_the_hand_written_step(small, rt, built, dev):
    """Parameters, loss, norm and metrics bit-identical to a second model taken through the same two steps by hand.

    Both run under raft_train.reproducible().  Without it this does not hold on an MI355X, and not because of the code under test: two
    models built from the same bytes give bit-identical forward passes but gradients of the feature encoder whose last bits differ from
    run to run (measured, four models in one process, step 1: coarse flows, masks, loss and epe identical to 17 digits; 22 of the small
    model's 106 gradients and 61 of the basic model's 124, all under fnet., differ), and after two steps 82 of 106 and 105 of 124 parameters
    differ from the twin's by up to 4.7e-6, the size of one update.  Repeated on fixed inputs, torch.matmul as CorrBlock's backward calls it
    is stable and the library convolution's backward is not, unless torch.backends.cudnn.deterministic is set, which is what reproducible()
    does: profiles/train/README.md."""
    r = train_runs(small, rt, dev)
    model, twin = r["model"], r["twin"]
    worst = (0.0, None)
    differ = []
    for (k, p), q in zip(model.named_parameters(), twin.parameters()):
        if not same_bytes(p.detach(), q.detach()):
            differ.append(k)
            worst = max(worst, (float((p.detach().double() - q.detach().double()).abs().max()), k))
    for s, ((loss, metrics, norm), (wloss, wmetrics, wnorm)) in enumerate(zip(r["got"], r["want"])):
        print("train_step %s step %d: loss %.9g / by hand %.9g, total_norm %.9g / %.9g, epe %.17g / %.17g"
              % ("small" if small else "basic", s + 1, float(loss), float(wloss), float(norm), float(wnorm), metrics["epe"], wmetrics["epe"]))
    print("train_step %s: %d of %d parameters differ from the hand-written twin's, largest difference %.3e (%s)"
          % ("small" if small else "basic", len(differ), len(list(twin.parameters())), worst[0], worst[1]))
    for (loss, metrics, norm), (wloss, wmetrics, wnorm) in zip(r["got"], r["want"]):
        assert same_bytes(loss, wloss) and same_bytes(norm, wnorm) and metrics == wmetrics
    assert not differ, differ
