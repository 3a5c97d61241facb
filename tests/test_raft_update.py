"""RAFT's update block with the GRU's pointwise work fused (mpiflow_amd/raft_update.py; mpf_gru_reset / _update and their _backward calls of
mpf_gru.hip).

The reference is the reference's own update.py, recorded on the CPU by tests/golden/make_update_golden.py into tests/golden/raft_update.npz:
per array 150 sampled entries of the DOUBLE run, err32 = max |fp32 run - double run| over the whole array, and max |ref64|.  Inputs and weights
are rebuilt from seeds (their float64 sums are checked).  A missing golden fails these tests; it does not skip them.

Bars.  Kernels alone: 3 * err32 of the recorded array they produce (the bar of tests/test_raft_corr.py and tests/test_raft_upsample.py), at the
samples against the recorded double run and at every entry against the formulas below in float64.  Two kernel results have no recorded
counterpart - d h of either backward kernel is only a share of the recorded total - and the scalar-path check runs on inputs of its own; their
bar comes from the number format: FMT_BAR = 16 * 2^-24 * max(1, max |result|).  (A result is a product of at most three factors, each good to
a few ulp: sigmoid and tanh about 2 ulp each, the fp32 sum of three terms of magnitude up to ~8 moves a gate by at most 0.25 * 8 * 2^-24,
one rounding per product; 16 ulp of the largest magnitude covers that with a factor of about two in hand.)
Modules: the convolutions are MIOpen's, so per array the bar is the larger of 3 * err32 and 2 x the error that the cat-form restatement below -
plain torch ops, the same device, fp32 - makes against the same double run.

Measured on an MI355X: profiles/update/README.md."""
import ctypes
import importlib.util
import os
import subprocess
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "raft_update.npz")
SYMBOLS = ("mpf_gru_reset", "mpf_gru_update", "mpf_gru_update_backward", "mpf_gru_reset_backward")
HALVES = {"SepConvGRU": (("1", (0, 2)), ("2", (2, 0))), "ConvGRU": (("", 1),)}
EPS32 = 2.0 ** -24


def _maker():
    spec = importlib.util.spec_from_file_location("make_update_golden", os.path.join(ROOT, "tests", "golden", "make_update_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN, allow_pickle=False)                  # a missing file is an error here, not a skip
    mk = _maker()
    g = dict(mk=mk, z=z, gru={}, block={}, state={k: [str(s) for s in z["state/" + k]] for k in ("SepConvGRU", "ConvGRU", "BasicUpdateBlock", "SmallUpdateBlock")})
    for name in [str(n) for n in z["gru_names"]]:
        B, C, Cx, n_ctx, H, W, seed = [int(v) for v in z[name + "/settings"]]
        h, x, cot = mk.case_inputs(B, C, Cx, H, W, seed)
        c = dict(name=name, cls=name.split("/")[0], B=B, C=C, Cx=Cx, n_ctx=n_ctx, H=H, W=W, seed=seed, h=h, x=x, cot=cot, sums=z[name + "/input_sums"])
        assert np.array_equal(np.array([a.astype(np.float64).sum() for a in (h, x, cot)]), c["sums"][:3]), "the seeded inputs of %s are not the recorded ones" % name
        _load_arrays(c, z, mk, seed)
        g["gru"][name] = c
    for name in [str(n) for n in z["block_names"]]:
        B, H, W, levels, radius, iters, seed = [int(v) for v in z[name + "/settings"]]
        d = mk.block_inputs(name.split("/")[0], B, H, W, levels, radius, iters, seed)
        c = dict(name=name, cls=name.split("/")[0], B=B, H=H, W=W, levels=levels, radius=radius, iters=iters, seed=seed, d=d, sums=z[name + "/input_sums"])
        assert sum(v.astype(np.float64).sum() for v in d.values()) == c["sums"][0], "the seeded inputs of %s are not the recorded ones" % name
        _load_arrays(c, z, mk, seed)
        g["block"][name] = c
    assert len(g["gru"]) == 10 and len(g["block"]) == 2
    return g


def _load_arrays(c, z, mk, seed):
    c["keys"] = [str(k) for k in z[c["name"] + "/keys"]]
    c["rec"] = {k: dict(f64=z["%s/%s_f64" % (c["name"], k)], err32=float(z["%s/%s_err32" % (c["name"], k)]), absmax=float(z["%s/%s_absmax" % (c["name"], k)]))
                for k in c["keys"]}
    c["index"] = lambda n, seed=seed: mk.sample_index(n, seed)


# ---------------------------------------------------------------------------------------- the formulas, restated (not code under test)


def sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def gru_cat(P, cls, h, x, cap=None, prefix=""):
    """the GRU as the issue states upstream's: convolutions over cat([h, x]) and cat([r*h, x])"""
    for s, pad in HALVES[cls]:
        w = lambda g: (P["%sconv%s%s.weight" % (prefix, g, s)], P["%sconv%s%s.bias" % (prefix, g, s)])
        hx = torch.cat([h, x], dim=1)
        pre_z, pre_r = F.conv2d(hx, *w("z"), padding=pad), F.conv2d(hx, *w("r"), padding=pad)
        r = torch.sigmoid(pre_r)
        rh = r * h
        pre_q = F.conv2d(torch.cat([rh, x], dim=1), *w("q"), padding=pad)
        z, q = torch.sigmoid(pre_z), torch.tanh(pre_q)
        if cap is not None:
            cap.update({"pre_z" + s: pre_z, "pre_r" + s: pre_r, "pre_q" + s: pre_q, "z" + s: z, "r" + s: r, "q" + s: q, "rh" + s: rh})
            if s != HALVES[cls][0][0]:
                cap["h_in" + s] = h
        h = (1 - z) * h + z * q
    return h


def gru_split(P, cls, h, x, n_ctx=0, cap=None, prefix=""):
    """the split form: per gate conv(h, W[:, :C]) + conv(x, W[:, C:]) + b, and with n_ctx > 0 the x part split once more into the hoisted
    context term conv(x[:, :n_ctx], W[:, C:C+n_ctx]) + b - computed for both halves BEFORE the first half runs - and the rest"""
    C = h.shape[1]
    inp, rest = x[:, :n_ctx], x[:, n_ctx:]
    ctx = {}
    for s, pad in HALVES[cls]:
        for g in "zrq":
            W, b = P["%sconv%s%s.weight" % (prefix, g, s)], P["%sconv%s%s.bias" % (prefix, g, s)]
            ctx[g + s] = F.conv2d(inp, W[:, C:C + n_ctx], b, padding=pad) if n_ctx else b[None, :, None, None]
    for s, pad in HALVES[cls]:
        W = lambda g: P["%sconv%s%s.weight" % (prefix, g, s)]
        part = lambda g, hh: F.conv2d(hh, W(g)[:, :C], None, padding=pad) + F.conv2d(rest, W(g)[:, C + n_ctx:], None, padding=pad) + ctx[g + s]
        pre_z, pre_r = part("z", h), part("r", h)
        r = sigmoid(pre_r)
        rh = r * h
        pre_q = part("q", rh)
        z, q = sigmoid(pre_z), torch.tanh(pre_q)
        if cap is not None:
            cap.update({"pre_z" + s: pre_z, "pre_r" + s: pre_r, "pre_q" + s: pre_q, "z" + s: z, "r" + s: r, "q" + s: q, "rh" + s: rh})
            if s != HALVES[cls][0][0]:
                cap["h_in" + s] = h
        h = (1 - z) * h + z * q
    return h


def block_formula(P, cls, net, inp, corr, flow, gru=gru_cat):
    """the update blocks as upstream composes them: motion encoder, GRU over cat([inp, motion]), flow head, 0.25 * mask head"""
    conv = lambda name, t, pad: F.conv2d(t, P[name + ".weight"], P[name + ".bias"], padding=pad)
    cor = F.relu(conv("encoder.convc1", corr, 0))
    if cls == "BasicUpdateBlock":
        cor = F.relu(conv("encoder.convc2", cor, 1))
    flo = F.relu(conv("encoder.convf2", F.relu(conv("encoder.convf1", flow, 3)), 1))
    motion = torch.cat([F.relu(conv("encoder.conv", torch.cat([cor, flo], dim=1), 1)), flow], dim=1)
    net = gru(P, "SepConvGRU" if cls == "BasicUpdateBlock" else "ConvGRU", net, torch.cat([inp, motion], dim=1), prefix="gru.")
    dflow = conv("flow_head.conv2", F.relu(conv("flow_head.conv1", net, 1)), 1)
    mask = 0.25 * conv("mask.2", F.relu(conv("mask.0", net, 1)), 0) if cls == "BasicUpdateBlock" else None
    return net, mask, dflow


def make_module(c, dev="cpu", **kw):
    """this repository's module for a case, its parameters the recorded ones (the maker's seeded draws, checked by their sum)"""
    from mpiflow_amd import raft_update as ru
    if "C" in c:
        m = getattr(ru, c["cls"])(hidden_dim=c["C"], input_dim=c["Cx"])
    else:
        m = getattr(ru, c["cls"])(types.SimpleNamespace(corr_levels=c["levels"], corr_radius=c["radius"]), **kw)
    total = _maker().fill_params(m, c["seed"])
    assert total == c["sums"][-1], "the seeded weights of %s are not the recorded ones" % c["name"]
    return m.to(dev)


def params_of(module, dtype, dev="cpu"):
    return {k: v.detach().clone().to(dtype).to(dev).requires_grad_(True) for k, v in module.state_dict().items()}


def run_gru_formula(c, form, dtype, dev="cpu", n_ctx=0):
    """every recorded array of a GRU case from a restatement: dict of tensors"""
    P = params_of(make_module(c), dtype, dev)
    t = lambda a: torch.from_numpy(a).to(dtype).to(dev)
    h, x = t(c["h"]).requires_grad_(True), t(c["x"]).requires_grad_(True)
    cap = {}
    out = form(P, c["cls"], h, x, cap=cap) if form is gru_cat else form(P, c["cls"], h, x, n_ctx=n_ctx, cap=cap)
    last = HALVES[c["cls"]][-1][0]
    keep = [cap["pre_%s%s" % (g, last)] for g in "zrq"] + [cap["rh" + last]]
    for k in keep:
        k.retain_grad()
    out.backward(t(c["cot"]))
    res = dict(h_out=out, grad_h=h.grad, grad_x=x.grad, d_pre_z=keep[0].grad, d_pre_r=keep[1].grad, d_pre_q=keep[2].grad, grad_rh=keep[3].grad)
    res.update({k: v for k, v in cap.items()})
    res.update({"grad_" + k: v.grad for k, v in P.items()})
    return {k: v.detach() for k, v in res.items()}


def run_block_formula(c, dtype, dev="cpu", gru=gru_cat):
    P = params_of(make_module(c), dtype, dev)
    t = lambda a: torch.from_numpy(a).to(dtype).to(dev)
    d = c["d"]
    net0, inp = t(d["net0"]).requires_grad_(True), t(d["inp"]).requires_grad_(True)
    return _block_loop(c, lambda net, i: block_formula(P, c["cls"], net, inp, t(d["corr_%d" % i]), t(d["flow_%d" % i]), gru=gru), net0, inp, P, t)


def _block_loop(c, step, net0, inp, P, t):
    d, net, loss, res = c["d"], net0, 0.0, {}
    for i in range(c["iters"]):
        net, mask, dflow = step(net, i)
        res["delta_flow_%d" % i] = dflow
        loss = loss + (dflow * t(d["cd_%d" % i])).sum()
        if c["cls"] == "BasicUpdateBlock":
            loss = loss + (mask * t(d["cm_%d" % i])).sum()
            res["mask_last"] = mask
        else:
            assert mask is None
    loss = loss + (net * t(d["cn"])).sum()
    loss.backward()
    res.update(net_out=net, grad_inp=inp.grad, grad_net0=net0.grad)
    res.update({"grad_" + k: v.grad for k, v in P.items()})
    return {k: v.detach() for k, v in res.items()}


def sample_err(c, key, value):
    s = c["rec"][key]
    v = value.double().cpu().numpy().reshape(-1)
    return float(np.abs(v[c["index"](v.size)] - s["f64"]).max())


# ---------------------------------------------------------------------------------------------------------------- host


def test_both_libraries_export_the_symbols(built):
    for path in (built.LIB_PATH, built.WITNESS_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for n in SYMBOLS + ("k_gru",):
            assert n in syms, (path, n)
    lib = built.load()
    for n in SYMBOLS:
        assert n in built.SIGNATURES and hasattr(lib, n)


def test_ctypes_structs_match_the_header(built, tmp_path):
    """ctypes mirror == the C structs: compare sizeof and every offsetof through gcc."""
    for struct in ("MpfGruTerm", "MpfGruArgs"):
        cls = getattr(built, struct)
        fields = [f[0] for f in cls._fields_]
        src, exe = tmp_path / (struct + ".c"), tmp_path / struct
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpiflow_hip.h"\nint main(void){printf("%%zu", sizeof(%s));\n' % struct
                       + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) + "return 0;}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert vals[0] == ctypes.sizeof(cls)
        assert vals[1:] == [getattr(cls, f).offset for f in fields]
    assert built.GRU_MAX_TERMS == 3 and "#define MPF_GRU_MAX_TERMS 3" in open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read()


def _args(built, **kw):
    a = built.MpfGruArgs()
    one = 256
    for arr in (a.z, a.r, a.q, a.dz, a.dr, a.dq):
        for t in arr:
            t.p, t.channels, t.offset = one, 384, 128
    a.h = a.g = a.out = a.dh = one
    a.nz = a.nr = a.nq = 3
    a.B, a.C, a.H, a.W = 2, 128, 36, 120
    for k, v in kw.items():
        if isinstance(v, tuple):                             # (array, index, field, value)
            setattr(getattr(a, k)[v[0]], v[1], v[2])
        else:
            setattr(a, k, v)
    return a


def test_c_abi_refuses_bad_arguments(built):
    """validated before anything is launched: no GPU is needed to be told so.  Status 10001 and a message that names the argument."""
    lib = built.load()
    fns = dict(reset=lib.mpf_gru_reset, update=lib.mpf_gru_update, ubwd=lib.mpf_gru_update_backward, rbwd=lib.mpf_gru_reset_backward)
    common = [(dict(h=None), b"(h)"), (dict(B=0), b"bad shape"), (dict(C=0), b"bad shape"), (dict(H=-1), b"bad shape"), (dict(W=0), b"bad shape"),
              (dict(B=1 << 12, H=1 << 10, W=1 << 10), b"2^31")]
    r_terms = [(dict(nr=4), b"1..3 terms"), (dict(nr=0), b"1..3 terms"), (dict(r=(1, "offset", 257)), b"exceeds"), (dict(r=(0, "offset", -1)), b"offset"),
               (dict(r=(2, "channels", 0)), b"channels"), (dict(nr=1, r=(0, "p", None)), b"every term of r")]
    zq_terms = [(dict(nz=4), b"1..3 terms"), (dict(nq=7), b"1..3 terms"), (dict(nq=-1), b"1..3 terms"), (dict(z=(0, "offset", 300)), b"exceeds"),
                (dict(q=(2, "offset", 257)), b"exceeds"), (dict(nz=1, z=(0, "p", None)), b"every term of z")]
    only = dict(reset=r_terms + [(dict(out=None), b"out")], update=zq_terms + [(dict(out=None), b"out")],
                ubwd=zq_terms + [(dict(g=None), b"(g)"), (dict(dh=None), b"(dh)"), (dict(dz=(0, "p", None)), b"dz[0]"), (dict(dq=(0, "p", None)), b"dq[0]"),
                                 (dict(dz=(1, "offset", 257)), b"exceeds"), (dict(dq=(0, "channels", 100)), b"exceeds")],
                rbwd=r_terms + [(dict(g=None), b"(g)"), (dict(dh=None), b"(dh)"), (dict(dr=(0, "p", None)), b"dr[0]"), (dict(dr=(1, "offset", 300)), b"exceeds")])
    for name, fn in fns.items():
        assert fn(None, None) == 10001 and b"null argument block" in lib.mpf_last_error()
        for kw, word in common + only[name]:
            assert fn(ctypes.byref(_args(built, **kw)), None) == 10001, (name, kw)
            assert word in lib.mpf_last_error(), (name, kw, lib.mpf_last_error())


def test_public_classes_refuse_what_they_cannot_take(built):
    from mpiflow_amd import raft_update as ru
    E = built.MpiFlowHipError
    gru = ru.SepConvGRU(hidden_dim=8, input_dim=12)
    h, x = torch.zeros(1, 8, 4, 6), torch.zeros(1, 12, 4, 6)
    for g in (gru, ru.ConvGRU(hidden_dim=8, input_dim=12)):
        with pytest.raises(E, match="no CPU path"):
            g(h, x)
        with pytest.raises(E, match="no CPU path"):
            g.context(torch.zeros(1, 5, 4, 6))
    for bad in (torch.float16, torch.bfloat16):
        with pytest.raises(E, match=r"h must be float32.*\.float\(\)"):
            gru(h.to(bad), x)
        with pytest.raises(E, match=r"x must be float32.*\.float\(\)"):
            gru(h, x.to(bad))
        with pytest.raises(E, match=r"inp must be float32.*\.float\(\)"):
            gru.context(torch.zeros(1, 5, 4, 6, dtype=bad))
    with pytest.raises(E, match="h must be float32"):
        gru(h.double(), x)
    for wrong in (torch.zeros(1, 7, 4, 6), torch.zeros(8, 4, 6)):
        with pytest.raises(E, match="h must be"):
            gru(wrong, x)
    for wrong in (torch.zeros(1, 11, 4, 6), torch.zeros(1, 12, 4, 7), torch.zeros(2, 12, 4, 6)):
        with pytest.raises(E, match="x must be"):
            gru(h, wrong)
    with pytest.raises(E, match="h must be contiguous"):
        gru(torch.zeros(1, 4, 6, 8).permute(0, 3, 1, 2), x)
    with pytest.raises(E, match="x must be contiguous"):
        gru(h, torch.zeros(1, 12, 6, 4).transpose(2, 3))
    with pytest.raises(E, match="fewer than input_dim"):
        gru.context(torch.zeros(1, 12, 4, 6))
    with pytest.raises(E, match="context must come from"):
        gru(h, x, context=torch.zeros(1))
    args = types.SimpleNamespace(corr_levels=4, corr_radius=4)
    blk = ru.BasicUpdateBlock(args)
    with pytest.raises(E, match="no CPU path"):
        blk(torch.zeros(1, 128, 4, 6), torch.zeros(1, 128, 4, 6), torch.zeros(1, 324, 4, 6), torch.zeros(1, 2, 4, 6))
    with pytest.raises(E, match=r"inp must be float32.*\.float\(\)"):
        blk(torch.zeros(1, 128, 4, 6), torch.zeros(1, 128, 4, 6).half(), torch.zeros(1, 324, 4, 6), torch.zeros(1, 2, 4, 6))


def test_state_dicts_equal_the_recorded_reference(built, golden):
    from mpiflow_amd import raft_update as ru
    a4, a3 = types.SimpleNamespace(corr_levels=4, corr_radius=4), types.SimpleNamespace(corr_levels=4, corr_radius=3)
    mods = dict(SepConvGRU=ru.SepConvGRU(hidden_dim=128, input_dim=256), ConvGRU=ru.ConvGRU(hidden_dim=96, input_dim=146),
                BasicUpdateBlock=ru.BasicUpdateBlock(a4, hidden_dim=128), SmallUpdateBlock=ru.SmallUpdateBlock(a3, hidden_dim=96))
    for name, m in mods.items():
        assert [str(s) for s in golden["mk"].state_list(m)] == golden["state"][name], name
        fake = {}
        for entry in golden["state"][name]:
            k, shape = entry.split(":")
            fake[k] = torch.full([int(s) for s in shape.split("x")], 0.5)
        m.load_state_dict(fake, strict=True)
        assert all(bool((v == 0.5).all()) for v in m.state_dict().values())


def test_formulas_equal_the_recorded_reference(golden):
    """the cat form, the split form and the split form with the hoisted context, in float64 == the reference's double run at the sampled
    entries to 1e-12 of the array's largest entry: every intermediate, h' and every gradient.  This ties the algebra of the split to the
    reference.  The blocks' restatement likewise."""
    for c in golden["gru"].values():
        forms = (("cat", gru_cat, 0), ("split", gru_split, 0), ("hoisted", gru_split, c["n_ctx"]))
        for what, form, n_ctx in forms:
            res = run_gru_formula(c, form, torch.float64, n_ctx=n_ctx)
            assert sorted(res) == sorted(c["keys"]), (c["name"], sorted(set(res) ^ set(c["keys"])))
            for key in c["keys"]:
                d = sample_err(c, key, res[key])
                assert d <= 1e-12 * c["rec"][key]["absmax"], (c["name"], what, key, d, c["rec"][key]["absmax"])
    for c in golden["block"].values():
        for gru in (gru_cat, lambda P, cls, h, x, prefix: gru_split(P, cls, h, x, n_ctx=x.shape[1] - (128 if cls == "SepConvGRU" else 82), prefix=prefix)):
            res = run_block_formula(c, torch.float64, gru=gru)
            assert sorted(res) == sorted(c["keys"])
            for key in c["keys"]:
                d = sample_err(c, key, res[key])
                assert d <= 1e-12 * c["rec"][key]["absmax"], (c["name"], key, d, c["rec"][key]["absmax"])


# ----------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(built):
    from mpiflow_amd import ops
    return ops


def fmt_bar(t):
    return 16 * EPS32 * max(1.0, float(t.abs().max()))


def kernel_formulas(h, pre_z, pre_r, pre_q, g_h, g_rh):
    """what the four kernels compute, in the dtype of the inputs"""
    z, r, q = sigmoid(pre_z), sigmoid(pre_r), torch.tanh(pre_q)
    return dict(rh=r * h, h_out=(1 - z) * h + z * q, d_pre_z=g_h * (q - h) * z * (1 - z), d_pre_q=g_h * z * (1 - q * q), dh_update=g_h * (1 - z),
                d_pre_r=g_rh * h * r * (1 - r), dh_reset=g_rh * r)


@pytest.mark.gpu
def test_gpu_kernels_alone_at_the_recorded_samples(golden, ops, dev):
    """the recorded pre-activations and h at the sampled entries, as [1,1,1,150] tensors: rh and h' of every half, d pre_z / d pre_q / d pre_r of
    the last half, each within 3 * err32 of the double run"""
    for c in golden["gru"].values():
        n = c["B"] * c["C"] * c["H"] * c["W"]
        idx = c["index"](n)
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(1, 1, 1, -1).to(dev)
        rec = lambda key: f32(c["rec"][key]["f64"])
        halves = [s for s, _ in HALVES[c["cls"]]]
        for k, s in enumerate(halves):
            h = f32(c["h"].reshape(-1)[idx]) if k == 0 else rec("h_in" + s)
            rh = ops.gru_reset(h, [(rec("pre_r" + s), 0)])
            hn = ops.gru_update(h, [(rec("pre_z" + s), 0)], [(rec("pre_q" + s), 0)])
            out_key = "h_out" if s == halves[-1] else "h_in" + halves[k + 1]
            got = [("rh" + s, rh), (out_key, hn)]
            if s == halves[-1]:
                dz, dq, dr = torch.empty_like(h), torch.empty_like(h), torch.empty_like(h)
                ops.gru_update_backward(f32(c["cot"].reshape(-1)[idx]), h, [(rec("pre_z" + s), 0)], [(rec("pre_q" + s), 0)], dz=[(dz, 0)], dq=[(dq, 0)])
                ops.gru_reset_backward(rec("grad_rh"), h, [(rec("pre_r" + s), 0)], dr=[(dr, 0)])
                got += [("d_pre_z", dz), ("d_pre_q", dq), ("d_pre_r", dr)]
            for key, val in got:
                s_ = c["rec"][key]
                d = float(np.abs(val.double().cpu().numpy().reshape(-1) - s_["f64"]).max())
                print("kernel %-26s %-8s |hip - ref64| at the samples %.2e = %.2f err32 (err32 %.2e)" % (c["name"], key, d, d / s_["err32"], s_["err32"]))
                assert d <= 3 * s_["err32"], (c["name"], key, d, s_["err32"])


def _layout(c, dev, seed, dtype=torch.float32):
    """seeded tensors in the modules' layout for a case's shape: hg [B,2C], xg [B,3C], cx [B,3C], qg [B,C], h, g_h, g_rh; each pre-activation is the
    sum of three N(0,1) terms, h = tanh(N(0,1))"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    rnd = lambda ch: torch.randn(B, ch, H, W, generator=gen, dtype=dtype).to(dev)
    return dict(hg=rnd(2 * C), xg=rnd(3 * C), cx=rnd(3 * C), qg=rnd(C), h=torch.tanh(rnd(C)), g_h=rnd(C), g_rh=rnd(C))


def _run_kernels(ops, t, C):
    """the four kernels on a _layout: three-term sums read as slices, gradients written to two destinations each"""
    z = [(t["hg"], 0), (t["xg"], 0), (t["cx"], 0)]
    r = [(t["hg"], C), (t["xg"], C), (t["cx"], C)]
    q = [(t["qg"], 0), (t["xg"], 2 * C), (t["cx"], 2 * C)]
    g3, g2, dq = torch.full_like(t["xg"], 7.0), torch.full_like(t["hg"], 7.0), torch.full_like(t["qg"], 7.0)
    out = dict(rh=ops.gru_reset(t["h"], r), h_out=ops.gru_update(t["h"], z, q))
    out["dh_update"] = ops.gru_update_backward(t["g_h"], t["h"], z, q, dz=[(g3, 0), (g2, 0)], dq=[(g3, 2 * C), (dq, 0)])
    out["dh_reset"] = ops.gru_reset_backward(t["g_rh"], t["h"], r, dr=[(g3, C), (g2, C)])
    acc = out["dh_update"].clone()
    assert ops.gru_reset_backward(t["g_rh"], t["h"], r, dr=[(g3, C), (g2, C)], dh=acc) is acc
    out.update(dh_sum=acc, g3=g3, g2=g2, dq=dq)
    return out


def _formula_of_layout(t, C):
    d = {k: v.double() for k, v in t.items()}
    pre = lambda gate: d["hg"][:, gate * C:(gate + 1) * C] + d["xg"][:, gate * C:(gate + 1) * C] + d["cx"][:, gate * C:(gate + 1) * C]
    return kernel_formulas(d["h"], pre(0), pre(1), d["qg"] + d["xg"][:, 2 * C:] + d["cx"][:, 2 * C:], d["g_h"], d["g_rh"])


@pytest.mark.gpu
def test_gpu_kernels_alone_at_every_entry(golden, ops, dev):
    """three-term sums read as channel slices, gradients written as slices to two destinations: every entry against the formulas in float64
    on the shapes of the 2 x 36 x 120 cases; rh, h' and the d pre within 3 * err32 of the case's recorded arrays, d h within FMT_BAR"""
    for name in ("SepConvGRU/real_2x36x120", "ConvGRU/real_2x36x120"):
        c = golden["gru"][name]
        C = c["C"]
        t = _layout(c, dev, c["seed"])
        got, want = _run_kernels(ops, t, C), _formula_of_layout(t, C)
        last = HALVES[c["cls"]][-1][0]
        g3, g2 = got["g3"], got["g2"]
        checks = [("rh", got["rh"], "rh" + last), ("h_out", got["h_out"], "h_out"), ("d_pre_z", g3[:, :C], "d_pre_z"), ("d_pre_r", g3[:, C:2 * C], "d_pre_r"),
                  ("d_pre_q", g3[:, 2 * C:], "d_pre_q"), ("dh_update", got["dh_update"], None), ("dh_reset", got["dh_reset"], None)]
        for key, val, rec_key in checks:
            d = float((val.double() - want[key]).abs().max())
            bar = 3 * c["rec"][rec_key]["err32"] if rec_key else fmt_bar(want[key])
            print("kernel %-26s %-10s every entry |hip - formula64| %.2e = %.2f of the bar %.2e" % (name, key, d, d / bar, bar))
            assert d <= bar, (name, key, d, bar)
        # the second destinations hold the same bits, and accumulate adds exactly one rounding
        assert torch.equal(g2[:, :C], g3[:, :C]) and torch.equal(g2[:, C:], g3[:, C:2 * C]) and torch.equal(got["dq"], g3[:, 2 * C:])
        assert torch.equal(got["dh_sum"], got["dh_update"] + got["dh_reset"])


def _gru_on_device(c, dev, with_context):
    gru = make_module(c, dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    h, cot = t(c["h"]).requires_grad_(True), t(c["cot"])
    if with_context:
        inp, rest = t(c["x"][:, :c["n_ctx"]].copy()).requires_grad_(True), t(c["x"][:, c["n_ctx"]:].copy()).requires_grad_(True)
        out = gru(h, rest, context=gru.context(inp))
        out.backward(cot)
        gx = torch.cat([inp.grad, rest.grad], dim=1)
    else:
        x = t(c["x"]).requires_grad_(True)
        out = gru(h, x)
        out.backward(cot)
        gx = x.grad
    res = dict(h_out=out.detach(), grad_h=h.grad, grad_x=gx)
    res.update({"grad_" + k: p.grad for k, p in gru.named_parameters()})
    return res


def check_module(c, what, got, cat32):
    worst = (0.0, 0.0)
    for key, val in got.items():
        s = c["rec"][key]
        d, dcat = sample_err(c, key, val), sample_err(c, key, cat32[key])
        bar = max(3 * s["err32"], 2 * dcat)
        worst = max(worst, (d / s["err32"], d / dcat if dcat else 0.0))
        print("module %-26s %-9s %-22s |hip - ref64| %.2e = %.2f err32 = %.2f x the cat form's %.2e" % (c["name"], what, key, d, d / s["err32"], d / dcat if dcat else 0.0, dcat))
        assert d <= bar, (c["name"], what, key, d, s["err32"], dcat)
    print("module %-26s %-9s worst: %.2f err32, %.2f x the cat form's error" % (c["name"], what, worst[0], worst[1]))


@pytest.mark.gpu
def test_gpu_grus_match_the_recorded_reference(golden, built, dev):
    for c in golden["gru"].values():
        cat32 = run_gru_formula(c, gru_cat, torch.float32, dev)
        for with_context in (False, True):
            check_module(c, "context" if with_context else "plain", _gru_on_device(c, dev, with_context), cat32)


def _block_on_device(c, dev, hoist):
    blk = make_module(c, dev, hoist_context=hoist)
    t = lambda a: torch.from_numpy(a).to(dev)
    d = c["d"]
    net0, inp = t(d["net0"]).requires_grad_(True), t(d["inp"]).requires_grad_(True)
    res = _block_loop(c, lambda net, i: blk(net, inp, t(d["corr_%d" % i]), t(d["flow_%d" % i])), net0, inp, dict(blk.named_parameters()), t)
    return res, blk


@pytest.mark.gpu
def test_gpu_update_blocks_match_the_recorded_reference(golden, built, dev):
    for c in golden["block"].values():
        cat32 = run_block_formula(c, torch.float32, dev)
        for hoist in (True, False):
            got, blk = _block_on_device(c, dev, hoist)
            assert blk.context_computed == (1 if hoist else c["iters"])
            check_module(c, "hoisted" if hoist else "unhoisted", got, cat32)


@pytest.mark.gpu
def test_gpu_checkpoint_loads_strictly(golden, built, dev):
    """a dict shaped like the reference's state_dict loads with strict=True, and the loaded module computes with those weights"""
    c = golden["gru"]["SepConvGRU/tiny_1x4x6"]
    from mpiflow_amd import raft_update as ru
    src = make_module(c, dev)
    ckpt = {k: v.detach().cpu().clone() for k, v in src.state_dict().items()}
    assert ["%s:%s" % (k, "x".join(str(s) for s in v.shape)) for k, v in ckpt.items()] == [str(s) for s in golden["mk"].state_list(src)]
    dst = ru.SepConvGRU(hidden_dim=c["C"], input_dim=c["Cx"]).to(dev)
    missing = dst.load_state_dict(ckpt, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    h, x = torch.from_numpy(c["h"]).to(dev), torch.from_numpy(c["x"]).to(dev)
    with torch.no_grad():
        assert torch.equal(dst(h, x), src(h, x))
    for cls, a in (("BasicUpdateBlock", types.SimpleNamespace(corr_levels=4, corr_radius=4)), ("SmallUpdateBlock", types.SimpleNamespace(corr_levels=4, corr_radius=3))):
        fake = {}
        for entry in golden["state"][cls]:
            k, shape = entry.split(":")
            fake[k] = torch.zeros([int(s) for s in shape.split("x")])
        getattr(ru, cls)(a).to(dev).load_state_dict(fake, strict=True)


@pytest.mark.gpu
def test_gpu_memory_is_below_the_cat_form(built, dev):
    """forward + backward of 12 chained SepConvGRU calls at 8 x 36 x 120, C = 128: peak memory above the inputs, fused against the cat form"""
    from mpiflow_amd import raft_update as ru
    torch.manual_seed(5)
    gru = ru.SepConvGRU(128, 256).to(dev)
    P = {k: v for k, v in gru.named_parameters()}
    h0, x = torch.tanh(torch.randn(8, 128, 36, 120, device=dev)), torch.relu(torch.randn(8, 256, 36, 120, device=dev))
    peak = {}
    for what, step in (("cat", lambda h: gru_cat(P, "SepConvGRU", h, x)), ("fused", lambda h: gru(h, x))):
        for rep in range(2):                                  # the first pass warms MIOpen's workspaces and the allocator
            gru.zero_grad(set_to_none=True)
            h = h0.clone().requires_grad_(True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            out = h
            for _ in range(12):
                out = step(out)
            out.sum().backward()
            torch.cuda.synchronize()
            peak[what] = torch.cuda.max_memory_allocated(dev) - before
            del out, h
    print("12 chained SepConvGRU calls at 8x36x120, forward + backward: peak above the inputs %.1f MB fused, %.1f MB cat form, ratio %.3f"
          % (peak["fused"] / 1e6, peak["cat"] / 1e6, peak["fused"] / peak["cat"]))
    assert peak["fused"] < peak["cat"]


def _snap(obj):
    """a copy of a kernel call's arguments: tensors cloned, lists and (tensor, offset) pairs rebuilt"""
    if isinstance(obj, torch.Tensor):
        return obj.detach().clone()
    if isinstance(obj, (list, tuple)):
        return type(obj)(_snap(o) for o in obj)
    if isinstance(obj, dict):
        return {k: _snap(v) for k, v in obj.items()}
    return obj


@pytest.mark.gpu
def test_gpu_two_runs_are_bit_identical(golden, ops, dev, monkeypatch):
    """a full forward + backward of the basic block over three iterations: every one of its 24 kernel calls is captured where the module makes
    it - arguments as they were before the call, outputs as they were after it - and run a second time on those arguments: the return value
    and every gradient slice written are bit-identical.  (The convolutions between the kernels are MIOpen's; whether two whole passes agree to
    the bit is theirs to decide and is printed, not asserted.)"""
    c = golden["block"]["BasicUpdateBlock/2x10x14"]
    calls = []
    for fn in ("gru_reset", "gru_update", "gru_update_backward", "gru_reset_backward"):
        def spy(*a, _f=getattr(ops, fn), **kw):
            before = (_snap(a), _snap(kw))
            out = _f(*a, **kw)
            calls.append((_f, before, _snap(out), _snap({k: kw[k] for k in ("dz", "dq", "dr") if k in kw})))
            return out
        monkeypatch.setattr(ops, fn, spy)
    first, _ = _block_on_device(c, dev, True)
    monkeypatch.undo()
    assert len(calls) == 3 * 2 * 4
    written = 0
    for f, (a, kw), out, dests in calls:
        again = f(*a, **kw)                                              # kw holds its own copies of the destinations, as they were before
        assert torch.equal(again, out), f.__name__
        C = out.shape[1]
        for k, pairs in dests.items():
            for (t1, off), (t2, _) in zip(pairs, kw[k]):
                assert torch.equal(t1[:, off:off + C], t2[:, off:off + C]), (f.__name__, k)
                written += 1
    assert written == 3 * 2 * (4 + 2)
    second, _ = _block_on_device(c, dev, True)
    same = all(torch.equal(first[k], second[k]) for k in first)
    print("two whole passes of the basic block (MIOpen convolutions included) bit-identical: %s" % same)


@pytest.mark.gpu
def test_gpu_context_cache(golden, built, dev):
    c = golden["block"]["SmallUpdateBlock/2x9x7"]
    blk = make_module(c, dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    d = c["d"]
    net, inp, corr, flow = t(d["net0"]), t(d["inp"]), t(d["corr_0"]), t(d["flow_0"])
    with torch.no_grad():
        a = blk(net, inp, corr, flow)[0]
        b = blk(net, inp, corr, flow)[0]
        close = lambda u, v: float((u - v).abs().max()) <= 1e-5          # MIOpen's convolutions are not bit-reproducible from call to call
        assert blk.context_computed == 1 and close(a, b)                 # the same object: reused
        blk(net, inp.clone(), corr, flow)
        assert blk.context_computed == 2                                 # another tensor: recomputed
        blk(net, inp, corr, flow)
        assert blk.context_computed == 3
        inp.mul_(2.0)                                                    # changed in place: recomputed, and the result follows the new values
        e = blk(net, inp, corr, flow)[0]
        assert blk.context_computed == 4 and float((e - a).abs().max()) > 1e-2
        fresh = make_module(c, dev, hoist_context=False)
        assert close(e, fresh(net, inp, corr, flow)[0]) and fresh.context_computed == 1 and fresh._cache is None
        blk(net, inp, corr, flow)
        assert blk.context_computed == 4
        blk.reset()
        assert blk._cache is None
        blk(net, inp, corr, flow)
        assert blk.context_computed == 5
        with torch.enable_grad():                                        # a context computed without a graph is not reused where one is needed
            blk(net, inp, corr, flow)
        assert blk.context_computed == 6
        for p in blk.gru.parameters():                                   # an optimizer step: the weights changed in place
            p.mul_(1.0)
        blk(net, inp, corr, flow)
        assert blk.context_computed == 7
        tmp = inp.clone()
        blk(net, tmp, corr, flow)
        assert blk._cache is not None
        del tmp                                                          # the cache does not keep inp alive, and empties itself when it dies
        assert blk._cache is None
    # gradients with respect to inp: cached against uncached, within the module bar (both are compared with the double run)
    cat32 = run_block_formula(c, torch.float32, dev)
    for hoist in (True, False):
        got, _ = _block_on_device(c, dev, hoist)
        check_module(c, "inp grad", dict(grad_inp=got["grad_inp"]), cat32)


@pytest.mark.gpu
def test_gpu_nan_stays_where_torch_puts_it(golden, ops, dev):
    """a NaN planted in h or in one term of a pre-activation: every kernel output is NaN exactly where the float64 formula on the same inputs
    is, and keeps its bits everywhere else"""
    c = golden["gru"]["SepConvGRU/odd_2x5x7"]
    C = c["C"]
    clean = _run_kernels(ops, _layout(c, dev, 77), C)
    for where, pos in (("h", (1, 2, 3, 4)), ("xg", (0, C + 1, 2, 2)), ("cx", (1, 1, 0, 6)), ("qg", (0, 3, 4, 0)), ("hg", (1, C + 4, 1, 1)), ("g_rh", (0, 0, 0, 0))):
        t = _layout(c, dev, 77)
        t[where][pos] = float("nan")
        got, want = _run_kernels(ops, t, C), _formula_of_layout(t, C)
        g3 = got["g3"]
        pairs = [("rh", got["rh"], clean["rh"]), ("h_out", got["h_out"], clean["h_out"]), ("d_pre_z", g3[:, :C], clean["g3"][:, :C]),
                 ("d_pre_r", g3[:, C:2 * C], clean["g3"][:, C:2 * C]), ("d_pre_q", g3[:, 2 * C:], clean["g3"][:, 2 * C:]),
                 ("dh_update", got["dh_update"], clean["dh_update"]), ("dh_reset", got["dh_reset"], clean["dh_reset"])]
        hit = 0
        for key, val, ok in pairs:
            bad = torch.isnan(val)
            assert torch.equal(bad, torch.isnan(want[key])), (where, key)
            assert torch.equal(val[~bad], ok[~bad]), (where, key)
            hit += int(bad.sum())
        assert 1 <= hit <= 7, (where, hit)
    t = _layout(c, dev, 77)
    t["xg"][0, 0, 0, 0], t["xg"][0, 2 * C, 0, 1], t["h"][0, 0, 0, 2] = float("inf"), float("-inf"), float("inf")
    got, want = _run_kernels(ops, t, C), _formula_of_layout(t, C)
    for key in ("rh", "h_out", "dh_update", "dh_reset"):
        assert torch.equal(torch.isnan(got[key]), torch.isnan(want[key])), key
        fin = torch.isfinite(want[key])
        assert torch.equal(torch.isfinite(got[key]), fin) and float((got[key][fin].double() - want[key][fin]).abs().max()) <= fmt_bar(want[key][fin])


@pytest.mark.gpu
def test_gpu_side_stream_and_interleaved_streams(golden, built, dev):
    ca, cb = golden["gru"]["SepConvGRU/odd_2x5x7"], golden["gru"]["ConvGRU/h1_2x1x72"]
    mods = {c["name"]: make_module(c, dev) for c in (ca, cb)}

    def forward(c):
        t = lambda a: torch.from_numpy(a).to(dev)
        h, x = t(c["h"]).requires_grad_(True), t(c["x"]).requires_grad_(True)
        return h, x, mods[c["name"]](h, x), t(c["cot"])

    def run(c):
        h, x, out, cot = forward(c)
        out.backward(cot)
        return [out.detach(), h.grad, x.grad]

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
    state, got = {}, {}
    for c, s in ((ca, s1), (cb, s2)):                                    # forward of each, then backward of each
        with torch.cuda.stream(s):
            state[c["name"]] = forward(c)
    for c, s in ((ca, s1), (cb, s2)):
        with torch.cuda.stream(s):
            h, x, out, cot = state[c["name"]]
            out.backward(cot)
            got[c["name"]] = [out.detach(), h.grad, x.grad]
    s1.synchronize()
    s2.synchronize()
    busy.synchronize()
    for c in (ca, cb):
        for a, b in zip(got[c["name"]], alone[c["name"]]):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_gpu_odd_sizes_take_the_scalar_path(golden, ops, dev):
    """H*W = 35: 4-byte accesses.  Every entry within FMT_BAR of the float64 formula (three-term slices, two destinations), and - the op being
    pointwise - the same bits as the 16-byte path gives for the same values laid out with H*W = 140; a slice whose pointer is not 16-byte aligned
    (an odd channel offset at H*W = 6) takes the scalar path as well"""
    c = golden["gru"]["SepConvGRU/odd_2x5x7"]
    assert (c["H"] * c["W"]) % 4 != 0
    C = c["C"]
    t = _layout(c, dev, 31)
    got, want = _run_kernels(ops, t, C), _formula_of_layout(t, C)
    g3 = got["g3"]
    for key, val in (("rh", got["rh"]), ("h_out", got["h_out"]), ("d_pre_z", g3[:, :C]), ("d_pre_r", g3[:, C:2 * C]), ("d_pre_q", g3[:, 2 * C:]),
                     ("dh_update", got["dh_update"]), ("dh_reset", got["dh_reset"])):
        d = float((val.double() - want[key]).abs().max())
        print("scalar path %-10s every entry |hip - formula64| %.2e = %.2f of FMT_BAR" % (key, d, d / fmt_bar(want[key])))
        assert d <= fmt_bar(want[key]), (key, d)
    assert torch.equal(got["g2"][:, :C], g3[:, :C]) and torch.equal(got["dq"], g3[:, 2 * C:])
    gen = torch.Generator(device="cpu").manual_seed(8)
    flat = [torch.randn(420, generator=gen).to(dev) for _ in range(4)]
    outs = []
    for shape in ((2, 6, 5, 7), (1, 3, 4, 35)):
        h, pz, pq, g = [f.reshape(shape).contiguous() for f in flat]
        dz, dq, dr = torch.empty_like(h), torch.empty_like(h), torch.empty_like(h)
        o = [ops.gru_reset(h, [(pz, 0)]), ops.gru_update(h, [(pz, 0)], [(pq, 0)]), ops.gru_update_backward(g, h, [(pz, 0)], [(pq, 0)], dz=[(dz, 0)], dq=[(dq, 0)]),
             ops.gru_reset_backward(g, h, [(pz, 0)], dr=[(dr, 0)]), dz, dq, dr]
        outs.append([v.reshape(-1) for v in o])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    h, src = torch.randn(2, 1, 2, 3, device=dev), torch.randn(2, 4, 2, 3, device=dev)      # offset 1: the slice starts 24 bytes into the tensor
    assert torch.equal(ops.gru_reset(h, [(src, 1)]), ops.gru_reset(h, [(src[:, 1:2].contiguous(), 0)]))
    from mpiflow_amd._lib import MpiFlowHipError
    with pytest.raises(MpiFlowHipError, match="takes 1..3 slices"):
        ops.gru_reset(h, [(src, 0)] * 4)
    with pytest.raises(MpiFlowHipError, match="not inside"):
        ops.gru_reset(h, [(src, 4)])
