"""RAFT's encoders with the norm / ReLU / shortcut / ReLU chain fused (mpiflow_amd/raft_extractor.py; mpf_norm_stats, mpf_norm_act and the two
backward calls of mpf_norm.hip).

The reference is the reference's own extractor.py and the torch.nn.functional chain its modules call, recorded on the CPU by
tests/golden/make_extractor_golden.py into tests/golden/raft_extractor.npz: per array up to 150 sampled entries of the DOUBLE run, err32 =
max |fp32 run - double run| over the whole array, and max |ref64|.  Inputs and weights are rebuilt from seeds (their float64 sums are checked).
A missing golden fails these tests; it does not skip them.

Bars.  Kernels alone: 3 * err32 of the recorded array they produce (the bar of tests/test_raft_corr.py, test_raft_upsample.py and
test_raft_update.py), at the samples against the recorded double run and at every entry against the formulas below in numpy float64.  The
identity shortcut's gradient is a masked copy of the cotangent: err32 = 0, so the bar asks for equality.
Modules and encoders: the convolutions are MIOpen's, so per array the bar is the larger of 3 * err32 and 2 x the error that the same
state_dict, loaded with strict=True into a second instance whose forward calls its torch.nn submodules the plain way (norm module, F.relu,
add, F.relu) on the same device, makes against the same double run.  The running statistics of a training pass: 3 * err32.
The float64 formulas against the recorded double run: 1e-11 * max(1, max |ref64|) (2^-53, sums over at most 4160 entries of magnitude <= 10).

Figures, once measured on an MI355X: profiles/extractor/README.md."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "raft_extractor.npz")
SYMBOLS = ("mpf_norm_stats", "mpf_norm_act", "mpf_norm_act_backward_reduce", "mpf_norm_act_backward")
EPS = 1e-5


def _maker():
    spec = importlib.util.spec_from_file_location("make_extractor_golden", os.path.join(ROOT, "tests", "golden", "make_extractor_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


def _records(z, prefix):
    keys = [str(k) for k in z[prefix + "keys"]]
    return {k: dict(f64=z[prefix + k + "_f64"], err32=float(z[prefix + k + "_err32"]), absmax=float(z[prefix + k + "_absmax"])) for k in keys}


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN, allow_pickle=False)                  # a missing file is an error here, not a skip
    mk = _maker()
    g = dict(mk=mk, z=z, op={}, enc={}, inputs={})
    for name, N, C, H, W, norm, groups, seed in mk.OP_CASES:
        d = mk.op_inputs(N, C, H, W, norm, seed)
        assert np.array_equal(np.array([d[k].astype(np.float64).sum() for k in sorted(d)]), z["op/%s/input_sums" % name]), "the seeded inputs of %s are not the recorded ones" % name
        g["inputs"][name] = d
        for mode in mk.op_modes(norm):
            for variant in mk.VARIANTS:
                key = "op/%s/%s/%s" % (name, mode, variant)
                g["op"][key] = dict(name=key, case=name, mode=mode, variant=variant, groups=groups, seed=seed, d=d, rec=_records(z, key + "/"))
    assert sorted(g["op"]) == sorted(str(n) for n in z["op_names"]) and len(g["op"]) == 24
    for name, cls, fn, out_dim, batches, N, H, W, training, seed in mk.ENCODER_CASES:
        images, cot = mk.encoder_inputs(batches, N, H, W, out_dim, seed)
        c = dict(name=name, cls=cls, fn=fn, out_dim=out_dim, training=training, seed=seed, images=images, cot=cot, sums=z[name + "/input_sums"], rec=_records(z, name + "/"))
        assert sum(im.astype(np.float64).sum() for im in images) == c["sums"][0] and cot.astype(np.float64).sum() == c["sums"][1], name
        g["enc"][name] = c
    assert sorted(g["enc"]) == sorted(str(n) for n in z["encoder_names"]) and len(g["enc"]) == 6
    return g


def sample_err(c, key, value):
    s = c["rec"][key]
    v = np.asarray(value, dtype=np.float64).reshape(-1)
    return float(np.abs(v[_maker_index(v.size, c["seed"])] - s["f64"]).max())


def _maker_index(n, seed, _mk=[]):
    if not _mk:
        _mk.append(_maker())
    return _mk[0].sample_index(n, seed)


# ---------------------------------------------------------------------------------------- the formulas, restated (not code under test)


def set_mean(a, mode, groups):
    """the mean of `a` over every statistic set, broadcast back to a's shape"""
    N, C, H, W = a.shape
    if mode == "instance":
        return np.broadcast_to(a.mean(axis=(2, 3), keepdims=True), a.shape)
    if mode == "batch_train":
        return np.broadcast_to(a.mean(axis=(0, 2, 3), keepdims=True), a.shape)
    return np.broadcast_to(a.reshape(N, groups, -1).mean(axis=2)[:, :, None], (N, groups, (C // groups) * H * W)).reshape(a.shape)


def np_norm(d, p, mode, groups):
    """(normalised value, xhat, rstd, w, statistics) of the term with prefix p ('' or 'r'), float64"""
    x = d[("x" if p == "" else "rx")].astype(np.float64)
    C = x.shape[1]
    affine = mode != "instance"
    w = d[p + "weight"].astype(np.float64).reshape(1, C, 1, 1) if affine else np.ones((1, C, 1, 1))
    b = d[p + "bias"].astype(np.float64).reshape(1, C, 1, 1) if affine else np.zeros((1, C, 1, 1))
    if mode == "batch_eval":
        mean, var = (d[p + k].astype(np.float64).reshape(1, C, 1, 1) for k in ("running_mean", "running_var"))
    else:
        mean = set_mean(x, mode, groups)
        var = set_mean((x - mean) ** 2, mode, groups)
    rstd = 1.0 / np.sqrt(var + EPS)
    xhat = (x - mean) * rstd
    return xhat * w + b, xhat, rstd, w, (mean, var)


def np_norm_backward(dv, xhat, rstd, w, mode, groups):
    """(dx, dweight, dbias) from the cotangent dv of the normalised value"""
    dw, db = (dv * xhat).sum(axis=(0, 2, 3)), dv.sum(axis=(0, 2, 3))
    dxhat = dv * w
    if mode == "batch_eval":
        return dxhat * rstd, dw, db
    return rstd * (dxhat - set_mean(dxhat, mode, groups) - xhat * set_mean(dxhat * xhat, mode, groups)), dw, db


def np_chain(d, mode, groups, variant):
    """every recorded array of an op-level case in numpy float64"""
    v, xhat, rstd, w, (mean, var) = np_norm(d, "", mode, groups)
    y = np.where(v < 0, 0.0, v)
    g = d["cot"].astype(np.float64)
    res = {}
    if variant == "plain":
        out, g2 = y, g
    else:
        if variant == "res":
            r = d["res"].astype(np.float64)
        else:
            r, rxhat, rrstd, rw, (rmean, rvar) = np_norm(d, "r", mode, groups)
        s = r + y
        out, g2 = np.where(s < 0, 0.0, s), np.where(s <= 0, 0.0, g)
        if variant == "res":
            res["grad_res"] = g2
        else:
            res["grad_rx"], res["grad_rweight"], res["grad_rbias"] = np_norm_backward(g2, rxhat, rrstd, rw, mode, groups)
    res["out"] = out
    res["grad_x"], res["grad_weight"], res["grad_bias"] = np_norm_backward(np.where(v <= 0, 0.0, g2), xhat, rstd, w, mode, groups)
    if mode == "instance":
        res = {k: a for k, a in res.items() if not k.endswith(("weight", "bias"))}
    if mode == "batch_train":
        m = v.size // v.shape[1]
        stats = [("", mean, var)] + ([("r", rmean, rvar)] if variant == "rterm" else [])
        for p, mu, va in stats:
            res[p + "running_mean_new"] = 0.9 * d[p + "running_mean"].astype(np.float64) + 0.1 * mu[0, :, 0, 0]
            res[p + "running_var_new"] = 0.9 * d[p + "running_var"].astype(np.float64) + 0.1 * va[0, :, 0, 0] * (m / (m - 1.0))
    return res


def plain_block(blk, x):
    """a block of mpiflow_amd.raft_extractor computed the plain way: its torch.nn submodules called one after the other, the ReLUs in place as upstream's"""
    y = F.relu(blk.norm1(blk.conv1(x)), inplace=True)
    y = F.relu(blk.norm2(blk.conv2(y)), inplace=True)
    if hasattr(blk, "conv3"):
        y = F.relu(blk.norm3(blk.conv3(y)), inplace=True)
    if blk.downsample is not None:
        x = blk.downsample(x)
    return F.relu(x + y, inplace=True)


def plain_encoder(enc, x):
    is_list = isinstance(x, (list, tuple))
    if is_list:
        n = x[0].shape[0]
        x = torch.cat(x, dim=0)
    x = F.relu(enc.norm1(enc.conv1(x)), inplace=True)
    for layer in (enc.layer1, enc.layer2, enc.layer3):
        for blk in layer:
            x = plain_block(blk, x)
    x = enc.conv2(x)
    return torch.split(x, [n, n], dim=0) if is_list else x


def make_encoder(c, golden, plain_from=None):
    """this repository's encoder for a case with the recorded (seeded, sum-checked) parameters; with plain_from, a second instance that loads
    the first's state_dict with strict=True and whose forward is the plain torch form"""
    from mpiflow_amd import raft_extractor as rx
    enc = getattr(rx, c["cls"])(output_dim=c["out_dim"], norm_fn=c["fn"], dropout=0.0)
    if plain_from is None:
        assert golden["mk"].fill_params(enc, c["seed"]) == c["sums"][2], "the seeded weights of %s are not the recorded ones" % c["name"]
        return enc
    ckpt = {k: v.detach().cpu().clone() for k, v in plain_from.state_dict().items()}
    missing = enc.load_state_dict(ckpt, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    enc.forward = lambda x: plain_encoder(enc, x)
    return enc


# ---------------------------------------------------------------------------------------------------------------- host


def test_both_libraries_export_the_symbols(built):
    for path in (built.LIB_PATH, built.WITNESS_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for n in SYMBOLS + ("k_norm_stats", "k_norm_act", "k_norm_bwd_reduce", "k_norm_bwd"):
            assert n in syms, (path, n)
    lib = built.load()
    for n in SYMBOLS:
        assert n in built.SIGNATURES and hasattr(lib, n)


def test_ctypes_structs_match_the_header(built, tmp_path):
    """ctypes mirror == the C structs: compare sizeof and every offsetof through gcc."""
    for struct in ("MpfNormTerm", "MpfNormArgs"):
        cls = getattr(built, struct)
        fields = [f[0] for f in cls._fields_]
        src, exe = tmp_path / (struct + ".c"), tmp_path / struct
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpiflow_hip.h"\nint main(void){printf("%%zu", sizeof(%s));\n' % struct
                       + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) + "return 0;}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert vals[0] == ctypes.sizeof(cls)
        assert vals[1:] == [getattr(cls, f).offset for f in fields]
    hdr = open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read()
    for k, name in enumerate(("NONE", "INSTANCE", "BATCH_TRAIN", "BATCH_EVAL", "GROUP")):
        assert "#define MPF_NORM_%s %d\n" % (name, k) in hdr and getattr(built, "NORM_" + name) == k
    assert "#define MPF_NORM_MAX_CHUNKS %d\n" % built.NORM_MAX_CHUNKS in hdr


def _args(built, **kw):
    a = built.MpfNormArgs()
    one = 256
    for t in (a.y, a.r):
        for f, _ in built.MpfNormTerm._fields_[:13]:
            setattr(t, f, one)
        t.mode, t.groups = built.NORM_GROUP, 8
    a.out = a.g = a.dres = one
    a.res = None
    a.chunks = 2
    a.N, a.C, a.H, a.W = 2, 64, 16, 24
    for k, v in kw.items():
        if isinstance(v, tuple):                             # (term, field, value)
            setattr(getattr(a, v[0]), v[1], v[2])
        else:
            setattr(a, k, v)
    return a


def test_c_abi_refuses_bad_arguments(built):
    """validated before anything is launched: no GPU is needed to be told so.  Status 10001 and a message that names the argument."""
    lib = built.load()
    fns = dict(stats=lib.mpf_norm_stats, act=lib.mpf_norm_act, reduce=lib.mpf_norm_act_backward_reduce, bwd=lib.mpf_norm_act_backward)
    common = [(dict(N=0), b"bad shape"), (dict(C=-1), b"bad shape"), (dict(H=0), b"bad shape"), (dict(W=0), b"bad shape"), (dict(chunks=0), b"chunks must be"),
              (dict(chunks=-3), b"chunks must be"), (dict(chunks=1025), b"chunks must be"), (dict(N=1 << 12, H=1 << 10, W=1 << 10), b"2^31"),
              (dict(a=("y", "x", None)), b"(y.x)"), (dict(a=("y", "mode", 5)), b"y.mode"), (dict(a=("r", "mode", -1)), b"r.mode"),
              (dict(a=("y", "groups", 7)), b"y.groups must divide"), (dict(a=("r", "groups", 0)), b"r.groups must divide"), (dict(res=256), b"not both"),
              (dict(a=("y", "mode", 3), b=("y", "running_var", None)), b"running_mean / running_var")]
    only = dict(stats=[(dict(a=("y", "partials", None)), b"y.partials"), (dict(a=("y", "mode", 0), b=("r", "mode", 3)), b"no term has a mode with statistics")],
                act=[(dict(out=None), b"(out)"), (dict(a=("r", "partials", None)), b"r.partials"), (dict(a=("y", "mean", None)), b"y.mean / rstd"),
                     (dict(a=("y", "mode", 2), b=("y", "rstd", None)), b"y.mean / rstd")],
                reduce=[(dict(g=None), b"(g)"), (dict(a=("y", "grad_partials", None)), b"y.grad_partials"), (dict(a=("r", "mean", None)), b"r.mean / rstd")],
                bwd=[(dict(g=None), b"(g)"), (dict(a=("y", "dx", None)), b"y.dx"), (dict(a=("r", "dx", None)), b"r.dx"), (dict(a=("r", "grad_partials", None)), b"r.grad_partials"),
                     (dict(a=("r", "x", None), res=256, dres=None), b"(dres)"), (dict(a=("y", "mode", 3), b=("y", "grad_partials", None)), b"y.grad_partials")])
    for name, fn in fns.items():
        assert fn(None, None) == 10001 and b"null argument block" in lib.mpf_last_error()
        for kw, word in common + only[name]:
            assert fn(ctypes.byref(_args(built, **kw)), None) == 10001, (name, kw)
            assert word in lib.mpf_last_error(), (name, kw, lib.mpf_last_error())


def test_public_classes_refuse_what_they_cannot_take(built):
    from mpiflow_amd import ops, raft_extractor as rx
    E = built.MpiFlowHipError
    img = torch.zeros(1, 3, 32, 48)
    for enc in (rx.BasicEncoder(128, "instance"), rx.SmallEncoder(128, "batch"), rx.BasicEncoder(64, "none")):
        with pytest.raises(E, match="no CPU path"):
            enc(img)
        with pytest.raises(E, match="no CPU path"):
            enc([img, img])
        for bad in (torch.float16, torch.bfloat16, torch.float64):
            with pytest.raises(E, match=r"x must be float32.*\.float\(\)"):
                enc(img.to(bad))
            with pytest.raises(E, match=r"x\[1\] must be float32.*\.float\(\)"):
                enc((img, img.to(bad)))
        with pytest.raises(E, match="two image batches"):
            enc([img, img, img])
        with pytest.raises(E, match="share shape and device"):
            enc([img, torch.zeros(2, 3, 32, 48)])
        with pytest.raises(E, match="3 channels"):
            enc(torch.zeros(1, 4, 32, 48))
        with pytest.raises(E, match=r"must be \[N,C,H,W\]"):
            enc(torch.zeros(3, 32, 48))
        with pytest.raises(E, match="must be a torch.Tensor"):
            enc(np.zeros((1, 3, 32, 48), np.float32))
    for blk in (rx.ResidualBlock(8, 16, "group", stride=2), rx.BottleneckBlock(8, 16, "instance")):
        with pytest.raises(E, match="no CPU path"):
            blk(torch.zeros(1, 8, 6, 6))
        with pytest.raises(E, match=r"x must be float32.*\.float\(\)"):
            blk(torch.zeros(1, 8, 6, 6).half())
        with pytest.raises(E, match="x must have 8 channels"):
            blk(torch.zeros(1, 7, 6, 6))
    with pytest.raises(E, match="norm_fn must be one of"):
        rx.ResidualBlock(8, 8, "layer")
    with pytest.raises(E, match="norm_fn must be one of"):
        rx.BasicEncoder(128, "Batch")
    # a single value per statistic set: torch raises for it too
    with pytest.raises(ValueError):
        F.instance_norm(torch.zeros(1, 8, 1, 1))
    with pytest.raises(ValueError):
        nn.BatchNorm2d(8)(torch.zeros(1, 8, 1, 1))
    with pytest.raises(E, match="norm1 would take 'instance' statistics over a single value"):
        rx.ResidualBlock(8, 8, "instance", stride=2)(torch.zeros(2, 8, 2, 2))
    with pytest.raises(E, match="norm1 would take 'batch_train' statistics over a single value"):
        rx.ResidualBlock(8, 8, "batch", stride=2)(torch.zeros(1, 8, 2, 2))
    with pytest.raises(E, match="statistics over a single value"):
        rx.BasicEncoder(128, "instance")(torch.zeros(1, 3, 8, 8))                  # 1 x 1 at 1/8 resolution
    with pytest.raises(E, match="no CPU path"):                                     # eval mode: running statistics, nothing to refuse but the device
        rx.ResidualBlock(8, 8, "batch", stride=2).eval()(torch.zeros(1, 8, 2, 2))
    with pytest.raises(E, match="no CPU path"):
        rx.ResidualBlock(8, 8, "batch", stride=2)(torch.zeros(2, 8, 2, 2))
    x = torch.zeros(2, 8, 4, 6)
    with pytest.raises(E, match="no CPU path"):
        ops.norm_act(ops.NormTerm(x, "instance"))
    with pytest.raises(E, match="mode must be one of"):
        ops.norm_act(ops.NormTerm(x, "layer"))
    with pytest.raises(E, match="groups must divide"):
        ops.norm_act(ops.NormTerm(x, "group", groups=3))
    with pytest.raises(E, match="needs running_mean and running_var"):
        ops.norm_act(ops.NormTerm(x, "batch_eval"))
    with pytest.raises(E, match=r"weight must be a contiguous float32 tensor \[8\]"):
        ops.norm_act(ops.NormTerm(x, "group", weight=torch.zeros(7), groups=2))
    with pytest.raises(E, match="statistics over a single value"):
        ops.norm_act(ops.NormTerm(torch.zeros(2, 8, 1, 1), "instance"))
    with pytest.raises(E, match="has no statistics"):
        ops.norm_stats(x, "none")
    with pytest.raises(E, match="chunks must be an integer"):
        ops.norm_act(ops.NormTerm(x, "instance"), chunks=0)
    with pytest.raises(E, match="residual must be"):
        ops.norm_act(ops.NormTerm(x, "none"), residual=torch.zeros(2, 8, 4, 7))


def test_state_dicts_equal_the_recorded_reference(built, golden):
    from mpiflow_amd import raft_extractor as rx
    for cls in ("BasicEncoder", "SmallEncoder"):
        for fn in ("group", "batch", "instance", "none"):
            m = getattr(rx, cls)(output_dim=128, norm_fn=fn, dropout=0.0)
            want = [str(s) for s in golden["z"]["state/%s/%s" % (cls, fn)]]
            assert [str(s) for s in golden["mk"].state_list(m)] == want, (cls, fn)
            fake = {}
            for entry in want:
                k, shape = entry.split(":")
                fake[k] = torch.full([int(s) for s in shape.split("x")] if shape else [], 2, dtype=torch.long if k.endswith("num_batches_tracked") else torch.float32)
            m.load_state_dict(fake, strict=True)
            assert all(bool((v == 2).all()) for v in m.state_dict().values())
            if fn != "none":                                 # the reference's quirk: a strided block's last norm is also downsample.1
                assert m.layer2[0].downsample[1] is getattr(m.layer2[0], "norm3" if cls == "BasicEncoder" else "norm4")
    assert rx.BasicEncoder(128, "batch", dropout=0.5).dropout.p == 0.5 and rx.SmallEncoder(128, "batch").dropout is None


def test_formulas_equal_the_recorded_reference(golden):
    """the numpy float64 restatement == the recorded double run of torch.nn.functional's chain at the sampled entries: out, every gradient,
    the updated running statistics, of all 24 op-level cases"""
    for c in golden["op"].values():
        res = np_chain(c["d"], c["mode"], c["groups"], c["variant"])
        assert sorted(res) == sorted(c["rec"]), (c["name"], sorted(set(res) ^ set(c["rec"])))
        for key, s in c["rec"].items():
            d = sample_err(c, key, res[key])
            assert d <= 1e-11 * max(1.0, s["absmax"]), (c["name"], key, d, s["absmax"])


# ----------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(built):
    from mpiflow_amd import ops
    return ops


def _holder(d, p, mode, groups, dev):
    """the torch.nn module that HOLDS a term's parameters, as the blocks keep it"""
    C = d["weight"].shape[0]
    t = lambda k: torch.from_numpy(d[p + k].copy()).to(dev)
    if mode == "instance":
        return nn.InstanceNorm2d(C).to(dev)
    m = nn.GroupNorm(groups, C) if mode == "group" else nn.BatchNorm2d(C)
    m = m.to(dev)
    with torch.no_grad():
        m.weight.copy_(t("weight"))
        m.bias.copy_(t("bias"))
        if mode != "group":
            m.running_mean.copy_(t("running_mean"))
            m.running_var.copy_(t("running_var"))
    return m.train(mode != "batch_eval")


def run_node(c, dev):
    """an op-level case through the autograd node the blocks use (raft_extractor._fused): every recorded array"""
    from mpiflow_amd import raft_extractor as rx
    d, mode, variant = c["d"], c["mode"], c["variant"]
    t = lambda k: torch.from_numpy(d[k].copy()).to(dev).requires_grad_(True)
    x, norm = t("x"), _holder(d, "", mode, c["groups"], dev)
    res = {}
    if variant == "plain":
        out = rx._fused(x, norm)
    elif variant == "res":
        r = t("res")
        out = rx._fused(x, norm, res=r)
    else:
        r, rnorm = t("rx"), _holder(d, "r", mode, c["groups"], dev)
        out = rx._fused(x, norm, rx=r, rnorm=rnorm)
    out.backward(torch.from_numpy(d["cot"]).to(dev))
    res.update(out=out.detach(), grad_x=x.grad)
    if variant == "res":
        res["grad_res"] = r.grad
    if variant == "rterm":
        res["grad_rx"] = r.grad
    for p, m in (("", norm),) + ((("r", rnorm),) if variant == "rterm" else ()):
        if mode != "instance":
            res["grad_%sweight" % p], res["grad_%sbias" % p] = m.weight.grad, m.bias.grad
        if mode == "batch_train":
            assert int(m.num_batches_tracked) == 1
            res[p + "running_mean_new"], res[p + "running_var_new"] = m.running_mean, m.running_var
    return {k: v.detach().cpu().numpy() for k, v in res.items()}


def run_ops(ops, c, dev, chunks=None, pre_stats=False, d=None):
    """an op-level case through the four kernels alone: out and every gradient (no running statistics)"""
    d, mode, variant, groups = d or c["d"], c["mode"], c["variant"], c["groups"]
    t = lambda k: torch.from_numpy(d[k].copy()).to(dev)

    def term(p):
        x = t("x" if p == "" else "rx")
        kw = {}
        if mode != "instance":
            kw.update(weight=t(p + "weight"), bias=t(p + "bias"))
        if mode == "batch_eval":
            kw.update(running_mean=t(p + "running_mean"), running_var=t(p + "running_var"))
        if pre_stats and mode != "batch_eval":
            kw.update(partials=ops.norm_stats(x, mode, groups=groups, chunks=chunks))
        return ops.NormTerm(x, mode, groups=groups, **kw)

    y = term("")
    residual = None if variant == "plain" else (t("res") if variant == "res" else term("r"))
    out = ops.norm_act(y, residual, chunks=chunks)
    dx, dw, db, dr = ops.norm_act_backward(t("cot"), y, residual, chunks=chunks)
    res = dict(out=out, grad_x=dx)
    if mode != "instance":
        res.update(grad_weight=dw, grad_bias=db)
    if variant == "res":
        res["grad_res"] = dr
    if variant == "rterm":
        res["grad_rx"] = dr[0]
        if mode != "instance":
            res.update(grad_rweight=dr[1], grad_rbias=dr[2])
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.gpu
def test_gpu_kernels_alone_at_the_recorded_samples(golden, built, dev):
    """all 24 op-level cases through the blocks' autograd node: out, every gradient and the updated running statistics within 3 * err32 of
    the recorded double run at the samples"""
    worst = (0.0, "")
    for c in golden["op"].values():
        got = run_node(c, dev)
        assert sorted(got) == sorted(c["rec"]), (c["name"], sorted(set(got) ^ set(c["rec"])))
        for key, s in c["rec"].items():
            d = sample_err(c, key, got[key])
            mult = d / s["err32"] if s["err32"] else 0.0
            worst = max(worst, (mult, c["name"] + " " + key))
            print("kernel %-40s %-18s |hip - ref64| at the samples %.2e = %.2f err32 (err32 %.2e)" % (c["name"], key, d, mult, s["err32"]))
            assert d <= 3 * s["err32"], (c["name"], key, d, s["err32"])
    print("kernels at the samples, worst: %.2f err32 (%s)" % worst)


@pytest.mark.gpu
def test_gpu_kernels_alone_at_every_entry(golden, ops, dev):
    """the four kernels alone against the numpy float64 formulas at EVERY entry, 3 * err32 of the recorded array; the split cases with the
    default chunks, with chunks forced to 1, 3 and 8, and with the statistics computed by a separate norm_stats call"""
    worst = (0.0, "")
    for c in golden["op"].values():
        want = np_chain(c["d"], c["mode"], c["groups"], c["variant"])
        runs = [(None, False)] + ([(1, False), (3, False), (8, False), (3, True), (None, True)] if c["case"].startswith("split") else [(2, True)])
        for chunks, pre in runs:
            got = run_ops(ops, c, dev, chunks=chunks, pre_stats=pre)
            for key, val in got.items():
                s = c["rec"][key]
                d = float(np.abs(val.astype(np.float64) - want[key]).max())
                mult = d / s["err32"] if s["err32"] else 0.0
                worst = max(worst, (mult, "%s %s chunks=%s" % (c["name"], key, chunks)))
                print("kernel %-40s chunks %-4s pre %d %-14s every entry |hip - formula64| %.2e = %.2f err32" % (c["name"], chunks, pre, key, d, mult))
                assert d <= 3 * s["err32"], (c["name"], chunks, pre, key, d, s["err32"])
    print("kernels at every entry, worst: %.2f err32 (%s)" % worst)
    assert ops.norm_default_chunks(128, 220 * 512) > 1 and ops.norm_default_chunks(768, 184 * 248) >= 2 and ops.norm_default_chunks(32, 40 * 52) == 1


def check_arrays(c, what, got, plain, stats_bar=False):
    worst = (0.0, 0.0)
    for key, val in got.items():
        s = c["rec"][key]
        d, dp = sample_err(c, key, val), sample_err(c, key, plain[key])
        kernel_bar = stats_bar and key.startswith("buf_")
        bar = 3 * s["err32"] if kernel_bar else max(3 * s["err32"], 2 * dp)
        worst = max(worst, (d / s["err32"], d / dp if dp else 0.0))
        print("module %-26s %-8s %-44s |hip - ref64| %.2e = %.2f err32 = %.2f x the plain form's %.2e%s"
              % (c["name"], what, key, d, d / s["err32"], d / dp if dp else 0.0, dp, "  (bar: 3 err32)" if kernel_bar else ""))
        assert d <= bar, (c["name"], what, key, d, s["err32"], dp)
    print("module %-26s %-8s worst: %.2f err32, %.2f x the plain form's error" % (c["name"], what, worst[0], worst[1]))


@pytest.mark.gpu
def test_gpu_encoders_match_the_recorded_reference(golden, built, dev):
    """the six encoder cases: output, image gradients and every parameter gradient; a training pass's running statistics at the kernel bar.
    The plain form is a second instance that loaded the first's state_dict with strict=True."""
    mk = golden["mk"]
    for c in golden["enc"].values():
        fused = make_encoder(c, golden)
        plain = make_encoder(c, golden, plain_from=fused)
        got = mk.run_encoder(fused, c["images"], c["cot"], torch.float32, c["training"], device=dev)
        ref = mk.run_encoder(plain, c["images"], c["cot"], torch.float32, c["training"], device=dev)
        assert sorted(got) == sorted(c["rec"]) == sorted(ref), (c["name"], sorted(set(got) ^ set(c["rec"])))
        check_arrays(c, "train" if c["training"] else "eval", got, ref, stats_bar=True)


@pytest.mark.gpu
def test_gpu_blocks_match_the_plain_form(built, dev):
    """both block classes alone, strided and not, under all four norm_fn: output and every gradient against the plain form in float64 on the
    CPU; bar: 3 x what the plain fp32 form on the device makes against the same float64 run (no recorded err32 here, so the plain form's error
    stands in for it; the 3 is the kernel bar's factor).  A convolution bias in front of a norm that subtracts a mean has gradient zero: float64
    leaves less than 1e-10 there, both fp32 forms leave rounding residue, and there is nothing to compare."""
    from mpiflow_amd import raft_extractor as rx
    gen = torch.Generator().manual_seed(11)
    for cls, planes in ((rx.ResidualBlock, 16), (rx.BottleneckBlock, 32)):
        for fn in rx.NORM_FNS:
            for stride in (1, 2):
                torch.manual_seed(3)
                blk = cls(planes if stride == 1 else 8, planes, fn, stride=stride)
                with torch.no_grad():
                    for name, p in blk.named_parameters():
                        if p.dim() == 1:
                            p.add_(0.3 * torch.randn(p.shape, generator=gen))
                x0 = torch.randn(2, blk.conv1.in_channels, 9, 11, generator=gen)
                cot = torch.randn(2, planes, 9 if stride == 1 else 5, 11 if stride == 1 else 6, generator=gen)
                runs = {}
                for what, dtype, device, fwd in (("ref64", torch.float64, "cpu", plain_block), ("plain", torch.float32, dev, plain_block), ("fused", torch.float32, dev, None)):
                    m = cls(blk.conv1.in_channels, planes, fn, stride=stride)
                    m.load_state_dict(blk.state_dict(), strict=True)
                    m = m.to(dtype).to(device)
                    x = x0.to(dtype).to(device).requires_grad_(True)
                    out = m(x) if fwd is None else fwd(m, x)
                    out.backward(cot.to(dtype).to(device))
                    runs[what] = dict(out=out.detach(), grad_x=x.grad, **{"grad_" + k: p.grad for k, p in m.named_parameters()})
                    runs[what] = {k: v.double().cpu() for k, v in runs[what].items()}
                for key, ref in runs["ref64"].items():
                    if float(ref.abs().max()) < 1e-10:
                        continue
                    d, dp = float((runs["fused"][key] - ref).abs().max()), float((runs["plain"][key] - ref).abs().max())
                    print("block %-16s %-8s stride %d %-22s |hip - ref64| %.2e, plain form %.2e" % (cls.__name__, fn, stride, key, d, dp))
                    assert d <= 3 * dp, (cls.__name__, fn, stride, key, d, dp)


@pytest.mark.gpu
def test_gpu_checkpoint_contract(golden, built, dev):
    """freeze_bn: RAFT's isinstance walk puts every BatchNorm2d in eval mode while the encoder stays in training mode; then no running statistic
    changes and the results are the recorded eval case's.  (strict=True loading: make_encoder, in every module test.)"""
    mk = golden["mk"]
    c = golden["enc"]["BasicEncoder/batch_eval"]
    fused = make_encoder(c, golden)
    plain = make_encoder(c, golden, plain_from=fused)
    for enc in (fused, plain):
        enc.train()
        for m in enc.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()
    n_bn = sum(isinstance(m, nn.BatchNorm2d) for m in fused.modules())
    assert n_bn == 15 and fused.training
    before = {k: v.clone() for k, v in fused.state_dict().items()}
    keep_mode = lambda enc: (lambda *a, **k: enc)                  # run_encoder calls .train(training): keep the frozen state
    fused.train, plain.train = keep_mode(fused), keep_mode(plain)
    got = mk.run_encoder(fused, c["images"], c["cot"], torch.float32, False, device=dev)
    ref = mk.run_encoder(plain, c["images"], c["cot"], torch.float32, False, device=dev)
    after = fused.state_dict()
    for k, v in before.items():
        if "running" in k or "num_batches" in k:
            assert torch.equal(v.to(dev), after[k]), k
    check_arrays(c, "frozen", got, ref)


@pytest.mark.gpu
def test_gpu_two_calls_are_bit_identical(golden, ops, dev):
    """every kernel twice on identical arguments, every forced chunks: the same bits"""
    for c in golden["op"].values():
        for chunks in ((None, 1, 3, 8) if c["case"].startswith("split") else (None, 2)):
            a, b = run_ops(ops, c, dev, chunks=chunks), run_ops(ops, c, dev, chunks=chunks)
            for key in a:
                assert bits_equal(a[key], b[key]) == 0, (c["name"], chunks, key)
    c = golden["op"]["op/split_batch/batch_train/rterm"]
    x = torch.from_numpy(c["d"]["x"]).to(dev)
    for chunks in (1, 3, 8):
        assert bits_equal(ops.norm_stats(x, "batch_train", chunks=chunks).cpu().numpy(), ops.norm_stats(x, "batch_train", chunks=chunks).cpu().numpy()) == 0
    acc = torch.full((2, 16, 40, 52), 0.5, device=dev)                             # the accumulate flag adds exactly one rounding
    cr = golden["op"]["op/split_instance/instance/res"]
    t = lambda k: torch.from_numpy(cr["d"][k]).to(dev)
    y = ops.NormTerm(t("x"), "instance")
    ops.norm_act(y, t("res"))
    alone = ops.norm_act_backward(t("cot"), y, t("res"))[3]
    assert ops.norm_act_backward(t("cot"), y, t("res"), dres=acc)[3] is acc and torch.equal(acc, alone + 0.5)


@pytest.mark.gpu
def test_gpu_non_finite_values_stay_where_torch_puts_them(golden, ops, dev):
    """NaN, +inf and -inf planted in x and in the residual: every output is NaN / +inf / -inf exactly where the torch.nn.functional chain (float64,
    CPU) has them, and within the bar everywhere else"""
    mk = golden["mk"]
    plants = ((0, 1, 2, 3, np.nan), (1, 2, 0, 1, np.inf), (1, 4, 4, 6, -np.inf))
    for name, in_x, in_r in (("op/odd/instance/res", plants, ((0, 0, 0, 0, np.nan), (0, 3, 1, 1, np.inf), (1, 0, 2, 2, -np.inf))),
                             ("op/odd/instance/rterm", plants[:1], ((1, 5, 4, 0, np.nan),)),
                             ("op/batch/batch_eval/rterm", ((0, 1, 2, 3, np.nan), (1, 2, 0, 1, np.inf), (2, 4, 3, 5, -np.inf)), ((2, 7, 1, 1, np.nan), (0, 0, 0, 0, np.inf))),
                             ("op/group/group/res", ((1, 9, 2, 2, np.nan),), ((0, 0, 4, 6, -np.inf), (0, 15, 0, 0, np.nan)))):
        c = golden["op"][name]
        d = {k: v.copy() for k, v in c["d"].items()}
        for n, ch, i, j, v in in_x:
            d["x"][n, ch, i, j] = v
        for n, ch, i, j, v in in_r:
            d["res" if c["variant"] == "res" else "rx"][n, ch, i, j] = v
        want = mk.op_reference(d, c["mode"], c["groups"], c["variant"], torch.float64)
        got = run_ops(ops, c, dev, d=d)
        hit = 0
        for key, val in got.items():
            w = want[key]
            assert np.array_equal(np.isnan(val), np.isnan(w)), (name, key, int(np.isnan(val).sum()), int(np.isnan(w).sum()))
            assert np.array_equal(np.isposinf(val), np.isposinf(w)) and np.array_equal(np.isneginf(val), np.isneginf(w)), (name, key)
            fin = np.isfinite(w)
            hit += int((~fin).sum())
            if fin.any():
                assert float(np.abs(val[fin].astype(np.float64) - w[fin]).max()) <= 3 * c["rec"][key]["err32"], (name, key)
        assert hit >= len(in_x) + len(in_r), (name, hit)


@pytest.mark.gpu
def test_gpu_side_stream_and_interleaved_streams(golden, ops, dev):
    ca, cb = golden["op"]["op/split_batch/batch_train/rterm"], golden["op"]["op/odd/instance/res"]
    alone = {c["name"]: run_ops(ops, c, dev, chunks=3) for c in (ca, cb)}
    torch.cuda.synchronize()
    busy, s1, s2 = [torch.cuda.Stream(device=dev) for _ in range(3)]
    big = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(busy):
        for _ in range(20):
            big = big @ big * 1e-3
    with torch.cuda.stream(s1):
        side = run_ops(ops, ca, dev, chunks=3)                                      # ends in a device-to-host copy on s1
    for k in side:
        assert bits_equal(side[k], alone[ca["name"]][k]) == 0, k
    t = lambda c, k: torch.from_numpy(c["d"][k].copy()).to(dev)
    state, got = {}, {}
    torch.cuda.synchronize()
    for c, s in ((ca, s1), (cb, s2)):                                              # forward of each, then backward of each
        with torch.cuda.stream(s):
            if c is ca:
                y = ops.NormTerm(t(c, "x"), "batch_train", weight=t(c, "weight"), bias=t(c, "bias"))
                r = ops.NormTerm(t(c, "rx"), "batch_train", weight=t(c, "rweight"), bias=t(c, "rbias"))
            else:
                y, r = ops.NormTerm(t(c, "x"), "instance"), t(c, "res")
            state[c["name"]] = (y, r, t(c, "cot"), ops.norm_act(y, r, chunks=3))
    for c, s in ((ca, s1), (cb, s2)):
        with torch.cuda.stream(s):
            y, r, cot, out = state[c["name"]]
            dx, dw, db, dr = ops.norm_act_backward(cot, y, r, chunks=3)
            got[c["name"]] = dict(out=out, grad_x=dx, grad_r=dr[0] if isinstance(dr, tuple) else dr)
    s1.synchronize()
    s2.synchronize()
    busy.synchronize()
    for c in (ca, cb):
        a = alone[c["name"]]
        for k, ref in (("out", a["out"]), ("grad_x", a["grad_x"]), ("grad_r", a["grad_rx"] if c is ca else a["grad_res"])):
            assert bits_equal(got[c["name"]][k].cpu().numpy(), ref) == 0, (c["name"], k)


@pytest.mark.gpu
def test_gpu_memory_is_below_the_plain_form(built, dev):
    """forward + backward of one ResidualBlock (instance, stride 2) at 2 x 64 x 96 x 128: peak memory above the inputs, fused against the plain form"""
    from mpiflow_amd import raft_extractor as rx
    torch.manual_seed(5)
    blk = rx.ResidualBlock(64, 96, "instance", stride=2).to(dev)
    x0 = torch.randn(2, 64, 96, 128, device=dev)
    peak = {}
    for what, step in (("plain", lambda x: plain_block(blk, x)), ("fused", blk)):
        for rep in range(2):                                  # the first pass warms MIOpen's workspaces and the allocator
            blk.zero_grad(set_to_none=True)
            x = x0.clone().requires_grad_(True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            step(x).sum().backward()
            torch.cuda.synchronize()
            peak[what] = torch.cuda.max_memory_allocated(dev) - before
            del x
    print("ResidualBlock(64, 96, instance, stride 2) at 2x64x96x128, forward + backward: peak above the inputs %.1f MB fused, %.1f MB plain form, ratio %.3f"
          % (peak["fused"] / 1e6, peak["plain"] / 1e6, peak["fused"] / peak["plain"]))
    assert peak["fused"] < peak["plain"]
