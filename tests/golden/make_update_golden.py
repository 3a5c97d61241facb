#!/usr/bin/env python3
"""Record RAFT's update block by RUNNING THE REFERENCE ITSELF (SepConvGRU, ConvGRU, BasicUpdateBlock and SmallUpdateBlock of
RAFT/core/update.py, CPU) -> tests/golden/raft_update.npz.

    python tests/golden/make_update_golden.py [--out PATH]        (in the build container: needs the reference tree, numpy, torch)

Per case the reference runs in fp32 and on .double() copies; err32 = max |fp32 run - double run| over the WHOLE array is stored per array: the
yardstick of tests/test_raft_update.py.

GRU cases (both classes, five shapes): h', and per half - captured with hooks on the reference's own convolutions, nothing recomputed - the
pre-activations pre_z, pre_r, pre_q (the convolutions' outputs), the second half's input state h_in2, rh (the first C channels of convq's input) and
z, r, q (torch.sigmoid / torch.tanh of the captured outputs, as the reference applies them); for a fixed random cotangent the gradients with
respect to h, x and every parameter, and for the LAST half what the backward kernels compute on their own: the gradients of the three
pre-activations (retain_grad on the captured outputs) and grad_rh (the first C channels of the gradient of convq's input).
Block cases: three chained calls with the same inp; every delta_flow, the last mask, the final net, and the gradients of
sum_i <delta_flow_i, cd_i> + <mask_i, cm_i> + <net_final, cn> with respect to inp, net0 and every parameter.

What the file holds, to stay below the 1 MiB a committed file may have: inputs and weights are draws of np.random.RandomState(seed), rebuilt
by case_inputs() / block_inputs() / fill_params(); the file carries their float64 sums as a check.  Of every recorded array N_SAMPLE entries of
the double run at the flat indices of sample_index(), plus err32 and max |ref64|.  And the state_dict names and shapes of the four classes.

Weights come from RandomState draws, not torch's initialisers, scaled (GRU_GAIN) so that the gates are exercised: the recorder asserts that
between MIN_SHARE and MAX_SHARE of the recorded z and r values of every GRU case lie outside [0.25, 0.75], and err32 > 0 for every array."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

N_SAMPLE = 150
GRU_GAIN = 2.5          # weight std = gain / sqrt(fan_in): pre-activations of a few units, gates from nearly shut to nearly open
NET_GAIN = 1.4          # the other convolutions of the blocks (ReLU chains: keeps the activations' scale)
BIAS_STD = 0.3
MIN_SHARE, MAX_SHARE = 0.1, 0.9   # per gate array; the 5 x 1 half at H = 1 sees one tap of five, hence the low floor

# (name, class, B, hidden C, input_dim, channels of x that are `inp`, H, W, seed)
GRU_CASES = []
for _cls, _s in (("SepConvGRU", 9400), ("ConvGRU", 9500)):
    GRU_CASES += [("%s/tiny_1x4x6" % _cls, _cls, 1, 8, 12, 5, 4, 6, _s), ("%s/odd_2x5x7" % _cls, _cls, 2, 6, 10, 4, 5, 7, _s + 10),
                  ("%s/h1_2x1x72" % _cls, _cls, 2, 8, 12, 6, 1, 72, _s + 20), ("%s/w1_2x9x1" % _cls, _cls, 2, 8, 12, 6, 9, 1, _s + 30),
                  ("%s/real_2x36x120" % _cls, _cls, 2, 128, 256, 128, 36, 120, _s + 40)]
# (name, class, B, H, W, corr_levels, corr_radius, iterations, seed)
BLOCK_CASES = [("BasicUpdateBlock/2x10x14", "BasicUpdateBlock", 2, 10, 14, 4, 4, 3, 9600),
               ("SmallUpdateBlock/2x9x7", "SmallUpdateBlock", 2, 9, 7, 4, 3, 3, 9700)]
BLOCK_DIMS = {"BasicUpdateBlock": (128, 128), "SmallUpdateBlock": (96, 64)}        # hidden, context channels


def halves_of(cls):
    return ("1", "2") if cls == "SepConvGRU" else ("",)


def case_inputs(B, C, Cx, H, W, seed):
    """(h, x, cot) float32: h like a hidden state (tanh of a draw), x like relu'd features (half of them zero), cot the cotangent of h'"""
    rs = np.random.RandomState(seed)
    h = np.tanh(rs.standard_normal((B, C, H, W))).astype(np.float32)
    x = np.maximum(rs.standard_normal((B, Cx, H, W)), 0.0).astype(np.float32)
    cot = rs.standard_normal((B, C, H, W)).astype(np.float32)
    return h, x, cot


def block_inputs(cls, B, H, W, levels, radius, iters, seed):
    """dict of float32 arrays: net0, inp, per iteration corr_i and flow_i, and the cotangents cd_i, cm_i (basic block only), cn"""
    rs = np.random.RandomState(seed)
    hidden, cdim = BLOCK_DIMS[cls]
    planes = levels * (2 * radius + 1) ** 2
    d = dict(net0=np.tanh(rs.standard_normal((B, hidden, H, W))), inp=np.maximum(rs.standard_normal((B, cdim, H, W)), 0.0),
             cn=rs.standard_normal((B, hidden, H, W)))
    for i in range(iters):
        d["corr_%d" % i] = rs.standard_normal((B, planes, H, W))
        d["flow_%d" % i] = 2.0 * rs.standard_normal((B, 2, H, W))
        d["cd_%d" % i] = rs.standard_normal((B, 2, H, W))
        if cls == "BasicUpdateBlock":
            d["cm_%d" % i] = rs.standard_normal((B, 576, H, W))
    return {k: v.astype(np.float32) for k, v in d.items()}


def fill_params(module, seed):
    """Every parameter of `module` (a GRU or a block, the reference's or this repository's: same state_dict) from RandomState draws, in
    state_dict order: weights gain / sqrt(fan_in) * N(0,1), biases BIAS_STD * N(0,1); returns the float64 sum of all of them."""
    rs = np.random.RandomState(seed + 7)
    total = 0.0
    top_is_gru = not any(k.startswith("gru.") for k in module.state_dict())
    with torch.no_grad():
        for name, p in module.state_dict().items():
            shape = tuple(p.shape)
            if name.endswith(".weight"):
                gain = GRU_GAIN if (top_is_gru or name.startswith("gru.")) else NET_GAIN
                v = rs.standard_normal(shape) * (gain / np.sqrt(np.prod(shape[1:])))
            else:
                v = BIAS_STD * rs.standard_normal(shape)
            v = v.astype(np.float32)
            total += float(v.astype(np.float64).sum())
            p.copy_(torch.from_numpy(v).to(p.dtype))
    return total


def sample_index(n, seed):
    return np.random.RandomState(seed + 1).randint(0, n, N_SAMPLE)


def state_list(module):
    return np.array(["%s:%s" % (k, "x".join(str(s) for s in v.shape)) for k, v in module.state_dict().items()])


def load_reference():
    from ref_harness import REFERENCE_ROOT
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_raft_update", os.path.join(REFERENCE_ROOT, "RAFT", "core", "update.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_gru(ref, cls, C, Cx, h, x, cot, seed, dtype):
    """the reference GRU on (h, x) in `dtype`: dict of numpy arrays"""
    gru = getattr(ref, cls)(hidden_dim=C, input_dim=Cx)
    fill_params(gru, seed)
    gru = gru.to(dtype)
    t = lambda a: torch.from_numpy(a).to(dtype)
    ht, xt = t(h).requires_grad_(True), t(x).requires_grad_(True)
    cap = {}
    hooks = []
    for s in halves_of(cls):
        for g in "zrq":
            def out_hook(mod, inputs, output, key="pre_%s%s" % (g, s)):
                output.retain_grad()
                cap[key] = output
            hooks.append(getattr(gru, "conv%s%s" % (g, s)).register_forward_hook(out_hook))

        def in_hook(mod, inputs, key="hx%s" % s):
            cap[key] = inputs[0]
        hooks.append(getattr(gru, "convz%s" % s).register_forward_pre_hook(in_hook))

        def q_in_hook(mod, inputs, key="rhx%s" % s):
            inputs[0].retain_grad()
            cap[key] = inputs[0]
        hooks.append(getattr(gru, "convq%s" % s).register_forward_pre_hook(q_in_hook))
    out = gru(ht, xt)
    assert out.dtype == dtype
    out.backward(t(cot))
    for hk in hooks:
        hk.remove()
    res = dict(h_out=out.detach().numpy(), grad_h=ht.grad.numpy(), grad_x=xt.grad.numpy())
    for name, p in gru.named_parameters():
        res["grad_" + name] = p.grad.numpy()
    for s in halves_of(cls):
        with torch.no_grad():
            for g in "zrq":
                pre = cap["pre_%s%s" % (g, s)]
                res["pre_%s%s" % (g, s)] = pre.detach().numpy()
                res["%s%s" % (g, s)] = (torch.tanh(pre) if g == "q" else torch.sigmoid(pre)).numpy()
            if s != halves_of(cls)[0]:                      # the first half's input state is h itself
                res["h_in" + s] = cap["hx" + s][:, :C].detach().numpy().copy()
            res["rh" + s] = cap["rhx" + s][:, :C].detach().numpy().copy()
    last = halves_of(cls)[-1]
    for g in "zrq":
        res["d_pre_" + g] = cap["pre_%s%s" % (g, last)].grad.numpy()
    res["grad_rh"] = cap["rhx" + last].grad[:, :C].numpy().copy()
    return res


def run_block(ref, cls, levels, radius, iters, d, seed, dtype):
    args = types.SimpleNamespace(corr_levels=levels, corr_radius=radius)
    blk = getattr(ref, cls)(args, hidden_dim=BLOCK_DIMS[cls][0])
    fill_params(blk, seed)
    blk = blk.to(dtype)
    t = lambda a: torch.from_numpy(a).to(dtype)
    net, inp = t(d["net0"]).requires_grad_(True), t(d["inp"]).requires_grad_(True)
    net0 = net
    loss = 0.0
    res = {}
    for i in range(iters):
        net, mask, dflow = blk(net, inp, t(d["corr_%d" % i]), t(d["flow_%d" % i]))
        res["delta_flow_%d" % i] = dflow.detach().numpy()
        loss = loss + (dflow * t(d["cd_%d" % i])).sum()
        if mask is not None:
            loss = loss + (mask * t(d["cm_%d" % i])).sum()
            res["mask_last"] = mask.detach().numpy()
    loss = loss + (net * t(d["cn"])).sum()
    loss.backward()
    res["net_out"] = net.detach().numpy()
    res["grad_inp"], res["grad_net0"] = inp.grad.numpy(), net0.grad.numpy()
    for name, p in blk.named_parameters():
        res["grad_" + name] = p.grad.numpy()
    return res


def store(rec, prefix, r32, r64, seed):
    errs = []
    for key in r64:
        v32, v64 = r32[key], r64[key]
        assert v32.dtype == np.float32 and v64.dtype == np.float64 and v32.shape == v64.shape, key
        idx = sample_index(v64.size, seed)
        err = float(np.abs(v32.astype(np.float64) - v64).max())
        assert err > 0.0, "err32 of %s%s is zero" % (prefix, key)
        rec[prefix + key + "_f64"] = v64.reshape(-1)[idx]
        rec[prefix + key + "_err32"] = np.float64(err)
        rec[prefix + key + "_absmax"] = np.float64(np.abs(v64).max())
        errs.append(err)
    rec[prefix + "keys"] = np.array(list(r64))
    return errs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "raft_update.npz"))
    a = ap.parse_args()
    ref = load_reference()
    torch.manual_seed(0)
    rec = {"numpy_version": np.array(np.__version__), "torch_version": np.array(torch.__version__), "n_sample": np.int64(N_SAMPLE),
           "gru_names": np.array([c[0] for c in GRU_CASES]), "block_names": np.array([c[0] for c in BLOCK_CASES])}
    args = types.SimpleNamespace(corr_levels=4, corr_radius=4)
    rec["state/SepConvGRU"] = state_list(ref.SepConvGRU(hidden_dim=128, input_dim=256))
    rec["state/ConvGRU"] = state_list(ref.ConvGRU(hidden_dim=96, input_dim=146))
    rec["state/BasicUpdateBlock"] = state_list(ref.BasicUpdateBlock(args, hidden_dim=128))
    rec["state/SmallUpdateBlock"] = state_list(ref.SmallUpdateBlock(types.SimpleNamespace(corr_levels=4, corr_radius=3), hidden_dim=96))
    for name, cls, B, C, Cx, n_ctx, H, W, seed in GRU_CASES:
        h, x, cot = case_inputs(B, C, Cx, H, W, seed)
        r32 = run_gru(ref, cls, C, Cx, h, x, cot, seed, torch.float32)
        r64 = run_gru(ref, cls, C, Cx, h, x, cot, seed, torch.float64)
        p = name + "/"
        rec[p + "settings"] = np.array([B, C, Cx, n_ctx, H, W, seed], np.int64)
        gru = getattr(ref, cls)(hidden_dim=C, input_dim=Cx)
        rec[p + "input_sums"] = np.array([h.astype(np.float64).sum(), x.astype(np.float64).sum(), cot.astype(np.float64).sum(), fill_params(gru, seed)])
        shares = []
        for s in halves_of(cls):
            for g in "zr":
                v = r64[g + s]
                shares.append(float(((v < 0.25) | (v > 0.75)).mean()))
        assert all(MIN_SHARE <= s <= MAX_SHARE for s in shares), (name, shares)
        errs = store(rec, p, r32, r64, seed)
        print("%-28s gates outside [0.25, 0.75]: %s  err32 h' %.1e  min/max err32 %.1e / %.1e  (%d arrays)"
              % (name, " ".join("%.2f" % s for s in shares), rec[p + "h_out_err32"], min(errs), max(errs), len(errs)))
    for name, cls, B, H, W, levels, radius, iters, seed in BLOCK_CASES:
        d = block_inputs(cls, B, H, W, levels, radius, iters, seed)
        r32 = run_block(ref, cls, levels, radius, iters, d, seed, torch.float32)
        r64 = run_block(ref, cls, levels, radius, iters, d, seed, torch.float64)
        p = name + "/"
        rec[p + "settings"] = np.array([B, H, W, levels, radius, iters, seed], np.int64)
        blk = getattr(ref, cls)(types.SimpleNamespace(corr_levels=levels, corr_radius=radius), hidden_dim=BLOCK_DIMS[cls][0])
        rec[p + "input_sums"] = np.array([sum(v.astype(np.float64).sum() for v in d.values()), fill_params(blk, seed)])
        errs = store(rec, p, r32, r64, seed)
        print("%-28s err32 net %.1e (absmax %.1e) delta_flow %.1e (absmax %.1e) grad_inp %.1e  (%d arrays)"
              % (name, rec[p + "net_out_err32"], rec[p + "net_out_absmax"], rec[p + "delta_flow_2_err32"], rec[p + "delta_flow_2_absmax"],
                 rec[p + "grad_inp_err32"], len(errs)))
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 1 << 20
    return 0


if __name__ == "__main__":
    sys.exit(main())
