#!/usr/bin/env python3
"""Record the assembled RAFT model, basic and small, by RUNNING THE REFERENCE ITSELF (RAFT/core/raft.py, CPU) -> tests/golden/raft_model.npz.

    python tests/golden/make_raft_golden.py [--out PATH]        (in the build container: needs the reference tree, numpy, torch)

Per case the reference runs in fp32 and in double; err32 = max |fp32 run - double run| over the WHOLE array is stored per array: the yardstick
of tests/test_raft_model.py.  The reference casts to fp32 in coords_grid, in RAFT.forward (fmap.float()) and at the end of CorrBlock.__call__;
for the double run torch.Tensor.float is neutralised for the duration of the call (floating tensors come back unchanged, integer ones as
double), as make_corr_golden.py does for the one cast it meets; the recorder asserts that what comes out is float64.

Cases (CASES): the smallest frames the reference can run - below 128 x 128 the coarsest correlation level is 1 x 1 and its sampler divides by
zero - one side not a power of two in the training cases.  Forward: every prediction of a training case, or the (coarse flow, flow_up) pair of
a test_mode case; net and inp after the split and fmap1 (forward hooks on update_block and fnet: nothing is recomputed); for basic/train the
last up_mask.  Backward, training cases: the gradients of sum_i <pred_i, cot_i> (linear: no L1 kink) with respect to EVERY parameter.

What the file holds, to stay below the 1 MiB a committed file may have: images, flow_init, cotangents and weights are draws of
np.random.RandomState(seed), rebuilt by case_inputs() / fill_params(); the file carries their float64 sums as a check.  Of every recorded
array N_SAMPLE entries of the double run at the flat indices of sample_index(), plus err32 and max |ref64|.  The state_dict names and shapes
of both variants.  Per training case `zero_grads`: the parameters whose double gradient is structurally zero (|g64| <= 1e-9 x the case's
largest gradient absmax): the biases of convolutions that feed an instance or batch norm in training mode.  Every bar of the tests is
absolute, so these need no special rule; the list exists so that nobody divides by their magnitude.

The recorder asserts: no NaN; err32 > 0 for every array; err32 <= 1e-3 * absmax for every forward array; final |flow| absmax >= 1 px (the
lookups really move)."""
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
CONV_GAIN = 1.0         # weight std = gain / sqrt(fan_in): flows of a few px to a few tens, inside the frame
BIAS_STD = 0.1
SHIFT = (3, 5)          # image2 = image1 rolled by (rows, columns): the correlation has structure

# (name, small, N, H, W, iterations, training case, seed)
CASES = [("basic/train_2x128x136", False, 2, 128, 136, 3, True, 9800), ("basic/eval_1x128x128", False, 1, 128, 128, 12, False, 9810),
         ("small/train_2x136x128", True, 2, 136, 128, 3, True, 9820), ("small/eval_1x128x128", True, 1, 128, 128, 12, False, 9830)]


def make_args(small):
    return argparse.Namespace(small=small, mixed_precision=False, dropout=0, alternate_corr=False)


def case_inputs(N, H, W, iters, train, seed):
    """dict of float32 arrays: image1, image2 (integers 0..255), and for a training case the cotangents cot_i [N,2,H,W], for a test_mode case
    flow_init [N,2,H/8,W/8]"""
    rs = np.random.RandomState(seed)
    d = dict(image1=rs.randint(0, 256, (N, 3, H, W)).astype(np.float32))
    d["image2"] = np.roll(d["image1"], SHIFT, axis=(2, 3)).copy()
    if train:
        for i in range(iters):
            d["cot_%d" % i] = rs.standard_normal((N, 2, H, W)).astype(np.float32)
    else:
        d["flow_init"] = (2.0 * rs.standard_normal((N, 2, H // 8, W // 8))).astype(np.float32)
    return d


def fill_params(module, seed):
    """Every entry of `module`'s state_dict (the reference's RAFT or this repository's: same state_dict) from RandomState draws, in state_dict
    order: convolution weights CONV_GAIN / sqrt(fan_in) * N(0,1), norm weights 1 + 0.1 N(0,1), biases and running means BIAS_STD * N(0,1),
    running variances 0.5 + |N(0,1)|; num_batches_tracked stays.  Returns the float64 sum of what was drawn."""
    rs = np.random.RandomState(seed + 7)
    total = 0.0
    with torch.no_grad():
        for name, p in module.state_dict().items():
            shape = tuple(p.shape)
            if name.endswith("num_batches_tracked"):
                continue
            if name.endswith(".weight") and len(shape) > 1:
                v = rs.standard_normal(shape) * (CONV_GAIN / np.sqrt(np.prod(shape[1:])))
            elif name.endswith(".weight"):
                v = 1.0 + 0.1 * rs.standard_normal(shape)
            elif name.endswith("running_var"):
                v = 0.5 + np.abs(rs.standard_normal(shape))
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
    core = os.path.join(REFERENCE_ROOT, "RAFT", "core")
    sys.path.insert(0, core)                                 # raft.py does `from update import ...`, `from utils.utils import ...`
    sys.dont_write_bytecode = True
    try:
        import scipy.interpolate  # noqa: F401
    except ImportError:                                      # utils/utils.py imports it at top level and never uses it here
        stub = types.ModuleType("scipy")
        stub.interpolate = types.ModuleType("scipy.interpolate")
        sys.modules["scipy"], sys.modules["scipy.interpolate"] = stub, stub.interpolate
    spec = importlib.util.spec_from_file_location("ref_raft_model", os.path.join(core, "raft.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_case(ref, small, iters, train, d, seed, dtype):
    """the reference RAFT on the case in `dtype`: dict of numpy arrays, the parameter gradients under "grad_<name>" """
    model = ref.RAFT(make_args(small))
    fill_params(model, seed)
    model = model.to(dtype)
    if train:
        model.train()
    else:
        model.freeze_bn()
        model.eval()
    t = lambda a: torch.from_numpy(a).to(dtype)
    cap = {}

    def fnet_hook(mod, inputs, output):
        cap["fmap1"] = output[0]

    def pre_hook(mod, inputs):
        if "net" not in cap:
            cap["net"], cap["inp"] = inputs[0], inputs[1]

    def out_hook(mod, inputs, output):
        if output[1] is not None:
            cap["up_mask_last"] = output[1]
    hooks = [model.fnet.register_forward_hook(fnet_hook), model.update_block.register_forward_pre_hook(pre_hook),
             model.update_block.register_forward_hook(out_hook)]
    keep = torch.Tensor.float
    if dtype == torch.float64:                               # the reference's own casts to fp32; restored below
        torch.Tensor.float = lambda self: self if self.is_floating_point() else self.double()
    try:
        if train:
            preds = model(t(d["image1"]), t(d["image2"]), iters=iters)
        else:
            with torch.no_grad():
                preds = model(t(d["image1"]), t(d["image2"]), iters=iters, flow_init=t(d["flow_init"]), test_mode=True)
    finally:
        torch.Tensor.float = keep
    for hk in hooks:
        hk.remove()
    res = {}
    if train:
        assert len(preds) == iters
        loss = 0.0
        for i, p in enumerate(preds):
            res["pred_%d" % i] = p.detach().numpy()
            loss = loss + (p * t(d["cot_%d" % i])).sum()
        loss.backward()
    else:
        res["flow_coarse"], res["flow_up"] = preds[0].numpy(), preds[1].numpy()
    for key in ("net", "inp", "fmap1") + (("up_mask_last",) if train and not small else ()):
        res[key] = cap[key].detach().numpy()
    if train:
        for name, p in model.named_parameters():
            res["grad_" + name] = p.grad.numpy()
    for key, v in res.items():
        assert v.dtype == (np.float64 if dtype == torch.float64 else np.float32), (key, v.dtype)
        assert np.isfinite(v).all(), key
    return res


def store(rec, prefix, r32, r64, seed):
    for key in r64:
        v32, v64 = r32[key], r64[key]
        assert v32.shape == v64.shape, key
        err = float(np.abs(v32.astype(np.float64) - v64).max())
        absmax = float(np.abs(v64).max())
        assert err > 0.0, "err32 of %s%s is zero" % (prefix, key)
        if not key.startswith("grad_"):
            assert err <= 1e-3 * absmax, "err32 of %s%s is %.2e of absmax %.2e" % (prefix, key, err, absmax)
        rec[prefix + key + "_f64"] = v64.reshape(-1)[sample_index(v64.size, seed)]
        rec[prefix + key + "_err32"] = np.float64(err)
        rec[prefix + key + "_absmax"] = np.float64(absmax)
    rec[prefix + "keys"] = np.array(list(r64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "raft_model.npz"))
    a = ap.parse_args()
    ref = load_reference()
    torch.manual_seed(0)
    rec = {"numpy_version": np.array(np.__version__), "torch_version": np.array(torch.__version__), "n_sample": np.int64(N_SAMPLE),
           "names": np.array([c[0] for c in CASES])}
    for small in (False, True):
        rec["state/small" if small else "state/basic"] = state_list(ref.RAFT(make_args(small)))
    for name, small, N, H, W, iters, train, seed in CASES:
        d = case_inputs(N, H, W, iters, train, seed)
        r32 = run_case(ref, small, iters, train, d, seed, torch.float32)
        r64 = run_case(ref, small, iters, train, d, seed, torch.float64)
        p = name + "/"
        rec[p + "settings"] = np.array([int(small), N, H, W, iters, int(train), seed], np.int64)
        rec[p + "input_sums"] = np.array([sum(v.astype(np.float64).sum() for v in d.values()), fill_params(ref.RAFT(make_args(small)), seed)])
        store(rec, p, r32, r64, seed)
        final = "pred_%d" % (iters - 1) if train else "flow_up"
        assert rec[p + final + "_absmax"] >= 1.0, (name, rec[p + final + "_absmax"])
        fwd = [k for k in r64 if not k.startswith("grad_")]
        line = "%-24s final |flow| absmax %.2f px; forward err32/absmax %.1e .. %.1e (%d arrays)" % (
            name, rec[p + final + "_absmax"], min(rec[p + k + "_err32"] / rec[p + k + "_absmax"] for k in fwd),
            max(rec[p + k + "_err32"] / rec[p + k + "_absmax"] for k in fwd), len(fwd))
        if train:
            grads = [k for k in r64 if k.startswith("grad_")]
            top = max(rec[p + k + "_absmax"] for k in grads)
            zero = [k[len("grad_"):] for k in grads if rec[p + k + "_absmax"] <= 1e-9 * top]
            rec[p + "zero_grads"] = np.array(zero)
            noise = max(rec[p + "grad_" + k + "_err32"] for k in zero)
            line += "; %d gradients, largest absmax %.2e, worst err32 %.1e; %d structurally zero (fp32 noise there %.1e)" % (
                len(grads), top, max(rec[p + k + "_err32"] for k in grads), len(zero), noise)
        print(line)
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 1 << 20
    return 0


if __name__ == "__main__":
    sys.exit(main())
