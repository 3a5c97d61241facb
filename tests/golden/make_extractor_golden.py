#!/usr/bin/env python3
"""Record RAFT's encoders by RUNNING THE REFERENCE ITSELF (ResidualBlock, BottleneckBlock, BasicEncoder and SmallEncoder of
RAFT/core/extractor.py, CPU) -> tests/golden/raft_extractor.npz.

    python tests/golden/make_extractor_golden.py [--out PATH]        (in the build container: needs the reference tree, numpy, torch)

Every case runs in fp32 and on .double() copies; err32 = max |fp32 run - double run| over the WHOLE array is stored per array: the yardstick of
tests/test_raft_extractor.py.

Op-level cases (OP_CASES x VARIANTS): the chain the reference's modules call - torch.nn.functional's instance_norm / batch_norm / group_norm,
relu, add, relu - on one activation: out = relu(norm(x)) ('plain'), relu(res + relu(norm(x))) ('res', an identity shortcut) and
relu(norm(rx) + relu(norm(x))) ('rterm', the downsample branch); for a fixed cotangent every input and parameter gradient; batch norm in
training mode (with the updated running statistics) and in eval mode.
Encoder cases (ENCODER_CASES): the reference's encoder on seeded images; its output and, for a fixed cotangent, the gradients with respect to
the images and every parameter; the batch-norm encoder in training mode (with every running statistic after the pass) and in eval mode.

What the file holds, to stay below the 1 MiB a committed file may have: inputs and weights are draws of np.random.RandomState(seed), rebuilt
by op_inputs() / encoder_inputs() / fill_params(); the file carries their float64 sums as a check.  Of every recorded array N_SAMPLE entries of
the double run at the flat indices of sample_index() (the whole array where it has no more entries than that), plus err32 and max |ref64|.
And the state_dict names and shapes of both encoders under all four norm_fn values.

Activations are drawn with mean 3 and standard deviation 0.5 - a convolution's output carries a bias - and convolution weights with
gain / sqrt(fan_in) and non-zero biases; affine parameters and running statistics are non-trivial draws.  The recorder asserts err32 > 0 for
every array (but the identity shortcut's gradient, a masked copy of the cotangent, where it asserts err32 = 0) and that between 20 % and 80 % of every recorded op-level output (all post-ReLU) is zero."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

N_SAMPLE = 150
EPS = 1e-5
MOMENTUM = 0.1
CONV_GAIN = 1.4
BIAS_STD = 0.3
X_MEAN, X_STD = 3.0, 0.5
EXACT = ("grad_res",)   # the identity shortcut's gradient is the cotangent or 0: exact in both runs, err32 = 0, and the tests' bar 3 * err32 asks for equality

# (name, N, C, H, W, norm, groups, seed)
OP_CASES = [("tiny", 1, 8, 2, 3, "instance", 1, 9800), ("odd", 2, 6, 5, 7, "instance", 1, 9810), ("group", 2, 16, 5, 7, "group", 2, 9820),
            ("batch", 3, 8, 4, 6, "batch", 1, 9830), ("split_instance", 2, 16, 40, 52, "instance", 1, 9840), ("split_batch", 2, 16, 40, 52, "batch", 1, 9850)]
VARIANTS = ("plain", "res", "rterm")
# (name, class, norm_fn, output_dim, image batches, N, H, W, training, seed)
ENCODER_CASES = [("BasicEncoder/instance", "BasicEncoder", "instance", 256, 2, 1, 32, 48, True, 9900),
                 ("BasicEncoder/batch_train", "BasicEncoder", "batch", 256, 1, 2, 32, 48, True, 9910),
                 ("BasicEncoder/batch_eval", "BasicEncoder", "batch", 256, 1, 2, 32, 48, False, 9910),
                 ("BasicEncoder/group", "BasicEncoder", "group", 128, 1, 1, 32, 48, True, 9920),
                 ("SmallEncoder/instance", "SmallEncoder", "instance", 128, 1, 2, 37, 51, True, 9930),
                 ("SmallEncoder/none", "SmallEncoder", "none", 160, 1, 2, 32, 48, True, 9940)]


def op_modes(norm):
    """the kernel modes a case's norm is recorded in"""
    return ("batch_train", "batch_eval") if norm == "batch" else (norm,)


def op_inputs(N, C, H, W, norm, seed):
    """dict of float32 arrays: x, rx (activations, mean 3, std 0.5), res (a shortcut: about 60 % of res + relu(.) positive), cot, and the
    parameters of both terms: weight, bias, rweight, rbias (affine norms), running_mean, running_var, rrunning_mean, rrunning_var (batch)"""
    rs = np.random.RandomState(seed)
    shape = (N, C, H, W)
    d = dict(x=X_MEAN + X_STD * rs.standard_normal(shape), rx=X_MEAN + X_STD * rs.standard_normal(shape), res=rs.standard_normal(shape) - 0.6,
             cot=rs.standard_normal(shape))
    for p in ("", "r"):
        d[p + "weight"] = 1.0 + 0.3 * rs.standard_normal(C)
        d[p + "bias"] = 0.3 * rs.standard_normal(C)
        d[p + "running_mean"] = X_MEAN + 0.3 * rs.standard_normal(C)
        d[p + "running_var"] = X_STD ** 2 * (0.5 + rs.uniform(size=C))
    return {k: v.astype(np.float32) for k, v in d.items()}


def op_reference(d, mode, groups, variant, dtype):
    """the torch.nn.functional chain in `dtype` on CPU: dict of numpy arrays (out, every gradient, the updated running statistics)"""
    t = {k: torch.from_numpy(v.copy()).to(dtype) for k, v in d.items()}
    affine = mode != "instance"
    leaves = ["x"] + (["weight", "bias"] if affine else [])
    if variant == "res":
        leaves += ["res"]
    if variant == "rterm":
        leaves += ["rx"] + (["rweight", "rbias"] if affine else [])
    for k in leaves:
        t[k].requires_grad_(True)

    def norm(x, p):
        if mode == "instance":
            return F.instance_norm(x, eps=EPS)
        if mode == "group":
            return F.group_norm(x, groups, t[p + "weight"], t[p + "bias"], eps=EPS)
        return F.batch_norm(x, t[p + "running_mean"], t[p + "running_var"], t[p + "weight"], t[p + "bias"], training=mode == "batch_train",
                            momentum=MOMENTUM, eps=EPS)

    y = F.relu(norm(t["x"], ""))
    if variant == "res":
        y = F.relu(t["res"] + y)
    elif variant == "rterm":
        y = F.relu(norm(t["rx"], "r") + y)
    y.backward(t["cot"])
    out = {"out": y.detach().numpy()}
    for k in leaves:
        out["grad_" + k] = t[k].grad.numpy()
    if mode == "batch_train":
        for p in ("", "r") if variant == "rterm" else ("",):
            out[p + "running_mean_new"], out[p + "running_var_new"] = t[p + "running_mean"].numpy(), t[p + "running_var"].numpy()
    return out


def encoder_inputs(batches, N, H, W, out_dim, seed):
    """(list of `batches` images [N,3,H,W] in [-1, 1], cotangent of the concatenated output [batches*N,out_dim,H/8,W/8]) float32"""
    rs = np.random.RandomState(seed)
    images = [rs.uniform(-1.0, 1.0, (N, 3, H, W)).astype(np.float32) for _ in range(batches)]
    h2, w2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    h4, w4 = (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1
    h8, w8 = (h4 - 1) // 2 + 1, (w4 - 1) // 2 + 1
    cot = rs.standard_normal((batches * N, out_dim, h8, w8)).astype(np.float32)
    return images, cot


def fill_params(module, seed):
    """Every entry of `module`'s state_dict (the reference's encoder or this repository's: same state_dict) from RandomState draws, in
    state_dict order: convolution weights gain / sqrt(fan_in) * N(0,1), norm weights 1 + 0.3 N(0,1), biases 0.3 N(0,1), running means
    0.3 N(0,1), running variances 0.5 + U(0,1); num_batches_tracked stays.  Returns the float64 sum of everything written."""
    rs = np.random.RandomState(seed + 7)
    total = 0.0
    with torch.no_grad():
        for name, p in module.state_dict().items():
            shape = tuple(p.shape)
            if name.endswith("num_batches_tracked"):
                continue
            if name.endswith(".weight") and len(shape) == 4:
                v = rs.standard_normal(shape) * (CONV_GAIN / np.sqrt(np.prod(shape[1:])))
            elif name.endswith(".weight"):
                v = 1.0 + 0.3 * rs.standard_normal(shape)
            elif name.endswith("running_var"):
                v = 0.5 + rs.uniform(size=shape)
            else:
                v = BIAS_STD * rs.standard_normal(shape)
            v = v.astype(np.float32)
            total += float(v.astype(np.float64).sum())
            p.copy_(torch.from_numpy(v).to(p.dtype))
    return total


def run_encoder(enc, images, cot, dtype, training, device="cpu"):
    """an encoder (any implementation with the reference's forward contract) on the seeded images: dict of numpy arrays"""
    enc = enc.to(dtype).to(device)
    enc.train(training)
    ims = [torch.from_numpy(im).to(dtype).to(device).requires_grad_(True) for im in images]
    out = enc(ims) if len(ims) == 2 else enc(ims[0])
    if len(ims) == 2:
        assert isinstance(out, tuple) and len(out) == 2
        out = torch.cat(out, dim=0)
    out.backward(torch.from_numpy(cot).to(dtype).to(device))
    res = {"out": out}
    for k, im in enumerate(ims):
        res["grad_image%d" % k] = im.grad
    for name, p in enc.named_parameters():
        res["grad_" + name] = p.grad
    if training:
        for name, b in enc.named_buffers():
            if name.endswith(("running_mean", "running_var")):
                res["buf_" + name] = b
    return {k: v.detach().cpu().numpy() for k, v in res.items()}


def sample_index(n, seed):
    return np.arange(n) if n <= N_SAMPLE else np.random.RandomState(seed + 1).randint(0, n, N_SAMPLE)


def state_list(module):
    return np.array(["%s:%s" % (k, "x".join(str(s) for s in v.shape)) for k, v in module.state_dict().items()])


def load_reference():
    from ref_harness import REFERENCE_ROOT
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_raft_extractor", os.path.join(REFERENCE_ROOT, "RAFT", "core", "extractor.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def store(rec, prefix, r32, r64, seed):
    errs = []
    for key in r64:
        v32, v64 = r32[key], r64[key]
        assert v32.dtype == np.float32 and v64.dtype == np.float64 and v32.shape == v64.shape, key
        err = float(np.abs(v32.astype(np.float64) - v64).max())
        assert (err == 0.0) if key in EXACT else (err > 0.0), "err32 of %s%s is %g" % (prefix, key, err)
        rec[prefix + key + "_f64"] = v64.reshape(-1)[sample_index(v64.size, seed)]
        rec[prefix + key + "_err32"] = np.float64(err)
        rec[prefix + key + "_absmax"] = np.float64(np.abs(v64).max())
        errs.append(err)
    rec[prefix + "keys"] = np.array(list(r64))
    return errs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "raft_extractor.npz"))
    a = ap.parse_args()
    ref = load_reference()
    torch.manual_seed(0)
    rec = {"numpy_version": np.array(np.__version__), "torch_version": np.array(torch.__version__), "n_sample": np.int64(N_SAMPLE)}
    for cls in ("BasicEncoder", "SmallEncoder"):
        for fn in ("group", "batch", "instance", "none"):
            rec["state/%s/%s" % (cls, fn)] = state_list(getattr(ref, cls)(output_dim=128, norm_fn=fn, dropout=0.0))
    names = []
    for name, N, C, H, W, norm, groups, seed in OP_CASES:
        d = op_inputs(N, C, H, W, norm, seed)
        for mode in op_modes(norm):
            for variant in VARIANTS:
                p = "op/%s/%s/%s/" % (name, mode, variant)
                names.append(p[:-1])
                r32, r64 = op_reference(d, mode, groups, variant, torch.float32), op_reference(d, mode, groups, variant, torch.float64)
                zero = float((r64["out"] == 0).mean())
                assert 0.2 <= zero <= 0.8, (p, zero)
                errs = store(rec, p, r32, r64, seed)
                print("%-40s zero share of out %.2f  err32 out %.1e  min/max err32 %.1e / %.1e  (%d arrays)" % (p, zero, rec[p + "out_err32"], min(errs), max(errs), len(errs)))
        rec["op/%s/input_sums" % name] = np.array([d[k].astype(np.float64).sum() for k in sorted(d)])
    rec["op_names"] = np.array(names)
    for name, cls, fn, out_dim, batches, N, H, W, training, seed in ENCODER_CASES:
        images, cot = encoder_inputs(batches, N, H, W, out_dim, seed)
        runs = {}
        for dtype in (torch.float32, torch.float64):
            enc = getattr(ref, cls)(output_dim=out_dim, norm_fn=fn, dropout=0.0)
            total = fill_params(enc, seed)
            runs[dtype] = run_encoder(enc, images, cot, dtype, training)
        p = name + "/"
        rec[p + "input_sums"] = np.array([sum(im.astype(np.float64).sum() for im in images), cot.astype(np.float64).sum(), total])
        errs = store(rec, p, runs[torch.float32], runs[torch.float64], seed)
        print("%-28s out %s err32 %.1e (absmax %.1e)  grad_image0 err32 %.1e  min/max err32 %.1e / %.1e  (%d arrays)"
              % (name, runs[torch.float64]["out"].shape, rec[p + "out_err32"], rec[p + "out_absmax"], rec[p + "grad_image0_err32"], min(errs), max(errs), len(errs)))
    rec["encoder_names"] = np.array([c[0] for c in ENCODER_CASES])
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 1 << 20
    return 0


if __name__ == "__main__":
    sys.exit(main())
