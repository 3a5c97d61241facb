#!/usr/bin/env python3
"""Record RAFT's correlation lookup by RUNNING THE REFERENCE ITSELF (CorrBlock of RAFT/core/corr.py, CPU) -> tests/golden/raft_corr.npz.

    python tests/golden/make_corr_golden.py [--out PATH]        (in the build container: needs the reference tree, numpy, torch)

Per case: CorrBlock(fmap1, fmap2, L, r)(coords) in fp32 and on .double() inputs, and for a fixed random cotangent g the reference's
fmap1.grad / fmap2.grad (autograd through CorrBlock), fp32 and double.  err32 = max |fp32 run - double run| over the WHOLE array is stored
per case for the output and both gradients: it is the yardstick of tests/test_raft_corr.py.

What the file holds, so that it stays far below the 1 MiB a committed file may have (the double output of the largest case alone is 2.2 MB):
  * the feature maps and the cotangent are NOT stored: they are standard_normal draws of np.random.RandomState(seed) (a frozen stream), cast
    to float32; case_inputs() below rebuilds them and the file carries their float64 sums as a check.  coords are stored in full.
  * of the output and of each gradient, N_SAMPLE entries at flat indices drawn by RandomState(seed + 1) (rebuilt by sample_index()), fp32 and
    float64; the full-array maxima (err32, max |ref64|) and, bit-packed, which output entries the reference reports as exactly 0.
tests/test_raft_corr.py checks its fp64 restatement of the formula against these samples, and the kernel against the samples AND, entry by
entry, against that restatement."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

N_SAMPLE = 5000

# (name, C, H, W, num_levels, radius, seed, coords: "random" | "adversarial")
CASES = [
    ("c64_17x29_r3_l2", 64, 17, 29, 2, 3, 9100, "random"),
    ("c256_23x37", 256, 23, 37, 4, 4, 9110, "random"),
    ("c128_16x24", 128, 16, 24, 4, 4, 9120, "random"),
    ("c64_16x24_adversarial", 64, 16, 24, 4, 4, 9130, "adversarial"),
]


def adversarial_coords(H, W, rs):
    """exact integers, exact half pixels, negative fractions, windows wholly outside on every side, +-1e9"""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    c = np.stack([xs, ys]).copy()                                            # rows 0-1: the identity grid (exact integers)
    c[:, 2:4] += np.float32(0.5)                                             # exact half pixels
    c[:, 4:6] = np.round(c[:, 4:6] + rs.uniform(-6, 6, (2, 2, W))).astype(np.float32)        # other exact integers
    c[0, 6], c[1, 6] = np.float32(-0.25), np.float32(-7.5)                   # negative fractions (floor, not truncation)
    c[0, 7], c[1, 7] = np.float32(-7.5), np.float32(-0.25)
    c[0, 8] = np.float32(-40.0)                                              # wholly outside: left, right, above, below
    c[0, 9] = np.float32(W + 40.0)
    c[1, 10] = np.float32(-40.0)
    c[1, 11] = np.float32(H + 40.0)
    c[0, 12, ::2], c[0, 12, 1::2] = np.float32(1e9), np.float32(-1e9)
    c[1, 13, ::2], c[1, 13, 1::2] = np.float32(-1e9), np.float32(1e9)
    c[:, 14] = (c[:, 14] + rs.uniform(-0.999, 0.0, (2, W))).astype(np.float32) - np.float32(3.0)   # straddling the left / top edge
    c[0, 15] = np.float32(W - 1.0)                                           # the last column, exactly
    c[1, 15] = np.float32(H - 1.0)
    return c[None].astype(np.float32)


def case_inputs(C, H, W, L, r, seed, kind):
    """(fmap1, fmap2, g, coords-or-None) of a case, float32: what the recorder fed the reference (coords of the file take precedence)"""
    rs = np.random.RandomState(seed)
    f1 = rs.standard_normal((1, C, H, W)).astype(np.float32)
    f2 = rs.standard_normal((1, C, H, W)).astype(np.float32)
    g = rs.standard_normal((1, L * (2 * r + 1) ** 2, H, W)).astype(np.float32)
    if kind == "adversarial":
        coords = adversarial_coords(H, W, rs)
    else:
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        coords = (np.stack([xs, ys])[None] + 6.0 * rs.standard_normal((1, 2, H, W))).astype(np.float32)
    return f1, f2, g, coords


def sample_index(n, seed):
    return np.random.RandomState(seed + 1).randint(0, n, N_SAMPLE)


def load_reference_corr():
    from ref_harness import REFERENCE_ROOT
    core = os.path.join(REFERENCE_ROOT, "RAFT", "core")
    sys.path.insert(0, core)                                 # corr.py does `from utils.utils import bilinear_sampler, coords_grid`
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_raft_corr", os.path.join(core, "corr.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_case(corr, f1, f2, g, coords, L, r, dtype):
    """CorrBlock's output and gradients in `dtype`.  CorrBlock.__call__ ends in `.float()`; for the double run that cast is undone by running
    its body up to the cast: the class's own pyramid and sampler, only the final cast left out."""
    t = lambda a: torch.from_numpy(a).to(dtype)
    a, b = t(f1).requires_grad_(True), t(f2).requires_grad_(True)
    blk = corr.CorrBlock(a, b, num_levels=L, radius=r)
    if dtype == torch.float32:
        out = blk(t(coords))
    else:
        keep = torch.Tensor.float
        torch.Tensor.float = lambda self: self               # the one cast of CorrBlock.__call__; restored below
        try:
            out = blk(t(coords))
        finally:
            torch.Tensor.float = keep
    assert out.dtype == dtype
    out.backward(t(g))
    return out.detach().numpy(), a.grad.numpy(), b.grad.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "raft_corr.npz"))
    a = ap.parse_args()
    corr = load_reference_corr()
    torch.manual_seed(0)
    rec = {"numpy_version": np.array(np.__version__), "torch_version": np.array(torch.__version__), "n_sample": np.int64(N_SAMPLE),
           "names": np.array([c[0] for c in CASES])}
    for name, C, H, W, L, r, seed, kind in CASES:
        f1, f2, g, coords = case_inputs(C, H, W, L, r, seed, kind)
        o32, a32, b32 = run_case(corr, f1, f2, g, coords, L, r, torch.float32)
        o64, a64, b64 = run_case(corr, f1, f2, g, coords, L, r, torch.float64)
        p = name + "/"
        rec[p + "settings"] = np.array([C, H, W, L, r, seed], np.int64)
        rec[p + "kind"] = np.array(kind)
        rec[p + "coords"] = coords
        rec[p + "input_sums"] = np.array([f1.astype(np.float64).sum(), f2.astype(np.float64).sum(), g.astype(np.float64).sum()])
        rec[p + "out_zero_bits"] = np.packbits(o32.reshape(-1) == 0)
        assert ((o32 == 0) == (o64 == 0)).all() or kind == "adversarial"
        for key, v32, v64 in (("out", o32, o64), ("grad_fmap1", a32, a64), ("grad_fmap2", b32, b64)):
            idx = sample_index(v64.size, seed)
            rec[p + key + "_f32"] = v32.reshape(-1)[idx].astype(np.float32)
            rec[p + key + "_f64"] = v64.reshape(-1)[idx].astype(np.float64)
            rec[p + key + "_err32"] = np.float64(np.abs(v32.astype(np.float64) - v64).max())
            rec[p + key + "_absmax"] = np.float64(np.abs(v64).max())
        print("%-24s err32 out %.2e  grad_fmap1 %.2e  grad_fmap2 %.2e   max|out| %.2f  zeros %.1f %%" % (
            name, rec[p + "out_err32"], rec[p + "grad_fmap1_err32"], rec[p + "grad_fmap2_err32"], rec[p + "out_absmax"], 100.0 * (o32 == 0).mean()))
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
