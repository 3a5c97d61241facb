#!/usr/bin/env python3
"""Record RAFT's warm start by RUNNING THE REFERENCE ITSELF (forward_interpolate of RAFT/core/utils/utils.py: scipy's griddata, CPU)
-> tests/golden/raft_warm_start.npz.

    python tests/golden/make_warm_start_golden.py [--out PATH]   (in the build container: needs the reference tree, numpy, scipy, torch)

Per sample the reference's float32 output [2,h,w] is stored whole.  The inputs are draws of np.random.default_rng(seed), rebuilt by the test
with sample_flow() below; the file carries their float64 sums.  Two families:

    noise   sigma * standard_normal((2,h,w))
    zoom    ((zoom - 1) * (x - w / 2) + sx, (zoom - 1) * (y - h / 2) + sy) + 0.25 * standard_normal((2,h,w))

both cast to float32.  Cases (CASES): a grid far below one tile, 5 x 7; two samples of one size with about 80 % and about 28 % valid
sources; odd sides; 55 x 128 (Sintel's coarse grid: more than one target tile, source tile and source chunk, a valid count that is no
multiple of anything) as noise and as a zoom in; 47 x 156 (KITTI's) as a zoom out, where every source is valid.

The recorder restates the rule the package implements (brute_force(): float64 d2 with each product and the sum rounded on its own, the first
minimum over original flat indices) and asserts, per sample: its selection equals the reference's output bit for bit; no target has two
sources at exactly the same least d2; the smallest relative gap between the least and the second least d2, (second - least) / second, is at
least MIN_GAP = 1e-9, so that neither the tie rule nor a last-bit difference in d2 can decide any pixel; at least 10 % of the sources are
invalid, except in the all-valid case, where none is.  The valid counts, the gaps and the tie counts are stored."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MIN_GAP = 1e-9

# (name, h, w, samples); a sample: (kind, sigma or zoom, (sx, sy), seed)
CASES = [("1x5x7", 5, 7, [("noise", 2.0, (0.0, 0.0), 7100)]),
         ("2x16x24", 16, 24, [("noise", 3.0, (0.0, 0.0), 7110), ("noise", 12.0, (0.0, 0.0), 7111)]),
         ("1x17x33", 17, 33, [("noise", 6.0, (0.0, 0.0), 7120)]),
         ("2x55x128", 55, 128, [("noise", 8.0, (0.0, 0.0), 7130), ("zoom", 1.15, (3.3, -2.1), 7131)]),
         ("1x47x156", 47, 156, [("zoom", 0.85, (-6.2, 1.4), 7140)])]
ALL_VALID = ("1x47x156",)


def sample_flow(kind, param, shift, seed, h, w):
    """one sample [2,h,w] float32"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return (rng.standard_normal((2, h, w)) * param).astype(np.float32)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    smooth = np.stack([(param - 1) * (x - w / 2) + shift[0], (param - 1) * (y - h / 2) + shift[1]])
    return (smooth + 0.25 * rng.standard_normal((2, h, w))).astype(np.float32)


def case_inputs(h, w, samples):
    """[N,2,h,w] float32"""
    return np.stack([sample_flow(kind, param, shift, seed, h, w) for kind, param, shift, seed in samples])


def sources(flow):
    """x1, y1 (float64, flat) and the validity of every pixel of one sample as a source: upstream's expressions"""
    h, w = flow.shape[1:]
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    x1, y1 = (x0 + flow[0]).reshape(-1), (y0 + flow[1]).reshape(-1)           # int64 + float32 -> float64
    assert x1.dtype == np.float64
    return x1, y1, (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)


def brute_force(flow, block=256):
    """the rule, restated: -> (out [2,h,w] float32, least d2 [h*w], second least d2 [h*w] (inf with fewer than two valid sources)).  No valid
    source: zeros"""
    h, w = flow.shape[1:]
    x1, y1, valid = sources(flow)
    idx = np.nonzero(valid)[0]                               # ascending original flat indices: argmin's first minimum is the lowest
    out = np.zeros((2, h * w), np.float32)
    least, second = np.full(h * w, np.inf), np.full(h * w, np.inf)
    if len(idx):
        sx, sy = x1[idx], y1[idx]
        for t0 in range(0, h * w, block):
            t = np.arange(t0, min(t0 + block, h * w))
            ex, ey = sx[None, :] - (t % w)[:, None].astype(np.float64), sy[None, :] - (t // w)[:, None].astype(np.float64)
            d2 = ex * ex + ey * ey
            sel = np.argmin(d2, axis=1)
            out[:, t] = flow.reshape(2, -1)[:, idx[sel]]
            least[t] = d2[np.arange(len(t)), sel]
            if len(idx) > 1:
                d2[np.arange(len(t)), sel] = np.inf
                second[t] = d2.min(axis=1)
    return out.reshape(2, h, w), least, second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "raft_warm_start.npz"))
    a = ap.parse_args()
    import scipy
    import torch
    sys.path.insert(0, HERE)
    from ref_harness import REFERENCE_ROOT
    sys.path.insert(0, os.path.join(REFERENCE_ROOT, "RAFT", "core"))
    sys.dont_write_bytecode = True
    from utils.utils import forward_interpolate              # the reference's own
    rec = {"numpy_version": np.array(np.__version__), "scipy_version": np.array(scipy.__version__), "names": np.array([c[0] for c in CASES]),
           "min_gap_required": np.float64(MIN_GAP)}
    for name, h, w, samples in CASES:
        flows = case_inputs(h, w, samples)
        outs, stats = [], []
        for flow in flows:
            ref = forward_interpolate(torch.from_numpy(flow)).numpy()
            assert ref.dtype == np.float32 and ref.shape == flow.shape and np.isfinite(ref).all()
            mine, least, second = brute_force(flow)
            nvalid = int(sources(flow)[2].sum())
            ties = int((second == least).sum())
            gap = float(((second - least) / second).min())
            differ = int((mine.view(np.uint32) != ref.view(np.uint32)).sum())
            assert differ == 0, (name, "the restated rule differs from the reference in %d words" % differ)
            assert ties == 0 and gap >= MIN_GAP, (name, ties, gap)
            if name in ALL_VALID:
                assert nvalid == h * w, (name, nvalid)
            else:
                assert nvalid <= 0.9 * h * w, (name, nvalid, h * w)
            outs.append(ref)
            stats.append([nvalid, ties, gap])
            print("%-9s %-5s %-5g seed %d: %5d of %5d sources valid (%.0f %%), restated rule == reference bit for bit, 0 ties, smallest relative gap %.2e"
                  % (name, samples[len(outs) - 1][0], samples[len(outs) - 1][1], samples[len(outs) - 1][3], nvalid, h * w, 100.0 * nvalid / (h * w), gap))
        p = name + "/"
        rec[p + "settings"] = np.array([len(samples), h, w], np.int64)
        rec[p + "kinds"] = np.array([s[0] for s in samples])
        rec[p + "params"] = np.array([[s[1], s[2][0], s[2][1], s[3]] for s in samples], np.float64)
        rec[p + "input_sum"] = np.float64(flows.astype(np.float64).sum())
        rec[p + "out"] = np.stack(outs)
        rec[p + "valid_ties_gap"] = np.array(stats, np.float64)
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 200 * 1000
    return 0


if __name__ == "__main__":
    sys.exit(main())
