#!/usr/bin/env python3
"""The GPU NS hole fill (ops.inpaint_ns, mpf_inpaint_ns) on tools/bench_inpaint_threads.py's frame - 384 x 1280, eight 300 x 12 disocclusion
bands + 1 % scattered pixels - in batches of B = 1, 8 and 40 copies: device time per call from events (median of --reps after a warm-up),
the cluster count and the largest cluster of one frame.  Byte identity with ops.inpaint_host is checked once per B.
--phases: one more call per B through the witness build, whose fill kernel sums shader clocks per phase of the front over its waves
(pop, rejected neighbour tests, neighbour test + arrival, disc offsets, ordered fold, output + push): the share of each and clocks per fill.
  python tools/bench_inpaint_ns.py [--reps 20] [--batches 1,8,40] [--phases]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpiflow_amd import ops  # noqa: E402


def frame(H=384, W=1280):
    rs = np.random.RandomState(0)
    img = (rs.rand(H, W, 3) * 255).astype(np.uint8)
    mask = np.zeros((H, W), np.uint8)
    for x0 in range(60, W, 160):
        mask[40:340, x0:x0 + 12] = 1
    mask |= (rs.rand(H, W) < 0.01).astype(np.uint8)
    return img, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,8,40")
    ap.add_argument("--phases", action="store_true")
    a = ap.parse_args()
    img, mask = frame()
    H, W = mask.shape
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    want = ops.inpaint_host(img, mask, 3, ops.INPAINT_NS)
    host_ms = (time.perf_counter() - t0) * 1e3
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        ys, xs = np.nonzero(mask)
        idx = -np.ones((H, W), np.int64)
        idx[ys, xs] = np.arange(len(ys))
        a_, b_ = [], []
        for dy in range(-4, 5):
            for dx in range(-4, 5):
                y2, x2 = ys + dy, xs + dx
                ok = (y2 >= 0) & (y2 < H) & (x2 >= 0) & (x2 < W)
                j = np.full(len(ys), -1)
                j[ok] = idx[y2[ok], x2[ok]]
                a_.append(np.nonzero(j >= 0)[0])
                b_.append(j[j >= 0])
        a_, b_ = np.concatenate(a_), np.concatenate(b_)
        n, lab = connected_components(coo_matrix((np.ones(len(a_)), (a_, b_)), shape=(len(ys), len(ys))), directed=False)
        clusters = dict(count=int(n), largest=int(np.bincount(lab).max()))
    except ImportError:
        clusters = None
    print("frame %d x %d, %d hole pixels, clusters at link distance 4: %s; host NS fill, one thread: %.1f ms"
          % (H, W, int(mask.sum()), clusters, host_ms))
    for B in [int(x) for x in a.batches.split(",")]:
        ti = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(img, (B,) + img.shape))).to(dev)
        tm = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(mask, (B,) + mask.shape))).to(dev)
        ws = torch.empty(ops.inpaint_ns_workspace(B, H, W), dtype=torch.uint8, device=dev)
        out = torch.empty_like(ti)
        ops.inpaint_ns(ti, tm, 3, out=out, workspace=ws)
        torch.cuda.synchronize()
        same = bool((out.cpu().numpy() == want[None]).all())
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.inpaint_ns(ti, tm, 3, out=out, workspace=ws)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        print("B=%2d: %.3f ms per call (median of %d; min %.3f, max %.3f), %.3f ms per frame, byte-identical to inpaint_host: %s, workspace %.1f MB"
              % (B, float(np.median(ms)), a.reps, min(ms), max(ms), float(np.median(ms)) / B, same, ws.numel() / 1e6))
        print("  counters:", ops.inpaint_ns_counters(ws))
        if a.phases:
            phases(ti, tm, out, ws)


PHASES = ("setup (band scan)", "pop", "rejected neighbour tests", "neighbour test + arrival", "disc offsets", "ordered fold", "output + push")


def phases(ti, tm, out, ws):
    from mpiflow_amd import _lib
    with _lib.witness():
        ops.inpaint_ns(ti, tm, 3, out=out, workspace=ws)
        torch.cuda.synchronize()
    clk = ws[64:64 + 8 * 9].view(torch.int64).cpu().tolist()          # NS_PHASE_WORD = 16 (32-bit words): NsPhase, 9 words
    fills, pops, tot = clk[7], clk[8], sum(clk[:7])
    print("  phases (witness build, clocks summed over waves): %d fills, %d pops, %.0f clocks per fill in all" % (fills, pops, tot / max(fills, 1)))
    for name, c in zip(PHASES, clk[:7]):
        print("    %-26s %5.1f %%  %7.0f clocks per fill" % (name, 100.0 * c / max(tot, 1), c / max(fills, 1)))


if __name__ == "__main__":
    main()
