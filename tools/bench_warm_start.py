#!/usr/bin/env python3
"""RAFT's warm start on the device: the time of ops.forward_interpolate (mpf_warm_start.hip: brute force, every target against every source)
at the coarse grids of Sintel (1 x 55 x 128) and KITTI (1 x 47 x 156) and at the largest a 1080p frame gives (1 x 135 x 240); beside it, where
scipy imports, what upstream's evaluate.py spends on the same flow; and one RAFT.predict at 436 x 1024 with 32 iterations (basic model) with
and without warm_start, which says what share of a frame the kernel is.

    python tools/bench_warm_start.py [--rounds 7] [--warmup 2] [--calls 200] [--out profiles/warm_start/bench.json]

The host form is upstream's expression restated: copy the flow to the host (.cpu(), which synchronises), push every pixel along its own flow,
keep the sources that land strictly inside the frame, query scipy.interpolate.griddata(..., method='nearest') once per channel on the integer
grid, stack the two answers and copy them back (.cuda()).  It is timed with a host clock around the whole expression, ending in a
synchronise; the op with device events around `calls` launches in a row.  Both run on one flow, a zoom with noise (about three quarters of
the sources valid), and the tool counts the words in which the two answers differ: faster and different is not faster.  The two predict forms
alternate round by round after a warm-up; every figure is the median of the rounds with min and max beside it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpiflow_amd import ops  # noqa: E402
from mpiflow_amd.raft import RAFT  # noqa: E402

GRIDS = [("sintel", 55, 128), ("kitti", 47, 156), ("1080p", 135, 240)]

try:
    from scipy.interpolate import griddata
except ImportError:
    griddata = None


def zoom_flow(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    smooth = np.stack([0.15 * (x - w / 2) + 3.3, 0.15 * (y - h / 2) - 2.1])
    return (smooth + 0.25 * rng.standard_normal((2, h, w))).astype(np.float32)


def host_form(flow_dev):
    """upstream's warm start on one sample [2,h,w] of a device tensor -> a device tensor"""
    flow = flow_dev.cpu().numpy()
    dx, dy = flow[0], flow[1]
    h, w = dx.shape
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    x1, y1 = (x0 + dx).reshape(-1), (y0 + dy).reshape(-1)
    keep = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)
    points = (x1[keep], y1[keep])
    fx = griddata(points, dx.reshape(-1)[keep], (x0, y0), method="nearest", fill_value=0)
    fy = griddata(points, dy.reshape(-1)[keep], (x0, y0), method="nearest", fill_value=0)
    return torch.from_numpy(np.stack([fx, fy], axis=0)).float().cuda()


def stats(ms):
    return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_warm_start.py needs a GPU"
    dev = torch.device("cuda:0")
    out = []
    for name, h, w in GRIDS:
        flow = torch.from_numpy(zoom_flow(h, w, 5)[None]).to(dev)
        res = torch.empty_like(flow)
        times = []
        for r in range(a.warmup + a.rounds):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(a.calls):
                ops.forward_interpolate(flow, out=res)
            t1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times.append(t0.elapsed_time(t1) / a.calls)
        rec = dict(what="ops.forward_interpolate", grid=name, shape="1x%dx%d" % (h, w), calls_per_round=a.calls, pairs=(h * w) ** 2, **stats(times))
        rec["pairs_per_second"] = round(rec["pairs"] / (rec["ms_median"] * 1e-3), 0)
        out.append(rec)
        print(json.dumps(rec))
        if griddata is not None:
            host = []
            for r in range(a.warmup + a.rounds):
                torch.cuda.synchronize()
                c0 = time.perf_counter()
                ans = host_form(flow[0])
                torch.cuda.synchronize()
                if r >= a.warmup:
                    host.append(1e3 * (time.perf_counter() - c0))
            differ = int((ans.view(torch.int32) != res[0].view(torch.int32)).sum())
            rec = dict(what="upstream's host form (cpu, two griddata, cuda)", grid=name, shape="1x%dx%d" % (h, w), words_differing_from_the_op=differ, **stats(host))
            out.append(rec)
            print(json.dumps(rec))
    if griddata is None:
        rec = dict(what="upstream's host form (cpu, two griddata, cuda)", missing="scipy does not import on this machine")
        out.append(rec)
        print(json.dumps(rec))

    # the share of a frame: one predict at Sintel's size with and without the warm start
    torch.manual_seed(1)
    model = RAFT(argparse.Namespace(small=False, mixed_precision=False)).to(dev).eval()
    H, W, iters = 436, 1024, 32
    im1 = torch.randint(0, 256, (1, 3, H, W), device=dev).float()
    im2 = torch.roll(im1, (2, 5), dims=(2, 3))
    prev = torch.from_numpy(zoom_flow(55, 128, 6)[None]).to(dev)
    forms = dict(predict_cold=dict(), predict_warm_start=dict(warm_start=prev))
    times = {k: [] for k in forms}
    for r in range(a.warmup + a.rounds):
        for k, kw in forms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            model.predict(im1, im2, iters=iters, **kw)
            t1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[k].append(t0.elapsed_time(t1))
    op_ms = out[0]["ms_median"]
    for k, v in times.items():
        rec = dict(what=k, model="basic", shape="1x%dx%d" % (H, W), iters=iters, **stats(v))
        if k == "predict_warm_start":
            rec["forward_interpolate_share_of_the_frame"] = round(op_ms / rec["ms_median"], 5)
        out.append(rec)
        print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
