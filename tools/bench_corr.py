#!/usr/bin/env python3
"""Time RAFT's correlation lookup three ways on one GPU, in one process, alternating: (a) the all-pairs form in torch (CorrBlock restated: the
(HW)^2 volume by matmul, its avg_pool2d pyramid once, then 12 grid_sample lookups), (b) mpiflow_amd.raft_corr.AlternateCorrBlock (the
channel-last maps once, then 12 launches of mpf_corr_lookup) and (c) mpiflow_amd.raft_corr.CorrBlock (the all-pairs form with its pyramid,
lookups and gradients in HIP), forward only and with the backward pass of all 12 lookups; plus the peak memory of each, the time of ONE
forward lookup of the on-demand kernel beside the plain one-thread-per-entry kernel it grew from, and the four ops of (c) alone.

    python tools/bench_corr.py [--reps 10] [--warmup 2] [--lookups 12] [--shapes 8x36x120,8x48x160,2x128x192] [--channels 256] [--json PATH]

Device time from events, median of --reps after --warmup.  Prints one table and, with --json, writes the numbers."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpiflow_amd import ops, raft_corr  # noqa: E402

L, R = 4, 4


class AllPairs:
    def __init__(self, f1, f2):
        B, C, H, W = f1.shape
        vol = torch.matmul(f1.reshape(B, C, H * W).transpose(1, 2), f2.reshape(B, C, H * W)) / torch.sqrt(torch.tensor(C).float())
        vol = vol.reshape(B * H * W, 1, H, W)
        self.pyr = [vol]
        for _ in range(L - 1):
            self.pyr.append(F.avg_pool2d(self.pyr[-1], 2, stride=2))
        d = torch.linspace(-R, R, 2 * R + 1, device=f1.device)
        self.delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1)[None]

    def __call__(self, coords):
        B, _, H, W = coords.shape
        cen = coords.permute(0, 2, 3, 1).reshape(B * H * W, 1, 1, 2)
        outs = []
        for i, vol in enumerate(self.pyr):
            h, w = vol.shape[-2:]
            p = cen / 2 ** i + self.delta
            grid = torch.stack([2 * p[..., 0] / (w - 1) - 1, 2 * p[..., 1] / (h - 1) - 1], dim=-1)
            outs.append(F.grid_sample(vol, grid, align_corners=True).reshape(B, H, W, -1))
        return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def step(make, f1, f2, coords, lookups, backward):
    """one RAFT step's worth: construct once, `lookups` lookups at drifting coordinates, optionally the backward pass of their sum"""
    if backward:
        f1, f2 = f1.detach().requires_grad_(True), f2.detach().requires_grad_(True)
    with torch.set_grad_enabled(backward):
        fn = make(f1, f2)
        total = None
        for k in range(lookups):
            out = fn(coords[k])
            if backward:
                s = out.sum()
                total = s if total is None else total + s
        if backward:
            total.backward()


def timed(fn, reps, warmup):
    ts = []
    for k in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= warmup:
            ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lookups", type=int, default=12)
    ap.add_argument("--shapes", default="8x36x120,8x48x160,2x128x192")
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for shape in a.shapes.split(","):
        B, H, W = [int(v) for v in shape.split("x")]
        C = a.channels
        gen = torch.Generator(device="cpu").manual_seed(1)
        f1, f2 = [torch.randn(B, C, H, W, generator=gen).to(dev) for _ in range(2)]
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        grid = torch.stack([xs, ys])[None]
        # a smooth flow field (RAFT's flow at 1/8 resolution is smooth) that grows from lookup to lookup, plus a little noise
        flow = torch.stack([3.0 * torch.sin(ys / 9.0) + 2.0, 2.0 * torch.cos(xs / 11.0)])[None]
        coords = [(grid + flow * (k + 1) / a.lookups + 0.25 * torch.randn(B, 2, H, W, generator=gen)).to(dev).contiguous() for k in range(a.lookups)]
        row = dict(B=B, C=C, H=H, W=W, lookups=a.lookups)
        forms = (("allpairs", AllPairs), ("ondemand", lambda x, y: raft_corr.AlternateCorrBlock(x, y, num_levels=L, radius=R)),
                 ("volume", lambda x, y: raft_corr.CorrBlock(x, y, num_levels=L, radius=R)))
        for backward in (False, True):
            ts = {n: [] for n, _ in forms}
            for k in range(a.warmup + a.reps):                       # alternating: one step of each form per round
                for n, make in forms:
                    t = timed(lambda: step(make, f1, f2, coords, a.lookups, backward), 1, 0)[0]
                    if k >= a.warmup:
                        ts[n].append(t)
            for n, _ in forms:
                row["%s_%s_ms" % (n, "fwd_bwd" if backward else "fwd")] = statistics.median(ts[n])
        for n, make in forms:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            step(make, f1, f2, coords, a.lookups, True)
            torch.cuda.synchronize()
            row["%s_peak_MB" % n] = (torch.cuda.max_memory_allocated(dev) - base) / 1e6
        blk = raft_corr.AlternateCorrBlock(f1, f2, num_levels=L, radius=R)
        out = torch.empty(B, L * 81, H, W, device=dev)
        ts = {0: [], 1: []}
        for k in range(a.warmup + a.reps):
            for plain in (0, 1):
                t = timed(lambda: ops.corr_lookup(blk.fmap1_nhwc, blk.f2_levels_nhwc, coords[-1], R, out=out, plain=bool(plain)), 1, 0)[0]
                if k >= a.warmup:
                    ts[plain].append(t)
        g = torch.randn_like(out)
        tb = timed(lambda: ops.corr_lookup_backward(blk.fmap1_nhwc, blk.f2_levels_nhwc, coords[-1], g, R), a.reps, a.warmup)
        row["lookup_kernel_ms"], row["lookup_plain_kernel_ms"] = statistics.median(ts[0]), statistics.median(ts[1])
        row["lookup_backward_kernel_ms"] = statistics.median(tb)
        flop = 2.0 * B * H * W * L * 100 * C                           # the (rd+1)^2 grid dot products of every pixel and level
        row["lookup_TFLOPs"] = flop / (row["lookup_kernel_ms"] * 1e-3) / 1e12
        row["lookup_grid_bytes_MB"] = B * H * W * L * 100 * C * 4 / 1e6
        del blk
        # the four ops of CorrBlock alone, on buffers of their own.  The pyramid op rescales its level 0 at every call (values shrink, time does
        # not) and allocates levels 1.. each time (caching-allocator hits): it is the op, not the bare kernel; the other three allocate nothing
        norm = float(torch.sqrt(torch.tensor(C).float()))
        raw = torch.matmul(f1.view(B, C, H * W).transpose(1, 2), f2.view(B, C, H * W)).view(B * H * W, H, W)
        levels = ops.corr_pyramid(raw, L, norm)
        grads = [torch.zeros_like(t) for t in levels]
        kernels = (("volume_pyramid_kernel_ms", lambda: ops.corr_pyramid(raw, L, norm)),
                   ("volume_lookup_kernel_ms", lambda: ops.corr_volume_lookup(levels, coords[-1], R, out=out)),
                   ("volume_lookup_backward_kernel_ms", lambda: ops.corr_volume_lookup_backward(grads, coords[-1], g, R)),
                   ("volume_fold_kernel_ms", lambda: ops.corr_pyramid_backward(grads, norm)))
        for name, fn in kernels:
            row[name] = statistics.median(timed(fn, a.reps, a.warmup))
        row["volume_pyramid_MB"] = sum(t.numel() for t in levels) * 4 / 1e6
        row["volume_lookup_bytes_MB"] = B * H * W * L * (100 + 81) * 4 / 1e6       # the patches read + the outputs written
        del raw, levels, grads
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("\n| B x H x W | all-pairs fwd ms | on-demand fwd ms | all-pairs fwd+bwd ms | on-demand fwd+bwd ms | all-pairs peak MB | on-demand peak MB | "
          "lookup kernel ms | plain kernel ms | backward kernel ms | lookup TFLOP/s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %d x %d x %d | %.2f | %.2f | %.2f | %.2f | %.0f | %.0f | %.3f | %.3f | %.3f | %.1f |" % (
            r["B"], r["H"], r["W"], r["allpairs_fwd_ms"], r["ondemand_fwd_ms"], r["allpairs_fwd_bwd_ms"], r["ondemand_fwd_bwd_ms"],
            r["allpairs_peak_MB"], r["ondemand_peak_MB"], r["lookup_kernel_ms"], r["lookup_plain_kernel_ms"], r["lookup_backward_kernel_ms"], r["lookup_TFLOPs"]))
    print("\n| B x H x W | CorrBlock fwd ms | CorrBlock fwd+bwd ms | CorrBlock peak MB | pyramid MB | pyramid op ms | lookup kernel ms | "
          "lookup backward kernel ms | fold kernel ms |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %d x %d x %d | %.2f | %.2f | %.0f | %.0f | %.3f | %.3f | %.3f | %.3f |" % (
            r["B"], r["H"], r["W"], r["volume_fwd_ms"], r["volume_fwd_bwd_ms"], r["volume_peak_MB"], r["volume_pyramid_MB"], r["volume_pyramid_kernel_ms"],
            r["volume_lookup_kernel_ms"], r["volume_lookup_backward_kernel_ms"], r["volume_fold_kernel_ms"]))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
