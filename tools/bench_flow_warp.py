#!/usr/bin/env python3
"""Time the flow warps (mpiflow_amd.utils.transform.warp / warp_rife: mpf_flow_warp.hip) against the torch-op restatement of the reference
(utils/transform.py:60-111 with F.grid_sample on the device), forward and forward + backward, in one process.

    python tools/bench_flow_warp.py [--reps 5] [--iters 100] [--json PATH]

Per shape and function: the two forms alternate, `reps` times `iters` calls each after a warm-up of both, timed with device events around the
batch of calls; the median over the repetitions and their spread (min..max) are printed in ms per call, with the peak memory torch's allocator
saw above the inputs during one call.  Shapes: 8 x 3 x 384 x 1280 (a frame batch) and 8 x 256 x 48 x 160 (RAFT's fmap2 at 1/8).  Needs a GPU."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpiflow_amd.utils import transform as T  # noqa: E402

SHAPES = ((8, 3, 384, 1280), (8, 256, 48, 160))


def torch_warp(x, flo):
    B, C, H, W = x.size()
    xx = torch.arange(0, W, device=x.device).view(1, -1).repeat(H, 1).view(1, 1, H, W).repeat(B, 1, 1, 1)
    yy = torch.arange(0, H, device=x.device).view(-1, 1).repeat(1, W).view(1, 1, H, W).repeat(B, 1, 1, 1)
    vgrid = torch.cat((xx, yy), 1).float() + flo
    vgrid = torch.stack((2.0 * vgrid[:, 0] / max(W - 1, 1) - 1.0, 2.0 * vgrid[:, 1] / max(H - 1, 1) - 1.0), dim=3)
    output = F.grid_sample(x, vgrid, align_corners=False)
    mask = F.grid_sample(torch.ones_like(x), vgrid, align_corners=False).detach()
    return output, mask


_grid = {}


def torch_warp_rife(x, flow):
    k = (str(flow.device), tuple(flow.shape))
    if k not in _grid:
        B, _, H, W = flow.shape
        hor = torch.linspace(-1.0, 1.0, W, device=flow.device).view(1, 1, 1, W).expand(B, -1, H, -1)
        ver = torch.linspace(-1.0, 1.0, H, device=flow.device).view(1, 1, H, 1).expand(B, -1, -1, W)
        _grid[k] = torch.cat([hor, ver], 1)
    flow = torch.cat([flow[:, 0:1] / ((x.shape[3] - 1.0) / 2.0), flow[:, 1:2] / ((x.shape[2] - 1.0) / 2.0)], 1)
    g = (_grid[k] + flow).permute(0, 2, 3, 1)
    return F.grid_sample(input=x, grid=g, mode="bilinear", padding_mode="border", align_corners=True)


def first(r):
    return r[0] if isinstance(r, tuple) else r


def make_call(fn, x, flow, g, backward):
    if not backward:
        def call():
            with torch.no_grad():
                return first(fn(x, flow))
        return call
    xg, fg = x.clone().requires_grad_(True), flow.clone().requires_grad_(True)

    def call():
        xg.grad = fg.grad = None
        first(fn(xg, fg)).backward(g)
    return call


def timed(call, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def peak(call):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    call()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flow_warp needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    rows = []
    for B, C, H, W in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(5)
        x = torch.randn(B, C, H, W, device=dev, generator=gen)
        g = torch.randn(B, C, H, W, device=dev, generator=gen)
        # a smooth field of a few pixels plus pixel noise, as a predicted flow is; samples near the rim leave the frame
        base = F.interpolate(torch.randn(B, 2, H // 16, W // 16, device=dev, generator=gen) * 12.0, size=(H, W), mode="bilinear", align_corners=False)
        flow = (base + 0.5 * torch.randn(B, 2, H, W, device=dev, generator=gen)).contiguous()
        for name, ours, ref in (("warp", T.warp, torch_warp), ("warp_rife", T.warp_rife, torch_warp_rife)):
            o, r = first(ours(x, flow)), first(ref(x, flow))
            dev_err = float((o - r).abs().max() / r.abs().max())
            for backward in (False, True):
                calls = dict(hip=make_call(ours, x, flow, g, backward), torch=make_call(ref, x, flow, g, backward))
                for c in calls.values():
                    for _ in range(5):
                        c()
                torch.cuda.synchronize()
                t = dict(hip=[], torch=[])
                for _ in range(a.reps):
                    for k, c in calls.items():
                        t[k].append(timed(c, a.iters))
                row = dict(shape=[B, C, H, W], fn=name, what="forward + backward" if backward else "forward", max_rel_diff_forward=dev_err)
                for k in calls:
                    s = sorted(t[k])
                    row[k + "_ms"], row[k + "_min"], row[k + "_max"], row[k + "_peak_mib"] = s[len(s) // 2], s[0], s[-1], peak(calls[k])
                rows.append(row)
                print("%dx%dx%dx%d %-9s %-18s hip %.3f ms (%.3f..%.3f) %.1f MiB | torch %.3f ms (%.3f..%.3f) %.1f MiB | x%.2f | forward diff %.1e" % (
                    B, C, H, W, name, row["what"], row["hip_ms"], row["hip_min"], row["hip_max"], row["hip_peak_mib"], row["torch_ms"], row["torch_min"],
                    row["torch_max"], row["torch_peak_mib"], row["torch_ms"] / row["hip_ms"], dev_err), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
