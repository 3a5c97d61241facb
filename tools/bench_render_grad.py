#!/usr/bin/env python3
"""Forward + backward of render_tgt_rgb_depth per image on one GPU: the HIP generic form, the HIP fused form and the torch restatement of the
reference formulas (tests/render_grad_restated.py) on the same device, with the peak memory of each.

    python tools/bench_render_grad.py [--S 64 --H 384 --W 1280] [--iters 10 --warmup 3] [--json PATH]

Method: inputs are uploaded once; each timed iteration is one forward and one backward (torch.autograd.backward of rgb and depth with fixed upstream
gradients, .grad reset to None before it); `warmup` untimed iterations, then `iters` iterations between two CUDA events on the current stream, one
synchronize at the end; the figure is the mean per iteration, and the run is repeated `--repeats` times to show its spread (min / median / max).
Peak memory: torch.cuda.max_memory_allocated over one iteration minus what was allocated before it."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--H", type=int, default=384)
    ap.add_argument("--W", type=int, default=1280)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forms", default="fused,generic,torch")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import render_grad_restated as rr
    from mpiflow_amd.utils.mpi import mpi_rendering as R
    from mpiflow_amd.utils.mpi.homography_sampler import HomographySample
    dev = torch.device("cuda")
    S, H, W = a.S, a.H, a.W
    rng = np.random.default_rng(0)
    f = 0.9 * W
    K = torch.tensor([[[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1]]], dtype=torch.float32)
    Kinv = torch.linalg.inv(K.double()).float()
    G = torch.eye(4).unsqueeze(0)
    G[0, :3, 3] = torch.tensor([-0.06, 0.045, 0.03])
    disp = torch.linspace(1.0, 0.05, S).unsqueeze(0)
    rgb = torch.from_numpy(rng.random((1, S, 3, H, W), dtype=np.float32)).to(dev).requires_grad_(True)
    sigma = torch.from_numpy(rng.random((1, S, 1, H, W), dtype=np.float32)).to(dev).requires_grad_(True)
    g_rgb = torch.from_numpy(rng.standard_normal((1, 3, H, W)).astype(np.float32)).to(dev)
    g_depth = torch.from_numpy(rng.standard_normal((1, 1, H, W)).astype(np.float32)).to(dev)
    sampler = HomographySample(H, W, dev)
    xs = R.get_src_xyz_from_plane_disparity(sampler.meshgrid, disp.to(dev), Kinv)
    xt = R.get_tgt_xyz_from_plane_disparity(xs, G)
    Gd, Kd, Kinvd, dispd = G.to(dev), K.to(dev), Kinv.to(dev), disp.to(dev)

    def step(form):
        rgb.grad = sigma.grad = None
        if form == "torch":
            out = rr.render_tgt_rgb_depth(rgb, sigma, dispd, Gd, Kinvd, Kd)
        else:
            out = R.render_tgt_rgb_depth(sampler, rgb, sigma, dispd, xt, xs, G, Kinv, K, fused=None if form == "fused" else False)
        torch.autograd.backward([out[0], out[1]], [g_rgb, g_depth])

    result = dict(S=S, H=H, W=W, iters=a.iters, warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0), forms={})
    for form in a.forms.split(","):
        for _ in range(a.warmup):
            step(form)
        torch.cuda.synchronize()
        rgb.grad = sigma.grad = None
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step(form)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        times = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                step(form)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / a.iters)
        result["forms"][form] = dict(ms_min=min(times), ms_median=statistics.median(times), ms_max=max(times), peak_bytes=int(peak))
        print("%-8s forward + backward %8.3f ms per image (min %.3f, max %.3f over %d runs of %d)   peak %8.1f MiB"
              % (form, statistics.median(times), min(times), max(times), a.repeats, a.iters, peak / 2.0 ** 20), flush=True)
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
