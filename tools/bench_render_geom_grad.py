#!/usr/bin/env python3
"""Forward + backward of render_tgt_rgb_depth per image on one GPU with and without the disparity gradient (mpiflow_amd.utils.mpi.plane_geometry_grad):
the fused form with it (mpf_warp_composite_bwd_disp), the fused form without it (mpf_warp_composite_bwd, the path that existed before), and the generic
form with and without, with the peak memory of each.

    python tools/bench_render_geom_grad.py [--S 64 --H 384 --W 1280] [--iters 10 --warmup 3 --repeats 5] [--json PATH]

Method (that of tools/bench_render_grad.py): inputs are uploaded once; one timed iteration is one forward and one backward of rgb and depth with fixed
upstream gradients, every .grad reset to None before it.  The xyz tensors are built once per form, outside the timed region: with the disparity
gradient they come from a disparity that requires grad, built inside the context manager.  `warmup` untimed iterations per form, then `repeats` rounds;
a round times every form once, one after the other (`iters` iterations between two events on the current stream, one synchronize), so the forms
alternate in one process and share whatever the device's clocks do.  The figure is the median over the rounds, with min and max; the ratio with /
without is taken per round and its median reported.  Peak memory: torch.cuda.max_memory_allocated over one iteration minus what was allocated
before it."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("fused_with", "fused_without", "generic_with", "generic_without")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--H", type=int, default=384)
    ap.add_argument("--W", type=int, default=1280)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from mpiflow_amd.utils import mpi
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
    rgb = torch.from_numpy(rng.random((1, S, 3, H, W), dtype=np.float32)).to(dev).requires_grad_(True)
    sigma = torch.from_numpy(rng.random((1, S, 1, H, W), dtype=np.float32)).to(dev).requires_grad_(True)
    g_rgb = torch.from_numpy(rng.standard_normal((1, 3, H, W)).astype(np.float32)).to(dev)
    g_depth = torch.from_numpy(rng.standard_normal((1, 1, H, W)).astype(np.float32)).to(dev)
    sampler = HomographySample(H, W, dev)
    forms = a.forms.split(",")
    geo = {}
    for form in forms:
        with_disp = form.endswith("_with")
        disp = torch.linspace(1.0, 0.05, S).unsqueeze(0).to(dev).requires_grad_(with_disp)
        with mpi.plane_geometry_grad():
            xs = R.get_src_xyz_from_plane_disparity(sampler.meshgrid, disp, Kinv)
            xt = R.get_tgt_xyz_from_plane_disparity(xs, G)
        geo[form] = (disp, xs, xt)

    def step(form):
        disp, xs, xt = geo[form]
        rgb.grad = sigma.grad = disp.grad = None
        fused = True if form.startswith("fused") else False
        if form.endswith("_with"):
            with mpi.plane_geometry_grad():
                out = R.render_tgt_rgb_depth(sampler, rgb, sigma, disp, xt, xs, G, Kinv, K, fused=fused)
            torch.autograd.backward([out[0], out[1]], [g_rgb, g_depth], retain_graph=True)     # the graph of the xyz tensors is built once
            assert disp.grad is not None
        else:
            out = R.render_tgt_rgb_depth(sampler, rgb, sigma, disp, xt, xs, G, Kinv, K, fused=fused)
            torch.autograd.backward([out[0], out[1]], [g_rgb, g_depth])

    result = dict(S=S, H=H, W=W, iters=a.iters, warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0), forms={})
    peaks, times = {}, {form: [] for form in forms}
    for form in forms:
        for _ in range(a.warmup):
            step(form)
        torch.cuda.synchronize()
        rgb.grad = sigma.grad = geo[form][0].grad = None
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step(form)
        torch.cuda.synchronize()
        peaks[form] = torch.cuda.max_memory_allocated() - before
    for _ in range(a.repeats):
        for form in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                step(form)
            e1.record()
            torch.cuda.synchronize()
            times[form].append(e0.elapsed_time(e1) / a.iters)
    for form in forms:
        ts = times[form]
        result["forms"][form] = dict(ms_min=min(ts), ms_median=statistics.median(ts), ms_max=max(ts), peak_bytes=int(peaks[form]))
        print("%-16s forward + backward %8.3f ms per image (min %.3f, max %.3f over %d rounds of %d)   peak %8.1f MiB"
              % (form, statistics.median(ts), min(ts), max(ts), a.repeats, a.iters, peaks[form] / 2.0 ** 20), flush=True)
    for kind in ("fused", "generic"):
        if kind + "_with" in times and kind + "_without" in times:
            ratios = [x / y for x, y in zip(times[kind + "_with"], times[kind + "_without"])]
            result["ratio_" + kind] = dict(median=statistics.median(ratios), min=min(ratios), max=max(ratios))
            print("%-8s with / without the disparity gradient: %.3f x (per round: min %.3f, max %.3f)" % (kind, statistics.median(ratios), min(ratios), max(ratios)))
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
