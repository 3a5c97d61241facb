#!/usr/bin/env python3
"""Time the plane-adjustment network (MPIPredictor(adjust_planes=True); mpf_pan.hip) at the generator's size, 64 planes x 384 x 1280:

    block 1 (first residual block + pool)   fused (ops.pan_block1) against the torch path of the same module, in this process
    whole dpn                               with the fused block and with the torch block
    whole forward                           HipPredictor (graph) without and with the adjusted planes (dpn + the copy of the planes + replay)

    python tools/bench_pan.py [--reps 7] [--iters 20] [--json PATH]

HIP events around `iters` back-to-back calls after a warm-up, the median over `reps` rounds, the rounds of the forms interleaved.  Random
parameters (there are no weights offline): the arithmetic does not depend on them."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--json", type=str, default=None)
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pan needs a GPU: a CPU run gives no time")
    from mpiflow_amd.model import MPIPredictor
    from mpiflow_amd.model.engine import HipPredictor
    dev = torch.device("cuda:0")
    S, H, W = o.planes, o.height, o.width
    m = MPIPredictor(W, H, S, adjust_planes=True).randomize_(1).eval().to(dev)
    with torch.no_grad():
        m.dpn.to_disp.linear.weight.mul_(0.01)
    g = torch.Generator().manual_seed(2)
    img, dsp = torch.rand(1, 3, H, W, generator=g).to(dev), torch.rand(1, 1, H, W, generator=g).to(dev)
    init = m.plane_disparities(img)
    rgb_low = F.interpolate(img, size=m.low_res_size, mode="bilinear", align_corners=True)
    disp_low = F.interpolate(dsp, size=m.low_res_size, mode="bilinear", align_corners=True)
    h, w = m.low_res_size
    dpn = m.dpn
    hp = HipPredictor(m, graph=True)

    def dpn_with(fused):
        x = dpn.block1(init, rgb_low, disp_low, fused)
        ctx = F.adaptive_avg_pool2d(dpn.context_encoder(x, start=1), (1, 1)).reshape(1, S, -1)
        return dpn.to_disp(dpn.embed(dpn.self_attention(ctx)), init)

    forms = {"block1_fused": lambda: dpn.block1(init, rgb_low, disp_low, True), "block1_torch": lambda: dpn.block1(init, rgb_low, disp_low, False),
             "dpn_fused": lambda: dpn_with(True), "dpn_torch": lambda: dpn_with(False),
             "forward_fixed_planes": lambda: hp(img, dsp), "forward_adjusted_planes": lambda: hp(img, dsp, plane_disp=m.render_disparities(img, dsp)[0])}
    times = {k: [] for k in forms}
    with torch.no_grad():
        for fn in forms.values():                                 # warm-up: the graph capture, MIOpen's choices, the caches
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(o.reps):
            for k, fn in forms.items():
                times[k].append(timed(fn, o.iters))
        diff = float((dpn_with(True) - dpn_with(False)).abs().max())
    med = {k: statistics.median(v) for k, v in times.items()}
    n_in, n_mid, n_out = S * 5 * h * w * 4, S * 8 * h * w * 4, S * 8 * (h // 2) * (w // 2) * 4
    res = dict(device=torch.cuda.get_device_name(0), planes=S, height=H, width=W, low_res=[h, w], reps=o.reps, iters=o.iters, ms_median=med,
               ms_min={k: min(v) for k, v in times.items()}, ms_max={k: max(v) for k, v in times.items()},
               block1_speedup=med["block1_torch"] / med["block1_fused"], block1_share_of_dpn_torch=med["block1_torch"] / med["dpn_torch"],
               rest_of_dpn_ms=med["dpn_fused"] - med["block1_fused"], adjust_planes_cost_ms=med["forward_adjusted_planes"] - med["forward_fixed_planes"],
               bytes=dict(torch_input=n_in, torch_intermediate_each=n_mid, fused_maps=(2 + 1) * 8 * h * w * 4, fused_output=n_out),
               dpn_fused_vs_torch_max_abs=diff)
    print(json.dumps(res))
    if o.json:
        os.makedirs(os.path.dirname(os.path.abspath(o.json)), exist_ok=True)
        with open(o.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
