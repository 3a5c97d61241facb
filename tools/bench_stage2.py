#!/usr/bin/env python3
"""Warp-back stage 2 on the device (mpf_canny.hip, mpf_stage2.hip, warpback.warp_and_inpaint) at B = 8, 256 x 384, on one stream: each stage
of ops.canny_masked alone through `passes`, the whole call, the four pointwise launches, warp_and_inpaint with the closed-form weights of
tests/stage2_pattern.py, and beside them the host path the edge detector replaces: copy to the host, one float64 scipy Canny per image
(tests/canny_restated.py: canny_witness, the shape of skimage's), copy back.

    python tools/bench_stage2.py [--rounds 7] [--warmup 2] [--calls 500] [--out profiles/stage2/bench.json]

Device events around `calls` launches in a row, after a warm-up; every figure is the median of the rounds with min and max beside it.  The
calls take 15 to 100 microseconds each, so a timed window is 500 of them (8 to 50 ms): a window of a few calls would time the launch, not
the work.  These are call times; kernel times come from a kernel trace of a run of their own (profiles/stage2/README.md).  The
scene is a near block on a sloped background under a checkered, shaded image, rendered at the reference's pose (x = 0.2): the edge detector
sees the render and its visibility mask.  The host path is timed with a wall clock around one whole batch, synchronised at both ends.
Algorithmic bytes per pixel of the Canny stages: stage 1 reads 8 and writes 4; stage 2 reads 8 and writes 1; stage 3 reads 1 and writes 4."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import canny_restated  # noqa: E402
import stage2_pattern  # noqa: E402
from mpiflow_amd import ops  # noqa: E402
from mpiflow_amd.warpback import RGBDRenderer, networks, warp_and_inpaint  # noqa: E402

B, H, W = 8, 256, 384


def scene(b, h, w):
    y, x = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
    rgb = np.stack([[0.5 + 0.3 * np.sin(9 * x + c + i) * np.cos(7 * y - c) for c in range(3)] for i in range(b)])
    rgb += 0.3 * (((np.floor(12 * x) + np.floor(8 * y)) % 2) == 0)
    block = (np.abs(x - 0.5) < 0.2) & (np.abs(y - 0.5) < 0.25)
    disp = np.broadcast_to(np.where(block, 0.9, 0.25 + 0.03 * x + 0.02 * y), (b, 1, h, w))
    return np.clip(rgb, 0, 1).astype(np.float32), np.ascontiguousarray(disp, dtype=np.float32)


def timed(fn, a, calls=None):
    calls = calls or a.calls
    ms = []
    for r in range(a.warmup + a.rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        if r >= a.warmup:
            ms.append(t0.elapsed_time(t1) / calls)
    return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stage2.py needs a GPU"
    dev = torch.device("cuda:0")
    rgb, disp = scene(B, H, W)
    image, disp = torch.from_numpy(rgb).to(dev), torch.from_numpy(disp).to(dev)
    cam_int = torch.tensor([[0.58, 0, 0.5], [0, 0.58, 0.5], [0, 0, 1]], device=dev).repeat(B, 1, 1)
    ext = torch.eye(4, device=dev)[:3].repeat(B, 1, 1)
    ext[:, 0, 3] = 0.2
    inv = ext.clone()
    inv[:, 0, 3] = -0.2
    r = RGBDRenderer(dev)
    warp_image, warp_disp, mask = (t.contiguous() for t in r.render_mesh(r.construct_mesh(torch.cat([image, disp], 1), cam_int), cam_int, ext))
    shape = "%dx%dx%d" % (B, H, W)
    px = B * H * W
    out = []

    def put(rec):
        out.append(rec)
        print(json.dumps(rec), flush=True)

    gray, hole = ops.stage2_gray_hole(warp_image, mask)
    ws = ops.canny_workspace(B, H, W, dev)
    edge = torch.empty_like(gray)
    whole = ops.canny_masked(gray, mask, out=edge, workspace=ws)
    classes = ops.canny_workspace_views(ws, B, H, W)[1]
    put(dict(what="scene", shape=shape, hole_share=round(float((mask == 0).float().mean()), 4), edge_pixels=int(whole.sum()),
             weak=int((classes == 1).sum()), strong=int((classes == 2).sum())))
    for name, nbytes in (("smooth", 12), ("classify", 9), ("hysteresis", 5)):
        put(dict(what="ops.canny_masked, passes=%r alone" % name, shape=shape, algorithmic_bytes=nbytes * px,
                 **timed(lambda: ops.canny_masked(gray, mask, out=edge, workspace=ws, passes=name), a)))
    put(dict(what="ops.canny_masked, whole, out and workspace given", shape=shape, **timed(lambda: ops.canny_masked(gray, mask, out=edge, workspace=ws), a)))
    put(dict(what="ops.canny_masked, whole, allocating", shape=shape, **timed(lambda: ops.canny_masked(gray, mask), a)))
    assert torch.equal(edge, whole)

    def host_path():
        g, m = gray.squeeze(1).cpu().numpy(), mask.squeeze(1).cpu().numpy()
        e = np.stack([canny_restated.canny_witness(g[i], m[i], 2.0) for i in range(B)])
        return torch.from_numpy(e[:, None].astype(np.float32)).to(dev)
    host_ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_edge = host_path()
        torch.cuda.synchronize()
        host_ms.append(1e3 * (time.perf_counter() - t0))
    put(dict(what="host path: copy out, float64 scipy canny per image, copy back (wall clock)", shape=shape, ms_median=round(statistics.median(host_ms), 2),
             ms_min=round(min(host_ms), 2), ms_max=round(max(host_ms), 2), pixels_differing_from_the_kernel=int((host_edge != whole).sum())))

    edge_inpaint = torch.rand_like(gray)
    image_inpaint, disp_inpaint = torch.rand_like(warp_image), torch.rand_like(warp_disp)
    put(dict(what="ops.stage2_gray_hole", shape=shape, algorithmic_bytes=24 * px, **timed(lambda: ops.stage2_gray_hole(warp_image, mask), a)))
    put(dict(what="ops.stage2_edge_input", shape=shape, algorithmic_bytes=24 * px, **timed(lambda: ops.stage2_edge_input(gray, edge, hole), a)))
    put(dict(what="ops.stage2_gen_inputs", shape=shape, algorithmic_bytes=48 * px, **timed(lambda: ops.stage2_gen_inputs(warp_image, warp_disp, hole, edge_inpaint), a)))
    put(dict(what="ops.stage2_merge", shape=shape, algorithmic_bytes=52 * px,
             **timed(lambda: ops.stage2_merge(warp_image, image_inpaint, warp_disp, disp_inpaint, hole), a)))

    models = tuple(networks.fold_spectral_norm(stage2_pattern.load_pattern(stage2_pattern.build(networks, n))).to(dev) for n in stage2_pattern.GENERATORS)
    put(dict(what="warpback.warp_and_inpaint, pattern weights (one render, canny, three generators)", shape=shape,
             **timed(lambda: warp_and_inpaint(image, disp, cam_int, ext, inv, models, r), a, calls=2)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
