#!/usr/bin/env python3
"""The pair launch (k_pair_overlap) with and without the dead-tile skip, for masks between the two extremes.

  --mask box    bench.py's object (synth.soft_box_mask, 1/16 of the frame): ~89 % of view 0's tiles are dead
  --mask half   0.5 everywhere: obj_mask and its complement are non-zero on every texel, NOTHING can be skipped - the worst case, every
                Stage B workgroup pays the test and then renders
  --mask ones / zero   one whole view is dead
  --skip 0      the renderer without support maps (the full render, the entry points of before)
  --ablate 1|2  witness build: only the Stage B / only the Stage A+C workgroups run (role-alone times; results invalid)
  --root DIR    import the package from another checkout (same-box comparison with an older tree, which has no skip: --skip is ignored there)
Prints the mean / min / max duration of the fused launch over the timed pushes (HIP events on its stream)."""
import argparse
import inspect
import os
import random
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--planes", type=int, default=64)
ap.add_argument("--height", type=int, default=640)
ap.add_argument("--width", type=int, default=960)
ap.add_argument("--images", type=int, default=4)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--mask", default="box", choices=["box", "half", "ones", "zero"])
ap.add_argument("--skip", type=int, default=1)
ap.add_argument("--ablate", type=int, default=0)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import bench  # noqa: E402
from mpiflow_amd import _lib, host_math, pipeline, synth  # noqa: E402

dev = torch.device("cuda:0")
S, H, W, B = a.planes, a.height, a.width, a.images
if a.ablate:
    lib = _lib.select_witness()
    _lib.check(lib.mpf_tune(b"ovl_ablate", a.ablate))
kw = dict(merge_in_launch=True)
has_skip = "skip_dead_tiles" in inspect.signature(pipeline.OverlappedPairRenderer.__init__).parameters
if has_skip:
    kw["skip_dead_tiles"] = bool(a.skip)
r = pipeline.OverlappedPairRenderer(S, H, W, dev, **kw)
K, disp = synth.intrinsics(H, W), synth.plane_disparities(S)
rng = random.Random(114514)
images, preps = [], []
for i in range(B):
    images.append(bench.make_image(S, H, W, dev, seed=i))
    G_dyn = host_math.generate_random_pose(0.15, rng=rng)
    G_cam = host_math.generate_random_pose(0.15, base_motions=(0, 0, 0), rng=rng)
    preps.append(r.prepare(K, disp, [G_cam, G_dyn]))
mask = {"box": synth.soft_box_mask(H, W), "half": np.full((H, W), 0.5, np.float32), "ones": np.ones((H, W), np.float32),
        "zero": np.zeros((H, W), np.float32)}[a.mask]
om = torch.from_numpy(mask).to(dev)
outs = [(torch.empty((H, W, 2), device=dev), torch.empty((H, W, 3), dtype=torch.uint8, device=dev), torch.empty((H, W), dtype=torch.uint8, device=dev)) for _ in range(3)]
ev = []


def hook(launch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    ev.append((e0, e1))


r.on_fused = hook
n = 0
for step in range(a.steps + 2):
    if step == 2:
        torch.cuda.synchronize()
        ev.clear()
    for i in range(B):
        r.push(images[i][0], images[i][1], preps[i], om, out=outs[n % 3])
        n += 1
r.flush()
torch.cuda.synchronize()
t = np.array([e0.elapsed_time(e1) for e0, e1 in ev]) * 1e3
print("mask %s skip %s ablate %d (%s): fused launch mean %.1f us  min %.1f  max %.1f  over %d launches" % (
    a.mask, (a.skip if has_skip else "n/a"), a.ablate, os.path.abspath(a.root), t.mean(), t.min(), t.max(), len(t)), flush=True)
