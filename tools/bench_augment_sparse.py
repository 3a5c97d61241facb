#!/usr/bin/env python3
"""Device time of the sparse augmentation kernel (mpf_augment_sparse_pairs) next to the dense one (mpf_augment_pairs) at the online source's
flagship size: B = 8 pairs of 384 x 1280 frames, crop 288 x 960, the KITTI stage's draws (online.sparse_augment_params with
RAFT_KITTI_AUGMENT), the same resize / flip / crop for both kernels, KITTI's 16-bit code on.  The two kernels alternate, `reps` batches each;
prints one JSON line with the device time per launch of each from events.  Run it under rocprofv3 --kernel-trace --stats for the kernel times
of one trace (k_augment_sparse_pairs, k_augment_pairs).
Usage: bench_augment_sparse.py [reps]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpiflow_amd import online, ops  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    B, H, W, crop = 8, 384, 1280, (288, 960)
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    src = torch.from_numpy(rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).to(dev)
    dst = torch.from_numpy(rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).to(dev)
    flow = torch.from_numpy(((rs.rand(B, H, W, 2) - 0.5) * 200).astype(np.float32)).to(dev)
    params = [[online.sparse_augment_params(rs, H, W, crop, online.RAFT_KITTI_AUGMENT) for _ in range(B)] for _ in range(reps)]
    sparse = [[dict(src=src[b], dst=dst[b], flow=flow[b], quantize=1, **p[b]) for b in range(B)] for p in params]
    dense = [[dict(src=src[b], dst=dst[b], flow=flow[b], flip_v=0, **p[b]) for b in range(B)] for p in params]
    out = ops.augment_pairs(dense[0], size=crop)
    for i in range(3):
        ops.augment_pairs(dense[i], out=out)
        ops.augment_sparse_pairs(sparse[i], out=out)
    torch.cuda.synchronize()
    ev = {k: [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)] for k in ("dense", "sparse")}
    for i in range(reps):
        ev["dense"][2 * i].record()
        ops.augment_pairs(dense[i], out=out)
        ev["dense"][2 * i + 1].record()
        ev["sparse"][2 * i].record()
        ops.augment_sparse_pairs(sparse[i], out=out)
        ev["sparse"][2 * i + 1].record()
    torch.cuda.synchronize()
    us = {k: [1e3 * e[2 * i].elapsed_time(e[2 * i + 1]) for i in range(reps)] for k, e in ev.items()}
    res = dict(B=B, H=H, W=W, crop=crop, reps=reps, resized=sum(p["resize"] for ps in params for p in ps) / (B * reps),
               dense_us_median=float(np.median(us["dense"])), sparse_us_median=float(np.median(us["sparse"])))
    res["ratio_sparse_dense"] = res["sparse_us_median"] / res["dense_us_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
