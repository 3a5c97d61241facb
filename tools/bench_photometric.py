#!/usr/bin/env python3
"""Cost of RAFT's photometric augmentation in the online source (mpf_photometric_pairs) at its flagship size: B = 8 pairs of 384 x 1280
frames, online.RAFT_PHOTOMETRIC draws.  Prints one JSON line: the host draw time per batch, the launch (ops.photometric_pairs) time per batch
on the host, and the device time per batch from events around `reps` back-to-back batches.  Run it under rocprofv3 --kernel-trace --stats for
the time of each of its kernels.
Usage: bench_photometric.py [reps]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpiflow_amd import online, ops  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    B, H, W = 8, 384, 1280
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    src = torch.from_numpy(rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).to(dev)
    dst = torch.from_numpy(rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).to(dev)
    c = online.photometric_config(True)
    t = time.perf_counter()
    draws = [[online.photometric_params(rs, H, W, c) for _ in range(B)] for _ in range(reps)]
    draw_us = 1e6 * (time.perf_counter() - t) / reps
    out = dict(src=torch.empty_like(src), dst=torch.empty_like(dst))
    for d in draws[:5]:
        ops.photometric_pairs([dict(src=src[b], dst=dst[b], **d[b]) for b in range(B)], out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    e0.record()
    for d in draws:
        ops.photometric_pairs([dict(src=src[b], dst=dst[b], **d[b]) for b in range(B)], out=out)
    e1.record()
    host_us = 1e6 * (time.perf_counter() - t) / reps
    torch.cuda.synchronize()
    dev_us = 1e3 * e0.elapsed_time(e1) / reps
    print(json.dumps(dict(B=B, H=H, W=W, reps=reps, draw_us_per_batch=draw_us, launch_host_us_per_batch=host_us, device_us_per_batch=dev_us,
                          bytes_per_batch_min=2 * 2 * B * H * W * 3)))


if __name__ == "__main__":
    main()
