#!/usr/bin/env python3
"""Time per frame of the colour-coded flow, host against device, at Sintel's and KITTI's frame sizes (profiles/flow_viz/README.md).

    python tools/bench_flow_viz.py [--rounds 5] [--frames 20] [--device-frames 2000] [--warmup 3] [--out PATH.json]

(a) host    the float32 flow [1,2,H,W] copied to the host (8 B/px), then the colour wheel in numpy with upstream flow_viz's arithmetic and
            precisions (host_flow_to_image below: one global maximum, arctan2, a table blend and a floor per channel, one thread)
(b) device  ops.flow_to_image, then the uint8 frame [1,H,W,3] copied to the host (3 B/px)

Both end with the picture in host memory and a synchronised device.  Per size the two are run alternately, `rounds` times, `frames` host
frames and `device-frames` device frames per round (windows of a few tenths of a second each) after `warmup` unmeasured frames; the figure
is the median over rounds of the mean time per frame, with the smallest and largest round.  The two pictures are compared once per size
(bytes that differ, largest difference).  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = ((436, 1024), (375, 1242))


def wheel():
    w = np.zeros((55, 3))
    col = 0
    for n, full, ramp, down in ((15, 0, 1, False), (6, 1, 0, True), (4, 1, 2, False), (11, 2, 1, True), (13, 2, 0, False), (6, 0, 2, True)):
        steps = np.floor(255 * np.arange(n) / n)
        w[col:col + n, full] = 255
        w[col:col + n, ramp] = 255 - steps if down else steps
        col += n
    return w


def host_flow_to_image(flow_hw2):
    """[H,W,2] float32 -> [H,W,3] uint8: float32 up to fk, float64 from the blend on, channel by channel as upstream loops"""
    u, v = flow_hw2[:, :, 0], flow_hw2[:, :, 1]
    d = np.sqrt(np.square(u) + np.square(v)).max() + 1e-5
    u, v = u / d, v / d
    rad = np.sqrt(np.square(u) + np.square(v))
    fk = (np.arctan2(-v, -u) / np.pi + 1) / 2 * 54
    k0 = np.floor(fk).astype(np.int32)
    k1 = k0 + 1
    k1[k1 == 55] = 0
    f = fk - k0
    inside = rad <= 1
    out = np.zeros(u.shape + (3,), np.uint8)
    table = wheel()
    for c in range(3):
        col = (1 - f) * (table[k0, c] / 255.0) + f * (table[k1, c] / 255.0)
        col[inside] = 1 - rad[inside] * (1 - col[inside])
        col[~inside] = col[~inside] * 0.75
        out[:, :, c] = np.floor(255 * col)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--device-frames", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flow_viz needs a GPU")
    from mpiflow_amd import ops
    result = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, numpy=np.__version__, rounds=a.rounds, frames=a.frames,
                  device_frames=a.device_frames, warmup=a.warmup, host_threads=1, sizes={})
    for H, W in SIZES:
        g = torch.Generator().manual_seed(9150 + H)
        flow = (torch.randn(1, 2, H, W, generator=g) * 8).cuda()

        def host():
            return host_flow_to_image(np.ascontiguousarray(flow[0].permute(1, 2, 0).cpu().numpy()))

        def device():
            return ops.flow_to_image(flow)[0].cpu().numpy()

        diff = np.abs(host().astype(np.int64) - device().astype(np.int64))
        times = {"host": [], "device": []}
        for fn in (host, device):
            for _ in range(a.warmup):
                fn()
        for _ in range(a.rounds):
            for name, fn, frames in (("host", host, a.frames), ("device", device, a.device_frames)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(frames):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / frames * 1e3)
        row = {name: dict(median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t)) for name, t in times.items()}
        row["bytes_differing"], row["largest_difference"], row["bytes"] = int((diff != 0).sum()), int(diff.max()), int(diff.size)
        result["sizes"]["%dx%d" % (H, W)] = row
        print("%4d x %4d  host %8.2f ms (%.2f .. %.2f)   device %7.3f ms (%.3f .. %.3f)   %d of %d bytes differ, by at most %d"
              % (H, W, row["host"]["median_ms"], row["host"]["min_ms"], row["host"]["max_ms"], row["device"]["median_ms"], row["device"]["min_ms"],
                 row["device"]["max_ms"], row["bytes_differing"], row["bytes"], row["largest_difference"]), flush=True)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
