#!/usr/bin/env python3
"""The sparse bilateral filter (ops.sparse_bilateral_filter, mpf_bilateral.hip) on 384 x 1280 uint8 disparities, on one stream:

  kernel    time per frame for the windows [5,5] and 3d-photo-inpainting's [7,7,5,5,5], on a real-looking disparity (smooth regions with object
            edges: few pixels select) and on the blocky test pattern of tests/bilateral_restated.py (most do).  Warm-up, then HIP events
            around `reps` calls that cycle through `frames` different inputs, out and workspace handed in; the median of `rounds` such
            measurements.  Algorithmic bytes per pixel and iteration for uint8: the map reads v and the input and writes D (3), the selection
            reads v and D and writes its output (3).
  --cli N   gen_3dphoto_dynamic.py on N synthetic KITTI-shaped images (375 x 1242 -> 384 x 1280, 64 planes, repeat 5, random weights), with and
            without --disp-filter 5,5, runs alternating after one warm-up run; the CLI's own steady-state pairs/s.

    python tools/bench_bilateral.py [--cli N] [--json PATH]"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 384, 1280


def real_looking(seed, h=H, w=W):
    """a ground plane's ramp, a few objects of constant disparity with soft 2-pixel edges, +-1 noise -> uint8"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = 30 + 170 * np.clip((yy - 0.35 * h) / (0.65 * h), 0, 1)
    for _ in range(7):
        cy, cx, ry, rx, lev = rs.uniform(0.3, 0.9) * h, rs.uniform(0, 1) * w, rs.uniform(20, 70), rs.uniform(30, 120), rs.uniform(60, 240)
        inside = np.clip((1 - np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)) * min(ry, rx) / 2 + 0.5, 0, 1)
        d = d * (1 - inside) + lev * inside
    return np.clip(np.rint(d + rs.randint(-1, 2, (h, w))), 1, 255).astype(np.uint8)


def kernel_part(records):
    import torch
    import bilateral_restated as R
    from mpiflow_amd import ops
    dev = torch.device("cuda:0")
    frames, reps, rounds = 16, 64, 7
    ws = ops.sparse_bilateral_workspace(torch.uint8, 1, H, W, dev)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    for kind, make in (("real-looking", real_looking), ("blocky", lambda s: R.blocky(s, H, W))):
        host = [make(100 + i) for i in range(frames)]
        xs = [torch.from_numpy(a).to(dev) for a in host]
        for windows in ((5, 5), (7, 7, 5, 5, 5)):
            changed = float(np.mean([(ops.sparse_bilateral_filter(x, windows).cpu().numpy() != a).mean() for x, a in zip(xs[:4], host[:4])]))
            D = R.discontinuity_map(host[0].astype(np.float64) / 255, host[0].astype(np.float64) / 255, 0.04)
            m = windows[0] // 2
            active = float(R.windows(np.pad(np.pad(D[1:-1, 1:-1], 1, "edge"), m, "edge"), m).any(-1).mean())
            for i in range(2 * frames):
                ops.sparse_bilateral_filter(xs[i % frames], windows, out=out, workspace=ws)
            torch.cuda.synchronize()
            ms = []
            for _ in range(rounds):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for i in range(reps):
                    ops.sparse_bilateral_filter(xs[i % frames], windows, out=out, workspace=ws)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b) / reps)
            med, nbytes = statistics.median(ms), 6 * H * W * len(windows)
            rec = dict(what="ops.sparse_bilateral_filter, uint8 %d x %d, out and workspace given" % (H, W), input=kind, windows=list(windows),
                       first_iteration_pixels_that_select=round(active, 4), pixels_changed=round(changed, 4), ms_per_frame_median=round(med, 4),
                       ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), algorithmic_bytes=nbytes, achieved_GB_per_s=round(nbytes / med / 1e6, 2))
            records.append(rec)
            print(json.dumps(rec), flush=True)


def cli_part(records, n_img):
    from PIL import Image
    tmp = tempfile.mkdtemp(prefix="mpf_bil_")
    base = os.path.join(tmp, "data")
    for d in ("images", "disps", "masks"):
        os.makedirs(os.path.join(base, d))
    rs = np.random.RandomState(0)
    yy, xx = np.mgrid[0:375, 0:1242]
    for i in range(n_img):
        img = (np.clip(0.5 + 0.25 * np.sin(xx / (17.0 + i)) + 0.25 * np.cos(yy / 23.0) + 0.05 * rs.randn(375, 1242), 0, 1) * 255).astype(np.uint8)
        Image.fromarray(np.stack([img, np.roll(img, 7, 1), np.roll(img, 13, 0)], -1)).save(os.path.join(base, "images", "%04d.png" % i))
        Image.fromarray(real_looking(i, 375, 1242)).save(os.path.join(base, "disps", "%04d.png" % i))
        m = np.zeros((375, 1242), np.uint8)
        m[150:300, 300:600] = 1
        m[200:330, 800:1000] = 2
        Image.fromarray(m).save(os.path.join(base, "masks", "%04d.png" % i))
    rates = {"off": [], "on": []}
    try:
        for run, which in enumerate(("warm-up", "off", "on", "off", "on", "off", "on")):
            out = os.path.join(tmp, "out")
            extra = ["--disp-filter", "5,5"] if which == "on" else []
            r = subprocess.run([sys.executable, os.path.join(ROOT, "gen_3dphoto_dynamic.py"), "--base", base, "--out", out, "--repeat", "5", "--mpi-from", "model",
                                "--ckpt_path", "random:0", "--model-engine", "hip", "--writers", "16", "--inpaint", "peel"] + extra, capture_output=True, text=True, timeout=300)
            shutil.rmtree(out, ignore_errors=True)
            steady = [l for l in r.stdout.splitlines() if l.startswith("steady")]
            if r.returncode != 0 or not steady:
                print(r.stdout[-600:] + r.stderr[-600:])
                raise SystemExit("the CLI run %d (%s) failed" % (run, which))
            rate = float(steady[-1].split(":")[1].split()[0])
            print("run %d, --disp-filter %s: %s" % (run, which, steady[-1]), flush=True)
            if which in rates:
                rates[which].append(rate)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    rec = dict(what="gen_3dphoto_dynamic.py, %d images x 5 pairs, hip engine, peel fill, 16 writers: steady-state pairs/s, runs alternating" % n_img,
               without_filter=rates["off"], with_disp_filter_5_5=rates["on"])
    records.append(rec)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cli", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    records = []
    kernel_part(records)
    if a.cli > 0:
        cli_part(records, a.cli)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
