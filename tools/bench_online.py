#!/usr/bin/env python3
"""Throughput of the online pair source (mpiflow_amd/online.py) at the generator's flagship size: 384 x 1280, 64 planes, random weights on the
fast HIP engine, crop 288 x 960, batches of 8, RAFT's default spatial augmentation.

  1. the source alone, fill=builtin (host NS threads) and fill=peel (GPU): samples/s after a warm-up epoch;
  2. beside a synthetic consumer on the caller's stream - a fixed loop of fp32 GEMMs sized to ~20 ms per step - the consumer's step time
     with and without the source feeding it.

With --photometric: the source alone (fill=peel) with RAFT's photometric augmentation off and on (online.RAFT_PHOTOMETRIC), alternated,
`--rounds` times each (default 2), and the on / off ratio of their medians; nothing else.
With --sparse: the same A/B between RAFT's dense path (the default augmentation) and its sparse KITTI-stage path
(sparse=True, augment=online.RAFT_KITTI_AUGMENT), and the sparse / dense ratio of their medians.

Same synthetic KITTI-shaped dataset as tools/bench_cli.py (375 x 1242 PNGs); compare with its "steady state" line for the CLI's rate.
With --fill a,b,...: parts 1 and 2 for those fill methods, in that order (default peel,builtin; ns-hip = the GPU NS fill); --alone-only skips part 2.
Usage: bench_online.py [n_images] [--json out.json] [--photometric | --sparse [--rounds N] | --fill LIST [--alone-only]]"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpiflow_amd.online import RAFT_KITTI_AUGMENT, OnlinePairs  # noqa: E402


def dataset(n_img):
    base = os.path.join(tempfile.mkdtemp(prefix="mpf_online_"), "data")
    for d in ("images", "disps", "masks"):
        os.makedirs(os.path.join(base, d))
    rs = np.random.RandomState(0)
    yy, xx = np.mgrid[0:375, 0:1242]
    for i in range(n_img):
        img = (np.clip(0.5 + 0.25 * np.sin(xx / (17.0 + i)) + 0.25 * np.cos(yy / 23.0) + 0.05 * rs.randn(375, 1242), 0, 1) * 255).astype(np.uint8)
        Image.fromarray(np.stack([img, np.roll(img, 7, 1), np.roll(img, 13, 0)], -1)).save(os.path.join(base, "images", "%04d.png" % i))
        Image.fromarray((255 * (0.1 + 0.8 * yy / 375)).astype(np.uint8)).save(os.path.join(base, "disps", "%04d.png" % i))
        m = np.zeros((375, 1242), np.uint8)
        m[150:300, 300:600] = 1
        m[200:330, 800:1000] = 2
        Image.fromarray(m).save(os.path.join(base, "masks", "%04d.png" % i))
    return base


def source(base, fill, photometric=None, sparse=None):
    kw = dict(sparse=True, augment=RAFT_KITTI_AUGMENT) if sparse else {}
    return OnlinePairs(base, batch_size=8, crop=(288, 960), width=1280, height=384, seed=114514, pairs_per_image=5, mpi_from="model",
                       ckpt_path="random:0", planes=64, fill=fill, mix=32, prefetch=2, photometric=photometric, **kw)


def alone(base, fill, photometric=None, sparse=None):
    with source(base, fill, photometric, sparse) as src:
        t0 = time.perf_counter()
        n0 = sum(b["valid"].shape[0] for b in src)                # warm-up epoch: graph capture, first launches, pinned slots
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        n1 = 0
        for _ in range(2):
            for b in src:
                n1 += b["valid"].shape[0]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
    return dict(fill=fill, photometric=photometric is not None, sparse=bool(sparse), warmup_samples=n0, warmup_s=t1 - t0, samples=n1, seconds=t2 - t1,
                samples_per_s=n1 / (t2 - t1))


def photometric_ab(base, rounds):
    runs = {False: [], True: []}
    for _ in range(rounds):
        for on in (False, True):
            r = alone(base, "peel", True if on else None)
            print(json.dumps(r), flush=True)
            runs[on].append(r["samples_per_s"])
    off, on = float(np.median(runs[False])), float(np.median(runs[True]))
    return dict(fill="peel", rounds=rounds, samples_per_s_off=runs[False], samples_per_s_on=runs[True], median_off=off, median_on=on,
                ratio_on_off=on / off)


def sparse_ab(base, rounds):
    runs = {False: [], True: []}
    for _ in range(rounds):
        for on in (False, True):
            r = alone(base, "peel", sparse=on)
            print(json.dumps(r), flush=True)
            runs[on].append(r["samples_per_s"])
    dense, sparse = float(np.median(runs[False])), float(np.median(runs[True]))
    return dict(fill="peel", rounds=rounds, samples_per_s_dense=runs[False], samples_per_s_sparse=runs[True], median_dense=dense,
                median_sparse=sparse, ratio_sparse_dense=sparse / dense)


def consumer(reps):
    a = torch.randn(4096, 4096, device="cuda")
    b = torch.randn(4096, 4096, device="cuda")

    def step(batch=None):
        x = a
        for _ in range(reps):
            x = torch.mm(x, b) * 1e-3
        if batch is not None:
            x[0, 0] += batch["flow"][0, 0, 0, 0] + batch["image1"][0, 0, 0, 0]     # the step reads the batch
        return x
    return step


def timed_steps(step, n, feed=None):
    ts = []
    it = iter(feed) if feed is not None else None
    for _ in range(n):
        batch = next(it) if it is not None else None
        torch.cuda.synchronize()
        t = time.perf_counter()
        step(batch)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return ts


def beside(base, fill):
    probe = consumer(1)
    for _ in range(3):
        probe()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(10):
        probe()
    torch.cuda.synchronize()
    reps = max(1, int(round(0.020 / ((time.perf_counter() - t) / 10))))
    step = consumer(reps)
    timed_steps(step, 5)
    lone = timed_steps(step, 30)
    with source(base, fill) as src:
        def forever():
            while True:
                for b in src:
                    yield b
        feed = forever()
        timed_steps(step, 10, feed)                                    # warm-up
        t0 = time.perf_counter()
        fed = timed_steps(step, 60, feed)
        wall = time.perf_counter() - t0
    # the step time alone includes the synchronise; the wall time with the source includes waiting for batches the source had not finished
    return dict(fill=fill, gemm_reps=reps, step_ms_alone=1e3 * float(np.median(lone)), step_ms_with_source=1e3 * float(np.median(fed)),
                step_ms_with_source_p90=1e3 * float(np.percentile(fed, 90)), wall_ms_per_step_with_source=1e3 * wall / 60,
                samples_per_s_with_consumer=60 * 8 / wall)


def main():
    n_img = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 24
    out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    base = dataset(n_img)
    if "--photometric" in sys.argv:
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 2
        res = dict(images=n_img, pairs_per_epoch=5 * n_img, photometric=photometric_ab(base, rounds))
        print(json.dumps(res["photometric"]), flush=True)
        if out:
            with open(out, "w") as f:
                json.dump(res, f, indent=1)
        return
    if "--sparse" in sys.argv:
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 2
        res = dict(images=n_img, pairs_per_epoch=5 * n_img, sparse=sparse_ab(base, rounds))
        print(json.dumps(res["sparse"]), flush=True)
        if out:
            with open(out, "w") as f:
                json.dump(res, f, indent=1)
        return
    fills = sys.argv[sys.argv.index("--fill") + 1].split(",") if "--fill" in sys.argv else ["peel", "builtin"]
    res = dict(images=n_img, pairs_per_epoch=5 * n_img, alone=[], beside=[])
    for fill in fills:
        r = alone(base, fill)
        print(json.dumps(r), flush=True)
        res["alone"].append(r)
    if "--alone-only" in sys.argv:
        fills = []
    for fill in fills:
        r = beside(base, fill)
        print(json.dumps(r), flush=True)
        res["beside"].append(r)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
