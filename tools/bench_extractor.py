#!/usr/bin/env python3
"""RAFT's encoders: the fused form (mpiflow_amd/raft_extractor.py) against the plain torch form on the same parameters, in ONE process, the
forms alternating round by round after a warm-up, every figure the median of the rounds with min and max beside it.

    python tools/bench_extractor.py [--rounds 15] [--warmup 3] [--out profiles/extractor/bench.json] [--only NAME]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_extractor.py --trace-shape things_6x400x720      (a run of its own)

Per shape, for fnet (BasicEncoder(256, 'instance') on a list of two image batches) and cnet (BasicEncoder(256, 'batch'), training mode):
  encoder  forward (no_grad) and forward + backward of the whole encoder, fused against plain
  tails    the norm kernels alone on the first block's activation (1/2 resolution, 64 channels): statistics + relu(norm(x)), and the tail
           relu(res + relu(norm(x))), forward and backward, against the torch chain; algorithmic bytes and the fraction of the 8 TB/s HBM roofline

The plain form calls the module's own torch.nn submodules one after the other: norm module, F.relu, add, F.relu.  Shapes: RAFT's training crops
at the batch sizes of its train_standard.sh (chairs 10 x 368 x 496, things 6 x 400 x 720, kitti 6 x 288 x 960) and a 1 x 440 x 1024 inference call."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpiflow_amd import ops, raft_extractor as rx  # noqa: E402

ROOFLINE = 8.0e12
# (name, B, H, W, backward too)
SHAPES = [("chairs_10x368x496", 10, 368, 496, True), ("things_6x400x720", 6, 400, 720, True), ("kitti_6x288x960", 6, 288, 960, True),
          ("infer_1x440x1024", 1, 440, 1024, False)]


def plain_block(blk, x):
    y = F.relu(blk.norm1(blk.conv1(x)), inplace=True)
    y = F.relu(blk.norm2(blk.conv2(y)), inplace=True)
    if hasattr(blk, "conv3"):
        y = F.relu(blk.norm3(blk.conv3(y)), inplace=True)
    if blk.downsample is not None:
        x = blk.downsample(x)
    return F.relu(x + y, inplace=True)


def plain_encoder(enc, x):
    is_list = isinstance(x, (list, tuple))
    if is_list:
        n = x[0].shape[0]
        x = torch.cat(x, dim=0)
    x = F.relu(enc.norm1(enc.conv1(x)), inplace=True)
    for layer in (enc.layer1, enc.layer2, enc.layer3):
        for blk in layer:
            x = plain_block(blk, x)
    x = enc.conv2(x)
    return torch.split(x, [n, n], dim=0) if is_list else x


def measure(forms, rounds, warmup):
    """forms: name -> callable.  Alternates them; -> name -> (median, min, max) in ms"""
    times = {k: [] for k in forms}
    for r in range(warmup + rounds):
        for k, fn in forms.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def report(out, shape, net, what, res, extra=None):
    for k, (med, lo, hi) in res.items():
        rec = dict(shape=shape, net=net, measurement=what, form=k, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
        if extra and k in extra:
            rec.update(extra[k])
        out.append(rec)
        print(json.dumps(rec), flush=True)


def encoder_run(enc, images, form, backward):
    def run():
        with torch.set_grad_enabled(backward):
            out = enc(images) if form == "fused" else plain_encoder(enc, images)
            if backward:
                (sum(o.sum() for o in out) if isinstance(out, tuple) else out.sum()).backward()
                enc.zero_grad(set_to_none=True)
    return run


def bench_shape(out, name, B, H, W, backward, rounds, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    im1, im2 = (torch.rand(B, 3, H, W, device=dev) * 2 - 1 for _ in range(2))
    for net, fn, images in (("fnet", "instance", [im1, im2]), ("cnet", "batch", im1)):
        enc = rx.BasicEncoder(output_dim=256, norm_fn=fn, dropout=0.0).to(dev)
        for bwd in ((False, True) if backward else (False,)):
            res = measure({f: encoder_run(enc, images, f, bwd) for f in ("plain", "fused")}, rounds, warmup)
            report(out, name, net, "encoder_" + ("fwd_bwd" if bwd else "fwd"), res)
        # ---- the kernels alone, at the first block's activation
        N, C, H2, W2 = (2 * B if net == "fnet" else B), 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1
        mode = "instance" if fn == "instance" else "batch_train"
        x, r, g = (3.0 + 0.5 * torch.randn(N, C, H2, W2, device=dev) for _ in range(3))
        w, b = (torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)) if fn == "batch" else (None, None)
        plane = x.numel() * 4
        kw = dict(weight=w, bias=b)
        state = {}

        def hip_fwd(res):
            def run():
                state["y"] = ops.NormTerm(x, mode, **kw)
                ops.norm_act(state["y"], r if res else None)
            return run

        def hip_bwd(res):
            def run():
                ops.norm_act_backward(g, state["y"], r if res else None)
            return run

        def torch_chain(res, bwd):
            def run():
                with torch.set_grad_enabled(bwd):
                    xx = x.detach().requires_grad_(bwd)
                    rr = r.detach().requires_grad_(bwd)
                    y = F.relu(F.instance_norm(xx) if fn == "instance" else F.batch_norm(xx, None, None, w, b, training=True))
                    if res:
                        y = F.relu(rr + y)
                    if bwd:
                        y.backward(g)
            return run
        for res, tag in ((False, "norm_relu"), (True, "tail")):
            fwd_bytes = (3 + (1 if res else 0)) * plane                 # statistics: 1 read; act: 1 (+1) reads, 1 write
            bwd_bytes = (2 + (1 if res else 0)) * plane + (3 + (2 if res else 0)) * plane     # reduce: x, g (+res); backward: x, g (+res) read, dx (+dres) written
            t = measure(dict(hip=hip_fwd(res), torch=torch_chain(res, False)), rounds, warmup)
            report(out, name, net, tag + "_fwd", t, dict(hip=dict(bytes=fwd_bytes, roofline_fraction=round(fwd_bytes / (t["hip"][0] * 1e-3) / ROOFLINE, 3))))
            if backward:
                t = measure(dict(hip=hip_bwd(res), torch_fwd_bwd=torch_chain(res, True), torch_fwd=torch_chain(res, False)), rounds, warmup)
                report(out, name, net, tag + "_bwd", t, dict(hip=dict(bytes=bwd_bytes, roofline_fraction=round(bwd_bytes / (t["hip"][0] * 1e-3) / ROOFLINE, 3))))


def trace_shape(name):
    """three forward + backward passes of the fused fnet and cnet at one shape, for a kernel trace"""
    dev = torch.device("cuda:0")
    _, B, H, W, backward = [s for s in SHAPES if s[0] == name][0]
    torch.manual_seed(1)
    im1, im2 = (torch.rand(B, 3, H, W, device=dev) * 2 - 1 for _ in range(2))
    for fn, images in (("instance", [im1, im2]), ("batch", im1)):
        enc = rx.BasicEncoder(output_dim=256, norm_fn=fn, dropout=0.0).to(dev)
        for _ in range(3):
            encoder_run(enc, images, "fused", backward)()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--trace-shape", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_extractor.py needs a GPU"
    if a.trace_shape:
        trace_shape(a.trace_shape)
        return 0
    out = []
    for s in SHAPES:
        if a.only in (None, s[0]):
            bench_shape(out, *s, rounds=a.rounds, warmup=a.warmup)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
