#!/usr/bin/env python3
"""One evaluation frame of RAFT on a frame whose sides are no multiples of 8: RAFT.predict + FlowMetrics (the padding fused into the image
scaling, the unpadded window of the last prediction written alone, the metrics in one launch pair, nothing copied to the host) against the
torch form a port of evaluate.py writes without them - F.pad, forward(test_mode=True), the slice, evaluate.py's elementwise expressions
and its .item() / .cpu() per frame - on the SAME model, in ONE process, the forms alternating round by round after a warm-up; every figure
the median of the rounds with min and max beside it, and the peak allocated memory of a frame.

    python tools/bench_raft_eval.py [--rounds 7] [--warmup 2] [--out profiles/raft_eval/bench.json]

Cases: 1 x 375 x 1242 as validate_kitti runs it ('kitti' padding, 24 iterations, the valid mask) and 1 x 436 x 1024 as validate_sintel does
('sintel' padding, 32 iterations, every pixel), for the basic and the small model.  The convolutions dominate both forms."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpiflow_amd.raft import RAFT  # noqa: E402
from mpiflow_amd.raft_eval import FlowMetrics, InputPadder  # noqa: E402

CASES = [("kitti", 375, 1242, 24), ("sintel", 436, 1024, 32)]


def torch_frame(model, kind, iters, im1, im2, gt, valid):
    """evaluate.py's loop body (validate_kitti / validate_sintel) on this package's strict forward"""
    padder = InputPadder(im1.shape, mode=kind)
    p1, p2 = padder.pad(im1, im2)
    _, flow_pr = model(p1, p2, iters=iters, test_mode=True)
    flow = padder.unpad(flow_pr[0])
    epe = torch.sum((flow - gt[0]) ** 2, dim=0).sqrt()
    if kind == "sintel":
        return epe.view(-1).cpu().numpy()
    mag = torch.sum(gt[0] ** 2, dim=0).sqrt()
    epe, mag = epe.view(-1), mag.view(-1)
    val = valid[0].view(-1) >= 0.5
    out = ((epe > 3.0) & ((epe / mag) > 0.05)).float()
    return epe[val].mean().item(), out[val].cpu().numpy()


def fused_frame(model, kind, iters, im1, im2, gt, valid):
    metrics = FlowMetrics()
    _, flow_pr = model.predict(im1, im2, iters=iters, mode=kind)
    metrics.update(flow_pr, gt, valid if kind == "kitti" else None)
    return metrics.result(kind)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_raft_eval.py needs a GPU"
    dev = torch.device("cuda:0")
    out = []
    for small in (False, True):
        torch.manual_seed(1)
        model = RAFT(argparse.Namespace(small=small, mixed_precision=False)).to(dev).eval()
        for kind, H, W, iters in CASES:
            im1 = torch.randint(0, 256, (1, 3, H, W), device=dev).float()
            im2 = torch.roll(im1, (2, 5), dims=(2, 3))
            gt = 5.0 * torch.randn(1, 2, H, W, device=dev)
            valid = (torch.rand(1, H, W, device=dev) > 0.1).float()
            forms = dict(predict_flow_metrics=fused_frame, torch_pad_slice_metrics=torch_frame)
            times, peak, results = {k: [] for k in forms}, {}, {}
            with torch.no_grad():
                for r in range(a.warmup + a.rounds):
                    for k, fn in forms.items():
                        torch.cuda.synchronize()
                        torch.cuda.reset_peak_memory_stats(dev)
                        held = torch.cuda.memory_allocated(dev)
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0.record()
                        results[k] = fn(model, kind, iters, im1, im2, gt, valid)   # both forms end in a device-to-host copy
                        t1.record()
                        torch.cuda.synchronize()
                        if r >= a.warmup:
                            times[k].append(t0.elapsed_time(t1))
                            peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated(dev) - held)
            # faster and different is not faster: the two forms' numbers on this frame
            if kind == "kitti":
                t_epe, t_out = results["torch_pad_slice_metrics"]
                want = {"kitti-epe": float(t_epe), "kitti-f1": float(100 * np.mean(t_out))}
            else:
                e = results["torch_pad_slice_metrics"]
                want = {"epe": float(np.mean(e)), "1px": float(np.mean(e < 1)), "3px": float(np.mean(e < 3)), "5px": float(np.mean(e < 5))}
            got = results["predict_flow_metrics"]
            for k, v in times.items():
                rec = dict(model="small" if small else "basic", case=kind, shape="1x%dx%d" % (H, W), iters=iters, form=k, ms_median=round(statistics.median(v), 3),
                           ms_min=round(min(v), 3), ms_max=round(max(v), 3), peak_mib=round(peak[k] / 2 ** 20, 2),
                           metrics={m: (got if k == "predict_flow_metrics" else want)[m] for m in sorted(want)})
                out.append(rec)
                print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
