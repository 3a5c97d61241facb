#!/usr/bin/env python3
"""Time the tail of a RAFT training step two ways on one GPU, in one process, alternating: (a) a plain-torch composite of the same math
(softmax over the 9 taps, the 3 x 3 neighbourhood of 8 * flow, broadcast product, sum, permute; then the masked L1 mean of every
prediction) and (b) mpiflow_amd.raft_upsample.sequence_loss on the coarse flows and masks; forward only, forward plus backward, and the
peak memory of each.  Then each of the four kernels alone, with its algorithmic bytes and the fraction of the HBM roofline they amount to
(bytes the algorithm has to move over the time, against 8.0 TB/s).

    python tools/bench_upsample.py [--reps 20] [--warmup 3] [--iters 12] [--shapes 8x36x120,8x48x160] [--json PATH]

Device time from events, median of --reps after --warmup.  Prints one JSON line per shape and two tables; with --json, writes the numbers."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpiflow_amd import ops, raft_upsample  # noqa: E402

GAMMA, MAX_FLOW, HBM_PEAK = 0.8, 400.0, 8.0e12


def composite_upsample(flow, mask):
    N, _, H, W = flow.shape
    p = torch.softmax(mask.view(N, 1, 9, 8, 8, H, W), dim=2)
    padded = F.pad(8 * flow, (1, 1, 1, 1))
    nb = torch.stack([padded[:, :, k // 3:k // 3 + H, k % 3:k % 3 + W] for k in range(9)], dim=2)      # [N,2,9,H,W]
    up = (p * nb.view(N, 2, 9, 1, 1, H, W)).sum(dim=2)
    return up.permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * H, 8 * W)


def composite_loss(flows, masks, gt, valid):
    n = len(flows)
    v = (valid >= 0.5) & (torch.sqrt((gt ** 2).sum(dim=1)) < MAX_FLOW)
    loss = 0.0
    for i in range(n):
        loss = loss + GAMMA ** (n - i - 1) * (v[:, None] * (composite_upsample(flows[i], masks[i]) - gt).abs()).mean()
    up = composite_upsample(flows[-1], masks[-1]).detach()
    epe = torch.sqrt(((up - gt) ** 2).sum(dim=1)).view(-1)[v.view(-1)]
    return loss, {"epe": epe.mean().item(), "1px": (epe < 1).float().mean().item(), "3px": (epe < 3).float().mean().item(),
                  "5px": (epe < 5).float().mean().item()}


def fused_loss(flows, masks, gt, valid):
    return raft_upsample.sequence_loss(flows, masks, gt, valid, gamma=GAMMA, max_flow=MAX_FLOW)


def step(fn, flows, masks, gt, valid, backward):
    if backward:
        flows, masks = [t.detach().requires_grad_(True) for t in flows], [t.detach().requires_grad_(True) for t in masks]
    with torch.set_grad_enabled(backward):
        loss, _ = fn(flows, masks, gt, valid)
        if backward:
            loss.backward()
    return loss


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--shapes", default="8x36x120,8x48x160")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for shape in a.shapes.split(","):
        N, H, W = [int(v) for v in shape.split("x")]
        gen = torch.Generator(device="cpu").manual_seed(1)
        flows = [(3.0 * torch.randn(N, 2, H, W, generator=gen)).to(dev) for _ in range(a.iters)]
        masks = [(2.0 * torch.randn(N, 576, H, W, generator=gen)).to(dev) for _ in range(a.iters)]
        gt = (30.0 * torch.randn(N, 2, 8 * H, 8 * W, generator=gen)).to(dev)
        valid = (torch.rand(N, 8 * H, 8 * W, generator=gen) > 0.1).float().to(dev)
        row = dict(N=N, H=H, W=W, iters=a.iters)
        forms = (("torch", composite_loss), ("fused", fused_loss))
        l_t, l_f = float(step(composite_loss, flows, masks, gt, valid, False)), float(step(fused_loss, flows, masks, gt, valid, False))
        row["loss_torch"], row["loss_fused"] = l_t, l_f
        assert abs(l_t - l_f) <= 1e-5 * abs(l_t), (l_t, l_f)             # faster and different is not faster
        for backward in (False, True):
            ts = {n: [] for n, _ in forms}
            for k in range(a.warmup + a.reps):                         # alternating: one step of each form per round
                for n, fn in forms:
                    t = timed(lambda: step(fn, flows, masks, gt, valid, backward))
                    if k >= a.warmup:
                        ts[n].append(t)
            for n, _ in forms:
                row["%s_%s_ms" % (n, "fwd_bwd" if backward else "fwd")] = statistics.median(ts[n])
                row["%s_%s_ms_min_max" % (n, "fwd_bwd" if backward else "fwd")] = [min(ts[n]), max(ts[n])]
        for n, fn in forms:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            step(fn, flows, masks, gt, valid, False)
            torch.cuda.synchronize()
            row["%s_fwd_peak_MB" % n] = (torch.cuda.max_memory_allocated(dev) - base) / 1e6
            torch.cuda.reset_peak_memory_stats(dev)
            step(fn, flows, masks, gt, valid, True)
            torch.cuda.synchronize()
            grads = 4 * sum(t.numel() for t in flows + masks)
            row["%s_fwd_bwd_peak_MB" % n] = (torch.cuda.max_memory_allocated(dev) - base) / 1e6
            row["%s_fwd_bwd_peak_beyond_grads_MB" % n] = (torch.cuda.max_memory_allocated(dev) - base - grads) / 1e6
        # the four kernels alone; floats the algorithm has to move per coarse pixel
        f, m = flows[-1], masks[-1]
        cot, g = torch.randn_like(gt), torch.ones((), device=dev)
        px = N * H * W
        kernels = (("upsample_flow", lambda: ops.upsample_flow(f, m), 576 + 2 + 128),
                   ("upsample_flow_backward", lambda: ops.upsample_flow_backward(f, m, cot), 576 + 2 + 128 + 576 + 2 + 2 * 18),
                   ("flow_loss_term", lambda: ops.flow_loss_term(f, m, gt, valid, MAX_FLOW), 576 + 2 + 128 + 64),
                   ("flow_loss_term_backward", lambda: ops.flow_loss_term_backward(f, m, gt, valid, g, MAX_FLOW), 576 + 2 + 128 + 64 + 576 + 2 + 2 * 18))
        ts = {n: [] for n, _, _ in kernels}
        for k in range(a.warmup + a.reps):
            for n, fn, _ in kernels:
                t = timed(fn)
                if k >= a.warmup:
                    ts[n].append(t)
        for n, _, floats in kernels:
            ms = statistics.median(ts[n])
            row[n + "_ms"], row[n + "_MB"] = ms, floats * 4 * px / 1e6
            row[n + "_hbm_fraction"] = floats * 4 * px / (ms * 1e-3) / HBM_PEAK
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("\n| N x H x W | torch fwd ms | fused fwd ms | torch fwd+bwd ms | fused fwd+bwd ms | torch fwd peak MB | fused fwd peak MB | "
          "torch fwd+bwd peak MB | fused fwd+bwd peak MB |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %d x %d x %d | %.3f | %.3f | %.3f | %.3f | %.1f | %.3f | %.1f | %.1f |" % (
            r["N"], r["H"], r["W"], r["torch_fwd_ms"], r["fused_fwd_ms"], r["torch_fwd_bwd_ms"], r["fused_fwd_bwd_ms"],
            r["torch_fwd_peak_MB"], r["fused_fwd_peak_MB"], r["torch_fwd_bwd_peak_MB"], r["fused_fwd_bwd_peak_MB"]))
    print("\n| N x H x W | kernel | ms | algorithmic MB | fraction of 8.0 TB/s |")
    print("|---|---|---|---|---|")
    for r in rows:
        for n in ("upsample_flow", "upsample_flow_backward", "flow_loss_term", "flow_loss_term_backward"):
            print("| %d x %d x %d | %s | %.4f | %.1f | %.3f |" % (r["N"], r["H"], r["W"], n, r[n + "_ms"], r[n + "_MB"], r[n + "_hbm_fraction"]))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
