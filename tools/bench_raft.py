#!/usr/bin/env python3
"""One training step of the assembled RAFT model (mpiflow_amd/raft.py): the HIP glue with coarse=True feeding the fused sequence_loss, against
the same four modules - the SAME parameters - wired with upstream's torch glue, full-resolution predictions and train.py's loss; in ONE
process, the forms alternating round by round after a warm-up, every figure the median of the rounds with min and max beside it.

    python tools/bench_raft.py [--small] [--rounds 7] [--warmup 2] [--batch 8] [--height 288] [--width 960] [--iters 12] [--out profiles/raft/bench.json]

Per form: forward (grad enabled, as in training: what backward needs is kept) and forward + backward, time and peak allocated memory.  The
glue is a small share of a step; what coarse=True buys is the memory of the predictions and of what upsampling keeps for backward.

--small: the small model.  coarse="flow" feeding sequence_loss(flows, None, ...) (the fused bilinear loss) against the way without it: the
model's own upflow8 predictions (coarse=False) and train.py's loss in torch.  Same process, same parameters, alternating.  Also the loss
tail alone, on the coarse flows of one forward pass, detached: tail_fwd and tail_fwd_bwd, the same two forms."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpiflow_amd import raft_upsample  # noqa: E402
from mpiflow_amd.raft import RAFT, coords_grid  # noqa: E402
from mpiflow_amd.raft_corr import CorrBlock  # noqa: E402


def torch_glue_forward(model, image1, image2, iters):
    """upstream's RAFT.forward over the model's own modules: torch scaling, the encoder's cat, split / tanh / relu, a prediction per iteration"""
    image1 = (2 * (image1 / 255.0) - 1.0).contiguous()
    image2 = (2 * (image2 / 255.0) - 1.0).contiguous()
    fmap1, fmap2 = model.fnet([image1, image2])
    corr_fn = CorrBlock(fmap1, fmap2, radius=model.args.corr_radius)
    net, inp = torch.split(model.cnet(image1), [model.hidden_dim, model.context_dim], dim=1)
    net, inp = torch.tanh(net).contiguous(), torch.relu(inp).contiguous()
    N, _, H, W = image1.shape
    coords0 = coords_grid(N, H // 8, W // 8, image1.device)
    coords1 = coords0.clone()
    preds = []
    for _ in range(iters):
        coords1 = coords1.detach()
        net, up_mask, delta_flow = model.update_block(net, inp, corr_fn(coords1), coords1 - coords0)
        coords1 = coords1 + delta_flow
        preds.append(raft_upsample.upsample_flow(coords1 - coords0, up_mask))
    return preds


def torch_sequence_loss(preds, flow_gt, valid, gamma=0.8, max_flow=400):
    """RAFT/train.py's sequence_loss (without the metrics)"""
    mag = torch.sum(flow_gt ** 2, dim=1).sqrt()
    valid = (valid >= 0.5) & (mag < max_flow)
    loss = 0.0
    for i, p in enumerate(preds):
        loss = loss + gamma ** (len(preds) - i - 1) * (valid[:, None] * (p - flow_gt).abs()).mean()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=288)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_raft.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    model = RAFT(argparse.Namespace(small=a.small, mixed_precision=False)).to(dev).train()
    im1 = torch.randint(0, 256, (a.batch, 3, a.height, a.width), device=dev).float()
    im2 = torch.roll(im1, (2, 5), dims=(2, 3))
    gt = 5.0 * torch.randn(a.batch, 2, a.height, a.width, device=dev)
    valid = (torch.rand(a.batch, a.height, a.width, device=dev) > 0.1).float()

    def hip_coarse():
        out = model(im1, im2, iters=a.iters, coarse=True)
        return raft_upsample.sequence_loss([f for f, _ in out], [m for _, m in out], gt, valid, gamma=0.8)[0]

    def torch_glue():
        return torch_sequence_loss(torch_glue_forward(model, im1, im2, a.iters), gt, valid)

    def small_coarse_flow():
        return raft_upsample.sequence_loss(model(im1, im2, iters=a.iters, coarse="flow"), None, gt, valid, gamma=0.8)[0]

    def small_upflow8_full():
        return torch_sequence_loss(model(im1, im2, iters=a.iters), gt, valid)

    groups = {"step": dict(hip_glue_coarse=hip_coarse, torch_glue_full=torch_glue)}
    if a.small:
        with torch.no_grad():
            coarse = [f.clone().requires_grad_(True) for f in model(im1, im2, iters=a.iters, coarse="flow")]

        def clear():
            for f in coarse:
                f.grad = None

        groups = {"step": dict(coarse_flow_fused_loss=small_coarse_flow, upflow8_torch_loss=small_upflow8_full),
                  "tail": dict(coarse_flow_fused_loss=lambda: (clear(), raft_upsample.sequence_loss(coarse, None, gt, valid, gamma=0.8)[0])[1],
                               upflow8_torch_loss=lambda: (clear(), torch_sequence_loss([raft_upsample.upflow8(f) for f in coarse], gt, valid))[1])}
    forms = {(g, k): fn for g, d in groups.items() for k, fn in d.items()}
    times = {(k, b): [] for k in forms for b in (False, True)}
    peak, rise = {}, {}                                                  # peak allocated, and its rise above what was held before the call
    for r in range(a.warmup + a.rounds):
        for backward in (False, True):
            for k, fn in forms.items():
                model.zero_grad(set_to_none=True)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                held = torch.cuda.memory_allocated(dev)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                loss = fn()
                if backward:
                    loss.backward()
                t1.record()
                torch.cuda.synchronize()
                del loss
                if r >= a.warmup:
                    times[(k, backward)].append(t0.elapsed_time(t1))
                    peak[(k, backward)] = max(peak.get((k, backward), 0), torch.cuda.max_memory_allocated(dev))
                    rise[(k, backward)] = max(rise.get((k, backward), 0), torch.cuda.max_memory_allocated(dev) - held)
    out = []
    for (k, backward), v in times.items():
        rec = dict(model="small" if a.small else "basic", shape="%dx%dx%d" % (a.batch, a.height, a.width), iters=a.iters,
                   measurement=k[0] + ("_fwd_bwd" if backward else "_fwd"), form=k[1],
                   ms_median=round(statistics.median(v), 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3), peak_mib=round(peak[(k, backward)] / 2 ** 20, 1),
                   rise_mib=round(rise[(k, backward)] / 2 ** 20, 1))
        out.append(rec)
        print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
