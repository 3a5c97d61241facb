#!/usr/bin/env python3
"""The training-time kernels of utils/mpi (mpf_mpi_train.hip) against torch-op restatements of the same definitions on the same device, on one stream:

  loss        disparity_consistency_src_to_tgt, forward plus backward (both gradients), at B = 4, 384 x 1280
  sample_pdf  ops.sample_pdf at B = 1, N = 384 * 1280, S = 64, N_samples = 64, values contiguous and expanded over the rays

The project had no such functions before, so the restatement written here with torch ops is the baseline, not the code under test.  Method: warm-up,
then `rounds` rounds in which the two forms ALTERNATE, each timed with HIP events around `reps` calls; medians.  Bytes: the tensors' compulsory traffic
(every input read once, every output written once), which the achieved GB/s is quoted against.  Peak memory: torch's allocator peak above what was
allocated before the call.  The tool fails when a fused form is not faster than its restatement, when sample_pdf allocates more than its output, or
when the loss allocates a frame-sized tensor beside its two gradients.

    python tools/bench_mpi_training.py [--json PATH] [--small]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_loss(K_src_inv, disparity_src, G_tgt_src, K_tgt, disparity_tgt, grid):
    """the definition of INTEGRATION.md section 21 in torch ops"""
    import torch
    B, _, H, W = disparity_src.shape
    xyz = torch.matmul(K_src_inv, grid).reshape(B, 3, H, W) * torch.reciprocal(disparity_src)
    xyz = xyz.view(B, 3, H * W)
    p = torch.matmul(G_tgt_src, torch.cat((xyz, torch.ones_like(xyz[:, 0:1])), dim=1))[:, 0:3]
    q = torch.matmul(K_tgt, p)
    pxpy = q[:, 0:2] / q[:, 2:]
    mask = (pxpy[:, 0:1] >= 0) & (pxpy[:, 0:1] <= W - 1) & (pxpy[:, 1:2] >= 0) & (pxpy[:, 1:2] <= H - 1)
    with torch.no_grad():
        i = torch.round(pxpy).to(torch.int64)
        idx = i[:, 0:1].clamp(0, W - 1) + W * i[:, 1:2].clamp(0, H - 1)
    tgt = torch.gather(disparity_tgt.view(B, 1, H * W), 2, idx)
    return torch.mean(torch.abs(torch.reciprocal(p[:, 2:]) - tgt)[mask])


def torch_sample_pdf(values, weights, u):
    import torch
    B, N, S = weights.size(0), weights.size(2), weights.size(3)
    n = u.size(3)
    edges = torch.cat((values[..., 0:1], (values[..., 1:] + values[..., :-1]) * 0.5, values[..., -1:]), dim=3)
    pdf = weights / (torch.sum(weights, dim=3, keepdim=True) + 1e-5)
    cdf = torch.cat((torch.zeros((B, 1, N, 1), dtype=pdf.dtype, device=pdf.device), torch.cumsum(pdf, dim=3)), dim=3)
    idx = torch.searchsorted(cdf, u, right=True)
    both = torch.cat((torch.clamp(idx - 1, min=0), torch.clamp(idx, max=S)), dim=3)
    c, e = torch.gather(cdf, 3, both), torch.gather(edges, 3, both)
    ci, bi = c[..., n:] - c[..., :n], e[..., n:] - e[..., :n]
    t = (u - c[..., :n]) / torch.clamp(ci, min=1e-5)
    t = torch.where(ci <= 1e-4, torch.full_like(t, 0.5), t)
    return e[..., :n] + t * bi


def timed(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def peak_above(fn):
    import torch
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del keep
    return peak


def alternate(forms, reps, rounds):
    for fn in forms.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            ms[k].append(timed(fn, reps))
    return {k: statistics.median(v) for k, v in ms.items()}, {k: (min(v), max(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--small", action="store_true", help="a tenth of the sizes: a rehearsal, not a measurement")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_mpi_training.py measures on a GPU"
    from mpiflow_amd import ops
    from mpiflow_amd.utils.mpi import mpi_rendering as R
    from mpiflow_amd.utils.mpi.homography_sampler import HomographySample
    dev = torch.device("cuda:0")
    records, failed = [], []
    B, H, W = (4, 384, 1280) if not a.small else (2, 96, 160)
    g = torch.Generator(device="cpu").manual_seed(0)
    K = torch.tensor([[0.9 * W, 0, (W - 1) / 2], [0, 0.9 * W, (H - 1) / 2], [0, 0, 1]], dtype=torch.float64)
    Ki = torch.linalg.inv(K).float().repeat(B, 1, 1).to(dev)
    Kt = K.float().repeat(B, 1, 1).to(dev)
    G = torch.eye(4).repeat(B, 1, 1)
    G[:, 0, 3], G[:, 1, 3], G[:, 2, 3] = 0.06, -0.04, 0.03
    G = G.to(dev)
    d_src = (0.2 + 0.8 * torch.rand((B, 1, H, W), generator=g)).to(dev).requires_grad_(True)
    d_tgt = (0.2 + 0.8 * torch.rand((B, 1, H, W), generator=g)).to(dev).requires_grad_(True)
    mesh = HomographySample(H, W, dev).meshgrid
    grid = mesh.reshape(1, 3, H * W).repeat(B, 1, 1)

    def fused_loss():
        loss = R.disparity_consistency_src_to_tgt(mesh, Ki, d_src, G, Kt, d_tgt)
        return torch.autograd.grad(loss, [d_src, d_tgt])

    def restated_loss():
        return torch.autograd.grad(torch_loss(Ki, d_src, G, Kt, d_tgt, grid), [d_src, d_tgt])

    a_, b_ = fused_loss(), restated_loss()
    agree = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(a_, b_)]
    med, spread = alternate(dict(fused=fused_loss, torch=restated_loss), 20, 7)
    nbytes = 16 * B * H * W
    rec = dict(what="disparity_consistency_src_to_tgt forward + backward, B = %d, %d x %d" % (B, H, W), ms_fused=round(med["fused"], 4),
               ms_torch_ops=round(med["torch"], 4), ms_fused_min_max=[round(x, 4) for x in spread["fused"]],
               ms_torch_min_max=[round(x, 4) for x in spread["torch"]], speedup=round(med["torch"] / med["fused"], 2), compulsory_bytes=nbytes,
               fused_GB_per_s=round(nbytes / med["fused"] / 1e6, 1), peak_bytes_fused=peak_above(fused_loss), peak_bytes_torch_ops=peak_above(restated_loss),
               gradients_rel_diff=agree)
    records.append(rec)
    print(json.dumps(rec), flush=True)
    if not med["fused"] < med["torch"]:
        failed.append("the fused loss is not faster than its torch-op restatement")
    # any materialised intermediate of the chain is at least one [B,1,H,W] tensor: the peak must stay below the two gradients plus one such tensor
    if rec["peak_bytes_fused"] >= 3 * 4 * B * H * W:
        failed.append("the fused loss allocates a frame-sized temporary beside its two gradients")

    Bp, N, S, NS = (1, 384 * 1280, 64, 64) if not a.small else (1, 96 * 160, 64, 64)
    base = torch.linspace(1.0, 0.01, S).view(1, 1, 1, S).repeat(Bp, 1, 1, 1).to(dev)
    weights = torch.rand((Bp, 1, N, S), generator=g).to(dev)
    u = torch.rand((Bp, 1, N, NS), generator=g).to(dev)
    for layout, values in (("contiguous", base.expand(Bp, 1, N, S).contiguous()), ("expanded", base.expand(Bp, 1, N, S))):
        out = torch.empty_like(u)
        forms = dict(fused=lambda: ops.sample_pdf(values, weights, u, out=out), torch=lambda: torch_sample_pdf(values, weights, u))
        # the two forms round their cdf differently (torch's device cumsum is a parallel scan), so among millions of draws a few sit on the other side of
        # the 1e-4 interval switch and differ by up to half a bin; everywhere else the forms agree to rounding
        diff = (forms["fused"]() - forms["torch"]()).abs()
        apart, diff = float((diff > 1e-5).float().mean()), float(diff.max())
        med, spread = alternate(forms, 10, 7)
        nbytes = 4 * Bp * N * (S + 2 * NS) + 4 * (Bp * N * S if layout == "contiguous" else Bp * S)
        rec = dict(what="sample_pdf, B = %d, N = %d, S = %d, N_samples = %d, values %s" % (Bp, N, S, NS, layout), ms_fused=round(med["fused"], 4),
                   ms_torch_ops=round(med["torch"], 4), ms_fused_min_max=[round(x, 4) for x in spread["fused"]],
                   ms_torch_min_max=[round(x, 4) for x in spread["torch"]], speedup=round(med["torch"] / med["fused"], 2), compulsory_bytes=nbytes,
                   fused_GB_per_s=round(nbytes / med["fused"] / 1e6, 1), peak_bytes_fused=peak_above(lambda: ops.sample_pdf(values, weights, u)),
                   peak_bytes_torch_ops=peak_above(forms["torch"]), one_BNS_tensor_bytes=4 * Bp * N * S, max_abs_diff=diff,
                   fraction_of_draws_more_than_1e_5_apart=apart)
        records.append(rec)
        print(json.dumps(rec), flush=True)
        if not med["fused"] < med["torch"]:
            failed.append("the fused sample_pdf (%s) is not faster than its torch-op restatement" % layout)
        if rec["peak_bytes_fused"] > 4 * Bp * N * NS + (1 << 20):
            failed.append("the fused sample_pdf (%s) allocates more than its output" % layout)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")
    for msg in failed:
        print("FAILED: " + msg)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
