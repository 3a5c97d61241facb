#!/usr/bin/env python3
"""RAFT's update block: the fused GRU (mpiflow_amd/raft_update.py) against the cat-form torch block, in ONE process, the forms alternating
round by round after a warm-up, every figure the median of the rounds with min and max beside it.

    python tools/bench_update.py [--rounds 15] [--warmup 3] [--out profiles/update/bench.json]

Four measurements per shape, each forward and forward + backward:
  gru     the GRU alone, fused (with and without the hoisted context) against the cat form
  gates   the four gate kernels alone against the torch pointwise chain on the same convolution outputs: time, algorithmic bytes, fraction of
          the 8 TB/s HBM roofline
  block   the whole update block over 12 iterations, hoist_context on / off, and with the cat-form GRU in the same block
  convs   the GRU's convolutions alone, split form (x -> 3C, h -> 2C, rh -> C; hoisted: motion -> 3C) against cat form (three C+Cx -> C), so
          that a MIOpen regression from the changed shapes shows up on its own
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpiflow_amd import ops, raft_update as ru  # noqa: E402

ROOFLINE = 8.0e12
# (name, GRU class, B, H, W, C, context channels, motion channels, corr planes)
SHAPES = [("basic_8x36x120", "SepConvGRU", 8, 36, 120, 128, 128, 128, 324), ("basic_8x48x160", "SepConvGRU", 8, 48, 160, 128, 128, 128, 324),
          ("small_8x36x120", "ConvGRU", 8, 36, 120, 96, 64, 82, 196)]


def cat_gru(gru, h, x):
    """the cat form on the module's own parameters"""
    for suffix, _, pad in gru.HALVES:
        cz, cr, cq = (getattr(gru, "conv%s%s" % (g, suffix)) for g in "zrq")
        hx = torch.cat([h, x], dim=1)
        z, r = torch.sigmoid(cz(hx)), torch.sigmoid(cr(hx))
        q = torch.tanh(cq(torch.cat([r * h, x], dim=1)))
        h = (1 - z) * h + z * q
    return h


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


def report(out, shape, what, res, extra=None):
    for k, (med, lo, hi) in res.items():
        rec = dict(shape=shape, measurement=what, form=k, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
        if extra and k in extra:
            rec.update(extra[k])
        out.append(rec)
        print(json.dumps(rec))


def bench_shape(out, name, cls, B, H, W, C, n_ctx, n_m, planes, rounds, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    gru = getattr(ru, cls)(hidden_dim=C, input_dim=n_ctx + n_m).to(dev)
    h0 = torch.tanh(torch.randn(B, C, H, W, device=dev))
    inp, motion = torch.relu(torch.randn(B, n_ctx, H, W, device=dev)), torch.relu(torch.randn(B, n_m, H, W, device=dev))
    x = torch.cat([inp, motion], dim=1)
    cot = torch.randn(B, C, H, W, device=dev)

    # ---- gru
    def gru_run(form, backward):
        def run():
            with torch.set_grad_enabled(backward):
                h = h0.clone().requires_grad_(backward)
                if form == "cat":
                    o = cat_gru(gru, h, x)
                elif form == "fused":
                    o = gru(h, x)
                else:
                    o = gru(h, motion, context=ctx_holder[backward])
                if backward:
                    o.backward(cot, retain_graph=(form == "fused_context"))       # the context's graph is shared by the rounds
        return run
    with torch.no_grad():
        ctx_ng = gru.context(inp)
    ctx_holder = {False: ctx_ng, True: gru.context(inp)}
    for backward in (False, True):
        res = measure({f: gru_run(f, backward) for f in ("cat", "fused", "fused_context")}, rounds, warmup)
        report(out, name, "gru_" + ("fwd_bwd" if backward else "fwd"), res)
        gru.zero_grad(set_to_none=True)

    # ---- gates: the convolution outputs of one half as the fused module lays them out
    hg, xg, cx, qg = (torch.randn(B, k * C, H, W, device=dev) for k in (2, 3, 3, 1))
    g_h, g_rh = torch.randn_like(h0), torch.randn_like(h0)
    zt = [(hg, 0), (xg, 0), (cx, 0)]
    rt = [(hg, C), (xg, C), (cx, C)]
    qt = [(qg, 0), (xg, 2 * C), (cx, 2 * C)]
    g3, g2, dq = torch.empty_like(xg), torch.empty_like(hg), torch.empty_like(qg)
    n_bytes = h0.numel() * 4

    def hip_fwd():
        ops.gru_reset(h0, rt)
        ops.gru_update(h0, zt, qt)

    def hip_bwd():
        dh = ops.gru_update_backward(g_h, h0, zt, qt, dz=[(g3, 0), (g2, 0)], dq=[(g3, 2 * C), (dq, 0)])
        ops.gru_reset_backward(g_rh, h0, rt, dr=[(g3, C), (g2, C)], dh=dh)

    def torch_chain(backward):
        def run():
            with torch.set_grad_enabled(backward):
                hh = h0.clone().requires_grad_(backward)
                t = [v.requires_grad_(backward) for v in (hg.detach(), xg.detach(), cx.detach(), qg.detach())]
                pre = t[0] + t[1][:, :2 * C] + t[2][:, :2 * C]
                z, r = torch.sigmoid(pre[:, :C]), torch.sigmoid(pre[:, C:])
                rh = r * hh
                q = torch.tanh(t[3] + t[1][:, 2 * C:] + t[2][:, 2 * C:])
                o = (1 - z) * hh + z * q
                if backward:
                    torch.autograd.backward([o, rh], [g_h, g_rh])
        return run
    fwd_bytes, bwd_bytes = (5 + 8) * n_bytes, (13 + 9) * n_bytes        # reset 4 reads + 1 write, update 7 + 1; update_bwd 8 + 5, reset_bwd 6 + 3
    res = measure(dict(hip=hip_fwd, torch=torch_chain(False)), rounds, warmup)
    report(out, name, "gates_fwd", res, dict(hip=dict(bytes=fwd_bytes, roofline_fraction=round(fwd_bytes / (res["hip"][0] * 1e-3) / ROOFLINE, 3))))
    res = measure(dict(hip=hip_bwd, torch_fwd_bwd=torch_chain(True), torch_fwd=torch_chain(False)), rounds, warmup)
    report(out, name, "gates_bwd", res, dict(hip=dict(bytes=bwd_bytes, roofline_fraction=round(bwd_bytes / (res["hip"][0] * 1e-3) / ROOFLINE, 3))))

    # ---- convs alone
    def convs(form, backward):
        w = {}
        for suffix, ksize, pad in gru.HALVES:
            kh, kw = (ksize, ksize) if isinstance(ksize, int) else ksize
            mk = lambda co, ci: (torch.randn(co, ci, kh, kw, device=dev) * 0.02).requires_grad_(True)
            w[suffix] = dict(cat=[mk(C, C + n_ctx + n_m) for _ in range(3)], split=[mk(3 * C, n_ctx + n_m), mk(2 * C, C), mk(C, C)],
                             hoisted=[mk(3 * C, n_m), mk(2 * C, C), mk(C, C)])
        hx = torch.cat([h0, x], dim=1)

        def run():
            with torch.set_grad_enabled(backward):
                outs = []
                srcs = dict(cat=[hx, hx, hx], split=[x, h0, h0], hoisted=[motion, h0, h0])[form]
                srcs = [s.detach().requires_grad_(backward) for s in srcs]
                for suffix, _, pad in gru.HALVES:
                    outs += [F.conv2d(s, wt, None, padding=pad) for s, wt in zip(srcs, w[suffix][form])]
                if backward:
                    torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
        return run
    for backward in (False, True):
        res = measure({f: convs(f, backward) for f in ("cat", "split", "hoisted")}, rounds, warmup)
        report(out, name, "convs_" + ("fwd_bwd" if backward else "fwd"), res)

    # ---- block over 12 iterations
    args = types.SimpleNamespace(corr_levels=4, corr_radius=4 if cls == "SepConvGRU" else 3)
    Block = ru.BasicUpdateBlock if cls == "SepConvGRU" else ru.SmallUpdateBlock
    blk = Block(args).to(dev)
    corr, flow = torch.randn(B, planes, H, W, device=dev), torch.randn(B, 2, H, W, device=dev)

    class CatGRU(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, hh, motion_features, context=None):
            return cat_gru(self.inner, hh, torch.cat([context, motion_features], dim=1))

    def block_run(form, backward):
        def run():
            blk.hoist_context = form == "hoisted"
            blk.reset()
            fused_gru = blk.gru
            if form == "cat":                                            # the same block, the GRU in cat form, inp passed through as the "context"
                blk.gru = CatGRU(fused_gru)
                blk._context = lambda t: t
            try:
                with torch.set_grad_enabled(backward):
                    net = h0.clone().requires_grad_(backward)
                    ii = inp.clone().requires_grad_(backward)
                    total = 0.0
                    for _ in range(12):
                        res = blk(net, ii, corr, flow)
                        net = res[0]
                        total = total + res[2].sum()
                    if backward:
                        (total + net.sum()).backward()
            finally:
                if form == "cat":
                    blk.gru = fused_gru
                    del blk._context
        return run
    for backward in (False, True):
        res = measure({f: block_run(f, backward) for f in ("cat", "unhoisted", "hoisted")}, rounds, warmup)
        report(out, name, "block12_" + ("fwd_bwd" if backward else "fwd"), res)
        blk.zero_grad(set_to_none=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_update.py needs a GPU"
    out = []
    for s in SHAPES:
        bench_shape(out, *s, rounds=a.rounds, warmup=a.warmup)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
