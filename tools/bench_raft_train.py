#!/usr/bin/env python3
"""The optimizer tail of a RAFT training step (mpiflow_amd/raft_train.py) against torch's, and the whole step with either tail; in ONE process,
the forms alternating round by round after a warm-up, every figure the median of the rounds with min and max beside it (tools/bench_raft.py's
method).

    python tools/bench_raft_train.py [--rounds 7] [--warmup 2] [--reps 20] [--iters 12] [--skip-steps] [--out profiles/train/bench.json]

(a) tail: on the real basic and small parameter sets with random gradients, per form `reps` consecutive tails between two device events and
    inside a host clock that ends in a synchronise; reported per tail.  The forms:
      clipped_adamw     ClippedAdamW.step(zero_grad=True)
      torch_foreach     clip_grad_norm_ + torch.optim.AdamW(foreach=True).step() + zero_grad(set_to_none=False)
      torch_fused       the same with fused=True
    The device figure is the stream's time from the first launch to the last kernel's end, so it contains the host's launch gaps wherever the
    host is the slower side; the host figure is the whole wall time.  In a training step the device is busy with backward while the host
    queues the tail, so there the device figure is the one that adds to the step.
    Kernel launches per tail: counted by torch.profiler, one tail per form, after everything else has been measured and written.
(b) step: train_step at 8x288x960 and 3x368x496 (train.py's per-GPU batch) against the same step with clip_grad_norm_ + AdamW(fused=True) +
    zero_grad(), basic and small.

One JSON record per line; --out also writes them as one file."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpiflow_amd import raft_train, raft_upsample  # noqa: E402
from mpiflow_amd.raft import RAFT  # noqa: E402

HYPER = dict(lr=4e-4, weight_decay=1e-4, eps=1e-8)
CLIP = 1.0


def tail_forms(model, dev):
    """three copies of the model's parameters, each with its optimizer and a fixed set of random gradients -> {form: (callable, params)}"""
    forms = {}
    for name in ("clipped_adamw", "torch_foreach", "torch_fused"):
        params = [p.detach().clone().requires_grad_(True) for p in model.parameters()]
        gen = torch.Generator(device=dev).manual_seed(3)
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=gen)
        if name == "clipped_adamw":
            opt = raft_train.ClippedAdamW(params, clip=CLIP, **HYPER)
            fn = lambda opt=opt: opt.step(zero_grad=True)
        else:
            opt = torch.optim.AdamW(params, foreach=name == "torch_foreach", fused=name == "torch_fused", **HYPER)

            def fn(opt=opt, params=params):
                torch.nn.utils.clip_grad_norm_(params, CLIP)
                opt.step()
                opt.zero_grad(set_to_none=False)
        forms[name] = (fn, params)
    return forms


def timed(fn, reps):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    h0 = time.perf_counter()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps, (time.perf_counter() - h0) * 1e3 / reps


def summary(v):
    return dict(ms_median=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4))


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_raft_train.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    out = []

    def emit(rec):
        out.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    models = {name: RAFT(argparse.Namespace(small=name == "small", mixed_precision=False)).to(dev).train() for name in ("basic", "small")}
    tails = {}
    for name, model in models.items():
        forms = tails[name] = tail_forms(model, dev)
        n_tensors, n_elems = len(forms["clipped_adamw"][1]), sum(p.numel() for p in forms["clipped_adamw"][1])
        dev_ms, host_ms = {k: [] for k in forms}, {k: [] for k in forms}
        for r in range(a.warmup + a.rounds):
            for k, (fn, _) in forms.items():
                d, h = timed(fn, a.reps)
                if r >= a.warmup:
                    dev_ms[k].append(d), host_ms[k].append(h)
        for k in forms:
            emit(dict(measurement="tail", model=name, form=k, tensors=n_tensors, elements=n_elems, reps=a.reps, device=summary(dev_ms[k]), host=summary(host_ms[k])))

    if not a.skip_steps:
        for name, model in models.items():
            small = name == "small"
            for (N, H, W) in ((8, 288, 960), (3, 368, 496)):
                batch = dict(image1=torch.randint(0, 256, (N, 3, H, W), device=dev).float())
                batch["image2"] = torch.roll(batch["image1"], (2, 5), dims=(2, 3))
                batch["flow"] = 5.0 * torch.randn(N, 2, H, W, device=dev)
                batch["valid"] = (torch.rand(N, H, W, device=dev) > 0.1).float()
                args = argparse.Namespace(num_steps=1000, wdecay=HYPER["weight_decay"], epsilon=HYPER["eps"], clip=CLIP, lr=HYPER["lr"])
                ours = copy.deepcopy(model)
                opt, sched = raft_train.fetch_optimizer(args, ours)
                theirs = copy.deepcopy(model)
                topt = torch.optim.AdamW(theirs.parameters(), lr=args.lr, weight_decay=args.wdecay, eps=args.epsilon, fused=True)
                tsched = torch.optim.lr_scheduler.OneCycleLR(topt, args.lr, args.num_steps + 100, pct_start=0.05, cycle_momentum=False, anneal_strategy="linear")

                def torch_tail_step():
                    topt.zero_grad()
                    res = theirs(batch["image1"], batch["image2"], iters=a.iters, coarse="flow" if small else True)
                    if small:
                        loss, metrics = raft_upsample.sequence_loss(res, None, batch["flow"], batch["valid"], 0.8)
                    else:
                        loss, metrics = raft_upsample.sequence_loss([f for f, _ in res], [m for _, m in res], batch["flow"], batch["valid"], 0.8)
                    loss.backward()
                    torch.nn.utils.clip_grad_norm_(theirs.parameters(), args.clip)
                    topt.step()
                    tsched.step()

                forms = dict(train_step=lambda: raft_train.train_step(ours, opt, sched, batch, iters=a.iters, gamma=0.8), torch_fused_tail=torch_tail_step)
                dev_ms, host_ms = {k: [] for k in forms}, {k: [] for k in forms}
                for r in range(a.warmup + a.rounds):
                    for k, fn in forms.items():
                        d, h = timed(fn, 1)
                        if r >= a.warmup:
                            dev_ms[k].append(d), host_ms[k].append(h)
                for k in forms:
                    emit(dict(measurement="step", model=name, shape="%dx%dx%d" % (N, H, W), iters=a.iters, form=k, device=summary(dev_ms[k]), host=summary(host_ms[k])))
                del ours, theirs, opt, topt, batch
                torch.cuda.empty_cache()

    if not a.skip_launch_count:
        for name, forms in tails.items():
            for k, (fn, _) in forms.items():
                try:
                    emit(dict(measurement="launches_per_tail", model=name, form=k, kernels=count_launches(fn)))
                except Exception as e:                                   # noqa: BLE001 - a profiler that is not there must not cost the timings
                    emit(dict(measurement="launches_per_tail", model=name, form=k, kernels=None, error="%s: %s" % (type(e).__name__, e)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
