#!/usr/bin/env python3
"""Record RAFT's convex upsampling and sequence loss by RUNNING THE REFERENCE ITSELF (RAFT.upsample_flow of RAFT/core/raft.py, called
unbound, and sequence_loss of RAFT/train.py, CPU) -> tests/golden/raft_upsample.npz.

    python tests/golden/make_upsample_golden.py [--out PATH]        (in the build container: needs the reference tree, numpy, torch)

Per case, in fp32 and on .double() inputs: every iteration's prediction, sequence_loss over all of them (loss and metrics) and over each one
alone with gamma = 1 (the per-iteration terms), the gradients of the loss for every iteration's flow and mask, and for the last iteration
the gradients of upsample_flow alone for a fixed random cotangent.  err32 = max |fp32 run - double run| over the WHOLE array is stored per
array: the yardstick of tests/test_raft_upsample.py.

train.py imports cv2, matplotlib, tensorboard, evaluate and datasets at its top; the two functions never touch them, so empty stand-in
modules are put into sys.modules while it loads.

What the file holds, to stay far below the 1 MiB a committed file may have:
  * inputs are draws of np.random.RandomState(seed), rebuilt by case_inputs(); the file carries their float64 sums as a check.  flow_gt is
    the exception: fix_flow_gt() below moves entries of it until the two conditions hold, and the file stores the moved entries (flat index,
    value) for apply_fixes().
  * of each large array N_SAMPLE entries at flat indices drawn by sample_index(), fp32 and float64, plus err32 and max |ref64|.
  * in full: the per-iteration terms, the loss, upstream's metrics and the five metric accumulators, in both precisions.

The two conditions on flow_gt (checked here on the double run, re-asserted by the test from its own formula):
  * no sign ties: every entry of every iteration has |pred64 - flow_gt| >= TIE_MARGIN, so the L1 gradient's sign is the same in every
    precision and no entry has to be left out of a comparison;
  * no threshold ties: | |flow_gt| - max_flow | >= 1 on every pixel (some pixels are set above max_flow on purpose) and the last prediction's
    epe is at least EPE_MARGIN away from 1, 3 and 5 (some pixels are planted below each threshold so that the counts are not all zero)."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

N_SAMPLE = 600
MAX_FLOW = 400.0
GAMMA = 0.8
TIE_MARGIN = 1e-2
EPE_MARGIN = 1e-3

# (name, N, H, W, iterations, seed)
CASES = [
    ("tiny_1x5x7", 1, 5, 7, 3, 9200),
    ("h1_2x1x70", 2, 1, 70, 2, 9210),
    ("w1_2x9x1", 2, 9, 1, 2, 9220),
    ("mid_1x13x83", 1, 13, 83, 3, 9230),
    ("real_2x36x120", 2, 36, 120, 12, 9240),
]


def case_inputs(N, H, W, iters, seed):
    """(flows, masks, flow_gt, valid, cot) of a case, float32: flows / masks are lists over the iterations; flow_gt BEFORE apply_fixes()"""
    rs = np.random.RandomState(seed)
    target = rs.standard_normal((N, 2, H, W)) * 3.0                              # coarse flows drift towards a field of a few coarse pixels
    flows = [(target * (k + 1) / iters + 0.5 * rs.standard_normal((N, 2, H, W))).astype(np.float32) for k in range(iters)]
    masks = [(2.0 * rs.standard_normal((N, 576, H, W))).astype(np.float32) for _ in range(iters)]
    flow_gt = (30.0 * rs.standard_normal((N, 2, 8 * H, 8 * W))).astype(np.float32)
    far = rs.rand(N, 8 * H, 8 * W) < 0.02                                         # beyond max_flow on purpose
    for c in range(2):
        flow_gt[:, c][far] = (np.where(rs.rand(int(far.sum())) < 0.5, -1.0, 1.0) * (300.0 + 20.0 * rs.rand(int(far.sum())))).astype(np.float32)
    valid = (rs.rand(N, 8 * H, 8 * W) > 0.1).astype(np.float32)
    cot = rs.standard_normal((N, 2, 8 * H, 8 * W)).astype(np.float32)
    return flows, masks, flow_gt, valid, cot


def apply_fixes(flow_gt, idx, val):
    out = flow_gt.copy()
    out.reshape(-1)[idx] = val
    return out


def sample_index(n, seed):
    return np.random.RandomState(seed + 1).randint(0, n, N_SAMPLE)


def load_reference():
    """(RAFT class, train module) of the reference, train.py's unused imports replaced by empty modules while it loads"""
    from ref_harness import REFERENCE_ROOT
    raft_dir = os.path.join(REFERENCE_ROOT, "RAFT")
    sys.path.insert(0, os.path.join(raft_dir, "core"))
    sys.dont_write_bytecode = True
    stand_ins = {}
    for name in ("cv2", "matplotlib", "matplotlib.pyplot", "evaluate", "datasets", "torch.utils.tensorboard"):
        stand_ins[name] = sys.modules.get(name)
        sys.modules[name] = types.ModuleType(name)
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["torch.utils.tensorboard"].SummaryWriter = object
    try:
        spec = importlib.util.spec_from_file_location("ref_raft_train", os.path.join(raft_dir, "train.py"))
        train = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(train)
    finally:
        for name, old in stand_ins.items():
            if old is None:
                del sys.modules[name]
            else:
                sys.modules[name] = old
    return train.RAFT, train


def predictions(RAFT, flows, masks, dtype):
    with torch.no_grad():
        return [RAFT.upsample_flow(None, torch.from_numpy(f).to(dtype), torch.from_numpy(m).to(dtype)).numpy() for f, m in zip(flows, masks)]


def fix_flow_gt(flow_gt, preds64, seed):
    """Plant pixels under each epe threshold of the last prediction, then move entries of flow_gt until both conditions hold."""
    rs = np.random.RandomState(seed + 2)
    gt = flow_gt.copy()
    N, _, H8, W8 = gt.shape
    npix = N * H8 * W8
    last = preds64[-1]
    pick = rs.choice(npix, size=max(3, npix // 50), replace=False)
    for q, pix in enumerate(pick):
        n, y, x = np.unravel_index(pix, (N, H8, W8))
        r = (0.5, 2.0, 4.0)[q % 3]                                                # epe of the planted pixel: below 1, 3 and 5 in turn
        ang = rs.uniform(0.2, 1.3)
        gt[n, 0, y, x] = np.float32(last[n, 0, y, x] + r * np.cos(ang))
        gt[n, 1, y, x] = np.float32(last[n, 1, y, x] + r * np.sin(ang))
    for _ in range(100):
        g64 = gt.astype(np.float64)
        tie = np.zeros(gt.shape, bool)
        for p in preds64:
            tie |= np.abs(p - g64) < TIE_MARGIN
        epe = np.sqrt(((last - g64) ** 2).sum(1))
        near = np.zeros(epe.shape, bool)
        for thr in (1.0, 3.0, 5.0):
            near |= np.abs(epe - thr) < 4 * EPE_MARGIN
        tie[:, 0] |= near
        if not tie.any():
            break
        gt[tie] += np.float32(0.05)
    else:
        raise RuntimeError("flow_gt could not be moved clear of the ties")
    mag = np.sqrt((gt.astype(np.float64) ** 2).sum(1))
    assert (np.abs(mag - MAX_FLOW) >= 1.0).all() and (mag > MAX_FLOW).any()
    return gt


def accumulators(pred, gt, valid, dtype):
    """the five metric accumulators from the reference's own last prediction, in `dtype`: sum of epe over v, counts below 1, 3, 5, count of v"""
    pred, gt = pred.astype(dtype), gt.astype(dtype)
    v = (valid >= 0.5) & (np.sqrt((gt ** 2).sum(1)) < dtype(MAX_FLOW))
    epe = np.sqrt(((pred - gt) ** 2).sum(1))[v]
    return np.array([epe.astype(np.float64).sum(), (epe < 1).sum(), (epe < 3).sum(), (epe < 5).sum(), v.sum()], np.float64)


def run_case(RAFT, train, flows, masks, gt, valid, cot, dtype):
    t = lambda a: torch.from_numpy(a).to(dtype)
    fl = [t(f).requires_grad_(True) for f in flows]
    mk = [t(m).requires_grad_(True) for m in masks]
    preds = [RAFT.upsample_flow(None, f, m) for f, m in zip(fl, mk)]
    assert preds[0].dtype == dtype
    loss, metrics = train.sequence_loss(preds, t(gt), t(valid), gamma=GAMMA, max_flow=MAX_FLOW)
    loss.backward()
    res = dict(loss=np.float64(loss.item()), metrics=np.array([metrics[k] for k in ("epe", "1px", "3px", "5px")], np.float64),
               grad_flow=[f.grad.numpy() for f in fl], grad_mask=[m.grad.numpy() for m in mk], pred_last=preds[-1].detach().numpy())
    with torch.no_grad():
        res["terms"] = np.array([train.sequence_loss([p.detach()], t(gt), t(valid), gamma=1.0, max_flow=MAX_FLOW)[0].item() for p in preds], np.float64)
    f, m = t(flows[-1]).requires_grad_(True), t(masks[-1]).requires_grad_(True)
    RAFT.upsample_flow(None, f, m).backward(t(cot))
    res["up_grad_flow"], res["up_grad_mask"] = f.grad.numpy(), m.grad.numpy()
    res["acc"] = accumulators(res["pred_last"], gt, valid, np.float32 if dtype == torch.float32 else np.float64)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "raft_upsample.npz"))
    a = ap.parse_args()
    RAFT, train = load_reference()
    torch.manual_seed(0)
    rec = {"numpy_version": np.array(np.__version__), "torch_version": np.array(torch.__version__), "n_sample": np.int64(N_SAMPLE),
           "names": np.array([c[0] for c in CASES]), "gamma": np.float64(GAMMA), "max_flow": np.float64(MAX_FLOW),
           "tie_margin": np.float64(TIE_MARGIN), "epe_margin": np.float64(EPE_MARGIN)}
    for name, N, H, W, iters, seed in CASES:
        flows, masks, gt0, valid, cot = case_inputs(N, H, W, iters, seed)
        gt = fix_flow_gt(gt0, predictions(RAFT, flows, masks, torch.float64), seed)
        moved = np.flatnonzero(gt.reshape(-1) != gt0.reshape(-1))
        assert np.array_equal(apply_fixes(gt0, moved, gt.reshape(-1)[moved]), gt)
        r32 = run_case(RAFT, train, flows, masks, gt, valid, cot, torch.float32)
        r64 = run_case(RAFT, train, flows, masks, gt, valid, cot, torch.float64)
        assert np.array_equal(r32["acc"][1:], r64["acc"][1:]), "fp32 and fp64 runs disagree on a count: %s %s" % (r32["acc"], r64["acc"])
        nv = r64["acc"][4]
        assert (r64["acc"][1:4] > 0).all() and r64["acc"][1] < r64["acc"][2] < r64["acc"][3] < nv
        assert np.allclose(r64["metrics"], [r64["acc"][0] / nv, r64["acc"][1] / nv, r64["acc"][2] / nv, r64["acc"][3] / nv], rtol=1e-6, atol=0)
        p = name + "/"
        rec[p + "settings"] = np.array([N, H, W, iters, seed], np.int64)
        rec[p + "gt_fix_idx"] = moved.astype(np.int64)
        rec[p + "gt_fix_val"] = gt.reshape(-1)[moved].astype(np.float32)
        rec[p + "input_sums"] = np.array([sum(f.astype(np.float64).sum() for f in flows), sum(m.astype(np.float64).sum() for m in masks),
                                          gt.astype(np.float64).sum(), valid.astype(np.float64).sum(), cot.astype(np.float64).sum()])
        for key in ("loss", "terms", "metrics", "acc"):
            rec[p + key + "_f32"], rec[p + key + "_f64"] = np.asarray(r32[key], np.float64), np.asarray(r64[key], np.float64)
        big = [("pred_last", r32["pred_last"], r64["pred_last"]), ("up_grad_flow", r32["up_grad_flow"], r64["up_grad_flow"]),
               ("up_grad_mask", r32["up_grad_mask"], r64["up_grad_mask"])]
        for i in range(iters):
            big.append(("grad_flow_%d" % i, r32["grad_flow"][i], r64["grad_flow"][i]))
            big.append(("grad_mask_%d" % i, r32["grad_mask"][i], r64["grad_mask"][i]))
        for key, v32, v64 in big:
            idx = sample_index(v64.size, seed)
            rec[p + key + "_f32"] = v32.reshape(-1)[idx].astype(np.float32)
            rec[p + key + "_f64"] = v64.reshape(-1)[idx].astype(np.float64)
            rec[p + key + "_err32"] = np.float64(np.abs(v32.astype(np.float64) - v64).max())
            rec[p + key + "_absmax"] = np.float64(np.abs(v64).max())
        rel = np.abs(r32["terms"] - r64["terms"]) / np.abs(r64["terms"])
        print("%-16s moved %5d  loss %.6f  terms rel err32 %.1e..%.1e  err32 pred %.1e up_gf %.1e up_gm %.1e gf0 %.1e gm0 %.1e  acc %s" % (
            name, moved.size, r64["loss"], rel.min(), rel.max(), rec[p + "pred_last_err32"], rec[p + "up_grad_flow_err32"],
            rec[p + "up_grad_mask_err32"], rec[p + "grad_flow_0_err32"], rec[p + "grad_mask_0_err32"], r64["acc"].tolist()))
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 1 << 20
    return 0


if __name__ == "__main__":
    sys.exit(main())
