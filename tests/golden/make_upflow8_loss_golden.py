#!/usr/bin/env python3
"""Record the small RAFT model's loss by RUNNING THE REFERENCE ITSELF (upflow8 of RAFT/core/utils/utils.py followed by sequence_loss of
RAFT/train.py, CPU) -> tests/golden/raft_upflow8_loss.npz.

    python tests/golden/make_upflow8_loss_golden.py [--out PATH]        (in the build container: needs the reference tree, numpy, torch)

In the style of make_upsample_golden.py, whose load_reference, fix_flow_gt, apply_fixes, sample_index and accumulators are used as they are.
Per case, in fp32 and on .double() inputs: sequence_loss over all iterations' predictions (loss and metrics) and over each one alone with
gamma = 1 (the per-iteration terms), the five metric accumulators of the last prediction, and the gradient of the loss for every iteration's
coarse flow.  In full: loss, terms, metrics, accumulators.  Of each grad_flow N_SAMPLE entries at sample_index()'s flat indices, fp32 and
float64, plus err32 = max |fp32 run - double run| over the WHOLE array and max |ref64|.

Inputs are draws of np.random.RandomState(seed), rebuilt by case_inputs(); the file carries their float64 sums.  flow_gt is then moved by
fix_flow_gt() until, on the double run, every |pred64 - flow_gt| >= TIE_MARGIN in every iteration, | |flow_gt| - max_flow | >= 1 and the last
prediction's epe is EPE_MARGIN clear of 1, 3 and 5; the file stores the moved entries for apply_fixes().  tests/test_raft_upflow8_loss.py
re-asserts the conditions from its own float64 restatement: no entry is left out of any comparison."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_upsample_golden import (EPE_MARGIN, GAMMA, MAX_FLOW, N_SAMPLE, TIE_MARGIN, accumulators, apply_fixes, fix_flow_gt,  # noqa: E402
                                  load_reference, sample_index)

# (name, N, H, W, iterations, seed): both degenerate axes, a width that is no multiple of 4, a map that does not fill a block, one frame at
# the OnlinePairs crop
CASES = [
    ("one_1x1x1", 1, 1, 1, 2, 9300),
    ("h1_2x1x9", 2, 1, 9, 2, 9310),
    ("w1_2x5x1", 2, 5, 1, 2, 9320),
    ("tiny_1x5x7", 1, 5, 7, 3, 9330),
    ("mid_1x13x83", 1, 13, 83, 3, 9340),
    ("real_2x36x120", 2, 36, 120, 4, 9350),
]


def case_inputs(N, H, W, iters, seed):
    """(flows, flow_gt, valid) of a case, float32: flows is a list over the iterations; flow_gt BEFORE apply_fixes()"""
    rs = np.random.RandomState(seed)
    target = rs.standard_normal((N, 2, H, W)) * 3.0                              # coarse flows drift towards a field of a few coarse pixels
    flows = [(target * (k + 1) / iters + 0.5 * rs.standard_normal((N, 2, H, W))).astype(np.float32) for k in range(iters)]
    flow_gt = (30.0 * rs.standard_normal((N, 2, 8 * H, 8 * W))).astype(np.float32)
    far = rs.rand(N, 8 * H, 8 * W) < 0.02                                         # beyond max_flow on purpose, at least one pixel
    far.reshape(-1)[rs.randint(far.size)] = True
    for c in range(2):
        flow_gt[:, c][far] = (np.where(rs.rand(int(far.sum())) < 0.5, -1.0, 1.0) * (300.0 + 20.0 * rs.rand(int(far.sum())))).astype(np.float32)
    valid = (rs.rand(N, 8 * H, 8 * W) > 0.1).astype(np.float32)
    return flows, flow_gt, valid


def run_case(upflow8, train, flows, gt, valid, dtype):
    t = lambda a: torch.from_numpy(a).to(dtype)
    fl = [t(f).requires_grad_(True) for f in flows]
    preds = [upflow8(f) for f in fl]
    assert preds[0].dtype == dtype and preds[0].shape == gt.shape
    loss, metrics = train.sequence_loss(preds, t(gt), t(valid), gamma=GAMMA, max_flow=MAX_FLOW)
    loss.backward()
    res = dict(loss=np.float64(loss.item()), metrics=np.array([metrics[k] for k in ("epe", "1px", "3px", "5px")], np.float64),
               grad_flow=[f.grad.numpy() for f in fl], pred_last=preds[-1].detach().numpy())
    with torch.no_grad():
        res["terms"] = np.array([train.sequence_loss([p.detach()], t(gt), t(valid), gamma=1.0, max_flow=MAX_FLOW)[0].item() for p in preds], np.float64)
    res["acc"] = accumulators(res["pred_last"], gt, valid, np.float32 if dtype == torch.float32 else np.float64)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "raft_upflow8_loss.npz"))
    a = ap.parse_args()
    RAFT, train = load_reference()
    upflow8 = sys.modules[RAFT.__module__].upflow8                               # RAFT/core/utils/utils.py's, as raft.py imports it
    assert upflow8.__module__ == "utils.utils"
    torch.manual_seed(0)
    rec = {"numpy_version": np.array(np.__version__), "torch_version": np.array(torch.__version__), "n_sample": np.int64(N_SAMPLE),
           "names": np.array([c[0] for c in CASES]), "gamma": np.float64(GAMMA), "max_flow": np.float64(MAX_FLOW),
           "tie_margin": np.float64(TIE_MARGIN), "epe_margin": np.float64(EPE_MARGIN)}
    for name, N, H, W, iters, seed in CASES:
        flows, gt0, valid = case_inputs(N, H, W, iters, seed)
        with torch.no_grad():
            preds64 = [upflow8(torch.from_numpy(f).double()).numpy() for f in flows]
        gt = fix_flow_gt(gt0, preds64, seed)
        moved = np.flatnonzero(gt.reshape(-1) != gt0.reshape(-1))
        assert np.array_equal(apply_fixes(gt0, moved, gt.reshape(-1)[moved]), gt)
        r32 = run_case(upflow8, train, flows, gt, valid, torch.float32)
        r64 = run_case(upflow8, train, flows, gt, valid, torch.float64)
        assert np.array_equal(r32["acc"][1:], r64["acc"][1:]), "fp32 and fp64 runs disagree on a count: %s %s" % (r32["acc"], r64["acc"])
        nv = r64["acc"][4]
        assert (r64["acc"][1:4] > 0).all() and r64["acc"][1] < r64["acc"][2] < r64["acc"][3] < nv
        assert np.allclose(r64["metrics"], [r64["acc"][0] / nv, r64["acc"][1] / nv, r64["acc"][2] / nv, r64["acc"][3] / nv], rtol=1e-6, atol=0)
        p = name + "/"
        rec[p + "settings"] = np.array([N, H, W, iters, seed], np.int64)
        rec[p + "gt_fix_idx"] = moved.astype(np.int64)
        rec[p + "gt_fix_val"] = gt.reshape(-1)[moved].astype(np.float32)
        rec[p + "input_sums"] = np.array([sum(f.astype(np.float64).sum() for f in flows), gt.astype(np.float64).sum(), valid.astype(np.float64).sum()])
        for key in ("loss", "terms", "metrics", "acc"):
            rec[p + key + "_f32"], rec[p + key + "_f64"] = np.asarray(r32[key], np.float64), np.asarray(r64[key], np.float64)
        for i in range(iters):
            key, v32, v64 = "grad_flow_%d" % i, r32["grad_flow"][i], r64["grad_flow"][i]
            idx = sample_index(v64.size, seed)
            rec[p + key + "_f32"] = v32.reshape(-1)[idx].astype(np.float32)
            rec[p + key + "_f64"] = v64.reshape(-1)[idx].astype(np.float64)
            rec[p + key + "_err32"] = np.float64(np.abs(v32.astype(np.float64) - v64).max())
            rec[p + key + "_absmax"] = np.float64(np.abs(v64).max())
        rel = np.abs(r32["terms"] - r64["terms"]) / np.abs(r64["terms"])
        print("%-16s moved %5d  loss %.6f  terms rel err32 %.1e..%.1e  err32 gf0 %.1e (absmax %.1e)  acc %s" % (
            name, moved.size, r64["loss"], rel.min(), rel.max(), rec[p + "grad_flow_0_err32"], rec[p + "grad_flow_0_absmax"], r64["acc"].tolist()))
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 1 << 20
    return 0


if __name__ == "__main__":
    sys.exit(main())
