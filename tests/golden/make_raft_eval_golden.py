#!/usr/bin/env python3
"""Record RAFT's evaluation path on frames whose sides are no multiples of 8 by RUNNING THE REFERENCE ITSELF (RAFT/core/raft.py and
RAFT/core/utils/utils.py's InputPadder, CPU) -> tests/golden/raft_eval.npz.

    python tests/golden/make_raft_eval_golden.py [--out PATH]   (in the build container: needs the reference tree, numpy, torch)

The recorded expression is evaluate.py's:

    padder = InputPadder(image1.shape, mode)
    flow_low, flow_pr = model(*padder.pad(image1, image2), iters=12, test_mode=True)
    flow_up = padder.unpad(flow_pr)

Built like make_raft_golden.py, whose case_inputs(), fill_params(), sample_index() and load_reference() it imports: per case the reference runs
in fp32 and in double (torch.Tensor.float neutralised for the double run, as there); per array (flow_low, flow_up) the file keeps N_SAMPLE
entries of the double run at the flat indices of sample_index(), err32 = max |fp32 run - double run| over the WHOLE array and max |ref64|.
Images and weights are draws of np.random.RandomState(seed), rebuilt by the test; the file carries their float64 sums and the padder's _pad.

Cases (CASES): both models, both modes, sides that leave every pad split the arithmetic has: 121 -> 7 (3 + 4, or 0 + 7), 123 -> 5, 127 -> 1
(0 + 1), 129 -> 7, 130 -> 6 (3 + 3), 131 -> 5 (2 + 3).  Every padded frame is 128 x 136, the smallest the reference can run.

The recorder asserts: no NaN; err32 > 0 and err32 <= 1e-3 * absmax for every array; final |flow| absmax >= 1 px."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_raft_golden import case_inputs, fill_params, load_reference, make_args, sample_index      # noqa: E402

ITERS = 12

# (name, small, N, H, W, mode, seed)
CASES = [("basic/sintel_1x121x131", False, 1, 121, 131, "sintel", 9900), ("basic/kitti_1x123x130", False, 1, 123, 130, "kitti", 9910),
         ("small/kitti_1x121x131", True, 1, 121, 131, "kitti", 9920), ("small/sintel_1x127x129", True, 1, 127, 129, "sintel", 9930)]


def eval_inputs(N, H, W, seed):
    """image1, image2 of make_raft_golden.case_inputs (integers 0..255, image2 a rolled image1); its flow_init is not used here"""
    d = case_inputs(N, H, W, ITERS, False, seed)
    return dict(image1=d["image1"], image2=d["image2"])


def run_case(ref, padder_cls, small, mode, d, seed, dtype):
    model = ref.RAFT(make_args(small))
    fill_params(model, seed)
    model = model.to(dtype)
    model.freeze_bn()
    model.eval()
    t = lambda a: torch.from_numpy(a).to(dtype)
    keep = torch.Tensor.float
    if dtype == torch.float64:                               # the reference's own casts to fp32; restored below
        torch.Tensor.float = lambda self: self if self.is_floating_point() else self.double()
    try:
        with torch.no_grad():
            padder = padder_cls(d["image1"].shape, mode)
            flow_low, flow_pr = model(*padder.pad(t(d["image1"]), t(d["image2"])), iters=ITERS, test_mode=True)
            flow_up = padder.unpad(flow_pr)
    finally:
        torch.Tensor.float = keep
    res = dict(flow_low=flow_low.numpy(), flow_up=flow_up.contiguous().numpy())
    for key, v in res.items():
        assert v.dtype == (np.float64 if dtype == torch.float64 else np.float32), (key, v.dtype)
        assert np.isfinite(v).all(), key
    return res, [int(p) for p in padder._pad]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "raft_eval.npz"))
    a = ap.parse_args()
    ref = load_reference()
    from utils.utils import InputPadder                      # the reference's own: load_reference() put RAFT/core on sys.path
    torch.manual_seed(0)
    rec = {"numpy_version": np.array(np.__version__), "torch_version": np.array(torch.__version__), "names": np.array([c[0] for c in CASES])}
    for name, small, N, H, W, mode, seed in CASES:
        d = eval_inputs(N, H, W, seed)
        r32, pad = run_case(ref, InputPadder, small, mode, d, seed, torch.float32)
        r64, pad64 = run_case(ref, InputPadder, small, mode, d, seed, torch.float64)
        assert pad == pad64
        p = name + "/"
        rec[p + "settings"] = np.array([int(small), N, H, W, ITERS, int(mode != "sintel"), seed], np.int64)
        rec[p + "pad"] = np.array(pad, np.int64)
        rec[p + "input_sums"] = np.array([sum(v.astype(np.float64).sum() for v in d.values()), fill_params(ref.RAFT(make_args(small)), seed)])
        Hp, Wp = H + pad[2] + pad[3], W + pad[0] + pad[1]
        assert r64["flow_low"].shape == (N, 2, Hp // 8, Wp // 8) and r64["flow_up"].shape == (N, 2, H, W) and Hp % 8 == 0 and Wp % 8 == 0
        for key in ("flow_low", "flow_up"):
            v32, v64 = r32[key], r64[key]
            err, absmax = float(np.abs(v32.astype(np.float64) - v64).max()), float(np.abs(v64).max())
            assert 0.0 < err <= 1e-3 * absmax, (name, key, err, absmax)
            rec[p + key + "_f64"] = v64.reshape(-1)[sample_index(v64.size, seed)]
            rec[p + key + "_err32"] = np.float64(err)
            rec[p + key + "_absmax"] = np.float64(absmax)
        assert rec[p + "flow_up_absmax"] >= 1.0, (name, rec[p + "flow_up_absmax"])
        print("%-24s %s pad %s -> %d x %d; |flow_up| absmax %.2f px; err32 flow_low %.2e, flow_up %.2e"
              % (name, mode, pad, Hp, Wp, rec[p + "flow_up_absmax"], rec[p + "flow_low_err32"], rec[p + "flow_up_err32"]))
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < os.path.getsize(os.path.join(HERE, "raft_model.npz"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
