#!/usr/bin/env python3
"""Record AdaMPI's plane-adjustment network by RUNNING THE REFERENCE ITSELF (model/PAN.py, model/AdaMPI.py; CPU) -> tests/golden/pan.npz.

    python tests/golden/make_pan_golden.py [--out PATH]        (in the build container: needs the reference tree, numpy, torch)

The reference's DepthPredictionNetwork and MPIPredictor are imported through ref_harness.py; none of their text is copied.  Parameters AND BatchNorm
statistics are draws of np.random.RandomState(seed), rebuilt by fill_params() on the reference's modules and on this repository's alike (same
state_dict); inputs likewise (case_inputs()).  The file keeps seeds and the float64 sums of what was drawn, not the draws.  Everything runs in eval
mode, once in float32 and once in float64.

Per case of CASES (low-resolution size h x w: 32 x 32 is the smallest that survives five halvings, 33 x 47 is odd - the pool drops a row and a
column at several levels -, 40 x 72; S in 1, 5, 64; B in 1, 2):
    <case>/block1_f64      the first residual block's output after its 2 x 2 average pool [B*S,8,h//2,w//2] in float64: the whole array where it has
                           at most FULL_MAX entries, else its entries at sample_index() (flat indices)
    <case>/block1_e_ref    max |float32 run - float64 run| / max |float64 run| over the WHOLE array;  <case>/block1_absmax  that maximum
    <case>/dpn_f32, dpn_f64, dpn_e_ref      the network's output [B,S] (the adjusted planes), likewise
    <case>/settings, input_sum
The case MODEL runs the reference's MPIPredictor modules the way its commented line would (model/AdaMPI.py:60-72): low-resolution inputs by
bilinear interpolation with align_corners=True, render_disp = dpn(fixed planes, ...), fmn(image, disparity, render_disp):
    model/planes_f32, planes_f64, planes_e_ref      the adjusted planes [1,S]
    model/fmn_f32          the feature mask on the adjusted planes (float32 run), its entries at sample_index()
The initial planes of the other cases are the fixed planes plus a per-image jitter, so that a batch entry read from the wrong row shows."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

FULL_MAX = 16384
N_SAMPLE = 4096
# name: (B, S, h, w, seed)
CASES = {"b1_s1_32x32": (1, 1, 32, 32, 9900), "b1_s5_33x47": (1, 5, 33, 47, 9901), "b2_s1_40x72": (2, 1, 40, 72, 9902), "b2_s5_33x47": (2, 5, 33, 47, 9903),
         "b1_s64_32x32": (1, 64, 32, 32, 9904), "b2_s64_40x72": (2, 64, 40, 72, 9905), "b1_s64_33x47": (1, 64, 33, 47, 9906)}
MODEL = dict(S=5, H=128, W=128, seed=9910)          # low-resolution size 32 x 32


def fixed_planes(S):
    return torch.linspace(1, 0.001, S + 2)[1:-1]


def case_inputs(B, S, h, w, seed):
    """float32 arrays: rgb_low [B,3,h,w], disp_low [B,1,h,w] in [0, 1); init_disp [B,S]: the fixed planes + 0.01 N(0,1)"""
    rs = np.random.RandomState(seed)
    d = dict(rgb_low=rs.rand(B, 3, h, w).astype(np.float32), disp_low=rs.rand(B, 1, h, w).astype(np.float32))
    d["init_disp"] = (fixed_planes(S).numpy()[None] + 0.01 * rs.standard_normal((B, S))).astype(np.float32)
    return d


def model_inputs():
    rs = np.random.RandomState(MODEL["seed"])
    return dict(image=rs.rand(1, 3, MODEL["H"], MODEL["W"]).astype(np.float32), disp=rs.rand(1, 1, MODEL["H"], MODEL["W"]).astype(np.float32))


def fill_params(module, seed):
    """Every entry of `module`'s state_dict from RandomState draws, in state_dict order: weights of two or more dimensions N(0,1) / sqrt(fan_in) -
    twice that for convolutions, which a ReLU follows -, norm weights 1 + 0.1 N(0,1), biases and running means 0.1 N(0,1), running variances
    0.5 + |N(0,1)|; num_batches_tracked stays.  Returns the float64 sum of what was drawn."""
    rs = np.random.RandomState(seed + 7)
    total = 0.0
    with torch.no_grad():
        for name, p in module.state_dict().items():
            shape = tuple(p.shape)
            if name.endswith("num_batches_tracked"):
                continue
            if name.endswith(".weight") and len(shape) > 1:
                v = rs.standard_normal(shape) * ((2.0 if len(shape) == 4 else 1.0) / np.sqrt(np.prod(shape[1:])))
            elif name.endswith(".weight"):
                v = 1.0 + 0.1 * rs.standard_normal(shape)
            elif name.endswith("running_var"):
                v = 0.5 + np.abs(rs.standard_normal(shape))
            else:
                v = 0.1 * rs.standard_normal(shape)
            v = v.astype(np.float32)
            total += float(v.astype(np.float64).sum())
            p.copy_(torch.from_numpy(v).to(p.dtype))
    return total


def sample_index(n, seed):
    return np.random.RandomState(seed + 1).randint(0, n, N_SAMPLE)


def kept(a, seed):
    """what the file keeps of an array: the whole of a small one, the entries at sample_index() of a large one (flat)"""
    flat = np.ascontiguousarray(a).reshape(-1)
    return flat if flat.size <= FULL_MAX else flat[sample_index(flat.size, seed)]


def e_ref(v32, v64):
    return float(np.abs(v32.astype(np.float64) - v64).max() / np.abs(v64).max())


def run_dpn(dpn, d, dtype):
    """the reference network on a case in `dtype` -> (block 1 after its pool, the network's output), numpy"""
    dpn = dpn.to(dtype).eval()
    cap = {}
    hook = dpn.context_encoder.res_blocks[0].register_forward_hook(lambda mod, inp, out: cap.__setitem__("block1", F.avg_pool2d(out, kernel_size=2)))
    with torch.no_grad():
        out = dpn(*(torch.from_numpy(d[k]).to(dtype) for k in ("init_disp", "rgb_low", "disp_low")))
    hook.remove()
    return cap["block1"].numpy(), out.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "pan.npz"))
    a = ap.parse_args()
    import ref_harness
    ref_harness.install()
    from model.AdaMPI import MPIPredictor
    from model.PAN import DepthPredictionNetwork
    torch.manual_seed(0)
    rec = {"numpy_version": np.array(np.__version__), "torch_version": np.array(torch.__version__), "names": np.array(list(CASES)),
           "full_max": np.int64(FULL_MAX), "n_sample": np.int64(N_SAMPLE)}
    for name, (B, S, h, w, seed) in CASES.items():
        d = case_inputs(B, S, h, w, seed)
        res = {}
        for dtype in (torch.float32, torch.float64):
            dpn = DepthPredictionNetwork(disp_range=[0.001, 1], n_planes=S)
            psum = fill_params(dpn, seed)
            res[dtype] = run_dpn(dpn, d, dtype)
        (b32, o32), (b64, o64) = res[torch.float32], res[torch.float64]
        assert b32.dtype == np.float32 and b64.dtype == np.float64 and b64.shape == (B * S, 8, h // 2, w // 2) and o64.shape == (B, S)
        p = name + "/"
        rec[p + "settings"] = np.array([B, S, h, w, seed], np.int64)
        rec[p + "input_sum"] = np.float64(sum(v.astype(np.float64).sum() for v in d.values()) + psum)
        rec[p + "block1_f64"], rec[p + "block1_e_ref"], rec[p + "block1_absmax"] = kept(b64, seed), np.float64(e_ref(b32, b64)), np.float64(np.abs(b64).max())
        rec[p + "dpn_f32"], rec[p + "dpn_f64"], rec[p + "dpn_e_ref"] = o32, o64, np.float64(e_ref(o32, o64))
        assert 0 < rec[p + "block1_e_ref"] < 1e-5 and 0 < rec[p + "dpn_e_ref"] < 1e-4 and (b64 > 0).mean() > 0.2
        assert np.abs(o64 - d["init_disp"]).max() > 1e-4, "the network does not move the planes"
        print("%-14s block1 absmax %.2f e_ref %.2e (%d of %d entries kept); dpn e_ref %.2e, moves the planes by up to %.3f" % (
            name, rec[p + "block1_absmax"], rec[p + "block1_e_ref"], rec[p + "block1_f64"].size, b64.size, rec[p + "dpn_e_ref"],
            np.abs(o64 - d["init_disp"]).max()))
    # the whole predictor with the commented line of its forward switched on
    d = model_inputs()
    res = {}
    for dtype in (torch.float32, torch.float64):
        m = MPIPredictor(width=MODEL["W"], height=MODEL["H"], num_planes=MODEL["S"])
        psum = fill_params(m, MODEL["seed"])
        m = m.to(dtype).eval()
        img, dsp = torch.from_numpy(d["image"]).to(dtype), torch.from_numpy(d["disp"]).to(dtype)
        with torch.no_grad():
            rgb_low = F.interpolate(img, size=m.low_res_size, mode="bilinear", align_corners=True)
            disp_low = F.interpolate(dsp, size=m.low_res_size, mode="bilinear", align_corners=True)
            planes = m.dpn(fixed_planes(MODEL["S"]).to(dtype).unsqueeze(0), rgb_low, disp_low)
            res[dtype] = (planes.numpy(), m.fmn(img, dsp, planes).numpy())
    (p32, f32), (p64, f64) = res[torch.float32], res[torch.float64]
    rec["model/settings"] = np.array([MODEL["S"], MODEL["H"], MODEL["W"], MODEL["seed"]], np.int64)
    rec["model/input_sum"] = np.float64(sum(v.astype(np.float64).sum() for v in d.values()) + psum)
    rec["model/planes_f32"], rec["model/planes_f64"], rec["model/planes_e_ref"] = p32, p64, np.float64(e_ref(p32, p64))
    rec["model/fmn_f32"] = kept(f32, MODEL["seed"])
    assert f32.shape == (1, MODEL["S"], MODEL["H"], MODEL["W"]) and 0 < rec["model/planes_e_ref"] < 1e-4 and np.abs(f32.astype(np.float64) - f64).max() < 1e-4
    print("model          planes %s (e_ref %.2e); fmn |f32 - f64| %.2e" % (np.round(p64[0], 4), rec["model/planes_e_ref"], np.abs(f32 - f64).max()))
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 1 << 20
    return 0


if __name__ == "__main__":
    sys.exit(main())
