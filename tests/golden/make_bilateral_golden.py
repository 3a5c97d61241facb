#!/usr/bin/env python3
"""Record the sparse bilateral filter by RUNNING THE REFERENCE ITSELF (bilateral_filter.py: numpy only) on the CPU -> tests/golden/bilateral.npz.

    python tests/golden/make_bilateral_golden.py [--out-dir DIR]   (in the build container: needs the reference tree and numpy)

The file holds inputs and the reference's outputs only.  Inputs are stored once per shape and dtype (in_f64_<shape>, in_f32_<shape>,
in_u8_<shape>, mask_<shape>: float32 0 / 1), outputs per case: out_<dtype>_<shape>_w<windows>[_mask].  The uint8 call site is the reference fed
u8 / 255 in float64 (cv2.imread(path, 0) / 255); its output is stored as bytes after the recorder has checked that bytes / 255.0 gives the
reference's float64 output back bit for bit.  tests/bilateral_restated.py names the pattern (blocky) and the masks.

The recorder asserts what makes the cases worth keeping: every case of the grid changes between 20 % and 97 % of its pixels, and over the set
at least one pixel selects among n samples with k*(n) != n // 2 + 1 AND would get another value under n // 2 + 1."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import bilateral_restated as R  # noqa: E402

SHAPES = ((23, 29), (9, 40))
WINDOWS = ((3,), (5, 5), (7, 5, 3), (9,))


def inputs(h, w):
    """the three inputs of a shape: float64 (levels over 251, so no byte holds them), float32, uint8"""
    u8 = R.blocky(1000 + h, h, w)
    return {"f64": u8.astype(np.float64) / 251.0, "f32": (u8.astype(np.float64) / 255.0).astype(np.float32), "u8": u8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=HERE)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import ref_harness
    ref_harness.install()
    import bilateral_filter as ref              # the reference's own

    def run(x, ws, mask=None):
        x = x.astype(np.float64) / 255 if x.dtype == np.uint8 else x
        return ref.sparse_bilateral_filtering(x.copy(), filter_size=list(ws), mask=None if mask is None else mask.copy(), num_iter=len(ws))

    def put(name, y, src):
        if src.dtype == np.uint8:
            b = np.rint(y * 255.0).astype(np.uint8)
            assert y.dtype == np.float64 and (b.astype(np.float64) / 255.0 == y).all(), name
            y = b
        assert y.dtype == src.dtype and y.shape == src.shape, name
        rec[name] = y
        return float((y != src).mean())

    rec, tricky = {"numpy_version": np.array(np.__version__)}, 0
    for h, w in SHAPES:
        shape = "%dx%d" % (h, w)
        ins = inputs(h, w)
        mask = R.random_mask(2000 + h, h, w)
        rec["mask_" + shape] = mask
        for dt, x in ins.items():
            rec["in_%s_%s" % (dt, shape)] = x
            for ws in WINDOWS:
                for mk in (None, mask):
                    name = "out_%s_%s_w%s%s" % (dt, shape, "".join(map(str, ws)), "" if mk is None else "_mask")
                    changed = put(name, run(x, ws, mk), x)
                    print("%-32s changed %.3f" % (name, changed))
                    assert 0.20 <= changed <= 0.97, (name, changed)
                    # the first iteration under k* and under n // 2 + 1: pixels whose n is one of the odd ones out and whose value shows it
                    xf = x.astype(np.float64) / 255 if x.dtype == np.uint8 else x
                    D = R.discontinuity_map(xf, xf, 0.04, mk)
                    good, n = R.select(xf, D, ws[0], mk, with_n=True)
                    naive = R.select(xf, D, ws[0], mk, rank=lambda i: i // 2 + 1)
                    odd = np.isin(n, [i for i in range(1, 82) if R.kstar(i) != i // 2 + 1])
                    assert ((good != naive) <= odd).all()
                    tricky += int((good != naive).sum())
    # one smooth ramp with no discontinuity: only the ring rule acts
    ramp = (0.3 + 0.002 * np.arange(11)[:, None] + 0.001 * np.arange(13)[None, :]).astype(np.float64)
    assert not R.discontinuity_map(ramp, ramp, 0.04).any()
    rec["in_ramp"] = ramp
    put("out_ramp_w5", run(ramp, (5,)), ramp)
    assert (rec["out_ramp_w5"][1:-1, 1:-1] == ramp[1:-1, 1:-1]).all() and (rec["out_ramp_w5"] != ramp).any()
    # 5 x 7 under window 9: every window is mostly padding
    small = R.blocky(7, 5, 7).astype(np.float64) / 255.0
    rec["in_small"] = small
    print("small changed %.3f" % put("out_small_w9", run(small, (9,)), small))
    # an all-zero block: 1 / 0 = inf, inf - inf = NaN
    zb = R.blocky(11, 16, 18)
    zb[4:11, 5:13] = 0
    rec["in_zeroblock"] = zb
    print("zeroblock changed %.3f" % put("out_zeroblock_w55", run(zb, (5, 5)), zb))
    print("pixels whose value shows k*(n) != n // 2 + 1: %d" % tricky)
    assert tricky >= 1
    out = os.path.join(a.out_dir, "bilateral.npz")
    np.savez_compressed(out, **rec)
    print("wrote %s, %d bytes, %d arrays" % (out, os.path.getsize(out), len(rec)))
    assert os.path.getsize(out) < 200 * 1000
    return 0


if __name__ == "__main__":
    sys.exit(main())
