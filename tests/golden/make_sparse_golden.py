#!/usr/bin/env python3
"""Record RAFT's sparse augmentation (the KITTI stage's loader) by RUNNING THE REFERENCE ITSELF -> tests/golden/sparse_augment.npz.

    python tests/golden/make_sparse_golden.py [--out PATH]        (in the build container: needs the reference tree, numpy, torch)

It imports the reference's core/utils/augmentor.py (SparseFlowAugmentor) and core/utils/frame_utils.py (writeFlowKITTI / readFlowKITTI)
read-only, with stubs for what the container lacks:
  * cv2: `resize` returns zeros of cv2's dsize (rint(W*fx) x rint(H*fy)) and records fx / fy (the image arithmetic is not pinned here, only
    the sizes it hands on); `imwrite` / `imread` keep the array in memory (a 16-bit PNG is lossless); `setNumThreads`, `ocl.setUseOpenCL`.
  * torchvision.transforms.ColorJitter: inert (never called: only spatial_transform runs).
np.random.uniform / rand / randint are wrapped to log every draw.  Per case: np.random.seed(seed), then the flow through writeFlowKITTI ->
readFlowKITTI (cases with quantize=1; the others hand the float flow over as it is), a valid mask (all ones, or random: the flow is zeroed
where it is invalid, the repository's rule for invalid sources), then SparseFlowAugmentor.spatial_transform.  Recorded: the inputs (raw
flow before the code, mask), the settings, the logged draws, fx / fy, the resized frame size and the reference's output flow and valid.
tests/test_online_sparse.py replays the draws with online.sparse_augment_params and the outputs with its restatement of the kernel."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_harness import REFERENCE_ROOT  # noqa: E402

# (H, W, h, w, do_flip, min_scale, max_scale, spatial_aug_prob, mask: ones | random, quantize)
CASES = [
    (40, 64, 24, 40, False, -0.2, 0.4, 0.8, "ones", 1),
    (40, 64, 24, 40, True, -0.2, 0.4, 0.8, "ones", 1),
    (40, 64, 24, 40, True, -0.5, 0.7, 1.0, "random", 1),
    (40, 64, 24, 40, False, -0.5, -0.3, 1.0, "random", 1),
    (40, 64, 24, 40, True, 0.3, 0.7, 1.0, "ones", 1),
    (40, 64, 24, 40, True, -0.2, 0.4, 0.0, "random", 1),
    (61, 97, 33, 57, False, -0.2, 0.4, 0.8, "ones", 1),
    (61, 97, 33, 57, True, -0.2, 0.4, 0.8, "random", 1),
    (61, 97, 33, 57, True, -0.6, 0.6, 1.0, "random", 0),
    (61, 97, 33, 57, False, 0.2, 0.6, 1.0, "ones", 0),
    (61, 97, 33, 57, True, -0.6, -0.4, 1.0, "ones", 1),
    (61, 97, 33, 57, True, -0.2, 0.4, 1.0, "random", 1),
    (37, 53, 19, 31, True, -0.4, 0.5, 1.0, "random", 1),
    (37, 53, 19, 31, False, -0.4, 0.5, 1.0, "ones", 0),
    (37, 53, 37, 53, True, -0.2, 0.4, 0.0, "ones", 1),      # the crop equals the frame (no resize)
    (37, 53, 37, 53, False, -0.2, 0.4, 0.0, "random", 1),
    (29, 71, 20, 50, True, -0.3, 0.8, 1.0, "random", 1),
    (29, 71, 20, 50, True, -0.3, 0.8, 1.0, "ones", 1),
    (48, 48, 30, 30, True, 0.5, 0.9, 1.0, "random", 0),
    (48, 48, 30, 30, False, -0.7, -0.5, 1.0, "random", 1),
]


def install_stubs():
    rec = {"resize": [], "files": {}}
    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_ANYDEPTH, cv2.IMREAD_COLOR, cv2.INTER_LINEAR = 2, 1, 1
    cv2.setNumThreads = lambda n: None
    cv2.ocl = types.SimpleNamespace(setUseOpenCL=lambda on: None)

    def resize(img, dsize, fx=None, fy=None, interpolation=None):
        assert dsize is None
        rec["resize"].append((float(fx), float(fy)))
        H, W = img.shape[:2]
        return np.zeros((int(np.rint(H * fy)), int(np.rint(W * fx))) + img.shape[2:], img.dtype)

    def imwrite(name, a):
        assert a.dtype == np.uint16
        rec["files"][name] = np.array(a)
        return True

    cv2.resize, cv2.imwrite = resize, imwrite
    cv2.imread = lambda name, flags=None: np.array(rec["files"][name])
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")

    class ColorJitter:
        def __init__(self, *a, **k):
            pass

        def __call__(self, img):
            raise AssertionError("ColorJitter is not on the recorded path")
    tvt.ColorJitter = ColorJitter
    tv.transforms = tvt
    sys.modules.update({"cv2": cv2, "torchvision": tv, "torchvision.transforms": tvt})
    return rec


def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REFERENCE_ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class DrawLog:
    """np.random.uniform / rand / randint wrapped: (kind 0 / 1 / 2, low, high, value) per draw."""

    def __init__(self):
        self.log = []
        self.orig = (np.random.uniform, np.random.rand, np.random.randint)

    def __enter__(self):
        u, r, ri = self.orig

        def uniform(lo=0.0, hi=1.0, size=None):
            v = u(lo, hi, size)
            self.log.append((0, lo, hi, float(v)))
            return v

        def rand(*a):
            v = r(*a)
            self.log.append((1, 0, 1, float(v)))
            return v

        def randint(lo, hi=None, size=None):
            v = ri(lo, hi, size)
            self.log.append((2, lo, hi, float(v)))
            return v
        np.random.uniform, np.random.rand, np.random.randint = uniform, rand, randint
        return self

    def __exit__(self, *exc):
        np.random.uniform, np.random.rand, np.random.randint = self.orig
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "sparse_augment.npz"))
    a = ap.parse_args()
    rec = install_stubs()
    aug = load("ref_augmentor", os.path.join("core", "utils", "augmentor.py"))
    fu = load("ref_frame_utils", os.path.join("core", "utils", "frame_utils.py"))
    out = {"numpy_version": np.array(np.__version__), "n_cases": np.int64(len(CASES))}
    for i, (H, W, h, w, do_flip, lo, hi, prob, mask, quantize) in enumerate(CASES):
        seed = 7000 + i
        inp = np.random.RandomState(seed + 500)
        flow = (np.round((inp.rand(H, W, 2) - 0.5) * 1000 * 256) / 256).astype(np.float32)     # |u| < 500: inside the 16-bit code's range;
        flow[::3, ::5] = np.round(flow[::3, ::5] * 64) / 64                     # a 1/256 grid (compresses), some values on the code's own
        valid_in = np.ones((H, W), np.uint8) if mask == "ones" else (inp.rand(H, W) < 0.6).astype(np.uint8)
        if quantize:
            fu.writeFlowKITTI("flow_%d.png" % i, flow)
            fq, vq = fu.readFlowKITTI("flow_%d.png" % i)
            assert (vq == 1).all()
        else:
            fq = flow.copy()
        fq = np.where(valid_in[..., None] != 0, fq, 0).astype(np.float32)
        sa = aug.SparseFlowAugmentor((h, w), min_scale=lo, max_scale=hi, do_flip=do_flip)
        sa.spatial_aug_prob = prob
        img = np.zeros((H, W, 3), np.uint8)
        rec["resize"].clear()
        np.random.seed(seed)
        with DrawLog() as log:
            _, _, f_out, v_out = sa.spatial_transform(img, img.copy(), fq, valid_in.astype(np.float32))
        fx, fy = rec["resize"][0] if rec["resize"] else (np.nan, np.nan)
        p = "c%02d_" % i
        out.update({p + "settings": np.array([H, W, h, w, int(do_flip), lo, hi, prob, quantize, seed], np.float64),
                    p + "flow_in": flow, p + "valid_in": valid_in, p + "draws": np.array(log.log, np.float64),
                    p + "fxfy": np.array([fx, fy], np.float64), p + "flow": np.ascontiguousarray(f_out, np.float32),
                    p + "valid": np.ascontiguousarray(v_out, np.float32)})
        print("case %2d: %dx%d -> %dx%d  fx %.4f  flip %s  draws %d  valid %.2f" % (i, H, W, h, w, fx, do_flip, len(log.log), v_out.mean()))
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
