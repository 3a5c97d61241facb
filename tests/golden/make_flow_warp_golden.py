#!/usr/bin/env python3
"""Record the backward warps by a flow field by RUNNING THE REFERENCE ITSELF (utils/transform.py:60-111, warp and warp_rife, torch on the CPU; and
its numpy gen_random_perspective / get_flow) -> tests/golden/flow_warp.npz.

    python tests/golden/make_flow_warp_golden.py [--out PATH]   (needs the reference tree, numpy, torch)

The reference module is imported with cv2 stubbed (ref_harness), .cuda() the identity and, should it not import, utils.flow_viz stubbed.  warp()
cannot run in float64 as written (its tensor of ones is float32: "expected scalar type Float but found Double"), so the float64 runs of both
functions are made under torch.set_default_dtype(torch.float64); warp_rife's grid cache is emptied between the runs (it is keyed by size alone).

Per shape the file holds the inputs x, flow and the upstream gradient g (shared by the two functions), and per function ("warp/", "rife/"):
  ref32/out, ref32/mask (warp), ref32/grad_x, ref32/grad_flow     the reference's float32 run
  d64/...                                                          float32(float64 run - float32 run): the float64 value is ref32 + d64, exact to
                                                                   ~1e-14 of the value (tests/flow_warp_restated.py: golden_f64); stored this way
                                                                   because four more float64 tensors per case would not fit the size limit
  e_ref/...                                                        max|ref32 - f64| / max|f64| per tensor
plus rife/zero_flow (an all-zero flow: output only), and get_flow/... (seeded gen_random_perspective matrices and get_flow's bytes).

Conditions on the flows, asserted here (grad_flow jumps where a coordinate crosses an integer; nothing is excluded from any comparison):
  every sample coordinate of the float32 run, for both functions, lies at least 1e-3 px from an integer, and for warp_rife its unclamped
  coordinate at least 1e-3 px from the clamp bounds 0 and n - 1; flows are redrawn at offending pixels until none is left;
  the float32 and the float64 run take the same cells and the same side of the clamp;
  tests/flow_warp_restated.py equals the reference's float64 run to 1e-9 on every tensor."""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import flow_warp_restated as rs  # noqa: E402

# name -> B, C, H, W: less than a wave; the plain case; odd sizes, more than one block; the channel split over grid.z (64 + 6 channels)
CASES = {"b1_c1_5x7": (1, 1, 5, 7), "b2_c3_24x40": (2, 3, 24, 40), "b3_c2_33x65": (3, 2, 33, 65), "b1_c70_9x11": (1, 70, 9, 11)}
MODES = {"warp": rs.WARP, "rife": rs.RIFE}
ZERO_FLOW_SHAPE = (2, 3, 6, 9)
GET_FLOW_SHAPES = ((9, 13, 3), (24, 40), (1, 5))
MARGIN = 1e-3


def draw_flow(rng, n, H, W):
    """half of the pixels move a few pixels, the others up to 1.5 frames: taps inside, partly outside, all outside, and both sides of the clamp"""
    small = rng.random(n) < 0.5
    u = np.where(small, rng.uniform(-4, 4, n), rng.uniform(-1.5 * W, 1.5 * W, n))
    v = np.where(small, rng.uniform(-4, 4, n), rng.uniform(-1.5 * H, 1.5 * H, n))
    return u.astype(np.float32), v.astype(np.float32)


def inputs(name, lin32):
    B, C, H, W = CASES[name]
    rng = np.random.default_rng(8200 + list(CASES).index(name))
    x = (rng.integers(-128, 129, (B, C, H, W)) / 64.0).astype(np.float32)
    g = rng.integers(-4, 5, (B, C, H, W)).astype(np.float32)
    flow = np.zeros((B, 2, H, W), np.float32)
    bad = np.ones((B, H, W), bool)
    for _ in range(1000):
        n = int(bad.sum())
        if n == 0:
            break
        u, v = draw_flow(rng, n, H, W)
        flow[:, 0][bad], flow[:, 1][bad] = u, v
        bad = np.zeros((B, H, W), bool)
        for mode in MODES.values():
            for dtype in (np.float32, np.float64):
                bad |= rs.near_flip(rs.sample_positions(flow, mode, dtype, lin32(H, W) if dtype == np.float32 else None), mode, H, W, MARGIN)
    else:
        raise AssertionError("%s: pixels near a discrete boundary remain" % name)
    return x, flow, g


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "flow_warp.npz"))
    a = ap.parse_args()
    import torch
    import ref_harness
    ref_harness.install()
    try:
        from utils import flow_viz  # noqa: F401
    except Exception:                                            # noqa: BLE001
        sys.modules["utils.flow_viz"] = types.ModuleType("utils.flow_viz")
    import utils.transform as T                                  # the reference's own
    out = {}

    def lin32(H, W):
        return torch.linspace(-1.0, 1.0, W).numpy(), torch.linspace(-1.0, 1.0, H).numpy()

    def run(mode, dtype, x, flow, g):
        prev = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        T.backwarp_tenGrid.clear()
        try:
            xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
            ft = torch.from_numpy(flow).to(dtype).requires_grad_(True)
            if mode == "warp":
                o, m = T.warp(xt, ft)
                assert not m.requires_grad
            else:
                o, m = T.warp_rife(xt, ft), None
            assert o.dtype == dtype
            o.backward(torch.from_numpy(g).to(dtype))
        finally:
            torch.set_default_dtype(prev)
            T.backwarp_tenGrid.clear()
        r = dict(out=o.detach().numpy(), grad_x=xt.grad.numpy(), grad_flow=ft.grad.numpy())
        if m is not None:
            assert (m[:, :1] == m).all()                         # the same in every channel
            r["mask"] = m[:, :1].numpy()
        return r

    for name, (B, C, H, W) in CASES.items():
        x, flow, g = inputs(name, lin32)
        out["%s/x" % name], out["%s/flow" % name], out["%s/g" % name] = x, flow, g
        for mode, code in MODES.items():
            k = "%s/%s/" % (name, mode)
            r32, r64 = run(mode, torch.float32, x, flow, g), run(mode, torch.float64, x, flow, g)
            rest = rs.flow_warp(x, flow, code, g)
            p32 = rs.sample_positions(flow, code, np.float32, lin32(H, W))
            assert not rs.near_flip(p32, code, H, W, MARGIN).any() and not rs.near_flip(rest["pos"], code, H, W, MARGIN).any(), k
            for c32, c64 in zip(rs.cells(p32), rs.cells(rest["pos"])):
                assert (c32 == c64).all(), "%s: the float32 run takes other cells than float64" % k
            cov = rest["all_in"].mean(), (rest["mask"] == 0).mean(), ((rest["mask"] > 0) & ~rest["all_in"][:, None]).mean(), 1 - rest["pos"]["mx"].mean()
            for f, v32 in r32.items():
                v64 = r64[f]
                assert v32.dtype == np.float32 and v64.dtype == np.float64 and v32.shape == v64.shape
                assert rel(rest[f], v64) <= 1e-9, "%s%s: the restatement is %.3g from the reference's float64" % (k, f, rel(rest[f], v64))
                d = (v64 - v32.astype(np.float64)).astype(np.float32)
                assert rel(v32.astype(np.float64) + d.astype(np.float64), v64) <= 1e-12
                out[k + "ref32/" + f], out[k + "d64/" + f] = v32, d
                out[k + "e_ref/" + f] = np.float64(rel(v32.astype(np.float64), v64))
            print("%-22s all taps inside %.2f, none %.2f, some %.2f, clamped in x %.2f;  e_ref %s" % (
                k, *cov, "  ".join("%s %.2e" % (f, out[k + "e_ref/" + f]) for f in r32)))

    B, C, H, W = ZERO_FLOW_SHAPE
    rng = np.random.default_rng(8300)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    z = np.zeros((B, 2, H, W), np.float32)
    T.backwarp_tenGrid.clear()
    o = T.warp_rife(torch.from_numpy(x), torch.from_numpy(z)).numpy()
    T.backwarp_tenGrid.clear()
    assert np.abs(o - x).max() <= 1e-5
    out["rife/zero_flow/x"], out["rife/zero_flow/out"] = x, o

    for i, shape in enumerate(GET_FLOW_SHAPES):
        np.random.seed(9400 + i)
        M = T.gen_random_perspective()
        out["get_flow/%d/M" % i] = M
        out["get_flow/%d/shape" % i] = np.array(shape, np.int64)
        out["get_flow/%d/flow" % i] = T.get_flow(np.zeros(shape, np.uint8), M)
        assert out["get_flow/%d/flow" % i].dtype == np.float32

    np.savez_compressed(a.out, **out)
    print("%s: %d arrays, %d bytes" % (a.out, len(out), os.path.getsize(a.out)))
    assert os.path.getsize(a.out) < 1 << 20


if __name__ == "__main__":
    main()
