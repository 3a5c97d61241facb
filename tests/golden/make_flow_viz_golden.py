#!/usr/bin/env python3
"""Record RAFT's flow outputs by RUNNING THE REFERENCE ITSELF (flow_to_image of RAFT/core/utils/flow_viz.py, writeFlowKITTI of
RAFT/core/utils/frame_utils.py; numpy, CPU) -> tests/golden/flow_viz.npz.

    python tests/golden/make_flow_viz_golden.py [--out PATH]   (in the build container: needs the reference tree, numpy, PIL)

Colour fixtures (VIZ_CASES), each with its inputs, the reference's uint8 output per image and `dist`, see below:

    rand37x53   one 37 x 53 flow, sigma 8 px: more than one block of the colouring pass, nothing a multiple of 4, 8 or 64
    hand5x7     background noise below 1 px and hand-placed pixels (HAND): (+0, +0); v = +0 with u > 0 (atan2(-0, -u) = -pi: a = -1, k0 = 0);
                v = -0 with u > 0 (atan2(+0, -u) = +pi: a = 1, k0 = 54, k1 wraps to 0, f = 0); the carrier of rad_max, (3, 4), whose rad is
                just under 1 after the normalisation by rad_max + 1e-5
    edge5x7     the carrier (0, 4096): 4096 + 1e-5 rounds to 4096 in float32, so its rad is EXACTLY 1 after the normalisation, the boundary of
                upstream's `rad <= 1` branch, and a = -0.5 exactly; with (+0, +0) and both signs of zero again
    zero4x6     all zeros: upstream gets atan2(-0, -0) = -pi and every byte 255
    batch2      two 11 x 19 images with sigma 0.3 and 30 px: rad_max 100 x apart; the reference is called per image
    clip5       rand37x53's flow with clip_flow=5 (upstream clips to [0, 5])
    bgr         rand37x53's flow with convert_to_bgr=True
    stacked     a 13 x 21 flow under a random frame whose values include x.999 fractions: demo.py:viz's np.concatenate([img, flo], axis=0)
                as uint8 (truncation, not rounding); the frame half has dist = 0.5 (no band)

`dist`: the script evaluates the same formula in float64 throughout (eval64 below, written from the formula, no reference text) and stores per
byte the distance of 255 * col from the nearest integer.  THE PARITY RULE of tests/test_raft_flow_outputs.py: a byte with dist > DELTA = 0.01
equals the reference exactly; a byte inside the band may differ by 1.  DELTA is a bound, not a measurement: a few ulp of a float32 atan2
(about 2.4e-7 in a) times 27 in fk times at most 255 levels is about 2e-3 levels; DELTA is five times that.

Two thirds of all bytes cannot feel the atan2 at all and get dist = 0.5, NO band, whatever their value (many are exactly 255 or 0, which the
plain distance would put inside the band): a channel whose two wheel entries are equal (on every ramp of the wheel one channel stays 255
and one stays 0), and every byte of a vector with a zero component (after the clip), whose angle 0, +-pi/2 or +-pi every atan2 returns
exactly.  There the kernel repeats the reference's correctly rounded operations one for one.  Asserted here per image: with the plain
distance the reference itself obeys the rule against floor(eval64); after the override the band holds at most 5 % of the bytes (a
uniform fraction predicts 2 % of the remaining third); every hand-placed pixel (`hand`: their positions) and the whole all-zero image lie
outside the band, so the test demands them exact.  A fixture that fails gets another seed or another hand-placed vector, never a wider DELTA.

KITTI (kitti9x13): the array the reference's writeFlowKITTI hands to cv2.imwrite (captured by ref_harness's cv2 stub, B, G, R) reversed to
the file's R, G, B order, for a 9 x 13 flow of both signs with exact multiples of 1/64 and products with 64 whose fraction is >= 0.5
(truncation); `valid` is a sparse 0 / 1 map and `code_valid` the same code with it in the third channel (upstream's writer has no
valid argument: it writes ones).  readFlowKITTI needs a real cv2 and is not run."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DELTA = 0.01
MAX_BAND = 0.05

# hand-placed pixels: (y, x, u, v)
HAND = [(0, 0, 0.0, 0.0), (1, 2, 2.5, 0.0), (2, 3, 1.25, -0.0), (3, 5, 3.0, 4.0), (4, 6, -0.0, 0.0)]
EDGE = [(0, 0, 0.0, 0.0), (1, 1, 1000.0, 0.0), (2, 4, 2000.0, -0.0), (3, 3, 0.0, 4096.0), (4, 6, -1024.0, 512.0)]


def colorwheel64():
    """the 55 x 3 wheel: six ramps of 15, 6, 4, 11, 13, 6 steps between R, Y, G, C, B, M, R"""
    wheel = np.zeros((55, 3))
    col = 0
    for n, full, ramp, down in ((15, 0, 1, False), (6, 1, 0, True), (4, 1, 2, False), (11, 2, 1, True), (13, 2, 0, False), (6, 0, 2, True)):
        steps = np.floor(255 * np.arange(n) / n)
        wheel[col:col + n, full] = 255
        wheel[col:col + n, ramp] = 255 - steps if down else steps
        col += n
    return wheel


def eval64(flow_2hw, clip_flow=None, convert_to_bgr=False):
    """-> (255 * col before the floor [H,W,3], float64 throughout; `fixed` [H,W,3]: the bytes on which the last bits of a float32 atan2 have no
    influence: the two wheel entries of the blend are equal, with fk further than 1e-3 from an integer, so that no evaluation blends another
    pair; or the (clipped) vector has a zero component, whose angle, 0, +-pi/2 or +-pi, every atan2 returns exactly)"""
    uv = flow_2hw.astype(np.float64)
    if clip_flow is not None:
        uv = np.clip(uv, 0, clip_flow)
    u, v = uv
    axis = (u == 0) | (v == 0)
    d = np.sqrt(u * u + v * v).max() + 1e-5
    u, v = u / d, v / d
    rad = np.sqrt(u * u + v * v)
    fk = (np.arctan2(-v, -u) / np.pi + 1) / 2 * 54
    k0 = np.clip(np.floor(fk).astype(np.int64), 0, 54)
    k1 = (k0 + 1) % 55
    f = (fk - k0)[..., None]
    wheel = colorwheel64() / 255.0
    col = (1 - f) * wheel[k0] + f * wheel[k1]
    col = np.where((rad <= 1)[..., None], 1 - rad[..., None] * (1 - col), col * 0.75)
    fixed = ((wheel[k0] == wheel[k1]) & (np.abs(fk - np.round(fk)) > 1e-3)[..., None]) | axis[..., None]
    flip = (lambda t: t[..., ::-1]) if convert_to_bgr else (lambda t: t)
    return 255 * flip(col), flip(fixed)


def place(flow, pixels):
    for y, x, u, v in pixels:
        flow[0, y, x], flow[1, y, x] = u, v
    return flow


def viz_cases():
    """name -> (flow [N,2,H,W] float32, image [N,3,H,W] float32 or None, clip_flow, convert_to_bgr, hand-placed pixels)"""
    rng = lambda seed: np.random.default_rng(seed)
    rand = (rng(9100).standard_normal((1, 2, 37, 53)) * 8).astype(np.float32)
    hand = place((rng(9101).standard_normal((2, 5, 7)) * 0.4).astype(np.float32), HAND)[None]
    edge = place((rng(9102).standard_normal((2, 5, 7)) * 300).astype(np.float32), EDGE)[None]
    batch = np.stack([(rng(9103).standard_normal((2, 11, 19)) * 0.3).astype(np.float32), (rng(9104).standard_normal((2, 11, 19)) * 30).astype(np.float32)])
    sflow = (rng(9105).standard_normal((1, 2, 13, 21)) * 5).astype(np.float32)
    r = rng(9106)
    image = r.uniform(0, 255, (1, 3, 13, 21))
    image = np.where(r.uniform(size=image.shape) < 0.3, np.floor(image) + 0.999, image).astype(np.float32)
    return {"rand37x53": (rand, None, None, False, []), "hand5x7": (hand, None, None, False, HAND), "edge5x7": (edge, None, None, False, EDGE),
            "zero4x6": (np.zeros((1, 2, 4, 6), np.float32), None, None, False, [(y, x, 0.0, 0.0) for y in range(4) for x in range(6)]),
            "batch2": (batch, None, None, False, []), "clip5": (rand, None, 5.0, False, []), "bgr": (rand, None, None, True, []),
            "stacked": (sflow, image, None, False, [])}


def kitti_flow():
    rng = np.random.default_rng(9120)
    flow = (rng.standard_normal((2, 9, 13)) * 20).astype(np.float32)
    flow[:, 0, :4] = np.array([[-3.0, 7.5, 1 / 64, -1 / 64], [0.0, -0.0, 511.984375, -512.0]], np.float32)     # exact multiples of 1/64, the range's ends
    flow[:, 1, :4] = np.array([[0.5 / 64, 0.75 / 64, -0.5 / 64, -0.75 / 64], [10 + 0.99 / 64, -10 - 0.99 / 64, 100.0078125, -100.0078125]], np.float32)
    valid = (rng.uniform(size=(9, 13)) < 0.3).astype(np.float32)
    return flow, valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "flow_viz.npz"))
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import ref_harness
    ref_harness.install()                                    # the cv2 stub: imwrite records its argument
    sys.path.insert(0, os.path.join(ref_harness.REFERENCE_ROOT, "RAFT", "core"))
    for m in [m for m in sys.modules if m == "utils" or m.startswith("utils.")]:
        del sys.modules[m]
    from utils import flow_viz, frame_utils                  # the reference's own
    assert np.array_equal(flow_viz.make_colorwheel(), colorwheel64())
    rec = {"numpy_version": np.array(np.__version__), "delta": np.float64(DELTA), "names": np.array(list(viz_cases()))}
    for name, (flow, image, clip, bgr, hand) in viz_cases().items():
        refs, dists = [], []
        for n in range(flow.shape[0]):
            ref = flow_viz.flow_to_image(np.ascontiguousarray(flow[n].transpose(1, 2, 0)), clip_flow=clip, convert_to_bgr=bgr)
            assert ref.dtype == np.uint8 and ref.shape == flow.shape[2:] + (3,)
            x, fixed = eval64(flow[n], clip, bgr)
            dist = np.abs(x - np.round(x))
            far = dist > DELTA
            exact = np.floor(x)
            assert np.array_equal(ref[far], exact[far].astype(np.uint8)), (name, "the reference differs from the float64 evaluation outside the band")
            assert (np.abs(ref.astype(np.int64) - np.round(x).astype(np.int64)) <= 1).all(), (name, "the reference is more than 1 from the float64 evaluation")
            dist[fixed] = 0.5                                # no band for them: the kernel repeats the reference operation for operation there
            share = (dist <= DELTA).mean()
            assert share <= MAX_BAND, (name, "the band holds %.1f %% of the bytes: another seed" % (100 * share))
            for y, xx, _, _ in hand:
                assert (dist[y, xx] > DELTA).all(), (name, "the hand-placed pixel (%d, %d) lies in the band" % (y, xx))
            if image is not None:
                top = np.transpose(image[n], (1, 2, 0))      # demo.py:viz: img = img[0].permute(1,2,0).cpu().numpy()
                ref = np.concatenate([top, ref], axis=0).astype(np.uint8)
                assert (top.astype(np.uint8) != np.round(top).astype(np.uint8)).mean() > 0.3, "the frame does not tell truncation from rounding"
                dist = np.concatenate([np.full(top.shape, 0.5), dist], axis=0)
            refs.append(ref)
            dists.append(dist.astype(np.float32))
            print("%-10s image %d: %4d bytes, %5.2f %% in the band, %5.2f %% free of the angle's last bits, reference == floor(float64) outside the band"
                  % (name, n, far.size, 100 * share, 100 * fixed.mean()))
        p = name + "/"
        rec[p + "flow"] = flow
        if image is not None:
            rec[p + "image"] = image
        rec[p + "clip_flow"] = np.float64(np.nan if clip is None else clip)
        rec[p + "convert_to_bgr"] = np.bool_(bgr)
        rec[p + "hand"] = np.array([(y, x) for y, x, _, _ in hand], np.int64).reshape(-1, 2)
        rec[p + "out"] = np.stack(refs)
        rec[p + "dist"] = np.stack(dists)
    assert (rec["zero4x6/out"] == 255).all()
    edge = rec["edge5x7/flow"][0]
    d32 = np.sqrt(np.square(edge[0]) + np.square(edge[1])).max() + np.float32(1e-5)
    assert d32.dtype == np.float32 and d32 == 4096.0, "edge5x7: the carrier's rad is not exactly 1 after the normalisation"
    m = rec["batch2/flow"]
    rm = np.sqrt((m.astype(np.float64) ** 2).sum(axis=1)).max(axis=(1, 2))
    assert rm[1] / rm[0] > 50, rm

    flow, valid = kitti_flow()
    frame_utils.writeFlowKITTI("unused.png", np.ascontiguousarray(flow.transpose(1, 2, 0)))
    code = np.ascontiguousarray(ref_harness.captured["imwrite"]["img"][..., ::-1])       # cv2 takes B, G, R: the file holds R, G, B
    assert code.dtype == np.uint16 and code.shape == (9, 13, 3) and (code[..., 2] == 1).all()
    x = 64.0 * flow.astype(np.float64) + 2 ** 15
    assert x.min() >= 0 and x.max() < 65536, "a code outside 0..65535 is undefined in numpy"
    frac = x - np.floor(x)
    assert ((frac >= 0.5).sum() >= 20) and ((frac == 0).sum() >= 8) and (flow < 0).any() and (flow > 0).any()
    assert 0.1 < valid.mean() < 0.5
    rec["kitti9x13/flow"], rec["kitti9x13/valid"], rec["kitti9x13/code"] = flow[None], valid[None], code[None]
    with_valid = code.copy()
    with_valid[..., 2] = valid.astype(np.uint16)
    rec["kitti9x13/code_valid"] = with_valid[None]
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 200 * 1000
    return 0


if __name__ == "__main__":
    sys.exit(main())
