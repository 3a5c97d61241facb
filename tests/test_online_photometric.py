"""RAFT's photometric augmentation in the online pair source: mpf_photometric_pairs (mpf_photometric.hip), ops.photometric_pairs and
OnlinePairs(photometric=...).

Host tests: a numpy restatement of the contract (include/mpiflow_hip.h, MpfPhotoSample) against Pillow - exhaustively over every RGB and HSV
triple for L, the HSV conversions, the blend ops and the hue round trip, and on whole jitter chains in every op order - the draw rules and
the C ABI.  GPU tests: the kernel bit for bit against the restatement, and the source with the feature off, on, and resumed."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, I64 = np.float32, np.float64, np.int64


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------- the contract, restated in numpy

def lum(r, g, b):
    return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16


def blend(a, x, f):
    """PIL's Image.blend of u8 values: (float)a + f * (float)(x - a) in fp32, clamped to 0..255, truncated"""
    a = np.asarray(a, I64)
    t = a.astype(F32) + F32(f) * (x - a).astype(F32)
    return np.clip(t, 0, 255).astype(I64)


def rgb2hsv(r, g, b):
    """Pillow's Convert.c rgb2hsv: float quotients, the hue sum and fmod in double"""
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(F32)
        s = cr / maxc.astype(F32)
        rc, gc, bc = ((maxc - c).astype(F32) / cr for c in (r, g, b))
        h = np.where(r == maxc, bc - gc, np.where(g == maxc, (2.0 + rc.astype(F64) - bc.astype(F64)).astype(F32),
                                                  (4.0 + gc.astype(F64) - rc.astype(F64)).astype(F32)))
        h = np.fmod(h.astype(F64) / 6.0 + 1.0, 1.0).astype(F32)
        gray = maxc == minc
        H = np.where(gray, 0, np.nan_to_num(h.astype(F64) * 255.0)).astype(I64)
        S = np.where(gray, 0, np.nan_to_num(s.astype(F64) * 255.0)).astype(I64)
    return np.clip(H, 0, 255), np.clip(S, 0, 255), maxc


def _round(x):
    """C round() of values >= 0: half away from zero"""
    t = np.trunc(x)
    return (t + (x - t >= 0.5)).astype(I64)


def hsv2rgb(H, S, V):
    """Pillow's Convert.c hsv2rgb: the sector and remainder in double, fs and fs * f in float, the three products in double"""
    h6 = H.astype(F64) * 6.0 / 255.0
    i = np.floor(h6).astype(I64)
    f = (h6 - i.astype(F64)).astype(F32)
    fs = (S.astype(F64) / 255.0).astype(F32)
    v = V.astype(F64)
    p = np.clip(_round(v * (1.0 - fs.astype(F64))), 0, 255)
    q = np.clip(_round(v * (1.0 - (fs * f).astype(F64))), 0, 255)
    t = np.clip(_round(v * (1.0 - fs.astype(F64) * (1.0 - f.astype(F64)))), 0, 255)
    sel = i % 6
    r = np.choose(sel, [V, q, p, p, t, V])
    g = np.choose(sel, [t, V, V, q, p, p])
    b = np.choose(sel, [p, p, t, V, V, q])
    gray = S == 0
    return np.where(gray, V, r), np.where(gray, V, g), np.where(gray, V, b)


def hue(r, g, b, shift):
    H, S, V = rgb2hsv(r, g, b)
    return hsv2rgb((H + shift) & 255, S, V)


def ref_jitter(rgb, p):
    """one parameter set's chain on an int [..., 3] RGB image (the contrast mean over all of it)"""
    r, g, b = (rgb[..., c].astype(I64) for c in range(3))
    for op in p["order"]:
        if op == 0:
            r, g, b = (blend(0, c, p["brightness"]) for c in (r, g, b))
        elif op == 1:
            L = lum(r, g, b)
            m = int(int(L.sum()) / L.size + 0.5)
            r, g, b = (blend(m, c, p["contrast"]) for c in (r, g, b))
        elif op == 2:
            L = lum(r, g, b)
            r, g, b = (blend(L, c, p["saturation"]) for c in (r, g, b))
        else:
            r, g, b = hue(r, g, b, p["hue_shift"])
    return np.stack([r, g, b], -1)


def ref_photometric(src, dst, s):
    """the whole contract on one pair of u8 [H,W,3] BGR frames -> (src_out, dst_out)"""
    H = src.shape[0]
    a, b = src[..., ::-1].astype(I64), dst[..., ::-1].astype(I64)
    if s["joint"]:
        st = ref_jitter(np.concatenate([a, b], 0), s["jitter"][0])
        a, b = st[:H], st[H:]
    else:
        a, b = ref_jitter(a, s["jitter"][0]), ref_jitter(b, s["jitter"][1])
    o1, o2 = np.ascontiguousarray(a[..., ::-1].astype(np.uint8)), np.ascontiguousarray(b[..., ::-1].astype(np.uint8))
    if s["rects"]:
        mean = o2.reshape(-1, 3).astype(I64).sum(0) // (o2.shape[0] * o2.shape[1])
        for x0, y0, dx, dy in s["rects"]:
            o2[y0:y0 + dy, x0:x0 + dx] = mean
    return o1, o2


# ------------------------------------------------------------------------------------------------------- Pillow, as torchvision drives it

def _pil():
    return pytest.importorskip("PIL.Image"), pytest.importorskip("PIL.ImageEnhance")


def pil_jitter(rgb_u8, p):
    Image, ImageEnhance = _pil()
    im = Image.fromarray(np.ascontiguousarray(rgb_u8, np.uint8))
    for op in p["order"]:
        if op == 0:
            im = ImageEnhance.Brightness(im).enhance(p["brightness"])
        elif op == 1:
            im = ImageEnhance.Contrast(im).enhance(p["contrast"])
        elif op == 2:
            im = ImageEnhance.Color(im).enhance(p["saturation"])
        else:
            h, s, v = im.convert("HSV").split()
            h = Image.fromarray(((np.array(h).astype(I64) + p["hue_shift"]) & 255).astype(np.uint8))
            im = Image.merge("HSV", (h, s, v)).convert("RGB")
    return np.array(im)


def _all_triples():
    """[4096, 4096, 3] u8 holding every RGB triple once"""
    i = np.arange(1 << 24, dtype=I64)
    return np.stack([i >> 16, (i >> 8) & 255, i & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.fixture(scope="module")
def triples():
    return _all_triples()


def _split(img):
    return tuple(img[..., c].astype(I64) for c in range(3))


def test_luma_equals_pillow_on_every_rgb_triple(triples):
    Image, _ = _pil()
    assert (np.array(Image.fromarray(triples).convert("L")).astype(I64) == lum(*_split(triples))).all()


def test_rgb_to_hsv_equals_pillow_on_every_rgb_triple(triples):
    Image, _ = _pil()
    want = np.array(Image.fromarray(triples).convert("HSV")).astype(I64)
    got = np.stack(rgb2hsv(*_split(triples)), -1)
    assert (got == want).all()


def test_hsv_to_rgb_equals_pillow_on_every_hsv_triple(triples):
    Image, _ = _pil()
    want = np.array(Image.frombytes("HSV", (4096, 4096), triples.tobytes()).convert("RGB")).astype(I64)
    got = np.stack(hsv2rgb(*_split(triples)), -1)
    assert (got == want).all()


@pytest.mark.parametrize("op,factor", [(0, 0.6), (0, 1.2345), (0, 2.5), (1, 0.6), (1, 1.37), (1, 3.0), (2, 0.0), (2, 0.71), (2, 1.4), (2, 2.2)])
def test_blend_ops_equal_pillow_on_every_rgb_triple(triples, op, factor):
    name = ("brightness", "contrast", "saturation")[op]
    p = dict(order=[op], **{name: float(F32(factor))})
    assert (ref_jitter(triples, p) == pil_jitter(triples, p)).all()


@pytest.mark.parametrize("shift", [-40, 0, 40])
def test_hue_round_trip_equals_pillow_on_every_rgb_triple(triples, shift):
    p = dict(order=[3], hue_shift=shift)
    got = ref_jitter(triples, p)
    assert (got == pil_jitter(triples, p)).all()
    if shift == 0:
        assert (got != triples).any(axis=-1).sum() > 10_000_000            # the round trip is lossy


def test_jitter_chains_in_every_order_equal_pillow_stacked_and_per_frame():
    from mpiflow_amd import online
    rs = np.random.RandomState(3)
    c = online.photometric_config(True)
    for n, order in enumerate(itertools.permutations(range(4))):
        a = rs.randint(0, 256, (13, 17, 3)).astype(np.uint8)
        b = np.clip(a.astype(I64) + rs.randint(-60, 60, a.shape), 0, 255).astype(np.uint8)
        p1, p2 = online.jitter_params(rs, c), online.jitter_params(rs, c)
        p1["order"], p2["order"] = list(order), list(order[n % 4:] + order[:n % 4])
        stack = np.concatenate([a, b], 0)                                    # RAFT's symmetric jitter
        assert (ref_jitter(stack.astype(I64), p1) == pil_jitter(stack, p1)).all(), order
        for img, p in ((a, p1), (b, p2)):                                    # asymmetric: a set and a mean per frame
            assert (ref_jitter(img.astype(I64), p) == pil_jitter(img, p)).all(), order


# ------------------------------------------------------------------------------------------------------- draw rules

def test_draws_follow_torchvision_and_raft_rules():
    from mpiflow_amd import online
    c = online.photometric_config(True)
    assert c == online.RAFT_PHOTOMETRIC and c["hue"] == 0.5 / 3.14
    rs = np.random.RandomState(11)
    H, W, n = 384, 1280, 3000
    asym = erased = 0
    counts = []
    for _ in range(n):
        s = online.photometric_params(rs, H, W, c)
        assert len(s["jitter"]) == (1 if s["joint"] else 2)
        asym += not s["joint"]
        for p in s["jitter"]:
            assert sorted(p["order"]) == [0, 1, 2, 3]
            for k in ("brightness", "contrast", "saturation"):
                assert 0.6 <= p[k] <= 1.4 and float(F32(p[k])) == p[k]
            assert abs(p["hue"]) <= 0.5 / 3.14 and float(F32(p["hue"])) == p["hue"]
            assert p["hue_shift"] == int(p["hue"] * 255.0) and -40 <= p["hue_shift"] <= 40
        if s["rects"]:
            erased += 1
            counts.append(len(s["rects"]))
            for x0, y0, dx, dy in s["rects"]:
                assert 0 <= x0 < W and 0 <= y0 < H and 50 <= dx < 100 and 50 <= dy < 100
    assert abs(asym / n - 0.2) < 0.03 and abs(erased / n - 0.5) < 0.04
    assert set(counts) == {1, 2}


def test_zero_settings_are_neither_drawn_nor_applied_and_the_draw_order_is_raft_s():
    from mpiflow_amd import online
    c = online.photometric_config(dict(brightness=0, hue=0, asymmetric_prob=1.0, eraser_prob=1.0, eraser_bounds=(3, 9)))
    rs, replay = np.random.RandomState(4), np.random.RandomState(4)
    s = online.photometric_params(rs, 20, 30, c)
    assert replay.rand() < 1.0
    for p in s["jitter"]:
        perm = [int(v) for v in replay.permutation(4)]
        assert p["order"] == [o for o in perm if o in (1, 2)]
        assert p["contrast"] == float(F32(replay.uniform(0.6, 1.4))) and p["saturation"] == float(F32(replay.uniform(0.6, 1.4)))
        assert p["brightness"] == 1.0 and p["hue_shift"] == 0
    assert replay.rand() < 1.0
    k = replay.randint(1, 3)
    want = []
    for _ in range(k):
        x0, y0 = replay.randint(0, 30), replay.randint(0, 20)
        want.append((x0, y0, replay.randint(3, 9), replay.randint(3, 9)))
    assert s["rects"] == want
    assert rs.randint(1 << 30) == replay.randint(1 << 30)                  # nothing else consumed
    assert online.photometric_config(None) is None
    for bad in (dict(hue=0.6), dict(contrast=-0.1), dict(eraser_bounds=(5, 5)), dict(eraser_prob=1.5), dict(nope=1)):
        with pytest.raises(ValueError):
            online.photometric_config(bad)


def test_photometric_draws_leave_the_spatial_stream_alone():
    """the source's fifth stream is RandomState([seed, 3]); the spatial draws come from [seed, 1] alone, whatever the photometric ones take"""
    from mpiflow_amd import online
    seed, H, W = 114514, 96, 128
    ref = np.random.RandomState([seed, 1])
    want = [online.augment_params(ref, H, W, (64, 96), dict(min_scale=-0.2, max_scale=0.5)) for _ in range(20)]
    aug, photo = np.random.RandomState([seed, 1]), np.random.RandomState([seed, 3])
    got = []
    for _ in range(20):
        got.append(online.augment_params(aug, H, W, (64, 96), dict(min_scale=-0.2, max_scale=0.5)))
        online.photometric_params(photo, H, W, online.RAFT_PHOTOMETRIC)
    assert got == want
    a, b = np.random.RandomState([seed, 3]).rand(8), np.random.RandomState([seed, 1]).rand(8)
    assert not np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------- C ABI

def _layout(tmp_path, struct, fields):
    src = tmp_path / ("%s.c" % struct)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpiflow_hip.h"\nint main(void){printf("%%zu", sizeof(%s));\n' % struct
                   + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) + "return 0;}\n")
    exe = tmp_path / struct
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


def test_photometric_abi_declared_and_structs_match_header(lib, tmp_path):
    for name in ("mpf_photometric_pairs", "mpf_photometric_workspace"):
        assert name in lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read()
    assert "int mpf_photometric_pairs(" in hdr and "size_t mpf_photometric_workspace(" in hdr
    for cls in (lib.MpfPhotoJitter, lib.MpfPhotoSample):
        fields = [f[0] for f in cls._fields_]
        vals = _layout(tmp_path, cls.__name__, fields)
        assert vals[0] == ctypes.sizeof(cls)
        assert vals[1:] == [getattr(cls, f).offset for f in fields]
    L = lib.load()
    assert L.mpf_photometric_workspace(1) >= 40 and L.mpf_photometric_workspace(7) == 7 * L.mpf_photometric_workspace(1)
    assert L.mpf_version() == 601


def test_photometric_bad_arguments_return_error_codes(lib):
    L = lib.load()
    one, H, W = 256, 8, 8
    ws_bytes = L.mpf_photometric_workspace(1)

    def sample(**kw):
        a = lib.MpfPhotoSample(src=one, dst=one, src_out=one, dst_out=one, joint=1, n_rect=0)
        for j in range(2):
            a.jitter[j].n_ops = 4
            for k in range(4):
                a.jitter[j].order[k] = k
            a.jitter[j].brightness = a.jitter[j].contrast = a.jitter[j].saturation = 1.0
        for k, v in kw.items():
            if k.startswith("j_"):
                setattr(a.jitter[1], k[2:], v)
            elif k == "order":
                for i, o in enumerate(v):
                    a.jitter[0].order[i] = o
            elif k == "rects":
                a.n_rect = len(v)
                for i, r in enumerate(v):
                    for c in range(4):
                        a.rect[i][c] = r[c]
            else:
                setattr(a, k, v)
        return (lib.MpfPhotoSample * 1)(a)

    def call(arr, B=1, h=H, w=W, ws=ctypes.c_void_p(one), nbytes=ws_bytes):
        return L.mpf_photometric_pairs(arr, B, h, w, ws, nbytes, None)

    def err(rc, text):
        return rc == 10001 and text in L.mpf_last_error()

    assert err(call(None), b"null pointer")
    assert err(call(sample(), ws=None), b"null pointer")
    assert err(call(sample(), B=0), b"B must be")
    assert err(call(sample(), h=0), b"bad shape")
    assert err(call(sample(), w=-3), b"bad shape")
    assert err(call(sample(src_out=None)), b"null pointer in sample 0")
    assert err(call(sample(dst=None)), b"null pointer in sample 0")
    assert err(call(sample(joint=2)), b"joint")
    assert err(call(sample(order=[0, 1, 1, 3])), b"distinct")
    assert err(call(sample(order=[0, 1, 4, 3])), b"distinct")
    assert err(call(sample(j_n_ops=5)), b"n_ops")
    assert err(call(sample(j_contrast=float("nan"))), b"finite")
    assert err(call(sample(j_brightness=float("inf"))), b"finite")
    assert err(call(sample(j_saturation=-0.5)), b"finite")
    assert err(call(sample(j_hue_shift=128)), b"hue shift")
    assert err(call(sample(j_hue_shift=-129)), b"hue shift")
    assert err(call(sample(n_rect=3)), b"n_rect")
    assert err(call(sample(n_rect=-1)), b"n_rect")
    assert err(call(sample(rects=[(8, 0, 2, 2)])), b"rectangle 0")
    assert err(call(sample(rects=[(0, 0, 2, 2), (0, -1, 2, 2)])), b"rectangle 1")
    assert err(call(sample(rects=[(0, 0, 0, 2)])), b"extent")
    assert err(call(sample(), nbytes=ws_bytes - 1), b"workspace")
    assert err(call(sample(), ws=ctypes.c_void_p(one + 4)), b"aligned")


# ------------------------------------------------------------------------------------------------------- GPU: the kernel

@pytest.fixture(scope="module")
def dev(lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib.load()
    return torch.device("cuda:0")


def _run(dev, srcs, dsts, samples):
    from mpiflow_amd import ops
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    out = ops.photometric_pairs([dict(src=T(s), dst=T(d), **p) for s, d, p in zip(srcs, dsts, samples)])
    torch.cuda.synchronize()
    return out["src"].cpu().numpy(), out["dst"].cpu().numpy()


def _check(dev, srcs, dsts, samples):
    o1, o2 = _run(dev, srcs, dsts, samples)
    for b, (s, d, p) in enumerate(zip(srcs, dsts, samples)):
        w1, w2 = ref_photometric(s, d, p)
        assert (o1[b] == w1).all(), ("src", b, p, int((o1[b] != w1).sum()))
        assert (o2[b] == w2).all(), ("dst", b, p, int((o2[b] != w2).sum()))
    return o1, o2


def _set(order, **kw):
    p = dict(order=list(order), brightness=1.0, contrast=1.0, saturation=1.0, hue_shift=0)
    p.update(kw)
    return p


@pytest.mark.gpu
def test_kernel_single_ops_on_every_rgb_triple(dev, triples):
    bgr = np.ascontiguousarray(triples[..., ::-1])
    rev = np.ascontiguousarray(bgr[::-1, ::-1])
    for p in (_set([0], brightness=1.3717), _set([1], contrast=0.6123), _set([1], contrast=1.39), _set([2], saturation=1.27),
              _set([2], saturation=0.0), _set([3], hue_shift=40), _set([3], hue_shift=0), _set([3], hue_shift=-40)):
        p = {k: (float(F32(v)) if isinstance(v, float) else v) for k, v in p.items()}
        # src and dst on separate sets (joint 0): each holds every triple, the contrast mean is each frame's own
        _check(dev, [bgr], [rev], [dict(joint=0, jitter=[p, p], rects=[])])


@pytest.mark.gpu
@pytest.mark.parametrize("asym", [0.0, 1.0])
def test_kernel_random_frames_random_draws(dev, asym):
    from mpiflow_amd import online
    rs = np.random.RandomState(21 + int(asym))
    H, W, B = 37, 53, 9
    c = online.photometric_config(dict(asymmetric_prob=asym, eraser_prob=0.7, eraser_bounds=(4, 30)))
    srcs = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    dsts = np.clip(srcs.astype(I64) + rs.randint(-40, 40, srcs.shape), 0, 255).astype(np.uint8)
    samples = [online.photometric_params(rs, H, W, c) for _ in range(B)]
    assert all(s["joint"] == (asym == 0.0) for s in samples) and any(s["rects"] for s in samples)
    _check(dev, srcs, dsts, samples)


@pytest.mark.gpu
def test_kernel_contrast_first_middle_last_and_clipped_rectangles(dev):
    rs = np.random.RandomState(8)
    H, W = 61, 259
    f = dict(brightness=float(F32(1.21)), contrast=float(F32(0.77)), saturation=float(F32(1.33)), hue_shift=-17)
    g = dict(brightness=float(F32(0.66)), contrast=float(F32(1.38)), saturation=float(F32(0.81)), hue_shift=23)
    orders = [[1, 0, 2, 3], [3, 2, 1, 0], [0, 3, 2, 1], [2, 1], [1], [3, 1]]
    samples = []
    for n, o in enumerate(orders):
        rects = [[(W - 3, H - 2, 50, 60)], [(0, 0, W + 10, 1), (5, H - 1, 3, 9)], [(W - 1, 0, 1, H + 5)], [], [(10, 20, 30, 10)], []][n]
        samples.append(dict(joint=n % 2, jitter=[_set(o, **f), _set(o[::-1], **g)], rects=rects))
    samples.append(dict(joint=0, jitter=[_set([]), _set([1, 3], **g)], rects=[(0, 0, 1, 1)]))     # an empty chain passes the frame through
    srcs = rs.randint(0, 256, (len(samples), H, W, 3)).astype(np.uint8)
    dsts = rs.randint(0, 256, (len(samples), H, W, 3)).astype(np.uint8)
    o1, _ = _check(dev, srcs, dsts, samples)
    assert (o1[-1] == srcs[-1]).all()


@pytest.mark.gpu
def test_kernel_more_than_32_samples_and_repeated_runs_byte_identical(dev):
    from mpiflow_amd import online
    rs = np.random.RandomState(5)
    H, W, B = 9, 11, 37
    c = online.photometric_config(dict(asymmetric_prob=0.5, eraser_prob=0.8, eraser_bounds=(1, 6)))
    srcs = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    dsts = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    samples = [online.photometric_params(rs, H, W, c) for _ in range(B)]
    _check(dev, srcs, dsts, samples)
    # a frame size with many blocks per frame, run three times: the integer atomics leave no trace of the order the blocks ran in
    H, W, B = 384, 1280, 4
    srcs = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    dsts = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    samples = [online.photometric_params(rs, H, W, c) for _ in range(B)]
    for s in samples:
        s["jitter"] = [dict(p, order=[0, 1, 2, 3]) for p in s["jitter"]]
    first = _check(dev, srcs, dsts, samples)
    for _ in range(2):
        again = _run(dev, srcs, dsts, samples)
        assert all((a == b).all() for a, b in zip(first, again))


# ------------------------------------------------------------------------------------------------------- GPU: the source

def _toy_dataset(base, names, size=(40, 56)):
    from PIL import Image
    for d in ("images", "disps", "masks"):
        (base / d).mkdir(parents=True, exist_ok=True)
    h, w = size
    for n in names:
        rs = np.random.RandomState(sum(map(ord, n)))
        Image.fromarray((rs.rand(h, w, 3) * 255).astype(np.uint8)).save(base / "images" / (n + ".png"))
        yy, xx = np.mgrid[0:h, 0:w]
        Image.fromarray((255 * (0.2 + 0.6 * xx / w)).astype(np.uint8)).save(base / "disps" / (n + ".png"))
        m = np.zeros((h, w), np.uint8)
        m[h // 4:(5 * h) // 8, w // 4:(5 * w) // 8] = 1
        m[(7 * h) // 10:(9 * h) // 10, w // 10:w // 3] = 2
        Image.fromarray(m).save(base / "masks" / (n + ".png"))


PHOTO = dict(asymmetric_prob=0.5, eraser_prob=0.7, eraser_bounds=(5, 25))


def _source(base, dev, **kw):
    from mpiflow_amd.online import OnlinePairs
    args = dict(batch_size=3, crop=(40, 56), width=64, height=48, seed=5, pairs_per_image=2, mpi_from="disparity", planes=16, fill="peel",
                augment=dict(min_scale=-0.2, max_scale=0.5, do_flip=True), shuffle=True, mix=5, device=dev)
    args.update(kw)
    return OnlinePairs(str(base), **args)


def _batches(src, epochs=1):
    out = []
    for _ in range(epochs):
        for batch in src:
            torch.cuda.synchronize()
            out.append({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()})
    return out


def _same(a, b, keys):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in keys:
            if isinstance(x[k], np.ndarray):
                assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), k
            else:
                assert x[k] == y[k], k


@pytest.mark.gpu
def test_source_without_photometric_is_unchanged_and_with_it_keeps_the_spatial_draws(dev, tmp_path):
    _toy_dataset(tmp_path, ["g%d" % i for i in range(5)])
    with _source(tmp_path, dev) as a:
        plain = _batches(a, 2)
        st_plain = a.state_dict()
    with _source(tmp_path, dev, photometric=None) as b:
        none = _batches(b, 2)
        assert sorted(b.state_dict()) == sorted(st_plain) and "photo_rs" not in st_plain
    assert len(plain) >= 4 and all(sorted(x) == ["flow", "image1", "image2", "meta", "valid"] for x in none)
    _same(plain, none, ["image1", "image2", "flow", "valid", "meta"])
    with _source(tmp_path, dev, photometric=PHOTO) as c:
        on = _batches(c, 2)
        assert "photo_rs" in c.state_dict()
    _same(plain, on, ["flow", "valid", "meta"])
    assert all(len(x["photo_meta"]) == 3 for x in on)
    assert any((x["image1"] != y["image1"]).any() for x, y in zip(plain, on))


@pytest.mark.gpu
def test_source_images_equal_the_restatement_of_the_unaugmented_frames(dev, tmp_path):
    _toy_dataset(tmp_path, ["h%d" % i for i in range(4)])
    kw = dict(crop=None, augment=None, shuffle=False, mix=0, batch_size=2)
    with _source(tmp_path, dev, **kw) as a:
        off = _batches(a)
    with _source(tmp_path, dev, photometric=PHOTO, **kw) as b:
        on = _batches(b)
    assert len(on) == len(off) >= 3
    metas = [s for x in on for s in x["photo_meta"]]
    assert any(not s["joint"] for s in metas) and any(s["joint"] for s in metas) and any(s["rects"] for s in metas)
    to_bgr = lambda t: np.ascontiguousarray(t.transpose(1, 2, 0)[..., ::-1]).astype(np.uint8)     # noqa: E731 - [3,H,W] RGB -> u8 BGR
    for x, y in zip(off, on):
        assert x["meta"] == y["meta"]
        for i, s in enumerate(y["photo_meta"]):
            w1, w2 = ref_photometric(to_bgr(x["image1"][i]), to_bgr(x["image2"][i]), s)
            assert (to_bgr(y["image1"][i]) == w1).all() and (to_bgr(y["image2"][i]) == w2).all()


@pytest.mark.gpu
def test_source_resumes_photometric_batches_exactly(dev, tmp_path):
    _toy_dataset(tmp_path, ["k%d" % i for i in range(5)])
    with _source(tmp_path, dev, photometric=True, prefetch=1) as a:
        full = _batches(a, 2)
    k = 2
    with _source(tmp_path, dev, photometric=True, prefetch=3) as b:
        it = iter(b)
        for _ in range(k):
            next(it)
        st = b.state_dict()
    with _source(tmp_path, dev, photometric=True, prefetch=2) as c:
        c.load_state_dict(st)
        rest = _batches(c, 2)
        with pytest.raises(ValueError):
            c.load_state_dict({key: v for key, v in st.items() if key != "photo_rs"})
    keys = ["image1", "image2", "flow", "valid", "meta", "photo_meta"]
    _same(rest[:len(full) - k], full[k:], keys)
