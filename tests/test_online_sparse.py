"""RAFT's sparse (KITTI-stage) augmentation: the kernel mpf_augment_sparse_pairs (mpf_augment_sparse.hip), its host draws
online.sparse_augment_params and OnlinePairs(sparse=...).

Host tests: the C ABI, argument validation, the draws and a numpy restatement of the kernel's contract against tests/golden/sparse_augment.npz
(RAFT's own SparseFlowAugmentor and KITTI flow code, recorded by tests/golden/make_sparse_golden.py), the sparse photometric draws and the
configuration errors.  GPU tests: the kernel bit for bit against the restatement and the golden, its images against mpf_augment_pairs', and
the source end to end, resumed and prefetched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_online import _bits, _toy_dataset, ref_augment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------------------- the restatement

def ref_source(flow, valid, quantize):
    """KITTI's code and the source validity: -> (u_q, v_q) [H,W,2] f32 (0 where invalid), ok [H,W] bool"""
    ok = np.ones(flow.shape[:2], bool) if valid is None else valid != 0
    flow = flow.astype(np.float32)
    if not quantize:
        return np.where(ok[..., None], flow, np.float32(0)), ok
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.float32(64) * flow + np.float32(32768)
        inside = (t > -1) & (t < 65536)
    ok = ok & inside[..., 0] & inside[..., 1]
    q = np.where(ok[..., None], t, np.float32(0)).astype(np.int64)              # trunc toward zero
    fq = (q - 32768).astype(np.float32) / np.float32(64)
    return np.where(ok[..., None], fq, np.float32(0)), ok


def _candidates(n_src, n_dst, s):
    """per target index d < n_dst, the source indices with rint(i * s) == d in descending order (-1 padded); target 0 has none"""
    tgt = np.rint(np.arange(n_src, dtype=np.float64) * s).astype(np.int64)
    lists = [np.nonzero(tgt == d)[0][::-1] for d in range(n_dst)]
    lists[0] = lists[0][:0]
    out = np.full((n_dst, max(1, max(len(v) for v in lists))), -1, np.int64)
    for d, v in enumerate(lists):
        out[d, :len(v)] = v
    return out


def ref_sparse_flow(flow, valid, quantize, p, h, w):
    """numpy restatement of include/mpiflow_hip.h's mpf_augment_sparse_pairs for flow and valid, in the gather form:
    -> flow [2,h,w] f32, valid [h,w] f32"""
    fq, ok = ref_source(flow, valid, quantize)
    if not p.get("resize", 0):
        F, V = fq, ok
    else:
        sx, sy, Hr, Wr = p["scale_x"], p["scale_y"], p["Hr"], p["Wr"]
        cy, cx = _candidates(ok.shape[0], Hr, sy), _candidates(ok.shape[1], Wr, sx)
        F, V = np.zeros((Hr, Wr, 2), np.float32), np.zeros((Hr, Wr), bool)
        for ky in range(cy.shape[1]):                                  # the largest row with a valid candidate, then its largest column
            ys = np.broadcast_to(cy[:, ky][:, None], (Hr, Wr))
            for kx in range(cx.shape[1]):
                xs = np.broadcast_to(cx[:, kx][None, :], (Hr, Wr))
                hit = (ys >= 0) & (xs >= 0) & ~V
                hit &= ok[np.maximum(ys, 0), np.maximum(xs, 0)]
                F[hit] = fq[ys[hit], xs[hit]]
                V |= hit
        F = np.stack([(F[..., 0].astype(np.float64) * sx).astype(np.float32), (F[..., 1].astype(np.float64) * sy).astype(np.float32)], -1)
    if p.get("flip_h", 0):
        F = F[:, ::-1].copy()
        F[..., 0] = -F[..., 0]
        V = V[:, ::-1]
    y0, x0 = p.get("y0", 0), p.get("x0", 0)
    return np.ascontiguousarray(F[y0:y0 + h, x0:x0 + w].transpose(2, 0, 1)), V[y0:y0 + h, x0:x0 + w].astype(np.float32)


class _LogRS:
    """a RandomState that logs uniform / rand / randint as make_sparse_golden.py logs the reference's global draws"""

    def __init__(self, seed):
        self.rs, self.log = np.random.RandomState(seed), []

    def uniform(self, lo, hi):
        v = self.rs.uniform(lo, hi)
        self.log.append((0, lo, hi, float(v)))
        return v

    def rand(self):
        v = self.rs.rand()
        self.log.append((1, 0, 1, float(v)))
        return v

    def randint(self, lo, hi):
        v = self.rs.randint(lo, hi)
        self.log.append((2, lo, hi, float(v)))
        return v


def _golden_cases():
    g = load_golden("sparse_augment")
    out = []
    for i in range(int(g["n_cases"])):
        c = "c%02d_" % i
        H, W, h, w, do_flip, lo, hi, prob, quantize, seed = g[c + "settings"]
        out.append(dict(H=int(H), W=int(W), h=int(h), w=int(w), augment=dict(min_scale=float(lo), max_scale=float(hi), do_flip=bool(do_flip),
                        spatial_aug_prob=float(prob)), quantize=int(quantize), seed=int(seed), flow_in=g[c + "flow_in"], valid_in=g[c + "valid_in"],
                        draws=g[c + "draws"], fxfy=g[c + "fxfy"], flow=g[c + "flow"], valid=g[c + "valid"]))
    return out


def _golden_params(case):
    from mpiflow_amd import online
    rs = _LogRS(case["seed"])
    p = online.sparse_augment_params(rs, case["H"], case["W"], (case["h"], case["w"]), case["augment"])
    return p, np.array(rs.log, np.float64)


# ---------------------------------------------------------------------------------------------------------------- host tests

def test_sparse_abi_declared_exported_and_struct_matches_header(lib, tmp_path):
    assert "mpf_augment_sparse_pairs" in lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read()
    assert "int mpf_augment_sparse_pairs(" in hdr and "} MpfSparseAugmentSample;" in hdr
    for so in (lib.LIB_PATH, lib.WITNESS_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
        assert " mpf_augment_sparse_pairs\n" in syms, so
    fields = [f[0] for f in lib.MpfSparseAugmentSample._fields_]
    src = tmp_path / "o.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpiflow_hip.h"\nint main(void){printf("%zu", sizeof(MpfSparseAugmentSample));\n'
                   + "".join('printf(" %%zu", offsetof(MpfSparseAugmentSample, %s));\n' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "o"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(lib.MpfSparseAugmentSample)
    assert vals[1:] == [getattr(lib.MpfSparseAugmentSample, f).offset for f in fields]


def test_sparse_bad_arguments_return_error_codes(lib):
    L = lib.load()
    one = 256
    outs = [ctypes.c_void_p(one)] * 4

    def sample(**kw):
        a = lib.MpfSparseAugmentSample(src=one, dst=one, flow=one, valid=None, quantize=1, resize=0, scale_x=1.0, scale_y=1.0, Hr=8, Wr=8, flip_h=0,
                                       y0=0, x0=0)
        for k, v in kw.items():
            setattr(a, k, v)
        return (lib.MpfSparseAugmentSample * 1)(a)

    def call(arr, B=1, h=8, w=8, o=outs):
        return L.mpf_augment_sparse_pairs(arr, B, 8, 8, h, w, *o, None)

    assert call(None) == 10001 and b"null pointer" in L.mpf_last_error()
    assert call(sample(), o=outs[:3] + [None]) == 10001 and b"null pointer" in L.mpf_last_error()
    assert call(sample(), B=0) == 10001 and b"B must be" in L.mpf_last_error()
    assert call(sample(flow=None)) == 10001 and b"null pointer in sample 0" in L.mpf_last_error()
    assert call(sample(Wr=9)) == 10001 and b"resize == 0 needs" in L.mpf_last_error()
    assert call(sample(x0=1)) == 10001 and b"outside the resized frame" in L.mpf_last_error()
    assert call(sample(resize=1, scale_x=2.0, scale_y=2.0, Hr=16, Wr=16, y0=9)) == 10001 and b"outside" in L.mpf_last_error()
    assert call(sample(resize=1, scale_y=-1.0)) == 10001 and b"bad scale" in L.mpf_last_error()
    assert call(sample(resize=2)) == 10001 and b"resize must be" in L.mpf_last_error()
    assert call(sample(quantize=3)) == 10001 and b"quantize must be" in L.mpf_last_error()
    assert call(sample(flip_h=-1)) == 10001 and b"flip_h must be" in L.mpf_last_error()
    assert call(sample(), w=9) == 10001 and b"outside" in L.mpf_last_error()


def test_golden_covers_the_cases_it_is_for():
    cases = _golden_cases()
    assert len(cases) >= 20
    assert any(c["fxfy"][0] < 1 for c in cases) and any(c["fxfy"][0] > 1 for c in cases) and any(np.isnan(c["fxfy"][0]) for c in cases)
    assert any((c["H"], c["W"]) == (c["h"], c["w"]) for c in cases)
    assert any(c["valid_in"].all() for c in cases) and any(not c["valid_in"].all() for c in cases)
    assert any(c["quantize"] for c in cases) and any(not c["quantize"] for c in cases)
    flips = [_golden_params(c)[0]["flip_h"] for c in cases]
    assert 0 < sum(flips) < len(flips)


def test_draws_replay_the_reference_spatial_transform():
    for c in _golden_cases():
        p, log = _golden_params(c)
        assert log.shape == c["draws"].shape and (log == c["draws"]).all(), c["seed"]
        fx, fy = c["fxfy"]
        if np.isnan(fx):
            assert p["resize"] == 0 and (p["Hr"], p["Wr"], p["scale_x"], p["scale_y"]) == (c["H"], c["W"], 1.0, 1.0)
        else:
            assert p["resize"] == 1 and p["scale_x"] == fx and p["scale_y"] == fy
            assert (p["Hr"], p["Wr"]) == (int(np.rint(c["H"] * fy)), int(np.rint(c["W"] * fx)))
        assert 0 <= p["y0"] <= p["Hr"] - c["h"] and 0 <= p["x0"] <= p["Wr"] - c["w"]
        assert p["y0"] == min(int(log[-2, 3]), p["Hr"] - c["h"]) and p["x0"] == min(max(int(log[-1, 3]), 0), p["Wr"] - c["w"])
        assert p["flip_h"] == int(c["augment"]["do_flip"] and log[2, 3] < 0.5)


def test_restatement_equals_the_reference_sparse_augmentor_bit_for_bit():
    holes = collisions = 0
    for c in _golden_cases():
        p, _ = _golden_params(c)
        f, v = ref_sparse_flow(c["flow_in"], c["valid_in"], c["quantize"], p, c["h"], c["w"])
        assert _bits(f, c["flow"].transpose(2, 0, 1)) == 0, c["seed"]
        assert _bits(v, c["valid"]) == 0, c["seed"]
        if p["resize"]:
            holes += p["scale_x"] > 1
            collisions += p["scale_x"] < 1
            if p["y0"] == 0:
                assert (v[0] == 0).all()                                   # row 0 of the resized map is never written
    assert holes and collisions


def test_sparse_draw_rules():
    from mpiflow_amd import online
    rs = np.random.RandomState(3)
    H, W, crop = 384, 1280, (288, 960)
    lo = max(289 / 384, 961 / 1280)
    n, resized, flips = 3000, 0, 0
    for _ in range(n):
        p = online.sparse_augment_params(rs, H, W, crop, dict(online.RAFT_KITTI_AUGMENT, do_flip=True))
        assert p["scale_x"] == p["scale_y"] and "flip_v" not in p
        if p["resize"]:
            resized += 1
            assert lo <= p["scale_x"] <= 2 ** 0.4 + 1e-12
        assert 0 <= p["y0"] <= p["Hr"] - crop[0] and 0 <= p["x0"] <= p["Wr"] - crop[1]
        flips += p["flip_h"]
    assert abs(resized / n - 0.8) < 0.03 and abs(flips / n - 0.5) < 0.03
    assert not any(online.sparse_augment_params(rs, H, W, crop, online.RAFT_KITTI_AUGMENT)["flip_h"] for _ in range(200))
    # augment=None: no resize, no flip, the crop still drawn by the margin rule (two randint draws)
    a, b = np.random.RandomState(9), np.random.RandomState(9)
    p = online.sparse_augment_params(a, 48, 64, (40, 56), None)
    y0, x0 = b.randint(0, 48 - 40 + 20), b.randint(-50, 64 - 56 + 50)
    assert p == dict(resize=0, scale_x=1.0, scale_y=1.0, Hr=48, Wr=64, flip_h=0, y0=min(y0, 8), x0=min(max(x0, 0), 8))
    assert a.rand() == b.rand()


def test_sparse_photometric_draws_are_symmetric_with_the_sparse_settings():
    from mpiflow_amd import online
    c = online.photometric_config(True, sparse=True)
    assert c == dict(brightness=0.3, contrast=0.3, saturation=0.3, hue=0.3 / 3.14, asymmetric_prob=0.0, eraser_prob=0.5, eraser_bounds=(50, 100))
    assert online.photometric_config(True) == online.RAFT_PHOTOMETRIC
    for seed in range(20):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        got = online.photometric_params(a, 48, 64, c, asymmetric=False)
        want_j = online.jitter_params(b, c)                          # no rand() for the asymmetric case in front of it
        rects = []
        if b.rand() < 0.5:
            for _ in range(int(b.randint(1, 3))):
                rects.append((int(b.randint(0, 64)), int(b.randint(0, 48)), int(b.randint(50, 100)), int(b.randint(50, 100))))
        assert got == dict(joint=1, jitter=[want_j], rects=rects)
        assert a.rand() == b.rand()
        j = got["jitter"][0]
        assert all(0.7 <= j[k] <= 1.3 for k in ("brightness", "contrast", "saturation")) and abs(j["hue"]) <= 0.3 / 3.14
    # the dense default is unchanged: it still draws the asymmetric case first
    a, b = np.random.RandomState(1), np.random.RandomState(1)
    online.photometric_params(a, 48, 64, online.RAFT_PHOTOMETRIC)
    b.rand()
    online.jitter_params(b, online.RAFT_PHOTOMETRIC)


def test_sparse_configuration_errors():
    from mpiflow_amd import online
    assert online.sparse_config(None, None) is None and online.sparse_config(False, dict(stretch_prob=0.8)) is None
    assert online.sparse_config(True, online.RAFT_KITTI_AUGMENT) == dict(quantize=True)
    assert online.sparse_config(dict(quantize=False), None) == dict(quantize=False)
    with pytest.raises(ValueError, match="unknown keys"):
        online.sparse_config(dict(quantise=True), None)
    for bad in (dict(stretch_prob=0.5), dict(v_flip_prob=0.1), dict(max_stretch=0.2), dict(h_flip_prob=0.5)):
        with pytest.raises(ValueError, match="reads only"):
            online.sparse_config(True, dict(online.RAFT_KITTI_AUGMENT, **bad))
    with pytest.raises(ValueError, match="symmetric"):
        online.photometric_config(dict(asymmetric_prob=0.2), sparse=True)
    assert online.photometric_config(dict(asymmetric_prob=0.2))["asymmetric_prob"] == 0.2
    # OnlinePairs checks them before it touches a device or the dataset
    for kw in (dict(sparse=True, augment=dict(stretch_prob=0.8)), dict(sparse=True, photometric=dict(asymmetric_prob=0.1)),
               dict(sparse=dict(quantize=True, margin=3))):
        with pytest.raises(ValueError):
            online.OnlinePairs("/nonexistent", **kw)


# ---------------------------------------------------------------------------------------------------------------- GPU tests

@pytest.fixture(scope="module")
def dev(lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib.load()
    return torch.device("cuda:0")


def _special_flow(rs, H, W):
    """flows on the 16-bit code's edges: k/64 +- 1 ulp, negative fractions, beyond +-512, the range limits"""
    k = rs.randint(-40000, 40000, (H, W, 2)).astype(np.float32) / np.float32(64)
    f = k.copy()
    m = rs.randint(0, 6, (H, W, 2))
    f[m == 1] = np.nextafter(k[m == 1], np.float32(np.inf))
    f[m == 2] = np.nextafter(k[m == 2], np.float32(-np.inf))
    f[m == 3] = -rs.rand(int((m == 3).sum())).astype(np.float32) * 3
    edge = np.array([-512, -512.0 - 1 / 64, -512.0 - 1 / 128, -512.02, 511.984375, 511.99, 512, 600, -700, 1e6], np.float32)
    f[m == 4] = edge[rs.randint(0, len(edge), int((m == 4).sum()))]
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,h,w,B", [(37, 53, 17, 25, 5), (61, 97, 33, 57, 6), (23, 301, 11, 140, 35), (40, 64, 40, 64, 3)])
def test_sparse_kernel_is_bit_exact_against_the_contract(dev, H, W, h, w, B):
    from mpiflow_amd import ops
    rs = np.random.RandomState(H * 1000 + W)
    src = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    dst = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    flow = np.stack([_special_flow(rs, H, W) if b % 2 else ((rs.rand(H, W, 2) - 0.5) * 1400).astype(np.float32) for b in range(B)])
    masks = (rs.rand(B, H, W) < 0.6).astype(np.uint8)
    lo = max((h + 1) / H, (w + 1) / W)
    params, valids = [], []
    for b in range(B):
        p = dict(quantize=int(b % 3 != 2), resize=0, scale_x=1.0, scale_y=1.0, Hr=H, Wr=W, flip_h=int(rs.rand() < 0.5), y0=0, x0=0)
        s = {1: 0.77, 2: 1.31, 3: 1.0, 4: float(rs.uniform(0.75, 1.6))}.get(b % 5)      # collisions, holes, resize == 1 at scale 1, any
        if s is not None:
            s = max(s, lo)                                                   # the crop must fit the resized frame
            p.update(resize=1, scale_x=s, scale_y=s, Hr=int(np.rint(H * s)), Wr=int(np.rint(W * s)))
        ymax, xmax = p["Hr"] - h, p["Wr"] - w
        p["y0"], p["x0"] = [(rs.randint(0, ymax + 1), rs.randint(0, xmax + 1)), (0, 0), (ymax, xmax), (0, xmax), (ymax, 0)][b % 5]
        params.append(p)
        valids.append(None if b % 4 == 0 else masks[b])
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    samples = [dict(src=T(src[b]), dst=T(dst[b]), flow=T(flow[b]), valid=None if valids[b] is None else T(valids[b]), **params[b]) for b in range(B)]
    out = ops.augment_sparse_pairs(samples, size=(h, w))
    torch.cuda.synchronize()
    assert any(p["resize"] and p["scale_x"] < 1 for p in params) or lo > 0.77
    for b in range(B):
        f, v = ref_sparse_flow(flow[b], valids[b], params[b]["quantize"], params[b], h, w)
        dense = dict(params[b], flip_v=0)
        i1, i2, _, _ = ref_augment(src[b], dst[b], flow[b], dense, h, w)
        for k, ref in (("image1", i1), ("image2", i2), ("flow", f), ("valid", v)):
            assert _bits(out[k][b].cpu().numpy(), ref) == 0, (k, b, params[b])


@pytest.mark.gpu
def test_sparse_kernel_equals_the_reference_on_the_golden_inputs(dev):
    from mpiflow_amd import ops
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    for c in _golden_cases():
        p, _ = _golden_params(c)
        img = T(np.zeros((c["H"], c["W"], 3), np.uint8))
        valid = None if c["valid_in"].all() else T(c["valid_in"])
        out = ops.augment_sparse_pairs([dict(src=img, dst=img, flow=T(c["flow_in"]), valid=valid, quantize=c["quantize"], **p)], size=(c["h"], c["w"]))
        torch.cuda.synchronize()
        assert _bits(out["flow"][0].cpu().numpy(), c["flow"].transpose(2, 0, 1)) == 0, c["seed"]
        assert _bits(out["valid"][0].cpu().numpy(), c["valid"]) == 0, c["seed"]


@pytest.mark.gpu
def test_sparse_images_equal_the_dense_kernel_images(dev):
    from mpiflow_amd import ops
    rs = np.random.RandomState(11)
    H, W, h, w = 45, 133, 30, 90
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    src, dst = T(rs.randint(0, 256, (H, W, 3)).astype(np.uint8)), T(rs.randint(0, 256, (H, W, 3)).astype(np.uint8))
    flow = T(((rs.rand(H, W, 2) - 0.5) * 300).astype(np.float32))
    ps = []
    for s, flip in ((0.77, 0), (0.9, 1), (1.0, 1), (1.23, 0), (1.6, 1)):
        Hr, Wr = int(np.rint(H * s)), int(np.rint(W * s))
        ps.append(dict(resize=int(s != 1.0), scale_x=s, scale_y=s, Hr=Hr, Wr=Wr, flip_h=flip, y0=int(rs.randint(0, Hr - h + 1)), x0=int(rs.randint(0, Wr - w + 1))))
    sp = ops.augment_sparse_pairs([dict(src=src, dst=dst, flow=flow, quantize=1, **p) for p in ps], size=(h, w))
    de = ops.augment_pairs([dict(src=src, dst=dst, flow=flow, flip_v=0, **p) for p in ps], size=(h, w))
    torch.cuda.synchronize()
    for k in ("image1", "image2"):
        assert _bits(sp[k].cpu().numpy(), de[k].cpu().numpy()) == 0, k


def _source(base, dev, **kw):
    from mpiflow_amd.online import OnlinePairs
    args = dict(batch_size=3, crop=(40, 56), width=64, height=48, seed=5, pairs_per_image=2, mpi_from="disparity", planes=16, fill="peel",
                augment=dict(min_scale=-0.3, max_scale=0.5, do_flip=True), shuffle=True, mix=5, device=dev, sparse=True)
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
def test_sparse_source_equals_the_restatement_of_the_raw_pairs(dev, tmp_path):
    _toy_dataset(tmp_path, ["s%d" % i for i in range(5)])
    H, W, (h, w) = 48, 64, (40, 56)
    with _source(tmp_path, dev, sparse=None, crop=None, augment=None, mix=0) as a:
        raw = _batches(a)
    with _source(tmp_path, dev, mix=0) as b:
        sp = _batches(b)
    assert len(raw) == len(sp) >= 3
    to_bgr = lambda t: np.ascontiguousarray(t.transpose(1, 2, 0)[..., ::-1]).astype(np.uint8)     # noqa: E731 - [3,H,W] RGB -> u8 BGR
    resized = flipped = holes = 0
    for x, y in zip(raw, sp):
        for i, m in enumerate(y["meta"]):
            assert m[:3] == x["meta"][i][:3] and m[6] == 0 and m[3] == m[4]
            s = m[3]
            p = dict(resize=int(s != 1.0), scale_x=s, scale_y=s, Hr=int(np.rint(H * s)) if s != 1.0 else H, Wr=int(np.rint(W * s)) if s != 1.0 else W,
                     flip_h=m[5], y0=m[7], x0=m[8])
            src, dst, flow = to_bgr(x["image1"][i]), to_bgr(x["image2"][i]), np.ascontiguousarray(x["flow"][i].transpose(1, 2, 0))
            i1, i2, _, _ = ref_augment(src, dst, flow, dict(p, flip_v=0), h, w)
            f, v = ref_sparse_flow(flow, None, 1, p, h, w)
            for k, ref in (("image1", i1), ("image2", i2), ("flow", f), ("valid", v)):
                assert _bits(y[k][i], ref) == 0, (k, m)
            resized += p["resize"]
            flipped += p["flip_h"]
            holes += (v == 0).sum()
    assert resized and flipped and holes


@pytest.mark.gpu
def test_sparse_photometric_source_resumes_exactly_and_ignores_prefetch(dev, tmp_path):
    _toy_dataset(tmp_path, ["t%d" % i for i in range(5)])
    with _source(tmp_path, dev, photometric=True, prefetch=1) as a:
        full = _batches(a, 2)
    with _source(tmp_path, dev, photometric=True, prefetch=4) as a4:
        full4 = _batches(a4, 2)
    keys = ["image1", "image2", "flow", "valid", "meta", "photo_meta"]
    _same(full, full4, keys)
    assert all(s["joint"] == 1 for x in full for s in x["photo_meta"])
    k = 2
    with _source(tmp_path, dev, photometric=True, prefetch=3) as b:
        it = iter(b)
        for _ in range(k):
            next(it)
        st = b.state_dict()
    with _source(tmp_path, dev, photometric=True, prefetch=2) as c:
        c.load_state_dict(st)
        rest = _batches(c, 2)
    _same(rest[:len(full) - k], full[k:], keys)
