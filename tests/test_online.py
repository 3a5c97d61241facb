"""The online pair source (mpiflow_amd/online.py) and its kernel mpf_augment_pairs (mpf_augment.hip).

Host tests: the C ABI of the kernel, the schedule replay against the CLI's draws on the global generators, the augmentation draws.
GPU tests: the kernel bit for bit against a numpy restatement of its contract, online == the CLI's files, sharding, determinism and
resume, stream hand-over."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


def _toy_dataset(base, names, size=(40, 56), empty_mask=()):
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
        if n not in empty_mask:
            m[h // 4:(5 * h) // 8, w // 4:(5 * w) // 8] = 1
            m[(7 * h) // 10:(9 * h) // 10, w // 10:w // 3] = 2 + (len(n) + ord(n[-1])) % 3
        Image.fromarray(m).save(base / "masks" / (n + ".png"))


# ---------------------------------------------------------------------------------------------------------------- host tests

def test_augment_abi_declared_and_struct_matches_header(lib, tmp_path):
    assert "mpf_augment_pairs" in lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read()
    assert "int mpf_augment_pairs(" in hdr and "MpfAugmentSample" in hdr
    fields = [f[0] for f in lib.MpfAugmentSample._fields_]
    src = tmp_path / "o.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpiflow_hip.h"\nint main(void){printf("%zu", sizeof(MpfAugmentSample));\n'
                   + "".join('printf(" %%zu", offsetof(MpfAugmentSample, %s));\n' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "o"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(lib.MpfAugmentSample)
    assert vals[1:] == [getattr(lib.MpfAugmentSample, f).offset for f in fields]


def test_augment_bad_arguments_return_error_codes(lib):
    L = lib.load()
    one = 256
    outs = [ctypes.c_void_p(one)] * 4

    def sample(**kw):
        a = lib.MpfAugmentSample(src=one, dst=one, flow=one, resize=0, scale_x=1.0, scale_y=1.0, Hr=8, Wr=8, flip_h=0, flip_v=0, y0=0, x0=0)
        for k, v in kw.items():
            setattr(a, k, v)
        return (lib.MpfAugmentSample * 1)(a)

    def call(arr, B=1, h=8, w=8, o=outs):
        return L.mpf_augment_pairs(arr, B, 8, 8, h, w, *o, None)

    assert call(None) == 10001 and b"null pointer" in L.mpf_last_error()
    assert call(sample(), o=[None] + outs[1:]) == 10001 and b"null pointer" in L.mpf_last_error()
    assert call(sample(), B=0) == 10001 and b"B must be" in L.mpf_last_error()
    assert call(sample(src=None)) == 10001 and b"null pointer in sample 0" in L.mpf_last_error()
    assert call(sample(Hr=9)) == 10001 and b"resize == 0 needs" in L.mpf_last_error()
    assert call(sample(y0=1)) == 10001 and b"outside the resized frame" in L.mpf_last_error()
    assert call(sample(resize=1, scale_x=2.0, scale_y=2.0, Hr=16, Wr=16, x0=9)) == 10001 and b"outside" in L.mpf_last_error()
    assert call(sample(resize=1, scale_x=0.0, Hr=8, Wr=8)) == 10001 and b"bad scale" in L.mpf_last_error()
    assert call(sample(flip_h=2)) == 10001 and b"flips" in L.mpf_last_error()
    assert call(sample(), h=9) == 10001 and b"outside" in L.mpf_last_error()


def _cli_draws(seed, mask_max, R, ext_cz=0.15, poses="v2"):
    """The CLI's loop (gen_3dphoto_dynamic.py main()) on the global generators, seeded as it seeds them."""
    from mpiflow_amd import host_math
    random.seed(seed)
    np.random.seed(seed)
    out = []
    for m in mask_max:
        if m <= 0:
            out.append(None)
            continue
        ids, pp = [], []
        for _ in range(R):
            ids.append(np.random.randint(m) + 1)
            pp.append(host_math.draw_pose_parameters(ext_cz, profile=poses))
            pp.append(host_math.draw_pose_parameters(ext_cz, base_motions=[0, 0, 0], profile=poses))
        out.append((ids, pp))
    return out


def test_schedule_replays_the_cli_draws_on_private_streams(tmp_path):
    from mpiflow_amd import io_formats, online
    names = ["a0", "a1", "a2", "a3", "a4"]
    _toy_dataset(tmp_path, names, empty_mask=("a2",))
    mask_max = [io_formats.mask_max_of_file(str(tmp_path / "masks" / (n + ".png"))) for n in names]
    assert mask_max[2] == 0 and min(mask_max[:2] + mask_max[3:]) >= 2
    random.seed(99)
    np.random.seed(99)
    g_py, g_np = random.getstate(), np.random.get_state()
    for poses in ("v2", "coco"):
        sched = online.Schedule(114514, 0.15, 3, poses)
        mine = [sched.draw(m) for m in mask_max]
        assert random.getstate() == g_py
        st = np.random.get_state()
        assert st[0] == g_np[0] and (st[1] == g_np[1]).all() and st[2:] == g_np[2:]
        want = _cli_draws(114514, mask_max, 3, poses=poses)
        assert mine[2] is None and want[2] is None
        for a, b in zip(mine, want):
            if a is None:
                continue
            assert a[0] == b[0]
            assert len(a[1]) == 6 and a[1] == b[1]                    # 12 floats per pair, every one equal (Python floats)
        # epoch 2 continues the streams: a second pass equals the CLI's draws of the list twice in a row
        again = [sched.draw(m) for m in mask_max]
        twice = _cli_draws(114514, mask_max + mask_max, 3, poses=poses)
        assert again == twice[len(mask_max):]
        random.setstate(g_py)
        np.random.set_state(g_np)


def test_augmentation_draws_follow_raft_rules():
    from mpiflow_amd import online
    rs = np.random.RandomState(5)
    H, W, crop = 384, 1280, (288, 960)
    min_scale = max((288 + 8) / 384, (960 + 8) / 1280)
    n, resized, fh, fv, stretched = 4000, 0, 0, 0, 0
    for _ in range(n):
        p = online.augment_params(rs, H, W, crop, dict(min_scale=-0.2, max_scale=0.5, do_flip=True))
        if p["resize"]:
            resized += 1
            assert p["scale_x"] >= min_scale and p["scale_y"] >= min_scale
            assert p["scale_x"] <= 2 ** 0.7 + 1e-9 and p["scale_y"] <= 2 ** 0.7 + 1e-9
            assert p["Hr"] == int(np.rint(H * p["scale_y"])) and p["Wr"] == int(np.rint(W * p["scale_x"]))
            stretched += p["scale_x"] != p["scale_y"]
        else:
            assert (p["Hr"], p["Wr"], p["scale_x"], p["scale_y"]) == (H, W, 1.0, 1.0)
        assert 0 <= p["y0"] and p["y0"] + crop[0] <= p["Hr"] and 0 <= p["x0"] and p["x0"] + crop[1] <= p["Wr"]
        assert p["y0"] < max(1, p["Hr"] - crop[0]) and p["x0"] < max(1, p["Wr"] - crop[1])     # randint's upper bound is exclusive
        fh += p["flip_h"]
        fv += p["flip_v"]
    assert abs(resized / n - 0.8) < 0.03 and abs(fh / n - 0.5) < 0.03 and abs(fv / n - 0.1) < 0.02
    assert stretched / resized > 0.7
    p = online.augment_params(rs, H, W, crop, dict(do_flip=False))
    assert p["flip_h"] == p["flip_v"] == 0
    assert online.augment_params(rs, H, W, (H, W), None) == dict(resize=0, scale_x=1.0, scale_y=1.0, Hr=H, Wr=W, flip_h=0, flip_v=0, y0=0, x0=0)


# ---------------------------------------------------------------------------------------------------------------- GPU tests

@pytest.fixture(scope="module")
def dev(lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib.load()
    return torch.device("cuda:0")


def _taps(d, n, scale):
    f = ((d.astype(np.float64) + 0.5) * (1.0 / scale) - 0.5).astype(np.float32)
    lo, hi = f < 0, f >= np.float32(n - 1)
    i0 = np.floor(f).astype(np.int64)
    a = (f - i0.astype(np.float32)).astype(np.float32)
    i0[lo], a[lo] = 0, 0
    i0[hi], a[hi] = n - 1, 0
    return i0, np.minimum(i0 + 1, n - 1), a


def _lerp(img, ty, tx):
    (y0, y1, ay), (x0, x1, ax) = ty, tx
    ay, ax = ay[:, None, None], ax[None, :, None]
    one = np.float32(1)
    r0 = img[y0][:, x0] * (one - ax) + img[y0][:, x1] * ax
    r1 = img[y1][:, x0] * (one - ax) + img[y1][:, x1] * ax
    return r0 * (one - ay) + r1 * ay


def ref_augment(src, dst, flow, p, h, w):
    """numpy float32 restatement of include/mpiflow_hip.h's mpf_augment_pairs, in the kernel's operation order"""
    H, W = src.shape[:2]
    yy, xx = p["y0"] + np.arange(h), p["x0"] + np.arange(w)
    if p["flip_h"]:
        xx = p["Wr"] - 1 - xx
    if p["flip_v"]:
        yy = p["Hr"] - 1 - yy
    if not p["resize"]:
        i1, i2, f = src[yy][:, xx].astype(np.float32), dst[yy][:, xx].astype(np.float32), flow[yy][:, xx].copy()
    else:
        ty, tx = _taps(yy, H, p["scale_y"]), _taps(xx, W, p["scale_x"])
        i1 = np.clip(np.rint(_lerp(src.astype(np.float32), ty, tx)), 0, 255)
        i2 = np.clip(np.rint(_lerp(dst.astype(np.float32), ty, tx)), 0, 255)
        f = _lerp(flow, ty, tx)
        f = np.stack([(f[..., 0].astype(np.float64) * p["scale_x"]).astype(np.float32), (f[..., 1].astype(np.float64) * p["scale_y"]).astype(np.float32)], -1)
    if p["flip_h"]:
        f[..., 0] = -f[..., 0]
    if p["flip_v"]:
        f[..., 1] = -f[..., 1]
    valid = ((np.abs(f[..., 0]) < 1000) & (np.abs(f[..., 1]) < 1000)).astype(np.float32)
    return i1[..., ::-1].transpose(2, 0, 1), i2[..., ::-1].transpose(2, 0, 1), f.transpose(2, 0, 1), valid


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,h,w,B", [(37, 53, 17, 25, 5), (48, 64, 30, 40, 16), (61, 259, 33, 157, 3), (40, 300, 40, 300, 2)])
def test_augment_kernel_is_bit_exact_against_the_contract(dev, H, W, h, w, B):
    from mpiflow_amd import ops
    rs = np.random.RandomState(H * 1000 + W)
    src = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    dst = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    flow = ((rs.rand(B, H, W, 2) - 0.5) * 2400).astype(np.float32)
    lo = max(h / H, w / W) + 0.02
    params = []
    for b in range(B):
        p = dict(resize=0, scale_x=1.0, scale_y=1.0, Hr=H, Wr=W, flip_h=int(rs.rand() < 0.5), flip_v=int(rs.rand() < 0.5), y0=0, x0=0)
        if (H, W) != (h, w) and (b < 2 or rs.rand() < 0.8):
            sx, sy = rs.uniform(lo, 2.2), rs.uniform(lo, 2.2)
            if b == 0:
                sx, sy = lo + 0.03, lo + 0.01                                  # both axes shrink
            elif b == 1:
                sx, sy = 1.9, 1.3                                              # both grow, stretched
            p.update(resize=1, scale_x=float(sx), scale_y=float(sy), Hr=int(np.rint(H * sy)), Wr=int(np.rint(W * sx)))
        ymax, xmax = p["Hr"] - h, p["Wr"] - w
        p["y0"], p["x0"] = [(rs.randint(0, ymax + 1), rs.randint(0, xmax + 1)), (0, 0), (ymax, xmax), (0, xmax), (ymax, 0)][b % 5]   # all four edges
        params.append(p)
    T = lambda a: torch.from_numpy(a).to(dev)                                # noqa: E731
    s_d, d_d, f_d = T(src), T(dst), T(flow)
    out = ops.augment_pairs([dict(src=s_d[b], dst=d_d[b], flow=f_d[b], **params[b]) for b in range(B)], size=(h, w))
    torch.cuda.synchronize()
    for b in range(B):
        want = ref_augment(src[b], dst[b], flow[b], params[b], h, w)
        for k, ref in zip(("image1", "image2", "flow", "valid"), want):
            assert _bits(out[k][b].cpu().numpy(), ref) == 0, (k, b, params[b])


@pytest.mark.gpu
def test_augment_kernel_identity_and_every_scale_regime(dev):
    from mpiflow_amd import ops
    rs = np.random.RandomState(1)
    H, W = 23, 71
    src = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    dst = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    flow = rs.randn(H, W, 2).astype(np.float32) * 300
    T = lambda a: torch.from_numpy(a).to(dev)                                # noqa: E731
    out = ops.augment_pairs([dict(src=T(src), dst=T(dst), flow=T(flow))] * 2)
    torch.cuda.synchronize()
    for b in range(2):
        assert _bits(out["image1"][b].cpu().numpy(), src[..., ::-1].transpose(2, 0, 1).astype(np.float32)) == 0
        assert _bits(out["image2"][b].cpu().numpy(), dst[..., ::-1].transpose(2, 0, 1).astype(np.float32)) == 0
        assert _bits(out["flow"][b].cpu().numpy(), flow.transpose(2, 0, 1)) == 0
    cases = [(0.5, 0.5), (0.731, 1.37), (1.0, 1.0), (2.0, 3.0), (1.61, 0.93)]
    ps = []
    for sx, sy in cases:
        Hr, Wr = int(np.rint(H * sy)), int(np.rint(W * sx))
        ps.append(dict(resize=1, scale_x=sx, scale_y=sy, Hr=Hr, Wr=Wr, flip_h=int(sx > 1), flip_v=int(sy > 1), y0=Hr - 11, x0=Wr - 35))
    out = ops.augment_pairs([dict(src=T(src), dst=T(dst), flow=T(flow), **p) for p in ps], size=(11, 35))
    torch.cuda.synchronize()
    for b, p in enumerate(ps):
        for k, ref in zip(("image1", "image2", "flow", "valid"), ref_augment(src, dst, flow, p, 11, 35)):
            assert _bits(out[k][b].cpu().numpy(), ref) == 0, (k, p)


def _run_cli(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gen_3dphoto_dynamic.py")] + args, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]


def _samples(src, epochs=1):
    out = []
    for _ in range(epochs):
        for batch in src:
            torch.cuda.synchronize()
            for b, m in enumerate(batch["meta"]):
                out.append((m, {k: batch[k][b].cpu().numpy() for k in ("image1", "image2", "flow", "valid")}))
    return out


def _compare_with_files(samples, out_dir, names_in_order, R, count=None):
    from PIL import Image
    from mpiflow_amd import io_formats
    want = [(n, r) for n in names_in_order for r in range(R)][:count]
    assert [(m[0], m[1]) for m, _ in samples] == want
    for (m, s) in samples:
        stem = "%s_%d" % (m[0], m[1])
        im1 = np.array(Image.open(os.path.join(out_dir, "src_images", stem + ".png")).convert("RGB"))
        im2 = np.array(Image.open(os.path.join(out_dir, "dst_images", stem + ".png")).convert("RGB"))
        flo = io_formats.read_flo(os.path.join(out_dir, "flows", stem + ".flo"))
        assert _bits(s["image1"], im1.transpose(2, 0, 1).astype(np.float32)) == 0, stem
        assert _bits(s["image2"], im2.transpose(2, 0, 1).astype(np.float32)) == 0, stem
        assert _bits(s["flow"], flo.transpose(2, 0, 1)) == 0, stem
        assert (s["valid"] == ((np.abs(flo[..., 0]) < 1000) & (np.abs(flo[..., 1]) < 1000))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("fill,inpaint", [("peel", "hip"), ("builtin", "builtin")])
def test_online_equals_the_cli_files_disparity_producer(dev, tmp_path, fill, inpaint):
    from mpiflow_amd.online import OnlinePairs
    names = ["b0", "b1", "b2", "b3"]
    _toy_dataset(tmp_path / "data", names, empty_mask=("b2",))
    _run_cli(["--base", str(tmp_path / "data"), "--out", str(tmp_path / "out"), "--width", "64", "--height", "48", "--repeat", "2", "--planes", "16",
              "--inpaint", inpaint, "--mpi-from", "disparity", "--seed", "7"])
    with OnlinePairs(str(tmp_path / "data"), batch_size=2, crop=None, width=64, height=48, seed=7, pairs_per_image=2, mpi_from="disparity", planes=16,
                     fill=fill, augment=None, shuffle=False, mix=0, prefetch=2, device=dev) as src:
        samples = _samples(src)
        assert src.skipped and src.skipped[0][0] == "b2"
    _compare_with_files(samples, tmp_path / "out", ["b0", "b1", "b3"], 2)


@pytest.mark.gpu
def test_online_equals_the_cli_files_hip_network(dev, tmp_path):
    from mpiflow_amd.online import OnlinePairs
    names = ["c0", "c1"]
    _toy_dataset(tmp_path / "data", names, size=(96, 120))
    _run_cli(["--base", str(tmp_path / "data"), "--out", str(tmp_path / "out"), "--width", "128", "--height", "128", "--repeat", "2", "--planes", "8",
              "--ckpt_path", "random:3", "--inpaint", "builtin", "--seed", "11"])
    with OnlinePairs(str(tmp_path / "data"), batch_size=3, crop=None, width=128, height=128, seed=11, pairs_per_image=2, mpi_from="model",
                     ckpt_path="random:3", planes=8, fill="builtin", augment=None, shuffle=False, mix=0, device=dev) as src:
        samples = _samples(src)
    assert len(samples) == 3                                                  # 4 pairs, batches of 3: the fourth waits for the next epoch
    _compare_with_files(samples, tmp_path / "out", ["c0", "c1"], 2, count=3)


def _disp_source(base, dev, **kw):
    from mpiflow_amd.online import OnlinePairs
    args = dict(batch_size=2, crop=None, width=64, height=48, seed=5, pairs_per_image=2, mpi_from="disparity", planes=16, fill="peel", augment=None,
                shuffle=False, mix=0, device=dev)
    args.update(kw)
    return OnlinePairs(str(base), **args)


@pytest.mark.gpu
def test_two_ranks_yield_the_samples_of_one(dev, tmp_path):
    names = ["d%d" % i for i in range(5)]
    _toy_dataset(tmp_path, names, empty_mask=("d3",))
    got = {}
    for rank in range(2):
        with _disp_source(tmp_path, dev, batch_size=1, rank=rank, world_size=2) as src:
            for m, s in _samples(src):
                assert int(m[0][1:]) % 2 == rank
                got[(m[0], m[1])] = s
    with _disp_source(tmp_path, dev, batch_size=1, rank=0, world_size=1) as src:
        one = _samples(src)
    assert sorted(got) == sorted((m[0], m[1]) for m, _ in one) and len(one) == 8
    for m, s in one:
        for k in s:
            assert _bits(s[k], got[(m[0], m[1])][k]) == 0


def _aug_source(base, dev, **kw):
    args = dict(batch_size=3, crop=(40, 56), fill="builtin", augment=dict(min_scale=-0.2, max_scale=0.5, do_flip=True), shuffle=True, mix=5)
    args.update(kw)
    return _disp_source(base, dev, **args)


def _flat(samples):
    return [(m, [s[k] for k in ("image1", "image2", "flow", "valid")]) for m, s in samples]


def _same(a, b):
    assert len(a) == len(b)
    for (ma, sa), (mb, sb) in zip(a, b):
        assert ma == mb
        for x, y in zip(sa, sb):
            assert _bits(x, y) == 0


@pytest.mark.gpu
def test_batches_do_not_depend_on_prefetch_or_fill_pool_and_resume_exactly(dev, tmp_path):
    names = ["e%d" % i for i in range(6)]
    _toy_dataset(tmp_path, names, empty_mask=("e4",))
    with _aug_source(tmp_path, dev, prefetch=1, fill_threads=2) as a:
        ea1, ea2 = _flat(_samples(a)), _flat(_samples(a))
    with _aug_source(tmp_path, dev, prefetch=4, fill_threads=5) as b:
        eb1, eb2 = _flat(_samples(b)), _flat(_samples(b))
    _same(ea1, eb1)
    _same(ea2, eb2)
    assert len(ea1) >= 6 and [m for m, _ in ea1] != [m for m, _ in ea2]
    assert any(m[3] != 1.0 for m, _ in ea1) and any(m[5] for m, _ in ea1)        # resized and flipped samples among them
    # resume after k batches
    k = 2
    with _aug_source(tmp_path, dev, prefetch=3) as c:
        it = iter(c)
        for _ in range(k):
            next(it)
        st = c.state_dict()
    with _aug_source(tmp_path, dev, prefetch=2) as d:
        d.load_state_dict(st)
        rest = _flat(_samples(d)) + _flat(_samples(d))
    _same(rest, (ea1 + ea2)[3 * k:])


@pytest.mark.gpu
def test_batches_on_a_side_stream_equal_synchronised_ones_and_global_rng_untouched(dev, tmp_path):
    names = ["f%d" % i for i in range(4)]
    _toy_dataset(tmp_path, names)
    random.seed(1)
    np.random.seed(2)
    torch.manual_seed(3)
    g = (random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state(dev))
    with _aug_source(tmp_path, dev, prefetch=2) as a:
        ref = _flat(_samples(a))
    side = torch.cuda.Stream(device=dev)
    got = []
    with _aug_source(tmp_path, dev, prefetch=3) as b, torch.cuda.stream(side):
        for batch in b:
            copies = {k: batch[k] * 1.0 for k in ("image1", "image2", "flow", "valid")}       # consumed on `side`, no synchronisation
            got.append((batch["meta"], copies))
        host = [(meta, {k: v.cpu() for k, v in c.items()}) for meta, c in got]
    flat = []
    for meta, c in host:
        for i, m in enumerate(meta):
            flat.append((m, [c[k][i].numpy() for k in ("image1", "image2", "flow", "valid")]))
    _same(flat, ref)
    assert random.getstate() == g[0]
    st = np.random.get_state()
    assert (st[1] == g[1][1]).all() and st[2:] == g[1][2:]
    assert torch.equal(torch.get_rng_state(), g[2]) and torch.equal(torch.cuda.get_rng_state(dev), g[3])
