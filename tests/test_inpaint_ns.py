"""The GPU Navier-Stokes hole fill (mpf_inpaint_ns, mpiflow_amd/csrc/mpf_inpaint_ns.hip) and its fill method "ns-hip".

Host tests: the decomposition the kernel rests on - OpenCV's NS front run on each cluster of hole pixels (holes within Chebyshev distance
range + 1 of each other) alone gives the whole-frame bytes of mpf_inpaint_host - and a case where clusters linked at distance `range` only
do NOT (the bound is not vacuous); the C ABI's validation; the "ns-hip" method's plumbing.
GPU tests: byte identity with ops.inpaint_host frame by frame (goldens, the bench frame, edge cases, radii 1 - 4, batches on a side stream,
repeat calls), OnlinePairs(fill="ns-hip") == fill="builtin", and the CLI's --inpaint ns-hip files == --inpaint builtin's."""
import ctypes
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ops(lib):
    from mpiflow_amd import ops
    return ops


def clusters(mask, link):
    """label of every hole pixel (-1 elsewhere): connected components of the holes under "Chebyshev distance <= link" """
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    H, W = mask.shape
    idx = -np.ones((H, W), np.int64)
    ys, xs = np.nonzero(mask)
    idx[ys, xs] = np.arange(len(ys))
    a, b = [], []
    for dy in range(-link, link + 1):
        for dx in range(-link, link + 1):
            y2, x2 = ys + dy, xs + dx
            ok = (y2 >= 0) & (y2 < H) & (x2 >= 0) & (x2 < W)
            j = np.full(len(ys), -1)
            j[ok] = idx[y2[ok], x2[ok]]
            sel = j >= 0
            a.append(np.nonzero(sel)[0])
            b.append(j[sel])
    a, b = np.concatenate(a), np.concatenate(b)
    n, lab = connected_components(coo_matrix((np.ones(len(a)), (a, b)), shape=(len(ys), len(ys))), directed=False)
    out = -np.ones((H, W), np.int64)
    out[ys, xs] = lab
    return out, n


def per_cluster(ops, img, mask, radius, link):
    """the frame built from one inpaint_host run per cluster, each contributing its own hole pixels"""
    lab, n = clusters(mask, link)
    out = img.copy()
    for c in range(n):
        mc = (lab == c)
        out[mc] = ops.inpaint_host(img, mc.astype(np.uint8), radius, ops.INPAINT_NS)[mc]
    return out, n


def bench_frame(H=384, W=1280, seed=0):
    """tools/bench_inpaint_threads.py's frame: disocclusion bands + 1 % scattered pixels"""
    rs = np.random.RandomState(seed)
    img = (rs.rand(H, W, 3) * 255).astype(np.uint8)
    mask = np.zeros((H, W), np.uint8)
    for x0 in range(60, W, 160):
        mask[40:340, x0:x0 + 12] = 1
    mask |= (rs.rand(H, W) < 0.01).astype(np.uint8)
    return img, mask


def random_frame(rs, H, W, bands=3, p=0.01, border=False):
    img = (rs.rand(H, W, 3) * 255).astype(np.uint8)
    img = np.ascontiguousarray(np.cumsum(img.astype(np.int64), axis=1) % 256).astype(np.uint8)   # structure, so the gradients matter
    mask = (rs.rand(H, W) < p).astype(np.uint8)
    for _ in range(bands):
        y, x = rs.randint(0, H - 4), rs.randint(0, W - 3)
        mask[y:y + rs.randint(3, max(H // 2, 4)), x:x + rs.randint(2, 6)] = 1
    if border:
        mask[0, rs.randint(0, W):] = 1
        mask[:, W - 1][rs.rand(H) < 0.3] = 1
        mask[rs.randint(0, H), 0] = 1
        mask[H - 1, :rs.randint(1, W)] = 1
    return img, mask


# ---------------------------------------------------------------------------------------------------------------- host tests

@pytest.mark.parametrize("radius", [1, 2, 3, 4])
@pytest.mark.parametrize("border", [False, True])
def test_per_cluster_fronts_give_the_whole_frame(ops, radius, border):
    rs = np.random.RandomState(100 * radius + border)
    for _ in range(3):
        img, mask = random_frame(rs, 40, 56, bands=3, p=0.02, border=border)
        want = ops.inpaint_host(img, mask, radius, ops.INPAINT_NS)
        got, n = per_cluster(ops, img, mask, radius, radius + 1)
        assert n > 1
        assert (got == want).all()


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_link_distance_range_plus_one_links_range_plus_two_may_split(ops, radius):
    rs = np.random.RandomState(7 + radius)
    img = (rs.rand(24, 40, 3) * 255).astype(np.uint8)
    for gap, linked in ((radius + 1, True), (radius + 2, False)):
        mask = np.zeros((24, 40), np.uint8)
        mask[8:14, 10:13] = 1
        mask[11, 12 + gap] = 1                                  # Chebyshev distance `gap` from the block
        mask[10:12, 12 + gap:15 + gap] = 1
        lab, n = clusters(mask, radius + 1)
        assert (n == 1) == linked
        got, _ = per_cluster(ops, img, mask, radius, radius + 1)
        assert (got == ops.inpaint_host(img, mask, radius, ops.INPAINT_NS)).all()


def negative_control():
    """a frame where clusters linked at distance `range` (not range + 1) do not give the whole-frame bytes: two holes exactly range + 1 apart"""
    rs = np.random.RandomState(3)
    img = (rs.rand(20, 28, 3) * 255).astype(np.uint8)
    mask = np.zeros((20, 28), np.uint8)
    mask[6:14, 8:11] = 1
    mask[6:14, 14:17] = 1                                       # columns 10 and 14: distance 4 = range + 1 at radius 3
    return img, mask, 3


def test_link_distance_range_is_not_enough(ops):
    img, mask, radius = negative_control()
    want = ops.inpaint_host(img, mask, radius, ops.INPAINT_NS)
    split, n = per_cluster(ops, img, mask, radius, radius)
    assert n == 2
    assert (split != want).any()
    joined, n = per_cluster(ops, img, mask, radius, radius + 1)
    assert n == 1 and (joined == want).all()


def test_bench_frame_decomposes(ops):
    img, mask = bench_frame(96, 640)
    got, n = per_cluster(ops, img, mask, 3, 4)
    assert n > 50
    assert (got == ops.inpaint_host(img, mask, 3, ops.INPAINT_NS)).all()


def test_abi_symbols_and_validation(lib):
    cl = ctypes.CDLL(lib.LIB_PATH)
    wl = ctypes.CDLL(lib.WITNESS_PATH)
    for n in ("mpf_inpaint_ns", "mpf_inpaint_ns_workspace"):
        assert hasattr(cl, n) and hasattr(wl, n) and n in lib.SIGNATURES
    L = lib.load()
    B, H, W = 2, 8, 12
    need = L.mpf_inpaint_ns_workspace(B, H, W, 3.0)
    assert need >= B * (H + 2) * (W + 2) * 16
    img, mask, out, ws = (ctypes.c_void_p(a) for a in (1 << 20, 2 << 20, 3 << 20, 4 << 20))
    call = lambda **k: L.mpf_inpaint_ns(k.get("img", img), k.get("mask", mask), k.get("B", B), k.get("H", H), k.get("W", W),
                                        k.get("radius", 3.0), k.get("out", out), k.get("ws", ws), k.get("nws", need), None)
    assert call(radius=5.0) == 10002 and b"radius" in L.mpf_last_error()
    assert call(radius=4.6) == 10002
    assert call(H=1) == 10002 and call(W=1) == 10002
    assert call(H=0) == 10001
    assert call(out=ctypes.c_void_p((1 << 20) + 5)) == 10001 and b"alias" in L.mpf_last_error()
    assert call(out=mask) == 10001
    assert call(nws=need - 1) == 10001 and b"workspace" in L.mpf_last_error()
    assert call(img=None) == 10001


def test_ns_hip_method_plumbing():
    import gen_3dphoto_dynamic as gen
    from mpiflow_amd.utils import utils as U
    assert "ns-hip" in U.INPAINT_METHODS and U.resolve_inpaint("ns-hip") == "ns-hip"
    assert U.resolve_inpaint("auto") in ("cv2", "builtin")
    assert gen.parse(["--base", "b", "--out", "o", "--inpaint", "ns-hip"]).inpaint == "ns-hip"
    frame, hole = torch.zeros((4, 4, 3), dtype=torch.uint8), torch.zeros((4, 4), dtype=torch.uint8)
    with pytest.raises(ValueError, match="Telea"):
        U._inpaint(frame, hole, "ns-hip", algo="telea")


# ---------------------------------------------------------------------------------------------------------------- GPU tests

@pytest.fixture(scope="module")
def dev(lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib.load()
    return torch.device("cuda:0")


def gpu_fill(ops, dev, img, mask, radius=3):
    out = ops.inpaint_ns(torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev), radius)
    return out.cpu().numpy()


def _pair_fixtures():
    sys.path.insert(0, GOLDEN)
    import make_cv2_golden as mk
    return mk.PAIR_FIXTURES


@pytest.mark.gpu
@pytest.mark.parametrize("name", _pair_fixtures())
def test_gpu_equals_host_on_goldens(ops, dev, name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    img, mask = np.ascontiguousarray(g["frame_mix"]), np.ascontiguousarray(g["fill_mask"]).astype(np.uint8)
    assert mask.any()
    assert (gpu_fill(ops, dev, img, mask) == ops.inpaint_host(img, mask, 3, ops.INPAINT_NS)).all()


@pytest.mark.gpu
def test_gpu_equals_host_bench_frame(ops, dev):
    img, mask = bench_frame()
    assert (gpu_fill(ops, dev, img, mask) == ops.inpaint_host(img, mask, 3, ops.INPAINT_NS)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [1, 2, 3, 4, 0.4, 3.6])
def test_gpu_equals_host_radii_and_borders(ops, dev, radius):
    rs = np.random.RandomState(int(radius * 10))
    for shape, border in (((40, 56), False), ((37, 61), True), ((5, 300), True)):
        img, mask = random_frame(rs, *shape, bands=3, p=0.03, border=border)
        assert (gpu_fill(ops, dev, img, mask, radius) == ops.inpaint_host(img, mask, radius, ops.INPAINT_NS)).all(), (shape, border)


@pytest.mark.gpu
def test_gpu_edge_cases(ops, dev):
    rs = np.random.RandomState(5)
    img = (rs.rand(300, 40, 3) * 255).astype(np.uint8)
    band = np.zeros((300, 40), np.uint8)
    band[:, 14:26] = 1                                          # one 300 x 12 band touching the top and bottom rows
    cases = [(img, band), (img, np.zeros_like(band)), (img, np.ones_like(band))]
    tiny = (rs.rand(2, 2, 3) * 255).astype(np.uint8)
    cases += [(tiny, np.array([[1, 0], [0, 0]], np.uint8)), (tiny, np.array([[0, 1], [1, 0]], np.uint8)), (tiny, np.ones((2, 2), np.uint8))]
    for im, m in cases:
        want = ops.inpaint_host(im, m, 3, ops.INPAINT_NS)
        assert (gpu_fill(ops, dev, im, m) == want).all()
    assert (gpu_fill(ops, dev, img, np.ones_like(band)) == img).all()           # all hole: no band, nothing filled


@pytest.mark.gpu
def test_gpu_batch_on_a_side_stream_and_repeat_calls(ops, dev):
    rs = np.random.RandomState(11)
    H, W = 96, 160
    frames = [random_frame(rs, H, W, bands=4, p=0.01 * (b % 4), border=b % 2 == 1) for b in range(8)]
    img = np.stack([f[0] for f in frames])
    mask = np.stack([f[1] for f in frames])
    mask[3] = 0
    want = np.stack([ops.inpaint_host(img[b], mask[b], 3, ops.INPAINT_NS) for b in range(8)])
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ti, tm = torch.from_numpy(img).to(dev, non_blocking=True), torch.from_numpy(mask).to(dev, non_blocking=True)
        ws = torch.empty(ops.inpaint_ns_workspace(8, H, W), dtype=torch.uint8, device=dev)
        a = ops.inpaint_ns(ti, tm, 3, workspace=ws)
        b = ops.inpaint_ns(ti, tm, 3, workspace=ws)
        ha, hb = a.to("cpu", non_blocking=False), b.to("cpu", non_blocking=False)
    side.synchronize()
    assert (ha.numpy() == want).all()
    assert (hb.numpy() == ha.numpy()).all()


def _run_with_counters(ops, dev, img, mask, radius=3):
    ti, tm = torch.from_numpy(np.ascontiguousarray(img)).to(dev), torch.from_numpy(np.ascontiguousarray(mask)).to(dev)
    B, H, W = (1,) + mask.shape if mask.ndim == 2 else mask.shape
    ws = torch.empty(ops.inpaint_ns_workspace(B, H, W), dtype=torch.uint8, device=dev)
    out = ops.inpaint_ns(ti, tm, radius, workspace=ws).cpu().numpy()
    return out, ops.inpaint_ns_counters(ws)


def spill_at_start_frame():
    """one cluster whose band alone (about 2 490 pixels) outgrows the LDS heap (2 048 items): the heap starts in the global pool"""
    rs = np.random.RandomState(21)
    img = (rs.rand(16, 1280, 3) * 255).astype(np.uint8)
    mask = np.zeros((16, 1280), np.uint8)
    mask[6:10, 20:1260] = 1
    return img, mask


def spill_running_frame():
    """one cluster of 3-wide hole stripes with 1-pixel gaps: band about 1 670 pixels (fits LDS), but the front peaks near 2 700 items, so
    the heap moves from LDS to the pool while the front runs"""
    rs = np.random.RandomState(22)
    img = np.ascontiguousarray(np.cumsum((rs.rand(24, 308, 3) * 255).astype(np.int64), axis=0) % 256).astype(np.uint8)
    mask = np.zeros((24, 308), np.uint8)
    mask[4:20, 4:304] = 1
    mask[4:20, 7:304:4] = 0
    return img, mask


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["at_start", "running"])
def test_gpu_heap_spill_paths_equal_host(ops, dev, case):
    img, mask = spill_at_start_frame() if case == "at_start" else spill_running_frame()
    out, cnt = _run_with_counters(ops, dev, img, mask)
    assert cnt["failed"] == 0 and cnt["clusters"] == 1
    assert cnt["spilled_at_start"] == (case == "at_start") and cnt["spilled_running"] == (case == "running"), cnt
    assert (out == ops.inpaint_host(img, mask, 3, ops.INPAINT_NS)).all()


@pytest.mark.gpu
def test_gpu_spilling_and_lds_clusters_in_one_batch(ops, dev):
    """both spill paths beside clusters that stay in LDS, in one call: the pool regions of several clusters side by side"""
    a_img, a_mask = spill_at_start_frame()
    b_img, b_mask = spill_running_frame()
    H, W = 40, 1280
    img = np.zeros((3, H, W, 3), np.uint8)
    mask = np.zeros((3, H, W), np.uint8)
    rs = np.random.RandomState(23)
    img[:] = (rs.rand(3, H, W, 3) * 255).astype(np.uint8)
    img[0, :16], mask[0, :16] = a_img, a_mask
    img[0, 20:36, :1280] = a_img
    mask[0, 20:36] = a_mask                                     # a second spilling-at-start cluster in the same frame
    img[1, 8:32, 100:408], mask[1, 8:32, 100:408] = b_img, b_mask
    img[1, 8:32, 700:1008], mask[1, 8:32, 700:1008] = b_img, b_mask
    img[2], mask[2] = random_frame(rs, H, W, bands=6, p=0.02, border=True)
    out, cnt = _run_with_counters(ops, dev, img, mask)
    assert cnt["failed"] == 0 and cnt["spilled_at_start"] == 2 and cnt["spilled_running"] == 2, cnt
    for b in range(3):
        assert (out[b] == ops.inpaint_host(img[b], mask[b], 3, ops.INPAINT_NS)).all(), b


@pytest.mark.gpu
def test_gpu_bench_frame_counters(ops, dev):
    img, mask = bench_frame()
    out, cnt = _run_with_counters(ops, dev, img, mask)
    assert cnt["failed"] == 0 and cnt["spilled_at_start"] == 0 and cnt["spilled_running"] == 0
    assert cnt["clusters"] > 2000
    assert (out == ops.inpaint_host(img, mask, 3, ops.INPAINT_NS)).all()


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


@pytest.mark.gpu
def test_online_ns_hip_equals_builtin(dev, tmp_path):
    from mpiflow_amd.online import OnlinePairs
    _toy_dataset(tmp_path / "data", ["d0", "d1", "d2"])
    got = {}
    for fill in ("ns-hip", "builtin"):
        with OnlinePairs(str(tmp_path / "data"), batch_size=2, crop=(40, 56), width=64, height=48, seed=9, pairs_per_image=2, mpi_from="disparity",
                         planes=16, fill=fill, mix=4, prefetch=2, device=dev) as src:
            it = iter(src)
            batches = [next(it) for _ in range(2)]
            torch.cuda.synchronize()
            got[fill] = [{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in b.items()} for b in batches]
    for a, b in zip(got["ns-hip"], got["builtin"]):
        assert sorted(a) == sorted(b)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
            else:
                assert a[k] == b[k], k


@pytest.mark.gpu
def test_cli_ns_hip_files_equal_builtin(dev, tmp_path):
    _toy_dataset(tmp_path / "data", ["e0", "e1"])
    for inpaint in ("ns-hip", "builtin"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "gen_3dphoto_dynamic.py"), "--base", str(tmp_path / "data"),
                            "--out", str(tmp_path / inpaint), "--width", "64", "--height", "48", "--repeat", "2", "--planes", "16",
                            "--inpaint", inpaint, "--mpi-from", "disparity", "--seed", "7"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    n = 0
    for sub in ("flows", "dst_images", "src_images"):
        names = sorted(os.listdir(tmp_path / "builtin" / sub))
        assert names and names == sorted(os.listdir(tmp_path / "ns-hip" / sub))
        for f in names:
            assert filecmp.cmp(tmp_path / "builtin" / sub / f, tmp_path / "ns-hip" / sub / f, shallow=False), (sub, f)
            n += 1
    assert n == 3 * 4
