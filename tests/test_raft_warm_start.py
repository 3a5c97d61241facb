"""RAFT's warm start (ops.forward_interpolate / mpf_forward_interpolate of mpf_warm_start.hip, raft_eval.forward_interpolate,
RAFT.predict(warm_start=...), raft_eval.predict_sequence).

The operation has an exact definition (include/mpiflow_hip.h), so every comparison here is bit for bit and no
pixel is excluded anywhere:

golden   tests/golden/raft_warm_start.npz holds the output of the reference's own forward_interpolate (scipy's griddata, CPU) on seeded
         flows, recorded by tests/golden/make_warm_start_golden.py, which also asserted that on these inputs no target has two sources at
         the same least d2 and that the least and the second least differ by a relative 1e-9 or more: neither the tie rule nor a last-bit
         difference in d2 decides a pixel, so scipy's answer is THE answer.  A missing golden fails.
ties     where scipy defines nothing the rule is ours: the reference is restated() below, numpy's float64 d2 (each product and the sum
         rounded on its own) and argmin's first minimum over the valid sources in ascending flat index.
model    predict(warm_start=fl) against predict(flow_init=ops.forward_interpolate(fl)), predict_sequence against the hand-written loop: the
         same kernels on the same bytes, compared bit for bit under raft_train.reproducible() (the convolution library's deterministic
         algorithms) and after one unmeasured call (the first call of a convolution configuration in a process may pick another algorithm).
"""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "raft_warm_start.npz")
SYMBOLS = ("mpf_forward_interpolate", "mpf_forward_interpolate_workspace")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def raft(built):
    from mpiflow_amd import raft as module
    return module


@pytest.fixture(scope="module")
def raft_eval(built):
    from mpiflow_amd import raft_eval as module
    return module


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN, allow_pickle=False)                  # a missing file is an error here, not a skip
    mk = _load("make_warm_start_golden")
    g = dict(mk=mk, cases={}, min_gap=float(z["min_gap_required"]))
    for name in [str(n) for n in z["names"]]:
        N, h, w = [int(v) for v in z[name + "/settings"]]
        samples = [(str(k), float(p[0]), (float(p[1]), float(p[2])), int(p[3])) for k, p in zip(z[name + "/kinds"], z[name + "/params"])]
        flows = mk.case_inputs(h, w, samples)
        assert flows.dtype == np.float32 and flows.shape == (N, 2, h, w)
        assert flows.astype(np.float64).sum() == float(z[name + "/input_sum"]), "the seeded inputs of %s are not the recorded ones" % name
        g["cases"][name] = dict(name=name, N=N, h=h, w=w, samples=samples, flows=flows, out=z[name + "/out"], stats=z[name + "/valid_ties_gap"])
    return g


def restated(flow):
    """The rule, in numpy, for one sample [2,h,w] float32 -> [2,h,w] float32.  x1 = x0 + dx, y1 = y0 + dy in float64 (int64 + float32); valid
    iff 0 < x1 < w and 0 < y1 < h, all strict; per target the first minimum (np.argmin) of float64 d2 = ex * ex + ey * ey over the valid
    sources in ascending flat index; the selected source's two values copied; no valid source: zeros."""
    h, w = flow.shape[1:]
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    with np.errstate(invalid="ignore"):
        x1, y1 = (x0 + flow[0]).reshape(-1), (y0 + flow[1]).reshape(-1)
        valid = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)
    assert x1.dtype == np.float64
    idx = np.nonzero(valid)[0]
    if not len(idx):
        return np.zeros_like(flow)
    ex = x1[idx][None, :] - x0.reshape(-1, 1).astype(np.float64)
    ey = y1[idx][None, :] - y0.reshape(-1, 1).astype(np.float64)
    sel = idx[np.argmin(ex * ex + ey * ey, axis=1)]
    return flow.reshape(2, -1)[:, sel].reshape(2, h, w)


def tied_targets(flow):
    """the number of targets whose least d2 is reached by more than one valid source"""
    h, w = flow.shape[1:]
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    x1, y1 = (x0 + flow[0]).reshape(-1), (y0 + flow[1]).reshape(-1)
    idx = np.nonzero((x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h))[0]
    ex, ey = x1[idx][None, :] - x0.reshape(-1, 1), y1[idx][None, :] - y0.reshape(-1, 1)
    d2 = ex * ex + ey * ey
    return int(((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ no GPU needed


def test_golden_is_present_and_its_recorded_conditions_hold(golden):
    cases = golden["cases"]
    assert sorted(cases) == ["1x17x33", "1x47x156", "1x5x7", "2x16x24", "2x55x128"]
    assert golden["min_gap"] == 1e-9
    assert os.path.getsize(GOLDEN) < 200 * 1000
    kinds = set()
    for c in cases.values():
        assert c["out"].dtype == np.float32 and c["out"].shape == c["flows"].shape and np.isfinite(c["out"]).all()
        assert c["stats"].shape == (c["N"], 3)
        for flow, out, (nvalid, ties, gap), sample in zip(c["flows"], c["out"], c["stats"], c["samples"]):
            kinds.add(sample[0])
            hw = c["h"] * c["w"]
            assert ties == 0 and gap >= golden["min_gap"], (c["name"], ties, gap)
            assert nvalid == hw if c["name"] == "1x47x156" else 1 <= nvalid <= 0.9 * hw, (c["name"], nvalid)
            if hw <= 1024:                                   # the rule restated here agrees with the recorded reference (the recorder checked all)
                assert (words(restated(flow)) == words(out)).all(), c["name"]
                assert tied_targets(flow) == 0
            # every output vector is some source's vector
            src = set(zip(words(flow[0]).reshape(-1).tolist(), words(flow[1]).reshape(-1).tolist()))
            assert set(zip(words(out[0]).reshape(-1).tolist(), words(out[1]).reshape(-1).tolist())) <= src, c["name"]
    assert kinds == {"noise", "zoom"}
    assert abs(cases["2x16x24"]["stats"][0][0] / 384 - 0.8) < 0.06 and abs(cases["2x16x24"]["stats"][1][0] / 384 - 0.28) < 0.06


def test_restated_rule_on_the_documented_tie_cases():
    half = np.zeros((2, 6, 8), np.float32)
    half[0] = 0.5
    assert tied_targets(half) == 42                          # x1 = x0 + 0.5: every target but column 0's has two sources at 0.25
    out = restated(half)
    assert (out[0] == 0.5).all() and (out[1] == 0).all()
    zero = np.zeros((2, 5, 7), np.float32)
    assert (restated(zero) == 0).all()


def test_symbols_are_declared_bound_and_exported_and_validate_before_launching(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read(), flags=re.S)
    for path in (built.LIB_PATH, built.WITNESS_PATH):
        lib = ctypes.CDLL(path)
        for name in SYMBOLS:
            assert name in built.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name), name
    assert re.search(r"#define\s+MPF_WARM_MAX_HW\s+%d\b" % built.WARM_MAX_HW, hdr) and re.search(r"#define\s+MPF_WARM_MAX_NHW\s+%d\b" % built.WARM_MAX_NHW, hdr)
    lib = built.load()
    fn, size = lib.mpf_forward_interpolate, lib.mpf_forward_interpolate_workspace
    a = built.MpfWarmStartArgs()
    refused = lambda what: fn(ctypes.byref(a), None) == 10001 and what in lib.mpf_last_error()
    assert fn(None, None) == 10001 and b"null argument block" in lib.mpf_last_error()
    for shape in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        a.N, a.h, a.w = shape
        assert refused(b"bad shape") and size(*shape) == 0, shape
    # the limits: 135 x 240 (a 1080p frame's coarse grid) and 1 x 1 are accepted, h * w above MPF_WARM_MAX_HW is not
    assert built.WARM_MAX_HW >= 135 * 240
    for shape in ((1, 257, 256), (1, 1, 65537), (1, 65536, 65536), (65536, 1, 1), (65, 256, 256)):
        a.N, a.h, a.w = shape
        assert refused(b"bad shape") and size(*shape) == 0, shape
    a.N, a.h, a.w = 1, 135, 240
    assert refused(b"null pointer (flow or out)")
    a.flow, a.out = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    assert refused(b"out must not overlap flow")
    a.out = ctypes.c_void_p(1 << 24)
    assert refused(b"null pointer (workspace)")
    a.workspace = ctypes.c_void_p((1 << 28) + 4)
    assert refused(b"workspace must be 8-byte aligned")
    a.workspace = ctypes.c_void_p(1 << 28)
    need = size(1, 135, 240)
    assert need > 0 and need % 8 == 0 and need >= 12 * 135 * 240
    a.workspace_bytes = need - 8
    assert refused(b"workspace holds")
    # 12 bytes per target and source chunk; one chunk up to 256 sources, at most 32 chunks
    assert size(1, 1, 1) == 16 and size(1, 16, 16) == 12 * 256 and size(2, 5, 7) == 2 * 35 * 12
    assert size(1, 55, 128) == 28 * 7040 * 12 and size(1, 256, 256) == 32 * 65536 * 12 and size(64, 256, 256) == 64 * 32 * 65536 * 12
    a.N, a.h, a.w, a.workspace_bytes = 1, 1, 1, 8            # 1 x 1 itself is a shape the call takes: only its 16 bytes are missing
    assert refused(b"workspace holds 8 bytes, 16 needed")


def test_ops_forward_interpolate_refuses_in_the_order_of_the_contract_and_the_device_last(built, raft_eval):
    from mpiflow_amd import ops
    E = built.MpiFlowHipError
    z = torch.zeros
    with pytest.raises(E, match="flow must be a torch.Tensor"):
        ops.forward_interpolate(np.zeros((1, 2, 4, 4), np.float32))
    with pytest.raises(E, match="flow must be float32.*float64"):
        ops.forward_interpolate(z(1, 3, 4, 4, dtype=torch.float64))                        # the dtype before the shape
    with pytest.raises(E, match=r"flow must be \[N,2,h,w\]"):
        ops.forward_interpolate(z(1, 3, 4, 4))
    with pytest.raises(E, match=r"flow must be \[N,2,h,w\]"):
        ops.forward_interpolate(z(2, 4, 4))
    with pytest.raises(E, match="flow must be contiguous"):
        ops.forward_interpolate(z(1, 2, 4, 6).transpose(2, 3))
    with pytest.raises(E, match="out must be float32"):
        ops.forward_interpolate(z(1, 2, 4, 4), out=z(1, 2, 4, 4, dtype=torch.float16))
    with pytest.raises(E, match=r"out must be \[N,2,h,w\] like flow"):
        ops.forward_interpolate(z(1, 2, 4, 4), out=z(1, 2, 4, 5))
    with pytest.raises(E, match="at least one sample and one pixel"):
        ops.forward_interpolate(z(0, 2, 4, 4))
    with pytest.raises(E, match="brute force.*65536"):
        ops.forward_interpolate(z(1, 2, 257, 256))                                         # the limit before the device
    with pytest.raises(E, match="brute force"):
        ops.forward_interpolate(z(65, 2, 256, 256))
    with pytest.raises(E, match="flow must live on the GPU"):
        ops.forward_interpolate(z(1, 2, 135, 240))
    with pytest.raises(E, match="flow must live on the GPU"):
        ops.forward_interpolate(z(1, 2, 1, 1), out=z(1, 2, 1, 1))
    # upstream's name: [2,h,w] is one sample; anything else goes to the op as it is
    with pytest.raises(E, match="flow must live on the GPU"):
        raft_eval.forward_interpolate(z(2, 4, 4))
    with pytest.raises(E, match=r"flow must be \[N,2,h,w\]"):
        raft_eval.forward_interpolate(z(3, 4, 4))
    with pytest.raises(E, match="flow must be a torch.Tensor"):
        raft_eval.forward_interpolate(None)


def test_predict_refuses_flow_init_with_warm_start_and_a_warm_start_of_the_wrong_shape(raft, built):
    mk = _load("make_raft_eval_golden")
    E = built.MpiFlowHipError
    ok = torch.zeros(1, 3, 121, 131)                         # pads to 128 x 136: the coarse grid is 16 x 17
    low = torch.zeros(1, 2, 16, 17)
    for small in (False, True):
        model = raft.RAFT(mk.make_args(small)).eval()
        with pytest.raises(E, match="flow_init or warm_start, not both"):
            model.predict(ok, ok, flow_init=low, warm_start=low)
        with pytest.raises(E, match=r"warm_start must be \[N,2,Hp/8,Wp/8\]"):
            model.predict(ok, ok, warm_start=torch.zeros(1, 2, 15, 16))                     # H/8, W/8 of the unpadded frame
        with pytest.raises(E, match=r"warm_start must be \[N,2,Hp/8,Wp/8\]"):
            model.predict(ok, ok, warm_start=torch.zeros(2, 16, 17))
        with pytest.raises(E, match="warm_start must be float32"):
            model.predict(ok, ok, warm_start=low.double())
        with pytest.raises(E, match="warm_start must be a torch.Tensor"):
            model.predict(ok, ok, warm_start=low.numpy())
        with pytest.raises(E, match=r"flow_init must be \[N,2,Hp/8,Wp/8\]"):
            model.predict(ok, ok, flow_init=torch.zeros(1, 2, 15, 16), warm_start=low)      # a tensor's own fault before the pair's
        with pytest.raises(E, match="image1 must live on the GPU"):
            model.predict(ok, ok, warm_start=low)                                           # valid tensors on the CPU: the device, and only now
    import inspect
    assert inspect.signature(raft.RAFT.predict).parameters["warm_start"].default is None


# --------------------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_op(flows, dev):
    """ops.forward_interpolate on a numpy batch -> numpy"""
    from mpiflow_amd import ops
    got = ops.forward_interpolate(torch.from_numpy(np.ascontiguousarray(flows)).to(dev))
    assert got.dtype == torch.float32 and got.is_contiguous() and got.device == dev and tuple(got.shape) == flows.shape
    return got.cpu().numpy()


def check_restated(flows, dev, what):
    got = run_op(flows, dev)
    want = np.stack([restated(f) for f in flows])
    differ = int((words(got) != words(want)).sum())
    assert differ == 0, (what, "%d words differ from the restated rule" % differ)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1x5x7", "2x16x24", "1x17x33", "2x55x128", "1x47x156"])
def test_gpu_golden_bit_for_bit_and_the_same_bytes_twice(name, golden, built, dev):
    c = golden["cases"][name]
    runs = [run_op(c["flows"], dev) for _ in range(2)]
    differ = int((words(runs[0]) != words(c["out"])).sum())
    print("forward_interpolate %-9s %d of %d words differ from the recorded reference" % (name, differ, c["out"].size))
    assert differ == 0
    assert (words(runs[0]) == words(runs[1])).all(), "two runs differ"


@pytest.mark.gpu
def test_gpu_ties_go_to_the_lowest_flat_index(built, dev):
    half = np.zeros((1, 2, 6, 8), np.float32)
    half[:, 0] = 0.5
    assert tied_targets(half[0]) == 42
    check_restated(half, dev, "constant (0.5, 0) at 6 x 8")
    both = np.full((1, 2, 6, 8), 0.5, np.float32)
    assert tied_targets(both[0]) > 0
    check_restated(both, dev, "constant (0.5, 0.5) at 6 x 8")
    # the tied sources above carry one vector.  Ties between DISTINCT vectors: sources that land on the same point.  Pixel (x0, y0) and its right neighbour both land on x0 + 0.5 when
    # dx = 0.5 and -0.5; every target then has exact ties between two different vectors, and the lower flat index must win
    twin = np.zeros((1, 2, 6, 8), np.float32)
    twin[0, 0, :, 0::2], twin[0, 0, :, 1::2] = 0.5, -0.5
    twin[0, 1] = 0.25                                        # y1 = y0 + 0.25: inside the frame on every row
    assert tied_targets(twin[0]) == 48
    got = check_restated(twin, dev, "coincident sources at 6 x 8")
    assert (got[0, 0] == 0.5).all()                          # of each coincident pair the even column, the lower index
    # all-zero flow at 5 x 7: row 0 and column 0 are no sources (x1 > 0 and y1 > 0 are strict); their targets take a neighbour's zero
    zero = np.zeros((1, 2, 5, 7), np.float32)
    assert (check_restated(zero, dev, "zero flow at 5 x 7") == 0).all()
    # the same with distinct values planted: dx = 1e-3 in column 0 makes those pixels sources (of their own targets), exactly 0 does not,
    # so a kernel that took x1 >= 0 for valid would answer differently
    planted = np.zeros((1, 2, 5, 7), np.float32)
    planted[0, 1] = 0.125 * (1 + np.arange(35, dtype=np.float32).reshape(5, 7))           # dy tells the sources apart; row 0 becomes valid in y
    strict = check_restated(planted, dev, "zero dx at 5 x 7, distinct dy")
    # target (0, 0): with x1 >= 0 the source (0, 0) at y1 = 0.125 would be nearest (d2 = 0.0156); strictly it is (1, 0) at d2 = 1 + 0.25^2
    assert strict[0, 1, 0, 0] == planted[0, 1, 0, 1] != planted[0, 1, 0, 0]
    moved = planted.copy()
    moved[0, 0, :, 0] = 1e-3
    got = check_restated(moved, dev, "dx = 1e-3 in column 0")
    assert got[0, 1, 0, 0] == moved[0, 1, 0, 0] and got[0, 0, 0, 0] == np.float32(1e-3)
    assert (words(got) != words(strict)).any()


@pytest.mark.gpu
def test_gpu_degenerate_shapes_and_non_finite_values(golden, built, dev):
    one = np.full((1, 2, 1, 1), 0.5, np.float32)
    assert (words(check_restated(one, dev, "1 x 1, (0.5, 0.5)")) == words(one)).all()
    assert (words(run_op(np.zeros((1, 2, 1, 1), np.float32), dev)) == 0).all()            # no valid source: zeros, also no -0.0
    out = np.zeros((1, 2, 8, 8), np.float32)
    out[0, 0], out[0, 1] = 100.0, -100.0
    assert (words(check_restated(out, dev, "8 x 8, all out of frame")) == 0).all()
    # a batch where only the middle sample has no valid source
    mixed = np.concatenate([np.full((1, 2, 8, 8), 0.5, np.float32), out, np.full((1, 2, 8, 8), 0.25, np.float32)])
    got = check_restated(mixed, dev, "batch with one sample without a source")
    assert (got[1] == 0).all() and (got[0] == 0.5).all() and (got[2] == 0.25).all()
    # NaN and +-inf planted in a noise case, both channels non-finite at each plant: such a pixel is no source, so no NaN comes out
    c = golden["cases"]["1x17x33"]
    flows = c["flows"].copy()
    rs = np.random.RandomState(11)
    plants = rs.choice(17 * 33, 60, replace=False)
    for i, p in enumerate(plants):
        a, b = [(np.nan, np.nan), (np.inf, -np.inf), (-np.inf, np.nan), (np.nan, np.inf), (np.inf, np.inf), (-np.inf, -np.inf)][i % 6]
        flows[0, 0].reshape(-1)[p], flows[0, 1].reshape(-1)[p] = a, b
    got = check_restated(flows, dev, "17 x 33 with NaN and inf planted")
    assert np.isfinite(got).all()
    # one channel non-finite alone drops the pixel as well (x1 or y1 fails its comparison)
    flows = c["flows"].copy()
    flows[0, 0, 3, 4], flows[0, 1, 9, 20], flows[0, 0, 16, 32] = np.nan, np.inf, -np.inf
    assert np.isfinite(check_restated(flows, dev, "17 x 33 with one channel non-finite")).all()


@pytest.mark.gpu
def test_gpu_batch_is_the_samples_and_out_is_written_alone(golden, built, raft_eval, dev):
    from mpiflow_amd import ops
    c = golden["cases"]["2x16x24"]
    flows = np.concatenate([c["flows"], golden["cases"]["2x55x128"]["flows"][:, :, :16, :24]])
    batch = run_op(flows, dev)
    for n in range(len(flows)):
        assert (words(run_op(flows[n:n + 1], dev)) == words(batch[n:n + 1])).all(), n
    assert (words(batch[:2]) == words(c["out"])).all()
    # out= and the input inside one buffer of sentinels, at offsets that are no multiples of 16 bytes
    SENTINEL, GUARD = -12345.0, 37
    n = flows.size
    buf = torch.full((GUARD + n + GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    src = buf[GUARD:GUARD + n].view(flows.shape)
    src.copy_(torch.from_numpy(flows))
    out = buf[2 * GUARD + n:2 * GUARD + 2 * n].view(flows.shape)
    assert src.data_ptr() % 16 != 0 and out.data_ptr() % 16 != 0
    assert ops.forward_interpolate(src, out=out) is out
    host = buf.cpu().numpy()
    assert (words(host[2 * GUARD + n:2 * GUARD + 2 * n]) == words(batch).reshape(-1)).all()
    assert (words(host[GUARD:GUARD + n]) == words(flows).reshape(-1)).all(), "the input was written"
    for lo, hi in ((0, GUARD), (GUARD + n, 2 * GUARD + n), (2 * GUARD + 2 * n, 3 * GUARD + 2 * n)):
        assert (host[lo:hi] == SENTINEL).all(), "wrote outside out"
    # out overlapping flow is refused by the library, before anything is launched
    with pytest.raises(built.MpiFlowHipError, match="out must not overlap flow"):
        ops.forward_interpolate(src, out=src)
    # a non-contiguous input is refused, as the contract says (nothing is copied behind the caller's back)
    t = torch.from_numpy(flows).to(dev)
    with pytest.raises(built.MpiFlowHipError, match="flow must be contiguous"):
        ops.forward_interpolate(t.transpose(2, 3))
    with pytest.raises(built.MpiFlowHipError, match="flow must be contiguous"):
        ops.forward_interpolate(t[:, :, :, ::2])
    # upstream's shapes: [2,h,w] -> [2,h,w] on the device, the op's bytes; [N,2,h,w] as the op
    got = raft_eval.forward_interpolate(t[1])
    assert got.shape == (2, 16, 24) and got.device == dev and got.dtype == torch.float32
    assert (words(got.cpu().numpy()) == words(batch[1])).all()
    assert same_bytes(got[None].cuda(), torch.from_numpy(batch[1:2]).to(dev))              # upstream's `forward_interpolate(flow_low[0])[None].cuda()`
    assert same_bytes(raft_eval.forward_interpolate(t), torch.from_numpy(batch).to(dev))


def _model(raft, small, dev):
    mk = _load("make_raft_eval_golden")
    model = raft.RAFT(mk.make_args(small))
    mk.fill_params(model, 9950 + int(small))
    model.to(dev)
    model.freeze_bn()
    return model.eval(), mk


def _frames(mk, dev, count):
    """`count` frames [1,3,121,131]: the recorder's seeded image and shifted copies of it"""
    d = mk.eval_inputs(1, 121, 131, 9960)
    first = torch.from_numpy(d["image1"]).to(dev)
    return [torch.roll(first, shifts=(2 * i, -3 * i), dims=(2, 3)).contiguous() for i in range(count)]


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True], ids=["basic", "small"])
def test_gpu_predict_with_warm_start_is_predict_with_the_interpolated_flow_init(small, raft, built, dev):
    from mpiflow_amd import ops, raft_train
    model, mk = _model(raft, small, dev)
    a, b = _frames(mk, dev, 2)
    fl = torch.from_numpy((3.0 * np.random.RandomState(21).standard_normal((1, 2, 16, 17))).astype(np.float32)).to(dev)
    with raft_train.reproducible():
        model.predict(a, b, iters=4, flow_init=fl)           # unmeasured: see the module docstring
        want_low, want_up = model.predict(a, b, iters=4, flow_init=ops.forward_interpolate(fl))
        got_low, got_up = model.predict(a, b, iters=4, warm_start=fl)
        cold_low, _ = model.predict(a, b, iters=4)
    assert got_low.shape == (1, 2, 16, 17) and got_up.shape == (1, 2, 121, 131)
    assert same_bytes(got_low, want_low) and same_bytes(got_up, want_up)
    assert not same_bytes(got_low, cold_low), "warm_start was ignored"
    assert bool(torch.isfinite(got_up).all())


@pytest.mark.gpu
def test_gpu_predict_sequence_is_the_hand_written_loop(raft, raft_eval, built, dev):
    from mpiflow_amd import raft_train
    model, mk = _model(raft, True, dev)
    frames = _frames(mk, dev, 3)
    with raft_train.reproducible():
        model.predict(frames[0], frames[1], iters=4, flow_init=torch.zeros(1, 2, 16, 17, device=dev))    # unmeasured
        seq = raft_eval.predict_sequence(model, iter(frames), iters=4)
        assert iter(seq) is seq                              # a generator: nothing has run yet
        got = list(seq)
        prev, want = None, []
        for t in range(2):
            low, up = model.predict(frames[t], frames[t + 1], iters=4, mode="sintel", warm_start=prev)
            want.append((low, up))
            prev = low
        cold = list(raft_eval.predict_sequence(model, frames, iters=4, warm_start=False))
        alone = [model.predict(frames[t], frames[t + 1], iters=4) for t in range(2)]
    assert len(got) == 2 and all(isinstance(p, tuple) and len(p) == 2 for p in got)
    for t in range(2):
        assert got[t][0].shape == (1, 2, 16, 17) and got[t][1].shape == (1, 2, 121, 131) and got[t][0].device == dev
        assert same_bytes(got[t][0], want[t][0]) and same_bytes(got[t][1], want[t][1]), t
        assert same_bytes(cold[t][0], alone[t][0]) and same_bytes(cold[t][1], alone[t][1]), t
    assert same_bytes(got[0][1], cold[0][1])                 # the first pair has nothing to start from
    assert not same_bytes(got[1][1], cold[1][1]), "the second pair ignored its warm start"
    assert list(raft_eval.predict_sequence(model, frames[:1], iters=4)) == [] and list(raft_eval.predict_sequence(model, [], iters=4)) == []
