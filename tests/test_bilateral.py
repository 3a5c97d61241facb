"""ops.sparse_bilateral_filter (mpf_bilateral.hip), the sparse bilateral filter of the reference's bilateral_filter.py, against

golden     tests/golden/bilateral.npz: the reference's own outputs (make_bilateral_golden.py).  The filter's output is a selection of input
           values, so every comparison is bit for bit; there is no tolerance anywhere in this file.
restated   tests/bilateral_restated.py, INTEGRATION.md section 18 in numpy: it must give the goldens (CPU), and the kernel must give what it
           gives at shapes the goldens do not cover.

A missing golden is a failure: np.load, not conftest's load_golden (which skips)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bilateral_restated as R  # noqa: E402
from conftest import bits_equal  # noqa: E402

SHAPES = ("23x29", "9x40")
WINDOWS = ((3,), (5, 5), (7, 5, 3), (9,))
DTYPES = ("f64", "f32", "u8")


def same(a, b):
    return bits_equal(a, b) == 0


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "bilateral.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def grid_cases():
    """(name of the output, name of the input, windows, name of the mask or None) of every golden case"""
    out = []
    for shape in SHAPES:
        for dt in DTYPES:
            for ws in WINDOWS:
                for mk in (None, "mask_" + shape):
                    out.append(("out_%s_%s_w%s%s" % (dt, shape, "".join(map(str, ws)), "_mask" if mk else ""), "in_%s_%s" % (dt, shape), ws, mk))
    out += [("out_ramp_w5", "in_ramp", (5,), None), ("out_small_w9", "in_small", (9,), None), ("out_zeroblock_w55", "in_zeroblock", (5, 5), None)]
    return out


CASES = grid_cases()


# ---------------------------------------------------------------- CPU

def test_the_golden_holds_every_case(golden):
    assert len(CASES) == 51
    for name, src, ws, mk in CASES:
        assert name in golden and src in golden and (mk is None or mk in golden), name
        assert golden[name].dtype == golden[src].dtype and golden[name].shape == golden[src].shape


def test_the_restatement_equals_every_golden_bit_for_bit(golden):
    for name, src, ws, mk in CASES:
        x, mask = golden[src], None if mk is None else golden[mk]
        got = R.restated_u8(x, ws, mask=mask)[1] if x.dtype == np.uint8 else R.sparse_bilateral_restated(x, ws, mask=mask)
        assert same(got, golden[name]), name


def test_the_ramp_isolates_the_ring_rule(golden):
    x, y = golden["in_ramp"], golden["out_ramp_w5"]
    assert same(y, np.pad(x[1:-1, 1:-1], 1, "edge")) and not same(y, x)


def test_kstar_is_not_the_plain_median_rank():
    odd = [n for n in range(1, 82) if R.kstar(n) != n // 2 + 1]
    assert odd and all(n % 2 == 0 and R.kstar(n) == n // 2 for n in odd)          # an even n whose float32 half sum lands on 0.5 or below
    assert all(R.kstar(n) == n // 2 + 1 for n in range(1, 82, 2))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


def test_the_library_s_rank_table_equals_its_definition_in_numpy_float32(built):
    lib = built.load()
    for n in range(1, 82):
        c = np.float32(1) / np.float32(n)
        s, k = np.float32(0), 1
        for _ in range(n):
            s = np.float32(s + c)
            k += int(s <= np.float32(0.5))
        assert lib.mpf_sparse_bilateral_rank(n) == k == R.kstar(n), n
    assert lib.mpf_sparse_bilateral_rank(0) == 0 and lib.mpf_sparse_bilateral_rank(82) == 0


def test_the_c_entry_points_validate_before_they_launch(built):
    import ctypes
    lib = built.load()
    a = built.MpfBilateralArgs()
    assert lib.mpf_sparse_bilateral(None, None) != 0 and b"null argument block" in lib.mpf_last_error()
    assert lib.mpf_sparse_bilateral(ctypes.byref(a), None) != 0
    assert lib.mpf_sparse_bilateral_workspace(0, 1, 2, 9) == 0 and lib.mpf_sparse_bilateral_workspace(3, 1, 9, 9) == 0
    assert lib.mpf_sparse_bilateral_workspace(1, 2, 5, 7) == 2 * 560 + 70 and lib.mpf_sparse_bilateral_workspace(2, 1, 5, 7) == 2 * 48 + 35
    a.dtype, a.B, a.h, a.w, a.num_iter = 0, 1, 8, 8, 1
    a.filter_size[0] = 4
    assert lib.mpf_sparse_bilateral(ctypes.byref(a), None) != 0 and b"filter_size[0] must be 3, 5, 7 or 9 (got 4)" in lib.mpf_last_error()
    a.filter_size[0], a.num_iter = 5, 9
    assert lib.mpf_sparse_bilateral(ctypes.byref(a), None) != 0 and b"num_iter" in lib.mpf_last_error()


def test_the_drop_in_refuses_what_it_does_not_support(built):
    from mpiflow_amd import bilateral_filter as bf
    x = np.ones((6, 6))
    with pytest.raises(built.MpiFlowHipError, match="range-weighted"):
        bf.bilateral_filter(x, 4.0, 0.5, 5)
    with pytest.raises(built.MpiFlowHipError, match="label=True"):
        bf.vis_depth_discontinuity(x, 0.04, label=True)
    overs = bf.vis_depth_discontinuity(np.array([[1, 1, 1, 1], [1, 1, 2, 1], [1, 1, 1, 1.0]]), 0.04)
    # 1 / depth is 0.5 at (1, 2) and 1 elsewhere: its four differences are over there, and the one to the right of (1, 1)
    assert [o[1].tolist() for o in overs] == [[0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 1, 0], [0, 1, 1, 0]]
    assert all(o.dtype == np.float32 and o.shape == (3, 4) and not o[0].any() and not o[2].any() for o in overs)


def test_disp_filter_is_parsed_and_off_by_default(built):
    import inspect
    from mpiflow_amd import online, producer
    from mpiflow_amd.utils import utils as U
    from mpiflow_amd.warpback import WarpBackStage1Dataset, WarpBackStage2Dataset
    assert producer.parse_disp_filter(None) is None and producer.parse_disp_filter("5,5") == (5, 5) and producer.parse_disp_filter([7, 5, 3]) == (7, 5, 3)
    for bad in ("4", "5,11", "x", (), [5] * 9):
        with pytest.raises(ValueError, match="disp_filter"):
            producer.parse_disp_filter(bad)
    for fn, key in ((producer.Lane.__init__, "disp_filter"), (online.OnlinePairs.__init__, "disp_filter"), (WarpBackStage1Dataset.__init__, "disp_filter"),
                    (WarpBackStage2Dataset.__init__, "disp_filter"), (U.disparity_to_tensor, "filter_size")):
        assert inspect.signature(fn).parameters[key].default is None
    import gen_3dphoto_dynamic as cli
    assert cli.parse(["--base", "b", "--out", "o"]).disp_filter is None and cli.parse(["--base", "b", "--out", "o", "--disp-filter", "5,5"]).disp_filter == "5,5"


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def dev(built):
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def run(dev, x, ws, mask=None, **kw):
    import torch
    from mpiflow_amd import ops
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return ops.sparse_bilateral_filter(t(x), list(ws), mask=t(mask), **kw).cpu().numpy()


@pytest.mark.gpu
def test_every_golden_case_is_bit_exact_in_all_three_dtypes(built, dev, golden):
    for name, src, ws, mk in CASES:
        got = run(dev, golden[src], ws, None if mk is None else golden[mk])
        assert same(got, golden[name]), "%s: %d of %d values differ" % (name, bits_equal(got, golden[name]), got.size)


@pytest.mark.gpu
def test_the_u8_result_is_the_float64_result(built, dev, golden):
    for shape in SHAPES + ("zeroblock",):
        u8 = golden["in_zeroblock" if shape == "zeroblock" else "in_u8_" + shape]
        for ws in WINDOWS:
            for mask in (None,) if shape == "zeroblock" else (None, golden["mask_" + shape]):
                b = run(dev, u8, ws, mask)
                f = run(dev, u8.astype(np.float64) / 255.0, ws, mask)
                assert b.dtype == np.uint8 and same(b.astype(np.float64) / 255.0, f), (shape, ws)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(67, 131), (100, 150)])
def test_larger_shapes_equal_the_restatement(built, dev, h, w):
    u8 = R.blocky(h * w, h, w)
    mask = R.random_mask(h + w, h, w)
    for ws in ((5, 5), (7,), (7, 5)):
        for mk in (None, mask):
            f32 = (u8.astype(np.float64) / 255.0).astype(np.float32)
            assert same(run(dev, f32, ws, mk), R.sparse_bilateral_restated(f32, ws, mask=mk)), (ws, mk is None)
            assert same(run(dev, u8, ws, mk), R.restated_u8(u8, ws, mask=mk)[1]), (ws, mk is None)
    f64 = u8.astype(np.float64) / 251.0
    assert same(run(dev, f64, (7, 5), mask, depth_threshold=0.1), R.sparse_bilateral_restated(f64, (7, 5), 0.1, mask))
    assert same(run(dev, f64, (7, 5, 3), mask, num_iter=2), R.sparse_bilateral_restated(f64, (7, 5), mask=mask))


@pytest.mark.gpu
def test_a_batch_equals_its_single_calls(built, dev):
    import torch
    from mpiflow_amd import ops
    h, w = 37, 45
    frames = np.stack([R.blocky(s, h, w) for s in (1, 2, 3)])
    mask = R.random_mask(4, h, w)
    masks = np.stack([R.random_mask(s, h, w) for s in (5, 6, 7)])
    for x in (frames, (frames.astype(np.float64) / 255.0).astype(np.float32), frames.astype(np.float64) / 255.0):
        for mk in (None, mask, masks, mask != 0, (masks != 0).astype(np.uint8)):
            got = run(dev, x, (5, 5), mk)
            for i in range(3):
                one = run(dev, x[i], (5, 5), mk if mk is None or mk.ndim == 2 else mk[i])
                assert same(got[i], one), (x.dtype, i)
            assert same(run(dev, x[:, None], (5, 5), mk if mk is None or mk.ndim == 2 else mk[:, None])[:, 0], got)
    assert not same(run(dev, frames, (5, 5), mask), run(dev, frames, (5, 5)))
    # out and workspace handed in
    x = torch.from_numpy(frames).to(dev)
    out, ws = torch.empty_like(x), ops.sparse_bilateral_workspace(torch.uint8, 3, h, w, dev)
    assert ops.sparse_bilateral_filter(x, (5, 5), out=out, workspace=ws) is out and same(out.cpu().numpy(), run(dev, frames, (5, 5)))


@pytest.mark.gpu
def test_two_runs_give_the_same_bytes_and_a_side_stream_works(built, dev):
    import torch
    u8 = R.blocky(9, 67, 131)
    first = run(dev, u8, (7, 5, 3))
    assert same(first, run(dev, u8, (7, 5, 3))) and same(first, R.restated_u8(u8, (7, 5, 3))[1])
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        again = run(dev, u8, (7, 5, 3))
    s.synchronize()
    assert same(first, again)


@pytest.mark.gpu
def test_refusals_come_in_the_contract_s_order_and_name_the_value(built, dev):
    import torch
    from mpiflow_amd import ops
    E = built.MpiFlowHipError
    x = torch.zeros(8, 9, device=dev)
    cpu = torch.zeros(8, 9)
    for args, kw, msg in (
            ((np.zeros((8, 9)), [5]), {}, r"depth must be a torch.Tensor \(got ndarray\)"),
            ((cpu.half(), [4]), {}, r"depth must be float32 or float64 or uint8 \(got torch.float16\)"),      # dtype before the window, and before the device
            ((torch.zeros(2, 2, 8, 9), [4]), {}, r"got shape \(2, 2, 8, 9\)"),
            ((cpu.t(), [4]), {}, "contiguous"),
            ((cpu, [5]), dict(mask=torch.zeros(8, 9, dtype=torch.float64)), r"mask must be bool or uint8 or float32 \(got torch.float64\)"),
            ((cpu, [5]), dict(mask=torch.zeros(8, 8)), r"mask must be .*got shape \(8, 8\)"),
            ((cpu, [5]), dict(out=torch.zeros(8, 9, dtype=torch.float64)), r"out must be float32 \(got torch.float64\)"),
            ((cpu, [4]), {}, r"odd \(got 4 "),
            ((cpu, [5, 11]), {}, r"3, 5, 7 or 9 \(got 11 "),
            ((cpu, [1]), {}, r"3, 5, 7 or 9 \(got 1 "),
            ((torch.zeros(2, 9), [5]), {}, r"at least 3 rows and 3 columns \(got h, w = 2, 9\)"),
            ((cpu, [5, 5]), dict(num_iter=3), r"num_iter = 3 needs 3 windows, filter_size holds 2"),
            ((cpu, [5]), dict(depth_threshold=float("nan")), "NaN"),
            ((cpu, [5]), {}, r"depth must live on the GPU \(got cpu\)"),                                       # the device last
            ((x, [5]), dict(mask=torch.zeros(8, 9)), r"mask must live on the GPU"),
            ((x, [5]), dict(out=x), "out must not be depth itself"),
            ((x, [5]), dict(workspace=torch.empty(10, dtype=torch.uint8, device=dev)), r"workspace holds 10 bytes, \d+ needed")):
        with pytest.raises(E, match=msg):
            ops.sparse_bilateral_filter(*args, **kw)


@pytest.mark.gpu
def test_the_drop_in_module_and_the_loader_equal_the_golden(built, dev, golden, tmp_path):
    import torch
    from PIL import Image
    from mpiflow_amd import bilateral_filter as bf
    from mpiflow_amd.utils import utils as U
    for name, src, ws, mk in CASES[::5]:
        got = bf.sparse_bilateral_filtering(golden[src], filter_size=list(ws), mask=None if mk is None else golden[mk], num_iter=len(ws))
        assert isinstance(got, np.ndarray) and same(got, golden[name]), name
    x = golden["in_f32_23x29"]
    got = bf.sparse_bilateral_filtering(torch.from_numpy(x).to(dev), [5, 5])                                  # num_iter=None: len(filter_size)
    assert isinstance(got, torch.Tensor) and got.is_cuda and same(got.cpu().numpy(), golden["out_f32_23x29_w55"])
    # the reference's pipeline with its commented line live: cv2.imread(path, 0) / 255 -> the filter -> float32 [1,1,h,w]
    u8 = golden["in_u8_23x29"]
    path = str(tmp_path / "disp.png")
    Image.fromarray(u8).save(path)
    want = torch.from_numpy(golden["out_u8_23x29_w55"].astype(np.float64) / 255.0)[None, None].float()
    got = U.disparity_to_tensor(path, filter_size=[5, 5], num_iter=2)
    assert got.dtype == torch.float32 and got.shape == (1, 1, 23, 29) and torch.equal(got, want)
    assert torch.equal(U.disparity_to_tensor(path, unsqueeze=False), torch.from_numpy(u8.astype(np.float64) / 255)[None].float())


@pytest.mark.gpu
def test_lane_front_filters_the_uploaded_disparity_and_is_unchanged_without(built, dev):
    import torch
    from mpiflow_amd import ops, producer
    H, W, h, w = 48, 64, 37, 45
    rs = np.random.RandomState(3)
    item = dict(rgb_u8=torch.from_numpy(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)), disp_u8=torch.from_numpy(R.blocky(5, h, w)),
                ids_u8=torch.from_numpy(rs.randint(0, 3, (h, w)).astype(np.uint8)))
    d8 = item["disp_u8"].to(dev)
    filtered = ops.sparse_bilateral_filter(d8, (5, 5))
    assert not torch.equal(filtered, d8)
    for disp_filter, source in (((5, 5), filtered), ("5,5", filtered), (None, d8)):
        lane = producer.Lane(dev, H, W, 16, disp_filter=disp_filter)
        with torch.cuda.stream(lane.stream):
            lane.front(item)
        lane.stream.synchronize()
        want = ops.prepare_inputs(disp_u8=source, size=(H, W))["disp"]
        assert torch.equal(lane.inputs["disp"], want), disp_filter


class _Slice(object):
    """a stand-in generator: the first `n` channels of its input, through a sigmoid (any deterministic map of the right shape will do)"""

    def __init__(self, n):
        self.n = n

    def to(self, device):
        return self

    def eval(self):
        return self

    def __call__(self, x):
        import torch
        return torch.sigmoid(x[:, :self.n])


@pytest.mark.gpu
def test_the_warp_back_datasets_equal_the_unfiltered_path_fed_a_filtered_disparity(built, dev):
    import torch
    from mpiflow_amd import ops
    from mpiflow_amd.warpback import WarpBackStage1Dataset, WarpBackStage2Dataset
    b, h, w = 2, 32, 48
    rs = np.random.RandomState(8)
    image = torch.from_numpy(rs.rand(b, 3, h, w).astype(np.float32))
    disp = torch.from_numpy(np.stack([(np.clip(R.blocky(s, h, w), 1, 255).astype(np.float64) / 255.0).astype(np.float32) for s in (1, 2)])[:, None])
    pre = ops.sparse_bilateral_filter(disp.to(dev), (5, 5)).cpu()
    assert float((pre != disp).float().mean()) > 0.2
    root = os.path.join(HERE, "no_such_directory")
    for make in (lambda **kw: WarpBackStage1Dataset(root, width=w, height=h, device=dev, **kw),
                 lambda **kw: WarpBackStage2Dataset(root, width=w, height=h, device=dev, models=(_Slice(1), _Slice(3), _Slice(1)), **kw)):
        torch.manual_seed(5)
        got = make(disp_filter=(5, 5)).collect_data([(image[i], disp[i]) for i in range(b)])
        torch.manual_seed(5)
        want = make().collect_data([(image[i], pre[i]) for i in range(b)])
        torch.manual_seed(5)
        plain = make().collect_data([(image[i], disp[i]) for i in range(b)])
        assert got.keys() == want.keys()
        assert all(torch.equal(got[k], want[k]) for k in got), [k for k in got if not torch.equal(got[k], want[k])]
        assert any(not torch.equal(got[k], plain[k]) for k in got)
