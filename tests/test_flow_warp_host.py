"""CPU checks for the flow warps (mpiflow_amd.utils.transform): the golden tests/golden/flow_warp.npz is intact and keeps what
tests/golden/make_flow_warp_golden.py promises, tests/flow_warp_restated.py reproduces the reference's float64 values, get_flow and
gen_random_perspective equal the recorded reference bits, the C ABI declares the new calls and refuses bad arguments, and the module imports
without cv2."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flow_warp_restated as rs  # noqa: E402
import make_flow_warp_golden as mg  # noqa: E402

NEW_SYMBOLS = ("mpf_flow_warp", "mpf_flow_warp_bwd", "mpf_flow_warp_workspace")


@pytest.fixture(scope="module")
def gold():
    return load_golden("flow_warp")


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def fields(mode):
    return ("out", "mask", "grad_x", "grad_flow") if mode == "warp" else ("out", "grad_x", "grad_flow")


def test_golden_is_intact(gold):
    assert dict(mg.CASES) == {"b1_c1_5x7": (1, 1, 5, 7), "b2_c3_24x40": (2, 3, 24, 40), "b3_c2_33x65": (3, 2, 33, 65), "b1_c70_9x11": (1, 70, 9, 11)}
    for name, (B, C, H, W) in mg.CASES.items():
        assert gold[name + "/x"].shape == gold[name + "/g"].shape == (B, C, H, W) and gold[name + "/flow"].shape == (B, 2, H, W)
        assert gold[name + "/x"].dtype == gold[name + "/g"].dtype == gold[name + "/flow"].dtype == np.float32
        for mode in mg.MODES:
            k = "%s/%s/" % (name, mode)
            for f in fields(mode):
                assert gold[k + "ref32/" + f].dtype == gold[k + "d64/" + f].dtype == np.float32 and gold[k + "e_ref/" + f].dtype == np.float64
                assert gold[k + "ref32/" + f].shape == gold[k + "d64/" + f].shape
                assert 0 < float(gold[k + "e_ref/" + f]) < 1e-4
            assert gold[k + "ref32/out"].shape == (B, C, H, W) and gold[k + "ref32/grad_flow"].shape == (B, 2, H, W)
            assert (k + "ref32/mask" in gold) == (mode == "warp")
        assert gold[name + "/warp/ref32/mask"].shape == (B, 1, H, W)
    assert gold["rife/zero_flow/out"].shape == gold["rife/zero_flow/x"].shape == mg.ZERO_FLOW_SHAPE
    assert os.path.getsize(os.path.join(GOLDEN, "flow_warp.npz")) < 1 << 20


def test_cases_keep_clear_of_discrete_flips_and_reach_every_branch(gold):
    for name, (B, C, H, W) in mg.CASES.items():
        flow = gold[name + "/flow"]
        assert np.abs(flow[:, 0]).max() > W and np.abs(flow[:, 1]).max() > H                   # flows past the frame
        for mode, code in mg.MODES.items():
            p64 = rs.sample_positions(flow, code)
            p32 = rs.sample_positions(flow, code, np.float32)
            # (p32 uses numpy's linspace, the script torch's: an ulp apart, hence the 1 % of slack on the margin)
            assert not rs.near_flip(p64, code, H, W, 0.99 * mg.MARGIN).any() and not rs.near_flip(p32, code, H, W, 0.99 * mg.MARGIN).any(), (name, mode)
            for c32, c64 in zip(rs.cells(p32), rs.cells(p64)):
                assert (c32 == c64).all(), (name, mode)
            r = rs.flow_warp(gold[name + "/x"], flow, code)
            some = (r["mask"][:, 0] > 0) & ~r["all_in"]
            if mode == "warp":
                assert r["all_in"].any() and (r["mask"] == 0).any() and (some.any() or name == "b1_c1_5x7"), name
            else:
                assert p64["mx"].any() and (~p64["mx"]).any() and (~p64["my"]).any() and (p64["rx"] < 0).any() and (p64["rx"] > W - 1).any(), name
    assert mg.CASES["b1_c70_9x11"][1] > 64                                                       # more than one 64-channel chunk


def test_restatement_reproduces_the_float64_values(gold):
    for name in mg.CASES:
        for mode, code in mg.MODES.items():
            r = rs.flow_warp(gold[name + "/x"], gold[name + "/flow"], code, gold[name + "/g"])
            for f in fields(mode):
                f64 = rs.golden_f64(gold, name, mode, f)
                assert rel(r[f], f64) <= 1e-9, (name, mode, f)
                # the reference's own float32 run sits where e_ref says
                k = "%s/%s/" % (name, mode)
                assert rel(gold[k + "ref32/" + f].astype(np.float64), f64) == pytest.approx(float(gold[k + "e_ref/" + f]), rel=1e-5, abs=1e-12)
    z = rs.flow_warp(gold["rife/zero_flow/x"], np.zeros((mg.ZERO_FLOW_SHAPE[0], 2) + mg.ZERO_FLOW_SHAPE[2:], np.float32), rs.RIFE)
    assert np.abs(z["out"] - gold["rife/zero_flow/out"]).max() <= 1e-5


def test_mask_restated_is_one_where_every_tap_is_inside(gold):
    for name in mg.CASES:
        r = rs.flow_warp(gold[name + "/x"], gold[name + "/flow"], rs.WARP)
        assert np.abs(r["mask"][:, 0][r["all_in"]] - 1.0).max() <= 1e-12


def test_get_flow_and_gen_random_perspective_equal_the_reference_bits(gold):
    from mpiflow_amd.utils import transform as T
    for i, shape in enumerate(mg.GET_FLOW_SHAPES):
        assert tuple(gold["get_flow/%d/shape" % i]) == shape
        np.random.seed(9400 + i)
        M = T.gen_random_perspective()
        assert M.dtype == np.float64 and M.tobytes() == gold["get_flow/%d/M" % i].tobytes()
        flow = T.get_flow(np.zeros(shape, np.uint8), M)
        want = gold["get_flow/%d/flow" % i]
        assert flow.dtype == np.float32 and flow.shape == want.shape == (shape[0], shape[1], 2) and flow.tobytes() == want.tobytes()


def test_transform_raises_and_the_module_imports_without_cv2():
    import subprocess
    code = ("import sys; sys.modules['cv2'] = None\n"
            "import inspect, numpy as np\n"
            "import mpiflow_amd.utils.transform as T\n"
            "assert 'cv2' not in [m for m in sys.modules if sys.modules[m] is not None]\n"
            "assert list(inspect.signature(T.warp).parameters) == ['x', 'flo']\n"
            "assert list(inspect.signature(T.warp_rife).parameters) == ['tenInput', 'tenFlow']\n"
            "assert list(inspect.signature(T.get_flow).parameters) == ['img', 'M'] and list(inspect.signature(T.transform).parameters) == ['img', 'flow']\n"
            "try:\n    T.transform(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 2), np.float32))\n"
            "except NotImplementedError as e:\n    assert 'cv2.remap' in str(e)\nelse:\n    raise SystemExit('transform did not raise')\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_header_declares_the_new_calls_and_the_ctypes_table_mirrors_them():
    from mpiflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in _lib.SIGNATURES, n
    body = re.search(r"typedef struct MpfFlowWarpArgs \{(.*?)\} MpfFlowWarpArgs;", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s*]", "", part.split()[-1]) for part in decl.split(",")]
    assert names == [f[0] for f in _lib.MpfFlowWarpArgs._fields_]
    assert ctypes.sizeof(_lib.MpfFlowWarpArgs) == 10 * 8 + 8 + 6 * 4
    assert _lib.FLOW_WARP_CHUNK == int(re.search(r"#define MPF_FLOW_WARP_CHUNK (\d+)", hdr).group(1))
    assert (_lib.FLOW_WARP_WARP, _lib.FLOW_WARP_RIFE) == tuple(int(re.search(r"#define MPF_FLOW_WARP_%s (\d+)" % n, hdr).group(1)) for n in ("WARP", "RIFE"))
    assert "mpf_flow_warp.hip" in open(os.path.join(ROOT, "mpiflow_amd", "csrc", "Makefile")).read()


def test_library_refuses_bad_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    lib = _lib.load()
    assert lib.mpf_flow_warp(None, None) == 10001 and b"null argument block" in lib.mpf_last_error()
    assert lib.mpf_flow_warp_bwd(None, None) == 10001
    one = 256
    a = _lib.MpfFlowWarpArgs()
    a.x, a.flow, a.out, a.B, a.C, a.H, a.W, a.mode = one, one, one, 1, 3, 4, 1, _lib.FLOW_WARP_RIFE
    a.lin_w = a.lin_h = one
    assert lib.mpf_flow_warp(ctypes.byref(a), None) == 10001 and b"at least 2" in lib.mpf_last_error()
    a.W, a.mask = 4, one
    assert lib.mpf_flow_warp(ctypes.byref(a), None) == 10001 and b"no mask" in lib.mpf_last_error()
    a.mask, a.lin_w = None, None
    assert lib.mpf_flow_warp(ctypes.byref(a), None) == 10001 and b"lin_w" in lib.mpf_last_error()
    a.mode = 2
    assert lib.mpf_flow_warp(ctypes.byref(a), None) == 10001 and b"mode must be" in lib.mpf_last_error()
    a.mode, a.B = _lib.FLOW_WARP_WARP, 40000
    assert lib.mpf_flow_warp(ctypes.byref(a), None) == 10001 and b"bad shape" in lib.mpf_last_error()
    a.B, a.C, a.H, a.W = 1, 1 << 12, 1 << 10, 1 << 10
    assert lib.mpf_flow_warp(ctypes.byref(a), None) == 10001 and b"2^31" in lib.mpf_last_error()
    a.C, a.H, a.W, a.out = 70, 9, 11, None
    assert lib.mpf_flow_warp(ctypes.byref(a), None) == 10001 and b"(out)" in lib.mpf_last_error()
    a.grad_out = one
    assert lib.mpf_flow_warp_bwd(ctypes.byref(a), None) == 10001 and b"one gradient at least" in lib.mpf_last_error()
    a.grad_flow = one                                           # 70 channels = two chunks: their shares of grad_flow need the workspace
    assert lib.mpf_flow_warp_bwd(ctypes.byref(a), None) == 10001 and b"workspace" in lib.mpf_last_error()
    assert lib.mpf_flow_warp_workspace(1, 70, 9, 11, 0) == 2 * 1 * 2 * 9 * 11 * 4
    assert lib.mpf_flow_warp_workspace(1, 70, 9, 11, 1) == 0 and lib.mpf_flow_warp_workspace(2, 64, 9, 11, 0) == 0
    assert lib.mpf_flow_warp_workspace(0, 3, 9, 11, 0) == 0


def test_ops_refuse_before_launch_without_a_gpu():
    import torch
    from mpiflow_amd import _lib, ops
    from mpiflow_amd.utils import transform as T
    x, f = torch.zeros(2, 3, 4, 5), torch.zeros(2, 2, 4, 5)
    with pytest.raises(_lib.MpiFlowHipError, match="no CPU path"):
        T.warp(x, f)
    with pytest.raises(_lib.MpiFlowHipError, match=r"x must be float32.*\.float\(\)"):
        T.warp(x.double(), f)
    with pytest.raises(_lib.MpiFlowHipError, match=r"flow must be float32.*\.float\(\)"):
        T.warp_rife(x, f.half())
    with pytest.raises(_lib.MpiFlowHipError, match="flow must have x's batch size"):
        T.warp(x, f[:1])
    with pytest.raises(_lib.MpiFlowHipError, match=r"flow must be \[B,2,H,W\]"):
        T.warp(x, torch.zeros(2, 3, 4, 5))
    with pytest.raises(_lib.MpiFlowHipError, match="at least 2"):
        T.warp_rife(torch.zeros(2, 3, 4, 1), torch.zeros(2, 2, 4, 1))
    with pytest.raises(_lib.MpiFlowHipError, match="no mask"):
        ops.flow_warp(x, f, _lib.FLOW_WARP_RIFE, True)
    with pytest.raises(_lib.MpiFlowHipError, match="g_out must be"):
        ops.flow_warp_backward(x, f, torch.zeros(2, 3, 4, 6), _lib.FLOW_WARP_WARP)
    with pytest.raises(_lib.MpiFlowHipError, match="one gradient at least"):
        ops.flow_warp_backward(x, f, x, _lib.FLOW_WARP_WARP, want_x=False, want_flow=False)
