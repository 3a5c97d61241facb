"""CPU checks for the plane-adjustment network (MPIPredictor(adjust_planes=True), ops.pan_block1): tests/pan_restated.py - the factorisation the
kernel computes - reproduces the reference's recorded float64 first block on every case of tests/golden/pan.npz; the switch changes no state_dict
and, off, never runs the network; the torch path reproduces the reference's float32 run; every new refusal names its fault, the device last; the C
ABI declares, binds and exports the new calls and refuses bad arguments."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_pan_golden as mg  # noqa: E402
import pan_restated as rs  # noqa: E402

NEW_SYMBOLS = ("mpf_pan_block1", "mpf_pan_block1_workspace")


def load_pan_golden():
    """a missing golden FAILS (np.load raises): it is committed, and nothing here is worth a skip"""
    z = np.load(os.path.join(GOLDEN, "pan.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def gold():
    return load_pan_golden()


def seeded_dpn(S, seed):
    from mpiflow_amd.model.adampi import DepthPredictionNetwork
    dpn = DepthPredictionNetwork()
    psum = mg.fill_params(dpn, seed)
    return dpn.eval(), psum


def block1_params(dpn):
    return {k: v.double().numpy() for k, v in dpn.context_encoder.res_blocks[0].state_dict().items()}


def test_golden_is_intact_and_rebuilds_from_its_seeds(gold):
    assert list(gold["names"]) == list(mg.CASES) and os.path.getsize(os.path.join(GOLDEN, "pan.npz")) < 1 << 20
    sizes = {(c[2], c[3]) for c in mg.CASES.values()}
    assert sizes == {(32, 32), (33, 47), (40, 72)} and {c[1] for c in mg.CASES.values()} == {1, 5, 64} and {c[0] for c in mg.CASES.values()} == {1, 2}
    for name, (B, S, h, w, seed) in mg.CASES.items():
        assert tuple(gold[name + "/settings"]) == (B, S, h, w, seed)
        d = mg.case_inputs(B, S, h, w, seed)
        _, psum = seeded_dpn(S, seed)
        assert abs(sum(v.astype(np.float64).sum() for v in d.values()) + psum - float(gold[name + "/input_sum"])) < 1e-6, name
        n = B * S * 8 * (h // 2) * (w // 2)
        assert gold[name + "/block1_f64"].dtype == np.float64 and gold[name + "/block1_f64"].size == (n if n <= mg.FULL_MAX else mg.N_SAMPLE)
        assert gold[name + "/dpn_f64"].shape == gold[name + "/dpn_f32"].shape == (B, S)
        assert 0 < float(gold[name + "/block1_e_ref"]) < 1e-5 and 0 < float(gold[name + "/dpn_e_ref"]) < 1e-4
    assert any(B * S * 8 * (h // 2) * (w // 2) <= mg.FULL_MAX and h % 2 and w % 2 for B, S, h, w, _ in mg.CASES.values())   # an odd case kept whole


def test_restatement_equals_the_reference_float64_first_block(gold):
    """1e-12 relative on every case: the factorisation, the border sums, the halo rule; 33 x 47 proves the floor pooling (16 x 23 from 33 x 47)"""
    for name, (B, S, h, w, seed) in mg.CASES.items():
        d = mg.case_inputs(B, S, h, w, seed)
        dpn, _ = seeded_dpn(S, seed)
        got = rs.block1(d["rgb_low"], d["disp_low"], d["init_disp"], block1_params(dpn))
        assert got.shape == (B * S, 8, h // 2, w // 2)
        want = gold[name + "/block1_f64"]
        err = np.abs(mg.kept(got, seed) - want).max() / float(gold[name + "/block1_absmax"])
        print("%s: restated vs reference float64 %.2e" % (name, err))
        assert err <= 1e-12, (name, err)


def test_torch_path_reproduces_the_reference_float32_run(gold):
    """the module is the reference's function: its CPU float32 output sits where the reference's own float32 run sits"""
    for name in ("b1_s1_32x32", "b2_s5_33x47"):
        B, S, h, w, seed = mg.CASES[name]
        d = mg.case_inputs(B, S, h, w, seed)
        dpn, _ = seeded_dpn(S, seed)
        with torch.no_grad():
            out = dpn(*(torch.from_numpy(d[k]) for k in ("init_disp", "rgb_low", "disp_low"))).numpy()
        f64 = gold[name + "/dpn_f64"]
        assert np.abs(out - f64).max() / np.abs(f64).max() <= max(4 * float(gold[name + "/dpn_e_ref"]), 1e-6), name


def test_switch_changes_no_state_dict_and_off_never_runs_the_network(monkeypatch):
    from mpiflow_amd.model import MPIPredictor
    from mpiflow_amd.model.adampi import DepthPredictionNetwork
    off, on = MPIPredictor(128, 128, 3), MPIPredictor(128, 128, 3, adjust_planes=True)
    a, b = off.state_dict(), on.state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)
    assert off.adjust_planes is False and on.adjust_planes is True and MPIPredictor().adjust_planes is False
    calls = []
    real = DepthPredictionNetwork.forward
    monkeypatch.setattr(DepthPredictionNetwork, "forward", lambda self, *args: calls.append(1) or real(self, *args))
    on.load_state_dict(off.randomize_(3).state_dict())
    img, dsp = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(1)), torch.rand(1, 1, 128, 128, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        mpi, planes = off.eval()(img, dsp)
    assert calls == [] and torch.equal(planes, off.plane_disparities(img)) and torch.equal(planes[0], torch.linspace(1, 0.001, 5)[1:-1])
    with torch.no_grad():
        mpi_on, planes_on = on.eval()(img, dsp)
        again = on.dpn(on.plane_disparities(img), *(torch.nn.functional.interpolate(t, size=on.low_res_size, mode="bilinear", align_corners=True) for t in (img, dsp)))
    assert len(calls) == 2 and planes_on.shape == planes.shape and not torch.equal(planes_on, planes) and torch.equal(again, planes_on)
    assert mpi_on.shape == mpi.shape and not torch.equal(mpi_on, mpi)


def test_cpu_and_grad_calls_take_the_torch_path(monkeypatch):
    from mpiflow_amd import ops
    dpn, _ = seeded_dpn(5, 1)
    fused = []
    monkeypatch.setattr(ops, "pan_block1", lambda *a, **k: fused.append(1))
    x = (torch.rand(1, 5), torch.rand(1, 3, 32, 32), torch.rand(1, 1, 32, 32))
    assert not dpn.fused_block1_applies(*x)
    with torch.no_grad():
        dpn(*x)
    dpn.train()
    assert not dpn.fused_block1_applies(*x)
    assert fused == []


def test_refusals_name_their_fault_the_device_last():
    from mpiflow_amd import _lib, ops, producer
    from mpiflow_amd.model.planes import PerCallPlanes
    E = _lib.MpiFlowHipError
    f = torch.zeros
    good = dict(rgb_low=f(2, 3, 8, 8), disp_low=f(2, 1, 8, 8), plane_disp=f(2, 5), w1=f(8, 5, 3, 3), b1=f(8), bn_scale=f(8), bn_shift=f(8), w2=f(8, 8, 3, 3),
                b2=f(8), w3=f(8, 5, 1, 1), b3=f(8))
    for key, bad, match in (("rgb_low", None, "rgb_low must be a torch.Tensor"), ("rgb_low", f(2, 3, 8, 8).double(), r"rgb_low must be float32.*\.float\(\)"),
                            ("rgb_low", f(2, 4, 8, 8), r"rgb_low must be \[B,3,h,w\]"), ("disp_low", f(2, 1, 8, 9), r"disp_low must be \[B,1,h,w\]"),
                            ("disp_low", f(2, 1, 8, 16)[..., ::2], "disp_low must be contiguous"), ("plane_disp", f(3, 5), r"plane_disp must be \[B,S\]"),
                            ("w2", f(8, 5, 3, 3), "w2 must be"), ("b3", f(8).half(), "b3 must be float32"), ("rgb_low", f(2, 3, 1, 8), "h and w at least 2"),
                            ("plane_disp", f(2, 0), "at least one image and one plane"), ("out", f(10, 8, 4, 3), r"out must be \[B\*S,8,h//2,w//2\]")):
        with pytest.raises(E, match=match):
            args = dict(good, **{key: bad})
            if key == "rgb_low" and isinstance(bad, torch.Tensor) and bad.shape[2] == 1:
                args["disp_low"] = f(2, 1, 1, 8)
            ops.pan_block1(**args)
    with pytest.raises(E, match="rgb_low must live on the GPU"):            # every tensor is sound: only now the device
        ops.pan_block1(**good)

    class Planes(PerCallPlanes):
        _planes, _plane_disp, _planes_are_fixed = f(5), f(5), True
    p = Planes()
    p._set_planes(None)                                                      # the fixed planes: nothing to check, nothing copied
    for bad, match in ((np.zeros(5, np.float32), "plane_disp must be a torch.Tensor"), (f(5).double(), "plane_disp must be float32"),
                       (f(4), r"plane_disp must be \[S\] with the model's S = 5"), (f(1, 5), r"plane_disp must be \[S\]"), (f(10)[::2], "plane_disp must be contiguous"),
                       (f(5), "must live on the GPU")):
        with pytest.raises(E, match=match):
            p._set_planes(bad)
    assert p._planes_are_fixed
    producer.check_planes("img_7", torch.tensor([0.9, 0.5, 0.1]))
    for planes, k in ((torch.tensor([0.9, 0.5, -0.07]), 2), (torch.tensor([0.9, 0.0, 0.2]), 1), (torch.tensor([float("nan"), 0.5, 0.2]), 0)):
        with pytest.raises(producer.PlaneRefused, match=r"image img_7: plane %d of 3 has disparity .* after plane adjustment.*not rendered" % k):
            producer.check_planes("img_7", planes)


def test_the_switches_default_to_off():
    import inspect
    import gen_3dphoto_dynamic as cli
    from mpiflow_amd import online, producer
    from mpiflow_amd.model import MPIPredictor
    assert cli.parse(["--base", "b", "--out", "o"]).adjust_planes is False and cli.parse(["--base", "b", "--out", "o", "--adjust-planes"]).adjust_planes is True
    assert inspect.signature(online.OnlinePairs.__init__).parameters["adjust_planes"].default is False
    assert inspect.signature(producer.load_model).parameters["adjust_planes"].default is False
    assert inspect.signature(MPIPredictor.from_checkpoint).parameters["adjust_planes"].default is False
    assert list(inspect.signature(MPIPredictor.__init__).parameters)[1:] == ["width", "height", "num_planes", "adjust_planes"]
    with pytest.raises(SystemExit, match="--adjust-planes .* --mpi-from model"):
        cli.main(["--base", "b", "--out", "o", "--adjust-planes", "--mpi-from", "disparity"])


def test_header_declares_the_new_calls_and_the_ctypes_table_mirrors_them():
    from mpiflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in _lib.SIGNATURES, n
    body = re.search(r"typedef struct MpfPanArgs \{(.*?)\} MpfPanArgs;", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s*]", "", part.split()[-1]) for part in decl.split(",")]
    assert names == [f[0] for f in _lib.MpfPanArgs._fields_]
    assert ctypes.sizeof(_lib.MpfPanArgs) == 13 * 8 + 8 + 4 * 4
    assert _lib.PAN_C == int(re.search(r"#define MPF_PAN_C (\d+)", hdr).group(1))
    assert _lib.PAN_PLANES_PER_GROUP == int(re.search(r"#define MPF_PAN_PLANES_PER_GROUP (\d+)", hdr).group(1))
    assert "mpf_pan.hip" in open(os.path.join(ROOT, "mpiflow_amd", "csrc", "Makefile")).read()


def test_library_exports_the_calls_and_refuses_bad_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in NEW_SYMBOLS)
    assert lib.mpf_pan_block1(None, None) == 10001 and b"null argument block" in lib.mpf_last_error()
    one = 256
    a = _lib.MpfPanArgs()
    a.B, a.S, a.h, a.w = 1, 5, 33, 47
    assert lib.mpf_pan_block1(ctypes.byref(a), None) == 10001 and b"null pointer (rgb_low" in lib.mpf_last_error()
    a.rgb_low = a.disp_low = a.plane_disp = a.out = one
    assert lib.mpf_pan_block1(ctypes.byref(a), None) == 10001 and b"null pointer (w1" in lib.mpf_last_error()
    a.w1 = a.b1 = a.bn_scale = a.bn_shift = a.w2 = a.b2 = a.w3 = a.b3 = one
    a.h = 1
    assert lib.mpf_pan_block1(ctypes.byref(a), None) == 10001 and b"at least 2" in lib.mpf_last_error()
    a.h, a.S = 33, 0
    assert lib.mpf_pan_block1(ctypes.byref(a), None) == 10001 and b"at least 1" in lib.mpf_last_error()
    a.S, a.B = 5, 70000
    assert lib.mpf_pan_block1(ctypes.byref(a), None) == 10001 and b"bad shape" in lib.mpf_last_error()
    a.B, a.S, a.h, a.w = 1, 1 << 10, 1 << 10, 1 << 10
    assert lib.mpf_pan_block1(ctypes.byref(a), None) == 10001 and b"2^31" in lib.mpf_last_error()
    a.S, a.h, a.w, a.w2 = 5, 33, 47, one + 2
    assert lib.mpf_pan_block1(ctypes.byref(a), None) == 10001 and b"4-byte aligned" in lib.mpf_last_error()
    a.w2 = one
    assert lib.mpf_pan_block1(ctypes.byref(a), None) == 10001 and b"workspace" in lib.mpf_last_error()
    need = lib.mpf_pan_block1_workspace(1, 33, 47)
    assert need == (2 * 1 + 1) * 8 * 33 * 47 * 4 and lib.mpf_pan_block1_workspace(2, 40, 72) == 5 * 8 * 40 * 72 * 4
    assert lib.mpf_pan_block1_workspace(1, 1, 47) == 0 and lib.mpf_pan_block1_workspace(0, 33, 47) == 0
    a.workspace, a.workspace_bytes = one, need - 1
    assert lib.mpf_pan_block1(ctypes.byref(a), None) == 10001 and b"workspace" in lib.mpf_last_error()
