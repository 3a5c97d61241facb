"""RAFT evaluation on frames of any size (mpiflow_amd/raft_eval.py, RAFT.predict) and its kernels (mpf_raft_images_padded,
mpf_upsample_flow_crop, mpf_upflow8_crop, mpf_flow_metrics of mpf_raft_eval.hip).

InputPadder: `_pad` against upstream's arithmetic restated here, for every (H, W) in 120..137 x 120..137 and both modes; pad / unpad against
F.pad(mode='replicate') and the slice.

The three data-movement kernels are bit-identical to the strict path they stand beside: raft_images_padded to ops.raft_images of the
F.pad'ed images, the two crops to the slice of ops.upsample_flow / ops.upflow8.  The crops write into the middle of a buffer filled with a
sentinel, at an offset that is no multiple of 16 bytes: nothing outside the window changes.

flow_metrics against evaluate.py's expressions restated in float64 numpy.  The inputs keep every threshold clear of rounding: ground-truth
magnitudes from {0, 10, 40, 100, 200}, error magnitudes from {0.25, 0.9, 1.1, 2.5, 3.5, 4.5, 7}, random directions; the test asserts in
float64 that no epe lies within 1e-3 of 1, 3 or 5 and no epe / mag within 1 percent of 0.05 (a condition on the inputs, not a tolerance).
Then the five counts are exact, and the epe sum over the count lies within FMT_BAR = 16 * 2^-24 * max(1, max epe) of the float64 value (the
format bar of tests/test_raft_model.py: the differences, squares, sum and root of an epe are a handful of fp32 roundings, each at most
2^-24 of max epe, and the sums themselves are float64).  Shapes: one pixel; odd sizes below one block; more than one block with a width
that is no multiple of 64; more than 512 * 256 pixels, where a block takes more than one pixel per lane.

The model: the reference's own `padder.unpad(model(*padder.pad(image1, image2), iters=12, test_mode=True)[1])` and flow_low, recorded on
the CPU in fp32 and double by tests/golden/make_raft_eval_golden.py into tests/golden/raft_eval.npz (150 sampled entries of the double run,
err32 and max |ref64| per array; inputs and weights rebuilt from seeds, their sums checked).  A missing golden fails.  The bar is that of
tests/test_raft_model.py: per array the larger of 3 * err32 and 2 x the error of the parts, which here are the strict path the feature
stands beside: unpad(RAFT.forward(*pad(image1, image2), test_mode=True)) with torch's F.pad and slicing, measured against the same double
run, on the same device, in the same test, after one unmeasured call (the first call of a convolution configuration in a process may pick
another MIOpen algorithm).  Measured on an MI355X: profiles/raft_eval/README.md."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "raft_eval.npz")
SYMBOLS = ("mpf_raft_images_padded", "mpf_upsample_flow_crop", "mpf_upflow8_crop", "mpf_flow_metrics")
U = 2.0 ** -24
PADS = [(0, 0, 0, 0), (2, 3, 3, 4), (3, 4, 0, 7), (0, 1, 0, 1), (3, 4, 3, 4)]


def fmt_bar(magnitude):
    return 16 * U * max(1.0, magnitude)


def _maker():
    spec = importlib.util.spec_from_file_location("make_raft_eval_golden", os.path.join(ROOT, "tests", "golden", "make_raft_eval_golden.py"))
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
    mk = _maker()
    g = dict(mk=mk, cases={})
    for name in [str(n) for n in z["names"]]:
        small, N, H, W, iters, kitti, seed = [int(v) for v in z[name + "/settings"]]
        d = mk.eval_inputs(N, H, W, seed)
        c = dict(name=name, small=bool(small), N=N, H=H, W=W, iters=iters, mode="kitti" if kitti else "sintel", seed=seed, d=d,
                 pad=[int(p) for p in z[name + "/pad"]], sums=z[name + "/input_sums"])
        assert sum(v.astype(np.float64).sum() for v in d.values()) == c["sums"][0], "the seeded inputs of %s are not the recorded ones" % name
        c["rec"] = {k: dict(f64=z["%s/%s_f64" % (name, k)], err32=float(z["%s/%s_err32" % (name, k)]), absmax=float(z["%s/%s_absmax" % (name, k)]))
                    for k in ("flow_low", "flow_up")}
        g["cases"][name] = c
    return g


def upstream_pad(H, W, mode):
    """RAFT/core/utils/utils.py:10-16, restated"""
    pad_ht = (((H // 8) + 1) * 8 - H) % 8
    pad_wd = (((W // 8) + 1) * 8 - W) % 8
    if mode == "sintel":
        return [pad_wd // 2, pad_wd - pad_wd // 2, pad_ht // 2, pad_ht - pad_ht // 2]
    return [pad_wd // 2, pad_wd - pad_wd // 2, 0, pad_ht]


def crop_of(x, pad):
    """InputPadder.unpad, restated"""
    ht, wd = x.shape[-2:]
    return x[..., pad[2]:ht - pad[3], pad[0]:wd - pad[1]]


# ------------------------------------------------------------------------------------------------------------------ no GPU needed


def test_input_padder_pads_as_upstream_does(raft_eval):
    for mode in ("sintel", "kitti"):
        for H in range(120, 138):
            for W in range(120, 138):
                p = raft_eval.InputPadder((1, 3, H, W), mode)
                assert p._pad == upstream_pad(H, W, mode) and (p.ht, p.wd) == (H, W), (H, W, mode, p._pad)
                assert (H + p._pad[2] + p._pad[3]) % 8 == 0 and (W + p._pad[0] + p._pad[1]) % 8 == 0 and all(0 <= q <= 7 for q in p._pad)
    assert raft_eval.InputPadder((3, 436, 1024))._pad == [0, 0, 2, 2]                   # the mode defaults to 'sintel'
    assert raft_eval.InputPadder((3, 375, 1242), mode="kitti")._pad == [3, 3, 0, 1]


def test_pad_and_unpad_are_replicate_padding_and_its_slice(raft_eval):
    rs = np.random.RandomState(5)
    for (H, W), mode in (((121, 131), "sintel"), ((121, 131), "kitti"), ((9, 15), "sintel"), ((128, 136), "kitti"), ((1, 1), "sintel")):
        a, b = torch.from_numpy(rs.rand(2, 3, H, W).astype(np.float32)), torch.from_numpy(rs.rand(2, 3, H, W).astype(np.float32))
        p = raft_eval.InputPadder(a.shape, mode)
        pa, pb = p.pad(a, b)
        assert torch.equal(pa, F.pad(a, upstream_pad(H, W, mode), mode="replicate")) and torch.equal(pb, F.pad(b, upstream_pad(H, W, mode), mode="replicate"))
        assert pa.shape[-2] % 8 == 0 and pa.shape[-1] % 8 == 0
        assert torch.equal(p.unpad(pa), a) and torch.equal(p.unpad(pb), b)
        flow = torch.from_numpy(rs.rand(2, 2, pa.shape[-2], pa.shape[-1]).astype(np.float32))
        assert torch.equal(p.unpad(flow), crop_of(flow, upstream_pad(H, W, mode))) and p.unpad(flow).shape == (2, 2, H, W)


def test_golden_is_present_and_its_recorded_conditions_hold(golden, raft_eval):
    cases = golden["cases"]
    assert sorted(cases) == ["basic/kitti_1x123x130", "basic/sintel_1x121x131", "small/kitti_1x121x131", "small/sintel_1x127x129"]
    for c in cases.values():
        assert c["iters"] == 12 and c["pad"] == raft_eval.InputPadder((c["H"], c["W"]), c["mode"])._pad == upstream_pad(c["H"], c["W"], c["mode"])
        for s in c["rec"].values():
            assert np.isfinite(s["f64"]).all() and s["f64"].dtype == np.float64 and len(s["f64"]) == 150
            assert 0.0 < s["err32"] <= 1e-3 * s["absmax"]
        assert c["rec"]["flow_up"]["absmax"] >= 1.0
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "raft_model.npz"))


def test_symbols_are_declared_bound_and_exported_and_validate_before_launching(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read(), flags=re.S)
    for path in (built.LIB_PATH, built.WITNESS_PATH):
        lib = ctypes.CDLL(path)
        for name in SYMBOLS + ("mpf_flow_metrics_workspace",):
            assert name in built.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name), name
    lib = built.load()
    a = built.MpfRaftEvalArgs()
    refused = lambda fn, what: fn(ctypes.byref(a), None) == 10001 and what in lib.mpf_last_error()
    for name in SYMBOLS:
        fn = getattr(lib, name)
        assert fn(None, None) == 10001 and b"null argument block" in lib.mpf_last_error(), name
        a.pad_left, a.pad_right, a.pad_top, a.pad_bottom = 2, 2, 2, 2
        a.N, a.H, a.W = 1, 0, 4
        assert refused(fn, b"bad shape"), name
        a.N, a.H, a.W = 1, 4, 4                              # 4 + 2 + 2 = 8: a frame the padded batch accepts
        assert refused(fn, b"null pointer"), name
        a.pad_left, a.pad_right, a.pad_top, a.pad_bottom = 0, 0, 0, 0
        a.N, a.H, a.W = 1024, 1024, 1024
        assert refused(fn, b"2^31"), name
    # what the pad itself can get wrong; every pointer set, so that only the shape can be the fault (nothing is launched: no GPU here)
    fake = ctypes.c_void_p(256)
    a.image1 = a.image2 = a.pair = a.flow = a.mask = a.flow_up = a.flow_pr = a.flow_gt = a.metrics = a.workspace = fake
    for name in SYMBOLS[:3]:
        fn = getattr(lib, name)
        a.N, a.H, a.W = 1, 8, 8
        a.pad_left, a.pad_right, a.pad_top, a.pad_bottom = 0, 8, 0, 0
        assert refused(fn, b"bad shape") and b"0..7" in lib.mpf_last_error(), name
        a.pad_left, a.pad_right, a.pad_top, a.pad_bottom = 0, 0, -1, 1
        assert refused(fn, b"bad shape") and b"0..7" in lib.mpf_last_error(), name
    a.pad_left, a.pad_right, a.pad_top, a.pad_bottom = 0, 0, 0, 1
    assert refused(lib.mpf_raft_images_padded, b"bad shape") and b"multiples of 8" in lib.mpf_last_error()
    a.pad_bottom, a.pair = 0, ctypes.c_void_p(260)          # rows of 16-byte vectors: the batch itself must be 16-byte aligned
    assert refused(lib.mpf_raft_images_padded, b"pair must be 16-byte aligned")
    a.pair = fake
    a.N, a.H, a.W = 1, 1, 1
    a.pad_left, a.pad_right, a.pad_top, a.pad_bottom = 0, 0, 4, 4
    assert refused(lib.mpf_upsample_flow_crop, b"bad shape") and b"no window" in lib.mpf_last_error()
    assert refused(lib.mpf_upflow8_crop, b"bad shape") and b"no window" in lib.mpf_last_error()
    # the metrics' workspace: sized by its own entry, 0 for a refused shape, and too small a one is refused
    assert lib.mpf_flow_metrics_workspace(1, 1, 1) == 48 and lib.mpf_flow_metrics_workspace(2, 16, 17) == 2 * 2 * 48
    assert lib.mpf_flow_metrics_workspace(1, 375, 1242) == 512 * 48                     # capped: a block then takes several pixels per lane
    assert lib.mpf_flow_metrics_workspace(1, 0, 4) == 0 and lib.mpf_flow_metrics_workspace(1024, 1024, 1024) == 0
    a.N, a.H, a.W, a.workspace_bytes = 2, 16, 17, 2 * 2 * 48 - 8
    assert refused(lib.mpf_flow_metrics, b"workspace holds")
    a.workspace = None
    assert refused(lib.mpf_flow_metrics, b"null pointer (workspace)")


def test_predict_refuses_in_the_order_of_the_contract_and_the_device_last(golden, raft, built):
    mk = golden["mk"]
    E = built.MpiFlowHipError
    img = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    ok = img(1, 3, 121, 131)                                 # pads to 128 x 136
    for small in (False, True):
        model = raft.RAFT(mk.make_args(small)).eval()
        with pytest.raises(E, match="image1 must be a torch.Tensor"):
            model.predict(ok.numpy(), ok)
        with pytest.raises(E, match="image2 must be float32.*float16"):
            model.predict(ok, ok.half())
        with pytest.raises(E, match=r"image1 must be \[N,3,H,W\]"):
            model.predict(img(3, 121, 131), ok)
        with pytest.raises(E, match=r"image2 must be \[N,3,H,W\] like image1"):
            model.predict(ok, img(1, 3, 121, 130))
        with pytest.raises(E, match="padded frame must be at least 128 x 128.*100 x 200, padded to 104 x 200"):
            model.predict(img(1, 3, 100, 200), img(1, 3, 100, 200))
        with pytest.raises(E, match="padded frame must be at least 128 x 128.*121 x 119, padded to 128 x 120"):
            model.predict(img(1, 3, 121, 119), img(1, 3, 121, 119), mode="kitti")
        with pytest.raises(E, match=r"flow_init must be \[N,2,Hp/8,Wp/8\]"):
            model.predict(ok, ok, flow_init=torch.zeros(1, 2, 15, 16))                      # H/8, W/8 of the unpadded frame
        with pytest.raises(E, match="flow_init must be float32"):
            model.predict(ok, ok, flow_init=torch.zeros(1, 2, 16, 17, dtype=torch.float64))
        # valid tensors on the CPU: the device, and only now; 127 x 129 is accepted (it pads to 128 x 136), as is a non-contiguous image
        with pytest.raises(E, match="image1 must live on the GPU"):
            model.predict(ok, ok, flow_init=torch.zeros(1, 2, 16, 17))
        with pytest.raises(E, match="image1 must live on the GPU"):
            model.predict(img(2, 3, 127, 129), img(2, 3, 127, 129), mode="kitti")
        with pytest.raises(E, match="image1 must live on the GPU"):
            model.predict(ok.transpose(2, 3).contiguous().transpose(2, 3), ok)
        # training mode: named after the tensors' own faults, before the device
        model.train()
        with pytest.raises(E, match=r"training mode.*\.eval\(\)"):
            model.predict(ok, ok)
        with pytest.raises(E, match=r"flow_init must be \[N,2,Hp/8,Wp/8\]"):
            model.predict(ok, ok, flow_init=torch.zeros(1, 2, 15, 16))
        with pytest.raises(E, match="must be float32"):
            model.predict(img(1, 3, 64, 96, dtype=torch.float64), ok)
        model.eval()
        with pytest.raises(E, match=r"image2 must be \[N,3,H,W\] like image1"):
            model.predict(img(1, 3, 64, 96), ok)                                          # a wrong shape before the frame's size


def test_forward_keeps_its_strict_refusals(golden, raft, built):
    mk = golden["mk"]
    E = built.MpiFlowHipError
    for small in (False, True):
        model = raft.RAFT(mk.make_args(small))
        with pytest.raises(E, match="RAFT: the frame's H and W must be multiples of 8 \\(got 130 x 136; pad it first, as upstream's InputPadder does\\)"):
            model(torch.zeros(1, 3, 130, 136), torch.zeros(1, 3, 130, 136))
        with pytest.raises(E, match="multiples of 8.*121 x 131"):
            model(torch.zeros(1, 3, 121, 131), torch.zeros(1, 3, 121, 131), test_mode=True)
        with pytest.raises(E, match="frame must be at least 128 x 128.*64 x 96"):
            model(torch.zeros(1, 3, 64, 96), torch.zeros(1, 3, 64, 96))
        with pytest.raises(E, match="image1 must live on the GPU"):
            model(torch.zeros(1, 3, 128, 136), torch.zeros(1, 3, 128, 136))


def test_ops_refuse_what_the_kernels_would_not_and_the_device_last(built, raft_eval):
    from mpiflow_amd import ops
    E = built.MpiFlowHipError
    z = torch.zeros
    with pytest.raises(E, match="image2 must be"):
        ops.raft_images_padded(z(1, 3, 5, 5), z(1, 3, 5, 6), (1, 2, 1, 2))
    with pytest.raises(E, match="pad must be .*four integers 0..7"):
        ops.raft_images_padded(z(1, 3, 5, 5), z(1, 3, 5, 5), (1, 2, 3))
    with pytest.raises(E, match="pad must be .*four integers 0..7"):
        ops.raft_images_padded(z(1, 3, 5, 5), z(1, 3, 5, 5), (1, 2, 8, 0))
    with pytest.raises(E, match="pad must be .*four integers 0..7"):
        ops.upflow8_crop(z(1, 2, 4, 4), (1.0, 2, 0, 0))
    with pytest.raises(E, match="multiples of 8.*5 x 5.*8 x 7"):
        ops.raft_images_padded(z(1, 3, 5, 5), z(1, 3, 5, 5), (1, 1, 1, 2))
    with pytest.raises(E, match="image1 must live on the GPU"):
        ops.raft_images_padded(z(1, 3, 5, 5), z(1, 3, 5, 5), [1, 2, 1, 2])
    with pytest.raises(E, match="made for 5 x 5 frames"):
        raft_eval.InputPadder((5, 5)).pair(z(1, 3, 5, 6), z(1, 3, 5, 6))
    with pytest.raises(E, match="image1 must live on the GPU"):
        raft_eval.InputPadder((5, 5)).pair(z(1, 3, 5, 5), z(1, 3, 5, 5))
    with pytest.raises(E, match="mask must be"):
        ops.upsample_flow_crop(z(1, 2, 4, 4), z(1, 576, 4, 5), (0, 0, 0, 0))
    with pytest.raises(E, match="leaves no window"):
        ops.upflow8_crop(z(1, 2, 1, 4), (0, 0, 4, 4))
    with pytest.raises(E, match=r"out must be \[N,2,8H-top-bottom,8W-left-right\]"):
        ops.upflow8_crop(z(1, 2, 4, 4), (1, 2, 3, 4), out=z(1, 2, 32, 32))
    with pytest.raises(E, match="flow must live on the GPU"):
        ops.upflow8_crop(z(1, 2, 4, 4), (1, 2, 3, 4), out=z(1, 2, 25, 29))
    with pytest.raises(E, match="flow must live on the GPU"):
        ops.upsample_flow_crop(z(1, 2, 4, 4), z(1, 576, 4, 4), (1, 2, 3, 4))
    with pytest.raises(E, match="flow_gt must be"):
        ops.flow_metrics(z(1, 2, 4, 4), z(1, 2, 4, 5))
    with pytest.raises(E, match="valid must be"):
        ops.flow_metrics(z(1, 2, 4, 4), z(1, 2, 4, 4), z(1, 1, 4, 4))
    with pytest.raises(E, match="valid must be float32"):
        ops.flow_metrics(z(1, 2, 4, 4), z(1, 2, 4, 4), z(1, 4, 4, dtype=torch.bool))
    with pytest.raises(E, match="flow_pr must live on the GPU"):
        ops.flow_metrics(z(1, 2, 4, 4), z(1, 2, 4, 4), z(1, 4, 4))
    m = raft_eval.FlowMetrics()
    with pytest.raises(E, match="no frame has been added"):
        m.result("sintel")
    with pytest.raises(E, match="kind must be 'sintel' or 'kitti'"):
        m.result("chairs")


# --------------------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W,mode", [(1, 1, 1, "sintel"), (2, 121, 131, "sintel"), (2, 121, 131, "kitti"), (1, 127, 129, "kitti"), (1, 128, 136, "sintel"),
                                        (1, 9, 15, "sintel")], ids=lambda v: str(v))
def test_gpu_raft_images_padded_is_raft_images_of_the_padded_images_bit_for_bit(N, H, W, mode, built, raft_eval, dev):
    from mpiflow_amd import ops
    rs = np.random.RandomState(61 + H + W)
    shape = (N, 3, H, W)
    ints = np.resize(np.arange(256, dtype=np.float32), int(np.prod(shape))).reshape(shape)
    pad = upstream_pad(H, W, mode)
    for what, im1, im2 in (("0..255", ints, ints[..., ::-1, ::-1].copy()),
                           ("non-integers", (255.0 * rs.rand(*shape)).astype(np.float32), (300.0 * rs.rand(*shape) - 20.0).astype(np.float32))):
        a, b = torch.from_numpy(im1).to(dev), torch.from_numpy(im2).to(dev)
        padder = raft_eval.InputPadder(a.shape, mode)
        assert padder._pad == pad
        want = ops.raft_images(*[t.contiguous() for t in padder.pad(a, b)])
        got = padder.pair(a, b)
        assert got.shape == (2 * N, 3, H + pad[2] + pad[3], W + pad[0] + pad[1]) and got.dtype == torch.float32 and got.is_contiguous()
        assert same_bytes(got, want), (what, int((got != want).sum()))
        assert same_bytes(got, ops.raft_images_padded(a, b, pad))
        if not any(pad):
            assert same_bytes(got, ops.raft_images(a, b)), what


@pytest.mark.gpu
@pytest.mark.parametrize("N,h,w", [(1, 1, 1), (2, 1, 9), (2, 5, 1), (2, 16, 17)], ids=lambda v: str(v))
def test_gpu_cropped_upsamplings_are_the_slices_bit_for_bit_and_write_nothing_else(N, h, w, built, dev):
    from mpiflow_amd import ops
    rs = np.random.RandomState(71 + 10 * h + w)
    flow = torch.from_numpy((3.0 * rs.standard_normal((N, 2, h, w))).astype(np.float32)).to(dev)
    mask = torch.from_numpy((2.0 * rs.standard_normal((N, 576, h, w))).astype(np.float32)).to(dev)
    full = dict(convex=ops.upsample_flow(flow, mask), bilinear=ops.upflow8(flow))
    SENTINEL, GUARD = -12345.0, 37                           # 37 floats: the window then starts at no multiple of 16 bytes
    for pad in PADS:
        Ho, Wo = 8 * h - pad[2] - pad[3], 8 * w - pad[0] - pad[1]
        assert Ho >= 1 and Wo >= 1
        for kind, call in (("convex", lambda **kw: ops.upsample_flow_crop(flow, mask, pad, **kw)), ("bilinear", lambda **kw: ops.upflow8_crop(flow, pad, **kw))):
            want = crop_of(full[kind], pad).contiguous()
            got = call()
            assert got.shape == (N, 2, Ho, Wo) and got.dtype == torch.float32 and got.is_contiguous()
            assert same_bytes(got, want), (kind, pad, int((got != want).sum()))
            n = N * 2 * Ho * Wo
            buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
            out = buf[GUARD:GUARD + n].view(N, 2, Ho, Wo)
            assert out.data_ptr() % 16 != 0 and call(out=out) is out
            assert same_bytes(out, want), (kind, pad, "into a window of a larger buffer")
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), (kind, pad, "wrote outside its window")


def make_flows(N, H, W, seed):
    """flow_gt, flow_pr, valid as float32 arrays: magnitudes from the issue's sets, random directions; the first pixels of every frame are
    mag = 0 with an error below 3 and above 3 (where there are that many pixels)"""
    rs = np.random.RandomState(seed)
    gmag = rs.choice([0.0, 10.0, 40.0, 100.0, 200.0], (N, H, W))
    emag = rs.choice([0.25, 0.9, 1.1, 2.5, 3.5, 4.5, 7.0], (N, H, W))
    flat_g, flat_e = gmag.reshape(N, -1), emag.reshape(N, -1)
    for i, (g, e) in enumerate(((0.0, 2.5), (0.0, 3.5), (0.0, 7.0), (0.0, 0.25))):
        if i < H * W - 1:
            flat_g[:, i], flat_e[:, i] = g, e
    ga, ea = 2 * np.pi * rs.rand(N, H, W), 2 * np.pi * rs.rand(N, H, W)
    gt = np.stack([gmag * np.cos(ga), gmag * np.sin(ga)], axis=1).astype(np.float32)
    pr = (gt.astype(np.float64) + np.stack([emag * np.cos(ea), emag * np.sin(ea)], axis=1)).astype(np.float32)
    valid = rs.choice([0.0, 0.4, 0.5, 1.0], (N, H, W)).astype(np.float32)
    return gt, pr, valid


def restated(gt, pr, valid):
    """evaluate.py's expressions (validate_sintel / validate_kitti) in float64: per frame [sum epe, counted, epe < 1, < 3, < 5, outliers], the
    largest epe, and the check that the inputs keep every threshold clear of rounding"""
    gt, pr = gt.astype(np.float64), pr.astype(np.float64)
    epe = np.sqrt(((pr - gt) ** 2).sum(axis=1))
    mag = np.sqrt((gt ** 2).sum(axis=1))
    for thr in (1.0, 3.0, 5.0):
        assert (np.abs(epe - thr) > 1e-3).all(), "an epe lies within 1e-3 of %g" % thr
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = epe / mag
    assert (np.abs(ratio[np.isfinite(ratio)] - 0.05) > 0.01 * 0.05).all(), "an epe / mag lies within 1 percent of 0.05"
    val = np.ones(epe.shape, bool) if valid is None else valid >= 0.5
    out = (epe > 3.0) & (ratio > 0.05)
    rows = [[epe[n][val[n]].sum(), val[n].sum(), (epe[n][val[n]] < 1).sum(), (epe[n][val[n]] < 3).sum(), (epe[n][val[n]] < 5).sum(), out[n][val[n]].sum()]
            for n in range(len(epe))]
    return np.array(rows, np.float64), float(epe.max())


def check_rows(got, want, epe_max, what):
    assert got.shape == want.shape and got.dtype == np.float64
    assert (got[:, 1:] == want[:, 1:]).all(), (what, got[:, 1:], want[:, 1:])
    for g, w in zip(got, want):
        if w[1]:
            d = abs(g[0] / g[1] - w[0] / w[1])
            print("flow_metrics %-28s mean epe %.6f, |hip - float64| %.2e = %.3f of FMT_BAR" % (what, w[0] / w[1], d, d / fmt_bar(epe_max)))
            assert d <= fmt_bar(epe_max), (what, d, fmt_bar(epe_max))
        else:
            assert g[0] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 5, 7), (1, 37, 53), (2, 67, 131), (1, 363, 365)], ids=lambda v: str(v))
def test_gpu_flow_metrics_match_evaluate_py_restated(N, H, W, built, dev):
    from mpiflow_amd import ops
    gt, pr, valid = make_flows(N, H, W, 83 + H)
    t = lambda a: torch.from_numpy(a).to(dev)
    for use_valid in (False, True):
        want, epe_max = restated(gt, pr, valid if use_valid else None)
        runs = [ops.flow_metrics(t(pr), t(gt), t(valid) if use_valid else None) for _ in range(2)]
        assert runs[0].shape == (N, 6) and runs[0].dtype == torch.float64 and runs[0].device == dev
        assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64)), "two runs differ"
        check_rows(runs[0].cpu().numpy(), want, epe_max, "%dx%dx%d %s" % (N, H, W, "valid" if use_valid else "all pixels"))
    if H * W > 4:                                            # the forced pixels: mag = 0 with epe below and above 3; only the latter are outliers
        acc = ops.flow_metrics(t(pr[:, :, :1, :4].copy()), t(gt[:, :, :1, :4].copy())).cpu().numpy()
        assert (acc[:, 1] == 4).all() and (acc[:, 5] == 2).all() and (acc[:, 2] == 1).all() and (acc[:, 3] == 2).all() and (acc[:, 4] == 3).all(), acc


@pytest.mark.gpu
def test_gpu_flow_metrics_results_aggregate_as_evaluate_py_does(built, raft_eval, dev):
    t = lambda a: torch.from_numpy(a).to(dev)
    # validate_kitti over two frames of one update and one more of another size; frame 1 has no valid pixel
    gt, pr, valid = make_flows(2, 37, 53, 97)
    gt2, pr2, valid2 = make_flows(1, 5, 7, 98)
    m = raft_eval.FlowMetrics()
    m.update(t(pr), t(gt), t(valid))
    m.update(t(pr2), t(gt2), t(valid2))
    rows = np.concatenate([restated(gt, pr, valid)[0], restated(gt2, pr2, valid2)[0]])
    bar = fmt_bar(max(restated(gt, pr, valid)[1], restated(gt2, pr2, valid2)[1]))
    res = m.result("kitti")
    assert sorted(res) == ["kitti-epe", "kitti-f1"] and all(type(v) is float for v in res.values())
    want_epe, want_f1 = float(np.mean(rows[:, 0] / rows[:, 1])), float(100.0 * rows[:, 5].sum() / rows[:, 1].sum())
    print("kitti: epe %.6f (restated %.6f), f1 %.6f (restated %.6f)" % (res["kitti-epe"], want_epe, res["kitti-f1"], want_f1))
    assert abs(res["kitti-epe"] - want_epe) <= bar and abs(res["kitti-f1"] - want_f1) <= 1e-9
    valid[1] = 0.4                                           # below 0.5 everywhere: upstream's epe[val].mean() of nothing is nan
    m = raft_eval.FlowMetrics()
    m.update(t(pr), t(gt), t(valid))
    res = m.result("kitti")
    rows = restated(gt, pr, valid)[0]
    assert rows[1, 1] == 0 and np.isnan(res["kitti-epe"]) and abs(res["kitti-f1"] - 100.0 * rows[0, 5] / rows[0, 1]) <= 1e-9
    m = raft_eval.FlowMetrics()
    m.update(t(pr[1:]), t(gt[1:]), t(valid[1:]))
    assert all(np.isnan(v) for v in m.result("sintel").values()) and all(np.isnan(v) for v in m.result("kitti").values())
    # validate_sintel / validate_chairs: every pixel of frames of mixed sizes, np.mean(np.concatenate(epe_list)) and its companions
    m = raft_eval.FlowMetrics()
    m.update(t(pr), t(gt))
    m.update(t(pr2), t(gt2))
    rows = np.concatenate([restated(gt, pr, None)[0], restated(gt2, pr2, None)[0]])
    res = m.result("sintel")
    assert sorted(res) == ["1px", "3px", "5px", "epe"] and all(type(v) is float for v in res.values())
    total = rows.sum(axis=0)
    assert total[1] == 2 * 37 * 53 + 5 * 7
    assert abs(res["epe"] - total[0] / total[1]) <= bar
    for key, q in (("1px", 2), ("3px", 3), ("5px", 4)):
        assert abs(res[key] - total[q] / total[1]) <= 1e-12, key


_RUNS = {}


def _prepare(c, model, dev, mk):
    assert mk.fill_params(model, c["seed"]) == c["sums"][1], "the seeded weights of %s are not the recorded ones" % c["name"]
    model.to(dev)
    model.freeze_bn()
    return model.eval()


def torch_form(model, raft_eval, a, b, c):
    """the strict path with torch's glue: what a port of evaluate.py does without this feature"""
    padder = raft_eval.InputPadder(a.shape, c["mode"])
    with torch.no_grad():
        pa, pb = padder.pad(a, b)
        flow_low, flow_pr = model(pa, pb, iters=c["iters"], test_mode=True)
        return dict(flow_low=flow_low, flow_up=padder.unpad(flow_pr).contiguous())


def fused_form(model, a, b, c):
    flow_low, flow_up = model.predict(a, b, iters=c["iters"], mode=c["mode"])
    return dict(flow_low=flow_low, flow_up=flow_up)


def sample_err(c, mk, key, val):
    idx = mk.sample_index(val.numel(), c["seed"])
    return float(np.abs(val.double().cpu().numpy().reshape(-1)[idx] - c["rec"][key]["f64"]).max())


def runs_of(c, raft, raft_eval, dev, mk):
    """predict and the strict path on one case, once per module: (model, a, b, {key: predict's result}, {key: (predict's error, the parts', bar)})"""
    if c["name"] not in _RUNS:
        model = _prepare(c, raft.RAFT(mk.make_args(c["small"])), dev, mk)
        a, b = torch.from_numpy(c["d"]["image1"]).to(dev), torch.from_numpy(c["d"]["image2"]).to(dev)
        torch_form(model, raft_eval, a, b, c)                # unmeasured: see the module docstring
        got = fused_form(model, a, b, c)
        parts = torch_form(model, raft_eval, a, b, c)
        Hp, Wp = c["H"] + c["pad"][2] + c["pad"][3], c["W"] + c["pad"][0] + c["pad"][1]
        assert got["flow_low"].shape == (c["N"], 2, Hp // 8, Wp // 8) and got["flow_up"].shape == (c["N"], 2, c["H"], c["W"])
        table = {}
        for key in ("flow_low", "flow_up"):
            assert got[key].shape == parts[key].shape and got[key].dtype == torch.float32 and got[key].is_contiguous() and not got[key].requires_grad
            d, dp = sample_err(c, mk, key, got[key]), sample_err(c, mk, key, parts[key])
            table[key] = (d, dp, max(3 * c["rec"][key]["err32"], 2 * dp), float((got[key] - parts[key]).abs().max()))
        _RUNS[c["name"]] = (model, a, b, got, table)
    return _RUNS[c["name"]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["basic/sintel_1x121x131", "basic/kitti_1x123x130", "small/kitti_1x121x131", "small/sintel_1x127x129"])
def test_gpu_predict_matches_the_recorded_reference(name, golden, raft, raft_eval, dev):
    c = golden["cases"][name]
    _, _, _, _, table = runs_of(c, raft, raft_eval, dev, golden["mk"])
    for key, (d, dp, bar, diff) in table.items():
        s = c["rec"][key]
        print("predict %-24s %-9s |hip - ref64| %.2e = %.2f err32 (%.2e) = %.3f of the bar; strict path with torch's pad and slice %.2e; |predict - strict| %.1e; absmax %.2e"
              % (name, key, d, d / s["err32"], s["err32"], d / bar, dp, diff, s["absmax"]))
    for key, (d, dp, bar, _) in table.items():
        assert d <= bar, (name, key, d, c["rec"][key]["err32"], dp)


@pytest.mark.gpu
def test_gpu_predict_with_alternate_corr_gives_the_all_pairs_prediction(golden, raft, raft_eval, dev):
    c = golden["cases"]["basic/sintel_1x121x131"]
    mk = golden["mk"]
    _, a, b, got, table = runs_of(c, raft, raft_eval, dev, mk)
    args = mk.make_args(False)
    args.alternate_corr = True
    model = _prepare(c, raft.RAFT(args), dev, mk)
    assert model.args.alternate_corr is True
    alt = fused_form(model, a, b, c)
    for key in ("flow_low", "flow_up"):
        d = sample_err(c, mk, key, alt[key])
        print("predict, alternate_corr %-9s |hip - ref64| %.2e = %.3f of the bar; |alt - all pairs| %.2e" % (key, d, d / table[key][2], float((alt[key] - got[key]).abs().max())))
        assert d <= table[key][2], (key, d, table[key])


@pytest.mark.gpu
def test_gpu_predict_takes_flow_init_of_the_padded_frame(golden, raft, raft_eval, dev):
    c = golden["cases"]["small/sintel_1x127x129"]
    model, a, b, _, _ = runs_of(c, raft, raft_eval, dev, golden["mk"])
    init = torch.from_numpy((2.0 * np.random.RandomState(3).standard_normal((1, 2, 16, 17))).astype(np.float32)).to(dev)
    padder = raft_eval.InputPadder(a.shape, c["mode"])
    with torch.no_grad():
        low, up = model(*padder.pad(a, b), iters=3, flow_init=init, test_mode=True)
    got_low, got_up = model.predict(a, b, iters=3, flow_init=init, mode=c["mode"])
    # the same kernels on the same bytes up to the convolutions, whose algorithm the library may choose per call: the model's own bar
    bar = 3 * c["rec"]["flow_up"]["err32"]
    d_low, d_up = float((got_low - low).abs().max()), float((got_up - padder.unpad(up)).abs().max())
    print("predict with flow_init: |predict - strict| flow_low %.2e, flow_up %.2e (bar %.2e)" % (d_low, d_up, bar))
    assert got_up.shape == (1, 2, 127, 129) and d_low <= bar and d_up <= bar


@pytest.mark.gpu
def test_gpu_predict_allocates_no_more_than_the_strict_path(golden, raft, raft_eval, dev):
    c = golden["cases"]["basic/sintel_1x121x131"]
    model, a, b, _, _ = runs_of(c, raft, raft_eval, dev, golden["mk"])        # both forms have run: every convolution has its algorithm
    peaks = {}
    for name, form in (("fused", lambda: fused_form(model, a, b, c)), ("torch", lambda: torch_form(model, raft_eval, a, b, c)), ("fused again", lambda: fused_form(model, a, b, c))):
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = form()
        torch.cuda.synchronize(dev)
        peaks[name] = torch.cuda.max_memory_allocated(dev) - base
        del out
    Hp, Wp = 128, 136
    print("peak allocation above the inputs, 1 x 121 x 131 basic: predict %d bytes, the strict path with torch's pad and slice %d bytes (%d more; one padded "
          "prediction is %d bytes, the two padded images %d)" % (peaks["fused"], peaks["torch"], peaks["torch"] - peaks["fused"], 2 * Hp * Wp * 4, 6 * Hp * Wp * 4))
    assert peaks["fused"] <= peaks["torch"] and peaks["fused again"] <= peaks["torch"]
