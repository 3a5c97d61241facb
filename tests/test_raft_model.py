"""The assembled RAFT model (mpiflow_amd/raft.py) and its glue kernels (mpf_raft_images, mpf_context_split, mpf_upflow8 and their _backward calls
of mpf_raft_glue.hip).

The reference is the reference's own raft.py, recorded on the CPU by tests/golden/make_raft_golden.py into tests/golden/raft_model.npz: per
array 150 sampled entries of the DOUBLE run, err32 = max |fp32 run - double run| over the whole array, and max |ref64|.  Inputs and weights are
rebuilt from seeds (their float64 sums are checked).  A missing golden fails these tests; it does not skip them.

Bars.  Every bar is absolute.

The model: the convolutions are MIOpen's and their summation order is not the CPU's, so per recorded array the bar is the larger of 3 * err32
and 2 x the error that PartsRAFT below makes against the same double run, in the same test, on the same device.  PartsRAFT is the parent
commit's four modules wired together with upstream's plain-torch glue (the image scaling, torch.split / tanh / relu, F.interpolate): not the
code under test.  Measured on an MI355X: profiles/raft/README.md.

upflow8, against the formula restated in float64 (UP8).  Per axis of coarse size n the weight with which a fine pixel reads a coarse one is a
hat function of the source coordinate src = dst * (n-1)/(8n-1), Lipschitz 1.  The kernel rounds the scale once and the product once, and
src <= n-1, so |d src| <= 2 u (n-1), u = 2^-24; 1 - l, the products and the sums of the blend add at most 6 u to a tap of weight <= 1.  With
the factor 8 a tap's coefficient is good to e = 8 u (2 (H-1) + 2 (W-1) + 6).  Forward: four taps of magnitude <= max |flow|: bar = 4 e max |flow|.
Backward (sums in fp64, so nothing else adds): a coarse pixel is touched by at most Ky * Kx fine pixels, K = min(8n, floor(2 (8n-1)/(n-1)) + 1)
(8 for n = 1): bar = Ky Kx e max |g|.  Worst-case bounds: a wrong index or scale is an error of the order of the values themselves.
torch's F.interpolate on the same device shares the coordinate arithmetic; the forward bar is asked of that difference too.

context_split: inp and the gradient's mask are bit-identical to torch's relu.  net and its gradient against float64 tanh: the bar of
tests/test_raft_update.py, FMT_BAR = 16 u max(1, magnitude): tanhf is good to about 2 ulp, |net| <= 1, so 1 - net^2 is good to 5 u and the
gradient to 5 u |g| plus a rounding; the magnitude is max |g| there.

raft_images is bit-identical to 2 * (x / 255.0) - 1.0 as torch's CPU kernel computes it - a true division, the arithmetic the reference was
recorded with.  (torch's GPU kernel for a division by a Python scalar multiplies by the rounded reciprocal instead, which differs in the last
bit for most values; the test prints how many entries that is.)

coarse=True: the loss of raft_upsample.sequence_loss on the coarse pairs against train.py's sequence_loss restated in torch (float64 sums)
on the predictions of the coarse=False call: relative bar 3.72e-7, the largest of tests/test_raft_upsample.py's recorded bars (3 x the
reference's own fp32 error on a loss term, case real_2x36x120).  Parameter gradients of the two calls agree under the model bar of the same
array, as the issue sets it.  That bar belongs to the recorded loss, whose cotangents are of unit scale; sequence_loss's are at most
1 / (N*2*H*W), so here it is loose, and the test prints the difference relative to the gradient's own magnitude beside it.  (Dividing the bar
by N*2*H*W is NOT sound: the recorded cotangents have random signs, sequence_loss's follow the prediction, so its gradients do not shrink by
that factor; measured, the difference of the two calls is up to 5.2 x such a bar, 1.8e-8 on the structurally zero gradients.)

Every case runs the parts once, unmeasured, before the two measured runs: the first call of a convolution configuration in a process may
pick another MIOpen algorithm than the later ones.  Without it one run on an MI355X had ten weight gradients of fnet (basic/train) at 3.4 to
4.7 err32, up to 1.57 x their bar, the parts at 0.03 to 1.7 err32; a second run of the same code on another machine had every array of every
case below 0.47 of its bar."""
import argparse
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "raft_model.npz")
SYMBOLS = ("mpf_raft_images", "mpf_context_split", "mpf_context_split_backward", "mpf_upflow8", "mpf_upflow8_backward")
U = 2.0 ** -24
LOSS_REL_BAR = 3.72e-7


def _maker():
    spec = importlib.util.spec_from_file_location("make_raft_golden", os.path.join(ROOT, "tests", "golden", "make_raft_golden.py"))
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
def golden():
    z = np.load(GOLDEN, allow_pickle=False)                  # a missing file is an error here, not a skip
    mk = _maker()
    g = dict(mk=mk, z=z, cases={}, state={k: [str(s) for s in z["state/" + k]] for k in ("basic", "small")})
    for name in [str(n) for n in z["names"]]:
        small, N, H, W, iters, train, seed = [int(v) for v in z[name + "/settings"]]
        d = mk.case_inputs(N, H, W, iters, bool(train), seed)
        c = dict(name=name, small=bool(small), N=N, H=H, W=W, iters=iters, train=bool(train), seed=seed, d=d, sums=z[name + "/input_sums"])
        assert sum(v.astype(np.float64).sum() for v in d.values()) == c["sums"][0], "the seeded inputs of %s are not the recorded ones" % name
        c["keys"] = [str(k) for k in z[name + "/keys"]]
        c["rec"] = {k: dict(f64=z["%s/%s_f64" % (name, k)], err32=float(z["%s/%s_err32" % (name, k)]), absmax=float(z["%s/%s_absmax" % (name, k)]))
                    for k in c["keys"]}
        c["zero_grads"] = [str(k) for k in z[name + "/zero_grads"]] if train else []
        g["cases"][name] = c
    return g


def state_dict_of(entries, prefix=""):
    out = {}
    for e in entries:
        name, shape = e.rsplit(":", 1)
        shape = tuple(int(s) for s in shape.split("x")) if shape else ()
        out[prefix + name] = torch.zeros(shape, dtype=torch.int64 if name.endswith("num_batches_tracked") else torch.float32)
    return out


# ------------------------------------------------------------------------------------------------------------------ no GPU needed


def test_golden_is_present_and_its_recorded_conditions_hold(golden):
    cases = golden["cases"]
    assert sorted(cases) == ["basic/eval_1x128x128", "basic/train_2x128x136", "small/eval_1x128x128", "small/train_2x136x128"]
    for c in cases.values():
        forward = [k for k in c["keys"] if not k.startswith("grad_")]
        want = ["pred_%d" % i for i in range(c["iters"])] if c["train"] else ["flow_coarse", "flow_up"]
        want += ["net", "inp", "fmap1"] + (["up_mask_last"] if c["train"] and not c["small"] else [])
        assert forward == want, (c["name"], forward)
        assert c["iters"] == (3 if c["train"] else 12)
        for k in c["keys"]:
            s = c["rec"][k]
            assert np.isfinite(s["f64"]).all() and s["f64"].dtype == np.float64 and len(s["f64"]) == 150
            assert s["err32"] > 0.0, (c["name"], k)
            if k in forward:
                assert s["err32"] <= 1e-3 * s["absmax"], (c["name"], k, s["err32"], s["absmax"])
        assert c["rec"][want[c["iters"] - 1 if c["train"] else 1]]["absmax"] >= 1.0
        if c["train"]:
            grads = [k for k in c["keys"] if k.startswith("grad_")]
            assert len(grads) == (106 if c["small"] else 124) and len(c["zero_grads"]) == (21 if c["small"] else 30)
            top = max(c["rec"][k]["absmax"] for k in grads)
            assert c["zero_grads"] == [k[5:] for k in grads if c["rec"][k]["absmax"] <= 1e-9 * top]
            assert all(k.endswith(".bias") and (k.startswith("fnet.") or k.startswith("cnet.")) for k in c["zero_grads"])


def test_state_dicts_are_the_recorded_ones(golden, raft):
    mk = golden["mk"]
    for small in (False, True):
        args = mk.make_args(small)
        model = raft.RAFT(args)
        assert list(mk.state_list(model)) == golden["state"]["small" if small else "basic"]
        assert (args.corr_levels, args.corr_radius) == ((4, 3) if small else (4, 4))
        assert (model.hidden_dim, model.context_dim) == ((96, 64) if small else (128, 128))
        for name in ("fnet", "cnet", "update_block"):
            assert isinstance(getattr(model, name), nn.Module)
    args = argparse.Namespace(small=False, mixed_precision=False)      # upstream's defaults, written into args
    raft.RAFT(args)
    assert args.dropout == 0 and args.alternate_corr is False


def test_a_recorded_state_dict_loads_strictly_with_and_without_the_dataparallel_prefix(golden, raft):
    mk = golden["mk"]
    for small in (False, True):
        entries = golden["state"]["small" if small else "basic"]
        for prefix in ("", "module."):
            model = raft.RAFT(mk.make_args(small))
            sd = state_dict_of(entries, prefix)
            sd[prefix + "update_block.flow_head.conv2.bias"] += 3.0
            assert raft.RAFT.load_checkpoint(model, sd) is model
            assert float(model.update_block.flow_head.conv2.bias[0]) == 3.0 and not model.fnet.conv1.weight.any()
        model = raft.RAFT(mk.make_args(small))
        model.load_state_dict(state_dict_of(entries), strict=True)
        broken = state_dict_of(entries)
        broken.pop("fnet.conv1.bias")
        with pytest.raises(RuntimeError):
            raft.RAFT.load_checkpoint(model, broken)


def test_refusals_name_the_fault_and_the_device_is_judged_last(golden, raft, built):
    mk = golden["mk"]
    E = built.MpiFlowHipError
    with pytest.raises(E, match="mixed_precision.*float32 only"):
        raft.RAFT(argparse.Namespace(small=False, mixed_precision=True))
    basic, small = raft.RAFT(mk.make_args(False)), raft.RAFT(mk.make_args(True))
    img = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    ok = img(1, 3, 128, 136)
    for model in (basic, small):
        with pytest.raises(E, match="image1 must be a torch.Tensor"):
            model(ok.numpy(), ok)
        with pytest.raises(E, match="image2 must be float32.*float16"):
            model(ok, ok.half())
        with pytest.raises(E, match="image1 must be float32.*uint8"):
            model(img(1, 3, 128, 136, dtype=torch.uint8), ok)
        with pytest.raises(E, match=r"image1 must be \[N,3,H,W\]"):
            model(img(3, 128, 136), ok)
        with pytest.raises(E, match=r"image1 must be \[N,3,H,W\]"):
            model(img(1, 1, 128, 136), img(1, 1, 128, 136))
        with pytest.raises(E, match=r"image2 must be \[N,3,H,W\] like image1"):
            model(ok, img(1, 3, 128, 128))
        with pytest.raises(E, match="multiples of 8.*130 x 136"):
            model(img(1, 3, 130, 136), img(1, 3, 130, 136))
        with pytest.raises(E, match="frame must be at least 128 x 128.*64 x 96"):
            model(img(1, 3, 64, 96), img(1, 3, 64, 96))
        with pytest.raises(E, match="frame must be at least 128 x 128.*128 x 120"):
            model(img(1, 3, 128, 120), img(1, 3, 128, 120))
        with pytest.raises(E, match=r"flow_init must be \[N,2,H/8,W/8\]"):
            model(ok, ok, flow_init=torch.zeros(1, 2, 128, 136))
        with pytest.raises(E, match="flow_init must be float32"):
            model(ok, ok, flow_init=torch.zeros(1, 2, 16, 17, dtype=torch.float64))
        with pytest.raises(E, match="coarse=True.*test_mode" if model is basic else "coarse=True needs the basic model"):
            model(ok, ok, test_mode=True, coarse=True)
        # valid tensors on the CPU: the device, and only now
        with pytest.raises(E, match="image1 must live on the GPU"):
            model(ok, ok, flow_init=torch.zeros(1, 2, 16, 17))
        with pytest.raises(E, match="image1 must live on the GPU"):
            model(ok.transpose(2, 3).contiguous().transpose(2, 3), ok)          # non-contiguous: made contiguous, not refused
    with pytest.raises(E, match="coarse=True needs the basic model"):
        small(ok, ok, coarse=True)
    # a wrong dtype is named before a wrong shape, a wrong shape before the frame's size
    with pytest.raises(E, match="must be float32"):
        basic(img(1, 3, 64, 96, dtype=torch.float64), ok)
    with pytest.raises(E, match=r"image2 must be \[N,3,H,W\] like image1"):
        basic(img(1, 3, 64, 96), ok)


def test_ops_refuse_cpu_tensors_after_everything_else(built):
    from mpiflow_amd import ops, raft_upsample
    E = built.MpiFlowHipError
    with pytest.raises(E, match=r"flow must be \[None, 2, None, None\]|flow must be .*4 dimensions"):
        ops.upflow8(torch.zeros(1, 3, 4, 4))
    with pytest.raises(E, match="flow must live on the GPU"):
        raft_upsample.upflow8(torch.zeros(1, 2, 4, 4))
    with pytest.raises(E, match=r"8H,8W"):
        ops.upflow8_backward(torch.zeros(1, 2, 12, 16))
    with pytest.raises(E, match="grad_out must live on the GPU"):
        ops.upflow8_backward(torch.zeros(1, 2, 16, 16))
    with pytest.raises(E, match="hdim must be 1..7"):
        ops.context_split(torch.zeros(1, 8, 4, 4), 8)
    with pytest.raises(E, match="cnet must live on the GPU"):
        ops.context_split(torch.zeros(1, 8, 4, 4), 3)
    with pytest.raises(E, match="g_inp must be"):
        ops.context_split_backward(torch.zeros(1, 3, 4, 4), torch.zeros(1, 5, 4, 4), torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, 4))
    with pytest.raises(E, match="net must live on the GPU"):
        ops.context_split_backward(torch.zeros(1, 3, 4, 4), torch.zeros(1, 5, 4, 4), torch.zeros(1, 3, 4, 4), torch.zeros(1, 5, 4, 4))
    with pytest.raises(E, match="image2 must be"):
        ops.raft_images(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 16))
    with pytest.raises(E, match="image1 must be float32"):
        ops.raft_images(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), torch.zeros(1, 3, 8, 8))
    with pytest.raises(E, match="image1 must live on the GPU"):
        ops.raft_images(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))


def test_symbols_are_declared_bound_and_exported_and_validate_before_launching(built):
    import ctypes
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read(), flags=re.S)
    for path in (built.LIB_PATH, built.WITNESS_PATH):
        lib = ctypes.CDLL(path)
        for name in SYMBOLS:
            assert name in built.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name), name
    lib = built.load()
    a = built.MpfRaftGlueArgs()
    for name in SYMBOLS:
        fn = getattr(lib, name)
        assert fn(None, None) == 10001 and b"null argument block" in lib.mpf_last_error(), name
        a.N, a.H, a.W, a.hdim, a.cdim = 1, 0, 4, 2, 2
        assert fn(ctypes.byref(a), None) == 10001 and b"bad shape" in lib.mpf_last_error(), name
        a.N, a.H, a.W = 1, 4, 4
        assert fn(ctypes.byref(a), None) == 10001 and b"null pointer" in lib.mpf_last_error(), name
        a.N, a.H, a.W = 1024, 1024, 1024
        assert fn(ctypes.byref(a), None) == 10001 and b"2^31" in lib.mpf_last_error(), name
    a.N, a.H, a.W, a.hdim, a.cdim = 1, 4, 4, 0, 2
    assert lib.mpf_context_split(ctypes.byref(a), None) == 10001 and b"hdim and cdim" in lib.mpf_last_error()


# ------------------------------------------------------------------------------------------------ the formulas, restated (not code under test)


def up8_matrix(n):
    """[8n, n] float64: the weights with which fine index I reads the coarse ones, align_corners=True: src = I * (n-1)/(8n-1)"""
    A = np.zeros((8 * n, n))
    for I in range(8 * n):
        src = I * (n - 1) / (8 * n - 1) if n > 1 else 0.0
        i0 = min(int(np.floor(src)), n - 1)
        i1 = min(i0 + 1, n - 1)
        A[I, i0] += 1.0 - (src - i0)
        A[I, i1] += src - i0
    return A


def UP8(flow64):
    """8 * bilinear, align_corners=True, float64; as a pair of matrices it is its own adjoint's statement: UP8T"""
    Ay, Ax = up8_matrix(flow64.shape[2]), up8_matrix(flow64.shape[3])
    return 8.0 * np.einsum("Yy,ncyx,Xx->ncYX", Ay, flow64, Ax)


def UP8T(g64):
    Ay, Ax = up8_matrix(g64.shape[2] // 8), up8_matrix(g64.shape[3] // 8)
    return 8.0 * np.einsum("Yy,ncYX,Xx->ncyx", Ay, g64, Ax)


def up8_bars(H, W, flow_max, g_max):
    e = 8 * U * (2 * (H - 1) + 2 * (W - 1) + 6)
    K = lambda n: 8 if n == 1 else min(8 * n, (2 * (8 * n - 1)) // (n - 1) + 1)
    return 4 * e * flow_max, K(H) * K(W) * e * g_max


def fmt_bar(magnitude):
    return 16 * U * max(1.0, magnitude)


class PartsRAFT(nn.Module):
    """The parent commit's parts - the four modules as they were - with upstream's plain-torch glue between them.  Attribute names are
    upstream's, so the state dict is the reference's and fill_params() fills it as it fills the model under test."""

    def __init__(self, args):
        super().__init__()
        from mpiflow_amd.raft_extractor import BasicEncoder, SmallEncoder
        from mpiflow_amd.raft_update import BasicUpdateBlock, SmallUpdateBlock
        self.small = args.small
        args.corr_levels, args.corr_radius = 4, (3 if args.small else 4)
        self.radius = args.corr_radius
        if args.small:
            self.hidden_dim, self.context_dim = 96, 64
            self.fnet = SmallEncoder(output_dim=128, norm_fn="instance", dropout=0)
            self.cnet = SmallEncoder(output_dim=160, norm_fn="none", dropout=0)
            self.update_block = SmallUpdateBlock(args, hidden_dim=96)
        else:
            self.hidden_dim, self.context_dim = 128, 128
            self.fnet = BasicEncoder(output_dim=256, norm_fn="instance", dropout=0)
            self.cnet = BasicEncoder(output_dim=256, norm_fn="batch", dropout=0)
            self.update_block = BasicUpdateBlock(args, hidden_dim=128)

    def freeze_bn(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()

    def forward(self, image1, image2, iters=12, flow_init=None, test_mode=False, cap=None):
        from mpiflow_amd.raft_corr import CorrBlock
        from mpiflow_amd.raft_upsample import upsample_flow
        image1 = (2 * (image1 / 255.0) - 1.0).contiguous()
        image2 = (2 * (image2 / 255.0) - 1.0).contiguous()
        fmap1, fmap2 = self.fnet([image1, image2])
        corr_fn = CorrBlock(fmap1, fmap2, radius=self.radius)
        net, inp = torch.split(self.cnet(image1), [self.hidden_dim, self.context_dim], dim=1)
        net, inp = torch.tanh(net).contiguous(), torch.relu(inp).contiguous()
        if cap is not None:
            cap.update(net=net, inp=inp, fmap1=fmap1)
        N, _, H, W = image1.shape
        ys, xs = torch.meshgrid(torch.arange(H // 8, device=image1.device), torch.arange(W // 8, device=image1.device), indexing="ij")
        coords0 = torch.stack([xs, ys], dim=0).float()[None].repeat(N, 1, 1, 1)
        coords1 = coords0.clone() if flow_init is None else coords0 + flow_init
        preds = []
        for _ in range(iters):
            coords1 = coords1.detach()
            corr = corr_fn(coords1)
            net, up_mask, delta_flow = self.update_block(net, inp, corr, coords1 - coords0)
            coords1 = coords1 + delta_flow
            if up_mask is None:
                flow_up = 8 * F.interpolate(coords1 - coords0, size=(H, W), mode="bilinear", align_corners=True)
            else:
                flow_up = upsample_flow(coords1 - coords0, up_mask)
                if cap is not None:
                    cap["up_mask_last"] = up_mask
            preds.append(flow_up)
        return (coords1 - coords0, flow_up) if test_mode else preds


def sequence_loss_restated(preds, flow_gt, valid, gamma=0.8, max_flow=400):
    """RAFT/train.py's sequence_loss, its sums in float64"""
    mag = torch.sum(flow_gt.double() ** 2, dim=1).sqrt()
    ok = ((valid >= 0.5) & (mag < max_flow))[:, None].double()
    loss = 0.0
    for i, p in enumerate(preds):
        loss = loss + gamma ** (len(preds) - i - 1) * (ok * (p.double() - flow_gt.double()).abs()).mean()
    return loss


# --------------------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 2, 1, 1), (2, 2, 1, 9), (2, 2, 5, 1), (2, 2, 3, 5), (2, 2, 16, 17)], ids=lambda s: "x".join(map(str, s)))
def test_gpu_upflow8_matches_the_formula_and_torch(shape, built, dev):
    from mpiflow_amd import raft_upsample
    N, _, H, W = shape
    rs = np.random.RandomState(31 + H * 100 + W)
    flow = (3.0 * rs.standard_normal(shape)).astype(np.float32)
    cot = rs.standard_normal((N, 2, 8 * H, 8 * W)).astype(np.float32)
    bar_f, bar_b = up8_bars(H, W, float(np.abs(flow).max()), float(np.abs(cot).max()))
    runs = []
    for _ in range(2):
        f = torch.from_numpy(flow).to(dev).requires_grad_(True)
        out = raft_upsample.upflow8(f)
        assert out.shape == (N, 2, 8 * H, 8 * W) and out.dtype == torch.float32 and out.is_contiguous()
        out.backward(torch.from_numpy(cot).to(dev))
        runs.append((out.detach(), f.grad))
    assert same_bytes(runs[0][0], runs[1][0]) and same_bytes(runs[0][1], runs[1][1])
    out, grad = runs[0]
    d_f = float(np.abs(out.double().cpu().numpy() - UP8(flow.astype(np.float64))).max())
    d_b = float(np.abs(grad.double().cpu().numpy() - UP8T(cot.astype(np.float64))).max())
    ft = torch.from_numpy(flow).to(dev).requires_grad_(True)
    want = 8 * F.interpolate(ft, size=(8 * H, 8 * W), mode="bilinear", align_corners=True)
    want.backward(torch.from_numpy(cot).to(dev))
    d_t = float((out.double() - want.detach().double()).abs().max())
    d_tb = float((grad.double() - ft.grad.double()).abs().max())
    print("upflow8 %-10s forward |hip - formula64| %.2e = %.3f of the bar %.2e, |hip - torch| %.2e; backward %.2e = %.3f of the bar %.2e, |hip - torch| %.2e"
          % ("x".join(map(str, shape)), d_f, d_f / bar_f, bar_f, d_t, d_b, d_b / bar_b, bar_b, d_tb))
    assert d_f <= bar_f and d_t <= bar_f and d_b <= bar_b and d_tb <= 2 * bar_b


@pytest.mark.gpu
@pytest.mark.parametrize("shape,hdim", [((2, 7, 3, 5), 3), ((2, 224, 16, 17), 128), ((1, 160, 16, 16), 96)], ids=["scalar_2x7x3x5", "basic_2x16x17", "small_1x16x16"])
def test_gpu_context_split_matches_torch(shape, hdim, built, raft, dev):
    rs = np.random.RandomState(47 + hdim)
    x = (2.0 * rs.standard_normal(shape)).astype(np.float32)
    x.reshape(-1)[::7] = 0.0                                            # exact zeros: relu's edge
    cdim = shape[1] - hdim
    g_net = rs.standard_normal((shape[0], hdim) + shape[2:]).astype(np.float32)
    g_inp = rs.standard_normal((shape[0], cdim) + shape[2:]).astype(np.float32)
    runs = []
    for _ in range(2):
        c = torch.from_numpy(x).to(dev).requires_grad_(True)
        net, inp = raft.context_split(c, hdim)
        assert net.shape == (shape[0], hdim) + shape[2:] and inp.shape == (shape[0], cdim) + shape[2:] and net.is_contiguous() and inp.is_contiguous()
        torch.autograd.backward([net, inp], [torch.from_numpy(g_net).to(dev), torch.from_numpy(g_inp).to(dev)])
        runs.append((net.detach(), inp.detach(), c.grad))
    for a, b in zip(*runs):
        assert same_bytes(a, b)
    net, inp, grad = runs[0]
    ct = torch.from_numpy(x).to(dev).requires_grad_(True)
    tn, ti = torch.split(ct, [hdim, cdim], dim=1)
    tn, ti = torch.tanh(tn), torch.relu(ti)
    torch.autograd.backward([tn, ti], [torch.from_numpy(g_net).to(dev), torch.from_numpy(g_inp).to(dev)])
    assert same_bytes(inp, ti.detach()), "inp is not torch's relu bit for bit"
    assert same_bytes(grad[:, hdim:], ct.grad[:, hdim:]), "the gradient of inp is not torch's bit for bit"
    x64 = x.astype(np.float64)
    d_n = float(np.abs(net.double().cpu().numpy() - np.tanh(x64[:, :hdim])).max())
    d_g = float(np.abs(grad[:, :hdim].double().cpu().numpy() - g_net.astype(np.float64) * (1.0 - np.tanh(x64[:, :hdim]) ** 2)).max())
    bar_n, bar_g = fmt_bar(1.0), fmt_bar(float(np.abs(g_net).max()))
    print("context_split %s net |hip - tanh64| %.2e = %.3f of FMT_BAR, its gradient %.2e = %.3f of FMT_BAR" % (shape, d_n, d_n / bar_n, d_g, d_g / bar_g))
    assert d_n <= bar_n and d_g <= bar_g


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 3, 5), (2, 3, 16, 24)], ids=["scalar_1x3x5", "vector_2x16x24"])
def test_gpu_raft_images_is_the_true_division_bit_for_bit(shape, built, dev):
    from mpiflow_amd import ops
    rs = np.random.RandomState(53)
    n = int(np.prod(shape))
    ints = np.resize(np.arange(256, dtype=np.float32), n).reshape(shape)
    for what, im1, im2 in (("0..255", ints, ints[..., ::-1].copy()), ("non-integers", (255.0 * rs.rand(*shape)).astype(np.float32), (300.0 * rs.rand(*shape) - 20.0).astype(np.float32))):
        a, b = torch.from_numpy(im1), torch.from_numpy(im2)
        pair = ops.raft_images(a.to(dev), b.to(dev))
        assert pair.shape == (2 * shape[0],) + shape[1:] and pair.is_contiguous()
        assert same_bytes(pair, ops.raft_images(a.to(dev), b.to(dev)))
        want = torch.cat([2 * (a / 255.0) - 1.0, 2 * (b / 255.0) - 1.0], dim=0)             # torch's CPU kernel: a true division
        on_device = torch.cat([2 * (a.to(dev) / 255.0) - 1.0, 2 * (b.to(dev) / 255.0) - 1.0], dim=0)
        diff = int((pair.view(torch.int32) != on_device.view(torch.int32)).sum())
        print("raft_images %s %-12s entries that differ from the device's own 2 * (x / 255.0) - 1.0 (a reciprocal multiply): %d of %d, max %.1e"
              % (shape, what, diff, 2 * n, float((pair - on_device).abs().max())))
        assert same_bytes(pair.cpu(), want), what
        # the two forms of x / 255 differ by at most 3 u |x / 255| (one rounding against three), |x / 255| < 1.2; doubled, plus the subtraction's rounding
        assert float((pair - on_device).abs().max()) <= 8 * U


_RUNS = {}


def _collect(c, model, preds, cap):
    res = {}
    if c["train"]:
        t = lambda a: torch.from_numpy(a).to(preds[0].device)
        loss = 0.0
        for i, p in enumerate(preds):
            res["pred_%d" % i] = p.detach()
            loss = loss + (p * t(c["d"]["cot_%d" % i])).sum()
        loss.backward()
        res.update({"grad_" + k: p.grad for k, p in model.named_parameters()})
    else:
        res["flow_coarse"], res["flow_up"] = preds[0].detach(), preds[1].detach()
    res.update({k: v.detach() for k, v in cap.items()})
    return res


def _prepare(c, model, dev, mk):
    assert mk.fill_params(model, c["seed"]) == c["sums"][1], "the seeded weights of %s are not the recorded ones" % c["name"]
    model.to(dev)
    if c["train"]:
        model.train()
    else:
        model.freeze_bn()
        model.eval()
    return model


def _run_model(c, raft, dev, mk, **kw):
    model = _prepare(c, raft.RAFT(argparse.Namespace(small=c["small"], mixed_precision=False, **kw)), dev, mk)
    t = lambda a: torch.from_numpy(a).to(dev)
    cap = {}

    def fnet_hook(mod, inputs, output):
        cap["fmap1"] = output[:c["N"]]

    def pre_hook(mod, inputs):
        if "net" not in cap:
            cap["net"], cap["inp"] = inputs[0], inputs[1]

    def out_hook(mod, inputs, output):
        if c["train"] and output[1] is not None:
            cap["up_mask_last"] = output[1]
    hooks = [model.fnet.register_forward_hook(fnet_hook), model.update_block.register_forward_pre_hook(pre_hook),
             model.update_block.register_forward_hook(out_hook)]
    if c["train"]:
        preds = model(t(c["d"]["image1"]), t(c["d"]["image2"]), iters=c["iters"])
        assert isinstance(preds, list) and len(preds) == c["iters"]
    else:
        with torch.no_grad():
            preds = model(t(c["d"]["image1"]), t(c["d"]["image2"]), iters=c["iters"], flow_init=t(c["d"]["flow_init"]), test_mode=True)
        assert isinstance(preds, tuple) and len(preds) == 2 and preds[0].shape == (c["N"], 2, c["H"] // 8, c["W"] // 8)
    for h in hooks:
        h.remove()
    return model, _collect(c, model, preds, cap)


def _run_parts(c, dev, mk):
    model = _prepare(c, PartsRAFT(argparse.Namespace(small=c["small"])), dev, mk)
    t = lambda a: torch.from_numpy(a).to(dev)
    cap = {}
    if c["train"]:
        preds = model(t(c["d"]["image1"]), t(c["d"]["image2"]), iters=c["iters"], cap=cap)
    else:
        with torch.no_grad():
            preds = model(t(c["d"]["image1"]), t(c["d"]["image2"]), iters=c["iters"], flow_init=t(c["d"]["flow_init"]), test_mode=True, cap=cap)
        cap.pop("up_mask_last", None)
    return _collect(c, model, preds, cap)


def sample_err(c, mk, key, val):
    s = c["rec"][key]
    return float(np.abs(val.double().cpu().numpy().reshape(-1)[mk.sample_index(val.numel(), c["seed"])] - s["f64"]).max())


def runs_of(c, raft, dev, mk):
    """the model under test and the parent's parts on one case, once per module: {key: (error of the model, error of the parts, bar)}"""
    if c["name"] not in _RUNS:
        _run_parts(c, dev, mk)                                           # unmeasured: see the module docstring
        model, got = _run_model(c, raft, dev, mk)
        parts = _run_parts(c, dev, mk)
        assert sorted(got) == sorted(parts) == sorted(c["keys"]), (sorted(set(got) ^ set(c["keys"])), sorted(set(parts) ^ set(c["keys"])))
        table = {}
        for key in c["keys"]:
            assert got[key].shape == parts[key].shape and got[key].dtype == torch.float32
            d, dp = sample_err(c, mk, key, got[key]), sample_err(c, mk, key, parts[key])
            table[key] = (d, dp, max(3 * c["rec"][key]["err32"], 2 * dp))
        _RUNS[c["name"]] = (model, got, table)
    return _RUNS[c["name"]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["basic/train_2x128x136", "basic/eval_1x128x128", "small/train_2x136x128", "small/eval_1x128x128"])
def test_gpu_model_matches_the_recorded_reference(name, golden, raft, dev):
    c = golden["cases"][name]
    _, _, table = runs_of(c, raft, dev, golden["mk"])
    worst = (0.0, None)
    for key in c["keys"]:
        d, dp, bar = table[key]
        s = c["rec"][key]
        print("model %-22s %-44s |hip - ref64| %.2e = %.2f err32 (%.2e); parts %.2e; absmax %.2e%s"
              % (name, key, d, d / s["err32"], s["err32"], dp, s["absmax"], "  [structurally zero]" if key[5:] in c["zero_grads"] else ""))
        worst = max(worst, (d / bar, key))
    print("model %-22s worst: %.3f of its bar (%s)" % (name, worst[0], worst[1]))
    for key in c["keys"]:
        d, dp, bar = table[key]
        assert d <= bar, (name, key, d, c["rec"][key]["err32"], dp)


@pytest.mark.gpu
def test_gpu_coarse_pairs_feed_sequence_loss(golden, raft, dev):
    from mpiflow_amd import raft_upsample
    c = golden["cases"]["basic/train_2x128x136"]
    mk = golden["mk"]
    _, _, table = runs_of(c, raft, dev, mk)
    rs = np.random.RandomState(c["seed"] + 3)
    t = lambda a: torch.from_numpy(a).to(dev)
    gt = t((10.0 * rs.standard_normal((c["N"], 2, c["H"], c["W"]))).astype(np.float32))
    valid = t((rs.rand(c["N"], c["H"], c["W"]) > 0.1).astype(np.float32))
    grads = []
    for coarse in (True, False):
        model = _prepare(c, raft.RAFT(mk.make_args(False)), dev, mk)
        out = model(t(c["d"]["image1"]), t(c["d"]["image2"]), iters=c["iters"], coarse=coarse)
        assert len(out) == c["iters"]
        if coarse:
            for flow, mask in out:
                assert flow.shape == (c["N"], 2, c["H"] // 8, c["W"] // 8) and mask.shape == (c["N"], 576, c["H"] // 8, c["W"] // 8)
            loss, metrics = raft_upsample.sequence_loss([f for f, _ in out], [m for _, m in out], gt, valid, gamma=0.8)
            assert sorted(metrics) == ["1px", "3px", "5px", "epe"]
        else:
            loss = sequence_loss_restated(out, gt, valid, gamma=0.8)
        loss.backward()
        grads.append((float(loss), {k: p.grad for k, p in model.named_parameters()}))
    (fused, g_fused), (plain, g_plain) = grads
    rel = abs(fused - plain) / abs(plain)
    print("coarse: loss fused %.9g, restated %.9g, rel %.2e = %.3f of the bar" % (fused, plain, rel, rel / LOSS_REL_BAR))
    worst, worst_rel = (0.0, None), (0.0, None)
    top = max(float(g.abs().max()) for g in g_plain.values())
    diffs = {k: float((g_fused[k].double() - g_plain[k].double()).abs().max()) for k in g_fused}
    for k, d in diffs.items():
        worst = max(worst, (d / table["grad_" + k][2], k))
        worst_rel = max(worst_rel, (d / top, k))
    print("coarse: parameter gradients, worst %.2e of its bar (%s); worst difference %.2e of the largest gradient %.2e (%s)"
          % (worst[0], worst[1], worst_rel[0], top, worst_rel[1]))
    assert rel <= LOSS_REL_BAR
    for k, d in diffs.items():
        assert d <= table["grad_" + k][2], (k, d, table["grad_" + k])


@pytest.mark.gpu
def test_gpu_alternate_corr_gives_the_all_pairs_predictions(golden, raft, dev):
    c = golden["cases"]["basic/eval_1x128x128"]
    mk = golden["mk"]
    _, got, table = runs_of(c, raft, dev, mk)
    model, alt = _run_model(c, raft, dev, mk, alternate_corr=True)
    assert model.args.alternate_corr is True
    for key in ("flow_coarse", "flow_up"):
        d = sample_err(c, mk, key, alt[key])
        print("alternate_corr %-12s |hip - ref64| %.2e = %.3f of the bar; |alt - all pairs| %.2e" % (key, d, d / table[key][2], float((alt[key] - got[key]).abs().max())))
        assert d <= table[key][2], (key, d, table[key])


@pytest.mark.gpu
def test_gpu_context_is_computed_once_per_forward_pass(golden, raft, dev):
    c = golden["cases"]["basic/eval_1x128x128"]
    model = _prepare(c, raft.RAFT(golden["mk"].make_args(False)), dev, golden["mk"])
    t = lambda a: torch.from_numpy(a).to(dev)
    assert model.update_block.hoist_context and model.update_block.context_computed == 0
    for n in (1, 2):
        with torch.no_grad():
            model(t(c["d"]["image1"]), t(c["d"]["image2"]), iters=12, test_mode=True)
        assert model.update_block.context_computed == n
