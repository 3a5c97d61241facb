"""RAFT's on-demand correlation lookup (mpiflow_amd/raft_corr.py, mpf_corr_lookup / mpf_corr_lookup_backward of mpf_corr.hip).

The reference is the reference's own CorrBlock (RAFT/core/corr.py), recorded on the CPU by tests/golden/make_corr_golden.py into
tests/golden/raft_corr.npz: fp32 and double runs, output and both gradients, and err32 = max |fp32 run - double run| per array - the
yardstick: the kernel must stay within 3 * err32 of the DOUBLE run.  The golden holds the inputs as seeds and 5000 sampled entries per array
(the double output of one case alone would be twice the size a committed file may have), so every comparison is made twice: at the sampled
entries against the recorded double run, and at EVERY entry against formula() below in float64, which the host test ties to those samples at
1e-12.  A missing golden fails these tests; it does not skip them.

Host tests: formula() against the golden; the C ABI's validation; the exported symbols; CPU tensors are refused.
GPU tests: golden forward / backward, a RAFT-sized case against the all-pairs form in float64 on the GPU, non-finite coordinates, the
extension-layout module functions and the `alt_cuda_corr` alias, peak memory, a side stream and two live blocks.

Measured on an MI355X (max |hip - ref64| / err32 per golden case; the bound is 3): see profiles/corr/README.md."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "raft_corr.npz")


def _maker():
    spec = importlib.util.spec_from_file_location("make_corr_golden", os.path.join(ROOT, "tests", "golden", "make_corr_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN, allow_pickle=False)                  # a missing file is an error here, not a skip
    mk = _maker()
    cases = {}
    for name in [str(n) for n in z["names"]]:
        C, H, W, L, r, seed = [int(v) for v in z[name + "/settings"]]
        f1, f2, g, _ = mk.case_inputs(C, H, W, L, r, seed, str(z[name + "/kind"]))
        sums = [a.astype(np.float64).sum() for a in (f1, f2, g)]
        assert np.array_equal(np.array(sums), z[name + "/input_sums"]), "the seeded inputs of %s are not the recorded ones" % name
        c = dict(name=name, C=C, H=H, W=W, L=L, r=r, f1=f1, f2=f2, g=g, coords=z[name + "/coords"],
                 zero=np.unpackbits(z[name + "/out_zero_bits"])[:g.size].astype(bool).reshape(g.shape))
        for key in ("out", "grad_fmap1", "grad_fmap2"):
            n = {"out": g.size, "grad_fmap1": f1.size, "grad_fmap2": f2.size}[key]
            c[key] = dict(idx=mk.sample_index(n, seed), f32=z["%s/%s_f32" % (name, key)], f64=z["%s/%s_f64" % (name, key)],
                          err32=float(z["%s/%s_err32" % (name, key)]), absmax=float(z["%s/%s_absmax" % (name, key)]))
        cases[name] = c
    assert len(cases) == 4
    return cases


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


def formula(f1, f2, coords, L, r):
    """The lookup as the issue states it, on pooled feature maps, in the dtype / on the device of its inputs, differentiable:
        out[b, i*rd^2 + a*rd + c, y, x] = 1/sqrt(C) * sum_ch f1[b,ch,y,x] * bilinear(f2_i[b,ch], cx/2^i + a - r, cy/2^i + c - r)
    with bilinear = the four integer taps around (floor X, floor Y), a tap outside f2_i = 0.  The sum over channels is taken first (V = all
    products of f1 with the level's map: the level is tiny next to C), the four-tap blend second; the two commute.  1/sqrt(C) is RAFT's:
    the square root is taken in float32.  No grid_sample, no code of the reference."""
    B, C, H, W = f1.shape
    rd = 2 * r + 1
    root = torch.sqrt(torch.tensor(C).float()).to(f1.dtype).to(f1.device)
    a1 = f1.reshape(B, C, H * W).transpose(1, 2)                         # [B, HW, C]
    d = torch.arange(-r, r + 1, device=f1.device, dtype=f1.dtype)
    outs = []
    lvl = f2
    for i in range(L):
        if i:
            lvl = F.avg_pool2d(lvl, 2, stride=2)
        Hl, Wl = lvl.shape[-2:]
        V = torch.matmul(a1, lvl.reshape(B, C, Hl * Wl)) / root             # [B, HW, Hl*Wl]
        X = (coords[:, 0].reshape(B, H * W) / 2 ** i)[:, :, None, None] + d[None, None, :, None]      # [B, HW, a, 1]: a moves x
        Y = (coords[:, 1].reshape(B, H * W) / 2 ** i)[:, :, None, None] + d[None, None, None, :]      # [B, HW, 1, c]: c moves y
        X, Y = X.expand(B, H * W, rd, rd), Y.expand(B, H * W, rd, rd)
        x0, y0 = torch.floor(X), torch.floor(Y)
        fx, fy = X - x0, Y - y0
        acc = torch.zeros(B, H * W, rd, rd, dtype=f1.dtype, device=f1.device)
        for dy, wy in ((0, 1 - fy), (1, fy)):
            for dx, wx in ((0, 1 - fx), (1, fx)):
                xi, yi = x0 + dx, y0 + dy
                inside = (xi >= 0) & (xi <= Wl - 1) & (yi >= 0) & (yi <= Hl - 1)
                idx = (yi.clamp(0, Hl - 1) * Wl + xi.clamp(0, Wl - 1)).long().reshape(B, H * W, rd * rd)
                tap = torch.gather(V, 2, idx).reshape(B, H * W, rd, rd)
                acc = acc + torch.where(inside, wx * wy * tap, torch.zeros_like(tap))
        outs.append(acc.reshape(B, H, W, rd * rd))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def allpairs(f1, f2, coords, L, r):
    """The all-pairs form (what CorrBlock computes), restated: the (HW)^2 volume by matmul, its avg_pool2d pyramid, grid_sample lookups."""
    B, C, H, W = f1.shape
    vol = torch.matmul(f1.reshape(B, C, H * W).transpose(1, 2), f2.reshape(B, C, H * W)) / torch.sqrt(torch.tensor(C).float()).to(f1)
    vol = vol.reshape(B * H * W, 1, H, W)
    d = torch.linspace(-r, r, 2 * r + 1, device=f1.device, dtype=f1.dtype)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1)        # delta[a, c] = (d[a], d[c]) is added to (x, y): a moves x
    cen = coords.permute(0, 2, 3, 1).reshape(B * H * W, 1, 1, 2)
    outs = []
    for i in range(L):
        if i:
            vol = F.avg_pool2d(vol, 2, stride=2)
        h, w = vol.shape[-2:]
        p = cen / 2 ** i + delta[None]
        grid = torch.stack([2 * p[..., 0] / (w - 1) - 1, 2 * p[..., 1] / (h - 1) - 1], dim=-1)
        outs.append(F.grid_sample(vol, grid, align_corners=True).reshape(B, H, W, -1))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def with_grads(fn, f1, f2, coords, g, L, r):
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    out = fn(a, b, coords, L, r)
    out.backward(g)
    return out.detach(), a.grad, b.grad


def t64(a):
    return torch.from_numpy(np.asarray(a)).double()


# ---------------------------------------------------------------------------------------------------------------- host


def test_formula_equals_the_recorded_reference(golden):
    """formula() in float64 == CorrBlock on double inputs at the sampled entries to 1e-12 of the array's largest entry (output and both
    gradients); formula() in float32 is within 3 * err32 of the double run; the entries the reference reports as exactly 0 are exactly 0."""
    for c in golden.values():
        res64 = with_grads(formula, t64(c["f1"]), t64(c["f2"]), t64(c["coords"]), t64(c["g"]), c["L"], c["r"])
        res32 = with_grads(formula, *[torch.from_numpy(c[k]) for k in ("f1", "f2", "coords", "g")], c["L"], c["r"])
        for key, v64, v32 in zip(("out", "grad_fmap1", "grad_fmap2"), res64, res32):
            s = c[key]
            d64 = np.abs(v64.numpy().reshape(-1)[s["idx"]] - s["f64"]).max()
            d32 = np.abs(v32.numpy().astype(np.float64).reshape(-1)[s["idx"]] - s["f64"]).max()
            full32 = np.abs(v32.numpy().astype(np.float64) - v64.numpy()).max()
            print("%-24s %-10s |f64 - ref64| %.2e (max %.2f)   |f32 - ref64| %.2e = %.2f err32   every entry |f32 - f64| %.2f err32"
                  % (c["name"], key, d64, s["absmax"], d32, d32 / s["err32"], full32 / s["err32"]))
            assert d64 <= 1e-12 * s["absmax"], (c["name"], key, d64)
            assert d32 <= 3 * s["err32"] and full32 <= 3 * s["err32"], (c["name"], key, d32, full32, s["err32"])
        assert c["zero"].any() and (res64[0].numpy()[c["zero"]] == 0).all() and (res32[0].numpy()[c["zero"]] == 0).all()


def test_first_window_index_moves_x():
    """channel a*rd + c looks at (x + a - r, y + c - r): one hot feature at (y, x) = (5, 9) is found by the query at (5, 6) in channel a = r + 3"""
    f1 = torch.zeros(1, 32, 16, 16, dtype=torch.float64)
    f2 = torch.zeros(1, 32, 16, 16, dtype=torch.float64)
    f1[0, 0, 5, 6], f2[0, 0, 5, 9] = 1.0, 1.0
    ys, xs = torch.meshgrid(torch.arange(16.0), torch.arange(16.0), indexing="ij")
    out = formula(f1, f2, torch.stack([xs, ys])[None].double(), 1, 4)
    hot = out[0, :, 5, 6].nonzero().flatten().tolist()
    assert hot == [(4 + 3) * 9 + 4]


def _args(built, **kw):
    a = built.MpfCorrArgs()
    one = 256
    a.fmap1 = a.coords = a.out = a.grad_fmap1 = one
    a.B, a.C, a.H, a.W, a.radius, a.levels, a.scale = 1, 64, 16, 24, 4, 4, 0.125
    for i in range(4):
        a.f2[i], a.grad_f2[i], a.Hl[i], a.Wl[i] = one, one, 16 >> i, 24 >> i
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def test_c_abi_refuses_bad_arguments(built):
    """validated before anything is launched: no GPU is needed to be told so.  Status 10001 and a message that names the argument."""
    lib = built.load()
    bad = [(dict(fmap1=None), b"fmap1"), (dict(coords=None), b"coords"), (dict(out=None), b"out"), (dict(f2=(2, None)), b"f2[2]"),
           (dict(C=48), b"C must be a multiple of 32"), (dict(C=0), b"C must be"), (dict(Hl=(3, 1)), b"Hl[3]"), (dict(Wl=(3, 1)), b"Wl[3]"),
           (dict(radius=0), b"radius"), (dict(radius=9), b"radius"), (dict(levels=0), b"levels"), (dict(levels=7), b"levels"),
           (dict(fmap1=260), b"fmap1 must be 16-byte aligned"), (dict(B=0), b"bad shape"), (dict(scale=float("nan")), b"scale"), (dict(plain=2), b"plain")]
    for fn in (lib.mpf_corr_lookup, lib.mpf_corr_lookup_backward):
        assert fn(None, None) == 10001 and b"null argument block" in lib.mpf_last_error()
        for kw, word in bad:
            assert fn(ctypes.byref(_args(built, **kw)), None) == 10001, kw
            assert word in lib.mpf_last_error(), (kw, lib.mpf_last_error())
    for kw, word in ((dict(grad_fmap1=None), b"grad_fmap1"), (dict(grad_f2=(1, None)), b"grad_f2[1]")):
        assert lib.mpf_corr_lookup_backward(ctypes.byref(_args(built, **kw)), None) == 10001 and word in lib.mpf_last_error()


def test_both_libraries_export_both_symbols(built):
    for path in (built.LIB_PATH, built.WITNESS_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for n in ("mpf_corr_lookup", "mpf_corr_lookup_backward", "k_corr_forward", "k_corr_backward"):
            assert n in syms, (path, n)
    assert built.load().mpf_version() == 601


def test_cpu_tensors_and_bad_shapes_are_refused(built):
    from mpiflow_amd import ops, raft_corr
    f = torch.zeros(1, 32, 16, 16)
    with pytest.raises(built.MpiFlowHipError, match="no CPU path"):
        raft_corr.AlternateCorrBlock(f, f)
    with pytest.raises(built.MpiFlowHipError, match="no CPU path"):
        ops.corr_lookup(f.permute(0, 2, 3, 1).contiguous(), [f.permute(0, 2, 3, 1).contiguous()], torch.zeros(1, 2, 16, 16), 4)
    with pytest.raises(built.MpiFlowHipError, match="no CPU path"):
        raft_corr.forward(f, f, torch.zeros(1, 1, 32, 16, 2), 4)


# ----------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rc(built):
    from mpiflow_amd import raft_corr
    return raft_corr


def hip_with_grads(rc, f1, f2, coords, g, L, r):
    a, b, c = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True), coords.clone().requires_grad_(True)
    out = rc.AlternateCorrBlock(a, b, num_levels=L, radius=r)(c)
    out.backward(g)
    assert c.grad is None                                    # no gradient for coords: the autograd function returns None there
    return out.detach(), a.grad, b.grad


def check_case(c, key, hip, full64, what):
    """the rule of the issue, twice: sampled entries against the recorded double run, every entry against formula() in float64"""
    s = c[key]
    hip = hip.double().cpu().numpy()
    d_s = np.abs(hip.reshape(-1)[s["idx"]] - s["f64"]).max()
    d_f = np.abs(hip - full64.numpy()).max()
    print("%s %-24s %-10s |hip - ref64| sampled %.2e = %.2f err32, every entry vs formula64 %.2e = %.2f err32 (err32 %.2e)"
          % (what, c["name"], key, d_s, d_s / s["err32"], d_f, d_f / s["err32"], s["err32"]))
    assert d_s <= 3 * s["err32"] and d_f <= 3 * s["err32"], (c["name"], key, d_s, d_f, s["err32"])


@pytest.mark.gpu
def test_gpu_forward_matches_the_recorded_reference(golden, rc, dev):
    from mpiflow_amd import ops
    for c in golden.values():
        f1, f2, co = [torch.from_numpy(c[k]).to(dev) for k in ("f1", "f2", "coords")]
        blk = rc.AlternateCorrBlock(f1, f2, num_levels=c["L"], radius=c["r"])
        out = blk(co)
        assert out.shape == c["g"].shape and out.dtype == torch.float32 and out.is_contiguous()
        want = formula(t64(c["f1"]), t64(c["f2"]), t64(c["coords"]), c["L"], c["r"])
        check_case(c, "out", out, want, "forward")
        assert (out.cpu().numpy()[c["zero"]] == 0).all()
        plain = ops.corr_lookup(blk.fmap1_nhwc, blk.f2_levels_nhwc, co, c["r"], plain=True)          # the first form of the kernel: same contract
        check_case(c, "out", plain, want, "plain  ")
        assert (plain.cpu().numpy()[c["zero"]] == 0).all()


@pytest.mark.gpu
def test_gpu_backward_matches_the_recorded_reference(golden, rc, dev):
    """grad_fmap2 is the SCATTER form (fp32 atomics): two runs agree within err32_grad, not bit for bit; grad_fmap1 is bit-identical."""
    for c in golden.values():
        args = [torch.from_numpy(c[k]).to(dev) for k in ("f1", "f2", "coords", "g")]
        _, w1, w2 = with_grads(formula, t64(c["f1"]), t64(c["f2"]), t64(c["coords"]), t64(c["g"]), c["L"], c["r"])
        _, a1, a2 = hip_with_grads(rc, *args, c["L"], c["r"])
        check_case(c, "grad_fmap1", a1, w1, "backward")
        check_case(c, "grad_fmap2", a2, w2, "backward")
        _, b1, b2 = hip_with_grads(rc, *args, c["L"], c["r"])
        assert torch.equal(a1, b1)
        d = float((a2.double() - b2.double()).abs().max())
        print("backward %-24s two runs: grad_fmap1 identical, grad_fmap2 differ by %.2e (err32 %.2e)" % (c["name"], d, c["grad_fmap2"]["err32"]))
        assert d <= c["grad_fmap2"]["err32"]


@pytest.mark.gpu
def test_gpu_raft_sized_case_against_all_pairs_in_float64(rc, dev):
    """B = 2, C = 256, 48 x 160, L = 4, r = 4 (the generator's frames at 1/8): within 3 x the distance of the float32 all-pairs form from
    the float64 one, forward and both gradients."""
    B, C, H, W, L, r = 2, 256, 48, 160, 4, 4
    gen = torch.Generator(device="cpu").manual_seed(77)
    f1, f2 = [torch.randn(B, C, H, W, generator=gen).to(dev) for _ in range(2)]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    coords = (torch.stack([xs, ys])[None] + 6.0 * torch.randn(B, 2, H, W, generator=gen)).to(dev)
    g = torch.randn(B, L * 81, H, W, generator=gen).to(dev)
    ref64 = with_grads(allpairs, f1.double(), f2.double(), coords.double(), g.double(), L, r)
    ref32 = with_grads(allpairs, f1, f2, coords, g, L, r)
    hip = hip_with_grads(rc, f1, f2, coords, g, L, r)
    for key, w64, w32, h in zip(("out", "grad_fmap1", "grad_fmap2"), ref64, ref32, hip):
        e32 = float((w32.double() - w64).abs().max())
        d = float((h.double() - w64).abs().max())
        print("raft-sized %-10s |hip - allpairs64| %.2e = %.2f x |allpairs32 - allpairs64| (%.2e)" % (key, d, d / e32, e32))
        assert d <= 3 * e32, (key, d, e32)


@pytest.mark.gpu
def test_gpu_non_finite_and_huge_coordinates(rc, dev):
    """NaN, +-inf, +-1e30 in 10 % of the pixels: outputs and gradient contributions of those pixels are 0; every other pixel equals, bit for
    bit, the run in which those pixels' coordinates are a far-outside finite value.  grad_fmap2 is a sum of fp32 atomics whose order varies:
    there the two runs agree to reordering error, bounded here by 64 ulp of the largest entry (sums of at most a few hundred terms of
    either sign: reordering moves a sum by about sqrt(n) ulp of its largest partial sum)."""
    B, C, H, W, L, r = 2, 64, 32, 48, 4, 4
    gen = torch.Generator(device="cpu").manual_seed(5)
    f1, f2 = [torch.randn(B, C, H, W, generator=gen) for _ in range(2)]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([xs, ys])[None] + 3.0 * torch.randn(B, 2, H, W, generator=gen)
    g = torch.randn(B, L * 81, H, W, generator=gen)
    bad = torch.rand(B, H, W, generator=gen) < 0.1
    vals = torch.tensor([float("nan"), float("inf"), float("-inf"), 1e30, -1e30])
    pick = vals[torch.randint(0, 5, (B, 2, H, W), generator=gen)]
    axis = torch.randint(0, 3, (B, H, W), generator=gen)                  # 0: x only, 1: y only, 2: both
    hit = torch.stack([bad & (axis != 1), bad & (axis != 0)], dim=1)
    wild = torch.where(hit, pick, base)
    tame = torch.where(bad[:, None].expand_as(base), torch.full_like(base, -1e6), base)
    assert int(bad.sum()) > 100 and torch.isnan(wild).any() and torch.isinf(wild).any()
    to = lambda t: t.to(dev)
    ow, w1, w2 = hip_with_grads(rc, to(f1), to(f2), to(wild), to(g), L, r)
    ot, t1, t2 = hip_with_grads(rc, to(f1), to(f2), to(tame), to(g), L, r)
    torch.cuda.synchronize()
    badd = to(bad)
    assert (ow.permute(0, 2, 3, 1)[badd] == 0).all() and (w1.permute(0, 2, 3, 1)[badd] == 0).all()
    assert torch.equal(ow, ot) and torch.equal(w1, t1)
    assert torch.isfinite(ow).all() and torch.isfinite(w1).all() and torch.isfinite(w2).all()
    d = float((w2 - t2).abs().max())
    print("non-finite: grad_fmap2 of the two runs differ by %.2e, largest entry %.2f" % (d, float(t2.abs().max())))
    assert d <= 64 * 2.0 ** -23 * float(t2.abs().max())
    assert float(ot.abs().max()) > 0.5 and float(t2.abs().max()) > 0.5


@pytest.mark.gpu
def test_gpu_extension_layout_and_alias(golden, rc, dev):
    """forward / backward in alt_cuda_corr's layouts == the class up to 1/sqrt(C) and the permutes; with the module aliased as `alt_cuda_corr`
    the reference's AlternateCorrBlock logic (restated: pyramid, permutes, forward per level, stack, scale) reproduces the class's output."""
    import importlib
    c = golden["c128_16x24"]
    L, r, C = c["L"], c["r"], c["C"]
    f1, f2, co, g = [torch.from_numpy(c[k]).to(dev) for k in ("f1", "f2", "coords", "g")]
    want = rc.AlternateCorrBlock(f1, f2, num_levels=L, radius=r)(co)
    sys.modules["alt_cuda_corr"] = rc
    try:
        ext = importlib.import_module("alt_cuda_corr")
        pyr = [f2]
        for _ in range(L - 1):
            pyr.append(F.avg_pool2d(pyr[-1], 2, stride=2))
        nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
        cl = co.permute(0, 2, 3, 1)
        per = [ext.forward(nhwc(f1), nhwc(pyr[i]), (cl / 2 ** i).reshape(1, 1, c["H"], c["W"], 2).contiguous(), r)[0].squeeze(1) for i in range(L)]
        got = torch.stack(per, dim=1).reshape(1, -1, c["H"], c["W"]) / torch.sqrt(torch.tensor(C).float())
    finally:
        del sys.modules["alt_cuda_corr"]
    assert per[0].shape == (1, 81, c["H"], c["W"])
    # the extension returns unscaled sums and the caller divides; the class multiplies by the rounded reciprocal inside the kernel: two roundings apart
    assert float((got - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max())
    check_case(c, "out", got, formula(t64(c["f1"]), t64(c["f2"]), t64(c["coords"]), L, r), "alias  ")
    # backward of level 0 in the extension's layout against the kernel's own gradient for a one-level block
    g0 = g[:, :81].contiguous()
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    rc.AlternateCorrBlock(a, b, num_levels=1, radius=r)(co).backward(g0)
    e1, e2, e3 = rc.backward(nhwc(f1), nhwc(f2), cl.reshape(1, 1, c["H"], c["W"], 2).contiguous(), g0[:, None].contiguous(), r)
    s = float(torch.sqrt(torch.tensor(C).float()))
    assert e3.shape == (1, 1, c["H"], c["W"], 2) and not e3.any()
    tol = c["grad_fmap2"]["err32"]
    assert float((e1.permute(0, 3, 1, 2) / s - a.grad).abs().max()) <= tol and float((e2.permute(0, 3, 1, 2) / s - b.grad).abs().max()) <= tol


@pytest.mark.gpu
def test_gpu_peak_memory_is_linear_in_the_frame(rc, dev):
    """B = 1, C = 256, 128 x 192, L = 4, r = 4: construction + one lookup + backward allocate at most twice the channel-last copies, the
    output, its cotangent and the gradients (about 190 MB; the all-pairs pyramid is 3.2 GB)."""
    B, C, H, W, L, r = 1, 256, 128, 192, 4, 4
    f1 = torch.randn(B, C, H, W, device=dev).requires_grad_(True)
    f2 = torch.randn(B, C, H, W, device=dev).requires_grad_(True)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev), indexing="ij")
    coords = (torch.stack([xs, ys])[None] + 4.0 * torch.randn(B, 2, H, W, device=dev)).contiguous()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    out = rc.AlternateCorrBlock(f1, f2, num_levels=L, radius=r)(coords)
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated(dev) - before
    grads = f1.grad.numel() + f2.grad.numel()
    budget = 4 * (B * H * W * (2 * C * (1 + 1 / 4 + 1 / 16 + 1 / 64) + 2 * L * 81) + grads)
    print("peak memory %.1f MB, budget 2 x %.1f MB, all-pairs pyramid %.0f MB" % (used / 1e6, budget / 1e6, B * (H * W) ** 2 * 4 * (1 + 1 / 4 + 1 / 16 + 1 / 64) / 1e6))
    assert used <= 2 * budget, (used, budget)


@pytest.mark.gpu
def test_gpu_side_stream_and_two_live_blocks(golden, rc, dev):
    """lookups on a non-default stream while another stream is busy, and two blocks alive at once (each holds its own maps; the kernels keep
    no scratch between calls): both give what they give alone on the default stream."""
    ca, cb = golden["c128_16x24"], golden["c64_17x29_r3_l2"]
    alone = {}
    for c in (ca, cb):
        alone[c["name"]] = hip_with_grads(rc, *[torch.from_numpy(c[k]).to(dev) for k in ("f1", "f2", "coords", "g")], c["L"], c["r"])
    torch.cuda.synchronize()
    busy, side = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    big = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(busy):
        for _ in range(20):
            big = big @ big * 1e-3
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ta = [torch.from_numpy(ca[k]).to(dev) for k in ("f1", "f2", "coords", "g")]
        tb = [torch.from_numpy(cb[k]).to(dev) for k in ("f1", "f2", "coords", "g")]
        A = rc.AlternateCorrBlock(ta[0].requires_grad_(True), ta[1].requires_grad_(True), num_levels=ca["L"], radius=ca["r"])
        Bk = rc.AlternateCorrBlock(tb[0].requires_grad_(True), tb[1].requires_grad_(True), num_levels=cb["L"], radius=cb["r"])
        oa1, ob, oa2 = A(ta[2]), Bk(tb[2]), A(ta[2])               # interleaved lookups of the two live blocks
        (oa1 + oa2).backward(ta[3] * 0.5)
        ob.backward(tb[3])
    side.synchronize()
    busy.synchronize()
    assert torch.equal(oa1.detach(), alone[ca["name"]][0]) and torch.equal(oa2.detach(), oa1.detach()) and torch.equal(ob.detach(), alone[cb["name"]][0])
    assert torch.equal(ta[0].grad, alone[ca["name"]][1]) and torch.equal(tb[0].grad, alone[cb["name"]][1])
    for t, c in ((ta[1], ca), (tb[1], cb)):
        assert float((t.grad - alone[c["name"]][2]).abs().max()) <= c["grad_fmap2"]["err32"]
