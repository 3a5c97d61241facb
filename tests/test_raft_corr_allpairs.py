"""RAFT's all-pairs CorrBlock (mpiflow_amd/raft_corr.py: CorrBlock; mpf_corr_pyramid, mpf_corr_volume_lookup, mpf_corr_volume_lookup_backward,
mpf_corr_pyramid_backward of mpf_corr_volume.hip).

The reference is the one tests/test_raft_corr.py uses, and so is the bar: tests/golden/raft_corr.npz IS the reference's CorrBlock (fp32 and
double runs, output and both gradients, err32 = max |fp32 run - double run| per array); the block must stay within 3 * err32 of the DOUBLE
run, at the sampled entries against the recording and at every entry against formula() in float64.  The golden, its maker and the helpers
(formula, allpairs, with_grads, check_case, the fixtures) are loaded from the existing files by path; a missing golden fails, it does not skip.

Host tests: exported symbols and kernels; header, ctypes table and struct layout; the C ABI's validation; the Python layer's refusals.
GPU tests: the pyramid; forward / backward on the golden; a training-shaped step of twelve dependent lookups on one block (the shared gradient
pyramid); reproducibility; the gradient buffer's life cycle; non-finite coordinates; peak memory.

Measured on an MI355X: see profiles/corr/README.md."""
import ctypes
import importlib.util
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _load("raft_corr_ondemand_tests", "tests", "test_raft_corr.py")
golden, built, dev, rc = T.golden, T.built, T.dev, T.rc     # the fixtures of the existing file: the golden cases, the built library, cuda:0, raft_corr
formula, allpairs, with_grads, check_case, t64 = T.formula, T.allpairs, T.with_grads, T.check_case, T.t64

ENTRY_POINTS = ("mpf_corr_pyramid", "mpf_corr_volume_lookup", "mpf_corr_volume_lookup_backward", "mpf_corr_pyramid_backward")


def root_of(C):
    return float(torch.sqrt(torch.tensor(C).float()))


# ---------------------------------------------------------------------------------------------------------------- host


def test_both_libraries_export_the_entry_points_and_kernels(built):
    for path in (built.LIB_PATH, built.WITNESS_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for n in ENTRY_POINTS + ("k_cv_pyramid", "k_cv_lookup", "k_cv_lookup_backward", "k_cv_fold"):
            assert n in syms, (path, n)
    assert built.load().mpf_version() == 601


def test_header_ctypes_table_and_struct_layout_agree(built, tmp_path):
    """the four declarations are in the header and in SIGNATURES with the struct pointer; the ctypes struct has the C struct's size and field offsets"""
    hdr = open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read()
    for n in ENTRY_POINTS:
        assert "int %s(const MpfCorrVolumeArgs *a, void *stream);" % n in hdr
        assert built.SIGNATURES[n] == (ctypes.c_int, [ctypes.POINTER(built.MpfCorrVolumeArgs), ctypes.c_void_p])
    fields = [f[0] for f in built.MpfCorrVolumeArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpiflow_hip.h"\nint main(void) { printf("%zu", sizeof(MpfCorrVolumeArgs));\n'
                   + "".join('printf(" %%zu", offsetof(MpfCorrVolumeArgs, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(built.MpfCorrVolumeArgs)] + [getattr(built.MpfCorrVolumeArgs, f).offset for f in fields]


def _args(built, H=16, W=24, levels=4, **kw):
    a = built.MpfCorrVolumeArgs()
    one = 256
    a.coords = a.out = one
    a.B, a.H, a.W, a.radius, a.levels, a.norm = 1, H, W, 4, levels, 8.0
    for i in range(4):
        a.level[i], a.Hl[i], a.Wl[i] = one, max(H, 0) >> i, max(W, 0) >> i
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def test_c_abi_refuses_bad_arguments(built):
    """validated before anything is launched: no GPU is needed to be told so.  Status 10001 and a message that names the entry point and the argument."""
    lib = built.load()
    every = [(dict(level=(2, None)), b"level[2]"), (dict(level=(1, 258)), b"level[1] must be"), (dict(levels=0), b"levels"),
             (dict(levels=7), b"levels"), (dict(B=0), b"bad shape"), (dict(H=0), b"bad shape"), (dict(W=-1), b"bad shape"),
             (dict(Hl=(1, 9)), b"Hl[1]"), (dict(Wl=(2, 5)), b"Wl[2]"), (dict(Hl=(0, 15)), b"Hl[0]"),
             (dict(H=8), b"Hl[3] x Wl[3] = 1 x 3"), (dict(W=15), b"Hl[3] x Wl[3] = 2 x 1"),          # H or W below 2^levels
             (dict(H=1 << 15, W=1 << 15), b"too large")]
    lookups = [(dict(coords=None), b"coords"), (dict(out=None), b"out"), (dict(radius=0), b"radius"), (dict(radius=9), b"radius"),
               (dict(level=(1, 258)), b"level[1] must be 4-byte aligned")]
    pyramids = [(dict(norm=0.0), b"norm"), (dict(norm=float("nan")), b"norm"), (dict(norm=float("inf")), b"norm"),
                (dict(level=(1, 260)), b"level[1] must be 16-byte aligned"),
                (dict(levels=1, W=12292), b"W * 2^(levels-1)")]
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)
        assert fn(None, None) == 10001 and b"null argument block" in lib.mpf_last_error()
        for kw, word in every + (lookups if "lookup" in name else pyramids):
            assert fn(ctypes.byref(_args(built, **kw)), None) == 10001, (name, kw)
            assert name.encode() + b":" in lib.mpf_last_error() and word in lib.mpf_last_error(), (name, kw, lib.mpf_last_error())


def test_python_layer_refuses_what_it_cannot_run(built):
    """CPU tensors, half precision, non-contiguous maps, mismatched shapes, H or W below 2^L: MpiFlowHipError from CorrBlock and from the four
    ops functions; nothing is copied, cast or computed in torch instead."""
    from mpiflow_amd import ops, raft_corr
    E = built.MpiFlowHipError
    f = torch.zeros(1, 32, 16, 24)
    with pytest.raises(E, match="no CPU path"):
        raft_corr.CorrBlock(f, f)
    with pytest.raises(E, match="float32"):
        raft_corr.CorrBlock(f.half(), f.half())
    with pytest.raises(E, match="float32"):
        raft_corr.CorrBlock(f, f.double())
    with pytest.raises(E, match="contiguous"):
        raft_corr.CorrBlock(f.transpose(2, 3), f.transpose(2, 3))
    with pytest.raises(E, match="contiguous"):
        raft_corr.CorrBlock(f[0], f[0])
    with pytest.raises(E, match="must agree"):
        raft_corr.CorrBlock(f, torch.zeros(1, 32, 16, 16))
    for shape in ((1, 32, 15, 24), (1, 32, 16, 15)):
        with pytest.raises(E, match="at least 2\\^num_levels"):
            raft_corr.CorrBlock(torch.zeros(shape), torch.zeros(shape))
    assert raft_corr.CorrBlock.__init__.__defaults__ == (4, 4)
    for bad in (dict(num_levels=0), dict(num_levels=7), dict(radius=0), dict(radius=9)):
        with pytest.raises(E, match="must be 1\\.\\."):
            raft_corr.CorrBlock(f, f, **bad)
    raw = torch.zeros(16 * 24, 16, 24)
    lv = [torch.zeros(16 * 24, 16 >> i, 24 >> i) for i in range(4)]
    co, g = torch.zeros(1, 2, 16, 24), torch.zeros(1, 4 * 81, 16, 24)
    calls = (lambda t=raw, l=lv: ops.corr_pyramid(t, 4, 8.0), lambda t=raw, l=lv: ops.corr_volume_lookup(l, co, 4),
             lambda t=raw, l=lv: ops.corr_volume_lookup_backward(l, co, g, 4), lambda t=raw, l=lv: ops.corr_pyramid_backward(l, 8.0))
    for call in calls:
        with pytest.raises(E, match="no CPU path"):
            call()
        with pytest.raises(E, match="float32"):
            call(raw.half(), [t.half() for t in lv])
        with pytest.raises(E, match="contiguous"):
            call(raw.transpose(1, 2), [t.transpose(1, 2) for t in lv])
        with pytest.raises(E, match="dimensions"):
            call(raw[None], [t[None] for t in lv])


def shape_refusals(ops, dev):
    """(call, words of the message) for every way the tensors of the four ops functions can disagree with each other, on `dev`, and the
    tensors themselves.  The C ABI sees bare pointers: these refusals are what ties a tensor's real size to what the kernels index."""
    z = lambda *shape: torch.full(shape, 7.0, device=dev)
    N, H, W, L, r = 2 * 16 * 24, 16, 24, 4, 4
    lv = [z(N, H >> i, W >> i) for i in range(L)]
    co, g, out = z(2, 2, H, W), z(2, L * 81, H, W), z(2, L * 81, H, W)
    swap = lambda i, t: lv[:i] + [t] + lv[i + 1:]
    small = [z(2 * 8 * 24, 8 >> i, 24 >> i) for i in range(L)]             # H = 8 < 2^4
    narrow = [z(2 * 16 * 15, 16 >> i, 15 >> i) for i in range(L)]           # W = 15 < 2^4
    cases = []
    for name, fn in (("corr_volume_lookup", lambda l, c=co, rad=r, o=None: ops.corr_volume_lookup(l, c, rad, out=o)),
                     ("corr_volume_lookup_backward", lambda l, c=co, rad=r, o=g: ops.corr_volume_lookup_backward(l, c, o, rad)),
                     ("corr_pyramid_backward", lambda l: ops.corr_pyramid_backward(l, 8.0))):
        cases += [(lambda fn=fn: fn(swap(1, z(N - 1, 8, 12))), name + ": levels\\[1\\] must be"),          # another row count
                  (lambda fn=fn: fn(swap(2, z(N, 4, 5))), name + ": levels\\[2\\] must be"),               # not the pooled size
                  (lambda fn=fn: fn(swap(0, z(N + 1, H, W))), name + ": level 0 .* must hold B \\* H \\* W rows"),
                  (lambda fn=fn: fn(small), name + ": H, W = 8, 24 must be at least 2\\^num_levels"),
                  (lambda fn=fn: fn(narrow), name + ": H, W = 16, 15 must be at least 2\\^num_levels"),
                  (lambda fn=fn: fn([]), name + ": num_levels"), (lambda fn=fn: fn(lv + lv), name + ": num_levels")]
        if "lookup" in name:
            cases += [(lambda fn=fn: fn(lv, z(1, 2, H, W)), name + ": coords must be \\[B,2,H,W\\]"),       # B*H*W != N
                      (lambda fn=fn: fn(lv, z(2, 2, W, H)), name + ": coords must be"), (lambda fn=fn: fn(lv, z(2, 3, H, W)), name + ": coords must be"),
                      (lambda fn=fn: fn(lv, co, 0), name + ": radius"), (lambda fn=fn: fn(lv, co, 9), name + ": radius"),
                      (lambda fn=fn: fn(lv, co, r, z(2, L * 81, H, W + 1)), name + ": (out|grad_out) must be"),
                      (lambda fn=fn: fn(lv, co, 3, z(2, L * 81, H, W)), name + ": (out|grad_out) must be"),   # the output of another radius
                      (lambda fn=fn: fn(lv, co, r, z(1, L * 81, H, W)), name + ": (out|grad_out) must be")]
    cases += [(lambda: ops.corr_pyramid(z(N + 1, H, W), L, 8.0), "corr_pyramid: level 0 .* must hold"),
              (lambda: ops.corr_pyramid(z(N, H, W), 5, 8.0), "corr_pyramid: H, W = 16, 24 must be at least 2\\^num_levels = 32"),
              (lambda: ops.corr_pyramid(z(2 * 16 * 15, 16, 15), L, 8.0), "corr_pyramid: H, W = 16, 15 must be at least"),
              (lambda: ops.corr_pyramid(z(N, H, W), 0, 8.0), "corr_pyramid: num_levels"), (lambda: ops.corr_pyramid(z(N, H, W), 7, 8.0), "corr_pyramid: num_levels")]
    return cases, lv + [co, g, out]


def test_ops_refuse_tensors_that_disagree(built):
    """every shape refusal of the four ops functions, on the host: shapes are judged before the device, so CPU tensors can ask for each"""
    from mpiflow_amd import ops
    cases, _ = shape_refusals(ops, torch.device("cpu"))
    assert len(cases) > 40
    for call, words in cases:
        with pytest.raises(built.MpiFlowHipError, match=words):
            call()


# ----------------------------------------------------------------------------------------------------------------- GPU


def case_tensors(c, dev):
    return [torch.from_numpy(c[k]).to(dev) for k in ("f1", "f2", "coords", "g")]


def hip_with_grads(rc, f1, f2, coords, g, L, r):
    a, b, c = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True), coords.clone().requires_grad_(True)
    out = rc.CorrBlock(a, b, num_levels=L, radius=r)(c)
    out.backward(g)
    assert c.grad is None                                    # no gradient for coords: the autograd function returns None there
    return out.detach(), a.grad, b.grad


@pytest.mark.gpu
def test_gpu_tensors_that_disagree_are_refused_and_nothing_is_launched(golden, rc, dev, built):
    """the refusals of the host test on GPU tensors: MpiFlowHipError naming the function and the argument, and no buffer that was passed has
    changed; CorrBlock.__call__ with coordinates of another frame, batch, layout, dtype or device is refused the same way"""
    from mpiflow_amd import ops
    E = built.MpiFlowHipError
    cases, bufs = shape_refusals(ops, dev)
    for call, words in cases:
        with pytest.raises(E, match=words):
            call()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in bufs)
    with pytest.raises(E, match="no CPU path"):
        ops.corr_volume_lookup(bufs[:4], bufs[4].cpu(), 4)
    with pytest.raises(E, match="no CPU path"):
        ops.corr_volume_lookup_backward(bufs[:4], bufs[4], bufs[5].cpu(), 4)
    c = golden["c128_16x24"]
    f1, f2, co, _ = case_tensors(c, dev)
    blk = rc.CorrBlock(f1, f2, num_levels=c["L"], radius=c["r"])
    want = blk(co)
    for bad, words in ((co[:, :, :-1].contiguous(), "coords must be"), (co.repeat(2, 1, 1, 1), "coords must be"), (co[0], "dimensions"),
                       (co.transpose(2, 3).contiguous(), "coords must be"), (co.transpose(2, 3).contiguous().transpose(2, 3), "contiguous"),
                       (co.double(), "float32"), (co.half(), "float32"), (co.cpu(), "no CPU path")):
        with pytest.raises(E, match="corr_volume_lookup: .*" + words):
            blk(bad)
    assert torch.equal(blk(co), want)


def torch_pyramid(f1, f2, L):
    """CorrBlock's pyramid restated (the first lines of allpairs()): the volume by matmul over sqrt(C) in float32, chained avg_pool2d"""
    B, C, H, W = f1.shape
    vol = torch.matmul(f1.reshape(B, C, H * W).transpose(1, 2), f2.reshape(B, C, H * W)) / torch.sqrt(torch.tensor(C).float()).to(f1)
    pyr = [vol.reshape(B * H * W, 1, H, W)]
    for _ in range(L - 1):
        pyr.append(F.avg_pool2d(pyr[-1], 2, stride=2))
    return pyr


@pytest.mark.gpu
def test_gpu_pyramid_matches_torch_in_float64(golden, rc, dev):
    """every level (17 x 29 and 23 x 37 are among the cases: floor pooling drops the last row / column), bar: 3 x the distance of the float32
    torch pyramid from the float64 one"""
    for c in golden.values():
        f1, f2 = case_tensors(c, dev)[:2]
        pyr = rc.CorrBlock(f1, f2, num_levels=c["L"], radius=c["r"]).corr_pyramid
        p32, p64 = torch_pyramid(f1, f2, c["L"]), torch_pyramid(f1.double(), f2.double(), c["L"])
        assert len(pyr) == c["L"]
        for i, (h, w32, w64) in enumerate(zip(pyr, p32, p64)):
            assert h.shape == w64.shape == (c["H"] * c["W"], 1, c["H"] >> i, c["W"] >> i) and h.dtype == torch.float32
            e32, d = float((w32.double() - w64).abs().max()), float((h.double() - w64).abs().max())
            print("pyramid %-24s level %d %3d x %3d  |hip - torch64| %.2e = %.2f x |torch32 - torch64| (%.2e)" % (c["name"], i, h.shape[2], h.shape[3], d, d / e32, e32))
            assert d <= 3 * e32, (c["name"], i, d, e32)


@pytest.mark.gpu
def test_gpu_forward_and_backward_match_the_recorded_reference(golden, rc, dev):
    """output, grad_fmap1, grad_fmap2 within 3 * err32 of the double run, both ways of comparing; what the reference reports as exactly 0
    (windows wholly outside, exact integers and half pixels, +-1e9 in the adversarial case) is exactly 0"""
    for c in golden.values():
        want = with_grads(formula, t64(c["f1"]), t64(c["f2"]), t64(c["coords"]), t64(c["g"]), c["L"], c["r"])
        got = hip_with_grads(rc, *case_tensors(c, dev), c["L"], c["r"])
        assert got[0].shape == c["g"].shape and got[0].dtype == torch.float32 and got[0].is_contiguous()
        for key, h, w in zip(("out", "grad_fmap1", "grad_fmap2"), got, want):
            check_case(c, key, h, w, "all-pairs")
        assert c["zero"].any() and (got[0].cpu().numpy()[c["zero"]] == 0).all()


def base_grid(B, H, W):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return torch.stack([xs, ys])[None].repeat(B, 1, 1, 1)


def training_step(make, f1, f2, coords, cots, hids):
    """One RAFT-shaped step on ONE block: len(cots) lookups; a hidden state h carries every output into all later loss terms (RAFT's GRU
    state), the coordinates of lookup k + 1 come from h after lookup k, detached (RAFT/core/raft.py:123), and every lookup has its own seeded
    cotangent.  coords: the list to look up at, or a one-element list to start from (then the list is grown as RAFT would and returned)."""
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    fn = make(a, b)
    coords = list(coords)
    grow = len(coords) == 1
    h, loss, outs = torch.zeros_like(coords[0]), 0.0, []
    for k, (g, q) in enumerate(zip(cots, hids)):
        out = fn(coords[k])
        outs.append(out.detach())
        B, CH, H, W = out.shape
        h = 0.5 * h + out.reshape(B, 2, CH // 2, H, W).mean(2)
        loss = loss + (out * g).sum() + (h * q).sum()
        if grow and k + 1 < len(cots):
            coords.append((coords[k] + torch.tanh(h)).detach().contiguous())
    loss.backward()
    return outs, a.grad, b.grad, coords


def training_inputs(B, C, H, W, L, r, n, seed, dev, dtype=torch.float32):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    f1, f2 = [torch.randn(B, C, H, W, generator=gen).to(dev) for _ in range(2)]
    start = (base_grid(B, H, W) + 4.0 * torch.randn(B, 2, H, W, generator=gen)).to(dev)
    cots = [torch.randn(B, L * (2 * r + 1) ** 2, H, W, generator=gen).to(dev) for _ in range(n)]
    hids = [torch.randn(B, 2, H, W, generator=gen).to(dev) for _ in range(n)]
    return f1, f2, start, cots, hids


@pytest.mark.gpu
def test_gpu_training_shaped_step_of_twelve_lookups_on_one_block(rc, dev):
    """B = 2, C = 256, 36 x 120, L = 4, r = 4, twelve dependent lookups: every output and both gradients within 3 x |allpairs32 - allpairs64|,
    both measured here, at the coordinates the block's own run produced.  The test of the shared gradient pyramid."""
    B, C, H, W, L, r, n = 2, 256, 36, 120, 4, 4, 12
    f1, f2, start, cots, hids = training_inputs(B, C, H, W, L, r, n, 1234, dev)
    outs, g1, g2, coords = training_step(lambda a, b: rc.CorrBlock(a, b, num_levels=L, radius=r), f1, f2, [start], cots, hids)
    assert len(coords) == n and float((coords[-1] - coords[0]).abs().max()) > 0.5
    ref = lambda a, b: (lambda co: allpairs(a, b, co.to(a.dtype), L, r))
    o32, a32, b32, _ = training_step(ref, f1, f2, coords, cots, hids)
    o64, a64, b64, _ = training_step(ref, f1.double(), f2.double(), [c.double() for c in coords], [g.double() for g in cots], [q.double() for q in hids])
    rows = [("out[%d]" % k, outs[k], o32[k], o64[k]) for k in range(n)] + [("grad_fmap1", g1, a32, a64), ("grad_fmap2", g2, b32, b64)]
    worst = 0.0
    for key, h, w32, w64 in rows:
        e32, d = float((w32.double() - w64).abs().max()), float((h.double() - w64).abs().max())
        worst = max(worst, d / e32)
        print("training step %-10s |hip - allpairs64| %.2e = %.2f x |allpairs32 - allpairs64| (%.2e)" % (key, d, d / e32, e32))
        assert d <= 3 * e32, (key, d, e32)
    print("training step: worst ratio %.2f (bound 3)" % worst)


def folded_gradient(rc, f1, f2, coords, cots, L, r):
    """the gradient of the raw product for the loss sum_k <lookup(coords[k]), cots[k]>, through ops alone: what the HIP kernels produce"""
    from mpiflow_amd import ops
    blk = rc.CorrBlock(f1, f2, num_levels=L, radius=r)
    grad = [torch.zeros_like(t.squeeze(1)) for t in blk.corr_pyramid]
    for co, g in zip(coords, cots):
        ops.corr_volume_lookup_backward(grad, co, g, r)
    return ops.corr_pyramid_backward(grad, root_of(f1.shape[1]))


@pytest.mark.gpu
def test_gpu_the_same_step_twice_is_reproducible(rc, dev):
    """all twelve outputs and the folded gradient of the raw product are bit-identical (no atomics anywhere); grad_fmap1 / grad_fmap2 come out
    of torch.matmul: asserted within err32 = |allpairs32 - allpairs64| (measured here) of each other, and the observed difference is printed."""
    B, C, H, W, L, r, n = 2, 256, 36, 120, 4, 4, 12
    f1, f2, start, cots, hids = training_inputs(B, C, H, W, L, r, n, 99, dev)
    make = lambda a, b: rc.CorrBlock(a, b, num_levels=L, radius=r)
    o1, a1, b1, c1 = training_step(make, f1, f2, [start], cots, hids)
    o2, a2, b2, c2 = training_step(make, f1, f2, [start], cots, hids)
    assert all(torch.equal(x, y) for x, y in zip(o1, o2)) and all(torch.equal(x, y) for x, y in zip(c1, c2))
    fa, fb = folded_gradient(rc, f1, f2, c1, cots, L, r), folded_gradient(rc, f1, f2, c1, cots, L, r)
    assert torch.equal(fa, fb) and float(fa.abs().max()) > 0
    ref = lambda a, b: (lambda co: allpairs(a, b, co.to(a.dtype), L, r))
    _, a32, b32, _ = training_step(ref, f1, f2, c1, cots, hids)
    _, a64, b64, _ = training_step(ref, f1.double(), f2.double(), [c.double() for c in c1], [g.double() for g in cots], [q.double() for q in hids])
    for key, x, y, w32, w64 in (("grad_fmap1", a1, a2, a32, a64), ("grad_fmap2", b1, b2, b32, b64)):
        d, e32 = float((x - y).abs().max()), float((w32.double() - w64).abs().max())
        print("two runs: %s differ by %.2e (err32 %.2e); outputs and folded gradient identical" % (key, d, e32))
        assert d <= e32


@pytest.mark.gpu
def test_gpu_second_block_sees_nothing_of_the_first(golden, rc, dev):
    """a block built and trained after another gives what it gives alone: the gradient pyramid is the block's own and is released"""
    ca, cb = golden["c128_16x24"], golden["c64_17x29_r3_l2"]
    alone = hip_with_grads(rc, *case_tensors(cb, dev), cb["L"], cb["r"])
    hip_with_grads(rc, *case_tensors(ca, dev), ca["L"], ca["r"])
    after = hip_with_grads(rc, *case_tensors(cb, dev), cb["L"], cb["r"])
    assert torch.equal(alone[0], after[0])
    for key, x, y in zip(("grad_fmap1", "grad_fmap2"), alone[1:], after[1:]):
        assert float((x - y).abs().max()) <= cb[key]["err32"]
    # the same block trained twice (two graphs over one pyramid need retain_graph): the second pass starts from a fresh, zeroed buffer
    f1, f2, co, g = case_tensors(cb, dev)
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    blk = rc.CorrBlock(a, b, num_levels=cb["L"], radius=cb["r"])
    blk(co).backward(g, retain_graph=True)
    assert blk._shared.levels is None
    a.grad = b.grad = None
    blk(co).backward(g)
    assert blk._shared.levels is None
    assert float((a.grad - alone[1]).abs().max()) <= cb["grad_fmap1"]["err32"] and float((b.grad - alone[2]).abs().max()) <= cb["grad_fmap2"]["err32"]


@pytest.mark.gpu
def test_gpu_side_stream_and_two_live_blocks(golden, rc, dev):
    """two live blocks with interleaved lookups on a non-default stream while another stream is busy: each gives what it gives alone on the
    default stream (each owns its pyramid and its gradient pyramid; the kernels keep no scratch between calls)"""
    ca, cb = golden["c128_16x24"], golden["c64_17x29_r3_l2"]
    alone = {c["name"]: hip_with_grads(rc, *case_tensors(c, dev), c["L"], c["r"]) for c in (ca, cb)}
    torch.cuda.synchronize()
    busy, side = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    big = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(busy):
        for _ in range(20):
            big = big @ big * 1e-3
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ta, tb = case_tensors(ca, dev), case_tensors(cb, dev)
        A = rc.CorrBlock(ta[0].requires_grad_(True), ta[1].requires_grad_(True), num_levels=ca["L"], radius=ca["r"])
        Bk = rc.CorrBlock(tb[0].requires_grad_(True), tb[1].requires_grad_(True), num_levels=cb["L"], radius=cb["r"])
        oa1, ob, oa2 = A(ta[2]), Bk(tb[2]), A(ta[2])               # interleaved lookups of the two live blocks
        (oa1 + oa2).backward(ta[3] * 0.5)
        ob.backward(tb[3])
    side.synchronize()
    busy.synchronize()
    assert torch.equal(oa1.detach(), alone[ca["name"]][0]) and torch.equal(oa2.detach(), oa1.detach()) and torch.equal(ob.detach(), alone[cb["name"]][0])
    for t, c in ((ta, ca), (tb, cb)):
        assert float((t[0].grad - alone[c["name"]][1]).abs().max()) <= c["grad_fmap1"]["err32"]
        assert float((t[1].grad - alone[c["name"]][2]).abs().max()) <= c["grad_fmap2"]["err32"]


@pytest.mark.gpu
def test_gpu_only_some_lookups_reach_the_loss(golden, rc, dev):
    """three lookups, the loss uses the first and the third: the gradients are those of a block on which the second was never made"""
    c = golden["c128_16x24"]
    f1, f2, co, g = case_tensors(c, dev)
    res = []
    for unused in (True, False):
        a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        blk = rc.CorrBlock(a, b, num_levels=c["L"], radius=c["r"])
        o1 = blk(co)
        o2 = blk(co + 1.25) if unused else None
        o3 = blk(co - 0.5)
        ((o1 * g).sum() + 2.0 * (o3 * g).sum()).backward()
        assert blk._shared.levels is None
        res.append((o1.detach(), o3.detach(), a.grad, b.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float((res[0][2] - res[1][2]).abs().max()) <= c["grad_fmap1"]["err32"] and float((res[0][3] - res[1][3]).abs().max()) <= c["grad_fmap2"]["err32"]
    assert float(res[0][2].abs().max()) > 0.1
    # no lookup reaches the loss: the maps get no gradient from the block, and nothing is left behind
    a = f1.clone().requires_grad_(True)
    blk = rc.CorrBlock(a, f2, num_levels=c["L"], radius=c["r"])
    (blk(co).detach().sum() + (a * a).sum()).backward()
    assert blk._shared.levels is None and torch.equal(a.grad, 2 * f1)


@pytest.mark.gpu
def test_gpu_block_under_no_grad(golden, rc, dev):
    c = golden["c128_16x24"]
    f1, f2, co, g = case_tensors(c, dev)
    want = hip_with_grads(rc, f1, f2, co, g, c["L"], c["r"])[0]
    with torch.no_grad():
        blk = rc.CorrBlock(f1.clone().requires_grad_(True), f2.clone().requires_grad_(True), num_levels=c["L"], radius=c["r"])
        out = blk(co)
    assert torch.equal(out, want) and not out.requires_grad and not blk.corr_pyramid[0].requires_grad and blk._shared.levels is None
    out = rc.CorrBlock(f1, f2, num_levels=c["L"], radius=c["r"])(co)          # neither map requires a gradient
    assert torch.equal(out, want) and not out.requires_grad


@pytest.mark.gpu
def test_gpu_non_finite_and_huge_coordinates(rc, dev):
    """NaN, +-inf, +-1e30 in 10 % of the pixels: outputs and gradient contributions of those pixels are 0; everything the HIP kernels produce
    (outputs, the folded gradient of the raw product) equals, bit for bit, the run in which those pixels' coordinates are a far-outside finite
    value: nothing here is atomic."""
    B, C, H, W, L, r = 2, 64, 32, 48, 4, 4
    gen = torch.Generator(device="cpu").manual_seed(5)
    f1, f2 = [torch.randn(B, C, H, W, generator=gen) for _ in range(2)]
    base = base_grid(B, H, W) + 3.0 * torch.randn(B, 2, H, W, generator=gen)
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
    fw = folded_gradient(rc, to(f1), to(f2), [to(wild)], [to(g)], L, r)
    ft = folded_gradient(rc, to(f1), to(f2), [to(tame)], [to(g)], L, r)
    torch.cuda.synchronize()
    badd = to(bad)
    assert torch.equal(ow, ot) and torch.equal(fw, ft)
    assert (ow.permute(0, 2, 3, 1)[badd] == 0).all() and (fw.reshape(B, H, W, H * W)[badd] == 0).all() and (w1.permute(0, 2, 3, 1)[badd] == 0).all()
    assert torch.isfinite(ow).all() and torch.isfinite(fw).all() and torch.isfinite(w1).all() and torch.isfinite(w2).all()
    for x, y in ((w1, t1), (w2, t2)):                                    # torch.matmul of identical operands
        assert float((x - y).abs().max()) <= 2.0 ** -20 * float(y.abs().max())
    assert float(ot.abs().max()) > 0.5 and float(t2.abs().max()) > 0.5 and float(ft.abs().max()) > 0


def peak_of(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    keep = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - before, keep


@pytest.mark.gpu
def test_gpu_peak_memory(rc, dev):
    """B = 1, C = 256, 48 x 160, L = 4, r = 4.  P = the pyramid's bytes.  Under no_grad, construction plus a lookup: at most P (the raw product
    is level 0 itself) + the linear terms; with backward and the block alive through it: at most 2 P (the pyramid and ONE gradient pyramid) +
    the linear terms, which is less than 2.3 P here, so a third pyramid-sized allocation fails the test.  Linear terms:
    the output and, with backward, its cotangent and product with it (3 outputs), the two gradients, one map-sized operand copy per GEMM (3
    maps).  Beyond its result torch.matmul may allocate a workspace: measured first, on the same device, for the same three GEMMs, and allowed."""
    B, C, H, W, L, r = 1, 256, 48, 160, 4, 4
    HW = H * W
    f1, f2 = torch.randn(B, C, H, W, device=dev), torch.randn(B, C, H, W, device=dev)
    coords = (base_grid(B, H, W).to(dev) + 4.0 * torch.randn(B, 2, H, W, device=dev)).contiguous()
    G = torch.randn(B, HW, HW, device=dev)
    gemms = (lambda: torch.matmul(f1.view(B, C, HW).transpose(1, 2), f2.view(B, C, HW)), lambda: torch.matmul(f2.view(B, C, HW), G.transpose(1, 2)),
             lambda: torch.matmul(f1.view(B, C, HW), G))
    extra = 0
    for gemm in gemms:
        used, res = peak_of(gemm, dev)
        extra = max(extra, used - res.numel() * 4)
        del res
    del G
    P = 4 * B * HW * sum((H >> i) * (W >> i) for i in range(L))
    out_bytes, map_bytes = 4 * B * L * 81 * HW, 4 * B * C * HW

    def no_grad():
        with torch.no_grad():
            return rc.CorrBlock(f1, f2, num_levels=L, radius=r)(coords)

    def train(make, keep=False):
        a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        fn = make(a, b)
        out = fn(coords)
        if not keep:                                         # as RAFT.forward does on return; a lookup's backward needs no pyramid values
            del fn
        (out * out).sum().backward()
        return a.grad, b.grad

    used_ng, _ = peak_of(no_grad, dev)
    used_bw, _ = peak_of(lambda: train(lambda a, b: rc.CorrBlock(a, b, num_levels=L, radius=r), keep=True), dev)
    used_dropped, _ = peak_of(lambda: train(lambda a, b: rc.CorrBlock(a, b, num_levels=L, radius=r)), dev)
    used_torch, _ = peak_of(lambda: train(lambda a, b: (lambda co: allpairs(a, b, co, L, r))), dev)
    budget_ng = P + out_bytes + map_bytes + extra
    budget_bw = 2 * P + 3 * out_bytes + (2 + 2 + 3) * map_bytes + extra          # + the two clones train() makes
    print("peak memory: P %.1f MB, matmul workspace %.1f MB; no_grad %.1f MB (budget %.1f); forward + backward %.1f MB (budget %.1f); "
          "the same with the block dropped before backward %.1f MB; torch all-pairs forward + backward %.1f MB"
          % (P / 1e6, extra / 1e6, used_ng / 1e6, budget_ng / 1e6, used_bw / 1e6, budget_bw / 1e6, used_dropped / 1e6, used_torch / 1e6))
    assert used_ng <= budget_ng, (used_ng, budget_ng)
    assert 2 * P <= used_bw <= budget_bw, (used_bw, budget_bw)          # the block alive through backward: the pyramid and ONE gradient pyramid, no third
    assert used_dropped <= used_bw
