"""The single-view form of the fused renderer - PairRenderer(n_views=1), prepare(K, disparity, [G]) with P == 1, run(..., complement=(c,)) -
against the CPU oracle, bit for bit.

It is the reference's camera-only configuration (utils/utils.py:291-349) and what bench.py's `c2` record times.  The kernels underneath have
tests of their own; what is checked here is their assembly with ONE pose: the P == 1 parameter block (record = s * P + p), the one-sided
mask-quad selection, the per-view Stage B launch, the one-view buffers and the flow-only re-run after blend().

The reference of every GPU test is put together from the oracle's existing pieces (`_reference`: oracle.render_pair with one pose) in its
kernel-exp mode, where it runs the kernels' IEEE operation sequence: every comparison is `bits_equal(...) == 0`, there is no tolerance.
Only the parameter-block test at the end runs without a device.
"""
import contextlib
import functools
import importlib.util
import os
import random

import numpy as np
import pytest
import torch

from conftest import ROOT, bits_equal

SENTINEL = 0x7FC5A5A5                    # a quiet NaN with a payload no kernel produces: "this float was never written"
SENTINEL_U8 = 0xAB
SCALES = (0.15, 0.4, 0.9)                # the reference sampler's ext_cz and up to 6 x beyond it (planes behind the camera, samples off the frame)


def _random_shapes():
    rng = random.Random(7001)
    return [(rng.randint(1, 40), rng.randint(1, 60), rng.randint(1, 90)) for _ in range(12)]


RANDOM_SHAPES = _random_shapes()
# one pixel / one plane, the tallest stack on one pixel, one row, one column, one wave's width and one either side of it, an odd multi-row frame
EDGE_SHAPES = [(1, 1, 1), (40, 1, 1), (3, 1, 90), (3, 60, 1), (2, 5, 63), (2, 5, 64), (2, 5, 65), (7, 17, 33)]
SHAPES = RANDOM_SHAPES + EDGE_SHAPES
MASKS = ("ones", "soft", "zeros")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mpiflow_amd import _lib
    _lib.load()      # fails loudly if the HIP library was not built
    return torch.device("cuda:0")


@contextlib.contextmanager
def _kernel_exp(oracle):
    oracle.set_exp_mode(1)
    try:
        yield oracle
    finally:
        oracle.set_exp_mode(0)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def _stack(rs, S, H, W):
    """A random stack with the soak's sigma, a random image and the soak's soft mask."""
    mpi = rs.rand(S, 4, H, W).astype(np.float32)
    mpi[:, 3] = np.maximum(3.0 * rs.randn(S, H, W) - 3.0, 0.0).astype(np.float32) + np.float32(1e-4)
    img = rs.rand(3, H, W).astype(np.float32)
    soft = (rs.rand(H, W) * (rs.rand(H, W) > 0.4)).astype(np.float32)
    return mpi, img, soft


@functools.lru_cache(maxsize=None)
def _problem(S, H, W, seed, scale):
    """Inputs as in test_soak.py::test_pair_vs_oracle_soak; built once per shape and shared, never modified."""
    from mpiflow_amd import synth
    from oracle import mpi_oracle
    mpi, img, soft = _stack(np.random.RandomState(seed), S, H, W)
    rng = random.Random(seed * 31 + 5)
    G_dyn, G_cam = mpi_oracle.random_pose(rng, scale), mpi_oracle.random_pose(rng, scale, base_motions=(0, 0, 0))
    masks = dict(ones=np.ones((H, W), np.float32), soft=soft, zeros=np.zeros((H, W), np.float32))
    return dict(S=S, H=H, W=W, mpi=mpi, img=img, masks=masks, K=synth.intrinsics(H, W), pd=synth.plane_disparities(S), scale=scale,
                poses=dict(cam=G_cam, dyn=G_dyn), stage_a={})


def _shape_problem(idx):
    S, H, W = SHAPES[idx]
    return _problem(S, H, W, 100 + idx, SCALES[idx % 3])


def _reference(oracle, p, which, om, comp):
    """oracle.render_pair with one pose (call with the oracle in kernel-exp mode).  Stage A+C depends on the pose only: kept per problem."""
    G = p["poses"][which]
    d, k_inv = oracle.plane_depths(p["pd"]), oracle.k_inverse(p["K"])
    Hts, Hst = oracle.homographies(G, k_inv, p["K"], d)
    if which not in p["stage_a"]:
        p["stage_a"][which] = oracle.src_blend_flow(p["mpi"], p["img"], k_inv, d, Hts[None])
    a = p["stage_a"][which]
    m = (1.0 - torch.from_numpy(om)).numpy() if comp else om
    v = oracle.warp_composite(a["rgba"], m, Hst, k_inv, G, d)
    return dict(flow=a["flows"][0], rgba=a["rgba"], rgb=v["rgb"], objmask=v["objmask"], src_u8=oracle.to_u8_bgr(p["img"]))


def _fill(t):
    if t.dtype == torch.uint8:
        t.fill_(SENTINEL_U8)
    else:
        t.view(torch.int32).fill_(SENTINEL)


def _untouched(t):
    a = N(t)
    return bool((a == SENTINEL_U8).all()) if a.dtype == np.uint8 else bool((a.view(np.uint32) == SENTINEL).all())


def _poison(r, stack=True):
    """Everything run() is to write gets the sentinel, so that nothing left over from an earlier run can pass for an output."""
    for t in [r.flows, r.quads[0], r.quads[1]] + [v[k] for v in r.views for k in ("rgb", "objmask", "rgb_u8")] + ([r.src_u8] if stack else []):
        _fill(t)


def _run_single(r, dev_in, p, which, comp, **kw):
    mpi, img, om = dev_in
    prep = r.prepare(p["K"], p["pd"], [p["poses"][which]])
    assert prep["P"] == 1 and len(prep["warp"]) == 1
    flows, views = r.run(mpi, img, prep, om, complement=(comp,), **kw)
    torch.cuda.synchronize()
    return flows, views


def _assert_view(oracle, r, flows, views, want, om_dev, comp, tag, stack=True):
    from mpiflow_amd import ops
    H, W = want["objmask"].shape
    assert flows is r.flows and tuple(flows.shape) == (1, 2, H, W) and len(views) == 1, tag
    assert bits_equal(N(flows[0]), want["flow"]) == 0, (tag, "flow")
    assert bits_equal(N(views[0]["rgb"]), want["rgb"]) == 0, (tag, "rgb")
    assert bits_equal(N(views[0]["objmask"]), want["objmask"]) == 0, (tag, "objmask")
    if stack:
        assert bits_equal(N(r.src_u8), want["src_u8"]) == 0, (tag, "src_u8")
        assert bits_equal(N(r.rgba), want["rgba"]) == 0, (tag, "rgba")
    # the mask quads: the side the view samples is written, the other one is not touched
    assert bits_equal(N(r.quads[1 if comp else 0]), N(ops.mask_quads(om_dev, complement=comp))) == 0, (tag, "quads")
    assert _untouched(r.quads[0 if comp else 1]), (tag, "the mask quads that were not requested")
    # the frame as u8 BGR: pinned by test_hip_parity.py::test_fused_byproducts_equal_standalone_kernels to the stand-alone kernel on the view's
    # own rgb, which test_merge_and_u8_bit_exact pins to the oracle's
    assert torch.equal(views[0]["rgb_u8"], ops.to_u8_bgr(views[0]["rgb"])), (tag, "rgb_u8")
    assert bits_equal(N(views[0]["rgb_u8"]), oracle.to_u8_bgr(want["rgb"])) == 0, (tag, "rgb_u8 vs oracle")


# ---- 1. PairRenderer(n_views=1) equals the single-view reference ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=["%dx%dx%d" % s for s in SHAPES])
def test_single_view_renderer_equals_the_oracle(dev, oracle, idx):
    """Twelve seeded random shapes (S 1..40, H 1..60, W 1..90) and eight edge shapes; per shape both pose kinds of the reference sampler
    (at scale 0.15 / 0.4 / 0.9 by shape) x complement False / True x the all-ones (camera-only), soft random and all-zeros masks on ONE renderer
    whose outputs are poisoned before every run: flow, frame, rendered mask, blended stack, source frame and the frame as u8 bit for bit, the
    requested mask quads equal to the stand-alone kernel's and the other buffer untouched."""
    from mpiflow_amd import pipeline
    p = _shape_problem(idx)
    S, H, W = p["S"], p["H"], p["W"]
    with _kernel_exp(oracle):
        r = pipeline.PairRenderer(S, H, W, dev, n_views=1)
        assert tuple(r.flows.shape) == (1, 2, H, W) and len(r.views) == 1
        mpi, img = T(p["mpi"], dev), T(p["img"], dev)
        for name in MASKS:
            om = T(p["masks"][name], dev)
            for which in ("cam", "dyn"):
                for comp in (False, True):
                    want = _reference(oracle, p, which, p["masks"][name], comp)
                    _poison(r)
                    flows, views = _run_single(r, (mpi, img, om), p, which, comp)
                    _assert_view(oracle, r, flows, views, want, om, comp, (S, H, W, p["scale"], name, which, comp))


# ---- 2. one view is the pair's view -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(0, 12, 2), ids=["%dx%dx%d" % SHAPES[i] for i in range(0, 12, 2)])
def test_single_view_is_the_pairs_view(dev, idx):
    """The pair on the default two-view renderer (both views in one Stage B launch), then each of its poses alone on an n_views=1 renderer:
    G_cam with obj_mask, G_dyn with 1 - obj_mask.  Same bytes; and multi_view = False on the single-view renderer changes none."""
    from mpiflow_amd import pipeline
    p = _shape_problem(idx)
    S, H, W = p["S"], p["H"], p["W"]
    mpi, img, om = T(p["mpi"], dev), T(p["img"], dev), T(p["masks"]["soft"], dev)
    out = pipeline.render_pair(img, om, mpi, p["pd"], p["K"], p["poses"]["cam"], p["poses"]["dyn"])
    torch.cuda.synchronize()
    pair = {("cam", False): (N(out["flows"][0]), out["view_cam"]), ("dyn", True): (N(out["flows"][1]), out["view_dyn"])}
    pair = {k: (f, N(v["rgb"]), N(v["objmask"])) for k, (f, v) in pair.items()}
    stack, src = N(out["rgba"]), N(out["src_np"])
    r = pipeline.PairRenderer(S, H, W, dev, n_views=1)
    for multi_view in (True, False):
        r.multi_view = multi_view
        for (which, comp), (flow, rgb, objmask) in pair.items():
            _poison(r)
            flows, views = _run_single(r, (mpi, img, om), p, which, comp)
            tag = (S, H, W, which, multi_view)
            assert tuple(flows.shape) == (1, 2, H, W), tag
            assert bits_equal(N(flows[0]), flow) == 0, (tag, "flow")
            assert bits_equal(N(views[0]["rgb"]), rgb) == 0, (tag, "rgb")
            assert bits_equal(N(views[0]["objmask"]), objmask) == 0, (tag, "objmask")
            assert bits_equal(N(r.rgba), stack) == 0 and bits_equal(N(r.src_u8), src) == 0, (tag, "stack")
            assert _untouched(r.quads[0 if comp else 1]), (tag, "the mask quads that were not requested")


# ---- 3. blend() + reuse_blend=True with one pose --------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_blend_once_then_flow_only_single_views(dev, oracle):
    """The single-view twin of test_hip_parity.py::test_blend_once_then_flow_only_pairs: blend() once, then one reuse_blend run per pose
    (flow-only Stage A+C with P == 1) gives the bytes of a fresh renderer's plain run() and of the oracle, and leaves the blended stack and
    the source frame byte-unchanged."""
    from mpiflow_amd import pipeline
    S, H, W = 5, 33, 65
    p = _problem(S, H, W, 301, 0.4)
    rng = random.Random(12)
    poses = [oracle.random_pose(rng, 0.15), oracle.random_pose(rng, 0.4, base_motions=(0, 0, 0)), oracle.random_pose(rng, 0.9)]
    mpi, img, om = T(p["mpi"], dev), T(p["img"], dev), T(p["masks"]["soft"], dev)
    with _kernel_exp(oracle):
        r = pipeline.PairRenderer(S, H, W, dev, n_views=1)
        _fill(r.src_u8)
        r.blend(mpi, img, p["K"], p["pd"])
        torch.cuda.synchronize()
        stack0, src0 = N(r.rgba).copy(), N(r.src_u8).copy()
        for i, (G, comp) in enumerate(zip(poses, (False, True, False))):
            q = dict(p, poses={"pose%d" % i: G})
            want = _reference(oracle, q, "pose%d" % i, p["masks"]["soft"], comp)
            assert bits_equal(stack0, want["rgba"]) == 0 and bits_equal(src0, want["src_u8"]) == 0
            fresh = pipeline.PairRenderer(S, H, W, dev, n_views=1)
            _poison(fresh)
            f_flows, f_views = _run_single(fresh, (mpi, img, om), q, "pose%d" % i, comp)
            _poison(r, stack=False)
            flows, views = _run_single(r, (mpi, img, om), q, "pose%d" % i, comp, reuse_blend=True)
            _assert_view(oracle, r, flows, views, want, om, comp, ("reuse", i, comp), stack=False)
            assert bits_equal(N(flows), N(f_flows)) == 0, i
            for k in ("rgb", "objmask", "rgb_u8"):
                assert bits_equal(N(views[0][k]), N(f_views[0][k])) == 0, (i, k)
            assert bits_equal(N(r.quads[1 if comp else 0]), N(fresh.quads[1 if comp else 0])) == 0, i
            assert bits_equal(N(r.rgba), stack0) == 0 and bits_equal(N(r.src_u8), src0) == 0, (i, "blend() results changed by a reuse run")


# ---- 4. the fused activation epilogue with one pose -----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("S,H,W", [(8, 24, 64), (5, 33, 65)])
def test_activation_epilogue_with_one_pose(dev, oracle, S, H, W):
    """The raw decoder output + cum_mask through run() with P == 1 against the stack activated with torch, the identity and the bars of
    test_model.py::test_forward_on_gpu_and_fused_epilogue: sigma identical (mul, max, add), rgb within 1e-6 (sigmoid to a few ulp), flow within
    1e-4.  Beyond those bars, what follows the epilogue is bit for bit the oracle's on the stack the epilogue wrote: the flow from its sigma,
    the view from its texels."""
    from mpiflow_amd import pipeline
    p = _problem(S, H, W, 401, 0.15)
    g = torch.Generator().manual_seed(S * 100 + W)
    raw = torch.randn((S, 4, H, W), generator=g).to(dev)
    cum = torch.rand((S, H, W), generator=g).to(dev)
    act = torch.cat((torch.sigmoid(raw[:, :3]), torch.relu(raw[:, 3:] * cum.unsqueeze(1)) + 1e-4), dim=1).contiguous()
    img, om = T(p["img"], dev), T(p["masks"]["soft"], dev)
    with _kernel_exp(oracle):
        ra, rb = pipeline.PairRenderer(S, H, W, dev, n_views=1), pipeline.PairRenderer(S, H, W, dev, n_views=1)
        for which, comp in (("cam", False), ("dyn", True)):
            _poison(ra)
            _poison(rb)
            fa, va = _run_single(ra, (act, img, om), p, which, comp)
            fb, vb = _run_single(rb, (raw, img, om), p, which, comp, cum_mask=cum)
            assert tuple(fb.shape) == (1, 2, H, W)
            assert torch.equal(ra.rgba[..., 3], rb.rgba[..., 3])
            assert float((ra.rgba - rb.rgba).abs().max()) < 1e-6
            assert float((fa - fb).abs().max()) < 1e-4
            assert torch.equal(ra.src_u8, rb.src_u8) and torch.equal(ra.quads[1 if comp else 0], rb.quads[1 if comp else 0])
            assert _untouched(rb.quads[0 if comp else 1])
            # downstream of the epilogue: the oracle on the texels the fused run left in rb.rgba
            G = p["poses"][which]
            d, k_inv = oracle.plane_depths(p["pd"]), oracle.k_inverse(p["K"])
            Hts, Hst = oracle.homographies(G, k_inv, p["K"], d)
            texels = N(rb.rgba)
            planar = np.ascontiguousarray(texels.transpose(0, 3, 1, 2))         # the flow reads channel 3 (sigma) only
            assert bits_equal(N(fb[0]), oracle.src_blend_flow(planar, p["img"], k_inv, d, Hts[None], want_rgba=False)["flows"][0]) == 0
            m = (1.0 - torch.from_numpy(p["masks"]["soft"])).numpy() if comp else p["masks"]["soft"]
            v = oracle.warp_composite(texels, m, Hst, k_inv, G, d)
            assert bits_equal(N(vb[0]["rgb"]), v["rgb"]) == 0 and bits_equal(N(vb[0]["objmask"]), v["objmask"]) == 0


# ---- 5. what the benchmark's camera-only record times ---------------------------------------------------------------------------------

_BENCH = []


def _bench(monkeypatch):
    """bench.py as a module, loaded as tests/test_host_logic.py::test_bench_output_dump_is_bounded_and_seeded does."""
    if not _BENCH:
        monkeypatch.delenv("HSA_ENABLE_IPC_MODE_LEGACY", raising=False)        # bench.py sets a default at import: restored after the test
        spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _BENCH.append(mod)
    return _BENCH[0]


@pytest.mark.gpu
@pytest.mark.parametrize("S,H,W", [(8, 24, 40), (5, 33, 65)])
def test_bench_camera_only_workload_renders_the_single_view(dev, oracle, monkeypatch, S, H, W):
    """bench.Workload(dynamic=False) - the `c2` sub-record: one pose per image (the G_dyn draw of its pose stream), all-ones mask, the quads of
    the mask itself.  What pair() leaves in the renderer is the single-view reference, with and without the event brackets between the launches."""
    from mpiflow_amd import host_math, synth
    bench = _bench(monkeypatch)
    w = bench.Workload(S, H, W, 2, dev, dynamic=False)
    assert w.r.n_views == 1 and tuple(w.r.flows.shape) == (1, 2, H, W) and len(w.r.views) == 1
    rng = random.Random(114514)
    poses = []
    for _ in range(2):
        G_dyn = host_math.generate_random_pose(0.15, rng=rng)
        host_math.generate_random_pose(0.15, base_motions=(0, 0, 0), rng=rng)          # G_cam: drawn, not rendered
        poses.append(G_dyn.numpy() if torch.is_tensor(G_dyn) else np.asarray(G_dyn))
    ones = N(w.om)
    assert ones.shape == (H, W) and (ones == 1).all()
    with _kernel_exp(oracle):
        for i in range(2):
            assert w.preps[i]["P"] == 1
            mpi, img = w.images[i]
            p = dict(mpi=N(mpi), img=N(img), K=synth.intrinsics(H, W), pd=synth.plane_disparities(S), poses=dict(view=poses[i]), stage_a={})
            want = _reference(oracle, p, "view", ones, False)
            for timed in (False, True):
                _poison(w.r)
                w.pair(i, timed=timed)
                torch.cuda.synchronize()
                _assert_view(oracle, w.r, w.r.flows, w.r.views, want, w.om, False, (S, H, W, i, timed))
        assert len(w.ev_ac) == 2 and len(w.ev_b) == 2


# ---- 6. the drop-in entry with the camera-only mask -----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("S,H,W", [(8, 24, 40), (3, 7, 65)])
def test_render_novel_view_dynamic_with_the_camera_only_mask(dev, oracle, S, H, W):
    """utils.utils.render_novel_view_dynamic (arguments as in test_dropin_api.py::test_render_novel_view_dynamic_signature) with an all-ones
    obj_mask: frame, depth and rendered mask equal the oracle's Stage B on the planar stack, the flow its Stage A+C flow."""
    from mpiflow_amd.utils import utils as U
    from mpiflow_amd.utils.mpi.homography_sampler import HomographySample
    p = _problem(S, H, W, 601, 0.15)
    hs = HomographySample(H, W, dev)
    ones = p["masks"]["ones"]
    with _kernel_exp(oracle):
        d, k_inv = oracle.plane_depths(p["pd"]), oracle.k_inverse(p["K"])
        blended = oracle.src_blend_flow(p["mpi"], p["img"], k_inv, d, None, want_rgba=False, want_planar=True)["rgb_planar"]
        planar = np.ascontiguousarray(np.concatenate([blended, p["mpi"][:, 3:]], axis=1))
        rgb_b = T(blended, dev)[None]
        sig = T(p["mpi"], dev)[None][:, :, 3:]            # a strided view, as in the reference (utils/utils.py:189)
        om = T(ones, dev)[None, None]
        for which in ("cam", "dyn"):
            G = p["poses"][which]
            Hts, Hst = oracle.homographies(G, k_inv, p["K"], d)
            want = oracle.warp_composite(planar, ones, Hst, k_inv, G, d, interleaved=False)
            want_flow = oracle.src_blend_flow(p["mpi"], p["img"], k_inv, d, Hts[None])["flows"][0]
            frame, depth, flow, mask = U.render_novel_view_dynamic(om, rgb_b, sig, T(p["pd"], dev)[None], T(G, dev), T(k_inv, dev)[None],
                                                                   T(p["K"], dev)[None], T(p["K"], dev)[None], None, hs)
            assert tuple(frame.shape) == (1, 3, H, W) and tuple(depth.shape) == (1, 1, H, W) and tuple(flow.shape) == (1, 2, H, W)
            assert tuple(mask.shape) == (1, 1, H, W)
            assert bits_equal(N(frame[0]), want["rgb"]) == 0, which
            assert bits_equal(N(depth[0, 0]), want["depth"]) == 0, which
            assert bits_equal(N(mask[0, 0]), want["objmask"]) == 0, which
            assert bits_equal(N(flow[0]), want_flow) == 0, which


# ---- 7. host side: the parameter block with one pose ----------------------------------------------------------------------------------

def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("S", [1, 5, 32])
def test_blend_flow_params_with_one_pose(S):
    """ops.blend_flow_params packs record = s * P + p behind a PARAMS_HEADER-float header (layout: pipeline.pack_pair_blocks).  The header
    carries K^-1 and no field for P (P is a kernel argument), so the one-pose block's header equals the two-pose block's outright, and its S
    records are the two-pose block's records of that pose - stride 1 instead of 2."""
    from mpiflow_amd import host_math, ops
    HDR, REC = host_math.PARAMS_HEADER, host_math.PLANE_RECORD
    g = torch.Generator().manual_seed(50 + S)
    k_inv = torch.randn((3, 3), generator=g)
    d = torch.rand((S,), generator=g) + 0.5
    H_ts = torch.randn((2, S, 3, 3), generator=g)
    two, P2 = ops.blend_flow_params(k_inv, d, H_ts)
    assert P2 == 2 and two.dtype == torch.float32 and two.numel() == HDR + REC * 2 * S
    rec2 = two[HDR:].view(S, 2, REC)
    for p, one_pose in ((0, H_ts[:1]), (1, H_ts[1:])):
        one, P1 = ops.blend_flow_params(k_inv, d, one_pose)
        assert P1 == 1 and one.dtype == torch.float32 and one.numel() == HDR + REC * S
        assert torch.equal(_bits(one[:HDR]), _bits(two[:HDR]))
        rec1 = one[HDR:].view(S, REC)
        assert torch.equal(_bits(rec1), _bits(rec2[:, p])), p
        # and the records are what the layout says: the pose's homography, the plane's depth, zero padding
        assert torch.equal(_bits(rec1[:, 0:9]), _bits(H_ts[p].reshape(S, 9))) and torch.equal(_bits(rec1[:, 9]), _bits(d))
        assert not rec1[:, 10:].any()
    assert torch.equal(_bits(two[0:9]), _bits(k_inv.reshape(9))) and not two[9:HDR].any()
