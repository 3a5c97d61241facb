"""Mask support maps (include/mpiflow_hip.h): Stage B does not render the tiles whose object-mask taps are all zero.

What must hold: the merged products of every pair of an OverlappedPairRenderer stream are bit-identical to the CPU oracle (kernel-exp mode),
whatever the mask looks like and whatever an earlier pair left in the slot's maps; a tile the device reports dead has an all-zero composited
mask in the oracle; on the benchmark's shape the skip reaches most of view 0; and the views that must not skip (thresh <= 0, depth wanted)
equal the full render on every pixel."""
import random

import numpy as np
import pytest
import torch

from conftest import bits_equal

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mpiflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _box(H, W, y0, y1, x0, x1, value=1.0):
    m = np.zeros((H, W), np.float32)
    m[y0:y1, x0:x1] = value
    return m


def stress_masks(H, W, seed):
    """Masks that stress the support map: name -> [H,W] float32."""
    from mpiflow_amd import synth
    g = np.random.Generator(np.random.PCG64(seed))
    speckle = np.where(g.random((H, W)) < 0.004, g.random((H, W)), 0.0).astype(np.float32)
    negzero = _box(H, W, H // 3, H // 3 + 5, W // 2, W // 2 + 9, 0.75)
    negzero[g.random((H, W)) < 0.3] *= np.float32(-1.0)            # -0.0 wherever the mask is zero, negative values inside the box
    negzero = np.where(negzero < 0, np.float32(-0.0), negzero).astype(np.float32)
    out = {"zero": np.zeros((H, W), np.float32), "one": np.ones((H, W), np.float32), "soft_box": synth.soft_box_mask(H, W), "speckle": speckle,
           "negzero": negzero, "all_negzero": np.full((H, W), -0.0, np.float32)}
    for name, (y, x) in {"px_nw": (0, 0), "px_ne": (0, W - 1), "px_sw": (H - 1, 0), "px_se": (H - 1, W - 1), "px_last_row": (H - 1, W // 2),
                         "px_last_col": (H // 2, W - 1)}.items():
        m = np.zeros((H, W), np.float32)
        m[y, x] = 1.0
        out[name] = m
    return out


def run_stream(dev, oracle, S, H, W, masks, scale, merge_in_launch, seed, thresh=0.99, kind="smooth"):
    """Pushes one pair per mask through an OverlappedPairRenderer - ONE caller-owned mask tensor, rewritten after every push() - and
    compares every handed-back pair (prologue and flush() pairs included) with the oracle, bit for bit."""
    from mpiflow_amd import pipeline, synth
    inp = [synth.make_inputs(S, H, W, seed=seed + k, kind=kind) for k in range(2)]
    K, disp = inp[0]["K"], inp[0]["disparity"]
    rng = random.Random(seed)
    r = pipeline.OverlappedPairRenderer(S, H, W, dev, thresh=thresh, merge_in_launch=merge_in_launch)
    assert r.skip_dead_tiles
    mpis, imgs = [T(x["mpi"], dev) for x in inp], [T(x["image"], dev) for x in inp]
    om_t = torch.empty((H, W), dtype=torch.float32, device=dev)
    poses, done = [], []
    for k, m in enumerate(masks):
        G_dyn = oracle.random_pose(rng, scale)
        G_cam = oracle.random_pose(rng, scale, base_motions=(0, 0, 0))
        poses.append((G_cam, G_dyn))
        om_t.copy_(T(m, dev))
        res = r.push(mpis[k % 2], imgs[k % 2], r.prepare(K, disp, [G_cam, G_dyn]), om_t)
        om_t.fill_(float("nan"))                                  # the mask is consumed by the push() it was given to
        if res is not None:
            done.append(res)
    done += r.flush()
    torch.cuda.synchronize()
    assert len(done) == len(masks)
    oracle.set_exp_mode(1)
    try:
        for k, (m, (G_cam, G_dyn)) in enumerate(zip(masks, poses)):
            o = oracle.render_pair(inp[k % 2]["image"], m, inp[k % 2]["mpi"], disp, K, G_cam, G_dyn, thresh=thresh)
            for j, key in enumerate(("flow_mix", "frame_mix", "fill_mask")):
                bad = bits_equal(N(done[k][j]), o[key])
                assert bad == 0, "pair %d: %s differs from the oracle on %d values" % (k, key, bad)
    finally:
        oracle.set_exp_mode(0)


# frames that are not multiples of the 32 x 8 tile / cell, S = 1 and S > 64, pose scales up to 0.9
SHAPES = [(5, 45, 70, 0.15), (1, 40, 64, 0.4), (70, 33, 50, 0.9), (8, 64, 96, 0.9), (6, 71, 130, 0.4)]


@pytest.mark.parametrize("merge_in_launch", [False, True])
@pytest.mark.parametrize("S,H,W,scale", SHAPES)
def test_stream_products_equal_the_oracle_for_masks_that_stress_the_map(dev, oracle, S, H, W, scale, merge_in_launch):
    masks = list(stress_masks(H, W, seed=S * 7 + H).values())
    run_stream(dev, oracle, S, H, W, masks, scale, merge_in_launch, seed=31 + S)


@pytest.mark.parametrize("merge_in_launch", [False, True])
def test_stale_cells_of_a_slot_neither_keep_a_tile_alive_nor_kill_one(dev, oracle, merge_in_launch):
    """Two slots alternate, so pairs k and k + 2 share one: L L E E L L E E sends every slot large -> empty -> large -> empty."""
    S, H, W = 6, 72, 128
    large = np.ones((H, W), np.float32)
    large[:, :5] = 0.0
    box = _box(H, W, 20, 40, 30, 70, 0.995)
    empty = np.zeros((H, W), np.float32)
    run_stream(dev, oracle, S, H, W, [large, box, empty, empty, box, large, empty, empty, large], 0.4, merge_in_launch, seed=77)


def _stage_ac(dev, inp, G_cam, G_dyn, mask, tag=5):
    """Stand-alone Stage A+C with the support maps; -> (renderer-like dict)"""
    from mpiflow_amd import ops, pipeline
    S, _, H, W = inp["mpi"].shape
    r = pipeline.PairRenderer(S, H, W, dev)
    prep = r.prepare(inp["K"], inp["disparity"], [G_cam, G_dyn])
    b = dict(rgba=ops.alloc_rgba_stack(S, H, W, dev), flows=torch.empty((2, 2, H, W), dtype=torch.float32, device=dev),
             quads=[torch.empty((H, W, 4), dtype=torch.float32, device=dev) for _ in range(2)],
             support=[torch.full(ops.support_cells(H, W), tag - 2, dtype=torch.int32, device=dev) for _ in range(2)], prep=prep, tag=tag)
    ops.src_blend_flow(T(inp["mpi"], dev), T(inp["image"], dev), out_rgba=b["rgba"], out_flows=b["flows"], dparams=prep["blend"], P=2, obj_mask=T(mask, dev),
                       quads=b["quads"][0], quads_complement=b["quads"][1], support=b["support"][0], support_complement=b["support"][1], tag=tag)
    return b


def _views(dev, b, H, W, support=True, thresh=0.99, depth=False):
    out = []
    for v in range(2):
        o = dict(rgb=torch.empty((3, H, W), dtype=torch.float32, device=dev), objmask=torch.empty((H, W), dtype=torch.float32, device=dev),
                 rgb_u8=torch.empty((H, W, 3), dtype=torch.uint8, device=dev))
        if depth:
            o["depth"] = torch.empty((H, W), dtype=torch.float32, device=dev)
        out.append(dict(dparams=b["prep"]["warp"][v], quads=b["quads"][v], out=o, support=(b["support"][v], b["tag"], thresh) if support else None))
    return out


def _tile_mask(dead_v, H, W):
    return np.repeat(np.repeat(dead_v.astype(bool), 8, axis=0), 32, axis=1)[:H, :W]


def test_a_tile_the_device_reports_dead_has_an_all_zero_mask_in_the_oracle(dev, oracle):
    from mpiflow_amd import ops, synth
    g = np.random.Generator(np.random.PCG64(2024))
    rng = random.Random(9)
    flagged = tiles = 0
    for case in range(40):
        S = int(g.integers(1, 25))
        H, W = int(g.integers(24, 121)), int(g.integers(40, 201))
        scale = (0.15, 0.4, 0.9)[case % 3]
        inp = synth.make_inputs(S, H, W, seed=300 + case, kind="smooth")
        y0, x0 = int(g.integers(0, H - 4)), int(g.integers(0, W - 4))
        y1, x1 = int(g.integers(y0 + 1, H + 1)), int(g.integers(x0 + 1, W + 1))
        mask = np.zeros((H, W), np.float32)
        mask[y0:y1, x0:x1] = g.random((y1 - y0, x1 - x0), dtype=np.float32)
        G_dyn = oracle.random_pose(rng, scale)
        G_cam = oracle.random_pose(rng, scale, base_motions=(0, 0, 0))
        b = _stage_ac(dev, inp, G_cam, G_dyn, mask)
        views = _views(dev, b, H, W)
        dead = N(ops.support_dead_tiles(views, S, H, W))
        ops.warp_composite_views(b["rgba"], views, interleaved=2)
        full = _views(dev, b, H, W, support=False)
        ops.warp_composite_views(b["rgba"], full, interleaved=2)
        torch.cuda.synchronize()
        oracle.set_exp_mode(1)
        try:
            o = oracle.render_pair(inp["image"], mask, inp["mpi"], inp["disparity"], inp["K"], G_cam, G_dyn)
        finally:
            oracle.set_exp_mode(0)
        for v, key in enumerate(("view_cam", "view_dyn")):
            d = _tile_mask(dead[v], H, W)
            assert not (o[key]["objmask"][d] != 0).any(), "case %d view %d: a dead tile holds a non-zero oracle objmask" % (case, v)
            # the launch skips exactly the tiles the query reports: zeros there, the full render's bits everywhere else
            for name in ("rgb", "objmask", "rgb_u8"):
                got, want = N(views[v]["out"][name]), N(full[v]["out"][name])
                dd = d[None] if name == "rgb" else (d[..., None] if name == "rgb_u8" else d)
                assert not (got * dd != 0).any() and bits_equal(np.where(dd, want, got), want) == 0, (case, v, name)
            assert bits_equal(N(full[v]["out"]["objmask"]), o[key]["objmask"]) == 0
            flagged += int(dead[v].sum())
            tiles += dead[v].size
    print("dead tiles: %d of %d" % (flagged, tiles))
    assert flagged > tiles // 10                                # the test above is not vacuous


def test_most_of_view_0_is_dead_on_the_benchmark_shape(dev):
    """bench.py's shape, mask and first 8 pose pairs (random.Random(114514): dynamic pose, then camera pose, scale 0.15)."""
    from mpiflow_amd import host_math, ops, pipeline, synth
    S, H, W = 64, 640, 960
    r = pipeline.PairRenderer(S, H, W, dev)
    K, disp = synth.intrinsics(H, W), synth.plane_disparities(S)
    rng = random.Random(114514)
    g = torch.Generator(device=dev).manual_seed(1000)
    mpi = torch.rand((S, 4, H, W), generator=g, device=dev)
    img = torch.rand((3, H, W), generator=g, device=dev)
    om = T(synth.soft_box_mask(H, W), dev)
    quads = [torch.empty((H, W, 4), dtype=torch.float32, device=dev) for _ in range(2)]
    sup = [ops.alloc_support_map(H, W, dev) for _ in range(2)]
    flows = torch.empty((2, 2, H, W), dtype=torch.float32, device=dev)
    for pair in range(8):
        G_dyn = host_math.generate_random_pose(0.15, rng=rng)
        G_cam = host_math.generate_random_pose(0.15, base_motions=(0, 0, 0), rng=rng)
        prep = r.prepare(K, disp, [G_cam, G_dyn])
        ops.src_blend_flow(mpi, img, want_rgba=False, out_flows=flows, dparams=prep["blend"], P=2, obj_mask=om, quads=quads[0], quads_complement=quads[1],
                           support=sup[0], support_complement=sup[1], tag=pair + 1)
        o = dict(rgb=flows, objmask=flows)                      # never written: the query launches no render
        views = [dict(dparams=prep["warp"][v], quads=quads[v], out=o, support=(sup[v], pair + 1, 0.99)) for v in range(2)]
        dead = N(ops.support_dead_tiles(views, S, H, W)).reshape(2, -1)
        share = dead.mean(axis=1)
        print("pair %d: dead share view 0 %.4f, view 1 %.4f" % (pair, share[0], share[1]))
        assert share[0] >= 0.85, share


def test_views_that_must_not_skip_equal_the_full_render_on_every_pixel(dev, oracle):
    from mpiflow_amd import ops, synth
    S, H, W = 7, 64, 160
    inp = synth.make_inputs(S, H, W, seed=12, kind="smooth")
    rng = random.Random(4)
    G_dyn = oracle.random_pose(rng, 0.15)
    G_cam = oracle.random_pose(rng, 0.15, base_motions=(0, 0, 0))
    b = _stage_ac(dev, inp, G_cam, G_dyn, inp["obj_mask"])
    full = _views(dev, b, H, W, support=False, depth=True)
    ops.warp_composite_views(b["rgba"], full, interleaved=2)
    assert int(ops.support_dead_tiles(_views(dev, b, H, W), S, H, W)[0].sum()) > 0        # something WOULD be skipped
    for kw in (dict(thresh=0.0), dict(thresh=-1.0), dict(depth=True)):
        views = _views(dev, b, H, W, **kw)
        assert int(ops.support_dead_tiles(views, S, H, W).sum()) == 0
        ops.warp_composite_views(b["rgba"], views, interleaved=2)
        torch.cuda.synchronize()
        for v in range(2):
            for name in views[v]["out"]:
                assert bits_equal(N(views[v]["out"][name]), N(full[v]["out"][name])) == 0, (kw, v, name)
    # and the pipelined renderer with thresh = 0 (view 0 is selected everywhere: 0 >= 0) hands back the oracle's products
    run_stream(dev, oracle, S, H, W, [inp["obj_mask"], np.zeros((H, W), np.float32), inp["obj_mask"]], 0.15, True, seed=5, thresh=0.0)
