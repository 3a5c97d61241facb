"""The warp-back RGB-D mesh renderer (ops.rgbd_mesh_vertices / ops.rasterize_grid of mpf_mesh.hip, mpiflow_amd.warpback) against

restated   tests/warpback_restated.py: the rasteriser's definition in numpy float32, every pixel against every
           face.  The kernel must give its bytes: pix_to_face, zbuf, bary and out, no pixel excluded.
golden     tests/golden/warpback.npz: what the reference's own RGBDRenderer hands to pytorch3d (verts_ndc, faces, face_attributes), its pose
           helpers and get_rand_ext's seeded draws, recorded on the CPU by tests/golden/make_warpback_golden.py.

pytorch3d is installed nowhere, so parity with pytorch3d's own arithmetic is unpinned; the definition is the contract.

Vertex stage, measured on an MI355X against the float64 restatement of the formulas (largest absolute error per component; the bound is 4 x
the reference's own float32 error, for a different association of the dot products and a closed-form inverse): see profiles/warpback/README.md.
"""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import warpback_restated as R  # noqa: E402
from conftest import bits_equal, load_golden  # noqa: E402
from make_warpback_golden import B as GB, H as GH, W as GW, RANGES, SEED, sample_rgbd  # noqa: E402

F32 = np.float32
SYMBOLS = ("mpf_rgbd_mesh_vertices", "mpf_rasterize_grid", "mpf_rasterize_grid_workspace")
K = np.array([[0.58, 0, 0.5], [0, 0.58, 0.5], [0, 0, 1]], F32)
IDENT = np.eye(4, dtype=F32)[:3]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def golden():
    g = load_golden("warpback")
    rgbd = sample_rgbd()
    assert np.float64(rgbd.astype(np.float64).sum()) == g["rgbd_sum"] and int(g["seed"]) == SEED
    g["rgbd"] = rgbd
    return g


@pytest.fixture(scope="module")
def dev(built):
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---------------------------------------------------------------- scenes

def scene(seed, b, h, w, kind):
    """[b,4,h,w] float32.  "step": a near block on a far, gently sloped background; "far": the same with the background's disparity 0 (a far
    region whose depths are all equal); "smooth": no discontinuity"""
    rng = np.random.default_rng(seed)
    rgb = rng.random((b, 3, h, w))
    y, x = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
    bg = 0.25 + 0.03 * x + 0.02 * y
    if kind == "smooth":
        disp = np.broadcast_to(bg + 0.02 * np.sin(4 * x) * np.cos(3 * y), (b, h, w))
    else:
        block = (np.abs(x - 0.5) < 0.2) & (np.abs(y - 0.5) < 0.25)
        disp = np.broadcast_to(np.where(block, 0.9, 0.0 if kind == "far" else bg), (b, h, w))
    return np.concatenate([rgb, disp[:, None]], axis=1).astype(F32)


def pose(b, seed):
    """[b,3,4] float32: translation in x, y and z and a small rotation (host_math: the reference's own helper, mirrored)"""
    import torch
    from mpiflow_amd.host_math import transformation_from_parameters
    rng = np.random.default_rng(seed)
    aa = torch.from_numpy((0.04 * (rng.random((b, 1, 3)) - 0.5)).astype(F32))
    tr = torch.from_numpy((np.array([0.2, 0.08, -0.1]) * rng.choice([-1.0, 1.0], (b, 1, 3))).astype(F32))
    return transformation_from_parameters(aa, tr)[:, :-1].contiguous().numpy()


def regular_verts(h, w, z=1.0):
    """[1,h*w,3]: vertex (r, c) exactly at the centre of pixel (r, c)"""
    px, py = R.pixel_centres(h, w)
    return np.stack([px, py, np.full((h, w), z, F32)], -1).reshape(1, h * w, 3).astype(F32)


# ---------------------------------------------------------------- without a GPU

def test_restated_rasteriser_gives_the_hand_worked_values():
    """3 x 3 vertices, axis-aligned cells, rows on the pixel rows.  a = 2/3 is the first pixel column's centre, the rows are at (a, 0, -a).
    Unfolded, columns at x = (2a, 0, -2a): pixel column 0 lies midway between vertex columns 0 and 1 on a mesh edge (barycentrics 1/2, 1/2, 0:
    the mean of the two attributes), column 1 on vertex column 1, column 2 midway between columns 1 and 2.
    Folded, columns at x = (2a, 0, a), z = (1, 1, 0.5): the second cell column lies over the first; pixel column 0 sits on its far vertices at
    z = 0.5 and hides the z = 1 faces under it; pixel column 1 sees z = 1; nothing reaches pixel column 2."""
    px, py = R.pixel_centres(3, 3)
    a = px[0, 0]
    assert abs(a - 2 / 3) < 1e-7 and px[0, 1] == 0 and px[0, 2] == -a and py[0, 0] == a and py[2, 0] == -a
    attr = np.arange(9, dtype=F32).reshape(1, 9, 1) * F32(0.125)          # vertex v carries v / 8
    A = attr[0, :, 0].reshape(3, 3)

    def mesh(xs, zs):
        v = np.zeros((3, 3, 3), F32)
        v[..., 0], v[..., 1], v[..., 2] = np.array(xs, F32)[None, :], py[:, :1], np.array(zs, F32)[None, :]
        return v.reshape(1, 9, 3)

    pix, zbuf, bary, out = R.rasterize(mesh([2 * a, 0, -2 * a], [1, 1, 1]), attr, 3, 3)
    assert (pix >= 0).all() and np.abs(zbuf - 1).max() < 1e-6
    want = np.stack([(A[:, 0] + A[:, 1]) / 2, A[:, 1], (A[:, 1] + A[:, 2]) / 2], -1)
    assert np.abs(out[0, 0] - want).max() < 1e-6
    assert np.abs(np.sort(bary[0, :, 0], -1) - np.array([0, 0.5, 0.5], F32)).max() < 1e-6      # on an edge, midway
    assert np.abs(np.sort(bary[0, :, 1], -1) - np.array([0, 0, 1], F32)).max() < 1e-6          # on a vertex
    assert np.abs(bary.sum(-1) - 1).max() < 1e-6

    pix, zbuf, bary, out = R.rasterize(mesh([2 * a, 0, a], [1, 1, 0.5]), attr, 3, 3)
    assert (pix[0, :, 2] == -1).all() and (zbuf[0, :, 2] == -1).all() and (bary[0, :, 2] == -1).all() and (out[0, 0, :, 2] == 0).all()
    assert np.abs(zbuf[0, :, 0] - 0.5).max() < 1e-6 and np.abs(zbuf[0, :, 1] - 1).max() < 1e-6
    assert np.abs(out[0, 0, :, 0] - A[:, 2]).max() < 1e-6 and np.abs(out[0, 0, :, 1] - A[:, 1]).max() < 1e-6
    faces = R.grid_faces(3, 3)
    assert all(set(faces[f]) & {2, 5, 8} for f in pix[0, :, 0])           # the winners of column 0 are faces of the folded, near column
    # the far face alone: the same pixel sees z = 1 once the near column is pushed behind the camera
    assert np.abs(R.rasterize(mesh([2 * a, 0, a], [1, 1, -3]), attr, 3, 3)[1][0, :, 0] - 1).max() < 1e-6
    # equal depth: the lowest face index wins
    flat = R.rasterize(regular_verts(3, 3), attr, 3, 3)[0]
    for r in range(3):
        for c in range(3):
            v = r * 3 + c
            assert flat[0, r, c] == min(f for f in range(8) if v in faces[f])


def test_get_faces_equals_the_golden(built, golden):
    from mpiflow_amd.warpback.utils import RGBDRenderer
    got = RGBDRenderer("cpu").get_faces(GH, GW)
    assert got.dtype.is_floating_point is False and tuple(got.shape) == (1, 2 * (GH - 1) * (GW - 1), 3)
    for b in range(GB):
        assert (got[0].numpy() == golden["faces"][b]).all()
    assert (R.grid_faces(GH, GW) == golden["faces"][0]).all()
    mesh = RGBDRenderer("cpu").construct_mesh(__import__("torch").from_numpy(golden["rgbd"]), __import__("torch").from_numpy(golden["cam_int"]))
    assert list(mesh.keys()) == ["vertice", "faces", "attributes", "size"] and mesh["size"] == [GH, GW]
    assert (mesh["faces"].numpy() == golden["faces"]).all() and mesh["faces"].dtype == __import__("torch").int64
    assert (mesh["attributes"].numpy() == golden["attributes"]).all()     # rgb and the visibility bit, by the same torch expressions
    assert np.abs(mesh["vertice"].numpy() - golden["vertice"]).max() < 1e-4 * np.abs(golden["vertice"]).max()
    fresh = RGBDRenderer("cpu").construct_mesh(__import__("torch").from_numpy(golden["rgbd"]), __import__("torch").from_numpy(golden["cam_int"]))
    assert list(fresh) == list(fresh.keys()) and len(fresh) == 4 and sorted(dict(fresh)) == ["attributes", "faces", "size", "vertice"]
    assert fresh.get("faces") is fresh["faces"] and fresh.get("nothing") is None and [k for k, _ in fresh.items()] == list(fresh.keys())
    assert not fresh._by_hand                                            # reading builds the tensors; only an assignment leaves the fused path
    fresh["attributes"] = fresh["attributes"].clone()
    assert fresh._by_hand


def test_pose_helpers_and_get_rand_ext_are_within_1e6_of_the_golden(built, golden):
    """entries of at most 1 in size through fewer than 16 float32 operations: 16 * 2^-24 < 1e-6"""
    import torch
    from mpiflow_amd.warpback.stage1_dataset import WarpBackStage1Dataset
    from mpiflow_amd.warpback.utils import RGBDRenderer, get_translation_matrix, rot_from_axisangle, transformation_from_parameters
    aa, tr = torch.from_numpy(golden["axisangle"]), torch.from_numpy(golden["translation"])
    assert np.abs(rot_from_axisangle(aa).numpy() - golden["rot"]).max() <= 1e-6
    assert np.abs(get_translation_matrix(tr).numpy() - golden["trans"]).max() <= 1e-6
    assert np.abs(transformation_from_parameters(aa, tr).numpy() - golden["M"]).max() <= 1e-6
    assert np.abs(transformation_from_parameters(aa, tr, invert=True).numpy() - golden["M_inv"]).max() <= 1e-6
    assert (RGBDRenderer("cpu").get_perspective_from_intrinsic(torch.from_numpy(golden["cam_int"])).numpy() == golden["persp"]).all()
    for i, rng in enumerate(RANGES):
        ds = WarpBackStage1Dataset(data_root=os.path.join(HERE, "no_such_directory"), device="cpu", trans_range=dict(rng))
        assert len(ds) == 0 and ds.width == 384 and ds.height == 256
        torch.manual_seed(SEED + i)
        ext, ext_inv = ds.get_rand_ext(4)
        assert tuple(ext.shape) == (4, 3, 4) and tuple(ext_inv.shape) == (4, 3, 4)
        assert np.abs(ext.numpy() - golden["rand_ext_%d" % i]).max() <= 1e-6
        assert np.abs(ext_inv.numpy() - golden["rand_ext_inv_%d" % i]).max() <= 1e-6
        assert (torch.rand(3).numpy() == golden["rand_after_%d" % i]).all()                    # the host generator was consumed alike
    assert (ds.rand_tensor(-1, 5) == 0).all() and tuple(ds.rand_tensor(0.2, 5).shape) == (5, 1, 1)
    t = ds.rand_tensor(0.2, 64).abs()
    assert float(t.min()) >= 0.1 and float(t.max()) <= 0.2


def test_c_abi_declares_and_exports_the_mesh_symbols(built):
    import ctypes
    hdr = open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(built.LIB_PATH)
    for n in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, plain) and hasattr(lib, n) and n in built.SIGNATURES
    assert re.search(r"#define\s+MPF_MESH_MAX_ATTRS\s+%d\b" % built.MESH_MAX_ATTRS, hdr) and re.search(r"#define\s+MPF_MESH_MAX_BHW\s+%d\b" % built.MESH_MAX_BHW, hdr)
    lib = built.load()
    assert lib.mpf_rasterize_grid(None, None) == 10001 and b"null argument block" in lib.mpf_last_error()
    assert lib.mpf_rgbd_mesh_vertices(None, None) == 10001
    assert lib.mpf_rasterize_grid_workspace(2, 40, 72) == 2 * 40 * 72 * 8
    assert lib.mpf_rasterize_grid_workspace(1, 1, 72) == 0 and lib.mpf_rasterize_grid_workspace(1, 1 << 14, 1 << 15) == 0
    a = built.MpfMeshRasterArgs()
    a.B, a.h, a.w, a.C = 1, 4, 4, 9
    assert lib.mpf_rasterize_grid(ctypes.byref(a), None) == 10001 and b"C must be" in lib.mpf_last_error()
    a.C, a.h = 5, 1
    assert lib.mpf_rasterize_grid(ctypes.byref(a), None) == 10001 and b"h, w >= 2" in lib.mpf_last_error()


def test_identity_extrinsic_returns_the_image_times_its_visibility_restated():
    """Every pixel centre sits on its own vertex: the barycentric error is at most the rounding of px (about 1e-7) over a cell (about 5e-3 at
    this size or larger), the attributes differ by at most 1 between neighbours: 1e-4."""
    rgbd = scene(11, 1, 12, 18, "smooth")
    render, disp, mask = R.render_mesh(rgbd, K[None], IDENT[None])
    vis = (R.sobel_alpha(rgbd[:, 3], F32) > F32(0.3)).astype(F32)[:, None]
    assert 0.3 < vis.mean() < 1.0                                         # the Sobel's zero padding hides the border
    assert np.abs(mask - vis).max() <= 1e-4
    assert np.abs(render - rgbd[:, :3] * vis).max() <= 1e-4
    assert np.abs(disp - rgbd[:, 3:] * vis).max() <= 1e-4


def _refusals(ops, Err, z):
    v, at = z(1, 20, 3), z(1, 20, 5)
    import torch
    with pytest.raises(Err, match="float32"):
        ops.rasterize_grid(z(1, 20, 3, dtype=torch.float64), at, 4, 5)
    with pytest.raises(Err, match="float32"):
        ops.rasterize_grid(v, z(1, 20, 5, dtype=torch.float16), 4, 5)
    with pytest.raises(Err, match="3 dimensions"):
        ops.rasterize_grid(z(1, 20, 4), at, 4, 5)
    with pytest.raises(Err, match="3 dimensions"):
        ops.rasterize_grid(v, z(2, 20, 5), 4, 5)
    with pytest.raises(Err, match="contiguous"):
        ops.rasterize_grid(z(1, 3, 20).transpose(1, 2), at, 4, 5)
    with pytest.raises(Err, match="h \\* w"):
        ops.rasterize_grid(v, at, 4, 6)
    with pytest.raises(Err, match="at least 2"):
        ops.rasterize_grid(v, at, 1, 20)
    with pytest.raises(Err, match="1..8 channels"):
        ops.rasterize_grid(v, z(1, 20, 9), 4, 5)
    with pytest.raises(Err, match="blur_radius"):
        ops.rasterize_grid(v, at, 4, 5, blur_radius=-1.0)
    with pytest.raises(Err, match="torch.Tensor"):
        ops.rgbd_mesh_vertices(np.zeros((1, 4, 4, 4), F32), z(1, 3, 3), z(1, 3, 4))
    with pytest.raises(Err, match="float32"):
        ops.rgbd_mesh_vertices(z(1, 4, 4, 4, dtype=torch.float64), z(1, 3, 3), z(1, 3, 4))
    with pytest.raises(Err, match="4 dimensions"):
        ops.rgbd_mesh_vertices(z(1, 3, 4, 4), z(1, 3, 3), z(1, 3, 4))
    with pytest.raises(Err, match="cam_int"):
        ops.rgbd_mesh_vertices(z(2, 4, 4, 4), z(1, 3, 3), z(2, 3, 4))
    with pytest.raises(Err, match="cam_ext must be contiguous"):
        ops.rgbd_mesh_vertices(z(2, 4, 4, 4), z(2, 3, 3), z(2, 4, 4)[:, :-1])      # a [b,4,4] pose without its last row, not made contiguous
    with pytest.raises(Err, match="h, w >= 2"):
        ops.rgbd_mesh_vertices(z(1, 4, 1, 8), z(1, 3, 3), z(1, 3, 4))


def test_refusals_come_in_the_order_of_the_contract_and_the_device_last(built):
    import torch
    from mpiflow_amd import ops
    _refusals(ops, built.MpiFlowHipError, lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype))
    with pytest.raises(built.MpiFlowHipError, match="no CPU path"):
        ops.rasterize_grid(torch.zeros(1, 20, 3), torch.zeros(1, 20, 5), 4, 5)
    with pytest.raises(built.MpiFlowHipError, match="no CPU path"):
        ops.rgbd_mesh_vertices(torch.zeros(1, 4, 4, 5), torch.zeros(1, 3, 3), torch.zeros(1, 3, 4))


# ---------------------------------------------------------------- on the GPU

def _gpu_raster(dev, verts, attrs, h, w, blur=1e-6):
    import torch
    from mpiflow_amd import ops
    got = ops.rasterize_grid(torch.from_numpy(verts).to(dev), torch.from_numpy(attrs).to(dev), h, w, blur)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in got]


def _same_as_restated(dev, verts, attrs, h, w, what, blur=1e-6):
    want = R.rasterize(verts, attrs, h, w, blur)
    got = _gpu_raster(dev, verts, attrs, h, w, blur)
    again = _gpu_raster(dev, verts, attrs, h, w, blur)
    diffs = [bits_equal(g, x) for g, x in zip(got, want)]
    print("%-28s %dx%dx%d: words that differ (pix_to_face, zbuf, bary, out) = %s; %d of %d pixels covered"
          % (what, verts.shape[0], h, w, diffs, int((want[0] >= 0).sum()), want[0].size))
    assert diffs == [0, 0, 0, 0], (what, diffs)
    assert [bits_equal(g, x) for g, x in zip(got, again)] == [0, 0, 0, 0], "two runs differ"
    assert want[0].dtype == np.int64 and got[0].dtype == np.int64
    return want


# 9 x 18: 272 faces, one more cell row and column than the 256 faces of a z-pass workgroup (8 x 16 cells); 17 x 17: 289 pixels, past one
# resolve workgroup
SHAPES = [(1, 5, 7), (1, 16, 24), (1, 24, 16), (1, 17, 17), (1, 9, 18), (2, 40, 72)]


@pytest.mark.gpu
@pytest.mark.parametrize("b,h,w", SHAPES)
@pytest.mark.parametrize("kind", ["step", "far"])
def test_rasterize_grid_equals_the_restatement_bit_for_bit(built, dev, kind, b, h, w):
    """(a) step: stretched, folded, back-facing and off-screen faces; (b) far: a region at disparity 0 whose depths are bit-equal (the tie rule)"""
    rgbd = scene(100 + h, b, h, w, kind)
    verts, attrs = R.mesh_vertices(rgbd, np.broadcast_to(K, (b, 3, 3)), pose(b, 200 + w), F32)
    want = _same_as_restated(dev, verts, attrs, h, w, kind)
    cov = (want[0] >= 0).mean()
    assert 0.3 < cov < 1.0, cov                                           # most of the frame is drawn, some of it is off the mesh
    if kind == "far":
        z = want[1][want[0] >= 0]
        assert len(np.unique(z)) < 0.8 * len(z)                           # bit-equal depths did occur


@pytest.mark.gpu
def test_rasterize_grid_degenerate_faces_equal_the_restatement(built, dev):
    """(c) hand-made: every pixel centre exactly on a vertex, and on an edge; coincident corners, a face of no area, a NaN vertex, an inf
    vertex, faces wholly behind the camera"""
    h, w = 5, 7
    v = regular_verts(h, w)
    attrs = np.random.default_rng(5).random((1, h * w, 8)).astype(F32)
    _same_as_restated(dev, v, attrs, h, w, "regular, centres on vertices")
    v[0, 1 * w + 1] = v[0, 1 * w + 2]                                     # coincident corners: zero-area faces around them
    # two slivers of non-zero area on either side of the skip rule, at column 3, where x is about 0 and float32 resolves 1e-8: the lower-left
    # face (tl, bl, br) of a cell has area (br.x - tl.x) * (bl.y - tl.y) when tl.x == bl.x, and the rows are 0.4 apart.
    #   cell (0, 3), face 3:  br.x = -1.5e-8, |area| = 6e-9  <= 1e-8: skipped.  Drawn, its weights would be scaled by area / den = 3/8 and its
    #                         depth 0.375 would beat the 1.0 of its neighbours at pixel (0, 3)
    #   cell (2, 3), face 15: br.x = -5e-8,   |area| = 2e-8  >  1e-8: drawn with den = area + 1e-8, so its weights are scaled by 2/3 and its
    #                         depth 0.667 DOES beat its neighbours at pixel (2, 3)
    for r, x in ((0, -1.5e-8), (2, -5e-8)):
        v[0, r * w + 3, 0] = v[0, (r + 1) * w + 3, 0] = 0.0
        v[0, (r + 1) * w + 4, 0] = x
    v[0, 0 * w + 5, 0] = np.nan
    v[0, 4 * w + 0, 1] = np.inf
    v[0, [2 * w + 5, 2 * w + 6, 3 * w + 6, 3 * w + 5], 2] = -1.0          # one cell wholly behind; its neighbours partly (pz < 0 at some pixels)
    want = _same_as_restated(dev, v, attrs, h, w, "degenerate")
    assert (want[0] < 0).any() and (want[0] >= 0).any()
    area = lambda f: R.edge(*[v[0, i, k] for i in R.grid_faces(h, w)[f][[2, 0, 1]] for k in (0, 1)])
    assert 0 < abs(area(3)) <= 1e-8 and abs(area(3)) > 3e-9, area(3)
    assert 1e-8 < abs(area(15)) < 3e-8, area(15)
    assert (want[0] != 3).all() and want[1][0, 0, 3] > 0.99                                  # the 6e-9 face is skipped: pixel (0, 3), its tl, keeps depth 1
    assert want[0][0, 2, 3] == 15 and abs(want[1][0, 2, 3] - 2 / 3) < 1e-3                   # the 2e-8 face is drawn at its tl, with den = area + 1e-8
    assert sum(abs(area(f)) == 0 for f in range(2 * (h - 1) * (w - 1))) >= 2                 # and the coincident corners' exact zeros
    half = regular_verts(h, w)
    half[0, :, 0] *= F32(0.5)                                             # centres on edges and between vertices, columns folded to half width
    _same_as_restated(dev, half, attrs, h, w, "half width")
    _same_as_restated(dev, regular_verts(h, w), attrs, h, w, "no blur", blur=0.0)


@pytest.mark.gpu
def test_rasterize_grid_one_face_over_the_whole_frame(built, dev):
    """(d) one cell's lower-left face covers every pixel (its wave walks the whole frame), every other vertex sits on one far point"""
    h, w = 16, 24
    v = np.zeros((1, h * w, 3), F32)
    v[..., 0], v[..., 1], v[..., 2] = 50.0, 50.0, 2.0
    q = 7 * w + 11
    v[0, q], v[0, q + w], v[0, q + w + 1] = (9.0, 21.0, 1.0), (9.0, -21.0, 1.5), (-33.0, -21.0, 0.5)
    attrs = np.random.default_rng(6).random((1, h * w, 3)).astype(F32)
    want = _same_as_restated(dev, v, attrs, h, w, "one face")
    assert (want[0] == 7 * (w - 1) + 11).all()


@pytest.mark.gpu
def test_rasterize_grid_large_thin_faces_keep_every_pixel_of_a_strip(built, dev):
    """The bounding box must not change a pixel.  64 x 96, seeded: bands of vertex columns squeezed in x by 1e-3 .. 1e-6 and stretched in y by
    3 .. 6 about the frame's centre, tilted a little, so that long faces are seen nearly edge-on, with areas from 1e-5 down through the 1e-8
    skip rule, many of them far larger than MESH_HEAVY pixels in their boxes and some below the kernel's no-cull threshold.  The restatement
    (no box of any kind) is too slow for the frame, so three strips of rows are compared: top, middle, bottom."""
    h, w = 64, 96
    rng = np.random.default_rng(77)
    v = regular_verts(h, w).reshape(h, w, 3)
    v[..., 2] = (1 + rng.random((h, w))).astype(F32)
    for c0, squeeze in ((8, 1e-3), (24, 1e-4), (40, 1e-5), (56, 3e-6), (72, 1e-6)):
        cols = slice(c0, c0 + 8)
        x0 = v[0, c0, 0]
        tilt = F32(rng.uniform(-0.02, 0.02))
        v[:, cols, 0] = (x0 + (v[:, cols, 0] - x0) * F32(squeeze) + tilt * v[:, cols, 1]).astype(F32)
        v[:, cols, 1] *= F32(rng.uniform(3, 6))
    v = v.reshape(1, h * w, 3)
    attrs = rng.random((1, h * w, 2)).astype(F32)
    faces = R.grid_faces(h, w)
    a, b, c = (v[0, faces[:, k]] for k in (0, 1, 2))
    area = np.abs(R.edge(c[:, 0], c[:, 1], a[:, 0], a[:, 1], b[:, 0], b[:, 1]))
    assert ((area > 0) & (area <= 1e-8)).sum() > 50 and ((area > 1e-8) & (area < 1e-6)).sum() > 50
    got = _gpu_raster(dev, v, attrs, h, w)
    again = _gpu_raster(dev, v, attrs, h, w)
    assert [bits_equal(g, x) for g, x in zip(got, again)] == [0, 0, 0, 0]
    thin = 0
    for rows in (slice(0, 3), slice(31, 34), slice(61, 64)):
        want = R.rasterize(v, attrs, h, w, rows=rows)
        diffs = [bits_equal(got[0][:, rows], want[0]), bits_equal(got[1][:, rows], want[1]), bits_equal(got[2][:, rows], want[2]),
                 bits_equal(got[3][:, :, rows], want[3])]
        won = want[0][want[0] >= 0]
        thin += int((area[won] < 1e-6).sum())
        print("thin faces, rows %2d..%2d: words that differ = %s; %d of %d pixels covered" % (rows.start, rows.stop - 1, diffs, len(won), want[0].size))
        assert diffs == [0, 0, 0, 0], (rows, diffs)
    assert thin > 0                                                       # thin faces did win pixels of the strips


@pytest.mark.gpu
def test_vertex_stage_against_the_golden(built, dev, golden):
    import torch
    from mpiflow_amd import ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    verts, attrs = ops.rgbd_mesh_vertices(t(golden["rgbd"]), t(golden["cam_int"]), t(golden["cam_ext"]))
    torch.cuda.synchronize()
    verts, attrs = verts.cpu().numpy(), attrs.cpu().numpy()
    assert verts.shape == (GB, GH * GW, 3) and attrs.shape == (GB, GH * GW, 5) and verts.dtype == F32
    v64, a64 = R.mesh_vertices(golden["rgbd"], golden["cam_int"], golden["cam_ext"], np.float64)
    nf = golden["faces"].shape[1]
    ref_attr = np.zeros((GB, GH * GW, 5), F32)                            # the reference's per-vertex attributes, back from its face_attributes
    fa = golden["face_attributes"].reshape(GB, nf, 3, 5)
    for b in range(GB):
        ref_attr[b, golden["faces"][b].reshape(-1)] = fa[b].reshape(-1, 5)
    pairs = [("x", verts[..., 0], golden["verts_ndc"][..., 0], v64[..., 0]), ("y", verts[..., 1], golden["verts_ndc"][..., 1], v64[..., 1]),
             ("z", verts[..., 2], golden["verts_ndc"][..., 2], v64[..., 2]), ("depth", attrs[..., 4], ref_attr[..., 4], a64[..., 4])]
    for name, mine, ref, exact in pairs:
        e_mine, e_ref = np.abs(mine - exact).max(), np.abs(ref - exact).max()
        print("vertex stage %-5s largest error against float64: kernel %.3e, reference %.3e" % (name, e_mine, e_ref))
    for name, mine, ref, exact in pairs:
        assert np.abs(mine - exact).max() <= 4 * np.abs(ref - exact).max(), name
    assert bits_equal(attrs[..., :3], ref_attr[..., :3]) == 0
    band = golden["near_threshold"]
    assert band.mean() <= 0.005
    assert (attrs[..., 3][~band] == ref_attr[..., 3][~band]).all()


@pytest.mark.gpu
def test_render_mesh_is_the_two_kernels_and_the_stated_tail(built, dev):
    import torch
    from mpiflow_amd import ops
    from mpiflow_amd.warpback.utils import RGBDRenderer
    b, h, w = 2, 24, 36
    rgbd = torch.from_numpy(scene(31, b, h, w, "step")).to(dev)
    cam_int = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(K, (b, 3, 3)))).to(dev)
    cam_ext = torch.from_numpy(pose(b, 32)).to(dev)
    r = RGBDRenderer(dev)
    mesh = r.construct_mesh(rgbd, cam_int)
    render, disp, mask = r.render_mesh(mesh, cam_int, cam_ext)
    verts, attrs = ops.rgbd_mesh_vertices(rgbd, cam_int, cam_ext)
    pix, _, _, out = ops.rasterize_grid(verts, attrs, h, w, 1e-6)
    m = out[:, 3:4]
    assert torch.equal(mask, m) and torch.equal(render, out[:, :3] * m) and torch.equal(disp, torch.reciprocal(out[:, 4:5] + 1e-4) * m)
    assert tuple(render.shape) == (b, 3, h, w) and tuple(disp.shape) == (b, 1, h, w) and tuple(mask.shape) == (b, 1, h, w)
    # the hand-made dict: transformed in torch.  At the identity pose every vertex sits on its own pixel's centre, so only the faces that hold
    # a pixel's own vertex reach the pixel (the blur radius is an eightieth of a pixel here), and their vertices lie in the 3 x 3 block around
    # it: where the two paths' vertices are bit-equal over that block, the same face wins.  (Elsewhere every pixel is a tie that the
    # last bit of a vertex decides.)
    smooth = torch.from_numpy(scene(33, b, h, w, "smooth")).to(dev)
    small = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(IDENT, (b, 3, 4)))).to(dev)
    fused = r.construct_mesh(smooth, cam_int)
    hand = {"vertice": fused["vertice"], "attributes": fused["attributes"], "size": [h, w]}
    v1 = ops.rgbd_mesh_vertices(smooth, cam_int, small)[0]
    v2, a2 = r._transform(hand["vertice"], hand["attributes"], cam_int, small, h, w)
    p1 = ops.rasterize_grid(v1, ops.rgbd_mesh_vertices(smooth, cam_int, small)[1], h, w)[0]
    p2 = ops.rasterize_grid(v2, a2, h, w)[0]
    r2 = r.render_mesh(hand, cam_int, small)
    assert torch.equal(r2[2], ops.rasterize_grid(v2, a2, h, w)[3][:, 3:4])
    same = (v1 == v2).all(-1).reshape(b, 1, h, w).float()
    near = -torch.nn.functional.max_pool2d(-same, 3, 1, 1)                # 1 where every vertex of the 3 x 3 block is bit-equal
    sel = near[:, 0] > 0
    print("hand-made dict: %d of %d vertices bit-equal to the fused path's, %d pixels compared" % (int(same.sum()), same.numel(), int(sel.sum())))
    assert torch.equal(p1[sel], p2[sel])


@pytest.mark.gpu
def test_warp_back_keys_mask_and_the_side_of_the_holes(built, dev):
    import torch
    from mpiflow_amd.warpback import WarpBackStage1Dataset, warp_back
    b, h, w = 2, 24, 96
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cam_int = t(np.broadcast_to(K, (b, 3, 3)))
    ident = t(np.broadcast_to(IDENT, (b, 3, 4)))
    sm = scene(41, b, h, w, "smooth")
    d = warp_back(t(sm[:, :3]), t(sm[:, 3:]), cam_int, ident, ident)
    assert list(d) == ["rgb", "disp", "mask", "warp_rgb", "warp_disp", "warp_back_rgb", "warp_back_disp"]
    for k, c in (("rgb", 3), ("disp", 1), ("mask", 1), ("warp_rgb", 3), ("warp_disp", 1), ("warp_back_rgb", 3), ("warp_back_disp", 1)):
        assert tuple(d[k].shape) == (b, c, h, w) and d[k].dtype == torch.float32 and d[k].device == dev, k
    # zero translation: every centre on its vertex in both renders, so the mask is the visibility of the first render's disparity
    wd = d["warp_disp"].cpu().numpy()
    alpha2 = R.sobel_alpha(wd[:, 0], F32)
    vis1 = (R.sobel_alpha(sm[:, 3], F32) > F32(0.3)).astype(F32)
    assert np.abs(wd[:, 0] - sm[:, 3] * vis1).max() <= 1e-4
    clear = np.abs(alpha2 - F32(0.3)) >= 1e-5
    assert clear.mean() > 0.99
    mask = d["mask"].cpu().numpy()[:, 0]
    assert np.abs(mask - (alpha2 > F32(0.3)))[clear].max() <= 1e-4
    assert 0.2 < mask.mean() < 1.0

    # the reference's x = 0.2 through collect_data: the near block (columns 0.3 w .. 0.7 w) moves further than the background, so the
    # novel view hides a strip of background, 0.58 |t_x| (0.9 - 0.27) w = 3.5 to 7 pixels wide, on the side the block moves to, and the
    # warp-back holes lie there, on top of the Sobel bands that both edges of the block get alike.  Counted within 12 pixels of each edge,
    # clear of the frame's own border.
    st = scene(42, b, h, w, "step")
    ds = WarpBackStage1Dataset(data_root=os.path.join(HERE, "no_such_directory"), width=w, height=h, device=dev)
    torch.manual_seed(3)
    out = ds.collect_data([(torch.from_numpy(st[i, :3]), torch.from_numpy(st[i, 3:])) for i in range(b)])
    assert list(out) == list(d) and tuple(out["mask"].shape) == (b, 1, h, w)
    torch.manual_seed(3)
    ext = ds.get_rand_ext(b)[0]
    holes = (out["mask"].cpu().numpy()[:, 0] < 0.5)
    rows = slice(int(0.3 * h), int(0.7 * h))
    x0, x1 = int(round(0.3 * w)), int(round(0.7 * w))
    for i in range(b):
        right, left = holes[i, rows, x1:x1 + 12].sum(), holes[i, rows, x0 - 12:x0].sum()
        moved_right = float(ext[i, 0, 3]) > 0
        print("sample %d: t_x = %+.3f, holes left of the block %d, right of it %d" % (i, float(ext[i, 0, 3]), left, right))
        assert (right > left) if moved_right else (left > right)


@pytest.mark.gpu
def test_refusals_on_the_device(built, dev):
    import torch
    from mpiflow_amd import ops
    _refusals(ops, built.MpiFlowHipError, lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev))
    with pytest.raises(built.MpiFlowHipError, match="no CPU path"):
        ops.rasterize_grid(torch.zeros(1, 20, 3, device=dev), torch.zeros(1, 20, 5), 4, 5)
