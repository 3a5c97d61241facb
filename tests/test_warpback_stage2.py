"""Warp-back stage 2 (mpiflow_amd.warpback.networks / stage2_dataset, ops.stage2_* of mpf_stage2.hip) against

keys       tests/golden/edgeconnect_keys.json: the state-dict keys and shapes of the reference's three generators.
golden     tests/golden/stage2.npz: the reference's generators, filled with the closed-form weights of tests/stage2_pattern.py, on a 32 x 32
           input, in float32 and in float64 (tests/golden/make_stage2_golden.py, on the CPU).  The yardstick is the reference's own
           float32 error e_ref = max|ref32 - ref64|; the project's output on the GPU must lie within 4 e_ref of ref64.
torch      the expressions of the reference's inpaint, for the four pointwise launches: bit for bit.
composed   warp_and_inpaint against the same steps composed in the test, the generators behind recorders: the edge map, every generator's
           input and the merge of the recorded outputs bit for bit; the generators called directly, under the convolution library's
           deterministic setting (raft_train.reproducible), bit for bit as well.

The EdgeConnect checkpoints are installed nowhere: what real weights give is unpinned.
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import canny_restated as R  # noqa: E402
import stage2_pattern as P  # noqa: E402
from conftest import load_golden  # noqa: E402

F32 = np.float32
KEYS = ("src_rgb", "src_disp", "tgt_rgb", "tgt_disp", "warp_rgb", "warp_disp", "cam_int", "cam_ext")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def dev(built):
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    """the three generators with the pattern weights, spectral norm folded, on the GPU: built once, never modified"""
    from mpiflow_amd.warpback import networks
    return tuple(networks.fold_spectral_norm(P.load_pattern(P.build(networks, n))).to(dev) for n in P.GENERATORS)


# ---------------------------------------------------------------- CPU

def test_state_dict_keys_and_shapes_are_the_reference_s_and_load_strictly(built):
    import torch
    from mpiflow_amd.warpback import networks
    with open(os.path.join(HERE, "golden", "edgeconnect_keys.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted(P.GENERATORS)
    for name in P.GENERATORS:
        model = P.build(networks, name)
        got = {k: list(v.shape) for k, v in model.state_dict().items()}
        assert got == want[name], name
        sd = {k: torch.from_numpy(v) for k, v in P.pattern_state_dict(want[name]).items()}
        model.load_state_dict(sd, strict=True)
        fresh = P.build(networks, name)
        fresh.load_state_dict(sd, strict=True)
        networks.fold_spectral_norm(fresh)
        assert not any(k.endswith(("weight_orig", "weight_u", "weight_v")) for k in fresh.state_dict())
    edge = want["edge"]
    assert "encoder.1.weight_orig" in edge and "encoder.1.weight_u" in edge and "middle.7.conv_block.5.weight_v" in edge and "decoder.7.weight" in edge
    assert "middle.0.conv_block.1.bias" not in edge and "middle.0.conv_block.1.bias" in want["inpaint"]


def test_folded_weight_is_weight_orig_over_u_w_v(built):
    import torch
    from mpiflow_amd.warpback import networks
    model = P.load_pattern(P.build(networks, "edge"))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    networks.fold_spectral_norm(model)
    for key, dim in (("encoder.1", 0), ("decoder.0", 1), ("middle.3.conv_block.5", 0)):
        w, u, v = sd[key + ".weight_orig"], sd[key + ".weight_u"], sd[key + ".weight_v"]
        mat = w.transpose(0, dim).reshape(w.shape[dim], -1) if dim else w.reshape(w.shape[0], -1)
        sigma = torch.dot(u, torch.mv(mat, v))
        assert torch.allclose(model.state_dict()[key + ".weight"], w / sigma, rtol=1e-6, atol=0)


def test_without_models_and_without_checkpoints_the_error_names_the_three_files(built, tmp_path):
    from mpiflow_amd.warpback import WarpBackStage2Dataset, get_edge_connect
    for call in (lambda: WarpBackStage2Dataset(str(tmp_path), device="cpu", ec_weight_dir=str(tmp_path / "ecweight")), lambda: get_edge_connect(str(tmp_path))):
        with pytest.raises(FileNotFoundError) as e:
            call()
        for name in ("EdgeModel_gen.pth", "InpaintingModel_gen.pth", "InpaintingModel_disp.pth"):
            assert name in str(e.value)


def test_seeded_get_rand_ext_equals_stage_1_s(built, tmp_path):
    import torch
    from mpiflow_amd.warpback import WarpBackStage1Dataset, WarpBackStage2Dataset
    tr = {"x": 0.2, "y": 0.1, "z": 0.05, "a": 48, "b": 64, "c": 96}
    one = WarpBackStage1Dataset(str(tmp_path), device="cpu", trans_range=dict(tr))
    two = WarpBackStage2Dataset(str(tmp_path), device="cpu", trans_range=dict(tr), models=(torch.nn.Identity(),) * 3)
    assert WarpBackStage2Dataset.rand_tensor is WarpBackStage1Dataset.rand_tensor and WarpBackStage2Dataset.get_rand_ext is WarpBackStage1Dataset.get_rand_ext
    torch.manual_seed(11)
    a = one.get_rand_ext(3)
    ra = torch.rand(2)
    torch.manual_seed(11)
    b = two.get_rand_ext(3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(ra, torch.rand(2)) and a[0].shape == (3, 3, 4)
    assert (two.width, two.height, len(two)) == (384, 256, 0)


# ---------------------------------------------------------------- GPU: the generators

@pytest.mark.gpu
@pytest.mark.parametrize("name", P.GENERATORS)
def test_generator_is_within_4x_the_reference_s_own_float32_error(built, dev, models, name):
    import torch
    from mpiflow_amd.warpback import networks
    g = load_golden("stage2")
    x = P.golden_input(name)
    assert (x == g[name + "_in"]).all()
    ref32, ref64 = g[name + "_ref32"], g[name + "_ref64"]
    e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
    xd = torch.from_numpy(x).to(dev)
    folded = models[P.GENERATORS.index(name)](xd).cpu().numpy().astype(np.float64)
    unfolded = P.load_pattern(P.build(networks, name)).to(dev)(xd).cpu().numpy().astype(np.float64)
    e_folded, e_unfolded, e_between = (float(np.abs(a - b).max()) for a, b in ((folded, ref64), (unfolded, ref64), (folded, unfolded)))
    print("%s: e_ref %.3e  folded %.3e (ratio %.2f)  unfolded %.3e (ratio %.2f)  folded vs unfolded %.3e (ratio %.2f)"
          % (name, e_ref, e_folded, e_folded / e_ref, e_unfolded, e_unfolded / e_ref, e_between, e_between / e_ref))
    assert folded.shape == ref64.shape
    assert e_folded <= 4 * e_ref and e_unfolded <= 4 * e_ref and e_between <= 4 * e_ref


# ---------------------------------------------------------------- GPU: the pointwise chain

def _scene(dev, b, h, w):
    """(image [b,3,h,w], disp [b,1,h,w], cam_int, cam_ext, cam_ext_inv) on the device: smooth colours, a near block on a sloped background"""
    import torch
    from mpiflow_amd.host_math import transformation_from_parameters
    y, x = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
    rgb = np.stack([[0.5 + 0.4 * np.sin(7 * x + c + i) * np.cos(5 * y - c) for c in range(3)] for i in range(b)])
    rgb += 0.3 * (((np.floor(6 * x) + np.floor(4 * y)) % 2) == 0)
    block = (np.abs(x - 0.5) < 0.2) & (np.abs(y - 0.5) < 0.25)
    disp = np.stack([np.where(block, 0.9, 0.25 + 0.03 * x + 0.02 * y + 0.01 * i)[None] for i in range(b)])
    axisangle = torch.tensor([[[0.0, 0.02 * (i + 1), 0.0]] for i in range(b)])
    translation = torch.tensor([[[0.12 * (1 if i % 2 == 0 else -1), 0.02, 0.0]] for i in range(b)])
    M = transformation_from_parameters(axisangle, translation)
    K = torch.tensor([[0.58, 0, 0.5], [0, 0.58, 0.5], [0, 0, 1]]).repeat(b, 1, 1)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev).contiguous()  # noqa: E731
    return t(np.clip(rgb, 0, 1)), t(disp), K.to(dev), M[:, :-1].contiguous().to(dev), torch.inverse(M)[:, :-1].contiguous().to(dev)


def _masks(dev):
    """masks [2,1,9,13]: exact 0.0 / 1.0; fractional; and what render_mesh returns (the visibility interpolated over a face is fractional in places)"""
    import torch
    from mpiflow_amd.warpback import RGBDRenderer
    rng = np.random.RandomState(3)
    exact = torch.from_numpy((rng.rand(2, 1, 9, 13) > 0.4).astype(F32)).to(dev)
    frac = torch.from_numpy(rng.rand(2, 1, 9, 13).astype(F32)).to(dev)
    image, disp, K, E, _ = _scene(dev, 2, 9, 13)
    r = RGBDRenderer(dev)
    rendered = r.render_mesh(r.construct_mesh(torch.cat([image, disp], 1), K), K, E)
    return {"exact": (None, None, exact), "fractional": (None, None, frac), "rendered": tuple(t.contiguous() for t in rendered)}


@pytest.mark.gpu
def test_pointwise_chain_equals_the_torch_expressions_bit_for_bit(built, dev):
    import torch
    from mpiflow_amd import ops
    rng = np.random.RandomState(5)
    rnd = lambda *s: torch.from_numpy(rng.rand(*s).astype(F32)).to(dev)  # noqa: E731
    seen_fraction = False
    for kind, (image, disp, mask) in _masks(dev).items():
        image = rnd(2, 3, 9, 13) if image is None else image
        disp = rnd(2, 1, 9, 13) if disp is None else disp
        seen_fraction |= kind == "rendered" and bool(((mask > 0) & (mask < 1)).any())
        # (a) torchvision's Grayscale, and 1 - mask
        gray, hole = ops.stage2_gray_hole(image, mask)
        r, g, b = image.unbind(dim=-3)
        assert torch.equal(gray, (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(dim=-3)), kind
        assert torch.equal(hole, 1 - mask), kind
        # (b)
        edge = (rnd(2, 1, 9, 13) > 0.7).float()
        assert torch.equal(ops.stage2_edge_input(gray, edge, hole), torch.cat([gray, edge, hole], dim=1)), kind
        # (c)
        edge_inpaint = rnd(2, 1, 9, 13)
        xi, xd = ops.stage2_gen_inputs(image, disp, hole, edge_inpaint)
        assert torch.equal(xi, torch.cat([image + hole, edge_inpaint], dim=1)) and xi.shape == (2, 4, 9, 13), kind
        assert torch.equal(xd, torch.cat([disp + hole, edge_inpaint], dim=1)) and xd.shape == (2, 2, 9, 13), kind
        # (d)
        image_inpaint, disp_inpaint = rnd(2, 3, 9, 13), rnd(2, 1, 9, 13)
        mi, md = ops.stage2_merge(image, image_inpaint, disp, disp_inpaint, hole)
        assert torch.equal(mi, image * (1 - hole) + image_inpaint * hole), kind
        assert torch.equal(md, disp * (1 - hole) + disp_inpaint * hole), kind
    print("render_mesh's mask has fractional values at 2x9x13:", seen_fraction)
    try:
        from torchvision import transforms
    except Exception:                                          # noqa: BLE001
        return
    image = rnd(2, 3, 9, 13)
    assert torch.equal(ops.stage2_gray_hole(image, rnd(2, 1, 9, 13))[0], transforms.Grayscale()(image))


def test_pointwise_chain_refuses_by_the_tensor_contract(built):
    import torch
    from mpiflow_amd import ops
    img, one = torch.zeros(2, 3, 9, 13), torch.zeros(2, 1, 9, 13)
    for call, text in ((lambda: ops.stage2_gray_hole(img, one), "image must live on the GPU"), (lambda: ops.stage2_gray_hole(img.double(), one), "image must be float32"),
                       (lambda: ops.stage2_gray_hole(img, img), "mask must be"), (lambda: ops.stage2_edge_input(one, one, img), "mask_hole must be"),
                       (lambda: ops.stage2_gen_inputs(img, img, one, one), "disp must be"), (lambda: ops.stage2_merge(img, one, one, one, one), "image_inpaint must be"),
                       (lambda: ops.stage2_edge_input(one, one, one, out=one), "out must be")):
        with pytest.raises(built.MpiFlowHipError, match=text):
            call()


# ---------------------------------------------------------------- GPU: end to end

def _recording(model):
    """`model` behind a module that keeps a copy of the input and of the output of every call (.calls), and hands the output on untouched"""
    import torch

    class Recording(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.model, self.calls = model, []

        def forward(self, x):
            y = self.model(x)
            self.calls.append((x.clone(), y.clone()))
            return y
    return Recording()


def _last(recorders):
    """(input, output) of each recorder's one call since the last _last: ((edge), (inpaint), (disp))"""
    calls = [r.calls for r in recorders]
    assert [len(c) for c in calls] == [1, 1, 1]
    return tuple(c.pop() for c in calls)


@pytest.mark.gpu
def test_warp_and_inpaint_equals_the_steps_composed_by_hand(built, dev, models):
    """warp_and_inpaint at 2 x 32 x 48 against the same steps composed here: warp_back's first render, canny_restated on the host, torch's
    glue, the generators.  The three generators sit behind recorders, so what warp_and_inpaint handed each of them and what it got back are
    on record: every input must equal the torch expression and src_rgb / src_disp the torch merge of the recorded outputs, bit for bit.
    That holds everything the project computes to exact equality; what a generator returns on the same bytes a second time is the
    generator's own matter and is checked apart (below)."""
    import torch
    from mpiflow_amd import ops, raft_train
    from mpiflow_amd.warpback import RGBDRenderer, WarpBackStage2Dataset, stage2_dataset, warp_and_inpaint
    b, h, w = 2, 32, 48
    image, disp, K, E, E_inv = _scene(dev, b, h, w)
    rec = tuple(_recording(m) for m in models)
    out = warp_and_inpaint(image, disp, K, E, E_inv, rec)
    assert tuple(out) == KEYS
    for k, c in (("src_rgb", 3), ("src_disp", 1), ("tgt_rgb", 3), ("tgt_disp", 1), ("warp_rgb", 3), ("warp_disp", 1)):
        assert out[k].shape == (b, c, h, w) and out[k].dtype == torch.float32, k
    assert out["cam_int"].shape == (b, 3, 3) and out["cam_ext"] is E_inv and out["tgt_rgb"] is image and out["tgt_disp"] is disp
    (edge_in, edge_inpaint), (image_in, image_inpaint), (disp_in, disp_inpaint) = _last(rec)

    # by hand: the first render, canny on the host, torch's glue
    r = RGBDRenderer(dev)
    warp_image, warp_disp, mask = r.render_mesh(r.construct_mesh(torch.cat([image, disp], 1), K), K, E)
    assert torch.equal(out["warp_rgb"], warp_image) and torch.equal(out["warp_disp"], warp_disp)
    cr, cg, cb = warp_image.unbind(dim=-3)
    gray = (0.2989 * cr + 0.587 * cg + 0.114 * cb).unsqueeze(dim=-3)
    wts = np.array(ops.canny_weights(2.0)[1], F32)
    gray_np, mask_np = gray.cpu().numpy(), mask.cpu().numpy()
    edge_np = np.stack([R.canny_restated(gray_np[i, 0], mask_np[i, 0], wts) for i in range(b)])[:, None]
    edge = torch.from_numpy(edge_np).to(dev)
    hole = 1 - mask
    print("hole == 1: %.3f  hole == 0: %.3f  fractional: %.3f  edge pixels: %d" % (float((hole == 1).float().mean()), float((hole == 0).float().mean()),
                                                                                  float(((hole > 0) & (hole < 1)).float().mean()), int(edge_np.sum())))
    assert bool((hole == 1).any()) and bool((hole < 1).any()) and edge_np.sum() > 20      # there are holes to fill and edges to find
    assert torch.equal(stage2_dataset.get_edge(gray.contiguous(), mask.contiguous()), edge)

    # the edge map is identical; so is every generator's input; src_rgb and src_disp are the torch merge of what the generators returned
    assert torch.equal(edge_in[:, 1:2], edge)
    assert torch.equal(edge_in, torch.cat([gray, edge, hole], dim=1))
    assert torch.equal(image_in, torch.cat([warp_image + hole, edge_inpaint], dim=1))
    assert torch.equal(disp_in, torch.cat([warp_disp + hole, edge_inpaint], dim=1))
    want_rgb = warp_image * (1 - hole) + image_inpaint * hole
    want_disp = warp_disp * (1 - hole) + disp_inpaint * hole
    assert torch.equal(out["src_rgb"], want_rgb) and torch.equal(out["src_disp"], want_disp)
    keep = (hole == 0)
    assert torch.equal(out["src_rgb"][keep.expand(-1, 3, -1, -1)], warp_image[keep.expand(-1, 3, -1, -1)]) and torch.equal(out["src_disp"][keep], warp_disp[keep])
    assert float((out["src_rgb"] - warp_image).abs().max()) > 0.05                        # the holes were filled with something

    # the generators called directly on the torch glue, under the convolution library's deterministic attribute (raft_train.reproducible):
    # the whole composition, the generators' forwards included, gives warp_and_inpaint's bytes
    with raft_train.reproducible():
        det = warp_and_inpaint(image, disp, K, E, E_inv, models)
        edge_model, inpaint_model, disp_model = models
        direct_edge = edge_model(torch.cat([gray, edge, hole], dim=1))
        direct_rgb = warp_image * (1 - hole) + inpaint_model(torch.cat([warp_image + hole, direct_edge], dim=1)) * hole
        direct_disp = warp_disp * (1 - hole) + disp_model(torch.cat([warp_disp + hole, direct_edge], dim=1)) * hole
    print("under reproducible(): src_rgb vs the direct composition: max abs difference %.3e; src_disp: %.3e"
          % (float((det["src_rgb"] - direct_rgb).abs().max()), float((det["src_disp"] - direct_disp).abs().max())))
    print("the default call vs the deterministic one: src_rgb %.3e; src_disp %.3e"
          % (float((out["src_rgb"] - det["src_rgb"]).abs().max()), float((out["src_disp"] - det["src_disp"]).abs().max())))
    assert torch.equal(det["src_rgb"], direct_rgb) and torch.equal(det["src_disp"], direct_disp)

    # identical wherever the hole mask is 0: a mask of exact zeros and ones keeps every valid pixel's bytes
    exact = (mask > 0.5).float()
    kept_rgb, kept_disp, kept_edge = stage2_dataset.inpaint(warp_image, warp_disp, exact, rec)
    (_, _), (_, exact_image_inpaint), (_, exact_disp_inpaint) = _last(rec)
    valid = exact == 1
    assert 0.3 < float(valid.float().mean()) < 0.98
    assert torch.equal(kept_rgb[valid.expand(-1, 3, -1, -1)], warp_image[valid.expand(-1, 3, -1, -1)]) and torch.equal(kept_disp[valid], warp_disp[valid])
    assert torch.equal(kept_rgb[(~valid).expand(-1, 3, -1, -1)], exact_image_inpaint[(~valid).expand(-1, 3, -1, -1)]) and torch.equal(kept_disp[~valid], exact_disp_inpaint[~valid])
    assert float((kept_rgb - warp_image)[(~valid).expand(-1, 3, -1, -1)].abs().max()) > 0.05

    # the dataset's collect_data: the same function behind the reference's eight keys
    ds = WarpBackStage2Dataset(os.path.join(HERE, "no_such_directory"), width=w, height=h, device=dev, models=rec)
    assert ds.edge_model is rec[0] and ds.inpaint_model is rec[1] and ds.disp_model is rec[2]
    torch.manual_seed(5)
    batch = ds.collect_data([(image[i].cpu(), disp[i].cpu()) for i in range(b)])
    (_, _), (_, batch_image_inpaint), (_, batch_disp_inpaint) = _last(rec)
    assert tuple(batch) == KEYS and batch["src_rgb"].shape == (b, 3, h, w) and batch["src_disp"].shape == (b, 1, h, w)
    assert batch["cam_int"].shape == (b, 3, 3) and batch["cam_ext"].shape == (b, 3, 4) and torch.equal(batch["tgt_rgb"], image) and torch.equal(batch["tgt_disp"], disp)
    torch.manual_seed(5)
    ext, ext_inv = ds.get_rand_ext(b)
    assert torch.equal(batch["cam_ext"].cpu(), ext_inv)
    bw_image, bw_disp, bw_mask = ds.renderer.render_mesh(ds.renderer.construct_mesh(torch.cat([image, disp], 1), batch["cam_int"]), batch["cam_int"], ext.to(dev).contiguous())
    assert torch.equal(batch["warp_rgb"], bw_image) and torch.equal(batch["warp_disp"], bw_disp)
    bw_hole = 1 - bw_mask
    assert torch.equal(batch["src_rgb"], bw_image * (1 - bw_hole) + batch_image_inpaint * bw_hole)
    assert torch.equal(batch["src_disp"], bw_disp * (1 - bw_hole) + batch_disp_inpaint * bw_hole)
    merged = ds.inpaint(warp_image, warp_disp, mask)
    (_, _), (_, m_image_inpaint), (_, m_disp_inpaint) = _last(rec)
    assert len(merged) == 2 and torch.equal(merged[0], warp_image * (1 - hole) + m_image_inpaint * hole) and torch.equal(merged[1], warp_disp * (1 - hole) + m_disp_inpaint * hole)

