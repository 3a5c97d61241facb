"""GPU checks for the plane-adjustment network: ops.pan_block1 (csrc/mpf_pan.hip) against the reference's recorded float64 run on every case of
tests/golden/pan.npz, the fused DepthPredictionNetwork.forward against the same module's torch path and against the golden, the whole
MPIPredictor(adjust_planes=True), the engines' per-call plane set, and the loader path end to end with its refusal.

The bar, per case: max |got - f64| / max |f64| <= max(4 * e_ref, 1e-6), e_ref being the reference's own float32 run held against its float64 run
(tests/test_render_grad.py's rule).  Each comparison prints its error and the fraction of the bar it uses (pytest -s)."""
import numpy as np
import pytest
import torch

from test_pan_host import load_pan_golden, mg, seeded_dpn          # mg: tests/golden/make_pan_golden.py (cases, seeded inputs and parameters)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from mpiflow_amd import _lib
    _lib.load()                                                               # the library as built (python __graft_entry__.py); a missing one raises
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return load_pan_golden()


def held(what, got, f64, e_ref, absmax=None):
    scale = float(np.abs(f64).max()) if absmax is None else float(absmax)
    err, bar = float(np.abs(np.asarray(got, np.float64) - f64).max()) / scale, max(4.0 * float(e_ref), 1e-6)
    print("%s: err %.3e  e_ref %.3e  bar %.3e  (%.0f %% of the bar)" % (what, err, float(e_ref), bar, 100 * err / bar))
    return err <= bar


def case(name, dev):
    B, S, h, w, seed = mg.CASES[name]
    d = {k: torch.from_numpy(v).to(dev) for k, v in mg.case_inputs(B, S, h, w, seed).items()}
    return seeded_dpn(S, seed)[0].to(dev), d, seed


def fused_block1(dpn, d):
    with torch.no_grad():
        return dpn.block1(d["init_disp"], d["rgb_low"], d["disp_low"], fused=True)


@pytest.mark.parametrize("name", list(mg.CASES))
def test_block1_against_the_float64_golden_and_identical_bytes(dev, gold, name):
    """33 x 47: partial tiles, the dropped row and column; S = 1 and S = 5: a partial plane group (4 planes per workgroup); B = 2: the second image's planes"""
    dpn, d, seed = case(name, dev)
    B, S, h, w, _ = mg.CASES[name]
    out = fused_block1(dpn, d)
    again = fused_block1(dpn, d)
    assert out.shape == (B * S, 8, h // 2, w // 2) and out.dtype == torch.float32 and torch.equal(out, again)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert held(name + " block1", mg.kept(got, seed), gold[name + "/block1_f64"], gold[name + "/block1_e_ref"], gold[name + "/block1_absmax"])
    with torch.no_grad():                                                     # the torch form of the same module, the whole array
        ref = dpn.block1(d["init_disp"], d["rgb_low"], d["disp_low"], fused=False)
    assert float((out - ref).abs().max()) <= 1e-5 * float(gold[name + "/block1_absmax"])      # two float32 sums in different orders


@pytest.mark.parametrize("name", list(mg.CASES))
def test_fused_forward_against_the_torch_path_and_the_golden(dev, gold, name, monkeypatch):
    from mpiflow_amd import ops
    dpn, d, _ = case(name, dev)
    calls = []
    real = ops.pan_block1
    monkeypatch.setattr(ops, "pan_block1", lambda *a, **k: calls.append(1) or real(*a, **k))
    args = (d["init_disp"], d["rgb_low"], d["disp_low"])
    with torch.no_grad():
        fused = dpn(*args)
    assert calls == [1]
    assert any(p.requires_grad for p in dpn.parameters()) and torch.is_grad_enabled()
    torch_out = dpn(*args)                                                    # grad mode, parameters that require grad: the torch path carries the gradient
    assert calls == [1] and torch_out.requires_grad and not fused.requires_grad
    for p in dpn.parameters():
        p.requires_grad_(False)
    nograd = dpn(*args)                                                       # grad mode, but nothing wants a gradient: fused again
    assert calls == [1, 1] and not nograd.requires_grad
    f64, e_ref = gold[name + "/dpn_f64"], gold[name + "/dpn_e_ref"]
    # the fused path asks torch for MIOpen's deterministic algorithms in blocks 2-5 (their default choice differs from call to call in one
    # process: at 33 x 47, S = 5 a second call once sat at 1.4e-6 and a first at 2.4e-6, past the bar): an image gets the same planes every time
    assert torch.equal(nograd, fused)
    ok_gold = held(name + " fused forward vs golden", fused.cpu().numpy(), f64, e_ref)
    ok_torch = held(name + " torch path (GPU) vs golden", torch_out.detach().cpu().numpy(), f64, e_ref)
    ok_pair = held(name + " fused forward vs torch path", fused.cpu().numpy(), torch_out.detach().double().cpu().numpy(), e_ref, np.abs(f64).max())
    assert ok_gold and ok_pair, (ok_gold, ok_torch, ok_pair)


def test_whole_predictor_with_adjusted_planes(dev, gold, monkeypatch):
    from mpiflow_amd import ops
    from mpiflow_amd.model import MPIPredictor
    S, H, W, seed = (int(v) for v in gold["model/settings"])
    d = mg.model_inputs()
    m = MPIPredictor(W, H, S, adjust_planes=True)
    psum = mg.fill_params(m, seed)
    assert abs(sum(v.astype(np.float64).sum() for v in d.values()) + psum - float(gold["model/input_sum"])) < 1e-6
    m = m.eval().to(dev)
    img, dsp = torch.from_numpy(d["image"]).to(dev), torch.from_numpy(d["disp"]).to(dev)
    calls, seen = [], {}
    real, real_fmn = ops.pan_block1, m.fmn.forward
    monkeypatch.setattr(ops, "pan_block1", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(m.fmn, "forward", lambda *a: seen.setdefault("fmn", real_fmn(*a)))
    with torch.no_grad():
        mpi, planes = m(img, dsp)
    assert calls == [1] and mpi.shape == (1, S, 4, H, W) and planes.shape == (1, S) and bool(torch.isfinite(mpi).all())
    assert held("model planes", planes.cpu().numpy(), gold["model/planes_f64"], gold["model/planes_e_ref"])
    fmn = mg.kept(seen["fmn"].cpu().numpy(), seed)
    err = float(np.abs(fmn - gold["model/fmn_f32"]).max())
    print("model fmn on the adjusted planes: max abs %.3e (bar 2e-3)" % err)
    assert err < 2e-3                                                         # tests/test_model.py's bar for the model on the GPU against the CPU run


def test_engines_take_a_plane_set_per_call(dev, monkeypatch):
    from mpiflow_amd.model import MPIPredictor
    from mpiflow_amd.model.engine import HipPredictor
    from mpiflow_amd.model.precise import PrecisePredictor
    from test_conv_engine import ENGINE_BARS
    S, H, W, seed = 8, 128, 256, 5
    m = MPIPredictor(W, H, S).randomize_(seed).eval().to(dev)
    g = torch.Generator().manual_seed(2)
    img, dsp = torch.rand(1, 3, H, W, generator=g).to(dev), torch.rand(1, 1, H, W, generator=g).to(dev)
    fixed = m.plane_disparities(img)[0].contiguous()
    shifted = (fixed * 0.9 + 0.03).contiguous()
    hp = HipPredictor(m, graph=True)
    keep = lambda out: tuple(t.clone() for t in out)                          # noqa: E731 - the graph's outputs are static buffers
    base = keep(hp(img, dsp))
    assert torch.equal(base[2], fixed) and len(hp._graphs) == 1
    same = keep(hp(img, dsp, plane_disp=fixed))
    moved = keep(hp(img, dsp, plane_disp=shifted))
    back = keep(hp(img, dsp))
    assert len(hp._graphs) == 1                                               # no re-capture
    assert all(torch.equal(a, b) for a, b in zip(base, same)) and all(torch.equal(a, b) for a, b in zip(base, back))
    assert torch.equal(moved[2], shifted) and not torch.equal(moved[0], base[0])
    eager = HipPredictor(m, graph=False)(img, dsp, plane_disp=shifted)
    assert all(torch.equal(a, b) for a, b in zip(moved, eager))
    # the torch model on the shifted planes, within the engine's bars (tests/test_conv_engine.py)
    monkeypatch.setattr(m, "plane_disparities", lambda like: shifted.unsqueeze(0))
    with torch.no_grad():
        ref_raw, ref_cum, ref_disp = m(img, dsp, raw=True)
    monkeypatch.undo()
    assert torch.equal(ref_disp[0], shifted) and float((moved[1] - ref_cum[0]).abs().max()) < 2e-3
    act = lambda r, c: (torch.sigmoid(r[:, :3].float()), torch.relu(r[:, 3].float() * c.float()) + 1e-4)      # noqa: E731
    for name, got, ref in zip(("rgb", "sigma"), act(moved[0], moved[1]), act(ref_raw[0], ref_cum[0])):
        e = (got - ref).abs().flatten()
        e_mean, e_tail = float(e.mean()), float(e.kthvalue(int(e.numel() * 0.999)).values)
        print("engine on shifted planes, %s: mean %.2e tail %.2e (bars %s)" % (name, e_mean, e_tail, ENGINE_BARS[(S, H, W, seed)][name]))
        assert e_mean <= ENGINE_BARS[(S, H, W, seed)][name][0] and e_tail <= ENGINE_BARS[(S, H, W, seed)][name][1]
    pp = PrecisePredictor(m)
    p_base = keep(pp(img, dsp))
    p_same, p_moved, p_back = keep(pp(img, dsp, plane_disp=fixed)), keep(pp(img, dsp, plane_disp=shifted)), keep(pp(img, dsp))
    assert all(torch.equal(a, b) for a, b in zip(p_base, p_same)) and all(torch.equal(a, b) for a, b in zip(p_base, p_back))
    assert torch.equal(p_moved[2], shifted) and not torch.equal(p_moved[0], p_base[0])
    assert float((p_moved[1] - ref_cum[0]).abs().max()) < 2e-3                # its masks are the torch model's on the shifted planes, not on the fixed ones
    with pytest.raises(Exception, match=r"plane_disp must be \[S\]"):
        hp(img, dsp, plane_disp=shifted[:-1].contiguous())
    with pytest.raises(Exception, match="plane_disp must live on the GPU"):
        pp(img, dsp, plane_disp=shifted.cpu())


def test_loader_path_end_to_end_and_the_refusal(dev):
    """128 x 128, S = 5, a seeded model through producer.load_model and Lane - what the CLI's --adjust-planes and OnlinePairs(adjust_planes=True) run"""
    from mpiflow_amd import host_math, producer
    H = W = 128
    S = 5
    rs = np.random.RandomState(11)
    item = dict(name="img_0042", rgb_u8=torch.from_numpy(rs.randint(0, 256, (H, W, 3)).astype(np.uint8)),
                disp_u8=torch.from_numpy(rs.randint(1, 256, (H, W)).astype(np.uint8)), ids_u8=torch.from_numpy((rs.rand(H, W) < 0.3).astype(np.uint8)))
    model = producer.load_model("random:4", W, H, S, dev, adjust_planes=True)
    with torch.no_grad():
        model.dpn.to_disp.linear.weight.mul_(0.01)                            # a small adjustment: the planes move and stay positive
        model.dpn.to_disp.linear.bias.zero_()
    lane = producer.Lane(dev, H, W, S, model, "auto")
    assert lane.adjust_planes
    draws = producer.Schedule(1, 0.15, 1).draw(1)
    returned = []                                                             # what dpn returned: a second run of torch's convolutions may differ by an ulp
    real_dpn = model.dpn.forward
    model.dpn.forward = lambda *a: returned.append(real_dpn(*a)) or returned[-1]
    with torch.cuda.stream(lane.stream):
        front = lane.front(item)
        results = lane.pairs(front, *draws)
    lane.stream.synchronize()
    planes = front[3]
    assert len(returned) == 1 and returned[0].shape == (1, S)                 # once per image
    want = returned[0][0]
    fixed = model.plane_disparities(want)[0]
    assert not planes.is_cuda and planes.numpy().tobytes() == want.cpu().numpy().tobytes()        # the renderer's planes are the bytes dpn returned
    assert bool((planes > 0).all()) and 1e-6 < float((want - fixed).abs().max()) < 0.1
    assert torch.equal(lane.predictor._planes, want) and torch.equal(lane.renderer._const[1], host_math.plane_depths(planes))
    for k in ("flow_mix", "frame_mix"):
        assert bool(torch.isfinite(results[0][k].float()).all()), k
    # a bias that pushes every plane below zero: refused on the host values, naming the image and the plane, before anything renders
    with torch.no_grad():
        model.dpn.to_disp.linear.bias.fill_(-1.0 * S)
    blends = []
    real_blend = lane.renderer.blend
    lane.renderer.blend = lambda *a, **k: blends.append(1) or real_blend(*a, **k)
    with torch.cuda.stream(lane.stream):
        with pytest.raises(producer.PlaneRefused, match=r"image img_0042: plane 0 of 5 has disparity -0\.\d+ after plane adjustment"):
            lane.front(item)
    lane.stream.synchronize()
    assert blends == []
