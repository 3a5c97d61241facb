#!/usr/bin/env python3
"""Record the GEOMETRY gradients of the utils/mpi renderer by RUNNING THE REFERENCE ITSELF under autograd (utils/mpi/homography_sampler.py and
utils/mpi/mpi_rendering.py, torch on the CPU), once in float64 and once in float32 -> tests/golden/render_geom_grad.npz.

    python tests/golden/make_render_geom_grad_golden.py [--out PATH]   (needs the reference tree, numpy, torch)

The inputs are the draws of make_render_grad_golden.py (draw(), geometry(), POSES, B, H, W are imported from it).  Per gradient the file holds the
float64 gradient (g64/...) and e_ref = max|g32 - g64| / max|g64| of the reference's own float32 run (e_ref/...), per case the seed and the float64 sum
of the inputs.  Families:

    render/<case>              render(...), all six outputs weighted: d / d (xyz_BS3HW, src_xyz_BS3HW).  The hard case stores only what differs from
                               its base case (src_xyz_BS3HW).
    rtd/<case>/<which>         render_tgt_rgb_depth(...), `full` = rgb, depth, flowA2B and the rendered mask weighted, `noflow` = without flowA2B:
                               d / d (xyz_tgt_BS3HW, xyz_src_BS3HW, mpi_disparity_src), three leaves independent of each other
    e2e/<case>/<which>         ONE disparity leaf BxS through get_src_xyz_from_plane_disparity, get_tgt_xyz_from_plane_disparity and
                               render_tgt_rgb_depth; the gradient [3,B,S] for three draws of the upstream gradients (seed, seed+100, seed+200), e_ref
                               the largest of the three.  s5_dup: two adjacent planes at one disparity (a plane distance of exactly 0).
    helpers/s5                 get_src_xyz_from_plane_disparity with a random upstream gradient: d / d disparity
    sample_inverse/s5          HomographySample.sample_inverse with a random upstream gradient: d / d d_src_B

ZERO_BY_CONSTRUCTION names the gradients that are identically zero in the reference (and must be identically zero in the port); every other recorded
gradient has max|g64| > 0, asserted below together with the coverage that make_render_grad_golden.py asserts (invalid pixels, clamps at the four
borders, a plane with no valid pixel, a sampled z < 0)."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_render_grad_golden import B, H, POSES, W, draw, geometry, input_sum  # noqa: E402,F401

RENDER_CASES = [("s1_mask", 1, True, False, True, 9001), ("s5_mask", 5, True, False, True, 9002), ("s5_mask_hard", 5, True, True, True, 9002),
                ("s5_plain", 5, False, False, False, 9004)]          # name, S, with_mask, hard_flow, with_src, seed: make_render_grad_golden's
RTD_CASES = [("s1_mask", 1, 9011), ("s5_mask", 5, 9012)]
E2E_CASES = [("s5_mask", False, 9031), ("s5_dup", True, 9032)]       # name, duplicated plane, seed
E2E_DRAWS = (0, 100, 200)
HELPERS_SEED, SAMPLE_INVERSE_SEED = 9041, 9051
UPSTREAM = ("g_rgb", "g_depth", "g_flow2", "g_mask")
# without flowA2B in the loss nothing depends on xyz_src or on the disparity argument; hard_flow's one-hot selection is constant in the distances
ZERO_BY_CONSTRUCTION = ["render/s5_mask_hard/g64/src_xyz_BS3HW", "rtd/s1_mask/noflow/g64/xyz_src_BS3HW", "rtd/s1_mask/noflow/g64/mpi_disparity_src",
                        "rtd/s5_mask/noflow/g64/xyz_src_BS3HW", "rtd/s5_mask/noflow/g64/mpi_disparity_src",
                        # S = 1: the only plane distance is the constant 1e3
                        "render/s1_mask/g64/src_xyz_BS3HW", "rtd/s1_mask/full/g64/xyz_src_BS3HW"]


def e2e_disparity(dup):
    disp = geometry(5)[0].copy()
    if dup:
        disp[:, 2] = disp[:, 1]
    return disp


def helpers_upstream():
    return np.random.default_rng(HELPERS_SEED).standard_normal((B, 5, 3, H, W)).astype(np.float32)


def sample_inverse_upstream():
    return np.random.default_rng(SAMPLE_INVERSE_SEED).standard_normal((B * 5, H, W, 2)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "render_geom_grad.npz"))
    a = ap.parse_args()
    import torch
    import ref_harness
    ref_harness.install()
    from utils.mpi import mpi_rendering as R                     # the reference's own
    from utils.mpi.homography_sampler import HomographySample
    torch.manual_seed(0)
    rec = {"torch_version": np.array(torch.__version__), "zero_by_construction": np.array(ZERO_BY_CONSTRUCTION),
           "render_cases": np.array([c[0] for c in RENDER_CASES]), "rtd_cases": np.array([c[0] for c in RTD_CASES]),
           "e2e_cases": np.array([c[0] for c in E2E_CASES])}

    def T(x, dt, grad=False):
        return None if x is None else torch.from_numpy(np.asarray(x)).to(dt).requires_grad_(grad)

    def rep(m, S):
        return m.unsqueeze(1).repeat(1, S, 1, 1).reshape(B * S, m.shape[-2], m.shape[-1])

    def xyz(S, dt, disp=None, grad=False):
        disp0, G, K, Kinv = geometry(S)
        disp = T(disp0 if disp is None else disp, dt, grad)
        sampler = HomographySample(H, W)
        xs = R.get_src_xyz_from_plane_disparity(sampler.meshgrid.to(dt), disp, T(Kinv, dt))
        return sampler, xs, R.get_tgt_xyz_from_plane_disparity(xs, T(G, dt)), disp, T(G, dt), T(K, dt), T(Kinv, dt)

    def grads(loss, leaves):
        names = [k for k, v in leaves.items() if v is not None]
        gs = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
        return {k: (np.zeros(tuple(leaves[k].shape)) if g is None else g.detach().numpy()) for k, g in zip(names, gs)}

    def store(prefix, g64s, g32s, only=None):
        """g64s / g32s: name -> array, or name -> list of arrays (several draws: stacked, e_ref the largest)"""
        for k in g64s:
            many = isinstance(g64s[k], list)
            l64 = g64s[k] if many else [g64s[k]]
            l32 = [g.astype(np.float64) for g in (g32s[k] if many else [g32s[k]])]
            e_ref = 0.0
            for g64, g32 in zip(l64, l32):
                assert np.isfinite(g64).all() and np.isfinite(g32).all(), (prefix, k)
                scale = np.abs(g64).max()
                name = prefix + "g64/" + k
                assert (scale == 0) == (name in ZERO_BY_CONSTRUCTION), (name, scale)
                e_ref = max(e_ref, np.abs(g32 - g64).max() / scale if scale > 0 else 0.0)
            print("  %-24s %-18s max|g64| %.3e   e_ref %.3e%s" % (prefix, k, max(np.abs(g).max() for g in l64), e_ref,
                                                                "" if only is None or k in only else "   (not stored: equals the base case's)"))
            if only is None or k in only:
                rec[prefix + "g64/" + k] = np.stack(l64) if many else l64[0]
                rec[prefix + "e_ref/" + k] = np.float64(e_ref)

    # ---- render: d / d (xyz, src_xyz) ----------------------------------------------------------------------------------------------------
    for name, S, with_mask, hard, with_src, seed in RENDER_CASES:
        d = draw(seed, S, with_mask)
        per = {}
        for dt in (torch.float64, torch.float32):
            _, xs, xt, *_ = xyz(S, dt)
            leaves = dict(xyz_BS3HW=xt.detach().requires_grad_(True), src_xyz_BS3HW=xs.detach().requires_grad_(True) if with_src else None)
            out = R.render(T(d["rgb"], dt), T(d["sigma"], dt), leaves["xyz_BS3HW"], T(d["src_sigma"], dt) if with_src else None,
                           T(d["src_flow"], dt) if with_src else None, leaves["src_xyz_BS3HW"], hard_flow=hard, obj_mask=T(d["obj_mask"], dt))
            ups = [d["g_rgb"], d["g_depth"], d["g_tacc"], d["g_weights"], d["g_flow"], d["g_mask"]]
            loss = sum((o * T(u, dt)).sum() for o, u in zip(out, ups) if o is not None)
            per[dt] = grads(loss, leaves)
        p = "render/%s/" % name
        rec[p + "settings"] = np.array([S, int(with_mask), int(hard), int(with_src)], np.int64)
        rec[p + "seed"], rec[p + "input_sum"] = np.int64(seed), np.float64(input_sum(d))
        store(p, per[torch.float64], per[torch.float32], only=("src_xyz_BS3HW",) if hard else None)

    # ---- render_tgt_rgb_depth: three independent leaves -------------------------------------------------------------------------------------
    def rtd_loss(out, d, dt, which, ups=None):
        rgb, depth, tgt_mask, flow, om = out
        ups = d if ups is None else ups
        loss = (rgb * T(ups["g_rgb"], dt)).sum() + (depth * T(ups["g_depth"], dt)).sum() + (om * T(ups["g_mask"], dt)).sum()
        if which == "full":
            loss = loss + (flow * T(ups["g_flow2"], dt)).sum()
        return loss

    cover = {}
    for name, S, seed in RTD_CASES:
        d = draw(seed, S, True)
        for which in ("full", "noflow"):
            per = {}
            for dt in (torch.float64, torch.float32):
                sampler, xs, xt, disp, G, K, Kinv = xyz(S, dt)
                leaves = dict(xyz_tgt_BS3HW=xt.detach().requires_grad_(True), xyz_src_BS3HW=xs.detach().requires_grad_(True),
                              mpi_disparity_src=disp.detach().requires_grad_(True))
                out = R.render_tgt_rgb_depth(sampler, T(d["rgb"], dt), T(d["sigma"], dt), leaves["mpi_disparity_src"], leaves["xyz_tgt_BS3HW"],
                                             leaves["xyz_src_BS3HW"], G, Kinv, K, obj_mask=T(d["obj_mask"], dt))
                per[dt] = grads(rtd_loss(out, d, dt, which), leaves)
                if dt == torch.float32 and which == "full":
                    src = torch.cat((xt.reshape(B * S, 3, H, W)[:, 2:3],), dim=1)
                    z, valid, flow = sampler.sample(src, torch.reciprocal(disp).view(B * S), rep(G, S), rep(Kinv, S), rep(K, S))
                    u, v = (flow[..., 0] + sampler.meshgrid[0]).numpy(), (flow[..., 1] + sampler.meshgrid[1]).numpy()
                    cover[name] = dict(z_negative=int((z < 0).sum()), invalid=int((~valid).sum()), clamp_left=int((u < 0).sum()),
                                       clamp_right=int((u > W - 1).sum()), clamp_top=int((v < 0).sum()), clamp_bottom=int((v > H - 1).sum()),
                                       planes_all_invalid=int((valid.view(B * S, -1).sum(1) == 0).sum()))
            store("rtd/%s/%s/" % (name, which), per[torch.float64], per[torch.float32])
        p = "rtd/%s/" % name
        rec[p + "settings"] = np.array([S, 1, 0], np.int64)
        rec[p + "seed"], rec[p + "input_sum"] = np.int64(seed), np.float64(input_sum(d))

    # ---- end to end: one disparity leaf ---------------------------------------------------------------------------------------------------------
    for name, dup, seed in E2E_CASES:
        S = 5
        d = draw(seed, S, True)
        ups = [{k: draw(seed + off, S, True)[k] for k in UPSTREAM} for off in E2E_DRAWS]
        for which in ("full", "noflow"):
            per = {torch.float64: [], torch.float32: []}
            for dt in per:
                for up in ups:
                    sampler, xs, xt, disp, G, K, Kinv = xyz(S, dt, e2e_disparity(dup), grad=True)
                    out = R.render_tgt_rgb_depth(sampler, T(d["rgb"], dt), T(d["sigma"], dt), disp, xt, xs, G, Kinv, K, obj_mask=T(d["obj_mask"], dt))
                    (g,) = torch.autograd.grad(rtd_loss(out, d, dt, which, up), [disp])
                    assert torch.isfinite(g).all(), (name, which)          # s5_dup: a plane distance of exactly 0 must not poison the gradient
                    per[dt].append(g.numpy())
            store("e2e/%s/%s/" % (name, which), dict(disparity=per[torch.float64]), dict(disparity=per[torch.float32]))
        p = "e2e/%s/" % name
        rec[p + "seed"], rec[p + "disparity"] = np.int64(seed), e2e_disparity(dup)
        rec[p + "input_sum"] = np.float64(input_sum(d) + sum(input_sum(u) for u in ups))
        if dup:
            sampler, xs, *_ = xyz(S, torch.float32, e2e_disparity(dup))
            assert float((xs[:, 2] - xs[:, 1]).abs().max()) == 0.0

    # ---- the helpers and sample_inverse -----------------------------------------------------------------------------------------------------
    per = {}
    for dt in (torch.float64, torch.float32):
        sampler, xs, xt, disp, G, K, Kinv = xyz(5, dt, grad=True)
        per[dt] = grads((xs * T(helpers_upstream(), dt)).sum(), dict(disparity=disp))
    rec["helpers/s5/seed"], rec["helpers/s5/input_sum"] = np.int64(HELPERS_SEED), np.float64(helpers_upstream().astype(np.float64).sum())
    store("helpers/s5/", per[torch.float64], per[torch.float32])
    per = {}
    for dt in (torch.float64, torch.float32):
        sampler, xs, xt, disp, G, K, Kinv = xyz(5, dt)
        leaf = torch.reciprocal(disp).view(B * 5).detach().requires_grad_(True)
        flow = sampler.sample_inverse(xs.reshape(B * 5, 3, H, W), leaf, rep(G, 5), rep(Kinv, 5), rep(K, 5))
        per[dt] = grads((flow * T(sample_inverse_upstream(), dt)).sum(), dict(d_src_B=leaf))
    rec["sample_inverse/s5/seed"] = np.int64(SAMPLE_INVERSE_SEED)
    rec["sample_inverse/s5/input_sum"] = np.float64(sample_inverse_upstream().astype(np.float64).sum())
    store("sample_inverse/s5/", per[torch.float64], per[torch.float32])

    # ---- coverage, as make_render_grad_golden.py asserts it -----------------------------------------------------------------------------------
    print("coverage:", cover)
    c5 = cover["s5_mask"]
    assert c5["invalid"] > 0 and min(c5["clamp_left"], c5["clamp_right"], c5["clamp_top"], c5["clamp_bottom"]) > 0, c5
    assert c5["planes_all_invalid"] >= 1 and c5["z_negative"] > 0, c5
    assert cover["s1_mask"]["invalid"] > 0, cover
    for k, v in cover.items():
        for kk, vv in v.items():
            rec["coverage/%s/%s" % (k, kk)] = np.int64(vv)
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 1000 * 1000
    return 0


if __name__ == "__main__":
    sys.exit(main())
