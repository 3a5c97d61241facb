#!/usr/bin/env python3
"""Record the gradients of the utils/mpi renderer by RUNNING THE REFERENCE ITSELF under autograd (utils/mpi/homography_sampler.py and
utils/mpi/mpi_rendering.py, torch on the CPU), once in float64 and once in float32 -> tests/golden/render_grad.npz.

    python tests/golden/make_render_grad_golden.py [--out PATH]   (needs the reference tree, numpy, torch)

Three families, every input and every upstream gradient a draw of np.random.default_rng(seed):

    sample/<case>   HomographySample.sample(src): d(sum(tgt * g_tgt)) / d src
    render/<case>   render(...): all six returned tensors weighted by their upstream gradients; d / d (rgb, sigma, src_sigma, src_flow, obj_mask)
    rtd/<case>      render_tgt_rgb_depth(...): `full` = rgb, depth, flowA2B and the rendered mask weighted; `noflow` = the same without flowA2B (what the
                    fused form connects); d / d (mpi_rgb_src, mpi_sigma_src, obj_mask)

A committed file may hold 1 MiB at most, and random float64 gradients do not compress, so per case the file holds: the seed and the float64 sum of
the inputs and upstream gradients (the test rebuilds them with draw() / geometry() below and checks the sum, as the warm-start golden does), the
float64 B x C x H x W outputs, the float64 input gradients (g64/...), and for each of them e_ref = max|g32 - g64| / max|g64| of the reference's own
float32 run (e_ref/...) - the number the tests' tolerance is computed from - instead of the float32 gradients themselves.  The hard_flow cases share
their base case's seed and store only the gradients that hard_flow changes.  Nothing is excluded anywhere: every gradient is with respect to values the outputs are smooth in.  (render's hard_flow output is
piecewise constant in sigma; torch's gradient of it with respect to sigma is identically zero and is recorded as such.)

Shapes: B = 2, S in {1, 5}, H x W = 13 x 21.  The poses (POSES) are chosen so that, over a case's planes, some target pixels are invalid, taps are clamped
at each of the four borders, one plane of the S = 5 stack has NO valid target pixel, and at least one plane-pixel has a sampled z < 0; main() asserts
all of it and stores the counts (coverage/...).  The 8 x 64 x 96 case of the memory check compares no values, so the file holds its settings only
(memory/...): the test draws its inputs from the seed.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
B, H, W = 2, 13, 21
MEMORY_CASE = dict(B=1, S=8, H=64, W=96, seed=9100)

# per batch item: rotation vector (rad), translation
POSES = [((0.010, 0.035, -0.008), (-0.060, 0.045, 0.030)),
         ((-0.020, -0.030, 0.012), (0.160, -0.120, -0.700))]


def disparities(S):
    """BxS, near to far; S = 5: item 1's nearest plane is so near that no target pixel sees it"""
    if S == 1:
        return np.array([[2.2], [3.0]], np.float32)
    return np.array([np.linspace(1.6, 0.25, S), np.concatenate(([40.0], np.linspace(1.8, 0.2, S - 1)))], np.float32)


def intrinsics(h, w):
    f = 0.9 * w
    return np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1]], np.float32)


def pose(rvec, t):
    rx, ry, rz = rvec
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    G = np.eye(4)
    G[:3, :3] = Rz @ Ry @ Rx
    G[:3, 3] = t
    return G.astype(np.float32)


def geometry(S, h=H, w=W, b=B):
    """float32 (disparity BxS, G Bx4x4, K Bx3x3, K_inv Bx3x3)"""
    K = intrinsics(h, w)
    Kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    G = np.stack([pose(*POSES[i % len(POSES)]) for i in range(b)])
    return disparities(S)[:b], G, np.stack([K] * b), np.stack([Kinv] * b)


def draw(seed, S, with_mask, h=H, w=W, b=B):
    """the value inputs and the upstream gradients of one case, float32"""
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.random(shape, dtype=np.float64).astype(np.float32)
    g = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    # the last plane's distance is 1e3: with S = 1 a density of order 1 would leave t = exp(-1e3 sigma) = 0 and nothing to differentiate
    ss = np.float32(2.5 if S > 1 else 0.004)
    d = dict(rgb=f(b, S, 3, h, w), sigma=ss * f(b, S, 1, h, w), src_sigma=ss * f(b, S, 1, h, w), src_flow=3.0 * g(b, S, 2, h, w),
             g_rgb=g(b, 3, h, w), g_depth=g(b, 1, h, w), g_tacc=g(b, S, 1, h, w), g_weights=g(b, S, 1, h, w), g_flow=g(b, 2, h, w),
             g_mask=g(b, 1, h, w), g_flow2=g(b, 2, h, w), g_tgt=g(b * S, 4, h, w))
    mask = np.repeat((f(b, 1, 1, h, w) > 0.5).astype(np.float32) * 0.75 + 0.125, S, axis=1)      # one mask on every plane
    d["obj_mask"] = mask if with_mask else None
    return d


def input_sum(d):
    """float64 sum over every array of a draw: the file carries it, the test checks its rebuilt inputs against it"""
    return float(sum(np.asarray(v, np.float64).sum() for v in d.values() if v is not None))


RENDER_CASES = [("s1_mask", 1, True, False, True, 9001), ("s5_mask", 5, True, False, True, 9002), ("s5_mask_hard", 5, True, True, True, 9002),
                ("s5_plain", 5, False, False, False, 9004)]          # name, S, with_mask, hard_flow, with_src, seed
# name, S, with_mask, hard_flow, seed.  The reference's render_tgt_rgb_depth cannot run with obj_mask=None (mpi_rendering.py:95 multiplies by it): the
# mask-less call is covered by the gradient set `noflow_nomask` - the masked call with the rendered mask left out of the loss, which is what the
# mask-less call computes for mpi_rgb_src and mpi_sigma_src - and by render's s5_plain case.
RTD_CASES = [("s1_mask", 1, True, False, 9011), ("s5_mask", 5, True, False, 9012), ("s5_mask_hard", 5, True, True, 9012)]
SAMPLE_CASES = [("s1", 1, 9021), ("s5", 5, 9022)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "render_grad.npz"))
    a = ap.parse_args()
    import torch
    sys.path.insert(0, HERE)
    import ref_harness
    ref_harness.install()
    from utils.mpi import mpi_rendering as R                     # the reference's own
    from utils.mpi.homography_sampler import HomographySample
    torch.manual_seed(0)
    rec = {"torch_version": np.array(torch.__version__), "poses": np.array(POSES, np.float64),
           "render_cases": np.array([c[0] for c in RENDER_CASES]), "rtd_cases": np.array([c[0] for c in RTD_CASES]),
           "sample_cases": np.array([c[0] for c in SAMPLE_CASES])}
    for k, v in MEMORY_CASE.items():
        rec["memory/" + k] = np.int64(v)

    def T(x, dt, grad=False):
        return None if x is None else torch.from_numpy(np.asarray(x)).to(dt).requires_grad_(grad)

    def xyz(S, dt):
        disp, G, K, Kinv = geometry(S)
        sampler = HomographySample(H, W)
        xs = R.get_src_xyz_from_plane_disparity(sampler.meshgrid.to(dt), T(disp, dt), T(Kinv, dt))
        return sampler, xs, R.get_tgt_xyz_from_plane_disparity(xs, T(G, dt)), T(disp, dt), T(G, dt), T(K, dt), T(Kinv, dt)

    def grads(loss, leaves):
        names = [k for k, v in leaves.items() if v is not None]
        gs = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
        return {k: (np.zeros(tuple(leaves[k].shape)) if g is None else g.detach().numpy()) for k, g in zip(names, gs)}

    def store(prefix, per_dtype, only=None):
        for k, v in per_dtype[torch.float64][0].items():
            if v.ndim <= 4 and v.shape[0] == B:             # the B x C x H x W outputs; S-deep ones are not needed by any check
                rec[prefix + "out/" + k] = v
        for k in per_dtype[torch.float64][1]:
            g64, g32 = per_dtype[torch.float64][1][k], per_dtype[torch.float32][1][k].astype(np.float64)
            assert np.isfinite(g64).all() and np.isfinite(g32).all(), (prefix, k)
            scale = np.abs(g64).max()
            e_ref = np.abs(g32 - g64).max() / scale if scale > 0 else 0.0
            print("  %-28s %-14s max|g64| %.3e   e_ref %.3e%s" % (prefix, k, scale, e_ref, "" if only is None or k in only else "   (not stored: equals the base case's)"))
            if only is None or k in only:
                rec[prefix + "g64/" + k] = g64
                rec[prefix + "e_ref/" + k] = np.float64(e_ref)

    cover = {}
    # ---- HomographySample.sample -------------------------------------------------------------------------------------------------------
    for name, S, seed in SAMPLE_CASES:
        d = draw(seed, S, False)
        src = np.concatenate([d["rgb"], d["sigma"]], axis=2).reshape(B * S, 4, H, W)
        per = {}
        for dt in (torch.float64, torch.float32):
            sampler, _, _, disp, G, K, Kinv = xyz(S, dt)
            rep = lambda m: m.unsqueeze(1).repeat(1, S, 1, 1).reshape(B * S, m.shape[-2], m.shape[-1])
            leaf = T(src, dt, True)
            tgt, valid, flow = sampler.sample(leaf, torch.reciprocal(disp).view(B * S), rep(G), rep(Kinv), rep(K))
            per[dt] = (dict(tgt=tgt.detach().numpy(), valid=valid.numpy(), flowB2A=flow.detach().numpy()),
                       grads((tgt * T(d["g_tgt"], dt)).sum(), dict(src=leaf)))
            if dt == torch.float32:
                u, v = (flow[..., 0] + sampler.meshgrid[0]).detach().numpy(), (flow[..., 1] + sampler.meshgrid[1]).detach().numpy()
                cover[name] = dict(invalid=int((~valid).sum()), clamp_left=int((u < 0).sum()), clamp_right=int((u > W - 1).sum()),
                                   clamp_top=int((v < 0).sum()), clamp_bottom=int((v > H - 1).sum()),
                                   planes_all_invalid=int((valid.view(B * S, -1).sum(1) == 0).sum()))
        p = "sample/%s/" % name
        rec[p + "seed"], rec[p + "input_sum"] = np.int64(seed), np.float64(src.astype(np.float64).sum() + d["g_tgt"].astype(np.float64).sum())
        store(p, per)

    # ---- render ---------------------------------------------------------------------------------------------------------------------------
    for name, S, with_mask, hard, with_src, seed in RENDER_CASES:
        d = draw(seed, S, with_mask)
        per = {}
        for dt in (torch.float64, torch.float32):
            _, xs, xt, *_ = xyz(S, dt)
            leaves = dict(rgb=T(d["rgb"], dt, True), sigma=T(d["sigma"], dt, True), src_sigma=T(d["src_sigma"], dt, True) if with_src else None,
                          src_flow=T(d["src_flow"], dt, True) if with_src else None, obj_mask=T(d["obj_mask"], dt, True) if with_mask else None)
            out = R.render(leaves["rgb"], leaves["sigma"], xt, leaves["src_sigma"], leaves["src_flow"], xs if with_src else None, hard_flow=hard,
                           obj_mask=leaves["obj_mask"])
            ups = [d["g_rgb"], d["g_depth"], d["g_tacc"], d["g_weights"], d["g_flow"], d["g_mask"]]
            names = ["rgb", "depth", "tacc", "weights", "flowA2B", "obj_mask"]
            loss = sum((o * T(u, dt)).sum() for o, u in zip(out, ups) if o is not None)
            per[dt] = ({k: o.detach().numpy() for k, o in zip(names, out) if o is not None}, grads(loss, leaves))
        p = "render/%s/" % name
        rec[p + "settings"] = np.array([S, int(with_mask), int(hard), int(with_src)], np.int64)
        rec[p + "seed"], rec[p + "input_sum"] = np.int64(seed), np.float64(input_sum(d))
        store(p, per, only=("src_sigma", "src_flow") if hard else None)

    # ---- render_tgt_rgb_depth -------------------------------------------------------------------------------------------------------------
    for name, S, with_mask, hard, seed in RTD_CASES:
        d = draw(seed, S, with_mask)
        for which in (("full",) if hard else ("full", "noflow", "noflow_nomask")):
            per = {}
            for dt in (torch.float64, torch.float32):
                sampler, xs, xt, disp, G, K, Kinv = xyz(S, dt)
                leaves = dict(mpi_rgb_src=T(d["rgb"], dt, True), mpi_sigma_src=T(d["sigma"], dt, True),
                              obj_mask=T(d["obj_mask"], dt, True) if with_mask else None)
                out = R.render_tgt_rgb_depth(sampler, leaves["mpi_rgb_src"], leaves["mpi_sigma_src"], disp, xt, xs, G, Kinv, K, hard_flow=hard,
                                             obj_mask=leaves["obj_mask"])
                rgb, depth, tgt_mask, flow, om = out
                loss = (rgb * T(d["g_rgb"], dt)).sum() + (depth * T(d["g_depth"], dt)).sum()
                if which == "full":
                    loss = loss + (flow * T(d["g_flow2"], dt)).sum()
                if om is not None and which != "noflow_nomask":
                    loss = loss + (om * T(d["g_mask"], dt)).sum()
                outs = dict(rgb=rgb, depth=depth, tgt_mask=tgt_mask, flowA2B=flow)
                if om is not None:
                    outs["obj_mask"] = om
                per[dt] = ({k: o.detach().numpy() for k, o in outs.items()}, grads(loss, leaves))
                if dt == torch.float32 and which == "full":
                    rep = lambda m: m.unsqueeze(1).repeat(1, S, 1, 1).reshape(B * S, m.shape[-2], m.shape[-1])
                    z, valid, _ = sampler.sample(xt.reshape(B * S, 3, H, W)[:, 2:3], torch.reciprocal(disp).view(B * S), rep(G), rep(Kinv), rep(K))
                    cover["rtd_" + name] = dict(z_negative=int((z < 0).sum()), invalid=int((~valid).sum()))
            store("rtd/%s/%s/" % (name, which), per,
                  only=("mpi_sigma_src",) if hard else None if which == "full" else ("mpi_sigma_src", "obj_mask") if which == "noflow" else ("mpi_sigma_src",))
        p = "rtd/%s/" % name
        rec[p + "settings"] = np.array([S, int(with_mask), int(hard)], np.int64)
        rec[p + "seed"], rec[p + "input_sum"] = np.int64(seed), np.float64(input_sum(d))
    for S in (1, 5):
        disp, G, K, Kinv = geometry(S)
        rec["geometry/s%d/disparity" % S], rec["geometry/s%d/G" % S], rec["geometry/s%d/K" % S], rec["geometry/s%d/K_inv" % S] = disp, G, K, Kinv

    # ---- coverage the issue asks for ----------------------------------------------------------------------------------------------------
    c5 = cover["s5"]
    print("coverage:", cover)
    assert c5["invalid"] > 0 and min(c5["clamp_left"], c5["clamp_right"], c5["clamp_top"], c5["clamp_bottom"]) > 0, c5
    assert c5["planes_all_invalid"] >= 1, c5
    assert cover["rtd_s5_mask"]["z_negative"] > 0, cover
    assert cover["s1"]["invalid"] > 0, cover
    for k, v in cover.items():
        for kk, vv in v.items():
            rec["coverage/%s/%s" % (k, kk)] = np.int64(vv)
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 1000 * 1000
    return 0


if __name__ == "__main__":
    sys.exit(main())
