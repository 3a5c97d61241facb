#!/usr/bin/env python3
"""Record MINE's plane samplers and disparity-consistency loss by RUNNING THE REFERENCE ITSELF (utils/mpi/rendering_utils.py:26-139 and
utils/mpi/mpi_rendering.py:180-210, torch on the CPU) -> tests/golden/mpi_training.npz.

    python tests/golden/make_mpi_training_golden.py [--out PATH]   (needs the reference tree, numpy, torch)

Per case the file holds the inputs, the reference's float32 outputs and gradients (ref32/...), float64 values (f64/...) and
e_ref = max|ref32 - f64| / max|f64| (e_ref/...), plus coverage counts (cov/...).

The reference's loss cannot run in float64 as written (gather_pixel_by_pxpy binds pxpy_int for float32 coordinates only), so the float64 values come
from tests/mpi_training_restated.py; this script cross-checks that restatement (1e-9 relative) against the reference's float64 autograd with the
coordinates cast to float32 at the gather's boundary only.  For sample_pdf, torch.rand returns the recorded u while the reference runs; the float64
run uses the same float32 u.

Conditions on the inputs, asserted here (they keep a discrete flip from hiding or faking a failure; nothing is excluded from any comparison):
  loss        in float64 no pixel has px or py within 1e-3 of a half-integer or of the mask bounds 0, W - 1, H - 1, and no |p.z| < 1e-3: the source
              disparity is redrawn at offending pixels until none is left (cov/.../near_boundary = 0)
  sample_pdf  in float64 no draw has u within 1e-5 of a cdf entry (an entry that is exactly 0 against u == 0 apart: it is 0 in every precision), and
              no selected cdf interval within 1e-6 of the 1e-4 switch: such u are redrawn
  self-check  the reference's own float32 run gives the indices and masks of float64 on every case"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import mpi_training_restated as rs  # noqa: E402

LOSS_CASES = ["b1_5x7", "b2_24x40", "b3_33x65", "mostly_out", "collide", "behind", "empty"]
PDF_CASES = ["b2_n50_s8", "s1", "n3_s128", "n130_s70"]
GATHER_CASES = [("c1", 1, "f32"), ("c3", 3, "f32"), ("c5", 5, "i64")]
COV = ("count", "near_boundary", "out_left", "out_right", "out_top", "out_bottom", "max_collisions", "behind_in_mask")


def intrinsics(f, H, W):
    return np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1]], dtype=np.float64)


def pose(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = Rz @ Ry @ Rx, t
    return G


def loss_inputs(name):
    """-> K_src_inv [B,3,3], G [B,4,4], K_tgt [B,3,3], d_src, d_tgt [B,1,H,W], all float32, d_src redrawn until no pixel is near a discrete boundary"""
    rng = np.random.default_rng(7100 + LOSS_CASES.index(name))
    shape = {"b1_5x7": (1, 5, 7), "b2_24x40": (2, 24, 40), "b3_33x65": (3, 33, 65)}.get(name, (1, 12, 20))
    B, H, W = shape
    Ks, Gs, Kt = [], [], []
    for b in range(B):
        f = W * (0.9 + 0.15 * b)
        K = intrinsics(f, H, W)
        G = pose(0.02 + 0.01 * b, -0.03 + 0.02 * b, 0.01 * (b + 1), (0.06 - 0.05 * b, -0.04 + 0.03 * b, 0.03 * b))
        Ktb = intrinsics(f * (1.0 + 0.05 * b), H, W)
        if name == "mostly_out":
            Ktb = intrinsics(3.0 * f, H, W)                          # a zoom in: the frame's rim leaves on all four sides
        elif name == "collide":
            Ktb = intrinsics(0.3 * f, H, W)                          # a zoom out: many source pixels per target pixel
        elif name == "behind":
            G = pose(0.01, 0.02, 0.0, (0.02, 0.01, -2.0))            # depth in 1..5 and t_z = -2: some points end behind the target camera
        elif name == "empty":
            G = pose(0.0, 0.0, 0.0, (100.0, 37.0, 0.0))              # every projection leaves the frame
        Ks.append(np.linalg.inv(K)); Gs.append(G); Kt.append(Ktb)
    Ki, G, Kt = (np.stack(a).astype(np.float32) for a in (Ks, Gs, Kt))
    d_src = rng.uniform(0.2, 1.0, (B, 1, H, W)).astype(np.float32)
    d_tgt = rng.uniform(0.2, 1.0, (B, 1, H, W)).astype(np.float32)
    for _ in range(1000):
        r = rs.disparity_consistency(Ki, d_src, G, Kt, d_tgt)
        bad = rs.near_boundary(r["px"], r["py"], r["pz"], H, W).reshape(B, 1, H, W)
        if not bad.any():
            break
        d_src[bad] = rng.uniform(0.2, 1.0, int(bad.sum())).astype(np.float32)
    else:
        raise AssertionError("%s: pixels near a discrete boundary remain" % name)
    return Ki, G, Kt, d_src, d_tgt


def loss_coverage(r, H, W):
    m, px, py = r["mask"], r["px"], r["py"]
    hits = np.concatenate([np.bincount(r["idx"][b][m[b]], minlength=H * W) for b in range(m.shape[0])])
    return np.array([r["count"], int(rs.near_boundary(px, py, r["pz"], H, W).sum()), int((px < 0).sum()), int((px > W - 1).sum()), int((py < 0).sum()),
                     int((py > H - 1).sum()), int(hits.max()), int((m & (r["pz"] < 0)).sum())], dtype=np.int64)


def pdf_inputs(name):
    """-> values (contiguous [B,1,N,S], or [B,1,1,S] to be expanded over N), weights [B,1,N,S], u [B,1,N,NS], float32"""
    rng = np.random.default_rng(7200 + PDF_CASES.index(name))
    B, N, S, NS, expanded = {"b2_n50_s8": (2, 50, 8, 6, False), "s1": (1, 20, 1, 4, False), "n3_s128": (1, 3, 128, 128, False),
                             "n130_s70": (2, 130, 70, 5, True)}[name]
    rows = 1 if expanded else N
    values = -np.sort(-rng.uniform(0.05, 1.0, (B, 1, rows, S)), axis=3).astype(np.float32)           # disparities, from large to small
    weights = rng.uniform(0.0, 1.0, (B, 1, N, S)).astype(np.float32)
    weights[:, :, 0, :] = 0.0                                                                       # a row of zero weights
    weights[:, :, 1, :] = 0.0
    weights[:, :, 1, S // 2] = 1e-3                                                                 # a one-hot row
    u = rng.uniform(0.0, 1.0, (B, 1, N, NS)).astype(np.float32)
    top = np.nextafter(np.float32(1.0), np.float32(0.0))
    for row in (0, 1):                                              # a full row's last cdf entry is within 1e-5 of the top draw
        u[:, :, row, 0] = 0.0
        u[:, :, row, 1 % NS if NS > 1 else 0] = top
    if NS == 1:
        u[:, :, 0, 0] = 0.0
    fixed = np.zeros(u.shape, dtype=bool)
    fixed[:, :, 0:2, 0:2] = True
    v_full = np.broadcast_to(values, (B, 1, N, S))
    for _ in range(1000):
        r = rs.sample_pdf(v_full, weights, u)
        bad = rs.pdf_near_flip(r["cdf"], u, r["cdf_interval"])
        assert not (bad & fixed).any(), "%s: a fixed draw sits near a flip" % name
        if not bad.any():
            break
        u[bad] = rng.uniform(0.0, 1.0, int(bad.sum())).astype(np.float32)
    else:
        raise AssertionError("%s: draws near a flip remain" % name)
    return values, weights, u, expanded


def gather_inputs(name, C, kind):
    rng = np.random.default_rng(7300 + C)
    B, H, W, N = 2, 6, 9, 300
    img = rng.standard_normal((B, C, H, W)).astype(np.float32)
    pxpy = np.stack((rng.uniform(-3.0, W + 2.0, (B, N)), rng.uniform(-3.0, H + 2.0, (B, N))), axis=1).astype(np.float32)
    pxpy[:, 0, 0:6] = [0.5, 1.5, 2.5, -0.5, W - 1.5, W - 0.5]                                       # exact ties, negatives, beyond range
    pxpy[:, 1, 0:6] = [0.5, 1.5, 2.5, -0.5, H - 1.5, H - 0.5]
    pxpy[:, :, 6] = [-40.0, 1e9]
    if kind == "i64":
        pxpy = np.round(pxpy).clip(-50, 50).astype(np.int64)
    g_out = rng.integers(-8, 9, (B, C, N)).astype(np.float32)                                       # small integers: every order of addition gives one float
    return img, pxpy, g_out


def rel(a, b):
    s = np.abs(b).max()
    return 0.0 if s == 0.0 or not np.isfinite(s) else float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "mpi_training.npz"))
    a = ap.parse_args()
    import torch
    import ref_harness
    ref_harness.install()
    from utils.mpi import mpi_rendering as R                     # the reference's own
    from utils.mpi import rendering_utils as U
    from utils.mpi.homography_sampler import HomographySample
    out = {}

    def ref_loss(dtype, Ki, G, Kt, d_src, d_tgt):
        H, W = d_src.shape[2:]
        mesh = HomographySample(H, W).meshgrid.to(dtype)
        ds, dt = (torch.from_numpy(x).to(dtype).requires_grad_(True) for x in (d_src, d_tgt))
        m = [torch.from_numpy(x).to(dtype) for x in (Ki, G, Kt)]
        loss = R.disparity_consistency_src_to_tgt(mesh, m[0], ds, m[1], m[2], dt)
        loss.backward()
        # the discrete choices of this run, from the reference's own functions
        xyz = R.get_xyz_from_depth(mesh, torch.reciprocal(ds.detach()), m[0]).view(ds.shape[0], 3, H * W)
        q = torch.matmul(m[2], U.transform_G_xyz(m[1], xyz))
        pxpy = (q[:, 0:2] / q[:, 2:]).to(torch.float32)
        mask = (pxpy[:, 0] >= 0) & (pxpy[:, 0] <= W - 1) & (pxpy[:, 1] >= 0) & (pxpy[:, 1] <= H - 1)
        idx = U.gather_pixel_by_pxpy(torch.arange(H * W, dtype=torch.float32).view(1, 1, H, W).repeat(ds.shape[0], 1, 1, 1), pxpy)[:, 0].to(torch.int64)
        return loss.detach().numpy(), ds.grad.numpy(), dt.grad.numpy(), mask.numpy(), idx.numpy()

    gather_orig = R.gather_pixel_by_pxpy
    for name in LOSS_CASES:
        Ki, G, Kt, d_src, d_tgt = loss_inputs(name)
        B, _, H, W = d_src.shape
        l32, gs32, gt32, mask32, idx32 = ref_loss(torch.float32, Ki, G, Kt, d_src, d_tgt)
        R.gather_pixel_by_pxpy = lambda img, pxpy: gather_orig(img, pxpy.to(torch.float32))      # float32 at the gather's boundary only
        try:
            l64, gs64, gt64, mask64, idx64 = ref_loss(torch.float64, Ki, G, Kt, d_src, d_tgt)
        finally:
            R.gather_pixel_by_pxpy = gather_orig
        r = rs.disparity_consistency(Ki, d_src, G, Kt, d_tgt)
        assert (mask32 == mask64).all() and (idx32 == idx64).all(), "%s: the reference's float32 run takes other pixels than float64" % name
        assert (r["mask"] == mask64).all() and (r["idx"] == idx64).all(), name
        cov = loss_coverage(r, H, W)
        if name == "empty":
            assert cov[0] == 0 and np.isnan(l32) and np.isnan(l64) and np.isnan(r["loss"]) and not gs64.any() and not gt64.any() and not gs32.any() \
                and not gt32.any() and not r["grad_src"].any() and not r["grad_tgt"].any()
        else:
            assert cov[0] > 0
            for mine, ref in ((r["loss"], l64), (r["grad_src"], gs64), (r["grad_tgt"], gt64)):
                assert rel(mine, ref) <= 1e-9, (name, rel(mine, ref))
        assert cov[1] == 0, name
        if name == "mostly_out":
            assert cov[2] > 0 and cov[3] > 0 and cov[4] > 0 and cov[5] > 0, cov
        if name == "collide":
            assert cov[6] >= 4, cov
        if name == "behind":
            assert cov[7] > 0, cov
        if name == "b3_33x65":
            assert B * ((H * W + 255) // 256) > 20
        k = "loss/%s/" % name
        out.update({k + "K_src_inv": Ki, k + "G_tgt_src": G, k + "K_tgt": Kt, k + "disparity_src": d_src, k + "disparity_tgt": d_tgt, k + "cov": cov,
                    k + "ref32/loss": np.float32(l32), k + "ref32/grad_src": gs32, k + "ref32/grad_tgt": gt32,
                    k + "f64/loss": np.float64(r["loss"]), k + "f64/grad_src": r["grad_src"], k + "f64/grad_tgt": r["grad_tgt"],
                    k + "e_ref/loss": np.float64(rel(l32, np.float64(r["loss"]))), k + "e_ref/grad_src": np.float64(rel(gs32, r["grad_src"])),
                    k + "e_ref/grad_tgt": np.float64(rel(gt32, r["grad_tgt"]))})
        print("%-12s count %5d of %5d  loss %.6f  e_ref %.2e %.2e %.2e  cov %s" % (name, cov[0], B * H * W, r["loss"], out[k + "e_ref/loss"],
                                                                                 out[k + "e_ref/grad_src"], out[k + "e_ref/grad_tgt"], cov.tolist()))

    real_rand = torch.rand
    for name in PDF_CASES:
        values, weights, u, expanded = pdf_inputs(name)
        B, _, N, S = weights.shape
        NS = u.shape[3]
        v_full = np.ascontiguousarray(np.broadcast_to(values, (B, 1, N, S)))
        res = {}
        for dtype in (torch.float32, torch.float64):
            def fake_rand(size, dtype=None, device=None, _u=u):
                assert tuple(size) == _u.shape
                return torch.from_numpy(_u).to(dtype)
            torch.rand = fake_rand
            try:
                res[dtype] = U.sample_pdf(torch.from_numpy(v_full).to(dtype), torch.from_numpy(weights).to(dtype), NS).numpy()
            finally:
                torch.rand = real_rand
        r = rs.sample_pdf(v_full, weights, u)
        assert rel(r["samples"], res[torch.float64]) <= 1e-9, name
        # the reference's float32 run picks the float64 bins: its cdf, rebuilt with its own operations
        w32 = torch.from_numpy(weights)
        cdf32 = torch.cumsum(w32 / (torch.sum(w32, dim=3, keepdim=True) + 1e-5), dim=3)
        cdf32 = torch.cat((torch.zeros((B, 1, N, 1)), cdf32), dim=3)
        idx32 = torch.searchsorted(cdf32, torch.from_numpy(u), right=True).numpy()
        assert (idx32 == r["idx"]).all(), "%s: the reference's float32 run takes other bins than float64" % name
        ci32 = (torch.gather(cdf32, 3, torch.from_numpy(np.minimum(idx32, S))) - torch.gather(cdf32, 3, torch.from_numpy(np.maximum(idx32 - 1, 0)))).numpy()
        assert ((ci32 <= np.float32(1e-4)) == (r["cdf_interval"] <= 1e-4)).all(), name
        cov = np.array([int(rs.pdf_near_flip(r["cdf"], u, r["cdf_interval"]).sum()), int((weights.sum(axis=3) == 0).sum()),
                        int(((weights != 0).sum(axis=3) == 1).sum()), int((u == 0).sum()), int((u == np.nextafter(np.float32(1), np.float32(0))).sum()),
                        int((r["cdf_interval"] <= 1e-4).sum()), int(expanded)], dtype=np.int64)
        assert cov[0] == 0 and cov[1] > 0 and cov[2] > 0 and cov[3] > 0 and cov[4] > 0
        k = "pdf/%s/" % name
        out.update({k + "values": values, k + "weights": weights, k + "u": u, k + "cov": cov, k + "ref32": res[torch.float32], k + "f64": r["samples"],
                    k + "e_ref": np.float64(rel(res[torch.float32], r["samples"]))})
        print("%-12s B %d N %3d S %3d NS %3d  e_ref %.2e  cov %s" % (name, B, N, S, NS, out[k + "e_ref"], cov.tolist()))

    for name, C, kind in GATHER_CASES:
        img, pxpy, g_out = gather_inputs(name, C, kind)
        ti = torch.from_numpy(img).requires_grad_(True)
        # the reference binds pxpy_int for float32 alone (:35-37): integer coordinates go through it as the same numbers in float32, which holds them exactly
        o = U.gather_pixel_by_pxpy(ti, torch.from_numpy(pxpy.astype(np.float32)))
        o.backward(torch.from_numpy(g_out))
        B, _, H, W = img.shape
        assert (o.detach().numpy() == rs.gather_pixel_by_pxpy(img, pxpy)).all() and (ti.grad.numpy() == rs.gather_pixel_by_pxpy_backward(g_out, pxpy, H, W)).all()
        hits = np.bincount(rs.flat_index(pxpy, H, W).reshape(-1), minlength=H * W)
        assert hits.max() >= 4
        k = "gather/%s/" % name
        out.update({k + "img": img, k + "pxpy": pxpy, k + "grad_out": g_out, k + "out": o.detach().numpy(), k + "grad_img": ti.grad.numpy()})
        print("%-12s C %d %s  max collisions per batch pair %d" % (name, C, kind, hits.max()))

    np.savez_compressed(a.out, **out)
    print("wrote %s: %d arrays, %d bytes" % (a.out, len(out), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
