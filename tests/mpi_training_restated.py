"""Hand-written float64 restatement (NumPy, explicit gradient formulas, no autograd) of the training-time half of the reference's utils/mpi as
INTEGRATION.md section 21 defines it: gather_pixel_by_pxpy, sample_pdf and disparity_consistency_src_to_tgt.

The reference's loss cannot run in float64 as written (gather_pixel_by_pxpy binds pxpy_int for float32 coordinates only), so the float64 values of
tests/golden/mpi_training.npz come from here; tests/golden/make_mpi_training_golden.py cross-checks this file against the reference's float64 autograd
with the coordinates cast to float32 at the gather's boundary only."""
import numpy as np


def pixel_index(v, n):
    """round to nearest even, clamp to [0, n - 1]; NaN and -inf give 0, +inf gives n - 1"""
    r = np.rint(np.asarray(v, dtype=np.float64))
    r = np.where(r >= 0, r, 0.0)
    return np.minimum(r, n - 1).astype(np.int64)


def gather_pixel_by_pxpy(img, pxpy):
    """img [B,C,H,W], pxpy [B,2,N] (float or integer) -> [B,C,N]"""
    B, C, H, W = img.shape
    idx = flat_index(pxpy, H, W)
    return np.take_along_axis(img.reshape(B, C, H * W), np.repeat(idx[:, None, :], C, axis=1), axis=2)


def flat_index(pxpy, H, W):
    if np.issubdtype(np.asarray(pxpy).dtype, np.integer):
        ix, iy = np.clip(pxpy[:, 0], 0, W - 1), np.clip(pxpy[:, 1], 0, H - 1)
    else:
        ix, iy = pixel_index(pxpy[:, 0], W), pixel_index(pxpy[:, 1], H)
    return (iy * W + ix).astype(np.int64)


def gather_pixel_by_pxpy_backward(grad_out, pxpy, H, W):
    """grad_out [B,C,N] -> grad_img [B,C,H,W]: a scatter-add"""
    B, C, N = grad_out.shape
    idx = flat_index(pxpy, H, W)
    g = np.zeros((B, C, H * W), dtype=np.float64)
    for b in range(B):
        for c in range(C):
            np.add.at(g[b, c], idx[b], grad_out[b, c].astype(np.float64))
    return g.reshape(B, C, H, W)


def sample_pdf(values, weights, u):
    """values, weights [B,1,N,S], u [B,1,N,NS] -> dict(samples [B,1,N,NS], idx (the searchsorted result), cdf_interval, u_margin: the smallest |u - cdf entry|)"""
    v, w, u = (np.asarray(a, dtype=np.float64) for a in (values, weights, u))
    B, _, N, S = w.shape
    edges = np.concatenate((v[..., 0:1], (v[..., 1:] + v[..., :-1]) * 0.5, v[..., -1:]), axis=3)
    pdf = w / (w.sum(axis=3, keepdims=True) + 1e-5)
    cdf = np.concatenate((np.zeros((B, 1, N, 1)), np.cumsum(pdf, axis=3)), axis=3)
    idx = (cdf[..., None, :] <= u[..., :, None]).sum(axis=-1)                 # searchsorted(right=True) on a non-decreasing row
    lo, hi = np.maximum(idx - 1, 0), np.minimum(idx, S)
    c_lo, c_hi = np.take_along_axis(cdf, lo, axis=3), np.take_along_axis(cdf, hi, axis=3)
    e_lo, e_hi = np.take_along_axis(edges, lo, axis=3), np.take_along_axis(edges, hi, axis=3)
    ci = c_hi - c_lo
    t = (u - c_lo) / np.maximum(ci, 1e-5)
    t = np.where(ci <= 1e-4, 0.5, t)
    return dict(samples=e_lo + t * (e_hi - e_lo), idx=idx, cdf_interval=ci, cdf=cdf)


def pdf_near_flip(cdf, u, cdf_interval):
    """per draw: u within 1e-5 of a cdf entry, or the selected interval within 1e-6 of the 1e-4 switch - where float32 could flip a discrete choice.
    A cdf entry that is exactly 0 (the leading one, and those behind zero weights: 0 / x is 0 in every precision) cannot flip against u == 0."""
    u = np.asarray(u, dtype=np.float64)
    gap = np.abs(cdf[..., None, :] - u[..., :, None])
    exact = (cdf[..., None, :] == 0.0) & (u[..., :, None] == 0.0)
    return (np.where(exact, 1.0, gap).min(axis=-1) < 1e-5) | (np.abs(cdf_interval - 1e-4) < 1e-6)


def disparity_consistency(K_src_inv, disparity_src, G_tgt_src, K_tgt, disparity_tgt, g=1.0):
    """disparity_src, disparity_tgt [B,1,H,W]; K_src_inv, K_tgt [B,3,3]; G_tgt_src [B,4,4]; g: the upstream gradient of the loss.
    -> dict(loss, count, grad_src, grad_tgt [B,1,H,W], mask [B,HW], idx [B,HW], px, py, pz [B,HW])"""
    Ki, ds, G, Kt, dt = (np.asarray(a, dtype=np.float64) for a in (K_src_inv, disparity_src, G_tgt_src, K_tgt, disparity_tgt))
    B, _, H, W = ds.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    grid = np.stack((xs.reshape(-1), ys.reshape(-1), np.ones(H * W)))           # [3,HW]
    r = Ki @ grid                                                                # [B,3,HW]
    d = ds.reshape(B, 1, H * W)
    depth = 1.0 / d
    p = G[:, :3, :3] @ (r * depth) + G[:, :3, 3:4]
    q = Kt @ p
    with np.errstate(divide="ignore", invalid="ignore"):
        px, py = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        mask = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
        idx = pixel_index(py, H) * W + pixel_index(px, W)
        inv_pz = 1.0 / p[:, 2]
    tgt = np.take_along_axis(dt.reshape(B, H * W), idx, axis=1)
    diff = inv_pz - tgt
    count = int(mask.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        loss = np.float64(np.abs(diff)[mask].sum()) / np.float64(count)          # count 0: 0 / 0 = NaN, the mean of an empty selection
        s = np.where(mask, np.sign(diff), 0.0)
        coef = np.where(mask, g * s / np.float64(count), 0.0)                    # dL / d (1 / p.z); 0 outside the mask, whatever count is
        gr = np.einsum("bk,bkn->bn", G[:, 2, :3], r)                             # d p.z / d depth
        grad_src = np.where(mask, coef * (-inv_pz * inv_pz) * gr * (-depth[:, 0] * depth[:, 0]), 0.0)
    grad_tgt = np.zeros((B, H * W))
    for b in range(B):
        np.add.at(grad_tgt[b], idx[b][mask[b]], -coef[b][mask[b]])
    return dict(loss=loss, count=count, grad_src=grad_src.reshape(B, 1, H, W), grad_tgt=grad_tgt.reshape(B, 1, H, W), mask=mask, idx=idx, px=px, py=py,
                pz=p[:, 2])


def near_boundary(px, py, pz, H, W, eps=1e-3):
    """per pixel: px or py within eps of a half-integer or of the mask bounds 0, W - 1, H - 1, or |p.z| < eps - where float32 could flip a discrete choice"""
    def near_half(v):
        f = v - np.floor(v)
        return np.abs(f - 0.5) < eps
    with np.errstate(invalid="ignore"):
        bad = near_half(px) | near_half(py) | (np.abs(px) < eps) | (np.abs(px - (W - 1)) < eps) | (np.abs(py) < eps) | (np.abs(py - (H - 1)) < eps)
        bad |= (np.abs(pz) < eps) | ~np.isfinite(px) | ~np.isfinite(py)
    return bad
