"""TEST INFRASTRUCTURE: the warp-back renderer's definition restated in numpy, the oracle of tests/test_warpback.py.

rasterize()       the rasteriser: np.float32 scalars and arrays, one rounding per operation in the order of the definition, a loop over the
                  faces in ascending order, every pixel of the frame against every face (no bounding box of any kind).
mesh_vertices()   the vertex stage's formulas in a dtype of choice: float64 is the yardstick the kernel's and the reference's float32 errors
                  are measured against; float32 serves render_mesh().
render_mesh()     RGBDRenderer.render_mesh(construct_mesh(rgbd)) on top of the two.
"""
import numpy as np

F32 = np.float32
EPS8 = F32(1e-8)


def grid_faces(h, w):
    """[F,3] int64: cell q = r (w - 1) + c; face q = (tl, bl, br), face Q + q = (br, tr, tl)"""
    r, c = np.meshgrid(np.arange(h - 1), np.arange(w - 1), indexing="ij")
    tl = (r * w + c).reshape(-1)
    tr, bl, br = tl + 1, tl + w, tl + w + 1
    return np.concatenate([np.stack([tl, bl, br], -1), np.stack([br, tr, tl], -1)]).astype(np.int64)


def ndc(k, S1, S2):
    rng = F32(2) if S1 <= S2 else (F32(S1) * F32(2)) / F32(S2)
    off = rng / F32(2)
    return -off + (rng * np.asarray(k).astype(F32) + off) / F32(S1)


def pixel_centres(h, w):
    """(px, py), [h,w] float32 each: +x left, +y up"""
    py = ndc(h - 1 - np.arange(h), h, w)
    px = ndc(w - 1 - np.arange(w), w, h)
    return np.broadcast_to(px[None, :], (h, w)).copy(), np.broadcast_to(py[:, None], (h, w)).copy()


def edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def seg(px, py, ax, ay, bx, by):
    abx, aby = bx - ax, by - ay
    l2 = abx * abx + aby * aby
    if l2 <= EPS8:
        ex, ey = px - bx, py - by
        return ex * ex + ey * ey
    t = (abx * (px - ax) + aby * (py - ay)) / l2
    t = np.where(t < 0, F32(0), t)
    t = np.where(t > 1, F32(1), t)
    qx, qy = ax + t * abx, ay + t * aby
    ex, ey = px - qx, py - qy
    return ex * ex + ey * ey


def rasterize(verts_ndc, attrs, h, w, blur_radius=1e-6, rows=None):
    """verts_ndc [B,h*w,3], attrs [B,h*w,C] float32 -> (pix_to_face int64 [B,h,w], zbuf [B,h,w], bary [B,h,w,3], out [B,C,h,w]).
    rows: a slice of output rows to compute alone (every face still meets every pixel of them): the outputs then hold those rows only"""
    verts_ndc, attrs = np.asarray(verts_ndc), np.asarray(attrs)
    assert verts_ndc.dtype == F32 and attrs.dtype == F32
    B, C = verts_ndc.shape[0], attrs.shape[2]
    faces = grid_faces(h, w)
    nf = len(faces)
    blur = F32(blur_radius)
    px, py = pixel_centres(h, w)
    if rows is not None:
        px, py = px[rows], py[rows]
    hh = px.shape[0]
    pix = np.full((B, hh, w), -1, np.int64)
    zbuf = np.full((B, hh, w), -1, F32)
    bary = np.full((B, hh, w, 3), -1, F32)
    out = np.zeros((B, C, hh, w), F32)
    with np.errstate(all="ignore"):
        for b in range(B):
            best = np.full((hh, w), np.inf, F32)
            for f in range(nf):
                (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = verts_ndc[b, faces[f]]
                if not np.isfinite(verts_ndc[b, faces[f]]).all():
                    continue
                area = edge(x2, y2, x0, y0, x1, y1)
                if abs(area) <= EPS8 or max(z0, z1, z2) < 0:
                    continue
                den = area + EPS8
                w0 = edge(px, py, x1, y1, x2, y2) / den
                w1 = edge(px, py, x2, y2, x0, y0) / den
                w2 = edge(px, py, x0, y0, x1, y1) / den
                pz = (w0 * z0 + w1 * z1) + w2 * z2
                inside = (w0 > 0) & (w1 > 0) & (w2 > 0)
                d = seg(px, py, x0, y0, x1, y1)
                d02 = seg(px, py, x0, y0, x2, y2)
                d12 = seg(px, py, x1, y1, x2, y2)
                d = np.where(d02 < d, d02, d)
                d = np.where(d12 < d, d12, d)
                covered = (pz >= 0) & (inside | (d < blur))
                take = covered & ((pix[b] < 0) | (pz < best))            # ascending f and a strict <: the lowest face wins equal depth
                if not take.any():
                    continue
                best[take] = pz[take]
                pix[b][take] = b * nf + f
                zbuf[b][take] = pz[take]
                bary[b][take] = np.stack([w0, w1, w2], -1)[take]
                a0, a1, a2 = attrs[b, faces[f]]
                for k in range(C):
                    out[b, k][take] = ((w0 * a0[k] + w1 * a1[k]) + w2 * a2[k])[take]
    assert zbuf.dtype == F32 and bary.dtype == F32 and out.dtype == F32
    return pix, zbuf, bary, out


def sobel_alpha(disp, T):
    """disp [B,h,w] -> exp(-10 |Sobel|) in dtype T, zero padding"""
    d = np.pad(disp.astype(T), ((0, 0), (1, 1), (1, 1)))
    two = T(2)
    gx = ((d[:, :-2, 2:] - d[:, :-2, :-2]) + two * (d[:, 1:-1, 2:] - d[:, 1:-1, :-2])) + (d[:, 2:, 2:] - d[:, 2:, :-2])
    gy = ((d[:, 2:, :-2] - d[:, :-2, :-2]) + two * (d[:, 2:, 1:-1] - d[:, :-2, 1:-1])) + (d[:, 2:, 2:] - d[:, :-2, 2:])
    return np.exp(T(-10) * np.sqrt(gx * gx + gy * gy))


def mesh_vertices(rgbd, cam_int, cam_ext, T=np.float64):
    """the vertex stage's formulas with every operation in dtype T (the inputs are float32 values) -> (verts_ndc [B,h*w,3], attrs [B,h*w,5])"""
    rgbd, K, E = np.asarray(rgbd), np.asarray(cam_int), np.asarray(cam_ext).astype(T)
    B, _, h, w = rgbd.shape
    Kinv = np.linalg.inv(K.astype(np.float64)).astype(T)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    u, v = (x.astype(T) + T(0.5)) / T(w), (y.astype(T) + T(0.5)) / T(h)
    verts = np.zeros((B, h, w, 3), T)
    attrs = np.zeros((B, h, w, 5), T)
    near, far = T(F32(1e-4)), T(F32(1e4))
    pa, pb = (near + far) / (far - near), ((T(-2) * near) * far) / (far - near)
    if T == F32:
        pa, pb = (F32(1e-4) + F32(1e4)) / (F32(1e4) - F32(1e-4)), ((F32(-2) * F32(1e-4)) * F32(1e4)) / (F32(1e4) - F32(1e-4))
    aspect = T(F32(w / h))
    alpha = sobel_alpha(rgbd[:, 3], T)
    for b in range(B):
        depth = T(1) / (rgbd[b, 3].astype(T) + T(F32(1e-4)))
        k, e, Kb = Kinv[b], E[b], K[b].astype(T)
        P = [((k[i, 0] * u + k[i, 1] * v) + k[i, 2]) * depth for i in range(3)]
        Wd = [((e[i, 0] * P[0] + e[i, 1] * P[1]) + e[i, 2] * P[2]) + e[i, 3] for i in range(3)]
        nx = (T(2) * Kb[0, 0]) * Wd[0] + (T(2) * Kb[0, 2] - T(1)) * Wd[2]
        ny = (T(2) * Kb[1, 1]) * Wd[1] + (T(2) * Kb[1, 2] - T(1)) * Wd[2]
        nz = pa * Wd[2] + pb
        verts[b, ..., 0] = (nx / Wd[2]) * T(-1) * aspect
        verts[b, ..., 1] = (ny / Wd[2]) * T(-1)
        verts[b, ..., 2] = nz / Wd[2]
        attrs[b, ..., :3] = rgbd[b, :3].transpose(1, 2, 0)
        attrs[b, ..., 3] = alpha[b] > T(F32(0.3))
        attrs[b, ..., 4] = Wd[2]
    return verts.reshape(B, h * w, 3), attrs.reshape(B, h * w, 5)


def render_mesh(rgbd, cam_int, cam_ext, blur_radius=1e-6):
    """RGBDRenderer.render_mesh(construct_mesh(rgbd, cam_int), cam_int, cam_ext) -> (render * mask, disparity * mask, mask), float32"""
    _, _, h, w = rgbd.shape
    verts, attrs = mesh_vertices(np.asarray(rgbd, F32), np.asarray(cam_int, F32), np.asarray(cam_ext, F32), F32)
    assert verts.dtype == F32 and attrs.dtype == F32
    out = rasterize(verts, attrs, h, w, blur_radius)[3]
    mask = out[:, 3:4]
    with np.errstate(all="ignore"):
        disparity = F32(1) / (out[:, 4:5] + F32(1e-4))
    return out[:, :3] * mask, disparity * mask, mask
