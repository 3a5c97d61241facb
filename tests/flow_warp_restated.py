"""The backward warps by a flow field (the reference's utils/transform.py:60-111, warp and warp_rife) restated by hand: numpy, float64 by default,
no autograd.  INTEGRATION.md section 22 holds the same formulas in words.  tests/golden/make_flow_warp_golden.py checks this file against the
reference's own float64 run; the GPU tests compare the kernels with it.

Per pixel (x, y) with (u, v) = flow[b, :, y, x]:
  warp        g = 2 (x + u) / max(W - 1, 1) - 1;  ix = ((g + 1) W - 1) / 2;  zero padding;  mask = the sum of the weights of the taps inside;
              d ix / d u = W / max(W - 1, 1)
  warp_rife   g = lin_W[x] + u / ((W - 1) / 2);  ix = (g + 1) / 2 (W - 1) clamped to [0, W - 1], no gradient where the unclamped ix <= 0 or >= W - 1;
              d ix / d u = 1 inside
  both        x0 = floor(ix), a = ix - x0 (y0, b likewise);  out = sum over the four taps of x[tap] * weight, weights (1 - a)(1 - b), a (1 - b),
              (1 - a) b, a b;  grad_x[tap] += weight * g_out;  grad_flow[b, 0] = d ix / d u * sum over c of g_out * d out / d ix."""
import numpy as np

WARP, RIFE = 0, 1


def golden_f64(gold, case, mode, field):
    """the reference's float64 value of tests/golden/flow_warp.npz: the file keeps its float32 run and float32(float64 run - float32 run)"""
    k = "%s/%s/" % (case, mode)
    return gold[k + "ref32/" + field].astype(np.float64) + gold[k + "d64/" + field].astype(np.float64)


def sample_positions(flow, mode, dtype=np.float64, lin=None):
    """-> dict(ix, iy: the sample coordinates [B,H,W] (clamped for RIFE), rx, ry: the same before the clamp, mx, my: 1 where a gradient passes,
    sx, sy: d ix / d u and d iy / d v).  dtype=np.float32 rounds every operation to float32 in the reference's order (a check of which cells its
    float32 run takes); lin: (lin_W, lin_H) of that run, np.linspace in `dtype` otherwise."""
    B, two, H, W = flow.shape
    assert two == 2
    t = dtype
    f = flow.astype(t)
    xs, ys = np.arange(W, dtype=t)[None, None, :], np.arange(H, dtype=t)[None, :, None]
    if mode == WARP:
        gx = t(2) * (xs + f[:, 0]) / t(max(W - 1, 1)) - t(1)
        gy = t(2) * (ys + f[:, 1]) / t(max(H - 1, 1)) - t(1)
        rx = ((gx + t(1)) * t(W) - t(1)) / t(2)
        ry = ((gy + t(1)) * t(H) - t(1)) / t(2)
        ix, iy = rx, ry
        mx, my = np.ones(rx.shape, bool), np.ones(ry.shape, bool)
        sx, sy = W / max(W - 1, 1), H / max(H - 1, 1)
    else:
        assert H >= 2 and W >= 2
        lw, lh = (np.linspace(-1, 1, W).astype(t), np.linspace(-1, 1, H).astype(t)) if lin is None else (np.asarray(lin[0], t), np.asarray(lin[1], t))
        gx = lw[None, None, :] + f[:, 0] / t((W - 1.0) / 2.0)
        gy = lh[None, :, None] + f[:, 1] / t((H - 1.0) / 2.0)
        rx = (gx + t(1)) / t(2) * t(W - 1)
        ry = (gy + t(1)) / t(2) * t(H - 1)
        mx, my = (rx > 0) & (rx < W - 1), (ry > 0) & (ry < H - 1)
        ix, iy = np.clip(rx, 0, W - 1), np.clip(ry, 0, H - 1)
        sx = sy = 1.0
    return dict(ix=ix, iy=iy, rx=rx, ry=ry, mx=mx, my=my, sx=sx, sy=sy)


def cells(pos):
    """the integer cell of every sample: (floor(ix), floor(iy)) as int64, and for RIFE which side of the clamp it is on"""
    return np.floor(pos["ix"]).astype(np.int64), np.floor(pos["iy"]).astype(np.int64), pos["mx"], pos["my"]


def near_flip(pos, mode, H, W, margin=1e-3):
    """pixels whose coordinate sits within `margin` of a place where grad_flow jumps: an integer, and for RIFE the clamp bounds 0 and n - 1 (a
    coordinate the clamp has caught is on a bound by construction and stays there: only its unclamped value is looked at)"""
    bad = np.zeros(pos["rx"].shape, bool)
    for r, m, n in ((pos["rx"], pos["mx"], W), (pos["ry"], pos["my"], H)):
        near_int = np.abs(r - np.round(r)) < margin
        if mode == WARP:
            bad |= near_int
        else:
            bad |= (near_int & m) | (np.abs(r) < margin) | (np.abs(r - (n - 1)) < margin)
    return bad


def flow_warp(x, flow, mode, g_out=None):
    """-> dict(out [B,C,H,W], mask [B,1,H,W], all_in [B,H,W] bool: every tap inside; with g_out also grad_x [B,C,H,W] and grad_flow [B,2,H,W]),
    float64"""
    B, C, H, W = x.shape
    x64 = x.astype(np.float64)
    pos = sample_positions(flow, mode)
    ix, iy = pos["ix"], pos["iy"]
    x0, y0 = np.floor(ix), np.floor(iy)
    a, b = ix - x0, iy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    bi = np.arange(B)[:, None, None]
    out = np.zeros((B, C, H, W))
    mask = np.zeros((B, H, W))
    dix, diy = np.zeros((B, C, H, W)), np.zeros((B, C, H, W))
    all_in = np.ones((B, H, W), bool)
    grad_x = np.zeros((B, C, H * W)) if g_out is not None else None
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):                  # nw, ne, sw, se
        wx, wy = (a if dx else 1.0 - a), (b if dy else 1.0 - b)
        dwx, dwy = (1.0 if dx else -1.0), (1.0 if dy else -1.0)
        xi, yi = x0 + dx, y0 + dy
        inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        all_in &= inside
        xc, yc = np.clip(xi, 0, W - 1), np.clip(yi, 0, H - 1)
        val = x64[bi, :, yc, xc].transpose(0, 3, 1, 2) * inside[:, None]       # [B,H,W,C] -> [B,C,H,W]; 0 outside
        w = wx * wy * inside
        out += val * w[:, None]
        mask += w
        dix += val * (dwx * wy)[:, None]
        diy += val * (wx * dwy)[:, None]
        if g_out is not None:
            flat = (yc * W + xc).reshape(B, H * W)
            contrib = (g_out.astype(np.float64) * w[:, None]).reshape(B, C, H * W)
            for bb in range(B):
                for c in range(C):
                    np.add.at(grad_x[bb, c], flat[bb], contrib[bb, c])
    r = dict(out=out, mask=mask[:, None], all_in=all_in, pos=pos)
    if g_out is not None:
        g = g_out.astype(np.float64)
        gfx = pos["sx"] * pos["mx"] * (g * dix).sum(axis=1)
        gfy = pos["sy"] * pos["my"] * (g * diy).sum(axis=1)
        r["grad_x"] = grad_x.reshape(B, C, H, W)
        r["grad_flow"] = np.stack([gfx, gfy], axis=1)
    return r
