"""INTEGRATION.md section 18 restated in numpy: the sparse bilateral filter (a 0/1-weighted median around disparity discontinuities).

sparse_bilateral_restated   the whole filter on one [h,w] array of float32 or float64 (the uint8 call site is value = u / 255.0 in float64,
                            and the result's bytes are round(out * 255): a selection of input values, so exact).  It must equal the
                            reference's recorded outputs (tests/golden/bilateral.npz) and ops.sparse_bilateral_filter bit for bit.
kstar                       k*(n) by its definition in numpy float32.

Vectorised over the pixels (one sort of the windows), so that 100 x 150 takes well under a second.  Does not import the package."""
import numpy as np

F32 = np.float32


def kstar(n):
    """1 + #{k <= n : S_k <= 0.5}, S_k the float32 sum of k copies of fl32(1 / n) added one at a time"""
    c = np.ones(n, F32) / F32(n)
    return 1 + int((np.cumsum(c, dtype=F32) <= F32(0.5)).sum())


def discontinuity_map(v, depth, threshold, mask=None):
    """step 1: D [h,w] bool.  v: this iteration's input, depth: the call's input, both of one float dtype"""
    h, w = v.shape
    thr = v.dtype.type(threshold)
    with np.errstate(divide="ignore", invalid="ignore"):
        disp = v.dtype.type(1) / v
        D = np.zeros((h, w), bool)
        c = disp[1:-1, 1:-1]
        mc = None if mask is None else mask[1:-1, 1:-1] != 0
        for sl in ((slice(0, -2), slice(1, -1)), (slice(2, None), slice(1, -1)), (slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None))):
            over = np.abs(c - disp[sl]) > thr                              # NaN > t is false
            if mask is not None:
                over &= mc & (mask[sl] != 0)                               # diff * 0 is 0 or NaN: never over
            D[1:-1, 1:-1] |= over
    D[depth == 0] = True
    if mask is not None:
        D[mask == 0] = False
    return D


def windows(a, m):
    return np.lib.stride_tricks.sliding_window_view(a, (2 * m + 1, 2 * m + 1)).reshape(a.shape[0] - 2 * m, a.shape[1] - 2 * m, -1)


def select(v, D, ws, mask=None, rank=kstar, with_n=False):
    """steps 2 and 3: one iteration's output (with_n: and the valid count of every pixel that selects, 0 elsewhere).  `rank`: k*(n)"""
    m = ws // 2
    ring = lambda a: np.pad(a[1:-1, 1:-1], 1, "edge")
    v1, D1 = ring(v), ring(D)
    out = v1.copy()
    pv, pD = windows(np.pad(v1, m, "edge"), m), windows(np.pad(D1, m, "edge"), m)
    valid = ~pD
    active = pD.any(-1)
    if mask is not None:
        valid = valid & windows(np.pad(mask != 0, m, "constant"), m)
        active &= mask != 0
    n = valid.sum(-1)
    active &= n > 0                                                        # n == 0: the centre of v', which out holds
    table = np.array([0] + [rank(i) for i in range(1, ws * ws + 1)])
    keys = np.where(valid, pv, np.inf)[active]                             # finite inputs: the invalid sort last
    keys.sort(-1)
    out[active] = keys[np.arange(len(keys)), table[n[active]] - 1]
    return (out, np.where(active, n, 0)) if with_n else out


def sparse_bilateral_restated(depth, filter_size, depth_threshold=0.04, mask=None, num_iter=None):
    num_iter = len(filter_size) if num_iter is None else num_iter
    v = depth.copy()
    for i in range(num_iter):
        v = select(v, discontinuity_map(v, depth, depth_threshold, mask), filter_size[i], mask)
    return v


def restated_u8(u8, filter_size, depth_threshold=0.04, mask=None, num_iter=None):
    """the uint8 call site: (float64 result, its bytes)"""
    out = sparse_bilateral_restated(u8.astype(np.float64) / 255.0, filter_size, depth_threshold, mask, num_iter)
    b = np.rint(out * 255.0).astype(np.uint8)
    assert (b.astype(np.float64) / 255.0 == out).all()
    return out, b


def blocky(seed, h, w, zeros=0.03):
    """the test pattern: 4 x 4 blocks of random levels with +-3 noise and about 3 % zero pixels -> uint8 [h,w]"""
    rs = np.random.RandomState(seed)
    lev = rs.randint(8, 248, ((h + 3) // 4, (w + 3) // 4))
    a = np.kron(lev, np.ones((4, 4), int))[:h, :w] + rs.randint(-3, 4, (h, w))
    a = np.clip(a, 1, 255)
    a[rs.rand(h, w) < zeros] = 0
    return a.astype(np.uint8)


def random_mask(seed, h, w, keep=0.85):
    return (np.random.RandomState(seed).rand(h, w) < keep).astype(F32)
