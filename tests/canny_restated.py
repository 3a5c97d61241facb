"""INTEGRATION.md section 17 restated: the masked Canny of warp-back stage 2, twice.

canny_restated   numpy float32, one operation at a time in the order section 17 writes them, on the float32 weights the kernel is handed
                 (ops.canny_weights).  ops.canny_masked must equal it on every pixel, and each stage alone its intermediate, bit for bit.
canny_witness    float64 with scipy.ndimage, in the shape of skimage's own implementation (gaussian_filter(mode='constant'), sobel,
                 binary_erosion(border_value=0), the four sectors as whole-array masks, label with a 3 x 3 structure).  It shares no code with
                 the restatement and guards it against a mistake of transcription that a bit-exact kernel would faithfully reproduce.

Neither imports the package; test_canny.py hands the weights in."""
import numpy as np

F32_EPS = np.float32(np.finfo(np.float32).eps)


def host_weights(sigma):
    """what ops.canny_weights computes, for callers without the package: (radius, float32 weights)"""
    import math
    radius = int(4.0 * float(sigma) + 0.5)
    phi = [math.exp(-0.5 / (float(sigma) * float(sigma)) * (k * k)) for k in range(-radius, radius + 1)]
    total = math.fsum(phi)
    return radius, np.array([p / total for p in phi], dtype=np.float64).astype(np.float32)


# ---------------------------------------------------------------- the restatement (float32)

def _smooth_axis(x, weights, axis):
    """taps from -r up, from 0, zero outside the image"""
    r = (len(weights) - 1) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(x, pad)
    n = x.shape[axis]
    acc = np.zeros_like(x)
    for k in range(2 * r + 1):
        sl = [slice(None), slice(None)]
        sl[axis] = slice(k, k + n)
        acc = acc + weights[k] * p[tuple(sl)]
    return acc


def restated_smooth(gray, mask, weights):
    weights = np.asarray(weights, dtype=np.float32)
    inside = mask != 0
    masked = np.where(inside, gray, np.float32(0)).astype(np.float32)
    ones = inside.astype(np.float32)
    g = _smooth_axis(_smooth_axis(masked, weights, 0), weights, 1)
    bleed = _smooth_axis(_smooth_axis(ones, weights, 0), weights, 1)
    with np.errstate(all="ignore"):
        return g / (bleed + F32_EPS)


def restated_classes(smoothed, mask, low, high):
    """0, 1 (weak), 2 (strong) per pixel"""
    h, w = smoothed.shape
    low, high = np.float32(low), np.float32(high)
    s = np.pad(smoothed, 1, mode="symmetric")                     # d c b a | a b c d
    two = np.float32(2)

    def at(dy, dx):
        return s[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    with np.errstate(all="ignore"):
        jsobel = ((at(-1, 1) - at(-1, -1)) + (at(1, 1) - at(1, -1))) + two * (at(0, 1) - at(0, -1))
        isobel = ((at(1, -1) - at(-1, -1)) + (at(1, 1) - at(-1, 1))) + two * (at(1, 0) - at(-1, 0))
        mag = np.sqrt(isobel * isobel + jsobel * jsobel)
    inside = mask != 0
    cls = np.zeros((h, w), dtype=np.uint8)
    one = np.float32(1)
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            m = mag[y, x]
            if not inside[y - 1:y + 2, x - 1:x + 2].all() or not m >= low:
                continue
            i, j = isobel[y, x], jsobel[y, x]
            up, down, right, left = i >= 0, i <= 0, j >= 0, j <= 0
            same = (up and right) or (down and left)
            opposite = (down and right) or (up and left)
            if not same and not opposite:
                continue
            ai, aj = np.abs(i), np.abs(j)
            with np.errstate(all="ignore"):
                if same:
                    diag = (1, 1)
                    if ai > aj:
                        wgt, axis = aj / ai, (1, 0)
                    else:
                        wgt, axis = ai / aj, (0, 1)
                else:
                    diag = (-1, 1)
                    if ai < aj:
                        wgt, axis = ai / aj, (0, 1)
                    else:
                        wgt, axis = aj / ai, (-1, 0)
                rest = one - wgt
                plus = mag[y + diag[0], x + diag[1]] * wgt + mag[y + axis[0], x + axis[1]] * rest
                minus = mag[y - diag[0], x - diag[1]] * wgt + mag[y - axis[0], x - axis[1]] * rest
            if plus <= m and minus <= m:
                cls[y, x] = 2 if m >= high else 1
    return cls


def restated_hysteresis(cls):
    """1.0 on the weak or strong pixels 8-connected through weak or strong pixels to a strong one: grown one ring at a time"""
    cand = (cls == 1) | (cls == 2)
    on = cls == 2
    while True:
        p = np.pad(on, 1)
        grown = np.zeros_like(on)
        for dy in range(3):
            for dx in range(3):
                grown |= p[dy:dy + on.shape[0], dx:dx + on.shape[1]]
        nxt = on | (cand & grown)
        if (nxt == on).all():
            return on.astype(np.float32)
        on = nxt


def canny_restated(gray, mask, weights, low=0.1, high=0.2, parts=False):
    """gray, mask [h,w] float32 -> edges [h,w] float32 of 0 and 1; parts=True: (edges, smoothed, classes)"""
    gray, mask = np.asarray(gray, dtype=np.float32), np.asarray(mask, dtype=np.float32)
    smoothed = restated_smooth(gray, mask, weights)
    cls = restated_classes(smoothed, mask, low, high)
    out = restated_hysteresis(cls)
    return (out, smoothed, cls) if parts else out


# ---------------------------------------------------------------- the witness (float64, scipy)

def canny_witness(gray, mask, sigma=2.0, low=0.1, high=0.2):
    """skimage.feature.canny's steps on float64 arrays -> bool [h,w]"""
    import scipy.ndimage as ndi
    image = np.asarray(gray, dtype=np.float64)
    mask = np.asarray(mask) != 0
    masked_image = np.zeros_like(image)
    masked_image[mask] = image[mask]
    bleed_over = ndi.gaussian_filter(mask.astype(np.float64), sigma, mode="constant") + float(F32_EPS)
    smoothed = ndi.gaussian_filter(masked_image, sigma, mode="constant") / bleed_over
    eroded_mask = ndi.binary_erosion(mask, np.ones((3, 3), bool), border_value=0)
    jsobel = ndi.sobel(smoothed, axis=1)
    isobel = ndi.sobel(smoothed, axis=0)
    abs_isobel, abs_jsobel = np.abs(isobel), np.abs(jsobel)
    magnitude = np.hypot(isobel, jsobel)
    eroded_mask = eroded_mask & (magnitude >= low)
    eroded_mask[0, :] = eroded_mask[-1, :] = False
    eroded_mask[:, 0] = eroded_mask[:, -1] = False
    local_maxima = np.zeros(image.shape, bool)

    def sector(pts, c1p, c2p, c1m, c2m, num, den):
        pts = pts & eroded_mask
        # cXY: slices of magnitude at the axis (1) and diagonal (2) neighbour of every pixel, + and - side, as (row shift, column shift)
        ys, xs = np.nonzero(pts)
        if not len(ys):
            return
        m = magnitude[ys, xs]
        with np.errstate(all="ignore"):
            wgt = num[ys, xs] / den[ys, xs]
        c_plus = magnitude[ys + c2p[0], xs + c2p[1]] * wgt + magnitude[ys + c1p[0], xs + c1p[1]] * (1 - wgt) <= m
        c_minus = magnitude[ys + c2m[0], xs + c2m[1]] * wgt + magnitude[ys + c1m[0], xs + c1m[1]] * (1 - wgt) <= m
        local_maxima[ys, xs] = c_plus & c_minus

    pos = (isobel >= 0) & (jsobel >= 0)
    neg = (isobel <= 0) & (jsobel <= 0)
    mix1 = (isobel <= 0) & (jsobel >= 0)
    mix2 = (isobel >= 0) & (jsobel <= 0)
    # the later sector wins where two hold (a zero component, equal components): they then give the same pair or the same weight
    sector((mix1 | mix2) & (abs_isobel >= abs_jsobel), (-1, 0), (-1, 1), (1, 0), (1, -1), abs_jsobel, abs_isobel)      # 135 to 180 degrees
    sector((mix1 | mix2) & (abs_isobel < abs_jsobel), (0, 1), (-1, 1), (0, -1), (1, -1), abs_isobel, abs_jsobel)       # 90 to 135
    sector((pos | neg) & (abs_isobel <= abs_jsobel), (0, 1), (1, 1), (0, -1), (-1, -1), abs_isobel, abs_jsobel)        # 45 to 90
    sector((pos | neg) & (abs_isobel > abs_jsobel), (1, 0), (1, 1), (-1, 0), (-1, -1), abs_jsobel, abs_isobel)         # 0 to 45
    high_mask = local_maxima & (magnitude >= high)
    labels, count = ndi.label(local_maxima, np.ones((3, 3), bool))
    if count == 0:
        return local_maxima
    sums = np.array(ndi.sum(high_mask, labels, np.arange(count, dtype=np.int32) + 1), copy=False, ndmin=1)
    good = np.zeros(count + 1, bool)
    good[1:] = sums > 0
    return good[labels]


# ---------------------------------------------------------------- cases

def random_case(seed, b, h, w):
    """seeded images of a few smooth blobs and steps over noise, with blobs of mask; every image of the batch has its own mask"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    gray = np.zeros((b, 1, h, w), np.float32)
    mask = np.ones((b, 1, h, w), np.float32)
    for i in range(b):
        img = 0.05 * rng.rand(h, w)
        for _ in range(4):
            cy, cx, rad = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2, max(3.0, min(h, w) / 2))
            img += rng.uniform(0.3, 1.0) * ((yy - cy) ** 2 + (xx - cx) ** 2 < rad * rad)
        img += rng.uniform(0.2, 0.8) * (xx * np.cos(i + 0.3) + yy * np.sin(i + 0.3) > rng.uniform(0.3, 0.7) * (h + w) / 2)
        gray[i, 0] = img.astype(np.float32)
        for _ in range(2):
            cy, cx, rad = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1, max(2.0, min(h, w) / 4))
            mask[i, 0][(yy - cy) ** 2 + (xx - cx) ** 2 < rad * rad] = 0
    return gray, mask


# the committed random cases: (seed, b, h, w).  Seeds are checked on the CPU against canny_witness (test_canny.py); INTEGRATION.md section 17
# records the seeds tried and rejected.
# 9 x 170 is wider than twice the kernels' 64-pixel tile and its halo of 8 on either side: two interior tile seams
RANDOM_CASES = [(1, 1, 5, 7), (2, 1, 17, 19), (3, 2, 33, 70), (4, 1, 9, 170)]
