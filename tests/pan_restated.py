"""The first residual block of the plane-adjustment network as mpf_pan_block1 computes it - factorised over the constant plane channel - restated
in float64 numpy.  TEST INFRASTRUCTURE: it is what tests/test_pan_host.py holds against the reference's recorded float64 run (tests/golden/pan.npz),
so that the factorisation, the border sums, the halo rule and the floor pooling are pinned without a GPU.  Not code under test.

    x_s = cat(rgb_low, disp_low, d_s);  block(x_s) = relu(conv3(x_s) + conv2(bn(relu(conv1(x_s)))));  out = avg_pool2d(block, 2)
    conv1(x_s) = A1 + d_s * B1          A1 = b1 + conv1 over the four image channels;  B1[o,y,x] = the sum of w1[o,4,tap] over the taps inside the frame
    conv3(x_s) = A3 + d_s * w3[:,4]     A3 = bias3 + conv3 over the four image channels
"""
import numpy as np

EPS = 1e-5          # nn.BatchNorm2d's default


def taps(h, w):
    """(dy, dx, the [h,w] mask of the pixels whose tap (dy, dx) lies inside the frame) for the nine taps of a 3 x 3 with zero padding"""
    yy, xx = np.mgrid[0:h, 0:w]
    for t in range(9):
        dy, dx = t // 3 - 1, t % 3 - 1
        yield t, dy, dx, (yy + dy >= 0) & (yy + dy < h) & (xx + dx >= 0) & (xx + dx < w)


def shifted(x, dy, dx):
    """x [C,h,w] read at (y + dy, x + dx), zero outside the frame"""
    C, h, w = x.shape
    pad = np.zeros((C, h + 2, w + 2), x.dtype)
    pad[:, 1:-1, 1:-1] = x
    return pad[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def conv3x3(x, weight):
    """x [C,h,w], weight [O,C,3,3] -> [O,h,w], zero padding 1, no bias"""
    out = np.zeros((weight.shape[0],) + x.shape[1:], np.float64)
    for t, dy, dx, _ in taps(*x.shape[1:]):
        out += np.einsum("oc,chw->ohw", weight[:, :, t // 3, t % 3], shifted(x, dy, dx))
    return out


def shared_maps(x4, P):
    """x4 [4,h,w] (rgb, disparity) -> A1 [8,h,w], B1 [8,h,w], A3 [8,h,w]"""
    h, w = x4.shape[1:]
    A1 = P["conv1.bias"][:, None, None] + conv3x3(x4, P["conv1.weight"][:, :4])
    B1 = np.zeros((8, h, w), np.float64)
    for t, dy, dx, inside in taps(h, w):                        # border sums: only the taps that fall inside the frame see the constant
        B1 += P["conv1.weight"][:, 4, t // 3, t % 3][:, None, None] * inside[None]
    A3 = P["conv3.bias"][:, None, None] + np.einsum("oc,chw->ohw", P["conv3.weight"][:, :4, 0, 0], x4)
    return A1, B1, A3


def block1(rgb_low, disp_low, init_disp, P):
    """rgb_low [B,3,h,w], disp_low [B,1,h,w], init_disp [B,S]; P: the block's state_dict entries ("conv1.weight", ..., "bn.running_var") -> [B*S,8,h//2,w//2]"""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    B, S = init_disp.shape
    h, w = rgb_low.shape[-2:]
    hp, wp = h // 2, w // 2                                     # avg_pool2d floors: an odd last row / column is dropped
    scale = P["bn.weight"] / np.sqrt(P["bn.running_var"] + EPS)
    shift = P["bn.bias"] - P["bn.running_mean"] * scale
    out = np.zeros((B * S, 8, hp, wp), np.float64)
    for b in range(B):
        A1, B1, A3 = shared_maps(np.concatenate([rgb_low[b], disp_low[b]]).astype(np.float64), P)
        for s in range(S):
            d = float(init_disp[b, s])
            m = scale[:, None, None] * np.maximum(A1 + d * B1, 0.0) + shift[:, None, None]
            # the halo rule: conv2 pads ITS input, m, with zeros - outside the frame m is 0, not bn(relu(conv1)) of a padded x
            v = np.maximum(P["conv2.bias"][:, None, None] + conv3x3(m, P["conv2.weight"]) + A3 + d * P["conv3.weight"][:, 4, 0, 0][:, None, None], 0.0)
            out[b * S + s] = v[:, :2 * hp, :2 * wp].reshape(8, hp, 2, wp, 2).mean(axis=(2, 4))
    return out
