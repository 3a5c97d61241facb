// mpf_canny.hip - warp-back stage 2's edge detector for gfx950: skimage.feature.canny(gray, sigma, mask=mask) per image of a batch, on the
// stream, with no host copy (the reference's get_edge copies to the host and loops over the images in Python).
//
// Contract: include/mpiflow_hip.h (MpfCannyArgs); INTEGRATION.md section 17 holds the definition, which tests/canny_restated.py restates in
// numpy.  Every operation is fp32, rounded once, in the order written there (the build has no contraction and correctly rounded divide / sqrt).
//
// k_canny_smooth     a 64 x 16 tile of pixels per workgroup.  The masked image and the 0/1 mask of the tile and its halo of `radius` go to
//                    LDS (zero outside the image), are filtered along the row index into LDS, then along the column index; the quotient is
//                    stored.  LDS: 8 ((16 + 2 r)(64 + 2 r) + 16 (64 + 2 r)) bytes: 30 KiB at r = 8, 48 KiB at the bound r = 16.
// k_canny_classify   the same tile.  smoothed with a halo of 2 (indices clamped: the reflected border of a 3-tap filter) and the mask with a
//                    halo of 1 go to LDS; the magnitude of the tile and a halo of 1 is formed in LDS; every pixel then recomputes its own
//                    two Sobel responses and takes its class.  LDS: 11.3 KiB.
// k_canny_hyst       one workgroup of 1024 per image.  The classes are packed by wave ballots into two bit planes, C (weak or strong) and
//                    S (on; strong at first), one 32-bit word per 32 pixels of a row, in LDS - or, past MPF_CANNY_LDS_WORDS words per plane,
//                    in the workspace, with the same code.  A sweep gives every word S <- fill(S | C & dilate3x3(S)) where fill floods S
//                    along the runs of C inside the word; words are updated in place (S only grows, so a stale read costs a sweep, never
//                    a bit).  The loop ends on the first sweep in which no word changed (__syncthreads_or), or after h w sweeps: every
//                    sweep but the last turns a pixel on.  The fixpoint is unique, so the bytes do not depend on the schedule.
//                    WORST CASE: a sweep visits all n = h ceil(w / 32) words of the image, ceil(n / 1024) per thread, on ONE workgroup, and
//                    a one-pixel-wide weak chain lit from one end advances by as little as one word per sweep, so the count of sweeps can
//                    reach the count of words on the chain (about n / 2 for a serpentine over half the map).  The work is then of order
//                    n^2 / 2 word visits on one CU: about 5e3 at 33 x 70 and 5e6 for 256 x 384 in LDS, but 3.5e13 for a single
//                    16384 x 16384 image in the workspace (B h w = 2^28, the bound), which keeps one workgroup busy for a very long
//                    time.  The loop is bounded and waits on nobody, but a caller on a shared machine who cannot rule such
//                    chains out should keep single images small (tile them, or stay within the LDS path: h ceil(w / 32) <= 6144).
//
// No workgroup waits for another, no launch depends on data, every loop is bounded by the shape, and no address depends on a tensor's value.
#include "mpf_common.h"
#include <float.h>
#include <math.h>

#define CN_TW 64
#define CN_TH 16
#define CN_THREADS 256
#define CN_HYST_THREADS 1024

struct CannyDev {
    const float *gray, *mask;
    float *smoothed;             // [B,h,w]
    unsigned char *cls;          // [B,h,w]
    unsigned int *bits;          // [B,2,h,wpr]: k_canny_hyst's planes where they do not fit in LDS
    float *out;
    int h, w, hw, r, wpr, tiles_x;
    float lo, hi;
    float wt[2 * MPF_CANNY_MAX_RADIUS + 1];
};

// ---------------------------------------------------------------- stage 1

__global__ __launch_bounds__(CN_THREADS) void k_canny_smooth(const CannyDev a)
{
    extern __shared__ float sm[];
    const int r = a.r, IW = CN_TW + 2 * r, IH = CN_TH + 2 * r;
    float *sImg = sm, *sOne = sImg + IH * IW, *vImg = sOne + IH * IW, *vOne = vImg + CN_TH * IW;
    const int tyi = blockIdx.x / a.tiles_x, txi = blockIdx.x - tyi * a.tiles_x;
    const int x0 = txi * CN_TW, y0 = tyi * CN_TH;
    const size_t plane = (size_t)blockIdx.y * a.hw;
    for (int i = threadIdx.x; i < IH * IW; i += CN_THREADS) {
        const int yy = i / IW, xx = i - yy * IW;
        const int gy = y0 - r + yy, gx = x0 - r + xx;
        float v = 0.0f, one = 0.0f;
        if (gy >= 0 && gy < a.h && gx >= 0 && gx < a.w) {
            const size_t o = plane + (size_t)gy * a.w + gx;
            if (a.mask[o] != 0.0f) v = a.gray[o], one = 1.0f;
        }
        sImg[i] = v, sOne[i] = one;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CN_TH * IW; i += CN_THREADS) {          // along the row index
        const int ty = i / IW, xx = i - ty * IW;
        float s0 = 0.0f, s1 = 0.0f;
        for (int k = 0; k <= 2 * r; ++k) {
            s0 = s0 + a.wt[k] * sImg[(ty + k) * IW + xx];
            s1 = s1 + a.wt[k] * sOne[(ty + k) * IW + xx];
        }
        vImg[i] = s0, vOne[i] = s1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CN_TH * CN_TW; i += CN_THREADS) {       // along the column index
        const int ty = i / CN_TW, tx = i - ty * CN_TW;
        const int gy = y0 + ty, gx = x0 + tx;
        if (gy >= a.h || gx >= a.w) continue;                             // no barrier below
        float s0 = 0.0f, s1 = 0.0f;
        for (int k = 0; k <= 2 * r; ++k) {
            s0 = s0 + a.wt[k] * vImg[ty * IW + tx + k];
            s1 = s1 + a.wt[k] * vOne[ty * IW + tx + k];
        }
        a.smoothed[plane + (size_t)gy * a.w + gx] = s0 / (s1 + FLT_EPSILON);
    }
}

// ---------------------------------------------------------------- stage 2

#define CN_SW (CN_TW + 4)
#define CN_SH (CN_TH + 4)
#define CN_MW (CN_TW + 2)
#define CN_MH (CN_TH + 2)

// the two Sobel responses at (py, px) of the smoothed tile (tile coordinates with the halo of 2)
__device__ __forceinline__ void canny_sobel(const float *s, int py, int px, float &isobel, float &jsobel)
{
    const float *u = s + (py - 1) * CN_SW + px, *c = u + CN_SW, *d = c + CN_SW;
    jsobel = ((u[1] - u[-1]) + (d[1] - d[-1])) + 2.0f * (c[1] - c[-1]);
    isobel = ((d[-1] - u[-1]) + (d[1] - u[1])) + 2.0f * (d[0] - u[0]);
}

__global__ __launch_bounds__(CN_THREADS) void k_canny_classify(const CannyDev a)
{
    __shared__ float sS[CN_SH * CN_SW];
    __shared__ float sM[CN_MH * CN_MW];
    __shared__ unsigned char sE[CN_MH * CN_MW];
    const int tyi = blockIdx.x / a.tiles_x, txi = blockIdx.x - tyi * a.tiles_x;
    const int x0 = txi * CN_TW, y0 = tyi * CN_TH;
    const size_t plane = (size_t)blockIdx.y * a.hw;
    for (int i = threadIdx.x; i < CN_SH * CN_SW; i += CN_THREADS) {
        const int yy = i / CN_SW, xx = i - yy * CN_SW;
        int gy = y0 - 2 + yy, gx = x0 - 2 + xx;
        gy = gy < 0 ? 0 : (gy > a.h - 1 ? a.h - 1 : gy);                  // d c b a | a b c d, one sample deep
        gx = gx < 0 ? 0 : (gx > a.w - 1 ? a.w - 1 : gx);
        sS[i] = a.smoothed[plane + (size_t)gy * a.w + gx];
    }
    for (int i = threadIdx.x; i < CN_MH * CN_MW; i += CN_THREADS) {
        const int yy = i / CN_MW, xx = i - yy * CN_MW;
        const int gy = y0 - 1 + yy, gx = x0 - 1 + xx;
        const bool in = gy >= 0 && gy < a.h && gx >= 0 && gx < a.w;
        sE[i] = in && a.mask[plane + (size_t)gy * a.w + gx] != 0.0f ? 1 : 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CN_MH * CN_MW; i += CN_THREADS) {
        const int yy = i / CN_MW, xx = i - yy * CN_MW;
        float is, js;
        canny_sobel(sS, yy + 1, xx + 1, is, js);
        sM[i] = sqrtf(is * is + js * js);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CN_TH * CN_TW; i += CN_THREADS) {
        const int ty = i / CN_TW, tx = i - ty * CN_TW;
        const int gy = y0 + ty, gx = x0 + tx;
        if (gy >= a.h || gx >= a.w) continue;                             // no barrier below
        unsigned char cls = 0;
        const float *M = sM + (ty + 1) * CN_MW + tx + 1;
        const unsigned char *E = sE + (ty + 1) * CN_MW + tx + 1;
        const float m = M[0];
        const bool eroded = E[-CN_MW - 1] && E[-CN_MW] && E[-CN_MW + 1] && E[-1] && E[0] && E[1] && E[CN_MW - 1] && E[CN_MW] && E[CN_MW + 1];
        if (gy >= 1 && gy <= a.h - 2 && gx >= 1 && gx <= a.w - 2 && eroded && m >= a.lo) {
            float is, js;
            canny_sobel(sS, ty + 2, tx + 2, is, js);
            const bool up = is >= 0.0f, down = is <= 0.0f, right = js >= 0.0f, left = js <= 0.0f;
            const bool same = (up && right) || (down && left), opposite = (down && right) || (up && left);
            if (same || opposite) {
                const float ai = fabsf(is), aj = fabsf(js);
                int axis, diag;                                           // offsets in sM of the pair on the + side; the - side negates them
                float wgt;
                if (same) {
                    diag = CN_MW + 1;
                    if (ai > aj) wgt = aj / ai, axis = CN_MW;
                    else wgt = ai / aj, axis = 1;
                } else {
                    diag = -CN_MW + 1;
                    if (ai < aj) wgt = ai / aj, axis = 1;
                    else wgt = aj / ai, axis = -CN_MW;
                }
                const float rest = 1.0f - wgt;
                const float plus = M[diag] * wgt + M[axis] * rest;
                const float minus = M[-diag] * wgt + M[-axis] * rest;
                if (plus <= m && minus <= m) cls = m >= a.hi ? 2 : 1;
            }
        }
        a.cls[plane + (size_t)gy * a.w + gx] = cls;
    }
}

// ---------------------------------------------------------------- stage 3

// floods g along the runs of p inside one word, both ways
__device__ __forceinline__ unsigned int canny_fill(unsigned int g, unsigned int p)
{
    unsigned int u = g, q = p;
    u |= q & (u << 1), q &= q << 1;
    u |= q & (u << 2), q &= q << 2;
    u |= q & (u << 4), q &= q << 4;
    u |= q & (u << 8), q &= q << 8;
    u |= q & (u << 16);
    q = p;
    u |= q & (u >> 1), q &= q >> 1;
    u |= q & (u >> 2), q &= q >> 2;
    u |= q & (u >> 4), q &= q >> 4;
    u |= q & (u >> 8), q &= q >> 8;
    u |= q & (u >> 16);
    return u;
}

__device__ __forceinline__ unsigned int canny_ld(const unsigned int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void canny_st(unsigned int *p, unsigned int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

template <bool kLds>
__global__ __launch_bounds__(CN_HYST_THREADS) void k_canny_hyst(const CannyDev a)
{
    extern __shared__ unsigned int sBits[];
    const int b = blockIdx.x, n = a.h * a.wpr, wpr = a.wpr;
    unsigned int *C = kLds ? sBits : a.bits + (size_t)b * 2 * n;
    unsigned int *S = C + n;
    const unsigned char *cls = a.cls + (size_t)b * a.hw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunks = (a.w + 63) >> 6;
    for (int i = wave; i < a.h * chunks; i += CN_HYST_THREADS / 64) {     // wave-uniform: 64 pixels of a row per ballot
        const int r = i / chunks, c = i - r * chunks, x = c * 64 + lane;
        const unsigned char v = x < a.w ? cls[(size_t)r * a.w + x] : 0;
        const unsigned long long mc = __ballot(v == 1 || v == 2), ms = __ballot(v == 2);
        if (lane == 0) {
            const int o = r * wpr + 2 * c;
            C[o] = (unsigned int)mc, S[o] = (unsigned int)ms;
            if (2 * c + 1 < wpr) C[o + 1] = (unsigned int)(mc >> 32), S[o + 1] = (unsigned int)(ms >> 32);
        }
    }
    __syncthreads();
    for (int sweep = 0; sweep < a.hw; ++sweep) {
        int changed = 0;
        for (int i = threadIdx.x; i < n; i += CN_HYST_THREADS) {
            const unsigned int c = C[i];
            const unsigned int s = canny_ld(S + i);
            if (s == c) continue;                                         // nothing left to turn on (c == 0 included)
            const int r = i / wpr, j = i - r * wpr;
            unsigned int d = 0;
            for (int dr = -1; dr <= 1; ++dr) {
                const int rr = r + dr;
                if (rr < 0 || rr >= a.h) continue;
                const unsigned int *row = S + rr * wpr + j;
                const unsigned int m = canny_ld(row);
                const unsigned int l = j > 0 ? canny_ld(row - 1) : 0u, rt = j + 1 < wpr ? canny_ld(row + 1) : 0u;
                d |= m | (m << 1) | (m >> 1) | (l >> 31) | (rt << 31);
            }
            const unsigned int t = canny_fill(s | (c & d), c);
            if (t != s) canny_st(S + i, t), changed = 1;
        }
        if (!__syncthreads_or(changed)) break;                            // uniform
    }
    float *out = a.out + (size_t)b * a.hw;
    for (int p = threadIdx.x; p < a.hw; p += CN_HYST_THREADS) {
        const int r = p / a.w, x = p - r * a.w;
        out[p] = (S[r * wpr + (x >> 5)] >> (x & 31)) & 1u ? 1.0f : 0.0f;
    }
}

// ---------------------------------------------------------------- launcher

static int canny_shape(int B, int h, int w, const char *who)
{
    MPF_REQUIRE(B >= 1 && B <= 65535, "%s: bad shape: B must be 1..65535 (got %d)", who, B);
    MPF_REQUIRE(h >= 1 && w >= 1, "%s: bad shape: h, w must be at least 1 (got h, w = %d, %d)", who, h, w);
    MPF_REQUIRE((int64_t)B * h * w <= MPF_CANNY_MAX_BHW, "%s: bad shape: B * h * w must be at most %d (got B, h, w = %d, %d, %d)", who, MPF_CANNY_MAX_BHW, B, h, w);
    return 0;
}

static size_t canny_cls_offset(int B, int h, int w) { return (size_t)B * h * w * 4; }
static size_t canny_bits_offset(int B, int h, int w) { return canny_cls_offset(B, h, w) + (((size_t)B * h * w + 3) & ~(size_t)3); }

extern "C" size_t mpf_canny_workspace(int B, int h, int w)
{
    if (canny_shape(B, h, w, "mpf_canny_workspace")) return 0;
    return canny_bits_offset(B, h, w) + (size_t)B * 2 * h * ((w + 31) / 32) * 4;
}

static bool canny_overlap(const void *p, size_t pn, const void *q, size_t qn)
{
    const char *a = (const char *)p, *b = (const char *)q;
    return a && b && a < b + qn && b < a + pn;
}

extern "C" int mpf_canny(const MpfCannyArgs *a, void *stream)
{
    const char *who = "mpf_canny";
    MPF_REQUIRE(a, "%s: null argument block", who);
    const int rc = canny_shape(a->B, a->h, a->w, who);
    if (rc) return rc;
    MPF_REQUIRE(a->passes >= MPF_CANNY_PASS_ALL && a->passes <= MPF_CANNY_PASS_HYSTERESIS, "%s: passes must be 0..3 (got %d)", who, a->passes);
    const bool all = a->passes == MPF_CANNY_PASS_ALL;
    const bool smooth = all || a->passes == MPF_CANNY_PASS_SMOOTH, classify = all || a->passes == MPF_CANNY_PASS_CLASSIFY;
    const bool hyst = all || a->passes == MPF_CANNY_PASS_HYSTERESIS;
    MPF_REQUIRE(a->radius >= 0 && a->radius <= MPF_CANNY_MAX_RADIUS, "%s: radius must be 0..%d (got %d)", who, MPF_CANNY_MAX_RADIUS, a->radius);
    MPF_REQUIRE(a->low_threshold <= a->high_threshold, "%s: low_threshold must be at most high_threshold, neither NaN (got %g, %g)", who,
                (double)a->low_threshold, (double)a->high_threshold);
    MPF_REQUIRE(!smooth || a->gray, "%s: null pointer (gray)", who);
    MPF_REQUIRE(!(smooth || classify) || a->mask, "%s: null pointer (mask)", who);
    MPF_REQUIRE(!hyst || a->out, "%s: null pointer (out)", who);
    MPF_REQUIRE(a->workspace, "%s: null pointer (workspace)", who);
    MPF_REQUIRE((((uintptr_t)a->workspace) & 3) == 0, "%s: workspace must be 4-byte aligned", who);
    const size_t need = mpf_canny_workspace(a->B, a->h, a->w);
    MPF_REQUIRE(a->workspace_bytes >= need, "%s: workspace holds %zu bytes, %zu needed (mpf_canny_workspace)", who, a->workspace_bytes, need);
    const size_t nb = (size_t)a->B * a->h * a->w * 4;
    MPF_REQUIRE(!canny_overlap(a->out, nb, a->gray, nb) && !canny_overlap(a->out, nb, a->mask, nb) && !canny_overlap(a->out, nb, a->workspace, need) &&
                !canny_overlap(a->gray, nb, a->workspace, need) && !canny_overlap(a->mask, nb, a->workspace, need),
                "%s: out and the workspace must not overlap gray, mask or each other (a pixel reads its neighbours)", who);
    CannyDev d = CannyDev{};
    char *ws = (char *)a->workspace;
    d.gray = a->gray, d.mask = a->mask, d.out = a->out;
    d.smoothed = (float *)ws, d.cls = (unsigned char *)(ws + canny_cls_offset(a->B, a->h, a->w));
    d.bits = (unsigned int *)(ws + canny_bits_offset(a->B, a->h, a->w));
    d.h = a->h, d.w = a->w, d.hw = a->h * a->w, d.r = a->radius, d.wpr = (a->w + 31) / 32;
    d.tiles_x = (a->w + CN_TW - 1) / CN_TW;
    d.lo = a->low_threshold, d.hi = a->high_threshold;
    for (int k = 0; k <= 2 * a->radius; ++k) d.wt[k] = a->weights[k];
    const dim3 tiles((unsigned)(d.tiles_x * ((a->h + CN_TH - 1) / CN_TH)), (unsigned)a->B);
    if (smooth) {
        const int IW = CN_TW + 2 * d.r, IH = CN_TH + 2 * d.r;
        const size_t lds = (size_t)(2 * IH * IW + 2 * CN_TH * IW) * sizeof(float);      // 48 KiB at the bound
        hipLaunchKernelGGL(k_canny_smooth, tiles, dim3(CN_THREADS), lds, (hipStream_t)stream, d);
        const int st = mpf_launch_status("k_canny_smooth");
        if (st) return st;
    }
    if (classify) {
        hipLaunchKernelGGL(k_canny_classify, tiles, dim3(CN_THREADS), 0, (hipStream_t)stream, d);
        const int st = mpf_launch_status("k_canny_classify");
        if (st) return st;
    }
    if (hyst) {
        const int n = d.h * d.wpr;
        if (n <= MPF_CANNY_LDS_WORDS)
            hipLaunchKernelGGL(k_canny_hyst<true>, dim3((unsigned)a->B), dim3(CN_HYST_THREADS), (size_t)2 * n * sizeof(unsigned int), (hipStream_t)stream, d);
        else
            hipLaunchKernelGGL(k_canny_hyst<false>, dim3((unsigned)a->B), dim3(CN_HYST_THREADS), 0, (hipStream_t)stream, d);
        return mpf_launch_status("k_canny_hyst");
    }
    return 0;
}
