// mpf_corr.hip - RAFT's on-demand correlation lookup (RAFT/alt_cuda_corr; AlternateCorrBlock of RAFT/core/corr.py:63-91) for gfx950.
//
// Contract: include/mpiflow_hip.h (MpfCorrArgs).  Per query pixel and pyramid level the lookup needs the (rd+1)^2 dot products of the pixel's
// fmap1 vector with the fmap2 vectors on the integer grid around (floor x, floor y) ("the grid", D below); the rd^2 outputs are four-tap
// blends of D with ONE pair of fractions (every tap of a window shares the centre's fraction).  The gradient runs the same two steps
// backwards: the cotangent is spread onto the grid (gD), then grad_fmap1 = sum gD * f2 (a per-pixel sum) and grad_f2 += gD * fmap1 (a scatter).
//
// k_corr_forward   grid (tiles of 16 query pixels, levels), 256 threads.  A wave owns 4 pixels of the tile, one after the other.  Lane =
//                  (g, l): 8 groups of 8 lanes; a group owns one grid point at a time and its 8 lanes cover 32 channels with one 16-byte load
//                  each, so one wave-instruction fetches 8 grid points x 128 contiguous bytes.  Each lane carries 13 accumulators (104 >= the
//                  100 grid points of radius 4: one pass over C; larger radii take more passes), so 13 independent loads are in flight per
//                  lane and the cross-lane sum costs 3 shuffles per 13 * C/8 fused multiply-adds.  D goes to LDS, the wave blends it, and
//                  the tile's outputs leave through LDS as 64-byte runs along x.
// k_corr_backward  one wave per query pixel, all levels (so grad_fmap1 is a plain sum in a fixed order, written once).  Lane = (g, l): 2
//                  groups of 32 lanes, one channel per lane: an atomic wave-instruction adds two 128-byte row segments.  Per 32 channels:
//                  first every load (sum into grad_fmap1's accumulator), then every atomic, so that no load waits behind an atomic.
// k_corr_plain     the formula as it stands, one thread per output entry (MpfCorrArgs.plain).
//
// Untrusted coordinates: corr_axis() (mpf_corr_common.h) is the only place a coordinate becomes an integer.  It compares in floating point first (NaN fails
// both comparisons), so the integer it returns lies in [-(2r+2), n+1] whatever the input, and every grid point is tested against the level's
// bounds before its address is formed.
#include "mpf_common.h"
#include "mpf_corr_common.h"

#define CORR_TILE 16             // query pixels per block of k_corr_forward
#define CORR_THREADS 256
#define CORR_NACC 13             // grid points per group and pass
#define CORR_MAX_RD1 18          // 2 * 8 + 2

struct CorrDev {
    const float *fmap1;
    const float *f2[MPF_CORR_MAX_LEVELS];
    const float *coords;
    float *out;
    float *grad_fmap1;
    float *grad_f2[MPF_CORR_MAX_LEVELS];
    int B, C, H, W;
    int Hl[MPF_CORR_MAX_LEVELS], Wl[MPF_CORR_MAX_LEVELS];
    int radius, levels;
    float scale;
};

__global__ __launch_bounds__(CORR_THREADS) void k_corr_forward(const CorrDev a)
{
    __shared__ float sD[CORR_THREADS / 64][CORR_MAX_RD1 * CORR_MAX_RD1 + 4];
    __shared__ float sOut[(2 * 8 + 1) * (2 * 8 + 1)][CORR_TILE + 1];
    const int lvl = blockIdx.y;
    const int r = a.radius, rd = 2 * r + 1, rd1 = rd + 1, npts = rd1 * rd1;
    const int HW = a.H * a.W;
    const long long NP = (long long)a.B * HW;
    const long long tile0 = (long long)blockIdx.x * CORR_TILE;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 3, l = lane & 7;
    const int Hl = a.Hl[lvl], Wl = a.Wl[lvl], C = a.C;
    const float *__restrict__ f2 = a.f2[lvl];
    const float inv = 1.0f / (float)(1 << lvl);

    for (int pp = 0; pp < CORR_TILE / 4; ++pp) {
        const int pt = wave * (CORR_TILE / 4) + pp;
        const long long pix = tile0 + pt;
        const bool live = pix < NP;                          // wave-uniform
        int x0 = -(2 * r + 2), y0 = -(2 * r + 2), b = 0;
        float fx = 0.0f, fy = 0.0f;
        if (live) {
            b = (int)(pix / HW);
            const int yx = (int)(pix - (long long)b * HW);
            corr_axis(a.coords[((long long)b * 2 + 0) * HW + yx], inv, Wl, r, x0, fx);
            corr_axis(a.coords[((long long)b * 2 + 1) * HW + yx], inv, Hl, r, y0, fy);
        }
        const float *__restrict__ f1 = a.fmap1 + (live ? pix : 0) * C;
        for (int t0 = 0; t0 < npts; t0 += 8 * CORR_NACC) {
            int off[CORR_NACC];
            bool in[CORR_NACC];
            float acc[CORR_NACC];
#pragma unroll
            for (int u = 0; u < CORR_NACC; ++u) {
                const int t = t0 + g + 8 * u;
                const int jy = t / rd1, jx = t - jy * rd1;
                const int ix = x0 + jx, iy = y0 + jy;
                in[u] = live && t < npts && (unsigned)ix < (unsigned)Wl && (unsigned)iy < (unsigned)Hl;
                off[u] = in[u] ? (((b * Hl + iy) * Wl + ix) * C) : 0;      // outside: a legal address whose sum is discarded
                acc[u] = 0.0f;
            }
            for (int ch = 4 * l; ch < C; ch += 32) {
                const float4 p = *(const float4 *)(f1 + ch);
#pragma unroll
                for (int u = 0; u < CORR_NACC; ++u) {
                    const float4 q = *(const float4 *)(f2 + off[u] + ch);
                    acc[u] = fmaf(p.x, q.x, acc[u]);
                    acc[u] = fmaf(p.y, q.y, acc[u]);
                    acc[u] = fmaf(p.z, q.z, acc[u]);
                    acc[u] = fmaf(p.w, q.w, acc[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < CORR_NACC; ++u) {
                float v = in[u] ? acc[u] : 0.0f;
                v += __shfl_xor(v, 1);
                v += __shfl_xor(v, 2);
                v += __shfl_xor(v, 4);
                const int t = t0 + g + 8 * u;
                if (l == 0 && t < npts) sD[wave][t] = v;
            }
        }
        __syncthreads();
        for (int o = lane; o < rd * rd; o += 64) {
            const int ai = o / rd, ci = o - ai * rd;             // ai moves x, ci moves y
            const float *d = &sD[wave][ci * rd1 + ai];
            sOut[o][pt] = a.scale * corr_blend(d[0], d[1], d[rd1], d[rd1 + 1], fx, fy);
        }
        __syncthreads();
    }
    const long long CH = (long long)a.levels * rd * rd;
    for (int idx = threadIdx.x; idx < rd * rd * CORR_TILE; idx += CORR_THREADS) {
        const int o = idx / CORR_TILE, pt = idx - o * CORR_TILE;
        const long long pix = tile0 + pt;
        if (pix < NP) {
            const long long b = pix / HW, yx = pix - b * HW;
            a.out[(b * CH + (long long)lvl * rd * rd + o) * HW + yx] = sOut[o][pt];
        }
    }
}

__global__ __launch_bounds__(CORR_THREADS) void k_corr_plain(const CorrDev a)
{
    const int r = a.radius, rd = 2 * r + 1;
    const int HW = a.H * a.W;
    const long long CH = (long long)a.levels * rd * rd;
    const long long total = (long long)a.B * CH * HW;
    const long long i = (long long)blockIdx.x * CORR_THREADS + threadIdx.x;
    if (i >= total) return;
    const int yx = (int)(i % HW);
    const int chn = (int)((i / HW) % CH);
    const int b = (int)(i / (HW * CH));
    const int lvl = chn / (rd * rd), o = chn - lvl * rd * rd, ai = o / rd, ci = o - ai * rd;
    const int Hl = a.Hl[lvl], Wl = a.Wl[lvl], C = a.C;
    const float inv = 1.0f / (float)(1 << lvl);
    int x0, y0;
    float fx, fy;
    corr_axis(a.coords[((long long)b * 2 + 0) * HW + yx], inv, Wl, r, x0, fx);
    corr_axis(a.coords[((long long)b * 2 + 1) * HW + yx], inv, Hl, r, y0, fy);
    const float *f1 = a.fmap1 + ((long long)b * HW + yx) * C;
    const float *f2 = a.f2[lvl];
    float d[2][2];
    for (int jy = 0; jy < 2; ++jy)
        for (int jx = 0; jx < 2; ++jx) {
            const int ix = x0 + ai + jx, iy = y0 + ci + jy;
            float s = 0.0f;
            if ((unsigned)ix < (unsigned)Wl && (unsigned)iy < (unsigned)Hl) {
                const float *q = f2 + ((long long)(b * Hl + iy) * Wl + ix) * C;
                for (int ch = 0; ch < C; ++ch) s = fmaf(f1[ch], q[ch], s);
            }
            d[jy][jx] = s;
        }
    a.out[i] = a.scale * corr_blend(d[0][0], d[0][1], d[1][0], d[1][1], fx, fy);
}

__global__ __launch_bounds__(CORR_THREADS) void k_corr_backward(const CorrDev a)
{
    extern __shared__ __align__(16) float sG[];              // [waves][levels][rd1*rd1]: the cotangent spread onto the grid, 0 outside the level
    __shared__ int sBase[CORR_THREADS / 64][MPF_CORR_MAX_LEVELS][2];
    const int r = a.radius, rd = 2 * r + 1, rd1 = rd + 1, npts = rd1 * rd1;
    const int HW = a.H * a.W, C = a.C, L = a.levels;
    const long long NP = (long long)a.B * HW;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 5, l = lane & 31;
    const long long pix = (long long)blockIdx.x * (CORR_THREADS / 64) + wave;
    const bool live = pix < NP;                              // wave-uniform
    const int b = live ? (int)(pix / HW) : 0;
    const int yx = live ? (int)(pix - (long long)b * HW) : 0;
    const long long CH = (long long)L * rd * rd;
    float *gw = sG + (size_t)wave * L * npts;

    for (int lvl = 0; lvl < L; ++lvl) {
        const int Hl = a.Hl[lvl], Wl = a.Wl[lvl];
        const float inv = 1.0f / (float)(1 << lvl);
        int x0 = -(2 * r + 2), y0 = -(2 * r + 2);
        float fx = 0.0f, fy = 0.0f;
        if (live) {
            corr_axis(a.coords[((long long)b * 2 + 0) * HW + yx], inv, Wl, r, x0, fx);
            corr_axis(a.coords[((long long)b * 2 + 1) * HW + yx], inv, Hl, r, y0, fy);
        }
        if (lane == 0) {
            sBase[wave][lvl][0] = x0;
            sBase[wave][lvl][1] = y0;
        }
        const float gx = 1.0f - fx, gy = 1.0f - fy;
        const float *go = a.out + ((long long)b * CH + (long long)lvl * rd * rd) * HW + yx;
        for (int t = lane; t < npts; t += 64) {
            const int jy = t / rd1, jx = t - jy * rd1;
            const int ix = x0 + jx, iy = y0 + jy;
            float s = 0.0f;
            if (live && (unsigned)ix < (unsigned)Wl && (unsigned)iy < (unsigned)Hl) {
                // grid point (jy, jx) is tap d00 of output (a = jx, c = jy), d01 of (jx - 1, jy), d10 of (jx, jy - 1), d11 of (jx - 1, jy - 1)
                if (jx < rd && jy < rd) s = (gx * gy) * go[(long long)(jx * rd + jy) * HW];
                if (jx > 0 && jy < rd) s = fmaf(fx * gy, go[(long long)((jx - 1) * rd + jy) * HW], s);
                if (jx < rd && jy > 0) s = fmaf(gx * fy, go[(long long)(jx * rd + jy - 1) * HW], s);
                if (jx > 0 && jy > 0) s = fmaf(fx * fy, go[(long long)((jx - 1) * rd + jy - 1) * HW], s);
                s *= a.scale;
            }
            gw[lvl * npts + t] = s;
        }
    }
    __syncthreads();
    if (!live) return;
    const float *__restrict__ f1 = a.fmap1 + pix * C;
    for (int ch = l; ch < C; ch += 32) {
        const float p = f1[ch];
        float acc = 0.0f;
        for (int lvl = 0; lvl < L; ++lvl) {
            const int Hl = a.Hl[lvl], Wl = a.Wl[lvl];
            const int x0 = sBase[wave][lvl][0], y0 = sBase[wave][lvl][1];
            const float *__restrict__ f2 = a.f2[lvl];
            for (int jy = 0; jy < rd1; ++jy) {
                const int iy = y0 + jy;
                if ((unsigned)iy >= (unsigned)Hl) continue;
#pragma unroll 5
                for (int jx = g; jx < rd1; jx += 2) {
                    const int ix = x0 + jx;
                    const float w = gw[lvl * npts + jy * rd1 + jx];
                    if ((unsigned)ix < (unsigned)Wl) acc = fmaf(w, f2[((b * Hl + iy) * Wl + ix) * C + ch], acc);
                }
            }
        }
        for (int lvl = 0; lvl < L; ++lvl) {
            const int Hl = a.Hl[lvl], Wl = a.Wl[lvl];
            const int x0 = sBase[wave][lvl][0], y0 = sBase[wave][lvl][1];
            float *g2 = a.grad_f2[lvl];
            for (int jy = 0; jy < rd1; ++jy) {
                const int iy = y0 + jy;
                if ((unsigned)iy >= (unsigned)Hl) continue;
                for (int jx = g; jx < rd1; jx += 2) {
                    const int ix = x0 + jx;
                    const float w = gw[lvl * npts + jy * rd1 + jx];
                    if ((unsigned)ix < (unsigned)Wl && w != 0.0f) atomicAdd(g2 + ((b * Hl + iy) * Wl + ix) * C + ch, w * p);
                }
            }
        }
        acc += __shfl_xor(acc, 32);
        if (g == 0) a.grad_fmap1[pix * C + ch] = acc;
    }
}

static int corr_check(const MpfCorrArgs *a, bool backward, const char *who, CorrDev &d)
{
    MPF_REQUIRE(a, "%s: null argument block", who);
    MPF_REQUIRE(a->fmap1 && a->coords && a->out, "%s: null pointer (fmap1, coords or out)", who);
    MPF_REQUIRE(a->levels >= 1 && a->levels <= MPF_CORR_MAX_LEVELS, "%s: levels must be 1..%d (got %d)", who, MPF_CORR_MAX_LEVELS, a->levels);
    MPF_REQUIRE(a->radius >= 1 && a->radius <= 8, "%s: radius must be 1..8 (got %d)", who, a->radius);
    MPF_REQUIRE(a->C >= 32 && a->C % 32 == 0, "%s: C must be a multiple of 32 (got %d)", who, a->C);
    MPF_REQUIRE(a->B >= 1 && a->H >= 1 && a->W >= 1, "%s: bad shape B, H, W = %d, %d, %d", who, a->B, a->H, a->W);
    const int64_t lim = (int64_t)1 << 31;
    const int rd = 2 * a->radius + 1;
    MPF_REQUIRE((int64_t)a->B * a->H * a->W * a->C < lim, "%s: fmap1 must hold fewer than 2^31 elements", who);
    MPF_REQUIRE((int64_t)a->B * a->H * a->W < lim / (CORR_THREADS * 2), "%s: B * H * W too large", who);
    MPF_REQUIRE((int64_t)a->B * a->levels * rd * rd * a->H * a->W < ((int64_t)1 << 40), "%s: output too large", who);
    MPF_REQUIRE(mpf_aligned16(a->fmap1), "%s: fmap1 must be 16-byte aligned", who);
    MPF_REQUIRE(a->scale == a->scale && a->scale - a->scale == 0.0f, "%s: scale must be finite", who);
    MPF_REQUIRE(a->plain == 0 || a->plain == 1, "%s: plain must be 0 or 1", who);
    if (backward) MPF_REQUIRE(a->grad_fmap1, "%s: null pointer (grad_fmap1)", who);
    d = CorrDev{};
    for (int i = 0; i < a->levels; ++i) {
        MPF_REQUIRE(a->f2[i], "%s: null pointer (f2[%d])", who, i);
        MPF_REQUIRE(mpf_aligned16(a->f2[i]), "%s: f2[%d] must be 16-byte aligned", who, i);
        MPF_REQUIRE(a->Hl[i] >= 2 && a->Wl[i] >= 2,
                    "%s: Hl[%d] x Wl[%d] = %d x %d: every level must be at least 2 x 2 (H, W >= 2^levels for a pooled pyramid)", who, i, i, a->Hl[i],
                    a->Wl[i]);
        MPF_REQUIRE((int64_t)a->B * a->Hl[i] * a->Wl[i] * a->C < lim, "%s: f2[%d] must hold fewer than 2^31 elements", who, i);
        if (backward) MPF_REQUIRE(a->grad_f2[i], "%s: null pointer (grad_f2[%d])", who, i);
        d.f2[i] = a->f2[i];
        d.grad_f2[i] = a->grad_f2[i];
        d.Hl[i] = a->Hl[i];
        d.Wl[i] = a->Wl[i];
    }
    d.fmap1 = a->fmap1;
    d.coords = a->coords;
    d.out = a->out;
    d.grad_fmap1 = a->grad_fmap1;
    d.B = a->B, d.C = a->C, d.H = a->H, d.W = a->W;
    d.radius = a->radius, d.levels = a->levels, d.scale = a->scale;
    return 0;
}

extern "C" int mpf_corr_lookup(const MpfCorrArgs *a, void *stream)
{
    CorrDev d;
    const int rc = corr_check(a, false, "mpf_corr_lookup", d);
    if (rc) return rc;
    const int64_t NP = (int64_t)d.B * d.H * d.W;
    if (a->plain) {
        const int rd = 2 * d.radius + 1;
        const int64_t total = NP * d.levels * rd * rd;
        MPF_REQUIRE((total + CORR_THREADS - 1) / CORR_THREADS < ((int64_t)1 << 31), "mpf_corr_lookup: output too large for plain = 1");
        hipLaunchKernelGGL(k_corr_plain, dim3((unsigned)((total + CORR_THREADS - 1) / CORR_THREADS)), dim3(CORR_THREADS), 0, (hipStream_t)stream, d);
        return mpf_launch_status("k_corr_plain");
    }
    hipLaunchKernelGGL(k_corr_forward, dim3((unsigned)((NP + CORR_TILE - 1) / CORR_TILE), (unsigned)d.levels), dim3(CORR_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_corr_forward");
}

extern "C" int mpf_corr_lookup_backward(const MpfCorrArgs *a, void *stream)
{
    CorrDev d;
    const int rc = corr_check(a, true, "mpf_corr_lookup_backward", d);
    if (rc) return rc;
    const int64_t NP = (int64_t)d.B * d.H * d.W;
    const int waves = CORR_THREADS / 64, rd1 = 2 * d.radius + 2;
    const size_t lds = (size_t)waves * d.levels * rd1 * rd1 * sizeof(float);     // <= 4 * 6 * 324 * 4 = 31,104 bytes
    hipLaunchKernelGGL(k_corr_backward, dim3((unsigned)((NP + waves - 1) / waves)), dim3(CORR_THREADS), lds, (hipStream_t)stream, d);
    return mpf_launch_status("k_corr_backward");
}
