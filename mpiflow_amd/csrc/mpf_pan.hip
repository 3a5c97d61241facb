// mpf_pan.hip - the first residual block of AdaMPI's plane-adjustment network (model/PAN.py:18-46) over the S plane-images of an image, with its
// 2 x 2 average pool, for gfx950.  Eval mode, float32, no gradient.
//
// Contract: include/mpiflow_hip.h (MpfPanArgs); INTEGRATION.md section 23 holds the definitions, which tests/pan_restated.py restates in float64.
// The build has no contraction: every fused multiply-add below is written as fmaf, every other operation is rounded on its own.
//
// The S inputs of an image differ in one constant channel d_s, and conv1 / conv3 are affine in it:
//   conv1(x_s) = A1 + d_s * B1,  conv3(x_s) = A3 + d_s * w3[:,4]
// with A1, A3 per image and B1 per size (zero padding makes the constant channel's response position-dependent on the one-pixel border).
//
// k_pan_maps    the prologue: one thread per pixel writes the 8 channels of A1 and A3 of its image, and (blockIdx.y = 0) of B1.
// k_pan_block1  one workgroup owns a tile of PAN_PH x PAN_PW pooled pixels (2 PAN_PH x 2 PAN_PW before the pool) and walks
//               MPF_PAN_PLANES_PER_GROUP planes of one image over it.  Each thread keeps its PAN_SLOTS elements of the tile's A1 and B1 with a
//               one-pixel halo, and the A3 of its 2 x 2 pixels, in registers for all its planes.  Per plane it writes m = bn(relu(A1 + d_s * B1)),
//               or 0 for a halo pixel outside the frame - conv2 pads its own input, which is m, with zeros - into the LDS tile [8][PAN_TH][PAN_TW];
//               then a thread is one pooled pixel and half of the output channels: it reads its 4 x 4 window of every input channel as eight
//               8-byte LDS reads (a pooled row of 32 threads covers the 64 banks once: no conflicts), runs the 8 -> 4 channels 3 x 3 over its
//               2 x 2 pixels with the weights in scalar registers (the channel half is wave-uniform), adds b2 + A3 + d_s * w3[:,4], applies the
//               ReLU, averages and stores.  Lanes run along x: the stores coalesce.
// A pooled pixel past h / 2 or w / 2 (a partial tile; the dropped odd row / column) is computed from the zero-filled tile and not stored; every
// global read is checked against the frame first.  No workgroup waits for another; every loop has a constant bound or is bounded by S.
#include "mpf_common.h"
#include <math.h>

#define PAN_C MPF_PAN_C
#define PAN_PG MPF_PAN_PLANES_PER_GROUP
#define PAN_THREADS 256
#define PAN_PH 4                                              // pooled rows of a tile
#define PAN_PW 32                                             // pooled columns of a tile: one 32-lane half of a wave
#define PAN_TH (2 * PAN_PH + 2)                               // tile rows with the halo
#define PAN_TW (2 * PAN_PW + 2)                               // tile columns with the halo; even: the 8-byte LDS reads stay aligned
#define PAN_TILE (PAN_C * PAN_TH * PAN_TW)
#define PAN_SLOTS ((PAN_TILE + PAN_THREADS - 1) / PAN_THREADS)

static_assert(PAN_THREADS == 2 * PAN_PH * PAN_PW, "a thread is one pooled pixel and one half of the output channels");
static_assert(PAN_TW % 2 == 0 && (PAN_TH * PAN_TW) % 2 == 0, "8-byte LDS reads");

struct PanDev {
    const float *rgb, *disp, *plane_disp, *w1, *b1, *scale, *shift, *w2, *b2, *w3, *b3;
    float *A1, *A3, *B1, *out;
    int S, h, w, hp, wp, groups;
};

__global__ __launch_bounds__(PAN_THREADS) void k_pan_maps(const PanDev a)
{
    const int hw = a.h * a.w;
    const int p = (int)(blockIdx.x * PAN_THREADS + threadIdx.x);
    if (p >= hw) return;
    const int b = (int)blockIdx.y;
    const int y = p / a.w, x = p - y * a.w;
    const float *src[4] = {a.rgb + (size_t)b * 3 * hw, a.rgb + (size_t)b * 3 * hw + hw, a.rgb + (size_t)b * 3 * hw + 2 * hw, a.disp + (size_t)b * hw};
    float v[4][9];
    bool in[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        in[t] = yy >= 0 && yy < a.h && xx >= 0 && xx < a.w;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c][t] = in[t] ? src[c][yy * a.w + xx] : 0.0f;
    }
    float *A1 = a.A1 + (size_t)b * PAN_C * hw + p, *A3 = a.A3 + (size_t)b * PAN_C * hw + p;
#pragma unroll
    for (int o = 0; o < PAN_C; ++o) {
        float s1 = a.b1[o], s3 = a.b3[o], sb = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int t = 0; t < 9; ++t) s1 = fmaf(a.w1[(o * 5 + c) * 9 + t], v[c][t], s1);
            s3 = fmaf(a.w3[o * 5 + c], v[c][4], s3);
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) sb += in[t] ? a.w1[(o * 5 + 4) * 9 + t] : 0.0f;
        A1[(size_t)o * hw] = s1;
        A3[(size_t)o * hw] = s3;
        if (b == 0) a.B1[(size_t)o * hw + p] = sb;
    }
}

__global__ __launch_bounds__(PAN_THREADS) void k_pan_block1(const PanDev a)
{
    __shared__ __attribute__((aligned(16))) float m[PAN_TILE];
    __shared__ float bn[2 * PAN_C];                                                                // the folded BatchNorm: scale, then shift
    const int tid = (int)threadIdx.x;
    const int hw = a.h * a.w;
    const int b = (int)blockIdx.z / a.groups, g = (int)blockIdx.z - b * a.groups;
    const int y0 = (int)blockIdx.y * 2 * PAN_PH - 1, x0 = (int)blockIdx.x * 2 * PAN_PW - 1;        // frame position of the tile's element [0][0]
    const float *A1 = a.A1 + (size_t)b * PAN_C * hw, *A3 = a.A3 + (size_t)b * PAN_C * hw;

    if (tid < 2 * PAN_C) bn[tid] = tid < PAN_C ? a.scale[tid] : a.shift[tid - PAN_C];             // read after the plane loop's first barrier
    // this thread's elements of the tile: A1 and B1; `inside`: bit k = element k lies in the frame
    float ra[PAN_SLOTS], rb[PAN_SLOTS];
    unsigned inside = 0;
#pragma unroll
    for (int k = 0; k < PAN_SLOTS; ++k) {
        const int e = tid + k * PAN_THREADS;
        const int c = e / (PAN_TH * PAN_TW), r = e - c * (PAN_TH * PAN_TW);
        const int y = y0 + r / PAN_TW, x = x0 + r % PAN_TW;
        const bool ok = e < PAN_TILE && y >= 0 && y < a.h && x >= 0 && x < a.w;
        ra[k] = ok ? A1[(size_t)c * hw + y * a.w + x] : 0.0f;
        rb[k] = ok ? a.B1[(size_t)c * hw + y * a.w + x] : 0.0f;
        inside |= ok ? 1u << k : 0u;
    }

    const int half = __builtin_amdgcn_readfirstlane(tid >> 7);                                     // waves 0, 1: channels 0..3; waves 2, 3: 4..7
    const int q = tid & 127, qy = q >> 5, qx = q & 31;                                             // pooled pixel of the tile
    const int py = (int)blockIdx.y * PAN_PH + qy, px = (int)blockIdx.x * PAN_PW + qx;              // pooled pixel of the frame
    const bool live = py < a.hp && px < a.wp;
    float r3[4][4];                                                                                // A3 [channel of the half][2 x 2 pixel]
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int i = 0; i < 4; ++i) r3[o][i] = live ? A3[(size_t)(half * 4 + o) * hw + (2 * py + (i >> 1)) * a.w + 2 * px + (i & 1)] : 0.0f;

    const float *w2 = a.w2 + half * 4 * PAN_C * 9;
    const int s_end = min(a.S, (g + 1) * PAN_PG);
    for (int s = g * PAN_PG; s < s_end; ++s) {
        const float d = a.plane_disp[(size_t)b * a.S + s];
        __syncthreads();                                                                           // the previous plane's reads of m are done
#pragma unroll
        for (int k = 0; k < PAN_SLOTS; ++k) {
            const int e = tid + k * PAN_THREADS;
            const int c = min(e / (PAN_TH * PAN_TW), PAN_C - 1);                                   // the last slot runs past the tile: stay inside bn
            if (e < PAN_TILE) m[e] =(inside >> k) & 1u ? fmaf(bn[c], fmaxf(fmaf(d, rb[k], ra[k]), 0.0f), bn[PAN_C + c]) : 0.0f;
        }
        __syncthreads();
        float acc[4][4];
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[o][i] = 0.0f;
#pragma unroll 2
        for (int c = 0; c < PAN_C; ++c) {
            float win[4][4];                                                                       // rows 2 qy .. 2 qy + 3, columns 2 qx .. 2 qx + 3 of the tile
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float2 *row = reinterpret_cast<const float2 *>(m + (c * PAN_TH + 2 * qy + r) * PAN_TW + 2 * qx);
                const float2 lo = row[0], hi = row[1];
                win[r][0] = lo.x; win[r][1] = lo.y; win[r][2] = hi.x; win[r][3] = hi.y;
            }
#pragma unroll
            for (int o = 0; o < 4; ++o)
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const float wt = w2[(o * PAN_C + c) * 9 + t];
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[o][i] = fmaf(wt, win[(i >> 1) + t / 3][(i & 1) + t % 3], acc[o][i]);
                }
        }
        if (live) {
            float *out = a.out + (((size_t)b * a.S + s) * PAN_C + half * 4) * a.hp * a.wp + (size_t)py * a.wp + px;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const float k = fmaf(d, a.w3[(half * 4 + o) * 5 + 4], a.b2[half * 4 + o]);
                float sum = 0.0f;
#pragma unroll
                for (int i = 0; i < 4; ++i) sum += fmaxf((acc[o][i] + r3[o][i]) + k, 0.0f);
                out[(size_t)o * a.hp * a.wp] = sum * 0.25f;
            }
        }
    }
}

static bool pan_shape_ok(int B, int S, int h, int w)
{
    if (B < 1 || S < 1 || h < 2 || w < 2) return false;
    const int64_t hp = h / 2, wp = w / 2, groups = (S + PAN_PG - 1) / PAN_PG;
    return (int64_t)B * S * PAN_C * hp * wp < ((int64_t)1 << 31) && (int64_t)B * PAN_C * h * w < ((int64_t)1 << 31) && (hp + PAN_PH - 1) / PAN_PH <= 65535 &&
           (int64_t)B * groups <= 65535 && B <= 65535;
}

extern "C" size_t mpf_pan_block1_workspace(int B, int h, int w)
{
    if (!pan_shape_ok(B, 1, h, w)) return 0;
    return (size_t)(2 * B + 1) * PAN_C * h * w * sizeof(float);
}

extern "C" int mpf_pan_block1(const MpfPanArgs *a, void *stream)
{
    const char *who = "mpf_pan_block1";
    MPF_REQUIRE(a, "%s: null argument block", who);
    MPF_REQUIRE(a->rgb_low && a->disp_low && a->plane_disp && a->out, "%s: null pointer (rgb_low, disp_low, plane_disp, out)", who);
    MPF_REQUIRE(a->w1 && a->b1 && a->bn_scale && a->bn_shift && a->w2 && a->b2 && a->w3 && a->b3, "%s: null pointer (w1, b1, bn_scale, bn_shift, w2, b2, w3, b3)", who);
    MPF_REQUIRE(a->h >= 2 && a->w >= 2, "%s: h and w must be at least 2 (got h, w = %d, %d): the 2 x 2 pool leaves nothing of a smaller map", who, a->h, a->w);
    MPF_REQUIRE(a->B >= 1 && a->S >= 1, "%s: B and S must be at least 1 (got B, S = %d, %d)", who, a->B, a->S);
    MPF_REQUIRE(pan_shape_ok(a->B, a->S, a->h, a->w),
                "%s: bad shape: B * S * 8 * (h / 2) * (w / 2) and B * 8 * h * w below 2^31, at most 65535 row tiles and 65535 (image, plane group) slices "
                "(got B, S, h, w = %d, %d, %d, %d)", who, a->B, a->S, a->h, a->w);
    const void *ptrs[] = {a->rgb_low, a->disp_low, a->plane_disp, a->w1, a->b1, a->bn_scale, a->bn_shift, a->w2, a->b2, a->w3, a->b3, a->out, a->workspace};
    for (const void *p : ptrs) MPF_REQUIRE(((uintptr_t)p & 3) == 0, "%s: every pointer must be 4-byte aligned (got %p)", who, p);
    const size_t need = mpf_pan_block1_workspace(a->B, a->h, a->w);
    MPF_REQUIRE(a->workspace && a->workspace_bytes >= need, "%s: workspace of %zu bytes needed for the shared maps A1, A3, B1 (got %zu)", who, need, a->workspace_bytes);
    const size_t hw = (size_t)a->h * a->w;
    PanDev d;
    d.rgb = a->rgb_low; d.disp = a->disp_low; d.plane_disp = a->plane_disp; d.w1 = a->w1; d.b1 = a->b1; d.scale = a->bn_scale; d.shift = a->bn_shift;
    d.w2 = a->w2; d.b2 = a->b2; d.w3 = a->w3; d.b3 = a->b3; d.out = a->out;
    d.A1 = (float *)a->workspace; d.A3 = d.A1 + (size_t)a->B * PAN_C * hw; d.B1 = d.A3 + (size_t)a->B * PAN_C * hw;
    d.S = a->S; d.h = a->h; d.w = a->w; d.hp = a->h / 2; d.wp = a->w / 2; d.groups = (a->S + PAN_PG - 1) / PAN_PG;
    hipLaunchKernelGGL(k_pan_maps, dim3((unsigned)((hw + PAN_THREADS - 1) / PAN_THREADS), (unsigned)a->B), dim3(PAN_THREADS), 0, (hipStream_t)stream, d);
    const int st = mpf_launch_status("k_pan_maps");
    if (st) return st;
    const dim3 grid((unsigned)((d.wp + PAN_PW - 1) / PAN_PW), (unsigned)((d.hp + PAN_PH - 1) / PAN_PH), (unsigned)(a->B * d.groups));
    hipLaunchKernelGGL(k_pan_block1, grid, dim3(PAN_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_pan_block1");
}
