// mpf_upsample.hip - RAFT's convex upsampling (RAFT.upsample_flow, RAFT/core/raft.py:72-83) and the per-prediction term of its sequence loss
// (RAFT/train.py:47-72) for gfx950, fused: the loss entry points never write the full-resolution prediction.
//
// Contract: include/mpiflow_hip.h (MpfUpsampleArgs).  Per coarse pixel and sub-position (i, j) the op is a softmax over the 9 taps of the mask
// and a 9-term blend of the 3 x 3 neighbourhood of 8 * flow.  One kernel body, four modes:
//
// k_upsample<UP_FWD>       writes out.
// k_upsample<UP_BWD>       reads the cotangent, recomputes the softmax, writes grad_mask and the per-pixel tap sums T (below).
// k_upsample<UP_LOSS>      blends in registers, compares with flow_gt under the validity mask, leaves one partial sum (and five metric partials)
//                          per block; k_upsample_finish folds the partials in a fixed order in fp64.
// k_upsample<UP_LOSS_BWD>  forms the cotangent g / count * v * sign(out - flow_gt) in registers, then as UP_BWD.
//
// Layout: block = 256 threads = 4 waves over ONE tile of 64 consecutive coarse pixels of one sample (the flat index h * W + w, so a tile may
// span rows and W need not be a multiple of anything); lane = pixel, wave = the sub-rows 2 * wave and 2 * wave + 1.  A wave's read of one mask
// channel is then one 256-byte run, the eight floats a lane owns of an output row are two 16-byte accesses, and each of the 576 channels is
// read by exactly one wave, once.  A lane past the end of the sample works on the sample's last pixel and stores nothing.
//
// grad_flow without atomics: T[n, c, k, h, w] = sum_ij p[k,i,j] * cot[c,i,j] is what pixel (h, w) owes its neighbour (h + ky - 1, w + kx - 1).
// The four waves of a block fold their sub-rows through LDS in wave order and store T to the workspace; k_upsample_fold then GATHERS
// grad_flow[n,c,h,w] = 8 * sum_k T[n, c, k, h - ky + 1, w - kx + 1] in tap order.  Sums over (i, j) and over k are carried in fp64 and rounded
// once.  Every output is therefore bit-identical from run to run.
//
// No address depends on a tensor's values: NaN and inf travel through the arithmetic as they do in torch (fmaxf drops a NaN from the maximum,
// but the NaN's own exponential poisons the softmax sum all the same; 0 * inf and inf - inf give the NaN torch gives).
//
// The small model has no mask: its prediction is upflow8, 8 x bilinear with align_corners=True (mpf_raft_glue.hip).  The same loss term for it:
//
// k_up8_loss               a lane owns 4 consecutive fine pixels of one row: three float4 loads (flow_gt u, v; valid), the prediction formed in
//                          registers from the 64 x smaller coarse map (cache) with k_upflow8's own expression (up8_value, mpf_upflow8.h), compared and summed as
//                          UP_LOSS does; grid-stride over at most UP8_MAX_BLOCKS blocks, one partial row per block, folded by k_upsample_finish.
// k_up8_loss_bwd           a gather: UP8_GROUP = 32 lanes per COARSE pixel (both channels).  The lanes take consecutive fine columns of the
//                          pixel's footprint (up8_range; one coalesced run per row) and walk its rows; each candidate's prediction and cotangent
//                          g / count * v * sign(pred - flow_gt) are formed in registers and weighted with up8_weight.  A lane sums its column in
//                          fp64 in row order, the 32 lanes fold in a fixed butterfly: no atomics, no workspace, bit-identical from run to run.
#include "mpf_common.h"
#include "mpf_convex.h"          // up_neighbourhood, up_convex: shared with the cropped upsampling of mpf_raft_eval.hip
#include "mpf_reduce.h"
#include "mpf_upflow8.h"

#define UP_THREADS 256
#define UP_WAVES 4
#define UP_ROWS 2                // sub-rows per wave: UP_WAVES * UP_ROWS = 8
#define UP_NPART 6               // partials per block: S, sum epe, n(epe < 1), n(epe < 3), n(epe < 5), n(v)
#define UP8_MAX_BLOCKS 4096      // k_up8_loss: grid-stride beyond this many blocks
#define UP8_GROUP 32             // k_up8_loss_bwd: lanes per coarse pixel

enum { UP_FWD = 0, UP_BWD = 1, UP_LOSS = 2, UP_LOSS_BWD = 3 };

struct UpDev {
    const float *flow;
    const float *mask;
    const float *flow_gt;
    const float *valid;
    const float *g;
    float *out;                  // UP_FWD: written; UP_BWD: the cotangent, read
    float *grad_flow;
    float *grad_mask;
    float *term;
    double *metrics;
    double *partials;            // [blocks][UP_NPART]
    float *T;                    // [N, 2, 9, H, W]
    int N, H, W, HW, tiles;
    float max_flow;
};

template <int MODE>
__global__ __launch_bounds__(UP_THREADS) void k_upsample(const UpDev a)
{
    constexpr bool kGrad = MODE == UP_BWD || MODE == UP_LOSS_BWD;
    constexpr bool kLoss = MODE == UP_LOSS || MODE == UP_LOSS_BWD;
    __shared__ double sT[kGrad ? UP_WAVES * 18 * 64 : 1];
    __shared__ double sP[MODE == UP_LOSS ? UP_WAVES * UP_NPART : 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x / a.tiles, tile = blockIdx.x - n * a.tiles;
    const int H = a.H, W = a.W, HW = a.HW;
    const int p = tile * 64 + lane;
    const bool live = p < HW;
    const int pc = live ? p : HW - 1;
    const int h = pc / W, w = pc - h * W;

    float f[2][9];                                           // 8 * flow on the 3 x 3 neighbourhood, 0 outside the map
    up_neighbourhood(a.flow, n, H, W, h, w, f);

    float gs = 0.0f;
    if (MODE == UP_LOSS_BWD) gs = a.g[0] / (float)((long long)a.N * 128 * HW);      // the mean's share of the upstream gradient
    double t[2][9];
    if (kGrad) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int k = 0; k < 9; ++k) t[c][k] = 0.0;
    }
    double S = 0.0, esum = 0.0;
    int n1 = 0, n3 = 0, n5 = 0, nv = 0;

    for (int r = 0; r < UP_ROWS; ++r) {
        const int i = wave * UP_ROWS + r;
        const int row = (8 * h + i) * 8 * W + 8 * w;         // offset of the lane's eight entries inside one [8H, 8W] plane
        const int plane = 64 * HW;
        float x[2][8], val[8];                               // UP_BWD: the cotangent; loss modes: flow_gt and valid
        if (MODE != UP_FWD) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float *src = (MODE == UP_BWD ? a.out : a.flow_gt) + (n * 2 + c) * plane + row;
                const float4 q0 = *(const float4 *)src, q1 = *(const float4 *)(src + 4);
                x[c][0] = q0.x, x[c][1] = q0.y, x[c][2] = q0.z, x[c][3] = q0.w;
                x[c][4] = q1.x, x[c][5] = q1.y, x[c][6] = q1.z, x[c][7] = q1.w;
            }
        }
        if (kLoss) {
            const float *src = a.valid + n * plane + row;
            const float4 q0 = *(const float4 *)src, q1 = *(const float4 *)(src + 4);
            val[0] = q0.x, val[1] = q0.y, val[2] = q0.z, val[3] = q0.w;
            val[4] = q1.x, val[5] = q1.y, val[6] = q1.z, val[7] = q1.w;
        }
        float o[2][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ch0 = (n * 576 + i * 8 + j) * HW + pc;
            float m[9], o0, o1;
            up_convex(a.mask + ch0, plane, f, m, o0, o1);    // m is now the softmax p[k]
            o[0][j] = o0, o[1][j] = o1;

            float c0 = 0.0f, c1 = 0.0f;                      // the cotangent at this entry
            if (MODE == UP_BWD) c0 = x[0][j], c1 = x[1][j];
            if (kLoss) {
                const float gu = x[0][j], gv = x[1][j];
                const bool v = val[j] >= 0.5f && sqrtf(gu * gu + gv * gv) < a.max_flow;
                const float vf = v ? 1.0f : 0.0f;
                const float d0 = o0 - gu, d1 = o1 - gv;
                if (MODE == UP_LOSS) {
                    if (live) {
                        S += (double)(vf * fabsf(d0)) + (double)(vf * fabsf(d1));
                        if (a.metrics && v) {
                            const float epe = sqrtf(d0 * d0 + d1 * d1);
                            esum += (double)epe;
                            n1 += epe < 1.0f, n3 += epe < 3.0f, n5 += epe < 5.0f, nv += 1;
                        }
                    }
                } else {                                     // sign(0) = 0, and a NaN difference has sign 0 as torch's sgn has
                    const float gv_ = gs * vf;
                    c0 = gv_ * (float)((d0 > 0.0f) - (d0 < 0.0f));
                    c1 = gv_ * (float)((d1 > 0.0f) - (d1 < 0.0f));
                }
            }
            if (kGrad) {
                // softmax backward as torch writes it: (dp[k] - sum_k' dp[k'] p[k']) * p[k], dp[k] = sum_c cot[c] * 8 flow[c, tap k]
                float dp[9], dot = 0.0f;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    dp[k] = fmaf(c1, f[1][k], c0 * f[0][k]);
                    dot = fmaf(dp[k], m[k], dot);
                    t[0][k] += (double)(m[k] * c0);
                    t[1][k] += (double)(m[k] * c1);
                }
                if (live) {
#pragma unroll
                    for (int k = 0; k < 9; ++k) a.grad_mask[ch0 + k * plane] = (dp[k] - dot) * m[k];
                }
            }
        }
        if (MODE == UP_FWD && live) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                float *dst = a.out + (n * 2 + c) * plane + row;
                *(float4 *)dst = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
                *(float4 *)(dst + 4) = make_float4(o[c][4], o[c][5], o[c][6], o[c][7]);
            }
        }
    }

    if (kGrad) {                                             // fold the four waves' sub-rows in wave order, store T along w
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int k = 0; k < 9; ++k) sT[(wave * 18 + c * 9 + k) * 64 + lane] = t[c][k];
        __syncthreads();
        for (int idx = threadIdx.x; idx < 18 * 64; idx += UP_THREADS) {
            const int ck = idx >> 6, l = idx & 63;
            double v = sT[ck * 64 + l];
#pragma unroll
            for (int q = 1; q < UP_WAVES; ++q) v += sT[(q * 18 + ck) * 64 + l];
            if (tile * 64 + l < HW) a.T[(n * 18 + ck) * HW + tile * 64 + l] = (float)v;
        }
    }
    if (MODE == UP_LOSS) {
        const double part[UP_NPART] = {S, esum, (double)n1, (double)n3, (double)n5, (double)nv};
        mpf_block_sums<UP_WAVES>(part, a.metrics ? UP_NPART : 1, sP, a.partials + (long long)blockIdx.x * UP_NPART);
    }
}

// grad_flow[n,c,h,w] = 8 * sum_k T[n, c, k, h - ky + 1, w - kx + 1]: pixel (h - ky + 1, w - kx + 1) used (h, w) as its tap k
__global__ __launch_bounds__(UP_THREADS) void k_upsample_fold(const UpDev a)
{
    const int idx = blockIdx.x * UP_THREADS + threadIdx.x;
    if (idx >= a.N * 2 * a.HW) return;
    const int nc = idx / a.HW, yx = idx - nc * a.HW;
    const int h = yx / a.W, w = yx - h * a.W;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int hh = h - (k / 3 - 1), ww = w - (k % 3 - 1);
        if ((unsigned)hh < (unsigned)a.H && (unsigned)ww < (unsigned)a.W) s += (double)a.T[(nc * 9 + k) * a.HW + hh * a.W + ww];
    }
    a.grad_flow[idx] = 8.0f * (float)s;
}

// one block: the blocks' partials in a fixed order, fp64; term = S / count
__global__ __launch_bounds__(UP_THREADS) void k_upsample_finish(const UpDev a, int blocks)
{
    __shared__ double sR[UP_THREADS];
    const int nq = a.metrics ? UP_NPART : 1;
    for (int q = 0; q < nq; ++q) {
        double v = 0.0;
        for (int b = threadIdx.x; b < blocks; b += UP_THREADS) v += a.partials[(long long)b * UP_NPART + q];
        mpf_block_tree_sum<UP_THREADS>(v, sR);
        if (threadIdx.x == 0) {
            if (q == 0)
                a.term[0] = (float)(sR[0] / ((double)a.N * 128.0 * (double)a.HW));
            else
                a.metrics[q - 1] = sR[0];
        }
        __syncthreads();
    }
}

// the bilinear loss: what the kernels need beyond UpDev
struct Up8Geo {
    float sy, sx;                // up8_scale(H), up8_scale(W)
    unsigned total;              // k_up8_loss: lanes = N * 8H * 2W; k_up8_loss_bwd: coarse pixels = N * H * W
};

__global__ __launch_bounds__(UP_THREADS) void k_up8_loss(const UpDev a, const Up8Geo q)
{
    __shared__ double sP[UP_WAVES * UP_NPART];
    const int H = a.H, W = a.W, H8 = 8 * H, W8 = 8 * W;
    const unsigned per_row = (unsigned)(2 * W);
    const size_t plane = (size_t)H8 * W8;
    double S = 0.0, esum = 0.0;
    int n1 = 0, n3 = 0, n5 = 0, nv = 0;
    // t < total < 2^29 and the stride is at most UP8_MAX_BLOCKS * UP_THREADS = 2^20, so the last increment cannot wrap
    for (unsigned t = blockIdx.x * UP_THREADS + threadIdx.x; t < q.total; t += gridDim.x * UP_THREADS) {
        const unsigned row = t / per_row;                                 // n * 8H + Y
        const int X = (int)(t - row * per_row) * 4;
        const int n = (int)(row / (unsigned)H8), Y = (int)(row - (unsigned)n * H8);
        int y0, y1;
        float ly;
        up8_taps(Y, H, q.sy, y0, y1, ly);
        const float hy = 1.0f - ly;
        const float *u0 = a.flow + ((size_t)(n * 2) * H + y0) * W, *u1 = a.flow + ((size_t)(n * 2) * H + y1) * W;
        const float *v0 = u0 + a.HW, *v1 = u1 + a.HW;
        const float *gsrc = a.flow_gt + ((size_t)(n * 2) * H8 + Y) * W8 + X;
        const float4 qu = *(const float4 *)gsrc, qv = *(const float4 *)(gsrc + plane), qa = *(const float4 *)(a.valid + (size_t)row * W8 + X);
        const float gu4[4] = {qu.x, qu.y, qu.z, qu.w}, gv4[4] = {qv.x, qv.y, qv.z, qv.w}, val[4] = {qa.x, qa.y, qa.z, qa.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int x0, x1;
            float lx;
            up8_taps(X + e, W, q.sx, x0, x1, lx);
            const float hx = 1.0f - lx;
            const float o0 = up8_value(u0, u1, x0, x1, hy, ly, hx, lx), o1 = up8_value(v0, v1, x0, x1, hy, ly, hx, lx);
            const float gu = gu4[e], gv = gv4[e];
            const bool v = val[e] >= 0.5f && sqrtf(gu * gu + gv * gv) < a.max_flow;
            const float vf = v ? 1.0f : 0.0f;
            const float d0 = o0 - gu, d1 = o1 - gv;
            S += (double)(vf * fabsf(d0)) + (double)(vf * fabsf(d1));
            if (a.metrics && v) {
                const float epe = sqrtf(d0 * d0 + d1 * d1);
                esum += (double)epe;
                n1 += epe < 1.0f, n3 += epe < 3.0f, n5 += epe < 5.0f, nv += 1;
            }
        }
    }
    const double part[UP_NPART] = {S, esum, (double)n1, (double)n3, (double)n5, (double)nv};
    mpf_block_sums<UP_WAVES>(part, a.metrics ? UP_NPART : 1, sP, a.partials + (size_t)blockIdx.x * UP_NPART);
}

__global__ __launch_bounds__(UP_THREADS) void k_up8_loss_bwd(const UpDev a, const Up8Geo q)
{
    const int sub = threadIdx.x & (UP8_GROUP - 1);
    const unsigned pix = blockIdx.x * (UP_THREADS / UP8_GROUP) + (threadIdx.x / UP8_GROUP);
    const bool live = pix < q.total;
    const unsigned p = live ? pix : q.total - 1;                          // a group past the end works on the last pixel and stores nothing
    const int H = a.H, W = a.W, HW = a.HW, H8 = 8 * H, W8 = 8 * W;
    const int n = (int)(p / (unsigned)HW), yx = (int)(p - (unsigned)n * HW);
    const int y = yx / W, x = yx - y * W;
    int ylo, yhi, xlo, xhi;
    up8_range(y, H, ylo, yhi);
    up8_range(x, W, xlo, xhi);
    const float gs = a.g[0] / (float)((long long)a.N * 128 * HW);        // the mean's share of the upstream gradient
    const float *fu = a.flow + (size_t)(n * 2) * HW, *fv = fu + HW;
    const size_t plane = (size_t)H8 * W8;
    const float *gt = a.flow_gt + (size_t)(n * 2) * plane, *va = a.valid + (size_t)n * plane;
    double acc0 = 0.0, acc1 = 0.0;
    for (int X = xlo + sub; X <= xhi; X += UP8_GROUP) {
        const float wx = up8_weight(X, x, W, q.sx);
        if (wx == 0.0f) continue;
        int x0, x1;
        float lx;
        up8_taps(X, W, q.sx, x0, x1, lx);
        const float hx = 1.0f - lx;
        for (int Y = ylo; Y <= yhi; ++Y) {
            const float wy = up8_weight(Y, y, H, q.sy);
            if (wy == 0.0f) continue;
            int y0, y1;
            float ly;
            up8_taps(Y, H, q.sy, y0, y1, ly);
            const float hy = 1.0f - ly;
            const float o0 = up8_value(fu + y0 * W, fu + y1 * W, x0, x1, hy, ly, hx, lx);
            const float o1 = up8_value(fv + y0 * W, fv + y1 * W, x0, x1, hy, ly, hx, lx);
            const size_t at = (size_t)Y * W8 + X;
            const float gu = gt[at], gv = gt[plane + at];
            const bool v = va[at] >= 0.5f && sqrtf(gu * gu + gv * gv) < a.max_flow;
            const float d0 = o0 - gu, d1 = o1 - gv;
            const float gv_ = gs * (v ? 1.0f : 0.0f);                     // sign(0) = 0, and a NaN difference has sign 0 as torch's sgn has
            const float c0 = gv_ * (float)((d0 > 0.0f) - (d0 < 0.0f)), c1 = gv_ * (float)((d1 > 0.0f) - (d1 < 0.0f));
            const double w = (double)wy * (double)wx;                     // exact
            acc0 += w * (double)c0;
            acc1 += w * (double)c1;
        }
    }
#pragma unroll
    for (int m = UP8_GROUP / 2; m >= 1; m >>= 1) {
        acc0 += __shfl_xor(acc0, m);
        acc1 += __shfl_xor(acc1, m);
    }
    if (live && sub == 0) {
        a.grad_flow[(size_t)(n * 2) * HW + yx] = (float)(8.0 * acc0);
        a.grad_flow[(size_t)(n * 2 + 1) * HW + yx] = (float)(8.0 * acc1);
    }
}

static size_t up_partials_bytes(int64_t blocks) { return (size_t)blocks * UP_NPART * sizeof(double); }

static int up_shape(int N, int H, int W, const char *who, int64_t &blocks)
{
    MPF_REQUIRE(N >= 1 && H >= 1 && W >= 1, "%s: bad shape N, H, W = %d, %d, %d", who, N, H, W);
    const int64_t lim = (int64_t)1 << 31;
    const int64_t hw = (int64_t)H * W;
    MPF_REQUIRE(hw < lim / 576 && (int64_t)N * hw < lim / 576, "%s: mask [N,576,H,W] must hold fewer than 2^31 elements (N, H, W = %d, %d, %d)", who, N, H, W);
    blocks = (int64_t)N * ((hw + 63) / 64);
    return 0;
}

extern "C" size_t mpf_upsample_workspace(int N, int H, int W, int backward)
{
    int64_t blocks;
    if (up_shape(N, H, W, "mpf_upsample_workspace", blocks)) return 0;
    return backward ? (size_t)N * 18 * H * W * sizeof(float) : up_partials_bytes(blocks);
}

static int up_check(const MpfUpsampleArgs *a, int mode, const char *who, UpDev &d, int64_t &blocks)
{
    MPF_REQUIRE(a, "%s: null argument block", who);
    MPF_REQUIRE(a->flow && a->mask, "%s: null pointer (flow or mask)", who);
    const int rc = up_shape(a->N, a->H, a->W, who, blocks);
    if (rc) return rc;
    const bool grad = mode == UP_BWD || mode == UP_LOSS_BWD, loss = mode == UP_LOSS || mode == UP_LOSS_BWD;
    if (!loss) {
        MPF_REQUIRE(a->out, "%s: null pointer (out)", who);
        MPF_REQUIRE(mpf_aligned16(a->out), "%s: out must be 16-byte aligned", who);
    } else {
        MPF_REQUIRE(a->flow_gt && a->valid, "%s: null pointer (flow_gt or valid)", who);
        MPF_REQUIRE(mpf_aligned16(a->flow_gt) && mpf_aligned16(a->valid), "%s: flow_gt and valid must be 16-byte aligned", who);
    }
    if (mode == UP_LOSS) MPF_REQUIRE(a->term, "%s: null pointer (term)", who);
    if (mode == UP_LOSS_BWD) MPF_REQUIRE(a->g, "%s: null pointer (g)", who);
    if (grad) MPF_REQUIRE(a->grad_flow && a->grad_mask, "%s: null pointer (grad_flow or grad_mask)", who);
    if (grad || mode == UP_LOSS) {
        const size_t need = grad ? (size_t)a->N * 18 * a->H * a->W * sizeof(float) : up_partials_bytes(blocks);
        MPF_REQUIRE(a->workspace, "%s: null pointer (workspace)", who);
        MPF_REQUIRE((((uintptr_t)a->workspace) & 7) == 0, "%s: workspace must be 8-byte aligned", who);
        MPF_REQUIRE(a->workspace_bytes >= need, "%s: workspace holds %zu bytes, %zu needed (mpf_upsample_workspace)", who, a->workspace_bytes, need);
    }
    d = UpDev{};
    d.flow = a->flow, d.mask = a->mask, d.flow_gt = a->flow_gt, d.valid = a->valid, d.g = a->g;
    d.out = a->out, d.grad_flow = a->grad_flow, d.grad_mask = a->grad_mask, d.term = a->term;
    d.metrics = mode == UP_LOSS ? a->metrics : nullptr;
    d.partials = (double *)a->workspace, d.T = (float *)a->workspace;
    d.N = a->N, d.H = a->H, d.W = a->W, d.HW = a->H * a->W, d.tiles = (d.HW + 63) / 64;
    d.max_flow = a->max_flow;
    return 0;
}

template <int MODE>
static int up_launch(const MpfUpsampleArgs *a, void *stream, const char *who)
{
    UpDev d;
    int64_t blocks;
    const int rc = up_check(a, MODE, who, d, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL(k_upsample<MODE>, dim3((unsigned)blocks), dim3(UP_THREADS), 0, (hipStream_t)stream, d);
    int st = mpf_launch_status("k_upsample");
    if (st) return st;
    if (MODE == UP_BWD || MODE == UP_LOSS_BWD) {
        const int64_t n = (int64_t)d.N * 2 * d.HW;
        hipLaunchKernelGGL(k_upsample_fold, dim3((unsigned)((n + UP_THREADS - 1) / UP_THREADS)), dim3(UP_THREADS), 0, (hipStream_t)stream, d);
        st = mpf_launch_status("k_upsample_fold");
    }
    if (MODE == UP_LOSS) {
        hipLaunchKernelGGL(k_upsample_finish, dim3(1), dim3(UP_THREADS), 0, (hipStream_t)stream, d, (int)blocks);
        st = mpf_launch_status("k_upsample_finish");
    }
    return st;
}

extern "C" int mpf_upsample_flow(const MpfUpsampleArgs *a, void *stream) { return up_launch<UP_FWD>(a, stream, "mpf_upsample_flow"); }

extern "C" int mpf_upsample_flow_backward(const MpfUpsampleArgs *a, void *stream)
{
    return up_launch<UP_BWD>(a, stream, "mpf_upsample_flow_backward");
}

extern "C" int mpf_flow_loss_term(const MpfUpsampleArgs *a, void *stream) { return up_launch<UP_LOSS>(a, stream, "mpf_flow_loss_term"); }

extern "C" int mpf_flow_loss_term_backward(const MpfUpsampleArgs *a, void *stream)
{
    return up_launch<UP_LOSS_BWD>(a, stream, "mpf_flow_loss_term_backward");
}

// the bilinear loss: N, H, W >= 1 and flow_gt [N,2,8H,8W] below 2^31 elements; blocks of k_up8_loss (one partial row each)
static int up8_loss_shape(int N, int H, int W, const char *who, int64_t &blocks)
{
    MPF_REQUIRE(N >= 1 && H >= 1 && W >= 1, "%s: bad shape N, H, W = %d, %d, %d", who, N, H, W);
    const int64_t lim = (int64_t)1 << 31;
    const int64_t hw = (int64_t)H * W;
    MPF_REQUIRE(hw < lim / 128 && (int64_t)N * hw < lim / 128, "%s: flow_gt [N,2,8H,8W] must hold fewer than 2^31 elements (N, H, W = %d, %d, %d)", who, N, H, W);
    blocks = ((int64_t)N * hw * 16 + UP_THREADS - 1) / UP_THREADS;
    if (blocks > UP8_MAX_BLOCKS) blocks = UP8_MAX_BLOCKS;
    return 0;
}

extern "C" size_t mpf_upflow8_loss_workspace(int N, int H, int W, int backward)
{
    int64_t blocks;
    if (up8_loss_shape(N, H, W, "mpf_upflow8_loss_workspace", blocks)) return 0;
    return backward ? 0 : up_partials_bytes(blocks);                      // the backward call is a gather: no workspace
}

static int up8_loss_check(const MpfUpsampleArgs *a, bool backward, const char *who, UpDev &d, Up8Geo &q, int64_t &blocks)
{
    MPF_REQUIRE(a, "%s: null argument block", who);
    MPF_REQUIRE(a->flow, "%s: null pointer (flow)", who);
    const int rc = up8_loss_shape(a->N, a->H, a->W, who, blocks);
    if (rc) return rc;
    MPF_REQUIRE(a->flow_gt && a->valid, "%s: null pointer (flow_gt or valid)", who);
    MPF_REQUIRE(mpf_aligned16(a->flow_gt) && mpf_aligned16(a->valid), "%s: flow_gt and valid must be 16-byte aligned", who);
    if (!backward) {
        MPF_REQUIRE(a->term, "%s: null pointer (term)", who);
        MPF_REQUIRE(a->workspace, "%s: null pointer (workspace)", who);
        MPF_REQUIRE((((uintptr_t)a->workspace) & 7) == 0, "%s: workspace must be 8-byte aligned", who);
        MPF_REQUIRE(a->workspace_bytes >= up_partials_bytes(blocks), "%s: workspace holds %zu bytes, %zu needed (mpf_upflow8_loss_workspace)", who,
                    a->workspace_bytes, up_partials_bytes(blocks));
    } else {
        MPF_REQUIRE(a->g, "%s: null pointer (g)", who);
        MPF_REQUIRE(a->grad_flow, "%s: null pointer (grad_flow)", who);
    }
    d = UpDev{};
    d.flow = a->flow, d.flow_gt = a->flow_gt, d.valid = a->valid, d.g = a->g, d.grad_flow = a->grad_flow, d.term = a->term;
    d.metrics = backward ? nullptr : a->metrics;
    d.partials = backward ? nullptr : (double *)a->workspace;
    d.N = a->N, d.H = a->H, d.W = a->W, d.HW = a->H * a->W;
    d.max_flow = a->max_flow;
    q.sy = up8_scale(a->H), q.sx = up8_scale(a->W);
    q.total = (unsigned)((int64_t)a->N * d.HW * (backward ? 1 : 16));
    return 0;
}

extern "C" int mpf_upflow8_loss_term(const MpfUpsampleArgs *a, void *stream)
{
    UpDev d;
    Up8Geo q;
    int64_t blocks;
    const int rc = up8_loss_check(a, false, "mpf_upflow8_loss_term", d, q, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL(k_up8_loss, dim3((unsigned)blocks), dim3(UP_THREADS), 0, (hipStream_t)stream, d, q);
    const int st = mpf_launch_status("k_up8_loss");
    if (st) return st;
    hipLaunchKernelGGL(k_upsample_finish, dim3(1), dim3(UP_THREADS), 0, (hipStream_t)stream, d, (int)blocks);
    return mpf_launch_status("k_upsample_finish");
}

extern "C" int mpf_upflow8_loss_term_backward(const MpfUpsampleArgs *a, void *stream)
{
    UpDev d;
    Up8Geo q;
    int64_t blocks;
    const int rc = up8_loss_check(a, true, "mpf_upflow8_loss_term_backward", d, q, blocks);
    if (rc) return rc;
    const unsigned per = UP_THREADS / UP8_GROUP;
    hipLaunchKernelGGL(k_up8_loss_bwd, dim3((q.total + per - 1) / per), dim3(UP_THREADS), 0, (hipStream_t)stream, d, q);
    return mpf_launch_status("k_up8_loss_bwd");
}
