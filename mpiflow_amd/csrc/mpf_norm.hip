// mpf_norm.hip - the memory-bound chain between the convolutions of RAFT's encoders (RAFT/core/extractor.py) for gfx950, fused: normalise, ReLU,
// add the shortcut, ReLU, forward and gradient, in four kernels.
//
// Contract: include/mpiflow_hip.h (MpfNormTerm, MpfNormArgs).  A term is a convolution output x [N,C,H,W] with a norm mode; a block's tail is
// out = relu(residual + relu(norm(y.x))) with the residual a plain tensor (identity shortcut) or a second normalised term (the downsample
// branch), so the tail of a strided block is one pass over two inputs and one output.
//
// k_norm_stats          per (plane, chunk): mean and centred sum of squares M2 of the chunk, from fp64 sums of d = x - x[first of the chunk] and d*d
//                       (shifted: a convolution's bias never meets its variance), written as one fp64 pair: how a plane is split into chunks
//                       changes the statistics in the last bits of fp64 only, far below the one fp32 rounding of mean and rstd.
// k_norm_act            prologue: wave 0 merges the pairs of the workgroup's statistic set with Chan's formula in fp64 - lane l takes pairs l, l + 64,
//                       ... in order, then a fixed shuffle tree - and hands mean and rstd to the other waves through LDS; one workgroup per set
//                       writes them out.  Then the pointwise pass over its chunk.
// k_norm_bwd_reduce     recomputes both ReLU masks from the same inputs and the saved mean / rstd (the same arithmetic as forward: the same bits);
//                       per (plane, chunk) sum dy and sum dy * xhat of every normalised term, fp64 sums, one fp64 pair each.
// k_norm_bwd            prologue: wave 0 merges those pairs over the set (weighted by the channel's weight: one form for instance, batch and group
//                       norm), in the same fixed order; the workgroup of (n = 0, chunk 0) of a channel also sums that channel's pairs to dweight
//                       and dbias.  Then dx of every term, and the shortcut's gradient, written or accumulated.
//
// Layout: grid (N*C planes, chunks); a workgroup of 256 walks its chunk of one plane, a lane 4 consecutive floats (one 16-byte access) when
// H*W % 4 == 0 and every pointer is 16-byte aligned, one float otherwise.  The chunk length does not depend on which: L = ceil(HW / chunks)
// rounded up to a multiple of 4.  chunks > 1 is for few, large planes (a B = 1 inference call has 64 - 128 planes at 1/2 resolution for 256 CUs).
// No atomics, and every reduction runs in an order fixed by the arguments: results are bit-identical from call to call.
//
// Numerics: eps = 1e-5.  relu(v) = v < 0 ? 0 : v (fmaxf would turn NaN into 0, torch keeps it), and the gradient passes where !(v <= 0), which
// is torch's threshold_backward.  No address depends on a tensor's values.
#include "mpf_common.h"
#include "mpf_math.h"
#include "mpf_reduce.h"

#define NORM_THREADS 256
#define NORM_WAVES (NORM_THREADS / 64)
#define NORM_EPS 1e-5

struct NormTermDev {
    const float *x, *w, *b, *rmean, *rvar;
    double *partials, *gpartials;
    float *mean, *rstd, *var, *dx, *dw, *db;
    int mode, groups;
};

struct NormDev {
    NormTermDev t[2];            // 0: the main term; 1: the residual term (x == nullptr: absent)
    const float *res, *g;
    float *out, *dres;
    int accumulate, N, C, HW, chunks, L;
};

struct NormShared {
    double red[NORM_WAVES][4];
    float stat[2][2];            // per term: mean, rstd
    float gsum[2][2];            // per term: mean(dy w), mean(dy w xhat) over the set
};

struct NormCoef {                // what the pointwise pass needs of one term
    float mean, rstd, w, b;
};

struct NormSet {                 // the (plane, chunk) pairs of one statistic set: pair(o, i) = base + o * stride + i, o < outer, i < inner
    int base, outer, stride, inner, index;
    double m;                    // elements of the set
    bool writer;                 // this workgroup writes the set's mean / rstd
};

__device__ __forceinline__ bool norm_has_stats(int mode) { return mode == MPF_NORM_INSTANCE || mode == MPF_NORM_BATCH_TRAIN || mode == MPF_NORM_GROUP; }

__device__ __forceinline__ int norm_chunk_count(const NormDev &a, int k)
{
    const long long s = (long long)k * a.L, e = s + a.L < a.HW ? s + a.L : a.HW;
    return e > s ? (int)(e - s) : 0;
}

__device__ __forceinline__ NormSet norm_set(const NormTermDev &t, const NormDev &a, int n, int c, int k)
{
    NormSet s;
    if (t.mode == MPF_NORM_BATCH_TRAIN) {
        s.base = c * a.chunks, s.outer = a.N, s.stride = a.C * a.chunks, s.inner = a.chunks, s.index = c;
        s.m = (double)a.N * a.HW, s.writer = n == 0 && k == 0;
    } else if (t.mode == MPF_NORM_GROUP) {
        const int cpg = a.C / t.groups, g = c / cpg;
        s.base = (n * a.C + g * cpg) * a.chunks, s.outer = 1, s.stride = 0, s.inner = cpg * a.chunks, s.index = n * t.groups + g;
        s.m = (double)cpg * a.HW, s.writer = c == g * cpg && k == 0;
    } else {
        s.base = (n * a.C + c) * a.chunks, s.outer = 1, s.stride = 0, s.inner = a.chunks, s.index = n * a.C + c;
        s.m = (double)a.HW, s.writer = k == 0;
    }
    return s;
}

// Chan et al.: (n, mean, M2) of the union of two disjoint samples
__device__ __forceinline__ void norm_chan(double &an, double &am, double &a2, double bn, double bm, double b2)
{
    if (bn == 0.0) return;
    if (an == 0.0) {
        an = bn, am = bm, a2 = b2;
        return;
    }
    const double n = an + bn, d = bm - am;
    am = am + d * (bn / n);
    a2 = a2 + b2 + d * d * (an * bn / n);
    an = n;
}

// wave 0, all 64 lanes: the set's mean and rstd -> sh.stat[term]; the writer also stores them
__device__ __forceinline__ void norm_merge_stats(const NormTermDev &t, const NormDev &a, const NormSet &s, float *stat)
{
    const int lane = threadIdx.x, total = s.outer * s.inner;
    double cn = 0.0, cm = 0.0, c2 = 0.0;
    for (int j = lane; j < total; j += 64) {
        const int o = j / s.inner, off = s.base + o * s.stride + (j - o * s.inner);
        norm_chan(cn, cm, c2, (double)norm_chunk_count(a, off % a.chunks), t.partials[2 * (size_t)off], t.partials[2 * (size_t)off + 1]);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double bn = __shfl_down(cn, o, 64), bm = __shfl_down(cm, o, 64), b2 = __shfl_down(c2, o, 64);
        norm_chan(cn, cm, c2, bn, bm, b2);
    }
    if (lane == 0) {
        const double var = c2 / cn;
        const float mean = (float)cm, rstd = (float)(1.0 / sqrt(var + NORM_EPS));
        stat[0] = mean, stat[1] = rstd;
        if (s.writer) {
            t.mean[s.index] = mean, t.rstd[s.index] = rstd;
            if (t.var) t.var[s.index] = (float)var;
        }
    }
}

// the sums of up to four values over the workgroup, in a fixed order, to every thread
template <int K>
__device__ __forceinline__ void norm_block_sum(double (&v)[K], NormShared &sh)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < K; ++e) {
        v[e] = mpf_wave_sum(v[e]);
        if (lane == 0) sh.red[wave][e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < K; ++e) {
        double s = sh.red[0][e];
#pragma unroll
        for (int w = 1; w < NORM_WAVES; ++w) s += sh.red[w][e];
        v[e] = s;
    }
}

__device__ __forceinline__ float norm_relu(float v) { return v < 0.0f ? 0.0f : v; }

__device__ __forceinline__ float norm_xhat(float x, const NormCoef &c) { return (x - c.mean) * c.rstd; }

__device__ __forceinline__ float norm_value(float x, const NormCoef &c, int mode) { return mode == MPF_NORM_NONE ? x : norm_xhat(x, c) * c.w + c.b; }

// weight, bias and - BATCH_EVAL, or with `saved` the statistics modes too - mean and rstd of channel c
__device__ __forceinline__ NormCoef norm_coef(const NormTermDev &t, const NormDev &a, int n, int c, bool saved)
{
    NormCoef k = NormCoef{0.0f, 1.0f, 1.0f, 0.0f};
    if (t.mode == MPF_NORM_NONE) return k;
    if (t.w) k.w = t.w[c];
    if (t.b) k.b = t.b[c];
    if (t.mode == MPF_NORM_BATCH_EVAL) {
        k.mean = t.rmean[c];
        k.rstd = (float)(1.0 / sqrt((double)t.rvar[c] + NORM_EPS));
    } else if (saved) {
        const int index = norm_set(t, a, n, c, 0).index;
        k.mean = t.mean[index], k.rstd = t.rstd[index];
    }
    return k;
}

template <int VEC>
__global__ __launch_bounds__(NORM_THREADS) void k_norm_stats(const NormDev a)
{
    __shared__ NormShared sh;
    const NormTermDev &t = a.t[blockIdx.z];
    const int plane = blockIdx.x, k = blockIdx.y, count = norm_chunk_count(a, k);
    const float *p = t.x + (size_t)plane * a.HW + (size_t)k * a.L;
    const double shift = count > 0 ? (double)p[0] : 0.0;
    double s[2] = {0.0, 0.0};
    for (int i = threadIdx.x * VEC; i < count; i += NORM_THREADS * VEC) {
        float v[VEC];
        mpf_load_vec<VEC>(p + i, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const double d = (double)v[e] - shift;
            s[0] += d, s[1] += d * d;
        }
    }
    norm_block_sum<2>(s, sh);
    if (threadIdx.x == 0) {
        double mean = 0.0, m2 = 0.0;
        if (count > 0) {
            const double q = s[1] - s[0] * s[0] / count;
            mean = shift + s[0] / count, m2 = q < 0.0 ? 0.0 : q;
        }
        double *o = t.partials + 2 * ((size_t)plane * a.chunks + k);
        o[0] = mean, o[1] = m2;
    }
}

template <int VEC>
__global__ __launch_bounds__(NORM_THREADS) void k_norm_act(const NormDev a)
{
    __shared__ NormShared sh;
    const int plane = blockIdx.x, k = blockIdx.y, n = plane / a.C, c = plane - n * a.C;
    const bool has_r = a.t[1].x != nullptr;
    if (threadIdx.x < 64) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (a.t[j].x && norm_has_stats(a.t[j].mode)) norm_merge_stats(a.t[j], a, norm_set(a.t[j], a, n, c, k), sh.stat[j]);
    }
    __syncthreads();
    NormCoef co[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (!a.t[j].x) continue;
        co[j] = norm_coef(a.t[j], a, n, c, false);
        if (norm_has_stats(a.t[j].mode)) co[j].mean = sh.stat[j][0], co[j].rstd = sh.stat[j][1];
    }
    const int count = norm_chunk_count(a, k);
    const size_t base = (size_t)plane * a.HW + (size_t)k * a.L;
    for (int i = threadIdx.x * VEC; i < count; i += NORM_THREADS * VEC) {
        float x[VEC], r[VEC], o[VEC];
        mpf_load_vec<VEC>(a.t[0].x + base + i, x);
        if (has_r)
            mpf_load_vec<VEC>(a.t[1].x + base + i, r);
        else if (a.res)
            mpf_load_vec<VEC>(a.res + base + i, r);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float y = norm_relu(norm_value(x[e], co[0], a.t[0].mode));
            if (has_r)
                o[e] = norm_relu(norm_value(r[e], co[1], a.t[1].mode) + y);
            else if (a.res)
                o[e] = norm_relu(r[e] + y);
            else
                o[e] = y;
        }
        mpf_store_vec<VEC>(a.out + base + i, o);
    }
}

// the cotangents of the two terms' normalised values at one element: dy of the main term, g2 of the residual
__device__ __forceinline__ void norm_masks(float g, float v0, bool residual, float rv, float &dy, float &g2)
{
    const float y = norm_relu(v0);
    g2 = residual ? ((rv + y) <= 0.0f ? 0.0f : g) : g;
    dy = v0 <= 0.0f ? 0.0f : g2;
}

template <int VEC>
__global__ __launch_bounds__(NORM_THREADS) void k_norm_bwd_reduce(const NormDev a)
{
    __shared__ NormShared sh;
    const int plane = blockIdx.x, k = blockIdx.y, n = plane / a.C, c = plane - n * a.C;
    const bool has_r = a.t[1].x != nullptr, residual = has_r || a.res;
    NormCoef co[2];
    co[0] = norm_coef(a.t[0], a, n, c, true);
    if (has_r) co[1] = norm_coef(a.t[1], a, n, c, true);
    const int count = norm_chunk_count(a, k);
    const size_t base = (size_t)plane * a.HW + (size_t)k * a.L;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x * VEC; i < count; i += NORM_THREADS * VEC) {
        float x[VEC], r[VEC], g[VEC];
        mpf_load_vec<VEC>(a.t[0].x + base + i, x);
        mpf_load_vec<VEC>(a.g + base + i, g);
        if (has_r)
            mpf_load_vec<VEC>(a.t[1].x + base + i, r);
        else if (a.res)
            mpf_load_vec<VEC>(a.res + base + i, r);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float rv = has_r ? norm_value(r[e], co[1], a.t[1].mode) : (a.res ? r[e] : 0.0f);
            float dy, g2;
            norm_masks(g[e], norm_value(x[e], co[0], a.t[0].mode), residual, rv, dy, g2);
            s[0] += (double)dy, s[1] += (double)dy * (double)norm_xhat(x[e], co[0]);
            if (has_r) s[2] += (double)g2, s[3] += (double)g2 * (double)norm_xhat(r[e], co[1]);
        }
    }
    norm_block_sum<4>(s, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!a.t[j].x || !a.t[j].gpartials) continue;
            double *o = a.t[j].gpartials + 2 * ((size_t)plane * a.chunks + k);
            o[0] = s[2 * j], o[1] = s[2 * j + 1];
        }
    }
}

// wave 0, all 64 lanes: the set's mean(dy w) and mean(dy w xhat) -> gsum; the workgroup of (n = 0, chunk 0) also writes dweight[c], dbias[c]
__device__ __forceinline__ void norm_merge_grads(const NormTermDev &t, const NormDev &a, int n, int c, int k, float *gsum)
{
    const int lane = threadIdx.x;
    if (norm_has_stats(t.mode)) {
        const NormSet s = norm_set(t, a, n, c, k);
        const int total = s.outer * s.inner;
        double sa = 0.0, sb = 0.0;
        for (int j = lane; j < total; j += 64) {
            const int o = j / s.inner, off = s.base + o * s.stride + (j - o * s.inner);
            const double w = t.w ? (double)t.w[(off / a.chunks) % a.C] : 1.0;
            sa += w * t.gpartials[2 * (size_t)off], sb += w * t.gpartials[2 * (size_t)off + 1];
        }
        sa = mpf_wave_sum(sa), sb = mpf_wave_sum(sb);
        if (lane == 0) gsum[0] = (float)(sa / s.m), gsum[1] = (float)(sb / s.m);
    }
    if (n == 0 && k == 0 && (t.dw || t.db)) {
        const int total = a.N * a.chunks;
        double sa = 0.0, sb = 0.0;
        for (int j = lane; j < total; j += 64) {
            const int nn = j / a.chunks, off = (nn * a.C + c) * a.chunks + (j - nn * a.chunks);
            sa += t.gpartials[2 * (size_t)off], sb += t.gpartials[2 * (size_t)off + 1];
        }
        sa = mpf_wave_sum(sa), sb = mpf_wave_sum(sb);
        if (lane == 0) {
            if (t.db) t.db[c] = (float)sa;
            if (t.dw) t.dw[c] = (float)sb;
        }
    }
}

// dx of one term from the cotangent d of its normalised value
__device__ __forceinline__ float norm_dx(float d, float x, const NormCoef &c, int mode, const float *gsum)
{
    if (mode == MPF_NORM_NONE) return d;
    if (mode == MPF_NORM_BATCH_EVAL) return d * (c.w * c.rstd);
    return c.rstd * (d * c.w - gsum[0] - norm_xhat(x, c) * gsum[1]);
}

template <int VEC>
__global__ __launch_bounds__(NORM_THREADS) void k_norm_bwd(const NormDev a)
{
    __shared__ NormShared sh;
    const int plane = blockIdx.x, k = blockIdx.y, n = plane / a.C, c = plane - n * a.C;
    const bool has_r = a.t[1].x != nullptr, residual = has_r || a.res;
    if (threadIdx.x < 64) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (a.t[j].x && a.t[j].mode != MPF_NORM_NONE && a.t[j].gpartials) norm_merge_grads(a.t[j], a, n, c, k, sh.gsum[j]);
    }
    __syncthreads();
    NormCoef co[2];
    co[0] = norm_coef(a.t[0], a, n, c, true);
    if (has_r) co[1] = norm_coef(a.t[1], a, n, c, true);
    const int count = norm_chunk_count(a, k);
    const size_t base = (size_t)plane * a.HW + (size_t)k * a.L;
    for (int i = threadIdx.x * VEC; i < count; i += NORM_THREADS * VEC) {
        float x[VEC], r[VEC], g[VEC], d0[VEC], d1[VEC];
        mpf_load_vec<VEC>(a.t[0].x + base + i, x);
        mpf_load_vec<VEC>(a.g + base + i, g);
        if (has_r)
            mpf_load_vec<VEC>(a.t[1].x + base + i, r);
        else if (a.res)
            mpf_load_vec<VEC>(a.res + base + i, r);
        if (a.res && a.accumulate) mpf_load_vec<VEC>(a.dres + base + i, d1);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float rv = has_r ? norm_value(r[e], co[1], a.t[1].mode) : (a.res ? r[e] : 0.0f);
            float dy, g2;
            norm_masks(g[e], norm_value(x[e], co[0], a.t[0].mode), residual, rv, dy, g2);
            d0[e] = norm_dx(dy, x[e], co[0], a.t[0].mode, sh.gsum[0]);
            if (has_r)
                d1[e] = norm_dx(g2, r[e], co[1], a.t[1].mode, sh.gsum[1]);
            else if (a.res)
                d1[e] = a.accumulate ? d1[e] + g2 : g2;
        }
        mpf_store_vec<VEC>(a.t[0].dx + base + i, d0);
        if (has_r)
            mpf_store_vec<VEC>(a.t[1].dx + base + i, d1);
        else if (a.res)
            mpf_store_vec<VEC>(a.dres + base + i, d1);
    }
}

enum { NORM_STATS = 0, NORM_ACT = 1, NORM_BWD_REDUCE = 2, NORM_BWD = 3 };

// one term's pointers for the call `what`; `all16` is cleared by a tensor pointer that is not 16-byte aligned
static int norm_term(const MpfNormTerm &t, const MpfNormArgs *a, int what, const char *who, const char *name, NormTermDev &d, bool &all16)
{
    d = NormTermDev{};
    d.mode = MPF_NORM_NONE, d.groups = 1;
    if (!t.x) return 0;
    MPF_REQUIRE(t.mode >= MPF_NORM_NONE && t.mode <= MPF_NORM_GROUP, "%s: %s.mode must be one of MPF_NORM_* 0..4 (got %d)", who, name, t.mode);
    const bool stats = t.mode == MPF_NORM_INSTANCE || t.mode == MPF_NORM_BATCH_TRAIN || t.mode == MPF_NORM_GROUP;
    d.x = t.x, d.mode = t.mode;
    all16 = all16 && mpf_aligned16(t.x);
    if (t.mode == MPF_NORM_NONE) {
        if (what == NORM_BWD) {
            MPF_REQUIRE(t.dx, "%s: null pointer (%s.dx)", who, name);
            d.dx = t.dx;
            all16 = all16 && mpf_aligned16(t.dx);
        }
        return 0;
    }
    if (t.mode == MPF_NORM_GROUP) {
        MPF_REQUIRE(t.groups >= 1 && a->C % t.groups == 0, "%s: %s.groups must divide C = %d (got %d)", who, name, a->C, t.groups);
        d.groups = t.groups;
    }
    d.w = t.weight, d.b = t.bias;
    if (t.mode == MPF_NORM_BATCH_EVAL) {
        MPF_REQUIRE(t.running_mean && t.running_var, "%s: null pointer (%s.running_mean / running_var, MPF_NORM_BATCH_EVAL)", who, name);
        d.rmean = t.running_mean, d.rvar = t.running_var;
    }
    if (stats && (what == NORM_STATS || what == NORM_ACT)) {
        MPF_REQUIRE(t.partials, "%s: null pointer (%s.partials)", who, name);
        d.partials = t.partials;
    }
    if (stats && what != NORM_STATS) {
        MPF_REQUIRE(t.mean && t.rstd, "%s: null pointer (%s.mean / rstd)", who, name);
        d.mean = t.mean, d.rstd = t.rstd, d.var = t.var;
    }
    if (what == NORM_BWD_REDUCE || what == NORM_BWD) {
        MPF_REQUIRE(t.grad_partials || !(stats || t.dweight || t.dbias), "%s: null pointer (%s.grad_partials)", who, name);
        d.gpartials = t.grad_partials;
    }
    if (what == NORM_BWD) {
        MPF_REQUIRE(t.dx, "%s: null pointer (%s.dx)", who, name);
        d.dx = t.dx, d.dw = t.dweight, d.db = t.dbias;
        all16 = all16 && mpf_aligned16(t.dx);
    }
    return 0;
}

template <int WHAT>
static int norm_launch(const MpfNormArgs *a, void *stream, const char *who)
{
    MPF_REQUIRE(a, "%s: null argument block", who);
    MPF_REQUIRE(a->N >= 1 && a->C >= 1 && a->H >= 1 && a->W >= 1, "%s: bad shape N, C, H, W = %d, %d, %d, %d", who, a->N, a->C, a->H, a->W);
    MPF_REQUIRE(a->chunks >= 1 && a->chunks <= MPF_NORM_MAX_CHUNKS, "%s: chunks must be 1..%d (got %d)", who, MPF_NORM_MAX_CHUNKS, a->chunks);
    const int64_t hw = (int64_t)a->H * a->W, planes = (int64_t)a->N * a->C, lim = ((int64_t)1 << 31) - 8192;
    MPF_REQUIRE(hw < lim && planes * hw < lim && planes * a->chunks < lim, "%s: N*C*max(H*W, chunks) must stay below 2^31 (%d, %d, %d, %d; chunks %d)", who,
                a->N, a->C, a->H, a->W, a->chunks);
    MPF_REQUIRE(a->y.x, "%s: null pointer (y.x)", who);
    MPF_REQUIRE(!(a->r.x && a->res), "%s: the residual is either the tensor res or the term r, not both", who);
    NormDev d = NormDev{};
    bool all16 = true;
    int rc = norm_term(a->y, a, WHAT, who, "y", d.t[0], all16);
    if (!rc) rc = norm_term(a->r, a, WHAT, who, "r", d.t[1], all16);
    if (rc) return rc;
    d.N = a->N, d.C = a->C, d.HW = (int)hw, d.chunks = a->chunks;
    d.L = (int)(((hw + a->chunks - 1) / a->chunks + 3) / 4 * 4);
    dim3 grid((unsigned)planes, (unsigned)a->chunks, 1);
    if (WHAT == NORM_STATS) {
        NormTermDev with[2];
        int n = 0;
        for (int j = 0; j < 2; ++j)
            if (d.t[j].x && d.t[j].partials) with[n++] = d.t[j];
        MPF_REQUIRE(n >= 1, "%s: no term has a mode with statistics (instance, batch_train, group)", who);
        all16 = true;
        for (int j = 0; j < n; ++j) d.t[j] = with[j], all16 = all16 && mpf_aligned16(with[j].x);
        grid.z = (unsigned)n;
    } else {
        if (a->res) all16 = all16 && mpf_aligned16(a->res);
        d.res = a->res;
        if (WHAT == NORM_ACT) {
            MPF_REQUIRE(a->out, "%s: null pointer (out)", who);
            d.out = a->out;
            all16 = all16 && mpf_aligned16(a->out);
        } else {
            MPF_REQUIRE(a->g, "%s: null pointer (g)", who);
            d.g = a->g;
            all16 = all16 && mpf_aligned16(a->g);
            if (WHAT == NORM_BWD && a->res) {
                MPF_REQUIRE(a->dres, "%s: null pointer (dres)", who);
                d.dres = a->dres, d.accumulate = a->accumulate != 0;
                all16 = all16 && mpf_aligned16(a->dres);
            }
        }
    }
    if (WHAT == NORM_BWD_REDUCE && !d.t[0].gpartials && !(d.t[1].x && d.t[1].gpartials)) return 0;     // nothing asks for a sum
    const bool vec = hw % 4 == 0 && all16;
    const hipStream_t s = (hipStream_t)stream;
#define NORM_GO(kernel)                                                                                \
    do {                                                                                               \
        if (vec)                                                                                       \
            hipLaunchKernelGGL((kernel<4>), grid, dim3(NORM_THREADS), 0, s, d);                        \
        else                                                                                           \
            hipLaunchKernelGGL((kernel<1>), grid, dim3(NORM_THREADS), 0, s, d);                        \
    } while (0)
    if (WHAT == NORM_STATS)
        NORM_GO(k_norm_stats);
    else if (WHAT == NORM_ACT)
        NORM_GO(k_norm_act);
    else if (WHAT == NORM_BWD_REDUCE)
        NORM_GO(k_norm_bwd_reduce);
    else
        NORM_GO(k_norm_bwd);
#undef NORM_GO
    return mpf_launch_status(who);
}

extern "C" int mpf_norm_stats(const MpfNormArgs *a, void *stream) { return norm_launch<NORM_STATS>(a, stream, "mpf_norm_stats"); }

extern "C" int mpf_norm_act(const MpfNormArgs *a, void *stream) { return norm_launch<NORM_ACT>(a, stream, "mpf_norm_act"); }

extern "C" int mpf_norm_act_backward_reduce(const MpfNormArgs *a, void *stream)
{
    return norm_launch<NORM_BWD_REDUCE>(a, stream, "mpf_norm_act_backward_reduce");
}

extern "C" int mpf_norm_act_backward(const MpfNormArgs *a, void *stream) { return norm_launch<NORM_BWD>(a, stream, "mpf_norm_act_backward"); }
