// mpf_gru.hip - the pointwise work of RAFT's convolutional GRU (ConvGRU / SepConvGRU, RAFT/core/update.py:16-60) for gfx950, fused: everything
// between the gate convolutions, forward and gradient, in four kernels.
//
// Contract: include/mpiflow_hip.h (MpfGruTerm, MpfGruArgs).  A pre-activation is the sum of up to three TERMS, each a channel slice of an NCHW
// tensor read in place (pointer, channels of that tensor, channel offset): a convolution over cat([h, x]) is the sum of one over h and one over
// x, so the concatenations never exist, and a [B,3C,H,W] convolution output hands its z, r and q slices over without a copy.
//
// k_gru<GRU_RESET>        rh = sigmoid(sum r-terms) * h
// k_gru<GRU_UPDATE>       z = sigmoid(sum z-terms), q = tanh(sum q-terms), h' = (1 - z) * h + z * q          (nothing else is written)
// k_gru<GRU_UPDATE_BWD>   recomputes z and q from the same terms; d pre_z = g (q - h) z (1 - z), d pre_q = g z (1 - q^2), d h = g (1 - z)
// k_gru<GRU_RESET_BWD>    recomputes r; d pre_r = g h r (1 - r), d h (+)= g r
// The gradients of the pre-activations are written as slices too, each to up to two destinations (the same values are the gradient of every
// term of the sum, and the convolutions' backward passes want them inside contiguous [B,3C,H,W] and [B,2C,H,W] tensors).
//
// Layout: lane = 4 consecutive floats (one 16-byte access) of the flat H*W index of one (b, channel) plane when H*W % 4 == 0 and every pointer
// is 16-byte aligned - then every plane of every slice starts 16-byte aligned - and one float otherwise.  A wave's access to one tensor is one
// contiguous run of 1 KiB (256 bytes on the scalar path) except where it crosses a plane boundary.  Grid: at most GRU_MAX_BLOCKS blocks, grid-stride over the rest.
// Pure streaming: 2 - 8 tensors read, 1 - 5 written, no reuse, no LDS, no atomics: every result is bit-identical from run to run.
//
// Numerics: sigmoid(x) = 1 / (1 + expf(-x)) with the correctly rounded divide the library is built with and ocml's expf / tanhf (about 1 ulp);
// the fast-math forms (__expf, a tanh from one __expf) are not used: their absolute error near saturation is several ulp of 1, beyond 3 x the
// fp32 run's own error that the tests allow.  No address depends on a tensor's values: NaN and inf travel through the arithmetic as in torch.
#include "mpf_common.h"
#include "mpf_math.h"

#define GRU_THREADS 256
#define GRU_MAX_BLOCKS 2048

enum { GRU_RESET = 0, GRU_UPDATE = 1, GRU_UPDATE_BWD = 2, GRU_RESET_BWD = 3 };

struct GruSlice {                // element (b, c, i) of the slice: p[b * bstride + c * HW + i], the channel offset already folded into p
    float *p;
    int bstride;
};

struct GruDev {
    GruSlice z[MPF_GRU_MAX_TERMS], r[MPF_GRU_MAX_TERMS], q[MPF_GRU_MAX_TERMS];
    GruSlice dz[2], dr[2], dq[2];
    const float *h, *g;
    float *out, *dh;
    int accumulate;
    int C, HW, total;            // total: lanes of work = B * C * HW / VEC
};

// the sum of the present terms, in term order; the launcher guarantees that one is present
template <int VEC>
__device__ __forceinline__ void gru_sum(const GruSlice (&t)[MPF_GRU_MAX_TERMS], int b, int off, float (&s)[VEC])
{
    bool first = true;
#pragma unroll
    for (int k = 0; k < MPF_GRU_MAX_TERMS; ++k) {
        if (!t[k].p) continue;                                // uniform: a kernel argument
        float v[VEC];
        mpf_load_vec<VEC>(t[k].p + (size_t)b * t[k].bstride + off, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) s[e] = first ? v[e] : s[e] + v[e];
        first = false;
    }
}

template <int VEC>
__device__ __forceinline__ void gru_store_slices(const GruSlice (&d)[2], int b, int off, const float (&v)[VEC])
{
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (d[k].p) mpf_store_vec<VEC>(d[k].p + (size_t)b * d[k].bstride + off, v);
}

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int MODE, int VEC>
__global__ __launch_bounds__(GRU_THREADS) void k_gru(const GruDev a)
{
    const int per_plane = a.HW / VEC;
    // unsigned: total < 2^31 and the stride is at most GRU_MAX_BLOCKS * GRU_THREADS = 2^19, so the last increment cannot wrap
    for (unsigned t = blockIdx.x * GRU_THREADS + threadIdx.x; t < (unsigned)a.total; t += gridDim.x * GRU_THREADS) {
        const int plane = (int)(t / (unsigned)per_plane), i = ((int)t - plane * per_plane) * VEC;
        const int b = plane / a.C, c = plane - b * a.C;
        const int off = c * a.HW + i;                         // inside one sample of a slice
        const size_t flat = (size_t)plane * a.HW + i;         // inside a [B,C,H,W] tensor
        float h[VEC], o[VEC];
        mpf_load_vec<VEC>(a.h + flat, h);
        if (MODE == GRU_RESET) {
            float s[VEC];
            gru_sum<VEC>(a.r, b, off, s);
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = gru_sigmoid(s[e]) * h[e];
            mpf_store_vec<VEC>(a.out + flat, o);
        } else if (MODE == GRU_RESET_BWD) {
            float s[VEC], g[VEC], dr[VEC], dh[VEC];
            gru_sum<VEC>(a.r, b, off, s);
            mpf_load_vec<VEC>(a.g + flat, g);
            if (a.accumulate) {
                mpf_load_vec<VEC>(a.dh + flat, dh);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) dh[e] = 0.0f;
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float r = gru_sigmoid(s[e]);
                dr[e] = (g[e] * h[e]) * (r * (1.0f - r));
                dh[e] = a.accumulate ? dh[e] + g[e] * r : g[e] * r;
            }
            gru_store_slices<VEC>(a.dr, b, off, dr);
            mpf_store_vec<VEC>(a.dh + flat, dh);
        } else {
            float sz[VEC], sq[VEC];
            gru_sum<VEC>(a.z, b, off, sz);
            gru_sum<VEC>(a.q, b, off, sq);
            if (MODE == GRU_UPDATE) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float z = gru_sigmoid(sz[e]), q = tanhf(sq[e]);
                    o[e] = (1.0f - z) * h[e] + z * q;
                }
                mpf_store_vec<VEC>(a.out + flat, o);
            } else {
                float g[VEC], dz[VEC], dq[VEC], dh[VEC];
                mpf_load_vec<VEC>(a.g + flat, g);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float z = gru_sigmoid(sz[e]), q = tanhf(sq[e]);
                    dz[e] = (g[e] * (q - h[e])) * (z * (1.0f - z));
                    dq[e] = (g[e] * z) * (1.0f - q * q);
                    dh[e] = g[e] * (1.0f - z);
                }
                gru_store_slices<VEC>(a.dz, b, off, dz);
                gru_store_slices<VEC>(a.dq, b, off, dq);
                mpf_store_vec<VEC>(a.dh + flat, dh);
            }
        }
    }
}

// one slice: folds the channel offset into the pointer; `all16` is cleared by a pointer that is not 16-byte aligned
static int gru_slice(const MpfGruTerm &t, const MpfGruArgs *a, const char *who, const char *name, int k, GruSlice &s, bool &all16)
{
    s = GruSlice{nullptr, 0};
    if (!t.p) return 0;
    const int64_t hw = (int64_t)a->H * a->W;
    MPF_REQUIRE(t.channels >= 1 && t.offset >= 0, "%s: %s[%d] has channels %d, offset %d", who, name, k, t.channels, t.offset);
    MPF_REQUIRE((int64_t)t.offset + a->C <= t.channels, "%s: %s[%d]: offset + C = %d + %d exceeds its tensor's %d channels", who, name, k, t.offset,
                a->C, t.channels);
    MPF_REQUIRE((int64_t)a->B * t.channels * hw < ((int64_t)1 << 31), "%s: the tensor of %s[%d] must hold fewer than 2^31 elements", who, name, k);
    s.p = t.p + (int64_t)t.offset * hw;
    s.bstride = (int)(t.channels * hw);
    all16 = all16 && mpf_aligned16(s.p);
    return 0;
}

static int gru_terms(const MpfGruTerm *t, int n, const MpfGruArgs *a, const char *who, const char *name, GruSlice *out, bool &all16)
{
    MPF_REQUIRE(n >= 1 && n <= MPF_GRU_MAX_TERMS, "%s: %s must count 1..%d terms (got %d)", who, name, MPF_GRU_MAX_TERMS, n);
    bool any = false;
    for (int k = 0; k < MPF_GRU_MAX_TERMS; ++k) {
        out[k] = GruSlice{nullptr, 0};
        if (k >= n) continue;
        const int rc = gru_slice(t[k], a, who, name, k, out[k], all16);
        if (rc) return rc;
        any = any || out[k].p;
    }
    MPF_REQUIRE(any, "%s: null pointer (every term of %s is absent)", who, name);
    return 0;
}

static int gru_dests(const MpfGruTerm *t, const MpfGruArgs *a, const char *who, const char *name, GruSlice *out, bool &all16)
{
    MPF_REQUIRE(t[0].p, "%s: null pointer (%s[0])", who, name);
    for (int k = 0; k < 2; ++k) {
        const int rc = gru_slice(t[k], a, who, name, k, out[k], all16);
        if (rc) return rc;
    }
    return 0;
}

template <int MODE>
static int gru_launch(const MpfGruArgs *a, void *stream, const char *who)
{
    MPF_REQUIRE(a, "%s: null argument block", who);
    MPF_REQUIRE(a->B >= 1 && a->C >= 1 && a->H >= 1 && a->W >= 1, "%s: bad shape B, C, H, W = %d, %d, %d, %d", who, a->B, a->C, a->H, a->W);
    const int64_t hw = (int64_t)a->H * a->W, n = (int64_t)a->B * a->C * hw;
    MPF_REQUIRE(hw < ((int64_t)1 << 31) && n < ((int64_t)1 << 31), "%s: [B,C,H,W] must hold fewer than 2^31 elements (%d, %d, %d, %d)", who, a->B,
                a->C, a->H, a->W);
    MPF_REQUIRE(a->h, "%s: null pointer (h)", who);
    constexpr bool kBwd = MODE == GRU_UPDATE_BWD || MODE == GRU_RESET_BWD, kReset = MODE == GRU_RESET || MODE == GRU_RESET_BWD;
    GruDev d = GruDev{};
    bool all16 = mpf_aligned16(a->h);
    int rc = 0;
    if (kReset) {
        rc = gru_terms(a->r, a->nr, a, who, "r", d.r, all16);
    } else {
        rc = gru_terms(a->z, a->nz, a, who, "z", d.z, all16);
        if (!rc) rc = gru_terms(a->q, a->nq, a, who, "q", d.q, all16);
    }
    if (rc) return rc;
    if (!kBwd) {
        MPF_REQUIRE(a->out, "%s: null pointer (out)", who);
        all16 = all16 && mpf_aligned16(a->out);
    } else {
        MPF_REQUIRE(a->g, "%s: null pointer (g)", who);
        MPF_REQUIRE(a->dh, "%s: null pointer (dh)", who);
        all16 = all16 && mpf_aligned16(a->g) && mpf_aligned16(a->dh);
        if (kReset) {
            rc = gru_dests(a->dr, a, who, "dr", d.dr, all16);
        } else {
            rc = gru_dests(a->dz, a, who, "dz", d.dz, all16);
            if (!rc) rc = gru_dests(a->dq, a, who, "dq", d.dq, all16);
        }
        if (rc) return rc;
    }
    d.h = a->h, d.g = a->g, d.out = a->out, d.dh = a->dh;
    d.accumulate = MODE == GRU_RESET_BWD && a->accumulate != 0;
    d.C = a->C, d.HW = (int)hw;
    const bool vec = hw % 4 == 0 && all16;
    d.total = (int)(vec ? n / 4 : n);
    int64_t blocks = ((int64_t)d.total + GRU_THREADS - 1) / GRU_THREADS;
    if (blocks > GRU_MAX_BLOCKS) blocks = GRU_MAX_BLOCKS;
    if (vec)
        hipLaunchKernelGGL((k_gru<MODE, 4>), dim3((unsigned)blocks), dim3(GRU_THREADS), 0, (hipStream_t)stream, d);
    else
        hipLaunchKernelGGL((k_gru<MODE, 1>), dim3((unsigned)blocks), dim3(GRU_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_gru");
}

extern "C" int mpf_gru_reset(const MpfGruArgs *a, void *stream) { return gru_launch<GRU_RESET>(a, stream, "mpf_gru_reset"); }

extern "C" int mpf_gru_update(const MpfGruArgs *a, void *stream) { return gru_launch<GRU_UPDATE>(a, stream, "mpf_gru_update"); }

extern "C" int mpf_gru_update_backward(const MpfGruArgs *a, void *stream)
{
    return gru_launch<GRU_UPDATE_BWD>(a, stream, "mpf_gru_update_backward");
}

extern "C" int mpf_gru_reset_backward(const MpfGruArgs *a, void *stream)
{
    return gru_launch<GRU_RESET_BWD>(a, stream, "mpf_gru_reset_backward");
}
