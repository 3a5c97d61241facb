// mpf_raft_glue.hip - what RAFT.forward (RAFT/core/raft.py:86-144) does between its modules, for gfx950: the image scaling, the split of the
// context network's output, and the small model's bilinear 8x upsampling (utils/utils.py:80-82) with its gradient.
//
// Contract: include/mpiflow_hip.h (MpfRaftGlueArgs).
//
// k_raft_images            pair[2N,3,H,W] = 2 * (x / 255) - 1 of image1 (first N) and image2 (last N): the batch the feature network consumes,
//                          its first half what the context network consumes; no cat.  A TRUE fp32 division (the library is built with the
//                          correctly rounded divide), as torch's CPU kernel computes the expression the reference was recorded with.
// k_context_split          net = tanh(cnet[:, :hdim]), inp = relu(cnet[:, hdim:]), both contiguous, one pass over cnet
// k_context_split_bwd      grad_cnet[:, :hdim] = g_net * (1 - net^2), grad_cnet[:, hdim:] = g_inp where !(inp <= 0): from the saved OUTPUTS, one
//                          [N,hdim+cdim,H,W] gradient, no cat
// k_upflow8                out[N,2,8H,8W] = 8 * bilinear(flow), align_corners=True: source coordinate = dst * scale, scale = (H-1)/(8H-1) in fp32
//                          (0 for H == 1), i0 = (int)src, i1 = i0 + (i0 < H-1), l = src - i0, value = (1-ly)*((1-lx)*v00 + lx*v01) + ly*((1-lx)*v10
//                          + lx*v11): ATen's upsample_bilinear2d, operation for operation
// k_upflow8_bwd            one lane per COARSE element: gathers the fine pixels whose footprint touches it - the candidates are a range computed
//                          with a margin, each tested with the forward kernel's own (i0, i1, l) - weights summed in fp64 in a fixed order.  No
//                          atomics: bit-identical from run to run.
//
// Layout: the pointwise kernels give a lane 4 consecutive floats (one 16-byte access) where the plane size is a multiple of 4 and every
// pointer is 16-byte aligned, one float otherwise; at most GLUE_MAX_BLOCKS blocks, grid-stride over the rest.  k_upflow8 gives a lane 4
// consecutive outputs of one fine row (8W is a multiple of 4); its reads of the 64 x smaller coarse map hit the cache.  No LDS.
// No address depends on a tensor's values: NaN and inf travel through the arithmetic as in torch.
#include "mpf_common.h"
#include "mpf_math.h"
#include "mpf_raft_scale.h"     // raft_scale: shared with the padded batch of mpf_raft_eval.hip
#include "mpf_upflow8.h"        // up8_taps, up8_range, up8_weight, up8_value: shared with the fused bilinear loss of mpf_upsample.hip

#define GLUE_THREADS 256
#define GLUE_MAX_BLOCKS 2048

static unsigned glue_blocks(int64_t lanes)
{
    int64_t blocks = (lanes + GLUE_THREADS - 1) / GLUE_THREADS;
    return (unsigned)(blocks > GLUE_MAX_BLOCKS ? GLUE_MAX_BLOCKS : blocks);
}

// every loop below: t < total < 2^31 and the stride is at most GLUE_MAX_BLOCKS * GLUE_THREADS = 2^19, so the last increment cannot wrap

template <int VEC>
__global__ __launch_bounds__(GLUE_THREADS) void k_raft_images(const float *im1, const float *im2, float *pair, unsigned per, unsigned total)
{
    for (unsigned t = blockIdx.x * GLUE_THREADS + threadIdx.x; t < total; t += gridDim.x * GLUE_THREADS) {
        const float *src = t < per ? im1 + (size_t)t * VEC : im2 + (size_t)(t - per) * VEC;
        float v[VEC];
        mpf_load_vec<VEC>(src, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = raft_scale(v[e]);
        mpf_store_vec<VEC>(pair + (size_t)t * VEC, v);
    }
}

struct SplitDev {
    const float *cnet, *g_net, *g_inp;       // forward: cnet; backward: the two cotangents
    float *net, *inp, *grad_cnet;            // forward: written; backward: net and inp are READ, grad_cnet written
    int hdim, cdim, HW;
    unsigned total;                          // lanes = N * (hdim + cdim) * HW / VEC
};

template <bool BWD, int VEC>
__global__ __launch_bounds__(GLUE_THREADS) void k_context_split(const SplitDev a)
{
    const unsigned per_plane = (unsigned)(a.HW / VEC);
    const int C = a.hdim + a.cdim;
    for (unsigned t = blockIdx.x * GLUE_THREADS + threadIdx.x; t < a.total; t += gridDim.x * GLUE_THREADS) {
        const int plane = (int)(t / per_plane), i = (int)(t - (unsigned)plane * per_plane) * VEC;
        const int n = plane / C, c = plane - n * C;
        const bool is_net = c < a.hdim;                                   // uniform per plane
        const size_t flat = (size_t)plane * a.HW + i;                     // inside [N,hdim+cdim,H,W]
        const size_t part = is_net ? ((size_t)n * a.hdim + c) * a.HW + i : ((size_t)n * a.cdim + (c - a.hdim)) * a.HW + i;
        float v[VEC], o[VEC];
        if (!BWD) {
            mpf_load_vec<VEC>(a.cnet + flat, v);
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = is_net ? tanhf(v[e]) : (v[e] < 0.0f ? 0.0f : v[e]);
            mpf_store_vec<VEC>((is_net ? a.net : a.inp) + part, o);
        } else {
            float g[VEC];
            mpf_load_vec<VEC>((is_net ? a.net : a.inp) + part, v);
            mpf_load_vec<VEC>((is_net ? a.g_net : a.g_inp) + part, g);
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = is_net ? g[e] * (1.0f - v[e] * v[e]) : (v[e] <= 0.0f ? 0.0f : g[e]);
            mpf_store_vec<VEC>(a.grad_cnet + flat, o);
        }
    }
}

struct Up8Dev {
    const float *in;             // forward: flow [N,2,H,W]; backward: the cotangent [N,2,8H,8W]
    float *out;                  // forward: [N,2,8H,8W]; backward: grad_flow [N,2,H,W]
    int H, W;
    float sy, sx;                // (H-1)/(8H-1), (W-1)/(8W-1) in fp32
    unsigned total;
};

template <int VEC>
__global__ __launch_bounds__(GLUE_THREADS) void k_upflow8(const Up8Dev a)
{
    const int W8 = 8 * a.W, H8 = 8 * a.H;
    const unsigned per_row = (unsigned)(W8 / VEC);
    for (unsigned t = blockIdx.x * GLUE_THREADS + threadIdx.x; t < a.total; t += gridDim.x * GLUE_THREADS) {
        const unsigned row = t / per_row;
        const int X = (int)(t - row * per_row) * VEC;
        const int plane = (int)(row / (unsigned)H8), Y = (int)(row - (unsigned)plane * H8);
        int y0, y1;
        float ly;
        up8_taps(Y, a.H, a.sy, y0, y1, ly);
        const float *p0 = a.in + ((size_t)plane * a.H + y0) * a.W, *p1 = a.in + ((size_t)plane * a.H + y1) * a.W;
        const float hy = 1.0f - ly;
        float o[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            int x0, x1;
            float lx;
            up8_taps(X + e, a.W, a.sx, x0, x1, lx);
            const float hx = 1.0f - lx;
            o[e] = up8_value(p0, p1, x0, x1, hy, ly, hx, lx);
        }
        mpf_store_vec<VEC>(a.out + (size_t)row * W8 + X, o);
    }
}

__global__ __launch_bounds__(GLUE_THREADS) void k_upflow8_bwd(const Up8Dev a)
{
    const int W8 = 8 * a.W, H8 = 8 * a.H;
    for (unsigned t = blockIdx.x * GLUE_THREADS + threadIdx.x; t < a.total; t += gridDim.x * GLUE_THREADS) {
        const unsigned row = t / (unsigned)a.W;
        const int x = (int)(t - row * (unsigned)a.W);
        const int plane = (int)(row / (unsigned)a.H), y = (int)(row - (unsigned)plane * a.H);
        int ylo, yhi, xlo, xhi;
        up8_range(y, a.H, ylo, yhi);
        up8_range(x, a.W, xlo, xhi);
        const float *g = a.in + (size_t)plane * H8 * W8;
        double acc = 0.0;
        for (int Y = ylo; Y <= yhi; ++Y) {
            const float wy = up8_weight(Y, y, a.H, a.sy);
            if (wy == 0.0f) continue;
            const float *grow = g + (size_t)Y * W8;
            double rsum = 0.0;
            for (int X = xlo; X <= xhi; ++X) rsum += (double)up8_weight(X, x, a.W, a.sx) * (double)grow[X];
            acc += (double)wy * rsum;
        }
        a.out[t] = (float)(8.0 * acc);
    }
}

static int glue_shape(const MpfRaftGlueArgs *a, const char *who, int64_t channels, int64_t scale, int64_t &hw, int64_t &n)
{
    MPF_REQUIRE(a, "%s: null argument block", who);
    MPF_REQUIRE(a->N >= 1 && a->H >= 1 && a->W >= 1, "%s: bad shape N, H, W = %d, %d, %d", who, a->N, a->H, a->W);
    hw = (int64_t)a->H * a->W;
    n = (int64_t)a->N * channels * hw;
    MPF_REQUIRE(n * scale < ((int64_t)1 << 31), "%s: every tensor must hold fewer than 2^31 elements (N, H, W = %d, %d, %d)", who, a->N, a->H, a->W);
    return 0;
}

extern "C" int mpf_raft_images(const MpfRaftGlueArgs *a, void *stream)
{
    const char *who = "mpf_raft_images";
    int64_t hw, n;
    const int rc = glue_shape(a, who, 3, 2, hw, n);
    if (rc) return rc;
    MPF_REQUIRE(a->image1 && a->image2 && a->pair, "%s: null pointer (image1, image2 or pair)", who);
    const bool vec = n % 4 == 0 && mpf_aligned16(a->image1) && mpf_aligned16(a->image2) && mpf_aligned16(a->pair);
    const int64_t per = vec ? n / 4 : n;
    if (vec)
        hipLaunchKernelGGL((k_raft_images<4>), dim3(glue_blocks(2 * per)), dim3(GLUE_THREADS), 0, (hipStream_t)stream, a->image1, a->image2, a->pair,
                           (unsigned)per, (unsigned)(2 * per));
    else
        hipLaunchKernelGGL((k_raft_images<1>), dim3(glue_blocks(2 * per)), dim3(GLUE_THREADS), 0, (hipStream_t)stream, a->image1, a->image2, a->pair,
                           (unsigned)per, (unsigned)(2 * per));
    return mpf_launch_status("k_raft_images");
}

template <bool BWD>
static int split_launch(const MpfRaftGlueArgs *a, void *stream, const char *who)
{
    MPF_REQUIRE(a, "%s: null argument block", who);
    MPF_REQUIRE(a->hdim >= 1 && a->cdim >= 1, "%s: hdim and cdim must be positive (got %d, %d)", who, a->hdim, a->cdim);
    int64_t hw, n;
    const int rc = glue_shape(a, who, (int64_t)a->hdim + a->cdim, 1, hw, n);
    if (rc) return rc;
    MPF_REQUIRE(a->net && a->inp, "%s: null pointer (net or inp)", who);
    SplitDev d = SplitDev{};
    bool all16 = mpf_aligned16(a->net) && mpf_aligned16(a->inp);
    if (!BWD) {
        MPF_REQUIRE(a->cnet, "%s: null pointer (cnet)", who);
        all16 = all16 && mpf_aligned16(a->cnet);
    } else {
        MPF_REQUIRE(a->g_net && a->g_inp && a->grad_cnet, "%s: null pointer (g_net, g_inp or grad_cnet)", who);
        all16 = all16 && mpf_aligned16(a->g_net) && mpf_aligned16(a->g_inp) && mpf_aligned16(a->grad_cnet);
    }
    d.cnet = a->cnet, d.g_net = a->g_net, d.g_inp = a->g_inp, d.net = a->net, d.inp = a->inp, d.grad_cnet = a->grad_cnet;
    d.hdim = a->hdim, d.cdim = a->cdim, d.HW = (int)hw;
    const bool vec = hw % 4 == 0 && all16;
    d.total = (unsigned)(vec ? n / 4 : n);
    if (vec)
        hipLaunchKernelGGL((k_context_split<BWD, 4>), dim3(glue_blocks(d.total)), dim3(GLUE_THREADS), 0, (hipStream_t)stream, d);
    else
        hipLaunchKernelGGL((k_context_split<BWD, 1>), dim3(glue_blocks(d.total)), dim3(GLUE_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_context_split");
}

extern "C" int mpf_context_split(const MpfRaftGlueArgs *a, void *stream) { return split_launch<false>(a, stream, "mpf_context_split"); }

extern "C" int mpf_context_split_backward(const MpfRaftGlueArgs *a, void *stream)
{
    return split_launch<true>(a, stream, "mpf_context_split_backward");
}

static int up8_dev(const MpfRaftGlueArgs *a, const char *who, const float *in, float *out, Up8Dev &d, int64_t &coarse)
{
    int64_t hw;
    const int rc = glue_shape(a, who, 2, 64, hw, coarse);
    if (rc) return rc;
    MPF_REQUIRE(in && out, "%s: null pointer", who);
    d.in = in, d.out = out, d.H = a->H, d.W = a->W;
    d.sy = up8_scale(a->H), d.sx = up8_scale(a->W);
    return 0;
}

extern "C" int mpf_upflow8(const MpfRaftGlueArgs *a, void *stream)
{
    Up8Dev d = Up8Dev{};
    int64_t coarse;
    const int rc = up8_dev(a, "mpf_upflow8", a ? a->flow : nullptr, a ? a->flow_up : nullptr, d, coarse);
    if (rc) return rc;
    const bool vec = mpf_aligned16(a->flow_up);                           // 8W % 4 == 0: every fine row then starts 16-byte aligned
    d.total = (unsigned)(vec ? coarse * 16 : coarse * 64);
    if (vec)
        hipLaunchKernelGGL((k_upflow8<4>), dim3(glue_blocks(d.total)), dim3(GLUE_THREADS), 0, (hipStream_t)stream, d);
    else
        hipLaunchKernelGGL((k_upflow8<1>), dim3(glue_blocks(d.total)), dim3(GLUE_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_upflow8");
}

extern "C" int mpf_upflow8_backward(const MpfRaftGlueArgs *a, void *stream)
{
    Up8Dev d = Up8Dev{};
    int64_t coarse;
    const int rc = up8_dev(a, "mpf_upflow8_backward", a ? a->g_up : nullptr, a ? a->grad_flow : nullptr, d, coarse);
    if (rc) return rc;
    d.total = (unsigned)coarse;
    hipLaunchKernelGGL(k_upflow8_bwd, dim3(glue_blocks(d.total)), dim3(GLUE_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_upflow8_bwd");
}
