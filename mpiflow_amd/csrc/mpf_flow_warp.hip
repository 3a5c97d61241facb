// mpf_flow_warp.hip - the reference's backward warps by a flow field (utils/transform.py:60-111: warp and warp_rife) for gfx950, forward and adjoint.
//
// Contract: include/mpiflow_hip.h (MpfFlowWarpArgs); INTEGRATION.md section 22 holds the definitions, which tests/flow_warp_restated.py restates in
// float64.  The build has no contraction and correctly rounded divides; every operation below is rounded on its own.
//
// fw_taps          a pixel's sample position, built once: the coordinate by the mode's formula, the four tap offsets (-1: outside the image), the
//                  four one-dimensional weights and, for MPF_FLOW_WARP_RIFE, whether the border clamp passes a gradient.  A tap outside the image
//                  is never read; its value and its weight count as 0.  The floor is clamped to [-2, n + 1] before the cast, so a flow of any value
//                  (NaN, inf) ends outside the image instead of in an integer overflow.
// k_flow_warp      one thread per pixel, lanes along x (stores coalesce; for a smooth flow the gathers do too), the taps in registers, a loop over
//                  the channels of the thread's slice: grid.z cuts C into slices of MPF_FLOW_WARP_CHUNK channels (RAFT feature maps, C = 128 / 256,
//                  would otherwise leave the device to B * H * W / 256 workgroups).  The slice 0 writes the mask.
// k_flow_warp_bwd  the same walk.  grad_x: a float atomic add per tap and channel into a zeroed buffer (the last bits depend on the order of the
//                  adds).  grad_flow: per chunk of MPF_FLOW_WARP_CHUNK channels a sequential sum starting at 0, in torch's order (nw, ne, sw, se per
//                  channel), the chunk sums then added in chunk order.  One thread either walks every chunk (grid.z = 1) and stores the gradient, or
//                  takes one chunk (grid.z = chunks) and stores its partial; k_flow_warp_gf_sum then adds the partials in chunk order.  Both forms
//                  add the same numbers in the same order: the same bytes, without atomics, on every run.
//
// No workgroup waits for another; every loop is bounded by C; every tap offset is checked against the frame before it is used.
#include "mpf_common.h"
#include "mpf_math.h"
#include <math.h>

#define FW_THREADS 256
#define FW_CHUNK MPF_FLOW_WARP_CHUNK

struct FwTaps {
    int o_nw, o_ne, o_sw, o_se;                                 // y * W + x of each tap, or -1
    float wx0, wx1, wy0, wy1;                                   // ix - ix_nw, ix_se - ix, iy - iy_nw, iy_se - iy
    float mx, my;                                               // 1, or 0 where the border clamp of MPF_FLOW_WARP_RIFE stops the gradient
};

struct FwDev {
    const float *x, *flow, *lin_w, *lin_h, *g_out;
    float *out, *mask, *grad_x, *grad_flow, *partial;
    float sx, sy;                                               // d ix / d u and d iy / d v away from the clamp
    int C, H, W, mode, nchunks;
};

// torch's clip_coordinates_set_grad: [0, n - 1], no gradient at or past either bound; NaN goes to 0 without one
MPF_DEV float fw_clip(float v, int n, float *m)
{
    const float top = (float)(n - 1);
    if (!(v > 0.0f)) { *m = 0.0f; return 0.0f; }
    if (v >= top) { *m = 0.0f; return top; }
    *m = 1.0f;
    return v;
}

MPF_DEV int fw_cell(float f, int n) { return (int)fminf(fmaxf(f, -2.0f), (float)n + 1.0f); }          // fmaxf(NaN, -2) = -2: outside

MPF_DEV FwTaps fw_taps(const FwDev &a, const float *flow_b, int p)
{
    const int H = a.H, W = a.W;
    const int py = p / W, px = p - py * W;
    const float u = flow_b[p], v = flow_b[(size_t)H * W + p];
    float ix, iy;
    FwTaps t;
    if (a.mode == MPF_FLOW_WARP_WARP) {                         // normalised for align_corners=True, sampled at grid_sample's default (False): the reference's own
        const float gx = 2.0f * ((float)px + u) / (float)(W > 1 ? W - 1 : 1) - 1.0f;
        const float gy = 2.0f * ((float)py + v) / (float)(H > 1 ? H - 1 : 1) - 1.0f;
        ix = ((gx + 1.0f) * (float)W - 1.0f) / 2.0f;
        iy = ((gy + 1.0f) * (float)H - 1.0f) / 2.0f;
        t.mx = t.my = 1.0f;
    } else {                                                    // align_corners=True, border padding
        const float gx = a.lin_w[px] + u / ((float)(W - 1) / 2.0f);
        const float gy = a.lin_h[py] + v / ((float)(H - 1) / 2.0f);
        ix = fw_clip((gx + 1.0f) / 2.0f * (float)(W - 1), W, &t.mx);
        iy = fw_clip((gy + 1.0f) / 2.0f * (float)(H - 1), H, &t.my);
    }
    const float fx = floorf(ix), fy = floorf(iy);
    t.wx0 = ix - fx;
    t.wx1 = (fx + 1.0f) - ix;
    t.wy0 = iy - fy;
    t.wy1 = (fy + 1.0f) - iy;
    const int x0 = fw_cell(fx, W), y0 = fw_cell(fy, H);
    const bool x0in = x0 >= 0 && x0 < W, x1in = x0 + 1 >= 0 && x0 + 1 < W, y0in = y0 >= 0 && y0 < H, y1in = y0 + 1 >= 0 && y0 + 1 < H;
    t.o_nw = x0in && y0in ? y0 * W + x0 : -1;
    t.o_ne = x1in && y0in ? y0 * W + x0 + 1 : -1;
    t.o_sw = x0in && y1in ? (y0 + 1) * W + x0 : -1;
    t.o_se = x1in && y1in ? (y0 + 1) * W + x0 + 1 : -1;
    return t;
}

MPF_DEV float fw_read(const float *plane, int o) { return o >= 0 ? plane[o] : 0.0f; }

__global__ __launch_bounds__(FW_THREADS) void k_flow_warp(const FwDev a)
{
    const int hw = a.H * a.W;
    const int p = (int)(blockIdx.x * FW_THREADS + threadIdx.x);
    if (p >= hw) return;
    const int b = (int)blockIdx.y;
    const FwTaps t = fw_taps(a, a.flow + (size_t)b * 2 * hw, p);
    const float nw = t.o_nw >= 0 ? t.wx1 * t.wy1 : 0.0f, ne = t.o_ne >= 0 ? t.wx0 * t.wy1 : 0.0f;
    const float sw = t.o_sw >= 0 ? t.wx1 * t.wy0 : 0.0f, se = t.o_se >= 0 ? t.wx0 * t.wy0 : 0.0f;
    if (a.mask && blockIdx.z == 0) {
        float m = 0.0f;
        m += nw; m += ne; m += sw; m += se;
        a.mask[(size_t)b * hw + p] = m;
    }
    const int c0 = (int)blockIdx.z * FW_CHUNK, c1 = gridDim.z == 1 || c0 + FW_CHUNK > a.C ? a.C : c0 + FW_CHUNK;         // grid.z = 1: every channel
    const float *xc = a.x + ((size_t)b * a.C + c0) * hw;
    float *oc = a.out + ((size_t)b * a.C + c0) * hw + p;
#pragma unroll 4
    for (int c = c0; c < c1; ++c, xc += hw, oc += hw) {
        float acc = 0.0f;
        acc += fw_read(xc, t.o_nw) * nw;
        acc += fw_read(xc, t.o_ne) * ne;
        acc += fw_read(xc, t.o_sw) * sw;
        acc += fw_read(xc, t.o_se) * se;
        *oc = acc;
    }
}

template <bool GX, bool GF>
__global__ __launch_bounds__(FW_THREADS) void k_flow_warp_bwd(const FwDev a)
{
    const int hw = a.H * a.W;
    const int p = (int)(blockIdx.x * FW_THREADS + threadIdx.x);
    if (p >= hw) return;
    const int b = (int)blockIdx.y;
    const FwTaps t = fw_taps(a, a.flow + (size_t)b * 2 * hw, p);
    const float nw = t.wx1 * t.wy1, ne = t.wx0 * t.wy1, sw = t.wx1 * t.wy0, se = t.wx0 * t.wy0;
    const bool split = gridDim.z > 1;
    const int k0 = split ? (int)blockIdx.z : 0, k1 = split ? k0 + 1 : a.nchunks;
    float tx = 0.0f, ty = 0.0f;
    for (int k = k0; k < k1; ++k) {
        const int c0 = k * FW_CHUNK, c1 = c0 + FW_CHUNK < a.C ? c0 + FW_CHUNK : a.C;
        const float *gc = a.g_out + ((size_t)b * a.C + c0) * hw + p;
        const float *xc = a.x + ((size_t)b * a.C + c0) * hw;
        float *dc = GX ? a.grad_x + ((size_t)b * a.C + c0) * hw : nullptr;
        float gix = 0.0f, giy = 0.0f;
#pragma unroll 2
        for (int c = c0; c < c1; ++c, gc += hw, xc += hw, dc += hw) {
            const float g = *gc;
            if (GF) {
                const float v_nw = fw_read(xc, t.o_nw), v_ne = fw_read(xc, t.o_ne), v_sw = fw_read(xc, t.o_sw), v_se = fw_read(xc, t.o_se);
                gix -= v_nw * t.wy1 * g;  giy -= v_nw * t.wx1 * g;
                gix += v_ne * t.wy1 * g;  giy -= v_ne * t.wx0 * g;
                gix -= v_sw * t.wy0 * g;  giy += v_sw * t.wx1 * g;
                gix += v_se * t.wy0 * g;  giy += v_se * t.wx0 * g;
            }
            if (GX) {
                if (t.o_nw >= 0) atomicAdd(dc + t.o_nw, nw * g);
                if (t.o_ne >= 0) atomicAdd(dc + t.o_ne, ne * g);
                if (t.o_sw >= 0) atomicAdd(dc + t.o_sw, sw * g);
                if (t.o_se >= 0) atomicAdd(dc + t.o_se, se * g);
            }
        }
        if (k == k0) { tx = gix; ty = giy; }
        else { tx += gix; ty += giy; }
    }
    if (GF) {
        tx = t.mx != 0.0f ? tx : 0.0f;                          // a select, not a product: +0 whatever the sum's sign, in a chunk's share as in the whole sum
        ty = t.my != 0.0f ? ty : 0.0f;
        if (split) {
            float *pp = a.partial + ((size_t)blockIdx.z * gridDim.y + b) * 2 * hw + p;
            pp[0] = tx;
            pp[hw] = ty;
        } else {
            float *gf = a.grad_flow + (size_t)b * 2 * hw + p;
            gf[0] = a.sx * tx;
            gf[hw] = a.sy * ty;
        }
    }
}

// partial [chunks][B][2][H*W] -> grad_flow [B][2][H*W]: the chunks' shares added in chunk order
__global__ __launch_bounds__(FW_THREADS) void k_flow_warp_gf_sum(const float *__restrict__ partial, float *__restrict__ grad_flow, int nchunks, int hw,
                                                                 size_t per_chunk, float sx, float sy)
{
    const int p = (int)(blockIdx.x * FW_THREADS + threadIdx.x);
    if (p >= hw) return;
    const size_t o = (size_t)blockIdx.y * hw + p;               // blockIdx.y = b * 2 + component
    float tot = partial[o];
    for (int k = 1; k < nchunks; ++k) tot += partial[(size_t)k * per_chunk + o];
    grad_flow[o] = ((blockIdx.y & 1) ? sy : sx) * tot;
}

static int fw_chunks(int C) { return (C + FW_CHUNK - 1) / FW_CHUNK; }

static bool fw_shape_ok(int B, int C, int H, int W)
{
    return B >= 1 && B <= 32767 && C >= 1 && H >= 1 && W >= 1 && (int64_t)H * W <= ((int64_t)1 << 30) && (int64_t)B * C * H * W < ((int64_t)1 << 31) &&
           (int64_t)B * 2 * H * W < ((int64_t)1 << 31) && fw_chunks(C) <= 65535;
}

extern "C" size_t mpf_flow_warp_workspace(int B, int C, int H, int W, int whole)
{
    if (!fw_shape_ok(B, C, H, W)) return 0;
    const int n = fw_chunks(C);
    return n > 1 && !whole ? (size_t)n * B * 2 * H * W * sizeof(float) : 0;
}

static int fw_check(const MpfFlowWarpArgs *a, const char *who, FwDev *d)
{
    MPF_REQUIRE(a, "%s: null argument block", who);
    MPF_REQUIRE(a->mode == MPF_FLOW_WARP_WARP || a->mode == MPF_FLOW_WARP_RIFE, "%s: mode must be 0 (warp) or 1 (warp_rife) (got %d)", who, a->mode);
    MPF_REQUIRE(fw_shape_ok(a->B, a->C, a->H, a->W),
                "%s: bad shape: B must be 1..32767, C, H, W at least 1, H * W at most 2^30, B * C * H * W and B * 2 * H * W below 2^31 and C below %d "
                "(got B, C, H, W = %d, %d, %d, %d)", who, 65535 * FW_CHUNK, a->B, a->C, a->H, a->W);
    if (a->mode == MPF_FLOW_WARP_RIFE) {
        MPF_REQUIRE(a->H >= 2 && a->W >= 2, "%s: warp_rife needs H and W of at least 2 (got H, W = %d, %d): its scale (W - 1) / 2 is 0 at one pixel", who, a->H, a->W);
        MPF_REQUIRE(a->lin_w && a->lin_h, "%s: null pointer (lin_w, lin_h): warp_rife reads torch.linspace(-1, 1, W) and (-1, 1, H)", who);
        MPF_REQUIRE(!a->mask, "%s: warp_rife has no mask", who);
    }
    MPF_REQUIRE(a->x && a->flow, "%s: null pointer (x, flow)", who);
    d->x = a->x; d->flow = a->flow; d->lin_w = a->lin_w; d->lin_h = a->lin_h; d->g_out = a->grad_out;
    d->out = a->out; d->mask = a->mask; d->grad_x = a->grad_x; d->grad_flow = a->grad_flow; d->partial = (float *)a->workspace;
    d->C = a->C; d->H = a->H; d->W = a->W; d->mode = a->mode; d->nchunks = fw_chunks(a->C);
    if (a->mode == MPF_FLOW_WARP_WARP) {
        d->sx = (float)a->W / (float)(a->W > 1 ? a->W - 1 : 1);
        d->sy = (float)a->H / (float)(a->H > 1 ? a->H - 1 : 1);
    } else {
        d->sx = d->sy = 1.0f;
    }
    return 0;
}

extern "C" int mpf_flow_warp(const MpfFlowWarpArgs *a, void *stream)
{
    const char *who = "mpf_flow_warp";
    FwDev d;
    const int rc = fw_check(a, who, &d);
    if (rc) return rc;
    MPF_REQUIRE(a->out, "%s: null pointer (out)", who);
    const int hw = a->H * a->W;
    const dim3 grid((unsigned)((hw + FW_THREADS - 1) / FW_THREADS), (unsigned)a->B, (unsigned)(a->whole ? 1 : d.nchunks));
    hipLaunchKernelGGL(k_flow_warp, grid, dim3(FW_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_flow_warp");
}

extern "C" int mpf_flow_warp_bwd(const MpfFlowWarpArgs *a, void *stream)
{
    const char *who = "mpf_flow_warp_bwd";
    FwDev d;
    const int rc = fw_check(a, who, &d);
    if (rc) return rc;
    MPF_REQUIRE(a->grad_out, "%s: null pointer (grad_out)", who);
    MPF_REQUIRE(a->grad_x || a->grad_flow, "%s: null pointer (grad_x and grad_flow): one gradient at least", who);
    const bool cut = d.nchunks > 1 && !a->whole;
    if (cut && a->grad_flow) {
        const size_t need = mpf_flow_warp_workspace(a->B, a->C, a->H, a->W, 0);
        MPF_REQUIRE(a->workspace && a->workspace_bytes >= need, "%s: workspace of %zu bytes needed for the chunks' shares of grad_flow (got %zu)", who, need,
                    a->workspace_bytes);
    }
    const int hw = a->H * a->W;
    const dim3 grid((unsigned)((hw + FW_THREADS - 1) / FW_THREADS), (unsigned)a->B, (unsigned)(cut ? d.nchunks : 1));
    if (a->grad_x && a->grad_flow) hipLaunchKernelGGL((k_flow_warp_bwd<true, true>), grid, dim3(FW_THREADS), 0, (hipStream_t)stream, d);
    else if (a->grad_x) hipLaunchKernelGGL((k_flow_warp_bwd<true, false>), grid, dim3(FW_THREADS), 0, (hipStream_t)stream, d);
    else hipLaunchKernelGGL((k_flow_warp_bwd<false, true>), grid, dim3(FW_THREADS), 0, (hipStream_t)stream, d);
    const int st = mpf_launch_status("k_flow_warp_bwd");
    if (st || !(cut && a->grad_flow)) return st;
    const dim3 sgrid((unsigned)((hw + FW_THREADS - 1) / FW_THREADS), (unsigned)(2 * a->B));
    hipLaunchKernelGGL(k_flow_warp_gf_sum, sgrid, dim3(FW_THREADS), 0, (hipStream_t)stream, (const float *)d.partial, a->grad_flow, d.nchunks, hw,
                       (size_t)a->B * 2 * hw, d.sx, d.sy);
    return mpf_launch_status("k_flow_warp_gf_sum");
}
