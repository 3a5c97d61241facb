// mpf_render_bwd.hip - adjoints of the utils/mpi renderer with respect to the per-plane VALUES (colour, density, extras); geometry is constant.
//
//   k_volume_render_bwd      adjoint of k_volume_render      (mpf_generic.hip; utils/mpi/mpi_rendering.py:62-99, :102-139)
//   k_homography_sample_bwd  adjoint of k_homography_sample  (mpf_generic.hip; utils/mpi/homography_sampler.py:124-158)
//   k_warp_composite_bwd     adjoint of mpf_warp_composite_split, the fused standard call of render_tgt_rgb_depth
//
// The composite, per pixel:  d_s = |xyz_{s+1} - xyz_s| (d_{S-1} = 1e3),  t_s = exp(-sigma_s d_s),  A_0 = 1, A_s = prod_{k<s} (t_k + 1e-6),
// w_s = A_s (1 - t_s),  D = sum w_s,  depth = sum w_s z_s / (D + 1e-5).  With the upstream gradients g_rgb[3], g_depth, g_extra[E], g_w[S], g_A[S]:
//   q_s      = g_rgb . c_s + g_extra . e_s + g_depth (z_s - depth) / (D + 1e-5) + g_w[s]          (= dL/dw_s)
//   dL/dc_s  = w_s g_rgb,   dL/de_s = w_s g_extra
//   a_s      = q_s (1 - t_s) + g_A[s]                                                             (= the direct part of dL/dA_s)
//   dL/dt_j  = -A_j q_j + (sum_{s>j} A_s a_s) / (t_j + 1e-6)
//   dL/dsigma_j = -d_j t_j dL/dt_j
// Two passes over the planes: front to back for D and depth (the forward's own sequence: same helpers, same order, same bits), back to front
// for the suffix sum.  No kernel writes anything S-deep but the gradients themselves.  The sampling adjoints scatter with float atomic adds
// (one global_atomic_add_f32 each) into zero-initialised gradient stacks through the forward's own clamped taps: the map is the exact transpose
// of the forward's gather, and the last bits of a sum depend on the order in which its addends arrive.
#include "mpf_common.h"
#include "mpf_math.h"
#include "mpf_render_geom.h"

// ---- plane_volume_rendering / _flow ----------------------------------------------------------------------------------------------------

// grad_sigma doubles as the kernel's only S-deep scratch: the front-to-back pass parks A_s (the forward's float transparency_acc) in the slot
// that the back-to-front pass then overwrites with dL/dsigma_s - each thread touches its own pixel's column only.
template <int NL>
__global__ void __launch_bounds__(256)
k_volume_render_bwd(const float *__restrict__ rgb, const float *__restrict__ sigma, const float *__restrict__ xyz, const float *__restrict__ extra_in,
                    int S, int64_t N, int E, int hard, const float *__restrict__ g_rgb, const float *__restrict__ g_depth,
                    const float *__restrict__ g_extra, const float *__restrict__ g_w, const float *__restrict__ g_tacc,
                    float *__restrict__ grad_rgb, float *__restrict__ grad_sigma, float *__restrict__ grad_extra)
{
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double acc = 1.0;
    MpfCsum<NL> cw, cd;
    cw.init(); cd.init();
    float best_w = 0.0f;
    int best_s = 0;
    for (int s = 0; s < S; ++s) {                                   // the forward's sequence (k_volume_render)
        const float *p = xyz + (int64_t)s * 3 * N + n;
        const float X = p[0], Y = p[N], Z = p[2 * N];
        float dist = 1e3f;
        if (s + 1 < S) {
            const float *q = p + 3 * N;
            dist = mpf_norm3(q[0] - X, q[N] - Y, q[2 * N] - Z);
        }
        const float T = mpf_expf(-sigma[(int64_t)s * N + n] * dist);
        const float tacc = (float)acc;
        const float w = tacc * (1.0f - T);
        acc *= (double)(T + 1e-6f);
        grad_sigma[(int64_t)s * N + n] = tacc;
        if (s == 0 || w > best_w) { best_w = w; best_s = s; }
        cw.push(w);
        cd.push(w * Z);
        if (((s + 1) & 15) == 0) { cw.fold(s + 1); cd.fold(s + 1); }
    }
    float ge[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (g_extra && e < E) ge[e] = g_extra[(int64_t)e * N + n];
    if (hard) {
        // hard_flow (:126-130): the extra is the arg-max plane's value, a one-hot selection that is constant in sigma
        for (int s = 0; s < S; ++s) {
            grad_sigma[(int64_t)s * N + n] = 0.0f;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (grad_extra && e < E) grad_extra[((int64_t)s * E + e) * N + n] = (s == best_s) ? ge[e] : 0.0f;
        }
        return;
    }
    const float Dn = cw.final() + 1e-5f;
    const float depth = cd.final() / Dn;
    float gr[3] = { 0.0f, 0.0f, 0.0f };
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (g_rgb && rgb) gr[c] = g_rgb[(int64_t)c * N + n];
    const float gd = g_depth ? g_depth[n] : 0.0f;
    float Xn = 0.0f, Yn = 0.0f, Zn = 0.0f;
    double R = 0.0;                                                  // sum_{s>j} A_s a_s
    for (int s = S - 1; s >= 0; --s) {
        const float *p = xyz + (int64_t)s * 3 * N + n;
        const float X = p[0], Y = p[N], Z = p[2 * N];
        const float dist = (s + 1 < S) ? mpf_norm3(Xn - X, Yn - Y, Zn - Z) : 1e3f;
        Xn = X; Yn = Y; Zn = Z;
        const float T = mpf_expf(-sigma[(int64_t)s * N + n] * dist);
        const float alpha = 1.0f - T;
        const float tacc = grad_sigma[(int64_t)s * N + n];
        const float w = tacc * alpha;
        float q = gd * ((Z - depth) / Dn);
        if (g_w) q += g_w[(int64_t)s * N + n];
        if (rgb) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                q = fmaf(gr[c], rgb[((int64_t)s * 3 + c) * N + n], q);
                if (grad_rgb) grad_rgb[((int64_t)s * 3 + c) * N + n] = w * gr[c];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < E) {
                q = fmaf(ge[e], extra_in[((int64_t)s * E + e) * N + n], q);
                if (grad_extra) grad_extra[((int64_t)s * E + e) * N + n] = w * ge[e];
            }
        float a = q * alpha;
        if (g_tacc) a += g_tacc[(int64_t)s * N + n];
        const float dLdt = (float)R / (T + 1e-6f) - tacc * q;
        grad_sigma[(int64_t)s * N + n] = -dist * T * dLdt;
        R += (double)tacc * (double)a;
    }
}

extern "C" int mpf_volume_render_bwd(const float *d_rgb, const float *d_sigma, const float *d_xyz, const float *d_extra_in, int S, int64_t N, int E, int hard,
                                     const float *d_g_rgb, const float *d_g_depth, const float *d_g_extra, const float *d_g_weights, const float *d_g_tacc,
                                     float *d_grad_rgb, float *d_grad_sigma, float *d_grad_extra, void *stream)
{
    MPF_REQUIRE(d_sigma && d_xyz && d_grad_sigma, "mpf_volume_render_bwd: null pointer (sigma, xyz and grad_sigma are required)");
    MPF_REQUIRE(S >= 1 && S < 4096 && N >= 1, "mpf_volume_render_bwd: bad shape S=%d N=%lld", S, (long long)N);
    MPF_REQUIRE(E >= 0 && E <= 4 && ((E == 0) == (d_extra_in == nullptr)), "mpf_volume_render_bwd: extra channels: 0..4, with extra_in exactly when E > 0");
    MPF_REQUIRE(E > 0 || (!d_g_extra && !d_grad_extra), "mpf_volume_render_bwd: extra gradients without extra channels");
    MPF_REQUIRE(d_rgb || (!d_g_rgb && !d_grad_rgb), "mpf_volume_render_bwd: rgb gradients without rgb");
    MPF_REQUIRE(!hard || (!d_rgb && E > 0 && !d_g_depth && !d_g_weights && !d_g_tacc),
                "mpf_volume_render_bwd: hard is the flow form: extras only, no rgb, depth, weights or transparency gradients");
    dim3 grid((unsigned)((N + 255) / 256)), block(256);
#define MPF_VRB(NLv) hipLaunchKernelGGL(k_volume_render_bwd<NLv>, grid, block, 0, (hipStream_t)stream, d_rgb, d_sigma, d_xyz, d_extra_in, S, N, E, hard, d_g_rgb, \
                                        d_g_depth, d_g_extra, d_g_weights, d_g_tacc, d_grad_rgb, d_grad_sigma, d_grad_extra)
    if (S < 256) MPF_VRB(2); else MPF_VRB(3);
#undef MPF_VRB
    return mpf_launch_status("k_volume_render_bwd");
}

// ---- HomographySample.sample ---------------------------------------------------------------------------------------------------------

// the four adds of one value through one tap set: exactly the texels the forward read (out-of-image neighbours were read as 0: no add)
MPF_DEV void mpf_scatter4(float *__restrict__ pl, int o00, int W, bool e_in, bool s_in, float nw, float ne, float sw, float se, float g)
{
    atomicAdd(pl + o00, g * nw);
    if (e_in) atomicAdd(pl + o00 + 1, g * ne);
    if (s_in) atomicAdd(pl + o00 + W, g * sw);
    if (e_in && s_in) atomicAdd(pl + o00 + W + 1, g * se);
}

__global__ void __launch_bounds__(256)
k_homography_sample_bwd(const float *__restrict__ g_tgt, const float *__restrict__ params, int S, int C, int H, int W, int c0, int c1,
                        float *__restrict__ g_src)
{
    const int64_t N = (int64_t)H * W;
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y;
    if (n >= N) return;
    const float fx = (float)(n % W), fy = (float)(n / W);
    const float *rec = params + MPF_PARAMS_HEADER + MPF_PLANE_RECORD * s;
    float qx = mpf_row3_xy1(rec[0], rec[1], rec[2], fx, fy);
    float qy = mpf_row3_xy1(rec[3], rec[4], rec[5], fx, fy);
    float qz = mpf_row3_xy1(rec[6], rec[7], rec[8], fx, fy);
    float u = qx / qz, v = qy / qz;
    MpfTaps t = mpf_make_taps(u, v, W, H);          // x0 in [0, W-1], y0 in [0, H-1] (clamped), e_in / s_in guard the +1 neighbours
    const int o00 = t.y0 * W + t.x0;
    for (int c = c0; c < c1; ++c) {
        const float g = g_tgt[((int64_t)s * C + c) * N + n];
        mpf_scatter4(g_src + ((int64_t)s * C + c) * N, o00, W, t.e_in, t.s_in, t.nw, t.ne, t.sw, t.se, g);
    }
}

extern "C" int mpf_homography_sample_bwd(const float *d_g_tgt, const float *d_params, int S, int C, int H, int W, int c0, int c1, float *d_g_src, void *stream)
{
    MPF_REQUIRE(d_g_tgt && d_params && d_g_src, "mpf_homography_sample_bwd: null pointer");
    MPF_REQUIRE(S >= 1 && S < 65536 && C >= 1 && H >= 1 && W >= 1, "mpf_homography_sample_bwd: bad shape S=%d C=%d H=%d W=%d", S, C, H, W);
    MPF_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "mpf_homography_sample_bwd: H*W too large");
    MPF_REQUIRE(c0 >= 0 && c0 < c1 && c1 <= C, "mpf_homography_sample_bwd: channel range [%d, %d) outside [0, %d)", c0, c1, C);
    const int64_t N = (int64_t)H * W;
    hipLaunchKernelGGL(k_homography_sample_bwd, dim3((unsigned)((N + 255) / 256), S), dim3(256), 0, (hipStream_t)stream, d_g_tgt, d_params, S, C, H, W,
                       c0, c1, d_g_src);
    return mpf_launch_status("k_homography_sample_bwd");
}

// ---- the fused standard call (mpf_warp_composite_split) ------------------------------------------------------------------------------

struct MpfBwdGeom {
    float nw, ne, sw, se;
    float X, Y, Z;
    int o00;
    bool e_in, s_in;
};

template <bool KS>
MPF_DEV void mpf_bwd_geom(const MpfConstParams params, int s, const MpfConsts &c, MpfBwdGeom &g)
{
    int x0, y0;
    float qz;
    mpf_geom_core<KS, false>(params, s, c, g.nw, g.ne, g.sw, g.se, g.X, g.Y, g.Z, x0, y0, qz);
    g.o00 = y0 * c.W + x0;                      // x0 in [0, W-1], y0 in [0, H-1]: the coordinate is clamped before it is truncated
    g.e_in = (x0 + 1) < c.W;
    g.s_in = (y0 + 1) < c.H;
}

// one channel plane through one tap set.  The forward reads the east / south neighbour even where it lies outside the image (some finite texel, or 0
// past the tensor's end) with a weight that is exactly 0 there; re-reading the north-west texel instead adds the same exact 0.
MPF_DEV float mpf_bwd_sample(const float *__restrict__ pl, const MpfBwdGeom &g, int W)
{
    const float a = pl[g.o00];
    const float b = g.e_in ? pl[g.o00 + 1] : a;
    const float c = g.s_in ? pl[g.o00 + W] : a;
    const float d = (g.e_in && g.s_in) ? pl[g.o00 + W + 1] : a;
    return mpf_tap4w(g, a, b, c, d);
}

MPF_DEV float mpf_bwd_transparency(const float *__restrict__ sigma_plane, const MpfBwdGeom &g, int W, float dist)
{
    float sg = mpf_bwd_sample(sigma_plane, g, W);
    sg = (g.Z >= 0.0f) ? sg : 0.0f;             // mpi_rendering.py:336-338
    return mpf_expf_fast(-sg * dist);
}

// One thread per target pixel.  Pass 1 (front to back) is the forward's own recurrence and yields D, depth and the last plane whose float
// transparency_acc is non-zero together with the double running product there.  Pass 2 (back to front) rebuilds A_s from that product by division -
// A_s = A_{s+1} / (t_s + 1e-6), in double, started where the product is still far above the double range's floor - and scatters each plane's
// dL/drgb and dL/dsigma through the plane's taps.  Planes behind that last plane have w = 0 and A = 0 in the forward: they receive nothing.
template <bool KS, bool HAS_MASK, int NL>
MPF_DEV void mpf_wcb_body(const float *__restrict__ rgb, const float *__restrict__ sigma, const float *__restrict__ quads, const MpfConstParams params,
                          int S, int H, int W, const float *__restrict__ g_rgb, const float *__restrict__ g_depth, const float *__restrict__ g_om,
                          float *__restrict__ grad_rgb, float *__restrict__ grad_sigma, int x, int y)
{
    const int64_t N = (int64_t)H * W;
    MpfConsts c;
    c.fx = (float)x; c.fy = (float)y;
    c.W = W; c.H = H; c.Wf = (float)W; c.Hf = (float)H;
    c.halfW = (float)W * 0.5f; c.halfH = (float)H * 0.5f;
    c.rhalfW = 1.0f / c.halfW; c.rhalfH = 1.0f / c.halfH;
    c.maxx = (float)(W - 1); c.maxy = (float)(H - 1);
    c.row_bytes = (unsigned)W * 16u;
    mpf_consts_pose(c, params);

    MpfBwdGeom cur, nxt;
    mpf_bwd_geom<KS>(params, 0, c, cur);
    double acc = 1.0, acc_last = 1.0;
    int s_last = 0;
    MpfCsum<NL> cw, cd;
    cw.init(); cd.init();
    for (int s = 0; s < S; ++s) {
        float dist = 1e3f;
        nxt = cur;
        if (s + 1 < S) {
            mpf_bwd_geom<KS>(params, s + 1, c, nxt);
            dist = mpf_norm3_nr(nxt.X - cur.X, nxt.Y - cur.Y, nxt.Z - cur.Z);
        }
        const float T = mpf_bwd_transparency(sigma + (int64_t)s * N, cur, W, dist);
        const float tacc = (float)acc;
        if (tacc != 0.0f) { s_last = s; acc_last = acc; }
        const float w = tacc * (1.0f - T);
        acc *= (double)(T + 1e-6f);
        cw.push(w);
        cd.push(w * cur.Z);
        if (((s + 1) & 15) == 0) { cw.fold(s + 1); cd.fold(s + 1); }
        cur = nxt;
    }
    const float Dn = cw.final() + 1e-5f;
    const float depth = cd.final() / Dn;
    const int64_t n = (int64_t)y * W + x;
    const float gr = g_rgb[n], gg = g_rgb[N + n], gb = g_rgb[2 * N + n];
    const float gd = g_depth ? g_depth[n] : 0.0f;
    const float gm = (HAS_MASK && g_om) ? g_om[n] : 0.0f;

    double A = acc_last, R = 0.0;
    for (int s = S - 1; s >= 0; --s) {
        mpf_bwd_geom<KS>(params, s, c, cur);
        const float dist = (s + 1 < S) ? mpf_norm3_nr(nxt.X - cur.X, nxt.Y - cur.Y, nxt.Z - cur.Z) : 1e3f;
        nxt = cur;
        if (s > s_last) continue;
        const float T = mpf_bwd_transparency(sigma + (int64_t)s * N, cur, W, dist);
        if (s < s_last) A = A / (double)(T + 1e-6f);
        const float alpha = 1.0f - T;
        const float tacc = (float)A;
        const float w = tacc * alpha;
        const float *prgb = rgb + (int64_t)s * 3 * N;
        float q = gd * ((cur.Z - depth) / Dn);
        q = fmaf(gr, mpf_bwd_sample(prgb, cur, W), q);
        q = fmaf(gg, mpf_bwd_sample(prgb + N, cur, W), q);
        q = fmaf(gb, mpf_bwd_sample(prgb + 2 * N, cur, W), q);
        if (HAS_MASK) {
            const float4 mq = reinterpret_cast<const float4 *>(quads)[cur.o00];     // quads carry the zeros of out-of-image neighbours
            q = fmaf(gm, mpf_tap4w(cur, mq.x, mq.y, mq.z, mq.w), q);
        }
        const float dLdt = (float)R / (T + 1e-6f) - tacc * q;
        const float gs = (cur.Z >= 0.0f) ? -dist * T * dLdt : 0.0f;
        R += (double)tacc * (double)(q * alpha);
        float *drgb = grad_rgb + (int64_t)s * 3 * N;
        if (w != 0.0f) {
            mpf_scatter4(drgb, cur.o00, W, cur.e_in, cur.s_in, cur.nw, cur.ne, cur.sw, cur.se, w * gr);
            mpf_scatter4(drgb + N, cur.o00, W, cur.e_in, cur.s_in, cur.nw, cur.ne, cur.sw, cur.se, w * gg);
            mpf_scatter4(drgb + 2 * N, cur.o00, W, cur.e_in, cur.s_in, cur.nw, cur.ne, cur.sw, cur.se, w * gb);
        }
        if (gs != 0.0f) mpf_scatter4(grad_sigma + (int64_t)s * N, cur.o00, W, cur.e_in, cur.s_in, cur.nw, cur.ne, cur.sw, cur.se, gs);
    }
}

template <bool HAS_MASK, int NL>
__global__ void __launch_bounds__(256)
k_warp_composite_bwd(const float *__restrict__ rgb, const float *__restrict__ sigma, const float *__restrict__ quads, const float *__restrict__ params,
                     int S, int H, int W, const float *__restrict__ g_rgb, const float *__restrict__ g_depth, const float *__restrict__ g_om,
                     float *__restrict__ grad_rgb, float *__restrict__ grad_sigma)
{
    constexpr int TW = 32, TH = 8;                                   // the forward's tile (k_warp_composite_planar)
    const unsigned tiles_x = (W + TW - 1) / TW;
    const unsigned tile = mpf_xcd_remap(blockIdx.x, gridDim.x);
    const int x = (tile % tiles_x) * TW + (threadIdx.x % TW);
    const int y = (tile / tiles_x) * TH + (threadIdx.x / TW);
    if (x >= W || y >= H) return;                                    // no barrier below: threads past the edge simply leave
    const MpfConstParams cp = (MpfConstParams)params;
    const bool pinhole = (cp[1] == 0.0f) & (cp[3] == 0.0f) & (cp[6] == 0.0f) & (cp[7] == 0.0f) & (cp[8] == 1.0f);   // the forward's own test
    if (pinhole)
        mpf_wcb_body<true, HAS_MASK, NL>(rgb, sigma, quads, cp, S, H, W, g_rgb, g_depth, g_om, grad_rgb, grad_sigma, x, y);
    else
        mpf_wcb_body<false, HAS_MASK, NL>(rgb, sigma, quads, cp, S, H, W, g_rgb, g_depth, g_om, grad_rgb, grad_sigma, x, y);
}

extern "C" int mpf_warp_composite_bwd(const float *d_rgb_S3HW, const float *d_sigma_SHW, const float *d_mask_quads, const float *d_params, int S, int H, int W,
                                      const float *d_g_rgb, const float *d_g_depth, const float *d_g_objmask, float *d_grad_rgb_S3HW,
                                      float *d_grad_sigma_SHW, void *stream)
{
    MPF_REQUIRE(d_rgb_S3HW && d_sigma_SHW && d_params && d_g_rgb && d_grad_rgb_S3HW && d_grad_sigma_SHW, "mpf_warp_composite_bwd: null pointer");
    MPF_REQUIRE(S >= 1 && S < 4096 && H >= 1 && W >= 1, "mpf_warp_composite_bwd: bad shape S=%d H=%d W=%d", S, H, W);
    MPF_REQUIRE((int64_t)H * W < ((int64_t)1 << 27), "mpf_warp_composite_bwd: H*W too large for 32-bit offsets");
    MPF_REQUIRE(d_mask_quads || !d_g_objmask, "mpf_warp_composite_bwd: an objmask gradient needs the mask quads");
    MPF_REQUIRE(!d_mask_quads || mpf_aligned16(d_mask_quads), "mpf_warp_composite_bwd: mask quads must be 16-byte aligned");
    const unsigned tiles = ((W + 31) / 32) * ((H + 7) / 8);
#define MPF_WCB(HM, NLv) hipLaunchKernelGGL((k_warp_composite_bwd<HM, NLv>), dim3(tiles), dim3(256), 0, (hipStream_t)stream, d_rgb_S3HW, d_sigma_SHW, d_mask_quads, \
                                            d_params, S, H, W, d_g_rgb, d_g_depth, d_g_objmask, d_grad_rgb_S3HW, d_grad_sigma_SHW)
    if (S < 256) { if (d_mask_quads) MPF_WCB(true, 2); else MPF_WCB(false, 2); }
    else         { if (d_mask_quads) MPF_WCB(true, 3); else MPF_WCB(false, 3); }
#undef MPF_WCB
    return mpf_launch_status("k_warp_composite_bwd");
}
