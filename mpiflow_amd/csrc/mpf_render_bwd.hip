// mpf_render_bwd.hip - adjoints of the utils/mpi renderer with respect to the per-plane VALUES (colour, density, extras) and, on request, with
// respect to the plane GEOMETRY that a disparity reaches: the xyz tensors of the composite, the plane disparities and the plane depth of the
// source-to-target flow.  Poses and intrinsics are constant, and so is the sampling grid (the reference inverts its homography under no_grad).
//
//   k_volume_render_bwd      adjoint of k_volume_render      (mpf_generic.hip; utils/mpi/mpi_rendering.py:62-99, :102-139)
//   k_homography_sample_bwd  adjoint of k_homography_sample  (mpf_generic.hip; utils/mpi/homography_sampler.py:124-158)
//   k_warp_composite_bwd     adjoint of mpf_warp_composite_split, the fused standard call of render_tgt_rgb_depth (DISP: + the disparity gradient)
//   k_src_xyz_bwd            adjoint of k_src_xyz            (mpf_generic.hip; utils/mpi/mpi_rendering.py:213-239) with respect to the disparities
//   k_plane_flow_bwd         adjoint of k_homography_flow    (mpf_generic.hip; utils/mpi/homography_sampler.py:160-220) with respect to the plane depth
//
// The composite, per pixel:  d_s = |xyz_{s+1} - xyz_s| (d_{S-1} = 1e3),  t_s = exp(-sigma_s d_s),  A_0 = 1, A_s = prod_{k<s} (t_k + 1e-6),
// w_s = A_s (1 - t_s),  D = sum w_s,  depth = sum w_s z_s / (D + 1e-5).  With the upstream gradients g_rgb[3], g_depth, g_extra[E], g_w[S], g_A[S]:
//   q_s      = g_rgb . c_s + g_extra . e_s + g_depth (z_s - depth) / (D + 1e-5) + g_w[s]          (= dL/dw_s)
//   dL/dc_s  = w_s g_rgb,   dL/de_s = w_s g_extra
//   a_s      = q_s (1 - t_s) + g_A[s]                                                             (= the direct part of dL/dA_s)
//   dL/dt_j  = -A_j q_j + (sum_{s>j} A_s a_s) / (t_j + 1e-6)
//   dL/dsigma_j = -d_j t_j dL/dt_j
//   dL/dd_j  = -sigma_j t_j dL/dt_j  (j < S-1; d_{S-1} is the constant 1e3),   u_j = (xyz_{j+1} - xyz_j) / d_j  (0 where d_j = 0, as torch's norm)
//   dL/dxyz_s = u_{s-1} dL/dd_{s-1} - u_s dL/dd_s + (0, 0, 1) g_depth w_s / (D + 1e-5)
// Two passes over the planes: front to back for D and depth (the forward's own sequence: same helpers, same order, same bits), back to front
// for the suffix sum.  No kernel writes anything S-deep but the gradients themselves.  The sampling adjoints scatter with float atomic adds
// (one global_atomic_add_f32 each) into zero-initialised gradient stacks through the forward's own clamped taps: the map is the exact transpose
// of the forward's gather, and the last bits of a sum depend on the order in which its addends arrive.  The geometry gradients use no atomics: the
// xyz gradient is one store per element, the per-plane sums over all pixels go wave -> LDS slot -> per-block partial -> a second kernel that adds the
// partials in block order in double (mpf_plane_sum_*): two runs give the same bits.
#include "mpf_common.h"
#include "mpf_math.h"
#include "mpf_reduce.h"
#include "mpf_render_geom.h"

// ---- plane_volume_rendering / _flow ----------------------------------------------------------------------------------------------------

// grad_sigma doubles as the kernel's only S-deep scratch: the front-to-back pass parks A_s (the forward's float transparency_acc) in the slot
// that the back-to-front pass then overwrites with dL/dsigma_s - each thread touches its own pixel's column only.
// WX: also write dL/dxyz [S,3,N] - going back to front, plane s+1's gradient is complete once plane s's distance term is known (one store per element).
template <int NL, bool WX>
__global__ void __launch_bounds__(256)
k_volume_render_bwd(const float *__restrict__ rgb, const float *__restrict__ sigma, const float *__restrict__ xyz, const float *__restrict__ extra_in,
                    int S, int64_t N, int E, int hard, const float *__restrict__ g_rgb, const float *__restrict__ g_depth,
                    const float *__restrict__ g_extra, const float *__restrict__ g_w, const float *__restrict__ g_tacc,
                    float *__restrict__ grad_rgb, float *__restrict__ grad_sigma, float *__restrict__ grad_extra, float *__restrict__ grad_xyz)
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
            if (WX) {
                float *gx = grad_xyz + (int64_t)s * 3 * N + n;
                gx[0] = 0.0f; gx[N] = 0.0f; gx[2 * N] = 0.0f;
            }
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
    float Px = 0.0f, Py = 0.0f, Pz = 0.0f;                           // WX: what plane s+1's own terms give dL/dxyz_{s+1}
    for (int s = S - 1; s >= 0; --s) {
        const float *p = xyz + (int64_t)s * 3 * N + n;
        const float X = p[0], Y = p[N], Z = p[2 * N];
        const float dx = Xn - X, dy = Yn - Y, dz = Zn - Z;
        const float dist = (s + 1 < S) ? mpf_norm3(dx, dy, dz) : 1e3f;
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
        if (WX) {
            float ux = 0.0f, uy = 0.0f, uz = 0.0f;                   // u_s dL/dd_s
            if (s + 1 < S) {
                if (dist > 0.0f) {
                    const float r = (-sigma[(int64_t)s * N + n] * T * dLdt) / dist;
                    ux = dx * r; uy = dy * r; uz = dz * r;
                }
                float *gx = grad_xyz + (int64_t)(s + 1) * 3 * N + n;
                gx[0] = Px + ux; gx[N] = Py + uy; gx[2 * N] = Pz + uz;
            }
            Px = -ux; Py = -uy; Pz = gd * (w / Dn) - uz;
        }
    }
    if (WX) {
        float *gx = grad_xyz + n;
        gx[0] = Px; gx[N] = Py; gx[2 * N] = Pz;
    }
}

extern "C" int mpf_volume_render_bwd_xyz(const float *d_rgb, const float *d_sigma, const float *d_xyz, const float *d_extra_in, int S, int64_t N, int E, int hard,
                                         const float *d_g_rgb, const float *d_g_depth, const float *d_g_extra, const float *d_g_weights, const float *d_g_tacc,
                                         float *d_grad_rgb, float *d_grad_sigma, float *d_grad_extra, float *d_grad_xyz, void *stream)
{
    MPF_REQUIRE(d_sigma && d_xyz && d_grad_sigma, "mpf_volume_render_bwd: null pointer (sigma, xyz and grad_sigma are required)");
    MPF_REQUIRE(S >= 1 && S < 4096 && N >= 1, "mpf_volume_render_bwd: bad shape S=%d N=%lld", S, (long long)N);
    MPF_REQUIRE(E >= 0 && E <= 4 && ((E == 0) == (d_extra_in == nullptr)), "mpf_volume_render_bwd: extra channels: 0..4, with extra_in exactly when E > 0");
    MPF_REQUIRE(E > 0 || (!d_g_extra && !d_grad_extra), "mpf_volume_render_bwd: extra gradients without extra channels");
    MPF_REQUIRE(d_rgb || (!d_g_rgb && !d_grad_rgb), "mpf_volume_render_bwd: rgb gradients without rgb");
    MPF_REQUIRE(!hard || (!d_rgb && E > 0 && !d_g_depth && !d_g_weights && !d_g_tacc),
                "mpf_volume_render_bwd: hard is the flow form: extras only, no rgb, depth, weights or transparency gradients");
    dim3 grid((unsigned)((N + 255) / 256)), block(256);
#define MPF_VRB(NLv, WXv) hipLaunchKernelGGL((k_volume_render_bwd<NLv, WXv>), grid, block, 0, (hipStream_t)stream, d_rgb, d_sigma, d_xyz, d_extra_in, S, N, E, hard, \
                                             d_g_rgb, d_g_depth, d_g_extra, d_g_weights, d_g_tacc, d_grad_rgb, d_grad_sigma, d_grad_extra, d_grad_xyz)
    if (d_grad_xyz) { if (S < 256) MPF_VRB(2, true); else MPF_VRB(3, true); }
    else            { if (S < 256) MPF_VRB(2, false); else MPF_VRB(3, false); }
#undef MPF_VRB
    return mpf_launch_status("k_volume_render_bwd");
}

extern "C" int mpf_volume_render_bwd(const float *d_rgb, const float *d_sigma, const float *d_xyz, const float *d_extra_in, int S, int64_t N, int E, int hard,
                                     const float *d_g_rgb, const float *d_g_depth, const float *d_g_extra, const float *d_g_weights, const float *d_g_tacc,
                                     float *d_grad_rgb, float *d_grad_sigma, float *d_grad_extra, void *stream)
{
    return mpf_volume_render_bwd_xyz(d_rgb, d_sigma, d_xyz, d_extra_in, S, N, E, hard, d_g_rgb, d_g_depth, d_g_extra, d_g_weights, d_g_tacc, d_grad_rgb,
                                     d_grad_sigma, d_grad_extra, nullptr, stream);
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

MPF_DEV float mpf_bwd_sigma(const float *__restrict__ sigma_plane, const MpfBwdGeom &g, int W)
{
    const float sg = mpf_bwd_sample(sigma_plane, g, W);
    return (g.Z >= 0.0f) ? sg : 0.0f;           // mpi_rendering.py:336-338
}

MPF_DEV float mpf_bwd_transparency(const float *__restrict__ sigma_plane, const MpfBwdGeom &g, int W, float dist)
{
    return mpf_expf_fast(-mpf_bwd_sigma(sigma_plane, g, W) * dist);
}

// ---- per-plane sums over all pixels, without atomics ----------------------------------------------------------------------------------
// At plane s every wave adds its 64 lanes (mpf_wave_sum: every lane must be there, so callers keep threads past the image alive with v = 0) and
// lane 0 parks the sum in the LDS slot [wave][s]; after the plane loop the workgroup adds its wave slots in wave order into partial[block][s];
// k_plane_sum_final adds the partials in block order, in double.  Every order is fixed: two runs give the same bits.
MPF_DEV void mpf_plane_sum_push(float v, int s, int S, float *__restrict__ lds)
{
    v = mpf_wave_sum(v);
    if ((threadIdx.x & 63u) == 0) lds[(threadIdx.x >> 6) * S + s] = v;
}

MPF_DEV void mpf_plane_sum_flush(const float *__restrict__ lds, int S, float *__restrict__ partial_row)
{
    __syncthreads();
    const int waves = (int)(blockDim.x >> 6);
    for (int s = (int)threadIdx.x; s < S; s += (int)blockDim.x) {
        float a = lds[s];
        for (int w = 1; w < waves; ++w) a += lds[w * S + s];
        partial_row[s] = a;
    }
}

__global__ void __launch_bounds__(256)
k_plane_sum_final(const float *__restrict__ partial, int blocks, int S, float *__restrict__ out)
{
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= S) return;
    double a = 0.0;
    for (int b = 0; b < blocks; ++b) a += (double)partial[(int64_t)b * S + s];
    out[s] = (float)a;
}

static int mpf_plane_sum_finish(const float *d_partial, int blocks, int S, float *d_out, void *stream, const char *what)
{
    hipLaunchKernelGGL(k_plane_sum_final, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_partial, blocks, S, d_out);
    return mpf_launch_status(what);
}

// One thread per target pixel.  Pass 1 (front to back) is the forward's own recurrence and yields D, depth and the last plane whose float
// transparency_acc is non-zero together with the double running product there.  Pass 2 (back to front) rebuilds A_s from that product by division -
// A_s = A_{s+1} / (t_s + 1e-6), in double, started where the product is still far above the double range's floor - and scatters each plane's
// dL/drgb and dL/dsigma through the plane's taps.  Planes behind that last plane have w = 0 and A = 0 in the forward: they receive nothing.
//
// DISP: also the gradient of the plane disparities.  The scan yields dL/dxyz_tgt_s(q) exactly as k_volume_render_bwd<WX> does (the density being the
// sampled one, zero where z < 0; the sampling coordinate is a constant), and the analytic field xyz_tgt_s(q) = depth_s R K^-1 (ix, iy, 1) + t gives
// d xyz_tgt_s(q) / d disparity_s = -depth_s (xyz_tgt_s(q) - t): the dot product is summed over the pixels per plane (mpf_plane_sum_*), no [S,3,H,W]
// gradient is written.  `live` is false for the threads past the image's edge, which a DISP launch keeps (clamped to the last pixel) for the wave sums.
template <bool KS, bool HAS_MASK, int NL, bool DISP>
MPF_DEV void mpf_wcb_body(const float *__restrict__ rgb, const float *__restrict__ sigma, const float *__restrict__ quads, const MpfConstParams params,
                          int S, int H, int W, const float *__restrict__ g_rgb, const float *__restrict__ g_depth, const float *__restrict__ g_om,
                          float *__restrict__ grad_rgb, float *__restrict__ grad_sigma, int x, int y, bool live, float *__restrict__ lds)
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
    const float tx = params[12], ty = params[16], tz = params[20];   // DISP: the translation of G_tgt_src
    float Px = 0.0f, Py = 0.0f, Pz = 0.0f;                           // DISP: what plane s+1's own terms give dL/dxyz_{s+1}

    double A = acc_last, R = 0.0;
    for (int s = S - 1; s >= 0; --s) {
        mpf_bwd_geom<KS>(params, s, c, cur);
        const float dx = nxt.X - cur.X, dy = nxt.Y - cur.Y, dz = nxt.Z - cur.Z;
        const float dist = (s + 1 < S) ? mpf_norm3_nr(dx, dy, dz) : 1e3f;
        const float nX = nxt.X, nY = nxt.Y, nZ = nxt.Z;             // DISP: plane s+1's xyz_tgt
        nxt = cur;
        float ux = 0.0f, uy = 0.0f, uz = 0.0f, wz = 0.0f;            // DISP: u_s dL/dd_s and the depth term of plane s
        if (s <= s_last) {
            const float sg = mpf_bwd_sigma(sigma + (int64_t)s * N, cur, W);
            const float T = mpf_expf_fast(-sg * dist);
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
            if (w != 0.0f && live) {
                mpf_scatter4(drgb, cur.o00, W, cur.e_in, cur.s_in, cur.nw, cur.ne, cur.sw, cur.se, w * gr);
                mpf_scatter4(drgb + N, cur.o00, W, cur.e_in, cur.s_in, cur.nw, cur.ne, cur.sw, cur.se, w * gg);
                mpf_scatter4(drgb + 2 * N, cur.o00, W, cur.e_in, cur.s_in, cur.nw, cur.ne, cur.sw, cur.se, w * gb);
            }
            if (gs != 0.0f && live) mpf_scatter4(grad_sigma + (int64_t)s * N, cur.o00, W, cur.e_in, cur.s_in, cur.nw, cur.ne, cur.sw, cur.se, gs);
            if (DISP) {
                if (s + 1 < S && dist > 0.0f) {
                    const float r = (-sg * T * dLdt) / dist;
                    ux = dx * r; uy = dy * r; uz = dz * r;
                }
                wz = gd * (w / Dn);
            }
        }
        if (DISP) {
            if (s + 1 < S) {                                         // plane s+1 is complete; S is uniform, every lane of every wave arrives here
                const float d1 = params[MPF_PARAMS_HEADER + MPF_PLANE_RECORD * (s + 1) + 9];
                float v = (Px + ux) * (nX - tx);
                v = fmaf(Py + uy, nY - ty, v);
                v = fmaf(Pz + uz, nZ - tz, v);
                mpf_plane_sum_push(live ? -d1 * v : 0.0f, s + 1, S, lds);
            }
            Px = -ux; Py = -uy; Pz = wz - uz;
        }
    }
    if (DISP) {
        const float d0 = params[MPF_PARAMS_HEADER + 9];
        float v = Px * (cur.X - tx);
        v = fmaf(Py, cur.Y - ty, v);
        v = fmaf(Pz, cur.Z - tz, v);
        mpf_plane_sum_push(live ? -d0 * v : 0.0f, 0, S, lds);
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
        mpf_wcb_body<true, HAS_MASK, NL, false>(rgb, sigma, quads, cp, S, H, W, g_rgb, g_depth, g_om, grad_rgb, grad_sigma, x, y, true, nullptr);
    else
        mpf_wcb_body<false, HAS_MASK, NL, false>(rgb, sigma, quads, cp, S, H, W, g_rgb, g_depth, g_om, grad_rgb, grad_sigma, x, y, true, nullptr);
}

// the same with the disparity gradient: every thread of the block stays (the wave sums need all 64 lanes, the flush a barrier); one past the image's
// edge works on the nearest pixel inside and contributes nothing.  Dynamic LDS: [4 waves][S] floats.
template <bool HAS_MASK, int NL>
__global__ void __launch_bounds__(256)
k_warp_composite_bwd_disp(const float *__restrict__ rgb, const float *__restrict__ sigma, const float *__restrict__ quads, const float *__restrict__ params,
                          int S, int H, int W, const float *__restrict__ g_rgb, const float *__restrict__ g_depth, const float *__restrict__ g_om,
                          float *__restrict__ grad_rgb, float *__restrict__ grad_sigma, float *__restrict__ partial)
{
    extern __shared__ float mpf_wcb_lds[];
    constexpr int TW = 32, TH = 8;
    const unsigned tiles_x = (W + TW - 1) / TW;
    const unsigned tile = mpf_xcd_remap(blockIdx.x, gridDim.x);
    int x = (tile % tiles_x) * TW + (threadIdx.x % TW);
    int y = (tile / tiles_x) * TH + (threadIdx.x / TW);
    const bool live = (x < W) & (y < H);
    x = min(x, W - 1); y = min(y, H - 1);
    const MpfConstParams cp = (MpfConstParams)params;
    const bool pinhole = (cp[1] == 0.0f) & (cp[3] == 0.0f) & (cp[6] == 0.0f) & (cp[7] == 0.0f) & (cp[8] == 1.0f);
    if (pinhole)
        mpf_wcb_body<true, HAS_MASK, NL, true>(rgb, sigma, quads, cp, S, H, W, g_rgb, g_depth, g_om, grad_rgb, grad_sigma, x, y, live, mpf_wcb_lds);
    else
        mpf_wcb_body<false, HAS_MASK, NL, true>(rgb, sigma, quads, cp, S, H, W, g_rgb, g_depth, g_om, grad_rgb, grad_sigma, x, y, live, mpf_wcb_lds);
    mpf_plane_sum_flush(mpf_wcb_lds, S, partial + (int64_t)blockIdx.x * S);
}

extern "C" int mpf_warp_composite_bwd_disp(const float *d_rgb_S3HW, const float *d_sigma_SHW, const float *d_mask_quads, const float *d_params, int S, int H, int W,
                                           const float *d_g_rgb, const float *d_g_depth, const float *d_g_objmask, float *d_grad_rgb_S3HW,
                                           float *d_grad_sigma_SHW, float *d_partial, int partial_blocks, float *d_grad_disparity, void *stream)
{
    MPF_REQUIRE(d_rgb_S3HW && d_sigma_SHW && d_params && d_g_rgb && d_grad_rgb_S3HW && d_grad_sigma_SHW, "mpf_warp_composite_bwd: null pointer");
    MPF_REQUIRE(S >= 1 && S < 4096 && H >= 1 && W >= 1, "mpf_warp_composite_bwd: bad shape S=%d H=%d W=%d", S, H, W);
    MPF_REQUIRE((int64_t)H * W < ((int64_t)1 << 27), "mpf_warp_composite_bwd: H*W too large for 32-bit offsets");
    MPF_REQUIRE(d_mask_quads || !d_g_objmask, "mpf_warp_composite_bwd: an objmask gradient needs the mask quads");
    MPF_REQUIRE(!d_mask_quads || mpf_aligned16(d_mask_quads), "mpf_warp_composite_bwd: mask quads must be 16-byte aligned");
    const unsigned tiles = ((W + 31) / 32) * ((H + 7) / 8);
    MPF_REQUIRE((d_grad_disparity != nullptr) == (d_partial != nullptr), "mpf_warp_composite_bwd_disp: the disparity gradient and its workspace come together");
    MPF_REQUIRE(!d_partial || partial_blocks >= (int)tiles, "mpf_warp_composite_bwd_disp: workspace of %d rows, %u tiles", partial_blocks, tiles);
    if (d_grad_disparity) {
        const size_t lds = (size_t)4 * S * sizeof(float);            // S < 4096: below the 64 KiB a workgroup may ask for
#define MPF_WCBD(HM, NLv) hipLaunchKernelGGL((k_warp_composite_bwd_disp<HM, NLv>), dim3(tiles), dim3(256), lds, (hipStream_t)stream, d_rgb_S3HW, d_sigma_SHW, \
                                             d_mask_quads, d_params, S, H, W, d_g_rgb, d_g_depth, d_g_objmask, d_grad_rgb_S3HW, d_grad_sigma_SHW, d_partial)
        if (S < 256) { if (d_mask_quads) MPF_WCBD(true, 2); else MPF_WCBD(false, 2); }
        else         { if (d_mask_quads) MPF_WCBD(true, 3); else MPF_WCBD(false, 3); }
#undef MPF_WCBD
        const int rc = mpf_launch_status("k_warp_composite_bwd_disp");
        return rc ? rc : mpf_plane_sum_finish(d_partial, (int)tiles, S, d_grad_disparity, stream, "k_plane_sum_final");
    }
#define MPF_WCB(HM, NLv) hipLaunchKernelGGL((k_warp_composite_bwd<HM, NLv>), dim3(tiles), dim3(256), 0, (hipStream_t)stream, d_rgb_S3HW, d_sigma_SHW, d_mask_quads, \
                                            d_params, S, H, W, d_g_rgb, d_g_depth, d_g_objmask, d_grad_rgb_S3HW, d_grad_sigma_SHW)
    if (S < 256) { if (d_mask_quads) MPF_WCB(true, 2); else MPF_WCB(false, 2); }
    else         { if (d_mask_quads) MPF_WCB(true, 3); else MPF_WCB(false, 3); }
#undef MPF_WCB
    return mpf_launch_status("k_warp_composite_bwd");
}

extern "C" int mpf_warp_composite_bwd(const float *d_rgb_S3HW, const float *d_sigma_SHW, const float *d_mask_quads, const float *d_params, int S, int H, int W,
                                      const float *d_g_rgb, const float *d_g_depth, const float *d_g_objmask, float *d_grad_rgb_S3HW,
                                      float *d_grad_sigma_SHW, void *stream)
{
    return mpf_warp_composite_bwd_disp(d_rgb_S3HW, d_sigma_SHW, d_mask_quads, d_params, S, H, W, d_g_rgb, d_g_depth, d_g_objmask, d_grad_rgb_S3HW,
                                       d_grad_sigma_SHW, nullptr, 0, nullptr, stream);
}

// ---- get_src_xyz_from_plane_disparity: xyz_s(p) = K^-1 (x, y, 1) / disparity_s  =>  dL/d disparity_s = -depth_s^2 sum_p <g_s(p), K^-1 (x, y, 1)> ------------

__global__ void __launch_bounds__(256)
k_src_xyz_bwd(const float *__restrict__ g_xyz, const float *__restrict__ params_, int S, int H, int W, float *__restrict__ partial)
{
    extern __shared__ float mpf_sxb_lds[];
    const MpfConstParams params = (MpfConstParams)params_;
    const int64_t N = (int64_t)H * W;
    const int64_t n0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = n0 < N;
    const int64_t n = live ? n0 : N - 1;
    const float fx = (float)(n % W), fy = (float)(n / W);
    const float rx = mpf_row3_xy1(params[0], params[1], params[2], fx, fy);          // the forward's ray (k_src_xyz)
    const float ry = mpf_row3_xy1(params[3], params[4], params[5], fx, fy);
    const float rz = mpf_row3_xy1(params[6], params[7], params[8], fx, fy);
    for (int s = 0; s < S; ++s) {
        const float d = params[MPF_PARAMS_HEADER + MPF_PLANE_RECORD * s + 9];
        const float *g = g_xyz + (int64_t)s * 3 * N + n;
        float v = g[0] * rx;
        v = fmaf(g[N], ry, v);
        v = fmaf(g[2 * N], rz, v);
        mpf_plane_sum_push(live ? -(d * d) * v : 0.0f, s, S, mpf_sxb_lds);
    }
    mpf_plane_sum_flush(mpf_sxb_lds, S, partial + (int64_t)blockIdx.x * S);
}

extern "C" int mpf_src_xyz_bwd(const float *d_g_xyz_S3HW, const float *d_params, int S, int H, int W, float *d_partial, int partial_blocks,
                               float *d_grad_disparity, void *stream)
{
    MPF_REQUIRE(d_g_xyz_S3HW && d_params && d_partial && d_grad_disparity, "mpf_src_xyz_bwd: null pointer");
    MPF_REQUIRE(S >= 1 && S < 4096 && H >= 1 && W >= 1, "mpf_src_xyz_bwd: bad shape S=%d H=%d W=%d", S, H, W);
    MPF_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "mpf_src_xyz_bwd: H*W too large");
    const int64_t N = (int64_t)H * W;
    const int blocks = (int)((N + 255) / 256);
    MPF_REQUIRE(partial_blocks >= blocks, "mpf_src_xyz_bwd: workspace of %d rows, %d blocks", partial_blocks, blocks);
    hipLaunchKernelGGL(k_src_xyz_bwd, dim3((unsigned)blocks), dim3(256), (size_t)4 * S * sizeof(float), (hipStream_t)stream, d_g_xyz_S3HW, d_params, S, H, W,
                       d_partial);
    const int rc = mpf_launch_status("k_src_xyz_bwd");
    return rc ? rc : mpf_plane_sum_finish(d_partial, blocks, S, d_grad_disparity, stream, "k_plane_sum_final");
}

// ---- HomographySample.sample_inverse: H_s = A + B / d_s, A = K_tgt R K_src^-1, B = K_tgt t n^T K_src^-1 with n = (0, 0, 1) ---------------------------------
// (X, Y, Z) = H_s (x, y, 1), flow = (X / Z - x, Y / Z - y).  B (x, y, 1) = (K_tgt t) <third row of K_src^-1, (x, y, 1)>, so d(X, Y, Z)/dd = -B (x, y, 1) / d^2
// and the flow's derivative follows by the quotient rule.  Record s: [0..8] H_tgt_src, [9] d_s, [10..12] K_tgt t, [13..15] the third row of K_src^-1.

__global__ void __launch_bounds__(256)
k_plane_flow_bwd(const float *__restrict__ g_flow, const float *__restrict__ params_, int S, int H, int W, float *__restrict__ partial)
{
    extern __shared__ float mpf_pfb_lds[];
    const MpfConstParams params = (MpfConstParams)params_;
    const int64_t N = (int64_t)H * W;
    const int64_t n0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = n0 < N;
    const int64_t n = live ? n0 : N - 1;
    const float fx = (float)(n % W), fy = (float)(n / W);
    for (int s = 0; s < S; ++s) {
        const MpfConstParams rec = params + MPF_PARAMS_HEADER + MPF_PLANE_RECORD * s;
        const float qx = mpf_row3_xy1(rec[0], rec[1], rec[2], fx, fy);               // the forward's (X, Y, Z) (k_homography_flow)
        const float qy = mpf_row3_xy1(rec[3], rec[4], rec[5], fx, fy);
        const float qz = mpf_row3_xy1(rec[6], rec[7], rec[8], fx, fy);
        const float d = rec[9];
        const float k = -mpf_row3_xy1(rec[13], rec[14], rec[15], fx, fy) / (d * d);
        const float bx = rec[10] * k, by = rec[11] * k, bz = rec[12] * k;            // d(X, Y, Z) / dd
        const float2 g = reinterpret_cast<const float2 *>(g_flow)[(int64_t)s * N + n];
        const float z2 = qz * qz;
        float v = g.x * ((bx * qz - qx * bz) / z2);
        v = fmaf(g.y, (by * qz - qy * bz) / z2, v);
        mpf_plane_sum_push(live ? v : 0.0f, s, S, mpf_pfb_lds);
    }
    mpf_plane_sum_flush(mpf_pfb_lds, S, partial + (int64_t)blockIdx.x * S);
}

extern "C" int mpf_plane_flow_bwd(const float *d_g_flow_SHW2, const float *d_params, int S, int H, int W, float *d_partial, int partial_blocks,
                                  float *d_grad_depth, void *stream)
{
    MPF_REQUIRE(d_g_flow_SHW2 && d_params && d_partial && d_grad_depth, "mpf_plane_flow_bwd: null pointer");
    MPF_REQUIRE(S >= 1 && S < 4096 && H >= 1 && W >= 1, "mpf_plane_flow_bwd: bad shape S=%d H=%d W=%d", S, H, W);
    MPF_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "mpf_plane_flow_bwd: H*W too large");
    MPF_REQUIRE((((uintptr_t)d_g_flow_SHW2) & 7) == 0, "mpf_plane_flow_bwd: the flow gradient must be 8-byte aligned");
    const int64_t N = (int64_t)H * W;
    const int blocks = (int)((N + 255) / 256);
    MPF_REQUIRE(partial_blocks >= blocks, "mpf_plane_flow_bwd: workspace of %d rows, %d blocks", partial_blocks, blocks);
    hipLaunchKernelGGL(k_plane_flow_bwd, dim3((unsigned)blocks), dim3(256), (size_t)4 * S * sizeof(float), (hipStream_t)stream, d_g_flow_SHW2, d_params, S, H, W,
                       d_partial);
    const int rc = mpf_launch_status("k_plane_flow_bwd");
    return rc ? rc : mpf_plane_sum_finish(d_partial, blocks, S, d_grad_depth, stream, "k_plane_sum_final");
}

