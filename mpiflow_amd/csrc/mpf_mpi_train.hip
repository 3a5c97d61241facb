// mpf_mpi_train.hip - the training-time half of the reference's utils/mpi for gfx950: gather_pixel_by_pxpy (rendering_utils.py:26-43) with its
// scatter adjoint, sample_pdf (rendering_utils.py:90-139) and disparity_consistency_src_to_tgt (mpi_rendering.py:180-210) with its adjoint.
//
// Contract: include/mpiflow_hip.h (MpfGatherPxpyArgs, MpfSamplePdfArgs, MpfDispConsistencyArgs); INTEGRATION.md section 21 holds the definitions,
// which tests/mpi_training_restated.py restates in float64.  The build has no contraction and correctly rounded divides.
//
// mpt_index        the pixel index both the gather and the loss use: round to nearest even, then clamp.  The clamp is taken on the rounded FLOAT,
//                  so the cast never sees a value outside [0, n - 1]: NaN and -inf read index 0, +inf (and every finite value past the frame)
//                  the last index.
// k_gather_pxpy    one thread per point, a loop over the channels.  k_gather_pxpy_bwd: the same walk, a float atomic add per channel into a
//                  zeroed gradient (points that share a pixel decide the last bits of its sum by their arrival order).
// k_sample_pdf     a workgroup takes a tile of TR rows (a row = one ray: S values, S weights, NS draws).  Rows are contiguous, so values and
//                  weights enter LDS by coalesced loads, at odd row strides (thread r walks row r: the rows fall into different banks); thread
//                  r < TR then turns its row of weights into the cdf in place, sequentially, as torch's CPU cumsum does (a running f64 sum, every entry rounded to f32).  The draws of a tile are one
//                  contiguous range of u and of the output: the workgroup walks that range in flat order, so both u's load and the sample's
//                  store are coalesced as they stand and need no staging; each draw binary-searches its row's cdf in LDS.  Expanded values
//                  (stride 0 over the rays) are staged from the one row of their batch entry, in place.  LDS at S = 128: 32 rows x 258 words =
//                  33,024 bytes; at S <= 64: 64 rows x 130 words = 33,280 bytes - four to five workgroups of the 160 KiB of a CU.
// k_dispc_fwd      one thread per source pixel.  The masked sum of |1 / p.z - d_tgt[idx]| and the count go wave butterfly -> one LDS slot per
//                  wave -> a per-block partial; k_dispc_final adds the partials in block order in double (256 threads own consecutive chunks,
//                  thread 0 adds the 256 chunk sums in order) and divides.  No atomics: two runs give the same bits.  Loss and count stay on
//                  the device.
// k_dispc_bwd      recomputes the pixel, one store for d_src's gradient (reproducible), one float atomic add into d_tgt's zeroed gradient.
//
// No workgroup waits for another, every loop is bounded by S, NS or C, and every index that depends on a tensor's value is clamped to its frame.
#include "mpf_common.h"
#include "mpf_math.h"
#include "mpf_reduce.h"
#include <math.h>

#define MPT_THREADS 256

MPF_DEV int mpt_index(float v, int n)
{
    const float r = rintf(v);                                   // ties to even, as torch.round
    if (!(r >= 0.0f)) return 0;                                 // negatives, -inf and NaN
    if (r >= (float)(n - 1)) return n - 1;                      // +inf too
    return (int)r;
}

MPF_DEV int mpt_index(long long v, int n) { return v < 0 ? 0 : (v > (long long)(n - 1) ? n - 1 : (int)v); }

// ---------------------------------------------------------------- gather_pixel_by_pxpy

template <typename P, bool BWD>
__global__ __launch_bounds__(MPT_THREADS) void k_gather_pxpy(const float *__restrict__ src, const P *__restrict__ pxpy, float *__restrict__ dst, int C,
                                                             int H, int W, int N)
{
    const int n = (int)(blockIdx.x * MPT_THREADS + threadIdx.x);
    if (n >= N) return;
    const int b = (int)blockIdx.y;
    const P *pp = pxpy + (size_t)b * 2 * N;
    const int ix = mpt_index(pp[n], W), iy = mpt_index(pp[N + n], H);
    const size_t hw = (size_t)H * W, o = (size_t)iy * W + ix;
    for (int c = 0; c < C; ++c) {
        const size_t img = ((size_t)b * C + c) * hw + o, pt = ((size_t)b * C + c) * N + n;
        if (BWD) atomicAdd(dst + img, src[pt]);                 // src: the upstream gradient [B,C,N]; dst: grad_img [B,C,H,W], zeroed
        else dst[pt] = src[img];                                // src: img [B,C,H,W]; dst: out [B,C,N]
    }
}

static int gather_check(const MpfGatherPxpyArgs *a, const char *who, const void *written, const char *written_name)
{
    MPF_REQUIRE(a, "%s: null argument block", who);
    MPF_REQUIRE(a->pxpy_dtype == MPF_PXPY_F32 || a->pxpy_dtype == MPF_PXPY_I64, "%s: pxpy_dtype must be 0 (f32) or 1 (i64) (got %d)", who, a->pxpy_dtype);
    MPF_REQUIRE(a->B >= 1 && a->B <= 65535 && a->C >= 1 && a->H >= 1 && a->W >= 1 && a->N >= 1,
                "%s: bad shape: B must be 1..65535 and C, H, W, N at least 1 (got B, C, H, W, N = %d, %d, %d, %d, %d)", who, a->B, a->C, a->H, a->W, a->N);
    MPF_REQUIRE((int64_t)a->B * a->C * a->H * a->W < ((int64_t)1 << 31) && (int64_t)a->B * a->C * a->N < ((int64_t)1 << 31),
                "%s: bad shape: B * C * H * W and B * C * N must stay below 2^31 (got B, C, H, W, N = %d, %d, %d, %d, %d)", who, a->B, a->C, a->H, a->W, a->N);
    MPF_REQUIRE(a->pxpy && written, "%s: null pointer (pxpy, %s)", who, written_name);
    return 0;
}

template <bool BWD>
static int gather_launch(const MpfGatherPxpyArgs *a, const float *src, float *dst, void *stream, const char *what)
{
    const dim3 grid((unsigned)((a->N + MPT_THREADS - 1) / MPT_THREADS), (unsigned)a->B);
    if (a->pxpy_dtype == MPF_PXPY_F32)
        hipLaunchKernelGGL((k_gather_pxpy<float, BWD>), grid, dim3(MPT_THREADS), 0, (hipStream_t)stream, src, (const float *)a->pxpy, dst, a->C, a->H, a->W, a->N);
    else
        hipLaunchKernelGGL((k_gather_pxpy<long long, BWD>), grid, dim3(MPT_THREADS), 0, (hipStream_t)stream, src, (const long long *)a->pxpy, dst, a->C, a->H,
                           a->W, a->N);
    return mpf_launch_status(what);
}

extern "C" int mpf_gather_pxpy(const MpfGatherPxpyArgs *a, void *stream)
{
    const char *who = "mpf_gather_pxpy";
    const int rc = gather_check(a, who, a ? a->out : nullptr, "out");
    if (rc) return rc;
    MPF_REQUIRE(a->img, "%s: null pointer (img)", who);
    return gather_launch<false>(a, a->img, a->out, stream, "k_gather_pxpy");
}

extern "C" int mpf_gather_pxpy_bwd(const MpfGatherPxpyArgs *a, void *stream)
{
    const char *who = "mpf_gather_pxpy_bwd";
    const int rc = gather_check(a, who, a ? a->grad_img : nullptr, "grad_img");
    if (rc) return rc;
    MPF_REQUIRE(a->grad_out, "%s: null pointer (grad_out)", who);
    return gather_launch<true>(a, a->grad_out, a->grad_img, stream, "k_gather_pxpy_bwd");
}

// ---------------------------------------------------------------- sample_pdf

#define MPT_PDF_LDS_WORDS 8320                                  // 32 rows x (129 + 129) at S = 128; 64 rows x (65 + 65) at S <= 64

struct PdfDev {
    const float *values, *weights, *u;
    float *out;
    long long values_batch_stride, values_row_stride;           // in floats; the row stride is S, or 0 for values expanded over the rays
    long long R;                                                // rows: B * N
    int N, S, NS, TR, sv, sc;                                   // rows per tile; the LDS row strides of the values and of the cdf (both odd)
};

__global__ __launch_bounds__(MPT_THREADS) void k_sample_pdf(const PdfDev a)
{
    __shared__ float lds[MPT_PDF_LDS_WORDS];
    float *sV = lds, *sC = lds + a.TR * a.sv;
    const long long row0 = (long long)blockIdx.x * a.TR;
    const int rows = (int)(a.R - row0 < (long long)a.TR ? a.R - row0 : (long long)a.TR);
    const int S = a.S, NS = a.NS;
    for (int i = (int)threadIdx.x; i < rows * S; i += MPT_THREADS) {
        const int r = i / S, j = i - r * S;
        const long long row = row0 + r;
        const long long b = row / a.N, n = row - b * a.N;
        sV[r * a.sv + j] = a.values[b * a.values_batch_stride + n * a.values_row_stride + j];
        sC[r * a.sc + 1 + j] = a.weights[row0 * S + i];
    }
    __syncthreads();
    if ((int)threadIdx.x < rows) {                              // the row's cdf in place: sC[0] = 0, sC[k + 1] = sC[k] + w[k] / (sum w + 1e-5)
        float *c = sC + (int)threadIdx.x * a.sc;
        double sum = 0.0;                                       // torch.sum is no sequential f32 sum: the correctly rounded one is within an ulp of it
        for (int k = 1; k <= S; ++k) sum += (double)c[k];
        const float den = (float)sum + 1e-5f;
        double acc = 0.0;                                       // torch's CPU cumsum of f32 keeps its running sum in f64 and rounds every output
        c[0] = 0.0f;
        for (int k = 1; k <= S; ++k) {
            acc += (double)(c[k] / den);                        // the pdf entry itself is an f32 divide
            c[k] = (float)acc;
        }
    }
    __syncthreads();
    const long long base = row0 * NS;
    for (int i = (int)threadIdx.x; i < rows * NS; i += MPT_THREADS) {
        const int r = i / NS;
        const float *c = sC + r * a.sc, *v = sV + r * a.sv;
        const float u = a.u[base + i];
        int lo = 0, hi = S + 1;                                  // searchsorted(right=True): the first index whose cdf is greater than u
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (!(c[mid] > u)) lo = mid + 1;
            else hi = mid;
        }
        const int il = lo - 1 < 0 ? 0 : lo - 1, iu = lo > S ? S : lo;
        const float cl = c[il], ch = c[iu];
        // bin edges: the values' midpoints with both ends duplicated
        const float el = il == 0 ? v[0] : (il == S ? v[S - 1] : (v[il] + v[il - 1]) * 0.5f);
        const float eh = iu == 0 ? v[0] : (iu == S ? v[S - 1] : (v[iu] + v[iu - 1]) * 0.5f);
        const float ci = ch - cl, bi = eh - el, ul = u - cl;
        float t = ul / (ci < 1e-5f ? 1e-5f : ci);
        if (ci <= 1e-4f) t = 0.5f;
        a.out[base + i] = el + t * bi;
    }
}

extern "C" int mpf_sample_pdf(const MpfSamplePdfArgs *a, void *stream)
{
    const char *who = "mpf_sample_pdf";
    MPF_REQUIRE(a, "%s: null argument block", who);
    MPF_REQUIRE(a->B >= 1 && a->N >= 1, "%s: bad shape: B and N must be at least 1 (got B, N = %d, %d)", who, a->B, a->N);
    MPF_REQUIRE(a->S >= 1 && a->S <= MPF_SAMPLE_PDF_MAX_S, "%s: S must be 1..%d (got %d)", who, MPF_SAMPLE_PDF_MAX_S, a->S);
    MPF_REQUIRE(a->n_samples >= 1 && a->n_samples <= MPF_SAMPLE_PDF_MAX_SAMPLES, "%s: n_samples must be 1..%d (got %d)", who, MPF_SAMPLE_PDF_MAX_SAMPLES,
                a->n_samples);
    const int64_t R = (int64_t)a->B * a->N;
    const int widest = a->S > a->n_samples ? a->S : a->n_samples;
    MPF_REQUIRE(R * widest < ((int64_t)1 << 31), "%s: bad shape: B * N * max(S, n_samples) must stay below 2^31 (got B, N, S, n_samples = %d, %d, %d, %d)", who,
                a->B, a->N, a->S, a->n_samples);
    MPF_REQUIRE(a->values_row_stride == 0 || a->values_row_stride == a->S, "%s: values_row_stride must be S (contiguous rows) or 0 (expanded over the rays) (got %lld)",
                who, (long long)a->values_row_stride);
    MPF_REQUIRE(a->values_batch_stride >= 0, "%s: values_batch_stride must not be negative (got %lld)", who, (long long)a->values_batch_stride);
    MPF_REQUIRE(a->values && a->weights && a->u && a->out, "%s: null pointer (values, weights, u, out)", who);
    PdfDev d = PdfDev{};
    d.values = a->values, d.weights = a->weights, d.u = a->u, d.out = a->out;
    d.values_batch_stride = a->values_batch_stride, d.values_row_stride = a->values_row_stride;
    d.R = R, d.N = a->N, d.S = a->S, d.NS = a->n_samples;
    d.sv = a->S | 1, d.sc = (a->S + 1) | 1;
    d.TR = a->S <= 64 ? 64 : 32;
    if (d.TR * (d.sv + d.sc) > MPT_PDF_LDS_WORDS) {
        mpf_set_error("%s: internal: a tile of %d rows of S = %d does not fit the LDS image", who, d.TR, a->S);
        return MPF_ERR_UNSUPPORTED;
    }
    const unsigned blocks = (unsigned)((R + d.TR - 1) / d.TR);
    hipLaunchKernelGGL(k_sample_pdf, dim3(blocks), dim3(MPT_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_sample_pdf");
}

// ---------------------------------------------------------------- disparity_consistency_src_to_tgt

struct DispcPixel {
    bool mask;
    int idx;                                                    // the rounded, clamped target pixel
    float inv_pz;                                               // 1 / p.z: the source disparity seen from the target
    float depth, gr;                                            // 1 / d_src; G[2,:3] . r
};

// r = K_src_inv (x, y, 1); xyz = r * depth; p = G (xyz, 1); q = K_tgt p; (px, py) = q.xy / q.z - the reference's own sequence
MPF_DEV DispcPixel dispc_pixel(const float *__restrict__ Ki, const float *__restrict__ G, const float *__restrict__ Kt, float d_src, int x, int y, int H, int W)
{
    DispcPixel o;
    const float fx = (float)x, fy = (float)y;
    const float r0 = mpf_row3_xy1(Ki[0], Ki[1], Ki[2], fx, fy), r1 = mpf_row3_xy1(Ki[3], Ki[4], Ki[5], fx, fy), r2 = mpf_row3_xy1(Ki[6], Ki[7], Ki[8], fx, fy);
    o.depth = 1.0f / d_src;
    const float X = r0 * o.depth, Y = r1 * o.depth, Z = r2 * o.depth;
    const float p0 = mpf_row4_xyz1(G[0], G[1], G[2], G[3], X, Y, Z), p1 = mpf_row4_xyz1(G[4], G[5], G[6], G[7], X, Y, Z);
    const float p2 = mpf_row4_xyz1(G[8], G[9], G[10], G[11], X, Y, Z);
    const float q0 = fmaf(Kt[2], p2, fmaf(Kt[1], p1, Kt[0] * p0)), q1 = fmaf(Kt[5], p2, fmaf(Kt[4], p1, Kt[3] * p0));
    const float q2 = fmaf(Kt[8], p2, fmaf(Kt[7], p1, Kt[6] * p0));
    const float px = q0 / q2, py = q1 / q2;
    o.mask = px >= 0.0f && px <= (float)(W - 1) && py >= 0.0f && py <= (float)(H - 1);      // NaN compares false
    o.idx = mpt_index(py, H) * W + mpt_index(px, W);
    o.inv_pz = 1.0f / p2;
    o.gr = fmaf(G[10], r2, fmaf(G[9], r1, G[8] * r0));
    return o;
}

// workspace: [0] double sum, [1] int64 count, then float partial sums [blocks], then int partial counts [blocks]
#define MPT_WS_HEAD 16

__global__ __launch_bounds__(MPT_THREADS) void k_dispc_fwd(const float *__restrict__ Ki, const float *__restrict__ G, const float *__restrict__ Kt,
                                                           const float *__restrict__ d_src, const float *__restrict__ d_tgt, int H, int W,
                                                           float *__restrict__ part_sum, int *__restrict__ part_cnt)
{
    __shared__ float s_sum[MPT_THREADS / 64];
    __shared__ int s_cnt[MPT_THREADS / 64];
    const int hw = H * W, p = (int)(blockIdx.x * MPT_THREADS + threadIdx.x), b = (int)blockIdx.y;
    float v = 0.0f;
    int c = 0;
    if (p < hw) {                                               // threads past the frame stay for the butterfly, with nothing to add
        const int y = p / W, x = p - y * W;
        const DispcPixel o = dispc_pixel(Ki + b * 9, G + b * 16, Kt + b * 9, d_src[(size_t)b * hw + p], x, y, H, W);
        if (o.mask) {
            v = fabsf(o.inv_pz - d_tgt[(size_t)b * hw + o.idx]);
            c = 1;
        }
    }
    v = mpf_wave_sum(v), c = mpf_wave_sum(c);
    // the float sum and the int count share one barrier, so the block step is spelt out here and not two mpf_block_sums calls
    if ((threadIdx.x & 63u) == 0) s_sum[threadIdx.x >> 6] = v, s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = s_sum[0];
        int n = s_cnt[0];
        for (int w = 1; w < MPT_THREADS / 64; ++w) a += s_sum[w], n += s_cnt[w];
        const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        part_sum[blk] = a;
        part_cnt[blk] = n;
    }
}

__global__ __launch_bounds__(MPT_THREADS) void k_dispc_final(const float *__restrict__ part_sum, const int *__restrict__ part_cnt, int blocks,
                                                             double *__restrict__ head_sum, long long *__restrict__ head_cnt, float *__restrict__ loss)
{
    __shared__ double s_sum[MPT_THREADS];
    __shared__ long long s_cnt[MPT_THREADS];
    const int per = (blocks + MPT_THREADS - 1) / MPT_THREADS;
    const int b0 = (int)threadIdx.x * per, b1 = b0 + per < blocks ? b0 + per : blocks;
    double a = 0.0;
    long long n = 0;
    for (int b = b0; b < b1; ++b) a += (double)part_sum[b], n += part_cnt[b];
    s_sum[threadIdx.x] = a, s_cnt[threadIdx.x] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        a = 0.0, n = 0;
        for (int t = 0; t < MPT_THREADS; ++t) a += s_sum[t], n += s_cnt[t];
        *head_sum = a, *head_cnt = n;
        *loss = (float)(a / (double)n);                         // count 0: 0 / 0 = NaN, the mean of an empty selection
    }
}

__global__ __launch_bounds__(MPT_THREADS) void k_dispc_bwd(const float *__restrict__ Ki, const float *__restrict__ G, const float *__restrict__ Kt,
                                                           const float *__restrict__ d_src, const float *__restrict__ d_tgt, int H, int W,
                                                           const float *__restrict__ g_loss, const long long *__restrict__ head_cnt,
                                                           float *__restrict__ grad_src, float *__restrict__ grad_tgt)
{
    const int hw = H * W, p = (int)(blockIdx.x * MPT_THREADS + threadIdx.x), b = (int)blockIdx.y;
    if (p >= hw) return;
    const int y = p / W, x = p - y * W;
    const DispcPixel o = dispc_pixel(Ki + b * 9, G + b * 16, Kt + b * 9, d_src[(size_t)b * hw + p], x, y, H, W);
    float gs = 0.0f;
    if (o.mask) {                                               // with count 0 no pixel comes here: every gradient stays 0
        const float diff = o.inv_pz - d_tgt[(size_t)b * hw + o.idx];
        const float sgn = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);
        const float gd = (g_loss[0] / (float)head_cnt[0]) * sgn;                            // dL/d(1 / p.z); NaN's sign is 0
        if (grad_tgt && sgn != 0.0f) atomicAdd(grad_tgt + (size_t)b * hw + o.idx, -gd);
        const float g_pz = -gd * (o.inv_pz * o.inv_pz);
        const float g_depth = g_pz * o.gr;
        gs = -g_depth * (o.depth * o.depth);
    }
    if (grad_src) grad_src[(size_t)b * hw + p] = gs;
}

static int dispc_shape(int B, int H, int W, const char *who)
{
    MPF_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "%s: bad shape: B must be 1..65535 and H, W at least 1 (got B, H, W = %d, %d, %d)", who, B, H, W);
    MPF_REQUIRE((int64_t)B * H * W < ((int64_t)1 << 31), "%s: bad shape: B * H * W must stay below 2^31 (got B, H, W = %d, %d, %d)", who, B, H, W);
    return 0;
}

static int dispc_blocks(int H, int W) { return (int)(((int64_t)H * W + MPT_THREADS - 1) / MPT_THREADS); }

extern "C" size_t mpf_disp_consistency_workspace(int B, int H, int W)
{
    if (dispc_shape(B, H, W, "mpf_disp_consistency_workspace")) return 0;
    return MPT_WS_HEAD + (size_t)B * dispc_blocks(H, W) * (sizeof(float) + sizeof(int));
}

static int dispc_check(const MpfDispConsistencyArgs *a, const char *who)
{
    MPF_REQUIRE(a, "%s: null argument block", who);
    const int rc = dispc_shape(a->B, a->H, a->W, who);
    if (rc) return rc;
    MPF_REQUIRE(a->K_src_inv && a->G_tgt_src && a->K_tgt && a->disparity_src && a->disparity_tgt,
                "%s: null pointer (K_src_inv, G_tgt_src, K_tgt, disparity_src, disparity_tgt)", who);
    MPF_REQUIRE(a->workspace, "%s: null pointer (workspace)", who);
    MPF_REQUIRE((((uintptr_t)a->workspace) & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    const size_t need = mpf_disp_consistency_workspace(a->B, a->H, a->W);
    MPF_REQUIRE(a->workspace_bytes >= need, "%s: workspace holds %zu bytes, %zu needed (mpf_disp_consistency_workspace)", who, a->workspace_bytes, need);
    return 0;
}

extern "C" int mpf_disp_consistency(const MpfDispConsistencyArgs *a, void *stream)
{
    const char *who = "mpf_disp_consistency";
    const int rc = dispc_check(a, who);
    if (rc) return rc;
    MPF_REQUIRE(a->loss, "%s: null pointer (loss)", who);
    const int per = dispc_blocks(a->H, a->W), blocks = a->B * per;
    char *ws = (char *)a->workspace;
    float *part_sum = (float *)(ws + MPT_WS_HEAD);
    int *part_cnt = (int *)(part_sum + blocks);
    hipLaunchKernelGGL(k_dispc_fwd, dim3((unsigned)per, (unsigned)a->B), dim3(MPT_THREADS), 0, (hipStream_t)stream, a->K_src_inv, a->G_tgt_src, a->K_tgt,
                       a->disparity_src, a->disparity_tgt, a->H, a->W, part_sum, part_cnt);
    const int st = mpf_launch_status("k_dispc_fwd");
    if (st) return st;
    hipLaunchKernelGGL(k_dispc_final, dim3(1), dim3(MPT_THREADS), 0, (hipStream_t)stream, part_sum, part_cnt, blocks, (double *)ws, (long long *)(ws + 8), a->loss);
    return mpf_launch_status("k_dispc_final");
}

extern "C" int mpf_disp_consistency_bwd(const MpfDispConsistencyArgs *a, void *stream)
{
    const char *who = "mpf_disp_consistency_bwd";
    const int rc = dispc_check(a, who);
    if (rc) return rc;
    MPF_REQUIRE(a->grad_loss, "%s: null pointer (grad_loss)", who);
    MPF_REQUIRE(a->grad_disparity_src || a->grad_disparity_tgt, "%s: null pointer (grad_disparity_src and grad_disparity_tgt: one at least)", who);
    const char *ws = (const char *)a->workspace;
    hipLaunchKernelGGL(k_dispc_bwd, dim3((unsigned)dispc_blocks(a->H, a->W), (unsigned)a->B), dim3(MPT_THREADS), 0, (hipStream_t)stream, a->K_src_inv, a->G_tgt_src,
                       a->K_tgt, a->disparity_src, a->disparity_tgt, a->H, a->W, a->grad_loss, (const long long *)(ws + 8), a->grad_disparity_src,
                       a->grad_disparity_tgt);
    return mpf_launch_status("k_dispc_bwd");
}
