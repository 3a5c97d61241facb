// mpf_raft_eval.hip - what RAFT/evaluate.py does around the model on frames whose sides are no multiples of 8, for gfx950: InputPadder's
// replicate padding fused into the image scaling, the unpadded window of the last prediction written without the padded prediction, and
// the accumulators of validate_sintel / validate_kitti per frame.
//
// Contract: include/mpiflow_hip.h (MpfRaftEvalArgs).  pad = (left, right, top, bottom), each 0..7, as InputPadder._pad.
//
// k_raft_images_padded     pair[2N,3,Hp,Wp] = raft_scale(image[clamp(Y - top), clamp(X - left)]), image1 first: F.pad(mode='replicate') of both
//                          images, the scaling and the cat in one pass.  Wp is a multiple of 8: a lane owns 4 consecutive outputs of one row and
//                          stores them as one 16-byte vector (pair must be 16-byte aligned); source rows have any width and alignment, so the
//                          loads are scalar.  raft_scale is k_raft_images' own (mpf_raft_scale.h).
// k_upsample_crop          out[N,2,8H-top-bottom,8W-left-right] = the window of the convex upsampling.  k_upsample's layout (block = 64 consecutive
//                          coarse pixels, lane = pixel, wave = two sub-rows) and its arithmetic (mpf_convex.h).  A sub-position outside the window
//                          reads no mask and stores nothing, so a lane whose 8 x 8 block lies outside does no work and one that straddles the
//                          window writes only its inside.  Output rows have any width and alignment: scalar stores.
// k_upflow8_crop           the same window of 8 * bilinear(flow), align_corners=True: one lane per output element; the coordinates are those of
//                          the padded frame (mpf_upflow8.h), the window only offsets them.
// k_flow_metrics           per frame six fp64 accumulators: sum of epe, counted pixels, epe < 1, < 3, < 5, outliers (epe > 3 and epe / mag > 0.05;
//                          mag = 0 gives the IEEE quotient inf, an outlier, as torch gets).  epe and mag in fp32 as evaluate.py computes them.
//                          grid = (blocks per frame, N), grid-stride inside a frame; one partial row per block, folded per frame by
//                          k_flow_metrics_finish in a fixed order: no atomics, bit-identical from run to run.  Scalar loads: any H, W, alignment.
//
// No address depends on a tensor's values.  No LDS beyond the reductions' few hundred bytes.
#include "mpf_common.h"
#include "mpf_convex.h"
#include "mpf_math.h"             // mpf_store_vec
#include "mpf_raft_scale.h"
#include "mpf_reduce.h"
#include "mpf_upflow8.h"

#define EVAL_THREADS 256
#define EVAL_WAVES 4
#define EVAL_MAX_BLOCKS 2048     // the grid-stride kernels
#define MET_NACC 6               // sum epe, n(counted), n(epe < 1), n(epe < 3), n(epe < 5), n(outlier)
#define MET_MAX_BLOCKS 512       // k_flow_metrics: blocks per frame

static unsigned eval_blocks(int64_t lanes)
{
    int64_t blocks = (lanes + EVAL_THREADS - 1) / EVAL_THREADS;
    return (unsigned)(blocks > EVAL_MAX_BLOCKS ? EVAL_MAX_BLOCKS : blocks);
}

// every grid-stride loop below: t < total < 2^31 and the stride is at most EVAL_MAX_BLOCKS * EVAL_THREADS = 2^19, so the last increment cannot wrap

struct PadDev {
    const float *im1, *im2;
    float *pair;
    int H, W, Hp, Wp, left, top;
    unsigned planes1;            // 3N: the planes of image1
    unsigned total;              // lanes = 6N * Hp * Wp / 4
};

__global__ __launch_bounds__(EVAL_THREADS) void k_raft_images_padded(const PadDev a)
{
    constexpr int VEC = 4;
    const unsigned per_row = (unsigned)(a.Wp / VEC);
    for (unsigned t = blockIdx.x * EVAL_THREADS + threadIdx.x; t < a.total; t += gridDim.x * EVAL_THREADS) {
        const unsigned row = t / per_row;                                 // plane * Hp + Y
        const int X = (int)(t - row * per_row) * VEC;
        const unsigned plane = row / (unsigned)a.Hp;
        const int Y = (int)(row - plane * (unsigned)a.Hp);
        const int y = min(max(Y - a.top, 0), a.H - 1);
        const float *src = (plane < a.planes1 ? a.im1 + (size_t)plane * a.H * a.W : a.im2 + (size_t)(plane - a.planes1) * a.H * a.W) + (size_t)y * a.W;
        float v[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = raft_scale(src[min(max(X + e - a.left, 0), a.W - 1)]);
        mpf_store_vec<VEC>(a.pair + (size_t)row * a.Wp + X, v);
    }
}

struct CropDev {
    const float *flow, *mask;
    float *out;
    int N, H, W, HW, tiles;      // the coarse map
    int left, top, Ho, Wo;       // the window: rows top .. top + Ho - 1, columns left .. left + Wo - 1 of the [8H, 8W] prediction
    float sy, sx;                // k_upflow8_crop: up8_scale(H), up8_scale(W)
    unsigned total;              // k_upflow8_crop: N * 2 * Ho * Wo
};

__global__ __launch_bounds__(EVAL_THREADS) void k_upsample_crop(const CropDev a)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x / a.tiles, tile = blockIdx.x - n * a.tiles;
    const int H = a.H, W = a.W, HW = a.HW;
    const int p = tile * 64 + lane;
    if (p >= HW) return;                                                  // no barrier below
    const int h = p / W, w = p - h * W;
    // the sub-columns of this pixel inside the window: [jlo, jhi)
    const int jlo = max(0, a.left - 8 * w), jhi = min(8, a.left + a.Wo - 8 * w);
    if (jlo >= jhi) return;
    const int plane = 64 * HW;
    bool loaded = false;
    float f[2][9];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = wave * 2 + r;
        const int y = 8 * h + i - a.top;                                  // the output row
        if ((unsigned)y >= (unsigned)a.Ho) continue;
        if (!loaded) {
            up_neighbourhood(a.flow, n, H, W, h, w, f);
            loaded = true;
        }
        float *dst0 = a.out + ((size_t)(n * 2) * a.Ho + y) * a.Wo + (8 * w - a.left), *dst1 = dst0 + (size_t)a.Ho * a.Wo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < jlo || j >= jhi) continue;
            float m[9], o0, o1;
            up_convex(a.mask + (n * 576 + i * 8 + j) * HW + p, plane, f, m, o0, o1);
            dst0[j] = o0, dst1[j] = o1;
        }
    }
}

__global__ __launch_bounds__(EVAL_THREADS) void k_upflow8_crop(const CropDev a)
{
    for (unsigned t = blockIdx.x * EVAL_THREADS + threadIdx.x; t < a.total; t += gridDim.x * EVAL_THREADS) {
        const unsigned row = t / (unsigned)a.Wo;                          // plane * Ho + y
        const int x = (int)(t - row * (unsigned)a.Wo);
        const int plane = (int)(row / (unsigned)a.Ho), y = (int)(row - (unsigned)plane * a.Ho);
        int y0, y1, x0, x1;
        float ly, lx;
        up8_taps(y + a.top, a.H, a.sy, y0, y1, ly);
        up8_taps(x + a.left, a.W, a.sx, x0, x1, lx);
        const float *p0 = a.flow + ((size_t)plane * a.H + y0) * a.W, *p1 = a.flow + ((size_t)plane * a.H + y1) * a.W;
        a.out[t] = up8_value(p0, p1, x0, x1, 1.0f - ly, ly, 1.0f - lx, lx);
    }
}

struct MetDev {
    const float *pr, *gt, *valid;    // valid may be NULL
    double *partials;                // [N][blocks per frame][MET_NACC]
    double *metrics;                 // [N][MET_NACC]
    int HW;
};

__global__ __launch_bounds__(EVAL_THREADS) void k_flow_metrics(const MetDev a)
{
    __shared__ double sP[EVAL_WAVES * MET_NACC];
    const int n = blockIdx.y;
    const unsigned blocks = gridDim.x;
    const float *pu = a.pr + (size_t)n * 2 * a.HW, *pv = pu + a.HW, *gu = a.gt + (size_t)n * 2 * a.HW, *gv = gu + a.HW;
    const float *va = a.valid ? a.valid + (size_t)n * a.HW : nullptr;
    double esum = 0.0;
    int nv = 0, n1 = 0, n3 = 0, n5 = 0, no = 0;
    // i < HW < 2^30 and the stride is at most MET_MAX_BLOCKS * EVAL_THREADS = 2^17, so the last increment cannot wrap
    for (unsigned i = blockIdx.x * EVAL_THREADS + threadIdx.x; i < (unsigned)a.HW; i += blocks * EVAL_THREADS) {
        if (va && !(va[i] >= 0.5f)) continue;
        const float tu = gu[i], tv = gv[i];
        const float d0 = pu[i] - tu, d1 = pv[i] - tv;
        const float epe = sqrtf(d0 * d0 + d1 * d1), mag = sqrtf(tu * tu + tv * tv);
        esum += (double)epe;
        nv += 1, n1 += epe < 1.0f, n3 += epe < 3.0f, n5 += epe < 5.0f;
        no += epe > 3.0f && epe / mag > 0.05f;
    }
    const double part[MET_NACC] = {esum, (double)nv, (double)n1, (double)n3, (double)n5, (double)no};
    mpf_block_sums<EVAL_WAVES>(part, MET_NACC, sP, a.partials + ((size_t)n * blocks + blockIdx.x) * MET_NACC);
}

// one block per frame: its blocks' partials in a fixed order
__global__ __launch_bounds__(EVAL_THREADS) void k_flow_metrics_finish(const MetDev a, int blocks)
{
    __shared__ double sR[EVAL_THREADS];
    const int n = blockIdx.x;
    const double *part = a.partials + (size_t)n * blocks * MET_NACC;
    for (int q = 0; q < MET_NACC; ++q) {
        double v = 0.0;
        for (int b = threadIdx.x; b < blocks; b += EVAL_THREADS) v += part[(size_t)b * MET_NACC + q];
        mpf_block_tree_sum<EVAL_THREADS>(v, sR);
        if (threadIdx.x == 0) a.metrics[(size_t)n * MET_NACC + q] = sR[0];
        __syncthreads();
    }
}

static int eval_block(const MpfRaftEvalArgs *a, const char *who)
{
    MPF_REQUIRE(a, "%s: null argument block", who);
    MPF_REQUIRE(a->N >= 1 && a->H >= 1 && a->W >= 1, "%s: bad shape N, H, W = %d, %d, %d", who, a->N, a->H, a->W);
    return 0;
}

static int eval_pad(const MpfRaftEvalArgs *a, const char *who)
{
    MPF_REQUIRE((unsigned)a->pad_left < 8u && (unsigned)a->pad_right < 8u && (unsigned)a->pad_top < 8u && (unsigned)a->pad_bottom < 8u,
                "%s: bad shape: every pad must be 0..7 (got left, right, top, bottom = %d, %d, %d, %d)", who, a->pad_left, a->pad_right, a->pad_top,
                a->pad_bottom);
    return 0;
}

extern "C" int mpf_raft_images_padded(const MpfRaftEvalArgs *a, void *stream)
{
    const char *who = "mpf_raft_images_padded";
    int rc = eval_block(a, who);
    if (rc) return rc;
    if ((rc = eval_pad(a, who))) return rc;
    const int64_t Hp = (int64_t)a->H + a->pad_top + a->pad_bottom, Wp = (int64_t)a->W + a->pad_left + a->pad_right;
    MPF_REQUIRE(Hp % 8 == 0 && Wp % 8 == 0, "%s: bad shape: the padded frame must have sides that are multiples of 8 (H, W = %d, %d pad to %lld x %lld)", who,
                a->H, a->W, (long long)Hp, (long long)Wp);
    const int64_t lim = (int64_t)1 << 31;
    MPF_REQUIRE(Hp * Wp < lim / 6 && (int64_t)a->N * Hp * Wp < lim / 6, "%s: pair [2N,3,Hp,Wp] must hold fewer than 2^31 elements (N, Hp, Wp = %d, %lld, %lld)",
                who, a->N, (long long)Hp, (long long)Wp);
    MPF_REQUIRE(a->image1 && a->image2 && a->pair, "%s: null pointer (image1, image2 or pair)", who);
    MPF_REQUIRE(mpf_aligned16(a->pair), "%s: pair must be 16-byte aligned", who);      // Wp % 8 == 0: every row then starts 16-byte aligned
    PadDev d = PadDev{};
    d.im1 = a->image1, d.im2 = a->image2, d.pair = a->pair;
    d.H = a->H, d.W = a->W, d.Hp = (int)Hp, d.Wp = (int)Wp, d.left = a->pad_left, d.top = a->pad_top;
    d.planes1 = 3u * (unsigned)a->N;
    d.total = (unsigned)((int64_t)a->N * 6 * Hp * Wp / 4);
    hipLaunchKernelGGL(k_raft_images_padded, dim3(eval_blocks(d.total)), dim3(EVAL_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_raft_images_padded");
}

// the two cropped upsamplings: the coarse map, the pad, the window; `channels`: of the largest tensor per coarse pixel (576: the mask; 128: flow_up)
static int crop_dev(const MpfRaftEvalArgs *a, const char *who, int64_t channels, const char *largest, CropDev &d)
{
    int rc = eval_block(a, who);
    if (rc) return rc;
    if ((rc = eval_pad(a, who))) return rc;
    const int Ho = 8 * (int64_t)a->H - a->pad_top - a->pad_bottom > 0 ? (int)(8 * (int64_t)a->H - a->pad_top - a->pad_bottom) : 0;
    const int Wo = 8 * (int64_t)a->W - a->pad_left - a->pad_right > 0 ? (int)(8 * (int64_t)a->W - a->pad_left - a->pad_right) : 0;
    MPF_REQUIRE(Ho >= 1 && Wo >= 1, "%s: bad shape: the pad leaves no window of the %d x %d coarse map's prediction (left, right, top, bottom = %d, %d, %d, %d)", who,
                a->H, a->W, a->pad_left, a->pad_right, a->pad_top, a->pad_bottom);
    const int64_t lim = (int64_t)1 << 31;
    const int64_t hw = (int64_t)a->H * a->W;
    MPF_REQUIRE(hw < lim / channels && (int64_t)a->N * hw < lim / channels, "%s: %s must hold fewer than 2^31 elements (N, H, W = %d, %d, %d)", who, largest, a->N,
                a->H, a->W);
    MPF_REQUIRE(a->flow && a->flow_up && (channels != 576 || a->mask), "%s: null pointer (flow, %sflow_up)", who, channels == 576 ? "mask or " : "or ");
    d = CropDev{};
    d.flow = a->flow, d.mask = a->mask, d.out = a->flow_up;
    d.N = a->N, d.H = a->H, d.W = a->W, d.HW = (int)hw, d.tiles = (int)((hw + 63) / 64);
    d.left = a->pad_left, d.top = a->pad_top, d.Ho = Ho, d.Wo = Wo;
    d.sy = up8_scale(a->H), d.sx = up8_scale(a->W);
    d.total = (unsigned)((int64_t)a->N * 2 * Ho * Wo);
    return 0;
}

extern "C" int mpf_upsample_flow_crop(const MpfRaftEvalArgs *a, void *stream)
{
    CropDev d;
    const int rc = crop_dev(a, "mpf_upsample_flow_crop", 576, "mask [N,576,H,W]", d);
    if (rc) return rc;
    hipLaunchKernelGGL(k_upsample_crop, dim3((unsigned)((int64_t)d.N * d.tiles)), dim3(EVAL_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_upsample_crop");
}

extern "C" int mpf_upflow8_crop(const MpfRaftEvalArgs *a, void *stream)
{
    CropDev d;
    const int rc = crop_dev(a, "mpf_upflow8_crop", 128, "the padded prediction [N,2,8H,8W]", d);
    if (rc) return rc;
    hipLaunchKernelGGL(k_upflow8_crop, dim3(eval_blocks(d.total)), dim3(EVAL_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_upflow8_crop");
}

// N, H, W >= 1 and flow [N,2,H,W] below 2^31 elements; the blocks per frame of k_flow_metrics (one partial row each)
static int met_shape(int N, int H, int W, const char *who, int64_t &blocks)
{
    MPF_REQUIRE(N >= 1 && H >= 1 && W >= 1, "%s: bad shape N, H, W = %d, %d, %d", who, N, H, W);
    const int64_t lim = (int64_t)1 << 31;
    const int64_t hw = (int64_t)H * W;
    MPF_REQUIRE(hw < lim / 2 && (int64_t)N * hw < lim / 2, "%s: flow [N,2,H,W] must hold fewer than 2^31 elements (N, H, W = %d, %d, %d)", who, N, H, W);
    MPF_REQUIRE(N <= 65535, "%s: bad shape: at most 65535 frames per call (got N = %d)", who, N);
    blocks = (hw + EVAL_THREADS - 1) / EVAL_THREADS;
    if (blocks > MET_MAX_BLOCKS) blocks = MET_MAX_BLOCKS;
    return 0;
}

extern "C" size_t mpf_flow_metrics_workspace(int N, int H, int W)
{
    int64_t blocks;
    if (met_shape(N, H, W, "mpf_flow_metrics_workspace", blocks)) return 0;
    return (size_t)N * blocks * MET_NACC * sizeof(double);
}

extern "C" int mpf_flow_metrics(const MpfRaftEvalArgs *a, void *stream)
{
    const char *who = "mpf_flow_metrics";
    MPF_REQUIRE(a, "%s: null argument block", who);
    int64_t blocks;
    const int rc = met_shape(a->N, a->H, a->W, who, blocks);
    if (rc) return rc;
    MPF_REQUIRE(a->flow_pr && a->flow_gt && a->metrics, "%s: null pointer (flow_pr, flow_gt or metrics)", who);
    const size_t need = (size_t)a->N * blocks * MET_NACC * sizeof(double);
    MPF_REQUIRE(a->workspace, "%s: null pointer (workspace)", who);
    MPF_REQUIRE((((uintptr_t)a->workspace) & 7) == 0 && (((uintptr_t)a->metrics) & 7) == 0, "%s: workspace and metrics must be 8-byte aligned", who);
    MPF_REQUIRE(a->workspace_bytes >= need, "%s: workspace holds %zu bytes, %zu needed (mpf_flow_metrics_workspace)", who, a->workspace_bytes, need);
    MetDev d = MetDev{};
    d.pr = a->flow_pr, d.gt = a->flow_gt, d.valid = a->valid, d.partials = (double *)a->workspace, d.metrics = a->metrics;
    d.HW = a->H * a->W;
    hipLaunchKernelGGL(k_flow_metrics, dim3((unsigned)blocks, (unsigned)a->N), dim3(EVAL_THREADS), 0, (hipStream_t)stream, d);
    const int st = mpf_launch_status("k_flow_metrics");
    if (st) return st;
    hipLaunchKernelGGL(k_flow_metrics_finish, dim3((unsigned)a->N), dim3(EVAL_THREADS), 0, (hipStream_t)stream, d, (int)blocks);
    return mpf_launch_status("k_flow_metrics_finish");
}
