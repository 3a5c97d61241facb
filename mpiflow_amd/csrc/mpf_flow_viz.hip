// mpf_flow_viz.hip - what upstream RAFT does with a prediction, for gfx950: demo.py's colour coding (RAFT/core/utils/flow_viz.py: flow_to_image,
// flow_uv_to_colors, make_colorwheel), optionally stacked under the frame (demo.py:viz), and the code of KITTI's 16-bit flow PNG
// (frame_utils.writeFlowKITTI up to the file).
//
// Contract: include/mpiflow_hip.h (MpfFlowVizArgs).
//
// k_flow_rad_max           per image and block the maximum of rad = sqrt(u^2 + v^2) (fp32, after the optional clip) over the block's pixels
//                          into one slot of the workspace: grid = (blocks per image, N), grid-stride inside an image.  A maximum does not
//                          depend on the order: no atomics, bit-identical from run to run.  NaN is dropped (fmaxf).
// k_flow_colour            the colouring pass.  The output [N,P,3] u8 (P = H * W pixels, 2 * H * W with the frame on top) is one flat run of
//                          N * P pixels of 3 bytes.  A lane owns 4 consecutive pixels, 12 bytes, and stores them as 3 dwords: a wave writes 768
//                          consecutive bytes (out must be 4-byte aligned; the last lane stores the bytes of its remaining pixels one by one).
//                          A block owns 1024 consecutive pixels, which may belong to several images: each wave folds the slots of the images
//                          the block touches into LDS first (rad_max + 1e-5, the divisor), so there is no launch and no host step in between.
//                          Arithmetic and precisions are upstream's: u, v, rad, a = atan2(-v, -u) / pi and fk in fp32; the wheel, the blend,
//                          the rad <= 1 / 0.75 branches and floor(255 * col) in fp64.  k0 is clamped to 0..54 before it indexes the wheel.
// k_flow_encode_kitti      out [N,H,W,3] u16 = (64 * u + 2^15, 64 * v + 2^15, valid), each product and sum rounded in fp32, truncated toward
//                          zero, clamped to 0..65535 (NaN: 0).  A lane owns 2 consecutive pixels, 12 bytes, stored as 3 dwords.
//
// The only value-dependent address is the wheel entry (LDS, index clamped).  Flow and frame rows have any width and alignment: scalar loads.
#include "mpf_common.h"
#include "mpf_reduce.h"

#define VIZ_THREADS 256
#define VIZ_WAVES 4
#define VIZ_PX 4                                   // pixels per lane of k_flow_colour
#define VIZ_BLOCK_PX (VIZ_THREADS * VIZ_PX)
#define VIZ_MAX_SLOTS 256                          // k_flow_rad_max: blocks per image
#define VIZ_NCOLS 55                               // 15 + 6 + 4 + 11 + 13 + 6

struct VizDev {
    const float *flow, *image, *valid;
    float *slots;                                  // [N][blocks per image]
    unsigned char *out8;
    unsigned short *out16;
    unsigned HW, P, total;                         // pixels of a frame, of an output image, of the whole output
    int nslots, clip, bgr;
    float clip_flow;
    double wheel[VIZ_NCOLS * 3];                   // make_colorwheel() / 255.0
};

// np.clip(x, 0, clip_flow) (upstream clips to [0, clip_flow], not to [-clip_flow, clip_flow])
__device__ __forceinline__ float viz_clip(const VizDev &a, float x) { return a.clip ? fminf(fmaxf(x, 0.0f), a.clip_flow) : x; }

__global__ __launch_bounds__(VIZ_THREADS) void k_flow_rad_max(const VizDev a)
{
    __shared__ float sM[VIZ_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned n = blockIdx.y;
    const float *pu = a.flow + (size_t)n * 2 * a.HW, *pv = pu + a.HW;
    float m = 0.0f;
    // i < HW < 2^30 and the stride is at most VIZ_MAX_SLOTS * VIZ_THREADS = 2^16, so the last increment cannot wrap
    for (unsigned i = blockIdx.x * VIZ_THREADS + threadIdx.x; i < a.HW; i += gridDim.x * VIZ_THREADS) {
        const float u = viz_clip(a, pu[i]), v = viz_clip(a, pv[i]);
        m = fmaxf(m, sqrtf(u * u + v * v));
    }
    m = mpf_wave_max(m);
    if (lane == 0) sM[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) a.slots[(size_t)n * gridDim.x + blockIdx.x] = fmaxf(fmaxf(sM[0], sM[1]), fmaxf(sM[2], sM[3]));
}

__device__ __forceinline__ unsigned viz_u8(double t) { return t >= 0.0 ? (t <= 255.0 ? (unsigned)t : 255u) : 0u; }      // NaN: 0

// one pixel's colour as c0 | c1 << 8 | c2 << 16 in output channel order; u, v: the flow over rad_max + 1e-5
__device__ __forceinline__ unsigned viz_colour(const double *sW, float u, float v, int bgr)
{
    const float rad = sqrtf(u * u + v * v);
    const float a = atan2f(-v, -u) / 3.14159265358979323846f;
    const float fk = (a + 1.0f) / 2.0f * (float)(VIZ_NCOLS - 1);
    const float fl = floorf(fk);
    const int k0 = fl >= 0.0f ? (fl <= (float)(VIZ_NCOLS - 1) ? (int)fl : VIZ_NCOLS - 1) : 0;      // clamped; NaN: 0
    const int k1 = k0 + 1 == VIZ_NCOLS ? 0 : k0 + 1;
    const double f = (double)fk - (double)k0;
    unsigned px = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double col = (1.0 - f) * sW[k0 * 3 + c] + f * sW[k1 * 3 + c];
        col = rad <= 1.0f ? 1.0 - (double)rad * (1.0 - col) : col * 0.75;
        px |= viz_u8(floor(255.0 * col)) << (8 * (bgr ? 2 - c : c));
    }
    return px;
}

__global__ __launch_bounds__(VIZ_THREADS) void k_flow_colour(const VizDev a)
{
    __shared__ double sW[VIZ_NCOLS * 3];
    __shared__ float sD[VIZ_BLOCK_PX];                                    // the divisor of image n_first + k
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < VIZ_NCOLS * 3) sW[threadIdx.x] = a.wheel[threadIdx.x];
    const unsigned g0 = blockIdx.x * VIZ_BLOCK_PX;                        // total < 2^31 / 3: no wrap
    const unsigned g_last = min(g0 + VIZ_BLOCK_PX - 1, a.total - 1);
    const unsigned n_first = g0 / a.P, n_count = g_last / a.P - n_first + 1;     // at most VIZ_BLOCK_PX images (P >= 1)
    for (unsigned k = wave; k < n_count; k += VIZ_WAVES) {
        const float *slot = a.slots + (size_t)(n_first + k) * a.nslots;
        float m = 0.0f;
        for (int b = lane; b < a.nslots; b += 64) m = fmaxf(m, slot[b]);
        m = mpf_wave_max(m);
        if (lane == 0) sD[k] = m + 1e-5f;
    }
    __syncthreads();
    const unsigned g = g0 + threadIdx.x * VIZ_PX;
    if (g >= a.total) return;
    const unsigned top = a.image ? a.HW : 0u;                             // pixels of the frame above the colours
    unsigned px[VIZ_PX];
#pragma unroll
    for (int e = 0; e < VIZ_PX; ++e) {
        px[e] = 0;
        if (g + e >= a.total) continue;
        const unsigned n = (g + e) / a.P, q = (g + e) - n * a.P;
        if (q < top) {                                                    // astype(np.uint8) of the frame: truncation
            const float *im = a.image + (size_t)n * 3 * a.HW + q;
#pragma unroll
            for (int c = 0; c < 3; ++c) px[e] |= viz_u8((double)truncf(im[(size_t)c * a.HW])) << (8 * (a.bgr ? 2 - c : c));
        } else {
            const float *pu = a.flow + (size_t)n * 2 * a.HW + (q - top);
            const float d = sD[n - n_first];
            px[e] = viz_colour(sW, viz_clip(a, pu[0]) / d, viz_clip(a, pu[a.HW]) / d, a.bgr);
        }
    }
    unsigned char *dst = a.out8 + (size_t)g * 3;
    if (g + VIZ_PX <= a.total) {
        unsigned *w = (unsigned *)dst;                                    // 12 * lane bytes past a 4-byte aligned base
        w[0] = px[0] | px[1] << 24;
        w[1] = px[1] >> 8 | px[2] << 16;
        w[2] = px[2] >> 16 | px[3] << 8;
    } else {
        for (unsigned e = 0; g + e < a.total; ++e)
            dst[3 * e] = (unsigned char)px[e], dst[3 * e + 1] = (unsigned char)(px[e] >> 8), dst[3 * e + 2] = (unsigned char)(px[e] >> 16);
    }
}

// astype(np.uint16) of an in-range value: toward zero; outside 0..65535 clamped, NaN: 0
__device__ __forceinline__ unsigned viz_u16(float x) { return x >= 0.0f ? (x < 65536.0f ? (unsigned)x : 65535u) : 0u; }

__global__ __launch_bounds__(VIZ_THREADS) void k_flow_encode_kitti(const VizDev a)
{
    const unsigned g = (blockIdx.x * VIZ_THREADS + threadIdx.x) * 2;      // total < 2^31 / 6: no wrap
    if (g >= a.total) return;
    unsigned code[2][3];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        code[e][0] = code[e][1] = code[e][2] = 0;
        if (g + e >= a.total) continue;
        const unsigned n = (g + e) / a.HW, q = (g + e) - n * a.HW;
        const float *pu = a.flow + (size_t)n * 2 * a.HW + q;
        code[e][0] = viz_u16(64.0f * pu[0] + 32768.0f);
        code[e][1] = viz_u16(64.0f * pu[a.HW] + 32768.0f);
        code[e][2] = a.valid ? (a.valid[(size_t)n * a.HW + q] >= 0.5f ? 1u : 0u) : 1u;
    }
    unsigned short *dst = a.out16 + (size_t)g * 3;
    if (g + 2 <= a.total) {
        unsigned *w = (unsigned *)dst;                                    // 12 * lane bytes past a 4-byte aligned base
        w[0] = code[0][0] | code[0][1] << 16;
        w[1] = code[0][2] | code[1][0] << 16;
        w[2] = code[1][1] | code[1][2] << 16;
    } else {
        dst[0] = (unsigned short)code[0][0], dst[1] = (unsigned short)code[0][1], dst[2] = (unsigned short)code[0][2];
    }
}

// make_colorwheel() / 255.0, as flow_uv_to_colors divides it: 55 rows of (R, G, B)
static void viz_wheel(double *wheel)
{
    const int RY = 15, YG = 6, GC = 4, CB = 11, BM = 13, MR = 6;
    double (*w)[3] = (double (*)[3])wheel;
    for (int i = 0; i < VIZ_NCOLS * 3; ++i) wheel[i] = 0.0;
    int col = 0;
    for (int i = 0; i < RY; ++i) w[col + i][0] = 255.0, w[col + i][1] = floor(255.0 * i / RY);
    col += RY;
    for (int i = 0; i < YG; ++i) w[col + i][0] = 255.0 - floor(255.0 * i / YG), w[col + i][1] = 255.0;
    col += YG;
    for (int i = 0; i < GC; ++i) w[col + i][1] = 255.0, w[col + i][2] = floor(255.0 * i / GC);
    col += GC;
    for (int i = 0; i < CB; ++i) w[col + i][1] = 255.0 - floor(255.0 * i / CB), w[col + i][2] = 255.0;
    col += CB;
    for (int i = 0; i < BM; ++i) w[col + i][2] = 255.0, w[col + i][0] = floor(255.0 * i / BM);
    col += BM;
    for (int i = 0; i < MR; ++i) w[col + i][2] = 255.0 - floor(255.0 * i / MR), w[col + i][0] = 255.0;
    for (int i = 0; i < VIZ_NCOLS * 3; ++i) wheel[i] /= 255.0;
}

// N, H, W >= 1, N <= 65535 and the largest output, [N,2H,W,3] bytes / [N,H,W,3] u16, below 2^31 bytes; the blocks per image of k_flow_rad_max
static int viz_shape(int N, int H, int W, const char *who, int64_t &nslots)
{
    MPF_REQUIRE(N >= 1 && H >= 1 && W >= 1, "%s: bad shape N, H, W = %d, %d, %d", who, N, H, W);
    const int64_t lim = (int64_t)1 << 31;
    const int64_t hw = (int64_t)H * W;
    MPF_REQUIRE(hw < lim / 6 && (int64_t)N * hw < lim / 6, "%s: the output must hold fewer than 2^31 bytes (N, H, W = %d, %d, %d)", who, N, H, W);
    MPF_REQUIRE(N <= 65535, "%s: bad shape: at most 65535 frames per call (got N = %d)", who, N);
    nslots = (hw + VIZ_THREADS - 1) / VIZ_THREADS;
    if (nslots > VIZ_MAX_SLOTS) nslots = VIZ_MAX_SLOTS;
    return 0;
}

extern "C" size_t mpf_flow_to_image_workspace(int N, int H, int W)
{
    int64_t nslots;
    if (viz_shape(N, H, W, "mpf_flow_to_image_workspace", nslots)) return 0;
    return (size_t)N * nslots * sizeof(float);
}

extern "C" int mpf_flow_to_image(const MpfFlowVizArgs *a, void *stream)
{
    const char *who = "mpf_flow_to_image";
    MPF_REQUIRE(a, "%s: null argument block", who);
    int64_t nslots;
    const int rc = viz_shape(a->N, a->H, a->W, who, nslots);
    if (rc) return rc;
    MPF_REQUIRE(a->flow && a->out, "%s: null pointer (flow or out)", who);
    MPF_REQUIRE((((uintptr_t)a->out) & 3) == 0, "%s: out must be 4-byte aligned", who);
    MPF_REQUIRE(!a->clip || a->clip_flow == a->clip_flow, "%s: clip_flow must not be NaN", who);
    const size_t need = (size_t)a->N * nslots * sizeof(float);
    MPF_REQUIRE(a->workspace, "%s: null pointer (workspace)", who);
    MPF_REQUIRE((((uintptr_t)a->workspace) & 3) == 0, "%s: workspace must be 4-byte aligned", who);
    MPF_REQUIRE(a->workspace_bytes >= need, "%s: workspace holds %zu bytes, %zu needed (mpf_flow_to_image_workspace)", who, a->workspace_bytes, need);
    VizDev d = VizDev{};
    d.flow = a->flow, d.image = a->image, d.slots = (float *)a->workspace, d.out8 = (unsigned char *)a->out;
    d.HW = (unsigned)(a->H * a->W), d.P = a->image ? 2 * d.HW : d.HW, d.total = (unsigned)a->N * d.P;
    d.nslots = (int)nslots, d.clip = a->clip != 0, d.clip_flow = a->clip_flow, d.bgr = a->convert_to_bgr != 0;
    viz_wheel(d.wheel);
    hipLaunchKernelGGL(k_flow_rad_max, dim3((unsigned)nslots, (unsigned)a->N), dim3(VIZ_THREADS), 0, (hipStream_t)stream, d);
    const int st = mpf_launch_status("k_flow_rad_max");
    if (st) return st;
    hipLaunchKernelGGL(k_flow_colour, dim3((d.total + VIZ_BLOCK_PX - 1) / VIZ_BLOCK_PX), dim3(VIZ_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_flow_colour");
}

extern "C" int mpf_flow_encode_kitti(const MpfFlowVizArgs *a, void *stream)
{
    const char *who = "mpf_flow_encode_kitti";
    MPF_REQUIRE(a, "%s: null argument block", who);
    int64_t nslots;
    const int rc = viz_shape(a->N, a->H, a->W, who, nslots);
    if (rc) return rc;
    MPF_REQUIRE(a->flow && a->out, "%s: null pointer (flow or out)", who);
    MPF_REQUIRE((((uintptr_t)a->out) & 3) == 0, "%s: out must be 4-byte aligned", who);
    VizDev d = VizDev{};
    d.flow = a->flow, d.valid = a->valid, d.out16 = (unsigned short *)a->out;
    d.HW = (unsigned)(a->H * a->W), d.P = d.HW, d.total = (unsigned)a->N * d.HW;
    const unsigned lanes = (d.total + 1) / 2;
    hipLaunchKernelGGL(k_flow_encode_kitti, dim3((lanes + VIZ_THREADS - 1) / VIZ_THREADS), dim3(VIZ_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_flow_encode_kitti");
}
