// mpf_photometric.hip - the photometric half of RAFT's FlowAugmentor: color_transform and eraser_transform
// (RAFT/core/utils/augmentor.py:36-65), which __call__ runs on the full-size u8 frames before spatial_transform (mpf_augment.hip).
//
// Per pair (include/mpiflow_hip.h, MpfPhotoSample): src = image 1, dst = image 2, u8 [H,W,3] BGR in memory, RGB semantics (RAFT reads its PNGs
// with PIL): r = byte 2, g = byte 1, b = byte 0.
//   Jitter: torchvision ColorJitter on a PIL RGB image, the ops of jitter.order[0 .. n_ops) in that order:
//     0 brightness f:  blend(0, x, f)
//     1 contrast f:    blend(m, x, f),  m = int(sumL / n + 0.5) in double, sumL = sum of L over the image AS IT STANDS before the contrast op
//     2 saturation f:  blend(L(x), x, f)
//     3 hue shift:     PIL's RGB -> HSV (Convert.c rgb2hsv), H' = (H + shift) & 255, PIL's HSV -> RGB (hsv2rgb); lossy even at shift 0
//     L(r,g,b) = (19595 r + 38470 g + 7471 b + 0x8000) >> 16;  blend(a, x, f): t = (float)a + f * (float)(x - a) in fp32 (no contraction),
//     0 if t <= 0, 255 if t >= 255, else (u8)t.  The HSV maths keep PIL's float / double mix operation by operation.
//     joint = 1 (RAFT's symmetric jitter of np.concatenate([img1, img2])): jitter[0] for both frames and one contrast mean over both
//     (n = 2 H W);  joint = 0: jitter[0] on src, jitter[1] on dst, each with its own mean (n = H W).
//   Eraser (after the jitter, on the jittered dst only): mean_c = sum_c // (H W) per channel, then the n_rect rectangles
//     [y0, y0+dy) x [x0, x0+dx), clipped at the frame edge as numpy slicing clips, are filled with it.
//
// Three passes, no host synchronisation: (a) k_photo_stats - sumL of the pre-contrast image of every frame whose chain holds contrast, the ops
// in front of contrast applied on the fly; (b) k_photo_apply - the chain, into the output frames, + the per-channel sums of the jittered dst of
// samples with rectangles; (c) k_photo_erase - the rectangles.  Every sum is an integer: per-wave shuffle, per-block LDS, one 64-bit vector
// atomicAdd per block into the workspace (zeroed by hipMemsetAsync on the stream), so results do not depend on the order blocks run in.
// Memory-bound and small: at 384 x 1280 and B = 8 a batch reads the frames once or twice and writes them once, ~50-70 MB.  The inputs are
// read through buffer descriptors sized to the frame.
#include "mpf_common.h"
#include "mpf_reduce.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int PH_THREADS = 256;
constexpr int PH_PPT = 8;                        // pixels per thread in (a) and (b): strided by PH_THREADS, so every load is coalesced
constexpr int PH_MAX_PER_LAUNCH = 32;            // samples per launch: the per-sample blocks travel as kernel arguments (32 x 88 B)
constexpr int PH_WS_WORDS = 8;                   // u64 per sample: sumL of src, sumL of dst, channel sums of the jittered dst (B, G, R), pad

enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3 };

struct PhotoDev {                                // MpfPhotoSample as (a) and (b) read it
    const uint8_t *in[2];
    uint8_t *out[2];
    float fac[2][3];                             // brightness, contrast, saturation
    int n_ops[2];
    int ops[2];                                  // op k in bits 2k .. 2k+1
    int hue[2];
    int joint, sums;                             // sums: accumulate the channel sums of the jittered dst (the sample has rectangles)
};

struct PhotoBatch {
    PhotoDev s[PH_MAX_PER_LAUNCH];
};

struct EraseDev {                                // the rectangles, clipped on the host
    uint8_t *dst;
    int n_rect;
    int rect[2][4];                              // x0, y0, dx, dy
};

struct EraseBatch {
    EraseDev s[PH_MAX_PER_LAUNCH];
};

__device__ __forceinline__ int clip8(int v) { return v <= 0 ? 0 : v >= 255 ? 255 : v; }

__device__ __forceinline__ int lum(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__device__ __forceinline__ int blend(int a, int x, float f)
{
    const float t = (float)a + f * (float)(x - a);
    return t <= 0.0f ? 0 : t >= 255.0f ? 255 : (int)t;
}

// PIL's RGB -> HSV -> RGB round trip with the hue channel shifted (Convert.c rgb2hsv_row / hsv2rgb), in its float / double mix
__device__ __forceinline__ void hue_shift(int &r, int &g, int &b, int shift)
{
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b)), v = maxc;
    int h = 0, s = 0;
    if (maxc != minc) {
        const float cr = (float)(maxc - minc);
        const float sf = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float hf;
        if (r == maxc) hf = bc - gc;
        else if (g == maxc) hf = (float)(2.0 + (double)rc - (double)bc);
        else hf = (float)(4.0 + (double)gc - (double)rc);
        const double x = (double)hf / 6.0 + 1.0;              // in [5/6, 11/6]: fmod(x, 1.0) is x - 1 (exact) from 1 on
        hf = (float)(x >= 1.0 ? x - 1.0 : x);
        h = clip8((int)((double)hf * 255.0));
        s = clip8((int)((double)sf * 255.0));
    }
    h = (h + shift) & 255;
    if (s == 0) {
        r = g = b = v;
        return;
    }
    const double h6 = (double)h * 6.0 / 255.0;
    const int i = (int)floor(h6);
    const float f = (float)(h6 - (double)i);
    const float fs = (float)((double)s / 255.0);
    const int p = clip8((int)round((double)v * (1.0 - (double)fs)));
    const int q = clip8((int)round((double)v * (1.0 - (double)(fs * f))));
    const int t = clip8((int)round((double)v * (1.0 - (double)fs * (1.0 - (double)f))));
    switch (i % 6) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

// ops k0 .. k1 of a chain on one pixel; m = the contrast mean (unused when the range holds no contrast op)
__device__ __forceinline__ void run_ops(int &r, int &g, int &b, const PhotoDev &s, int j, int k0, int k1, int m)
{
    for (int k = k0; k < k1; ++k) {
        const int op = (s.ops[j] >> (2 * k)) & 3;
        if (op == OP_BRIGHTNESS) {
            const float f = s.fac[j][0];
            r = blend(0, r, f); g = blend(0, g, f); b = blend(0, b, f);
        } else if (op == OP_CONTRAST) {
            const float f = s.fac[j][1];
            r = blend(m, r, f); g = blend(m, g, f); b = blend(m, b, f);
        } else if (op == OP_SATURATION) {
            const float f = s.fac[j][2];
            const int l = lum(r, g, b);
            r = blend(l, r, f); g = blend(l, g, f); b = blend(l, b, f);
        } else {
            hue_shift(r, g, b, s.hue[j]);
        }
    }
}

__device__ __forceinline__ int contrast_pos(const PhotoDev &s, int j)
{
    for (int k = 0; k < s.n_ops[j]; ++k)
        if (((s.ops[j] >> (2 * k)) & 3) == OP_CONTRAST) return k;
    return -1;
}

// block-wide sums of N per-thread values -> one 64-bit atomicAdd per value (threads 0 .. N-1)
template <int N>
__device__ __forceinline__ void block_add(unsigned (&v)[N], unsigned long long *dst)
{
    __shared__ unsigned part[PH_THREADS / 64][N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        v[c] = mpf_wave_sum(v[c]);
        if (lane == 0) part[wave][c] = v[c];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < PH_THREADS / 64; ++w) t += part[w][threadIdx.x];
        atomicAdd(dst + threadIdx.x, t);
    }
}

__device__ __forceinline__ int ld_u8(__amdgpu_buffer_rsrc_t rs, unsigned off) { return (int)__builtin_amdgcn_raw_buffer_load_b8(rs, off, 0, 0); }

// (a) blockIdx.z = 2 * sample + frame; frames whose chain holds no contrast op leave at once
__global__ __launch_bounds__(PH_THREADS) void k_photo_stats(const PhotoBatch batch, int H, int W, unsigned long long *__restrict__ ws)
{
    const int b = blockIdx.z >> 1, fr = blockIdx.z & 1;
    const PhotoDev &s = batch.s[b];
    const int j = s.joint ? 0 : fr;
    const int kc = contrast_pos(s, j);
    if (kc < 0) return;
    const unsigned npx = (unsigned)H * (unsigned)W;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(s.in[fr]), 0, npx * 3u, 0x00020000);
    unsigned acc[1] = {0};
    const unsigned base = blockIdx.x * (unsigned)(PH_THREADS * PH_PPT) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < PH_PPT; ++k) {
        const unsigned p = base + (unsigned)(k * PH_THREADS);
        if (p < npx) {
            int bb = ld_u8(rs, 3u * p), g = ld_u8(rs, 3u * p + 1u), r = ld_u8(rs, 3u * p + 2u);
            run_ops(r, g, bb, s, j, 0, kc, 0);
            acc[0] += (unsigned)lum(r, g, bb);
        }
    }
    block_add<1>(acc, ws + (size_t)b * PH_WS_WORDS + fr);
}

// (b) the chain into the output frames; + the channel sums of the jittered dst
__global__ __launch_bounds__(PH_THREADS) void k_photo_apply(const PhotoBatch batch, int H, int W, unsigned long long *__restrict__ ws)
{
    const int b = blockIdx.z >> 1, fr = blockIdx.z & 1;
    const PhotoDev &s = batch.s[b];
    const int j = s.joint ? 0 : fr;
    const unsigned npx = (unsigned)H * (unsigned)W;
    const unsigned long long *w = ws + (size_t)b * PH_WS_WORDS;
    int m = 0;
    if (contrast_pos(s, j) >= 0) {
        const unsigned long long sum = s.joint ? w[0] + w[1] : w[fr];
        const double n = s.joint ? 2.0 * (double)npx : (double)npx;
        m = (int)((double)sum / n + 0.5);
    }
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(s.in[fr]), 0, npx * 3u, 0x00020000);
    uint8_t *out = s.out[fr];
    unsigned acc[3] = {0, 0, 0};
    const unsigned base = blockIdx.x * (unsigned)(PH_THREADS * PH_PPT) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < PH_PPT; ++k) {
        const unsigned p = base + (unsigned)(k * PH_THREADS);
        if (p < npx) {
            int bb = ld_u8(rs, 3u * p), g = ld_u8(rs, 3u * p + 1u), r = ld_u8(rs, 3u * p + 2u);
            run_ops(r, g, bb, s, j, 0, s.n_ops[j], m);
            out[3u * p] = (uint8_t)bb;
            out[3u * p + 1u] = (uint8_t)g;
            out[3u * p + 2u] = (uint8_t)r;
            acc[0] += (unsigned)bb;
            acc[1] += (unsigned)g;
            acc[2] += (unsigned)r;
        }
    }
    if (fr == 1 && s.sums) block_add<3>(acc, ws + (size_t)b * PH_WS_WORDS + 2);
}

// (c) blockIdx.z = 2 * sample + rectangle; (x, y) inside the clipped rectangle
__global__ __launch_bounds__(PH_THREADS) void k_photo_erase(const EraseBatch batch, int H, int W, const unsigned long long *__restrict__ ws)
{
    const int b = blockIdx.z >> 1, k = blockIdx.z & 1;
    const EraseDev &s = batch.s[b];
    if (k >= s.n_rect) return;
    const int x = blockIdx.x * PH_THREADS + threadIdx.x, y = blockIdx.y;
    if (x >= s.rect[k][2] || y >= s.rect[k][3]) return;
    const unsigned long long *w = ws + (size_t)b * PH_WS_WORDS + 2;
    const unsigned long long n = (unsigned long long)H * (unsigned long long)W;
    uint8_t *o = s.dst + 3 * ((size_t)(s.rect[k][1] + y) * (size_t)W + (size_t)(s.rect[k][0] + x));
    o[0] = (uint8_t)(w[0] / n);
    o[1] = (uint8_t)(w[1] / n);
    o[2] = (uint8_t)(w[2] / n);
}

}  // namespace

extern "C" size_t mpf_photometric_workspace(int B) { return B < 1 ? 0 : (size_t)B * PH_WS_WORDS * sizeof(unsigned long long); }

extern "C" int mpf_photometric_pairs(const MpfPhotoSample *s, int B, int H, int W, void *d_workspace, size_t workspace_bytes, void *stream)
{
    MPF_REQUIRE(s && d_workspace, "mpf_photometric_pairs: null pointer");
    MPF_REQUIRE(B >= 1, "mpf_photometric_pairs: B must be >= 1 (got %d)", B);
    MPF_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W * 3 < ((int64_t)1 << 31) && H <= 65535, "mpf_photometric_pairs: bad shape");
    MPF_REQUIRE(workspace_bytes >= mpf_photometric_workspace(B), "mpf_photometric_pairs: workspace of %zu bytes, %zu needed", workspace_bytes,
                mpf_photometric_workspace(B));
    MPF_REQUIRE((((uintptr_t)d_workspace) & 7) == 0, "mpf_photometric_pairs: workspace not 8-byte aligned");
    int any_contrast = 0, max_dx = 1, max_dy = 1;
    for (int b = 0; b < B; ++b) {
        const MpfPhotoSample &a = s[b];
        MPF_REQUIRE(a.src && a.dst && a.src_out && a.dst_out, "mpf_photometric_pairs: null pointer in sample %d", b);
        MPF_REQUIRE(a.joint == 0 || a.joint == 1, "mpf_photometric_pairs: sample %d: joint must be 0 or 1", b);
        for (int j = 0; j < 2; ++j) {
            const MpfPhotoJitter &t = a.jitter[j];
            MPF_REQUIRE(t.n_ops >= 0 && t.n_ops <= 4, "mpf_photometric_pairs: sample %d: jitter %d: n_ops must be 0..4", b, j);
            int seen = 0;
            for (int k = 0; k < t.n_ops; ++k) {
                MPF_REQUIRE(t.order[k] >= 0 && t.order[k] <= 3 && !(seen & (1 << t.order[k])),
                            "mpf_photometric_pairs: sample %d: jitter %d: op order must hold distinct values in 0..3", b, j);
                seen |= 1 << t.order[k];
            }
            if (seen & (1 << OP_CONTRAST) && (j == 0 || !a.joint)) any_contrast = 1;
            const float f[3] = {t.brightness, t.contrast, t.saturation};
            for (int c = 0; c < 3; ++c)
                MPF_REQUIRE(std::isfinite(f[c]) && f[c] >= 0.0f, "mpf_photometric_pairs: sample %d: jitter %d: factors must be finite and >= 0", b, j);
            MPF_REQUIRE(t.hue_shift >= -128 && t.hue_shift <= 127, "mpf_photometric_pairs: sample %d: jitter %d: hue shift outside -128..127", b, j);
        }
        MPF_REQUIRE(a.n_rect >= 0 && a.n_rect <= 2, "mpf_photometric_pairs: sample %d: n_rect must be 0..2", b);
        for (int k = 0; k < a.n_rect; ++k) {
            const int *r = a.rect[k];
            MPF_REQUIRE(r[0] >= 0 && r[0] < W && r[1] >= 0 && r[1] < H && r[2] >= 1 && r[3] >= 1,
                        "mpf_photometric_pairs: sample %d: rectangle %d: origin outside the frame or extent < 1", b, k);
            max_dx = std::max(max_dx, std::min(r[2], W - r[0]));               // the extents clipped at the frame edge
            max_dy = std::max(max_dy, std::min(r[3], H - r[1]));
        }
    }
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *ws = (unsigned long long *)d_workspace;
    MPF_HIP(hipMemsetAsync(ws, 0, mpf_photometric_workspace(B), st));
    const unsigned npx = (unsigned)H * (unsigned)W;
    const unsigned gx = (npx + PH_THREADS * PH_PPT - 1) / (PH_THREADS * PH_PPT);
    for (int b0 = 0; b0 < B; b0 += PH_MAX_PER_LAUNCH) {
        const int nb = B - b0 < PH_MAX_PER_LAUNCH ? B - b0 : PH_MAX_PER_LAUNCH;
        PhotoBatch batch = {};
        EraseBatch erase = {};
        int any_rect = 0;
        for (int i = 0; i < nb; ++i) {
            const MpfPhotoSample &a = s[b0 + i];
            PhotoDev &d = batch.s[i];
            d.in[0] = a.src;
            d.in[1] = a.dst;
            d.out[0] = a.src_out;
            d.out[1] = a.dst_out;
            for (int j = 0; j < 2; ++j) {
                const MpfPhotoJitter &t = a.jitter[j];
                d.fac[j][0] = t.brightness;
                d.fac[j][1] = t.contrast;
                d.fac[j][2] = t.saturation;
                d.n_ops[j] = t.n_ops;
                for (int k = 0; k < t.n_ops; ++k) d.ops[j] |= t.order[k] << (2 * k);
                d.hue[j] = t.hue_shift;
            }
            d.joint = a.joint;
            d.sums = a.n_rect > 0;
            EraseDev &e = erase.s[i];
            e.dst = a.dst_out;
            e.n_rect = a.n_rect;
            for (int k = 0; k < a.n_rect; ++k) {
                const int *r = a.rect[k];
                e.rect[k][0] = r[0];
                e.rect[k][1] = r[1];
                e.rect[k][2] = std::min(r[2], W - r[0]);
                e.rect[k][3] = std::min(r[3], H - r[1]);
            }
            any_rect |= a.n_rect > 0;
        }
        unsigned long long *w = ws + (size_t)b0 * PH_WS_WORDS;
        if (any_contrast) {
            hipLaunchKernelGGL(k_photo_stats, dim3(gx, 1, (unsigned)(2 * nb)), dim3(PH_THREADS), 0, st, batch, H, W, w);
            const int rc = mpf_launch_status("k_photo_stats");
            if (rc) return rc;
        }
        hipLaunchKernelGGL(k_photo_apply, dim3(gx, 1, (unsigned)(2 * nb)), dim3(PH_THREADS), 0, st, batch, H, W, w);
        int rc = mpf_launch_status("k_photo_apply");
        if (rc) return rc;
        if (any_rect) {
            hipLaunchKernelGGL(k_photo_erase, dim3((unsigned)((max_dx + PH_THREADS - 1) / PH_THREADS), (unsigned)max_dy, (unsigned)(2 * nb)),
                               dim3(PH_THREADS), 0, st, erase, H, W, (const unsigned long long *)w);
            rc = mpf_launch_status("k_photo_erase");
            if (rc) return rc;
        }
    }
    return 0;
}
