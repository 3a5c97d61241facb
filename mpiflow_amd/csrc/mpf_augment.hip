// mpf_augment.hip - the training side of a pair: RAFT's FlowAugmentor.spatial_transform (RAFT/core/utils/augmentor.py:67-109) and the
// tensor packing of its dataset (RAFT/core/datasets.py:85-90), fused, for a batch of rendered pairs that never leave the GPU
// (mpiflow_amd/online.py).
//
// Per output pixel (b, y, x) of a crop h x w (include/mpiflow_hip.h, MpfAugmentSample):
//   yy = y0 + y, xx = x0 + x;  flip_h: xx = Wr-1-xx;  flip_v: yy = Hr-1-yy          (resize, then flip, then crop - RAFT's order)
//   resize == 0: (yy, xx) is the source pixel.  resize == 1: cv2 INTER_LINEAR's coordinate map per axis,
//     f = (float)((xx + 0.5) * (1.0 / scale) - 0.5), s = floor(f), a = f - s;  s < 0 -> (0, 0);  s >= n-1 -> (n-1, 0);  s1 = min(s+1, n-1)
//     and fp32 interpolation, horizontal first: r_i = p_i0*(1-ax) + p_i1*ax, out = r_0*(1-ay) + r_1*ay, every operation rounded on its own
//     (the library builds with -ffp-contract=off).
//   image1/image2: rintf, clamp 0..255, as float, RGB (the inputs are BGR).  cv2's u8 path uses 11-bit fixed-point weights and can differ by one
//     LSB: an unpinned deviation (no OpenCV on any box this was written on).
//   flow: u' = (float)((double)u * scale_x), v' = (float)((double)v * scale_y) when resized (RAFT: `flow * [sx, sy]` in float64, then .float());
//     -u' under flip_h, -v' under flip_v.  valid = |u'| < 1000 && |v'| < 1000.
//
// Memory-bound and small: per output pixel it writes 36 bytes (2 x 3 image floats, 2 flow floats, 1 valid float) and reads, at scale ~1,
// about 14 bytes of source (3 + 3 u8 image bytes, 8 flow bytes; the four taps of neighbouring pixels share cache lines).  At 288 x 960 and
// B = 8 that is 80 MB written / ~31 MB read per launch: ~14 us at 8 TB/s.  One workgroup = one 256-pixel segment of one output row of one
// sample; every sample of the launch is in one grid (blockIdx.z).  The sources are read through buffer descriptors sized to the frame, so a
// tap can never reach past it.
#include "mpf_augment_common.h"

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_MAX_PER_LAUNCH = 32;          // samples per launch: the per-sample blocks travel as kernel arguments (32 x 88 B)

struct AugDev {                                  // MpfAugmentSample as the kernel reads it: 1 / scale computed on the host, in double
    const uint8_t *src, *dst;
    const float *flow;
    double scale_x, scale_y, inv_x, inv_y;
    int resize, Hr, Wr, flip_h, flip_v, y0, x0, pad;
};

struct AugBatch {
    AugDev s[AUG_MAX_PER_LAUNCH];
};

__global__ __launch_bounds__(AUG_THREADS) void k_augment_pairs(const AugBatch batch, int H, int W, int h, int w, float *__restrict__ image1,
                                                               float *__restrict__ image2, float *__restrict__ flow_out, float *__restrict__ valid)
{
    const int b = blockIdx.z, y = blockIdx.y, x = blockIdx.x * AUG_THREADS + threadIdx.x;
    const AugDev &s = batch.s[b];
    const unsigned img_bytes = (unsigned)H * (unsigned)W * 3u, flo_bytes = (unsigned)H * (unsigned)W * 8u;
    const __amdgpu_buffer_rsrc_t rs_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(s.src), 0, img_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_dst = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(s.dst), 0, img_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_flo = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(s.flow), 0, flo_bytes, 0x00020000);
    if (x >= w) return;
    int yy = s.y0 + y, xx = s.x0 + x;
    if (s.flip_h) xx = s.Wr - 1 - xx;
    if (s.flip_v) yy = s.Hr - 1 - yy;

    float im1[3], im2[3], u, v;
    if (!s.resize) {
        const unsigned p = (unsigned)yy * (unsigned)W + (unsigned)xx;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            im1[c] = ld_u8(rs_src, 3u * p + c);
            im2[c] = ld_u8(rs_dst, 3u * p + c);
        }
        const float2 f = ld_f2(rs_flo, 8u * p);
        u = f.x;
        v = f.y;
    } else {
        const Tap tx = lin_tap(xx, W, s.inv_x), ty = lin_tap(yy, H, s.inv_y);
        const unsigned p00 = (unsigned)ty.i0 * W + tx.i0, p01 = (unsigned)ty.i0 * W + tx.i1, p10 = (unsigned)ty.i1 * W + tx.i0,
                       p11 = (unsigned)ty.i1 * W + tx.i1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            im1[c] = to_pixel(lerp2(ld_u8(rs_src, 3u * p00 + c), ld_u8(rs_src, 3u * p01 + c), ld_u8(rs_src, 3u * p10 + c), ld_u8(rs_src, 3u * p11 + c), tx.a, ty.a));
            im2[c] = to_pixel(lerp2(ld_u8(rs_dst, 3u * p00 + c), ld_u8(rs_dst, 3u * p01 + c), ld_u8(rs_dst, 3u * p10 + c), ld_u8(rs_dst, 3u * p11 + c), tx.a, ty.a));
        }
        const float2 f00 = ld_f2(rs_flo, 8u * p00), f01 = ld_f2(rs_flo, 8u * p01), f10 = ld_f2(rs_flo, 8u * p10), f11 = ld_f2(rs_flo, 8u * p11);
        u = (float)((double)lerp2(f00.x, f01.x, f10.x, f11.x, tx.a, ty.a) * s.scale_x);
        v = (float)((double)lerp2(f00.y, f01.y, f10.y, f11.y, tx.a, ty.a) * s.scale_y);
    }
    if (s.flip_h) u = -u;
    if (s.flip_v) v = -v;

    const int64_t hw = (int64_t)h * w, o = (int64_t)y * w + x;
    float *i1 = image1 + (int64_t)b * 3 * hw + o, *i2 = image2 + (int64_t)b * 3 * hw + o;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                 // BGR -> RGB
        i1[c * hw] = im1[2 - c];
        i2[c * hw] = im2[2 - c];
    }
    flow_out[(int64_t)b * 2 * hw + o] = u;
    flow_out[(int64_t)b * 2 * hw + hw + o] = v;
    valid[(int64_t)b * hw + o] = (fabsf(u) < 1000.0f && fabsf(v) < 1000.0f) ? 1.0f : 0.0f;
}

}  // namespace

extern "C" int mpf_augment_pairs(const MpfAugmentSample *s, int B, int H, int W, int h, int w, float *d_image1, float *d_image2, float *d_flow,
                                 float *d_valid, void *stream)
{
    MPF_REQUIRE(s && d_image1 && d_image2 && d_flow && d_valid, "mpf_augment_pairs: null pointer");
    MPF_REQUIRE(B >= 1, "mpf_augment_pairs: B must be >= 1 (got %d)", B);
    MPF_REQUIRE(H >= 1 && W >= 1 && h >= 1 && w >= 1 && h <= 65535 && (int64_t)H * W * 8 < ((int64_t)1 << 31), "mpf_augment_pairs: bad shape");
    MPF_REQUIRE((int64_t)B * 3 * h * w < ((int64_t)1 << 40), "mpf_augment_pairs: batch too large");
    for (int b = 0; b < B; ++b) {
        const MpfAugmentSample &a = s[b];
        MPF_REQUIRE(a.src && a.dst && a.flow, "mpf_augment_pairs: null pointer in sample %d", b);
        MPF_REQUIRE(a.resize == 0 || a.resize == 1, "mpf_augment_pairs: sample %d: resize must be 0 or 1", b);
        MPF_REQUIRE((a.flip_h == 0 || a.flip_h == 1) && (a.flip_v == 0 || a.flip_v == 1), "mpf_augment_pairs: sample %d: flips must be 0 or 1", b);
        if (a.resize == 0) {
            MPF_REQUIRE(a.Hr == H && a.Wr == W, "mpf_augment_pairs: sample %d: resize == 0 needs Hr == H and Wr == W (got %d x %d for %d x %d)", b,
                        a.Hr, a.Wr, H, W);
        } else {
            MPF_REQUIRE(a.scale_x > 0.0 && a.scale_y > 0.0 && a.scale_x < 1e4 && a.scale_y < 1e4, "mpf_augment_pairs: sample %d: bad scale", b);
            MPF_REQUIRE(a.Hr >= 1 && a.Wr >= 1 && a.Hr <= (1 << 20) && a.Wr <= (1 << 20), "mpf_augment_pairs: sample %d: bad resized size", b);
        }
        MPF_REQUIRE(a.y0 >= 0 && a.x0 >= 0 && (int64_t)a.y0 + h <= a.Hr && (int64_t)a.x0 + w <= a.Wr,
                    "mpf_augment_pairs: sample %d: crop %d x %d at (%d, %d) outside the resized frame %d x %d", b, h, w, a.y0, a.x0, a.Hr, a.Wr);
    }
    const int64_t hw = (int64_t)h * w;
    for (int b0 = 0; b0 < B; b0 += AUG_MAX_PER_LAUNCH) {
        const int nb = B - b0 < AUG_MAX_PER_LAUNCH ? B - b0 : AUG_MAX_PER_LAUNCH;
        AugBatch batch = {};
        for (int i = 0; i < nb; ++i) {
            const MpfAugmentSample &a = s[b0 + i];
            batch.s[i] = AugDev{a.src, a.dst, a.flow, a.scale_x, a.scale_y, 1.0 / a.scale_x, 1.0 / a.scale_y, a.resize, a.Hr, a.Wr, a.flip_h, a.flip_v,
                                a.y0, a.x0, 0};
        }
        hipLaunchKernelGGL(k_augment_pairs, dim3((unsigned)((w + AUG_THREADS - 1) / AUG_THREADS), (unsigned)h, (unsigned)nb), dim3(AUG_THREADS), 0,
                           (hipStream_t)stream, batch, H, W, h, w, d_image1 + b0 * 3 * hw, d_image2 + b0 * 3 * hw, d_flow + b0 * 2 * hw, d_valid + b0 * hw);
        const int rc = mpf_launch_status("k_augment_pairs");
        if (rc) return rc;
    }
    return 0;
}
