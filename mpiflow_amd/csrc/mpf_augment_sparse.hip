// mpf_augment_sparse.hip - the sparse path of RAFT's loader, the one its KITTI stage trains through: KITTI's 16-bit flow code
// (writeFlowKITTI -> readFlowKITTI, core/utils/frame_utils.py:102-120), SparseFlowAugmentor.spatial_transform (core/utils/augmentor.py:194-232)
// with resize_sparse_flow_map's nearest-pixel scatter (:160-192), and the dataset's packing (core/datasets.py:85-90), fused, for a batch of
// rendered pairs that never leave the GPU (mpiflow_amd/online.py, sparse=).
//
// Per output pixel (b, y, x) of a crop h x w (include/mpiflow_hip.h, MpfSparseAugmentSample):
//   Y = y0 + y, X = x0 + x;  flip_h: X = Wr-1-X                                        (resize, then flip, then crop - RAFT's order)
//   images: exactly mpf_augment_pairs' path (mpf_augment.hip): the source pixel (resize 0) or cv2 INTER_LINEAR by 1 / scale (resize 1), rintf,
//     clamp 0..255, as float, RGB.  cv2's own u8 resize rounds 11-bit fixed-point weights and may differ by one LSB: unpinned.
//   source validity and quantization, per source pixel p: valid[p] != 0 (valid == NULL: every pixel);  quantize: t = 64.0f*u + 32768.0f in fp32,
//     each operation rounded on its own (-ffp-contract=off), q = trunc(t), u_q = (float)(q - 32768) / 64.0f, the same for v, and the pixel
//     is invalid unless -1 < t < 65536 for both components (the reference's uint16 cast is undefined there: this rule is this library's).
//   flow, resize 0: (u_q, v_q) of the source pixel (Y, X) where it is valid, else 0;  valid = its validity.
//   flow, resize 1: the gather form of the scatter flow_img[round(ys*fy), round(xs*fx)] = flow[ys, xs] * (fx, fy) over the valid sources in
//     raster order.  X < 1 or Y < 1: 0, valid 0 (the scatter keeps xx > 0, yy > 0).  Else candidate rows {ys : rint((double)ys*scale_y) == Y},
//     candidate columns {xs : rint((double)xs*scale_x) == X} (rint = half to even, as np.round on the float64 product); the largest ys that
//     has a valid candidate xs, then the largest such xs, is numpy's last writer: u' = (float)((double)u_q * scale_x),
//     v' = (float)((double)v_q * scale_y), valid 1.  No valid candidate: 0, 0, valid 0 (an upscale's hole).  A candidate lies in
//     [floor((X-0.5)/s)-1, ceil((X+0.5)/s)+1] ∩ [0, n-1]: at RAFT's KITTI scales (~0.75..1.32) that is 3-4 indices, at most 2 of which match.
//   flip_h: u' = -u' (a hole's 0 becomes -0.0, as RAFT's `flow * [-1.0, 1.0]`);  valid is mirrored with the map, not negated.
//
// Memory-bound like k_augment_pairs: it writes the same 36 bytes per output pixel and reads the same image taps; the flow costs one 8-byte
// read of the winning candidate (and the valid bytes of the candidates tried) instead of four bilinear taps.  One workgroup = one 256-pixel
// segment of one output row of one sample; every sample of the launch is in one grid (blockIdx.z).  All sources are read through buffer
// descriptors sized to the frame, so no tap or candidate can reach past one.
#include "mpf_augment_common.h"

namespace {

constexpr int SPA_THREADS = 256;
constexpr int SPA_MAX_PER_LAUNCH = 32;          // samples per launch: the per-sample blocks travel as kernel arguments (32 x 96 B)

struct SpaDev {                                  // MpfSparseAugmentSample as the kernel reads it: 1 / scale computed on the host, in double
    const uint8_t *src, *dst, *valid;
    const float *flow;
    double scale_x, scale_y, inv_x, inv_y;
    int resize, quantize, Hr, Wr, flip_h, y0, x0, pad;
};

struct SpaBatch {
    SpaDev s[SPA_MAX_PER_LAUNCH];
};

// source pixel p after KITTI's code: false when invalid (valid byte 0, or outside the 16-bit code's range under quantize)
__device__ __forceinline__ bool source_flow(__amdgpu_buffer_rsrc_t rs_flo, __amdgpu_buffer_rsrc_t rs_val, bool has_valid, int quantize, unsigned p,
                                            float &u, float &v)
{
    if (has_valid && __builtin_amdgcn_raw_buffer_load_b8(rs_val, p, 0, 0) == 0) return false;
    const float2 f = ld_f2(rs_flo, 8u * p);
    if (!quantize) {
        u = f.x;
        v = f.y;
        return true;
    }
    const float tu = 64.0f * f.x + 32768.0f, tv = 64.0f * f.y + 32768.0f;
    if (!(tu > -1.0f && tu < 65536.0f && tv > -1.0f && tv < 65536.0f)) return false;      // NaN included
    u = (float)((int)tu - 32768) / 64.0f;
    v = (float)((int)tv - 32768) / 64.0f;
    return true;
}

// candidate source indices of target index d on an axis of n source pixels: [floor((d-0.5)/s)-1, ceil((d+0.5)/s)+1] ∩ [0, n-1]
__device__ __forceinline__ void candidates(int d, int n, double inv, int &lo, int &hi)
{
    lo = (int)fmax(0.0, floor(((double)d - 0.5) * inv) - 1.0);
    hi = (int)fmin((double)(n - 1), ceil(((double)d + 0.5) * inv) + 1.0);
}

__global__ __launch_bounds__(SPA_THREADS) void k_augment_sparse_pairs(const SpaBatch batch, int H, int W, int h, int w, float *__restrict__ image1,
                                                                      float *__restrict__ image2, float *__restrict__ flow_out,
                                                                      float *__restrict__ valid_out)
{
    const int b = blockIdx.z, y = blockIdx.y, x = blockIdx.x * SPA_THREADS + threadIdx.x;
    const SpaDev &s = batch.s[b];
    const unsigned npix = (unsigned)H * (unsigned)W, img_bytes = npix * 3u, flo_bytes = npix * 8u;
    const bool has_valid = s.valid != nullptr;
    const __amdgpu_buffer_rsrc_t rs_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(s.src), 0, img_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_dst = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(s.dst), 0, img_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_flo = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(s.flow), 0, flo_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_val = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(s.valid), 0, has_valid ? npix : 0u, 0x00020000);
    if (x >= w) return;
    const int Y = s.y0 + y;
    int X = s.x0 + x;
    if (s.flip_h) X = s.Wr - 1 - X;

    float im1[3], im2[3], u = 0.0f, v = 0.0f;
    bool ok = false;
    if (!s.resize) {
        const unsigned p = (unsigned)Y * (unsigned)W + (unsigned)X;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            im1[c] = ld_u8(rs_src, 3u * p + c);
            im2[c] = ld_u8(rs_dst, 3u * p + c);
        }
        ok = source_flow(rs_flo, rs_val, has_valid, s.quantize, p, u, v);
    } else {
        const Tap tx = lin_tap(X, W, s.inv_x), ty = lin_tap(Y, H, s.inv_y);
        const unsigned p00 = (unsigned)ty.i0 * W + tx.i0, p01 = (unsigned)ty.i0 * W + tx.i1, p10 = (unsigned)ty.i1 * W + tx.i0,
                       p11 = (unsigned)ty.i1 * W + tx.i1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            im1[c] = to_pixel(lerp2(ld_u8(rs_src, 3u * p00 + c), ld_u8(rs_src, 3u * p01 + c), ld_u8(rs_src, 3u * p10 + c), ld_u8(rs_src, 3u * p11 + c), tx.a, ty.a));
            im2[c] = to_pixel(lerp2(ld_u8(rs_dst, 3u * p00 + c), ld_u8(rs_dst, 3u * p01 + c), ld_u8(rs_dst, 3u * p10 + c), ld_u8(rs_dst, 3u * p11 + c), tx.a, ty.a));
        }
        if (X >= 1 && Y >= 1) {
            int ylo, yhi, xlo, xhi;
            candidates(Y, H, s.inv_y, ylo, yhi);
            candidates(X, W, s.inv_x, xlo, xhi);
            for (int ys = yhi; ys >= ylo && !ok; --ys) {                // raster order backwards: the first valid hit is the last writer
                if (rint((double)ys * s.scale_y) != (double)Y) continue;
                for (int xs = xhi; xs >= xlo; --xs) {
                    if (rint((double)xs * s.scale_x) != (double)X) continue;
                    if (source_flow(rs_flo, rs_val, has_valid, s.quantize, (unsigned)ys * (unsigned)W + (unsigned)xs, u, v)) {
                        ok = true;
                        break;
                    }
                }
            }
            if (ok) {
                u = (float)((double)u * s.scale_x);
                v = (float)((double)v * s.scale_y);
            }
        }
    }
    if (!ok) u = v = 0.0f;
    if (s.flip_h) u = -u;

    const int64_t hw = (int64_t)h * w, o = (int64_t)y * w + x;
    float *i1 = image1 + (int64_t)b * 3 * hw + o, *i2 = image2 + (int64_t)b * 3 * hw + o;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                 // BGR -> RGB
        i1[c * hw] = im1[2 - c];
        i2[c * hw] = im2[2 - c];
    }
    flow_out[(int64_t)b * 2 * hw + o] = u;
    flow_out[(int64_t)b * 2 * hw + hw + o] = v;
    valid_out[(int64_t)b * hw + o] = ok ? 1.0f : 0.0f;
}

}  // namespace

extern "C" int mpf_augment_sparse_pairs(const MpfSparseAugmentSample *s, int B, int H, int W, int h, int w, float *d_image1, float *d_image2,
                                        float *d_flow, float *d_valid, void *stream)
{
    MPF_REQUIRE(s && d_image1 && d_image2 && d_flow && d_valid, "mpf_augment_sparse_pairs: null pointer");
    MPF_REQUIRE(B >= 1, "mpf_augment_sparse_pairs: B must be >= 1 (got %d)", B);
    MPF_REQUIRE(H >= 1 && W >= 1 && h >= 1 && w >= 1 && h <= 65535 && (int64_t)H * W * 8 < ((int64_t)1 << 31), "mpf_augment_sparse_pairs: bad shape");
    MPF_REQUIRE((int64_t)B * 3 * h * w < ((int64_t)1 << 40), "mpf_augment_sparse_pairs: batch too large");
    for (int b = 0; b < B; ++b) {
        const MpfSparseAugmentSample &a = s[b];
        MPF_REQUIRE(a.src && a.dst && a.flow, "mpf_augment_sparse_pairs: null pointer in sample %d", b);
        MPF_REQUIRE(a.resize == 0 || a.resize == 1, "mpf_augment_sparse_pairs: sample %d: resize must be 0 or 1", b);
        MPF_REQUIRE(a.quantize == 0 || a.quantize == 1, "mpf_augment_sparse_pairs: sample %d: quantize must be 0 or 1", b);
        MPF_REQUIRE(a.flip_h == 0 || a.flip_h == 1, "mpf_augment_sparse_pairs: sample %d: flip_h must be 0 or 1", b);
        if (a.resize == 0) {
            MPF_REQUIRE(a.Hr == H && a.Wr == W, "mpf_augment_sparse_pairs: sample %d: resize == 0 needs Hr == H and Wr == W (got %d x %d for %d x %d)",
                        b, a.Hr, a.Wr, H, W);
        } else {
            MPF_REQUIRE(a.scale_x > 0.0 && a.scale_y > 0.0 && a.scale_x < 1e4 && a.scale_y < 1e4, "mpf_augment_sparse_pairs: sample %d: bad scale", b);
            MPF_REQUIRE(a.Hr >= 1 && a.Wr >= 1 && a.Hr <= (1 << 20) && a.Wr <= (1 << 20), "mpf_augment_sparse_pairs: sample %d: bad resized size", b);
        }
        MPF_REQUIRE(a.y0 >= 0 && a.x0 >= 0 && (int64_t)a.y0 + h <= a.Hr && (int64_t)a.x0 + w <= a.Wr,
                    "mpf_augment_sparse_pairs: sample %d: crop %d x %d at (%d, %d) outside the resized frame %d x %d", b, h, w, a.y0, a.x0, a.Hr, a.Wr);
    }
    const int64_t hw = (int64_t)h * w;
    for (int b0 = 0; b0 < B; b0 += SPA_MAX_PER_LAUNCH) {
        const int nb = B - b0 < SPA_MAX_PER_LAUNCH ? B - b0 : SPA_MAX_PER_LAUNCH;
        SpaBatch batch = {};
        for (int i = 0; i < nb; ++i) {
            const MpfSparseAugmentSample &a = s[b0 + i];
            batch.s[i] = SpaDev{a.src, a.dst, a.valid, a.flow, a.scale_x, a.scale_y, 1.0 / a.scale_x, 1.0 / a.scale_y, a.resize, a.quantize, a.Hr, a.Wr,
                                a.flip_h, a.y0, a.x0, 0};
        }
        hipLaunchKernelGGL(k_augment_sparse_pairs, dim3((unsigned)((w + SPA_THREADS - 1) / SPA_THREADS), (unsigned)h, (unsigned)nb), dim3(SPA_THREADS), 0,
                           (hipStream_t)stream, batch, H, W, h, w, d_image1 + b0 * 3 * hw, d_image2 + b0 * 3 * hw, d_flow + b0 * 2 * hw, d_valid + b0 * hw);
        const int rc = mpf_launch_status("k_augment_sparse_pairs");
        if (rc) return rc;
    }
    return 0;
}
