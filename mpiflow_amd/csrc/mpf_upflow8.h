// mpf_upflow8.h - the coordinate arithmetic of RAFT's upflow8 (8 x bilinear, align_corners=True), shared by the kernels that write the
// upsampled flow (mpf_raft_glue.hip: k_upflow8, k_upflow8_bwd), by those that only compare it (mpf_upsample.hip: k_up8_loss, k_up8_loss_bwd)
// and by the one that writes a window of it (mpf_raft_eval.hip: k_upflow8_crop), so that a prediction formed anywhere is the prediction
// mpf_upflow8 writes, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

// the scale of an axis of coarse size n, rounded once in fp32: (n-1)/(8n-1), 0 for n == 1
static inline float up8_scale(int n) { return n > 1 ? (float)(n - 1) / (float)(8 * n - 1) : 0.0f; }

// source index pair and weight of fine index I along an axis of coarse size n: ATen's area_pixel_compute_source_index with align_corners
__device__ __forceinline__ void up8_taps(int I, int n, float s, int &i0, int &i1, float &l)
{
    const float src = s * (float)I;
    i0 = min((int)src, n - 1);                                            // the product rounds to n-1 at most; the min only guards the bound
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    l = src - (float)i0;
}

// the fine indices that can touch coarse index i: those whose source coordinate lies in (i-1, i+1), with a margin of one fine index per side
// for the roundings (a coordinate is good to a few 1e-5 of a coarse pixel, a fine index is about 1/8 of one); every candidate is tested
__device__ __forceinline__ void up8_range(int i, int n, int &lo, int &hi)
{
    const int n8 = 8 * n;
    lo = 0, hi = n8 - 1;
    if (n == 1) return;                                                   // scale 0: every fine index reads coarse index 0
    const float inv = (float)(n8 - 1) / (float)(n - 1);
    lo = max(lo, (int)floorf((float)(i - 1) * inv) - 1);
    hi = min(hi, (int)ceilf((float)(i + 1) * inv) + 1);
}

// the weight with which fine index I reads coarse index i: the adjoint of up8_taps' two taps (both, where i0 == i1 at the last index)
__device__ __forceinline__ float up8_weight(int I, int i, int n, float s)
{
    int i0, i1;
    float l;
    up8_taps(I, n, s, i0, i1, l);
    return (i0 == i ? 1.0f - l : 0.0f) + (i1 == i ? l : 0.0f);
}

// 8 * bilinear at one fine pixel from the two coarse rows r0, r1, the taps and weights of up8_taps per axis (hy = 1 - ly, hx = 1 - lx):
// ATen's upsample_bilinear2d, operation for operation.  Every kernel that forms a prediction of upflow8 forms it here.
__device__ __forceinline__ float up8_value(const float *r0, const float *r1, int x0, int x1, float hy, float ly, float hx, float lx)
{
    return 8.0f * (hy * (hx * r0[x0] + lx * r0[x1]) + ly * (hx * r1[x0] + lx * r1[x1]));
}
