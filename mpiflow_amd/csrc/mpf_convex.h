// mpf_convex.h - the arithmetic of RAFT's convex upsampling (RAFT.upsample_flow, RAFT/core/raft.py:72-83) at one fine pixel, shared by the
// kernel that writes, differentiates or compares the whole prediction (mpf_upsample.hip: k_upsample) and by the one that writes a window of it
// (mpf_raft_eval.hip: k_upsample_crop), so that the window is the slice of the whole, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

// 8 * flow on the 3 x 3 neighbourhood of coarse pixel (h, w) of sample n, both channels, 0 outside the map
__device__ __forceinline__ void up_neighbourhood(const float *flow, int n, int H, int W, int h, int w, float f[2][9])
{
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int hh = h + k / 3 - 1, ww = w + k % 3 - 1;
            const bool in = (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W;
            f[c][k] = in ? 8.0f * flow[((n * 2 + c) * H + (in ? hh : h)) * W + (in ? ww : w)] : 0.0f;
        }
}

// one sub-position: taps points at the mask's tap 0 of this pixel and sub-position, the taps lie `plane` = 64 * H * W floats apart.  Leaves the
// max-subtracted softmax p[k] in m and the blend sum_k p[k] * f[c][k] of both channels in o0, o1.
__device__ __forceinline__ void up_convex(const float *taps, int plane, const float f[2][9], float m[9], float &o0, float &o1)
{
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = taps[k * plane];
    float mx = m[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) mx = fmaxf(mx, m[k]);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        m[k] = expf(m[k] - mx);
        s += m[k];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = m[k] / s;
    o0 = m[0] * f[0][0], o1 = m[0] * f[1][0];
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        o0 = fmaf(m[k], f[0][k], o0);
        o1 = fmaf(m[k], f[1][k], o1);
    }
}
