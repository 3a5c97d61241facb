// mpf_corr_common.h - the two device helpers RAFT's correlation lookups share (mpf_corr.hip: on-demand; mpf_corr_volume.hip: all-pairs)
#pragma once
#include <hip/hip_runtime.h>

// first grid index of the window along one axis and the fraction shared by its taps; n = the level's extent along the axis
__device__ __forceinline__ void corr_axis(float c, float inv, int n, int r, int &i0, float &frac)
{
    const float v = c * inv;                                 // exact: inv is a power of two
    const float fl = floorf(v);
    if (fl >= (float)(-(r + 2)) && fl <= (float)(n + r + 1)) {
        i0 = (int)fl - r;
        frac = v - fl;
    } else {                                                 // NaN, +-inf, or no tap can be inside: the window ends at -1
        i0 = -(2 * r + 2);
        frac = 0.0f;
    }
}

__device__ __forceinline__ float corr_blend(float d00, float d01, float d10, float d11, float fx, float fy)
{
    // d[y][x]; the four bilinear weights, each product rounded
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    float v = (gx * gy) * d00;
    v = fmaf(fx * gy, d01, v);
    v = fmaf(gx * fy, d10, v);
    v = fmaf(fx * fy, d11, v);
    return v;
}
