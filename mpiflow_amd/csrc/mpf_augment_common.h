// mpf_augment_common.h - device helpers shared by the augmentation kernels (mpf_augment.hip, mpf_augment_sparse.hip): cv2 INTER_LINEAR's
// coordinate map and fp32 interpolation, the u8 rounding of the images, and the loads through buffer descriptors sized to each source.
#pragma once
#include "mpf_common.h"

namespace {

struct Tap { int i0, i1; float a; };

// cv2 INTER_LINEAR's source coordinate of destination index d on an axis of n source pixels
__device__ __forceinline__ Tap lin_tap(int d, int n, double inv)
{
    const float f = (float)(((double)d + 0.5) * inv - 0.5);
    Tap t;
    if (f < 0.0f) { t.i0 = 0; t.a = 0.0f; }
    else if (f >= (float)(n - 1)) { t.i0 = n - 1; t.a = 0.0f; }
    else { t.i0 = (int)floorf(f); t.a = f - (float)t.i0; }
    t.i1 = min(t.i0 + 1, n - 1);
    return t;
}

__device__ __forceinline__ float lerp2(float p00, float p01, float p10, float p11, float ax, float ay)
{
    const float bx = 1.0f - ax, by = 1.0f - ay;
    const float r0 = p00 * bx + p01 * ax;
    const float r1 = p10 * bx + p11 * ax;
    return r0 * by + r1 * ay;
}

__device__ __forceinline__ float to_pixel(float v) { return fminf(fmaxf(rintf(v), 0.0f), 255.0f); }

__device__ __forceinline__ float ld_u8(__amdgpu_buffer_rsrc_t rs, unsigned off)
{
    return (float)__builtin_amdgcn_raw_buffer_load_b8(rs, off, 0, 0);
}

// two dword loads (hipcc pairs them into one buffer_load_dwordx2): a form that took the lanes of __builtin_amdgcn_raw_buffer_load_b64's result
// read v equal to u on the GPU (tests/test_online.py caught it)
__device__ __forceinline__ float2 ld_f2(__amdgpu_buffer_rsrc_t rs, unsigned off)
{
    return make_float2(__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0)),
                       __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off + 4u, 0, 0)));
}

}  // namespace
