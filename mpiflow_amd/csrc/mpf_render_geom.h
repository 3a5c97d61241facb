// mpf_render_geom.h - the per-plane geometry of Stage B (target pixel -> source coordinate, bilinear weights, warped xyz_tgt), shared by the forward
// kernels of mpf_render.hip and their adjoint in mpf_render_bwd.hip, so that both perform the identical IEEE op sequence.
#pragma once
#include "mpf_common.h"
#include "mpf_math.h"

// d_params is read-only for the whole launch.  hipcc proves that for a plain global pointer only while nothing in the kernel could
// alias it: behind a workgroup barrier (the fence of __syncthreads() counts as a clobber), or inside a kernel that also carries another
// role with stores through unrelated pointers (k_pair_overlap), the per-plane records turn into VECTOR loads issued right before their
// use - measured: 3-6 extra VMEM instructions and a full memory latency per wave and plane, plus the registers to hold them (spills at
// 5 waves per SIMD).  Reading them through the constant address space keeps them on the scalar unit, whatever surrounds the body.
typedef const __attribute__((address_space(4))) float *MpfConstParams;

#ifndef MPF_XYZ_MFMA
#define MPF_XYZ_MFMA 0          // 1: xyz_tgt = G . (r; 1) on the matrix cores (4 x v_mfma_f32_4x4x1 instead of 12 VALU ops), see mpf_geom_core
#endif
struct MpfConsts {
    float fx, fy;
    float halfW, halfH, rhalfW, rhalfH, maxx, maxy;
    float Wf, Hf;
    int W, H;
    unsigned row_bytes;
#if MPF_XYZ_MFMA
    float G0, G1, G2, G3;        // column k of G_tgt_src's 3x4 block, row (lane % 4) - the A operands of the 4x4x1 outer products (row 3: zero)
#endif
};

template <class ParamPtr>
MPF_DEV void mpf_consts_pose(MpfConsts &c, const ParamPtr params)
{
#if MPF_XYZ_MFMA
    const unsigned r = threadIdx.x & 3u;
    c.G0 = r == 0 ? params[9] : (r == 1 ? params[13] : (r == 2 ? params[17] : 0.0f));
    c.G1 = r == 0 ? params[10] : (r == 1 ? params[14] : (r == 2 ? params[18] : 0.0f));
    c.G2 = r == 0 ? params[11] : (r == 1 ? params[15] : (r == 2 ? params[19] : 0.0f));
    c.G3 = r == 0 ? params[12] : (r == 1 ? params[16] : (r == 2 ? params[20] : 0.0f));
#endif
}

// KS: K_src^-1 has the pinhole form [[a,0,b],[0,c,e],[0,0,1]] (checked at run time, uniform).  Then the reference's dense
//     3x3 . (ix,iy,1) chain collapses exactly: a*ix + 0*iy is a*ix, 0*ix + c*iy is c*iy, the third row is exactly 1, and
//     1 * d is d - same bits, 6 fewer VALU ops per plane.
// TP: the stack is followed by >= (W+1) texels of finite padding, so the east / south taps can always be read at
//     +16 / +row bytes (immediate offsets); where they fall outside the image their weight is exactly 0.
// The arithmetic of one plane for one target pixel: source coordinate, bilinear weights, north-west texel (x0, y0) and the
// warped xyz_tgt at the clamped coordinate.  Shared by the gather kernels and the LDS-staged kernel (and by the latter's
// tile-corner evaluation), so every variant performs the identical IEEE op sequence.
template <bool KS, bool WANT_VALID, class ParamPtr>
MPF_DEV float mpf_geom_core(const ParamPtr params, int s, const MpfConsts &c, float &nw, float &ne, float &sw, float &se,
                            float &X, float &Y, float &Z, int &x0, int &y0, float &qz_out)
{
    const ParamPtr rec = params + MPF_PARAMS_HEADER + MPF_PLANE_RECORD * s;
    float qx = mpf_row3_xy1(rec[0], rec[1], rec[2], c.fx, c.fy);
    float qy = mpf_row3_xy1(rec[3], rec[4], rec[5], c.fx, c.fy);
    float qz = mpf_row3_xy1(rec[6], rec[7], rec[8], c.fx, c.fy);
    qz_out = qz;
    const float rz = mpf_rcp_nr(qz);
    float u = mpf_div_nr(qx, qz, rz), v = mpf_div_nr(qy, qz, rz);
    float valid = 0.0f;
    if (WANT_VALID) {
        const bool inside = (u < c.Wf) & (u > -1.0f) & (v < c.Hf) & (v > -1.0f);
        valid = inside ? 1.0f : 0.0f;
    }
    float gx = mpf_div_by_const(u + 0.5f, c.halfW, c.rhalfW) - 1.0f;
    float gy = mpf_div_by_const(v + 0.5f, c.halfH, c.rhalfH) - 1.0f;
    float ix = (gx + 1.0f) * c.halfW - 0.5f;
    float iy = (gy + 1.0f) * c.halfH - 0.5f;
    ix = __builtin_amdgcn_fmed3f(ix, 0.0f, c.maxx);       // min(max_val, max(x, 0)) in one op (inputs are never NaN here)
    iy = __builtin_amdgcn_fmed3f(iy, 0.0f, c.maxy);
    // ix >= 0: x - floor(x) is exact and equals v_fract_f32(x); trunc == floor
    float w = __builtin_amdgcn_fractf(ix), e = 1.0f - w;
    float n = __builtin_amdgcn_fractf(iy), sgt = 1.0f - n;
    nw = sgt * e; ne = sgt * w; sw = n * e; se = n * w;
    x0 = (int)ix; y0 = (int)iy;
    const float d = rec[9];
    float rx, ry, rzz;
    if (KS) {
        rx = (params[0] * ix + params[2]) * d;
        ry = (params[4] * iy + params[5]) * d;
        rzz = d;
    } else {
        rx = mpf_row3_xy1(params[0], params[1], params[2], ix, iy) * d;
        ry = mpf_row3_xy1(params[3], params[4], params[5], ix, iy) * d;
        rzz = mpf_row3_xy1(params[6], params[7], params[8], ix, iy) * d;
    }
#if MPF_XYZ_MFMA
    // v_mfma_f32_4x4x1_16b_f32: D_v(lane) = A(lane 4 * (lane / 4) + v) * B(lane) + C_v(lane), one exact IEEE fma per element - identical to
    // v_fma_f32 on 2 * 10^10 operand triples of this path's ranges (tools/mfma_fma_exact.hip, profiles/r3/mfma_fma_exact.log) - so the chain
    // a0*X, fma(a1,Y,.), fma(a2,Z,.), fma(a3,1,.) of the three rows of G becomes 4 dependent outer products: rows in the accumulator index,
    // this lane's (rx, ry, rz, 1) as B.  (The first step is fma(a0, X, +0): equal to the product except for the sign of an exact zero.)
    typedef float mpf_f4 __attribute__((ext_vector_type(4)));
    mpf_f4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
    acc = __builtin_amdgcn_mfma_f32_4x4x1f32(c.G0, rx, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_4x4x1f32(c.G1, ry, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_4x4x1f32(c.G2, rzz, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_4x4x1f32(c.G3, 1.0f, acc, 0, 0, 0);
    X = acc[0]; Y = acc[1]; Z = acc[2];
#else
    X = mpf_row4_xyz1(params[9], params[10], params[11], params[12], rx, ry, rzz);
    Y = mpf_row4_xyz1(params[13], params[14], params[15], params[16], rx, ry, rzz);
    Z = mpf_row4_xyz1(params[17], params[18], params[19], params[20], rx, ry, rzz);
#endif
    return valid;
}

template <class Geom>
MPF_DEV float mpf_tap4w(const Geom &g, float a, float b, float c, float d)
{
    float o = a * g.nw;
    o = fmaf(b, g.ne, o);
    o = fmaf(c, g.sw, o);
    o = fmaf(d, g.se, o);
    return o;
}
