// mpf_mesh.hip - the warp-back RGB-D mesh renderer for gfx950: what warpback/utils.py asks of pytorch3d (one rasterisation of a regular grid
// mesh with faces_per_pixel = 1, one barycentric interpolation) and the vertex pipeline in front of it.
//
// Contract: include/mpiflow_hip.h (MpfMeshVertexArgs, MpfMeshRasterArgs); INTEGRATION.md section 16 holds the definition, which
// tests/warpback_restated.py restates in numpy.  Every operation is fp32, rounded once, in the order written there (the build has no
// contraction and correctly rounded divide / sqrt).
//
// k_mesh_vertices   one thread per pixel: unproject with depth = 1 / (disp + 1e-4), the extrinsic, the near / far perspective matrix, the
//                   divide, the sign and aspect changes, and the attributes (r, g, b, Sobel visibility, depth after the extrinsic).  Thread 0
//                   of a workgroup inverts cam_int in f64 by the adjugate and rounds it to f32 into LDS.  Nothing intermediate is stored.
// k_mesh_zpass      one thread per face (2 q + which: the two faces of cell q in neighbouring lanes).  The faces are implicit.  A face that
//                   is not skipped gets a bounding box of pixels (below); a LIGHT face (at most MESH_HEAVY pixels) is walked by its lane, a
//                   HEAVY one (stretched across a depth discontinuity, or one face over the whole frame) by its whole wave: the wave
//                   takes its heavy lanes in turn (ballot), broadcasts the face and strides the box 64 pixels at a time.  Every covered
//                   pixel takes a 64-bit atomic min of (bits(pz) << 32) | f: pz >= 0, so the unsigned order is (pz, f) - the least pz, then
//                   the lowest face.  A minimum does not depend on arrival order: identical bytes on every run.
// k_mesh_resolve    one thread per pixel: recomputes the winner's barycentrics with the same function and interpolates.
//
// THE BOUNDING BOX is an accelerator and must not change a pixel.  mesh_cover's sign tests are exact tests on rounded differences, so a
// pixel strictly beyond every vertex on one side can pass all three only if (1) the box is nearer than about 2^-23 of the largest
// vertex-to-pixel distance Dm, or (2) the whole face subtends less than about 2^-23 rad seen from the pixel, which needs
// |area| <= 2^-23 * (longest edge L) * Dm.  The box is therefore widened by sqrt(blur_radius) (d is a squared distance) plus 2^-18 * Dm
// and a quarter pixel for the conversion to indices, and a face with |area| <= 2^-18 * L * Dm, or with anything non-finite in these
// bounds, is not culled at all: its box is the frame.  Every loop is bounded by the box clipped to the frame.
//
// No value-dependent address: a pixel index comes from a clipped box, a face index from a key the z pass wrote (f < F; the resolve pass treats
// any other key as no face, so MPF_MESH_PASS_RESOLVE on a foreign workspace reads nothing out of bounds), a vertex index from a face index.  LDS: 36 bytes (k_mesh_vertices).
#include "mpf_common.h"
#include <math.h>

#define MESH_THREADS 256
#define MESH_HEAVY 64            // pixels in a face's box above which its wave, not its lane, walks it

struct MeshVertDev {
    const float *rgbd, *cam_int, *cam_ext;
    float *verts, *attrs;
    int h, w, hw;
    float pa, pb;                // the perspective matrix's (near + far) / (far - near) and -2 near far / (far - near)
    float aspect;                // float(w / h)
};

struct MeshDev {
    const float *verts, *attrs;  // [B,hw,3], [B,hw,C]
    unsigned long long *keys;    // [B,hw]
    int64_t *pix_to_face;
    float *zbuf, *bary, *out;
    int h, w, hw, C, Q;
    float blur;
    float rblur;                 // the box's share of blur_radius: sqrt, rounded up
    float rangex, offx, rangey, offy, pmax;
};

struct MeshTri {
    float x0, y0, z0, x1, y1, z1, x2, y2, z2;
};

// ---------------------------------------------------------------- the definition, shared by both passes

static inline __host__ __device__ void mesh_ndc_range(int S1, int S2, float &range, float &offset)
{
    range = S1 <= S2 ? 2.0f : ((float)S1 * 2.0f) / (float)S2;
    offset = range / 2.0f;
}

__device__ __forceinline__ float mesh_ndc(int k, int S1, float range, float offset)
{
    return (range * (float)k + offset) / (float)S1 - offset;             // -offset + x, the same sum
}

__device__ __forceinline__ float mesh_edge(float px, float py, float ax, float ay, float bx, float by)
{
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

__device__ __forceinline__ float mesh_seg(float px, float py, float ax, float ay, float bx, float by)
{
    const float abx = bx - ax, aby = by - ay;
    const float l2 = abx * abx + aby * aby;
    if (l2 <= 1e-8f) {
        const float ex = px - bx, ey = py - by;
        return ex * ex + ey * ey;
    }
    float t = (abx * (px - ax) + aby * (py - ay)) / l2;
    if (t < 0.0f) t = 0.0f;
    if (t > 1.0f) t = 1.0f;
    const float qx = ax + t * abx, qy = ay + t * aby;
    const float ex = px - qx, ey = py - qy;
    return ex * ex + ey * ey;
}

__device__ __forceinline__ bool mesh_finite(float v) { return fabsf(v) < __int_as_float(0x7f800000); }

// the face-level skip rules; area = E(v2; v0, v1)
__device__ __forceinline__ bool mesh_face_ok(const MeshTri &t, float &area)
{
    const bool fin = mesh_finite(t.x0) && mesh_finite(t.y0) && mesh_finite(t.z0) && mesh_finite(t.x1) && mesh_finite(t.y1) && mesh_finite(t.z1) &&
                     mesh_finite(t.x2) && mesh_finite(t.y2) && mesh_finite(t.z2);
    area = mesh_edge(t.x2, t.y2, t.x0, t.y0, t.x1, t.y1);
    if (!fin || fabsf(area) <= 1e-8f) return false;
    if (t.z0 < 0.0f && t.z1 < 0.0f && t.z2 < 0.0f) return false;        // max(z0, z1, z2) < 0
    return true;
}

// one face at one pixel centre: barycentrics, depth, and whether the face covers the pixel
__device__ __forceinline__ bool mesh_cover(const MeshTri &t, float area, float px, float py, float blur, float &w0, float &w1, float &w2, float &pz)
{
    const float den = area + 1e-8f;
    w0 = mesh_edge(px, py, t.x1, t.y1, t.x2, t.y2) / den;
    w1 = mesh_edge(px, py, t.x2, t.y2, t.x0, t.y0) / den;
    w2 = mesh_edge(px, py, t.x0, t.y0, t.x1, t.y1) / den;
    pz = (w0 * t.z0 + w1 * t.z1) + w2 * t.z2;
    if (!(pz >= 0.0f)) return false;
    if (w0 > 0.0f && w1 > 0.0f && w2 > 0.0f) return true;
    float d = mesh_seg(px, py, t.x0, t.y0, t.x1, t.y1);
    const float d02 = mesh_seg(px, py, t.x0, t.y0, t.x2, t.y2);
    const float d12 = mesh_seg(px, py, t.x1, t.y1, t.x2, t.y2);
    if (d02 < d) d = d02;
    if (d12 < d) d = d12;
    return d < blur;
}

// face f of the grid: cell q = r (w - 1) + c; f < Q: (tl, bl, br), else (br, tr, tl)
__device__ __forceinline__ void mesh_face_verts(int f, int Q, int w, int &i0, int &i1, int &i2)
{
    const int q = f < Q ? f : f - Q;
    const int r = q / (w - 1), c = q - r * (w - 1);
    const int tl = r * w + c, bl = tl + w;
    if (f < Q) i0 = tl, i1 = bl, i2 = bl + 1;
    else i0 = bl + 1, i1 = tl + 1, i2 = tl;
}

__device__ __forceinline__ void mesh_load(const float *v, int i0, int i1, int i2, MeshTri &t)
{
    const float *p0 = v + (size_t)i0 * 3, *p1 = v + (size_t)i1 * 3, *p2 = v + (size_t)i2 * 3;
    t.x0 = p0[0], t.y0 = p0[1], t.z0 = p0[2];
    t.x1 = p1[0], t.y1 = p1[1], t.z1 = p1[2];
    t.x2 = p2[0], t.y2 = p2[1], t.z2 = p2[2];
}

// ---------------------------------------------------------------- the bounding box (an accelerator; see the head of the file)

// pixel indices [i0, i1] of one axis whose centres may lie in [lo, hi]; the index DEcreases with the coordinate.  NaN gives the whole axis.
__device__ __forceinline__ void mesh_axis(float lo, float hi, int S, float range, float offset, int &i0, int &i1)
{
    const float fS = (float)S, last = (float)(S - 1);
    const float fa = last - ((hi + offset) * fS - offset) / range - 0.25f;
    const float fb = last - ((lo + offset) * fS - offset) / range + 0.25f;
    i0 = !(fa > 0.0f) ? 0 : (fa >= fS ? S : (int)fa);
    i1 = !(fb < last) ? S - 1 : (fb < 0.0f ? -1 : (int)fb + 1);
    if (i1 > S - 1) i1 = S - 1;
}

__device__ __forceinline__ void mesh_box(const MeshDev &a, const MeshTri &t, float area, int &c0, int &c1, int &r0, int &r1)
{
    const float xmin = fminf(t.x0, fminf(t.x1, t.x2)), xmax = fmaxf(t.x0, fmaxf(t.x1, t.x2));
    const float ymin = fminf(t.y0, fminf(t.y1, t.y2)), ymax = fmaxf(t.y0, fmaxf(t.y1, t.y2));
    const float amax = fmaxf(fmaxf(fabsf(xmin), fabsf(xmax)), fmaxf(fabsf(ymin), fabsf(ymax)));
    const float Dm = 2.0f * (a.pmax + amax);
    const float L = 2.0f * fmaxf(xmax - xmin, ymax - ymin);
    const float slack = 0x1p-18f * Dm;
    if (!(fabsf(area) > slack * L) || !mesh_finite(slack * L)) {          // seen edge-on within rounding, or out of range: no cull
        c0 = 0, c1 = a.w - 1, r0 = 0, r1 = a.h - 1;
        return;
    }
    const float m = a.rblur + slack;
    mesh_axis(xmin - m, xmax + m, a.w, a.rangex, a.offx, c0, c1);
    mesh_axis(ymin - m, ymax + m, a.h, a.rangey, a.offy, r0, r1);
}

__device__ __forceinline__ void mesh_vote(const MeshDev &a, unsigned long long *keys, const MeshTri &t, float area, int f, int r, int c)
{
    const float py = mesh_ndc(a.h - 1 - r, a.h, a.rangey, a.offy);
    const float px = mesh_ndc(a.w - 1 - c, a.w, a.rangex, a.offx);
    float w0, w1, w2, pz;
    if (!mesh_cover(t, area, px, py, a.blur, w0, w1, w2, pz)) return;
    const unsigned int zb = pz == 0.0f ? 0u : __float_as_uint(pz);        // -0 ties with +0
    atomicMin(keys + (size_t)r * a.w + c, ((unsigned long long)zb << 32) | (unsigned int)f);
}

__global__ __launch_bounds__(MESH_THREADS) void k_mesh_zpass(const MeshDev a)
{
    const int b = blockIdx.y;
    const int t = blockIdx.x * MESH_THREADS + threadIdx.x;                // 2 q + which
    const int lane = threadIdx.x & 63;
    unsigned long long *keys = a.keys + (size_t)b * a.hw;
    MeshTri tri = MeshTri{};
    float area = 0.0f;
    int f = 0, c0 = 0, c1 = -1, r0 = 0, r1 = -1;
    if (t < 2 * a.Q) {
        f = (t & 1) ? a.Q + (t >> 1) : (t >> 1);
        int i0, i1, i2;
        mesh_face_verts(f, a.Q, a.w, i0, i1, i2);
        mesh_load(a.verts + (size_t)b * a.hw * 3, i0, i1, i2, tri);
        if (mesh_face_ok(tri, area)) mesh_box(a, tri, area, c0, c1, r0, r1);
    }
    const int bw = c1 - c0 + 1, bh = r1 - r0 + 1;
    const int n = (bw > 0 && bh > 0) ? bw * bh : 0;                       // at most h * w
    const bool heavy = n > MESH_HEAVY;
    if (n > 0 && !heavy)
        for (int r = r0; r <= r1; ++r)
            for (int c = c0; c <= c1; ++c) mesh_vote(a, keys, tri, area, f, r, c);
    unsigned long long todo = __ballot(heavy);                            // wave-uniform: every lane walks every heavy face of its wave
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        MeshTri s;
        s.x0 = __shfl(tri.x0, src), s.y0 = __shfl(tri.y0, src), s.z0 = __shfl(tri.z0, src);
        s.x1 = __shfl(tri.x1, src), s.y1 = __shfl(tri.y1, src), s.z1 = __shfl(tri.z1, src);
        s.x2 = __shfl(tri.x2, src), s.y2 = __shfl(tri.y2, src), s.z2 = __shfl(tri.z2, src);
        const float sarea = __shfl(area, src);
        const int sf = __shfl(f, src), sc0 = __shfl(c0, src), sr0 = __shfl(r0, src), sbw = __shfl(bw, src), sn = __shfl(n, src);
        for (int i = lane; i < sn; i += 64) {
            const int rr = i / sbw;
            mesh_vote(a, keys, s, sarea, sf, sr0 + rr, sc0 + (i - rr * sbw));
        }
    }
}

__global__ __launch_bounds__(MESH_THREADS) void k_mesh_resolve(const MeshDev a)
{
    const int b = blockIdx.y;
    const int p = blockIdx.x * MESH_THREADS + threadIdx.x;
    if (p >= a.hw) return;                                                // no barrier below
    const size_t o = (size_t)b * a.hw + p;
    const unsigned long long key = a.keys[o];
    float *out = a.out + (size_t)b * a.C * a.hw + p;
    if (key == ~0ull || (unsigned int)(key & 0xffffffffull) >= 2u * (unsigned int)a.Q) {   // no face; or, resolve pass alone, not a key of a z pass
        a.pix_to_face[o] = -1;
        a.zbuf[o] = -1.0f;
        a.bary[o * 3 + 0] = -1.0f, a.bary[o * 3 + 1] = -1.0f, a.bary[o * 3 + 2] = -1.0f;
        for (int k = 0; k < a.C; ++k) out[(size_t)k * a.hw] = 0.0f;
        return;
    }
    const int f = (int)(unsigned int)(key & 0xffffffffull);               // < 2 Q, checked above
    int i0, i1, i2;
    mesh_face_verts(f, a.Q, a.w, i0, i1, i2);
    MeshTri tri;
    mesh_load(a.verts + (size_t)b * a.hw * 3, i0, i1, i2, tri);
    const float area = mesh_edge(tri.x2, tri.y2, tri.x0, tri.y0, tri.x1, tri.y1);
    const int r = p / a.w, c = p - r * a.w;
    const float py = mesh_ndc(a.h - 1 - r, a.h, a.rangey, a.offy);
    const float px = mesh_ndc(a.w - 1 - c, a.w, a.rangex, a.offx);
    float w0, w1, w2, pz;
    mesh_cover(tri, area, px, py, a.blur, w0, w1, w2, pz);
    a.pix_to_face[o] = (int64_t)b * (2 * (int64_t)a.Q) + f;
    a.zbuf[o] = pz;
    a.bary[o * 3 + 0] = w0, a.bary[o * 3 + 1] = w1, a.bary[o * 3 + 2] = w2;
    const float *at = a.attrs + (size_t)b * a.hw * a.C;
    const float *a0 = at + (size_t)i0 * a.C, *a1 = at + (size_t)i1 * a.C, *a2 = at + (size_t)i2 * a.C;
    for (int k = 0; k < a.C; ++k) out[(size_t)k * a.hw] = (w0 * a0[k] + w1 * a1[k]) + w2 * a2[k];
}

// ---------------------------------------------------------------- the vertex stage

__global__ __launch_bounds__(MESH_THREADS) void k_mesh_vertices(const MeshVertDev a)
{
    __shared__ float sKinv[9];
    const int b = blockIdx.y;
    if (threadIdx.x == 0) {                                               // the adjugate in f64, rounded to f32 once
        const float *K = a.cam_int + (size_t)b * 9;
        const double k0 = K[0], k1 = K[1], k2 = K[2], k3 = K[3], k4 = K[4], k5 = K[5], k6 = K[6], k7 = K[7], k8 = K[8];
        const double c0 = k4 * k8 - k5 * k7, c1 = k5 * k6 - k3 * k8, c2 = k3 * k7 - k4 * k6;
        const double det = k0 * c0 + k1 * c1 + k2 * c2;
        sKinv[0] = (float)(c0 / det), sKinv[1] = (float)((k2 * k7 - k1 * k8) / det), sKinv[2] = (float)((k1 * k5 - k2 * k4) / det);
        sKinv[3] = (float)(c1 / det), sKinv[4] = (float)((k0 * k8 - k2 * k6) / det), sKinv[5] = (float)((k2 * k3 - k0 * k5) / det);
        sKinv[6] = (float)(c2 / det), sKinv[7] = (float)((k1 * k6 - k0 * k7) / det), sKinv[8] = (float)((k0 * k4 - k1 * k3) / det);
    }
    __syncthreads();
    const int p = blockIdx.x * MESH_THREADS + threadIdx.x;
    if (p >= a.hw) return;                                                // after the only barrier
    const int y = p / a.w, x = p - y * a.w;
    const float *img = a.rgbd + (size_t)b * 4 * a.hw;
    const float *D = img + (size_t)3 * a.hw;
    const float u = ((float)x + 0.5f) / (float)a.w, v = ((float)y + 0.5f) / (float)a.h;
    const float depth = 1.0f / (D[p] + 1e-4f);
    const float X = ((sKinv[0] * u + sKinv[1] * v) + sKinv[2]) * depth;
    const float Y = ((sKinv[3] * u + sKinv[4] * v) + sKinv[5]) * depth;
    const float Z = ((sKinv[6] * u + sKinv[7] * v) + sKinv[8]) * depth;
    const float *E = a.cam_ext + (size_t)b * 12;
    const float wx = ((E[0] * X + E[1] * Y) + E[2] * Z) + E[3];
    const float wy = ((E[4] * X + E[5] * Y) + E[6] * Z) + E[7];
    const float wz = ((E[8] * X + E[9] * Y) + E[10] * Z) + E[11];
    const float *K = a.cam_int + (size_t)b * 9;
    const float nx = (2.0f * K[0]) * wx + (2.0f * K[2] - 1.0f) * wz;      // the matrix's zero entries add nothing
    const float ny = (2.0f * K[4]) * wy + (2.0f * K[5] - 1.0f) * wz;
    const float nz = a.pa * wz + a.pb;
    float *vo = a.verts + ((size_t)b * a.hw + p) * 3;
    vo[0] = (nx / wz) * -1.0f * a.aspect;
    vo[1] = (ny / wz) * -1.0f;
    vo[2] = nz / wz;
    // Sobel of the disparity, zero padding
    const bool up = y > 0, dn = y < a.h - 1, lf = x > 0, rt = x < a.w - 1;
    const float d00 = up && lf ? D[p - a.w - 1] : 0.0f, d01 = up ? D[p - a.w] : 0.0f, d02 = up && rt ? D[p - a.w + 1] : 0.0f;
    const float d10 = lf ? D[p - 1] : 0.0f, d12 = rt ? D[p + 1] : 0.0f;
    const float d20 = dn && lf ? D[p + a.w - 1] : 0.0f, d21 = dn ? D[p + a.w] : 0.0f, d22 = dn && rt ? D[p + a.w + 1] : 0.0f;
    const float gx = ((d02 - d00) + 2.0f * (d12 - d10)) + (d22 - d20);
    const float gy = ((d20 - d00) + 2.0f * (d21 - d01)) + (d22 - d02);
    const float alpha = expf(-10.0f * sqrtf(gx * gx + gy * gy));
    float *ao = a.attrs + ((size_t)b * a.hw + p) * 5;
    ao[0] = img[p], ao[1] = img[(size_t)a.hw + p], ao[2] = img[(size_t)2 * a.hw + p];
    ao[3] = alpha > 0.3f ? 1.0f : 0.0f;
    ao[4] = wz;
}

// ---------------------------------------------------------------- launchers

static int mesh_shape(int B, int h, int w, const char *who)
{
    MPF_REQUIRE(B >= 1 && B <= 65535, "%s: bad shape: B must be 1..65535 (got %d)", who, B);
    MPF_REQUIRE(h >= 2 && w >= 2, "%s: bad shape: a grid mesh needs h, w >= 2 (got h, w = %d, %d)", who, h, w);
    MPF_REQUIRE((int64_t)B * h * w <= MPF_MESH_MAX_BHW, "%s: bad shape: B * h * w must be at most %d: the face count 2 (h - 1)(w - 1) and every index stay in an int "
                "(got B, h, w = %d, %d, %d)", who, MPF_MESH_MAX_BHW, B, h, w);
    return 0;
}

static bool mesh_overlap(const void *p, size_t pn, const void *q, size_t qn)
{
    const char *a = (const char *)p, *b = (const char *)q;
    return a < b + qn && b < a + pn;
}

extern "C" int mpf_rgbd_mesh_vertices(const MpfMeshVertexArgs *a, void *stream)
{
    const char *who = "mpf_rgbd_mesh_vertices";
    MPF_REQUIRE(a, "%s: null argument block", who);
    const int rc = mesh_shape(a->B, a->h, a->w, who);
    if (rc) return rc;
    MPF_REQUIRE(a->rgbd && a->cam_int && a->cam_ext && a->verts_ndc && a->attrs, "%s: null pointer (rgbd, cam_int, cam_ext, verts_ndc or attrs)", who);
    const size_t hw = (size_t)a->h * a->w, nin = (size_t)a->B * 4 * hw * 4, nv = (size_t)a->B * hw * 12, na = (size_t)a->B * hw * 20;
    MPF_REQUIRE(!mesh_overlap(a->verts_ndc, nv, a->rgbd, nin) && !mesh_overlap(a->attrs, na, a->rgbd, nin) && !mesh_overlap(a->verts_ndc, nv, a->attrs, na),
                "%s: the outputs must not overlap rgbd or each other (a vertex reads its neighbours' disparity)", who);
    MeshVertDev d = MeshVertDev{};
    d.rgbd = a->rgbd, d.cam_int = a->cam_int, d.cam_ext = a->cam_ext, d.verts = a->verts_ndc, d.attrs = a->attrs;
    d.h = a->h, d.w = a->w, d.hw = (int)hw;
    const float near_z = 1e-4f, far_z = 1e4f;                             // RGBDRenderer.near_z / far_z, in the reference's f32 order
    d.pa = (near_z + far_z) / (far_z - near_z);
    d.pb = ((-2.0f * near_z) * far_z) / (far_z - near_z);
    d.aspect = (float)((double)a->w / (double)a->h);
    hipLaunchKernelGGL(k_mesh_vertices, dim3((unsigned)((hw + MESH_THREADS - 1) / MESH_THREADS), (unsigned)a->B), dim3(MESH_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_mesh_vertices");
}

extern "C" size_t mpf_rasterize_grid_workspace(int B, int h, int w)
{
    if (mesh_shape(B, h, w, "mpf_rasterize_grid_workspace")) return 0;
    return (size_t)B * h * w * sizeof(unsigned long long);
}

extern "C" int mpf_rasterize_grid(const MpfMeshRasterArgs *a, void *stream)
{
    const char *who = "mpf_rasterize_grid";
    MPF_REQUIRE(a, "%s: null argument block", who);
    const int rc = mesh_shape(a->B, a->h, a->w, who);
    if (rc) return rc;
    MPF_REQUIRE(a->C >= 1 && a->C <= MPF_MESH_MAX_ATTRS, "%s: C must be 1..%d attributes per vertex (got %d)", who, MPF_MESH_MAX_ATTRS, a->C);
    MPF_REQUIRE(a->passes == MPF_MESH_PASS_ALL || a->passes == MPF_MESH_PASS_Z || a->passes == MPF_MESH_PASS_RESOLVE, "%s: passes must be 0, 1 or 2 (got %d)", who, a->passes);
    const bool resolve = a->passes != MPF_MESH_PASS_Z, zpass = a->passes != MPF_MESH_PASS_RESOLVE;
    MPF_REQUIRE(a->verts_ndc && a->attrs, "%s: null pointer (verts_ndc or attrs)", who);
    MPF_REQUIRE(!resolve || (a->pix_to_face && a->zbuf && a->bary && a->out), "%s: null pointer (pix_to_face, zbuf, bary or out)", who);
    MPF_REQUIRE((((uintptr_t)a->pix_to_face) & 7) == 0, "%s: pix_to_face must be 8-byte aligned", who);
    MPF_REQUIRE(a->workspace, "%s: null pointer (workspace)", who);
    MPF_REQUIRE((((uintptr_t)a->workspace) & 7) == 0, "%s: workspace must be 8-byte aligned", who);
    const size_t hw = (size_t)a->h * a->w, need = (size_t)a->B * hw * sizeof(unsigned long long);
    MPF_REQUIRE(a->workspace_bytes >= need, "%s: workspace holds %zu bytes, %zu needed (mpf_rasterize_grid_workspace)", who, a->workspace_bytes, need);
    const size_t nv = (size_t)a->B * hw * 12, na = (size_t)a->B * hw * a->C * 4;
    const void *outs[4] = {a->pix_to_face, a->zbuf, a->bary, a->out};
    const size_t outn[4] = {(size_t)a->B * hw * 8, (size_t)a->B * hw * 4, nv, na};
    for (int i = 0; resolve && i < 4; ++i)
        MPF_REQUIRE(!mesh_overlap(outs[i], outn[i], a->verts_ndc, nv) && !mesh_overlap(outs[i], outn[i], a->attrs, na) &&
                    !mesh_overlap(outs[i], outn[i], a->workspace, need), "%s: an output overlaps verts_ndc, attrs or the workspace (a pixel reads any vertex)", who);
    MeshDev d = MeshDev{};
    d.verts = a->verts_ndc, d.attrs = a->attrs, d.keys = (unsigned long long *)a->workspace;
    d.pix_to_face = a->pix_to_face, d.zbuf = a->zbuf, d.bary = a->bary, d.out = a->out;
    d.h = a->h, d.w = a->w, d.hw = (int)hw, d.C = a->C, d.Q = (a->h - 1) * (a->w - 1);
    d.blur = a->blur_radius;
    d.rblur = a->blur_radius > 0.0f ? sqrtf(a->blur_radius) * 1.001f : 0.0f;
    mesh_ndc_range(a->w, a->h, d.rangex, d.offx);
    mesh_ndc_range(a->h, a->w, d.rangey, d.offy);
    d.pmax = d.offx > d.offy ? d.offx : d.offy;
    if (zpass) {
        MPF_HIP(hipMemsetAsync(a->workspace, 0xff, need, (hipStream_t)stream));   // every key: no face
        const unsigned faces = 2u * (unsigned)d.Q;
        hipLaunchKernelGGL(k_mesh_zpass, dim3((faces + MESH_THREADS - 1) / MESH_THREADS, (unsigned)a->B), dim3(MESH_THREADS), 0, (hipStream_t)stream, d);
        const int st = mpf_launch_status("k_mesh_zpass");
        if (st || !resolve) return st;
    }
    hipLaunchKernelGGL(k_mesh_resolve, dim3((unsigned)((hw + MESH_THREADS - 1) / MESH_THREADS), (unsigned)a->B), dim3(MESH_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_mesh_resolve");
}
