// mpf_corr_volume.hip - RAFT's all-pairs correlation block (CorrBlock of RAFT/core/corr.py:12-60) for gfx950: the pyramid of the volume, the
// lookup of all levels in one launch, and both gradients.  The three GEMMs (the volume; grad_fmap1, grad_fmap2) stay with the caller.
//
// Contract: include/mpiflow_hip.h (MpfCorrVolumeArgs).  level[l] is [B*H*W, Hl, Wl]: ROW p of every level belongs to query pixel p alone.
// That is what the two gradient kernels live on: the scatter of a lookup's cotangent touches only the rows of its own pixels, so one thread
// owns every entry it updates (a plain load, add, store: no atomics, bit-identical from run to run), and twelve lookups add into ONE
// gradient pyramid that is folded once.
//
// k_cv_pyramid   block = one strip of S = 2^(levels-1) image rows of one row p (the smallest piece that pools down to whole entries of every
//                level).  The strip of level 0 is divided by norm in place and kept in LDS, each further level is pooled from the one before
//                it in LDS (torch's order: ((a00 + a01) + a10) + a11, times 1/4) and stored: one read and one write of level 0, one write of
//                the rest.
// k_cv_lookup    block = CV_TILE consecutive query pixels of one level.  The (rd+1)^2 patch of each pixel's row goes to LDS once (lane = patch
//                point, so a wave-instruction fetches whole 4*(rd+1)-byte row segments), then lane = pixel blends the rd^2 outputs of a
//                channel: the stores are runs of CV_TILE pixels along x.  The patch stride in LDS is odd: lane = pixel reads without conflicts.
// k_cv_lookup_backward  the transpose with the same two mappings: the tile's cotangent goes to LDS in runs of CV_TILE pixels, then
//                lane = patch point gathers its (at most four) cotangent entries and adds the sum into its own entry of the gradient pyramid.
// k_cv_fold      same strips as k_cv_pyramid; entry (y, x) of level 0 becomes (g0 + (g1 + (g2 + ...) / 4) / 4) / norm, with g_l taken at
//                (y >> l, x >> l) where level l covers it (floor pooling drops the last odd row / column), in place.
// With W a multiple of 4 (and 16-byte aligned levels) the level-0 traffic of k_cv_pyramid and k_cv_fold is 16 bytes per lane.
//
// Untrusted coordinates: corr_axis() (mpf_corr_common.h) is the only place a coordinate becomes an integer; a NaN, +-inf or far-out value puts
// the whole window at negative indices, and every patch point is tested against the level's bounds before its address is formed.  Row offsets
// are 64-bit: level 0 of 2 x 128 x 192 has 1.2e9 entries.
#include "mpf_common.h"
#include "mpf_corr_common.h"

#define CV_TILE 32               // query pixels per block of the two lookup kernels
#define CV_THREADS 256
#define CV_MAX_STRIP 12288       // floats of one strip of level 0 (S * W): with the pooled levels behind it 64 KiB of LDS

struct CvDev {
    float *level[MPF_CORR_MAX_LEVELS];
    const float *coords;
    float *out;
    int B, H, W;
    int Hl[MPF_CORR_MAX_LEVELS], Wl[MPF_CORR_MAX_LEVELS];
    int radius, levels;
    float norm;
};

template <bool VEC>
__global__ __launch_bounds__(CV_THREADS) void k_cv_pyramid(const CvDev a, int nstrips)
{
    extern __shared__ __align__(16) float sm[];              // the strip of level 0, then of level 1, ...
    const int L = a.levels, S = 1 << (L - 1), H = a.H, W = a.W;
    const long long p = blockIdx.x / nstrips;
    const int y0 = (int)(blockIdx.x - p * nstrips) * S;
    const int n0 = min(S, H - y0) * W;
    float *g0 = a.level[0] + p * ((long long)H * W) + (long long)y0 * W;
    const float norm = a.norm;
    if (VEC) {
        for (int i = 4 * threadIdx.x; i < n0; i += 4 * CV_THREADS) {
            float4 v = *(const float4 *)(g0 + i);
            v.x /= norm, v.y /= norm, v.z /= norm, v.w /= norm;
            *(float4 *)(g0 + i) = v;
            *(float4 *)(sm + i) = v;
        }
    } else {
        for (int i = threadIdx.x; i < n0; i += CV_THREADS) {
            const float v = g0[i] / norm;
            g0[i] = v;
            sm[i] = v;
        }
    }
    __syncthreads();
    float *src = sm;
    int srcW = W;
    for (int l = 1; l < L; ++l) {
        const int Hl = a.Hl[l], Wl = a.Wl[l];
        const int yl0 = y0 >> l;
        const int nl = min(S >> l, Hl - yl0) * Wl;           // <= 0: the strip holds only rows this level drops
        float *dst = src + (S >> (l - 1)) * srcW;
        float *gl = a.level[l] + p * ((long long)Hl * Wl) + (long long)yl0 * Wl;
        for (int i = threadIdx.x; i < nl; i += CV_THREADS) {
            const int y = i / Wl, x = i - y * Wl;
            const float *q = src + (2 * y) * srcW + 2 * x;
            const float v = (((q[0] + q[1]) + q[srcW]) + q[srcW + 1]) * 0.25f;
            dst[i] = v;
            gl[i] = v;
        }
        __syncthreads();
        src = dst;
        srcW = Wl;
    }
}

// what the levels above 0 add to the gradient of entry (y, x) of level 0, before the division by 4 of level 1's own pooling
__device__ __forceinline__ float cv_upper(const CvDev &a, long long p, int y, int x)
{
    float acc = 0.0f;
    for (int l = a.levels - 1; l >= 1; --l) {
        const int Hl = a.Hl[l], Wl = a.Wl[l], yl = y >> l, xl = x >> l;
        if (yl < Hl && xl < Wl) acc = a.level[l][p * ((long long)Hl * Wl) + yl * Wl + xl] + 0.25f * acc;       // a level that covers (y, x): so do all below it
    }
    return acc;
}

template <bool VEC>
__global__ __launch_bounds__(CV_THREADS) void k_cv_fold(const CvDev a, int nstrips)
{
    const int S = 1 << (a.levels - 1), H = a.H, W = a.W;
    const long long p = blockIdx.x / nstrips;
    const int y0 = (int)(blockIdx.x - p * nstrips) * S;
    const int n0 = min(S, H - y0) * W;
    float *g0 = a.level[0] + p * ((long long)H * W) + (long long)y0 * W;
    const float norm = a.norm;
    if (VEC) {
        for (int i = 4 * threadIdx.x; i < n0; i += 4 * CV_THREADS) {
            const int y = y0 + i / W, x = i % W;             // W % 4 == 0: the four entries share the row
            float4 v = *(const float4 *)(g0 + i);
            v.x = (v.x + 0.25f * cv_upper(a, p, y, x)) / norm;
            v.y = (v.y + 0.25f * cv_upper(a, p, y, x + 1)) / norm;
            v.z = (v.z + 0.25f * cv_upper(a, p, y, x + 2)) / norm;
            v.w = (v.w + 0.25f * cv_upper(a, p, y, x + 3)) / norm;
            *(float4 *)(g0 + i) = v;
        }
    } else {
        for (int i = threadIdx.x; i < n0; i += CV_THREADS) {
            const int y = y0 + i / W, x = i % W;
            g0[i] = (g0[i] + 0.25f * cv_upper(a, p, y, x)) / norm;
        }
    }
}

// LDS of the two lookup kernels: the tile's patches (forward) or cotangents (backward), then per pixel: window origin, fractions, batch index
// and position in the frame (b < 0: the tile ends before this pixel)
struct CvTile {
    float *data;
    int *x0, *y0, *b, *yx;
    float *fx, *fy;
};

__device__ __forceinline__ CvTile cv_tile(float *sm, int ndata, const CvDev &a, int lvl, int r, long long tile0)
{
    CvTile t;
    t.data = sm;
    t.x0 = (int *)(sm + ndata);
    t.y0 = t.x0 + CV_TILE;
    t.b = t.y0 + CV_TILE;
    t.yx = t.b + CV_TILE;
    t.fx = (float *)(t.yx + CV_TILE);
    t.fy = t.fx + CV_TILE;
    if (threadIdx.x < CV_TILE) {
        const int HW = a.H * a.W;
        const long long pix = tile0 + threadIdx.x;
        int x0 = -(2 * r + 2), y0 = -(2 * r + 2), b = -1, yx = 0;      // past the end: every patch point is outside
        float fx = 0.0f, fy = 0.0f;
        if (pix < (long long)a.B * HW) {
            b = (int)(pix / HW);
            yx = (int)(pix - (long long)b * HW);
            const float inv = 1.0f / (float)(1 << lvl);
            corr_axis(a.coords[((long long)b * 2 + 0) * HW + yx], inv, a.Wl[lvl], r, x0, fx);
            corr_axis(a.coords[((long long)b * 2 + 1) * HW + yx], inv, a.Hl[lvl], r, y0, fy);
        }
        t.x0[threadIdx.x] = x0, t.y0[threadIdx.x] = y0, t.b[threadIdx.x] = b, t.yx[threadIdx.x] = yx;
        t.fx[threadIdx.x] = fx, t.fy[threadIdx.x] = fy;
    }
    __syncthreads();
    return t;
}

// R: the radius as a compile-time constant (RAFT's 4: the index arithmetic becomes shifts and multiplies), 0: read it from the arguments
template <int R>
__global__ __launch_bounds__(CV_THREADS) void k_cv_lookup(const CvDev a)
{
    extern __shared__ __align__(16) float sm[];
    const int r = R ? R : a.radius, rd = 2 * r + 1, rd1 = rd + 1, npts = rd1 * rd1, stride = npts + 1;      // npts is even: an odd stride
    const int lvl = blockIdx.y, Hl = a.Hl[lvl], Wl = a.Wl[lvl], HW = a.H * a.W;
    const long long tile0 = (long long)blockIdx.x * CV_TILE, HWl = (long long)Hl * Wl;
    const CvTile t = cv_tile(sm, CV_TILE * stride, a, lvl, r, tile0);
    const float *__restrict__ vol = a.level[lvl];
#pragma unroll 4
    for (int i = threadIdx.x; i < CV_TILE * npts; i += CV_THREADS) {
        const int p = i / npts, k = i - p * npts, jy = k / rd1, jx = k - jy * rd1;
        const int ix = t.x0[p] + jx, iy = t.y0[p] + jy;
        float v = 0.0f;
        if ((unsigned)ix < (unsigned)Wl && (unsigned)iy < (unsigned)Hl) v = vol[(tile0 + p) * HWl + iy * Wl + ix];
        t.data[p * stride + k] = v;
    }
    __syncthreads();
    const long long CH = (long long)a.levels * rd * rd;
    for (int i = threadIdx.x; i < rd * rd * CV_TILE; i += CV_THREADS) {
        const int o = i / CV_TILE, p = i - o * CV_TILE;
        if (t.b[p] < 0) continue;
        const int ai = o / rd, ci = o - ai * rd;             // ai moves x, ci moves y
        const float *d = t.data + p * stride + ci * rd1 + ai;
        a.out[(t.b[p] * CH + (long long)lvl * rd * rd + o) * HW + t.yx[p]] = corr_blend(d[0], d[1], d[rd1], d[rd1 + 1], t.fx[p], t.fy[p]);
    }
}

template <int R>
__global__ __launch_bounds__(CV_THREADS) void k_cv_lookup_backward(const CvDev a)
{
    extern __shared__ __align__(16) float sm[];
    const int r = R ? R : a.radius, rd = 2 * r + 1, rd1 = rd + 1, npts = rd1 * rd1, nout = rd * rd;          // nout is odd: the stride of a pixel's cotangents
    const int lvl = blockIdx.y, Hl = a.Hl[lvl], Wl = a.Wl[lvl], HW = a.H * a.W;
    const long long tile0 = (long long)blockIdx.x * CV_TILE, HWl = (long long)Hl * Wl;
    const CvTile t = cv_tile(sm, CV_TILE * nout, a, lvl, r, tile0);
    const long long CH = (long long)a.levels * nout;
    for (int i = threadIdx.x; i < nout * CV_TILE; i += CV_THREADS) {
        const int o = i / CV_TILE, p = i - o * CV_TILE;
        t.data[p * nout + o] = t.b[p] < 0 ? 0.0f : a.out[(t.b[p] * CH + (long long)lvl * nout + o) * HW + t.yx[p]];
    }
    __syncthreads();
    float *__restrict__ grad = a.level[lvl];
#pragma unroll 4
    for (int i = threadIdx.x; i < CV_TILE * npts; i += CV_THREADS) {
        const int p = i / npts, k = i - p * npts, jy = k / rd1, jx = k - jy * rd1;
        const int ix = t.x0[p] + jx, iy = t.y0[p] + jy;
        if ((unsigned)ix >= (unsigned)Wl || (unsigned)iy >= (unsigned)Hl) continue;
        // patch point (jy, jx) is tap d00 of output (a = jx, c = jy), d01 of (jx - 1, jy), d10 of (jx, jy - 1), d11 of (jx - 1, jy - 1)
        const float fx = t.fx[p], fy = t.fy[p], gx = 1.0f - fx, gy = 1.0f - fy;
        const float *go = t.data + p * nout;
        float s = 0.0f;
        if (jx < rd && jy < rd) s = (gx * gy) * go[jx * rd + jy];
        if (jx > 0 && jy < rd) s = fmaf(fx * gy, go[(jx - 1) * rd + jy], s);
        if (jx < rd && jy > 0) s = fmaf(gx * fy, go[jx * rd + jy - 1], s);
        if (jx > 0 && jy > 0) s = fmaf(fx * fy, go[(jx - 1) * rd + jy - 1], s);
        float *g = grad + (tile0 + p) * HWl + iy * Wl + ix;  // this thread is the only one of the launch that touches this entry
        *g += s;
    }
}

static int cv_check(const MpfCorrVolumeArgs *a, bool lookup, const char *who, CvDev &d)
{
    MPF_REQUIRE(a, "%s: null argument block", who);
    MPF_REQUIRE(a->levels >= 1 && a->levels <= MPF_CORR_MAX_LEVELS, "%s: levels must be 1..%d (got %d)", who, MPF_CORR_MAX_LEVELS, a->levels);
    MPF_REQUIRE(a->B >= 1 && a->H >= 1 && a->W >= 1, "%s: bad shape B, H, W = %d, %d, %d", who, a->B, a->H, a->W);
    const int64_t lim = (int64_t)1 << 31;
    const int64_t NP = (int64_t)a->B * a->H * a->W;
    MPF_REQUIRE((int64_t)a->H * a->W < lim / 4 && NP < lim / 4, "%s: B * H * W too large", who);
    d = CvDev{};
    for (int i = 0; i < a->levels; ++i) {
        MPF_REQUIRE(a->level[i], "%s: null pointer (level[%d])", who, i);
        if (lookup)
            MPF_REQUIRE(((uintptr_t)a->level[i] & 3) == 0, "%s: level[%d] must be 4-byte aligned", who, i);
        else                                                 // level 0 moves as float4 where W allows; one rule for the whole pyramid
            MPF_REQUIRE(mpf_aligned16(a->level[i]), "%s: level[%d] must be 16-byte aligned", who, i);
        MPF_REQUIRE(a->Hl[i] == a->H >> i && a->Wl[i] == a->W >> i, "%s: Hl[%d] x Wl[%d] = %d x %d, a pooled pyramid of %d x %d has %d x %d there", who, i,
                    i, a->Hl[i], a->Wl[i], a->H, a->W, a->H >> i, a->W >> i);
        MPF_REQUIRE(a->Hl[i] >= 2 && a->Wl[i] >= 2, "%s: Hl[%d] x Wl[%d] = %d x %d: every level must be at least 2 x 2 (H, W >= 2^levels)", who, i, i,
                    a->Hl[i], a->Wl[i]);
        d.level[i] = a->level[i];
        d.Hl[i] = a->Hl[i];
        d.Wl[i] = a->Wl[i];
    }
    if (lookup) {
        MPF_REQUIRE(a->coords && a->out, "%s: null pointer (coords or out)", who);
        MPF_REQUIRE(a->radius >= 1 && a->radius <= 8, "%s: radius must be 1..8 (got %d)", who, a->radius);
        const int rd = 2 * a->radius + 1;
        MPF_REQUIRE(NP * a->levels * rd * rd < ((int64_t)1 << 40), "%s: output too large", who);
    } else {
        MPF_REQUIRE(a->norm == a->norm && a->norm - a->norm == 0.0f && a->norm != 0.0f, "%s: norm must be finite and not 0", who);
        MPF_REQUIRE(((int64_t)a->W << (a->levels - 1)) <= CV_MAX_STRIP, "%s: W * 2^(levels-1) must be at most %d (got %d, levels %d)", who, CV_MAX_STRIP,
                    a->W, a->levels);
        const int S = 1 << (a->levels - 1);
        MPF_REQUIRE(NP * ((a->H + S - 1) / S) < lim, "%s: B * H * W * H too large", who);
    }
    d.coords = a->coords;
    d.out = a->out;
    d.B = a->B, d.H = a->H, d.W = a->W;
    d.radius = a->radius, d.levels = a->levels, d.norm = a->norm;
    return 0;
}

extern "C" int mpf_corr_pyramid(const MpfCorrVolumeArgs *a, void *stream)
{
    CvDev d;
    const int rc = cv_check(a, false, "mpf_corr_pyramid", d);
    if (rc) return rc;
    const int S = 1 << (d.levels - 1), nstrips = (d.H + S - 1) / S;
    size_t lds = 0;
    for (int l = 0; l < d.levels; ++l) lds += (size_t)(S >> l) * d.Wl[l] * sizeof(float);     // <= 4/3 * 4 * CV_MAX_STRIP = 65,536 bytes
    const dim3 grid((unsigned)((int64_t)d.B * d.H * d.W * nstrips));
    if (d.W % 4 == 0)
        hipLaunchKernelGGL(k_cv_pyramid<true>, grid, dim3(CV_THREADS), lds, (hipStream_t)stream, d, nstrips);
    else
        hipLaunchKernelGGL(k_cv_pyramid<false>, grid, dim3(CV_THREADS), lds, (hipStream_t)stream, d, nstrips);
    return mpf_launch_status("k_cv_pyramid");
}

extern "C" int mpf_corr_pyramid_backward(const MpfCorrVolumeArgs *a, void *stream)
{
    CvDev d;
    const int rc = cv_check(a, false, "mpf_corr_pyramid_backward", d);
    if (rc) return rc;
    const int S = 1 << (d.levels - 1), nstrips = (d.H + S - 1) / S;
    const dim3 grid((unsigned)((int64_t)d.B * d.H * d.W * nstrips));
    if (d.W % 4 == 0)
        hipLaunchKernelGGL(k_cv_fold<true>, grid, dim3(CV_THREADS), 0, (hipStream_t)stream, d, nstrips);
    else
        hipLaunchKernelGGL(k_cv_fold<false>, grid, dim3(CV_THREADS), 0, (hipStream_t)stream, d, nstrips);
    return mpf_launch_status("k_cv_fold");
}

static size_t cv_tile_bytes(int ndata) { return ((size_t)ndata + 6 * CV_TILE) * sizeof(float); }      // <= 32 * 325 + 192 floats = 42,368 bytes

extern "C" int mpf_corr_volume_lookup(const MpfCorrVolumeArgs *a, void *stream)
{
    CvDev d;
    const int rc = cv_check(a, true, "mpf_corr_volume_lookup", d);
    if (rc) return rc;
    const int rd1 = 2 * d.radius + 2;
    const dim3 grid((unsigned)(((int64_t)d.B * d.H * d.W + CV_TILE - 1) / CV_TILE), (unsigned)d.levels);
    const size_t lds = cv_tile_bytes(CV_TILE * (rd1 * rd1 + 1));
    if (d.radius == 4)
        hipLaunchKernelGGL(k_cv_lookup<4>, grid, dim3(CV_THREADS), lds, (hipStream_t)stream, d);
    else
        hipLaunchKernelGGL(k_cv_lookup<0>, grid, dim3(CV_THREADS), lds, (hipStream_t)stream, d);
    return mpf_launch_status("k_cv_lookup");
}

extern "C" int mpf_corr_volume_lookup_backward(const MpfCorrVolumeArgs *a, void *stream)
{
    CvDev d;
    const int rc = cv_check(a, true, "mpf_corr_volume_lookup_backward", d);
    if (rc) return rc;
    const int rd = 2 * d.radius + 1;
    const dim3 grid((unsigned)(((int64_t)d.B * d.H * d.W + CV_TILE - 1) / CV_TILE), (unsigned)d.levels);
    const size_t lds = cv_tile_bytes(CV_TILE * rd * rd);
    if (d.radius == 4)
        hipLaunchKernelGGL(k_cv_lookup_backward<4>, grid, dim3(CV_THREADS), lds, (hipStream_t)stream, d);
    else
        hipLaunchKernelGGL(k_cv_lookup_backward<0>, grid, dim3(CV_THREADS), lds, (hipStream_t)stream, d);
    return mpf_launch_status("k_cv_lookup_backward");
}
