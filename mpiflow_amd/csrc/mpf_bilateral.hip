// mpf_bilateral.hip - 3d-photo-inpainting's sparse bilateral filter (the reference's bilateral_filter.py) for gfx950: a 0/1-weighted median
// around disparity discontinuities, iterated, on the stream, for a batch.  The output is a SELECTION of input values, so it equals the
// reference's bit for bit.
//
// Contract: include/mpiflow_hip.h (MpfBilateralArgs); INTEGRATION.md section 18 holds the definition, which tests/bilateral_restated.py
// restates in numpy.  The build has no contraction and correctly rounded divides, which the discontinuity map relies on.
//
// Two launches per iteration, both one thread per pixel:
// k_bil_map      D [B,h,w] u8: 1 where one of the four differences of 1 / v to a neighbour exceeds the threshold (interior pixels, under the
//                mask's products), or where the ORIGINAL input is 0; 0 where the mask is 0.
// k_bil_select   a 32 x 8 tile per workgroup.  The tile and its halo of m = ws / 2 are staged in LDS once: the key of every position (its
//                value of v', or a marker that compares false where the position is not a valid sample: D' set or mask 0) and its D'.
//                v' and D' are v and D with the outermost ring replaced by its inner neighbour and then edge-padded, which is ONE clamp of
//                the index to [1, h - 2] x [1, w - 2]; the mask is zero outside the image.  A pixel whose mask is 0 or whose window holds
//                no D' stores v' (most pixels of a real disparity).  Another counts the n valid samples of its window and takes the
//                k*(n)-th smallest by rank counting out of LDS: for a candidate c, lt = #{valid < c} and le = #{valid <= c}; c is the
//                answer when lt < k <= le.  No per-thread array, so no scratch; the first candidate that fits ends the search, and tied
//                candidates are equal values.  LDS: 640 keys (5 KiB for f64) + 640 + 82 bytes.
// The map is a launch of its own and not recomputed from the tile because it reads what the selection must not see: the ring of v before
// its replacement and the original input (the zero rule); it costs one byte written and read per pixel.
// k*(n) = 1 + #{k <= n : S_k <= 0.5}, S_k the f32 sum of k copies of fl32(1 / n) added one at a time (numpy's normalise, cumsum, digitize):
// bil_rank below, compiled for the device (a table in LDS per workgroup) and for the host (mpf_sparse_bilateral_rank, which a test reads).
//
// No atomics, no workgroup waits for another, every loop is bounded by the window, and no address depends on a tensor's value.
#include "mpf_common.h"
#include <math.h>

#define BL_TW 32
#define BL_TH 8
#define BL_THREADS (BL_TW * BL_TH)
#define BL_MAX_M (MPF_BILATERAL_MAX_WINDOW / 2)
#define BL_LDS ((BL_TW + 2 * BL_MAX_M) * (BL_TH + 2 * BL_MAX_M))
#define BL_MAX_N (MPF_BILATERAL_MAX_WINDOW * MPF_BILATERAL_MAX_WINDOW)

__host__ __device__ static inline int bil_rank(int n)
{
    const float c = 1.0f / (float)n;
    float s = 0.0f;
    int k = 1;
    for (int j = 0; j < n; ++j) {
        s = s + c;
        if (s <= 0.5f) ++k;
    }
    return k;
}

// S: the stored type; T: the type the map's arithmetic runs in; K: the key in LDS, with a marker no value equals and every comparison refuses
template <typename S> struct BilType;
template <> struct BilType<float> {
    typedef float T;
    typedef float K;
    __device__ static T value(float s) { return s; }
    __device__ static K invalid() { return __builtin_nanf(""); }
    __device__ static bool is_valid(K k) { return k == k; }
};
template <> struct BilType<double> {
    typedef double T;
    typedef double K;
    __device__ static T value(double s) { return s; }
    __device__ static K invalid() { return __builtin_nan(""); }
    __device__ static bool is_valid(K k) { return k == k; }
};
template <> struct BilType<unsigned char> {                     // u / 255.0 in f64, as cv2.imread(path, 0) / 255; ordered as the bytes are
    typedef double T;
    typedef short K;
    __device__ static T value(unsigned char s) { return (double)s / 255.0; }
    __device__ static K invalid() { return 32767; }
    __device__ static bool is_valid(K k) { return k != 32767; }
};

template <typename S> struct BilDev {
    const S *orig, *v;                 // [B,h,w]: the call's input (the zero rule) and this iteration's input
    S *out;                            // [B,h,w]
    unsigned char *D;                  // [B,h,w]
    const unsigned char *mask;         // [h,w] per image, mask_stride apart, or NULL
    size_t mask_stride;
    int h, w, hw, m, tiles_x;
    typename BilType<S>::T thr;
};

template <typename S>
__global__ __launch_bounds__(BL_THREADS) void k_bil_map(const BilDev<S> a)
{
    typedef typename BilType<S>::T T;
    const int p = blockIdx.x * BL_THREADS + threadIdx.x;
    if (p >= a.hw) return;
    const int y = p / a.w, x = p - y * a.w;
    const size_t plane = (size_t)blockIdx.y * a.hw;
    const S *v = a.v + plane;
    const unsigned char *mk = a.mask ? a.mask + (size_t)blockIdx.y * a.mask_stride : nullptr;
    bool d = false;
    if (y >= 1 && y <= a.h - 2 && x >= 1 && x <= a.w - 2) {
        const T one = (T)1;
        const T c = one / BilType<S>::value(v[p]);
        const int q[4] = {p - a.w, p + a.w, p - 1, p + 1};                  // unrolled: registers
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const T diff = c - one / BilType<S>::value(v[q[i]]);            // inf and NaN take their course: NaN > thr is false
            const bool both = !mk || (mk[p] != 0 && mk[q[i]] != 0);          // diff * 0 is 0 or NaN: never over
            d = d || (both && fabs(diff) > a.thr);
        }
    }
    if (BilType<S>::value(a.orig[plane + p]) == (T)0) d = true;
    if (mk && mk[p] == 0) d = false;
    a.D[plane + p] = d ? 1 : 0;
}

template <typename S>
__global__ __launch_bounds__(BL_THREADS) void k_bil_select(const BilDev<S> a)
{
    typedef typename BilType<S>::K K;
    __shared__ K sKey[BL_LDS];
    __shared__ unsigned char sD[BL_LDS];
    __shared__ unsigned char sRank[BL_MAX_N + 1];
    const int m = a.m, ws = 2 * m + 1, IW = BL_TW + 2 * m, IH = BL_TH + 2 * m;
    const int tyi = blockIdx.x / a.tiles_x, txi = blockIdx.x - tyi * a.tiles_x;
    const int x0 = txi * BL_TW, y0 = tyi * BL_TH;
    const size_t plane = (size_t)blockIdx.y * a.hw;
    const S *v = a.v + plane;
    const unsigned char *D = a.D + plane;
    const unsigned char *mk = a.mask ? a.mask + (size_t)blockIdx.y * a.mask_stride : nullptr;
    if (threadIdx.x >= 1 && threadIdx.x <= ws * ws) sRank[threadIdx.x] = (unsigned char)bil_rank((int)threadIdx.x);
    for (int i = threadIdx.x; i < IH * IW; i += BL_THREADS) {
        const int yy = i / IW, xx = i - yy * IW;
        const int gy = y0 - m + yy, gx = x0 - m + xx;
        const int cy = gy < 1 ? 1 : (gy > a.h - 2 ? a.h - 2 : gy);          // the ring replaced, then edge-padded: one clamp (h, w >= 3)
        const int cx = gx < 1 ? 1 : (gx > a.w - 2 ? a.w - 2 : gx);
        const int o = cy * a.w + cx;
        const bool in = gy >= 0 && gy < a.h && gx >= 0 && gx < a.w;
        const bool inside = mk ? (in && mk[gy * a.w + gx] != 0) : true;     // the mask is zero-padded and NOT ring-replaced
        const unsigned char d = D[o];
        sD[i] = d;
        sKey[i] = (d == 0 && inside) ? (K)v[o] : BilType<S>::invalid();
    }
    __syncthreads();
    const int ty = threadIdx.x / BL_TW, tx = threadIdx.x - ty * BL_TW;
    const int gy = y0 + ty, gx = x0 + tx;
    if (gy >= a.h || gx >= a.w) return;                                     // no barrier below
    const int cy = gy < 1 ? 1 : (gy > a.h - 2 ? a.h - 2 : gy), cx = gx < 1 ? 1 : (gx > a.w - 2 ? a.w - 2 : gx);
    S result = v[cy * a.w + cx];                                            // the iteration's output starts as v'
    const int base = ty * IW + tx;                                          // the window's first position in the tile
    bool active = !mk || mk[gy * a.w + gx] != 0;
    if (active) {
        int any = 0, n = 0;
        for (int r = 0; r < ws; ++r)
            for (int c = 0; c < ws; ++c) {
                any |= sD[base + r * IW + c];
                n += BilType<S>::is_valid(sKey[base + r * IW + c]) ? 1 : 0;
            }
        if (any && n > 0) {                                                 // n == 0: the window's centre of v', which result holds
            const int k = sRank[n];
            bool found = false;
            for (int r = 0; r < ws && !found; ++r)
                for (int c = 0; c < ws && !found; ++c) {
                    const K cand = sKey[base + r * IW + c];
                    if (!BilType<S>::is_valid(cand)) continue;
                    int lt = 0, le = 0;
                    for (int rr = 0; rr < ws; ++rr)
                        for (int cc = 0; cc < ws; ++cc) {
                            const K o = sKey[base + rr * IW + cc];           // the marker compares false both ways
                            lt += o < cand ? 1 : 0;
                            le += o <= cand ? 1 : 0;
                        }
                    if (lt < k && k <= le) result = (S)cand, found = true;
                }
        }
    }
    a.out[plane + (size_t)gy * a.w + gx] = result;
}

// ---------------------------------------------------------------- launcher

static size_t bil_elem(int dtype) { return dtype == MPF_BILATERAL_F32 ? 4 : dtype == MPF_BILATERAL_F64 ? 8 : 1; }
static size_t bil_buf_bytes(int dtype, int B, int h, int w) { return ((size_t)B * h * w * bil_elem(dtype) + 15) & ~(size_t)15; }

static int bil_shape(int dtype, int B, int h, int w, const char *who)
{
    MPF_REQUIRE(dtype == MPF_BILATERAL_F32 || dtype == MPF_BILATERAL_F64 || dtype == MPF_BILATERAL_U8, "%s: dtype must be 0 (f32), 1 (f64) or 2 (u8) (got %d)", who, dtype);
    MPF_REQUIRE(B >= 1 && B <= 65535, "%s: bad shape: B must be 1..65535 (got %d)", who, B);
    MPF_REQUIRE(h >= 3 && w >= 3, "%s: bad shape: h, w must be at least 3 (got h, w = %d, %d)", who, h, w);
    MPF_REQUIRE((int64_t)B * h * w <= MPF_BILATERAL_MAX_BHW, "%s: bad shape: B * h * w must be at most %d (got B, h, w = %d, %d, %d)", who, MPF_BILATERAL_MAX_BHW, B, h, w);
    return 0;
}

extern "C" int mpf_sparse_bilateral_rank(int n)
{
    if (n < 1 || n > BL_MAX_N) return 0;
    return bil_rank(n);
}

extern "C" size_t mpf_sparse_bilateral_workspace(int dtype, int B, int h, int w)
{
    if (bil_shape(dtype, B, h, w, "mpf_sparse_bilateral_workspace")) return 0;
    return 2 * bil_buf_bytes(dtype, B, h, w) + (size_t)B * h * w;
}

static bool bil_overlap(const void *p, size_t pn, const void *q, size_t qn)
{
    const char *a = (const char *)p, *b = (const char *)q;
    return a && b && a < b + qn && b < a + pn;
}

template <typename S>
static int bil_run(const MpfBilateralArgs *a, hipStream_t stream)
{
    typedef typename BilType<S>::T T;
    char *ws = (char *)a->workspace;
    const size_t buf = bil_buf_bytes(a->dtype, a->B, a->h, a->w);
    S *pong[2] = {(S *)ws, (S *)(ws + buf)};
    BilDev<S> d = BilDev<S>{};
    d.orig = (const S *)a->depth, d.D = (unsigned char *)(ws + 2 * buf);
    d.mask = a->mask, d.mask_stride = a->mask_shared ? 0 : (size_t)a->h * a->w;
    d.h = a->h, d.w = a->w, d.hw = a->h * a->w, d.tiles_x = (a->w + BL_TW - 1) / BL_TW;
    d.thr = (T)a->depth_threshold;                                          // f32 for f32 values: the threshold rounded once
    const dim3 pixels((unsigned)((d.hw + BL_THREADS - 1) / BL_THREADS), (unsigned)a->B);
    const dim3 tiles((unsigned)(d.tiles_x * ((a->h + BL_TH - 1) / BL_TH)), (unsigned)a->B);
    const S *cur = d.orig;
    for (int i = 0; i < a->num_iter; ++i) {
        d.v = cur, d.out = i == a->num_iter - 1 ? (S *)a->out : pong[i & 1], d.m = a->filter_size[i] / 2;
        hipLaunchKernelGGL(k_bil_map<S>, pixels, dim3(BL_THREADS), 0, stream, d);
        int st = mpf_launch_status("k_bil_map");
        if (st) return st;
        hipLaunchKernelGGL(k_bil_select<S>, tiles, dim3(BL_THREADS), 0, stream, d);
        st = mpf_launch_status("k_bil_select");
        if (st) return st;
        cur = d.out;
    }
    return 0;
}

extern "C" int mpf_sparse_bilateral(const MpfBilateralArgs *a, void *stream)
{
    const char *who = "mpf_sparse_bilateral";
    MPF_REQUIRE(a, "%s: null argument block", who);
    const int rc = bil_shape(a->dtype, a->B, a->h, a->w, who);
    if (rc) return rc;
    MPF_REQUIRE(a->num_iter >= 1 && a->num_iter <= MPF_BILATERAL_MAX_ITER, "%s: num_iter must be 1..%d (got %d)", who, MPF_BILATERAL_MAX_ITER, a->num_iter);
    for (int i = 0; i < a->num_iter; ++i) {
        const int ws = a->filter_size[i];
        MPF_REQUIRE(ws >= 3 && ws <= MPF_BILATERAL_MAX_WINDOW && (ws & 1), "%s: filter_size[%d] must be 3, 5, 7 or 9 (got %d)", who, i, ws);
    }
    MPF_REQUIRE(a->depth_threshold == a->depth_threshold, "%s: depth_threshold must not be NaN", who);
    MPF_REQUIRE(a->depth && a->out, "%s: null pointer (depth, out)", who);
    MPF_REQUIRE(a->workspace, "%s: null pointer (workspace)", who);
    MPF_REQUIRE((((uintptr_t)a->workspace) & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    const size_t need = mpf_sparse_bilateral_workspace(a->dtype, a->B, a->h, a->w);
    MPF_REQUIRE(a->workspace_bytes >= need, "%s: workspace holds %zu bytes, %zu needed (mpf_sparse_bilateral_workspace)", who, a->workspace_bytes, need);
    const size_t nb = (size_t)a->B * a->h * a->w * bil_elem(a->dtype);
    const size_t mb = (size_t)(a->mask_shared ? 1 : a->B) * a->h * a->w;
    MPF_REQUIRE(!bil_overlap(a->out, nb, a->depth, nb) && !bil_overlap(a->out, nb, a->mask, mb) && !bil_overlap(a->out, nb, a->workspace, need) &&
                !bil_overlap(a->depth, nb, a->workspace, need) && !bil_overlap(a->mask, mb, a->workspace, need),
                "%s: out and the workspace must not overlap depth, mask or each other (a pixel reads its neighbours)", who);
    if (a->dtype == MPF_BILATERAL_F32) return bil_run<float>(a, (hipStream_t)stream);
    if (a->dtype == MPF_BILATERAL_F64) return bil_run<double>(a, (hipStream_t)stream);
    return bil_run<unsigned char>(a, (hipStream_t)stream);
}
