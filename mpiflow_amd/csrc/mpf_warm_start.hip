// mpf_warm_start.hip - RAFT's warm start for gfx950: forward_interpolate (RAFT/core/utils/utils.py) as an exact nearest-source search.
//
// Contract: include/mpiflow_hip.h (MpfWarmStartArgs).  Per sample, flow [2,h,w] = (dx, dy):
//   source   every pixel (x0, y0), flat index s = y0 * w + x0, at x1 = double(x0) + double(dx), y1 = double(y0) + double(dy); VALID iff
//            x1 > 0 && x1 < w && y1 > 0 && y1 < h (strict; NaN and +-inf fail the comparisons).
//   target   every pixel (gx, gy) takes (dx, dy) of the valid source with the least d2 = (x1 - gx) * (x1 - gx) + (y1 - gy) * (y1 - gy) in
//            f64, each product rounded, then the sum (__dmul_rn / __dadd_rn: never contracted); equal d2: the lowest s.  No valid source
//            at all: zeros.
//
// Brute force on purpose (the work is (h * w)^2 per sample):
// k_warm_partial   grid = (target tiles, source chunks, N), WARM_THREADS threads, one thread per target.  A chunk is `tiles_per_chunk`
//                  consecutive tiles of WARM_THREADS consecutive sources; a tile is staged in LDS as (x1, y1) doubles, thread j the source
//                  tile_base + j, so a source's flat index is its place in the tile and needs no storage.  An invalid source (and the
//                  tail past h * w) is staged as (+inf, 0): its d2 is +inf for every target, which the strict `<` below never takes, so
//                  the lowest-index rule holds over ORIGINAL flat indices without compaction.  Every lane of a wave reads the same LDS
//                  address (a broadcast, no bank conflict).  Sources are visited in ascending s and replaced only on d2 < best: the
//                  first minimum.  Each (target, chunk) writes its (d2, s) into the workspace.
// k_warm_fold      one thread per target: the lexicographic minimum of its chunks' (d2, s), then out = (dx, dy) of s, or zeros when the
//                  least d2 is +inf.  A minimum is order-independent: no atomics, bit-identical from run to run.
//
// The only value-dependent address is the fold's read of flow at s, and s < h * w by construction (it is a loop counter, not data).
// LDS: WARM_THREADS * 16 bytes = 4 KiB per workgroup.
#include "mpf_common.h"

#define WARM_THREADS 256
#define WARM_MAX_CHUNKS 32       // source chunks per sample: the workspace holds 12 bytes per (target, chunk)

struct WarmDev {
    const float *flow;           // [N,2,h,w]
    float *out;                  // [N,2,h,w]
    double *part_d2;             // [N][chunks][hw]
    int *part_idx;               // [N][chunks][hw]
    int w, h, hw;
    int chunks, tiles_per_chunk;
};

// h * w <= MPF_WARM_MAX_HW: the tiles of a sample, its chunks (at most WARM_MAX_CHUNKS, none empty) and the tiles of a chunk
static void warm_split(int hw, int &tiles, int &chunks, int &tiles_per_chunk)
{
    tiles = (hw + WARM_THREADS - 1) / WARM_THREADS;
    tiles_per_chunk = (tiles + WARM_MAX_CHUNKS - 1) / WARM_MAX_CHUNKS;
    chunks = (tiles + tiles_per_chunk - 1) / tiles_per_chunk;
}

__global__ __launch_bounds__(WARM_THREADS) void k_warm_partial(const WarmDev a)
{
    __shared__ double2 sSrc[WARM_THREADS];
    const int tid = threadIdx.x;
    const int n = blockIdx.z, chunk = blockIdx.y;
    const int t = blockIdx.x * WARM_THREADS + tid;                        // the target; t >= hw only stages sources
    const int ty = t / a.w;
    const double gx = (double)(t - ty * a.w), gy = (double)ty;
    const float *fx = a.flow + (size_t)n * 2 * a.hw, *fy = fx + a.hw;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double best = inf;
    int best_s = 0;
    const int tile0 = chunk * a.tiles_per_chunk;
    for (int tile = tile0; tile < tile0 + a.tiles_per_chunk; ++tile) {
        const int base = tile * WARM_THREADS;
        if (base >= a.hw) break;                                          // uniform over the workgroup
        const int s = base + tid;
        double2 src = make_double2(inf, 0.0);
        if (s < a.hw) {
            const int y0 = s / a.w, x0 = s - y0 * a.w;
            const double x1 = (double)x0 + (double)fx[s], y1 = (double)y0 + (double)fy[s];
            if (x1 > 0.0 && x1 < (double)a.w && y1 > 0.0 && y1 < (double)a.h) src = make_double2(x1, y1);
        }
        __syncthreads();                                                  // the previous tile has been read
        sSrc[tid] = src;
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < WARM_THREADS; ++j) {
            const double2 p = sSrc[j];
            const double ex = p.x - gx, ey = p.y - gy;
            const double d2 = __dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey));
            if (d2 < best) best = d2, best_s = base + j;
        }
    }
    if (t < a.hw) {
        const size_t o = ((size_t)n * a.chunks + chunk) * a.hw + t;
        a.part_d2[o] = best;
        a.part_idx[o] = best_s;
    }
}

__global__ __launch_bounds__(WARM_THREADS) void k_warm_fold(const WarmDev a)
{
    const int n = blockIdx.y;
    const int t = blockIdx.x * WARM_THREADS + threadIdx.x;
    if (t >= a.hw) return;                                                // no barrier below
    const size_t o = (size_t)n * a.chunks * a.hw + t;
    double best = a.part_d2[o];
    int best_s = a.part_idx[o];
    for (int c = 1; c < a.chunks; ++c) {
        const double d2 = a.part_d2[o + (size_t)c * a.hw];
        const int s = a.part_idx[o + (size_t)c * a.hw];
        if (d2 < best || (d2 == best && s < best_s)) best = d2, best_s = s;
    }
    const float *fx = a.flow + (size_t)n * 2 * a.hw, *fy = fx + a.hw;
    float *ox = a.out + (size_t)n * 2 * a.hw, *oy = ox + a.hw;
    const bool found = best < __longlong_as_double(0x7ff0000000000000ll);
    ox[t] = found ? fx[best_s] : 0.0f;
    oy[t] = found ? fy[best_s] : 0.0f;
}

static int warm_shape(int N, int h, int w, const char *who)
{
    MPF_REQUIRE(N >= 1 && h >= 1 && w >= 1, "%s: bad shape N, h, w = %d, %d, %d", who, N, h, w);
    MPF_REQUIRE((int64_t)h * w <= MPF_WARM_MAX_HW, "%s: bad shape: h * w must be at most %d, the work is quadratic in it (got h, w = %d, %d)", who,
                MPF_WARM_MAX_HW, h, w);
    MPF_REQUIRE(N <= 65535 && (int64_t)N * h * w <= MPF_WARM_MAX_NHW, "%s: bad shape: at most 65535 samples and N * h * w <= %d per call (got N, h, w = %d, %d, %d)",
                who, MPF_WARM_MAX_NHW, N, h, w);
    return 0;
}

static size_t warm_bytes(int N, int hw)
{
    int tiles, chunks, tpc;
    warm_split(hw, tiles, chunks, tpc);
    return ((size_t)N * chunks * hw * (sizeof(double) + sizeof(int)) + 7) & ~(size_t)7;   // a whole number of doubles
}

extern "C" size_t mpf_forward_interpolate_workspace(int N, int h, int w)
{
    if (warm_shape(N, h, w, "mpf_forward_interpolate_workspace")) return 0;
    return warm_bytes(N, h * w);
}

extern "C" int mpf_forward_interpolate(const MpfWarmStartArgs *a, void *stream)
{
    const char *who = "mpf_forward_interpolate";
    MPF_REQUIRE(a, "%s: null argument block", who);
    const int rc = warm_shape(a->N, a->h, a->w, who);
    if (rc) return rc;
    MPF_REQUIRE(a->flow && a->out, "%s: null pointer (flow or out)", who);
    const int hw = a->h * a->w;
    const size_t floats = (size_t)a->N * 2 * hw;
    MPF_REQUIRE(a->out + floats <= a->flow || a->flow + floats <= a->out, "%s: out must not overlap flow (a target reads sources anywhere in its sample)", who);
    MPF_REQUIRE(a->workspace, "%s: null pointer (workspace)", who);
    MPF_REQUIRE((((uintptr_t)a->workspace) & 7) == 0, "%s: workspace must be 8-byte aligned", who);
    const size_t need = warm_bytes(a->N, hw);
    MPF_REQUIRE(a->workspace_bytes >= need, "%s: workspace holds %zu bytes, %zu needed (mpf_forward_interpolate_workspace)", who, a->workspace_bytes, need);
    int tiles;
    WarmDev d = WarmDev{};
    warm_split(hw, tiles, d.chunks, d.tiles_per_chunk);
    d.flow = a->flow, d.out = a->out;
    d.part_d2 = (double *)a->workspace;
    d.part_idx = (int *)(d.part_d2 + (size_t)a->N * d.chunks * hw);
    d.w = a->w, d.h = a->h, d.hw = hw;
    hipLaunchKernelGGL(k_warm_partial, dim3((unsigned)tiles, (unsigned)d.chunks, (unsigned)a->N), dim3(WARM_THREADS), 0, (hipStream_t)stream, d);
    const int st = mpf_launch_status("k_warm_partial");
    if (st) return st;
    hipLaunchKernelGGL(k_warm_fold, dim3((unsigned)tiles, (unsigned)a->N), dim3(WARM_THREADS), 0, (hipStream_t)stream, d);
    return mpf_launch_status("k_warm_fold");
}
