// mpf_optim.hip - the optimizer tail of RAFT/train.py for gfx950: clip_grad_norm_ and torch's single-tensor AdamW over a whole parameter set as
// one multi-tensor path, two kernels and a finish kernel, no host synchronisation.
//
// Contract: include/mpiflow_hip.h (MpfOptTensor, MpfAdamWArgs).
//
// The tensor table is a HOST array.  The calls copy it, OPT_T = MPF_OPT_TENSORS_PER_LAUNCH records at a time and without the records whose grad
// is NULL, into an OptLaunch that is passed BY VALUE: a launch's pointers, sizes and the prefix of its tensors' chunk counts are kernel
// arguments.  A workgroup finds its (tensor, chunk) by a binary search of that prefix with its block index: uniform, so scalar loads of the
// argument segment; no device-resident table, nothing of the caller's that has to outlive the call.
//
// k_opt_sumsq          one workgroup per chunk of MPF_OPT_CHUNK elements: sum of g * g in fp64, one partial per workgroup.
// k_opt_norm_finish    one workgroup: the partials in a fixed order -> the sum, total_norm = (float) sqrt(sum), coef = min(1, max_norm /
//                      (total_norm + 1e-6f)) into the workspace's tail.  With n < 0 it takes the sum an earlier call left there.
// k_opt_adamw          one workgroup per chunk: g = coef * grad, the update, optional zeros to grad.
//
// A lane owns the same elements of a chunk on the vector path (whole chunk, pointers 16-byte aligned: 4 x 16 bytes per lane and array, every
// wave instruction 1 KiB contiguous) and on the scalar path (the last chunk of a tensor, or an offset view), and adds them in the same
// order: the norm does not depend on the alignment.  Streaming: 16 B read, 12 or 16 B written per element, nothing reused, so no LDS beyond
// the 32 bytes of the block reduction.  256 threads = 4 waves and 16 elements per lane: the 16 loads of k_opt_adamw are issued before the
// first use, which is what hides the latency here; its registers (see csrc/resource_usage.sh) leave 6 waves per SIMD.
//
// No address depends on a tensor's values.
#include <math.h>
#include "mpf_common.h"
#include "mpf_math.h"             // mpf_load_vec, mpf_store_vec
#include "mpf_reduce.h"

#define OPT_THREADS 256
#define OPT_WAVES 4
#define OPT_T MPF_OPT_TENSORS_PER_LAUNCH
#define OPT_VEC 4
#define OPT_ROUNDS (MPF_OPT_CHUNK / (OPT_THREADS * OPT_VEC))      // 16-byte accesses per lane and array
static_assert(OPT_ROUNDS * OPT_THREADS * OPT_VEC == MPF_OPT_CHUNK, "a chunk is a whole number of 16-byte rounds of the block");
static_assert(MPF_OPT_WORKSPACE_TAIL == 16, "OptTail");

struct OptTail {
    double sumsq;
    float norm, coef;
};

struct OptLaunch {
    MpfOptTensor t[OPT_T];
    unsigned first[OPT_T + 1];       // first[i]: the launch's first block of tensor i; first[count]: its grid
    int count;
    unsigned partial_base;           // k_opt_sumsq: the launch's first partial
    double *partials;
    OptTail *tail;
    float decay, w1, b2, w2, step_size, bc2_sqrt, eps;      // 1 - lr * wd, 1 - beta1, beta2, 1 - beta2, lr / bc1, sqrt(bc2), eps
    int zero_grad;
};
static_assert(sizeof(OptLaunch) <= 4096, "the launch record must fit the kernel argument segment");

// the tensor of block b: first[i] <= b < first[i + 1].  b is uniform, so are the loads
__device__ __forceinline__ int opt_find(const OptLaunch &a, unsigned b)
{
    int lo = 0, hi = a.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.first[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(OPT_THREADS) void k_opt_sumsq(const OptLaunch a)
{
    __shared__ double sW[OPT_WAVES];
    const int i = opt_find(a, blockIdx.x);
    const int64_t base = (int64_t)(blockIdx.x - a.first[i]) * MPF_OPT_CHUNK;
    const int64_t left = a.t[i].numel - base;
    const int n = left < MPF_OPT_CHUNK ? (int)left : MPF_OPT_CHUNK;
    const float *g = a.t[i].grad + base;
    float x[OPT_ROUNDS][OPT_VEC];
    if (n == MPF_OPT_CHUNK && mpf_aligned16(g)) {
#pragma unroll
        for (int r = 0; r < OPT_ROUNDS; ++r) mpf_load_vec<OPT_VEC>(g + (r * OPT_THREADS + (int)threadIdx.x) * OPT_VEC, x[r]);
    } else {
#pragma unroll
        for (int r = 0; r < OPT_ROUNDS; ++r)
#pragma unroll
            for (int e = 0; e < OPT_VEC; ++e) {
                const int k = (r * OPT_THREADS + (int)threadIdx.x) * OPT_VEC + e;
                x[r][e] = k < n ? g[k] : 0.0f;                            // + 0.0 leaves the sum as it is
            }
    }
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < OPT_ROUNDS; ++r)
#pragma unroll
        for (int e = 0; e < OPT_VEC; ++e) s += (double)x[r][e] * (double)x[r][e];
    const double part[1] = {s};
    mpf_block_sums<OPT_WAVES>(part, 1, sW, a.partials + a.partial_base + blockIdx.x);
}

// one workgroup: lane t adds partials t, t + 256, ... in that order, then the tree: a fixed order
__global__ __launch_bounds__(OPT_THREADS) void k_opt_norm_finish(const double *partials, int n, OptTail *tail, float max_norm, float *total_norm)
{
    __shared__ double sR[OPT_THREADS];
    if (n >= 0) {
        double v = 0.0;
        for (int b = threadIdx.x; b < n; b += OPT_THREADS) v += partials[b];
        mpf_block_tree_sum<OPT_THREADS>(v, sR);
    }
    if (threadIdx.x == 0) {
        const double sum = n >= 0 ? sR[0] : tail->sumsq;
        const float norm = (float)sqrt(sum);
        const float c = max_norm / (norm + 1e-6f);
        tail->sumsq = sum;
        tail->norm = norm;
        tail->coef = c > 1.0f ? 1.0f : c;                                 // clamp(max=1): a NaN stays a NaN
        *total_norm = norm;
    }
}

__global__ __launch_bounds__(OPT_THREADS) void k_opt_adamw(const OptLaunch a)
{
    const int i = opt_find(a, blockIdx.x);
    const int64_t base = (int64_t)(blockIdx.x - a.first[i]) * MPF_OPT_CHUNK;
    const int64_t left = a.t[i].numel - base;
    const int n = left < MPF_OPT_CHUNK ? (int)left : MPF_OPT_CHUNK;
    float *pp = a.t[i].param + base, *pm = a.t[i].exp_avg + base, *pv = a.t[i].exp_avg_sq + base, *pg = a.t[i].grad + base;
    const float coef = a.tail->coef;
    const bool vec = n == MPF_OPT_CHUNK && mpf_aligned16(pp) && mpf_aligned16(pm) && mpf_aligned16(pv) && mpf_aligned16(pg);
    float p[OPT_ROUNDS][OPT_VEC], m[OPT_ROUNDS][OPT_VEC], v[OPT_ROUNDS][OPT_VEC], g[OPT_ROUNDS][OPT_VEC];
    if (vec) {
#pragma unroll
        for (int r = 0; r < OPT_ROUNDS; ++r) {
            const int k = (r * OPT_THREADS + (int)threadIdx.x) * OPT_VEC;
            mpf_load_vec<OPT_VEC>(pg + k, g[r]);
            mpf_load_vec<OPT_VEC>(pp + k, p[r]);
            mpf_load_vec<OPT_VEC>(pm + k, m[r]);
            mpf_load_vec<OPT_VEC>(pv + k, v[r]);
        }
    } else {
#pragma unroll
        for (int r = 0; r < OPT_ROUNDS; ++r)
#pragma unroll
            for (int e = 0; e < OPT_VEC; ++e) {
                const int k = (r * OPT_THREADS + (int)threadIdx.x) * OPT_VEC + e;
                const bool in = k < n;
                g[r][e] = in ? pg[k] : 0.0f, p[r][e] = in ? pp[k] : 0.0f, m[r][e] = in ? pm[k] : 0.0f, v[r][e] = in ? pv[k] : 0.0f;
            }
    }
#pragma unroll
    for (int r = 0; r < OPT_ROUNDS; ++r)
#pragma unroll
        for (int e = 0; e < OPT_VEC; ++e) {
            const float gc = coef * g[r][e];
            const float pd = p[r][e] * a.decay;
            const float mn = m[r][e] + a.w1 * (gc - m[r][e]);
            const float vn = a.b2 * v[r][e] + (a.w2 * gc) * gc;
            const float denom = sqrtf(vn) / a.bc2_sqrt + a.eps;
            p[r][e] = pd - (a.step_size * mn) / denom;
            m[r][e] = mn, v[r][e] = vn, g[r][e] = 0.0f;
        }
    if (vec) {
#pragma unroll
        for (int r = 0; r < OPT_ROUNDS; ++r) {
            const int k = (r * OPT_THREADS + (int)threadIdx.x) * OPT_VEC;
            mpf_store_vec<OPT_VEC>(pp + k, p[r]);
            mpf_store_vec<OPT_VEC>(pm + k, m[r]);
            mpf_store_vec<OPT_VEC>(pv + k, v[r]);
            if (a.zero_grad) mpf_store_vec<OPT_VEC>(pg + k, g[r]);
        }
    } else {
#pragma unroll
        for (int r = 0; r < OPT_ROUNDS; ++r)
#pragma unroll
            for (int e = 0; e < OPT_VEC; ++e) {
                const int k = (r * OPT_THREADS + (int)threadIdx.x) * OPT_VEC + e;
                if (k < n) {
                    pp[k] = p[r][e], pm[k] = m[r][e], pv[k] = v[r][e];
                    if (a.zero_grad) pg[k] = 0.0f;
                }
            }
    }
}

static int64_t opt_chunks(int64_t numel) { return (numel + MPF_OPT_CHUNK - 1) / MPF_OPT_CHUNK; }

// the table's sizes: count >= 1, every numel >= 1, at most MPF_OPT_MAX_CHUNKS chunks over ALL records (what the workspace is sized by)
static int opt_table(const MpfOptTensor *t, int count, const char *who, int64_t &chunks)
{
    MPF_REQUIRE(t, "%s: null pointer (tensors)", who);
    MPF_REQUIRE(count >= 1, "%s: count must be at least 1 (got %d)", who, count);
    chunks = 0;
    for (int i = 0; i < count; ++i) {
        MPF_REQUIRE(t[i].numel >= 1, "%s: tensors[%d].numel must be at least 1 (got %lld)", who, i, (long long)t[i].numel);
        MPF_REQUIRE(t[i].numel <= (int64_t)MPF_OPT_MAX_CHUNKS * MPF_OPT_CHUNK, "%s: too many chunks: tensors[%d] alone has more than %d (numel = %lld)", who, i,
                    MPF_OPT_MAX_CHUNKS, (long long)t[i].numel);
        chunks += opt_chunks(t[i].numel);
        MPF_REQUIRE(chunks <= MPF_OPT_MAX_CHUNKS, "%s: too many chunks: the table has more than %d chunks of %d elements (reached at tensors[%d])", who,
                    MPF_OPT_MAX_CHUNKS, MPF_OPT_CHUNK, i);
    }
    return 0;
}

extern "C" size_t mpf_adamw_workspace(const MpfOptTensor *tensors, int count)
{
    int64_t chunks;
    if (opt_table(tensors, count, "mpf_adamw_workspace", chunks)) return 0;
    return MPF_OPT_WORKSPACE_TAIL + (size_t)chunks * sizeof(double);
}

static bool opt_aligned4(const void *p) { return (((uintptr_t)p) & 3) == 0; }

// everything both calls refuse, before anything is launched; `update`: mpf_adamw_clipped, which also touches param and the moments
static int opt_check(const MpfAdamWArgs *a, const char *who, bool update)
{
    MPF_REQUIRE(a, "%s: null argument block", who);
    int64_t chunks;
    const int rc = opt_table(a->tensors, a->count, who, chunks);
    if (rc) return rc;
    for (int i = 0; i < a->count; ++i) {
        const MpfOptTensor &t = a->tensors[i];
        if (!t.grad) continue;
        MPF_REQUIRE(!update || (t.param && t.exp_avg && t.exp_avg_sq), "%s: null pointer (param, exp_avg or exp_avg_sq of tensors[%d], which has a grad)", who, i);
        MPF_REQUIRE(opt_aligned4(t.grad) && (!update || (opt_aligned4(t.param) && opt_aligned4(t.exp_avg) && opt_aligned4(t.exp_avg_sq))),
                    "%s: the pointers of tensors[%d] must be 4-byte aligned", who, i);
    }
    MPF_REQUIRE(a->total_norm, "%s: null pointer (total_norm)", who);
    MPF_REQUIRE(a->workspace, "%s: null pointer (workspace)", who);
    MPF_REQUIRE((((uintptr_t)a->workspace) & 7) == 0, "%s: workspace must be 8-byte aligned", who);
    const bool ready = update && a->norm_ready;
    const size_t need = MPF_OPT_WORKSPACE_TAIL + (ready ? 0 : (size_t)chunks * sizeof(double));
    MPF_REQUIRE(a->workspace_bytes >= need, "%s: workspace holds %zu bytes, %zu needed (mpf_adamw_workspace)", who, a->workspace_bytes, need);
    if (!update) return 0;
    MPF_REQUIRE(a->zero_grad == 0 || a->zero_grad == 1, "%s: zero_grad must be 0 or 1 (got %d)", who, a->zero_grad);
    MPF_REQUIRE(a->norm_ready == 0 || a->norm_ready == 1, "%s: norm_ready must be 0 or 1 (got %d)", who, a->norm_ready);
    MPF_REQUIRE(isfinite(a->lr) && isfinite(a->beta1) && isfinite(a->beta2) && isfinite(a->eps) && isfinite(a->weight_decay) && isfinite(a->bias_correction1) &&
                    isfinite(a->bias_correction2_sqrt),
                "%s: non-finite hyperparameter (lr, beta1, beta2, eps, weight_decay = %g, %g, %g, %g, %g; bias corrections %g, %g)", who, a->lr, a->beta1,
                a->beta2, a->eps, a->weight_decay, a->bias_correction1, a->bias_correction2_sqrt);
    MPF_REQUIRE(a->lr >= 0.0, "%s: lr must not be negative (got %g)", who, a->lr);
    MPF_REQUIRE(a->eps > 0.0 && (float)a->eps > 0.0f, "%s: eps must be positive, in float32 too (got %g)", who, a->eps);
    MPF_REQUIRE(a->weight_decay >= 0.0, "%s: weight_decay must not be negative (got %g)", who, a->weight_decay);
    MPF_REQUIRE(a->beta1 >= 0.0 && a->beta1 < 1.0 && a->beta2 >= 0.0 && a->beta2 < 1.0, "%s: the betas must lie in [0, 1) (got %g, %g)", who, a->beta1, a->beta2);
    MPF_REQUIRE(a->bias_correction1 > 0.0 && a->bias_correction1 <= 1.0 && a->bias_correction2_sqrt > 0.0 && a->bias_correction2_sqrt <= 1.0,
                "%s: the bias corrections 1 - beta1^t and sqrt(1 - beta2^t) must lie in (0, 1] (got %g, %g)", who, a->bias_correction1, a->bias_correction2_sqrt);
    MPF_REQUIRE(a->max_norm > 0.0 && (float)a->max_norm > 0.0f, "%s: max_norm must be positive, in float32 too; +inf for no clipping (got %g)", who,
                a->max_norm);                                              // a NaN fails the comparison
    return 0;
}

// the table, without the records that have no grad, OPT_T records per launch.  pass 1: k_opt_sumsq, 2: k_opt_adamw.  -> the chunks launched
static int opt_launches(const MpfAdamWArgs *a, OptLaunch &L, int pass, hipStream_t stream, unsigned &launched)
{
    launched = 0;
    int i = 0;
    while (i < a->count) {
        L.count = 0;
        L.first[0] = 0;
        for (; i < a->count && L.count < OPT_T; ++i) {
            if (!a->tensors[i].grad) continue;
            L.t[L.count] = a->tensors[i];
            L.first[L.count + 1] = L.first[L.count] + (unsigned)opt_chunks(a->tensors[i].numel);
            ++L.count;
        }
        if (!L.count) break;
        for (int k = L.count + 1; k <= OPT_T; ++k) L.first[k] = L.first[L.count];
        L.partial_base = launched;
        const unsigned grid = L.first[L.count];
        if (pass == 1) hipLaunchKernelGGL(k_opt_sumsq, dim3(grid), dim3(OPT_THREADS), 0, stream, L);
        else hipLaunchKernelGGL(k_opt_adamw, dim3(grid), dim3(OPT_THREADS), 0, stream, L);
        const int st = mpf_launch_status(pass == 1 ? "k_opt_sumsq" : "k_opt_adamw");
        if (st) return st;
        launched += grid;
    }
    return 0;
}

static int opt_norm(const MpfAdamWArgs *a, OptLaunch &L, float max_norm, bool ready, hipStream_t stream)
{
    unsigned n = 0;
    if (!ready) {
        const int st = opt_launches(a, L, 1, stream, n);
        if (st) return st;
    }
    hipLaunchKernelGGL(k_opt_norm_finish, dim3(1), dim3(OPT_THREADS), 0, stream, (const double *)L.partials, ready ? -1 : (int)n, L.tail, max_norm, a->total_norm);
    return mpf_launch_status("k_opt_norm_finish");
}

static void opt_workspace(const MpfAdamWArgs *a, OptLaunch &L)
{
    L = OptLaunch{};
    L.tail = (OptTail *)a->workspace;
    L.partials = (double *)((char *)a->workspace + MPF_OPT_WORKSPACE_TAIL);
}

extern "C" int mpf_grad_norm(const MpfAdamWArgs *a, void *stream)
{
    const int rc = opt_check(a, "mpf_grad_norm", false);
    if (rc) return rc;
    OptLaunch L;
    opt_workspace(a, L);
    return opt_norm(a, L, INFINITY, false, (hipStream_t)stream);
}

extern "C" int mpf_adamw_clipped(const MpfAdamWArgs *a, void *stream)
{
    const int rc = opt_check(a, "mpf_adamw_clipped", true);
    if (rc) return rc;
    OptLaunch L;
    opt_workspace(a, L);
    const int st = opt_norm(a, L, (float)a->max_norm, a->norm_ready != 0, (hipStream_t)stream);
    if (st) return st;
    L.decay = (float)(1.0 - a->lr * a->weight_decay);
    L.w1 = (float)(1.0 - a->beta1);
    L.b2 = (float)a->beta2;
    L.w2 = (float)(1.0 - a->beta2);
    L.step_size = (float)(a->lr / a->bias_correction1);
    L.bc2_sqrt = (float)a->bias_correction2_sqrt;
    L.eps = (float)a->eps;
    L.zero_grad = a->zero_grad;
    unsigned n;
    return opt_launches(a, L, 2, (hipStream_t)stream, n);
}
