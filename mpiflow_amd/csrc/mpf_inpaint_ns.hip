// mpf_inpaint_ns.hip - the reference's hole fill, cv2.inpaint(frame_mix, fill_mask, 3, cv2.INPAINT_NS) (utils/utils.py:284-286), on the
// GPU: the same bytes as mpf_inpaint_host's NS branch (mpf_inpaint.hip, fill<3>), for a batch of frames, stream-ordered.
//
// Why a sequential front can run on the device.  Filling ext pixel p (NS) reads the T values and flags of p's 4-neighbours
// (arrival) and, for each offset (k,l) of the radius-`range` disc around p, the flag of (k,l), the flags of its 4-neighbours and
// the colours at (k,l) and its +-1 neighbours along rows and columns (OpenCV's edge-clamped km / kp / lm / lp stay within one
// pixel of (k,l)).  Every read lies within Chebyshev distance range + 1 of p.  LINK two hole pixels of a frame when they lie
// within that distance of each other (D_LINK = range + 1 below) and call the connected components clusters.  Then
//   1. a band pixel is 4-adjacent to hole pixels of one cluster only (two holes sharing a band pixel are at most 2 apart);
//   2. one cluster's fills never read a pixel another cluster writes (a pixel within range + 1 of a hole of A that is a hole of B
//      would link A and B);
//   3. the front queue orders by (T, push sequence); a cluster's items get their T from the cluster's own data and are pushed in
//      the same relative order with or without the other clusters, so its pops come in the order of a run of the cluster alone.
// Hence the unchanged serial algorithm run on every cluster independently gives the whole-frame result byte for byte
// (tests/test_inpaint_ns.py checks the decomposition on the host, and that linking at distance `range` is NOT enough).  A larger
// link distance only merges clusters and would be correct too.
//
// Kernels (one stream, no host round trip, no allocation):
//   k_ns_init   flags (INSIDE / not), T (0 on the band, 1e6 elsewhere), union-find parents, out = img
//   k_ns_link   union-find over hole pixels within D_LINK; roots hang under the smaller index, so every cluster's root is its
//               minimum ext raster index (deterministic)
//   k_ns_roots  flattening (parent = root: cluster membership from here on); every root appends itself to the cluster list
//   k_ns_box    the bounding box of every cluster (atomics from the pixels on its 4-boundary only)
//   k_ns_fill   persistent one-wave workgroups take clusters from an atomic counter.  Per cluster: its band pixels pushed in raster
//               order, then the serial front of fill<3>'s NS branch.  The front logic is wave-uniform (every lane computes and
//               stores the same values, so each lane reads its own writes); lane o evaluates disc offset o, and the sums Ia / sw
//               fold over the offsets in disc raster order from lane 0 upwards (readlane, not a tree).  The heap lives in LDS and
//               moves to the cluster's region of a global pool if it outgrows it.  The order in which clusters run does not
//               change a byte: clusters share no pixel they write.
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include "mpf_common.h"

namespace {

enum : uint8_t { NS_KNOWN = 0, NS_INSIDE = 2 };        // fill<3>'s f: only "INSIDE or not" is ever tested
constexpr int NS_MAX_RANGE = 4;                        // disc of at most 49 offsets: one per lane of a 64-wide wave
constexpr int NS_WAVE = 64;
constexpr int NS_LDS_HEAP = 2048;                      // front items held in LDS (32 KB) before a cluster's heap spills to its pool region
constexpr int NS_FILL_BLOCKS_PER_CU = 4;

// the workspace's first words, readable after the call (mpiflow_hip.h): what the call did, and whether an internal bound broke
enum NsCounter { NS_CLUSTERS = 0, NS_WORK = 1, NS_POOL_ITEMS = 2, NS_SPILLED_AT_START = 3, NS_SPILLED_RUNNING = 4, NS_FAILED = 5, NS_PHASE_WORD = 16, NS_COUNTER_WORDS = 64 };

// witness build only: shader clocks per phase of the fill, summed over the waves, as 64-bit words from word NS_PHASE_WORD of the workspace
// (tools/bench_inpaint_ns.py --phases).  A phase ends at the clock read after its last instruction; a load it issued but did not
// wait for is charged to the phase that waits for it.
enum NsPhase { NSP_SETUP = 0, NSP_POP, NSP_REJECT, NSP_ARRIVAL, NSP_DISC, NSP_FOLD, NSP_PUSH, NSP_FILLS, NSP_POPS, NSP_N };
#ifdef MPF_WITNESS
#define NS_CLOCK(v) const uint64_t v = clock64()
#define NS_ADD(k, v) (ph[k] += (v))
#else
#define NS_CLOCK(v)
#define NS_ADD(k, v)
#endif

struct HeapItem { uint64_t key; uint32_t idx; uint32_t pad; };  // key = (bits of T >= 0) << 32 | push sequence: (T, seq) order as one integer

struct NsLayout { size_t counters, flags, T, parent, list, box, heap, total; };

inline size_t ns_align(size_t x) { return (x + 255) & ~(size_t)255; }

NsLayout ns_layout(int B, int H, int W)
{
    const size_t n = (size_t)B * (size_t)(H + 2) * (size_t)(W + 2);
    NsLayout L;
    size_t o = 0;
    L.counters = o; o = ns_align(o + NS_COUNTER_WORDS * sizeof(unsigned));   // NsCounter, then NsPhase clocks from NS_PHASE_WORD
    L.flags = o;    o = ns_align(o + n);
    L.T = o;        o = ns_align(o + n * sizeof(float));
    L.parent = o;   o = ns_align(o + n * sizeof(int));
    L.list = o;     o = ns_align(o + n * sizeof(int));
    L.box = o;      o = ns_align(o + n * 4 * sizeof(int));       // per root: min row, min col, max row, max col
    L.heap = o;     o = ns_align(o + n * sizeof(HeapItem));        // sum over clusters of (band + hole pixels) <= ext pixels (point 1)
    L.total = o;
    return L;
}

__device__ inline int ld_relaxed(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st_relaxed(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x with path halving: a non-root's parent only ever moves to one of its ancestors (smaller indices), so the shortcut
// stores race harmlessly with each other and with links, which only ever change roots
__device__ int ns_find(int *parent, int x)
{
    int p = ld_relaxed(&parent[x]);
    while (p != x) {
        const int gp = ld_relaxed(&parent[p]);
        if (gp != p) st_relaxed(&parent[x], gp);
        x = p;
        p = gp;
    }
    return x;
}

__device__ void ns_unite(int *parent, int a, int b)
{
    for (;;) {
        a = ns_find(parent, a);
        b = ns_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        if (atomicCAS(&parent[a], a, b) == a) return;          // the larger root hangs under the smaller; lost the race: retry
    }
}

__global__ __launch_bounds__(256) void k_ns_init(const uint8_t *__restrict__ img, const uint8_t *__restrict__ mask, int B, int H, int W,
                                                 uint8_t *__restrict__ out, uint8_t *__restrict__ flags, float *__restrict__ T,
                                                 int *__restrict__ parent, unsigned *__restrict__ counters)
{
    const int er = H + 2, ec = W + 2;
    const int64_t E = (int64_t)er * ec;
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n == 0)
        for (int k = 0; k < NS_COUNTER_WORDS; ++k) counters[k] = 0u;        // NsCounter, then the witness build's phase clocks
    if (n >= (int64_t)B * E) return;
    const int b = (int)(n / E);
    const int r = (int)(n - b * E), i = r / ec, j = r - i * ec;
    const uint8_t *m = mask + (int64_t)b * H * W;
    auto hole = [&](int y, int x) { return y > 0 && x > 0 && y < er - 1 && x < ec - 1 && m[(int64_t)(y - 1) * W + (x - 1)] != 0; };
    const bool interior = i > 0 && j > 0 && i < er - 1 && j < ec - 1;
    const bool h = hole(i, j);
    // fill<3>: band = cross dilation of the hole minus the hole, ext border cleared; T = 0 there, 1e6 elsewhere
    const bool band = interior && !h && (hole(i - 1, j) || hole(i + 1, j) || hole(i, j - 1) || hole(i, j + 1));
    flags[n] = h ? NS_INSIDE : NS_KNOWN;
    T[n] = band ? 0.0f : 1.0e6f;
    parent[n] = h ? (int)n : -1;
    if (interior) {
        const int64_t q = ((int64_t)b * H * W + (int64_t)(i - 1) * W + (j - 1)) * 3;
        out[q] = img[q]; out[q + 1] = img[q + 1]; out[q + 2] = img[q + 2];
    }
}

// D_LINK = range + 1: every read of a fill lies within Chebyshev distance range + 1 of the pixel filled (header)
__global__ __launch_bounds__(256) void k_ns_link(int B, int H, int W, int d_link, const uint8_t *__restrict__ flags, int *parent)
{
    const int er = H + 2, ec = W + 2;
    const int64_t E = (int64_t)er * ec;
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= (int64_t)B * E || flags[n] != NS_INSIDE) return;
    const int b = (int)(n / E);
    const int r = (int)(n - b * E), i = r / ec, j = r - i * ec;
    const int64_t base = (int64_t)b * E;
    for (int dy = -d_link; dy <= 0; ++dy) {                    // the half window before n in raster order: every pair once
        const int y = i + dy;
        if (y < 1) continue;
        for (int dx = -d_link; dx <= d_link; ++dx) {
            if (dy == 0 && dx >= 0) break;
            const int x = j + dx;
            if (x < 1 || x > ec - 2) continue;
            const int64_t q = base + (int64_t)y * ec + x;
            if (flags[q] == NS_INSIDE) ns_unite(parent, (int)n, (int)q);
        }
    }
}

__global__ __launch_bounds__(256) void k_ns_roots(int64_t N, const uint8_t *__restrict__ flags, int *parent, int *__restrict__ list,
                                                  int *__restrict__ box, unsigned *counters)
{
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N || flags[n] != NS_INSIDE) return;
    // read-only walk: a shortcut store here could overwrite a pixel's flattened root with an intermediate ancestor after its own thread
    // stored the root, and k_ns_box / k_ns_fill take parent == root as cluster membership
    int r = (int)n, p = ld_relaxed(&parent[r]);
    while (p != r) { r = p; p = ld_relaxed(&parent[r]); }
    if (r == (int)n) {
        list[atomicAdd(&counters[NS_CLUSTERS], 1u)] = r;
        box[4 * n] = box[4 * n + 1] = INT32_MAX;
        box[4 * n + 2] = box[4 * n + 3] = -1;
    } else {
        st_relaxed(&parent[n], r);
    }
}

__global__ __launch_bounds__(256) void k_ns_box(int B, int H, int W, const uint8_t *__restrict__ flags, const int *__restrict__ parent,
                                                int *box)
{
    const int er = H + 2, ec = W + 2;
    const int64_t E = (int64_t)er * ec;
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= (int64_t)B * E || flags[n] != NS_INSIDE) return;
    // an extreme row / column of a set is attained at a pixel with a 4-neighbour outside it (the ext border is never a hole)
    if (flags[n - ec] == NS_INSIDE && flags[n + ec] == NS_INSIDE && flags[n - 1] == NS_INSIDE && flags[n + 1] == NS_INSIDE) return;
    const int b = (int)(n / E);
    const int r = (int)(n - b * E), i = r / ec, j = r - i * ec;
    int *bx = box + 4 * (int64_t)parent[n];
    atomicMin(&bx[0], i); atomicMin(&bx[1], j); atomicMax(&bx[2], i); atomicMax(&bx[3], j);
}

constexpr int ns_offsets(int R)
{
    int c = 0;
    for (int dk = -R; dk <= R; ++dk)
        for (int dl = -R; dl <= R; ++dl) c += dk * dk + dl * dl <= R * R;
    return c;
}

__device__ inline uint8_t ns_sat8(long v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
__device__ inline float ns_rdf(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

template <int R>
__global__ __launch_bounds__(NS_WAVE) void k_ns_fill(int B, int H, int W, uint8_t *out, uint8_t *flags, float *T, const int *__restrict__ parent,
                                                     const int *__restrict__ list, const int *__restrict__ box, HeapItem *pool,
                                                     int64_t pool_items, unsigned *counters)
{
    constexpr int NOFF = ns_offsets(R);
    static_assert(NOFF <= NS_WAVE, "one disc offset per lane");
    __shared__ HeapItem lheap[NS_LDS_HEAP];
    const int lane = threadIdx.x;
    const int er = H + 2, ec = W + 2;
    const int64_t E = (int64_t)er * ec;

    // this lane's disc offset (fill<3>'s `offs`: raster order over (dk, dl)) and its weight 1 / (len2^2 + 1)
    int odk = 0, odl = 0;
    float ow = 0.0f;
    bool olive = false;
    {
        int o = 0;
        for (int dk = -R; dk <= R; ++dk)
            for (int dl = -R; dl <= R; ++dl) {
                if (dk * dk + dl * dl > R * R) continue;
                if (o == lane) {
                    odk = dk; odl = dl; olive = true;
                    const float len2 = (float)dl * (float)dl + (float)dk * (float)dk;
                    ow = 1 / (len2 * len2 + 1);
                }
                ++o;
            }
    }

    for (;;) {
        unsigned c = 0;
        if (lane == 0) c = atomicAdd(&counters[NS_WORK], 1u);
        c = (unsigned)__builtin_amdgcn_readfirstlane((int)c);
        if (c >= __hip_atomic_load(&counters[NS_CLUSTERS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        const int root = list[c];
        const int b = (int)(root / E);
        const int64_t base = (int64_t)b * E;
        uint8_t *fl = flags + base;
        float *tt = T + base;
        const int *par = parent + base;
        uint8_t *im = out + (int64_t)b * H * W * 3;
        const int *bx = box + 4 * (int64_t)root;
        const int r0 = max(bx[0] - 1, 1), r1 = min(bx[2] + 1, er - 2), c0 = max(bx[1] - 1, 1), c1 = min(bx[3] + 1, ec - 2);
        const int rw = c1 - c0 + 1;
        const int64_t area = (int64_t)(r1 - r0 + 1) * rw;
        const uint64_t lt = (lane ? ((~0ull) >> (64 - lane)) : 0ull);

        // the cluster's band pixels, in raster order: not a hole, 4-adjacent to a hole of this cluster (point 1: of no other)
        auto classify = [&](int64_t t, bool &isb, bool &ish, int &idx) {
            isb = ish = false;
            idx = 0;
            if (t >= area) return;
            const int i = r0 + (int)(t / rw), j = c0 + (int)(t % rw);
            idx = i * ec + j;
            const int p = par[idx];
            ish = p == root;
            isb = p < 0 && (par[idx - ec] == root || par[idx + ec] == root || par[idx - 1] == root || par[idx + 1] == root);
        };
#ifdef MPF_WITNESS
        uint64_t ph[NSP_N] = {};
#endif
        NS_CLOCK(c_start);
        int nb = 0, nh = 0;
        for (int64_t t0 = 0; t0 < area; t0 += NS_WAVE) {
            bool isb, ish;
            int idx;
            classify(t0 + lane, isb, ish, idx);
            nb += __popcll(__ballot(isb));
            nh += __popcll(__ballot(ish));
        }
        const int total = nb + nh;                         // every pixel is pushed at most once: the heap never holds more

        bool in_lds = nb <= NS_LDS_HEAP;
        HeapItem *gheap = nullptr;
        int cap = NS_LDS_HEAP;
        auto spill_region = [&]() -> bool {
            unsigned off = 0;
            if (lane == 0) off = atomicAdd(&counters[NS_POOL_ITEMS], (unsigned)total);
            off = (unsigned)__builtin_amdgcn_readfirstlane((int)off);
            if ((int64_t)off + total > pool_items) {                   // impossible by point 1; never write past the pool, and say so
                if (lane == 0) atomicAdd(&counters[NS_FAILED], 1u);
                return false;
            }
            gheap = pool + off;
            cap = total;
            return true;
        };
        if (!in_lds) {                                        // the band alone outgrows LDS: the heap starts in the pool
            if (!spill_region()) continue;
            if (lane == 0) atomicAdd(&counters[NS_SPILLED_AT_START], 1u);
        }
        int nput = 0;
        for (int64_t t0 = 0; t0 < area; t0 += NS_WAVE) {
            bool isb, ish;
            int idx;
            classify(t0 + lane, isb, ish, idx);
            const uint64_t m = __ballot(isb);
            if (isb) {
                const int pos = nput + __popcll(m & lt);
                const HeapItem it = {(uint64_t)(unsigned)pos, (uint32_t)idx, 0u};   // T = 0: sorted by sequence, already a heap
                if (in_lds) lheap[pos] = it; else gheap[pos] = it;
            }
            nput += __popcll(m);
        }
        __syncthreads();
        int size = nb;
        unsigned seq = (unsigned)nb;

        auto hget = [&](int k) -> HeapItem { return in_lds ? lheap[k] : gheap[k]; };
        auto hset = [&](int k, const HeapItem &v) { if (in_lds) lheap[k] = v; else gheap[k] = v; };

        NS_CLOCK(c_setup);
        NS_ADD(NSP_SETUP, c_setup - c_start);
        while (size > 0) {
            NS_CLOCK(c_pop0);
            // pop the least (T, seq)
            const HeapItem top = hget(0);
            --size;
            if (size > 0) {
                const HeapItem last = hget(size);
                int k = 0;
                for (;;) {
                    int ch = 2 * k + 1;
                    if (ch >= size) break;
                    HeapItem cv = hget(ch);
                    if (ch + 1 < size) {
                        const HeapItem cw = hget(ch + 1);
                        if (cw.key < cv.key) { cv = cw; ++ch; }
                    }
                    if (last.key < cv.key) break;
                    hset(k, cv);
                    k = ch;
                }
                hset(k, last);
            }
            const int ii = (int)top.idx / ec, jj = (int)top.idx - ((int)top.idx / ec) * ec;
            NS_CLOCK(c_pop1);
            NS_ADD(NSP_POP, c_pop1 - c_pop0);
            NS_ADD(NSP_POPS, 1);
            const int ni[4] = {ii - 1, ii, ii + 1, ii}, nj[4] = {jj, jj - 1, jj, jj + 1};
            for (int q = 0; q < 4; ++q) {
                const int i = ni[q], j = nj[q];
                NS_CLOCK(c_q0);
                if (i <= 0 || j <= 0 || i > er - 1 || j > ec - 1 || fl[i * ec + j] != NS_INSIDE) {
                    NS_CLOCK(c_rej);
                    NS_ADD(NSP_REJECT, c_rej - c_q0);
                    continue;
                }
                auto inside = [&](int a, int bb) { return fl[a * ec + bb] == NS_INSIDE; };
                auto eik = [&](int i1, int j1, int i2, int j2) -> float {     // eikonal2, in double
                    const double a11 = tt[i1 * ec + j1], a22 = tt[i2 * ec + j2], m12 = (a22 < a11) ? a22 : a11;
                    const bool in1 = inside(i1, j1), in2 = inside(i2, j2);
                    double sol;
                    if (!in1) {
                        if (!in2) sol = (fabs(a11 - a22) >= 1.0) ? 1 + m12 : (a11 + a22 + sqrt((double)(2 - (a11 - a22) * (a11 - a22)))) * 0.5;
                        else sol = 1 + a11;
                    } else {
                        sol = !in2 ? 1 + a22 : 1 + m12;
                    }
                    return (float)sol;
                };
                const float ea = eik(i - 1, j, i, j - 1), eb = eik(i + 1, j, i, j - 1);
                const float ec_ = eik(i - 1, j, i, j + 1), ed = eik(i + 1, j, i, j + 1);
                const float m1 = (eb < ea) ? eb : ea, m2 = (ed < ec_) ? ed : ec_;
                const float dist = (m2 < m1) ? m2 : m1;
                tt[i * ec + j] = dist;
                NS_CLOCK(c_q1);
                NS_ADD(NSP_ARRIVAL, c_q1 - c_q0);

                // lane o: disc offset o (fill<3>'s NS branch, one channel per component)
                bool valid = false;
                float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f, x0 = 0.0f, x1 = 0.0f, x2 = 0.0f;
                if (olive) {
                    const int k = i + odk, l = j + odl;
                    if (k > 0 && l > 0 && k < er - 1 && l < ec - 1 && !inside(k, l)) {
                        valid = true;
                        const int km = k - 1 + (k == 1), kp = k - 1 - (k == er - 2), lm = l - 1 + (l == 1), lp = l - 1 - (l == ec - 2);
                        const float ry = (float)(k - i), rx = (float)(l - j);
                        const float r2 = rx * rx + ry * ry;
                        const bool e_in = inside(k, l + 1), w_in = inside(k, l - 1), s_in = inside(k + 1, l), n_in = inside(k - 1, l);
                        const uint8_t *pc = im + ((int64_t)km * W + lm) * 3;
                        const uint8_t *ps1 = im + ((int64_t)(kp + 1) * W + lm) * 3, *ps0 = im + ((int64_t)kp * W + lm) * 3;
                        const uint8_t *pn = im + ((int64_t)(km - 1) * W + lm) * 3;
                        const uint8_t *pe = im + ((int64_t)km * W + lp + 1) * 3, *pw = im + ((int64_t)km * W + lm - 1) * 3;
                        float wch[3], xch[3];
                        for (int c = 0; c < 3; ++c) {
                            const float ctr = (float)pc[c];
                            float gIx, gIy;
                            if (!s_in) {
                                const float a = (float)ps1[c], bb = (float)ps0[c];
                                gIx = !n_in ? fabsf(a - bb) + fabsf(bb - (float)pn[c]) : fabsf(a - bb) * 2.0f;
                            } else {
                                gIx = !n_in ? fabsf((float)ps0[c] - (float)pn[c]) * 2.0f : 0.0f;
                            }
                            if (!e_in) {
                                const float a = (float)pe[c];
                                gIy = !w_in ? fabsf(a - ctr) + fabsf(ctr - (float)pw[c]) : fabsf(a - ctr) * 2.0f;
                            } else {
                                gIy = !w_in ? fabsf(ctr - (float)pw[c]) * 2.0f : 0.0f;
                            }
                            gIx = -gIx;
                            const float num = rx * gIx + ry * gIy;
                            const float qd = fabsf(num / sqrtf(r2 * (gIx * gIx + gIy * gIy)));
                            const float dir = fabsf(num) <= 0.01f ? 0.000001f : qd;
                            const float w = ow * dir;
                            wch[c] = w;
                            xch[c] = w * ctr;
                        }
                        w0 = wch[0]; w1 = wch[1]; w2 = wch[2];
                        x0 = xch[0]; x1 = xch[1]; x2 = xch[2];
                    }
                }
                // the fp32 sums in offset order, from 1e-20 / 0 (not a tree: the same roundings as the host loop)
                NS_CLOCK(c_q2);
                NS_ADD(NSP_DISC, c_q2 - c_q1);
                const uint64_t vm = __ballot(valid);
                float Ia0 = 0.0f, Ia1 = 0.0f, Ia2 = 0.0f, s0 = 1.0e-20f, s1 = 1.0e-20f, s2 = 1.0e-20f;
#pragma unroll
                for (int o = 0; o < NOFF; ++o) {
                    if ((vm >> o) & 1) {
                        Ia0 += ns_rdf(x0, o); Ia1 += ns_rdf(x1, o); Ia2 += ns_rdf(x2, o);
                        s0 += ns_rdf(w0, o); s1 += ns_rdf(w1, o); s2 += ns_rdf(w2, o);
                    }
                }
                NS_CLOCK(c_q3);
                NS_ADD(NSP_FOLD, c_q3 - c_q2);
                uint8_t *po = im + ((int64_t)(i - 1) * W + (j - 1)) * 3;
                po[0] = ns_sat8((long)rint((double)Ia0 / s0));
                po[1] = ns_sat8((long)rint((double)Ia1 / s1));
                po[2] = ns_sat8((long)rint((double)Ia2 / s2));
                fl[i * ec + j] = NS_KNOWN;                  // fill<3> marks it BAND: no longer INSIDE is all that is tested

                // push (dist, seq)
                if (size == cap) {
                    if (!in_lds) {                              // cannot happen: total bounds the pushes
                        if (lane == 0) atomicAdd(&counters[NS_FAILED], 1u);
                        size = -1;
                        break;
                    }
                    if (!spill_region()) { size = -1; break; }
                    for (int k = lane; k < size; k += NS_WAVE) gheap[k] = lheap[k];     // the front outgrows LDS: move it to the pool
                    __syncthreads();
                    in_lds = false;
                    if (lane == 0) atomicAdd(&counters[NS_SPILLED_RUNNING], 1u);
                }
                const HeapItem it = {((uint64_t)__float_as_uint(dist) << 32) | seq++, (uint32_t)(i * ec + j), 0u};
                int k = size++;
                while (k > 0) {
                    const int p = (k - 1) / 2;
                    const HeapItem pv = hget(p);
                    if (pv.key < it.key) break;
                    hset(k, pv);
                    k = p;
                }
                hset(k, it);
                NS_CLOCK(c_q4);
                NS_ADD(NSP_PUSH, c_q4 - c_q3);
                NS_ADD(NSP_FILLS, 1);
            }
        }
#ifdef MPF_WITNESS
        if (lane == 0)
            for (int k = 0; k < NSP_N; ++k) atomicAdd((unsigned long long *)(counters + NS_PHASE_WORD) + k, (unsigned long long)ph[k]);
#endif
        __syncthreads();                                       // the LDS heap is the next cluster's
    }
}

template <int R>
int ns_launch_fill(int blocks, int B, int H, int W, uint8_t *out, uint8_t *flags, float *T, const int *parent, const int *list, const int *box,
                   HeapItem *pool, int64_t pool_items, unsigned *counters, hipStream_t st)
{
    hipLaunchKernelGGL(k_ns_fill<R>, dim3(blocks), dim3(NS_WAVE), 0, st, B, H, W, out, flags, T, parent, list, box, pool, pool_items, counters);
    return mpf_launch_status("k_ns_fill");
}

bool ns_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}   // namespace

extern "C" size_t mpf_inpaint_ns_workspace(int B, int H, int W, double radius)
{
    (void)radius;
    if (B < 1 || H < 1 || W < 1) return 0;
    return ns_layout(B, H, W).total;
}

extern "C" int mpf_inpaint_ns(const uint8_t *d_img, const uint8_t *d_mask, int B, int H, int W, double radius, uint8_t *d_out, void *d_ws,
                              size_t ws_bytes, void *stream)
{
    MPF_REQUIRE(d_img && d_mask && d_out && d_ws, "mpf_inpaint_ns: null pointer");
    MPF_REQUIRE(B >= 1 && H >= 1 && W >= 1, "mpf_inpaint_ns: bad shape %d x %d x %d", B, H, W);
    MPF_REQUIRE((int64_t)B * (H + 2) * (int64_t)(W + 2) < ((int64_t)1 << 31) - 1, "mpf_inpaint_ns: batch too large (%d x %d x %d)", B, H, W);
    MPF_REQUIRE(isfinite(radius), "mpf_inpaint_ns: radius must be finite");
    if (H < 2 || W < 2) {
        mpf_set_error("mpf_inpaint_ns: frames of fewer than 2 rows or columns are not supported (%d x %d); use mpf_inpaint_host", H, W);
        return MPF_ERR_UNSUPPORTED;
    }
    int range = (int)lrint(radius);
    range = range < 1 ? 1 : (range > 100 ? 100 : range);        // cvInpaint: cvRound, then clamped to [1, 100]
    if (range > NS_MAX_RANGE) {
        mpf_set_error("mpf_inpaint_ns: radius %g rounds to %d; the device fill supports 1 - %d (use mpf_inpaint_host)", radius, range, NS_MAX_RANGE);
        return MPF_ERR_UNSUPPORTED;
    }
    const size_t npx = (size_t)B * H * W;
    MPF_REQUIRE(!ns_overlap(d_out, 3 * npx, d_img, 3 * npx) && !ns_overlap(d_out, 3 * npx, d_mask, npx),
                "mpf_inpaint_ns: d_out may not alias the image or the mask");
    const NsLayout L = ns_layout(B, H, W);
    MPF_REQUIRE(ws_bytes >= L.total, "mpf_inpaint_ns: workspace of %zu bytes, %zu needed (mpf_inpaint_ns_workspace)", ws_bytes, L.total);
    MPF_REQUIRE(!ns_overlap(d_ws, L.total, d_out, 3 * npx) && !ns_overlap(d_ws, L.total, d_img, 3 * npx) && !ns_overlap(d_ws, L.total, d_mask, npx),
                "mpf_inpaint_ns: the workspace may not alias the image, the mask or d_out");

    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)d_ws;
    unsigned *counters = (unsigned *)(ws + L.counters);
    uint8_t *flags = ws + L.flags;
    float *T = (float *)(ws + L.T);
    int *parent = (int *)(ws + L.parent), *list = (int *)(ws + L.list);
    int *box = (int *)(ws + L.box);
    HeapItem *pool = (HeapItem *)(ws + L.heap);
    const int64_t N = (int64_t)B * (H + 2) * (W + 2);
    const unsigned grid = (unsigned)((N + 255) / 256);

    hipLaunchKernelGGL(k_ns_init, dim3(grid), dim3(256), 0, st, d_img, d_mask, B, H, W, d_out, flags, T, parent, counters);
    if (int e = mpf_launch_status("k_ns_init")) return e;
    hipLaunchKernelGGL(k_ns_link, dim3(grid), dim3(256), 0, st, B, H, W, range + 1, flags, parent);
    if (int e = mpf_launch_status("k_ns_link")) return e;
    hipLaunchKernelGGL(k_ns_roots, dim3(grid), dim3(256), 0, st, N, flags, parent, list, box, counters);
    if (int e = mpf_launch_status("k_ns_roots")) return e;
    hipLaunchKernelGGL(k_ns_box, dim3(grid), dim3(256), 0, st, B, H, W, flags, parent, box);
    if (int e = mpf_launch_status("k_ns_box")) return e;

    int dev = 0, cus = 0;
    MPF_HIP(hipGetDevice(&dev));
    MPF_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const int64_t most = (int64_t)B * H * W;                      // no more clusters than hole pixels
    const int blocks = (int)std::min<int64_t>((int64_t)std::max(cus, 1) * NS_FILL_BLOCKS_PER_CU, most);
    switch (range) {
    case 1: return ns_launch_fill<1>(blocks, B, H, W, d_out, flags, T, parent, list, box, pool, N, counters, st);
    case 2: return ns_launch_fill<2>(blocks, B, H, W, d_out, flags, T, parent, list, box, pool, N, counters, st);
    case 3: return ns_launch_fill<3>(blocks, B, H, W, d_out, flags, T, parent, list, box, pool, N, counters, st);
    default: return ns_launch_fill<4>(blocks, B, H, W, d_out, flags, T, parent, list, box, pool, N, counters, st);
    }
}
