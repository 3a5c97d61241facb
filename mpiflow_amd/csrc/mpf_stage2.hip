// mpf_stage2.hip - the pointwise chain of warp-back stage 2's inpaint (warpback/stage2_dataset.py) around the three EdgeConnect generators,
// one launch where the reference runs two to eight small torch operations.
//
// Contract: include/mpiflow_hip.h (MpfStage2Args).  One thread per pixel of one image; every operation fp32, rounded once, in torch's order
// (the build has no contraction), so each result equals the torch expression bit for bit:
//   k_s2_gray_hole    gray = (0.2989 r + 0.587 g) + 0.114 b (torchvision's Grayscale);  mask_hole = 1 - mask
//   k_s2_edge_input   edge_input = cat(gray, edge, mask_hole)
//   k_s2_gen_inputs   image_input = cat(image + mask_hole, edge_inpaint);  disp_input = cat(disp + mask_hole, edge_inpaint)
//   k_s2_merge        x_merged = x * (1 - mask_hole) + x_inpaint * mask_hole for the image's three channels and the disparity
// Every address is plane * hw + p with p < hw.  No LDS.
#include "mpf_common.h"

#define S2_THREADS 256

struct Stage2Dev {
    const float *image, *disp, *mask, *edge, *edge_inpaint, *image_inpaint, *disp_inpaint;
    float *gray, *mask_hole, *edge_input, *image_input, *disp_input, *image_merged, *disp_merged;
    int hw;
};

__global__ __launch_bounds__(S2_THREADS) void k_s2_gray_hole(const Stage2Dev a)
{
    const int p = blockIdx.x * S2_THREADS + threadIdx.x;
    if (p >= a.hw) return;
    const size_t b = blockIdx.y, hw = a.hw;
    const float *img = a.image + b * 3 * hw + p;
    a.gray[b * hw + p] = (0.2989f * img[0] + 0.587f * img[hw]) + 0.114f * img[2 * hw];
    a.mask_hole[b * hw + p] = 1.0f - a.mask[b * hw + p];
}

__global__ __launch_bounds__(S2_THREADS) void k_s2_edge_input(const Stage2Dev a)
{
    const int p = blockIdx.x * S2_THREADS + threadIdx.x;
    if (p >= a.hw) return;
    const size_t b = blockIdx.y, hw = a.hw;
    float *o = a.edge_input + b * 3 * hw + p;
    o[0] = a.gray[b * hw + p], o[hw] = a.edge[b * hw + p], o[2 * hw] = a.mask_hole[b * hw + p];
}

__global__ __launch_bounds__(S2_THREADS) void k_s2_gen_inputs(const Stage2Dev a)
{
    const int p = blockIdx.x * S2_THREADS + threadIdx.x;
    if (p >= a.hw) return;
    const size_t b = blockIdx.y, hw = a.hw;
    const float mh = a.mask_hole[b * hw + p], e = a.edge_inpaint[b * hw + p];
    const float *img = a.image + b * 3 * hw + p;
    float *oi = a.image_input + b * 4 * hw + p, *od = a.disp_input + b * 2 * hw + p;
    oi[0] = img[0] + mh, oi[hw] = img[hw] + mh, oi[2 * hw] = img[2 * hw] + mh, oi[3 * hw] = e;
    od[0] = a.disp[b * hw + p] + mh, od[hw] = e;
}

__global__ __launch_bounds__(S2_THREADS) void k_s2_merge(const Stage2Dev a)
{
    const int p = blockIdx.x * S2_THREADS + threadIdx.x;
    if (p >= a.hw) return;
    const size_t b = blockIdx.y, hw = a.hw;
    const float mh = a.mask_hole[b * hw + p], keep = 1.0f - mh;
    const float *img = a.image + b * 3 * hw + p, *inp = a.image_inpaint + b * 3 * hw + p;
    float *o = a.image_merged + b * 3 * hw + p;
    for (int c = 0; c < 3; ++c) o[c * hw] = img[c * hw] * keep + inp[c * hw] * mh;
    a.disp_merged[b * hw + p] = a.disp[b * hw + p] * keep + a.disp_inpaint[b * hw + p] * mh;
}

// ---------------------------------------------------------------- launchers

static bool s2_overlap(const void *p, size_t pn, const void *q, size_t qn)
{
    const char *a = (const char *)p, *b = (const char *)q;
    return a < b + qn && b < a + pn;
}

// ins / outs: pointer and channel count of every tensor the call reads / writes
static int s2_check(const MpfStage2Args *a, const char *who, const void *const *ins, const int *inc, int ni, void *const *outs, const int *outc, int no, Stage2Dev &d)
{
    MPF_REQUIRE(a, "%s: null argument block", who);
    MPF_REQUIRE(a->B >= 1 && a->B <= 65535 && a->h >= 1 && a->w >= 1 && (int64_t)a->B * a->h * a->w <= (1 << 28),
                "%s: bad shape: B must be 1..65535, h, w >= 1 and B * h * w at most 2^28 (got B, h, w = %d, %d, %d)", who, a->B, a->h, a->w);
    const size_t plane = (size_t)a->B * a->h * a->w * 4;
    for (int i = 0; i < ni; ++i) MPF_REQUIRE(ins[i], "%s: null pointer (input %d of the call)", who, i);
    for (int i = 0; i < no; ++i) {
        MPF_REQUIRE(outs[i], "%s: null pointer (output %d of the call)", who, i);
        for (int k = 0; k < ni; ++k)
            MPF_REQUIRE(!s2_overlap(outs[i], plane * outc[i], ins[k], plane * inc[k]), "%s: output %d overlaps input %d", who, i, k);
        for (int k = 0; k < i; ++k)
            MPF_REQUIRE(!s2_overlap(outs[i], plane * outc[i], outs[k], plane * outc[k]), "%s: outputs %d and %d overlap", who, i, k);
    }
    d = Stage2Dev{};
    d.image = a->image, d.disp = a->disp, d.mask = a->mask, d.edge = a->edge, d.edge_inpaint = a->edge_inpaint;
    d.image_inpaint = a->image_inpaint, d.disp_inpaint = a->disp_inpaint;
    d.gray = a->gray, d.mask_hole = a->mask_hole, d.edge_input = a->edge_input, d.image_input = a->image_input, d.disp_input = a->disp_input;
    d.image_merged = a->image_merged, d.disp_merged = a->disp_merged;
    d.hw = a->h * a->w;
    return 0;
}

#define S2_LAUNCH(kernel)                                                                                                                  \
    hipLaunchKernelGGL(kernel, dim3((unsigned)((d.hw + S2_THREADS - 1) / S2_THREADS), (unsigned)a->B), dim3(S2_THREADS), 0, (hipStream_t)stream, d); \
    return mpf_launch_status(#kernel)

extern "C" int mpf_stage2_gray_hole(const MpfStage2Args *a, void *stream)
{
    Stage2Dev d;
    const void *ins[2] = {a ? a->image : 0, a ? a->mask : 0};
    void *outs[2] = {a ? a->gray : 0, a ? a->mask_hole : 0};
    const int inc[2] = {3, 1}, outc[2] = {1, 1};
    const int rc = s2_check(a, "mpf_stage2_gray_hole", ins, inc, 2, outs, outc, 2, d);
    if (rc) return rc;
    S2_LAUNCH(k_s2_gray_hole);
}

extern "C" int mpf_stage2_edge_input(const MpfStage2Args *a, void *stream)
{
    Stage2Dev d;
    const void *ins[3] = {a ? a->gray : 0, a ? a->edge : 0, a ? a->mask_hole : 0};
    void *outs[1] = {a ? a->edge_input : 0};
    const int inc[3] = {1, 1, 1}, outc[1] = {3};
    const int rc = s2_check(a, "mpf_stage2_edge_input", ins, inc, 3, outs, outc, 1, d);
    if (rc) return rc;
    S2_LAUNCH(k_s2_edge_input);
}

extern "C" int mpf_stage2_gen_inputs(const MpfStage2Args *a, void *stream)
{
    Stage2Dev d;
    const void *ins[4] = {a ? a->image : 0, a ? a->disp : 0, a ? a->mask_hole : 0, a ? a->edge_inpaint : 0};
    void *outs[2] = {a ? a->image_input : 0, a ? a->disp_input : 0};
    const int inc[4] = {3, 1, 1, 1}, outc[2] = {4, 2};
    const int rc = s2_check(a, "mpf_stage2_gen_inputs", ins, inc, 4, outs, outc, 2, d);
    if (rc) return rc;
    S2_LAUNCH(k_s2_gen_inputs);
}

extern "C" int mpf_stage2_merge(const MpfStage2Args *a, void *stream)
{
    Stage2Dev d;
    const void *ins[5] = {a ? a->image : 0, a ? a->disp : 0, a ? a->mask_hole : 0, a ? a->image_inpaint : 0, a ? a->disp_inpaint : 0};
    void *outs[2] = {a ? a->image_merged : 0, a ? a->disp_merged : 0};
    const int inc[5] = {3, 1, 1, 3, 1}, outc[2] = {3, 1};
    const int rc = s2_check(a, "mpf_stage2_merge", ins, inc, 5, outs, outc, 2, d);
    if (rc) return rc;
    S2_LAUNCH(k_s2_merge);
}
