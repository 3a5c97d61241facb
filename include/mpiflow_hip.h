/* mpiflow_hip.h - C ABI of libmpiflow_hip.so: the MI355X (gfx950) implementation of MPI-Flow's per-image hot path.
 *
 * The reference (Sharpiless/MPI-Flow) has no plugin/operator registry.  Its boundary for this path is
 *   (1) one real FFI symbol: `forward_warping` in external/forward_warping/warping.c:6, loaded with ctypes at
 *       moving_obj.py:12-13 and called with host pointers at moving_obj.py:127-129; and
 *   (2) plain Python call signatures (utils/utils.py, utils/mpi/ modules, geometry.py, moving_obj.py), whose arithmetic
 *       is carried out by PyTorch ATen kernels.
 * This library therefore exports (1) under its exact name and semantics, and for (2) one device-pointer entry point
 * per reference function on the path (the comment on each cites the reference lines it replaces).  The Python
 * package mpiflow_amd/ mirrors the reference's signatures and binds these symbols with ctypes; INTEGRATION.md shows
 * the same binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every mpf_* function returns 0 on success, otherwise a hipError_t value (or MPF_ERR_*); mpf_last_error()
 *     returns a description for the calling thread.  Nothing is thrown, nothing aborts.
 *   - pointers named d_* are DEVICE pointers (fp32 unless stated), row-major, contiguous; the caller owns them.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All calls are asynchronous on that
 *     stream and graph-capturable: no allocation, no synchronisation, no host<->device copies inside, except the
 *     two host-pointer conveniences at the bottom which say so.
 *   - small per-call matrices (K^-1, G, per-plane homographies, plane depths) arrive in ONE device buffer
 *     `d_params` of MPF_PARAMS_FLOATS(records) floats laid out as below; the host computes them with the
 *     reference's own batched torch-CPU expressions (bit-identical homographies are a parity requirement).
 *   - B == 1 (as in the reference's entry point); S planes ordered near -> far; N = H*W; S < 4096.
 */
#ifndef MPIFLOW_HIP_H
#define MPIFLOW_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPF_VERSION 601   /* round 3 (301): + mpf_warp_views_and_blend_next, mpf_warp_composite_split, mpf_src_flow, mpf_merge_depth_ordered;
                             round 4 (401): + mpf_moving_object_chain, mpf_warp_views_blend_next_merge_prev, mpf_stream_create_cu_subset / _destroy,
                             mpf_encoder_input, mpf_conv2d_f32, mpf_maxpool3x3s2_f32; MpfConvArgs + plane_major, loaders 4 / 5, epilogues 4 / 5 / 6;
                             round 5 (501): + the parity-grade producer engine mpf_pconv, mpf_pfmn_input, mpf_pencoder_input, mpf_pbilinear2x, mpf_pper_plane,
                             mpf_pplane_masks, mpf_pmaxpool3x3s2; MpfMergeArgs + obj_mask_stride, mpf_merge_ex, mpf_src_flow_hard;
                             (503): MpfConvArgs + bprime_table, pw (planes per workgroup of the few-block layers);
                             round 6 (601): + loader 6 (MPF_CONV_LD_NEAREST_PHASE), mpf_tune("fwarp_gate"), mpf_forward_warp_workspace + 256 bytes;
                             the RAFT entry points added since (mpf_corr_*, mpf_upsample_*, mpf_flow_loss_term*, and now mpf_gru_reset, mpf_gru_update and
                             their _backward calls with MpfGruTerm / MpfGruArgs, and now mpf_norm_stats, mpf_norm_act, mpf_norm_act_backward_reduce and
                             mpf_norm_act_backward with MpfNormTerm / MpfNormArgs, and now mpf_raft_images, mpf_context_split, mpf_upflow8 and
                             their _backward calls with MpfRaftGlueArgs, and now mpf_upflow8_loss_term, its _backward call and
                             mpf_upflow8_loss_workspace with MpfUpsampleArgs, and now mpf_raft_images_padded, mpf_upsample_flow_crop, mpf_upflow8_crop,
                             mpf_flow_metrics and mpf_flow_metrics_workspace with MpfRaftEvalArgs, and now mpf_grad_norm, mpf_adamw_clipped and
                             mpf_adamw_workspace with MpfOptTensor / MpfAdamWArgs, and now mpf_forward_interpolate and
                             mpf_forward_interpolate_workspace with MpfWarmStartArgs, and now mpf_flow_to_image, mpf_flow_to_image_workspace and
                             mpf_flow_encode_kitti with MpfFlowVizArgs, and now mpf_rgbd_mesh_vertices, mpf_rasterize_grid and
                             mpf_rasterize_grid_workspace with MpfMeshVertexArgs / MpfMeshRasterArgs, and now mpf_canny and mpf_canny_workspace
                             with MpfCannyArgs and the four mpf_stage2_* calls with MpfStage2Args, and now mpf_sparse_bilateral, mpf_sparse_bilateral_workspace
                             and mpf_sparse_bilateral_rank with MpfBilateralArgs, and now mpf_gather_pxpy, mpf_gather_pxpy_bwd, mpf_sample_pdf,
                             mpf_disp_consistency, its _bwd and _workspace calls with MpfGatherPxpyArgs / MpfSamplePdfArgs / MpfDispConsistencyArgs, and now mpf_flow_warp,
                             mpf_flow_warp_bwd and mpf_flow_warp_workspace with MpfFlowWarpArgs, and now mpf_pan_block1 and mpf_pan_block1_workspace with
                             MpfPanArgs) only ADD symbols: the number, which tests/test_capi.py pins, stays 601 */

/* d_params layout (floats):
 *   [0..8]   K_src^-1 (3x3 row-major)            [9..20]  G_tgt_src rows 0..2 (3x4 row-major: R | t)
 *   [21..31] reserved (zero)
 *   then one 16-float record per plane (per plane and pose for mpf_src_blend_flow: record = s*P + p):
 *     [0..8] 3x3 homography (H_src_tgt for warps, H_tgt_src for flows)   [9] plane depth d_s = 1/disparity_s
 *     [10..15] reserved (zero)                                                                                  */
#define MPF_PARAMS_HEADER 32
#define MPF_PLANE_RECORD 16
#define MPF_PARAMS_FLOATS(records) (MPF_PARAMS_HEADER + MPF_PLANE_RECORD * (records))

#define MPF_ERR_BAD_ARGUMENT 10001
#define MPF_ERR_UNSUPPORTED  10002

int mpf_version(void);
const char *mpf_last_error(void);
/* fills CU count, HBM bytes, gfx arch name (e.g. "gfx950"); any pointer may be NULL */
int mpf_device_info(int device, int *cu_count, size_t *hbm_bytes, char *arch, size_t arch_len);
/* A stream restricted to every `stride`-th compute unit (starting at `offset`): hipExtStreamCreateWithCUMask.  For latency-sized side work
 * underneath a chip-filling launch on another stream (pipeline.OverlappedPairRenderer.attach_chain(cu_stride=...)).  The caller owns the
 * stream (mpf_stream_destroy). */
int mpf_stream_create_cu_subset(int stride, int offset, void **out_stream);
int mpf_stream_destroy(void *stream);

/* Scheduling knobs of the product library (libmpiflow_hip.so) - none of them can change a result, every setting gives the same bytes (asserted by the tests):
 *   "sbf_px" = pixels per thread of mpf_src_blend_flow (0 auto, 1, 2);  "conv_pf" = 0 | 1 (default): the plane-walking conv kernels (MpfConvArgs.pw > 1) copy the
 *   next step's weight fragments / raw tile into a second LDS buffer during the current MFMA phase;  "chain_grid" / "chain_prio" = grid cap / s_setprio of the
 *   forward-warp kernels;  "fwarp_gate" = bucket visits above which caller-supplied targets leave the gather path for the radix path (-1 = default: one visit per
 *   source; 0 = always radix).
 * Keys that select RETIRED KERNEL VARIANTS ("stage_b", "planar_lds", "ovl_depth", "ovl_xcd_a", "view_shift", "fwarp_path": bit-identical witnesses of the shipped
 * kernels) or TIMING ABLATIONS ("ovl_ablate", "stage_b" 101..106: INVALID results) exist only in the witness build, libmpiflow_hip_witness.so (-DMPF_WITNESS; the
 * tests and tools load it through mpiflow_amd._lib.witness()); the product library returns MPF_ERR_BAD_ARGUMENT for them and does not contain those kernels.
 * The knobs are PROCESS-GLOBAL plain ints, not per-stream and NOT thread-safe: set them from one thread while no other thread is launching work through this
 * library.  Unknown keys return MPF_ERR_BAD_ARGUMENT. */
int mpf_tune(const char *key, int value);
int mpf_is_witness_build(void);   /* 1 for libmpiflow_hip_witness.so, 0 for the product library */

/* ================= fused hot path =============================================================================== */

/* Stage A + C.  Replaces utils/utils.py:190-204 (get_src_xyz_from_plane_disparity + render() in the source frame +
 * the blend of the source image into every plane) fused with HomographySample.sample_inverse
 * (utils/mpi/homography_sampler.py:160-220) + plane_volume_rendering_flow (utils/mpi/mpi_rendering.py:102-139) for
 * P = 0, 1 or 2 poses sharing the same source-frame weights.
 *   d_mpi [S,4,H,W] planar (rgb, sigma);  d_img [3,H,W];  d_params with S*P records (S records if P == 0; only the
 *   depth is read then).  Outputs, each optional (NULL to skip):
 *   d_out_rgba [S,H,W,4] interleaved blended rgb + sigma (the layout mpf_warp_composite streams fastest);
 *   d_out_rgb_planar [S,3,H,W];  d_out_tacc [S,H,W] (= "blend_weights");  d_flows [P,2,H,W], clipped to
 *   +-flow_clip when flow_clip > 0 (utils/utils.py:348).
 *   Per-pixel by-products fused into the same pass (each NULL to skip): d_src_u8_bgr [H,W,3] = the source frame as uint8
 *   BGR (utils/utils.py:174-177);  d_quads / d_quads_complement = mpf_build_mask_quads(d_obj_mask, 0 / 1).
 *   d_cum_mask [S,H,W] (NULL = d_mpi is already activated): d_mpi then holds the RAW last-layer output of the AdaMPI
 *   decoder and the network's activation epilogue (model/CPN/decoder.py:166-173: rgb = sigmoid(x), sigma = relu(x * cum_mask)
 *   + 1e-4) is applied in registers while the stack is streamed. */
int mpf_src_blend_flow(const float *d_mpi, const float *d_img, const float *d_params, int P, int S, int H, int W,
                       float flow_clip, float *d_out_rgba, float *d_out_rgb_planar, float *d_out_tacc,
                       float *d_flows, uint8_t *d_src_u8_bgr, const float *d_obj_mask, float *d_quads,
                       float *d_quads_complement, const float *d_cum_mask, void *stream);

/* obj_mask [H,W] -> per-texel quads (m[y,x], m[y,x+1], m[y+1,x], m[y+1,x+1]) as float4 [H,W,4], out-of-range
 * neighbours 0, of (complement ? 1 - m : m): the four bilinear taps of the mask channel in one 16-byte load.
 * (utils/utils.py:328 repeats the same [H,W] mask over all S planes; :225 passes 1 - obj_mask.) */
int mpf_build_mask_quads(const float *d_obj_mask, int complement, int H, int W, float *d_quads, void *stream);

/* Stage B - the north-star kernel.  Replaces HomographySample.sample (utils/mpi/homography_sampler.py:80-158) on the
 * 8-channel stack + render_tgt_rgb_depth's composite (utils/mpi/mpi_rendering.py:336-347 -> plane_volume_rendering
 * :62-99 -> weighted_sum_mpi :142-154), streamed per target pixel; xyz_tgt is evaluated analytically at the clamped
 * source coordinate instead of being warped as 3 extra channels.
 *   d_rgba: planar [S,4,H,W] if interleaved == 0; [S,H,W,4] if interleaved == 1; interleaved == 2 is [S,H,W,4] with the
 *   promise that at least (W+1)*16 bytes of readable, FINITE padding follow the last plane (lets the east/south taps use
 *   fixed offsets; an out-of-image tap has weight exactly 0).  d_mask_quads from mpf_build_mask_quads or NULL;
 *   d_params with S records holding H_src_tgt.  Outputs: d_rgb [3,H,W], d_depth [H,W] (NULL ok),
 *   d_objmask [H,W] (NULL iff d_mask_quads NULL), d_tgt_mask [H,W] = number of planes whose source coordinate is in
 *   range (NULL ok), d_rgb_u8_bgr [H,W,3] = the rendered frame as uint8 BGR, clip(rint(x*255)) (utils/utils.py:240-242;
 *   NULL ok).  Passing NULL for both d_depth and d_tgt_mask selects a leaner kernel body. */
int mpf_warp_composite(const float *d_rgba, int interleaved, const float *d_mask_quads, const float *d_params,
                       int S, int H, int W, float *d_rgb, float *d_depth, float *d_objmask, float *d_tgt_mask,
                       uint8_t *d_rgb_u8_bgr, void *stream);

/* Stage B on the stack as render_novel_view_dynamic receives it (utils/utils.py:291-349: mpi_all_rgb_src [1,S,3,H,W] and
 * mpi_all_sigma_src [1,S,1,H,W], two separate channel-planar tensors): the body of mpf_warp_composite reading the three colour planes
 * and the sigma plane where they lie - a tap pair of one channel row is one 8-byte load - so the caller assembles nothing (the
 * reference concatenates 8 channels per plane, utils/mpi/mpi_rendering.py:288-301).  Outputs as mpf_warp_composite; bit-identical to it.
 * mpf_warp_composite(interleaved = 0) runs the same kernel on one [S,4,H,W] tensor. */
int mpf_warp_composite_split(const float *d_rgb_S3HW, const float *d_sigma_SHW, const float *d_mask_quads, const float *d_params,
                             int S, int H, int W, float *d_rgb, float *d_depth, float *d_objmask, float *d_tgt_mask,
                             uint8_t *d_rgb_u8_bgr, void *stream);
/* Adjoint of mpf_warp_composite_split with respect to the rgb and sigma stacks (same d_params and mask quads as the forward call).  Upstream
 * gradients g_rgb [3,H,W], g_depth [H,W] (NULL ok), g_objmask [H,W] (NULL ok; needs the quads); tgt_mask has none.  Per target pixel: the forward's
 * recurrence again, a back-to-front scan, and each plane's gradient scattered through its taps with float atomic adds into grad_rgb [S,3,H,W] and
 * grad_sigma [S,H,W], which must be zero-initialised; nothing [S,C,H,W]-shaped exists in between.  Last bits depend on the order of the adds. */
int mpf_warp_composite_bwd(const float *d_rgb_S3HW, const float *d_sigma_SHW, const float *d_mask_quads, const float *d_params, int S, int H, int W,
                           const float *d_g_rgb, const float *d_g_depth, const float *d_g_objmask, float *d_grad_rgb_S3HW, float *d_grad_sigma_SHW,
                           void *stream);
/* mpf_warp_composite_bwd plus the gradient of the S plane disparities (d_grad_disparity [S]; NULL together with d_partial: exactly
 * mpf_warp_composite_bwd).  Per target pixel q and plane s the scan yields dL/dxyz_tgt_s(q) as mpf_volume_render_bwd_xyz does, the analytic field gives
 * d xyz_tgt_s(q) / d disparity_s = -depth_s (xyz_tgt_s(q) - t), and the dot product is summed over the pixels per plane without atomics (see
 * mpf_src_xyz_bwd): d_partial [tiles, S] with tiles = ceil(W/32) * ceil(H/8), partial_blocks rows.  No [S,3,H,W] gradient is written. */
int mpf_warp_composite_bwd_disp(const float *d_rgb_S3HW, const float *d_sigma_SHW, const float *d_mask_quads, const float *d_params, int S, int H, int W,
                                const float *d_g_rgb, const float *d_g_depth, const float *d_g_objmask, float *d_grad_rgb_S3HW, float *d_grad_sigma_SHW,
                                float *d_partial, int partial_blocks, float *d_grad_disparity, void *stream);

/* Stage C alone on a bare sigma tensor [S,H,W]: the volume-rendered flows of P = 1 or 2 poses (HomographySample.sample_inverse,
 * utils/mpi/homography_sampler.py:160-220, + plane_volume_rendering_flow, utils/mpi/mpi_rendering.py:102-139) - what
 * render_novel_view_dynamic needs besides the warp (utils/utils.py:340-348).  d_params as for mpf_src_blend_flow (S*P records);
 * d_flows [P,2,H,W], clipped to +-flow_clip when flow_clip > 0.  Same arithmetic as mpf_src_blend_flow's flows: bit-identical. */
int mpf_src_flow(const float *d_sigma_SHW, const float *d_params, int P, int S, int H, int W, float flow_clip, float *d_flows, void *stream);
/* hard_flow = True (utils/mpi/mpi_rendering.py:126-130): per pixel the flow of the plane with the largest rendering weight (the first one on ties, as
 * torch.argmax) instead of the weighted sum - one pass over the sigma planes, nothing per-plane materialised.  d_sigma: plane s at d_sigma + s *
 * plane_stride floats (H*W for a bare [S,H,W] tensor; 4*H*W with d_sigma = stack + 3*H*W for the [S,4,H,W] stack).  Weights with mpf_src_blend_flow's
 * arithmetic; equals mpf_homography_flow + mpf_volume_render(hard) bit for bit. */
int mpf_src_flow_hard(const float *d_sigma, int64_t plane_stride, const float *d_params, int P, int S, int H, int W, float flow_clip, float *d_flows,
                      void *stream);

/* Stage B for SEVERAL views of one stack in one launch.  The reference renders two poses of every stack
 * (utils/utils.py:210-222 with obj_mask / cam_ext and :224-236 with 1 - obj_mask / cam_ext_dynamic) and `repeat` such
 * pairs per image (gen_3dphoto_dynamic_v2.py:99-118); launched together, the views' workgroups walk the planes side by
 * side and the stack is fetched from HBM once per launch instead of once per view.  Results are bit-identical to n_views
 * calls of mpf_warp_composite.  `views` is a HOST array of n_views (<= MPF_MAX_VIEWS) descriptors holding DEVICE
 * pointers with the meaning of the same-named mpf_warp_composite arguments; it is copied into the kernel arguments, so
 * it may be reused or freed as soon as the call returns.  All views take a mask, or none does.  interleaved: 1 or 2. */
#define MPF_MAX_VIEWS 16
typedef struct MpfWarpView {
    const float *d_params;
    const float *d_mask_quads;
    float *d_rgb, *d_depth, *d_objmask, *d_tgt_mask;
    uint8_t *d_rgb_u8_bgr;
} MpfWarpView;
int mpf_warp_composite_views(const float *d_rgba, int interleaved, const MpfWarpView *views, int n_views, int S, int H,
                             int W, void *stream);

/* Stage B of one image AND Stage A+C of the NEXT image in one launch - the throughput form of the reference's unit of work
 * (utils/utils.py:190-236: one source-frame pass, :190-204 + render :7-39, then two target-frame passes, :210-236).  Run back to back
 * the two stages are an HBM-bound kernel followed by a VALU-issue-bound one; here a heterogeneous grid interleaves their workgroups
 * so that every CU holds both kinds at once.  Exactly the arithmetic of
 *     mpf_warp_composite_views(d_rgba, 2, views, n_views, S, H, W)                                              and
 *     mpf_src_blend_flow(d_mpi_next, d_img_next, d_params_next, P, S, H, W, flow_clip, d_out_rgba_next, NULL, NULL, d_flows_next,
 *                        d_src_u8_bgr_next, d_obj_mask_next, d_quads_next, d_quads_complement_next, d_cum_mask_next)
 * - results are bit-identical to those two calls; arguments have the meaning of their same-named counterparts there.
 * d_rgba (read) is a tail-padded interleaved stack (interleaved == 2); d_out_rgba_next (written) must be a DIFFERENT buffer, and so
 * must every *_next output be from anything the views read or write: the two halves of the launch are unordered. */
int mpf_warp_views_and_blend_next(const float *d_rgba, const MpfWarpView *views, int n_views,
                                  const float *d_mpi_next, const float *d_img_next, const float *d_params_next, int P,
                                  float flow_clip, float *d_out_rgba_next, float *d_flows_next, uint8_t *d_src_u8_bgr_next,
                                  const float *d_obj_mask_next, float *d_quads_next, float *d_quads_complement_next,
                                  const float *d_cum_mask_next, int S, int H, int W, void *stream);

/* The same launch with Stage D (mpf_merge) of an EARLIER pair folded in: the Stage A+C role runs it as a per-pixel prologue, so a stream
 * of pairs is ONE launch per pair with nothing between two launches (pipeline.OverlappedPairRenderer(merge_in_launch=True): pair i's
 * Stage A+C in launch i, its Stage B in launch i+1, its merge in launch i+2).  merge_prev = mpf_merge's arguments (NULL: plain
 * mpf_warp_views_and_blend_next).  Its d_flow / d_flow_dyn MAY be (parts of) d_flows_next - the thread that merges a pixel is the one that
 * later writes that pixel's new flows; its frames / masks must not be the views this launch renders. */
typedef struct MpfMergeArgs {
    const float *d_frame, *d_frame_dyn;        /* [3,H,W] the two rendered views */
    const float *d_mask, *d_mask_dyn;          /* [H,W] their rendered object masks */
    const float *d_flow, *d_flow_dyn;          /* [2,H,W] the two volume-rendered flows */
    const float *d_obj_mask;                   /* [H,W] source-frame object mask (see obj_mask_stride) */
    float thresh;
    float *d_flow_mix;                         /* [H,W,2] */
    uint8_t *d_frame_mix, *d_fill_mask;        /* [H,W,3] BGR, [H,W] */
    int obj_mask_stride;                       /* floats between consecutive pixels of d_obj_mask: 0 | 1 = a plain [H,W] map; 4 = the first component of a
                                                  mask-quad buffer [H,W,4] (what Stage A+C wrote for that pair: quads[n].x == obj_mask[n]) - lets a pipelined
                                                  caller merge a pair from buffers it owns, whatever happened to the caller's mask tensor since */
} MpfMergeArgs;
int mpf_warp_views_blend_next_merge_prev(const float *d_rgba, const MpfWarpView *views, int n_views,
                                         const float *d_mpi_next, const float *d_img_next, const float *d_params_next, int P,
                                         float flow_clip, float *d_out_rgba_next, float *d_flows_next, uint8_t *d_src_u8_bgr_next,
                                         const float *d_obj_mask_next, float *d_quads_next, float *d_quads_complement_next,
                                         const float *d_cum_mask_next, int S, int H, int W, const MpfMergeArgs *merge_prev, void *stream);

/* ---- mask support maps: Stage B tiles the merge cannot read are not rendered ----------------------------------------------------
 * The merge (utils/utils.py:270-283) takes a view's rgb only where that view's composited object mask reaches the threshold, and that mask
 * is sum_s weights_s * warped_mask_s (utils/mpi/mpi_rendering.py:95-96): exactly 0 wherever every bilinear tap of the mask is 0 on every
 * plane.  The reference renders view 0 with obj_mask - ONE instance of the image (gen_3dphoto_dynamic_v2.py:101-105) - and view 1 with
 * 1 - obj_mask (utils/utils.py:210-236), so most target tiles of view 0 see no mask at all.
 *   A SUPPORT MAP is a uint32 [ceil(H / MPF_SUPPORT_CELL_H), ceil(W / MPF_SUPPORT_CELL_W)] over the source frame.  Stage A+C, where it writes a
 * mask-quad buffer, stores `tag` into every cell that holds a quad with a non-zero component (-0.0 counts as zero); other cells are left
 * alone.  Stage B, given (d_cells, tag) for a view, treats the cells EQUAL to tag as live: give every pair a tag of its own (a counter;
 * start from a zeroed map and tag 1) and a map never needs clearing.  A Stage B tile (32 x 8 target pixels) is DEAD when on every plane the
 * homography's denominator is finite and positive at the tile's four corner pixels and the corners' bounding box, widened by one texel
 * and clamped to the frame, touches no live cell; everything else is rendered as before.
 *   OUTPUT CONTRACT with a support map: a view's d_rgb / d_objmask / d_rgb_u8_bgr hold the full render's values except on dead tiles, where
 * d_objmask is 0 (the full render's value there for finite inputs) and d_rgb / d_rgb_u8_bgr are 0 (the full render's value is never selected
 * by mpf_merge with thresh > 0).  flow_mix / frame_mix / fill_mask of the merge are bit-identical to the full render's.
 *   A view renders every tile (the launcher decides, per view) when d_cells is NULL, when thresh <= 0 (then `0 >= thresh` selects the view),
 * or when it asks for d_depth or d_tgt_mask, which do not depend on the mask. */
#define MPF_SUPPORT_CELL_W 32
#define MPF_SUPPORT_CELL_H 8
#define MPF_SUPPORT_CELLS(H, W) ((((H) + MPF_SUPPORT_CELL_H - 1) / MPF_SUPPORT_CELL_H) * (((W) + MPF_SUPPORT_CELL_W - 1) / MPF_SUPPORT_CELL_W))
typedef struct MpfViewSupport {
    const uint32_t *d_cells;     /* the support map of the view's d_mask_quads, or NULL */
    uint32_t tag;                /* the value live cells carry */
    float thresh;                /* the threshold the views will be merged with */
} MpfViewSupport;

/* mpf_src_blend_flow that also writes the support maps of d_quads / d_quads_complement (each optional, needs its quads). */
int mpf_src_blend_flow_support(const float *d_mpi, const float *d_img, const float *d_params, int P, int S, int H, int W,
                               float flow_clip, float *d_out_rgba, float *d_out_rgb_planar, float *d_out_tacc,
                               float *d_flows, uint8_t *d_src_u8_bgr, const float *d_obj_mask, float *d_quads,
                               float *d_quads_complement, const float *d_cum_mask, uint32_t *d_support, uint32_t *d_support_complement,
                               uint32_t tag, void *stream);
/* mpf_warp_composite_views with one MpfViewSupport per view (`supports`: host array of n_views, or NULL = mpf_warp_composite_views). */
int mpf_warp_composite_views_support(const float *d_rgba, int interleaved, const MpfWarpView *views, const MpfViewSupport *supports, int n_views,
                                     int S, int H, int W, void *stream);
/* mpf_warp_views_blend_next_merge_prev: the views test `supports`, the Stage A+C role writes the next pair's maps with tag_next.  A map
 * this launch writes must not be one it tests (the two halves are unordered); outputs otherwise equal the two stand-alone calls above. */
int mpf_warp_views_blend_next_merge_prev_support(const float *d_rgba, const MpfWarpView *views, const MpfViewSupport *supports, int n_views,
                                                 const float *d_mpi_next, const float *d_img_next, const float *d_params_next, int P,
                                                 float flow_clip, float *d_out_rgba_next, float *d_flows_next, uint8_t *d_src_u8_bgr_next,
                                                 const float *d_obj_mask_next, float *d_quads_next, float *d_quads_complement_next,
                                                 const float *d_cum_mask_next, uint32_t *d_support_next, uint32_t *d_support_complement_next,
                                                 uint32_t tag_next, int S, int H, int W, const MpfMergeArgs *merge_prev, void *stream);
/* The device's decision itself: d_dead [n_views, ceil(H/8) * ceil(W/32)] uint8, 1 where the launches above skip the tile (row-major tiles). */
int mpf_support_dead_tiles(const MpfWarpView *views, const MpfViewSupport *supports, int n_views, int S, int H, int W, uint8_t *d_dead, void *stream);

/* Stage D.  Replaces utils/utils.py:237-283 (uint8 BGR conversion, threshold, layer select, fill mask).
 * frames [3,H,W] RGB float, masks [H,W], flows [2,H,W], obj_mask [H,W] ->
 * d_flow_mix [H,W,2] f32, d_frame_mix [H,W,3] u8 BGR, d_fill_mask [H,W] u8 (1 = hole to inpaint). */
int mpf_merge(const float *d_frame, const float *d_frame_dyn, const float *d_mask, const float *d_mask_dyn,
              const float *d_flow, const float *d_flow_dyn, const float *d_obj_mask, float thresh, int H, int W,
              float *d_flow_mix, uint8_t *d_frame_mix, uint8_t *d_fill_mask, void *stream);

/* mpf_merge with its arguments as the struct (obj_mask_stride honoured) */
int mpf_merge_ex(const MpfMergeArgs *args, int H, int W, void *stream);

/* The depth-ordered variant of Stage D's frame ("utils/utils copy.py":278-303, the reference's older per-image module): frame_mix as
 * mpf_merge computes it, except that where both layers cover the pixel (both masks non-zero) and depth > depth_dyn the dynamic layer's
 * pixel is taken.  depths [H,W] are the two views' composited depths (mpf_warp_composite's d_depth).
 * -> d_frame_mix_depth [H,W,3] u8 BGR; d_depth_mask [H,W] u8 (optional, may be NULL): 1 where the dynamic layer was picked. */
int mpf_merge_depth_ordered(const float *d_frame, const float *d_frame_dyn, const float *d_mask, const float *d_mask_dyn,
                            const float *d_depth, const float *d_depth_dyn, float thresh, int H, int W,
                            uint8_t *d_frame_mix_depth, uint8_t *d_depth_mask, void *stream);

/* Built-in hole fill used when OpenCV is absent (NOT cv2.inpaint's Navier-Stokes / Telea, utils/utils.py:284-286,
 * moving_obj.py:162; row A13 is parity-unpinned): onion peel - pass k gives every hole pixel that touches
 * a pixel known after pass k-1 the rounded mean of those 8-neighbours.  In place on d_img u8 [H,W,3]; d_hole u8 [H,W]
 * (1 = hole) is cleared where filled (holes without any known pixel in their connected region stay 1).  One launch
 * sequence on the stream, no host round trip.  d_workspace: mpf_fill_holes_workspace(H, W) bytes. */
size_t mpf_fill_holes_workspace(int H, int W);
int mpf_fill_holes(uint8_t *d_img, uint8_t *d_hole, int H, int W, void *d_workspace, size_t workspace_bytes, void *stream);

/* The reference's own hole filling, on the HOST (host pointers, synchronous, re-entrant, no GPU involved): OpenCV's
 * cv2.inpaint(img, mask, radius, flags) for flags = cv2.INPAINT_NS (utils/utils.py:284-286: frame_mix, fill_mask, radius 3)
 * and cv2.INPAINT_TELEA (moving_obj.py:162: im1_raw, 1 - H, radius 3) - the fast-marching front of modules/photo/src/inpaint.cpp
 * with its order of operations (third-party arithmetic: parity with cv2 itself is unpinned until a test has run next to a real
 * cv2).  img u8 [H,W,C] (C = 1 or 3), mask u8 [H,W] (non-zero = fill), out u8 [H,W,C] (may not alias img).
 * Filling is sequential by nature (every pixel reads pixels filled before it), so callers run one frame per host thread. */
#define MPF_INPAINT_NS 0
#define MPF_INPAINT_TELEA 1
int mpf_inpaint_host(const uint8_t *img, const uint8_t *mask, int H, int W, int C, double radius, int method, uint8_t *out);

/* The NS branch of mpf_inpaint_host on the GPU, byte for byte: cv2.inpaint(frame_mix, fill_mask, 3, cv2.INPAINT_NS) (utils/utils.py:284-286)
 * for a batch of B frames.  d_img u8 [B,H,W,3] (BGR, as frame_mix), d_mask u8 [B,H,W] (non-zero = fill) -> d_out u8 [B,H,W,3] (may not
 * alias the inputs).  The hole pixels of a frame fall into clusters (holes within Chebyshev distance radius + 1 of each other) whose
 * fast-marching fronts never read each other's pixels; each cluster runs the serial front on one wave (mpf_inpaint_ns.hip).  radius
 * is rounded and clamped like cvInpaint; 1 - 4 are supported (MPF_ERR_UNSUPPORTED otherwise), as are H, W >= 2 only.  Stream-ordered,
 * no host synchronisation, no allocation; arguments are validated before any device work.
 * d_ws: mpf_inpaint_ns_workspace(B, H, W, radius) bytes, about 45 per pixel of the frames padded by one (per padded pixel: flag 1, T 4,
 * union-find parent 4, cluster list 4, bounding box 16, heap pool 16 - all sized for the worst case of one cluster per hole pixel and a
 * heap holding every band and hole pixel; ~110 MB for 5 frames of 384 x 1280).
 * After the call has completed, the first 32-bit words of d_ws hold: [0] clusters, [1] (work counter), [2] heap pool items handed out,
 * [3] clusters whose heap started in the pool (band > 2048 pixels), [4] clusters whose heap moved to the pool while running,
 * [5] clusters left unfilled because a bound the fill relies on broke (always 0 unless the kernel is wrong). */
size_t mpf_inpaint_ns_workspace(int B, int H, int W, double radius);
int mpf_inpaint_ns(const uint8_t *d_img, const uint8_t *d_mask, int B, int H, int W, double radius, uint8_t *d_out, void *d_ws,
                   size_t ws_bytes, void *stream);

/* End-of-batch statistics of one pair, without a host round trip: d_out holds
 * MPF_PAIR_STATS_SLICES rows of 4 doubles, one per fixed contiguous slice of the frame:
 * { sum |flow|, hole pixels, max |flow|, max(-flow) } of d_flow_mix [H,W,2] f32 / d_fill_mask [H,W] u8 (empty slices: 0, 0,
 * -inf, -inf).  Sum the first two columns and take the maximum of the last two.  Deterministic summation order. */
#define MPF_PAIR_STATS_SLICES 64
int mpf_pair_stats(const float *d_flow_mix, const uint8_t *d_fill_mask, int H, int W, double *d_out, void *stream);

/* Measurement aid (bench.py `hbm_reference`; SURVEY.md 8(d) asks for an on-box streaming figure beside the 8 TB/s specification):
 * mode 0 reads `bytes` from d_src with 16-byte loads (d_dst: one float, never written for ordinary data), mode 1 copies d_src to
 * d_dst.  16-byte aligned device buffers, bytes a multiple of 16.  No counterpart in the reference. */
int mpf_stream_probe(const void *d_src, void *d_dst, size_t bytes, int mode, void *stream);

/* Frame -> PNG scanlines on the device (what cv2.imwrite does first, utils/utils.py:240-242 / gen_3dphoto_dynamic_v2.py:121-122):
 * d_bgr u8 [H,W,3] -> d_scanlines u8 [H, 1 + 3W]: filter byte 2 ("Up") followed by the RGB row minus the previous row
 * (mod 256).  The host only deflates these bytes and wraps them in chunks (mpiflow_amd/io_formats.py). */
int mpf_png_filter_up(const uint8_t *d_bgr, int H, int W, uint8_t *d_scanlines, void *stream);

/* Training batches from rendered pairs (mpiflow_amd/online.py): RAFT's FlowAugmentor.spatial_transform (resize, flips, crop;
 * RAFT/core/utils/augmentor.py:67-109) and its dataset's tensor packing (RAFT/core/datasets.py:85-90) in one pass.  One
 * MpfAugmentSample per sample, in a HOST array of B (read by the launcher; the pointers in it are device pointers):
 *   src, dst  u8 [H,W,3] BGR (image 1 = the source frame, image 2 = the filled target frame);  flow  f32 [H,W,2] (flow_mix)
 *   resize    0: Hr == H, Wr == W, no resampling;  1: cv2 INTER_LINEAR to Hr x Wr (cv2: Wr = rint(W*scale_x), Hr = rint(H*scale_y)),
 *             source coordinate (float)((d + 0.5) * (1.0 / scale) - 0.5), fp32 interpolation horizontal first, flow * (scale_x, scale_y)
 *             in double then rounded to float
 *   flip_h / flip_v  mirror the resized frame (and negate u / v);  y0, x0  crop origin in the resized, flipped frame
 * -> d_image1, d_image2 f32 [B,3,h,w] RGB 0..255 (rintf, clamped);  d_flow f32 [B,2,h,w];  d_valid f32 [B,h,w] = |u| < 1000 && |v| < 1000.
 * Identity (resize 0, no flips, crop = frame) reproduces the inputs exactly.  Validated before anything is launched (null pointers,
 * B < 1, resize == 0 with Hr x Wr != H x W, a crop outside the resized frame).  One launch per 32 samples.  cv2's own u8 resize
 * rounds 11-bit fixed-point weights and may differ by one LSB: unpinned (see mpf_augment.hip). */
typedef struct MpfAugmentSample {
    const uint8_t *src;
    const uint8_t *dst;
    const float *flow;
    int resize;
    double scale_x, scale_y;
    int Hr, Wr;
    int flip_h, flip_v;
    int y0, x0;
} MpfAugmentSample;
int mpf_augment_pairs(const MpfAugmentSample *s, int B, int H, int W, int h, int w, float *image1, float *image2, float *flow, float *valid,
                      void *stream);

/* The sparse path of RAFT's loader (its KITTI stage): SparseFlowAugmentor.spatial_transform (RAFT/core/utils/augmentor.py:194-232) with
 * resize_sparse_flow_map's nearest-pixel scatter (:160-192), after KITTI's 16-bit flow code (writeFlowKITTI -> readFlowKITTI,
 * core/utils/frame_utils.py:102-120), and the dataset's packing.  Same outputs and layout as mpf_augment_pairs.  One MpfSparseAugmentSample
 * per sample, in a HOST array of B (device pointers):
 *   src, dst  u8 [H,W,3] BGR;  flow  f32 [H,W,2];  valid  u8 [H,W], nonzero = valid, NULL = every pixel valid (what writeFlowKITTI writes)
 *   quantize  1: t = 64.0f*u + 32768.0f in fp32 (each operation rounded), q = trunc(t), u_q = (float)(q - 32768) / 64.0f, the same for v.
 *             A pixel whose t lies outside -1 < t < 65536 for either component is INVALID: the reference's uint16 cast is undefined
 *             there, so that rule is this library's.  0: u_q = u, v_q = v.
 *   resize, scale_x, scale_y, Hr, Wr, flip_h, y0, x0  as MpfAugmentSample (no v-flip); the images take exactly mpf_augment_pairs' path.
 * Flow and valid per output pixel, (Y, X) = its pixel in the Hr x Wr map after the crop and the flip:
 *   resize 0: the source pixel (Y, X); valid = its validity; flow (u_q, v_q), 0 where invalid.
 *   resize 1: the gather form of the scatter.  X < 1 or Y < 1: 0, 0, valid 0 (the scatter never writes row 0 or column 0).  Else the
 *             candidate rows are {ys : rint((double)ys * scale_y) == Y}, the candidate columns {xs : rint((double)xs * scale_x) == X}
 *             (rint: half to even, in double); the largest ys with a valid candidate xs, then the largest such xs, wins (numpy's last
 *             writer in raster order): flow ((float)((double)u_q * scale_x), (float)((double)v_q * scale_y)), valid 1.  No valid candidate:
 *             0, 0, valid 0 (a hole).
 *   flip_h negates u after all of this (a hole's 0 becomes -0.0, as RAFT's `flow * [-1.0, 1.0]` does); valid is mirrored, not negated.
 * -> d_image1, d_image2 f32 [B,3,h,w] RGB;  d_flow f32 [B,2,h,w];  d_valid f32 [B,h,w] (0 / 1).  Validated before anything is launched
 * (null pointers, B < 1, flags other than 0 / 1, resize == 0 with Hr x Wr != H x W, a scale <= 0, a crop outside the resized frame).
 * One launch per 32 samples.  Contract in full: mpf_augment_sparse.hip. */
typedef struct MpfSparseAugmentSample {
    const uint8_t *src;
    const uint8_t *dst;
    const float *flow;
    const uint8_t *valid;
    int quantize;
    int resize;
    double scale_x, scale_y;
    int Hr, Wr;
    int flip_h;
    int y0, x0;
} MpfSparseAugmentSample;
int mpf_augment_sparse_pairs(const MpfSparseAugmentSample *s, int B, int H, int W, int h, int w, float *image1, float *image2, float *flow,
                             float *valid, void *stream);

/* The photometric half of RAFT's FlowAugmentor (color_transform + eraser_transform, RAFT/core/utils/augmentor.py:36-65), which it runs on the
 * full-size u8 frames before spatial_transform: run it before mpf_augment_pairs, whose src / dst it writes.  One MpfPhotoSample per sample,
 * in a HOST array of B (the pointers in it are device pointers):
 *   src, dst  u8 [H,W,3] BGR (image 1, image 2), read with RGB semantics (R = byte 2);  src_out, dst_out  u8 [H,W,3] BGR results (may be
 *             src / dst themselves; no other overlap)
 *   jitter    torchvision ColorJitter on a PIL RGB image: the ops order[0 .. n_ops) in that order, 0 brightness blend(0, x, f),
 *             1 contrast blend(m, x, f) with m = int(sumL / n + 0.5) over the image as it stands before the op, 2 saturation
 *             blend(L(x), x, f), 3 hue: PIL's RGB -> HSV, H = (H + hue_shift) & 255, PIL's HSV -> RGB (lossy even at shift 0).
 *             L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16;  blend(a, x, f) = (float)a + f * (float)(x - a) in fp32, clamped, truncated.
 *   joint     1: jitter[0] on both frames, one contrast mean over both (RAFT's symmetric jitter of the stacked pair);  0: jitter[0] on src,
 *             jitter[1] on dst, each its own mean
 *   n_rect, rect  0..2 rectangles {x0, y0, dx, dy} filled, after the jitter, on dst_out with its mean colour sum_c // (H W) (RAFT's eraser);
 *             clipped at the frame edge
 * d_workspace: mpf_photometric_workspace(B) bytes, 8-byte aligned; zeroed on the stream by the call.  Validated before anything is launched
 * (null pointers, B < 1, a bad shape, op orders that are not distinct values in 0..3, non-finite or negative factors, a hue shift outside
 * -128..127, n_rect outside 0..2, a rectangle origin outside the frame or an extent < 1, a short or misaligned workspace).  At most three
 * launches per 32 samples; integer sums with integer atomics: repeated runs are byte-identical.  Contract in full: mpf_photometric.hip. */
typedef struct MpfPhotoJitter {
    int n_ops;                   /* 0..4 */
    int order[4];                /* op codes of the chain, order[0] first */
    float brightness, contrast, saturation;   /* factors, finite, >= 0 (read when their op is in the chain) */
    int hue_shift;               /* int(hue * 255.0) truncated toward zero, -128..127 */
} MpfPhotoJitter;
typedef struct MpfPhotoSample {
    const uint8_t *src;
    const uint8_t *dst;
    uint8_t *src_out;
    uint8_t *dst_out;
    int joint;
    MpfPhotoJitter jitter[2];
    int n_rect;
    int rect[2][4];              /* x0, y0, dx, dy */
} MpfPhotoSample;
size_t mpf_photometric_workspace(int B);
int mpf_photometric_pairs(const MpfPhotoSample *s, int B, int H, int W, void *d_workspace, size_t workspace_bytes, void *stream);

/* RAFT's on-demand correlation lookup (RAFT/alt_cuda_corr, called by AlternateCorrBlock, RAFT/core/corr.py:63-91): the 81 * L window of
 * correlations around each query pixel's current match, from the two feature maps, without the all-pairs volume.  All maps channel-last:
 *   fmap1   f32 [B,H,W,C];  f2[i]  f32 [B,Hl[i],Wl[i],C], level i of fmap2's average-pooled pyramid (i < levels);  coords  f32 [B,2,H,W],
 *   (x, y) in pixels of level 0;  rd = 2 * radius + 1
 *   out[b, i*rd*rd + a*rd + c, y, x] = scale * sum_ch fmap1[b,y,x,ch] * bilinear(f2[i][b,:,:,ch], X, Y),
 *       X = coords[b,0,y,x] / 2^i + (a - radius),  Y = coords[b,1,y,x] / 2^i + (c - radius)      (the FIRST window index moves x, as RAFT's does)
 *   bilinear: the four integer taps around (floor X, floor Y), a tap outside the level contributes 0 (grid_sample, align_corners, zero padding).
 *   Evaluated as RAFT's kernel does: the (rd+1)^2 dot products on the integer grid around (floor x, floor y), then the four-tap blend of those.
 * coords are UNTRUSTED: any value is legal.  A coordinate that is NaN, +-inf, or so far out that no tap can lie in the level puts every tap of
 * that pixel and level outside: its outputs are exactly 0 and it adds nothing to any gradient.  (It is clamped in floating point before the
 * conversion to int; no value of coords makes the kernels touch memory outside the buffers.)
 * mpf_corr_lookup           writes out f32 [B, levels*rd*rd, H, W]; one launch for all levels.
 * mpf_corr_lookup_backward  reads out as the cotangent [B, levels*rd*rd, H, W]; WRITES grad_fmap1 f32 [B,H,W,C] (a per-pixel sum: bit-identical
 *                           from run to run) and ADDS into grad_f2[i] f32 [B,Hl[i],Wl[i],C] with fp32 atomics (the caller zeroes them; sums
 *                           differ in the last bits from run to run).  No gradient for coords (RAFT detaches them before every lookup).
 * fp32 throughout.  C a multiple of 32; radius 1..8; levels 1..MPF_CORR_MAX_LEVELS; every level at least 2 x 2 (H, W >= 2^levels for a pooled
 * pyramid: below that the reference's own sampler divides by zero); maps 16-byte aligned; every map below 2^31 elements.  Validated before
 * anything is launched.  plain = 1 selects the first form of the forward kernel (one thread per output entry, four gathered taps, no sharing):
 * kept as the same-box yardstick of tools/bench_corr.py and as a cross-check in the tests; same contract, same results up to rounding. */
#define MPF_CORR_MAX_LEVELS 6
typedef struct MpfCorrArgs {
    const float *fmap1;
    const float *f2[MPF_CORR_MAX_LEVELS];
    const float *coords;
    float *out;                              /* forward: written;  backward: the cotangent, read */
    float *grad_fmap1;                       /* backward only */
    float *grad_f2[MPF_CORR_MAX_LEVELS];     /* backward only */
    int B, C, H, W;
    int Hl[MPF_CORR_MAX_LEVELS], Wl[MPF_CORR_MAX_LEVELS];
    int radius, levels;
    float scale;                             /* RAFT: 1 / sqrt(C) */
    int plain;
} MpfCorrArgs;
int mpf_corr_lookup(const MpfCorrArgs *a, void *stream);
int mpf_corr_lookup_backward(const MpfCorrArgs *a, void *stream);

/* RAFT's all-pairs correlation block (CorrBlock, RAFT/core/corr.py:12-60): the pyramid of the volume, the lookup of every level in one launch, and
 * both gradients.  The three GEMMs (raw = fmap1^T fmap2; grad_fmap1, grad_fmap2 from the folded gradient) are the caller's.
 *   level[i]  f32 [B*H*W, Hl[i], Wl[i]], Hl[i] = H >> i, Wl[i] = W >> i (chained 2 x 2 average pooling with floor sizes): ROW p of every level is
 *             query pixel p = (b*H + y)*W + x against all of frame 2.  Either the pyramid itself or its gradient, see the calls.
 *   coords    f32 [B,2,H,W], (x, y) in pixels of level 0;  rd = 2 * radius + 1
 *   out[b, i*rd*rd + a*rd + c, y, x] = bilinear(level[i][p], X, Y),   X = coords[b,0,y,x] / 2^i + (a - radius),  Y = coords[b,1,y,x] / 2^i + (c - radius)
 *             (the FIRST window index moves x); bilinear as for mpf_corr_lookup: four integer taps, a tap outside the level contributes 0.
 * mpf_corr_pyramid                 level[0] holds the raw product on entry: divides it by norm IN PLACE and writes level[1 .. levels-1]
 *                                  (torch's avg_pool2d: ((a00 + a01) + a10) + a11, times 1/4; each level from the rounded one before it).
 * mpf_corr_volume_lookup           reads level[], writes out f32 [B, levels*rd*rd, H, W]; one launch for all levels; each pixel reads the (rd+1)^2
 *                                  patch of its own row once per level.
 * mpf_corr_volume_lookup_backward  reads out as the cotangent; ADDS its gradient into level[] (the caller's gradient pyramid, zeroed once by the
 *                                  caller, shared by any number of lookups).  One thread owns every entry it updates (a lookup of pixel p touches
 *                                  row p only): plain loads and stores, no atomics, bit-identical from run to run.  Calls that share a gradient
 *                                  pyramid must be ordered (one stream, or events).  No gradient for coords.
 * mpf_corr_pyramid_backward        level[] holds the gradient pyramid: folds it into the gradient of the raw product, IN PLACE in level[0]:
 *                                  level[0][p,y,x] = (g0 + (g1[y>>1, x>>1] + (g2[y>>2, x>>2] + ...) / 4) / 4) / norm, a level taking part where it covers
 *                                  (y, x) (floor pooling drops a last odd row / column).  level[1 ..] are read only.
 * coords are UNTRUSTED, as for mpf_corr_lookup: NaN, +-inf and far-out values give exactly 0 and add nothing to the gradient; they are clamped in
 * floating point before the conversion to int and no value makes a kernel touch memory outside its buffers.  Row offsets are 64-bit (B*H*W*H*W
 * may exceed 2^31).  fp32 throughout.  levels 1..MPF_CORR_MAX_LEVELS; every level at least 2 x 2.  Lookup calls: radius 1..8, level[] 4-byte
 * aligned.  Pyramid calls: level[] 16-byte aligned (level 0 moves 16 bytes per lane where W allows), norm finite and not 0, and
 * W * 2^(levels-1) <= 12288 (mpf_corr_pyramid pools one strip of 2^(levels-1) image rows in LDS; mpf_corr_pyramid_backward uses no LDS but takes
 * the same shapes and no others: a pyramid that cannot be built has no gradient).  Validated before anything is launched. */
typedef struct MpfCorrVolumeArgs {
    float *level[MPF_CORR_MAX_LEVELS];       /* the pyramid (pyramid: written; lookup: read) or its gradient (lookup backward: added to; pyramid backward: folded) */
    const float *coords;                     /* lookup calls */
    float *out;                              /* lookup: written;  lookup backward: the cotangent, read */
    int B, H, W;
    int Hl[MPF_CORR_MAX_LEVELS], Wl[MPF_CORR_MAX_LEVELS];
    int radius, levels;
    float norm;                              /* pyramid calls; RAFT: sqrt(C) in float32 */
} MpfCorrVolumeArgs;
int mpf_corr_pyramid(const MpfCorrVolumeArgs *a, void *stream);
int mpf_corr_volume_lookup(const MpfCorrVolumeArgs *a, void *stream);
int mpf_corr_volume_lookup_backward(const MpfCorrVolumeArgs *a, void *stream);
int mpf_corr_pyramid_backward(const MpfCorrVolumeArgs *a, void *stream);

/* RAFT's convex upsampling (RAFT.upsample_flow, RAFT/core/raft.py:72-83) and the per-prediction term of its sequence loss (RAFT/train.py:47-72),
 * fused.  All tensors f32, contiguous:
 *   flow  [N,2,H,W];  mask  [N,576,H,W], channel k*64 + i*8 + j = tap k = ky*3 + kx, sub-row i, sub-column j
 *   p[k,i,j]           = softmax over k of mask[n, k*64+i*8+j, h, w]                       (max-subtracted)
 *   out[n,c,8h+i,8w+j] = sum_k p[k,i,j] * 8 * flow[n, c, h+ky-1, w+kx-1]                   (a neighbour outside the map is 0 and keeps its weight)
 * mpf_upsample_flow            writes out f32 [N,2,8H,8W].
 * mpf_upsample_flow_backward   reads out as the cotangent [N,2,8H,8W], recomputes the softmax; WRITES grad_flow [N,2,H,W] and grad_mask [N,576,H,W].
 * mpf_flow_loss_term           never forms out in memory.  flow_gt f32 [N,2,8H,8W], valid f32 [N,8H,8W];
 *                                  v = (valid >= 0.5) & (sqrt(gt_u^2 + gt_v^2) < max_flow)   (fp32),   S = sum over all entries of v * |out - flow_gt|
 *                              writes term[0] = S / (N*2*8H*8W) (f32, device).  With metrics != NULL it also writes five f64 accumulators of THIS
 *                              prediction to metrics[0..4]: sum of epe over v, the counts of epe < 1, < 3, < 5 over v, and the count of v
 *                              (epe = sqrt(du^2 + dv^2) in fp32).
 * mpf_flow_loss_term_backward  g: ONE f32 on the device, the gradient that reaches term (read by the kernel: no host synchronisation).  WRITES grad_flow
 *                              and grad_mask for the cotangent g / (N*2*8H*8W) * v * sign(out - flow_gt), sign(0) = 0.
 * workspace: mpf_upsample_workspace(N, H, W, backward) bytes of device memory, 8-byte aligned, contents irrelevant before and after the call
 * (backward = 0: the loss term's per-block partials; backward = 1: the two backward calls' tap sums [N,2,9,H,W]); mpf_upsample_flow needs none.
 * No floating-point atomics: the sums are per-block partials folded in a fixed order (in fp64), grad_flow is gathered from the tap sums, so every
 * output is bit-identical from run to run.  The mask is read once per call and nothing of its size is written by the forward calls.
 * Any N, H, W >= 1 with N*576*H*W < 2^31; out, flow_gt and valid 16-byte aligned.  Tensor VALUES are unrestricted: NaN and inf propagate as they
 * do in torch and no value changes an address.  Validated before anything is launched (MPF_ERR_BAD_ARGUMENT). */
typedef struct MpfUpsampleArgs {
    const float *flow;
    const float *mask;
    float *out;                  /* upsample forward: written;  upsample backward: the cotangent, read;  loss calls: unused */
    const float *flow_gt;        /* loss calls */
    const float *valid;          /* loss calls */
    const float *g;              /* loss backward: device scalar */
    float *term;                 /* loss forward: device scalar, written */
    double *metrics;             /* loss forward: NULL or 5 doubles on the device, written */
    float *grad_flow;            /* backward calls */
    float *grad_mask;            /* backward calls */
    void *workspace;
    size_t workspace_bytes;
    int N, H, W;
    float max_flow;              /* RAFT: 400 */
} MpfUpsampleArgs;
size_t mpf_upsample_workspace(int N, int H, int W, int backward);   /* 0 for a shape the calls refuse */
int mpf_upsample_flow(const MpfUpsampleArgs *a, void *stream);
int mpf_upsample_flow_backward(const MpfUpsampleArgs *a, void *stream);
int mpf_flow_loss_term(const MpfUpsampleArgs *a, void *stream);
int mpf_flow_loss_term_backward(const MpfUpsampleArgs *a, void *stream);

/* The same loss term for the small model, which has no mask: its prediction is upflow8(flow) = 8 * bilinear(flow), align_corners = true (mpf_upflow8
 * below, whose coordinate arithmetic these calls share operation for operation: the scale (H-1)/(8H-1) rounded once in fp32, 0 for H == 1).
 * They take the same MpfUpsampleArgs; mask, out and grad_mask are ignored.
 * mpf_upflow8_loss_term           flow [N,2,H,W], flow_gt [N,2,8H,8W], valid [N,8H,8W], max_flow; the prediction is formed in registers and never
 *                                 stored.  v, S, term[0] = S / (N*2*8H*8W) and, with metrics != NULL, the five f64 accumulators: as mpf_flow_loss_term.
 * mpf_upflow8_loss_term_backward  g: ONE f32 on the device.  WRITES grad_flow [N,2,H,W] for the cotangent g / (N*2*8H*8W) * v * sign(pred - flow_gt),
 *                                 sign(0) = 0 and a NaN difference gives 0.  The prediction is recomputed; nothing of full-resolution size is written.
 *                                 A gather per coarse pixel over the fine pixels that read it, summed in fp64 in a fixed order.
 * workspace: mpf_upflow8_loss_workspace(N, H, W, backward) bytes, 8-byte aligned (backward = 0: per-block partials; backward = 1: 0, the gather needs
 * none and the field is ignored).  No atomics: every output is bit-identical from run to run.
 * Any N, H, W >= 1 with N*2*8H*8W < 2^31; flow_gt and valid 16-byte aligned.  Tensor VALUES are unrestricted: NaN and inf propagate as they do in
 * torch and no value changes an address.  Validated before anything is launched (MPF_ERR_BAD_ARGUMENT). */
size_t mpf_upflow8_loss_workspace(int N, int H, int W, int backward);   /* 0 for a shape the calls refuse; 0 for backward */
int mpf_upflow8_loss_term(const MpfUpsampleArgs *a, void *stream);
int mpf_upflow8_loss_term_backward(const MpfUpsampleArgs *a, void *stream);

/* The pointwise work of RAFT's convolutional GRU (ConvGRU / SepConvGRU, RAFT/core/update.py:16-60) between its gate convolutions, fused.
 * All tensors f32, NCHW, contiguous.  A pre-activation is the sum of up to MPF_GRU_MAX_TERMS terms; a term is the channel slice
 * [offset, offset + C) of a tensor [B,channels,H,W], read in place; p = NULL: the term is absent (one of the counted terms must be present).
 * Gradients of pre-activations are written the same way, each to up to two slices (index 0 required, index 1 optional).
 *   mpf_gru_reset            out = rh = sigmoid(sum r) * h                                                           [B,C,H,W]
 *   mpf_gru_update           z = sigmoid(sum z), q = tanh(sum q);  out = h' = (1 - z) * h + z * q                    [B,C,H,W]
 *   mpf_gru_update_backward  g = grad h'; recomputes z, q;  dz <- g (q - h) z (1 - z),  dq <- g z (1 - q^2),  dh = g (1 - z)   (dh WRITTEN)
 *   mpf_gru_reset_backward   g = grad rh; recomputes r;     dr <- g h r (1 - r);  dh = g r, or dh += g r with accumulate != 0
 * 16-byte accesses when H*W % 4 == 0 and every pointer (slice offsets applied) is 16-byte aligned, 4-byte ones otherwise: any B, C, H, W >= 1
 * with every tensor below 2^31 elements.  No atomics: bit-identical from run to run.  Tensor VALUES are unrestricted: NaN and inf propagate as
 * they do in torch and no value changes an address.  Outputs must not overlap inputs (dh with accumulate excepted).  Validated before anything
 * is launched (MPF_ERR_BAD_ARGUMENT): NULL required pointers, non-positive sizes, offset + C > channels, a term count outside 1..3. */
#define MPF_GRU_MAX_TERMS 3
typedef struct MpfGruTerm {
    float *p;                    /* the tensor's first element, NOT the slice's; read only where the term is an input */
    int channels;                /* of that tensor */
    int offset;                  /* first channel of the slice */
} MpfGruTerm;
typedef struct MpfGruArgs {
    MpfGruTerm z[MPF_GRU_MAX_TERMS];     /* update calls */
    MpfGruTerm r[MPF_GRU_MAX_TERMS];     /* reset calls */
    MpfGruTerm q[MPF_GRU_MAX_TERMS];     /* update calls */
    MpfGruTerm dz[2], dr[2], dq[2];      /* backward calls: written */
    const float *h;              /* [B,C,H,W] */
    const float *g;              /* backward calls: the cotangent [B,C,H,W] */
    float *out;                  /* forward calls: written */
    float *dh;                   /* backward calls: [B,C,H,W] */
    int nz, nr, nq;              /* terms counted in z, r, q: 1..MPF_GRU_MAX_TERMS where the call uses them */
    int accumulate;              /* mpf_gru_reset_backward: add into dh */
    int B, C, H, W;
} MpfGruArgs;
int mpf_gru_reset(const MpfGruArgs *a, void *stream);
int mpf_gru_update(const MpfGruArgs *a, void *stream);
int mpf_gru_update_backward(const MpfGruArgs *a, void *stream);
int mpf_gru_reset_backward(const MpfGruArgs *a, void *stream);

/* The memory-bound chain between the convolutions of RAFT's encoders (ResidualBlock / BottleneckBlock / BasicEncoder / SmallEncoder,
 * RAFT/core/extractor.py): normalise, ReLU, add the shortcut, ReLU - forward and gradient, fused.  All tensors f32, NCHW, contiguous; the per-chunk partial sums are fp64
 * (a few numbers per plane), so that splitting a plane into chunks does not add an fp32 rounding per chunk to the statistics.
 * A TERM is an activation x [N,C,H,W] with a norm mode; a statistic SET is what one mean / variance is taken over:
 *   MPF_NORM_NONE         identity
 *   MPF_NORM_INSTANCE     sets (n, c) over H*W, biased variance                         N*C sets
 *   MPF_NORM_BATCH_TRAIN  sets c over N*H*W                                             C sets
 *   MPF_NORM_BATCH_EVAL   running_mean / running_var [C], no reduction at all
 *   MPF_NORM_GROUP        sets (n, g) over the C/groups channels of group g             N*groups sets
 * normalised value = (x - mean) * rstd * weight[c] + bias[c], rstd = 1 / sqrt(var + 1e-5); weight and bias are optional (NULL: 1 and 0).
 *   mpf_norm_stats    per present term with a statistics mode: partials[N,C,chunks,2] <- (mean, centred sum of squares M2) of chunk k of
 *                     plane (n, c): the elements [k*L, min((k+1)*L, H*W)), L = ceil(H*W / chunks) rounded up to a multiple of 4 (a chunk may
 *                     be empty: (0, 0)).  Sums of (x - x[first]) and its square in fp64: no E[x^2] - E[x]^2 cancellation.
 *   mpf_norm_act      out = relu(norm(y.x)); with a residual - `res`, a plain tensor, or the term `r`, normalised WITHOUT a ReLU - out =
 *                     relu(residual + relu(norm(y.x))).  Every workgroup merges the partials of its set with Chan's formula in a fixed order
 *                     (fp64); mean[set], rstd[set] and, where non-NULL, var[set] (biased) are written once.
 *   mpf_norm_act_backward_reduce   g = grad out; recomputes both ReLU masks from the same inputs and mean / rstd;
 *                     grad_partials[N,C,chunks,2] <- (sum dy, sum dy * xhat) per chunk for every normalised term that has the buffer.
 *   mpf_norm_act_backward          merges those in a fixed order; dx <- rstd * (dy * weight - mean(dy weight) - xhat * mean(dy weight xhat)) per
 *                     set (BATCH_EVAL: dy * weight * rstd, NONE: dy; neither reads grad_partials for dx); dweight[c] <- sum dy * xhat, dbias[c]
 *                     <- sum dy where non-NULL (these need grad_partials in every normalised mode); dres <- the shortcut's gradient, or dres +=
 *                     with accumulate != 0.
 * relu(v) = v < 0 ? 0 : v and its gradient passes where !(v <= 0): NaN stays where torch keeps it.  16-byte accesses when H*W % 4 == 0 and
 * every tensor pointer is 16-byte aligned, 4-byte ones otherwise; the chunk layout does not depend on that.  No atomics: bit-identical from
 * call to call for equal arguments (chunks included).  Outputs must not overlap inputs (dres with accumulate excepted).  Validated before
 * anything is launched (MPF_ERR_BAD_ARGUMENT): NULL required pointers, a mode outside 0..4, groups < 1 or C % groups != 0, chunks outside
 * 1..MPF_NORM_MAX_CHUNKS, non-positive sizes, N*C*max(H*W, chunks) >= 2^31, both `res` and `r`. */
#define MPF_NORM_NONE 0
#define MPF_NORM_INSTANCE 1
#define MPF_NORM_BATCH_TRAIN 2
#define MPF_NORM_BATCH_EVAL 3
#define MPF_NORM_GROUP 4
#define MPF_NORM_MAX_CHUNKS 1024
typedef struct MpfNormTerm {
    const float *x;              /* [N,C,H,W]; NULL: the term is absent (r only) */
    const float *weight;         /* [C] or NULL */
    const float *bias;           /* [C] or NULL */
    const float *running_mean;   /* [C], BATCH_EVAL */
    const float *running_var;    /* [C], BATCH_EVAL */
    double *partials;            /* [N,C,chunks,2] fp64: written by mpf_norm_stats, read by mpf_norm_act */
    float *mean;                 /* [sets]: written by mpf_norm_act, read by the backward calls */
    float *rstd;                 /* [sets]: likewise */
    float *var;                  /* [sets] or NULL: written by mpf_norm_act (biased variance, for running statistics) */
    double *grad_partials;       /* [N,C,chunks,2] fp64: written by mpf_norm_act_backward_reduce, read by mpf_norm_act_backward */
    float *dx;                   /* [N,C,H,W]: written by mpf_norm_act_backward */
    float *dweight;              /* [C] or NULL */
    float *dbias;                /* [C] or NULL */
    int mode;                    /* MPF_NORM_* */
    int groups;                  /* GROUP: divides C; otherwise ignored */
} MpfNormTerm;
typedef struct MpfNormArgs {
    MpfNormTerm y;               /* the main term */
    MpfNormTerm r;               /* the residual as a normalised term (r.x != NULL), e.g. norm3(conv1x1(x)) of a strided block */
    const float *res;            /* or the residual as a plain tensor [N,C,H,W] (identity shortcut); NULL with r.x NULL: no residual */
    float *out;                  /* mpf_norm_act: written */
    const float *g;              /* backward calls: the cotangent of out */
    float *dres;                 /* mpf_norm_act_backward with `res`: written, or added to with accumulate */
    int accumulate;
    int chunks;                  /* 1..MPF_NORM_MAX_CHUNKS; the same number in all four calls of one forward / backward */
    int N, C, H, W;
} MpfNormArgs;
int mpf_norm_stats(const MpfNormArgs *a, void *stream);
int mpf_norm_act(const MpfNormArgs *a, void *stream);
int mpf_norm_act_backward_reduce(const MpfNormArgs *a, void *stream);
int mpf_norm_act_backward(const MpfNormArgs *a, void *stream);

/* What RAFT.forward (RAFT/core/raft.py:86-144) does between its modules.  All tensors f32, NCHW, contiguous; every tensor below 2^31 elements.
 *   mpf_raft_images             pair[2N,3,H,W] <- 2 * (x / 255) - 1 of image1 [N,3,H,W] (first N) and image2 (last N), one launch: the feature
 *                               network's batch, whose first half is the context network's input.  A true, correctly rounded fp32 division.
 *   mpf_context_split           cnet [N,hdim+cdim,H,W]: net [N,hdim,H,W] <- tanh(cnet[:, :hdim]), inp [N,cdim,H,W] <- relu(cnet[:, hdim:]), one launch
 *   mpf_context_split_backward  grad_cnet [N,hdim+cdim,H,W] <- (g_net * (1 - net^2) | g_inp where !(inp <= 0), else 0) from the saved outputs
 *   mpf_upflow8                 flow [N,2,H,W]: flow_up [N,2,8H,8W] <- 8 * bilinear(flow), align_corners = true (utils/utils.py:80-82): the source
 *                               coordinate is dst * (H-1)/(8H-1), scale 0 for a size of 1; ATen's upsample_bilinear2d operation for operation
 *   mpf_upflow8_backward        g_up [N,2,8H,8W]: grad_flow [N,2,H,W] <- per coarse element the weighted sum (fp64, fixed order) over the fine
 *                               pixels whose footprint touches it
 * relu(v) = v < 0 ? 0 : v.  16-byte accesses where the sizes and pointers allow, 4-byte ones otherwise: any N, H, W >= 1.  No atomics:
 * bit-identical from run to run.  Outputs must not overlap inputs.  Validated before anything is launched (MPF_ERR_BAD_ARGUMENT): NULL
 * pointers the call uses, non-positive sizes, a tensor of 2^31 elements or more. */
typedef struct MpfRaftGlueArgs {
    const float *image1, *image2;    /* mpf_raft_images: [N,3,H,W] each */
    float *pair;                     /* mpf_raft_images: [2N,3,H,W], written */
    const float *cnet;               /* mpf_context_split: [N,hdim+cdim,H,W] */
    float *net, *inp;                /* mpf_context_split: written; _backward: read */
    const float *g_net, *g_inp;      /* mpf_context_split_backward: the cotangents of net and inp */
    float *grad_cnet;                /* mpf_context_split_backward: [N,hdim+cdim,H,W], written */
    const float *flow;               /* mpf_upflow8: [N,2,H,W] */
    float *flow_up;                  /* mpf_upflow8: [N,2,8H,8W], written */
    const float *g_up;               /* mpf_upflow8_backward: the cotangent [N,2,8H,8W] */
    float *grad_flow;                /* mpf_upflow8_backward: [N,2,H,W], written */
    int N, H, W;                     /* mpf_raft_images: the frame; the other calls: the coarse (1/8) map */
    int hdim, cdim;                  /* the context split */
} MpfRaftGlueArgs;
int mpf_raft_images(const MpfRaftGlueArgs *a, void *stream);
int mpf_context_split(const MpfRaftGlueArgs *a, void *stream);
int mpf_context_split_backward(const MpfRaftGlueArgs *a, void *stream);
int mpf_upflow8(const MpfRaftGlueArgs *a, void *stream);
int mpf_upflow8_backward(const MpfRaftGlueArgs *a, void *stream);

/* What RAFT/evaluate.py does around the model on frames whose sides are no multiples of 8.  All tensors f32, contiguous.  The pad is
 * InputPadder's (RAFT/core/utils/utils.py:7-24): pad_left, pad_right, pad_top, pad_bottom, each 0..7.
 *   mpf_raft_images_padded   image1, image2 [N,3,H,W]; Hp = H + pad_top + pad_bottom and Wp = W + pad_left + pad_right multiples of 8:
 *                            pair [2N,3,Hp,Wp] <- 2 * (x / 255) - 1 of the replicate-padded images (source indices clamped), image1 first: what
 *                            mpf_raft_images makes of F.pad(image, pad, mode='replicate'), bit for bit, the padded images never written.  With a
 *                            pad of zeros it is mpf_raft_images.
 *   mpf_upsample_flow_crop   flow [N,2,H,W], mask [N,576,H,W] (H, W: the coarse map): flow_up [N,2,8H-pad_top-pad_bottom,8W-pad_left-pad_right]
 *                            <- rows pad_top .., columns pad_left .. of mpf_upsample_flow's [N,2,8H,8W], bit for bit; that tensor is never
 *                            written, and mask channels of sub-positions outside the window are not read.
 *   mpf_upflow8_crop         flow [N,2,H,W]: the same window of mpf_upflow8's result, bit for bit (mask ignored).
 *   mpf_flow_metrics         flow_pr, flow_gt [N,2,H,W], valid [N,H,W] or NULL (every pixel counts): metrics [N,6] f64 <- per frame, over the
 *                            pixels with valid >= 0.5: the sum of epe, their number, the numbers with epe < 1, < 3, < 5, and the number of
 *                            outliers, epe > 3 and epe / mag > 0.05 (validate_kitti; mag = 0 gives inf, an outlier).  epe = sqrt(du^2 + dv^2) and
 *                            mag = sqrt(gt_u^2 + gt_v^2) in fp32.  No max_flow rule.  Sums in f64, per-block partials folded in a fixed order, no
 *                            atomics: bit-identical from run to run.  workspace: mpf_flow_metrics_workspace(N, H, W) bytes, 8-byte aligned,
 *                            contents irrelevant before and after; N <= 65535.
 * Any sizes >= 1 with every tensor below 2^31 elements; pair must be 16-byte aligned (it is stored 16 bytes at a time), no other f32 tensor
 * needs any alignment.  Outputs must not overlap inputs.  Tensor VALUES are unrestricted and no value changes an address.  Validated before
 * anything is launched (MPF_ERR_BAD_ARGUMENT): a NULL block, non-positive sizes, a pad outside 0..7, a padded frame that is no multiple of 8,
 * a pad that leaves no window, a tensor of 2^31 elements or more, NULL pointers the call uses. */
typedef struct MpfRaftEvalArgs {
    const float *image1, *image2;    /* mpf_raft_images_padded: [N,3,H,W] each */
    float *pair;                     /* mpf_raft_images_padded: [2N,3,Hp,Wp], written */
    const float *flow;               /* crop calls: [N,2,H,W] */
    const float *mask;               /* mpf_upsample_flow_crop: [N,576,H,W] */
    float *flow_up;                  /* crop calls: the window, written */
    const float *flow_pr, *flow_gt;  /* mpf_flow_metrics: [N,2,H,W] each */
    const float *valid;              /* mpf_flow_metrics: [N,H,W] or NULL */
    double *metrics;                 /* mpf_flow_metrics: [N,6], written */
    void *workspace;                 /* mpf_flow_metrics */
    size_t workspace_bytes;
    int N, H, W;                     /* mpf_raft_images_padded: the unpadded frame; crop calls: the coarse (1/8) map; mpf_flow_metrics: the frame */
    int pad_left, pad_right, pad_top, pad_bottom;
} MpfRaftEvalArgs;
int mpf_raft_images_padded(const MpfRaftEvalArgs *a, void *stream);
int mpf_upsample_flow_crop(const MpfRaftEvalArgs *a, void *stream);
int mpf_upflow8_crop(const MpfRaftEvalArgs *a, void *stream);
size_t mpf_flow_metrics_workspace(int N, int H, int W);   /* 0 for a shape the call refuses */
int mpf_flow_metrics(const MpfRaftEvalArgs *a, void *stream);

/* RAFT's warm start: forward_interpolate (RAFT/core/utils/utils.py:26-54; evaluate.py: create_sintel_submission) without the host round trip.
 * flow, out [N,2,h,w] f32, contiguous; samples are independent.  Per sample, with dx = flow[0], dy = flow[1]:
 *   sources    every pixel (x0, y0) at x1 = (double)x0 + (double)dx, y1 = (double)y0 + (double)dy (numpy's int64 + float32), VALID iff
 *              x1 > 0 && x1 < w && y1 > 0 && y1 < h: all four strict, as upstream's, so a pixel of column 0 with dx == 0 is no source; NaN
 *              and +-inf fail the comparisons and drop out.
 *   selection  every pixel (gx, gy) takes (dx, dy) of the valid source with the least d2 = (x1 - gx) * (x1 - gx) + (y1 - gy) * (y1 - gy),
 *              in f64, each product rounded and then the sum (no fused multiply-add).  The two f32 values are copied, so the result is
 *              bit-exact whenever the selection is: what scipy's griddata(method='nearest') returns wherever the nearest source is unique.
 *   ties       equal d2 goes to the source with the lowest flat index y0 * w + x0 (scipy defines no order there; this rule is ours).
 *   no source  a sample without a valid source gives zeros, a cold start (upstream: NaN; the one intended difference).
 * Brute force, every target against every source: the work is (h * w)^2 per sample, so h * w <= MPF_WARM_MAX_HW (a 1080p frame's coarse
 * grid, 135 x 240, is half of that), N <= 65535 and N * h * w <= MPF_WARM_MAX_NHW.  A minimum over (d2, index): no atomics, bit-identical
 * from run to run.  workspace: mpf_forward_interpolate_workspace(N, h, w) bytes (12 bytes per target and source chunk, at most 32 chunks, rounded up to 8),
 * 8-byte aligned, contents irrelevant before and after.  No f32 tensor needs any alignment.  out must not overlap flow.  Tensor VALUES are
 * unrestricted; the only value-dependent address is the selected source's, an index below h * w by construction.  Validated before anything
 * is launched (MPF_ERR_BAD_ARGUMENT): a NULL block, non-positive sizes, a shape above the limits, NULL pointers, out overlapping flow, a
 * workspace that is NULL, misaligned or too small. */
#define MPF_WARM_MAX_HW 65536            /* h * w of one sample */
#define MPF_WARM_MAX_NHW 4194304         /* 2^22: N * h * w of one call (the workspace then stays below 1.5 GiB) */
typedef struct MpfWarmStartArgs {
    const float *flow;               /* [N,2,h,w] */
    float *out;                      /* [N,2,h,w], written */
    void *workspace;
    size_t workspace_bytes;
    int N, h, w;
} MpfWarmStartArgs;
size_t mpf_forward_interpolate_workspace(int N, int h, int w);   /* 0 for a shape the call refuses */
int mpf_forward_interpolate(const MpfWarmStartArgs *a, void *stream);

/* What upstream RAFT does with a prediction: demo.py's colour coding and the code of KITTI's 16-bit flow PNG.  flow [N,2,H,W] f32, contiguous.
 *   mpf_flow_to_image        RAFT/core/utils/flow_viz.py's flow_to_image (make_colorwheel, flow_uv_to_colors) per image of the batch:
 *                            out [N,H,W,3] u8.  Two launches, no host step between them: the per-image maximum rad_max of sqrt(u^2 + v^2)
 *                            into the workspace (one slot per block, no atomics: a maximum has no order, bit-identical from run to run),
 *                            then the colours.  Upstream's arithmetic at upstream's precisions: with clip != 0 first u, v <- min(max(., 0),
 *                            clip_flow) (np.clip(flow, 0, clip_flow): upstream's lower bound IS 0); u, v <- u, v / (rad_max + 1e-5f);
 *                            rad = sqrt(u^2 + v^2), a = atan2(-v, -u) / pi, fk = (a + 1) / 2 * 54, all f32; k0 = floor(fk), k1 = k0 + 1
 *                            (55 wraps to 0), f = fk - k0, col = (1 - f) * wheel[k0] / 255 + f * wheel[k1] / 255, then rad <= 1 ?
 *                            1 - rad * (1 - col) : 0.75 * col, and the byte floor(255 * col), all f64.  The 55-entry wheel is built on the
 *                            host per call as make_colorwheel builds it.  Channels R, G, B; B, G, R with convert_to_bgr != 0.  An all-zero
 *                            image is white (atan2(-0, -0) = -pi).  Against numpy the f32 atan2 may differ in its last bits, so a byte whose
 *                            exact value lies within 0.01 of an integer may differ by 1 (tests/test_raft_flow_outputs.py).
 *                            image [N,3,H,W] f32 in 0..255, R, G, B planes (what RAFT takes), or NULL.  With an image, out is [N,2H,W,3]: the
 *                            frame on top, truncated toward zero as astype(uint8) and clamped to 0..255, the colours below: demo.py:viz's
 *                            np.concatenate([img, flo], axis=0).  convert_to_bgr reverses the channels of both halves.
 *                            NON-FINITE flow: k0 is clamped to 0..54 before it indexes the wheel, rad_max drops NaN; the colours of an image
 *                            that holds a non-finite vector are unspecified (upstream's are, too), no address depends on them.
 *                            workspace: mpf_flow_to_image_workspace(N, H, W) bytes, 4-byte aligned, contents irrelevant before and after.
 *   mpf_flow_encode_kitti    frame_utils.writeFlowKITTI's array: out [N,H,W,3] u16 = (64 * u + 2^15, 64 * v + 2^15, valid), in the order the
 *                            file holds them as R, G, B (upstream hands cv2 the reversed array as B, G, R; readFlowKITTI reverses what
 *                            cv2 reads back).  The product and the sum are rounded in f32, as numpy's, and the code is truncated toward zero,
 *                            as astype(uint16).  valid [N,H,W] f32 or NULL: 1 where valid >= 0.5, else 0; NULL: all ones, as upstream writes.
 *                            THE ONE DEVIATION: a code outside 0..65535 (|flow| >= 512 px), undefined in numpy, is clamped to 0 / 65535;
 *                            NaN gives 0.
 * Both outputs are stored 12 bytes per lane as dwords: out must be 4-byte aligned; flow, image and valid need no alignment.  N, H, W >= 1,
 * N <= 65535, N * H * W < 2^31 / 6.  Outputs must not overlap inputs.  Validated before anything is launched (MPF_ERR_BAD_ARGUMENT): a NULL
 * block, non-positive or too large sizes, NULL flow or out, a misaligned out, a NaN clip_flow, a workspace that is NULL, misaligned or too small. */
typedef struct MpfFlowVizArgs {
    const float *flow;               /* [N,2,H,W] */
    const float *image;              /* mpf_flow_to_image: [N,3,H,W] or NULL */
    const float *valid;              /* mpf_flow_encode_kitti: [N,H,W] or NULL */
    void *out;                       /* mpf_flow_to_image: u8 [N,H,W,3], [N,2H,W,3] with an image; mpf_flow_encode_kitti: u16 [N,H,W,3]; written */
    void *workspace;                 /* mpf_flow_to_image */
    size_t workspace_bytes;
    int N, H, W;
    int clip;                        /* mpf_flow_to_image: != 0: clip the flow to [0, clip_flow] first */
    float clip_flow;
    int convert_to_bgr;              /* mpf_flow_to_image */
} MpfFlowVizArgs;
size_t mpf_flow_to_image_workspace(int N, int H, int W);   /* 0 for a shape the call refuses */
int mpf_flow_to_image(const MpfFlowVizArgs *a, void *stream);
int mpf_flow_encode_kitti(const MpfFlowVizArgs *a, void *stream);

/* The warp-back RGB-D mesh renderer (warpback/utils.py: RGBDRenderer) without pytorch3d.  All tensors f32 and contiguous unless stated.
 *   mpf_rgbd_mesh_vertices   construct_mesh and the first half of render_mesh (warpback/utils.py:31-51, 84-111, 174-218) per pixel (y, x),
 *                            vertex y * w + x, with nothing intermediate stored:
 *                              (u, v) = ((x + 0.5) / w, (y + 0.5) / h); depth = 1 / (disp + 1e-4); P = (cam_int^-1 (u, v, 1)) * depth, each row
 *                              (k0 u + k1 v) + k2, the inverse by the adjugate in f64 and rounded to f32 once; Wd = cam_ext (P, 1), each row
 *                              ((e0 X + e1 Y) + e2 Z) + e3; n = (2 fx Wd.x + (2 cx - 1) Wd.z, 2 fy Wd.y + (2 cy - 1) Wd.z, a Wd.z + b),
 *                              a = (near + far) / (far - near), b = -2 near far / (far - near) in f32 with near = 1e-4, far = 1e4;
 *                              verts_ndc = (-(n.x / Wd.z) * float(w / h), -(n.y / Wd.z), n.z / Wd.z).
 *                              attrs = (r, g, b, vis, Wd.z); vis = exp(-10 sqrt(gx^2 + gy^2)) > 0.3 ? 1 : 0 with gx, gy the 3 x 3 Sobel
 *                              responses of the disparity under zero padding (get_visible_mask).
 *                            The reference's f32 matmul and inverse associate differently: tests/test_warpback.py bounds the difference.
 *   mpf_rasterize_grid       pytorch3d's rasterize_meshes (faces_per_pixel = 1, perspective_correct = False, clip_barycentric_coords =
 *                            False, cull_backfaces = False, no z clipping) followed by interpolate_face_attributes, on the regular grid
 *                            mesh of h x w vertices whose faces are implicit: Q = (h - 1)(w - 1), F = 2 Q; cell q = r (w - 1) + c has
 *                            tl = r w + c, tr = tl + 1, bl = tl + w, br = bl + 1; face q = (tl, bl, br), face Q + q = (br, tr, tl).
 *                            INTEGRATION.md section 16 is the definition, operation by operation (tests/warpback_restated.py restates it).
 *                            Outputs, with the value of a pixel no face covers: pix_to_face i64 [B,h,w] = b F + f (-1); zbuf [B,h,w] (-1);
 *                            bary [B,h,w,3], unclipped (-1); out [B,C,h,w] (+0).  The winner of a pixel is the covering face of the least
 *                            depth, the lowest face index on equal depth; a face with a non-finite coordinate is skipped.  A 64-bit atomic
 *                            minimum per covered pixel: identical bytes on every run.
 *                            workspace: mpf_rasterize_grid_workspace(B, h, w) bytes (8 per pixel), 8-byte aligned, contents irrelevant
 *                            before and after.  pix_to_face must be 8-byte aligned; no f32 tensor needs any alignment.
 * Limits: h, w >= 2; B <= 65535; B * h * w <= MPF_MESH_MAX_BHW (so 2 (h - 1)(w - 1) < 2^31); 1 <= C <= MPF_MESH_MAX_ATTRS.  Tensor VALUES
 * are unrestricted: no address depends on one.  No gradients.  Validated before anything is launched (MPF_ERR_BAD_ARGUMENT): a NULL block,
 * a shape outside the limits, NULL pointers, outputs that overlap inputs, a workspace that is NULL, misaligned or too small. */
#define MPF_MESH_MAX_ATTRS 8
#define MPF_MESH_PASS_ALL 0              /* clear, z pass, resolve pass */
#define MPF_MESH_PASS_Z 1                /* clear and z pass only: the keys stay in the workspace, no output is written (the four output pointers may be NULL) */
#define MPF_MESH_PASS_RESOLVE 2          /* resolve pass only, from the keys an MPF_MESH_PASS_Z call with the same arguments left in the workspace */
#define MPF_MESH_MAX_BHW 268435456       /* 2^28: B * h * w of one call (the workspace is then 2 GiB) */
typedef struct MpfMeshVertexArgs {
    const float *rgbd;               /* [B,4,h,w]: r, g, b, disparity */
    const float *cam_int;            /* [B,3,3] */
    const float *cam_ext;            /* [B,3,4] */
    float *verts_ndc;                /* [B,h*w,3], written */
    float *attrs;                    /* [B,h*w,5], written */
    int B, h, w;
} MpfMeshVertexArgs;
typedef struct MpfMeshRasterArgs {
    const float *verts_ndc;          /* [B,h*w,3] */
    const float *attrs;              /* [B,h*w,C] */
    int64_t *pix_to_face;            /* [B,h,w], written */
    float *zbuf;                     /* [B,h,w], written */
    float *bary;                     /* [B,h,w,3], written */
    float *out;                      /* [B,C,h,w], written */
    void *workspace;
    size_t workspace_bytes;
    int B, h, w, C;
    float blur_radius;               /* a SQUARED distance in NDC units, as pytorch3d's */
    int passes;                      /* MPF_MESH_PASS_ALL, or one half of the call on its own (tools/bench_warpback.py times them) */
} MpfMeshRasterArgs;
int mpf_rgbd_mesh_vertices(const MpfMeshVertexArgs *a, void *stream);
size_t mpf_rasterize_grid_workspace(int B, int h, int w);   /* 0 for a shape the call refuses */
int mpf_rasterize_grid(const MpfMeshRasterArgs *a, void *stream);

/* Warp-back stage 2 (warpback/stage2_dataset.py): the masked Canny of get_edge on the device, and the pointwise chain of inpaint around the
 * three EdgeConnect generators.  All tensors f32 and contiguous unless stated; every operation f32, rounded once, never contracted.
 *   mpf_canny        skimage.feature.canny(gray, sigma, low_threshold, high_threshold, mask) per image of a batch, in three stages whose
 *                    definition INTEGRATION.md section 17 states operation by operation (tests/canny_restated.py restates it):
 *                      1  smoothed = G(mask ? gray : 0) / (G(mask ? 1 : 0) + FLT_EPSILON), G the separable Gaussian of `weights` (2 radius + 1
 *                         taps, along the row index first, then along the column index, zero outside the image, taps added from -radius up)
 *                      2  Sobel of smoothed under a reflected border, magnitude, and the class of every pixel: 0, or for a pixel of the
 *                         3 x 3-eroded mask off the border ring whose magnitude is >= low_threshold and >= the two magnitudes interpolated
 *                         along its gradient, 1 (weak) or 2 (strong: magnitude >= high_threshold)
 *                      3  out = 1.0 where a weak or strong pixel is 8-connected through weak or strong pixels to a strong one, else 0.0
 *                    The workspace keeps smoothed [B,h,w] f32 at offset 0 and the classes [B,h,w] u8 at offset 4 B h w; `passes` runs one
 *                    stage alone on what the stage before left there.  Stage 3 is one workgroup per image sweeping a bit map (in LDS up to
 *                    MPF_CANNY_LDS_WORDS words per plane, else in the workspace) to the fixpoint: at most h w sweeps, no workgroup waits
 *                    for another, identical bytes on every run.  Class bytes other than 1 and 2 count as 0.
 * Limits: B <= 65535; h, w >= 1; B * h * w <= MPF_CANNY_MAX_BHW; 0 <= radius <= MPF_CANNY_MAX_RADIUS; low_threshold <= high_threshold, no NaN.
 * Validated before anything is launched (MPF_ERR_BAD_ARGUMENT); tensor VALUES are unrestricted: no address depends on one. */
#define MPF_CANNY_MAX_RADIUS 16
#define MPF_CANNY_MAX_BHW 268435456      /* 2^28 */
#define MPF_CANNY_LDS_WORDS 6144         /* h * ceil(w / 32) up to which stage 3 keeps its two bit planes in LDS (48 KiB) */
#define MPF_CANNY_PASS_ALL 0
#define MPF_CANNY_PASS_SMOOTH 1          /* stage 1 only: gray, mask -> workspace (smoothed); out may be NULL */
#define MPF_CANNY_PASS_CLASSIFY 2        /* stage 2 only: workspace (smoothed), mask -> workspace (classes); gray and out may be NULL */
#define MPF_CANNY_PASS_HYSTERESIS 3      /* stage 3 only: workspace (classes) -> out; gray and mask may be NULL */
typedef struct MpfCannyArgs {
    const float *gray;               /* [B,1,h,w] */
    const float *mask;               /* [B,1,h,w]: nonzero is inside */
    float *out;                      /* [B,1,h,w], written: 0.0 or 1.0 */
    void *workspace;                 /* mpf_canny_workspace(B, h, w) bytes, 4-byte aligned */
    size_t workspace_bytes;
    int B, h, w;
    int radius;                      /* int(4 sigma + 0.5) */
    float weights[2 * MPF_CANNY_MAX_RADIUS + 1];   /* weights[radius + k] = exp(-0.5 k^2 / sigma^2) / sum, formed in f64 on the host, rounded once */
    float low_threshold, high_threshold;
    int passes;                      /* MPF_CANNY_PASS_* */
} MpfCannyArgs;
size_t mpf_canny_workspace(int B, int h, int w);   /* 0 for a shape the call refuses */
int mpf_canny(const MpfCannyArgs *a, void *stream);

/*   mpf_stage2_*     inpaint's torch glue, one launch each, every result equal to the torch expression bit for bit:
 *                      _gray_hole    gray = (0.2989 r + 0.587 g) + 0.114 b of image; mask_hole = 1 - mask
 *                      _edge_input   edge_input [B,3,h,w] = (gray, edge, mask_hole)
 *                      _gen_inputs   image_input [B,4,h,w] = (image + mask_hole per channel, edge_inpaint); disp_input [B,2,h,w] = (disp +
 *                                    mask_hole, edge_inpaint)
 *                      _merge        image_merged = image * (1 - mask_hole) + image_inpaint * mask_hole per channel; disp_merged likewise
 *                    Each call reads and writes only the fields named for it; an output must not overlap an input.  B * h * w <= 2^28. */
typedef struct MpfStage2Args {
    const float *image;              /* [B,3,h,w] */
    const float *disp;               /* [B,1,h,w] */
    const float *mask;               /* [B,1,h,w] */
    const float *edge;               /* [B,1,h,w] */
    const float *edge_inpaint;       /* [B,1,h,w] */
    const float *image_inpaint;      /* [B,3,h,w] */
    const float *disp_inpaint;       /* [B,1,h,w] */
    float *gray;                     /* [B,1,h,w]: written by _gray_hole, read by _edge_input */
    float *mask_hole;                /* [B,1,h,w]: written by _gray_hole, read by the other three */
    float *edge_input;               /* [B,3,h,w] */
    float *image_input;              /* [B,4,h,w] */
    float *disp_input;               /* [B,2,h,w] */
    float *image_merged;             /* [B,3,h,w] */
    float *disp_merged;              /* [B,1,h,w] */
    int B, h, w;
} MpfStage2Args;
int mpf_stage2_gray_hole(const MpfStage2Args *a, void *stream);
int mpf_stage2_edge_input(const MpfStage2Args *a, void *stream);
int mpf_stage2_gen_inputs(const MpfStage2Args *a, void *stream);
int mpf_stage2_merge(const MpfStage2Args *a, void *stream);

/* The sparse bilateral filter of 3d-photo-inpainting (the reference's bilateral_filter.py: sparse_bilateral_filtering): a 0/1-weighted median
 * around disparity discontinuities, num_iter times, per image of a batch.  INTEGRATION.md section 18 states it operation by operation
 * (tests/bilateral_restated.py restates it).  With v = depth, per iteration i, ws = filter_size[i], m = ws / 2:
 *   1  D = 1 at interior pixels where |1 / v[p] - 1 / v[q]| > depth_threshold for one of the four neighbours q (with a mask: only where
 *      mask[p] and mask[q] are both nonzero), 1 where the call's INPUT is 0, then 0 where the mask is 0.  The divide is correctly rounded;
 *      inf and NaN take their IEEE course (NaN > t is false).
 *   2  v' and D' are v and D with the outermost ring replaced by its inner neighbour, then edge-padded by m; the mask is zero-padded.
 *   3  a pixel whose mask is 0, or whose ws x ws window holds no D', gets v'.  Another gets the k*(n)-th smallest of the n valid values
 *      of its window (D' = 0 and mask nonzero), or v' when n = 0.  k*(n) = mpf_sparse_bilateral_rank(n): 1 + #{k <= n : S_k <= 0.5} with
 *      S_k the f32 sum of k copies of fl32(1 / n) added one at a time, which is NOT n / 2 + 1 for every n.
 * dtype: MPF_BILATERAL_F32 (arithmetic in f32, the threshold rounded to f32), _F64, or _U8, whose value is u / 255.0 in f64 and whose output
 * is the selected pixel's byte.  The result is a selection of input values: identical bytes on every run, no atomics.  One call runs every
 * iteration (two launches each), between two buffers of the workspace; the last iteration writes out.
 * Limits: B <= 65535; h, w >= 3; B * h * w <= MPF_BILATERAL_MAX_BHW; 1 <= num_iter <= MPF_BILATERAL_MAX_ITER; filter_size[i] in 3, 5, 7, 9;
 * depth_threshold not NaN.  Validated before anything is launched (MPF_ERR_BAD_ARGUMENT).  Values are meant to be finite; NaN is not looked for. */
#define MPF_BILATERAL_F32 0
#define MPF_BILATERAL_F64 1
#define MPF_BILATERAL_U8 2
#define MPF_BILATERAL_MAX_WINDOW 9
#define MPF_BILATERAL_MAX_ITER 8
#define MPF_BILATERAL_MAX_BHW 268435456  /* 2^28 */
typedef struct MpfBilateralArgs {
    const void *depth;               /* [B,h,w] of dtype */
    const unsigned char *mask;       /* [B,h,w] u8, or [h,w] with mask_shared, nonzero is inside; NULL: no mask */
    void *out;                       /* [B,h,w] of dtype, written; must not overlap depth */
    void *workspace;                 /* mpf_sparse_bilateral_workspace(dtype, B, h, w) bytes, 16-byte aligned */
    size_t workspace_bytes;
    int dtype;                       /* MPF_BILATERAL_F32 / _F64 / _U8 */
    int B, h, w;
    int mask_shared;                 /* 1: one [h,w] mask for every image */
    int num_iter;
    int filter_size[MPF_BILATERAL_MAX_ITER];
    double depth_threshold;
} MpfBilateralArgs;
size_t mpf_sparse_bilateral_workspace(int dtype, int B, int h, int w);   /* 0 for a dtype or shape the call refuses */
int mpf_sparse_bilateral_rank(int n);                                    /* k*(n) for 1 <= n <= 81, else 0; host arithmetic, no GPU */
int mpf_sparse_bilateral(const MpfBilateralArgs *a, void *stream);

/* The training-time half of the reference's utils/mpi (MINE's plane samplers and its disparity-consistency loss); INTEGRATION.md section 21 states
 * each operation by operation (tests/mpi_training_restated.py restates them in float64).  All tensors f32 and contiguous unless said otherwise;
 * everything is validated before anything is launched (MPF_ERR_BAD_ARGUMENT), and nothing synchronises with the host.
 *
 * The pixel index of a coordinate v in a frame of n: rint(v) (ties to even), clamped to [0, n - 1] as a float before the cast - NaN and -inf
 * give 0, +inf gives n - 1; an i64 coordinate is clamped as it is.
 *
 * mpf_gather_pxpy       out[b,c,i] = img[b,c, index(pxpy[b,1,i], H) * W + index(pxpy[b,0,i], W)]   (rendering_utils.py:26-43)
 * mpf_gather_pxpy_bwd   grad_img[b,c,that pixel] += grad_out[b,c,i], float atomic adds into a buffer the caller zeroed: points that share a pixel
 *                       decide the last bits of its sum by their order.  pxpy receives no gradient (the reference indexes under no_grad).
 * Limits: B <= 65535; B * C * H * W and B * C * N below 2^31. */
#define MPF_PXPY_F32 0
#define MPF_PXPY_I64 1
typedef struct MpfGatherPxpyArgs {
    const float *img;                /* [B,C,H,W]; read by mpf_gather_pxpy */
    const void *pxpy;                /* [B,2,N] f32 or i64 (pxpy_dtype): row 0 is x, row 1 is y */
    float *out;                      /* [B,C,N], written by mpf_gather_pxpy */
    const float *grad_out;           /* [B,C,N]; read by mpf_gather_pxpy_bwd */
    float *grad_img;                 /* [B,C,H,W], added into by mpf_gather_pxpy_bwd */
    int pxpy_dtype;                  /* MPF_PXPY_F32 / _I64 */
    int B, C, H, W, N;
} MpfGatherPxpyArgs;
int mpf_gather_pxpy(const MpfGatherPxpyArgs *a, void *stream);
int mpf_gather_pxpy_bwd(const MpfGatherPxpyArgs *a, void *stream);

/* mpf_sample_pdf   rendering_utils.py:90-139 with the draws u handed in.  Per row (b, n) of S values v and S weights w, in f32, every operation
 *                  rounded on its own:  edges e[0] = v[0], e[k] = (v[k] + v[k-1]) * 0.5, e[S] = v[S-1];  cdf c[0] = 0, c[k+1] = c[k] + w[k] / (sum w + 1e-5),
 *                  the cdf added one element at a time in order with the running sum kept in f64 and every entry rounded to f32 (torch's CPU cumsum), sum w
 *                  the correctly rounded sum (added in f64, rounded once);  per draw u: i = the first index with c[i] > u (S + 1 if none), lo = max(i - 1, 0),
 *                  hi = min(i, S), t = (u - c[lo]) / max(c[hi] - c[lo], 1e-5), replaced by 0.5 where c[hi] - c[lo] <= 1e-4;  out = e[lo] + t * (e[hi] - e[lo]).
 * values may be contiguous (values_row_stride = S, values_batch_stride = N * S) or expanded over the rays (values_row_stride = 0: one row of S per
 * batch entry, values_batch_stride floats apart), which is read in place.
 * Limits: 1 <= S <= MPF_SAMPLE_PDF_MAX_S; 1 <= n_samples <= MPF_SAMPLE_PDF_MAX_SAMPLES; B * N * max(S, n_samples) below 2^31.  No atomics: identical
 * bytes on every run. */
#define MPF_SAMPLE_PDF_MAX_S 128
#define MPF_SAMPLE_PDF_MAX_SAMPLES 128
typedef struct MpfSamplePdfArgs {
    const float *values;             /* [B,1,N,S], or its expanded form (see above) */
    const float *weights;            /* [B,1,N,S] */
    const float *u;                  /* [B,1,N,n_samples] */
    float *out;                      /* [B,1,N,n_samples], written */
    long long values_batch_stride;   /* floats between two batch entries of values */
    long long values_row_stride;     /* S, or 0 */
    int B, N, S, n_samples;
} MpfSamplePdfArgs;
int mpf_sample_pdf(const MpfSamplePdfArgs *a, void *stream);

/* mpf_disp_consistency       mpi_rendering.py:180-210.  Per source pixel (x, y) of batch entry b, in f32:  r = K_src_inv (x, y, 1);  depth = 1 / disparity_src;
 *                            p = G_tgt_src (r * depth, 1);  q = K_tgt p[:3];  (px, py) = q.xy / q.z;  mask = 0 <= px <= W - 1 and 0 <= py <= H - 1 (false with
 *                            NaN);  diff = |1 / p.z - disparity_tgt[b, index(py, H), index(px, W)]|;  loss = sum over the mask of diff / count.  p.z's sign is
 *                            not looked at.  The sum: wave butterfly, one LDS slot per wave, per-block partials, then a double sum in block order - no atomics,
 *                            identical bits on every run; count is an exact integer.  count = 0 gives NaN.  The workspace keeps sum and count for the backward.
 * mpf_disp_consistency_bwd   with s = sign(1 / p.z - disparity_tgt[idx]) and g = grad_loss[0]:  grad_disparity_src = g s / count * (-1 / p.z^2) * (G[2,:3] . r) *
 *                            (-1 / disparity_src^2), one store per pixel (0 outside the mask; reproducible);  grad_disparity_tgt[idx] += -g s / count, float
 *                            atomic adds into a buffer the caller zeroed (source pixels that share a target pixel decide its last bits by their order).
 *                            Either gradient pointer may be NULL, not both.  The workspace is the forward's, untouched since.
 * Limits: B <= 65535; B * H * W below 2^31. */
typedef struct MpfDispConsistencyArgs {
    const float *K_src_inv;          /* [B,3,3] on the device */
    const float *G_tgt_src;          /* [B,4,4] on the device */
    const float *K_tgt;              /* [B,3,3] on the device */
    const float *disparity_src;      /* [B,1,H,W] */
    const float *disparity_tgt;      /* [B,1,H,W] */
    float *loss;                     /* [1], written by mpf_disp_consistency */
    const float *grad_loss;          /* [1] on the device; read by mpf_disp_consistency_bwd */
    float *grad_disparity_src;       /* [B,1,H,W], written by mpf_disp_consistency_bwd, or NULL */
    float *grad_disparity_tgt;       /* [B,1,H,W], added into by mpf_disp_consistency_bwd, or NULL */
    void *workspace;                 /* mpf_disp_consistency_workspace(B, H, W) bytes, 16-byte aligned: [0] f64 sum, [8] i64 count, then the partials */
    size_t workspace_bytes;
    int B, H, W;
} MpfDispConsistencyArgs;
size_t mpf_disp_consistency_workspace(int B, int H, int W);              /* 0 for a shape the call refuses */
int mpf_disp_consistency(const MpfDispConsistencyArgs *a, void *stream);
int mpf_disp_consistency_bwd(const MpfDispConsistencyArgs *a, void *stream);

/* The reference's backward warps by a flow field (utils/transform.py:60-111); INTEGRATION.md section 22 states both (tests/flow_warp_restated.py
 * restates them in float64).  All tensors f32 and contiguous; everything is validated before anything is launched (MPF_ERR_BAD_ARGUMENT); nothing
 * synchronises with the host.  Per pixel (x, y) of batch entry b with (u, v) = flow[b,:,y,x], in f32, every operation rounded on its own:
 *   MPF_FLOW_WARP_WARP   warp():  g = 2 * (x + u) / max(W - 1, 1) - 1;  ix = ((g + 1) * W - 1) / 2  (normalised for align_corners=True, sampled
 *                        at grid_sample's default False, as the reference does);  zero padding: a tap outside the image contributes 0;
 *                        mask = the sum of the weights of the taps inside;  d ix / d u = W / max(W - 1, 1).
 *   MPF_FLOW_WARP_RIFE   warp_rife():  g = lin_w[x] + u / ((W - 1) / 2) with lin_w = torch.linspace(-1, 1, W) handed in;  ix = (g + 1) / 2 * (W - 1),
 *                        clamped to [0, W - 1] (border padding; no gradient where ix <= 0 or ix >= W - 1, torch's clip_coordinates_set_grad);
 *                        d ix / d u = 1 inside the clamp.  No mask.  H, W >= 2.
 *   both, y likewise.    ix_nw = floor(ix);  nw = (ix_se - ix) * (iy_se - iy), ne = (ix - ix_sw) * (iy_sw - iy), sw = (ix_ne - ix) * (iy - iy_ne),
 *                        se = (ix - ix_nw) * (iy - iy_nw);  out[b,c,y,x] = x[nw tap] * nw + ... summed nw, ne, sw, se.  A non-finite coordinate
 *                        samples outside the image (WARP) or at index 0 (RIFE).
 * mpf_flow_warp       writes out and, where mask is not NULL (WARP only), mask [B,1,H,W].
 * mpf_flow_warp_bwd   grad_x[tap] += weight * grad_out, float atomic adds into a buffer the caller zeroed (the order of the adds decides its last
 *                     bits);  grad_flow[b,0] = d ix / d u * sum over c of grad_out * d out / d ix (and [b,1] likewise): one store per pixel, the sum
 *                     taken per chunk of MPF_FLOW_WARP_CHUNK channels in channel order, the chunks in chunk order - no atomics, identical bytes
 *                     on every run.  Either gradient pointer may be NULL, not both.  With more than one chunk the chunks run as grid.z slices and
 *                     grad_flow needs mpf_flow_warp_workspace bytes for their shares; whole != 0 makes one thread walk every chunk instead (no
 *                     workspace; the same bytes).
 * Limits: B <= 32767; H * W <= 2^30; B * C * H * W and B * 2 * H * W below 2^31. */
#define MPF_FLOW_WARP_WARP 0
#define MPF_FLOW_WARP_RIFE 1
#define MPF_FLOW_WARP_CHUNK 64
typedef struct MpfFlowWarpArgs {
    const float *x;                  /* [B,C,H,W] */
    const float *flow;               /* [B,2,H,W] */
    const float *lin_w;              /* [W]: torch.linspace(-1, 1, W); MPF_FLOW_WARP_RIFE only */
    const float *lin_h;              /* [H]: torch.linspace(-1, 1, H); MPF_FLOW_WARP_RIFE only */
    float *out;                      /* [B,C,H,W], written by mpf_flow_warp */
    float *mask;                     /* [B,1,H,W], written by mpf_flow_warp, or NULL */
    const float *grad_out;           /* [B,C,H,W]; read by mpf_flow_warp_bwd */
    float *grad_x;                   /* [B,C,H,W], added into by mpf_flow_warp_bwd, or NULL */
    float *grad_flow;                /* [B,2,H,W], written by mpf_flow_warp_bwd, or NULL */
    void *workspace;                 /* mpf_flow_warp_workspace(B, C, H, W, whole) bytes; read and written by mpf_flow_warp_bwd for grad_flow */
    size_t workspace_bytes;
    int mode;                        /* MPF_FLOW_WARP_WARP / _RIFE */
    int B, C, H, W;
    int whole;                       /* 0: channel chunks as grid.z slices; else one thread per pixel walks every channel */
} MpfFlowWarpArgs;
size_t mpf_flow_warp_workspace(int B, int C, int H, int W, int whole);    /* 0 where none is needed, and for a shape the calls refuse */
int mpf_flow_warp(const MpfFlowWarpArgs *a, void *stream);
int mpf_flow_warp_bwd(const MpfFlowWarpArgs *a, void *stream);

/* The first residual block of AdaMPI's plane-adjustment network (model/PAN.py:18-46, block 0 of its DownsizeEncoder) over the S plane-images of
 * each of B images, in eval mode, with its 2 x 2 average pool; INTEGRATION.md section 23 states it (tests/pan_restated.py restates it in float64).
 * The S inputs x_s = cat(rgb_low, disp_low, d_s) of an image differ only in the constant channel d_s = plane_disp[b,s], and conv1 / conv3 are
 * affine in it, so the launch splits in two:
 *   prologue, once per image   A1[o,y,x] = b1[o] + sum over the four image channels and the in-frame taps of w1[o,c,tap] * x[c,y+dy,x+dx]
 *                              B1[o,y,x] = sum over the in-frame taps of w1[o,4,tap]    (zero padding: it differs from the inner value only on the border)
 *                              A3[o,y,x] = bias3[o] + sum over the four image channels of w3[o,c] * x[c,y,x]
 *   per plane, fused           m = bn_scale * relu(A1 + d_s * B1) + bn_shift inside the frame, 0 outside it (conv2 pads ITS input with zeros);
 *                              v = relu(b2 + conv2(m) + A3 + d_s * w3[o,4]);  out = the mean of v over 2 x 2, h / 2 x w / 2 pixels (floor: an odd
 *                              last row / column is dropped, as avg_pool2d drops it).
 * bn_scale = weight / sqrt(running_var + eps) and bn_shift = bias - running_mean * bn_scale are folded by the caller.  All tensors f32, contiguous,
 * 4-byte aligned; sums in f32 with fused multiply-adds; no atomics: identical bytes on every run.  plane_disp is read on the device.  Everything is
 * validated before anything is launched (MPF_ERR_BAD_ARGUMENT): a NULL block or pointer, a pointer that is not 4-byte aligned, h or w below 2,
 * B or S below 1, a workspace that is too small, B * S * 8 * (h / 2) * (w / 2) or B * 8 * h * w of 2^31 or more, more than 65535 row tiles or
 * (image, plane group) slices.  Nothing synchronises with the host. */
#define MPF_PAN_C 8                  /* channels of the block: conv1 5 -> 8, conv2 8 -> 8, conv3 5 -> 8 */
#define MPF_PAN_PLANES_PER_GROUP 4   /* planes one workgroup walks with the tile's A1 / B1 / A3 in registers */
typedef struct MpfPanArgs {
    const float *rgb_low;            /* [B,3,h,w] */
    const float *disp_low;           /* [B,1,h,w] */
    const float *plane_disp;         /* [B,S] on the device */
    const float *w1, *b1;            /* conv1 [8,5,3,3], [8] */
    const float *bn_scale, *bn_shift;/* [8], [8]: the eval-mode BatchNorm folded */
    const float *w2, *b2;            /* conv2 [8,8,3,3], [8] */
    const float *w3, *b3;            /* conv3 [8,5,1,1], [8] */
    float *out;                      /* [B*S,8,h/2,w/2] */
    void *workspace;                 /* mpf_pan_block1_workspace(B, h, w) bytes: A1 [B,8,h,w], A3 [B,8,h,w], B1 [8,h,w]; contents irrelevant before the call */
    size_t workspace_bytes;
    int B, S, h, w;
} MpfPanArgs;
size_t mpf_pan_block1_workspace(int B, int h, int w);                     /* 0 for a shape the call refuses */
int mpf_pan_block1(const MpfPanArgs *a, void *stream);

/* The optimizer tail of RAFT/train.py (train.py:178-181: clip_grad_norm_, AdamW.step) over a whole parameter set, as one multi-tensor path:
 * the global gradient norm, the clip coefficient and torch's single-tensor AdamW update, without host synchronisation.  All tensors f32.
 *   mpf_grad_norm        total_norm [1] <- (float) sqrt(sum over every record with a gradient of g * g), the sum in f64: what clip_grad_norm_
 *                        returns.  Nothing else the caller owns is written.  The workspace keeps the sum (see norm_ready).
 *   mpf_adamw_clipped    the same norm, then coef = min(1, max_norm / (total_norm + 1e-6f)) in f32 (a NaN norm stays NaN) and per element, with
 *                        g = coef * grad, in f32 with every operation rounded on its own (no fused multiply-add; divide and sqrt correctly
 *                        rounded):
 *                            p = p * (1 - lr * weight_decay)
 *                            m = m + (1 - beta1) * (g - m)
 *                            v = beta2 * v + ((1 - beta2) * g) * g
 *                            p = p - ((lr / bias_correction1) * m) / (sqrt(v) / bias_correction2_sqrt + eps)
 *                        p, m and v are stored; grad is read only, or with zero_grad overwritten by zeros.  The five scalars in brackets and
 *                        beta2, bias_correction2_sqrt, eps are formed in double on the host and rounded to f32 once, as torch forms them.
 *                        coef == 1 (max_norm = +inf, or a norm below max_norm) multiplies exactly: the results are the unclipped ones bit for bit.
 * A record whose grad is NULL is skipped as torch skips `p.grad is None`: it is not counted in the norm and nothing of it is read or written.
 * The table `tensors` is a HOST array; the call copies at most MPF_OPT_TENSORS_PER_LAUNCH records into the arguments of each kernel launch,
 * so nothing the caller owns has to outlive the call and the pointers may change from call to call.  One workgroup handles MPF_OPT_CHUNK
 * consecutive elements of one tensor.  The norm: one f64 partial per workgroup, folded by one workgroup in a fixed order; no atomics, so every
 * result is bit-identical from run to run, and the same for any alignment of the tensors.  Tensors whose four pointers are 16-byte aligned are
 * read and written 16 bytes at a time; any 4-byte alignment works (an offset view).
 * workspace: mpf_adamw_workspace(tensors, count) bytes, 8-byte aligned: MPF_OPT_WORKSPACE_TAIL bytes (the sum of squares f64, the norm and the
 * coefficient f32) followed by one f64 per chunk of every record, whether its grad is NULL or not.  Contents irrelevant before the call.
 * norm_ready = 1 (mpf_adamw_clipped; several parameter groups under one global norm): the workspace is the one an earlier mpf_grad_norm on this
 * stream left, over whatever table that call had; this call takes the sum from it, forms total_norm and the coefficient for its own max_norm
 * and updates its own table.  MPF_OPT_WORKSPACE_TAIL bytes suffice then.
 * Validated before anything is launched (MPF_ERR_BAD_ARGUMENT): a NULL block, table, total_norm or workspace; count < 1; numel < 1; more than
 * MPF_OPT_MAX_CHUNKS chunks in all; a NULL param / exp_avg / exp_avg_sq (mpf_adamw_clipped) of a record with a gradient; a pointer that is not
 * 4-byte aligned; a workspace that is too small or not 8-byte aligned; and, by mpf_adamw_clipped, lr < 0, eps <= 0, weight_decay < 0, a beta
 * outside [0, 1), a bias correction outside (0, 1], max_norm <= 0 or NaN, any non-finite hyperparameter other than max_norm = +inf.
 * mpf_grad_norm reads no hyperparameter. */
#define MPF_OPT_CHUNK 4096               /* elements one workgroup handles */
#define MPF_OPT_TENSORS_PER_LAUNCH 64    /* tensor records passed by value per kernel launch */
#define MPF_OPT_WORKSPACE_TAIL 16        /* bytes at the head of the workspace: f64 sum of squares, f32 norm, f32 coefficient */
#define MPF_OPT_MAX_CHUNKS 8388608       /* 2^23: chunks of one call (a grid dimension of 256-thread workgroups stays below 2^31 threads) */
typedef struct MpfOptTensor {
    float *param, *exp_avg, *exp_avg_sq;     /* [numel] each, updated in place */
    float *grad;                             /* [numel], or NULL: the record is skipped */
    int64_t numel;
} MpfOptTensor;
typedef struct MpfAdamWArgs {
    const MpfOptTensor *tensors;             /* HOST array of `count` records; device pointers inside */
    int count;
    int zero_grad;                           /* 1: write zeros to every grad after it is consumed */
    int norm_ready;                          /* 1: take the sum of squares an earlier mpf_grad_norm left in the workspace */
    double lr, beta1, beta2, eps, weight_decay;
    double bias_correction1;                 /* 1 - beta1^t */
    double bias_correction2_sqrt;            /* sqrt(1 - beta2^t) */
    double max_norm;                         /* > 0; +inf = no clipping */
    float *total_norm;                       /* device, [1], written: the norm before clipping */
    void *workspace;
    size_t workspace_bytes;
} MpfAdamWArgs;
size_t mpf_adamw_workspace(const MpfOptTensor *tensors, int count);   /* 0 for a table the calls refuse */
int mpf_grad_norm(const MpfAdamWArgs *a, void *stream);
int mpf_adamw_clipped(const MpfAdamWArgs *a, void *stream);

/* [3,H,W] float RGB -> [H,W,3] u8 BGR, clip(rint(x*255))  (utils/utils.py:174-177) */
int mpf_to_u8_bgr(const float *d_img, int H, int W, uint8_t *d_out, void *stream);

/* Input stage.  Replaces, for one image: image_to_tensor / disparity_to_tensor after the file decode (utils/utils.py:35-52:
 * u8 / 255 in fp32 for the image, u8 / 255 in fp64 cast to fp32 for the disparity), the instance mask (ids == obj_index) as
 * float (gen_3dphoto_dynamic_v2.py:101-103) and the three F.interpolate(size=(H,W), mode='bilinear', align_corners=True) calls
 * (:86-89, :104-105), bit for bit as ATen's CPU kernels compute them.  d_rgb_u8 [h,w,3] -> d_image [3,H,W];
 * d_disp_u8 [h,w] -> d_disp [H,W]; d_ids_u8 [h,w] -> d_mask [H,W]; each pair optional (both NULL to skip). */
int mpf_prepare_inputs(const uint8_t *d_rgb_u8, const uint8_t *d_disp_u8, const uint8_t *d_ids_u8, int obj_index, int h, int w,
                       int H, int W, float *d_image, float *d_disp, float *d_mask, void *stream);

/* ================= generic (materialised-tensor) ops behind the utils/mpi function signatures ==================== */

/* get_src_xyz_from_plane_disparity (utils/mpi/mpi_rendering.py:213-239): params header K^-1 + S records (depth) */
int mpf_src_xyz(const float *d_params, int S, int H, int W, float *d_xyz_S3HW, void *stream);
/* transform_G_xyz (utils/mpi/rendering_utils.py:4-23): params header G; xyz [S,3,N] -> [S,3,N] */
int mpf_transform_xyz(const float *d_params, const float *d_xyz, int S, int64_t N, float *d_out, void *stream);
/* HomographySample.sample after H_src_tgt is known (utils/mpi/homography_sampler.py:124-158):
 * src [S,C,H,W] -> tgt [S,C,H,W], valid u8 [S,H,W] (NULL ok), flowB2A [S,H,W,2] (NULL ok) */
int mpf_homography_sample(const float *d_src, const float *d_params, int S, int C, int H, int W, float *d_tgt,
                          uint8_t *d_valid, float *d_flowB2A, void *stream);
/* HomographySample.sample_inverse after H_tgt_src is known (utils/mpi/homography_sampler.py:197-218): [S,H,W,2] */
int mpf_homography_flow(const float *d_params, int S, int H, int W, float *d_flow, void *stream);
/* plane_volume_rendering / plane_volume_rendering_flow / weighted_sum_mpi (utils/mpi/mpi_rendering.py:62-154) on
 * materialised rgb [S,3,N] (NULL ok), sigma [S,N], xyz [S,3,N]; extra_in [S,E,N] (E <= 4) is summed with the same
 * weights into extra_out [E,N] (flow and/or obj-mask).  hard != 0: extra is taken from the arg-max-weight plane only
 * (hard_flow, :126-130). */
int mpf_volume_render(const float *d_rgb, const float *d_sigma, const float *d_xyz, int S, int64_t N,
                      float *d_rgb_out, float *d_depth_out, float *d_tacc_out, float *d_weights_out,
                      const float *d_extra_in, int E, float *d_extra_out, int hard, void *stream);
/* Adjoint of mpf_volume_render with respect to rgb, sigma and the extras (xyz is constant).  Upstream gradients, each NULL when its output was not
 * used: g_rgb [3,N], g_depth [N], g_extra [E,N], g_weights [S,N], g_tacc [S,N].  Results: grad_rgb [S,3,N] (NULL ok), grad_sigma [S,N] (required: it
 * is also the kernel's only S-deep scratch), grad_extra [S,E,N] (NULL ok); every element is written, none needs initialising.  Two passes over the
 * planes per pixel, t / A / w recomputed with the forward's own helpers.  d_rgb == NULL: the flow form.  hard != 0 (flow form only): grad_extra goes to
 * the arg-max plane's values alone and grad_sigma is zero, as in torch, where the one-hot selection is constant. */
int mpf_volume_render_bwd(const float *d_rgb, const float *d_sigma, const float *d_xyz, const float *d_extra_in, int S, int64_t N, int E, int hard,
                          const float *d_g_rgb, const float *d_g_depth, const float *d_g_extra, const float *d_g_weights, const float *d_g_tacc,
                          float *d_grad_rgb, float *d_grad_sigma, float *d_grad_extra, void *stream);
/* Adjoint of mpf_homography_sample with respect to src, for the channels [c0, c1): g_src [S,C,H,W] += weight * g_tgt [S,C,H,W] through the taps the
 * forward read (same d_params), as float atomic adds: d_g_src must be zero-initialised (or hold a sum to add to), channels outside the range are not
 * touched, and the last bits of the result depend on the order in which the adds arrive.  valid and flowB2A have no gradient. */
int mpf_homography_sample_bwd(const float *d_g_tgt, const float *d_params, int S, int C, int H, int W, int c0, int c1, float *d_g_src, void *stream);
/* mpf_volume_render_bwd plus the gradient of xyz: d_grad_xyz [S,3,N] (NULL: exactly mpf_volume_render_bwd).  With dL/dt_j of that adjoint:
 * dL/ddist_j = -sigma_j t_j dL/dt_j (j < S-1; the last distance is the constant 1e3), u_j = (xyz_{j+1} - xyz_j) / dist_j (0 where dist_j = 0, as torch's
 * norm), dL/dxyz_s = u_{s-1} dL/ddist_{s-1} - u_s dL/ddist_s + (0, 0, 1) g_depth w_s / (D + 1e-5).  hard != 0: exactly zero.  One store per element, no
 * atomics: two runs give the same bits. */
int mpf_volume_render_bwd_xyz(const float *d_rgb, const float *d_sigma, const float *d_xyz, const float *d_extra_in, int S, int64_t N, int E, int hard,
                              const float *d_g_rgb, const float *d_g_depth, const float *d_g_extra, const float *d_g_weights, const float *d_g_tacc,
                              float *d_grad_rgb, float *d_grad_sigma, float *d_grad_extra, float *d_grad_xyz, void *stream);
/* The per-plane sums over all pixels of the three launchers below use no atomics: wave sum -> LDS slot [wave][s] -> d_partial [blocks, S] (a workspace
 * of the caller's, partial_blocks rows, nothing to initialise) -> a second kernel that adds the rows in order, in double.  S < 4096.
 *
 * Adjoint of mpf_src_xyz with respect to the plane DISPARITIES (same d_params): g_xyz [S,3,H,W] -> grad_disparity [S],
 * dL/ddisparity_s = -depth_s^2 sum_p <g_s(p), K^-1 (x, y, 1)>.  blocks = ceil(H*W / 256). */
int mpf_src_xyz_bwd(const float *d_g_xyz_S3HW, const float *d_params, int S, int H, int W, float *d_partial, int partial_blocks,
                    float *d_grad_disparity, void *stream);
/* Adjoint of mpf_homography_flow with respect to the plane DEPTH d_s of H_s = K_tgt (R + t n^T / d_s) K_src^-1, n = (0, 0, 1): g_flow [S,H,W,2] ->
 * grad_depth [S].  d_params: mpf_homography_flow's records (H_tgt_src in [0..8]) with [9] = d_s, [10..12] = K_tgt t and [13..15] = the third row of
 * K_src^-1; d(X, Y, Z)/dd = -(K_tgt t) <row, (x, y, 1)> / d^2 and the flow's derivative follows by the quotient rule.  blocks = ceil(H*W / 256). */
int mpf_plane_flow_bwd(const float *d_g_flow_SHW2, const float *d_params, int S, int H, int W, float *d_partial, int partial_blocks, float *d_grad_depth,
                       void *stream);

/* weighted_sum_mpi's sums with caller-supplied weights (utils/mpi/mpi_rendering.py:143-152):
 * out[c,n] = cascade-sum_s weights[s,n] * values[s,c,n]   (values NULL: plain sum of the weights, C must be 1) */
int mpf_weighted_sum(const float *d_weights, const float *d_values, int S, int C, int64_t N, float *d_out, void *stream);

/* alpha_composition (utils/mpi/mpi_rendering.py:42-59) and the blend weights of render(use_alpha=True) (:36):
 * d_alpha [S,N]; d_values [S,C,N] with d_out [C,N] = cascade-sum_s values * weights (both NULL to skip);
 * d_weights [S,N] = alpha_s * prod_{k<s}(1 - alpha_k) (optional); d_cumprod_eps [S,N] = prod_{k<=s}(1 - alpha_k + 1e-6) (optional) */
int mpf_alpha_composite(const float *d_alpha, const float *d_values, int S, int C, int64_t N, float *d_out, float *d_weights,
                        float *d_cumprod_eps, void *stream);

/* ================= depth -> flow projection and forward warp (geometry.py, moving_obj.py, warping.c) ============= */

/* moving_obj.py:29-30: depth = 1 / (disp + 0.005), values above 100 clamped to 100 */
int mpf_disp_to_depth(const float *d_disp, int64_t N, float *d_depth, void *stream);
/* BackprojectDepth + Project3D (geometry.py:41-49, :63-76): depth [H,W]; inv_K 3x3 and P = (K.T)[:3,:] 3x4 passed BY
 * VALUE from host pointers; outputs pix [H,W,2] (normalised as the reference returns them) and z [H,W]. */
int mpf_backproject_project(const float *d_depth, const float *h_inv_k9, const float *h_P12, int H, int W,
                            float *d_pix, float *d_z, void *stream);
/* The two halves on their own, for the class-level drop-ins: BackprojectDepth.forward -> cam points [4,N] (rows X,Y,Z,1)
 * and Project3D.forward on arbitrary homogeneous points [4,N] with eps (geometry.py:55, :70). */
int mpf_backproject(const float *d_depth, const float *h_inv_k9, int H, int W, float *d_cam_points, void *stream);
int mpf_project3d(const float *d_points_4N, const float *h_P12, float eps, int H, int W, float *d_pix, float *d_z,
                  void *stream);
/* moving_obj.py:108-124, :153: select object/static projection by instance mask, to pixel units, truncate + clamp.
 * outputs p1 [H,W,2], z1 [H,W], safe_x/safe_y int64 [H,W], flow01 [H,W,2] */
int mpf_select_truncate(const float *d_p_static, const float *d_z_static, const float *d_p_obj, const float *d_z_obj,
                        const float *d_inst, int H, int W, float *d_p1, float *d_z1, int64_t *d_safe_x,
                        int64_t *d_safe_y, float *d_flow01, void *stream);
/* moving_obj.py:29-124 and :153 fused into one pass: depth from disparity, back-projection, the static and the object
 * projection (selected per pixel by the instance mask), pixel units, truncation + clamp, flow = p1 - p0.
 * inv_K 3x3, P_static = (K.T1)[:3,:], P_obj = (K.Ti)[:3,:] by value from host pointers. */
int mpf_moving_object_project(const float *d_disp, const float *h_inv_k9, const float *h_P_static12, const float *h_P_obj12,
                              const float *d_inst, int H, int W, float *d_p1, float *d_z1, int64_t *d_safe_x,
                              int64_t *d_safe_y, float *d_flow01, void *stream);
/* Order-preserving parallel equivalent of warping.c:6-33 on device buffers.  d_warped u8 [h,w,5] is fully written
 * (no need to zero it).  d_workspace: mpf_forward_warp_workspace(h,w) bytes of scratch. */
size_t mpf_forward_warp_workspace(int h, int w);
int mpf_forward_warp(const uint8_t *d_src, const int64_t *d_idx, const int64_t *d_idy, const float *d_z,
                     uint8_t *d_warped, int h, int w, void *d_workspace, size_t workspace_bytes, void *stream);
/* moving_obj.py:133-150: masks H, M, M' = dilate3x3(M), P = (M' == M), H' = H*P, each u8 [H,W] */
int mpf_warp_masks(const uint8_t *d_warped, int H, int W, uint8_t *d_Hm, uint8_t *d_M, uint8_t *d_Md, uint8_t *d_P,
                   uint8_t *d_Hp, void *stream);

/* moving_obj.py:29-150 in ONE call on device buffers: mpf_moving_object_project (fused into the first pass of the forward warp's sort:
 * the int64 targets are written for the caller but never read back), mpf_forward_warp, mpf_warp_masks - 5 launches, no allocation.
 * The source frame that is splatted (moving_obj.py:124), ONE of: d_src_u8 u8 [H,W,3], or d_src_f32_3HW float [3,H,W] in 0..1 whose
 * uint8 BGR form (utils/utils.py:174-177: rint(255 v), clamped - what Stage A+C writes as the pair's source frame) is splatted, converted
 * per winner on the fly, so that the chain needs no output of the render path.  Masks: all five pointers or none.
 * d_workspace: mpf_forward_warp_workspace(H, W) bytes, 256-byte aligned. */
typedef struct MpfMovingObjectOut {
    float *d_p1, *d_z1;               /* [H,W,2], [H,W] */
    int64_t *d_safe_x, *d_safe_y;     /* [H,W] */
    float *d_flow01;                  /* [H,W,2] */
    uint8_t *d_warped;                /* [H,W,5] */
    uint8_t *d_Hm, *d_M, *d_Md, *d_P, *d_Hp;   /* [H,W] each */
} MpfMovingObjectOut;
int mpf_moving_object_chain(const float *d_disp, const float *h_inv_k9, const float *h_P_static12, const float *h_P_obj12,
                            const float *d_inst, const uint8_t *d_src_u8, const float *d_src_f32_3HW, int H, int W,
                            const MpfMovingObjectOut *out, void *d_workspace, size_t workspace_bytes, void *stream);

/* ================= MPI producer network: 3x3 convolution engine ====================== */

/* One launch = one 3x3 / pad 1 / stride 1|2 convolution over S plane-images with its surrounding plumbing fused:
 * the LOADER synthesises the layer's (virtual) NHWC input, the EPILOGUE applies bias / BatchNorm / activation / gate.
 * Replaces, for S planes at once: ConvBNReLU (model/CPN/unet.py:6-15), GatedConv + ELU + BatchNorm
 * (model/CPN/decoder.py:10-71) and the expand / cat / ReflectionPad2d / upsample tensors around them
 * (model/CPN/unet.py:44-66, model/CPN/decoder.py:131-163).  Activations: fp16 NHWC, channels padded to a multiple of 8.
 * fp16 MFMA, fp32 accumulation, fp32 epilogue - the precision of the reference's own GPU run (.half(),
 * gen_3dphoto_dynamic_v2.py:46,59,82-84). */
#define MPF_CONV_LD_FMN_INPUT     0   /* (r,g,b,disparity,plane disparity,0,0,0): srcA = image f32 [3,H,W], srcB = disparity f32 [H,W], plane_vals f32 [S] */
#define MPF_CONV_LD_DIRECT        1   /* srcA f16 [S,Hin,Win,CA] */
#define MPF_CONV_LD_BILINEAR_CAT  2   /* x2 bilinear (align_corners) of srcA f16 [S,HA,WA,CA]  ++  srcB f16 [S,Hin,Win,CB]; fparams = {(HA-1)/(Hin-1), (WA-1)/(Win-1)} */
#define MPF_CONV_LD_NEAREST_PLANE 3   /* x2 nearest (or same size) of srcA f16 [S,HA,WA,CA] (CA may be 0)  ++  per-plane skip: srcB f16 [Hin,Win,CB-8] shared
                                         features * cm[s], then (cm[s], fm[s], 0 x6); cm, fm f32 [S,Hin,Win]; CB == 0: no skip */
#define MPF_CONV_LD_FMN_SYNTH      4   /* the feature-mask network's first layer never materialised: channels = relu(A' + plane_vals[s] * B'), srcA = A', srcB = B',
                                         both f32 [Hin,Win,16] (A' = its pre-activation output for plane value 0, B' = the plane channel's share) */
#define MPF_CONV_LD_BILINEAR_SYNTH 5   /* LD_BILINEAR_CAT whose skip source is synthesised the same way: srcB = A', cm = B' f32 [Hin,Win,16], CB = 16 */
#define MPF_CONV_LD_NEAREST_PHASE   6   /* LD_NEAREST_PLANE with HA = Hin / 2, reflection padding, PHASE-DECOMPOSED: on the upsampled source the 3x3 window of an output pixel covers
                                            2 x 2 distinct srcA pixels, chosen - with host-summed weights - by the pixel's phase (y & 1, x & 1); 4 taps instead of 9 there, the skip
                                            source as in LD_NEAREST_PLANE.  Chunks: ceil(CA / ct) of srcA, then ceil(CB / ct) of the skip; wpack = [chunkA][phase 2 py + px][ksteps(4 taps)]
                                            [nblk][64][8] ++ [chunkB][ksteps(9 taps)][nblk][64][8]  (engine.py: pack_weights_up).  Gated epilogues 2 / 6 only */
#define MPF_CONV_EP_AFFINE_RELU      0   /* out f16 [S,Hout,Wout,Cst] = relu(acc * ep[0][row] + ep[1][row]) */
#define MPF_CONV_EP_AFFINE_RELU_F32  1   /* same, output channel 0 only, out f32 [S,Hout,Wout] */
#define MPF_CONV_EP_GATED_ELU        2   /* g = (accF + ep[0][rowF]) * sigmoid(accM + ep[0][rowM]); out f16 NHWC = elu(g * ep[1][rowF] + ep[2][rowF]) */
#define MPF_CONV_EP_AFFINE_F32_NHWC  4   /* out f32 [S,Hout,Wout,Cst] = acc * ep[0][row] + ep[1][row], NO activation */
#define MPF_CONV_EP_GATED_PLANAR_F32 3   /* out f32 [S,Cst,Hout,Wout] = g (no BatchNorm / activation: the decoder's raw output layer) */
#define MPF_CONV_EP_GATED_ELU_PAIRED 6   /* EP_GATED_ELU with feature / gate rows interleaved (packed row 2c = feature c, 2c+1 = gate c; ep[1], ep[2] indexed by channel):
                                           24 output channels in 3 blocks instead of 4 */
#define MPF_CONV_EP_GATED_PLANAR_F32_PAIRED 5 /* the same from ONE 16-row block (nblk = 1, Cst <= 8): packed row 2c = feature c, row 2c+1 = gate c */

typedef struct MpfConvArgs {
    const void *srcA, *srcB;          /* see the loader */
    const float *cm, *fm;             /* per-plane masks at the conv-input resolution (LD_NEAREST_PLANE with CB > 0) */
    const float *plane_vals;          /* LD_FMN_INPUT */
    const void *wpack;                /* f16 weights in MFMA-fragment order: [nchunk][ksteps][nblk][64 lanes][8]   (mpiflow_amd/model/engine.py: pack_weights) */
    const float *ep;                  /* f32 [3][nblk*16] epilogue rows, in packed row order */
    void *out;
    int S, Hin, Win, Hout, Wout;      /* Hin x Win: the virtual conv input (after upsampling / concatenation) */
    int CA, CB, HA, WA;               /* padded channels of the two sources; size of source A */
    int ct, nchunk;                   /* channels staged per tap and chunk (8, 16, 32); number of chunks */
    int nblk, ncg;                    /* 16-row output blocks in total; workgroup column groups (nblk % ncg == 0) */
    int Cst;                          /* channels of the output tensor (NHWC pitch, or planes for the planar epilogue) */
    int loader, epi, stride, pad_mode; /* pad_mode 0 zero, 1 reflection */
    float fparams[4];
    int wlds;                         /* 1: the A fragments of a chunk are staged in LDS once per workgroup (many-chunk / many-block
                                         layers), 0: every wave loads its fragments from global memory (tuning choice, same results) */
    int plane_major;                  /* 1: the plane index is the fastest grid dimension (the S workgroups of a tile back to back: per-image sources
                                         shared by the planes stay in L2); scheduling only, same results */
    int bprime_table;                 /* LD_FMN_SYNTH / LD_BILINEAR_SYNTH: 1 = B' (srcB / cm) is the [3][3][16] table of its border classes (top / inner / bottom row x
                                         left / inner / right column: B' depends on the pixel only through which taps fall inside the image), 0 = an [Hin,Win,16] map */
    int pw;                           /* planes per workgroup (0 / 1: one): a workgroup walks pw consecutive planes at its tile position and computes what depends
                                         on the pixel only once (nblk / ncg <= 2 only; S % pw == 0); scheduling only, same results */
} MpfConvArgs;

int mpf_conv3x3_f16(const MpfConvArgs *args, void *stream);

/* The plane masks of the decoder in one pass over the feature-mask logits [S,H,W] (model/CPN/unet.py:68-69 softmax over the
 * planes; model/CPN/decoder.py:126-130 cumulative and context masks; :131-150 their adaptive_avg_pool2d at every decoder
 * scale).  Outputs: d_feature_mask [S,H,W] (optional), d_cum_mask [S,H,W], and for the five scales k = 2,4,8,16,32
 * d_cm[i], d_fm[i] [S,H/k,W/k] = the k x k block means of the context mask (1 - cumulative mask of the planes in front)
 * and of the feature mask.  d_cm / d_fm are HOST arrays of 5 device pointers.  H, W multiples of 32. */
int mpf_plane_masks(const float *d_logits, int S, int H, int W, float *d_feature_mask, float *d_cum_mask, float *const *d_cm,
                    float *const *d_fm, void *stream);

/* ---- the single-image part of the producer in fp32: RGBD ResNet-18 encoder + the decoder's bottleneck ----------------------
 * (model/CPN/encoder.py:20-101: conv1 7x7/2 + bn1 + relu, maxpool, layer1-4 of two BasicBlocks each;
 *  model/CPN/decoder.py:85-88,131-138: maxpool, conv1x1 + BN + LeakyReLU(0.1), maxpool, conv3x3, x2 nearest, conv3x3, x2 nearest, conv1x1.)
 * Activations: fp32 NHWC.  fp32 MFMA (v_mfma_f32_16x16x4_f32), fp32 epilogue. */

/* x = cat((image - mean) / std, disparity) (model/CPN/encoder.py:84-85,89-93): image f32 [3,H,W], disparity f32 [H,W] -> f32 [H,W,4] */
int mpf_encoder_input(const float *d_image_3HW, const float *d_disp_HW, int H, int W, float *d_out_HW4, void *stream);

/* One convolution (no bias) + per-channel affine (BatchNorm folded) [+ residual] + activation over one NHWC fp32 image:
 *   out[p, c] = act(conv(src)[p, c] * scale[c] + shift[c] (+ residual[p, c])),  zero padding.
 * up = 1: the convolution's input is the x2 nearest-neighbour upsampling of src (Hin x Win is the UPSAMPLED size; src is [Hin/2, Win/2, Cin]).
 * wpack: f32 [Cout/16][nsteps][64 lanes][4], nsteps = ceil(ksize^2 * Cin/4 / 4): lane (m = l % 16, g = l / 16) of step s holds, for j = 0..3,
 *   W[16 blk + m][channel 4 (v % (Cin/4)) + j][tap v / (Cin/4)] with v = 4 s + g, zero when the tap index exceeds ksize^2 - 1
 *   (mpiflow_amd/model/engine.py: pack_weights_f32).  Cin a power of two >= 4, Cout a multiple of 32.
 * out (f32) and out_f16 (f16, same NHWC shape: what the per-plane decoder's loaders read) are both optional, at least one is required. */
typedef struct MpfConv2dArgs {
    const float *src;
    const float *wpack;
    const float *scale, *shift;       /* f32 [Cout] */
    const float *residual;            /* f32 [Hout,Wout,Cout] or NULL */
    float *out;                       /* f32 [Hout,Wout,Cout] or NULL */
    void *out_f16;                    /* f16 [Hout,Wout,Cout] or NULL */
    int Hin, Win, Cin, Hout, Wout, Cout;
    int ksize, stride, pad;           /* ksize 1, 3 or 7; stride 1 or 2 */
    int up;                           /* 0, or 1: x2 nearest upsampling of src in front of the convolution */
    int act;                          /* 0 none, 1 ReLU, 2 LeakyReLU(slope) */
    float slope;
} MpfConv2dArgs;
int mpf_conv2d_f32(const MpfConv2dArgs *args, void *stream);

/* nn.MaxPool2d(3, stride 2, padding 1) on an NHWC fp32 image: [Hin,Win,C] -> [(Hin-1)/2+1, (Win-1)/2+1, C]; C a multiple of 4 */
int mpf_maxpool3x3s2_f32(const float *d_src_HWC, int Hin, int Win, int C, float *d_out, void *stream);

/* ---- the producer network's PARITY-GRADE engine: fp32 or fp64 throughout (mpiflow_amd/csrc/mpf_pconv.hip) -------------------------
 * Every convolution of MPIPredictor.forward (model/AdaMPI.py:55-78) in the arithmetic of the reference's CPU path: fp32 storage, fp32
 * products, fp32 accumulation (v_mfma_f32_16x16x4_f32), or fp64 throughout (v_mfma_f64_16x16x4_f64) - `dtype` selects.  Activations are
 * NHWC tensors of `dtype` with the channel count zero-padded to a multiple of 4; the accuracy mode behind
 * `gen_3dphoto_dynamic.py --model-engine hip --model-dtype fp32|fp64` (mpiflow_amd/model/precise.py: PrecisePredictor). */
#define MPF_DTYPE_F32 0
#define MPF_DTYPE_F64 1
#define MPF_DTYPE_F32X3      2 /* mpf_pconv only: fp32 tensors; every product a b from the three bf16 pieces each factor is exactly the sum of (six of the nine
                                * piece products: a relative 2^-24 per product dropped) on v_mfma_f32_16x16x32_bf16; accumulation as MPF_DTYPE_F32.  1 x 1 and 3 x 3.
                                * wpack: [nblk][steps][3 pieces][64 lanes][8] bf16, a step = two K-steps of the fp32 packing, every source padded to an even count */
#define MPF_DTYPE_F32X3_TILE 3 /* the same arithmetic for 3 x 3 / stride 1 / padding 1 layers with CA + CB <= 56 and nblk <= 3: the input tile of both sources is
                                * split once into LDS.  wpack: K-vector 4 t + g = (tap, 8-channel vector of the CONCATENATED channels, zero-padded to 8) */
#define MPF_DTYPE_F32X3_CHUNK 4 /* the same arithmetic for 3 x 3 / stride 1 / padding 1 layers of any width: per 32-channel chunk of the concatenated sources the input tile is
                                * split once into LDS, nine steps (one per tap) per chunk.  wpack: step = chunk * 9 + tap, K-vector g = 8-channel vector g of the chunk */
#define MPF_PCONV_EP_AFFINE       0   /* out [S,Hout,Wout,Cst] = act(acc * scale[row] + shift[row] (+ residual))   (ConvBNReLU model/CPN/unet.py:6-15; the encoder's conv + BN) */
#define MPF_PCONV_EP_AFFINE_MAP   1   /* same, row 0 only, out [S,Hout,Wout]   (the feature-mask logits, model/CPN/unet.py:66) */
#define MPF_PCONV_EP_GATED        2   /* g = accF * sigmoid(accM) (biases = initial accumulators); out NHWC = elu(g * scale[c] + shift[c])   (model/CPN/decoder.py:10-71) */
#define MPF_PCONV_EP_GATED_PLANAR 3   /* out [S,Cst,Hout,Wout] = g   (the decoder's raw output layer, model/CPN/decoder.py:164-165) */

/* One convolution over S plane-images (or one image, S = 1):  input = cat(A', B) along channels, A' = srcA or its x2 nearest up-sampling
 * (up = 1; HA = Hin / 2), zero or reflection padding, ksize 1 | 3 | 7, stride 1 | 2.
 * wpack: [nblk][nsteps][64 lanes][4] of dtype; K runs over source A's (tap, 4-channel vector) pairs, then over source B's: nsteps = nstA + nstB,
 *   nstX = ceil(ksize^2 * (CX/4) / 4).  Lane (m = l % 16, g = l / 16) of step s of source X holds, for j = 0..3, W[physical row 16 blk + m][channel
 *   4 (v % VX) + j of X][tap v / VX] with v = 4 s + g, VX = CX/4, zero past X's last tap.
 *   LOGICAL row L of a block (what the epilogue rows are indexed by) sits at physical row L for fp32 and at (L >> 2) + 4 (L & 3) for fp64
 *   (the C/D register layouts of the two MFMA instructions differ).  Gated epilogues: logical rows (2c, 2c+1) of the packed row sequence
 *   = (feature, gate) of channel c; bias [nblk*16] by logical row; scale / shift [nblk*8] by channel.  Affine epilogues: scale / shift
 *   [nblk*16] by logical row (conv bias folded into shift). */
typedef struct MpfPConvArgs {
    const void *srcA;                 /* dtype [S (or 1 when shareA), HA, WA, CA] */
    const void *srcB;                 /* dtype [S (or 1 when shareB), Hin, Win, CB] or NULL (CB = 0) */
    const void *wpack;
    const void *scale, *shift;        /* dtype, see above */
    const void *bias;                 /* dtype [nblk*16], gated epilogues only */
    const void *residual;             /* dtype [S,Hout,Wout,Cst] or NULL (EP_AFFINE) */
    void *out;
    int dtype;                        /* MPF_DTYPE_F32 | MPF_DTYPE_F64 | MPF_DTYPE_F32X3 | MPF_DTYPE_F32X3_TILE (tensors fp32 for the last two) */
    int S, Hin, Win, Hout, Wout;      /* Hin x Win: the virtual conv input (after up-sampling) */
    int HA, WA, CA, CB;
    int up, shareA, shareB;           /* up: 0 | 1 = x2 nearest up-sampling of srcA in front of the convolution | 2 (round 6; MPF_DTYPE_F32X3_TILE, 3 x 3 / stride 1 / reflection padding,
                                         CB = 0) = the same layer PHASE-DECOMPOSED: four 2 x 2 convolutions on the low-resolution map, wpack = [phase 2 py + px][row block][steps of
                                         4 taps] with the nine weights summed per phase in float64 (mpiflow_amd/model/precise.py: pack_weights_x3_tile_phase) */
    int ksize, stride, pad, pad_mode; /* pad_mode 0 zero, 1 reflection (pad 1) */
    int nblk, Cst, epi, act;          /* act: 0 none, 1 ReLU, 2 LeakyReLU(slope) (affine epilogues) */
    double slope;                     /* rounded to `dtype` by the kernel, as torch rounds the Python float to the tensor's dtype */
} MpfPConvArgs;
int mpf_pconv(const MpfPConvArgs *args, void *stream);

/* the tensors the reference builds with expand / cat / Upsample / adaptive_avg_pool2d, materialised in `dtype`:
 * mpf_pfmn_input      cat(image, disparity, plane disparity) per plane (model/CPN/unet.py:44-50) -> [S,H,W,8] (channels 5..7 zero)
 * mpf_pencoder_input  cat((image - mean) / std, disparity) (model/CPN/encoder.py:84-85,89-93) -> [H,W,4]
 * mpf_pbilinear2x     nn.Upsample(x2, bilinear, align_corners=True) (model/CPN/unet.py:42): [S,h,w,C] -> [S,2h,2w,C]
 * mpf_pper_plane      cat(feat * context_mask, context_mask, feature_mask) (model/CPN/decoder.py:140-150): feat [h,w,C], masks [S,h,w] -> [S,h,w,C+4]
 * mpf_pplane_masks    softmax over the planes (model/CPN/unet.py:68-69), cumulative / context masks (model/CPN/decoder.py:126-130) and their
 *                     k x k block means for k = 2..32 (adaptive_avg_pool2d, :143-146); d_cm / d_fm are HOST arrays of 5 device pointers
 * mpf_pmaxpool3x3s2   nn.MaxPool2d(3, 2, 1) on [Hin,Win,C] */
int mpf_pfmn_input(const float *d_image_3HW, const float *d_disp_HW, const float *d_plane_vals, int S, int H, int W, void *d_out, int dtype, void *stream);
int mpf_pencoder_input(const float *d_image_3HW, const float *d_disp_HW, int H, int W, void *d_out, int dtype, void *stream);
int mpf_pbilinear2x(const void *d_src, int S, int h, int w, int C, void *d_dst, int dtype, void *stream);
int mpf_pper_plane(const void *d_feat_hwC, const void *d_cm, const void *d_fm, int S, int h, int w, int C, void *d_out, int dtype, void *stream);
int mpf_pplane_masks(const void *d_logits, int S, int H, int W, void *d_feature_mask, void *d_cum_mask, void *d_context_mask, void *const *d_cm,
                     void *const *d_fm, int dtype, void *stream);
int mpf_pmaxpool3x3s2(const void *d_src_HWC, int Hin, int Win, int C, void *d_out, int dtype, void *stream);

/* THE REFERENCE'S FFI SYMBOL (external/forward_warping/warping.c:6; bound at moving_obj.py:12-13, called at :127-129).
 * Same name, same argument meaning, HOST pointers: src u8 [h*w*3], idx/idy int64 [h*w] (pre-clamped by the caller, as
 * in the reference), z f32 [h*w], warped u8 [h*w*5] (caller-owned).  Synchronous.  Runs the HIP kernels above on the
 * current device (copies in, warps, copies out); there is no CPU implementation behind it - without a GPU it prints
 * the HIP error to stderr and leaves `warped` untouched (the reference signature has no error channel). */
void forward_warping(const void *src, const void *idx, const void *idy, const void *z, void *warped, int h, int w);
/* same, with an error code */
int mpf_forward_warping_host(const void *src, const void *idx, const void *idy, const void *z, void *warped, int h,
                             int w);

#ifdef __cplusplus
}
#endif
#endif
