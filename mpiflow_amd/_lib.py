"""ctypes binding of libmpiflow_hip.so (C ABI: include/mpiflow_hip.h).

The shared library is built in-tree by `python __graft_entry__.py` / `make -C mpiflow_amd/csrc` with
`hipcc --offload-arch=gfx950`.  There is NO fallback: if the library is missing or a call fails, this module raises.
"""
import ctypes
import os

# PyTorch bundles its own libamdhip64.so (same SONAME as /opt/rocm's).  It must be the first HIP runtime mapped into the
# process so that libmpiflow_hip.so binds to the one that owns torch's device context and streams; loading ours first
# leaves two half-initialised runtimes ("no ROCm-capable device is detected").
import torch  # noqa: F401,E402

_HERE = os.path.dirname(os.path.abspath(__file__))
# MPIFLOW_HIP_LIB: development hook for same-box A/B timing of two builds of the library (tools/); symbols an older build lacks are skipped
LIB_PATH = os.environ.get("MPIFLOW_HIP_LIB") or os.path.join(_HERE, "libmpiflow_hip.so")

# the WITNESS build of the same sources (-DMPF_WITNESS): + retired kernel variants and timing ablations, selectable through mpf_tune keys the product library
# refuses.  Test / tool infrastructure: the product never loads it on its own (witness() / select_witness() below).
WITNESS_PATH = os.path.join(_HERE, "libmpiflow_hip_witness.so")

_lib = None
_witness = None

c_p = ctypes.c_void_p
c_i = ctypes.c_int
c_f = ctypes.c_float
c_i64 = ctypes.c_int64
c_sz = ctypes.c_size_t



class MpfConvArgs(ctypes.Structure):
    """struct MpfConvArgs of include/mpiflow_hip.h (field order and types must match)."""
    _fields_ = [("srcA", c_p), ("srcB", c_p), ("cm", c_p), ("fm", c_p), ("plane_vals", c_p), ("wpack", c_p), ("ep", c_p),
                ("out", c_p),
                ("S", c_i), ("Hin", c_i), ("Win", c_i), ("Hout", c_i), ("Wout", c_i),
                ("CA", c_i), ("CB", c_i), ("HA", c_i), ("WA", c_i),
                ("ct", c_i), ("nchunk", c_i), ("nblk", c_i), ("ncg", c_i), ("Cst", c_i),
                ("loader", c_i), ("epi", c_i), ("stride", c_i), ("pad_mode", c_i),
                ("fparams", c_f * 4), ("wlds", c_i), ("plane_major", c_i), ("bprime_table", c_i), ("pw", c_i)]


class MpfConv2dArgs(ctypes.Structure):
    """struct MpfConv2dArgs of include/mpiflow_hip.h: one fp32 convolution of the single-image encoder / bottleneck."""
    _fields_ = [("src", c_p), ("wpack", c_p), ("scale", c_p), ("shift", c_p), ("residual", c_p), ("out", c_p), ("out_f16", c_p),
                ("Hin", c_i), ("Win", c_i), ("Cin", c_i), ("Hout", c_i), ("Wout", c_i), ("Cout", c_i),
                ("ksize", c_i), ("stride", c_i), ("pad", c_i), ("up", c_i), ("act", c_i), ("slope", c_f)]


class MpfPConvArgs(ctypes.Structure):
    """struct MpfPConvArgs of include/mpiflow_hip.h: one convolution of the parity-grade (fp32 / fp64) producer engine."""
    _fields_ = [("srcA", c_p), ("srcB", c_p), ("wpack", c_p), ("scale", c_p), ("shift", c_p), ("bias", c_p), ("residual", c_p), ("out", c_p),
                ("dtype", c_i), ("S", c_i), ("Hin", c_i), ("Win", c_i), ("Hout", c_i), ("Wout", c_i),
                ("HA", c_i), ("WA", c_i), ("CA", c_i), ("CB", c_i), ("up", c_i), ("shareA", c_i), ("shareB", c_i),
                ("ksize", c_i), ("stride", c_i), ("pad", c_i), ("pad_mode", c_i), ("nblk", c_i), ("Cst", c_i), ("epi", c_i), ("act", c_i), ("slope", ctypes.c_double)]


class MpfWarpView(ctypes.Structure):
    """struct MpfWarpView of include/mpiflow_hip.h: one view of mpf_warp_composite_views (device pointers)."""
    _fields_ = [("d_params", c_p), ("d_mask_quads", c_p), ("d_rgb", c_p), ("d_depth", c_p), ("d_objmask", c_p),
                ("d_tgt_mask", c_p), ("d_rgb_u8_bgr", c_p)]


class MpfViewSupport(ctypes.Structure):
    """struct MpfViewSupport of include/mpiflow_hip.h: the mask support map one view of a Stage B launch tests (device pointer, tag, merge threshold)."""
    _fields_ = [("d_cells", c_p), ("tag", ctypes.c_uint32), ("thresh", c_f)]


class MpfMovingObjectOut(ctypes.Structure):
    """struct MpfMovingObjectOut of include/mpiflow_hip.h: the output buffers of mpf_moving_object_chain (device pointers)."""
    _fields_ = [("d_p1", c_p), ("d_z1", c_p), ("d_safe_x", c_p), ("d_safe_y", c_p), ("d_flow01", c_p), ("d_warped", c_p),
                ("d_Hm", c_p), ("d_M", c_p), ("d_Md", c_p), ("d_P", c_p), ("d_Hp", c_p)]


class MpfMergeArgs(ctypes.Structure):
    """struct MpfMergeArgs of include/mpiflow_hip.h: mpf_merge's arguments, for the merge folded into a pair launch."""
    _fields_ = [("d_frame", c_p), ("d_frame_dyn", c_p), ("d_mask", c_p), ("d_mask_dyn", c_p), ("d_flow", c_p), ("d_flow_dyn", c_p),
                ("d_obj_mask", c_p), ("thresh", c_f), ("d_flow_mix", c_p), ("d_frame_mix", c_p), ("d_fill_mask", c_p), ("obj_mask_stride", c_i)]


class MpfAugmentSample(ctypes.Structure):
    """struct MpfAugmentSample of include/mpiflow_hip.h: one sample of mpf_augment_pairs (device pointers, crop / resize / flip parameters)."""
    _fields_ = [("src", c_p), ("dst", c_p), ("flow", c_p), ("resize", c_i), ("scale_x", ctypes.c_double), ("scale_y", ctypes.c_double),
                ("Hr", c_i), ("Wr", c_i), ("flip_h", c_i), ("flip_v", c_i), ("y0", c_i), ("x0", c_i)]


class MpfSparseAugmentSample(ctypes.Structure):
    """struct MpfSparseAugmentSample of include/mpiflow_hip.h: one sample of mpf_augment_sparse_pairs (device pointers, KITTI code, resize / flip /
    crop parameters)."""
    _fields_ = [("src", c_p), ("dst", c_p), ("flow", c_p), ("valid", c_p), ("quantize", c_i), ("resize", c_i), ("scale_x", ctypes.c_double),
                ("scale_y", ctypes.c_double), ("Hr", c_i), ("Wr", c_i), ("flip_h", c_i), ("y0", c_i), ("x0", c_i)]


class MpfPhotoJitter(ctypes.Structure):
    """struct MpfPhotoJitter of include/mpiflow_hip.h: one ColorJitter parameter set of mpf_photometric_pairs."""
    _fields_ = [("n_ops", c_i), ("order", c_i * 4), ("brightness", c_f), ("contrast", c_f), ("saturation", c_f), ("hue_shift", c_i)]


class MpfPhotoSample(ctypes.Structure):
    """struct MpfPhotoSample of include/mpiflow_hip.h: one sample of mpf_photometric_pairs (device pointers, jitter, eraser rectangles)."""
    _fields_ = [("src", c_p), ("dst", c_p), ("src_out", c_p), ("dst_out", c_p), ("joint", c_i), ("jitter", MpfPhotoJitter * 2), ("n_rect", c_i),
                ("rect", (c_i * 4) * 2)]


CORR_MAX_LEVELS = 6     # MPF_CORR_MAX_LEVELS


class MpfCorrArgs(ctypes.Structure):
    """struct MpfCorrArgs of include/mpiflow_hip.h: RAFT's on-demand correlation lookup and its gradient (device pointers, channel-last maps)."""
    _fields_ = [("fmap1", c_p), ("f2", c_p * CORR_MAX_LEVELS), ("coords", c_p), ("out", c_p), ("grad_fmap1", c_p), ("grad_f2", c_p * CORR_MAX_LEVELS),
                ("B", c_i), ("C", c_i), ("H", c_i), ("W", c_i), ("Hl", c_i * CORR_MAX_LEVELS), ("Wl", c_i * CORR_MAX_LEVELS),
                ("radius", c_i), ("levels", c_i), ("scale", c_f), ("plain", c_i)]


class MpfCorrVolumeArgs(ctypes.Structure):
    """struct MpfCorrVolumeArgs of include/mpiflow_hip.h: RAFT's all-pairs correlation block: pyramid, lookup and both gradients (device pointers)."""
    _fields_ = [("level", c_p * CORR_MAX_LEVELS), ("coords", c_p), ("out", c_p), ("B", c_i), ("H", c_i), ("W", c_i),
                ("Hl", c_i * CORR_MAX_LEVELS), ("Wl", c_i * CORR_MAX_LEVELS), ("radius", c_i), ("levels", c_i), ("norm", c_f)]


class MpfUpsampleArgs(ctypes.Structure):
    """struct MpfUpsampleArgs of include/mpiflow_hip.h: RAFT's convex upsampling and its loss term, forward and gradient (device pointers)."""
    _fields_ = [("flow", c_p), ("mask", c_p), ("out", c_p), ("flow_gt", c_p), ("valid", c_p), ("g", c_p), ("term", c_p), ("metrics", c_p),
                ("grad_flow", c_p), ("grad_mask", c_p), ("workspace", c_p), ("workspace_bytes", c_sz),
                ("N", c_i), ("H", c_i), ("W", c_i), ("max_flow", c_f)]


GRU_MAX_TERMS = 3       # MPF_GRU_MAX_TERMS


class MpfGruTerm(ctypes.Structure):
    """struct MpfGruTerm of include/mpiflow_hip.h: the channel slice [offset, offset + C) of a [B,channels,H,W] tensor (device pointer)."""
    _fields_ = [("p", c_p), ("channels", c_i), ("offset", c_i)]


class MpfGruArgs(ctypes.Structure):
    """struct MpfGruArgs of include/mpiflow_hip.h: the pointwise work of RAFT's convolutional GRU, forward and gradient (device pointers)."""
    _fields_ = [("z", MpfGruTerm * GRU_MAX_TERMS), ("r", MpfGruTerm * GRU_MAX_TERMS), ("q", MpfGruTerm * GRU_MAX_TERMS),
                ("dz", MpfGruTerm * 2), ("dr", MpfGruTerm * 2), ("dq", MpfGruTerm * 2), ("h", c_p), ("g", c_p), ("out", c_p), ("dh", c_p),
                ("nz", c_i), ("nr", c_i), ("nq", c_i), ("accumulate", c_i), ("B", c_i), ("C", c_i), ("H", c_i), ("W", c_i)]


NORM_NONE, NORM_INSTANCE, NORM_BATCH_TRAIN, NORM_BATCH_EVAL, NORM_GROUP = range(5)      # MPF_NORM_*
NORM_MAX_CHUNKS = 1024  # MPF_NORM_MAX_CHUNKS


class MpfNormTerm(ctypes.Structure):
    """struct MpfNormTerm of include/mpiflow_hip.h: one activation with its norm mode, statistics and gradient buffers (device pointers)."""
    _fields_ = [("x", c_p), ("weight", c_p), ("bias", c_p), ("running_mean", c_p), ("running_var", c_p), ("partials", c_p), ("mean", c_p),
                ("rstd", c_p), ("var", c_p), ("grad_partials", c_p), ("dx", c_p), ("dweight", c_p), ("dbias", c_p), ("mode", c_i), ("groups", c_i)]


class MpfNormArgs(ctypes.Structure):
    """struct MpfNormArgs of include/mpiflow_hip.h: the norm / ReLU / shortcut / ReLU chain of RAFT's encoders, forward and gradient."""
    _fields_ = [("y", MpfNormTerm), ("r", MpfNormTerm), ("res", c_p), ("out", c_p), ("g", c_p), ("dres", c_p), ("accumulate", c_i),
                ("chunks", c_i), ("N", c_i), ("C", c_i), ("H", c_i), ("W", c_i)]


class MpfRaftGlueArgs(ctypes.Structure):
    """struct MpfRaftGlueArgs of include/mpiflow_hip.h: the glue of RAFT.forward: image scaling, context split, 8x bilinear upsampling."""
    _fields_ = [("image1", c_p), ("image2", c_p), ("pair", c_p), ("cnet", c_p), ("net", c_p), ("inp", c_p), ("g_net", c_p), ("g_inp", c_p),
                ("grad_cnet", c_p), ("flow", c_p), ("flow_up", c_p), ("g_up", c_p), ("grad_flow", c_p),
                ("N", c_i), ("H", c_i), ("W", c_i), ("hdim", c_i), ("cdim", c_i)]


class MpfRaftEvalArgs(ctypes.Structure):
    """struct MpfRaftEvalArgs of include/mpiflow_hip.h: RAFT evaluation on frames of any size: padded image batch, cropped upsampling, metrics."""
    _fields_ = [("image1", c_p), ("image2", c_p), ("pair", c_p), ("flow", c_p), ("mask", c_p), ("flow_up", c_p), ("flow_pr", c_p), ("flow_gt", c_p),
                ("valid", c_p), ("metrics", c_p), ("workspace", c_p), ("workspace_bytes", c_sz),
                ("N", c_i), ("H", c_i), ("W", c_i), ("pad_left", c_i), ("pad_right", c_i), ("pad_top", c_i), ("pad_bottom", c_i)]


class MpfWarmStartArgs(ctypes.Structure):
    """struct MpfWarmStartArgs of include/mpiflow_hip.h: RAFT's warm start, forward_interpolate as an exact nearest-source search."""
    _fields_ = [("flow", c_p), ("out", c_p), ("workspace", c_p), ("workspace_bytes", c_sz), ("N", c_i), ("h", c_i), ("w", c_i)]


class MpfFlowVizArgs(ctypes.Structure):
    """struct MpfFlowVizArgs of include/mpiflow_hip.h: RAFT's outputs: the colour-coded flow (under the frame) and KITTI's 16-bit code."""
    _fields_ = [("flow", c_p), ("image", c_p), ("valid", c_p), ("out", c_p), ("workspace", c_p), ("workspace_bytes", c_sz),
                ("N", c_i), ("H", c_i), ("W", c_i), ("clip", c_i), ("clip_flow", c_f), ("convert_to_bgr", c_i)]


class MpfMeshVertexArgs(ctypes.Structure):
    """struct MpfMeshVertexArgs of include/mpiflow_hip.h: the warp-back renderer's vertex stage (RGB-D -> NDC vertices and attributes)."""
    _fields_ = [("rgbd", c_p), ("cam_int", c_p), ("cam_ext", c_p), ("verts_ndc", c_p), ("attrs", c_p), ("B", c_i), ("h", c_i), ("w", c_i)]


class MpfMeshRasterArgs(ctypes.Structure):
    """struct MpfMeshRasterArgs of include/mpiflow_hip.h: the warp-back renderer's rasteriser of a regular grid mesh with implicit faces."""
    _fields_ = [("verts_ndc", c_p), ("attrs", c_p), ("pix_to_face", c_p), ("zbuf", c_p), ("bary", c_p), ("out", c_p), ("workspace", c_p),
                ("workspace_bytes", c_sz), ("B", c_i), ("h", c_i), ("w", c_i), ("C", c_i), ("blur_radius", c_f), ("passes", c_i)]


MESH_MAX_ATTRS = 8              # MPF_MESH_MAX_ATTRS
MESH_PASS_ALL, MESH_PASS_Z, MESH_PASS_RESOLVE = 0, 1, 2    # MPF_MESH_PASS_*
MESH_MAX_BHW = 1 << 28          # MPF_MESH_MAX_BHW

CANNY_MAX_RADIUS = 16           # MPF_CANNY_MAX_RADIUS
CANNY_MAX_BHW = 1 << 28         # MPF_CANNY_MAX_BHW
CANNY_LDS_WORDS = 6144          # MPF_CANNY_LDS_WORDS
CANNY_PASS_ALL, CANNY_PASS_SMOOTH, CANNY_PASS_CLASSIFY, CANNY_PASS_HYSTERESIS = 0, 1, 2, 3    # MPF_CANNY_PASS_*


class MpfCannyArgs(ctypes.Structure):
    """struct MpfCannyArgs of include/mpiflow_hip.h: warp-back stage 2's masked Canny (smoothing, classes, hysteresis), batched."""
    _fields_ = [("gray", c_p), ("mask", c_p), ("out", c_p), ("workspace", c_p), ("workspace_bytes", c_sz), ("B", c_i), ("h", c_i), ("w", c_i),
                ("radius", c_i), ("weights", c_f * (2 * CANNY_MAX_RADIUS + 1)), ("low_threshold", c_f), ("high_threshold", c_f), ("passes", c_i)]


class MpfStage2Args(ctypes.Structure):
    """struct MpfStage2Args of include/mpiflow_hip.h: the pointwise chain of warp-back stage 2's inpaint around the three generators."""
    _fields_ = [("image", c_p), ("disp", c_p), ("mask", c_p), ("edge", c_p), ("edge_inpaint", c_p), ("image_inpaint", c_p), ("disp_inpaint", c_p),
                ("gray", c_p), ("mask_hole", c_p), ("edge_input", c_p), ("image_input", c_p), ("disp_input", c_p), ("image_merged", c_p),
                ("disp_merged", c_p), ("B", c_i), ("h", c_i), ("w", c_i)]


BILATERAL_F32, BILATERAL_F64, BILATERAL_U8 = 0, 1, 2    # MPF_BILATERAL_F32 / _F64 / _U8
BILATERAL_MAX_WINDOW = 9        # MPF_BILATERAL_MAX_WINDOW
BILATERAL_MAX_ITER = 8          # MPF_BILATERAL_MAX_ITER
BILATERAL_MAX_BHW = 1 << 28     # MPF_BILATERAL_MAX_BHW


class MpfBilateralArgs(ctypes.Structure):
    """struct MpfBilateralArgs of include/mpiflow_hip.h: the sparse bilateral filter (a 0/1-weighted median around discontinuities), batched."""
    _fields_ = [("depth", c_p), ("mask", c_p), ("out", c_p), ("workspace", c_p), ("workspace_bytes", c_sz), ("dtype", c_i), ("B", c_i), ("h", c_i),
                ("w", c_i), ("mask_shared", c_i), ("num_iter", c_i), ("filter_size", c_i * BILATERAL_MAX_ITER), ("depth_threshold", ctypes.c_double)]


PXPY_F32, PXPY_I64 = 0, 1       # MPF_PXPY_F32 / _I64
SAMPLE_PDF_MAX_S = 128          # MPF_SAMPLE_PDF_MAX_S
SAMPLE_PDF_MAX_SAMPLES = 128    # MPF_SAMPLE_PDF_MAX_SAMPLES


class MpfGatherPxpyArgs(ctypes.Structure):
    """struct MpfGatherPxpyArgs of include/mpiflow_hip.h: gather_pixel_by_pxpy and its scatter-add adjoint."""
    _fields_ = [("img", c_p), ("pxpy", c_p), ("out", c_p), ("grad_out", c_p), ("grad_img", c_p), ("pxpy_dtype", c_i), ("B", c_i), ("C", c_i), ("H", c_i),
                ("W", c_i), ("N", c_i)]


class MpfSamplePdfArgs(ctypes.Structure):
    """struct MpfSamplePdfArgs of include/mpiflow_hip.h: sample_pdf with the draws handed in."""
    _fields_ = [("values", c_p), ("weights", c_p), ("u", c_p), ("out", c_p), ("values_batch_stride", ctypes.c_longlong),
                ("values_row_stride", ctypes.c_longlong), ("B", c_i), ("N", c_i), ("S", c_i), ("n_samples", c_i)]


class MpfDispConsistencyArgs(ctypes.Structure):
    """struct MpfDispConsistencyArgs of include/mpiflow_hip.h: disparity_consistency_src_to_tgt, forward and backward."""
    _fields_ = [("K_src_inv", c_p), ("G_tgt_src", c_p), ("K_tgt", c_p), ("disparity_src", c_p), ("disparity_tgt", c_p), ("loss", c_p), ("grad_loss", c_p),
                ("grad_disparity_src", c_p), ("grad_disparity_tgt", c_p), ("workspace", c_p), ("workspace_bytes", c_sz), ("B", c_i), ("H", c_i), ("W", c_i)]


FLOW_WARP_WARP, FLOW_WARP_RIFE = 0, 1       # MPF_FLOW_WARP_WARP / _RIFE
FLOW_WARP_CHUNK = 64                        # MPF_FLOW_WARP_CHUNK


class MpfFlowWarpArgs(ctypes.Structure):
    """struct MpfFlowWarpArgs of include/mpiflow_hip.h: the backward warps by a flow field (warp, warp_rife), forward and adjoint."""
    _fields_ = [("x", c_p), ("flow", c_p), ("lin_w", c_p), ("lin_h", c_p), ("out", c_p), ("mask", c_p), ("grad_out", c_p), ("grad_x", c_p),
                ("grad_flow", c_p), ("workspace", c_p), ("workspace_bytes", c_sz), ("mode", c_i), ("B", c_i), ("C", c_i), ("H", c_i), ("W", c_i),
                ("whole", c_i)]


PAN_C = 8                                   # MPF_PAN_C
PAN_PLANES_PER_GROUP = 4                    # MPF_PAN_PLANES_PER_GROUP


class MpfPanArgs(ctypes.Structure):
    """struct MpfPanArgs of include/mpiflow_hip.h: the first residual block of the plane-adjustment network over the S plane-images, pooled."""
    _fields_ = [("rgb_low", c_p), ("disp_low", c_p), ("plane_disp", c_p), ("w1", c_p), ("b1", c_p), ("bn_scale", c_p), ("bn_shift", c_p), ("w2", c_p),
                ("b2", c_p), ("w3", c_p), ("b3", c_p), ("out", c_p), ("workspace", c_p), ("workspace_bytes", c_sz), ("B", c_i), ("S", c_i), ("h", c_i),
                ("w", c_i)]


WARM_MAX_HW = 65536             # MPF_WARM_MAX_HW
WARM_MAX_NHW = 1 << 22          # MPF_WARM_MAX_NHW

OPT_CHUNK = 4096                # MPF_OPT_CHUNK
OPT_TENSORS_PER_LAUNCH = 64     # MPF_OPT_TENSORS_PER_LAUNCH
OPT_WORKSPACE_TAIL = 16         # MPF_OPT_WORKSPACE_TAIL
OPT_MAX_CHUNKS = 1 << 23        # MPF_OPT_MAX_CHUNKS


class MpfOptTensor(ctypes.Structure):
    """struct MpfOptTensor of include/mpiflow_hip.h: one parameter with its AdamW moments and its gradient (device pointers; grad may be NULL)."""
    _fields_ = [("param", c_p), ("exp_avg", c_p), ("exp_avg_sq", c_p), ("grad", c_p), ("numel", c_i64)]


class MpfAdamWArgs(ctypes.Structure):
    """struct MpfAdamWArgs of include/mpiflow_hip.h: the clipped AdamW step over a host table of MpfOptTensor records."""
    _fields_ = [("tensors", ctypes.POINTER(MpfOptTensor)), ("count", c_i), ("zero_grad", c_i), ("norm_ready", c_i),
                ("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("weight_decay", ctypes.c_double), ("bias_correction1", ctypes.c_double), ("bias_correction2_sqrt", ctypes.c_double),
                ("max_norm", ctypes.c_double), ("total_norm", c_p), ("workspace", c_p), ("workspace_bytes", c_sz)]


MAX_VIEWS = 16          # MPF_MAX_VIEWS
SUPPORT_CELL_W, SUPPORT_CELL_H = 32, 8      # MPF_SUPPORT_CELL_W / _H

# name -> (restype, argtypes); must list every symbol include/mpiflow_hip.h declares (tests/test_capi.py checks)
SIGNATURES = {
    "mpf_version": (c_i, []),
    "mpf_last_error": (ctypes.c_char_p, []),
    "mpf_device_info": (c_i, [c_i, ctypes.POINTER(c_i), ctypes.POINTER(c_sz), ctypes.c_char_p, c_sz]),
    "mpf_stream_create_cu_subset": (c_i, [c_i, c_i, ctypes.POINTER(c_p)]),
    "mpf_stream_destroy": (c_i, [c_p]),
    "mpf_src_blend_flow": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "mpf_build_mask_quads": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p]),
    "mpf_warp_composite": (c_i, [c_p, c_i, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "mpf_warp_composite_split": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "mpf_src_flow": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p, c_p]),
    "mpf_src_flow_hard": (c_i, [c_p, c_i64, c_p, c_i, c_i, c_i, c_i, c_f, c_p, c_p]),
    "mpf_warp_composite_views": (c_i, [c_p, c_i, ctypes.POINTER(MpfWarpView), c_i, c_i, c_i, c_i, c_p]),
    "mpf_warp_views_and_blend_next": (c_i, [c_p, ctypes.POINTER(MpfWarpView), c_i, c_p, c_p, c_p, c_i, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p]),
    "mpf_warp_views_blend_next_merge_prev": (c_i, [c_p, ctypes.POINTER(MpfWarpView), c_i, c_p, c_p, c_p, c_i, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i,
                                                  ctypes.POINTER(MpfMergeArgs), c_p]),
    "mpf_src_blend_flow_support": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_uint32, c_p]),
    "mpf_warp_composite_views_support": (c_i, [c_p, c_i, ctypes.POINTER(MpfWarpView), ctypes.POINTER(MpfViewSupport), c_i, c_i, c_i, c_i, c_p]),
    "mpf_warp_views_blend_next_merge_prev_support": (c_i, [c_p, ctypes.POINTER(MpfWarpView), ctypes.POINTER(MpfViewSupport), c_i, c_p, c_p, c_p, c_i, c_f, c_p, c_p, c_p,
                                                          c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_uint32, c_i, c_i, c_i, ctypes.POINTER(MpfMergeArgs), c_p]),
    "mpf_support_dead_tiles": (c_i, [ctypes.POINTER(MpfWarpView), ctypes.POINTER(MpfViewSupport), c_i, c_i, c_i, c_i, c_p, c_p]),
    "mpf_merge": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_i, c_i, c_p, c_p, c_p, c_p]),
    "mpf_merge_ex": (c_i, [ctypes.POINTER(MpfMergeArgs), c_i, c_i, c_p]),
    "mpf_merge_depth_ordered": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_i, c_i, c_p, c_p, c_p]),
    "mpf_fill_holes_workspace": (c_sz, [c_i, c_i]),
    "mpf_fill_holes": (c_i, [c_p, c_p, c_i, c_i, c_p, c_sz, c_p]),
    "mpf_prepare_inputs": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    "mpf_inpaint_host": (c_i, [c_p, c_p, c_i, c_i, c_i, ctypes.c_double, c_i, c_p]),
    "mpf_inpaint_ns_workspace": (c_sz, [c_i, c_i, c_i, ctypes.c_double]),
    "mpf_inpaint_ns": (c_i, [c_p, c_p, c_i, c_i, c_i, ctypes.c_double, c_p, c_p, c_sz, c_p]),
    "mpf_png_filter_up": (c_i, [c_p, c_i, c_i, c_p, c_p]),
    "mpf_pair_stats": (c_i, [c_p, c_p, c_i, c_i, c_p, c_p]),
    "mpf_stream_probe": (c_i, [c_p, c_p, ctypes.c_size_t, c_i, c_p]),
    "mpf_to_u8_bgr": (c_i, [c_p, c_i, c_i, c_p, c_p]),
    "mpf_augment_pairs": (c_i, [ctypes.POINTER(MpfAugmentSample), c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "mpf_augment_sparse_pairs": (c_i, [ctypes.POINTER(MpfSparseAugmentSample), c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "mpf_photometric_workspace": (c_sz, [c_i]),
    "mpf_photometric_pairs": (c_i, [ctypes.POINTER(MpfPhotoSample), c_i, c_i, c_i, c_p, c_sz, c_p]),
    "mpf_corr_lookup": (c_i, [ctypes.POINTER(MpfCorrArgs), c_p]),
    "mpf_corr_lookup_backward": (c_i, [ctypes.POINTER(MpfCorrArgs), c_p]),
    "mpf_corr_pyramid": (c_i, [ctypes.POINTER(MpfCorrVolumeArgs), c_p]),
    "mpf_corr_volume_lookup": (c_i, [ctypes.POINTER(MpfCorrVolumeArgs), c_p]),
    "mpf_corr_volume_lookup_backward": (c_i, [ctypes.POINTER(MpfCorrVolumeArgs), c_p]),
    "mpf_corr_pyramid_backward": (c_i, [ctypes.POINTER(MpfCorrVolumeArgs), c_p]),
    "mpf_upsample_workspace": (c_sz, [c_i, c_i, c_i, c_i]),
    "mpf_upsample_flow": (c_i, [ctypes.POINTER(MpfUpsampleArgs), c_p]),
    "mpf_upsample_flow_backward": (c_i, [ctypes.POINTER(MpfUpsampleArgs), c_p]),
    "mpf_flow_loss_term": (c_i, [ctypes.POINTER(MpfUpsampleArgs), c_p]),
    "mpf_flow_loss_term_backward": (c_i, [ctypes.POINTER(MpfUpsampleArgs), c_p]),
    "mpf_upflow8_loss_workspace": (c_sz, [c_i, c_i, c_i, c_i]),
    "mpf_upflow8_loss_term": (c_i, [ctypes.POINTER(MpfUpsampleArgs), c_p]),
    "mpf_upflow8_loss_term_backward": (c_i, [ctypes.POINTER(MpfUpsampleArgs), c_p]),
    "mpf_gru_reset": (c_i, [ctypes.POINTER(MpfGruArgs), c_p]),
    "mpf_gru_update": (c_i, [ctypes.POINTER(MpfGruArgs), c_p]),
    "mpf_gru_update_backward": (c_i, [ctypes.POINTER(MpfGruArgs), c_p]),
    "mpf_gru_reset_backward": (c_i, [ctypes.POINTER(MpfGruArgs), c_p]),
    "mpf_norm_stats": (c_i, [ctypes.POINTER(MpfNormArgs), c_p]),
    "mpf_norm_act": (c_i, [ctypes.POINTER(MpfNormArgs), c_p]),
    "mpf_norm_act_backward_reduce": (c_i, [ctypes.POINTER(MpfNormArgs), c_p]),
    "mpf_norm_act_backward": (c_i, [ctypes.POINTER(MpfNormArgs), c_p]),
    "mpf_raft_images": (c_i, [ctypes.POINTER(MpfRaftGlueArgs), c_p]),
    "mpf_context_split": (c_i, [ctypes.POINTER(MpfRaftGlueArgs), c_p]),
    "mpf_context_split_backward": (c_i, [ctypes.POINTER(MpfRaftGlueArgs), c_p]),
    "mpf_upflow8": (c_i, [ctypes.POINTER(MpfRaftGlueArgs), c_p]),
    "mpf_upflow8_backward": (c_i, [ctypes.POINTER(MpfRaftGlueArgs), c_p]),
    "mpf_raft_images_padded": (c_i, [ctypes.POINTER(MpfRaftEvalArgs), c_p]),
    "mpf_upsample_flow_crop": (c_i, [ctypes.POINTER(MpfRaftEvalArgs), c_p]),
    "mpf_upflow8_crop": (c_i, [ctypes.POINTER(MpfRaftEvalArgs), c_p]),
    "mpf_flow_metrics_workspace": (c_sz, [c_i, c_i, c_i]),
    "mpf_flow_metrics": (c_i, [ctypes.POINTER(MpfRaftEvalArgs), c_p]),
    "mpf_forward_interpolate_workspace": (c_sz, [c_i, c_i, c_i]),
    "mpf_forward_interpolate": (c_i, [ctypes.POINTER(MpfWarmStartArgs), c_p]),
    "mpf_flow_to_image_workspace": (c_sz, [c_i, c_i, c_i]),
    "mpf_flow_to_image": (c_i, [ctypes.POINTER(MpfFlowVizArgs), c_p]),
    "mpf_flow_encode_kitti": (c_i, [ctypes.POINTER(MpfFlowVizArgs), c_p]),
    "mpf_rgbd_mesh_vertices": (c_i, [ctypes.POINTER(MpfMeshVertexArgs), c_p]),
    "mpf_rasterize_grid_workspace": (c_sz, [c_i, c_i, c_i]),
    "mpf_rasterize_grid": (c_i, [ctypes.POINTER(MpfMeshRasterArgs), c_p]),
    "mpf_canny_workspace": (c_sz, [c_i, c_i, c_i]),
    "mpf_canny": (c_i, [ctypes.POINTER(MpfCannyArgs), c_p]),
    "mpf_stage2_gray_hole": (c_i, [ctypes.POINTER(MpfStage2Args), c_p]),
    "mpf_stage2_edge_input": (c_i, [ctypes.POINTER(MpfStage2Args), c_p]),
    "mpf_stage2_gen_inputs": (c_i, [ctypes.POINTER(MpfStage2Args), c_p]),
    "mpf_stage2_merge": (c_i, [ctypes.POINTER(MpfStage2Args), c_p]),
    "mpf_sparse_bilateral_workspace": (c_sz, [c_i, c_i, c_i, c_i]),
    "mpf_sparse_bilateral_rank": (c_i, [c_i]),
    "mpf_sparse_bilateral": (c_i, [ctypes.POINTER(MpfBilateralArgs), c_p]),
    "mpf_gather_pxpy": (c_i, [ctypes.POINTER(MpfGatherPxpyArgs), c_p]),
    "mpf_gather_pxpy_bwd": (c_i, [ctypes.POINTER(MpfGatherPxpyArgs), c_p]),
    "mpf_sample_pdf": (c_i, [ctypes.POINTER(MpfSamplePdfArgs), c_p]),
    "mpf_disp_consistency_workspace": (c_sz, [c_i, c_i, c_i]),
    "mpf_disp_consistency": (c_i, [ctypes.POINTER(MpfDispConsistencyArgs), c_p]),
    "mpf_disp_consistency_bwd": (c_i, [ctypes.POINTER(MpfDispConsistencyArgs), c_p]),
    "mpf_flow_warp_workspace": (c_sz, [c_i, c_i, c_i, c_i, c_i]),
    "mpf_flow_warp": (c_i, [ctypes.POINTER(MpfFlowWarpArgs), c_p]),
    "mpf_flow_warp_bwd": (c_i, [ctypes.POINTER(MpfFlowWarpArgs), c_p]),
    "mpf_pan_block1_workspace": (c_sz, [c_i, c_i, c_i]),
    "mpf_pan_block1": (c_i, [ctypes.POINTER(MpfPanArgs), c_p]),
    "mpf_adamw_workspace": (c_sz, [ctypes.POINTER(MpfOptTensor), c_i]),
    "mpf_grad_norm": (c_i, [ctypes.POINTER(MpfAdamWArgs), c_p]),
    "mpf_adamw_clipped": (c_i, [ctypes.POINTER(MpfAdamWArgs), c_p]),
    "mpf_src_xyz": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p]),
    "mpf_transform_xyz": (c_i, [c_p, c_p, c_i, c_i64, c_p, c_p]),
    "mpf_homography_sample": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    "mpf_homography_flow": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p]),
    "mpf_volume_render": (c_i, [c_p, c_p, c_p, c_i, c_i64, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_i, c_p]),
    "mpf_volume_render_bwd": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i64, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "mpf_homography_sample_bwd": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p]),
    "mpf_warp_composite_bwd": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "mpf_volume_render_bwd_xyz": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i64, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "mpf_warp_composite_bwd_disp": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p]),
    "mpf_src_xyz_bwd": (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_i, c_p, c_p]),
    "mpf_plane_flow_bwd": (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_i, c_p, c_p]),
    "mpf_weighted_sum": (c_i, [c_p, c_p, c_i, c_i, c_i64, c_p, c_p]),
    "mpf_alpha_composite": (c_i, [c_p, c_p, c_i, c_i, c_i64, c_p, c_p, c_p, c_p]),
    "mpf_disp_to_depth": (c_i, [c_p, c_i64, c_p, c_p]),
    "mpf_backproject_project": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p]),
    "mpf_backproject": (c_i, [c_p, c_p, c_i, c_i, c_p, c_p]),
    "mpf_project3d": (c_i, [c_p, c_p, c_f, c_i, c_i, c_p, c_p, c_p]),
    "mpf_select_truncate": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "mpf_moving_object_project": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "mpf_forward_warp_workspace": (c_sz, [c_i, c_i]),
    "mpf_forward_warp": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_p, c_sz, c_p]),
    "mpf_warp_masks": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "mpf_moving_object_chain": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, ctypes.POINTER(MpfMovingObjectOut), c_p, c_sz, c_p]),
    "forward_warping": (None, [c_p, c_p, c_p, c_p, c_p, c_i, c_i]),
    "mpf_forward_warping_host": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i]),
    "mpf_tune": (c_i, [ctypes.c_char_p, c_i]),
    "mpf_is_witness_build": (c_i, []),
    "mpf_conv3x3_f16": (c_i, [ctypes.POINTER(MpfConvArgs), c_p]),
    "mpf_plane_masks": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_p), c_p]),
    "mpf_encoder_input": (c_i, [c_p, c_p, c_i, c_i, c_p, c_p]),
    "mpf_conv2d_f32": (c_i, [ctypes.POINTER(MpfConv2dArgs), c_p]),
    "mpf_maxpool3x3s2_f32": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p]),
    "mpf_pconv": (c_i, [ctypes.POINTER(MpfPConvArgs), c_p]),
    "mpf_pfmn_input": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_i, c_p]),
    "mpf_pencoder_input": (c_i, [c_p, c_p, c_i, c_i, c_p, c_i, c_p]),
    "mpf_pbilinear2x": (c_i, [c_p, c_i, c_i, c_i, c_i, c_p, c_i, c_p]),
    "mpf_pper_plane": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_i, c_p]),
    "mpf_pplane_masks": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_p), c_i, c_p]),
    "mpf_pmaxpool3x3s2": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_p]),
}


class MpiFlowHipError(RuntimeError):
    pass


def _bind(path, missing_ok=False):
    """dlopen + set every signature of SIGNATURES; -> (library, names it lacks: only ever non-empty with missing_ok)"""
    lib = ctypes.CDLL(path)
    skipped = []
    for name, (res, args) in SIGNATURES.items():
        if missing_ok and not hasattr(lib, name):
            skipped.append(name)
            continue
        fn = getattr(lib, name)          # AttributeError here = header and library disagree
        fn.restype = res
        fn.argtypes = args
    return lib, skipped


def load_witness():
    """The witness build (libmpiflow_hip_witness.so), loaded once, NOT made the library the package's calls go through (see witness())."""
    global _witness
    if _witness is None:
        if not os.path.exists(WITNESS_PATH):
            raise MpiFlowHipError("libmpiflow_hip_witness.so not found at %s - `make -C mpiflow_amd/csrc` builds it beside the product library" % WITNESS_PATH)
        _witness = _bind(WITNESS_PATH)[0]
        assert _witness.mpf_is_witness_build() == 1
    return _witness


class witness:
    """`with _lib.witness() as lib:` - inside the block every call of the package goes through the WITNESS build, whose mpf_tune accepts the variant / ablation
    keys ("stage_b", "planar_lds", "fwarp_path", "ovl_depth", "ovl_xcd_a", "view_shift", "ovl_ablate").  Tests and tools only; not re-entrant, one thread."""

    def __enter__(self):
        global _lib
        self.prev = load()
        _lib = load_witness()
        return _lib

    def __exit__(self, *exc):
        global _lib
        _lib = self.prev
        return False


def select_witness():
    """Process-wide switch to the witness build (tools/ that time retired variants; bench.py --witness)."""
    global _lib
    _lib = load_witness()
    return _lib


def load():
    """Load the HIP library once.  Raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MpiFlowHipError(
            "libmpiflow_hip.so not found at %s - build it with `python __graft_entry__.py` or "
            "`make -C mpiflow_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    lib, skipped = _bind(LIB_PATH, missing_ok=bool(os.environ.get("MPIFLOW_HIP_LIB")))
    if skipped:                          # development hook only: say which calls will fail instead of failing late with an AttributeError
        import sys
        sys.stderr.write("mpiflow_amd: MPIFLOW_HIP_LIB=%s lacks %d symbol(s) of include/mpiflow_hip.h: %s\n" % (LIB_PATH, len(skipped), ", ".join(skipped)))
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().mpf_last_error()
        raise MpiFlowHipError("%s failed with code %d: %s" % (what or "libmpiflow_hip call", rc,
                                                              msg.decode() if msg else "?"))


def device_info(device=0):
    lib = load()
    cu, mem = c_i(0), c_sz(0)
    arch = ctypes.create_string_buffer(64)
    check(lib.mpf_device_info(device, ctypes.byref(cu), ctypes.byref(mem), arch, 64), "mpf_device_info")
    return dict(cu_count=cu.value, hbm_bytes=mem.value, arch=arch.value.decode())
