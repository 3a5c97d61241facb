"""The reference's warpback/ without pytorch3d and without skimage.  Stage 1 makes the warp-back pairs AdaMPI's inpainting network is trained
on: an RGB-D image is lifted to a grid mesh, rendered at a random pose and rendered back; the mask that survives both renders marks what to
inpaint.  Stage 2 makes the AdaMPI training samples: the image rendered at a random pose, its holes inpainted by the three EdgeConnect
generators, handed out as the source view.

    utils            RGBDRenderer, the pose helpers, the two image readers                        (warpback/utils.py)
    stage1_dataset   WarpBackStage1Dataset, warp_back                                             (warpback/stage1_dataset.py)
    networks         EdgeGenerator, InpaintGenerator, ResnetBlock, get_edge_connect,              (warpback/networks.py)
                     fold_spectral_norm
    stage2_dataset   WarpBackStage2Dataset, warp_and_inpaint                                      (warpback/stage2_dataset.py)

The rasteriser is ops.rasterize_grid (mpf_mesh.hip), stage 2's edge detector ops.canny_masked (mpf_canny.hip) and its pointwise glue
ops.stage2_* (mpf_stage2.hip); INTEGRATION.md sections 16 and 17 state what they compute.  The generators' convolutions are torch's.  Not
here: the EdgeConnect checkpoints (get_edge_connect loads them from a directory the caller names), training the generators, gradients
through the renderer or the edge detector, faces_per_pixel > 1, canny's use_quantiles and its other border modes."""
from .networks import EdgeGenerator, InpaintGenerator, ResnetBlock, fold_spectral_norm, get_edge_connect  # noqa: F401
from .stage1_dataset import WarpBackStage1Dataset, warp_back  # noqa: F401
from .stage2_dataset import WarpBackStage2Dataset, warp_and_inpaint  # noqa: F401
from .utils import RGBDRenderer  # noqa: F401
