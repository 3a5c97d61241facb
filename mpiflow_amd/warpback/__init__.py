"""The reference's warpback/ stage 1 (the warp-back pairs AdaMPI's inpainting network is trained on) without pytorch3d: an RGB-D image is
lifted to a grid mesh, rendered at a random pose and rendered back; the mask that survives both renders marks what to inpaint.

    utils            RGBDRenderer, the pose helpers, the two image readers      (warpback/utils.py)
    stage1_dataset   WarpBackStage1Dataset, warp_back                           (warpback/stage1_dataset.py)

The rasteriser is ops.rasterize_grid (mpf_mesh.hip); INTEGRATION.md section 16 states what it computes.  Not here: stage 2 (the EdgeConnect
networks, skimage's Canny), gradients through the renderer, faces_per_pixel > 1."""
from .stage1_dataset import WarpBackStage1Dataset, warp_back  # noqa: F401
from .utils import RGBDRenderer  # noqa: F401
