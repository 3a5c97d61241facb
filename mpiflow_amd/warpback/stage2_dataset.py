"""warpback/stage2_dataset.py of the reference: WarpBackStage2Dataset, the AdaMPI training samples - an RGB-D image warped to a random novel
view, the holes of that view inpainted by the three EdgeConnect generators and handed out as the source view - and warp_and_inpaint, the
same steps as a plain function for callers that already hold device tensors.

Everything between the render and the generators stays on the GPU and on the stream: get_edge is ops.canny_masked (the reference copies the
batch to the host and calls skimage's canny per image), and inpaint's torch glue is the four ops.stage2_* launches.  __getitem__,
preprocess_rgbd, get_rand_ext and rand_tensor are stage 1's own (same host-generator draw order).  `models=(edge, inpaint, disp)` is the
one constructor keyword the reference lacks: generators handed in, for callers without the checkpoint directory."""
import torch
from torch.utils.data.dataloader import default_collate

from .. import ops
from .networks import get_edge_connect
from .stage1_dataset import WarpBackStage1Dataset
from .utils import RGBDRenderer


def get_edge(image_gray, mask, workspace=None):
    """image_gray, mask [b,1,h,w] -> canny(image_gray, sigma=2, mask=mask) per image as float32 0 / 1 [b,1,h,w], on the device"""
    return ops.canny_masked(image_gray, mask, sigma=2.0, workspace=workspace)


def inpaint(image, disp, mask, models):
    """image [b,3,h,w], disp and mask [b,1,h,w] (mask: 1 where the render is valid), models = (edge, inpaint, disp) -> (image_merged, disp_merged,
    edge): the holes filled by the generators, the rest kept; edge is what get_edge found"""
    edge_model, inpaint_model, disp_model = models
    image, disp, mask = image.contiguous(), disp.contiguous(), mask.contiguous()
    image_gray, mask_hole = ops.stage2_gray_hole(image, mask)
    edge = get_edge(image_gray, mask)
    edge_inpaint = edge_model(ops.stage2_edge_input(image_gray, edge, mask_hole)).contiguous()
    image_input, disp_input = ops.stage2_gen_inputs(image, disp, mask_hole, edge_inpaint)
    image_inpaint = inpaint_model(image_input).contiguous()
    disp_inpaint = disp_model(disp_input).contiguous()
    image_merged, disp_merged = ops.stage2_merge(image, image_inpaint, disp, disp_inpaint, mask_hole)
    return image_merged, disp_merged, edge


def warp_and_inpaint(image, disp, cam_int, cam_ext, cam_ext_inv, models, renderer=None):
    """image [b,3,h,w], disp [b,1,h,w], cam_int [b,3,3], cam_ext and cam_ext_inv [b,3,4], float32 on the GPU; models = (edge, inpaint, disp)
    generators on that device -> collect_data's dict: the image rendered at cam_ext (warp_rgb, warp_disp), its holes inpainted (src_rgb,
    src_disp), the input as the target (tgt_rgb, tgt_disp), cam_int, and cam_ext_inv as cam_ext (from the source view back to the target)."""
    renderer = renderer or RGBDRenderer(image.device)
    rgbd = torch.cat([image, disp], dim=1)
    warp_image, warp_disp, warp_mask = renderer.render_mesh(renderer.construct_mesh(rgbd, cam_int), cam_int, cam_ext)
    with torch.no_grad():
        src_image, src_disp, _ = inpaint(warp_image, warp_disp, warp_mask, models)
    return {"src_rgb": src_image, "src_disp": src_disp, "tgt_rgb": image, "tgt_disp": disp, "warp_rgb": warp_image, "warp_disp": warp_disp,
            "cam_int": cam_int, "cam_ext": cam_ext_inv}


class WarpBackStage2Dataset(WarpBackStage1Dataset):
    def __init__(self, data_root, width=384, height=256, depth_dir_name="dpt_depth", device="cuda",
                 trans_range={"x": 0.2, "y": -1, "z": -1, "a": -1, "b": -1, "c": -1}, ec_weight_dir="warpback/ecweight", models=None,
                 disp_filter=None):
        super().__init__(data_root, width=width, height=height, depth_dir_name=depth_dir_name, device=device, trans_range=trans_range,
                         disp_filter=disp_filter)
        if models is None:
            models = get_edge_connect(ec_weight_dir)              # FileNotFoundError naming the three files it looked for
        self.edge_model, self.inpaint_model, self.disp_model = (m.to(self.device).eval() for m in models)

    def get_edge(self, image_gray, mask):
        return get_edge(image_gray, mask)

    def inpaint(self, image, disp, mask):
        return inpaint(image, disp, mask, (self.edge_model, self.inpaint_model, self.disp_model))[:2]

    def collect_data(self, batch):
        image, disp = default_collate(batch)
        image = image.to(self.device)
        disp = self.filter_disp(disp.to(self.device))
        b = image.shape[0]
        cam_int = self.K.repeat(b, 1, 1)
        cam_ext, cam_ext_inv = self.get_rand_ext(b)
        return warp_and_inpaint(image, disp, cam_int, cam_ext.to(self.device).contiguous(), cam_ext_inv.to(self.device).contiguous(),
                                (self.edge_model, self.inpaint_model, self.disp_model), self.renderer)
