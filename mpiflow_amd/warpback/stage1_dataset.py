"""warpback/stage1_dataset.py of the reference: WarpBackStage1Dataset with the reference's constructor, rand_tensor, get_rand_ext and
collect_data, and warp_back, the two renders as a plain function for callers that already hold device tensors.

rand_tensor and get_rand_ext draw from torch's HOST generator in the reference's order (rand, then randn_like, per component x, y, z, a, b,
c; a negative range draws nothing), so a seeded run meets the reference's poses."""
import glob
import math
import os

import torch
import torch.nn.functional as F
from torch.utils.data.dataloader import default_collate
from torch.utils.data.dataset import Dataset

from .. import ops
from .utils import RGBDRenderer, disparity_to_tensor, image_to_tensor, transformation_from_parameters


def warp_back(image, disp, cam_int, cam_ext, cam_ext_inv, renderer=None):
    """image [b,3,h,w], disp [b,1,h,w], cam_int [b,3,3], cam_ext and cam_ext_inv [b,3,4], float32 on the GPU -> collect_data's dict: the image
    rendered at cam_ext (warp_rgb, warp_disp), that render lifted again and rendered back at cam_ext_inv (warp_back_rgb, warp_back_disp), and
    mask, the visibility that survives both renders."""
    renderer = renderer or RGBDRenderer(image.device)
    rgbd = torch.cat([image, disp], dim=1)
    warp_image, warp_disp, _ = renderer.render_mesh(renderer.construct_mesh(rgbd, cam_int), cam_int, cam_ext)
    warp_rgbd = torch.cat([warp_image, warp_disp], dim=1)
    warp_back_image, warp_back_disp, mask = renderer.render_mesh(renderer.construct_mesh(warp_rgbd, cam_int), cam_int, cam_ext_inv)
    return {"rgb": image, "disp": disp, "mask": mask, "warp_rgb": warp_image, "warp_disp": warp_disp,
            "warp_back_rgb": warp_back_image, "warp_back_disp": warp_back_disp}


class WarpBackStage1Dataset(Dataset):
    def __init__(self, data_root, width=384, height=256, depth_dir_name="dpt_depth", device="cuda",
                 trans_range={"x": 0.2, "y": -1, "z": -1, "a": -1, "b": -1, "c": -1}, disp_filter=None):
        self.data_root = data_root
        self.disp_filter = disp_filter         # the one keyword the reference lacks: windows of ops.sparse_bilateral_filter, None = off
        self.depth_dir_name = depth_dir_name
        self.renderer = RGBDRenderer(device)
        self.width = width
        self.height = height
        self.device = device
        self.trans_range = trans_range
        self.image_path_list = glob.glob(os.path.join(self.data_root, "*.jpg"))
        self.image_path_list += glob.glob(os.path.join(self.data_root, "*.png"))
        self.K = torch.tensor([[0.58, 0, 0.5], [0, 0.58, 0.5], [0, 0, 1]]).to(device)

    def __len__(self):
        return len(self.image_path_list)

    def __getitem__(self, idx):
        image_path = self.image_path_list[idx]
        image_name = os.path.splitext(os.path.basename(image_path))[0]
        disp_path = os.path.join(self.data_root, self.depth_dir_name, "%s.png" % image_name)
        image = image_to_tensor(image_path, unsqueeze=False)
        disp = disparity_to_tensor(disp_path, unsqueeze=False)
        return self.preprocess_rgbd(image, disp)

    def preprocess_rgbd(self, image, disp):
        image = F.interpolate(image.unsqueeze(0), (self.height, self.width), mode="bilinear").squeeze(0)
        disp = F.interpolate(disp.unsqueeze(0), (self.height, self.width), mode="bilinear").squeeze(0)
        return image, disp

    def get_rand_ext(self, bs):
        """-> (cam_ext, cam_ext_inv), [bs,3,4] each, on the host"""
        r = self.trans_range
        cix, ciy, ciz = (self.rand_tensor(r[k], bs) for k in "xyz")
        aix, aiy, aiz = (self.rand_tensor(math.pi / r[k], bs) for k in "abc")
        axisangle = torch.cat([aix, aiy, aiz], dim=-1)
        translation = torch.cat([cix, ciy, ciz], dim=-1)
        cam_ext = transformation_from_parameters(axisangle, translation)
        cam_ext_inv = torch.inverse(cam_ext)
        return cam_ext[:, :-1], cam_ext_inv[:, :-1]

    def rand_tensor(self, r, l):
        """[l,1,1], each element in [-r, -r/2] or [r/2, r]; r < 0: zeros, and nothing is drawn"""
        if r < 0:
            return torch.zeros((l, 1, 1))
        rand = torch.rand((l, 1, 1))
        sign = 2 * (torch.randn_like(rand) > 0).float() - 1
        return sign * (r / 2 + r / 2 * rand)

    def filter_disp(self, disp):
        """preprocess_rgbd's note, "filter the depth map to reduce artifacts around depth discontinuities": the sparse bilateral filter on
        the uploaded [b,1,h,w] disparity, once, where disp_filter asks for it"""
        return disp if self.disp_filter is None else ops.sparse_bilateral_filter(disp.contiguous(), self.disp_filter)

    def collect_data(self, batch):
        image, disp = default_collate(batch)
        image = image.to(self.device)
        disp = self.filter_disp(disp.to(self.device))
        b = image.shape[0]
        cam_int = self.K.repeat(b, 1, 1)
        cam_ext, cam_ext_inv = self.get_rand_ext(b)
        return warp_back(image, disp, cam_int, cam_ext.to(self.device).contiguous(), cam_ext_inv.to(self.device).contiguous(), self.renderer)
