"""warpback/utils.py of the reference: RGBDRenderer with the same methods and signatures, on ops.rgbd_mesh_vertices and ops.rasterize_grid
instead of pytorch3d; the pose helpers and the image readers are the package's own (host_math, utils/utils.py).

render_mesh on a mesh_dict that construct_mesh made takes the fused path: one vertex launch from the RGB-D image the dict remembers, then
the rasteriser.  On a hand-made dict (vertice, attributes, size) it transforms in torch, as the reference does, and calls the rasteriser.
Either way the faces are the regular grid's (get_faces): mesh_dict["faces"] is built lazily, for callers that read it, and never used here.
A construct_mesh dict whose vertice, faces or attributes the caller has assigned, or that is rendered with another cam_int tensor than it was
made with, takes the torch path and reads the dict.  The dict REMEMBERS rgbd, it does not copy it: editing rgbd in place between
construct_mesh and render_mesh changes the render (the reference's dict holds tensors computed at construct_mesh time).
No gradients; faces_per_pixel is 1."""
import torch

from .. import ops
from .._lib import MpiFlowHipError
from ..host_math import get_translation_matrix, rot_from_axisangle, transformation_from_parameters  # noqa: F401
from ..utils.utils import disparity_to_tensor, image_to_tensor  # noqa: F401


class _MeshDict(dict):
    """construct_mesh's result: the reference's keys, "faces" built on first use ([b,nface,3] int64 is 48 bytes per pixel nobody needs)"""

    def __init__(self, renderer, rgbd, cam_int):
        b, _, h, w = rgbd.shape
        super().__init__(size=[h, w])
        self._renderer, self._rgbd, self._cam_int, self._b, self._by_hand = renderer, rgbd, cam_int, b, False

    def __missing__(self, key):
        r, (h, w) = self._renderer, self["size"]
        if key == "faces":
            val = r.get_faces(h, w).repeat(self._b, 1, 1).long()
        elif key == "vertice":
            val = r._unproject(self._rgbd, self._cam_int)
        elif key == "attributes":
            x = self._rgbd.permute(0, 2, 3, 1)
            val = torch.cat([x[..., :-1].reshape(self._b, h * w, 3), r.get_visible_mask(x[..., -1:]).reshape(self._b, h * w, 1)], dim=-1)
        else:
            raise KeyError(key)
        dict.__setitem__(self, key, val)
        return val

    _LAZY = ("vertice", "faces", "attributes")

    def __setitem__(self, key, val):
        if key in self._LAZY:
            self._by_hand = True                 # the caller's own tensor: render_mesh must read the dict, not the remembered image
        dict.__setitem__(self, key, val)

    def keys(self):
        return ["vertice", "faces", "attributes", "size"]

    def __contains__(self, key):
        return key in ("vertice", "faces", "attributes", "size")

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return 4

    def get(self, key, default=None):
        return self[key] if key in self else default

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]


class RGBDRenderer:
    def __init__(self, device):
        self.device = device
        self.eps = 1e-4
        self.near_z = 1e-4
        self.far_z = 1e4
        self.blur_radius = 1e-6

    def render_mesh(self, mesh_dict, cam_int, cam_ext):
        """mesh_dict of construct_mesh (or vertice [b,h*w,3], attributes [b,h*w,4], size), cam_int [b,3,3], cam_ext [b,3,4] ->
        (render * mask [b,3,h,w], disparity * mask [b,1,h,w], mask [b,1,h,w])"""
        h, w = mesh_dict["size"]
        if isinstance(mesh_dict, _MeshDict) and mesh_dict._cam_int is cam_int and not mesh_dict._by_hand:
            verts, attrs = ops.rgbd_mesh_vertices(mesh_dict._rgbd, cam_int, cam_ext)
        else:
            verts, attrs = self._transform(mesh_dict["vertice"], mesh_dict["attributes"], cam_int, cam_ext, h, w)
        out = ops.rasterize_grid(verts, attrs, h, w, self.blur_radius)[3]
        mask = out[:, 3:4]
        render = out[:, :3]
        disparity = torch.reciprocal(out[:, 4:5] + self.eps)
        return render * mask, disparity * mask, mask

    def _transform(self, vertice, attributes, cam_int, cam_ext, h, w):
        """render_mesh's first half in torch (warpback/utils.py:38-51), for vertices that are not construct_mesh's"""
        world = torch.matmul(cam_ext.unsqueeze(1), self.lift_to_homo(vertice)[..., None]).squeeze(-1)
        attrs = torch.cat([attributes, world[..., -1:]], dim=-1)
        persp = self.get_perspective_from_intrinsic(cam_int)
        ndc = torch.matmul(persp.unsqueeze(1), self.lift_to_homo(world)[..., None]).squeeze(-1)
        ndc = ndc[..., :-1] / ndc[..., -1:]
        ndc[..., :-1] *= -1
        ndc[..., 0] *= w / h
        return ndc.contiguous(), attrs.contiguous()

    def construct_mesh(self, rgbd, cam_int):
        """rgbd [b,4,h,w] (r, g, b, disparity in 0..1), cam_int [b,3,3] -> mesh_dict with the reference's keys: vertice [b,h*w,3], faces
        [b,nface,3], attributes [b,h*w,4], size [h,w].  The tensors are made when they are read; render_mesh reads none of them."""
        if not isinstance(rgbd, torch.Tensor) or rgbd.dim() != 4 or rgbd.shape[1] != 4:
            raise MpiFlowHipError("construct_mesh: rgbd must be a [b,4,h,w] tensor (got %s)" % (tuple(rgbd.shape) if isinstance(rgbd, torch.Tensor) else type(rgbd).__name__))
        return _MeshDict(self, rgbd, cam_int)

    def _unproject(self, rgbd, cam_int):
        b, _, h, w = rgbd.shape
        pixel_2d_homo = self.lift_to_homo(self.get_screen_pixel_coord(h, w))
        depth = torch.reciprocal(rgbd.permute(0, 2, 3, 1)[..., -1:] + self.eps)
        cam_int_inv = torch.inverse(cam_int.double()).to(cam_int.dtype)
        pixel_3d = torch.matmul(cam_int_inv[:, None, None, :, :], pixel_2d_homo[..., None]).squeeze(-1)
        return (pixel_3d * depth).reshape(b, h * w, 3)

    def get_screen_pixel_coord(self, h, w):
        """normalised pixel centres [1,h,w,2], x to the right, y down"""
        x = (torch.arange(w).to(self.device) + 0.5) / w
        y = (torch.arange(h).to(self.device) + 0.5) / h
        return torch.stack([x[None, :].expand(h, w), y[:, None].expand(h, w)], dim=-1)[None]

    def lift_to_homo(self, coord):
        return torch.cat([coord, torch.ones_like(coord[..., -1:])], dim=-1)

    def get_faces(self, h, w):
        """[1,nface,3] int64: per cell (tl, bl, br), then per cell (br, tr, tl)"""
        x = torch.arange(w - 1).to(self.device)
        y = torch.arange(h - 1).to(self.device)
        tl = (y[:, None] * w + x[None, :]).reshape(-1)
        tr, bl, br = tl + 1, tl + w, tl + w + 1
        return torch.cat([torch.stack([tl, bl, br], dim=-1), torch.stack([br, tr, tl], dim=-1)], dim=0)[None]

    def get_visible_mask(self, disparity, beta=10, alpha_threshold=0.3):
        """disparity [b,h,w,1] -> 1 where exp(-beta |Sobel(disparity)|) > alpha_threshold, else 0, [b,h,w,1]"""
        import torch.nn.functional as F
        b, h, w, _ = disparity.size()
        d = disparity.reshape(b, 1, h, w)
        kx = torch.tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])[None, None].float().to(d.device)
        ky = torch.tensor([[-1, -2, -1], [0, 0, 0], [1, 2, 1]])[None, None].float().to(d.device)
        mag = torch.sqrt(F.conv2d(d, kx, padding=(1, 1)) ** 2 + F.conv2d(d, ky, padding=(1, 1)) ** 2).reshape(b, h, w, 1)
        return torch.greater(torch.exp(-1.0 * beta * mag), alpha_threshold).float()

    def get_perspective_from_intrinsic(self, cam_int):
        """cam_int [b,3,3] -> the near / far perspective matrix [b,4,4]"""
        fx, fy = cam_int[:, 0, 0], cam_int[:, 1, 1]
        cx, cy = cam_int[:, 0, 2], cam_int[:, 1, 2]
        one, zero = torch.ones_like(cx), torch.zeros_like(cx)
        near_z, far_z = self.near_z * one, self.far_z * one
        a = (near_z + far_z) / (far_z - near_z)
        b = -2.0 * near_z * far_z / (far_z - near_z)
        rows = [[2.0 * fx, zero, 2.0 * cx - 1.0, zero], [zero, 2.0 * fy, 2.0 * cy - 1.0, zero], [zero, zero, a, b], [zero, zero, one, zero]]
        return torch.stack([torch.stack(row, dim=-1) for row in rows], dim=-2)
