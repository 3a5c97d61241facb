#!/usr/bin/env python3
"""Record the warp-back renderer's vertex pipeline and poses by RUNNING THE REFERENCE ITSELF (warpback/utils.py: RGBDRenderer and the pose
helpers; warpback/stage1_dataset.py: get_rand_ext) on the CPU -> tests/golden/warpback.npz.

    python tests/golden/make_warpback_golden.py [--out PATH]   (in the build container: needs the reference tree, numpy, torch)

pytorch3d is installed nowhere: `pytorch3d.*` is stubbed so that rasterize_meshes and interpolate_face_attributes RECORD their arguments and
return dummies of the right shapes.  What the file holds is therefore everything the reference computes up to the rasteriser - verts_ndc (the
Meshes' vertices), faces, face_attributes - and nothing of pytorch3d's own arithmetic, whose parity is unpinned.

Inputs (sample_rgbd below, rebuilt by the test from the seed): B = 2 RGB-D images of 16 x 24, a smooth disparity with a step edge, at one
pose per image with translation in x, y, z and a small rotation.  Also: the pose helpers on seeded arguments, and get_rand_ext's draws under
torch.manual_seed(SEED) for two trans_range settings.  The recorder asserts that at most 0.5 % of the vertices have a Sobel alpha within 1e-5
of the 0.3 threshold (near_threshold marks them), so that the visibility bit is pinned everywhere else."""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 8200
B, H, W = 2, 16, 24
K = [[0.58, 0, 0.5], [0, 0.58, 0.5], [0, 0, 1]]
POSES = [([0.02, -0.015, 0.01], [0.2, -0.05, 0.08]), ([-0.01, 0.03, -0.02], [-0.15, 0.1, -0.06])]      # (axis-angle, translation) per image
RANGES = [{"x": 0.2, "y": -1, "z": -1, "a": -1, "b": -1, "c": -1}, {"x": 0.2, "y": 0.1, "z": 0.05, "a": 48, "b": 64, "c": 96}]
BAND = 1e-5


def sample_rgbd(seed=SEED, b=B, h=H, w=W):
    """[b,4,h,w] float32: noise colours; a smooth disparity near 0.3 with a step to 0.9 right of a slanted line (the zero padding of the Sobel
    hides the border vertices as well)"""
    rng = np.random.default_rng(seed)
    rgb = rng.random((b, 3, h, w))
    y, x = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
    disp = np.stack([0.3 + 0.04 * np.sin(3 * x + i) * np.cos(2 * y) + 0.004 * rng.random((h, w)) for i in range(b)])
    disp = np.where((x + 0.3 * y > 0.6)[None], 0.9 - 0.02 * y[None], disp)
    return np.concatenate([rgb, disp[:, None]], axis=1).astype(np.float32)


def install_stubs(captured):
    import torch
    names = ("pytorch3d", "pytorch3d.renderer", "pytorch3d.renderer.mesh", "pytorch3d.structures", "pytorch3d.ops")
    mods = {n: types.ModuleType(n) for n in names}

    class Meshes:
        def __init__(self, verts, faces):
            self.verts, self.faces = verts, faces
            captured["verts_ndc"], captured["faces"] = verts.clone(), faces.clone()

    def rasterize_meshes(mesh, image_size, faces_per_pixel=None, blur_radius=None, **kw):
        b, (h, w) = mesh.verts.shape[0], image_size
        captured["raster_kwargs"] = dict(image_size=tuple(image_size), faces_per_pixel=faces_per_pixel, blur_radius=blur_radius, **kw)
        return (torch.full((b, h, w, 1), -1, dtype=torch.int64), torch.full((b, h, w, 1), -1.0), torch.full((b, h, w, 1, 3), -1.0), torch.full((b, h, w, 1), -1.0))

    def interpolate_face_attributes(pix_to_face, bary, face_attributes):
        captured["face_attributes"] = face_attributes.clone()
        return torch.zeros(pix_to_face.shape + (face_attributes.shape[-1],))

    mods["pytorch3d.renderer.mesh"].rasterize_meshes = rasterize_meshes
    mods["pytorch3d.structures"].Meshes = Meshes
    mods["pytorch3d.ops"].interpolate_face_attributes = interpolate_face_attributes
    sys.modules.update(mods)
    if "PIL" not in sys.modules:
        try:
            import PIL  # noqa: F401
        except Exception:                                    # noqa: BLE001  only the image readers use it; they are not run here
            pil = types.ModuleType("PIL")
            pil.Image = types.ModuleType("PIL.Image")
            sys.modules.update({"PIL": pil, "PIL.Image": pil.Image})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "warpback.npz"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, HERE)
    import ref_harness
    ref_harness.install()
    captured = {}
    install_stubs(captured)
    from warpback.utils import RGBDRenderer, get_translation_matrix, rot_from_axisangle, transformation_from_parameters   # the reference's own
    from warpback.stage1_dataset import WarpBackStage1Dataset

    rgbd = sample_rgbd()
    cam_int = torch.tensor(K)[None].repeat(B, 1, 1)
    axisangle = torch.tensor([p[0] for p in POSES])[:, None, :]
    translation = torch.tensor([p[1] for p in POSES])[:, None, :]
    M = transformation_from_parameters(axisangle, translation)
    M_inv = transformation_from_parameters(axisangle, translation, invert=True)
    cam_ext = M[:, :-1].contiguous()
    r = RGBDRenderer("cpu")
    mesh = r.construct_mesh(torch.from_numpy(rgbd), cam_int)
    r.render_mesh(mesh, cam_int, cam_ext)
    assert captured["raster_kwargs"] == dict(image_size=(H, W), faces_per_pixel=1, blur_radius=1e-6), captured["raster_kwargs"]
    nf = captured["faces"].shape[1]
    assert captured["face_attributes"].shape == (B * nf, 3, 5) and captured["verts_ndc"].shape == (B, H * W, 3)

    # the Sobel alpha, by the reference's own expressions (get_visible_mask returns only the bit)
    d = torch.from_numpy(rgbd[:, 3:4])
    kx = torch.tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])[None, None].float()
    ky = torch.tensor([[-1, -2, -1], [0, 0, 0], [1, 2, 1]])[None, None].float()
    alpha = torch.exp(-1.0 * 10 * torch.sqrt(F.conv2d(d, kx, padding=(1, 1)) ** 2 + F.conv2d(d, ky, padding=(1, 1)) ** 2)).reshape(B, H * W)
    vis = torch.greater(alpha, 0.3).float()
    assert torch.equal(vis, mesh["attributes"][..., 3])
    near = (alpha - 0.3).abs() < BAND
    share = float(near.float().mean())
    assert share <= 0.005, share
    hidden = float(1 - vis.mean())
    assert 0.02 < hidden < 0.5, hidden                       # the step edge hides some vertices, not most

    rec = {"seed": np.int64(SEED), "rgbd_sum": np.float64(rgbd.astype(np.float64).sum()), "cam_int": cam_int.numpy(), "cam_ext": cam_ext.numpy(),
           "axisangle": axisangle.numpy(), "translation": translation.numpy(), "M": M.numpy(), "M_inv": M_inv.numpy(),
           "rot": rot_from_axisangle(axisangle).numpy(), "trans": get_translation_matrix(translation).numpy(),
           "persp": r.get_perspective_from_intrinsic(cam_int).numpy(),
           "vertice": mesh["vertice"].numpy(), "attributes": mesh["attributes"].numpy(), "verts_ndc": captured["verts_ndc"].numpy(),
           "faces": captured["faces"].numpy().astype(np.int32), "face_attributes": captured["face_attributes"].numpy(),
           "near_threshold": near.numpy(), "near_threshold_share": np.float64(share), "torch_version": np.array(torch.__version__)}
    for i, tr in enumerate(RANGES):
        ds = WarpBackStage1Dataset(data_root=os.path.join(HERE, "no_such_directory"), device="cpu", trans_range=dict(tr))
        torch.manual_seed(SEED + i)
        ext, ext_inv = ds.get_rand_ext(4)
        rec["rand_ext_%d" % i], rec["rand_ext_inv_%d" % i] = ext.numpy(), ext_inv.numpy()
        rec["rand_after_%d" % i] = torch.rand(3).numpy()     # the generator's state afterwards: the draws were consumed in the same number
    np.savez_compressed(a.out, **rec)
    print("wrote %s, %d bytes; %.2f %% of the vertices within %g of the threshold, %.1f %% hidden" % (a.out, os.path.getsize(a.out), 100 * share, BAND, 100 * hidden))
    assert os.path.getsize(a.out) < 200 * 1000
    return 0


if __name__ == "__main__":
    sys.exit(main())
