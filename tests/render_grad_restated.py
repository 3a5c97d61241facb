"""The formulas of the reference's utils/mpi renderer, restated in plain torch (any device, any float dtype, differentiable by construction): the
baseline tools/bench_render_grad.py times the HIP forward + backward against on the same GPU, and what tests/test_render_grad_host.py checks against
the reference's own float64 gradients.  This is the project's own text of published formulas (plane-induced homography, bilinear border sampling,
front-to-back volume rendering of a multiplane image); it materialises every [B,S,C,H,W] intermediate, as the reference does."""
import torch
import torch.nn.functional as F


def meshgrid(H, W, like):
    y, x = torch.meshgrid(torch.arange(H, dtype=like.dtype, device=like.device), torch.arange(W, dtype=like.dtype, device=like.device), indexing="ij")
    return torch.stack((x, y, torch.ones_like(x)))                                 # 3xHxW: (x, y, 1)


def homographies(depth_B, G, K_inv, K):
    """H_tgt_src = K (R + t n^T / d) K^-1 for the plane n = (0, 0, 1) at depth d"""
    n = torch.tensor([0.0, 0.0, 1.0], dtype=K.dtype, device=K.device).view(1, 1, 3)
    R_tnd = G[:, :3, :3] + G[:, :3, 3:4] * n / depth_B.view(-1, 1, 1)
    return K @ R_tnd @ K_inv


def sample(src_BCHW, depth_B, G, K_inv, K):
    """every plane warped into the target view: -> (tgt_BCHW, valid BxHxW, flowB2A BxHxWx2)"""
    B, _, H, W = src_BCHW.shape
    with torch.no_grad():
        H_src_tgt = torch.linalg.inv(homographies(depth_B, G, K_inv, K).double()).to(K.dtype)
    grid = meshgrid(H, W, src_BCHW).view(1, 3, -1)
    q = (H_src_tgt @ grid).view(B, 3, H, W).permute(0, 2, 3, 1)
    uv = q[..., 0:2] / q[..., 2:]
    flow = uv - grid.view(1, 3, H, W).permute(0, 2, 3, 1)[..., 0:2]
    valid = (uv[..., 0] < W) & (uv[..., 0] > -1) & (uv[..., 1] < H) & (uv[..., 1] > -1)
    norm = torch.stack(((uv[..., 0] + 0.5) / (W * 0.5) - 1, (uv[..., 1] + 0.5) / (H * 0.5) - 1), dim=-1)
    return F.grid_sample(src_BCHW, norm, padding_mode="border", align_corners=False), valid, flow


def flow_src_to_tgt(depth_B, G, K_inv, K, H, W):
    grid = meshgrid(H, W, K).view(1, 3, -1)
    q = (homographies(depth_B, G, K_inv, K) @ grid).view(-1, 3, H, W).permute(0, 2, 3, 1)
    return q[..., 0:2] / q[..., 2:] - grid.view(1, 3, H, W).permute(0, 2, 3, 1)[..., 0:2]


def weights_of(sigma_BS1HW, xyz_BS3HW):
    """-> (transparency_acc A_s, weights w_s = A_s (1 - t_s)) with t_s = exp(-sigma_s |xyz_{s+1} - xyz_s|), the last distance 1e3"""
    B, S, _, H, W = sigma_BS1HW.shape
    dist = torch.norm(xyz_BS3HW[:, 1:] - xyz_BS3HW[:, :-1], dim=2, keepdim=True)
    dist = torch.cat((dist, torch.full((B, 1, 1, H, W), 1e3, dtype=dist.dtype, device=dist.device)), dim=1)
    t = torch.exp(-sigma_BS1HW * dist)
    acc = torch.cumprod(t + 1e-6, dim=1)
    acc = torch.cat((torch.ones_like(acc[:, :1]), acc[:, :-1]), dim=1)
    return acc, acc * (1 - t)


def render(rgb, sigma, xyz, src_sigma=None, src_flow=None, src_xyz=None, hard_flow=False, obj_mask=None):
    """-> (rgb Bx3xHxW, depth Bx1xHxW, transparency_acc, weights, flowA2B | None, rendered mask | obj_mask)"""
    acc, w = weights_of(sigma, xyz)
    rgb_out = (w * rgb).sum(1)
    depth = (w * xyz[:, :, 2:]).sum(1) / (w.sum(1) + 1e-5)
    flow = None
    if src_sigma is not None:
        obj_mask = (w * obj_mask).sum(1)
        _, ws = weights_of(src_sigma, src_xyz)
        if hard_flow:
            ws = torch.zeros_like(ws).scatter_(1, ws.max(1, keepdim=True)[1], 1.0)
        flow = (ws * src_flow).sum(1)
    return rgb_out, depth, acc, w, flow, obj_mask


def plane_xyz(disparity_BS, G, K_inv, H, W):
    """-> (xyz_src, xyz_tgt) BxSx3xHxW of the fronto-parallel planes"""
    B, S = disparity_BS.shape
    rays = (K_inv @ meshgrid(H, W, K_inv).view(1, 3, -1)).view(B, 1, 3, H * W)
    xyz_src = rays / disparity_BS.view(B, S, 1, 1)
    xyz_tgt = G[:, None, :3, :3] @ xyz_src + G[:, None, :3, 3:4]
    return xyz_src.view(B, S, 3, H, W), xyz_tgt.view(B, S, 3, H, W)


def render_tgt_rgb_depth(mpi_rgb_src, mpi_sigma_src, disparity_BS, G, K_inv, K, hard_flow=False, obj_mask=None):
    """-> (rgb, depth, tgt_mask, flowA2B, rendered mask)"""
    B, S, _, H, W = mpi_rgb_src.shape
    xyz_src, xyz_tgt = plane_xyz(disparity_BS, G, K_inv, H, W)
    stack = torch.cat((mpi_rgb_src, mpi_sigma_src, xyz_tgt) + ((obj_mask,) if obj_mask is not None else ()), dim=2)
    rep = lambda m: m.unsqueeze(1).expand(B, S, *m.shape[1:]).reshape(B * S, *m.shape[1:])
    depth_Bs = torch.reciprocal(disparity_BS).reshape(B * S)
    tgt, valid, _ = sample(stack.view(B * S, -1, H, W), depth_Bs, rep(G), rep(K_inv), rep(K))
    flowB2A = flow_src_to_tgt(depth_Bs, rep(G), rep(K_inv), rep(K), H, W).permute(0, 3, 1, 2).reshape(B, S, 2, H, W)
    tgt = tgt.view(B, S, -1, H, W)
    t_rgb, t_sigma, t_xyz = tgt[:, :, 0:3], tgt[:, :, 3:4], tgt[:, :, 4:7]
    t_sigma = torch.where(t_xyz[:, :, 2:] >= 0, t_sigma, torch.zeros_like(t_sigma))
    rgb, depth, _, _, flow, om = render(t_rgb, t_sigma, t_xyz, mpi_sigma_src, flowB2A, xyz_src, hard_flow=hard_flow,
                                        obj_mask=tgt[:, :, 7:] if obj_mask is not None else torch.zeros_like(t_sigma))
    tgt_mask = valid.view(B, S, H, W).to(rgb.dtype).sum(1, keepdim=True)
    return rgb, depth, tgt_mask, flow, (om if obj_mask is not None else None)
