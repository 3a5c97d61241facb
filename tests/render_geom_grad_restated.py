"""The geometry gradients of the utils/mpi renderer written out BY HAND in plain torch (any float dtype, no autograd): the formulas that the HIP kernels
mpf_volume_render_bwd_xyz, mpf_src_xyz_bwd, mpf_plane_flow_bwd and mpf_warp_composite_bwd_disp implement.  tests/test_render_geom_grad_host.py checks
them in float64 against the reference's own float64 autograd (tests/golden/render_geom_grad.npz); tests/test_render_geom_grad.py checks the kernels
against them where the golden has no case (S above a wave's 64 lanes)."""
import torch

import render_grad_restated as rr


def composite_xyz_grad(sigma, xyz, rgb=None, extra=None, g_rgb=None, g_depth=None, g_extra=None, g_w=None, g_tacc=None):
    """Item 1.  sigma [S,N], xyz [S,3,N], rgb [S,3,N] | None, extra [S,E,N] | None; upstream g_rgb [3,N], g_depth [N], g_extra [E,N], g_w [S,N],
    g_tacc [S,N] (None: zero) -> dL/dxyz [S,3,N]"""
    S, N = sigma.shape
    diff = xyz[1:] - xyz[:-1]
    dist = torch.cat((diff.norm(dim=1), torch.full((1, N), 1e3, dtype=sigma.dtype)))
    t = torch.exp(-sigma * dist)
    A = torch.cat((torch.ones(1, N, dtype=sigma.dtype), torch.cumprod(t + 1e-6, dim=0)[:-1]))
    w = A * (1 - t)
    Dn = w.sum(0) + 1e-5
    z = xyz[:, 2]
    depth = (w * z).sum(0) / Dn
    q = torch.zeros_like(sigma)
    if g_depth is not None:
        q = q + g_depth * (z - depth) / Dn
    if g_w is not None:
        q = q + g_w
    if rgb is not None and g_rgb is not None:
        q = q + (rgb * g_rgb).sum(1)
    if extra is not None and g_extra is not None:
        q = q + (extra * g_extra).sum(1)
    a = q * (1 - t)
    if g_tacc is not None:
        a = a + g_tacc
    Aa = A * a
    suffix = torch.flip(torch.cumsum(torch.flip(Aa, [0]), 0), [0]) - Aa               # sum_{s>j} A_s a_s
    dLdt = -A * q + suffix / (t + 1e-6)
    g_dist = (-sigma * t * dLdt)[:-1]                                                 # the last distance is a constant
    u = torch.where(dist[:-1] > 0, 1 / dist[:-1], torch.zeros_like(dist[:-1])).unsqueeze(1) * diff
    flow = u * g_dist.unsqueeze(1)                                                    # u_j dL/dd_j, j < S-1
    g = torch.zeros_like(xyz)
    g[1:] += flow
    g[:-1] -= flow
    if g_depth is not None:
        g[:, 2] += g_depth * w / Dn
    return g


def src_xyz_disparity_grad(g_xyz, disparity, K_inv, H, W):
    """Item 3.  g_xyz [S,3,H,W], disparity [S], K_inv [3,3] -> [S]: -depth_s^2 sum_p <g_s(p), K^-1 (x, y, 1)>"""
    rays = K_inv @ rr.meshgrid(H, W, K_inv).view(3, -1)
    return -(g_xyz.reshape(-1, 3, H * W) * rays).sum((1, 2)) / disparity ** 2


def rotate_back(g_xyz, G):
    """Item 3.  g [S,3,N] -> R^T g"""
    return G[:3, :3].t() @ g_xyz


def plane_flow_depth_grad(g_flow, depth, G, K_inv, K, H, W):
    """Item 4.  g_flow [S,H,W,2], depth [S]; G [S,4,4], K_inv, K [S,3,3] -> dL/ddepth [S]"""
    grid = rr.meshgrid(H, W, K).view(1, 3, -1)
    n = torch.tensor([0.0, 0.0, 1.0], dtype=K.dtype).view(1, 1, 3)
    A = K @ G[:, :3, :3] @ K_inv
    Bm = K @ (G[:, :3, 3:4] * n) @ K_inv
    P = (A + Bm / depth.view(-1, 1, 1)) @ grid                                        # (X, Y, Z)
    dP = -(Bm @ grid) / depth.view(-1, 1, 1) ** 2
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    dfx = (dP[:, 0] * Z - X * dP[:, 2]) / Z ** 2
    dfy = (dP[:, 1] * Z - Y * dP[:, 2]) / Z ** 2
    g = g_flow.reshape(-1, H * W, 2)
    return (g[..., 0] * dfx + g[..., 1] * dfy).sum(1)


def fused_disparity_grad(mpi_rgb, mpi_sigma, disparity, G, K_inv, K, g_rgb, g_depth, obj_mask=None, g_mask=None):
    """Item 5, for one batch item.  mpi_rgb [S,3,H,W], mpi_sigma [S,1,H,W], disparity [S]; G [4,4], K_inv, K [3,3]; upstream g_rgb [3,H,W], g_depth
    [1,H,W], the rendered mask's g_mask [1,H,W] -> [S]: sum_q <dL/dxyz_tgt_s(q), -depth_s (xyz_tgt_s(q) - t)>"""
    S, _, H, W = mpi_rgb.shape
    _, xyz_tgt = rr.plane_xyz(disparity.view(1, S), G.unsqueeze(0), K_inv.unsqueeze(0), H, W)
    parts = (mpi_rgb, mpi_sigma, xyz_tgt[0]) + ((obj_mask,) if obj_mask is not None else ())
    rep = lambda m: m.unsqueeze(0).expand(S, *m.shape)
    tgt, _, _ = rr.sample(torch.cat(parts, dim=1), torch.reciprocal(disparity), rep(G), rep(K_inv), rep(K))
    t_xyz = tgt[:, 4:7].reshape(S, 3, -1)
    t_sigma = torch.where(t_xyz[:, 2] >= 0, tgt[:, 3].reshape(S, -1), torch.zeros_like(t_xyz[:, 2]))
    g = composite_xyz_grad(t_sigma, t_xyz, rgb=tgt[:, 0:3].reshape(S, 3, -1), extra=tgt[:, 7:].reshape(S, 1, -1) if obj_mask is not None else None,
                           g_rgb=g_rgb.reshape(3, -1), g_depth=g_depth.reshape(-1), g_extra=g_mask.reshape(1, -1) if obj_mask is not None else None)
    field = -(t_xyz - G[:3, 3].view(1, 3, 1)) / disparity.view(S, 1, 1)
    return (g * field).sum((1, 2))


def flow_route_disparity_grad(src_sigma, disparity, G, K_inv, K, g_flow, H, W):
    """The two paths the rendered source-to-target flow adds, for one batch item: xyz_src -> the flow composite's distances (items 1 and 3) and
    sample_inverse's plane depth (item 4).  src_sigma [S,1,H,W], g_flow [2,H,W] -> [S]"""
    S = disparity.numel()
    rep = lambda m: m.unsqueeze(0).expand(S, *m.shape)
    depth = torch.reciprocal(disparity)
    xyz_src, _ = rr.plane_xyz(disparity.view(1, S), G.unsqueeze(0), K_inv.unsqueeze(0), H, W)
    flowB2A = rr.flow_src_to_tgt(depth, rep(G), rep(K_inv), rep(K), H, W).permute(0, 3, 1, 2)            # [S,2,H,W]
    g_xyz = composite_xyz_grad(src_sigma.reshape(S, -1), xyz_src[0].reshape(S, 3, -1), extra=flowB2A.reshape(S, 2, -1), g_extra=g_flow.reshape(2, -1))
    via_xyz = src_xyz_disparity_grad(g_xyz.reshape(S, 3, H, W), disparity, K_inv, H, W)
    _, ws = rr.weights_of(src_sigma.unsqueeze(0), xyz_src)
    g_fb = (ws[0] * g_flow.unsqueeze(0)).permute(0, 2, 3, 1)                                             # dL/dflowB2A [S,H,W,2]
    via_flow = plane_flow_depth_grad(g_fb, depth, rep(G), rep(K_inv), rep(K), H, W) * (-depth ** 2)
    return via_xyz + via_flow
