"""Drop-in for the reference's utils/mpi/rendering_utils.py: same names, same signatures.

transform_G_xyz (:4-23) is the part on the generation path.  The training-time samplers of that file (:26-139), which the generation path never
calls, are provided too:

gather_pixel_by_pxpy                            mpf_gather_pxpy; differentiable with respect to img (a float-atomic scatter-add), never pxpy
uniformly_sample_disparity_from_bins            [B,S] outputs: plain torch on the device, drawing with the reference's one torch.rand((B, S))
uniformly_sample_disparity_from_linspace_bins   the same
sample_pdf                                      the reference's torch.rand, then mpf_sample_pdf in one launch; forward only
"""
import torch

from ... import _lib, ops
from . import _autograd


def transform_G_xyz(G, xyz, is_return_homo=False):
    """xyz_out = (G . [xyz; 1])[:3]  -  reference utils/mpi/rendering_utils.py:4-23.

    :param G: Bx4x4 (or 4x4 with xyz 3xN); every batch entry must hold the same matrix (the reference's callers
              repeat one G over the S planes, utils/mpi/mpi_rendering.py:251-254)
    :param xyz: Bx3xN on the GPU
    :return: Bx3xN (Bx4xN with a row of ones when is_return_homo)"""
    assert len(G.size()) == len(xyz.size())
    squeeze = len(G.size()) == 2
    G_B44 = G.unsqueeze(0) if squeeze else G
    xyz_B3N = xyz.unsqueeze(0) if squeeze else xyz
    G_cpu = G_B44.detach().to("cpu", torch.float32)
    if not bool((G_cpu == G_cpu[0:1]).all()):
        out = torch.stack([ops.transform_xyz(G_cpu[b], xyz_B3N[b:b + 1])[0] for b in range(G_cpu.shape[0])])
    else:
        out = ops.transform_xyz(G_cpu[0], xyz_B3N)
    if is_return_homo:
        out = torch.cat((out, torch.ones_like(out[:, 0:1, :])), dim=1)
    return out[0] if squeeze else out


def gather_pixel_by_pxpy(img, pxpy):
    """out[b,c,i] = img[b,c,y_i,x_i], (x_i, y_i) = pxpy[b,:,i] rounded (ties to even) and clamped to the frame  (reference :26-43)

    :param img: BxCxHxW float32 on the GPU
    :param pxpy: Bx2xN, float32 or an integer dtype; any other dtype raises the reference's own UnboundLocalError (:35-37 binds pxpy_int for float32 only)
    :return: BxCxN

    A NaN or -inf coordinate reads index 0, +inf the last index (the reference leaves them to the platform's float-to-int cast).  Differentiable with
    respect to img (mpf_gather_pxpy_bwd: float atomic adds, so points that share a pixel decide the last bits of its gradient by their order); pxpy
    never receives a gradient, as in the reference, which indexes under torch.no_grad()."""
    if isinstance(pxpy, torch.Tensor) and pxpy.dtype != torch.float32 and (pxpy.dtype.is_floating_point or pxpy.dtype.is_complex):
        raise UnboundLocalError("local variable 'pxpy_int' referenced before assignment (reference utils/mpi/rendering_utils.py:37, pxpy of %s)" % pxpy.dtype)
    if isinstance(pxpy, torch.Tensor):
        pxpy = pxpy.detach()
        if pxpy.dtype != torch.float32:
            pxpy = pxpy.to(torch.int64)                                         # :37
    if _autograd.wants_grad(img):
        _autograd.check_values("gather_pixel_by_pxpy", img=img)
        return _autograd.GatherPxpyFn.apply(img, pxpy)
    return ops.gather_pixel_by_pxpy(img.detach() if isinstance(img, torch.Tensor) else img, pxpy)


def uniformly_sample_disparity_from_bins(batch_size, disparity_np, device):
    """One uniform draw per bin of the S + 1 edges disparity_np (numpy, from large to small)  (reference :46-66) -> BxS on `device`"""
    assert disparity_np[0] > disparity_np[-1]
    S = disparity_np.shape[0] - 1
    B = batch_size
    bin_edges = torch.from_numpy(disparity_np).to(dtype=torch.float32, device=device)      # S+1
    interval = bin_edges[1:] - bin_edges[0:-1]                                              # S
    bin_edges_start = bin_edges[0:-1].unsqueeze(0).repeat(B, 1)
    interval = interval.unsqueeze(0).repeat(B, 1)
    random_float = torch.rand((B, S), dtype=torch.float32, device=device)                   # the one draw: the generator moves as the reference's does
    return bin_edges_start + interval * random_float


def uniformly_sample_disparity_from_linspace_bins(batch_size, num_bins, start, end, device):
    """One uniform draw per bin of num_bins equal bins from start down to end  (reference :69-87) -> BxS on `device`"""
    assert start > end
    B, S = batch_size, num_bins
    bin_edges = torch.linspace(start, end, num_bins + 1, dtype=torch.float32, device=device)
    interval = bin_edges[1] - bin_edges[0]
    bin_edges_start = bin_edges[0:-1].unsqueeze(0).repeat(B, 1)
    random_float = torch.rand((B, S), dtype=torch.float32, device=device)
    return bin_edges_start + interval * random_float


def sample_pdf(values, weights, N_samples):
    """Draw N_samples per ray from the piecewise-linear distribution weights = p(values)  (reference :90-139)

    :param values: Bx1xNxS float32 on the GPU, contiguous or expanded over N (stride 0 in dim 2), which is read in place
    :param weights: Bx1xNxS float32 on the GPU, contiguous
    :param N_samples: 1..128 (S too)
    :return: Bx1xNxN_samples

    The uniform draws are the reference's torch.rand((B, 1, N, N_samples), dtype=weights.dtype, device=weights.device): same shape, dtype and place in the
    generator's stream; everything after them is one launch (ops.sample_pdf).  Forward only: values or weights requiring grad while grad mode is on is
    refused."""
    for name, t in (("values", values), ("weights", weights)):
        if _autograd.wants_grad(t):
            raise _lib.MpiFlowHipError("sample_pdf: %s requires grad, but sample_pdf is forward only here (its gradient is not provided); detach %s"
                                       % (name, name))
    B, N, S = weights.size(0), weights.size(2), weights.size(3)
    assert values.size() == (B, 1, N, S)
    u = torch.rand((B, 1, N, N_samples), dtype=weights.dtype, device=weights.device)
    return ops.sample_pdf(values.detach(), weights.detach(), u)
