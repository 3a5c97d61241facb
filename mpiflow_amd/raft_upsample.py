"""RAFT's convex upsampling and sequence loss on the GPU, fused: drop-ins for RAFT.upsample_flow (RAFT/core/raft.py:72-83) and for
sequence_loss (RAFT/train.py:47-72).

Three ways in:

    from mpiflow_amd.raft_upsample import upsample_flow                  # (a) leave raft.py and train.py as they are
    RAFT.upsample_flow = lambda self, flow, mask: upsample_flow(flow, mask)

    from mpiflow_amd.raft_upsample import sequence_loss                  # (b) hand the COARSE flows and masks to the loss
    loss, metrics = sequence_loss(flows, masks, flow_gt, valid, gamma)   #     (RAFT.forward appends (coords1 - coords0, up_mask) instead of flow_up)

    loss, metrics = sequence_loss(flows, None, flow_gt, valid, gamma)    # (c) the small model: coarse flows alone, masks=None

(a) replaces the softmax / unfold / product / sum / permute chain, and the [N,2,9,8,8,H,W] product it keeps for backward, by one kernel each
way.  (b) goes further: a prediction is blended in registers, compared with the ground truth and summed, and never exists in memory; the
backward pass recomputes it.  Each prediction is ONE autograd node that saves only its inputs, so backward frees iteration by iteration.
`upflow8` is the small model's upsampling (no mask: 8 x bilinear, align_corners=True), one kernel each way.  (c) is (b) for it: with None in
place of the mask(s), `flow_loss_term` and `sequence_loss` form 8 x bilinear(flow) in registers with upflow8's own coordinate arithmetic
(mpf_upflow8_loss_term / _backward); backward is a gather per coarse pixel and writes only grad_flow.

What differs from upstream: `sequence_loss` takes (flows, masks) instead of the upsampled predictions; its sums are folded in fp64 in a fixed
order (upstream: torch's fp32 mean), so results are bit-identical from run to run; the four metrics cost one device-to-host copy of five
numbers instead of four `.item()` calls.  float32 only: a half-precision mask (what --mixed_precision hands over) is refused with a message
that says to call `.float()`.  Tensors are held to the contract of _tensors.py: no eager fallback, MpiFlowHipError.
"""
import torch

from . import ops
from ._lib import MpiFlowHipError


class _Upsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, mask):
        ctx.save_for_backward(flow, mask)
        return ops.upsample_flow(flow, mask)

    @staticmethod
    def backward(ctx, grad_out):
        flow, mask = ctx.saved_tensors
        return ops.upsample_flow_backward(flow, mask, grad_out.contiguous())


class _LossTerm(torch.autograd.Function):
    """term = flow_loss_term(flow, mask, flow_gt, valid); gradients for flow and mask, None for the rest.  With want_metrics the five
    accumulators ride along as a second, non-differentiable output."""

    @staticmethod
    def forward(ctx, flow, mask, flow_gt, valid, max_flow, want_metrics):
        ctx.max_flow = max_flow
        ctx.save_for_backward(flow, mask, flow_gt, valid)
        term, acc = ops.flow_loss_term(flow, mask, flow_gt, valid, max_flow, metrics=want_metrics)
        if not want_metrics:
            return term
        ctx.mark_non_differentiable(acc)
        return term, acc

    @staticmethod
    def backward(ctx, g, *unused):
        flow, mask, flow_gt, valid = ctx.saved_tensors
        gf, gm = ops.flow_loss_term_backward(flow, mask, flow_gt, valid, g.contiguous(), ctx.max_flow)
        return gf, gm, None, None, None, None


class _Up8LossTerm(torch.autograd.Function):
    """term = flow_loss_term(flow, None, flow_gt, valid): _LossTerm for the small model's bilinear prediction; gradient for flow alone"""

    @staticmethod
    def forward(ctx, flow, flow_gt, valid, max_flow, want_metrics):
        ctx.max_flow = max_flow
        ctx.save_for_backward(flow, flow_gt, valid)
        term, acc = ops.upflow8_loss_term(flow, flow_gt, valid, max_flow, metrics=want_metrics)
        if not want_metrics:
            return term
        ctx.mark_non_differentiable(acc)
        return term, acc

    @staticmethod
    def backward(ctx, g, *unused):
        flow, flow_gt, valid = ctx.saved_tensors
        return ops.upflow8_loss_term_backward(flow, flow_gt, valid, g.contiguous(), ctx.max_flow), None, None, None, None


def _term(flow, mask, flow_gt, valid, max_flow, want_metrics):
    if mask is None:
        return _Up8LossTerm.apply(flow, flow_gt, valid, max_flow, want_metrics)
    return _LossTerm.apply(flow, mask, flow_gt, valid, max_flow, want_metrics)


class _Upflow8(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow):
        return ops.upflow8(flow)

    @staticmethod
    def backward(ctx, grad_out):
        return ops.upflow8_backward(grad_out.contiguous())


def upflow8(flow):
    """RAFT/core/utils/utils.py's upflow8, what the small model upsamples with: flow [N,2,H,W] -> 8 * F.interpolate(flow, (8H, 8W),
    mode='bilinear', align_corners=True), differentiable.  One kernel each way (mpf_upflow8, mpf_upflow8_backward: a gather, no atomics).
    float32, contiguous, on the GPU."""
    return _Upflow8.apply(flow)


def upsample_flow(flow, mask):
    """RAFT.upsample_flow: flow [N,2,H,W], mask [N,576,H,W] -> [N,2,8H,8W], differentiable in both.  float32, contiguous, on the GPU."""
    return _Upsample.apply(flow, mask)


def flow_loss_term(flow, mask, flow_gt, valid, max_flow=400):
    """(v[:,None] * |upsample_flow(flow, mask) - flow_gt|).mean() as a 0-d device tensor, v = (valid >= 0.5) & (|flow_gt| < max_flow), without
    the prediction ever being written.  Differentiable in flow and mask.  flow_gt [N,2,8H,8W], valid [N,8H,8W], float32.
    mask=None: the small model's term, with upflow8(flow) in place of upsample_flow(flow, mask); differentiable in flow."""
    return _term(flow, mask, flow_gt, valid, float(max_flow), False)


def sequence_loss(flows, masks, flow_gt, valid, gamma=0.8, max_flow=400):
    """train.py's sequence_loss on the coarse flows and masks of the refinement iterations:
    loss = sum_i gamma**(n-1-i) * flow_loss_term(flows[i], masks[i], ...); metrics = {'epe', '1px', '3px', '5px'} of the LAST prediction as
    Python floats (one device-to-host copy, the only synchronisation; nan where no pixel is valid, as upstream).
    masks=None: the small model's loss, every prediction upflow8(flows[i]) (flow_loss_term with mask=None)."""
    flows = list(flows)
    bilinear = masks is None
    masks = [None] * len(flows) if bilinear else list(masks)
    n = len(flows)
    if n < 1 or len(masks) != n:
        raise MpiFlowHipError("sequence_loss: needs as many masks as flows, at least one (got %d flows, %d masks)" % (n, len(masks)))
    node = _term if bilinear else _LossTerm.apply                       # a None inside a list of masks is refused as before
    loss = 0.0
    acc = None
    for i in range(n):
        weight = gamma ** (n - i - 1)
        if i < n - 1:
            term = node(flows[i], masks[i], flow_gt, valid, float(max_flow), False)
        else:
            term, acc = node(flows[i], masks[i], flow_gt, valid, float(max_flow), True)
        loss = loss + weight * term
    esum, n1, n3, n5, nv = acc.tolist()
    nan = float("nan")
    metrics = {"epe": esum / nv if nv else nan, "1px": n1 / nv if nv else nan, "3px": n3 / nv if nv else nan, "5px": n5 / nv if nv else nan}
    return loss, metrics
