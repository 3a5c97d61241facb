"""RAFT's update block on the GPU (RAFT/core/update.py): SepConvGRU, ConvGRU, BasicUpdateBlock and SmallUpdateBlock with the GRU's pointwise
work fused in HIP and the iteration-invariant part of its convolutions hoisted out of the refinement loop.

Two ways in:

    from mpiflow_amd.raft_update import BasicUpdateBlock, SmallUpdateBlock     # (a) RAFT/core/raft.py as written, only this import changes

    from mpiflow_amd.raft_update import SepConvGRU                              # (b) the GRU alone, the context term explicit
    ctx = gru.context(inp)                                                      #     once per forward pass
    for _ in range(iters): net = gru(net, motion_features, context=ctx)         #     instead of gru(net, cat([inp, motion_features]))

Parameter names and shapes are the reference's (convz1.weight ... convq2.bias; encoder.*, flow_head.*, mask.*), so a RAFT checkpoint loads
with load_state_dict(strict=True).

What differs from upstream.  A convolution over cat([h, x]) is the sum of one over h and one over x with the matching slices of the weights,
and x is the same tensor for z, r and q.  Per half the module therefore runs three convolutions - x -> 3C (z|r|q, biases here), h -> 2C (z|r),
r*h -> C - and two kernels, mpf_gru_reset and mpf_gru_update, that read the slices of those outputs in place.  No activation is concatenated,
no sigmoid / tanh / blend tensor exists, and backward is two kernels (mpf_gru_update_backward, mpf_gru_reset_backward) that recompute the gates
and write the pre-activations' gradients straight into one [B,3C,H,W] and one [B,2C,H,W] buffer, which autograd receives as the gradients of
the two convolution outputs (the shared-buffer pattern of raft_corr.CorrBlock): no slice gradient is zero-filled.  x = cat([inp, motion]), and
inp does not change over the iterations: `context(inp)` computes its share of all gate convolutions once, and a call with `context=` convolves
only the motion features.  Results equal upstream's up to fp32 summation order.  The convolutions themselves are torch's (MIOpen).

Limits: tensors are held to the contract of _tensors.py: float32 only (the refusal says to call `.float()`), contiguous NCHW,
on the GPU, the device judged last; nothing runs on the CPU and there is no eager fallback: MpiFlowHipError.  Double backward is refused.
torch.autograd.grad with respect to the GRU's internal convolution outputs is not supported (their gradients travel in the shared buffers).
"""
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import ops
from ._lib import MpiFlowHipError
from ._tensors import check_devices, check_tensor


class _HalfGrads:
    """What the two autograd nodes of one GRU half share: the update node's backward allocates the buffers and fills the z and q slices, the
    reset node's backward - which runs later: the update depends on it through the r*h convolution - fills the r slices and hands them on."""

    def __init__(self):
        self.g3 = self.g2 = self.dh = None


def _terms(hg, xg, cx, C, gate):
    """the slices whose sum is the pre-activation of gate 0 (z) or 1 (r)"""
    return [(hg, gate * C), (xg, gate * C), None if cx is None else (cx, gate * C)]


class _Update(torch.autograd.Function):
    """h' = (1 - z) * h + z * q from the convolution outputs hg [B,2C] (z|r), xg [B,3C] (z|r|q), cx [B,3C] or None, qg [B,C].  Backward returns
    a gradient for qg only; those of h, hg, xg and cx travel in `shared` and are returned by _Reset."""

    @staticmethod
    def forward(ctx, shared, h, hg, xg, cx, qg):
        ctx.shared = shared
        ctx.save_for_backward(h, hg, xg, cx, qg)
        C = h.shape[1]
        return ops.gru_update(h, _terms(hg, xg, cx, C, 0), [(qg, 0), (xg, 2 * C), None if cx is None else (cx, 2 * C)])

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        h, hg, xg, cx, qg = ctx.saved_tensors
        B, C, H, W = h.shape
        s = ctx.shared
        s.g3, s.g2, dq = torch.empty_like(xg), torch.empty_like(hg), torch.empty_like(qg)
        s.dh = ops.gru_update_backward(grad_out.contiguous(), h, _terms(hg, xg, cx, C, 0), [(qg, 0), (xg, 2 * C), None if cx is None else (cx, 2 * C)],
                                       dz=[(s.g3, 0), (s.g2, 0)], dq=[(s.g3, 2 * C), (dq, 0)])
        return None, None, None, None, None, dq


class _Reset(torch.autograd.Function):
    """rh = sigmoid(r) * h.  Its backward completes the shared buffers and returns them: d h (the update's share included), d hg, d xg, d cx."""

    @staticmethod
    def forward(ctx, shared, h, hg, xg, cx):
        ctx.shared = shared
        ctx.save_for_backward(h, hg, xg, cx)
        return ops.gru_reset(h, _terms(hg, xg, cx, h.shape[1], 1))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        h, hg, xg, cx = ctx.saved_tensors
        C = h.shape[1]
        s = ctx.shared
        if s.g3 is None:
            raise MpiFlowHipError("raft_update: a gradient reached r*h that did not come through the GRU's own update (torch.autograd.grad with "
                                  "respect to an internal tensor is not supported)")
        g3, g2, dh = s.g3, s.g2, s.dh
        s.g3 = s.g2 = s.dh = None
        ops.gru_reset_backward(grad_out.contiguous(), h, _terms(hg, xg, cx, C, 1), dr=[(g3, C), (g2, C)], dh=dh)
        return None, dh, g2, g3, (g3 if cx is not None else None)


class GruContext:
    """The iteration-invariant part of a GRU's gate convolutions for one `inp` (from `context(inp)`): per half the [B,3C,H,W] sum-term (z|r|q,
    biases included) and the weights packed for the rest of the input.  Differentiable: its gradient accumulates over the calls that use it."""

    def __init__(self, terms, packed, channels, shape):
        self.terms, self.packed, self.channels, self.shape = terms, packed, channels, shape


class _SplitGRU(nn.Module):
    """The common part of ConvGRU and SepConvGRU: HALVES lists (name suffix, kernel size, padding) of the reference's convolutions."""
    HALVES = ()

    def __init__(self, hidden_dim, input_dim):
        super().__init__()
        self.hidden_dim, self.input_dim = int(hidden_dim), int(input_dim)
        if self.hidden_dim < 1 or self.input_dim < 1:
            raise MpiFlowHipError("%s: hidden_dim and input_dim must be positive (got %s, %s)" % (type(self).__name__, hidden_dim, input_dim))
        for suffix, ksize, pad in self.HALVES:
            for gate in "zrq":                                  # the reference's names, shapes and (torch's default) initialisation
                setattr(self, "conv%s%s" % (gate, suffix), nn.Conv2d(self.hidden_dim + self.input_dim, self.hidden_dim, ksize, padding=pad))

    def _pack(self, n_ctx):
        """per half: (w_ctx [3C,n_ctx,..] or None, bias [3C], w_x [3C,input_dim-n_ctx,..], w_h [2C,C,..] (z|r), w_q [C,C,..]): weights only, a few
        MB, never activations"""
        C = self.hidden_dim
        out = []
        for suffix, _, _ in self.HALVES:
            cz, cr, cq = (getattr(self, "conv%s%s" % (g, suffix)) for g in "zrq")
            wx = torch.cat([cz.weight[:, C:], cr.weight[:, C:], cq.weight[:, C:]], dim=0)
            out.append((wx[:, :n_ctx].contiguous() if n_ctx else None, torch.cat([cz.bias, cr.bias, cq.bias]),
                        wx[:, n_ctx:].contiguous() if n_ctx else wx, torch.cat([cz.weight[:, :C], cr.weight[:, :C]], dim=0),
                        cq.weight[:, :C].contiguous()))
        return out

    def context(self, inp):
        """The share of `inp` - the FIRST inp.shape[1] channels of the GRU's input x = cat([inp, rest]) - in all gate convolutions of both halves,
        biases included.  Compute it once per forward pass and pass it to every call as `context=`."""
        who = type(self).__name__ + ".context"
        inp = check_tensor(inp, "inp", who, 4, "[B,C,H,W]")
        n_ctx = inp.shape[1]
        if not 1 <= n_ctx < self.input_dim:
            raise MpiFlowHipError("%s: inp must have 1..%d channels, fewer than input_dim (got shape %s)" % (who, self.input_dim - 1, tuple(inp.shape)))
        check_devices(who, dict(inp=inp))
        packed = self._pack(n_ctx)
        terms = [F.conv2d(inp, p[0], p[1], padding=half[2]) for p, half in zip(packed, self.HALVES)]
        return GruContext(terms, packed, n_ctx, (inp.shape[0], inp.shape[2], inp.shape[3]))

    def forward(self, h, x, context=None):
        """h [B,hidden_dim,H,W], x [B,input_dim,H,W] -> h'.  With `context=self.context(inp)`, x is the REST of the input: the
        input_dim - inp.shape[1] channels that follow inp in upstream's cat([inp, motion_features])."""
        who = type(self).__name__
        h = check_tensor(h, "h", who, (None, self.hidden_dim, None, None))
        B, C, H, W = h.shape
        if context is None:
            n_x, packed, terms = self.input_dim, self._pack(0), [None] * len(self.HALVES)
        else:
            if not isinstance(context, GruContext) or len(context.terms) != len(self.HALVES):
                raise MpiFlowHipError("%s: context must come from this module's context() (got %s)" % (who, type(context).__name__))
            if context.shape != (B, H, W):
                raise MpiFlowHipError("%s: context was computed for [B,H,W] = %s, h is %s" % (who, list(context.shape), tuple(h.shape)))
            n_x, packed, terms = self.input_dim - context.channels, context.packed, context.terms
        x = check_tensor(x, "x", who, (B, n_x, H, W))
        check_devices(who, dict(h=h, x=x, **({} if context is None else {"context": terms[0]})))
        for (_, bias, w_x, w_h, w_q), cx, (_, _, pad) in zip(packed, terms, self.HALVES):
            shared = _HalfGrads()
            xg = F.conv2d(x, w_x, bias if cx is None else None, padding=pad)
            hg = F.conv2d(h, w_h, None, padding=pad)
            rh = _Reset.apply(shared, h, hg, xg, cx)
            qg = F.conv2d(rh, w_q, None, padding=pad)
            h = _Update.apply(shared, h, hg, xg, cx, qg)
        return h


class ConvGRU(_SplitGRU):
    """RAFT/core/update.py's ConvGRU (3 x 3 gates; the small model's): ConvGRU(hidden_dim, input_dim)(h, x) -> h'.  Parameters convz, convr,
    convq as upstream.  See the module docstring and _SplitGRU.forward / .context."""
    HALVES = (("", 3, 1),)

    def __init__(self, hidden_dim=128, input_dim=192 + 128):
        super().__init__(hidden_dim, input_dim)


class SepConvGRU(_SplitGRU):
    """RAFT/core/update.py's SepConvGRU (a 1 x 5 half, then a 5 x 1 half; the basic model's): SepConvGRU(hidden_dim, input_dim)(h, x) -> h'.
    Parameters convz1 ... convq2 as upstream.  See the module docstring and _SplitGRU.forward / .context."""
    HALVES = (("1", (1, 5), (0, 2)), ("2", (5, 1), (2, 0)))

    def __init__(self, hidden_dim=128, input_dim=256):
        super().__init__(hidden_dim, input_dim)


class FlowHead(nn.Module):
    """upstream's flow head: 3 x 3 conv, ReLU, 3 x 3 conv to 2 channels (torch modules, unchanged)"""

    def __init__(self, input_dim=128, hidden_dim=256):
        super().__init__()
        self.conv1 = nn.Conv2d(input_dim, hidden_dim, 3, padding=1)
        self.conv2 = nn.Conv2d(hidden_dim, 2, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.conv2(self.relu(self.conv1(x)))


class BasicMotionEncoder(nn.Module):
    """upstream's motion encoder of the basic model (torch modules, unchanged): (flow, corr) -> [B,128,H,W], the last two channels the flow"""

    def __init__(self, args):
        super().__init__()
        cor_planes = args.corr_levels * (2 * args.corr_radius + 1) ** 2
        self.convc1 = nn.Conv2d(cor_planes, 256, 1, padding=0)
        self.convc2 = nn.Conv2d(256, 192, 3, padding=1)
        self.convf1 = nn.Conv2d(2, 128, 7, padding=3)
        self.convf2 = nn.Conv2d(128, 64, 3, padding=1)
        self.conv = nn.Conv2d(64 + 192, 128 - 2, 3, padding=1)

    def forward(self, flow, corr):
        cor = F.relu(self.convc2(F.relu(self.convc1(corr))))
        flo = F.relu(self.convf2(F.relu(self.convf1(flow))))
        out = F.relu(self.conv(torch.cat([cor, flo], dim=1)))
        return torch.cat([out, flow], dim=1)


class SmallMotionEncoder(nn.Module):
    """upstream's motion encoder of the small model (torch modules, unchanged): (flow, corr) -> [B,82,H,W]"""

    def __init__(self, args):
        super().__init__()
        cor_planes = args.corr_levels * (2 * args.corr_radius + 1) ** 2
        self.convc1 = nn.Conv2d(cor_planes, 96, 1, padding=0)
        self.convf1 = nn.Conv2d(2, 64, 7, padding=3)
        self.convf2 = nn.Conv2d(64, 32, 3, padding=1)
        self.conv = nn.Conv2d(128, 80, 3, padding=1)

    def forward(self, flow, corr):
        cor = F.relu(self.convc1(corr))
        flo = F.relu(self.convf2(F.relu(self.convf1(flow))))
        out = F.relu(self.conv(torch.cat([cor, flo], dim=1)))
        return torch.cat([out, flow], dim=1)


class _UpdateBlock(nn.Module):
    """What both update blocks share: the GRU call with the context term of `inp` cached over the refinement iterations.

    The cache: the block computes gru.context(inp) at the first call with a given `inp` and reuses it while THE SAME TENSOR OBJECT, at the same
    `_version` (no in-place change since), keeps arriving, the GRU's parameters are at the versions they had (an optimizer step changes them)
    and grad mode is what it was.  Anything else recomputes it; reset() drops it; hoist_context=False computes it at every call and keeps
    nothing.  `context_computed` counts the computations.

    A finished step's graph is not kept alive past the next forward pass, in two ways: the cache refers to `inp` only weakly and empties itself
    when that tensor dies (at the end of RAFT.forward, or after backward where the graph held it); and whatever is still cached is replaced at the
    first call of the next forward pass, whose `inp` is another tensor.  What can outlive a step until then is the context tensor itself, not the
    step's saved activations, which backward() frees as usual."""

    def _init_cache(self, hoist_context):
        self.hoist_context = bool(hoist_context)
        self.context_computed = 0
        self._cache = None

    def reset(self):
        """forget the cached context"""
        self._cache = None

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_cache"] = None                                  # a weak reference cannot be pickled or deep-copied
        return state

    def _key(self, inp):
        return (inp._version, torch.is_grad_enabled(), tuple(p._version for p in self.gru.parameters()))

    def _context(self, inp):
        if not isinstance(inp, torch.Tensor):
            raise MpiFlowHipError("%s: inp must be a torch.Tensor (got %s)" % (type(self).__name__, type(inp).__name__))
        c = self._cache
        if self.hoist_context and c is not None and c[0]() is inp and c[1] == self._key(inp):
            return c[2]
        context = self.gru.context(inp)
        self.context_computed += 1
        if self.hoist_context:
            me = weakref.ref(self)

            def drop(ref, me=me):
                blk = me()
                if blk is not None and blk._cache is not None and blk._cache[0] is ref:
                    blk._cache = None
            self._cache = (weakref.ref(inp, drop), self._key(inp), context)
        return context


class BasicUpdateBlock(_UpdateBlock):
    """RAFT/core/update.py's BasicUpdateBlock: BasicUpdateBlock(args, hidden_dim=128)(net, inp, corr, flow) -> (net, mask, delta_flow), same
    constructor, parameter names and results as upstream (args.corr_levels, args.corr_radius).  The motion encoder, the flow head and the mask
    head are torch modules as upstream; the GRU is SepConvGRU of this module, fed inp's share through the cached context (see _UpdateBlock) and
    the motion features directly: cat([inp, motion_features]) is never built."""

    def __init__(self, args, hidden_dim=128, input_dim=128, hoist_context=True):
        super().__init__()
        self.args = args
        self.encoder = BasicMotionEncoder(args)
        self.gru = SepConvGRU(hidden_dim=hidden_dim, input_dim=128 + hidden_dim)
        self.flow_head = FlowHead(hidden_dim, hidden_dim=256)
        self.mask = nn.Sequential(nn.Conv2d(128, 256, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(256, 64 * 9, 1, padding=0))
        self._init_cache(hoist_context)

    def forward(self, net, inp, corr, flow, upsample=True):
        context = self._context(inp)
        net = self.gru(net, self.encoder(flow, corr), context=context)
        delta_flow = self.flow_head(net)
        mask = .25 * self.mask(net)                             # upstream's scale, to balance gradients
        return net, mask, delta_flow


class SmallUpdateBlock(_UpdateBlock):
    """RAFT/core/update.py's SmallUpdateBlock: SmallUpdateBlock(args, hidden_dim=96)(net, inp, corr, flow) -> (net, None, delta_flow); ConvGRU
    of this module, otherwise as BasicUpdateBlock."""

    def __init__(self, args, hidden_dim=96, hoist_context=True):
        super().__init__()
        self.encoder = SmallMotionEncoder(args)
        self.gru = ConvGRU(hidden_dim=hidden_dim, input_dim=82 + 64)
        self.flow_head = FlowHead(hidden_dim, hidden_dim=128)
        self._init_cache(hoist_context)

    def forward(self, net, inp, corr, flow):
        context = self._context(inp)
        net = self.gru(net, self.encoder(flow, corr), context=context)
        return net, None, self.flow_head(net)
