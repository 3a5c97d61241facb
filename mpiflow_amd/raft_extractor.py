"""RAFT's feature and context encoders on the GPU (RAFT/core/extractor.py): ResidualBlock, BottleneckBlock, BasicEncoder and SmallEncoder with
everything between their convolutions - normalise, ReLU, add the shortcut, ReLU - fused in HIP.

    from mpiflow_amd.raft_extractor import BasicEncoder, SmallEncoder         # RAFT/core/raft.py as written, only this import changes

Constructor signatures, the initialisation rule, parameter and buffer names and shapes are the reference's - `norm3` / `norm4` of a strided
block is registered a second time as `downsample.1`, as there - so a RAFT checkpoint loads with load_state_dict(strict=True).  The
nn.BatchNorm2d / nn.GroupNorm / nn.InstanceNorm2d submodules HOLD the parameters and running statistics and are never called; what they would
compute is part of the fused kernels.  They are real instances, so RAFT.freeze_bn (an isinstance walk that calls .eval()) works unchanged:
a BatchNorm2d in eval mode normalises with its running statistics and updates nothing.

What runs.  Per convolution output one autograd node: mpf_norm_stats (mean and centred sum of squares per plane chunk; none for 'none' and a
BatchNorm in eval mode) and mpf_norm_act, which merges them and writes relu(norm(x)) - or, at the end of a block, relu(shortcut + relu(norm(x)))
with the shortcut either the block's input or, in a strided block, norm(conv1x1(input)) read as a second term: one pass over two inputs.
Backward is mpf_norm_act_backward_reduce and mpf_norm_act_backward, which recompute both ReLU masks.  A node saves the convolution outputs it
read, mean / rstd per statistic set and - through the next convolution - its output; no normalised tensor, no mask, no sum is kept.  A
BatchNorm2d in training mode gets its running statistics updated as torch does (momentum, unbiased variance, num_batches_tracked).  The
convolutions are torch's (MIOpen), and so is Dropout2d.

The gradient of an identity shortcut is written to a tensor of its own and added to the first convolution's input gradient by autograd
(ops.norm_act_backward can add into a given buffer, but that gradient does not exist yet when the block's tail runs its backward).

Limits: inputs are held to the contract of _tensors.py: float32 only (the refusal says to call `.float()`), on the GPU, the
device judged last - with one difference: non-contiguous input is made contiguous, not refused.  A training-mode instance or
batch norm over a single value per statistic set is refused, as torch refuses it.  Nothing runs on the CPU and there is no eager fallback:
MpiFlowHipError.  Double backward is refused.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import ops
from ._lib import MpiFlowHipError
from ._tensors import check_devices, check_tensor

NORM_FNS = ("group", "batch", "instance", "none")


def _make_norm(norm_fn, channels, groups, who):
    if norm_fn == "group":
        return nn.GroupNorm(num_groups=groups, num_channels=channels)
    if norm_fn == "batch":
        return nn.BatchNorm2d(channels)
    if norm_fn == "instance":
        return nn.InstanceNorm2d(channels)
    if norm_fn == "none":
        return nn.Sequential()
    raise MpiFlowHipError("%s: norm_fn must be one of %s (got %r)" % (who, ", ".join(NORM_FNS), norm_fn))


def _mode(norm):
    """the kernel's mode for a holder module in its present state"""
    if isinstance(norm, nn.GroupNorm):
        return "group"
    if isinstance(norm, nn.BatchNorm2d):
        return "batch_train" if norm.training or norm.running_mean is None else "batch_eval"
    if isinstance(norm, nn.InstanceNorm2d):
        return "instance"
    return "none"


def _term(x, norm, mode=None, mean=None, rstd=None):
    """the kernel's term for x and its holder module; backward passes the mode the forward pass saw, not the holder's present state, and the
    statistics that pass saved"""
    mode = _mode(norm) if mode is None else mode
    if mode == "none":
        return ops.NormTerm(x, "none")
    term = ops.NormTerm(x, mode, weight=getattr(norm, "weight", None), bias=getattr(norm, "bias", None), groups=getattr(norm, "num_groups", 1),
                        running_mean=norm.running_mean if mode == "batch_eval" else None, running_var=norm.running_var if mode == "batch_eval" else None)
    term.mean, term.rstd = mean, rstd
    return term


def _update_running(norm, term, count):
    """nn.BatchNorm2d's bookkeeping in training mode, from the mean and biased variance the kernel wrote: a few ops on [C] tensors"""
    if norm.running_mean is None:
        return
    if norm.num_batches_tracked is not None:
        norm.num_batches_tracked += 1
    momentum = norm.momentum if norm.momentum is not None else 1.0 / float(norm.num_batches_tracked)
    norm.running_mean.mul_(1.0 - momentum).add_(term.mean, alpha=momentum)
    norm.running_var.mul_(1.0 - momentum).add_(term.var * (count / (count - 1.0)), alpha=momentum)


class _NormAct(torch.autograd.Function):
    """out = relu(norm(x)), relu(res + relu(norm(x))) or relu(rnorm(rx) + relu(norm(x))); norm and rnorm are the holder modules, which are read
    (mode, parameters, running statistics) and, a BatchNorm2d in training mode, updated, but never called."""

    @staticmethod
    def forward(ctx, norm, rnorm, x, weight, bias, res, rx, rweight, rbias):
        x = x.contiguous()
        term = _term(x, norm)
        rterm = _term(rx.contiguous(), rnorm) if rx is not None else None
        res = res.contiguous() if rx is None and res is not None else None
        out = ops.norm_act(term, rterm if rterm is not None else res)
        count = x.shape[0] * x.shape[2] * x.shape[3]
        stats = []
        for t, holder in ((term, norm), (rterm, rnorm)):
            if t is not None and t.mode == "batch_train":
                _update_running(holder, t, count)
            stats += [None, None] if t is None else [t.mean, t.rstd]
        ctx.holders = (norm, rnorm, term.mode, None if rterm is None else rterm.mode)
        ctx.save_for_backward(x, res, None if rterm is None else rterm.x, *stats)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, res, rx, mean, rstd, rmean, rrstd = ctx.saved_tensors
        norm, rnorm, mode, rmode = ctx.holders
        term = _term(x, norm, mode, mean, rstd)
        residual = _term(rx, rnorm, rmode, rmean, rrstd) if rx is not None else res
        needs = ctx.needs_input_grad
        dx, dw, db, dr = ops.norm_act_backward(grad_out.contiguous(), term, residual, param_grads=any(needs[3:5]) or any(needs[7:9]))
        drx = drw = drb = dres = None
        if rx is not None:
            drx, drw, drb = dr
        else:
            dres = dr
        return None, None, dx, dw, db, dres, drx, drw, drb


def _fused(x, norm, res=None, rx=None, rnorm=None):
    if rx is not None and _mode(rnorm) == "none":
        res, rx, rnorm = rx, None, None
    p = lambda m, name: getattr(m, name, None) if m is not None and _mode(m) != "none" else None
    return _NormAct.apply(norm, rnorm, x, p(norm, "weight"), p(norm, "bias"), res, rx, p(rnorm, "weight"), p(rnorm, "bias"))


def _contiguous(x):
    """a module input is made contiguous where it is not (the module docstring promises it); the contract of _tensors only checks"""
    return x.contiguous() if isinstance(x, torch.Tensor) else x


def _conv_out(size, conv, axis):
    return (size + 2 * conv.padding[axis] - conv.kernel_size[axis]) // conv.stride[axis] + 1


def _refuse_single(norm, N, H, W, who, name):
    """torch raises for training-mode batch / instance statistics over one value; say so before anything runs"""
    mode = _mode(norm)
    if (mode == "instance" and H * W == 1) or (mode == "batch_train" and N * H * W == 1):
        raise MpiFlowHipError("%s: %s would take '%s' statistics over a single value (its input is %dx%dx%d, N x H x W): use a larger input, or "
                              "eval mode with running statistics for a BatchNorm" % (who, name, mode, N, H, W))


class _Block(nn.Module):
    """What both block classes share: the holder modules in the reference's registration order, and the shape walk."""

    def _finish(self, in_planes, planes, norm_fn, stride, groups, last):
        who = type(self).__name__
        if stride != 1:
            setattr(self, last, _make_norm(norm_fn, planes, groups, who))
            self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, kernel_size=1, stride=stride), getattr(self, last))
        else:
            self.downsample = None
        self.norm_fn = norm_fn

    def _walk(self, N, H, W, who):
        """output (H, W); refuses a single-valued statistic set on the way"""
        for conv, norm, name in self._chain():
            H, W = _conv_out(H, conv, 0), _conv_out(W, conv, 1)
            _refuse_single(norm, N, H, W, who, name)
        return H, W

    def _check(self, x):
        who = type(self).__name__
        x = check_tensor(_contiguous(x), "x", who, 4, "[N,C,H,W]")
        if x.shape[1] != self.conv1.in_channels:
            raise MpiFlowHipError("%s: x must have %d channels (got shape %s)" % (who, self.conv1.in_channels, tuple(x.shape)))
        self._walk(x.shape[0], x.shape[2], x.shape[3], who)
        check_devices(who, dict(x=x))
        return x


class ResidualBlock(_Block):
    """RAFT/core/extractor.py's ResidualBlock: ResidualBlock(in_planes, planes, norm_fn='group', stride=1)(x) -> [N,planes,H/stride,W/stride].
    Two 3 x 3 convolutions, two fused tails.  See the module docstring."""

    def __init__(self, in_planes, planes, norm_fn="group", stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1)
        groups = planes // 8
        self.norm1 = _make_norm(norm_fn, planes, groups, "ResidualBlock")
        self.norm2 = _make_norm(norm_fn, planes, groups, "ResidualBlock")
        self._finish(in_planes, planes, norm_fn, stride, groups, "norm3")

    def _chain(self):
        return [(self.conv1, self.norm1, "norm1"), (self.conv2, self.norm2, "norm2")]

    def forward(self, x):
        x = self._check(x)
        y = _fused(self.conv1(x), self.norm1)
        if self.downsample is None:
            return _fused(self.conv2(y), self.norm2, res=x)
        return _fused(self.conv2(y), self.norm2, rx=self.downsample[0](x), rnorm=self.norm3)


class BottleneckBlock(_Block):
    """RAFT/core/extractor.py's BottleneckBlock: 1 x 1 to planes/4, 3 x 3 (strided), 1 x 1 to planes; three fused tails."""

    def __init__(self, in_planes, planes, norm_fn="group", stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes // 4, kernel_size=1, padding=0)
        self.conv2 = nn.Conv2d(planes // 4, planes // 4, kernel_size=3, padding=1, stride=stride)
        self.conv3 = nn.Conv2d(planes // 4, planes, kernel_size=1, padding=0)
        groups = planes // 8
        self.norm1 = _make_norm(norm_fn, planes // 4, groups, "BottleneckBlock")
        self.norm2 = _make_norm(norm_fn, planes // 4, groups, "BottleneckBlock")
        self.norm3 = _make_norm(norm_fn, planes, groups, "BottleneckBlock")
        self._finish(in_planes, planes, norm_fn, stride, groups, "norm4")

    def _chain(self):
        return [(self.conv1, self.norm1, "norm1"), (self.conv2, self.norm2, "norm2"), (self.conv3, self.norm3, "norm3")]

    def forward(self, x):
        x = self._check(x)
        y = _fused(self.conv1(x), self.norm1)
        y = _fused(self.conv2(y), self.norm2)
        if self.downsample is None:
            return _fused(self.conv3(y), self.norm3, res=x)
        return _fused(self.conv3(y), self.norm3, rx=self.downsample[0](x), rnorm=self.norm4)


class _Encoder(nn.Module):
    """What both encoders share.  STEM: channels after conv1; DIMS: the three stages; BLOCK: their block class."""
    STEM, DIMS, BLOCK = 0, (), None

    def __init__(self, output_dim=128, norm_fn="batch", dropout=0.0):
        super().__init__()
        who = type(self).__name__
        self.norm_fn = norm_fn
        self.norm1 = _make_norm(norm_fn, self.STEM, 8, who)
        self.conv1 = nn.Conv2d(3, self.STEM, kernel_size=7, stride=2, padding=3)
        self.in_planes = self.STEM
        self.layer1 = self._make_layer(self.DIMS[0], stride=1)
        self.layer2 = self._make_layer(self.DIMS[1], stride=2)
        self.layer3 = self._make_layer(self.DIMS[2], stride=2)
        self._tail(output_dim, dropout)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.InstanceNorm2d, nn.GroupNorm)):
                if m.weight is not None:
                    nn.init.constant_(m.weight, 1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def _make_layer(self, dim, stride=1):
        layers = (self.BLOCK(self.in_planes, dim, self.norm_fn, stride=stride), self.BLOCK(dim, dim, self.norm_fn, stride=1))
        self.in_planes = dim
        return nn.Sequential(*layers)

    def forward(self, x):
        who = type(self).__name__
        is_list = isinstance(x, (tuple, list))
        if is_list:
            if len(x) != 2:
                raise MpiFlowHipError("%s: a list input must hold two image batches (got %d)" % (who, len(x)))
            x = [check_tensor(_contiguous(t), "x[%d]" % k, who, 4, "[N,C,H,W]") for k, t in enumerate(x)]
            if x[0].shape != x[1].shape or x[0].device != x[1].device:
                raise MpiFlowHipError("%s: the two image batches must share shape and device (got %s on %s, %s on %s)"
                                      % (who, tuple(x[0].shape), x[0].device, tuple(x[1].shape), x[1].device))
            batch_dim = x[0].shape[0]
            x = torch.cat(x, dim=0)
        x = check_tensor(_contiguous(x), "x", who, 4, "[N,C,H,W]")
        if x.shape[1] != 3:
            raise MpiFlowHipError("%s: x must have 3 channels (got shape %s)" % (who, tuple(x.shape)))
        N, H, W = x.shape[0], _conv_out(x.shape[2], self.conv1, 0), _conv_out(x.shape[3], self.conv1, 1)
        _refuse_single(self.norm1, N, H, W, who, "norm1")
        for layer in (self.layer1, self.layer2, self.layer3):
            for blk in layer:
                H, W = blk._walk(N, H, W, who)
        check_devices(who, dict(x=x))
        x = _fused(self.conv1(x), self.norm1)
        x = self.layer3(self.layer2(self.layer1(x)))
        x = self.conv2(x)
        if self.training and self.dropout is not None:
            x = self.dropout(x)
        if is_list:
            x = torch.split(x, [batch_dim, batch_dim], dim=0)
        return x


class BasicEncoder(_Encoder):
    """RAFT/core/extractor.py's BasicEncoder: BasicEncoder(output_dim=128, norm_fn='batch', dropout=0.0)(x) -> [N,output_dim,H/8,W/8]; x is
    [N,3,H,W] or a list / tuple of two such batches (then a tuple of two comes back).  7 x 7 stem, six ResidualBlocks (64, 96, 128), 1 x 1
    output convolution.  RAFT's fnet is BasicEncoder(256, 'instance'), its cnet BasicEncoder(hidden + context, 'batch')."""
    STEM, DIMS, BLOCK = 64, (64, 96, 128), ResidualBlock

    def _tail(self, output_dim, dropout):
        self.conv2 = nn.Conv2d(128, output_dim, kernel_size=1)
        self.dropout = nn.Dropout2d(p=dropout) if dropout > 0 else None


class SmallEncoder(_Encoder):
    """RAFT/core/extractor.py's SmallEncoder: as BasicEncoder with a 32-channel stem and six BottleneckBlocks (32, 64, 96)."""
    STEM, DIMS, BLOCK = 32, (32, 64, 96), BottleneckBlock

    def _tail(self, output_dim, dropout):
        self.dropout = nn.Dropout2d(p=dropout) if dropout > 0 else None
        self.conv2 = nn.Conv2d(96, output_dim, kernel_size=1)
