"""RAFT itself (RAFT/core/raft.py), basic and small, assembled from this package's modules: BasicEncoder / SmallEncoder (raft_extractor),
CorrBlock / AlternateCorrBlock (raft_corr), BasicUpdateBlock / SmallUpdateBlock (raft_update), upsample_flow / upflow8 (raft_upsample), and
the glue between them in HIP (mpf_raft_glue.hip).

    from mpiflow_amd.raft import RAFT                                    # instead of `from raft import RAFT`
    model = RAFT(args)                                                   # args.small, args.mixed_precision (must be False), optionally
    model.load_checkpoint("models/raft-things.pth")                      # args.dropout and args.alternate_corr, as upstream

Constructor, attributes (fnet, cnet, update_block, hidden_dim, context_dim), freeze_bn, initialize_flow, upsample_flow and the signature and
return values of forward are upstream's; the constructor sets args.corr_levels / args.corr_radius / args.dropout / args.alternate_corr as
upstream's does.  state_dict() is the reference's key for key and shape for shape, so its checkpoints load with strict=True (load_checkpoint
strips the `module.` prefix nn.DataParallel leaves).

What differs from upstream.  (1) The glue is three kernels: both images are scaled straight into the [2N,3,H,W] batch fnet consumes, whose
first half cnet consumes (mpf_raft_images; no cat); tanh / relu of the context network's output are one launch each way and the split's
gradient is written as one tensor (mpf_context_split); the small model upsamples with mpf_upflow8, a gather in backward.  The per-iteration
coords1 - coords0 and coords1 + delta_flow stay torch's.  (2) forward takes one more keyword: coarse=True (basic model, not test_mode) returns
per iteration the pair (coords1 - coords0, up_mask) instead of the upsampled prediction - what raft_upsample.sequence_loss takes, which then
never writes a full-resolution prediction; coarse="flow" (small model, not test_mode) returns per iteration coords1 - coords0 [N,2,H/8,W/8]
alone and upsamples nothing - what raft_upsample.sequence_loss(flows, None, ...) takes, which forms upflow8's prediction in registers.
(3) In test_mode only the last iteration is upsampled (the others' upsampled flows are dropped upstream too).  (4) Refused instead of computed: mixed_precision=True (the modules are float32 only); frames whose sides are not multiples of
8 (upstream pads them first: utils.InputPadder) or are below 8 * 2^corr_levels = 128 (there the reference's sampler divides by zero at the
coarsest level and every prediction is NaN).

Beside forward: predict(image1, image2, iters=12, flow_init=None, mode='sintel', warm_start=None) is evaluate.py's pad / forward(test_mode=True)
/ unpad for frames of any size, with the padding fused into the image scaling and the last prediction written as its unpadded window
(raft_eval.py); warm_start, the previous pair's flow_low, is pushed forward along itself on the device (ops.forward_interpolate) and used as
flow_init: upstream's video recipe.

Limits: the contract of _tensors.py: float32 images on the GPU, checked in its order (type, dtype, shape, what the call
requires, the device last); non-contiguous images are made contiguous, as upstream does.  No CPU path, no eager fallback: MpiFlowHipError.
"""
import torch
import torch.nn as nn

from . import ops
from ._lib import MpiFlowHipError
from ._tensors import check_devices, check_tensor
from .raft_corr import AlternateCorrBlock, CorrBlock
from .raft_eval import InputPadder
from .raft_extractor import BasicEncoder, SmallEncoder
from .raft_update import BasicUpdateBlock, SmallUpdateBlock
from .raft_upsample import upflow8, upsample_flow


class _ContextSplit(torch.autograd.Function):
    """(net, inp) = (tanh(cnet[:, :hdim]), relu(cnet[:, hdim:])); backward needs only the two outputs"""

    @staticmethod
    def forward(ctx, cnet, hdim):
        net, inp = ops.context_split(cnet, hdim)
        ctx.save_for_backward(net, inp)
        return net, inp

    @staticmethod
    def backward(ctx, g_net, g_inp):
        net, inp = ctx.saved_tensors
        return ops.context_split_backward(net, inp, g_net.contiguous(), g_inp.contiguous()), None


def context_split(cnet, hdim):
    """RAFT.forward's `net, inp = torch.split(cnet, [hdim, cdim], dim=1); net = tanh(net); inp = relu(inp)`: cnet [N,hdim+cdim,H,W] ->
    (net, inp), contiguous, differentiable.  Non-contiguous input is made contiguous."""
    return _ContextSplit.apply(cnet.contiguous() if isinstance(cnet, torch.Tensor) else cnet, int(hdim))


def coords_grid(batch, ht, wd, device):
    """upstream's utils.coords_grid: [batch,2,ht,wd] float32, channel 0 the x index, channel 1 the y index"""
    ys, xs = torch.meshgrid(torch.arange(ht, device=device), torch.arange(wd, device=device), indexing="ij")
    return torch.stack([xs, ys], dim=0).float()[None].repeat(batch, 1, 1, 1)


class RAFT(nn.Module):
    """RAFT/core/raft.py's RAFT: RAFT(args)(image1, image2, iters=12, flow_init=None, upsample=True, test_mode=False) -> the list of
    upsampled predictions [N,2,H,W], or in test_mode (coords1 - coords0, flow_up).  image1, image2 [N,3,H,W] float32 in 0..255 on the GPU, H and
    W multiples of 8 and at least 128; flow_init [N,2,H/8,W/8].  coarse=True (basic) / coarse="flow" (small): see the module docstring."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        if getattr(args, "mixed_precision", False):
            raise MpiFlowHipError("RAFT: mixed_precision=True is not supported: this package's modules are float32 only (construct with "
                                  "mixed_precision=False; a half-precision checkpoint loads after .float())")
        if args.small:
            self.hidden_dim = hdim = 96
            self.context_dim = cdim = 64
            args.corr_levels = 4
            args.corr_radius = 3
        else:
            self.hidden_dim = hdim = 128
            self.context_dim = cdim = 128
            args.corr_levels = 4
            args.corr_radius = 4
        if not hasattr(args, "dropout"):
            args.dropout = 0
        if not hasattr(args, "alternate_corr"):
            args.alternate_corr = False
        if args.small:
            self.fnet = SmallEncoder(output_dim=128, norm_fn="instance", dropout=args.dropout)
            self.cnet = SmallEncoder(output_dim=hdim + cdim, norm_fn="none", dropout=args.dropout)
            self.update_block = SmallUpdateBlock(self.args, hidden_dim=hdim)
        else:
            self.fnet = BasicEncoder(output_dim=256, norm_fn="instance", dropout=args.dropout)
            self.cnet = BasicEncoder(output_dim=hdim + cdim, norm_fn="batch", dropout=args.dropout)
            self.update_block = BasicUpdateBlock(self.args, hidden_dim=hdim)

    def load_checkpoint(self, path_or_dict):
        """Load a RAFT checkpoint - a path torch.load reads, or a state dict - with strict=True; the `module.` prefix of a checkpoint saved
        from nn.DataParallel (all of upstream's are) is stripped.  Returns self."""
        state = torch.load(path_or_dict, map_location="cpu") if isinstance(path_or_dict, (str, bytes)) or hasattr(path_or_dict, "__fspath__") else path_or_dict
        if not hasattr(state, "items"):
            raise MpiFlowHipError("RAFT.load_checkpoint: expected a path or a state dict (got %s)" % type(state).__name__)
        self.load_state_dict({(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}, strict=True)
        return self

    def freeze_bn(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()

    def initialize_flow(self, img):
        """Flow is represented as difference between two coordinate grids: flow = coords1 - coords0"""
        N, C, H, W = img.shape
        coords0 = coords_grid(N, H // 8, W // 8, device=img.device)
        coords1 = coords_grid(N, H // 8, W // 8, device=img.device)
        return coords0, coords1

    def upsample_flow(self, flow, mask):
        """Upsample flow field [H/8, W/8, 2] -> [H, W, 2] using convex combination (raft_upsample.upsample_flow)"""
        return upsample_flow(flow, mask)

    def _check(self, image1, image2, flow_init, test_mode, coarse):
        """the refusals, in the order of _tensors.py; returns the images, contiguous"""
        who = "RAFT"
        contiguous = lambda t: t.contiguous() if isinstance(t, torch.Tensor) else t
        image1 = check_tensor(contiguous(image1), "image1", who, (None, 3, None, None), "[N,3,H,W]")
        N, _, H, W = image1.shape
        image2 = check_tensor(contiguous(image2), "image2", who, (N, 3, H, W), "[N,3,H,W] like image1")
        if H % 8 or W % 8:
            raise MpiFlowHipError("%s: the frame's H and W must be multiples of 8 (got %d x %d; pad it first, as upstream's InputPadder does)" % (who, H, W))
        side = 8 * 2 ** self.args.corr_levels
        if H < side or W < side:
            raise MpiFlowHipError("%s: the frame must be at least %d x %d (got %d x %d): at 1/8 resolution every one of the %d correlation levels "
                                  "needs 2 x 2 cells" % (who, side, side, H, W, self.args.corr_levels))
        tensors = dict(image1=image1, image2=image2)
        if flow_init is not None:
            tensors["flow_init"] = check_tensor(contiguous(flow_init), "flow_init", who, (N, 2, H // 8, W // 8), "[N,2,H/8,W/8]")
        if not isinstance(coarse, bool) and not (isinstance(coarse, str) and coarse == "flow"):
            raise MpiFlowHipError("%s: coarse must be False, True or \"flow\" (got %r)" % (who, coarse))
        if coarse is True and self.args.small:
            raise MpiFlowHipError("%s: coarse=True needs the basic model: the small one has no upsampling mask to hand to sequence_loss; "
                                  "coarse=\"flow\" returns its coarse flows for sequence_loss(flows, None, ...)" % who)
        if coarse == "flow" and not self.args.small:
            raise MpiFlowHipError("%s: coarse=\"flow\" is the small model's: the basic one has an upsampling mask, use coarse=True" % who)
        if coarse and test_mode:
            raise MpiFlowHipError("%s: coarse=%s returns the training list; it cannot be combined with test_mode=True" % (who, "True" if coarse is True else '"flow"'))
        check_devices(who, tensors)
        return image1, image2, tensors.get("flow_init")

    def forward(self, image1, image2, iters=12, flow_init=None, upsample=True, test_mode=False, coarse=False):
        """Estimate optical flow between pair of frames"""
        image1, image2, flow_init = self._check(image1, image2, flow_init, test_mode, coarse)
        pair = ops.raft_images(image1, image2)                  # [2N,3,H,W]: 2 * (x / 255) - 1, image1 first
        return self._refine(pair, iters, flow_init, test_mode, coarse)

    def _refine(self, pair, iters, flow_init, test_mode, coarse, crop=None):
        """forward from the prepared batch on: pair [2N,3,H,W], H and W multiples of 8.  crop (test_mode only): InputPadder._pad; the last
        prediction is then written as its unpadded window alone (ops.upsample_flow_crop / ops.upflow8_crop)."""
        N = pair.shape[0] // 2
        hdim = self.hidden_dim

        fmaps = self.fnet(pair)
        fmap1, fmap2 = fmaps[:N], fmaps[N:]
        if self.args.alternate_corr:
            corr_fn = AlternateCorrBlock(fmap1, fmap2, radius=self.args.corr_radius)
        else:
            corr_fn = CorrBlock(fmap1, fmap2, radius=self.args.corr_radius)

        net, inp = context_split(self.cnet(pair[:N]), hdim)

        coords0, coords1 = self.initialize_flow(pair[:N])
        if flow_init is not None:
            coords1 = coords1 + flow_init

        flow_predictions = []
        flow_up = None
        for itr in range(iters):
            coords1 = coords1.detach()
            corr = corr_fn(coords1)                             # index correlation volume
            flow = coords1 - coords0
            net, up_mask, delta_flow = self.update_block(net, inp, corr, flow)
            coords1 = coords1 + delta_flow                      # F(t+1) = F(t) + \Delta(t)
            if coarse:
                flow_predictions.append((coords1 - coords0, up_mask) if coarse is True else coords1 - coords0)
                continue
            if test_mode and itr < iters - 1:
                continue
            if crop is not None:
                flow_up = ops.upflow8_crop(coords1 - coords0, crop) if up_mask is None else ops.upsample_flow_crop(coords1 - coords0, up_mask.contiguous(), crop)
            elif up_mask is None:
                flow_up = upflow8(coords1 - coords0)
            else:
                flow_up = self.upsample_flow(coords1 - coords0, up_mask)
            flow_predictions.append(flow_up)

        if test_mode:
            return coords1 - coords0, flow_up
        return flow_predictions

    @torch.no_grad()
    def predict(self, image1, image2, iters=12, flow_init=None, mode="sintel", warm_start=None):
        """evaluate.py's `padder = InputPadder(image1.shape, mode); flow_low, flow_pr = model(*padder.pad(image1, image2), iters, flow_init,
        test_mode=True); flow_up = padder.unpad(flow_pr)` for frames of ANY size: -> (flow_low [N,2,Hp/8,Wp/8], flow_up [N,2,H,W]), Hp x Wp
        the padded frame.  The padded images, their cat, the padded prediction and its slice are never formed (ops.raft_images_padded,
        ops.upsample_flow_crop / ops.upflow8_crop).  flow_init [N,2,Hp/8,Wp/8].  warm_start [N,2,Hp/8,Wp/8]: the previous pair's flow_low;
        flow_init is then ops.forward_interpolate(warm_start), create_sintel_submission's warm start without its host round trip (give one
        of the two, not both).  The model must be in eval mode.  No gradients."""
        who = "RAFT.predict"
        contiguous = lambda t: t.contiguous() if isinstance(t, torch.Tensor) else t
        image1 = check_tensor(contiguous(image1), "image1", who, (None, 3, None, None), "[N,3,H,W]")
        N, _, H, W = image1.shape
        image2 = check_tensor(contiguous(image2), "image2", who, (N, 3, H, W), "[N,3,H,W] like image1")
        padder = InputPadder((H, W), mode)
        Hp, Wp = H + padder._pad[2] + padder._pad[3], W + padder._pad[0] + padder._pad[1]
        side = 8 * 2 ** self.args.corr_levels
        if Hp < side or Wp < side:
            raise MpiFlowHipError("%s: the padded frame must be at least %d x %d (got %d x %d, padded to %d x %d): at 1/8 resolution every one of "
                                  "the %d correlation levels needs 2 x 2 cells" % (who, side, side, H, W, Hp, Wp, self.args.corr_levels))
        tensors = dict(image1=image1, image2=image2)
        if flow_init is not None:
            tensors["flow_init"] = check_tensor(contiguous(flow_init), "flow_init", who, (N, 2, Hp // 8, Wp // 8), "[N,2,Hp/8,Wp/8] of the padded frame")
        if warm_start is not None:
            tensors["warm_start"] = check_tensor(contiguous(warm_start), "warm_start", who, (N, 2, Hp // 8, Wp // 8), "[N,2,Hp/8,Wp/8] of the padded frame")
        if flow_init is not None and warm_start is not None:
            raise MpiFlowHipError("%s: give flow_init or warm_start, not both: warm_start IS a flow_init, forward_interpolate(warm_start)" % who)
        if self.training:
            raise MpiFlowHipError("%s: the model is in training mode, where batch norm would update its running statistics during evaluation; "
                                  "call .eval() first" % who)
        check_devices(who, tensors)
        pair = padder.pair(image1, image2)                      # [2N,3,Hp,Wp]
        flow_init = tensors.get("flow_init") if warm_start is None else ops.forward_interpolate(tensors["warm_start"])
        return self._refine(pair, iters, flow_init, True, False, crop=padder._pad)
