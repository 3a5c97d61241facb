"""RAFT's training step (RAFT/train.py:79-86, :168-181): the optimizer tail - clip_grad_norm_, AdamW.step, OneCycleLR.step - with the clip and
the update fused in HIP (mpf_optim.hip), and the step from an OnlinePairs batch to updated weights.

    from mpiflow_amd.raft import RAFT
    from mpiflow_amd.raft_train import fetch_optimizer, train_step
    model = RAFT(args).cuda().train()
    optimizer, scheduler = fetch_optimizer(args, model)                  # args.lr, args.wdecay, args.epsilon, args.clip, args.num_steps
    for batch in pairs:                                                  # OnlinePairs: image1, image2, flow, valid on the GPU
        loss, metrics, total_norm = train_step(model, optimizer, scheduler, batch, iters=args.iters, gamma=args.gamma)

ClippedAdamW is torch.optim.AdamW with the gradient clipping of train.py:178 inside its step: the global norm over every parameter group
(fp64 sums in a fixed order, no atomics), the clip coefficient and the update are two kernels and a finish kernel over all parameters, with no
host synchronisation; results are bit-identical from run to run.  Its state_dict() is torch.optim.AdamW's key for key - per parameter `step`
(a CPU float32 scalar tensor), `exp_avg`, `exp_avg_sq`; the same param_groups keys plus `clip` - so a checkpoint moves between the two classes
in either direction.  torch's schedulers drive param_groups[...]['lr'] as a host float.

What differs from clip_grad_norm_ + AdamW.step: `p.grad` is NOT scaled in place (the clipped gradient exists only in registers); step()
returns total_norm, the norm before clipping, as a [1] device tensor (also kept as `last_grad_norm`), not the closure's loss; step(zero_grad=True)
writes zeros to every gradient it consumed, in the same pass, so the next backward accumulates into the same memory.  Non-finite gradients
propagate as upstream's do.  Refused at construction: amsgrad, maximize, parameters that are not dense float32 tensors on one GPU.

Reproducible runs.  Every kernel of this package on the step's path sums in a fixed order, but the library convolutions' backward does not
by default: its weight and input gradients differ in their last bits from call to call, and AdamW turns such a difference around zero into
a step of either sign.  `with reproducible():` around the loop (torch.backends.cudnn.deterministic = True, which torch hands to the
convolution library as its deterministic attribute) makes two runs from the same bytes agree bit for bit; it may select slower convolutions.

Not here: --add_noise, DataParallel and any multi-GPU gradient exchange, mixed_precision / GradScaler (the modules are float32 only),
checkpoint files, logging, the dataset readers.
"""
import contextlib

import torch

from . import ops
from ._lib import MpiFlowHipError
from .raft_upsample import sequence_loss


class ClippedAdamW(torch.optim.Optimizer):
    """ClippedAdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, clip=1.0): clip_grad_norm_(all parameters, clip), then
    torch.optim.AdamW's update.  clip=float('inf'): no clipping.  `clip` may differ between parameter groups; the norm is always global."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, clip=1.0, amsgrad=False, maximize=False):
        who = "ClippedAdamW"
        if amsgrad:
            raise MpiFlowHipError("%s: amsgrad=True is not supported (the fused update keeps no running maximum)" % who)
        if maximize:
            raise MpiFlowHipError("%s: maximize=True is not supported" % who)
        # torch.optim.AdamW's own defaults, key for key, so that param_groups - and with them state_dict() - carry what its load_state_dict reads
        defaults = dict(torch.optim.AdamW([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, clip=clip)
        self.last_grad_norm = None
        super().__init__(params, defaults)

    @staticmethod
    def _check_group(group, who="ClippedAdamW"):
        lr, (beta1, beta2), eps, wd, clip = group["lr"], group["betas"], group["eps"], group["weight_decay"], group["clip"]
        if isinstance(lr, torch.Tensor):
            raise MpiFlowHipError("%s: lr must be a Python float (a tensor lr would cost a synchronisation per step)" % who)
        if not lr >= 0.0:
            raise MpiFlowHipError("%s: invalid learning rate: %r" % (who, lr))
        if not eps > 0.0:
            raise MpiFlowHipError("%s: eps must be positive (got %r)" % (who, eps))
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise MpiFlowHipError("%s: the betas must lie in [0, 1) (got %r)" % (who, (beta1, beta2)))
        if not wd >= 0.0:
            raise MpiFlowHipError("%s: invalid weight_decay: %r" % (who, wd))
        if not clip > 0.0:
            raise MpiFlowHipError("%s: clip must be positive, float('inf') for no clipping (got %r)" % (who, clip))
        if group.get("amsgrad") or group.get("maximize"):
            raise MpiFlowHipError("%s: amsgrad and maximize are not supported (got amsgrad=%r, maximize=%r)" % (who, group.get("amsgrad"), group.get("maximize")))

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        who = "ClippedAdamW"
        group = self.param_groups[-1]
        self._check_group(group)
        # the tensor contract's order: type (Optimizer has checked it), dtype, layout; the device last
        for i, p in enumerate(group["params"]):
            if p.dtype != torch.float32:
                raise MpiFlowHipError("%s: parameter %d of group %d must be float32 (got %s); the kernels are float32 only" % (who, i, len(self.param_groups) - 1, p.dtype))
            if p.is_sparse or p.layout != torch.strided:
                raise MpiFlowHipError("%s: parameter %d of group %d must be a dense tensor (got layout %s)" % (who, i, len(self.param_groups) - 1, p.layout))
            if not p.is_contiguous():
                raise MpiFlowHipError("%s: parameter %d of group %d must be contiguous (got shape %s with strides %s)"
                                      % (who, i, len(self.param_groups) - 1, tuple(p.shape), p.stride()))
        first = self.param_groups[0]["params"][0]
        for g, grp in enumerate(self.param_groups):
            for i, p in enumerate(grp["params"]):
                if not p.is_cuda:
                    raise MpiFlowHipError("%s: parameter %d of group %d must live on the GPU (got %s); mpiflow_amd has no CPU path" % (who, i, g, p.device))
                if p.device != first.device:
                    raise MpiFlowHipError("%s: parameter %d of group %d is on %s, the first one on %s: the norm is global, so all parameters must "
                                          "share one device" % (who, i, g, p.device, first.device))

    def load_state_dict(self, state_dict):
        """torch.optim.AdamW's state dict, or this class's: `clip` is kept from this optimizer where the loaded groups have none"""
        clips = [g["clip"] for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, clip in zip(self.param_groups, clips):
            g.setdefault("clip", clip)
            self._check_group(g, "ClippedAdamW.load_state_dict")
        for state in self.state.values():                                # a fused or capturable AdamW keeps `step` on the device
            if "step" in state:
                state["step"] = torch.as_tensor(state["step"], dtype=torch.float32).cpu()

    @torch.no_grad()
    def step(self, closure=None, zero_grad=False):
        """One update of every parameter that has a gradient -> total_norm, the global gradient norm before clipping, a [1] float32 device
        tensor (no synchronisation).  closure: called first, with gradients enabled, as torch's optimizers do; its value is dropped.
        zero_grad=True: every consumed gradient is left all-zero at its address (a parameter without a gradient stays without one)."""
        who = "ClippedAdamW.step"
        if closure is not None:
            with torch.enable_grad():
                closure()
        # one call per (group, step number): parameters of one group differ in their step number only if some have skipped updates
        calls = {}
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise MpiFlowHipError("%s: sparse gradients are not supported (a parameter of shape %s has one)" % (who, tuple(p.shape)))
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)           # torch's default: a CPU scalar, never read by a kernel
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["step"] += 1
                t = int(state["step"])                                               # a host tensor: no synchronisation
                cols = calls.get((gi, t))
                if cols is None:
                    cols = calls[(gi, t)] = ([], [], [], [])
                cols[0].append(p), cols[1].append(g), cols[2].append(state["exp_avg"]), cols[3].append(state["exp_avg_sq"])
        if not calls:
            dev = self.param_groups[0]["params"][0].device
            self.last_grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)    # clip_grad_norm_ without gradients: 0
            return self.last_grad_norm
        norm = None
        if len(calls) > 1:
            norm = ops.grad_norm([g for cols in calls.values() for g in cols[1]], keep_workspace=True)
        total = None
        for (gi, t), (ps, gs, ms, vs) in calls.items():
            group = self.param_groups[gi]
            total = ops.adamw_clipped(ps, gs, ms, vs, lr=group["lr"], betas=group["betas"], eps=group["eps"], weight_decay=group["weight_decay"], step=t,
                                      max_norm=group["clip"], zero_grad=zero_grad, norm=norm)
        self.last_grad_norm = total if norm is None else norm[0]
        return self.last_grad_norm


@contextlib.contextmanager
def reproducible():
    """Inside the block the library convolutions, forward and backward, use only their deterministic algorithms
    (torch.backends.cudnn.deterministic = True; the setting before is restored on the way out).  With it two training runs from the same
    bytes on the same batches give the same bytes: the rest of train_step is order-stable as it is."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = before


def fetch_optimizer(args, model):
    """train.py:79-86 with ClippedAdamW: the optimizer over model.parameters() (args.lr, args.wdecay, args.epsilon, and args.clip, which
    train.py hands to clip_grad_norm_) and upstream's OneCycleLR (args.lr, args.num_steps + 100 steps, pct_start=0.05, linear, no momentum
    cycling) -> (optimizer, scheduler)"""
    optimizer = ClippedAdamW(model.parameters(), lr=args.lr, weight_decay=args.wdecay, eps=args.epsilon, clip=args.clip)
    scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer, args.lr, args.num_steps + 100, pct_start=0.05, cycle_momentum=False, anneal_strategy="linear")
    return optimizer, scheduler


def train_step(model, optimizer, scheduler, batch, iters=12, gamma=0.8):
    """One iteration of train.py's loop on an OnlinePairs batch (a mapping with image1, image2 [N,3,H,W] in 0..255, flow [N,2,H,W], valid
    [N,H,W], float32 on the GPU): the forward pass on the coarse outputs (coarse=True, or coarse="flow" for the small model), the fused
    sequence loss, backward, ClippedAdamW.step(zero_grad=True), scheduler.step() -> (loss, metrics, total_norm): the loss as a 0-d device
    tensor, sequence_loss's metrics, the gradient norm before clipping as a [1] device tensor.  Nothing here reads a device value; the one
    device-to-host copy of a step is sequence_loss's five metric numbers.  The first call may find `p.grad is None`; later calls find the
    zeroed gradients of the call before at the same addresses, so there is no optimizer.zero_grad() in the loop."""
    if not isinstance(optimizer, ClippedAdamW):
        raise MpiFlowHipError("train_step: optimizer must be a ClippedAdamW, whose step clips and zeroes the gradients (got %s); see fetch_optimizer"
                              % type(optimizer).__name__)
    small = bool(model.args.small)
    out = model(batch["image1"], batch["image2"], iters=iters, coarse="flow" if small else True)
    if small:
        loss, metrics = sequence_loss(out, None, batch["flow"], batch["valid"], gamma)
    else:
        loss, metrics = sequence_loss([f for f, _ in out], [m for _, m in out], batch["flow"], batch["valid"], gamma)
    loss.backward()
    total_norm = optimizer.step(zero_grad=True)
    scheduler.step()
    return loss.detach(), metrics, total_norm
