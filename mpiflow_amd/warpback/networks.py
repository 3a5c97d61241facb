"""warpback/networks.py of the reference: the three EdgeConnect generators stage 2 inpaints with, for inference.

EdgeGenerator, InpaintGenerator and ResnetBlock take the reference's constructor arguments and hold the reference's module tree (encoder /
middle / decoder Sequentials with the same indices), so state_dict() has the published checkpoints' keys and shapes - the weight_orig,
weight_u and weight_v of nn.utils.spectral_norm included - and those files load with strict=True.

The convolutions and reflection pads are torch's (MIOpen).  forward walks the tree itself: a convolution followed by InstanceNorm2d and
ReLU hands its output to ops.norm_act in 'instance' mode without affine parameters (epsilon 1e-5, InstanceNorm2d's default), one launch
for the pair.  NOT fused: the tail of a ResnetBlock, x + InstanceNorm(conv(...)), which has no ReLU; the closing tanh / sigmoid.

fold_spectral_norm replaces every spectral-norm weight by weight_orig / (u . W v) once (what an eval-mode forward recomputes every time);
get_edge_connect calls it after loading.  No gradients: forward runs under torch.no_grad()."""
import os

import torch
import torch.nn as nn
from torch.nn.utils.spectral_norm import SpectralNorm

from .. import ops
from .._lib import MpiFlowHipError

CHECKPOINTS = ("EdgeModel_gen.pth", "InpaintingModel_gen.pth", "InpaintingModel_disp.pth")


def _sn(module, on):
    return nn.utils.spectral_norm(module) if on else module


def _in(ch):
    return nn.InstanceNorm2d(ch, track_running_stats=False)


def _run(seq, x):
    """nn.Sequential.forward with every conv -> InstanceNorm2d -> ReLU run as conv, then one ops.norm_act launch"""
    layers = list(seq)
    i = 0
    while i < len(layers):
        m = layers[i]
        fused = (isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)) and i + 2 < len(layers) and isinstance(layers[i + 1], nn.InstanceNorm2d)
                 and isinstance(layers[i + 2], nn.ReLU))
        if fused:
            n = layers[i + 1]
            if n.affine or n.track_running_stats or n.eps != 1e-5:
                raise MpiFlowHipError("networks: ops.norm_act's 'instance' mode is InstanceNorm2d without affine parameters or running statistics at eps 1e-5")
            x = ops.norm_act(ops.NormTerm(m(x).contiguous(), "instance"))
            i += 3
        else:
            x = m(x)
            i += 1
    return x


class BaseNetwork(nn.Module):
    def init_weights(self, init_type="normal", gain=0.02):
        """the reference's initialisation of Conv / Linear weights: normal | xavier | kaiming | orthogonal, biases zero"""
        fill = {"normal": lambda w: nn.init.normal_(w, 0.0, gain), "xavier": lambda w: nn.init.xavier_normal_(w, gain=gain),
                "kaiming": lambda w: nn.init.kaiming_normal_(w, a=0, mode="fan_in"), "orthogonal": lambda w: nn.init.orthogonal_(w, gain=gain)}

        def init_func(m):
            name = m.__class__.__name__
            if hasattr(m, "weight") and ("Conv" in name or "Linear" in name):
                if init_type in fill:
                    fill[init_type](m.weight.data)
                if getattr(m, "bias", None) is not None:
                    nn.init.constant_(m.bias.data, 0.0)
            elif "BatchNorm2d" in name:
                nn.init.normal_(m.weight.data, 1.0, gain)
                nn.init.constant_(m.bias.data, 0.0)
        self.apply(init_func)


def _trunk(in_channels, out_channels, residual_blocks, sn):
    """(encoder, middle, decoder): 7 x 7 stem, two stride-2 4 x 4 convolutions, dilated residual blocks, two transposed convolutions, 7 x 7 head"""
    encoder = nn.Sequential(
        nn.ReflectionPad2d(3), _sn(nn.Conv2d(in_channels, 64, kernel_size=7, padding=0), sn), _in(64), nn.ReLU(True),
        _sn(nn.Conv2d(64, 128, kernel_size=4, stride=2, padding=1), sn), _in(128), nn.ReLU(True),
        _sn(nn.Conv2d(128, 256, kernel_size=4, stride=2, padding=1), sn), _in(256), nn.ReLU(True))
    middle = nn.Sequential(*[ResnetBlock(256, 2, use_spectral_norm=sn) for _ in range(residual_blocks)])
    decoder = nn.Sequential(
        _sn(nn.ConvTranspose2d(256, 128, kernel_size=4, stride=2, padding=1), sn), _in(128), nn.ReLU(True),
        _sn(nn.ConvTranspose2d(128, 64, kernel_size=4, stride=2, padding=1), sn), _in(64), nn.ReLU(True),
        nn.ReflectionPad2d(3), nn.Conv2d(64, out_channels, kernel_size=7, padding=0))
    return encoder, middle, decoder


class InpaintGenerator(BaseNetwork):
    def __init__(self, residual_blocks=8, init_weights=True, in_channels=4, out_channels=3):
        super().__init__()
        self.encoder, self.middle, self.decoder = _trunk(in_channels, out_channels, residual_blocks, False)
        if init_weights:
            self.init_weights()

    @torch.no_grad()
    def forward(self, x):
        x = _run(self.decoder, _run(self.middle, _run(self.encoder, x)))
        return (torch.tanh(x) + 1) / 2


class EdgeGenerator(BaseNetwork):
    def __init__(self, residual_blocks=8, use_spectral_norm=True, init_weights=True):
        super().__init__()
        self.encoder, self.middle, self.decoder = _trunk(3, 1, residual_blocks, use_spectral_norm)
        if init_weights:
            self.init_weights()

    @torch.no_grad()
    def forward(self, x):
        return torch.sigmoid(_run(self.decoder, _run(self.middle, _run(self.encoder, x))))


class ResnetBlock(nn.Module):
    def __init__(self, dim, dilation=1, use_spectral_norm=False):
        super().__init__()
        bias = not use_spectral_norm
        self.conv_block = nn.Sequential(
            nn.ReflectionPad2d(dilation), _sn(nn.Conv2d(dim, dim, kernel_size=3, padding=0, dilation=dilation, bias=bias), use_spectral_norm),
            _in(dim), nn.ReLU(True),
            nn.ReflectionPad2d(1), _sn(nn.Conv2d(dim, dim, kernel_size=3, padding=0, dilation=1, bias=bias), use_spectral_norm), _in(dim))

    @torch.no_grad()
    def forward(self, x):
        return x + _run(self.conv_block, x)                      # the tail has no ReLU: torch's InstanceNorm2d and add


def fold_spectral_norm(module):
    """every nn.utils.spectral_norm weight of `module` becomes the plain parameter weight_orig / (u . W v), computed once without a power
    iteration - what the eval-mode forward computes on every call; weight_orig, weight_u and weight_v leave the state dict.  Returns module."""
    for m in module.modules():
        if any(isinstance(h, SpectralNorm) for h in m._forward_pre_hooks.values()):
            nn.utils.remove_spectral_norm(m)
    return module


def get_edge_connect(weight_dir):
    """(edge_model, inpaint_model, disp_model) from EdgeModel_gen.pth, InpaintingModel_gen.pth and InpaintingModel_disp.pth of weight_dir (each a
    dict whose "generator" entry is the state dict), in eval mode, spectral norm folded"""
    paths = [os.path.join(str(weight_dir), name) for name in CHECKPOINTS]
    missing = [p for p in paths if not os.path.isfile(p)]
    if missing:
        raise FileNotFoundError("get_edge_connect: no EdgeConnect checkpoints: looked for %s; missing %s.  They are not part of this repository; "
                                "pass models=(edge, inpaint, disp) to use generators of your own" % (", ".join(paths), ", ".join(missing)))
    models = [EdgeGenerator(), InpaintGenerator(), InpaintGenerator(in_channels=2, out_channels=1)]
    for model, path in zip(models, paths):
        model.load_state_dict(torch.load(path, map_location="cpu")["generator"], strict=True)
        model.eval()
        fold_spectral_norm(model)
    return tuple(models)
