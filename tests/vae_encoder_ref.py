"""fp32 CPU restatement of the SD1.5 AutoencoderKL encoder half (TEST REFERENCE ONLY).

diffusers==0.23.1 semantics (not installed here, so unpinned, like oracle/vae_ref.py's decoder): Encoder =
conv_in 3 -> 128, four DownEncoderBlock2D of two ResnetBlock2D (eps 1e-6, no time embedding; 128, 256, 512,
512 channels) with Downsample2D(padding=0) -- F.pad(x, (0, 1, 0, 1)) then a 3x3 stride-2 conv with padding 0 --
after the first three, UNetMidBlock2D(resnet, Attention(1 head, GroupNorm eps 1e-6, residual), resnet),
GroupNorm + SiLU, conv_out 512 -> 8; then quant_conv 8 -> 8 (1x1).  The moments are DiagonalGaussianDistribution's
(mean, logvar) = chunk(2, dim=1), logvar clamped to [-30, 20], std = exp(0.5 logvar); the pipeline scales the
sample (or the mode) by 0.18215.  A torch module with diffusers' parameter names, so its state dict is the
checkpoint key set.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

SCALING = 0.18215


class _Resnet(nn.Module):
    def __init__(self, cin, cout, groups):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, cin, eps=1e-6)
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1)
        self.norm2 = nn.GroupNorm(groups, cout, eps=1e-6)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1)

    def forward(self, x):
        h = self.conv1(F.silu(self.norm1(x)))
        h = self.conv2(F.silu(self.norm2(h)))
        if hasattr(self, "conv_shortcut"):
            x = self.conv_shortcut(x)
        return x + h


class _Downsample(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, stride=2, padding=0)

    def forward(self, x):
        return self.conv(F.pad(x, (0, 1, 0, 1)))


class _Attention(nn.Module):
    def __init__(self, c, groups):
        super().__init__()
        self.group_norm = nn.GroupNorm(groups, c, eps=1e-6)
        self.to_q, self.to_k, self.to_v = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)
        self.to_out = nn.ModuleList([nn.Linear(c, c)])

    def forward(self, x):
        b, c, h, w = x.shape
        y = self.group_norm(x).view(b, c, h * w).transpose(1, 2)
        p = torch.softmax(self.to_q(y) @ self.to_k(y).transpose(1, 2) / c ** 0.5, dim=-1)
        o = self.to_out[0](p @ self.to_v(y))
        return o.transpose(1, 2).reshape(b, c, h, w) + x


class _Block(nn.Module):
    pass


class VAEEncoderRef(nn.Module):
    def __init__(self, channels=(128, 256, 512, 512), layers=2, groups=32, latent=4):
        super().__init__()
        enc = _Block()
        enc.conv_in = nn.Conv2d(3, channels[0], 3, padding=1)
        enc.down_blocks = nn.ModuleList()
        out_c = channels[0]
        for i, c in enumerate(channels):
            prev, out_c = out_c, c
            blk = _Block()
            blk.resnets = nn.ModuleList([_Resnet(prev if j == 0 else out_c, out_c, groups) for j in range(layers)])
            if i < len(channels) - 1:
                blk.downsamplers = nn.ModuleList([_Downsample(out_c)])
            enc.down_blocks.append(blk)
        enc.mid_block = _Block()
        enc.mid_block.resnets = nn.ModuleList([_Resnet(out_c, out_c, groups), _Resnet(out_c, out_c, groups)])
        enc.mid_block.attentions = nn.ModuleList([_Attention(out_c, groups)])
        enc.conv_norm_out = nn.GroupNorm(groups, out_c, eps=1e-6)
        enc.conv_out = nn.Conv2d(out_c, 2 * latent, 3, padding=1)
        self.encoder = enc
        self.quant_conv = nn.Conv2d(2 * latent, 2 * latent, 1)

    @torch.no_grad()
    def moments(self, images_u8: torch.Tensor) -> torch.Tensor:
        """uint8 NHWC [B,H,W,3] -> fp32 moments NCHW [B,8,H/8,W/8] (mean | log-variance)."""
        e = self.encoder
        x = e.conv_in(images_u8.permute(0, 3, 1, 2).float() / 127.5 - 1.0)
        for blk in e.down_blocks:
            for r in blk.resnets:
                x = r(x)
            if hasattr(blk, "downsamplers"):
                x = blk.downsamplers[0](x)
        x = e.mid_block.resnets[0](x)
        x = e.mid_block.attentions[0](x)
        x = e.mid_block.resnets[1](x)
        return self.quant_conv(e.conv_out(F.silu(e.conv_norm_out(x))))


def posterior(moments: torch.Tensor, eps: torch.Tensor | None = None, scaling: float = SCALING) -> torch.Tensor:
    """DiagonalGaussianDistribution.sample with the given eps (None: .mode()), times the scaling factor."""
    mean, logvar = moments.float().chunk(2, dim=1)
    z = mean if eps is None else mean + torch.exp(0.5 * logvar.clamp(-30.0, 20.0)) * eps
    return z * scaling


def encoder_ref(sd: dict) -> VAEEncoderRef:
    m = VAEEncoderRef().eval()
    m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return m
