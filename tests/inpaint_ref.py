"""float64 restatement of the inpainting loop (TEST REFERENCE ONLY).

diffusers==0.23.1 StableDiffusionInpaintPipeline with a 4-channel UNet (num_channels_unet == 4): the UNet sees the
plain latents; after every scheduler step
    latents = (1 - m) * known + m * latents
with known = scheduler.add_noise(z0, noise, timesteps[i + 1]) for every step but the last and known = z0 at the
last one, z0 the scaled image latents, noise the tensor the initial latents were made of, m the mask (1 = repaint)
at the latents' size, broadcast over the channels.  The mask is binarised at 0.5 and resized with F.interpolate
(nearest) to the latents' size.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.ddim_ref import alphas_cumprod, ddim_step, timesteps


def latent_mask(mask_u8: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """uint8 [B, H, W] -> fp32 [B, h, w] of 0 / 1: the pipeline's binarisation and nearest resize."""
    return F.interpolate((mask_u8.float() / 255 >= 0.5).float()[:, None], size=(h, w))[:, 0]


def masked_loop(eps_fn, x: torch.Tensor, z0: torch.Tensor, noise: torch.Tensor, mask: torch.Tensor, steps: int,
                start: int = 0, dtype=torch.float64) -> torch.Tensor:
    """The last steps - start steps of the masked loop in `dtype`.  eps_fn(x, t) -> the guided noise prediction
    for latents x at timestep t; x [B, 4, h, w] is the start (already noised to timesteps[start]); mask [B, h, w]."""
    ac, ts = alphas_cumprod().to(dtype), timesteps(steps)
    x, z0, noise, m = x.to(dtype), z0.to(dtype), noise.to(dtype), mask.to(dtype)[:, None]
    for i in range(start, steps):
        t = int(ts[i])
        x = ddim_step(eps_fn(x, t).to(dtype), t, x, steps, ac)
        known = z0
        if i < steps - 1:
            a = ac[int(ts[i + 1])]
            known = a ** 0.5 * z0 + (1 - a) ** 0.5 * noise
        x = (1 - m) * known + m * x
    return x


def masked_step(eps: torch.Tensor, x: torch.Tensor, z0: torch.Tensor, noise: torch.Tensor, mask: torch.Tensor,
                guidance: float, coef: torch.Tensor, st: int, dtype=torch.float64) -> torch.Tensor:
    """One step as c2d_cfg_ddim_step_masked states it, in `dtype`, from the values the kernel reads: eps NHWC
    [2B, h, w, 4] (fp16-rounded, uncond rows first), coef fp32 [steps, 2] = (alpha_t, alpha_prev), step st."""
    eu, ec = eps.to(dtype).permute(0, 3, 1, 2).chunk(2)
    e = eu + torch.tensor(guidance, dtype=dtype) * (ec - eu)
    a_t, a_p = coef[st].to(dtype)
    x0 = (x.to(dtype) - (1 - a_t).sqrt() * e) / a_t.sqrt()
    xn = a_p.sqrt() * x0 + (1 - a_p).sqrt() * e
    known = z0.to(dtype)
    if st < coef.shape[0] - 1:
        known = a_p.sqrt() * known + (1 - a_p).sqrt() * noise.to(dtype)
    m = mask.to(dtype)[:, None]
    return (1 - m) * known + m * xn
