"""float64 restatement of DPM-Solver++(2M) on the project's grid (TEST REFERENCE ONLY).

Lu et al. 2022, Algorithm 2 (the data-prediction multistep solver), on DDIMScheduler's timesteps: leading spacing,
steps_offset 1, the last step lands on alphas_cumprod[0].  It is written from the definitions, straight from
a = alphas_cumprod and the lambdas, and never reads the scheduler's coefficient table:
    alpha = sqrt(a), sigma = sqrt(1 - a), lambda = log(alpha / sigma)
    step i of S: s = timesteps[i] -> t = timesteps[i + 1] (the terminal alpha for i = S - 1), h = lambda_t - lambda_s
    x0 = (x - sigma_s e) / alpha_s
    D  = x0 on a first-order step, else x0 + (x0 - x0_prev) / (2 r), r = (lambda_s - lambda_s_prev) / h
    x' = (sigma_t / sigma_s) x + alpha_t (1 - exp(-h)) D,   x0_prev <- x0
First-order: the first step of a run, the last step when S < 15 (lower_order_final), every step at solver_order 1.
Every function takes dtype: float64 is the reference, float32 the same formulas in fp32 from the float64 lambdas
rounded to fp32 (the error E the tests' bars are multiples of).
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from oracle.ddim_ref import alphas_cumprod, timesteps


class Grid(NamedTuple):
    """Per step i, float64 [S] each: the alphas_cumprod at both ends and (alpha, sigma, lambda) there."""
    ts: list
    a_s: torch.Tensor
    a_t: torch.Tensor
    alpha_s: torch.Tensor
    sigma_s: torch.Tensor
    lam_s: torch.Tensor
    alpha_t: torch.Tensor
    sigma_t: torch.Tensor
    lam_t: torch.Tensor


def _asl(a: torch.Tensor):
    alpha, sigma = a.sqrt(), (1 - a).sqrt()
    return alpha, sigma, (alpha / sigma).log()


def grid(steps: int) -> Grid:
    ac = alphas_cumprod().double()
    ts = [int(t) for t in timesteps(steps)]
    a_s = ac[ts]
    a_t = torch.cat([a_s[1:], ac[:1]])          # the next step's alpha; the terminal alpha after the last step
    return Grid(ts, a_s, a_t, *_asl(a_s), *_asl(a_t))


def first_order(i: int, steps: int, first: int = 0, solver_order: int = 2, lower_order_final: bool = True) -> bool:
    return i == first or solver_order == 1 or (lower_order_final and i == steps - 1 and steps < 15)


def cfg(eps: torch.Tensor, guidance: float, dtype=torch.float64) -> torch.Tensor:
    """eps NHWC [2B, h, w, 4] (uncond rows first) -> the guided prediction NCHW [B, 4, h, w] in dtype."""
    eu, ec = eps.to(dtype).permute(0, 3, 1, 2).chunk(2)
    return eu + torch.tensor(guidance, dtype=dtype) * (ec - eu)


def step(e: torch.Tensor, x: torch.Tensor, x0_prev: torch.Tensor | None, g: Grid, i: int, first: bool,
         dtype=torch.float64):
    """One step from the guided prediction e -> (x', x0) in dtype; x0_prev is not read on a first-order step."""
    alpha_s, sigma_s, lam_s, alpha_t, sigma_t, lam_t = (v[i].to(dtype) for v in g[3:])
    e, x = e.to(dtype), x.to(dtype)
    h = lam_t - lam_s
    x0 = (x - sigma_s * e) / alpha_s
    d = x0
    if not first:
        r = (lam_s - g.lam_s[i - 1].to(dtype)) / h
        d = x0 + (x0 - x0_prev.to(dtype)) / (2 * r)
    return (sigma_t / sigma_s) * x + alpha_t * -torch.expm1(-h) * d, x0


def blend(xn: torch.Tensor, z0: torch.Tensor, noise: torch.Tensor, mask: torch.Tensor, g: Grid, i: int,
          dtype=torch.float64) -> torch.Tensor:
    """(1 - m) known + m x': known is z0 noised to the next step's timestep, z0 itself at the last step."""
    known = z0.to(dtype)
    if i < len(g.ts) - 1:
        known = g.alpha_t[i].to(dtype) * known + g.sigma_t[i].to(dtype) * noise.to(dtype)
    m = mask.to(dtype)[:, None]
    return (1 - m) * known + m * xn.to(dtype)


def masked_step(e, x, x0_prev, z0, noise, mask, g: Grid, i: int, first: bool, dtype=torch.float64):
    """step followed by the inpainting blend -> (x, x0)."""
    xn, x0 = step(e, x, x0_prev, g, i, first, dtype)
    return blend(xn, z0, noise, mask, g, i, dtype), x0


def run(eps_fn, x: torch.Tensor, steps: int, start: int = 0, solver_order: int = 2, lower_order_final: bool = True,
        z0=None, noise=None, mask=None, dtype=torch.float64) -> torch.Tensor:
    """The last steps - start steps.  eps_fn(x, t) -> the guided prediction at timestep t; x is the start (already
    noised to timesteps[start]); with mask [B, h, w] (and z0, noise) every step ends with the blend."""
    g = grid(steps)
    x, x0_prev = x.to(dtype), None
    for i in range(start, steps):
        first = first_order(i, steps, start, solver_order, lower_order_final)
        x, x0_prev = step(eps_fn(x, g.ts[i]), x, x0_prev, g, i, first, dtype)
        if mask is not None:
            x = blend(x, z0, noise, mask, g, i, dtype)
    return x
