"""DDIM scheduler (diffusers 0.23.1 DDIMScheduler semantics, SD1.5 config).

scaled_linear betas 0.00085 -> 0.012 over 1000 train steps, set_alpha_to_one
False (final alpha_cumprod = alphas_cumprod[0]), steps_offset 1, "leading"
timestep spacing, eta 0, epsilon prediction, no clipping.  Besides the
diffusers-style set_timesteps / step API (torch, host-driven), `device_tables`
returns the per-step (timestep, alpha_t, alpha_prev) tables the fused
c2d_cfg_ddim_step kernel reads through a device step counter, so a captured
hipGraph of one denoise step can be replayed for every step.
"""
from __future__ import annotations

import math

import numpy as np
import torch


class DDIMScheduler:
    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 steps_offset: int = 1, set_alpha_to_one: bool = False):
        self.num_train_timesteps = num_train_timesteps
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.steps_offset = steps_offset
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = None

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        ratio = self.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.steps_offset
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _alphas(self, t: int):
        prev = t - self.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_p = self.alphas_cumprod[prev] if prev >= 0 else self.final_alpha_cumprod
        return a_t, a_p

    def step(self, model_output: torch.Tensor, timestep: int, sample: torch.Tensor):
        a_t, a_p = self._alphas(int(timestep))
        x0 = (sample - (1 - a_t) ** 0.5 * model_output) / a_t ** 0.5
        prev = a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * model_output
        return type("DDIMOutput", (), {"prev_sample": prev, "pred_original_sample": x0})()

    @staticmethod
    def img2img_start(num_inference_steps: int, strength: float) -> int:
        """First step index of an image-to-image run (diffusers StableDiffusionImg2ImgPipeline.get_timesteps):
        init = min(int(steps * strength), steps), t_start = max(steps - init, 0); the run starts from the
        image noised to timesteps[t_start] and takes the last `init` steps."""
        if not 0.0 <= strength <= 1.0:
            raise ValueError(f"strength must be in [0, 1], got {strength}")
        init = min(int(num_inference_steps * strength), num_inference_steps)
        if init < 1:
            raise ValueError(f"strength {strength} with {num_inference_steps} steps leaves no denoising step")
        return max(num_inference_steps - init, 0)

    def add_noise(self, original: torch.Tensor, noise: torch.Tensor, timestep: int) -> torch.Tensor:
        """diffusers DDIMScheduler.add_noise at one timestep (host-side form of c2d_vae_posterior_noise)."""
        a = self.alphas_cumprod[int(timestep)]
        return a ** 0.5 * original + (1 - a) ** 0.5 * noise

    def device_tables(self, device) -> tuple[torch.Tensor, torch.Tensor]:
        """-> (t_table fp32 [S], coef fp32 [S, 2] = (alpha_t, alpha_prev))."""
        assert self.timesteps is not None, "call set_timesteps first"
        ts = [int(t) for t in self.timesteps]
        coef = torch.tensor([[float(a) for a in self._alphas(t)] for t in ts], dtype=torch.float32)
        return (torch.tensor(ts, dtype=torch.float32, device=device), coef.to(device))


class DPMSolverMultistepScheduler(DDIMScheduler):
    """DPM-Solver++(2M): the data-prediction multistep solver of Lu et al. 2022 (Algorithm 2), restated on this
    project's own grid.  It is not diffusers' DPMSolverMultistepScheduler bit for bit: the timesteps and the terminal
    alpha are DDIMScheduler's (leading spacing, steps_offset 1, the last step lands on alphas_cumprod[0]), so
    img2img_start, the time-embedding table, add_noise at timesteps[t_start] and the inpainting rule "alpha_prev of
    this step = alpha_t of the next" hold for both schedulers, which is why this one derives from DDIMScheduler.

    With a = alphas_cumprod, alpha = sqrt(a), sigma = sqrt(1 - a), lambda = log(alpha / sigma), step i goes from
    s = timesteps[i] to t = timesteps[i + 1] (the terminal alpha for the last step), h = lambda_t - lambda_s:
        x0 = (x - sigma_s e) / alpha_s
        D  = x0                                 on a first-order step
             x0 + (x0 - x0_prev) / (2 r)        otherwise, r = (lambda_s - lambda_s_prev) / h
        x' = (sigma_t / sigma_s) x + alpha_t (1 - exp(-h)) D,     x0_prev <- x0
    First-order steps: the first step a run takes (reset's t_start), the last step when there are fewer than 15
    steps and lower_order_final, every step with solver_order = 1 (algebraically DDIM), and a step onto sigma_t = 0
    (set_alpha_to_one: h is infinite and r undefined).  `device_tables` adds the per-step coefficient rows the fused
    c2d_cfg_dpm_step kernel reads through the device step counter."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 steps_offset: int = 1, set_alpha_to_one: bool = False, solver_order: int = 2,
                 lower_order_final: bool = True):
        super().__init__(num_train_timesteps, beta_start, beta_end, steps_offset, set_alpha_to_one)
        if solver_order not in (1, 2):
            raise ValueError(f"solver_order must be 1 or 2, got {solver_order}")
        self.solver_order, self.lower_order_final = solver_order, bool(lower_order_final)
        self.reset()

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        super().set_timesteps(num_inference_steps, device)
        self.reset()

    def reset(self, t_start: int = 0) -> None:
        """Forget the previous run: the next step() is step t_start of the grid, and it is first-order."""
        self._first = self._next = int(t_start)
        self._x0_prev = None

    @staticmethod
    def _asl(a: float) -> tuple[float, float, float]:
        """alpha_cumprod -> (alpha, sigma, lambda) in float64."""
        alpha, sigma = math.sqrt(a), math.sqrt(1.0 - a)
        return alpha, sigma, (math.log(alpha / sigma) if sigma > 0.0 else math.inf)

    def coefficients(self, i: int) -> tuple[float, ...]:
        """Step i's (alpha_s, sigma_s, alpha_t, sigma_t, sigma_t / sigma_s, alpha_t (1 - exp(-h)), 1 / (2 r), order)
        in float64: a row of device_tables' mcoef before its rounding.  1 / (2 r) is 0 in row 0 (no earlier step);
        order is 1.0 where the row is first-order whatever the run, else 2.0."""
        ts = [int(t) for t in self.timesteps]
        a_s, a_t = (float(a) for a in self._alphas(ts[i]))
        alpha_s, sigma_s, lam_s = self._asl(a_s)
        alpha_t, sigma_t, lam_t = self._asl(a_t)
        h = lam_t - lam_s
        first_order = self.solver_order == 1 or not math.isfinite(h) \
            or (self.lower_order_final and i == len(ts) - 1 and len(ts) < 15)
        inv2r = 0.0
        if i > 0 and math.isfinite(h):
            inv2r = h / (2.0 * (lam_s - self._asl(float(self.alphas_cumprod[ts[i - 1]]))[2]))
        return (alpha_s, sigma_s, alpha_t, sigma_t, sigma_t / sigma_s, alpha_t * -math.expm1(-h), inv2r,
                1.0 if first_order else 2.0)

    def step(self, model_output: torch.Tensor, timestep: int, sample: torch.Tensor):
        """One host step in the sample's dtype (the coefficients are float64 scalars).  The steps of a run come in
        the grid's order from reset's t_start on; anything else raises."""
        assert self.timesteps is not None, "call set_timesteps first"
        i = self._next
        if i >= len(self.timesteps):
            raise RuntimeError("the run is finished: call reset(t_start) before the next one")
        if int(timestep) != int(self.timesteps[i]):
            raise ValueError(f"step {i} of this run is timestep {int(self.timesteps[i])}, got {int(timestep)}")
        alpha_s, sigma_s, _, _, ratio, gain, inv2r, order = self.coefficients(i)
        x0 = (sample - sigma_s * model_output) / alpha_s
        d = x0 if i == self._first or order == 1.0 else x0 + (x0 - self._x0_prev) * inv2r
        prev = ratio * sample + gain * d
        self._x0_prev, self._next = x0, i + 1
        return type("DPMSolverOutput", (), {"prev_sample": prev, "pred_original_sample": x0})()

    def device_tables(self, device) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (t_table fp32 [S], coef2 fp32 [S, 2], mcoef fp32 [S, 8]): DDIMScheduler.device_tables' two tensors
        (coef2 is what c2d_vae_posterior_noise and c2d_inpaint_prepare keep reading) and the `coefficients` rows,
        computed in float64 and rounded once."""
        t_table, coef2 = super().device_tables(device)
        rows = [self.coefficients(i) for i in range(len(self.timesteps))]
        return t_table, coef2, torch.tensor(rows, dtype=torch.float64).to(torch.float32).to(device)
