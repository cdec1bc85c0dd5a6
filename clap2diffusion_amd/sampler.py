"""CFG + DDIM (or DPM-Solver++(2M)) denoise loop driven by a captured hipGraph.

One denoise step = latent -> NHWC fp16 (duplicated for the [uncond, cond]
CFG pair), sinusoidal timestep embedding, the HIP UNet forward, and the fused
CFG+DDIM update, which also advances a device-side step counter.  The step
reads its timestep and DDIM coefficients through that counter, so the same
graph is replayed for every step: no host work and no host<->device traffic
inside the 50-step loop.

The cross-attention K|V of every attn2 layer (text context + gated audio
tokens, AudioAttnProcessor :76-122) does not depend on the latent: it is
computed once per run into persistent buffers and passed to the processors as
cross_attention_kwargs['context_kv'], so the captured step holds only the
latent-dependent work.  The same holds for the time conditioning (sinusoidal
embedding -> TimestepEmbedding MLP -> all 22 time_emb_proj): it depends on the
step only, so one run computes it for every step at once (M = steps rows instead
of four M = 2B launches per step, whose K loops are pure latency) and the step
selects its row through the device step counter, broadcast to the CFG batch by a
zero leading stride.

With a DPMSolverMultistepScheduler the step ends with the fused CFG + DPM-Solver++(2M) update instead: the
denoiser then also holds the previous step's data prediction x0_prev and a device copy of the step the run was
entered at (first_idx: that step is first-order and does not read x0_prev), so the one captured graph serves
text-to-image and img2img entered at any step.  Everything before the final launch is the same.
"""
from __future__ import annotations

import torch

from . import ops
from .scheduler import DDIMScheduler, DPMSolverMultistepScheduler
from .vae import SCALING


class GraphDenoiser:
    def __init__(self, unet, scheduler: DDIMScheduler, batch: int, height: int, width: int, guidance: float,
                 encoder_hidden_states: torch.Tensor, cross_attention_kwargs: dict | None, use_graph: bool = True):
        dev = encoder_hidden_states.device
        self.unet, self.sched = unet, scheduler
        self.b, self.h, self.w, self.g = batch, height, width, float(guidance)
        assert encoder_hidden_states.shape[0] == 2 * batch, "ehs must be [uncond; cond] for the CFG pair"
        self.ehs = encoder_hidden_states.to(torch.float16).contiguous()
        self.kw = dict(cross_attention_kwargs or {})
        self.cross_attns = [m for m in unet.modules()
                            if getattr(m, "is_cross_attention", False) and hasattr(m.processor, "context_kv")]
        self.context_kv = {}
        self.dpm = isinstance(scheduler, DPMSolverMultistepScheduler)
        self.t_table, self.coef, *mcoef = scheduler.device_tables(dev)
        self.steps = self.t_table.numel()
        self.x = torch.zeros(batch, 4, height, width, dtype=torch.float32, device=dev)
        self.step_idx = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.dpm:   # the multistep state; a DDIM denoiser allocates none of it
            self.mcoef, = mcoef
            self.x0_prev = torch.zeros_like(self.x)
            self.first_idx = torch.zeros(1, dtype=torch.int32, device=dev)
        self.use_graph = use_graph
        self.graph = None
        # inpainting: the known latents, the noise that made the initial latents and the latent mask, read by the
        # masked step; allocated (and its graph captured) on the first masked use, so text-to-image holds none
        self.z0 = self.noise = self.mask = None
        self.graph_masked = None
        self.temb_ch = unet.cfg["block_out_channels"][0]
        self.temb_table = None   # [steps, 22 x cout] fp16: every resnet's time_emb_proj output per step
        self.temb_cur = None     # [1, 22 x cout]: this step's row

    def prepare_time(self) -> None:
        """(Re)compute the time-conditioning table for every step (eager or inside a graph)."""
        u = self.unet
        t_sin = torch.cat([ops.timestep_embedding(self.t_table[i:i + 1], None, 1, self.temb_ch)
                           for i in range(self.steps)])
        table = u.time_conditioning(t_sin)
        if self.temb_table is None:
            self.temb_table = torch.empty_like(table)
            self.temb_cur = torch.empty((1, table.shape[1]), device=table.device, dtype=table.dtype)
        self.temb_table.copy_(table)

    def prepare_context(self) -> None:
        """(Re)compute every cross-attention K|V into its persistent buffer, and the
        time-conditioning table (eager, or captured into the conditioning graph)."""
        self.prepare_time()
        audio = self.kw.get("audio")
        for attn in self.cross_attns:
            buf = self.context_kv.get(attn)
            self.context_kv[attn] = attn.processor.context_kv(attn, self.ehs, audio, out=buf)

    def masked_buffers(self) -> None:
        """Allocate the static z0 / noise (fp32, x's shape) and mask (fp32 [B, h, w]) of the masked step once."""
        if self.z0 is None:
            self.z0, self.noise = torch.zeros_like(self.x), torch.zeros_like(self.x)
            self.mask = torch.ones(self.b, self.h, self.w, dtype=torch.float32, device=self.x.device)

    def _body(self, masked: bool = False) -> None:
        # the CFG pair [x; x] enters the UNet as x once (forward_nhwc cfg_pair: the prefix before
        # the first cross-attention runs on one half and is duplicated there)
        xin = ops.latent_to_nhwc(self.x, self.unet.in_pad, dup=False)
        torch.index_select(self.temb_table, 0, self.step_idx, out=self.temb_cur)
        temb_all = self.temb_cur.expand(2 * self.b, self.temb_cur.shape[1])   # zero row stride: one row for all
        eps = self.unet.forward_nhwc(xin, None, self.ehs, dict(self.kw, context_kv=self.context_kv),
                                     temb_all=temb_all, cfg_pair=True)
        if self.dpm and masked:
            ops.cfg_dpm_step_masked(eps, self.x, self.x0_prev, self.z0, self.noise, self.mask, self.g, self.mcoef,
                                    self.step_idx, self.first_idx, advance=True)
        elif self.dpm:
            ops.cfg_dpm_step(eps, self.x, self.x0_prev, self.g, self.mcoef, self.step_idx, self.first_idx,
                             advance=True)
        elif masked:   # inpainting: the same update blended with the known region (z0 re-noised to the next step)
            ops.cfg_ddim_step_masked(eps, self.x, self.z0, self.noise, self.mask, self.g, self.coef, self.step_idx,
                                     advance=True)
        else:
            ops.cfg_ddim_step(eps, self.x, self.g, self.coef, self.step_idx, advance=True)

    def _capture(self, masked: bool, pool=None) -> torch.cuda.CUDAGraph:
        self.step_idx.zero_()   # the warm-up below runs the step kernel: keep the counter inside the table
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._body(masked)  # warm-up: packs lazily-built weights, primes the allocator
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, pool=pool):
            self._body(masked)
        self.step_idx.zero_()
        return graph

    def ensure_captured(self, masked: bool = False) -> None:
        """Capture the step graph, and for a masked run the masked buffers and graph, on their first use.  The
        warm-up and the recorded step run on x, so call this before start().  The masked body is a second graph;
        self.graph stays as it is.  It is captured into the first graph's memory pool: the two bodies allocate the
        same UNet activations, neither reads anything the other left there (all state is in the static buffers),
        and one stream replays them one after the other, so the activations are held once."""
        if masked:
            self.masked_buffers()
        if not self.use_graph:
            return
        if self.graph is None:
            self.graph = self._capture(False)
        if masked and self.graph_masked is None:
            self.graph_masked = self._capture(True, pool=self.graph.pool())

    def start(self, latents: torch.Tensor, t_start: int = 0, moments: torch.Tensor | None = None,
              eps: torch.Tensor | None = None, mask_u8: torch.Tensor | None = None) -> None:
        """Write the state the loop starts from: x, the device step counter and, with a mask, z0 / noise / mask.
        latents fp32 [B, 4, h, w] on the device, contiguous: the initial noise.  No host synchronisation, so a
        caller may record it into a graph.
        moments None (text-to-image): x = latents * init_noise_sigma, counter 0.
        moments (the VAE encoder's fp16 rows of the init images; img2img): x = the posterior sample (eps fp32, None:
        the mode) noised with latents to timesteps[t_start]; the kernel reads that step's alpha through the counter.
        mask_u8 uint8 [B, 8h, 8w] as well (inpainting): one launch writes z0, x (latents themselves when t_start is
        0: strength 1 starts from pure noise, init_noise_sigma is 1 for DDIM) and the latent mask."""
        if not 0 <= t_start < self.steps:
            raise ValueError(f"t_start {t_start} outside [0, {self.steps})")
        if moments is None and (t_start or mask_u8 is not None):
            raise ValueError("t_start and mask_u8 need the init image's moments")
        if moments is None:
            self.x.copy_(latents * self.sched.init_noise_sigma)
            self.step_idx.zero_()
        elif mask_u8 is None:
            self.step_idx.fill_(t_start)
            ops.vae_posterior_noise(moments, self.x, SCALING, eps=eps, noise=latents, coef=self.coef,
                                    step_index=self.step_idx)
        else:
            self.masked_buffers()
            self.step_idx.fill_(t_start)
            ops.inpaint_prepare(moments, latents, mask_u8, SCALING, eps=eps, coef=self.coef, step_index=self.step_idx,
                                pure_noise=t_start == 0, z0=self.z0, x=self.x, mask=self.mask)
            self.noise.copy_(latents)
        if self.dpm:   # the step the counter was just set to is this run's first: first-order, x0_prev unread
            self.first_idx.fill_(t_start)

    def step(self, masked: bool = False) -> None:
        """One step: a replay of the (masked) step graph, or the eager body."""
        if self.use_graph:
            (self.graph_masked if masked else self.graph).replay()
        else:
            self._body(masked)

    def denoise(self, t_start: int = 0, masked: bool = False) -> torch.Tensor:
        """The loop: steps - t_start steps from the state start() wrote -> denoised latents fp32 (self.x)."""
        for _ in range(self.steps - t_start):
            self.step(masked)
        return self.x

    @torch.no_grad()
    def run(self, latents: torch.Tensor, t_start: int = 0, moments: torch.Tensor | None = None,
            eps: torch.Tensor | None = None, mask_u8: torch.Tensor | None = None) -> torch.Tensor:
        """start()'s arguments -> denoised latents fp32: the whole run of one denoiser on its own."""
        self.prepare_context()
        self.ensure_captured(mask_u8 is not None)
        self.start(latents, t_start, moments, eps, mask_u8)
        return self.denoise(t_start, mask_u8 is not None)
