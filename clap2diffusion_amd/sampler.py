"""CFG + DDIM denoise loop driven by a captured hipGraph.

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
"""
from __future__ import annotations

import torch

from . import ops
from .scheduler import DDIMScheduler


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
        self.t_table, self.coef = scheduler.device_tables(dev)
        self.steps = self.t_table.numel()
        self.x = torch.zeros(batch, 4, height, width, dtype=torch.float32, device=dev)
        self.step_idx = torch.zeros(1, dtype=torch.int32, device=dev)
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
        if masked:   # inpainting: the same update blended with the known region (z0 re-noised to the next step)
            ops.cfg_ddim_step_masked(eps, self.x, self.z0, self.noise, self.mask, self.g, self.coef, self.step_idx,
                                     advance=True)
        else:
            ops.cfg_ddim_step(eps, self.x, self.g, self.coef, self.step_idx, advance=True)

    def capture(self) -> None:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._body()  # warm-up: packs lazily-built weights, primes the allocator
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._body()
        self.step_idx.zero_()

    def capture_masked(self) -> None:
        """The masked body as a second graph; self.graph stays as it is.  It is captured into the first graph's
        memory pool: the two bodies allocate the same UNet activations, neither reads anything the other left
        there (all state is in the static buffers), and one stream replays them one after the other, so the
        activations are held once."""
        self.masked_buffers()
        if self.graph is None:
            self.capture()
        self.step_idx.zero_()   # the warm-up below runs the step kernel: keep the counter inside the table
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._body(masked=True)
        torch.cuda.current_stream().wait_stream(s)
        self.graph_masked = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_masked, pool=self.graph.pool()):
            self._body(masked=True)
        self.step_idx.zero_()

    def step_masked(self) -> None:
        """One masked step: a replay of the masked graph, or the eager body."""
        self.graph_masked.replay() if self.use_graph else self._body(masked=True)

    @torch.no_grad()
    def run(self, latents: torch.Tensor | None, start: int = 0, masked: bool = False) -> torch.Tensor:
        """latents [B,4,h,w] (scaled by init_noise_sigma = 1) -> denoised latents fp32.
        start: first step index (img2img: latents already noised to timesteps[start]); the device counter is
        set to it and the same captured step is replayed steps - start times.
        masked (inpainting): self.z0 / self.noise / self.mask / self.x are already filled (ops.inpaint_prepare;
        latents is not read) and the masked step runs steps - start times."""
        if not 0 <= start < self.steps:
            raise ValueError(f"start {start} outside [0, {self.steps})")
        self.prepare_context()
        if masked:
            if self.z0 is None:
                raise RuntimeError("masked run before masked_buffers(): z0 / noise / mask / x are not filled")
            if self.use_graph and self.graph_masked is None:
                x = self.x.clone()      # the capture's warm-up and the step it records run on x
                self.capture_masked()
                self.x.copy_(x)
            self.step_idx.fill_(start)
            for _ in range(self.steps - start):
                self.step_masked()
            return self.x
        if self.use_graph and self.graph is None:
            self.capture()
        self.x.copy_(latents)
        self.step_idx.fill_(start)
        for _ in range(self.steps - start):
            if self.use_graph:
                self.graph.replay()
            else:
                self._body()
        return self.x
