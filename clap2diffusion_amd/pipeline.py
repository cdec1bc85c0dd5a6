"""AudioToImageInference — drop-in for the reference scripts/inference.py API.

Same class, constructor, methods and CLI flags as the reference
(scripts/inference.py:21-216): load_models, load_audio, extract_clap_embedding,
apply_normalization, generate, batch_generate, main(--audio --text --output
--checkpoint_dir --steps --cfg_scale --seed --no_hierarchical).  Where the
reference stubs the CLAP embedding (:85-90) and the image (:161-164), this
runs the real path:
  audio -> ClapFeatureExtractor (CPU) -> HTSAT (HIP) -> ImprovedHierarchicalAudioEncoder
  -> routed {early, mid, late} tokens -> 16 AudioAttnProcessor cross-attentions
  -> 50-step CFG+DDIM on the HIP UNet (captured hipGraph) -> VAE decode -> PIL image.
Composition contract: ehs = CLIP([uncond "", prompt]);
routed tokens repeated for both CFG halves; adapter + Norm-60 and the legacy
HierarchicalAudioV4 outputs are computed for API fidelity but not fed to the UNet.
Checkpoints are loaded when present (clap_encoder.pth -> the HTSAT tower,
audio_projector_stage2.pth 'adapter_state_dict', hierarchical_v4_final.pth,
unet_adapter_final.pth -> the per-level audio processors; all with weights_only=True),
otherwise every network uses seeded synthetic weights.
"""
from __future__ import annotations

import argparse
import os
import warnings
from pathlib import Path
from typing import NamedTuple

import numpy as np
import torch

from . import weights as W
from .audio_io import SR, _read_wav, read_audio, synthetic_thunder  # noqa: F401  (_read_wav: imported from here)
from .features import ClapLogMel
from .htsat import HTSATEncoder
from .image_io import prepare_image_array, prepare_mask_array
from .processor import AudioProcessorManager
from .projectors import AudioAdapter, HierarchicalAudioV4, ImprovedHierarchicalAudioEncoder, normalize_tokens
from .sampler import GraphDenoiser
from .scheduler import DDIMScheduler, DPMSolverMultistepScheduler
from .text_encoder import TextEncoder, make_tokenizer
from .unet import UNet2DConditionModel
from .vae import VAEDecoder, VAEEncoder
from . import ops

# Supported image sizes: the UNet halves the 8x-downsampled latent three times and concatenates each level with
# its skip on the way up, so the latent height and width must be multiples of 8 (pixels: of 64); the smallest,
# 64 x 64 pixels (8 x 8 latents, 1 x 1 images at the innermost level), is the smallest the kernel tests cover
# (tests/test_small_shapes_gpu.py, DESIGN.md "Smallest supported shapes").
IMAGE_SIZE_MULTIPLE = 64
MIN_IMAGE_SIZE = 64


# sampler= names: the solver of the denoise loop.  Both run on DDIMScheduler's timestep grid.
SAMPLERS = {"ddim": DDIMScheduler, "dpmpp_2m": DPMSolverMultistepScheduler}


def check_sampler(sampler: str) -> str:
    """ValueError unless `sampler` names a solver the pipeline runs."""
    if sampler not in SAMPLERS:
        raise ValueError(f"unknown sampler {sampler!r}: choose one of {', '.join(SAMPLERS)}")
    return sampler


def check_image_size(height: int, width: int) -> None:
    """ValueError unless height x width (pixels) is a size the pipeline runs."""
    for name, v in (("height", height), ("width", width)):
        if v < MIN_IMAGE_SIZE:
            raise ValueError(f"{name} {v} is below the smallest supported size {MIN_IMAGE_SIZE} "
                             f"(supported sizes: multiples of {IMAGE_SIZE_MULTIPLE} from {MIN_IMAGE_SIZE} up)")
        if int(v) != v or v % IMAGE_SIZE_MULTIPLE:
            raise ValueError(f"{name} {v} is not a multiple of {IMAGE_SIZE_MULTIPLE}: the latent ({name} / 8) is "
                             "halved exactly by each of the UNet's three stride-2 levels, so it must be a multiple "
                             f"of 8 (supported sizes: multiples of {IMAGE_SIZE_MULTIPLE} from {MIN_IMAGE_SIZE} up)")


def check_latent_size(h: int, w: int) -> None:
    """check_image_size for a latent h x w (pixels / 8): latent_hw= and caller-supplied latents."""
    check_image_size(8 * int(h), 8 * int(w))


def _seeded_noise(seeds: list[int], h: int, w: int, device, draws: int) -> list[torch.Tensor]:
    """`draws` tensors [B, 4, h, w], drawn one after the other from each sample's own CPU generator
    (torch.Generator().manual_seed(seed)): identical on any number of GPUs."""
    gens = [torch.Generator().manual_seed(int(s)) for s in seeds]
    per_sample = [[torch.randn(4, h, w, generator=g) for _ in range(draws)] for g in gens]
    return [torch.stack(t).to(device) for t in zip(*per_sample)]


def initial_latents(seeds: list[int], h: int, w: int, device=None) -> torch.Tensor:
    """The initial noise of each sample: the first draw of its generator."""
    return _seeded_noise(seeds, h, w, device, 1)[0]


def initial_latents_and_eps(seeds: list[int], h: int, w: int, device=None) -> tuple[torch.Tensor, torch.Tensor]:
    """img2img noise: each sample's generator draws the initial noise (the same tensor initial_latents gives)
    and, right after it, the posterior noise of the VAE encoder's sample."""
    lat, eps = _seeded_noise(seeds, h, w, device, 2)
    return lat, eps


class _Request(NamedTuple):
    """What a call asked for beyond text-to-image, resolved (AudioToImageInference._resolve): the first step that
    runs, the init images uint8 [B, H, W, 3] and masks uint8 [B, H, W] on the device (None: none given), and
    whether the kept pixels are pasted back."""
    t_start: int
    images: torch.Tensor | None
    masks: torch.Tensor | None
    composite: bool


class AudioToImageInference:
    def __init__(self, checkpoint_dir="../checkpoints", device=None, seed: int = 0, height: int = 512,
                 width: int = 512, use_graph: bool = True, verbose: bool = True, sd_model_path=None,
                 clap_model_path=None):
        """sd_model_path: a diffusers-format SD1.5 folder (unet/, vae/, text_encoder/);
        clap_model_path: a ClapModel weights file or folder (e.g. laion/clap-htsat-unfused, the
        model the reference loads at models/audio_encoder.py:47).  Without them the weights
        are the seeded synthetic recipe (weights.py); checkpoint_dir/clap_encoder.pth and the
        projector checkpoints load as in the reference."""
        self.checkpoint_dir = Path(checkpoint_dir)
        self.sd_model_path = sd_model_path
        self.clap_model_path = clap_model_path
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        if self.device.type != "cuda":
            raise RuntimeError("the sampling path runs on the HIP kernels only (MI355X); no CPU fallback")
        check_image_size(height, width)
        self.seed, self.height, self.width = seed, height, width
        self.use_graph, self.verbose = use_graph, verbose
        self.load_models()
        self.OPTIMAL_NORM = 60.0
        self._denoisers = {}
        self._batch_graphs = {}
        self.last_denoiser = None
        self._vae_encoder = None   # built on the first init image: text-to-image allocates nothing for it

    # ------------------------------------------------------------ models
    def _log(self, *a):
        if self.verbose:
            print(*a)

    def load_models(self):
        dev = self.device
        self._log(f"Initializing inference pipeline on {dev}")
        sd15 = None
        if self.sd_model_path:
            self._log(f"Loading SD1.5 weights from {self.sd_model_path}")
            sd15 = W.load_sd15_folder(self.sd_model_path)
        self.unet = UNet2DConditionModel().to(dev)
        self.unet.load_diffusers_state_dict(sd15["unet"] if sd15 else W.synth_unet(self.seed))
        self.manager = AudioProcessorManager(self.unet)
        self.manager.setup_processors(verbose=self.verbose)
        procs = self.manager.level_processors()
        for level, p in procs.items():
            p.load_state_dict(W.synth_processor_weights(level, self.seed))
        # the trained processors (audio_proj.*, alpha per level): reference scripts/inference.py:61-65
        # (also app/gradio_app.py:39-46, scripts/train_stage3.py:78-81); forms: weights.processor_state_dicts
        unet_adapter_path = self.checkpoint_dir / "unet_adapter_final.pth"
        if unet_adapter_path.exists():
            self._log(f"Loading UNet Adapter from {unet_adapter_path}")
            per_level = W.processor_state_dicts(torch.load(unet_adapter_path, map_location="cpu", weights_only=True),
                                                self.manager.level_mapping)
            if not per_level:
                warnings.warn(f"{unet_adapter_path}: no audio-processor keys (audio_proj.* / alpha) recognised; "
                              "keeping the current processor weights")
            for level, sd in per_level.items():
                if level in procs:
                    procs[level].load_state_dict(sd)
        for p in procs.values():
            p.to(dev).eval()
        self.clap = HTSATEncoder().to(dev)
        clap_sd, clap_src = W.resolve_clap_weights(self.checkpoint_dir, self.clap_model_path, self.seed)
        self._log(f"CLAP audio tower: {clap_src}")
        self.clap.load_clap_state_dict(clap_sd)
        self.hier_encoder = W.fill_module(ImprovedHierarchicalAudioEncoder(), "improved.", self.seed).to(dev).eval()
        adapter_path = self.checkpoint_dir / "audio_projector_stage2.pth"
        self.audio_adapter = W.fill_module(AudioAdapter(), "adapter.", self.seed).to(dev).eval()
        if adapter_path.exists():
            self._log(f"Loading Audio Adapter from {adapter_path}")
            ck = torch.load(adapter_path, map_location=dev, weights_only=True)
            if "adapter_state_dict" in ck:
                self.audio_adapter.load_state_dict(ck["adapter_state_dict"])
        self.hierarchical_model = W.fill_module(HierarchicalAudioV4(), "v4.", self.seed).to(dev).eval()
        hpath = self.checkpoint_dir / "hierarchical_v4_final.pth"
        if hpath.exists():
            self._log(f"Loading Hierarchical Model from {hpath}")
            self.hierarchical_model.load_state_dict(torch.load(hpath, map_location=dev, weights_only=True))
        # CLIPTextModel-keyed weights: the SD1.5 text_encoder, else the seeded recipe
        self.text_encoder = TextEncoder(dev, seed=self.seed, state_dict=sd15["text_encoder"] if sd15 else None)
        # the SD1.5 folder's CLIP BPE tokenizer (tokenizer/vocab.json + merges.txt), else hash ids
        self.tokenizer = make_tokenizer(self.sd_model_path)
        self.vae = VAEDecoder().to(dev)
        self.vae.load_diffusers_state_dict(sd15["vae"] if sd15 else W.synth_vae_decoder(self.seed))
        self.scheduler = DDIMScheduler()
        # the reference's ClapProcessor feature extraction (models/audio_encoder.py:163-167) on the GPU
        self.feature_extractor = ClapLogMel(dev)

    # ------------------------------------------------------------ reference API
    def load_audio(self, audio_path, duration=10):
        if str(audio_path).startswith("synthetic:"):
            audio = synthetic_thunder(int(str(audio_path).split(":", 1)[1] or 0), duration)
        else:
            x, sr = read_audio(audio_path, max_seconds=duration)
            if sr != SR:
                from scipy.signal import resample_poly
                g = np.gcd(sr, SR)
                x = resample_poly(x, SR // g, sr // g).astype(np.float32)
            audio = x[: int(duration * SR)]
        return audio / (np.abs(audio).max() + 1e-8)

    def mel_features(self, audios: list) -> torch.Tensor:
        return self.feature_extractor(audios)  # [B, 1001, 64] fp32 on device

    def extract_clap_embedding(self, audio) -> torch.Tensor:
        audios = audio if isinstance(audio, list) else [audio]
        return self.clap(self.mel_features(audios))

    def apply_normalization(self, audio_tokens, target_norm=60.0):
        return normalize_tokens(audio_tokens, target_norm)

    # ------------------------------------------------------------ img2img
    @property
    def vae_encoder(self) -> VAEEncoder:
        """The AutoencoderKL encoder, built and loaded on first use (the SD1.5 folder's vae/ file when one was
        given, else the seeded recipe)."""
        if self._vae_encoder is None:
            enc = VAEEncoder().to(self.device)
            enc.load_diffusers_state_dict(W.load_sd15_vae_encoder(self.sd_model_path) if self.sd_model_path
                                          else W.synth_vae_encoder(self.seed))
            self._vae_encoder = enc
        return self._vae_encoder

    def prepare_images(self, images, n: int | None = None) -> torch.Tensor:
        """Init image(s) (prepare_image_array forms) -> uint8 [B, H, W, 3] on the device at the pipeline's size.  A
        uint8 tensor of that size, one image or n of them, stays on its device (one is repeated for n requests)."""
        if isinstance(images, torch.Tensor) and images.dtype == torch.uint8 and images.dim() == 4 \
                and tuple(images.shape[1:]) == (self.height, self.width, 3) \
                and (n is None or images.shape[0] in (1, n)):
            return images.to(self.device).expand(n or -1, -1, -1, -1).contiguous()
        return torch.from_numpy(prepare_image_array(images, self.height, self.width, n)).to(self.device)

    @torch.no_grad()
    def encode_image(self, images, eps: torch.Tensor | None = None) -> torch.Tensor:
        """Image(s) (prepare_images forms) -> scaled latents fp32 [B, 4, H/8, W/8]; eps None = the posterior mode."""
        return self.vae_encoder.encode(self.prepare_images(images), eps)

    def prepare_masks(self, masks, n: int | None = None) -> torch.Tensor:
        """Inpainting mask(s) (prepare_mask_array forms) -> uint8 [B, H, W] on the device at the pipeline's size,
        >= 128 = repaint.  A uint8 device tensor of that size and count is used as it is."""
        if isinstance(masks, torch.Tensor) and masks.is_cuda and masks.dtype == torch.uint8 and masks.dim() == 3 \
                and tuple(masks.shape[1:]) == (self.height, self.width) and n in (None, masks.shape[0]):
            return masks.to(self.device).contiguous()
        return torch.from_numpy(prepare_mask_array(masks, self.height, self.width, n)).to(self.device)

    def _resolve(self, b: int, steps: int, init_images, strength: float, masks, composite: bool) -> _Request:
        """The init images and masks of b requests on the device (prepare_images / prepare_masks), the step the
        schedule is entered at (DDIMScheduler.img2img_start; 0 for text-to-image) and whether to composite."""
        if init_images is None:
            if masks is not None:
                raise ValueError("a mask needs an init image: inpainting repaints a region of it "
                                 "(init_image= / init_images=)")
            return _Request(0, None, None, False)
        t_start = DDIMScheduler.img2img_start(steps, strength)
        images = self.prepare_images(init_images, b)
        if masks is not None:
            masks = self.prepare_masks(masks, b)
            if tuple(masks.shape) != tuple(images.shape[:3]):
                raise ValueError(f"masks {tuple(masks.shape)} do not match init images {tuple(images.shape)}")
        return _Request(t_start, images, masks, bool(composite) and masks is not None)

    def _request_latents(self, n: int, seed, with_eps: bool = False):
        """(latents, eps) of n requests as the reference's generate() seeds them
        (scripts/inference.py:113-116: torch.manual_seed(seed) / np.random.seed(seed) when a seed
        is given, the RNG left as it is otherwise): each request draws [1, 4, h/8, w/8] from the
        global CPU generator right after its (re-)seeding, so a given seed always yields
        initial_latents([seed]) and seed=None draws fresh noise every call.  with_eps (img2img with a sampled
        posterior): each request draws its posterior noise right after its initial noise, so a seed fixes
        both; eps is None otherwise."""
        h, w = self.height // 8, self.width // 8
        lat, eps = [], []
        for _ in range(n):
            if seed is not None:
                torch.manual_seed(seed)
                np.random.seed(seed)
            lat.append(torch.randn(1, 4, h, w))
            if with_eps:
                eps.append(torch.randn(1, 4, h, w))
        return torch.cat(lat).to(self.device), torch.cat(eps).to(self.device) if with_eps else None

    @torch.no_grad()
    def _generate_u8(self, audio_paths, text_prompts, num_inference_steps=50, guidance_scale=7.5, seed=None,
                     use_hierarchical=True, init_images=None, strength=0.8, sample_posterior=True, masks=None,
                     composite=True, sampler="ddim", **_):
        """generate() for a list of requests -> generate_batch's uint8 [B, H, W, 3] device tensor; keywords it does
        not know are ignored."""
        check_sampler(sampler)   # before any work on the audio
        mel = self.mel_features([self.load_audio(p) for p in audio_paths])
        lat, eps = self._request_latents(len(audio_paths), seed, with_eps=init_images is not None)
        return self.generate_batch(mel, list(text_prompts), num_inference_steps, guidance_scale,
                                   use_hierarchical=use_hierarchical, latents=lat, init_images=init_images,
                                   strength=strength, posterior_eps=eps if sample_posterior else None, masks=masks,
                                   composite=composite, sampler=sampler)

    def _generate(self, audio_paths, text_prompts, *args, **kwargs):
        """_generate_u8 -> PIL images."""
        return self.to_pil(self._generate_u8(audio_paths, text_prompts, *args, **kwargs))

    def generate(self, audio_path, text_prompt="", num_inference_steps=50, guidance_scale=7.5, seed=None,
                 use_hierarchical=True, init_image=None, strength=0.8, sample_posterior=True, mask=None,
                 composite=True, sampler="ddim"):
        """init_image (a PIL image, a path or a uint8 tensor [1, H, W, 3]): audio-guided image-to-image, the
        schedule entered at DDIMScheduler.img2img_start(steps, strength) from the encoded image plus scheduled
        noise; sample_posterior=False takes the VAE posterior's mode instead of a sample.
        mask (prepare_mask_array forms; >= 128 = repaint, < 128 = keep) with init_image: audio-guided inpainting
        (diffusers StableDiffusionInpaintPipeline with a 4-channel UNet): after every step the kept latents are
        set back to the image's, re-noised to that step; strength 1 starts from pure noise.  composite: the kept
        pixels of the result are the init image's own bytes, else the plain decode.
        sampler: "ddim" (the default) or "dpmpp_2m", DPM-Solver++(2M) on the same timestep grid (usually run at
        20-25 steps); anything else is a ValueError."""
        return self._generate([audio_path], [text_prompt], num_inference_steps, guidance_scale, seed, use_hierarchical,
                              init_image, strength, sample_posterior, mask, composite, sampler=sampler)[0]

    def batch_generate(self, audio_paths, text_prompts=None, **kwargs):
        """The reference runs generate(path, prompt, **kwargs) per item (scripts/inference.py:168-180),
        so every item is re-seeded with the same seed (the same initial noise for every item) and
        seed=None leaves the RNG unseeded; here the items run as one batch with those latents.
        init_images= and masks= (one per item, or one for all), strength=, sample_posterior=, composite=, sampler=
        as generate()."""
        return self.to_pil(self.batch_generate_u8(audio_paths, text_prompts, **kwargs))

    def batch_generate_u8(self, audio_paths, text_prompts=None, **kwargs) -> torch.Tensor:
        """batch_generate without the copy to the host: the images as generate_batch leaves them, uint8
        [B, H, W, 3] on the device (what the evaluator scores)."""
        if text_prompts is None:
            text_prompts = [""] * len(audio_paths)
        return self._generate_u8(audio_paths, text_prompts, **kwargs)

    # ------------------------------------------------------------ batched core
    def initial_latents(self, seeds: list[int]) -> torch.Tensor:
        """Per-sample CPU generator (seed) -> identical latents on any number of GPUs."""
        return initial_latents(seeds, self.height // 8, self.width // 8, self.device)

    def denoiser(self, b: int, steps: int, guidance: float, ehs, audio_kwargs, latent_hw=None,
                 slot: int = 0, sampler: str = "ddim") -> GraphDenoiser:
        """The captured-graph denoise loop for (batch, steps, guidance, latent size, sampler), built once;
        `slot` keeps separate sampler states for batches run concurrently on different streams."""
        h, w = latent_hw or (self.height // 8, self.width // 8)
        check_latent_size(h, w)   # latent_hw= and caller-supplied latents (generate_batch, BatchGraph) come through here
        key = (b, steps, float(guidance), h, w, slot, check_sampler(sampler))
        d = self._denoisers.get(key)
        if d is None:
            sch = SAMPLERS[sampler]()
            sch.set_timesteps(steps)
            d = GraphDenoiser(self.unet, sch, b, h, w, guidance, ehs, audio_kwargs, use_graph=self.use_graph)
            self._denoisers[key] = d
        self.last_denoiser = d
        return d

    @torch.no_grad()
    def condition(self, mel: torch.Tensor, ids_uncond: torch.Tensor, ids_cond: torch.Tensor,
                  use_hierarchical: bool = True):
        """mel [B,T,64] -> (ehs [2B,77,768], routed audio kwargs, extras)."""
        clap = self.clap(mel)
        b = clap.shape[0]
        extras = {}
        adapter_tokens = self.apply_normalization(self.audio_adapter(clap), self.OPTIMAL_NORM)
        extras["adapter_tokens"] = adapter_tokens
        if use_hierarchical:
            extras["tokens_77"], extras["hierarchy"] = self.hierarchical_model(clap, return_intermediate=True)
        routed = self.hier_encoder.routed_tokens(clap)   # == forward(clap, return_all=True)[1]["routed"]
        routed = {k: torch.cat([v, v], 0).to(torch.float16).contiguous() for k, v in routed.items()}
        ehs = self.text_encoder(torch.cat([ids_uncond, ids_cond], 0))
        extras["clap"] = clap
        return ehs, self.manager.get_audio_kwargs(routed), extras

    @torch.no_grad()
    def generate_batch(self, mel: torch.Tensor, prompts: list[str] | None, num_inference_steps: int = 50,
                       guidance_scale: float = 7.5, seeds: list[int] | None = None, use_hierarchical: bool = True,
                       ids: tuple | None = None, latents: torch.Tensor | None = None, init_images=None,
                       strength: float = 0.8, posterior_eps: torch.Tensor | None = None,
                       sample_posterior: bool = True, masks=None, composite: bool = True,
                       sampler: str = "ddim") -> torch.Tensor:
        """mel [B, 1001, 64] on device -> uint8 images NHWC [B, H, W, 3] on device.  The
        image size follows the latents ([B, 4, H/8, W/8]; default: the pipeline's size).
        init_images (prepare_images forms; the pipeline's size): image-to-image.  The images are encoded, the
        posterior sampled with posterior_eps [B, 4, H/8, W/8] (None: drawn after each sample's initial noise from
        its seed's generator when sample_posterior, else the mode), noised with `latents` to
        timesteps[t_start] (c2d_vae_posterior_noise, alpha read through the device step counter) and the last
        steps - t_start steps run, t_start = DDIMScheduler.img2img_start(steps, strength).
        masks (prepare_mask_array forms; the pipeline's size) with init_images: inpainting.  One launch
        (c2d_inpaint_prepare) writes the sampler's z0 (the scaled posterior sample or mode), its first latents (z0
        noised to timesteps[t_start], or `latents` themselves when t_start is 0) and its latent mask; the masked
        step (c2d_cfg_ddim_step_masked) runs steps - t_start times; with composite the kept pixels of the decode are
        set back to the init images' bytes (c2d_composite_u8).
        sampler "dpmpp_2m": the same loop on a denoiser of its own whose step ends with c2d_cfg_dpm_step
        (c2d_cfg_dpm_step_masked with masks)."""
        check_sampler(sampler)
        b = mel.shape[0]
        req = self._resolve(b, num_inference_steps, init_images, strength, masks, composite)
        seeds = seeds if seeds is not None else list(range(b))
        if latents is None and req.images is not None and posterior_eps is None and sample_posterior:
            latents, posterior_eps = initial_latents_and_eps(seeds, self.height // 8, self.width // 8, self.device)
        elif latents is None:
            latents = self.initial_latents(seeds)
        if req.images is not None and tuple(latents.shape[-2:]) != (self.height // 8, self.width // 8):
            raise ValueError(f"latents {tuple(latents.shape)} do not match init images {tuple(req.images.shape)}")
        if ids is None:
            ids = (self.tokenizer([""] * b, self.device), self.tokenizer(prompts or [""] * b, self.device))
        ehs, kw, _ = self.condition(mel, ids[0], ids[1], use_hierarchical)
        den = self.denoiser(b, num_inference_steps, guidance_scale, ehs, kw, latent_hw=tuple(latents.shape[-2:]),
                            sampler=sampler)
        den.ehs.copy_(ehs)
        for k, v in kw["audio"].items():
            den.kw["audio"][k].copy_(v)
        moments = self.vae_encoder(req.images) if req.images is not None else None
        den.prepare_context()
        masked = req.masks is not None
        den.ensure_captured(masked)
        eps = posterior_eps.to(self.device, torch.float32).contiguous() if posterior_eps is not None else None
        den.start(latents.to(self.device, torch.float32).contiguous(), req.t_start, moments=moments, eps=eps,
                  mask_u8=req.masks)
        img = self.vae(den.denoise(req.t_start, masked))
        return ops.composite_u8(img, req.images, req.masks, out=img) if req.composite else img

    @torch.no_grad()
    def generate_batch_graphed(self, wave: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor,
                               ids: tuple, latents: torch.Tensor, num_inference_steps: int = 50,
                               guidance_scale: float = 7.5, use_hierarchical: bool = True,
                               slot: int = 0, init_images: torch.Tensor | None = None, strength: float = 0.8,
                               posterior_eps: torch.Tensor | None = None, masks=None,
                               composite: bool = True, sampler: str = "ddim") -> torch.Tensor:
        """generate_batch from device-resident inputs (48 kHz clips concatenated + offsets /
        lengths, token ids, latents) as hipGraphs: one graph for the conditioning leg, the
        denoise-step graph replayed per DDIM step, one graph for the VAE decode (BatchGraph).
        The graphs are built on the first call for a given batch / steps / guidance / size and
        replayed afterwards with the new inputs copied into their static buffers.
        init_images (uint8 [B, H, W, 3] on the device, the latents' size x 8): image-to-image.  The conditioning
        graph then also runs the VAE encoder over a static image buffer, writes the noised latents into the
        sampler state (c2d_vae_posterior_noise; posterior_eps None = the mode) and sets the step counter to
        t_start; steps - t_start replays of the same step graph follow.
        masks (uint8 [B, H, W] on the device, or any prepare_mask_array form) with init_images: inpainting.  The
        conditioning graph then ends with c2d_inpaint_prepare over static image and mask buffers, the steps
        replay the sampler's masked graph, and with composite the decode graph ends with c2d_composite_u8; a
        call with another image or mask copies it into the static buffers and replays the same graphs.
        sampler as generate_batch; it is part of the graphs' key, so the two solvers never share state."""
        check_sampler(sampler)
        req = self._resolve(offsets.numel(), num_inference_steps, init_images, strength, masks, composite)
        key = (offsets.numel(), wave.numel(), num_inference_steps, float(guidance_scale), tuple(latents.shape),
               bool(use_hierarchical), slot, sampler, req.masks is not None, req.composite, req.t_start,
               req.images is not None, posterior_eps is not None)
        bg = self._batch_graphs.get(key)
        if bg is None:
            bg = BatchGraph(self, wave, offsets, lengths, ids, latents, num_inference_steps, guidance_scale,
                            use_hierarchical, slot, req, posterior_eps, sampler)
            self._batch_graphs[key] = bg
        return bg.run(wave, offsets, lengths, ids, latents, req.images, posterior_eps, req.masks)

    @staticmethod
    def to_pil(images: torch.Tensor):
        from PIL import Image
        return [Image.fromarray(im) for im in images.cpu().numpy()]


class BatchGraph:
    """One request batch as hipGraphs (c2 latency path, bench step):
      g_cond -- log-mel (c2d_clap_log_mel) -> HTSAT -> adapter + Norm-60 / legacy hierarchy
                (API fidelity) -> routed tokens -> CLIP text tower -> every cross-attention K|V
                (GraphDenoiser.prepare_context) -> latents into the sampler state;
      the GraphDenoiser step graph, replayed once per DDIM step (device step counter);
      g_vae  -- VAE decode of the final latents into a static uint8 image buffer.
    Inputs are copied into static device buffers, so a replay sees new audio, prompts and
    latents; all workspaces come from the graphs' private pools (allocated at capture).
    With init images (img2img) g_cond also holds the VAE encoder over a static image buffer and
    c2d_vae_posterior_noise writing the sampler state, and sets the step counter to t_start; the step graph
    is the text-to-image one, replayed steps - t_start times.
    With masks as well (inpainting) a static uint8 mask buffer joins the image's; g_cond ends with
    c2d_inpaint_prepare writing the sampler's z0 / x / mask, the copy of the noise into its noise buffer and the
    counter set to t_start; the steps replay the sampler's masked graph; with composite g_vae ends with
    c2d_composite_u8 into the static image."""

    def __init__(self, pipe: AudioToImageInference, wave, offsets, lengths, ids, latents, steps: int,
                 guidance: float, use_hierarchical: bool, slot: int, req: _Request, posterior_eps=None,
                 sampler: str = "ddim"):
        self.pipe, self.use_hier = pipe, use_hierarchical
        self.t_start, self.composite = req.t_start, req.composite
        self.masks = req.masks.clone() if req.masks is not None else None
        self.images = req.images.clone() if req.images is not None else None
        self.eps = posterior_eps.float().clone() if posterior_eps is not None else None
        self.enc = pipe.vae_encoder if self.images is not None else None
        self.wave, self.offs, self.lens = wave.clone(), offsets.clone(), lengths.clone()
        self.ids_u, self.ids_c = ids[0].clone(), ids[1].clone()
        self.lat = latents.float().clone()
        b = self.offs.numel()
        fe = pipe.feature_extractor
        self.mel = torch.empty(b, fe.frames, fe.n_mels, device=pipe.device, dtype=torch.float32)
        # eager warm-up: builds (and captures) the denoiser, caches HTSAT tables, packs lazily
        ehs, kw, _ = pipe.condition(fe.from_device(self.wave, self.offs, self.lens, out=self.mel), self.ids_u,
                                    self.ids_c, use_hierarchical)
        self.den = pipe.denoiser(b, steps, guidance, ehs, kw, latent_hw=tuple(self.lat.shape[-2:]), slot=slot,
                                 sampler=sampler)
        self.den.ehs.copy_(ehs)
        self.den.prepare_context()
        self.den.ensure_captured(self.masks is not None)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._cond()
            self._decode()
        torch.cuda.current_stream().wait_stream(side)
        self.g_cond = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g_cond):
            self._cond()
        self.g_vae = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g_vae):
            self.img = self._decode()

    def _decode(self) -> torch.Tensor:
        img = self.pipe.vae(self.den.x)
        if self.composite:
            ops.composite_u8(img, self.images, self.masks, out=img)
        return img

    def _cond(self) -> None:
        pipe, den = self.pipe, self.den
        mel = pipe.feature_extractor.from_device(self.wave, self.offs, self.lens, out=self.mel)
        ehs, kw, _ = pipe.condition(mel, self.ids_u, self.ids_c, self.use_hier)
        den.ehs.copy_(ehs)
        for k, v in kw["audio"].items():
            den.kw["audio"][k].copy_(v)
        den.prepare_context()
        moments = self.enc(self.images) if self.images is not None else None
        den.start(self.lat, self.t_start, moments=moments, eps=self.eps, mask_u8=self.masks)

    def run(self, wave, offsets, lengths, ids, latents, init_images=None, posterior_eps=None,
            masks=None) -> torch.Tensor:
        pairs = [(self.wave, wave), (self.offs, offsets), (self.lens, lengths), (self.ids_u, ids[0]),
                 (self.ids_c, ids[1]), (self.lat, latents)]
        if self.images is not None:
            pairs.append((self.images, init_images))
        if self.masks is not None:
            pairs.append((self.masks, masks))
        if self.eps is not None:
            pairs.append((self.eps, posterior_eps))
        for dst, src in pairs:
            if src.data_ptr() != dst.data_ptr():
                dst.copy_(src)
        self.g_cond.replay()
        self.den.denoise(self.t_start, self.masks is not None)
        self.g_vae.replay()
        self.pipe.last_denoiser = self.den
        return self.img


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="CLAP2Diffusion Inference (MI355X HIP path)")
    ap.add_argument("--audio", type=str, required=True, help="Path to audio file (or synthetic:<seed>)")
    ap.add_argument("--text", type=str, default="", help="Text prompt")
    ap.add_argument("--output", type=str, default="output.png", help="Output image path")
    ap.add_argument("--checkpoint_dir", type=str, default="../checkpoints", help="Checkpoint directory")
    ap.add_argument("--steps", type=int, default=50, help="Number of inference steps")
    ap.add_argument("--cfg_scale", type=float, default=7.5, help="Guidance scale")
    ap.add_argument("--seed", type=int, default=None, help="Random seed")
    ap.add_argument("--no_hierarchical", action="store_true", help="Disable hierarchical processing")
    ap.add_argument("--sd_model", type=str, default=None, help="diffusers-format SD1.5 folder (unet/, vae/, text_encoder/)")
    ap.add_argument("--clap_model", type=str, default=None, help="ClapModel weights file or folder")
    ap.add_argument("--init_image", type=str, default=None, help="Start from this image (audio-guided img2img)")
    ap.add_argument("--strength", type=float, default=0.8, help="img2img strength in (0, 1]: 1 = ignore the image")
    ap.add_argument("--mask", type=str, default=None,
                    help="Inpaint --init_image: a grey-scale image, >= 128 = repaint, < 128 = keep")
    ap.add_argument("--sampler", type=str, default="ddim", choices=sorted(SAMPLERS),
                    help="Solver of the denoise loop: ddim, or dpmpp_2m (DPM-Solver++(2M), usually 20-25 --steps)")
    ap.add_argument("--no_composite", action="store_true",
                    help="With --mask: return the plain decode instead of pasting the kept pixels back")
    return ap


def main():
    a = build_parser().parse_args()
    if a.mask is not None and a.init_image is None:
        raise SystemExit("--mask needs --init_image")
    pipe = AudioToImageInference(checkpoint_dir=a.checkpoint_dir, sd_model_path=a.sd_model, clap_model_path=a.clap_model)
    img = pipe.generate(audio_path=a.audio, text_prompt=a.text, num_inference_steps=a.steps,
                        guidance_scale=a.cfg_scale, seed=a.seed, use_hierarchical=not a.no_hierarchical,
                        init_image=a.init_image, strength=a.strength, mask=a.mask, composite=not a.no_composite,
                        sampler=a.sampler)
    img.save(a.output)
    print(f"Image saved to {a.output}")


if __name__ == "__main__":
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    main()
