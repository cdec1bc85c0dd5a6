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

import numpy as np
import torch

from . import weights as W
from .features import ClapLogMel
from .htsat import HTSATEncoder
from .processor import AudioProcessorManager
from .projectors import AudioAdapter, HierarchicalAudioV4, ImprovedHierarchicalAudioEncoder, normalize_tokens
from .sampler import GraphDenoiser
from .scheduler import DDIMScheduler
from .text_encoder import TextEncoder, make_tokenizer
from .unet import UNet2DConditionModel
from .vae import SCALING, VAEDecoder, VAEEncoder
from . import ops

SR = 48000

# Supported image sizes: the UNet halves the 8x-downsampled latent three times and concatenates each level with
# its skip on the way up, so the latent height and width must be multiples of 8 (pixels: of 64); the smallest,
# 64 x 64 pixels (8 x 8 latents, 1 x 1 images at the innermost level), is the smallest the kernel tests cover
# (tests/test_small_shapes_gpu.py, DESIGN.md "Smallest supported shapes").
IMAGE_SIZE_MULTIPLE = 64
MIN_IMAGE_SIZE = 64


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


def synthetic_thunder(seed: int = 0, seconds: float = 10.0, sr: int = SR) -> np.ndarray:
    """SURVEY.md §8(d) stand-in for the LFS-stub assets/Thunder.wav: low-passed white
    noise with three exponentially decaying bursts, peak-normalised."""
    from scipy.signal import lfilter
    rs = np.random.RandomState(seed)
    n = int(seconds * sr)
    y = lfilter([0.005], [1.0, -0.995], rs.randn(n))  # 1-pole IIR low-pass, a = 0.995
    t = np.arange(n) / sr
    env = 0.05 + sum(np.where(t >= t0, np.exp(-(t - t0) / 0.6), 0.0) for t0 in (1.0, 4.5, 7.0))
    y = y * env
    return (y / (np.abs(y).max() + 1e-8)).astype(np.float32)


def initial_latents(seeds: list[int], h: int, w: int, device=None) -> torch.Tensor:
    """Per-sample CPU generator (torch.Generator().manual_seed(seed) -> randn [4, h, w]):
    identical latents on any number of GPUs."""
    lat = [torch.randn(4, h, w, generator=torch.Generator().manual_seed(int(s))) for s in seeds]
    return torch.stack(lat).to(device)


def initial_latents_and_eps(seeds: list[int], h: int, w: int, device=None) -> tuple[torch.Tensor, torch.Tensor]:
    """img2img noise: each sample's generator draws the initial noise (the same tensor initial_latents gives)
    and, right after it, the posterior noise of the VAE encoder's sample."""
    lat, eps = [], []
    for s in seeds:
        g = torch.Generator().manual_seed(int(s))
        lat.append(torch.randn(4, h, w, generator=g))
        eps.append(torch.randn(4, h, w, generator=g))
    return torch.stack(lat).to(device), torch.stack(eps).to(device)


def _mask_planes(m) -> list[np.ndarray]:
    """One mask argument -> its uint8 [H, W] planes (prepare_mask_array's accepted forms, lists aside)."""
    if isinstance(m, torch.Tensor):
        m = m.detach().cpu().numpy()
    if isinstance(m, (str, os.PathLike)):
        from PIL import Image
        m = Image.open(m)
    if not isinstance(m, np.ndarray):
        if not hasattr(m, "convert"):
            raise ValueError(f"a mask must be a PIL image, a path or a uint8 / bool array, got {type(m).__name__}")
        m = np.asarray(m.convert("L"), dtype=np.uint8)
    if m.dtype == np.bool_:
        m = m.astype(np.uint8) * 255
    if m.dtype != np.uint8:
        raise ValueError(f"a mask array must be uint8 (>= 128 = repaint) or bool, got {m.dtype}")
    if m.ndim not in (2, 3):
        raise ValueError(f"a mask array must be [H, W] or [B, H, W], got shape {tuple(m.shape)}")
    return [m] if m.ndim == 2 else list(m)


def prepare_mask_array(masks, height: int, width: int, n: int | None = None) -> np.ndarray:
    """Inpainting mask(s) -> uint8 [B, height, width] on the host, >= 128 = repaint, < 128 = keep.  Accepted: a
    PIL image (converted to "L"), a path, a numpy or torch uint8 array [H, W] / [B, H, W], a bool array
    (True -> 255), or a list of those; resized with NEAREST where the size differs, so the bytes stay the
    mask's own.  One mask given for n requests is repeated; any other count, dtype or rank is a ValueError."""
    planes = []
    for m in (masks if isinstance(masks, (list, tuple)) else [masks]):
        planes.extend(_mask_planes(m))
    if not planes:
        raise ValueError("no mask given")
    for k, m in enumerate(planes):
        if m.shape != (height, width):
            from PIL import Image
            planes[k] = np.asarray(Image.fromarray(np.ascontiguousarray(m)).resize((width, height), Image.NEAREST),
                                   dtype=np.uint8)
    out = np.ascontiguousarray(np.stack(planes), dtype=np.uint8)
    if n is not None and out.shape[0] != n:
        if out.shape[0] != 1:
            raise ValueError(f"{out.shape[0]} masks for {n} requests")
        out = np.ascontiguousarray(np.repeat(out, n, axis=0))
    return out


_WAVE_PCM, _WAVE_FLOAT, _WAVE_EXTENSIBLE = 1, 3, 0xFFFE


def _read_wav(path: str, max_seconds: float | None = None) -> tuple[np.ndarray, int]:
    """RIFF/WAVE reader -> (mono float32 in [-1, 1], native rate): PCM 8 (unsigned) / 16 / 24 / 32-bit,
    IEEE float 32 / 64-bit, WAVE_FORMAT_EXTENSIBLE of either; channels averaged (librosa mono=True).
    max_seconds: keep the first max_seconds of the file at its native rate (librosa's duration=,
    applied before resampling as librosa.load does).  read_audio adds AIFF / AIFC and Sun AU; other
    containers (mp3, flac, ...) need a decoder this image does not have: convert them first."""
    data = Path(path).read_bytes()
    if data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file (only WAV is decoded without librosa)")
    fmt = None
    pos = 12
    body = None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], int.from_bytes(data[pos + 4:pos + 8], "little")
        chunk = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            tag, ch, sr = int.from_bytes(chunk[0:2], "little"), int.from_bytes(chunk[2:4], "little"), \
                int.from_bytes(chunk[4:8], "little")
            bits = int.from_bytes(chunk[14:16], "little")
            if tag == _WAVE_EXTENSIBLE and len(chunk) >= 26:
                tag = int.from_bytes(chunk[24:26], "little")   # first two bytes of the SubFormat GUID
            fmt = (tag, ch, sr, bits)
        elif cid == b"data":
            body = chunk
        pos += 8 + size + (size & 1)
    if fmt is None or body is None:
        raise ValueError(f"{path}: WAV without fmt / data chunk")
    tag, ch, sr, bits = fmt
    bps = bits // 8
    frames = len(body) // (bps * ch)
    if max_seconds is not None:
        frames = min(frames, int(max_seconds * sr))
    body = body[: frames * bps * ch]
    if tag == _WAVE_FLOAT and bits in (32, 64):
        x = np.frombuffer(body, dtype=np.float32 if bits == 32 else np.float64).astype(np.float32)
    elif tag == _WAVE_PCM and bits == 8:
        x = (np.frombuffer(body, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif tag == _WAVE_PCM and bits in (16, 32):
        x = np.frombuffer(body, dtype=np.int16 if bits == 16 else np.int32).astype(np.float32) / float(2 ** (bits - 1))
    elif tag == _WAVE_PCM and bits == 24:
        b = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) / float(1 << 23)
    else:
        raise ValueError(f"{path}: unsupported WAV encoding (format tag {tag}, {bits} bits)")
    return x.reshape(-1, ch).mean(axis=1), sr


def _pcm_to_float(raw: bytes, width: int, big: bool) -> np.ndarray:
    """Signed linear PCM of `width` bytes per sample -> float32 in [-1, 1)."""
    if width == 1:
        return np.frombuffer(raw, dtype=np.int8).astype(np.float32) / 128.0
    if width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = (b[:, 0] << 16 | b[:, 1] << 8 | b[:, 2]) if big else (b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16)
        return (np.where(v >= 1 << 23, v - (1 << 24), v)).astype(np.float32) / float(1 << 23)
    dt = {2: "i2", 4: "i4"}[width]
    return np.frombuffer(raw, dtype=(">" if big else "<") + dt).astype(np.float32) / float(2 ** (8 * width - 1))


def _read_stdlib(mod, path: str, max_seconds: float | None) -> tuple[np.ndarray, int]:
    """AIFF / AIFC (aifc) and Sun AU (sunau) through the standard library's readers: linear PCM
    8 / 16 / 24 / 32-bit (big-endian; AIFC 'sowt' comes back big-endian from aifc) and the
    companded codecs those modules expand to native-endian 16-bit (u-law / a-law / G.722)."""
    with mod.open(path, "rb") as f:
        ch, width, sr, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        if max_seconds is not None:
            n = min(n, int(max_seconds * sr))
        raw = f.readframes(n)
        comp = f.getcomptype()
    comp = comp.decode() if isinstance(comp, bytes) else str(comp)
    big = comp.upper() in ("NONE", "SOWT") or comp == "not compressed"
    if width not in (1, 2, 3, 4):
        raise ValueError(f"{path}: unsupported sample width {width}")
    x = _pcm_to_float(raw[: len(raw) // (width * ch) * width * ch], width, big)
    return x.reshape(-1, ch).mean(axis=1), sr


def read_audio(path: str, max_seconds: float | None = None) -> tuple[np.ndarray, int]:
    """(mono float32, native rate) of a WAV, AIFF / AIFC or Sun AU file, chosen by its header (the
    containers this image decodes without librosa; reference scripts/inference.py:78 reads any
    format librosa does).  max_seconds: keep the first max_seconds at the native rate."""
    head = Path(path).read_bytes()[:12]
    if head[:4] == b"RIFF" and head[8:12] == b"WAVE":
        return _read_wav(path, max_seconds)
    import warnings
    with warnings.catch_warnings():   # aifc / sunau are deprecated from Python 3.11 on
        warnings.simplefilter("ignore", DeprecationWarning)
        if head[:4] == b"FORM" and head[8:12] in (b"AIFF", b"AIFC"):
            import aifc
            return _read_stdlib(aifc, path, max_seconds)
        if head[:4] == b".snd":
            import sunau
            return _read_stdlib(sunau, path, max_seconds)
    raise ValueError(f"{path}: not a RIFF/WAVE, AIFF/AIFC or Sun AU file (other formats need a decoder this "
                     "image does not have: convert them first)")


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
        """PIL image(s), path(s) or a uint8 tensor [B, H, W, 3] -> uint8 [B, H, W, 3] on the device at the
        pipeline's size: converted to RGB and resized on the host (bicubic) where the size differs.  One
        image given for n requests is repeated."""
        if isinstance(images, torch.Tensor):
            if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
                raise ValueError(f"init images as a tensor must be uint8 [B, H, W, 3], got {images.dtype} "
                                 f"{tuple(images.shape)}")
            if tuple(images.shape[1:3]) == (self.height, self.width):
                out = images.to(self.device).contiguous()
            else:
                images = list(images.cpu().numpy())
        if not isinstance(images, torch.Tensor):
            from PIL import Image
            arr = []
            for im in (list(images) if isinstance(images, (list, tuple)) else [images]):
                if isinstance(im, (str, os.PathLike)):
                    im = Image.open(im)
                elif isinstance(im, np.ndarray):
                    im = Image.fromarray(im)
                im = im.convert("RGB")
                if im.size != (self.width, self.height):
                    im = im.resize((self.width, self.height), Image.BICUBIC)
                arr.append(np.asarray(im, dtype=np.uint8))
            out = torch.from_numpy(np.stack(arr)).to(self.device)
        if n is not None and out.shape[0] != n:
            if out.shape[0] != 1:
                raise ValueError(f"{out.shape[0]} init images for {n} requests")
            out = out.expand(n, -1, -1, -1).contiguous()
        return out

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

    @staticmethod
    def _check_masks(masks: torch.Tensor, imgs: torch.Tensor | None) -> None:
        if imgs is None:
            raise ValueError("a mask needs an init image: inpainting repaints a region of it (init_image= / init_images=)")
        if tuple(masks.shape) != tuple(imgs.shape[:3]):
            raise ValueError(f"masks {tuple(masks.shape)} do not match init images {tuple(imgs.shape)}")

    def _request_latents(self, n: int, seed, with_eps: bool = False):
        """Initial latents of n requests as the reference's generate() seeds them
        (scripts/inference.py:113-116: torch.manual_seed(seed) / np.random.seed(seed) when a seed
        is given, the RNG left as it is otherwise): each request draws [1, 4, h/8, w/8] from the
        global CPU generator right after its (re-)seeding, so a given seed always yields
        initial_latents([seed]) and seed=None draws fresh noise every call.  with_eps (img2img with a sampled
        posterior): each request draws its posterior noise right after its initial noise, so a seed fixes
        both; returns (latents, eps)."""
        h, w = self.height // 8, self.width // 8
        lat, eps = [], []
        for _ in range(n):
            if seed is not None:
                torch.manual_seed(seed)
                np.random.seed(seed)
            lat.append(torch.randn(1, 4, h, w))
            if with_eps:
                eps.append(torch.randn(1, 4, h, w))
        if with_eps:
            return torch.cat(lat).to(self.device), torch.cat(eps).to(self.device)
        return torch.cat(lat).to(self.device)

    @torch.no_grad()
    def generate(self, audio_path, text_prompt="", num_inference_steps=50, guidance_scale=7.5, seed=None,
                 use_hierarchical=True, init_image=None, strength=0.8, sample_posterior=True, mask=None,
                 composite=True):
        """init_image (a PIL image, a path or a uint8 tensor [1, H, W, 3]): audio-guided image-to-image, the
        schedule entered at DDIMScheduler.img2img_start(steps, strength) from the encoded image plus scheduled
        noise; sample_posterior=False takes the VAE posterior's mode instead of a sample.
        mask (prepare_mask_array forms; >= 128 = repaint, < 128 = keep) with init_image: audio-guided inpainting
        (diffusers StableDiffusionInpaintPipeline with a 4-channel UNet): after every step the kept latents are
        set back to the image's, re-noised to that step; strength 1 starts from pure noise.  composite: the kept
        pixels of the result are the init image's own bytes, else the plain decode."""
        if mask is not None and init_image is None:
            raise ValueError("mask= needs init_image=: inpainting repaints a region of that image")
        audio = self.load_audio(audio_path)
        if init_image is None:
            img = self.generate_batch(self.mel_features([audio]), [text_prompt], num_inference_steps, guidance_scale,
                                      use_hierarchical=use_hierarchical, latents=self._request_latents(1, seed))
            return self.to_pil(img)[0]
        lat, eps = self._request_latents(1, seed, with_eps=True)
        img = self.generate_batch(self.mel_features([audio]), [text_prompt], num_inference_steps, guidance_scale,
                                  use_hierarchical=use_hierarchical, latents=lat, init_images=init_image,
                                  strength=strength, posterior_eps=eps if sample_posterior else None,
                                  masks=mask, composite=composite)
        return self.to_pil(img)[0]

    def batch_generate(self, audio_paths, text_prompts=None, **kwargs):
        """The reference runs generate(path, prompt, **kwargs) per item (scripts/inference.py:168-180),
        so every item is re-seeded with the same seed (the same initial noise for every item) and
        seed=None leaves the RNG unseeded; here the items run as one batch with those latents."""
        if text_prompts is None:
            text_prompts = [""] * len(audio_paths)
        steps = kwargs.get("num_inference_steps", 50)
        g = kwargs.get("guidance_scale", 7.5)
        seed = kwargs.get("seed", None)
        mel = self.mel_features([self.load_audio(p) for p in audio_paths])
        init_images = kwargs.get("init_images", None)
        masks = kwargs.get("masks", None)   # masks= (one per item, or one for all), composite= as generate()
        if masks is not None and init_images is None:
            raise ValueError("masks= needs init_images=: inpainting repaints a region of those images")
        if init_images is None:
            img = self.generate_batch(mel, list(text_prompts), steps, g,
                                      use_hierarchical=kwargs.get("use_hierarchical", True),
                                      latents=self._request_latents(len(audio_paths), seed))
            return self.to_pil(img)
        # init_images= (one per item, or one for all), strength=, sample_posterior= as generate()
        lat, eps = self._request_latents(len(audio_paths), seed, with_eps=True)
        img = self.generate_batch(mel, list(text_prompts), steps, g,
                                  use_hierarchical=kwargs.get("use_hierarchical", True), latents=lat,
                                  init_images=init_images, strength=kwargs.get("strength", 0.8),
                                  posterior_eps=eps if kwargs.get("sample_posterior", True) else None,
                                  masks=masks, composite=kwargs.get("composite", True))
        return self.to_pil(img)

    # ------------------------------------------------------------ batched core
    def initial_latents(self, seeds: list[int]) -> torch.Tensor:
        """Per-sample CPU generator (seed) -> identical latents on any number of GPUs."""
        return initial_latents(seeds, self.height // 8, self.width // 8, self.device)

    def denoiser(self, b: int, steps: int, guidance: float, ehs, audio_kwargs, latent_hw=None,
                 slot: int = 0) -> GraphDenoiser:
        """The captured-graph denoise loop for (batch, steps, guidance, latent size), built once;
        `slot` keeps separate sampler states for batches run concurrently on different streams."""
        h, w = latent_hw or (self.height // 8, self.width // 8)
        check_latent_size(h, w)   # latent_hw= and caller-supplied latents (generate_batch, BatchGraph) come through here
        key = (b, steps, float(guidance), h, w, slot)
        d = self._denoisers.get(key)
        if d is None:
            sch = DDIMScheduler()
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
                       sample_posterior: bool = True, masks=None, composite: bool = True) -> torch.Tensor:
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
        set back to the init images' bytes (c2d_composite_u8)."""
        if masks is not None and init_images is None:
            raise ValueError("masks= needs init_images=: inpainting repaints a region of those images")
        b = mel.shape[0]
        if ids is None:
            ids = (self.tokenizer([""] * b, self.device), self.tokenizer(prompts or [""] * b, self.device))
        ehs, kw, _ = self.condition(mel, ids[0], ids[1], use_hierarchical)
        t_start = 0
        if init_images is not None:
            t_start = DDIMScheduler.img2img_start(num_inference_steps, strength)
            imgs = self.prepare_images(init_images, b)
            if masks is not None:
                masks = self.prepare_masks(masks, b)
                self._check_masks(masks, imgs)
            if latents is None and posterior_eps is None and sample_posterior:
                latents, posterior_eps = initial_latents_and_eps(seeds if seeds is not None else list(range(b)),
                                                                 self.height // 8, self.width // 8, self.device)
        if latents is None:
            latents = self.initial_latents(seeds if seeds is not None else list(range(b)))
        den = self.denoiser(b, num_inference_steps, guidance_scale, ehs, kw, latent_hw=tuple(latents.shape[-2:]))
        den.ehs.copy_(ehs)
        for k, v in kw["audio"].items():
            den.kw["audio"][k].copy_(v)
        if init_images is None:
            x = den.run(latents * self.scheduler.init_noise_sigma)
            return self.vae(x)
        if tuple(latents.shape[-2:]) != (imgs.shape[1] // 8, imgs.shape[2] // 8):
            raise ValueError(f"latents {tuple(latents.shape)} do not match init images {tuple(imgs.shape)}")
        noise = latents.to(self.device, torch.float32).contiguous()
        eps = posterior_eps.to(self.device, torch.float32).contiguous() if posterior_eps is not None else None
        den.step_idx.fill_(t_start)   # the kernel reads the alpha of the first step that runs through the counter
        if masks is not None:
            den.masked_buffers()
            # t_start 0 (strength 1): the loop starts from the noise itself (init_noise_sigma is 1 for DDIM)
            ops.inpaint_prepare(self.vae_encoder(imgs), noise, masks, SCALING, eps=eps, coef=den.coef,
                                step_index=den.step_idx, pure_noise=t_start == 0, z0=den.z0, x=den.x, mask=den.mask)
            den.noise.copy_(noise)
            img = self.vae(den.run(None, start=t_start, masked=True))
            return ops.composite_u8(img, imgs, masks, out=img) if composite else img
        x0 = ops.vae_posterior_noise(self.vae_encoder(imgs), torch.empty_like(noise), SCALING, eps=eps, noise=noise,
                                     coef=den.coef, step_index=den.step_idx)
        return self.vae(den.run(x0, start=t_start))

    @torch.no_grad()
    def generate_batch_graphed(self, wave: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor,
                               ids: tuple, latents: torch.Tensor, num_inference_steps: int = 50,
                               guidance_scale: float = 7.5, use_hierarchical: bool = True,
                               slot: int = 0, init_images: torch.Tensor | None = None, strength: float = 0.8,
                               posterior_eps: torch.Tensor | None = None, masks=None,
                               composite: bool = True) -> torch.Tensor:
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
        call with another image or mask copies it into the static buffers and replays the same graphs."""
        if masks is not None and init_images is None:
            raise ValueError("masks= needs init_images=: inpainting repaints a region of those images")
        t_start = 0
        if init_images is not None:
            t_start = DDIMScheduler.img2img_start(num_inference_steps, strength)
            init_images = self.prepare_images(init_images, offsets.numel())
        if masks is not None:
            masks = self.prepare_masks(masks, offsets.numel())
            self._check_masks(masks, init_images)
        composite = bool(composite) and masks is not None
        key = (offsets.numel(), wave.numel(), num_inference_steps, float(guidance_scale), tuple(latents.shape),
               bool(use_hierarchical), slot, masks is not None, composite, t_start, init_images is not None,
               posterior_eps is not None)
        bg = self._batch_graphs.get(key)
        if bg is None:
            bg = BatchGraph(self, wave, offsets, lengths, ids, latents, num_inference_steps, guidance_scale,
                            use_hierarchical, slot, init_images, t_start, posterior_eps, masks, composite)
            self._batch_graphs[key] = bg
        return bg.run(wave, offsets, lengths, ids, latents, init_images, posterior_eps, masks)

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
                 guidance: float, use_hierarchical: bool, slot: int = 0, init_images=None, t_start: int = 0,
                 posterior_eps=None, masks=None, composite: bool = True):
        self.pipe, self.steps, self.use_hier = pipe, steps, use_hierarchical
        self.t_start = t_start
        if masks is not None and init_images is None:
            raise ValueError("masks need init images")
        self.masks = masks.clone() if masks is not None else None
        self.composite = bool(composite) and masks is not None
        self.images = init_images.clone() if init_images is not None else None
        self.eps = posterior_eps.float().clone() if posterior_eps is not None else None
        self.enc = pipe.vae_encoder if init_images is not None else None
        self.wave, self.offs, self.lens = wave.clone(), offsets.clone(), lengths.clone()
        self.ids_u, self.ids_c = ids[0].clone(), ids[1].clone()
        self.lat = latents.float().clone()
        b = self.offs.numel()
        fe = pipe.feature_extractor
        self.mel = torch.empty(b, fe.frames, fe.n_mels, device=pipe.device, dtype=torch.float32)
        # eager warm-up: builds (and captures) the denoiser, caches HTSAT tables, packs lazily
        ehs, kw, _ = pipe.condition(fe.from_device(self.wave, self.offs, self.lens, out=self.mel), self.ids_u,
                                    self.ids_c, use_hierarchical)
        self.den = pipe.denoiser(b, steps, guidance, ehs, kw, latent_hw=tuple(self.lat.shape[-2:]), slot=slot)
        self.den.ehs.copy_(ehs)
        self.den.prepare_context()
        if self.den.use_graph and self.den.graph is None:
            self.den.capture()
        if self.masks is not None:
            self.den.masked_buffers()
            if self.den.use_graph and self.den.graph_masked is None:
                self.den.capture_masked()
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
        if self.images is None:
            den.x.copy_(self.lat * pipe.scheduler.init_noise_sigma)
            den.step_idx.zero_()
            return
        den.step_idx.fill_(self.t_start)
        if self.masks is not None:
            ops.inpaint_prepare(self.enc(self.images), self.lat, self.masks, SCALING, eps=self.eps, coef=den.coef,
                                step_index=den.step_idx, pure_noise=self.t_start == 0, z0=den.z0, x=den.x,
                                mask=den.mask)
            den.noise.copy_(self.lat)
            return
        ops.vae_posterior_noise(self.enc(self.images), den.x, SCALING, eps=self.eps, noise=self.lat, coef=den.coef,
                                step_index=den.step_idx)

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
        for _ in range(self.steps - self.t_start):
            if self.masks is not None:
                self.den.step_masked()
            else:
                self.den.graph.replay() if self.den.use_graph else self.den._body()
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
                        init_image=a.init_image, strength=a.strength, mask=a.mask, composite=not a.no_composite)
    img.save(a.output)
    print(f"Image saved to {a.output}")


if __name__ == "__main__":
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    main()
