"""float64 restatements for the CLIP-score path (TEST REFERENCE ONLY; numpy / plain torch, no product kernels).

* CLIPImageProcessor: PIL Image.BICUBIC resize of the shorter side to `size` (ImagingResample: separable, the
  horizontal pass first, a = -0.5 cubic, the taps normalised over the part inside the image, the value rounded
  to a byte after each pass), centre crop, (v / 255 - mean) / std, and the ViT patch cut in the K order
  include/c2d.h documents for c2d_clip_preprocess.
* transformers CLIPVisionModelWithProjection / CLIPTextModelWithProjection (modeling_clip.py) from a CLIPModel-keyed
  state dict, and the cosine.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
EOS = 49407


# ------------------------------------------------------------------ preprocess
def _cubic(x: np.ndarray) -> np.ndarray:
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1, ((a + 2) * x - (a + 3)) * x * x + 1,
                    np.where(x < 2, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def resample_matrix(n_in: int, n_out: int, first: int = 0, count: int | None = None) -> np.ndarray:
    """float64 [count, n_in]: row i holds the normalised tap weights of output index first + i."""
    count = n_out - first if count is None else count
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    m = np.zeros((count, n_in), dtype=np.float64)
    for r in range(count):
        centre = (first + r + 0.5) * scale
        lo = max(int(centre - support + 0.5), 0)
        hi = min(int(centre + support + 0.5), n_in)
        j = np.arange(lo, hi, dtype=np.float64)
        w = _cubic((j + 0.5 - centre) / fs)
        m[r, lo:hi] = w / w.sum()
    return m


def _store(v: np.ndarray) -> np.ndarray:
    return np.clip(np.floor(v + 0.5), 0, 255)


def resized_size(h: int, w: int, size: int) -> tuple[int, int]:
    """CLIPImageProcessor: the shorter side becomes size, the longer int(size * long / short)."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    return (new_long, size) if w <= h else (size, new_long)


def resize_bicubic(img: np.ndarray, out_h: int, out_w: int, box=None) -> np.ndarray:
    """uint8 [H, W, C] -> uint8 [out_h, out_w, C] (or the window box = (top, left, height, width) of it)."""
    h, w, _ = img.shape
    top, left, bh, bw = box or (0, 0, out_h, out_w)
    mx = resample_matrix(w, out_w, left, bw)
    my = resample_matrix(h, out_h, top, bh)
    t = _store(np.einsum("xw,hwc->hxc", mx, img.astype(np.float64)))
    return _store(np.einsum("yh,hxc->yxc", my, t)).astype(np.uint8)


def crop_box(h: int, w: int, size: int) -> tuple[int, int, int, int]:
    rh, rw = resized_size(h, w, size)
    return (rh - size) // 2, (rw - size) // 2, size, size


def preprocess_bytes(images: np.ndarray, size: int = 224) -> np.ndarray:
    """uint8 [B, H, W, 3] -> uint8 [B, size, size, 3]: resize and centre crop (only the window is computed)."""
    _, h, w, _ = images.shape
    rh, rw = resized_size(h, w, size)
    return np.stack([resize_bicubic(im, rh, rw, crop_box(h, w, size)) for im in images])


def normalise(pix_u8: np.ndarray, mean=CLIP_MEAN, std=CLIP_STD) -> np.ndarray:
    """uint8 [..., 3] -> float64 (v / 255 - mean) / std."""
    return (pix_u8.astype(np.float64) / 255 - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)


def patch_rows(pix: np.ndarray, patch: int = 14) -> np.ndarray:
    """[B, S, S, 3] -> [B * (S / patch)^2, 3 * patch^2]: row = (image, py, px), column = (dy, dx, channel)."""
    b, s, _, c = pix.shape
    g = s // patch
    return pix.reshape(b, g, patch, g, patch, c).transpose(0, 1, 3, 2, 4, 5).reshape(b * g * g, patch * patch * c)


def preprocess(images: np.ndarray, size: int = 224, patch: int = 14, mean=CLIP_MEAN, std=CLIP_STD) -> np.ndarray:
    """uint8 [B, H, W, 3] -> float64 patch rows [B * (size / patch)^2, 3 * patch^2]."""
    return patch_rows(normalise(preprocess_bytes(images, size), mean, std), patch)


def rows_to_bytes(rows: np.ndarray, mean=CLIP_MEAN, std=CLIP_STD) -> np.ndarray:
    """Patch rows [M, 3 * patch^2] (any float type) -> the bytes they encode, float64 (undo the normalisation, round)."""
    v = rows.astype(np.float64).reshape(rows.shape[0], -1, 3)
    return np.floor((v * np.asarray(std, np.float64) + np.asarray(mean, np.float64)) * 255 + 0.5).reshape(rows.shape)


def noise_images(b: int, h: int, w: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=(b, h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------ towers
def _ln(x, sd, key, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), sd[key + ".weight"], sd[key + ".bias"], eps)


def _encoder(x: torch.Tensor, sd: dict, prefix: str, layers: int, heads: int, causal: bool) -> torch.Tensor:
    """CLIPEncoder: pre-LN blocks, quick_gelu MLP; x [B, T, C]."""
    bsz, t, c = x.shape
    d = c // heads
    mask = torch.full((t, t), float("-inf"), dtype=x.dtype).triu(1) if causal else None
    for i in range(layers):
        b = f"{prefix}encoder.layers.{i}."
        h = _ln(x, sd, b + "layer_norm1")
        q, k, v = (F.linear(h, sd[f"{b}self_attn.{n}_proj.weight"], sd[f"{b}self_attn.{n}_proj.bias"])
                   .view(bsz, t, heads, d).transpose(1, 2) for n in "qkv")
        s = q @ k.transpose(-1, -2) / math.sqrt(d)
        if mask is not None:
            s = s + mask
        a = (s.softmax(-1) @ v).transpose(1, 2).reshape(bsz, t, c)
        x = x + F.linear(a, sd[b + "self_attn.out_proj.weight"], sd[b + "self_attn.out_proj.bias"])
        h = _ln(x, sd, b + "layer_norm2")
        h = F.linear(h, sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"])
        h = h * torch.sigmoid(1.702 * h)
        x = x + F.linear(h, sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"])
    return x


def _cast(sd: dict, dtype) -> dict:
    return {k: v.detach().to(dtype) for k, v in sd.items() if v.is_floating_point()}


@torch.no_grad()
def image_embeds(rows, sd: dict, cfg: dict, dtype=torch.float64) -> torch.Tensor:
    """Patch rows [B * g^2, 3 * patch^2] (preprocess) -> image_embeds [B, proj] in `dtype`: the patch embedding as
    a matrix product over the rows, class token, position embeddings, pre_layrnorm, the encoder, post_layernorm
    on the class token, visual_projection."""
    sd = _cast(sd, dtype)
    v, w, g2 = "vision_model.", cfg["width"], (cfg["image"] // cfg["patch"]) ** 2
    rows = torch.as_tensor(rows).to(dtype)
    wpe = sd[v + "embeddings.patch_embedding.weight"].permute(0, 2, 3, 1).reshape(w, -1)   # K = (dy, dx, channel)
    patches = (rows @ wpe.T).view(-1, g2, w)
    cls = sd[v + "embeddings.class_embedding"].expand(patches.shape[0], 1, w)
    x = torch.cat([cls, patches], 1) + sd[v + "embeddings.position_embedding.weight"]
    x = _ln(x, sd, v + "pre_layrnorm")
    x = _encoder(x, sd, v, cfg["layers"], cfg["heads"], causal=False)
    return _ln(x[:, 0], sd, v + "post_layernorm") @ sd["visual_projection.weight"].T


@torch.no_grad()
def text_embeds(ids: torch.Tensor, sd: dict, layers: int, heads: int, dtype=torch.float64) -> torch.Tensor:
    """ids [B, L] -> text_embeds [B, proj]: the final-LayerNorm row at each prompt's first EOS, text_projection."""
    sd = _cast(sd, dtype)
    t = "text_model."
    ids = ids.cpu().long()
    x = sd[t + "embeddings.token_embedding.weight"][ids] + sd[t + "embeddings.position_embedding.weight"][:ids.shape[1]]
    x = _ln(_encoder(x, sd, t, layers, heads, causal=True), sd, t + "final_layer_norm")
    pooled = x[torch.arange(ids.shape[0]), first_eos(ids)]
    return pooled @ sd["text_projection.weight"].T


def first_eos(ids: torch.Tensor) -> torch.Tensor:
    return (ids == EOS).int().argmax(-1)


def cosine(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    a, b = a.double(), b.double()
    return (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1)).clamp_min(1e-12)
