"""CLIP ViT-L/14 vision tower with its projection on the HIP kernels: the image half of a CLIP score.

Semantics of transformers CLIPVisionModelWithProjection (modeling_clip.py CLIPVisionTransformer):
  uint8 images -> c2d_clip_preprocess (CLIPImageProcessor: resize, centre crop, normalise, patch cut; one launch)
  -> patch-embedding GEMM over the patch rows (no bias; the position embeddings ride its residual epilogue)
  -> class token + its position embedding in row 0 -> pre_layrnorm
  -> per layer LN -> fused QKV GEMM -> c2d_attention_fwd (d = 64, every token sees every token) -> out-proj GEMM
     + residual -> LN -> fc1 GEMM with the quick_gelu epilogue -> fc2 GEMM + residual
  -> post_layernorm on the class rows (a strided view) -> visual_projection (no bias).
The geometry comes from a config dict (weights.CLIP_VISION_CFG, ViT-L/14 by default), the weights from a
CLIPModel-keyed state dict, by default the seeded recipe weights.synth_clip_vision.  There is no torch compute
path; the product never imports transformers.
"""
from __future__ import annotations

import torch

from . import ops
from .layers import HLinear


class ImageEncoder:
    D = 64   # head width of every CLIP ViT; the attention kernel's d

    def __init__(self, device, seed: int = 0, state_dict: dict | None = None, cfg: dict | None = None,
                 mean=ops.CLIP_MEAN, std=ops.CLIP_STD):
        """state_dict: CLIPModel keys (vision_model.*, visual_projection.weight; other keys are ignored);
        default: weights.synth_clip_vision(seed, cfg)."""
        from .weights import CLIP_VISION_CFG, synth_clip_vision
        cfg = dict(cfg or CLIP_VISION_CFG)
        sd = state_dict if state_dict is not None else synth_clip_vision(seed, cfg)
        w, self.heads, self.size, self.patch = cfg["width"], cfg["heads"], cfg["image"], cfg["patch"]
        if w != self.heads * self.D:
            raise ValueError(f"width {w} is not heads {self.heads} x {self.D}")
        if self.size % self.patch:
            raise ValueError(f"image {self.size} is no multiple of patch {self.patch}")
        self.cfg, self.width, self.mean, self.std = cfg, w, tuple(mean), tuple(std)
        self.grid = self.size // self.patch
        self.tokens = self.grid ** 2 + 1
        dev = torch.device(device)
        self.device = dev
        v = "vision_model."
        f32 = lambda k: sd[k].detach().float().contiguous().to(dev)  # noqa: E731
        pos = sd[v + "embeddings.position_embedding.weight"].detach().float()
        if tuple(pos.shape) != (self.tokens, w):
            raise ValueError(f"position embedding {tuple(pos.shape)} for {self.tokens} tokens of width {w}")
        self.pos_patch = pos[1:].half().contiguous().to(dev)
        self.cls_row = (sd[v + "embeddings.class_embedding"].detach().float() + pos[0]).half().to(dev)
        # Conv2d(3, w, patch, stride patch) as a GEMM over c2d_clip_preprocess's rows: K ordered (dy, dx, channel)
        self.patch_embed = HLinear(3 * self.patch ** 2, w, bias=False)
        self.patch_embed.load(sd[v + "embeddings.patch_embedding.weight"].detach().float().permute(0, 2, 3, 1)
                              .reshape(w, -1))
        self.patch_embed.to(dev)
        self.pre_ln = (f32(v + "pre_layrnorm.weight"), f32(v + "pre_layrnorm.bias"))
        self.layers = []
        for i in range(cfg["layers"]):
            b = f"{v}encoder.layers.{i}."
            a = b + "self_attn."
            qkv = HLinear(w, 3 * w)
            qkv.load(torch.cat([sd[a + "q_proj.weight"], sd[a + "k_proj.weight"], sd[a + "v_proj.weight"]]).float(),
                     torch.cat([sd[a + "q_proj.bias"], sd[a + "k_proj.bias"], sd[a + "v_proj.bias"]]).float())
            out, fc1, fc2 = HLinear(w, w), HLinear(w, cfg["mlp"]), HLinear(cfg["mlp"], w)
            out.load(sd[a + "out_proj.weight"].float(), sd[a + "out_proj.bias"].float())
            fc1.load(sd[b + "mlp.fc1.weight"].float(), sd[b + "mlp.fc1.bias"].float())
            fc2.load(sd[b + "mlp.fc2.weight"].float(), sd[b + "mlp.fc2.bias"].float())
            self.layers.append(dict(
                ln1=(f32(b + "layer_norm1.weight"), f32(b + "layer_norm1.bias")),
                ln2=(f32(b + "layer_norm2.weight"), f32(b + "layer_norm2.bias")),
                qkv=qkv.to(dev), out=out.to(dev), fc1=fc1.to(dev), fc2=fc2.to(dev)))
        self.post_ln = (f32(v + "post_layernorm.weight"), f32(v + "post_layernorm.bias"))
        self.proj = HLinear(w, cfg["proj"], bias=False)
        self.proj.load(sd["visual_projection.weight"].float())
        self.proj.to(dev)
        self.eps = 1e-5   # CLIPVisionConfig.layer_norm_eps

    @torch.no_grad()
    def embed_tokens(self, images_u8: torch.Tensor) -> torch.Tensor:
        """uint8 [B, H, W, 3] on the device -> the embeddings' output [B, tokens, width] fp16 (before pre_layrnorm)."""
        n, t, w = images_u8.shape[0], self.tokens, self.width
        rows = ops.clip_preprocess(images_u8.contiguous(), self.size, self.patch, self.mean, self.std)
        x = torch.empty((n, t, w), device=self.device, dtype=torch.float16)
        x[:, 0] = self.cls_row
        per = t - 1
        for b in range(n):   # an image's patch rows land behind its class row: one GEMM per image
            self.patch_embed(rows[b * per:(b + 1) * per], resid=self.pos_patch, out=x[b, 1:])
        return x

    @torch.no_grad()
    def __call__(self, images_u8: torch.Tensor) -> torch.Tensor:
        """uint8 [B, H, W, 3] on the device (any H, W) -> image_embeds fp32 [B, proj] (not normalised)."""
        n, t, c = images_u8.shape[0], self.tokens, self.width
        x = ops.layer_norm(self.embed_tokens(images_u8).view(n * t, c), *self.pre_ln, self.eps)
        for p in self.layers:
            h = ops.layer_norm(x, *p["ln1"], self.eps)
            qkv = p["qkv"](h)
            a = ops.attention(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], n, self.heads, t, t, self.D)
            x = p["out"](a, resid=x)
            h = ops.layer_norm(x, *p["ln2"], self.eps)
            x = p["fc2"](p["fc1"](h, act="quick_gelu"), resid=x)
        pooled = ops.layer_norm(x.view(n, t, c)[:, 0], *self.post_ln, self.eps)
        return self.proj(pooled).float()
