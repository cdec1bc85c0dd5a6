"""CLIP score on the HIP kernels: the cosine between CLIP ViT-L/14's image and text embeddings.

ClipScorer holds the vision tower (image_encoder.ImageEncoder), a text tower of its own (text_encoder.TextEncoder
built from the CLIP checkpoint's text_model.*, so the pipeline's text encoder is never touched) and the
text_projection.  Images are the sampler's uint8 [B, H, W, 3] device tensors as they are: resize, crop,
normalise and patch cut happen in one launch (c2d_clip_preprocess), the cosine in another (c2d_cosine_rows).

Without a CLIP checkpoint the weights are the seeded recipe weights.synth_clip_model, and without a vocabulary
the prompts map to hash ids (text_encoder.tokenize): the score is then deterministic and meaningless, as the
images of the seeded pipeline are.  It measures something only with real CLIP weights (clip_model_path) and the
CLIP BPE tokenizer.
"""
from __future__ import annotations

import torch

from . import ops
from .image_encoder import ImageEncoder
from .layers import HLinear
from .text_encoder import EOS, TextEncoder, tokenize


class ClipScorer:
    def __init__(self, device, clip_model_path=None, seed: int = 0, tokenizer=None):
        """clip_model_path: a transformers CLIPModel folder or weights file (openai/clip-vit-large-patch14);
        None: weights.synth_clip_model(seed).  tokenizer: prompts, device -> ids [B, 77] (make_tokenizer's
        result; default the hash-id fallback)."""
        from . import weights as W
        sd = W.load_clip_model(clip_model_path) if clip_model_path else W.synth_clip_model(seed)
        self.device = torch.device(device)
        self.image_encoder = ImageEncoder(self.device, state_dict=sd)
        self.text_encoder = TextEncoder(self.device, state_dict={k: v for k, v in sd.items()
                                                                 if k.startswith("text_model.")})
        tp = sd["text_projection.weight"].detach().float()
        self.text_projection = HLinear(tp.shape[1], tp.shape[0], bias=False)
        self.text_projection.load(tp)
        self.text_projection.to(self.device)
        self.tokenizer = tokenizer or tokenize

    def tokenize(self, prompts: list[str]) -> torch.Tensor:
        return self.tokenizer(list(prompts), self.device)

    def _images(self, images_u8: torch.Tensor) -> torch.Tensor:
        if images_u8.dim() == 3:
            images_u8 = images_u8[None]
        return images_u8.to(self.device).contiguous()

    @torch.no_grad()
    def image_embeds(self, images_u8: torch.Tensor) -> torch.Tensor:
        """uint8 [B, H, W, 3] (any H, W) -> fp32 [B, 768], CLIPModel.get_image_features (not normalised)."""
        return self.image_encoder(self._images(images_u8))

    @torch.no_grad()
    def text_embeds(self, ids: torch.Tensor) -> torch.Tensor:
        """ids [B, 77] -> fp32 [B, 768], CLIPModel.get_text_features: the final-LayerNorm row at each prompt's
        first EOS (transformers' pooled output), then text_projection."""
        ids = ids.to(self.device)
        hidden = self.text_encoder(ids)
        eos = (ids == EOS).int().argmax(-1)
        pooled = hidden[torch.arange(ids.shape[0], device=self.device), eos]
        return self.text_projection(pooled.contiguous()).float()

    @torch.no_grad()
    def score(self, images_u8: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
        """-> fp32 [B] on the device: cosine(image_embeds[i], text_embeds[i])."""
        return ops.cosine_rows(self.image_embeds(images_u8), self.text_embeds(ids))

    @torch.no_grad()
    def image_similarity(self, a_u8: torch.Tensor, b_u8: torch.Tensor) -> torch.Tensor:
        """-> fp32 [B]: the same cosine between two image batches."""
        return ops.cosine_rows(self.image_embeds(a_u8), self.image_embeds(b_u8))
