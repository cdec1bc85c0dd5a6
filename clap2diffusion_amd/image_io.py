"""Host-side preparation of init images and inpainting masks: any accepted form -> one uint8 array at the
pipeline's size."""
from __future__ import annotations

import os

import numpy as np
import torch


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


def prepare_image_array(images, height: int, width: int, n: int | None = None) -> np.ndarray:
    """Init image(s) -> uint8 [B, height, width, 3] on the host.  Accepted: a PIL image, a path, a numpy uint8 array
    [H, W, 3], a list of those, or a uint8 tensor [B, H, W, 3]; converted to RGB and resized (bicubic) where the size
    differs.  One image given for n requests is repeated; any other count is a ValueError."""
    from PIL import Image
    if isinstance(images, torch.Tensor):
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
            raise ValueError(f"init images as a tensor must be uint8 [B, H, W, 3], got {images.dtype} "
                             f"{tuple(images.shape)}")
        images = list(images.cpu().numpy())
    arr = []
    for im in (list(images) if isinstance(images, (list, tuple)) else [images]):
        if isinstance(im, (str, os.PathLike)):
            im = Image.open(im)
        elif isinstance(im, np.ndarray):
            im = Image.fromarray(im)
        im = im.convert("RGB")
        if im.size != (width, height):
            im = im.resize((width, height), Image.BICUBIC)
        arr.append(np.asarray(im, dtype=np.uint8))
    out = np.stack(arr)
    if n is not None and out.shape[0] != n:
        if out.shape[0] != 1:
            raise ValueError(f"{out.shape[0]} init images for {n} requests")
        out = np.ascontiguousarray(np.repeat(out, n, axis=0))
    return out
