"""Torch-facing API over the C ABI (include/c2d.h), through the torch.library ops.

Tensors are plain device buffers here: activations NHWC / row-major fp16,
statistics fp32.  Each function checks its operands, allocates the outputs and
calls the registered ``torch.ops.c2d.*`` operator (clap2diffusion_amd.torch_ops),
whose CUDA implementation launches the HIP kernel on torch's current stream, so
the calls can be captured into a torch.cuda.CUDAGraph (hipGraph) as is.
"""
from __future__ import annotations

import ctypes
import functools
import math
import os

import torch

from . import torch_ops  # noqa: F401  (registers the c2d:: operators)
from ._lib import C2D_ACT, C2D_PRO_LNFOLD, ConvDesc, check, lib

C2D = torch.ops.c2d

F16 = torch.float16


def _require(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a device tensor (HIP path only, no CPU fallback)")


# ----------------------------------------------------------------- packing
def kpad_of(k: int) -> int:
    return (k + 63) // 64 * 64


def pack_conv_weight(w: torch.Tensor, cin_pad: int | None = None) -> tuple[torch.Tensor, int]:
    """[cout, cin, kh, kw] -> fp16 [cout][kpad] with K ordered (ky, kx, cin)."""
    cout, cin, kh, kw = w.shape
    if cin_pad and cin_pad > cin:
        w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, cin_pad - cin))
        cin = cin_pad
    k = kh * kw * cin
    wp = w.permute(0, 2, 3, 1).reshape(cout, k)
    kp = kpad_of(k)
    if kp > k:
        wp = torch.nn.functional.pad(wp, (0, kp - k))
    return wp.to(F16).contiguous(), kp


def pack_weights_device(w: torch.Tensor, cin_pad: int | None = None) -> tuple[torch.Tensor, int]:
    """c2d_pack_weights: the on-device form of pack_conv_weight / pack_linear_weight
    (fp32 weight already on the GPU -> fp16 [cout][kpad])."""
    _require(w, "w")
    w = w.float().contiguous()
    cout, cin = w.shape[:2]
    ks = w.shape[2] if w.dim() == 4 else 1
    cp = max(cin_pad or cin, cin)
    kp = kpad_of(ks * ks * cp)
    out = torch.empty(cout, kp, device=w.device, dtype=F16)
    C2D.pack_weights(w, cout, cin, ks, cp, kp, out)
    return out, kp


def pack_linear_weight(w: torch.Tensor) -> tuple[torch.Tensor, int]:
    """[out, in] -> fp16 [out][kpad]."""
    out_f, in_f = w.shape
    kp = kpad_of(in_f)
    wp = torch.nn.functional.pad(w, (0, kp - in_f)) if kp > in_f else w
    return wp.to(F16).contiguous(), kp


# nearest x2 followed by a 3x3 (pad 1): output pixel (2i + a, 2j + b) reads only a 2x2 low-res neighbourhood;
# _UPFOLD_TAPS[a][t] = the 3x3 taps along one axis that land on 2x2 tap t of phase a
_UPFOLD_TAPS = (((0,), (1, 2)), ((0, 1), (2,)))


@torch.no_grad()
def fold_upsample_weight(w: torch.Tensor, dtype: torch.dtype = F16) -> tuple[torch.Tensor, int]:
    """Upsample2D's [cout, cin, 3, 3] weight -> the four 2x2 phase convs of the low-res image
    (c2d_conv_desc::up = 2): [4][cout][kpad = 4 cin], phase 2a + b, K ordered (ty, tx, cin).  Tap (ty, tx) of
    output (2i + a, 2j + b) reads low-res pixel (i + a - 1 + ty, j + b - 1 + tx).  Summed in w's dtype (the
    fp32 checkpoint weights) and rounded to `dtype` once."""
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3
    out = w.new_zeros(4, cout, 2, 2, cin)
    for a in range(2):
        for b in range(2):
            for ty in range(2):
                for tx in range(2):
                    acc = out[2 * a + b, :, ty, tx, :]
                    for ky in _UPFOLD_TAPS[a][ty]:
                        for kx in _UPFOLD_TAPS[b][tx]:
                            acc += w[:, :, ky, kx]
    return out.reshape(4, cout, 4 * cin).to(dtype).contiguous(), 4 * cin


def _shape_desc(n: int, h: int, w: int, c0: int, cout: int, ksize: int, *, c1: int = 0, oh: int | None = None,
                ow: int | None = None, stride: int = 1, up: int = 0, kpad: int | None = None, act: str | None = None,
                out_ld: int | None = None, src_pad: bool = False, lnfold: bool = False, resid: bool = False,
                temb: bool = False, groups: int = 0, operands: bool = False) -> ConvDesc:
    """A c2d_conv_desc of shapes and flags for the planner's queries, which read no memory: output oh x ow (h x w
    unless given), kpad of the plain K = ksize^2 (c0 + c1), out_ld = cout.  resid / temb: a 16-B aligned stand-in of
    leading dimension cout; operands: the same for out and src1, and a workspace that holds any split, as ops.conv
    passes them (the queries only test pointers for presence and alignment)."""
    d = ConvDesc()
    d.c0, d.c1, d.n, d.h, d.w, d.oh, d.ow = c0, c1, n, h, w, (h if oh is None else oh), (w if ow is None else ow)
    d.ksize, d.stride, d.up, d.src_pad, d.act = ksize, stride, up, int(src_pad), C2D_ACT[act]
    d.cout, d.kpad = cout, (kpad_of(ksize * ksize * (c0 + c1)) if kpad is None else kpad)
    d.out_ld, d.gn_groups = (cout if out_ld is None else out_ld), groups
    if lnfold:
        d.pro, d.pro_eps = C2D_PRO_LNFOLD, 1e-5
    if resid:
        d.resid, d.resid_ld = 256, cout
    if temb:
        d.temb, d.temb_ld = 256, cout
    if operands:
        d.out, d.ws, d.ws_bytes = 256, 256, 1 << 40
        if c1:
            d.src1 = 256
    return d


def _plan_query(d: ConvDesc) -> tuple[int, int, int]:
    """c2d_conv2d_igemm_plan -> (return code, tile id, K slices)."""
    tid, ks = ctypes.c_int(), ctypes.c_int()
    rc = lib().c2d_conv2d_igemm_plan(ctypes.byref(d), ctypes.byref(tid), ctypes.byref(ks))
    return rc, tid.value, ks.value


@functools.lru_cache(maxsize=None)
def upfold_ok(n: int, h: int, w: int, cin: int, cout: int) -> bool:
    """Does the library take this Upsample2D conv as a folded upsample (c2d_conv_desc::up = 2)?  Not with
    cin % 64 != 0, nor a build without the mode: the caller then materialises the x2 tensor."""
    return _plan_query(_shape_desc(n, h, w, cin, cout, 3, oh=2 * h, ow=2 * w, up=2, kpad=4 * cin))[0] == 0


def geglu_interleave(w: torch.Tensor, b: torch.Tensor | None):
    """GEGLU proj [2I, in] (rows: h then g, diffusers chunk(2, -1)) -> rows in
    32-row blocks [h(16) | g(16)] so one MFMA column tile pair yields h*gelu(g)."""
    two_i = w.shape[0]
    inner = two_i // 2
    assert inner % 16 == 0
    idx = torch.arange(two_i).view(2, inner // 16, 16).permute(1, 0, 2).reshape(-1)
    wi = w[idx]
    bi = b[idx] if b is not None else None
    return wi, bi


# ----------------------------------------------------------------- kernels
def conv(x: torch.Tensor, weight: torch.Tensor, kpad: int, cout: int, *, ksize: int, bias=None, stride: int = 1,
         up: bool = False, x2: torch.Tensor | None = None, gn=None, gn_silu: bool = False, ln=None,
         silu_in: bool = False, act: str | None = None, temb: torch.Tensor | None = None,
         resid: torch.Tensor | None = None, out: torch.Tensor | None = None, padded: bool = False,
         ln_fold=None, gn_moments: int = 0, up_fold: bool = False, pad_after: bool = False):
    """Implicit-GEMM conv / linear (c2d::conv2d_igemm).

    x: NHWC [N, H, W, C0] fp16 (or 2-D [M, C0] for a linear layer); padded: x is the
    zero-bordered [N, H + 2, W + 2, C0] of group_norm(pad=True) (3x3, stride 1, one source).
    gn: (scale, shift) fp32 [N, C0+C1]; ln: (stats [M, 2], gamma, beta).
    ln_fold: eps of a LayerNorm folded into this linear: x is the LayerNorm's raw input
    (weight = W diag(gamma), bias = b + W beta; fold_layernorm builds them), panel GEMM shapes only.
    gn_moments = G > 0: also have the conv emit the GroupNorm moments of its output over G groups
    where the library can (c2d_conv2d_gn_rows); returns (out, GnMoments or None) instead of out.
    up_fold: the folded upsample (c2d_conv_desc::up = 2): x is the low-res tensor, weight the phase pack of
    fold_upsample_weight, the output [N, 2H, 2W, cout]; `up` keeps its meaning (the nearest-x2 view).
    pad_after: the AutoencoderKL encoder's downsample (c2d_conv_desc::pad_mode = C2D_PAD_AFTER): 3x3, stride 2,
    F.pad(x, (0, 1, 0, 1)) then padding 0, without the padded tensor; H and W even, output [N, H/2, W/2, cout].
    """
    _require(x, "x")
    if x.dim() == 2:
        h, w = 1, x.shape[0]
    else:
        _, h, w, _ = x.shape
        if padded:
            assert ksize == 3 and stride == 1 and not up and x2 is None, "padded source: 3x3, stride 1, one source"
            # the zero border is data to the kernels (pad 0): a prologue would map it to shift / SiLU(shift)
            assert gn is None and ln is None and not silu_in, "padded source: no GN / LN / SiLU prologue"
            h, w = h - 2, w - 2
    assert x.is_contiguous() and x.dtype == F16
    if x2 is not None:
        assert x2.is_contiguous() and x2.dtype == F16 and x2.shape[:-1] == x.shape[:-1]
    if up_fold:
        assert ksize == 3 and stride == 1 and not up and not padded and x2 is None and x.dim() == 4
        assert gn is None and ln is None and not silu_in and act is None and temb is None and resid is None
        assert not gn_moments and not ln_fold
    if pad_after:
        assert ksize == 3 and stride == 2 and not up and not up_fold and not padded and x.dim() == 4
        assert h % 2 == 0 and w % 2 == 0, "pad-after downsample: even H and W"
    oh, ow = torch_ops.conv_out_hw(h, w, ksize, stride, up, up_fold, pad_after)
    out_cols = cout // 2 if act == "geglu" else cout
    if out is None:
        shape = (x.shape[0], out_cols) if x.dim() == 2 else (x.shape[0], oh, ow, out_cols)
        out = torch.empty(shape, device=x.device, dtype=F16)
    assert out.stride(-1) == 1
    if resid is not None:
        assert resid.stride(-1) == 1
    gs, gh = gn if gn is not None else (None, None)
    ls, lg, lb = ln if ln is not None else (None, None, None)
    mom, rows = None, 0
    if gn_moments and x.dim() == 4 and act is None and not up and not pad_after and out.is_contiguous():
        rows = gn_moment_rows(out.shape[0], oh, ow, x.shape[-1], cout, ksize, stride, bool(padded), resid is not None,
                              temb is not None, gn_moments, x2.shape[-1] if x2 is not None else 0)
        if rows:
            mom = torch.empty((out.shape[0], oh * ow // rows, gn_moments, 2), device=x.device, dtype=torch.float32)
    C2D.conv2d_igemm(x, weight, kpad, cout, ksize, stride, up, x2, gs, gh, gn_silu, ls, lg, lb, silu_in, bias,
                     C2D_ACT[act], temb, resid, out, bool(padded), float(ln_fold or 0.0), mom, int(gn_moments),
                     bool(up_fold), bool(pad_after))
    if gn_moments:
        return out, (GnMoments(out, mom, rows, gn_moments) if mom is not None else None)
    return out


class GnMoments:
    """GroupNorm moments a conv emitted for its output (c2d_conv_desc::gn_mom): mom fp32
    [N][H*W / rows][groups][2] of {mean, M2}; valid for `of` (that exact tensor) until it is written again."""

    def __init__(self, of: torch.Tensor, mom: torch.Tensor, rows: int, groups: int):
        self.of, self.mom, self.rows, self.groups = of, mom, rows, groups

    def matches(self, x: torch.Tensor, groups: int) -> bool:
        return (x is self.of and groups == self.groups and x.dim() == 4 and
                tuple(self.mom.shape[:1]) == tuple(x.shape[:1]))


@functools.lru_cache(maxsize=None)
def gn_moment_rows(n: int, oh: int, ow: int, cin: int, cout: int, ksize: int, stride: int, padded: bool, resid: bool,
                   temb: bool, groups: int, c1: int = 0) -> int:
    """c2d_conv2d_gn_rows for a conv of these shapes as ops.conv issues it (16-B aligned operands, a workspace
    for any split): rows per moment block, 0 = this conv cannot emit its output's GroupNorm moments."""
    h, w = (oh, ow) if padded or ksize == 1 or stride == 1 else (oh * stride, ow * stride)
    d = _shape_desc(n, h, w, cin, cout, ksize, c1=c1, oh=oh, ow=ow, stride=stride, src_pad=padded, resid=resid,
                    temb=temb, groups=groups, operands=True)
    return int(lib().c2d_conv2d_gn_rows(ctypes.byref(d)))


@torch.no_grad()
def fold_layernorm(weight: torch.Tensor, bias: torch.Tensor | None, gamma: torch.Tensor, beta: torch.Tensor,
                   in_features: int):
    """LayerNorm(gamma, beta) -> Linear(packed fp16 weight [cout][kpad], bias) as one GEMM over the
    normalised rows (C2D_PRO_LNFOLD): (W diag(gamma) fp16, b + W beta fp32)."""
    w = weight[:, :in_features].float()
    wp = torch.zeros_like(weight)
    wp[:, :in_features] = (w * gamma.float().view(1, -1)).to(F16)
    b = w @ beta.float()
    if bias is not None:
        b = b + bias.float()
    return wp.contiguous(), b.contiguous()


@functools.lru_cache(maxsize=None)
def panel_gemm(m: int, k: int, cout: int, geglu: bool, lnfold: bool = False) -> bool:
    """Does c2d's planner run this 1x1 GEMM (m x k -> cout) on the panel GEMM (tile 70)?  Where it
    does, a LayerNorm before it folds in.  lnfold: would the library take this GEMM with a folded
    LayerNorm (C2D_PRO_LNFOLD: the panel GEMM's shapes and switches, else C2D_E_SHAPE)?"""
    rc, tile, _ = _plan_query(_shape_desc(1, 1, m, k, cout, 1, act="geglu" if geglu else None,
                                          out_ld=cout // 2 if geglu else cout, lnfold=lnfold))
    return rc == 0 and tile == 70


ROWRING_TILES = (42, 43, 44)   # igemm_pp16r.h: output width 64 / 32 / 16


@functools.lru_cache(maxsize=None)
def rowring_conv(n: int, h: int, w: int, cin: int, cout: int) -> bool:
    """Does c2d's planner run a 3x3 stride-1 conv (n x h x w, cin -> cout) on a row-ring tile (42 / 43
    / 44, by output width) when its source is zero-bordered?  (Asked of the library, c2d_conv2d_igemm_plan: the padded
    layout is worth writing only where that kernel reads it.)"""
    rc, tile, _ = _plan_query(_shape_desc(n, h, w, cin, cout, 3, src_pad=True))
    check(rc, "c2d_conv2d_igemm_plan")
    return tile in ROWRING_TILES


def conv_workspace_bytes(n: int, h: int, w: int, c0: int, c1: int, cout: int, ksize: int) -> int:
    """Split-K workspace c2d_conv2d_igemm asks for on a stride-1 conv (n x h x w, c0 [+ c1] -> cout),
    as torch_ops.conv2d_igemm allocates it (c2d_conv2d_igemm_workspace_size)."""
    return int(lib().c2d_conv2d_igemm_workspace_size(ctypes.byref(_shape_desc(n, h, w, c0, cout, ksize, c1=c1))))


class record_conv_plans:
    """Context manager collecting the (tile_id, ksplit) plan of every conv call
    (c2d_conv2d_igemm_plan) -- lets tests assert which kernel configuration ran -- and, in ws_bytes, the
    split-K workspace each call allocated."""

    def __enter__(self):
        self.plans, self.ws_bytes = [], []
        torch_ops._plan_probe, torch_ops._ws_probe = self.plans, self.ws_bytes
        return self.plans

    def __exit__(self, *exc):
        torch_ops._plan_probe = torch_ops._ws_probe = None
        return False


class force_plan:
    """Context manager forcing the implicit-GEMM plan (tile id, K split; 0 = planner) through
    c2d_set_plan_override -- tests and tuning sweeps only, never the product path."""

    def __init__(self, tile: int, split: int = 0):
        self.tile, self.split = int(tile), int(split)

    def __enter__(self):
        t, sp = ctypes.c_int(0), ctypes.c_int(0)
        check(lib().c2d_get_plan_override(ctypes.byref(t), ctypes.byref(sp)), "c2d_get_plan_override")
        self.prev = (t.value, sp.value)   # restored on exit: nested overrides / env sweeps survive
        check(lib().c2d_set_plan_override(self.tile, self.split), "c2d_set_plan_override")
        rowring_conv.cache_clear()        # the planner's answers change under an override
        gn_moment_rows.cache_clear()
        return self

    def __exit__(self, *exc):
        lib().c2d_set_plan_override(*self.prev)
        rowring_conv.cache_clear()
        gn_moment_rows.cache_clear()
        return False


def plan_override_from_env() -> None:
    """Opt-in for the tuning scripts: C2D_GEMM_TILE / C2D_GEMM_SPLIT (environment) ->
    c2d_set_plan_override.  The library itself never reads them."""
    t, sp = int(os.environ.get("C2D_GEMM_TILE", "0") or 0), int(os.environ.get("C2D_GEMM_SPLIT", "0") or 0)
    if t or sp:
        check(lib().c2d_set_plan_override(t, sp), "c2d_set_plan_override")


def group_norm_stats(x: torch.Tensor, groups: int, eps: float, gamma: torch.Tensor, beta: torch.Tensor,
                     x2: torch.Tensor | None = None):
    """-> (scale, shift) fp32 [N, C] folding GroupNorm(groups, eps) + affine."""
    _require(x, "x")
    c = x.shape[-1] + (x2.shape[-1] if x2 is not None else 0)
    scale = torch.empty((x.shape[0], c), device=x.device, dtype=torch.float32)
    shift = torch.empty_like(scale)
    C2D.groupnorm_stats(x, x2, groups, float(eps), gamma, beta, scale, shift)
    return scale, shift


def group_norm_apply(x: torch.Tensor, gn, silu: bool, x2: torch.Tensor | None = None,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """Materialise act(GroupNorm(cat[x, x2])) from the folded (scale, shift) tables."""
    _require(x, "x")
    c = x.shape[-1] + (x2.shape[-1] if x2 is not None else 0)
    if out is None:
        out = torch.empty((*x.shape[:-1], c), device=x.device, dtype=F16)
    C2D.groupnorm_apply(x, x2, gn[0], gn[1], bool(silu), out)
    return out


def group_norm(x: torch.Tensor, groups: int, eps: float, gamma: torch.Tensor, beta: torch.Tensor, silu: bool,
               x2: torch.Tensor | None = None, out: torch.Tensor | None = None, pad: bool = False,
               mom: "GnMoments | None" = None) -> torch.Tensor:
    """act(GroupNorm(cat[x, x2])) in one c2d::groupnorm call (single fused kernel for
    small images, stats + apply otherwise).  pad: write the zero-bordered layout
    [N, H + 2, W + 2, C] (c2d::groupnorm_pad) for a conv(..., padded=True).  mom: the moments x's
    producing conv emitted (conv(..., gn_moments=groups)): one launch, no statistics pass."""
    _require(x, "x")
    c = x.shape[-1] + (x2.shape[-1] if x2 is not None else 0)
    if mom is not None and x2 is None and mom.matches(x, groups):
        n, h, w, _ = x.shape
        if out is None:
            out = torch.empty((n, h + 2, w + 2, c) if pad else x.shape, device=x.device, dtype=F16)
        C2D.groupnorm_moments(x, groups, float(eps), gamma, beta, bool(silu), mom.mom, mom.rows, bool(pad), out)
        return out
    if pad:
        n, h, w, _ = x.shape
        if out is None:
            out = torch.empty((n, h + 2, w + 2, c), device=x.device, dtype=F16)
        C2D.groupnorm_pad(x, x2, groups, float(eps), gamma, beta, bool(silu), out)
        return out
    if out is None:
        out = torch.empty((*x.shape[:-1], c), device=x.device, dtype=F16)
    C2D.groupnorm(x, x2, groups, float(eps), gamma, beta, bool(silu), out)
    return out


def layer_norm_stats(x2d: torch.Tensor, eps: float) -> torch.Tensor:
    _require(x2d, "x")
    st = torch.empty((x2d.shape[0], 2), device=x2d.device, dtype=torch.float32)
    C2D.layernorm_stats(x2d, float(eps), st)
    return st


def layer_norm(x2d: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
               out: torch.Tensor | None = None) -> torch.Tensor:
    _require(x2d, "x")
    if out is None:
        out = torch.empty(x2d.shape, device=x2d.device, dtype=F16)
    C2D.layernorm(x2d, gamma, beta, float(eps), out)
    return out


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, batch: int, heads: int, lq: int, lk: int,
              d: int, scale: float | None = None, out: torch.Tensor | None = None,
              key_bias: torch.Tensor | None = None) -> torch.Tensor:
    """q/k/v: 2-D row views [batch*L, >= heads*d] (column slices allowed).
    key_bias: optional additive score bias, fp32, either per key [batch|1, heads|1, lk]
    (c2d_attention_fwd_bias) or per (query, key) [batch|1, heads|1, lq|1, lk]
    (c2d_attention_fwd_mask); size-1 dims broadcast."""
    _require(q, "q")
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    if out is None:
        out = torch.empty((batch * lq, heads * d), device=q.device, dtype=F16)
    ldb = ldh = ldq = 0
    kb = None
    if key_bias is not None:
        kb = key_bias.to(device=q.device, dtype=torch.float32)
        if kb.dim() == 3:
            kb = kb.unsqueeze(2)
        if (kb.dim() != 4 or kb.shape[-1] != lk or kb.shape[0] not in (1, batch) or kb.shape[1] not in (1, heads)
                or kb.shape[2] not in (1, lq)):
            raise ValueError(f"key_bias must be [batch|1, heads|1, ({lq}|1,) {lk}], got {tuple(key_bias.shape)}")
        kb = kb.contiguous()
        ldb = kb.stride(0) if kb.shape[0] > 1 else 0
        ldh = kb.stride(1) if kb.shape[1] > 1 else 0
        ldq = kb.stride(2) if kb.shape[2] > 1 else 0
    C2D.attention_fwd(q, k, v, batch, heads, lq, lk, d, float(scale), kb, ldb, ldh, out, ldq)
    return out


def attention_small(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, batch: int, heads: int, l: int, d: int,
                    causal: bool, scale: float | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Short-sequence (l <= 128, d = 64) attention, optionally causal (c2d::attention_small)."""
    _require(q, "q")
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    if out is None:
        out = torch.empty((batch * l, heads * d), device=q.device, dtype=F16)
    C2D.attention_small(q, k, v, batch, heads, l, d, float(scale), bool(causal), out)
    return out


def window_attention(qkv: torch.Tensor, row_map: torch.Tensor, n_windows: int, heads: int, d: int,
                     bias: torch.Tensor, mask: torch.Tensor | None, out: torch.Tensor) -> torch.Tensor:
    C2D.window_attention(qkv, row_map, n_windows, heads, d, bias, mask, out)
    return out


def htsat_mel_patches(mel: torch.Tensor, bn_scale: torch.Tensor, bn_shift: torch.Tensor) -> torch.Tensor:
    b, t, f = mel.shape
    assert f == 64 and mel.dtype == torch.float32 and mel.is_contiguous()
    out = torch.empty((b * 4096, 64), device=mel.device, dtype=F16)
    C2D.htsat_mel_patches(mel, bn_scale, bn_shift, out)
    return out


def patch_merge_gather(x: torch.Tensor, b: int, h: int, w: int, c: int) -> torch.Tensor:
    out = torch.empty((b * (h // 2) * (w // 2), 4 * c), device=x.device, dtype=F16)
    C2D.patch_merge_gather(x, b, h, w, c, out)
    return out


def row_mean(x: torch.Tensor, b: int, rows: int) -> torch.Tensor:
    out = torch.empty((b, x.shape[1]), device=x.device, dtype=torch.float32)
    C2D.row_mean(x, b, rows, out)
    return out


def softmax_rows(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Row softmax of a 2-D fp16 matrix (c2d::softmax_rows); out may alias x."""
    _require(x, "x")
    assert x.dim() == 2 and x.dtype == F16 and x.stride(1) == 1
    out = torch.empty_like(x) if out is None else out
    assert out.shape == x.shape and out.stride(1) == 1
    C2D.softmax_rows(x, out)
    return out


def l2_normalize_(x: torch.Tensor) -> torch.Tensor:
    C2D.l2_normalize(x)
    return x


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)   # OpenAI CLIP's image_mean / image_std (CLIPImageProcessor)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_preprocess(images_u8: torch.Tensor, size: int = 224, patch: int = 14, mean=CLIP_MEAN, std=CLIP_STD,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 [B, H, W, 3] (any H, W) -> fp16 [B * (size / patch)^2, kpad_of(3 * patch^2)]: CLIPImageProcessor in one
    launch (c2d::clip_preprocess): PIL-bicubic resize of the shorter side to `size`, centre crop, (v / 255 - mean) /
    std, and the patch cut with K ordered (dy, dx, channel) as pack_conv_weight orders a patch x patch conv."""
    _require(images_u8, "images_u8")
    assert images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[-1] == 3
    assert images_u8.is_contiguous()
    if size <= 0 or patch <= 0 or size % patch:
        raise ValueError(f"size {size} is no positive multiple of patch {patch}")
    rows, kp = images_u8.shape[0] * (size // patch) ** 2, kpad_of(3 * patch * patch)
    if out is None:
        out = torch.empty((rows, kp), device=images_u8.device, dtype=F16)
    assert out.dtype == F16 and out.is_contiguous() and tuple(out.shape) == (rows, kp)
    C2D.clip_preprocess(images_u8, int(size), int(patch), [float(v) for v in mean], [float(v) for v in std], out)
    return out


def cosine_rows(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [M, C] row pairs -> fp32 [M]: a_i . b_i / max(|a_i| |b_i|, 1e-12) (c2d::cosine_rows)."""
    _require(a, "a")
    assert a.dim() == 2 and a.shape == b.shape and b.is_cuda
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous()
    if out is None:
        out = torch.empty((a.shape[0],), device=a.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (a.shape[0],)
    C2D.cosine_rows(a, b, out)
    return out


def timestep_embedding(t_table: torch.Tensor, step_index: torch.Tensor | None, n: int, dim: int) -> torch.Tensor:
    out = torch.empty((n, dim), device=t_table.device, dtype=F16)
    C2D.timestep_embedding(t_table, step_index, n, dim, out)
    return out


def cfg_ddim_step(eps: torch.Tensor, x: torch.Tensor, guidance: float, coef: torch.Tensor, step_index: torch.Tensor,
                  advance: bool = True) -> torch.Tensor:
    C2D.cfg_ddim_step(eps, x, float(guidance), coef, step_index, bool(advance))
    return x


def latent_to_nhwc(x: torch.Tensor, cpad: int, dup: bool) -> torch.Tensor:
    b, c, hgt, wid = x.shape
    out = torch.empty(((2 if dup else 1) * b, hgt, wid, cpad), device=x.device, dtype=F16)
    C2D.latent_to_nhwc(x, cpad, bool(dup), out)
    return out


def image_to_nhwc(img: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 NHWC [N, H, W, 3] -> fp16 NHWC [N, H, W, 8] in [-1, 1], channels 3..7 zero (c2d::image_to_nhwc)."""
    _require(img, "img")
    assert img.dtype == torch.uint8 and img.dim() == 4 and img.shape[-1] == 3 and img.is_contiguous()
    if out is None:
        out = torch.empty((*img.shape[:-1], 8), device=img.device, dtype=F16)
    C2D.image_to_nhwc(img, out)
    return out


def vae_posterior_noise(moments: torch.Tensor, out: torch.Tensor, scaling: float, eps: torch.Tensor | None = None,
                        noise: torch.Tensor | None = None, coef: torch.Tensor | None = None,
                        step_index: torch.Tensor | None = None) -> torch.Tensor:
    """moments fp16 [N * h * w, >= 8] (mean | log-variance) -> out fp32 [N, 4, h, w] (c2d::vae_posterior_noise):
    z = (mean + std * eps) * scaling (eps None: the mode); with noise, DDIMScheduler.add_noise at the alpha
    coef[2 * step_index] read on the device."""
    _require(moments, "moments")
    assert moments.dim() == 2 and moments.dtype == F16 and moments.stride(1) == 1 and moments.shape[1] >= 8
    assert out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 4 and out.shape[1] == 4
    assert moments.shape[0] == out.shape[0] * out.shape[2] * out.shape[3]
    for t in (eps, noise):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.shape == out.shape and t.is_cuda)
    if noise is not None:
        assert coef is not None and step_index is not None and coef.dtype == torch.float32
        assert step_index.dtype == torch.int32
    C2D.vae_posterior_noise(moments, eps, noise, coef, step_index, float(scaling), out)
    return out


def cfg_ddim_step_masked(eps: torch.Tensor, x: torch.Tensor, z0: torch.Tensor, noise: torch.Tensor, mask: torch.Tensor,
                         guidance: float, coef: torch.Tensor, step_index: torch.Tensor,
                         advance: bool = True) -> torch.Tensor:
    """The inpainting step's update of x fp32 [B, 4, h, w] in place (c2d::cfg_ddim_step_masked): cfg_ddim_step's
    result where mask fp32 [B, h, w] is 1, the original z0 re-noised with `noise` to the next step's timestep
    (z0 itself at the last step) where it is 0, the blend in between."""
    _require(x, "x")
    assert eps.dtype == F16 and eps.is_contiguous() and eps.numel() == 2 * x.numel()
    assert x.dim() == 4 and x.shape[1] == 4
    for t in (x, z0, noise):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == x.shape and t.is_cuda
    assert mask.dtype == torch.float32 and mask.is_contiguous() and mask.is_cuda
    assert tuple(mask.shape) == (x.shape[0], x.shape[2], x.shape[3])
    assert coef.dtype == torch.float32 and coef.is_contiguous() and coef.dim() == 2 and coef.shape[1] == 2
    assert step_index.dtype == torch.int32
    C2D.cfg_ddim_step_masked(eps, x, z0, noise, mask, float(guidance), coef, step_index, bool(advance))
    return x


def _check_dpm_step(eps, x, x0_prev, mcoef, step_index, first_step) -> None:
    _require(x, "x")
    assert eps.dtype == F16 and eps.is_contiguous() and eps.numel() == 2 * x.numel()
    assert x.dim() == 4 and x.shape[1] == 4
    for t in (x, x0_prev):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == x.shape and t.is_cuda
    assert x0_prev is not x
    assert mcoef.dtype == torch.float32 and mcoef.is_contiguous() and mcoef.dim() == 2 and mcoef.shape[1] == 8
    for t in (step_index, first_step):
        assert t.dtype == torch.int32 and t.numel() == 1


def cfg_dpm_step(eps: torch.Tensor, x: torch.Tensor, x0_prev: torch.Tensor, guidance: float, mcoef: torch.Tensor,
                 step_index: torch.Tensor, first_step: torch.Tensor, advance: bool = True) -> torch.Tensor:
    """The DPM-Solver++(2M) step's update of x fp32 [B, 4, h, w] in place (c2d::cfg_dpm_step): classifier-free
    guidance over eps fp16 NHWC [2B, h, w, 4], then the multistep update from mcoef fp32 [steps, 8]
    (DPMSolverMultistepScheduler.device_tables) at the device counter step_index.  x0_prev (fp32, x's shape) is
    the previous step's data prediction, overwritten with this step's; the step equal to the device int32
    first_step is first-order and does not read it."""
    _check_dpm_step(eps, x, x0_prev, mcoef, step_index, first_step)
    C2D.cfg_dpm_step(eps, x, x0_prev, float(guidance), mcoef, step_index, first_step, bool(advance))
    return x


def cfg_dpm_step_masked(eps: torch.Tensor, x: torch.Tensor, x0_prev: torch.Tensor, z0: torch.Tensor,
                        noise: torch.Tensor, mask: torch.Tensor, guidance: float, mcoef: torch.Tensor,
                        step_index: torch.Tensor, first_step: torch.Tensor, advance: bool = True) -> torch.Tensor:
    """cfg_dpm_step for inpainting (c2d::cfg_dpm_step_masked): its result where mask fp32 [B, h, w] is 1, the
    original z0 re-noised with `noise` to the next step's timestep (z0 itself at the last step) where it is 0, the
    blend in between."""
    _check_dpm_step(eps, x, x0_prev, mcoef, step_index, first_step)
    for t in (z0, noise):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == x.shape and t.is_cuda
    assert mask.dtype == torch.float32 and mask.is_contiguous() and mask.is_cuda
    assert tuple(mask.shape) == (x.shape[0], x.shape[2], x.shape[3])
    C2D.cfg_dpm_step_masked(eps, x, x0_prev, z0, noise, mask, float(guidance), mcoef, step_index, first_step,
                            bool(advance))
    return x


def mask_to_latent(mask_u8: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 [N, H, W] (H, W multiples of 8; >= 128 = repaint) -> fp32 [N, H/8, W/8] of 0 / 1: the sample at
    (8y, 8x), i.e. the binarised mask under F.interpolate nearest (c2d::mask_to_latent)."""
    _require(mask_u8, "mask_u8")
    assert mask_u8.dtype == torch.uint8 and mask_u8.dim() == 3 and mask_u8.is_contiguous()
    n, hgt, wid = mask_u8.shape
    assert hgt % 8 == 0 and wid % 8 == 0 and hgt > 0 and wid > 0, f"mask size {hgt}x{wid} is no multiple of 8"
    if out is None:
        out = torch.empty((n, hgt // 8, wid // 8), device=mask_u8.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n, hgt // 8, wid // 8)
    C2D.mask_to_latent(mask_u8, out)
    return out


def composite_u8(decoded: torch.Tensor, original: torch.Tensor, mask_u8: torch.Tensor,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 images [N, H, W, 3] and mask [N, H, W] -> mask >= 128 ? decoded : original (c2d::composite_u8); out may
    be decoded."""
    _require(decoded, "decoded")
    for t in (decoded, original):
        assert t.dtype == torch.uint8 and t.is_contiguous() and t.is_cuda and t.shape == decoded.shape
    assert decoded.dim() == 4 and decoded.shape[-1] == 3
    assert mask_u8.dtype == torch.uint8 and mask_u8.is_contiguous() and mask_u8.is_cuda
    assert mask_u8.shape == decoded.shape[:-1]
    if out is None:
        out = torch.empty_like(decoded)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == decoded.shape
    C2D.composite_u8(decoded, original, mask_u8, out)
    return out


def inpaint_prepare(moments: torch.Tensor, noise: torch.Tensor, mask_u8: torch.Tensor, scaling: float,
                    eps: torch.Tensor | None = None, coef: torch.Tensor | None = None,
                    step_index: torch.Tensor | None = None, pure_noise: bool = False, z0: torch.Tensor | None = None,
                    x: torch.Tensor | None = None, mask: torch.Tensor | None = None):
    """The entry into the inpainting loop in one launch (c2d::inpaint_prepare) -> (z0, x, mask): moments fp16
    [N * h * w, >= 8] and noise fp32 [N, 4, h, w] as vae_posterior_noise takes them, mask_u8 uint8 [N, 8h, 8w].
    z0 = (mean + std * eps) * scaling (eps None: the mode); x = noise when pure_noise (the loop starts at step 0),
    else add_noise(z0, noise) at the alpha coef[2 * step_index] read on the device; mask fp32 [N, h, w] as
    mask_to_latent gives it.  x must not be noise or z0."""
    _require(moments, "moments")
    assert moments.dim() == 2 and moments.dtype == F16 and moments.stride(1) == 1 and moments.shape[1] >= 8
    assert noise.dtype == torch.float32 and noise.is_contiguous() and noise.dim() == 4 and noise.shape[1] == 4
    n, _, hgt, wid = noise.shape
    assert moments.shape[0] == n * hgt * wid
    assert mask_u8.dtype == torch.uint8 and mask_u8.is_contiguous() and mask_u8.is_cuda
    assert tuple(mask_u8.shape) == (n, 8 * hgt, 8 * wid), f"mask {tuple(mask_u8.shape)} for latents {tuple(noise.shape)}"
    if z0 is None:
        z0 = torch.empty_like(noise)
    if x is None:
        x = torch.empty_like(noise)
    if mask is None:
        mask = torch.empty((n, hgt, wid), device=noise.device, dtype=torch.float32)
    for t in (eps, noise, z0, x):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.shape == noise.shape and t.is_cuda)
    assert x is not noise and x is not z0
    assert mask.dtype == torch.float32 and mask.is_contiguous() and tuple(mask.shape) == (n, hgt, wid)
    if not pure_noise:
        assert coef is not None and step_index is not None and coef.dtype == torch.float32
        assert step_index.dtype == torch.int32
    C2D.inpaint_prepare(moments, eps, noise, mask_u8, coef, step_index, bool(pure_noise), float(scaling), z0, x, mask)
    return z0, x, mask


def upsample_nearest2x(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """NHWC fp16 nearest x2 (diffusers Upsample2D interpolate step)."""
    n, h, w, c = x.shape
    x = x.contiguous()
    if out is None:
        out = torch.empty(n, 2 * h, 2 * w, c, device=x.device, dtype=x.dtype)
    C2D.upsample_nearest2x(x, out)
    return out


def add(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    if out is None:
        out = torch.empty_like(a)
    C2D.add(a, b, out)
    return out
