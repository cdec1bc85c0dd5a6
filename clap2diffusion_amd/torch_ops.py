"""torch.library custom ops over the C ABI ("callers via torch.library
custom-op wrappers that pass torch.cuda.current_stream()").

Every entry point of include/c2d.h that the sampling path calls is registered as a
``c2d::<name>`` operator with a CUDA (HIP) implementation only -- a CPU tensor reaching one
fails in the dispatcher, there is no fallback -- and a fake (meta) implementation, so the
ops are visible to torch (FakeTensor tracing, torch.compile graphs, schema checks) rather
than opaque ctypes calls.  All ops are out-variants: the caller (clap2diffusion_amd.ops)
allocates the outputs, the op mutates them (``mutates_args``) and returns nothing, which
keeps the fake implementations trivial and lets a GEMM write its result into the
residual it adds (in-place residual epilogues).  Each launch goes to
torch.cuda.current_stream(), so the ops are hipGraph-capturable as they stand.
"""
import ctypes
from typing import Optional

import torch
from torch import Tensor
from torch.library import custom_op

from ._lib import C2D_PAD_AFTER, C2D_PAD_SAME, C2D_PRO_GN, C2D_PRO_LN, C2D_PRO_LNFOLD, C2D_PRO_NONE, C2D_PRO_SILU, ConvDesc, check, lib, ptr, stream_ptr

_CU = "cuda"


def conv_out_hw(h: int, w: int, ksize: int, stride: int, up: bool, up_fold: bool, pad_after: bool) -> tuple[int, int]:
    """Output size of c2d::conv2d_igemm over an h x w image: a 3x3 pads 1 on the (nearest-x2, up or up_fold) view;
    pad_after is F.pad(x, (0, 1, 0, 1)) + conv(stride 2, padding 0), (h + 1 - 3) // 2 + 1; a 1x1 keeps the size."""
    if ksize != 3:
        return h, w
    if pad_after:
        return (h - 2) // 2 + 1, (w - 2) // 2 + 1
    vh, vw = (2 * h, 2 * w) if up or up_fold else (h, w)
    return (vh + 2 - 3) // stride + 1, (vw + 2 - 3) // stride + 1


def _conv_desc(x, weight, kpad, cout, ksize, stride, up, x2, gn_scale, gn_shift, gn_silu, ln_stats, ln_gamma,
               ln_beta, silu_in, bias, act, temb, resid, out, src_pad=False, lnf_eps=0.0, gn_mom=None,
               gn_groups=0, up_fold=False, pad_after=False) -> ConvDesc:
    if x.dim() == 2:
        n, h, w = 1, 1, x.shape[0]
        c0 = x.shape[1]
    else:
        n, h, w, c0 = x.shape
        if src_pad:   # zero-bordered [n][h + 2][w + 2][c0]: logical size h x w
            h, w = h - 2, w - 2
    c1 = x2.shape[-1] if x2 is not None else 0
    oh, ow = conv_out_hw(h, w, ksize, stride, up, up_fold, pad_after)
    d = ConvDesc()
    d.src0 = ptr(x); d.src1 = ptr(x2); d.c0 = c0; d.c1 = c1
    d.n, d.h, d.w, d.oh, d.ow = n, h, w, oh, ow
    d.ksize, d.stride, d.up = ksize, stride, (2 if up_fold else int(up))   # 2: the folded upsample
    d.weight = ptr(weight); d.cout = cout; d.kpad = kpad
    if lnf_eps > 0.0:   # LayerNorm folded into the panel GEMM (weight = W diag(gamma), bias = b + W beta)
        d.pro = C2D_PRO_LNFOLD; d.pro_eps = lnf_eps
    elif gn_scale is not None:
        d.pro = C2D_PRO_GN; d.pro_silu = int(gn_silu); d.pro_a = ptr(gn_scale); d.pro_b = ptr(gn_shift)
    elif ln_stats is not None:
        d.pro = C2D_PRO_LN; d.pro_a = ptr(ln_stats); d.gamma = ptr(ln_gamma); d.beta = ptr(ln_beta)
    elif silu_in:
        d.pro = C2D_PRO_SILU
    else:
        d.pro = C2D_PRO_NONE
    d.bias = ptr(bias)
    d.act = act
    if temb is not None:
        d.temb = ptr(temb); d.temb_ld = temb.stride(0)
    if resid is not None:
        d.resid = ptr(resid); d.resid_ld = resid.stride(-2) if resid.dim() == 2 else resid.shape[-1]
    d.out = ptr(out)
    d.out_ld = out.stride(-2) if out.dim() == 2 else out.shape[-1]
    d.src_pad = int(src_pad)
    if gn_mom is not None:
        d.gn_mom = ptr(gn_mom); d.gn_groups = gn_groups
    d.pad_mode = C2D_PAD_AFTER if pad_after else C2D_PAD_SAME
    return d


_plan_probe: Optional[list] = None   # ops.record_conv_plans: the (tile, K slices) c2d_conv2d_igemm_plan reports per call
_ws_probe: Optional[list] = None     # ... and the bytes of split-K workspace the call allocated


@custom_op("c2d::conv2d_igemm", mutates_args=("out",), device_types=_CU)
def conv2d_igemm(x: Tensor, weight: Tensor, kpad: int, cout: int, ksize: int, stride: int, up: bool,
                 x2: Optional[Tensor], gn_scale: Optional[Tensor], gn_shift: Optional[Tensor], gn_silu: bool,
                 ln_stats: Optional[Tensor], ln_gamma: Optional[Tensor], ln_beta: Optional[Tensor], silu_in: bool,
                 bias: Optional[Tensor], act: int, temb: Optional[Tensor], resid: Optional[Tensor],
                 out: Tensor, src_pad: bool = False, lnf_eps: float = 0.0, gn_mom: Optional[Tensor] = None,
                 gn_groups: int = 0, up_fold: bool = False, pad_after: bool = False) -> None:
    """c2d_conv2d_igemm (+ its split-K workspace, sized by c2d_conv2d_igemm_workspace_size).
    src_pad: x is the zero-bordered layout [n][h + 2][w + 2][c] (c2d_groupnorm_pad).
    lnf_eps > 0: a LayerNorm (that eps) folded into the GEMM (C2D_PRO_LNFOLD).
    gn_mom: fp32 [n][hw / rows][gn_groups][2], the output's GroupNorm moments written by the conv
    (c2d_conv_desc::gn_mom; rows = c2d_conv2d_gn_rows).
    up_fold: the folded upsample (c2d_conv_desc::up = 2): x low-res, weight the [4][cout][4 cin] phase pack, out
    [n][2h][2w][cout]; `up` stays the nearest-x2 view of the register-staged 3x3.
    pad_after: c2d_conv_desc::pad_mode = C2D_PAD_AFTER, the 3x3 stride-2 conv of F.pad(x, (0, 1, 0, 1)) with
    padding 0 (even h, w; out [n][h / 2][w / 2][cout])."""
    d = _conv_desc(x, weight, kpad, cout, ksize, stride, up, x2, gn_scale, gn_shift, gn_silu, ln_stats, ln_gamma,
                   ln_beta, silu_in, bias, act, temb, resid, out, src_pad, lnf_eps, gn_mom, gn_groups, up_fold,
                   pad_after)
    wsb = lib().c2d_conv2d_igemm_workspace_size(ctypes.byref(d))
    if wsb:
        ws = torch.empty(wsb // 4, device=x.device, dtype=torch.float32)
        d.ws = ptr(ws); d.ws_bytes = wsb
    if _ws_probe is not None:
        _ws_probe.append(ws.numel() * ws.element_size() if wsb else 0)
    if _plan_probe is not None:
        tid, ks = ctypes.c_int(), ctypes.c_int()
        check(lib().c2d_conv2d_igemm_plan(ctypes.byref(d), ctypes.byref(tid), ctypes.byref(ks)), "c2d_conv2d_igemm_plan")
        _plan_probe.append((tid.value, ks.value))
    check(lib().c2d_conv2d_igemm(ctypes.byref(d), stream_ptr()), "c2d_conv2d_igemm")


@conv2d_igemm.register_fake
def _(x, weight, kpad, cout, ksize, stride, up, x2, gn_scale, gn_shift, gn_silu, ln_stats, ln_gamma, ln_beta,
      silu_in, bias, act, temb, resid, out, src_pad=False, lnf_eps=0.0, gn_mom=None, gn_groups=0, up_fold=False,
      pad_after=False):
    return None


@custom_op("c2d::pack_weights", mutates_args=("out",), device_types=_CU)
def pack_weights(w: Tensor, cout: int, cin: int, ksize: int, cin_pad: int, kpad: int, out: Tensor) -> None:
    check(lib().c2d_pack_weights(ptr(w), cout, cin, ksize, cin_pad, kpad, ptr(out), stream_ptr()), "c2d_pack_weights")


@custom_op("c2d::groupnorm_stats", mutates_args=("scale", "shift"), device_types=_CU)
def groupnorm_stats(x: Tensor, x2: Optional[Tensor], groups: int, eps: float, gamma: Tensor, beta: Tensor,
                    scale: Tensor, shift: Tensor) -> None:
    n, c0 = x.shape[0], x.shape[-1]
    c1 = x2.shape[-1] if x2 is not None else 0
    hw = x.numel() // (n * c0)
    ws = torch.empty(lib().c2d_groupnorm_workspace_size(n, c0 + c1, hw) // 4, device=x.device, dtype=torch.float32)
    check(lib().c2d_groupnorm_stats(ptr(x), ptr(x2), c0, c1, n, hw, groups, eps, ptr(gamma), ptr(beta), ptr(scale),
                                    ptr(shift), ptr(ws), stream_ptr()), "c2d_groupnorm_stats")


@custom_op("c2d::groupnorm_apply", mutates_args=("out",), device_types=_CU)
def groupnorm_apply(x: Tensor, x2: Optional[Tensor], scale: Tensor, shift: Tensor, silu: bool, out: Tensor) -> None:
    n, c0 = x.shape[0], x.shape[-1]
    c1 = x2.shape[-1] if x2 is not None else 0
    hw = x.numel() // (n * c0)
    check(lib().c2d_groupnorm_apply(ptr(x), ptr(x2), c0, c1, n, hw, ptr(scale), ptr(shift), int(silu), ptr(out),
                                    stream_ptr()), "c2d_groupnorm_apply")


@custom_op("c2d::groupnorm", mutates_args=("out",), device_types=_CU)
def groupnorm(x: Tensor, x2: Optional[Tensor], groups: int, eps: float, gamma: Tensor, beta: Tensor, silu: bool,
              out: Tensor) -> None:
    n, c0 = x.shape[0], x.shape[-1]
    c1 = x2.shape[-1] if x2 is not None else 0
    hw = x.numel() // (n * c0)
    wsb = lib().c2d_groupnorm_run_workspace_size(n, c0 + c1, hw, groups)
    ws = torch.empty((wsb + 15) // 16 * 4, device=x.device, dtype=torch.float32) if wsb else None
    check(lib().c2d_groupnorm(ptr(x), ptr(x2), c0, c1, n, hw, groups, eps, ptr(gamma), ptr(beta), int(silu), ptr(out),
                              ptr(ws), wsb, stream_ptr()), "c2d_groupnorm")


@custom_op("c2d::groupnorm_pad", mutates_args=("out",), device_types=_CU)
def groupnorm_pad(x: Tensor, x2: Optional[Tensor], groups: int, eps: float, gamma: Tensor, beta: Tensor, silu: bool,
                  out: Tensor) -> None:
    """c2d_groupnorm_pad: x [n][h][w][c0] (+ x2) -> out [n][h + 2][w + 2][c0 + c1], zero border."""
    n, h, w, c0 = x.shape
    c1 = x2.shape[-1] if x2 is not None else 0
    wsb = lib().c2d_groupnorm_pad_workspace_size(n, c0 + c1, h, w)
    ws = torch.empty((wsb + 15) // 16 * 4, device=x.device, dtype=torch.float32)
    check(lib().c2d_groupnorm_pad(ptr(x), ptr(x2), c0, c1, n, h, w, groups, eps, ptr(gamma), ptr(beta), int(silu),
                                  ptr(out), ptr(ws), wsb, stream_ptr()), "c2d_groupnorm_pad")


@custom_op("c2d::groupnorm_moments", mutates_args=("out",), device_types=_CU)
def groupnorm_moments(x: Tensor, groups: int, eps: float, gamma: Tensor, beta: Tensor, silu: bool, mom: Tensor,
                      rows: int, pad: bool, out: Tensor) -> None:
    """c2d_groupnorm_moments: x [n][h][w][c] normalised with the {mean, M2} moments its producing conv
    wrote (mom [n][h*w / rows][groups][2]) -> out [n][h][w][c], or with pad the zero-bordered
    [n][h + 2][w + 2][c]."""
    n, h, w, c = x.shape
    check(lib().c2d_groupnorm_moments(ptr(x), c, n, h * w, groups, eps, ptr(gamma), ptr(beta), int(silu), ptr(mom),
                                      rows, w + 2 if pad else 0, ptr(out), stream_ptr()), "c2d_groupnorm_moments")


@custom_op("c2d::layernorm_stats", mutates_args=("stats",), device_types=_CU)
def layernorm_stats(x: Tensor, eps: float, stats: Tensor) -> None:
    m, c = x.shape
    check(lib().c2d_layernorm_stats(ptr(x), m, c, x.stride(0), eps, ptr(stats), stream_ptr()), "c2d_layernorm_stats")


@custom_op("c2d::layernorm", mutates_args=("out",), device_types=_CU)
def layernorm(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, out: Tensor) -> None:
    m, c = x.shape
    check(lib().c2d_layernorm(ptr(x), m, c, x.stride(0), eps, ptr(gamma), ptr(beta), ptr(out), out.stride(0),
                              stream_ptr()), "c2d_layernorm")


@custom_op("c2d::attention_fwd", mutates_args=("out",), device_types=_CU)
def attention_fwd(q: Tensor, k: Tensor, v: Tensor, batch: int, heads: int, lq: int, lk: int, d: int, scale: float,
                  key_bias: Optional[Tensor], bias_ld_batch: int, bias_ld_head: int, out: Tensor,
                  bias_ld_query: int = 0) -> None:
    """c2d_attention_fwd, or c2d_attention_fwd_mask with an additive score bias (bias_ld_query 0:
    a per-key bias, else a query-varying one)."""
    if key_bias is None:
        check(lib().c2d_attention_fwd(ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(out),
                                      out.stride(0), batch, heads, lq, lk, d, scale, 1, stream_ptr()), "c2d_attention_fwd")
    else:
        check(lib().c2d_attention_fwd_mask(ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(out),
                                           out.stride(0), batch, heads, lq, lk, d, scale, 1, ptr(key_bias),
                                           bias_ld_batch, bias_ld_head, bias_ld_query, stream_ptr()),
              "c2d_attention_fwd_mask")


@custom_op("c2d::attention_small", mutates_args=("out",), device_types=_CU)
def attention_small(q: Tensor, k: Tensor, v: Tensor, batch: int, heads: int, l: int, d: int, scale: float,
                    causal: bool, out: Tensor) -> None:
    check(lib().c2d_attention_small(ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(out),
                                    out.stride(0), batch, heads, l, d, scale, int(causal), stream_ptr()),
          "c2d_attention_small")


@custom_op("c2d::window_attention", mutates_args=("out",), device_types=_CU)
def window_attention(qkv: Tensor, row_map: Tensor, n_windows: int, heads: int, d: int, bias: Tensor,
                     mask: Optional[Tensor], out: Tensor) -> None:
    n_mask = mask.shape[0] if mask is not None else 0
    check(lib().c2d_window_attention(ptr(qkv), qkv.stride(0), ptr(row_map), n_windows, heads, d, ptr(bias), ptr(mask),
                                     n_mask, ptr(out), out.stride(0), stream_ptr()), "c2d_window_attention")


@custom_op("c2d::htsat_mel_patches", mutates_args=("out",), device_types=_CU)
def htsat_mel_patches(mel: Tensor, bn_scale: Tensor, bn_shift: Tensor, out: Tensor) -> None:
    b, t, _ = mel.shape
    check(lib().c2d_htsat_mel_patches(ptr(mel), b, t, ptr(bn_scale), ptr(bn_shift), ptr(out), stream_ptr()),
          "c2d_htsat_mel_patches")


@custom_op("c2d::patch_merge_gather", mutates_args=("out",), device_types=_CU)
def patch_merge_gather(x: Tensor, b: int, h: int, w: int, c: int, out: Tensor) -> None:
    check(lib().c2d_patch_merge_gather(ptr(x), b, h, w, c, ptr(out), stream_ptr()), "c2d_patch_merge_gather")


@custom_op("c2d::row_mean", mutates_args=("out",), device_types=_CU)
def row_mean(x: Tensor, b: int, rows: int, out: Tensor) -> None:
    check(lib().c2d_row_mean(ptr(x), b, rows, x.shape[1], x.stride(0), ptr(out), stream_ptr()), "c2d_row_mean")


@custom_op("c2d::softmax_rows", mutates_args=("out",), device_types=_CU)
def softmax_rows(x: Tensor, out: Tensor) -> None:
    check(lib().c2d_softmax_rows(ptr(x), x.shape[0], x.shape[1], x.stride(0), ptr(out), out.stride(0), stream_ptr()),
          "c2d_softmax_rows")


@custom_op("c2d::l2_normalize", mutates_args=("x",), device_types=_CU)
def l2_normalize(x: Tensor) -> None:
    m, c = x.shape
    check(lib().c2d_l2_normalize(ptr(x), m, c, stream_ptr()), "c2d_l2_normalize")


@custom_op("c2d::clap_log_mel", mutates_args=("out",), device_types=_CU)
def clap_log_mel(wave: Tensor, offsets: Tensor, lengths: Tensor, max_len: int, n_fft: int, hop: int, window: Tensor,
                 filters: Tensor, filter_range: Tensor, n_mels: int, out: Tensor) -> None:
    check(lib().c2d_clap_log_mel(ptr(wave), ptr(offsets), ptr(lengths), offsets.numel(), max_len, n_fft, hop,
                                 ptr(window), ptr(filters), ptr(filter_range), n_mels, ptr(out), stream_ptr()),
          "c2d_clap_log_mel")


@custom_op("c2d::timestep_embedding", mutates_args=("out",), device_types=_CU)
def timestep_embedding(t_table: Tensor, step_index: Optional[Tensor], n: int, dim: int, out: Tensor) -> None:
    check(lib().c2d_timestep_embedding(ptr(t_table), ptr(step_index), n, dim, ptr(out), stream_ptr()),
          "c2d_timestep_embedding")


@custom_op("c2d::cfg_ddim_step", mutates_args=("x", "step_index"), device_types=_CU)
def cfg_ddim_step(eps: Tensor, x: Tensor, guidance: float, coef: Tensor, step_index: Tensor, advance: bool) -> None:
    b, c, hgt, wid = x.shape
    check(lib().c2d_cfg_ddim_step(ptr(eps), ptr(x), b, c, hgt * wid, guidance, ptr(coef), ptr(step_index), int(advance),
                                  stream_ptr()), "c2d_cfg_ddim_step")


@custom_op("c2d::latent_to_nhwc", mutates_args=("out",), device_types=_CU)
def latent_to_nhwc(x: Tensor, cpad: int, dup: bool, out: Tensor) -> None:
    b, c, hgt, wid = x.shape
    check(lib().c2d_latent_to_nhwc(ptr(x), b, c, hgt * wid, cpad, int(dup), ptr(out), stream_ptr()),
          "c2d_latent_to_nhwc")


@custom_op("c2d::image_to_nhwc", mutates_args=("out",), device_types=_CU)
def image_to_nhwc(img: Tensor, out: Tensor) -> None:
    """c2d_image_to_nhwc: uint8 [n][h][w][3] -> fp16 [n][h][w][8], u / 127.5 - 1 and five zero channels."""
    n, h, w, _ = img.shape
    check(lib().c2d_image_to_nhwc(ptr(img), n, h * w, ptr(out), stream_ptr()), "c2d_image_to_nhwc")


@custom_op("c2d::vae_posterior_noise", mutates_args=("x",), device_types=_CU)
def vae_posterior_noise(moments: Tensor, eps: Optional[Tensor], noise: Optional[Tensor], coef: Optional[Tensor],
                        step_index: Optional[Tensor], scaling: float, x: Tensor) -> None:
    """c2d_vae_posterior_noise: moments fp16 [n * hw][ld] -> x fp32 [n][4][h][w] (sample or mode, * scaling,
    add_noise at coef[*step_index] when noise is given)."""
    n = x.shape[0]
    hw = x.numel() // (4 * n)
    check(lib().c2d_vae_posterior_noise(ptr(moments), moments.stride(0), ptr(eps), ptr(noise), ptr(coef),
                                        ptr(step_index), n, hw, scaling, ptr(x), stream_ptr()),
          "c2d_vae_posterior_noise")


@custom_op("c2d::cfg_ddim_step_masked", mutates_args=("x", "step_index"), device_types=_CU)
def cfg_ddim_step_masked(eps: Tensor, x: Tensor, z0: Tensor, noise: Tensor, mask: Tensor, guidance: float,
                         coef: Tensor, step_index: Tensor, advance: bool) -> None:
    """c2d_cfg_ddim_step_masked: the CFG + DDIM update of x [b][4][h][w] blended with the known region (z0, noise
    as x; mask fp32 [b][h][w]); the number of steps is coef's row count."""
    b, _, hgt, wid = x.shape
    check(lib().c2d_cfg_ddim_step_masked(ptr(eps), ptr(x), ptr(z0), ptr(noise), ptr(mask), b, hgt * wid,
                                         coef.shape[0], guidance, ptr(coef), ptr(step_index), int(advance),
                                         stream_ptr()), "c2d_cfg_ddim_step_masked")


@custom_op("c2d::mask_to_latent", mutates_args=("out",), device_types=_CU)
def mask_to_latent(mask_u8: Tensor, out: Tensor) -> None:
    """c2d_mask_to_latent: uint8 [n][8h][8w] -> fp32 [n][h][w], 1 where the sample at (8y, 8x) is >= 128."""
    n, h, w = out.shape
    check(lib().c2d_mask_to_latent(ptr(mask_u8), n, h, w, ptr(out), stream_ptr()), "c2d_mask_to_latent")


@custom_op("c2d::composite_u8", mutates_args=("out",), device_types=_CU)
def composite_u8(decoded: Tensor, original: Tensor, mask_u8: Tensor, out: Tensor) -> None:
    """c2d_composite_u8: out = mask_u8 >= 128 ? decoded : original over uint8 [n][h][w][3] images."""
    check(lib().c2d_composite_u8(ptr(decoded), ptr(original), ptr(mask_u8), mask_u8.numel(), ptr(out), stream_ptr()),
          "c2d_composite_u8")


@custom_op("c2d::inpaint_prepare", mutates_args=("z0", "x", "mask"), device_types=_CU)
def inpaint_prepare(moments: Tensor, eps: Optional[Tensor], noise: Tensor, mask_u8: Tensor, coef: Optional[Tensor],
                    step_index: Optional[Tensor], pure_noise: bool, scaling: float, z0: Tensor, x: Tensor,
                    mask: Tensor) -> None:
    """c2d_inpaint_prepare: moments fp16 [n * h * w][ld], mask_u8 [n][8h][8w] -> z0, x fp32 [n][4][h][w] and mask
    fp32 [n][h][w] (the posterior sample or mode * scaling, the loop's first latents, the latent mask)."""
    n, h, w = mask.shape
    check(lib().c2d_inpaint_prepare(ptr(moments), moments.stride(0), ptr(eps), ptr(noise), ptr(mask_u8), ptr(coef),
                                    ptr(step_index), int(pure_noise), n, h, w, scaling, ptr(z0), ptr(x), ptr(mask),
                                    stream_ptr()), "c2d_inpaint_prepare")


@custom_op("c2d::cfg_dpm_step", mutates_args=("x", "x0_prev", "step_index"), device_types=_CU)
def cfg_dpm_step(eps: Tensor, x: Tensor, x0_prev: Tensor, guidance: float, mcoef: Tensor, step_index: Tensor,
                 first_step: Tensor, advance: bool) -> None:
    """c2d_cfg_dpm_step: the CFG + DPM-Solver++(2M) update of x [b][4][h][w] and x0_prev (as x); the number of
    steps is mcoef's row count."""
    b, _, hgt, wid = x.shape
    check(lib().c2d_cfg_dpm_step(ptr(eps), ptr(x), ptr(x0_prev), b, hgt * wid, mcoef.shape[0], guidance, ptr(mcoef),
                                 ptr(step_index), ptr(first_step), int(advance), stream_ptr()), "c2d_cfg_dpm_step")


@custom_op("c2d::cfg_dpm_step_masked", mutates_args=("x", "x0_prev", "step_index"), device_types=_CU)
def cfg_dpm_step_masked(eps: Tensor, x: Tensor, x0_prev: Tensor, z0: Tensor, noise: Tensor, mask: Tensor,
                        guidance: float, mcoef: Tensor, step_index: Tensor, first_step: Tensor,
                        advance: bool) -> None:
    """c2d_cfg_dpm_step_masked: cfg_dpm_step blended with the known region (z0, noise as x; mask fp32 [b][h][w])."""
    b, _, hgt, wid = x.shape
    check(lib().c2d_cfg_dpm_step_masked(ptr(eps), ptr(x), ptr(x0_prev), ptr(z0), ptr(noise), ptr(mask), b, hgt * wid,
                                        mcoef.shape[0], guidance, ptr(mcoef), ptr(step_index), ptr(first_step),
                                        int(advance), stream_ptr()), "c2d_cfg_dpm_step_masked")


@custom_op("c2d::clip_preprocess", mutates_args=("out",), device_types=_CU)
def clip_preprocess(img: Tensor, size: int, patch: int, mean: list[float], std: list[float], out: Tensor) -> None:
    """c2d_clip_preprocess: uint8 [n][h][w][3] -> fp16 [n * (size / patch)^2][kpad] normalised patch rows (PIL
    bicubic resize of the shorter side to `size`, centre crop, (v / 255 - mean) / std, patch cut)."""
    n, h, w, _ = img.shape
    f3 = ctypes.c_float * 3
    check(lib().c2d_clip_preprocess(ptr(img), n, h, w, size, patch, f3(*mean), f3(*std), out.shape[1], ptr(out),
                                    stream_ptr()), "c2d_clip_preprocess")


@custom_op("c2d::cosine_rows", mutates_args=("out",), device_types=_CU)
def cosine_rows(a: Tensor, b: Tensor, out: Tensor) -> None:
    """c2d_cosine_rows: fp32 [m][c] row pairs -> out fp32 [m], a_i . b_i / max(|a_i| |b_i|, 1e-12)."""
    m, c = a.shape
    check(lib().c2d_cosine_rows(ptr(a), ptr(b), m, c, ptr(out), stream_ptr()), "c2d_cosine_rows")


@custom_op("c2d::upsample_nearest2x", mutates_args=("out",), device_types=_CU)
def upsample_nearest2x(x: Tensor, out: Tensor) -> None:
    n, h, w, c = x.shape
    check(lib().c2d_upsample_nearest2x(ptr(x), n, h, w, c, ptr(out), stream_ptr()), "c2d_upsample_nearest2x")


@custom_op("c2d::add", mutates_args=("out",), device_types=_CU)
def add(a: Tensor, b: Tensor, out: Tensor) -> None:
    check(lib().c2d_add(ptr(a), ptr(b), ptr(out), a.numel(), stream_ptr()), "c2d_add")


# fake (meta) implementations: every op only mutates caller-allocated outputs
for _op in (pack_weights, groupnorm_stats, groupnorm_apply, groupnorm, groupnorm_pad, groupnorm_moments, layernorm_stats, layernorm, attention_fwd,
            attention_small, window_attention, htsat_mel_patches, patch_merge_gather, row_mean, softmax_rows,
            l2_normalize, clap_log_mel, timestep_embedding, cfg_ddim_step, latent_to_nhwc, upsample_nearest2x, add,
            image_to_nhwc, vae_posterior_noise, cfg_ddim_step_masked, mask_to_latent, composite_u8, inpaint_prepare,
            cfg_dpm_step, cfg_dpm_step_masked, clip_preprocess, cosine_rows):
    _op.register_fake(lambda *args, **kwargs: None)

OPS = ("conv2d_igemm", "pack_weights", "groupnorm_stats", "groupnorm_apply", "groupnorm", "groupnorm_pad", "groupnorm_moments",
       "layernorm_stats",
       "layernorm", "attention_fwd", "attention_small", "window_attention", "htsat_mel_patches", "patch_merge_gather",
       "row_mean", "softmax_rows", "l2_normalize", "clap_log_mel", "timestep_embedding", "cfg_ddim_step",
       "latent_to_nhwc", "upsample_nearest2x", "add", "image_to_nhwc", "vae_posterior_noise",
       "cfg_ddim_step_masked", "mask_to_latent", "composite_u8", "inpaint_prepare",
       "cfg_dpm_step", "cfg_dpm_step_masked", "clip_preprocess", "cosine_rows")
