"""The SD1.5 AutoencoderKL decoder and encoder as ordered stages, for tests/test_vae_stages_cpu.py and
tests/test_vae_stages_gpu.py.  CPU only: nothing here launches a kernel.  Activations are NHWC throughout, as the
HIP modules hold them; the weights are a diffusers-keyed state dict (weights.synth_vae_decoder / _encoder).

Three ways to run a stage (the convention of tests/small_shape_ref.py):
  trace       float64 on the original fp32 weights, nothing rounded: the network itself.  `trace(x)` chains the stages
              and returns every stage's float64 input and output.
  stage_ref   float64 on an fp16-rounded input, with conv / linear weights rounded to fp16 (what HConv2d / HLinear
              hold); GroupNorm affine and all biases stay fp32.  What the kernel should compute from what it reads.
  stage_emul  the same stage in fp32 with every tensor the HIP modules store rounded to fp16: the GroupNorm(+SiLU)
              output, each conv output (the shortcut's too), q (from to_q with 1/sqrt(c) folded in and rounded again,
              VAEAttention.finalize), k, V^T, the scores, the probabilities, P V + b_v, and the stage output.
The bar of a stage is small_shape_ref.bar_of / bar_l2_of(stage_emul, stage_ref): max(3 E, half-ulp floor), capped.

An upsampler's emulation is the folded form (four 2x2 phase convs whose weights are summed in fp32 and rounded to fp16
once, ops.fold_upsample_weight), because that is what Upsample2D runs wherever the library takes it; its reference is
the plain nearest x2 + 3x3 with the fp16-rounded 3x3 weights.  E therefore holds the fold's own weight rounding, and
the materialised form (stage_emul(..., folded=False)) lies inside the same bar.

Defects (stage_ref(..., defect=)): each is a float64 run of the stage with one thing wrong, and has to land outside
the stage's bar (tests/test_vae_stages_cpu.py):
  qscale     to_q (weight and bias) x 1.1: a 10 % error in the softmax scale
  vbias      b_v dropped
  image      the attention of image i uses image 0's keys (n > 1)
  phase      upsampler phases (0, 1) and (1, 0) use each other's weights (small_shape_ref.upfold_ref's defect)
  shortcut   conv_shortcut's bias dropped (the resnets that change width)
  padbefore  the encoder downsampler pads before the image instead of after
  normeps    a resnet's two GroupNorms (or the attention's, or the final one) run with eps 1e-2 for 1e-6
'eps' (GroupNorm eps 1e-5 for 1e-6 in the final norm) is kept only to show it cannot be held to a bar: the groups'
variances there are 0.26 to 0.68, so it moves the output by 1.3e-5 relative and 2e-5 at most, a twentieth of half an
fp16 ulp of the output; fp16 storage cannot resolve it (test_vae_stages_cpu.test_eps_1e5_is_below_fp16).  'normeps'
stands in for it with a wrong eps that can be seen.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from clap2diffusion_amd import ops
from tests import small_shape_ref as R

F64, F32 = torch.float64, torch.float32
SCALING = 0.18215
GROUPS = 32
EPS = 1e-6

# decoder latents (n, h, w) and encoder images (n, H, W): the smallest the mid attention takes (h w % 64 == 0), an
# odd batch for the per-image row slices, and a non-square one
DEC_CASES = [(1, 8, 8), (3, 8, 8), (2, 8, 16)]
ENC_CASES = [(1, 64, 64), (3, 64, 64), (2, 64, 128)]
# The clamp case: AutoencoderKL ends in GroupNorm -> SiLU -> conv_out, so the image's spread (std ~ 0.16 around 0)
# is set by conv_out and no scale of the latents moves it: x1, x4 and x64 latents all leave under 0.1 % of the
# pixels at 0 or 255.  The saturating case therefore decodes x4 latents with decoder.conv_out's bias moved by
# SAT_BIAS: red sits near the top of the range, green near the bottom, about 15 % of all pixels clamp (half at each
# end) and the errors keep their size in grey levels, which a gain on conv_out's weight would multiply.
SAT_CASE = (1, 8, 8)
SAT_LATENT_SCALE = 4.0
SAT_BIAS = (0.9, -0.9, 0.0)


def latents_of(n, h, w, seed=0, scale=1.0):
    return R.gen(n, 4, h, w, seed=1000 + seed) * scale * SCALING


def image_of(n, h, w, seed=0):
    """uint8 NHWC: smooth colour gradients plus noise."""
    g = torch.Generator().manual_seed(2000 + seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    base = torch.stack([yy, xx, 1 - 0.5 * (yy + xx)], dim=-1)[None].repeat(n, 1, 1, 1)
    img = 0.5 + 0.4 * torch.sin(6.0 * (base + torch.rand(n, 1, 1, 3, generator=g))) + \
        0.05 * torch.randn(n, h, w, 3, generator=g)
    return (img.clamp(0, 1) * 255).round().to(torch.uint8)


def saturating_sd(sd: dict) -> dict:
    out = dict(sd)
    out["decoder.conv_out.bias"] = sd["decoder.conv_out.bias"].float() + torch.tensor(SAT_BIAS)
    return out


def quantize(x: torch.Tensor) -> torch.Tensor:
    """Pre-affine RGB -> uint8, as VAEDecoder.quantize: (x / 2 + 0.5) clamped to [0, 1], x 255, rounded."""
    return ((x[..., :3] / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8)


def saturated_share(img_u8: torch.Tensor) -> float:
    return ((img_u8 == 0) | (img_u8 == 255)).float().mean().item()


class _Mode:
    """How one run treats numbers: dtype of the arithmetic, whether conv / linear weights are rounded to fp16, and
    whether stored tensors are."""

    def __init__(self, sd, dtype, w16, store16):
        self.sd, self.dtype, self.w16, self.store16 = sd, dtype, w16, store16
        self.cache = {}

    def w(self, key, scale=1.0):
        """conv [cout, cin, k, k] -> taps [k, k, cin, cout]; linear [cout, cin] -> [cin, cout]."""
        ck = (key, scale)
        if ck not in self.cache:
            w = self.sd[key + ".weight"].float()
            if self.w16:
                w = w.half().float()
                if scale != 1.0:
                    w = (w * scale).half().float()       # VAEAttention.finalize: the held fp16 weight, scaled, rounded
            elif scale != 1.0:
                w = w.double() * scale
            w = w.to(self.dtype)
            self.cache[ck] = w.permute(2, 3, 1, 0).contiguous() if w.dim() == 4 else w.t().contiguous()
        return self.cache[ck]

    def b(self, key):
        return self.sd[key + ".bias"].float().to(self.dtype)

    def st(self, t):
        return t.half().to(self.dtype) if self.store16 else t


def _conv(m: _Mode, key, x, stride=1, pad_before=False, bias=True):
    """NHWC conv by taps: 1x1; 3x3 pad 1 stride 1; 3x3 stride 2 padded after the image (pad_before: before it)."""
    wt = m.w(key)
    b = m.b(key) if bias else 0.0
    if wt.dim() == 2 or wt.shape[0] == 1:
        return x @ wt.reshape(wt.shape[-2], wt.shape[-1]) + b
    n, h, w, _ = x.shape
    if stride == 1:
        xp, oh, ow = F.pad(x, (0, 0, 1, 1, 1, 1)), h, w
    else:
        xp, oh, ow = F.pad(x, (0, 0, 1, 0, 1, 0) if pad_before else (0, 0, 0, 1, 0, 1)), h // 2, w // 2
    out = None
    for ky in range(3):
        for kx in range(3):
            slab = xp[:, ky:ky + (oh - 1) * stride + 1:stride, kx:kx + (ow - 1) * stride + 1:stride, :]
            term = slab.reshape(-1, slab.shape[-1]) @ wt[ky, kx]
            out = term if out is None else out + term
    return (out + b).view(n, oh, ow, -1)


def _gn(m: _Mode, key, x, silu, eps=EPS):
    return R.gn_ref(x, m.sd[key + ".weight"].float(), m.sd[key + ".bias"].float(), GROUPS, eps, silu, dtype=m.dtype)


def _resnet(m: _Mode, key, x, defect=None):
    eps = 1e-2 if defect == "normeps" else EPS
    h = m.st(_conv(m, key + ".conv1", m.st(_gn(m, key + ".norm1", x, True, eps))))
    h = _conv(m, key + ".conv2", m.st(_gn(m, key + ".norm2", h, True, eps)))
    if key + ".conv_shortcut.weight" in m.sd:
        x = m.st(_conv(m, key + ".conv_shortcut", x, bias=defect != "shortcut"))
    return m.st(h + x)


def _attention(m: _Mode, key, x, defect=None):
    """x + to_out(softmax(q k^T / sqrt(c)) v) as VAEAttention runs it: 1/sqrt(c) inside to_q, V^T without its bias,
    fp16 scores, the softmax's fp16 probabilities, b_v added to P V (the rows of P sum to 1)."""
    n, h, w, c = x.shape
    sc = c ** -0.5
    xn = m.st(_gn(m, key + ".group_norm", x, False, 1e-2 if defect == "normeps" else EPS)).view(n, h * w, c)
    gain = 1.1 if defect == "qscale" else 1.0
    q = m.st((xn @ m.w(key + ".to_q", sc) + m.b(key + ".to_q") * sc) * gain)
    k = m.st(xn @ m.w(key + ".to_k") + m.b(key + ".to_k"))
    v = m.st(xn @ m.w(key + ".to_v"))
    if defect == "image":
        k = k[:1].expand_as(k)
    p = m.st(torch.softmax(m.st(q @ k.transpose(1, 2)), dim=-1))
    o = p @ v
    if defect != "vbias":
        o = o + m.b(key + ".to_v")
    o = m.st(o)
    return m.st(o @ m.w(key + ".to_out.0") + m.b(key + ".to_out.0") + x.reshape(n, h * w, c)).view(n, h, w, c)


def _upsample(m: _Mode, key, x, defect=None, folded=True):
    if m.store16 and folded or defect == "phase":
        w3 = m.sd[key + ".weight"].float()
        wf = ops.fold_upsample_weight(w3)[0].view(4, w3.shape[0], 2, 2, w3.shape[1])
        return m.st(R.upfold_ref(x, wf, m.b(key), dtype=m.dtype, defect=defect))
    return m.st(_conv(m, key, x.repeat_interleave(2, 1).repeat_interleave(2, 2)))


def _norm_conv_out(m: _Mode, prefix, x, defect=None):
    eps = 1e-2 if defect == "normeps" else 1e-5 if defect == "eps" else EPS
    return m.st(_conv(m, prefix + "conv_out", m.st(_gn(m, prefix + "conv_norm_out", x, True, eps))))


class VaeStages:
    """One half of the VAE ('decoder' or 'encoder') over a diffusers-keyed state dict."""

    def __init__(self, sd: dict, half: str):
        assert half in ("decoder", "encoder")
        self.half = half
        self.sd = {k: v.float() for k, v in sd.items()}
        self.modes = {"trace": _Mode(self.sd, F64, False, False), "ref": _Mode(self.sd, F64, True, False),
                      "emul": _Mode(self.sd, F32, True, True)}
        self.stages = self._decoder() if half == "decoder" else self._encoder()
        self.fn = dict(self.stages)
        self.names = [n for n, _ in self.stages]

    # every stage function: (mode, x, **kw) -> y
    def _decoder(self):
        p = "decoder."
        st = [("post_quant_conv", lambda m, x, **kw: m.st(_conv(m, "post_quant_conv", x))),
              ("conv_in", lambda m, x, **kw: m.st(_conv(m, p + "conv_in", x))),
              ("mid.resnets.0", lambda m, x, **kw: _resnet(m, p + "mid_block.resnets.0", x, **kw)),
              ("mid.attentions.0", lambda m, x, **kw: _attention(m, p + "mid_block.attentions.0", x, **kw)),
              ("mid.resnets.1", lambda m, x, **kw: _resnet(m, p + "mid_block.resnets.1", x, **kw))]
        for i in range(4):
            for j in range(3):
                st.append((f"up_blocks.{i}.resnets.{j}",
                           lambda m, x, k=f"{p}up_blocks.{i}.resnets.{j}", **kw: _resnet(m, k, x, **kw)))
            if i < 3:
                st.append((f"up_blocks.{i}.upsamplers.0",
                           lambda m, x, k=f"{p}up_blocks.{i}.upsamplers.0.conv", **kw: _upsample(m, k, x, **kw)))
        st.append(("conv_norm_out+conv_out", lambda m, x, **kw: _norm_conv_out(m, p, x, **kw)))
        return st

    def _encoder(self):
        p = "encoder."
        st = [("conv_in", lambda m, x, **kw: m.st(_conv(m, p + "conv_in", x)))]
        for i in range(4):
            for j in range(2):
                st.append((f"down_blocks.{i}.resnets.{j}",
                           lambda m, x, k=f"{p}down_blocks.{i}.resnets.{j}", **kw: _resnet(m, k, x, **kw)))
            if i < 3:
                st.append((f"down_blocks.{i}.downsamplers.0",
                           lambda m, x, k=f"{p}down_blocks.{i}.downsamplers.0.conv", defect=None:
                           m.st(_conv(m, k, x, stride=2, pad_before=defect == "padbefore"))))
        st += [("mid.resnets.0", lambda m, x, **kw: _resnet(m, p + "mid_block.resnets.0", x, **kw)),
               ("mid.attentions.0", lambda m, x, **kw: _attention(m, p + "mid_block.attentions.0", x, **kw)),
               ("mid.resnets.1", lambda m, x, **kw: _resnet(m, p + "mid_block.resnets.1", x, **kw)),
               ("conv_norm_out+conv_out", lambda m, x, **kw: _norm_conv_out(m, p, x, **kw)),
               ("quant_conv", lambda m, x, **kw: m.st(_conv(m, "quant_conv", x)))]
        return st

    def defects(self, name: str, n: int) -> list:
        """The planted defects that apply to a stage at batch n."""
        if "attentions" in name:
            return ["qscale", "vbias", "normeps"] + (["image"] if n > 1 else [])
        if "upsamplers" in name:
            return ["phase"]
        if "downsamplers" in name:
            return ["padbefore"]
        if "resnets" in name:
            key = self.half + "." + name.replace("mid.", "mid_block.")
            return ["normeps"] + (["shortcut"] if key + ".conv_shortcut.weight" in self.sd else [])
        if name == "conv_norm_out+conv_out":
            return ["normeps"]
        return []

    def first_input(self, x: torch.Tensor) -> torch.Tensor:
        """Decoder: scaled latents [B, 4, h, w] -> latents / 0.18215 (in fp32, as VAEDecoder divides) NHWC float64.
        Encoder: uint8 NHWC image -> image / 127.5 - 1."""
        if self.half == "decoder":
            return (x.float() / SCALING).permute(0, 2, 3, 1).contiguous().double()
        return x.double() / 127.5 - 1.0

    def trace(self, x: torch.Tensor) -> list:
        """[(stage, float64 input, float64 output)] of the network on its original weights."""
        m, out = self.modes["trace"], []
        y = self.first_input(x)
        for name, fn in self.stages:
            x_in, y = y, fn(m, y)
            out.append((name, x_in, y))
        return out

    def stage_ref(self, name: str, x16: torch.Tensor, defect=None) -> torch.Tensor:
        kw = {"defect": defect} if defect else {}
        return self.fn[name](self.modes["ref"], x16.double(), **kw)

    def stage_emul(self, name: str, x16: torch.Tensor, folded: bool = True) -> torch.Tensor:
        kw = {} if folded else {"folded": False}
        return self.fn[name](self.modes["emul"], x16.float(), **kw).half()

    def chain_emul(self, x: torch.Tensor) -> torch.Tensor:
        """The emulation end to end: every stage on the fp16 output of the one before."""
        y = self.first_input(x).half()
        for name in self.names:
            y = self.stage_emul(name, y)
        return y


def stage_table(vs: VaeStages, x: torch.Tensor) -> list:
    """Per stage of the trace on x: name, the fp16-rounded input the kernel is fed, stage_ref and stage_emul on it,
    and both bars ((E, bar) of max|.|, (E, bar) of rel-L2)."""
    rows = []
    for name, x_in, _ in vs.trace(x):
        x16 = x_in.half()
        ref, emu = vs.stage_ref(name, x16), vs.stage_emul(name, x16)
        rows.append({"name": name, "x16": x16, "ref": ref, "emu": emu,
                     "bar": R.bar_of(emu, ref), "bar_l2": R.bar_l2_of(emu, ref)})
    return rows
