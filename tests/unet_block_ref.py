"""The SD1.5 UNet2DConditionModel as ordered stages over the diffusers state-dict keys, for tests/test_unet_blocks_cpu.py
and tests/test_unet_blocks_gpu.py.  CPU only: nothing here launches a kernel, and no product module is imported but
`weights` (the seeded recipes).  Activations are NHWC, as the HIP modules hold them.

Ways to run a stage (the convention of tests/vae_stage_ref.py):
  trace   float64 on the original fp32 weights, nothing rounded: the network itself.  `trace(inputs)` chains the stages,
          skip stack included, and returns every stage's float64 inputs and output ('trace32': the same in fp32).
  ref     float64 on fp16-rounded inputs, with conv / linear weights rounded to fp16 (what HConv2d / HLinear hold);
          norm affines and all biases stay fp32.  What the kernels should compute from what they read.
  emul    the same stage in fp32 with every tensor the HIP modules store rounded to fp16, in the default form of
          unet.py: each GroupNorm(+SiLU) / LayerNorm output, each conv / GEMM output, q / k / v, the softmax
          probabilities (small_shape_ref.attn_emul), the audio projection, its pooled gate and the K|V row it adds, the
          GEGLU product, and the folded [Wp | Wp W2] weight rounded once with h_ff never materialised.  Where the
          walker's `lnf_on(rows, c, cout, geglu)` says the LayerNorm runs inside the GEMM (BasicTransformerBlock._lnf_on,
          handed in by the tests: this file asks no library), the emulation rounds the normalised rows and W diag(gamma).
The bar of a stage is small_shape_ref.bar_of / bar_l2_of(emul, ref), unchanged.

Stages, in execution order (names(): 1 + 1 + 22 resnets + 16 transformers + 3 + 3 samplers + 1 = 47):
  time                    t_sin -> time_embedding.linear_1 (SiLU) -> linear_2 -> every resnet's time_emb_proj(SiLU(.))
                          side by side, resnet r at column temb_off[r] (UNet2DConditionModel.time_conditioning);
                          sinusoid(t) is the float64 embedding the kernel's fp16 t_sin is held to
  conv_in                 3x3, 4 -> 320 (the HIP module reads the input zero-padded to 8 channels)
  *.resnets.j             GN(1e-5)+SiLU, conv1 + temb, GN+SiLU, conv2, + x or conv_shortcut(x); x = cat[h, skip] upward
  *.attentions.j          GN(1e-6), proj_in, LN1 self-attention, LN2 cross-attention over ehs + sigmoid(alpha)
                          mean_tokens(audio_proj(audio[level])) with the encoder mask's key bias, LN3 GEGLU ff.net.2,
                          proj_out + x
  *.downsamplers.0        3x3 stride 2 pad 1;   *.upsamplers.0   nearest x2 then 3x3 (emul: the four folded phase convs)
  conv_norm_out+conv_out  GN(1e-5)+SiLU, 3x3 320 -> 4

Defects (stage(..., defect=)): a float64 run with one thing wrong; tests/test_unet_blocks_cpu.py lists them.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from clap2diffusion_amd.weights import SD15_UNET
from tests import small_shape_ref as R

F64, F32 = torch.float64, torch.float32
GROUPS, HEADS = 32, 8
LEVELS = ("early", "mid", "late")
# (n, h, w, keep): the two cases of the GPU stage test; keep = real tokens per image of the encoder mask
CASES = [(2, 16, 16, (9, 30)), (3, 16, 24, None)]


def level_of(name: str) -> str:
    """The audio level of a transformer: down 0-1 early, down 2 and up 0-1 late, the mid block and up 2-3 mid."""
    if name.startswith("mid_block"):
        return "mid"
    kind, i = name.split(".")[0], int(name.split(".")[1])
    if kind == "down_blocks":
        return "early" if i < 2 else "late"
    return "late" if i < 2 else "mid"


def inputs_of(n, h, w, keep=None, seed=0, t=601.0):
    g = torch.Generator().manual_seed(4000 + seed + 16 * n + h * w)
    inp = {"sample": torch.randn(n, 4, h, w, generator=g), "t": t, "ehs": torch.randn(n, 77, 768, generator=g),
           "audio": {lv: torch.randn(n, 10, 768, generator=g) * 0.5 for lv in LEVELS}, "keep": None}
    if keep is not None:
        inp["keep"] = torch.stack([(torch.arange(77) < k).float() for k in keep])
    return inp


def sinusoid(t, n, dim=320, dtype=F64):
    """diffusers get_timestep_embedding(flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin]."""
    half = dim // 2
    freq = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=dtype) / half)
    arg = torch.as_tensor(t, dtype=dtype).reshape(-1, 1).expand(n, 1) * freq
    return torch.cat([torch.cos(arg), torch.sin(arg)], -1)


class _Mode:
    """How one run treats numbers: dtype of the arithmetic, conv / linear weights rounded to fp16 or not, stored
    tensors rounded or not."""

    def __init__(self, sd, procs, dtype, w16, store16, lnf_on=None):
        self.sd, self.procs, self.dtype, self.w16, self.store16 = sd, procs, dtype, w16, store16
        self.lnf_on = lnf_on if store16 and lnf_on is not None else (lambda rows, c, cout, geglu: False)

    def cast(self, w):
        w = w.float()
        return (w.half().float() if self.w16 else w).to(self.dtype)

    def w(self, key):
        return self.cast(self.sd[key + ".weight"])

    def b(self, key):
        return self.sd[key + ".bias"].to(self.dtype)

    def st(self, t):
        return t.half().to(self.dtype) if self.store16 else t


def _lin(m, key, x, bias=True):
    y = x @ m.w(key).t()
    return y + m.b(key) if bias else y


def _conv(m, key, x, stride=1):
    """NHWC conv by taps: 1x1, or 3x3 pad 1 with stride 1 or 2."""
    w = m.w(key)
    if w.shape[-1] == 1:
        return x @ w.reshape(w.shape[0], -1).t() + m.b(key)
    n, h, wd, _ = x.shape
    oh, ow = (h - 1) // stride + 1, (wd - 1) // stride + 1
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = None
    for ky in range(3):
        for kx in range(3):
            slab = xp[:, ky:ky + (oh - 1) * stride + 1:stride, kx:kx + (ow - 1) * stride + 1:stride, :]
            term = slab.reshape(-1, slab.shape[-1]) @ w[:, :, ky, kx].t()
            out = term if out is None else out + term
    return (out + m.b(key)).view(n, oh, ow, -1)


def _gn(m, key, x, silu, eps, mom_of=None):
    """GroupNorm (+ SiLU) over 32 groups, biased variance; mom_of: the tensor whose group moments normalise x (the
    'moments of the wrong tensor' defect; None = x's own)."""
    n, h, w, c = x.shape

    def grouped(t):
        return t.reshape(n, t.shape[1] * t.shape[2], GROUPS, -1).permute(0, 2, 1, 3).reshape(n, GROUPS, -1)
    v, s = grouped(x), grouped(x if mom_of is None else mom_of)
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    y = ((v - mean) / torch.sqrt(var + eps)).reshape(n, GROUPS, h * w, c // GROUPS).permute(0, 2, 1, 3).reshape(n, h, w, c)
    y = y * m.sd[key + ".weight"].to(m.dtype) + m.sd[key + ".bias"].to(m.dtype)
    return y * torch.sigmoid(y) if silu else y


def _ln_linear(m, norm, x, w, b, geglu=False):
    """Linear(LayerNorm(x)) -> stored; folded into the GEMM where m.lnf_on says so: the panel's rows (x - mean) rstd
    rounded to fp16 against W diag(gamma) rounded to fp16, bias b + W beta."""
    gamma, beta = m.sd[norm + ".weight"].to(m.dtype), m.sd[norm + ".bias"].to(m.dtype)
    xh = (x - x.mean(-1, keepdim=True)) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + 1e-5)
    if m.lnf_on(x.numel() // x.shape[-1], x.shape[-1], w.shape[0], geglu):
        y = m.st(xh) @ m.st(w * gamma).t() + w @ beta
    else:
        y = m.st(xh * gamma + beta) @ w.t()
    if b is not None:
        y = y + b
    if geglu:
        hid, gate = y.chunk(2, -1)
        y = hid * 0.5 * gate * (1.0 + torch.erf(gate / math.sqrt(2.0)))
    return m.st(y)


def _attend(m, q, k, v, n, lq, lk, bias):
    """softmax(q k^T / sqrt(d) + bias) v per image and head on [n, l, c]; emul: fp32 scores, fp16 probabilities."""
    c = q.shape[-1]
    d = c // HEADS
    out = []
    for i in range(n):     # per image: bounded score memory at 64 x 64
        bi = None if bias is None else bias[i:i + 1]
        if m.store16:
            o = R.attn_emul(q[i].half(), k[i].half(), v[i].half(), bi, 1, HEADS, lq, lk, d)
        else:
            o = R.attn_ref(q[i], k[i], v[i], bi, 1, HEADS, lq, lk, d, dtype=m.dtype)
        out.append(o.to(m.dtype))
    return torch.stack(out)


def _context_kv(m, blk, level, ehs, audio):
    """K, V [n, 77, c] of a cross-attention over ehs + sigmoid(alpha) mean_tokens(audio_proj(audio[level])).  emul: as
    AudioAttnProcessor.context_kv forms it, K|V = ehs W^T + (gate pooled) W^T with every operand stored in fp16."""
    wk, wv = m.w(blk + ".attn2.to_k"), m.w(blk + ".attn2.to_v")
    p = m.procs.get(level) if audio is not None and level in audio else None
    if p is None:
        return m.st(ehs @ wk.t()), m.st(ehs @ wv.t())
    a = audio[level].to(m.dtype)
    a = a @ m.cast(p["audio_proj.0.weight"]).t() + p["audio_proj.0.bias"].to(m.dtype)
    a = m.st(a * 0.5 * (1.0 + torch.erf(a / math.sqrt(2.0))))
    a = m.st(a @ m.cast(p["audio_proj.3.weight"]).t() + p["audio_proj.3.bias"].to(m.dtype))
    gp = torch.sigmoid(p["alpha"].to(m.dtype)) * a.mean(1, keepdim=True)
    if not m.store16:
        ctx = ehs + gp
        return ctx @ wk.t(), ctx @ wv.t()
    gp = m.st(gp)
    return m.st(ehs @ wk.t() + m.st(gp @ wk.t())), m.st(ehs @ wv.t() + m.st(gp @ wv.t()))


def resnet(m, key, x, temb, skip=None, defect=None):
    """temb [n, cout]: this resnet's slice of the time stage.  defects: 'catswap' cat[skip, h]; 'mominput' norm2
    normalises conv1's output with the moments of the block's input."""
    xc = x if skip is None else torch.cat([skip, x] if defect == "catswap" else [x, skip], -1)
    h = _conv(m, key + ".conv1", m.st(_gn(m, key + ".norm1", xc, True, 1e-5)))
    h = m.st(h + temb.to(m.dtype)[:, None, None, :])
    mom = xc if defect == "mominput" else None      # any width: the moments are per group
    h = _conv(m, key + ".conv2", m.st(_gn(m, key + ".norm2", h, True, 1e-5, mom_of=mom)))
    res = m.st(_conv(m, key + ".conv_shortcut", xc)) if key + ".conv_shortcut.weight" in m.sd else xc
    return m.st(h + res)


def transformer(m, key, x, ehs, audio, bias, level=None, defect=None, mom_of=None, fold_ff=True):
    """x [n, h, w, c]; ehs [n', 77, 768] with n' = n, or n' = 2 n for a CFG pair whose halves share x (cfg_dup: the
    output is the pair's); bias: additive key bias [n', 1, 1, 77] or None.  defects: 'gneps' GroupNorm eps 1e-5;
    'gegluswap'; 'noresid' proj_out without + x; 'audiolevel' another level's audio; 'maskattn1' the key bias on the
    self-attention's first keys and none on attn2; 'mominput' the norm uses mom_of's moments; 'cfgstale' the pair's
    second half enters attn2 as it was before the self-attention.  fold_ff False: the two-GEMM form's storage."""
    n, hh, ww, c = x.shape
    level = level or level_of(key)
    if defect == "audiolevel":
        level = LEVELS[(LEVELS.index(level) + 1) % 3]
    blk = key + ".transformer_blocks.0"
    a = m.st(_gn(m, key + ".norm", x, False, 1e-5 if defect == "gneps" else 1e-6, mom_of if defect == "mominput" else None))
    h = m.st(_conv(m, key + ".proj_in", a)).view(n, hh * ww, c)
    l = hh * ww
    wqkv = torch.cat([m.w(blk + ".attn1.to_q"), m.w(blk + ".attn1.to_k"), m.w(blk + ".attn1.to_v")], 0)
    q, k, v = _ln_linear(m, blk + ".norm1", h, wqkv, None).chunk(3, -1)
    b1 = None
    if defect == "maskattn1" and bias is not None:
        b1 = F.pad(bias[:n, ..., :min(l, 77)].to(m.dtype), (0, max(l - 77, 0)))
    h0, h = h, m.st(_attend(m, q, k, v, n, l, l, b1) @ m.w(blk + ".attn1.to_out.0").t() + m.b(blk + ".attn1.to_out.0") + h)
    if ehs.shape[0] == 2 * n:
        h, x = torch.cat([h, h0 if defect == "cfgstale" else h], 0), torch.cat([x, x], 0)
        n = 2 * n
    q = _ln_linear(m, blk + ".norm2", h, m.w(blk + ".attn2.to_q"), None)
    kk, vv = _context_kv(m, blk, level, ehs.to(m.dtype), audio)
    o = _attend(m, q, kk, vv, n, l, 77, None if defect == "maskattn1" else bias)
    h = m.st(o @ m.w(blk + ".attn2.to_out.0").t() + m.b(blk + ".attn2.to_out.0") + h)
    w0, b0 = m.w(blk + ".ff.net.0.proj"), m.b(blk + ".ff.net.0.proj")
    if defect == "gegluswap":
        w0, b0 = torch.cat([w0[4 * c:], w0[:4 * c]], 0), torch.cat([b0[4 * c:], b0[:4 * c]], 0)
    g = _ln_linear(m, blk + ".norm3", h, w0, b0, geglu=True)
    wp, w2 = m.w(key + ".proj_out").reshape(c, c), m.w(blk + ".ff.net.2")
    x2 = x.reshape(n, l, c)
    if m.store16 and fold_ff:      # [Wp | Wp W2] in fp32 from the fp16 weights, rounded once; h_ff never stored
        y = h @ wp.t() + g @ m.st(wp @ w2).t() + (wp @ m.b(blk + ".ff.net.2") + m.b(key + ".proj_out"))
    else:
        y = m.st(g @ w2.t() + m.b(blk + ".ff.net.2") + h) @ wp.t() + m.b(key + ".proj_out")
    if defect != "noresid":
        y = y + x2
    return m.st(y).view(n, hh, ww, c)


def upsample(m, key, x, folded=True):
    """nearest x2 then 3x3; emul (folded): the four 2x2 phase convs, their taps summed in fp32 from the checkpoint
    weight and rounded to fp16 once (ops.fold_upsample_weight), as Upsample2D runs wherever the library takes it."""
    if not (m.store16 and folded):
        return m.st(_conv(m, key, x.repeat_interleave(2, 1).repeat_interleave(2, 2)))
    w3 = m.sd[key + ".weight"].float()
    taps = (((0,), (1, 2)), ((0, 1), (2,)))
    wf = w3.new_zeros(4, w3.shape[0], 2, 2, w3.shape[1])
    for a in range(2):
        for b in range(2):
            for ty in range(2):
                for tx in range(2):
                    for ky in taps[a][ty]:
                        for kx in taps[b][tx]:
                            wf[2 * a + b, :, ty, tx, :] += w3[:, :, ky, kx]
    return m.st(R.upfold_ref(x, wf.half(), m.b(key), dtype=m.dtype))


class UNetBlocks:
    """The walker: the UNet over a diffusers-keyed state dict and per-level processor weights."""

    def __init__(self, sd: dict, procs: dict | None = None, lnf_on=None, cfg: dict = SD15_UNET):
        self.sd = {k: v.float() for k, v in sd.items()}
        self.procs = {lv: {k: v.float() for k, v in p.items()} for lv, p in (procs or {}).items()}
        mk = lambda dtype, w16, s16: _Mode(self.sd, self.procs, dtype, w16, s16, lnf_on)   # noqa: E731
        self.modes = {"trace": mk(F64, False, False), "trace32": mk(F32, False, False), "ref": mk(F64, True, False),
                      "emul": mk(F32, True, True)}
        ch, nl = cfg["block_out_channels"], cfg["layers_per_block"]
        self.order = ["time", "conv_in"]
        self.resnets = []               # in temb column order: down, mid, up
        up = []
        for i in range(len(ch)):
            for j in range(nl):
                self.order.append(f"down_blocks.{i}.resnets.{j}")
                if cfg["attn_blocks"][i]:
                    self.order.append(f"down_blocks.{i}.attentions.{j}")
            if i < len(ch) - 1:
                self.order.append(f"down_blocks.{i}.downsamplers.0")
        self.order += ["mid_block.resnets.0", "mid_block.attentions.0", "mid_block.resnets.1"]
        for i in range(len(ch)):
            for j in range(nl + 1):
                up.append(f"up_blocks.{i}.resnets.{j}")
                if cfg["attn_blocks"][len(ch) - 1 - i]:
                    up.append(f"up_blocks.{i}.attentions.{j}")
            if i < len(ch) - 1:
                up.append(f"up_blocks.{i}.upsamplers.0")
        self.order += up + ["conv_norm_out+conv_out"]
        self.resnets = [s for s in self.order if ".resnets." in s]
        self.temb_off, off = {}, 0
        for r in self.resnets:
            self.temb_off[r] = off
            off += self.sd[r + ".conv1.weight"].shape[0]
        self.temb_total = off

    def names(self):
        return list(self.order)

    # ---------------------------------------------------------------- stages
    def time(self, m, t_sin):
        t1 = _lin(m, "time_embedding.linear_1", t_sin)
        temb = m.st(_lin(m, "time_embedding.linear_2", m.st(t1 * torch.sigmoid(t1))))
        s = m.st(temb * torch.sigmoid(temb))
        return m.st(torch.cat([_lin(m, r + ".time_emb_proj", s) for r in self.resnets], -1))

    def temb_slice(self, name, temb_all, defect=None):
        """This resnet's columns of the time stage; 'tembshift': as many columns from the neighbouring resnet's
        offset (the one after; the one before for the last)."""
        cout = self.sd[name + ".conv1.weight"].shape[0]
        if defect == "tembshift":
            i = self.resnets.index(name)
            name = self.resnets[i + 1 if i + 1 < len(self.resnets) else i - 1]
        off = self.temb_off[name]
        assert off + cout <= self.temb_total
        return temb_all[:, off:off + cout]

    def stage(self, name, mode, io, defect=None, **kw):
        """One stage on io = {x, skip, temb (the whole time-stage output), ehs, audio, bias, prev_x}."""
        m = self.modes[mode]
        c = lambda t: None if t is None else t.to(m.dtype)   # noqa: E731
        x = c(io["x"])
        if name == "time":
            return self.time(m, x)
        if name == "conv_in":
            return m.st(_conv(m, "conv_in", x))
        if name == "conv_norm_out+conv_out":
            return m.st(_conv(m, "conv_out", m.st(_gn(m, "conv_norm_out", x, True, 1e-5))))
        if ".resnets." in name:
            temb = self.temb_slice(name, io["temb"], defect)
            return resnet(m, name, x, temb, c(io.get("skip")), None if defect == "tembshift" else defect)
        if ".attentions." in name:
            audio = None if io.get("audio") is None else {k: c(v) for k, v in io["audio"].items()}
            return transformer(m, name, x, c(io["ehs"]), audio, io.get("bias"), defect=defect, mom_of=c(io.get("prev_x")), **kw)
        if ".downsamplers." in name:
            return m.st(_conv(m, name + ".conv", x, stride=2))
        return upsample(m, name + ".conv", x, **kw)

    def defects(self, name, io):
        if ".resnets." in name:
            return ["tembshift", "mominput"] + (["catswap"] if io.get("skip") is not None else [])
        if ".attentions." in name:
            d = ["gneps", "gegluswap", "noresid", "audiolevel", "mominput"]
            return d + (["maskattn1"] if io.get("bias") is not None else [])
        return []

    # ---------------------------------------------------------------- the whole network
    def context(self, inputs):
        bias = None
        if inputs.get("keep") is not None:
            bias = ((1.0 - inputs["keep"].float()) * -10000.0)[:, None, None, :]
        return {"ehs": inputs["ehs"], "audio": inputs.get("audio"), "bias": bias}

    def trace(self, inputs, mode="trace"):
        """[(stage, io, output)] of the network on its original weights, in execution order; io holds the stage's
        inputs as the trace produced them (x, skip, temb, prev_x) plus the shared context."""
        m = self.modes[mode]
        ctx = self.context(inputs)
        n = inputs["sample"].shape[0]
        out, skips, prev_x = [], [], None
        temb = h = None
        for name in self.order:
            io = dict(ctx)
            if name == "time":
                io["x"] = sinusoid(inputs["t"], n, dtype=m.dtype)
            elif name == "conv_in":
                io["x"] = inputs["sample"].to(m.dtype).permute(0, 2, 3, 1).contiguous()
            else:
                io["x"], io["temb"], io["prev_x"] = h, temb, prev_x
                if name.startswith("up_blocks") and ".resnets." in name:
                    io["skip"] = skips.pop()
            y = self.stage(name, mode, io)
            out.append((name, io, y))
            if name == "time":
                temb = y
                continue
            prev_x, h = (io["x"] if ".resnets." in name else None), y
            nxt = self.order[self.order.index(name) + 1] if name != self.order[-1] else ""
            if name == "conv_in" or ".downsamplers." in name or (
                    name.startswith("down_blocks") and ".resnets." in name and ".attentions." not in nxt) or (
                    name.startswith("down_blocks") and ".attentions." in name):
                skips.append(y)
        assert not skips
        return out


def stage_table(walker: UNetBlocks, inputs: dict) -> list:
    """Per stage of the trace on inputs: the name, io16 (the fp16-rounded inputs the kernel is fed: x, skip, temb, and
    the shared ehs / audio / bias), ref and emul on those same inputs, and both bars ((E, bar) of max|.| and of
    rel-L2, small_shape_ref.bar_of / bar_l2_of)."""
    h16 = lambda t: t.half() if torch.is_tensor(t) and t.dtype in (F32, F64) else t   # noqa: E731
    rows = []
    for name, io, _ in walker.trace(inputs):
        io16 = {k: ({a: h16(b) for a, b in v.items()} if isinstance(v, dict) else h16(v)) for k, v in io.items()}
        if io16.get("bias") is not None:
            io16["bias"] = io["bias"].float()           # the additive key bias stays fp32
        ref = walker.stage(name, "ref", io16)
        emu = walker.stage(name, "emul", io16).half()
        rows.append({"name": name, "io16": io16, "ref": ref, "emu": emu,
                     "bar": R.bar_of(emu, ref), "bar_l2": R.bar_l2_of(emu, ref)})
    return rows
