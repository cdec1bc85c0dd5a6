"""Shared by tests/test_htsat_gpu.py and tests/test_htsat_cpu.py: the Swin block / tower cases, the
fp16-storage emulation of the oracle that sets the tolerances, the metrics, and the tolerance constants.
CPU only: nothing here launches a kernel.

How a tolerance is made.  The HIP tower stores fp16 where the oracle keeps fp32: the block input, qkv,
the attention output, dense + residual, the GELU'd intermediate and output + residual (and, around the
blocks, the patch matrix, patch-embed output, its LayerNorm, every patch-merge reduction, the final
LayerNorm, the pooled vector and the two projection outputs).  `swin_block_q` / `tower_points` with
quant=fp16 round exactly there and nowhere else.  The distance of that emulation from the fp32 oracle,
worst of three seeds, is the CPU-emulated fp16 error E of a metric; its tolerance is 3 * E (the factor
covers what the emulation leaves out: GEMM accumulation order, __expf, the fp16 weights' rounding meeting
the LayerNorm prologue).  tests/test_htsat_cpu.py recomputes E and checks the constants below against it,
and checks that every seeded defect lands at least 4 tolerances away.
"""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn.functional as F

import oracle.htsat_ref as R
from clap2diffusion_amd.weights import HTSAT_CFG, htsat_param_shapes, synth_generic

E_ = "audio_model.audio_encoder."
BLOCK_KEY = E_ + "layers.0.blocks.0"
SEEDS = (0, 1, 2)

# (C, heads, grid, shift, batch)
BLOCK_CASES = ((96, 4, 16, 0, 2), (96, 4, 16, 4, 2), (192, 8, 16, 4, 2), (384, 16, 16, 4, 2), (768, 32, 8, 0, 2),
               (96, 4, 16, 4, 3))

# Per block case, two metrics of the block output against the fp32 oracle:
#   l2  = global rel-L2
#   win = worst rel-L2 of one 64-token window of the roll-and-partition grouping (a defect confined to one
#         window is diluted in l2)
# E = CPU-emulated fp16 error, worst of SEEDS; the tolerance is 3 * E; D = the smallest distance any
# applicable seeded defect (DEFECTS below) puts between the defective and the correct fp32 oracle over SEEDS.
# test_htsat_cpu.py recomputes E, and asserts D > 4 * tolerance (measured: D / tolerance >= 90 everywhere).
BLOCK_E = {
    #  C  heads grid shift b     E_l2      E_win        D_l2      D_win  (CPU-measured)
    (96, 4, 16, 0, 2):      (3.316e-4, 3.410e-4),   # 9.15e-2   9.28e-2
    (96, 4, 16, 4, 2):      (3.404e-4, 3.517e-4),   # 1.15e-1   1.32e-1
    (192, 8, 16, 4, 2):     (3.373e-4, 3.466e-4),   # 1.16e-1   1.40e-1
    (384, 16, 16, 4, 2):    (3.385e-4, 3.480e-4),   # 1.15e-1   1.31e-1
    (768, 32, 8, 0, 2):     (3.314e-4, 3.320e-4),   # 9.59e-2   9.63e-2
    (96, 4, 16, 4, 3):      (3.400e-4, 3.517e-4),   # 1.15e-1   1.34e-1
}
TOL_FACTOR, SEPARATION = 3.0, 4.0
BLOCK_TOL = {case: (TOL_FACTOR * e[0], TOL_FACTOR * e[1]) for case, e in BLOCK_E.items()}

# The wired tower (synth_htsat weights, batch 2).  Stage points use the per-window metric over the windows
# of the stage's last block (grid, shift) = TOWER_GRIDS; at stage 3 (one window per image) that is the
# per-image rel-L2.  Global rel-L2 does not separate at the stage points: "last window unmasked" moves
# stage 0 by 4.6e-3 globally against a tolerance of 1.4e-3, so the stage metric is per-window, where the
# same defect moves it by 3.8e-2.  The pooled vector and the embedding are compared by global rel-L2.
# E as above over weight seeds SEEDS and mel seeds T + seed.  Defect separation (every DEFECTS entry
# applied to every block of the oracle tower, T = 300): smallest distance at stage 0 / 1 / 2 is
# 2.7e-2 / 2.0e-2 / 1.09e-2 (bias dropped), >= 5 tolerances, asserted in test_htsat_cpu.py.  At stage 3
# (no shifted block, 5.2e-3 .. 1.2e-2), the pooled vector (5.4e-4 .. 5.0e-3) and the embedding the defects
# of earlier stages arrive diluted and do not separate; those tolerances rest on the emulation alone.
TOWER_GRIDS = ((64, 4), (32, 4), (16, 4), (8, 0))
TOWER_T = (1024, 300, 1001)
TOWER_POINTS = ("stage0", "stage1", "stage2", "stage3", "pooled", "embedding")
TOWER_E = {
    # T:    win stage0  win stage1  win stage2  win stage3  l2 pooled   l2 embedding   (CPU-measured)
    1024:  (4.954e-4,   5.526e-4,   6.949e-4,   6.343e-4,   1.287e-4,   3.872e-4),
    300:   (4.976e-4,   5.480e-4,   6.930e-4,   6.312e-4,   1.254e-4,   3.971e-4),
    1001:  (4.962e-4,   5.469e-4,   6.935e-4,   6.339e-4,   1.253e-4,   3.850e-4),
}
TOWER_TOL = {t: tuple(TOL_FACTOR * v for v in e) for t, e in TOWER_E.items()}
TOWER_MEL_SEED = {1024: 1024, 300: 300, 1001: 77}     # the seeds of tests/golden/htsat_ext.npz and htsat.npz


def fp16(t: torch.Tensor) -> torch.Tensor:
    return t.half().float()


def round_linear_weights(sd: dict) -> "OrderedDict[str, torch.Tensor]":
    """The state dict as the HIP modules hold it: GEMM weights fp16 (HLinear), everything else
    (biases, LayerNorm / BatchNorm parameters, relative-position table) fp32."""
    return OrderedDict((k, fp16(v) if k.endswith(".weight") and v.dim() >= 2 else v.float()) for k, v in sd.items())


def block_state_dict(c: int, heads: int, seed: int) -> "OrderedDict[str, torch.Tensor]":
    """Synthetic weights of a one-block tower of width c (block_cfg), GEMM weights rounded through fp16: the
    block lies under BLOCK_KEY, and HTSATEncoder(block_cfg(c, heads)).load_clap_state_dict takes the whole dict."""
    return round_linear_weights(synth_generic(htsat_param_shapes(block_cfg(c, heads)), seed, "htsat."))


def block_cfg(c: int, heads: int) -> dict:
    return dict(HTSAT_CFG, depths=(1,), embed=c, heads=(heads,), hidden=c)


def block_input(c: int, grid: int, b: int, seed: int) -> torch.Tensor:
    """[b, grid*grid, c] fp32 holding fp16 values: unit-scale tokens, as the patch-embed LayerNorm leaves them."""
    g = torch.Generator().manual_seed(1000 + seed)
    return fp16(torch.randn(b, grid * grid, c, generator=g))


def swin_block_q(x, sd, k, b, h, w, c, heads, shift, quant=None):
    """oracle.htsat_ref.swin_block with `quant` applied where the HIP path stores fp16 (quant None: the
    oracle's own arithmetic, op for op -- test_htsat_cpu.py asserts bit equality)."""
    q_ = quant or (lambda t: t)
    win = R.WINDOW
    if min(h, w) <= win:
        shift, win = 0, min(h, w)
    short = x = q_(x)
    y = R._ln(x, sd, k + ".layernorm_before").view(b, h, w, c)
    if shift:
        y = torch.roll(y, (-shift, -shift), (1, 2))
    y = y.view(b, h // win, win, w // win, win, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, win * win, c)
    nw = y.shape[0]
    d = c // heads
    q, kk, v = (q_(R._lin(y, sd, f"{k}.attention.self.{n}")).view(nw, -1, heads, d).transpose(1, 2)
                for n in ("query", "key", "value"))
    s = q @ kk.transpose(-1, -2) / d ** 0.5
    table = sd[k + ".attention.self.relative_position_bias_table"]
    bias = table[R.relative_position_index(win).reshape(-1)].view(win * win, win * win, heads).permute(2, 0, 1)
    s = s + bias.unsqueeze(0)
    if shift:
        m = R.shift_mask(h, w, win, shift)
        s = (s.view(b, m.shape[0], heads, win * win, win * win) + m[None, :, None]).view(nw, heads, win * win, -1)
    o = q_((s.softmax(-1) @ v).transpose(1, 2).reshape(nw, win * win, c))
    o = R._lin(o, sd, k + ".attention.output.dense")
    o = o.view(b, h // win, w // win, win, win, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, c)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    x = q_(short + o.reshape(b, h * w, c))
    m = q_(F.gelu(R._lin(R._ln(x, sd, k + ".layernorm_after"), sd, k + ".intermediate.dense")))
    return q_(x + R._lin(m, sd, k + ".output.dense"))


def tower_points(sd: dict, mel: torch.Tensor, quant=None) -> dict:
    """oracle.htsat_ref.htsat_forward rebuilt from its swin_block and patch_merge, keeping each stage's
    last block output ([b, h*w, c], "stage0".."stage3"), "pooled" and "embedding".  quant None runs the
    oracle's own functions (so a monkeypatched oracle.htsat_ref shows here); quant=fp16 rounds where the
    HIP tower stores fp16."""
    q_ = quant or (lambda t: t)
    x = mel.float()[:, 0]
    b, t, f = x.shape
    x = (x - sd[E_ + "batch_norm.running_mean"]) / torch.sqrt(sd[E_ + "batch_norm.running_var"] + 1e-5) \
        * sd[E_ + "batch_norm.weight"] + sd[E_ + "batch_norm.bias"]
    if t < 1024:
        x = F.interpolate(x[:, None], (1024, f), mode="bicubic", align_corners=True)[:, 0]
    img = q_(x.reshape(b, 4, 256, f).permute(0, 1, 3, 2).reshape(b, 1, 4 * f, 256))
    x = q_(F.conv2d(img, sd[E_ + "patch_embed.proj.weight"], sd[E_ + "patch_embed.proj.bias"], stride=4))
    x = q_(R._ln(x.flatten(2).transpose(1, 2), sd, E_ + "patch_embed.norm"))
    h = w = 64
    c = x.shape[-1]
    pts = {}
    for i, depth in enumerate(R.DEPTHS):
        for j in range(depth):
            k, shift = f"{E_}layers.{i}.blocks.{j}", 0 if j % 2 == 0 else R.WINDOW // 2
            if quant is None:
                x = R.swin_block(x, sd, k, b, h, w, c, R.HEADS[i], shift)
            else:
                x = swin_block_q(x, sd, k, b, h, w, c, R.HEADS[i], shift, quant)
        pts[f"stage{i}"] = x
        if i < len(R.DEPTHS) - 1:
            x = q_(R.patch_merge(x, sd, f"{E_}layers.{i}.downsample", b, h, w, c))
            h, w, c = h // 2, w // 2, 2 * c
    pooled = q_(R._ln(x, sd, E_ + "norm")).mean(dim=1)
    pts["pooled"] = pooled
    y = q_(F.relu(F.linear(q_(pooled), sd["audio_projection.linear1.weight"], sd["audio_projection.linear1.bias"])))
    y = q_(F.linear(y, sd["audio_projection.linear2.weight"], sd["audio_projection.linear2.bias"]))
    pts["embedding"] = F.normalize(y, dim=-1)
    return pts


def golden_mel(t: int, b: int, seed: int) -> torch.Tensor:
    """The seeded mel of scripts/make_goldens.py (seed 77 at T = 1001, the recipe of htsat_ext.npz elsewhere)."""
    return torch.randn(b, 1, t, 64, generator=torch.Generator().manual_seed(seed)) * 2.0 - 4.0


def window_rows(b: int, grid: int, shift: int) -> torch.Tensor:
    """[n_windows, 64] token rows of each window of the roll-and-partition grouping, by torch.roll itself."""
    win = min(R.WINDOW, grid)
    idx = torch.arange(b * grid * grid).view(b, grid, grid)
    if shift and grid > win:
        idx = torch.roll(idx, (-shift, -shift), (1, 2))
    return idx.view(b, grid // win, win, grid // win, win).permute(0, 1, 3, 2, 4).reshape(-1, win * win)


def block_metrics(out: torch.Tensor, ref: torch.Tensor, b: int, grid: int, shift: int) -> tuple[float, float]:
    """(global rel-L2, worst per-window rel-L2) of a block output [b*grid*grid, C] (any leading shape)."""
    out, ref = out.double().reshape(-1, ref.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    rows = window_rows(b, grid, shift)
    d, r = (out - ref)[rows], ref[rows]                      # [nw, 64, C]
    per = d.flatten(1).norm(dim=1) / r.flatten(1).norm(dim=1)
    return ((out - ref).norm() / ref.norm()).item(), per.max().item()


def tower_metrics(pts: dict, ref: dict, b: int) -> tuple:
    """The six TOWER_POINTS metrics: per-window at the stages, global rel-L2 at pooled / embedding."""
    return tuple(block_metrics(pts[f"stage{i}"], ref[f"stage{i}"], b, g, s)[1] for i, (g, s) in enumerate(TOWER_GRIDS)) \
        + (rel_l2(pts["pooled"], ref["pooled"]), rel_l2(pts["embedding"], ref["embedding"]))


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().reshape(b.shape), b.double()
    return ((a - b).norm() / b.norm()).item()


# ------------------------------------------------------------------ seeded defects
# Each entry patches oracle.htsat_ref (through pytest's monkeypatch, `mp`) into a wrong Swin block and
# returns the function to call in place of R.swin_block.  "needs_shift": a no-op on an unshifted block.
def _defect_mask_zeroed(mp):
    orig = R.shift_mask
    mp.setattr(R, "shift_mask", lambda *a: torch.zeros_like(orig(*a)))
    return R.swin_block


def _defect_last_window_unmasked(mp):
    orig = R.shift_mask

    def f(*a):
        m = orig(*a).clone()
        m[-1] = 0
        return m
    mp.setattr(R, "shift_mask", f)
    return R.swin_block


def _defect_no_roll(mp):
    mp.setattr(torch, "roll", lambda x, *a, **k: x)
    return R.swin_block


def _defect_index_transposed(mp):
    orig = R.relative_position_index
    mp.setattr(R, "relative_position_index", lambda w=R.WINDOW: orig(w).t().contiguous())
    return R.swin_block


def _defect_bias_dropped(mp):
    real_swin = R.swin_block

    def f(x, sd, k, *a):
        key = k + ".attention.self.relative_position_bias_table"
        return real_swin(x, {**sd, key: torch.zeros_like(sd[key])}, k, *a)
    return f


def _defect_mask_window_offset(mp):
    """Image 0 reads the mask of window w + 1 (a wrong `w % n_mask`); the other images are right."""
    orig, real_swin = R.shift_mask, R.swin_block

    def f(x, sd, k, b, *a):
        mp.setattr(R, "shift_mask", lambda *s: torch.roll(orig(*s), -1, 0))
        first = real_swin(x[:1], sd, k, 1, *a)
        mp.setattr(R, "shift_mask", orig)
        return torch.cat([first, real_swin(x[1:], sd, k, b - 1, *a)]) if b > 1 else first
    return f


DEFECTS = OrderedDict((
    ("mask_zeroed", (_defect_mask_zeroed, True)),
    ("last_window_unmasked", (_defect_last_window_unmasked, True)),
    ("no_roll", (_defect_no_roll, True)),
    ("index_transposed", (_defect_index_transposed, False)),
    ("bias_dropped", (_defect_bias_dropped, False)),
    ("mask_window_offset", (_defect_mask_window_offset, True)),
))


def case_id(case) -> str:
    return "C{}_h{}_g{}_s{}_b{}".format(*case)


def measure_block_case(case, seeds=SEEDS) -> tuple[float, float]:
    """CPU-emulated fp16 error of a block case: worst (global, per-window) rel-L2 of the fp16-storage
    emulation against the fp32 oracle over `seeds`."""
    c, heads, grid, shift, b = case
    worst = [0.0, 0.0]
    for s in seeds:
        sd, x = block_state_dict(c, heads, s), block_input(c, grid, b, s)
        with torch.no_grad():
            ref = R.swin_block(x, sd, BLOCK_KEY, b, grid, grid, c, heads, shift)
            emu = swin_block_q(x, sd, BLOCK_KEY, b, grid, grid, c, heads, shift, fp16)
        worst = [max(a, m) for a, m in zip(worst, block_metrics(emu, ref, b, grid, shift))]
    return worst[0], worst[1]

