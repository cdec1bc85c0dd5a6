"""Which launches does a latent size make?  Runs unet.UNet2DConditionModel.forward_nhwc, vae.VAEDecoder and
vae.VAEEncoder on fake tensors (torch FakeTensorMode, device "cuda" without a GPU) through the fake
implementations the c2d:: custom ops register in clap2diffusion_amd/torch_ops.py, and records every c2d:: call a
TorchDispatchMode sees: the op, its tensor shapes and leading dimensions, its flags.  No layer bypasses the custom
ops, so this is the fake-tensor route, not a stub at clap2diffusion_amd.ops.  The planner queries the modules make
on the way (ops.rowring_conv, gn_moment_rows, upfold_ok, panel_gemm) are host code and run for real.

launches(h, w)        the set of launch keys at latent h x w (UNet at the CFG pair n = 2, VAE at one image)
never_made()          launches(8, 8) - launches(16, 16): what the suite's smallest latent never launched
plan_rows(keys)       for every conv / linear key: a filled c2d_conv_desc asked of c2d_conv2d_igemm_plan,
                      c2d_conv2d_igemm_workspace_size and c2d_conv2d_gn_rows
plan_table()          the planner's answers over the runs of PLAN_TABLE_RUNS and the towers' linear shapes, with the
                      launch-key digest of every run (tests/golden/conv_plan_table.json)
CPU only: nothing here touches a device.
"""
from __future__ import annotations

import ctypes
import functools
import hashlib

import torch
from torch._subclasses.fake_tensor import FakeTensorMode
from torch.utils._python_dispatch import TorchDispatchMode


def _desc(a):
    if isinstance(a, torch.Tensor):
        ld = a.stride(-2) if a.dim() >= 2 else 1
        return ("T", tuple(a.shape), int(ld))
    if isinstance(a, (bool, int, str)) or a is None:
        return a
    if isinstance(a, float):
        return round(a, 9)
    return str(a)


class Recorder(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.calls = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "_schema", None)
        if name is not None and func._schema.name.startswith("c2d::"):
            names = [x.name for x in func._schema.arguments]
            full = {x.name: x.default_value for x in func._schema.arguments if x.has_default_value()}
            full.update(zip(names, args))
            full.update(kwargs)
            self.calls.append((func._schema.name[5:], tuple((k, _desc(full.get(k))) for k in names)))
        return func(*args, **kwargs)


def _run(fn):
    rec = Recorder()
    with FakeTensorMode(allow_non_fake_inputs=True), torch.device("cuda"), torch.no_grad():
        with rec:
            fn()
    return rec.calls


def unet_calls(h: int, w: int, n: int = 2):
    from clap2diffusion_amd.unet import UNet2DConditionModel

    def go():
        m = UNet2DConditionModel()
        m.finalize()
        x = torch.empty(n, h, w, 8, dtype=torch.float16)
        t_sin = torch.empty(n, 320, dtype=torch.float16)
        ehs = torch.empty(n, 77, 768, dtype=torch.float16)
        m.forward_nhwc(x, t_sin, ehs)
    return _run(go)


def vae_calls(h: int, w: int, n: int = 1, parts=("dec", "enc")):
    from clap2diffusion_amd.vae import VAEDecoder, VAEEncoder

    def go():
        if "dec" in parts:
            dec = VAEDecoder()
            dec.decoder.mid_block.attentions[0].finalize()
            dec(torch.empty(n, 4, h, w, dtype=torch.float32))
        if "enc" in parts:
            enc = VAEEncoder()
            enc.encoder.mid_block.attentions[0].finalize()
            enc(torch.empty(n, 8 * h, 8 * w, 3, dtype=torch.uint8))
    return _run(go)


def launches(h: int, w: int) -> set:
    return set(unet_calls(h, w)) | set(vae_calls(h, w))


def never_made(small=(8, 8), covered=(16, 16)) -> list:
    return sorted(launches(*small) - launches(*covered), key=repr)


def conv_desc_of(key):
    """The c2d_conv_desc torch_ops._conv_desc fills for a recorded conv2d_igemm call, with stand-in 256-aligned
    pointers (the planner reads only whether they are set and aligned) and a workspace large enough for any split."""
    from clap2diffusion_amd import _lib
    op, items = key
    assert op == "conv2d_igemm"
    a = dict(items)
    shp = lambda k: a[k][1] if isinstance(a.get(k), tuple) else None
    xs = shp("x")
    d = _lib.ConvDesc()
    if len(xs) == 2:
        n, h, w, c0 = 1, 1, xs[0], xs[1]
    else:
        n, h, w, c0 = xs
        if a["src_pad"]:
            h, w = h - 2, w - 2
    c1 = shp("x2")[-1] if shp("x2") else 0
    ksize, stride, up, fold, pa = a["ksize"], a["stride"], a["up"], a["up_fold"], a["pad_after"]
    if ksize == 3:
        vh, vw = (2 * h, 2 * w) if up or fold else (h, w)
        oh, ow = (vh - 1) // stride + 1, (vw - 1) // stride + 1
        if pa:
            oh, ow = h // 2, w // 2
    else:
        oh, ow = h, w
    d.src0, d.c0, d.c1 = 256, c0, c1
    if c1:
        d.src1 = 256
    d.n, d.h, d.w, d.oh, d.ow, d.ksize, d.stride, d.up = n, h, w, oh, ow, ksize, stride, 2 if fold else int(up)
    d.weight, d.cout, d.kpad, d.act = 256, a["cout"], a["kpad"], a["act"]
    if a["lnf_eps"] > 0:
        d.pro, d.pro_eps = _lib.C2D_PRO_LNFOLD, a["lnf_eps"]
    elif shp("gn_scale"):
        d.pro, d.pro_silu, d.pro_a, d.pro_b = _lib.C2D_PRO_GN, int(a["gn_silu"]), 256, 256
    elif shp("ln_stats"):
        d.pro, d.pro_a, d.gamma, d.beta = _lib.C2D_PRO_LN, 256, 256, 256
    elif a["silu_in"]:
        d.pro = _lib.C2D_PRO_SILU
    if shp("bias"):
        d.bias = 256
    if shp("temb"):
        d.temb, d.temb_ld = 256, a["temb"][2]
    if shp("resid"):
        d.resid, d.resid_ld = 256, a["resid"][2]
    d.out, d.out_ld = 256, a["out"][2]
    d.src_pad = int(a["src_pad"])
    d.pad_mode = _lib.C2D_PAD_AFTER if pa else _lib.C2D_PAD_SAME
    return d


def plan_rows(keys) -> list:
    """One row per conv / linear launch: shape, flags, and what the three host queries answer."""
    from clap2diffusion_amd import _lib
    L = _lib.lib()
    rows = []
    for key in keys:
        if key[0] != "conv2d_igemm":
            continue
        d = conv_desc_of(key)
        ws = int(L.c2d_conv2d_igemm_workspace_size(ctypes.byref(d)))
        d.ws, d.ws_bytes = 256, 1 << 40
        tid, ks = ctypes.c_int(-9), ctypes.c_int(-9)
        rc = L.c2d_conv2d_igemm_plan(ctypes.byref(d), ctypes.byref(tid), ctypes.byref(ks))
        d.gn_groups = 32
        gn = int(L.c2d_conv2d_gn_rows(ctypes.byref(d))) if d.cout % 32 == 0 else 0
        rows.append({"n": d.n, "h": d.h, "w": d.w, "c0": d.c0, "c1": d.c1, "oh": d.oh, "ow": d.ow, "ksize": d.ksize,
                     "stride": d.stride, "up": d.up, "cout": d.cout, "kpad": d.kpad, "pro": d.pro, "act": d.act,
                     "temb": bool(d.temb), "resid": bool(d.resid), "out_ld": d.out_ld, "src_pad": d.src_pad,
                     "pad_mode": d.pad_mode, "rc": rc, "tile": tid.value, "split": ks.value, "ws_bytes": ws,
                     "gn_rows": gn})
    rows.sort(key=lambda r: tuple(r[k] for k in ("ksize", "n", "h", "w", "c0", "c1", "cout", "stride", "up", "pro",
                                                  "act", "temb", "resid", "out_ld", "src_pad", "pad_mode")))
    uniq = []
    for r in rows:
        if not uniq or uniq[-1] != r:
            uniq.append(r)
    return uniq


def summary(keys) -> dict:
    """Launch keys -> {op: sorted list of distinct tensor-shape signatures} for the non-conv ops."""
    out = {}
    for op, items in keys:
        if op == "conv2d_igemm":
            continue
        sig = [[k, list(v[1]), v[2]] if isinstance(v, tuple) else [k, v] for k, v in items]
        out.setdefault(op, []).append(sig)
    return {k: sorted(v, key=repr) for k, v in sorted(out.items())}


# ------------------------------------------------------------------ the plan table
# (name, calls): the runs whose conv / linear launches make the rows of tests/golden/conv_plan_table.json
PLAN_TABLE_RUNS = (
    ("unet_8x8_n2", lambda: unet_calls(8, 8, 2)),
    ("unet_16x16_n2", lambda: unet_calls(16, 16, 2)),
    ("unet_64x64_n2", lambda: unet_calls(64, 64, 2)),
    ("unet_64x64_n32", lambda: unet_calls(64, 64, 32)),
    ("unet_96x96_n16", lambda: unet_calls(96, 96, 16)),
    ("vae_8x8_n1", lambda: vae_calls(8, 8, 1)),
    ("vae_64x64_n1", lambda: vae_calls(64, 64, 1)),
    ("vae_dec_64x64_n8", lambda: vae_calls(64, 64, 8, parts=("dec",))),
)
DESC_FIELDS = ("n", "h", "w", "c0", "c1", "oh", "ow", "ksize", "stride", "up", "cout", "kpad", "pro", "act", "bias",
               "temb_ld", "resid_ld", "out_ld", "src_pad", "pad_mode")
# per variant: (rc, tile, split) of c2d_conv2d_igemm_plan without a workspace, with a large one and with one a byte
# short of the need; c2d_conv2d_igemm_workspace_size; c2d_conv2d_gn_rows at 32 groups with and without a residual
ANSWER_FIELDS = ("rc0", "tile0", "split0", "rc", "tile", "split", "rc_short", "tile_short", "split_short", "ws_bytes",
                 "gn_rows_resid", "gn_rows_plain")


def tower_linears() -> list:
    """(M, K, cout) of every HLinear of the CLIP text tower (one prompt and the CFG pair), the CLIP vision tower
    (one image, with and without the class row) and HTSAT (one clip), from the modules' own sizes."""
    from clap2diffusion_amd.htsat import HTSATEncoder
    from clap2diffusion_amd.layers import HLinear
    from clap2diffusion_amd.weights import CLIP_VISION_CFG as V
    out = []
    for m in (154, 77):   # text_encoder.TextEncoder: 77 tokens of width 768, mlp 3072
        out += [(m, 768, 2304), (m, 768, 768), (m, 768, 3072), (m, 3072, 768)]
    w, tokens = V["width"], (V["image"] // V["patch"]) ** 2
    out.append((tokens, 3 * V["patch"] ** 2, w))   # patch_embed: K = 588 -> kpad 640
    for m in (tokens + 1, tokens):
        out += [(m, w, 3 * w), (m, w, w), (m, w, V["mlp"]), (m, V["mlp"], w)]
    out.append((1, w, V["proj"]))
    with torch.device("meta"):
        enc = HTSATEncoder()
    rows = 4096   # 64 x 64 patches of a 1024-frame clip, a quarter after every merge
    out.append((rows, enc.patch_proj.in_features, enc.patch_proj.out_features))
    for i, stage in enumerate(enc.stages):
        for lin in (x for x in stage.modules() if isinstance(x, HLinear)):
            out.append((rows, lin.in_features, lin.out_features))
        if i < len(enc.merges):
            rows //= 4
            out.append((rows, enc.merges[i].reduction.in_features, enc.merges[i].reduction.out_features))
    out += [(1, enc.linear1.in_features, enc.linear1.out_features), (1, enc.linear2.in_features, enc.linear2.out_features)]
    return sorted(set(out))


def linear_desc(m: int, k: int, cout: int):
    """A plain linear (no prologue, activation, residual) of m rows as ops.conv issues it for a 2-D input."""
    from clap2diffusion_amd import _lib
    d = _lib.ConvDesc()
    d.src0, d.weight, d.bias, d.out = 256, 256, 256, 256
    d.c0, d.n, d.h, d.w, d.oh, d.ow, d.ksize, d.stride = k, 1, 1, m, 1, m, 1, 1
    d.cout, d.kpad, d.out_ld = cout, (k + 63) // 64 * 64, cout
    return d


def answers(d) -> list:
    """ANSWER_FIELDS for descriptor d under the plan override in force; d comes back as it was."""
    from clap2diffusion_amd import _lib
    L = _lib.lib()
    keep = (d.ws, d.ws_bytes, d.resid, d.resid_ld, d.gn_groups)
    d.ws, d.ws_bytes = None, 0
    need = int(L.c2d_conv2d_igemm_workspace_size(ctypes.byref(d)))
    out = []
    for ws, nbytes in ((None, 0), (256, 1 << 40), (256, max(need - 1, 0))):
        d.ws, d.ws_bytes = ws, nbytes
        tid, ks = ctypes.c_int(-9), ctypes.c_int(-9)
        out += [L.c2d_conv2d_igemm_plan(ctypes.byref(d), ctypes.byref(tid), ctypes.byref(ks)), tid.value, ks.value]
    out.append(need)
    d.ws, d.ws_bytes, d.gn_groups = 256, 1 << 40, 32
    for resid in (True, False):
        d.resid, d.resid_ld = (256, keep[3] or d.cout) if resid else (None, 0)
        out.append(int(L.c2d_conv2d_gn_rows(ctypes.byref(d))) if d.cout % 32 == 0 else 0)
    d.ws, d.ws_bytes, d.resid, d.resid_ld, d.gn_groups = keep
    return out


def launch_digest(calls) -> str:
    return hashlib.sha256(repr(sorted(set(calls), key=repr)).encode()).hexdigest()[:16]


@functools.lru_cache(maxsize=None)
def plan_table() -> dict:
    """{"runs": {name: {"launches": distinct launch keys, "digest": their hash}}, "rows": [...]}: one row per distinct
    descriptor of the runs' conv / linear launches and of tower_linears(), "d" its DESC_FIELDS, "base" its
    ANSWER_FIELDS; the 3x3 rows with c0 + c1 a multiple of 64 also "src_pad" (the answers with src_pad = 1) and
    "forced" ({"tile/split": answers} under ops.force_plan for every LDS-DMA tile and the panel GEMM, split 0 and
    2)."""
    from clap2diffusion_amd import ops
    from tests.test_kernels_gpu import DMA_TILE_IDS
    runs, descs = {}, {}
    for name, calls in PLAN_TABLE_RUNS:
        keys = set(calls())
        runs[name] = {"launches": len(keys), "digest": launch_digest(keys)}
        for key in keys:
            if key[0] == "conv2d_igemm":
                d = conv_desc_of(key)
                row = tuple(int(bool(getattr(d, f))) if f == "bias" else getattr(d, f) for f in DESC_FIELDS)
                descs.setdefault(row, d)
    for shape in tower_linears():
        d = linear_desc(*shape)
        descs.setdefault(tuple(int(bool(getattr(d, f))) if f == "bias" else getattr(d, f) for f in DESC_FIELDS), d)
    rows = []
    for key in sorted(descs):
        d = descs[key]
        row = {"d": list(key), "base": answers(d)}
        if d.ksize == 3 and (d.c0 + d.c1) % 64 == 0:
            if not d.src_pad:
                d.src_pad = 1
                row["src_pad"] = answers(d)
                d.src_pad = 0
            row["forced"] = {}
            for tile in (*DMA_TILE_IDS, 70):
                for split in (0, 2):
                    with ops.force_plan(tile, split):
                        row["forced"][f"{tile}/{split}"] = answers(d)
        rows.append(row)
    return {"desc_fields": list(DESC_FIELDS), "answer_fields": list(ANSWER_FIELDS), "runs": runs, "rows": rows}


def dump_plan_table(table: dict) -> str:
    """The golden's text: one row per line."""
    import json
    head = {k: v for k, v in table.items() if k != "rows"}
    lines = ",\n".join(json.dumps(r, separators=(",", ":")) for r in table["rows"])
    return json.dumps(head, indent=1)[:-2] + ',\n "rows": [\n' + lines + "\n ]\n}\n"


if __name__ == "__main__":
    import pathlib
    pathlib.Path(__file__).parent.joinpath("golden", "conv_plan_table.json").write_text(dump_plan_table(plan_table()))
