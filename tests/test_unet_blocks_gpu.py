"""The HIP UNet block by block and form by form against float64 (tests/unet_block_ref.py): every stage of the real UNet
is fed the reference's own fp16-rounded inputs and held to the bars its fp16-storage emulation sets; then
Transformer2DModel, ResnetBlock2D, Downsample2D and Upsample2D standalone in each of their forms (FOLD_FF_OUT x FOLD_LN,
cfg_dup, GroupNorm moments threaded between blocks, the row-ring layout, the folded and the materialised upsample), each
asserting through the recorded plans and calls that the route it is named for ran, and that the caller's inputs are
bit-unchanged afterwards."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from clap2diffusion_amd import ops
from clap2diffusion_amd import unet as U
from clap2diffusion_amd import weights as W
from clap2diffusion_amd.layers import HConv2d, HGroupNorm, HLayerNorm, HLinear
from clap2diffusion_amd.processor import AudioAttnProcessor, AudioProcessorManager
from tests import parity_log
from tests import small_shape_ref as R
from tests import unet_block_ref as B

pytestmark = pytest.mark.gpu

F16 = torch.float16
TKEY, TLEVEL = "down_blocks.0.attentions.0", "early"    # the standalone transformer: c = 320, 8 heads, cross 768
# the smallest image pair whose rows reach BasicTransformerBlock._lnf_on at c = 320: the planner runs none of the
# three GEMMs on the panel kernel by itself below 8192 rows (asked of the library in test_lnf_shape_is_the_smallest)
LNF_SHAPE, SMALL_SHAPE = (2, 64, 64), (2, 16, 16)


def lnf_on(rows, c, cout, geglu):
    """BasicTransformerBlock._lnf_on of a finalized block at the default switches, asked of the planner."""
    stub = SimpleNamespace(lnf_folded=c in (320, 640), norm1=SimpleNamespace(c=c))
    return U.BasicTransformerBlock._lnf_on(stub, rows, cout, geglu)


def load_module(mod, sd, prefix):
    """A standalone block from the UNet's diffusers keys under prefix, as load_diffusers_state_dict loads them."""
    for name, m in mod.named_modules():
        key = f"{prefix}.{name}" if name else prefix
        if isinstance(m, U.FeedForward):
            m.load_geglu(sd[key + ".net.0.proj.weight"], sd[key + ".net.0.proj.bias"])
        elif isinstance(m, (HLinear, HConv2d, HGroupNorm, HLayerNorm)) and not name.endswith("net.0.proj"):
            m.load(sd[key + ".weight"], sd.get(key + ".bias"))
    for m in mod.modules():
        if isinstance(m, U.Attention):
            m.finalize()
    if isinstance(mod, U.Transformer2DModel):
        mod.finalize()
    return mod


def audio_processor(procs, level, dev):
    p = AudioAttnProcessor(level)
    p.load_state_dict(procs[level])
    return p.to(dev).eval()


@pytest.fixture(scope="module")
def net(dev):
    """The HIP UNet with its audio processors, and the walker, over the same seeded weights; 'cache' holds the float64
    tables, computed once by the test that first asks and left unchanged."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = W.synth_unet(0)
    procs = {lv: W.synth_processor_weights(lv, 0) for lv in B.LEVELS}
    hip = U.UNet2DConditionModel().to(dev)
    hip.load_diffusers_state_dict(sd)
    mgr = AudioProcessorManager(hip)
    mgr.setup_processors(verbose=False)
    for level, p in mgr.level_processors().items():
        p.load_state_dict(procs[level])
        p.to(dev).eval()
    return SimpleNamespace(sd=sd, procs=procs, hip=hip, wk=B.UNetBlocks(sd, procs, lnf_on=lnf_on), cache={})


@pytest.fixture
def tables(net, progress):
    def get(case):
        if case not in net.cache:
            n, h, w, keep = case
            progress(f"float64 stage table {n}x{h}x{w}")
            net.cache[case] = B.stage_table(net.wk, B.inputs_of(n, h, w, keep))
            progress("table done")
        return net.cache[case]
    return get


def row_of(wk, name, io16, **kw):
    """ref, emul and the two bars of one standalone block on fp16 inputs."""
    ref = wk.stage(name, "ref", io16, **kw)
    emu = wk.stage(name, "emul", io16, **kw).half()
    return {"name": name, "ref": ref, "emu": emu, "bar": R.bar_of(emu, ref), "bar_l2": R.bar_l2_of(emu, ref)}


def judge(tag, name, out, row, plans, failures):
    """One line and one parity_log row per stage or form; a miss is collected, so a run names every one that fails."""
    ref = row["ref"]
    (e, bar), (e2, bar2) = row["bar"], row["bar_l2"]
    o = out.float().cpu()
    c = ref.shape[-1]
    finite = bool(torch.isfinite(o).all())
    pad_zero = bool((o[..., c:] == 0).all())
    shape_ok = tuple(o.shape[:-1]) == tuple(ref.shape[:-1])
    err, l2 = (R.max_err(o[..., :c], ref), R.rel_l2(o[..., :c], ref)) if shape_ok else (float("inf"), float("inf"))
    plan = ",".join(f"{t}/{k}" for t, k in plans)
    parity_log.record(stage=f"{tag}:{name}", max_abs=err, emul_E=e, bar=bar, rel_l2=l2, emul_E_l2=e2, tol_l2=bar2, plans=plan)
    print(f"UNETBLOCK {tag} {name} E={e:.3e} gpu={err:.3e} bar={bar:.3e} | rel-L2 E={e2:.3e} gpu={l2:.3e} bar={bar2:.3e} "
          f"| plans {plan}")
    if not (finite and pad_zero and shape_ok and err <= bar and l2 <= bar2):
        failures.append(f"{tag} {name}: finite {finite}, pad channels zero {pad_zero}, shape {tuple(o.shape)}, max|out - ref| "
                        f"{err:.3e} (bar {bar:.3e}, E {e:.3e}), rel-L2 {l2:.3e} (bar {bar2:.3e}, E {e2:.3e}), plans {plan}")


def dev_io(io16, dev):
    """The fp16 inputs of a row on the device, with the clones the bit-unchanged check compares against."""
    d = {k: io16[k].contiguous().to(dev) for k in ("x", "skip", "temb") if io16.get(k) is not None}
    return d, {k: v.clone() for k, v in d.items()}


def context_args(io16, dev):
    """ehs, cross_attention_kwargs and the additive key bias as forward_nhwc hands them to a transformer."""
    kw = {"audio": {k: v.contiguous().to(dev) for k, v in io16["audio"].items()}} if io16.get("audio") else {}
    bias = io16.get("bias")
    return io16["ehs"].contiguous().to(dev), kw, None if bias is None else bias.reshape(bias.shape[0], 1, 77).to(dev)


def unchanged(tag, d, keep, failures):
    for k in ("x", "skip"):
        if k in d and not torch.equal(d[k], keep[k]):
            failures.append(f"{tag}: the caller's {k} was written")


def run_stage(hip, name, io16, dev, failures):
    d, keep = dev_io(io16, dev)
    if name == "time":
        out = hip.time_conditioning(d["x"])
    elif name == "conv_in":
        out = hip.conv_in(F.pad(d["x"], (0, hip.in_pad - 4)).contiguous())
    elif name == "conv_norm_out+conv_out":
        out = hip.conv_out(hip.conv_norm_out.apply(d["x"], silu=True))
    elif ".resnets." in name:
        out = hip.get_submodule(name)(d["x"], d["temb"], skip=d.get("skip"))
    elif ".attentions." in name:
        out = hip.get_submodule(name)(d["x"], *context_args(io16, dev))
    else:
        out = hip.get_submodule(name)(d["x"])
    torch.cuda.synchronize()
    unchanged(name, d, keep, failures)
    return out


# ------------------------------------------------------------------ a. stage by stage
@pytest.mark.parametrize("case", B.CASES, ids=["x".join(map(str, c[:3])) for c in B.CASES])
def test_stage_by_stage(dev, net, tables, case):
    table = tables(case)
    tag = "x".join(map(str, case[:3]))
    assert [r["name"] for r in table] == net.hip.execution_order()
    failures = []
    with torch.no_grad():
        for row in table:
            with ops.record_conv_plans() as plans:
                out = run_stage(net.hip, row["name"], row["io16"], dev, failures)
            judge(tag, row["name"], out, row, plans, failures)
    assert not failures, "\n".join(failures)


def test_timestep_sinusoid(dev):
    """c2d::timestep_embedding's fp16 rows against the float64 sinusoid: bar_of with the fp32 sinusoid as emulation."""
    for t in (1.0, 601.0, 981.0):
        ref = B.sinusoid(t, 3)
        emu = B.sinusoid(t, 3, dtype=torch.float32).half()
        e, bar = R.bar_of(emu, ref)
        out = ops.timestep_embedding(torch.tensor([t], device=dev), None, 3, 320)
        err = R.max_err(out, ref)
        parity_log.record(stage=f"sinusoid t={t}", max_abs=err, emul_E=e, bar=bar)
        print(f"UNETBLOCK sinusoid t={t} E={e:.3e} gpu={err:.3e} bar={bar:.3e}")
        assert tuple(out.shape) == (3, 320) and err <= bar, (t, err, bar)


# ------------------------------------------------------------------ b. Transformer2DModel, form by form
class Spy:
    """Counts the calls a form is named for: ops.conv with a folded LayerNorm, the two-source K = 5C GEMM, and the
    materialised LayerNorms."""

    def __init__(self, monkeypatch):
        self.lnfold = self.two_source = self.layer_norm = 0
        conv, ln = ops.conv, ops.layer_norm

        def conv_spy(x, weight, kpad, cout, **kw):
            self.lnfold += bool(kw.get("ln_fold"))
            self.two_source += kw.get("x2") is not None and kw.get("ksize") == 1 and kpad == ops.kpad_of(5 * cout)
            return conv(x, weight, kpad, cout, **kw)

        def ln_spy(*a, **kw):
            self.layer_norm += 1
            return ln(*a, **kw)
        monkeypatch.setattr(ops, "conv", conv_spy)
        monkeypatch.setattr(ops, "layer_norm", ln_spy)


def transformer_io(net, shape, seed, pair=False):
    """fp16 inputs of the standalone transformer at (n, h, w): x, and the context of 2 (pair: 2 n) images."""
    n, h, w = shape
    nctx = 2 * n if pair else n
    inp = B.inputs_of(nctx, h, w, keep=(9, 30) + (77,) * (nctx - 2) if nctx >= 2 else None, seed=seed)
    io = net.wk.context(inp)
    io16 = {"ehs": io["ehs"].half(), "audio": {k: v.half() for k, v in io["audio"].items()}, "bias": io["bias"]}
    io16["x"] = R.gen(n, h, w, 320, seed=seed + 31).half()
    return io16


def test_lnf_shape_is_the_smallest(net):
    """Where the folded-LayerNorm forms run: the planner takes them at LNF_SHAPE and at no image pair below it."""
    n, h, w = LNF_SHAPE
    for cout, geglu in ((960, False), (320, False), (2560, True)):
        assert lnf_on(n * h * w, 320, cout, geglu)
        for hh, ww in ((16, 16), (32, 32), (32, 64), (48, 64)):
            assert not lnf_on(2 * hh * ww, 320, cout, geglu), (hh, ww, cout)


@pytest.mark.parametrize("fold_ln", [True, False], ids=["lnfold", "ln"])
@pytest.mark.parametrize("fold_ff", [True, False], ids=["ff5c", "ff2gemm"])
@pytest.mark.parametrize("shape", [SMALL_SHAPE, LNF_SHAPE], ids=["2x16x16", "2x64x64"])
def test_transformer_forms(dev, net, progress, monkeypatch, shape, fold_ff, fold_ln):
    """FOLD_FF_OUT x FOLD_LN, each against the same float64 row inside the same bar (the default form's emulation), at a
    shape below the LayerNorm fold and at the smallest one the planner folds at."""
    monkeypatch.setattr(U, "FOLD_LN", fold_ln)
    monkeypatch.setattr(U, "FOLD_FF_OUT", fold_ff)
    key = ("transformer", shape)
    if key not in net.cache:
        progress(f"float64 transformer row {shape}")
        io16 = transformer_io(net, shape, seed=3)
        net.cache[key] = (io16, row_of(net.wk, TKEY, io16))
        progress("row done")
    io16, row = net.cache[key]
    mod = load_module(U.Transformer2DModel(320, 8, 768).to(dev), net.sd, TKEY)
    mod.transformer_blocks[0].attn2.set_processor(audio_processor(net.procs, TLEVEL, dev))
    assert mod.transformer_blocks[0].lnf_folded == fold_ln
    spy = Spy(monkeypatch)
    d, keep = dev_io(io16, dev)
    failures = []
    with torch.no_grad(), ops.record_conv_plans() as plans:
        out = mod(d["x"], *context_args(io16, dev))
        torch.cuda.synchronize()
    folds = shape == LNF_SHAPE and fold_ln
    assert (spy.lnfold, spy.layer_norm) == ((3, 0) if folds else (0, 3)), (spy.lnfold, spy.layer_norm)
    assert spy.two_source == int(fold_ff)
    assert (70 in {t for t, _ in plans}) or not folds, plans
    unchanged("transformer", d, keep, failures)
    judge(f"transformer {'x'.join(map(str, shape))} ff_fold={int(fold_ff)} ln_fold={int(fold_ln)}", TKEY, out, row, plans, failures)
    assert not failures, "\n".join(failures)


def test_transformer_cfg_dup(dev, net):
    """The forward on the first half of a pair buffer against the reference of the duplicated input with the pair's
    two contexts; the buffer's second half is the copy of x the code promises."""
    io16 = transformer_io(net, (1, 16, 16), seed=5, pair=True)
    row = row_of(net.wk, TKEY, io16)
    mod = load_module(U.Transformer2DModel(320, 8, 768).to(dev), net.sd, TKEY)
    mod.transformer_blocks[0].attn2.set_processor(audio_processor(net.procs, TLEVEL, dev))
    x = io16["x"].to(dev)
    buf = torch.full((2, 16, 16, 320), float("nan"), dtype=F16, device=dev)
    buf[:1].copy_(x)
    failures = []
    with torch.no_grad(), ops.record_conv_plans() as plans:
        out = mod(buf[:1], *context_args(io16, dev), cfg_dup=buf)
        torch.cuda.synchronize()
    assert tuple(out.shape) == (2, 16, 16, 320)
    assert torch.equal(buf[:1], x), "the caller's x was written"
    assert torch.equal(buf[1:], buf[:1]), "cfg_dup[n:] is not the copy of cfg_dup[:n]"
    judge("transformer cfg_dup 1x16x16", TKEY, out, row, plans, failures)
    assert not failures, "\n".join(failures)


def gn_row(x16, norm, silu):
    """float64 GroupNorm of an fp16 tensor with a HIP norm's parameters, and its bar."""
    g, b = norm.weight.float().cpu(), norm.bias.float().cpu()
    ref = R.gn_ref(x16, g, b, norm.num_groups, norm.eps, silu)
    emu = R.gn_emul(x16, g, b, norm.num_groups, norm.eps, silu)
    return {"ref": ref, "emu": emu, "bar": R.bar_of(emu, ref), "bar_l2": R.bar_l2_of(emu, ref)}


def test_transformer_moments_in_and_out(dev, net):
    """x_mom from the resnet that produced x, want_mom=True: the output against float64 on the fp16 x, and the next
    norm applied through the moments the K = 5C GEMM emitted against float64 GroupNorm of the fp16 output."""
    rkey = "down_blocks.0.resnets.0"
    res = load_module(U.ResnetBlock2D(320, 320).to(dev), net.sd, rkey)
    res.temb_off = 0
    mod = load_module(U.Transformer2DModel(320, 8, 768).to(dev), net.sd, TKEY)
    mod.transformer_blocks[0].attn2.set_processor(audio_processor(net.procs, TLEVEL, dev))
    io16 = transformer_io(net, SMALL_SHAPE, seed=7)
    temb = (R.gen(2, 320, seed=8) * 0.5).half().to(dev)
    failures = []
    with torch.no_grad(), ops.record_conv_plans() as plans:
        x, xm = res(io16["x"].to(dev), temb, want_mom=True)
        assert xm is not None, "the resnet's conv2 emitted no moments at a shape c2d_conv2d_gn_rows takes"
        keep = x.clone()
        out, om = mod(x, *context_args(io16, dev), x_mom=xm, want_mom=True)
        torch.cuda.synchronize()
    assert torch.equal(x, keep), "the caller's x was written"
    judge("transformer x_mom want_mom", TKEY, out, row_of(net.wk, TKEY, dict(io16, x=x.cpu())), plans, failures)
    assert om is not None, "the K = 5C GEMM emitted no moments"
    nxt = net.hip.get_submodule("down_blocks.0.resnets.1").norm1
    with torch.no_grad():
        a = nxt.apply(out, silu=True, mom=om)
        torch.cuda.synchronize()
    judge("transformer next norm from moments", "down_blocks.0.resnets.1.norm1", a, gn_row(out.cpu(), nxt, True), [], failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ c. ResnetBlock2D, form by form
# name -> (key, c of x, c of skip, cout, the smallest (n, h, w) where ops.rowring_conv takes conv1 and conv2, its tile)
RESNETS = {"320-320": ("down_blocks.0.resnets.0", 320, 0, 320, (12, 64, 16), 44),
           "320-640": ("down_blocks.1.resnets.0", 320, 0, 640, (1, 64, 32), 43),
           "640+320-640": ("up_blocks.2.resnets.2", 640, 320, 640, (1, 64, 32), 43)}


def resnet_io(cx, cs, cout, shape, seed):
    n, h, w = shape
    io16 = {"x": R.gen(n, h, w, cx, seed=seed).half(), "temb": (R.gen(n, cout, seed=seed + 1) * 0.5).half()}
    if cs:
        io16["skip"] = R.gen(n, h, w, cs, seed=seed + 2).half()
    return io16


def resnet_row(net, key, io16):
    """The walker's resnet on a standalone temb [n, cout] (column offset 0)."""
    out = {}
    for mode in ("ref", "emul"):
        m = net.wk.modes[mode]
        c = lambda t: None if t is None else t.to(m.dtype)   # noqa: E731
        out[mode] = B.resnet(m, key, c(io16["x"]), c(io16["temb"]), c(io16.get("skip")))
    ref, emu = out["ref"], out["emul"].half()
    return {"name": key, "ref": ref, "emu": emu, "bar": R.bar_of(emu, ref), "bar_l2": R.bar_l2_of(emu, ref)}


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "stats"])
@pytest.mark.parametrize("ring", [False, True], ids=["plain", "rowring"])
@pytest.mark.parametrize("which", list(RESNETS))
def test_resnet_forms(dev, net, progress, monkeypatch, which, ring, moments):
    key, cx, cs, cout, ring_shape, tile = RESNETS[which]
    shape = ring_shape if ring else SMALL_SHAPE
    n, h, w = shape
    assert ops.rowring_conv(n, h, w, cx + cs, cout) == ring and ops.rowring_conv(n, h, w, cout, cout) == ring
    monkeypatch.setattr(U, "GN_MOMENTS", moments)
    ck = ("resnet", which, ring)
    if ck not in net.cache:
        progress(f"float64 resnet row {which} {shape}")
        io16 = resnet_io(cx, cs, cout, shape, seed=40 + len(which))
        net.cache[ck] = (io16, resnet_row(net, key, io16))
        progress("row done")
    io16, row = net.cache[ck]
    mod = load_module(U.ResnetBlock2D(cx + cs, cout).to(dev), net.sd, key)
    mod.temb_off = 0
    d, keep = dev_io(io16, dev)
    failures = []
    with torch.no_grad(), ops.record_conv_plans() as plans:
        out, om = mod(d["x"], d["temb"], skip=d.get("skip"), want_mom=True)
        torch.cuda.synchronize()
    tiles = [t for t, _ in plans]
    assert len(plans) == 2 + (cx + cs != cout)
    if ring:
        assert tiles.count(tile) == 2 and set(tiles) & set(ops.ROWRING_TILES) == {tile}, plans
    else:
        assert not set(tiles) & set(ops.ROWRING_TILES), plans
    assert moments or om is None
    unchanged(which, d, keep, failures)
    judge(f"resnet {which} {'x'.join(map(str, shape))} gn_moments={int(moments)}", key, out, row, plans, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("first", ["resnet", "downsample"])
def test_moments_threaded_through_a_chain(dev, net, monkeypatch, first):
    """resnet -> resnet and downsample -> resnet with x_mom / want_mom threaded and the second block writing into the
    caller's buffer: the second block against float64 on the fp16 tensor it was fed, and against the same call with
    GN_MOMENTS off.  Both forms compute one function of one fp16 input and differ only in where the moments come from
    (the conv's fp32 accumulators, or the rounded tensor the emulation also uses), so their difference is held to the
    stage's bar as well.  A moments tensor that describes another tensor fails both."""
    if first == "resnet":
        k1, k2, cout, shape = "down_blocks.0.resnets.0", "down_blocks.0.resnets.1", 320, SMALL_SHAPE
        a = load_module(U.ResnetBlock2D(320, 320).to(dev), net.sd, k1)
        a.temb_off = 0
    else:
        k1, k2, cout, shape = "down_blocks.0.downsamplers.0", "down_blocks.1.resnets.0", 640, (2, 32, 32)
        a = load_module(U.Downsample2D(320).to(dev), net.sd, k1)
    b = load_module(U.ResnetBlock2D(320, cout).to(dev), net.sd, k2)
    b.temb_off = 0
    n = shape[0]
    x0 = R.gen(*shape, 320, seed=61).half().to(dev)
    t1, t2 = ((R.gen(n, c, seed=s) * 0.5).half().to(dev) for c, s in ((320, 62), (cout, 63)))
    failures = []
    with torch.no_grad(), ops.record_conv_plans() as plans:
        y1, m1 = a(x0, t1, want_mom=True) if first == "resnet" else a(x0, want_mom=True)
        assert m1 is not None, f"the {first} emitted no moments at a shape c2d_conv2d_gn_rows takes"
        keep = y1.clone()
        buf = torch.full((*y1.shape[:-1], cout), float("nan"), dtype=F16, device=dev)
        y2, m2 = b(y1, t2, x_mom=m1, want_mom=True, out=buf)
        torch.cuda.synchronize()
        assert y2.data_ptr() == buf.data_ptr() and m2 is not None
        monkeypatch.setattr(U, "GN_MOMENTS", False)
        y2_off, m2_off = b(y1, t2, want_mom=True)
        torch.cuda.synchronize()
    assert m2_off is None and torch.equal(y1, keep), "the caller's x was written"
    row = resnet_row(net, k2, {"x": y1.cpu(), "temb": t2.cpu()})
    judge(f"chain {first}->resnet moments", k2, y2, row, plans, failures)
    judge(f"chain {first}->resnet stats", k2, y2_off, row, [], failures)
    diff = (y2.float() - y2_off.float()).abs().max().item()
    print(f"UNETBLOCK chain {first}->resnet moments vs stats max {diff:.3e} bar {row['bar'][1]:.3e}")
    if diff > row["bar"][1]:
        failures.append(f"chain {first}->resnet: GN_MOMENTS on vs off differ by {diff:.3e} > bar {row['bar'][1]:.3e}")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ d. Downsample2D / Upsample2D
@pytest.mark.parametrize("key,c,shape", [("down_blocks.0.downsamplers.0", 320, (2, 16, 16)),
                                         ("down_blocks.2.downsamplers.0", 1280, (2, 4, 4))], ids=["level0", "level2"])
def test_downsample(dev, net, key, c, shape):
    io16 = {"x": R.gen(*shape, c, seed=71).half()}
    row = row_of(net.wk, key, io16)
    mod = load_module(U.Downsample2D(c).to(dev), net.sd, key)
    d, keep = dev_io(io16, dev)
    failures = []
    with torch.no_grad(), ops.record_conv_plans() as plans:
        out = mod(d["x"])
        torch.cuda.synchronize()
    assert tuple(out.shape) == (shape[0], shape[1] // 2, shape[2] // 2, c)
    unchanged(key, d, keep, failures)
    judge(f"downsample {'x'.join(map(str, shape))}", key, out, row, plans, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("form", ["folded", "refused"])
@pytest.mark.parametrize("key,c,shape", [("up_blocks.2.upsamplers.0", 640, (2, 8, 8)),
                                         ("up_blocks.0.upsamplers.0", 1280, (2, 2, 2))], ids=["to_level0", "to_level2"])
def test_upsample_forms(dev, net, monkeypatch, key, c, shape, form):
    """Upsample2D where ops.upfold_ok takes the shape (the UNet's own widths and weights), and at 96 channels, which the
    library refuses (cin % 64 != 0), so the x2 tensor is materialised; the same float64 reference rule for both."""
    n, h, w = shape
    calls = {"folded": 0, "materialised": 0}
    up2x = ops.upsample_nearest2x
    monkeypatch.setattr(ops, "upsample_nearest2x", lambda *a, **k: (calls.__setitem__("materialised", calls["materialised"] + 1),
                                                                    up2x(*a, **k))[1])
    if form == "folded":
        sd, pre = net.sd, key
    else:
        c, pre = 96, "up"
        sd = {"up.conv.weight": R.gen(c, c, 3, 3, seed=81, scale=(27 * c) ** -0.5), "up.conv.bias": R.gen(c, seed=82) * 0.02}
    assert ops.upfold_ok(n, h, w, c, c) == (form == "folded")
    io16 = {"x": R.gen(n, h, w, c, seed=83).half()}
    if form == "folded":
        ref, emu = net.wk.stage(pre, "ref", io16), net.wk.stage(pre, "emul", io16).half()
    else:      # the walker's upsample on the two keys drawn here, the emulation in the materialised form
        ref = B.upsample(B._Mode(sd, {}, torch.float64, True, False), "up.conv", io16["x"].double())
        emu = B.upsample(B._Mode(sd, {}, torch.float32, True, True), "up.conv", io16["x"].float(), folded=False).half()
    row = {"ref": ref, "emu": emu, "bar": R.bar_of(emu, ref), "bar_l2": R.bar_l2_of(emu, ref)}
    mod = load_module(U.Upsample2D(c).to(dev), sd, pre)
    fold = mod.conv.forward_folded
    monkeypatch.setattr(mod.conv, "forward_folded", lambda x: (calls.__setitem__("folded", calls["folded"] + 1), fold(x))[1])
    d, keep = dev_io(io16, dev)
    failures = []
    with torch.no_grad(), ops.record_conv_plans() as plans:
        out = mod(d["x"])
        torch.cuda.synchronize()
    assert calls == ({"folded": 1, "materialised": 0} if form == "folded" else {"folded": 0, "materialised": 1}), calls
    assert tuple(out.shape) == (n, 2 * h, 2 * w, c) and len(plans) == 1
    unchanged(key, d, keep, failures)
    judge(f"upsample {form} {'x'.join(map(str, shape))} c={c}", key, out, row, plans, failures)
    assert not failures, "\n".join(failures)
