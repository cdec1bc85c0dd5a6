"""tests/unet_block_ref.py checked without a GPU: the float64 walker is the same network as oracle/unet_ref.py block by
block and end to end, its stage list is UNet2DConditionModel's execution order, no stage's bar sits at a cap, every
stage's emulation lies inside its bar, and every seeded defect leaves the bar of a stage it touches."""
from types import SimpleNamespace

import pytest
import torch

from clap2diffusion_amd import unet as U
from clap2diffusion_amd import weights as W
from oracle.unet_ref import UNetRef
from tests import small_shape_ref as R
from tests import unet_block_ref as B

# the stages the defects are seeded in: one resnet / transformer per level and direction (a defect costs one more
# float64 run of the stage); the bars of all 47 stages are checked
DEFECT_STAGES = ("down_blocks.0.resnets.0", "down_blocks.0.attentions.0", "down_blocks.1.resnets.0",
                 "down_blocks.2.attentions.1", "mid_block.resnets.0", "mid_block.attentions.0", "up_blocks.0.resnets.2",
                 "up_blocks.1.attentions.0", "up_blocks.2.resnets.2", "up_blocks.3.resnets.0", "up_blocks.3.attentions.2")
HELD = {"tembshift", "catswap", "gegluswap", "noresid", "audiolevel", "maskattn1", "mominput", "cfgstale"}


def lnf_on(rows, c, cout, geglu):
    """BasicTransformerBlock._lnf_on of a finalized block at the default switches, asked of the planner."""
    stub = SimpleNamespace(lnf_folded=c in (320, 640) and U.FOLD_LN, norm1=SimpleNamespace(c=c))
    return U.BasicTransformerBlock._lnf_on(stub, rows, cout, geglu)


@pytest.fixture(scope="module")
def net():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = W.synth_unet(0)
    procs = {lv: W.synth_processor_weights(lv, 0) for lv in B.LEVELS}
    return sd, procs, B.UNetBlocks(sd, procs, lnf_on=lnf_on)


def test_stage_list_is_the_execution_order(net):
    _, _, wk = net
    with torch.device("meta"):
        hip = U.UNet2DConditionModel()
    names = wk.names()
    assert names == hip.execution_order()
    assert len(names) == 47 and len(set(names)) == 47
    offs = {n[:-len(".conv1")]: m for n, m in hip.named_modules() if n.endswith(".conv1")}
    assert sorted(offs) == sorted(wk.resnets)
    for r in wk.resnets:
        assert hip.get_submodule(r).temb_off == wk.temb_off[r], r
    assert hip.temb_total == wk.temb_total


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def test_blocks_are_the_oracle(net):
    """The walker's resnet, attention and transformer against UNetRef's on the same weights.  The bound is 10 x the
    larger fp32-against-float64 self-difference of the two (UNetRef runs in float64 once its weights are doubled,
    except audio_context and __call__, which cast to fp32).  Observed rel-L2 (walker fp32 vs oracle fp32 | self-
    differences walker, oracle): resnet with shortcut 2.9e-7 | 3.5e-7, 3.3e-7; up-block resnet 4.1e-7 | 3.7e-7,
    3.6e-7; attention with a key bias 6.8e-8 | 4.6e-7, 4.6e-7; transformer with audio and mask 1.2e-7 | 1.5e-7,
    (walker only)."""
    sd, procs, wk = net
    o32 = UNetRef(sd, processors=procs)
    o64 = UNetRef(sd, processors=procs)
    o64.sd = {k: v.double() for k, v in sd.items()}
    inp = B.inputs_of(2, 16, 16, keep=(9, 30))
    ctx = wk.context(inp)
    g = torch.Generator().manual_seed(5)
    temb = torch.randn(2, 1280, generator=g)

    def temb_all(name, mode):
        m = wk.modes[mode]
        t = temb.to(m.dtype)
        row = B._lin(m, name + ".time_emb_proj", t * torch.sigmoid(t))
        full = torch.zeros(2, wk.temb_total, dtype=m.dtype)
        full[:, wk.temb_off[name]:wk.temb_off[name] + row.shape[1]] = row
        return full

    def check(tag, w32, w64, r32, r64):
        dw, do = R.rel_l2(w32, w64), (R.rel_l2(r32, r64) if r64 is not None else 0.0)
        got = R.rel_l2(w32, r32.double())
        print(f"UNETBLOCK oracle {tag}: walker32 vs oracle32 {got:.3e}; self-difference walker {dw:.3e} oracle {do:.3e}")
        assert got <= 10.0 * max(dw, do), (tag, got, dw, do)

    for name, c_in, c_skip in (("down_blocks.1.resnets.0", 320, 0), ("up_blocks.2.resnets.2", 640, 320)):
        x, skip = torch.randn(2, 16, 16, c_in, generator=g), (torch.randn(2, 16, 16, c_skip, generator=g) if c_skip else None)
        outs = {md: wk.stage(name, md, {"x": x, "skip": skip, "temb": temb_all(name, md)}) for md in ("trace32", "trace")}
        xc = nchw(x if skip is None else torch.cat([x, skip], -1))
        check(name, outs["trace32"], outs["trace"], o32.resnet(name, xc, temb).permute(0, 2, 3, 1),
              o64.resnet(name, xc.double(), temb.double()).permute(0, 2, 3, 1))
    name = "down_blocks.0.attentions.0"
    x = torch.randn(2, 16, 16, 320, generator=g)
    blk = name + ".transformer_blocks.0.attn2"
    tok, kv = x.view(2, 256, 320), inp["ehs"]

    def own_attention(mode):
        m = wk.modes[mode]
        q, k, v = (t.to(m.dtype) @ m.w(f"{blk}.{p}").t() for t, p in ((tok, "to_q"), (kv, "to_k"), (kv, "to_v")))
        return B._attend(m, q, k, v, 2, 256, 77, ctx["bias"]) @ m.w(blk + ".to_out.0").t() + m.b(blk + ".to_out.0")
    check("attention", own_attention("trace32"), own_attention("trace"), o32.attention(blk, tok, kv, ctx["bias"]),
          o64.attention(blk, tok.double(), kv.double(), ctx["bias"].double()))
    outs = {md: wk.stage(name, md, dict(ctx, x=x)) for md in ("trace32", "trace")}
    check(name, outs["trace32"], outs["trace"],
          o32.transformer(name, nchw(x), inp["ehs"], inp["audio"], ctx["bias"]).permute(0, 2, 3, 1), None)


def test_chained_walk_is_the_oracle(net):
    """The whole UNet at n = 2, 16 x 16 with audio and an encoder mask: the walker's chained fp32 trace against
    UNetRef.__call__ (fp32 only), within 10 x the walker's own fp32-against-float64 difference.  Observed: walker32 vs
    oracle 2.6e-6, walker32 vs walker64 1.2e-6 (bound 1.2e-5); walker64 vs oracle 2.5e-6."""
    sd, procs, wk = net
    inp = B.inputs_of(2, 16, 16, keep=(9, 30))
    w32 = wk.trace(inp, "trace32")[-1][2]
    w64 = wk.trace(inp, "trace")[-1][2]
    ref = UNetRef(sd, processors=procs)(inp["sample"], inp["t"], inp["ehs"], inp["audio"], encoder_attention_mask=inp["keep"])
    ref = ref.permute(0, 2, 3, 1)
    dw, got = R.rel_l2(w32, w64), R.rel_l2(w32, ref.double())
    print(f"UNETBLOCK oracle whole: walker32 vs oracle32 {got:.3e}; walker32 vs walker64 {dw:.3e}; "
          f"walker64 vs oracle32 {R.rel_l2(ref, w64):.3e}")
    assert got <= 10.0 * dw, (got, dw)


@pytest.mark.parametrize("case", B.CASES, ids=["x".join(map(str, c[:3])) for c in B.CASES])
def test_bars_hold_the_emulation_and_reject_the_defects(net, case):
    """Per stage: finite, the emulation within bar_of / bar_l2_of, neither cap binding, no stage missing.  Each defect
    is seeded in DEFECT_STAGES; one row per (stage, defect) is printed and each defect of HELD has to leave the bar of at
    least one stage.  'gneps' (the transformer's GroupNorm eps 1e-5 for 1e-6) is printed only: fp16 storage cannot
    resolve it (test_gn_eps_1e5_is_below_fp16)."""
    _, _, wk = net
    n, h, w, keep = case
    table = B.stage_table(wk, B.inputs_of(n, h, w, keep))
    assert [r["name"] for r in table] == wk.names()
    worst = {}
    for row in table:
        name, ref = row["name"], row["ref"]
        (e, bar), (e2, bar2) = row["bar"], row["bar_l2"]
        assert torch.isfinite(ref).all() and torch.isfinite(row["emu"].float()).all(), name
        assert e <= bar and e2 <= bar2, (name, e, bar, e2, bar2)
        top = ref.abs().max().item()
        assert bar < R.CAP_MAX * top and bar2 < R.CAP_L2, f"{name}: a cap binds"
        assert min(ref.shape[1:3]) > 1 or name == "time", f"{name}: a 1 x 1 image"
        line = f"UNETBLOCK {n}x{h}x{w} {name} E={e:.3e} bar={bar:.3e} | rel-L2 E={e2:.3e} bar={bar2:.3e}"
        for d in (wk.defects(name, row["io16"]) if name in DEFECT_STAGES else []):
            bad = wk.stage(name, "ref", row["io16"], defect=d)
            over = max(R.max_err(bad, ref) / bar, R.rel_l2(bad, ref) / bar2)
            line += f" | {d} {over:.2f}x"
            worst[d] = max(worst.get(d, 0.0), over)
        print(line)
    want = HELD - {"cfgstale"} - (set() if keep else {"maskattn1"})
    assert set(worst) == want | {"gneps"}
    hidden = {d: v for d, v in worst.items() if d in HELD and v <= 1.0}
    assert not hidden, f"defects inside every bar they touch: {hidden}"


def test_cfg_dup_and_its_stale_copy(net):
    """A CFG pair through one transformer: x once, the pair's two contexts -> the reference of the duplicated input;
    the second half taken before the self-attention instead of after it leaves the bar."""
    _, _, wk = net
    name = "down_blocks.0.attentions.0"
    inp = B.inputs_of(2, 16, 16)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 16, 16, 320, generator=g).half()
    io = dict(wk.context(inp), x=x)
    io["ehs"], io["audio"] = io["ehs"].half(), {k: v.half() for k, v in io["audio"].items()}
    ref = wk.stage(name, "ref", io)
    full = wk.stage(name, "ref", dict(io, x=torch.cat([x, x], 0)))
    assert ref.shape[0] == 2 and torch.equal(ref, full)
    emu = wk.stage(name, "emul", io).half()
    (e, bar), (e2, bar2) = R.bar_of(emu, ref), R.bar_l2_of(emu, ref)
    bad = wk.stage(name, "ref", io, defect="cfgstale")
    assert torch.equal(bad[:1], ref[:1])
    over = max(R.max_err(bad, ref) / bar, R.rel_l2(bad, ref) / bar2)
    print(f"UNETBLOCK cfg_dup {name} E={e:.3e} bar={bar:.3e} | rel-L2 E={e2:.3e} bar={bar2:.3e} | cfgstale {over:.2f}x")
    assert over > 1.0


def test_gn_eps_1e5_is_below_fp16(net):
    """Why 'gneps' is a printed row and no assertion: the groups' variances at a transformer's input are of order
    0.1 to 1, so eps 1e-5 for 1e-6 moves the output by a small fraction of half an fp16 ulp, the bar's floor."""
    _, _, wk = net
    inp = B.inputs_of(2, 16, 16)
    g = torch.Generator().manual_seed(13)
    for name, c in (("down_blocks.0.attentions.0", 320), ("mid_block.attentions.0", 1280)):
        io = dict(wk.context(inp), x=torch.randn(2, 4, 4, c, generator=g).half())
        ref, bad = wk.stage(name, "ref", io), wk.stage(name, "ref", io, defect="gneps")
        print(f"UNETBLOCK gneps {name}: max {R.max_err(bad, ref):.3e} (half ulp {R.half_ulp16(ref.abs().max().item()):.3e}), "
              f"rel-L2 {R.rel_l2(bad, ref):.3e}")
        assert R.max_err(bad, ref) < 0.1 * R.half_ulp16(ref.abs().max().item())
        assert R.rel_l2(bad, ref) < 0.1 * 2.0 ** -11
