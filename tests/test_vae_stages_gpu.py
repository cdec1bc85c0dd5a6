"""The HIP VAE decoder and encoder stage by stage against float64 (tests/vae_stage_ref.py): every stage is fed the
reference's own input to it, rounded to fp16, and held to the bar its fp16-storage emulation sets; then the whole
halves as float tensors, the decoder's quantisation and clamp, and its refusal of sizes the mid attention cannot run."""
import pytest
import torch
import torch.nn.functional as F

from clap2diffusion_amd import ops
from clap2diffusion_amd import weights as W
from clap2diffusion_amd.vae import VAEDecoder, VAEEncoder
from tests import parity_log
from tests import small_shape_ref as R
from tests import vae_stage_ref as V

pytestmark = pytest.mark.gpu

F16 = torch.float16
CASES = [("decoder", c) for c in V.DEC_CASES] + [("encoder", c) for c in V.ENC_CASES]
IDS = [f"{h}-{'x'.join(map(str, c))}" for h, c in CASES]


@pytest.fixture(scope="module")
def nets(dev):
    """HIP modules and the stage walkers over the same seeded weights; 'saturating' is the decoder with conv_out's
    bias moved (vae_stage_ref.SAT_BIAS)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = {"decoder": W.synth_vae_decoder(0), "encoder": W.synth_vae_encoder(0)}
    sd["saturating"] = V.saturating_sd(sd["decoder"])
    hip = {"decoder": VAEDecoder().to(dev), "encoder": VAEEncoder().to(dev), "saturating": VAEDecoder().to(dev)}
    for k, m in hip.items():
        m.load_diffusers_state_dict(sd[k])
    vs = {k: V.VaeStages(sd[k], "encoder" if k == "encoder" else "decoder") for k in sd}
    return hip, vs


@pytest.fixture(scope="module")
def tables(nets):
    """(half, case) -> (input, stage_table), computed once and left unchanged."""
    _, vs = nets
    cache = {}

    def get(half, case):
        if (half, case) not in cache:
            x = V.latents_of(*case) if half == "decoder" else V.image_of(*case)
            cache[half, case] = (x, V.stage_table(vs[half], x))
        return cache[half, case]
    return get


def pad_c(x16: torch.Tensor, c: int, dev) -> torch.Tensor:
    return F.pad(x16, (0, c - x16.shape[-1])).contiguous().to(dev)


def run_stage(hip, half: str, name: str, x16: torch.Tensor, dev) -> torch.Tensor:
    """The HIP submodule of a stage on the stage's fp16 NHWC input -> its fp16 output (pad channels included)."""
    net = hip.decoder if half == "decoder" else hip.encoder
    if name == "post_quant_conv":
        return hip.post_quant_conv(pad_c(x16, 8, dev))
    if name == "conv_in":
        return net.conv_in(pad_c(x16, 8, dev))
    x = x16.contiguous().to(dev)
    if name == "quant_conv":
        return hip.quant_conv(x)
    if name == "conv_norm_out+conv_out":
        return net.conv_out(net.conv_norm_out.apply(x, silu=True))
    parts = name.split(".")
    if parts[0] == "mid":
        return getattr(net.mid_block, parts[1])[int(parts[2])](x)
    blk = getattr(net, parts[0])[int(parts[1])]
    return getattr(blk, parts[2])[int(parts[3])](x)


def judge(tag, name, out, row, plans, failures):
    """One line and one parity_log row per stage; a miss is collected, so that a run names every stage that fails."""
    ref = row["ref"]
    (e, bar), (e2, bar2) = row["bar"], row["bar_l2"]
    o = out.float().cpu()
    c = ref.shape[-1]
    finite = bool(torch.isfinite(o).all())
    pad_zero = bool((o[..., c:] == 0).all())
    err, l2 = R.max_err(o[..., :c], ref), R.rel_l2(o[..., :c], ref)
    plan = ",".join(f"{t}/{k}" for t, k in plans)
    parity_log.record(stage=f"{tag}:{name}", max_abs=err, emul_E=e, bar=bar, rel_l2=l2, emul_E_l2=e2, tol_l2=bar2, plans=plan)
    print(f"VAESTAGE {tag} {name} E={e:.3e} gpu={err:.3e} bar={bar:.3e} | rel-L2 E={e2:.3e} gpu={l2:.3e} bar={bar2:.3e} "
          f"| plans {plan}")
    if not (finite and pad_zero and tuple(o.shape[:-1]) == tuple(ref.shape[:-1]) and err <= bar and l2 <= bar2):
        failures.append(f"{tag} {name}: finite {finite}, pad channels zero {pad_zero}, max|out - ref| {err:.3e} "
                        f"(bar {bar:.3e}, E {e:.3e}), rel-L2 {l2:.3e} (bar {bar2:.3e}, E {e2:.3e}), plans {plan}")


@pytest.mark.parametrize("half,case", CASES, ids=IDS)
def test_stage_by_stage(dev, nets, tables, half, case):
    hip, _ = nets
    _, table = tables(half, case)
    tag = f"{half} {'x'.join(map(str, case))}"
    failures = []
    for row in table:
        with ops.record_conv_plans() as plans:
            out = run_stage(hip[half], half, row["name"], row["x16"], dev)
            torch.cuda.synchronize()
        judge(tag, row["name"], out, row, plans, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("form", ["folded", "materialised"])
@pytest.mark.parametrize("case", V.DEC_CASES, ids=["x".join(map(str, c)) for c in V.DEC_CASES])
def test_upsamplers_in_both_forms(dev, nets, tables, monkeypatch, case, form):
    """Upsample2D at 512 -> 512 (twice) and 256 -> 256: the four folded phase convs where ops.upfold_ok takes the
    shape, and nearest x2 + 3x3 when it refuses; one reference and one bar for both."""
    hip, _ = nets
    _, table = tables("decoder", case)
    calls = {"folded": 0, "materialised": 0}
    up2x = ops.upsample_nearest2x
    monkeypatch.setattr(ops, "upsample_nearest2x", lambda *a, **k: (calls.__setitem__("materialised", calls["materialised"] + 1),
                                                                    up2x(*a, **k))[1])
    if form == "materialised":
        monkeypatch.setattr(ops, "upfold_ok", lambda *a: False)
    failures = []
    rows = [r for r in table if "upsamplers" in r["name"]]
    assert len(rows) == 3
    for row in rows:
        n, h, w, c = row["x16"].shape
        blk = hip["decoder"].decoder.up_blocks[int(row["name"].split(".")[1])].upsamplers[0]
        fold = blk.conv.forward_folded
        monkeypatch.setattr(blk.conv, "forward_folded", lambda x, fold=fold: (calls.__setitem__("folded", calls["folded"] + 1),
                                                                               fold(x))[1])
        if form == "folded":
            assert ops.upfold_ok(n, h, w, c, c), f"the library refuses the folded upsample at {(n, h, w, c)}"
        before = dict(calls)
        with ops.record_conv_plans() as plans:
            out = blk(row["x16"].contiguous().to(dev))
            torch.cuda.synchronize()
        other = "materialised" if form == "folded" else "folded"
        assert calls[form] == before[form] + 1 and calls[other] == before[other], (form, calls)
        assert tuple(out.shape) == (n, 2 * h, 2 * w, c)
        judge(f"decoder {'x'.join(map(str, case))} {form}", row["name"], out, row, plans, failures)
    assert not failures, "\n".join(failures)


def chain_bar(vs, x, ref):
    """(E_chain, bar) of a whole half: the emulation run end to end against the float64 trace on the original
    weights; bar = max(3 E_chain, 2^-11)."""
    e = R.rel_l2(vs.chain_emul(x), ref)
    return e, max(3.0 * e, 2.0 ** -11)


@pytest.mark.parametrize("half,case", CASES, ids=IDS)
def test_whole_network_float(dev, nets, tables, half, case):
    """decode_nhwc's pre-affine RGB and the encoder's moments against the float64 network on the original weights."""
    hip, vs = nets
    x, _ = tables(half, case)
    ref = vs[half].trace(x)[-1][2]
    e, bar = chain_bar(vs[half], x, ref)
    if half == "decoder":
        out = hip[half].decode_nhwc(x.to(dev)).float().cpu()
        assert tuple(out.shape) == (*ref.shape[:-1], 4)
        assert (out[..., 3] == 0).all(), "the padded fourth output channel is not exactly 0"
        out = out[..., :3]
    else:
        out = hip[half](x.to(dev)).float().cpu().view(ref.shape)
    assert torch.isfinite(out).all()
    l2 = R.rel_l2(out, ref)
    parity_log.record(stage=f"{half} {'x'.join(map(str, case))}:whole", rel_l2=l2, emul_E_chain=e, tol_l2=bar)
    print(f"VAESTAGE {half} {case} whole rel-L2 E_chain={e:.3e} gpu={l2:.3e} bar={bar:.3e}")
    assert l2 <= bar, f"{half} {case}: rel-L2 {l2:.3e} > bar {bar:.3e} (E_chain {e:.3e})"


@pytest.mark.parametrize("which", ["unit", "saturating"])
def test_quantisation_and_clamp(dev, nets, which):
    hip, vs = nets
    if which == "unit":
        key, z = "decoder", V.latents_of(*V.DEC_CASES[2])
    else:
        key, z = "saturating", V.latents_of(*V.SAT_CASE, scale=V.SAT_LATENT_SCALE)
    img = hip[key](z.to(dev))
    x = hip[key].decode_nhwc(z.to(dev))
    assert img.dtype == torch.uint8 and tuple(img.shape) == (*x.shape[:-1], 3)
    assert torch.equal(img, VAEDecoder.quantize(x)), "forward is not the quantisation of its own decode_nhwc"
    assert torch.equal(img.cpu(), V.quantize(x.float().cpu())), "the uint8 tail differs from (x / 2 + 0.5) clamped, x 255, rounded"
    ref_x = vs[key].trace(z)[-1][2]
    ref = V.quantize(ref_x)
    emu = V.quantize(vs[key].chain_emul(z).double())
    d_gpu, d_emu = (img.cpu().int() - ref.int()).abs(), (emu.int() - ref.int()).abs()
    share_gpu, share_emu = (d_gpu == 1).float().mean().item(), (d_emu == 1).float().mean().item()
    sat = V.saturated_share(ref)
    parity_log.record(stage=f"quantise {which}", max_levels=d_gpu.max().item(), share_off_by_one=share_gpu,
                      emul_share_off_by_one=share_emu, saturated_share=sat)
    print(f"VAESTAGE quantise {which}: max {d_gpu.max().item()} levels, off by one gpu={share_gpu:.4f} "
          f"emul={share_emu:.4f}, reference pixels at 0 / 255: {sat:.4f}")
    assert d_gpu.max().item() <= 1
    assert share_gpu <= 3.0 * share_emu, (share_gpu, share_emu)
    if which == "saturating":
        assert 0.05 <= sat <= 0.5
        level = (ref_x / 2 + 0.5) * 255                      # unclamped grey level
        deep = (level <= -1.0) | (level >= 256.0)            # clamped with at least one level to spare
        assert deep.float().mean().item() > 0.01
        assert torch.equal(img.cpu()[deep], ref[deep]), "a pixel the reference clamps with a level to spare is not clamped"


@pytest.mark.parametrize("h,w", [(4, 4), (8, 12), (0, 8)])
def test_decoder_refuses_sizes_before_any_launch(dev, nets, h, w):
    hip, _ = nets
    z = torch.zeros(1, 4, h, w, device=dev)
    for call in (hip["decoder"], hip["decoder"].decode_nhwc):
        with ops.record_conv_plans() as plans:
            with pytest.raises(ValueError):
                call(z)
        assert plans == []
    with pytest.raises(ValueError):
        VAEDecoder.check_size(h, w)
    VAEDecoder.check_size(8, 8)
    VAEDecoder.check_size(4, 16)
