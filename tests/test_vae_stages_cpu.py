"""tests/vae_stage_ref.py checked without a GPU: the float64 walker is the same network as the two committed VAE
references, every stage's emulation lies inside its bar at every case the GPU tests run, every planted defect lies
outside, and the saturating decoder case saturates."""
import pytest
import torch

from clap2diffusion_amd import weights as W
from oracle.vae_ref import VAEDecoderRef
from tests import small_shape_ref as R
from tests import vae_stage_ref as V
from tests.vae_encoder_ref import encoder_ref

CASES = [("decoder", c) for c in V.DEC_CASES] + [("encoder", c) for c in V.ENC_CASES]


@pytest.fixture(scope="module")
def halves():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = {"decoder": W.synth_vae_decoder(0), "encoder": W.synth_vae_encoder(0)}
    return sd, {h: V.VaeStages(sd[h], h) for h in sd}


def input_of(half, case):
    return V.latents_of(*case) if half == "decoder" else V.image_of(*case)


def test_stage_lists(halves):
    _, vs = halves
    assert len(vs["decoder"].names) == 5 + 12 + 3 + 1 and len(set(vs["decoder"].names)) == 21
    assert len(vs["encoder"].names) == 1 + 8 + 3 + 3 + 2 and len(set(vs["encoder"].names)) == 17
    assert vs["decoder"].names[3] == "mid.attentions.0" and vs["decoder"].names[-1] == "conv_norm_out+conv_out"
    assert vs["encoder"].names[3] == "down_blocks.0.downsamplers.0" and vs["encoder"].names[-1] == "quant_conv"


def test_walker_is_the_decoder_oracle(halves):
    sd, vs = halves
    z = V.latents_of(2, 8, 16)
    x = vs["decoder"].trace(z)[-1][2]
    img = (x / 2 + 0.5).clamp(0, 1).permute(0, 3, 1, 2)
    rel = R.rel_l2(VAEDecoderRef(sd["decoder"])(z), img)
    print(f"VAESTAGE decoder walker vs oracle/vae_ref rel-L2 {rel:.3e}")
    assert rel <= 1e-5


def test_walker_is_the_encoder_reference(halves):
    sd, vs = halves
    img = V.image_of(2, 64, 128)
    mom = vs["encoder"].trace(img)[-1][2]
    rel = R.rel_l2(encoder_ref(sd["encoder"]).moments(img).permute(0, 2, 3, 1), mom)
    print(f"VAESTAGE encoder walker vs tests/vae_encoder_ref rel-L2 {rel:.3e}")
    assert rel <= 1e-5


@pytest.mark.parametrize("half,case", CASES, ids=[f"{h}-{'x'.join(map(str, c))}" for h, c in CASES])
def test_emulation_inside_and_defects_outside_every_bar(halves, half, case):
    """Per stage: the emulation (and an upsampler's materialised form) within bar_of / bar_l2_of, with neither cap
    binding; every defect that applies beyond at least one of the two, so the GPU test would fail on it."""
    _, vs = halves
    vs = vs[half]
    seen = set()
    for row in V.stage_table(vs, input_of(half, case)):
        name, x16, ref = row["name"], row["x16"], row["ref"]
        (e, bar), (e2, bar2) = row["bar"], row["bar_l2"]
        assert torch.isfinite(ref).all() and torch.isfinite(row["emu"].float()).all(), name
        assert e <= bar and e2 <= bar2, (name, e, bar, e2, bar2)
        assert 3 * e <= R.CAP_MAX * ref.abs().max().item() and 3 * e2 <= R.CAP_L2, f"{name}: a cap binds"
        if "upsamplers" in name:
            mat = vs.stage_emul(name, x16, folded=False)
            assert R.max_err(mat, ref) <= bar and R.rel_l2(mat, ref) <= bar2, name
        line = f"VAESTAGE {half} {case} {name} E={e:.3e} bar={bar:.3e} | rel-L2 E={e2:.3e} bar={bar2:.3e}"
        for d in vs.defects(name, case[0]):
            bad = vs.stage_ref(name, x16, defect=d)
            over, over2 = R.max_err(bad, ref) / bar, R.rel_l2(bad, ref) / bar2
            line += f" | {d} {over:.1f}x {over2:.1f}x"
            assert max(over, over2) > 1.0, f"{name}: defect {d} hides inside the bar ({over:.2f}x, {over2:.2f}x)"
            seen.add(d)
        print(line)
    want = {"decoder": {"qscale", "vbias", "phase", "shortcut", "normeps"},
            "encoder": {"qscale", "vbias", "padbefore", "shortcut", "normeps"}}[half]
    assert seen == want | ({"image"} if case[0] > 1 else set())


def test_eps_1e5_is_below_fp16(halves):
    """Why there is no 'eps' defect: eps 1e-5 for 1e-6 in the final norm moves the output by a small fraction of
    the bar's floor, half an fp16 ulp."""
    _, vs = halves
    for half, case in (("decoder", V.DEC_CASES[0]), ("encoder", V.ENC_CASES[0])):
        name, x_in, _ = vs[half].trace(input_of(half, case))[-2 if half == "encoder" else -1]
        assert name == "conv_norm_out+conv_out"
        ref = vs[half].stage_ref(name, x_in.half())
        bad = vs[half].stage_ref(name, x_in.half(), defect="eps")
        assert R.max_err(bad, ref) < 0.1 * R.half_ulp16(ref.abs().max().item())
        assert R.rel_l2(bad, ref) < 0.1 * 2.0 ** -11


def test_saturating_case_saturates(halves):
    sd, vs = halves
    z = V.latents_of(*V.SAT_CASE, scale=V.SAT_LATENT_SCALE)
    plain = V.saturated_share(V.quantize(vs["decoder"].trace(z)[-1][2]))
    sat = V.VaeStages(V.saturating_sd(sd["decoder"]), "decoder")
    q = V.quantize(sat.trace(z)[-1][2])
    share, lo, hi = V.saturated_share(q), (q == 0).float().mean().item(), (q == 255).float().mean().item()
    print(f"VAESTAGE saturated share {share:.4f} (0: {lo:.4f}, 255: {hi:.4f}); the latent scale alone: {plain:.4f}")
    assert plain < 0.01                      # the scale alone does not reach the clamp
    assert 0.05 <= share <= 0.5
    assert lo > 0.01 and hi > 0.01           # both ends
    emu = V.quantize(sat.chain_emul(z).double())
    assert (emu.int() - q.int()).abs().max().item() <= 1
