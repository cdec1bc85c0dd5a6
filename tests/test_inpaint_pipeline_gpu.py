"""Inpainting end to end on the GPU: c2d_inpaint_prepare against tests/vae_encoder_ref.posterior, the add_noise
formula and tests/inpaint_ref.latent_mask, and generate_batch / generate_batch_graphed / generate with a mask
against text-to-image, the init image's bytes and the fp32 composition of tests/inpaint_ref.masked_loop with the
oracle's UNet / CFG / decoder.

Bars.  inpaint_prepare: z0 and x at rtol 1e-5 / atol 1e-6, the bar of test_img2img_gpu.py::test_vae_posterior_noise
(fp32 both sides; expf against torch.exp differ by a few ulp); with pure_noise x is the noise bit for bit; the mask
is bit-exact.  Pipeline: bit equality wherever two HIP runs are compared (mask of ones against text-to-image, graph
against eager, kept pixels against the original); against the fp32 composition PSNR >= 30 dB and mean |diff| <= 3
(uint8 units), the project's documented end-to-end floor and the img2img test's bar at this size."""
import functools

import numpy as np
import pytest
import torch

from clap2diffusion_amd import ops, weights as W
from clap2diffusion_amd.pipeline import AudioToImageInference, initial_latents, synthetic_thunder
from clap2diffusion_amd.scheduler import DDIMScheduler
from clap2diffusion_amd.text_encoder import tokenize
from clap2diffusion_amd.vae import SCALING
from tests import parity_log
from tests.inpaint_ref import latent_mask, masked_loop
from tests.test_img2img_gpu import make_image, posterior_case, psnr
from tests.test_inpaint_gpu import guarded, guards_intact
from tests.test_kernels_gpu import gen, nhwc
from tests.vae_encoder_ref import encoder_ref, posterior

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ c2d_inpaint_prepare
# (n, h, w, ld): one partial 256-thread block; four blocks with a ragged last one and strided moments
KERNEL_SHAPES = [(2, 6, 8, 8), (3, 10, 26, 16)]


@functools.lru_cache(maxsize=None)
def prepare_case(n, h, w):
    """(moments NCHW fp16 [n, 8, h, w], eps, noise, coef, mask_u8 [n, 8h, 8w]) of one shape, computed once, never
    written.  The log-variances carry posterior_case()'s clamp cases; the mask holds 0 / 127 / 128 / 255 at the
    sampled (8y, 8x) positions in regions whose edges are off the 8-pixel grid, and the opposite side of the
    threshold right next to every sample."""
    mom0, eps0, noise0, coef = posterior_case()
    if (n, h, w) == tuple(mom0.shape[:1] + mom0.shape[2:]):
        mom, eps, noise = mom0, eps0, noise0
    else:
        mom = gen(n, 8, h, w, seed=61).half()
        mom[0, 4, 0, 0], mom[n - 1, 7, h - 1, w - 1], mom[0, 5, 2, 3] = -40.0, 25.0, 19.0
        eps, noise = gen(n, 4, h, w, seed=62), gen(n, 4, h, w, seed=63)
    yy, xx = torch.meshgrid(torch.arange(8 * h), torch.arange(8 * w), indexing="ij")
    inside = (yy >= 11) & (yy < 8 * h - 13) & (xx >= 5) & (xx < 8 * w - 19)         # edges off the grid
    alt = ((yy // 8 + xx // 8) % 2).bool()
    m = torch.where(inside, torch.where(alt, 255, 128), torch.where(alt, 127, 0)).to(torch.uint8)
    m = m[None].repeat(n, 1, 1)
    m[1] = 255 - m[1]                                                                # another image, another mask
    near = m.clone()
    near[:, 1::8, :] = 255 - m[:, 1::8, :]                                           # rows and columns next to the
    near[:, :, 1::8] = 255 - m[:, :, 1::8]                                           # samples: never read
    near[:, ::8, ::8] = m[:, ::8, ::8]
    return mom, eps, noise, coef, near.contiguous()


@pytest.mark.parametrize("step", [0, 3])
@pytest.mark.parametrize("pure_noise", [False, True])
@pytest.mark.parametrize("use_eps", [True, False])
@pytest.mark.parametrize("n,h,w,ld", KERNEL_SHAPES)
def test_inpaint_prepare(dev, n, h, w, ld, use_eps, pure_noise, step):
    mom, eps, noise, coef, m8 = prepare_case(n, h, w)
    z_ref = posterior(mom, eps if use_eps else None)
    x_ref = noise if pure_noise else coef[step, 0].sqrt() * z_ref + (1 - coef[step, 0]).sqrt() * noise
    m_ref = latent_mask(m8, h, w)
    assert {int(v) for v in m8[:, ::8, ::8].unique()} == {0, 127, 128, 255} and 0 < m_ref.mean() < 1
    assert torch.equal((m8[:, 1::8, ::8] >= 128).float(), 1 - m_ref)     # the row below every sample says the opposite
    rows = torch.full((n * h * w, ld), 30000.0, dtype=torch.float16, device=dev)   # columns 8.. are never read
    rows[:, :8] = nhwc(mom).reshape(n * h * w, 8).to(dev)
    bz, z0 = guarded((n, 4, h, w), torch.float32, dev)
    bx, x = guarded((n, 4, h, w), torch.float32, dev)
    bm, mask = guarded((n, h, w), torch.float32, dev)
    idx = torch.tensor([step], dtype=torch.int32, device=dev)
    epsd, noised, m8d, coefd = eps.to(dev) if use_eps else None, noise.to(dev), m8.to(dev), coef.to(dev)
    got = ops.inpaint_prepare(rows, noised, m8d, SCALING, eps=epsd, coef=None if pure_noise else coefd,
                              step_index=None if pure_noise else idx, pure_noise=pure_noise, z0=z0, x=x, mask=mask)
    assert [t.data_ptr() for t in got] == [z0.data_ptr(), x.data_ptr(), mask.data_ptr()]
    assert idx.item() == step                                            # the counter is read, never advanced
    assert guards_intact(bz) and guards_intact(bx) and guards_intact(bm)
    assert torch.equal(noised.cpu(), noise) and torch.equal(m8d.cpu(), m8)
    ez, ex = (z0.cpu() - z_ref).abs().max().item(), (x.cpu() - x_ref).abs().max().item()
    parity_log.record(z0_max_abs=ez, x_max_abs=ex)
    print(f"n={n} h={h} w={w} ld={ld} eps={use_eps} pure={pure_noise} step={step}: z0 {ez:.3e} x {ex:.3e}")
    assert torch.allclose(z0.cpu(), z_ref, rtol=1e-5, atol=1e-6), ez
    assert torch.allclose(x.cpu(), x_ref, rtol=1e-5, atol=1e-6), ex
    if pure_noise:
        assert torch.equal(x.cpu(), noise)
    assert torch.equal(mask.cpu(), m_ref)


def test_inpaint_prepare_is_the_three_launches_it_replaces(dev):
    """Against the kernels it fuses: c2d_vae_posterior_noise without and with noise, c2d_mask_to_latent."""
    n, h, w, _ = KERNEL_SHAPES[1]
    mom, eps, noise, coef, m8 = prepare_case(n, h, w)
    rows = nhwc(mom).reshape(n * h * w, 8).to(dev)
    idx = torch.tensor([3], dtype=torch.int32, device=dev)
    z0, x, mask = ops.inpaint_prepare(rows, noise.to(dev), m8.to(dev), SCALING, eps=eps.to(dev), coef=coef.to(dev),
                                      step_index=idx)
    z_old = ops.vae_posterior_noise(rows, torch.empty_like(z0), SCALING, eps=eps.to(dev))
    x_old = ops.vae_posterior_noise(rows, torch.empty_like(z0), SCALING, eps=eps.to(dev), noise=noise.to(dev),
                                    coef=coef.to(dev), step_index=idx)
    assert torch.allclose(z0, z_old, rtol=1e-5, atol=1e-6) and torch.allclose(x, x_old, rtol=1e-5, atol=1e-6)
    assert torch.equal(mask, ops.mask_to_latent(m8.to(dev)))


# ------------------------------------------------------------------ end to end
STEPS, GUIDANCE, SIZE = 4, 7.5, 64


@pytest.fixture(scope="module")
def pipe(dev):
    return AudioToImageInference(device=dev, height=SIZE, width=SIZE, verbose=False)


@pytest.fixture(scope="module")
def request_inputs(pipe, dev):
    wave = synthetic_thunder(3)
    mel = pipe.mel_features([wave])
    ids = (tokenize([""], dev), tokenize(["a beach"], dev))
    noise = initial_latents([5], SIZE // 8, SIZE // 8, dev)
    return wave, mel, ids, noise, make_image(SIZE, SIZE, seed=7).to(dev)


def partial_mask(seed=0):
    """Repaint pixel columns < 36 (latent columns 0..4: column 32 is the last sampled one below 36), plus isolated
    127 / 128 pixels, on and off the sampled grid, on either side."""
    m = torch.zeros(1, SIZE, SIZE, dtype=torch.uint8)
    m[:, :, :36] = 255
    m[0, 8, 48], m[0, 16, 56] = 128, 127            # sampled positions in the kept half: one flips to repaint
    m[0, 24, 8], m[0, 32, 16] = 127, 128            # sampled positions in the repainted half: one flips to keep
    m[0, 3, 50], m[0, 5, 10] = 128, 127             # off the grid: pixel space only
    if seed:
        m = m.flip(2).contiguous()
    return m


def run(pipe, request_inputs, mask, strength, composite=True, img=None, **kw):
    _, mel, ids, noise, image = request_inputs
    return pipe.generate_batch(mel, None, STEPS, GUIDANCE, ids=ids, latents=noise,
                               init_images=image if img is None else img, strength=strength, sample_posterior=False,
                               masks=mask, composite=composite, **kw)


def test_mask_of_ones_at_strength_1_is_text_to_image(pipe, request_inputs, dev):
    _, mel, ids, noise, img = request_inputs
    t2i = pipe.generate_batch(mel, None, STEPS, GUIDANCE, ids=ids, latents=noise).clone()
    den = pipe.last_denoiser
    graph = den.graph
    assert graph is not None and den.z0 is None and den.graph_masked is None   # text-to-image holds nothing masked
    ones = torch.full((1, SIZE, SIZE), 255, dtype=torch.uint8, device=dev)
    out = run(pipe, request_inputs, ones, 1.0).clone()
    assert pipe.last_denoiser is den and den.graph is graph and den.graph_masked is not None
    assert den.step_idx.item() == STEPS
    assert torch.equal(den.mask, torch.ones_like(den.mask)) and torch.equal(den.noise, noise)
    assert torch.equal(out, t2i)
    again = pipe.generate_batch(mel, None, STEPS, GUIDANCE, ids=ids, latents=noise)
    assert den.graph is graph and torch.equal(again, t2i)   # text-to-image is untouched by a masked call in between


@pytest.mark.parametrize("strength", [0.5, 1.0])
def test_mask_of_zeros_keeps_the_image(pipe, request_inputs, dev, strength):
    _, _, _, _, img = request_inputs
    zeros = torch.zeros(1, SIZE, SIZE, dtype=torch.uint8, device=dev)
    out = run(pipe, request_inputs, zeros, strength).clone()
    den = pipe.last_denoiser
    assert torch.equal(den.x, den.z0) and torch.equal(den.mask, torch.zeros_like(den.mask))
    z0 = den.z0.clone()
    assert torch.equal(z0, pipe.encode_image(img))          # the posterior's mode, as the img2img path encodes it
    assert torch.equal(out, img)
    plain = run(pipe, request_inputs, zeros, strength, composite=False)
    assert torch.equal(plain, pipe.vae(z0))
    assert not torch.equal(plain, img)                      # the VAE round trip is lossy: the composite did the work


@pytest.fixture(scope="module")
def oracle(request_inputs):
    """The fp32 reference's parts, built once: guided eps function, z0 of the init image, decoder."""
    from oracle.pipeline_ref import ReferencePipeline
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _, mel, ids, noise, img = request_inputs
    rp = ReferencePipeline(0)
    ehs, audio = rp.condition(mel.cpu(), ids[0].cpu(), ids[1].cpu())
    z0 = posterior(encoder_ref(W.synth_vae_encoder(0)).moments(img.cpu()), None)

    def eps_fn(x, t):
        with torch.no_grad():
            eu, ec = rp.unet(torch.cat([x, x], 0), int(t), ehs, audio).chunk(2)
        return eu + GUIDANCE * (ec - eu)

    def decode(x):
        with torch.no_grad():
            return (rp.vae(x).permute(0, 2, 3, 1) * 255).round().to(torch.uint8)
    return eps_fn, z0, decode


@pytest.mark.parametrize("strength,t_start", [(0.5, 2), (1.0, 0)])
def test_partial_mask_matches_fp32_composition(pipe, request_inputs, oracle, dev, strength, t_start):
    from oracle.ddim_ref import alphas_cumprod, timesteps
    _, mel, ids, noise, img = request_inputs
    eps_fn, z0, decode = oracle
    assert DDIMScheduler.img2img_start(STEPS, strength) == t_start
    m8 = partial_mask()
    keep = (m8 < 128)[0].to(dev)
    comp = run(pipe, request_inputs, m8.to(dev), strength).clone()
    assert torch.equal(comp[0][keep], img[0][keep])                     # every kept pixel is the original's bytes
    assert not torch.equal(comp[0][~keep], img[0][~keep])
    out = run(pipe, request_inputs, m8.to(dev), strength, composite=False).cpu()
    assert pipe.last_denoiser.step_idx.item() == STEPS
    lat_hip = pipe.last_denoiser.x.cpu().clone()
    assert torch.equal(comp[0][~keep].cpu(), out[0][~keep.cpu()])       # the composite only touches kept pixels
    ml = latent_mask(m8, SIZE // 8, SIZE // 8)
    assert torch.equal(pipe.last_denoiser.mask.cpu(), ml)
    assert ml[0, 1, 6] == 1 and ml[0, 2, 7] == 0 and ml[0, 3, 1] == 0 and ml[0, 4, 2] == 1   # the 127 / 128 samples
    assert ml[0, :, :5].sum() == 8 * 5 - 1 and ml[0, :, 5:].sum() == 1

    x = noise.cpu()
    if t_start:
        a = alphas_cumprod()[int(timesteps(STEPS)[t_start])]
        x = a.sqrt() * z0 + (1 - a).sqrt() * noise.cpu()                # DDIMScheduler.add_noise at timesteps[t_start]
    x = masked_loop(eps_fn, x, z0, noise.cpu(), ml, STEPS, t_start, dtype=torch.float32)
    ref = decode(x)
    p, mad = psnr(out, ref), (out.float() - ref.float()).abs().mean().item()
    rel = ((lat_hip - x).norm() / x.norm()).item()                      # recorded, no bar of its own
    parity_log.record(psnr_db=p, mean_abs_diff=mad, psnr_min=30.0, mad_max=3.0, latent_rel_l2=rel)
    print(f"strength {strength}: PSNR {p:.2f} dB, mean|diff| {mad:.3f}, latent rel-L2 {rel:.3e}")
    assert p >= 30.0 and mad <= 3.0, f"PSNR {p:.2f} dB, mean|diff| {mad:.2f}"

    i2i = pipe.generate_batch(mel, None, STEPS, GUIDANCE, ids=ids, latents=noise, init_images=img, strength=strength,
                              sample_posterior=False).cpu()
    t2i = pipe.generate_batch(mel, None, STEPS, GUIDANCE, ids=ids, latents=noise).cpu()
    assert not torch.equal(out, i2i) and not torch.equal(out, t2i)


def masked_keys(pipe):
    return [k for k in pipe._batch_graphs if k[-5]]          # (..., masked, composite, t_start, image, eps)


@pytest.mark.parametrize("strength,composite", [(0.5, True), (1.0, False)])
def test_batch_graph_matches_eager_and_follows_image_and_mask(pipe, request_inputs, dev, strength, composite):
    wave, mel, ids, noise, img = request_inputs
    clips = pipe.feature_extractor.crop([wave])
    wv = torch.from_numpy(np.concatenate(clips)).to(dev)
    lens = torch.tensor([c.size for c in clips], dtype=torch.int32, device=dev)
    offs = torch.zeros(1, dtype=torch.int64, device=dev)
    melg = pipe.feature_extractor.from_device(wv, offs, lens)
    before = len(masked_keys(pipe))
    m1, m2 = partial_mask().to(dev), partial_mask(1).to(dev)

    def eager(image, mask):
        return pipe.generate_batch(melg, None, STEPS, GUIDANCE, ids=ids, latents=noise, init_images=image,
                                   strength=strength, sample_posterior=False, masks=mask, composite=composite).clone()

    def graphed(image, mask):
        return pipe.generate_batch_graphed(wv, offs, lens, ids, noise, STEPS, GUIDANCE, init_images=image,
                                           strength=strength, masks=mask, composite=composite).clone()
    e = eager(img, m1)
    g = graphed(img, m1)
    den = pipe.last_denoiser
    assert den.step_idx.item() == STEPS and den.graph_masked is not None
    assert torch.equal(g, e)                                 # the bar of the text-to-image BatchGraph-against-eager test
    assert len(masked_keys(pipe)) == before + 1
    graphs = (den.graph, den.graph_masked)
    other = make_image(SIZE, SIZE, seed=8).to(dev)
    g2 = graphed(other, m2)
    assert len(masked_keys(pipe)) == before + 1              # a replay of the same graphs, not a new capture
    assert (den.graph, den.graph_masked) == graphs
    assert not torch.equal(g2, g)
    assert torch.equal(g2, eager(other, m2))
    assert all(k[-2] for k in masked_keys(pipe))             # the key still ends (init image, posterior eps)


def test_eager_body_matches_graph_replay_in_every_mode(pipe, request_inputs, dev):
    """A use_graph=False pipeline (every step the sampler's eager body, nothing captured) against the graphed `pipe`
    in text-to-image, img2img and inpainting.  Bar: bit equality of the images and the final latents; the body and
    its replay launch the same kernels on the same static buffers, and were measured bit-identical in all three
    modes at this size."""
    _, mel, ids, noise, img = request_inputs
    body = AudioToImageInference(device=dev, height=SIZE, width=SIZE, verbose=False, use_graph=False)
    modes = {"text-to-image": {}, "img2img": dict(init_images=img, strength=0.5),
             "inpaint": dict(init_images=img, strength=0.5, masks=partial_mask().to(dev))}
    for name, kw in modes.items():
        kw = dict(kw, ids=ids, latents=noise, sample_posterior=False)
        got = body.generate_batch(mel, None, STEPS, GUIDANCE, **kw)
        assert body.last_denoiser.graph is None and body.last_denoiser.graph_masked is None
        want = pipe.generate_batch(mel, None, STEPS, GUIDANCE, **kw)
        assert pipe.last_denoiser.graph is not None
        assert torch.equal(got, want), name
        assert torch.equal(body.last_denoiser.x, pipe.last_denoiser.x), name


def test_seed_fixes_both_noises(pipe, request_inputs):
    _, _, _, _, img = request_inputs
    kw = dict(text_prompt="a beach", num_inference_steps=STEPS, init_image=img[:1], strength=0.5,
              mask=partial_mask()[0].numpy())
    a = np.asarray(pipe.generate("synthetic:3", seed=11, **kw))
    b = np.asarray(pipe.generate("synthetic:3", seed=11, **kw))
    c = np.asarray(pipe.generate("synthetic:3", seed=11, sample_posterior=False, **kw))
    d = np.asarray(pipe.generate("synthetic:3", seed=12, **kw))
    assert a.shape == (SIZE, SIZE, 3) and np.array_equal(a, b)
    assert not np.array_equal(a, c)                          # the sampled posterior differs from its mode
    assert not np.array_equal(a, d)
    keep = partial_mask()[0].numpy() < 128
    assert np.array_equal(a[keep], img[0].cpu().numpy()[keep])   # composite is the default


def test_mask_needs_an_init_image(pipe, request_inputs, dev):
    wave, mel, ids, noise, img = request_inputs
    m = partial_mask()
    with pytest.raises(ValueError):
        pipe.generate("synthetic:3", num_inference_steps=STEPS, mask=m[0].numpy())
    with pytest.raises(ValueError):
        pipe.batch_generate(["synthetic:3"], num_inference_steps=STEPS, masks=m)
    with pytest.raises(ValueError):
        pipe.generate_batch(mel, None, STEPS, GUIDANCE, ids=ids, latents=noise, masks=m)
    offs, lens = torch.zeros(1, dtype=torch.int64, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        pipe.generate_batch_graphed(torch.zeros(1, device=dev), offs, lens, ids, noise, STEPS, GUIDANCE, masks=m)
    with pytest.raises(ValueError):                          # two masks for one request
        pipe.generate_batch(mel, None, STEPS, GUIDANCE, ids=ids, latents=noise, init_images=img,
                            masks=torch.cat([m, m]))
    with pytest.raises(ValueError):                          # latents of another size than the image and mask
        pipe.generate_batch(mel, None, STEPS, GUIDANCE, ids=ids, latents=initial_latents([5], 8, 16, dev),
                            init_images=img, masks=m)
