"""DPM-Solver++(2M) on the GPU: c2d_cfg_dpm_step and c2d_cfg_dpm_step_masked against the float64 restatement of
tests/dpm_ref.py and against c2d_cfg_ddim_step, the sampler's graph against its eager body and a host loop over the
scheduler's host step, and the pipeline's sampler= argument.

Bars.  Against float64 (evaluated from the fp16-rounded eps the kernel reads): max-abs error <= 3 E, E the max-abs
error of the same formulas evaluated by torch in fp32 on the CPU from the reference's lambdas, floor 1e-5 absolute:
the recipe of test_inpaint_gpu.py.  x and x0_prev each have their own E.  Masked step: bit-identical to the unmasked
op where the mask is 1; where it is 0 bit-identical to z0 at the last step and rtol 1e-5 / atol 1e-6 against the
fp32 add_noise formula otherwise.  Wherever two HIP runs of the same launches are compared (graph against eager, a
second run, the default against sampler="ddim", BatchGraph against generate_batch): bit equality."""
import functools

import numpy as np
import pytest
import torch

from clap2diffusion_amd import ops
from clap2diffusion_amd.pipeline import AudioToImageInference, initial_latents, synthetic_thunder
from clap2diffusion_amd.sampler import GraphDenoiser
from clap2diffusion_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
from clap2diffusion_amd.text_encoder import tokenize
from tests import dpm_ref, parity_log
from tests.test_img2img_gpu import make_image
from tests.test_inpaint_gpu import MASK_VALUES, SHAPES, guarded, guards_intact
from tests.test_kernels_gpu import gen, nhwc

pytestmark = pytest.mark.gpu

GUIDANCE = 7.5
# (steps, step): the first, a middle and the last step of a table whose last row is first-order (S < 15) and of one
# whose last row is second-order
STEP_CASES = [(4, 0), (4, 2), (4, 3), (16, 0), (16, 7), (16, 15)]
IDX_FILL = -77


@functools.lru_cache(maxsize=None)
def tables(steps, solver_order=2):
    """(mcoef, DDIM's coef) fp32 on the host."""
    s = DPMSolverMultistepScheduler(solver_order=solver_order)
    s.set_timesteps(steps)
    _, coef2, mcoef = s.device_tables("cpu")
    return mcoef, coef2


@functools.lru_cache(maxsize=None)
def step_case(b, hw):
    """(x, x0_prev, z0, noise NCHW fp32, eps NHWC fp16 [2b]) of one shape, computed once, never written."""
    h, w = SHAPES[hw]
    x, x0p, z0, noise = (gen(b, 4, h, w, seed=70 + k + hw) for k in range(4))
    return x, x0p, z0, noise, nhwc(gen(2 * b, 4, h, w, seed=75 + hw)).half()


def is_first_order(steps, st, first, solver_order=2):
    """Row 0 has no earlier step (1 / (2 r) = 0): it is first-order whatever first_step says."""
    return st == 0 or dpm_ref.first_order(st, steps, first, solver_order)


def counter(value, dev):
    """(guarded int32 buffer, its one-element view) holding `value`."""
    buf, idx = guarded((1,), torch.int32, dev, fill=IDX_FILL)
    idx.fill_(value)
    return buf, idx


def run_step(dev, b, hw, steps, st, first, advance, x0_prev=None, masked=None, solver_order=2, eps=None):
    """One launch on guarded copies of the case's buffers -> (x, x0_prev) on the host, every guard and the counter
    checked.  masked: (z0, noise, mask) on the host, or None; x0_prev, eps: in place of the case's."""
    x, x0p, _, _, case_eps = step_case(b, hw)
    eps = case_eps if eps is None else eps
    h, w = SHAPES[hw]
    bx, xd = guarded((b, 4, h, w), torch.float32, dev)
    bp, pd = guarded((b, 4, h, w), torch.float32, dev)
    xd.copy_(x)
    pd.copy_(x0p if x0_prev is None else x0_prev)
    bi, idx = counter(st, dev)
    bf, fst = counter(first, dev)
    mcoef = tables(steps, solver_order)[0].to(dev)
    if masked is None:
        out = ops.cfg_dpm_step(eps.to(dev), xd, pd, GUIDANCE, mcoef, idx, fst, advance=advance)
    else:
        z0d, nd, md = (t.to(dev) for t in masked)
        out = ops.cfg_dpm_step_masked(eps.to(dev), xd, pd, z0d, nd, md, GUIDANCE, mcoef, idx, fst, advance=advance)
        assert all(torch.equal(d.cpu(), t) for d, t in zip((z0d, nd, md), masked))
    assert out.data_ptr() == xd.data_ptr()
    assert idx.item() == st + int(advance) and fst.item() == first
    assert all(guards_intact(g) for g in (bx, bp)) and all(guards_intact(g, IDX_FILL) for g in (bi, bf))
    assert torch.equal(mcoef.cpu(), tables(steps, solver_order)[0])
    return xd.cpu(), pd.cpu()


def check_against_reference(got, ref, ref32, what):
    err, e_cpu = (got.double() - ref).abs().max().item(), (ref32.double() - ref).abs().max().item()
    bar = max(3.0 * e_cpu, 1e-5)
    parity_log.record(**{f"{what}_max_abs": err, f"{what}_cpu_fp32_max_abs": e_cpu, f"{what}_bar": bar,
                         f"{what}_ref_max": ref.abs().max().item()})
    print(f"  {what}: E={e_cpu:.3e} gpu={err:.3e} bar={bar:.3e}")
    assert err <= bar, (what, err, e_cpu, bar)


# ------------------------------------------------------------------ unmasked step
@pytest.mark.parametrize("steps,st", STEP_CASES)
@pytest.mark.parametrize("hw", sorted(SHAPES))
@pytest.mark.parametrize("b", [1, 3])
def test_cfg_dpm_step(dev, b, hw, steps, st):
    """Measured on an MI355X: in every case whose bar is 3 E the GPU error equals E to the printed digits (0.33 of
    the bar: the kernel performs the fp32 restatement's operations), e.g. b = 1, hw = 63, S = 4, step 0:
    x 3.388e-6 / 3.388e-6 / 1.016e-5 (E / GPU error / bar); S = 16, step 7: x0_prev 4.058e-6 / 4.058e-6 / 1.217e-5.
    Every case is in the parity log."""
    x, x0p, _, _, eps = step_case(b, hw)
    g = dpm_ref.grid(steps)
    for first in (st, (st + 1) % steps):                       # this step opens the run / another one did
        order1 = is_first_order(steps, st, first)
        refs = [dpm_ref.step(dpm_ref.cfg(eps, GUIDANCE, dt), x, x0p, g, st, order1, dt)
                for dt in (torch.float64, torch.float32)]
        outs = {}
        for advance in (True, False):
            print(f"b={b} hw={hw} S={steps} st={st} first={first} advance={advance}")
            gx, gp = outs[advance] = run_step(dev, b, hw, steps, st, first, advance)
            check_against_reference(gx, refs[0][0], refs[1][0], "x")
            check_against_reference(gp, refs[0][1], refs[1][1], "x0_prev")
        assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])
    if 0 < st < steps - 1:                                      # the two orders are different tensors there
        one, two = (dpm_ref.step(dpm_ref.cfg(eps, GUIDANCE), x, x0p, g, st, o)[0] for o in (True, False))
        assert not torch.allclose(one, two, atol=1e-2)


@pytest.mark.parametrize("steps,st,first,solver_order", [(4, 0, 0, 2), (4, 2, 2, 2), (4, 3, 0, 2), (16, 7, 0, 1)])
def test_first_order_step_does_not_read_x0_prev(dev, steps, st, first, solver_order):
    """The run's first step, the lower-order final step and a solver_order = 1 row: x0_prev may hold anything."""
    b, hw = 3, 1000
    nan = torch.full_like(step_case(b, hw)[0], float("nan"))
    gx, gp = run_step(dev, b, hw, steps, st, first, True, x0_prev=nan, solver_order=solver_order)
    assert torch.isfinite(gx).all() and torch.isfinite(gp).all()
    wx, wp = run_step(dev, b, hw, steps, st, first, True, solver_order=solver_order)
    assert torch.equal(gx, wx) and torch.equal(gp, wp)


def test_second_order_step_reads_x0_prev(dev):
    """The counterpart: where the step is second-order a NaN in x0_prev reaches x (and x0_prev is still rewritten)."""
    b, hw = 1, 64
    nan = torch.full_like(step_case(b, hw)[0], float("nan"))
    gx, gp = run_step(dev, b, hw, 4, 2, 0, True, x0_prev=nan)
    assert torch.isnan(gx).all() and torch.isfinite(gp).all()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("value", [4, -1, 1 << 20])
def test_counter_outside_the_table_touches_nothing(dev, value, masked):
    b, hw, steps = 3, 1000, 4
    x, x0p, z0, noise, eps = step_case(b, hw)
    h, w = SHAPES[hw]
    for advance in (False, True):
        bx, xd = guarded((b, 4, h, w), torch.float32, dev)
        bp, pd = guarded((b, 4, h, w), torch.float32, dev)
        xd.copy_(x)
        pd.copy_(x0p)
        bi, idx = counter(value, dev)
        fst = torch.full((1,), value, dtype=torch.int32, device=dev)
        mcoef = tables(steps)[0].to(dev)
        if masked:
            ops.cfg_dpm_step_masked(eps.to(dev), xd, pd, z0.to(dev), noise.to(dev), torch.ones(b, h, w, device=dev),
                                    GUIDANCE, mcoef, idx, fst, advance=advance)
        else:
            ops.cfg_dpm_step(eps.to(dev), xd, pd, GUIDANCE, mcoef, idx, fst, advance=advance)
        assert torch.equal(xd.cpu(), x) and torch.equal(pd.cpu(), x0p)
        assert guards_intact(bx) and guards_intact(bp) and guards_intact(bi, IDX_FILL)   # the counter's neighbours
        assert idx.item() == value + int(advance)


@pytest.mark.parametrize("st", [0, 2, 3])
@pytest.mark.parametrize("hw", sorted(SHAPES))
@pytest.mark.parametrize("b", [1, 3])
def test_solver_order_1_table_is_the_ddim_kernel(dev, b, hw, st):
    """Against the kernel the tree already trusts: with a solver_order = 1 table the update is algebraically DDIM.

    The bar (3 E, floor 1e-5) is the DPM formula's; the DDIM kernel has an error of its own, which the inputs must
    keep below that floor for the comparison to say anything about the new kernel.  DDIM's last line adds the
    rounded products sqrt(a_prev) x0 and sqrt(1 - a_prev) e, which cancel: its error is up to about 2 ulp of the
    larger product T.  With the other tests' inputs (unit-variance eps at guidance 7.5: e has std 9.9 and reaches
    36) T reaches 76 at step 0, 2 ulp of that is 1.5e-5, and that is what was measured on an MI355X and in an fp32
    CPU restatement of both kernels at b = 3, hw = 63, step 0: |dpm - ddim| = 1.526e-5 against a bar of 1.10e-5,
    with the DPM kernel 2.9e-7 and the DDIM form 1.50e-5 from float64 at that element.  So this test scales eps by
    1 / 16 (exact in fp16; the guided e then has std 0.62, the range of a real UNet's prediction) and asserts
    T < 16, where 2 ulp is 3.8e-6; shapes, steps, table and bar are unchanged.  Measured then on an MI355X: the
    largest |dpm - ddim| is 1.907e-6 (b = 1, hw = 1000, step 0, E 1.398e-6, bar 1e-5)."""
    steps = 4
    x, x0p, _, _, eps16 = step_case(b, hw)
    eps = eps16 / 16
    g = dpm_ref.grid(steps)
    e64 = dpm_ref.cfg(eps, GUIDANCE)
    x0_64 = dpm_ref.step(e64, x, None, g, st, True)[1]
    assert max((g.alpha_t[st] * x0_64).abs().max(), (g.sigma_t[st] * e64).abs().max()) < 16.0
    xd = x.clone().to(dev)                                     # the case's tensors are shared: never written
    ops.cfg_ddim_step(eps.to(dev), xd, GUIDANCE, tables(steps)[1].to(dev),
                      torch.tensor([st], dtype=torch.int32, device=dev), advance=False)
    gx, gp = run_step(dev, b, hw, steps, st, (st + 1) % steps, False, solver_order=1, eps=eps)
    ref, ref32 = (dpm_ref.step(dpm_ref.cfg(eps, GUIDANCE, dt), x, None, g, st, True, dt)
                  for dt in (torch.float64, torch.float32))
    e_cpu = (ref32[0].double() - ref[0]).abs().max().item()
    diff, bar = (gx - xd.cpu()).abs().max().item(), max(3.0 * e_cpu, 1e-5)
    parity_log.record(max_abs_vs_ddim=diff, cpu_fp32_max_abs=e_cpu, bar=bar)
    print(f"b={b} hw={hw} st={st}: E={e_cpu:.3e} |dpm - ddim|={diff:.3e} bar={bar:.3e}")
    assert diff <= bar, (diff, e_cpu, bar)
    check_against_reference(gx, ref[0], ref32[0], "x")


# ------------------------------------------------------------------ masked step
@pytest.mark.parametrize("steps,st,first", [(4, 0, 0), (4, 2, 0), (4, 3, 0), (16, 15, 3)])
@pytest.mark.parametrize("hw", sorted(SHAPES))
@pytest.mark.parametrize("b", [1, 3])
def test_cfg_dpm_step_masked(dev, b, hw, steps, st, first):
    x, x0p, z0, noise, eps = step_case(b, hw)
    h, w = SHAPES[hw]
    g = dpm_ref.grid(steps)
    mcoef = tables(steps)[0]
    order1 = is_first_order(steps, st, first)
    plain_x, plain_p = run_step(dev, b, hw, steps, st, first, False)
    alpha_t, sigma_t = mcoef[st, 2], mcoef[st, 3]
    known = z0 if st == steps - 1 else alpha_t * z0 + sigma_t * noise
    for shift in (range(4) if b * hw < 4 else (0,)):           # every mask value reaches the smallest cases too
        mask = MASK_VALUES[(torch.arange(b * hw) + shift) % 4].view(b, h, w)
        print(f"b={b} hw={hw} S={steps} st={st} shift={shift}")
        gx, gp = run_step(dev, b, hw, steps, st, first, True, masked=(z0, noise, mask))
        m4 = mask[:, None].expand_as(gx)
        assert torch.equal(gp, plain_p)                        # the data prediction is the unmasked one everywhere
        assert torch.equal(gx[m4 == 1], plain_x[m4 == 1])
        if st == steps - 1:
            assert torch.equal(gx[m4 == 0], z0[m4 == 0])
        else:
            assert torch.allclose(gx[m4 == 0], known[m4 == 0], rtol=1e-5, atol=1e-6)
        ref, ref32 = (dpm_ref.masked_step(dpm_ref.cfg(eps, GUIDANCE, dt), x, x0p, z0, noise, mask, g, st, order1, dt)
                      for dt in (torch.float64, torch.float32))
        check_against_reference(gx, ref[0], ref32[0], "x")


# ------------------------------------------------------------------ sampler
STEPS, SIZE = 4, 64
LAT = SIZE // 8


@pytest.fixture(scope="module")
def pipe(dev):
    return AudioToImageInference(device=dev, height=SIZE, width=SIZE, verbose=False)


@pytest.fixture(scope="module")
def conditioning(pipe, dev):
    """What a denoiser is built from and started with, at the smallest supported size (8 x 8 latents, b = 1)."""
    mel = pipe.mel_features([synthetic_thunder(3)])
    ids = (tokenize([""], dev), tokenize(["a beach"], dev))
    with torch.no_grad():
        ehs, kw, _ = pipe.condition(mel, ids[0], ids[1])
        moments = pipe.vae_encoder(make_image(SIZE, SIZE, seed=7).to(dev))
    mask = torch.zeros(1, SIZE, SIZE, dtype=torch.uint8)
    mask[:, :, :36] = 255
    return dict(mel=mel, ids=ids, ehs=ehs, kw=kw, moments=moments, mask=mask.to(dev),
                noise=initial_latents([5], LAT, LAT, dev))


def make_denoiser(pipe, conditioning, use_graph):
    sched = DPMSolverMultistepScheduler()
    sched.set_timesteps(STEPS)
    return GraphDenoiser(pipe.unet, sched, 1, LAT, LAT, GUIDANCE, conditioning["ehs"], conditioning["kw"],
                         use_graph=use_graph)


def modes(c):
    """mode -> (t_start, start()'s keywords)."""
    return {"text-to-image": (0, {}), "img2img": (2, dict(moments=c["moments"])),
            "inpaint": (1, dict(moments=c["moments"], mask_u8=c["mask"]))}


@torch.no_grad()
def sample(den, c, mode, spy=None):
    """One run -> (final latents, the latents the loop started from), both cloned.  spy: a list that receives every
    UNet output of the run (the eager body only)."""
    t_start, kw = modes(c)[mode]
    masked = "mask_u8" in kw
    den.prepare_context()
    den.ensure_captured(masked)
    den.start(c["noise"], t_start, eps=None, **kw)
    assert den.first_idx.item() == t_start and den.step_idx.item() == t_start
    x_start = den.x.clone()
    if spy is not None:
        inner = den.unet.forward_nhwc

        def recording(*args, **kwargs):
            out = inner(*args, **kwargs)
            spy.append(out.clone())
            return out
        den.unet.forward_nhwc = recording
    try:
        out = den.denoise(t_start, masked).clone()
    finally:
        if spy is not None:
            del den.unet.forward_nhwc
    assert den.step_idx.item() == STEPS and den.first_idx.item() == t_start
    return out, x_start


def host_loop(eps_per_step, x_start, t_start, dtype, blend=None):
    """The scheduler's host step over the recorded UNet outputs (fp16 NHWC), in dtype, with the inpainting blend of
    tests/dpm_ref.py after each step when blend = (z0, noise, mask)."""
    sched = DPMSolverMultistepScheduler()
    sched.set_timesteps(STEPS)
    sched.reset(t_start)
    g = dpm_ref.grid(STEPS)
    x = x_start.cpu().to(dtype)
    for i, eps in zip(range(t_start, STEPS), eps_per_step):
        x = sched.step(dpm_ref.cfg(eps.cpu(), GUIDANCE, dtype), g.ts[i], x).prev_sample
        assert x.dtype == dtype
        if blend is not None:
            x = dpm_ref.blend(x, *blend, g, i, dtype)
    return x


def test_sampler_graph_eager_and_host_loop(pipe, conditioning):
    """Measured on an MI355X (E / GPU error / bar): text-to-image 3.554e-6 / 3.554e-6 / 1.066e-5, img2img
    2.152e-7 / 2.152e-7 / 1e-5, inpainting 8.870e-7 / 8.870e-7 / 1e-5."""
    c = conditioning
    graphed, eager = make_denoiser(pipe, c, True), make_denoiser(pipe, c, False)
    first_run = {}
    for mode, (t_start, kw) in modes(c).items():
        spy = []
        want, x_start = sample(eager, c, mode, spy)
        assert eager.graph is None and eager.graph_masked is None and len(spy) == STEPS - t_start
        got, x_start_g = sample(graphed, c, mode)
        assert graphed.graph is not None
        assert torch.equal(x_start_g, x_start) and torch.equal(got, want), mode        # replay == eager body, bit for bit
        first_run[mode] = got
        blend = None
        if "mask_u8" in kw:
            assert graphed.graph_masked is not None
            blend = (eager.z0.cpu(), eager.noise.cpu(), eager.mask.cpu())
            assert 0 < blend[2].mean() < 1
        ref = host_loop(spy, x_start, t_start, torch.float64, blend)
        ref32 = host_loop(spy, x_start, t_start, torch.float32, blend)
        print(mode)
        check_against_reference(got.cpu(), ref, ref32, "latents")
    for mode in modes(c):                                       # nothing leaks from run to run through x0_prev
        assert torch.equal(sample(graphed, c, mode)[0], first_run[mode]), mode
    assert not torch.equal(first_run["text-to-image"], first_run["img2img"])
    # a DDIM denoiser on the same UNet holds none of the multistep state and gives other latents
    sched = DDIMScheduler()
    sched.set_timesteps(STEPS)
    ddim = GraphDenoiser(pipe.unet, sched, 1, LAT, LAT, GUIDANCE, c["ehs"], c["kw"], use_graph=False)
    assert not hasattr(ddim, "x0_prev")
    with torch.no_grad():
        assert not torch.equal(ddim.run(c["noise"]), first_run["text-to-image"])


# ------------------------------------------------------------------ pipeline
def test_generate_sampler_argument(pipe):
    kw = dict(text_prompt="a beach", num_inference_steps=STEPS, seed=1)
    a = np.asarray(pipe.generate("synthetic:3", sampler="dpmpp_2m", **kw))
    b = np.asarray(pipe.generate("synthetic:3", sampler="dpmpp_2m", **kw))
    default = np.asarray(pipe.generate("synthetic:3", **kw))
    ddim = np.asarray(pipe.generate("synthetic:3", sampler="ddim", **kw))
    assert a.shape == (SIZE, SIZE, 3) and np.array_equal(a, b)
    assert np.array_equal(default, ddim)
    assert not np.array_equal(a, ddim)
    assert pipe.last_denoiser.dpm is False
    samplers = sorted(k[-1] for k in pipe._denoisers)
    assert set(samplers) == {"ddim", "dpmpp_2m"}
    with pytest.raises(ValueError):
        pipe.generate("synthetic:3", sampler="euler", **kw)


def test_batch_graph_matches_generate_batch(pipe, conditioning, dev):
    c = conditioning
    clips = pipe.feature_extractor.crop([synthetic_thunder(3)])
    wv = torch.from_numpy(np.concatenate(clips)).to(dev)
    lens = torch.tensor([x.size for x in clips], dtype=torch.int32, device=dev)
    offs = torch.zeros(1, dtype=torch.int64, device=dev)
    melg = pipe.feature_extractor.from_device(wv, offs, lens)
    eager = pipe.generate_batch(melg, None, STEPS, GUIDANCE, ids=c["ids"], latents=c["noise"],
                                sampler="dpmpp_2m").clone()
    assert pipe.last_denoiser.dpm
    graphed = pipe.generate_batch_graphed(wv, offs, lens, c["ids"], c["noise"], STEPS, GUIDANCE,
                                          sampler="dpmpp_2m").clone()
    assert pipe.last_denoiser.dpm and pipe.last_denoiser.step_idx.item() == STEPS
    assert torch.equal(graphed, eager)
    ddim = pipe.generate_batch_graphed(wv, offs, lens, c["ids"], c["noise"], STEPS, GUIDANCE).clone()
    assert not pipe.last_denoiser.dpm and not torch.equal(ddim, graphed)
    assert torch.equal(ddim, pipe.generate_batch(melg, None, STEPS, GUIDANCE, ids=c["ids"], latents=c["noise"]))
    again = pipe.generate_batch_graphed(wv, offs, lens, c["ids"], c["noise"], STEPS, GUIDANCE, sampler="dpmpp_2m")
    assert torch.equal(again, graphed)                         # the two samplers' graphs share no state
    assert sorted(k[7] for k in pipe._batch_graphs) == ["ddim", "dpmpp_2m"]
