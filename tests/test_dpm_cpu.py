"""DPM-Solver++(2M) without a GPU: the scheduler's grid and coefficient table against DDIMScheduler and the float64
restatement of tests/dpm_ref.py, the host step's identities and state, the two entry points' validation through the
C ABI (no launch), the torch ops' schemas and FakeTensor tracing, and the sampler= plumbing of the pipeline.

Bars.  Table: every entry within one fp32 rounding of the float64 reference (relative 2^-23).  Identities on the
host step in float64: rtol 1e-12 (float64 round-off through a handful of operations).  Host step in fp32 over a
6-step run (and a 16-step one, whose last step is second-order): max-abs error <= 3 E against tests/dpm_ref.run in float64, E the max-abs error of the same formulas
evaluated by torch in fp32 from the reference's lambdas, floor 1e-5 absolute (the recipe of test_inpaint_gpu.py)."""
import ctypes
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from clap2diffusion_amd import ops, pipeline
from clap2diffusion_amd.pipeline import AudioToImageInference, build_parser
from clap2diffusion_amd.sampler import GraphDenoiser
from clap2diffusion_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
from tests import dpm_ref

OK, E_ARG, E_SHAPE, E_ALIGN = 0, -1, -2, -3
STEP_COUNTS = [1, 4, 14, 15, 20, 50]


def dpm(steps, **kw):
    s = DPMSolverMultistepScheduler(**kw)
    s.set_timesteps(steps)
    return s


def ddim(steps, float64=False):
    s = DDIMScheduler()
    s.set_timesteps(steps)
    if float64:   # DDIMScheduler.step takes its coefficients' dtype from the table: float64 for a float64 bar
        s.alphas_cumprod, s.final_alpha_cumprod = s.alphas_cumprod.double(), s.final_alpha_cumprod.double()
    return s


# ------------------------------------------------------------------ grid and table
@pytest.mark.parametrize("steps", STEP_COUNTS)
def test_grid_is_ddims(steps):
    s, d = dpm(steps), ddim(steps)
    assert torch.equal(s.timesteps, d.timesteps)
    assert [int(t) for t in s.timesteps] == dpm_ref.grid(steps).ts
    t_table, coef2, mcoef = s.device_tables("cpu")
    t_ddim, coef_ddim = d.device_tables("cpu")
    assert torch.equal(t_table, t_ddim) and t_table.dtype == torch.float32
    assert torch.equal(coef2, coef_ddim) and coef2.dtype == torch.float32 and coef2.shape == (steps, 2)
    assert mcoef.shape == (steps, 8) and mcoef.dtype == torch.float32 and mcoef.is_contiguous()
    assert s.init_noise_sigma == 1.0 and s.scale_model_input(t_table) is t_table
    assert DPMSolverMultistepScheduler.img2img_start is DDIMScheduler.img2img_start      # shared, not duplicated
    x, n = torch.randn(2, 3), torch.randn(2, 3)
    assert torch.equal(s.add_noise(x, n, int(s.timesteps[0])), d.add_noise(x, n, int(d.timesteps[0])))


def reference_table(steps, solver_order=2, lower_order_final=True):
    """The [S, 8] table in float64 from tests/dpm_ref.grid."""
    g = dpm_ref.grid(steps)
    h = g.lam_t - g.lam_s
    inv2r = torch.zeros(steps, dtype=torch.float64)
    inv2r[1:] = h[1:] / (2 * (g.lam_s[1:] - g.lam_s[:-1]))
    order = torch.tensor([1.0 if dpm_ref.first_order(i, steps, -1, solver_order, lower_order_final) else 2.0
                          for i in range(steps)], dtype=torch.float64)
    return torch.stack([g.alpha_s, g.sigma_s, g.alpha_t, g.sigma_t, g.sigma_t / g.sigma_s,
                        g.alpha_t * -torch.expm1(-h), inv2r, order], 1)


@pytest.mark.parametrize("steps", STEP_COUNTS)
def test_table_against_float64(steps):
    mcoef = dpm(steps).device_tables("cpu")[2]
    ref = reference_table(steps)
    rel = ((mcoef.double() - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
    print(f"S={steps}: max relative error {rel:.3e} (bar {2.0 ** -23:.3e})")
    assert rel <= 2.0 ** -23
    assert mcoef[0, 6] == 0.0                                  # no earlier step: 1 / (2 r) is 0 in row 0
    assert torch.equal(mcoef[:, 7], ref[:, 7].float())
    assert mcoef[steps - 1, 7] == (1.0 if steps < 15 else 2.0)
    assert (mcoef[:-1, 7] == 2.0).all()
    assert torch.equal(mcoef[:-1, 2:4], mcoef[1:, 0:2])        # this step's (alpha_t, sigma_t) are the next step's (alpha_s, sigma_s)


def test_table_order_flags():
    assert (dpm(20, solver_order=1).device_tables("cpu")[2][:, 7] == 1.0).all()
    assert (dpm(4, lower_order_final=False).device_tables("cpu")[2][:, 7] == 2.0).all()
    assert torch.equal(dpm(4, solver_order=1).device_tables("cpu")[2][:, :7], dpm(4).device_tables("cpu")[2][:, :7])
    with pytest.raises(ValueError):
        DPMSolverMultistepScheduler(solver_order=3)


# ------------------------------------------------------------------ host step: identities in float64
@pytest.mark.parametrize("steps", [4, 20])
def test_constant_data_prediction_is_reproduced(steps):
    """eps chosen so that x0 == c at every step, x = alpha_s c + sigma_s n: every step returns alpha_t c + sigma_t n."""
    g = dpm_ref.grid(steps)
    gen = torch.Generator().manual_seed(steps)
    c, n = (torch.randn(2, 4, 3, 5, generator=gen, dtype=torch.float64) for _ in range(2))
    s = dpm(steps)
    x = g.alpha_s[0] * c + g.sigma_s[0] * n
    for i, t in enumerate(g.ts):
        out = s.step(n, t, x)
        want = g.alpha_t[i] * c + g.sigma_t[i] * n
        assert out.prev_sample.dtype == torch.float64
        torch.testing.assert_close(out.prev_sample, want, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(out.pred_original_sample, c, rtol=1e-12, atol=1e-12)
        x = want


@pytest.mark.parametrize("steps", [4, 20, 50])
def test_solver_order_1_is_ddim(steps):
    s, d = dpm(steps, solver_order=1), ddim(steps, float64=True)
    gen = torch.Generator().manual_seed(steps)
    x = torch.randn(2, 4, 3, 5, generator=gen, dtype=torch.float64)
    for t in s.timesteps:
        e = torch.randn(x.shape, generator=gen, dtype=torch.float64)
        got, want = s.step(e, int(t), x), d.step(e, int(t), x)
        torch.testing.assert_close(got.prev_sample, want.prev_sample, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(got.pred_original_sample, want.pred_original_sample, rtol=1e-12, atol=1e-12)
        x = want.prev_sample


# ------------------------------------------------------------------ host step against the float64 reference
def fake_eps(x, t):
    """A fixed pseudo-random prediction per timestep, with a small dependence on the latents."""
    g = torch.Generator().manual_seed(t)
    return (torch.randn(x.shape, generator=g, dtype=torch.float64) + 0.1 * x.double()).to(x.dtype)


@pytest.mark.parametrize("start", [0, 2])
@pytest.mark.parametrize("steps,solver_order", [(6, 2), (6, 1), (16, 2)])
def test_host_step_fp32_against_reference(steps, solver_order, start):
    x = torch.randn(2, 4, 5, 7, generator=torch.Generator().manual_seed(3))
    ref = dpm_ref.run(fake_eps, x, steps, start, solver_order)
    e_cpu = (dpm_ref.run(fake_eps, x, steps, start, solver_order, dtype=torch.float32).double() - ref).abs().max().item()
    s = dpm(steps, solver_order=solver_order)
    s.reset(start)
    got = x.clone()
    for t in s.timesteps[start:]:
        got = s.step(fake_eps(got, int(t)), int(t), got).prev_sample
    assert got.dtype == torch.float32
    err, bar = (got.double() - ref).abs().max().item(), max(3.0 * e_cpu, 1e-5)
    print(f"S={steps} order={solver_order} start={start}: E={e_cpu:.3e} host={err:.3e} bar={bar:.3e}")
    assert err <= bar, (err, e_cpu, bar)
    s64 = dpm(steps, solver_order=solver_order)                # and in float64 the two agree to round-off
    s64.reset(start)
    got64 = x.double()
    for t in s64.timesteps[start:]:
        got64 = s64.step(fake_eps(got64, int(t)), int(t), got64).prev_sample
    torch.testing.assert_close(got64, ref, rtol=1e-12, atol=1e-12)


def test_second_order_differs_from_first():
    x = torch.randn(2, 4, 5, 7, generator=torch.Generator().manual_seed(3))
    assert not torch.allclose(dpm_ref.run(fake_eps, x, 6), dpm_ref.run(fake_eps, x, 6, solver_order=1), atol=1e-3)
    assert not torch.allclose(dpm_ref.run(fake_eps, x, 6), dpm_ref.run(fake_eps, x, 6, lower_order_final=False),
                              atol=1e-6)


# ------------------------------------------------------------------ host step: state
def test_reset_makes_its_step_first_order():
    steps, start = 6, 2
    g = dpm_ref.grid(steps)
    gen = torch.Generator().manual_seed(9)
    x, e0, e1 = (torch.randn(1, 4, 3, 3, generator=gen, dtype=torch.float64) for _ in range(3))
    s = dpm(steps)
    s.step(e0, g.ts[0], x)                                     # an earlier run leaves its x0_prev behind
    s.reset(start)
    got = s.step(e0, g.ts[start], x).prev_sample
    want, x0 = dpm_ref.step(e0, x, None, g, start, True)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    second = dpm_ref.step(e0, x, torch.zeros_like(x), g, start, False)[0]
    assert not torch.allclose(got, second, atol=1e-3)          # a second-order step there is another tensor
    got2 = s.step(e1, g.ts[start + 1], got).prev_sample        # and the step after it is second-order
    torch.testing.assert_close(got2, dpm_ref.step(e1, want, x0, g, start + 1, False)[0], rtol=1e-12, atol=1e-12)


def test_stepping_out_of_turn_raises():
    steps = 4
    s = dpm(steps)
    x = torch.zeros(1, 4, 2, 2)
    with pytest.raises(ValueError):
        s.step(x, int(s.timesteps[1]), x)                      # the run starts at step 0
    for t in s.timesteps:
        s.step(x, int(t), x)
    with pytest.raises(RuntimeError):
        s.step(x, int(s.timesteps[0]), x)                      # finished: reset first
    s.reset()
    s.step(x, int(s.timesteps[0]), x)
    s.set_timesteps(steps)                                     # a new grid is a new run
    s.step(x, int(s.timesteps[0]), x)


# ------------------------------------------------------------------ entry points
@pytest.fixture(scope="module")
def L():
    from clap2diffusion_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def hostbuf():
    buf = ctypes.create_string_buffer(4096)   # host memory: never dereferenced on these paths
    return buf, (ctypes.addressof(buf) + 15) & ~15


def entry(L, p, masked):
    """(function, good arguments, index of each named argument): x and x0_prev are 1 KiB apart, b * 4 * hw floats
    of 256 bytes each."""
    x, x0p = p + 1024, p + 2048
    if masked:
        names = ["eps", "x", "x0_prev", "z0", "noise", "mask", "b", "hw", "steps", "g", "mcoef", "idx", "first",
                 "advance", "stream"]
        good = [p, x, x0p, p, p, p, 1, 16, 4, 7.5, p, p, p, 1, None]
        return L.c2d_cfg_dpm_step_masked, good, {n: k for k, n in enumerate(names)}
    names = ["eps", "x", "x0_prev", "b", "hw", "steps", "g", "mcoef", "idx", "first", "advance", "stream"]
    good = [p, x, x0p, 1, 16, 4, 7.5, p, p, p, 1, None]
    return L.c2d_cfg_dpm_step, good, {n: k for k, n in enumerate(names)}


def test_entries_are_exported_and_declared(L):
    from clap2diffusion_amd import _lib
    for name in ("c2d_cfg_dpm_step", "c2d_cfg_dpm_step_masked"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.c2d_version().endswith(b"r7")                     # added to the r7 ABI: no struct changed


@pytest.mark.parametrize("masked", [False, True])
def test_cfg_dpm_step_validates(L, hostbuf, masked):
    """Every bad argument answers its code; none of them launches (a launch on this path would answer the HIP
    code, or 0)."""
    _, p = hostbuf
    f, good, at = entry(L, p, masked)
    pointers = ["eps", "x", "x0_prev", "mcoef", "idx", "first"] + (["z0", "noise", "mask"] if masked else [])
    for name in pointers:
        args = list(good)
        args[at[name]] = None
        assert f(*args) == E_ARG, name
    for name in ("b", "hw", "steps"):
        for bad in (0, -1):
            args = list(good)
            args[at[name]] = bad
            assert f(*args) == E_SHAPE, (name, bad)
    for b, hw in ((65536, 65536), (1 << 15, 1 << 15), (1 << 29, 1), (1, 1 << 29), (2147483647, 2147483647)):
        args = list(good)                                      # b * hw wraps an int, or b * 4 * hw passes 2^31
        args[at["b"]], args[at["hw"]] = b, hw
        assert f(*args) == E_SHAPE, (b, hw)
    for off in (0, 4, 252, -252):                              # x0_prev inside x's 256 bytes, or x inside x0_prev's
        args = list(good)
        args[at["x0_prev"]] = args[at["x"]] + off
        assert f(*args) == E_ARG, off
    args = list(good)
    args[at["eps"]] = p + 4                                     # eps is read in 8-byte pixels
    assert f(*args) == E_ALIGN
    for name in pointers[1:]:
        args = list(good)
        args[at[name]] += 2
        assert f(*args) == E_ALIGN, name
    # validation order as in the neighbouring entry points: a null pointer before a shape before an alignment
    args = list(good)
    args[at["x"]], args[at["b"]] = None, 0
    assert f(*args) == E_ARG
    args = list(good)
    args[at["b"]], args[at["mcoef"]] = 0, p + 2
    assert f(*args) == E_SHAPE


# ------------------------------------------------------------------ torch ops
def test_fake_tracing_of_the_dpm_ops():
    with FakeTensorMode():
        dev = torch.device("cuda", 0)
        x = torch.empty(2, 4, 8, 16, device=dev)
        x0p = torch.empty_like(x)
        eps = torch.empty(4, 8, 16, 4, dtype=torch.float16, device=dev)
        mask = torch.empty(2, 8, 16, device=dev)
        mcoef = torch.empty(4, 8, device=dev)
        idx = torch.empty(1, dtype=torch.int32, device=dev)
        first = torch.empty(1, dtype=torch.int32, device=dev)
        assert ops.cfg_dpm_step(eps, x, x0p, 7.5, mcoef, idx, first) is x
        assert ops.cfg_dpm_step(eps, x, x0p, 7.5, mcoef, idx, first, advance=False) is x
        z0, noise = torch.empty_like(x), torch.empty_like(x)
        assert ops.cfg_dpm_step_masked(eps, x, x0p, z0, noise, mask, 7.5, mcoef, idx, first) is x
        bad = [
            dict(x0_prev=x),                                                 # the two in-place buffers are distinct
            dict(x0_prev=torch.empty(2, 4, 8, 8, device=dev)),               # x's shape
            dict(x0_prev=x0p.half()),                                        # fp32
            dict(mcoef=torch.empty(4, 2, device=dev)),                       # the DDIM table is not this one
            dict(mcoef=mcoef.double()),
            dict(eps=eps.float()),                                           # fp16
            dict(eps=torch.empty(2, 8, 16, 4, dtype=torch.float16, device=dev)),   # the CFG pair
            dict(step_index=idx.long()),
            dict(first_step=first.long()),
            dict(first_step=torch.empty(2, dtype=torch.int32, device=dev)),
            dict(x=torch.empty(2, 3, 8, 16, device=dev), x0_prev=torch.empty(2, 3, 8, 16, device=dev)),   # c = 4 only
        ]
        base = dict(eps=eps, x=x, x0_prev=x0p, guidance=7.5, mcoef=mcoef, step_index=idx, first_step=first)
        masked = dict(base, z0=z0, noise=noise, mask=mask)
        for kw in bad:
            with pytest.raises(AssertionError):
                ops.cfg_dpm_step(**dict(base, **kw))
            with pytest.raises(AssertionError):
                ops.cfg_dpm_step_masked(**dict(masked, **kw))
        for kw in (dict(mask=torch.empty_like(x)), dict(mask=mask.half()), dict(z0=z0.half()),
                   dict(noise=torch.empty(2, 4, 8, 8, device=dev))):
            with pytest.raises(AssertionError):                              # one fp32 mask value per latent pixel
                ops.cfg_dpm_step_masked(**dict(masked, **kw))
    with pytest.raises(RuntimeError):                                        # a host tensor: no CPU path
        ops.cfg_dpm_step(torch.empty(2, 2, 2, 4, dtype=torch.float16), torch.empty(1, 4, 2, 2), torch.empty(1, 4, 2, 2),
                         7.5, torch.empty(4, 8), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    # the schemas name the mutated arguments, and only those
    mutated = {n: re.findall(r"Tensor\(a\d+!\) (\w+)", str(getattr(torch.ops.c2d, n).default._schema))
               for n in ("cfg_dpm_step", "cfg_dpm_step_masked")}
    assert mutated == {"cfg_dpm_step": ["x", "x0_prev", "step_index"],
                       "cfg_dpm_step_masked": ["x", "x0_prev", "step_index"]}
    from clap2diffusion_amd import torch_ops
    assert "cfg_dpm_step" in torch_ops.OPS and "cfg_dpm_step_masked" in torch_ops.OPS


# ------------------------------------------------------------------ pipeline and command line
class StubUNet:
    """What GraphDenoiser's constructor reads of the UNet."""
    cfg = {"block_out_channels": [320]}

    def modules(self):
        return []


@pytest.fixture
def stub_pipe():
    """An AudioToImageInference without its models: the sampler= plumbing runs on host tensors."""
    pipe = object.__new__(AudioToImageInference)
    pipe.device, pipe.height, pipe.width = torch.device("cpu"), 64, 64
    pipe.unet, pipe.use_graph = StubUNet(), False
    pipe._denoisers, pipe._batch_graphs, pipe.last_denoiser = {}, {}, None
    return pipe


def test_unknown_sampler_raises(stub_pipe):
    for call in (lambda: pipeline.check_sampler("euler"),
                 lambda: stub_pipe.generate("synthetic:0", sampler="euler"),
                 lambda: stub_pipe.batch_generate(["synthetic:0"], sampler="euler"),
                 lambda: stub_pipe.batch_generate_u8(["synthetic:0"], sampler="euler"),
                 lambda: stub_pipe.generate_batch(torch.zeros(1, 1001, 64), None, sampler="euler"),
                 lambda: stub_pipe.generate_batch_graphed(torch.zeros(4), torch.zeros(1), torch.zeros(1), None,
                                                          torch.zeros(1, 4, 8, 8), sampler="euler"),
                 lambda: stub_pipe.denoiser(1, 4, 7.5, torch.zeros(2, 77, 768), {}, sampler="euler")):
        with pytest.raises(ValueError, match="ddim.*dpmpp_2m"):
            call()
    assert pipeline.check_sampler("ddim") == "ddim" and pipeline.check_sampler("dpmpp_2m") == "dpmpp_2m"


def test_parser_has_the_sampler_flag():
    ap = build_parser()
    assert ap.parse_args(["--audio", "synthetic:0"]).sampler == "ddim"
    assert ap.parse_args(["--audio", "synthetic:0", "--sampler", "dpmpp_2m"]).sampler == "dpmpp_2m"
    with pytest.raises(SystemExit):
        ap.parse_args(["--audio", "synthetic:0", "--sampler", "euler"])


def test_denoisers_are_keyed_by_sampler(stub_pipe):
    ehs = torch.zeros(2, 77, 768)
    default = stub_pipe.denoiser(1, 4, 7.5, ehs, {})
    d_ddim = stub_pipe.denoiser(1, 4, 7.5, ehs, {}, sampler="ddim")
    d_dpm = stub_pipe.denoiser(1, 4, 7.5, ehs, {}, sampler="dpmpp_2m")
    assert default is d_ddim and d_dpm is not d_ddim and len(stub_pipe._denoisers) == 2
    assert stub_pipe.denoiser(1, 4, 7.5, ehs, {}, sampler="dpmpp_2m") is d_dpm
    k_ddim, k_dpm = sorted(stub_pipe._denoisers)
    assert [a for a, b in zip(k_ddim, k_dpm) if a != b] == ["ddim"]
    assert isinstance(d_ddim, GraphDenoiser) and type(d_ddim.sched) is DDIMScheduler
    assert type(d_dpm.sched) is DPMSolverMultistepScheduler
    # a DDIM denoiser holds none of the multistep state
    assert not any(hasattr(d_ddim, n) for n in ("x0_prev", "first_idx", "mcoef"))
    assert d_dpm.x0_prev.shape == d_dpm.x.shape == (1, 4, 8, 8) and d_dpm.x0_prev.dtype == torch.float32
    assert d_dpm.x0_prev.data_ptr() != d_dpm.x.data_ptr()
    assert d_dpm.first_idx.dtype == torch.int32 and d_dpm.first_idx.shape == (1,)
    assert d_dpm.mcoef.shape == (4, 8) and torch.equal(d_dpm.coef, d_ddim.coef)
    assert torch.equal(d_dpm.t_table, d_ddim.t_table)
    assert d_dpm.z0 is None and d_dpm.graph is None and d_dpm.graph_masked is None


def test_batch_graphs_are_keyed_by_sampler(stub_pipe, monkeypatch):
    built = []

    class StubGraph:
        def __init__(self, *args):
            built.append(args)

        def run(self, *args):
            return self

    monkeypatch.setattr(pipeline, "BatchGraph", StubGraph)
    wave, offs, lens = torch.zeros(16), torch.zeros(1, dtype=torch.int64), torch.ones(1, dtype=torch.int32)
    lat = torch.zeros(1, 4, 8, 8)
    a = stub_pipe.generate_batch_graphed(wave, offs, lens, None, lat, 4, 7.5)
    b = stub_pipe.generate_batch_graphed(wave, offs, lens, None, lat, 4, 7.5, sampler="ddim")
    c = stub_pipe.generate_batch_graphed(wave, offs, lens, None, lat, 4, 7.5, sampler="dpmpp_2m")
    assert a is b and c is not a and len(built) == 2
    assert [args[-1] for args in built] == ["ddim", "dpmpp_2m"]              # the graph builds its sampler's denoiser
    k_ddim, k_dpm = sorted(stub_pipe._batch_graphs, key=str)
    assert [x for x, y in zip(k_ddim, k_dpm) if x != y] == ["ddim"]
    # the key still ends (masked, composite, t_start, init image, posterior eps), as the inpainting tests read it
    assert k_dpm[-5:] == (False, False, 0, False, False)
