"""The inpainting kernels without a GPU: the scheduler identity the masked step kernel leans on, the new entry
points' validation through the C ABI (no launch), FakeTensor tracing of the new ops, the byte threshold against
diffusers' rule, and the float64 restatement of the masked loop (tests/inpaint_ref.py) at its two ends."""
import ctypes
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from clap2diffusion_amd import ops
from clap2diffusion_amd.scheduler import DDIMScheduler
from oracle.ddim_ref import alphas_cumprod, ddim_step, timesteps
from tests.inpaint_ref import latent_mask, masked_loop

OK, E_ARG, E_SHAPE, E_ALIGN = 0, -1, -2, -3


# ------------------------------------------------------------------ scheduler
@pytest.mark.parametrize("steps", [1, 4, 20, 50, 1000])
def test_alpha_prev_is_the_next_steps_alpha(steps):
    """coef[i][1] == coef[i + 1][0]: under the leading spacing a step's previous timestep is the next step's
    timestep, so c2d_cfg_ddim_step_masked noises the known region to timesteps[i + 1] with this step's alpha_prev
    and never reads row i + 1.  With 1000 steps timesteps[0] is 1000, which has no alpha_t (in diffusers as here),
    so device_tables cannot build a table and the kernel cannot run: that case asserts the timestep identity,
    which is what makes the alphas equal, and that the table is indeed refused."""
    s = DDIMScheduler()
    s.set_timesteps(steps)
    ts = [int(t) for t in s.timesteps]
    ratio = s.num_train_timesteps // steps
    assert all(ts[i] - ratio == ts[i + 1] for i in range(steps - 1))
    if ts[0] >= s.num_train_timesteps:
        assert steps == 1000 and ts[0] == 1000
        with pytest.raises(IndexError):
            s.device_tables("cpu")
        return
    coef = s.device_tables("cpu")[1]
    assert coef.shape == (steps, 2)
    assert torch.equal(coef[:-1, 1], coef[1:, 0])
    for i in range(steps - 1):                      # and it is add_noise's alpha at timesteps[i + 1]
        assert float(coef[i, 1]) == float(s.alphas_cumprod[ts[i + 1]])


# ------------------------------------------------------------------ entry points
@pytest.fixture(scope="module")
def L():
    from clap2diffusion_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def hostbuf():
    buf = ctypes.create_string_buffer(256)   # host memory: never dereferenced on these paths
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_cfg_ddim_step_masked_validates(L, hostbuf):
    _, p = hostbuf
    f = L.c2d_cfg_ddim_step_masked
    good = [p, p, p, p, p, 1, 64, 4, 7.5, p, p, 1, None]   # eps, x, z0, noise, mask, b, hw, steps, g, coef, idx
    for k in (0, 1, 2, 3, 4, 9, 10):
        args = list(good)
        args[k] = None
        assert f(*args) == E_ARG, k
    for k in (5, 6, 7):
        for bad in (0, -1):
            args = list(good)
            args[k] = bad
            assert f(*args) == E_SHAPE, (k, bad)
    args = list(good)
    args[0] = p + 4                                         # eps is read in 8-byte pixels
    assert f(*args) == E_ALIGN
    for k in (1, 2, 3, 4):
        args = list(good)
        args[k] = p + 2
        assert f(*args) == E_ALIGN, k


def test_mask_to_latent_and_composite_validate(L, hostbuf):
    _, p = hostbuf
    f = L.c2d_mask_to_latent
    assert f(None, 1, 8, 8, p, None) == E_ARG
    assert f(p, 1, 8, 8, None, None) == E_ARG
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, -8, 8), (1, 8, -8)):
        assert f(p, n, h, w, p, None) == E_SHAPE, (n, h, w)
    assert f(p + 1, 1, 8, 8, p + 2, None) == E_ALIGN       # the byte mask may sit anywhere, the fp32 output not
    g = L.c2d_composite_u8
    for k in (0, 1, 2, 4):
        args = [p + 1, p + 2, p + 3, 16, p + 1, None]       # bytes: no alignment asked
        args[k] = None
        assert g(*args) == E_ARG, k
    assert g(p, p, p, 0, p, None) == E_SHAPE
    assert g(p, p, p, ctypes.c_size_t(-1).value, p, None) == E_SHAPE
    assert g(p, p, p, 2 ** 31, p, None) == E_SHAPE
    assert L.c2d_version().endswith(b"r7")                  # added to the r7 ABI: no struct changed


# ------------------------------------------------------------------ torch ops
def test_fake_tracing_of_the_inpaint_ops():
    with FakeTensorMode():
        dev = torch.device("cuda", 0)
        x = torch.empty(2, 4, 8, 16, device=dev)
        eps = torch.empty(4, 8, 16, 4, dtype=torch.float16, device=dev)
        mask = torch.empty(2, 8, 16, device=dev)
        idx = torch.empty(1, dtype=torch.int32, device=dev)
        y = ops.cfg_ddim_step_masked(eps, x, torch.empty_like(x), torch.empty_like(x), mask, 7.5,
                                     torch.empty(4, 2, device=dev), idx)
        assert y is x
        with pytest.raises(AssertionError):                 # one mask value per latent pixel, not per channel
            ops.cfg_ddim_step_masked(eps, x, torch.empty_like(x), torch.empty_like(x), torch.empty_like(x), 7.5,
                                     torch.empty(4, 2, device=dev), idx)
        m8 = torch.empty(2, 64, 128, dtype=torch.uint8, device=dev)
        ml = ops.mask_to_latent(m8)
        assert ml.shape == (2, 8, 16) and ml.dtype == torch.float32
        with pytest.raises(AssertionError):
            ops.mask_to_latent(torch.empty(2, 60, 128, dtype=torch.uint8, device=dev))
        img = torch.empty(2, 64, 128, 3, dtype=torch.uint8, device=dev)
        out = ops.composite_u8(img, torch.empty_like(img), m8)
        assert out.shape == img.shape and out.dtype == torch.uint8
        assert ops.composite_u8(img, torch.empty_like(img), m8, out=img) is img
        with pytest.raises(AssertionError):
            ops.composite_u8(img, torch.empty_like(img), m8.float())
    # the schemas name the mutated arguments, and only those
    mutated = {n: re.findall(r"Tensor\(a\d+!\) (\w+)", str(getattr(torch.ops.c2d, n).default._schema))
               for n in ("cfg_ddim_step_masked", "mask_to_latent", "composite_u8")}
    assert mutated == {"cfg_ddim_step_masked": ["x", "step_index"], "mask_to_latent": ["out"],
                       "composite_u8": ["out"]}


def test_byte_threshold_is_diffusers_rule():
    """The kernels repaint where the mask byte is >= 128: for every byte that is diffusers' mask / 255 >= 0.5."""
    u = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(u >= 128, u.float() / 255 >= 0.5)
    assert not bool(u[127].float() / 255 >= 0.5) and bool(u[128].float() / 255 >= 0.5)
    assert torch.equal(latent_mask(u.view(1, 16, 16), 16, 16).flatten(), (u >= 128).float())
    big = u.view(1, 16, 16).repeat_interleave(8, 1).repeat_interleave(8, 2)   # 128 x 128 -> 16 x 16: the (8y, 8x) sample
    big[:, 1::8, 1::8] = 255 - big[:, 1::8, 1::8]
    assert torch.equal(latent_mask(big, 16, 16).flatten(), (u >= 128).float())


# ------------------------------------------------------------------ float64 restatement
STEPS = 4


def fake_eps(x, t):
    """A deterministic stand-in for the guided UNet output: depends on the latents and the timestep."""
    g = torch.Generator().manual_seed(t)
    return torch.randn(x.shape, generator=g, dtype=torch.float64) + 0.1 * x


@pytest.fixture(scope="module")
def loop_inputs():
    g = torch.Generator().manual_seed(2)
    return tuple(torch.randn(2, 4, 5, 7, generator=g) for _ in range(3))   # start, z0, noise


@pytest.mark.parametrize("start", [0, 2])
def test_masked_loop_with_ones_is_the_ddim_loop(loop_inputs, start):
    x, z0, noise = loop_inputs
    got = masked_loop(fake_eps, x, z0, noise, torch.ones(2, 5, 7), STEPS, start)
    ac, ref = alphas_cumprod().double(), x.double()
    for t in timesteps(STEPS)[start:]:
        ref = ddim_step(fake_eps(ref, int(t)), int(t), ref, STEPS, ac)
    assert got.dtype == torch.float64 and torch.equal(got, ref)


@pytest.mark.parametrize("start", [0, 2, 3])
def test_masked_loop_with_zeros_ends_at_the_original(loop_inputs, start):
    x, z0, noise = loop_inputs
    got = masked_loop(fake_eps, x, z0, noise, torch.zeros(2, 5, 7), STEPS, start)
    assert torch.equal(got, z0.double())


def test_masked_loop_blends_per_pixel(loop_inputs):
    """A half mask: the kept half ends at z0, the other half is not the unmasked run's (the kept latents fed the
    stand-in's x term on the way) but stays finite and differs from z0."""
    x, z0, noise = loop_inputs
    m = torch.zeros(2, 5, 7)
    m[:, :, :3] = 1
    got = masked_loop(fake_eps, x, z0, noise, m, STEPS)
    assert torch.equal(got[..., 3:], z0.double()[..., 3:])
    assert torch.isfinite(got).all() and not torch.allclose(got[..., :3], z0.double()[..., :3])
    # one step before the end the kept half is z0 noised to the last timestep
    ac, ts = alphas_cumprod().double(), timesteps(STEPS)
    seen = {}

    def spy(xx, t):
        seen[t] = xx.clone()
        return fake_eps(xx, t)
    masked_loop(spy, x, z0, noise, m, STEPS)
    a = ac[int(ts[-1])]
    assert torch.equal(seen[int(ts[-1])][..., 3:], (a ** 0.5 * z0.double() + (1 - a) ** 0.5 * noise.double())[..., 3:])
