"""The inpainting kernels on the GPU: c2d_cfg_ddim_step_masked against c2d_cfg_ddim_step and the float64
restatement of tests/inpaint_ref.py, c2d_mask_to_latent against F.interpolate, c2d_composite_u8 against torch.where.

Bars.  Masked step: bit-identical to c2d_cfg_ddim_step where the mask is 1; where it is 0 bit-identical to z0 at
the last step and rtol 1e-5 / atol 1e-6 against the fp32 add_noise formula otherwise (the bar of
test_img2img_gpu.py::test_vae_posterior_noise for the same formula).  Over the whole tensor, fractional mask
values included, against the float64 restatement evaluated from the fp16-rounded eps: max-abs error <= 3 E, E the
max-abs error of the same formula evaluated by torch in fp32 on the CPU on the same inputs (the multiple
tests/htsat_parity.py uses), and never below test_kernels_gpu.py::test_cfg_ddim's tol_max = 1e-5, taken here as
an absolute error (stricter than that test's relative one: the references reach 50).  mask_to_latent,
composite_u8: bit-exact."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clap2diffusion_amd import ops
from clap2diffusion_amd.scheduler import DDIMScheduler
from tests import parity_log
from tests.inpaint_ref import latent_mask, masked_step
from tests.test_kernels_gpu import gen, nhwc

pytestmark = pytest.mark.gpu

STEPS, GUIDANCE = 4, 7.5
PAD, SENTINEL = 1024, -1234.0


def guarded(shape, dtype, dev, fill=SENTINEL):
    """(buffer, view of `shape` in its middle): PAD sentinel elements on either side."""
    n = int(np.prod(shape))
    buf = torch.full((PAD + n + PAD,), fill, dtype=dtype, device=dev)
    return buf, buf[PAD:PAD + n].view(shape)


def guards_intact(buf, fill=SENTINEL):
    return bool((buf[:PAD] == fill).all()) and bool((buf[-PAD:] == fill).all())


# ------------------------------------------------------------------ masked step
SHAPES = {1: (1, 1), 63: (7, 9), 64: (8, 8), 1000: (25, 40)}   # hw -> (h, w): below, at and above one 256-thread block
MASK_VALUES = torch.tensor([1.0, 0.0, 0.25, 0.5])


@functools.lru_cache(maxsize=None)
def coef_table():
    s = DDIMScheduler()
    s.set_timesteps(STEPS)
    return s.device_tables("cpu")[1]


@functools.lru_cache(maxsize=None)
def step_case(b, hw):
    """(x, z0, noise NCHW fp32, eps NHWC fp16 [2b]) of one shape, computed once, never written."""
    h, w = SHAPES[hw]
    x, z0, noise = (gen(b, 4, h, w, seed=50 + k + hw) for k in range(3))
    return x, z0, noise, nhwc(gen(2 * b, 4, h, w, seed=53 + hw)).half()


@functools.lru_cache(maxsize=None)
def plain_step(b, hw, st):
    """c2d_cfg_ddim_step (the parent's kernel, tested in test_kernels_gpu.py) on the case's inputs."""
    x, _, _, eps = step_case(b, hw)
    dev = torch.device("cuda:0")
    xd = x.to(dev)
    ops.cfg_ddim_step(eps.to(dev), xd, GUIDANCE, coef_table().to(dev), torch.tensor([st], dtype=torch.int32, device=dev),
                      advance=False)
    return xd.cpu()


@pytest.mark.parametrize("advance", [True, False])
@pytest.mark.parametrize("st", [0, 2, STEPS - 1])
@pytest.mark.parametrize("hw", sorted(SHAPES))
@pytest.mark.parametrize("b", [1, 3])
def test_cfg_ddim_step_masked(dev, b, hw, st, advance):
    """Measured on an MI355X (E / GPU error / bar), b = 3, hw = 1000: step 0 7.7e-6 / 1.5e-5 / 2.3e-5 (the case
    nearest its bar, 0.63 of it), step 2 3.3e-6 / 3.3e-6 / 1e-5, step 3 3.4e-7 / 3.9e-7 / 1e-5; every case is in
    the parity log."""
    x, z0, noise, eps = step_case(b, hw)
    h, w = SHAPES[hw]
    coef = coef_table()
    plain = plain_step(b, hw, st)
    a_p = coef[st, 1]
    known = z0 if st == STEPS - 1 else a_p.sqrt() * z0 + (1 - a_p).sqrt() * noise
    for shift in (range(4) if b * hw < 4 else (0,)):       # every mask value reaches the smallest cases too
        mask = MASK_VALUES[(torch.arange(b * hw) + shift) % 4].view(b, h, w)
        buf, xd = guarded((b, 4, h, w), torch.float32, dev)
        xd.copy_(x)
        z0d, nd, md = z0.to(dev), noise.to(dev), mask.to(dev)
        idx = torch.tensor([st], dtype=torch.int32, device=dev)
        out = ops.cfg_ddim_step_masked(eps.to(dev), xd, z0d, nd, md, GUIDANCE, coef.to(dev), idx, advance=advance)
        assert out.data_ptr() == xd.data_ptr()
        assert idx.item() == st + int(advance)
        assert guards_intact(buf)
        assert torch.equal(z0d.cpu(), z0) and torch.equal(nd.cpu(), noise) and torch.equal(md.cpu(), mask)
        got = xd.cpu()
        m4 = mask[:, None].expand_as(got)
        assert torch.equal(got[m4 == 1], plain[m4 == 1])
        if st == STEPS - 1:
            assert torch.equal(got[m4 == 0], z0[m4 == 0])
        else:
            assert torch.allclose(got[m4 == 0], known[m4 == 0], rtol=1e-5, atol=1e-6)
        ref = masked_step(eps, x, z0, noise, mask, GUIDANCE, coef, st)
        e_cpu = (masked_step(eps, x, z0, noise, mask, GUIDANCE, coef, st, dtype=torch.float32).double() - ref).abs().max().item()
        err = (got.double() - ref).abs().max().item()
        bar = max(3.0 * e_cpu, 1e-5)
        parity_log.record(max_abs=err, cpu_fp32_max_abs=e_cpu, bar=bar, ref_max=ref.abs().max().item())
        print(f"b={b} hw={hw} st={st} shift={shift}: E={e_cpu:.3e} gpu={err:.3e} bar={bar:.3e}")
        assert err <= bar, (err, e_cpu, bar)


def test_cfg_ddim_step_masked_steps_differ(dev):
    """The known region follows the counter: another step, another noise level; the last step, none."""
    x, z0, noise, eps = step_case(3, 64)
    outs = []
    for st in (0, 2, STEPS - 1):
        xd = x.to(dev)
        ops.cfg_ddim_step_masked(eps.to(dev), xd, z0.to(dev), noise.to(dev), torch.zeros(3, 8, 8, device=dev), GUIDANCE,
                                 coef_table().to(dev), torch.tensor([st], dtype=torch.int32, device=dev))
        outs.append(xd.cpu())
    assert not torch.allclose(outs[0], outs[1], atol=1e-2) and not torch.allclose(outs[1], outs[2], atol=1e-2)


# ------------------------------------------------------------------ mask_to_latent / composite_u8
BYTES = torch.tensor([0, 127, 128, 255], dtype=torch.uint8)


@pytest.mark.parametrize("h,w", [(64, 64), (64, 128)])
def test_mask_to_latent(dev, h, w):
    g = torch.Generator().manual_seed(h + w)
    m = BYTES[torch.randint(0, 4, (2, h, w), generator=g)]
    ref = F.interpolate((m.float() / 255 >= 0.5).float()[:, None], size=(h // 8, w // 8))[:, 0]
    assert torch.equal(ref, latent_mask(m, h // 8, w // 8))
    assert {int(v) for v in m[:, ::8, ::8].unique()} == {0, 127, 128, 255} and 0 < ref.mean() < 1
    buf, out = guarded((2, h // 8, w // 8), torch.float32, dev)
    assert ops.mask_to_latent(m.to(dev), out=out).data_ptr() == out.data_ptr()
    assert guards_intact(buf)
    assert torch.equal(out.cpu(), ref)
    assert torch.equal(ops.mask_to_latent(m.to(dev)).cpu(), ref)


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("npix", [1, 255, 4096 + 3])
def test_composite_u8(dev, npix, alias):
    g = torch.Generator().manual_seed(npix)
    dec = torch.randint(0, 256, (1, 1, npix, 3), generator=g, dtype=torch.uint8)
    orig = torch.randint(0, 256, (1, 1, npix, 3), generator=g, dtype=torch.uint8)
    mask = BYTES[(torch.arange(npix) + 1) % 4].view(1, 1, npix)         # 127 first: one pixel is a kept one
    ref = torch.where((mask >= 128)[..., None], dec, orig)
    buf, slot = guarded((1, 1, npix, 3), torch.uint8, dev, fill=77)
    origd, maskd = orig.to(dev), mask.to(dev)
    if alias:
        slot.copy_(dec)
        out = ops.composite_u8(slot, origd, maskd, out=slot)
    else:
        decd = dec.to(dev)
        out = ops.composite_u8(decd, origd, maskd, out=slot)
        assert torch.equal(decd.cpu(), dec)
    assert out.data_ptr() == slot.data_ptr() and guards_intact(buf, fill=77)
    assert torch.equal(slot.cpu(), ref)
    assert torch.equal(origd.cpu(), orig) and torch.equal(maskd.cpu(), mask)
    if not alias:
        assert torch.equal(ops.composite_u8(dec.to(dev), origd, maskd).cpu(), ref)
