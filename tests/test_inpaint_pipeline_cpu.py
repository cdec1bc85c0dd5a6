"""Inpainting end to end without a GPU: c2d_inpaint_prepare's validation through the C ABI (no launch), FakeTensor
tracing of ops.inpaint_prepare, the host-side mask preparation (pipeline.prepare_mask_array), the command line's new
flags, and the float64 restatement of the masked loop entered the way pure_noise enters it."""
import ctypes
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from clap2diffusion_amd import ops
from clap2diffusion_amd.pipeline import build_parser, prepare_mask_array
from clap2diffusion_amd.scheduler import DDIMScheduler
from oracle.ddim_ref import alphas_cumprod, timesteps
from tests.inpaint_ref import masked_loop

OK, E_ARG, E_SHAPE, E_ALIGN = 0, -1, -2, -3


# ------------------------------------------------------------------ entry point
@pytest.fixture(scope="module")
def L():
    from clap2diffusion_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def hostbuf():
    buf = ctypes.create_string_buffer(256)   # host memory: never dereferenced on these paths
    return buf, (ctypes.addressof(buf) + 15) & ~15


# moments, ld, eps, noise, mask_u8, coef, step_index, pure_noise, n, h, w, scaling, z0, x, mask, stream
MOM, LD, EPS, NOISE, MASK8, COEF, IDX, PURE, N, H, W, SCALE, Z0, X, MASK = range(15)


def good_args(p):
    return [p, 8, p, p, p, p, p, 0, 1, 8, 8, 0.18215, p, p, p, None]


def test_inpaint_prepare_is_exported_and_declared(L):
    from clap2diffusion_amd import _lib
    assert "c2d_inpaint_prepare" in _lib.EXPORTS
    assert hasattr(L, "c2d_inpaint_prepare")
    assert L.c2d_version().endswith(b"r7")                  # added to the r7 ABI: no struct changed


def test_inpaint_prepare_null_pointers(L, hostbuf):
    _, p = hostbuf
    f = L.c2d_inpaint_prepare
    for k in (MOM, NOISE, MASK8, Z0, X, MASK):
        for pure in (0, 1):
            args = good_args(p)
            args[k], args[PURE] = None, pure
            assert f(*args) == E_ARG, (k, pure)
    for k in (COEF, IDX):                                   # the table and the counter are read only to add noise
        args = good_args(p)
        args[k] = None
        assert f(*args) == E_ARG, k


def test_inpaint_prepare_shapes(L, hostbuf):
    _, p = hostbuf
    f = L.c2d_inpaint_prepare
    for k in (N, H, W):
        for bad in (0, -1):
            args = good_args(p)
            args[k] = bad
            assert f(*args) == E_SHAPE, (k, bad)
    for ld in (7, 0, -8):
        args = good_args(p)
        args[LD] = ld
        assert f(*args) == E_SHAPE, ld


def test_inpaint_prepare_alignment(L, hostbuf):
    _, p = hostbuf
    f = L.c2d_inpaint_prepare
    args = good_args(p)
    args[MOM] = p + 1                                       # fp16 rows: 2-byte aligned
    assert f(*args) == E_ALIGN
    for k in (EPS, NOISE, COEF, Z0, X, MASK):               # fp32: 4-byte aligned
        args = good_args(p)
        args[k] = p + 2
        assert f(*args) == E_ALIGN, k
    # validation order as in the neighbouring entry points: a null pointer before a shape before an alignment
    args = good_args(p)
    args[X], args[N] = None, 0
    assert f(*args) == E_ARG
    args = good_args(p)
    args[N], args[Z0] = 0, p + 2
    assert f(*args) == E_SHAPE


# ------------------------------------------------------------------ torch op
def test_fake_tracing_of_inpaint_prepare():
    with FakeTensorMode():
        dev = torch.device("cuda", 0)
        mom = torch.empty(2 * 8 * 16, 8, dtype=torch.float16, device=dev)
        noise = torch.empty(2, 4, 8, 16, device=dev)
        m8 = torch.empty(2, 64, 128, dtype=torch.uint8, device=dev)
        coef = torch.empty(4, 2, device=dev)
        idx = torch.empty(1, dtype=torch.int32, device=dev)
        z0, x, mask = ops.inpaint_prepare(mom, noise, m8, 0.18215, eps=torch.empty_like(noise), coef=coef, step_index=idx)
        assert z0.shape == x.shape == noise.shape and z0.dtype == x.dtype == torch.float32
        assert mask.shape == (2, 8, 16) and mask.dtype == torch.float32
        zz, xx, mm = torch.empty_like(noise), torch.empty_like(noise), torch.empty(2, 8, 16, device=dev)
        got = ops.inpaint_prepare(mom, noise, m8, 0.18215, pure_noise=True, z0=zz, x=xx, mask=mm)   # no table needed
        assert got[0] is zz and got[1] is xx and got[2] is mm
        strided = torch.empty(2 * 8 * 16, 16, dtype=torch.float16, device=dev)[:, :8]               # ld 16
        ops.inpaint_prepare(strided, noise, m8, 0.18215, pure_noise=True)
        with pytest.raises(AssertionError):                 # the mask is the image's size, 8 x the latents'
            ops.inpaint_prepare(mom, noise, torch.empty(2, 64, 64, dtype=torch.uint8, device=dev), 0.18215,
                                pure_noise=True)
        with pytest.raises(AssertionError):                 # not the latent-size mask either
            ops.inpaint_prepare(mom, noise, torch.empty(2, 8, 16, dtype=torch.uint8, device=dev), 0.18215,
                                pure_noise=True)
        with pytest.raises(AssertionError):                 # bytes, not floats
            ops.inpaint_prepare(mom, noise, m8.float(), 0.18215, pure_noise=True)
        with pytest.raises(AssertionError):                 # add_noise needs the table and the counter
            ops.inpaint_prepare(mom, noise, m8, 0.18215)
        with pytest.raises(AssertionError):                 # x must not be the noise
            ops.inpaint_prepare(mom, noise, m8, 0.18215, pure_noise=True, x=noise)
    schema = str(torch.ops.c2d.inpaint_prepare.default._schema)
    assert re.findall(r"Tensor\(a\d+!\) (\w+)", schema) == ["z0", "x", "mask"]
    from clap2diffusion_amd import torch_ops
    assert "inpaint_prepare" in torch_ops.OPS


# ------------------------------------------------------------------ prepare_mask_array
HGT, WID = 64, 64


@pytest.fixture(scope="module")
def mask64():
    m = np.zeros((HGT, WID), dtype=np.uint8)
    m[:, :36] = 255
    m[5, 50], m[6, 50], m[40, 3], m[41, 3] = 128, 127, 127, 128
    return m


def test_mask_forms_give_the_same_bytes(mask64, tmp_path):
    from PIL import Image
    ref = mask64[None]
    path = tmp_path / "mask.png"
    Image.fromarray(mask64).save(path)
    rgb = Image.fromarray(np.repeat(mask64[..., None], 3, axis=2))       # grey RGB: "L" gives the bytes back
    forms = [mask64, mask64[None], torch.from_numpy(mask64), torch.from_numpy(mask64)[None], Image.fromarray(mask64),
             rgb, path, str(path), [mask64], [Image.fromarray(mask64)], (torch.from_numpy(mask64),)]
    for f in forms:
        got = prepare_mask_array(f, HGT, WID)
        assert got.dtype == np.uint8 and got.shape == (1, HGT, WID) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, ref), type(f)
    b = mask64 >= 128
    for f in (b, torch.from_numpy(b), [b]):
        got = prepare_mask_array(f, HGT, WID)
        assert got.dtype == np.uint8 and np.array_equal(got, np.where(b, 255, 0)[None].astype(np.uint8))


def test_mask_threshold_bytes_survive(mask64):
    got = prepare_mask_array(mask64, HGT, WID)[0]
    assert (got[5, 50], got[6, 50], got[40, 3], got[41, 3]) == (128, 127, 127, 128)
    assert np.array_equal(got >= 128, mask64 >= 128)


def test_mask_nearest_resize_keeps_two_values():
    small = np.zeros((32, 32), dtype=np.uint8)
    small[3:20, 7:29] = 255
    got = prepare_mask_array(small, HGT, WID)
    assert got.shape == (1, HGT, WID) and set(np.unique(got)) == {0, 255}
    assert np.array_equal(got[0], np.repeat(np.repeat(small, 2, axis=0), 2, axis=1))   # nearest at an exact factor
    odd = np.zeros((50, 37), dtype=np.uint8)
    odd[10:, :20] = 255
    got = prepare_mask_array([odd, small], HGT, WID)
    assert got.shape == (2, HGT, WID) and set(np.unique(got)) == {0, 255}
    tall = prepare_mask_array(small, 128, 64)                # height and width are not swapped
    assert tall.shape == (1, 128, 64)


def test_mask_broadcast_and_counts(mask64):
    got = prepare_mask_array(mask64, HGT, WID, n=3)
    assert got.shape == (3, HGT, WID) and all(np.array_equal(g, mask64) for g in got) and got.flags["C_CONTIGUOUS"]
    two = np.stack([mask64, 255 - mask64])
    assert np.array_equal(prepare_mask_array(two, HGT, WID, n=2), two)
    assert np.array_equal(prepare_mask_array([mask64, 255 - mask64], HGT, WID, n=2), two)
    assert np.array_equal(prepare_mask_array(two, HGT, WID), two)
    with pytest.raises(ValueError):
        prepare_mask_array(two, HGT, WID, n=3)
    with pytest.raises(ValueError):
        prepare_mask_array([mask64, mask64, mask64], HGT, WID, n=2)
    with pytest.raises(ValueError):
        prepare_mask_array([], HGT, WID)


@pytest.mark.parametrize("bad", [
    np.zeros((HGT, WID), dtype=np.float32), np.zeros((HGT, WID), dtype=np.int64), torch.zeros(HGT, WID),
    torch.zeros(HGT, WID, dtype=torch.int32), np.zeros((HGT,), dtype=np.uint8), np.zeros((1, 1, HGT, WID), dtype=np.uint8),
    torch.zeros(1, 1, HGT, WID, dtype=torch.uint8), 3, None,
], ids=["f32", "i64", "torch_f32", "torch_i32", "rank1", "rank4", "torch_rank4", "int", "none"])
def test_mask_wrong_dtype_or_rank(bad):
    with pytest.raises(ValueError):
        prepare_mask_array(bad, HGT, WID)
    with pytest.raises(ValueError):
        prepare_mask_array([bad], HGT, WID)


# ------------------------------------------------------------------ command line
def test_parser_has_the_inpainting_flags():
    ap = build_parser()
    a = ap.parse_args(["--audio", "synthetic:0"])
    assert a.mask is None and a.no_composite is False       # the defaults: no inpainting, as before
    assert a.init_image is None and a.strength == 0.8 and a.steps == 50 and a.cfg_scale == 7.5 and a.seed is None
    a = ap.parse_args(["--audio", "x.wav", "--init_image", "i.png", "--mask", "m.png", "--no_composite"])
    assert a.mask == "m.png" and a.no_composite is True and a.init_image == "i.png"


# ------------------------------------------------------------------ float64 restatement
STEPS = 4


def fake_eps(x, t):
    g = torch.Generator().manual_seed(t)
    return torch.randn(x.shape, generator=g, dtype=torch.float64) + 0.1 * x


def test_pure_noise_start_is_the_loop_fed_the_noise():
    """strength 1: t_start is 0 and c2d_inpaint_prepare's pure_noise start is x = noise (init_noise_sigma = 1),
    whatever z0 is; below strength 1 the start is add_noise(z0, noise, timesteps[t_start]), another tensor."""
    assert DDIMScheduler.img2img_start(STEPS, 1.0) == 0 and DDIMScheduler().init_noise_sigma == 1.0
    g = torch.Generator().manual_seed(4)
    z0, noise = (torch.randn(2, 4, 5, 7, generator=g) for _ in range(2))
    m = torch.zeros(2, 5, 7)
    m[:, :, :3] = 1

    def start(t_start, pure_noise):   # c2d_inpaint_prepare's x, restated
        if pure_noise:
            return noise.clone()
        a = alphas_cumprod().double()[int(timesteps(STEPS)[t_start])]
        return a.sqrt() * z0.double() + (1 - a).sqrt() * noise.double()

    got = masked_loop(fake_eps, start(0, True), z0, noise, m, STEPS, 0)
    assert torch.equal(got, masked_loop(fake_eps, noise, z0, noise, m, STEPS, 0))
    assert torch.equal(got[..., 3:], z0.double()[..., 3:])               # the kept region still ends at the original
    noised = masked_loop(fake_eps, start(0, False), z0, noise, m, STEPS, 0)
    assert not torch.allclose(noised[..., :3], got[..., :3])             # add_noise at timesteps[0] is not pure noise
    t_start = DDIMScheduler.img2img_start(STEPS, 0.5)
    assert t_start == 2
    part = masked_loop(fake_eps, start(t_start, False), z0, noise, m, STEPS, t_start)
    assert torch.equal(part[..., 3:], z0.double()[..., 3:]) and not torch.allclose(part[..., :3], got[..., :3])
