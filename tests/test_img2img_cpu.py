"""Audio-guided img2img without a GPU: the strength rule, the encoder's checkpoint keys, the pad-after conv
mode's descriptor validation and plans through the C ABI (no launch), and FakeTensor tracing of the new ops."""
import ctypes

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from clap2diffusion_amd import ops, weights as W
from clap2diffusion_amd.scheduler import DDIMScheduler
from tests.vae_encoder_ref import VAEEncoderRef

E_ARG, E_SHAPE = -1, -2


# ------------------------------------------------------------------ scheduler
@pytest.mark.parametrize("steps,strength,t_start", [(50, 0.8, 10), (50, 1.0, 0), (10, 0.35, 7)])
def test_img2img_start(steps, strength, t_start):
    assert DDIMScheduler.img2img_start(steps, strength) == t_start


def test_img2img_start_timestep():
    s = DDIMScheduler()
    s.set_timesteps(50)
    assert int(s.timesteps[DDIMScheduler.img2img_start(50, 0.8)]) == 781


@pytest.mark.parametrize("strength", [0.0, 0.01, 1.2])
def test_img2img_start_rejects(strength):
    with pytest.raises(ValueError):
        DDIMScheduler.img2img_start(50, strength)


# ------------------------------------------------------------------ weights
def test_encoder_keys_match_reference_module():
    ref = {k: tuple(v.shape) for k, v in VAEEncoderRef().state_dict().items()}
    assert dict(W.vae_encoder_param_shapes()) == ref
    sd = W.synth_vae_encoder(3)
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref
    assert not torch.equal(sd["encoder.conv_in.weight"], W.synth_vae_encoder(4)["encoder.conv_in.weight"])


def test_state_dict_halves():
    dec, enc = W.synth_vae_decoder(1), W.synth_vae_encoder(1)
    merged = {**enc, **dec}
    got_e = W.vae_encoder_state_dict(merged)
    assert set(got_e) == set(enc) and all(torch.equal(got_e[k], enc[k]) for k in enc)
    got_d = W.vae_state_dict(merged)
    assert set(got_d) == set(dec) and all(torch.equal(got_d[k], dec[k]) for k in dec)
    assert W.vae_state_dict is W.vae_decoder_state_dict
    with pytest.raises(KeyError):
        W.vae_encoder_state_dict(dec)
    # the pre-0.14 attention names of the SD1.5 vae/ files
    old = {k.replace("to_q", "query"): (v[:, :, None, None] if "to_q.weight" in k else v) for k, v in enc.items()}
    back = W.vae_encoder_state_dict(old)
    assert set(back) == set(enc) and back["encoder.mid_block.attentions.0.to_q.weight"].dim() == 2


# ------------------------------------------------------------------ descriptor / planner
@pytest.fixture(scope="module")
def L():
    from clap2diffusion_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def hostbuf():
    buf = ctypes.create_string_buffer(256)   # host memory: never dereferenced on these paths
    return buf, (ctypes.addressof(buf) + 15) & ~15


def down_desc(addr, n=2, h=16, w=16, cin=128, cout=128, pad_mode=1):
    from clap2diffusion_amd import _lib
    d = _lib.ConvDesc()
    d.src0, d.weight, d.out = addr, addr, addr
    d.c0, d.n, d.h, d.w, d.oh, d.ow = cin, n, h, w, h // 2, w // 2
    d.ksize, d.stride = 3, 2
    d.cout, d.kpad, d.out_ld = cout, ops.kpad_of(9 * cin), cout
    d.pad_mode = pad_mode
    return d


def plan(L, d):
    tid, ks = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.c2d_conv2d_igemm_plan(ctypes.byref(d), ctypes.byref(tid), ctypes.byref(ks))
    return rc, tid.value, ks.value


BAD = [
    ("stride=1", lambda d, a: (setattr(d, "stride", 1), setattr(d, "oh", d.h), setattr(d, "ow", d.w)), E_SHAPE),
    ("up=1", lambda d, a: setattr(d, "up", 1), E_SHAPE),
    ("src_pad=1", lambda d, a: setattr(d, "src_pad", 1), E_SHAPE),
    ("odd h", lambda d, a: (setattr(d, "h", 15), setattr(d, "oh", 8)), E_SHAPE),
    ("odd w", lambda d, a: (setattr(d, "w", 15), setattr(d, "ow", 8)), E_SHAPE),
    ("oh != h/2", lambda d, a: setattr(d, "oh", d.h // 2 + 1), E_SHAPE),
    ("ksize=1", lambda d, a: setattr(d, "ksize", 1), E_SHAPE),
    ("pad_mode=2", lambda d, a: setattr(d, "pad_mode", 2), E_ARG),
    ("pad_mode=-1", lambda d, a: setattr(d, "pad_mode", -1), E_ARG),
]


@pytest.mark.parametrize("name,mutate,code", BAD, ids=[b[0] for b in BAD])
def test_pad_mode_validation(L, hostbuf, name, mutate, code):
    """The documented code from the launch entry point (before any HIP call) and the plan query alike; the
    workspace and gn_rows queries answer 0."""
    _, addr = hostbuf
    d = down_desc(addr)
    mutate(d, addr)
    assert L.c2d_conv2d_igemm(ctypes.byref(d), None) == code
    assert plan(L, d)[0] == code
    assert L.c2d_conv2d_igemm_workspace_size(ctypes.byref(d)) == 0
    d.gn_groups = 32
    assert L.c2d_conv2d_gn_rows(ctypes.byref(d)) == 0


NOT_FOR_THE_MODE = (42, 43, 44, 50, 70)   # row ring (src_pad only), persistent and panel GEMM (1x1 only)


@pytest.mark.parametrize("n", [1, 8])
@pytest.mark.parametrize("hw,c", [(512, 128), (256, 256), (128, 512)])
def test_encoder_downsample_plans(L, hostbuf, n, hw, c):
    _, addr = hostbuf
    d = down_desc(addr, n, hw, hw, c, c)
    rc, tid, ks = plan(L, d)
    assert rc == 0 and tid not in NOT_FOR_THE_MODE and tid != 0 and ks == 1, (tid, ks)
    # the mode plans exactly as the pad-1 stride-2 conv of the same shape
    assert plan(L, down_desc(addr, n, hw, hw, c, c, pad_mode=0)) == (rc, tid, ks)
    for forced in NOT_FOR_THE_MODE:   # a forced plan naming a tile without the mode is ignored
        L.c2d_set_plan_override(forced, 0)
        try:
            assert plan(L, d) == (rc, tid, ks), forced
        finally:
            L.c2d_set_plan_override(0, 0)


def test_zeroed_pad_mode_keeps_the_stride2_plan(L, hostbuf):
    """The UNet's level-0 downsampler at the c3 batch (16 x 64^2, 320 -> 320, stride 2): tile 7, one slice, the
    answer of the library before the field existed; and a split-K plan answers the same workspace in both modes."""
    _, addr = hostbuf
    d = down_desc(addr, 16, 64, 64, 320, 320, pad_mode=0)
    assert plan(L, d) == (0, 7, 1)
    L.c2d_set_plan_override(7, 2)
    try:
        d0, d1 = down_desc(addr, 2, 16, 16, 1280, 1280, pad_mode=0), down_desc(addr, 2, 16, 16, 1280, 1280)
        need = L.c2d_conv2d_igemm_workspace_size(ctypes.byref(d1))
        assert need == 2 * (2 * 8 * 8) * 1280 * 4 == L.c2d_conv2d_igemm_workspace_size(ctypes.byref(d0))
        assert plan(L, d1) == (0, 7, 1)
        d1.ws, d1.ws_bytes = addr, need
        assert plan(L, d1) == (0, 7, 2)
    finally:
        L.c2d_set_plan_override(0, 0)


def test_new_entry_points_validate(L, hostbuf):
    _, addr = hostbuf
    assert L.c2d_image_to_nhwc(None, 1, 4, addr, None) == E_ARG
    assert L.c2d_image_to_nhwc(addr, 0, 4, addr, None) == E_SHAPE
    assert L.c2d_image_to_nhwc(addr, 1, 4, addr + 8, None) == -3
    assert L.c2d_vae_posterior_noise(None, 8, None, None, None, None, 1, 4, 1.0, addr, None) == E_ARG
    assert L.c2d_vae_posterior_noise(addr, 8, None, addr, None, None, 1, 4, 1.0, addr, None) == E_ARG   # noise, no coef
    assert L.c2d_vae_posterior_noise(addr, 4, None, None, None, None, 1, 4, 1.0, addr, None) == E_SHAPE
    assert L.c2d_version().endswith(b"r7")


# ------------------------------------------------------------------ torch ops
def test_fake_tracing_of_the_img2img_ops():
    with FakeTensorMode():
        dev = torch.device("cuda", 0)
        img = torch.empty(2, 64, 128, 3, dtype=torch.uint8, device=dev)
        x = ops.image_to_nhwc(img)
        assert x.shape == (2, 64, 128, 8) and x.dtype == torch.float16
        a = torch.empty(2, 64, 128, 128, dtype=torch.float16, device=dev)
        w = torch.empty(128, 1152, dtype=torch.float16, device=dev)
        y = ops.conv(a, w, 1152, 128, ksize=3, stride=2, bias=torch.empty(128, device=dev), pad_after=True)
        assert y.shape == (2, 32, 64, 128) and y.dtype == torch.float16
        mom = torch.empty(2 * 8 * 16, 8, dtype=torch.float16, device=dev)
        lat = torch.empty(2, 4, 8, 16, device=dev)
        z = ops.vae_posterior_noise(mom, torch.empty_like(lat), 0.18215, eps=lat, noise=lat,
                                    coef=torch.empty(5, 2, device=dev),
                                    step_index=torch.empty(1, dtype=torch.int32, device=dev))
        assert z.shape == lat.shape and z.dtype == torch.float32
    for name in ("image_to_nhwc", "vae_posterior_noise"):
        assert "Tensor(a" in str(getattr(torch.ops.c2d, name).default._schema)
    assert "bool pad_after=False" in str(torch.ops.c2d.conv2d_igemm.default._schema)


def test_pad_after_rejects_odd_sizes_on_the_host():
    with FakeTensorMode():
        dev = torch.device("cuda", 0)
        a = torch.empty(1, 7, 8, 128, dtype=torch.float16, device=dev)
        with pytest.raises(AssertionError):
            ops.conv(a, torch.empty(128, 1152, dtype=torch.float16, device=dev), 1152, 128, ksize=3, stride=2,
                     pad_after=True)
