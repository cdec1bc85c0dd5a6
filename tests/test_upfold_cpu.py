"""The folded upsample (c2d_conv_desc::up = 2: nearest x2 + 3x3 as four 2x2 phase convs of the low-res image)
without a GPU: the weight-fold algebra, the pack layout, the descriptor validation through the C ABI, the plan /
workspace queries and the planner's routes."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from clap2diffusion_amd import ops

E_ARG, E_SHAPE = -1, -2


def phase_convs(x, wf, bias, cin):
    """Four torch 2x2 convs of the low-res x with the folded pack wf [4][cout][4 cin] -> [n, cout, 2h, 2w]."""
    n, _, h, w = x.shape
    cout = wf.shape[1]
    out = x.new_zeros(n, cout, 2 * h, 2 * w)
    xp = F.pad(x, (1, 1, 1, 1))   # xp[i + 1, j + 1] = x[i, j]: tap (ty, tx) of phase (a, b) reads xp[i + a + ty, j + b + tx]
    for a in range(2):
        for b in range(2):
            k = wf[2 * a + b].reshape(cout, 2, 2, cin).permute(0, 3, 1, 2)   # K order (ty, tx, cin) -> [co, ci, ty, tx]
            y = F.conv2d(xp, k, bias)   # [n, cout, h + 1, w + 1]
            out[:, :, a::2, b::2] = y[:, :, a:a + h, b:b + w]
    return out


def test_fold_algebra_float64_non_square():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 5, 3, 4, generator=g, dtype=torch.float64)
    w = torch.randn(7, 5, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(7, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
    wf, kpad = ops.fold_upsample_weight(w, dtype=torch.float64)
    assert kpad == 20
    got = phase_convs(x, wf, b, 5)
    assert torch.allclose(got, ref, rtol=0.0, atol=1e-10), (got - ref).abs().max().item()


def test_pack_layout():
    cout, cin = 3, 64
    w = torch.arange(cout * cin * 9, dtype=torch.float32).reshape(cout, cin, 3, 3) / 4096.0
    wf, kpad = ops.fold_upsample_weight(w)
    assert wf.dtype == torch.float16 and tuple(wf.shape) == (4, cout, 4 * cin) and kpad == 4 * cin
    assert wf.is_contiguous()
    v = wf.float().reshape(4, cout, 2, 2, cin)   # [phase 2a + b][co][ty][tx][ci]
    # phase (0, 0): tap (0, 0) is the 3x3's corner (0, 0) alone; tap (1, 1) sums the 2x2 block of taps {1, 2}^2
    assert torch.equal(v[0, :, 0, 0, :], w[:, :, 0, 0].half().float())
    assert torch.equal(v[0, :, 1, 1, :], (w[:, :, 1, 1] + w[:, :, 1, 2] + w[:, :, 2, 1] + w[:, :, 2, 2]).half().float())
    # phase (1, 0) = index 2: rows fold as {0, 1} / {2}, columns as {0} / {1, 2}
    assert torch.equal(v[2, :, 0, 1, :], (w[:, :, 0, 1] + w[:, :, 0, 2] + w[:, :, 1, 1] + w[:, :, 1, 2]).half().float())
    assert torch.equal(v[2, :, 1, 0, :], w[:, :, 2, 0].half().float())
    # phase (1, 1) = index 3: tap (1, 1) is the corner (2, 2) alone
    assert torch.equal(v[3, :, 1, 1, :], w[:, :, 2, 2].half().float())
    # the four taps of a phase sum to all nine 3x3 taps
    for ph in range(4):
        assert torch.allclose(v[ph].sum(dim=(1, 2)), w.sum(dim=(2, 3)), rtol=2e-3, atol=1e-3)


@pytest.fixture(scope="module")
def L():
    from clap2diffusion_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def hostbuf():
    buf = ctypes.create_string_buffer(256)   # host memory: never dereferenced on these paths
    return buf, (ctypes.addressof(buf) + 15) & ~15


def fold_desc(addr, n=2, h=8, w=8, cin=640, cout=640):
    from clap2diffusion_amd import _lib
    d = _lib.ConvDesc()
    d.src0, d.weight, d.out = addr, addr, addr
    d.c0, d.n, d.h, d.w, d.oh, d.ow = cin, n, h, w, 2 * h, 2 * w
    d.ksize, d.stride, d.up = 3, 1, 2
    d.cout, d.kpad, d.out_ld = cout, 4 * cin, cout
    return d


def plan(L, d):
    tid, ks = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.c2d_conv2d_igemm_plan(ctypes.byref(d), ctypes.byref(tid), ctypes.byref(ks))
    return rc, tid.value, ks.value


BAD = [
    ("ksize=1", lambda d, a: setattr(d, "ksize", 1), E_SHAPE),
    ("stride=2", lambda d, a: setattr(d, "stride", 2), E_SHAPE),
    ("src_pad=1", lambda d, a: setattr(d, "src_pad", 1), E_ARG),
    ("second source", lambda d, a: (setattr(d, "src1", a), setattr(d, "c1", 64)), E_SHAPE),
    ("oh != 2h", lambda d, a: setattr(d, "oh", d.h), E_SHAPE),
    ("kpad < 4 cin", lambda d, a: setattr(d, "kpad", 4 * d.c0 - 64), E_SHAPE),
    ("cin=192", lambda d, a: setattr(d, "c0", 192), E_SHAPE),   # the pack no longer matches: kpad != 4 cin
    ("cin=96", lambda d, a: (setattr(d, "c0", 96), setattr(d, "kpad", 384)), E_SHAPE),   # cin % 64 != 0
    ("resid", lambda d, a: (setattr(d, "resid", a), setattr(d, "resid_ld", d.cout)), E_ARG),
    ("gn_mom", lambda d, a: (setattr(d, "gn_mom", a), setattr(d, "gn_groups", 32)), E_SHAPE),
]


@pytest.mark.parametrize("name,mutate,code", BAD, ids=[b[0] for b in BAD])
def test_descriptor_validation(L, hostbuf, name, mutate, code):
    """Each returns the code include/c2d.h documents, from the launch entry point (before any HIP call) and
    from the plan query alike; the workspace query answers 0."""
    _, addr = hostbuf
    d = fold_desc(addr)
    mutate(d, addr)
    assert L.c2d_conv2d_igemm(ctypes.byref(d), None) == code
    assert plan(L, d)[0] == code
    assert L.c2d_conv2d_igemm_workspace_size(ctypes.byref(d)) == 0


def test_up_1_keeps_its_meaning(L, hostbuf):
    """up = 1 is still the nearest-x2 view of the register-staged 3x3 (tile id 0)."""
    _, addr = hostbuf
    d = fold_desc(addr)
    d.up, d.kpad = 1, 9 * 640
    assert plan(L, d) == (0, 0, 1)
    assert L.c2d_conv2d_gn_rows(ctypes.byref(d)) == 0


def test_plan_and_workspace_answer(L, hostbuf):
    _, addr = hostbuf
    # c3's up block 2: 16 x 32^2 -> 64^2, 640 -> 640: 4 phases x 64 row tiles x 2 column tiles of 256 x 320
    d = fold_desc(addr, n=16, h=32, w=32)
    assert plan(L, d) == (0, 40, 1)
    assert L.c2d_conv2d_igemm_workspace_size(ctypes.byref(d)) == 0
    assert L.c2d_conv2d_gn_rows(ctypes.byref(d)) == 0
    # an under-filled grid splits K: slabs of 4 n h w virtual rows; without the workspace the launch runs one slice
    d = fold_desc(addr, n=2, h=8, w=8, cin=1280, cout=1280)
    L.c2d_set_plan_override(7, 2)
    try:
        need = L.c2d_conv2d_igemm_workspace_size(ctypes.byref(d))
        assert need == 2 * (4 * 2 * 8 * 8) * 1280 * 4
        assert plan(L, d) == (0, 7, 1)
        d.ws, d.ws_bytes = addr, need
        assert plan(L, d) == (0, 7, 2)
    finally:
        L.c2d_set_plan_override(0, 0)
    assert ops.upfold_ok(2, 8, 8, 1280, 1280) and not ops.upfold_ok(2, 8, 8, 96, 96)


@pytest.mark.parametrize("forced", [42, 43, 44, 70, 50, 25, 28, 29])
def test_planner_never_routes_to_tiles_without_the_mode(L, hostbuf, forced):
    _, addr = hostbuf
    shapes = [(16, 32, 32, 640, 640), (16, 16, 16, 1280, 1280), (16, 8, 8, 1280, 1280), (2, 32, 32, 640, 640),
              (2, 8, 8, 1280, 1280), (8, 64, 64, 512, 512), (8, 256, 256, 256, 256), (1, 4, 4, 64, 4), (2, 16, 16, 128, 128)]
    without = (42, 43, 44, 70, 50, 25, 28, 29)
    L.c2d_set_plan_override(forced, 0)
    try:
        for n, h, w, cin, cout in shapes:
            rc, tid, ks = plan(L, fold_desc(addr, n, h, w, cin, cout))
            assert rc == 0 and tid not in without and tid != 0 and ks == 1, (n, h, w, cin, cout, tid, ks)
    finally:
        L.c2d_set_plan_override(0, 0)
    for n, h, w, cin, cout in shapes:   # and the planner's own choice
        rc, tid, _ = plan(L, fold_desc(addr, n, h, w, cin, cout))
        assert rc == 0 and tid not in without and tid != 0, (n, h, w, cin, cout, tid)
