"""The folded upsample on the GPU (c2d_conv_desc::up = 2): nearest x2 + 3x3 conv as four 2x2 phase convs of the
low-res tensor in one launch.  Reference: fp32 F.conv2d(F.interpolate(x16.float(), 2), w32, b, padding=1) on the
fp16-rounded input; bar: the project's conv bar (tests/test_kernels_gpu.py::close, rel-L2 <= 5e-3 and
rel-max <= 2e-2).  Random weights, so that any phase or tap mix-up shows."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from clap2diffusion_amd import ops
from clap2diffusion_amd.unet import Upsample2D
from tests import parity_log
from tests.test_kernels_gpu import close, force_plan, gen, nchw, nhwc  # noqa: F401  (force_plan: fixture)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(n, h, w, cin, cout):
    """(x fp16 NHWC, w fp32, bias, reference NCHW fp32) of one shape, computed once and shared (never written)."""
    x = gen(n, cin, h, w, seed=11 + h + cin)
    wt = gen(cout, cin, 3, 3, seed=12 + cout, scale=1.0 / math.sqrt(9 * cin))
    b = gen(cout, seed=13)
    x16 = x.half()
    ref = F.conv2d(F.interpolate(x16.float(), scale_factor=2.0, mode="nearest"), wt, b, padding=1)
    return nhwc(x16), wt, b, ref


def run_fold(dev, n, h, w, cin, cout, out=None):
    x16, wt, b, ref = case(n, h, w, cin, cout)
    wf, kp = ops.fold_upsample_weight(wt)
    with ops.record_conv_plans() as plans:
        y = ops.conv(x16.to(dev), wf.to(dev), kp, cout, ksize=3, bias=b.to(dev), up_fold=True, out=out)
    assert tuple(y.shape) == (n, 2 * h, 2 * w, cout)
    return y, ref, plans


@pytest.mark.parametrize("n,h,w,cin,cout", [
    (1, 4, 4, 320, 320),      # a phase (16 rows) smaller than every tile: borders dominate
    (3, 6, 10, 128, 320),     # 180 rows per phase: no multiple of any tile, not square
    (2, 8, 8, 640, 1280),     # several column tiles
])
def test_planned(dev, n, h, w, cin, cout):
    y, ref, plans = run_fold(dev, n, h, w, cin, cout)
    assert len(plans) == 1 and plans[0][0] not in (0, 25, 28, 29, 42, 43, 44, 50, 70), plans
    close(nchw(y), ref)


@pytest.mark.parametrize("tile", [40, 41])
@pytest.mark.parametrize("n,h,w", [(4, 8, 8), (4, 8, 16)])   # exactly one / exactly two 256-row tiles per phase
def test_pingpong_tiles_forced(dev, force_plan, tile, n, h, w):
    force_plan(tile, 1)
    y, ref, plans = run_fold(dev, n, h, w, 640, 640)
    assert plans == [(tile, 1)], plans
    close(nchw(y), ref)


@pytest.mark.parametrize("tile,split", [(40, 4), (7, 2), (80, 1), (80, 2)])
def test_split_k_forced_bit_identical(dev, force_plan, tile, split):
    """The combine's row map (and tile 80's two K groups); two runs are bit-identical (fixed-order sums)."""
    force_plan(tile, split)
    y0, ref, plans = run_fold(dev, 2, 8, 8, 1280, 1280)
    assert plans == [(tile, split)], plans
    y1, _, _ = run_fold(dev, 2, 8, 8, 1280, 1280)
    assert torch.equal(y0, y1)
    close(nchw(y0), ref)


@pytest.mark.parametrize("tile", [8, 9, 81])
def test_small_grid_tiles_forced(dev, force_plan, tile):
    force_plan(tile, 1)
    y, ref, plans = run_fold(dev, 2, 16, 16, 320, 320)
    assert plans == [(tile, 1)], plans
    close(nchw(y), ref)


def test_against_materialised_path(dev):
    """The same input through upsample_nearest2x + the 3x3 conv: both meet the bar; the two differ only by where
    the weights are rounded to fp16 (their rel-L2 is recorded, no bar of its own)."""
    n, h, w, cin, cout = 2, 8, 8, 640, 640
    x16, wt, b, ref = case(n, h, w, cin, cout)
    y, _, _ = run_fold(dev, n, h, w, cin, cout)
    wp, kp = ops.pack_conv_weight(wt)
    old = ops.conv(ops.upsample_nearest2x(x16.to(dev)), wp.to(dev), kp, cout, ksize=3, bias=b.to(dev))
    close(nchw(y), ref)
    close(nchw(old), ref)
    d = (y.float() - old.float()).norm() / old.float().norm()
    parity_log.record(fold_vs_materialised_rel_l2=d.item())
    assert d.item() <= 1e-2   # two results within 5e-3 of one reference


@pytest.mark.parametrize("c,folded", [(96, False), (192, True)])
def test_upsample2d_module_and_fallback(dev, c, folded):
    """Upsample2D end to end.  96 channels (cin % 64 != 0) is refused by the library: the materialised path
    runs (an upsample launch, the 3x3 pack).  192 = 3 x 64 channels meets the mode's rule and runs folded.
    Both match the reference."""
    n, h, w = 2, 6, 5
    x16, wt, b, ref = case(n, h, w, c, c)
    m = Upsample2D(c)
    m.conv.load(wt, b)
    m = m.to(dev)
    assert ops.upfold_ok(n, h, w, c, c) == folded
    with ops.record_conv_plans() as plans:
        y = m(x16.to(dev))
    assert len(plans) == 1 and (plans[0][0] != 0) == folded, plans   # tile 0: the register-staged 3x3 of cin % 64 != 0
    assert tuple(y.shape) == (n, 2 * h, 2 * w, c)
    close(nchw(y), ref)
    assert "weight_fold" not in m.state_dict() and "conv.weight" in m.state_dict()   # checkpoint keys unchanged


@pytest.mark.parametrize("n,h,w,cin,cout,tile,split", [
    (3, 6, 10, 128, 320, 0, 0),       # the planner's tile, M tail in every phase
    (3, 6, 10, 128, 320, 40, 1),      # the ping-pong tile, 180 of 256 rows live
    (2, 8, 8, 1280, 1280, 7, 2),      # the split-K combine's stores
])
def test_bytes_outside_the_output_stay_untouched(dev, force_plan, n, h, w, cin, cout, tile, split):
    if tile:
        force_plan(tile, split)
    numel, pad = n * 2 * h * 2 * w * cout, 4096
    sentinel = -1234.0
    buf = torch.full((pad + numel + pad,), sentinel, dtype=torch.float16, device=dev)
    out = buf[pad:pad + numel].view(n, 2 * h, 2 * w, cout)
    y, ref, _ = run_fold(dev, n, h, w, cin, cout, out=out)
    assert y.data_ptr() == out.data_ptr()
    assert bool((buf[:pad] == sentinel).all()) and bool((buf[pad + numel:] == sentinel).all())
    assert not bool((out == sentinel).any())   # and every output element was written
    close(nchw(y), ref)
