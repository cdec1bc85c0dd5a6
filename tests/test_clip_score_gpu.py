"""GPU tests of the CLIP-score path against the float64 / fp32 restatements of tests/clip_score_ref.py: the fused
preprocess, the row cosine, the attention kernel at the vision tower's ragged length, ImageEncoder, ClipScorer and
the Evaluator on a real (synthetic-weight) pipeline.

The tower and score gates are twice the error measured on an MI355X against the restatement, rounded up to one
digit (GATES below); every achieved figure goes to the parity log.
"""
import math

import numpy as np
import pytest
import torch

from clap2diffusion_amd import ops
from clap2diffusion_amd import weights as W
from tests import clip_score_ref as R
from tests import parity_log

pytestmark = pytest.mark.gpu

SMALL = dict(width=128, layers=2, heads=2, mlp=512, image=56, patch=14, proj=64)
WIDE = dict(width=1024, layers=2, heads=16, mlp=4096, image=224, patch=14, proj=768)
# Gates: twice the figure measured on an MI355X against the restatement, rounded up to one digit.  rel-L2 of the
# embeddings: 2 x 128 tower 7.7e-4, 2 x 1024 tower 7.0e-4, ViT-L/14 1.3e-3 (the cap for 24 layers is 2e-2); absolute
# error of ClipScorer.score: 4.8e-5
GATES = {"small": 2e-3, "wide": 2e-3, "full": 3e-3, "score": 1e-4}


def _rel_l2(got: torch.Tensor, want: torch.Tensor) -> float:
    got, want = got.double().cpu(), want.double().cpu()
    return float((got - want).norm() / want.norm())


# ------------------------------------------------------------------ c2d_clip_preprocess
def _check_preprocess(dev, imgs: np.ndarray, size: int, patch: int, exact: bool = False):
    got = ops.clip_preprocess(torch.from_numpy(imgs).to(dev), size, patch)
    k = 3 * patch * patch
    assert got.dtype == torch.float16 and tuple(got.shape) == (imgs.shape[0] * (size // patch) ** 2, ops.kpad_of(k))
    got = got.cpu()
    assert torch.count_nonzero(got[:, k:]) == 0, "pad columns must be exactly zero"
    want = R.patch_rows(R.preprocess_bytes(imgs, size).astype(np.float64), patch)
    d = np.abs(R.rows_to_bytes(got[:, :k].numpy()) - want)
    frac = float((d != 0).mean())
    parity_log.record(max_levels=d.max(), frac_differ=frac)
    print(f"{imgs.shape} size {size}: max {d.max():.0f} level(s), {100 * frac:.4f} % of bytes differ")
    assert d.max() <= (0 if exact else 1) and frac <= 1e-3
    # the fp16 values themselves: the restatement's normalised value of the byte the row decodes to, to fp16 rounding
    ref = torch.from_numpy(R.normalise(R.rows_to_bytes(got[:, :k].numpy()).reshape(-1, 3)).reshape(-1, k))
    assert torch.equal(got[:, :k], ref.half()) or (got[:, :k].double() - ref).abs().max() <= 2 ** -9
    return got


@pytest.mark.parametrize("b,h,w", [(1, 64, 64), (2, 512, 512), (1, 448, 320), (1, 320, 448), (1, 192, 256),
                                   (1, 64, 1024), (1, 65, 97)])
def test_clip_preprocess_matches_restatement(dev, b, h, w):
    imgs = R.noise_images(b, h, w, seed=31 * h + w)
    got = _check_preprocess(dev, imgs, 224, 14)
    if b > 1:
        assert not torch.equal(got[:256], got[256:]), "image 1 must differ from image 0"


def test_clip_preprocess_identity_is_exact(dev):
    _check_preprocess(dev, R.noise_images(1, 224, 224, seed=1), 224, 14, exact=True)


def test_clip_preprocess_small_tower_geometry(dev):
    got = _check_preprocess(dev, R.noise_images(2, 112, 112, seed=2), 56, 14)
    assert got.shape[0] == 2 * 16 and not torch.equal(got[:16], got[16:])


@pytest.mark.parametrize("level", [0, 255])
def test_clip_preprocess_constant_images(dev, level):
    imgs = np.full((1, 96, 160, 3), level, dtype=np.uint8)
    got = ops.clip_preprocess(torch.from_numpy(imgs).to(dev)).cpu()
    want = torch.from_numpy(R.normalise(np.full((3,), level, dtype=np.uint8))).half()   # per channel
    assert torch.equal(got[:, :588].reshape(-1, 3), want.expand(256 * 196, 3))
    assert torch.count_nonzero(got[:, 588:]) == 0


def test_clip_preprocess_rejects_bad_arguments(dev):
    img = torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        ops.clip_preprocess(img, 224, 15)
    with pytest.raises(RuntimeError, match="C2D_E_SHAPE"):
        torch.ops.c2d.clip_preprocess(img, 224, 14, list(R.CLIP_MEAN), list(R.CLIP_STD),
                                      torch.empty(256, 704, dtype=torch.float16, device=dev))


# ------------------------------------------------------------------ c2d_cosine_rows
@pytest.mark.parametrize("m,c", [(1, 768), (5, 768), (3, 7)])
def test_cosine_rows(dev, m, c):
    g = torch.Generator().manual_seed(100 * m + c)
    a, b = torch.randn(m, c, generator=g), torch.randn(m, c, generator=g)
    a[0] *= 1e4                      # elements near 1e4: the sums of squares reach ~1e11
    b[0] = b[0] * 1e4 + 3e3
    if m > 1:
        b[1] = a[1]                  # identical rows
    if m > 2:
        a[2] = 0                     # a zero row
    got = ops.cosine_rows(a.to(dev), b.to(dev)).cpu()
    want = R.cosine(a, b)
    err = (got.double() - want).abs().max().item()
    parity_log.record(max_abs=err)
    assert got.dtype == torch.float32 and tuple(got.shape) == (m,) and torch.isfinite(got).all()
    assert err <= 4 * c * 2 ** -24   # fp32 sums of c products, each within 2^-24 relative
    if m > 1:
        assert abs(got[1].item() - 1.0) <= 4 * 2 ** -23
    if m > 2:
        assert got[2].item() == 0.0


# ------------------------------------------------------------------ c2d_attention_fwd at the tower's shape
def test_attention_at_257_tokens(dev):
    """d = 64, 16 heads, lq = lk = 257 = 4 x 64 + 1, batch 2: the existing kernel at the vision tower's ragged length."""
    b, heads, t, d = 2, 16, 257, 64
    g = torch.Generator().manual_seed(257)
    qkv = torch.randn(b * t, 3 * heads * d, generator=g).half()
    c = heads * d
    got = ops.attention(*(qkv.to(dev)[:, i * c:(i + 1) * c] for i in range(3)), b, heads, t, t, d).cpu()
    q, k, v = (qkv[:, i * c:(i + 1) * c].double().view(b, t, heads, d).transpose(1, 2) for i in range(3))
    want = ((q @ k.transpose(-1, -2) / math.sqrt(d)).softmax(-1) @ v).transpose(1, 2).reshape(b * t, c)
    rel, mx = _rel_l2(got, want), (got.double() - want).abs().max().item()
    parity_log.record(rel_l2=rel, max_abs=mx)
    print(f"attention 257: rel-L2 {rel:.3g}, max abs {mx:.3g}")
    # the bound of the project's other attention tests (tests/test_kernels_gpu.py: rel-L2 5e-3, max error 2e-2 max|ref|)
    assert rel <= 5e-3 and mx <= 2e-2 * want.abs().max().item()


# ------------------------------------------------------------------ ImageEncoder
def _encoder_case(dev, cfg, batch, seed, gate, hw=(96, 80)):
    from clap2diffusion_amd.image_encoder import ImageEncoder
    sd = W.synth_clip_vision(seed, cfg)
    imgs = R.noise_images(batch, *hw, seed=seed)
    got = ImageEncoder(dev, state_dict=sd, cfg=cfg)(torch.from_numpy(imgs).to(dev))
    want = R.image_embeds(R.preprocess(imgs, cfg["image"], cfg["patch"]), sd, cfg)
    rel, mx = _rel_l2(got, want), (got.double().cpu() - want).abs().max().item()
    parity_log.record(rel_l2=rel, max_abs=mx, gate=gate)
    print(f"ImageEncoder {cfg['layers']} x {cfg['width']}: rel-L2 {rel:.3g}, max abs {mx:.3g} (gate {gate})")
    assert got.dtype == torch.float32 and tuple(got.shape) == (batch, cfg["proj"]) and torch.isfinite(got).all()
    assert rel <= gate


def test_image_encoder_small(dev):
    _encoder_case(dev, SMALL, 3, 11, GATES["small"])


def test_image_encoder_wide(dev):
    _encoder_case(dev, WIDE, 2, 12, GATES["wide"])


# ------------------------------------------------------------------ the full tower, ClipScorer
PROMPTS = ["thunder and rain", "birds chirping in a forest at dawn", "a dog"]


_DEEP = {}


@pytest.fixture
def deep(dev, progress):
    """The seeded CLIPModel, a ClipScorer on it and the fp32 CPU restatement of 3 images x 3 prompts: built by the
    first test that asks and shared unchanged by the rest of the module."""
    if not _DEEP:
        from clap2diffusion_amd.clip_score import ClipScorer
        sd = W.synth_clip_model(0)
        progress("synthetic CLIPModel drawn")
        scorer = ClipScorer(dev, seed=0)
        imgs = R.noise_images(3, 128, 192, seed=9)
        ids = scorer.tokenize(PROMPTS)
        ref_img = R.image_embeds(R.preprocess(imgs), sd, W.CLIP_VISION_CFG, dtype=torch.float32)
        progress("vision restatement done")
        ref_txt = R.text_embeds(ids, sd, W.CLIP_TEXT_CFG["layers"], W.CLIP_TEXT_CFG["heads"], dtype=torch.float32)
        progress("text restatement done")
        _DEEP.update(scorer=scorer, imgs=torch.from_numpy(imgs).to(dev), ids=ids, ref_img=ref_img, ref_txt=ref_txt)
    return _DEEP


def test_image_encoder_full_vit_l14(deep):
    got = deep["scorer"].image_encoder(deep["imgs"][:1])
    want = deep["ref_img"][:1]
    rel, mx = _rel_l2(got, want), (got.double().cpu() - want.double()).abs().max().item()
    parity_log.record(rel_l2=rel, max_abs=mx, gate=GATES["full"])
    print(f"ImageEncoder ViT-L/14: rel-L2 {rel:.3g}, max abs {mx:.3g} (gate {GATES['full']})")
    assert tuple(got.shape) == (1, 768) and GATES["full"] <= 2e-2 and rel <= GATES["full"]


def test_clip_scorer_score(deep):
    scorer, imgs, ids = deep["scorer"], deep["imgs"], deep["ids"]
    got = scorer.score(imgs, ids)
    want = R.cosine(deep["ref_img"], deep["ref_txt"])
    err = (got.double().cpu() - want).abs().max().item()
    parity_log.record(max_abs=err, gate=GATES["score"], rel_l2_text=_rel_l2(scorer.text_embeds(ids), deep["ref_txt"]))
    print(f"ClipScorer.score: {got.tolist()} vs {want.tolist()}; max abs error {err:.3g} (gate {GATES['score']})")
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (3,)
    assert err <= GATES["score"]
    ie, te = scorer.image_embeds(imgs), scorer.text_embeds(ids)
    assert tuple(ie.shape) == tuple(te.shape) == (3, 768) and ie.dtype == te.dtype == torch.float32
    assert (got.double().cpu() - R.cosine(ie.cpu(), te.cpu())).abs().max().item() <= 4 * 768 * 2 ** -24
    same = scorer.image_similarity(imgs, imgs)
    assert (same - 1).abs().max().item() <= 4 * 2 ** -23


# ------------------------------------------------------------------ Evaluator on a pipeline
def test_evaluator_single_on_pipeline(dev, deep, monkeypatch):
    from clap2diffusion_amd.evaluate import Evaluator
    from clap2diffusion_amd.pipeline import AudioToImageInference
    pipe = AudioToImageInference(device=dev, height=64, width=64, verbose=False)
    sampled, scored = [], []
    gen, score = pipe.generate_batch, deep["scorer"].score
    monkeypatch.setattr(pipe, "generate_batch", lambda *a, **k: sampled.append(gen(*a, **k)) or sampled[-1])
    monkeypatch.setattr(deep["scorer"], "score", lambda im, ids: scored.append(im) or score(im, ids))
    steps = {"num_inference_steps": 2}
    u8 = pipe.batch_generate_u8
    monkeypatch.setattr(pipe, "batch_generate_u8", lambda *a, **k: u8(*a, **{**steps, **k}))
    ev = Evaluator(pipeline=pipe, scorer=deep["scorer"])
    r1 = ev.evaluate_single("synthetic:1", "thunder and rain")
    den, graphs = dict(pipe._denoisers), dict(pipe._batch_graphs)
    captured = {k: (d.graph if hasattr(d, "graph") else None) for k, d in den.items()}
    r2 = ev.evaluate_single("synthetic:1", "thunder and rain", reference_image=r1["generated_image"])
    assert type(r1["clip_score"]) is float and math.isfinite(r1["clip_score"]) and -1.0 <= r1["clip_score"] <= 1.0
    assert r1["generated_image"].size == (64, 64)
    assert r2["clip_score"] == r1["clip_score"]                       # seed 42 both times
    assert abs(r2["image_similarity"] - 1.0) <= 4 * 2 ** -23          # the same image again
    assert len(sampled) == len(scored) == 2
    for s, im in zip(sampled, scored):                                # the sampler's device tensor itself
        assert im is s and im.is_cuda and im.dtype == torch.uint8 and tuple(im.shape) == (1, 64, 64, 3)
    assert pipe._denoisers.keys() == den.keys() and all(pipe._denoisers[k] is den[k] for k in den)
    assert all((pipe._denoisers[k].graph if hasattr(den[k], "graph") else None) is captured[k] for k in den)
    assert pipe._batch_graphs == graphs and ev.metrics["audio_alignment"] == []
