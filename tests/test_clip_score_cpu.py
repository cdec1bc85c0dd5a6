"""CPU tests of the CLIP-score evaluator: the float64 restatements (tests/clip_score_ref.py) against PIL and
transformers, the synthetic CLIPModel key layout, the Evaluator's host logic with an injected pipeline and scorer,
and the two new entry points' operator schemas and argument validation (nothing is launched)."""
import ctypes
import json

import numpy as np
import pytest
import torch

from clap2diffusion_amd import weights as W
from tests import clip_score_ref as R

SMALL_VISION = dict(width=128, layers=2, heads=2, mlp=512, image=56, patch=14, proj=64)
SMALL_TEXT = dict(vocab=49408, width=128, layers=2, heads=2, mlp=512, max_len=77)


def _levels(a: np.ndarray, b: np.ndarray):
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    return int(d.max()), float((d != 0).mean())


# ------------------------------------------------------------------ resize / preprocess against PIL
@pytest.mark.parametrize("h,w,size", [(512, 512, 224), (64, 64, 224), (256, 256, 224), (320, 320, 224),
                                       (448, 320, 224), (192, 256, 224), (64, 128, 224)])
def test_resize_restatement_matches_pil(h, w, size):
    from PIL import Image
    img = R.noise_images(1, h, w, seed=h * 1000 + w)[0]
    rh, rw = R.resized_size(h, w, size)
    want = np.asarray(Image.fromarray(img).resize((rw, rh), Image.BICUBIC))
    got = R.resize_bicubic(img, rh, rw)
    mx, frac = _levels(got, want)
    print(f"{h}x{w} -> {rh}x{rw}: max {mx} level(s), {100 * frac:.4f} % of bytes differ")
    assert got.shape == want.shape and mx <= 1 and frac <= 1e-3


@pytest.mark.parametrize("h,w", [(448, 320), (320, 448), (192, 256), (64, 1024)])
def test_preprocess_restatement_matches_pil_and_numpy(h, w):
    from PIL import Image
    size, patch = 224, 14
    imgs = R.noise_images(2, h, w, seed=7 * h + w)
    rh, rw = R.resized_size(h, w, size)
    top, left = (rh - size) // 2, (rw - size) // 2
    want_u8 = np.stack([np.asarray(Image.fromarray(im).resize((rw, rh), Image.BICUBIC))[top:top + size, left:left + size]
                        for im in imgs])
    got_u8 = R.preprocess_bytes(imgs, size)
    mx, frac = _levels(got_u8, want_u8)
    print(f"{h}x{w}: crop at ({top}, {left}) of {rh}x{rw}; max {mx} level(s), {100 * frac:.4f} % differ")
    assert got_u8.shape == (2, size, size, 3) and mx <= 1 and frac <= 1e-3
    # normalise and patch cut: the same arithmetic with numpy and torch's unfold on the restatement's own bytes
    want = (got_u8 / 255.0 - np.array(R.CLIP_MEAN)) / np.array(R.CLIP_STD)
    unf = torch.nn.functional.unfold(torch.from_numpy(want).permute(0, 3, 1, 2), patch, stride=patch)   # [B, c*p*p, g*g]
    unf = unf.view(2, 3, patch, patch, -1).permute(0, 4, 2, 3, 1).reshape(2 * (size // patch) ** 2, -1)
    rows = R.preprocess(imgs, size, patch)
    assert rows.shape == (2 * 256, 588) and np.array_equal(rows, unf.numpy())
    assert np.array_equal(R.rows_to_bytes(rows), R.patch_rows(got_u8.astype(np.float64), patch))


# ------------------------------------------------------------------ synthetic weights against transformers
def _fit(sd: dict, have) -> dict:
    """Drop the text_model. / vision_model. wrapper where this transformers' module has none (transformers >= 5
    drops it on some classes, as oracle/clip_ref.py handles for the text tower)."""
    out = {}
    for k, v in sd.items():
        if k not in have:
            for pre in ("text_model.", "vision_model."):
                if k.startswith(pre) and k[len(pre):] in have:
                    k = k[len(pre):]
        out[k] = v
    return out


def _clip_config(vision: dict, text: dict, proj: int):
    from transformers import CLIPConfig
    return CLIPConfig(
        text_config=dict(vocab_size=text["vocab"], hidden_size=text["width"], intermediate_size=text["mlp"],
                         num_hidden_layers=text["layers"], num_attention_heads=text["heads"],
                         max_position_embeddings=text["max_len"], hidden_act="quick_gelu", eos_token_id=R.EOS,
                         bos_token_id=49406, pad_token_id=1),
        vision_config=dict(hidden_size=vision["width"], intermediate_size=vision["mlp"],
                           num_hidden_layers=vision["layers"], num_attention_heads=vision["heads"],
                           image_size=vision["image"], patch_size=vision["patch"], hidden_act="quick_gelu"),
        projection_dim=proj)


def test_synth_clip_model_keys_match_transformers():
    from transformers import CLIPModel
    with torch.device("meta"):
        model = CLIPModel(_clip_config(W.CLIP_VISION_CFG, W.CLIP_TEXT_CFG, W.CLIP_VISION_CFG["proj"]))
    want = {k: tuple(v.shape) for k, v in model.state_dict().items() if "position_ids" not in k}
    shapes = dict(W.clip_text_param_shapes())
    shapes.update(W.clip_vision_param_shapes())
    shapes.update({"text_projection.weight": (768, 768), "logit_scale": ()})
    shapes = _fit(shapes, want)
    assert set(shapes) == set(want), (set(shapes) ^ set(want))
    assert all(tuple(shapes[k]) == want[k] for k in want)
    # the tensors themselves: one seeded model, the key set above (drawn at a cheap size: keys only need the names)
    small = W.synth_clip_vision(0, SMALL_VISION)
    assert set(small) == set(W.clip_vision_param_shapes(SMALL_VISION))
    assert all(tuple(v.shape) == tuple(W.clip_vision_param_shapes(SMALL_VISION)[k]) for k, v in small.items())


@pytest.mark.slow
def test_synth_clip_model_tensors():
    sd = W.synth_clip_model(0)
    text = W.synth_clip_text(0)
    assert all(torch.equal(sd[k], text[k]) for k in text)   # the pipeline's seeded text tower, tensor for tensor
    assert abs(float(sd["logit_scale"]) - np.log(1 / 0.07)) < 1e-6
    assert tuple(sd["vision_model.embeddings.position_embedding.weight"].shape) == (257, 1024)
    assert tuple(sd["vision_model.embeddings.patch_embedding.weight"].shape) == (1024, 3, 14, 14)


def test_vision_restatement_matches_transformers():
    from transformers import CLIPVisionModelWithProjection
    cfg = _clip_config(SMALL_VISION, SMALL_TEXT, SMALL_VISION["proj"])
    vc = cfg.vision_config
    vc.projection_dim = SMALL_VISION["proj"]
    model = CLIPVisionModelWithProjection(vc).eval()
    sd = W.synth_clip_vision(3, SMALL_VISION)
    missing, unexpected = model.load_state_dict(_fit(sd, set(model.state_dict())), strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    imgs = R.noise_images(3, 80, 112, seed=5)
    pix = R.normalise(R.preprocess_bytes(imgs, SMALL_VISION["image"]))
    with torch.no_grad():
        want = model(pixel_values=torch.from_numpy(pix).permute(0, 3, 1, 2).float()).image_embeds
    got = R.image_embeds(R.patch_rows(pix, SMALL_VISION["patch"]), sd, SMALL_VISION, dtype=torch.float32)
    assert got.shape == want.shape == (3, SMALL_VISION["proj"])
    assert torch.allclose(got, want, atol=1e-4, rtol=1e-4), (got - want).abs().max().item()


def test_text_restatement_matches_transformers():
    from transformers import CLIPTextModelWithProjection
    from clap2diffusion_amd.text_encoder import tokenize
    cfg = _clip_config(SMALL_VISION, SMALL_TEXT, SMALL_VISION["proj"])
    tc = cfg.text_config
    tc.projection_dim = SMALL_VISION["proj"]
    model = CLIPTextModelWithProjection(tc).eval()
    shapes = dict(W.clip_text_param_shapes(SMALL_TEXT))
    shapes["text_projection.weight"] = (SMALL_VISION["proj"], SMALL_TEXT["width"])
    sd = W.synth_clip_shapes(shapes, 3, "cpu")
    missing, unexpected = model.load_state_dict(_fit(sd, set(model.state_dict())), strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    ids = tokenize(["thunder and rain", "birds chirping in a forest at dawn", ""])
    assert R.first_eos(ids).tolist() == [4, 8, 1]
    with torch.no_grad():
        want = model(input_ids=ids).text_embeds
    got = R.text_embeds(ids, sd, SMALL_TEXT["layers"], SMALL_TEXT["heads"], dtype=torch.float32)
    assert torch.allclose(got, want, atol=1e-4, rtol=1e-4), (got - want).abs().max().item()


def test_cosine_restatement():
    a = torch.tensor([[3.0, 4.0], [0.0, 0.0], [1.0, 0.0]])
    b = torch.tensor([[4.0, 3.0], [1.0, 2.0], [-2.0, 0.0]])
    assert torch.allclose(R.cosine(a, b), torch.tensor([24 / 25, 0.0, -1.0], dtype=torch.float64))


# ------------------------------------------------------------------ Evaluator host logic
class FakePipeline:
    device, seed = torch.device("cpu"), 0

    def __init__(self):
        self.calls = []

    def batch_generate_u8(self, audio_paths, text_prompts=None, **kw):
        self.calls.append(([str(p) for p in audio_paths], list(text_prompts), kw))
        return torch.stack([torch.full((8, 8, 3), 10 * len(t), dtype=torch.uint8) for t in text_prompts])

    @staticmethod
    def to_pil(images):
        from PIL import Image
        return [Image.fromarray(im) for im in images.cpu().numpy()]


class FakeScorer:
    def __init__(self):
        self.scored, self.similar = [], []

    def tokenize(self, prompts):
        return torch.tensor([[len(p)] for p in prompts])

    def score(self, images_u8, ids):
        self.scored.append(images_u8)
        return images_u8[:, 0, 0, 0].float() / 255 - ids[:, 0].float() / 1000

    def image_similarity(self, a_u8, b_u8):
        self.similar.append((a_u8, b_u8))
        return torch.full((a_u8.shape[0],), 0.5)


def _dataset(tmp_path, entries, present):
    (tmp_path / "audio").mkdir(parents=True)
    for name in present:
        (tmp_path / "audio" / name).write_bytes(b"RIFF")
    if entries is not None:
        (tmp_path / "metadata.json").write_text(json.dumps(entries))
    return tmp_path


def _plain(o) -> bool:
    if isinstance(o, dict):
        return all(isinstance(k, str) and _plain(v) for k, v in o.items())
    if isinstance(o, list):
        return all(_plain(v) for v in o)
    return type(o) in (float, str)


def test_evaluator_dataset_loop(tmp_path, capsys):
    from clap2diffusion_amd.evaluate import Evaluator
    entries = [{"audio": "a.wav", "text": "rain", "id": "x1"}, {"audio": "gone.wav", "text": "wind", "id": "x2"},
               {"audio": "b.wav", "text": "a dog barks", "id": "x3"}, {"audio": "c.wav", "text": "sea", "id": "x4"}]
    data = _dataset(tmp_path / "data", entries, ["a.wav", "b.wav", "c.wav"])
    pipe, scorer = FakePipeline(), FakeScorer()
    ev = Evaluator(checkpoint_dir=tmp_path, pipeline=pipe, scorer=scorer, batch=2)
    assert list(ev.metrics) == ["clip_score", "fid_score", "inception_score", "audio_alignment"]
    out = tmp_path / "out" / "nested"
    avg = ev.evaluate_dataset(data, out)
    assert f"Warning: {data / 'audio' / 'gone.wav'} not found, skipping..." in capsys.readouterr().out
    # batches of 2 over the three entries that exist, every one from seed 42
    assert [(c[0], c[1]) for c in pipe.calls] == [([str(data / "audio" / "a.wav"), str(data / "audio" / "b.wav")],
                                                   ["rain", "a dog barks"]), ([str(data / "audio" / "c.wav")], ["sea"])]
    assert all(c[2] == {"seed": 42} for c in pipe.calls)
    # the scorer saw the pipeline's tensors themselves
    assert [tuple(s.shape) for s in scorer.scored] == [(2, 8, 8, 3), (1, 8, 8, 3)]
    want = [40 / 255 - 0.004, 110 / 255 - 0.011, 30 / 255 - 0.003]
    assert ev.metrics["clip_score"] == pytest.approx(want, abs=1e-6)
    assert ev.metrics["audio_alignment"] == [] and ev.metrics["fid_score"] == [] and ev.metrics["inception_score"] == []
    assert sorted(p.name for p in out.iterdir()) == ["evaluation_results.json", "x1_generated.png", "x3_generated.png",
                                                     "x4_generated.png"]
    from PIL import Image
    assert np.asarray(Image.open(out / "x3_generated.png")).shape == (8, 8, 3)
    res = json.loads((out / "evaluation_results.json").read_text())
    assert set(res) == {"individual_results", "average_metrics"}
    assert [r["id"] for r in res["individual_results"]] == ["x1", "x3", "x4"]
    assert all(set(r) == {"id", "audio", "text", "clip_score"} for r in res["individual_results"])
    assert set(res["average_metrics"]) == {"clip_score", "clip_score_std"}
    assert res["average_metrics"]["clip_score"] == pytest.approx(np.mean(want), abs=1e-6)
    assert res["average_metrics"]["clip_score_std"] == pytest.approx(np.std(want), abs=1e-6)
    assert _plain(res) and _plain(avg) and avg == res["average_metrics"]
    ev.print_results(avg)
    printed = capsys.readouterr().out
    assert "Evaluation Results" in printed and "clip_score" in printed and "±" in printed


def test_evaluator_dummy_metadata(tmp_path, capsys):
    from clap2diffusion_amd.evaluate import Evaluator
    data = _dataset(tmp_path / "d", None, ["sample2.wav"])
    pipe = FakePipeline()
    ev = Evaluator(pipeline=pipe, scorer=FakeScorer())
    avg = ev.evaluate_dataset(data, tmp_path / "o")
    out = capsys.readouterr().out
    assert "Evaluating 2 samples..." in out and "sample1.wav not found, skipping..." in out
    assert [c[1] for c in pipe.calls] == [["birds chirping"]]
    assert (tmp_path / "o" / "002_generated.png").exists() and set(avg) == {"clip_score", "clip_score_std"}
    assert avg["clip_score_std"] == 0.0


def test_evaluator_single_and_clip_score(tmp_path):
    from PIL import Image
    from clap2diffusion_amd.evaluate import Evaluator
    pipe, scorer = FakePipeline(), FakeScorer()
    ev = Evaluator(pipeline=pipe, scorer=scorer)
    r = ev.evaluate_single("some.wav", "rain")
    assert set(r) == {"clip_score", "generated_image"} and type(r["clip_score"]) is float
    assert r["generated_image"].size == (8, 8) and pipe.calls[-1][2] == {"seed": 42}
    ref = np.full((5, 7, 3), 9, dtype=np.uint8)
    r = ev.evaluate_single("some.wav", "rain", reference_image=ref)
    assert set(r) == {"clip_score", "generated_image", "image_similarity"} and r["image_similarity"] == 0.5
    assert tuple(scorer.similar[-1][1].shape) == (1, 5, 7, 3) and scorer.similar[-1][1].dtype == torch.uint8
    assert ev.metrics["audio_alignment"] == []
    # compute_clip_score: a PIL image, a path and a uint8 array give the same Python float
    arr = np.full((6, 4, 3), 51, dtype=np.uint8)
    Image.fromarray(arr).save(tmp_path / "im.png")
    vals = [ev.compute_clip_score(x, "abc") for x in (Image.fromarray(arr), tmp_path / "im.png", arr)]
    assert all(type(v) is float for v in vals) and vals == pytest.approx([51 / 255 - 0.003] * 3, abs=1e-6)
    with pytest.raises(ValueError):
        ev.compute_clip_score(np.zeros((4, 4), dtype=np.uint8), "abc")


def test_evaluate_cli_flags():
    from clap2diffusion_amd.evaluate import build_parser
    a = build_parser().parse_args([])
    assert (a.data_dir, a.checkpoint_dir, a.output_dir) == ("../data/audiocaps/test", "../checkpoints",
                                                            "evaluation_results")
    a = build_parser().parse_args(["--sd_model", "s", "--clap_model", "c", "--clip_model", "k", "--batch", "8"])
    assert (a.sd_model, a.clap_model, a.clip_model, a.batch) == ("s", "c", "k", 8)


# ------------------------------------------------------------------ operators and the C ABI
def test_new_ops_are_registered_with_fake_impls():
    from clap2diffusion_amd import torch_ops
    assert "clip_preprocess" in torch_ops.OPS and "cosine_rows" in torch_ops.OPS
    s = str(torch.ops.c2d.clip_preprocess.default._schema)
    assert "Tensor img" in s and "Int size" in s and "Int patch" in s and "float[] mean" in s and "!) out" in s
    s = str(torch.ops.c2d.cosine_rows.default._schema)
    assert "Tensor a" in s and "Tensor b" in s and "!) out" in s
    with torch.device("meta"):   # the fake implementations: shapes flow, nothing runs
        img = torch.empty(2, 96, 64, 3, dtype=torch.uint8)
        out = torch.empty(2 * 256, 640, dtype=torch.float16)
        assert torch.ops.c2d.clip_preprocess(img, 224, 14, [0.5] * 3, [0.25] * 3, out) is None
        a = torch.empty(4, 768)
        assert torch.ops.c2d.cosine_rows(a, a, torch.empty(4)) is None


def test_new_entry_points_validate_before_launch():
    """c2d_clip_preprocess / c2d_cosine_rows: the documented C2D_E_* codes on arguments that cannot be right,
    nothing launched (bogus non-null pointers, never dereferenced)."""
    from clap2diffusion_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 2)
    f3 = ctypes.c_float * 3
    mean, std = f3(*R.CLIP_MEAN), f3(*R.CLIP_STD)
    OK, ARG, SHAPE, ALIGN = 0, -1, -2, -3
    del OK
    cp = L.c2d_clip_preprocess   # (img, n, h, w, size, patch, mean, std, kpad, out, stream)
    assert cp(None, 1, 64, 64, 224, 14, mean, std, 640, p, None) == ARG
    assert cp(p, 1, 64, 64, 224, 14, None, std, 640, p, None) == ARG
    assert cp(p, 1, 64, 64, 224, 14, mean, None, 640, p, None) == ARG
    assert cp(p, 1, 64, 64, 224, 14, mean, std, 640, None, None) == ARG
    assert cp(p, 1, 64, 64, 224, 14, mean, f3(0.2, 0.0, 0.2), 640, p, None) == ARG
    for n, h, w, size, patch, kpad in ((0, 64, 64, 224, 14, 640), (-1, 64, 64, 224, 14, 640), (1, 0, 64, 224, 14, 640),
                                       (1, 64, -3, 224, 14, 640), (1, 64, 64, 0, 14, 640), (1, 64, 64, 224, 0, 640),
                                       (1, 64, 64, 224, 15, 704), (1, 64, 64, 225, 14, 640), (1, 64, 64, 224, 14, 588),
                                       (1, 64, 64, 224, 14, 704), (1, 64, 64, 66, 33, 3328)):
        assert cp(p, n, h, w, size, patch, mean, std, kpad, p, None) == SHAPE, (n, h, w, size, patch, kpad)
    assert cp(p, 1, 64, 64, 224, 14, mean, std, 640, odd, None) == ALIGN
    cr = L.c2d_cosine_rows       # (a, b, m, c, out, stream)
    assert cr(None, p, 2, 8, p, None) == ARG
    assert cr(p, None, 2, 8, p, None) == ARG
    assert cr(p, p, 2, 8, None, None) == ARG
    for m, c in ((0, 8), (-1, 8), (2, 0), (2, -8)):
        assert cr(p, p, m, c, p, None) == SHAPE, (m, c)
    assert cr(odd, p, 2, 8, p, None) == ALIGN
    assert cr(p, odd, 2, 8, p, None) == ALIGN
    assert cr(p, p, 2, 8, odd, None) == ALIGN
