"""Evaluator -- drop-in for the reference scripts/evaluate.py API (scripts/evaluate.py:19-183).

Same class, methods, result files and CLI flags as the reference: Evaluator(checkpoint_dir), self.metrics with
its four keys, compute_clip_score, evaluate_single, evaluate_dataset (metadata.json or the two dummy entries,
missing audio skipped with the reference's warning, <id>_generated.png, evaluation_results.json with
individual_results and average_metrics), print_results, main(--data_dir --checkpoint_dir --output_dir).  Where
the reference returns a random number for the CLIP score (:32-35), this computes it: the cosine between CLIP
ViT-L/14's image and text embeddings on the HIP kernels (clip_score.ClipScorer), scored on the sampler's uint8
device images without a trip through the host.  reference_image, which the reference declares and never uses,
adds image_similarity: the same cosine between the generated and the reference image.

fid_score and inception_score stay empty, as in the reference (they need InceptionV3 weights), and so does
audio_alignment: the reference's compute_audio_alignment is another random number, and CLIP and CLAP share no
embedding space, so an honest audio-to-image metric needs a model that is not part of this stack.  None is
invented here.

With the seeded synthetic weights and the hash-id tokenizer the scores are deterministic and meaningless, as the
images are; they measure something with real SD1.5 / CLAP / CLIP weights (--sd_model --clap_model --clip_model).
"""
from __future__ import annotations

import argparse
import json
import os
from pathlib import Path

import numpy as np
import torch


METRIC_NAMES = ("clip_score", "fid_score", "inception_score", "audio_alignment")   # the reference's four keys
# what the reference evaluates when data_dir has no metadata.json
DUMMY_METADATA = (("sample1.wav", "thunder and rain", "001"), ("sample2.wav", "birds chirping", "002"))
EVAL_SEED = 42   # the reference generates every evaluated image from this seed


def image_to_u8(image) -> torch.Tensor:
    """A PIL image, a path, or a uint8 array / tensor [H, W, 3] or [1, H, W, 3] -> uint8 tensor [1, H, W, 3]."""
    if isinstance(image, (str, os.PathLike)):
        from PIL import Image
        image = Image.open(image)
    if hasattr(image, "convert"):
        image = np.array(image.convert("RGB"), dtype=np.uint8)
    t = torch.as_tensor(image)
    if t.dim() == 3:
        t = t[None]
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[0] != 1 or t.shape[-1] != 3:
        raise ValueError(f"an image must be a PIL image, a path or a uint8 array [H, W, 3], got {t.dtype} "
                         f"{tuple(t.shape)}")
    return t


class Evaluator:
    def __init__(self, checkpoint_dir="../checkpoints", pipeline=None, scorer=None, clip_model_path=None,
                 batch: int = 4, sampler: str | None = None, **pipeline_kwargs):
        """pipeline / scorer: injected instances (tests, or a pipeline that is already loaded); by default the
        pipeline is AudioToImageInference(checkpoint_dir, **pipeline_kwargs) and the scorer a ClipScorer built on
        first use from clip_model_path (None: the seeded recipe) with the pipeline's tokenizer.  batch: requests
        per generate call in evaluate_dataset.  sampler: passed to every generate call as sampler= when given
        (None: the pipeline's default, DDIM)."""
        self.checkpoint_dir = Path(checkpoint_dir)
        if pipeline is None:
            from .pipeline import AudioToImageInference
            pipeline = AudioToImageInference(checkpoint_dir, **pipeline_kwargs)
        self.pipeline = pipeline
        self._scorer = scorer
        self.clip_model_path = clip_model_path
        self.batch = max(1, int(batch))
        self.generate_kwargs = {"sampler": sampler} if sampler is not None else {}

        self.metrics = {name: [] for name in METRIC_NAMES}

    @property
    def scorer(self):
        if self._scorer is None:
            from .clip_score import ClipScorer
            self._scorer = ClipScorer(self.pipeline.device, self.clip_model_path, seed=getattr(self.pipeline, "seed", 0),
                                      tokenizer=getattr(self.pipeline, "tokenizer", None))
        return self._scorer

    def _scores(self, images_u8: torch.Tensor, texts: list[str]) -> list[float]:
        return [float(s) for s in self.scorer.score(images_u8, self.scorer.tokenize(texts)).tolist()]

    def compute_clip_score(self, image, text):
        """The cosine between the CLIP embeddings of image (a PIL image, a path or a uint8 array) and text, as a
        Python float."""
        return self._scores(image_to_u8(image), [text])[0]

    def evaluate_single(self, audio_path, text_prompt, reference_image=None):
        """One request -> {"clip_score", "generated_image" (PIL)} and, with a reference image (a PIL image, a path
        or a uint8 array of any size), "image_similarity"."""
        images = self.pipeline.batch_generate_u8([audio_path], [text_prompt], seed=EVAL_SEED, **self.generate_kwargs)
        result = {"clip_score": self._scores(images, [text_prompt])[0],
                  "generated_image": self.pipeline.to_pil(images)[0]}
        if reference_image is not None:
            sim = self.scorer.image_similarity(images, image_to_u8(reference_image))
            result["image_similarity"] = float(sim[0])
        return result

    @staticmethod
    def load_metadata(data_dir: Path) -> list[dict]:
        """data_dir/metadata.json (a list of {"audio", "text", "id"}), else the reference's two dummy entries."""
        path = data_dir / "metadata.json"
        if path.exists():
            return json.loads(path.read_text())
        return [dict(audio=a, text=t, id=i) for a, t, i in DUMMY_METADATA]

    def evaluate_dataset(self, data_dir, output_dir="evaluation_results"):
        """Every entry of the metadata whose data_dir/audio/<audio> exists: generated `batch` at a time, scored on
        the device, saved as output_dir/<id>_generated.png.  Writes output_dir/evaluation_results.json
        ({"individual_results": [...], "average_metrics": {name, name_std}}, plain floats) and returns the
        averages."""
        data_dir, output_dir = Path(data_dir), Path(output_dir)
        output_dir.mkdir(parents=True, exist_ok=True)
        metadata = self.load_metadata(data_dir)
        print(f"Evaluating {len(metadata)} samples...")
        found = []
        for entry in metadata:
            audio_path = data_dir / "audio" / entry["audio"]
            if audio_path.exists():
                found.append((entry, audio_path))
            else:
                print(f"Warning: {audio_path} not found, skipping...")
        individual = []
        for start in range(0, len(found), self.batch):
            chunk = found[start:start + self.batch]
            texts = [entry["text"] for entry, _ in chunk]
            images = self.pipeline.batch_generate_u8([path for _, path in chunk], texts, seed=EVAL_SEED, **self.generate_kwargs)
            scores = self._scores(images, texts)
            for (entry, _), score, pil in zip(chunk, scores, self.pipeline.to_pil(images)):
                pil.save(output_dir / f"{entry['id']}_generated.png")
                self.metrics["clip_score"].append(score)
                individual.append({"id": entry["id"], "audio": entry["audio"], "text": entry["text"],
                                   "clip_score": score})
        averages = {}
        for name, values in self.metrics.items():
            if values:
                averages[name] = float(np.mean(values))
                averages[name + "_std"] = float(np.std(values))
        with open(output_dir / "evaluation_results.json", "w") as f:
            json.dump({"individual_results": individual, "average_metrics": averages}, f, indent=2)
        return averages

    def print_results(self, metrics):
        """The averages as `name: mean ± std` lines."""
        bar = "=" * 60
        print(f"\n{bar}\nEvaluation Results\n{bar}")
        for name in (k for k in metrics if not k.endswith("_std")):
            spread = f" ± {metrics[name + '_std']:.4f}" if name + "_std" in metrics else ""
            print(f"{name:20}: {metrics[name]:.4f}{spread}")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Evaluate CLAP2Diffusion (MI355X HIP path)")
    ap.add_argument("--data_dir", type=str, default="../data/audiocaps/test", help="Path to test data directory")
    ap.add_argument("--checkpoint_dir", type=str, default="../checkpoints", help="Path to checkpoint directory")
    ap.add_argument("--output_dir", type=str, default="evaluation_results", help="Output directory for results")
    ap.add_argument("--sd_model", type=str, default=None, help="diffusers-format SD1.5 folder (unet/, vae/, text_encoder/)")
    ap.add_argument("--clap_model", type=str, default=None, help="ClapModel weights file or folder")
    ap.add_argument("--clip_model", type=str, default=None, help="CLIPModel (ViT-L/14) weights file or folder")
    ap.add_argument("--batch", type=int, default=4, help="Requests per generate call")
    return ap


def main():
    args = build_parser().parse_args()
    bar = "=" * 60
    print(f"\n{bar}\nCLAP2Diffusion Evaluation\n{bar}\n")
    print(f"Data directory: {args.data_dir}\nCheckpoint directory: {args.checkpoint_dir}\n"
          f"Output directory: {args.output_dir}\n")
    evaluator = Evaluator(checkpoint_dir=args.checkpoint_dir, clip_model_path=args.clip_model, batch=args.batch,
                          sd_model_path=args.sd_model, clap_model_path=args.clap_model)
    evaluator.print_results(evaluator.evaluate_dataset(data_dir=args.data_dir, output_dir=args.output_dir))
    print(f"\nEvaluation complete. Results saved to {args.output_dir}")


if __name__ == "__main__":
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    main()
