"""bench.py's output dump (--dump-outputs) and option surface, without a GPU."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def test_dump_outputs_writes_float32_arrays(tmp_path):
    img = torch.arange(2 * 4 * 4 * 3, dtype=torch.int64).reshape(2, 4, 4, 3).to(torch.uint8)
    lat = torch.linspace(-3, 3, 2 * 4 * 2 * 2).reshape(2, 4, 2, 2).half()
    bench.dump_outputs(tmp_path / "d", {"images": img, "latents": lat})
    got_i, got_l = np.load(tmp_path / "d" / "images.npy"), np.load(tmp_path / "d" / "latents.npy")
    assert got_i.dtype == np.float32 and got_l.dtype == np.float32
    assert got_i.shape == (2, 4, 4, 3) and got_l.shape == (2, 4, 2, 2)
    assert np.array_equal(got_i, img.numpy().astype(np.float32))
    assert np.array_equal(got_l, lat.float().numpy())


def test_dump_outputs_samples_a_large_array_at_fixed_positions(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 100)
    t = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    bench.dump_outputs(tmp_path / "a", {"x": t})
    bench.dump_outputs(tmp_path / "b", {"x": t + 0.5})
    a, b = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert a.shape == (100,) and a.dtype == np.float32
    assert len(set(a.tolist())) == 100 and np.all(np.diff(a) > 0)   # distinct positions, in order
    assert np.array_equal(b - a, np.full(100, 0.5, np.float32))     # the same positions in both runs
    # the default cap keeps the two arrays of a run (images, latents) under 64 MB even if both hit it,
    # and writes the c3 batch's images (8 x 512 x 512 x 3) whole
    monkeypatch.undo()
    assert 2 * 4 * bench.DUMP_MAX_ELEMS <= 64 * 10 ** 6
    assert 8 * 512 * 512 * 3 <= bench.DUMP_MAX_ELEMS


def test_options():
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--help"], capture_output=True, text=True, check=True).stdout
    for opt in ("--gpus", "--steps", "--warmup", "--dump-outputs", "--full"):
        assert opt in out
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--steps" in r.stderr
