"""Audio in: the containers decoded without librosa (RIFF/WAVE, AIFF / AIFC, Sun AU) and the synthetic clip that
stands in for the reference's LFS-stub asset."""
from __future__ import annotations

import warnings
from pathlib import Path

import numpy as np

SR = 48000


def synthetic_thunder(seed: int = 0, seconds: float = 10.0, sr: int = SR) -> np.ndarray:
    """SURVEY.md §8(d) stand-in for the LFS-stub assets/Thunder.wav: low-passed white
    noise with three exponentially decaying bursts, peak-normalised."""
    from scipy.signal import lfilter
    rs = np.random.RandomState(seed)
    n = int(seconds * sr)
    y = lfilter([0.005], [1.0, -0.995], rs.randn(n))  # 1-pole IIR low-pass, a = 0.995
    t = np.arange(n) / sr
    env = 0.05 + sum(np.where(t >= t0, np.exp(-(t - t0) / 0.6), 0.0) for t0 in (1.0, 4.5, 7.0))
    y = y * env
    return (y / (np.abs(y).max() + 1e-8)).astype(np.float32)


_WAVE_PCM, _WAVE_FLOAT, _WAVE_EXTENSIBLE = 1, 3, 0xFFFE


def _read_wav(path: str, max_seconds: float | None = None) -> tuple[np.ndarray, int]:
    """RIFF/WAVE reader -> (mono float32 in [-1, 1], native rate): PCM 8 (unsigned) / 16 / 24 / 32-bit,
    IEEE float 32 / 64-bit, WAVE_FORMAT_EXTENSIBLE of either; channels averaged (librosa mono=True).
    max_seconds: keep the first max_seconds of the file at its native rate (librosa's duration=,
    applied before resampling as librosa.load does).  read_audio adds AIFF / AIFC and Sun AU; other
    containers (mp3, flac, ...) need a decoder this image does not have: convert them first."""
    data = Path(path).read_bytes()
    if data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file (only WAV is decoded without librosa)")
    fmt = None
    pos = 12
    body = None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], int.from_bytes(data[pos + 4:pos + 8], "little")
        chunk = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            tag, ch, sr = int.from_bytes(chunk[0:2], "little"), int.from_bytes(chunk[2:4], "little"), \
                int.from_bytes(chunk[4:8], "little")
            bits = int.from_bytes(chunk[14:16], "little")
            if tag == _WAVE_EXTENSIBLE and len(chunk) >= 26:
                tag = int.from_bytes(chunk[24:26], "little")   # first two bytes of the SubFormat GUID
            fmt = (tag, ch, sr, bits)
        elif cid == b"data":
            body = chunk
        pos += 8 + size + (size & 1)
    if fmt is None or body is None:
        raise ValueError(f"{path}: WAV without fmt / data chunk")
    tag, ch, sr, bits = fmt
    bps = bits // 8
    frames = len(body) // (bps * ch)
    if max_seconds is not None:
        frames = min(frames, int(max_seconds * sr))
    body = body[: frames * bps * ch]
    if tag == _WAVE_FLOAT and bits in (32, 64):
        x = np.frombuffer(body, dtype=np.float32 if bits == 32 else np.float64).astype(np.float32)
    elif tag == _WAVE_PCM and bits == 8:
        x = (np.frombuffer(body, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif tag == _WAVE_PCM and bits in (16, 32):
        x = np.frombuffer(body, dtype=np.int16 if bits == 16 else np.int32).astype(np.float32) / float(2 ** (bits - 1))
    elif tag == _WAVE_PCM and bits == 24:
        b = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) / float(1 << 23)
    else:
        raise ValueError(f"{path}: unsupported WAV encoding (format tag {tag}, {bits} bits)")
    return x.reshape(-1, ch).mean(axis=1), sr


def _pcm_to_float(raw: bytes, width: int, big: bool) -> np.ndarray:
    """Signed linear PCM of `width` bytes per sample -> float32 in [-1, 1)."""
    if width == 1:
        return np.frombuffer(raw, dtype=np.int8).astype(np.float32) / 128.0
    if width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = (b[:, 0] << 16 | b[:, 1] << 8 | b[:, 2]) if big else (b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16)
        return (np.where(v >= 1 << 23, v - (1 << 24), v)).astype(np.float32) / float(1 << 23)
    dt = {2: "i2", 4: "i4"}[width]
    return np.frombuffer(raw, dtype=(">" if big else "<") + dt).astype(np.float32) / float(2 ** (8 * width - 1))


def _read_stdlib(mod, path: str, max_seconds: float | None) -> tuple[np.ndarray, int]:
    """AIFF / AIFC (aifc) and Sun AU (sunau) through the standard library's readers: linear PCM
    8 / 16 / 24 / 32-bit (big-endian; AIFC 'sowt' comes back big-endian from aifc) and the
    companded codecs those modules expand to native-endian 16-bit (u-law / a-law / G.722)."""
    with mod.open(path, "rb") as f:
        ch, width, sr, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        if max_seconds is not None:
            n = min(n, int(max_seconds * sr))
        raw = f.readframes(n)
        comp = f.getcomptype()
    comp = comp.decode() if isinstance(comp, bytes) else str(comp)
    big = comp.upper() in ("NONE", "SOWT") or comp == "not compressed"
    if width not in (1, 2, 3, 4):
        raise ValueError(f"{path}: unsupported sample width {width}")
    x = _pcm_to_float(raw[: len(raw) // (width * ch) * width * ch], width, big)
    return x.reshape(-1, ch).mean(axis=1), sr


def read_audio(path: str, max_seconds: float | None = None) -> tuple[np.ndarray, int]:
    """(mono float32, native rate) of a WAV, AIFF / AIFC or Sun AU file, chosen by its header (the
    containers this image decodes without librosa; reference scripts/inference.py:78 reads any
    format librosa does).  max_seconds: keep the first max_seconds at the native rate."""
    head = Path(path).read_bytes()[:12]
    if head[:4] == b"RIFF" and head[8:12] == b"WAVE":
        return _read_wav(path, max_seconds)
    with warnings.catch_warnings():   # aifc / sunau are deprecated from Python 3.11 on
        warnings.simplefilter("ignore", DeprecationWarning)
        if head[:4] == b"FORM" and head[8:12] in (b"AIFF", b"AIFC"):
            import aifc
            return _read_stdlib(aifc, path, max_seconds)
        if head[:4] == b".snd":
            import sunau
            return _read_stdlib(sunau, path, max_seconds)
    raise ValueError(f"{path}: not a RIFF/WAVE, AIFF/AIFC or Sun AU file (other formats need a decoder this "
                     "image does not have: convert them first)")
