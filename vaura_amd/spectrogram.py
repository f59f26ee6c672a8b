"""Host side of the spectrogram (csrc/spectrogram.hip, vaura_amd/post.py): the integer plan of a stream of columns and the three tables
the kernel reads.  Pure host code; no device.

Column ``t`` of a clip is centred on sample ``hop t + hop/2`` and covers ``lo(t) = hop t + hop/2 - n_fft/2 .. lo(t) + n_fft - 1``; a clip
of ``n`` samples has ``ceil(n / hop)`` columns (one per codec frame at hop 512).

  ``columns(n)``          ``ceil(n / hop)``;
  ``releasable(r)``       the columns whose window's last sample has arrived: column t once ``r >= hop t + hop/2 + n_fft/2``;
  ``history()``           ``n_fft - 1``: the first unreleased column t* has ``hop t* > r - hop/2 - n_fft/2``, so ``lo(t*) >= r - n_fft + 1``.

Tables, all built in float64 and rounded once to fp32: the periodic Hann window, the twiddles ``e^{-2 pi i t / n_fft}`` for
``t < 3 n_fft / 4``, and the triangular mel filters as a compact table (first bin, count, offset per filter; weights packed).  The
filters follow the published formulas (Slaney's Auditory Toolbox scale: linear below 1 kHz, 15 mel at 1 kHz, logarithmic above with
27 steps per factor 6.4; HTK: ``2595 log10(1 + f / 700)``); torchaudio and librosa are absent here, so their parity is UNPINNED.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L

SAMPLE_RATE = 44100                  # the codec's rate
RECORD = 5                           # VAURA_SPECTROGRAM_RECORD: r0, L, t0, count, N of one clip
SIZES = (512, 1024, 2048)
MAX_MELS = 256                       # VAURA_SPECTROGRAM_MAX_MELS
SCALES = {"power": 0, "db": 1, "log": 2, "complex": 3}      # VAURA_SPEC_POWER / DB / LOG / COMPLEX


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


class SpectrogramPlan:
    """The integer side of one (n_fft, hop) pair."""

    def __init__(self, n_fft: int = 2048, hop: int = 512):
        if not _is_int(n_fft) or n_fft not in SIZES:
            raise L.VauraHipError(f"VAURA_ERR_SHAPE: n_fft must be one of {SIZES}, got {n_fft!r}")
        if not _is_int(hop) or hop < 1 or hop > n_fft or hop & (hop - 1):
            raise L.VauraHipError(f"VAURA_ERR_SHAPE: hop must be a power of two and at most n_fft = {n_fft}, got {hop!r}")
        self.n_fft, self.hop = n_fft, hop

    def lo(self, t: int) -> int:
        return self.hop * t + self.hop // 2 - self.n_fft // 2

    def columns(self, n: int) -> int:
        return -(-max(n, 0) // self.hop)

    def releasable(self, received: int) -> int:
        return max(0, (received - self.hop // 2 - self.n_fft // 2) // self.hop + 1)

    def history(self) -> int:
        return self.n_fft - 1


def push_records(pl: SpectrogramPlan, received: List[int], emitted: List[int], samples: List[int], final: List[bool]):
    """One push of a stream as the launch takes it: -> (records [[r0, L, t0, count, N]] per clip, new received, new emitted)."""
    recs, new_r, new_e = [], [], []
    for r0, t0, n_new, fin in zip(received, emitted, samples, final):
        r1 = r0 + n_new
        target = pl.columns(r1) if fin else min(pl.releasable(r1), pl.columns(r1))
        target = max(target, t0)
        recs.append([r0, n_new, t0, target - t0, r1 if fin else -1])
        new_r.append(r1)
        new_e.append(target)
    return recs, new_r, new_e


def window(n_fft: int) -> torch.Tensor:
    """The periodic Hann window ``0.5 - 0.5 cos(2 pi i / n_fft)`` in float64, rounded once to fp32."""
    i = torch.arange(n_fft, dtype=torch.float64)
    return i.mul(math.pi * 2.0 / n_fft).cos().mul(-0.5).add(0.5).to(torch.float32)


def twiddles(n_fft: int) -> torch.Tensor:
    """(3 n_fft / 4, 2) fp32: cos and -sin of ``2 pi t / n_fft``.  The quarter-turn multiples are exact."""
    t = np.arange(3 * n_fft // 4, dtype=np.float64)
    ang = 2.0 * np.pi * t / n_fft
    tw = np.stack([np.cos(ang), -np.sin(ang)], axis=1)
    q = n_fft // 4
    tw[0], tw[q], tw[2 * q] = (1.0, -0.0), (0.0, -1.0), (-1.0, -0.0)
    return torch.from_numpy((tw + 0.0).astype(np.float32))


def hz_to_mel(f, mel_scale: str = "slaney"):
    f = np.asarray(f, dtype=np.float64)
    if mel_scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    lin = 3.0 * f / 200.0
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) * (27.0 / np.log(6.4)), lin)


def mel_to_hz(m, mel_scale: str = "slaney"):
    m = np.asarray(m, dtype=np.float64)
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), 200.0 * m / 3.0)


def mel_filters(n_fft: int, n_mels: int, f_min: float = 0.0, f_max: Optional[float] = None, mel_scale: str = "slaney",
                norm: Optional[str] = None, sample_rate: int = SAMPLE_RATE) -> np.ndarray:
    """(n_mels, n_fft/2 + 1) float64: triangle m rises from centre m-1 to centre m and falls to centre m+1, the centres equally spaced
    in mel between ``f_min`` and ``f_max``; ``norm="slaney"`` scales triangle m by ``2 / (f[m+2] - f[m])`` (unit area in Hz)."""
    if mel_scale not in ("slaney", "htk"):
        raise L.VauraHipError(f"mel_scale must be 'slaney' or 'htk', got {mel_scale!r}")
    if norm not in (None, "slaney"):
        raise L.VauraHipError(f"norm must be None or 'slaney', got {norm!r}")
    if not _is_int(n_mels) or not 1 <= n_mels <= MAX_MELS:
        raise L.VauraHipError(f"VAURA_ERR_SHAPE: n_mels must lie in 1 .. {MAX_MELS}, got {n_mels!r}")
    f_max = sample_rate / 2.0 if f_max is None else float(f_max)
    f_min = float(f_min)
    if not 0.0 <= f_min < f_max <= sample_rate / 2.0:
        raise L.VauraHipError(f"the mel range must satisfy 0 <= f_min < f_max <= {sample_rate / 2.0}, got {f_min} .. {f_max}")
    bins = np.arange(n_fft // 2 + 1, dtype=np.float64) * (sample_rate / n_fft)
    pts = mel_to_hz(np.linspace(float(hz_to_mel(f_min, mel_scale)), float(hz_to_mel(f_max, mel_scale)), n_mels + 2), mel_scale)
    up = (bins[None, :] - pts[:-2, None]) / (pts[1:-1] - pts[:-2])[:, None]
    down = (pts[2:, None] - bins[None, :]) / (pts[2:] - pts[1:-1])[:, None]
    fb = np.maximum(0.0, np.minimum(up, down))
    if norm == "slaney":
        fb = fb * (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return fb


def compact(fb32: np.ndarray) -> Dict[str, torch.Tensor]:
    """A dense (F, bins) fp32 filterbank -> the table the kernel takes: ``bins`` (F, 3) int32 (first bin, count, offset) and ``weights``
    (sum of counts) fp32, every filter's span first non-zero .. last non-zero.  A filter without a non-zero weight is refused."""
    rows, weights, at = [], [], 0
    for m, row in enumerate(fb32):
        nz = np.nonzero(row)[0]
        if nz.size == 0:
            raise L.VauraHipError(f"VAURA_ERR_SHAPE: mel filter {m} of {fb32.shape[0]} has no non-zero weight on {fb32.shape[1]} bins "
                                  "(fewer filters, a larger n_fft or a narrower range)")
        first, count = int(nz[0]), int(nz[-1] - nz[0] + 1)
        rows.append([first, count, at])
        weights.append(row[first:first + count])
        at += count
    return {"bins": torch.tensor(rows, dtype=torch.int32), "weights": torch.from_numpy(np.concatenate(weights).astype(np.float32))}


def expand(table: Dict[str, torch.Tensor], n_bins: int) -> torch.Tensor:
    """The dense (F, n_bins) fp32 matrix of a compact table."""
    out = torch.zeros(table["bins"].shape[0], n_bins, dtype=torch.float32)
    for m, (first, count, at) in enumerate(table["bins"].tolist()):
        out[m, first:first + count] = table["weights"][at:at + count]
    return out


def mel_table(n_fft: int, n_mels: int, f_min: float = 0.0, f_max: Optional[float] = None, mel_scale: str = "slaney",
              norm: Optional[str] = None, sample_rate: int = SAMPLE_RATE) -> Dict[str, torch.Tensor]:
    """The filters of ``mel_filters`` rounded once to fp32, as the compact table."""
    return compact(mel_filters(n_fft, n_mels, f_min, f_max, mel_scale, norm, sample_rate).astype(np.float32))
