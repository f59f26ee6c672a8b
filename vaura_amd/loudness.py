"""Host side of the streaming loudness meter and the causal normaliser (csrc/loudness.hip, vaura_amd/post.py): the integer plan of a
stream of steps, the K-weighting coefficients and the chunk tables the kernel reads.  Pure host code; no device.

``step = nearbyint(0.1 rate)`` samples (100 ms), ``gate = 4 step`` (the 400 ms gating block of ITU-R BS.1770).  A rate is served when
``nearbyint(0.4 rate) == 4 step`` (11 025 Hz is not) and it lies in 8 .. 48 kHz.

K-weighting: the treble shelf (+4 dB, 1500 Hz, Q = 1/sqrt 2) and the high-pass (38 Hz, Q = 0.5) of csrc/post.hip's launcher, derived
in float64 and kept in float64.  Each biquad ``y[i] = b0 x[i] + b1 x[i-1] + b2 x[i-2] - a1 y[i-1] - a2 y[i-2]`` is linear in its
y-state, so a step is cut into ``C = ceil(step / L)`` chunks of ``L = ceil(step / lanes)`` samples; with ``s = (y[-1], y[-2])`` the state
in front of a chunk, ``y[i] = zs[i] + h1[i] s1 + h2[i] s2`` (``zs``: the chunk run from a zero state) and the state behind a chunk of
``n`` samples is ``(zs[n-1], zs[n-2]) + M(n) s``, ``M(n) = [[h1[n-1], h2[n-1]], [h1[n-2], h2[n-2]]]`` with ``h1[-1] = 1, h2[-1] = 0``.

  ``table()``     float64: the ten coefficients, then per stage ``h1`` (L), ``h2`` (L), ``M(L)`` (4), ``M(step - (C-1) L)`` (4);
  ``push_records`` one push of a stream as the launch takes it.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import numpy as np

from . import _lib as L_

RECORD = 2                           # VAURA_LOUDNESS_RECORD: r0, n of one clip
LANES = 256                          # threads of the push kernel's workgroup
MIN_HISTORY, MAX_HISTORY = 8, 4096   # VAURA_LOUDNESS_MIN_HISTORY / MAX_HISTORY (4096 = post.hip's LOUD_MAX_STEPS)
MIN_RATE, MAX_RATE = 8000, 48000
FUSE_MAX = 16384                     # samples per row up to which a push is one launch (LOUD_FUSE_MAX)
SHORT_TERM_STEPS = 30                # EBU Tech 3341: 3 s
LIMITERS = {"clip": 0, "tanh": 1}    # VAURA_LOUDNESS_CLIP / TANH


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def step_of(rate: int) -> int:
    """``nearbyint(0.1 rate)``, or a refusal: a rate outside 8 .. 48 kHz, or one whose gating block is not four whole steps."""
    if not _is_int(rate) or not MIN_RATE <= rate <= MAX_RATE:
        raise L_.VauraHipError(f"VAURA_ERR_SHAPE: the loudness meter serves {MIN_RATE} .. {MAX_RATE} Hz, got {rate!r}")
    step = int(np.rint(0.1 * rate))                                       # halves to even, as nearbyint
    if int(np.rint(0.4 * rate)) != 4 * step:
        raise L_.VauraHipError(f"VAURA_ERR_SHAPE: at {rate} Hz the 400 ms gating block is not four whole 100 ms steps")
    return step


def k_weighting(rate: int) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """((b0, b1, b2, a1, a2) of the shelf, the same of the high-pass), normalised by a0, float64."""
    w0 = 2.0 * math.pi * 1500.0 / rate
    A = math.exp(4.0 / 40.0 * math.log(10.0))
    alpha = math.sin(w0) / 2.0 / (1.0 / math.sqrt(2.0))
    t1, t2, t3 = 2.0 * math.sqrt(A) * alpha, (A - 1.0) * math.cos(w0), (A + 1.0) * math.cos(w0)
    b0, b1, b2 = A * ((A + 1.0) + t2 + t1), -2.0 * A * ((A - 1.0) + t3), A * ((A + 1.0) + t2 - t1)
    a0, a1, a2 = (A + 1.0) - t2 + t1, 2.0 * ((A - 1.0) - t3), (A + 1.0) - t2 - t1
    shelf = (b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0)
    w0 = 2.0 * math.pi * 38.0 / rate
    alpha = math.sin(w0) / 2.0 / 0.5
    b0 = (1.0 + math.cos(w0)) / 2.0
    b1, b2, a0, a1, a2 = -1.0 - math.cos(w0), b0, 1.0 + alpha, -2.0 * math.cos(w0), 1.0 - alpha
    return shelf, (b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0)


def homogeneous(a1: float, a2: float, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """(h1, h2), n values each: the outputs of ``y[i] = -a1 y[i-1] - a2 y[i-2]`` from the states (1, 0) and (0, 1)."""
    h = np.zeros((2, n))
    for k, (p1, p2) in enumerate(((1.0, 0.0), (0.0, 1.0))):
        for i in range(n):
            v = -a1 * p1 - a2 * p2
            h[k, i] = v
            p2, p1 = p1, v
    return h[0], h[1]


def transition(h1: np.ndarray, h2: np.ndarray, n: int) -> np.ndarray:
    """M(n), row-major: the state behind n samples of the homogeneous system as a function of the state in front of them."""
    at = lambda h, i, first: float(h[i]) if i >= 0 else first            # noqa: E731  (h[-1]: the state itself)
    return np.array([at(h1, n - 1, 1.0), at(h2, n - 1, 0.0), at(h1, n - 2, 1.0), at(h2, n - 2, 0.0)])


class LoudnessPlan:
    """The integer side of one rate, its coefficients and its chunk tables."""

    def __init__(self, rate: int = 44100, lanes: int = LANES):
        self.step = step_of(rate)
        if not _is_int(lanes) or lanes < 1:
            raise L_.VauraHipError(f"lanes must be a positive integer, got {lanes!r}")
        self.rate, self.gate, self.lanes = rate, 4 * self.step, lanes
        self.L = -(-self.step // lanes)                                   # samples of a chunk
        self.C = -(-self.step // self.L)                                  # chunks of a step
        self.last = self.step - (self.C - 1) * self.L                     # samples of a step's last chunk
        self.shelf, self.highpass = k_weighting(rate)
        self._table = None

    def table(self) -> np.ndarray:
        if self._table is None:
            parts = [np.array(self.shelf + self.highpass)]
            for co in (self.shelf, self.highpass):
                h1, h2 = homogeneous(co[3], co[4], self.L)
                parts += [h1, h2, transition(h1, h2, self.L), transition(h1, h2, self.last)]
            self._table = np.concatenate(parts).astype(np.float64)
        return self._table

    def boundaries(self, received: int) -> int:
        """whole steps among the first ``received`` samples: the boundaries 1 .. that many have been reached"""
        return max(received, 0) // self.step

    def blocks(self, received: int) -> int:
        """complete 400 ms gating blocks among the first ``received`` samples"""
        return max(0, self.boundaries(received) - 3)

    def windows(self, received: int) -> int:
        """complete 3 s short-term windows among the first ``received`` samples"""
        return max(0, self.boundaries(received) - SHORT_TERM_STEPS + 1)


def check_history(history_steps) -> int:
    if not _is_int(history_steps) or not MIN_HISTORY <= history_steps <= MAX_HISTORY:
        raise L_.VauraHipError(f"VAURA_ERR_SHAPE: history_steps must lie in {MIN_HISTORY} .. {MAX_HISTORY}, got {history_steps!r}")
    return history_steps


def push_records(pl: LoudnessPlan, received: List[int], samples: List[int]) -> Dict[str, List]:
    """One push of a stream as the launch takes it: ``records`` [[r0, n]] per clip, the ``received`` counts after it, and per clip how
    many ``boundaries`` the push reaches, how many gating ``blocks`` and short-term ``windows`` it completes; ``stride``: the rows of the
    meter's planes (the most boundaries of any clip, at least 1)."""
    recs, new_r, nb, blocks, windows = [], [], [], [], []
    for r0, n in zip(received, samples):
        r1 = r0 + n
        recs.append([r0, n])
        new_r.append(r1)
        nb.append(pl.boundaries(r1) - pl.boundaries(r0))
        blocks.append(pl.blocks(r1) - pl.blocks(r0))
        windows.append(pl.windows(r1) - pl.windows(r0))
    return {"records": recs, "received": new_r, "boundaries": nb, "blocks": blocks, "windows": windows, "stride": max(max(nb), 1)}
