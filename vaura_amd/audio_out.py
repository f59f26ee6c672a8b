"""Host arithmetic of the audio output (csrc/audio_out.hip, vaura_amd/post.py): which output samples of a 44.1 kHz -> ``rate`` stream
can leave once ``received`` input samples are there, and how much input history the next block needs.  Pure integer functions of the
table ``audio_preprocess.resample_table(44100, rate)``; no device.

Output ``m = q n + p`` reads the ``T`` input samples ``start(m) .. last(m)``, ``start(m) = q o + first[p] - w`` and ``last(m) =
start(m) + T - 1`` (the zero taps behind a phase's shorter run included: the kernel multiplies them too).  Both advance by ``o`` per
period of ``n`` outputs, so one period of the table decides everything.

  ``output_total(N)``     ``ceil(n N / o)``: the outputs of a clip of N samples (``audio_preprocess.output_length``);
  ``releasable(r)``       the largest M with ``last(m') < r`` for every ``m' < M`` — a prefix rule, so nothing rests on ``last`` being
                          monotone;
  ``history()``           the smallest H with ``start(m) >= r - H`` for every r and every ``m >= releasable(r)``: what the carry row
                          holds.  Exact, from one period.
The codec's own rate (``rate == 44100``) is the identity: ``releasable(r) = r``, no history.
"""
from __future__ import annotations

import bisect
from typing import Dict, List

from . import _lib as L
from . import audio_preprocess as AP

SOURCE_RATE = 44100                  # the codec's rate (dac_8kbps_wrapper.yaml): the rows the output side starts from
TILE = 1024                          # VAURA_AUDIO_OUT_TILE (include/vaura_hip.h): output samples per workgroup
RECORD = 5                           # VAURA_AUDIO_OUT_RECORD: r0, L, m0, count, N of one clip
MAX_CHANNELS = 8


class OutputPlan:
    """The integer side of one rate pair ``source -> rate``."""

    def __init__(self, rate: int, source: int = SOURCE_RATE):
        if isinstance(rate, bool) or not isinstance(rate, int) or rate < 1:
            raise L.VauraHipError(f"the output rate must be a positive integer (Hz), got {rate!r}")
        self.rate, self.source = rate, int(source)
        self.o, self.n, self.w = AP.rate_ratio(self.source, rate)
        self.identity = self.o == self.n
        if self.identity:
            self.table, self.T, self.first = None, 0, []
            self._start, self._prefix_last = [0], [0]
            return
        self.table = AP.resample_table(self.source, rate)               # refuses what the kernel refuses: > 64 taps, > 2^20 entries
        self.T = int(self.table["taps"])
        self.first = [int(v) for v in self.table["first"].tolist()]
        self._start = [f - self.w for f in self.first]                    # start(p) of the first period
        running, self._prefix_last = None, []                             # max of last(0 .. p): non-decreasing, so it can be bisected
        for s in self._start:
            running = s + self.T - 1 if running is None else max(running, s + self.T - 1)
            self._prefix_last.append(running)
        self._history = None

    def start(self, m: int) -> int:
        if self.identity:
            return m
        q, p = divmod(m, self.n)
        return q * self.o + self._start[p]

    def last(self, m: int) -> int:
        return self.start(m) + max(self.T, 1) - 1

    def output_total(self, n_samples: int) -> int:
        return AP.output_length(n_samples, self.source, self.rate)

    def releasable(self, received: int) -> int:
        if received <= 0:
            return 0
        if self.identity:
            return received
        # every output of the periods q < q0 has last(m) <= q o + max last of a period < received
        q = max(0, (received - 1 - self._prefix_last[-1]) // self.o + 1)
        while True:
            c = bisect.bisect_left(self._prefix_last, received - q * self.o)   # the p with prefix max last(q n .. q n + p) < received
            if c < self.n:
                return q * self.n + c
            q += 1

    def history(self) -> int:
        if self.identity:
            return 0
        if self._history is None:
            o, n = self.o, self.n
            # lowest start among the outputs m .. of the stream, for m in two periods: start(m + n) = start(m) + o > start(m), so
            # the n outputs from m on decide
            two = self._start + [s + o for s in self._start] + [s + 2 * o for s in self._start]
            low = list(two)
            for i in range(len(low) - 2, -1, -1):
                low[i] = min(low[i], low[i + 1])
            base = (self._prefix_last[-1] // o + 2) * o                   # a whole period of `received` away from the stream's start
            worst = 0
            for r in range(base, base + o):
                m = self.releasable(r)
                q, p = divmod(m, n)
                worst = max(worst, r - (q * o + low[p]))
            self._history = worst
        return self._history


_plans: Dict[int, OutputPlan] = {}


def plan(rate: int) -> OutputPlan:
    if isinstance(rate, bool) or not isinstance(rate, int) or rate not in _plans:     # 48000.0 == 48000 must not find the cached plan
        _plans[rate] = OutputPlan(rate)
    return _plans[rate]


def output_total(n_samples: int, rate: int) -> int:
    return plan(rate).output_total(n_samples)


def releasable(received: int, rate: int) -> int:
    return plan(rate).releasable(received)


def history(rate: int) -> int:
    return plan(rate).history()


def push_records(pl: OutputPlan, received: List[int], emitted: List[int], samples: List[int], final: List[bool]):
    """One push of a stream as the launch takes it: -> (records [[r0, L, m0, count, N]] per clip, new received, new emitted)."""
    recs, new_r, new_e = [], [], []
    for r0, m0, n_new, fin in zip(received, emitted, samples, final):
        r1 = r0 + n_new
        target = pl.output_total(r1) if fin else min(pl.releasable(r1), pl.output_total(r1))
        target = max(target, m0)
        recs.append([r0, n_new, m0, target - m0, r1 if fin else -1])
        new_r.append(r1)
        new_e.append(target)
    return recs, new_r, new_e
