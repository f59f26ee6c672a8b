"""Adversarial rows for csrc/step.hip sample_kernel and a plain reference of its token (tests/test_sampler_edges_host.py checks both on
the CPU, tests/test_gpu_sampler_edges.py runs the rows on the device).

The reference restates oracle/sampling_oracle.py::next_token with ONE difference: the top-p sort is stable
(``torch.sort(descending=True, stable=True)``), which is the kernel's documented "ties: lower id first".  It also takes rows that
already are probabilities (``input_is_probs``: utils/utils.py sample_top_k / sample_top_p take probabilities) and clamps top_k to V.

How a row pins a rule.  The kernel draws argmax(p / q) from an explicit noise tensor.  Every row has q = 1 everywhere except q = 1e-4
on ONE slot (a token; under top-p a rank, because the noise is indexed by rank there).  That slot wins by a factor of about 1e4 if
and only if the rule under test keeps it, so the expected token follows from the structure of the row — it is written down by the
builder, not computed — and never from how expf or a sum rounds in fp32.  ``margins`` measures, in fp64, how far every decision of a
row is from flipping:

  draw        the winner's p / q is at least 100 x every other slot's.  Rows flagged ``first_index`` are the exception: there the
              winner is the FIRST slot among the maximal ratios.  For those ``margins`` checks that every slot whose ratio is within
              100 x of the winner's has a ratio that is not larger (in fp64) and an index that is higher: division by one common
              denominator and by q = 1 is monotone in IEEE arithmetic, so whether or not two nearly equal ratios round to the same
              fp32 number, the first maximal slot is the same one.
  membership  top-k: every value is bit-equal to the k-th largest or at least 1e-3 relative away from it.  Rows that already are
              probabilities hold the same bits on both sides and reach the threshold through comparisons alone (no arithmetic comes
              before the radix select), so there the keys may differ by one bit: that is what the radix rows are for.
              top-p: every cs_r - p_r is exactly representable and compared exactly (``dyadic`` rows: every probability a multiple
              of 2^-24, total <= 1, so every partial sum is exact in any order), or at least 1e-4 away from top_p.
  range       no probability is subnormal (0 or >= 2^-126), and in logits mode every x / temp lies within 80 of the row maximum (or
              more than 200 below it, where expf is an exact 0 on both sides; no row here goes there).

``MUTANTS`` are four wrong implementations of the reference; the host test shows, on the CPU, which built rows tell each of them
from the reference — the argument that the device tests can fail.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

V = 1024
Q_SMALL = 1e-4
F32_MIN_NORMAL = 2.0 ** -126
TIE_EPS = 2.0 ** -22


class Params(NamedTuple):
    use_sampling: bool = True
    temp: float = 1.0
    top_k: int = 0
    top_p: float = 0.0
    cfg_scale: float = 1.0
    input_is_probs: bool = False


@dataclass
class Case:
    group: str
    name: str
    params: Params
    x: torch.Tensor                      # (V) fp32: logits (the conditional row under CFG) or probabilities
    noise: torch.Tensor                  # (V) fp32: 1 everywhere, Q_SMALL on the targeted token / rank
    expect: int                          # the token the structure of the row implies
    u: Optional[torch.Tensor] = None     # (V) fp32: the null-condition row (cfg_scale > 1)
    first_index: bool = False            # the draw (or the greedy argmax) is decided by "first index among equals"
    dyadic: bool = False                 # top-p: every partial sum is exact

    @property
    def id(self) -> str:
        return f"{self.group}/{self.name}"


def f32(v: float) -> float:
    return float(np.float32(v))


def mixed(case: Case) -> torch.Tensor:
    """the row the selection works on: the kernel's expression lu + (lc - lu) * s (exact on the integer rows built here)"""
    if case.u is None:
        return case.x
    return case.u + (case.x - case.u) * torch.tensor(case.params.cfg_scale, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------------------- the reference
MUTANTS = ("exact_k", "higher_id_first", "cut_ge", "last_wave")


def _argmax_first(v: torch.Tensor, mutant: Optional[str]) -> torch.Tensor:
    """first-index argmax over the last dim, keepdim (torch.argmax).  Mutant last_wave: among the four 256-token waves that hold
    the maximum, the LAST one's first maximal index wins."""
    if mutant != "last_wave":
        return torch.argmax(v, dim=-1, keepdim=True)
    w = v.reshape(*v.shape[:-1], 4, V // 4)
    wi = torch.argmax(w, dim=-1)
    wv = torch.gather(w, -1, wi[..., None])[..., 0]
    last = 3 - torch.argmax(torch.flip(wv, [-1]), dim=-1, keepdim=True)
    return torch.gather(wi, -1, last) + last * (V // 4)


def next_token(rows: torch.Tensor, *, use_sampling: bool, temp: float, top_k: int, top_p: float, noise: Optional[torch.Tensor],
               input_is_probs: bool = False, dtype: torch.dtype = torch.float32, mutant: Optional[str] = None) -> torch.Tensor:
    """rows (..., V), already CFG-mixed (or probabilities) -> tokens (..., 1) int64; noise of the same shape, indexed by token, under
    top-p by rank.  temp and top_p are held in fp32, as the kernel holds them, whatever ``dtype`` the arithmetic runs in."""
    assert mutant is None or mutant in MUTANTS
    x = rows.to(dtype)
    temp, top_p = f32(temp), f32(top_p)
    if not input_is_probs and not (use_sampling and temp > 0.0):
        return _argmax_first(x, mutant)
    probs = x if input_is_probs else torch.softmax(x / temp, dim=-1)
    q = noise.reshape(probs.shape).to(dtype)
    if top_p > 0.0:
        if mutant == "higher_id_first":      # an order among equals that is not "lower id first"
            ps, order = torch.sort(torch.flip(probs, [-1]), dim=-1, descending=True, stable=True)
            order = V - 1 - order
        else:
            ps, order = torch.sort(probs, dim=-1, descending=True, stable=True)
        cs = torch.cumsum(ps, dim=-1)
        drop = (cs - ps >= top_p) if mutant == "cut_ge" else (cs - ps > top_p)
        ps = ps * (~drop).to(dtype)
        ps = ps / ps.sum(dim=-1, keepdim=True)
        return torch.gather(order, -1, _argmax_first(ps / q, mutant))
    if top_k > 0:
        kk = min(top_k, V)
        if mutant == "exact_k":              # keeps exactly k tokens: the first k of a stable descending sort
            order = torch.sort(probs, dim=-1, descending=True, stable=True).indices[..., :kk]
            keep = torch.zeros_like(probs).scatter_(-1, order, 1.0)
        else:
            kth = torch.topk(probs, kk, dim=-1).values[..., [-1]]
            keep = (probs >= kth).to(dtype)
        probs = probs * keep
        probs = probs / probs.sum(dim=-1, keepdim=True)
    return _argmax_first(probs / q, mutant)


def reference_token(case: Case, dtype: torch.dtype = torch.float32, mutant: Optional[str] = None) -> int:
    p = case.params
    row = mixed(case)
    return int(next_token(row[None], use_sampling=p.use_sampling, temp=p.temp, top_k=p.top_k, top_p=p.top_p, noise=case.noise[None],
                          input_is_probs=p.input_is_probs, dtype=dtype, mutant=mutant)[0, 0])


def has_top_p_tie(case: Case) -> bool:
    """two equal probabilities under top-p: the oracle's unstable sort leaves their ranks undefined"""
    p = case.params
    if not (p.use_sampling and p.temp > 0.0 and p.top_p > 0.0):
        return False
    probs = case.x if p.input_is_probs else torch.softmax(mixed(case) / f32(p.temp), -1)
    return int(torch.unique(probs).numel()) < V


# --------------------------------------------------------------------------------------------------------------- fp64 margins
@dataclass
class Margins:
    winner: int                  # the token the fp64 arithmetic selects
    draw: float                  # winner's ratio / the best other ratio (inf: nothing else is kept); first_index rows: see first_ok
    first_ok: bool               # first_index rows: every slot within 100 x of the winner is not larger and has a higher index
    member: float                # top-k, logits mode: smallest relative distance to the threshold of a value not bit-equal to it
    cut: float                   # top-p, not dyadic: smallest |cs_r - p_r - top_p|
    dyadic_ok: bool              # top-p, dyadic: multiples of 2^-24 with total <= 1, and the fp32 running sum equals the fp64 one
    normal: bool                 # no subnormal probability, in fp64 and in the fp32 reference
    range_ok: bool               # logits mode: x / temp within 80 of the maximum, or more than 200 below it


def margins(case: Case) -> Margins:
    p = case.params
    x = mixed(case).double()
    inf = float("inf")
    if not (p.use_sampling and p.temp > 0.0):                # greedy: exact ties at the maximum, everything else at least 1 below
        mx = x.max()
        at_max = torch.nonzero(x == mx)[:, 0]
        rest = x[x != mx]
        gap = float(mx - rest.max()) if rest.numel() else inf
        return Margins(int(at_max[0]), gap, True, inf, inf, True, True, True)
    temp, top_p = f32(p.temp), f32(p.top_p)
    q = case.noise.double()
    if p.input_is_probs:
        probs, range_ok = x, True
        probs32 = case.x
    else:
        z = x / temp
        d = z.max() - z
        range_ok = bool(((d <= 80.0) | (d > 200.0)).all())
        probs = torch.softmax(z, -1)
        probs32 = torch.softmax(mixed(case) / temp, -1)
    normal = all(bool(((t == 0) | (t >= F32_MIN_NORMAL)).all()) for t in (probs, probs32))
    member, cut, dyadic_ok = inf, inf, True
    order = torch.arange(V)
    if top_p > 0.0:
        ps, order = torch.sort(probs, descending=True, stable=True)
        cs = torch.cumsum(ps, -1)
        keep = ~(cs - ps > top_p)
        if case.dyadic:
            cs32 = torch.cumsum(ps.float(), -1)
            dyadic_ok = bool((ps * 2.0 ** 24 == torch.round(ps * 2.0 ** 24)).all()) and float(cs[-1]) <= 1.0 and \
                bool((cs32.double() == cs).all()) and bool((probs32.double() == probs).all())
        else:
            cut = float(((cs - ps) - top_p).abs().min())
        kept = ps * keep
        ratios = (kept / kept.sum()) / q
    elif p.top_k > 0:
        kk = min(p.top_k, V)
        top = torch.topk(probs, kk)
        thr, at = top.values[-1], int(top.indices[-1])
        same = mixed(case) == mixed(case)[at]                # bit-equal inputs (no row here holds both zeros under top-k)
        keep = probs >= thr
        assert bool((keep == (x >= x[at])).all())
        if not p.input_is_probs and bool((~same).any()):
            member = float((probs[~same] / thr - 1.0).abs().min())
        kept = probs * keep
        ratios = (kept / kept.sum()) / q
    else:
        ratios = probs / q
    w = int(torch.argmax(ratios))
    others = ratios.clone()
    others[w] = -1.0
    best = float(others.max())
    draw = float(ratios[w]) / best if best > 0 else inf
    near = torch.nonzero(others >= ratios[w] / 100.0)[:, 0]
    first_ok = bool((near > w).all()) and bool((ratios[near] <= ratios[w]).all())
    return Margins(int(order[w]), draw, first_ok, member, cut, dyadic_ok, normal, range_ok)


# ------------------------------------------------------------------------------------------------------------------- row builders
def _noise(slot: int) -> torch.Tensor:
    q = torch.ones(V)
    q[slot] = Q_SMALL
    return q


def _perm(seed: int) -> List[int]:
    return torch.randperm(V, generator=torch.Generator().manual_seed(seed)).tolist()


TOP_KS = (1, 2, 128, 250, 1000, 1023, 1024, 2000)


def topk_threshold_rows() -> List[Case]:
    """1. The top-k threshold shared by several tokens.  min(k, V) - 4 distinct larger logits, then 9 tokens at the shared value 0 at
    scattered ids (ranks k-3 .. k+5; fewer where the vocabulary ends: 5 for k = 1023, 4 for k >= 1024), one token at -0.5, a flat
    tail at -2.  Three targets per (k, temperature):
      hi     the highest-id tied token wins (a keep-exactly-k selection drops it or its lowest-id twin);
      lo     the lowest-id tied token wins;
      below  the token at -0.5 must NOT win: the largest logit does (k <= 2: no larger logit, the first of the tied maxima — a draw
             tie).  k >= 1023 leaves no rank below the group; the third target there is the tied token of middle id, which is kept.
    The larger logits of the hi / lo rows rise to 4 temp above the group (winner's margin e^-4 x 1e4 = 183).  The below rows keep
    them within 0.75 temp and put the largest 4.7 temp above the second (it wins by e^4.7 = 110), 5.45 temp + 0.5 above the targeted
    token: a selection that kept that token would hand it the draw by 1e4 / e^6.2 = 21 x."""
    out = []
    for temp in (1.0, 0.7):
        for k in TOP_KS:
            kk = min(k, V)
            n_big = max(kk - 4, 0)
            n_tie = min(9, V - n_big)
            ids = _perm(100 + k)
            big, tie = ids[:n_big], sorted(ids[n_big:n_big + n_tie])
            below = ids[n_big + n_tie] if n_big + n_tie < V else None

            def row(peak: bool) -> torch.Tensor:
                x = torch.full((V,), -2.0)
                x[tie] = 0.0
                if below is not None:
                    x[below] = -0.5
                if n_big:
                    i = torch.arange(1, n_big + 1, dtype=torch.float64)
                    v = temp * (0.25 + 0.5 * i / n_big) if peak else temp * (0.5 + 3.5 * i / n_big)
                    if peak:
                        v[-1] = temp * (0.75 + 4.7)
                    x[big] = v.float()
                return x

            prm = Params(True, temp, k, 0.0)
            name = f"k{k}_t{temp}"
            out.append(Case("topk", name + "_hi", prm, row(False), _noise(tie[-1]), tie[-1]))
            out.append(Case("topk", name + "_lo", prm, row(False), _noise(tie[0]), tie[0]))
            if below is not None:
                out.append(Case("topk", name + "_below", prm, row(True), _noise(below), big[-1] if n_big else tie[0], first_index=n_big == 0))
            else:
                mid = tie[len(tie) // 2]
                out.append(Case("topk", name + "_mid", prm, row(False), _noise(mid), mid))
    return out


RADIX_BASE = 0x3C000000      # 2^-7


def _radix_keys() -> Dict[str, np.ndarray]:
    """the 1024 keys of every radix row, sorted descending; second value: the ranks k to test (1-based)"""
    r = np.arange(V)
    rng = np.random.default_rng(5)
    rand = np.sort(RADIX_BASE + rng.integers(0, 2 ** 25, V, dtype=np.int64))[::-1].copy()
    rand[300:305] = rand[300]                                  # one tie group inside the random keys
    return {
        "byte0": RADIX_BASE | (255 - r // 4),                  # 256 values x 4 copies, only the lowest byte differs
        "byte1": RADIX_BASE | ((255 - r // 4) << 8),
        "byte2": RADIX_BASE | ((255 - r // 4) << 16),
        "byte3": (0x3F - r // 256) << 24,                      # 2^-1, 2^-3, 2^-5, 2^-7: 256 copies each
        "random": rand,
        "equal": np.full(V, RADIX_BASE),
    }


def radix_rows() -> List[Case]:
    """2. Radix-select byte structure, rows that already are probabilities (the same bits on both sides, the threshold is pure
    comparison).  Keys that differ in one byte only, in random bits (25 of them: two bins in the first pass), in nothing.  k puts the
    k-th rank on the first element of a histogram bin of the pass that decides, on the last one, inside a tie group (rows whose keys
    differ in one byte: a bin of that pass IS a tie group of 4, or of 256 for byte 3).  Two targets per (row, k): the highest-id
    token at the threshold value wins; the largest dropped token (the next rank) does not — token 0, which holds the row's maximum in
    every row, wins then (first index among nearly equal ratios).  Rows without a dropped token (everything equal, k = V) target
    token 517 instead, which is kept."""
    ks = {"byte0": (149, 152, 150), "byte1": (149, 152, 150), "byte2": (149, 152, 150), "byte3": (257, 512, 300),
          "equal": (1, V, 500)}
    out = []
    for name, keys in _radix_keys().items():
        keys = np.asarray(keys, dtype=np.int64)
        assert bool((np.diff(keys) <= 0).all())
        scatter = [0] + [i for i in _perm(7) if i != 0]           # rank -> token id; the maximum sits on token 0
        row = torch.zeros(V)
        row[scatter] = torch.from_numpy(keys.astype(np.int32).view(np.float32).copy())
        if name == "random":
            n1 = int((keys >> 24 == keys[0] >> 24).sum())      # first bin of the first pass
            row_ks = (1, n1, n1 + 1, 302)
        else:
            row_ks = ks[name]
        for k in row_ks:
            thr = keys[k - 1]
            at_thr = [scatter[j] for j in np.nonzero(keys == thr)[0]]
            n_kept = int((keys >= thr).sum())
            prm = Params(True, 1.0, k, 0.0, 1.0, True)
            hi = max(at_thr)
            out.append(Case("radix", f"{name}_k{k}_kept", prm, row, _noise(hi), hi))
            if n_kept < V:
                out.append(Case("radix", f"{name}_k{k}_dropped", prm, row, _noise(scatter[n_kept]), 0, first_index=True))
            else:
                out.append(Case("radix", f"{name}_k{k}_kept517", prm, row, _noise(517), 517))
    return out


DYADIC_IDS = ([700, 10], [3, 517, 64, 900])                        # 1/4 at the first two, 1/8 at the other four
DYADIC_ORDER = [10, 700, 3, 64, 517, 900]                          # "lower id first"
EIGHTHS_IDS = [801, 40, 333, 7, 1000, 512, 96, 255]
LN3 = math.log(3.0)


def _dyadic_row() -> torch.Tensor:
    x = torch.zeros(V)
    x[DYADIC_IDS[0]] = 0.25
    x[DYADIC_IDS[1]] = 0.125
    return x


def _two_valued(bit: int, pol: int):
    ids = torch.arange(V)
    hi = ((ids >> bit) & 1) == pol
    order = torch.cat([ids[hi], ids[~hi]]).tolist()
    return torch.where(hi, torch.tensor(LN3, dtype=torch.float32), torch.tensor(0.0)), order


def topp_order_rows() -> List[Case]:
    """3. Top-p order among ties (the bitonic network); the noise is indexed by RANK, so the tiny noise at rank r must return the token
    the stable sort puts there.
      equal     1024 equal logits: p = 2^-10 exactly, sorted order = identity.  top_p = 0.999: rank 1023 (cs - p = 1023/1024 > fp32
                0.999) is dropped and token 0 wins instead, first among 1023 equal ratios.
      bit<b>_<v> 512 tokens at logit ln 3, 512 at 0, the larger value where bit b of the id equals v: the first comparison that
                decides falls into a register (bits 0), lane (2, 7), LDS-256 (8) or LDS-512 (9) stage.  top_p = 0.95 keeps ranks
                0 .. 921; rank 1000 is dropped and rank 0's token wins (first among the 512 equal ratios).
      asc, desc distinct logits 0.01 apart, ascending and descending in the id (top_p = 0.9 keeps about 230 ranks).
      dyadic    probabilities {1/4, 1/4, 1/8 x 4} at ids out of order, 0 elsewhere (top_p = 0.9 keeps the six)."""
    out = []
    prm = Params(True, 1.0, 0, 0.999)
    for r in (0, 3, 4, 255, 256, 511, 512, 1022):
        out.append(Case("topp_order", f"equal_r{r}", prm, torch.zeros(V), _noise(r), r, dyadic=True))
    out.append(Case("topp_order", "equal_r1023_dropped", prm, torch.zeros(V), _noise(1023), 0, first_index=True, dyadic=True))
    prm = Params(True, 1.0, 0, 0.95)
    for bit in (0, 2, 7, 8, 9):
        for pol in (1, 0):
            x, order = _two_valued(bit, pol)
            for r in (0, 1, 255, 256, 511, 512, 700):
                out.append(Case("topp_order", f"bit{bit}_{pol}_r{r}", prm, x, _noise(r), order[r]))
            out.append(Case("topp_order", f"bit{bit}_{pol}_r1000_dropped", prm, x, _noise(1000), order[0], first_index=True))
    prm = Params(True, 1.0, 0, 0.9)
    step = torch.arange(V, dtype=torch.float64) * 0.01
    for r in (0, 1, 2, 3, 4, 63, 64, 200):
        out.append(Case("topp_order", f"asc_r{r}", prm, step.float(), _noise(r), V - 1 - r))
        out.append(Case("topp_order", f"desc_r{r}", prm, (-step).float(), _noise(r), r))
    prm = Params(True, 1.0, 0, 0.9, 1.0, True)
    for r, tok in enumerate(DYADIC_ORDER):
        out.append(Case("topp_order", f"dyadic_r{r}", prm, _dyadic_row(), _noise(r), tok, dyadic=True))
    return out


def topp_cut_rows() -> List[Case]:
    """4. The top-p cut on its boundary: dyadic probabilities, so cs - p is exact in any order, and a strict cut (dropped when
    cs - p > top_p).  {1/4, 1/4, 1/8 x 4}: cs - p = 0, 1/4, 1/2, 5/8, 3/4, 7/8; top_p = 0.5, 0.625, 0.75 keep 3, 4, 5 ranks — the rank
    whose cs - p EQUALS top_p is kept; 0.625 and 0.75 cut inside the tie group of the four 1/8.  eighths: eight tokens at 1/8,
    top_p = 0.375 keeps ranks 0 .. 3 of one tie group.  The last kept rank wins; the first dropped rank does not — rank 0's token does
    (first among the equal largest ratios).  full: top_p = 1.0 on 1024 equal logits drops nothing and rank 1023 wins."""
    out = []
    for top_p, n_keep in ((0.5, 3), (0.625, 4), (0.75, 5)):
        prm = Params(True, 1.0, 0, top_p, 1.0, True)
        out.append(Case("topp_cut", f"dyadic_p{top_p}_last_kept", prm, _dyadic_row(), _noise(n_keep - 1), DYADIC_ORDER[n_keep - 1], dyadic=True))
        out.append(Case("topp_cut", f"dyadic_p{top_p}_first_dropped", prm, _dyadic_row(), _noise(n_keep), DYADIC_ORDER[0], first_index=True,
                        dyadic=True))
    x = torch.zeros(V)
    x[EIGHTHS_IDS] = 0.125
    order = sorted(EIGHTHS_IDS)
    prm = Params(True, 1.0, 0, 0.375, 1.0, True)
    out.append(Case("topp_cut", "eighths_last_kept", prm, x, _noise(3), order[3], dyadic=True))
    out.append(Case("topp_cut", "eighths_first_dropped", prm, x, _noise(4), order[0], first_index=True, dyadic=True))
    prm = Params(True, 1.0, 0, 1.0)
    for r in (1023, 0):
        out.append(Case("topp_cut", f"full_r{r}", prm, torch.zeros(V), _noise(r), r, dyadic=True))
    return out


GREEDY_TIES = (("thread_cols_0_3", (40, 43)), ("thread_cols_1_2", (41, 42)), ("lanes_wave0", (41, 130)), ("lanes_wave2", (600, 701)),
               ("waves_0_3", (7, 900)), ("waves_255_256", (255, 256)), ("thread_300_301", (300, 301)), ("waves_511_512", (511, 512)),
               ("waves_767_768", (767, 768)), ("three_waves", (100, 501, 1002)))
ZERO_IDS = (5, 601)


def greedy_rows(cfg_scale: float = 1.0) -> List[Case]:
    """5. Greedy first-index ties: the maximum (3) shared by two columns of one thread, two lanes of one wave, tokens of different waves
    (also across each 256-token boundary), all 1024 tokens; +0.0 and -0.0 as the tied maxima of a negative row (both orders).  The rest
    of a row is the integers -1 - (i mod 7).  cfg_scale = 6: the same mixed rows m, given as c = m - 5 d and u = m - 6 d with the
    integers d = (i mod 5) - 2, so u + (c - u) * 6 = m exactly and the tie exists only after the mix (the signed zeros become one
    case: the mix gives +0 twice)."""
    i = torch.arange(V)
    base = -1.0 - (i % 7).float()
    rows = []
    for name, ids in GREEDY_TIES:
        m = base.clone()
        m[list(ids)] = 3.0
        rows.append((name, m, ids[0]))
    rows.append(("all_equal", torch.full((V,), 3.0), 0))
    if cfg_scale > 1.0:
        m = base.clone()
        m[list(ZERO_IDS)] = 0.0
        rows.append(("zeros", m, ZERO_IDS[0]))
    else:
        for name, (a, b) in (("neg_zero_first", (-0.0, 0.0)), ("pos_zero_first", (0.0, -0.0))):
            m = base.clone()
            m[ZERO_IDS[0]], m[ZERO_IDS[1]] = a, b
            rows.append((name, m, ZERO_IDS[0]))
    prm = Params(False, 1.0, 0, 0.0, cfg_scale)
    out = []
    d = ((i % 5) - 2).float()
    for name, m, tok in rows:
        if cfg_scale > 1.0:
            out.append(Case("greedy_cfg", name, prm, m - 5.0 * d, torch.ones(V), tok, u=m - 6.0 * d, first_index=True))
        else:
            out.append(Case("greedy", name, prm, m, torch.ones(V), tok, first_index=True))
    return out


def near_tie_rows() -> List[List[Case]]:
    """6. Launches whose every row is an exact tie of the decision itself, for the near-tie detector (positive direction only): the
    greedy rows without and with the mix, and the k = 1 rows of group 1 whose draw is a tie (the below target), one per temperature."""
    k1 = [c for c in topk_threshold_rows() if c.params.top_k == 1 and c.first_index]
    return [greedy_rows(1.0), greedy_rows(6.0)] + [[c] for c in k1]


def all_cases() -> List[Case]:
    return topk_threshold_rows() + radix_rows() + topp_order_rows() + topp_cut_rows() + greedy_rows(1.0) + greedy_rows(6.0)


def launches(cases: List[Case]) -> List[List[Case]]:
    """the rows of one parameter set, in order of first appearance: one launch each"""
    by: Dict[Params, List[Case]] = {}
    for c in cases:
        by.setdefault(c.params, []).append(c)
    return list(by.values())


def pack(cases: List[Case], K: int = 4):
    """the (B, K) grid of one launch, padded with copies of its first row -> (rows (B or 2B, K, V), noise (B * K, V), expected (B, K))"""
    K = min(K, len(cases))
    B = -(-len(cases) // K)
    full = list(cases) + [cases[0]] * (B * K - len(cases))
    rows = torch.stack([c.x for c in full]).view(B, K, V)
    if full[0].u is not None:
        rows = torch.cat([rows, torch.stack([c.u for c in full]).view(B, K, V)])
    noise = torch.stack([c.noise for c in full])
    expect = torch.tensor([c.expect for c in full], dtype=torch.int32).view(B, K)
    return rows.contiguous(), noise.contiguous(), expect


# ------------------------------------------------------------------------------------------------------------ the golden tie rows
GOLDEN_TOP_P = (("topp90", 250, 0.9), ("topp30", 0, 0.3))
GOLDEN_TIE_ROWS = ((0, 0), (1, 3))
