"""Host side of the streaming loudness (vaura_amd/loudness.py) and its float64 oracle (tests/loudness_reference.py); no GPU.

  1. the chunk tables: h1, h2 and M reproduce L steps of the homogeneous system from a direct float64 recursion to 1e-12 relative,
     and the whole chunked form (zero-state chunks, the serial chain, the correction), restated here in numpy on the plan's tables,
     is the plain recursion;
  2. push_records: received counts, boundaries, blocks and windows for the partitions the device test pushes;
  3. the oracle against a literal sample-by-sample restatement, and its I at the last boundary against oracle/post_oracle.py;
  4. the device test's inputs keep every block 0.05 LU away from both gates; 5. what LoudnessTarget refuses."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_reference as RL  # noqa: E402
from oracle import post_oracle  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import loudness as LD  # noqa: E402

RATES = [44100, 48000, 16000]


# ------------------------------------------------------------------------------------- 1. tables
@pytest.mark.parametrize("rate", RATES + [8000, 22050, 32000])
@pytest.mark.parametrize("lanes", [256, 64])
def test_tables_reproduce_the_homogeneous_system(rate, lanes):
    # lanes: the kernel's 256 (L <= 19) and a quarter of it (L <= 75).  The high-pass has a double pole at r ~ 0.995: over n steps any
    # float64 recursion of it, the direct one this test compares with included, gathers about n^2 / 2 roundings (h1 ~ (n + 1) r^n and
    # h2 ~ -n r^n cancel), 3e-13 at n = 75; 1e-12 cannot be asked of chunks of several hundred samples from either side.
    pl = LD.LoudnessPlan(rate, lanes)
    assert pl.step == RL.step_of(rate) and pl.gate == 4 * pl.step
    assert pl.L == -(-pl.step // lanes) and (pl.C - 1) * pl.L < pl.step <= pl.C * pl.L and pl.C <= lanes and 1 <= pl.last <= pl.L
    t = pl.table()
    assert t.dtype == np.float64 and t.shape == (10 + 2 * (2 * pl.L + 8),)
    ref = RL.coefficients(rate)
    rng = np.random.default_rng(1)
    for s, (b, a) in enumerate(ref):
        co = t[5 * s:5 * s + 5]
        assert np.allclose(co, [b[0], b[1], b[2], a[1], a[2]], rtol=1e-15, atol=0)
        base = 10 + s * (2 * pl.L + 8)
        h1, h2 = t[base:base + pl.L], t[base + pl.L:base + 2 * pl.L]
        Mf, Ml = t[base + 2 * pl.L:base + 2 * pl.L + 4].reshape(2, 2), t[base + 2 * pl.L + 4:base + 2 * pl.L + 8].reshape(2, 2)
        for _ in range(4):
            s1, s2 = rng.standard_normal(2)
            y, p1, p2 = [], s1, s2
            for _i in range(pl.L):
                v = -a[1] * p1 - a[2] * p2
                y.append(v)
                p2, p1 = p1, v
            y = np.array(y)
            scale = np.abs(y).max()
            assert np.abs(h1 * s1 + h2 * s2 - y).max() <= 1e-12 * scale
            for M, n in ((Mf, pl.L), (Ml, pl.last)):
                want = np.array([y[n - 1], y[n - 2] if n >= 2 else s1])
                assert np.abs(M @ np.array([s1, s2]) - want).max() <= 1e-12 * max(scale, abs(s1))


def chunked(x, pl, stage, state):
    """one biquad over whole steps as the kernel runs it, on the plan's table, float64: (unclamped outputs, state behind them)"""
    t = pl.table()
    b0, b1, b2, a1, a2 = t[5 * stage:5 * stage + 5]
    base = 10 + stage * (2 * pl.L + 8)
    h1, h2 = t[base:base + pl.L], t[base + pl.L:base + 2 * pl.L]
    Mf, Ml = t[base + 2 * pl.L:base + 2 * pl.L + 4].reshape(2, 2), t[base + 2 * pl.L + 4:base + 2 * pl.L + 8].reshape(2, 2)
    xp = np.concatenate([[0.0, 0.0], x])
    out = np.zeros(len(x))
    s = np.array(state, dtype=np.float64)
    for j in range(len(x) // pl.step):
        ends, zs = [], []
        for c in range(pl.C):
            i0 = j * pl.step + c * pl.L
            n = min(pl.L, (j + 1) * pl.step - i0)
            y1 = y2 = 0.0
            z = np.zeros(n)
            for k in range(n):
                v = ((b0 * xp[i0 + k + 2] + b1 * xp[i0 + k + 1]) + b2 * xp[i0 + k]) - a1 * y1 - a2 * y2
                z[k] = v
                y2, y1 = y1, v
            zs.append(z)
            ends.append(np.array([y1, y2]))
        for c in range(pl.C):
            i0 = j * pl.step + c * pl.L
            n = len(zs[c])
            out[i0:i0 + n] = zs[c] + (h1[:n] * s[0] + h2[:n] * s[1])
            s = ends[c] + (Ml if c == pl.C - 1 else Mf) @ s
    return out, s


@pytest.mark.parametrize("rate,lanes", [(16000, 256), (8000, 256), (16000, 100)])
def test_the_chunked_form_is_the_recursion(rate, lanes):
    from scipy.signal import lfilter
    pl = LD.LoudnessPlan(rate, lanes)
    x = np.random.default_rng(2).standard_normal(3 * pl.step) * 0.3 + 0.1
    for stage, (b, a) in enumerate(RL.coefficients(rate)):
        got, s = chunked(x, pl, stage, (0.0, 0.0))
        want = lfilter(b, a, x)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(s - want[[-1, -2]]).max() <= 1e-12 * np.abs(want).max()


# ------------------------------------------------------------------------------------- 2. bookkeeping
def partitions(lengths, step):
    plans = {"one push": [list(lengths)]}
    for size in (8192, 1, step - 1, step, step + 1, 3 * step + 5):
        left, steps = list(lengths), []
        while any(left) and len(steps) < 40:
            take = [min(n, size) for n in left]
            steps.append(take)
            left = [n - s for n, s in zip(left, take)]
        if any(left):
            steps.append(left)                                           # the small sizes: a few pushes of that size, then the rest
        plans[f"{size} samples"] = steps
    return plans


@pytest.mark.parametrize("rate", RATES)
def test_push_records_bookkeeping(rate):
    pl = LD.LoudnessPlan(rate)
    step = pl.step
    lengths = [22 * step + 1234, 5 * step + 7, 3 * step]
    for name, steps in partitions(lengths, step).items():
        received = [0, 0, 0]
        total = {"boundaries": [0] * 3, "blocks": [0] * 3, "windows": [0] * 3}
        for take in steps:
            rec = LD.push_records(pl, received, take)
            assert rec["records"] == [[r, n] for r, n in zip(received, take)]
            assert rec["received"] == [r + n for r, n in zip(received, take)]
            assert rec["stride"] == max(max(rec["boundaries"]), 1)
            for b in range(3):
                assert rec["boundaries"][b] == (received[b] + take[b]) // step - received[b] // step
            for k in total:
                total[k] = [a + b for a, b in zip(total[k], rec[k])]
            received = rec["received"]
        assert received == lengths, name
        assert total["boundaries"] == [22, 5, 3] and total["blocks"] == [19, 2, 0] and total["windows"] == [0, 0, 0], name
    assert pl.windows(30 * step) == 1 and pl.windows(30 * step - 1) == 0 and pl.blocks(4 * step) == 1 and pl.blocks(4 * step - 1) == 0
    rec = LD.push_records(pl, [29 * step + 5], [2 * step])
    assert rec["boundaries"] == [2] and rec["blocks"] == [2] and rec["windows"] == [2]


# ------------------------------------------------------------------------------------- 3. the oracle
def test_oracle_against_a_literal_restatement():
    rate = 16000
    x = RL.stepped_noise(rate, [0.2, 1.5, 0.01], 77, 0.3, seed=4)
    # scipy's lfilter runs the transposed form II, the literal loop form I: two float64 roundings of one recursion whose double pole at
    # r = 1 - 0.015 (38 Hz at 16 kHz) amplifies a rounding by up to 1 / (1 - r)^2 = 4.5e3: 4.5e3 * 2^-53 * 2 = 1e-12 on outputs <= 1
    assert np.abs(RL.k_weight(x, rate) - RL.k_weight_literal(x, rate)).max() <= 1e-12
    step = RL.step_of(rate)
    x = RL.stepped_noise(rate, [0.2] * 5 + [0.0] * 2, 9, 0.2, seed=5)
    o = RL.oracle(x, rate, slew=5.0, limiter="tanh", initial_gain_db=3.0)
    w = RL.k_weight_literal(x, rate)
    S = [float(np.sum(w[j * step:(j + 1) * step] ** 2)) for j in range(7)]
    assert np.allclose(o["S"], S, rtol=1e-12)
    assert len(o["I"]) == 8 and all(np.isnan(o["I"][:4])) and not np.isnan(o["I"][4:]).any()
    d_prev, a_prev = 3.0, 10 ** (3.0 / 20)
    for i, xi in enumerate(x.astype(np.float64)):
        m, k = divmod(i, step)
        if k == 0:
            if m > 0:
                d_prev, a_prev = d_m, a_m
            tgt = d_prev if np.isnan(o["I"][m]) else min(max(-12.0 - o["I"][m], -20.0), 20.0)
            d_m = d_prev + min(max(tgt - d_prev, -0.5), 0.5)
            a_m = 10 ** (d_m / 20)
        g = a_prev + (a_m - a_prev) * (k + 1) / step
        assert abs(o["out"][i] - min(max(np.tanh(xi * g), -1.0), 1.0)) <= 1e-15, i
    assert o["momentary"].shape == (4,) and o["short_term"].shape == (0,)


@pytest.mark.parametrize("rate", RATES)
def test_oracle_integrated_against_post_oracle(rate):
    step = RL.step_of(rate)
    x = RL.stepped_noise(rate, RL.AMPS, 0, 0.0)                          # whole steps: both take the same blocks
    want = post_oracle.loudness_lkfs(torch.from_numpy(x)[None], rate)
    got = RL.meter(x, rate)["I"][-1]
    assert abs(got - want) <= 1e-9, (got, want)
    assert len(x) == 22 * step


# ------------------------------------------------------------------------------------- 4. the condition on the device test's inputs
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("history", [8, 4096])
def test_no_block_of_the_test_inputs_lies_near_a_gate(rate, history):
    step = RL.step_of(rate)
    x = RL.stepped_noise(rate, RL.AMPS, 1234, 0.3)
    for n in (22 * step + 1234, 5 * step + 7, 3 * step):
        m = RL.meter(x[:n], rate, history)
        assert m["margin"] >= 0.05, (n, m["margin"])
    full = RL.meter(x, rate, history)["I"]
    assert np.isnan(full[:4]).all() and not np.isnan(full[4:]).any()     # (the silent steps still hold the filters' decaying tail)
    if history == 8:                                                     # the window has left the first steps behind: the ring wrapped
        assert abs(full[22] - RL.meter(x, rate, 4096)["I"][22]) > 0.5


# ------------------------------------------------------------------------------------- 5. refusals on the host
def test_refusals_of_plan_and_target():
    from vaura_amd import post
    for rate in (11025, 7999, 48001, 44100.0, True):
        with pytest.raises(L.VauraHipError):
            LD.LoudnessPlan(rate)
        with pytest.raises(L.VauraHipError):
            post.LoudnessTarget(sample_rate=rate)
    for h in (4, 7, 4097, 8.0):
        with pytest.raises(L.VauraHipError):
            post.LoudnessTarget(history_steps=h)
    for kw in (dict(limiter="soft"), dict(max_gain_db=-1.0), dict(target_lkfs=float("nan")), dict(slew_db_per_s=0.0),
               dict(initial_gain_db=float("inf")), dict(target_lkfs=1.0)):
        with pytest.raises(L.VauraHipError):
            post.LoudnessTarget(**kw)
    t = post.LoudnessTarget()
    assert (t.target_lkfs, t.max_gain_db, t.slew_db_per_s, t.initial_gain_db, t.limiter, t.sample_rate, t.history_steps) == \
        (-12.0, 20.0, None, 0.0, "clip", 44100, 4096)
    assert post.LoudnessTarget(history_steps=8, sample_rate=8000).plan.step == 800
    assert "loudness.hip" in __import__("vaura_amd.csrc.build", fromlist=["SOURCES"]).SOURCES
    for name in ("vaura_audio_loudness_push", "vaura_audio_loudness_state_elems", "vaura_audio_loudness_table_elems",
                 "vaura_audio_loudness_lds_bytes"):
        assert name in L.SIGNATURES
    with pytest.raises(L.VauraHipError):
        post.LoudnessStream(t, 2, "cpu")
    with pytest.raises(L.VauraHipError):
        post.LoudnessStream(t, 0, "cuda")
