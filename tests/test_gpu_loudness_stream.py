"""Streaming loudness on the GPU: vaura_audio_loudness_push (csrc/loudness.hip) through post.measure_loudness /
normalize_loudness_causal / LoudnessStream / stream_loudness.

  1. pushes concatenated are the one-pass result, torch.equal, over partitions (8192-sample blocks; one push; pushes of 1, 0, step - 1,
     step, step + 1 and 3 step + 5 samples in turn; other counts per clip; a clip finished early), both limiters, with and without a
     slew that binds (0.3 dB per step), history_steps 8 and 4096;
  2. against the float64 oracle of tests/loudness_reference.py: momentary and short-term under the bar derived below, integrated within
     4 times the distance the parent's serial kernel (normalize_audio(strategy="loudness")) keeps from the same oracle on the same
     clips, measured here; the normalised samples under loudness_reference's sample bar;
  3. semantics: clips independent, poisoned input behind samples[b], guards around the output, a state full of 0xFF, clipped, the
     3-step clip untouched, the correction inside +-max_gain_db;  4. composition on the tiny model;  5. refusals before any launch.

Before anything is compared each test asserts the condition on its inputs: in the oracle no block lies within 0.05 LU of a gate, so
the fp32 and the float64 gating decisions cannot differ.

The bar of a momentary / short-term value l = -0.691 + 10 log10(e), u = 2^-24: the K-weighted samples are rounded to fp32 (their
squares: 2 u), S_j is rounded once (u), the window sum of n steps adds n - 1 roundings, the division one: (n + 3) u relative on e, i.e.
10 / ln 10 (n + 3) u on l;  log10f within 1 ulp = 2 u of |log10 e|, times 10;  the product and the sum: 2 u |l| each at most:
    bar(l) = 10 / ln 10 (n + 3) u + 20 u |log10 e| + 4 u (|l| + 0.691)
The bar of an integrated value I_m over N gated blocks (the gating decisions being the oracle's, by the condition above): every block's
energy carries the (4 + 3) u of a momentary one; their fp32 sum adds at most N - 1 roundings in whatever fixed order, the division by
the count one: (N + 7) u relative on the mean, then the same logarithm, product and sum:
    bar(I) = 10 / ln 10 (N + 7) u + 20 u |log10 mean| + 4 u (|I| + 0.691)
It is asserted at EVERY defined boundary of a 33-step clip, for history_steps 8 (the ring wraps, the window moves) and 4096.
With VAURA_PARITY_DIR set the figures go to loudness_stream_parity.txt."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_reference as RL  # noqa: E402
import test_gpu_per_clip_sampling as G  # noqa: E402  (the tiny plugin model)
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import loudness as LD  # noqa: E402
from vaura_amd import post, synth  # noqa: E402
from vaura_amd.post import (LoudnessStream, LoudnessTarget, PcmFormat, measure_loudness, normalize_audio,  # noqa: E402
                            normalize_loudness_causal, stream_loudness, stream_pcm)

DEV = "cuda:0"
RATES = [44100, 48000, 16000]
U = 2.0 ** -24
_lines = {}


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    out = os.environ.get("VAURA_PARITY_DIR")
    if _lines and out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "loudness_stream_parity.txt"), "w") as f:
            f.write("streaming loudness against float64 (tests/test_gpu_loudness_stream.py)\n")
            for k in sorted(_lines):
                f.write(f"{k}: {_lines[k]}\n")


def lengths_for(rate):
    step = RL.step_of(rate)
    return [22 * step + 1234, 5 * step + 7, 3 * step]


_clips = {}


def clips(rate):
    """((3, 1, N) fp32 on the host: the stepped noise, every clip a prefix of it; lengths), computed once and left unchanged"""
    if rate not in _clips:
        x = torch.from_numpy(RL.stepped_noise(rate, RL.AMPS, 1234, 0.3))
        _clips[rate] = x[None, None].repeat(3, 1, 1).contiguous()
    return _clips[rate], lengths_for(rate)


_meters = {}


def oracle_meter(rate, history):
    """per clip the oracle's meter, once; asserts the gate condition on the inputs"""
    if (rate, history) not in _meters:
        x, lengths = clips(rate)
        ms = [RL.meter(x[b, 0, :n].numpy(), rate, history) for b, n in enumerate(lengths)]
        for m in ms:
            assert m["margin"] >= 0.05, m["margin"]
        _meters[(rate, history)] = ms
    return _meters[(rate, history)]


def poison_behind(x, lengths):
    x = x.clone()
    for b, n in enumerate(lengths):
        x[b, :, n:] = float("nan")
    return x


# ------------------------------------------------------------------------------------- 1. stream == one pass
def partitions(lengths, step):
    def fixed(sizes):
        left, steps, i = list(lengths), [], 0
        while any(left):
            take = [min(n, sizes[i % len(sizes)]) for n in left]
            steps.append(take)
            left = [n - s for n, s in zip(left, take)]
            i += 1
        return steps
    plans = {"8192-sample blocks": fixed([8192]), "one push": [list(lengths)],
             "1, 0, step - 1, step, step + 1, 3 step + 5 in turn": fixed([1, 0, step - 1, step, step + 1, 3 * step + 5])}
    g = torch.Generator().manual_seed(5)
    ragged, left = [], list(lengths)
    while any(left):
        take = [min(n, int(torch.randint(0, 3 * step, (1,), generator=g))) if (len(ragged) + b) % 4 else 0 for b, n in enumerate(left)]
        ragged.append(take)
        left = [n - s for n, s in zip(left, take)]
    plans["other counts per clip"] = ragged
    return plans


def run_stream(target, x, steps, early_final=True):
    """push the plan -> (per-clip concatenation of the outputs, the last info, per-clip concatenations of momentary / integrated_steps)"""
    B = x.shape[0]
    stream = LoudnessStream(target, B, DEV)
    at, left = [0] * B, [sum(s[b] for s in steps) for b in range(B)]
    parts, mom, integ = [[] for _ in range(B)], [[] for _ in range(B)], [[] for _ in range(B)]
    info = None
    for take in steps:
        blk = torch.full((B, 1, max(max(take), 1)), float("nan"))         # what a block holds behind a clip's samples is never read
        for b in range(B):
            blk[b, 0, :take[b]] = x[b, 0, at[b]:at[b] + take[b]]
            at[b] += take[b]
            left[b] -= take[b]
        audio = None if max(take) == 0 else blk.to(DEV)
        fin = [n == 0 for n in left] if early_final else all(n == 0 for n in left)
        out, info = stream.push(audio, samples=None if audio is None else take, final=fin)
        assert out.shape[-1] == max(take) and stream.received == at
        for b in range(B):
            parts[b].append(out[b, 0, :take[b]])
            assert bool((out[b, 0, take[b]:] == 0).all())
            mom[b].append(info["momentary"][b, :info["blocks"][b]])
            integ[b].append(info["integrated_steps"][b, :info["boundaries"][b]])
            assert bool(info["momentary"][b, info["blocks"][b]:].isnan().all())
    return [torch.cat(p) for p in parts], info, [torch.cat(p) for p in mom], [torch.cat(p) for p in integ]


def same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7777.0), torch.nan_to_num(b, nan=-7777.0)) and torch.equal(a.isnan(), b.isnan())


PARAMS = [dict(limiter=lim, slew_db_per_s=slew, history_steps=h) for lim in ("clip", "tanh") for slew in (None, 3.0) for h in (8, 4096)]


@pytest.mark.parametrize("kw", PARAMS, ids=lambda k: f"{k['limiter']}-slew{k['slew_db_per_s']}-h{k['history_steps']}")
def test_pushes_concatenated_are_the_one_pass_result(kw):
    rate = 44100
    x, lengths = clips(rate)
    target = LoudnessTarget(sample_rate=rate, **kw)
    want, winfo = normalize_loudness_causal(poison_behind(x, lengths).to(DEV), target, lengths=lengths)
    assert want.shape == x.shape and winfo["blocks"] == [19, 2, 0] and winfo["boundaries"] == [22, 5, 3]
    if kw["slew_db_per_s"] is not None:                                   # the slew binds: without it the first correction is a jump
        free, _ = normalize_loudness_causal(x.to(DEV), LoudnessTarget(sample_rate=rate, **dict(kw, slew_db_per_s=None)), lengths=lengths)
        assert not torch.equal(free, want)
        steps = winfo["integrated_steps"][0].cpu().double().numpy()
        d = RL.gains_db(np.concatenate([[np.nan], steps]), slew=3.0)
        assert np.isclose(np.abs(np.diff(d)), 0.3, rtol=0, atol=1e-9).any()
    for name, steps in partitions(lengths, target.plan.step).items():
        got, info, mom, integ = run_stream(target, x, steps)
        for b, n in enumerate(lengths):
            assert got[b].shape[0] == n and torch.equal(got[b], want[b, 0, :n]), (name, b)
            assert same(mom[b], winfo["momentary"][b, :winfo["blocks"][b]]), (name, b)
            assert same(integ[b], winfo["integrated_steps"][b, :winfo["boundaries"][b]]), (name, b)
        for key in ("gain_db", "integrated", "clipped"):
            assert same(info[key].float(), winfo[key].float()), (name, key)
    assert bool((want[1, 0, lengths[1]:] == 0).all()) and bool((want[2, 0, lengths[2]:] == 0).all())


@pytest.mark.parametrize("rate", [48000, 16000])
def test_pushes_concatenated_are_the_one_pass_result_at_other_rates(rate):
    x, lengths = clips(rate)
    target = LoudnessTarget(sample_rate=rate, slew_db_per_s=3.0, limiter="tanh", initial_gain_db=-3.0)
    want, winfo = normalize_loudness_causal(poison_behind(x, lengths).to(DEV), target, lengths=lengths)
    for name, steps in partitions(lengths, target.plan.step).items():
        got, info, mom, integ = run_stream(target, x, steps, early_final=False)
        for b, n in enumerate(lengths):
            assert torch.equal(got[b], want[b, 0, :n]), (name, b)
            assert same(mom[b], winfo["momentary"][b, :winfo["blocks"][b]]), (name, b)
        for key in ("gain_db", "integrated", "clipped"):
            assert same(info[key].float(), winfo[key].float()), (name, key)


# ------------------------------------------------------------------------------------- 2. against float64
def level_bar(l, e, n):
    return 10 / math.log(10) * (n + 3) * U + 20 * U * np.abs(np.log10(e)) + 4 * U * (np.abs(l) + 0.691)


def integrated_bar(I, mean, count):
    return 10 / math.log(10) * (count + 7) * U + 20 * U * np.abs(np.log10(mean)) + 4 * U * (np.abs(I) + 0.691)


def test_meter_against_float64_and_the_parent_kernel():
    new_err, parent_err, worst_m = 0.0, 0.0, 0.0
    for rate in RATES:
        x, lengths = clips(rate)
        ms = oracle_meter(rate, 4096)
        got = measure_loudness(poison_behind(x, lengths).to(DEV), lengths=lengths, sample_rate=rate)
        assert got["blocks"] == [19, 2, 0] and got["windows"] == [0, 0, 0] and got["step"] == RL.step_of(rate)
        assert tuple(got["momentary"].shape) == (3, 19) and tuple(got["short_term"].shape) == (3, 0)
        parent = normalize_audio(poison_behind(x, lengths).to(DEV), strategy="loudness", sample_rate=rate, lengths=lengths)
        pg = parent.loudness_gains.cpu().double()
        assert parent.loudness_untouched.tolist() == [False, False, True]
        integ = got["integrated"].cpu().double()
        assert math.isnan(float(integ[2])) and math.isnan(ms[2]["I"][-1]) and bool(got["momentary"][2].isnan().all())
        for b in (0, 1):
            want = ms[b]["I"][-1]
            new_err = max(new_err, abs(float(integ[b]) - want))
            parent_err = max(parent_err, abs(-12.0 - 20.0 * math.log10(float(pg[b])) - want))
            S, step = ms[b]["S"], ms[b]["step"]
            e = np.array([(S[j] + S[j + 1] + S[j + 2] + S[j + 3]) / (4 * step) for j in range(len(S) - 3)])
            mom = got["momentary"][b, :got["blocks"][b]].cpu().double().numpy()
            ratio = np.abs(mom - ms[b]["momentary"]) / level_bar(ms[b]["momentary"], e, 4)
            worst_m = max(worst_m, float(ratio.max()))
            assert bool(got["momentary"][b, got["blocks"][b]:].isnan().all())
    _lines["integrated, largest |LKFS - float64| over 3 rates x 2 clips"] = (
        f"new meter {new_err:.3e} dB, parent's serial fp32 kernel {parent_err:.3e} dB, ratio {new_err / max(parent_err, 1e-300):.3f} (bar 4)")
    _lines["momentary, largest |error| / bar"] = f"{worst_m:.4f}"
    print(_lines)
    assert worst_m <= 1.0
    assert new_err <= 4.0 * parent_err


def test_short_term_and_a_wrapped_ring_against_float64():
    rate, step = 16000, 1600
    x = RL.stepped_noise(rate, RL.AMPS + [0.1] * 5 + [0.4] * 6, 321, 0.3, seed=0)       # 33 steps: four 3 s windows
    worst_s, worst_i, worst_db = 0.0, 0.0, 0.0
    for history in (8, 4096):
        m = RL.meter(x, rate, history)
        assert m["margin"] >= 0.05 and m["short_term"].shape == (4,)
        # step by step, so that every boundary's integrated value is seen; the ring of history 8 wraps four times
        stream = LoudnessStream(LoudnessTarget(sample_rate=rate, history_steps=history), 1, DEV)
        integ, st = [], []
        dev = torch.from_numpy(x)[None, None].to(DEV)
        for j in range(33):
            _, info = stream.push(dev[:, :, j * step:(j + 1) * step].contiguous())
            assert info["boundaries"] == [1]
            integ.append(info["integrated_steps"][0, 0])
            st.append(info["short_term"][0, :info["windows"][0]])
        integ = torch.stack(integ).cpu().double().numpy()
        st = torch.cat(st).cpu().double().numpy()
        want = m["I"][1:]
        assert np.array_equal(np.isnan(integ), np.isnan(want))
        ok = ~np.isnan(want)
        assert ok.sum() == 30                                            # every boundary from the fourth on is defined and compared
        bar = integrated_bar(want[ok], m["I_mean"][1:][ok], m["I_count"][1:][ok])
        ratio = np.abs(integ[ok] - want[ok]) / bar
        print(f"history {history}: integrated |error| / bar per boundary", np.round(ratio, 3), "largest |error|", np.abs(integ[ok] - want[ok]).max())
        worst_i = max(worst_i, float(ratio.max()))
        worst_db = max(worst_db, float(np.abs(integ[ok] - want[ok]).max()))
        e = np.array([m["S"][j:j + 30].sum() / (30 * step) for j in range(4)])
        worst_s = max(worst_s, float((np.abs(st - m["short_term"]) / level_bar(m["short_term"], e, 30)).max()))
        one = measure_loudness(dev, sample_rate=rate, history_steps=history)
        assert one["windows"] == [4] and torch.equal(one["short_term"][0].cpu().double(), torch.from_numpy(st))
        assert float(one["integrated"][0]) == integ[-1]
    _lines["short-term, largest |error| / bar"] = f"{worst_s:.4f}"
    _lines["integrated at every boundary of 33 steps (history 8 and 4096), largest |error| / bar"] = f"{worst_i:.4f} (largest |error| {worst_db:.3e} dB)"
    print(_lines)
    assert worst_s <= 1.0
    assert worst_i <= 1.0


@pytest.mark.parametrize("limiter,slew", [("clip", None), ("tanh", 3.0)])
@pytest.mark.parametrize("rate", RATES)
def test_normalised_samples_against_float64(rate, limiter, slew):
    x, lengths = clips(rate)
    oracle_meter(rate, 4096)                                             # the condition on the inputs
    kw = dict(max_gain_db=20.0, initial_gain_db=2.0)
    target = LoudnessTarget(sample_rate=rate, limiter=limiter, slew_db_per_s=slew, **kw)
    got, info = normalize_loudness_causal(poison_behind(x, lengths).to(DEV), target, lengths=lengths)
    g = got.cpu().double().numpy()
    worst = 0.0
    for b, n in enumerate(lengths):
        # the normaliser of the oracle on the integrated values the device's meter produced (test_short_term_and_a_wrapped_ring_against_float64 holds those to the oracle's at every boundary)
        I = np.concatenate([[np.nan], info["integrated_steps"][b, :info["boundaries"][b]].cpu().double().numpy()])
        ref = RL.normalise(x[b, 0, :n].numpy(), rate, I, slew=slew, limiter=limiter, **kw)
        near_one = np.abs(ref["xg"] - 1.0) <= 8 * U + ref["bar"]
        assert not near_one.any()                                        # no sample whose |x g| > 1 could be decided either way
        err = np.abs(g[b, 0, :n] - ref["out"])
        assert bool((err <= ref["bar"]).all()), (b, float((err - ref["bar"]).max()))
        nz = ref["bar"] > 0
        worst = max(worst, float((err[nz] / ref["bar"][nz]).max()))
        assert int(info["clipped"][b]) == ref["clipped"], b
        assert abs(float(info["gain_db"][b]) - ref["d"][-1]) <= 3 * U * 20.0 * (len(ref["d"]) + 1)
    assert int(info["clipped"][0]) > 0
    _lines[f"normalised samples, {rate} Hz, {limiter}, slew {slew}: largest |error| / bar"] = f"{worst:.4f}"
    print(rate, limiter, slew, worst)


# ------------------------------------------------------------------------------------- 3. semantics
def test_clips_are_independent_and_the_short_clip_is_untouched():
    rate = 44100
    x, lengths = clips(rate)
    target = LoudnessTarget(sample_rate=rate)
    want, winfo = normalize_loudness_causal(x.to(DEV), target, lengths=lengths)
    other = x.clone()
    other[0] = float("nan")
    other[2] = 5.0
    got, info = normalize_loudness_causal(other.to(DEV), target, lengths=[777, lengths[1], lengths[0]])
    assert torch.equal(got[1], want[1]) and same(info["integrated"][1], winfo["integrated"][1])
    perm = [2, 0, 1]
    moved, minfo = normalize_loudness_causal(x[perm].contiguous().to(DEV), target, lengths=[lengths[p] for p in perm])
    for i, p in enumerate(perm):
        assert torch.equal(moved[i], want[p]) and same(minfo["gain_db"][i], winfo["gain_db"][p]) and int(minfo["clipped"][i]) == int(winfo["clipped"][p])
    n = lengths[2]                                                       # three steps: no gating block, gain = initial_gain_db = 0 dB
    assert torch.equal(want[2, 0, :n], x[2, 0, :n].to(DEV).clamp(-1.0, 1.0)) and math.isnan(float(winfo["integrated"][2]))
    assert float(winfo["gain_db"][2]) == 0.0 and float(winfo["gain_db"][0]) != 0.0


def test_a_state_full_of_ff_bytes_and_a_clamped_correction():
    rate, step = 44100, 4410
    x, lengths = clips(rate)
    target = LoudnessTarget(sample_rate=rate, max_gain_db=6.0, history_steps=8)
    want, winfo = normalize_loudness_causal(x.to(DEV), target, lengths=lengths)
    stream = LoudnessStream(target, 3, DEV)
    stream._state.view(torch.uint8).fill_(0xFF)
    dev = x.to(DEV)
    parts, gains = [], []
    for j in range(0, x.shape[-1], step):                                # one boundary per push: every d_m is seen
        take = [max(0, min(step, n - j)) for n in lengths]
        out, info = stream.push(dev[:, :, j:j + step].contiguous(), samples=take)
        parts.append(out)
        gains.append(info["gain_db"])
    got = torch.cat(parts, dim=-1)
    for b, n in enumerate(lengths):
        assert torch.equal(got[b, 0, :n], want[b, 0, :n]), b
    g = torch.stack(gains).cpu()
    assert float(g.abs().max()) == 6.0 and bool((g.abs() <= 6.0).all())   # the clamp binds somewhere and holds everywhere
    assert same(info["gain_db"], winfo["gain_db"]) and torch.equal(info["clipped"], winfo["clipped"])


def raw_push(x, out, rec, state, rate, history, table, n_table, gains, meter, stride, info, clipped, B, in_stride, target=-12.0,
             max_gain=20.0, slew=0.0, init=0.0, limiter=0):
    rc = L.lib().vaura_audio_loudness_push(x, out, B, in_stride, rec, state, rate, history, table, n_table, target, max_gain, slew, init,
                                           limiter, gains, meter, stride, info, clipped, L.current_stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc


def test_guards_around_the_output_and_refusals_through_the_c_entry():
    rate = 16000
    x, lengths = clips(rate)
    pl = LD.LoudnessPlan(rate)
    B, N, guard = 3, x.shape[-1], 4096
    dev = poison_behind(x, lengths).to(DEV)
    rec = torch.tensor([[0, n] for n in lengths], dtype=torch.int64, device=DEV)
    table = torch.from_numpy(pl.table()).to(DEV)
    lib = L.lib()
    words = lib.vaura_audio_loudness_state_elems(B, rate, 4096)
    assert words == B * ((24 + 4096 + pl.step + 3) // 4 * 4) and lib.vaura_audio_loudness_table_elems(rate) == table.numel()
    assert 0 < lib.vaura_audio_loudness_lds_bytes(rate) <= 64 * 1024 and 0 < lib.vaura_audio_loudness_lds_bytes(48000) <= 64 * 1024
    assert lib.vaura_audio_loudness_lds_bytes(11025) == 0 and lib.vaura_audio_loudness_state_elems(B, rate, 4) == 0
    state = torch.full((words,), -77.0, device=DEV)
    stride = 22
    raw = torch.full((2 * guard + B * N,), -77.0, device=DEV)
    out = raw[guard:guard + B * N]
    gains, meter = torch.full((B, stride + 2), -77.0, device=DEV), torch.full((3, B, stride), -77.0, device=DEV)
    info, clipped = torch.full((B, 2), -77.0, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    base = dict(x=L.ptr(dev), out=L.ptr(out), rec=L.ptr(rec), state=L.ptr(state), rate=rate, history=4096, table=L.ptr(table),
                n_table=table.numel(), gains=L.ptr(gains), meter=L.ptr(meter), stride=stride, info=L.ptr(info), clipped=L.ptr(clipped),
                B=B, in_stride=N)
    ARG, SHAPE, DTYPE = -1, -2, -3
    cases = [(ARG, dict(x=0)), (ARG, dict(rec=0)), (ARG, dict(state=0)), (ARG, dict(table=0)), (ARG, dict(gains=0)), (ARG, dict(meter=0)),
             (ARG, dict(info=0)), (ARG, dict(clipped=0)), (ARG, dict(out=L.ptr(dev))), (ARG, dict(x=L.ptr(dev) + 2)), (ARG, dict(state=L.ptr(state) + 4)),
             (ARG, dict(rec=L.ptr(rec) + 4)), (ARG, dict(B=0)), (ARG, dict(in_stride=0)), (ARG, dict(stride=0)), (ARG, dict(n_table=table.numel() - 1)),
             (ARG, dict(max_gain=-1.0)), (ARG, dict(target=float("nan"))), (ARG, dict(slew=-0.5)), (ARG, dict(init=float("inf"))),
             (DTYPE, dict(limiter=2)), (DTYPE, dict(limiter=-1)), (SHAPE, dict(rate=11025)), (SHAPE, dict(rate=7999)), (SHAPE, dict(rate=48001)),
             (SHAPE, dict(history=4)), (SHAPE, dict(history=4097)), (SHAPE, dict(B=65536)), (SHAPE, dict(in_stride=2 ** 31))]
    for code, kw in cases:
        assert raw_push(**dict(base, **kw)) == code, kw
    for t in (raw, state, gains, meter, info):
        assert bool((t == -77.0).all())                                  # no refused call launched anything
    assert raw_push(**base) == 0                                         # and the same arguments, unaltered, run
    assert bool((raw[:guard] == -77.0).all()) and bool((raw[guard + B * N:] == -77.0).all())
    want, winfo = normalize_loudness_causal(dev, LoudnessTarget(sample_rate=rate), lengths=lengths)
    assert torch.equal(out.view(B, 1, N), want) and torch.equal(info[:, 0], winfo["gain_db"]) and torch.equal(clipped, winfo["clipped"])
    for b, n in enumerate(lengths):
        assert bool((out.view(B, N)[b, n:] == 0).all()) and bool(torch.isfinite(out.view(B, N)[b]).all())


# ------------------------------------------------------------------------------------- 4. composition
@pytest.fixture(scope="module")
def model(tiny_sampler_sd):
    return G._model(tiny_sampler_sd)


def check_generate_stream(model, target, B, T, pcm_fmt=None, **kw):
    hop = synth.FULL_CODEC.hop
    frames = synth.video_features(B, tokens=32, seed=31).reshape(B, 1, 32, 768).to(DEV)
    ref = model.generate(frames=frames, max_new_tokens=T, prompt_is_encoded=True, use_sampling=False, cfg_scale=1.0, **kw)
    lengths = [t * hop for t in T] if isinstance(T, list) else [T * hop] * B
    want, winfo = normalize_loudness_causal(ref["generated_audio"], target, lengths=lengths)
    raw = model.generate_stream(frames=frames, max_new_tokens=T, prompt_is_encoded=True, block_frames=7, use_sampling=False, cfg_scale=1.0, **kw)
    wrapped = model.loudness_stream(raw, target)
    blocks = list(stream_pcm(wrapped, pcm_fmt) if pcm_fmt is not None else wrapped)
    assert len(blocks) > 2 and blocks[-1]["final"]
    at = [0] * B
    for blk in blocks:
        fr = blk["frames"] if isinstance(blk["frames"], (list, tuple)) else [blk["frames"]] * B
        for b in range(B):
            n = fr[b] * hop
            assert torch.equal(blk["audio"][b, 0, :n], want[b, 0, at[b]:at[b] + n]), b
            at[b] += n
    assert at == lengths and same(blocks[-1]["loudness_gain_db"], winfo["gain_db"]) and torch.equal(blocks[-1]["loudness_clipped"], winfo["clipped"])
    if pcm_fmt is not None:
        pcm_want, n_out = post.audio_to_pcm(want, pcm_fmt, lengths=lengths)
        for b in range(B):
            got = torch.cat([blk["pcm"][b, :blk["pcm_samples"][b]] for blk in blocks])
            assert torch.equal(got, pcm_want[b, :int(n_out[b])]), b
    return want


def test_stream_loudness_of_generate_stream_is_the_causal_normaliser_of_generate(model):
    target = LoudnessTarget(max_gain_db=30.0)
    want = check_generate_stream(model, target, 4, [43, 23, 9, 1], video_lengths=[32, 20, 9, 1])
    assert bool(torch.isfinite(want).all())


def test_stream_pcm_composes_on_top_of_stream_loudness(model):
    check_generate_stream(model, LoudnessTarget(limiter="tanh", slew_db_per_s=20.0), 2, 43, pcm_fmt=PcmFormat())


def test_the_blocks_of_a_live_session_go_through_stream_loudness(model):
    B, SEG = 2, 8
    feats = synth.video_features(B, tokens=6 * SEG, seed=71).reshape(B, 6, SEG, 768).to(DEV)
    s = model.open_live(B, block_frames=16, use_sampling=False, cfg_scale=1.0)
    blocks = []
    for i in range(5):
        blocks += s.push(features=feats[:, i])
    blocks += s.close()
    assert len(blocks) > 2 and blocks[-1]["final"]
    whole = torch.cat([blk["audio"] for blk in blocks], dim=-1)
    target = LoudnessTarget()
    want, winfo = normalize_loudness_causal(whole, target)
    got = list(stream_loudness(blocks, target))
    assert torch.equal(torch.cat([blk["audio"] for blk in got], dim=-1), want)
    assert same(got[-1]["loudness_integrated"], winfo["integrated"]) and sum(blk["loudness_blocks"][0] for blk in got) == winfo["blocks"][0]
    assert all(torch.equal(a["sampled_indices"], b["sampled_indices"]) for a, b in zip(blocks, got))


# ------------------------------------------------------------------------------------- 5. refusals before any launch
def test_refusals():
    with pytest.raises(L.VauraHipError):
        LoudnessTarget(sample_rate=11025)
    with pytest.raises(L.VauraHipError):
        LoudnessTarget(history_steps=4)
    with pytest.raises(L.VauraHipError):
        measure_loudness(torch.zeros(1, 1, 20000, device=DEV), sample_rate=11025)
    target = LoudnessTarget()
    stream = LoudnessStream(target, 2, DEV)
    x = torch.zeros(2, 1, 1000, device=DEV)
    with pytest.raises(L.VauraHipError):
        stream.push(torch.zeros(3, 1, 1000, device=DEV))                 # a batch mismatch
    with pytest.raises(L.VauraHipError):
        stream.push(x.cpu())                                             # a CPU tensor
    with pytest.raises(L.VauraHipError):
        stream.push(x, samples=[1000, 1001])
    with pytest.raises(L.VauraHipError):
        stream.push(x, samples=[1, 2, 3])
    assert stream.received == [0, 0]                                     # nothing refused has moved the stream
    stream.push(x, final=[True, False])
    with pytest.raises(L.VauraHipError, match="takes no more samples"):
        stream.push(x)
    out, _ = stream.push(x, samples=[0, 1000])
    assert stream.received == [1000, 2000] and stream.finished == [True, False] and out.shape == (2, 1, 1000)
    with pytest.raises(L.VauraHipError):
        normalize_loudness_causal(x.cpu(), target)
    with pytest.raises(L.VauraHipError):
        normalize_loudness_causal(x, target, lengths=[1000])
    with pytest.raises(L.VauraHipError):
        measure_loudness(x, lengths=[0, 5])
