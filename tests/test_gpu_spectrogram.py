"""Spectrograms on the GPU: vaura_spectrogram (csrc/spectrogram.hip) through post.audio_to_spectrogram / SpectrogramStream /
stream_spectrogram.

  1. the transform itself (scale "complex"), the linear power spectrum and the mel power against the float64 restatement of
     tests/spectrogram_reference.py under its derived bars, every entry; beside them the measured condition: the device's largest
     |X^ - X| / beta is at most 4 times that of torch's fp32 rfft on the same frames;
  2. "db" / "log" are the device's own power output through the float64 formula, within the device log's documented error;
  3. per-clip lengths: NaN behind every length, a guard pattern behind the rows; 4. clips independent; 5. a NaN sample reaches exactly
     the columns whose window holds it; 6. pushes concatenated are the one-pass result; 7. a block at r0 ~ 2^33 is the block at the
     stream's start; 8. end to end on the tiny model; 9. the C entry's refusals leave guard-filled outputs untouched.

Every case prints its largest error over bar and the ratio to torch's figure; with VAURA_PARITY_DIR set they go to
spectrogram_parity.txt.

Shapes: three clips of 5 hops, 3 hops + 7 and hop - 212 samples (hop - 53 at hop 128): a whole clip, a ragged tail, a clip
shorter than one hop and far shorter than a window."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrogram_reference as RS  # noqa: E402
import test_gpu_per_clip_sampling as G  # noqa: E402  (the tiny plugin model)
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import post, synth  # noqa: E402
from vaura_amd import spectrogram as SG  # noqa: E402
from vaura_amd.post import (PcmFormat, SpectrogramFormat, SpectrogramStream, audio_to_spectrogram, stream_pcm,  # noqa: E402
                            stream_spectrogram)

DEV = "cuda:0"
SIZES = [(2048, 512), (512, 128), (1024, 512)]
_lines = {}


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    out = os.environ.get("VAURA_PARITY_DIR")
    if _lines and out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "spectrogram_parity.txt"), "w") as f:
            f.write("spectrogram against float64 (tests/test_gpu_spectrogram.py): largest |error| / bar per case; the largest error of\n"
                    "the transform in units of beta = 2^-24 sum |y|, the same of torch's fp32 rfft, and their ratio (at most 4)\n")
            for k in sorted(_lines):
                f.write(f"{_lines[k]}  {k}\n")


def lengths_for(hop):
    return [5 * hop, 3 * hop + 7, hop - 212 if hop > 212 else hop - 53]


@pytest.fixture(scope="module")
def noise():
    """(3, 1, 5 * 512) fp32 on the host, computed once and left unchanged"""
    return torch.randn(3, 1, 5 * 512, generator=torch.Generator().manual_seed(23)) * 0.3


def clips_of(noise, hop):
    lengths = lengths_for(hop)
    return noise[:, :, :max(lengths)].contiguous(), lengths


def poison_behind(x, lengths):
    x = x.clone()
    for b, nb in enumerate(lengths):
        x[b, :, nb:] = float("nan")
    return x


_refs = {}


def reference(noise, n_fft, hop):
    """per clip: (X, beta, y32, P, barP), computed once per size"""
    if (n_fft, hop) not in _refs:
        x, lengths = clips_of(noise, hop)
        out = []
        for b, n in enumerate(lengths):
            X, beta, y32 = RS.spectrum(x[b, 0, :n], n_fft, hop)
            P, barP = RS.power_bar(X, beta, n_fft)
            out.append((X, beta, y32, P, barP))
        _refs[(n_fft, hop)] = out
    return _refs[(n_fft, hop)]


# ------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("n_fft,hop", SIZES)
def test_transform_and_linear_power_against_float64(noise, n_fft, hop):
    x, lengths = clips_of(noise, hop)
    dev_x = poison_behind(x, lengths).to(DEV)
    got, cols = audio_to_spectrogram(dev_x, SpectrogramFormat(n_fft=n_fft, hop=hop, n_mels=None, scale="power"), lengths=lengths)
    spec, cols2 = audio_to_spectrogram(dev_x, SpectrogramFormat(n_fft=n_fft, hop=hop, n_mels=None, scale="complex"), lengths=lengths)
    assert got.dtype == torch.float32 and got.device.type == "cuda" and cols.tolist() == cols2.tolist() == [5, 4, 1]
    assert tuple(got.shape) == (3, 5, n_fft // 2 + 1) and tuple(spec.shape) == (3, 5, n_fft // 2 + 1, 2)
    g, z = got.cpu().double(), torch.view_as_complex(spec.cpu().double().contiguous())
    worst_x, worst_p, dev_units, torch_units = 0.0, 0.0, 0.0, 0.0
    for b, (X, beta, y32, P, barP) in enumerate(reference(noise, n_fft, hop)):
        c = X.shape[0]
        assert bool(torch.isfinite(g[b, :c]).all()) and bool((g[b, c:] == 0).all()) and bool((spec[b, c:] == 0).all())
        assert bool((beta > 0).all())
        units = (z[b, :c] - X).abs() / beta[:, None]
        worst_x = max(worst_x, float(units.max()) / RS.C_ROUNDINGS[n_fft])
        worst_p = max(worst_p, float(((g[b, :c] - P).abs() / barP).max()))
        dev_units = max(dev_units, float(units.max()))
        torch_units = max(torch_units, RS.torch_fp32_units(y32, X, beta))
        assert torch.equal(got[b, :c].cpu(), (spec[b, :c, :, 0] * spec[b, :c, :, 0] + spec[b, :c, :, 1] * spec[b, :c, :, 1]).cpu())   # P is re re + im im
    case = f"linear, n_fft {n_fft}, hop {hop}"
    _lines[case] = (f"X {worst_x:7.4f} of bar, P {worst_p:7.4f} of bar; device {dev_units:6.3f} units, torch fp32 {torch_units:6.3f}, "
                    f"ratio {dev_units / torch_units:5.2f}")
    print(case, _lines[case])
    assert worst_x <= 1.0 and worst_p <= 1.0
    assert dev_units <= 4.0 * torch_units


MEL_CASES = [(2048, 512, 128, "slaney", None), (2048, 512, 64, "slaney", None), (2048, 512, 128, "htk", None), (2048, 512, 128, "slaney", "slaney"),
             (2048, 512, 64, "htk", "slaney"), (1024, 512, 128, "slaney", None), (1024, 512, 64, "htk", None), (512, 128, 64, "slaney", None),
             (512, 128, 40, "htk", None)]


@pytest.mark.parametrize("n_fft,hop,n_mels,mel_scale,norm", MEL_CASES)
def test_mel_power_against_float64(noise, n_fft, hop, n_mels, mel_scale, norm):
    x, lengths = clips_of(noise, hop)
    fmt = SpectrogramFormat(n_fft=n_fft, hop=hop, n_mels=n_mels, mel_scale=mel_scale, norm=norm, scale="power")
    got, cols = audio_to_spectrogram(poison_behind(x, lengths).to(DEV), fmt, lengths=lengths)
    assert tuple(got.shape) == (3, 5, n_mels) and cols.tolist() == [5, 4, 1]
    want_fb, _ = RS.mel_filters(n_fft, n_mels, 0.0, None, mel_scale, norm)
    fb32 = SG.expand(fmt.mel, n_fft // 2 + 1).double()                    # the weights the kernel was given: the restated ones, rounded once
    assert float((fb32 - want_fb).abs().max()) <= 2.0 ** -24 * float(want_fb.max())
    g = got.cpu().double()
    worst = 0.0
    for b, (X, beta, y32, P, barP) in enumerate(reference(noise, n_fft, hop)):
        c = X.shape[0]
        M, barM = RS.mel_bar(fb32, P, barP)
        assert bool(torch.isfinite(g[b, :c]).all()) and bool((g[b, c:] == 0).all()) and bool((M > 0).all())
        worst = max(worst, float(((g[b, :c] - M).abs() / barM).max()))
    case = f"mel power, n_fft {n_fft}, hop {hop}, {n_mels} {mel_scale} bands, norm {norm}"
    _lines[case] = f"{worst:8.4f} of bar"
    print(case, _lines[case])
    assert worst <= 1.0


# ------------------------------------------------------------------------------------- 2. scales
@pytest.mark.parametrize("scale", ["db", "log"])
@pytest.mark.parametrize("n_mels", [None, 128])
def test_db_and_log_are_the_scaled_power_output(noise, scale, n_mels):
    x, lengths = clips_of(noise, 512)
    x = x.clone()
    x[2] = 0.0                                                            # an all-zero clip: amin is reached
    kw = dict(n_mels=n_mels, amin=1e-7)
    power, cols = audio_to_spectrogram(x.to(DEV), SpectrogramFormat(scale="power", **kw), lengths=lengths)
    got, cols2 = audio_to_spectrogram(x.to(DEV), SpectrogramFormat(scale=scale, **kw), lengths=lengths)
    assert cols.tolist() == cols2.tolist() and got.shape == power.shape
    want, bar = RS.scaled(power.cpu(), scale, 1e-7)
    g = got.cpu().double()
    worst = 0.0
    for b, c in enumerate(cols.tolist()):
        err = (g[b, :c] - want[b, :c]).abs()
        assert bool((err <= bar[b, :c]).all()), (b, float((err - bar[b, :c]).max()))
        worst = max(worst, float((err / bar[b, :c].clamp(min=1e-300)).max()))
        assert bool((g[b, c:] == 0).all())                                # rows behind the clip are zeros, not log(amin)
    floor = 10 * torch.log10(torch.tensor(1e-7, dtype=torch.float32).double()) if scale == "db" else torch.log(torch.tensor(1e-7, dtype=torch.float32).double())
    assert bool((power[2, :1] == 0).all()) and float((g[2, 0] - floor).abs().max()) <= float(bar[2, 0].max())
    case = f"{scale} of the device's power, {'linear' if n_mels is None else 'mel'}"
    _lines[case] = f"{worst:8.4f} of bar"
    print(case, _lines[case])


# ------------------------------------------------------------------------------------- 3. / 4. lengths, guards, independence
def tables(fmt):
    return post._spec_table(fmt, torch.device(DEV))


def raw_launch(fmt, x, records, out, out_stride, carry_in=None, carry_out=None):
    win, tw, bins, weights = tables(fmt)
    B = x.shape[0]
    rec = torch.tensor(records, dtype=torch.int64, device=DEV)
    rc = L.lib().vaura_spectrogram(L.ptr(x), B, x.shape[-1], L.ptr(rec), L.ptr(carry_in), L.ptr(carry_out),
                                   0 if carry_in is None else carry_in.shape[-1], fmt.n_fft, fmt.hop, L.ptr(win), L.ptr(tw), L.ptr(bins),
                                   L.ptr(weights), 0 if weights is None else weights.numel(), fmt.bins, SG.SCALES[fmt.scale], fmt.amin,
                                   L.ptr(out), out_stride, L.current_stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("n_fft,hop,n_mels", [(2048, 512, 128), (512, 128, None), (1024, 512, 64)])
def test_per_clip_lengths_poisoned_input_and_guarded_output(noise, n_fft, hop, n_mels):
    fmt = SpectrogramFormat(n_fft=n_fft, hop=hop, n_mels=n_mels)
    x, lengths = clips_of(noise, hop)
    got, cols = audio_to_spectrogram(poison_behind(x, lengths).to(DEV), fmt, lengths=lengths)
    for b, n in enumerate(lengths):                                       # each clip is the clip converted alone at its own length
        alone, alone_cols = audio_to_spectrogram(x[b:b + 1, :, :n].contiguous().to(DEV), fmt)
        assert alone_cols.tolist() == [int(cols[b])] and torch.equal(got[b, :alone.shape[1]], alone[0]), b
        assert bool((got[b, alone.shape[1]:] == 0).all())
    F, stride, guard = fmt.bins, 7, 4096                                  # rows longer than any clip's columns, guards on both sides
    raw = torch.full((2 * guard + 3 * stride * F,), -77.0, dtype=torch.float32, device=DEV)
    out = raw[guard:guard + 3 * stride * F]
    records = [[0, n, 0, int(c), n] for n, c in zip(lengths, cols.tolist())]
    assert raw_launch(fmt, poison_behind(x, lengths).to(DEV), records, out, stride) == 0
    assert bool((raw[:guard] == -77.0).all()) and bool((raw[guard + 3 * stride * F:] == -77.0).all())
    rows = out.view(3, stride, F)
    for b, c in enumerate(cols.tolist()):
        assert torch.equal(rows[b, :c], got[b, :c]) and bool((rows[b, c:] == 0).all()), b


def test_clips_of_a_batch_are_independent(noise):
    fmt = SpectrogramFormat()
    x, lengths = clips_of(noise, 512)
    got, cols = audio_to_spectrogram(x.to(DEV), fmt, lengths=lengths)
    other = x.clone()
    other[0] = float("nan")
    other[2] = 5.0
    changed, _ = audio_to_spectrogram(other.to(DEV), fmt, lengths=lengths)
    assert torch.equal(changed[1], got[1]) and bool(changed[0, :5].isnan().all())
    perm = [2, 0, 1]
    moved, mcols = audio_to_spectrogram(x[perm].contiguous().to(DEV), fmt, lengths=[lengths[p] for p in perm])
    for i, p in enumerate(perm):
        assert torch.equal(moved[i], got[p]) and int(mcols[i]) == int(cols[p])


# ------------------------------------------------------------------------------------- 5. non-finite locality
@pytest.mark.parametrize("n_fft,hop,n_mels,scale", [(2048, 512, 128, "db"), (2048, 512, None, "power"), (512, 128, 64, "log")])
def test_a_nan_sample_reaches_exactly_the_columns_that_hold_it(n_fft, hop, n_mels, scale):
    fmt = SpectrogramFormat(n_fft=n_fft, hop=hop, n_mels=n_mels, scale=scale)
    x = torch.randn(1, 1, 12 * hop, generator=torch.Generator().manual_seed(9)) * 0.3
    clean, _ = audio_to_spectrogram(x.to(DEV), fmt)
    s = 6 * hop + 100 * hop // 512
    bad = x.clone()
    bad[0, 0, s] = float("nan")
    got, cols = audio_to_spectrogram(bad.to(DEV), fmt)
    hit = [t for t in range(12) if fmt.plan.lo(t) <= s < fmt.plan.lo(t) + n_fft]
    assert cols.tolist() == [12] and len(hit) == n_fft // hop
    if (n_fft, hop) == (2048, 512):
        assert hit == [4, 5, 6, 7]
    for t in range(12):
        if t in hit:
            assert bool(got[0, t].isnan().all()), t
        else:
            assert torch.equal(got[0, t], clean[0, t]), t


# ------------------------------------------------------------------------------------- 6. streaming
def block_plans(lengths, hop, n_fft):
    plans = {"one single push": [list(lengths)]}
    for size in (hop - 1, hop + 37, 3 * n_fft // 2 + 5, 77):
        left, steps = list(lengths), []
        while any(left):
            step = [min(n, size) for n in left]
            steps.append(step)
            left = [n - s for n, s in zip(left, step)]
        plans[f"{size} samples"] = steps
    g = torch.Generator().manual_seed(5)
    ragged, left = [], list(lengths)
    while any(left):
        if len(ragged) == 2:
            step = [0] * len(left)                                        # a push in which no clip brings a sample
        else:
            step = [min(n, int(torch.randint(0, 2 * hop, (1,), generator=g))) if (len(ragged) + b) % 4 else 0 for b, n in enumerate(left)]
        ragged.append(step)
        left = [n - s for n, s in zip(left, step)]
    plans["ragged per clip with zero-sample pushes"] = ragged
    return plans


def run_stream(fmt, x, steps, none_for_empty=False):
    """push the plan, the last block of every clip as its final one -> per-clip concatenation"""
    B = x.shape[0]
    stream = SpectrogramStream(fmt, B, DEV)
    at, left = [0] * B, [sum(s[b] for s in steps) for b in range(B)]
    parts = [[] for _ in range(B)]
    for step in steps:
        blk = torch.full((B, 1, max(max(step), 1)), float("nan"))         # what a block holds behind a clip's samples is never read
        for b in range(B):
            blk[b, 0, :step[b]] = x[b, 0, at[b]:at[b] + step[b]]
            at[b] += step[b]
            left[b] -= step[b]
        start = list(stream.emitted)
        audio = None if none_for_empty and max(step) == 0 else blk.to(DEV)
        spec, counts = stream.push(audio, samples=None if audio is None else step, final=[n == 0 for n in left])
        assert [s + c for s, c in zip(start, counts)] == stream.emitted and spec.shape[1] == max(counts)
        for b in range(B):
            parts[b].append(spec[b, :counts[b]])
            assert bool((spec[b, counts[b]:] == 0).all())
    return [torch.cat(p) for p in parts]


@pytest.mark.parametrize("n_fft,hop,n_mels", [(2048, 512, 128), (512, 128, 64), (2048, 512, None)])
def test_pushes_concatenated_are_the_one_pass_result(noise, n_fft, hop, n_mels):
    fmt = SpectrogramFormat(n_fft=n_fft, hop=hop, n_mels=n_mels)
    x, lengths = clips_of(noise, hop)
    want, cols = audio_to_spectrogram(poison_behind(x, lengths).to(DEV), fmt, lengths=lengths)
    plans = block_plans(lengths, hop, n_fft)
    assert any(max(s) < hop for s in plans[f"{hop - 1} samples"]) and [0, 0, 0] in plans["ragged per clip with zero-sample pushes"]
    for name, steps in plans.items():
        got = run_stream(fmt, x, steps, none_for_empty=name.startswith("ragged"))
        for b, c in enumerate(cols.tolist()):
            assert got[b].shape[0] == c and torch.equal(got[b], want[b, :c]), (name, b)


def test_a_push_shorter_than_a_hop_yields_no_column(noise):
    fmt = SpectrogramFormat()
    stream = SpectrogramStream(fmt, 2, DEV)
    spec, counts = stream.push(noise[:2, :, :300].contiguous().to(DEV))
    assert counts == [0, 0] and tuple(spec.shape) == (2, 0, 128)
    spec, counts = stream.push(None)
    assert counts == [0, 0] and stream.received == [300, 300]
    spec, counts = stream.push(None, final=[True, False])
    assert counts == [1, 0] and stream.finished == [True, False]
    want, _ = audio_to_spectrogram(noise[:1, :, :300].contiguous().to(DEV), fmt)
    assert torch.equal(spec[0], want[0])


# ------------------------------------------------------------------------------------- 7. 64-bit positions
def test_a_block_far_into_a_stream_is_the_block_at_its_start(noise):
    fmt = SpectrogramFormat(scale="power")
    pl = fmt.plan
    H = pl.history()
    x = noise[:2, :, :2000].contiguous().to(DEV)
    carry = noise[:2, 0, 300:300 + H].contiguous().to(DEV)
    outs = []
    for K in (8, 8 + 2 ** 24):                                            # 8 hops in: the first window lies wholly at or above sample 0
        r0 = K * 512 + 11
        t0, t1 = pl.releasable(r0), pl.releasable(r0 + 2000)
        assert t1 - t0 >= 3
        out = torch.empty(2, t1 - t0, 128, dtype=torch.float32, device=DEV)
        nxt = torch.zeros(2, H, device=DEV)
        assert raw_launch(fmt, x, [[r0, 2000, t0, t1 - t0, -1]] * 2, out, t1 - t0, carry, nxt) == 0
        assert torch.equal(nxt, torch.cat([carry, x[:, 0]], dim=1)[:, -H:])
        outs.append(out)
    assert r0 > 2 ** 33 and torch.equal(outs[0], outs[1]) and bool((outs[0] > 0).all())


# ------------------------------------------------------------------------------------- 8. end to end
@pytest.fixture(scope="module")
def model(tiny_sampler_sd):
    return G._model(tiny_sampler_sd)


def frames_of(B, seed=31):
    return synth.video_features(B, tokens=32, seed=seed).reshape(B, 1, 32, 768).to(DEV)


def check_end_to_end(model, fmt, B, T, wrap, **kw):
    hop = synth.FULL_CODEC.hop
    frames = frames_of(B)
    ref = model.generate(frames=frames, max_new_tokens=T, prompt_is_encoded=True, use_sampling=False, cfg_scale=1.0, **kw)
    lengths = [t * hop for t in T] if isinstance(T, list) else None
    want, cols = model.audio_to_spectrogram(ref["generated_audio"], fmt, lengths=lengths)
    assert cols.tolist() == (T if isinstance(T, list) else [T] * B)       # hop 512: one column per codec frame
    blocks = list(wrap(model.generate_stream(frames=frames, max_new_tokens=T, prompt_is_encoded=True, block_frames=7, use_sampling=False,
                                             cfg_scale=1.0, **kw)))
    assert len(blocks) > 2 and [b["final"] for b in blocks] == [False] * (len(blocks) - 1) + [True]
    at = [0] * B
    for blk in blocks:
        assert blk["spec_start"] == at and "audio" in blk
        for b in range(B):
            n = blk["spec_columns"][b]
            assert torch.equal(blk["spectrogram"][b, :n], want[b, at[b]:at[b] + n]), b
            at[b] += n
    assert at == cols.tolist()
    return blocks, ref, lengths


def test_stream_spectrogram_of_generate_stream_is_audio_to_spectrogram_of_generate(model):
    fmt = SpectrogramFormat()
    check_end_to_end(model, fmt, 2, 43, lambda s: stream_spectrogram(s, fmt))
    assert model.audio_to_spectrogram(torch.zeros(1, 1, 1024, device=DEV))[0].shape == (1, 2, 128)      # fmt None: the default format


def test_stream_spectrogram_with_per_clip_lengths(model):
    fmt = SpectrogramFormat(n_mels=64, scale="log")
    check_end_to_end(model, fmt, 4, [43, 23, 9, 1], lambda s: stream_spectrogram(s, fmt), video_lengths=[32, 20, 9, 1])


def test_stream_spectrogram_composes_with_stream_pcm_in_both_orders(model):
    fmt, pcm_fmt = SpectrogramFormat(), PcmFormat(gain=8.0)
    a, ref, lengths = check_end_to_end(model, fmt, 2, 43, lambda s: stream_spectrogram(stream_pcm(s, pcm_fmt), fmt))
    b, _, _ = check_end_to_end(model, fmt, 2, 43, lambda s: stream_pcm(stream_spectrogram(s, fmt), pcm_fmt))
    want, n_out = post.audio_to_pcm(ref["generated_audio"], pcm_fmt, lengths=lengths)
    for blocks in (a, b):
        pcm = torch.cat([blk["pcm"][:, :max(blk["pcm_samples"])] for blk in blocks], dim=1)
        assert all(blk["pcm_samples"][0] == blk["pcm_samples"][1] for blk in blocks)
        assert torch.equal(pcm, want) and sum(blk["pcm_samples"][0] for blk in blocks) == int(n_out[0])


# ------------------------------------------------------------------------------------- 9. refusals through the C entry
def test_refusals_leave_guard_filled_outputs_untouched(noise):
    fmt = SpectrogramFormat()
    lib = L.lib()
    ARG, SHAPE, DTYPE = -1, -2, -3
    x = noise[:2, :, :2000].contiguous().to(DEV)
    H = fmt.plan.history()
    out = torch.full((2, 3, 128), -77.0, device=DEV)
    carry = torch.full((2, 2, H), -77.0, device=DEV)
    rec = torch.tensor([[0, 2000, 0, 2, -1]] * 2, dtype=torch.int64, device=DEV)
    win, tw, bins, weights = tables(fmt)
    base = dict(x=L.ptr(x), B=2, in_stride=2000, rec=L.ptr(rec), carry_in=L.ptr(carry[0]), carry_out=L.ptr(carry[1]), H=H, n_fft=2048, hop=512,
                window=L.ptr(win), tw=L.ptr(tw), bins=L.ptr(bins), weights=L.ptr(weights), total=weights.numel(), F=128, scale=1, amin=1e-10,
                out=L.ptr(out), out_stride=3)

    def call(**kw):
        a = dict(base, **kw)
        return lib.vaura_spectrogram(a["x"], a["B"], a["in_stride"], a["rec"], a["carry_in"], a["carry_out"], a["H"], a["n_fft"], a["hop"],
                                     a["window"], a["tw"], a["bins"], a["weights"], a["total"], a["F"], a["scale"], a["amin"], a["out"],
                                     a["out_stride"], L.current_stream(torch.device(DEV)))
    cases = [(ARG, dict(x=0)), (ARG, dict(rec=0)), (ARG, dict(window=0)), (ARG, dict(tw=0)), (ARG, dict(out=0)), (ARG, dict(carry_in=0)),
             (ARG, dict(bins=0)), (ARG, dict(weights=0)), (ARG, dict(x=L.ptr(x) + 2)), (ARG, dict(rec=L.ptr(rec) + 4)), (ARG, dict(out=L.ptr(out) + 2)),
             (ARG, dict(carry_out=L.ptr(carry[0]))), (ARG, dict(carry_out=L.ptr(carry[0]) + 4 * H)), (ARG, dict(B=0)), (ARG, dict(in_stride=0)),
             (ARG, dict(amin=0.0)), (DTYPE, dict(scale=4)), (DTYPE, dict(scale=-1)), (ARG, dict(scale=3)), (SHAPE, dict(n_fft=4096)), (SHAPE, dict(n_fft=256)),
             (SHAPE, dict(hop=384)), (SHAPE, dict(hop=4096)), (SHAPE, dict(F=257)), (SHAPE, dict(F=0)), (SHAPE, dict(total=127)),
             (SHAPE, dict(total=128 * 1025 + 1)), (SHAPE, dict(bins=0, weights=0, F=128)), (SHAPE, dict(B=65536)), (SHAPE, dict(in_stride=2 ** 31))]
    for code, kw in cases:
        assert call(**kw) == code, kw
    torch.cuda.synchronize()
    assert bool((out == -77.0).all()) and bool((carry == -77.0).all())     # no refused call launched anything
    assert call() == 0                                                     # and the same arguments, unaltered, run
    torch.cuda.synchronize()
    assert bool((out[:, :2] != -77.0).all()) and bool((out[:, 2] == 0).all()) and bool((carry[0] == -77.0).all())
    assert torch.equal(carry[1], torch.cat([carry[0], x[:, 0]], dim=1)[:, -H:])
