"""Audio output on the GPU: vaura_audio_output (csrc/audio_out.hip) through post.audio_to_pcm / PcmStream / stream_pcm.

  1. F32 output against the float64 restatement of tests/audio_out_reference.py under its derived bar (the largest |error| / bar of
     every case is printed; with VAURA_PARITY_DIR set they are kept in audio_out_parity.txt);
  2. S16 / S32 against the host quantisation, in double, of the F32 output of the same input — exact, planted edge values included;
  3. layouts: every channel of every layout is the mono result;
  4. edges: NaN behind every clip's length, a 0xFF-filled output between guards, clips independent of each other;
  5. streaming: the pushes of every block plan, concatenated per clip, are audio_to_pcm bit for bit, at any absolute position (the
     1-sample plan runs the full rows for 48 kHz int16 stereo and the first 400 samples of every clip for the other cases);
  6. end to end: stream_pcm(generate_stream(...)) is audio_to_pcm(generate(...)).

Shapes: rows of 2 900 samples — four tiles of 1 024 outputs at 48 kHz, two at 24 and 16 kHz (2 826 samples are the fewest that pass a tile
edge at 16 kHz) — and per-clip lengths 1, 3, one tile - 1, one tile + 1 (as output lengths) and the full row."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_out_reference as RO  # noqa: E402
import test_gpu_per_clip_sampling as G  # noqa: E402  (the tiny plugin model)
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import audio_out as AO  # noqa: E402
from vaura_amd import post, synth  # noqa: E402
from vaura_amd.post import PcmFormat, PcmStream, audio_to_pcm, stream_pcm  # noqa: E402

DEV = "cuda:0"
SRC = 44100
TILE = AO.TILE
N = 2900
GAINS = [1.0, 0.5, -1.25, 2.0, 0.75]

_ratios = {}


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    out = os.environ.get("VAURA_PARITY_DIR")
    if _ratios and out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "audio_out_parity.txt"), "w") as f:
            f.write("audio output (F32) against float64: largest |error| / bar per case, bar = (T + 5) 2^-24 |g| sum |k| |x| "
                    "(tests/test_gpu_audio_out.py)\n")
            for k in sorted(_ratios):
                f.write(f"{_ratios[k]:8.4f}  {k}\n")


def n_for(L_out, rate):
    """an input length whose output length is L_out, or the nearest one above"""
    pl = AO.plan(rate)
    nb = max(1, (L_out * pl.o) // pl.n)
    while pl.output_total(nb) < L_out:
        nb += 1
    return nb


def lengths_for(rate):
    return [1, 3, n_for(TILE - 1, rate), n_for(TILE + 1, rate), N]


@pytest.fixture(scope="module")
def noise():
    """(5, 1, N) fp32 on the host, computed once and left unchanged"""
    return torch.randn(5, 1, N, generator=torch.Generator().manual_seed(11)) * 0.3


def poison_behind(x, lengths):
    x = x.clone()
    for b, nb in enumerate(lengths):
        x[b, :, nb:] = float("nan")
    return x


def mono(pcm, fmt):
    """(B, N_out) of a one-channel result"""
    return pcm[:, :, 0] if fmt.interleaved else pcm[:, 0, :]


# ------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("rate", [48000, 24000, 16000, SRC])
def test_f32_output_against_float64(noise, rate):
    fmt = PcmFormat(rate=rate, dtype=torch.float32, channels=1, interleaved=False, gain=GAINS)
    lengths = lengths_for(rate)
    got, got_len = audio_to_pcm(poison_behind(noise, lengths).to(DEV), fmt, lengths=lengths)
    want, n_out, bar = RO.restate(noise, rate, lengths, GAINS, taps_per_phase=fmt.plan.T)
    assert got.dtype == torch.float32 and got.device.type == "cuda" and got_len.tolist() == n_out and tuple(got.shape) == (5, 1, max(n_out))
    if rate != SRC:
        assert n_out[2] in (TILE - 1, TILE) and n_out[3] in (TILE + 1, TILE + 2) and n_out[4] > n_out[3]   # both sides of a tile edge
    g = mono(got, fmt).cpu()
    assert bool(torch.isfinite(g).all())
    ratio = float(((g.double() - want).abs() / bar.clamp(min=1e-300)).max())
    case = f"44100 -> {rate} Hz, F32, gains {GAINS}"
    _ratios[case] = ratio
    print(f"{case}: largest |error| / bar {ratio:.4f}")
    assert ratio <= 1.0
    for b, n in enumerate(n_out):
        assert bool((g[b, n:] == 0).all()), b
    assert got.clipped.tolist() == [int((g[b, :n].abs() > 1).sum()) for b, n in enumerate(n_out)]         # counted on the fp32 values


# ------------------------------------------------------------------------------------- 2. integer formats
def planted(noise):
    """the noise with edge values every 37 samples: +-1, just beyond, exact half-LSB ties of both integer formats, +-inf, NaN"""
    x = noise.clone()
    one_up = float(torch.nextafter(torch.tensor(1.0), torch.tensor(2.0)))
    vals = [1.0, -1.0, one_up, -one_up, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, 32766.5 / 32768, 32767.5 / 32768,
            -32767.5 / 32768, 32767.4 / 32768, 0.5 / 2 ** 31, 1.5 / 2 ** 31, -2.5 / 2 ** 31, (2 ** 24 - 1.0) / 2 ** 24, (2 ** 23 + 0.5) / 2 ** 31,
            float("inf"), float("-inf"), float("nan"), 1.0 - 2.0 ** -15, 3.0, -3.0]
    for b in range(x.shape[0]):
        for i, v in enumerate(vals * 2):
            x[b, 0, 5 + 37 * i + b] = v
    return x


@pytest.mark.parametrize("rate", [SRC, 48000])
@pytest.mark.parametrize("dtype", [torch.int16, torch.int32])
def test_integer_formats_are_the_quantised_f32_output(noise, rate, dtype):
    x = planted(noise).to(DEV)
    lengths = [N, N - 1, 1500, 40, 6]
    gains = [1.0, 1.0, -1.0, 0.5, 2.0]                                    # powers of two: the planted values arrive as planted at 44.1 kHz
    f32, n_out = audio_to_pcm(x, PcmFormat(rate=rate, dtype=torch.float32, channels=1, gain=gains), lengths=lengths)
    got, got_len = audio_to_pcm(x, PcmFormat(rate=rate, dtype=dtype, channels=1, gain=gains), lengths=lengths)
    assert got.dtype == dtype and got_len.tolist() == n_out.tolist()
    y = f32.cpu()[:, :, 0]
    want, clipped = RO.quantise(y, dtype)
    _, clipped_f32 = RO.quantise(y, torch.float32)
    for b, n in enumerate(n_out.tolist()):
        assert torch.equal(got.cpu()[b, :n, 0], want[b, :n]), b
        assert bool((got[b, n:] == 0).all())
        assert int(got.clipped[b]) == int(clipped[b, :n].sum()), b
        assert int(f32.clipped[b]) == int(clipped_f32[b, :n].sum()), b
    assert int(got.clipped[0]) >= 10 and bool(y[0].isnan().any()) and bool(y[0].isinf().any())
    if rate == SRC:                                                       # the identity: the planted values themselves were quantised
        assert torch.equal(y[0, :N].nan_to_num(7.0), x.cpu()[0, 0].nan_to_num(7.0))
        info = torch.iinfo(dtype)
        assert int(got[0].max()) == info.max and int(got[0].min()) == info.min


# ------------------------------------------------------------------------------------- 3. layouts
@pytest.mark.parametrize("interleaved", [True, False], ids=["interleaved", "planar"])
@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
def test_every_channel_is_the_mono_result(noise, dtype, channels, interleaved):
    lengths = lengths_for(48000)
    x = poison_behind(noise * 4, lengths).to(DEV)                         # loud: some samples clip
    one, n_one = audio_to_pcm(x, PcmFormat(dtype=dtype, channels=1, interleaved=False), lengths=lengths)
    got, n_out = audio_to_pcm(x, PcmFormat(dtype=dtype, channels=channels, interleaved=interleaved), lengths=lengths)
    n_row = max(n_out.tolist())
    assert tuple(got.shape) == ((5, n_row, channels) if interleaved else (5, channels, n_row)) and n_out.tolist() == n_one.tolist()
    planes = got.transpose(1, 2) if interleaved else got
    for c in range(channels):
        assert torch.equal(planes[:, c], one[:, 0]), c
    assert torch.equal(got.clipped, one.clipped) and int(one.clipped.sum()) > 0


# ------------------------------------------------------------------------------------- 4. edges
def raw_launch(fmt, x, records, out, out_stride, gains, carry_in=None, carry_out=None, clipped=None):
    pl = fmt.plan
    B = x.shape[0]
    first, taps = (None, None) if pl.identity else post._pcm_table(pl, torch.device(DEV))
    rec = torch.tensor(records, dtype=torch.int64, device=DEV)
    gain = torch.tensor(gains, dtype=torch.float32, device=DEV)
    clipped = torch.zeros(B, dtype=torch.int32, device=DEV) if clipped is None else clipped
    rc = L.lib().vaura_audio_output(L.ptr(x), B, x.shape[-1], L.ptr(rec), L.ptr(carry_in), L.ptr(carry_out),
                                    0 if carry_in is None else carry_in.shape[-1], pl.o, pl.n, pl.w, L.ptr(first), L.ptr(taps), pl.n, pl.T,
                                    L.ptr(gain), post._PCM_FORMATS[fmt.dtype], int(fmt.interleaved), fmt.channels, L.ptr(out), out_stride,
                                    L.ptr(clipped), L.current_stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, clipped


@pytest.mark.parametrize("rate,dtype,channels,interleaved", [(48000, torch.int16, 2, True), (16000, torch.float32, 3, False),
                                                             (SRC, torch.int32, 1, True)])
def test_edges_poisoned_input_and_guarded_output(noise, rate, dtype, channels, interleaved):
    fmt = PcmFormat(rate=rate, dtype=dtype, channels=channels, interleaved=interleaved)
    lengths = lengths_for(rate)
    n_out = [fmt.plan.output_total(n) for n in lengths]
    x = poison_behind(noise, lengths).to(DEV)
    want, _ = audio_to_pcm(noise.to(DEV), fmt, lengths=lengths)           # clean input, rows of its own
    stride, G_ = max(n_out) + 5, 4096                                     # rows longer than any clip's output
    esize = torch.empty(0, dtype=dtype).element_size()
    raw = torch.full(((2 * G_ + 5 * channels * stride) * esize,), 0xFF, dtype=torch.uint8, device=DEV)
    out = raw[G_ * esize:(G_ + 5 * channels * stride) * esize].view(dtype)
    records = [[0, n, 0, m, n] for n, m in zip(lengths, n_out)]
    rc, clipped = raw_launch(fmt, x, records, out, stride, [1.0] * 5)
    assert rc == 0
    assert bool((raw[:G_ * esize] == 0xFF).all()) and bool((raw[(G_ + 5 * channels * stride) * esize:] == 0xFF).all())   # nothing outside the rows
    got = out.view(5, stride, channels) if interleaved else out.view(5, channels, stride)
    frames = got if interleaved else got.transpose(1, 2)
    want_frames = want if interleaved else want.transpose(1, 2)
    for b, n in enumerate(n_out):
        assert torch.equal(frames[b, :n], want_frames[b, :n]), b          # NaN behind a clip's length never reaches it
        assert bool((frames[b, n:] == 0).all()), b                        # exactly 0 from the clip's length to the row's end
    assert torch.equal(clipped, want.clipped)


def test_clips_of_a_batch_are_independent(noise):
    fmt = PcmFormat()
    lengths = lengths_for(48000)
    x = noise.to(DEV)
    got, n_out = audio_to_pcm(x, fmt, lengths=lengths)
    other = x.clone()
    other[1] = float("nan")
    other[3] = float("nan")
    changed, _ = audio_to_pcm(other, fmt, lengths=lengths)
    for b in (0, 2, 4):
        assert torch.equal(changed[b], got[b]) and int(changed.clipped[b]) == int(got.clipped[b])
    assert int(changed.clipped[1]) == n_out[1] and int(changed.clipped[3]) == n_out[3]
    for b, nb in enumerate(lengths):                                      # each clip is the clip converted alone at its own length
        alone, alone_len = audio_to_pcm(x[b:b + 1, :, :nb].contiguous(), fmt)
        assert alone_len.tolist() == [int(n_out[b])] and torch.equal(got[b, :alone.shape[1]], alone[0])


# ------------------------------------------------------------------------------------- 5. streaming
def block_plans(lengths, H):
    g = torch.Generator().manual_seed(5)
    ragged, left = [], list(lengths)
    while any(left):
        if len(ragged) == 2:
            step = [0] * len(left)                                        # a push in which no clip brings a sample
        else:
            step = [min(n, int(torch.randint(0, 900, (1,), generator=g))) if (len(ragged) + b) % 4 else 0 for b, n in enumerate(left)]
        ragged.append(step)
        left = [n - s for n, s in zip(left, step)]
    plans = {"ragged per clip with zero-sample pushes": ragged, "one single push": [list(lengths)]}
    for size in (3, H - 1, 512, 8192):
        left, steps = list(lengths), []
        while any(left):
            step = [min(n, size) for n in left]
            steps.append(step)
            left = [n - s for n, s in zip(left, step)]
        plans[f"{size} samples"] = steps
    return plans


def run_stream(fmt, x, steps):
    """push the plan, the last block of every clip as its final one -> (per-clip concatenation, clipped sums, launches)"""
    B = x.shape[0]
    host = x.cpu()
    stream = PcmStream(fmt, B, DEV)
    at, left = [0] * B, [sum(s[b] for s in steps) for b in range(B)]
    pushed, clipped = [], torch.zeros(B, dtype=torch.int32, device=DEV)
    for step in steps:
        blk = torch.full((B, 1, max(max(step), 1)), float("nan"))         # what a block holds behind a clip's samples is never read
        for b in range(B):
            blk[b, 0, :step[b]] = host[b, 0, at[b]:at[b] + step[b]]
            at[b] += step[b]
            left[b] -= step[b]
        start = list(stream.emitted)
        pcm, counts = stream.push(blk.to(DEV), samples=step, final=[n == 0 for n in left])
        assert [s + c for s, c in zip(start, counts)] == stream.emitted and pcm.shape[1] == max(counts)
        pushed.append((pcm, counts))
        clipped += pcm.clipped
    parts = [[] for _ in range(B)]
    for pcm, counts in pushed:                                            # interleaved (B, n, C): frames first
        behind = torch.arange(pcm.shape[1], device=DEV)[None, :] >= torch.tensor(counts, device=DEV)[:, None]
        assert not bool((pcm != 0)[behind].any())                         # zeros behind every clip's count
        for b in range(B):
            parts[b].append(pcm[b, :counts[b]])
    return [torch.cat(p) for p in parts], clipped


@pytest.mark.parametrize("rate", [48000, 16000])
@pytest.mark.parametrize("dtype,channels", [(torch.int16, 2), (torch.float32, 1)], ids=["s16_stereo", "f32_mono"])
def test_pushes_concatenated_are_the_one_pass_result(noise, rate, dtype, channels):
    fmt = PcmFormat(rate=rate, dtype=dtype, channels=channels, interleaved=True, gain=[1.0, 0.5, -1.25, 4.0, 3.0])
    lengths = lengths_for(rate)
    x = noise.to(DEV)
    want, n_out = audio_to_pcm(poison_behind(noise, lengths).to(DEV), fmt, lengths=lengths)
    assert int(want.clipped.sum()) > 0
    for name, steps in block_plans(lengths, fmt.plan.history()).items():
        got, clipped = run_stream(fmt, x, steps)
        for b, n in enumerate(n_out.tolist()):
            assert got[b].shape[0] == n and torch.equal(got[b], want[b, :n]), (name, b)
        assert torch.equal(clipped, want.clipped), name
    # one sample at a time: the full rows at 48 kHz int16 stereo (2 900 pushes: every tile edge, every clip's tail); the other three
    # cases take the first 400 samples of every clip only — the carry logic is the same, the run time is not
    cut = N if (rate, dtype) == (48000, torch.int16) else 400
    short = [min(n, cut) for n in lengths]
    want, n_out = audio_to_pcm(x[..., :cut].contiguous(), fmt, lengths=short)
    steps = [[1 if i < n else 0 for n in short] for i in range(cut)]
    got, clipped = run_stream(fmt, x, steps)
    for b, n in enumerate(n_out.tolist()):
        assert torch.equal(got[b], want[b, :n]), ("1 sample", b)
    assert torch.equal(clipped, want.clipped)


def test_identity_rate_streams_without_a_carry(noise):
    fmt = PcmFormat(rate=SRC, dtype=torch.int32, channels=2)
    x = noise.to(DEV)
    want, n_out = audio_to_pcm(x, fmt)
    steps = [[700] * 5, [0] * 5, [N - 700] * 5]
    got, clipped = run_stream(fmt, x, steps)
    assert all(torch.equal(got[b], want[b]) for b in range(5)) and torch.equal(clipped, want.clipped)


def test_a_block_far_into_a_stream_is_the_block_at_its_start(noise):
    """64-bit positions: the same carry and block 2^25 periods later (input index 4.9e9, output index 5.4e9) give the same bits."""
    fmt = PcmFormat(dtype=torch.float32, channels=1)
    pl = fmt.plan
    H = pl.history()
    x = noise[:2, :, :1500].contiguous().to(DEV)
    carry = noise[:2, 0, 2000:2000 + H].contiguous().to(DEV)
    outs = []
    for K in (3, 3 + 2 ** 25):
        r0 = K * pl.o + 11
        m0, m1 = pl.releasable(r0), pl.releasable(r0 + 1500)
        assert m1 - m0 > TILE
        out = torch.empty(2, m1 - m0, 1, dtype=torch.float32, device=DEV)
        nxt = torch.zeros(2, H, device=DEV)
        rc, _ = raw_launch(fmt, x, [[r0, 1500, m0, m1 - m0, -1]] * 2, out, m1 - m0, [1.0, 1.0], carry, nxt)
        assert rc == 0 and torch.equal(nxt, x[:, 0, -H:])
        outs.append(out)
    assert r0 > 2 ** 32 and m0 > 2 ** 32 and torch.equal(outs[0], outs[1]) and bool((outs[0] != 0).any())


# ------------------------------------------------------------------------------------- 6. end to end
@pytest.fixture(scope="module")
def model(tiny_sampler_sd):
    return G._model(tiny_sampler_sd)


def frames_of(B, seed=31):
    return synth.video_features(B, tokens=32, seed=seed).reshape(B, 1, 32, 768).to(DEV)


def check_end_to_end(model, fmt, B, T, **kw):
    hop = synth.FULL_CODEC.hop
    frames = frames_of(B)
    ref = model.generate(frames=frames, max_new_tokens=T, prompt_is_encoded=True, use_sampling=False, cfg_scale=1.0, **kw)
    lengths = [t * hop for t in T] if isinstance(T, list) else None
    want, n_out = audio_to_pcm(ref["generated_audio"], fmt, lengths=lengths)
    blocks = list(stream_pcm(model.generate_stream(frames=frames, max_new_tokens=T, prompt_is_encoded=True, block_frames=7, use_sampling=False,
                                                   cfg_scale=1.0, **kw), fmt))
    assert len(blocks) > 2 and [b["final"] for b in blocks] == [False] * (len(blocks) - 1) + [True]
    at = [0] * B
    for blk in blocks:
        assert blk["pcm_start"] == at and "audio" in blk
        for b in range(B):
            n = blk["pcm_samples"][b]
            assert torch.equal(blk["pcm"][b, :n], want[b, at[b]:at[b] + n]), b
            at[b] += n
    assert at == n_out.tolist()
    assert torch.equal(sum(b["pcm_clipped"] for b in blocks), want.clipped)


def test_stream_pcm_of_generate_stream_is_audio_to_pcm_of_generate(model):
    check_end_to_end(model, PcmFormat(gain=8.0), 2, 43)


def test_stream_pcm_with_per_clip_lengths(model):
    check_end_to_end(model, PcmFormat(rate=16000, dtype=torch.float32, channels=1), 4, [43, 23, 9, 1], video_lengths=[32, 20, 9, 1])
