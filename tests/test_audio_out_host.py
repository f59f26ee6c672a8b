"""Audio output without a GPU: the stream arithmetic of vaura_amd/audio_out.py against brute-force scans, a pure-torch fp32 simulation
of PcmStream (carry, release rule, flush) against the one-pass fp32 statement, the float64 restatement against a direct sum, every
refusal of vaura_audio_output and PcmFormat, and the dict bookkeeping of stream_pcm on fake blocks."""
import pytest
import torch

import audio_out_reference as RO
import audio_pre_reference as R
from vaura_amd import _lib as L
from vaura_amd import audio_out as AO
from vaura_amd import post
from vaura_amd.audio_preprocess import resample_table

SRC = 44100
RATES = [48000, 96000, 32000, 24000, 22050, 16000, 12000]


# ------------------------------------------------------------------------------------- stream arithmetic
def brute(rate):
    """start / last of every output of a few periods, straight from the table"""
    tab = resample_table(SRC, rate)
    o, n, w, T = tab["o"], tab["n"], tab["w"], tab["taps"]
    first = tab["first"].tolist()
    periods = 2 * ((2 * w + o) // o + 2) + 6
    start = [(m // n) * o + first[m % n] - w for m in range(periods * n)]
    return o, n, T, start, [s + T - 1 for s in start], periods


@pytest.mark.parametrize("rate", RATES)
def test_releasable_and_history_against_a_brute_force_scan(rate):
    pl = AO.plan(rate)
    o, n, T, start, last, periods = brute(rate)
    assert (pl.o, pl.n, pl.T) == (o, n, T)
    assert [pl.start(m) for m in range(0, len(start), 7)] == start[::7] and pl.last(5) == last[5]
    safe = (periods - 3) * o                                              # every output that matters below `safe` lies inside the scan
    worst = 0
    for r in range(0, safe):
        M = 0
        while last[M] < r:                                                # the prefix rule itself
            M += 1
        assert pl.releasable(r) == M, (rate, r)
        assert M <= pl.output_total(r)                                    # a stream never releases more than the clip will have
        if r >= 3 * o:                                                    # away from the start, where negative indices read zeros
            worst = max(worst, r - min(start[M:M + 2 * n]))
        assert min(start[M:M + 2 * n]) >= r - pl.history(), (rate, r)     # nothing unreleased reads below the carry
    assert pl.history() == worst                                          # and no smaller carry would do
    assert AO.releasable(1000, rate) == pl.releasable(1000) and AO.history(rate) == pl.history()
    assert AO.output_total(1001, rate) == -((-n * 1001) // o)


def test_history_of_48_khz_and_the_identity():
    pl = AO.plan(48000)
    # 13 taps per phase upwards (the 14 of 48 kHz -> 44.1 kHz are the other direction's); the first output held back is the one whose
    # last tap is the first sample still missing, so the carry holds the T - 1 before it
    assert (pl.o, pl.n, pl.T) == (147, 160, 13) and pl.history() == 12
    one = AO.plan(SRC)
    assert one.identity and one.history() == 0 and one.releasable(77) == 77 and one.output_total(77) == 77 and one.releasable(0) == 0
    big = 3 * 2 ** 31 + 12345                                             # a stream may pass 2^31 samples: Python integers all the way
    M = pl.releasable(big)
    assert pl.last(M - 1) < big <= pl.last(M) and pl.start(M) >= big - pl.history()


# ------------------------------------------------------------------------------------- the stream, simulated
class SimStream:
    """PcmStream in torch on the CPU for one clip: the records of audio_out.push_records, the kernel's sample rule (0 outside the
    clip, the carry below r0, the block above) and its carry update.  A read the launch must not make raises."""

    def __init__(self, rate, gain=1.0):
        self.pl = AO.plan(rate)
        self.tab, self.gain = resample_table(SRC, rate), gain
        self.H = self.pl.history()
        self.carry = torch.zeros(self.H)
        self.received, self.emitted = [0], [0]

    def push(self, block, final=False):
        recs, self.received, self.emitted = AO.push_records(self.pl, self.received, self.emitted, [block.shape[0]], [final])
        r0, L_, m0, count, N = recs[0]
        H, carry = self.H, self.carry

        def sample(s):
            zero = (s < 0) | ((s >= N) if N >= 0 else torch.zeros_like(s, dtype=torch.bool))
            in_carry = ~zero & (s < r0)
            in_block = ~zero & (s >= r0)
            assert bool((s[in_carry] >= r0 - H).all()), "a read below the carry"
            assert bool((s[in_block] < r0 + L_).all()), "a read behind the block"
            out = torch.zeros(s.shape[0])
            out[in_carry] = carry[s[in_carry] - (r0 - H)]
            out[in_block] = block[s[in_block] - r0]
            return out
        pcm = RO.form_f32(torch.arange(m0, m0 + count), sample, self.tab, self.gain)
        self.carry = torch.cat([carry, block])[-H:] if H else carry
        return pcm


def plans(N, H):
    g = torch.Generator().manual_seed(7)
    ragged = []
    while sum(ragged) < N:
        ragged.append(int(torch.randint(0, 3 * H, (1,), generator=g)) if len(ragged) % 3 else 0)     # every third push brings nothing
    return {"1": [1] * N, "3": [3] * (N // 3 + 1), "H-1": [H - 1] * (N // (H - 1) + 1), "H": [H] * (N // H + 1), "512": [512] * (N // 512 + 1),
            "ragged with zeros": ragged}


@pytest.mark.parametrize("rate", [48000, 16000, 96000])
def test_simulated_stream_is_the_one_pass_result(rate):
    N = 1100
    x = torch.randn(N, generator=torch.Generator().manual_seed(rate)) * 0.3
    tab = resample_table(SRC, rate)
    want = RO.one_pass_f32(x, tab, gain=0.7)
    assert want.shape[0] == AO.output_total(N, rate)
    for name, sizes in plans(N, AO.history(rate)).items():
        sim, got, at = SimStream(rate, gain=0.7), [], 0
        for size in sizes:
            blk = x[at:at + size]
            at += blk.shape[0]
            got.append(sim.push(blk))
        assert at == N
        held = want.shape[0] - sum(g.shape[0] for g in got)
        assert 0 < held <= tab["n"] * (tab["taps"] // tab["o"] + 2)       # the tail waits for its right-hand neighbours
        got.append(sim.push(x[:0], final=True))                           # the flush brings no samples of its own
        assert torch.equal(torch.cat(got), want), (rate, name)
    sim = SimStream(rate, gain=0.7)
    assert torch.equal(sim.push(x, final=True), want)                     # one single push


def test_one_pass_f32_meets_the_bar_of_the_float64_restatement():
    x = torch.randn(2, 1, 900, generator=torch.Generator().manual_seed(3)) * 0.5
    for rate in (48000, 24000, 16000):
        tab = resample_table(SRC, rate)
        y, n_out, bar = RO.restate(x, rate, lengths=[900, 317], gain=[0.5, -1.25], taps_per_phase=tab["taps"])
        for b, (nb, g) in enumerate([(900, 0.5), (317, -1.25)]):
            got = RO.one_pass_f32(x[b, 0, :nb], tab, gain=g)
            assert got.shape[0] == n_out[b]
            assert bool(((got.double() - y[b, :n_out[b]]).abs() <= bar[b, :n_out[b]]).all()), (rate, b)
            assert bool((y[b, n_out[b]:] == 0).all())


def test_quantisation_in_double():
    y = torch.tensor([0.0, 1.0, -1.0, 1.0 - 2.0 ** -15, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, float("inf"), float("-inf"),
                      float("nan"), 32767.4 / 32768], dtype=torch.float64)
    q, c = RO.quantise(y, torch.int16)
    assert q.tolist() == [0, 32767, -32768, 32767, 0, 2, 2, 0, 32767, -32768, 0, 32767]
    assert c.tolist() == [False, True, False, False, False, False, False, False, True, True, True, True]
    q, c = RO.quantise(y, torch.int32)
    assert q[1] == 2 ** 31 - 1 and q[2] == -2 ** 31 and q[10] == 0 and c.tolist()[:3] == [False, True, False]
    q, c = RO.quantise(torch.tensor([1.0, 1.0000001, -1.0, float("nan")]), torch.float32)
    assert c.tolist() == [False, True, False, True] and q[1] == torch.tensor(1.0000001)


# ------------------------------------------------------------------------------------- refusals
def test_tile_and_limits_are_the_library_s():
    lib = L.lib()
    assert lib.vaura_audio_output_tile() == AO.TILE
    pl = AO.plan(48000)
    need = lib.vaura_audio_output_lds_bytes(pl.o, pl.n, pl.w, pl.T)
    assert 4 * (AO.TILE * pl.o // pl.n) < need < 64 * 1024
    assert lib.vaura_audio_output_lds_bytes(0, 1, 1, 1) == 0


def test_span_of_a_tile_holds_every_tap_run():
    """The staged span starts at floor(mt o / n) - w for a tile whose first output is mt — any mt in a stream, not a multiple of the
    tile: every run of the tile's outputs must lie inside it (the kernel clamps, which would move a run silently)."""
    lib = L.lib()
    for rate in RATES:
        pl = AO.plan(rate)
        span = lib.vaura_audio_output_lds_bytes(pl.o, pl.n, pl.w, pl.T) // 4 - 4
        for mt in list(range(0, 2 * pl.n)) + [10 ** 12 + 7, 2 ** 40 + 3]:
            lo = (mt * pl.o) // pl.n - pl.w
            for m in list(range(mt, mt + pl.n + 1)) + list(range(mt + AO.TILE - pl.n - 1, mt + AO.TILE)):
                assert 0 <= pl.start(m) - lo <= span - pl.T, (rate, mt, m)


def test_entry_point_refuses_before_any_device_work():
    lib = L.lib()
    ARG, SHAPE, DTYPE = -1, -2, -3
    p = 4096                                                               # a non-null address that is never dereferenced: every call is refused

    def call(x=p, B=1, in_stride=1000, rec=p, carry_in=p, carry_out=p + 4096, H=14, o=147, n=160, w=7, first=p, taps=p, phases=160, T=14,
             gain=p, fmt=0, inter=1, C=2, out=p, out_stride=1089, clipped=p):
        return lib.vaura_audio_output(x, B, in_stride, rec, carry_in, carry_out, H, o, n, w, first, taps, phases, T, gain, fmt, inter, C, out,
                                      out_stride, clipped, 0)
    assert call(x=0) == ARG and call(rec=0) == ARG and call(gain=0) == ARG and call(clipped=0) == ARG and call(out=0) == ARG
    assert call(carry_in=0) == ARG and call(first=0) == ARG and call(taps=0) == ARG
    assert call(carry_out=p, H=0, carry_in=0) == ARG                       # a carry to write needs a history
    assert call(carry_out=p) == ARG and call(carry_out=p + 52) == ARG and call(carry_in=p + 4096 + 52) == ARG   # the pair overlaps (B x 14 x 4 bytes)
    assert call(carry_out=p + 4 * 14 * 2, B=3) == ARG                      # three clips: 168 bytes each way
    assert call(B=0) == ARG and call(phases=159) == ARG and call(rec=p + 4) == ARG
    assert call(in_stride=-1) == ARG and call(out_stride=-1) == ARG and call(H=-1) == ARG and call(in_stride=0) == ARG
    assert call(C=0) == SHAPE and call(C=9) == SHAPE
    assert call(fmt=3) == DTYPE and call(fmt=-1) == DTYPE
    assert call(T=65) == SHAPE
    assert call(n=44100, phases=44100, T=27, o=96001) == SHAPE             # more than 2^20 entries
    assert call(in_stride=2 ** 31) == SHAPE and call(out_stride=2 ** 31) == SHAPE
    assert call(o=64000, n=1, phases=1, T=64, w=32) == SHAPE               # the span of one tile does not fit the LDS
    assert call(B=65536) == SHAPE


def test_pcm_format_refusals():
    for rate in (8000, 4000, 6000):
        with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE.*taps per phase"):
            post.PcmFormat(rate=rate)
    with pytest.raises(L.VauraHipError, match="positive integer"):
        post.PcmFormat(rate=0)
    with pytest.raises(L.VauraHipError, match="positive integer"):
        post.PcmFormat(rate=48000.0)
    for dtype in (torch.uint8, torch.float64, torch.float16):
        with pytest.raises(L.VauraHipError, match="VAURA_ERR_DTYPE"):
            post.PcmFormat(dtype=dtype)
    for channels in (0, 9, -1, 2.0, True):
        with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE.*channels"):
            post.PcmFormat(channels=channels)
    fmt = post.PcmFormat()
    assert (fmt.rate, fmt.dtype, fmt.channels, fmt.interleaved, fmt.gain) == (48000, torch.int16, 2, True, 1.0)
    assert post.PcmFormat(rate=SRC).plan.identity and post.PcmFormat(gain=[0.5, 2]).gains(2) == [0.5, 2.0]
    with pytest.raises(L.VauraHipError, match="gain has 2 values"):
        post.PcmFormat(gain=[0.5, 2]).gains(3)
    with pytest.raises(L.VauraHipError, match="no CPU path"):
        post.audio_to_pcm(torch.zeros(1, 1, 64), fmt)
    with pytest.raises(L.VauraHipError, match="mono waveform"):
        post.audio_to_pcm(torch.zeros(1, 2, 64), fmt)
    with pytest.raises(L.VauraHipError, match="lengths must lie in 1 .. 64"):
        post.audio_to_pcm(torch.zeros(2, 1, 64), fmt, lengths=[64, 65])


# ------------------------------------------------------------------------------------- stream_pcm on fake blocks
def fake_launch(log):
    def launch(fmt, x, in_stride, records, gain, carry_in, carry_out, n_row, ring=None):
        log.append((in_stride, [list(r) for r in records], n_row))
        out = torch.zeros(len(records), n_row, fmt.channels, dtype=fmt.dtype)
        out.clipped = torch.zeros(len(records), dtype=torch.int32)
        return out
    return launch


def test_stream_pcm_bookkeeping_on_fake_blocks(monkeypatch):
    log = []
    monkeypatch.setattr(post, "_pcm_launch", fake_launch(log))
    fmt, hop = post.PcmFormat(), 512
    pl = fmt.plan
    # the ragged key style: lists of start frames and frames, the audio left-aligned in rows of max(frames) * hop samples
    frames = [[4, 2], [3, 0], [0, 0], [2, 1]]
    blocks = [{"audio": torch.zeros(2, 1, max(f) * hop), "start_frames": [0, 0], "frames": f, "sampled_indices": i, "final": i == 3}
              for i, f in enumerate(frames)]
    out = list(post.stream_pcm(iter(blocks), fmt))
    assert len(out) == 4 and all(o["sampled_indices"] == i and o["frames"] == frames[i] for i, o in enumerate(out))
    assert all(set(o) == set(blocks[0]) | {"pcm", "pcm_start", "pcm_samples", "pcm_clipped"} for o in out) and "pcm" not in blocks[0]
    at, got = [0, 0], [0, 0]
    for i, o in enumerate(out):
        assert o["pcm_start"] == at and tuple(o["pcm"].shape) == (2, max(o["pcm_samples"]), 2)
        got = [g + f * hop for g, f in zip(got, frames[i])]
        at = [a + c for a, c in zip(at, o["pcm_samples"])]
        want = [pl.output_total(g) if i == 3 else pl.releasable(g) for g in got]
        assert at == want, i
        assert log[i][0] == max(max(frames[i]) * hop, 1) and [r[1] for r in log[i][1]] == [f * hop for f in frames[i]]
        assert [r[4] for r in log[i][1]] == (got if i == 3 else [-1, -1])
    assert at == [pl.output_total(9 * hop), pl.output_total(3 * hop)] and out[2]["pcm_samples"] == [0, 0]
    # the equal-length style: ints
    log.clear()
    blocks = [{"audio": torch.zeros(3, 1, n * hop), "start_frame": s, "frames": n, "final": fin} for s, n, fin in [(0, 16, False), (16, 27, True)]]
    out = list(post.stream_pcm(blocks, post.PcmFormat(rate=SRC, dtype=torch.float32, channels=1)))
    assert [o["pcm_start"] for o in out] == [[0] * 3, [16 * hop] * 3] and [o["pcm_samples"] for o in out] == [[16 * hop] * 3, [27 * hop] * 3]


def test_save_pcm_wavs_round_trip(tmp_path):
    from scipy.io import wavfile
    g = torch.Generator().manual_seed(2)
    cases = [(post.PcmFormat(), torch.randint(-32768, 32768, (2, 50, 2), generator=g).to(torch.int16)),
             (post.PcmFormat(rate=24000, dtype=torch.int32, channels=3, interleaved=False),
              torch.randint(-2 ** 31, 2 ** 31, (2, 3, 50), generator=g, dtype=torch.int64).to(torch.int32)),
             (post.PcmFormat(rate=SRC, dtype=torch.float32, channels=1), torch.rand(2, 50, 1, generator=g))]
    for i, (fmt, pcm) in enumerate(cases):
        paths = [str(tmp_path / f"{i}_{b}.wav") for b in range(2)]
        post.save_pcm_wavs(paths, pcm, torch.tensor([50, 17]), fmt)
        for b, n in enumerate([50, 17]):
            rate, data = wavfile.read(paths[b])
            want = (pcm[b] if fmt.interleaved else pcm[b].t())[:n]
            assert rate == fmt.rate and str(data.dtype) == str(fmt.dtype).replace("torch.", "")
            assert torch.equal(torch.from_numpy(data.copy()).reshape(n, fmt.channels), want), (i, b)
    with pytest.raises(L.VauraHipError, match="is not PcmFormat"):
        post.save_pcm_wavs(["a", "b"], cases[0][1], [50, 17], cases[2][0])
    with pytest.raises(L.VauraHipError, match="1 paths and 2 lengths"):
        post.save_pcm_wavs(["a"], cases[0][1], [50, 17], cases[0][0])


def test_pcm_stream_refusals(monkeypatch):
    monkeypatch.setattr(post, "_pcm_launch", fake_launch([]))
    s = post.PcmStream(post.PcmFormat(), 2, "cpu")
    with pytest.raises(L.VauraHipError, match="samples must lie in 0 .. 100"):
        s.push(torch.zeros(2, 1, 100), samples=[100, 101])
    with pytest.raises(L.VauraHipError, match="samples has 3 values"):
        s.push(torch.zeros(2, 1, 100), samples=[1, 2, 3])
    with pytest.raises(L.VauraHipError, match="block of shape"):
        s.push(torch.zeros(3, 1, 100))
    pcm, counts = s.push(torch.zeros(2, 1, 100), samples=[100, 0], final=[False, True])
    assert counts == [s.fmt.plan.releasable(100), 0] and s.finished == [False, True]
    with pytest.raises(L.VauraHipError, match="clip 1 .* takes no more samples"):
        s.push(torch.zeros(2, 1, 10))
    pcm, counts = s.push(None, final=True)
    assert counts == [s.fmt.plan.output_total(100) - s.fmt.plan.releasable(100), 0] and s.received == [100, 0]
    with pytest.raises(L.VauraHipError, match="at least one clip"):
        post.PcmStream(post.PcmFormat(), 0, "cpu")
