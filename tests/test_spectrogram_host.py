"""Host side of the spectrogram (vaura_amd/spectrogram.py, vaura_amd/post.py) without a device: the plan arithmetic against brute force,
the three tables against float64 and known answers, the reference's own claims (tests/spectrogram_reference.py), every call-time
refusal, the C entry's refusals on addresses that are never dereferenced, and stream_spectrogram's bookkeeping on a stubbed launch."""
import math
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrogram_reference as RS  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import post  # noqa: E402
from vaura_amd import spectrogram as SG  # noqa: E402

SIZES = [(2048, 512), (512, 128), (1024, 512)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("n_fft,hop", SIZES + [(512, 512), (1024, 1)])
def test_plan_against_brute_force(n_fft, hop):
    pl = SG.SpectrogramPlan(n_fft, hop)
    last = lambda t: hop * t + hop // 2 - n_fft // 2 + n_fft - 1       # noqa: E731  the last sample of column t's window
    assert pl.history() <= n_fft
    worst = 0
    for r in list(range(0, 3 * n_fft + 3 * hop + 2)) + [10 ** 10 + 77]:
        assert pl.columns(r) == sum(1 for t in range(r // hop + 2) if hop * t < r) if r < 10 ** 6 else pl.columns(r) == math.ceil(r / hop)
        t = pl.releasable(r)
        assert (t == 0 or last(t - 1) < r) and last(t) >= r              # the count of complete windows, exactly
        worst = max(worst, r - pl.lo(t))                                 # what the first unreleased column reaches back for
        assert r - pl.lo(t) <= pl.history() or pl.lo(t) < 0 and r <= pl.history()
    assert worst == pl.history() == n_fft - 1                            # exact: nothing more is carried than is needed
    assert pl.lo(0) == hop // 2 - n_fft // 2 and pl.columns(0) == 0 and pl.releasable(0) == 0


@pytest.mark.parametrize("n_fft,hop", SIZES)
def test_push_records_tile_the_columns_and_stay_inside_carry_and_block(n_fft, hop):
    pl = SG.SpectrogramPlan(n_fft, hop)
    H = pl.history()
    rnd = random.Random(n_fft + hop)
    for trial in range(30):
        total = rnd.choice([1, hop - 1, hop, 3 * hop + 7, 5 * n_fft + 3])
        received, emitted, left, seen = [0], [0], total, []
        while True:
            step = min(left, rnd.choice([0, 1, 3, hop - 1, hop, hop + 1, n_fft, 3 * n_fft]))
            left -= step
            fin = left == 0 and rnd.random() < 0.7
            recs, received, emitted = SG.push_records(pl, received, emitted, [step], [fin])
            r0, Lb, t0, count, N = recs[0]
            assert (N == r0 + Lb) if fin else N == -1
            for t in range(t0, t0 + count):
                seen.append(t)
                for s in (pl.lo(t), pl.lo(t) + n_fft - 1):               # both ends of the window: served by carry ++ block, or zero by rule
                    inside = r0 - H <= s < r0 + Lb
                    assert inside or s < 0 or (fin and s >= N), (t, s, recs)
            if fin:
                break
        assert seen == list(range(pl.columns(total)))                    # every column once, in order
        more, _, e2 = SG.push_records(pl, received, emitted, [0], [True])
        assert more[0][3] == 0 and e2 == emitted


def test_plan_refusals():
    for n_fft in (256, 4096, 1000, 2048.0, True):
        with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE.*n_fft"):
            SG.SpectrogramPlan(n_fft, 128)
    for hop in (0, 3, 1000, 4096, 512.0, -512):
        with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE.*hop"):
            SG.SpectrogramPlan(2048, hop)
    with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE.*hop"):
        SG.SpectrogramPlan(512, 1024)


# ------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_window_is_torch_s_periodic_hann_bit_for_bit(n_fft):
    from scipy.signal import get_window
    w = SG.window(n_fft)
    assert w.dtype == torch.float32 and torch.equal(w, torch.hann_window(n_fft, periodic=True, dtype=torch.float64).float())
    sc = torch.from_numpy(get_window("hann", n_fft, fftbins=True))
    assert float((w.double() - sc).abs().max()) <= 2.0 ** -24           # the float64 values differ by rounding in their last place only
    assert w[0] == 0 and w[n_fft // 2] == 1


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_twiddles_against_float64(n_fft):
    tw = SG.twiddles(n_fft)
    assert tw.dtype == torch.float32 and tuple(tw.shape) == (3 * n_fft // 4, 2)
    t = torch.arange(3 * n_fft // 4, dtype=torch.float64)
    want = torch.stack([torch.cos(2 * math.pi * t / n_fft), -torch.sin(2 * math.pi * t / n_fft)], dim=1)
    assert float((tw.double() - want).abs().max()) <= 2.0 ** -25        # one rounding of a value of at most 1
    assert tw[0].tolist() == [1.0, 0.0] and tw[n_fft // 4].tolist() == [0.0, -1.0] and tw[n_fft // 2].tolist() == [-1.0, 0.0]


def test_mel_scale_known_answers():
    assert RS.hz_to_mel(1000.0, "slaney") == 15.0 and float(SG.hz_to_mel(1000.0, "slaney")) == 15.0
    assert RS.hz_to_mel(500.0, "slaney") == 7.5 and float(SG.hz_to_mel(500.0)) == 7.5             # linear below
    assert abs(float(SG.hz_to_mel(6400.0)) - 42.0) < 1e-12                                         # 27 steps per factor 6.4
    assert abs(float(SG.hz_to_mel(1000.0, "htk")) - 2595 * math.log10(1 + 1000 / 700)) < 1e-12
    for scale in ("slaney", "htk"):
        for f in (0.0, 100.0, 999.0, 1000.0, 4000.0, 22050.0):
            assert abs(float(SG.mel_to_hz(SG.hz_to_mel(f, scale), scale)) - f) < 1e-8
            assert abs(RS.mel_to_hz(RS.hz_to_mel(f, scale), scale) - f) < 1e-8


@pytest.mark.parametrize("n_fft,n_mels,scale,norm,f_min,f_max", [(2048, 128, "slaney", None, 0.0, None), (2048, 64, "htk", "slaney", 0.0, None),
                                                                 (2048, 128, "htk", None, 50.0, 16000.0), (1024, 128, "slaney", "slaney", 0.0, None),
                                                                 (512, 64, "slaney", None, 0.0, None)])
def test_mel_table_against_the_restatement_and_its_structure(n_fft, n_mels, scale, norm, f_min, f_max):
    want, pts = RS.mel_filters(n_fft, n_mels, f_min, f_max, scale, norm)
    dense = SG.mel_filters(n_fft, n_mels, f_min, f_max, scale, norm)
    assert float((torch.from_numpy(dense) - want).abs().max()) <= 1e-12 * float(want.max())
    table = SG.mel_table(n_fft, n_mels, f_min, f_max, scale, norm)
    bins, weights = table["bins"], table["weights"]
    assert bins.dtype == torch.int32 and tuple(bins.shape) == (n_mels, 3) and weights.dtype == torch.float32
    back = SG.expand(table, n_fft // 2 + 1)                              # the compact table round-trips to the dense matrix
    assert torch.equal(back, torch.from_numpy(dense.astype(np.float32)))
    assert bins[:, 2].tolist() == [0] + torch.cumsum(bins[:, 1], 0)[:-1].tolist() and int(bins[:, 1].sum()) == weights.numel()
    assert int(bins[:, 0].min()) >= 0 and int((bins[:, 0] + bins[:, 1]).max()) <= n_fft // 2 + 1 and int(bins[:, 1].min()) >= 1
    if norm is None:                                                     # the triangles sum to 1 between the first and the last centre
        f = torch.arange(n_fft // 2 + 1, dtype=torch.float64) * RS.SR / n_fft
        mid = (f >= pts[1]) & (f <= pts[-2])
        assert bool(mid.any()) and float((want.sum(dim=0)[mid] - 1).abs().max()) < 1e-9
    else:                                                                # unit area in Hz
        width = torch.tensor([pts[m + 2] - pts[m] for m in range(n_mels)], dtype=torch.float64)
        assert float((want.max(dim=1).values * width / 2).max()) <= 1 + 1e-12


def test_a_filterbank_with_an_empty_filter_is_refused():
    with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE.*no non-zero weight"):
        SG.mel_table(512, 128)                                           # 31 Hz between centres, 86 Hz between bins
    with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE.*no non-zero weight"):
        post.SpectrogramFormat(n_fft=512, hop=128)
    with pytest.raises(L.VauraHipError, match="no non-zero weight"):
        SG.compact(np.array([[0, 1, 0], [0, 0, 0]], dtype=np.float32))


# ------------------------------------------------------------------------------------- the reference's own claims
@pytest.mark.parametrize("n_fft,hop", SIZES)
def test_reference_columns_and_per_column_rfft(n_fft, hop):
    g = torch.Generator().manual_seed(7)
    for n in (5 * hop, 3 * hop + 7, hop - 12, 1):
        x = torch.randn(n, generator=g) * 0.3
        X, beta, y32 = RS.spectrum(x, n_fft, hop)
        assert X.shape[0] == math.ceil(n / hop) == RS.columns(n, hop) and X.shape[1] == n_fft // 2 + 1
        w = RS.hann(n_fft)
        for t in range(X.shape[0]):
            lo = hop * t + hop // 2 - n_fft // 2
            frame = torch.tensor([float(x[s]) if 0 <= s < n else 0.0 for s in range(lo, lo + n_fft)], dtype=torch.float64)
            assert float((torch.fft.rfft(frame * w) - X[t]).abs().max()) <= 1e-12 * max(1.0, float(X[t].abs().max()))
            assert torch.equal(y32[t], (frame.float() * w.float()))
            assert abs(float(beta[t]) - RS.U * float((frame * w).abs().sum())) <= 1e-20


def test_reference_nan_reaches_exactly_the_columns_that_hold_it():
    x = torch.randn(12 * 512, generator=torch.Generator().manual_seed(1))
    x[6 * 512 + 100] = float("nan")
    X, _, _ = RS.spectrum(x, 2048, 512)
    assert [t for t in range(12) if bool(X[t].real.isnan().any())] == [4, 5, 6, 7]
    assert all(bool(X[t].real.isnan().all()) for t in (4, 5, 6, 7))


def test_reference_scale_bars():
    l, bar = RS.scaled(torch.tensor([1.0, 100.0, 0.0, 1e-20], dtype=torch.float32), "db", 1e-10)
    assert l[0] == 0 and bar[0] == 0 and abs(float(l[1]) - 20.0) < 1e-12 and abs(float(l[2]) + 100.0) < 1e-5 and l[3] == l[2]
    assert float(bar[1]) == 10 * 3 * 2.0 ** -22 + 0.5 * 2.0 ** -19
    l, bar = RS.scaled(torch.tensor([math.e], dtype=torch.float32), "log", 1e-10)
    assert abs(float(l[0]) - 1) < 1e-7 and float(bar[0]) in (3 * 2.0 ** -23, 3 * 2.0 ** -24)


# ------------------------------------------------------------------------------------- call-time refusals
def test_format_refusals_and_defaults():
    fmt = post.SpectrogramFormat()
    assert (fmt.n_fft, fmt.hop, fmt.n_mels, fmt.f_min, fmt.f_max, fmt.mel_scale, fmt.norm, fmt.scale, fmt.amin, fmt.bins) == \
        (2048, 512, 128, 0.0, None, "slaney", None, "db", 1e-10, 128)
    assert post.SpectrogramFormat(n_mels=None).bins == 1025 and post.SpectrogramFormat(n_fft=512, hop=128, n_mels=None).mel is None
    with pytest.raises(L.VauraHipError, match="top_db is not served"):
        post.SpectrogramFormat(top_db=80.0)
    with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE.*n_fft"):
        post.SpectrogramFormat(n_fft=4096)
    with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE.*hop"):
        post.SpectrogramFormat(hop=500)
    for n_mels in (0, 257, 128.0, True):
        with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE.*n_mels"):
            post.SpectrogramFormat(n_mels=n_mels)
    with pytest.raises(L.VauraHipError, match="VAURA_ERR_DTYPE.*scale"):
        post.SpectrogramFormat(scale="magnitude")
    with pytest.raises(L.VauraHipError, match="mel_scale"):
        post.SpectrogramFormat(mel_scale="bark")
    with pytest.raises(L.VauraHipError, match="goes with n_mels=None"):
        post.SpectrogramFormat(scale="complex")
    with pytest.raises(L.VauraHipError, match="norm must be"):
        post.SpectrogramFormat(norm="area")
    for amin in (0.0, -1.0, float("nan"), "1e-10"):
        with pytest.raises(L.VauraHipError, match="amin"):
            post.SpectrogramFormat(amin=amin)
    for f_min, f_max in ((-1.0, None), (8000.0, 8000.0), (0.0, 30000.0)):
        with pytest.raises(L.VauraHipError, match="mel range"):
            post.SpectrogramFormat(f_min=f_min, f_max=f_max)


def test_audio_to_spectrogram_refusals():
    fmt = post.SpectrogramFormat()
    with pytest.raises(L.VauraHipError, match="no CPU path"):
        post.audio_to_spectrogram(torch.zeros(1, 1, 64), fmt)
    with pytest.raises(L.VauraHipError, match="mono waveform"):
        post.audio_to_spectrogram(torch.zeros(1, 2, 64), fmt)
    with pytest.raises(L.VauraHipError, match="mono waveform"):
        post.audio_to_spectrogram(torch.zeros(64), fmt)
    with pytest.raises(L.VauraHipError, match="holds no samples"):
        post.audio_to_spectrogram(torch.zeros(1, 1, 0), fmt)
    with pytest.raises(L.VauraHipError, match="lengths must lie in 1 .. 64"):
        post.audio_to_spectrogram(torch.zeros(2, 1, 64), fmt, lengths=[64, 65])
    with pytest.raises(L.VauraHipError, match="lengths must lie in 1 .. 64"):
        post.audio_to_spectrogram(torch.zeros(2, 1, 64), fmt, lengths=[0, 64])
    with pytest.raises(L.VauraHipError, match="3 values for a batch of 2"):
        post.audio_to_spectrogram(torch.zeros(2, 1, 64), fmt, lengths=[1, 2, 3])
    with pytest.raises(L.VauraHipError, match="one integer per clip"):
        post.audio_to_spectrogram(torch.zeros(2, 1, 64), fmt, lengths=64)


def fake_launch(log):
    def launch(fmt, x, in_stride, records, carry_in, carry_out, n_row, ring=None):
        log.append((in_stride, [list(r) for r in records], n_row, None if carry_in is None else carry_in.data_ptr(),
                    None if carry_out is None else carry_out.data_ptr()))
        return torch.zeros(len(records), n_row, fmt.bins)
    return launch


def test_spectrogram_stream_refusals_and_state(monkeypatch):
    log = []
    monkeypatch.setattr(post, "_spec_launch", fake_launch(log))
    fmt = post.SpectrogramFormat()
    pl = fmt.plan
    s = post.SpectrogramStream(fmt, 2, "cpu")
    with pytest.raises(L.VauraHipError, match="samples must lie in 0 .. 100"):
        s.push(torch.zeros(2, 1, 100), samples=[100, 101])
    with pytest.raises(L.VauraHipError, match="samples has 3 values"):
        s.push(torch.zeros(2, 1, 100), samples=[1, 2, 3])
    with pytest.raises(L.VauraHipError, match="block of shape"):
        s.push(torch.zeros(3, 1, 100))
    with pytest.raises(L.VauraHipError, match="mono waveform"):
        s.push(torch.zeros(2, 2, 100))
    assert log == [] and s.received == [0, 0]                              # a refused push leaves the stream as it was
    spec, counts = s.push(torch.zeros(2, 1, 3000), samples=[3000, 0], final=[False, True])
    assert counts == [pl.releasable(3000), 0] == [4, 0] and s.finished == [False, True] and tuple(spec.shape) == (2, 4, 128)
    with pytest.raises(L.VauraHipError, match="clip 1 .* takes no more samples"):
        s.push(torch.zeros(2, 1, 10))
    spec, counts = s.push(None, final=True)
    assert counts == [pl.columns(3000) - 4, 0] and s.received == [3000, 0] and s.emitted == [6, 0]
    assert log[0][3] == log[1][4] and log[0][4] == log[1][3] and log[0][3] != log[0][4]      # the carry pair swaps every push
    with pytest.raises(L.VauraHipError, match="at least one clip"):
        post.SpectrogramStream(fmt, 0, "cpu")
    with pytest.raises(L.VauraHipError, match="on cpu"):
        post.SpectrogramStream(fmt, 2, "cpu").push(torch.zeros(2, 1, 8, device="meta"))


def test_stream_spectrogram_bookkeeping_on_fake_blocks(monkeypatch):
    log = []
    monkeypatch.setattr(post, "_spec_launch", fake_launch(log))
    fmt, hop = post.SpectrogramFormat(), 512
    pl = fmt.plan
    frames = [[4, 2], [3, 0], [0, 0], [2, 1]]
    blocks = [{"audio": torch.zeros(2, 1, max(f) * hop), "start_frames": [0, 0], "frames": f, "sampled_indices": i, "final": i == 3,
               "pcm": "kept"} for i, f in enumerate(frames)]
    out = list(post.stream_spectrogram(iter(blocks), fmt))
    assert len(out) == 4 and all(o["sampled_indices"] == i and o["frames"] == frames[i] and o["pcm"] == "kept" for i, o in enumerate(out))
    assert all(set(o) == set(blocks[0]) | {"spectrogram", "spec_start", "spec_columns"} for o in out) and "spectrogram" not in blocks[0]
    at, got = [0, 0], [0, 0]
    for i, o in enumerate(out):
        assert o["spec_start"] == at and tuple(o["spectrogram"].shape) == (2, max(o["spec_columns"]), 128)
        got = [g + f * hop for g, f in zip(got, frames[i])]
        at = [a + c for a, c in zip(at, o["spec_columns"])]
        assert at == [pl.columns(g) if i == 3 else pl.releasable(g) for g in got], i
        assert log[i][0] == max(max(frames[i]) * hop, 1) and [r[1] for r in log[i][1]] == [f * hop for f in frames[i]]
        assert [r[4] for r in log[i][1]] == (got if i == 3 else [-1, -1])
    assert at == [9, 3]                                                    # hop 512: the columns are the frames
    log.clear()                                                            # the equal-length style: ints
    blocks = [{"audio": torch.zeros(3, 1, n * hop), "start_frame": s, "frames": n, "final": fin} for s, n, fin in [(0, 16, False), (16, 27, True)]]
    out = list(post.stream_spectrogram(blocks, fmt))
    assert [o["spec_start"] for o in out] == [[0] * 3, [14] * 3] and [o["spec_columns"] for o in out] == [[14] * 3, [29] * 3]


# ------------------------------------------------------------------------------------- ABI
def test_symbol_is_typed_and_declared():
    assert "vaura_spectrogram" in L.SIGNATURES and "vaura_spectrogram_lds_bytes" in L.SIGNATURES
    header = open(os.path.join(ROOT, "include", "vaura_hip.h")).read()
    decl = re.search(r"int vaura_spectrogram\(([^;]*)\);", header)
    assert decl and len(decl.group(1).split(",")) == len(L.SIGNATURES["vaura_spectrogram"][1]) == 20
    assert "size_t vaura_spectrogram_lds_bytes(int n_fft, int F);" in header
    assert "#define VAURA_SPECTROGRAM_RECORD 5" in header and SG.RECORD == 5 and f"#define VAURA_SPECTROGRAM_MAX_MELS {SG.MAX_MELS}" in header
    assert "spectrogram.hip" in __import__("vaura_amd.csrc.build", fromlist=["SOURCES"]).SOURCES
    lib = L.lib()
    for n_fft in (512, 1024, 2048):
        need = lib.vaura_spectrogram_lds_bytes(n_fft, 128)
        assert 8 * n_fft <= need <= 8 * n_fft + 1024 and need == lib.vaura_spectrogram_lds_bytes(n_fft, n_fft // 2 + 1)
    assert lib.vaura_spectrogram_lds_bytes(4096, 128) == 0 and lib.vaura_spectrogram_lds_bytes(2048, 0) == 0
    assert lib.vaura_spectrogram_lds_bytes(512, 258) == 0


def test_entry_point_refuses_before_any_device_work():
    lib = L.lib()
    ARG, SHAPE, DTYPE = -1, -2, -3
    p = 4096                                                               # a non-null address that is never dereferenced: every call is refused
    H = 2047

    def call(x=p, B=1, in_stride=1000, rec=p, carry_in=p, carry_out=p + 8192, H=H, n_fft=2048, hop=512, window=p, tw=p, bins=p, weights=p,
             total=3000, F=128, scale=1, amin=1e-10, out=p, out_stride=5):
        return lib.vaura_spectrogram(x, B, in_stride, rec, carry_in, carry_out, H, n_fft, hop, window, tw, bins, weights, total, F, scale, amin,
                                     out, out_stride, 0)
    assert call(x=0) == ARG and call(rec=0) == ARG and call(window=0) == ARG and call(tw=0) == ARG and call(out=0) == ARG
    assert call(carry_in=0) == ARG and call(bins=0) == ARG and call(weights=0) == ARG      # one half of the table without the other
    assert call(carry_out=p, H=0, carry_in=0) == ARG                       # a carry to write needs a history
    assert call(carry_out=p) == ARG and call(carry_out=p + 4 * H - 4) == ARG and call(carry_in=p + 8192 + 4 * H - 4) == ARG   # the pair overlaps
    assert call(carry_out=p + 8 * H, B=3) == ARG                           # three clips: 12 H bytes each way
    assert call(B=0) == ARG and call(B=-1) == ARG and call(in_stride=-1) == ARG and call(out_stride=-1) == ARG and call(H=-1) == ARG
    assert call(in_stride=0) == ARG and call(amin=0.0) == ARG and call(amin=float("nan")) == ARG and call(amin=-1.0) == ARG
    assert call(x=p + 2) == ARG and call(rec=p + 4) == ARG and call(tw=p + 4) == ARG and call(window=p + 1) == ARG and call(out=p + 2) == ARG
    assert call(bins=p + 2) == ARG and call(weights=p + 3) == ARG and call(carry_in=p + 2) == ARG and call(carry_out=p + 8194) == ARG
    assert call(scale=4) == DTYPE and call(scale=-1) == DTYPE
    assert call(scale=3) == ARG and call(scale=3, bins=0, weights=0, F=1025) != ARG      # the transform itself goes without a mel table
    assert call(n_fft=256) == SHAPE and call(n_fft=4096) == SHAPE and call(n_fft=1000) == SHAPE and call(n_fft=0) == SHAPE
    assert call(hop=0) == SHAPE and call(hop=384) == SHAPE and call(hop=4096) == SHAPE and call(n_fft=512, hop=1024, H=511) == SHAPE
    assert call(F=0) == SHAPE and call(F=257) == SHAPE
    assert call(total=127) == SHAPE and call(total=128 * 1025 + 1) == SHAPE      # a filter without a bin; a support that leaves 0 .. n_fft/2
    assert call(bins=0, weights=0, F=128) == SHAPE and call(bins=0, weights=0, F=1024) == SHAPE    # the linear spectrum has n_fft/2 + 1 bins
    assert call(in_stride=2 ** 31) == SHAPE and call(out_stride=2 ** 31 - 1) == SHAPE
    assert call(B=65536) == SHAPE
