"""Audio preprocessing, the host side (vaura_amd/audio_preprocess.py): the compact tap table against the full formula, the float64
restatement of tests/audio_pre_reference.py against an independent direct sum and against an analytic sine, the length rules, the
parsing of the reference's ``audio_transforms_test`` lists, every refusal, and ``reference()`` (torch ops, fp32) on the CPU against
the restatement under its bar."""
import math

import numpy as np
import pytest
import torch

import audio_pre_reference as R
from vaura_amd import _lib as L
from vaura_amd import audio_preprocess as AP
from vaura_amd.audio_preprocess import AudioPreprocessor, output_length, resample_table

NEW = 44100
RATES_TAPS = [(8000, 13), (16000, 13), (22050, 13), (32000, 13), (48000, 14), (96000, 27), (192000, 53)]

# the `audio_transforms_test` entries of configs/generate_vas.yaml:43-54 and data/demo/dataloader_config.yaml:13-20, interpolations
# resolved (model_max_duration = sample_duration = 2.56)
VAS_TRANSFORMS = [
    {"target": "models.data.transforms.audio_transforms.AudioStereoToMono", "params": {"keepdim": True}},
    {"target": "models.data.transforms.audio_transforms.AudioResample", "params": {"target_sr": 44100, "clip_duration": 2.56}},
    {"target": "models.data.transforms.audio_transforms.AudioTrim", "params": {"duration": 2.56, "sr": 44100}},
]
DEMO_TRANSFORMS = [dict(e, params=dict(e["params"])) for e in VAS_TRANSFORMS]     # the demo loader's list holds the same entries


def noise_pcm(dtype, B, C, N, seed, interleaved=False):
    g = torch.Generator().manual_seed(seed)
    shape = (B, N, C) if interleaved else (B, C, N)
    if dtype == torch.int16:
        return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16)
    if dtype == torch.int32:
        return torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=torch.int64).to(torch.int32)
    return torch.rand(shape, generator=g) * 2 - 1


# ------------------------------------------------------------------------------------- the compact table
@pytest.mark.parametrize("orig,taps", RATES_TAPS)
def test_compact_table_is_the_full_table_without_its_zeros(orig, taps):
    tab = resample_table(orig, NEW)
    full = R.full_table(orig, NEW).to(torch.float32)
    o, n, w, _ = R.ratio(orig, NEW)
    assert (tab["o"], tab["n"], tab["w"]) == (o, n, w) and tab["taps"] == taps
    assert tab["first"].dtype == torch.int32 and tab["weights"].dtype == torch.float32 and tuple(tab["weights"].shape) == (n, taps)
    assert taps <= math.floor(12 * o / (min(o, n) * 0.99)) + 1
    padded = torch.cat([full, torch.zeros(n, taps)], dim=1)
    cols = tab["first"].long()[:, None] + torch.arange(taps)[None, :]
    assert int(tab["first"].min()) >= 0 and int(tab["first"].max()) < 2 * w + o
    assert torch.equal(padded.gather(1, cols), tab["weights"])                      # equal as fp32 on the run
    outside = torch.ones_like(padded, dtype=torch.bool).scatter_(1, cols, False)
    assert bool((padded[outside] == 0).all())                                      # exactly 0 everywhere else
    nz = full != 0
    first_nz = torch.where(nz, torch.arange(full.shape[1])[None, :], full.shape[1]).amin(dim=1)
    last_nz = torch.where(nz, torch.arange(full.shape[1])[None, :], -1).amax(dim=1)
    assert torch.equal(first_nz, tab["first"].long())
    assert torch.equal(nz.sum(dim=1), last_nz - first_nz + 1)                       # the run is contiguous
    assert int((last_nz - first_nz).max()) + 1 == taps
    assert float((tab["weights_f64"].to(torch.float32) - tab["weights"]).abs().max()) == 0


def test_tile_and_limits_are_the_library_s():
    lib = L.lib()
    assert lib.vaura_audio_preprocess_tile() == AP.TILE
    tab = resample_table(48000, NEW)
    need = lib.vaura_audio_preprocess_lds_bytes(tab["o"], tab["n"], tab["w"], tab["taps"])
    assert 4 * (AP.TILE * tab["o"] // tab["n"]) < need <= 64 * 1024
    assert lib.vaura_audio_preprocess_lds_bytes(0, 1, 1, 1) == 0


# ------------------------------------------------------------------------------------- the restatement itself
def test_restatement_equals_a_direct_sum():
    orig, C, N = 48000, 2, 400
    pcm = noise_pcm(torch.float32, 1, C, N, seed=1)
    out, n_out, _ = R.restate(pcm, orig, NEW, taps_per_phase=14)
    o, n, w, _ = R.ratio(orig, NEW)
    k = R.full_table(orig, NEW).to(torch.float32).double().numpy()
    x = pcm[0].double().numpy().mean(axis=0)
    direct = np.zeros(n_out[0])
    for m in range(n_out[0]):
        q, p = divmod(m, n)
        for j in range(2 * w + o):
            i = q * o + j - w
            if 0 <= i < N:
                direct[m] += k[p, j] * x[i]
    assert n_out == [math.ceil(n * N / o)]
    err = float(np.abs(out[0, 0].numpy() - direct).max())
    print(f"restatement vs direct sum: max |diff| {err:.3e}")
    assert err < 1e-14


def test_restatement_of_a_sine_is_the_sine():
    orig, N, f = 48000, 4800, 1000.0
    x = torch.sin(2 * math.pi * f * torch.arange(N, dtype=torch.float64) / orig)[None]
    y = R.restate_f64_taps(x, orig, NEW)[0]
    want = torch.sin(2 * math.pi * f * torch.arange(y.shape[0], dtype=torch.float64) / NEW)
    err = float((y - want)[50:-50].abs().max())
    print(f"1 kHz sine 48 kHz -> 44.1 kHz: max |restatement - analytic| away from the ends {err:.3e}")
    assert y.shape[0] == 4410 and err < 1e-3


# ------------------------------------------------------------------------------------- lengths and parsing
def test_length_rule_and_identity_shortcut():
    for orig in (8000, 22050, 48000, 47999, 96000):
        o, n, _, _ = R.ratio(orig, NEW)
        for nb in (1, 5, 1000, 122880, 2 ** 31 - 1):
            assert output_length(nb, orig, NEW) == (n * nb + o - 1) // o == R.out_length(nb, orig, NEW)
    assert output_length(122880, 48000, NEW) == 112896 == math.ceil(2.56 * 44100)
    assert output_length(122880, 48000, NEW, duration=1.0) == 44100
    assert output_length(10, 48000, NEW, duration=1.0) == 10 and output_length(1, 8000, NEW) == 6
    assert output_length(777, NEW, NEW) == 777 and output_length(50000, NEW, NEW, duration=1.00001) == 44101
    pre = AudioPreprocessor()
    pcm = noise_pcm(torch.int16, 2, 2, 300, seed=2)
    out, lengths = pre.reference(pcm, sample_rate=NEW, lengths=[300, 7])
    want = (pcm / 32768).mean(dim=1, keepdim=True)
    assert lengths.tolist() == [300, 7] and torch.equal(out[0], want[0]) and torch.equal(out[1, :, :7], want[1, :, :7])
    assert bool((out[1, :, 7:] == 0).all())
    with pytest.raises(L.VauraHipError, match="identity"):
        resample_table(NEW, NEW)


def test_source_rate_from_clip_duration():
    pre = AudioPreprocessor(duration=0.01)
    pcm = noise_pcm(torch.float32, 1, 1, 480, seed=3)
    a, la = pre.reference(pcm, clip_duration=0.01)                         # int(480 / 0.01) = 48000
    b, lb = pre.reference(pcm, sample_rate=48000)
    assert la.tolist() == lb.tolist() == [441] and torch.equal(a, b)
    c, lc = pre.reference(pcm, clip_duration=0.0100001)                    # int(480 / 0.0100001) = 47999: the loader's rule, as it is
    assert int(480 / 0.0100001) == 47999 and lc.tolist() == [min(441, output_length(480, 47999, NEW))]
    with pytest.raises(L.VauraHipError, match="not both"):
        pre.reference(pcm, sample_rate=48000, clip_duration=0.01)
    with pytest.raises(L.VauraHipError, match="source rate is needed"):
        pre.reference(pcm)
    with pytest.raises(L.VauraHipError, match="per-clip lengths"):
        pre.reference(pcm, clip_duration=0.01, lengths=[100])


@pytest.mark.parametrize("transforms", [VAS_TRANSFORMS, DEMO_TRANSFORMS])
def test_from_transforms_config(transforms):
    pre = AudioPreprocessor.from_transforms_config(transforms)
    assert (pre.target_sr, pre.duration, pre.clip_duration) == (44100, 2.56, 2.56)
    pcm = noise_pcm(torch.int16, 1, 2, 1280, seed=4)                      # 2.56 s at 500 Hz: the loader's rule gives the rate
    _, lengths = pre.reference(pcm)
    assert lengths.tolist() == [math.ceil(2.56 * 44100)]
    assert AudioPreprocessor.from_transforms_config(transforms[:2]).duration is None
    other = {"target": "models.data.transforms.audio_transforms.AudioRandomVolume", "params": {"p": 0.5}}
    with pytest.raises(L.VauraHipError, match="AudioRandomVolume"):
        AudioPreprocessor.from_transforms_config(transforms + [other])
    with pytest.raises(L.VauraHipError, match="AudioUnsqueeze"):
        AudioPreprocessor.from_transforms_config([{"target": "models.data.transforms.audio_transforms.AudioUnsqueeze", "params": {"dim": 0}}])
    with pytest.raises(L.VauraHipError, match="in that order"):
        AudioPreprocessor.from_transforms_config([transforms[1], transforms[0], transforms[2]])
    with pytest.raises(L.VauraHipError, match="target_sr"):
        AudioPreprocessor.from_transforms_config(transforms[:2] + [dict(transforms[2], params={"duration": 2.56, "sr": 16000})])


# ------------------------------------------------------------------------------------- refusals
def test_table_limits():
    tab = resample_table(47999, NEW)                                       # gcd 7: 6300 phases of 14 taps
    assert (tab["n"], tab["taps"], tab["n"] * tab["taps"]) == (6300, 14, 88200)
    with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE.*table"):
        resample_table(96001, NEW)                                         # gcd 1: 44100 phases of 27 taps > 2^20 entries
    with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE.*taps per phase"):
        resample_table(6 * NEW, NEW)                                       # 73 taps per phase
    pre = AudioPreprocessor()
    with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE.*channels"):
        pre.reference(torch.zeros(1, 9, 16), sample_rate=48000)
    with pytest.raises(L.VauraHipError, match="VAURA_ERR_DTYPE"):
        pre.reference(torch.zeros(1, 2, 16, dtype=torch.float64), sample_rate=48000)
    with pytest.raises(L.VauraHipError, match="lengths must lie"):
        pre.reference(torch.zeros(2, 2, 16), sample_rate=48000, lengths=[16, 17])


def test_entry_point_refuses_before_any_device_work():
    lib = L.lib()
    ARG, SHAPE, DTYPE = -1, -2, -3
    p = 4096                                                               # a non-null address that is never dereferenced: every call is refused

    def call(pcm=p, fmt=AP.PCM_S16, C=2, n_in=p, o=160, n=147, w=7, first=p, taps=p, phases=147, T=14, out=p, n_out=p, in_stride=1000,
             out_stride=919, B=1):
        return lib.vaura_audio_preprocess(pcm, fmt, 0, B, C, in_stride, n_in, o, n, w, first, taps, phases, T, out, out_stride, n_out, 0)
    assert call(pcm=0) == ARG and call(n_in=0) == ARG and call(out=0) == ARG and call(n_out=0) == ARG
    assert call(first=0) == ARG and call(taps=0) == ARG
    assert call(B=0) == ARG and call(C=0) == ARG and call(phases=146) == ARG
    assert call(C=9) == SHAPE
    assert call(fmt=3) == DTYPE and call(fmt=-1) == DTYPE
    assert call(T=65) == SHAPE
    assert call(n=44100, phases=44100, T=27, o=96001) == SHAPE             # more than 2^20 entries
    assert call(in_stride=2 ** 31) == SHAPE and call(out_stride=2 ** 31) == SHAPE
    assert call(o=64000, n=1, phases=1, T=64, w=32) == SHAPE               # the span of one tile does not fit the LDS
    assert call(B=65536) == SHAPE


# ------------------------------------------------------------------------------------- reference() on the CPU
@pytest.mark.parametrize("orig,dtype,interleaved,C", [(8000, torch.int16, False, 1), (22050, torch.int32, True, 2),
                                                       (48000, torch.int16, True, 2), (96000, torch.float32, False, 6)])
def test_reference_on_the_cpu_meets_the_bar(orig, dtype, interleaved, C):
    pre = AudioPreprocessor(duration=0.05)
    pcm = noise_pcm(dtype, 3, C, 3000, seed=orig + C, interleaved=interleaved)
    lengths = [3000, 5, 1777]
    got, got_len = pre.reference(pcm, sample_rate=orig, lengths=lengths, interleaved=interleaved)
    want, n_out, bar = R.restate(pcm, orig, NEW, lengths, interleaved, 0.05, taps_per_phase=pre.table(orig)["taps"])
    assert got.dtype == torch.float32 and got_len.tolist() == n_out and got.shape == want.shape
    ratio = float(((got.double() - want).abs() / bar.clamp(min=1e-300)).max())
    print(f"reference() on the CPU, {orig} Hz {dtype} C={C}: largest |error| / bar {ratio:.4f}")
    assert ratio <= 1.0
    for b in range(3):
        assert bool((got[b, :, n_out[b]:] == 0).all())


def test_reference_gathered_route_equals_the_full_form_route(monkeypatch):
    """Rates with a small gcd take the gathered runs instead of the full-form conv1d: the same sums in another order."""
    pre = AudioPreprocessor()
    pcm = noise_pcm(torch.float32, 1, 2, 2000, seed=9)
    a, _ = pre.reference(pcm, sample_rate=48000)
    monkeypatch.setattr(AP, "_FULL_FORM_LIMIT", 0)
    b, _ = AudioPreprocessor().reference(pcm, sample_rate=48000)
    assert a.shape == b.shape and float((a - b).abs().max()) < 16 * 2.0 ** -24
