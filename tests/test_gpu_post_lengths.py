"""Per-clip lengths in the post stage, on the device: vaura_audio_normalize_clips / vaura_audio_loudness_clips (csrc/post.hip
audio_*_clips_kernel) and post.normalize_audio(lengths=..) / scale_batch / save_wavs on top of them.

The contract is bit equality with the one-clip call: clip b of the lengthed call, over its own samples [0, n_b), is what the existing
entry point gives for those samples alone at n_samples = n_b — torch.equal, no tolerance —, zeros behind it, and nothing behind a clip's
end is ever read (the input holds NaN there).  Against the CPU restatement (oracle/post_oracle.py) the bars are those of the existing
post tests (tests/test_gpu_plugins.py): 'clip' / 'peak' bit-exact, 'rms' 2e-6 of the clip's peak, 'loudness' gain 1e-3 relative and
waveform 1e-4 * max(1, gain); 'none' is a copy: bit-exact.

One batch: B = 6 rows of N = 112896 samples (2.56 s at 44.1 kHz); lengths [N, N - 1 (odd, no multiple of 4), 17641, 17640, 17639 (just
above, at and below one 400 ms gating block of 17640 samples), 1].  Seeded noise at about -20 dBFS; clip 0 has a loud first half and a
digitally silent second half (the gates matter), clip 1 is at about -70 dBFS (below the 2e-3 rms floor of 'loudness')."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import post_oracle as po  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import post, synth  # noqa: E402

DEV = "cuda:0"
SR = 44100
N = 112896
LENS = [112896, 112895, 17641, 17640, 17639, 1]
B = len(LENS)
QUIET, SHORT, SINGLE = 1, 4, 5


@pytest.fixture(scope="module")
def batch():
    g = torch.Generator().manual_seed(4410)
    host = (0.1 * torch.randn(B, 1, N, generator=g)).clamp(-0.95, 0.95)                      # about -20 dBFS
    host[0, 0, : N // 2] = (0.25 * torch.randn(N // 2, generator=g)).clamp(-0.95, 0.95)      # loud first half ..
    host[0, 0, N // 2:] = 0.0                                                                # .. digitally silent second half
    host[QUIET] = 10 ** (-70 / 20) * torch.randn(1, N, generator=g)                          # about -70 dBFS
    clips = [host[b, :, :n].clone() for b, n in enumerate(LENS)]                             # (1, n_b) on the CPU: the oracle's input
    for b, n in enumerate(LENS):
        host[b, :, n:] = float("nan")
    wav = host.to(DEV)
    alone = [wav[b:b + 1, :, :n].contiguous() for b, n in enumerate(LENS)]                   # (1, 1, n_b) on the device
    return dict(wav=wav, clips=clips, alone=alone)


def check_against_one_clip_calls(out, batch, **kw):
    """samples [0, n_b) are the bits of the one-clip call, zeros behind them (a NaN of the input's tail would show in either)"""
    ones = []
    for b, n in enumerate(LENS):
        one = post.normalize_audio(batch["alone"][b], **kw)
        assert torch.equal(out[b:b + 1, :, :n], one), (b, float((out[b:b + 1, :, :n] - one).abs().max()))
        assert bool((out[b, :, n:] == 0).all()), b
        ones.append(one)
    return ones


# ---------------------------------------------------------------------------------------------------------------- 1, 2: every strategy
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("strategy", ["clip", "peak", "rms", "none"])
@pytest.mark.parametrize("lengths_as", ["list", "int32_on_device"])
def test_each_clip_is_normalised_as_if_alone(batch, strategy, normalize, lengths_as):
    lengths = LENS if lengths_as == "list" else torch.tensor(LENS, dtype=torch.int32, device=DEV)
    kw = dict(normalize=normalize, strategy=strategy)
    out = post.normalize_audio(batch["wav"], lengths=lengths, **kw)
    assert out.shape == (B, 1, N) and out.dtype == torch.float32
    check_against_one_clip_calls(out, batch, **kw)
    got = out.cpu()
    for b, n in enumerate(LENS):
        ref = po.normalize_audio(batch["clips"][b].clone(), **kw)
        err, peak = float((got[b, :, :n] - ref).abs().max()), float(ref.abs().max())
        print(f"{strategy} normalize={normalize} clip {b} (n = {n}): max |device - oracle| = {err:.3e}, peak {peak:.3e}")
        if strategy == "rms":
            assert err <= 2e-6 * peak, (b, err, peak)
        else:
            assert torch.equal(got[b, :, :n], ref), (b, err)


@pytest.mark.parametrize("compressor", [False, True])
def test_loudness_of_each_clip_as_if_alone(batch, compressor):
    kw = dict(strategy="loudness", sample_rate=SR, loudness_headroom_db=14, loudness_compressor=compressor)
    out = post.normalize_audio(batch["wav"], lengths=LENS, **kw)
    ones = check_against_one_clip_calls(out, batch, **kw)
    assert out.loudness_gains.shape == (B,) and out.loudness_untouched.shape == (B,)
    for b, one in enumerate(ones):
        assert torch.equal(out.loudness_gains[b:b + 1], one.loudness_gains), b
        assert torch.equal(out.loudness_untouched[b:b + 1], one.loudness_untouched), b
    assert out.loudness_untouched.tolist() == [b in (QUIET, SHORT, SINGLE) for b in range(B)]
    got, gains = out.cpu(), out.loudness_gains.cpu()
    for b, n in enumerate(LENS):
        clip = batch["clips"][b]
        ref = po.normalize_loudness(clip, SR, loudness_headroom_db=14, loudness_compressor=compressor)
        if b in (QUIET, SHORT, SINGLE):
            assert float(gains[b]) == 1.0
        else:
            want = 10.0 ** ((-14 - po.loudness_lkfs(clip, SR)) / 20.0)
            print(f"loudness clip {b} (n = {n}): gain {float(gains[b]):.6f}, oracle {want:.6f}")
            assert abs(float(gains[b]) / want - 1.0) < 1e-3, (b, float(gains[b]), want)
        err = float((got[b, :, :n] - ref).abs().max())
        print(f"loudness compressor={compressor} clip {b} (n = {n}): max |device - oracle| = {err:.3e}")
        assert err < 1e-4 * max(1.0, float(gains[b])), (b, err)


# ---------------------------------------------------------------------------------------------------------------- 3: why it matters
def test_rms_without_lengths_is_too_loud_by_the_square_root_of_the_padding(batch):
    """The un-lengthed call on the zero-padded batch divides clip 2's energy by N instead of n_b = 17641: its gain is sqrt(N / n_b) =
    2.53 times the right one.  -30 dB of rms headroom keeps both gains below 1 / peak, so no sample is clamped and the ratio shows on
    every sample.  Bound: each gain is (1 / sqrt(ss / n)) * scale; ss is a sum of 17641 squares over 64 x 256 threads — at most 2 terms
    per thread, 8 butterfly levels, 64 ordered partials: <= 74 roundings, 74 * 2^-24 = 4.4e-6 relative, halved by the square root, for
    each of the two sums (their partitions differ), plus under ten single roundings (division, root, reciprocal, products) of 6e-8:
    5e-6 relative in all."""
    b, n = 2, LENS[2]
    kw = dict(strategy="rms", rms_headroom_db=30)
    padded = torch.nan_to_num(batch["wav"], nan=0.0)
    unlengthed = post.normalize_audio(padded, **kw)[b, 0, :n].cpu().double()
    lengthed = post.normalize_audio(batch["wav"], lengths=LENS, **kw)[b, 0, :n].cpu()
    factor = math.sqrt(N / n)
    assert float(unlengthed.abs().max()) < 1.0 and float(lengthed.abs().max()) > 0.0        # nothing was clamped
    rel = float(((unlengthed - lengthed.double() * factor).abs() / unlengthed.abs().clamp_min(1e-30)).max())
    print(f"rms: un-lengthed / lengthed on the {n}-sample clip = sqrt(N / n_b) = {factor:.6f} within {rel:.3e} relative")
    assert rel <= 5e-6
    ref = po.normalize_audio(batch["clips"][b].clone(), **kw)
    err = float((lengthed - ref[0]).abs().max())
    print(f"rms: lengthed against the oracle: {err:.3e} (peak {float(ref.abs().max()):.3e})")
    assert err <= 2e-6 * float(ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------- 4: helpers
@pytest.mark.parametrize("strategy", ["loudness", "clip"])
def test_scale_batch_and_save_wavs(batch, tmp_path, strategy):
    from scipy.io import wavfile
    half = batch["wav"].half()                                         # the reference's codec emits fp16 (scale_audio's dtype gate)
    clips = post.scale_batch(half, LENS, strategy=strategy, sample_rate=SR, db=3.0)
    assert len(clips) == B
    for b, n in enumerate(LENS):
        one = post.scale_audio(half[b, :, :n], strategy, SR, 3.0)
        assert clips[b].shape == (1, n) and clips[b].device.type == "cpu" and clips[b].dtype == torch.float32
        assert torch.equal(clips[b], one), b
    paths = [str(tmp_path / f"list_{b}.wav") for b in range(B)]
    post.save_wavs(paths, clips, sample_rate=SR)                       # scale_batch's list ..
    padded = [str(tmp_path / f"padded_{b}.wav") for b in range(B)]
    out = post.normalize_audio(half, strategy=strategy, sample_rate=SR, peak_clip_headroom_db=3.0, lengths=LENS)
    post.save_wavs(padded, out, torch.tensor(LENS, device=DEV), SR)    # .. or the padded batch on the device with its lengths
    for b, n in enumerate(LENS):
        for p in (paths[b], padded[b]):
            sr, data = wavfile.read(p)
            assert sr == SR and data.dtype == np.float32 and data.shape == (n,) and np.array_equal(data, clips[b].numpy().reshape(-1))


# ---------------------------------------------------------------------------------------------------------------- 5: end to end
def test_ragged_generate_into_one_post_call(tiny_sampler_sd):
    import test_gpu_logprobs as G
    model = G._model(tiny_sampler_sd)
    frames = synth.video_features(2, tokens=32, seed=31).reshape(2, 1, 32, 768).to(DEV)
    item = model.generate(frames=frames, prompt_is_encoded=True, top_k=250, cfg_scale=3.0, max_new_tokens=[20, 13])
    wav, lens = item["generated_audio"], item["audio_lengths"]
    hop = wav.shape[-1] // 20
    assert lens.tolist() == [20 * hop, 13 * hop]
    out = post.normalize_audio(wav, strategy="rms", lengths=lens)
    for b, n in enumerate(lens.tolist()):
        one = post.normalize_audio(wav[b:b + 1, :, :n].contiguous(), strategy="rms")
        assert torch.equal(out[b:b + 1, :, :n], one) and bool((out[b, :, n:] == 0).all()), b
    clips = post.scale_batch(wav, lens, sample_rate=SR)
    for b, n in enumerate(lens.tolist()):
        assert torch.equal(clips[b], post.scale_audio(wav[b, :, :n], sample_rate=SR)), b


# ---------------------------------------------------------------------------------------------------------------- 6: C-level refusals
@pytest.mark.parametrize("bad", [[N, 5, 0, 9], [N, 5, N + 1, 9], [-1, 5, 3, 9], None, "misaligned"])
def test_bad_lengths_are_refused_before_any_launch(batch, bad):
    lib = L.lib()
    wav = batch["wav"][:4]
    out = torch.full_like(wav, float("nan"))
    stream = L.current_stream(torch.device(DEV))
    lens = torch.tensor(bad, dtype=torch.int32, device=DEV) if isinstance(bad, list) else torch.zeros(8, dtype=torch.int32, device=DEV)
    p = None if bad is None else L.ptr(lens) + (2 if bad == "misaligned" else 0)
    s1 = torch.empty(lib.vaura_audio_scratch_elems(4), dtype=torch.float32, device=DEV)
    s2 = torch.empty(lib.vaura_audio_loudness_scratch_elems(4), dtype=torch.float32, device=DEV)
    for strategy in range(4):
        assert lib.vaura_audio_normalize_clips(L.ptr(wav), L.ptr(out), 4, N, p, strategy, 1, 6.0, 18.0, L.ptr(s1), stream) == -1
    assert lib.vaura_audio_loudness_clips(L.ptr(wav), L.ptr(out), 4, N, p, SR, 12.0, 0, 2e-3, L.ptr(s2), stream) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    if isinstance(bad, list):
        with pytest.raises(L.VauraHipError, match="VAURA_ERR_ARG"):        # an int32 tensor on the device is checked by the library
            post.normalize_audio(wav, strategy="peak", lengths=lens)
        good = torch.tensor([N, 5, 1, 9], dtype=torch.int32, device=DEV)
        assert lib.vaura_audio_loudness_clips(L.ptr(wav), L.ptr(out), 4, N, L.ptr(good), 11025, 12.0, 0, 2e-3, L.ptr(s2), stream) == -2
        assert bool(torch.isnan(out).all())
