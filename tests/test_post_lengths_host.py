"""Per-clip lengths in the post stage, host side: what normalize_audio / scale_batch / save_wavs refuse before any device work, that
``lengths=None`` is the call it always was (the same C entry points, the same arguments), where a lengthed call is routed, and that
the two new C entry points refuse a NULL length array without dereferencing anything."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from vaura_amd import _lib as L
from vaura_amd import post

N = 64


class FakeLib:
    """Stands in for libvaura_hip.so: records every call, touches nothing, reports success."""

    def __init__(self):
        self.calls = []

    def vaura_audio_scratch_elems(self, clips):
        return clips * 128

    def vaura_audio_loudness_scratch_elems(self, clips):
        return clips * 4097

    def __getattr__(self, name):
        def call(*args):
            if name.endswith("_clips"):       # the lengths as the library would read them
                args = args + (list((C.c_int32 * args[2]).from_address(args[4])),)
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture
def untouchable(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work was started")
    monkeypatch.setattr(L, "lib", touched)
    monkeypatch.setattr(L, "current_stream", touched)


@pytest.fixture
def fake(monkeypatch):
    """CPU tensors pass for device tensors and the library is a recorder: the host path runs to its end without a device."""
    lib = FakeLib()
    monkeypatch.setattr(L, "lib", lambda: lib)
    monkeypatch.setattr(L, "current_stream", lambda device=None: 77)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    return lib


BAD = [
    ([N, 5, 9], "3 values for a batch of 4"),
    ([N, 5, 9, 1, 2], "5 values for a batch of 4"),
    ([N, 5.0, 1, 9], "integers"),
    ([N, True, 1, 9], "integers"),
    (torch.tensor([1.0, 2.0, 3.0, 4.0]), "integers"),
    ([N, 5, 0, 9], "must lie in 1 .. 64"),
    ([N + 1, 5, 1, 9], "must lie in 1 .. 64"),
    (torch.tensor([N, 5, -3, 9]), "must lie in 1 .. 64"),
    (torch.ones(2, 2, dtype=torch.int64), "one-dimensional"),
    (torch.ones(2, 2, dtype=torch.int32), "one-dimensional"),
    (torch.ones(3, dtype=torch.int32), "3 values for a batch of 4"),
    (7, "one integer per clip"),
]


@pytest.mark.parametrize("strategy", ["rms", "none", "loudness"])
@pytest.mark.parametrize("lengths,match", BAD)
def test_refused_before_any_device_work(untouchable, strategy, lengths, match):
    wav = torch.zeros(4, 1, N)
    with pytest.raises(L.VauraHipError, match=match):
        post.normalize_audio(wav, strategy=strategy, sample_rate=44100, lengths=lengths)
    with pytest.raises(L.VauraHipError, match=match):
        post.scale_batch(wav, lengths, strategy=strategy, sample_rate=44100)


@pytest.mark.parametrize("strategy", ["clip", "loudness"])
def test_lengths_with_a_single_clip_tensor_are_refused(untouchable, strategy):
    with pytest.raises(L.VauraHipError, match=r"\(B, 1, N\) batch"):
        post.normalize_audio(torch.zeros(1, N), strategy=strategy, sample_rate=44100, lengths=[N])
    with pytest.raises(L.VauraHipError, match=r"\(B, 1, N\) batch"):
        post.normalize_audio(torch.zeros(N), strategy=strategy, sample_rate=44100, lengths=[N])


def test_save_wavs_refusals(tmp_path):
    wav = torch.zeros(2, 1, N)
    paths = [str(tmp_path / "a.wav"), str(tmp_path / "b.wav")]
    for args, match in (((paths[:1], wav), "1 paths for 2 clips"), ((paths, wav, [N]), "1 values for a batch of 2"),
                        ((paths, wav, [N, 0]), "must lie in 1 .. 64"), ((paths, wav, [N + 1, 3]), "must lie in 1 .. 64")):
        with pytest.raises(L.VauraHipError, match=match):
            post.save_wavs(*args)
    assert not os.listdir(tmp_path)


def test_save_wavs_writes_each_clip_at_its_own_length(tmp_path):
    from scipy.io import wavfile
    wav = torch.arange(3 * N, dtype=torch.float32).reshape(3, 1, N) / (3 * N)
    lens = [N, 17, 1]
    paths = [str(tmp_path / f"{b}.wav") for b in range(3)]
    post.save_wavs(paths, wav, torch.tensor(lens), 44100)
    for b, p in enumerate(paths):
        sr, data = wavfile.read(p)
        assert sr == 44100 and data.dtype == np.float32 and np.array_equal(data, wav[b, 0, :lens[b]].numpy())
    one = str(tmp_path / "one.wav")
    post.save_wav(one, wav[1, :, :17], 44100)                       # the file save_wav writes for the slice: the same bytes
    assert open(one, "rb").read() == open(paths[1], "rb").read()
    post.save_wavs(paths, [wav[b, :, :n] for b, n in enumerate(lens)], sample_rate=24000)       # scale_batch's list, no lengths
    sr, data = wavfile.read(paths[1])
    assert sr == 24000 and np.array_equal(data, wav[1, 0, :17].numpy())


def test_no_lengths_is_the_call_it_always_was(fake):
    wav = torch.zeros(4, 1, N)
    out = post.normalize_audio(wav, normalize=False, strategy="rms", peak_clip_headroom_db=3, rms_headroom_db=20)
    (name, args), = fake.calls
    assert name == "vaura_audio_normalize" and len(args) == 10
    assert args[2:8] == (4, N, 2, 0, 3.0, 20.0) and args[1] == out.data_ptr() and args[9] == 77 and args[8] != 0
    fake.calls.clear()
    out = post.normalize_audio(wav, strategy="loudness", sample_rate=44100, loudness_headroom_db=14, loudness_compressor=True)
    (name, args), = fake.calls
    assert name == "vaura_audio_loudness" and len(args) == 10
    assert args[2:8] == (4, N, 44100, 14.0, 1, 2e-3) and args[1] == out.data_ptr() and args[9] == 77
    fake.calls.clear()
    post.scale_audio(wav[0], "clip", 44100)
    (name, args), = fake.calls
    assert name == "vaura_audio_normalize" and args[2:8] == (1, N, 0, 1, 6.0, 18.0)


@pytest.mark.parametrize("lengths", [[N, 5, 1, 9], (N, 5, 1, 9), torch.tensor([N, 5, 1, 9]), torch.tensor([N, 5, 1, 9], dtype=torch.int32)])
def test_lengths_route_to_the_clips_entry_points(fake, lengths):
    wav = torch.zeros(4, 1, N)
    out = post.normalize_audio(wav, normalize=False, strategy="peak", peak_clip_headroom_db=3, lengths=lengths)
    (name, args), = fake.calls
    assert name == "vaura_audio_normalize_clips" and len(args) == 12
    assert args[2:4] == (4, N) and args[5:9] == (1, 0, 3.0, 18.0) and args[1] == out.data_ptr() and args[10] == 77
    assert args[4] % 4 == 0 and args[11] == [N, 5, 1, 9]
    if isinstance(lengths, torch.Tensor) and lengths.dtype == torch.int32:
        assert args[4] == lengths.data_ptr()                     # an int32 tensor that is where the waveform is goes in as it is
    fake.calls.clear()
    out = post.normalize_audio(wav, strategy="loudness", sample_rate=24000, lengths=lengths)
    (name, args), = fake.calls
    assert name == "vaura_audio_loudness_clips" and len(args) == 12
    assert args[2:4] == (4, N) and args[5:9] == (24000, 12.0, 0, 2e-3) and args[11] == [N, 5, 1, 9]
    assert out.loudness_gains.shape == (4,) and out.loudness_untouched.shape == (4,)
    fake.calls.clear()
    clips = post.scale_batch(wav, lengths, strategy="clip", sample_rate=44100, db=3.0)
    (name, args), = fake.calls
    assert name == "vaura_audio_normalize_clips" and args[5:9] == (0, 1, 3.0, 18.0)
    assert [tuple(c.shape) for c in clips] == [(1, N), (1, 5), (1, 1), (1, 9)] and all(c.device.type == "cpu" for c in clips)


def test_new_entry_points_refuse_a_null_length_array():
    """no array: refused, nothing dereferenced (the other pointers point nowhere)"""
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libvaura_hip.so is not built")
    one = C.c_void_p(16)
    lib = L.lib()
    assert lib.vaura_audio_normalize_clips(one, one, 4, N, None, 2, 1, 6.0, 18.0, one, None) == -1
    assert lib.vaura_audio_loudness_clips(one, one, 4, N, None, 44100, 12.0, 0, 2e-3, one, None) == -1
    assert lib.vaura_audio_normalize_clips(one, one, 4, 0, one, 2, 1, 6.0, 18.0, one, None) == -1
    assert lib.vaura_audio_normalize_clips(one, one, 4, N, C.c_void_p(18), 2, 1, 6.0, 18.0, one, None) == -1      # misaligned: before any copy
    assert lib.vaura_audio_loudness_clips(one, one, 4, N, C.c_void_p(18), 44100, 12.0, 0, 2e-3, one, None) == -1
