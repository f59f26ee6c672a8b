"""The step after the hot path: post-codec audio scaling and the wav write of
``save_results`` (/root/reference/scripts/generate.py:392-461, utils/data_utils.py:407-466).

``normalize_audio`` / ``scale_audio`` keep the reference's names, keywords and return conventions; the arithmetic
runs in libvaura_hip.so (``vaura_audio_normalize`` / ``vaura_audio_loudness``) on the device tensor the codec produced — there is no
CPU path.  The 'loudness' strategy (``scale_audio``'s own default) is ITU-R BS.1770-4 integrated loudness as the reference's dependency
torchaudio 2.2.1 computes it (``transforms.Loudness``) — third-party and absent here, so it is restated from the published algorithm
and its parity is UNPINNED, like DAC's; the mp4 mux (PyAV) is host I/O outside this package.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from . import _lib as L
from . import clip_params

_STRATEGIES = {"clip": 0, "peak": 1, "rms": 2, "": 3, "none": 3}


def _clip_lengths(wav: torch.Tensor, lengths) -> torch.Tensor:
    """``lengths`` of a (B, 1, N) batch as the library takes them: B int32 on the device of ``wav``, every value in 1 .. N.  Refused
    here, before any device work: another count than B, a non-integer entry, a value outside 1 .. N, a (1, N) single clip.  (The values
    of an int32 tensor that already is on the device stay there: the library reads them back once and refuses the same range.)"""
    if wav.dim() != 3:
        raise L.VauraHipError(f"lengths go with a (B, 1, N) batch of clips, got a waveform of shape {tuple(wav.shape)}")
    clips, n = wav.shape[0], wav.shape[-1]
    if not clip_params.is_per_clip(lengths):
        raise L.VauraHipError(f"lengths must be one integer per clip (a list, tuple or 1-D tensor), got {lengths!r}")
    on_device = isinstance(lengths, torch.Tensor) and lengths.dtype == torch.int32 and lengths.device == wav.device
    if on_device:
        if lengths.dim() != 1:
            raise L.VauraHipError(f"per-clip lengths must be one-dimensional (one value per clip), got shape {tuple(lengths.shape)}")
        count = lengths.shape[0]
    else:
        vals = clip_params._int_list("lengths", lengths)
        count = len(vals)
    if count != clips:
        raise L.VauraHipError(f"per-clip lengths has {count} values for a batch of {clips} clips")
    if on_device:
        return lengths.contiguous()
    if min(vals) < 1 or max(vals) > n:
        raise L.VauraHipError(f"lengths must lie in 1 .. {n} (the samples of a row), got {vals}")
    return torch.tensor(vals, dtype=torch.int32, device=wav.device)


def normalize_audio(wav: torch.Tensor, normalize: bool = True, strategy: str = "peak", peak_clip_headroom_db: float = 6,
                    rms_headroom_db: float = 18, loudness_headroom_db: float = 12, loudness_compressor: bool = False,
                    log_clipping: bool = False, sample_rate: Optional[int] = None, stem_name: Optional[str] = None,
                    lengths=None) -> torch.Tensor:
    """wav (C=1, N) or (B, 1, N) fp32 on a HIP device -> same shape; statistics are per clip (leading dims).
    ``lengths`` (B ints, or an integer tensor: the "audio_lengths" of a ragged ``generate()``): clip b holds ``lengths[b]`` samples of
    its row.  Each clip comes out exactly as if it had been normalised alone at its own length, with zeros behind it; what the input
    holds behind a clip's end is never read."""
    if strategy == "loudness":
        assert sample_rate is not None, "Loudness normalization requires sample rate."        # data_utils.py:454
        return _normalize_loudness(wav, int(sample_rate), float(loudness_headroom_db), bool(loudness_compressor), lengths=lengths)
    if strategy not in _STRATEGIES:
        raise AssertionError(f"Unexpected strategy: '{strategy}'")
    lens = None if lengths is None else _clip_lengths(wav, lengths)      # host checks first: nothing has touched the device yet
    if not wav.is_cuda:
        raise L.VauraHipError("normalize_audio runs on the HIP device that holds the decoded waveform; there is no CPU path")
    if wav.dim() >= 2 and wav.shape[-2] != 1:
        raise NotImplementedError("multi-channel audio: the codec is mono (dac_8kbps_wrapper.yaml)")
    x = wav.to(torch.float32).contiguous()
    n = x.shape[-1]
    clips = x.numel() // n
    out = torch.empty_like(x)
    scratch = torch.empty(L.lib().vaura_audio_scratch_elems(clips), dtype=torch.float32, device=x.device)
    if lens is None:
        L.check(L.lib().vaura_audio_normalize(L.ptr(x), L.ptr(out), clips, n, _STRATEGIES[strategy], int(bool(normalize)),
                                              float(peak_clip_headroom_db), float(rms_headroom_db), L.ptr(scratch),
                                              L.current_stream()), "vaura_audio_normalize")
    else:
        L.check(L.lib().vaura_audio_normalize_clips(L.ptr(x), L.ptr(out), clips, n, L.ptr(lens), _STRATEGIES[strategy],
                                                    int(bool(normalize)), float(peak_clip_headroom_db), float(rms_headroom_db),
                                                    L.ptr(scratch), L.current_stream()), "vaura_audio_normalize_clips")
    if strategy in ("", "none") :
        assert bool(out.abs().max() < 1)        # data_utils.py:460 (with lengths: out holds zeros behind each clip, the valid samples decide)
    return out


def _normalize_loudness(wav: torch.Tensor, sample_rate: int, loudness_headroom_db: float, loudness_compressor: bool,
                        energy_floor: float = 2e-3, lengths=None) -> torch.Tensor:
    """normalize_loudness + _clip_wav (utils/data_utils.py:347-404): gain every clip to -loudness_headroom_db LKFS, optional tanh
    compressor, clamp to [-1, 1]; a clip below ``energy_floor`` rms or shorter than one 400 ms gating block is only clamped (the
    reference returns it unchanged from normalize_loudness — its unfold raises on the short one — and then clips)."""
    lens = None if lengths is None else _clip_lengths(wav, lengths)      # host checks first: nothing has touched the device yet
    if not wav.is_cuda:
        raise L.VauraHipError("normalize_audio runs on the HIP device that holds the decoded waveform; there is no CPU path")
    if wav.dim() >= 2 and wav.shape[-2] != 1:
        raise NotImplementedError("multi-channel audio: the codec is mono (dac_8kbps_wrapper.yaml)")
    x = wav.to(torch.float32).contiguous()
    n = x.shape[-1]
    clips = x.numel() // n
    out = torch.empty_like(x)
    scratch = torch.empty(L.lib().vaura_audio_loudness_scratch_elems(clips), dtype=torch.float32, device=x.device)
    if lens is None:
        L.check(L.lib().vaura_audio_loudness(L.ptr(x), L.ptr(out), clips, n, sample_rate, loudness_headroom_db, int(loudness_compressor),
                                             float(energy_floor), L.ptr(scratch), L.current_stream()), "vaura_audio_loudness")
    else:
        L.check(L.lib().vaura_audio_loudness_clips(L.ptr(x), L.ptr(out), clips, n, L.ptr(lens), sample_rate, loudness_headroom_db,
                                                   int(loudness_compressor), float(energy_floor), L.ptr(scratch), L.current_stream()),
                "vaura_audio_loudness_clips")
    g = scratch[:clips]
    out.loudness_untouched = g < 0                # the library marks clips the reference leaves alone (quiet / too short / no gated block) with a negative gain
    out.loudness_gains = torch.where(g < 0, torch.ones_like(g), g)       # the gains that were applied (1 = left alone)
    return out


def scale_audio(audio: torch.Tensor, strategy: str = "loudness", sample_rate: int = 24000, db: float = 6.0) -> torch.Tensor:
    """scripts/generate.py:440-461: one clip -> (1, N) tensor on the CPU, ready to be written."""
    if audio.dtype not in [torch.float32, torch.int32, torch.int16, torch.uint8]:
        audio = audio.to(torch.float32)
    audio = normalize_audio(audio, strategy=strategy, sample_rate=sample_rate, peak_clip_headroom_db=db)
    return audio.reshape(1, -1).to("cpu")


def scale_batch(audio: torch.Tensor, lengths, strategy: str = "loudness", sample_rate: int = 24000, db: float = 6.0) -> List[torch.Tensor]:
    """``scale_audio`` for the (B, 1, N) waveform of a ragged ``generate()``: one normalisation call, one copy to the host, then clip b
    as a (1, lengths[b]) tensor on the CPU — what ``scale_audio(audio[b, :, :lengths[b]], ...)`` returns."""
    if audio.dtype not in [torch.float32, torch.int32, torch.int16, torch.uint8]:
        audio = audio.to(torch.float32)
    out = normalize_audio(audio, strategy=strategy, sample_rate=sample_rate, peak_clip_headroom_db=db, lengths=lengths)
    host = out.to("cpu")
    return [host[b, :, :n].reshape(1, -1).clone() for b, n in enumerate(_host_lengths(lengths))]


def _host_lengths(lengths) -> List[int]:
    return [int(n) for n in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]


def save_wav(path: str, audio: torch.Tensor, sample_rate: int = 44100) -> None:
    """The ``torchaudio.save(audio_path, audio, fps)`` of save_results (generate.py:421): (1, N) fp32 -> 32-bit float wav."""
    from scipy.io import wavfile
    wavfile.write(path, int(sample_rate), audio.detach().to("cpu", torch.float32).reshape(-1).numpy())


def save_wavs(paths: Sequence[str], audio, lengths=None, sample_rate: int = 44100) -> None:
    """``save_wav`` per clip: ``audio`` is a (B, 1, N) tensor or a list of (1, n_b) tensors (``scale_batch``'s result); clip b's first
    ``lengths[b]`` samples (all of them without ``lengths``) go to ``paths[b]``."""
    clips = len(audio)
    if len(paths) != clips:
        raise L.VauraHipError(f"{len(paths)} paths for {clips} clips")
    if lengths is None:
        lens = [int(audio[b].shape[-1]) for b in range(clips)]
    else:
        lens = _host_lengths(lengths)
        if len(lens) != clips:
            raise L.VauraHipError(f"per-clip lengths has {len(lens)} values for a batch of {clips} clips")
        for b, n in enumerate(lens):
            if n < 1 or n > audio[b].shape[-1]:
                raise L.VauraHipError(f"lengths must lie in 1 .. {audio[b].shape[-1]} (the samples of clip {b}), got {lens}")
    host = audio.detach().to("cpu") if isinstance(audio, torch.Tensor) else audio      # one copy for a batch on the device
    for b, path in enumerate(paths):
        save_wav(path, host[b][..., :lens[b]], sample_rate)
