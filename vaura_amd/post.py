"""The step after the hot path: post-codec audio scaling and the wav write of
``save_results`` (/root/reference/scripts/generate.py:392-461, utils/data_utils.py:407-466).

``normalize_audio`` / ``scale_audio`` keep the reference's names, keywords and return conventions; the arithmetic
runs in libvaura_hip.so (``vaura_audio_normalize`` / ``vaura_audio_loudness``) on the device tensor the codec produced — there is no
CPU path.  The 'loudness' strategy (``scale_audio``'s own default) is ITU-R BS.1770-4 integrated loudness as the reference's dependency
torchaudio 2.2.1 computes it (``transforms.Loudness``) — third-party and absent here, so it is restated from the published algorithm
and its parity is UNPINNED, like DAC's; the mp4 mux (PyAV) is host I/O outside this package.

What a player, an Opus / WebRTC sender or the AAC encoder behind ``write_video`` takes is integer PCM at its own rate with its own
channel count: ``PcmFormat`` / ``audio_to_pcm`` / ``PcmStream`` / ``stream_pcm`` / ``save_pcm_wavs`` turn the device waveform into that
in one launch of ``vaura_audio_output`` (csrc/audio_out.hip) per call or per streamed block, the blocks concatenated being the one-pass
result bit for bit (the filter history travels in a carry row on the device).

The picture of the audio — ``SpectrogramFormat`` / ``audio_to_spectrogram`` / ``SpectrogramStream`` / ``stream_spectrogram`` — is one
launch of ``vaura_spectrogram`` (csrc/spectrogram.hip) in the same way: log-mel or linear columns, one per codec frame at hop 512, the
streamed columns concatenated being the one-pass result bit for bit.

Loudness for a stream — ``LoudnessTarget`` / ``measure_loudness`` / ``normalize_loudness_causal`` / ``LoudnessStream`` /
``stream_loudness`` — is ``vaura_audio_loudness_push`` (csrc/loudness.hip): an ITU-R BS.1770 meter (momentary, short-term, integrated)
and a causal normaliser whose gain at a sample depends only on the 100 ms steps completed before it, so every pushed sample leaves in
the same push and the pushes concatenated are the one-pass result bit for bit.  ``normalize_audio(strategy="loudness")`` keeps its own
kernel and its bits.
"""
from __future__ import annotations

from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib as L
from . import audio_out as AO
from . import clip_params
from . import loudness as LD
from . import spectrogram as SG

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


# ------------------------------------------------------------------------------------------------ PCM at the consumer's rate
_PCM_FORMATS = {torch.int16: 0, torch.int32: 1, torch.float32: 2}      # VAURA_PCM_S16 / S32 / F32


class PcmFormat:
    """What the consumer of the audio takes: ``rate`` Hz, ``dtype`` int16 / int32 / float32, ``channels`` copies of the mono signal
    (1 .. 8), interleaved (B, N, C) or planar (B, C, N), and a ``gain`` — one factor, or one per clip — applied before the
    conversion (``normalize_audio`` needs whole-clip statistics; ``stream_loudness`` underneath levels a stream causally).
    Refused here: a rate the resampler's table refuses (8 kHz and below need more than 64 taps per phase from 44.1 kHz), another dtype, ``channels`` outside 1 .. 8."""

    def __init__(self, rate: int = 48000, dtype: torch.dtype = torch.int16, channels: int = 2, interleaved: bool = True,
                 gain: Union[float, Sequence[float]] = 1.0):
        if dtype not in _PCM_FORMATS:
            raise L.VauraHipError(f"VAURA_ERR_DTYPE: PCM output is int16, int32 or float32; got {dtype}")
        if isinstance(channels, bool) or not isinstance(channels, int) or not 1 <= channels <= AO.MAX_CHANNELS:
            raise L.VauraHipError(f"VAURA_ERR_SHAPE: {channels!r} output channels; 1 .. {AO.MAX_CHANNELS}")
        self.plan = AO.plan(rate)                                         # raises for rates the table refuses
        self.rate, self.dtype, self.channels, self.interleaved = rate, dtype, channels, bool(interleaved)
        if clip_params.is_per_clip(gain):
            self.gain = [float(g) for g in (gain.tolist() if hasattr(gain, "tolist") else gain)]
        else:
            self.gain = float(gain)

    def gains(self, clips: int) -> List[float]:
        if isinstance(self.gain, list):
            if len(self.gain) != clips:
                raise L.VauraHipError(f"PcmFormat.gain has {len(self.gain)} values for a batch of {clips} clips")
            return self.gain
        return [self.gain] * clips

    def __repr__(self):
        return (f"PcmFormat(rate={self.rate}, dtype={self.dtype}, channels={self.channels}, interleaved={self.interleaved}, "
                f"gain={self.gain})")


_pcm_tables: Dict[Tuple[int, str], tuple] = {}


def _pcm_table(pl: AO.OutputPlan, dev: torch.device):
    """(first, taps tap-major (T, n)) of a rate on a device, built once"""
    key = (pl.rate, str(dev))
    if key not in _pcm_tables:
        _pcm_tables[key] = (pl.table["first"].to(dev), pl.table["weights"].t().contiguous().to(dev))
    return _pcm_tables[key]


class _RecordRing:
    """Pinned (B, width) int64 buffers for the per-clip records, allocated once and reused in turn.  A slot is taken again only when the
    copy that last read it has finished (its event is queried, never waited for); while it has not, a fresh pinned tensor serves
    that one push, so the host never waits for the device."""
    SLOTS = 4

    def __init__(self, clips: int, width: int = AO.RECORD):
        self.clips, self.width, self.slots, self.events, self.at = clips, width, [], [], 0

    def send(self, records: List[List[int]], dev: torch.device) -> torch.Tensor:
        host = torch.tensor(records, dtype=torch.int64)
        if len(self.slots) < self.SLOTS:
            self.slots.append(torch.empty(self.clips, self.width, dtype=torch.int64).pin_memory())
            self.events.append(torch.cuda.Event())
            i = len(self.slots) - 1
        else:
            i, self.at = self.at, (self.at + 1) % self.SLOTS
            if not self.events[i].query():                                # still in flight: leave the slot alone
                return host.pin_memory().to(dev, non_blocking=True)
        self.slots[i].copy_(host)
        rec = self.slots[i].to(dev, non_blocking=True)
        self.events[i].record(torch.cuda.current_stream(dev))
        return rec


_pcm_rings: Dict[Tuple[int, str], _RecordRing] = {}
_pcm_gains: Dict[Tuple[tuple, str], torch.Tensor] = {}


def _pcm_gain(gains: List[float], dev: torch.device) -> torch.Tensor:
    """the per-clip gains on the device, built once per (values, device)"""
    key = (tuple(gains), str(dev))
    if key not in _pcm_gains:
        if len(_pcm_gains) >= 16:
            _pcm_gains.clear()
        _pcm_gains[key] = torch.tensor(gains, dtype=torch.float32).to(dev)
    return _pcm_gains[key]


def _pcm_launch(fmt: PcmFormat, x: torch.Tensor, in_stride: int, records: List[List[int]], gain: Optional[torch.Tensor],
                carry_in: Optional[torch.Tensor], carry_out: Optional[torch.Tensor], n_row: int,
                ring: Optional[_RecordRing] = None) -> torch.Tensor:
    """One launch of vaura_audio_output over ``x`` (B rows of ``in_stride`` fp32 samples on a HIP device) -> the PCM tensor with its
    ``clipped`` counts.  The records travel by one asynchronous copy from a pinned buffer of ``ring`` (default: the one kept per batch
    size and device); ``gain`` None: ``fmt``'s, cached on the device.  Nothing here waits for the device."""
    dev, B, pl = x.device, len(records), fmt.plan
    if not x.is_cuda:
        raise L.VauraHipError("PCM output runs on the HIP device that holds the decoded waveform; there is no CPU path")
    lib = L.lib()
    if not pl.identity and lib.vaura_audio_output_lds_bytes(pl.o, pl.n, pl.w, pl.T) > 64 * 1024:
        raise L.VauraHipError(f"VAURA_ERR_SHAPE: {pl.source} -> {pl.rate} Hz: the input span of one tile does not fit 64 KiB of LDS")
    with torch.cuda.device(dev):
        first, taps = (None, None) if pl.identity else _pcm_table(pl, dev)
        if ring is None:
            ring = _pcm_rings.setdefault((B, str(dev)), _RecordRing(B))
        rec = ring.send(records, dev)
        if gain is None:
            gain = _pcm_gain(fmt.gains(B), dev)
        shape = (B, n_row, fmt.channels) if fmt.interleaved else (B, fmt.channels, n_row)
        out = torch.empty(shape, dtype=fmt.dtype, device=dev)
        clipped = torch.zeros(B, dtype=torch.int32, device=dev)
        history = 0 if carry_in is None else carry_in.shape[-1]
        L.check(lib.vaura_audio_output(L.ptr(x), B, in_stride, L.ptr(rec), L.ptr(carry_in), L.ptr(carry_out), history,
                                       pl.o if not pl.identity else 1, pl.n if not pl.identity else 1, pl.w if not pl.identity else 0,
                                       L.ptr(first), L.ptr(taps), pl.n if not pl.identity else 1, pl.T,
                                       L.ptr(gain), _PCM_FORMATS[fmt.dtype], int(fmt.interleaved), fmt.channels,
                                       L.ptr(out) if n_row else 0, n_row, L.ptr(clipped), L.current_stream(dev)), "vaura_audio_output")
    out.clipped = clipped
    return out


def _mono_rows(wav: torch.Tensor, what: str) -> torch.Tensor:
    """(B, 1, N) or (1, N) fp32 on a HIP device -> contiguous (B, 1, N)"""
    if not torch.is_tensor(wav) or wav.dim() not in (2, 3) or wav.shape[-2] != 1:
        raise L.VauraHipError(f"{what} takes the codec's mono waveform, (B, 1, N) or (1, N); got "
                              f"{tuple(wav.shape) if torch.is_tensor(wav) else type(wav).__name__}")
    if wav.dim() == 2:
        wav = wav[None]
    return wav.to(torch.float32).contiguous()


def audio_to_pcm(wav: torch.Tensor, fmt: PcmFormat, lengths=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """wav (B, 1, N) fp32 at 44.1 kHz on a HIP device -> (pcm, pcm_lengths): ``pcm`` (B, N_out, C) — planar: (B, C, N_out) — of
    ``fmt.dtype`` on the same device, ``pcm_lengths`` (B,) int64 on the host, ``pcm.clipped`` (B,) int32 on the device: the samples that
    left the format's range.  ``lengths`` (the "audio_lengths" of a ragged ``generate()``): clip b is exactly the clip converted alone
    at its own length, zeros follow it, and nothing behind ``lengths[b]`` is read."""
    x = _mono_rows(wav, "audio_to_pcm")
    B, N = x.shape[0], x.shape[-1]
    if N < 1:
        raise L.VauraHipError(f"a waveform of shape {tuple(wav.shape)} holds no samples")
    if lengths is None:
        n_in = [N] * B
    else:
        if not clip_params.is_per_clip(lengths):
            raise L.VauraHipError(f"lengths must be one integer per clip (a list, tuple or 1-D tensor), got {lengths!r}")
        n_in = clip_params._int_list("lengths", lengths)
        if len(n_in) != B:
            raise L.VauraHipError(f"per-clip lengths has {len(n_in)} values for a batch of {B} clips")
        if min(n_in) < 1 or max(n_in) > N:
            raise L.VauraHipError(f"lengths must lie in 1 .. {N} (the samples of a row), got {n_in}")
    n_out = [fmt.plan.output_total(n) for n in n_in]
    if max(n_out) > (1 << 31) - 1:
        raise L.VauraHipError(f"VAURA_ERR_SHAPE: output rows of {max(n_out)} samples; at most {(1 << 31) - 1}")
    fmt.gains(B)                                                         # refuses another count than B before any device work
    records = [[0, n, 0, m, n] for n, m in zip(n_in, n_out)]             # the stream's one and last block, from its start
    pcm = _pcm_launch(fmt, x, N, records, None, None, None, max(n_out))
    return pcm, torch.tensor(n_out, dtype=torch.int64)


class PcmStream:
    """``audio_to_pcm`` block by block: ``push`` takes the next samples of every clip and returns the PCM that can no longer change.
    The pushes concatenated per clip are bit for bit ``audio_to_pcm`` of the whole clips.  State: two integers per clip on the host
    (samples received, outputs emitted) and a ping-pong pair of carry rows on the device (``audio_out.history()`` samples per clip).
    One push is one launch and one asynchronous copy of a (B, 5) record from a pinned buffer the stream keeps; nothing waits for the
    device."""

    def __init__(self, fmt: PcmFormat, batch: int, device):
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            raise L.VauraHipError(f"PcmStream takes a batch of at least one clip, got {batch!r}")
        self.fmt, self.batch, self.device = fmt, batch, torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        gains = fmt.gains(batch)
        self.received, self.emitted, self.finished = [0] * batch, [0] * batch, [False] * batch
        H = fmt.plan.history()
        self._carry = torch.zeros(2, batch, H, dtype=torch.float32, device=self.device) if H else None
        self._cur = 0
        self._gains, self._ring = gains, _RecordRing(batch)
        self._empty = torch.zeros(batch, 1, 1, dtype=torch.float32, device=self.device)

    def _per_clip(self, name, value, kind):
        if clip_params.is_per_clip(value):
            vals = [kind(v) for v in (value.tolist() if hasattr(value, "tolist") else value)]
            if len(vals) != self.batch:
                raise L.VauraHipError(f"{name} has {len(vals)} values for a stream of {self.batch} clips")
            return vals
        return [kind(value)] * self.batch

    def push(self, audio: Optional[torch.Tensor], samples=None, final=False) -> Tuple[torch.Tensor, List[int]]:
        """audio (B, 1, n) fp32 on the stream's device: the next ``samples[b]`` samples of clip b (default: all n; 0 is allowed, and
        ``audio`` may be None when every clip gives 0) -> (pcm (B, max(counts), C) or planar (B, C, max(counts)), counts): clip b's next
        ``counts[b]`` output samples, zeros behind them.  ``final`` (a bool, or one per clip) flushes the clip's tail up to
        ``output_total`` of everything it received; a finished clip takes no more samples."""
        if audio is None:
            x, n = self._empty, 0
        else:
            x = _mono_rows(audio, "PcmStream.push")
            n = x.shape[-1]
            if x.shape[0] != self.batch or x.device != self.device:
                raise L.VauraHipError(f"PcmStream of {self.batch} clips on {self.device}: got a block of shape {tuple(audio.shape)} on {x.device}")
            if n == 0:
                x = self._empty
        counts_in = [n] * self.batch if samples is None else self._per_clip("samples", samples, int)
        fin = self._per_clip("final", final, bool)
        if min(counts_in) < 0 or max(counts_in) > n:
            raise L.VauraHipError(f"samples must lie in 0 .. {n} (the samples of a block's row), got {counts_in}")
        for b in range(self.batch):
            if self.finished[b] and counts_in[b]:
                raise L.VauraHipError(f"clip {b} of the stream was flushed (final) and takes no more samples; got {counts_in[b]}")
        records, received, emitted = AO.push_records(self.fmt.plan, self.received, self.emitted, counts_in, fin)
        counts = [r[3] for r in records]
        if max(counts) > (1 << 31) - 1:
            raise L.VauraHipError(f"VAURA_ERR_SHAPE: output rows of {max(counts)} samples; at most {(1 << 31) - 1}")
        carry_in = carry_out = None
        if self._carry is not None:
            carry_in, carry_out = self._carry[self._cur], self._carry[1 - self._cur]
        pcm = _pcm_launch(self.fmt, x, max(n, 1), records, None, carry_in, carry_out, max(counts), ring=self._ring)
        self._cur = 1 - self._cur
        self.received, self.emitted = received, emitted
        self.finished = [a or b for a, b in zip(self.finished, fin)]
        return pcm, counts


def stream_pcm(blocks: Iterable[dict], fmt: PcmFormat) -> Iterator[dict]:
    """Wrap a streaming generator (``generate_stream``, ``generate_long_stream`` with or without ``block_frames``,
    ``generate_long_clips_stream``): every dict comes back with "pcm" (the block's audio in ``fmt``), "pcm_start" and "pcm_samples" (one
    int per clip: where the block's output samples start in the clip's PCM and how many there are) and "pcm_clipped" (B int32 on the
    device) added.  A clip's samples are ``frames`` times the hop (``audio.shape[-1] // max(frames)``).  The resampler holds a few
    output samples back until their right-hand neighbours exist; the dict whose "final" is true carries every clip's tail."""
    stream = None
    for blk in blocks:
        audio = blk["audio"]
        B = audio.shape[0]
        frames = blk["frames"]
        frames = [int(f) for f in frames] if isinstance(frames, (list, tuple)) else [int(frames)] * B
        hop = audio.shape[-1] // max(frames) if max(frames) > 0 else 0
        if stream is None:
            stream = PcmStream(fmt, B, audio.device)
        start = list(stream.emitted)
        pcm, counts = stream.push(audio, [f * hop for f in frames], final=bool(blk["final"]))
        out = dict(blk)
        out.update(pcm=pcm, pcm_start=start, pcm_samples=counts, pcm_clipped=pcm.clipped)
        yield out


def save_pcm_wavs(paths: Sequence[str], pcm: torch.Tensor, lengths, fmt: PcmFormat) -> None:
    """The counterpart of ``save_wavs`` for ``audio_to_pcm``'s result: clip b's first ``lengths[b]`` frames go to ``paths[b]`` as an
    int16, int32 or 32-bit float wav of ``fmt.channels`` channels at ``fmt.rate`` Hz (scipy.io.wavfile)."""
    from scipy.io import wavfile
    clips = pcm.shape[0]
    lens = _host_lengths(lengths)
    if len(paths) != clips or len(lens) != clips:
        raise L.VauraHipError(f"{len(paths)} paths and {len(lens)} lengths for {clips} clips")
    if pcm.dtype != fmt.dtype or pcm.dim() != 3 or pcm.shape[2 if fmt.interleaved else 1] != fmt.channels:
        raise L.VauraHipError(f"a PCM tensor of shape {tuple(pcm.shape)} and {pcm.dtype} is not {fmt!r}")
    host = pcm.detach().to("cpu")
    if not fmt.interleaved:
        host = host.transpose(1, 2)                                       # wavfile takes (frames, channels)
    for b, path in enumerate(paths):
        if lens[b] < 0 or lens[b] > host.shape[1]:
            raise L.VauraHipError(f"lengths must lie in 0 .. {host.shape[1]} (the frames of clip {b}), got {lens}")
        data = host[b, :lens[b]].contiguous().numpy()
        wavfile.write(path, fmt.rate, data[:, 0] if fmt.channels == 1 else data)


# ------------------------------------------------------------------------------------------------ spectrograms, one column per frame
class SpectrogramFormat:
    """Which picture of the audio: ``n_fft`` 512 / 1024 / 2048 samples per window, ``hop`` (a power of two, at most ``n_fft``; 512 is
    the codec's hop: one column per codec frame), ``n_mels`` triangular mel bands between ``f_min`` and ``f_max`` Hz (None: the Nyquist
    frequency) on the ``mel_scale`` "slaney" or "htk" with ``norm`` None or "slaney" — or ``n_mels=None``: the ``n_fft/2 + 1`` linear
    bins — and the ``scale``: "power", "db" (``10 log10(max(v, amin))``) or "log" (``ln(max(v, amin))``); with ``n_mels=None`` also
    "complex": the transform itself, a last axis of (re, im).  ``top_db`` is not served:
    it needs the maximum of the whole clip, which a stream does not have.  Refused here: sizes the kernel refuses, and a filterbank in
    which a filter has no non-zero weight (too many bands for the bins of ``n_fft``)."""

    def __init__(self, n_fft: int = 2048, hop: int = 512, n_mels: Optional[int] = 128, f_min: float = 0.0, f_max: Optional[float] = None,
                 mel_scale: str = "slaney", norm: Optional[str] = None, scale: str = "db", amin: float = 1e-10, top_db=None):
        if top_db is not None:
            raise L.VauraHipError("top_db is not served: it needs the maximum of the whole clip, which a stream does not have; "
                                  "clamp the result yourself once the clip is complete")
        self.plan = SG.SpectrogramPlan(n_fft, hop)
        if scale not in SG.SCALES:
            raise L.VauraHipError(f"VAURA_ERR_DTYPE: scale must be one of {sorted(SG.SCALES)}, got {scale!r}")
        if isinstance(amin, bool) or not isinstance(amin, (int, float)) or not float(amin) > 0.0:
            raise L.VauraHipError(f"amin must be a positive number, got {amin!r}")
        if scale == "complex" and n_mels is not None:
            raise L.VauraHipError('scale "complex" is the linear spectrum itself: it goes with n_mels=None')
        self.n_fft, self.hop, self.n_mels, self.f_min, self.f_max = n_fft, hop, n_mels, float(f_min), f_max
        self.mel_scale, self.norm, self.scale, self.amin = mel_scale, norm, scale, float(amin)
        self.mel = None if n_mels is None else SG.mel_table(n_fft, n_mels, f_min, f_max, mel_scale, norm)
        self.bins = n_fft // 2 + 1 if n_mels is None else n_mels         # F: the values of one column

    def key(self):
        return (self.n_fft, self.n_mels, self.f_min, self.f_max, self.mel_scale, self.norm)

    def __repr__(self):
        return (f"SpectrogramFormat(n_fft={self.n_fft}, hop={self.hop}, n_mels={self.n_mels}, f_min={self.f_min}, f_max={self.f_max}, "
                f"mel_scale={self.mel_scale!r}, norm={self.norm!r}, scale={self.scale!r}, amin={self.amin})")


_spec_tables: Dict[Tuple[tuple, str], tuple] = {}
_spec_rings: Dict[Tuple[int, str], _RecordRing] = {}


def _spec_table(fmt: SpectrogramFormat, dev: torch.device):
    """(window, twiddles, mel bins, mel weights) of a format on a device, built once"""
    key = (fmt.key(), str(dev))
    if key not in _spec_tables:
        if len(_spec_tables) >= 16:
            _spec_tables.clear()
        mel = (None, None) if fmt.mel is None else (fmt.mel["bins"].to(dev), fmt.mel["weights"].to(dev))
        _spec_tables[key] = (SG.window(fmt.n_fft).to(dev), SG.twiddles(fmt.n_fft).to(dev), *mel)
    return _spec_tables[key]


def _spec_launch(fmt: SpectrogramFormat, x: torch.Tensor, in_stride: int, records: List[List[int]], carry_in: Optional[torch.Tensor],
                 carry_out: Optional[torch.Tensor], n_row: int, ring: Optional[_RecordRing] = None) -> torch.Tensor:
    """One launch of vaura_spectrogram over ``x`` (B rows of ``in_stride`` fp32 samples on a HIP device) -> (B, n_row, F) fp32.  The
    records travel by one asynchronous copy from a pinned buffer of ``ring``; nothing here waits for the device."""
    dev, B = x.device, len(records)
    if not x.is_cuda:
        raise L.VauraHipError("the spectrogram runs on the HIP device that holds the decoded waveform; there is no CPU path")
    lib = L.lib()
    with torch.cuda.device(dev):
        win, tw, bins, weights = _spec_table(fmt, dev)
        if ring is None:
            ring = _spec_rings.setdefault((B, str(dev)), _RecordRing(B))
        rec = ring.send(records, dev)
        out = torch.empty((B, n_row, fmt.bins) + ((2,) if fmt.scale == "complex" else ()), dtype=torch.float32, device=dev)
        history = 0 if carry_in is None else carry_in.shape[-1]
        L.check(lib.vaura_spectrogram(L.ptr(x), B, in_stride, L.ptr(rec), L.ptr(carry_in), L.ptr(carry_out), history, fmt.n_fft, fmt.hop,
                                      L.ptr(win), L.ptr(tw), L.ptr(bins), L.ptr(weights), 0 if weights is None else weights.numel(),
                                      fmt.bins, SG.SCALES[fmt.scale], fmt.amin, L.ptr(out) if n_row else 0, n_row,
                                      L.current_stream(dev)), "vaura_spectrogram")
    return out


def audio_to_spectrogram(wav: torch.Tensor, fmt: SpectrogramFormat, lengths=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """wav (B, 1, N) fp32 at 44.1 kHz on a HIP device -> (spec, columns): ``spec`` (B, max(columns), F) fp32 on the same device,
    time-major — row t is column t, centred on sample ``hop t + hop/2``; ``spec.transpose(1, 2)`` is torchaudio's (B, F, time) layout —
    and ``columns`` (B,) int64 on the host, ``ceil(n_b / hop)``.  ``lengths`` (the "audio_lengths" of a ragged ``generate()``): clip b is
    exactly the clip converted alone at its own length, zero rows follow it, and nothing behind ``lengths[b]`` is read."""
    x = _mono_rows(wav, "audio_to_spectrogram")
    B, N = x.shape[0], x.shape[-1]
    if N < 1:
        raise L.VauraHipError(f"a waveform of shape {tuple(wav.shape)} holds no samples")
    if lengths is None:
        n_in = [N] * B
    else:
        if not clip_params.is_per_clip(lengths):
            raise L.VauraHipError(f"lengths must be one integer per clip (a list, tuple or 1-D tensor), got {lengths!r}")
        n_in = clip_params._int_list("lengths", lengths)
        if len(n_in) != B:
            raise L.VauraHipError(f"per-clip lengths has {len(n_in)} values for a batch of {B} clips")
        if min(n_in) < 1 or max(n_in) > N:
            raise L.VauraHipError(f"lengths must lie in 1 .. {N} (the samples of a row), got {n_in}")
    cols = [fmt.plan.columns(n) for n in n_in]
    records = [[0, n, 0, c, n] for n, c in zip(n_in, cols)]              # the stream's one and last block, from its start
    return _spec_launch(fmt, x, N, records, None, None, max(cols)), torch.tensor(cols, dtype=torch.int64)


class SpectrogramStream:
    """``audio_to_spectrogram`` block by block: ``push`` takes the next samples of every clip and returns the columns whose window is
    complete.  The pushes concatenated per clip are bit for bit ``audio_to_spectrogram`` of the whole clips.  State: two integers per
    clip on the host (samples received, columns emitted) and a ping-pong pair of carry rows on the device (``n_fft - 1`` samples per
    clip).  One push is one launch and one asynchronous copy of a (B, 5) record from a pinned buffer the stream keeps; nothing waits
    for the device."""

    def __init__(self, fmt: SpectrogramFormat, batch: int, device):
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            raise L.VauraHipError(f"SpectrogramStream takes a batch of at least one clip, got {batch!r}")
        self.fmt, self.batch, self.device = fmt, batch, torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.received, self.emitted, self.finished = [0] * batch, [0] * batch, [False] * batch
        self._carry = torch.zeros(2, batch, fmt.plan.history(), dtype=torch.float32, device=self.device)
        self._cur = 0
        self._ring = _RecordRing(batch)
        self._empty = torch.zeros(batch, 1, 1, dtype=torch.float32, device=self.device)

    _per_clip = PcmStream._per_clip

    def push(self, audio: Optional[torch.Tensor], samples=None, final=False) -> Tuple[torch.Tensor, List[int]]:
        """audio (B, 1, n) fp32 on the stream's device: the next ``samples[b]`` samples of clip b (default: all n; 0 is allowed, and
        ``audio`` may be None when every clip gives 0) -> (spec (B, max(counts), F), counts): clip b's next ``counts[b]`` columns, zero
        rows behind them.  A column leaves once the last sample of its window is there; ``final`` (a bool, or one per clip) flushes the
        clip's remaining columns up to ``ceil(received / hop)``, their windows zero-padded; a finished clip takes no more samples."""
        if audio is None:
            x, n = self._empty, 0
        else:
            x = _mono_rows(audio, "SpectrogramStream.push")
            n = x.shape[-1]
            if x.shape[0] != self.batch or x.device != self.device:
                raise L.VauraHipError(f"SpectrogramStream of {self.batch} clips on {self.device}: got a block of shape "
                                      f"{tuple(audio.shape)} on {x.device}")
            if n == 0:
                x = self._empty
        counts_in = [n] * self.batch if samples is None else self._per_clip("samples", samples, int)
        fin = self._per_clip("final", final, bool)
        if min(counts_in) < 0 or max(counts_in) > n:
            raise L.VauraHipError(f"samples must lie in 0 .. {n} (the samples of a block's row), got {counts_in}")
        for b in range(self.batch):
            if self.finished[b] and counts_in[b]:
                raise L.VauraHipError(f"clip {b} of the stream was flushed (final) and takes no more samples; got {counts_in[b]}")
        records, received, emitted = SG.push_records(self.fmt.plan, self.received, self.emitted, counts_in, fin)
        counts = [r[3] for r in records]
        spec = _spec_launch(self.fmt, x, max(n, 1), records, self._carry[self._cur], self._carry[1 - self._cur], max(counts),
                            ring=self._ring)
        self._cur = 1 - self._cur
        self.received, self.emitted = received, emitted
        self.finished = [a or b for a, b in zip(self.finished, fin)]
        return spec, counts


def stream_spectrogram(blocks: Iterable[dict], fmt: SpectrogramFormat) -> Iterator[dict]:
    """Wrap a streaming generator (``generate_stream``, ``generate_long_stream`` with or without ``block_frames``,
    ``generate_long_clips_stream``) or the blocks of a live session: every dict comes back with "spectrogram" ((B, max columns, F):
    the columns that became complete with this block), "spec_start" and "spec_columns" (one int per clip: the first column's index in
    the clip and how many there are) added; every other key passes through, so it composes with ``stream_pcm`` in either order.  A
    column waits for the last sample of its window, ``(n_fft - hop) / 2`` samples beyond its frame; the dict whose "final" is true
    carries every clip's remaining columns.  At hop 512 a clip's columns are its frames."""
    stream = None
    for blk in blocks:
        audio = blk["audio"]
        B = audio.shape[0]
        frames = blk["frames"]
        frames = [int(f) for f in frames] if isinstance(frames, (list, tuple)) else [int(frames)] * B
        hop = audio.shape[-1] // max(frames) if max(frames) > 0 else 0
        if stream is None:
            stream = SpectrogramStream(fmt, B, audio.device)
        start = list(stream.emitted)
        spec, counts = stream.push(audio, [f * hop for f in frames], final=bool(blk["final"]))
        out = dict(blk)
        out.update(spectrogram=spec, spec_start=start, spec_columns=counts)
        yield out


# ------------------------------------------------------------------------------------------------ loudness: a meter and a causal normaliser
def _number(name, v, lo=None, hi=None) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), float("-inf")):
        raise L.VauraHipError(f"{name} must be a finite number, got {v!r}")
    if (lo is not None and v < lo) or (hi is not None and v > hi):
        raise L.VauraHipError(f"{name} must lie in {lo} .. {hi}, got {v!r}")
    return float(v)


class LoudnessTarget:
    """Where a causal normaliser steers: ``target_lkfs`` (the integrated loudness aimed at; -12 is ``normalize_audio``'s
    ``loudness_headroom_db``), ``max_gain_db`` (the clamp on the correction, either way), ``slew_db_per_s`` (None: unlimited; else the most
    the correction moves per second), ``initial_gain_db`` (the gain before the first integrated value exists), ``limiter`` "clip"
    (``_clip_wav``) or "tanh" (``tanhf`` then the clip: the reference's ``loudness_compressor``), ``sample_rate`` and ``history_steps``
    (8 .. 4096: the 100 ms steps the integrated loudness looks back over; the state of a stream does not grow with the audio).  Refused
    here: a rate the meter refuses (outside 8 .. 48 kHz, or 11 025 Hz, whose gating block is not four whole steps), a history outside
    its range, a non-finite or out-of-range number, another limiter."""

    def __init__(self, target_lkfs: float = -12.0, max_gain_db: float = 20.0, slew_db_per_s: Optional[float] = None,
                 initial_gain_db: float = 0.0, limiter: str = "clip", sample_rate: int = 44100, history_steps: int = LD.MAX_HISTORY):
        self.plan = LD.LoudnessPlan(sample_rate)                          # raises for rates the meter refuses
        self.history_steps = LD.check_history(history_steps)
        self.target_lkfs = _number("target_lkfs", target_lkfs, -70.0, 0.0)
        self.max_gain_db = _number("max_gain_db", max_gain_db, 0.0, 80.0)
        self.initial_gain_db = _number("initial_gain_db", initial_gain_db, -80.0, 80.0)
        self.slew_db_per_s = None if slew_db_per_s is None else _number("slew_db_per_s", slew_db_per_s, 1e-3, 1e6)
        if limiter not in LD.LIMITERS:
            raise L.VauraHipError(f"VAURA_ERR_DTYPE: limiter must be one of {sorted(LD.LIMITERS)}, got {limiter!r}")
        self.limiter, self.sample_rate = limiter, sample_rate

    def __repr__(self):
        return (f"LoudnessTarget(target_lkfs={self.target_lkfs}, max_gain_db={self.max_gain_db}, slew_db_per_s={self.slew_db_per_s}, "
                f"initial_gain_db={self.initial_gain_db}, limiter={self.limiter!r}, sample_rate={self.sample_rate}, "
                f"history_steps={self.history_steps})")


_loud_tables: Dict[Tuple[int, str], torch.Tensor] = {}


def _loud_table(pl: LD.LoudnessPlan, dev: torch.device) -> torch.Tensor:
    """the fp64 chunk table of a rate on a device, built once"""
    key = (pl.rate, str(dev))
    if key not in _loud_tables:
        _loud_tables[key] = torch.from_numpy(pl.table()).to(dev)
    return _loud_tables[key]


class LoudnessStream:
    """The causal normaliser block by block: ``push`` takes the next samples of every clip and returns them normalised — all of them:
    the gain at a sample depends only on the 100 ms steps completed before it, so nothing is held back and ``final`` has no tail to
    flush.  The pushes concatenated per clip are bit for bit ``normalize_loudness_causal`` of the whole clips.  State: one integer per
    clip on the host (samples received) and one buffer on the device (per clip the filter state in fp64, the current gains, a ring of
    ``max(history_steps, 32)`` step energies and the raw tail shorter than one step): it does not grow with the audio.  One push is
    one launch (two above 16384 samples a row), one asynchronous copy of a (B, 2) record from a pinned buffer the stream keeps and two
    allocations (the samples; everything else the launch writes); nothing waits for the device."""

    def __init__(self, target: LoudnessTarget, batch: int, device):
        if not isinstance(target, LoudnessTarget):
            raise L.VauraHipError(f"LoudnessStream takes a LoudnessTarget, got {type(target).__name__}")
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            raise L.VauraHipError(f"LoudnessStream takes a batch of at least one clip, got {batch!r}")
        self.target, self.batch, self.device = target, batch, torch.device(device)
        if self.device.type != "cuda":
            raise L.VauraHipError("the loudness meter runs on the HIP device that holds the decoded waveform; there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.received, self.finished = [0] * batch, [False] * batch
        words = L.lib().vaura_audio_loudness_state_elems(batch, target.sample_rate, target.history_steps)
        self._state = torch.empty(words, dtype=torch.float32, device=self.device)      # a clip's first push reads none of it
        self._clipped = torch.zeros(batch, dtype=torch.int32, device=self.device)
        self._ring = _RecordRing(batch, LD.RECORD)
        self._empty = torch.zeros(batch, 1, 1, dtype=torch.float32, device=self.device)

    _per_clip = PcmStream._per_clip

    def push(self, audio: Optional[torch.Tensor], samples=None, final=False, _meter_only: bool = False) -> Tuple[torch.Tensor, dict]:
        """audio (B, 1, n) fp32 on the stream's device: the next ``samples[b]`` samples of clip b (default: all n; 0 is allowed, and
        ``audio`` may be None when every clip gives 0) -> (out (B, 1, n): clip b's ``samples[b]`` normalised samples, zeros behind them,
        info).  ``info``: "gain_db" and "integrated" ((B,) fp32 on the device: the correction and the integrated loudness at the clip's
        last 100 ms boundary, NaN while undefined), "momentary" ((B, max blocks) fp32: the momentary loudness of the 400 ms blocks this
        push completed, NaN behind them) with "blocks" (how many per clip), "short_term" / "windows" likewise for the 3 s windows,
        "integrated_steps" ((B, max boundaries): the integrated loudness at every boundary the push reached) with "boundaries", and
        "clipped" ((B,) int32: the samples so far with |x g| > 1 — the stream's own running counter, the same tensor in every push's
        info: clone it to keep a block's figure).  ``final`` (a bool, or one per clip) only closes the clip: a
        finished clip takes no more samples."""
        if audio is None:
            x, n = self._empty, 0
        else:
            x = _mono_rows(audio, "LoudnessStream.push")
            n = x.shape[-1]
            if x.shape[0] != self.batch or x.device != self.device:
                raise L.VauraHipError(f"LoudnessStream of {self.batch} clips on {self.device}: got a block of shape {tuple(audio.shape)} "
                                      f"on {x.device}")
            if n == 0:
                x = self._empty
        counts = [n] * self.batch if samples is None else self._per_clip("samples", samples, int)
        fin = self._per_clip("final", final, bool)
        if min(counts) < 0 or max(counts) > n:
            raise L.VauraHipError(f"samples must lie in 0 .. {n} (the samples of a block's row), got {counts}")
        for b in range(self.batch):
            if self.finished[b] and counts[b]:
                raise L.VauraHipError(f"clip {b} of the stream was closed (final) and takes no more samples; got {counts[b]}")
        t, dev, B = self.target, self.device, self.batch
        rec = LD.push_records(t.plan, self.received, counts)
        stride = rec["stride"]
        with torch.cuda.device(dev):
            records = self._ring.send(rec["records"], dev)
            out = None if _meter_only else torch.empty_like(x)
            # one buffer per push for everything the launch writes beside the samples: gains (B, stride + 2), meter (3, B, stride), info (B, 2)
            work = torch.empty(B * (stride + 2) + 3 * B * stride + 2 * B, dtype=torch.float32, device=dev)
            gains = work[:B * (stride + 2)]
            meter = work[B * (stride + 2):B * (stride + 2) + 3 * B * stride].view(3, B, stride)
            info = work[B * (stride + 2) + 3 * B * stride:].view(B, 2)
            table = _loud_table(t.plan, dev)
            slew = 0.0 if t.slew_db_per_s is None else 0.1 * t.slew_db_per_s
            L.check(L.lib().vaura_audio_loudness_push(L.ptr(x), L.ptr(out), B, x.shape[-1], L.ptr(records), L.ptr(self._state),
                                                      t.sample_rate, t.history_steps, L.ptr(table), table.numel(), t.target_lkfs,
                                                      t.max_gain_db, slew, t.initial_gain_db, LD.LIMITERS[t.limiter], L.ptr(gains),
                                                      L.ptr(meter), stride, L.ptr(info), L.ptr(self._clipped), L.current_stream(dev)),
                    "vaura_audio_loudness_push")                  # (the launch adds to the stream's own clipped counter)
        self.received = rec["received"]
        self.finished = [a or b for a, b in zip(self.finished, fin)]
        if out is not None and n == 0:
            out = out[:, :, :0]
        return out, {"gain_db": info[:, 0], "integrated": info[:, 1], "momentary": meter[1, :, :max(rec["blocks"])],
                     "blocks": rec["blocks"], "short_term": meter[2, :, :max(rec["windows"])], "windows": rec["windows"],
                     "integrated_steps": meter[0, :, :max(rec["boundaries"])], "boundaries": rec["boundaries"],
                     "clipped": self._clipped}


def _loud_lengths(x: torch.Tensor, lengths) -> List[int]:
    B, N = x.shape[0], x.shape[-1]
    if N < 1:
        raise L.VauraHipError(f"a waveform of shape {tuple(x.shape)} holds no samples")
    if lengths is None:
        return [N] * B
    if not clip_params.is_per_clip(lengths):
        raise L.VauraHipError(f"lengths must be one integer per clip (a list, tuple or 1-D tensor), got {lengths!r}")
    n_in = clip_params._int_list("lengths", lengths)
    if len(n_in) != B:
        raise L.VauraHipError(f"per-clip lengths has {len(n_in)} values for a batch of {B} clips")
    if min(n_in) < 1 or max(n_in) > N:
        raise L.VauraHipError(f"lengths must lie in 1 .. {N} (the samples of a row), got {n_in}")
    return n_in


def normalize_loudness_causal(wav: torch.Tensor, target: LoudnessTarget, lengths=None) -> Tuple[torch.Tensor, dict]:
    """wav (B, 1, N) fp32 on a HIP device -> (out, info): what a ``LoudnessStream`` of ``target`` returns for the clips, whole: sample i
    of a clip is scaled by a gain that follows the integrated loudness of the 100 ms steps completed before i towards ``target_lkfs``
    (``LoudnessStream.push`` names the entries of ``info``).  ``lengths`` (the "audio_lengths" of a ragged ``generate()``): clip b is
    exactly the clip normalised alone at its own length, zeros follow it, and nothing behind ``lengths[b]`` is read."""
    x = _mono_rows(wav, "normalize_loudness_causal")
    n_in = _loud_lengths(x, lengths)
    if not x.is_cuda:
        raise L.VauraHipError("the loudness meter runs on the HIP device that holds the decoded waveform; there is no CPU path")
    return LoudnessStream(target, x.shape[0], x.device).push(x, samples=n_in, final=True)


def measure_loudness(wav: torch.Tensor, lengths=None, sample_rate: int = 44100, history_steps: int = LD.MAX_HISTORY) -> dict:
    """wav (B, 1, N) fp32 on a HIP device -> {"integrated" (B,): the integrated loudness in LKFS at each clip's last 100 ms boundary,
    over the blocks of its last ``history_steps`` steps; "momentary" (B, max blocks): one value per 400 ms block, every 100 ms;
    "short_term" (B, max windows): the same over 3 s; "blocks" (per clip, on the host); "windows"; "step" (samples per 100 ms)}, fp32 on
    the device, NaN where undefined (a clip shorter than one block, no block above the gates) and behind a clip's values."""
    x = _mono_rows(wav, "measure_loudness")
    n_in = _loud_lengths(x, lengths)
    target = LoudnessTarget(sample_rate=sample_rate, history_steps=history_steps)
    if not x.is_cuda:
        raise L.VauraHipError("the loudness meter runs on the HIP device that holds the decoded waveform; there is no CPU path")
    _, info = LoudnessStream(target, x.shape[0], x.device).push(x, samples=n_in, final=True, _meter_only=True)
    return {"integrated": info["integrated"], "momentary": info["momentary"], "short_term": info["short_term"],
            "blocks": info["blocks"], "windows": info["windows"], "step": target.plan.step}


def stream_loudness(blocks: Iterable[dict], target: LoudnessTarget) -> Iterator[dict]:
    """Wrap a streaming generator (``generate_stream``, ``generate_long_stream`` with or without ``block_frames``,
    ``generate_long_clips_stream``) or the blocks of a live session: every dict comes back with "audio" replaced by the normalised
    block and "loudness_gain_db", "loudness_integrated", "loudness_momentary", "loudness_blocks", "loudness_short_term",
    "loudness_windows" and "loudness_clipped" (the stream's running counter: one tensor for all blocks) added (the
    entries of ``LoudnessStream.push``'s info); every other key passes through, so ``stream_pcm`` and ``stream_spectrogram`` compose on
    top.  No sample is held back: a block's audio is the block's audio."""
    stream = None
    for blk in blocks:
        audio = blk["audio"]
        B = audio.shape[0]
        frames = blk["frames"]
        frames = [int(f) for f in frames] if isinstance(frames, (list, tuple)) else [int(frames)] * B
        hop = audio.shape[-1] // max(frames) if max(frames) > 0 else 0
        if stream is None:
            stream = LoudnessStream(target, B, audio.device)
        norm, info = stream.push(audio, [f * hop for f in frames], final=bool(blk["final"]))
        out = dict(blk)
        out.update(audio=norm.reshape(audio.shape), loudness_gain_db=info["gain_db"], loudness_integrated=info["integrated"],
                   loudness_momentary=info["momentary"], loudness_blocks=info["blocks"], loudness_short_term=info["short_term"],
                   loudness_windows=info["windows"], loudness_clipped=info["clipped"])
        yield out
