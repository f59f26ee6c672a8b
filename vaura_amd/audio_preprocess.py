"""Audio preprocessing on the device: decoded PCM -> the codec's mono 44.1 kHz input.

What the reference's data loader does on the CPU with the ``audio_transforms_test`` list of configs/generate_vas.yaml:43-54 and
data/demo/dataloader_config.yaml:13-20 (classes in models/data/transforms/audio_transforms.py:162-192):

    AudioStereoToMono -> AudioResample(44100) -> AudioTrim

runs here as one launch of ``vaura_audio_preprocess`` (csrc/audio_pre.hip) per call: one source rate, one channel count and one
sample format per call, per-clip sample counts ``n_b``.

Arithmetic.
  1. to float: int16 is ``x / 32768`` (exact in fp32), int32 ``x / 2147483648``, float32 as is;
  2. mono: the channels added in channel order in fp32, then divided by C (``wav.mean(dim=0, keepdim=True)``);
  3. resample ``orig -> new``: ``AudioResample`` is ``torchaudio.transforms.Resample`` at its defaults (``sinc_interp_hann``,
     ``lowpass_filter_width = 6``, ``rolloff = 0.99``).  With ``g = gcd(orig, new)``, ``o = orig / g``, ``n = new / g``,
     ``base = min(o, n) * 0.99`` and ``w = ceil(6 o / base)``, phase ``p`` in [0, n) has the ``2 w + o`` taps
         t = clamp(((j - w) / o - p / n) * base, -6, 6);    k[p][j] = sinc(pi t) * cos^2(pi t / 12) * base / o
     (float64, then rounded to fp32), output sample ``m = q n + p`` is ``sum_j k[p][j] x[q o + j - w]`` with ``x = 0`` outside
     [0, n_b), and the output has ``ceil(n n_b / o)`` samples (integers).  ``orig == new`` is the mono signal unchanged;
  4. trim to ``ceil(duration * target_sr)`` samples when a duration is given;
  5. zeros from the clip's output length to the row's end.
The window clamps to zero outside |t| < 6: of a phase's ``2 w + o`` taps only one contiguous run of at most
``floor(12 o / base) + 1`` is non-zero, and every tap outside it is below 1.5e-49 in float64 — exactly 0 in fp32.  ``resample_table``
builds ``first[p]`` plus that run only (2 058 entries for 48 kHz, where the full form has 25 578; the full form of 44 101 Hz would have
1.9 G entries and is never built).  The data loader's own source rate is ``int(N / clip_duration)``; ``__call__`` takes either.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as Fn

from . import _lib as L
from . import clip_params

TILE = 1024                         # VAURA_AUDIO_PRE_TILE (include/vaura_hip.h): output samples per workgroup
MAX_TAPS = 64                       # VAURA_AUDIO_PRE_MAX_TAPS
MAX_TABLE = 1 << 20                 # table entries (phases x taps per phase)
MAX_CHANNELS = 8
MAX_ROW = (1 << 31) - 1
LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99
_FULL_FORM_LIMIT = 1 << 22          # reference(): the full-form conv1d below this many taps, the gathered run above

PCM_S16, PCM_S32, PCM_F32 = 0, 1, 2   # VAURA_PCM_*
_FORMATS = {torch.int16: PCM_S16, torch.int32: PCM_S32, torch.float32: PCM_F32}

_MONO = "models.data.transforms.audio_transforms.AudioStereoToMono"
_RESAMPLE = "models.data.transforms.audio_transforms.AudioResample"
_TRIM = "models.data.transforms.audio_transforms.AudioTrim"


def rate_ratio(orig: int, new: int) -> Tuple[int, int, int]:
    """(o, n, w) of a rate pair: both rates over their gcd and the half width of the full form."""
    orig, new = int(orig), int(new)
    if orig < 1 or new < 1:
        raise L.VauraHipError(f"sample rates must be positive integers, got {orig} -> {new}")
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    return o, n, int(math.ceil(LOWPASS_FILTER_WIDTH * o / (min(o, n) * ROLLOFF)))


def tap_values(j: torch.Tensor, p: torch.Tensor, o: int, n: int, w: int) -> torch.Tensor:
    """k[p][j] in float64 for broadcastable int64 tensors of tap and phase indices."""
    base = min(o, n) * ROLLOFF
    t = ((j - w).to(torch.float64) / o - p.to(torch.float64) / n) * base
    t = t.clamp(-LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    window = torch.cos(t * math.pi / LOWPASS_FILTER_WIDTH / 2) ** 2
    t = t * math.pi
    return torch.where(t == 0, torch.ones_like(t), t.sin() / t) * (window * (base / o))


def resample_table(orig: int, new: int) -> dict:
    """The fp32 taps of ``Resample(orig, new)`` with the exact zeros removed.

    Returns ``o``, ``n``, ``w``, ``taps`` (T, the longest run), ``first`` (n,) int32 — the index of phase p's first non-zero tap among
    the ``2 w + o`` of the full form — ``weights`` (n, T) fp32 and ``weights_f64`` (n, T): taps ``first[p] .. first[p] + T`` (zeros behind
    a shorter run, and behind tap ``2 w + o``).  Only the candidates around each phase's centre are ever computed.  Refused (the
    kernel's VAURA_ERR_SHAPE, here before anything is built): more than 64 taps per phase, more than 2^20 entries."""
    o, n, w = rate_ratio(orig, new)
    if o == n:
        raise L.VauraHipError(f"{orig} -> {new} Hz is the identity: there is no table")
    half = LOWPASS_FILTER_WIDTH * o / (min(o, n) * ROLLOFF)
    bound = int(math.floor(2 * half)) + 1                                # the longest run there can be
    if bound - 2 > MAX_TAPS:
        raise L.VauraHipError(f"VAURA_ERR_SHAPE: {orig} -> {new} Hz needs about {bound} taps per phase; the kernel is compiled for at "
                              f"most {MAX_TAPS}")
    if n * max(bound - 2, 1) > MAX_TABLE:
        raise L.VauraHipError(f"VAURA_ERR_SHAPE: {orig} -> {new} Hz needs {n} phases of about {bound} taps; the table holds at most "
                              f"{MAX_TABLE} entries")
    K = bound + 4                                                        # candidates per phase: the run and two on either side
    p = torch.arange(n, dtype=torch.int64)[:, None]
    j0 = torch.floor(w + torch.arange(n, dtype=torch.float64) * o / n - half).to(torch.int64)[:, None] - 1
    j = j0 + torch.arange(K, dtype=torch.int64)[None, :]
    inside = (j >= 0) & (j < 2 * w + o)                                   # the full form has no other taps
    k64 = torch.where(inside, tap_values(j, p, o, n, w), torch.zeros((), dtype=torch.float64))
    nz = k64.to(torch.float32) != 0
    if not bool(nz.any(dim=1).all()):
        raise L.VauraHipError(f"{orig} -> {new} Hz: a phase without a non-zero tap")
    cols = torch.arange(K)[None, :]
    lead = torch.where(nz, cols, torch.full_like(cols, K)).amin(dim=1)    # first / last non-zero candidate of each phase
    last = torch.where(nz, cols, torch.full_like(cols, -1)).amax(dim=1)
    if bool(((nz[:, 0] & (j[:, 0] > 0)) | (nz[:, -1] & (j[:, -1] < 2 * w + o - 1))).any()):   # the run must end inside the candidates
        raise L.VauraHipError(f"{orig} -> {new} Hz: a non-zero tap at the edge of the candidate window")
    T = int((last - lead).max()) + 1
    if T > MAX_TAPS:
        raise L.VauraHipError(f"VAURA_ERR_SHAPE: {orig} -> {new} Hz needs {T} taps per phase; the kernel is compiled for at most {MAX_TAPS}")
    if n * T > MAX_TABLE:
        raise L.VauraHipError(f"VAURA_ERR_SHAPE: {orig} -> {new} Hz needs {n} x {T} = {n * T} table entries; at most {MAX_TABLE}")
    take = (lead[:, None] + torch.arange(T)[None, :]).clamp(max=K - 1)
    keep = (lead[:, None] + torch.arange(T)[None, :]) <= last[:, None]
    w64 = torch.where(keep, k64.gather(1, take), torch.zeros((), dtype=torch.float64))
    return {"o": o, "n": n, "w": w, "taps": T, "first": (j0[:, 0] + lead).to(torch.int32), "weights": w64.to(torch.float32),
            "weights_f64": w64}


def output_length(n_samples: int, orig: int, new: int, duration: Optional[float] = None, target_sr: Optional[int] = None) -> int:
    """Samples a clip of ``n_samples`` has after Resample(orig, new) (``ceil(n n_b / o)``, integers) and AudioTrim(duration, target_sr)
    (``ceil(duration * target_sr)``; ``target_sr`` defaults to ``new``)."""
    o, n, _ = rate_ratio(orig, new)
    length = int(n_samples) if o == n else (n * int(n_samples) + o - 1) // o
    if duration is not None:
        length = min(length, int(math.ceil(duration * (new if target_sr is None else target_sr))))
    return length


class AudioPreprocessor:
    def __init__(self, target_sr: int = 44100, duration: Optional[float] = None, clip_duration: Optional[float] = None,
                 device: Union[str, torch.device, None] = None):
        self.target_sr = int(target_sr)
        self.duration = None if duration is None else float(duration)
        self.clip_duration = None if clip_duration is None else float(clip_duration)   # AudioResample's own rule for the source rate
        if self.target_sr < 1 or (self.duration is not None and self.duration <= 0) or (self.clip_duration is not None and self.clip_duration <= 0):
            raise L.VauraHipError(f"AudioPreprocessor(target_sr={target_sr}, duration={duration}, clip_duration={clip_duration}): positive values only")
        self.device = None if device is None else torch.device(device)
        self._tables: Dict[int, dict] = {}
        self._dev: Dict[Tuple[int, str], tuple] = {}
        self._len_dev: Dict[tuple, tuple] = {}

    # ---- configuration
    @classmethod
    def from_transforms_config(cls, transforms: Sequence[dict], **kw) -> "AudioPreprocessor":
        """From the reference's ``audio_transforms_test`` list (configs/generate_vas.yaml:43-54) as plain data, interpolations resolved."""
        seen: List[str] = []
        for entry in transforms:
            target = entry.get("target") if hasattr(entry, "get") else None
            params = dict(entry.get("params", None) or {}) if target is not None else {}
            if target == _MONO:
                if not params.get("keepdim", True):
                    raise L.VauraHipError(f"{_MONO} with keepdim=false drops the channel axis the codec input has")
            elif target == _RESAMPLE:
                kw["target_sr"] = int(params["target_sr"])
                if params.get("clip_duration") is not None:
                    kw["clip_duration"] = float(params["clip_duration"])
            elif target == _TRIM:
                kw["duration"] = float(params["duration"])
                if int(params.get("sr", kw.get("target_sr", 44100))) != kw.get("target_sr", 44100):
                    raise L.VauraHipError(f"{_TRIM}: sr {params['sr']} is not the resampler's target_sr {kw.get('target_sr', 44100)}")
            else:
                raise L.VauraHipError(f"audio transform {target!r} is not built; AudioPreprocessor takes AudioStereoToMono, AudioResample "
                                      "and AudioTrim")
            seen.append(target)
        if seen not in ([_MONO, _RESAMPLE], [_MONO, _RESAMPLE, _TRIM]):
            raise L.VauraHipError("audio transforms must be AudioStereoToMono -> AudioResample -> AudioTrim, in that order; got "
                                  f"{[str(t).rsplit('.', 1)[-1] for t in seen]}")
        return cls(**kw)

    def table(self, orig: int) -> dict:
        if orig not in self._tables:
            self._tables[orig] = resample_table(orig, self.target_sr)
        return self._tables[orig]

    def output_length(self, n_samples: int, orig: int) -> int:
        return output_length(n_samples, orig, self.target_sr, self.duration)

    # ---- input handling
    def _plan(self, pcm, sample_rate, clip_duration, lengths, interleaved):
        """-> (pcm (B, C, N) or (B, N, C), B, C, N, orig, [n_b], [output length of clip b]); every refusal happens here."""
        if not torch.is_tensor(pcm):
            raise L.VauraHipError(f"AudioPreprocessor takes a tensor of decoded PCM, got {type(pcm).__name__}")
        if pcm.dtype not in _FORMATS:
            raise L.VauraHipError(f"VAURA_ERR_DTYPE: decoded PCM is int16, int32 or float32; got {pcm.dtype}")
        if pcm.dim() == 2:
            pcm = pcm[None]
        if pcm.dim() != 3:
            raise L.VauraHipError(f"pcm must be (B, C, N) or (C, N) (interleaved: (B, N, C) or (N, C)); got {tuple(pcm.shape)}")
        B, C, N = (pcm.shape[0], pcm.shape[2], pcm.shape[1]) if interleaved else tuple(pcm.shape)
        if B < 1 or C < 1 or N < 1:
            raise L.VauraHipError(f"pcm of shape {tuple(pcm.shape)} holds no samples")
        if C > MAX_CHANNELS:
            raise L.VauraHipError(f"VAURA_ERR_SHAPE: {C} channels ({'interleaved' if interleaved else 'planar'} layout expected); at most {MAX_CHANNELS}")
        if N > MAX_ROW:
            raise L.VauraHipError(f"VAURA_ERR_SHAPE: rows of {N} samples; at most {MAX_ROW}")
        if sample_rate is not None and clip_duration is not None:
            raise L.VauraHipError("give the source rate as sample_rate or as clip_duration (orig = int(N / clip_duration)), not both")
        if sample_rate is None and clip_duration is None:
            clip_duration = self.clip_duration
        if sample_rate is not None:
            orig = int(sample_rate)
        elif clip_duration is not None:
            if lengths is not None:
                raise L.VauraHipError("clip_duration states the rate of rows that are whole clips; with per-clip lengths give sample_rate")
            orig = int(N / float(clip_duration))
        else:
            raise L.VauraHipError("the source rate is needed: sample_rate, or clip_duration for orig = int(N / clip_duration)")
        if orig < 1:
            raise L.VauraHipError(f"source rate {orig} Hz")
        if lengths is None:
            n_in = [N] * B
        else:
            if not clip_params.is_per_clip(lengths):
                raise L.VauraHipError(f"lengths must be one integer per clip (a list, tuple or 1-D tensor), got {lengths!r}")
            n_in = clip_params._int_list("lengths", lengths)
            if len(n_in) != B:
                raise L.VauraHipError(f"lengths has {len(n_in)} values for a batch of {B} clips")
            if min(n_in) < 1 or max(n_in) > N:
                raise L.VauraHipError(f"lengths must lie in 1 .. {N} (the samples of a row), got {n_in}")
        n_out = [self.output_length(nb, orig) for nb in n_in]
        if max(n_out) > MAX_ROW:
            raise L.VauraHipError(f"VAURA_ERR_SHAPE: output rows of {max(n_out)} samples; at most {MAX_ROW}")
        if orig != self.target_sr:
            self.table(orig)
        return pcm, B, C, N, orig, n_in, n_out

    # ---- torch restatement (fp32)
    @torch.no_grad()
    def reference(self, pcm, sample_rate=None, clip_duration=None, lengths=None, interleaved: bool = False):
        """The same result with torch ops in fp32, on ``pcm``'s device: convert, ``mean(dim=0)``, torchaudio's strided ``conv1d`` over
        the full-form kernel (rebuilt from the compact table; for rates whose full form is too large, the gathered runs instead),
        trim, zero padding.  One clip at a time, as the data loader works."""
        pcm, B, C, N, orig, n_in, n_out = self._plan(pcm, sample_rate, clip_duration, lengths, interleaved)
        dev = pcm.device
        out = torch.zeros(B, 1, max(n_out), dtype=torch.float32, device=dev)
        tab = None if orig == self.target_sr else self.table(orig)
        for b in range(B):
            x = pcm[b].t() if interleaved else pcm[b]
            x = x[:, :n_in[b]]
            if x.dtype != torch.float32:
                x = x / (32768 if x.dtype == torch.int16 else 2147483648)
            x = x.mean(dim=0, keepdim=True)
            if tab is not None:
                x = self._resample_torch(x, tab, dev)
            out[b, :, :n_out[b]] = x[:, :n_out[b]]
        return out, torch.tensor(n_out, dtype=torch.int64)

    def _resample_torch(self, x: torch.Tensor, tab: dict, dev: torch.device) -> torch.Tensor:
        o, n, w, T = tab["o"], tab["n"], tab["w"], tab["taps"]
        length = (n * x.shape[-1] + o - 1) // o
        first = tab["first"].to(torch.int64)
        if n * (2 * w + o) <= _FULL_FORM_LIMIT:
            key = ("full", str(dev))
            if key not in tab:
                full = torch.zeros(n, 2 * w + o + T, dtype=torch.float32)
                full.scatter_(1, first[:, None] + torch.arange(T)[None, :], tab["weights"])
                tab[key] = full[:, None, :2 * w + o].contiguous().to(dev)
            y = Fn.conv1d(Fn.pad(x, (w, w + o))[None], tab[key], stride=o)            # (1, n, frames)
            return y.transpose(1, 2).reshape(1, -1)[:, :length]
        key = ("run", str(dev))
        if key not in tab:
            tab[key] = (first.to(dev), tab["weights"].to(dev))
        first, weights = tab[key]
        m = torch.arange(length, device=dev)
        q, p = m // n, m % n
        xp = Fn.pad(x[0], (w, w + o + T))
        idx = (q * o + first[p])[:, None] + torch.arange(T, device=dev)[None, :]
        return (weights[p] * xp[idx]).sum(dim=1)[None]

    # ---- device path
    def _device_table(self, orig: int, dev: torch.device):
        key = (orig, str(dev))
        if key not in self._dev:
            tab = self.table(orig)
            self._dev[key] = (tab["first"].to(dev), tab["weights"].t().contiguous().to(dev))    # taps tap-major: (T, n)
        return self._dev[key]

    @torch.no_grad()
    def __call__(self, pcm, sample_rate=None, clip_duration=None, lengths=None, interleaved: bool = False):
        """Decoded PCM — int16, int32 or float32; (B, C, N) or (C, N), ``interleaved``: (B, N, C) or (N, C) — at ``sample_rate`` (or
        ``int(N / clip_duration)``) -> (wav (B, 1, N_out) fp32 on the device, lengths (B,) int64 on the host): clip b's
        ``lengths[b] = output_length(n_b)`` samples, zeros behind them.  ``lengths``: the real samples ``n_b`` of each row (None: the
        whole row).  Host tensors are copied to the device first, in their own format."""
        pcm, B, C, N, orig, n_in, n_out = self._plan(pcm, sample_rate, clip_duration, lengths, interleaved)
        dev = self.device
        if dev is None:
            dev = pcm.device if pcm.device.type == "cuda" else None
            if dev is None:
                if not torch.cuda.is_available():
                    raise L.VauraHipError("AudioPreprocessor runs on a HIP device only (reference() is the torch restatement)")
                dev = torch.device("cuda", torch.cuda.current_device())
        lib = L.lib()
        identity = orig == self.target_sr
        if identity:
            o = n = 1
            w = T = 0
        else:
            tab = self.table(orig)
            o, n, w, T = tab["o"], tab["n"], tab["w"], tab["taps"]
            if lib.vaura_audio_preprocess_lds_bytes(o, n, w, T) > 64 * 1024:
                raise L.VauraHipError(f"VAURA_ERR_SHAPE: {orig} -> {self.target_sr} Hz: the input span of one tile does not fit 64 KiB of LDS")
        n_row = max(n_out)
        with torch.cuda.device(dev):
            first, taps = (None, None) if identity else self._device_table(orig, dev)
            key = (str(dev), tuple(n_in), tuple(n_out))
            if key not in self._len_dev:
                self._len_dev.clear()                                          # the last call's lengths only
                self._len_dev[key] = (torch.tensor(n_in, dtype=torch.int32, device=dev), torch.tensor(n_out, dtype=torch.int32, device=dev))
            d_in, d_out = self._len_dev[key]
            src = pcm.to(dev, non_blocking=True).contiguous()
            out = torch.empty(B, 1, n_row, dtype=torch.float32, device=dev)
            L.check(lib.vaura_audio_preprocess(L.ptr(src), _FORMATS[pcm.dtype], int(bool(interleaved)), B, C, N, L.ptr(d_in), o, n, w,
                                               L.ptr(first), L.ptr(taps), n, T, L.ptr(out), n_row, L.ptr(d_out),
                                               L.current_stream(dev)), "vaura_audio_preprocess")
        return out, torch.tensor(n_out, dtype=torch.int64)
