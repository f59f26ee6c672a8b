"""Layout of a batch of clips of different lengths as ONE packed sequence for the codec (``CodecEngine.decode_clips``,
``CodecEncoderEngine.encode_clips``; include/vaura_hip.h vaura_dac_decode_clips / vaura_dac_encode_clips).  Pure host arithmetic.

The clips lie behind one another on the time axis with ``gap`` latent frames of zeros between neighbours; clip b starts at latent
row ``offsets[b]``, at row ``offsets[b] * rate`` on a level with ``rate`` rows per latent frame and at sample ``offsets[b] * hop``.
The gap is the smallest number of latent frames G with G * rate(level) >= the largest one-sided reach of any conv that runs on that
level: a k-tap conv of dilation d reaches (k - 1) / 2 * d rows, a transposed conv (k = 2r, stride r) one row of its input level, a
strided conv (k = 2r, stride r) one row of its OUTPUT level.  The library computes the same number from the conv descriptors
(vaura_dac_clips_gap / vaura_dac_encode_clips_gap).

``window_layout`` is the layout of ``CodecEngine.decode_window`` (vaura_dac_decode_window): a window of every clip with ``decode_halo``
frames of context either side, the windows packed like clips."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Sequence, Tuple

KERNEL = 7          # the k of the residual units' dilated conv and of the first / last conv on the waveform side (DAC 1.0.0)
LATENT_KERNEL = 3   # the encoder's last conv (C -> latent)


@dataclass(frozen=True)
class ClipLayout:
    gap: int                     # latent frames of zeros between neighbouring clips
    frames: Tuple[int, ...]      # latent frames of each clip
    offsets: Tuple[int, ...]     # first latent row of each clip in the packed sequence
    total: int                   # latent rows of the packed sequence (no gap behind the last clip)
    hop: int                     # samples per latent frame


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def decode_gap(cfg) -> int:
    """Gap of the decoder: conv_in (k7) at rate 1, per block the transposed conv on its input level and the three units on its
    output level, conv_out (k7) on the samples."""
    reach = (KERNEL - 1) // 2
    g, rate = reach, 1
    for r in cfg.decoder_rates:
        g = max(g, _ceil_div(1, rate))
        rate *= r
        for d in cfg.dilations:
            g = max(g, _ceil_div(reach * d, rate))
    return max(1, g, _ceil_div(reach, rate))


def encode_gap(cfg) -> int:
    """Gap of the encoder: conv_in (k7) on the samples, per block the three units on its input level and the strided conv on its
    output level, the last conv (k3) at rate 1."""
    reach = (KERNEL - 1) // 2
    rate = int(math.prod(cfg.encoder_rates))
    g = _ceil_div(reach, rate)
    for r in cfg.encoder_rates:
        for d in cfg.dilations:
            g = max(g, _ceil_div(reach * d, rate))
        rate //= r
        g = max(g, _ceil_div(1, rate))
    return max(1, g, _ceil_div((LATENT_KERNEL - 1) // 2, rate))


def clip_layout(lengths: Sequence[int], cfg, side: str = "decode") -> ClipLayout:
    """``side`` "decode": ``lengths`` are latent frames T_b; "encode": samples n_b, a clip takes ceil(n_b / hop) frames (its tail is
    zero-padded, DAC.preprocess).  Every length must be a positive int."""
    if side not in ("decode", "encode"):
        raise ValueError(f"side must be 'decode' or 'encode', got {side!r}")
    lens = list(lengths)
    if not lens or any(isinstance(n, bool) or not isinstance(n, int) or n < 1 for n in lens):
        raise ValueError(f"clip lengths must be positive integers, one per clip, got {lens}")
    if side == "decode":
        hop, gap, frames = int(math.prod(cfg.decoder_rates)), decode_gap(cfg), lens
    else:
        hop, gap = int(math.prod(cfg.encoder_rates)), encode_gap(cfg)
        frames = [_ceil_div(n, hop) for n in lens]
    offsets, o = [], 0
    for f in frames:
        offsets.append(o)
        o += f + gap
    return ClipLayout(gap=gap, frames=tuple(frames), offsets=tuple(offsets), total=o - gap, hop=hop)


# ---- a window of every clip (CodecEngine.decode_window; include/vaura_hip.h vaura_dac_decode_window)
@dataclass(frozen=True)
class WindowLayout:
    halo: int                    # frames of context either side of the frames asked for
    gap: int                     # latent frames of zeros between neighbouring windows
    clips: Tuple[int, ...]       # per window: the clip it belongs to (a clip with count 0 has no window)
    lo: Tuple[int, ...]          # per window: its first frame in the clip, max(0, start - halo)
    hi: Tuple[int, ...]          # per window: one past its last frame, min(length, start + count + halo)
    skips: Tuple[int, ...]       # per window: halo frames in front of the frames asked for, start - lo
    offsets: Tuple[int, ...]     # per window: its first latent row in the packed sequence
    total: int                   # latent rows of the packed sequence (no gap behind the last window)
    hop: int                     # samples per latent frame


def decode_halo(cfg) -> int:
    """Frames of context either side that the samples of ONE latent frame depend on: the rows [0, hop) of the last level, taken
    backwards through the layers.  A k-tap conv of dilation d widens the interval by (k - 1) / 2 * d rows either side; a transposed
    conv (stride r, k = 2r, pad ceil(r / 2)) writes row o from the input rows j with o = j * r - pad + t, 0 <= t < k, so [lo, hi]
    comes from [ceil((lo + pad - k + 1) / r), floor((hi + pad) / r)].  At the latent level the frame itself is row 0.  The library
    computes the same number from the conv descriptors (vaura_dac_decode_halo)."""
    reach = (KERNEL - 1) // 2
    lo, hi = -reach, int(math.prod(cfg.decoder_rates)) - 1 + reach          # conv_out on the samples
    for r in reversed(cfg.decoder_rates):
        unit = reach * sum(cfg.dilations)                                   # the three units; their 1 x 1 convs reach nothing
        lo, hi = lo - unit, hi + unit
        pad, k = _ceil_div(r, 2), 2 * r
        lo, hi = _ceil_div(lo + pad - k + 1, r), (hi + pad) // r
    return max(reach - lo, hi + reach)                                      # conv_in at rate 1


def window_layout(lengths: Sequence[int], starts: Sequence[int], counts: Sequence[int], cfg) -> WindowLayout:
    """The frames [starts[b], starts[b] + counts[b]) of clip b (``lengths[b]`` frames) with the halo either side, clamped to the
    clip, and the windows laid out behind one another with the gap of ``clip_layout``.  A count of 0 gives the clip no window."""
    lens, s, n = list(lengths), list(starts), list(counts)
    if not lens or not (len(lens) == len(s) == len(n)):
        raise ValueError(f"lengths, starts and counts must hold one value per clip, got {lens}, {s}, {n}")
    if any(isinstance(v, bool) or not isinstance(v, int) for v in lens + s + n):
        raise ValueError(f"lengths, starts and counts must be integers, got {lens}, {s}, {n}")
    if any(t < 1 or a < 0 or c < 0 or a + c > t for t, a, c in zip(lens, s, n)):
        raise ValueError(f"every window must lie inside its clip: lengths {lens}, starts {s}, counts {n}")
    H, gap = decode_halo(cfg), decode_gap(cfg)
    clips = [b for b, c in enumerate(n) if c > 0]
    lo = [max(0, s[b] - H) for b in clips]
    hi = [min(lens[b], s[b] + n[b] + H) for b in clips]
    offsets, o = [], 0
    for a, z in zip(lo, hi):
        offsets.append(o)
        o += z - a + gap
    return WindowLayout(halo=H, gap=gap, clips=tuple(clips), lo=tuple(lo), hi=tuple(hi), skips=tuple(s[b] - a for b, a in zip(clips, lo)),
                        offsets=tuple(offsets), total=max(0, o - gap), hop=int(math.prod(cfg.decoder_rates)))
