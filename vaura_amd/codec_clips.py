"""Layout of a batch of clips of different lengths as ONE packed sequence for the codec (``CodecEngine.decode_clips``,
``CodecEncoderEngine.encode_clips``; include/vaura_hip.h vaura_dac_decode_clips / vaura_dac_encode_clips).  Pure host arithmetic.

The clips lie behind one another on the time axis with ``gap`` latent frames of zeros between neighbours; clip b starts at latent
row ``offsets[b]``, at row ``offsets[b] * rate`` on a level with ``rate`` rows per latent frame and at sample ``offsets[b] * hop``.
The gap is the smallest number of latent frames G with G * rate(level) >= the largest one-sided reach of any conv that runs on that
level: a k-tap conv of dilation d reaches (k - 1) / 2 * d rows, a transposed conv (k = 2r, stride r) one row of its input level, a
strided conv (k = 2r, stride r) one row of its OUTPUT level.  The library computes the same number from the conv descriptors
(vaura_dac_clips_gap / vaura_dac_encode_clips_gap)."""
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
