"""Float64 restatement of the audio preprocessing (vaura_amd/audio_preprocess.py, csrc/audio_pre.hip), for rates whose FULL tap table
is small: to float -> mono -> torchaudio 2.2.1's ``Resample`` (``sinc_interp_hann``, ``lowpass_filter_width = 6``, ``rolloff = 0.99``;
the full ``n x (2 w + o)`` kernel and ``F.conv1d`` with stride ``o`` on the signal padded by ``(w, w + o)``) -> trim -> zeros.  It
shares no code with the module under test.  Never call it for a rate pair with a small gcd (44 101 Hz: 1.9 G taps).

The bar for one output sample:

    bar = (T + C + 3) * 2^-24 * sum_j |k_j| * (sum_c |x_c,j|) / C

``T`` = the taps per phase of the compact table.  One rounding each for: the tap (float64 -> fp32), every step of the mix and its divide
(C), the product, every add (T - 1); two of slack (the int32 -> fp32 conversion takes one of them).  Derived, not measured; torch's
own fp32 conv sits at about 4 * 2^-24 of that sum."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
FULL_LIMIT = 1 << 24            # refuse to build a full table above this many taps


def ratio(orig, new):
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    base = min(o, n) * 0.99
    return o, n, int(math.ceil(6 * o / base)), base


def full_table(orig, new):
    """torchaudio's _get_sinc_resample_kernel in float64: (n, 2 w + o)."""
    o, n, w, base = ratio(orig, new)
    assert n * (2 * w + o) <= FULL_LIMIT, f"{orig} -> {new}: the full table has {n * (2 * w + o)} taps; use a rate with a larger gcd"
    idx = torch.arange(-w, w + o, dtype=torch.float64)[None, :] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx
    t = t * base
    t = t.clamp(-6, 6)
    window = torch.cos(t * math.pi / 6 / 2) ** 2
    t = t * math.pi
    k = torch.where(t == 0, torch.ones_like(t), t.sin() / t)
    return k * (window * (base / o))


def to_f64(pcm):
    if pcm.dtype == torch.int16:
        return pcm.double() / 32768
    if pcm.dtype == torch.int32:
        return pcm.double() / 2147483648
    assert pcm.dtype in (torch.float32, torch.float64)
    return pcm.double()


def out_length(n_b, orig, new, duration=None):
    o, n, _, _ = ratio(orig, new)
    length = n_b if o == n else -((-n * n_b) // o)
    return length if duration is None else min(length, math.ceil(duration * new))


def _resample(x, k, o, n, w):
    """x (1, L) float64, k (n, 2 w + o) -> (1, ceil(n L / o))."""
    y = F.conv1d(F.pad(x, (w, w + o))[None], k[:, None, :], stride=o)        # (1, n, frames)
    return y.transpose(1, 2).reshape(1, -1)[:, : -((-n * x.shape[-1]) // o)]


def restate(pcm, orig, new, lengths=None, interleaved=False, duration=None, taps_per_phase=None):
    """pcm (B, C, N) / interleaved (B, N, C), CPU -> (out (B, 1, N_out) float64, [output length of clip b], bar (B, 1, N_out) float64).
    ``taps_per_phase``: T of the bar (required unless orig == new)."""
    pcm = pcm.cpu()
    if interleaved:
        pcm = pcm.transpose(1, 2)
    B, C, N = pcm.shape
    lengths = [N] * B if lengths is None else [int(v) for v in lengths]
    o, n, w, _ = ratio(orig, new)
    k = None if o == n else full_table(orig, new).to(torch.float32).double()      # the taps as fp32 holds them
    k_abs = None if k is None else k.abs()
    T = 0 if o == n else int(taps_per_phase)
    n_out = [out_length(nb, orig, new, duration) for nb in lengths]
    out = torch.zeros(B, 1, max(n_out), dtype=torch.float64)
    bar = torch.zeros_like(out)
    for b in range(B):
        x = to_f64(pcm[b, :, :lengths[b]])
        mono, mag = x.mean(dim=0, keepdim=True), x.abs().mean(dim=0, keepdim=True)
        if k is not None:
            mono, mag = _resample(mono, k, o, n, w), _resample(mag, k_abs, o, n, w)
        out[b, :, :n_out[b]] = mono[:, :n_out[b]]
        bar[b, :, :n_out[b]] = (T + C + 3) * U * mag[:, :n_out[b]]
    return out, n_out, bar


def restate_f64_taps(pcm, orig, new):
    """One planar clip (C, N) through the float64 taps (no fp32 rounding of the table): (1, ceil(n N / o)) float64."""
    o, n, w, _ = ratio(orig, new)
    return _resample(to_f64(pcm).mean(dim=0, keepdim=True), full_table(orig, new), o, n, w)
