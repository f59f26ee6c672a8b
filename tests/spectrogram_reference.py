"""Float64 restatement of the spectrogram (csrc/spectrogram.hip) on the CPU; shares no code with vaura_amd/spectrogram.py.

The quantity.  Clip b with n samples, zero outside; column t covers lo = hop t + hop/2 - n_fft/2 .. lo + n_fft - 1; y = w x with the
periodic Hann window w (as fp32 values, in double); X = rfft(y); P = |X|^2; M = f P.  Here: the clip is zero-padded by
(n_fft - hop) / 2 on the left and up to (cols - 1) hop + n_fft samples on the right, then ``torch.stft(center=False)`` in float64 —
exactly ceil(n / hop) columns, equal to the per-column rfft of that window (tests/test_spectrogram_host.py checks both).

The mel filters are restated from the published formulas (Slaney: 3 f / 200 below 1 kHz, 15 + 27 ln(f / 1000) / ln 6.4 above; HTK:
2595 log10(1 + f / 700)); torchaudio and librosa are not available, so the filterbank's PARITY IS UNPINNED.  It is held to known
answers and to its structure instead.

Bars, u = 2^-24, beta_t = u sum_i |y_t[i]|, none tuned:
  |X^ - X| <= c beta_t for every bin: every rounding on the way from the inputs to one output perturbs it by at most u times a partial
      sum of |y|, and c counts them along one path of the kernel's plan, as its header lists them — window product 1, a radix-4
      stage 5 (two sums, twiddle entry, product, product sum; 2 for the last one, whose twiddle is exactly 1), the radix-2 stage
      1, the real-input post-pass 5 — plus 3 of slack for the complex magnitudes:
          n_fft 2048: 1 + 4 * 5 + 2 + 5 + 3 = 31;  n_fft 1024: 1 + 4 * 5 + 1 + 5 + 3 = 30;  n_fft 512: 1 + 3 * 5 + 2 + 5 + 3 = 26
  |P^ - P| <= 2 |X| c beta + (c beta)^2 + 3 u P                    (two products and one sum)
  |M^ - M| <= sum_k f barP[k] + (count_m + 2) u sum_k f P          (an fmaf chain of count_m terms)
The worst-case bar is loose, so a measured condition sits beside it: max_k |X^ - X| / beta_t of the device is at most 4 times that
of ``torch.fft.rfft`` in fp32 on the same frames (0.40 / 0.47 / 0.63 units at n_fft 2048 / 1024 / 512 on the test's noise; the
device's own figures there: 0.41 / 0.56 / 0.68).

"db" / "log" are checked against the device's own "power" output pushed through the float64 formula.  The kernel calls ``log10f`` /
``logf`` of the device library, built to OpenCL's accuracy table: at most 3 ulp each.  Bars: "log" 3 ulp(l); "db" 10 * 3 ulp(l) +
ulp(10 l) / 2 for the one product; ulp(v) = 2^(floor(log2 |v|) - 23), and 0 for l = 0 (log(1) is exact)."""
import math

import torch

U = 2.0 ** -24
C_ROUNDINGS = {2048: 31, 1024: 30, 512: 26}
LOG_ULPS = 3.0
SR = 44100


def hann(n_fft):
    return torch.hann_window(n_fft, periodic=True, dtype=torch.float64).float().double()     # the fp32 values, in double


def columns(n, hop):
    return -(-n // hop)


def padded(x, n_fft, hop):
    """clip (n,) -> the padded float64 row stft(center=False) takes"""
    n = x.shape[0]
    cols = columns(n, hop)
    left = n_fft // 2 - hop // 2
    total = (cols - 1) * hop + n_fft
    row = torch.zeros(total, dtype=torch.float64)
    row[left:left + n] = x.double()
    return row


def spectrum(x, n_fft, hop):
    """clip (n,) -> X (cols, n_fft/2 + 1) complex128, beta (cols,): u sum |y|, and the fp32 frames y (cols, n_fft) as the device forms them"""
    row = padded(x, n_fft, hop)
    w = hann(n_fft)
    X = torch.stft(row, n_fft, hop_length=hop, window=w, center=False, return_complex=True).transpose(0, 1)
    frames = row.unfold(0, n_fft, hop)
    y = frames * w
    return X, U * y.abs().sum(dim=1), (frames.float() * w.float())


def torch_fp32_units(y32, X, beta):
    """max_k |rfft_fp32(y) - X| / beta over the columns with a non-zero frame"""
    got = torch.fft.rfft(y32).to(torch.complex128)
    keep = beta > 0
    return float(((got - X).abs().max(dim=1).values[keep] / beta[keep]).max()) if bool(keep.any()) else 0.0


def power_bar(X, beta, n_fft):
    cb = (C_ROUNDINGS[n_fft] * beta)[:, None]
    P = X.real ** 2 + X.imag ** 2
    return P, 2 * X.abs() * cb + cb ** 2 + 3 * U * P


# ------------------------------------------------------------------------------------------------ mel filters, restated
def hz_to_mel(f, scale):
    if scale == "htk":
        return 2595.0 * math.log10(1.0 + f / 700.0)
    return 3.0 * f / 200.0 if f < 1000.0 else 15.0 + 27.0 * math.log(f / 1000.0) / math.log(6.4)


def mel_to_hz(m, scale):
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return 200.0 * m / 3.0 if m < 15.0 else 1000.0 * math.exp(math.log(6.4) * (m - 15.0) / 27.0)


def mel_filters(n_fft, n_mels, f_min=0.0, f_max=None, scale="slaney", norm=None):
    """(n_mels, n_fft/2 + 1) float64, filter by filter and bin by bin"""
    f_max = SR / 2.0 if f_max is None else f_max
    m0, m1 = hz_to_mel(f_min, scale), hz_to_mel(f_max, scale)
    pts = [mel_to_hz(m0 + (m1 - m0) * i / (n_mels + 1), scale) for i in range(n_mels + 2)]
    fb = torch.zeros(n_mels, n_fft // 2 + 1, dtype=torch.float64)
    for m in range(n_mels):
        a, b, c = pts[m], pts[m + 1], pts[m + 2]
        for k in range(n_fft // 2 + 1):
            f = k * SR / n_fft
            v = max(0.0, min((f - a) / (b - a), (c - f) / (c - b)))
            fb[m, k] = v * (2.0 / (c - a)) if norm == "slaney" else v
    return fb, pts


def mel_bar(fb32, P, barP):
    """fb32 (F, bins) the fp32 weights in double -> M (cols, F), its bar"""
    count = (fb32 != 0).sum(dim=1).double()
    fP = P @ fb32.t()
    return fP, barP @ fb32.t() + (count + 2)[None, :] * U * fP


# ------------------------------------------------------------------------------------------------ scales
def ulp32(v):
    v = v.abs()
    e = torch.floor(torch.log2(v.clamp(min=2.0 ** -126)))
    return torch.where(v > 0, 2.0 ** (e - 23), torch.zeros_like(v))


def scaled(power32, scale, amin):
    """the device's own fp32 power values -> (float64 value, bar)"""
    a = float(torch.tensor(amin, dtype=torch.float32))
    v = power32.double().clamp(min=a)
    if scale == "log":
        l = torch.log(v)
        return l, LOG_ULPS * ulp32(l)
    l = torch.log10(v)
    return 10.0 * l, 10.0 * LOG_ULPS * ulp32(l) + 0.5 * ulp32(10.0 * l)
