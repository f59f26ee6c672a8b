"""Float64 restatement of the audio output (vaura_amd/post.py: audio_to_pcm, csrc/audio_out.hip): the float64 taps of torchaudio's
``Resample(44100, rate)`` (tests/audio_pre_reference.py: full_table, the full ``n x (2 w + o)`` form — no compact table, no fp32
rounding), a plain sum, the gain, then the quantisation and the ``clipped`` count in double.  It shares no code with the module under test.

The bar for one output sample is the input side's with one channel and one more unit for the gain product:

    bar = (T + 5) * 2^-24 * |g| * sum_j |k_j| |x_j|

One rounding each for: the tap (float64 -> fp32), the T fused steps, the gain product; three of slack, as there.  Derived, not measured.

``one_pass_f32`` is the fp32 statement of the same sum from the COMPACT table (first[p] and T taps, tap order): what the stream
simulation of tests/test_audio_out_host.py has to reproduce bit for bit."""
import torch

import audio_pre_reference as R

SRC = 44100
U = R.U
SCALE = {torch.int16: 32768.0, torch.int32: 2147483648.0}


def quantise(y, dtype):
    """y float64 -> (values of ``dtype``, clipped mask): rint half-to-even of y * scale, saturated, NaN -> 0; float32: y itself, counted
    outside [-1, 1]."""
    y = y.double()
    if dtype == torch.float32:
        return y.float(), (y < -1) | (y > 1) | y.isnan()
    s = SCALE[dtype]
    v = y * s
    clipped = (v < -s) | (v > s - 1) | v.isnan()
    q = torch.where(v.isnan(), torch.zeros_like(v), torch.round(v).clamp(-s, s - 1))
    return q.to(torch.int64).to(dtype), clipped


def restate(x, rate, lengths=None, gain=None, taps_per_phase=None):
    """x (B, 1, N) float, CPU -> (y (B, N_out) float64: the resampled clip times its gain, [output length of clip b], bar (B, N_out))."""
    x = x.cpu().double()
    B, _, N = x.shape
    lengths = [N] * B if lengths is None else [int(v) for v in lengths]
    gain = [1.0] * B if gain is None else [float(torch.tensor(g, dtype=torch.float32)) for g in gain]   # the gain as fp32 holds it
    o, n, w, _ = R.ratio(SRC, rate)
    k = None if o == n else R.full_table(SRC, rate)
    T = 0 if o == n else int(taps_per_phase)
    n_out = [R.out_length(nb, SRC, rate) for nb in lengths]
    y = torch.zeros(B, max(n_out), dtype=torch.float64)
    bar = torch.zeros_like(y)
    for b in range(B):
        v = x[b, :, :lengths[b]]
        mono, mag = v, v.abs()
        if k is not None:
            mono, mag = R._resample(v, k, o, n, w), R._resample(v.abs(), k.abs(), o, n, w)
        y[b, :n_out[b]] = mono[0, :n_out[b]] * gain[b]
        bar[b, :n_out[b]] = (T + 5) * U * abs(gain[b]) * mag[0, :n_out[b]]
    return y, n_out, bar


def one_pass_f32(x, table, gain=1.0):
    """One clip x (N,) fp32 through the compact table in fp32, tap order: (ceil(n N / o),) fp32."""
    o, n, w, T = table["o"], table["n"], table["w"], table["taps"]
    N = x.shape[0]
    total = -((-n * N) // o)
    return form_f32(torch.arange(total), lambda s: torch.where((s >= 0) & (s < N), x[s.clamp(0, N - 1)], torch.zeros(())), table, gain)


def form_f32(m, sample, table, gain=1.0):
    """outputs ``m`` (int64 tensor of absolute indices) from ``sample(s)`` (absolute input indices -> fp32 values)"""
    o, n, w, T = table["o"], table["n"], table["w"], table["taps"]
    q, p = m // n, m % n
    start = q * o + table["first"].to(torch.int64)[p] - w
    acc = torch.zeros(m.shape[0], dtype=torch.float32)
    for j in range(T):
        acc = acc + table["weights"][p, j] * sample(start + j)
    return acc * torch.tensor(gain, dtype=torch.float32)
