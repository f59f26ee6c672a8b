"""Float64 restatement of the streaming loudness meter and the causal normaliser (csrc/loudness.hip, vaura_amd/post.py) on the CPU;
shares no code with vaura_amd/loudness.py.

With ``step = rint(0.1 rate)`` and ``gate = 4 step``, for one clip x[0 .. n):
  K-weighting  two biquads in direct form I on their unclamped state (scipy's lfilter), the output of each clamped to [-1, 1];
  S_j          the sum of squares of the K-weighted samples of step j (whole steps only);
  M_j          -0.691 + 10 log10((S_j + .. + S_j+3) / gate);  short-term: the same over 30 steps;
  I_m          m >= 4: the blocks j in [max(0, m - history), m - 4]; absolute gate l > -70, relative gate 10 LU below the mean of the
               absolutely gated; NaN where no block exists or none passes a gate;
  d_m          clamp(target - I_m, +-max_gain_db), d_{m-1} where I_m is NaN, d_{-1} = initial_gain_db; with a slew
               d_{m-1} + clamp(d_m - d_{m-1}, +-0.1 slew);  a_m = 10^(d_m / 20);
  out[i]       m = i // step, k = i - m step:  limiter(x[i] (a_{m-1} + (a_m - a_{m-1}) (k + 1) / step)).

The bar of the normalised samples (``sample_bar``), in units of u = 2^-24 (half an fp32 ulp, relative), counts the fp32 operations of
the normaliser GIVEN the integrated values I_m it starts from (the meter has its own check):
  d_m      target - I: one rounding, |error| <= u D with D = max |d| <= max(max_gain_db, |initial_gain_db|); the clamp is exact.  With a
           slew two more (the difference, the sum), and d_m then depends on the rounded d_{m-1}: <= 3 u D (m + 1) after m boundaries;
  a_m      d / 20: one rounding; powf: the HIP math library documents 1 ulp, taken as 2 ulp = 4 u.  10^(d/20) turns an absolute error
           e of d into a relative ln(10)/20 e:   eps_a = ln(10)/20 (err_d + u D) + 4 u;
  g        a convex combination of a_{m-1} and a_m: their errors enter with at most eps_a max(a);  a_m - a_{m-1}, (k + 1) / step and
           their product: 3 u |a_m - a_{m-1}|;  the sum: u g;
  out      the product x g: u |x| g;  tanhf (2 ulp = 4 u of a value <= |x| g, slope <= 1);  the clip is exact.
  |out - oracle| <= |x| ((eps_a max(a) + 3 u |a_m - a_{m-1}|) + (2 + 4 [tanh]) u g)
"""
import math

import numpy as np
from scipy.signal import lfilter

U = 2.0 ** -24
SHORT_TERM_STEPS = 30


def step_of(rate):
    return int(np.rint(0.1 * rate))


def coefficients(rate):
    """((b, a) of the shelf, (b, a) of the high-pass), a[0] = 1"""
    w0 = 2 * math.pi * 1500.0 / rate
    A = math.exp(4.0 / 40 * math.log(10))
    alpha = math.sin(w0) / 2 / (1 / math.sqrt(2))
    t1, t2, t3 = 2 * math.sqrt(A) * alpha, (A - 1) * math.cos(w0), (A + 1) * math.cos(w0)
    a0 = (A + 1) - t2 + t1
    shelf = (np.array([A * ((A + 1) + t2 + t1), -2 * A * ((A - 1) + t3), A * ((A + 1) + t2 - t1)]) / a0,
             np.array([a0, 2 * ((A - 1) - t3), (A + 1) - t2 - t1]) / a0)
    w0 = 2 * math.pi * 38.0 / rate
    alpha = math.sin(w0) / 2 / 0.5
    a0 = 1 + alpha
    hp = (np.array([(1 + math.cos(w0)) / 2, -1 - math.cos(w0), (1 + math.cos(w0)) / 2]) / a0, np.array([a0, -2 * math.cos(w0), 1 - alpha]) / a0)
    return shelf, hp


def k_weight(x, rate):
    (bs, as_), (bh, ah) = coefficients(rate)
    y = np.clip(lfilter(bs, as_, np.asarray(x, dtype=np.float64)), -1.0, 1.0)
    return np.clip(lfilter(bh, ah, y), -1.0, 1.0)


def k_weight_literal(x, rate):
    """the same, sample by sample"""
    out = np.asarray(x, dtype=np.float64)
    for b, a in coefficients(rate):
        y = np.zeros(len(out))
        x1 = x2 = y1 = y2 = 0.0
        for i, xi in enumerate(out):
            v = b[0] * xi + b[1] * x1 + b[2] * x2 - a[1] * y1 - a[2] * y2
            x2, x1, y2, y1 = x1, xi, y1, v
            y[i] = min(max(v, -1.0), 1.0)
        out = y
    return out


def step_energies(x, rate):
    step = step_of(rate)
    w = k_weight(x, rate)
    return np.array([np.sum(w[j * step:(j + 1) * step] ** 2) for j in range(len(w) // step)])


def _lk(e):
    with np.errstate(divide="ignore"):
        return -0.691 + 10 * np.log10(e)


def integrated_parts(S, m, gate, history):
    """(I_m or NaN, the smallest distance in LU of a block from a gate it is compared with or inf, the mean energy of the blocks that
    pass both gates or NaN, how many they are)"""
    js = list(range(max(0, m - history), m - 3))
    if not js:
        return float("nan"), float("inf"), float("nan"), 0
    e = np.array([(S[j] + S[j + 1] + S[j + 2] + S[j + 3]) / gate for j in js])
    l = _lk(e)
    margin = float(np.abs(l + 70.0).min())
    g1 = l > -70.0
    if not g1.any():
        return float("nan"), margin, float("nan"), 0
    rel = -0.691 + 10 * np.log10(e[g1].mean()) - 10.0
    margin = min(margin, float(np.abs(l[g1] - rel).min()))
    g2 = g1 & (l > rel)
    if not g2.any():
        return float("nan"), margin, float("nan"), 0
    mean = float(e[g2].mean())
    return float(-0.691 + 10 * np.log10(mean)), margin, mean, int(g2.sum())


def integrated(S, m, gate, history):
    """(I_m or NaN, the smallest distance in LU of a block from a gate it is compared with, or inf)"""
    return integrated_parts(S, m, gate, history)[:2]


def meter(x, rate, history=4096):
    """-> dict: S, I (boundaries 0 .. steps) with the mean energy and the count of the blocks behind each (I_mean, I_count), momentary
    (blocks), short_term (windows), margin (LU, over every boundary)"""
    step = step_of(rate)
    S = step_energies(x, rate)
    ns = len(S)
    I, mean, count, margin = [], [], [], float("inf")
    for m in range(ns + 1):
        v, mg, e, n = integrated_parts(S, m, 4 * step, history)
        I.append(v)
        mean.append(e)
        count.append(n)
        margin = min(margin, mg)
    mom = np.array([_lk((S[j] + S[j + 1] + S[j + 2] + S[j + 3]) / (4 * step)) for j in range(max(0, ns - 3))])
    st = np.array([_lk(S[j:j + SHORT_TERM_STEPS].sum() / (SHORT_TERM_STEPS * step)) for j in range(max(0, ns - SHORT_TERM_STEPS + 1))])
    return {"S": S, "I": np.array(I), "I_mean": np.array(mean), "I_count": np.array(count), "momentary": mom, "short_term": st,
            "margin": margin, "step": step}


def gains_db(I, target=-12.0, max_gain_db=20.0, slew=None, initial_gain_db=0.0):
    """d_m for m = 0 .. len(I) - 1"""
    d, prev = [], float(initial_gain_db)
    for v in I:
        dm = prev if math.isnan(v) else min(max(target - v, -max_gain_db), max_gain_db)
        if slew is not None:
            dm = prev + min(max(dm - prev, -0.1 * slew), 0.1 * slew)
        d.append(dm)
        prev = dm
    return np.array(d)


def normalise(x, rate, I, target=-12.0, max_gain_db=20.0, slew=None, initial_gain_db=0.0, limiter="clip"):
    """The normaliser on the integrated values ``I`` (boundaries 0 .. steps) -> dict: out, xg = |x| g, d, clipped, bar (``sample_bar``)"""
    x = np.asarray(x, dtype=np.float64)
    step = step_of(rate)
    d = gains_db(I, target, max_gain_db, slew, initial_gain_db)
    a = np.concatenate([[10.0 ** (initial_gain_db / 20.0)], 10.0 ** (d / 20.0)])        # a[m + 1] = a_m
    i = np.arange(len(x))
    m = i // step
    k = i - m * step
    a0, a1 = a[m], a[m + 1]
    g = a0 + (a1 - a0) * (k + 1) / step
    y = x * g
    out = np.clip(np.tanh(y) if limiter == "tanh" else y, -1.0, 1.0)
    D = max(max_gain_db, abs(initial_gain_db))
    err_d = U * D * (3.0 * (m + 1) if slew is not None else 1.0)
    eps_a = math.log(10.0) / 20.0 * (err_d + U * D) + 4 * U
    bar = np.abs(x) * ((eps_a * np.maximum(a0, a1) + 3 * U * np.abs(a1 - a0)) + (2 + (4 if limiter == "tanh" else 0)) * U * g)
    return {"out": out, "xg": np.abs(y), "d": d, "clipped": int((np.abs(y) > 1.0).sum()), "bar": bar, "g": g}


def oracle(x, rate, history=4096, **kw):
    """meter and normaliser of one clip in float64"""
    mt = meter(x, rate, history)
    res = normalise(x, rate, mt["I"], **kw)
    res.update(mt)
    return res


def stepped_noise(rate, amps, tail, tail_amp, seed=0):
    """seeded Gaussian noise times one amplitude per step, plus a ragged tail (numpy default_rng(seed)), fp32"""
    step = step_of(rate)
    rng = np.random.default_rng(seed)
    parts = [a * rng.standard_normal(step) for a in amps] + [tail_amp * rng.standard_normal(tail)]
    return np.concatenate(parts).astype(np.float32)


AMPS = [0.2] * 4 + [0.05] * 2 + [0.6] * 4 + [0.0] * 4 + [1e-5] * 4 + [0.3] * 4
