"""fp64 reference of the decoder's attention (rope + causal softmax(q k^T / sqrt(hd)) v over a K / V cache), the storage roundings of the
narrow caches, the seeded input families and the acceptance rules of tests/test_gpu_attention.py.  Plain torch on the CPU: imported by
the -m gpu module and by the CPU self-checks in tests/test_attention_reference.py.

Shapes: q, k, v of a chunk are (R, H, n, hd) ("head-major"); a cache is (R, H, L, hd); an output is (R, n, H * hd)."""
import math

import torch

H, HD = 16, 96
D = H * HD
E4M3_MAX = 448.0
STORAGE = {0: "f32", 1: "f16", 2: "e4m3"}
FAMILIES = ("flat", "peaked", "late_max", "early_max", "huge_first", "huge_last", "huge_new", "wide")


# ---------------------------------------------------------------------------------------------------------------- rope
def _cs(rope, p0, n):
    t = rope[p0:p0 + n]                    # (n, hd/2, 2) fp32
    return t[None, None, :, :, 0], t[None, None, :, :, 1]


def rope64(x, rope, p0):
    """Interleaved rotation of x (R, H, n, hd) at positions p0.. with the fp32 table widened to double; fp64 result and the magnitude
    |x0 c| + |x1 s| of each value's two terms (the scale of the rounding error of any fp32 evaluation of the rotation)."""
    c, s = _cs(rope.double(), p0, x.shape[2])
    xs = x.double().reshape(*x.shape[:-1], -1, 2)
    a, b = xs[..., 0], xs[..., 1]
    y = torch.stack([a * c - b * s, b * c + a * s], dim=-1).flatten(3)
    m = torch.stack([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], dim=-1).flatten(3)
    return y, m


def rope32(x, rope, p0):
    """The same rotation as four fp32 operations per value (what the kernels and oracle.decoder_oracle.apply_rope compute)."""
    c, s = _cs(rope.float(), p0, x.shape[2])
    xs = x.float().reshape(*x.shape[:-1], -1, 2)
    a, b = xs[..., 0], xs[..., 1]
    return torch.stack([a * c - b * s, b * c + a * s], dim=-1).flatten(3)


def unrope(y, rope, p0):
    """fp32 inputs whose rotation is (up to fp32 rounding) y: the inverse rotation in fp64, rounded once."""
    c, s = _cs(rope.double(), p0, y.shape[2])
    ys = y.double().reshape(*y.shape[:-1], -1, 2)
    a, b = ys[..., 0], ys[..., 1]
    return torch.stack([a * c + b * s, b * c - a * s], dim=-1).flatten(3).float()


# ------------------------------------------------------------------------------------------------------------- storage
def narrow(x, kv_dtype):
    """x (fp32 or fp64) as the cache of `kv_dtype` holds it: fp32, fp16 (round to nearest even) or e4m3 — clamped to +-448 FIRST (the
    kernel saturates; torch's conversion alone does not), then rounded to nearest even."""
    if kv_dtype == 0:
        return x.float()
    if kv_dtype == 1:
        return x.half()
    return x.clamp(-E4M3_MAX, E4M3_MAX).float().to(torch.float8_e4m3fn)


def widen(t):
    return t.float().double()


def storage_step(a, kv_dtype):
    """Spacing of the storage's values at magnitude a (fp64 tensor, a >= 0)."""
    mant, emin = {0: (23, -126), 1: (10, -14), 2: (3, -6)}[kv_dtype]
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -200))).clamp_min(emin)
    return torch.exp2(e - mant)


def check_stored_k(got, y64, m64, kv_dtype):
    """The k-cache rule.  got: what the cache holds (storage dtype); y64 / m64: rope64 of the new k.  Returns (n_excluded, n_values).
    fp32 cache: |got - y| <= 2^-23 (|x0 c| + |x1 s|) for EVERY value — three fp32 roundings (two products, one sum) of at most half an ulp
    of a term each; that is one fp32 ulp of the value unless its two terms cancel.
    Narrow caches: got is the storage's rounding of y, except where a rounding boundary of the storage lies within w = 2^-22 (|x0 c| +
    |x1 s|) of y (twice the fp32 evaluation's error bound; 2^-22 relative to |y| itself unless the two terms cancel): there got may be
    the value on the other side, i.e. round(y - w) <= got <= round(y + w) (rounding is monotonic).  Such values are counted, not skipped,
    and none may be more than one step away — except where the window itself is wider than a step (cancelling terms whose sum falls into
    the storage's subnormals: the fp32 torch rotation alone does that to about one value in 10^7)."""
    g = widen(got)
    assert torch.isfinite(g).all()
    if kv_dtype == 0:
        bad = (g - y64).abs() > 2.0 ** -23 * m64 * (1 + 1e-9)
        assert not bool(bad.any()), f"fp32 k cache: {int(bad.sum())} values beyond the fp32 rotation's error bound"
        return 0, g.numel()
    r = widen(narrow(y64, kv_dtype))
    diff = g != r
    if not bool(diff.any()):
        return 0, g.numel()
    gd, rd, yd, wd = g[diff], r[diff], y64[diff], 2.0 ** -22 * m64[diff]
    lo, hi = widen(narrow(yd - wd, kv_dtype)), widen(narrow(yd + wd, kv_dtype))
    far = (gd < lo) | (gd > hi)
    assert not bool(far.any()), (f"{int(far.sum())} stored k values differ from the reference's although the fp64 value is not at a rounding "
                                 f"boundary, e.g. got {float(gd[far][0])!r} for {float(yd[far][0])!r} (rounds to {float(rd[far][0])!r})")
    step = storage_step(torch.maximum(gd.abs(), rd.abs()), kv_dtype)
    assert bool((((gd - rd).abs() <= step) | (2 * wd >= step)).all()), "a stored k value is more than one step of the storage from the reference's"
    return int(diff.sum()), g.numel()


# ----------------------------------------------------------------------------------------------------------- attention
def _mask(p0, n, L):
    return torch.arange(L)[None, :] <= (p0 + torch.arange(n))[:, None]       # key j visible to query i: j <= p0 + i


def _attention(q, K, V, p0):
    n, L = q.shape[2], K.shape[2]
    s = torch.matmul(q, K.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    p = torch.softmax(s.masked_fill(~_mask(p0, n, L), -math.inf), -1)
    merge = lambda o: o.transpose(1, 2).reshape(q.shape[0], n, -1)
    return merge(torch.matmul(p, V)), merge(torch.matmul(p, torch.ones_like(V)))


def attention64(q, K, V, p0):
    """q (R, H, n, hd): rotated queries of positions p0.. ; K, V (R, H, p0 + n, hd): the numbers the cache holds.  fp64 throughout.
    Returns (output, output with every v replaced by 1), each (R, n, H * hd)."""
    return _attention(q.double(), K.double(), V.double(), p0)


def attention32(q, K, V, p0):
    """The yardstick: the same operation as fp32 matmul, torch.softmax, fp32 matmul (the arithmetic of the existing oracle)."""
    return _attention(q.float(), K.float(), V.float(), p0)


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def bar(e_ref):
    """err <= max(3e-6, 4 e_ref): 3e-6 is the project's op-level bar on flat inputs; e_ref the error of attention32 against attention64
    on the case's own inputs (any fp32 evaluation's error grows with |score|); 4 for the different association of the sums."""
    return max(3e-6, 4.0 * e_ref)


def chunk_reference(qr, kr, v, rope, K64, V64, p0, kv_dtype, k_stored=None):
    """Reference of ONE call on the chunk [p0, p0 + n): qr / kr / v the raw (unrotated) fp32 q, k, v (R, H, n, hd); K64, V64 (R, H, >= p0,
    hd) fp64: the numbers the cache holds (its first p0 positions are used).  A decode step is n = 1.  Returns a dict: out64 / out32
    (R, n, D) and ones64 / ones32 (the same with every v, cached and new, replaced by 1: ones64 is 1 up to fp64 rounding), q64 / qm and
    k64 / km (rotated q, k and their term magnitudes), k_stored / v_stored (storage dtype).  k_stored: the chunk's k as the cache holds it
    after the call (judged on its own by check_stored_k) — the attention is then compared on exactly the numbers the kernel read back, so a
    k value that fell on the other side of a rounding boundary does not count against the softmax; None: the reference's own rounding."""
    q64, qm = rope64(qr, rope, p0)
    k64, km = rope64(kr, rope, p0)
    k_st, v_st = narrow(k64, kv_dtype) if k_stored is None else k_stored, narrow(v, kv_dtype)
    K = torch.cat([K64[:, :, :p0], widen(k_st)], dim=2)
    V = torch.cat([V64[:, :, :p0], widen(v_st)], dim=2)
    out64, ones64 = attention64(q64, K, V, p0)
    out32, ones32 = attention32(rope32(qr, rope, p0), K, V, p0)
    return {"out64": out64, "out32": out32, "ones64": ones64, "ones32": ones32, "q64": q64, "qm": qm, "k64": k64, "km": km,
            "k_stored": k_st, "v_stored": v_st}


def huge_key(kr, rows, seed, rope, hot):
    """Raw k of position `hot` carrying the huge_* families' one large key (see family)."""
    u = _direction(rows, seed)
    y, _ = rope64(kr[:, :, hot:hot + 1], rope, hot)
    return unrope(y + math.sqrt(80.0 * math.sqrt(HD)) * u, rope, hot)[:, :, 0]


def _direction(rows, seed):
    u = torch.randn(rows, H, 1, HD, generator=torch.Generator().manual_seed(seed + 7919))
    return u / u.norm(dim=-1, keepdim=True)


# ------------------------------------------------------------------------------------------------------------ families
def family(name, rows, T, seed, rope, hot=None):
    """Raw fp32 (q, k, v), each (rows, H, T, hd), of a sequence of T positions whose ROTATED q / k have the family's score structure
    (designed in the rotated domain, then un-rotated in fp64 and rounded once to fp32).
      flat       randn q, k, v: scores of standard deviation ~1
      peaked     q x 8: score standard deviation ~8, |score| up to ~30
      late_max   k gets a component along a direction shared with q that grows linearly with position (score + 40 j / T):
                 the running maximum moves at every tile / block / wave / split and the newest key is the largest
      early_max  the mirror image with slope -0.5 per position: position 0 dominates, later weights underflow
      huge_*     ONE key (index `hot`) whose score is ~80 above the rest
      wide       v with per-channel scales 1e-3 .. 1e3, +-6e4 in one channel per position; k with one entry of +-600 (beyond e4m3's 448)
                 and one of 3e-4 (below half of e4m3's smallest subnormal 2^-9) per position; q x 0.05 so those keys do not take all the mass"""
    g = torch.Generator().manual_seed(seed)
    shape = (rows, H, T, HD)
    q = torch.randn(shape, generator=g)
    k = torch.randn(shape, generator=g)
    v = torch.randn(shape, generator=g)
    u = _direction(rows, seed)
    j = torch.arange(T, dtype=torch.float32)[None, None, :, None]
    if name == "peaked":
        q = q * 8.0
    elif name in ("late_max", "early_max"):
        a = math.sqrt(HD) ** 0.5 * 4.0                      # q.u = a, k_j.u = g(j) sqrt(hd) / a  ->  score gets g(j)
        slope = 40.0 / T if name == "late_max" else -0.5
        q = q + a * u
        k = k + (slope * j) * (math.sqrt(HD) / a) * u
    elif name.startswith("huge"):
        a = math.sqrt(80.0 * math.sqrt(HD))                 # (a u) . (a u) / sqrt(hd) = 80
        q = q + a * u
        if hot is not None:                                 # None: the caller places the key itself (huge_key)
            k[:, :, hot] = k[:, :, hot] + a * u[:, :, 0]
    elif name == "wide":
        q = q * 0.05
        v = v * torch.logspace(-3, 3, HD)
        pos = torch.arange(T)
        sign = torch.where(pos % 2 == 0, 1.0, -1.0)
        k[:, :, pos, (pos * 7) % HD] = 600.0 * sign
        k[:, :, pos, (pos * 7 + 2) % HD] = 3e-4 * sign          # not the rotation partner of the +-600 entry
        v[:, :, pos, (pos * 5 + 2) % HD] = -6e4 * sign
    elif name != "flat":
        raise ValueError(name)
    return unrope(q, rope, 0), unrope(k, rope, 0), v.contiguous()
