"""CPU restatement of the scaled e4m3 K / V storage (vaura_decoder.kv_dtype = 3, include/vaura_hip.h): ``quantise``, ``widen``, the fp64
cache a kernel reads, and the boundary sets inside which a device whose fp32 rotation differs in the last bit may store other bits.  Plain
torch on the CPU: imported by tests/test_kv_f8s_host.py and tests/test_gpu_kv_f8s.py.

The rule, for a vector x of 96 channels (last dimension): amax = max |x_c|; e = the smallest integer with amax 2^-e <= 448, clamped to
[-127, 127], -127 for amax = 0; byte c = e4m3(x_c 2^-e) (exact multiply, one rounding to nearest even); exponent byte e + 127.  A vector
holding an inf or NaN: exponent byte 0xFF, bytes 0x7F, widened to NaN in every channel.  Widened value: float(byte) 2^e."""
import torch

E4M3_MAX = 448.0
NONFINITE = 0xFF


def exponent(amax):
    """e of the rule for amax >= 0 (finite, any float dtype), int64.  amax = m 2^ex with m in [0.5, 1); 448 = 0.875 * 2^9."""
    m, ex = torch.frexp(amax.double())
    e = ex.long() - 9 + (m > 0.875).long()
    return torch.where(amax == 0, torch.full_like(e, -127), e).clamp(-127, 127)


def scaled(x, e):
    """x 2^-e in fp64 (exact)."""
    return x.double() * torch.exp2(-e.double())[..., None]


def quantise(x):
    """x (..., 96) fp32 (or fp64: rounded through fp32 after the exact scaling) -> (bytes (..., 96) uint8, exponent bytes (...) uint8)."""
    amax = x.abs().amax(-1)
    ok = torch.isfinite(amax)
    e = exponent(torch.where(ok, amax, torch.zeros_like(amax)))
    b = scaled(torch.where(ok[..., None], x, torch.zeros_like(x)), e).float().to(torch.float8_e4m3fn).view(torch.uint8)
    b = torch.where(ok[..., None], b, torch.full_like(b, 0x7F))
    return b.contiguous(), torch.where(ok, e + 127, torch.full_like(e, NONFINITE)).to(torch.uint8)


def widen(b, eb):
    """(bytes, exponent bytes) -> fp64 values; NaN in every channel of a vector whose exponent byte is 0xFF."""
    v = b.view(torch.float8_e4m3fn).float().double() * torch.exp2(eb.double() - 127)[..., None]
    return torch.where((eb == NONFINITE)[..., None], torch.full_like(v, float("nan")), v)


def cache64(x):
    """The numbers a kernel reads back from a cache that stored x."""
    return widen(*quantise(x))


def near_power_of_two(amax64, rel=1e-6):
    """Vectors whose fp64 amax / 448 lies within a relative `rel` of a power of two: an fp32 evaluation of the same vector may pick the
    neighbouring exponent.  (amax = 0 is not near anything.)"""
    r = amax64.double() / E4M3_MAX
    p = torch.exp2(torch.round(torch.log2(r.clamp_min(2.0 ** -1000))))
    return (r > 0) & ((r / p - 1).abs() <= rel)


def boundary_elements(y64, m64, e):
    """k elements at an e4m3 rounding boundary in the sense of attention_reference.check_stored_k: a boundary of the grid lies within
    w = 2^-22 (|x0 c| + |x1 s|) of the fp64 rotation y (twice the error bound of any fp32 evaluation of it), judged on the scaled values."""
    s, w = scaled(y64, e), scaled(2.0 ** -22 * m64, e)
    lo, hi = (s - w).float().to(torch.float8_e4m3fn).view(torch.uint8), (s + w).float().to(torch.float8_e4m3fn).view(torch.uint8)
    return lo != hi


def check_stored_k(got_b, got_e, y64, m64):
    """The k-cache rule of storage 3.  got_b / got_e: what the device stored for the chunk; y64 / m64: attention_reference.rope64 of its
    raw k.  Outside the boundary sets (vectors: near_power_of_two; elements: boundary_elements) bytes and exponents are bit for bit the
    restatement's on y64.  Returns (excluded vectors, vectors, excluded elements, elements)."""
    amax = y64.abs().amax(-1)
    vec = near_power_of_two(amax)
    e = exponent(amax)
    assert torch.equal(got_e[~vec].long(), (e + 127)[~vec]), "a stored k exponent differs from the restatement's away from every power of two"
    want_b = scaled(y64, e).float().to(torch.float8_e4m3fn).view(torch.uint8)
    el = boundary_elements(y64, m64, e) | vec[..., None]
    bad = (got_b != want_b) & ~el
    assert not bool(bad.any()), f"{int(bad.sum())} stored k bytes differ from the restatement's away from every rounding boundary"
    return int(vec.sum()), vec.numel(), int((el & ~vec[..., None]).sum()), el.numel()
