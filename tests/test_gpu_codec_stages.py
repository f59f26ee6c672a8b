"""Codec kernels (csrc/dac.hip) stage by stage against torch fp64 on the CPU, through the op-level entry points that make exactly the
launches of vaura_dac_decode / vaura_dac_encode: every conv epilogue (residual add, Snake, raw + activated outputs, the activated copy as
pair planes or block-scaled e4m3), tile boundaries of the stride-1 and the transposed convs, the 256-row / one-launch-unit instances,
from_codes, the last conv, the encoder's first conv and one residual-VQ stage.

Conventions of every case
  * B = 2 and clip 1 is clip 0's distribution x 100: a halo row read across the clip boundary is an error of order 100, not of order 1.
  * Every output lives inside a larger allocation whose bytes are all 0xFF (fp32 / fp16 / e4m3 NaN, scale byte 255, code -1 — none of
    which a kernel writes for finite inputs): the guard bytes before and after must still be 0xFF and no output element may be.
  * The reference is fp64 on the numbers the kernel multiplies (quant.fp8_effective_weight, quant.mx8_effective_activation, .half() for
    "f16"), as in test_gpu_ops.py::test_codec_convolution_per_precision.

Bars (derived; none is tuned on the kernels)
  raw      |err| <= REL x max |conv ref| of the CLIP (+ 2^-23 |out| for the residual's one fp32 add), REL = 2e-6 pair paths, 6e-6 f32,
           5e-5 mx8: the bars test_codec_convolution_per_precision holds, per clip instead of per tensor.
  act      against fp64 Snake of the kernel's OWN raw output (on the fp32 product alpha x, like test_snake_sine): 4e-7 / alpha on the
           sin^2 term + 2^-22 |y| + 2^-25 representation.  Where the launch writes no raw output: against Snake of the fp64 reference,
           plus the raw bar through the Snake's Lipschitz constant 2 and 2^-24 |x| for the fp32 product.
  mx8 act  scale bytes == quant's rule and values == quant.mx8_effective_activation(snake64(raw)) except where the exact value is within
           1e-5 relative of an e4m3 rounding boundary (one grid step allowed) or the block's amax within 1e-5 relative of 448 x 2^k (one
           scale step allowed); those elements are at most 1e-3 of all (the reference's own share under a 1e-5 perturbation is printed
           next to it: ~1e-4).  Without a raw output: |deq - y| <= E + half a grid step at the kernel's scale, E as for "act".
  chains   fp32 single-chain kernels: |err| <= n 2^-24 sum |terms| (n = chain length + bias adds).
Measured values next to these bars: set VAURA_CODEC_STAGE_PARITY_OUT=<file> (profiles/codec_stage_parity.txt is such a file)."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import parity_helpers as ph
from vaura_amd import _lib as L
from vaura_amd import quant
from vaura_amd.variants import Variant, variants

DEV = "cuda:0"
PRECISIONS = ["f32", "f16pair", "f16", "f16pair_w8", "mx8"]
RAW_REL = {"f32": 6e-6, "f16pair": 2e-6, "f16": 2e-6, "f16pair_w8": 2e-6, "mx8": 5e-5}
U24 = 2.0 ** -24


# ----------------------------------------------------------------------------------------------------------------- guarded outputs
class Guarded:
    """`nbytes` of device memory inside a larger allocation filled with 0xFF; `guard` bytes (a multiple of 256) on either side."""

    def __init__(self, nbytes, guard):
        assert guard % 256 == 0 and nbytes % 4 == 0
        self.n, self.g = nbytes, guard
        self.buf = torch.full((guard + nbytes + guard,), 0xFF, dtype=torch.uint8, device=DEV)

    def view(self, dtype=torch.uint8):
        return self.buf[self.g: self.g + self.n].view(dtype)

    def host(self):
        """The payload bytes on the CPU, after asserting that both guards are bit-unchanged."""
        h = self.buf.cpu()
        assert bool((h[: self.g] == 0xFF).all()), "bytes BEFORE the output were written"
        assert bool((h[self.g + self.n:] == 0xFF).all()), "bytes BEHIND the output were written"
        return h[self.g: self.g + self.n].clone()


def guard_bytes(row_bytes, rows=8):
    return (rows * row_bytes + 255) // 256 * 256


def fp32_out(host_bytes, shape):
    t = host_bytes.view(torch.int32)
    assert bool((t != -1).all()), f"{int((t == -1).sum())} fp32 outputs were never written"
    return host_bytes.view(torch.float32).reshape(shape).clone()


def pair_out(host_bytes, rows, Cc):
    t = host_bytes.view(torch.int16)
    assert bool((t != -1).all()), f"{int((t == -1).sum())} fp16 plane entries were never written"
    return ph.pair_planes_to_f64(host_bytes, rows, Cc)


def mx8_out(host_bytes, rows, Cc):
    """-> (dequantised fp64, scale bytes).  Every e4m3 byte and every scale byte of a real block written; the padding between the two
    regions and the scale bytes of blocks past C (C % 128 != 0) still 0xFF."""
    n = rows * Cc
    off, nsc = ph.mx8_scale_offset(n), (Cc + 127) // 128
    assert host_bytes.numel() == off + rows * nsc * 4
    assert bool((host_bytes[:n] != 0xFF).all()), "e4m3 bytes never written"
    assert bool((host_bytes[n:off] == 0xFF).all())
    sw = host_bytes[off:].reshape(rows, nsc * 4)
    assert bool((sw[:, : Cc // 32] != 0xFF).all()), "scale bytes never written"
    assert bool((sw[:, Cc // 32:] == 0xFF).all()), "scale bytes of blocks that do not exist were written"
    return ph.mx8_to_f64(host_bytes, rows, Cc)


# ----------------------------------------------------------------------------------------------------------------- fp64 references
def snake64(x64, alpha):
    a = alpha.double()
    return x64 + (a + 1e-9).reciprocal() * torch.sin(a * x64) ** 2


def snake64_of_raw(raw32, alpha):
    """fp64 Snake of an fp32 tensor on the fp32 product alpha x — the argument the kernel (and torch fp32) takes the sine of."""
    a = alpha.double()
    return raw32.double() + (a + 1e-9).reciprocal() * torch.sin((alpha.float() * raw32).double()) ** 2


def conv_cl64(x64, w64, bias64, dilation):
    """Conv1d, 'same' padding, channels last, as shifted matrix products: x (B, L, Cin), w (Cout, Cin, k) -> (B, L, Cout) fp64."""
    B, Ln, _ = x64.shape
    k = w64.shape[2]
    out = bias64.expand(B, Ln, w64.shape[0]).clone()
    for t in range(k):
        sh = (t - (k - 1) // 2) * dilation
        lo, hi = max(0, -sh), min(Ln, Ln - sh)
        if hi > lo:
            out[:, lo:hi] += x64[:, lo + sh: hi + sh] @ w64[:, :, t].t()
    return out


def effective_operands(precision, x, w, flat, unflat):
    """The numbers the kernel of `precision` multiplies (x fp32 activated input, w fp32 weight)."""
    xe = x
    if precision in ("mx8", "f16pair_w8"):
        w = unflat(quant.fp8_effective_weight(flat(w))).contiguous()
    if precision == "mx8":
        xe = quant.mx8_effective_activation(x)
    if precision == "f16":
        xe, w = x.half().float(), w.half().float()
    return xe, w


def two_clips(shape, g, scale=3.0):
    """(2, L, C) activations like test_codec_convolution_per_precision's, clip 1 = the same distribution x 100."""
    _, Ln, Cc = shape
    x = torch.randn(2, Ln, Cc, generator=g) * torch.rand(2, Ln, 1, generator=g) * scale
    x[1] *= 100.0
    return x


RECORD = {}      # (case class, quantity) -> (measured, bar) of the case closest to its bar


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = ["# codec kernels stage by stage against fp64 (tests/test_gpu_codec_stages.py): per (case class, quantity) the measured value of the",
             "# case closest to its bar, and that bar.  'abs': max |err| against REL x max |conv ref| of the clip; 'error / allowed': max over the",
             "# elements of |err| / the element's own allowed error; 'excluded share': mx8 elements on a rounding or scale boundary (cap 1e-3)"]
    for (cls, what), (m, bar) in sorted(RECORD.items()):
        lines.append(f"{cls:52s} | {what:42s} | measured {m:.3e} | bar {bar:.3e}")
    print("\n".join(lines))
    out = os.environ.get("VAURA_CODEC_STAGE_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def note(cls, what, measured, bar):
    key = (cls, what)
    old = RECORD.get(key)
    if old is None or measured / bar > old[0] / old[1]:
        RECORD[key] = (measured, bar)
    print(f"[codec-stage] {cls} | {what}: measured {measured:.3e}  bar {bar:.3e}")


def check_raw(cls, got, ref_conv, res64, precision):
    """got (B, L, C) fp32 from the kernel; ref_conv fp64 = conv + bias; res64 the residual or None."""
    total = ref_conv if res64 is None else ref_conv + res64
    worst = 0.0
    for b in range(got.shape[0]):
        bar = RAW_REL[precision] * float(ref_conv[b].abs().max())
        err = (got[b].double() - total[b]).abs()
        if res64 is not None:
            err = (err - 2.0 ** -23 * total[b].abs()).clamp(min=0)
        note(cls, f"raw {precision} clip {b} (abs)", float(err.max()), bar)
        worst = max(worst, float(err.max()) / bar)
    assert worst <= 1.0, f"{cls} raw {precision}: error / bar = {worst:.3f}"


def raw_bar_abs(ref_conv, res64, precision):
    """(B, 1, 1)-broadcastable absolute raw bar per clip, and the total."""
    total = ref_conv if res64 is None else ref_conv + res64
    bar = RAW_REL[precision] * ref_conv.abs().amax(dim=(1, 2), keepdim=True)
    if res64 is not None:
        bar = bar + 2.0 ** -23 * total.abs()
    return bar, total


def act_reference(raw32, ref_conv, res64, alpha, precision):
    """-> (y fp64, allowed error E fp64) for the activated output: from the kernel's own raw output when it wrote one."""
    a = alpha.double() + 1e-9
    if raw32 is not None:
        y = snake64_of_raw(raw32, alpha)
        return y, 4e-7 / a + 2.0 ** -22 * y.abs() + 2.0 ** -25
    bar, total = raw_bar_abs(ref_conv, res64, precision)
    y = snake64(total, alpha)
    return y, 2.0 * bar + U24 * total.abs() + 4e-7 / a + 2.0 ** -22 * y.abs() + 2.0 ** -25


def check_act_plain(cls, act64, y, allowed, precision):
    ratio = float(((act64 - y).abs() / allowed).max())
    note(cls, f"act {precision} (error / allowed)", ratio, 1.0)
    assert ratio <= 1.0, f"{cls} act {precision}: error / allowed = {ratio:.3f}"


def check_act_mx8_exact(cls, deq, sb, y64):
    """The kernel's mx8 output against quant's rule on y64 = fp64 Snake of the kernel's own raw output (rows, C)."""
    rows, Cc = y64.shape
    y32 = y64.float()
    ref = quant.mx8_effective_activation(y32).double()
    ref_sb = ph.mx8_scale_bytes(y32)
    flips = lambda f: float(((quant.mx8_effective_activation(y32 * f).double() != ref).float().mean()))
    own_share = max(flips(1 + 1e-5), flips(1 - 1e-5))
    s_ref = torch.ldexp(torch.ones(rows, Cc // 32, dtype=torch.float64), ref_sb.to(torch.int32) - 127)
    r = y64.abs().reshape(rows, Cc // 32, 32).amax(dim=2) / (448.0 * s_ref)          # in (0.5, 1]
    near_blk = (r >= 1 - 1e-5) | (r <= 0.5 * (1 + 1e-5))
    dsb = sb.to(torch.int32) - ref_sb.to(torch.int32)
    bad_blk = dsb != 0
    assert bool((near_blk | ~bad_blk).all()), f"{cls}: {int((bad_blk & ~near_blk).sum())} scale bytes differ from quant's rule away from a boundary"
    assert bool((dsb.abs() <= 1).all())
    s_k = torch.ldexp(torch.ones(rows, Cc // 32, dtype=torch.float64), sb.to(torch.int32) - 127)
    s_big = torch.maximum(s_k, s_ref).repeat_interleave(32, dim=1)
    bad_el = bad_blk.repeat_interleave(32, dim=1)
    diff = (deq - ref).abs()
    lower = torch.minimum(deq.abs(), ref.abs()) / s_big
    one_step = diff <= ph.e4m3_step(lower) * s_big * (1 + 1e-12)
    mism = (deq != ref) & ~bad_el
    near_el = ((deq + ref) / 2 - y64).abs() <= 1e-5 * y64.abs()
    assert bool((one_step | ~(mism | bad_el)).all()), f"{cls}: an mx8 value is more than one grid step from the reference"
    assert bool((near_el | ~mism).all()), (f"{cls}: {int((mism & ~near_el).sum())} mx8 values differ although the exact value is not within "
                                            f"1e-5 of the rounding boundary")
    share = float((mism | bad_el).float().mean())
    print(f"[codec-stage] {cls} | mx8 act: excluded share, kernel {share:.2e}; reference under a 1e-5 perturbation {own_share:.2e}; "
          f"scale bytes off by one: {int(bad_blk.sum())}")
    note(cls, "act mx8 excluded share", share, 1e-3)
    assert share <= 1e-3, share


def check_act_mx8_bounded(cls, deq, sb, y64, E):
    """No raw output: the kernel's internal value is within E of y64; the scale byte is the rule's for some amax within E of the
    reference's, the value within E + half a grid step (at the kernel's scale) of y64."""
    rows, Cc = y64.shape
    Eb = E.expand(rows, Cc).reshape(rows, Cc // 32, 32).amax(dim=2)
    amax = y64.abs().reshape(rows, Cc // 32, 32).amax(dim=2)
    lo_sb = ph.mx8_scale_bytes(((amax - Eb).clamp(min=0) * (1 - 2.0 ** -23)).float().repeat_interleave(32, dim=1))
    hi_sb = ph.mx8_scale_bytes(((amax + Eb) * (1 + 2.0 ** -23)).float().repeat_interleave(32, dim=1))
    assert bool(((sb >= lo_sb) & (sb <= hi_sb)).all()), f"{cls}: a scale byte is outside what amax +- E allows"
    s_k = torch.ldexp(torch.ones(rows, Cc // 32, dtype=torch.float64), sb.to(torch.int32) - 127).repeat_interleave(32, dim=1)
    allowed = E + 0.5 * ph.e4m3_step((y64.abs() + E) / s_k) * s_k
    ratio = float(((deq - y64).abs() / allowed).max())
    note(cls, "act mx8 without raw (error / allowed)", ratio, 1.0)
    assert ratio <= 1.0, f"{cls}: mx8 act error / allowed = {ratio:.3f}"


def check_act(cls, precision, act_host, rows, Cc, raw32, ref_conv, res64, alpha):
    """act_host: the payload bytes of the activated output in the precision's own format; shapes (B, L, C) flattened to rows."""
    y, E = act_reference(raw32, ref_conv, res64, alpha, precision)
    y, E = y.reshape(rows, Cc), E.expand(y.shape).reshape(rows, Cc)
    if precision == "mx8":
        deq, sb = mx8_out(act_host, rows, Cc)
        if raw32 is not None:
            check_act_mx8_exact(cls, deq, sb, y)
        else:
            check_act_mx8_bounded(cls, deq, sb, y, E)
    elif precision == "f32":
        check_act_plain(cls, fp32_out(act_host, (rows, Cc)).double(), y, E, precision)
    else:
        check_act_plain(cls, pair_out(act_host, rows, Cc)[0], y, E, precision)


# ------------------------------------------------------------------------------------- a. epilogues of the 128-row instances
# (Cin, Cout, k, dilation, stride, combination)
_EPILOGUE_CASES = [(96, 96, 7, 9, 1, "act"), (192, 192, 7, 3, 1, "act"), (96, 96, 1, 1, 1, "res_raw_act"), (96, 96, 1, 1, 1, "res_act"),
                   (384, 192, 8, 1, 4, "up"), (192, 96, 4, 1, 2, "up")]
_EPILOGUE_64 = [(64, 64, 7, 9, 1, "act"), (128, 128, 1, 1, 1, "res_raw_act"), (128, 128, 1, 1, 1, "res_act")]
_EPILOGUE_PARAMS = [(c, p) for c in _EPILOGUE_CASES for p in PRECISIONS] + [(c, "f16pair") for c in _EPILOGUE_64]


@pytest.mark.parametrize("case,precision", _EPILOGUE_PARAMS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_conv_epilogues(case, precision):
    """One convolution with the epilogue the codec launches it with (act only: conv_in and a unit's 7-tap conv; res + raw + act: a unit's
    1 x 1 conv, u < 2; res + act: u = 2; transposed raw + act: the up conv), per instance class and precision.  Stride 1: L = 2 x 128 + 37
    (two full tiles and a ragged one; the dilation-9 halo crosses both boundaries); transposed: Lin = 128 + 5 (jcount = Lin + 1 crosses a
    tile).  A launch geometry below the 256-row gate: vaura_debug_counter(0) must stay 0."""
    from vaura_amd.engine import CodecConvOp, codec_act_bytes
    cin, cout, k, dil, stride, combo = case
    cls = f"epilogue {'x'.join(map(str, case[:5]))} {combo}"
    g = torch.Generator().manual_seed(1000 + cin * 7 + cout + k + dil + len(combo))
    B, Lin = 2, 2 * 128 + 37 if stride == 1 else 128 + 5
    Lout = Lin * stride
    x = two_clips((B, Lin, cin), g)
    bias = torch.randn(cout, generator=g) * 0.1
    alpha = torch.rand(cout, generator=g) * 3 + 0.05
    if stride > 1:
        w = torch.randn(cin, cout, k, generator=g) / (cin * 2) ** 0.5
        flat, unflat = (lambda t: t.permute(1, 0, 2).reshape(cout, -1)), (lambda t: t.reshape(cout, cin, k).permute(1, 0, 2))
    else:
        w = torch.randn(cout, cin, k, generator=g) / (cin * k) ** 0.5
        flat, unflat = (lambda t: t.reshape(cout, -1)), (lambda t: t.reshape(cout, cin, k))
    res = two_clips((B, Lout, cout), g, scale=1.0) if combo.startswith("res") else None
    xe, w = effective_operands(precision, x, w, flat, unflat)
    xd, wd = xe.double().transpose(1, 2), w.double()
    if stride > 1:
        ref = F.conv_transpose1d(xd, wd, bias.double(), stride=stride, padding=(stride + 1) // 2)
    else:
        ref = F.conv1d(xd, wd, bias.double(), dilation=dil, padding=(k - 1) // 2 * dil)
    ref = ref.transpose(1, 2).contiguous()
    assert ref.shape == (B, Lout, cout)
    res64 = None if res is None else res.double()

    want_raw = combo in ("res_raw_act", "up")
    rows = B * Lout
    raw_g = Guarded(rows * cout * 4, guard_bytes(cout * 4)) if want_raw else None
    act_g = Guarded(codec_act_bytes(precision, rows, cout), guard_bytes(cout * 4))
    op = CodecConvOp(w, bias, dil, stride, precision, DEV)
    L.lib().vaura_debug_counter(0)
    op.ex(x.to(DEV), res=None if res is None else res.to(DEV), alpha=alpha.to(DEV),
          out_raw=None if raw_g is None else raw_g.view(torch.float32), out_act=act_g.view())
    torch.cuda.synchronize()
    assert int(L.lib().vaura_debug_counter(0)) == 0
    raw32 = None
    if want_raw:
        raw32 = fp32_out(raw_g.host(), (B, Lout, cout))
        check_raw(cls, raw32, ref, res64, precision)
    check_act(cls, precision, act_g.host(), rows, cout, raw32, ref, res64, alpha)


# --------------------------------------------------------------------------------- b. the large instances against fp64
@functools.lru_cache(maxsize=None)
def _unit_problem(Cc):
    """Inputs of one residual unit at the smallest length that passes the gx x B >= 384 gate with a ragged last workgroup."""
    Ln = 191 * (256 if Cc == 96 else 128) + 37
    dil = 9 if Cc == 96 else 3
    g = torch.Generator().manual_seed(4000 + Cc)
    res = two_clips((2, Ln, Cc), g, scale=1.0)
    alpha_in = torch.rand(Cc, generator=g) * 3 + 0.05
    x = snake64_of_raw(res, alpha_in).float()          # what the producer of the unit's input hands over
    w7 = torch.randn(Cc, Cc, 7, generator=g) / (Cc * 7) ** 0.5
    w1 = torch.randn(Cc, Cc, 1, generator=g) / Cc ** 0.5
    b7, b1 = torch.randn(Cc, generator=g) * 0.1, torch.randn(Cc, generator=g) * 0.1
    alpha_mid, alpha_next = torch.rand(Cc, generator=g) * 3 + 0.05, torch.rand(Cc, generator=g) * 3 + 0.05
    return Ln, dil, x, res, w7, b7, w1, b1, alpha_mid, alpha_next


@pytest.mark.parametrize("precision", ["f16pair", "f16pair_w8", "f16"])
@pytest.mark.parametrize("Cc", [96, 192])
def test_large_instances_against_fp64(Cc, precision):
    """One residual unit as ONE launch (C = 96: conv_pair_kernel<.., 8, true>, L = 191 x 256 + 37; C = 192: conv_unit_kernel<12, 2, ..>,
    L = 191 x 128 + 37) against fp64 and against the two-launch form (CODEC_UNIT_TWO_LAUNCHES), bit for bit.  The fp64 reference follows the
    stages on the numbers the kernels multiply: the first conv's activated output (kept by the two-launch run) against Snake of the fp64
    conv, the unit's output against fp64 of res + conv1(that activated output — its hi planes for "f16").  At C = 96 the 7-tap conv also
    runs alone through vaura_dac_conv_ex on the 256-row instance (vaura_debug_counter(0) > 0) and is held to the same bars."""
    from vaura_amd.engine import CodecConvOp, CodecUnitOp, codec_act_bytes
    Ln, dil, x, res, w7, b7, w1, b1, alpha_mid, alpha_next = _unit_problem(Cc)
    cls = f"large C={Cc} L={Ln}"
    B, rows = 2, 2 * Ln
    flat, unflat7, unflat1 = (lambda t: t.reshape(Cc, -1)), (lambda t: t.reshape(Cc, Cc, 7)), (lambda t: t.reshape(Cc, Cc, 1))
    xe, w7e = effective_operands(precision, x, w7, flat, unflat7)
    _, w1e = effective_operands(precision, x[:, :1], w1, flat, unflat1)
    ref7 = conv_cl64(xe.double(), w7e.double(), b7.double(), dil)

    lib = L.lib()
    unit = CodecUnitOp(w7e, b7, dil, w1e, b1, precision, DEV)
    xd, resd = x.to(DEV), res.to(DEV)
    am, an = alpha_mid.to(DEV), alpha_next.to(DEV)
    gb = guard_bytes(Cc * 4)
    outs = {}
    for form, flags in (("one", 0), ("two", Variant.CODEC_UNIT_TWO_LAUNCHES)):
        with variants(flags):
            lib.vaura_debug_counter(0)
            lib.vaura_debug_counter(1)
            raw_g, act_g = Guarded(rows * Cc * 4, gb), Guarded(codec_act_bytes(precision, rows, Cc), gb)
            mid_g = Guarded(codec_act_bytes(precision, rows, Cc), gb) if form == "two" else None
            fused = unit(xd, resd, am, an, raw_g.view(torch.float32), act_g.view(), None if mid_g is None else mid_g.view())
            torch.cuda.synchronize()
            n_fused, n_256 = int(lib.vaura_debug_counter(1)), int(lib.vaura_debug_counter(0))
            if form == "one":
                assert fused and n_fused == 1 and n_256 == 0, (fused, n_fused, n_256)
            else:
                assert not fused and n_fused == 0 and n_256 == 2, (fused, n_fused, n_256)
            outs[form] = (raw_g.host(), act_g.host(), None if mid_g is None else mid_g.host())
    conv_alone = None
    if Cc == 96:
        lib.vaura_debug_counter(0)
        alone_g = Guarded(codec_act_bytes(precision, rows, Cc), gb)
        CodecConvOp(w7e, b7, dil, 1, precision, DEV).ex(xd, alpha=am, out_act=alone_g.view())
        torch.cuda.synchronize()
        assert int(lib.vaura_debug_counter(0)) > 0
        conv_alone = alone_g.host()
    assert torch.equal(outs["one"][0], outs["two"][0]), "raw output: one launch != two launches"
    assert torch.equal(outs["one"][1], outs["two"][1]), "activated output: one launch != two launches"

    # the first conv's activated output (no raw output there)
    mid, mid_hi, _ = pair_out(outs["two"][2], rows, Cc)
    y, E = act_reference(None, ref7, None, alpha_mid, precision)
    check_act_plain(cls + " conv7 (in the unit)", mid, y.reshape(rows, Cc), E.reshape(rows, Cc), precision)
    if conv_alone is not None:
        alone = pair_out(conv_alone, rows, Cc)[0]
        check_act_plain(cls + " conv7 alone, 256-row instance", alone, y.reshape(rows, Cc), E.reshape(rows, Cc), precision)
    # the unit's output on the activation the second conv read
    mid_used = (mid_hi if precision == "f16" else mid).reshape(B, Ln, Cc)
    ref1 = mid_used @ w1e.double()[:, :, 0].t() + b1.double()
    raw32 = fp32_out(outs["one"][0], (B, Ln, Cc))
    check_raw(cls + " unit", raw32, ref1, res.double(), precision)
    check_act(cls + " unit", precision, outs["one"][1], rows, Cc, raw32, ref1, res.double(), alpha_next)


# ------------------------------------------------------------------------------- b2. the 256-row gate, on both sides of it
# launch_conv takes the 256-row instances when g256 x column tiles x B x phases >= 384, g256 = ceil(jcount / 256); launch_conv_unit
# the one-launch unit (C = 96) when ceil(L / 256) x B >= 384.  (name, Cin, Cout, k, dilation, stride, precisions, ((Lin, product), ..))
_PAIR3 = ("f16pair", "f16pair_w8", "f16")
_GATE_CASES = [("one-tap", 96, 192, 1, 1, 1, _PAIR3, ((24576, 384), (24320, 380))),             # 96 x 2 tiles x 2 clips / 95 x 2 x 2
               ("64-columns", 64, 128, 1, 1, 1, _PAIR3[:2], ((24576, 384), (24320, 380))),      # the f16 mode has no 64-column 256-row instance
               ("transposed", 96, 96, 4, 1, 2, _PAIR3, ((24320, 384), (24319, 380)))]           # jcount = Lin + 1: 96 / 95 x 1 x 2 x 2 phases
_GATE_PARAMS = [(c[:6], p, Lin, prod) for c in _GATE_CASES for p in c[6] for Lin, prod in c[7]]


@functools.lru_cache(maxsize=None)
def _gate_problem(case, Lin):
    _, cin, cout, k, _, stride = case
    g = torch.Generator().manual_seed(8000 + cin + cout + k + stride)
    x = two_clips((2, Lin, cin), g)
    w = torch.randn(cin, cout, k, generator=g) / (cin * 2) ** 0.5 if stride > 1 else torch.randn(cout, cin, k, generator=g) / (cin * k) ** 0.5
    return x, w, torch.randn(cout, generator=g) * 0.1, torch.rand(cout, generator=g) * 3 + 0.05


@pytest.mark.parametrize("case,precision,Lin,product", _GATE_PARAMS, ids=lambda v: str(v) if isinstance(v, (str, int)) else v[0])
def test_256_row_gate_of_the_conv_launcher(case, precision, Lin, product):
    """vaura_dac_conv_ex at the two lengths either side of the gate, per instance family (96-column tiles, 64-column tiles, the two phases
    of a transposed conv with its jcount = Lin + 1) and pair precision: vaura_debug_counter(0) reads 1 at a product of exactly 384 and 0
    at 380, and 0 under CODEC_128_ROWS (128-row instances only); the activated output of the two runs is equal byte for byte and the
    guards are intact.  No fp64 reference: the smaller shapes above carry the numeric bars.  The largest tensor of a case is 37.7 MB."""
    from vaura_amd.engine import CodecConvOp, codec_act_bytes
    name, cin, cout, k, dil, stride = case
    ph_count, tiles = (stride if stride > 1 else 1), cout // (96 if cout % 96 == 0 else 64)
    jcount = Lin + 1 if stride > 1 else Lin
    assert -(-jcount // 256) * tiles * 2 * ph_count == product       # the case is what its comment says
    x, w, bias, alpha = _gate_problem(case, Lin)
    flat = (lambda t: t.permute(1, 0, 2).reshape(cout, -1)) if stride > 1 else (lambda t: t.reshape(cout, -1))
    unflat = (lambda t: t.reshape(cout, cin, k).permute(1, 0, 2)) if stride > 1 else (lambda t: t.reshape(cout, cin, k))
    _, we = effective_operands(precision, x[:, :1], w, flat, unflat)
    rows = 2 * Lin * stride
    lib = L.lib()
    op = CodecConvOp(we, bias, dil, stride, precision, DEV)
    xd, ad = x.to(DEV), alpha.to(DEV)
    outs, counts = [], []
    for flags in (0, Variant.CODEC_128_ROWS):
        with variants(flags):
            lib.vaura_debug_counter(0)
            act_g = Guarded(codec_act_bytes(precision, rows, cout), guard_bytes(cout * 4))
            op.ex(xd, alpha=ad, out_act=act_g.view())
            torch.cuda.synchronize()
            counts.append(int(lib.vaura_debug_counter(0)))
            outs.append(act_g.host())
            del act_g
    print(f"[codec-stage] gate {name} {precision} Lin={Lin}: product {product}, 256-row launches {counts[0]} (CODEC_128_ROWS: {counts[1]})")
    assert counts == [1 if product >= 384 else 0, 0], counts
    assert bool((outs[0].view(torch.int16) != -1).all()), "fp16 plane entries were never written"
    assert torch.equal(outs[0], outs[1]), "256-row / 128-row selection changed the output"


@pytest.mark.parametrize("precision", _PAIR3)
@pytest.mark.parametrize("Ln,product", [(49152, 384), (48896, 382)])
def test_256_row_gate_of_the_unit_launcher(Ln, product, precision):
    """vaura_dac_unit, C = 96, 7 taps of dilation 9, B = 2, either side of ceil(L / 256) x B >= 384: vaura_debug_counter(1) reads 1 at 384
    (one launch) and 0 at 382, where the unit runs as two convs whose own products are 382 as well (counter 0 == 0).  Under
    CODEC_UNIT_TWO_LAUNCHES (always two launches) the output is equal byte for byte; at 384 those two convs take the 256-row instances (counter 0 == 2)."""
    from vaura_amd.engine import CodecUnitOp, codec_act_bytes
    Cc, dil = 96, 9
    assert -(-Ln // 256) * 2 == product
    g = torch.Generator().manual_seed(8800)
    res = two_clips((2, Ln, Cc), g, scale=1.0)
    x = two_clips((2, Ln, Cc), g)
    w7, w1 = torch.randn(Cc, Cc, 7, generator=g) / (Cc * 7) ** 0.5, torch.randn(Cc, Cc, 1, generator=g) / Cc ** 0.5
    b7, b1 = torch.randn(Cc, generator=g) * 0.1, torch.randn(Cc, generator=g) * 0.1
    am, an = (torch.rand(Cc, generator=g) * 3 + 0.05).to(DEV), (torch.rand(Cc, generator=g) * 3 + 0.05).to(DEV)
    flat = lambda t: t.reshape(Cc, -1)
    _, w7e = effective_operands(precision, x[:, :1], w7, flat, lambda t: t.reshape(Cc, Cc, 7))
    _, w1e = effective_operands(precision, x[:, :1], w1, flat, lambda t: t.reshape(Cc, Cc, 1))
    rows, gb = 2 * Ln, guard_bytes(Cc * 4)
    lib = L.lib()
    unit = CodecUnitOp(w7e, b7, dil, w1e, b1, precision, DEV)
    xd, resd = x.to(DEV), res.to(DEV)
    mid = torch.empty(codec_act_bytes(precision, rows, Cc), dtype=torch.uint8, device=DEV)
    outs, seen = [], []
    for flags in (0, Variant.CODEC_UNIT_TWO_LAUNCHES):
        with variants(flags):
            lib.vaura_debug_counter(0)
            lib.vaura_debug_counter(1)
            act_g = Guarded(codec_act_bytes(precision, rows, Cc), gb)
            fused = unit(xd, resd, am, an, None, act_g.view(), mid)
            torch.cuda.synchronize()
            seen.append((fused, int(lib.vaura_debug_counter(1)), int(lib.vaura_debug_counter(0))))
            outs.append(act_g.host())
            del act_g
    print(f"[codec-stage] gate unit {precision} L={Ln}: product {product}, (one launch, counter 1, counter 0) = {seen[0]}; CODEC_UNIT_TWO_LAUNCHES: {seen[1]}")
    big = product >= 384
    assert seen == [(big, 1 if big else 0, 0), (False, 0, 2 if big else 0)], seen
    assert bool((outs[0].view(torch.int16) != -1).all()), "fp16 plane entries were never written"
    assert torch.equal(outs[0], outs[1]), "one launch != two launches"


# ----------------------------------------------------------------------------------------------------------------- c. from_codes
@pytest.mark.parametrize("pairs", [False, True], ids=["fp32", "pairs"])
@pytest.mark.parametrize("K,dim,latent", [(9, 8, 1024), (4, 5, 1024)])
def test_from_codes(K, dim, latent, pairs):
    """from_codes_kernel: T = 19 = two full groups of FC_NT = 8 frames and three more; dim = 5 takes the dim < 8 path; codes 0 and
    size - 1 are present in both clips.  (Codes have no scale: the two clips differ in their codes only.)  fp32 chain of 9 x (8 products +
    bias) sums: n = 81."""
    from vaura_amd.engine import codec_from_codes
    size, B, T = 1024, 2, 19
    g = torch.Generator().manual_seed(K * 100 + dim)
    codes = torch.randint(0, size, (B, K, T), generator=g, dtype=torch.int32)
    codes[0, 0, 0], codes[0, K - 1, T - 1], codes[1, 0, T - 1], codes[1, K - 1, 0], codes[1, 1, 16] = 0, size - 1, size - 1, 0, size - 1
    cb = torch.randn(K, size, dim, generator=g)
    pw = torch.randn(K, latent, dim, generator=g) / dim ** 0.5
    pb = torch.randn(K, latent, generator=g) * 0.1
    e = torch.stack([cb[k][codes[:, k].long()] for k in range(K)], dim=2).double()            # (B, T, K, dim)
    terms = torch.einsum("btkd,kcd->btkcd", e, pw.double())
    ref = terms.sum(dim=(2, 4)) + pb.double().sum(0)
    mag = terms.abs().sum(dim=(2, 4)) + pb.double().abs().sum(0)
    allowed = 81 * U24 * mag
    rows = B * T
    out = Guarded(rows * latent * 4, guard_bytes(latent * 4, 2))
    codec_from_codes(codes.to(DEV), cb.to(DEV), pw.to(DEV), pb.to(DEV), out.view(torch.float32), pairs)
    torch.cuda.synchronize()
    if pairs:
        got = pair_out(out.host(), rows, latent)[0].reshape(B, T, latent)
        allowed = allowed + 2.0 ** -22 * ref.abs() + 2.0 ** -25
    else:
        got = fp32_out(out.host(), (B, T, latent)).double()
    ratio = float(((got - ref).abs() / allowed).max())
    note(f"from_codes K={K} dim={dim}", "pairs" if pairs else "fp32", ratio, 1.0)
    assert ratio <= 1.0, ratio


# ----------------------------------------------------------------------------------------------------------------- d. conv_out
@pytest.mark.parametrize("precision", ["f32", "f16pair", "mx8"])
@pytest.mark.parametrize("Cc,untiled_flag", [(96, False), (96, True), (160, False)], ids=["C96-tiled", "C96-untiled", "C160-untiled"])
def test_conv_out(Cc, untiled_flag, precision):
    """The last conv (C -> 1, k = 7, tanh) on an input stored as fp32, pair planes or mx8: conv_out_tiled_kernel (C = 96), conv_out_kernel
    by CODEC_LAST_CONV_UNTILED and by shape (C = 160 > 128); L = 2 x 128 + 37.  Reference: tanh of the fp64 sum over the input AS STORED.  fp32
    chain: n = 7 C + 8; the pre-activation bound goes through tanh exactly (monotone), + 2^-21 for tanhf."""
    from vaura_amd.engine import codec_conv_out
    B, Ln = 2, 2 * 128 + 37
    g = torch.Generator().manual_seed(7000 + Cc)
    x = two_clips((B, Ln, Cc), g)
    w = torch.randn(1, Cc, 7, generator=g) / (Cc * 7) ** 0.5
    bias = torch.randn(1, generator=g) * 0.1
    if precision == "mx8":
        xs = quant.mx8_effective_activation(x).double()
    elif precision == "f16pair":
        hi = x.half()
        xs = hi.double() + (x - hi.float()).half().double()
    else:
        xs = x.double()
    wd = w.double()
    pre = F.conv1d(xs.transpose(1, 2), wd, bias.double(), padding=3)[:, 0]
    mag = F.conv1d(xs.abs().transpose(1, 2), wd.abs(), bias.double().abs(), padding=3)[:, 0]
    Epre = (7 * Cc + 8) * U24 * mag
    ref = torch.tanh(pre)
    allowed = torch.maximum(torch.tanh(pre + Epre) - ref, ref - torch.tanh(pre - Epre)) + 2.0 ** -21
    out = Guarded(B * Ln * 4, 256)
    with variants(Variant.CODEC_LAST_CONV_UNTILED if untiled_flag else 0):
        codec_conv_out(w, bias, x.to(DEV), out.view(torch.float32).reshape(B, Ln), precision)
        torch.cuda.synchronize()
    got = fp32_out(out.host(), (B, Ln)).double()
    ratio = float(((got - ref).abs() / allowed).max())
    note(f"conv_out C={Cc}{' CODEC_LAST_CONV_UNTILED' if untiled_flag else ''}", precision, ratio, 1.0)
    print(f"[codec-stage] conv_out C={Cc} {precision}: max |err| clip 0 {float((got - ref)[0].abs().max()):.2e}, clip 1 {float((got - ref)[1].abs().max()):.2e}")
    assert ratio <= 1.0, ratio


# ----------------------------------------------------------------------------------------------------------------- e. enc_conv_in
def test_enc_conv_in():
    """enc_conv_in_kernel (1 -> 64 channels, k = 7, pad 3) at L = 1003: raw fp32 output (chain of 7 products + bias: n = 8) and Snake of
    it as pair planes, both zero-padded ends included (rows 0..2 and L-3..L-1 read outside the clip)."""
    from vaura_amd.engine import codec_enc_conv_in
    B, Ln, Cc = 2, 1003, 64
    g = torch.Generator().manual_seed(64)
    wav = torch.randn(B, Ln, generator=g) * 0.3
    wav[1] *= 100.0
    w = torch.randn(7, Cc, generator=g) / 7 ** 0.5
    bias = torch.randn(Cc, generator=g) * 0.1
    alpha = torch.rand(Cc, generator=g) * 3 + 0.05
    wd = w.double().t()[:, None, :]                                                   # (C, 1, 7)
    ref = F.conv1d(wav.double()[:, None], wd, bias.double(), padding=3).transpose(1, 2)
    mag = F.conv1d(wav.double().abs()[:, None], wd.abs(), bias.double().abs(), padding=3).transpose(1, 2)
    rows = B * Ln
    raw_g, act_g = Guarded(rows * Cc * 4, guard_bytes(Cc * 4)), Guarded(rows * Cc * 4, guard_bytes(Cc * 4))
    codec_enc_conv_in(wav.to(DEV), w.to(DEV), bias.to(DEV), alpha.to(DEV), raw_g.view(torch.float32), act_g.view())
    torch.cuda.synchronize()
    raw32 = fp32_out(raw_g.host(), (B, Ln, Cc))
    ratio = float(((raw32.double() - ref).abs() / (8 * U24 * mag)).max())
    note("enc_conv_in", "raw (error / allowed)", ratio, 1.0)
    assert ratio <= 1.0, ratio
    for rws in (slice(0, 3), slice(Ln - 3, Ln)):
        assert float(((raw32.double() - ref)[:, rws].abs() / (8 * U24 * mag[:, rws])).max()) <= 1.0
    y = snake64_of_raw(raw32, alpha).reshape(rows, Cc)
    allowed = 4e-7 / (alpha.double() + 1e-9) + 2.0 ** -22 * y.abs() + 2.0 ** -25
    check_act_plain("enc_conv_in", pair_out(act_g.host(), rows, Cc)[0], y, allowed, "f16pair")


# ----------------------------------------------------------------------------------------------------------------- f. rvq_stage
@functools.lru_cache(maxsize=None)
def _rvq_problem():
    K, dim, latent, size, B, T = 9, 8, 1024, 1024, 2, 152
    g = torch.Generator().manual_seed(9)
    in_w = torch.randn(K, dim, latent, generator=g) / latent ** 0.5
    in_b = torch.randn(K, dim, generator=g) * 0.1
    cb = torch.randn(K, size, dim, generator=g)
    out_w = torch.randn(K, latent, dim, generator=g) / dim ** 0.5
    out_b = torch.randn(K, latent, generator=g) * 0.1
    residual = torch.randn(B, T, latent, generator=g)
    residual[1] *= 100.0
    return K, dim, latent, size, B, T, in_w, in_b, cb, out_w, out_b, residual


@pytest.mark.parametrize("k", [0, 4, 8])
def test_rvq_stage(k):
    """ONE rvq_stage_kernel launch (304 rows, latent 1024, dim 8, 1024 codes) on a given residual, for stages 0, 4 and 8 of a synthetic
    9-stage quantiser, against an fp64 restatement of one stage of oracle/dac_oracle.py::quantize.  The code equals the fp64 choice
    except on near-ties (fp64 best and second-best distance within 1e-5: either of the two; at most 1 % of the rows, and the reference's
    own share is asserted to be at most a tenth of that).  The updated residual is checked on every row whose code agrees: fp32 chain of
    8 products + bias + the subtraction (n = 10) plus the rounding of z_e + (c - z_e), 2^-23 (|c| + |z_e|) per component."""
    from vaura_amd.engine import codec_rvq_stage
    K, dim, latent, size, B, T, in_w, in_b, cb, out_w, out_b, residual = _rvq_problem()
    rows = B * T
    r64 = residual.double().reshape(rows, latent)
    ze = r64 @ in_w[k].double().t() + in_b[k].double()
    enc = ze / ze.norm(dim=1, keepdim=True).clamp(min=1e-12)
    cbd = cb[k].double()
    cbn = cbd / cbd.norm(dim=1, keepdim=True).clamp(min=1e-12)
    dist = enc.pow(2).sum(1, keepdim=True) - 2 * enc @ cbn.t() + cbn.pow(2).sum(1, keepdim=True).t()
    top = (-dist).topk(2, dim=1)
    best, second = top.indices[:, 0], top.indices[:, 1]
    near = (top.values[:, 0] - top.values[:, 1]) < 1e-5
    assert float(near.float().mean()) <= 1e-3, "reseed: the reference's own near-tie share is above a tenth of the cap"

    res_g = Guarded(rows * latent * 4, guard_bytes(latent * 4, 2))
    codes_g = Guarded(B * K * T * 4, 256)
    res_g.view(torch.float32).copy_(residual.reshape(-1).to(DEV))
    codec_rvq_stage(res_g.view(torch.float32).reshape(B, T, latent), in_w[k].contiguous().to(DEV), in_b[k].contiguous().to(DEV),
                    cb[k].contiguous().to(DEV), out_w[k].contiguous().to(DEV), out_b[k].contiguous().to(DEV),
                    codes_g.view(torch.int32).reshape(B, K, T), k)
    torch.cuda.synchronize()
    codes = codes_g.host().view(torch.int32).reshape(B, K, T)
    other = [j for j in range(K) if j != k]
    assert bool((codes[:, other] == -1).all()), "a code plane of another stage was written"
    got = codes[:, k].reshape(rows).long()
    assert bool(((got >= 0) & (got < size)).all())
    agree = got == best
    ok = agree | (near & (got == second))
    print(f"[codec-stage] rvq stage {k}: {int((~agree).sum())} of {rows} codes differ from the fp64 choice, near-tie rows {int(near.sum())}; "
          f"smallest fp64 margin {float((top.values[:, 0] - top.values[:, 1]).min()):.2e}")
    assert bool(ok.all()), f"{int((~ok).sum())} codes differ from the fp64 choice away from a tie"
    assert float(near.float().mean()) <= 1e-2
    new = fp32_out(res_g.host(), (rows, latent)).double()
    c = cbd[best]
    owd = out_w[k].double()
    ref = r64 - (c @ owd.t() + out_b[k].double())
    mag = c.abs() @ owd.abs().t() + out_b[k].double().abs() + r64.abs()
    allowed = 10 * U24 * mag + (2.0 ** -23 * (c.abs() + ze.abs())) @ owd.abs().t()
    ratio = float((((new - ref).abs() / allowed)[agree]).max())
    note("rvq_stage", f"stage {k} residual (error / allowed)", ratio, 1.0)
    assert ratio <= 1.0, ratio

