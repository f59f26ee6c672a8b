"""CPU checks (-m "not gpu") of the format decoders the codec stage parity tests read kernel outputs with
(tests/parity_helpers.py: pair planes, block-scaled e4m3), against vaura_amd.quant and a host restatement of the layouts written
element by element from csrc/conv_kernels.h::store_act_octet — a decoder bug must not pass as a kernel bug, nor hide one — and of what the
op-level entry points refuse without a GPU."""
import torch

import parity_helpers as ph
from vaura_amd import _lib as L
from vaura_amd import quant


def _pair_buffer(x):
    """store_act_octet, fmt 0, one element at a time: hi = fp16(x), lo = fp16(x - hi) at ((row * C/8 + c/8) * 2 + plane) * 8 + c % 8."""
    rows, Cc = x.shape
    buf = torch.zeros(rows * Cc * 2, dtype=torch.float16)
    hi = x.half()
    lo = (x - hi.float()).half()
    for r in range(rows):
        for c in range(Cc):
            base = ((r * (Cc >> 3) + (c >> 3)) * 2) * 8 + (c & 7)
            buf[base] = hi[r, c]
            buf[base + 8] = lo[r, c]
    return buf, hi, lo


def _mx8_buffer(x):
    """store_act_octet, fmt 1, one block at a time: bytes at row * C + c, the scale byte of block j at (row * ceil(C/128) + j/4) * 4 + j%4
    behind the padded bytes; the scale by the kernel's own integer rule (mx8_scale_byte), not by quant's frexp."""
    rows, Cc = x.shape
    nsc = (Cc + 127) >> 7
    off = (rows * Cc + 15) & ~15
    buf = torch.full((off + rows * nsc * 4,), 0xEE, dtype=torch.uint8)
    for r in range(rows):
        for j in range(Cc // 32):
            blk = x[r, 32 * j: 32 * j + 32]
            bits = int(blk.abs().max().view(torch.int32))
            e8 = ((bits >> 23) & 0xFF) - (8 if (bits & 0x7FFFFF) <= 0x600000 else 7)
            e8 = min(max(e8, 1), 253)
            inv = torch.tensor(2.0 ** (127 - e8), dtype=torch.float32)
            buf[r * Cc + 32 * j: r * Cc + 32 * j + 32] = (blk * inv).to(torch.float8_e4m3fn).view(torch.uint8)
            buf[off + (r * nsc + (j >> 2)) * 4 + (j & 3)] = e8
    return buf


def _data(rows, Cc, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, Cc, generator=g) * torch.rand(rows, 1, generator=g) * 3
    x[0, :32] = 0.0                       # an all-zero block: the clamped scale byte
    x[1, 5] = 448.0 * 2.0 ** -3           # amax exactly on a scale boundary
    x[2, 40] = 449.0 * 2.0 ** -3          # and just above one
    x[3, :] *= 1e-30                      # tiny values
    return x


def test_pair_plane_decoder_matches_the_layout_and_the_split():
    for rows, Cc in ((7, 96), (5, 64), (4, 192)):
        x = _data(rows, Cc, rows * Cc)
        buf, hi, lo = _pair_buffer(x)
        val, dhi, dlo = ph.pair_planes_to_f64(buf, rows, Cc)
        assert torch.equal(dhi, hi.double()) and torch.equal(dlo, lo.double())
        assert torch.equal(val, hi.double() + lo.double())
        # the pair carries x to 2^-22 relative (two 11-bit significands) down to the fp16 subnormals' 2^-25 absolute
        assert bool(((val - x.double()).abs() <= 2.0 ** -22 * x.double().abs() + 2.0 ** -25).all())
        # trailing bytes of a larger buffer (guard rows) are not read
        big = torch.cat([buf, torch.full((64,), float("nan"), dtype=torch.float16)])
        assert torch.equal(ph.pair_planes_to_f64(big, rows, Cc)[0], val)


def test_mx8_decoder_matches_quant_and_the_layout():
    for rows, Cc in ((7, 96), (5, 64), (4, 192), (4, 384)):
        x = _data(rows, Cc, rows + Cc)
        buf = _mx8_buffer(x)
        val, sb = ph.mx8_to_f64(buf, rows, Cc)
        assert sb.shape == (rows, Cc // 32)
        assert torch.equal(val, quant.mx8_effective_activation(x).double())
        assert torch.equal(sb, ph.mx8_scale_bytes(x))       # quant's frexp rule == the kernel's integer rule, clamp included
        assert int(sb[0, 0]) == 1 and bool((val[0, :32] == 0).all())
        # the scale is the SMALLEST power of two with amax <= 448 s
        amax = x.reshape(rows, -1, 32).abs().amax(dim=2).double()
        s = torch.ldexp(torch.ones_like(amax), sb.to(torch.int32) - 127)
        live = sb > 1
        assert bool((amax <= 448 * s)[live].all()) and bool((amax > 224 * s)[live].all())


def test_e4m3_step_is_the_grid_spacing():
    q = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().double()
    q = torch.unique(q[torch.isfinite(q) & (q >= 0)])           # sorted; +0 and -0 are one grid point
    gaps = q[1:] - q[:-1]
    assert torch.equal(ph.e4m3_step(q[:-1]), gaps)           # the gap ABOVE every grid point
    assert float(ph.e4m3_step(torch.tensor([300.0]))) == 32.0 and float(ph.e4m3_step(torch.tensor([1e-9]))) == 2.0 ** -9


def test_stage_entry_points_report_argument_errors_without_a_gpu():
    lib = L.lib()
    cv = L.Conv()
    cv.cin, cv.cout, cv.taps, cv.dilation, cv.stride = 96, 96, 7, 1, 1
    assert lib.vaura_dac_conv_ex(None, 1, 0, 0, 0, 0, 0, 0, 2, 8, 0) == -1
    assert lib.vaura_dac_conv_ex(cv, 1, 16, 0, 0, 0, 0, 16, 2, 8, 0) == -1        # neither output
    assert lib.vaura_dac_conv_ex(cv, 5, 16, 0, 0, 16, 0, 16, 2, 8, 0) == -1       # precision
    assert lib.vaura_dac_unit(cv, cv, 1, 16, 0, 16, 16, 0, 16, 16, 0, 2, 8, 0) == -1   # no residual
    assert lib.vaura_dac_from_codes(0, 0, 0, 0, 0, 2, 9, 19, 1024, 8, 1024, 0, 0) == -1
    assert lib.vaura_dac_from_codes(16, 16, 16, 16, 16, 2, 17, 19, 1024, 8, 1024, 0, 0) == -2
    assert lib.vaura_dac_conv_out(cv, 1, 0, 0, 0, 2, 8, 0) == -1
    assert lib.vaura_dac_enc_conv_in(0, 0, 0, 0, 0, 0, 2, 100, 64, 0) == -1
    assert lib.vaura_dac_enc_conv_in(16, 16, 16, 16, 16, 16, 2, 100, 60, 0) == -2
    assert lib.vaura_dac_rvq_stage(0, 0, 0, 0, 0, 0, 0, 2, 152, 1024, 8, 1024, 9, 0, 0) == -1
    assert lib.vaura_dac_rvq_stage(16, 16, 16, 16, 16, 16, 16, 2, 152, 1024, 8, 1024, 9, 9, 0) == -1
    assert lib.vaura_dac_rvq_stage(16, 16, 16, 16, 16, 16, 16, 2, 152, 4096, 8, 1024, 9, 0, 0) == -2
    assert L.DAC_UNIT_TWO_LAUNCHES == -100
