"""Extractor kernels (csrc/vit.hip and the linear-layer launcher of csrc/linear.hip) op by op against torch fp64 on the CPU
(tests/vit_reference.py), through the op-level entry points that call the SAME static launchers as vaura_avclip_forward.

Conventions of every case
  * n_seg = 2 and segment 1's values (for attention: its v; for the space pattern also the v of every odd frame) are x 100: a read across a
    segment / frame boundary is an error of order 100 in units of the reading element's own max |v|.
  * Every output lives inside a larger allocation whose bytes are all 0xFF (fp32 / fp16 NaN, which no kernel writes for finite inputs): the
    guard bytes on either side and every row the op must not touch are still 0xFF afterwards, and no element it must write is.
  * Rows the op must not READ (CLS rows under LayerNorm's map 1, row 0 under embed) hold NaN.

Bars (derived; none is tuned on the kernels)
  data movement   patchify, fill_rows, embed: torch.equal with the same fp32 operations on the host (embed: x + (pos + temp), the kernel's
                  order; and |got - fp64| <= 2^-24 (|pos + temp| + |y|): its two roundings, i.e. one fp32 ulp of the larger).
  fp32 class      LayerNorm, the CLS and time patterns, the exact-fp32 MFMA, one-thread and generic space kernels: tests/test_gpu_attention.py's
                  rule err <= max(3e-6, 4 e_ref), err and e_ref (the plain fp32 torch restatement's error on the same case) relative to the
                  element's scale: max |v| over the element's own keys for attention, max |w x^| + max |b| of the row for LayerNorm.  A pair
                  output adds its representation error 2^-22 |y| + 2^-25.  One exception, LayerNorm on CONSTANT rows (variance 0, the
                  exact output is the bias): the 3e-6 floor is replaced by vit_reference.ln_constant_row_floor, the kernel's 22 fp32
                  roundings of the mean x |w| / sqrt(eps), per row — torch's pairwise sum of equal values can be exact (e_ref = 0 on one
                  row) where the kernel's order, like any other, leaves a few ulps of the mean that 1 / sqrt(eps) = 1000 multiplies.
  pair class      the default space kernel (q, k, p, v as (hi, lo) fp16 pairs): the fp32-class bar plus, in units of max |v|,
                      2 x [3 x 2^-22 x 0.125 max_keys sum_i |q_i| |k_i|] + 3 x 2^-22
                  (vit_reference.pair_attention_apriori: a three-product score of two 22-bit operands is off by at most 3 x 2^-22 of its
                  sum of magnitudes; scores within +-e move an output by at most 2 e max |v|; p and v are 22-bit operands in turn),
                  computed per element from the inputs.  The three space kernels also agree pairwise within the sum of their bars.
  linear          the project's pair-GEMM bar (test_codec_convolution_per_precision, tests/test_gpu_codec_stages.py 'raw'):
                  |err| <= 2e-6 max |x W^T + b| of the sequence (+ 2^-23 |out| for the residual's one fp32 add), against fp64 on the
                  pair values of x and W.  The GELU output: that bar through GELU's Lipschitz constant 1.13, plus the GELU bar below.
  GELU            against fp64 0.5 x (1 + erf(x / sqrt 2)) on arguments the epilogue receives exactly:
                  |err| <= 1.3e-7 max(1, |x|) + 2^-22 |y| + 2^-25 (the kernel's stated bound + the planes' representation error), and the
                  sign is right wherever the fp64 value rounds to a nonzero pair.
Measured values next to these bars: set VAURA_AVCLIP_PARITY_OUT=<file> (profiles/avclip_op_parity.txt is such a file)."""
import ctypes as C
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import vit_reference as R
from vaura_amd import _lib as L
from vaura_amd.variants import Variant, variants

DEV = "cuda:0"
D, NF, HEADS = R.D, R.NF, R.HEADS
GELU_LIP = 1.13           # max |d gelu / dx| = 1.1289 (at x = 1.414)
LIN_REL = 2e-6


# ----------------------------------------------------------------------------------------------------------------- plumbing
class Guarded:
    """`nbytes` of device memory inside a larger allocation filled with 0xFF; `guard` bytes (a multiple of 256) on either side."""

    def __init__(self, nbytes, guard):
        assert guard % 256 == 0 and nbytes % 4 == 0
        self.n, self.g = nbytes, guard
        self.buf = torch.full((guard + nbytes + guard,), 0xFF, dtype=torch.uint8, device=DEV)

    def view(self, dtype=torch.uint8):
        return self.buf[self.g: self.g + self.n].view(dtype)

    def ptr(self):
        return L.ptr(self.buf) + self.g

    def host(self):
        """The payload bytes on the CPU, after asserting that both guards are bit-unchanged."""
        torch.cuda.synchronize()
        h = self.buf.cpu()
        assert bool((h[: self.g] == 0xFF).all()), "bytes BEFORE the output were written"
        assert bool((h[self.g + self.n:] == 0xFF).all()), "bytes BEHIND the output were written"
        return h[self.g: self.g + self.n].clone()


def guarded_rows(rows, row_bytes):
    return Guarded(rows * row_bytes, (8 * row_bytes + 255) // 256 * 256)


def split_rows(host_bytes, rows, row_bytes, written, word=torch.int16):
    """host bytes of `rows` rows -> the image in `word`s (int16: fp16 planes, int32: fp32; all-ones is a NaN in both) after asserting that
    exactly the rows of the bool mask `written` were written, each of them completely."""
    img = host_bytes.view(word).reshape(rows, -1)
    assert img.shape[1] * img.element_size() == row_bytes
    untouched = (img == -1).all(dim=1)
    partly = (img == -1).any(dim=1) & ~untouched
    assert not bool(partly.any()), f"rows written in part: {torch.nonzero(partly).flatten()[:8].tolist()}"
    bad = untouched == written
    assert not bool(bad.any()), (f"rows {torch.nonzero(bad & written).flatten()[:8].tolist()} never written, rows "
                                 f"{torch.nonzero(bad & ~written).flatten()[:8].tolist()} written but not the op's")
    return img


def pair_rows(host_bytes, rows, Cc, written):
    """-> fp64 values (n_written, C) of the written rows of pair planes."""
    split_rows(host_bytes, rows, Cc * 4, written)
    with_nan = R.decode_pair(host_bytes, rows, Cc)
    return with_nan[written]


def f32_rows(host_bytes, rows, Cc, written):
    split_rows(host_bytes, rows, Cc * 4, written, torch.int32)
    return host_bytes.view(torch.float32).reshape(rows, Cc)[written].clone()


def all_rows(rows):
    return torch.ones(rows, dtype=torch.bool)


def dev(t):
    return t.contiguous().to(DEV)


def make_vit(n_patches, **fields):
    v = L.Vit()
    v.depth, v.dim, v.heads, v.hidden = 12, D, HEADS, 4 * D
    v.n_patches, v.n_frames = n_patches, NF
    v.in_chans, v.frames, v.img, v.patch, v.patch_t, v.patch_k = 3, 16, 224, 16, 2, 1536
    v.eps = R.EPS
    for k, val in fields.items():
        setattr(v, k, val)
    return v


def call(name, *args):
    rc = getattr(L.lib(), name)(*args, L.current_stream(DEV))
    torch.cuda.synchronize()
    return rc


def run(name, *args):
    L.check(call(name, *args), name)


RECORD = {}      # (op, kernel, case) -> (err, e_ref, bar)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = ["# extractor kernels op by op against fp64 (tests/test_gpu_avclip_ops.py): per (op, kernel, case) the largest measured error, the",
             "# fp32 torch restatement's error on the same case (e_ref; - where the bar does not use one) and the bar, all in the units the",
             "# module docstring names (attention: max |v| of the element's keys; LayerNorm: max |w x^| + max |b| of the row; linear: abs;",
             "# gelu: error / allowed).  'ratio' = max over elements of |err| / the element's own allowed error (must be <= 1)."]
    for (op, kern, case), (err, e_ref, bar, ratio) in sorted(RECORD.items()):
        lines.append(f"{op:10s} {kern:12s} {case:34s} err {err:.3e}  e_ref {e_ref}  bar {bar:.3e}  ratio {ratio:.3f}")
    print("\n".join(lines))
    out = os.environ.get("VAURA_AVCLIP_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def note(op, kern, case, err, e_ref, bar, ratio):
    key = (op, kern, case)
    old = RECORD.get(key)
    if old is None or ratio > old[3]:
        RECORD[key] = (err, "-" if e_ref is None else f"{e_ref:.3e}", bar, ratio)
    print(f"[avclip-op] {op} {kern} {case}: err {err:.3e} e_ref {e_ref if e_ref is None else format(e_ref, '.3e')} bar {bar:.3e} ratio {ratio:.3f}")


def check_scaled(op, kern, case, got64, ref64, ref32, scale, extra=None, pair_out=True, floor=None):
    """The fp32-class rule per element: |got - ref| <= (max(3e-6, 4 e_ref) + extra) x scale (+ the pair planes' representation error).
    `floor`: a derived per-element floor in place of 3e-6 (LayerNorm on constant rows only).  -> the bar (relative, a tensor where
    `extra` or `floor` is one)."""
    assert bool(torch.isfinite(got64).all()), f"{op} {kern} {case}: non-finite output"
    e_ref = float(((ref32.double() - ref64).abs() / scale).max())
    bar = R.fp32_bar(e_ref) if floor is None else floor.clamp(min=R.FACTOR * e_ref)
    bar = bar + (0.0 if extra is None else extra)
    allowed = bar * scale + (R.pair_repr_err(ref64) if pair_out else 0.0)
    d = (got64 - ref64).abs()
    ratio = float((d / allowed).max())
    note(op, kern, case, float((d / scale).max()), e_ref, float(bar.max()) if torch.is_tensor(bar) else bar, ratio)
    if ratio > 1.0:
        i = int((d / allowed).argmax())
        r, c = divmod(i, got64.shape[-1])
        raise AssertionError(f"{op} {kern} {case}: |err| / allowed = {ratio:.3f} at row {r} channel {c}: got {got64.reshape(-1)[i]:.9g}, "
                             f"fp64 {ref64.reshape(-1)[i]:.9g}, e_ref {e_ref:.3e}")
    return bar


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_entry_points_refuse_what_the_forward_refuses():
    """VAURA_ERR_SHAPE (-2) / VAURA_ERR_ARG (-1) before any launch: the output stays 0xFF."""
    out = guarded_rows(64, D * 4)
    x = dev(torch.zeros(64, 3 * D))
    w = dev(torch.ones(D))
    o, xp, wp = out.ptr(), L.ptr(x), L.ptr(w)
    bad_dims = [dict(dim=512), dict(heads=8), dict(n_frames=4), dict(hidden=3000), dict(patch_k=1540)]
    for np_, fields in [(5, f) for f in bad_dims] + [(256, {}), (0, {})]:
        v = make_vit(np_, cls_token=wp, pos_embed=xp, temp_embed=xp, **fields)
        vr = C.byref(v)
        assert call("vaura_vit_embed", vr, o, 1) == -2, (np_, fields)
        assert call("vaura_vit_layernorm", vr, xp, wp, wp, o, None, 4, 0) == -2
        assert call("vaura_vit_fill_rows", vr, o, wp, 4, 1) == -2
        assert call("vaura_vit_cls_attention", vr, xp, o, None, 1, 6, 1) == -2
        assert call("vaura_vit_time_attention", vr, xp, o, 1) == -2
        assert call("vaura_vit_space_attention", vr, xp, o, 1) == -2
    v = make_vit(1, cls_token=wp, pos_embed=xp, temp_embed=xp)
    vr = C.byref(v)
    assert call("vaura_vit_embed", None, o, 1) == -1 and call("vaura_vit_embed", vr, None, 1) == -1 and call("vaura_vit_embed", vr, o, 0) == -1
    assert call("vaura_vit_embed", C.byref(make_vit(1)), o, 1) == -1                                    # no tables
    assert call("vaura_vit_layernorm", vr, xp, wp, wp, None, None, 4, 0) == -1 and call("vaura_vit_layernorm", vr, xp, wp, wp, o, None, 4, 2) == -1
    assert call("vaura_vit_layernorm", vr, xp, wp, wp, o, None, 0, 0) == -1 and call("vaura_vit_layernorm", vr, None, wp, wp, o, None, 4, 0) == -1
    assert call("vaura_vit_layernorm", vr, xp, wp, wp, o, None, 12, 1) == -2                            # map 1: whole segments (8 rows here)
    assert call("vaura_vit_fill_rows", vr, o, None, 4, 1) == -1 and call("vaura_vit_fill_rows", vr, o, wp, 4, 0) == -1
    assert call("vaura_vit_cls_attention", vr, xp, o, None, 1, 2042, 1) == -2 and call("vaura_vit_cls_attention", vr, xp, o, None, 1, 0, 1) == -2
    assert call("vaura_vit_cls_attention", vr, xp, o, None, 0, 6, 1) == -1 and call("vaura_vit_cls_attention", vr, xp, None, None, 1, 6, 1) == -1
    assert call("vaura_vit_time_attention", vr, None, o, 1) == -1 and call("vaura_vit_space_attention", vr, xp, o, 0) == -1
    assert call("vaura_vit_patchify", xp, o, 1, 3, 4, 24, 2, 12) == -2 and call("vaura_vit_patchify", xp, o, 1, 3, 4, 40, 2, 16) == -2
    assert call("vaura_vit_patchify", xp, o, 1, 3, 3, 32, 2, 16) == -2 and call("vaura_vit_patchify", xp + 4, o, 1, 3, 4, 32, 2, 16) == -2
    assert call("vaura_vit_patchify", None, o, 1, 3, 4, 32, 2, 16) == -1 and call("vaura_vit_patchify", xp, o, 0, 3, 4, 32, 2, 16) == -1
    lin = lambda *a: call("vaura_linear_pair", *a)
    assert lin(xp, xp, wp, None, o, None, 2, 1, 8, 8, 0, 40, 96) == -2 and lin(xp, xp, wp, None, o, None, 2, 1, 8, 8, 0, 32, 100) == -2
    assert lin(xp, xp, wp, None, o, None, 0, 1, 8, 8, 0, 32, 96) == -1 and lin(xp, xp, wp, None, o, None, 2, 1, 8, 8, 1, 32, 96) == -1
    assert lin(xp, xp, wp, None, None, None, 2, 1, 8, 8, 0, 32, 96) == -1 and lin(None, xp, wp, None, o, None, 2, 1, 8, 8, 0, 32, 96) == -1
    assert lin(xp, xp, wp, None, o, None, 2, 0, 8, 8, 0, 32, 96) == -1 and lin(xp, xp, None, None, o, None, 2, 1, 8, 8, 0, 32, 96) == -1
    assert bool((out.host() == 0xFF).all()), "a refused call launched something"


# ------------------------------------------------------------------------------------------------------------------ patchify
@pytest.mark.parametrize("geom", [(3, 16, 224, 2, 16), (3, 4, 32, 2, 16)], ids=["3x16x224x224", "3x4x32x32"])
def test_patchify_is_the_gather_in_weight_order(geom):
    Cc, T, HW, pt, ps = geom
    frames = torch.randn(2, Cc, T, HW, HW, generator=R.gen(21))
    frames[1] *= 100.0
    want = R.to_pair_planes(R.patch_gather(frames, pt, ps))                       # fp16 (rows, K/8, 2, 8)
    rows, K = want.shape[0], want.shape[1] * 8
    assert rows == 2 * (T // pt) * (HW // ps) ** 2 and K == Cc * pt * ps * ps
    out = guarded_rows(rows, K * 4)
    run("vaura_vit_patchify", L.ptr(dev(frames)), out.ptr(), 2, Cc, T, HW, pt, ps)
    img = split_rows(out.host(), rows, K * 4, all_rows(rows))
    assert torch.equal(img.reshape(-1), want.view(torch.int16).reshape(-1))


# ----------------------------------------------------------------------------------------------------------- embed, fill_rows
@pytest.mark.parametrize("n", [5, 196])
def test_embed_adds_the_separate_positional_embedding(n):
    g = R.gen(22 + n)
    Lq = 1 + NF * n
    x = torch.randn(2, Lq, D, generator=g)
    x[1] *= 100.0
    x[:, 0] = float("nan")                                   # the CLS row is written, never read
    cls, pos, temp = torch.randn(D, generator=g), torch.randn(1 + n, D, generator=g), torch.randn(NF, D, generator=g)
    buf = guarded_rows(2 * Lq, D * 4)
    buf.view(torch.float32).copy_(dev(x).reshape(-1))
    cd, pd, td = dev(cls), dev(pos), dev(temp)
    v = make_vit(n, cls_token=L.ptr(cd), pos_embed=L.ptr(pd), temp_embed=L.ptr(td))
    run("vaura_vit_embed", C.byref(v), buf.ptr(), 2)
    got = buf.host().view(torch.float32).reshape(2, Lq, D)
    want32 = R.embed(x, cls, pos, temp, NF, n)
    assert torch.equal(got, want32), f"{int((got != want32).sum())} values differ from x + (pos + temp) in fp32"
    ref = R.embed(x.double(), cls.double(), pos.double(), temp.double(), NF, n)
    inner = torch.cat(((cls + pos[0]).abs()[None] * 0, (pos[1:].repeat(NF, 1) + temp.repeat_interleave(n, 0)).abs()), dim=0).double()
    allowed = R.U24 * (inner + ref.abs())
    assert bool(((got.double() - ref).abs() <= allowed).all())


def test_fill_rows_writes_only_its_strided_rows():
    vec = torch.randn(D, generator=R.gen(23))
    vd = dev(vec)
    v = make_vit(196)
    for n, stride in ((16, 1), (16, 6), (16, 197), (1, 197), (3, 2)):
        rows = (n - 1) * stride + 1
        out = guarded_rows(rows, D * 4)
        run("vaura_vit_fill_rows", C.byref(v), out.ptr(), L.ptr(vd), n, stride)
        written = torch.zeros(rows, dtype=torch.bool)
        written[::stride] = True
        got = f32_rows(out.host(), rows, D, written)
        assert torch.equal(got, vec.expand(n, D)), (n, stride)


# ----------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("rows,map_", [(1, 0), (5, 0), (1569, 0), (2 * 1568, 1)])
def test_layernorm(rows, map_, family):
    n = 196
    x, w, b = R.ln_inputs(rows, family, 31 + rows)
    if map_:
        src, dst = R.ln_map1_rows(2, NF, n)
        xin = torch.full((2 * (1 + NF * n), D), float("nan"))         # CLS rows: NaN, never read
        xin[src] = x
        out_rows = 2 * NF * (n + 1)
        written = torch.zeros(out_rows, dtype=torch.bool)
        written[dst] = True
        order = torch.argsort(dst)                                    # written rows come back in row order
        assert torch.equal(order, torch.arange(rows))                 # ... which is the source order
    else:
        xin, out_rows, written = x, rows, all_rows(rows)
    x64, w64, b64 = x.double(), w.double(), b.double()
    ref = R.layernorm(x64, w64, b64)
    ref32 = R.layernorm(x, w, b)
    xhat = R.layernorm(x64, torch.ones(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64))
    scale = ((w64 * xhat).abs().amax(dim=1, keepdim=True) + b64.abs().max()).expand(rows, D)
    floor = R.ln_constant_row_floor(x, w) / scale if family == "constant" else None       # relative to the row's scale, like the bar
    xd, wd, bd = dev(xin), dev(w), dev(b)
    v = make_vit(n)
    for mode in ("f32", "pair", "both"):
        of = guarded_rows(out_rows, D * 4) if mode != "pair" else None
        op = guarded_rows(out_rows, D * 4) if mode != "f32" else None
        run("vaura_vit_layernorm", C.byref(v), L.ptr(xd), L.ptr(wd), L.ptr(bd), of.ptr() if of else None, op.ptr() if op else None, rows, map_)
        case = f"rows {rows} map {map_} {family}"
        if of:
            got = f32_rows(of.host(), out_rows, D, written)
            check_scaled("layernorm", "f32 out", case, got.double(), ref, ref32, scale, pair_out=False, floor=floor)
        if op:
            gp = pair_rows(op.host(), out_rows, D, written)
            check_scaled("layernorm", "pair out", case, gp, ref, ref32, scale, floor=floor)
        if of and op:                                                 # the planes are the split of the fp32 output
            assert torch.equal(gp, R.pair_value64(got))


# ------------------------------------------------------------------------------------------------------------- CLS attention
CLS_CASES = {"197": (197, True), "513-empty-last-split": (513, True), "1569-split": (1569, True), "1569-one-split": (1569, False)}
CLS_FAMILIES = ("flat", "peak30@first-key", "peak30@last-key", "peak30@first-split", "peak30@middle-split", "peak30@last-split", "big80", "ones")


def _cls_peak_row(Lseq, where):
    chunk = (((Lseq + 7) // 8) + 15) & ~15                  # the launcher's split arithmetic: 8 splits of `chunk` keys
    last = (Lseq - 1) // chunk                              # last split that holds a key
    return {"first-key": 0, "last-key": Lseq - 1, "first-split": min(7, Lseq - 1), "middle-split": min(3 * chunk + 10, Lseq - 2),
            "last-split": last * chunk + 1}[where]


def test_cls_split_arithmetic_of_the_cases():
    """513 keys: chunk 80, split 6 holds 33 keys and split 7 none; 1569: chunk 208, split 7 holds 113."""
    assert _cls_peak_row(513, "last-split") == 481 and 7 * 80 >= 513 and 513 - 6 * 80 == 33
    assert _cls_peak_row(1569, "last-split") == 7 * 208 + 1 and 1569 - 7 * 208 == 113
    assert _cls_peak_row(1569, "middle-split") == 634 and _cls_peak_row(513, "middle-split") == 250


@pytest.mark.parametrize("family", CLS_FAMILIES)
@pytest.mark.parametrize("case", list(CLS_CASES))
def test_cls_attention(case, family):
    Lseq, use_part = CLS_CASES[case]
    fam, _, where = family.partition("@")
    peak = torch.tensor([_cls_peak_row(Lseq, where)]) if where else None
    qkv = R.attention_inputs(2, Lseq, fam, 41 + Lseq, peak_rows=peak)
    R.scale_v(qkv, (1, slice(None)))
    ref, ref32, scale = R.cls_attention(qkv.double()), R.cls_attention(qkv), R.cls_vscale(qkv.double())
    qd = dev(qkv)
    part = torch.full((2 * HEADS * 8 * 66,), float("nan"), device=DEV) if use_part else None
    v = make_vit(196)
    for kern, bits in (("16-lane", 0), ("one-wg", Variant.VIT_CLS_UNSPLIT)):      # 16-lane: vit_cls_attn_split_kernel, 8 splits + combine only where `part` is given and Lseq > 512
        for stride in (1, Lseq):
            rows = stride + 1
            out = guarded_rows(rows, D * 4)
            with variants(bits):
                run("vaura_vit_cls_attention", C.byref(v), L.ptr(qd), out.ptr(), L.ptr(part), 2, Lseq, stride)
            written = torch.zeros(rows, dtype=torch.bool)
            written[[0, stride]] = True
            got = pair_rows(out.host(), rows, D, written)
            check_scaled("cls", kern, f"{case} {family} stride {stride}", got, ref, ref32, scale)


# ------------------------------------------------------------------------------------------------------ time / space attention
PATTERN_FAMILIES = ("flat", "peak30", "first", "last", "big80", "ones")


def _pattern_case(n, family, mode, seed):
    Lq = 1 + NF * n
    if family == "last":
        peak = R.last_key_rows(NF, n, mode)
    elif mode == "time":
        peak = 1 + 3 * n + torch.arange(n)                  # frame 3 of every location
    else:
        peak = 1 + torch.arange(NF) * n + min(3, n - 1)     # location 3 of every frame
    qkv = R.attention_inputs(2, Lq, family, seed, peak_rows=peak)
    R.scale_v(qkv, (1, slice(None)))
    if mode == "space":
        odd = (1 + torch.arange(NF * n))[(torch.arange(NF * n) // n) % 2 == 1]
        R.scale_v(qkv, odd)
    q64 = qkv.double()
    written = torch.ones(2 * Lq, dtype=torch.bool)
    written[[0, Lq]] = False                                # the CLS rows belong to the CLS pattern
    flat = lambda t: t.reshape(2 * NF * n, D)
    return qkv, flat(R.pattern_attention(q64, NF, n, mode)), flat(R.pattern_attention(qkv, NF, n, mode)), flat(R.pattern_vscale(q64, NF, n, mode)), written


@pytest.mark.parametrize("family", PATTERN_FAMILIES)
@pytest.mark.parametrize("n", [3, 196])
def test_time_attention(n, family):
    qkv, ref, ref32, scale, written = _pattern_case(n, family, "time", 51 + n)
    qd = dev(qkv)
    v = make_vit(n)
    for kern, bits in (("16-lane", 0), ("one-thread", Variant.VIT_TIME_THREAD_PER_HEAD_FRAME)):
        out = guarded_rows(written.numel(), D * 4)
        with variants(bits):
            run("vaura_vit_time_attention", C.byref(v), L.ptr(qd), out.ptr(), 2)
        got = pair_rows(out.host(), written.numel(), D, written)
        check_scaled("time", kern, f"np {n} {family}", got, ref, ref32, scale)


@pytest.mark.parametrize("family", PATTERN_FAMILIES)
@pytest.mark.parametrize("n", [15, 16, 196, 207, 208, 255])
def test_space_attention(n, family):
    qkv, ref, ref32, scale, written = _pattern_case(n, family, "space", 61 + n)
    apriori = R.pair_attention_apriori(qkv, NF, n, "space").reshape(2 * NF * n, D)
    qd = dev(qkv)
    v = make_vit(n)
    # above 207 patches the launcher takes vit_space_attn_kernel whatever the switches: one kernel, the fp32 class
    kernels = (("pair", 0, apriori), ("mfma-f32", Variant.VIT_SPACE_FP32_MFMA, None),
               ("one-thread", Variant.VIT_SPACE_THREAD_PER_QUERY, None)) if n <= 207 else (("generic", 0, None),)
    outs = []
    for kern, bits, extra in kernels:
        out = guarded_rows(written.numel(), D * 4)
        with variants(bits):
            run("vaura_vit_space_attention", C.byref(v), L.ptr(qd), out.ptr(), 2)
        got = pair_rows(out.host(), written.numel(), D, written)
        bar = check_scaled("space", kern, f"np {n} {family}", got, ref, ref32, scale, extra=extra)
        outs.append((kern, got, bar))
    for i in range(len(outs)):
        for j in range(i + 1, len(outs)):
            (ka, a, ba), (kb, b, bb) = outs[i], outs[j]
            allowed = (ba + bb) * scale + 2 * R.pair_repr_err(ref)
            assert bool(((a - b).abs() <= allowed).all()), f"{ka} and {kb} differ by more than the sum of their bars (np {n} {family})"


# -------------------------------------------------------------------------------------------------------------------- linear
@functools.lru_cache(maxsize=None)
def _weights(Cin, Cout):
    g = R.gen(71 + Cin + Cout)
    w = torch.randn(Cout, Cin, generator=g) * 0.05
    b = torch.randn(Cout, generator=g) * 0.3
    return dev(R.to_pair_planes(w)), R.pair_value64(w), dev(b), b.double()


LINEAR_KINDS = {
    # name: (Cin, Cout, B, oshift, residual, gelu)
    "patch-embed 1536x768 oshift 1": (1536, 768, 2, 1, None, False),
    "qkv 768x2304 raw": (768, 2304, 1, 0, None, False),
    "proj 768x768 + res in place": (768, 768, 1, 0, "inplace", False),
    "fc1 768x3072 gelu planes": (768, 3072, 1, 0, None, True),
    "fc2 3072x768 + res": (3072, 768, 1, 0, "separate", False),
    # Cout % 192 != 0: no shape of the extractor, the launcher's way onto the codec's 128 x 96 conv tile (129 rows: a full tile and a ragged one)
    "conv tile 96x96 oshift 1 + res": (96, 96, 2, 1, "separate", False),
}


@pytest.mark.parametrize("Lin", [8, 128, 129, 1569])
@pytest.mark.parametrize("kind", list(LINEAR_KINDS))
def test_linear_pair(kind, Lin):
    Cin, Cout, B, oshift, resk, gelu = LINEAR_KINDS[kind]
    Lout = Lin + oshift
    g = R.gen(81 + Lin + Cin)
    x = torch.randn(B, Lin, Cin, generator=g) * (0.2 + 2.0 * torch.rand(B, Lin, 1, generator=g))
    if B == 2:
        x[1] *= 100.0
    wd, w64, bd, b64 = _weights(Cin, Cout)
    xd = dev(R.to_pair_planes(x.reshape(B * Lin, Cin)))
    lin = R.linear(R.pair_value64(x), w64, b64)                                   # (B, Lin, Cout) fp64
    out = guarded_rows(B * Lout, Cout * 4)
    written = torch.ones(B, Lout, dtype=torch.bool)
    written[:, :oshift] = False
    res64, rd = None, None
    if resk:
        res = torch.randn(B, Lout, Cout, generator=g) * 2.0
        res64 = res.double()
        if resk == "inplace":
            out.view(torch.float32).copy_(dev(res).reshape(-1))
            rp = out.ptr()
        else:
            rd = dev(res)
            rp = L.ptr(rd)
    else:
        rp = None
    total = lin if res64 is None else lin + res64[:, oshift:]
    bar = LIN_REL * lin.abs().amax(dim=(1, 2), keepdim=True) + (R.U23 * total.abs() if res64 is not None else 0.0)
    if gelu:
        run("vaura_linear_pair", L.ptr(xd), L.ptr(wd), L.ptr(bd), rp, None, out.ptr(), 1, B, Lin, Lout, oshift, Cin, Cout)
        got = pair_rows(out.host(), B * Lout, Cout, written.reshape(-1)).reshape(B, Lin, Cout)
        ref = R.gelu(total)
        allowed = GELU_LIP * bar + R.gelu_allowed(total, ref)
    else:
        run("vaura_linear_pair", L.ptr(xd), L.ptr(wd), L.ptr(bd), rp, out.ptr(), None, 2, B, Lin, Lout, oshift, Cin, Cout)
        got = f32_rows(out.host(), B * Lout, Cout, written.reshape(-1)).double().reshape(B, Lin, Cout)
        ref, allowed = total, bar + torch.zeros_like(total)
    assert bool(torch.isfinite(got).all())
    d = (got - ref).abs()
    ratio = float((d / allowed).max())
    note("linear", "pair-gemm", f"{kind} rows {Lin}", float(d.max()), None, float(allowed.max()), ratio)
    assert ratio <= 1.0, f"{kind} rows {Lin}: |err| / allowed = {ratio:.3f} at {divmod(int((d / allowed).argmax()), Cout)}"


# ---------------------------------------------------------------------------------------------------------------- GELU alone
def _check_gelu(arg, got, what):
    """arg fp32 (n): the epilogue's arguments; got fp64 (n).  -> (worst |err| / allowed, number of sign-checked values)."""
    x64 = arg.double()
    ref = R.gelu(x64)
    d = (got - ref).abs() / R.gelu_allowed(x64, ref)
    j = int(d.argmax())
    assert float(d[j]) <= 1.0, f"{what}: gelu({float(arg[j])!r}): got {float(got[j])!r}, fp64 {float(ref[j])!r}, |err| / allowed {float(d[j]):.3f}"
    nz = R.pair_value64(ref.float()) != 0                                      # the fp64 value rounds to a nonzero pair
    wrong = nz & (torch.sign(got) != torch.sign(ref))
    assert not bool(wrong.any()), f"{what}: wrong sign or a zero at x = {arg[wrong][:8].tolist()}: got {got[wrong][:8].tolist()}"
    return float(d[j]), int(nz.sum())


def test_gelu_epilogue_against_fp64():
    """The (768, 3072) GELU linear with stacked identity blocks as weight, so that the epilogue receives chosen arguments exactly.
      bias pass   x = 0 and the sweep in the bias: every product is an exact zero and the epilogue holds 0 + bias; 8 rows per launch,
                  all of which must come back identical.  (The weight plays no part here.)
      x pass      bias = 0 and the sweep, rounded to fp16 (lo plane 0), in x: output column o of row r is 1 x x[r, o % 768], one exact
                  product plus exact zeros; the four column blocks must come back identical.
    Of +-0 only +0 can reach the epilogue: the accumulator starts at +0 and +0 + (-0) = +0 in either pass, for a -0 product and for a
    -0 bias alike.  The host mirrors that (0 + sweep) and the sweep keeps its -0 so that the path is run."""
    sweep = R.gelu_sweep()
    w = torch.zeros(4 * D, D)
    w[torch.arange(4 * D), torch.arange(4 * D) % D] = 1.0
    wd = dev(R.to_pair_planes(w))
    xd = dev(R.to_pair_planes(torch.zeros(8, D)))
    worst, n_signed = 0.0, 0
    for i in range(sweep.numel() // (4 * D)):
        arg = (torch.zeros(4 * D) + sweep[i * 4 * D:(i + 1) * 4 * D])             # what the fp32 epilogue holds: 0 + bias
        bd = dev(arg)
        out = guarded_rows(8, 4 * D * 4)
        run("vaura_linear_pair", L.ptr(xd), L.ptr(wd), L.ptr(bd), None, None, out.ptr(), 1, 1, 8, 8, 0, D, 4 * D)
        got = pair_rows(out.host(), 8, 4 * D, all_rows(8))
        assert bool((got == got[0]).all()), "rows of one launch differ"
        e, k = _check_gelu(arg, got[0], "bias pass")
        worst, n_signed = max(worst, e), n_signed + k
    assert n_signed > 15000
    note("gelu", "epilogue", f"bias pass {sweep.numel()} args in [-40, 40]", worst, None, 1.0, worst)
    rows = sweep.numel() // D
    xs = sweep.half().float().reshape(rows, D)
    planes = R.to_pair_planes(xs)
    assert not bool(planes[:, :, 1].float().abs().any())                           # fp16 values: the lo plane is zero
    out = guarded_rows(rows, 4 * D * 4)
    zb = dev(torch.zeros(4 * D))
    run("vaura_linear_pair", L.ptr(dev(planes)), L.ptr(wd), L.ptr(zb), None, None, out.ptr(), 1, 1, rows, rows, 0, D, 4 * D)
    got = pair_rows(out.host(), rows, 4 * D, all_rows(rows)).reshape(rows, 4, D)
    assert bool((got == got[:, :1]).all()), "the four identity blocks differ"
    e, k = _check_gelu((torch.zeros(rows, D) + xs).reshape(-1), got[:, 0].reshape(-1), "x pass")
    assert k > 15000
    note("gelu", "epilogue", f"x pass {sweep.numel()} fp16 args in [-40, 40]", e, None, 1.0, e)
