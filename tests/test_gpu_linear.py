"""Decoder linear kernels on the GPU (csrc/gemv.hip, gemv3.hip, gemv3_kernel.h, gemv_kernel.h) through vaura_gemv_pair / vaura_gemv.

  exact half      inputs of tests/linear_reference.py on which every partial sum is an fp32 number: whatever the instantiation, tiling,
                  K split or reduction order, the output is the exact value — torch.equal, every live row and column, for every row of
                  the dispatch table (linear_reference.PAIR_TABLE / GEMV_TABLE).  Where a rounding chain follows the sum (fused norm,
                  SwiGLU, GELU, ss_out) the bound is derived from the kernel's source, per element, relative to the element's own
                  value (linear_reference: C_NORM, swiglu_ref_and_bound, gelu_ref_and_bound, C_SS).
  dead space      every output buffer is filled with a sentinel and has a guard of one 16-row block behind its padded extent.
  precision half  random operands spread over 20 binades per row, against the fp64 product of the planes and weights actually held,
                  per row, under the project's rule  err_r <= max(3e-6, 4 x the fp32 torch product's error).
The largest observed error / bound per (path, storage) and the precision half's figures are printed; with VAURA_PARITY_DIR set they are
kept in linear_parity.txt.  (tests/test_linear_reference_host.py is the CPU proof that the reference itself is exact.)"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import linear_reference as R  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import ops, quant, synth  # noqa: E402
from vaura_amd.engine import h_effective_weight  # noqa: E402
from vaura_amd.variants import Variant, Variant2, variants  # noqa: E402

DEV = "cuda:0"
WD = {"h1": L.W_H1, "h2": L.W_H2, "fp8": L.W_FP8, "fp8h": L.W_FP8H}
SENT, SENT16 = 12345.0, 0x5A5A
ERR_SHAPE = -2

_ratios = {}             # "path [storage] kind" -> largest observed error / bound
_precision = {}          # "shape [storage]" -> line
_prepared = {}           # (shape, two_planes) -> _Prepared
_packed = {}             # (shape, storage) -> packed weights on the device
_gemv = {}               # (K, epi, norm) -> (GemvLattice, {bf16: packed weights})


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    for k in sorted(_ratios):
        print(f"linear_parity: {_ratios[k]:8.4f}  {k}")
    for k in sorted(_precision):
        print("linear_parity:", _precision[k])
    out = os.environ.get("VAURA_PARITY_DIR")
    if out and (_ratios or _precision):
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "linear_parity.txt"), "w") as f:
            f.write("decoder linear kernels against fp64 (tests/test_gpu_linear.py)\n"
                    "exact half: outputs without a rounding chain are bit-equal to the exact value and have no line here; below, the largest\n"
                    "|error| / bound per (path, storage), bounds derived from the source (tests/linear_reference.py: norm C_NORM U |ref|,\n"
                    "swiglu, gelu, ss_out C_SS U ref)\n")
            for k in sorted(_ratios):
                f.write(f"{_ratios[k]:8.4f}  {k}\n")
            f.write("precision half: 32 rows, x = randn 2^e_r with e_r spread over [-10, 10]; per row err_r = max_n |got - ref64| / max_n |ref64|,\n"
                    "e_ref_r the same for the fp32 torch product of the held operands; bar err_r <= max(3e-6, 4 e_ref_r)\n")
            for k in sorted(_precision):
                f.write(_precision[k] + "\n")


def _note(key, err, bound):
    live = bound > 0
    if bool(live.any()):
        _ratios[key] = max(_ratios.get(key, 0.0), float((err[live] / bound[live]).max()))


class _Prepared:
    """One shape on the lattice: inputs for max_rows(shape) rows, the exact sums per mode, the packed weights of the storages of its
    weight class.  The (N, K) matrices are dropped once packed: a case then costs one launch and a few small tensor operations."""

    def __init__(self, shape, two_planes):
        lat = R.PairLattice(shape, two_planes)
        s = R.PAIR_SHAPES[shape]
        self.exact, self.halves = {}, {}
        for mode in (("three",) if two_planes else ("full", "hi")):
            self.exact[mode], abs_sum = R.pair_products(lat, mode)
            worst, bound = R.lattice_condition(abs_sum, lat.res, lat.granule)
            assert worst < bound, (shape, mode, worst, bound)            # the condition under which any summation order is exact
            if s["ksplit"]:
                self.halves[mode] = (R.pair_products(lat, mode, 0, lat.K // 2)[0], R.pair_products(lat, mode, lat.K // 2, lat.K)[0])
        wd = lat.w.to(DEV)
        for st in (("h2",) if two_planes else ("h1", "fp8", "fp8h")):
            _packed[(shape, st)] = ops.pack_weight(wd, WD[st])
        del wd
        self.x, self.xhi, self.xlo, self.res, self.ss = lat.x, lat.xhi, lat.xlo, lat.res, lat.ss
        self.gain_in = None if lat.gain_in is None else lat.gain_in.to(DEV)
        self.gain_out = lat.gain_out
        self.gain_out_dev = None if lat.gain_out is None else lat.gain_out.to(DEV)
        # the planes the producer writes are the lattice's, bit for bit (33 rows: three row blocks)
        xs, _ = ops.split_rows(ops.pack_rows(self.x[:33].to(DEV)), 33, lat.K, self.gain_in)
        planes = ops.unsplit_rows(xs, 33, lat.K).cpu().double()
        assert torch.equal(planes[0], self.xhi[:33]) and torch.equal(planes[1], self.xlo[:33])


def _prepare(shape, two_planes):
    key = (shape, two_planes)
    if key not in _prepared:
        _prepared[key] = _Prepared(shape, two_planes)
    return _prepared[key]


def _guarded(n, guard, dtype=torch.float32):
    return torch.full((n + guard,), SENT16 if dtype == torch.int16 else SENT, dtype=dtype, device=DEV)


def _untouched(buf, n):
    return bool((buf[n:] == (SENT16 if buf.dtype == torch.int16 else SENT)).all())


def _variant_words(variant):
    return {"": (0, 0), "ROWSPLIT_OFF": (int(Variant.ROWSPLIT_OFF), 0), "FP8_ROWSPLIT_OFF": (0, int(Variant2.FP8_ROWSPLIT_OFF))}[variant]


def _id(c):
    return "-".join(str(v) for v in c if v != "")


@pytest.mark.parametrize("shape,storage,rows,variant", R.pair_cases(), ids=[_id(c) for c in R.pair_cases()])
def test_pair_exact(shape, storage, rows, variant):
    s = R.PAIR_SHAPES[shape]
    K, N, epi, norm, ksplit = s["K"], s["N"], s["epi"], s["norm"], s["ksplit"]
    P = _prepare(shape, storage == "h2")
    inst = R.pair_instance(shape, storage, rows, variant)            # the table names what this case runs (and the profile's lines)
    no, rp = R.n_out(shape), (rows + 15) // 16 * 16
    nrb, guard = rp // 16, 16 * no
    xs, _ = ops.split_rows(ops.pack_rows(P.x[:rows].to(DEV)), rows, K, P.gain_in)
    ss_in = R.ss_device_layout(P.ss[:rows]).to(DEV) if norm else None
    res = ops.pack_rows(P.res[:rows].to(DEV)) if epi == R.RESID else None
    n_live = rows * N if epi == R.LOGITS else rp * no
    out = _guarded(n_live, guard)
    out2 = _guarded(n_live, guard) if ksplit else None
    want_split, want_ss = epi != R.LOGITS and not ksplit, epi in (R.STORE, R.RESID) and not ksplit
    osp = _guarded(rp * 2 * no, 2 * guard, torch.int16) if want_split else None
    oss = _guarded(nrb * (no // 16) * 16, guard) if want_ss else None
    w1, w2 = _variant_words(variant)
    with variants(w1, w2):
        rc = L.lib().vaura_gemv_pair(L.ptr(_packed[(shape, storage)]), WD[storage], L.ptr(xs), L.ptr(ss_in), K // 16 if norm else 0, L.ptr(res),
                                     L.ptr(out), L.ptr(out2), L.ptr(osp), L.ptr(P.gain_out_dev) if want_split else 0, L.ptr(oss), rows, N, K, epi,
                                     R.EPS, L.current_stream())
    L.check(rc, f"vaura_gemv_pair {inst}")
    torch.cuda.synchronize()

    # dead space: nothing behind the padded extent (logits: behind rows x N) is written
    for buf, n in ((out, n_live), (out2, n_live), (osp, rp * 2 * no), (oss, nrb * (no // 16) * 16)):
        assert buf is None or _untouched(buf, n), inst

    def rows_of(buf):
        return (buf[:n_live].view(rows, N) if epi == R.LOGITS else ops.unpack_rows(buf[:n_live], rows, no)).cpu()

    mode = R.storage_mode(storage, rows)
    got = rows_of(out)
    assert not bool((got == SENT).any()), inst                       # every live element was written
    parts = [(got, P.exact[mode][:rows])] if not ksplit else \
        [(got, P.halves[mode][0][:rows]), (rows_of(out2), P.halves[mode][1][:rows])]      # each K half against its OWN reference
    key = f"{inst} [{storage}]"
    for g, exact in parts:
        if not norm:
            want = exact if epi != R.RESID else exact + P.res[:rows].double()
            assert torch.equal(g.double(), want), (inst, int((g.double() != want).sum()))
            continue
        y = exact * R.rinv64(P.ss[:rows].sum(1), K)[:, None]
        if epi == R.SWIGLU:
            y1, y3 = R.swiglu_halves(y, N)
            assert float(y1.abs().max()) <= 12.0
            ref, bound = R.swiglu_ref_and_bound(y1, y3)
        else:
            ref, bound = y, R.norm_bound(y)
        err = (g.double() - ref).abs()
        _note(key + (" swiglu" if epi == R.SWIGLU else " norm"), err, bound)
        assert bool((err <= bound).all()), (inst, float((err / bound.clamp(min=1e-300)).max()))      # (an exact 0 has bound 0: the output is 0)
    if want_split:
        planes = ops.unsplit_rows(osp[: rp * 2 * no], rows, no).cpu()
        hi, lo = R.split2(got if P.gain_out is None else got * P.gain_out)      # planes of v = out * gain_out, as split2 defines them
        assert torch.equal(planes[0], hi) and torch.equal(planes[1], lo), inst
    if want_ss:
        ssg = R.ss_out_rows(oss.cpu(), rows, no).double()
        ref, bound = R.ss_out_ref_and_bound(got)                     # of the `out` actually returned
        err = (ssg - ref).abs()
        _note(key + " ss_out", err, bound)
        assert bool((err <= bound).all()), (inst, float((err / bound.clamp(min=1e-300)).max()))


@pytest.mark.parametrize("storage", R.STORAGES)
@pytest.mark.parametrize("shape", [s for s in R.PAIR_SHAPES if not R.PAIR_SHAPES[s]["ksplit"]])
def test_k_half_output_is_refused_elsewhere(shape, storage):
    """out_khalf2 exists for the fused-norm STORE at K = 1536 below 16 row blocks only: any other shape is VAURA_ERR_SHAPE, nothing is launched."""
    s = R.PAIR_SHAPES[shape]
    if s["epi"] == R.STORE and s["norm"]:
        rows = 256                                                   # the K-split shape itself, at 16 row blocks
    else:
        rows = 16
    K, N, no = s["K"], s["N"], R.n_out(shape)
    wp = torch.zeros(L.lib().vaura_packed_weight_bytes(N, K, WD[storage]), dtype=torch.uint8, device=DEV)
    xs = torch.zeros(rows * 2 * K, dtype=torch.int16, device=DEV)
    ss = torch.ones((rows // 16) * (K // 16) * 16, device=DEV) if s["norm"] else None
    res = torch.zeros(rows * no, device=DEV) if s["epi"] == R.RESID else None
    out, out2 = _guarded(rows * N, 0), _guarded(rows * N, 0)
    rc = L.lib().vaura_gemv_pair(L.ptr(wp), WD[storage], L.ptr(xs), L.ptr(ss), K // 16 if s["norm"] else 0, L.ptr(res), L.ptr(out), L.ptr(out2), 0,
                                 0, 0, rows, N, K, s["epi"], R.EPS, L.current_stream())
    torch.cuda.synchronize()
    assert rc == ERR_SHAPE
    assert _untouched(out, 0) and _untouched(out2, 0)


# ------------------------------------------------------------------------------------------------------------------ vaura_gemv
def _gemv_prepared(K, epi, norm):
    key = (K, epi, norm)
    if key not in _gemv:
        G = R.GemvLattice(K, epi, norm)
        worst, bound = R.lattice_condition(G.abs_sum, G.res, G.granule)
        assert worst < bound
        wd = G.w.to(DEV)
        _gemv[key] = (G, {False: ops.pack_weight(wd, L.W_F32), True: ops.pack_weight(wd, L.W_BF16)})
    return _gemv[key]


@pytest.mark.parametrize("K,epi,norm,bf16,rows", R.gemv_cases(),
                         ids=lambda v: {True: "T", False: "F"}.get(v, str(v)) if isinstance(v, bool) else str(v))
def test_gemv_exact(K, epi, norm, bf16, rows):
    """Every instance of dispatch<> in gemv.hip, fp32 and bf16 storage (the lattice's weights are bf16 numbers: both hold them)."""
    G, packed = _gemv_prepared(K, epi, norm)
    inst = [t[3] for t in R.GEMV_TABLE if t[:3] == (K, epi, norm)][0].format(bf="true" if bf16 else "false")
    N = G.N
    no, rp = (N // 2 if epi == R.SWIGLU else N), (rows + 15) // 16 * 16
    xp = ops.pack_rows(G.x[:rows].to(DEV))
    gain = G.gain.to(DEV) if norm else None
    res = ops.pack_rows(G.res[:rows].to(DEV)) if epi == R.RESID else None
    n_live = rows * N if epi == R.LOGITS else rp * no
    out = _guarded(n_live, 16 * no)
    L.check(L.lib().vaura_gemv(L.ptr(packed[bf16]), L.W_BF16 if bf16 else L.W_F32, L.ptr(xp), L.ptr(gain), L.ptr(res), L.ptr(out), rows, N, K, epi,
                               R.EPS, L.current_stream()), f"vaura_gemv {inst}")
    torch.cuda.synchronize()
    assert _untouched(out, n_live), inst
    got = (out[:n_live].view(rows, N) if epi == R.LOGITS else ops.unpack_rows(out[:n_live], rows, no)).cpu().double()
    assert not bool((got == SENT).any()), inst
    exact = G.exact[:rows]
    key = f"{inst} [{'bf16' if bf16 else 'f32'}]"
    if norm:
        y = exact * R.rinv64(G.ssq[:rows], K)[:, None]
        if epi == R.SWIGLU:
            y1, y3 = R.swiglu_halves(y, N)
            ref, bound = R.swiglu_ref_and_bound(y1, y3)
        else:
            ref, bound = y, R.norm_bound(y)
        kind = " swiglu" if epi == R.SWIGLU else " norm"
    elif epi == R.GELU:
        ref, bound = R.gelu_ref_and_bound(exact)
        kind = " gelu"
    else:
        want = exact if epi != R.RESID else exact + G.res[:rows].double()
        assert torch.equal(got, want), (inst, int((got != want).sum()))
        return
    err = (got - ref).abs()
    _note(key + kind, err, bound)
    assert bool((err <= bound).all()), (inst, float((err / bound.clamp(min=1e-300)).max()))


# ------------------------------------------------------------------------------------------------------------------ precision half
@pytest.mark.parametrize("storage", R.STORAGES)
@pytest.mark.parametrize("shape", list(R.PAIR_SHAPES))
def test_pair_precision_per_row(shape, storage):
    """Random operands, each row in its own binade: the kernel's accumulation against the fp64 product of the numbers the storage and the
    planes HOLD (the fp16-subnormal loss of the lo plane, gemv3_kernel.h split2, is a property of the format and stays out; the planes
    themselves are asserted bit for bit in the exact half and in test_gpu_ops.py)."""
    s = R.PAIR_SHAPES[shape]
    K, N, epi, norm, ksplit = s["K"], s["N"], s["epi"], s["norm"], s["ksplit"]
    rows, no = 32, R.n_out(shape)
    g = torch.Generator().manual_seed(7000 + 10 * list(R.PAIR_SHAPES).index(shape) + R.STORAGES.index(storage))
    w = torch.randn(N, K, generator=g) * 0.02
    if storage == "h1":
        w = synth.to_bf16_exact(w)
    w_eff = quant.fp8_effective_weight(w) if storage in ("fp8", "fp8h") else h_effective_weight(w, 1 if storage == "h1" else 2)
    e_r = torch.linspace(-10, 10, rows).round()[torch.randperm(rows, generator=g)]
    x = torch.randn(rows, K, generator=g) * torch.ldexp(torch.ones(rows), e_r.int())[:, None]
    gain = torch.rand(K, generator=g) + 0.5 if norm else None
    assert float((x if gain is None else x * gain).abs().max()) < 65504.0
    res = torch.randn(rows, no, generator=g) if epi == R.RESID else None
    xs, ss = ops.split_rows(ops.pack_rows(x.to(DEV)), rows, K, gain.to(DEV) if norm else None, want_ss=norm)
    out2 = torch.zeros(rows * N, device=DEV) if ksplit else None
    out, _, _ = ops.gemv_pair(ops.pack_weight(w.to(DEV), WD[storage]), xs, rows, N, K, epi, ss_in=ss,
                              residual=ops.pack_rows(res.to(DEV)) if res is not None else None, eps=R.EPS, wdtype=WD[storage], out_khalf2=out2)
    got = (out.cpu() if epi == R.LOGITS else ops.unpack_rows(out, rows, no).cpu()).double()
    if ksplit:
        got = got + ops.unpack_rows(out2, rows, no).cpu().double()
    planes = ops.unsplit_rows(xs, rows, K).cpu()                        # the planes actually on the device
    held = planes[0] if storage == "fp8h" else planes[0] + planes[1]   # fp32: exact (the two planes lie inside x's 24 bits)
    assert torch.equal(held.double(), planes[0].double() if storage == "fp8h" else planes[0].double() + planes[1].double())
    ssq = ss.view(rows // 16, K // 16, 16).cpu().double().sum(1).reshape(rows) if norm else None

    def finish(y, dt):
        if norm:
            y = y * (1.0 / torch.sqrt(ssq.to(dt) / K + R.EPS))[:, None]
        if epi == R.SWIGLU:
            y1, y3 = R.swiglu_halves(y, N)
            return torch.nn.functional.silu(y1) * y3
        return y + res.to(dt) if epi == R.RESID else y

    ref = finish(held.double() @ w_eff.double().t(), torch.float64)
    ref32 = finish(held @ w_eff.t(), torch.float32).double()
    scale = ref.abs().amax(1)
    err = (got - ref).abs().amax(1) / scale
    e_ref = (ref32 - ref).abs().amax(1) / scale
    bar = torch.maximum(torch.full_like(e_ref, 3e-6), 4 * e_ref)
    worst = int((err / bar).argmax())
    _precision[f"{shape} [{storage}]"] = (f"{shape} [{storage}]: worst row {worst} (x 2^{int(e_r[worst])}) err_r {float(err[worst]):.3e} e_ref_r "
                                          f"{float(e_ref[worst]):.3e}; largest err_r {float(err.max()):.3e}, largest e_ref_r {float(e_ref.max()):.3e}")
    print("linear_parity:", _precision[f"{shape} [{storage}]"])
    assert bool((err <= bar).all()), _precision[f"{shape} [{storage}]"]
