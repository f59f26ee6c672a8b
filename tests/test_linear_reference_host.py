"""CPU proof of tests/linear_reference.py: that a failing comparison of tests/test_gpu_linear.py cannot come from the reference.

  1. the lattice is what the text says: the plane split of the activations, the storages hold the weights exactly;
  2. its exactness condition holds for every case of the dispatch table;
  3. fp32 accumulation of the plane products in random k-orders, and as eight partial sums, equals the fp64 value bit for bit;
  4. the dispatch table resolves every case to exactly one row, every row is run, and the bound functions behave.
"""
import functools

import numpy as np
import pytest
import torch

import linear_reference as R
from vaura_amd import quant
from vaura_amd.engine import h_effective_weight, h_row_scales

SHAPE_CLASSES = [(shape, two) for shape in R.PAIR_SHAPES for two in (False, True)]


@functools.lru_cache(maxsize=2)
def lattice(shape, two_planes):
    return R.PairLattice(shape, two_planes)


@pytest.mark.parametrize("shape", list(R.PAIR_SHAPES))
def test_activation_planes_are_the_lattice(shape):
    L = lattice(shape, False)
    assert set(L.a.unique().tolist()) == {-1.0, 0.0, 1.0} and set(L.b.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert 0.45 < float((L.a == 0).double().mean()) < 0.55
    assert bool((L.b[L.a == 0] == 0).all())                     # no low part without a high part
    assert torch.equal(L.x.double(), L.a + L.b * R.LO)           # fp32 holds x
    v = L.x if L.gain_in is None else L.x * L.gain_in            # what split_rows_kernel splits: v *= gain, exact (a power of two)
    hi, lo = R.split2(v)
    assert torch.equal(hi.double(), L.xhi) and torch.equal(lo.double(), L.xlo)
    assert bool((L.xlo != 0).any())                              # both planes carry information
    assert len({tuple(r) for r in L.a[:, :64].tolist()}) == L.rows      # every row its own a: the first 64 columns already differ
    if L.norm:
        assert set(L.gain_in.unique().tolist()) == {0.5, 1.0, 2.0}
        assert len(set(L.ss.sum(1).tolist())) == L.rows           # ... and its own sum of squares
        assert torch.equal(L.ss, L.ss.round()) and float(L.ss.sum(1).max()) < 2 ** 24
        dev = R.ss_device_layout(L.ss[:17])
        assert dev.numel() == 2 * (L.K // 16) * 16
        assert float(dev[(1 * (L.K // 16) + 5) * 16 + 0]) == float(L.ss[16, 5]) and float(dev[(0 * (L.K // 16) + 7) * 16 + 9]) == float(L.ss[9, 7])
        assert float(dev[(1 * (L.K // 16) + 5) * 16 + 1]) == 0.0


@pytest.mark.parametrize("shape,two_planes", SHAPE_CLASSES)
def test_storages_hold_the_weights(shape, two_planes):
    L = lattice(shape, two_planes)
    top = 1 if L.K >= 4096 else 2
    assert set(L.wa.unique().tolist()) == set(float(v) for v in range(-top, top + 1))
    assert 0.45 < float((L.wa == 0).float().mean()) < 0.55
    assert bool((L.wb[L.wa == 0] == 0).all())
    assert torch.equal(L.w.double(), L.wa.double() + L.wb.double() * R.LO)
    if not two_planes:
        assert not bool(L.wb.any())
        assert torch.equal(h_effective_weight(L.w, 1), L.w)       # one fp16 plane
        assert torch.equal(quant.fp8_effective_weight(L.w), L.w)  # e4m3
    else:
        assert set(L.wb.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert torch.equal(h_effective_weight(L.w, 2), L.w)
        sc = h_row_scales(L.w)[:, None]                           # hi + lo of the scaled row, as h_pack_kernel forms them
        hi, lo = R.split2(L.w / sc)
        assert torch.equal(hi * sc, L.wa) and torch.equal(lo * sc, L.wb * float(R.LO))


@pytest.mark.parametrize("shape,two_planes", SHAPE_CLASSES)
def test_lattice_condition_holds_for_every_case(shape, two_planes):
    L = lattice(shape, two_planes)
    modes = ("three",) if two_planes else ("full", "hi")
    for mode in modes:
        exact, abs_sum = R.pair_products(L, mode)
        worst, bound = R.lattice_condition(abs_sum, L.res, L.granule)
        print(f"{shape} {mode}: max sum |x||w| + |res| = {worst:.1f} < {bound:.0f}")
        assert worst < bound
        assert torch.equal(exact.float().double(), exact)
        if L.res is not None:
            assert float(L.res.abs().max()) <= 64 and torch.equal((L.res.double() / R.LO).round() * R.LO, L.res.double())
            assert torch.equal((exact + L.res.double()).float().double(), exact + L.res.double())
        if mode == "three":
            full = (L.xhi + L.xlo) @ (L.wa.double() + L.wb.double() * R.LO).t()
            assert bool(((full - exact).abs() <= R.dropped_term_bound(L)).all()) and bool((full != exact).any())
        if L.epi == R.SWIGLU:
            y1, _ = R.swiglu_halves(exact * R.rinv64(L.ss.sum(1), L.K)[:, None], L.N)
            assert float(y1.abs().max()) <= 12.0
    if R.PAIR_SHAPES[shape]["ksplit"]:          # the two K halves are references of their own and add up
        a, _ = R.pair_products(L, modes[0], 0, L.K // 2)
        b, _ = R.pair_products(L, modes[0], L.K // 2, L.K)
        assert torch.equal(a + b, R.pair_products(L, modes[0])[0]) and bool((b != 0).any())


def _accumulate_f32(terms, order, parts=1):
    """terms (M, n) fp32 products; sequential fp32 accumulation along `order`, as `parts` partial sums added at the end."""
    n = terms.shape[1]
    total = np.zeros(terms.shape[0], dtype=np.float32)
    for chunk in np.array_split(order, parts):
        acc = np.zeros(terms.shape[0], dtype=np.float32)
        for k in chunk:
            acc = acc + terms[:, k]               # float32 + float32: one rounding per step (none, if the lattice is right)
        total = total + acc
    assert n == len(order)
    return total


@pytest.mark.parametrize("shape,two_planes", SHAPE_CLASSES)
def test_fp32_accumulation_is_exact_in_any_order(shape, two_planes):
    """The plane products of a sample of outputs (the last 12 rows x 24 columns spread over the matrix), summed in fp32 in three random
    orders of ALL the terms (planes mixed: stronger than any order a kernel uses) and as eight partial sums: the fp64 value, bit for bit."""
    L = lattice(shape, two_planes)
    rows = slice(L.rows - 12, L.rows)
    cols = torch.linspace(0, L.N - 1, 24).long()
    xhi, xlo = L.xhi[rows].float().numpy(), L.xlo[rows].float().numpy()
    whi, wlo = L.wa[cols].numpy(), (L.wb[cols] * float(R.LO)).numpy()
    assert xhi.dtype == np.float32 and whi.dtype == np.float32
    planes = [(whi, xhi), (whi, xlo)] + ([(wlo, xhi)] if two_planes else [])
    # scaled as the storage holds them: a power of two per weight row, undone after the sum (exact either way)
    terms = np.concatenate([(x[:, None, :] * w[None, :, :]).reshape(-1, L.K) for w, x in planes], axis=1)      # fp32 products
    t64 = np.concatenate([(x.astype(np.float64)[:, None, :] * w.astype(np.float64)[None, :, :]).reshape(-1, L.K) for w, x in planes], axis=1)
    assert np.array_equal(terms.astype(np.float64), t64)                                                      # exact products
    exact, _ = R.pair_products(L, "three" if two_planes else "full")
    want = exact[rows][:, cols].reshape(-1).numpy()
    assert np.array_equal(t64.sum(1), want)
    rng = np.random.default_rng(7)
    for _ in range(3):
        assert np.array_equal(_accumulate_f32(terms, rng.permutation(terms.shape[1])).astype(np.float64), want)
    assert np.array_equal(_accumulate_f32(terms, rng.permutation(terms.shape[1]), parts=8).astype(np.float64), want)
    if L.res is not None:
        r = L.res[rows][:, cols].reshape(-1).numpy()
        got = _accumulate_f32(terms, np.arange(terms.shape[1])) + r
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want + r.astype(np.float64))


@pytest.mark.parametrize("K,epi,norm,inst", R.GEMV_TABLE)
def test_gemv_lattice(K, epi, norm, inst):
    G = R.GemvLattice(K, epi, norm)
    worst, bound = R.lattice_condition(G.abs_sum, G.res, G.granule)
    assert worst < bound
    assert torch.equal(G.x.double(), G.x64) and torch.equal(G.w.to(torch.bfloat16).float(), G.w)      # fp32 / bf16 hold the operands
    assert torch.equal(G.exact.float().double(), G.exact)
    if norm:
        assert torch.equal(G.ssq, G.ssq.round()) and bool((G.x64.abs() <= 1).all())
        if epi == R.SWIGLU:
            y1, _ = R.swiglu_halves(G.exact * R.rinv64(G.ssq, K)[:, None], G.N)
            assert float(y1.abs().max()) <= 12.0
    if epi == R.GELU:          # the sums land where the tanh moves, on both sides of zero
        assert float((G.exact.abs() < 3).double().mean()) > 0.5 and bool((G.exact < -0.5).any()) and bool((G.exact > 0.5).any())
    # fp32 x fp32 products summed in fp32, random order and eight partial sums
    xg = (G.x64 * (G.gain.double() if norm else 1.0)).float().numpy()[-8:]
    terms = (xg[:, None, :] * G.w.numpy()[None, ::4, :]).reshape(-1, K)
    want = G.exact[-8:, ::4].reshape(-1).numpy()
    rng = np.random.default_rng(K + epi)
    assert np.array_equal(_accumulate_f32(terms, rng.permutation(K)).astype(np.float64), want)
    assert np.array_equal(_accumulate_f32(terms, rng.permutation(K), parts=8).astype(np.float64), want)


def test_dispatch_table_is_total_and_every_row_is_run():
    cases = R.pair_cases()
    assert len(cases) == len(set(cases))
    hit = {R.pair_table_row(*c) for c in cases}               # raises unless exactly one row matches
    assert hit == set(range(len(R.PAIR_TABLE)))
    for shape, sts, var, ranges, inst in R.PAIR_TABLE:
        assert shape in R.PAIR_SHAPES and set(sts) <= set(R.STORAGES) and var in ("", R.OFF, R.F8OFF)
        assert R.EPI_NAMES[R.PAIR_SHAPES[shape]["epi"]] in inst
        assert inst.startswith("gemv3h_kernel") or ("true" if R.PAIR_SHAPES[shape]["norm"] else "false") in inst      # (the row-split kernel has no norm)
        if "{wt}" not in inst:
            assert len(sts) == 1 and f"WT={R.WT[sts[0]]}" in inst
    # the requested rows: every storage and shape at the seven row counts, the GEMM tiling at 16 and 17 row blocks, the fallbacks
    for shape in R.PAIR_SHAPES:
        for st in R.STORAGES:
            assert all((shape, st, r, "") in cases for r in (1, 8, 9, 16, 17, 32, 33))
    for shape in ("resid4096", "swiglu", "logits"):
        assert all((shape, st, r, "") in cases for st in ("h1", "h2", "fp8") for r in (250, 272))
    for shape in ("store1536", "resid1536", "resid4096", "store4096"):
        assert all((shape, st, r, "ROWSPLIT_OFF") in cases for st in R.STORAGES for r in (16, 32))
        assert all((shape, st, r, "FP8_ROWSPLIT_OFF") in cases for st in ("fp8", "fp8h") for r in (16, 32))
    # the GEMM rows of the table are what launch_gemm4's rule gives at 16 and 17 row blocks
    for shape in R.EXTRA_SHAPES:
        gx = R.PAIR_SHAPES[shape]["N"] // 256
        for rows in R.EXTRA_ROWS:
            nrb = (rows + 15) // 16
            assert R.gemm4_plan(nrb, gx, False) == [(4, 16, 0, nrb)] and "RBW=4,CT=16" in R.pair_instance(shape, "h1", rows)
            assert R.gemm4_plan(nrb, gx, True) == [(8, 8, 0, nrb)] and "RBW=8,CT=8" in R.pair_instance(shape, "h2", rows)
    assert R.gemm4_plan(166, 32, True) == [(8, 16, 0, 128), (6, 16, 128, 38)]        # the cut gemv3.hip describes: 2656 rows of w1||w3
    assert len(R.gemv_cases()) == len(R.GEMV_TABLE) * 2 * len(R.GEMV_ROWS)


def test_bounds():
    y = torch.tensor([-12.0, -3.0, -1.2785, 0.0, 0.5, 4.0, 12.0], dtype=torch.float64)
    ref, b = R.swiglu_ref_and_bound(y, torch.full_like(y, 2.0))
    assert torch.allclose(ref, torch.nn.functional.silu(y) * 2.0, rtol=1e-15, atol=0)
    rel = b[ref != 0] / ref[ref != 0].abs() / R.U
    assert float(rel.min()) >= 2 * R.C_NORM - 5 + 3 and float(rel.max()) <= R.C_NORM * 12 + 2 * R.C_NORM + 6      # condition of silu: at most 1 + |y|
    assert float(b[3]) == 0.0                                                       # exact zero in, exact zero out
    x = torch.tensor([-6.0, -2.0, -0.25, 0.0, 0.25, 2.0, 6.0], dtype=torch.float64)
    ref, b = R.gelu_ref_and_bound(x)
    assert torch.allclose(ref.float(), torch.nn.functional.gelu(x.float(), approximate="tanh"), rtol=1e-5, atol=1e-7)
    assert float(b[3]) == 0.0 and bool((b[[0, 1, 2, 4, 5, 6]] > 0).all()) and float((b / x.abs().clamp(min=1)).max()) < 40 * R.U
    out = torch.arange(64, dtype=torch.float32).view(2, 32)
    ref, b = R.ss_out_ref_and_bound(out)
    assert ref.shape == (2, 2) and float(ref[0, 0]) == sum(i * i for i in range(16)) and torch.equal(b, R.C_SS * R.U * ref * (1 + 64 * R.U))
    assert torch.equal(R.norm_bound(torch.tensor([-2.0, 0.0], dtype=torch.float64)), torch.tensor([2.0 * R.C_NORM * R.U, 0.0], dtype=torch.float64))
    ssbuf = torch.arange(2 * 2 * 16, dtype=torch.float32)
    assert float(R.ss_out_rows(ssbuf, 17, 32)[16, 1]) == float(ssbuf[(1 * 2 + 1) * 16 + 0])
