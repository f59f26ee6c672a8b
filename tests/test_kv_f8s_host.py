"""The scaled e4m3 K / V storage rule (kv_dtype = 3) on the CPU restatement alone (tests/kv_f8s_reference.py): range, scale invariance,
the per-element error bound, non-finite and zero vectors, and the cap on the boundary sets that tests/test_gpu_kv_f8s.py excludes when it
compares the device's stored k bits — asserted here on the reference, so the cap does not depend on any kernel."""
import pytest
import torch

import attention_reference as A
import kv_f8s_reference as F
from oracle.decoder_oracle import rope_table

ROWS, T = 2, 256
SEED = {name: 1000 + 17 * i for i, name in enumerate(A.FAMILIES)}
CASES = [(name, 0) for name in A.FAMILIES] + [("wide", -20), ("wide", 12)]
_INPUTS = {}


def inputs(name, j):
    """(rotated k fp32, v fp32, rope64 of the raw k: y64, m64), each (ROWS, H, T, 96), of a family scaled by 2^j."""
    if (name, j) not in _INPUTS:
        rope = rope_table(T, A.HD)
        _, kr, v = A.family(name, ROWS, T, SEED[name], rope, hot=100 if name.startswith("huge") else None)
        kr, v = kr * 2.0 ** j, v * 2.0 ** j
        _INPUTS[(name, j)] = (A.rope32(kr, rope, 0), v, *A.rope64(kr, rope, 0))
    return _INPUTS[(name, j)]


@pytest.mark.parametrize("name,j", CASES)
def test_range_error_bound_and_scale_invariance(name, j):
    k, v, _, _ = inputs(name, j)
    for x in (k, v):
        b, eb = F.quantise(x)
        e = eb.long() - 127
        amax = x.abs().amax(-1).double()
        s = F.scaled(x, e).abs()
        assert float(s.max()) <= 448.0, "a scaled element exceeds 448"
        assert bool((s.amax(-1)[amax > 0] > 224.0).all()), "a non-zero vector's scaled maximum is not in (224, 448]"
        err = (F.widen(b, eb) - x.double()).abs()
        bound = 2.0 ** -4 * x.double().abs() + 2.0 ** -10 * (amax / 224.0)[..., None]
        assert bool((err <= bound).all()), f"|widen - x| beyond 2^-4 |x| + 2^-10 amax / 224: worst excess {float((err - bound).max()):.3e}"
        for jj in (-20, -8, 5, 12):
            b2, eb2 = F.quantise(x * 2.0 ** jj)
            assert torch.equal(b2, b) and torch.equal(eb2.long(), eb.long() + jj), f"quantise(2^{jj} x) is not (same bytes, exponent + {jj})"


def test_non_finite_and_zero_vectors():
    x = torch.randn(6, A.HD)
    x[1, 5], x[2, 90], x[3, 0], x[4] = float("inf"), float("nan"), float("-inf"), 0.0
    x[5, 3] = -0.0
    b, eb = F.quantise(x)
    w = F.widen(b, eb)
    for r in (1, 2, 3):
        assert int(eb[r]) == 0xFF and bool(torch.isnan(w[r]).all()), "a vector holding an inf / NaN must widen to all-NaN, exponent byte 0xFF"
    assert bool(torch.isfinite(w[[0, 4, 5]]).all()) and int(eb[0]) != 0xFF
    assert int(eb[4]) == 0 and bool((w[4] == 0).all()) and bool((b[4] == 0).all()), "an all-zero vector widens to exact zeros (e = -127)"
    # the clamp: the largest and smallest fp32 magnitudes stay inside [-127, 127] and finite
    big, tiny = torch.full((1, A.HD), 3.0e38), torch.full((1, A.HD), 1.0e-44)
    assert int(F.quantise(big)[1]) == 127 + 120 and bool(torch.isfinite(F.cache64(big)).all())
    assert int(F.quantise(tiny)[1]) == 0 and bool(torch.isfinite(F.cache64(tiny)).all())


def test_exponent_is_the_smallest_that_fits():
    """e against its definition on exact cases around 448 2^n and 224 2^n."""
    for n in (-30, -1, 0, 7, 40):
        for a, want in ((448.0, n), (448.0 * (1 + 2.0 ** -23), n + 1), (224.0, n - 1), (224.0 * (1 + 2.0 ** -23), n)):
            x = torch.zeros(1, A.HD)
            x[0, 17] = -a * 2.0 ** n
            assert int(F.quantise(x)[1]) - 127 == want, (n, a)


def test_boundary_sets_stay_under_the_cap():
    """The shares the GPU test excludes, on the reference alone: vectors whose fp64 amax / 448 is within 1e-6 (relative) of a power of two,
    and k elements at an e4m3 rounding boundary (attention_reference.check_stored_k's window, on the scaled values): each < 0.1 %."""
    nv = tv = ne = te = 0
    for name, j in CASES:
        k, v, y64, m64 = inputs(name, j)
        for amax in (y64.abs().amax(-1), v.double().abs().amax(-1)):
            near = F.near_power_of_two(amax)
            nv, tv = nv + int(near.sum()), tv + near.numel()
        el = F.boundary_elements(y64, m64, F.exponent(y64.abs().amax(-1)))
        ne, te = ne + int(el.sum()), te + el.numel()
        # and the fp32 torch rotation itself obeys the k rule
        F.check_stored_k(*F.quantise(k), y64, m64)
    print(f"vectors near a power of two: {nv} of {tv}; k elements at a rounding boundary: {ne} of {te}")
    assert nv < 1e-3 * tv and ne < 1e-3 * te
