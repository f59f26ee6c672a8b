"""tests/sampler_edges_reference.py on the CPU: every built row meets the margins that make its expected token a matter of structure,
the reference returns that token in fp32 and in fp64, it equals oracle/sampling_oracle.py wherever the oracle is defined, and each of
four wrong implementations is told from it by named rows — so the device tests of tests/test_gpu_sampler_edges.py can fail."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_edges_reference as E  # noqa: E402
from oracle import sampling_oracle as so  # noqa: E402
from vaura_amd import synth  # noqa: E402

CASES = E.all_cases()
GROUPS = ("topk", "radix", "topp_order", "topp_cut", "greedy", "greedy_cfg")


def by_group(group):
    return [c for c in CASES if c.group == group]


def oracle_token(case):
    """oracle/sampling_oracle.py on one row; rows that already are probabilities enter behind its softmax"""
    p = case.params
    row, q = E.mixed(case)[None, None], case.noise[None]
    if not p.input_is_probs:
        return int(so.next_token(row, use_sampling=p.use_sampling, temp=p.temp, top_k=min(p.top_k, E.V), top_p=p.top_p, noise=q)[0, 0, 0])
    if p.top_p > 0.0:
        ps, order = so.top_p_sorted(row, p.top_p)
        return int(torch.gather(order, -1, so.draw(ps, q[None]))[0, 0, 0])
    return int(so.draw(so.top_k_filter(row, min(p.top_k, E.V)), q[None])[0, 0, 0])


def test_the_rows_are_the_ones_the_groups_describe():
    n = {g: len(by_group(g)) for g in GROUPS}
    print("rows per group:", n, "launches:", len(E.launches(CASES)))
    assert n == {"topk": 48, "radix": 38, "topp_order": 111, "topp_cut": 10, "greedy": 13, "greedy_cfg": 12}
    assert len({c.id for c in CASES}) == len(CASES)
    for c in CASES:
        assert c.x.shape == (E.V,) and c.x.dtype == torch.float32 and c.noise.dtype == torch.float32, c.id
        small = torch.nonzero(c.noise != 1.0)[:, 0].tolist()
        if c.params.use_sampling:
            assert len(small) == 1 and float(c.noise[small[0]]) == np.float32(E.Q_SMALL), c.id
        assert (c.u is not None) == (c.params.cfg_scale > 1.0), c.id
    # 1: nine tokens share the threshold wherever the vocabulary has room, and the k-th rank lies inside them
    for c in by_group("topk"):
        kk = min(c.params.top_k, E.V)
        srt = torch.sort(c.x, descending=True).values
        tied = int((c.x == srt[kk - 1]).sum())
        assert tied == min(9, E.V - max(kk - 4, 0)) and float(srt[kk - 1]) == 0.0, c.id
        if kk < 1023:
            assert float(srt[kk]) == 0.0 and int((c.x == -0.5).sum()) == 1, c.id        # rank k + 1 is tied too: ">= k-th" keeps more than k
    # 2: the keys of a byte row differ in that byte only
    for name, keys in E._radix_keys().items():
        diff = int(np.bitwise_or.reduce(np.asarray(keys, dtype=np.int64) ^ int(keys[0])))
        want = {"byte0": 0xFF, "byte1": 0xFF00, "byte2": 0xFF0000, "byte3": 0x03000000, "equal": 0}.get(name)
        assert diff == want if want is not None else diff >> 24 == 1, (name, hex(diff))
    # 5: under CFG neither input row holds the tie by itself
    for c in by_group("greedy_cfg"):
        m = E.mixed(c)
        ids = torch.nonzero(m == m.max())[:, 0]
        assert len(ids) >= 2 and len(torch.unique(c.x[ids])) > 1 and len(torch.unique(c.u[ids])) > 1, c.id
        assert bool((m == torch.round(m)).all()) and float(m.abs().max()) <= 8 and float(c.x.abs().max()) <= 32, c.id


@pytest.mark.parametrize("group", GROUPS)
def test_margins_and_expected_tokens(group):
    """draw margin, membership margin, no subnormal probability, exact dyadic sums, the logit range; the reference's token in fp32 and
    fp64 is the expected one; the oracle agrees wherever its order is defined"""
    worst = {"draw": float("inf"), "member": float("inf"), "cut": float("inf")}
    n_oracle = 0
    for c in by_group(group):
        m = E.margins(c)
        assert m.winner == c.expect == E.reference_token(c) == E.reference_token(c, torch.float64), c.id
        assert m.normal and m.range_ok and m.dyadic_ok, (c.id, m)
        if c.first_index:
            assert m.first_ok, (c.id, m)
            if not c.params.use_sampling:
                assert m.draw >= 1.0, (c.id, m)              # greedy: everything that is not the maximum lies a whole unit below
        else:
            assert m.draw >= 100.0, (c.id, m)
            worst["draw"] = min(worst["draw"], m.draw)
        assert m.member >= 1e-3, (c.id, m)
        assert m.cut >= 1e-4, (c.id, m)
        worst["member"], worst["cut"] = min(worst["member"], m.member), min(worst["cut"], m.cut)
        if c.dyadic and not c.params.input_is_probs:         # the all-equal logits row: the softmax itself is exact
            assert bool((torch.softmax(c.x / 1.0, -1) == 2.0 ** -10).all()), c.id
        if not E.has_top_p_tie(c):
            assert oracle_token(c) == c.expect, c.id
            n_oracle += 1
    print(f"{group}: smallest draw margin {worst['draw']:.1f}, membership {worst['member']:.3g}, cut {worst['cut']:.3g}; "
          f"{n_oracle} of {len(by_group(group))} rows compared with the oracle")
    assert n_oracle == {"topk": 48, "radix": 38, "topp_order": 16, "topp_cut": 0, "greedy": 13, "greedy_cfg": 12}[group]


def test_the_strict_cut_sits_on_its_boundary():
    """group 4: the last kept rank's cs - p EQUALS top_p (or, top_p = 1, nothing reaches it), the first dropped rank is one step above"""
    for c in by_group("topp_cut"):
        probs = c.x if c.params.input_is_probs else torch.softmax(c.x, -1)
        ps = torch.sort(probs, descending=True, stable=True).values
        cut = torch.cumsum(ps, -1) - ps
        top_p = np.float32(c.params.top_p)
        kept = int((~(cut > top_p)).sum())
        if c.name.startswith("full"):
            assert kept == E.V
        else:
            assert float(cut[kept - 1]) == float(top_p) and float(cut[kept]) > float(top_p) and float(ps[kept]) > 0.0, c.id
    c = next(c for c in by_group("topp_order") if c.name == "equal_r1023_dropped")
    assert np.float32(1023.0 / 1024.0) > np.float32(c.params.top_p) > np.float32(1022.0 / 1024.0)


MUTANT_ROWS = {
    "exact_k": ("topk", "k1_t1.0_hi"),                    # keeps one of nine tied maxima, the lowest id: the highest-id one cannot win
    "higher_id_first": ("topp_order", "equal_r3"),        # rank 3 of 1024 equal values must be token 3
    "cut_ge": ("topp_cut", "dyadic_p0.5_last_kept"),      # cs - p == top_p: kept by ">", dropped by ">="
    "last_wave": ("greedy", "waves_0_3"),                 # tokens 7 and 900 share the maximum: 7
}


@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_a_wrong_implementation_is_told_from_the_reference(mutant):
    """keep-exactly-k, an order among equals other than lower-id-first, ">=" in place of the strict cut, last wave wins: the rows on
    which each returns another token than the expected one (no device involved)"""
    failing = [c for c in CASES if E.reference_token(c, mutant=mutant) != c.expect]
    groups = sorted({c.group for c in failing})
    print(f"{mutant}: {len(failing)} rows fail ({groups}), e.g. {[c.id for c in failing[:4]]}")
    assert MUTANT_ROWS[mutant] in {(c.group, c.name) for c in failing}
    floor = {"exact_k": 20, "higher_id_first": 60, "cut_ge": 4, "last_wave": 10}[mutant]
    assert len(failing) >= floor


def test_golden_tie_rows_against_the_stable_reference(golden):
    """tests/golden/sampling.npz under top-p: the stable reference returns the reference project's tokens on every row without an exact
    tie, and on the two tie rows — where the recorded token depends on an order torch.sort does not define — its draw is not a near
    decision: the winner's ratio leads by more than 1e-3 relative and no cs - p lies within 1e-5 of top_p (fp64)."""
    g = golden("sampling.npz")
    logits = torch.from_numpy(g["logits"])
    noise = synth.exp_noise(1, 27, E.V, int(g["noise_seed"]))[0]
    for name, top_k, top_p in E.GOLDEN_TOP_P:
        for temp in (1.0, 0.7):
            tok = E.next_token(logits, use_sampling=True, temp=temp, top_k=top_k, top_p=top_p, noise=noise)
            keep = np.ones((3, 9), dtype=bool)
            for b, k in E.GOLDEN_TIE_ROWS:
                keep[b, k] = False
            assert np.array_equal(tok.numpy()[keep], g[f"{name}_t{temp}_tok"][keep])
            tok64 = E.next_token(logits, use_sampling=True, temp=temp, top_k=top_k, top_p=top_p, noise=noise, dtype=torch.float64)
            for b, k in E.GOLDEN_TIE_ROWS:
                assert int(tok[b, k, 0]) == int(tok64[b, k, 0])
                c = E.Case("golden", f"{name}_t{temp}_{b}_{k}", E.Params(True, temp, top_k, top_p), logits[b, k], noise[b * 9 + k], int(tok[b, k, 0]))
                m = E.margins(c)
                print(f"golden tie row {c.name}: token {c.expect}, draw margin {m.draw:.4f}, cut margin {m.cut:.3g}")
                assert m.winner == c.expect and m.draw >= 1.0 + 1e-3 and m.cut >= 1e-5 and m.normal
