"""CPU self-checks (-m "not gpu") of tests/attention_reference.py, the fp64 reference the -m gpu attention tests compare against: it is
pinned to the fp32 step restatement of test_gpu_ops.py::test_attention_step_matches_oracle (itself pinned to the reference project),
a chunk equals its positions one by one, the storage roundings are what they say, and the k-cache exclusion rule holds — under its
cap — for the fp32 torch rotation of the very seeds the GPU tests use."""
import math

import pytest
import torch

import attention_reference as A
from oracle.decoder_oracle import apply_rope, rope_table

H, HD, D = A.H, A.HD, A.D


def _fill(qr, kr, v, rope, kv_dtype):
    """The cache an exact kernel would have appended: storage rounding of the fp32 rotation."""
    return A.narrow(A.rope32(kr, rope, 0), kv_dtype), A.narrow(v, kv_dtype)


def test_fp64_step_agrees_with_the_fp32_step_restatement():
    rows, T = 3, 40
    rope = rope_table(T, HD)
    qr, kr, v = A.family("flat", rows, T, 11, rope)
    Kc, Vc = _fill(qr, kr, v, rope, 0)
    for pos in (0, 1, 17, 39):
        ref = A.chunk_reference(qr[:, :, pos:pos + 1], kr[:, :, pos:pos + 1], v[:, :, pos:pos + 1], rope, A.widen(Kc), A.widen(Vc), pos, 0)
        # the restatement of test_attention_step_matches_oracle, on the same inputs
        qkv = torch.cat([x[:, :, pos].reshape(rows, D) for x in (qr, kr, v)], dim=-1)
        q, k, vv = qkv.split([D, D, D], dim=-1)
        q = apply_rope(q.view(rows, 1, H, HD), rope[pos:pos + 1]).transpose(1, 2)
        k = apply_rope(k.view(rows, 1, H, HD), rope[pos:pos + 1]).transpose(1, 2)
        kk = torch.cat([Kc[:, :, :pos], k], dim=2)
        vc = torch.cat([Vc[:, :, :pos], vv.view(rows, H, 1, HD)], dim=2)
        s = torch.matmul(q, kk.transpose(-1, -2)) / math.sqrt(HD)
        old = torch.matmul(torch.softmax(s, -1), vc).transpose(1, 2).reshape(rows, D)
        assert A.rel_err(old, ref["out64"][:, 0]) < 1e-6
        assert A.rel_err(ref["out32"][:, 0], ref["out64"][:, 0]) < 1e-6
        assert torch.equal(A.rope32(kr[:, :, pos:pos + 1], rope, pos), k)          # rope32 IS apply_rope


@pytest.mark.parametrize("kv_dtype", [0, 1, 2])
@pytest.mark.parametrize("name", ["flat", "late_max", "wide"])
def test_chunk_equals_its_positions_one_by_one(name, kv_dtype):
    rows, T, p0, n = 2, 48, 13, 22
    rope = rope_table(T, HD)
    qr, kr, v = A.family(name, rows, T, 5, rope)
    Kc, Vc = _fill(qr, kr, v, rope, kv_dtype)
    sl = slice(p0, p0 + n)
    chunk = A.chunk_reference(qr[:, :, sl], kr[:, :, sl], v[:, :, sl], rope, A.widen(Kc), A.widen(Vc), p0, kv_dtype)
    # the caches the single-position calls see: earlier positions of the chunk as the REFERENCE stores them
    k64, _ = A.rope64(kr[:, :, sl], rope, p0)
    Kc, Vc = Kc.clone(), Vc.clone()
    Kc[:, :, sl], Vc[:, :, sl] = A.narrow(k64, kv_dtype), A.narrow(v[:, :, sl], kv_dtype)
    for i in range(n):
        p = p0 + i
        one = A.chunk_reference(qr[:, :, p:p + 1], kr[:, :, p:p + 1], v[:, :, p:p + 1], rope, A.widen(Kc), A.widen(Vc), p, kv_dtype)
        assert A.rel_err(one["out64"][:, 0], chunk["out64"][:, i]) < 1e-12
    assert float((chunk["ones64"] - 1).abs().max()) < 1e-14


def test_storage_roundings():
    x = torch.tensor([0.0, 1.0, -1.0, 447.9, 448.0, 449.0, 600.0, -1e4, 2.0 ** -9, 0.9 * 2.0 ** -10, 1.1 * 2.0 ** -10, 6e4, 1.0 + 2.0 ** -11])
    e = A.widen(A.narrow(x, 2))
    assert e.tolist() == [0.0, 1.0, -1.0, 448.0, 448.0, 448.0, 448.0, -448.0, 2.0 ** -9, 0.0, 2.0 ** -9, 448.0, 1.0]
    h = A.widen(A.narrow(x.double(), 1))
    assert h[11] == 60000.0 and h[12] == 1.0 and torch.isfinite(h).all()
    assert A.storage_step(torch.tensor([1.0, 1.5, 2.0, 2.0 ** -14, 2.0 ** -20], dtype=torch.float64), 1).tolist() == \
        [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24]
    assert A.storage_step(torch.tensor([448.0, 1.0, 2.0 ** -9], dtype=torch.float64), 2).tolist() == [32.0, 0.125, 2.0 ** -9]


def test_families_have_the_score_structure_they_name():
    rows, T = 2, 256
    rope = rope_table(T, HD)

    def scores(name, hot=None):
        qr, kr, _ = A.family(name, rows, T, 3, rope, hot=hot)
        q, _ = A.rope64(qr[:, :, T - 1:], rope, T - 1)
        k, _ = A.rope64(kr, rope, 0)
        return (torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(HD))[:, :, 0]     # (rows, H, T): the last query against every key
    assert 0.8 < float(scores("flat").std()) < 1.2
    assert 6.5 < float(scores("peaked").std()) < 9.5
    late = scores("late_max")
    assert bool((late.argmax(-1) >= T - 16).all()) and float((late[..., -1] - late[..., 0]).mean()) > 30
    early = scores("early_max")
    assert bool((early.argmax(-1) <= 16).all()) and float((early[..., 0] - early[..., -1]).mean()) > 100
    for hot in (64, 127, 255):
        s = scores("huge_first", hot)
        rest = torch.cat([s[..., :hot], s[..., hot + 1:]], -1)
        assert bool((s.argmax(-1) == hot).all()) and float((s[..., hot] - rest.max(-1).values).min()) > 50


@pytest.mark.parametrize("kv_dtype", [0, 1, 2])
def test_k_cache_rule_holds_for_the_fp32_rotation_of_the_test_seeds(kv_dtype):
    """The exclusion cap by the reference alone: the fp32 torch rotation of every family (the seeds of test_gpu_attention.py) against the
    fp64 one, under check_stored_k — fewer than 0.1 % excluded, none beyond one step."""
    import test_gpu_attention as G
    excluded = total = 0
    for name in A.FAMILIES:
        T = 256
        rope = rope_table(T, HD)
        qr, kr, _ = A.family(name, 8, T, G.seed_of(name), rope, hot=G.hot_for(name, T - 1))
        y64, m64 = A.rope64(kr, rope, 0)
        e, n = A.check_stored_k(A.narrow(A.rope32(kr, rope, 0), kv_dtype), y64, m64, kv_dtype)
        assert e < 1e-3 * n, (name, e, n)
        excluded, total = excluded + e, total + n
    print(f"k-cache rule, {A.STORAGE[kv_dtype]}: {excluded} of {total} values at a rounding boundary")
    # and the rule is not vacuous: a value one step off that is NOT at a boundary is refused
    if kv_dtype:
        bad = A.narrow(y64, kv_dtype).clone()
        flat = bad.view(-1).view(torch.int16 if kv_dtype == 1 else torch.uint8)
        i = int(torch.nonzero((A.widen(bad).view(-1).abs() > 0.5) & (A.widen(bad).view(-1).abs() < 100))[0])
        flat[i] += 1
        with pytest.raises(AssertionError):
            A.check_stored_k(bad, y64, m64, kv_dtype)
