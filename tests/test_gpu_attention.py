"""Every decoder attention kernel and K / V storage against ONE fp64 reference (tests/attention_reference.py), at the kernel's own level:
vaura_attention_step_ex (attention_step256_kernel<96, 0|1|2>, attention_step_kernel, attention_split_kernel with the in-launch merge or
attention_combine_kernel) and vaura_attention_prefill (rope_append_kernel<96, 0|1|2> + attention_prefill_kernel<96, 0|1|2> or the
per-position kernel), through the launchers the decode step and the prefill chunk call.

Inputs: the seeded families of attention_reference.family — flat (the control), peaked, late / early maximum, one huge key (first / last of a
64-key block, the new position), wide-range values.  The narrow caches are compared on the numbers the cache HOLDS, so every storage is held
to the same bar: err = max|got - ref64| / max|ref64| <= max(3e-6, 4 e_ref), e_ref the fp32 torch restatement's error on the same inputs
(3e-6 alone on flat); again with every v = 1 (reference exactly 1: the denominator alone).  Every (row, head, position, channel) of every
case is compared.  Measured lines: set VAURA_ATTENTION_PARITY_OUT=<file> (profiles/attention_parity.txt is such a file)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_reference as A
from oracle.decoder_oracle import rope_table
from vaura_amd import _lib as L
from vaura_amd import ops
from vaura_amd.variants import Variant, variants

DEV = "cuda:0"
H, HD, D = A.H, A.HD, A.D
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.float8_e4m3fn: torch.uint8}
POS_256 = [0, 1, 63, 64, 65, 127, 128, 191, 192, 193, 254, 255]
ROWS_256 = [1, 5, 16, 32]
PREFILL_256 = [(0, 1), (0, 15), (0, 16), (0, 17), (0, 64), (0, 65), (0, 166), (40, 20), (63, 2), (64, 64), (100, 130), (255, 1)]
PREFILL_1024 = [(0, 192), (300, 192), (960, 64), (1000, 24)]
PREFILL_FAMILIES = ["flat", "peaked", "late_max", "huge_first"]


def seed_of(name):
    return 1000 + 17 * A.FAMILIES.index(name)


def hot_for(name, pos):
    """Index of the one huge key for a step (or a chunk's last query) at `pos`; None for the other families."""
    if not name.startswith("huge"):
        return None
    if name == "huge_new" or pos == 0:
        return pos
    if name == "huge_first":
        return (pos - 1) // 64 * 64                      # first key of the last (possibly partial) 64-block of the cache
    return pos // 64 * 64 - 1 if pos >= 64 else pos - 1  # last key of the last full 64-block


def bits(t):
    return t.view(BITS[t.dtype])


# ----------------------------------------------------------------------------------------------------------- reporting
_LINES = {}


def _note(kernel, kv, name, err, e_ref, what="out"):
    k = (kernel, A.STORAGE[kv], name, what)
    old = _LINES.get(k, (0.0, 0.0, 0))
    _LINES[k] = (max(old[0], err), max(old[1], e_ref), old[2] + 1)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = ["# attention kernels against the fp64 reference (tests/test_gpu_attention.py): worst case per (kernel, storage, family)",
             "# err = max|got - ref64| / max|ref64|; e_ref = the same for the fp32 torch restatement; bar = max(3e-6, 4 e_ref); 'ones' = every v = 1"]
    for (kernel, st, name, what), (err, e_ref, n) in sorted(_LINES.items()):
        lines.append(f"{kernel:28s} {st:5s} {name:11s} {what:5s} err {err:.3e}  e_ref {e_ref:.3e}  calls {n}")
    print("\n".join(lines))
    out = os.environ.get("VAURA_ATTENTION_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def _judge(kernel, kv, name, got, ref64, ref32, what, where):
    """The bar.  `where` prefixes the failure message; the worst element's (row, position in chunk, head, channel) is named."""
    got = got.double()
    assert bool(torch.isfinite(got).all()), f"{where}: non-finite output"
    err, e_ref = A.rel_err(got, ref64), A.rel_err(ref32, ref64)
    print(f"{kernel} {A.STORAGE[kv]} {name} {what} {where}: err {err:.3e} e_ref {e_ref:.3e}")
    _note(kernel, kv, name, err, e_ref, what)
    limit = 3e-6 if name == "flat" else A.bar(e_ref)
    if err > limit:
        i = int((got - ref64).abs().argmax())
        r, rem = divmod(i, ref64.shape[1] * D)
        z, rem = divmod(rem, D)
        raise AssertionError(f"{kernel} {A.STORAGE[kv]} {name} {what} {where}: err {err:.3e} > {limit:.3e} (e_ref {e_ref:.3e}); worst at row {r}, "
                             f"chunk position {z}, head {rem // HD}, channel {rem % HD}: got {float(got.reshape(-1)[i])!r} ref {float(ref64.reshape(-1)[i])!r}")


# ---------------------------------------------------------------------------------------------------------------- data
class Seq:
    """One family's sequence of T positions for up to `rows` rows: raw fp32 q / k / v on the CPU, and per storage the cache an exact
    kernel would have built (storage rounding of the fp32 rotation) — on the CPU as fp64 (what the reference reads), on the device as a
    working copy the kernels write into and a pristine copy to compare it with."""

    def __init__(self, name, rows, T):
        self.name, self.rows, self.T = name, rows, T
        self.rope = rope_table(T, HD)
        self.rope_d = self.rope.to(DEV)
        self.qr, self.kr, self.v = A.family(name, rows, T, seed_of(name), self.rope)
        self.krot = A.rope32(self.kr, self.rope, 0)
        self.st = {}

    def storage(self, kv):
        if kv not in self.st:
            Kc, Vc = A.narrow(self.krot, kv), A.narrow(self.v, kv)
            s = {"K64": A.widen(Kc), "V64": A.widen(Vc), "Kp": Kc.to(DEV), "Vp": Vc.to(DEV)}
            s["V1p"] = A.narrow(torch.ones_like(self.v), kv).to(DEV)
            s["K"], s["V"], s["V1"] = s["Kp"].clone(), s["Vp"].clone(), s["V1p"].clone()
            self.st = {kv: s}               # one storage at a time on the device
        return self.st[kv]

    def place_hot(self, hot):
        """huge_*: put the one large key at `hot` (raw k, and slot `hot` of every copy of the cache); returns what undoes it."""
        saved = (hot, self.kr[:, :, hot].clone(), self.krot[:, :, hot].clone())
        self.kr[:, :, hot] = A.huge_key(self.kr, self.rows, seed_of(self.name), self.rope, hot)
        self.krot[:, :, hot] = A.rope32(self.kr[:, :, hot:hot + 1], self.rope, hot)[:, :, 0]
        self._sync_slot(hot)
        return saved

    def undo_hot(self, saved):
        hot, self.kr[:, :, hot], self.krot[:, :, hot] = saved
        self._sync_slot(hot)

    def _sync_slot(self, hot):
        for kv, s in self.st.items():
            slot = A.narrow(self.krot[:, :, hot], kv)
            s["K64"][:, :, hot] = A.widen(slot)
            bits(s["Kp"])[:, :, hot] = bits(slot).to(DEV)
            bits(s["K"])[:, :, hot] = bits(s["Kp"])[:, :, hot]

    def chunk(self, rows, p0, n):
        sl = slice(p0, p0 + n)
        return self.qr[:rows, :, sl], self.kr[:rows, :, sl], self.v[:rows, :, sl]


_SEQS = {}


def seq_for(name, rows, T):
    key = (name, rows, T)
    if key not in _SEQS:
        _SEQS.clear()                       # one sequence alive at a time (a 256-position, 32-row fp32 cache pair is 100 MB)
        _SEQS[key] = Seq(name, rows, T)
    return _SEQS[key]


def qkv_rows(q, k, v):
    """(R, H, 1, hd) x 3 -> the step's row-major (R, 3 D)."""
    R = q.shape[0]
    return torch.cat([x[:, :, 0].reshape(R, D) for x in (q, k, v)], dim=-1)


def check_cache_after(seq, kv, rows, p0, n, ref, v_ones, counts):
    """Slots [p0, p0 + n) of rows < `rows` hold the storage's rounding of the rotated k (k-cache rule) and of v (bit-exact); every other
    slot of every row and head equals its pre-call copy (whole buffers)."""
    s = seq.storage(kv)
    sl = slice(p0, p0 + n)
    e, t = A.check_stored_k(s["K"][:rows, :, sl].cpu(), ref["k64"], ref["km"], kv)
    counts[0] += e
    counts[1] += t
    Vw = s["V1"] if v_ones else s["V"]
    v_want = A.narrow(torch.ones_like(ref["k64"]), kv) if v_ones else ref["v_stored"]
    assert torch.equal(bits(Vw[:rows, :, sl].cpu()), bits(v_want)), "new v slots are not the storage's rounding of v, bit for bit"
    bits(s["K"])[:rows, :, sl] = bits(s["Kp"])[:rows, :, sl]
    if not v_ones:
        bits(s["V"])[:rows, :, sl] = bits(s["Vp"])[:rows, :, sl]
    assert torch.equal(bits(Vw), bits(s["V1p"] if v_ones else s["Vp"])), "a v-cache slot outside the new positions changed"
    assert torch.equal(bits(s["K"]), bits(s["Kp"])), "a k-cache slot outside the new positions changed"


def poison(seq, kv, rows, p0, n, v_ones=False):
    """The slots the call must write hold garbage (7.0) before it: a missing append must not pass on the pre-filled value."""
    s = seq.storage(kv)
    for name in ("K", "V1" if v_ones else "V"):
        bits(s[name])[:rows, :, p0:p0 + n] = (0x40E00000, 0x4700, 0x4E)[kv]


def assert_k_cap(counts, where):
    assert counts[0] < 1e-3 * max(1, counts[1]), f"{where}: {counts[0]} of {counts[1]} stored k values sit at a rounding boundary (cap 0.1 %)"
    print(f"{where}: {counts[0]} of {counts[1]} stored k values at a rounding boundary")


# --------------------------------------------------------------------------------------------------------- decode step
def step_case(seq, kv, rows, pos, kernel, counts, **kw):
    """One decode-step call (and the same with every v = 1) against the reference; returns the fp32 output rows (CPU)."""
    name, s = seq.name, seq.storage(kv)
    q, k, v = seq.chunk(rows, pos, 1)
    out = ref = None
    for v_ones in (False, True):
        poison(seq, kv, rows, pos, 1, v_ones)
        qp = ops.pack_rows(qkv_rows(q, k, torch.ones_like(v) if v_ones else v).to(DEV))
        o, _ = ops.attention_step_ex(qp, seq.rope_d, s["K"], s["V1"] if v_ones else s["V"], rows, H, HD, pos, kv_dtype=kv, **kw)
        got = ops.unpack_rows(o, rows, D).cpu()
        where = f"rows {rows} pos {pos}"
        if ref is None:                      # on the numbers the cache holds: the new k as stored (check_cache_after judges it)
            ref = A.chunk_reference(q, k, v, seq.rope, s["K64"][:rows], s["V64"][:rows], pos, kv, k_stored=s["K"][:rows, :, pos:pos + 1].cpu())
        if v_ones:
            _judge(kernel, kv, name, got[:, None], ref["ones64"], ref["ones32"], "ones", where)
        else:
            _judge(kernel, kv, name, got[:, None], ref["out64"], ref["out32"], "out", where)
            out = got
        check_cache_after(seq, kv, rows, pos, 1, ref, v_ones, counts)
    return out


@pytest.mark.parametrize("kv", [0, 1, 2])
@pytest.mark.parametrize("name", A.FAMILIES)
def test_step256_every_storage_family_position_and_row_count(name, kv):
    """attention_step256_kernel<96, kv> at max_len = 256 exactly: every NU body and both sides of each switch, rows 1 / 5 / 16 / 32."""
    seq = seq_for(name, 32, 256)
    counts = [0, 0]
    for pos in POS_256:
        hot = hot_for(name, pos)
        saved = seq.place_hot(hot) if hot is not None else None
        try:
            for rows in ROWS_256:
                step_case(seq, kv, rows, pos, "step256", counts)
        finally:
            if saved is not None:
                seq.undo_hot(saved)
    assert_k_cap(counts, f"step256 {A.STORAGE[kv]} {name}")


SPLIT_ROWS = {1: 5, 2: 5, 4: 4, 8: 2}


def split_positions(n_split):
    base = [0, 1, 30, 63, 64, 65, 255, 256, 257, 511, 512, 700, 1023]
    return sorted(set(base + [64 * n_split - 1, 64 * n_split, 64 * n_split + 1]))


@pytest.mark.parametrize("n_split", [1, 2, 4, 8])
@pytest.mark.parametrize("name", A.FAMILIES)
def test_long_cache_generic_and_range_split_kernels(name, n_split):
    """max_len = 1024, fp32 cache: attention_step_kernel (n_split = 1) and attention_split_kernel with the separate combine launch and
    with the in-launch merge.  The merge runs on the SAME out / part / arrival buffers call after call (every call has other inputs than
    the one before: a stale partial would not match the reference), the arrival words read zero after each call, and its output is
    torch.equal to the separate combine launch's."""
    seq = seq_for(name, 5, 1024)
    rows = SPLIT_ROWS[n_split]
    counts = [0, 0]
    part = torch.full((rows * H * n_split * (HD + 8),), float("nan"), device=DEV)
    arrivals = torch.zeros(rows * H, dtype=torch.int32, device=DEV)
    out_buf = torch.full((16 * D,), float("nan"), device=DEV)
    for pos in split_positions(n_split):
        hot = hot_for(name, pos)
        saved = seq.place_hot(hot) if hot is not None else None
        try:
            if n_split == 1:
                step_case(seq, 0, rows, pos, "step_generic", counts)
                continue
            sep = step_case(seq, 0, rows, pos, f"split{n_split}+combine", counts, n_split=n_split)
            merged = step_case(seq, 0, rows, pos, f"split{n_split} merged", counts, n_split=n_split, part=part, arrivals=arrivals, out=out_buf)
            assert int(arrivals.abs().sum()) == 0, f"pos {pos}: arrival words not back at zero"
            assert torch.equal(merged, sep), f"pos {pos}: in-launch merge differs from the separate combine launch"
        finally:
            if saved is not None:
                seq.undo_hot(saved)
    assert_k_cap(counts, f"long cache n_split {n_split} {name}")


@pytest.mark.parametrize("kv", [1, 2])
def test_narrow_cache_refuses_long_caches_and_splits(kv):
    """fp16 / e4m3 caches exist for max_len <= 256 without a range split: everything else is VAURA_ERR_SHAPE from the step's launcher AND
    from the prefill's (a prefill the following step would refuse), and nothing is written."""
    rope = rope_table(1024, HD).to(DEV)
    rows = 2
    dt = torch.float16 if kv == 1 else torch.float8_e4m3fn
    qp = ops.pack_rows(torch.randn(rows, 3 * D, device=DEV))
    for max_len, n_split in [(1024, 1), (257, 1), (256, 2), (1024, 4)]:
        kc = torch.zeros(rows, H, max_len, HD, device=DEV).to(dt)
        vc = kc.clone()
        out = torch.full((16 * D,), float("nan"), device=DEV)
        with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE"):
            ops.attention_step_ex(qp, rope, kc, vc, rows, H, HD, 5, kv_dtype=kv, n_split=n_split, out=out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and not bool(bits(kc).ne(0).any()) and not bool(bits(vc).ne(0).any())
    for max_len in (257, 1024):
        kc = torch.zeros(rows, H, max_len, HD, device=DEV).to(dt)
        vc = kc.clone()
        qkv = ops.pack_rows(torch.randn(4 * 16, 3 * D, device=DEV))
        before = qkv.clone()
        attn = torch.full((4 * 16 * D,), float("nan"), device=DEV)
        with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE"):
            ops.attention_prefill(qkv, rope, kc, vc, attn, None, rows, H, HD, 0, 4, kv_dtype=kv)
        torch.cuda.synchronize()
        assert bool(torch.isnan(attn).all()) and torch.equal(qkv, before) and not bool(bits(kc).ne(0).any()) and not bool(bits(vc).ne(0).any())
    # argument checks of the prefill entry point
    kc = torch.zeros(rows, H, 256, HD, device=DEV).to(dt)
    attn = torch.zeros(4 * 16 * D, device=DEV)
    qkv = ops.pack_rows(torch.randn(4 * 16, 3 * D, device=DEV))
    for p0, n in [(-1, 4), (0, 0), (253, 4)]:
        with pytest.raises(L.VauraHipError, match="VAURA_ERR_ARG"):
            ops.attention_prefill(qkv, rope, kc, kc.clone(), attn, None, rows, H, HD, p0, n, kv_dtype=kv)
    with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE"):
        ops.attention_prefill(qkv, rope, kc, kc.clone(), attn, None, rows, H, 64, 0, 4, kv_dtype=kv)
    with pytest.raises(L.VauraHipError, match="VAURA_ERR_ARG"):
        ops.attention_prefill(qkv, rope, kc, kc.clone(), None, None, rows, H, HD, 0, 4, kv_dtype=kv)


def _planes_of(v):
    hi = v.half().float()
    return hi, (v - hi).half().float()


STEP_OPTION_CASES = [(0, 256, 1, 200), (1, 256, 1, 130), (2, 256, 1, 64), (0, 1024, 1, 700), (0, 1024, 4, 700), (0, 1024, 4, 30)]


@pytest.mark.parametrize("kv,max_len,n_split,pos", STEP_OPTION_CASES)
@pytest.mark.parametrize("name", ["flat", "late_max", "wide"])
def test_step_options_qkv2_and_planes(kv, max_len, n_split, pos, name):
    """qkv2: qkv given as two partials a, b against the single buffer a + b (the fp32 sum) -> torch.equal outputs and caches.
    out_split with plane_shift 0 / 3: the fp32 out is torch.equal to the call without planes (the scale does not leak), and the planes
    are bit for bit hi = fp16(v), lo = fp16(v - hi) of v = out * 2^-S.  With a split: both merges."""
    rows = 5
    seq = seq_for(name, 32 if max_len == 256 else 5, max_len)
    s = seq.storage(kv)
    q, k, v = seq.chunk(rows, pos, 1)
    qkv = qkv_rows(q, k, v).to(DEV)
    a = torch.randn(rows, 3 * D, generator=torch.Generator().manual_seed(pos), dtype=torch.float32).to(DEV) * qkv.abs().mean()
    b = qkv - a
    for arrivals in ([None] if n_split == 1 else [None, torch.zeros(rows * H, dtype=torch.int32, device=DEV)]):
        kw = dict(kv_dtype=kv, n_split=n_split, arrivals=arrivals)
        base, _ = ops.attention_step_ex(ops.pack_rows(a + b), seq.rope_d, s["K"], s["V"], rows, H, HD, pos, **kw)
        kb, vb = s["K"][:rows, :, pos].clone(), s["V"][:rows, :, pos].clone()
        poison(seq, kv, rows, pos, 1)
        two, _ = ops.attention_step_ex(ops.pack_rows(a), seq.rope_d, s["K"], s["V"], rows, H, HD, pos, qkv2_p=ops.pack_rows(b), **kw)
        assert torch.equal(two, base), "qkv + qkv2 on load differs from the single buffer holding their fp32 sum"
        assert torch.equal(bits(s["K"][:rows, :, pos]), bits(kb)) and torch.equal(bits(s["V"][:rows, :, pos]), bits(vb))
        got = ops.unpack_rows(base, rows, D)
        assert bool(torch.isfinite(got).all())
        for shift in (0, 3):
            o, osp = ops.attention_step_ex(ops.pack_rows(a + b), seq.rope_d, s["K"], s["V"], rows, H, HD, pos, want_split=True,
                                           plane_shift=shift, **kw)
            assert torch.equal(o, base), f"plane_shift {shift}: the plane scale leaked into the fp32 output"
            planes = ops.unsplit_rows(osp, rows, D)
            hi, lo = _planes_of(got * 2.0 ** -shift)
            assert torch.equal(planes[0], hi) and torch.equal(planes[1], lo), f"plane_shift {shift}: planes are not fp16(v), fp16(v - hi)"
        if arrivals is not None:
            assert int(arrivals.abs().sum()) == 0
    bits(s["K"])[:rows, :, pos], bits(s["V"])[:rows, :, pos] = bits(s["Kp"])[:rows, :, pos], bits(s["Vp"])[:rows, :, pos]
    assert torch.equal(bits(s["K"]), bits(s["Kp"])) and torch.equal(bits(s["V"]), bits(s["Vp"]))


# ------------------------------------------------------------------------------------------------------------- prefill
def prefill_case(seq, kv, rows, p0, n, kernel, counts, plane_shift=None):
    """One vaura_attention_prefill call (and the same with every v = 1): outputs against the reference, q rotated in place, k / v
    columns of ws_qkv unchanged, cache slots of the chunk written and nothing else, NaN pre-fill of every row nobody owns intact."""
    name, s = seq.name, seq.storage(kv)
    q, k, v = seq.chunk(rows, p0, n)
    ref = None
    r16 = (rows + 15) // 16 * 16
    extra = 2                                                  # positions' worth of row blocks behind the chunk that must stay NaN
    for v_ones in (False, True):
        poison(seq, kv, rows, p0, n, v_ones)
        mat = torch.full((n, r16, 3 * D), float("nan"))
        vv = torch.ones_like(v) if v_ones else v
        mat[:, :rows] = torch.cat([x.permute(2, 0, 1, 3).reshape(n, rows, D) for x in (q, k, vv)], dim=-1)
        qkv_p = ops.pack_rows(mat.view(n * r16, 3 * D).to(DEV))
        attn = torch.full(((n + extra) * r16 * D,), float("nan"), device=DEV)
        attn_split = None
        if plane_shift is not None:
            attn_split = torch.full(((n + extra) * r16 * 2 * D,), 0x7e00, dtype=torch.int16, device=DEV)      # fp16 NaN
        ops.attention_prefill(qkv_p, seq.rope_d, s["K"], s["V1"] if v_ones else s["V"], attn, attn_split, rows, H, HD, p0, n,
                              kv_dtype=kv, plane_shift=plane_shift or 0)
        o = ops.unpack_rows(attn, (n + extra) * r16, D).cpu().view(n + extra, r16, D)
        got = o[:n, :rows].transpose(0, 1)                     # (rows, n, D)
        where = f"rows {rows} chunk ({p0}, {n})" + ("" if plane_shift is None else f" plane_shift {plane_shift}")
        if ref is None:                      # on the numbers the cache holds: the chunk's k as stored (check_cache_after judges it)
            ref = A.chunk_reference(q, k, v, seq.rope, s["K64"][:rows], s["V64"][:rows], p0, kv, k_stored=s["K"][:rows, :, p0:p0 + n].cpu())
        if v_ones:
            _judge(kernel, kv, name, got, ref["ones64"], ref["ones32"], "ones", where)
        else:
            _judge(kernel, kv, name, got, ref["out64"], ref["out32"], "out", where)
        assert bool(torch.isnan(o[n:]).all()) and bool(torch.isnan(o[:n, rows:]).all()), f"{where}: ws_attn rows outside the chunk were written"
        if attn_split is not None:
            planes = ops.unsplit_rows(attn_split, (n + extra) * r16, D).cpu().reshape(2, n + extra, r16, D)
            hi, lo = _planes_of(o[:n, :rows] * 2.0 ** -plane_shift)
            assert torch.equal(planes[0, :n, :rows], hi) and torch.equal(planes[1, :n, :rows], lo), f"{where}: planes are not fp16(v), fp16(v - hi)"
            assert bool(torch.isnan(planes[:, n:]).all()) and bool(torch.isnan(planes[:, :n, rows:]).all()), f"{where}: ws_attn_split rows outside the chunk were written"
        back = ops.unpack_rows(qkv_p, n * r16, 3 * D).cpu().view(n, r16, 3 * D)
        assert bool(torch.isnan(back[:, rows:]).all())
        assert torch.equal(back[:, :rows, D:], mat[:, :rows, D:]), f"{where}: k / v columns of ws_qkv changed"
        q_back = back[:, :rows, :D].reshape(n, rows, H, HD).permute(1, 2, 0, 3)
        A.check_stored_k(q_back, ref["q64"], ref["qm"], 0)     # the fp32 rule: q rotated in place
        check_cache_after(seq, kv, rows, p0, n, ref, v_ones, counts)


def _prefill_rows(i, kv):
    return [1, 5, 20][(i + kv) % 3]


@pytest.mark.parametrize("kv", [0, 1, 2])
@pytest.mark.parametrize("name", PREFILL_FAMILIES)
def test_prefill_chunks_every_storage(name, kv):
    """rope_append_kernel<96, kv> + attention_prefill_kernel<96, kv> at max_len = 256: chunks that start at p0 > 0, ragged n_pos, a single
    position, the last slot; rows 1 / 5 / 20 in turn (all three on the two largest chunks); planes with plane_shift 0 / 3 in turn."""
    seq = seq_for(name, 20, 256)
    counts = [0, 0]
    for i, (p0, n) in enumerate(PREFILL_256):
        last = p0 + n - 1
        hot = None if not name.startswith("huge") else (last // 64 * 64 - (i % 2) if last >= 64 else (last if i % 2 else 0))
        saved = seq.place_hot(hot) if hot is not None else None
        try:
            for rows in ([1, 5, 20] if (p0, n) in [(0, 166), (100, 130)] else [_prefill_rows(i, kv)]):
                prefill_case(seq, kv, rows, p0, n, "prefill_mfma", counts, plane_shift=[None, 0, 3][(i + rows) % 3])
        finally:
            if saved is not None:
                seq.undo_hot(saved)
    assert_k_cap(counts, f"prefill {A.STORAGE[kv]} {name}")


@pytest.mark.parametrize("per_position", [False, True])
@pytest.mark.parametrize("name", PREFILL_FAMILIES)
def test_prefill_long_cache_and_per_position_kernel(name, per_position):
    """fp32 cache, max_len = 1024 (several 64-key blocks before the chunk, chunks of three query blocks) and — PREFILL_ATTN_PER_POSITION — the
    per-position kernel on the same cases and on the 256-position ones: both kernels within the bar of the same reference."""
    counts = [0, 0]
    with variants(Variant.PREFILL_ATTN_PER_POSITION if per_position else 0):
        kernel = "prefill_per_position" if per_position else "prefill_mfma"
        seq = seq_for(name, 5, 1024)
        for i, (p0, n) in enumerate(PREFILL_1024):
            last = p0 + n - 1
            hot = None if not name.startswith("huge") else last // 64 * 64 - (i % 2)
            saved = seq.place_hot(hot) if hot is not None else None
            try:
                prefill_case(seq, 0, [5, 1][i % 2], p0, n, kernel, counts, plane_shift=[None, 3][i % 2])
            finally:
                if saved is not None:
                    seq.undo_hot(saved)
        if per_position:
            seq = seq_for(name, 20, 256)
            for i, (p0, n) in enumerate(PREFILL_256):
                last = p0 + n - 1
                hot = None if not name.startswith("huge") else (last // 64 * 64 - (i % 2) if last >= 64 else (last if i % 2 else 0))
                saved = seq.place_hot(hot) if hot is not None else None
                try:
                    prefill_case(seq, 0, _prefill_rows(i, 0), p0, n, kernel, counts, plane_shift=[0, None, 3][i % 3])
                finally:
                    if saved is not None:
                        seq.undo_hot(saved)
    assert_k_cap(counts, f"prefill long / per-position {name}")


@pytest.mark.parametrize("kv", [0, 1, 2])
@pytest.mark.parametrize("name", ["flat", "late_max"])
def test_step_and_prefill_leave_the_same_cache(name, kv):
    """The same 40 positions once as ONE prefill call and once as 40 step calls, from empty caches: v caches torch.equal in every storage,
    k caches each under the k-cache rule against the reference (so they differ from each other only at counted rounding boundaries), the
    last position's outputs agree within the bar and each matches the reference on the cache its own path built."""
    rows, n, T = 5, 40, 256
    seq = seq_for(name, 20, T)
    q, k, v = seq.chunk(rows, 0, n)
    dt = A.narrow(torch.zeros(1), kv).dtype
    empty = lambda: torch.zeros(rows, H, T, HD, device=DEV).to(dt)
    # one prefill call
    Kp, Vp = empty(), empty()
    mat = torch.zeros(n, 16, 3 * D)
    mat[:, :rows] = torch.cat([x.permute(2, 0, 1, 3).reshape(n, rows, D) for x in (q, k, v)], dim=-1)
    attn = torch.zeros(n * 16 * D, device=DEV)
    ops.attention_prefill(ops.pack_rows(mat.view(n * 16, 3 * D).to(DEV)), seq.rope_d, Kp, Vp, attn, None, rows, H, HD, 0, n, kv_dtype=kv)
    out_p = ops.unpack_rows(attn, n * 16, D).cpu().view(n, 16, D)[n - 1, :rows]
    # forty step calls
    Ks, Vs = empty(), empty()
    for pos in range(n):
        o, _ = ops.attention_step_ex(ops.pack_rows(qkv_rows(*seq.chunk(rows, pos, 1)).to(DEV)), seq.rope_d, Ks, Vs, rows, H, HD, pos, kv_dtype=kv)
    out_s = ops.unpack_rows(o, rows, D).cpu()
    assert torch.equal(bits(Vs), bits(Vp)), "v caches of the step path and the prefill path differ"
    k64, km = A.rope64(k, seq.rope, 0)
    es, t = A.check_stored_k(Ks[:, :, :n].cpu(), k64, km, kv)
    ep, _ = A.check_stored_k(Kp[:, :, :n].cpu(), k64, km, kv)
    assert es < 1e-3 * t and ep < 1e-3 * t
    n_diff = int((bits(Ks) != bits(Kp)).sum())
    assert n_diff <= es + ep and not bool(bits(Ks[:, :, n:]).ne(0).any()) and not bool(bits(Kp[:, :, n:]).ne(0).any())
    print(f"step / prefill caches {A.STORAGE[kv]} {name}: k differs in {n_diff} of {t} values (at a boundary: step {es}, prefill {ep})")
    e_ref = 0.0
    for path, Kc, Vc, got in (("step", Ks, Vs, out_s), ("prefill", Kp, Vp, out_p)):
        ql, kl, vl = seq.chunk(rows, n - 1, 1)
        ref = A.chunk_reference(ql, kl, vl, seq.rope, A.widen(Kc.cpu()), A.widen(Vc.cpu()), n - 1, kv, k_stored=Kc[:, :, n - 1:n].cpu())
        _judge(f"consistency {path}", kv, name, got[:, None], ref["out64"], ref["out32"], "out", f"40 positions via {path}")
        e_ref = max(e_ref, A.rel_err(ref["out32"], ref["out64"]))
    d = A.rel_err(out_s, out_p)
    assert d <= (3e-6 if name == "flat" else A.bar(e_ref)), f"last position: step and prefill outputs differ by {d:.3e}"


# ------------------------------------------------------------------- the two op-level step entry points are one launcher
def _c_step_ex(qp, rope, kc, vc, out, out_split, rows, n_head, head_dim, pos, kv):
    """vaura_attention_step_ex itself (ops.attention_step_ex goes through attention_step_kv); returns the C return code."""
    return L.lib().vaura_attention_step_ex(L.ptr(qp), 0, L.ptr(rope), L.ptr(kc), L.ptr(vc), L.ptr(out), L.ptr(out_split), 0, 0,
                                           rows, n_head, head_dim, kc.shape[-2], pos, 1, 0, kv, L.current_stream())


@pytest.mark.parametrize("kv", [0, 1, 2])
def test_step_ex_and_step_kv_are_bit_identical(kv):
    """ops.attention_step_ex, ops.attention_step_kv and the C entry point vaura_attention_step_ex: the same bits in out, out_split and
    both caches, on an empty cache and on both sides of a 64-position pass boundary."""
    rows, nh, T = 2, 2, 128
    g = torch.Generator().manual_seed(77 + kv)
    rope = rope_table(T, HD).to(DEV)
    K0, V0 = (A.narrow(torch.randn(rows, nh, T, HD, generator=g), kv).to(DEV) for _ in range(2))
    for pos in (0, 63, 64):
        qp = ops.pack_rows(torch.randn(rows, 3 * nh * HD, generator=g).to(DEV))
        got = []
        for fn in (ops.attention_step_ex, ops.attention_step_kv, None):
            kc, vc = K0.clone(), V0.clone()
            if fn is not None:
                o, osp = fn(qp, rope, kc, vc, rows, nh, HD, pos, kv_dtype=kv, want_split=True)
            else:
                o, osp = torch.zeros(16 * nh * HD, device=DEV), torch.zeros(16 * 2 * nh * HD, dtype=torch.int16, device=DEV)
                assert _c_step_ex(qp, rope, kc, vc, o, osp, rows, nh, HD, pos, kv) == 0
            got.append((o, osp, bits(kc), bits(vc)))
        assert bool(torch.isfinite(got[0][0]).all()) and bool(got[0][0].ne(0).any())
        for other in got[1:]:
            for a, b, what in zip(got[0], other, ("out", "out_split", "k cache", "v cache")):
                assert torch.equal(a, b), f"storage {A.STORAGE[kv]} pos {pos}: {what} differs between the entry points"


def test_op_level_refusals():
    """What the cache check refuses, through the op-level entry points: the documented code, and nothing launched (out stays NaN, the
    caches stay zero)."""
    rows, T = 2, 128
    rope = rope_table(512, HD).to(DEV)
    qp = ops.pack_rows(torch.randn(rows, 3 * D, device=DEV))
    qkv = ops.pack_rows(torch.randn(4 * 16, 3 * D, device=DEV))
    out = torch.full((16 * D,), float("nan"), device=DEV)
    attn = torch.full((4 * 16 * D,), float("nan"), device=DEV)
    cache = lambda dt, max_len=T, hd=HD: torch.zeros(rows, H, max_len, hd, device=DEV).to(dt)
    u8, before = cache(torch.uint8), qkv.clone()
    f32_64, f16_288 = cache(torch.float32, hd=64), cache(torch.float16, 288)
    ks = torch.zeros(rows, H, T, dtype=torch.uint8, device=DEV)
    step, prefill = ops.attention_step_kv, lambda kc, hd, **kw: ops.attention_prefill(qkv, rope, kc, kc.clone(), attn, None, rows, H, hd, 0, 4, **kw)
    table = [
        ("VAURA_ERR_SHAPE", lambda: step(qp, rope, f32_64, f32_64.clone(), rows, H, 64, 5, out=out)),
        ("VAURA_ERR_SHAPE", lambda: ops.attention_step_ex(qp, rope, f32_64, f32_64.clone(), rows, H, 64, 5, out=out)),
        ("VAURA_ERR_SHAPE", lambda: prefill(f32_64, 64)),
        ("VAURA_ERR_SHAPE", lambda: step(qp, rope, f16_288, f16_288.clone(), rows, H, HD, 5, kv_dtype=1, out=out)),
        ("VAURA_ERR_SHAPE", lambda: prefill(f16_288, HD, kv_dtype=1)),
        ("VAURA_ERR_ARG", lambda: step(qp, rope, u8, u8.clone(), rows, H, HD, 5, kv_dtype=3, out=out)),
        ("VAURA_ERR_ARG", lambda: step(qp, rope, u8, u8.clone(), rows, H, HD, 5, kv_dtype=3, kscale=ks, out=out)),
        ("VAURA_ERR_ARG", lambda: prefill(u8, HD, kv_dtype=3)),
        ("VAURA_ERR_ARG", lambda: ops.attention_step_ex(qp, rope, u8, u8.clone(), rows, H, HD, 5, kv_dtype=3, out=out)),
        ("VAURA_ERR_ARG", lambda: step(qp, rope, u8, u8.clone(), rows, H, HD, 5, kv_dtype=4, kscale=ks, vscale=ks.clone(), out=out)),
        ("VAURA_ERR_ARG", lambda: prefill(u8, HD, kv_dtype=4, kscale=ks, vscale=ks.clone())),
        # missing exponent bytes AND a wrong head_dim: the step's launcher reports the bytes, the prefill's entry point checks them first too
        ("VAURA_ERR_ARG", lambda: step(qp, rope, u8, u8.clone(), rows, H, 64, 5, kv_dtype=3, out=out)),
        ("VAURA_ERR_ARG", lambda: prefill(u8, 64, kv_dtype=3)),
    ]
    for i, (code, call) in enumerate(table):
        with pytest.raises(L.VauraHipError, match=code):
            call()
        print(f"refusal {i}: {code}")
    assert _c_step_ex(qp, rope, u8, u8.clone(), out, None, rows, H, HD, 5, 3) == -1      # VAURA_ERR_ARG from the C entry point itself
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(attn).all())
    assert not any(bool(t.ne(0).any()) for t in (u8, f32_64, f16_288, ks)) and torch.equal(qkv, before)
