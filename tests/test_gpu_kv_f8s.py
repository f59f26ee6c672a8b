"""The scaled e4m3 K / V cache (kv_dtype = 3 / "f8s": 96 e4m3 bytes + one E8M0 exponent byte per cached vector) on the device:
attention_step256_kernel<96, 3>, rope_append_kernel<96, 3> and attention_prefill_kernel<96, 3> through vaura_attention_step_kv and
vaura_attention_prefill, then DecoderEngine(kv_dtype="f8s").  Stored bits against the CPU restatement (tests/kv_f8s_reference.py), the
arithmetic against attention_reference.chunk_reference on the numbers the cache holds with the bar of every other storage, exact scale
invariance, the derivable quantisation bound, non-finite vectors and the refusals.  max_len = 256, 16 heads x 96 throughout.
Measured lines: with VAURA_ATTENTION_PARITY_OUT=<dir>/<file> set, <dir>/attention_parity_f8s.txt and <dir>/kv_f8s_loss.txt are written
(profiles/ holds such files)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_reference as A
import kv_f8s_reference as F
from oracle.decoder_oracle import rope_table
from vaura_amd import _lib as L
from vaura_amd import ops, synth
from vaura_amd.engine import DecoderEngine

DEV = "cuda:0"
H, HD, D, T = A.H, A.HD, A.D, 256
POS = [0, 1, 63, 64, 65, 127, 128, 191, 192, 193, 254, 255]
ROWS = [1, 5, 16, 32]
PREFILL = [(0, 1), (0, 17), (0, 64), (40, 20), (63, 2), (100, 130), (255, 1)]
POISON_B, POISON_E = 0x4E, 0x55


def seed_of(name):
    return 1000 + 17 * A.FAMILIES.index(name)


def hot_for(name, pos):
    """Index of the one huge key for a step (or a chunk's last query) at `pos`, as in tests/test_gpu_attention.py; None otherwise."""
    if not name.startswith("huge"):
        return None
    if name == "huge_new" or pos == 0:
        return pos
    if name == "huge_first":
        return (pos - 1) // 64 * 64
    return pos // 64 * 64 - 1 if pos >= 64 else pos - 1


def _out_dir():
    p = os.environ.get("VAURA_ATTENTION_PARITY_OUT")
    return os.path.dirname(os.path.abspath(p)) if p else None


# ----------------------------------------------------------------------------------------------------------- reporting
_LINES = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = ["# scaled e4m3 K / V cache against the fp64 reference (tests/test_gpu_kv_f8s.py): worst case per (kernel, storage, family)",
             "# err = max|got - ref64| / max|ref64|; e_ref = the same for the fp32 torch restatement; bar = max(3e-6, 4 e_ref); 'ones' = every v = 1"]
    for (kernel, name, what), (err, e_ref, n) in sorted(_LINES.items()):
        lines.append(f"{kernel:28s} {'f8s':5s} {name:11s} {what:5s} err {err:.3e}  e_ref {e_ref:.3e}  calls {n}")
    print("\n".join(lines))
    if _out_dir() and _LINES:
        with open(os.path.join(_out_dir(), "attention_parity_f8s.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")


def judge(kernel, name, got, ref64, ref32, what, where, keep=None):
    """The bar of every storage: err <= max(3e-6, 4 e_ref), 3e-6 alone on flat; every (row, position, head, channel) compared.
    keep (rows, H) bool: the (row, head) pairs that take part (the others are judged by the caller)."""
    got = got.double()
    if keep is not None:
        m = keep[:, None, :, None].expand(got.shape[0], got.shape[1], H, HD).reshape(got.shape)
        got, ref64, ref32 = torch.where(m, got, 0.0), torch.where(m, ref64, 0.0), torch.where(m, ref32.double(), 0.0)
    assert bool(torch.isfinite(got).all()), f"{where}: non-finite output"
    err, e_ref = A.rel_err(got, ref64), A.rel_err(ref32, ref64)
    print(f"{kernel} f8s {name} {what} {where}: err {err:.3e} e_ref {e_ref:.3e}")
    old = _LINES.get((kernel, name, what), (0.0, 0.0, 0))
    _LINES[(kernel, name, what)] = (max(old[0], err), max(old[1], e_ref), old[2] + 1)
    limit = 3e-6 if name == "flat" else A.bar(e_ref)
    assert err <= limit, f"{kernel} f8s {name} {what} {where}: err {err:.3e} > {limit:.3e} (e_ref {e_ref:.3e})"


# ---------------------------------------------------------------------------------------------------------------- data
class Seq:
    """One family's 256 positions for 32 rows: raw q / k / v on the CPU, the cache the restatement builds from the fp32 rotation (bytes and
    exponent bytes; fp64 widened for the reference), a working copy on the device and a pristine one to compare it with."""

    def __init__(self, name, rows=32, vscale=0, v=None, krot=None):
        self.name, self.rows = name, rows
        self.rope = rope_table(T, HD)
        self.rope_d = self.rope.to(DEV)
        self.qr, self.kr, self.v = A.family(name, rows, T, seed_of(name), self.rope)
        self.v = (self.v if v is None else v) * 2.0 ** vscale
        self.krot = A.rope32(self.kr, self.rope, 0) if krot is None else krot
        self.build()

    def build(self):
        (self.Kb, self.Ke), (self.Vb, self.Ve) = F.quantise(self.krot), F.quantise(self.v)
        (self.V1b, self.V1e) = F.quantise(torch.ones_like(self.v))
        self.K64, self.V64, self.V164 = F.widen(self.Kb, self.Ke), F.widen(self.Vb, self.Ve), F.widen(self.V1b, self.V1e)
        self.pristine = {k: getattr(self, k).to(DEV) for k in ("Kb", "Ke", "Vb", "Ve", "V1b", "V1e")}
        self.dev = {k: t.clone() for k, t in self.pristine.items()}

    def place_hot(self, hot):
        """huge_*: the one large key at `hot` (raw k, and slot `hot` of every copy of the cache); returns what undoes it."""
        saved = (hot, self.kr[:, :, hot].clone(), self.krot[:, :, hot].clone())
        self.kr[:, :, hot] = A.huge_key(self.kr, self.rows, seed_of(self.name), self.rope, hot)
        self.krot[:, :, hot] = A.rope32(self.kr[:, :, hot:hot + 1], self.rope, hot)[:, :, 0]
        self._sync_slot(hot)
        return saved

    def undo_hot(self, saved):
        hot, self.kr[:, :, hot], self.krot[:, :, hot] = saved
        self._sync_slot(hot)

    def _sync_slot(self, hot):
        b, e = F.quantise(self.krot[:, :, hot])
        self.Kb[:, :, hot], self.Ke[:, :, hot], self.K64[:, :, hot] = b, e, F.widen(b, e)
        for d in (self.pristine, self.dev):
            d["Kb"][:, :, hot], d["Ke"][:, :, hot] = b.to(DEV), e.to(DEV)

    def chunk(self, rows, p0, n):
        sl = slice(p0, p0 + n)
        return self.qr[:rows, :, sl], self.kr[:rows, :, sl], self.v[:rows, :, sl]

    def arrays(self, v_ones):
        d = self.dev
        return (d["Kb"], d["Ke"], d["V1b"], d["V1e"]) if v_ones else (d["Kb"], d["Ke"], d["Vb"], d["Ve"])

    def poison(self, rows, p0, n, v_ones):
        kb, ke, vb, ve = self.arrays(v_ones)
        kb[:rows, :, p0:p0 + n], vb[:rows, :, p0:p0 + n] = POISON_B, POISON_B
        ke[:rows, :, p0:p0 + n], ve[:rows, :, p0:p0 + n] = POISON_E, POISON_E

    def check_after(self, rows, p0, n, v_ones, y64, m64, counts):
        """New v bytes / exponents bit for bit the restatement's; new k under the k rule (kv_f8s_reference.check_stored_k); then the
        slots are restored and every byte of the four arrays equals its pre-call copy.  Returns the stored k and v of the chunk (CPU)."""
        sl = slice(p0, p0 + n)
        kb, ke, vb, ve = (t[:rows, :, sl].cpu() for t in self.arrays(v_ones))
        wb, we = F.quantise(torch.ones_like(self.v[:rows, :, sl]) if v_ones else self.v[:rows, :, sl])
        assert torch.equal(vb, wb) and torch.equal(ve, we), f"chunk ({p0}, {n}) rows {rows}: new v bytes / exponents are not the restatement's"
        c = F.check_stored_k(kb, ke, y64, m64)
        for i in range(4):
            counts[i] += c[i]
        names = ("Kb", "Ke", "V1b", "V1e") if v_ones else ("Kb", "Ke", "Vb", "Ve")
        for nm in names:
            self.dev[nm][:rows, :, sl] = self.pristine[nm][:rows, :, sl]
            assert torch.equal(self.dev[nm], self.pristine[nm]), f"chunk ({p0}, {n}) rows {rows}: {nm} changed outside the new positions"
        return (kb, ke), (vb, ve)


_SEQS = {}


def seq_for(name):
    if name not in _SEQS:
        _SEQS.clear()
        _SEQS[name] = Seq(name)
    return _SEQS[name]


def qkv_rows(q, k, v):
    R = q.shape[0]
    return torch.cat([x[:, :, 0].reshape(R, D) for x in (q, k, v)], dim=-1)


def assert_caps(counts, where):
    print(f"{where}: {counts[0]} of {counts[1]} k vectors near a power of two, {counts[2]} of {counts[3]} k elements at a rounding boundary")
    assert counts[0] < 1e-3 * max(1, counts[1]) and counts[2] < 1e-3 * max(1, counts[3]), f"{where}: boundary sets reach the 0.1 % cap: {counts}"


def reference(seq, q, k, v, p0, stored_k, stored_v, v_ones):
    """chunk_reference on the widened cache: the chunk's k and v as the cache holds them after the call (fp32 holds byte x 2^e exactly)."""
    return A.chunk_reference(q, k, F.widen(*stored_v).float(), seq.rope, seq.K64[:q.shape[0]], (seq.V164 if v_ones else seq.V64)[:q.shape[0]],
                             p0, 0, k_stored=F.widen(*stored_k).float())


def run_step(seq, rows, pos, v_ones=False, arrays=None):
    q, k, v = seq.chunk(rows, pos, 1)
    kb, ke, vb, ve = arrays or seq.arrays(v_ones)
    qp = ops.pack_rows(qkv_rows(q, k, torch.ones_like(v) if v_ones else v).to(DEV))
    o, _ = ops.attention_step_kv(qp, seq.rope_d, kb, vb, rows, H, HD, pos, kv_dtype=3, kscale=ke, vscale=ve)
    return ops.unpack_rows(o, rows, D).cpu()


def run_prefill(seq, rows, p0, n, v_ones=False, arrays=None):
    q, k, v = seq.chunk(rows, p0, n)
    kb, ke, vb, ve = arrays or seq.arrays(v_ones)
    r16 = (rows + 15) // 16 * 16
    mat = torch.zeros(n, r16, 3 * D)
    mat[:, :rows] = torch.cat([x.permute(2, 0, 1, 3).reshape(n, rows, D) for x in (q, k, torch.ones_like(v) if v_ones else v)], dim=-1)
    attn = torch.full((n * r16 * D,), float("nan"), device=DEV)
    ops.attention_prefill(ops.pack_rows(mat.view(n * r16, 3 * D).to(DEV)), seq.rope_d, kb, vb, attn, None, rows, H, HD, p0, n, kv_dtype=3,
                          kscale=ke, vscale=ve)
    return ops.unpack_rows(attn, n * r16, D).cpu().view(n, r16, D)[:, :rows].transpose(0, 1)      # (rows, n, D)


# ------------------------------------------------------------------------------------------ 1 + 2: bits and arithmetic
@pytest.mark.parametrize("name", A.FAMILIES)
def test_step_stored_bits_and_arithmetic(name):
    """Every position of POS x rows 1 / 5 / 16 / 32: poisoned slots, the stored bits (the k rule's exclusions counted and
    capped), every other byte unchanged, and the output (and the same with every v = 1) within the bar on the widened cache."""
    seq = seq_for(name)
    counts = [0, 0, 0, 0]
    for pos in POS:
        hot = hot_for(name, pos)
        saved = seq.place_hot(hot) if hot is not None else None
        for rows in ROWS:
            q, k, v = seq.chunk(rows, pos, 1)
            y64, m64 = A.rope64(k, seq.rope, pos)
            for v_ones in (False, True):
                seq.poison(rows, pos, 1, v_ones)
                got = run_step(seq, rows, pos, v_ones)
                sk, sv = seq.check_after(rows, pos, 1, v_ones, y64, m64, counts)
                ref = reference(seq, q, k, v, pos, sk, sv, v_ones)
                what = "ones" if v_ones else "out"
                judge("step256", name, got[:, None], ref[what + "64"], ref[what + "32"], what, f"rows {rows} pos {pos}")
        if saved is not None:
            seq.undo_hot(saved)
    assert_caps(counts, f"step256 f8s {name}")


@pytest.mark.parametrize("name", A.FAMILIES)
def test_prefill_stored_bits_arithmetic_and_step_consistency(name):
    """Every chunk of PREFILL (rows 16 / 32 / 1 / 5 in turn: 32 rows on the largest chunk): as above for rope_append_kernel<96, 3> +
    attention_prefill_kernel<96, 3>; then one decode step at the chunk's last position on the same inputs must store the SAME bits (k and v, bytes and exponents)."""
    seq = seq_for(name)
    counts = [0, 0, 0, 0]
    for i, (p0, n) in enumerate(PREFILL):
        rows = ROWS[(i + 2) % 4]             # (0, 1) -> 16, (0, 17) -> 32, (0, 64) -> 1, (40, 20) -> 5, (63, 2) -> 16, (100, 130) -> 32
        last = p0 + n - 1
        hot = None if not name.startswith("huge") else (last // 64 * 64 - (i % 2) if last >= 64 else (last if i % 2 else 0))
        saved = seq.place_hot(hot) if hot is not None else None
        q, k, v = seq.chunk(rows, p0, n)
        y64, m64 = A.rope64(k, seq.rope, p0)
        for v_ones in (False, True):
            seq.poison(rows, p0, n, v_ones)
            got = run_prefill(seq, rows, p0, n, v_ones)
            pre = [t[:rows, :, last].clone() for t in seq.arrays(v_ones)]
            seq.poison(rows, last, 1, v_ones)
            run_step(seq, rows, last, v_ones)
            for a, t in zip(pre, seq.arrays(v_ones)):
                assert torch.equal(a, t[:rows, :, last]), f"chunk ({p0}, {n}) rows {rows}: step and prefill store different bits at position {last}"
            sk, sv = seq.check_after(rows, p0, n, v_ones, y64, m64, counts)
            ref = reference(seq, q, k, v, p0, sk, sv, v_ones)
            what = "ones" if v_ones else "out"
            judge("prefill_mfma", name, got, ref[what + "64"], ref[what + "32"], what, f"rows {rows} chunk ({p0}, {n})")
        if saved is not None:
            seq.undo_hot(saved)
    assert_caps(counts, f"prefill f8s {name}")


# --------------------------------------------------------------------------------------------------- 3: scale invariance
def test_value_scale_invariance_is_exact():
    """wide, the same K, V x 2^j: the fp32 output of the step and of the prefill is torch.equal to 2^j x the j = 0 output, the V bytes
    are identical and the V exponents shifted by j."""
    rows, pos, chunk = 5, 193, (40, 20)
    base = {}
    for j in (0, -20, 12):
        seq = Seq("wide", rows=rows, vscale=j)
        arrays = seq.arrays(False)
        o_s = run_step(seq, rows, pos, arrays=arrays)
        o_p = run_prefill(seq, rows, *chunk, arrays=arrays)
        sl = slice(chunk[0], chunk[0] + chunk[1])
        vb = torch.cat([arrays[2][:, :, sl], arrays[2][:, :, pos:pos + 1]], 2).cpu()
        ve = torch.cat([arrays[3][:, :, sl], arrays[3][:, :, pos:pos + 1]], 2).cpu().long()
        assert bool(torch.isfinite(o_s).all()) and bool(torch.isfinite(o_p).all())
        if j == 0:
            base = dict(o_s=o_s, o_p=o_p, vb=vb, ve=ve)
            continue
        assert torch.equal(o_s, base["o_s"] * 2.0 ** j), f"step: out(V 2^{j}) is not 2^{j} out(V)"
        assert torch.equal(o_p, base["o_p"] * 2.0 ** j), f"prefill: out(V 2^{j}) is not 2^{j} out(V)"
        assert torch.equal(vb, base["vb"]) and torch.equal(ve, base["ve"] + j), f"j = {j}: V bytes differ or exponents are not shifted by j"


# ----------------------------------------------------------------------------------------------- 4: quantisation bound
def test_quantisation_bound_with_uniform_scores():
    """Every key of a (row, head) is the same vector (values e4m3 holds exactly, so the new key's last-bit rotation error cannot move
    a byte): the scores are uniform whatever the K rounding does, and the output error is the mean of the V quantisation errors:
    |got - ref64(unquantised)| <= (2^-4 + 1e-5) mean_i |v_ic| + 2^-10 / 224 mean_i amax_i per channel.  "f8" on the same inputs: recorded."""
    rows, pos = 5, 200
    rope = rope_table(T, HD)
    g = torch.Generator().manual_seed(4242)
    k0 = (torch.randint(1, 5, (rows, H, 1, HD), generator=g).float() * 0.5) * (torch.randint(0, 2, (rows, H, 1, HD), generator=g).float() * 2 - 1)
    krot = k0.expand(rows, H, T, HD).contiguous()
    v = A.family("wide", rows, T, seed_of("wide"), rope)[2] * 2.0 ** -12
    seq = Seq("flat", rows=rows, v=v, krot=krot)
    seq.qr = seq.qr * 0.05
    seq.kr = A.unrope(krot, rope, 0)
    got = run_step(seq, rows, pos)
    q64, _ = A.rope64(seq.qr[:, :, pos:pos + 1], rope, pos)
    ref, _ = A.attention64(q64, krot[:, :, :pos + 1], v[:, :, :pos + 1], pos)
    va = v[:, :, :pos + 1].double()
    bound = (2.0 ** -4 + 1e-5) * va.abs().mean(2) + 2.0 ** -10 / 224.0 * va.abs().amax(-1).mean(2)[..., None]      # (rows, H, hd)
    err = (got.double() - ref[:, 0]).abs().view(rows, H, HD)
    # the unscaled e4m3 cache on the same inputs (recorded, not asserted)
    k8, v8 = A.narrow(krot, 2).to(DEV), A.narrow(v, 2).to(DEV)
    o8, _ = ops.attention_step_ex(ops.pack_rows(qkv_rows(*seq.chunk(rows, pos, 1)).to(DEV)), seq.rope_d, k8, v8, rows, H, HD, pos, kv_dtype=2)
    err8 = (ops.unpack_rows(o8, rows, D).cpu().double() - ref[:, 0]).abs().view(rows, H, HD)
    print(f"uniform scores, v = wide x 2^-12: worst err / bound f8s {float((err / bound).max()):.3f}, f8 {float((err8 / bound).max()):.3f}; "
          f"rel err f8s {A.rel_err(got, ref[:, 0]):.3e}, f8 {float(err8.max() / ref.abs().max()):.3e}")
    assert bool((err <= bound).all()), f"worst err / bound {float((err / bound).max()):.3f}"


# ------------------------------------------------------------------------------------------------------- 5: non-finite
def test_non_finite_vectors_stay_non_finite_and_stay_put():
    """One inf in a cached v and one NaN in a cached k: the output of exactly those (row, head) pairs is non-finite, in the step and in
    the prefill; every other pair is finite and within the bar."""
    rows, pos, chunk = 5, 100, (40, 20)
    seq = Seq("flat", rows=rows)
    seq.v[1, 3, 10, 5] = float("inf")
    seq.krot[2, 7, 20, 9] = float("nan")
    seq.build()
    assert int(seq.Ve[1, 3, 10]) == 0xFF and int(seq.Ke[2, 7, 20]) == 0xFF
    keep = torch.ones(rows, H, dtype=torch.bool)
    keep[1, 3] = keep[2, 7] = False
    clean = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)
    seq.K64, seq.V64 = clean(seq.K64), clean(seq.V64)          # the reference of the pairs that are compared does not read them
    for kernel, p0, n, run in (("step256", pos, 1, run_step), ("prefill_mfma", *chunk, run_prefill)):
        got = run(seq, rows, p0) if n == 1 else run(seq, rows, p0, n)
        got = got[:, None] if n == 1 else got
        sl = slice(p0, p0 + n)
        arrays = [t[:rows, :, sl].cpu() for t in seq.arrays(False)]
        q, k, v = seq.chunk(rows, p0, n)
        ref = reference(seq, q, k, clean(v), p0, (arrays[0], arrays[1]), (arrays[2], arrays[3]), False)
        g4 = got.view(rows, n, H, HD)
        for r, h in ((1, 3), (2, 7)):
            assert not bool(torch.isfinite(g4[r, :, h]).any()), f"{kernel}: (row {r}, head {h}) read a non-finite vector and returned finite numbers"
        judge(kernel, "flat", got, ref["out64"], ref["out32"], "out", f"non-finite neighbours, chunk ({p0}, {n})", keep=keep)


# --------------------------------------------------------------------------------------------------------- 6: refusals
def test_refusals():
    rope = rope_table(1024, HD).to(DEV)
    rows = 2
    qp = ops.pack_rows(torch.randn(rows, 3 * D, device=DEV))
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)
    untouched = lambda *ts: not any(bool(t.ne(0).any()) for t in ts)
    for max_len, n_split in [(257, 1), (1024, 1), (256, 2)]:
        kc, vc, ks, vs = u8(rows, H, max_len, HD), u8(rows, H, max_len, HD), u8(rows, H, max_len), u8(rows, H, max_len)
        out = torch.full((16 * D,), float("nan"), device=DEV)
        with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE"):
            ops.attention_step_kv(qp, rope, kc, vc, rows, H, HD, 5, kv_dtype=3, kscale=ks, vscale=vs, n_split=n_split, out=out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and untouched(kc, vc, ks, vs)
        if n_split == 1:
            qkv = ops.pack_rows(torch.randn(4 * 16, 3 * D, device=DEV))
            before, attn = qkv.clone(), torch.full((4 * 16 * D,), float("nan"), device=DEV)
            with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE"):
                ops.attention_prefill(qkv, rope, kc, vc, attn, None, rows, H, HD, 0, 4, kv_dtype=3, kscale=ks, vscale=vs)
            torch.cuda.synchronize()
            assert bool(torch.isnan(attn).all()) and torch.equal(qkv, before) and untouched(kc, vc, ks, vs)
    kc, vc, ks = u8(rows, H, 256, HD), u8(rows, H, 256, HD), u8(rows, H, 256)
    out = torch.full((16 * D,), float("nan"), device=DEV)
    qkv = ops.pack_rows(torch.randn(4 * 16, 3 * D, device=DEV))
    attn = torch.full((4 * 16 * D,), float("nan"), device=DEV)
    for kw in (dict(kscale=None, vscale=ks), dict(kscale=ks, vscale=None), dict()):
        with pytest.raises(L.VauraHipError, match="VAURA_ERR_ARG"):
            ops.attention_step_kv(qp, rope, kc, vc, rows, H, HD, 5, kv_dtype=3, out=out, **kw)
        with pytest.raises(L.VauraHipError, match="VAURA_ERR_ARG"):
            ops.attention_prefill(qkv, rope, kc, vc, attn, None, rows, H, HD, 0, 4, kv_dtype=3, **kw)
    with pytest.raises(L.VauraHipError, match="VAURA_ERR_ARG"):
        ops.attention_step_ex(qp, rope, kc, vc, rows, H, HD, 5, kv_dtype=3, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(attn).all()) and untouched(kc, vc, ks)


# ------------------------------------------------------------------------------------------------------- 7 + 8: engine
def test_engine_generates_on_the_scaled_cache(tiny_sampler_sd, golden):
    g = golden("tiny_model.npz")
    feats = synth.video_features(2, seed=int(g["feat_seed"])).to(DEV)
    e = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype="h2", kv_dtype="f8s")
    Tn, S = 20, 29
    for kw in (dict(cfg_scale=6.0), dict(cfg_scale=6.0, use_sampling=True, top_k=250, seed=7)):
        a = e.generate_codes(feats, Tn, **kw).cpu()
        e.check_status()
        assert int(e.state[4].item()) == 0
        assert e.kcache.dtype == torch.uint8 and e.vcache.dtype == torch.uint8 and e.rows == 4 and e.dec.kv_dtype == 3
        assert a.shape == (2, 9, Tn) and int(a.min()) >= 0 and int(a.max()) < 1024
        for sc, cache in ((e.kscale, e.kcache), (e.vscale, e.vcache)):
            written = sc.ne(0)
            assert bool(written[..., :S - 1].all()) and not bool(written[..., S - 1:].any()), "scale bytes are non-zero exactly at the written positions"
            assert not bool(cache[:, :, :, S - 1:].ne(0).any()) and not bool(sc.eq(0xFF).any())
        b = e.generate_codes(feats, Tn, **kw).cpu()
        e.check_status()
        assert torch.equal(a, b), "a second identical call returned other tokens"


def test_rescaled_checkpoint_loss(tiny_sampler_sd, golden):
    """Checkpoint A' = A with every wv row x 2^-8 and every wo column x 2^8 (the same function; v 256 times smaller).  The storage is
    scale-free, so |L_f8s(A') - L32(A')| <= 2 |L_f8s(A) - L32(A)| + 1e-5 L32: the two errors differ only through the fp16 activation
    planes (factor 2), and 1e-5 is the project's loss tolerance.  "f8" on A' is recorded beside it."""
    g = golden("eval_tiny.npz")
    codes = torch.from_numpy(g["delayed_codes"].astype(np.int64)).to(DEV)
    feats = synth.video_features(codes.shape[0], seed=int(g["feat_seed"])).to(DEV)
    cfg = synth.tiny_sampler(2)
    Dm = cfg.d_model
    sd2 = dict(tiny_sampler_sd)
    for l in range(cfg.num_layers):
        wqkv = tiny_sampler_sd[f"layers.{l}.attention.wqkv.weight"].clone()
        wqkv[2 * Dm:] *= 2.0 ** -8
        sd2[f"layers.{l}.attention.wqkv.weight"] = wqkv
        sd2[f"layers.{l}.attention.wo.weight"] = tiny_sampler_sd[f"layers.{l}.attention.wo.weight"] * 2.0 ** 8

    def loss(sd, kv):
        e = DecoderEngine(cfg, sd, DEV, wdtype="h2", kv_dtype=kv)
        r = e.score(codes, feats)
        e.check_status()
        return float(r["loss"])
    L32a, Lsa = loss(tiny_sampler_sd, "f32"), loss(tiny_sampler_sd, "f8s")
    L32b, Lsb, L8b = loss(sd2, "f32"), loss(sd2, "f8s"), loss(sd2, "f8")
    lines = ["# teacher-forced loss (engine.score, eval_tiny delayed codes, h2 weights) on checkpoint A and on A' = A with wv x 2^-8, wo x 2^8",
             f"L32(A)  {L32a:.7f}   L_f8s(A)  {Lsa:.7f}   |diff| {abs(Lsa - L32a):.3e}",
             f"L32(A') {L32b:.7f}   L_f8s(A') {Lsb:.7f}   |diff| {abs(Lsb - L32b):.3e}",
             f"L_f8(A') {L8b:.7f}   |L_f8(A') - L32(A')| {abs(L8b - L32b):.3e}   (unscaled e4m3: recorded, not asserted)"]
    print("\n".join(lines))
    if _out_dir():
        with open(os.path.join(_out_dir(), "kv_f8s_loss.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    assert abs(Lsb - L32b) <= 2 * abs(Lsa - L32a) + 1e-5 * L32b, lines
