"""The host-side dispatch of csrc/step.hip and the kernels that serve several entry points through nullable arrays: the 24 instances of
sample_kernel reached from va_launch_sample's one composed pack, sequence_logprob_kernel (scalar / per-clip first frame / per-clip
length), pattern_build_kernel and pattern_revert_kernel<int32 | float> (with and without lengths).

Everything is bit equality.  The sampler is compared with itself (a wrong instance or a swapped pack member changes the result); the
means with tests/logprob_reference.py; the pattern ops with the index maps of vaura_amd.patterns.Pattern on the CPU, which
tests/test_patterns_delays.py pins against the reference's own values.

Shapes: B = 3, K = 4, V = 1024, T = 6 (sampler, patterns) and T = 70 (means: the smallest length at which a lane adds a second frame —
a loop bound that is wrong by a stride cannot be seen below it), delays (0, 1, 2, 3) and (0, 0, 0, 0)."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprob_reference as R  # noqa: E402
import test_gpu_logprobs as G  # noqa: E402  (record / struct helpers)
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd.patterns import Pattern  # noqa: E402

DEV = "cuda:0"
B, K, V, T = 3, 4, 1024, 6
P = G.P


def stream():
    return L.current_stream(torch.device(DEV))


def i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module", params=[(0, 1, 2, 3), (0, 0, 0, 0)], ids=["default", "parallel"])
def delays(request):
    return list(request.param)


# ------------------------------------------------------------------------------------------------ CPU restatement of the pattern ops
def ref_build(codes: torch.Tensor, delays, special: int, lengths=None) -> torch.Tensor:
    """codes (B, K, T) on the CPU -> (B, K, T + max(d) + 1): Pattern._build_indexes, clip b with its own T_b where lengths are given"""
    Bn, Kn, Tn = codes.shape
    pat = Pattern(delays, Tn)
    flat = torch.cat([codes.reshape(Bn, -1), torch.full((Bn, 1), special, dtype=codes.dtype)], dim=1)
    out = torch.empty(Bn, Kn, pat.seq_steps, dtype=codes.dtype)
    for b in range(Bn):
        idx, mask = pat._build_indexes(Tn, "cpu")
        if lengths is not None:      # t < T_b: the stride of the rows stays T
            idx = torch.where(mask & (pat._build_indexes(lengths[b], "cpu")[1]), idx, torch.full_like(idx, Kn * Tn))
        out[b] = flat[b, idx.view(-1)].view(Kn, -1)
    return out


def ref_revert(seq: torch.Tensor, delays, Tn: int, fill, pad=None, lengths=None) -> torch.Tensor:
    """seq (B, K, S) on the CPU, S <= T + max(d) + 1 -> (B, K, T): Pattern._revert_indexes, `pad` from T_b on where lengths are given"""
    Bn, Kn, S = seq.shape
    idx, _ = Pattern(delays, Tn)._revert_indexes(S, "cpu")
    flat = torch.cat([seq.reshape(Bn, -1), torch.full((Bn, 1), fill, dtype=seq.dtype)], dim=1)
    out = flat[:, idx.view(-1)].view(Bn, Kn, Tn).clone()
    for b, Tb in enumerate(lengths or []):
        out[b, :, Tb:] = pad
    return out


# ------------------------------------------------------------------------------------------------------------------------ 1. sampler
POS, STEP = 3, 2          # delays (0, 1, 2, 3): slot POS + 1 holds timesteps 3, 2, 1, 0 — free and valid for every clip and codebook
SET = P(True, 0.9, 50, cfg_scale=2.0)


def sample_seq(delays, logits, *, records, report, lengths, starts, Tn=T, pos=POS, step=STEP):
    """one launch on a fresh sequence -> (seq, state, the three report buffers), on the CPU; report: 0 none, 1 lp_seq, 2 all three"""
    lib, S = L.lib(), T + max(delays) + 1
    seq = torch.full((B, K, S), -1, dtype=torch.int32, device=DEV)
    seq[:, :, :pos + 1] = 5
    bufs = [torch.full((B, K, S), 7.0, device=DEV) for _ in range(3)]
    state = torch.zeros(8, dtype=torch.int32, device=DEV)
    state[0], state[2] = pos, step
    rec = G.records([SET] * B) if records else None
    clip_T, clip_n = (i32(v) if v else None for v in (lengths, starts))      # (held until the launch has run)
    sp = G.sampling(SET)
    head = (L.ptr(logits), B, K, V, C.byref(sp), L.ptr(rec), None, L.ptr(seq), Tn, S, L.ptr(state), L.delays_host(delays),
            L.ptr(clip_T))
    tail = (*(L.ptr(x) if j < (0, 1, 3)[report] else None for j, x in enumerate(bufs)), stream())
    if starts is None:
        assert lib.vaura_sample_seq(*head, *tail) == 0
    else:
        assert lib.vaura_sample_seq_starts(*head, L.ptr(clip_n), *tail) == 0
    torch.cuda.synchronize()
    return seq.cpu(), state.cpu(), [x.cpu() for x in bufs]


@pytest.fixture(scope="module")
def logits():
    return (torch.randn(2 * B, K, V, generator=torch.Generator().manual_seed(21)) * 3.0).to(DEV)


def test_every_sampler_instance_is_wired_to_its_pack(delays, logits):
    """{scalar, records} x {no report, lp_seq, lp_seq + cond_seq + null_seq} x {no lengths, clip_timesteps} x {vaura_sample_seq,
    vaura_sample_seq_starts}: the 24 instances, the optional arrays neutral (records = the scalars, T_b = T, n_b = state[0] - state[2]).
    Every one returns the plain instance's sequence and state, and the report buffers of the plain instance of its report mode."""
    plain = {r: sample_seq(delays, logits, records=False, report=r, lengths=None, starts=None) for r in (0, 1, 2)}
    seq0, state0, _ = plain[0]
    drawn = seq0[:, :, POS + 1]
    assert bool(((drawn >= 0) & (drawn < V)).all()) and int(state0[0]) == POS + 1 and int(state0[2]) == STEP + 1
    assert len({int(x) for x in drawn.flatten()}) > 1
    for r in (1, 2):       # a report is written exactly where a token was sampled, and only into the buffers that were passed
        for j, x in enumerate(plain[r][2]):
            assert bool((x[:, :, POS + 1] != 7.0).all()) == (j < (0, 1, 3)[r]) and bool((x[:, :, :POS + 1] == 7.0).all())
    for records, report, lengths, starts in itertools.product((False, True), (0, 1, 2), (None, [T] * B), (None, [POS - STEP] * B)):
        seq, state, bufs = sample_seq(delays, logits, records=records, report=report, lengths=lengths, starts=starts)
        what = (records, report, lengths, starts)
        assert torch.equal(seq, seq0) and torch.equal(state, state0), what
        for x, w in zip(bufs, plain[report][2]):
            assert torch.equal(bits(x), bits(w)), what


def test_sampler_pack_members_are_read(delays, logits):
    """the fullest instance (records, all three reports, lengths, starts) with lengths (2, 6, 4) and starts (0, 2, 1) at position 2,
    where the slots lie on both sides of a clip's end: clip b is the scalar call with T = T_b on a state whose step is position - n_b"""
    Tl, n, pos = [2, 6, 4], [0, 2, 1], 2
    seq, _, bufs = sample_seq(delays, logits, records=True, report=2, lengths=Tl, starts=n, pos=pos, step=pos)
    seen = set()
    for b in range(B):
        wseq, _, wbufs = sample_seq(delays, logits, records=False, report=2, lengths=None, starts=None, Tn=Tl[b], pos=pos, step=pos - n[b])
        assert torch.equal(seq[b], wseq[b]), b
        for x, w in zip(bufs, wbufs):
            assert torch.equal(bits(x[b]), bits(w[b])), b
        seen |= {"special" if int(v) == V else "token" for v in seq[b, :, pos + 1]}
    assert seen == {"special", "token"}          # the shapes do put slots on both sides of a clip's end


# -------------------------------------------------------------------------------------------------------------------------- 2. means
TM = 70
T0S, TBS = [0, 3, 69], [70, 65, 5]


@pytest.fixture(scope="module")
def lp_layout(delays):
    """log-probabilities in the layout of seq, one NaN: clip 1, codebook 2, frame 66 — read by the calls with T = 70, behind the end
    of the calls with T_1 = 65"""
    S = TM + max(delays) + 1
    lp = -torch.rand(B, K, S, generator=torch.Generator().manual_seed(4))
    lp[1, 2, 66 + 1 + delays[2]] = float("nan")
    frames = R.revert(lp.numpy(), delays, TM)
    return lp.to(DEV), frames


def same_f32(got: torch.Tensor, want: np.ndarray) -> bool:
    """the same bits, a NaN where and only where the restatement has one"""
    g, w = got.cpu().numpy(), np.asarray(want, dtype=np.float32)
    nan = np.isnan(w)
    return bool(np.array_equal(np.isnan(g), nan)) and bool(np.array_equal(g[~nan].view(np.int32), w[~nan].view(np.int32)))


def test_sequence_means_across_the_lane_stride(delays, lp_layout):
    """the three entry points against logprob_reference.sequence_logprob of clip b's frames [:, :, :T_b] with t0 = t0_b: first frames
    (0, 3, 69) and lengths (70, 65, 5) separately, and together — in the order (69, 3, 0), since a clip needs a frame behind its first
    one; the order as listed, clip 2 with t0 = 69 and T = 5, is refused"""
    lib = L.lib()
    lp, frames = lp_layout
    S, dl = TM + max(delays) + 1, L.delays_host(delays)
    t0s_d, t0s_rev, tbs_d = i32(T0S), i32(T0S[::-1]), i32(TBS)      # (held: an argument built in place would be freed before the launch)

    def check(fn, args, t0s, Tbs):
        pcb, clip = torch.zeros(B, K, device=DEV), torch.zeros(B, device=DEV)
        assert getattr(lib, fn)(L.ptr(lp), S, dl, B, K, TM, *args, L.ptr(pcb), L.ptr(clip), stream()) == 0, (fn, t0s, Tbs)
        torch.cuda.synchronize()
        for b in range(B):
            wp, wc = R.sequence_logprob(frames[b:b + 1, :, :Tbs[b]], t0s[b])
            assert same_f32(pcb[b], wp[0]) and same_f32(clip[b:b + 1], wc), (fn, t0s, Tbs, b)
        return clip.cpu()

    for t0 in T0S:
        clip = check("vaura_sequence_logprob", (t0,), [t0] * B, [TM] * B)
        assert [bool(x) for x in torch.isnan(clip)] == [False, t0 <= 66, False]
    for t0 in (0, 3):
        clip = check("vaura_sequence_logprob_clips", (t0, L.ptr(tbs_d)), [t0] * B, TBS)
        assert not bool(torch.isnan(clip).any())
    check("vaura_sequence_logprob_starts", (L.ptr(t0s_d), None), T0S, [TM] * B)
    check("vaura_sequence_logprob_starts", (L.ptr(t0s_rev), L.ptr(tbs_d)), T0S[::-1], TBS)
    pcb, clip = torch.full((B, K), 7.0, device=DEV), torch.full((B,), 7.0, device=DEV)
    assert lib.vaura_sequence_logprob_starts(L.ptr(lp), S, dl, B, K, TM, L.ptr(t0s_d), L.ptr(tbs_d), L.ptr(pcb), L.ptr(clip), stream()) == -1
    assert lib.vaura_sequence_logprob_clips(L.ptr(lp), S, dl, B, K, TM, 5, L.ptr(tbs_d), L.ptr(pcb), L.ptr(clip), stream()) == -1
    assert lib.vaura_sequence_logprob(L.ptr(lp), S, dl, B, K, TM, TM, L.ptr(pcb), L.ptr(clip), stream()) == -1
    torch.cuda.synchronize()
    assert bool((pcb == 7.0).all()) and bool((clip == 7.0).all())


# ----------------------------------------------------------------------------------------------------------------------- 3. patterns
TL = [1, T, 3]


def test_pattern_build_and_revert(delays):
    """build, and revert of tokens and fp32 values, with and without lengths (1, T, 3), revert also from a sequence cut short of
    T + max(d) + 1 (`fill`); then every refusal of include/vaura_hip.h: a negative code and nothing written"""
    lib, span = L.lib(), max(delays) + 1
    S, dl = T + span, L.delays_host(delays)
    unit = delays == list(range(K))
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, V, (B, K, T), generator=g, dtype=torch.int32)
    codes[:, :, 2:] = torch.where(torch.rand(B, K, T - 2, generator=g) < 0.5, torch.tensor(-1, dtype=torch.int32), codes[:, :, 2:])
    codes_d, guard = codes.to(DEV), -7
    # (held: an argument built in place would be freed before the launch)
    tl, tl_lo, tl_hi, tl_lo2, tl_hi2 = i32(TL), i32([0, T, 3]), i32([1, T + 1, 3]), i32([1, T, 0]), i32([T + 1, T, 3])

    def build(fn, *args):
        seq = torch.full((B, K, S), guard, dtype=torch.int32, device=DEV)
        rc = getattr(lib, fn)(L.ptr(codes_d), L.ptr(seq), B, K, T, *args, stream())
        torch.cuda.synchronize()
        return rc, seq.cpu()

    want = ref_build(codes, delays, V)
    rc, seq = build("vaura_pattern_build_delays", S, V, dl)
    assert rc == 0 and torch.equal(seq, want)
    if unit:
        rc, seq = build("vaura_pattern_build", V)
        assert rc == 0 and torch.equal(seq, want)
    rc, seq_l = build("vaura_pattern_build_clips", S, V, dl, L.ptr(tl))
    assert rc == 0 and torch.equal(seq_l, ref_build(codes, delays, V, TL))
    assert not torch.equal(seq_l, want)
    # refusals of build: no delays where they are required, unsorted / negative delays, S != T + max(d) + 1, no lengths, a length out of 1 .. T
    worse = L.delays_host([0, 2, 1, 3])
    for fn, args, code in (("vaura_pattern_build_delays", (S, V, None), -1), ("vaura_pattern_build_delays", (S, V, worse), -1),
                           ("vaura_pattern_build_delays", (S, V, L.delays_host([-1, 0, 1, 2])), -1),
                           ("vaura_pattern_build_delays", (S - 1, V, dl), -2), ("vaura_pattern_build_clips", (S + 1, V, dl, L.ptr(tl)), -2),
                           ("vaura_pattern_build_clips", (S, V, dl, None), -1), ("vaura_pattern_build_clips", (S, V, dl, L.ptr(tl_lo)), -1),
                           ("vaura_pattern_build_clips", (S, V, dl, L.ptr(tl_hi)), -1)):
        rc, seq = build(fn, *args)
        assert rc == code and bool((seq == guard).all()), (fn, args)

    seqf = torch.randn(B, K, S, generator=g)
    for src, fill, pad, sfx in ((want, -1, V, ""), (seqf, 0.5, -2.5, "_f32")):
        for Sc in (S, S - 2):                     # S - 2: the last frames of the last codebook have no slot
            cut = src[:, :, :Sc].contiguous().to(DEV)

            def revert(fn, *args, Sa=Sc):
                out = torch.full((B, K, T), guard, dtype=src.dtype, device=DEV)
                rc = getattr(lib, fn)(L.ptr(cut), L.ptr(out), B, K, T, Sa, *args, stream())
                torch.cuda.synchronize()
                return rc, out.cpu()

            w = ref_revert(src[:, :, :Sc], delays, T, fill)
            if sfx:
                assert bool((w == fill).any()) == (Sc < S)
            rc, out = revert("vaura_pattern_revert_delays" + sfx, fill, dl)
            assert rc == 0 and torch.equal(bits(out), bits(w)), (sfx, Sc)
            if unit:                              # the forms without an array of delays
                rc, out = revert("vaura_pattern_revert_delays_f32", fill, None) if sfx else revert("vaura_pattern_revert", fill)
                assert rc == 0 and torch.equal(bits(out), bits(w)), (sfx, Sc)
            rc, out = revert("vaura_pattern_revert_clips" + sfx, fill, pad, dl, L.ptr(tl))
            assert rc == 0 and torch.equal(bits(out), bits(ref_revert(src[:, :, :Sc], delays, T, fill, pad, TL))), (sfx, Sc)
            for fn, args, kw, code in (("vaura_pattern_revert_delays" + sfx, (fill, worse), {}, -1),
                                       ("vaura_pattern_revert_delays" + sfx, (fill, dl), {"Sa": S + 1}, -2),
                                       ("vaura_pattern_revert_clips" + sfx, (fill, pad, dl, None), {}, -1),
                                       ("vaura_pattern_revert_clips" + sfx, (fill, pad, dl, L.ptr(tl_lo2)), {}, -1),
                                       ("vaura_pattern_revert_clips" + sfx, (fill, pad, dl, L.ptr(tl_hi2)), {}, -1)):
                rc, out = revert(fn, *args, **kw)
                assert rc == code and bool((out == guard).all()), (fn, args, kw)
            if not sfx:
                rc, out = revert("vaura_pattern_revert_delays", fill, None)
                assert rc == -1 and bool((out == guard).all())
