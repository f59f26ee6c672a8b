"""Per-clip lengths in one batched call, on the device: vaura_decoder_ext2.clip_timesteps / clip_cond_tokens, the per-clip forms of the
step's small kernels (csrc/step.hip: sample_kernel<.., SampleLengths>, embed_clips_kernel, pattern_build_kernel,
pattern_revert_kernel, sequence_logprob_kernel with clip_T), DecoderEngine.generate_codes(max_new_tokens=[..], video_lengths=[..]) and
VAURAModel.generate / generate_tokens on top of them.

The contract is bit equality: clip b of the batched call, over its own frames [0, T_b), is what the scalar call AT THE SAME BATCH with
max_new_tokens = T_b (and the features cut to Tv_b) produces — every comparison here is torch.equal, nothing has a tolerance.

Shapes: B = 4, K = 9, T = [12, 5, 1, 9] (T_b = 1: every codebook but the first is past its end at once), Tv = 32 with video lengths
[32, 2, 1, 3]: at 7 tokens per frame and S = 21, clips 1-3 cross into empty_video_emb inside their valid positions."""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprob_reference as R  # noqa: E402
import test_gpu_logprobs as G  # noqa: E402  (record / struct helpers, the tiny plugin model)
import test_gpu_step_dispatch as D  # noqa: E402  (same_f32, the CPU restatement of the pattern ops)
from oracle import generate_oracle as go  # noqa: E402
from oracle.decoder_oracle import DecoderOracle  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import synth  # noqa: E402
from vaura_amd.engine import DecoderEngine  # noqa: E402

DEV = "cuda:0"
B, K, V = 4, 9, 1024
T = [12, 5, 1, 9]
TMAX, TV = 12, 32
VL = [32, 2, 1, 3]
P = G.P


def stream():
    return L.current_stream(torch.device(DEV))


def i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


@pytest.fixture(scope="module")
def even_delays(golden):
    return [int(d) for d in golden("tiny_delays_even.npz")["delays"]]


@pytest.fixture(scope="module", params=["default", "even"])
def delays(request, even_delays):
    return list(range(K)) if request.param == "default" else even_delays


def dl_arg(delays):
    return L.delays_host(delays)


# ---------------------------------------------------------------------------------------------------------------- 1. op level
def test_op_pattern_build_and_reverts(delays):
    lib, span = L.lib(), max(delays) + 1
    S = TMAX + span
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, V, (B, K, TMAX), generator=g, dtype=torch.int32)
    codes[:, :, 3:] = torch.where(torch.rand(B, K, TMAX - 3, generator=g) < 0.5, torch.tensor(-1, dtype=torch.int32), codes[:, :, 3:])
    codes = codes.to(DEV)
    seq = torch.full((B, K, S), -7, dtype=torch.int32, device=DEV)
    assert lib.vaura_pattern_build_clips(L.ptr(codes), L.ptr(seq), B, K, TMAX, S, V, dl_arg(delays), L.ptr(i32(T)), stream()) == 0
    seqf = torch.randn(B, K, S, generator=g).to(DEV)
    back = torch.full((B, K, TMAX), -7, dtype=torch.int32, device=DEV)
    backf = torch.full((B, K, TMAX), -7.0, device=DEV)
    assert lib.vaura_pattern_revert_clips(L.ptr(seq), L.ptr(back), B, K, TMAX, S, -1, V, dl_arg(delays), L.ptr(i32(T)), stream()) == 0
    assert lib.vaura_pattern_revert_clips_f32(L.ptr(seqf), L.ptr(backf), B, K, TMAX, S, 0.0, 0.0, dl_arg(delays), L.ptr(i32(T)), stream()) == 0
    # against the CPU (the entry points compared below share their kernels with the ones above): the pattern's index maps, and
    # logprob_reference.revert for the fp32 values
    assert torch.equal(seq.cpu(), D.ref_build(codes.cpu(), delays, V, T))
    assert torch.equal(back.cpu(), D.ref_revert(seq.cpu(), delays, TMAX, -1, V, T))
    wantf = torch.from_numpy(R.revert(seqf.cpu().numpy(), delays, TMAX))
    for b, Tb in enumerate(T):
        wantf[b, :, Tb:] = 0.0
    assert torch.equal(backf.cpu().view(torch.int32), wantf.view(torch.int32))
    for b, Tb in enumerate(T):
        Sb = Tb + span
        cb = codes[b:b + 1, :, :Tb].contiguous()
        want = torch.full((1, K, Sb), -7, dtype=torch.int32, device=DEV)
        assert lib.vaura_pattern_build_delays(L.ptr(cb), L.ptr(want), 1, K, Tb, Sb, V, dl_arg(delays), stream()) == 0
        assert torch.equal(seq[b, :, :Sb], want[0]) and bool((seq[b, :, Sb:] == V).all()), b
        wb = torch.full((1, K, Tb), -7, dtype=torch.int32, device=DEV)
        assert lib.vaura_pattern_revert_delays(L.ptr(want), L.ptr(wb), 1, K, Tb, Sb, -1, dl_arg(delays), stream()) == 0
        assert torch.equal(back[b, :, :Tb], wb[0]) and bool((back[b, :, Tb:] == V).all()), b
        sf = seqf[b:b + 1, :, :Sb].contiguous()
        wf = torch.full((1, K, Tb), -7.0, device=DEV)
        assert lib.vaura_pattern_revert_delays_f32(L.ptr(sf), L.ptr(wf), 1, K, Tb, Sb, 0.0, dl_arg(delays), stream()) == 0
        assert torch.equal(backf[b, :, :Tb], wf[0]) and bool((backf[b, :, Tb:] == 0).all()), b
    # refused on the host: a length outside 1 .. T, a missing array
    for bad in ([12, 5, 0, 9], [13, 5, 1, 9]):
        assert lib.vaura_pattern_build_clips(L.ptr(codes), L.ptr(seq), B, K, TMAX, S, V, dl_arg(delays), L.ptr(i32(bad)), stream()) == -1
    assert lib.vaura_pattern_build_clips(L.ptr(codes), L.ptr(seq), B, K, TMAX, S, V, dl_arg(delays), None, stream()) == -1


def test_op_sequence_means(delays):
    lib, span = L.lib(), max(delays) + 1
    S = TMAX + span
    lp = -torch.rand(B, K, S, generator=torch.Generator().manual_seed(4)).to(DEV)
    for t0, Tl in ((0, T), (1, [12, 5, 2, 9])):
        pcb, clip = torch.zeros(B, K, device=DEV), torch.zeros(B, device=DEV)
        assert lib.vaura_sequence_logprob_clips(L.ptr(lp), S, dl_arg(delays), B, K, TMAX, t0, L.ptr(i32(Tl)), L.ptr(pcb), L.ptr(clip), stream()) == 0
        frames = R.revert(lp.cpu().numpy(), delays, TMAX)
        for b, Tb in enumerate(Tl):
            rp, rc = R.sequence_logprob(frames[b:b + 1, :, :Tb], t0)      # the CPU restatement: the sibling below runs the same kernel
            assert D.same_f32(pcb[b], rp[0]) and D.same_f32(clip[b:b + 1], rc), (t0, b)
            one = lp[b:b + 1, :, :Tb + span].contiguous()
            wp, wc = torch.zeros(1, K, device=DEV), torch.zeros(1, device=DEV)
            assert lib.vaura_sequence_logprob(L.ptr(one), Tb + span, dl_arg(delays), 1, K, Tb, t0, L.ptr(wp), L.ptr(wc), stream()) == 0
            assert torch.equal(pcb[b].view(torch.int32), wp[0].view(torch.int32)) and torch.equal(clip[b:b + 1].view(torch.int32), wc.view(torch.int32)), (t0, b)
    pcb, clip = torch.zeros(B, K, device=DEV), torch.zeros(B, device=DEV)       # a clip that ends inside the prompt is refused
    assert lib.vaura_sequence_logprob_clips(L.ptr(lp), S, dl_arg(delays), B, K, TMAX, 1, L.ptr(i32(T)), L.ptr(pcb), L.ptr(clip), stream()) == -1


@pytest.mark.parametrize("per_clip", [False, True], ids=["scalar_params", "per_clip_params"])
def test_op_sampler_fixup_reports_and_counts_nothing_past_a_clips_end(delays, per_clip):
    """vaura_sample_seq with lengths against the same entry with T = T_b, at positions before, across and behind every clip's end; with
    tie_eps = 1 every used decision is a near-tie, so the counter is exactly the number of valid slots filled"""
    lib, span = L.lib(), max(delays) + 1
    S = TMAX + span
    g = torch.Generator().manual_seed(6)
    logits = (torch.randn(2 * B, K, V, generator=g) * 3.0).to(DEV)
    sets = [P(True, 0.8, 250, cfg_scale=3.0), P(False, cfg_scale=6.0), P(True, 1.2, 0, 0.9, cfg_scale=1.0), P(True, 0.7, 100, cfg_scale=2.0)]
    rec = G.records(sets) if per_clip else None
    sp = G.sampling(P(cfg_scale=2.0) if per_clip else sets[0])
    sp.tie_eps = 1.0

    def run(pos, Tscalar, lengths):
        seq = torch.full((B, K, S), -1, dtype=torch.int32, device=DEV)
        seq[0, 2, pos + 1] = 77                                    # a known token stays, whatever the lengths
        bufs = [torch.full((B, K, S), 7.0, device=DEV) for _ in range(3)]
        state = torch.zeros(8, dtype=torch.int32, device=DEV)
        state[0], state[2] = pos, pos
        rc = lib.vaura_sample_seq(L.ptr(logits), B, K, V, C.byref(sp), L.ptr(rec), None, L.ptr(seq), Tscalar, S, L.ptr(state),
                                  dl_arg(delays), L.ptr(lengths), *(L.ptr(x) for x in bufs), stream())
        assert rc == 0
        torch.cuda.synchronize()
        return seq.cpu(), [x.cpu() for x in bufs], state.cpu()

    for pos in (0, 1, 4, 6, 9, 13, S - 2):
        seq, bufs, state = run(pos, TMAX, i32(T))
        assert int(state[0]) == pos + 1 and int(state[2]) == pos + 1
        valid = torch.zeros(B, K, dtype=torch.bool)
        for Tb in sorted(set(T)):
            want_seq, want_bufs, _ = run(pos, Tb, None)
            for b in [i for i, v in enumerate(T) if v == Tb]:
                assert torch.equal(seq[b], want_seq[b]), (pos, b)
                for x, w in zip(bufs, want_bufs):
                    assert torch.equal(x[b].view(torch.int32), w[b].view(torch.int32)), (pos, b)
                for k in range(K):
                    t = pos - delays[k]
                    valid[b, k] = 0 <= t < Tb
        valid[0, 2] = False                                        # the known token: nothing sampled there
        col = seq[:, :, pos + 1]
        assert bool((col[~valid & (col != 77)] == V).all()) and bool((col[valid] < V).all())
        for x in bufs:                                             # written where — and only where — a valid slot was filled
            assert bool((x[:, :, pos + 1][valid] != 7.0).all()) and bool((x[:, :, pos + 1][~valid] == 7.0).all())
            x[:, :, pos + 1] = 7.0
            assert bool((x == 7.0).all())
        assert int(state[6]) == int(valid.sum()), (pos, int(state[6]), int(valid.sum()))
    bad = i32([12, 5, 13, 9])
    seq = torch.full((B, K, S), -1, dtype=torch.int32, device=DEV)
    state = torch.zeros(8, dtype=torch.int32, device=DEV)
    assert lib.vaura_sample_seq(L.ptr(logits), B, K, V, C.byref(sp), L.ptr(rec), None, L.ptr(seq), TMAX, S, L.ptr(state), dl_arg(delays),
                                L.ptr(bad), None, None, None, stream()) == -1
    assert bool((seq == -1).all())


@pytest.fixture(scope="module", params=["h2", "f32"])
def embed_engine(request, tiny_sampler_sd):
    return DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype=request.param, near_tie="off")


def _embed_rows(eng, pos_host, n_pos):
    """vaura_embed -> (n_pos, rows, d_model) row-major"""
    L.check(eng.lib.vaura_embed(C.byref(eng.dec), pos_host, n_pos, stream()), "vaura_embed")
    D, r16 = eng.cfg.d_model, eng._rows_padded(eng.rows)
    out = torch.empty(n_pos, eng.rows, D, device=DEV)
    for p in range(n_pos):
        L.check(eng.lib.vaura_unpack_rows(eng.ws_h.data_ptr() + p * r16 * D * 4, L.ptr(out[p]), eng.rows, D, stream()), "vaura_unpack_rows")
    torch.cuda.synchronize()
    return out


def _prepared(eng, feats, Tv, cfg_on, video_lengths, tokens, delays):
    """tokens (B, K, S) in [0, V]: EVERY slot known — the embedding gathers table rows by token, and the loop never lets it see a slot
    that still holds -1 (the sampler fills position p + 1 before the step that embeds it)"""
    eng.prepare(B, TMAX, Tv, cfg_on, 7, block_size=eng.cfg.block_size, delays=None if delays == list(range(K)) else delays)
    eng._set_lengths(None, video_lengths)
    eng.set_condition(feats[:, :Tv].contiguous())
    assert tokens.shape == (B, K, eng.S) and int(tokens.min()) >= 0 and int(tokens.max()) <= V
    eng.seq.copy_(tokens)
    eng._reset_state()


def test_op_embed(embed_engine, delays):
    eng = embed_engine
    feats = synth.video_features(B, tokens=TV, seed=31).to(DEV)
    S = TMAX + max(delays) + 1
    codes = torch.randint(0, V + 1, (B, K, S), generator=torch.Generator().manual_seed(8), dtype=torch.int32)     # special id included
    cd = eng.cfg.cond_dim
    # without CFG: against the scalar form on features cut to Tv_b, decode form (position from the state) and prefill form
    _prepared(eng, feats, TV, False, VL, codes, delays)
    n_pre = min(S - 1, eng._prefill_positions) if eng._prefill_positions else 0
    got_pre = _embed_rows(eng, 0, n_pre) if n_pre else None
    got = []
    for pos in range(S - 1):
        eng.state[0] = pos
        got.append(_embed_rows(eng, -1, 1)[0])
    got = torch.stack(got)
    if n_pre:
        assert torch.equal(got_pre, got[:n_pre])                   # the two forms agree with each other
    assert L.lib().vaura_embed(C.byref(eng.dec), 0, S + 1, stream()) == -1                    # more positions than the sequence has
    for Tvb in sorted(set(VL)):
        _prepared(eng, feats, Tvb, False, None, codes, delays)
        for pos in range(S - 1):
            eng.state[0] = pos
            want = _embed_rows(eng, -1, 1)[0]
            for b in [i for i, v in enumerate(VL) if v == Tvb]:
                assert torch.equal(got[pos, b], want[b]), (Tvb, pos, b)
    # with CFG: the null-condition row of a clip follows its clip (b = row % B), the stride of cond_proj stays Tv
    _prepared(eng, feats, TV, True, VL, codes, delays)
    proj = eng.cond_projection()
    for pos in (0, 6, 7, 13, 14, 20):
        eng.state[0] = pos
        h = _embed_rows(eng, -1, 1)[0]
        for row in range(2 * B):
            frame = pos // 7
            want = proj[row, frame] if frame < VL[row % B] else eng.empty_video
            assert torch.equal(h[row, :cd], want), (pos, row)
    eng._set_lengths(None, [32, 2, 33, 3])
    assert L.lib().vaura_embed(C.byref(eng.dec), -1, 1, stream()) == -1
    eng._set_lengths(None, None)


# ---------------------------------------------------------------------------------------------------------------- 2. loop
@pytest.fixture(scope="module", params=["h1", "h2", "f32"])
def engine(request, tiny_sampler_sd):
    return DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype=request.param, near_tie="off")


@pytest.fixture(scope="module")
def feats():
    return synth.video_features(B, tokens=TV, seed=31).to(DEV)


def scalar_calls(engine, feats, Tl, vl, **kw):
    """{(T_b, Tv_b): result of the scalar call at the same batch}"""
    out = {}
    for key in sorted(set(zip(Tl, vl))):
        out[key] = engine.generate_codes(feats[:, :key[1]].contiguous(), key[0], **kw)
        engine.check_status()
    return out


def check_tokens(got, ref, Tl, vl):
    assert got.shape == (B, K, max(Tl))
    for b, key in enumerate(zip(Tl, vl)):
        want = ref[key][0] if isinstance(ref[key], tuple) else ref[key]
        assert torch.equal(got[b, :, :Tl[b]], want[b]), b
        assert bool((got[b, :, Tl[b]:] == V).all()), b
        assert bool((got[b, :, :Tl[b]] < V).all()), b


SAMPLED = {"philox": P(True, 0.9, 250), "greedy": P(False)}
PER_CLIP = dict(use_sampling=[True, False, True, True], temp=[0.8, 1.0, 1.3, 0.7], top_k=[250, 0, 0, 64], top_p=[0.0, 0.0, 0.9, 0.0])


@pytest.mark.parametrize("mode", list(SAMPLED))
@pytest.mark.parametrize("case", ["tokens", "tokens_video", "cfg6_per_clip_params", "prompt"])
def test_loop_equals_the_scalar_calls_at_the_same_batch(engine, feats, delays, mode, case):
    dl = None if delays == list(range(K)) else delays
    kw = dict(seed=5, delays=dl, **SAMPLED[mode])
    Tl, vl = T, [TV] * B
    if case == "tokens_video":
        vl = VL
    elif case == "cfg6_per_clip_params":
        kw.update(cfg_scale=[6.0, 6.0, 1.0, 3.0], **(PER_CLIP if mode == "philox" else {}))
    elif case == "prompt":
        Tl = [12, 5, 2, 9]
        kw["prompt"] = torch.randint(0, V, (B, K, 1), generator=torch.Generator().manual_seed(9))
    ragged_kw = dict(kw, video_lengths=vl) if case == "tokens_video" else kw
    got = engine.generate_codes(feats, Tl, **ragged_kw)
    engine.check_status()
    ref = scalar_calls(engine, feats, Tl, vl, **kw)
    check_tokens(got, ref, Tl, vl)
    assert torch.equal(engine.generate_codes(feats, Tl, use_graph=False, **ragged_kw), got)      # with and without the captured graph
    engine.check_status()
    if case == "prompt":
        assert torch.equal(got[:, :, :1].cpu(), kw["prompt"])
    if case == "tokens_video":                                      # what lies behind a clip's last real video token does not matter
        dirty = feats.clone()
        for b, n in enumerate(vl):
            dirty[b, n:] = float("nan")
        assert torch.equal(engine.generate_codes(dirty, Tl, **ragged_kw), got)
        engine.check_status()


def test_loop_refusals(engine, feats):
    for bad_kw, match in ((dict(max_new_tokens=[12, 5, 9]), "3 values"), (dict(max_new_tokens=[12, 5, 0, 9]), "at least 1"),
                          (dict(max_new_tokens=[12, 5, 1, 9], video_lengths=[32, 2, 33, 3]), "video_lengths must lie"),
                          (dict(max_new_tokens=[12, 5, 1, 9], prompt=torch.zeros(B, K, 1, dtype=torch.int64)), "prompt")):
        kw = dict(bad_kw)
        with pytest.raises(L.VauraHipError, match=match):
            engine.generate_codes(feats, kw.pop("max_new_tokens"), **kw)


# ---------------------------------------------------------------------------------------------------------------- 3. CPU oracle
def test_greedy_clips_equal_the_cpu_oracle_run_alone(engine, feats, tiny_sampler_sd, delays):
    """default delays: oracle/generate_oracle.py stand-alone on clip b, T_b frames, its Tv_b video tokens.  The oracle's loop knows the
    default delays only; for the even set clip b's tokens are checked to be the greedy fixed point of the oracle's teacher-forced
    logits on the clip's own sequence (S_b = T_b + max(d) + 1), which is what its loop would produce step by step."""
    orc = DecoderOracle(tiny_sampler_sd, 2, 16)
    default = delays == list(range(K))
    got = engine.generate_codes(feats, T, delays=None if default else delays, video_lengths=VL).cpu()
    engine.check_status()
    for b, (Tb, Tvb) in enumerate(zip(T, VL)):
        fb = feats[b:b + 1, :Tvb].cpu()
        if default:
            want = go.generate(orc, fb, Tb, mode="cached")
            assert torch.equal(got[b:b + 1, :, :Tb], want), b
            continue
        Sb = Tb + max(delays) + 1
        seq = torch.full((1, K, Sb), V, dtype=torch.int64)
        for q, d in enumerate(delays):
            seq[0, q, 1 + d:1 + d + Tb] = got[b, q, :Tb]
        top = orc.forward_full(seq[..., :-1], fb).argmax(-1)        # position p decides step p + 1
        for q, d in enumerate(delays):
            assert torch.equal(top[0, q, d:d + Tb], got[b, q, :Tb]), (b, q)


# ---------------------------------------------------------------------------------------------------------------- 4. reporting
def test_logprobs_relevance_and_candidates(engine, feats, delays):
    dl = None if delays == list(range(K)) else delays
    N = 3
    kw = dict(seed=5, delays=dl, use_sampling=True, temp=[0.8, 1.0, 1.3, 0.7], top_k=250, cfg_scale=3.0, return_logprobs=True,
              return_relevance=True, num_candidates=N)
    got, rep = engine.generate_codes(feats, T, **kw)
    engine.check_status()
    vl = [TV] * B
    ref = scalar_calls(engine, feats, T, vl, **kw)
    assert got.shape == (B * N, K, TMAX)
    for b, Tb in enumerate(T):
        want, wrep = ref[(Tb, TV)]
        rows = slice(b * N, b * N + N)
        assert torch.equal(got[rows, :, :Tb], want[rows]) and bool((got[rows, :, Tb:] == V).all())
        for k in ("logprobs", "relevance", "logprob_cond", "logprob_null"):
            assert torch.equal(rep[k][rows, :, :Tb].view(torch.int32), wrep[k][rows].view(torch.int32)), (b, k)
            assert bool((rep[k][rows, :, Tb:] == 0).all()), (b, k)
        for k in ("per_codebook", "score", "relevance_per_codebook", "sequence_relevance"):        # the means: exactly the scalar calls'
            assert torch.equal(rep[k][rows].view(torch.int32), wrep[k][rows].view(torch.int32)), (b, k)
        assert bool(torch.isfinite(rep["score"][rows]).all())
    # the winner of each clip is the scalar call's winner (vaura_select_candidates on those scores, unchanged)
    c32 = got.to(torch.int32).contiguous()
    won, winner = torch.empty(B, K, TMAX, dtype=torch.int32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
    L.check(L.lib().vaura_select_candidates(L.ptr(rep["score"]), L.ptr(c32), B, N, K, TMAX, L.ptr(won), L.ptr(winner), stream()), "select")
    for b, Tb in enumerate(T):
        want, wrep = ref[(Tb, TV)]
        w32 = want.to(torch.int32).contiguous()
        wwon, wwin = torch.empty(B, K, Tb, dtype=torch.int32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
        L.check(L.lib().vaura_select_candidates(L.ptr(wrep["score"]), L.ptr(w32), B, N, K, Tb, L.ptr(wwon), L.ptr(wwin), stream()), "select")
        assert int(winner[b]) == int(wwin[b]) and torch.equal(won[b, :, :Tb], wwon[b])


# ---------------------------------------------------------------------------------------------------------------- 5. plugin surface
@pytest.fixture(scope="module")
def model(tiny_sampler_sd):
    return G._model(tiny_sampler_sd)


def test_generate_returns_padded_audio_and_lengths(model):
    frames = synth.video_features(B, tokens=TV, seed=31).reshape(B, 1, TV, 768).to(DEV)
    kw = dict(frames=frames, prompt_is_encoded=True, top_k=250, cfg_scale=3.0, return_sampled_indices=True, check=True)
    r = model.generate(max_new_tokens=T, **kw)
    assert set(r) == {"generated_audio", "s_attn_weights", "mha_attn_weights", "sampled_indices", "lengths", "audio_lengths"}
    tok, wav = r["sampled_indices"], r["generated_audio"]
    assert tok.shape == (B, K, TMAX) and torch.equal(r["lengths"].cpu(), torch.tensor(T))
    hop = wav.shape[-1] // TMAX
    assert wav.shape == (B, 1, TMAX * hop) and torch.equal(r["audio_lengths"].cpu(), torch.tensor(T) * hop)
    worst = 0.0
    for b, Tb in enumerate(T):
        alone = model.generate(max_new_tokens=Tb, **kw)
        assert torch.equal(tok[b, :, :Tb], alone["sampled_indices"][b]) and bool((tok[b, :, Tb:] == model.special_token_id).all())
        assert bool((wav[b, :, Tb * hop:] == 0).all())
        one = model.audio_encoder.decode([(tok[b:b + 1, :, :Tb], None)])
        worst = max(worst, float((wav[b:b + 1, :, :Tb * hop] - one).abs().max()))
        print(f"clip {b}: T_b = {Tb}: max |grouped decode - decode alone| = {worst:.3e}")
        assert torch.equal(wav[b:b + 1, :, :Tb * hop], one), (b, worst)
    # generate_tokens: a dict with the padded tokens and the lengths; video lengths alone give a dict too
    d = model.generate_tokens(frames=frames, max_new_tokens=T, prompt_is_encoded=True, top_k=250, cfg_scale=3.0)
    assert set(d) == {"tokens", "lengths"} and torch.equal(d["tokens"], tok)
    d = model.generate_tokens(frames=frames, max_new_tokens=TMAX, video_lengths=VL, prompt_is_encoded=True, top_k=250, check=True)
    assert set(d) == {"tokens", "lengths"} and torch.equal(d["lengths"].cpu(), torch.tensor([TMAX] * B))
    for b, n in enumerate(VL):
        alone = model.generate_tokens(frames=frames[:, :, :n].contiguous(), max_new_tokens=TMAX, prompt_is_encoded=True, top_k=250)
        assert torch.equal(d["tokens"][b], alone[b]), b
    # an int and no video lengths: exactly today's result
    r = model.generate(max_new_tokens=TMAX, **kw)
    assert set(r) == {"generated_audio", "s_attn_weights", "mha_attn_weights", "sampled_indices"}
    assert isinstance(model.generate_tokens(frames=frames, max_new_tokens=TMAX, prompt_is_encoded=True, top_k=250), torch.Tensor)


# ---------------------------------------------------------------------------------------------------------------- 6. one captured graph
def test_other_lengths_of_the_same_longest_clip_replay_the_same_graph(engine, feats):
    kw = dict(seed=5, use_sampling=True, top_k=250, temp=0.9)
    a = engine.generate_codes(feats, T, video_lengths=VL, **kw)
    graph, key = engine._graph.value, engine._graph_key
    assert int(engine.dec_ext2.clip_timesteps) == engine.clip_T.data_ptr() and int(engine.dec_ext2.clip_cond_tokens) == engine.clip_Tv.data_ptr()
    T2, VL2 = [3, 12, 7, 12], [5, 32, 1, 2]
    b = engine.generate_codes(feats, T2, video_lengths=VL2, **kw)
    engine.check_status()
    assert engine._graph.value == graph and engine._graph_key == key            # reused: the lengths live in arrays the engine rewrites
    check_tokens(b, scalar_calls(engine, feats, T2, VL2, **kw), T2, VL2)
    assert torch.equal(engine.generate_codes(feats, T, video_lengths=VL, **kw), a)
    engine.generate_codes(feats, TMAX, **kw)                                     # an int call: no arrays, another graph
    assert int(engine.dec_ext2.clip_timesteps or 0) == 0 and engine._graph_key != key
    engine.check_status()
