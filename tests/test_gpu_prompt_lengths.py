"""Per-clip audio prompt lengths in one batched call, on the device: vaura_decoder_ext3.row_prompt_steps, the masked append of the
group prefill pass (csrc/attention.hip rope_append_rows_kernel, vaura_prefill_rows), the sampler's per-clip counter step (csrc/step.hip
sample_kernel<.., SampleStarts>), the per-clip first frame of the means (sequence_logprob_kernel with clip_t0),
DecoderEngine.generate_codes(prompt_lengths=[..]) and VAURAModel.generate / generate_tokens on top of them.

The contract is bit equality: clip b of the ragged call, over its own frames [0, T_b), is what the same call AT THE SAME BATCH with the
common prompt prompt[..., :P_b] produces (no prompt for P_b = 0) — every comparison here is torch.equal, nothing has a tolerance.

Shapes: B = 4, K = 9, P = [6, 0, 3, 6] (three groups: one without a pass, one alone, one of two clips), max_new_tokens 14 and the
per-clip [14, 9, 14, 8].  PREFILL_POSITIONS 4 makes the pass of 6 positions two chunks, 192 one."""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprob_reference as R  # noqa: E402
import test_gpu_logprobs as G  # noqa: E402  (record / struct helpers, the tiny plugin model)
import test_gpu_step_dispatch as D  # noqa: E402  (same_f32)
from oracle import generate_oracle as go  # noqa: E402
from oracle.decoder_oracle import DecoderOracle  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import synth  # noqa: E402
from vaura_amd.engine import KV_DTYPES, DecoderEngine  # noqa: E402

DEV = "cuda:0"
B, K, V = 4, 9, 1024
PL = [6, 0, 3, 6]
PMAX = 6
TMAX, TV = 14, 32
TL = [14, 9, 14, 8]
P = G.P


def stream():
    return L.current_stream(torch.device(DEV))


def i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module")
def even_delays(golden):
    return [int(d) for d in golden("tiny_delays_even.npz")["delays"]]


@pytest.fixture(scope="module", params=["default", "even"])
def delays(request, even_delays):
    return list(range(K)) if request.param == "default" else even_delays


@pytest.fixture(scope="module")
def feats():
    return synth.video_features(B, tokens=TV, seed=31).to(DEV)


@pytest.fixture(scope="module")
def prompt():
    return torch.randint(0, V, (B, K, PMAX), generator=torch.Generator().manual_seed(9))


class Small(DecoderEngine):
    PREFILL_POSITIONS = 4


def make_engine(sd, wdtype, pp=192, **kw):
    return (Small if pp == 4 else DecoderEngine)(synth.tiny_sampler(2), sd, DEV, wdtype=wdtype, near_tie="off", **kw)


# ---------------------------------------------------------------------------------------------------------------- 1. op level
@pytest.mark.parametrize("kv", KV_DTYPES)
def test_op_rope_append_rows(tiny_sampler_sd, kv):
    """cache and scales pre-filled with 0xFF: the selected rows hold the plain launch's bytes, the others keep theirs, q is rotated
    for every row.  8 rows (cfg), a chunk of 3 positions from position 2, layer 1."""
    eng = make_engine(tiny_sampler_sd, "h2", 4, kv_dtype=kv)
    eng.prepare(B, TMAX, TV, True, 7, block_size=eng.cfg.block_size)
    lib, layer, p0, n = eng.lib, 1, 2, 3
    row_n = i32([6, 0, 3, 6, 6, 0, 3, 6])
    qkv0 = torch.randn(eng.ws_qkv.shape, generator=torch.Generator().manual_seed(12)).to(DEV) * 3.0
    scaled = kv == "f8s"

    def fill():
        eng.ws_qkv.copy_(qkv0)
        for t in (eng.kcache, eng.vcache) + ((eng.kscale, eng.vscale) if scaled else ()):
            t.view(torch.uint8).fill_(0xFF)

    def snap():
        torch.cuda.synchronize()
        return [t.view(torch.uint8).clone() for t in (eng.kcache, eng.vcache) + ((eng.kscale, eng.vscale) if scaled else ())], eng.ws_qkv.clone()

    fill()
    assert lib.vaura_attention_prefill(C.byref(eng.dec), layer, p0, n, stream()) == 0      # its first launch is the plain append
    want, want_q = snap()
    for n_sel, rows in ((6, [0, 3, 4, 7]), (3, [2, 6]), (5, [])):
        fill()
        assert lib.vaura_rope_append_rows(C.byref(eng.dec), layer, p0, n, L.ptr(row_n), n_sel, stream()) == 0
        got, got_q = snap()
        assert torch.equal(got_q.view(torch.int32), want_q.view(torch.int32)), n_sel          # q (and nothing else of qkv) rotated, every row
        for g, w in zip(got, want):
            assert g.shape[0] == eng.cfg.num_layers and g.shape[1] == eng.rows
            for r in range(eng.rows):
                if r in rows:
                    assert torch.equal(g[:, r], w[:, r]), (n_sel, r)
                    assert bool((g[layer, r, :, p0:p0 + n] != 0xFF).any())
                else:
                    assert bool((g[:, r] == 0xFF).all()), (n_sel, r)
    assert lib.vaura_rope_append_rows(C.byref(eng.dec), layer, p0, n, None, 6, stream()) == -1
    assert lib.vaura_rope_append_rows(C.byref(eng.dec), layer, eng.max_len - 1, 2, L.ptr(row_n), 6, stream()) == -1


@pytest.mark.parametrize("per_clip", [False, True], ids=["scalar_params", "per_clip_params"])
@pytest.mark.parametrize("lengths", [False, True], ids=["one_T", "per_clip_T"])
def test_op_sampler_counter_step_is_the_clips_own(delays, per_clip, lengths):
    """vaura_sample_seq_starts against vaura_sample_seq called at the shifted step index, at positions before, at and after every clip's
    start; with tie_eps = 1 every used decision is a near-tie, so the counter is exactly the number of slots actually filled"""
    lib, span = L.lib(), max(delays) + 1
    S = TMAX + span
    g = torch.Generator().manual_seed(6)
    logits = (torch.randn(2 * B, K, V, generator=g) * 3.0).to(DEV)
    sets = [P(True, 0.8, 250, cfg_scale=3.0), P(True, 1.0, 0, cfg_scale=6.0), P(True, 1.2, 0, 0.9, cfg_scale=1.0), P(True, 0.7, 100, cfg_scale=2.0)]
    rec = G.records(sets) if per_clip else None
    sp = G.sampling(P(cfg_scale=2.0) if per_clip else sets[0])
    sp.tie_eps = 1.0
    Tl = i32(TL) if lengths else None
    n = [p + delays[0] for p in PL]

    def start_seq():
        """every clip inside its prompt up to slot n_b (known tokens), -1 behind"""
        seq = torch.full((B, K, S), -1, dtype=torch.int32, device=DEV)
        for b in range(B):
            seq[b, :, :n[b] + 1] = 5
        return seq

    def run(pos, step, starts):
        seq = start_seq()
        bufs = [torch.full((B, K, S), 7.0, device=DEV) for _ in range(3)]
        state = torch.zeros(8, dtype=torch.int32, device=DEV)
        state[0], state[2] = pos, step
        if starts is None:
            rc = lib.vaura_sample_seq(L.ptr(logits), B, K, V, C.byref(sp), L.ptr(rec), None, L.ptr(seq), TMAX, S, L.ptr(state),
                                      L.delays_host(delays), L.ptr(Tl), *(L.ptr(x) for x in bufs), stream())
        else:
            rc = lib.vaura_sample_seq_starts(L.ptr(logits), B, K, V, C.byref(sp), L.ptr(rec), None, L.ptr(seq), TMAX, S, L.ptr(state),
                                             L.delays_host(delays), L.ptr(Tl), L.ptr(starts), *(L.ptr(x) for x in bufs), stream())
        assert rc == 0
        torch.cuda.synchronize()
        return seq.cpu(), [x.cpu() for x in bufs], state.cpu()

    base = start_seq().cpu()
    for pos in sorted({0, 1, min(n) + 1} | {m + d for m in n for d in (-1, 0, 1) if m + d >= 0} | {S - 2}):
        seq, bufs, state = run(pos, pos - min(n), i32(n))
        assert int(state[0]) == pos + 1 and int(state[2]) == pos - min(n) + 1          # the loop's own step goes on counting
        for n_b in sorted(set(n)):
            want_seq, want_bufs, _ = run(pos, pos - n_b, None)
            for b in [i for i, v in enumerate(n) if v == n_b]:
                assert torch.equal(seq[b], want_seq[b]), (pos, b)
                for x, w in zip(bufs, want_bufs):
                    assert torch.equal(bits(x[b]), bits(w[b])), (pos, b)
        filled = (base[:, :, pos + 1] == -1) & (seq[:, :, pos + 1] < V)          # a valid slot that held -1 and got a sampled token
        for b in range(B):
            if pos < n[b]:
                assert torch.equal(seq[b], base[b]) and not bool(filled[b].any()), (pos, b)      # still inside its prompt: nothing written
        for x in bufs:
            assert bool((x[:, :, pos + 1][filled] != 7.0).all()) and bool((x[:, :, pos + 1][~filled] == 7.0).all())
        assert int(state[6]) == int(filled.sum()), (pos, int(state[6]), int(filled.sum()))
    # refused on the host, before any launch: no array, a value out of range
    seq, state = start_seq(), torch.zeros(8, dtype=torch.int32, device=DEV)
    for starts in (None, i32([6, 0, S, 6]), i32([6, -1, 3, 6])):
        assert lib.vaura_sample_seq_starts(L.ptr(logits), B, K, V, C.byref(sp), L.ptr(rec), None, L.ptr(seq), TMAX, S, L.ptr(state),
                                           L.delays_host(delays), L.ptr(Tl), L.ptr(starts), None, None, None, stream()) == -1
    assert torch.equal(seq.cpu(), base) and int(state[0]) == 0


def test_op_sequence_means(delays):
    """the per-clip first frame against the sibling entry points called with t0 = P_b — the same kernel since the entry points share
    one —, and against the CPU restatement of clip b's frames [:, :, :T_b] with t0 = P_b"""
    lib, span = L.lib(), max(delays) + 1
    S = TMAX + span
    lp = -torch.rand(B, K, S, generator=torch.Generator().manual_seed(4)).to(DEV)
    frames = R.revert(lp.cpu().numpy(), delays, TMAX)
    dl = L.delays_host(delays)
    for Tl in (None, TL):
        pcb, clip = torch.zeros(B, K, device=DEV), torch.zeros(B, device=DEV)
        assert lib.vaura_sequence_logprob_starts(L.ptr(lp), S, dl, B, K, TMAX, L.ptr(i32(PL)), L.ptr(i32(Tl)) if Tl else None, L.ptr(pcb),
                                                 L.ptr(clip), stream()) == 0
        for b, t0 in enumerate(PL):
            rp, rc = R.sequence_logprob(frames[b:b + 1, :, :Tl[b] if Tl else TMAX], t0)
            assert D.same_f32(pcb[b], rp[0]) and D.same_f32(clip[b:b + 1], rc), (Tl, b)
            wp, wc = torch.zeros(B, K, device=DEV), torch.zeros(B, device=DEV)
            if Tl is None:
                assert lib.vaura_sequence_logprob(L.ptr(lp), S, dl, B, K, TMAX, t0, L.ptr(wp), L.ptr(wc), stream()) == 0
            else:
                assert lib.vaura_sequence_logprob_clips(L.ptr(lp), S, dl, B, K, TMAX, t0, L.ptr(i32(Tl)), L.ptr(wp), L.ptr(wc), stream()) == 0
            assert torch.equal(bits(pcb[b]), bits(wp[b])) and torch.equal(bits(clip[b:b + 1]), bits(wc[b:b + 1])), (Tl, b)
    pcb, clip = torch.zeros(B, K, device=DEV), torch.zeros(B, device=DEV)
    args = (L.ptr(pcb), L.ptr(clip), stream())
    assert lib.vaura_sequence_logprob_starts(L.ptr(lp), S, dl, B, K, TMAX, None, None, *args) == -1
    assert lib.vaura_sequence_logprob_starts(L.ptr(lp), S, dl, B, K, TMAX, L.ptr(i32([6, 0, 3, 14])), None, *args) == -1     # no frame behind the prompt
    assert lib.vaura_sequence_logprob_starts(L.ptr(lp), S, dl, B, K, TMAX, L.ptr(i32([6, 0, 3, 8])), L.ptr(i32(TL)), *args) == -1
    assert lib.vaura_sequence_logprob_starts(L.ptr(lp), S, dl, B, K, TMAX, L.ptr(i32([6, -1, 3, 6])), None, *args) == -1


# ---------------------------------------------------------------------------------------------------------------- 2. engine
STORAGES = [("h2", 4), ("h2", 192), ("h1", 4), ("h1", 192), ("f32", 192)]


@pytest.fixture(scope="module", params=STORAGES, ids=[f"{w}_pp{p}" for w, p in STORAGES])
def engine(request, tiny_sampler_sd):
    return make_engine(tiny_sampler_sd, *request.param)


def ragged_equals_scalar(engine, feats, prompt, Pl, Tl, N=1, **kw):
    """the ragged call, and against it the same call with the common prompt prompt[..., :p] for every distinct p; returns the ragged result"""
    got = engine.generate_codes(feats, Tl, prompt=prompt, prompt_lengths=Pl, **kw)
    engine.check_status()
    codes, rep = got if isinstance(got, tuple) else (got, None)
    Tb = Tl if isinstance(Tl, list) else [Tl] * B
    assert codes.shape == (B * N, K, max(Tb))
    for p in sorted(set(Pl)):
        ref = engine.generate_codes(feats, Tl, prompt=prompt[..., :p] if p else None, **kw)
        engine.check_status()
        want, wrep = ref if isinstance(ref, tuple) else (ref, None)
        for b in [i for i, v in enumerate(Pl) if v == p]:
            rows = slice(b * N, b * N + N)
            assert torch.equal(codes[rows, :, :Tb[b]], want[rows, :, :Tb[b]]), (p, b)
            assert torch.equal(codes[rows, :, :p].cpu(), prompt[b:b + 1, :, :p].expand(N, K, p)), (p, b)
            assert bool((codes[rows, :, :Tb[b]] < V).all()) and bool((codes[rows, :, Tb[b]:] == V).all()), (p, b)
            for k in (rep or {}):
                assert torch.equal(bits(rep[k][rows]), bits(wrep[k][rows])), (p, b, k)
                if rep[k].dim() == 3:
                    assert bool((rep[k][rows, :, :p] == 0).all()) and bool((rep[k][rows, :, Tb[b]:] == 0).all()), (p, b, k)
    return got


PER_CLIP = dict(use_sampling=[True, False, True, True], temp=[0.8, 1.0, 1.3, 0.7], top_k=[250, 0, 0, 64], top_p=[0.0, 0.0, 0.9, 0.0])
CASES = {
    "greedy": dict(),
    "greedy_cfg3": dict(cfg_scale=3.0),
    "sampled": dict(use_sampling=True, temp=0.9, top_k=250),
    "sampled_mix_cfg3": dict(cfg_scale=[3.0, 3.0, 1.0, 2.0], **PER_CLIP),
}


@pytest.mark.parametrize("Tl", [TMAX, TL], ids=["one_T", "per_clip_T"])
@pytest.mark.parametrize("case", list(CASES))
def test_ragged_call_equals_the_scalar_calls_at_the_same_batch(engine, feats, prompt, delays, case, Tl):
    kw = dict(seed=5, delays=None if delays == list(range(K)) else delays, **CASES[case])
    got = ragged_equals_scalar(engine, feats, prompt, PL, Tl, **kw)
    assert engine.rows == (2 * B if "cfg3" in case else B)
    assert torch.equal(engine.generate_codes(feats, Tl, prompt=prompt, prompt_lengths=PL, use_graph=False, **kw), got)     # with and without the captured graph
    engine.check_status()


def test_reports_and_their_means(engine, feats, prompt, delays):
    kw = dict(seed=5, delays=None if delays == list(range(K)) else delays, return_logprobs=True, return_relevance=True, cfg_scale=[3.0, 3.0, 1.0, 2.0],
              **PER_CLIP)
    for Tl in (TMAX, TL):
        _, rep = ragged_equals_scalar(engine, feats, prompt, PL, Tl, **kw)
        assert set(rep) == {"logprobs", "per_codebook", "score", "relevance", "logprob_cond", "logprob_null", "relevance_per_codebook",
                            "sequence_relevance"}
        assert bool(torch.isfinite(rep["score"]).all()) and bool((rep["logprobs"] != 0).any())


def test_candidates(engine, feats, prompt):
    ragged_equals_scalar(engine, feats, prompt, PL, TL, N=2, seed=5, use_sampling=True, temp=[0.8, 1.0, 1.3, 0.7], top_k=250, cfg_scale=3.0,
                         return_logprobs=True, num_candidates=2)
    assert engine.rows == 16


def test_scaled_fp8_cache(tiny_sampler_sd, feats, prompt):
    eng = make_engine(tiny_sampler_sd, "h2", 4, kv_dtype="f8s")
    ragged_equals_scalar(eng, feats, prompt, PL, TL, seed=5, cfg_scale=3.0, use_sampling=True, temp=0.9, top_k=250)


def test_rows_are_independent_and_nothing_behind_a_prompt_is_read(engine, feats, prompt):
    kw = dict(seed=5, cfg_scale=3.0, use_sampling=True, temp=0.9, top_k=250)
    got = engine.generate_codes(feats, TL, prompt=prompt, prompt_lengths=PL, **kw)
    dirty = prompt.clone()
    for b, p in enumerate(PL):
        dirty[b, :, p:] = 99999                # no token: would leave the embedding table if it were ever gathered
    assert torch.equal(engine.generate_codes(feats, TL, prompt=dirty, prompt_lengths=PL, **kw), got)      # clip 1 (P = 0): all of its prompt
    other = prompt.clone()
    other[2, :, :3] = (other[2, :, :3] + 1) % V
    alt = engine.generate_codes(feats, TL, prompt=other, prompt_lengths=PL, **kw)
    engine.check_status()
    for b in (0, 1, 3):
        assert torch.equal(alt[b], got[b]), b
    assert not torch.equal(alt[2], got[2])


def test_one_graph_for_every_set_of_lengths_and_the_scalar_path_for_equal_ones(engine, feats, prompt):
    kw = dict(seed=5, use_sampling=True, top_k=250, temp=0.9)
    a = engine.generate_codes(feats, TMAX, prompt=prompt, prompt_lengths=PL, **kw)
    graph, key = engine._graph.value, engine._graph_key
    assert int(engine.dec_ext3.row_prompt_steps) == engine.row_n.data_ptr() and engine.prompt_lengths == PL
    P2 = [0, 5, 5, 2]
    b = engine.generate_codes(feats, TMAX, prompt=prompt, prompt_lengths=P2, **kw)
    assert engine._graph.value == graph and engine._graph_key == key            # reused: the lengths live in arrays the engine rewrites
    assert torch.equal(ragged_equals_scalar(engine, feats, prompt, P2, TMAX, **kw), b)      # (its scalar calls capture graphs of their own)
    assert torch.equal(engine.generate_codes(feats, TMAX, prompt=prompt, prompt_lengths=PL, **kw), a)
    # all lengths equal: the scalar call, on its path — no array behind the descriptor, the keyword-less call's bits
    for p in (0, 4):
        same = engine.generate_codes(feats, TMAX, prompt=prompt, prompt_lengths=[p] * B, **kw)
        assert int(engine.dec_ext3.row_prompt_steps or 0) == 0 and engine.prompt_lengths is None and engine._graph_key != key
        assert torch.equal(same, engine.generate_codes(feats, TMAX, prompt=prompt[..., :p] if p else None, **kw))
    engine.check_status()


def test_refusals(engine, feats, prompt):
    for bad, match in (([6, 0, 3], "3 values"), ([6, 0, 3.0, 6], "integers"), ([6, -1, 3, 6], "must lie in 0 .. 6"), ([6, 0, 7, 6], "must lie in 0 .. 6"),
                       ([6, 0, 3, 6, 1], "5 values"), (3, "one integer per clip")):
        with pytest.raises(L.VauraHipError, match=match):
            engine.generate_codes(feats, TMAX, prompt=prompt, prompt_lengths=bad)
    with pytest.raises(L.VauraHipError, match="shorter than its max_new_tokens"):
        engine.generate_codes(feats, [14, 9, 3, 8], prompt=prompt, prompt_lengths=PL)
    with pytest.raises(L.VauraHipError, match="needs an audio prompt"):
        engine.generate_codes(feats, TMAX, prompt_lengths=PL)
    # the C ABI, on the host and before any launch
    engine.generate_codes(feats, TMAX, prompt=prompt, prompt_lengths=PL)
    torch.cuda.synchronize()
    lib, S = engine.lib, engine.S
    before = [t.clone() for t in (engine.kcache, engine.vcache)]
    if not engine.planes:            # tile storages have no prefill workspaces: no pass to run
        assert lib.vaura_prefill_rows(C.byref(engine.dec), 3, 3, stream()) == -1
        return
    for n_pre, n_sel in ((3, 0), (0, 3), (4, 3), (S, S), (3, S)):
        assert lib.vaura_prefill_rows(C.byref(engine.dec), n_pre, n_sel, stream()) == -1, (n_pre, n_sel)
    keep = engine.row_n.clone()
    engine.row_n[2] = S
    assert lib.vaura_prefill_rows(C.byref(engine.dec), 3, 3, stream()) == -1
    engine.row_n.copy_(keep)
    engine.dec_ext3.row_prompt_steps = 0
    assert lib.vaura_prefill_rows(C.byref(engine.dec), 3, 3, stream()) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(before, (engine.kcache, engine.vcache)))


# ---------------------------------------------------------------------------------------------------------------- 3. CPU oracle
def test_greedy_clips_equal_the_cpu_oracle_run_alone(tiny_sampler_sd, feats, prompt):
    eng = make_engine(tiny_sampler_sd, "f32")
    orc = DecoderOracle(tiny_sampler_sd, 2, 16)
    got = eng.generate_codes(feats, TMAX, prompt=prompt, prompt_lengths=PL).cpu()
    eng.check_status()
    for b, p in enumerate(PL):
        want = go.generate(orc, feats[b:b + 1].cpu(), TMAX, prompt=prompt[b:b + 1, :, :p] if p else None, mode="cached")
        assert torch.equal(got[b:b + 1], want), b


# ---------------------------------------------------------------------------------------------------------------- 4. plugin surface
@pytest.fixture(scope="module")
def model(tiny_sampler_sd):
    return G._model(tiny_sampler_sd)


@pytest.fixture(scope="module")
def frames():
    return synth.video_features(B, tokens=TV, seed=31).reshape(B, 1, TV, 768).to(DEV)


def test_generate_tokens_with_prompt_lengths(model, frames, prompt):
    sp = model.special_token_id
    kw = dict(frames=frames, prompt_is_encoded=True, top_k=250, cfg_scale=3.0, check=True)
    d = model.generate_tokens(audio=prompt.to(DEV), prompt_lengths=PL, max_new_tokens=TL, return_logprobs=True, **kw)
    assert set(d) == {"tokens", "lengths", "prompt_lengths", "logprobs", "logprob_per_codebook", "sequence_logprob"}
    assert torch.equal(d["lengths"].cpu(), torch.tensor(TL)) and torch.equal(d["prompt_lengths"].cpu(), torch.tensor(PL))
    for p in sorted(set(PL)):
        one = model.generate_tokens(audio=prompt[..., :p].to(DEV) if p else None, max_new_tokens=TL, return_logprobs=True, **kw)
        for b in [i for i, v in enumerate(PL) if v == p]:
            for k in ("tokens", "logprobs", "logprob_per_codebook", "sequence_logprob"):
                assert torch.equal(bits(d[k][b]), bits(one[k][b])), (p, b, k)
    # remove_prompts: clip b's frames [P_b, T_b) left-aligned, the special id / zeros behind them, lengths = T_b - P_b
    r = model.generate_tokens(audio=prompt.to(DEV), prompt_lengths=PL, max_new_tokens=TL, return_logprobs=True, remove_prompts=True, **kw)
    assert torch.equal(r["lengths"].cpu(), torch.tensor(TL) - torch.tensor(PL)) and torch.equal(r["prompt_lengths"].cpu(), torch.tensor(PL))
    assert r["tokens"].shape == (B, K, TMAX - min(PL))
    for b, (p, t) in enumerate(zip(PL, TL)):
        assert torch.equal(r["tokens"][b, :, :t - p], d["tokens"][b, :, p:t]) and bool((r["tokens"][b, :, t - p:] == sp).all()), b
        assert torch.equal(bits(r["logprobs"][b, :, :t - p]), bits(d["logprobs"][b, :, p:t])) and bool((r["logprobs"][b, :, t - p:] == 0).all()), b
    # one max_new_tokens for every clip: still a dict
    d1 = model.generate_tokens(audio=prompt.to(DEV), prompt_lengths=PL, max_new_tokens=TMAX, **kw)
    assert set(d1) == {"tokens", "lengths", "prompt_lengths"} and torch.equal(d1["lengths"].cpu(), torch.tensor([TMAX] * B))
    # equal lengths: the keyword-less call's bits
    same = model.generate_tokens(audio=prompt.to(DEV), prompt_lengths=[4] * B, max_new_tokens=TMAX, **kw)
    assert torch.equal(same["tokens"], model.generate_tokens(audio=prompt[..., :4].to(DEV), max_new_tokens=TMAX, **kw))
    # refused before any device work
    for bad_kw, match in ((dict(prompt_lengths=[6, 0, 3]), "3 values"), (dict(prompt_lengths=[6, 0, 7, 6]), "must lie"),
                          (dict(prompt_lengths=[6, 0, 3, 14]), "must lie"), (dict(prompt_lengths=PL, audio_lengths=[1, 2, 3, 4]), "both")):
        with pytest.raises(L.VauraHipError, match=match):
            model.generate_tokens(audio=prompt.to(DEV), max_new_tokens=TMAX, **dict(kw, **bad_kw))
    with pytest.raises(L.VauraHipError, match="needs an audio prompt"):
        model.generate_tokens(prompt_lengths=PL, max_new_tokens=TMAX, **kw)


def test_raw_audio_with_audio_lengths(model, frames):
    from vaura_amd.codec_clips import clip_layout
    hop = clip_layout([1], model.audio_encoder.cfg, "encode").hop
    n = [5 * hop, 1, 3 * hop - 7, 5 * hop]
    wav = (torch.randn(B, 1, max(n), generator=torch.Generator().manual_seed(2)) * 0.1).to(DEV)
    codes, plen = model._encode_clips(wav, n)
    assert plen == [5, 1, 3, 5]
    kw = dict(frames=frames, top_k=250, cfg_scale=3.0, max_new_tokens=TMAX)
    d = model.generate_tokens(audio=wav, audio_lengths=n, **kw)
    assert torch.equal(d["prompt_lengths"].cpu(), torch.tensor(plen))
    want = model.generate_tokens(audio=codes, prompt_is_encoded=True, prompt_lengths=plen, **kw)
    assert torch.equal(d["tokens"], want["tokens"])
    for b, p in enumerate(plen):
        assert torch.equal(d["tokens"][b, :, :p], codes[b, :, :p].to(torch.int64)), b


def test_generate_decodes_the_ragged_result(model, frames, prompt):
    kw = dict(frames=frames, prompt_is_encoded=True, top_k=250, cfg_scale=3.0, return_sampled_indices=True, audio=prompt.to(DEV), prompt_lengths=PL)
    for rm in (False, True):
        r = model.generate(max_new_tokens=TL, remove_prompts=rm, **kw)
        assert {"generated_audio", "sampled_indices", "lengths", "audio_lengths", "prompt_lengths"} <= set(r)
        tok, wav, lens = r["sampled_indices"], r["generated_audio"], r["lengths"].tolist()
        assert lens == [t - (p if rm else 0) for t, p in zip(TL, PL)]
        hop = wav.shape[-1] // tok.shape[-1]
        assert torch.equal(r["audio_lengths"].cpu(), torch.tensor(lens) * hop)
        assert torch.equal(wav, model.audio_encoder.decode_clips(tok, lens))
        for b, n in enumerate(lens):
            assert bool((wav[b, :, n * hop:] == 0).all()), b
