"""Video relevance on the device: csrc/step.hip sample_kernel<PC, true, SampleRelevance> (mode 2), vaura_sample_relevance,
vaura_decoder_ext.logprobs_cond / logprobs_null, DecoderEngine.generate_codes(return_relevance=), VAURAModel.generate(return_relevance=,
rank_by=), DecoderEngine.score(relevance=) / vaura_score_relevance.

Tokens are compared with torch.equal (the mode never changes a draw).  lc and lu are compared against fp64 with the bars
tests/test_gpu_logprobs.py applies to lp (``op_bar`` / ``loop_bar``: the same expression at tau = 1, no CFG mix), r = lc - lu with twice
the op bar; the reductions bit for bit against tests/relevance_reference.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relevance_reference as R  # noqa: E402
import test_gpu_logprobs as G  # noqa: E402  (its bars, its record / struct helpers, its tiny plugin model)
from oracle.decoder_oracle import DecoderOracle  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import synth  # noqa: E402
from vaura_amd.engine import DecoderEngine  # noqa: E402

DEV = "cuda:0"
B, K, V = 3, 9, 1024
P = G.P

_lines = []              # "case: largest |error|, bar" (printed; appended to $VAURA_PARITY_DIR/relevance_parity.txt when that is set)


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    out = os.environ.get("VAURA_PARITY_DIR")
    if _lines and out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "relevance_parity.txt"), "a") as f:
            f.write("video relevance against fp64: largest |error| and its bar per case (tests/test_gpu_relevance.py)\n")
            f.writelines(line + "\n" for line in _lines)


def note(case, what, err, bar):
    line = f"{case}: {what}: max |error| = {float(err):.3e}, bar = {float(bar):.3e}, ratio = {float(err) / float(bar):.4f}"
    _lines.append(line)
    print("relevance parity:", line)


# ---------------------------------------------------------------------------------------------------------------- a. op level
MODES = {"greedy": P(False), "topk250_t0.7": P(True, 0.7, 250), "topp0.9_t1.3": P(True, 1.3, 0, 0.9)}


@pytest.fixture(scope="module")
def op_inputs(golden):
    g = torch.Generator().manual_seed(41)
    logits = torch.randn(2 * B, K, V, generator=g) * 4.0
    tie = torch.from_numpy(golden("sampling.npz")["logits"])
    logits[0, 0] = tie[0, 0]          # ten exact copies of one value
    logits[B + 1, 3] = tie[1, 3]      # rounded to one decimal, in a null row: ties at its maximum
    logits[2, 5, 300:330] += 9.0      # a peaked conditional row against a flat null row: lc and lu far apart
    noise = torch.empty(B * K, V).exponential_(1, generator=g)
    return logits.contiguous(), noise.to(DEV).contiguous()


def run_rel(logits, sets, noise, per_clip, seq=None, state=None, sp=None, want_lp=True):
    """vaura_sample_relevance on 2B rows -> (rc, tokens, lp, lc, lu); scalar form: every clip has the set of clip 0"""
    step = 3 if noise is None else 0
    tok = torch.full((B, K), -1, dtype=torch.int32, device=DEV)
    lp, lc, lu = (torch.full((B, K), 7.0, dtype=torch.float32, device=DEV) for _ in range(3))
    rec = G.records(sets) if per_clip else None
    sp = sp or (G.sampling(P(cfg_scale=2.0)) if per_clip else G.sampling(sets[0]))
    rows = logits.to(DEV)
    rc = L.lib().vaura_sample_relevance(L.ptr(rows), B, K, V, C.byref(sp), L.ptr(rec), L.ptr(noise), step, L.ptr(tok), L.ptr(seq),
                                        100 if seq is not None else 0, 0 if seq is None else seq.shape[-1], L.ptr(state),
                                        L.ptr(lp) if want_lp else None, L.ptr(lc), L.ptr(lu), G.stream())
    torch.cuda.synchronize()
    return rc, tok.cpu(), lp.cpu(), lc.cpu(), lu.cpu()


def check_op(case, logits, sets, noise, per_clip):
    rc, tok, lp, lc, lu = run_rel(logits, sets, noise, per_clip)
    assert rc == 0
    assert int(tok.min()) >= 0 and int(tok.max()) < V
    # modes 0, 1, 2: the same tokens; mode 2's lp is mode 1's, bit for bit
    assert torch.equal(tok, G.run_plain(logits, sets, noise, per_clip)), case
    rc1, tok1, lp1 = G.run_lp(logits, sets, noise, per_clip)
    assert rc1 == 0 and torch.equal(tok, tok1) and torch.equal(lp.view(torch.int32), lp1.view(torch.int32)), case
    # lp is optional in mode 2: the same lc / lu without it
    _, tok2, _, lc2, lu2 = run_rel(logits, sets, noise, per_clip, want_lp=False)
    assert torch.equal(tok2, tok) and torch.equal(lc2.view(torch.int32), lc.view(torch.int32)) and torch.equal(lu2.view(torch.int32), lu.view(torch.int32))
    xc, xu = logits[:B].double(), logits[B:].double()
    idx = tok.long()[..., None]
    ref_c = torch.log_softmax(xc, -1).gather(-1, idx)[..., 0]
    ref_u = torch.log_softmax(xu, -1).gather(-1, idx)[..., 0]
    bar_c, bar_u = G.op_bar(xc.abs().amax(-1)), G.op_bar(xu.abs().amax(-1))        # tau = 1: A = max |x| of the row
    err_c, err_u = (lc.double() - ref_c).abs(), (lu.double() - ref_u).abs()
    r = (lc.to(DEV) - lu.to(DEV)).cpu()                                             # one fp32 subtraction, as the engine does it
    bar_r = 2.0 * torch.maximum(bar_c, bar_u)
    err_r = (r.double() - (ref_c - ref_u)).abs()
    for what, err, bar in (("lc", err_c, bar_c), ("lu", err_u, bar_u), ("r", err_r, bar_r)):
        i = int((err / bar).argmax())
        note(case, what, err.flatten()[i], bar.flatten()[i])
        assert bool((err <= bar).all()), (case, what, float((err / bar).max()))
    # the restatement in the kernel's reduction order agrees with the plain fp64 softmax far inside the bar
    want = R.token_relevance(logits[1, 2].numpy(), logits[B + 1, 2].numpy(), int(tok[1, 2]))
    assert abs(want[0] - float(ref_c[1, 2])) < 1e-10 and abs(want[1] - float(ref_u[1, 2])) < 1e-10
    return tok, lc, lu


@pytest.mark.parametrize("philox", [False, True], ids=["recorded", "philox"])
@pytest.mark.parametrize("mode", list(MODES))
def test_op_scalar_parameters(op_inputs, mode, philox):
    logits, noise = op_inputs
    sets = [dict(MODES[mode], cfg_scale=3.0)] * B
    check_op(f"op scalar {mode} cfg 3 {'philox' if philox else 'recorded'}", logits, sets, None if philox else noise, False)


@pytest.mark.parametrize("philox", [False, True], ids=["recorded", "philox"])
@pytest.mark.parametrize("order,cfgs", [([0, 1, 2], [3.0, 1.0, 2.0]), ([2, 0, 1], [0.5, 6.0, 1.0])], ids=["gkp", "pgk"])
def test_op_per_clip_records_mixing_all_three_modes(op_inputs, order, cfgs, philox):
    """one clip greedy, one top-k, one top-p; a clip whose scale is <= 1 draws un-mixed and its null row is read for lu only"""
    logits, noise = op_inputs
    modes = list(MODES.values())
    sets = [dict(modes[i], cfg_scale=c) for i, c in zip(order, cfgs)]
    check_op(f"op per-clip {order} cfg {cfgs} {'philox' if philox else 'recorded'}", logits, sets, None if philox else noise, True)


def test_op_every_clip_unmixed_in_a_doubled_batch(op_inputs):
    """the forced-doubling path of the engine: records with scale <= 1 only, the scalar scale says that rows [B, 2B) exist; the tokens
    are those of the B-row call"""
    logits, noise = op_inputs
    modes = list(MODES.values())
    sets = [dict(modes[i], cfg_scale=c) for i, c in zip([1, 0, 2], [1.0, 1.0, 0.5])]
    rc, tok, lp, lc, lu = run_rel(logits, sets, noise, True)
    assert rc == 0
    assert torch.equal(tok, G.run_plain(logits, sets, noise, True))                 # B rows, vaura_sample_clips
    rc1, tok1, lp1 = G.run_lp(logits, sets, noise, True)
    assert torch.equal(tok, tok1) and torch.equal(lp.view(torch.int32), lp1.view(torch.int32))
    idx = tok.long()[..., None]
    ref_c = torch.log_softmax(logits[:B].double(), -1).gather(-1, idx)[..., 0]
    ref_u = torch.log_softmax(logits[B:].double(), -1).gather(-1, idx)[..., 0]
    assert bool(((lc.double() - ref_c).abs() <= G.op_bar(logits[:B].double().abs().amax(-1))).all())
    assert bool(((lu.double() - ref_u).abs() <= G.op_bar(logits[B:].double().abs().amax(-1))).all())
    # greedy, un-mixed, tau = 1: lp IS lc (the same expression in the same order)
    assert torch.equal(lp[1].view(torch.int32), lc[1].view(torch.int32))


def test_op_two_equal_maxima_report_the_token_actually_chosen():
    """mixed logits 3 lc - 2 lu tie exactly at columns 100 and 700 (both 20) while the rows differ there: greedy takes 100, and lc / lu
    are those of column 100"""
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(2 * B, K, V, generator=g)
    for b in range(B):
        logits[b, :, 100], logits[B + b, :, 100] = 10.0, 5.0
        logits[b, :, 700], logits[B + b, :, 700] = 12.0, 8.0
    sets = [dict(P(False), cfg_scale=3.0)] * B
    rc, tok, lp, lc, lu = run_rel(logits, sets, None, False)
    assert rc == 0 and bool((tok == 100).all())
    ls_c, ls_u = torch.log_softmax(logits[:B].double(), -1), torch.log_softmax(logits[B:].double(), -1)
    assert bool(((lc.double() - ls_c[..., 100]).abs() <= G.op_bar(torch.tensor(12.0))).all())
    assert bool(((lu.double() - ls_u[..., 100]).abs() <= G.op_bar(torch.tensor(8.0))).all())
    assert bool(((lc.double() - ls_c[..., 700]).abs() > 1.0).all())                  # ... and not those of the other maximum


def test_op_inf_logit_gives_nan_in_both_and_the_status_bit(op_inputs):
    logits, noise = op_inputs
    sets = [dict(MODES["greedy"], cfg_scale=6.0), dict(MODES["topk250_t0.7"], cfg_scale=6.0), dict(MODES["topp0.9_t1.3"], cfg_scale=1.0)]
    bad = logits.clone()
    bad[0, 2, 17] = float("inf")          # clip 0, codebook 2, conditional row
    bad[B + 1, 4, 900] = float("-inf")    # clip 1, codebook 4, null row (mixed)
    bad[2, 7, 0] = float("nan")           # clip 2, codebook 7
    bad[B + 2, 1, 5] = float("-inf")      # clip 2 draws un-mixed: its null row is read for lu only
    S = K + 4
    seq = torch.full((B, K, S), -1, dtype=torch.int32, device=DEV)
    state = torch.zeros(8, dtype=torch.int32, device=DEV)
    state[0] = K
    rc, tok, lp, lc, lu = run_rel(bad, sets, noise, True, seq=seq, state=state)
    assert rc == 0
    assert int(state[4]) & 1
    nan = torch.zeros(B, K, dtype=torch.bool)
    nan[0, 2] = nan[1, 4] = nan[2, 7] = nan[2, 1] = True
    assert torch.equal(torch.isnan(lc), nan) and torch.equal(torch.isnan(lu), nan)
    assert int(tok.min()) >= 0 and int(tok.max()) < V and torch.equal(seq[:, :, K + 1].cpu(), tok)
    rc, tok0, lp0, lc0, lu0 = run_rel(logits, sets, noise, True)                     # the clean launch: the other rows' values
    assert torch.equal(tok[~nan], tok0[~nan]) and torch.equal(lc[~nan], lc0[~nan]) and torch.equal(lu[~nan], lu0[~nan])
    assert torch.equal(tok[2, 1], tok0[2, 1]) and torch.equal(lp[2, 1], lp0[2, 1])   # the un-mixed draw never read that null row


def test_op_refusals(op_inputs):
    logits, noise = op_inputs
    sets = [dict(MODES["greedy"], cfg_scale=1.0)] * B
    rc, tok, lp, lc, lu = run_rel(logits, sets, noise, False)                        # scalar scale 1: no null rows stated
    assert rc == -1 and bool((lc == 7.0).all()) and bool((tok == -1).all())          # VAURA_ERR_ARG, nothing launched
    rc, *_ = run_rel(logits, sets, noise, True, sp=G.sampling(P(cfg_scale=1.0)))     # records, but the scalar does not say doubled
    assert rc == -1
    sp = G.sampling(P(cfg_scale=3.0))
    one = torch.zeros(B, K, dtype=torch.float32, device=DEV)
    tk = torch.zeros(B, K, dtype=torch.int32, device=DEV)
    for lc_p, lu_p in ((L.ptr(one), None), (None, L.ptr(one))):                      # exactly one of the two pointers
        assert L.lib().vaura_sample_relevance(L.ptr(logits.to(DEV)), B, K, V, C.byref(sp), None, None, 0, L.ptr(tk), None, 0, 0, None, None,
                                              lc_p, lu_p, G.stream()) == -1


# ---------------------------------------------------------------------------------------------------------------- b. loop level
T, TV = 12, 32
LOOP = P(True, 0.8, 250)


@pytest.fixture(scope="module", params=["h2", "f32"])
def engine(request, tiny_sampler_sd):
    return DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype=request.param, near_tie="off")


@pytest.fixture(scope="module")
def oracle(tiny_sampler_sd):
    return DecoderOracle(tiny_sampler_sd, 2, 16)


@pytest.fixture(scope="module")
def loop_feats():
    return synth.video_features(B, tokens=TV, seed=31)


_oracle_cache = {}


def oracle_rows(oracle, feats, codes, delays):
    """fp64 log-softmax of the CPU oracle's conditional and null logits at the generated tokens -> (lc, lu, Ac, Au (B, K, T), biggest)"""
    key = (codes.numpy().tobytes(), tuple(delays))
    if key not in _oracle_cache:
        Bc, Kc, Tc = codes.shape
        S = Tc + max(delays) + 1
        seq = torch.full((Bc, Kc, S), V, dtype=torch.int64)
        for q, d in enumerate(delays):
            seq[:, q, 1 + d:1 + d + Tc] = codes[:, q]
        out = []
        for cond in (feats, oracle.null_condition(feats)):
            x = oracle.forward_full(seq[..., :-1], cond).double()                    # position p decides step p + 1
            lsm = torch.log_softmax(x, -1)
            lp, A = torch.zeros(Bc, Kc, Tc, dtype=torch.float64), torch.zeros(Bc, Kc, Tc, dtype=torch.float64)
            for q, d in enumerate(delays):
                lp[:, q] = lsm[:, q, d:d + Tc].gather(-1, codes[:, q, :, None])[..., 0]
                A[:, q] = x[:, q, d:d + Tc].abs().amax(-1)
            out.append((lp, A, float(x.abs().max())))
        _oracle_cache[key] = (out[0][0], out[1][0], out[0][1], out[1][1], max(out[0][2], out[1][2]))
    return _oracle_cache[key]


@pytest.mark.parametrize("pattern,Tp", [("default", 0), ("parallel", 0), ("default", 3)], ids=["default", "parallel", "default_prompt3"])
def test_loop_relevance(engine, oracle, loop_feats, pattern, Tp):
    s = dict(LOOP, cfg_scale=3.0)
    delays = None if pattern == "default" else [0] * K
    dl = list(range(K)) if delays is None else delays
    prompt = torch.randint(0, V, (B, K, Tp), generator=torch.Generator().manual_seed(9)) if Tp else None
    feats = loop_feats.to(DEV)
    kw = dict(prompt=prompt, seed=5, delays=delays, **s)
    plain = engine.generate_codes(feats, T, **kw).cpu()
    engine.check_status()
    got, rel = engine.generate_codes(feats, T, return_relevance=True, **kw)
    engine.check_status()
    got = got.cpu()
    assert set(rel) == {"relevance", "logprob_cond", "logprob_null", "relevance_per_codebook", "sequence_relevance"}
    # what is stored where (tests/relevance_reference.py ``stored``): only sampled tokens of real timesteps, 0 everywhere else
    lay_c, lay_u = engine.logprobs_cond.cpu(), engine.logprobs_null.cpu()
    S = T + max(dl) + 1
    written = torch.zeros(B, K, S, dtype=torch.bool)
    for q, d in enumerate(dl):
        written[:, q, 1 + d + Tp:1 + d + T] = True                                   # slots that held -1 and carry a timestep
    assert bool((lay_c[~written] == 0).all()) and bool((lay_u[~written] == 0).all())
    assert bool((lay_c[written] < 0).all()) and bool((lay_u[written] < 0).all())
    rel = {k: v.cpu() for k, v in rel.items()}
    assert torch.equal(got, plain)                                                   # relevance never changes a token ...
    both, lpr = engine.generate_codes(feats, T, return_relevance=True, return_logprobs=True, use_graph=False, **kw)
    assert torch.equal(both.cpu(), plain)                                            # ... with the log-probabilities, without the graph
    assert all(torch.equal(lpr[k].cpu().view(torch.int32), rel[k].view(torch.int32)) for k in rel)
    _, lp1 = engine.generate_codes(feats, T, return_logprobs=True, **kw)
    assert all(torch.equal(lpr[k].view(torch.int32), lp1[k].view(torch.int32)) for k in lp1)      # mode 2's lp is mode 1's
    if Tp:
        assert torch.equal(got[..., :Tp], prompt)
        assert all(bool((rel[k][..., :Tp] == 0).all()) for k in ("relevance", "logprob_cond", "logprob_null"))
    # against the CPU oracle: each row on its own, tau = 1, no mix -> the loop bar of an un-mixed greedy-temperature decision
    ref_c, ref_u, Ac, Au, biggest = oracle_rows(oracle, loop_feats, got, dl)
    one = P(False, cfg_scale=1.0)
    for what, val, ref, A in (("logprob_cond", rel["logprob_cond"], ref_c, Ac), ("logprob_null", rel["logprob_null"], ref_u, Au)):
        bar = G.loop_bar(A, one, biggest)[..., Tp:]
        err = (val.double() - ref).abs()[..., Tp:]
        i = int((err / bar).argmax())
        note(f"loop {engine.wdtype} {pattern} prompt {Tp}", what, err.flatten()[i], bar.flatten()[i])
        assert bool((err <= bar).all()), (what, float((err / bar).max()))
    # r and its reductions: bit-equal to the restatement applied to the returned values
    r, want_pcb, want_clip = R.sequence_relevance(rel["logprob_cond"].numpy(), rel["logprob_null"].numpy(), Tp)
    assert np.array_equal(rel["relevance"].numpy().view(np.int32), r.view(np.int32))
    assert np.array_equal(rel["relevance_per_codebook"].numpy().view(np.int32), want_pcb.view(np.int32))
    assert np.array_equal(rel["sequence_relevance"].numpy().view(np.int32), want_clip.view(np.int32))


@pytest.mark.parametrize("cfg", [3.0, 1.0, [3.0, 1.0, 0.5]], ids=["cfg3", "cfg1_forced_doubling", "per_clip"])
@pytest.mark.parametrize("mode", ["greedy", "topk"])
def test_loop_tokens_do_not_depend_on_the_flag_and_two_runs_agree(engine, loop_feats, cfg, mode):
    feats = loop_feats.to(DEV)
    kw = dict(seed=7, cfg_scale=cfg, **{k: v for k, v in (P(False) if mode == "greedy" else LOOP).items() if k != "cfg_scale"})
    plain = engine.generate_codes(feats, T, **kw)
    rows_plain = engine.rows
    engine.check_status()
    got, rel = engine.generate_codes(feats, T, return_relevance=True, **kw)
    engine.check_status()
    assert engine.rows == 2 * B and rows_plain == (B if cfg == 1.0 else 2 * B)       # cfg 1: the null rows are carried for the flag alone
    assert torch.equal(got, plain)
    again, rel2 = engine.generate_codes(feats, T, return_relevance=True, **kw)
    assert torch.equal(again, got)
    assert all(torch.equal(rel2[k].view(torch.int32), rel[k].view(torch.int32)) for k in rel)      # "sequence_relevance" among them
    assert bool(torch.isfinite(rel["sequence_relevance"]).all())
    assert torch.equal(engine.generate_codes(feats, T, **kw), plain)                 # and back: the flag leaves nothing behind
    assert int(engine.dec_ext.logprobs_cond or 0) == 0 and int(engine.dec_ext.logprobs_null or 0) == 0


def test_relevance_pointers_key_the_step_graph_and_one_alone_is_refused(engine, loop_feats):
    feats = loop_feats.to(DEV)
    s = dict(LOOP, cfg_scale=3.0)
    engine.generate_codes(feats, T, seed=5, **s)
    off = engine._graph_key
    engine.generate_codes(feats, T, seed=5, return_relevance=True, **s)
    assert int(engine.dec_ext.logprobs_cond or 0) == engine.logprobs_cond.data_ptr() and engine._graph_key != off
    torch.cuda.synchronize()
    engine.check_status()
    sp = engine._sampling(True, 0.8, 250, 0.0, 3.0, 5, 0)
    engine.dec_ext.logprobs_null = 0                                                     # exactly one of the two
    pos = int(engine.state[0])
    assert engine.lib.vaura_decode_step(C.byref(engine.dec), C.byref(sp), 1, L.current_stream(torch.device(DEV))) == -1
    torch.cuda.synchronize()
    assert int(engine.state[0]) == pos                                               # nothing ran
    engine.generate_codes(feats, T, seed=5, **s)
    assert engine._graph_key == off
    engine.check_status()


# ---------------------------------------------------------------------------------------------------------------- c. candidates
N = 3


@pytest.fixture(scope="module")
def model(tiny_sampler_sd):
    return G._model(tiny_sampler_sd)


def test_rank_by_relevance(model):
    LB = 2
    frames = synth.video_features(LB, tokens=TV, seed=31).reshape(LB, 1, TV, 768).to(DEV)
    kw = dict(max_new_tokens=T, prompt_is_encoded=True, use_sampling=True, top_k=250, temp=0.9, cfg_scale=3.0, return_sampled_indices=True)
    r = model.generate(frames=frames, num_candidates=N, rank_by="relevance", return_relevance=True, **kw)
    # all takes equal the repeated batch
    plain = model.generate(frames=frames.repeat_interleave(N, 0), return_relevance=True, **kw)
    assert r["candidate_indices"].shape == (LB * N, K, T)
    assert torch.equal(r["candidate_indices"], plain["sampled_indices"])
    scores = r["candidate_scores"].cpu()
    assert scores.shape == (LB, N) and bool(torch.isfinite(scores).all())
    assert torch.equal(r["candidate_scores"].reshape(-1), plain["sequence_relevance"])            # the score that ranked
    win = G.first_argmax(scores)
    assert torch.equal(r["selected_candidate"].cpu(), win)
    rows = torch.arange(LB) * N + win
    assert torch.equal(r["sampled_indices"].cpu(), r["candidate_indices"].cpu()[rows])
    assert torch.equal(r["sequence_relevance"].cpu(), scores[torch.arange(LB), win])
    assert torch.equal(r["relevance"].cpu(), plain["relevance"].cpu()[rows]) and r["relevance"].shape == (LB, K, T)
    assert "sequence_logprob" not in r and "logprobs" not in r
    assert r["generated_audio"].shape[0] == LB
    # without return_relevance: ranked the same way, nothing of the per-token values returned
    q = model.generate(frames=frames, num_candidates=N, rank_by="relevance", **kw)
    assert torch.equal(q["sampled_indices"], r["sampled_indices"]) and torch.equal(q["candidate_scores"], r["candidate_scores"])
    assert "relevance" not in q and "sequence_relevance" not in q
    # rank_by="logprob" is the call as it is today, whether spelled out or not
    a = model.generate(frames=frames, num_candidates=N, return_logprobs=True, **kw)
    b = model.generate(frames=frames, num_candidates=N, return_logprobs=True, rank_by="logprob", **kw)
    assert set(a) == set(b) == {"generated_audio", "s_attn_weights", "mha_attn_weights", "sampled_indices", "candidate_indices",
                                "candidate_scores", "selected_candidate", "logprobs", "logprob_per_codebook", "sequence_logprob"}
    assert all(torch.equal(a[k], b[k]) for k in a if a[k] is not None)
    assert torch.equal(a["candidate_scores"].cpu()[torch.arange(LB), a["selected_candidate"].cpu()], a["sequence_logprob"].cpu())
    assert torch.equal(a["candidate_indices"], r["candidate_indices"])               # the same takes, ranked by another score


def test_generate_tokens_returns_relevance_and_remove_prompts_slices_it(model):
    LB = 2
    frames = synth.video_features(LB, tokens=TV, seed=31).reshape(LB, 1, TV, 768).to(DEV)
    prompt = torch.randint(0, V, (LB, K, 3), generator=torch.Generator().manual_seed(9)).to(DEV)
    kw = dict(frames=frames, audio=prompt, max_new_tokens=T, prompt_is_encoded=True, top_k=250, cfg_scale=1.0)
    full = model.generate_tokens(return_relevance=True, **kw)
    cut = model.generate_tokens(return_relevance=True, remove_prompts=True, **kw)
    assert torch.equal(full["tokens"], model.generate_tokens(**kw))                  # cfg 1: the forced-doubling path
    assert set(full) == {"tokens", "relevance", "logprob_cond", "logprob_null", "relevance_per_codebook", "sequence_relevance"}
    for k in ("relevance", "logprob_cond", "logprob_null"):
        assert full[k].shape == (LB, K, T) and cut[k].shape == (LB, K, T - 3)
        assert torch.equal(cut[k], full[k][..., 3:]) and bool((full[k][..., :3] == 0).all())
    assert torch.equal(cut["sequence_relevance"], full["sequence_relevance"])


# ---------------------------------------------------------------------------------------------------------------- d. scoring
@pytest.fixture(scope="module")
def score_engine(tiny_sampler_sd):
    return DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype="h2", near_tie="off")


@pytest.mark.parametrize("name", ["delayed", "parallel"])
def test_score_relevance(score_engine, golden, name):
    g = golden("eval_tiny.npz")
    codes = torch.from_numpy(g[f"{name}_codes"].astype(np.int64)).to(DEV)
    d = [int(x) for x in g[f"{name}_delays"]]
    delays = None if d == list(range(K)) else d
    Bc = codes.shape[0]
    feats = synth.video_features(Bc, seed=int(g["feat_seed"])).to(DEV)
    eng = score_engine
    base = {k: v.clone() for k, v in eng.score(codes, feats, delays=delays).items()}
    r = {k: v.clone() for k, v in eng.score(codes, feats, delays=delays, relevance=True).items()}
    # today's entries: the bits of the call without the flag (the conditional rows do not notice the null rows next to them)
    assert set(base) <= set(r) and all(torch.equal(r[k], base[k]) for k in base)
    # "nll_per_codebook" (B, K): the fixed-order mean of today's "nll" over the timesteps
    want = np.stack([[R.codebook_mean(row, 0) for row in clip] for clip in base["nll"].cpu().numpy()])
    assert np.array_equal(r["nll_per_codebook"].cpu().numpy().view(np.int32), want.view(np.int32))
    # the null rows: score() of the same codes given the null condition explicitly
    null_feats = torch.zeros_like(feats) + eng.uncond.to(DEV)
    n = eng.score(codes, null_feats, delays=delays)
    assert float((r["nll_null"] - n["nll"]).abs().max()) < 1e-4
    rel_err = ((r["loss_null_per_codebook"] - n["loss_per_codebook"]).abs() / n["loss_per_codebook"].abs()).max()
    assert float(rel_err) < 1e-5 and abs(float(r["loss_null"]) - float(n["loss"])) < 1e-5 * abs(float(n["loss"]))
    want0 = np.stack([[R.codebook_mean(row, 0) for row in clip] for clip in n["nll"].cpu().numpy()]).astype(np.float64)
    got0 = r["nll_null_per_codebook"].cpu().numpy().astype(np.float64)
    assert float(np.max(np.abs(got0 - want0) / np.abs(want0))) < 1e-5
    # relevance: their difference, and its mean over the codebooks
    assert torch.equal(r["relevance_per_codebook"], r["nll_null_per_codebook"] - r["nll_per_codebook"])
    assert r["relevance_per_codebook"].shape == (Bc, K) and r["relevance"].shape == (Bc,)
    assert float((r["relevance"].double() - r["relevance_per_codebook"].double().mean(-1)).abs().max()) < 1e-6
    again = eng.score(codes, feats, delays=delays, relevance=True)
    assert all(torch.equal(again[k], r[k]) for k in r)                               # two calls: the same bits


def test_sampler_and_scoring_agree_on_generated_tokens(score_engine, loop_feats):
    """The one check that ties the two paths together.  Greedy generation at cfg 1 under the parallel pattern (every position's input in
    teacher-forced scoring is then the decode loop's: with delays, positions past Ta + d_0 are fed the special token instead of the
    last timestep); scoring the generated tokens gives -lc and -lu per token, so the per-codebook means agree within the mean of the
    loop bars — each path is held to that bar against the same oracle arithmetic."""
    eng = score_engine
    feats = loop_feats.to(DEV)
    delays = [0] * K
    codes, rel = eng.generate_codes(feats, T, delays=delays, return_relevance=True, use_sampling=False, cfg_scale=1.0)
    eng.check_status()
    codes = codes.clone()
    rel = {k: v.clone() for k, v in rel.items()}
    sc = eng.score(codes, feats, delays=delays, relevance=True, return_logits=True)
    sc = {k: v.clone() for k, v in sc.items()}
    null_logits = eng.score(codes, torch.zeros_like(feats) + eng.uncond.to(DEV), delays=delays, return_logits=True)["logits"]
    Ac, Au = sc["logits"].double().abs().amax(-1).cpu(), null_logits.double().abs().amax(-1).cpu()      # (B, K, T): max |x| of every row
    biggest = float(max(Ac.max(), Au.max()))
    one = P(False, cfg_scale=1.0)
    for what, mine, theirs, A in (("lc", rel["logprob_cond"], sc["nll_per_codebook"], Ac), ("lu", rel["logprob_null"], sc["nll_null_per_codebook"], Au)):
        bar = G.loop_bar(A, one, biggest).mean(-1)                                   # (B, K): the mean of the per-token bars
        err = (mine.double().mean(-1).cpu() + theirs.double().cpu()).abs()           # mean lc == -mean nll
        i = int((err / bar).argmax())
        note("sampler vs teacher-forced scoring, greedy cfg 1 parallel", what, err.flatten()[i], bar.flatten()[i])
        assert bool((err <= bar).all()), (what, float((err / bar).max()))
