"""Token log-probabilities and best-of-N candidates on the device: csrc/step.hip sample_kernel<PC, LP = true>, vaura_sample_logprobs,
vaura_decoder.logprobs, vaura_sequence_logprob, vaura_pattern_revert_delays_f32, vaura_select_candidates,
DecoderEngine.generate_codes(return_logprobs=, num_candidates=), VAURAModel.generate(return_logprobs=, num_candidates=, ...).

Tokens are compared with torch.equal (LP never changes a draw).  Log-probabilities are compared against fp64 with bars that come from
the arithmetic (see ``op_bar`` / ``loop_bar``), the reductions bit for bit against tests/logprob_reference.py."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprob_reference as R  # noqa: E402
from oracle.decoder_oracle import DecoderOracle  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import clip_params, synth  # noqa: E402
from vaura_amd.engine import DecoderEngine  # noqa: E402

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, K, V = 3, 9, 1024
NAMES = clip_params.NAMES
U = 2.0 ** -24           # unit roundoff of fp32


def P(use_sampling=False, temp=1.0, top_k=0, top_p=0.0, cfg_scale=1.0):
    return dict(use_sampling=use_sampling, temp=temp, top_k=top_k, top_p=top_p, cfg_scale=cfg_scale)


def tau_of(s):
    """the temperature the log-probability is taken at: temp where the clip samples, 1 where it is greedy (fp32, as the kernel holds it)"""
    return float(np.float32(s["temp"])) if (s["use_sampling"] and s["temp"] > 0) else 1.0


def stream():
    return L.current_stream(torch.device(DEV))


def sampling(s, seed=11):
    return L.Sampling(int(bool(s["use_sampling"])), float(s["temp"]), int(s["top_k"]), float(s["top_p"]), float(s["cfg_scale"]), seed, 0, 0, 0.0)


def records(sets):
    p = clip_params.resolve(len(sets), **{n: [s[n] for s in sets] for n in NAMES})
    return torch.frombuffer(bytearray(clip_params.pack_records(p)), dtype=torch.int32).view(len(sets), 8).to(DEV)


def mix_cpu(logits, sets):
    """the fp32 mixed logits of every clip, with the kernel's expression lu + (lc - lu) * s (cfg <= 1: the conditional row itself)"""
    n = len(sets)
    rows = []
    for b, s in enumerate(sets):
        lc = logits[b]
        if s["cfg_scale"] > 1.0:
            lu = logits[n + b]
            rows.append(lu + (lc - lu) * torch.tensor(s["cfg_scale"], dtype=torch.float32))
        else:
            rows.append(lc.clone())
    return torch.stack(rows)


def op_bar(A):
    """|lp - fp64| <= (4 A + 32) 2^-24 with A = max |x / tau| of the row: two roundings of x / tau on each side of the difference
    (x[token] / tau - mx), about 14 roundings and 2 ulp of expf across the 1024-term sum, 2 ulp of logf on at most ln 1024."""
    return (4.0 * A + 32.0) * U


_ratios = {}             # case -> largest observed |error| / bar (printed; written to $VAURA_PARITY_DIR/logprob_parity.txt when that is set)


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    out = os.environ.get("VAURA_PARITY_DIR")
    if _ratios and out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "logprob_parity.txt"), "w") as f:
            f.write("token log-probabilities against fp64: largest |error| / bar per case (tests/test_gpu_logprobs.py)\n")
            for k in sorted(_ratios):
                f.write(f"{_ratios[k]:8.4f}  {k}\n")


def note(case, ratio):
    _ratios[case] = max(_ratios.get(case, 0.0), float(ratio))
    print(f"logprob parity: {case}: max |error| / bar = {float(ratio):.4f}")


# ---------------------------------------------------------------------------------------------------------------- a. op level
MODES = {"greedy": P(False), "topk250_t0.7": P(True, 0.7, 250), "topp0.9_t1.3": P(True, 1.3, 0, 0.9)}


@pytest.fixture(scope="module")
def raw_inputs(golden):
    g = torch.Generator().manual_seed(23)
    logits = torch.randn(2 * B, K, V, generator=g)
    tie = torch.from_numpy(golden("sampling.npz")["logits"])
    logits[0, 0] = tie[0, 0]          # ten exact copies of one value: the k-th largest of a top-k cut is shared
    logits[1, 3] = tie[1, 3]          # rounded to one decimal: ties at the maximum, inside the nucleus and at its boundary
    noise = torch.empty(B * K, V).exponential_(1, generator=g)
    return logits, noise.to(DEV).contiguous()


def scaled(raw, sets, target):
    """every (clip, codebook) pair of rows times one factor such that max |x / tau| of the mixed row is about ``target``"""
    x = mix_cpu(raw, sets)
    f = torch.stack([target * tau_of(s) / x[b].abs().amax(-1) for b, s in enumerate(sets)])     # (B, K)
    return (raw * torch.cat([f, f])[..., None]).contiguous()


def run_lp(logits, sets, noise, per_clip, seq=None, state=None, sp=None):
    """vaura_sample_logprobs -> (rc, tokens, logprobs); scalar form: every clip has the same set"""
    step = 3 if noise is None else 0
    any_cfg = any(s["cfg_scale"] > 1.0 for s in sets)
    rows = logits if any_cfg else logits[:B].contiguous()
    tok = torch.full((B, K), -1, dtype=torch.int32, device=DEV)
    lp = torch.full((B, K), 7.0, dtype=torch.float32, device=DEV)
    rec = records(sets) if per_clip else None
    sp = sp or (sampling(P(cfg_scale=2.0 if any_cfg else 1.0)) if per_clip else sampling(sets[0]))
    rc = L.lib().vaura_sample_logprobs(L.ptr(rows.to(DEV)), B, K, V, C.byref(sp), L.ptr(rec), L.ptr(noise), step, L.ptr(tok), L.ptr(seq),
                                       100 if seq is not None else 0, 0 if seq is None else seq.shape[-1], L.ptr(state), L.ptr(lp),
                                       stream())
    torch.cuda.synchronize()
    return rc, tok.cpu(), lp.cpu()


def run_plain(logits, sets, noise, per_clip):
    """the same call through vaura_sample (scalars) / vaura_sample_clips (records): the tokens LP must not change"""
    step = 3 if noise is None else 0
    any_cfg = any(s["cfg_scale"] > 1.0 for s in sets)
    rows = (logits if any_cfg else logits[:B].contiguous()).to(DEV)
    tok = torch.full((B, K), -1, dtype=torch.int32, device=DEV)
    if per_clip:
        sp = sampling(P(cfg_scale=2.0 if any_cfg else 1.0))
        rc = L.lib().vaura_sample_clips(L.ptr(rows), B, K, V, C.byref(sp), L.ptr(records(sets)), L.ptr(noise), step, L.ptr(tok), None, 0, 0,
                                        None, stream())
    else:
        sp = sampling(sets[0])
        rc = L.lib().vaura_sample(L.ptr(rows), B, K, V, C.byref(sp), L.ptr(noise), step, L.ptr(tok), stream())
    torch.cuda.synchronize()
    assert rc == 0
    return tok.cpu()


def check_op(case, logits, sets, noise, per_clip):
    rc, tok, lp = run_lp(logits, sets, noise, per_clip)
    assert rc == 0
    assert torch.equal(tok, run_plain(logits, sets, noise, per_clip)), case
    assert int(tok.min()) >= 0 and int(tok.max()) < V
    x = mix_cpu(logits, sets)
    worst = 0.0
    for b, s in enumerate(sets):
        z = x[b].double() / tau_of(s)
        ref = torch.log_softmax(z, -1).gather(-1, tok[b].long()[:, None])[:, 0]
        bar = op_bar(z.abs().amax(-1))
        err = (lp[b].double() - ref).abs()
        print(f"{case} clip {b}: A = {float(z.abs().max()):.1f}, max |error| = {float(err.max()):.3e}, bar >= {float(bar.min()):.3e}")
        worst = max(worst, float((err / bar).max()))
        assert bool((err <= bar).all()), (case, b, float((err / bar).max()))
    note(case, worst)


@pytest.mark.parametrize("philox", [False, True], ids=["recorded", "philox"])
@pytest.mark.parametrize("target", [5.0, 80.0])
@pytest.mark.parametrize("cfg", [1.0, 6.0])
@pytest.mark.parametrize("mode", list(MODES))
def test_op_scalar_parameters(raw_inputs, mode, cfg, target, philox):
    raw, noise = raw_inputs
    sets = [dict(MODES[mode], cfg_scale=cfg)] * B
    check_op(f"op scalar {mode} cfg {cfg:g} A~{target:g}", scaled(raw, sets, target), sets, None if philox else noise, False)


@pytest.mark.parametrize("philox", [False, True], ids=["recorded", "philox"])
@pytest.mark.parametrize("target", [5.0, 80.0])
@pytest.mark.parametrize("cfgs", [[1.0] * 3, [6.0] * 3, [6.0, 1.0, 3.0]], ids=["cfg1", "cfg6", "cfg_mixed"])
@pytest.mark.parametrize("order", [[0, 1, 2], [2, 0, 1]], ids=["gkp", "pgk"])
def test_op_per_clip_records_mixing_all_three_modes(raw_inputs, order, cfgs, target, philox):
    raw, noise = raw_inputs
    modes = list(MODES.values())
    sets = [dict(modes[i], cfg_scale=c) for i, c in zip(order, cfgs)]
    check_op(f"op per-clip {order} cfg {cfgs} A~{target:g}", scaled(raw, sets, target), sets, None if philox else noise, True)


@pytest.mark.parametrize("mode", list(MODES))
def test_op_tie_rows_keep_their_tokens(raw_inputs, mode):
    """the two tie rows of tests/golden/sampling.npz, unscaled (the ties are exact): clip 0 codebook 0 and clip 1 codebook 3"""
    raw, noise = raw_inputs
    assert int((raw[0, 0] == raw[0, 0, 5]).sum()) >= 11 and int((raw[1, 3] == raw[1, 3].max()).sum()) >= 1
    sets = [MODES[mode]] * B
    check_op(f"op tie rows {mode}", raw.contiguous(), sets, noise, False)


def test_op_inf_logit_gives_nan_and_the_status_bit(raw_inputs):
    raw, noise = raw_inputs
    sets = [dict(MODES["greedy"], cfg_scale=6.0), dict(MODES["topk250_t0.7"], cfg_scale=6.0), dict(MODES["topp0.9_t1.3"], cfg_scale=1.0)]
    bad = raw.clone()
    bad[0, 2, 17] = float("inf")          # clip 0, codebook 2, conditional row
    bad[B + 1, 4, 900] = float("-inf")    # clip 1, codebook 4, null row
    bad[2, 7, 0] = float("nan")           # clip 2, codebook 7
    S = K + 4
    seq = torch.full((B, K, S), -1, dtype=torch.int32, device=DEV)
    state = torch.zeros(8, dtype=torch.int32, device=DEV)
    state[0] = K                          # every codebook's slot at K + 1 is a valid timestep
    rc, tok, lp = run_lp(bad, sets, noise, True, seq=seq, state=state)
    assert rc == 0
    assert int(state[4]) & 1
    nan = torch.zeros(B, K, dtype=torch.bool)
    nan[0, 2] = nan[1, 4] = nan[2, 7] = True
    assert torch.equal(torch.isnan(lp), nan)
    assert int(tok.min()) >= 0 and int(tok.max()) < V and torch.equal(seq[:, :, K + 1].cpu(), tok)
    # the clean rows of the launch: what the clean launch gives, tokens and values
    rc, tok0, lp0 = run_lp(raw, sets, noise, True)
    assert torch.equal(tok[~nan], tok0[~nan]) and torch.equal(lp[~nan], lp0[~nan])


def test_op_probability_rows_are_refused(raw_inputs):
    raw, noise = raw_inputs
    sp = sampling(MODES["topk250_t0.7"])
    sp.input_is_probs = 1
    probs = torch.softmax(raw, -1)
    rc, _, lp = run_lp(probs, [MODES["topk250_t0.7"]] * B, noise, False, sp=sp)
    assert rc == -1 and bool((lp == 7.0).all())           # VAURA_ERR_ARG, nothing launched


# ---------------------------------------------------------------------------------------------------------------- c. reduction / selection
def test_sequence_logprob_and_revert_against_the_restatement():
    Bc, T = 3, 70                                          # more than 64 frames: a lane adds two of them
    rng = np.random.default_rng(3)
    for delays in (list(range(K)), [0, 2, 4, 6, 8, 10, 12, 14, 16], [0] * K):
        S = T + max(delays) + 1
        lp_seq = (-rng.random((Bc, K, S), dtype=np.float32) * 9).astype(np.float32)
        lp_seq[2, 4, 1 + delays[4] + 33] = np.nan          # one NaN inside clip 2
        d = L.delays_host(delays)
        src = torch.from_numpy(lp_seq).to(DEV)
        rev = torch.empty(Bc, K, T, dtype=torch.float32, device=DEV)
        assert L.lib().vaura_pattern_revert_delays_f32(L.ptr(src), L.ptr(rev), Bc, K, T, S, 0.0, d, stream()) == 0
        # the int revert's index map, on the bits
        bits = src.view(torch.int32)
        rev_i = torch.empty(Bc, K, T, dtype=torch.int32, device=DEV)
        assert L.lib().vaura_pattern_revert_delays(L.ptr(bits), L.ptr(rev_i), Bc, K, T, S, 0, d, stream()) == 0
        assert torch.equal(rev.view(torch.int32), rev_i)
        assert np.array_equal(rev.cpu().numpy().view(np.int32), R.revert(lp_seq, delays, T).view(np.int32))
        for t0 in (0, 4, 69):
            pcb = torch.empty(Bc, K, dtype=torch.float32, device=DEV)
            clip = torch.empty(Bc, dtype=torch.float32, device=DEV)
            assert L.lib().vaura_sequence_logprob(L.ptr(src), S, d, Bc, K, T, t0, L.ptr(pcb), L.ptr(clip), stream()) == 0
            want_pcb, want_clip = R.sequence_logprob(R.revert(lp_seq, delays, T), t0)
            assert np.array_equal(pcb.cpu().numpy(), want_pcb, equal_nan=True), (delays, t0)
            assert np.array_equal(clip.cpu().numpy(), want_clip, equal_nan=True), (delays, t0)
            assert np.isnan(want_clip[2]) == (t0 <= 33) and not np.isnan(want_clip[:2]).any()
    # a short sequence: the fill where it ends, and the default delays through NULL
    short = torch.arange(2 * K * 6, dtype=torch.float32, device=DEV).view(2, K, 6)
    out = torch.empty(2, K, 5, dtype=torch.float32, device=DEV)
    assert L.lib().vaura_pattern_revert_delays_f32(L.ptr(short), L.ptr(out), 2, K, 5, 6, -1.0, None, stream()) == 0
    assert np.array_equal(out.cpu().numpy(), R.revert(short.cpu().numpy(), list(range(K)), 5, fill=-1.0))


def test_select_candidates_rule_and_rows():
    Bc, N, T = 3, 4, 5
    nan = float("nan")
    scores = torch.tensor([[-2.0, -1.0, -1.0, -3.0],       # two equal best scores: the lower index wins
                           [nan, -5.0, nan, -4.0],         # a NaN among numbers never wins
                           [nan, nan, nan, nan]])          # every score NaN: candidate 0
    codes = torch.randint(0, V, (Bc * N, K, T), dtype=torch.int32, generator=torch.Generator().manual_seed(1))
    out = torch.full((Bc, K, T), -1, dtype=torch.int32, device=DEV)
    win = torch.full((Bc,), -1, dtype=torch.int32, device=DEV)
    assert L.lib().vaura_select_candidates(L.ptr(scores.to(DEV)), L.ptr(codes.to(DEV)), Bc, N, K, T, L.ptr(out), L.ptr(win), stream()) == 0
    torch.cuda.synchronize()
    assert win.tolist() == [1, 3, 0] == R.select_candidates(scores.numpy()).tolist()
    for b, j in enumerate(win.tolist()):
        assert torch.equal(out[b].cpu(), codes[b * N + j])


# ---------------------------------------------------------------------------------------------------------------- b. loop level
LB, T, TV = 2, 12, 32
STORAGES = ["h2", "h1", "f32"]
# the per-logit bar the decode path is held to against the oracle (tests/test_gpu_generate.py: 3e-5 on the tiny checkpoint, and
# 3e-5 x max(1, largest |logit|) where logits grow)
DELTA_REL = 3e-5
LOOP_MODES = {"greedy": P(False), "topk250_t0.8": P(True, 0.8, 250)}


@pytest.fixture(scope="module", params=STORAGES)
def engine(request, tiny_sampler_sd):
    return DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype=request.param, near_tie="off")


@pytest.fixture(scope="module")
def oracle(tiny_sampler_sd):
    return DecoderOracle(tiny_sampler_sd, 2, 16)


@pytest.fixture(scope="module")
def loop_feats():
    return synth.video_features(LB, tokens=TV, seed=31)


@pytest.fixture(scope="module")
def even_delays(golden):
    return [int(d) for d in golden("tiny_delays_even.npz")["delays"]]


_oracle_cache = {}


def oracle_logprobs(oracle, feats, codes, delays, s):
    """fp64 log-probability of every generated token from the CPU oracle's logits of the generated sequence: conditional and null rows,
    mixed in fp64, over tau, log_softmax, the chosen token -> (lp (B, K, T), A (B, K, T) = max |x / tau| of the row, largest |logit|)"""
    key = (codes.numpy().tobytes(), tuple(delays), tuple(sorted(s.items())))
    if key in _oracle_cache:
        return _oracle_cache[key]
    Bc, Kc, Tc = codes.shape
    S = Tc + max(delays) + 1
    seq = torch.full((Bc, Kc, S), V, dtype=torch.int64)
    for q, d in enumerate(delays):
        seq[:, q, 1 + d:1 + d + Tc] = codes[:, q]
    lc = oracle.forward_full(seq[..., :-1], feats).double()                        # position p decides step p + 1
    x = lc
    biggest = float(lc.abs().max())
    if s["cfg_scale"] > 1.0:
        lu = oracle.forward_full(seq[..., :-1], oracle.null_condition(feats)).double()
        biggest = max(biggest, float(lu.abs().max()))
        x = lu + (lc - lu) * s["cfg_scale"]
    z = x / tau_of(s)
    lsm = torch.log_softmax(z, -1)
    lp = torch.zeros(Bc, Kc, Tc, dtype=torch.float64)
    A = torch.zeros(Bc, Kc, Tc, dtype=torch.float64)
    for q, d in enumerate(delays):
        rows = lsm[:, q, d:d + Tc]                                                 # frame t <- position t + d_q
        lp[:, q] = rows.gather(-1, codes[:, q, :, None])[..., 0]
        A[:, q] = z[:, q, d:d + Tc].abs().amax(-1)
    _oracle_cache[key] = (lp, A, biggest)
    return _oracle_cache[key]


def loop_bar(A, s, biggest):
    """the op bar + (2 cfg - 1) 2 delta / tau: a logit of either branch arrives within delta of the oracle's, the mix multiplies that by
    up to 2 cfg - 1, and the chosen logit and the log-sum-exp each move by at most that much over tau"""
    delta = DELTA_REL * max(1.0, biggest)
    mixf = 2.0 * s["cfg_scale"] - 1.0 if s["cfg_scale"] > 1.0 else 1.0
    return op_bar(A) + mixf * 2.0 * delta / tau_of(s)


@pytest.mark.parametrize("with_prompt", [False, True], ids=["no_prompt", "prompt4"])
@pytest.mark.parametrize("cfg", [1.0, 3.0])
@pytest.mark.parametrize("mode", list(LOOP_MODES))
@pytest.mark.parametrize("pattern", ["default", "even"])
def test_loop_logprobs(engine, oracle, loop_feats, even_delays, pattern, mode, cfg, with_prompt):
    s = dict(LOOP_MODES[mode], cfg_scale=cfg)
    delays = None if pattern == "default" else even_delays
    dl = list(range(K)) if delays is None else delays
    Tp = 4 if with_prompt else 0
    prompt = torch.randint(0, V, (LB, K, Tp), generator=torch.Generator().manual_seed(9)) if Tp else None
    feats = loop_feats.to(DEV)
    kw = dict(prompt=prompt, seed=5, delays=delays, **s)
    plain = engine.generate_codes(feats, T, **kw).cpu()
    engine.check_status()
    got, lp = engine.generate_codes(feats, T, return_logprobs=True, **kw)
    engine.check_status()
    got = got.cpu()
    lp = {k: v.cpu() for k, v in lp.items()}
    assert torch.equal(got, plain)                                     # LP never changes a token ...
    eager, lp_eager = engine.generate_codes(feats, T, return_logprobs=True, use_graph=False, **kw)
    assert torch.equal(eager.cpu(), plain)                             # ... through the captured step graph or without it
    assert all(torch.equal(lp_eager[k].cpu().view(torch.int32), lp[k].view(torch.int32)) for k in lp)
    assert torch.equal(engine.generate_codes(feats, T, use_graph=False, **kw).cpu(), plain)
    if Tp:
        assert torch.equal(got[..., :Tp], prompt)
        assert bool((lp["logprobs"][..., :Tp] == 0).all())             # prompt frames: exactly 0
    assert lp["logprobs"].shape == (LB, K, T) and lp["per_codebook"].shape == (LB, K) and lp["score"].shape == (LB,)
    assert bool((lp["logprobs"][..., Tp:] <= 0).all()) and bool((lp["logprobs"][..., Tp:] < 0).any())
    # against the CPU oracle
    ref, A, biggest = oracle_logprobs(oracle, loop_feats, got, dl, s)
    bar = loop_bar(A, s, biggest)
    err = (lp["logprobs"].double() - ref).abs()[..., Tp:]
    ratio = float((err / bar[..., Tp:]).max())
    case = f"loop {engine.wdtype} {pattern} {mode} cfg {cfg:g} prompt {Tp}"
    print(f"{case}: max |error| = {float(err.max()):.3e}, smallest bar = {float(bar.min()):.3e}, largest |logit| = {biggest:.2f}")
    note(case, ratio)
    assert ratio <= 1.0, (case, ratio)
    # the reductions: bit-equal to the restatement applied to the returned values, and from run to run
    want_pcb, want_clip = R.sequence_logprob(lp["logprobs"].numpy(), Tp)
    assert np.array_equal(lp["per_codebook"].numpy().view(np.int32), want_pcb.view(np.int32))
    assert np.array_equal(lp["score"].numpy().view(np.int32), want_clip.view(np.int32))
    again, lp2 = engine.generate_codes(feats, T, return_logprobs=True, **kw)
    assert torch.equal(again.cpu(), got)
    assert all(torch.equal(lp2[k].cpu().view(torch.int32), lp[k].view(torch.int32)) for k in lp)


def test_logprobs_pointer_keys_the_step_graph(engine, loop_feats):
    feats = loop_feats.to(DEV)
    s = dict(LOOP_MODES["topk250_t0.8"], cfg_scale=3.0)
    engine.generate_codes(feats, T, seed=5, **s)
    off = engine._graph_key
    assert int(engine.dec.logprobs or 0) == 0
    engine.generate_codes(feats, T, seed=5, return_logprobs=True, **s)
    assert int(engine.dec.logprobs or 0) == engine.logprobs.data_ptr() and engine._graph_key != off
    engine.generate_codes(feats, T, seed=5, **s)
    assert int(engine.dec.logprobs or 0) == 0 and engine._graph_key == off
    engine.check_status()


# ---------------------------------------------------------------------------------------------------------------- d. candidates
N = 3


def _model(sd):
    from vaura_amd.model import VAURAModel
    cfg = synth.tiny_sampler(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VAURAModel(
            feature_extractor_config={"target": "vaura_amd.feature_extractor.MotionFormer"},
            audio_encoder_config={"target": "vaura_amd.codec.DacModelWrapper", "params": {"model_sr": 44100, "synthetic": True}},
            sampler_config={"target": "vaura_amd.sampler.Transformer", "params": cfg.yaml_params()},
            visual_bridge_config={"target": "torch.nn.Identity"},
            pattern_provider_config={"target": "vaura_amd.patterns.DelayedPatternProvider", "params": {"n_q": 9}},
            flatten_vis_feats=True, freeze_feature_extractor=True, noise_mode="philox")
    m.sampler.load_state_dict(sd, strict=True)
    m.sampler.audio_tokens_per_video_frame = 7
    return m.to(DEV)


@pytest.fixture(scope="module")
def model(tiny_sampler_sd):
    return _model(tiny_sampler_sd)


class CountingExtractor(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.shapes = []

    def forward(self, x, *a, **k):
        self.shapes.append(tuple(x.shape))
        return self.inner(x, *a, **k)


def first_argmax(scores):
    """CPU argmax with the first index winning ties (no NaN here)"""
    return torch.tensor([int(np.flatnonzero(r == r.max())[0]) for r in scores.numpy()])


@pytest.mark.parametrize("temp", [0.9, [0.7, 1.2]], ids=["scalar", "per_clip_temp"])
@pytest.mark.parametrize("noise_mode", ["philox", "torch_cpu"])
def test_candidates_are_a_repeated_batch_and_the_winner_is_decoded(model, monkeypatch, noise_mode, temp):
    frames = synth.video_features(LB, tokens=TV, seed=31).reshape(LB, 1, TV, 768).to(DEV)
    kw = dict(max_new_tokens=T, prompt_is_encoded=True, use_sampling=True, top_k=250, cfg_scale=3.0, return_sampled_indices=True)
    monkeypatch.setattr(model, "noise_mode", noise_mode)
    counter = CountingExtractor(model.visual_feature_extractor)
    monkeypatch.setattr(model, "visual_feature_extractor", counter)
    torch.manual_seed(123)                # recorded noise: the global CPU generator is the stream (one draw of B N K rows per step)
    r = model.generate(frames=frames, temp=temp, num_candidates=N, return_logprobs=True, **kw)
    assert counter.shapes == [(LB, 1, TV, 768)]                        # the extractor saw B clips, not B N
    # N candidates are exactly the repeated batch
    temp_rep = temp if not isinstance(temp, list) else [t for t in temp for _ in range(N)]
    torch.manual_seed(123)
    plain = model.generate(frames=frames.repeat_interleave(N, 0), temp=temp_rep, **kw)
    assert counter.shapes[-1] == (LB * N, 1, TV, 768)
    assert r["candidate_indices"].shape == (LB * N, K, T)
    assert torch.equal(r["candidate_indices"], plain["sampled_indices"])
    assert len({r["candidate_indices"][j].cpu().numpy().tobytes() for j in range(LB * N)}) == LB * N     # the takes do differ
    # selection: CPU argmax of the scores, first index on ties; the winners' rows; their audio only
    scores = r["candidate_scores"].cpu()
    assert scores.shape == (LB, N) and bool(torch.isfinite(scores).all())
    win = first_argmax(scores)
    assert torch.equal(r["selected_candidate"].cpu(), win)
    rows = torch.arange(LB) * N + win
    assert torch.equal(r["sampled_indices"].cpu(), r["candidate_indices"].cpu()[rows])
    assert torch.equal(r["sequence_logprob"].cpu(), scores[torch.arange(LB), win])
    assert r["logprobs"].shape == (LB, K, T) and r["logprob_per_codebook"].shape == (LB, K)
    assert r["generated_audio"].shape[0] == LB
    assert torch.equal(r["generated_audio"], model.audio_encoder.decode([(r["sampled_indices"], None)]))
    # every candidate, nothing selected
    torch.manual_seed(123)
    allc = model.generate(frames=frames, temp=temp, num_candidates=N, return_all_candidates=True, **kw)
    assert torch.equal(allc["candidate_indices"], r["candidate_indices"]) and torch.equal(allc["sampled_indices"], r["candidate_indices"])
    assert torch.equal(allc["candidate_scores"], r["candidate_scores"]) and "selected_candidate" not in allc
    assert allc["generated_audio"].shape[0] == LB * N
    assert torch.equal(allc["generated_audio"], plain["generated_audio"])


def test_defaults_return_what_they_always_did(model):
    frames = synth.video_features(LB, tokens=TV, seed=31).reshape(LB, 1, TV, 768).to(DEV)
    r = model.generate(frames=frames, max_new_tokens=T, prompt_is_encoded=True, top_k=250, cfg_scale=3.0, return_sampled_indices=True)
    assert set(r) == {"generated_audio", "s_attn_weights", "mha_attn_weights", "sampled_indices"}
    toks = model.generate_tokens(frames=frames, max_new_tokens=T, prompt_is_encoded=True, top_k=250, cfg_scale=3.0)
    assert isinstance(toks, torch.Tensor) and torch.equal(toks, r["sampled_indices"])
    # return_logprobs alone: the same tokens, and remove_prompts slices the values like the tokens
    prompt = torch.randint(0, V, (LB, K, 4), generator=torch.Generator().manual_seed(9)).to(DEV)
    kw = dict(frames=frames, audio=prompt, max_new_tokens=T, prompt_is_encoded=True, top_k=250, cfg_scale=3.0)
    full = model.generate_tokens(return_logprobs=True, **kw)
    cut = model.generate_tokens(return_logprobs=True, remove_prompts=True, **kw)
    assert torch.equal(full["tokens"], model.generate_tokens(**kw))
    assert full["logprobs"].shape == (LB, K, T) and cut["logprobs"].shape == (LB, K, T - 4) and cut["tokens"].shape == (LB, K, T - 4)
    assert torch.equal(cut["logprobs"], full["logprobs"][..., 4:]) and bool((full["logprobs"][..., :4] == 0).all())
    assert torch.equal(cut["sequence_logprob"], full["sequence_logprob"])      # prompt frames are not counted either way
