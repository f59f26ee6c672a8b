"""Per-clip sampling parameters in one batched call: csrc/step.hip sample_kernel<true>, vaura_decoder.clip_sampling /
vaura_sample_clips, DecoderEngine.generate_codes(temp=[...], ...), VAURAModel.generate, longform.generate_long.

Every comparison is torch.equal: a clip of a per-clip call is decoded with the arithmetic of the scalar call that carries its
parameters — the parameters never enter a floating-point sum differently, so there is no tolerance to choose."""
import ctypes as C
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from vaura_amd import _lib as L
from vaura_amd import clip_params, synth
from vaura_amd.engine import DecoderEngine

DEV = "cuda:0"
B, K, V = 4, 9, 1024
T, TV = 12, 32         # (the CFG null embedding of the checkpoint has 32 tokens: a doubled batch needs Tv = 32)
NAMES = clip_params.NAMES


def P(use_sampling=False, temp=1.0, top_k=0, top_p=0.0, cfg_scale=1.0):
    return dict(use_sampling=use_sampling, temp=temp, top_k=top_k, top_p=top_p, cfg_scale=cfg_scale)


def columns(sets):
    """[one dict per clip] -> the keyword arguments of a per-clip call"""
    return {n: [s[n] for s in sets] for n in NAMES}


def records(sets):
    p = clip_params.resolve(len(sets), **columns(sets))
    return torch.frombuffer(bytearray(clip_params.pack_records(p)), dtype=torch.int32).view(len(sets), 8).to(DEV)


def sampling(s, tie_eps=0.0, seed=11):
    return L.Sampling(int(bool(s["use_sampling"])), float(s["temp"]), int(s["top_k"]), float(s["top_p"]), float(s["cfg_scale"]), seed, 0, 0,
                      float(tie_eps))


def stream():
    return L.current_stream(torch.device(DEV))


# ---------------------------------------------------------------------------------------------------------------- 1. op level
OP_GROUPS = [
    [P(False, cfg_scale=1.0), P(True, 0.0, 50, cfg_scale=3.0), P(True, 0.7, cfg_scale=6.0), P(True, 1.3, 1, cfg_scale=1.0)],
    [P(True, 1.0, 128, cfg_scale=6.0), P(True, 0.7, 250, cfg_scale=3.0), P(True, 1.3, 1024, cfg_scale=1.0), P(True, 1.0, 128, 0.3, cfg_scale=6.0)],
    [P(True, 0.7, 250, 0.95, cfg_scale=1.0), P(False, cfg_scale=6.0), P(True, 1.3, cfg_scale=1.0), P(True, 1.0, 250, cfg_scale=6.0)],
    [P(True, 1.3, 250, 0.3, cfg_scale=3.0), P(True, 0.7, 1024, cfg_scale=6.0), P(True, 0.7, 1, cfg_scale=3.0), P(True, 1.0, 128, 0.95, cfg_scale=1.0)],
]


@pytest.fixture(scope="module")
def op_inputs():
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(2 * B, K, V, generator=g) * 3
    # exact duplicates: the k-th largest value of a top-k cut and the boundary of the nucleus fall inside runs of equal probabilities
    logits[0::2, :, 512:] = logits[0::2, :, :512]
    logits[1, :, 100:400] = logits[1, :, 7:8]
    logits[5, :, 3::2] = 1.5
    noise = torch.empty(B * K, V).exponential_(1, generator=g)
    return logits.to(DEV).contiguous(), noise.to(DEV).contiguous()


def scalar_sample(logits, noise, s):
    step = 3 if noise is None else 0      # an explicit noise tensor holds one step of draws; Philox is keyed by the step index
    out = torch.full((B, K), -1, dtype=torch.int32, device=DEV)
    rows = logits if s["cfg_scale"] > 1.0 else logits[:B].contiguous()       # cfg <= 1: the call is made WITHOUT the null rows
    sp = sampling(s)
    L.check(L.lib().vaura_sample(L.ptr(rows), B, K, V, C.byref(sp), L.ptr(noise), step, L.ptr(out), stream()), "vaura_sample")
    return out


def clips_sample(logits, noise, sets, sp=None, seq=None, state=None):
    step = 3 if noise is None else 0
    out = torch.full((B, K), -1, dtype=torch.int32, device=DEV)
    rec = records(sets)
    sp = sp or sampling(P(cfg_scale=2.0 if any(s["cfg_scale"] > 1.0 for s in sets) else 1.0))
    rc = L.lib().vaura_sample_clips(L.ptr(logits), B, K, V, C.byref(sp), L.ptr(rec), L.ptr(noise), step, L.ptr(out), L.ptr(seq),
                                    100 if seq is not None else 0, 0 if seq is None else seq.shape[-1], L.ptr(state), stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("philox", [False, True])
@pytest.mark.parametrize("group", range(len(OP_GROUPS)))
def test_op_per_clip_equals_the_scalar_call_of_each_clip(op_inputs, group, philox):
    logits, noise = op_inputs
    noise = None if philox else noise
    sets = OP_GROUPS[group]
    rc, got = clips_sample(logits, noise, sets)
    assert rc == 0
    assert int(got.min()) >= 0 and int(got.max()) < V
    for b, s in enumerate(sets):
        ref = scalar_sample(logits, noise, s)
        assert torch.equal(got[b], ref[b]), (group, b, s)


def test_op_a_clip_at_cfg_1_does_not_read_its_null_row(op_inputs):
    """rows doubled, clip 0 and 3 at cfg 1: garbage in THEIR null rows changes nothing (and would, through lu + (x - lu) * 1)."""
    logits, noise = op_inputs
    sets = OP_GROUPS[0]
    _, ref = clips_sample(logits, noise, sets)
    bad = logits.clone()
    bad[B + 0] = float("nan")
    bad[B + 3] = 1e30
    _, got = clips_sample(bad, noise, sets)
    assert torch.equal(got, ref)


# ---------------------------------------------------------------------------------------------------------------- 2. / 3. loop
SETS = [P(False), P(True, 0.7, 128), P(True, 1.3, 250, 0.3), P(True, 1.0)]
CFG_UP = [2.0, 4.0, 6.0, 6.0]
CFG_MIXED = [1.0, 1.0, 6.0, 6.0]
ENGINE_KINDS = ["h1", "h2", "f32"]


def with_cfg(sets, cfgs):
    return [dict(s, cfg_scale=c) for s, c in zip(sets, cfgs)]


@pytest.fixture(scope="module")
def loop_inputs():
    feats = synth.video_features(B, tokens=TV, seed=31).to(DEV)
    noise = synth.exp_noise(T + K - 1, B * K, V, 77).to(DEV)
    return feats, noise


@pytest.fixture(scope="module", params=ENGINE_KINDS)
def engine(request, tiny_sampler_sd):
    return DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype=request.param, near_tie="off")


_scalar_refs = {}


def scalar_runs(eng, loop_inputs, sets):
    """clip i of the scalar-parameter run of the SAME batch with clip i's set — computed once per (storage, sets)"""
    key = (eng.wdtype, tuple(tuple(s.items()) for s in sets))
    if key not in _scalar_refs:
        feats, noise = loop_inputs
        rows = []
        for i, s in enumerate(sets):
            out = eng.generate_codes(feats, T, noise=noise, **s)
            eng.check_status()
            rows.append(out[i].cpu())
        _scalar_refs[key] = torch.stack(rows)
    return _scalar_refs[key]


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("cfgs", [[1.0] * 4, CFG_UP], ids=["cfg1", "cfg_up"])
def test_loop_each_clip_equals_its_scalar_run(engine, loop_inputs, cfgs, use_graph):
    feats, noise = loop_inputs
    sets = with_cfg(SETS, cfgs)
    ref = scalar_runs(engine, loop_inputs, sets)
    got = engine.generate_codes(feats, T, noise=noise, use_graph=use_graph, **columns(sets)).cpu()
    engine.check_status()
    assert int(got.min()) >= 0 and int(got.max()) < V
    for i in range(B):
        assert torch.equal(got[i], ref[i]), (i, sets[i])
    assert not torch.equal(got[1], engine.generate_codes(feats, T, noise=noise, **sets[0])[1].cpu())   # the sets do differ in effect


def test_loop_mixed_guidance_clips_are_independent(engine, loop_inputs):
    feats, noise = loop_inputs
    sets = with_cfg(SETS, CFG_MIXED)
    base = engine.generate_codes(feats, T, noise=noise, **columns(sets)).cpu()
    engine.check_status()
    # the cfg-6 clips: their scalar runs of check 2 (same rows, same row count)
    ref = scalar_runs(engine, loop_inputs, with_cfg(SETS, CFG_UP))
    assert torch.equal(base[2], ref[2]) and torch.equal(base[3], ref[3])
    # other clips' parameters do not reach a clip: change {0, 2}, then {1, 3}
    other = [P(True, 0.9, 40, cfg_scale=3.0), P(False, cfg_scale=5.0), P(False, cfg_scale=1.0), P(True, 0.8, 0, 0.6, cfg_scale=1.0)]
    alt = [other[0], sets[1], other[2], sets[3]]
    got = engine.generate_codes(feats, T, noise=noise, **columns(alt)).cpu()
    assert torch.equal(got[1], base[1]) and torch.equal(got[3], base[3])
    assert not torch.equal(got[0], base[0]) and not torch.equal(got[2], base[2])
    alt = [sets[0], other[1], sets[2], other[3]]
    got = engine.generate_codes(feats, T, noise=noise, **columns(alt)).cpu()
    assert torch.equal(got[0], base[0]) and torch.equal(got[2], base[2])
    assert not torch.equal(got[1], base[1]) and not torch.equal(got[3], base[3])
    engine.check_status()


# ---------------------------------------------------------------------------------------------------------------- 4. graph reuse
def test_two_per_clip_calls_replay_one_graph(tiny_sampler_sd, loop_inputs):
    feats, noise = loop_inputs
    a, b = with_cfg(SETS, CFG_UP), with_cfg(SETS[::-1], [6.0, 1.0, 3.0, 2.0])
    eng = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype="h2")
    first = eng.generate_codes(feats, T, noise=noise, **columns(a)).cpu()
    handle, key = eng._graph.value, eng._graph_key
    assert handle
    second = eng.generate_codes(feats, T, noise=noise, **columns(b)).cpu()
    assert eng._graph.value == handle and eng._graph_key == key          # the values are not in the key: the same captured step
    fresh = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype="h2")
    assert torch.equal(second, fresh.generate_codes(feats, T, noise=noise, **columns(b)).cpu())
    assert not torch.equal(first, second)
    # ... and a scalar call in between is still the scalar call (NULL records), the per-clip call after it still right
    sc = eng.generate_codes(feats, T, noise=noise, **a[2]).cpu()
    assert int(eng.dec.clip_sampling or 0) == 0
    assert torch.equal(sc, fresh.generate_codes(feats, T, noise=noise, **a[2]).cpu())
    assert torch.equal(eng.generate_codes(feats, T, noise=noise, **columns(a)).cpu(), first)
    eng.check_status(); fresh.check_status()


# ---------------------------------------------------------------------------------------------------------------- 5. status
@pytest.mark.parametrize("s", [P(False, cfg_scale=6.0), P(True, 1.0, 250, cfg_scale=6.0), P(True, 0.8, 40), P(True, 1.0, 0, 0.7)])
def test_near_tie_counter_of_a_uniform_per_clip_call_equals_the_scalar_call(tiny_sampler_sd, loop_inputs, s):
    feats, noise = loop_inputs
    eng = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype="h2", near_tie="report", near_tie_eps=1e-2)
    ref = eng.generate_codes(feats, T, noise=noise, **s).cpu()
    eng.check_status()
    want = eng.last_near_ties
    got = eng.generate_codes(feats, T, noise=noise, **columns([s] * B)).cpu()
    eng.check_status()
    assert torch.equal(got, ref)
    assert eng.last_near_ties == want
    if not s["use_sampling"]:
        assert want[0] > 0                # (a bound this wide flags greedy decisions of the tiny model: the counter is live)


def test_near_tie_rerun_hands_the_per_clip_values_to_the_exact_fp32_twin(tiny_sampler_sd, loop_inputs):
    """near_tie="rerun" with a bound wide enough to flag the call: the result is the exact-fp32 engine's, run with the same lists."""
    feats, noise = loop_inputs
    kw = columns(with_cfg(SETS, CFG_MIXED))
    eng = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype="h2", near_tie="rerun", near_tie_eps=1e-2)
    got = eng.generate_codes_checked(feats, T, noise=noise, **kw).cpu()
    assert eng.near_tie_reruns == 1
    f32 = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype="f32")
    ref = f32.generate_codes(feats, T, noise=noise, **kw).cpu()
    f32.check_status()
    assert torch.equal(got, ref)
    assert int(eng._range_twin.dec.clip_sampling or 0) == eng._range_twin.clip_params.data_ptr()


def _stateful(pos=K):
    S = K + 4
    seq = torch.full((B, K, S), -1, dtype=torch.int32, device=DEV)
    state = torch.zeros(8, dtype=torch.int32, device=DEV)
    state[0] = pos          # every codebook's slot at this position is a valid timestep (t = pos - k >= 0): every decision is used
    return seq, state


@pytest.mark.parametrize("margin,flagged_clips", [(0.035, 1), (0.03, 2), (0.015, 4), (0.3, 0)])
def test_op_near_tie_flag_follows_the_clips_own_cfg_factor(margin, flagged_clips):
    """Greedy rows with top-1 - top-2 = margin, |logit| max 10, null rows 0, tie_eps 1e-3.  The mixed margin is cfg x margin, the bound
    2 tie_eps (2 cfg - 1) 10 (factor 1 at cfg 1): cfg 1 -> 0.02, cfg 3 -> margin 3 m against 0.10, cfg 6 -> 6 m against 0.22.
    m = 0.035: only cfg 6 (0.21 < 0.22; 0.105 > 0.10); m = 0.03: cfg 3 and 6; m = 0.015: all four; m = 0.3: none."""
    cfgs = [1.0, 3.0, 6.0, 1.0]
    logits = torch.zeros(2 * B, K, V)
    logits[:B, :, 5] = 10.0
    logits[:B, :, 9] = 10.0 - margin
    seq, state = _stateful()
    sp = sampling(P(cfg_scale=2.0), tie_eps=1e-3)
    rc, _ = clips_sample(logits.to(DEV), None, [P(cfg_scale=c) for c in cfgs], sp=sp, seq=seq, state=state)
    assert rc == 0
    st = state.tolist()
    assert st[0] == K + 1 and st[1] == 0 and st[2] == 1
    assert st[6] == flagged_clips * K and bool(st[4] & 4) == (flagged_clips > 0)
    assert bool((seq[:, :, K + 1] == 5).all()) and bool((seq[:, :, :K + 1] == -1).all())


def test_op_non_finite_logit_raises_the_status_bit_and_yields_valid_ids(op_inputs):
    logits, noise = op_inputs
    sets = OP_GROUPS[1]
    bad = logits.clone()
    bad[1, 2, 17] = float("nan")          # clip 1 (top-k 250, cfg 3), codebook 2
    bad[B + 3, 4, 900] = float("inf")     # clip 3's null row (top-p, cfg 6)
    seq, state = _stateful()
    rc, tok = clips_sample(bad, noise, sets, seq=seq, state=state)
    assert rc == 0
    assert int(state[4]) & 1
    assert int(tok.min()) >= 0 and int(tok.max()) < V
    assert torch.equal(seq[:, :, K + 1], tok)
    # the clean rows of the same launch: what the clean launch gives
    _, clean = clips_sample(logits, noise, sets)
    keep = torch.ones(B, K, dtype=torch.bool)
    keep[1, 2] = keep[3, 4] = False
    assert torch.equal(tok.cpu()[keep], clean.cpu()[keep])


# ---------------------------------------------------------------------------------------------------------------- 6. surface
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


def test_model_generate_takes_lists_and_tensors(model):
    frames = synth.video_features(B, tokens=TV, seed=31).reshape(B, 1, TV, 768).to(DEV)
    sets = with_cfg(SETS, CFG_MIXED)
    kw = columns(sets)
    r = model.generate(frames=frames, max_new_tokens=T, return_sampled_indices=True, prompt_is_encoded=True, check=True,
                       use_sampling=kw["use_sampling"], temp=kw["temp"], top_k=torch.tensor(kw["top_k"]), top_p=tuple(kw["top_p"]),
                       cfg_scale=torch.tensor(kw["cfg_scale"], device=DEV))
    eng = model.sampler.engine()
    ref = eng.generate_codes(frames.reshape(B, TV, 768), T, seed=model.seed, clip_base=model.clip_base, tokens_per_frame=7, **kw)
    eng.check_status()
    assert torch.equal(r["sampled_indices"], ref)
    assert r["generated_audio"].shape == (B, 1, T * 512)
    # a scalar among them is broadcast
    r2 = model.generate_tokens(frames=frames, max_new_tokens=T, prompt_is_encoded=True, use_sampling=True, temp=kw["temp"], top_k=128,
                               top_p=0.0, cfg_scale=1.0)
    ref2 = eng.generate_codes(frames.reshape(B, TV, 768), T, seed=model.seed, tokens_per_frame=7, use_sampling=[True] * B,
                              temp=kw["temp"], top_k=[128] * B, top_p=[0.0] * B, cfg_scale=[1.0] * B)
    assert torch.equal(r2, ref2)


def test_generate_long_with_per_clip_values_over_two_chunks(model):
    from vaura_amd import longform
    Bl, S_seg, t_seg = 2, 4, 4
    feats = synth.video_features(Bl, tokens=S_seg * t_seg, seed=71).reshape(Bl, S_seg, t_seg, 768).to(DEV)
    sched = longform.chunk_schedule(0.40, 0.30, 0.10, 440)
    assert len(sched) == 2 and all(hi - lo == 8 for lo, hi in (c["positions"] for c in sched))     # 8 segments x 4 = 32 condition tokens
    kw = dict(stride=0.10, model_max_duration=0.30, vfps=440)
    sets = [P(False, cfg_scale=1.0), P(True, 0.8, 50, cfg_scale=3.0)]
    got = longform.generate_long(model, feats, 0.40, **kw, **columns(sets))["sampled_indices"]
    assert got.shape == (Bl, K, int(0.40 * longform.COMPRESSION_MODEL_FRAME_RATE))
    # clip 1: the scalar call with its values (same rows: cfg 3 doubles them too)
    ref1 = longform.generate_long(model, feats, 0.40, **kw, **sets[1])["sampled_indices"]
    assert torch.equal(got[1], ref1[1])
    # clip 0 (cfg 1 among doubled rows): independent of what clip 1 is given
    other = longform.generate_long(model, feats, 0.40, **kw, **columns([sets[0], P(False, cfg_scale=6.0)]))["sampled_indices"]
    assert torch.equal(got[0], other[0]) and not torch.equal(got[1], other[1])


def test_refusals(model, tiny_sampler_sd, op_inputs):
    frames = synth.video_features(B, tokens=TV, seed=31).reshape(B, 1, TV, 768).to(DEV)
    with pytest.raises(L.VauraHipError, match="3 values for a batch of 4"):
        model.generate(frames=frames, max_new_tokens=T, prompt_is_encoded=True, temp=[1.0, 0.7, 1.3])
    with pytest.raises(L.VauraHipError, match="temp has 4"):
        model.generate_tokens(frames=frames, max_new_tokens=T, prompt_is_encoded=True, temp=[1.0] * 4, cfg_scale=[1.0] * 3)
    eng = model.sampler.engine()
    feats = frames.reshape(B, TV, 768)
    with pytest.raises(L.VauraHipError, match="top_k = 2000 of clip 2"):
        eng.generate_codes(feats, T, use_sampling=True, top_k=[10, 1024, 2000, 0])
    eng.generate_codes(feats, T, use_sampling=[True, True, False, True], top_k=[10, 1024, 2000, 0], top_p=[0, 0, 0, 0.0])   # unused: fine
    eng.check_status()
    eng.prepare(B, T, TV, False)
    with pytest.raises(L.VauraHipError, match="null-condition rows"):
        eng._sampling(False, 1.0, 0, 0.0, [1.0, 6.0, 1.0, 1.0], 0, 0)
    # C ABI
    logits, noise = op_inputs
    sets = [P(cfg_scale=1.0), P(cfg_scale=6.0), P(), P()]
    rc, _ = clips_sample(logits, noise, sets, sp=sampling(P(cfg_scale=1.0)))
    assert rc == -1                       # a record with cfg_scale > 1, no null rows declared
    sp = sampling(P(cfg_scale=1.0))
    sp.input_is_probs = 1
    rc, _ = clips_sample(logits, noise, [P()] * B, sp=sp)
    assert rc == -1
    eng._sampling(False, 1.0, 0, 0.0, [1.0] * B, 0, 0)
    eng.clip_params.copy_(records(sets))  # records the engine would have refused, behind its back: the library refuses them too
    sp = sampling(P(cfg_scale=1.0))
    assert L.lib().vaura_decode_step(C.byref(eng.dec), C.byref(sp), 1, stream()) == -1
    handle = C.c_void_p()
    assert L.lib().vaura_step_graph_build(C.byref(eng.dec), C.byref(sp), stream(), C.byref(handle)) == -1
    assert L.lib().vaura_generate_loop(C.byref(eng.dec), C.byref(sp), 0, 1, None, stream()) == -1
    torch.cuda.synchronize()
