"""Delay patterns other than the default 0..K-1 on the device (codebook_patterns.py:374-419; configs/modules/codebook_patterns/
parallel_9cbs.yaml): pattern build / revert kernels, the decode loop's valid-slot fix-up under any delays, and the plugin surface,
against goldens the reference itself produced (tests/golden/make_golden_patterns.py)."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vaura_amd import _lib as L
from vaura_amd import synth
from vaura_amd.engine import DecoderEngine
from vaura_amd.patterns import DelayedPatternProvider, ParallelPatternProvider

DEV = "cuda:0"
PARALLEL = [0] * 9
EVEN = list(range(0, 18, 2))
# Two decisions of the parallel goldens sit close to the plane storages' arithmetic noise (the engine's near-tie detector band,
# engine.NEAR_TIE_EPS): greedy cfg 1, smallest top-1 - top-2 margin 1.36e-5 (band ~1.1e-5); cfg 6 / top-k 250 sampled, smallest
# relative margin of argmax(p / q) 6.0e-5 (band ~1.2e-4).  As for the delayed goldens' two literal ties (parity_helpers
# assert_tokens_or_recorded_near_tie), tokens must equal the reference's up to a first difference that sits on a step whose recorded
# margin is below these bounds; the report records which happened.
NEAR_TIE_GREEDY, NEAR_TIE_SAMPLED = 2e-5, 1.5e-4


def _ref(g, k):
    return torch.from_numpy(g[k].astype(np.int64))


def _assert_tokens(report, golden, storage, what, tok, ref, delays, margins, tol, first_step):
    """Token parity under a delay pattern: frame t of codebook k is decided at sequence step t + 1 + d_k, by pass step - first_step."""
    B, K, T = ref.shape
    steps = torch.arange(T)[None, :] + 1 + torch.tensor(delays)[:, None]
    e = {"golden": golden, "storage": storage, "what": what, "tokens_equal": bool(torch.equal(tok, ref)),
         "token_agreement": float((tok == ref).float().mean()), "reference_min_margin": float(margins.min()), "near_tie_tolerance": tol}
    if not e["tokens_equal"]:
        bad = tok != ref
        s = int(steps[None].expand_as(bad)[bad].min())
        at = bad & (steps[None] == s)
        m = min(float(margins[s - first_step, b, k]) for b, k in zip(*torch.nonzero(at.any(-1), as_tuple=True)))
        e.update(first_diff_step=s, reference_margin_there=m)
        before = (steps < s)[None].expand_as(ref)
        assert torch.equal(tok[before], ref[before]), e
        assert m < tol, (f"{golden} [{storage}] {what}: first differs at step {s} where the reference's margin is {m} >= {tol}")
    report.entries.append(e)
    return e


# ------------------------------------------------------------------------------------- build / revert kernels
@pytest.mark.parametrize("name", ["parallel", "d011", "even", "unit"])
def test_device_build_and_revert_match_reference(golden, name):
    g = golden("patterns_delays.npz")
    delays = [int(x) for x in g[name + "_delays"]]
    prov = ParallelPatternProvider(9) if name == "parallel" else DelayedPatternProvider(9, delays=delays)
    for T, Tp in ((4, 0), (20, 8), (55, 0), (220, 0), (221, 166)):
        k = f"{name}_T{T}_p{Tp}"
        pat = prov.get_pattern(T)
        seq, idx, mask = pat.build_pattern_sequence(_ref(g, k + "_codes").to(DEV), 1024)
        assert torch.equal(seq.cpu(), _ref(g, k + "_seq")), k
        assert np.array_equal(idx.cpu().numpy(), g[k + "_idx"]) and np.array_equal(mask.cpu().numpy(), g[k + "_mask"])
        rev, _, _ = pat.revert_pattern_sequence(_ref(g, k + "_filled").to(DEV), special_token=-1)
        assert torch.equal(rev.cpu(), _ref(g, k + "_rev")), k


# ------------------------------------------------------------------------------------- full depth, parallel pattern
def _full_model(sd, weight_dtype, pattern="vaura_amd.patterns.ParallelPatternProvider"):
    from vaura_amd.model import VAURAModel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VAURAModel(
            feature_extractor_config={"target": "vaura_amd.feature_extractor.MotionFormer"},
            audio_encoder_config={"target": "vaura_amd.codec.DacModelWrapper", "params": {"model_sr": 44100, "synthetic": True}},
            sampler_config={"target": "vaura_amd.sampler.Transformer",
                            "params": dict(synth.FULL_SAMPLER.yaml_params(), weight_dtype=weight_dtype)},
            visual_bridge_config={"target": "torch.nn.Identity"},
            pattern_provider_config={"target": pattern, "params": {"n_q": 9}},
            flatten_vis_feats=True, freeze_feature_extractor=True, noise_mode="torch_cpu")
    m.sampler.load_state_dict(sd, strict=True)
    m.sampler.audio_tokens_per_video_frame = 7
    return m.to(DEV)


def _kept_logits(eng, g, feats, cfg_scale):
    """Last-position logits of the reference's passes at the golden's kept steps, recomputed teacher-forced on the golden's own
    parallel-pattern sequence (step 0 special, step s = frame s - 1): (len(keep), rows, K, V)."""
    tok = _ref(g, "tokens")
    B = tok.shape[0]
    seq = torch.cat([torch.full((B, 9, 1), 1024, dtype=torch.long), tok], dim=-1)
    keep = [int(x) for x in g["logits_steps"]]
    if cfg_scale > 1.0:
        seq = torch.cat([seq, seq], 0)
        feats = torch.cat([feats, torch.zeros_like(feats) + eng.uncond], 0)
    lg = eng.logits_all_positions(seq[:, :, :max(keep)].to(DEV), feats).cpu()
    return torch.stack([lg[:, :, L - 1] for L in keep])


@pytest.mark.parametrize("weight_dtype", ["f32", "auto"])
def test_full_depth_parallel_generate_matches_reference(golden, full_sampler_sd_raw, parity_report, weight_dtype):
    """A model trained with parallel_9cbs.yaml, decoded through VAURAModel.generate (24 layers, un-rounded checkpoint, B=2, T=220:
    221 sequence steps, 220 sampled): tokens equal the reference's own generate() with ParallelPatternProvider(9) — greedy cfg 1,
    and cfg 6 / top-k 250 with the reference's noise stream — and the logits of its passes at the kept steps agree to the existing
    goldens' bars.  Before delay patterns were supported this decoded the delayed layout instead (other tokens, no error)."""
    m = _full_model(full_sampler_sd_raw, weight_dtype)
    eng = m.sampler.engine()
    storage = eng.wdtype
    assert storage == ("f32" if weight_dtype == "f32" else "h2")
    gg = golden("full_parallel_greedy_raw_B2_T220.npz")
    gs = golden("full_parallel_topk250_cfg6_raw_B2_T220.npz")
    assert [int(x) for x in gg["delays"]] == PARALLEL
    frames = synth.video_features(2, seed=int(gg["feat_seed"])).reshape(2, 4, 8, 768).to(DEV)
    r = m.generate(frames=frames, audio=None, max_new_tokens=220, return_sampled_indices=True, use_sampling=False,
                   prompt_is_encoded=True, cfg_scale=1.0, check=True)
    assert eng.S == 221 and eng.delays == tuple(PARALLEL)
    _assert_tokens(parity_report, "full_parallel_greedy_raw_B2_T220", storage, "parallel pattern, greedy cfg 1, B=2 (VAURAModel.generate)",
                   r["sampled_indices"].cpu(), _ref(gg, "tokens"), PARALLEL, gg["margins"], NEAR_TIE_GREEDY, 1)
    torch.manual_seed(int(gs["noise_seed"]))
    r = m.generate(frames=frames, audio=None, max_new_tokens=220, return_sampled_indices=True, use_sampling=True, temp=1.0,
                   top_k=int(gs["top_k"]), top_p=0.0, prompt_is_encoded=True, cfg_scale=float(gs["cfg_scale"]))
    _assert_tokens(parity_report, "full_parallel_topk250_cfg6_raw_B2_T220", storage,
                   "parallel pattern, cfg 6 / top-k 250 sampled, B=2 (VAURAModel.generate)", r["sampled_indices"].cpu(), _ref(gs, "tokens"),
                   PARALLEL, gs["margins"], NEAR_TIE_SAMPLED, 1)
    assert r["generated_audio"].shape == (2, 1, 220 * 512)
    feats = frames.reshape(2, 32, 768)
    for g, cfg_scale in ((gg, 1.0), (gs, 6.0)):
        lg = _kept_logits(eng, g, feats, cfg_scale)
        err = (lg - torch.from_numpy(g["logits"])).abs().amax(dim=(1, 2, 3))
        print(f"{weight_dtype} cfg {cfg_scale}: max-abs logit error per kept step {[f'{x:.2e}' for x in err.tolist()]}")
        assert float(err[0]) < 3e-5 and float(err.max()) < 1e-4, err
    del m, eng
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def full_engine(full_sampler_sd_raw):
    eng = DecoderEngine(synth.FULL_SAMPLER, full_sampler_sd_raw, DEV)
    assert eng.wdtype == "h2"
    yield eng
    del eng
    torch.cuda.empty_cache()


def test_explicit_default_delays_are_bit_identical_at_the_headline_shape(full_engine):
    """configs[1]'s shape (8 clips, cfg 6 -> 16 rows, top-k 250 sampled): delays 0..8 passed explicitly (the descriptor's delay
    field, has_pattern_delays = 1) give the same tokens and the same last-step logits, bit for bit, as delays=None."""
    eng = full_engine
    feats = synth.video_features(8, seed=0).to(DEV)
    nz = synth.exp_noise(228, 72, 1024, 4321)
    kw = dict(use_sampling=True, temp=1.0, top_k=250, cfg_scale=6.0, noise=nz)
    a = eng.generate_codes(feats, 220, **kw).clone()
    la = eng.ws_logits.clone()
    eng.check_status()
    assert eng.delays is None and eng.dec.has_pattern_delays == 0
    b = eng.generate_codes(feats, 220, delays=list(range(9)), **kw).clone()
    lb = eng.ws_logits.clone()
    eng.check_status()
    assert eng.delays == tuple(range(9)) and eng.dec.has_pattern_delays == 1
    assert torch.equal(a, b) and torch.equal(la, lb)


def test_one_engine_alternating_patterns_keeps_each_call_exact(golden, full_engine, parity_report):
    """Delayed, parallel, delayed, parallel on ONE engine with the captured step graph: the shape key (S, delays) and with it the
    graph key change with the pattern, so every call decodes its own layout (a stale graph would bake in the other S / delays)."""
    eng = full_engine
    gd = golden("full_greedy_raw_B2_T220.npz")
    gp = golden("full_parallel_greedy_raw_B2_T220.npz")
    feats = synth.video_features(2, seed=int(gd["feat_seed"])).to(DEV)
    for i in range(2):
        tok = eng.generate_codes(feats, 220).cpu()
        eng.check_status()
        assert eng.S == 229
        assert torch.equal(tok, _ref(gd, "tokens")), f"delayed call {i}"
        tok = eng.generate_codes(feats, 220, delays=PARALLEL).cpu()
        eng.check_status()
        assert eng.S == 221
        _assert_tokens(parity_report, "full_parallel_greedy_raw_B2_T220", "h2", f"alternating with the delayed pattern, call {i}", tok,
                       _ref(gp, "tokens"), PARALLEL, gp["margins"], NEAR_TIE_GREEDY, 1)
    with pytest.raises(L.VauraHipError, match="block_size"):      # S = 250 + 17 > 256: refused before anything is allocated
        eng.generate_codes(feats, 250, delays=EVEN)


def test_exact_fp32_twin_rerun_keeps_the_delays(golden, full_sampler_sd_raw, parity_report):
    """generate_codes_checked re-runs a flagged call on the exact-fp32 twin with the SAME arguments: a detector bound wide enough to
    flag every decision forces that re-run, and the parallel-pattern result must still be the reference's."""
    gs = golden("full_parallel_topk250_cfg6_raw_B2_T220.npz")
    eng = DecoderEngine(synth.FULL_SAMPLER, full_sampler_sd_raw, DEV, near_tie="rerun", near_tie_eps=1.0)
    feats = synth.video_features(2, seed=int(gs["feat_seed"])).to(DEV)
    nz = synth.exp_noise(220, 18, 1024, int(gs["noise_seed"]))
    tok = eng.generate_codes_checked(feats, 220, use_sampling=True, temp=1.0, top_k=int(gs["top_k"]), cfg_scale=float(gs["cfg_scale"]),
                                     noise=nz, delays=PARALLEL).cpu()
    assert eng.near_tie_reruns == 1 and eng._range_twin.delays == tuple(PARALLEL) and eng._range_twin.S == 221
    _assert_tokens(parity_report, "full_parallel_topk250_cfg6_raw_B2_T220", "f32 (twin re-run)", "parallel pattern, cfg 6 / top-k 250",
                   tok, _ref(gs, "tokens"), PARALLEL, gs["margins"], NEAR_TIE_SAMPLED, 1)
    del eng
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------- tiny model, delays 0,2,..,16, with a prompt
@pytest.mark.parametrize("wdtype", ["auto", "f32"])
@pytest.mark.parametrize("prefill", [192, 1])
def test_tiny_custom_delays_with_prompt_match_reference(golden, tiny_sampler_sd, wdtype, prefill):
    """2 layers, delays 0,2,..,16 (S = T + 17), T = 60 with a 40-frame prompt: greedy cfg 1 and cfg 6 / top-k 250 sampled equal the
    reference's tokens; prompt teacher-forced in one GEMM pass (PREFILL_POSITIONS 192) or one decode step per position (1), the
    sampled steps with and without the captured step graph."""
    g = golden("tiny_delays_even.npz")
    delays = [int(x) for x in g["delays"]]
    T, Tp = int(g["T"]), g["prompt"].shape[-1]
    eng = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype=wdtype)
    eng.PREFILL_POSITIONS = prefill
    feats = synth.video_features(2, seed=int(g["feat_seed"])).to(DEV)
    prompt = _ref(g, "prompt").to(DEV)
    S, start = T + max(delays) + 1, Tp + 1 + delays[0]
    nz = synth.exp_noise(S - start, 18, 1024, int(g["noise_seed"]))
    for use_graph in (False, True):
        tok = eng.generate_codes(feats, T, prompt=prompt, delays=delays, use_graph=use_graph).cpu()
        eng.check_status()
        assert torch.equal(tok, _ref(g, "greedy")), (wdtype, prefill, use_graph)
        tok = eng.generate_codes(feats, T, prompt=prompt, delays=delays, use_graph=use_graph, use_sampling=True, top_k=250,
                                 cfg_scale=6.0, noise=nz).cpu()
        eng.check_status()
        assert torch.equal(tok, _ref(g, "topk250_cfg6")), (wdtype, prefill, use_graph)
    assert eng.S == S and (eng._prefill_positions > 0) == (prefill > 1 and eng.planes)


def test_sliding_window_caller_with_a_parallel_pattern_model(tiny_sampler_sd):
    """vaura_amd.longform.generate_long (scripts/generate.py:327-369) on a model whose pattern provider is ParallelPatternProvider:
    every chunk decodes S = T + 1 steps with its prompt; the result has the clip's length, valid ids, a finite waveform, and a
    second run gives the same tokens."""
    from vaura_amd import longform
    from vaura_amd.model import VAURAModel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VAURAModel(
            feature_extractor_config={"target": "vaura_amd.feature_extractor.MotionFormer"},
            audio_encoder_config={"target": "vaura_amd.codec.DacModelWrapper", "params": {"model_sr": 44100, "synthetic": True}},
            sampler_config={"target": "vaura_amd.sampler.Transformer", "params": synth.tiny_sampler(2).yaml_params()},
            visual_bridge_config={"target": "torch.nn.Identity"},
            pattern_provider_config={"target": "vaura_amd.patterns.ParallelPatternProvider", "params": {"n_q": 9}},
            flatten_vis_feats=True, freeze_feature_extractor=True)
    m.sampler.load_state_dict(tiny_sampler_sd, strict=True)
    m.sampler.audio_tokens_per_video_frame = 7
    m = m.to(DEV)
    B, S_seg, t_seg = 2, 4, 2
    feats = synth.video_features(B, tokens=S_seg * t_seg, seed=71).reshape(B, S_seg, t_seg, 768).to(DEV)
    kw = dict(stride=0.10, model_max_duration=0.30, vfps=400, use_sampling=False, cfg_scale=1.0)
    got = longform.generate_long(m, feats, 0.62, **kw)
    tok = got["sampled_indices"].cpu()
    T = tok.shape[-1]
    assert tok.shape[:2] == (B, 9) and T >= int(0.62 * longform.COMPRESSION_MODEL_FRAME_RATE)
    assert int(tok.min()) >= 0 and int(tok.max()) < 1024
    assert m.sampler.engine().delays == tuple(PARALLEL)
    assert got["generated_audio"].shape == (B, 1, T * 512) and bool(torch.isfinite(got["generated_audio"]).all())
    assert torch.equal(longform.generate_long(m, feats, 0.62, **kw)["sampled_indices"].cpu(), tok)
