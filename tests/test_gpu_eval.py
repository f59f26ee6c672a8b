"""Teacher-forced scoring on the device (DecoderEngine.score, VAURAModel.forward / _compute_loss / test_step; csrc/score.hip) against
the reference's own forward + _compute_loss (tests/golden/make_golden_eval.py), and against itself."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vaura_amd import synth
from vaura_amd.engine import DecoderEngine, score_logits

DEV = "cuda:0"
SETS = ("delayed", "parallel", "even")


def _delays(g, name):
    d = [int(x) for x in g[f"{name}_delays"]]
    return None if d == list(range(9)) else d


def _check_parity(report, golden_name, storage, what, r, g, prefix, keep):
    loss, lpc, nll = float(r["loss"]), r["loss_per_codebook"].cpu().numpy(), r["nll"].cpu().numpy()
    rl, rlpc, rnll = float(g[prefix + "loss"]), g[prefix + "loss_per_codebook"], g[prefix + "nll"]
    e = {"golden": golden_name, "storage": storage, "what": what, "loss": loss, "reference_loss": rl,
         "loss_rel_err": abs(loss - rl) / abs(rl), "loss_per_codebook_max_rel_err": float(np.max(np.abs(lpc - rlpc) / np.abs(rlpc))),
         "nll_max_abs_err": float(np.abs(nll - rnll).max())}
    if "logits" in r:
        e["logits_max_abs_err"] = float((r["logits"][:, :, keep].cpu() - torch.from_numpy(g[prefix + "logits"])).abs().max())
    report.entries.append(e)
    assert bool(r["mask"].all()) and bool(torch.from_numpy(g[prefix + "mask"]).all())
    assert e["loss_rel_err"] < 1e-5, e
    assert e["loss_per_codebook_max_rel_err"] < 1e-5, e
    assert e["nll_max_abs_err"] < 1e-4, e
    if "logits" in r:
        assert e["logits_max_abs_err"] < 3e-5, e
    return e


@pytest.fixture(scope="module")
def tiny_engines(tiny_sampler_sd):
    cache = {}

    def get(storage):
        if storage not in cache:
            cache[storage] = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype=storage)
        return cache[storage]
    return get


@pytest.fixture(scope="module")
def full_engines(full_sampler_sd_raw):
    cache = {}

    def get(storage, **kw):
        key = (storage, tuple(sorted(kw.items())))
        if key not in cache:
            cache.clear()                  # one full-depth engine at a time (2.7 GB of fp32 tiles for "f32")
            torch.cuda.empty_cache()
            cache[key] = DecoderEngine(synth.FULL_SAMPLER, full_sampler_sd_raw, DEV, wdtype=storage, **kw)
        return cache[key]
    return get


# ------------------------------------------------------------------------------------- parity against the reference
@pytest.mark.parametrize("storage", ["h2", "h1", "f32"])
@pytest.mark.parametrize("name", SETS)
def test_tiny_score_matches_reference(tiny_engines, golden, parity_report, storage, name):
    g = golden("eval_tiny.npz")
    codes = torch.from_numpy(g[f"{name}_codes"].astype(np.int64)).to(DEV)
    feats = synth.video_features(codes.shape[0], seed=int(g["feat_seed"])).to(DEV)
    r = tiny_engines(storage).score(codes, feats, delays=_delays(g, name), return_logits=True)
    _check_parity(parity_report, "eval_tiny", storage, f"score, delays {name}", r, g, f"{name}_", [int(t) for t in g["keep_t"]])


@pytest.mark.parametrize("storage", ["h2", "f32"])
def test_full_score_matches_reference(full_engines, golden, parity_report, storage):
    g = golden("eval_full_raw_B2_T220.npz")
    feats = synth.video_features(2, seed=int(g["feat_seed"])).to(DEV)
    eng = full_engines(storage)
    greedy = torch.from_numpy(golden("full_greedy_raw_B2_T220.npz")["tokens"].astype(np.int64)).to(DEV)
    uniform = torch.from_numpy(g["uniform_codes"].astype(np.int64)).to(DEV)
    keep = [int(t) for t in g["keep_t"]]
    for name, codes in (("greedy", greedy), ("uniform", uniform)):
        r = eng.score(codes, feats, return_logits=True)
        _check_parity(parity_report, "eval_full_raw_B2_T220", storage, f"score, {name} codes", r, g, f"{name}_", keep)
        if name == "greedy":
            # every scored token is its row's greedy choice, so its NLL is the row's smallest one (up to the golden's near-ties) —
            # at the output positions s = t + d_q < Ta whose inputs are the decode loop's: the reference's forward feeds
            # codes[..., :-1], so from position Ta + d_0 on the special token replaces timestep Ta - 1 the loop had fed
            lg = r["logits"]
            nll_min = torch.logsumexp(lg, -1) - lg.max(-1).values
            same_input = (torch.arange(220, device=DEV)[None, :] + torch.arange(9, device=DEV)[:, None]) < 220
            assert float((r["nll"] - nll_min).abs()[:, same_input].max()) < 1e-4


# ------------------------------------------------------------------------------------- internal consistency
def test_batched_path_equals_per_position_path(tiny_sampler_sd, golden, monkeypatch):
    g = golden("eval_tiny.npz")
    codes = torch.from_numpy(g["even_codes"].astype(np.int64)).to(DEV)
    feats = synth.video_features(codes.shape[0], seed=int(g["feat_seed"])).to(DEV)
    batched = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype="h2").score(codes, feats, delays=_delays(g, "even"))
    monkeypatch.setattr(DecoderEngine, "PREFILL_POSITIONS", 1)
    step = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype="h2")
    per_pos = step.score(codes, feats, delays=_delays(g, "even"))
    assert step._prefill_positions == 0                       # the decode step with heads at every position
    assert float((batched["nll"] - per_pos["nll"]).abs().max()) < 2e-5
    assert abs(float(batched["loss"]) - float(per_pos["loss"])) < 1e-5 * float(per_pos["loss"])


def test_two_calls_are_bit_identical(tiny_engines, golden):
    g = golden("eval_tiny.npz")
    codes = torch.from_numpy(g["delayed_codes"].astype(np.int64)).to(DEV)
    feats = synth.video_features(codes.shape[0], seed=int(g["feat_seed"])).to(DEV)
    a = tiny_engines("h2").score(codes, feats)
    b = tiny_engines("h2").score(codes, feats)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["loss_per_codebook"], b["loss_per_codebook"])
    assert torch.equal(a["nll"], b["nll"])


def test_compute_loss_on_given_logits_equals_score(tiny_engines, golden):
    g = golden("eval_tiny.npz")
    codes = torch.from_numpy(g["parallel_codes"].astype(np.int64)).to(DEV)
    feats = synth.video_features(codes.shape[0], seed=int(g["feat_seed"])).to(DEV)
    r = tiny_engines("h2").score(codes, feats, delays=_delays(g, "parallel"), return_logits=True)
    loss, lpc, nll = score_logits(r["logits"], codes, r["mask"])
    assert torch.equal(nll, r["nll"])                         # same kernel, same rows
    assert torch.equal(loss, r["loss"]) and torch.equal(lpc, r["loss_per_codebook"])
    # a mask that drops entries: the mean runs over the kept ones only (vaura_model.py:270-275)
    mask = r["mask"].clone()
    mask[:, :, ::2] = False
    loss2, lpc2, _ = score_logits(r["logits"], codes, mask)
    want = torch.stack([r["nll"][:, q][mask[:, q]].double().mean() for q in range(9)])
    assert float((lpc2.double() - want).abs().max()) < 1e-5 * float(want.abs().max())


# ------------------------------------------------------------------------------------- plugin surface, end to end
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
            flatten_vis_feats=True, freeze_feature_extractor=True)
    m.sampler.load_state_dict(sd, strict=True)
    m.sampler.audio_tokens_per_video_frame = 7   # scripts/generate.py:216
    return m.to(DEV)


def test_forward_and_test_step_end_to_end(tiny_sampler_sd):
    m = _model(tiny_sampler_sd)
    B = 2
    frames = synth.video_features(B, seed=5).reshape(B, 4, 8, 768).to(DEV)
    g = torch.Generator().manual_seed(123)
    wav = (torch.randn(B, 1, 20 * 512, generator=g) * 0.3).to(DEV)
    logits, mask, aud = m.forward(frames, wav)
    assert logits.shape == (B, 9, 20, 1024) and mask.shape == (B, 9, 20) and bool(mask.all())
    loss, lpc = m._compute_loss(logits, aud[:, :9], mask)
    assert bool(torch.isfinite(loss)) and len(lpc) == 9
    codes = m.audio_encoder.encode(wav)
    assert torch.equal(codes, aud)
    direct = m.sampler.engine().score(codes, m._handle_visual_conditioning(frames), tokens_per_frame=7)
    assert torch.equal(loss, direct["loss"])
    batch = {"audio": wav, "frames": frames, "meta": {}}
    assert torch.equal(m.test_step(batch, 0), direct["loss"])
    assert set(m.last_eval_log) == {"test_loss", "test_loss_per_codebook"}
    assert torch.equal(m.validation_step(batch, 0), direct["loss"])
    # audio_tokens_per_video_frame None: set from the sequence (llama.py:_set_audio_tokens_per_video_frame) and kept
    m.sampler.audio_tokens_per_video_frame = None
    m.forward(frames, wav)
    assert m.sampler.audio_tokens_per_video_frame == -(-(20 + 9 - 9) // 32) == 1


# ------------------------------------------------------------------------------------- other storages: reported, not asserted
@pytest.mark.parametrize("storage,kw", [("fp8h", {}), ("h2", {"kv_dtype": "f16"})])
def test_low_precision_storages_report_distance_to_h2(full_engines, golden, parity_report, storage, kw):
    g = golden("eval_full_raw_B2_T220.npz")
    feats = synth.video_features(2, seed=int(g["feat_seed"])).to(DEV)
    codes = torch.from_numpy(g["uniform_codes"].astype(np.int64)).to(DEV)
    r = full_engines(storage, **kw).score(codes, feats)
    assert bool(torch.isfinite(r["loss"]))
    rl = float(g["uniform_loss"])
    parity_report.entries.append({"golden": "eval_full_raw_B2_T220", "storage": storage + "".join(f" {k}={v}" for k, v in kw.items()),
                                  "what": "score, uniform codes (reported only)", "loss": float(r["loss"]), "reference_loss": rl,
                                  "loss_rel_err": abs(float(r["loss"]) - rl) / rl,
                                  "nll_max_abs_err": float(np.abs(r["nll"].cpu().numpy() - g["uniform_nll"]).max())})
