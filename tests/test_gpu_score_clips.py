"""Per-clip lengths in teacher-forced scoring on the device (DecoderEngine.score_clips, VAURAModel.forward / test_step with
audio_lengths; csrc/score.hip score_nll_clips_kernel / score_reduce_clips_kernel): against the reference's full-length golden where the
inputs are the same, against every clip scored alone, and against itself.

Two places where the scalar counterpart of a check does not exist, and what stands there instead:
  * ``score(..., relevance=True)`` carries the CFG null embedding, which has Tv tokens: it refuses features cut to Tv_b < Tv.  A clip
    scored alone under its own Tv_b is therefore scored without the flag, and its "nll_per_codebook" is taken with the very call the
    flag makes (``_clip_codebook_means`` of its nll: the same kernel on the same bits).  Relevance is compared with the scalar call on
    clips cut in Ta and under the full video; with video lengths as well, the conditional half is pinned by the clip scored alone.
  * The same-input set of a cut clip, t + d_q < Ta_b + min(d), holds 81 / 117 (Ta_b = 13) and 28 / 63 (Ta_b = 7) of the clip's entries
    under the default delays and 49 / 117 and 16 / 63 under the even ones: pure counting, below one half for three of the four.  The
    lengths [20, 13, 7] are compared on exactly those sets, whose sizes are asserted; the share of at least one half is asserted on a
    second set of lengths, [20, 19, 17], added for it (99 / 171 and 81 / 153 under the even delays)."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vaura_amd import synth
from vaura_amd.engine import DecoderEngine, score_logits

DEV = "cuda:0"
SETS = ("delayed", "parallel", "even")
LENGTHS = [20, 13, 7]
LONGER = [20, 19, 17]
VIDEO = [32, 2, 1]           # clip 1's 21 positions and clip 2's 15 at 7 tokens per frame read frames behind their Tv_b
K, TA, V = 9, 20, 1024


def _delays(g, name):
    d = [int(x) for x in g[f"{name}_delays"]]
    return None if d == list(range(K)) else d


@pytest.fixture(scope="module")
def engines(tiny_sampler_sd):
    cache = {}

    def get(storage):
        if storage not in cache:
            cache[storage] = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype=storage)
        return cache[storage]
    return get


@pytest.fixture(scope="module")
def data(golden):
    g = golden("eval_tiny.npz")
    feats = synth.video_features(3, seed=int(g["feat_seed"])).to(DEV)

    def get(name):
        return torch.from_numpy(g[f"{name}_codes"].astype(np.int64)).to(DEV), feats, _delays(g, name)
    return get


def same_eq(a, b):
    """torch.equal with NaN equal to NaN"""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


# ------------------------------------------------------------------------------------- 1. pinned by the reference
def same_input(delays, Ta_b):
    """(K, TA) bool: the entries of a clip cut to Ta_b whose every input is the full-length call's — output position t + d_q lies before
    the first position at which the cut sequence holds the special token for a code the full one feeds (Ta_b + min(d)); all of a clip
    that is not cut."""
    d = torch.tensor(delays if delays is not None else list(range(K)))
    t = torch.arange(TA)
    if Ta_b == TA:
        return torch.ones(K, TA, dtype=torch.bool)
    return (t[None, :] < Ta_b) & (t[None, :] + d[:, None] < Ta_b + int(d.min()))


COUNTS = {("delayed", 13): 81, ("delayed", 7): 28, ("even", 13): 49, ("even", 7): 16, ("even", 19): 99, ("even", 17): 81,
          ("delayed", 19): 135, ("delayed", 17): 117}


@pytest.mark.parametrize("storage", ["h2", "h1", "f32"])
@pytest.mark.parametrize("name,lengths", [("parallel", LENGTHS), ("delayed", LENGTHS), ("even", LENGTHS), ("delayed", LONGER),
                                          ("even", LONGER)])
def test_clips_match_the_reference_where_the_inputs_are_the_same(engines, data, golden, storage, name, lengths):
    g = golden("eval_tiny.npz")
    codes, feats, dl = data(name)
    r = engines(storage).score_clips(codes, feats, lengths, delays=dl, return_logits=True)
    ref_nll, ref_logits = torch.from_numpy(g[f"{name}_nll"]), torch.from_numpy(g[f"{name}_logits"])
    keep = [int(t) for t in g["keep_t"]]
    for b, Ta_b in enumerate(lengths):
        m = same_input(dl, Ta_b)
        n = int(m.sum())
        if name == "parallel" or Ta_b == TA:
            assert n == K * Ta_b                                       # all delays zero: every entry of the clip
        else:
            assert n == COUNTS[(name, Ta_b)]
            if lengths is LONGER:
                assert 2 * n >= K * Ta_b, (name, Ta_b, n)              # at least half of the cut clip's entries are pinned
        err = (r["nll"][b].cpu() - ref_nll[b]).abs()[m]
        print(f"{storage} {name} clip {b} Ta_b {Ta_b}: {n} of {K * Ta_b} entries, nll max abs err {float(err.max()):.3g}")
        assert float(err.max()) < 1e-4
        for i, t in enumerate(keep):
            if t < Ta_b and bool(m[:, t].any()):
                e = (r["logits"][b, :, t].cpu() - ref_logits[b, :, i]).abs()[m[:, t]]
                print(f"   logits at t = {t}: max abs err {float(e.max()):.3g}")
                assert float(e.max()) < 3e-5


# ------------------------------------------------------------------------------------- 2. against the clip scored alone (+ 5. relevance)
@pytest.mark.parametrize("mode", ["f32", "h2_per_position", "h2_chunked"])
def test_every_clip_equals_the_clip_scored_alone(tiny_sampler_sd, data, monkeypatch, mode):
    codes, feats, dl = data("delayed")
    if mode == "h2_per_position":
        monkeypatch.setattr(DecoderEngine, "PREFILL_POSITIONS", 1)
    eng = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype=mode[:3].rstrip("_"))
    exact = mode != "h2_chunked"       # one decode step per position on identical rows; the chunks' row count differs between the calls

    def close(a, b, what, same_rows=True):
        d = float((a - b).abs().max())
        print(f"{mode} {what}: max abs diff {d:.3g}")
        assert torch.equal(a, b) if (exact and same_rows) else d < 2e-5, what

    r = eng.score_clips(codes, feats, LENGTHS, video_lengths=VIDEO, delays=dl)
    rr = eng.score_clips(codes, feats, LENGTHS, video_lengths=VIDEO, delays=dl, relevance=True)
    if mode == "h2_per_position":
        assert eng._prefill_positions == 0
    assert bool(torch.isfinite(rr["relevance"]).all()) and bool(torch.isfinite(rr["nll_null_per_codebook"]).all())
    for b, (Ta_b, Tv_b) in enumerate(zip(LENGTHS, VIDEO)):
        s = eng.score(codes[..., :Ta_b], feats[:, :Tv_b].contiguous(), delays=dl)
        pcb = eng._clip_codebook_means(s["nll"])                       # what relevance=True reports as "nll_per_codebook"
        # (the relevance call carries twice the rows of the clip scored alone without the flag: held to the bound between schedules)
        for got, what, same_rows in ((r, "score_clips", True), (rr, "score_clips relevance", False)):
            close(got["nll"][b, :, :Ta_b], s["nll"][b], f"{what} nll clip {b}", same_rows)
            close(got["nll_per_codebook"][b], pcb[b], f"{what} nll_per_codebook clip {b}", same_rows)
    # relevance: clips cut in Ta under the full video, against the scalar relevance call on the cut clips
    rel = eng.score_clips(codes, feats, LENGTHS, delays=dl, relevance=True)
    for b, Ta_b in enumerate(LENGTHS):
        s = eng.score(codes[..., :Ta_b], feats, delays=dl, relevance=True)
        for k in ("nll_per_codebook", "nll_null_per_codebook", "relevance_per_codebook", "relevance"):
            close(rel[k][b], s[k][b], f"{k} clip {b}")
        close(rel["nll_null"][b, :, :Ta_b], s["nll_null"][b], f"nll_null clip {b}")
    assert eng.range_fallbacks == 0


# ------------------------------------------------------------------------------------- 3. same schedule, same bits
def test_same_schedule_same_bits(engines, data):
    eng = engines("h2")
    codes, feats, dl = data("even")
    full = eng.score_clips(codes, feats, [TA] * 3, delays=dl, return_logits=True)
    plain = eng.score(codes, feats, delays=dl, return_logits=True)
    assert eng._prefill_positions > 1                                  # the chunked plane path
    for k in plain:
        assert torch.equal(full[k], plain[k]), k
    assert torch.equal(eng.score_clips(codes, feats, delays=dl)["nll"], plain["nll"])      # lengths None: every clip has Ta
    a = eng.score_clips(codes, feats, LENGTHS, video_lengths=VIDEO, delays=dl, return_logits=True)
    gen = torch.Generator().manual_seed(17)
    codes2, feats2 = codes.clone(), feats.clone()
    for b, (Ta_b, Tv_b) in enumerate(zip(LENGTHS, VIDEO)):             # other valid ids, other features, behind every clip's end
        codes2[b, :, Ta_b:] = torch.randint(0, V, (K, TA - Ta_b), generator=gen).to(DEV)
        feats2[b, Tv_b:] = torch.randn(feats.shape[1] - Tv_b, feats.shape[2], generator=gen).to(DEV)
    assert not torch.equal(codes2, codes) and not torch.equal(feats2, feats)
    b2 = eng.score_clips(codes2, feats2, LENGTHS, video_lengths=VIDEO, delays=dl, return_logits=True)
    again = eng.score_clips(codes, feats, LENGTHS, video_lengths=VIDEO, delays=dl, return_logits=True)
    for k in a:
        assert same_eq(a[k], b2[k]), k
        assert same_eq(a[k], again[k]), k
    # ids outside the codebook behind a clip's end are not the clip's codes: not range-checked
    codes2[1, :, 13:] = -7
    assert same_eq(eng.score_clips(codes2, feats2, LENGTHS, video_lengths=VIDEO, delays=dl)["nll"], a["nll"])
    codes2[1, 0, 12] = V
    with pytest.raises(Exception, match="codes must lie"):
        eng.score_clips(codes2, feats2, LENGTHS, video_lengths=VIDEO, delays=dl)


# ------------------------------------------------------------------------------------- 4. the reductions
@pytest.mark.parametrize("name", SETS)
def test_reductions_and_mask(engines, tiny_sampler_sd, data, name):
    eng = engines("h2")
    codes, feats, dl = data(name)
    r = eng.score_clips(codes, feats, LENGTHS, video_lengths=VIDEO, delays=dl, return_logits=True)
    want_mask = (torch.arange(TA, device=DEV)[None, None, :] < torch.tensor(LENGTHS, device=DEV)[:, None, None]).expand(3, K, TA)
    assert torch.equal(r["mask"], want_mask)
    assert torch.equal(r["nll"].isnan(), ~want_mask)
    assert torch.equal(r["logits"].isnan().all(-1), ~want_mask) and torch.equal(r["logits"].isnan().any(-1), ~want_mask)
    assert r["lengths"].dtype == torch.int32 and r["lengths"].tolist() == LENGTHS
    loss, lpc, _ = score_logits(r["logits"], codes, r["mask"])        # the same kernels in the same order
    assert torch.equal(loss, r["loss"]) and torch.equal(lpc, r["loss_per_codebook"])
    # the pooled mean: every valid (b, t) of a codebook weighs the same (the reference's _compute_loss under the mask)
    want = torch.stack([r["nll"][:, q][want_mask[:, q]].double().mean() for q in range(K)])
    assert float((r["loss_per_codebook"].double() - want).abs().max()) < 1e-5 * float(want.max())
    assert abs(float(r["loss"]) - float(want.mean())) < 1e-5 * float(want.mean())
    one = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype="h2") if name == "delayed" else None
    for b, (Ta_b, Tv_b) in enumerate(zip(LENGTHS, VIDEO)):
        pc = r["nll"][b, :, :Ta_b].double().mean(-1)
        assert float((r["nll_per_codebook"][b].double() - pc).abs().max()) < 1e-5 * float(pc.max())
        if one is not None:                                            # the loss clip b gets scored alone, at batch 1
            alone = float(one.score(codes[b:b + 1, :, :Ta_b], feats[b:b + 1, :Tv_b].contiguous(), delays=dl)["loss"])
            print(f"clip {b}: loss_per_clip {float(r['loss_per_clip'][b]):.7f}, alone at batch 1 {alone:.7f}")
            assert abs(float(r["loss_per_clip"][b]) - alone) < 1e-5 * alone


# ------------------------------------------------------------------------------------- 6. edges
def test_two_timesteps_a_list_of_clips_and_explicit_delays(engines, data):
    eng = engines("h2")
    codes, feats, dl = data("even")
    lengths = [2, 20, 9]
    r = eng.score_clips(codes, feats, lengths, video_lengths=[1, 32, 3], delays=dl, return_logits=True)
    assert bool(torch.isfinite(r["nll"][0, :, :2]).all()) and bool(r["nll"][0, :, 2:].isnan().all())
    assert bool(torch.isfinite(r["loss_per_clip"]).all()) and bool(torch.isfinite(r["loss"]))
    s = eng.score(codes[..., :2], feats[:, :1].contiguous(), delays=dl)
    assert float((r["nll"][0, :, :2] - s["nll"][0]).abs().max()) < 2e-5
    # a list: (K, Ta_b) and (1, K, Ta_b) entries, padded by the engine — the bits of the padded-tensor call
    as_list = [codes[0, :, :2], codes[1:2], codes[2, :, :9]]
    li = eng.score_clips(as_list, feats, video_lengths=[1, 32, 3], delays=dl, return_logits=True)
    assert set(li) == set(r)
    for k in r:
        assert same_eq(li[k], r[k]), k
    with pytest.raises(Exception, match="2 .. 20"):
        eng.score_clips(codes, feats, [1, 20, 9], delays=dl)
    # the C entry point reads the lengths back itself: a value outside 2 .. Ta never reaches a kernel
    eng.clip_T.copy_(torch.tensor([1, 20, 9], dtype=torch.int32))
    import ctypes as C
    from vaura_amd import _lib as L
    tg = codes.to(torch.int32).contiguous()
    f32 = dict(dtype=torch.float32, device=DEV)
    nll, lpc, loss = torch.empty(3, K, TA, **f32), torch.empty(K, **f32), torch.empty((), **f32)
    eng._reset_state()
    rc = eng.lib.vaura_score(C.byref(eng.dec), eng.S - 1, L.ptr(tg), L.ptr(eng._score_workspace()), None, L.ptr(nll), None, L.ptr(lpc),
                             L.ptr(loss), L.current_stream(eng.dev))
    assert rc == -1


# ------------------------------------------------------------------------------------- 7. model level
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
    m.sampler.audio_tokens_per_video_frame = 7
    return m.to(DEV)


def test_model_serves_a_padded_batch(tiny_sampler_sd):
    m = _model(tiny_sampler_sd)
    B = 2
    frames = synth.video_features(B, seed=5).reshape(B, 4, 8, 768).to(DEV)
    wav = (torch.randn(B, 1, 20 * 512, generator=torch.Generator().manual_seed(123)) * 0.3).to(DEV)
    n = [20 * 512, 11 * 512 + 100]
    alone = [m.audio_encoder.encode(wav[b:b + 1, :, :n[b]]) for b in range(B)]
    Ta = [int(c.shape[-1]) for c in alone]
    assert Ta[0] == 20 and 2 <= Ta[1] < 20
    logits, mask, aud = m.forward(frames, wav, audio_lengths=n)
    assert aud.shape[-1] == 20 and logits.shape == (B, 9, 20, 1024)
    for b in range(B):
        assert torch.equal(aud[b:b + 1, :, :Ta[b]], alone[b]), b       # the codes of the clip encoded alone
        assert bool(mask[b, :, :Ta[b]].all()) and not bool(mask[b, :, Ta[b]:].any())
    vis = m._handle_visual_conditioning(frames)
    direct = m.sampler.engine().score_clips(aud[:, :9], vis, Ta, tokens_per_frame=7)
    batch = {"audio": wav, "frames": frames, "meta": {}, "audio_lengths": n}
    assert torch.equal(m.test_step(batch, 0), direct["loss"])
    assert torch.equal(m.validation_step(dict(batch, video_lengths=[32, 3]), 0),
                       m.sampler.engine().score_clips(aud[:, :9], vis, Ta, video_lengths=[32, 3], tokens_per_frame=7)["loss"])
    rel = m.score_relevance(frames, wav, audio_lengths=n)
    assert rel["lengths"].tolist() == Ta and torch.equal(rel["loss"], direct["loss"]) and bool(torch.isfinite(rel["relevance"]).all())
    # without the keys: today's call
    plain = m.sampler.engine().score(m.audio_encoder.encode(wav)[:, :9], vis, tokens_per_frame=7)
    assert torch.equal(m.test_step({"audio": wav, "frames": frames, "meta": {}}, 0), plain["loss"])
    lg, mk, _ = m.forward(frames, wav)
    assert bool(mk.all()) and torch.equal(lg, m.sampler.engine().score(m.audio_encoder.encode(wav)[:, :9], vis, tokens_per_frame=7,
                                                                        return_logits=True)["logits"])
