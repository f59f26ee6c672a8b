"""Audio out of one generate() call while its decode loop still runs: vaura_dac_decode_window_seq (csrc/dac.hip),
DecoderEngine.generate_codes_stream, VAURAModel.generate_stream and longform.generate_long_stream(block_frames=...).

The contract is bit equality — every comparison is torch.equal, nothing has a tolerance: a window packed from the pattern sequence is
the window packed from the reverted codes, and the blocks of a stream, concatenated per clip, are the audio, the tokens and the
per-token values that generate() returns for the same call.  The loop runs in pieces whose lengths are no multiples of its graph
grouping, on the one captured step, so the tokens are the same by construction; what can go wrong is the bookkeeping — a window that
reads a slot not yet sampled, a halo taken from the wrong place, a block boundary off by one — and that shows as a changed sample.

Shapes: the tiny plugin model (2 layers, 9 codebooks, delays 0..8) with the full-size synthetic codec; T = 43 frames (51 sampled steps)
is three blocks at block_frames 16, nine at 4, five at 7 (pieces off the loop's 4-step grouping) and one at 64: the last block of a
clip takes every frame that is left once the loop has ended, the halo it had held back included."""
import os
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_per_clip_sampling as G  # noqa: E402  (the tiny plugin model)
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import clip_params, longform, ops, synth  # noqa: E402
from vaura_amd.codec_clips import decode_halo, window_layout  # noqa: E402
from vaura_amd.engine import CodecEngine, DecoderEngine  # noqa: E402

DEV = "cuda:0"
CFG = synth.FULL_CODEC
HOP = CFG.hop
H = decode_halo(CFG)
K, TV = 9, 32
PRECISIONS = ["f32", "f16pair", "f16", "f16pair_w8", "mx8"]
SMALL = ([64, 33, 7, 21], [(20, 9), (0, 33), (3, 1), (0, 0)])         # tests/test_gpu_codec_window.py
REL = ("relevance", "logprob_cond", "logprob_null")
GREEDY = dict(use_sampling=False, cfg_scale=1.0)
SAMPLED = dict(use_sampling=True, temp=0.9, top_k=128, cfg_scale=3.0)


# ---------------------------------------------------------------------------------------------------------------- a. the codec call
@pytest.fixture(scope="module")
def codec_sd():
    return dict(synth.codec_state_dict(CFG, seed=0))


@pytest.mark.parametrize("delays", [None, [0] * K], ids=["delays_0..8", "parallel"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_window_from_the_sequence_is_the_window_from_the_codes(codec_sd, precision, delays):
    eng = CodecEngine(CFG, codec_sd, DEV, precision=precision)
    lengths, windows = SMALL
    B, T = len(lengths), max(lengths)
    starts, counts = [s for s, _ in windows], [n for _, n in windows]
    codes = torch.randint(0, CFG.codebook_size, (B, K, T), generator=torch.Generator().manual_seed(1)).to(DEV)
    want = eng.decode_window(codes, starts, counts, lengths).clone()
    seq = ops.pattern_build(codes, CFG.codebook_size, delays).to(torch.int32)
    assert torch.equal(ops.pattern_revert(seq, T, -1, delays), codes.to(torch.int32))
    # everything of the sequence that the windows and their halos do not cover holds -1: a slot read outside them changes a sample
    d = list(range(K)) if delays is None else delays
    lay = window_layout(lengths, starts, counts, CFG)
    read = torch.zeros_like(seq, dtype=torch.bool)
    for b, lo, hi in zip(lay.clips, lay.lo, lay.hi):
        for q in range(K):
            read[b, q, lo + 1 + d[q]:hi + 1 + d[q]] = True
    seq = torch.where(read, seq, torch.full_like(seq, -1)).contiguous()
    assert int((seq == -1).sum()) > 0
    before = seq.clone()
    for w in eng._ws:                                                  # sized by the window call above: the seq call needs the same
        w.view(torch.uint8).fill_(0xFF)
    ws = [w.data_ptr() for w in eng._ws]
    got = eng.decode_window_seq(seq, starts, counts, lengths, delays)
    torch.cuda.synchronize()
    assert [w.data_ptr() for w in eng._ws] == ws                       # the poisoned buffers are the ones the call ran in
    assert torch.equal(seq, before)                                    # the caller's sequence is untouched
    assert bool(torch.isfinite(got).all()), "a 0xFF byte of the workspace reached the output"
    for b, n in enumerate(counts):
        d_max = float((got[b, :, :n * HOP] - want[b, :, :n * HOP]).abs().max()) if n else 0.0
        print(f"{precision}, clip {b}: frames [{starts[b]}, {starts[b] + n}): max |from seq - from codes| = {d_max:.3e}")
    assert torch.equal(got, want)


def test_window_seq_refusals(codec_sd):
    eng = CodecEngine(CFG, codec_sd, DEV)
    seq = torch.zeros(2, K, 52, dtype=torch.int32, device=DEV)         # T = 43
    with pytest.raises(L.VauraHipError, match="lengths must lie in 1 .. 43"):
        eng.decode_window_seq(seq, [0, 0], [4, 4], [44, 43])           # a clip that reaches a step >= S
    with pytest.raises(L.VauraHipError, match="inside its clip"):
        eng.decode_window_seq(seq, [40, 0], [4, 4])
    with pytest.raises(L.VauraHipError, match="int32"):
        eng.decode_window_seq(seq.to(torch.int64), [0, 0], [4, 4])
    with pytest.raises(L.VauraHipError, match="holds no frame"):
        eng.decode_window_seq(seq[:, :8].contiguous(), [0, 0], [4, 4])


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def model(tiny_sampler_sd):
    return G._model(tiny_sampler_sd)


def frames_of(B, seed=31):
    return synth.video_features(B, tokens=TV, seed=seed).reshape(B, 1, TV, 768).to(DEV)


def assemble(blocks, B, T, special, key, fill):
    """The blocks of a stream laid back onto (B, C, T [* HOP]); checks on the way that they tile every clip in order."""
    first = blocks[0][key]
    per = HOP if key == "audio" else 1
    out = torch.full((B, first.shape[1], T * per), fill, dtype=first.dtype, device=first.device)
    at = [0] * B
    for blk in blocks:
        s = blk["start_frames"] if "start_frames" in blk else [blk["start_frame"]] * B
        n = blk["frames"] if isinstance(blk["frames"], list) else [blk["frames"]] * B
        assert s == at, (s, at)
        for b in range(B):
            out[b, :, at[b] * per:(at[b] + n[b]) * per] = blk[key][b, :, :n[b] * per]
            assert bool((blk[key][b, :, n[b] * per:] == fill).all())   # left-aligned, the fill behind a clip's frames
            at[b] += n[b]
    return out, at


REF = {}


def reference(model, name, **kw):
    """generate() of a case, computed once per module and left unchanged"""
    if name not in REF:
        r = model.generate(return_sampled_indices=True, prompt_is_encoded=True, **kw)
        REF[name] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}
    return REF[name]


def check_stream_equals_generate(model, name, B, T, block_frames, way, lengths=None, start=1):
    frames = frames_of(B)
    ref = reference(model, name, frames=frames, max_new_tokens=T, **way)
    blocks = list(model.generate_stream(frames=frames, max_new_tokens=T, prompt_is_encoded=True, block_frames=block_frames, **way))
    plan = [r for _, r in clip_params.stream_schedule(T, lengths, start, None, H, block_frames, num_codebooks=K)]
    plan = [r for r in plan if any(hi > lo for lo, hi in r)]
    assert [(blk["start_frame"], blk["start_frame"] + blk["frames"]) for blk in blocks] == [r[0] for r in plan]
    assert [blk["final"] for blk in blocks] == [False] * (len(blocks) - 1) + [True]
    audio, at = assemble(blocks, B, T, model.special_token_id, "audio", 0.0)
    tokens, _ = assemble(blocks, B, T, model.special_token_id, "sampled_indices", model.special_token_id)
    assert at == [T] * B
    assert torch.equal(tokens, ref["sampled_indices"])
    for blk in blocks:
        lo, hi = blk["start_frame"] * HOP, (blk["start_frame"] + blk["frames"]) * HOP
        d = float((blk["audio"] - ref["generated_audio"][..., lo:hi]).abs().max())
        print(f"{name}, block_frames {block_frames}: frames [{blk['start_frame']}, {blk['start_frame'] + blk['frames']}): max |block - generate| = {d:.3e}")
    assert torch.equal(audio, ref["generated_audio"])
    return blocks


# ---------------------------------------------------------------------------------------------------------------- b. tokens and audio
@pytest.mark.parametrize("block_frames", [4, 7, 16, 64])
@pytest.mark.parametrize("name,way", [("greedy", GREEDY), ("sampled_cfg3", SAMPLED)], ids=["greedy", "sampled_cfg3"])
def test_stream_is_generate_cut_up(model, name, way, block_frames):
    blocks = check_stream_equals_generate(model, name, 2, 43, block_frames, way)
    assert len(blocks) == {4: 9, 7: 5, 16: 3, 64: 1}[block_frames]       # targets m < T with m + H + 1 + max(d) - start < S - start, + the end


# ---------------------------------------------------------------------------------------------------------------- c. per-clip calls
def test_per_clip_lengths_parameters_and_values(model):
    B, T = 4, [43, 23, 9, 1]
    Tp = 0
    frames = frames_of(B, seed=33)
    sets = G.with_cfg(G.SETS, G.CFG_MIXED)
    kw = dict(G.columns(sets), video_lengths=[32, 20, 9, 1], return_logprobs=True, return_relevance=True)
    ref = model.generate(frames=frames, max_new_tokens=T, return_sampled_indices=True, prompt_is_encoded=True, **kw)
    blocks = list(model.generate_stream(frames=frames, max_new_tokens=T, prompt_is_encoded=True, block_frames=7, **kw))
    plan = [r for _, r in clip_params.stream_schedule(43, T, Tp + 1, None, H, 7, num_codebooks=K)]
    assert [list(zip(b["start_frames"], b["frames"])) for b in blocks] == [[(lo, hi - lo) for lo, hi in r] for r in plan if any(hi > lo for lo, hi in r)]
    assert [b["final"] for b in blocks] == [False] * (len(blocks) - 1) + [True]
    assert sum(1 for b in blocks if b["frames"][2]) == 1 and sum(1 for b in blocks if b["frames"][3]) == 1       # T_b <= H: once
    sp = model.special_token_id
    for key, fill, want in [("audio", 0.0, "generated_audio"), ("sampled_indices", sp, "sampled_indices"), ("logprobs", 0.0, "logprobs")] + \
                           [(k, 0.0, k) for k in REL]:
        got, at = assemble(blocks, B, 43, sp, key, fill)
        assert at == T
        for b in range(B):
            n = T[b] * (HOP if key == "audio" else 1)
            assert torch.equal(got[b, :, :n], ref[want][b, :, :n]), (key, b)


def test_common_prompt_with_per_clip_lengths_and_parameters(model):
    """The 5-frame common prompt with per-clip lengths, video lengths and the parameter mix.  A common prompt must be shorter than every
    clip (generate() refuses it otherwise), so it cannot go with the 1-frame clip of the test above: the last clip has 6 frames here."""
    B, T, Tp = 4, [43, 23, 9, 6], 5
    frames = frames_of(B, seed=34)
    prompt = torch.randint(0, 1024, (B, K, Tp), generator=torch.Generator().manual_seed(5)).to(DEV)
    with pytest.raises(L.VauraHipError, match="shorter than every clip"):
        model.generate_stream(frames=frames, audio=prompt, max_new_tokens=[43, 23, 9, 1], prompt_is_encoded=True)
    kw = dict(G.columns(G.with_cfg(G.SETS, G.CFG_MIXED)), video_lengths=[32, 20, 9, 6], audio=prompt)
    ref = model.generate(frames=frames, max_new_tokens=T, return_sampled_indices=True, prompt_is_encoded=True, **kw)
    blocks = list(model.generate_stream(frames=frames, max_new_tokens=T, prompt_is_encoded=True, block_frames=16, **kw))
    plan = [r for _, r in clip_params.stream_schedule(43, T, Tp + 1, None, H, 16, num_codebooks=K)]
    assert [list(zip(b["start_frames"], b["frames"])) for b in blocks] == [[(lo, hi - lo) for lo, hi in r] for r in plan if any(hi > lo for lo, hi in r)]
    sp = model.special_token_id
    tokens, at = assemble(blocks, B, 43, sp, "sampled_indices", sp)
    audio, _ = assemble(blocks, B, 43, sp, "audio", 0.0)
    assert at == T
    assert torch.equal(tokens[..., :Tp], prompt)                       # the prompt frames are part of the stream
    for b in range(B):
        assert torch.equal(tokens[b, :, :T[b]], ref["sampled_indices"][b, :, :T[b]]), b
        assert torch.equal(audio[b, :, :T[b] * HOP], ref["generated_audio"][b, :, :T[b] * HOP]), b
    # equal per-clip prompt lengths are the common prompt; the same blocks
    same = list(model.generate_stream(frames=frames, max_new_tokens=T, prompt_is_encoded=True, block_frames=16,
                                      **dict(kw, audio=torch.nn.functional.pad(prompt, (0, 3)), prompt_lengths=[Tp] * B)))
    assert len(same) == len(blocks) and all(torch.equal(x["audio"], y["audio"]) for x, y in zip(same, blocks))


# ---------------------------------------------------------------------------------------------------------------- d. storages
@pytest.mark.parametrize("storage", [dict(weight_dtype="h1"), dict(weight_dtype="h2"), dict(weight_dtype="f32"), dict(kv_dtype="f8s")],
                         ids=["h1", "h2", "f32", "kv_f8s"])
def test_storages(model, storage):
    old = {k: getattr(model.sampler, k) for k in storage}
    try:
        for k, v in storage.items():
            setattr(model.sampler, k, v)                               # the sampler packs a new engine for it
        eng = model.sampler.engine()
        assert all(getattr(eng, {"weight_dtype": "wdtype"}.get(k, k)) == v for k, v in storage.items())
        B, T = 2, 43
        frames = frames_of(B)
        ref = model.generate(frames=frames, max_new_tokens=T, return_sampled_indices=True, prompt_is_encoded=True, **GREEDY)
        blocks = list(model.generate_stream(frames=frames, max_new_tokens=T, prompt_is_encoded=True, block_frames=16, **GREEDY))
        assert len(blocks) == 3
        assert torch.equal(torch.cat([b["sampled_indices"] for b in blocks], -1), ref["sampled_indices"])
        assert torch.equal(torch.cat([b["audio"] for b in blocks], -1), ref["generated_audio"])
    finally:
        for k, v in old.items():
            setattr(model.sampler, k, v)


# ---------------------------------------------------------------------------------------------------------------- e. early close
def test_closing_early_leaves_the_engine_reusable(model):
    B, T = 2, 43
    frames = frames_of(B)
    ref = reference(model, "sampled_cfg3", frames=frames, max_new_tokens=T, **SAMPLED)
    it = model.generate_stream(frames=frames, max_new_tokens=T, prompt_is_encoded=True, block_frames=4, **SAMPLED)
    first = next(it)
    it.close()                                                         # two pieces of the loop may still be running
    again = model.generate(frames=frames, max_new_tokens=T, return_sampled_indices=True, prompt_is_encoded=True, **SAMPLED)
    assert torch.equal(again["sampled_indices"], ref["sampled_indices"]) and torch.equal(again["generated_audio"], ref["generated_audio"])
    assert torch.equal(first["audio"], ref["generated_audio"][..., :first["frames"] * HOP])
    model.sampler.engine().check_status()                              # and nothing is left in the status word


# ---------------------------------------------------------------------------------------------------------------- f. long form
@pytest.mark.parametrize("way", [GREEDY, dict(use_sampling=True, temp=0.9, top_k=128, cfg_scale=3.0)], ids=["greedy", "sampled_cfg3"])
def test_long_stream_releases_inside_the_chunks(model, way):
    B = 2
    feats = synth.video_features(B, tokens=6 * 8, seed=71).reshape(B, 6, 8, 768).to(DEV)      # tests/test_gpu_codec_window.py: 3 chunks
    ref = longform.generate_long(model, feats, 3.84, **way)
    assert ref["sampled_indices"].shape[-1] == 331
    blocks = list(longform.generate_long_stream(model, feats, 3.84, block_frames=16, **way))
    assert blocks[0]["start_frame"] == 0 and blocks[0]["frames"] < 211
    assert blocks[0]["frames"] == 16 - H                                # 16 final frames, all but the halo
    at = 0
    for blk in blocks:
        assert blk["start_frame"] == at and blk["frames"] > 0
        at += blk["frames"]
    assert at == 331 and [b["final"] for b in blocks] == [False] * (len(blocks) - 1) + [True]
    print(f"{len(blocks)} blocks, frames {[b['frames'] for b in blocks]}")
    assert torch.equal(torch.cat([b["sampled_indices"] for b in blocks], -1), ref["sampled_indices"])
    assert torch.equal(torch.cat([b["audio"] for b in blocks], -1), ref["generated_audio"])


def test_long_stream_single_chunk_and_relevance(model):
    B = 2
    one = synth.video_features(B, tokens=4 * 8, seed=71).reshape(B, 4, 8, 768).to(DEV)
    kw = dict(use_sampling=True, temp=0.9, top_k=128, cfg_scale=1.0, return_relevance=True)
    ref = longform.generate_long(model, one, 0.5, **kw)
    blocks = list(longform.generate_long_stream(model, one, 0.5, block_frames=16, **kw))
    assert [b["frames"] for b in blocks] == [6, 16, 21] and blocks[-1]["final"]
    for k in REL + ("sampled_indices",):
        assert torch.equal(torch.cat([b[k] for b in blocks], -1), ref[k]), k
    assert torch.equal(torch.cat([b["audio"] for b in blocks], -1), ref["generated_audio"])


# ---------------------------------------------------------------------------------------------------------------- g. the status rule
# Through the host's read of the status words only (DecoderEngine._stream_status): the device word stays clean, nothing overflows and no
# hand-off gives up.
@pytest.fixture()
def engine(tiny_sampler_sd):
    return DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype="h1")


def status_at(eng, monkeypatch, call, value):
    """the `call`-th read of the status words (0-based) answers `value`, every other read the truth"""
    real, n = eng._stream_status, [0]

    def fake(words):
        n[0] += 1
        return value if n[0] - 1 == call else real(words)
    monkeypatch.setattr(eng, "_stream_status", fake)


def run_stream(eng, feats, **kw):
    it = eng.generate_codes_stream(feats, 43, block_frames=16, halo=H, **kw)
    ranges = []
    while True:
        try:
            ranges.append(next(it))
        except StopIteration as stop:
            return ranges, stop.value


def test_status_before_the_first_block_falls_back_and_streams_on(engine, monkeypatch):
    feats = synth.video_features(2, tokens=TV, seed=31).to(DEV)
    want = engine.generate_codes(feats, 43).clone()
    plain, codes = run_stream(engine, feats)
    assert torch.equal(codes, want) and engine.stream_engine is engine
    assert plain == [[(0, 16)] * 2, [(16, 32)] * 2, [(32, 43)] * 2]
    # bit 2, a hand-off that gave up: the separate launches, the same bits
    status_at(engine, monkeypatch, 0, 2)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ranges, codes = run_stream(engine, feats)
    assert any("separate launches" in str(x.message) for x in w)
    assert ranges == plain and torch.equal(codes, want)
    assert engine.one_launch_mlp is False and engine.handoff_fallbacks == 1 and engine.stream_engine is engine
    # bit 1, non-finite logits: the exact-fp32 twin with the same arguments; the ranges refer to ITS sequence
    status_at(engine, monkeypatch, 0, 1)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ranges, codes = run_stream(engine, feats)
    assert any("exact-fp32 twin" in str(x.message) for x in w)
    twin = engine._twin()
    assert engine.range_fallbacks == 1 and engine.stream_engine is twin and twin.wdtype == "f32"
    assert ranges == plain and torch.equal(codes, twin.generate_codes(feats, 43))
    engine.check_status()                                              # the device word never held a bit


def test_status_after_a_block_raises_with_what_has_left(engine, monkeypatch):
    feats = synth.video_features(2, tokens=TV, seed=31).to(DEV)
    status_at(engine, monkeypatch, 1, 1)
    it = engine.generate_codes_stream(feats, 43, block_frames=16, halo=H)
    assert next(it) == [(0, 16)] * 2
    with pytest.raises(L.VauraHipError, match="cannot be taken back") as e:
        next(it)
    assert e.value.status == 1 and e.value.frames_emitted == [16, 16]
    assert engine.range_fallbacks == 0                                 # no silent re-run behind audio that is out
    monkeypatch.undo()
    assert torch.equal(engine.generate_codes(feats, 43), run_stream(engine, feats)[1])      # the engine is reusable
    engine.check_status()


def status_once(eng, monkeypatch, st):
    """the next check_status of `eng` reads (and clears) the true word, then raises the error of status word `st`; later ones are the real ones"""
    real, done = eng.check_status, []

    def fake():
        real()
        if not done:
            done.append(st)
            raise DecoderEngine._status_error(st)
    monkeypatch.setattr(eng, "check_status", fake)


def fallback_warnings(w):
    return [str(x.message) for x in w if "separate launches" in str(x.message) or "exact-fp32 twin" in str(x.message)]


def test_checked_call_and_stream_share_one_fallback(engine, tiny_sampler_sd, monkeypatch):
    """generate_codes_checked and the stream leave a dirty status word through ONE method (DecoderEngine._status_fallback): the same
    switches, counters and warning texts.  The status is faked on the host (check_status / _stream_status), the device word stays clean."""
    feats = synth.video_features(2, tokens=TV, seed=31).to(DEV)
    want = engine.generate_codes(feats, 43).clone()
    engine.check_status()
    texts = {}
    for st, word in ((2, "separate launches"), (1, "exact-fp32 twin")):
        status_once(engine, monkeypatch, st)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            got = engine.generate_codes_checked(feats, 43)
        texts[st] = fallback_warnings(w)
        assert len(texts[st]) == 1 and word in texts[st][0], texts[st]                   # the one warning, once
        if st == 2:                                                                      # this engine again, on the separate launches
            assert torch.equal(got, want) and engine.one_launch_mlp is False and engine.handoff_fallbacks == 1 and engine.range_fallbacks == 0
        else:                                                                            # the twin's tokens
            assert engine.range_fallbacks == 1 and engine.handoff_fallbacks == 1
            assert torch.equal(got, engine._twin().generate_codes(feats, 43))
    engine.check_status()
    assert torch.equal(engine.generate_codes_checked(feats, 43), want) and engine.range_fallbacks == 1      # a clean call: no fallback
    # the stream of a fresh engine of the same model under the same faked status: the checked path's texts, word for word
    fresh = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype="h1")
    for st in (2, 1):
        status_at(fresh, monkeypatch, 0, st)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            run_stream(fresh, feats)
        assert fallback_warnings(w) == texts[st]
    assert fresh.one_launch_mlp is False and fresh.handoff_fallbacks == 1 and fresh.range_fallbacks == 1
    fresh.check_status()
