"""Live video in (vaura_amd/live.py, VAURAModel.open_live, DecoderEngine.append_condition, csrc/step.hip vaura_cond_window): segments
are pushed into a session while audio streams out.

Every comparison is torch.equal — the session runs the kernel instances of the calls it is compared with, on the same rows, and adds
one small kernel that moves and writes condition rows.  What can go wrong is bookkeeping: a step that runs ahead of the video (the
not-yet-received condition rows are NaN, so that shows as a dirty status word or a changed token), a prompt cut at the wrong frame, a
block boundary off by one.

Shapes: the tiny plugin model (2 layers, 9 codebooks, delays 0..8) with the full-size synthetic codec, B = 2, six segments of
synthetic features (three chunks, 331 frames).  The references are computed once per module and left unchanged."""
import ctypes as C
import os
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_per_clip_sampling as G  # noqa: E402  (the tiny plugin model)
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import clip_params, live, longform, synth  # noqa: E402
from vaura_amd.codec_clips import decode_halo  # noqa: E402
from vaura_amd.engine import DecoderEngine  # noqa: E402
from vaura_amd.post import PcmFormat, PcmStream, audio_to_pcm  # noqa: E402

DEV = "cuda:0"
HOP = synth.FULL_CODEC.hop
H = decode_halo(synth.FULL_CODEC)
B, K, TV, SEG, TPF = 2, 9, 32, 8, 7
REL = ("relevance", "logprob_cond", "logprob_null")
GREEDY = dict(use_sampling=False, cfg_scale=1.0)
SAMPLED = dict(use_sampling=True, temp=0.9, top_k=128, cfg_scale=3.0)
WAYS = {"greedy": GREEDY, "sampled_cfg3": SAMPLED}
PLAN = live.live_plan()
T0 = PLAN["first"]


@pytest.fixture(scope="module")
def model(tiny_sampler_sd):
    return G._model(tiny_sampler_sd)


@pytest.fixture(scope="module")
def feats():
    return synth.video_features(B, tokens=6 * SEG, seed=71).reshape(B, 6, SEG, 768).to(DEV)


REF = {}


def long_reference(model, feats, S, name, **kw):
    """generate_long over the first S segments, once per module"""
    if (name, S) not in REF:
        r = longform.generate_long(model, feats[:, :S], 0.64 * S, **kw)
        REF[(name, S)] = {k: v.clone() for k, v in r.items()}
    return REF[(name, S)]


def run_session(model, feats, S, block_frames, **kw):
    """push S segments, close -> (the blocks in order, the number of blocks every call returned)"""
    s = model.open_live(B, block_frames=block_frames, **kw)
    blocks, per_call = [], []
    for i in range(S):
        got = s.push(features=feats[:, i:i + 1]) if i % 2 else s.push(features=feats[:, i])      # both accepted layouts
        per_call.append(len(got))
        blocks += got
    got = s.close()
    per_call.append(len(got))
    return blocks + got, per_call


def joined(blocks, key):
    at = 0
    for blk in blocks:
        assert blk["start_frame"] == at and blk["frames"] > 0 and blk["sampled_indices"].shape[-1] == blk["frames"]
        assert blk["audio"].shape[-1] == blk["frames"] * HOP
        at += blk["frames"]
    assert [b["final"] for b in blocks] == [False] * (len(blocks) - 1) + [True]
    return torch.cat([b[key] for b in blocks], dim=-1)


def check_audio_is_one_decode(model, blocks):
    """contract (b): the concatenated audio is the codec's decode of the session's own tokens as one clip of that length"""
    tokens = joined(blocks, "sampled_indices")
    want = model.audio_encoder.decode([(tokens[..., :K, :], None)])
    assert torch.equal(joined(blocks, "audio"), want)
    return tokens


# ---------------------------------------------------------------------------------------------------------------- 1. the op
@pytest.mark.parametrize("cfg_on", [False, True], ids=["no_cfg", "cfg"])
def test_condition_window_in_place(tiny_sampler_sd, feats, cfg_on):
    eng = DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype="h1")
    flat = feats.reshape(B, 6 * SEG, 768)

    def whole(lo):                                                     # set_condition on the segments lo .. lo + 3
        eng.set_condition(flat[:, lo * SEG:(lo + 4) * SEG].contiguous())
        return eng.cond_projection().clone()
    eng.prepare(B, T0, TV, cfg_on, TPF, eng.cfg.block_size)
    want_14, want_03 = whole(1), whole(0)
    assert eng.cond_projection().shape == ((2 * B if cfg_on else B), TV, eng.cfg.cond_dim)
    # the window slides: segments 0..3, then shift by one segment and write segment 4 behind them
    eng.append_condition(flat[:, 4 * SEG:5 * SEG], first_token=3 * SEG, shift_tokens=SEG)
    assert torch.equal(eng.cond_projection(), want_14)
    # four appends into a NaN-filled buffer: the not-yet-received rows stay NaN until their segment arrives
    eng.cond_proj.fill_(float("nan"))
    for i in range(4):
        eng.append_condition(flat[:, i * SEG:(i + 1) * SEG], first_token=i * SEG)
        got = eng.cond_projection()
        assert torch.equal(got[:, :(i + 1) * SEG], want_03[:, :(i + 1) * SEG])
        assert bool(torch.isnan(got[:, (i + 1) * SEG:]).all())
    assert torch.equal(eng.cond_projection(), want_03)
    # refusals, by their status codes; nothing is launched
    lib, new = eng.lib, eng._live_bufs[("new", B * SEG)][2]
    null = L.ptr(eng._live_null) if cfg_on else 0
    args = lambda **kw: (kw.get("dec", C.byref(eng.dec)), kw.get("new", L.ptr(new)), kw.get("null", null), kw.get("shift", 0),
                         kw.get("first", 0), kw.get("n", SEG), L.current_stream(eng.dev))
    assert lib.vaura_cond_window(*args(first=3 * SEG)) == 0                 # segment 3 once more, where it stands
    assert lib.vaura_cond_window(*args(dec=None)) == -1
    assert lib.vaura_cond_window(*args(new=0)) == -1
    assert lib.vaura_cond_window(*args(n=0)) == -1 and lib.vaura_cond_window(*args(shift=-1)) == -1
    if cfg_on:
        assert lib.vaura_cond_window(*args(null=0)) == -1
    assert lib.vaura_cond_window(*args(first=TV - SEG + 1)) == -2      # first_token + n_tokens > Tv
    assert lib.vaura_cond_window(*args(shift=TV + 1)) == -2
    odd = L.DecoderExt3.from_buffer_copy(eng.dec_ext3)
    odd.ext2.ext.dec.dims.cond_dim = eng.cfg.cond_dim + 2
    assert lib.vaura_cond_window(*args(dec=C.byref(odd.ext2.ext.dec))) == -2
    torch.cuda.synchronize()
    assert torch.equal(eng.cond_projection(), want_03)                 # the refused calls wrote nothing


# ---------------------------------------------------------------------------------------------------------------- 2. contract (a) + (b)
@pytest.mark.parametrize("block_frames", [16, 7])
@pytest.mark.parametrize("name", list(WAYS))
def test_long_session_is_the_long_form_stream(model, feats, name, block_frames):
    ref = long_reference(model, feats, 6, name, **WAYS[name])
    assert ref["sampled_indices"].shape[-1] == 331
    blocks, per_call = run_session(model, feats, 6, block_frames, **WAYS[name])
    print(f"{name}, block_frames {block_frames}: blocks per call {per_call}, first block {blocks[0]['frames']} frames")
    assert per_call[0] > 0, "the first audio is due after ONE segment"
    book = live.LiveBook(PLAN, list(range(K)), block_frames, TPF, SEG, H)
    assert per_call[:-1] == [len(book.push()[1]) for _ in range(6)]
    tokens = check_audio_is_one_decode(model, blocks)
    assert torch.equal(tokens, ref["sampled_indices"])
    assert torch.equal(joined(blocks, "audio"), ref["generated_audio"])
    model.sampler.engine().check_status()


def test_long_session_relevance(model, feats):
    kw = dict(SAMPLED, return_relevance=True)
    ref = long_reference(model, feats, 6, "sampled_cfg3_relevance", **kw)
    blocks, _ = run_session(model, feats, 6, 16, **kw)
    for k in ("sampled_indices",) + REL:
        assert torch.equal(joined(blocks, k), ref[k]), k
    assert torch.equal(joined(blocks, "audio"), ref["generated_audio"])


# ---------------------------------------------------------------------------------------------------------------- 3. contract (c)
@pytest.mark.parametrize("name", list(WAYS))
@pytest.mark.parametrize("S", [1, 2, 3])
def test_closing_inside_chunk_0_is_causal(model, feats, S, name):
    """The session's frames are the prefix of generate_stream on the received segments followed by NaN segments — as long as the
    bound says.  The reference stream is read in blocks of 8 frames (48, 104 and 160 are multiples) and closed where the prefix ends:
    the piece behind it reads NaN condition rows, which leaves the status bit that is then read and cleared."""
    n = clip_params.final_frames(clip_params.video_step_bound(S * SEG, TV, TPF, 1, T0 + K), T0, 1, K - 1)
    assert n == {1: 48, 2: 104, 3: 160}[S]
    blocks, per_call = run_session(model, feats, S, 16, **WAYS[name])
    assert per_call[0] > 0
    tokens = check_audio_is_one_decode(model, blocks)
    assert tokens.shape[-1] == n
    eng = model.sampler.engine()
    eng.check_status()                                                 # the session itself never read ahead of its video
    nan4 = torch.cat([feats[:, :S], torch.full_like(feats[:, :4 - S], float("nan"))], dim=1)
    it = model.generate_stream(frames=nan4, max_new_tokens=T0, prompt_is_encoded=True, block_frames=8, decode=False, **WAYS[name])
    want = []
    for blk in it:
        want.append(blk["sampled_indices"])
        if blk["start_frame"] + blk["frames"] == n:
            break
    it.close()
    torch.cuda.synchronize()
    try:
        eng.check_status()
    except L.VauraHipError as e:                                       # the reference's pieces in flight read the NaN rows
        assert e.status == 1
    assert torch.equal(tokens, torch.cat(want, dim=-1))


# ---------------------------------------------------------------------------------------------------------------- 4. one value per clip
def test_per_clip_parameters(model, feats):
    kw = dict(use_sampling=[True, True], temp=[0.9, 1.1], top_k=[128, 64], cfg_scale=[3.0, 1.0])
    ref = long_reference(model, feats, 5, "per_clip", **kw)
    assert ref["sampled_indices"].shape[-1] == 276
    blocks, _ = run_session(model, feats, 5, 16, **kw)
    assert torch.equal(check_audio_is_one_decode(model, blocks), ref["sampled_indices"])
    assert torch.equal(joined(blocks, "audio"), ref["generated_audio"])


# ---------------------------------------------------------------------------------------------------------------- 5. contract (d)
def test_frames_and_features_of_a_segment_are_one_push(model):
    """push(frames=seg) is push(features=extractor(seg)) with the extractor called on that one segment at the session's batch.  Whether
    the extractor on (B, 1) segments gives the rows of its (B, 4) call is measured and recorded, not asserted: other row counts may
    select other kernel instances."""
    fx = model.visual_feature_extractor
    fx.extract_features = True
    fx.load_state_dict(synth.avclip_state_dict(seed=0), strict=True)
    fx.to(DEV)
    video = synth.video_frames(B, 4, seed=5).to(DEV)                   # (B, 4, 3, 16, 224, 224)
    seg = video[:, :1].contiguous()
    one, _ = fx(seg)
    assert one.shape == (B, 1, SEG, 768)
    got = {}
    for key, kw in (("frames", dict(frames=seg)), ("features", dict(features=one))):
        s = model.open_live(B, block_frames=16, **GREEDY)
        got[key] = s.push(**kw) + s.close()
    assert len(got["frames"]) == len(got["features"]) > 1
    for x, y in zip(got["frames"], got["features"]):
        assert torch.equal(x["sampled_indices"], y["sampled_indices"]) and torch.equal(x["audio"], y["audio"])
    four, _ = fx(video)
    diff = float((four[:, :1] - one).abs().max())
    line = (f"extractor on (B={B}, 1) segment vs the slice of its (B={B}, 4) call, tiny-decoder test configuration: "
            f"{'bit-equal' if torch.equal(four[:, :1], one) else 'NOT bit-equal'}, max |diff| = {diff:.3e}")
    print("live_parity:", line)
    out = os.environ.get("VAURA_PARITY_DIR")                           # printed always; kept in live_parity.txt when that is set
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "live_parity.txt"), "w") as f:
            f.write("live session, contract (d): the extractor on (B, 1) segments against the rows of its (B, 4) call — measured, "
                    "asserted nowhere (tests/test_gpu_live.py; tools/time_live.py --parity appends the 8-clip line)\n" + line + "\n")


# ---------------------------------------------------------------------------------------------------------------- 6. the status rule
# Through the host's read of the status words only (DecoderEngine._stream_status), as tests/test_gpu_generate_stream.py section g: the
# device word stays clean, nothing overflows and no hand-off gives up.
@pytest.fixture()
def own_model(tiny_sampler_sd):
    return G._model(tiny_sampler_sd)                                   # the fallbacks switch its engine for good


def status_at(eng, monkeypatch, call, value):
    """the `call`-th read of the status words (0-based) answers `value`, every other read the truth"""
    real, n = eng._stream_status, [0]

    def fake(words):
        n[0] += 1
        return value if n[0] - 1 == call else real(words)
    monkeypatch.setattr(eng, "_stream_status", fake)


def test_status_before_the_first_block_reruns_and_continues(own_model, feats, monkeypatch):
    model = own_model
    eng = model.sampler.engine()
    plain, _ = run_session(model, feats, 2, 16, **GREEDY)
    want = joined(plain, "sampled_indices")
    # bit 2 on the second piece of a session whose first block needs two (block_frames 4: 4 final frames hold no releasable one)
    status_at(eng, monkeypatch, 1, 2)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        blocks, _ = run_session(model, feats, 2, 4, **GREEDY)
    assert any("separate launches" in str(x.message) for x in w)
    assert eng.one_launch_mlp is False and eng.handoff_fallbacks == 1
    assert torch.equal(check_audio_is_one_decode(model, blocks), want)
    monkeypatch.undo()
    # bit 1 on the very first piece: the exact-fp32 twin, from the start of the session
    status_at(eng, monkeypatch, 0, 1)
    s = model.open_live(B, block_frames=16, **GREEDY)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        blocks = s.push(features=feats[:, 0]) + s.close()
    assert any("exact-fp32 twin" in str(x.message) for x in w)
    twin = eng._twin()
    assert eng.range_fallbacks == 1 and s._eng is twin and twin.wdtype == "f32"
    nan4 = torch.cat([feats[:, :1], torch.full_like(feats[:, :3], float("nan"))], dim=1).reshape(B, TV, 768)
    it = twin.generate_codes_stream(nan4, T0, block_frames=48)
    assert next(it) == [(0, 48)] * B
    ref = twin.stream_frames(twin.seq, [(0, 48)] * B, model.special_token_id).to(torch.int64)
    it.close()
    torch.cuda.synchronize()
    twin.state[4:5].zero_()                                            # what the reference's piece in flight left (it read NaN rows)
    assert torch.equal(check_audio_is_one_decode(model, blocks), ref)
    eng.check_status()                                                 # the device word of the session's engine never held a bit


def test_status_after_a_block_raises_with_what_has_left(own_model, feats, monkeypatch):
    model = own_model
    eng = model.sampler.engine()
    frames = feats[:, :4].reshape(B, 1, TV, 768)
    want = model.generate(frames=frames, max_new_tokens=43, return_sampled_indices=True, prompt_is_encoded=True, **GREEDY)
    want = {k: want[k].clone() for k in ("sampled_indices", "generated_audio")}
    status_at(eng, monkeypatch, 1, 1)                                  # block_frames 16: the first piece releases 16 - H frames
    s = model.open_live(B, block_frames=16, **GREEDY)
    with pytest.raises(L.VauraHipError, match="cannot be taken back") as e:
        s.push(features=feats[:, 0])
    assert e.value.status == 1 and e.value.frames_emitted == [16 - H] * B
    assert eng.range_fallbacks == 0                                    # no silent re-run behind audio that is out
    with pytest.raises(L.VauraHipError, match="open a new one"):
        s.push(features=feats[:, 1])
    monkeypatch.undo()
    again = model.generate(frames=frames, max_new_tokens=43, return_sampled_indices=True, prompt_is_encoded=True, **GREEDY)
    assert all(torch.equal(again[k], want[k]) for k in want)           # the engine is reusable
    eng.check_status()


# ---------------------------------------------------------------------------------------------------------------- 7. reuse
def test_engine_is_reusable_after_a_session(model, feats):
    frames = feats[:, :4].reshape(B, 1, TV, 768)
    want = model.generate(frames=frames, max_new_tokens=T0, return_sampled_indices=True, prompt_is_encoded=True, **SAMPLED)
    want = {k: want[k].clone() for k in ("sampled_indices", "generated_audio")}
    s = model.open_live(B, block_frames=16, **SAMPLED)
    s.push(features=feats[:, 0])
    s.push(features=feats[:, 1])
    s.close()
    with pytest.raises(L.VauraHipError, match="after close"):
        s.push(features=feats[:, 2])
    with pytest.raises(L.VauraHipError, match="after close"):
        s.close()
    for dropped in (False, True):
        if dropped:                                                    # a session dropped without close(): NaN rows stay in the buffer
            s = model.open_live(B, block_frames=16, **SAMPLED)
            s.push(features=feats[:, 0])
        got = model.generate(frames=frames, max_new_tokens=T0, return_sampled_indices=True, prompt_is_encoded=True, **SAMPLED)
        assert all(torch.equal(got[k], want[k]) for k in want), dropped
        model.sampler.engine().check_status()
    with pytest.raises(L.VauraHipError, match="another call has used"):       # generate() took the engine inside the session's chunk 0
        s.push(features=feats[:, 1])


def test_push_refusals_on_a_session(model, feats):
    s = model.open_live(B, block_frames=16, **GREEDY)
    with pytest.raises(L.VauraHipError, match="one segment is"):
        s.push(features=feats[:, :2])
    with pytest.raises(L.VauraHipError, match="not both and not neither"):
        s.push()
    with pytest.raises(L.VauraHipError, match="num_candidates = 1"):
        model.open_live(B, num_candidates=2)
    with pytest.raises(L.VauraHipError, match="live clock"):
        model.open_live(B, video_lengths=[32, 8])
    assert s.close() == []                                             # nothing was pushed: nothing to emit


# ---------------------------------------------------------------------------------------------------------------- 8. PCM hand-over
def test_blocks_go_to_the_pcm_stream_unchanged(model, feats):
    fmt = PcmFormat()
    blocks, _ = run_session(model, feats, 5, 16, **GREEDY)
    want, n_out = audio_to_pcm(joined(blocks, "audio"), fmt)
    stream = PcmStream(fmt, B, DEV)
    parts = [[] for _ in range(B)]
    for blk in blocks:
        pcm, counts = stream.push(blk["audio"], final=blk["final"])
        for b in range(B):
            parts[b].append(pcm[b, :counts[b]])
    for b in range(B):
        got = torch.cat(parts[b])
        assert got.shape[0] == int(n_out[b]) and torch.equal(got, want[b, :int(n_out[b])]), b
