"""Sliding-window generation for clips of different durations in one call: longform.generate_long_clips (one generate_tokens call
per chunk index over the per-clip lengths, finished clips parked), generate_tokens(video_segments=...), one decode_clips pass.

The contract is bit equality: clip b of the batched call, over its own frames [0, L_b), is what generate_long with clip b's duration
gives on the SAME batch with the same keywords — every comparison is torch.equal, nothing has a tolerance.

Tiny model of tests/test_gpu_per_clip_sampling.py (pass-through MotionFormer, synthetic codec, Philox noise), features (6, 4, 4, 768):
4 segments of 4 tokens, so positions wrap; 0.30 s window, 0.10 s stride, 440 video frames per second: 26-frame window, 8-frame stride,
18-frame prompt, 8 segments = 32 video tokens per full chunk.  Durations [0.62, 0.27, 0.45, 0.50, 0.31, 0.40]: 5 / 1 / 3 / 4 / 1 / 2
chunks — a last chunk of 22 frames over 7 segments, the single-chunk branch, a last chunk that generates ONE frame over 6 segments,
one chunk through the loop branch, and clips parked behind the longest.

Guidance and relevance (doubled rows).  The engine takes the null rows only at as many video tokens as the null embedding holds (32),
so generate_long itself REFUSES — under cfg_scale > 1 or return_relevance — every duration here with a chunk of fewer than 8 segments
(0.62, 0.27, 0.45, 0.50; the reference's own broadcast fails there as well).  generate_long_clips runs every call 8 segments wide and
serves such a clip through the per-clip video length.  For those durations there is no generate_long result to compare with, so the
tests (a) check that generate_long does refuse them, which keeps this note honest, and (b) compare with `wide_long` below: the same
one-duration loop, on the same batch with the same keywords, over generate_tokens calls 8 segments wide with video_lengths — which the
greedy cfg-1 case pins to generate_long bit for bit for every duration.  0.31 and 0.40 are compared with generate_long itself."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_per_clip_sampling as G  # noqa: E402  (the tiny plugin model, P / columns)
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import longform, post, synth  # noqa: E402

DEV = "cuda:0"
B, K, S_SEG, T_SEG, WIDTH = 6, 9, 4, 4, 8
GEO = dict(stride=0.10, model_max_duration=0.30, vfps=440)
DURATIONS = [0.62, 0.27, 0.45, 0.50, 0.31, 0.40]
LENGTHS = [54, 23, 39, 43, 26, 34]
REL = ("relevance", "logprob_cond", "logprob_null")
P, columns = G.P, G.columns

GREEDY = dict(use_sampling=False, cfg_scale=1.0)
SAMPLED = dict(use_sampling=True, temp=0.9, top_k=128, cfg_scale=1.0)
SAMPLED_CFG3 = dict(use_sampling=True, temp=0.9, top_k=128, cfg_scale=3.0)
MIX = columns([P(False, cfg_scale=1.0), P(True, 0.8, 50, cfg_scale=3.0), P(True, 1.2, 0, cfg_scale=1.0), P(True, 0.7, 128, cfg_scale=6.0),
               P(False, cfg_scale=2.0), P(True, 1.0, 250, cfg_scale=1.0)])
WAYS = {"greedy": GREEDY, "sampled": SAMPLED, "sampled_cfg3": SAMPLED_CFG3, "per_clip_mix": MIX}
DOUBLED = {"greedy": False, "sampled": False, "sampled_cfg3": True, "per_clip_mix": True}


@pytest.fixture(scope="module")
def model(tiny_sampler_sd):
    return G._model(tiny_sampler_sd)


@pytest.fixture(scope="module")
def feats():
    return synth.video_features(B, tokens=S_SEG * T_SEG, seed=71).reshape(B, S_SEG, T_SEG, 768).to(DEV)


def schedule(d):
    return longform.chunk_schedule(d, GEO["model_max_duration"], GEO["stride"], GEO["vfps"])


def has_short_chunk(d, S=S_SEG):
    return any((S if ch["positions"] is None else ch["positions"][1] - ch["positions"][0]) != WIDTH for ch in schedule(d))


def wide_long(model, frames, d, return_relevance=False, **kw):
    """generate_long for ONE duration, every call WIDTH segments wide: a chunk that selects fewer repeats its last segment behind them
    and says so in video_lengths (a chunk of WIDTH segments is the plain call generate_long makes)."""
    S = frames.shape[1]
    stride_tokens = int(longform.COMPRESSION_MODEL_FRAME_RATE * GEO["stride"])
    pieces, prompt = {k: [] for k in ("tokens",) + (REL if return_relevance else ())}, None
    for ch in schedule(d):
        idx = list(range(S)) if ch["positions"] is None else [p % S for p in range(*ch["positions"])]
        n = len(idx)
        sel = frames[:, idx + [idx[-1]] * (WIDTH - n)]
        out = model.generate_tokens(frames=sel, audio=prompt, max_new_tokens=ch["max_gen_len"], remove_prompts=False, prompt_is_encoded=True,
                                    **(dict(video_lengths=[n * T_SEG] * frames.shape[0]) if n != WIDTH else {}),
                                    **(dict(return_relevance=True) if return_relevance else {}), **kw)
        out = out if isinstance(out, dict) else {"tokens": out}
        Tp = 0 if prompt is None else prompt.shape[-1]
        for k in pieces:
            pieces[k].append(out[k][:, :, Tp:])
        prompt = out["tokens"][:, :, stride_tokens:]
    r = {k: torch.cat(v, dim=-1) for k, v in pieces.items()}
    r["sampled_indices"] = r.pop("tokens")
    return r


_refs = {}


def reference(model, frames, d, way, doubled, return_relevance=False, tag=""):
    """generate_long(model, frames, d, ...) on the same batch with the same keywords — computed once; where it refuses the duration
    (doubled rows and a chunk of fewer than WIDTH segments: see the module docstring), checked to refuse and replaced by wide_long."""
    key = (way, d, return_relevance, tag)
    if key not in _refs:
        kw = dict(WAYS[way], **(dict(return_relevance=True) if return_relevance else {}))
        if doubled and has_short_chunk(d, frames.shape[1]):
            with pytest.raises(L.VauraHipError, match="CFG null embedding has 32 tokens"):
                longform.generate_long(model, frames, d, **GEO, **kw)
            _refs[key] = wide_long(model, frames, d, **kw)
        else:
            _refs[key] = longform.generate_long(model, frames, d, **GEO, **kw)
    return _refs[key]


_got = {}


def batched(model, feats, way, **extra):
    key = (way, tuple(sorted(extra)))
    if key not in _got:
        _got[key] = longform.generate_long_clips(model, feats, DURATIONS, **GEO, **WAYS[way], **extra)
    return _got[key]


def check_clip(got, ref, b, L_b, special):
    tok = got["sampled_indices"]
    assert ref["sampled_indices"].shape[-1] == L_b
    assert torch.equal(tok[b, :, :L_b], ref["sampled_indices"][b]), b
    assert bool((tok[b, :, L_b:] == special).all()) and bool((tok[b, :, :L_b] < special).all()), b


# ---------------------------------------------------------------------------------------------------------------- 1. tokens
@pytest.mark.parametrize("way", list(WAYS))
def test_tokens_of_every_clip_equal_generate_long_with_its_duration(model, feats, way):
    got = batched(model, feats, way)
    assert got["sampled_indices"].shape == (B, K, max(LENGTHS))
    assert torch.equal(got["lengths"].cpu(), torch.tensor(LENGTHS))
    for b, d in enumerate(DURATIONS):
        check_clip(got, reference(model, feats, d, way, DOUBLED[way]), b, LENGTHS[b], model.special_token_id)
    if way == "greedy":
        # the wide loop that stands in for generate_long where it refuses guidance IS generate_long where both run: every duration
        for d in DURATIONS:
            assert torch.equal(wide_long(model, feats, d, **GREEDY)["sampled_indices"],
                               reference(model, feats, d, way, False)["sampled_indices"]), d
    if way == "sampled":
        assert not torch.equal(got["sampled_indices"], batched(model, feats, "greedy")["sampled_indices"])


# ---------------------------------------------------------------------------------------------------------------- 2. audio
@pytest.mark.parametrize("way", ["greedy", "sampled_cfg3"])
def test_audio_of_every_clip_is_its_own_frames_decoded_alone(model, feats, way):
    got = batched(model, feats, way)
    tok, wav = got["sampled_indices"], got["generated_audio"]
    hop = wav.shape[-1] // tok.shape[-1]
    assert hop == 512 and wav.shape == (B, 1, max(LENGTHS) * hop)
    assert torch.equal(got["audio_lengths"], got["lengths"] * hop)
    for b, L_b in enumerate(LENGTHS):
        alone = model.audio_encoder.decode([(tok[b:b + 1, :K, :L_b], None)])
        assert torch.equal(wav[b:b + 1, :, :L_b * hop], alone), b
        assert bool((wav[b, :, L_b * hop:] == 0).all()), b


# ---------------------------------------------------------------------------------------------------------------- 3. relevance
def test_relevance_of_every_clip_equals_the_scalar_call(model, feats):
    got = batched(model, feats, "sampled", return_relevance=True)
    assert set(got) == {"generated_audio", "sampled_indices", "lengths", "audio_lengths", *REL}
    assert torch.equal(got["sampled_indices"], batched(model, feats, "sampled")["sampled_indices"])       # the flag does not change the tokens
    for b, d in enumerate(DURATIONS):
        ref = reference(model, feats, d, "sampled", True, return_relevance=True)          # relevance doubles the rows
        L_b = LENGTHS[b]
        check_clip(got, ref, b, L_b, model.special_token_id)
        for k in REL:
            assert got[k].shape == (B, K, max(LENGTHS))
            assert torch.equal(got[k][b, :, :L_b].view(torch.int32), ref[k][b].view(torch.int32)), (b, k)
            assert bool((got[k][b, :, L_b:] == 0).all()), (b, k)
        assert bool((got["relevance"][b, :, :L_b] != 0).any()), b


# ---------------------------------------------------------------------------------------------------------------- 4. segments
def test_segments_wrap_every_clip_at_its_own_count_and_nothing_behind_is_read(model, feats):
    segments = [4, 3, 4, 2, 4, 3]
    dirty = feats.clone()
    for b, n in enumerate(segments):
        dirty[b, n:] = float("nan")
    got = longform.generate_long_clips(model, dirty, DURATIONS, segments=segments, **GEO, **GREEDY)
    assert torch.equal(got["lengths"].cpu(), torch.tensor(LENGTHS))
    assert bool(torch.isfinite(got["generated_audio"]).all())
    for b, (d, n) in enumerate(zip(DURATIONS, segments)):
        ref = reference(model, feats[:, :n].contiguous(), d, "greedy", False, tag=f"S{n}")
        check_clip(got, ref, b, LENGTHS[b], model.special_token_id)
    full = batched(model, feats, "greedy")["sampled_indices"]
    assert not torch.equal(got["sampled_indices"][3], full[3])          # two segments instead of four: another video


# ---------------------------------------------------------------------------------------------------------------- 5. independence
def test_another_clips_duration_and_features_do_not_reach_a_clip(model, feats):
    base = batched(model, feats, "sampled")
    other = feats.clone()
    other[0] = synth.video_features(1, tokens=S_SEG * T_SEG, seed=5).reshape(S_SEG, T_SEG, 768).to(DEV)
    durations = [0.36] + DURATIONS[1:]         # the longest clip now ends after 2 chunks: 0.50 s is the longest, the batch runs 4 chunks
    got = longform.generate_long_clips(model, other, durations, **GEO, **SAMPLED)
    last = schedule(0.36)[-1]
    assert len(schedule(0.36)) == 2 and int(got["lengths"][0]) == last["offset"] + last["max_gen_len"]
    assert got["sampled_indices"].shape[-1] == 43
    hop = 512
    for b in range(1, B):
        L_b = LENGTHS[b]
        assert torch.equal(got["sampled_indices"][b, :, :L_b], base["sampled_indices"][b, :, :L_b]), b
        assert torch.equal(got["generated_audio"][b, :, :L_b * hop], base["generated_audio"][b, :, :L_b * hop]), b
    assert not torch.equal(got["sampled_indices"][0, :, :26], base["sampled_indices"][0, :, :26])


# ---------------------------------------------------------------------------------------------------------------- 6. equal durations
def test_equal_durations_give_generate_long_plus_the_lengths(model, feats):
    got = longform.generate_long_clips(model, feats[:3], [0.40] * 3, **GEO, **SAMPLED)
    ref = longform.generate_long(model, feats[:3], 0.40, **GEO, **SAMPLED)
    assert set(got) == {"generated_audio", "sampled_indices", "lengths", "audio_lengths"}
    assert torch.equal(got["sampled_indices"], ref["sampled_indices"]) and torch.equal(got["generated_audio"], ref["generated_audio"])
    assert got["lengths"].tolist() == [34] * 3 and got["audio_lengths"].tolist() == [34 * 512] * 3
    # ... and with `segments` the same clips go through the merged plan: the same bits (every clip has one length: the plain decode)
    planned = longform.generate_long_clips(model, feats[:3], [0.40] * 3, segments=[4, 4, 4], **GEO, **SAMPLED)
    assert torch.equal(planned["sampled_indices"], ref["sampled_indices"]) and torch.equal(planned["generated_audio"], ref["generated_audio"])
    assert planned["lengths"].tolist() == [34] * 3


# ---------------------------------------------------------------------------------------------------------------- 7. video_segments
def test_video_segments_is_video_lengths_in_segments(model, feats):
    # 7 sequence steps per video token: clips 2 and 5 (one segment = 4 tokens) leave their video at step 28, inside their T_b + 9 steps
    T, n_seg = [40, 5, 38, 9, 7, 36], [4, 3, 1, 2, 4, 1]
    kw = dict(frames=feats, max_new_tokens=T, prompt_is_encoded=True, top_k=128, return_logprobs=True)
    got = model.generate_tokens(video_segments=n_seg, **kw)
    ref = model.generate_tokens(video_lengths=[n * T_SEG for n in n_seg], **kw)
    assert set(got) == set(ref) and "tokens" in got and "lengths" in got
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    assert not torch.equal(got["tokens"], model.generate_tokens(frames=feats, max_new_tokens=T, prompt_is_encoded=True, top_k=128)["tokens"])
    plain = model.generate_tokens(frames=feats, max_new_tokens=40, video_segments=torch.tensor(n_seg), prompt_is_encoded=True, top_k=128)
    assert torch.equal(plain["tokens"], model.generate_tokens(frames=feats, max_new_tokens=40, video_lengths=[n * T_SEG for n in n_seg],
                                                              prompt_is_encoded=True, top_k=128)["tokens"])


# ---------------------------------------------------------------------------------------------------------------- 8. post stage
def test_post_stage_takes_the_result_as_it_is(model, feats, tmp_path):
    r = batched(model, feats, "greedy")
    out = post.normalize_audio(r["generated_audio"], strategy="peak", lengths=r["audio_lengths"])
    assert out.shape == r["generated_audio"].shape and bool(torch.isfinite(out).all())
    for b, n in enumerate(r["audio_lengths"].tolist()):
        assert bool((out[b, :, n:] == 0).all()), b
        assert bool((out[b, :, :n] != 0).any()), b
    paths = [str(tmp_path / f"clip{b}.wav") for b in range(B)]
    post.save_wavs(paths, out, r["audio_lengths"], sample_rate=44100)
    from scipy.io import wavfile
    for b, p in enumerate(paths):
        assert wavfile.read(p)[1].shape[0] == LENGTHS[b] * 512
