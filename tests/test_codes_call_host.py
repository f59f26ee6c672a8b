"""The resolved call record of DecoderEngine.generate_codes (clip_params.resolve_codes_call / CodesCall): what it resolves, what it
refuses, and that the defaults of generate_codes exist in its signature alone.  No GPU, no library."""
import dataclasses
import inspect

import pytest
import torch

from vaura_amd import _lib as L
from vaura_amd import clip_params
from vaura_amd.clip_params import resolve_codes_call
from vaura_amd.engine import DecoderEngine

B, TV = 2, 32
PER_CLIP = ("use_sampling", "temp", "top_k", "top_p", "cfg_scale")


@pytest.mark.parametrize("cfg_scale,cfg_on", [(1.0, False), (0.5, False), (3.0, True), (torch.tensor(3.0), True)])
def test_all_scalar(cfg_scale, cfg_on):
    c = resolve_codes_call(B, TV, 43, use_sampling=True, temp=0.7, top_k=64, cfg_scale=cfg_scale)
    assert c.lengths is None and c.P is None and c.tv_lengths is None and c.prompt_frames == 0
    assert c.cfg_on is cfg_on and c.t_max == 43 and (c.batch, c.n_video_tokens, c.num_candidates) == (B, TV, 1)
    assert not any(clip_params.is_per_clip(getattr(c, n)) for n in PER_CLIP)
    assert c.cfg_scale == float(cfg_scale) and not torch.is_tensor(c.cfg_scale)          # the record holds no tensor
    assert not c.want_logprobs and not c.want_relevance


def test_per_clip_lengths():
    c = resolve_codes_call(B, TV, [43, 23])
    assert c.t_max == 43 and c.lengths == [43, 23] and c.tv_lengths is None
    c = resolve_codes_call(B, TV, torch.tensor([43, 23]), video_lengths=(32, 7))
    assert c.t_max == 43 and c.lengths == [43, 23] and c.tv_lengths == [32, 7]


@pytest.mark.parametrize("temp", [[0.7, 1.0], (0.7, 1.0), torch.tensor([0.7, 1.0], dtype=torch.float64)])
def test_candidates_repeat_every_per_clip_list_in_row_order(temp):
    c = resolve_codes_call(B, TV, [43, 23], num_candidates=3, use_sampling=True, temp=temp, video_lengths=[32, 7],
                           prompt_frames=5, prompt_lengths=[2, 5])
    rows = [b for b in range(B) for _ in range(3)]                                          # row b * N + j belongs to clip b
    assert c.num_candidates == 3 and c.batch == B
    assert c.temp == [[0.7, 1.0][b] for b in rows]
    assert c.lengths == [[43, 23][b] for b in rows] and c.tv_lengths == [[32, 7][b] for b in rows] and c.P == [[2, 5][b] for b in rows]
    assert c.use_sampling is True and c.top_k == 0                                          # scalars next to it stay scalars
    assert all(not torch.is_tensor(v) for v in dataclasses.asdict(c).values())


@pytest.mark.parametrize("N", [1, 3])
def test_relevance_carries_the_null_rows_unmixed(N):
    c = resolve_codes_call(B, TV, 43, return_relevance=True, cfg_scale=1.0, num_candidates=N)
    assert c.cfg_on is True and c.want_relevance and not c.want_logprobs
    assert c.cfg_scale == [1.0] * (B * N) and all(type(x) is float for x in c.cfg_scale)
    c = resolve_codes_call(B, TV, 43, return_relevance=True, cfg_scale=[0.5, 1.0], num_candidates=N)      # per-clip already: its own values
    assert c.cfg_on is True and c.cfg_scale == [x for x in (0.5, 1.0) for _ in range(N)]
    c = resolve_codes_call(B, TV, 43, return_relevance=True, cfg_scale=3.0)                 # mixing anyway: the scalar stays
    assert c.cfg_on is True and c.cfg_scale == 3.0


def test_prompt_lengths():
    c = resolve_codes_call(B, TV, 43, 5)                                                    # a common prompt
    assert c.prompt_frames == 5 and c.P is None
    c = resolve_codes_call(B, TV, 43, 5, prompt_lengths=[5, 5])                             # one length after all: the common prompt
    assert c.prompt_frames == 5 and c.P is None
    c = resolve_codes_call(B, TV, 43, 5, prompt_lengths=[3, 3])
    assert c.prompt_frames == 3 and c.P is None
    c = resolve_codes_call(B, TV, 43, 5, prompt_lengths=[2, 5])
    assert c.P == [2, 5] and c.prompt_frames == 5
    c = resolve_codes_call(B, TV, 43, 5, prompt_lengths=[0, 0])                             # no prompt
    assert c.prompt_frames == 0 and c.P is None
    assert resolve_codes_call(B, TV, 43, None).prompt_frames == 0


@pytest.mark.parametrize("args,kw,match", [
    ((43,), dict(num_candidates=0), "num_candidates must be an int >= 1"),
    ((43,), dict(num_candidates=True), "num_candidates must be an int >= 1"),
    ((43,), dict(num_candidates=1.5), "num_candidates must be an int >= 1"),
    ((43,), dict(temp=[0.7, 1.0, 1.0]), "per-clip temp has 3 values for a batch of 2"),
    ((43,), dict(temp=[0.7, 1.0], top_k=[1, 2, 3]), "one value per clip"),
    (([43, 23, 9],), {}, "max_new_tokens has 3 values for a batch of 2"),
    (([43, 0],), {}, "at least 1"),
    ((43,), dict(video_lengths=[32, 33]), "video_lengths must lie in 1 .. 32"),
    ((43,), dict(video_lengths=[32]), "video_lengths has 1 values for a batch of 2"),
    (([43, 5], 5), {}, "must be shorter than every clip's max_new_tokens"),               # a common prompt against the shortest clip
    (([43, 23], 23), {}, "must be shorter than every clip's max_new_tokens"),
    ((43,), dict(prompt_lengths=[2, 5]), "needs an audio prompt"),
    ((43, 5), dict(prompt_lengths=[2, 6]), "must lie in 0 .. 5"),
    ((43, 5), dict(prompt_lengths=[2]), "prompt_lengths has 1 values for a batch of 2"),
    (([43, 5], 5), dict(prompt_lengths=[2, 5]), "audio prompt of clip 1 .5 frames. must be shorter than its max_new_tokens .5."),   # P_b >= T_b
    ((5, 5), dict(prompt_lengths=[2, 5]), "audio prompt of clip 1"),
])
def test_refusals_are_those_of_generate_codes(args, kw, match):
    with pytest.raises(L.VauraHipError, match=match):
        resolve_codes_call(B, TV, *args, **kw)


# ------------------------------------------------------------------------------------------------------------ the defaults exist once
def codes_keywords():
    params = inspect.signature(DecoderEngine.generate_codes).parameters.values()
    return {p.name: p.default for p in params if p.kind is p.KEYWORD_ONLY}


def test_defaults_are_those_of_the_signature():
    kw = {n: d for n, d in codes_keywords().items() if n not in ("prompt", "noise")}          # the two tensors are no part of the record
    assert kw and all(d is not inspect.Parameter.empty for d in kw.values())
    assert resolve_codes_call(B, TV, 43) == resolve_codes_call(B, TV, 43, None, **kw)
    changed = dict(kw, tokens_per_frame=kw["tokens_per_frame"] + 1)
    assert resolve_codes_call(B, TV, 43) != resolve_codes_call(B, TV, 43, None, **changed)


def test_stream_accepts_exactly_the_keywords_of_generate_codes():
    stream = inspect.signature(DecoderEngine.generate_codes_stream).parameters
    assert [n for n, p in stream.items() if p.kind is p.KEYWORD_ONLY] == ["block_frames", "halo"]
    assert any(p.kind is p.VAR_KEYWORD for p in stream.values())                              # the rest: the keywords of generate_codes
    eng = object.__new__(DecoderEngine)                                                       # no __init__: no library, no device
    eng.near_tie = "rerun"                                                                    # refused at call time, after the keywords are bound
    feats = torch.zeros(B, TV, 768)
    defaults = codes_keywords()
    for name in defaults:
        with pytest.raises(L.VauraHipError, match="rerun"):
            eng.generate_codes_stream(feats, 43, **{name: defaults[name]})
    for name in ("max_tokens", "block_frame", "resolved"):
        with pytest.raises(TypeError, match=name):
            eng.generate_codes_stream(feats, 43, **{name: 1})
    with pytest.raises(TypeError, match="no_such_keyword"):
        resolve_codes_call(B, TV, 43, no_such_keyword=1)
