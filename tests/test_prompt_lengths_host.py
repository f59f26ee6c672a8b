"""Per-clip audio prompt lengths, host side: resolution and refusals (vaura_amd/clip_params.py), the schedule of prefill passes and
steps, the descriptor extension's layout and the keywords' places in the public signatures.  No device, no HIP library."""
import ctypes as C
import inspect

import pytest
import torch

from vaura_amd import _lib as L
from vaura_amd import clip_params as cp
from vaura_amd import dist


def kinds(plan):
    return [(e[0], e[1]) for e in plan]


def test_schedule_of_the_issue():
    """P = [6, 0, 3, 6], delays[0] = 0, S = 23: 3 steps, pass n = 3 on clip 2, 3 steps, pass n = 6 on clips 0 and 3, 16 steps"""
    plan = cp.prompt_schedule([6, 0, 3, 6], 0, 23)
    assert plan == [("steps", 3), ("prefill", 3, [2]), ("steps", 3), ("prefill", 6, [0, 3]), ("steps", 16)]
    assert 0 + sum(e[1] for e in plan if e[0] == "steps") == 23 - 1          # the earliest group: prefill positions + steps = S - 1
    assert cp.prompt_row_steps([6, 0, 3, 6], 0) == [6, 0, 3, 6]


def test_schedule_rows_with_cfg_and_candidates():
    plan = cp.prompt_schedule([6, 0, 3, 6], 0, 23, cfg=True, num_candidates=2)
    assert kinds(plan) == [("steps", 3), ("prefill", 3), ("steps", 3), ("prefill", 6), ("steps", 16)]
    assert plan[1][2] == [4, 5, 12, 13]                      # clip 2: its two candidates, then their null-condition rows (8 + ..)
    assert plan[3][2] == [0, 1, 6, 7, 8, 9, 14, 15]          # clips 0 and 3
    assert cp.prompt_rows([1], 4, cfg=True) == [1, 5] and cp.prompt_rows([1, 3], 4, num_candidates=3) == [3, 4, 5, 9, 10, 11]
    n = cp.prompt_row_steps([6, 0, 3, 6], 0, cfg=True, num_candidates=2)
    assert n == [6, 6, 0, 0, 3, 3, 6, 6] * 2
    for e in plan:                                           # a pass appends exactly to the rows whose n is the pass's
        if e[0] == "prefill":
            assert e[2] == [r for r, v in enumerate(n) if v == e[1]]


def test_schedule_with_a_first_delay():
    """delays[0] = 2: every clip teacher-forces P_b + 2 positions, so even P = 0 has a pass; S = 25"""
    plan = cp.prompt_schedule([6, 0, 3, 6], 2, 25)
    assert plan == [("prefill", 2, [1]), ("steps", 3), ("prefill", 5, [2]), ("steps", 3), ("prefill", 8, [0, 3]), ("steps", 16)]
    assert plan[0][1] + sum(e[1] for e in plan if e[0] == "steps") == 25 - 1
    assert cp.prompt_row_steps([6, 0, 3, 6], 2, cfg=True) == [8, 2, 5, 8, 8, 2, 5, 8]


def test_equal_lengths_give_the_scalar_plan():
    assert cp.prompt_schedule([4, 4, 4], 0, 23) == [("prefill", 4, [0, 1, 2]), ("steps", 18)]       # run(n_prefill = 4, n_steps = S - 5)
    assert cp.prompt_schedule([4, 4], 0, 23, cfg=True) == [("prefill", 4, [0, 1, 2, 3]), ("steps", 18)]
    assert cp.prompt_schedule([0, 0], 0, 23) == [("steps", 22)]
    assert cp.prompt_schedule([0, 0], 1, 24) == [("prefill", 1, [0, 1]), ("steps", 22)]


def test_no_pass_reaches_a_position_a_row_has_not_filled():
    """just before the pass at n_g the loop has run the steps up to position n_g - 1, which filled slot n_g: every row is known below n_g"""
    for P, d0, S in (([6, 0, 3, 6], 0, 23), ([5, 9, 1, 1, 7], 3, 40), ([0, 1], 0, 5)):
        pos = min(P) + d0
        for e in cp.prompt_schedule(P, d0, S):
            if e[0] == "steps":
                pos += e[1]
            else:
                assert e[1] == pos
        assert pos == S - 1
    with pytest.raises(L.VauraHipError, match="teacher-forced positions"):
        cp.prompt_schedule([6, 30], 0, 23)


def test_resolution_and_every_refusal():
    assert cp.resolve_prompt_lengths(4, None, 6, 14) is None
    assert cp.resolve_prompt_lengths(4, [6, 0, 3, 6], 6, 14) == [6, 0, 3, 6]
    assert cp.resolve_prompt_lengths(None, (6, 0, 3, 6), 6, 14, [14, 9, 14, 8]) == [6, 0, 3, 6]
    assert cp.resolve_prompt_lengths(4, torch.tensor([6, 0, 3, 6]), 6, 14) == [6, 0, 3, 6]
    for bad, kw, match in (([6, 0, 3], {}, "3 values for a batch of 4"), ([6, 0, 3, 6, 1], {}, "5 values"),
                           ([6, 0, 3.0, 6], {}, "must hold integers"), ([6, True, 3, 6], {}, "must hold integers"),
                           (torch.tensor([6.0, 0.0, 3.0, 6.0]), {}, "must hold integers"),
                           ([6, -1, 3, 6], {}, "must lie in 0 .. 6"), ([6, 0, 7, 6], {}, "must lie in 0 .. 6"),
                           (3, {}, "one integer per clip"), (torch.zeros(2, 2, dtype=torch.int64), {}, "one-dimensional"),
                           ([6, 0, 3, 6], dict(lens=[14, 9, 3, 8]), "clip 2 .3 frames. must be shorter than its max_new_tokens .3."),
                           ([6, 0, 3, 6], dict(lens=[14, 9, 8]), "max_new_tokens has 3")):
        with pytest.raises(L.VauraHipError, match=match):
            cp.resolve_prompt_lengths(4, bad, 6, 14, **kw)
    with pytest.raises(L.VauraHipError, match="shorter than its max_new_tokens"):
        cp.resolve_prompt_lengths(4, [6, 0, 3, 6], 6, 6)
    with pytest.raises(L.VauraHipError, match="needs an audio prompt"):
        cp.resolve_prompt_lengths(4, [6, 0, 3, 6], None, 14)


def test_the_extension_follows_the_older_structs():
    assert L.DecoderExt3.ext2.offset == 0 and L.DecoderExt3.row_prompt_steps.offset == C.sizeof(L.DecoderExt2) == 448
    assert C.sizeof(L.DecoderExt3) == 456
    x = L.DecoderExt3()
    assert x.ext2.ext.dec.ext_bytes == 0 and x.row_prompt_steps is None       # zero-filled: no prompt lengths
    assert C.addressof(x.ext2.ext.dec) == C.addressof(x)
    for name in ("vaura_prefill_rows", "vaura_rope_append_rows", "vaura_sample_seq_starts", "vaura_sequence_logprob_starts"):
        assert name in L.SIGNATURES


def test_keywords_of_the_public_calls():
    from vaura_amd.engine import DecoderEngine
    from vaura_amd.model import VAURAModel
    assert "prompt_lengths" in inspect.signature(DecoderEngine.generate_codes).parameters
    for fn in (VAURAModel.generate, VAURAModel.generate_tokens):
        p = inspect.signature(fn).parameters
        assert p["prompt_lengths"].default is None and p["audio_lengths"].default is None


def test_prompt_lengths_are_sharded_with_their_clips():
    p = dict(max_new_tokens=[12, 5, 9, 9, 7], prompt_lengths=[6, 0, 3, 6, 1], audio_lengths=[9, 8, 7, 6, 5], seed=3)
    got = [dist.shard_params(p, 5, r, 2) for r in range(2)]
    assert got[0]["prompt_lengths"] == [6, 0, 3] and got[1]["prompt_lengths"] == [6, 1]
    assert got[0]["audio_lengths"] == [9, 8, 7] and got[1]["audio_lengths"] == [6, 5] and got[1]["seed"] == 3


# ---------------------------------------------------------------------------------------------------------------- plugin refusals
@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from ckpt_fixture import write_checkpoint
    from vaura_amd import synth
    from vaura_amd.model import VAURAModel
    d = tmp_path_factory.mktemp("ckpt_prompt_lengths")
    ckpt, hp, _ = write_checkpoint(str(d), synth.tiny_sampler(2))
    return VAURAModel.load_from_checkpoint(ckpt, hparams_file=hp, map_location="cpu")


PROMPT = torch.zeros(4, 9, 6, dtype=torch.int64)


@pytest.mark.parametrize("kw,match", [
    (dict(audio=PROMPT, prompt_lengths=[6, 0, 3]), "3 values for a batch of 4"),
    (dict(audio=PROMPT, prompt_lengths=[6, 0, 3.5, 6]), "must hold integers"),
    (dict(audio=PROMPT, prompt_lengths=[6, -1, 3, 6]), "must lie in 0 .. 6"),
    (dict(audio=PROMPT, prompt_lengths=[6, 0, 7, 6]), "must lie in 0 .. 6"),
    (dict(audio=PROMPT, prompt_lengths=[6, 0, 3, 6], max_new_tokens=[14, 9, 3, 8]), "shorter than its max_new_tokens"),
    (dict(audio=PROMPT, prompt_lengths=[6, 0, 3, 6], max_new_tokens=6), "shorter than its max_new_tokens"),
    (dict(prompt_lengths=[6, 0, 3, 6]), "needs an audio prompt"),
    (dict(audio_lengths=[6, 1, 3, 6]), "needs an audio prompt"),
    (dict(audio=PROMPT, prompt_lengths=[6, 0, 3, 6], audio_lengths=[6, 1, 3, 6]), "pass one of them"),
    (dict(audio=PROMPT, audio_lengths=[6, 1, 3, 6]), "an encoded prompt takes prompt_lengths"),
])
@pytest.mark.parametrize("entry", ["generate", "generate_tokens"])
def test_refused_on_the_host_before_any_device_work(cpu_model, monkeypatch, entry, kw, match):
    m = cpu_model

    def touched(*a, **k):
        raise AssertionError("device work was started")
    monkeypatch.setattr(m, "_handle_visual_conditioning", touched)
    monkeypatch.setattr(m.sampler, "engine", touched)
    monkeypatch.setattr(m.audio_encoder, "decode", touched)
    monkeypatch.setattr(m.audio_encoder, "encode", touched)
    monkeypatch.setattr(m.audio_encoder, "encode_clips", touched)
    frames = torch.zeros(4, 1, 32, 768)
    with pytest.raises(L.VauraHipError, match=match):
        getattr(m, entry)(**dict(dict(frames=frames, max_new_tokens=14, prompt_is_encoded=True), **kw))
