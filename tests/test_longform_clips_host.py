"""Sliding-window generation with one duration per clip, host side: the merged chunk plan (longform.clip_chunk_plan) against every
clip's own chunk_schedule, what generate_long_clips and generate_tokens(video_segments=...) refuse before any device work, and the
sharding of the two new per-clip keys."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import dist, longform, synth  # noqa: E402

TINY = dict(model_max_duration=0.30, stride=0.10, vfps=440)
PROD = dict(model_max_duration=2.56, stride=0.64, vfps=25)
DURATIONS = [0.62, 0.27, 0.45, 0.50, 0.31, 0.40]
FR = longform.COMPRESSION_MODEL_FRAME_RATE


# ---------------------------------------------------------------------------------------------------------------- the plan
def check_plan(durations, segments, S, geo):
    plan = longform.clip_chunk_plan(durations, segments, S, **geo)
    seg = segments or [S] * len(durations)
    scheds = [longform.chunk_schedule(d, geo["model_max_duration"], geo["stride"], geo["vfps"]) for d in durations]
    stride_tokens = int(FR * geo["stride"])
    assert plan["stride_tokens"] == stride_tokens
    assert len(plan["chunks"]) == max(len(s) for s in scheds)
    for b, (cl, s) in enumerate(zip(plan["clips"], scheds)):
        assert cl["schedule"] == s and cl["segments"] == seg[b]
        assert cl["length"] == s[-1]["offset"] + s[-1]["max_gen_len"]
        assert cl["single"] == (durations[b] <= geo["model_max_duration"])
    for c, ch in enumerate(plan["chunks"]):
        assert ch["index"] == c
        for b, s in enumerate(scheds):
            if c >= len(s):                                          # parked: one frame behind the prompt, one segment
                assert ch["parked"][b] and ch["T"][b] == ch["prompt_len"] + 1 and ch["indices"][b] == [0] and ch["hi"][b] is None
                continue
            e = s[c]
            assert not ch["parked"][b]
            assert ch["T"][b] == e["max_gen_len"] and ch["prompt_len"] == e["prompt_len"] and e["offset"] == c * stride_tokens
            if e["positions"] is None:
                assert ch["hi"][b] is None and ch["indices"][b] == list(range(seg[b]))
            else:
                lo, hi = e["positions"]
                assert ch["lo"] == lo and ch["hi"][b] == hi
                assert ch["indices"][b] == (torch.arange(lo, hi) % seg[b]).tolist()
            assert ch["n_segments"][b] == len(ch["indices"][b]) <= ch["width"]
        assert not all(ch["parked"])
        assert ch["width"] >= max(ch["n_segments"])
    return plan


def test_plan_of_the_test_set_follows_every_clips_own_schedule():
    plan = check_plan(DURATIONS, None, 4, TINY)
    assert [len(cl["schedule"]) for cl in plan["clips"]] == [5, 1, 3, 4, 1, 2]
    assert [cl["length"] for cl in plan["clips"]] == [54, 23, 39, 43, 26, 34]
    assert [cl["single"] for cl in plan["clips"]] == [False, True, False, False, False, False]
    ch = plan["chunks"]
    assert [c["prompt_len"] for c in ch] == [0, 18, 18, 18, 18]
    assert ch[0]["T"] == [26, 23, 26, 26, 26, 26] and ch[0]["n_segments"] == [8, 4, 8, 8, 8, 8]
    assert ch[2]["T"][2] == 23 and (ch[2]["lo"], ch[2]["hi"][2]) == (5, 12) and ch[2]["n_segments"][2] == 7 and ch[2]["n_segments"][0] == 8
    assert ch[3]["T"][3] == 19 and ch[3]["n_segments"][3] == 6             # ONE new frame: T = prompt + 1
    assert ch[4]["T"][0] == 22 and ch[4]["n_segments"][0] == 7
    assert ch[4]["parked"] == [False, True, True, True, True, True]
    assert ch[2]["parked"] == [False, True, False, False, True, True]
    assert all(c["width"] == 8 for c in ch)                                # the window's 8 segments, also where every selection is shorter
    # parked slots: 4 (0.27), 2 (0.45), 1 (0.50), 4 (0.31), 3 (0.40) of 30
    assert sum(sum(c["parked"]) for c in ch) == 4 + 2 + 1 + 4 + 3


def test_plan_with_segments_wraps_every_clip_at_its_own_count():
    plan = check_plan(DURATIONS, [4, 3, 4, 2, 4, 3], 4, TINY)
    assert plan["chunks"][0]["indices"][1] == [0, 1, 2]                    # single-chunk clip: all ITS segments
    assert plan["chunks"][3]["indices"][3] == [1, 0, 1, 0, 1, 0]           # positions 7 .. 12 mod 2
    assert longform.clip_chunk_plan([0.4, 0.5], [3, 2], **TINY)["clips"][0]["segments"] == 3      # S: the widest clip


@pytest.mark.parametrize("durations,segments,S", [
    ([3.0, 4.2, 10.0, 2.0, 2.56, 2.57, 7.77, 5.0], None, 16),
    ([3.0, 4.2, 10.0, 2.0], [3, 4, 9, 2], 9),
    ([i / 7 + 0.1 for i in range(70)], None, 12),
])
def test_plan_in_the_production_geometry(durations, segments, S):
    plan = check_plan(durations, segments, S, PROD)
    assert all(ch["width"] >= 4 for ch in plan["chunks"])


def test_plan_refusals():
    for bad, match in (([], "empty"), (0.4, "one duration per clip"), ([0.4, float("nan")], "finite and positive"),
                       ([0.4, float("inf")], "finite and positive"), ([0.4, 0.0], "finite and positive"), ([0.4, -1.0], "finite and positive"),
                       ([0.4, 0.011], "gives no frame"), ([0.4, "1"], "number of seconds"), (torch.ones(2, 2), "one duration per clip")):
        with pytest.raises(L.VauraHipError, match=match):
            longform.clip_chunk_plan(bad, None, 4, **TINY)
    for bad, match in (([4, 4, 4], "3 values"), ([4, 0], "must lie in 1 .. 4"), ([4, 5], "must lie in 1 .. 4"), ([4, 2.0], "integers"), (3, "one integer per clip")):
        with pytest.raises(L.VauraHipError, match=match):
            longform.clip_chunk_plan([0.4, 0.5], bad, 4, **TINY)
    with pytest.raises(L.VauraHipError, match="needs S"):
        longform.clip_chunk_plan([0.4, 0.5], **TINY)


# ---------------------------------------------------------------------------------------------------------------- plugin refusals
@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    from ckpt_fixture import write_checkpoint
    from vaura_amd.model import VAURAModel
    d = tmp_path_factory.mktemp("ckpt_longform_clips")
    ckpt, hp, _ = write_checkpoint(str(d), synth.tiny_sampler(2))
    return VAURAModel.load_from_checkpoint(ckpt, hparams_file=hp, map_location="cpu")


def _untouchable(m, monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work was started")
    monkeypatch.setattr(m, "_handle_visual_conditioning", touched)
    monkeypatch.setattr(m, "generate_tokens", touched)
    monkeypatch.setattr(m.sampler, "engine", touched)
    monkeypatch.setattr(m.audio_encoder, "decode", touched)
    monkeypatch.setattr(m.audio_encoder, "decode_clips", touched)


@pytest.mark.parametrize("durations,kw,match", [
    (0.4, {}, "one duration per clip"),
    ([0.4, 0.5, 0.6], {}, "3 values for a batch of 2"),
    (torch.tensor([[0.4, 0.5]]), {}, "one duration per clip"),
    ([0.4, float("nan")], {}, "finite and positive"),
    ([0.4, float("inf")], {}, "finite and positive"),
    ([0.4, 0.0], {}, "finite and positive"),
    ([-0.4, 0.5], {}, "finite and positive"),
    ([0.4, 0.011], {}, "gives no frame"),
    ([0.4, 0.5], dict(segments=[4]), "1 values for a batch of 2"),
    ([0.4, 0.5], dict(segments=[4, 0]), "segments must lie in 1 .. 4"),
    ([0.4, 0.5], dict(segments=[5, 1]), "segments must lie in 1 .. 4"),
    ([0.4, 0.5], dict(segments=[4, 1.5]), "integers"),
    ([0.4, 0.5], dict(video_lengths=[8, 4]), "takes no video_lengths"),
    ([0.4, 0.5], dict(num_candidates=2), "takes no num_candidates"),
    ([0.4, 0.5], dict(num_candidates=1), "takes no num_candidates"),
    ([0.4, 0.27], dict(frame_step=2), "frame_step = 2 with a batch that mixes"),
    ([0.4, 0.5], dict(temp=[1.0, 0.7, 0.5]), "3 values for a batch of 2"),
])
def test_generate_long_clips_refuses_before_any_device_work(cpu_model, monkeypatch, durations, kw, match):
    _untouchable(cpu_model, monkeypatch)
    with pytest.raises(L.VauraHipError, match=match):
        longform.generate_long_clips(cpu_model, torch.zeros(2, 4, 4, 768), durations, **TINY, **kw)


def test_generate_long_still_takes_one_length(cpu_model, monkeypatch):
    _untouchable(cpu_model, monkeypatch)
    with pytest.raises(L.VauraHipError, match="generate_long takes one length"):
        longform.generate_long(cpu_model, torch.zeros(2, 4, 4, 768), [0.62, 0.40])
    with pytest.raises(L.VauraHipError, match="generate_long takes one length"):
        longform.generate_long(cpu_model, torch.zeros(2, 4, 4, 768), torch.tensor([0.62, 0.40]))


@pytest.mark.parametrize("kw,match", [
    (dict(video_segments=[4, 2], video_lengths=[16, 8]), "pass one of them"),
    (dict(video_segments=[4, 2, 1]), "3 values for a batch of 2"),
    (dict(video_segments=[4, 0]), "video_segments must lie in 1 .. 4"),
    (dict(video_segments=[5, 1]), "video_segments must lie in 1 .. 4"),
    (dict(video_segments=[4, 1.0]), "integers"),
    (dict(video_segments=3), "one integer per clip"),
    (dict(video_segments=[4, 2], max_new_tokens=[12, 5, 3]), "values"),
])
def test_video_segments_refusals_before_any_device_work(cpu_model, monkeypatch, kw, match):
    def touched(*a, **k):
        raise AssertionError("device work was started")
    monkeypatch.setattr(cpu_model, "_handle_visual_conditioning", touched)
    monkeypatch.setattr(cpu_model.sampler, "engine", touched)
    kw = dict(dict(max_new_tokens=12), **kw)
    with pytest.raises(L.VauraHipError, match=match):
        cpu_model.generate_tokens(frames=torch.zeros(2, 4, 4, 768), prompt_is_encoded=True, **kw)


def test_video_segments_needs_the_flattened_layout(cpu_model, monkeypatch):
    monkeypatch.setattr(cpu_model, "flatten_vis_feats", False)
    monkeypatch.setattr(cpu_model.sampler, "engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device work was started")))
    with pytest.raises(L.VauraHipError, match="flattened AVCLIP layout"):
        cpu_model.generate_tokens(frames=torch.zeros(2, 4, 4, 768), prompt_is_encoded=True, max_new_tokens=12, video_segments=[4, 2])


# ---------------------------------------------------------------------------------------------------------------- sharding
def test_durations_and_segments_are_sharded_with_their_clips():
    p = dict(durations=[3.0, 4.5, 10.0, 2.0, 7.7], segments=[2, 3, 6, 1, 5], temp=[0.5, 0.6, 0.7, 0.8, 0.9], stride=0.64)
    got = [dist.shard_params(p, 5, r, 2) for r in range(2)]
    assert got[0]["durations"] == [3.0, 4.5, 10.0] and got[1]["durations"] == [2.0, 7.7]
    assert got[0]["segments"] == [2, 3, 6] and got[1]["segments"] == [1, 5]
    assert got[1]["temp"] == [0.8, 0.9] and got[1]["stride"] == 0.64
    assert dist.shard_params(dict(durations=[3.0, 4.5], segments=None), 2, 1, 2) == dict(durations=[4.5], segments=None)
    assert torch.equal(dist.shard_params(dict(durations=torch.tensor([3.0, 4.0, 5.0])), 3, 1, 2)["durations"], torch.tensor([5.0]))
    with pytest.raises(L.VauraHipError, match="durations has 4 values"):
        dist.shard_params(dict(durations=[3.0, 4.5, 10.0, 2.0]), 5, 0, 2)
    with pytest.raises(L.VauraHipError, match="segments has 2 values"):
        dist.shard_params(dict(durations=[3.0] * 5, segments=[1, 2]), 5, 0, 2)
    with pytest.raises(L.VauraHipError, match="durations has no per-clip values"):
        dist.shard_params(dict(durations=3.0), 5, 0, 2)
