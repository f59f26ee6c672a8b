"""Per-clip lengths, host side: what is refused before any device work (clip_params.resolve_lengths, generate / generate_tokens,
generate_long, score), the descriptor layout (vaura_decoder and vaura_decoder_ext keep their sizes and offsets; the two arrays live
behind them, in vaura_decoder_ext2) and the sharding of both sequences with their clips."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_relevance_host as RH  # noqa: E402  (the pinned offsets, the refusal descriptor)
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import clip_params, dist, synth  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------- resolve
def test_resolve_lengths():
    assert clip_params.resolve_lengths(4, 12) == (12, None, None)
    assert clip_params.resolve_lengths(4, [12, 5, 1, 9], [32, 2, 1, 3], 32) == (12, [12, 5, 1, 9], [32, 2, 1, 3])
    assert clip_params.resolve_lengths(None, (3, 7)) == (7, [3, 7], None)
    assert clip_params.resolve_lengths(2, torch.tensor([3, 7]), torch.tensor([1, 2]), 2) == (7, [3, 7], [1, 2])
    assert clip_params.resolve_lengths(2, 5, [1, 2], None, prompt_len=4) == (5, None, [1, 2])
    for args, match in (((4, [12, 5, 9]), "3 values"), ((4, [12, 5.0, 1, 9]), "integers"), ((4, [12, True, 1, 9]), "integers"),
                        ((4, torch.tensor([1.0, 2.0, 3.0, 4.0])), "integers"), ((4, [12, 5, 0, 9]), "at least 1"),
                        ((4, torch.ones(2, 2, dtype=torch.int64)), "one-dimensional"), ((4, 12, [32, 2, 1]), "3 values"),
                        ((4, 12, [32, 2, 0, 3], 32), "video_lengths must lie"), ((4, 12, [32, 2, 33, 3], 32), "video_lengths must lie"),
                        ((4, 12, 3), "one integer per clip"), ((4, [12, 5, 1, 9], [32, 2, 1], 32), "values"),
                        ((4, [12, 5, 2, 9], None, None, 2), "prompt"), ((4, [12, 5, 2, 9], None, None, 5), "prompt")):
        with pytest.raises(L.VauraHipError, match=match):
            clip_params.resolve_lengths(*args)


# ---------------------------------------------------------------------------------------------------------------- plugin refusals
@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    from ckpt_fixture import write_checkpoint
    from vaura_amd.model import VAURAModel
    d = tmp_path_factory.mktemp("ckpt_clip_lengths")
    ckpt, hp, _ = write_checkpoint(str(d), synth.tiny_sampler(2))
    return VAURAModel.load_from_checkpoint(ckpt, hparams_file=hp, map_location="cpu")


def _untouchable(m, monkeypatch, allow_conditioning=False):
    def touched(*a, **k):
        raise AssertionError("device work was started")
    if allow_conditioning:       # the number of video tokens is known only from the features: they pass through, the engine stays untouched
        monkeypatch.setattr(m, "_handle_visual_conditioning", lambda frames, *a, **k: frames[:, 0])
    else:
        monkeypatch.setattr(m, "_handle_visual_conditioning", touched)
    monkeypatch.setattr(m.sampler, "engine", touched)
    monkeypatch.setattr(m.audio_encoder, "decode", touched)


@pytest.mark.parametrize("kw,match", [
    (dict(max_new_tokens=[12, 5, 9]), "3 values"),
    (dict(max_new_tokens=[12, 5.5, 1, 9]), "integers"),
    (dict(max_new_tokens=[12, 5, 0, 9]), "at least 1"),
    (dict(max_new_tokens=12, video_lengths=[32, 2, 0, 3]), "video_lengths must lie"),
    (dict(max_new_tokens=12, video_lengths=[32, 2]), "2 values"),
    (dict(max_new_tokens=12, video_lengths=4), "one integer per clip"),
    (dict(max_new_tokens=[12, 5, 2, 9], audio=torch.zeros(4, 9, 2, dtype=torch.int64)), "prompt"),
])
@pytest.mark.parametrize("entry", ["generate", "generate_tokens"])
def test_refused_before_any_device_work(cpu_model, monkeypatch, entry, kw, match):
    _untouchable(cpu_model, monkeypatch)
    with pytest.raises(L.VauraHipError, match=match):
        getattr(cpu_model, entry)(frames=torch.zeros(4, 1, 32, 768), prompt_is_encoded=True, **kw)


def test_video_length_beyond_the_features_is_refused_before_the_engine_is_touched(cpu_model, monkeypatch):
    """(generate() asks the engine for its device before anything else, to leave the null stream: its lengths are checked by the
    generate_tokens call inside it)"""
    _untouchable(cpu_model, monkeypatch, allow_conditioning=True)
    with pytest.raises(L.VauraHipError, match="video_lengths must lie in 1 .. 32"):
        cpu_model.generate_tokens(frames=torch.zeros(4, 1, 32, 768), prompt_is_encoded=True, max_new_tokens=[12, 5, 1, 9],
                                  video_lengths=[32, 2, 33, 3])


def test_sliding_window_and_scoring_keep_one_length_per_call(cpu_model, monkeypatch):
    from vaura_amd import longform
    from vaura_amd.engine import DecoderEngine
    _untouchable(cpu_model, monkeypatch)
    frames = torch.zeros(2, 4, 2, 768)
    with pytest.raises(L.VauraHipError, match="generate_long takes one length"):
        longform.generate_long(cpu_model, frames, [2.56, 1.3])
    with pytest.raises(L.VauraHipError, match="generate_long takes one length"):
        longform.generate_long(cpu_model, frames, 2.56, video_lengths=[2, 1])
    eng = object.__new__(DecoderEngine)              # refused before anything of the engine is read
    eng.cfg = synth.tiny_sampler(2)
    codes, feats = torch.zeros(2, 9, 12, dtype=torch.int64), torch.zeros(2, 32, 768)
    with pytest.raises(L.VauraHipError, match="one length for the whole call"):
        eng.score([codes[0:1], codes[1:2, :, :5]], feats)
    with pytest.raises(L.VauraHipError, match="one length for the whole call"):
        eng.score(codes, feats, video_lengths=[32, 2])


# ---------------------------------------------------------------------------------------------------------------- struct layout
def test_both_older_structs_keep_their_layout_and_the_arrays_follow_them():
    for n, off in RH.OFFSETS.items():
        assert getattr(L.Decoder, n).offset == off, n
    assert C.sizeof(L.Decoder) == 416 and C.sizeof(L.DecoderExt) == 432
    assert L.DecoderExt.logprobs_cond.offset == 416 and L.DecoderExt.logprobs_null.offset == 424
    assert L.DecoderExt2.ext.offset == 0 and L.DecoderExt2.clip_timesteps.offset == 432 and L.DecoderExt2.clip_cond_tokens.offset == 440
    assert C.sizeof(L.DecoderExt2) == 448
    lib = L.lib()
    assert [lib.vaura_struct_size(i) for i in (3, 10, 11)] == [416, 432, 448] and lib.vaura_struct_size(12) == 0
    x = L.DecoderExt2()
    assert x.ext.dec.ext_bytes == 0 and x.clip_timesteps is None and x.clip_cond_tokens is None      # zero-filled: no lengths
    x.ext.dec.batch = 5                                                                               # views of the one object
    assert x.ext.dec.batch == 5 and C.addressof(x.ext.dec) == C.addressof(x)


@pytest.mark.parametrize("ext_bytes,rc", [(0, 0), (16, 0), (32, 0), (8, -1), (24, -1), (48, -1)])
def test_accepted_extension_sizes(ext_bytes, rc):
    """a loop of no positions launches nothing and dereferences nothing: it returns what the descriptor check says"""
    x = L.DecoderExt2()
    src, _, keep = RH._descriptor(6)
    C.memmove(C.addressof(x), C.addressof(src), C.sizeof(L.DecoderExt))
    x.ext.dec.ext_bytes = ext_bytes
    sp = L.Sampling(0, 1.0, 0, 0.0, 3.0, 0, 0, 0, 0.0)
    assert L.lib().vaura_generate_loop(C.byref(x.ext.dec), C.byref(sp), 0, 0, None, None) == rc
    del keep


def test_lengths_are_checked_on_the_host_before_anything_is_launched():
    """a misaligned array pointer is refused before any copy; with the 16-byte extension the same bytes are not the library's to read"""
    x = L.DecoderExt2()
    src, _, keep = RH._descriptor(6)
    C.memmove(C.addressof(x), C.addressof(src), C.sizeof(L.DecoderExt))
    x.clip_timesteps = 18
    d = x.ext.dec
    d.ext_bytes = 32
    assert L.lib().vaura_embed(C.byref(d), 0, 1, None) == -1
    assert L.lib().vaura_embed(C.byref(d), 0, 0, None) == -1 and L.lib().vaura_embed(C.byref(d), -1, 2, None) == -1
    one = C.c_void_p(16)
    for fn, args in (("vaura_pattern_build_clips", (one, one, 4, 9, 12, 21, 1024, None, None, None)),
                     ("vaura_pattern_revert_clips", (one, one, 4, 9, 12, 21, -1, 1024, None, None, None)),
                     ("vaura_pattern_revert_clips_f32", (one, one, 4, 9, 12, 21, 0.0, 0.0, None, None, None)),
                     ("vaura_sequence_logprob_clips", (one, 21, None, 4, 9, 12, 0, None, one, one, None))):
        assert getattr(L.lib(), fn)(*args) == -1, fn             # no array: refused, nothing dereferenced
    sp = L.Sampling(0, 1.0, 0, 0.0, 1.0, 0, 0, 0, 0.0)
    assert L.lib().vaura_sample_seq(one, 4, 9, 1024, C.byref(sp), None, None, None, 12, 21, one, None, one, None, None, None, None) == -1
    assert L.lib().vaura_sample_seq(one, 4, 9, 1024, C.byref(sp), None, None, one, 12, 21, one, None, one, one, one, None, None) == -1
    del keep


# ---------------------------------------------------------------------------------------------------------------- sharding
def test_both_sequences_are_sharded_with_their_clips():
    p = dict(max_new_tokens=[12, 5, 1, 9, 7], video_lengths=[32, 2, 1, 3, 4], temp=[0.5, 0.6, 0.7, 0.8, 0.9], top_k=250, seed=3)
    got = [dist.shard_params(p, 5, r, 2) for r in range(2)]
    assert got[0]["max_new_tokens"] == [12, 5, 1] and got[1]["max_new_tokens"] == [9, 7]
    assert got[0]["video_lengths"] == [32, 2, 1] and got[1]["video_lengths"] == [3, 4]
    assert got[0]["temp"] == [0.5, 0.6, 0.7] and got[1]["top_k"] == 250 and got[1]["seed"] == 3
    one = dist.shard_params(dict(max_new_tokens=12, video_lengths=None, temp=0.9), 5, 1, 2)
    assert one == dict(max_new_tokens=12, video_lengths=None, temp=0.9)
    assert torch.equal(dist.shard_params(dict(max_new_tokens=torch.tensor([3, 4, 5])), 3, 1, 2)["max_new_tokens"], torch.tensor([5]))
    with pytest.raises(L.VauraHipError, match="4 values"):
        dist.shard_params(dict(max_new_tokens=[12, 5, 1, 9]), 5, 0, 2)
    with pytest.raises(L.VauraHipError, match="2 values"):
        dist.shard_params(dict(max_new_tokens=12, video_lengths=[1, 2]), 5, 0, 2)
