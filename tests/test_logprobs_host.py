"""Token log-probabilities and best-of-N candidates, host side: the descriptor layout, what the plugin refuses before any device
work, the argument checks of the new entry points, and the pure-Python restatement (tests/logprob_reference.py) of the reduction
and the selection rule, pinned against hand-made cases so that the GPU tests compare against something fixed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprob_reference as R  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import clip_params, synth  # noqa: E402

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- struct layout
def test_decoder_gains_logprobs_behind_clip_sampling_and_sampling_keeps_48_bytes():
    assert L.Decoder.logprobs.offset == L.Decoder.clip_sampling.offset + C.sizeof(C.c_void_p)
    assert L.Decoder.logprobs.offset + C.sizeof(C.c_void_p) == C.sizeof(L.Decoder)          # the last field
    lib = L.lib()
    assert C.sizeof(L.Decoder) == lib.vaura_struct_size(3)
    assert C.sizeof(L.Sampling) == 48 == lib.vaura_struct_size(2)
    assert L.Decoder().logprobs is None                                                      # zero-filled descriptor: LP off


def test_new_entry_points_check_their_arguments_without_a_gpu():
    lib = L.lib()
    one = C.c_void_p(16)          # never dereferenced: the checks come first
    sp = L.Sampling(0, 1.0, 0, 0.0, 1.0, 0, 0, 0, 0.0)
    assert lib.vaura_sample_logprobs(one, 3, 9, 1024, C.byref(sp), None, None, 0, one, None, 0, 0, None, None, None) == -1   # no logprobs_out
    assert lib.vaura_sample_logprobs(one, 3, 9, 1024, C.byref(sp), None, None, 0, None, None, 0, 0, None, one, None) == -1   # no token output
    assert lib.vaura_sample_logprobs(one, 3, 9, 1024, C.byref(sp), None, None, 0, None, one, 12, 21, None, one, None) == -1  # seq without state
    sp.input_is_probs = 1
    assert lib.vaura_sample_logprobs(one, 3, 9, 1024, C.byref(sp), None, None, 0, one, None, 0, 0, None, one, None) == -1    # probability rows
    d9 = (C.c_int32 * 9)(*range(9))
    assert lib.vaura_sequence_logprob(None, 21, None, 2, 9, 12, 0, one, one, None) == -1
    assert lib.vaura_sequence_logprob(one, 21, None, 2, 9, 12, 12, one, one, None) == -1       # t0 leaves no frame
    assert lib.vaura_sequence_logprob(one, 21, None, 2, 17, 12, 0, one, one, None) == -2       # K > 16
    assert lib.vaura_sequence_logprob(one, 20, d9, 2, 9, 12, 0, one, one, None) == -2          # seq_len != T + max(d) + 1
    bad = (C.c_int32 * 9)(0, 2, 1, 3, 4, 5, 6, 7, 8)
    assert lib.vaura_sequence_logprob(one, 21, bad, 2, 9, 12, 0, one, one, None) == -1         # unsorted delays
    assert lib.vaura_pattern_revert_delays_f32(one, None, 2, 9, 12, 21, 0.0, d9, None) == -1
    assert lib.vaura_pattern_revert_delays_f32(one, one, 2, 9, 12, 22, 0.0, d9, None) == -2    # longer than the pattern
    assert lib.vaura_select_candidates(one, one, 2, 0, 9, 12, one, one, None) == -1
    assert lib.vaura_select_candidates(one, None, 2, 3, 9, 12, one, one, None) == -1


# ---------------------------------------------------------------------------------------------------------------- host refusals
@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    from ckpt_fixture import write_checkpoint
    from vaura_amd.model import VAURAModel
    d = tmp_path_factory.mktemp("ckpt_logprobs")
    ckpt, hp, _ = write_checkpoint(str(d), synth.tiny_sampler(2))
    return VAURAModel.load_from_checkpoint(ckpt, hparams_file=hp, map_location="cpu")


@pytest.mark.parametrize("kw,match", [
    (dict(num_candidates=0), "at least 1"),
    (dict(num_candidates=-2), "at least 1"),
    (dict(num_candidates=2.0), "must be an int"),
    (dict(num_candidates="3"), "must be an int"),
    (dict(num_candidates=True), "must be an int"),
    (dict(num_candidates=3, use_sampling=False), "identical"),
    (dict(num_candidates=3, use_sampling=True, temp=0.0), "identical"),
    (dict(num_candidates=2, use_sampling=[False, True], temp=[1.0, 0.0]), "identical"),
    (dict(return_all_candidates=True), "needs num_candidates > 1"),
    (dict(return_all_candidates=True, num_candidates=1, return_logprobs=True), "needs num_candidates > 1"),
])
@pytest.mark.parametrize("entry", ["generate", "generate_tokens"])
def test_refused_on_the_host_before_any_device_work(cpu_model, monkeypatch, entry, kw, match):
    m = cpu_model

    def touched(*a, **k):
        raise AssertionError("device work was started")
    monkeypatch.setattr(m, "_handle_visual_conditioning", touched)
    monkeypatch.setattr(m.sampler, "engine", touched)
    monkeypatch.setattr(m.audio_encoder, "decode", touched)
    frames = torch.zeros(2, 1, 32, 768)
    with pytest.raises(L.VauraHipError, match=match):
        getattr(m, entry)(frames=frames, max_new_tokens=12, prompt_is_encoded=True, **kw)


def test_per_clip_values_are_repeated_per_candidate():
    assert clip_params.repeat([0.7, 1.2], 3) == [0.7, 0.7, 0.7, 1.2, 1.2, 1.2]
    assert clip_params.repeat(torch.tensor([5, 7]), 2) == [5, 5, 7, 7]
    assert clip_params.repeat(0.9, 4) == 0.9 and clip_params.repeat(True, 2) is True


# ---------------------------------------------------------------------------------------------------------------- restatement
def test_revert_follows_the_delay_index_map():
    B, K, T = 2, 3, 4
    delays = [0, 1, 3]
    S = T + 3 + 1
    seq = np.arange(B * K * S, dtype=F32).reshape(B, K, S)
    out = R.revert(seq, delays, T)
    for q, d in enumerate(delays):
        assert np.array_equal(out[:, q], seq[:, q, 1 + d:1 + d + T])
    short = R.revert(seq[..., :6], delays, T, fill=-7.0)         # a sequence that ends early: the fill
    assert np.array_equal(short[:, 2], np.array([[4 + 2 * S, 5 + 2 * S, -7, -7], [4 + 5 * S, 5 + 5 * S, -7, -7]], dtype=F32))


def test_wave_sum_is_the_tree_of_neighbouring_pairs():
    v = np.zeros(64, dtype=F32)
    v[0], v[1], v[2] = 1.0, 2.0 ** -24, 2.0 ** -24
    # (1 + 2^-24) rounds to 1 (ties to even), then 1 + 2^-24 again: 1.  Left-to-right would give the same; the tree differs here:
    v2 = np.zeros(64, dtype=F32)
    v2[0], v2[2], v2[3] = 1.0, 2.0 ** -24, 2.0 ** -24
    assert R.wave_sum(v) == F32(1.0)
    assert R.wave_sum(v2) == F32(1.0) + F32(2.0 ** -23)          # the two small ones meet first (lanes 2, 3), then reach 1 as 2^-23
    assert R.wave_sum(np.arange(64, dtype=F32)) == F32(2016.0)


def test_codebook_mean_order_prompt_exclusion_and_count():
    T = 70
    row = np.zeros(T, dtype=F32)
    row[0], row[64] = 1.0, 2.0 ** -24                 # both belong to lane 0: 1 + 2^-24 -> 1 inside the lane
    row[1], row[65] = 2.0 ** -24, 2.0 ** -24          # lane 1 holds 2^-23, added to lane 0 by the tree: 1 + 2^-23
    assert R.codebook_mean(row, 0) == F32(F32(1.0 + 2.0 ** -23) / F32(70))
    # prompt exclusion: frames [0, t0) are neither summed nor counted, and the lanes start at t0
    row2 = np.full(T, -1.0, dtype=F32)
    row2[:4] = 0.0
    assert R.codebook_mean(row2, 4) == F32(-1.0)
    assert R.codebook_mean(row2, 0) == F32(F32(-66.0) / F32(70))
    row3 = row2.copy()
    row3[:4] = np.nan                                 # ... whatever they hold
    assert R.codebook_mean(row3, 4) == F32(-1.0)


def test_sequence_logprob_means_and_nan_rule():
    B, K, T = 3, 9, 5
    lp = np.zeros((B, K, T), dtype=F32)
    for q in range(K):
        lp[0, q] = -(q + 1)
    lp[1] = -0.5
    lp[2] = -2.0
    lp[2, 4, 3] = np.nan
    pcb, clip = R.sequence_logprob(lp, 0)
    assert np.array_equal(pcb[0], -np.arange(1, 10, dtype=F32)) and clip[0] == F32(-5.0)
    assert np.array_equal(pcb[1], np.full(9, -0.5, dtype=F32)) and clip[1] == F32(-0.5)
    assert np.isnan(clip[2]) and np.isnan(pcb[2]).all()          # one NaN: the whole clip's scores are NaN
    lp[2, 4, 3] = -2.0
    lp[2, 4, 0] = np.nan                                          # ... unless it sits in an excluded prompt frame
    pcb, clip = R.sequence_logprob(lp, 1)
    assert clip[2] == F32(-2.0) and np.array_equal(pcb[2], np.full(9, -2.0, dtype=F32))
    # the clip mean adds the K means in codebook order in fp32
    lp2 = np.zeros((1, 3, 1), dtype=F32)
    lp2[0, :, 0] = [1.0, 2.0 ** -24, 2.0 ** -24]
    assert R.sequence_logprob(lp2)[1][0] == F32(F32(1.0) / F32(3))    # (1 + 2^-24) + 2^-24 = 1 in that order


def test_selection_rule():
    nan = np.nan
    scores = np.array([[-2.0, -1.0, -1.0, -3.0],       # two equal best: the lower index
                       [nan, -5.0, nan, -4.0],         # NaN among numbers: never wins
                       [nan, nan, nan, nan],           # every score NaN: candidate 0
                       [-1.0, nan, -1.0, -0.5],
                       [-np.inf, nan, -np.inf, nan]], dtype=F32)
    assert R.select_candidates(scores).tolist() == [1, 3, 0, 3, 0]
    finite = np.where(np.isnan(scores), -np.inf, scores)
    assert R.select_candidates(scores)[[0, 1, 3]].tolist() == np.argmax(finite, axis=1)[[0, 1, 3]].tolist()
