"""Host side of the per-clip sampling parameters (vaura_amd/clip_params.py, dist.shard_params): broadcasting, length checks,
the record layout and the sharding of the parameter lists — no GPU."""
import ctypes as C
import struct

import pytest
import torch

from vaura_amd import _lib as L
from vaura_amd import clip_params as cp
from vaura_amd import dist


def test_all_scalar_calls_stay_scalar():
    assert cp.resolve(4, True, 1.0, 250, 0.0, 6.0) is None
    assert cp.resolve(4, torch.tensor(True), torch.tensor(0.7), 250, 0.0, torch.tensor(6.0)) is None      # 0-d tensors are scalars
    assert cp.per_clip_length(temp=1.0, top_k=3) is None
    assert not cp.is_per_clip(1.0) and not cp.is_per_clip(torch.tensor(2.0)) and not cp.is_per_clip(True)
    assert cp.is_per_clip([1.0]) and cp.is_per_clip((1, 2)) and cp.is_per_clip(torch.zeros(3))


def test_scalars_are_broadcast_next_to_sequences_and_typed():
    p = cp.resolve(3, True, [0.7, 1.3, 0.0], torch.tensor([0, 128, 250]), 0.3, (1.0, 3.0, 6.0))
    assert p == {"use_sampling": [1, 1, 1], "temp": [0.7, 1.3, 0.0], "top_k": [0, 128, 250], "top_p": [0.3] * 3,
                 "cfg_scale": [1.0, 3.0, 6.0]}
    assert all(type(v) is int for v in p["use_sampling"] + p["top_k"])
    assert all(type(v) is float for v in p["temp"] + p["top_p"] + p["cfg_scale"])
    p = cp.resolve(2, [False, True], 1, 0, 0, 1)
    assert p["use_sampling"] == [0, 1] and p["temp"] == [1.0, 1.0]


def test_wrong_lengths_are_refused():
    with pytest.raises(L.VauraHipError, match="temp has 2 values for a batch of 4"):
        cp.resolve(4, True, [1.0, 2.0], 0, 0.0, 1.0)
    with pytest.raises(L.VauraHipError, match="top_k has 3 values but temp has 4"):
        cp.check_lengths(None, temp=[1.0] * 4, top_k=[1, 2, 3])
    with pytest.raises(L.VauraHipError, match="cfg_scale has 5 values for a batch of 4"):
        cp.check_lengths(4, temp=1.0, cfg_scale=torch.ones(5))
    with pytest.raises(L.VauraHipError, match="one-dimensional"):
        cp.check_lengths(2, temp=torch.ones(2, 2))
    cp.check_lengths(4, temp=[1.0] * 4, top_k=7)
    cp.check_lengths(None, temp=1.0)


def test_use_cfg_and_noise_follow_any_clip():
    assert cp.any_cfg(6.0) and not cp.any_cfg(1.0)
    assert cp.any_cfg([1.0, 1.0, 1.5]) and not cp.any_cfg(torch.tensor([1.0, 0.5]))
    assert cp.any_sampled(True, 1.0) and not cp.any_sampled(True, 0.0) and not cp.any_sampled(False, 1.0)
    assert cp.any_sampled([False, True], 0.7) and not cp.any_sampled([False, True], [0.7, 0.0])
    assert cp.any_sampled(True, torch.tensor([0.0, 0.2]))


def test_records_match_the_c_struct():
    assert C.sizeof(L.ClipSampling) == cp.RECORD_BYTES == 32 == L.lib().vaura_struct_size(9)
    assert L.lib().vaura_struct_size(2) == C.sizeof(L.Sampling)                  # the scalar struct is what it was
    assert L.Decoder.clip_sampling.offset == L.Decoder.vscale.offset + C.sizeof(C.c_void_p)     # appended after the last field
    assert L.Decoder().clip_sampling is None                                     # zero-filled = the scalars hold
    raw = cp.pack_records(cp.resolve(2, [True, False], [0.7, 1.0], 250, [0.0, 0.95], [6.0, 1.0]))
    assert len(raw) == 64
    rec = (L.ClipSampling * 2).from_buffer_copy(raw)
    assert (rec[0].use_sampling, rec[0].top_k, rec[1].use_sampling, rec[1].top_k) == (1, 250, 0, 250)
    f32 = lambda x: struct.unpack("f", struct.pack("f", x))[0]
    assert (rec[0].temp, rec[0].top_p, rec[0].cfg_scale) == (f32(0.7), 0.0, 6.0)
    assert (rec[1].temp, rec[1].top_p, rec[1].cfg_scale) == (1.0, f32(0.95), 1.0)
    assert list(rec[0].reserved) == [0, 0, 0]
    # the same float32 the scalar struct would carry
    assert rec[0].temp == L.Sampling(1, 0.7, 0, 0.0, 1.0, 0, 0, 0, 0.0).temp


def test_records_are_refused_without_a_device_where_no_device_is_needed():
    lib = L.lib()
    sp = L.Sampling(0, 1.0, 0, 0.0, 1.0, 0, 0, 0, 0.0)
    assert lib.vaura_sample_clips(1, 1, 9, 1024, C.byref(sp), None, None, 0, 1, None, 0, 0, None, 0) == -1      # no records
    assert lib.vaura_sample_clips(1, 1, 9, 1024, C.byref(sp), 16, None, 0, None, None, 0, 0, None, 0) == -1     # nowhere to write
    assert lib.vaura_sample_clips(1, 1, 9, 1024, C.byref(sp), 16, None, 0, None, 1, 4, 13, None, 0) == -1       # seq without state
    sp.input_is_probs = 1
    assert lib.vaura_sample_clips(1, 1, 9, 1024, C.byref(sp), 16, None, 0, 1, None, 0, 0, None, 0) == -1        # probability rows
    sp.input_is_probs = 0
    assert lib.vaura_sample_clips(1, 1, 9, 1024, C.byref(sp), 8, None, 0, 1, None, 0, 0, None, 0) == -1         # misaligned records


@pytest.mark.parametrize("total,world", [(8, 1), (8, 2), (7, 3), (5, 4), (3, 5)])
def test_parameter_lists_are_sharded_like_the_clips(total, world):
    params = dict(use_sampling=[i % 2 == 0 for i in range(total)], temp=torch.arange(total) * 0.1, top_k=list(range(total)),
                  top_p=0.0, cfg_scale=tuple(1.0 + i for i in range(total)), seed=5)
    seen = {k: [] for k in ("use_sampling", "temp", "top_k", "cfg_scale")}
    for rank in range(world):
        first, count = dist.shard(total, rank, world)
        loc = dist.shard_params(params, total, rank, world)
        assert loc["top_p"] == 0.0 and loc["seed"] == 5                                   # scalars and other keys pass through
        assert loc["top_k"] == list(range(first, first + count))
        assert torch.equal(loc["temp"], params["temp"][first:first + count])
        if count:
            assert cp.resolve(count, **{k: loc[k] for k in cp.NAMES})["cfg_scale"] == [1.0 + i for i in range(first, first + count)]
        for k in seen:
            seen[k] += list(loc[k].tolist() if hasattr(loc[k], "tolist") else loc[k])
    assert seen["top_k"] == params["top_k"] and seen["cfg_scale"] == list(params["cfg_scale"])      # every clip once, in order
    assert seen["use_sampling"] == params["use_sampling"]
    with pytest.raises(L.VauraHipError):
        dist.shard_params(dict(temp=[1.0] * (total + 1)), total, 0, world)
