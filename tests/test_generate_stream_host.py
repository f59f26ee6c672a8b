"""Streaming inside one generate() call, the host side: the schedule of the loop's pieces (clip_params.stream_schedule), the refusals
of DecoderEngine.generate_codes_stream / VAURAModel.generate_stream / longform.generate_long_stream(block_frames=...), which happen at
call time and before any engine work, and the new C symbols.  No GPU."""
import inspect
import itertools

import pytest
import torch

from vaura_amd import _lib as L
from vaura_amd import clip_params, longform
from vaura_amd.engine import CodecEngine, DecoderEngine
from vaura_amd.model import VAURAModel

H = 10                                   # codec_clips.decode_halo of the 44.1 kHz geometry
DELAYS = {"0..8": list(range(9)), "parallel": [0] * 9, "uneven": [0, 0, 1, 3]}


def clip_lengths(T):
    """per-clip length sets for a call of T frames: None (one length), and mixes that hold 1, a value <= H and T itself"""
    out = [None, [T, 1]]
    if T > 1:
        out.append([T, min(T, H), 1, max(1, T - 1)])
    if T > H + 1:
        out.append([H + 1, T, H])
    return out


def cases():
    for T, bf, name in itertools.product((1, 9, 10, 11, 12, 43), (1, 4, 7, 16, 64), DELAYS):
        for Tp in sorted({0, 3, T - 1}):
            if Tp >= T or Tp < 0:
                continue
            for lens in clip_lengths(T):
                if lens is not None and Tp >= min(lens):
                    continue             # a common prompt is shorter than every clip
                yield T, bf, name, Tp, lens


@pytest.mark.parametrize("T,bf,name,Tp,lens", list(cases()))
def test_stream_schedule(T, bf, name, Tp, lens):
    d = DELAYS[name]
    d_max = max(d)
    S, start = T + d_max + 1, Tp + 1 + d[0]
    pieces = clip_params.stream_schedule(T, lens, start, d, H, bf)
    assert all(n >= 1 for n, _ in pieces)
    assert sum(n for n, _ in pieces) == S - start                      # the loop's sampled steps, all of them, once
    T_b = [T] if lens is None else lens
    at, j = [0] * len(T_b), 0
    for i, (n, ranges) in enumerate(pieces):
        j += n
        assert len(ranges) == len(T_b)
        for b, (lo, hi) in enumerate(ranges):
            assert lo == at[b] and lo <= hi <= T_b[b]                  # in order, without gap or overlap
            F_b = min(clip_params.final_frames(j, T, start, d_max), T_b[b])
            if hi > lo:
                # the last frame of the range is final: its last codebook's step lies among the j sampled ones
                assert (hi - 1) + 1 + d_max < start + j, (i, b, lo, hi, j)
                assert hi <= F_b
            if hi != T_b[b]:
                assert hi <= max(0, F_b - H), (i, b, hi, F_b)          # only a clip's last range comes within H of F_b
            at[b] = hi
    assert at == T_b                                                    # every clip is tiled to its end


def test_schedule_of_the_issue_example():
    # 220 frames, delays 0..8, no prompt, 16-frame blocks: the first block is due after 34 of 228 sampled steps (229 sequence steps)
    pieces = clip_params.stream_schedule(220, None, 1, None, H, 16, num_codebooks=9)
    assert pieces[0] == (34, [(0, 16)]) and pieces[1] == (16, [(16, 32)])
    assert sum(n for n, _ in pieces) == 228 and pieces[-1][1] == [(208, 220)]
    assert clip_params.stream_schedule(43, None, 1, None, H, 64, num_codebooks=9) == [(51, [(0, 43)])]      # one block
    # a clip of at most H frames appears once, in the piece that finishes it
    ranges = [r[2] for _, r in clip_params.stream_schedule(43, [43, 23, 9], 1, None, H, 4, num_codebooks=9)]
    assert [r for r in ranges if r[1] > r[0]] == [(0, 9)]


@pytest.mark.parametrize("bad", [0, -1, 2.0, True, None, "16"])
def test_bad_block_frames(bad):
    with pytest.raises(L.VauraHipError, match="block_frames"):
        clip_params.stream_schedule(43, None, 1, list(range(9)), H, bad)


# ------------------------------------------------------------------------------------------------------------ refusals
class Untouchable:
    """Stands where an engine / sampler / extractor would be: any use is an error of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the refusal came too late: .{name} was reached")


def bare_engine(near_tie="report"):
    eng = object.__new__(DecoderEngine)      # no __init__: no library, no device
    eng.near_tie = near_tie
    for name in ("prepare", "run", "set_condition", "start_sequence", "_begin_sequence", "_codes_stream", "_finish_sequence", "_status_fallback"):
        setattr(eng, name, Untouchable())
    return eng


FEATS = torch.zeros(2, 32, 768)


@pytest.mark.parametrize("kw,match", [
    (dict(num_candidates=2), "num_candidates"),
    (dict(prompt=torch.zeros(2, 9, 5, dtype=torch.int64), prompt_lengths=[2, 5]), "one prompt length"),
    (dict(block_frames=0), "block_frames"),
    (dict(block_frames=True), "block_frames"),
])
def test_engine_refuses_at_call_time(kw, match):
    with pytest.raises(L.VauraHipError, match=match):
        bare_engine().generate_codes_stream(FEATS, 43, **kw)


def test_engine_refuses_near_tie_rerun_at_call_time():
    with pytest.raises(L.VauraHipError, match="rerun"):
        bare_engine("rerun").generate_codes_stream(FEATS, 43)


def bare_model(near_tie="report"):
    m = object.__new__(VAURAModel)
    torch.nn.Module.__init__(m)
    m.training = False
    sampler = Untouchable()
    object.__setattr__(sampler, "near_tie", near_tie)
    m.__dict__.update(sampler=sampler, audio_encoder=Untouchable(), visual_feature_extractor=Untouchable(), pattern_provider=Untouchable())
    return m


FRAMES = torch.zeros(2, 1, 32, 768)


@pytest.mark.parametrize("kw,match", [
    (dict(num_candidates=2), "num_candidates"),
    (dict(num_candidates=True), "num_candidates"),
    (dict(audio=torch.zeros(2, 9, 5, dtype=torch.int64), prompt_is_encoded=True, prompt_lengths=[2, 5]), "one prompt length"),
    (dict(block_frames=0), "block_frames"),
    (dict(block_frames=1.5), "block_frames"),
])
def test_model_refuses_before_any_engine_call(kw, match):
    with pytest.raises(L.VauraHipError, match=match):
        bare_model().generate_stream(frames=FRAMES, max_new_tokens=43, **kw)


def test_model_refuses_near_tie_rerun_before_any_engine_call():
    with pytest.raises(L.VauraHipError, match="rerun"):
        bare_model("rerun").generate_stream(frames=FRAMES, max_new_tokens=43)


def test_long_stream_refuses_bad_block_frames_and_emit_chunks():
    class M:
        sampler = Untouchable()
    with pytest.raises(L.VauraHipError, match="block_frames"):
        longform.generate_long_stream(M(), FRAMES, 3.84, block_frames=0)
    with pytest.raises(L.VauraHipError, match="emit_chunks must stay 1"):
        longform.generate_long_stream(M(), FRAMES, 3.84, block_frames=16, emit_chunks=2)


# ------------------------------------------------------------------------------------------------------------ surface and symbols
def test_symbols_and_keywords():
    for name in ("vaura_dac_decode_window_seq", "vaura_dac_decode_window_seq_workspace_elems"):
        assert name in L.SIGNATURES
        assert hasattr(L.lib(), name), f"{name} is not exported"
    # refused without a device: NULL arguments never reach a launch
    lib = L.lib()
    assert lib.vaura_dac_decode_window_seq(None, 0, 1, 9, 52, None, None, None, None, 0, 1, 0) == -1
    assert lib.vaura_dac_decode_window_seq_workspace_elems(None, 1, 9, 52, None, None, None, None) == 0
    assert "block_frames" in inspect.signature(DecoderEngine.generate_codes_stream).parameters
    assert "block_frames" in inspect.signature(VAURAModel.generate_stream).parameters
    assert inspect.signature(longform.generate_long_stream).parameters["block_frames"].default is None
    assert "block_frames" not in inspect.signature(longform.generate_long_clips_stream).parameters
    assert hasattr(CodecEngine, "decode_window_seq")
    for refused in ("return_all_candidates", "rank_by", "remove_prompts"):
        assert refused not in inspect.signature(VAURAModel.generate_stream).parameters


def test_window_seq_argument_checks_on_the_host():
    """A codec descriptor of the 44.1 kHz geometry without device memory: everything the call refuses, it refuses before a launch."""
    import ctypes as C
    from vaura_amd import synth
    cfg = synth.FULL_CODEC
    c = L.Codec()
    c.n_codebooks, c.codebook_size, c.codebook_dim, c.latent_dim = cfg.n_codebooks, cfg.codebook_size, cfg.codebook_dim, cfg.latent_dim
    c.n_blocks, c.n_units = len(cfg.decoder_rates), 3
    for i, r in enumerate(cfg.decoder_rates):
        c.rates[i] = r
    ch = 1536

    def conv(cv, cin, cout, taps, dil, stride):
        cv.cin, cv.cout, cv.taps, cv.dilation, cv.stride = cin, cout, taps, dil, stride
    conv(c.conv_in, cfg.latent_dim, ch, 7, 1, 1)
    for b, r in enumerate(cfg.decoder_rates):
        conv(c.up[b], ch, ch // 2, 2, 1, r)
        ch //= 2
        for u, dil in enumerate(cfg.dilations):
            conv(c.res[b][u][0], ch, ch, 7, dil, 1)
            conv(c.res[b][u][1], ch, ch, 1, 1, 1)
    conv(c.conv_out, ch, 1, 7, 1, 1)
    lib = L.lib()
    assert lib.vaura_dac_decode_halo(C.byref(c)) == H
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    K, S = 9, 52                                                       # T = 43 under the delays 0..8
    elems = lambda *a: lib.vaura_dac_decode_window_seq_workspace_elems(C.byref(c), *a)
    whole = lib.vaura_dac_decode_window_workspace_elems(C.byref(c), 2, i32(43, 23), i32(0, 3), i32(16, 20))
    assert whole > 0 and elems(2, K, S, None, i32(43, 23), i32(0, 3), i32(16, 20)) == whole      # the plan of the window call
    assert elems(2, K, S, i32(*range(9)), i32(43, 23), i32(0, 3), i32(16, 20)) == whole
    assert elems(2, K, S, None, i32(44, 23), i32(0, 3), i32(16, 20)) == 0     # a clip longer than the sequence holds frames
    assert elems(2, K, S, i32(*([0] * 9)), i32(51, 23), i32(0, 3), i32(16, 20)) > 0      # the parallel pattern: T = 51
    assert elems(2, 8, S, None, i32(43, 23), i32(0, 3), i32(16, 20)) == 0     # fewer rows than the codec has codebooks
    assert elems(2, 17, S, None, i32(43, 23), i32(0, 3), i32(16, 20)) == 0
    assert elems(2, K, S, i32(0, 1, 2, 3, 4, 5, 6, 7, -1), i32(43, 23), i32(0, 3), i32(16, 20)) == 0
    assert elems(2, K, 9, None, i32(1, 1), i32(0, 0), i32(1, 1)) == 0         # S - 1 - max(d) = 0 frames
    # the call itself: a non-NULL dummy for seq / wav is never dereferenced, the workspaces are NULL -> VAURA_ERR_ARG after the plan
    call = lambda *a: lib.vaura_dac_decode_window_seq(C.byref(c), 4096, *a, 4096, 20, 0)
    assert call(2, K, S, None, i32(44, 23), i32(0, 3), i32(16, 20)) == -1
    assert call(2, 8, S, None, i32(43, 23), i32(0, 3), i32(16, 20)) == -1
    assert call(2, K, S, None, i32(43, 23), i32(0, 3), i32(16, 20)) == -1     # (workspaces NULL)
