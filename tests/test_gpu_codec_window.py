"""Windowed codec decode on the device: vaura_dac_decode_window (csrc/dac.hip), CodecEngine.decode_window / decode_windowed, and the
streaming callers longform.generate_long_stream / generate_long_clips_stream on top of them.

The contract is bit equality: the samples of a window are the samples the whole decode has at those frames — every comparison is
torch.equal, nothing has a tolerance — and everything behind a clip's samples is exactly 0.  Outputs of the direct library calls live
inside an allocation of 0xFF bytes whose guards must stay 0xFF, and the engine's four workspaces are filled with 0xFF before the call
(tests/test_gpu_codec_clips.py: a gap row that is never cleared is a NaN that reaches the neighbouring window's edge).

Shapes: the full-size synthetic codec.  Lengths [64, 33, 7, 21] with windows (20, 9) — interior: 10 halo frames either side —, (0, 33) —
clamped at both ends —, (3, 1) — a clip shorter than the halo — and (0, 0) — nothing asked for: 77 packed frames, the 128-row and
two-launch instances.  Lengths [150, 130] with windows (40, 100) and (0, 120): 254 packed frames, 508 256-row workgroups at the last
level, which select the 256-row and one-launch instances."""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_per_clip_sampling as G  # noqa: E402  (the tiny plugin model)
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import longform, synth  # noqa: E402
from vaura_amd.codec_clips import decode_halo, window_layout  # noqa: E402
from vaura_amd.engine import CodecEngine  # noqa: E402

DEV = "cuda:0"
CFG = synth.FULL_CODEC
HOP = CFG.hop
PRECISIONS = ["f32", "f16pair", "f16", "f16pair_w8", "mx8"]
BIG_INSTANCES = {"f16pair", "f16", "f16pair_w8"}                    # tests/test_gpu_codec_clips.py: the precisions that have them
SMALL = ([64, 33, 7, 21], [(20, 9), (0, 33), (3, 1), (0, 0)])
BIG = ([150, 130], [(40, 100), (0, 120)])


class Guarded:
    """`nbytes` of device memory inside a larger allocation filled with 0xFF; `guard` bytes (a multiple of 256) on either side."""

    def __init__(self, nbytes, guard=4096):
        assert guard % 256 == 0 and nbytes % 4 == 0
        self.n, self.g = nbytes, guard
        self.buf = torch.full((guard + nbytes + guard,), 0xFF, dtype=torch.uint8, device=DEV)

    def view(self, dtype):
        return self.buf[self.g: self.g + self.n].view(dtype)

    def check(self):
        h = self.buf.cpu()
        assert bool((h[: self.g] == 0xFF).all()), "bytes BEFORE the output were written"
        assert bool((h[self.g + self.n:] == 0xFF).all()), "bytes BEHIND the output were written"


def poison(eng):
    for w in eng._ws:
        w.view(torch.uint8).fill_(0xFF)


def counters():
    return L.lib().vaura_debug_counter(0), L.lib().vaura_debug_counter(1)      # read and clear


@pytest.fixture(scope="module")
def sd():
    return dict(synth.codec_state_dict(CFG, seed=0))


@pytest.fixture(scope="module")
def engines(sd):
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = CodecEngine(CFG, sd, DEV, precision=precision)
        return made[precision]
    return get


def padded_codes(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, CFG.codebook_size, (len(lengths), CFG.n_codebooks, max(lengths)), generator=g).to(DEV)      # random behind a clip too


def check_window(eng, lengths, windows, seed):
    """-> the counters of the window call"""
    B, T = len(lengths), max(lengths)
    starts, counts = [s for s, _ in windows], [n for _, n in windows]
    N = max(counts)
    codes = padded_codes(lengths, seed)
    whole = eng.decode_clips(codes, lengths).clone()
    got = eng.decode_window(codes, starts, counts, lengths).clone()
    assert got.shape == (B, 1, N * HOP)
    counters()
    poison(eng)
    out = Guarded(B * N * HOP * 4)
    ci = codes.to(torch.int32).contiguous()
    before = ci.clone()
    i32 = lambda v: (C.c_int32 * B)(*v)
    rc = eng.lib.vaura_dac_decode_window(C.byref(eng.c), L.ptr(ci), B, T, i32(lengths), i32(starts), i32(counts), L.ptr(out.view(torch.float32)), N,
                                         L.current_stream(torch.device(DEV)))
    assert rc == 0
    c_window = counters()
    torch.cuda.synchronize()
    out.check()
    assert torch.equal(ci, before)                                   # the caller's codes are untouched
    wav = out.view(torch.float32).reshape(B, 1, N * HOP)
    assert bool(torch.isfinite(wav).all()), "a 0xFF byte of the workspace reached the output"
    for b, (s, n) in enumerate(windows):
        want = whole[b, :, s * HOP:(s + n) * HOP]
        d = float((wav[b, :, :n * HOP] - want).abs().max()) if n else 0.0
        print(f"clip {b}: T_b = {lengths[b]}, frames [{s}, {s + n}): max |window - whole| = {d:.3e}")
        assert torch.equal(wav[b, :, :n * HOP], want), (b, s, n, d)
        assert bool((wav[b, :, n * HOP:] == 0).all()), (b, s, n)
    assert torch.equal(got, wav)                                     # the engine method is that call
    return c_window


@pytest.mark.parametrize("precision", PRECISIONS)
def test_window_is_the_slice_of_the_whole_decode(engines, precision):
    assert check_window(engines(precision), *SMALL, seed=1) == (0, 0)        # 77 packed frames: the small instances


@pytest.mark.parametrize("precision", PRECISIONS)
def test_tall_windows_run_the_256_row_and_one_launch_instances(engines, precision):
    lay = window_layout(BIG[0], [s for s, _ in BIG[1]], [n for _, n in BIG[1]], CFG)
    assert lay.total * HOP // 256 >= 384
    c_window = check_window(engines(precision), *BIG, seed=2)
    print(f"{precision}: 256-row launches / one-launch units of the window call: {c_window}")
    if precision in BIG_INSTANCES:
        assert c_window[0] > 0 and c_window[1] > 0
    else:
        assert c_window == (0, 0)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_decode_windowed_is_the_one_pass(engines, precision):
    eng = engines(precision)
    lengths = [50, 17, 33]
    codes = padded_codes(lengths, 3)
    plain, clips = eng.decode(codes).clone(), eng.decode_clips(codes, lengths).clone()
    for window in (16, 1):
        assert torch.equal(eng.decode_windowed(codes, window), plain), window
        assert torch.equal(eng.decode_windowed(codes, window, lengths), clips), window
    assert torch.equal(eng.decode_windowed(codes, 50), plain) and torch.equal(eng.decode_windowed(codes, 64, lengths), clips)
    with pytest.raises(L.VauraHipError, match="window must be a positive"):
        eng.decode_windowed(codes, 0)
    with pytest.raises(L.VauraHipError, match="every count is 0"):
        eng.decode_window(codes, [0, 0, 0], [0, 0, 0], lengths)
    with pytest.raises(L.VauraHipError, match="inside its clip"):
        eng.decode_window(codes, [0, 10, 0], [5, 8, 5], lengths)


def test_decode_windowed_sizes_the_workspaces_by_the_window(sd):
    eng = CodecEngine(CFG, sd, DEV)                                  # fresh: its workspaces have seen nothing else
    B, T, window = 3, 50, 16
    codes = padded_codes([T] * B, 4)
    got = eng.decode_windowed(codes, window)
    i32 = lambda v: (C.c_int32 * B)(*v)
    need = max(eng.lib.vaura_dac_decode_window_workspace_elems(C.byref(eng.c), B, i32([T] * B), i32([s] * B), i32([min(window, T - s)] * B))
               for s in range(0, T, window))
    one_pass = eng.lib.vaura_dac_workspace_elems(C.byref(eng.c), B, T)
    H = decode_halo(CFG)
    assert need == (B * (H + window + H) + 2 * 4) * HOP * 96         # the widest call: a window with both halos per clip, two gaps
    assert all(w.numel() == need for w in eng._ws) and eng.c.ws_elems == need < one_pass
    assert torch.equal(got, eng.decode(codes))                       # (this grows them)
    assert eng.c.ws_elems == one_pass


# ---------------------------------------------------------------------------------------------------------------- the callers
@pytest.fixture(scope="module")
def model(tiny_sampler_sd):
    return G._model(tiny_sampler_sd)


REL = ("relevance", "logprob_cond", "logprob_null")


def joined(blocks, key="audio"):
    return torch.cat([b[key] for b in blocks], dim=-1)


@pytest.mark.parametrize("way", [dict(use_sampling=False, cfg_scale=1.0), dict(use_sampling=True, temp=0.9, top_k=128, cfg_scale=3.0)],
                         ids=["greedy", "sampled_cfg3"])
def test_stream_blocks_are_generate_long_cut_up(model, way):
    # 3.84 s at the released geometry: three chunks of 221 frames, 4 segments of 8 tokens each (the 32 the null embedding holds)
    B = 2
    feats = synth.video_features(B, tokens=6 * 8, seed=71).reshape(B, 6, 8, 768).to(DEV)
    ref = longform.generate_long(model, feats, 3.84, **way)
    assert ref["sampled_indices"].shape[-1] == 331
    blocks = list(longform.generate_long_stream(model, feats, 3.84, **way))
    assert [b["frames"] for b in blocks] == [211, 55, 65] and [b["start_frame"] for b in blocks] == [0, 211, 266]
    assert [b["final"] for b in blocks] == [False, False, True]
    assert torch.equal(joined(blocks, "sampled_indices"), ref["sampled_indices"])
    for b in blocks:
        lo, hi = b["start_frame"] * HOP, (b["start_frame"] + b["frames"]) * HOP
        d = float((b["audio"] - ref["generated_audio"][..., lo:hi]).abs().max())
        print(f"frames [{b['start_frame']}, {b['start_frame'] + b['frames']}): max |block - one pass| = {d:.3e}")
    assert torch.equal(joined(blocks), ref["generated_audio"])
    two = list(longform.generate_long_stream(model, feats, 3.84, emit_chunks=2, **way))
    assert [b["frames"] for b in two] == [266, 65]
    assert torch.equal(joined(two), ref["generated_audio"]) and torch.equal(joined(two, "sampled_indices"), ref["sampled_indices"])
    windowed = longform.generate_long(model, feats, 3.84, codec_window=64, **way)
    assert torch.equal(windowed["generated_audio"], ref["generated_audio"]) and torch.equal(windowed["sampled_indices"], ref["sampled_indices"])


def test_stream_carries_the_relevance_values_and_serves_a_single_chunk(model):
    B = 2
    feats = synth.video_features(B, tokens=6 * 8, seed=71).reshape(B, 6, 8, 768).to(DEV)
    kw = dict(use_sampling=True, temp=0.9, top_k=128, cfg_scale=1.0, return_relevance=True)
    ref = longform.generate_long(model, feats, 3.84, **kw)
    blocks = list(longform.generate_long_stream(model, feats, 3.84, **kw))
    for k in REL + ("sampled_indices",):
        assert torch.equal(joined(blocks, k), ref[k]), k
    assert torch.equal(joined(blocks), ref["generated_audio"])
    one = synth.video_features(B, tokens=4 * 8, seed=71).reshape(B, 4, 8, 768).to(DEV)
    ref = longform.generate_long(model, one, 0.5, use_sampling=False)
    blocks = list(longform.generate_long_stream(model, one, 0.5, use_sampling=False))
    assert len(blocks) == 1 and blocks[0]["final"] and blocks[0]["frames"] == 43
    assert torch.equal(blocks[0]["audio"], ref["generated_audio"]) and torch.equal(blocks[0]["sampled_indices"], ref["sampled_indices"])
    assert torch.equal(longform.generate_long(model, one, 0.5, use_sampling=False, codec_window=16)["generated_audio"], ref["generated_audio"])


def test_clips_stream_gives_every_clip_the_bits_of_generate_long_clips(model):
    # the batch of tests/test_gpu_longform_clips.py: 26-frame window, 8-frame stride; 5 / 1 / 3 / 4 / 1 / 2 chunks
    geo = dict(stride=0.10, model_max_duration=0.30, vfps=440)
    durations, lengths = [0.62, 0.27, 0.45, 0.50, 0.31, 0.40], [54, 23, 39, 43, 26, 34]
    B = len(durations)
    feats = synth.video_features(B, tokens=16, seed=71).reshape(B, 4, 4, 768).to(DEV)
    kw = dict(use_sampling=False, cfg_scale=1.0)
    ref = longform.generate_long_clips(model, feats, durations, **geo, **kw)
    assert ref["lengths"].tolist() == lengths
    blocks = list(longform.generate_long_clips_stream(model, feats, durations, **geo, **kw))
    assert len(blocks) == 5 and [b["final"] for b in blocks] == [False] * 4 + [True]
    assert blocks[0]["frames"] == [16, 23, 16, 16, 26, 16]            # window - halo; the single-chunk clips whole
    at = [0] * B
    audio = torch.zeros_like(ref["generated_audio"])
    tokens = torch.full_like(ref["sampled_indices"], model.special_token_id)
    for blk in blocks:
        assert blk["start_frames"] == at
        for b, n in enumerate(blk["frames"]):
            audio[b, :, at[b] * HOP:(at[b] + n) * HOP] = blk["audio"][b, :, :n * HOP]
            tokens[b, :, at[b]:at[b] + n] = blk["sampled_indices"][b, :, :n]
            assert bool((blk["audio"][b, :, n * HOP:] == 0).all()), b
            at[b] += n
    assert at == lengths
    assert torch.equal(tokens, ref["sampled_indices"])
    for b in range(B):
        d = float((audio[b] - ref["generated_audio"][b]).abs().max())
        print(f"clip {b}: max |blocks - one pass| = {d:.3e}")
    assert torch.equal(audio, ref["generated_audio"])
    windowed = longform.generate_long_clips(model, feats, durations, codec_window=16, **geo, **kw)
    assert torch.equal(windowed["generated_audio"], ref["generated_audio"]) and torch.equal(windowed["sampled_indices"], ref["sampled_indices"])
