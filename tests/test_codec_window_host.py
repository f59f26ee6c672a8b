"""Windowed codec decode, host side: the halo (codec_clips.decode_halo against the library's vaura_dac_decode_halo, and its tightness
against the CPU oracle), the window layout (codec_clips.window_layout), what vaura_dac_decode_window refuses before any launch, and
the emission schedule of longform.generate_long_stream / generate_long_clips_stream on a fake model that records its calls."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_codec_clips_host as HOST  # noqa: E402  (descriptors(): the library's descriptor with the geometry only)
from oracle import dac_oracle  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import longform, synth  # noqa: E402
from vaura_amd.codec_clips import decode_gap, decode_halo, window_layout  # noqa: E402

H = 10
HOP = 512


# ---------------------------------------------------------------------------------------------------------------- the halo
def test_halo_in_python_and_in_the_library():
    assert decode_halo(synth.FULL_CODEC) == decode_halo(synth.tiny_codec()) == H
    seen = set()
    for cfg in [synth.FULL_CODEC, synth.tiny_codec()] + HOST.OTHER:
        d, _ = HOST.descriptors(cfg)
        assert L.lib().vaura_dac_decode_halo(C.byref(d)) == decode_halo(cfg), cfg
        seen.add(decode_halo(cfg))
    # dilation 27 at 8 rows per frame: 3 * (1 + 3 + 27) rows more than conv_in's 3 frames and the transposed convs' share
    assert decode_halo(HOST.OTHER[0]) > H > decode_halo(HOST.OTHER[2])
    assert len(seen) > 2, "a hard-coded halo would pass"
    assert L.lib().vaura_dac_decode_halo(None) == -1
    d, _ = HOST.descriptors(synth.FULL_CODEC)
    d.conv_out.taps = 6                                             # an even kernel has no centre
    assert L.lib().vaura_dac_decode_halo(C.byref(d)) == -1
    d, _ = HOST.descriptors(synth.FULL_CODEC)
    d.up[1].stride = 3                                              # a transposed conv that does not follow its block's rate
    assert L.lib().vaura_dac_decode_halo(C.byref(d)) == -1
    d, _ = HOST.descriptors(synth.FULL_CODEC)
    d.n_units = 2
    assert L.lib().vaura_dac_decode_halo(C.byref(d)) == -1


def test_halo_is_tight_against_the_oracle():
    """Changing the codes of frame 30 changes the samples of frames 20 .. 40 and no other: the same oracle call on the same positions,
    so everything outside is equal bit for bit, and the two outermost frames do move."""
    cfg = synth.tiny_codec()
    sd = synth.codec_state_dict(cfg, seed=0)
    T, f = 64, 30
    codes = torch.randint(0, cfg.codebook_size, (1, cfg.n_codebooks, T), generator=torch.Generator().manual_seed(3))
    other = codes.clone()
    other[:, :, f] = (other[:, :, f] + 1 + torch.arange(cfg.n_codebooks)) % cfg.codebook_size
    a = dac_oracle.decode(sd, codes, cfg.decoder_rates).reshape(T, HOP)
    b = dac_oracle.decode(sd, other, cfg.decoder_rates).reshape(T, HOP)
    moved = [t for t in range(T) if not torch.equal(a[t], b[t])]
    print("output frames that moved:", moved)
    assert moved[0] == f - H and moved[-1] == f + H
    for t in list(range(0, f - H)) + list(range(f + H + 1, T)):
        assert torch.equal(a[t], b[t]), t


# ---------------------------------------------------------------------------------------------------------------- layout
def test_window_layout_arithmetic():
    cfg = synth.FULL_CODEC
    gap = decode_gap(cfg)
    lay = window_layout([64, 33, 7, 21], [20, 0, 3, 0], [9, 33, 1, 0], cfg)
    assert lay.halo == H and lay.gap == gap == 4 and lay.hop == HOP
    assert lay.clips == (0, 1, 2)                                   # count 0: no window
    assert lay.lo == (10, 0, 0) and lay.hi == (39, 33, 7)           # interior; clamped at both ends; a clip shorter than the halo
    assert lay.skips == (10, 0, 3)
    assert lay.offsets == (0, 29 + gap, 29 + gap + 33 + gap) and lay.total == 29 + 33 + 7 + 2 * gap
    # clamps: at 0 only, at the length only
    lay = window_layout([100, 100], [4, 85], [20, 15], cfg)
    assert lay.lo == (0, 75) and lay.hi == (34, 100) and lay.skips == (4, 10) and lay.offsets == (0, 34 + gap)
    # count 1 in the middle: 2 H + 1 frames; one window: no gap anywhere
    lay = window_layout([100], [50], [1], cfg)
    assert lay.lo == (40,) and lay.hi == (61,) and lay.total == 2 * H + 1 and lay.offsets == (0,)
    # every count 0: no window at all
    lay = window_layout([5, 6], [0, 6], [0, 0], cfg)
    assert lay.clips == () and lay.total == 0
    # the library sizes its workspaces for the same sequence
    d, _ = HOST.descriptors(cfg)
    d.latent_dim, d.conv_in.cout, d.n_codebooks = 8, 16, 9
    for b in range(4):
        d.up[b].cout = 16 >> (b + 1)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    lay = window_layout([64, 33, 7, 21], [20, 0, 3, 0], [9, 33, 1, 0], cfg)
    one = L.lib().vaura_dac_workspace_elems(C.byref(d), 1, lay.total)
    got = L.lib().vaura_dac_decode_window_workspace_elems(C.byref(d), 4, i32(64, 33, 7, 21), i32(20, 0, 3, 0), i32(9, 33, 1, 0))
    assert got == max(one, 9 * lay.total) > 0
    # without lengths no window is clamped at its clip's end: an upper bound
    free = L.lib().vaura_dac_decode_window_workspace_elems(C.byref(d), 4, None, i32(20, 0, 3, 0), i32(9, 33, 1, 0))
    assert free == L.lib().vaura_dac_workspace_elems(C.byref(d), 1, 29 + 43 + 14 + 2 * gap) > got


@pytest.mark.parametrize("lengths,starts,counts", [
    ([], [], []), ([5], [0, 0], [1, 1]), ([5], [-1], [2]), ([5], [0], [-1]), ([5], [3], [3]), ([0], [0], [0]), ([5], [0], [2.0]), ([5], [True], [1])])
def test_window_layout_refuses(lengths, starts, counts):
    with pytest.raises(ValueError):
        window_layout(lengths, starts, counts, synth.FULL_CODEC)


# ---------------------------------------------------------------------------------------------------------------- C entry points
def test_entry_point_refuses_before_any_launch():
    lib = L.lib()
    one = C.c_void_p(16)                                            # points nowhere: nothing may be dereferenced
    d, _ = HOST.descriptors(synth.FULL_CODEC)
    d.n_codebooks, d.codebook_dim, d.latent_dim, d.conv_in.cout = 9, 8, 1024, 1536
    for b in range(4):
        d.up[b].cout = 1536 >> (b + 1)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    n, s, c = i32(64, 33), i32(20, 0), i32(9, 33)
    call = lambda *a: lib.vaura_dac_decode_window(*a)
    # NULL pointers; lengths may be NULL, starts and counts may not
    assert call(None, one, 2, 64, n, s, c, one, 33, None) == -1
    assert call(C.byref(d), None, 2, 64, n, s, c, one, 33, None) == -1
    assert call(C.byref(d), one, 2, 64, n, None, c, one, 33, None) == -1
    assert call(C.byref(d), one, 2, 64, n, s, None, one, 33, None) == -1
    assert call(C.byref(d), one, 2, 64, n, s, c, None, 33, None) == -1
    assert call(C.byref(d), one, 0, 64, n, s, c, one, 33, None) == -1
    assert call(C.byref(d), one, 2, 0, n, s, c, one, 33, None) == -1
    assert call(C.byref(d), one, 2, 64, n, s, c, one, 0, None) == -1
    assert lib.vaura_dac_decode_window_workspace_elems(None, 2, n, s, c) == 0
    assert lib.vaura_dac_decode_window_workspace_elems(C.byref(d), 2, n, None, c) == 0
    assert lib.vaura_dac_decode_window_workspace_elems(C.byref(d), 2, n, s, None) == 0
    # a negative start or count, a window behind its clip's end, a count beyond the output, a length outside 1 .. T_max, every count 0
    d.ws_elems = 2 ** 62                                            # the workspace is not the reason
    for lens, st, ct in ((n, i32(-1, 0), c), (n, s, i32(9, -1)), (n, i32(56, 0), c), (n, s, i32(9, 34)), (i32(64, 0), s, i32(9, 0)), (n, s, i32(0, 0))):
        assert call(C.byref(d), one, 2, 64, lens, st, ct, one, 40, None) == -1
        assert lib.vaura_dac_decode_window_workspace_elems(C.byref(d), 2, lens, st, ct) == 0
    assert call(C.byref(d), one, 2, 64, i32(65, 33), s, c, one, 33, None) == -1          # a length beyond T_max
    assert call(C.byref(d), one, 2, 64, None, i32(20, 32), c, one, 33, None) == -1       # lengths NULL: T_max each, 32 + 33 > 64
    assert call(C.byref(d), one, 2, 64, n, s, i32(9, 33), one, 32, None) == -1          # counts[1] > N_max
    # good arguments: refused for the workspace (too small; then large enough with the four pointers NULL)
    need = lib.vaura_dac_decode_window_workspace_elems(C.byref(d), 2, n, s, c)
    assert need == (29 + 4 + 33) * 512 * 96
    d.ws_elems = need - 1
    assert call(C.byref(d), one, 2, 64, n, s, c, one, 33, None) == -1
    d.ws_elems = need
    assert call(C.byref(d), one, 2, 64, n, s, c, one, 33, None) == -1
    assert call(C.byref(d), one, 2, 64, None, s, c, one, 33, None) == -1                # lengths NULL: T_max each, the same refusal
    # packed windows whose widest level leaves the int range: VAURA_ERR_SHAPE, whatever the workspace
    d.ws_elems = 2 ** 62
    big = i32(30000, 30000)
    assert call(C.byref(d), one, 2, 30000, big, i32(0, 0), big, one, 30000, None) == -2
    assert lib.vaura_dac_decode_window_workspace_elems(C.byref(d), 2, big, i32(0, 0), big) > 2 ** 31
    # ... while a window of such clips is fine: refused only for the NULL workspaces
    assert call(C.byref(d), one, 2, 30000, big, i32(15000, 0), i32(64, 64), one, 64, None) == -1
    assert lib.vaura_dac_decode_window_workspace_elems(C.byref(d), 2, big, i32(15000, 0), i32(64, 64)) == (84 + 4 + 74) * 512 * 96
    d.conv_out.taps = 6                                             # no halo for this descriptor
    assert call(C.byref(d), one, 2, 64, n, s, c, one, 33, None) == -2
    assert lib.vaura_dac_decode_window_workspace_elems(C.byref(d), 2, n, s, c) == 0


# ---------------------------------------------------------------------------------------------------------------- emission schedule
class FakeCodec:
    cfg = synth.FULL_CODEC

    def __init__(self):
        self.windows, self.decodes = [], 0

    def decode_window(self, codes, starts, counts, lengths=None):
        self.windows.append(dict(T=int(codes.shape[-1]), starts=list(starts), counts=list(counts), lengths=None if lengths is None else list(lengths),
                                 first=[int(codes[b, 0, s]) if n else None for b, (s, n) in enumerate(zip(starts, counts))]))
        return torch.zeros(codes.shape[0], 1, max(counts) * HOP)

    def decode(self, codes):
        self.decodes += 1
        return torch.zeros(codes[0][0].shape[0], 1, codes[0][0].shape[-1] * HOP)


class FakeModel:
    """Records its calls.  The token of frame f of a clip is f: a chunk counts on from the last token of its prompt."""
    num_codebooks, special_token_id = 9, 1024

    def __init__(self, block_size=256):
        self.audio_encoder = FakeCodec()
        self.sampler = type("S", (), {"config": type("Cfg", (), {"block_size": block_size})()})()
        self.calls = []

    def generate_tokens(self, frames=None, audio=None, max_new_tokens=None, **kw):
        B = frames.shape[0]
        per_clip = isinstance(max_new_tokens, (list, tuple))
        T = list(max_new_tokens) if per_clip else [max_new_tokens] * B
        P = 0 if audio is None else int(audio.shape[-1])
        self.calls.append(dict(T=T, P=P))
        tok = torch.full((B, 9, max(T)), self.special_token_id, dtype=torch.int64)
        for b in range(B):
            first = 0 if audio is None else int(audio[b, 0, -1]) + 1 - P
            tok[b, :, :T[b]] = torch.arange(first, first + T[b])
        if kw.get("return_relevance"):
            return {"tokens": tok, **{k: tok.float() for k in longform.REL}}
        return {"tokens": tok} if per_clip else tok

    def generate(self, frames=None, audio=None, max_new_tokens=None, **kw):
        tok = self.generate_tokens(frames=frames, audio=audio, max_new_tokens=max_new_tokens, **kw)
        rel = tok if isinstance(tok, dict) else {}
        tok = rel.pop("tokens") if rel else tok
        return {"generated_audio": self.audio_encoder.decode([(tok, None)]), "sampled_indices": tok, **rel}


FRAMES = torch.zeros(2, 6, 8, 768)


def check_blocks(blocks, total, expect_frames=None):
    """The blocks tile [0, total) without overlap, carry their own frames, and only the last is final."""
    at = 0
    for i, blk in enumerate(blocks):
        n = blk["frames"]
        assert blk["start_frame"] == at and n >= 1
        assert blk["audio"].shape == (2, 1, n * HOP) and blk["sampled_indices"].shape == (2, 9, n)
        assert torch.equal(blk["sampled_indices"][0, 0], torch.arange(at, at + n))
        assert blk["final"] == (i + 1 == len(blocks))
        at += n
    assert at == total
    if expect_frames is not None:
        assert [blk["frames"] for blk in blocks] == expect_frames


def test_stream_emits_what_is_final_after_every_chunk():
    m = FakeModel()
    sched = longform.chunk_schedule(3.84)
    assert [(c["offset"], c["max_gen_len"]) for c in sched] == [(0, 221), (55, 221), (110, 221)]      # ceil(2.56 * 86): the last chunk ends one frame behind int(3.84 * 86)
    stream = longform.generate_long_stream(m, FRAMES, 3.84, use_sampling=False)
    assert not m.calls                                              # nothing runs before the first block is asked for
    first = next(stream)
    assert len(m.calls) == 1 and first["frames"] == 221 - H and first["start_frame"] == 0 and not first["final"]
    blocks = [first] + list(stream)
    check_blocks(blocks, 331, [211, 55, 65])
    assert m.audio_encoder.decodes == 0 and len(m.calls) == 3
    w = m.audio_encoder.windows
    # the codec sees the frames asked for and the halo in front of them, not the clip: 221, then 10 + 55 + 10, then 10 + 65
    assert [x["T"] for x in w] == [221, 75, 75] and [x["starts"] for x in w] == [[0, 0], [10, 10], [10, 10]]
    assert [x["counts"] for x in w] == [[211, 211], [55, 55], [65, 65]] and [x["first"] for x in w] == [[0, 0], [211, 211], [266, 266]]


@pytest.mark.parametrize("emit,frames", [(3, [331]), (2, [266, 65]), (4, [331])])
def test_stream_emit_chunks(emit, frames):
    m = FakeModel()
    blocks = list(longform.generate_long_stream(m, FRAMES, 3.84, emit_chunks=emit, use_sampling=False))
    check_blocks(blocks, 331, frames)
    assert len(m.audio_encoder.windows) == len(frames)


def test_stream_of_ten_seconds_and_relevance():
    m = FakeModel()
    blocks = list(longform.generate_long_stream(m, FRAMES, 10.24, emit_chunks=3, use_sampling=False, return_relevance=True))
    n_chunks = len(longform.chunk_schedule(10.24))
    assert len(m.calls) == n_chunks == 13 and len(blocks) == 5
    check_blocks(blocks, 881)
    for blk in blocks:
        for k in longform.REL:                                      # the values travel with their frames
            assert torch.equal(blk[k], blk["sampled_indices"].float())


def test_stream_single_chunk_yields_once():
    m = FakeModel()
    blocks = list(longform.generate_long_stream(m, FRAMES, 2.0, emit_chunks=2, use_sampling=False))
    check_blocks(blocks, 172, [172])
    assert m.audio_encoder.decodes == 1 and not m.audio_encoder.windows


def test_stream_refuses_before_any_call():
    m = FakeModel()
    for bad in (0, -1, 1.5, True):
        with pytest.raises(L.VauraHipError, match="emit_chunks"):
            longform.generate_long_stream(m, FRAMES, 3.84, emit_chunks=bad)
    with pytest.raises(L.VauraHipError):
        longform.generate_long_stream(m, FRAMES, [3.84, 2.0])
    for bad in (0, 2.5, True):
        with pytest.raises(L.VauraHipError, match="codec_window"):
            longform.generate_long(m, FRAMES, 3.84, codec_window=bad)
        with pytest.raises(L.VauraHipError, match="codec_window"):
            longform.generate_long_clips(m, FRAMES, [3.84, 2.0], codec_window=bad)
    assert not m.calls


def check_clip_blocks(blocks, lengths):
    at = [0] * len(lengths)
    for i, blk in enumerate(blocks):
        n = blk["frames"]
        assert blk["start_frames"] == at and max(n) >= 1 and min(n) >= 0
        assert blk["audio"].shape == (len(lengths), 1, max(n) * HOP) and blk["sampled_indices"].shape == (len(lengths), 9, max(n))
        for b, n_b in enumerate(n):
            assert torch.equal(blk["sampled_indices"][b, 0, :n_b], torch.arange(at[b], at[b] + n_b)), (i, b)
            assert bool((blk["sampled_indices"][b, :, n_b:] == FakeModel.special_token_id).all())
        assert blk["final"] == (i + 1 == len(blocks))
        at = [a + k for a, k in zip(at, n)]
    assert at == lengths


@pytest.mark.parametrize("emit", [1, 3])
def test_clips_stream_follows_every_clips_own_schedule(emit):
    m = FakeModel()
    durations = [5.12, 2.0, 3.84]                                   # 5 chunks, the single-chunk branch, 3 chunks
    lengths = [441, 172, 331]
    frames = torch.zeros(3, 6, 8, 768)
    blocks = list(longform.generate_long_clips_stream(m, frames, durations, emit_chunks=emit, use_sampling=False))
    check_clip_blocks(blocks, lengths)
    assert len(m.calls) == 5 and m.audio_encoder.decodes == 0
    if emit == 1:
        # chunk 0: the single-chunk clip is out at once, whole; chunk 2 is the last of the 3.84 s clip; behind its end a clip has count 0
        assert [blk["frames"] for blk in blocks] == [[211, 172, 211], [55, 0, 55], [55, 0, 65], [55, 0, 0], [65, 0, 0]]
        w = m.audio_encoder.windows
        assert [x["counts"] for x in w] == [blk["frames"] for blk in blocks]
        # the stretch of tokens handed to the codec follows the windows: from the earliest halo to the latest known frame
        assert [x["T"] for x in w] == [221, 75, 75, 75, 75]
        assert w[2]["starts"] == [10, 0, 10] and w[2]["lengths"] == [75, 1, 75] and w[2]["first"] == [266, None, 266]
        assert w[3]["starts"] == [10, 0, 0] and w[3]["lengths"] == [75, 1, 1]
    else:
        assert [blk["frames"] for blk in blocks] == [[321, 172, 331], [120, 0, 0]]


def test_clips_stream_of_equal_durations_is_the_scalar_stream():
    m = FakeModel()
    blocks = list(longform.generate_long_clips_stream(m, FRAMES, [3.84, 3.84], use_sampling=False))
    check_clip_blocks(blocks, [331, 331])
    assert [blk["frames"] for blk in blocks] == [[211, 211], [55, 55], [65, 65]]
    assert all("start_frame" not in blk for blk in blocks)
