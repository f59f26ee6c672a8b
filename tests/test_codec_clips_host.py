"""Clips of different lengths in one codec pass, host side: the layout function (codec_clips.clip_layout) and its gap rule against the
library's own (vaura_dac_clips_gap / vaura_dac_encode_clips_gap, from the conv descriptors), the gap argument itself in fp64 on the CPU
(tests/codec_clips_reference.py against oracle.dac_oracle of each clip alone), what the two C entry points refuse before any launch,
and where VAURAModel routes a call with and without per-clip lengths."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import codec_clips_reference as R  # noqa: E402
from oracle import dac_oracle  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import synth  # noqa: E402
from vaura_amd.codec_clips import clip_layout, decode_gap, encode_gap  # noqa: E402

BAR = 2.0 ** -40        # x max |reference|: fp64 rounding through ~45 layers of sums of <= 10 752 terms is orders below, a leaked halo row is of the order of the signal
OTHER = [synth.CodecCfg(dilations=(1, 3, 27)), synth.CodecCfg(decoder_rates=(2, 2, 4, 32), encoder_rates=(32, 4, 2, 2)),
         synth.CodecCfg(dilations=(1, 1, 1))]


# ---------------------------------------------------------------------------------------------------------------- layout
def gap_by_rule(cfg, side):
    """The rule, written out level by level: (rows per latent frame, one-sided reach of a conv that runs there)."""
    levels = []
    if side == "decode":
        rate = 1
        levels.append((rate, 3))                                   # conv_in, k = 7
        for r in cfg.decoder_rates:
            levels.append((rate, 1))                               # transposed conv: rows j, j - 1 of its input
            rate *= r
            levels += [(rate, 3 * d) for d in cfg.dilations]       # k = 7, dilation d
        levels.append((rate, 3))                                   # conv_out, k = 7
    else:
        rate = math.prod(cfg.encoder_rates)
        levels.append((rate, 3))
        for r in cfg.encoder_rates:
            levels += [(rate, 3 * d) for d in cfg.dilations]
            rate //= r
            levels.append((rate, 1))                               # strided conv: one row of r * C channels = one row of its output level
        levels.append((rate, 1))                                   # conv_out, k = 3
    g = 1
    while any(g * rate < reach for rate, reach in levels):
        g += 1
    return g


def descriptors(cfg):
    """The two library descriptors with the geometry only (no device pointer is read by the gap queries)."""
    def conv(cv, taps, dilation=1, stride=1):
        cv.taps, cv.dilation, cv.stride = taps, dilation, stride
    d = L.Codec()
    d.n_blocks, d.n_units = len(cfg.decoder_rates), 3
    conv(d.conv_in, 7)
    conv(d.conv_out, 7)
    e = L.CodecEncoder()
    e.n_blocks, e.n_units = len(cfg.encoder_rates), 3
    conv(e.conv_out, 3)
    for b in range(4):
        d.rates[b], e.rates[b] = cfg.decoder_rates[b], cfg.encoder_rates[b]
        conv(d.up[b], 2, 1, cfg.decoder_rates[b])
        conv(e.down[b], 3)
        for u, dil in enumerate(cfg.dilations):
            for x in (d, e):
                conv(x.res[b][u][0], 7, dil)
                conv(x.res[b][u][1], 1)
    return d, e


def test_gap_follows_the_rule_in_python_and_in_the_library():
    assert decode_gap(synth.FULL_CODEC) == 4 and encode_gap(synth.FULL_CODEC) == 4          # 27 rows at 8 rows per frame
    assert decode_gap(synth.tiny_codec()) == 4 and encode_gap(synth.tiny_codec()) == 4
    seen = set()
    for cfg in [synth.FULL_CODEC, synth.tiny_codec()] + OTHER:
        d, e = descriptors(cfg)
        for side, py, lib in (("decode", decode_gap(cfg), L.lib().vaura_dac_clips_gap(C.byref(d))),
                              ("encode", encode_gap(cfg), L.lib().vaura_dac_encode_clips_gap(C.byref(e)))):
            assert py == lib == gap_by_rule(cfg, side), (cfg, side, py, lib)
            seen.add(py)
    assert decode_gap(OTHER[0]) == 11 and encode_gap(OTHER[0]) == 11                        # 81 rows at 8 rows per frame
    assert decode_gap(OTHER[1]) == 14 and decode_gap(OTHER[2]) == 3                         # 27 rows at 2 per frame; conv_in's 3 rows
    assert len(seen) > 2, "a hard-coded gap would pass"
    assert L.lib().vaura_dac_clips_gap(None) == -1 and L.lib().vaura_dac_encode_clips_gap(None) == -1


@pytest.mark.parametrize("cfg", [synth.FULL_CODEC] + OTHER)
def test_layout(cfg):
    lens = [1, 7, 64, 33, 120]
    lay = clip_layout(lens, cfg, "decode")
    assert lay.frames == tuple(lens) and lay.gap == decode_gap(cfg) and lay.hop == cfg.hop
    assert all(b > a for a, b in zip(lay.offsets, lay.offsets[1:]))
    assert all(o1 - (o0 + f0) >= lay.gap for o0, f0, o1 in zip(lay.offsets, lay.frames, lay.offsets[1:]))
    assert lay.offsets[0] == 0 and lay.total == lay.offsets[-1] + lens[-1] == sum(lens) + 4 * lay.gap
    n = [511, 513, 20000, 4096, 1]
    hop = math.prod(cfg.encoder_rates)
    enc = clip_layout(n, cfg, "encode")
    assert enc.hop == hop and enc.frames == tuple(-(-x // hop) for x in n) and enc.gap == encode_gap(cfg)
    assert all(o1 - (o0 + f0) >= enc.gap for o0, f0, o1 in zip(enc.offsets, enc.frames, enc.offsets[1:]))
    # a clip's first sample is a whole number of frames into the packed waveform: the strided convs keep their r-row view
    assert all((o * hop) % hop == 0 and o * hop + x <= (o + f) * hop for o, f, x in zip(enc.offsets, enc.frames, n))
    # the library sizes its workspaces for the same sequence
    d, e = descriptors(cfg)
    d.latent_dim, d.conv_in.cout, d.n_codebooks = 8, 16, 9
    for b in range(4):
        d.up[b].cout = 16 >> (b + 1)
    one = L.lib().vaura_dac_workspace_elems(C.byref(d), 1, lay.total)
    assert L.lib().vaura_dac_decode_clips_workspace_elems(C.byref(d), 5, (C.c_int32 * 5)(*lens)) == max(one, 9 * lay.total) > 0
    e.enc_dim, e.latent_dim, e.n_codebooks = 32, 8, 9
    one = L.lib().vaura_dac_encode_workspace_elems(C.byref(e), 1, enc.total * hop)
    assert L.lib().vaura_dac_encode_clips_workspace_elems(C.byref(e), 5, (C.c_int64 * 5)(*n)) == one > 0


@pytest.mark.parametrize("bad", [[], [3, 0], [3, -1], [3, 2.0], [True, 2]])
def test_layout_refuses(bad):
    with pytest.raises(ValueError):
        clip_layout(bad, synth.FULL_CODEC)


# ---------------------------------------------------------------------------------------------------------------- the gap argument, fp64
@pytest.fixture(scope="module")
def tiny():
    cfg = synth.tiny_codec()
    sd = dict(synth.codec_state_dict(cfg, seed=0))
    sd.update(synth.codec_encoder_state_dict(cfg, seed=0))
    return cfg, R.f64_state_dict(sd)


def test_packed_decode_is_the_clip_alone_and_gap_zero_is_not(tiny):
    cfg, sd = tiny
    g = torch.Generator().manual_seed(7)
    codes = [torch.randint(0, cfg.codebook_size, (cfg.n_codebooks, t), generator=g) for t in (1, 3, 2)]
    alone = [dac_oracle.decode(sd, c[None], cfg.decoder_rates)[0, 0] for c in codes]
    assert all(a.dtype == torch.float64 for a in alone)
    scale = max(float(a.abs().max()) for a in alone)
    worst = {}
    for gap in (decode_gap(cfg), 0):
        got = R.packed_decode(sd, codes, cfg.decoder_rates, cfg.dilations, gap)
        worst[gap] = max(float((a - b).abs().max()) for a, b in zip(got, alone))
        print(f"decode, gap {gap}: max |packed - alone| = {worst[gap]:.3e}  (bar {BAR * scale:.3e}, max |wav| {scale:.3e})")
    assert worst[decode_gap(cfg)] <= BAR * scale
    assert worst[0] > BAR * scale, "the test does not see a leak"


def test_packed_encode_is_the_clip_alone_and_gap_zero_is_not(tiny):
    cfg, sd = tiny
    hop = math.prod(cfg.encoder_rates)
    g = torch.Generator().manual_seed(11)
    wavs = [torch.randn(n, generator=g, dtype=torch.float64) * 0.3 for n in (hop + 1, 3 * hop - 5, 700)]
    alone = [dac_oracle.encode_latent(sd, dac_oracle.preprocess(w[None, None], hop), cfg.encoder_rates)[0] for w in wavs]
    assert all(a.dtype == torch.float64 for a in alone) and [a.shape[-1] for a in alone] == [2, 3, 2]
    scale = max(float(a.abs().max()) for a in alone)
    worst, lat = {}, {}
    for gap in (encode_gap(cfg), 0):
        lat[gap] = R.packed_encode_latent(sd, wavs, cfg.encoder_rates, cfg.dilations, gap)
        worst[gap] = max(float((a - b).abs().max()) for a, b in zip(lat[gap], alone))
        print(f"encode, gap {gap}: max |packed latent - alone| = {worst[gap]:.3e}  (bar {BAR * scale:.3e}, max |z| {scale:.3e})")
    assert worst[encode_gap(cfg)] <= BAR * scale
    assert worst[0] > BAR * scale, "the test does not see a leak"
    # the codes: equal wherever the oracle's own best and second-best codeword are not a near-tie.  The scores are O(1) sums in fp64 and
    # the latents agree to 2^-40 relative: a margin above 1e-9 cannot flip.
    skipped = 0
    for a, b in zip(lat[encode_gap(cfg)], alone):
        want, margin = dac_oracle.quantize(sd, b[None], cfg.n_codebooks, return_margin=True)
        got = dac_oracle.quantize(sd, a[None], cfg.n_codebooks)
        safe = (margin > 1e-9).all(dim=1)[0]                      # a frame counts only if every stage of it is clear (stages feed each other)
        skipped += int((~safe).sum())
        assert torch.equal(got[..., safe], want[..., safe])
    print(f"frames skipped as near-ties: {skipped}")
    assert skipped <= 0


# ---------------------------------------------------------------------------------------------------------------- C entry points
def test_entry_points_refuse_before_any_launch():
    lib = L.lib()
    one = C.c_void_p(16)                                            # points nowhere: nothing may be dereferenced
    d, e = descriptors(synth.FULL_CODEC)
    d.n_codebooks = e.n_codebooks = 9
    d.codebook_dim = e.codebook_dim = 8
    d.latent_dim = e.latent_dim = 1024
    d.conv_in.cout, e.enc_dim, e.codebook_size = 1536, 64, 1024
    for b in range(4):
        d.up[b].cout = 1536 >> (b + 1)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    i64 = lambda *v: (C.c_int64 * len(v))(*v)
    ok, okn = i32(5, 3), i64(700, 1300)
    # NULL pointers, the length array among them
    assert lib.vaura_dac_decode_clips(None, one, 2, 8, ok, one, None) == -1
    assert lib.vaura_dac_decode_clips(C.byref(d), None, 2, 8, ok, one, None) == -1
    assert lib.vaura_dac_decode_clips(C.byref(d), one, 2, 8, None, one, None) == -1
    assert lib.vaura_dac_decode_clips(C.byref(d), one, 2, 8, ok, None, None) == -1
    assert lib.vaura_dac_encode_clips(None, one, 2, 2048, okn, one, None) == -1
    assert lib.vaura_dac_encode_clips(C.byref(e), None, 2, 2048, okn, one, None) == -1
    assert lib.vaura_dac_encode_clips(C.byref(e), one, 2, 2048, None, one, None) == -1
    assert lib.vaura_dac_encode_clips(C.byref(e), one, 2, 2048, okn, None, None) == -1
    assert lib.vaura_dac_decode_clips_workspace_elems(C.byref(d), 2, None) == 0
    assert lib.vaura_dac_encode_clips_workspace_elems(C.byref(e), 2, None) == 0
    # lengths outside 1 .. T_max / 1 .. n_max (the workspaces are NULL and too small as well: still no launch, still VAURA_ERR_ARG)
    for bad in (i32(5, 0), i32(5, 9), i32(-1, 3)):
        assert lib.vaura_dac_decode_clips(C.byref(d), one, 2, 8, bad, one, None) == -1
    assert lib.vaura_dac_decode_clips_workspace_elems(C.byref(d), 2, i32(5, 0)) == 0
    for bad in (i64(700, 0), i64(700, 2049), i64(-5, 3)):
        assert lib.vaura_dac_encode_clips(C.byref(e), one, 2, 2048, bad, one, None) == -1
    assert lib.vaura_dac_encode_clips_workspace_elems(C.byref(e), 2, i64(700, 0)) == 0
    # good lengths, no workspace: refused for the workspace
    need = lib.vaura_dac_decode_clips_workspace_elems(C.byref(d), 2, ok)
    assert need == (5 + 4 + 3) * 512 * 96 and lib.vaura_dac_decode_clips(C.byref(d), one, 2, 8, ok, one, None) == -1
    d.ws_elems = need                                               # large enough, but the four pointers are NULL
    assert lib.vaura_dac_decode_clips(C.byref(d), one, 2, 8, ok, one, None) == -1
    need = lib.vaura_dac_encode_clips_workspace_elems(C.byref(e), 2, okn)
    assert need == (2 + 4 + 3) * 512 * 64 and lib.vaura_dac_encode_clips(C.byref(e), one, 2, 2048, okn, one, None) == -1
    # a packed sequence whose widest level (rows x channels) leaves the int range: VAURA_ERR_SHAPE, whatever the workspace
    big = i32(30000, 30000)                                         # 60 004 frames x 512 x 96 > 2^31
    d.ws_elems = 2 ** 62
    assert lib.vaura_dac_decode_clips(C.byref(d), one, 2, 30000, big, one, None) == -2
    assert lib.vaura_dac_decode_clips_workspace_elems(C.byref(d), 2, big) > 2 ** 31
    bign = i64(30000 * 512, 45000 * 512)                            # 75 004 frames x 512 x 64 > 2^31
    e.ws_elems = 2 ** 62
    assert lib.vaura_dac_encode_clips(C.byref(e), one, 2, 45000 * 512, bign, one, None) == -2


# ---------------------------------------------------------------------------------------------------------------- routing
@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    from ckpt_fixture import write_checkpoint
    from vaura_amd.model import VAURAModel
    d = tmp_path_factory.mktemp("ckpt_codec_clips")
    ckpt, hp, _ = write_checkpoint(str(d), synth.tiny_sampler(2))
    return VAURAModel.load_from_checkpoint(ckpt, hparams_file=hp, map_location="cpu")


class Calls:
    def __init__(self, m, monkeypatch, tokens):
        self.decode, self.decode_clips, self.encode, self.encode_clips = [], [], [], []
        monkeypatch.setattr(m, "_generate_tokens", lambda *a, **kw: tokens)      # what generate() runs behind its host stage
        monkeypatch.setattr(m.sampler, "engine", lambda: type("E", (), {"dev": torch.device("cpu")})())
        monkeypatch.setattr(m.audio_encoder, "decode", lambda codes: self.decode.append(codes) or torch.zeros(codes[0][0].shape[0], 1, 512 * codes[0][0].shape[-1]))
        monkeypatch.setattr(m.audio_encoder, "decode_clips",
                            lambda codes, lengths: self.decode_clips.append((codes, lengths)) or torch.zeros(codes.shape[0], 1, 512 * codes.shape[-1]))
        monkeypatch.setattr(m.audio_encoder, "encode", lambda wav: self.encode.append(wav) or torch.zeros(wav.shape[0], 9, -(-wav.shape[-1] // 512), dtype=torch.int64))
        monkeypatch.setattr(m.audio_encoder, "encode_clips",
                            lambda wav, n: self.encode_clips.append((wav, n)) or torch.zeros(wav.shape[0], 9, -(-wav.shape[-1] // 512), dtype=torch.int64))


def test_generate_routes_lengths_to_one_decode_clips_call(cpu_model, monkeypatch):
    import vaura_amd.model as M
    import contextlib
    monkeypatch.setattr(M, "off_null_stream", lambda dev: contextlib.nullcontext(None))
    frames = torch.zeros(3, 1, 32, 768)
    tok = torch.zeros(3, 9, 12, dtype=torch.int64)
    calls = Calls(cpu_model, monkeypatch, tok)
    r = cpu_model.generate(frames=frames, prompt_is_encoded=True, max_new_tokens=12)
    assert len(calls.decode) == 1 and not calls.decode_clips and set(r) == {"generated_audio", "s_attn_weights", "mha_attn_weights", "sampled_indices"}
    calls = Calls(cpu_model, monkeypatch, {"tokens": tok, "lengths": torch.tensor([12, 5, 9])})
    r = cpu_model.generate(frames=frames, prompt_is_encoded=True, max_new_tokens=[12, 5, 9])
    assert not calls.decode and len(calls.decode_clips) == 1 and calls.decode_clips[0][1] == [12, 5, 9]
    assert r["generated_audio"].shape == (3, 1, 12 * 512) and r["audio_lengths"].tolist() == [12 * 512, 5 * 512, 9 * 512]
    # one length for every clip: the plain batched decode (the same bits without the packing), zero-padded to the call's width
    calls = Calls(cpu_model, monkeypatch, {"tokens": tok, "lengths": torch.tensor([7, 7, 7])})
    r = cpu_model.generate(frames=frames, prompt_is_encoded=True, max_new_tokens=12, video_lengths=[3, 2, 1])
    assert len(calls.decode) == 1 and not calls.decode_clips and calls.decode[0][0][0].shape == (3, 9, 7)
    assert r["generated_audio"].shape == (3, 1, 12 * 512) and r["audio_lengths"].tolist() == [7 * 512] * 3
    # every take of a clip has the clip's length (return_all_candidates: B * N rows)
    calls = Calls(cpu_model, monkeypatch, {"tokens": tok.repeat_interleave(2, 0), "lengths": torch.tensor([12, 5, 9])})
    cpu_model.generate(frames=frames, prompt_is_encoded=True, max_new_tokens=[12, 5, 9], use_sampling=True, num_candidates=2,
                       return_all_candidates=True, return_logprobs=True)
    assert not calls.decode and len(calls.decode_clips) == 1 and calls.decode_clips[0][1] == [12, 12, 5, 5, 9, 9]


def test_encode_routes_lengths_to_one_encode_clips_call(cpu_model, monkeypatch):
    calls = Calls(cpu_model, monkeypatch, None)
    wav = torch.zeros(3, 1, 3000)
    codes, lengths = cpu_model._encode_clips(wav)
    assert len(calls.encode) == 1 and not calls.encode_clips and lengths is None
    calls = Calls(cpu_model, monkeypatch, None)
    codes, lengths = cpu_model._encode_clips(wav, [511, 2049, 1024])
    assert not calls.encode and len(calls.encode_clips) == 1 and calls.encode_clips[0][1] == [511, 2049, 1024]
    assert lengths == [1, 5, 2] and codes.shape == (3, 9, 5) and calls.encode_clips[0][0].shape[-1] == 2049
    calls = Calls(cpu_model, monkeypatch, None)
    codes, lengths = cpu_model._encode_clips(wav, [1025, 1025, 1025])          # one length: the plain batched encode of the cut batch
    assert not calls.encode_clips and len(calls.encode) == 1 and calls.encode[0].shape == (3, 1, 1025) and lengths == [3, 3, 3]
