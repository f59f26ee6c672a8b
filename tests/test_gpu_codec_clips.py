"""Clips of different lengths in ONE codec pass, on the device: vaura_dac_decode_clips / vaura_dac_encode_clips (csrc/dac.hip),
CodecEngine.decode_clips / CodecEncoderEngine.encode_clips, and VAURAModel.generate / forward on top of them.

The contract is bit equality: clip b of the packed call is what decode() / encode() gives for the clip alone — every comparison is
torch.equal, nothing has a tolerance — and everything behind a clip is exactly 0.  Outputs of the direct library calls live inside an
allocation of 0xFF bytes whose guards must stay 0xFF, and the engine's four workspaces are filled with 0xFF before the call: a gap row
that is never cleared is a NaN (fp32, fp16 planes, e4m3; scale byte 255) that reaches the neighbouring clips' edges.

Shapes: the full-size synthetic codec; decode lengths [1, 7, 64, 33, 120] (241 packed frames: 482 256-row workgroups at the last
level, where no clip alone reaches the 384 that select the 256-row and one-launch instances) and [2, 1, 3] (14 packed frames: the
128-row and two-launch instances); encode sample lengths [511, 513, 20000, 4096, 1]."""
import ctypes as C
import math
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from vaura_amd import _lib as L
from vaura_amd import synth
from vaura_amd.codec_clips import clip_layout
from vaura_amd.engine import CodecEncoderEngine, CodecEngine

DEV = "cuda:0"
CFG = synth.FULL_CODEC
PRECISIONS = ["f32", "f16pair", "f16", "f16pair_w8", "mx8"]
# launch_conv / launch_conv_unit have 256-row and one-launch instances for the fp16-plane precisions only: conv_mfma_kernel (f32) and
# conv_mx8_kernel (every mx8 layer but conv_in, which is 1 workgroup tall here) have one instance each
BIG_INSTANCES = {"f16pair", "f16", "f16pair_w8"}
BIG, SMALL = [1, 7, 64, 33, 120], [2, 1, 3]
SAMPLES = [511, 513, 20000, 4096, 1]


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
    d = dict(synth.codec_state_dict(CFG, seed=0))
    d.update(synth.codec_encoder_state_dict(CFG, seed=0))
    return d


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


def check_decode(eng, lengths, seed):
    """-> (counters of the clips decoded alone, counters of the packed call)"""
    B, T, hop = len(lengths), max(lengths), CFG.hop
    codes = padded_codes(lengths, seed)
    counters()
    alone = [eng.decode(codes[b:b + 1, :, :n]).clone() for b, n in enumerate(lengths)]
    c_alone = counters()
    got = eng.decode_clips(codes, lengths).clone()                  # also sizes the workspaces for the packed sequence
    counters()
    poison(eng)
    out = Guarded(B * T * hop * 4)
    ci = codes.to(torch.int32).contiguous()
    rc = eng.lib.vaura_dac_decode_clips(C.byref(eng.c), L.ptr(ci), B, T, (C.c_int32 * B)(*lengths), L.ptr(out.view(torch.float32)),
                                        L.current_stream(torch.device(DEV)))
    assert rc == 0
    c_packed = counters()
    torch.cuda.synchronize()
    out.check()
    wav = out.view(torch.float32).reshape(B, 1, T * hop)
    assert bool(torch.isfinite(wav).all()), "a 0xFF byte of the workspace reached the output"
    for b, n in enumerate(lengths):
        assert alone[b].shape == (1, 1, n * hop)
        d = float((wav[b:b + 1, :, :n * hop] - alone[b]).abs().max())
        print(f"clip {b}: T_b = {n}: max |packed - alone| = {d:.3e}")
        assert torch.equal(wav[b:b + 1, :, :n * hop], alone[b]), (b, n, d)
        assert bool((wav[b, :, n * hop:] == 0).all()), (b, n)
    assert torch.equal(got, wav)                                     # the engine method is that call
    return c_alone, c_packed


@pytest.mark.parametrize("precision", PRECISIONS)
def test_decode_clips_is_each_clip_decoded_alone(engines, precision):
    c_alone, c_packed = check_decode(engines(precision), BIG, 1)
    print(f"{precision}: 256-row launches / one-launch units: alone {c_alone}, packed {c_packed}")
    assert c_alone == (0, 0)                                         # no clip alone is tall enough for either
    if precision in BIG_INSTANCES:
        assert c_packed[0] > 0 and c_packed[1] > 0
    else:
        assert c_packed == (0, 0)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_decode_clips_small_case_runs_the_small_instances(engines, precision):
    c_alone, c_packed = check_decode(engines(precision), SMALL, 2)
    assert c_alone == (0, 0) and c_packed == (0, 0)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_decode_clips_degenerate_batches(engines, precision):
    eng = engines(precision)
    codes = padded_codes([9, 9, 9], 3)
    plain = eng.decode(codes).clone()
    assert torch.equal(eng.decode_clips(codes, [9, 9, 9]), plain)
    assert torch.equal(eng.decode_clips(codes[1:2], [9]), plain[1:2])
    with pytest.raises(L.VauraHipError, match="must lie in 1 .. 9"):
        eng.decode_clips(codes, [9, 10, 1])
    with pytest.raises(L.VauraHipError, match="2 values for a batch of 3"):
        eng.decode_clips(codes, [9, 1])


def test_encode_clips_is_each_clip_encoded_alone(sd):
    enc = CodecEncoderEngine(CFG, sd, DEV)
    hop = math.prod(CFG.encoder_rates)
    B, N = len(SAMPLES), max(SAMPLES)
    T = -(-N // hop)
    wav = (torch.randn(B, 1, N, generator=torch.Generator().manual_seed(4)) * 0.3).to(DEV)        # random behind a clip too
    alone = [enc.encode(wav[b:b + 1, :, :n]).clone() for b, n in enumerate(SAMPLES)]
    got = enc.encode_clips(wav, SAMPLES).clone()
    assert got.shape == (B, CFG.n_codebooks, T) and got.dtype == torch.int64
    poison(enc)
    out = Guarded(B * CFG.n_codebooks * T * 4)
    x = wav[:, 0].contiguous()
    rc = enc.lib.vaura_dac_encode_clips(C.byref(enc.c), L.ptr(x), B, N, (C.c_int64 * B)(*SAMPLES), L.ptr(out.view(torch.int32)),
                                        L.current_stream(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    out.check()
    codes = out.view(torch.int32).reshape(B, CFG.n_codebooks, T).to(torch.int64)
    frames = clip_layout(SAMPLES, CFG, "encode").frames
    for b, n in enumerate(SAMPLES):
        f = -(-n // hop)
        assert f == frames[b] and alone[b].shape == (1, CFG.n_codebooks, f)
        print(f"clip {b}: n_b = {n}: {int((codes[b:b + 1, :, :f] != alone[b]).sum())} of {alone[b].numel()} codes differ from the clip alone")
        assert torch.equal(codes[b:b + 1, :, :f], alone[b]), (b, n)
        assert bool((codes[b, :, f:] == 0).all()), (b, n)
    assert torch.equal(got, codes)
    with pytest.raises(L.VauraHipError, match="must lie in 1 .. 20000"):
        enc.encode_clips(wav, [511, 513, 20001, 4096, 1])


# ---------------------------------------------------------------------------------------------------------------- plugin surface
@pytest.fixture(scope="module")
def model(tiny_sampler_sd):
    from vaura_amd.model import VAURAModel
    cfg = synth.tiny_sampler(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VAURAModel(
            feature_extractor_config={"target": "vaura_amd.feature_extractor.MotionFormer"},
            audio_encoder_config={"target": "vaura_amd.codec.DacModelWrapper", "params": {"model_sr": 44100, "synthetic": True}},
            sampler_config={"target": "vaura_amd.sampler.Transformer", "params": cfg.yaml_params()},
            visual_bridge_config={"target": "torch.nn.Identity"},
            pattern_provider_config={"target": "vaura_amd.patterns.DelayedPatternProvider", "params": {"n_q": 9}},
            flatten_vis_feats=True, freeze_feature_extractor=True)
    m.sampler.load_state_dict(tiny_sampler_sd, strict=True)
    m.sampler.audio_tokens_per_video_frame = 7
    return m.to(DEV)


def grouped_decode(model, tok, row_len):
    """The route generate() took before decode_clips: decode() once per distinct length on the rows of that length."""
    K, hop = model.num_codebooks, CFG.hop
    wav = torch.zeros(tok.shape[0], 1, tok.shape[-1] * hop, device=tok.device)
    for Tb in sorted(set(row_len)):
        idx = torch.tensor([i for i, n in enumerate(row_len) if n == Tb], device=tok.device)
        wav[idx, :, :Tb * hop] = model.audio_encoder.decode([(tok[idx][..., :K, :Tb], None)])
    return wav


def test_generate_with_lengths_is_the_grouped_route(model):
    B, T, TV = 4, [12, 5, 1, 9], 32
    frames = synth.video_features(B, tokens=TV, seed=31).reshape(B, 1, TV, 768).to(DEV)
    kw = dict(frames=frames, prompt_is_encoded=True, top_k=250, cfg_scale=3.0, return_sampled_indices=True)
    r = model.generate(max_new_tokens=T, **kw)
    assert set(r) == {"generated_audio", "s_attn_weights", "mha_attn_weights", "sampled_indices", "lengths", "audio_lengths"}
    assert r["generated_audio"].shape == (B, 1, 12 * CFG.hop) and torch.equal(r["audio_lengths"].cpu(), torch.tensor(T) * CFG.hop)
    assert torch.equal(r["generated_audio"], grouped_decode(model, r["sampled_indices"], T))
    r = model.generate(max_new_tokens=T, num_candidates=2, return_all_candidates=True, return_logprobs=True, use_sampling=True, **kw)
    rows = [n for n in T for _ in range(2)]
    assert r["generated_audio"].shape[0] == 2 * B
    assert torch.equal(r["generated_audio"], grouped_decode(model, r["sampled_indices"], rows))
    r = model.generate(max_new_tokens=12, **kw)                       # an int: the call it always was
    assert set(r) == {"generated_audio", "s_attn_weights", "mha_attn_weights", "sampled_indices"}
    assert torch.equal(r["generated_audio"], model.audio_encoder.decode([(r["sampled_indices"], None)]))


def test_forward_with_audio_lengths_is_the_grouped_encode(model):
    B = 3
    frames = synth.video_features(B, seed=5).reshape(B, 4, 8, 768).to(DEV)
    wav = (torch.randn(B, 1, 20 * 512, generator=torch.Generator().manual_seed(123)) * 0.3).to(DEV)
    n = [20 * 512, 11 * 512 + 100, 11 * 512 + 100]
    # the grouped route: one encode per distinct length, each group cut to its own samples
    want = torch.zeros(B, 9, 20, dtype=torch.int64, device=DEV)
    Ta = [0] * B
    for n_b in sorted(set(n)):
        idx = [b for b, v in enumerate(n) if v == n_b]
        c = model.audio_encoder.encode(wav[idx][..., :n_b])
        want[idx, :, :c.shape[-1]] = c
        for b in idx:
            Ta[b] = int(c.shape[-1])
    logits, mask, aud = model.forward(frames, wav, audio_lengths=n)
    assert Ta == [20, 12, 12] and torch.equal(aud, want)
    vis = model._handle_visual_conditioning(frames)
    direct = model.sampler.engine().score_clips(want[:, :9], vis, Ta, tokens_per_frame=7, return_logits=True)
    assert torch.equal(mask, direct["mask"]) and torch.equal(logits[mask], direct["logits"][mask])
    batch = {"audio": wav, "frames": frames, "meta": {}, "audio_lengths": n}
    assert torch.equal(model.test_step(batch, 0), direct["loss"])
    lg, mk, plain = model.forward(frames, wav)                        # without lengths: one encode of the whole batch
    assert torch.equal(plain, model.audio_encoder.encode(wav)) and bool(mk.all())
