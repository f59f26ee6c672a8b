"""Attention maps of generate(), host side (no GPU): the vaura_decoder_ext4 layout and its refusals, the three new C entries' argument
checks, every call-time refusal of the keywords, their defaults, the routing of generate(return_attention_weights=True) on a stubbed
engine, the numpy restatement of attention_map_kernel's fixed-order mean, and the seed of the loop-level GPU test: the plumbing faults
it must tell apart are at least 1e-2 apart in the fp64 restatement (tests/attention_maps_reference.py)."""
import contextlib
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_maps_reference as AM  # noqa: E402
import test_relevance_host as RH  # noqa: E402  (its descriptor that passes the shape checks)
from oracle.decoder_oracle import DecoderOracle  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import clip_params, synth  # noqa: E402
from vaura_amd.engine import DecoderEngine  # noqa: E402

# the loop-level case of tests/test_gpu_attention_maps.py
LOOP_B, LOOP_T, LOOP_TV, LOOP_FEAT_SEED = 3, 20, 32, 31


# ---------------------------------------------------------------------------------------------------------------- struct layout
def test_ext4_follows_ext3_and_is_480_bytes():
    assert L.DecoderExt4.ext3.offset == 0 and C.sizeof(L.DecoderExt3) == 456
    assert [getattr(L.DecoderExt4, n).offset for n in ("attn_probs", "attn_layer", "attn_pos0", "attn_steps", "attn_rows")] == [456, 464, 468, 472, 476]
    assert C.sizeof(L.DecoderExt4) == 480 and C.sizeof(L.DecoderExt4) - C.sizeof(L.Decoder) == 64
    lib = L.lib()
    assert lib.vaura_struct_size(14) == 480 and lib.vaura_struct_size(13) == 456 and lib.vaura_struct_size(12) == 0
    x = L.DecoderExt4()
    assert x.ext3.ext2.ext.dec.ext_bytes == 0 and x.attn_probs is None and x.attn_rows == 0       # zero-filled: no maps
    assert C.addressof(x.ext3.ext2.ext.dec) == C.addressof(x)


def _ext4(rows=6, ext_bytes=64):
    x = L.DecoderExt4()
    src, _, keep = RH._descriptor(rows)
    C.memmove(C.addressof(x), C.addressof(src), C.sizeof(L.DecoderExt))
    d = x.ext3.ext2.ext.dec
    d.ext_bytes = ext_bytes
    return x, d, keep


@pytest.mark.parametrize("ext_bytes,rc", [(0, 0), (16, 0), (32, 0), (40, 0), (64, 0), (8, -1), (24, -1), (48, -1), (56, -1), (72, -1)])
def test_accepted_extension_sizes(ext_bytes, rc):
    """a loop of no positions launches nothing and dereferences nothing: it returns what the descriptor check says"""
    x, d, _keep = _ext4(6, ext_bytes)
    sp = L.Sampling(0, 1.0, 0, 0.0, 3.0, 0, 0, 0, 0.0)
    assert L.lib().vaura_generate_loop(C.byref(d), C.byref(sp), 0, 0, None, None) == rc


@pytest.mark.parametrize("fields,rc", [
    (dict(), 0), (dict(attn_layer=1, attn_rows=6), 0),
    (dict(attn_layer=-1), -1), (dict(attn_layer=2), -1), (dict(attn_rows=0), -1), (dict(attn_rows=7), -1), (dict(attn_steps=0), -1),
    (dict(attn_pos0=-1), -1), (dict(max_len=288), -2),
    (dict(attn_probs=0, attn_layer=9, attn_rows=-3, attn_steps=0, attn_pos0=-5), 0),                 # no buffer: nothing is read
], ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_descriptor_refusals(fields, rc):
    x, d, _keep = _ext4(6)
    x.attn_probs, x.attn_layer, x.attn_pos0, x.attn_steps, x.attn_rows = 16, 0, 0, 20, 3
    for k, v in fields.items():
        if k == "max_len":
            d.max_len = v
        else:
            setattr(x, k, v)
    sp = L.Sampling(0, 1.0, 0, 0.0, 3.0, 0, 0, 0, 0.0)
    assert L.lib().vaura_generate_loop(C.byref(d), C.byref(sp), 0, 0, None, None) == rc
    if rc:                                                                                           # ... and before any launch of a step
        assert L.lib().vaura_decode_step(C.byref(d), C.byref(sp), 1, None) == rc
        d.ext_bytes = 40                                                                             # the same bytes are then not the library's to read
        assert L.lib().vaura_generate_loop(C.byref(d), C.byref(sp), 0, 0, None, None) == 0


def test_new_entries_are_exported_and_refuse_their_arguments_without_a_launch():
    lib = L.lib()
    for name in ("vaura_attention_step_probs", "vaura_attention_map", "vaura_attention_step_kv"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    one = C.c_void_p(16)
    base = (one, None, one, one, one, None, None, one, None, None, None)                            # qkv .. arrivals
    ok = dict(rows=6, n_head=16, head_dim=96, max_len=256, pos=5, n_split=1, plane_shift=0, kv_dtype=0, probs=one, pos0=0, n_steps=4, rows_out=3)

    def call(ptrs=base, **kw):
        a = dict(ok, **kw)
        return lib.vaura_attention_step_probs(*ptrs, a["rows"], a["n_head"], a["head_dim"], a["max_len"], a["pos"], a["n_split"], a["plane_shift"],
                                              a["kv_dtype"], a["probs"], a["pos0"], a["n_steps"], a["rows_out"], None)
    for kw in (dict(probs=None), dict(pos0=-1), dict(n_steps=0), dict(rows_out=0), dict(rows_out=7), dict(pos=256), dict(pos=-1), dict(kv_dtype=4),
               dict(n_split=2), dict(kv_dtype=3)):                                                   # (a split without scratch; storage 3 without its bytes)
        assert call(**kw) == -1, kw
    for i in (0, 2, 3, 4, 7):                                                                        # qkv, rope, kcache, vcache, out
        assert call(base[:i] + (None,) + base[i + 1:]) == -1, i
    assert call(max_len=257, pos=5) == -2 and call(head_dim=64) == -2                                # VAURA_ERR_SHAPE, nothing launched
    assert call(base[:9] + (one,) + base[10:], n_split=2) == -2                                      # a range split (with its scratch)
    m = lib.vaura_attention_map
    assert m(None, one, 4, 3, 16, 256, 28, 0, None) == -1 and m(one, None, 4, 3, 16, 256, 28, 0, None) == -1
    for bad in ((0, 3, 16, 256, 28), (4, 0, 16, 256, 28), (4, 3, 0, 256, 28), (4, 3, 16, 0, 28), (4, 3, 16, 256, 0), (4, 3, 16, 256, 257)):
        assert m(one, one, *bad, 1, None) == -1, bad


# ------------------------------------------------------------------------------------------------------------- keywords
def test_keyword_defaults():
    from vaura_amd.model import VAURAModel
    p = inspect.signature(DecoderEngine.generate_codes).parameters
    assert (p["return_attention_weights"].default, p["attention_layer"].default, p["attention_heads"].default) == (False, -1, "mean")
    for fn, flag in ((VAURAModel.generate, None), (VAURAModel.generate_tokens, False)):            # generate(): None = the constructor's flag
        p = inspect.signature(fn).parameters
        assert (p["return_attention_weights"].default, p["attention_layer"].default, p["attention_heads"].default) == (flag, -1, "mean")
    call = clip_params.resolve_codes_call(3, 32, 20)
    assert (call.want_attention, call.attention_layer, call.attention_heads) == (False, -1, "mean")
    call = clip_params.resolve_codes_call(3, 32, 20, return_attention_weights=True, attention_layer=0, attention_heads="all", cfg_scale=3.0)
    assert (call.want_attention, call.attention_layer, call.attention_heads, call.cfg_on) == (True, 0, "all", True)
    assert clip_params.check_attention_keywords(-1, "mean", 24) == 23 and clip_params.check_attention_keywords(-24, "all", 24) == 0
    assert clip_params.attention_max_len(29, 256) == 256 and clip_params.attention_max_len(229, 64) == 256


@pytest.mark.parametrize("kw,match", [
    (dict(num_candidates=2, use_sampling=True), "num_candidates = 1"),
    (dict(max_new_tokens=[20, 12, 9]), "one length for the whole call"),
    (dict(prompt_lengths=[0, 2, 3], prompt_frames=4), "one length for the whole call"),
    (dict(attention_heads="max"), 'attention_heads must be "mean" or "all"'),
    (dict(attention_layer=1.0), "attention_layer must be an int"),
    (dict(attention_layer=True), "attention_layer must be an int"),
])
def test_resolve_codes_call_refusals(kw, match):
    kw = dict(kw)
    T, pf = kw.pop("max_new_tokens", 20), kw.pop("prompt_frames", None)
    with pytest.raises(L.VauraHipError, match=match):
        clip_params.resolve_codes_call(3, 32, T, pf, return_attention_weights=True, **kw)
    clip_params.resolve_codes_call(3, 32, T, pf, **{k: v for k, v in kw.items() if not k.startswith("attention_")})      # fine without the flag


def test_engine_refuses_layer_and_cache_length_before_any_device_work():
    eng = object.__new__(DecoderEngine)              # refused before anything of the engine but its configuration is read
    eng.cfg = synth.tiny_sampler(2)
    feats = torch.zeros(3, 32, 768)
    for layer in (2, -3, 24):
        with pytest.raises(L.VauraHipError, match="out of range for a decoder of 2 layers"):
            eng.generate_codes(feats, 20, return_attention_weights=True, attention_layer=layer)
    eng.cfg = synth.tiny_sampler(2, block_size_audio=512)
    with pytest.raises(L.VauraHipError, match="caches of at most 256 positions"):
        eng.generate_codes(feats, 20, return_attention_weights=True)
    eng.cfg = synth.tiny_sampler(2)
    with pytest.raises(L.VauraHipError, match="caches of at most 256 positions"):
        eng.generate_codes(feats, 250, return_attention_weights=True)                                # S = 259 > 256
    with pytest.raises(L.VauraHipError, match="generate_codes_stream does not return attention weights"):
        eng.generate_codes_stream(feats, 20, return_attention_weights=True)
    call = clip_params.resolve_codes_call(3, 32, 20, return_attention_weights=True)
    with pytest.raises(L.VauraHipError, match="a live sequence does not return attention weights"):
        eng.begin_live(call)


@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    from ckpt_fixture import write_checkpoint
    from vaura_amd.model import VAURAModel
    d = tmp_path_factory.mktemp("ckpt_attention_maps")
    ckpt, hp, _ = write_checkpoint(str(d), synth.tiny_sampler(2))
    return VAURAModel.load_from_checkpoint(ckpt, hparams_file=hp, map_location="cpu")


def _untouchable(m, monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work was started")
    monkeypatch.setattr(m, "_handle_visual_conditioning", touched)
    monkeypatch.setattr(m.sampler, "engine", touched)
    monkeypatch.setattr(m.audio_encoder, "decode", touched)


@pytest.mark.parametrize("kw,match", [
    (dict(num_candidates=2), "num_candidates = 1"),
    (dict(max_new_tokens=[12, 5, 9, 7]), "one length for the whole call"),
    (dict(audio=torch.zeros(4, 9, 3, dtype=torch.int64), prompt_lengths=[0, 1, 2, 3]), "one length for the whole call"),
    (dict(audio=torch.zeros(4, 1, 3000), prompt_is_encoded=False, audio_lengths=[600, 3000, 1200, 2000]), "one length for the whole call"),
    (dict(max_new_tokens=250), "caches of at most 256 positions"),
    (dict(attention_layer=2), "out of range for a decoder of 2 layers"),
    (dict(attention_heads="sum"), "attention_heads must be"),
])
@pytest.mark.parametrize("entry", ["generate", "generate_tokens"])
def test_model_refusals_before_any_device_work(cpu_model, monkeypatch, entry, kw, match):
    _untouchable(cpu_model, monkeypatch)
    kw = dict(dict(max_new_tokens=12, prompt_is_encoded=True), **kw)
    with pytest.raises(L.VauraHipError, match=match):
        getattr(cpu_model, entry)(frames=torch.zeros(4, 1, 32, 768), return_attention_weights=True, **kw)


def test_block_size_above_256_is_refused(cpu_model, monkeypatch):
    _untouchable(cpu_model, monkeypatch)
    monkeypatch.setattr(cpu_model.sampler, "block_size", 512, raising=False)
    with pytest.raises(L.VauraHipError, match="block_size <= 256"):
        cpu_model.generate_tokens(frames=torch.zeros(4, 1, 32, 768), prompt_is_encoded=True, max_new_tokens=12, return_attention_weights=True)


def test_streams_live_and_long_form_refuse_the_flag(cpu_model, monkeypatch):
    from vaura_amd import longform
    _untouchable(cpu_model, monkeypatch)
    frames = torch.zeros(2, 4, 2, 768)
    with pytest.raises(L.VauraHipError, match="generate_stream does not return attention weights"):
        cpu_model.generate_stream(frames=frames, max_new_tokens=12, return_attention_weights=True)
    with pytest.raises(L.VauraHipError, match="a live session does not return attention weights"):
        cpu_model.open_live(2, return_attention_weights=True)
    for fn, args in ((longform.generate_long, (2.56,)), (longform.generate_long_stream, (2.56,)), (longform.generate_long_clips, ([2.56, 1.3],)),
                     (longform.generate_long_clips_stream, ([2.56, 1.3],))):
        with pytest.raises(L.VauraHipError, match=f"{fn.__name__} does not return attention weights"):
            fn(cpu_model, frames, *args, return_attention_weights=True)


class _StubEngine:
    """generate_codes_checked of an engine that samples nothing: zero tokens, and for a call that asks for them maps of the stated shape"""
    dev = torch.device("cpu")

    def __init__(self, K):
        self.K, self.calls = K, []

    def generate_codes_checked(self, feats, T, **kw):
        self.calls.append(kw)
        B = feats.shape[0]
        codes = torch.zeros(B, self.K, T, dtype=torch.int64)
        if not kw.get("return_attention_weights"):
            return codes
        d = kw["delays"] if kw["delays"] is not None else list(range(self.K))
        S = T + max(d) + 1
        start = (kw["prompt"].shape[-1] if kw["prompt"] is not None else 0) + 1 + d[0]
        shape = (B, 16, S - start, S - 1) if kw["attention_heads"] == "all" else (B, S - start, S - 1)
        return codes, {"attention": torch.full(shape, 0.25)}


def test_generate_returns_the_map_on_a_stubbed_engine(cpu_model, monkeypatch):
    """MUST FAIL ON THE PARENT: generate(return_attention_weights=True) raised NotImplementedError there."""
    import vaura_amd.model as M
    monkeypatch.setattr(M, "off_null_stream", lambda dev: contextlib.nullcontext(None))
    eng = _StubEngine(cpu_model.num_codebooks)
    monkeypatch.setattr(cpu_model.sampler, "engine", lambda: eng)
    monkeypatch.setattr(cpu_model.sampler, "audio_tokens_per_video_frame", 7)
    monkeypatch.setattr(cpu_model, "_handle_visual_conditioning", lambda frames, *a, **k: frames[:, 0])
    monkeypatch.setattr(cpu_model.audio_encoder, "decode", lambda codes: torch.zeros(codes[0][0].shape[0], 1, 512 * codes[0][0].shape[-1]))
    frames = torch.zeros(3, 1, 32, 768)
    K, T = cpu_model.num_codebooks, 20
    S = T + K
    r = cpu_model.generate(frames=frames, max_new_tokens=T, return_attention_weights=True, use_sampling=False)
    assert set(r) == {"generated_audio", "s_attn_weights", "mha_attn_weights", "sampled_indices"}
    assert r["s_attn_weights"].shape == (3, S - 1, S - 1) and r["s_attn_weights"].dtype == torch.float32 and r["mha_attn_weights"] is None
    assert eng.calls[-1]["return_attention_weights"] is True and eng.calls[-1]["attention_layer"] == 1 and eng.calls[-1]["attention_heads"] == "mean"
    prompt = torch.zeros(3, K, 5, dtype=torch.int64)
    r = cpu_model.generate(frames=frames, audio=prompt, prompt_is_encoded=True, max_new_tokens=T, return_attention_weights=True, attention_heads="all",
                           attention_layer=0, use_sampling=False, remove_prompts=True, return_sampled_indices=True)
    assert r["s_attn_weights"].shape == (3, 16, S - 6, S - 1) and r["sampled_indices"].shape == (3, K, T - 5)       # the map is not cut
    assert eng.calls[-1]["attention_layer"] == 0
    t = cpu_model.generate_tokens(frames=frames, max_new_tokens=T, return_attention_weights=True, use_sampling=False)
    assert set(t) == {"tokens", "s_attn_weights"} and t["s_attn_weights"].shape == (3, S - 1, S - 1)
    # without the flag: the call it always was, no new keyword reaches the engine
    r = cpu_model.generate(frames=frames, max_new_tokens=T, use_sampling=False)
    assert r["s_attn_weights"] is None and not any(k.startswith(("attention_", "return_attention")) for k in eng.calls[-1])
    # the constructor's flag is the default of generate()'s keyword, and the keyword overrides it
    monkeypatch.setattr(cpu_model, "return_attention_weights", True)
    assert cpu_model.generate(frames=frames, max_new_tokens=T, use_sampling=False)["s_attn_weights"].shape == (3, S - 1, S - 1)
    assert cpu_model.generate(frames=frames, max_new_tokens=T, use_sampling=False, return_attention_weights=False)["s_attn_weights"] is None


# ------------------------------------------------------------------------------------------------- attention_map_kernel, restated
def test_fixed_order_mean_restatement():
    rng = np.random.default_rng(5)
    p = rng.random((5, 3, 16, 64), dtype=np.float32)
    p[2, 1, :, 40:] = 0.0
    mean, allh = AM.attention_map_np(p, 37), AM.attention_map_np(p, 37, "all")
    assert mean.shape == (3, 5, 37) and allh.shape == (3, 16, 5, 37) and mean.dtype == allh.dtype == np.float32
    assert np.array_equal(allh[1, 7, 2], p[2, 1, 7, :37]) and np.array_equal(AM.mean_of_all_np(allh), mean)
    # the order is part of the contract: heads 0 .. 15 one after the other, one multiply by 1 / 16
    acc = np.float32(0.0)
    for h in range(16):
        acc = np.float32(acc + p[4, 2, h, 9])
    assert mean[2, 4, 9] == np.float32(acc * np.float32(0.0625))
    pairwise = p[:, :, :, :37].reshape(5, 3, 8, 2, 37).sum(3).sum(2) * np.float32(0.0625)           # another association: not the same bits
    assert not np.array_equal(pairwise.transpose(1, 0, 2), mean) and np.abs(pairwise.transpose(1, 0, 2) - mean).max() < 1e-6
    assert bool((mean[1, 2, 40 - 37:] >= 0).all()) and np.array_equal(AM.attention_map_np(p, 64)[1, 2, 40:], np.zeros(24, np.float32))


# ------------------------------------------------------------------------------------- the loop-level test's seed: d_min >= 1e-2
@pytest.fixture(scope="module")
def oracle(tiny_sampler_sd):
    return DecoderOracle(tiny_sampler_sd, 2, 16)


@pytest.mark.parametrize("cfg,Tp,pattern", [(3.0, 0, "default"), (1.0, 5, "parallel")])
def test_chosen_seed_separates_the_plumbing_faults(oracle, cfg, Tp, pattern):
    """d_min — the smallest max |wrong - right| over: the other layer, step i +- 1, another clip's row, the null-condition row — is at
    least 1e-2 on the fp64 restatement of a greedy CPU decode of the GPU test's clips, so `err < d_min / 4` there cannot pass vacuously."""
    K = oracle.K
    feats = synth.video_features(LOOP_B, tokens=LOOP_TV, seed=LOOP_FEAT_SEED)
    delays = list(range(K)) if pattern == "default" else [0] * K
    prompt = torch.randint(0, 1024, (LOOP_B, K, Tp), generator=torch.Generator().manual_seed(9)) if Tp else None
    seq = AM.greedy_sequence(oracle, feats, LOOP_T, cfg, delays, prompt)
    S = LOOP_T + max(delays) + 1
    assert seq.shape == (LOOP_B, K, S) and int(seq.min()) >= 0
    start = Tp + 1 + delays[0]
    cond = AM.layer_probs(oracle, seq[..., :S - 1], feats)
    null = AM.layer_probs(oracle, seq[..., :S - 1], oracle.null_condition(feats)) if cfg > 1.0 else None
    assert cond.shape == (2, LOOP_B, 16, S - 1, S - 1) and bool((cond.sum(-1) - 1).abs().max() < 1e-12)
    assert bool((cond.triu(1) == 0).all())
    for layer in (0, 1):
        d, faults = AM.d_min(cond, null, layer, start)
        print(f"cfg {cfg} prompt {Tp} {pattern} layer {layer}: d_min {d:.4f} {faults}")
        assert d >= 1e-2, (layer, faults)
        assert set(faults) == ({"layer", "step", "clip", "null"} if cfg > 1.0 else {"layer", "step", "clip"})
    # the fp32 restatement agrees with the fp64 one at fp32 level: the bar of the exact-fp32 engine is not vacuous either
    e_ref = AM.rel_err(AM.layer_probs(oracle, seq[..., :S - 1], feats, torch.float32), cond)
    print(f"e_ref {e_ref:.3e}")
    assert e_ref < 1e-4
