"""Attention maps on the device: attention_step256_probs_kernel<96, 0..3> through vaura_attention_step_probs (op level),
attention_map_kernel through vaura_attention_map, and generate_codes(return_attention_weights=True) on the tiny checkpoint (loop level).

Op level: the weights against the fp64 softmax of the reference's own q64 / k64 on the numbers the cache holds, bar = the project's
A.bar (3e-6 alone on flat); out, planes and appended K / V bit-equal to the launch without probs; nothing written where nothing is due.
Loop level: exact properties on every storage, and the map against an fp64 teacher-forced restatement of the engine's own tokens
(tests/attention_maps_reference.py) — A.bar on the exact-fp32 engine, err < d_min / 4 on the plane and narrow-cache engines.
Measured lines: set VAURA_ATTENTION_MAPS_PARITY_OUT=<file> (profiles/attention_maps_parity.txt holds such lines; appended)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_maps_reference as AM  # noqa: E402
import attention_reference as A  # noqa: E402
import kv_f8s_reference as F8  # noqa: E402
from oracle.decoder_oracle import DecoderOracle, rope_table  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import ops, synth  # noqa: E402
from vaura_amd.engine import DecoderEngine  # noqa: E402

DEV = "cuda:0"
H, HD, D = A.H, A.HD, A.D
MAX_LEN = 256
STORAGE = {0: "f32", 1: "f16", 2: "e4m3", 3: "e4m3s"}

_lines = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    out = os.environ.get("VAURA_ATTENTION_MAPS_PARITY_OUT")
    if _lines and out:
        with open(out, "a") as f:
            f.writelines(line + "\n" for line in _lines)


def note(line):
    _lines.append(line)
    print("attention maps:", line)


# ---------------------------------------------------------------------------------------------------------------- a. op level
FAMILIES = ("flat", "peaked", "huge_first", "huge_new")
POSITIONS = (0, 1, 63, 64, 65, 128, 193, 255)
ROWS = ((1, 1), (6, 3))                      # (rows, rows_out)


def seed_of(name):
    return 1000 + 17 * A.FAMILIES.index(name)


def hot_for(name, pos):
    """index of the one huge key: the new position, or the first key of the last (possibly partial) 64-block of the cache"""
    if not name.startswith("huge"):
        return None
    return pos if (name == "huge_new" or pos == 0) else (pos - 1) // 64 * 64


def store(x, kv):
    """x (..., 96) fp32 as storage kv holds it -> (elements, exponent bytes or None)"""
    if kv == 3:
        return F8.quantise(x)
    return A.narrow(x, kv), None


def widen(t, sc, kv):
    return F8.widen(t.view(torch.uint8), sc) if kv == 3 else A.widen(t)


def raw(t):
    return t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t


class Cache:
    """The K / V cache of one family in one storage, as an exact kernel would have built it: pristine device copies"""

    def __init__(self, name, kv, rows=6):
        self.name, self.kv, self.rows = name, kv, rows
        self.rope = rope_table(MAX_LEN, HD)
        self.rope_d = self.rope.to(DEV)
        self.qr, self.kr, self.v = A.family(name, rows, MAX_LEN, seed_of(name), self.rope)
        self.krot = A.rope32(self.kr, self.rope, 0)
        (self.K, self.Ks), (self.V, self.Vs) = store(self.krot, kv), store(self.v, kv)
        self.dev = [None if t is None else t.to(DEV) for t in (self.K, self.Ks, self.V, self.Vs)]

    def case(self, rows, pos):
        """(raw q, k, v of the new position (rows, H, 1, hd), device caches [K, Ks, V, Vs] of `rows` rows, fp64 keys [0, pos))"""
        q, k, v = (x[:rows, :, pos:pos + 1].clone() for x in (self.qr, self.kr, self.v))
        dev = [None if t is None else t[:rows].clone() for t in self.dev]
        K64 = widen(self.K[:rows, :, :pos], None if self.Ks is None else self.Ks[:rows, :, :pos], self.kv)
        hot = hot_for(self.name, pos)
        if hot is not None:
            kr_hot = A.huge_key(self.kr, self.rows, seed_of(self.name), self.rope, hot)[:rows]      # (rows, H, hd) raw
            if hot == pos:
                k = kr_hot[:, :, None].clone()
            else:
                t, sc = store(A.rope32(kr_hot[:, :, None], self.rope, hot)[:, :, 0], self.kv)
                raw(dev[0])[:, :, hot] = raw(t).to(DEV)
                if sc is not None:
                    dev[1][:, :, hot] = sc.to(DEV)
                K64[:, :, hot] = widen(t, sc, self.kv)
        # the slot the call must write holds garbage before it
        raw(dev[0])[:, :, pos] = 0x47 if self.kv else 7.0
        raw(dev[2])[:, :, pos] = 0x47 if self.kv else 7.0
        return q, k, v, dev, K64


def qkv_rows(q, k, v):
    R = q.shape[0]
    return torch.cat([x[:, :, 0].reshape(R, D) for x in (q, k, v)], dim=-1)


def launch(c, rows, pos, q, k, v, dev, probs=None, pos0=0, **kw):
    qp = ops.pack_rows(qkv_rows(q, k, v).to(DEV))
    a = dict(kv_dtype=c.kv, kscale=dev[1], vscale=dev[3], want_split=True, **kw)
    if probs is None:
        return ops.attention_step_kv(qp, c.rope_d, dev[0], dev[2], rows, H, HD, pos, **a)
    return ops.attention_step_probs(qp, c.rope_d, dev[0], dev[2], rows, H, HD, pos, probs, pos0, **a)


@pytest.mark.parametrize("kv", [0, 1, 2, 3])
@pytest.mark.parametrize("name", FAMILIES)
def test_step_probs_every_storage_family_position_and_row_count(name, kv):
    c = Cache(name, kv)
    worst = [0.0, 0.0, 0.0]
    for pos in POSITIONS:
        for rows, rows_out in ROWS:
            q, k, v, dev, K64 = c.case(rows, pos)
            base_dev = [None if t is None else t.clone() for t in dev]
            out0, split0 = launch(c, rows, pos, q, k, v, base_dev)
            # two steps' worth of buffer, this call is step 0 of it: step 1, rows >= rows_out and columns > pos must keep the 7.0
            probs = torch.full((2, rows_out, H, MAX_LEN), 7.0, device=DEV)
            out1, split1 = launch(c, rows, pos, q, k, v, dev, probs, pos)
            torch.cuda.synchronize()
            where = f"{STORAGE[kv]} {name} rows {rows} pos {pos}"
            assert torch.equal(out1, out0) and torch.equal(split1, split0), f"{where}: out / planes differ from the launch without probs"
            for got, want in zip(dev, base_dev):
                assert got is None or torch.equal(raw(got), raw(want)), f"{where}: cache / exponent bytes differ from the launch without probs"
            p = probs.cpu()
            assert bool((p[1] == 7.0).all()) and bool((p[0, :, :, pos + 1:] == 7.0).all()), f"{where}: written where nothing is due"
            got = p[0, :, :, :pos + 1].double()
            assert bool(torch.isfinite(got).all())
            # fp64 softmax of the reference's own rotated q against the keys the cache holds (the new one as stored by this call)
            q64, _ = A.rope64(q[:rows_out], c.rope, pos)
            k_new = widen(dev[0][:rows_out, :, pos:pos + 1].cpu(), None if dev[1] is None else dev[1][:rows_out, :, pos:pos + 1].cpu(), kv)
            keys = torch.cat([K64[:rows_out], k_new], dim=2)
            ref = torch.softmax(torch.matmul(q64, keys.transpose(-1, -2))[:, :, 0] / math.sqrt(HD), dim=-1)
            p32 = torch.softmax(torch.matmul(A.rope32(q[:rows_out], c.rope, pos), keys.float().transpose(-1, -2))[:, :, 0] / math.sqrt(HD), dim=-1)
            err, e_ref = A.rel_err(got, ref), A.rel_err(p32, ref)
            sum_err = float((got.sum(-1) - 1.0).abs().max())
            limit = 3e-6 if name == "flat" else A.bar(e_ref)
            print(f"{where}: err {err:.3e} e_ref {e_ref:.3e} |sum - 1| {sum_err:.3e} bar {limit:.3e}")
            worst = [max(worst[0], err), max(worst[1], e_ref), max(worst[2], sum_err)]
            assert err <= limit, f"{where}: err {err:.3e} > {limit:.3e} (e_ref {e_ref:.3e})"
            assert sum_err <= limit, f"{where}: |sum - 1| {sum_err:.3e} > {limit:.3e}"
            assert bool((got[..., pos] > 0).all()) or name != "flat"
    note(f"op step256_probs {STORAGE[kv]:5s} {name:10s} err {worst[0]:.3e}  e_ref {worst[1]:.3e}  |sum - 1| {worst[2]:.3e}  "
         f"bar {'3.0e-06' if name == 'flat' else 'max(3e-6, 4 e_ref)'}  calls {len(POSITIONS) * len(ROWS)}")


@pytest.mark.parametrize("kv", [0, 3])
def test_a_position_outside_the_request_writes_nothing(kv):
    c = Cache("flat", kv)
    rows, rows_out, n_steps, pos0 = 6, 3, 4, 60
    for pos in (pos0 - 1, pos0 + n_steps):
        q, k, v, dev, _ = c.case(rows, pos)
        base_dev = [None if t is None else t.clone() for t in dev]
        out0, split0 = launch(c, rows, pos, q, k, v, base_dev)
        probs = torch.full((n_steps, rows_out, H, MAX_LEN), 7.0, device=DEV)
        out1, split1 = launch(c, rows, pos, q, k, v, dev, probs, pos0)
        torch.cuda.synchronize()
        assert bool((probs == 7.0).all()), pos
        assert torch.equal(out1, out0) and torch.equal(split1, split0)
        assert all(g is None or torch.equal(raw(g), raw(w)) for g, w in zip(dev, base_dev))
    # the last step of the request lands in the last row of the buffer, and only there
    pos = pos0 + n_steps - 1
    q, k, v, dev, _ = c.case(rows, pos)
    probs = torch.full((n_steps, rows_out, H, MAX_LEN), 7.0, device=DEV)
    launch(c, rows, pos, q, k, v, dev, probs, pos0)
    torch.cuda.synchronize()
    assert bool((probs[:-1] == 7.0).all()) and bool((probs[-1, :, :, :pos + 1] < 1.0).all()) and bool((probs[-1, :, :, pos + 1:] == 7.0).all())


def test_long_caches_and_range_splits_are_refused_and_nothing_is_written():
    rows = 2
    qp = ops.pack_rows(torch.randn(rows, 3 * D, device=DEV))
    for max_len, n_split in ((257, 1), (256, 2), (1024, 4)):
        rope = rope_table(max_len, HD).to(DEV)
        kc = torch.zeros(rows, H, max_len, HD, device=DEV)
        vc = kc.clone()
        out = torch.full((16 * D,), float("nan"), device=DEV)
        probs = torch.full((1, rows, H, max_len), 7.0, device=DEV)
        with pytest.raises(L.VauraHipError, match="VAURA_ERR_SHAPE"):
            ops.attention_step_probs(qp, rope, kc, vc, rows, H, HD, 5, probs, 5, n_split=n_split, out=out)
        torch.cuda.synchronize()
        assert bool((probs == 7.0).all()) and bool(torch.isnan(out).all()) and not bool(kc.ne(0).any()) and not bool(vc.ne(0).any())


@pytest.mark.parametrize("shape,W", [((5, 3, 16, 64), 37), ((1, 1, 16, 256), 256), ((28, 3, 16, 256), 28)])
def test_attention_map_kernel_equals_its_restatement(shape, W):
    g = torch.Generator().manual_seed(11)
    p = torch.rand(shape, generator=g)
    p[0, 0, :, W // 2:] = 0.0
    for heads in ("mean", "all"):
        got = ops.attention_map(p.to(DEV), W, heads).cpu().numpy()
        want = AM.attention_map_np(p.numpy(), W, heads)
        assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), heads


# ---------------------------------------------------------------------------------------------------------------- b. loop level
B, K, V, T, TV, FEAT_SEED = 3, 9, 1024, 20, 32, 31          # tests/test_attention_maps_host.py holds d_min >= 1e-2 for these clips
ENGINES = [("f32", "f32"), ("h2", "f32"), ("h1", "f32"), ("h2", "f16"), ("h2", "f8s")]
#         cfg, sampled, prompt frames, pattern: every pair of values of any two of the four occurs
CASES = [(3.0, True, 0, "default"), (1.0, False, 5, "default"), (3.0, False, 5, "parallel"), (1.0, True, 0, "parallel"),
         (3.0, True, 5, "default"), (1.0, False, 0, "parallel")]


@pytest.fixture(scope="module", params=ENGINES, ids=lambda p: f"{p[0]}-kv_{p[1]}")
def engine(request, tiny_sampler_sd):
    w, kv = request.param
    return DecoderEngine(synth.tiny_sampler(2), tiny_sampler_sd, DEV, wdtype=w, near_tie="off", kv_dtype=kv)


_oracles, _refs = {}, {}


def reference(sd, wdtype, kv_dtype, seq, feats, cfg_on, start):
    """fp64 (and on "f32" fp32) per-head maps of both layers for the engine's own tokens, and d_min per layer — cached per (storages,
    tokens): the restatement runs once and is shared, unchanged, by whatever needs it.  It holds the numbers the storages hold: the
    effective weights of the fp16 planes, and k / v as the K / V cache stores them (AM.cache_values) — the weights are defined on the
    stored keys.  (Without the cache's rounding in the restatement the scaled e4m3 engine measured 1.0e-2 .. 2.0e-2 against it, above
    d_min / 4 = 0.009 .. 0.010 in the cfg-3 cases: that figure was the storage's own rounding of k, not the map's arithmetic.)"""
    if wdtype not in _oracles:
        _oracles[wdtype] = DecoderOracle(AM.effective_sd(sd, wdtype), 2, 16)
    orc = _oracles[wdtype]
    key = (wdtype, kv_dtype, seq.numpy().tobytes(), cfg_on, start)
    if key not in _refs:
        _refs.clear()
        seq_in = seq[..., :-1]
        cond = AM.layer_probs(orc, seq_in, feats, kv_dtype=kv_dtype)
        null = AM.layer_probs(orc, seq_in, orc.null_condition(feats), kv_dtype=kv_dtype) if cfg_on else None
        p32 = AM.layer_probs(orc, seq_in, feats, torch.float32) if wdtype == "f32" else None
        _refs[key] = (cond, p32, [AM.d_min(cond, null, l, start) for l in range(2)])
    return _refs[key]


@pytest.mark.parametrize("cfg,sampled,Tp,pattern", CASES, ids=lambda v: str(v))
def test_loop_maps(engine, tiny_sampler_sd, cfg, sampled, Tp, pattern):
    delays = None if pattern == "default" else [0] * K
    dl = list(range(K)) if delays is None else delays
    S, start = T + max(dl) + 1, Tp + 1 + dl[0]
    n = S - start
    feats_c = synth.video_features(B, tokens=TV, seed=FEAT_SEED)
    feats = feats_c.to(DEV)
    prompt = torch.randint(0, V, (B, K, Tp), generator=torch.Generator().manual_seed(9)) if Tp else None
    kw = dict(prompt=prompt, seed=5, delays=delays, cfg_scale=cfg, use_sampling=sampled, temp=0.8 if sampled else 1.0, top_k=250 if sampled else 0)
    case = f"loop {engine.wdtype} kv {engine.kv_dtype} cfg {cfg} {'philox' if sampled else 'greedy'} prompt {Tp} {pattern}"

    plain = engine.generate_codes(feats, T, **kw)
    engine.check_status()
    key_plain = engine._graph_key
    assert int(engine.dec.ext_bytes) == 40 and engine.attn_probs is None
    got, extra = engine.generate_codes(feats, T, return_attention_weights=True, **kw)
    engine.check_status()
    assert set(extra) == {"attention"} and int(engine.dec.ext_bytes) == 64 and engine._graph_key != key_plain
    assert engine.rows == (2 * B if cfg > 1.0 else B) and tuple(engine.attn_probs.shape) == (n, B, H, engine.max_len)
    m = extra["attention"]
    assert m.shape == (B, n, S - 1) and m.dtype == torch.float32 and m.device.type == "cuda"
    assert torch.equal(got, plain), "the flag changed a token"
    seq = engine.seq.cpu().to(torch.int64)
    # the graph run and the eager run give the same map, and the same tokens
    got_e, extra_e = engine.generate_codes(feats, T, return_attention_weights=True, use_graph=False, **kw)
    assert torch.equal(got_e, plain) and torch.equal(extra_e["attention"], m), "graph and eager maps differ"
    # row i: exactly 0 from column start + i on, > 0 at column start + i - 1
    cols = torch.arange(S - 1, device=DEV)[None, :]
    last = (start - 1 + torch.arange(n, device=DEV))[:, None]
    assert bool((m[:, cols.expand(n, -1) > last] == 0).all()), "weights right of a step's own position"
    assert bool((m[:, torch.arange(n, device=DEV), last[:, 0]] > 0).all()) and bool((m >= 0).all()) and bool(torch.isfinite(m).all())
    assert bool(((m.double().sum(-1) - 1).abs() < 1e-5).all())
    # every head, and its fixed-order mean; with both other flags in the same call
    got_a, extra_a = engine.generate_codes(feats, T, return_attention_weights=True, attention_heads="all", return_logprobs=True,
                                           return_relevance=cfg > 1.0, **kw)
    allh = extra_a["attention"]
    assert torch.equal(got_a, plain) and allh.shape == (B, H, n, S - 1)
    assert {"attention", "logprobs", "score"} <= set(extra_a) and ("relevance" in extra_a) == (cfg > 1.0)
    assert np.array_equal(AM.mean_of_all_np(allh.cpu().numpy()).view(np.int32), m.cpu().numpy().view(np.int32)), "mean is not the fixed-order mean of all"
    _, lp = engine.generate_codes(feats, T, return_logprobs=True, return_relevance=cfg > 1.0, **kw)
    assert all(torch.equal(lp[k_].view(torch.int32), extra_a[k_].view(torch.int32)) for k_ in lp), "the flag changed a reported value"
    # the two layers both run and differ; the default is the last layer
    _, e0 = engine.generate_codes(feats, T, return_attention_weights=True, attention_layer=0, attention_heads="all", **kw)
    _, e1 = engine.generate_codes(feats, T, return_attention_weights=True, attention_layer=1, attention_heads="all", **kw)
    _, em = engine.generate_codes(feats, T, return_attention_weights=True, attention_layer=-2, attention_heads="all", **kw)
    assert torch.equal(e1["attention"], allh) and torch.equal(em["attention"], e0["attention"]) and not torch.equal(e0["attention"], allh)
    # clip 1's map does not depend on the other clips' videos
    other = synth.video_features(B, tokens=TV, seed=FEAT_SEED + 1)
    other[1] = feats_c[1]
    got_o, extra_o = engine.generate_codes(other.to(DEV), T, return_attention_weights=True, **kw)
    assert torch.equal(got_o[1], plain[1]) and torch.equal(extra_o["attention"][1], m[1]) and not torch.equal(extra_o["attention"][0], m[0])
    # and back: an unflagged call after the flagged ones replays the graph it always did and returns the original tokens
    again = engine.generate_codes(feats, T, **kw)
    engine.check_status()
    assert torch.equal(again, plain) and engine._graph_key == key_plain and int(engine.dec.ext_bytes) == 40
    assert int(engine.dec_ext4.attn_probs or 0) == 0 and engine.attn_probs is None

    # arithmetic: the fp64 teacher-forced restatement of the returned tokens, on the storage's effective weights
    cond64, p32, dmins = reference(tiny_sampler_sd, engine.wdtype, engine.kv_dtype, seq, feats_c, cfg > 1.0, start)
    for layer, got_l in ((0, e0["attention"]), (1, allh)):
        ref = AM.map_all(cond64[layer], start)
        err_abs = float((got_l.cpu().double() - ref).abs().max())
        err = AM.rel_err(got_l.cpu(), ref)
        d, faults = dmins[layer]
        assert d >= 1e-2, (case, layer, faults)
        if engine.wdtype == "f32":
            e_ref = AM.rel_err(AM.map_all(p32[layer], start), ref)
            note(f"{case} layer {layer}: err {err:.3e}  e_ref {e_ref:.3e}  bar {A.bar(e_ref):.3e}  d_min {d:.4f}")
            assert err <= A.bar(e_ref), (case, layer, err, e_ref)
        else:
            note(f"{case} layer {layer}: max |error| {err_abs:.3e}  d_min {d:.4f}  d_min / 4 {d / 4:.4f}  ({min(faults, key=faults.get)})")
        assert err_abs < d / 4, (case, layer, err_abs, faults)


# ---------------------------------------------------------------------------------------------------------------- c. plugin surface
def _model(sd):
    import warnings
    from vaura_amd.model import VAURAModel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VAURAModel(
            feature_extractor_config={"target": "vaura_amd.feature_extractor.MotionFormer"},
            audio_encoder_config={"target": "vaura_amd.codec.DacModelWrapper", "params": {"model_sr": 44100, "synthetic": True}},
            sampler_config={"target": "vaura_amd.sampler.Transformer", "params": synth.tiny_sampler(2).yaml_params()},
            visual_bridge_config={"target": "torch.nn.Identity"},
            pattern_provider_config={"target": "vaura_amd.patterns.DelayedPatternProvider", "params": {"n_q": 9}},
            flatten_vis_feats=True, freeze_feature_extractor=True, noise_mode="philox")
    m.sampler.load_state_dict(sd, strict=True)
    m.sampler.audio_tokens_per_video_frame = 7
    return m.to(DEV)


def test_generate_returns_the_engine_map_and_changes_nothing_else(tiny_sampler_sd):
    m = _model(tiny_sampler_sd)
    frames = synth.video_features(B, tokens=TV, seed=FEAT_SEED).reshape(B, 1, TV, 768).to(DEV)
    kw = dict(frames=frames, max_new_tokens=T, use_sampling=True, temp=0.8, top_k=250, cfg_scale=3.0, return_sampled_indices=True)
    S = T + K
    plain = m.generate(**kw)
    assert plain["s_attn_weights"] is None and plain["mha_attn_weights"] is None
    r = m.generate(return_attention_weights=True, **kw)
    assert set(r) == set(plain) and r["mha_attn_weights"] is None
    assert torch.equal(r["sampled_indices"], plain["sampled_indices"]) and torch.equal(r["generated_audio"], plain["generated_audio"])
    w = r["s_attn_weights"]
    assert w.shape == (B, S - 1, S - 1) and w.dtype == torch.float32 and w.device.type == "cuda"
    assert bool((w.triu(1) == 0).all()) and bool((w.diagonal(dim1=1, dim2=2) > 0).all()) and bool(((w.double().sum(-1) - 1).abs() < 1e-5).all())
    eng = m.sampler.engine()
    assert torch.equal(w, eng.attention_map("mean")) and int(eng.dec_ext4.attn_layer) == 1        # the last layer of the two
    a = m.generate(return_attention_weights=True, attention_heads="all", attention_layer=0, return_relevance=True, **kw)
    assert a["s_attn_weights"].shape == (B, H, S - 1, S - 1) and torch.equal(a["sampled_indices"], plain["sampled_indices"])
    assert "relevance" in a and int(eng.dec_ext4.attn_layer) == 0
    t = m.generate_tokens(**{k: v for k, v in kw.items() if k != "return_sampled_indices"}, return_attention_weights=True)
    assert set(t) == {"tokens", "s_attn_weights"} and torch.equal(t["tokens"], plain["sampled_indices"]) and torch.equal(t["s_attn_weights"], w)
    again = m.generate(**kw)
    assert again["s_attn_weights"] is None and torch.equal(again["generated_audio"], plain["generated_audio"])
