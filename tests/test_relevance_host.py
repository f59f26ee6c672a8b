"""Video relevance, host side: the fp64 restatement (tests/relevance_reference.py) against a plain torch.log_softmax, what the plugin and
the C entry points refuse before any device work, and the descriptor layout (vaura_decoder keeps its size and every offset; the two
pointers live behind it, in vaura_decoder_ext)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relevance_reference as R  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import synth  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_reference_equals_log_softmax_in_fp64():
    g = torch.Generator().manual_seed(5)
    for scale in (1.0, 30.0):
        xc = (torch.randn(R.V, generator=g, dtype=torch.float64) * scale)
        xu = (torch.randn(R.V, generator=g, dtype=torch.float64) * scale)
        xc[17] = xc[900] = xc.max() + 1.0            # two equal maxima
        for tok in (0, 17, 900, 1023):
            lc, lu = R.token_relevance(xc.numpy(), xu.numpy(), tok)
            assert abs(lc - float(torch.log_softmax(xc, -1)[tok])) < 1e-12 * max(1.0, scale)
            assert abs(lu - float(torch.log_softmax(xu, -1)[tok])) < 1e-12 * max(1.0, scale)
    bad = xc.clone()
    bad[3] = float("-inf")
    assert all(np.isnan(v) for v in R.token_relevance(bad.numpy(), xu.numpy(), 5))
    assert all(np.isnan(v) for v in R.token_relevance(xc.numpy(), bad.numpy(), 5))


def test_stored_rule_and_means():
    assert R.stored(-1, 0, 12, -2.5) == -2.5 and R.stored(-1, 11, 12, -2.5) == -2.5
    assert R.stored(7, 3, 12, -2.5) == 0.0                       # prompt / known token
    assert R.stored(-1, -1, 12, -2.5) == 0.0 and R.stored(-1, 12, 12, -2.5) == 0.0      # special slots
    lc = np.full((2, 9, 5), -1.0, dtype=np.float32)
    lu = np.full((2, 9, 5), -3.0, dtype=np.float32)
    lu[1, 4, 2] = np.nan
    r, pcb, clip = R.sequence_relevance(lc, lu, 1)
    assert r[0, 0, 0] == 2.0 and np.all(pcb[0] == 2.0) and clip[0] == 2.0
    assert np.isnan(clip[1]) and np.isnan(pcb[1]).all()          # the NaN rule of vaura_sequence_logprob
    assert not np.isnan(R.sequence_relevance(lc, lu, 3)[2]).any()


# ---------------------------------------------------------------------------------------------------------------- struct layout
# offsets of vaura_decoder before this feature (x86-64); sizeof = 416, four bytes of padding at 380
OFFSETS = {'dims': 0, 'wdtype': 48, 'batch': 52, 'rows': 56, 'max_len': 60, 'timesteps': 64, 'seq_len': 68, 'n_cond_tokens': 72,
           'prefill_positions': 76, 'plane_shift': 80, 'kv_dtype': 84, 'layers_host': 88, 'heads': 96, 'final_norm': 104, 'tok_emb': 112,
           'tok_proj_w': 120, 'tok_proj_b': 128, 'tok_table': 136, 'empty_video': 144, 'rope': 152, 'cond_proj': 160, 'kcache': 168,
           'vcache': 176, 'seq': 184, 'state': 192, 'noise': 200, 'ws_h': 208, 'ws_qkv': 216, 'ws_qkv2': 224, 'ws_attn': 232, 'ws_ffn': 240,
           'ws_logits': 248, 'ws_h_split': 256, 'ws_attn_split': 264, 'ws_ffn_split': 272, 'ws_ss': 280, 'first_norm': 288,
           'ws_attn_part': 296, 'ws_sync': 304, 'has_pattern_delays': 312, 'pattern_delays': 316, 'kscale': 384, 'vscale': 392,
           'clip_sampling': 400, 'logprobs': 408}


def test_decoder_keeps_its_size_and_every_offset_and_the_pointers_follow_it():
    names = [n for n, _ in L.Decoder._fields_]
    assert [n for n in names if n != "ext_bytes"] == list(OFFSETS)
    for n, off in OFFSETS.items():
        assert getattr(L.Decoder, n).offset == off, n
    assert L.Decoder.ext_bytes.offset == 380 and L.Decoder.ext_bytes.size == 4      # the padding in front of kscale
    assert C.sizeof(L.Decoder) == 416
    assert L.DecoderExt.dec.offset == 0 and L.DecoderExt.logprobs_cond.offset == 416 and L.DecoderExt.logprobs_null.offset == 424
    assert C.sizeof(L.DecoderExt) == 432
    lib = L.lib()
    assert C.sizeof(L.Decoder) == lib.vaura_struct_size(3) and C.sizeof(L.DecoderExt) == lib.vaura_struct_size(10)
    assert C.sizeof(L.Sampling) == 48 == lib.vaura_struct_size(2)
    x = L.DecoderExt()
    assert x.dec.ext_bytes == 0 and x.logprobs_cond is None and x.logprobs_null is None      # zero-filled: relevance off
    x.dec.batch = 5                                                                 # ``dec`` is a view of the extension's memory
    assert x.dec.batch == 5 and C.addressof(x.dec) == C.addressof(x)


# ---------------------------------------------------------------------------------------------------------------- C entry points
def test_entry_points_refuse_before_any_device_work():
    lib = L.lib()
    one = C.c_void_p(16)          # never dereferenced: the checks come first
    sp = L.Sampling(0, 1.0, 0, 0.0, 3.0, 0, 0, 0, 0.0)
    args = lambda sp, tok, lc, lu: (one, 3, 9, 1024, C.byref(sp), None, None, 0, tok, None, 0, 0, None, None, lc, lu, None)  # noqa: E731
    assert lib.vaura_sample_relevance(*args(sp, one, None, one)) == -1              # exactly one of the two outputs
    assert lib.vaura_sample_relevance(*args(sp, one, one, None)) == -1
    assert lib.vaura_sample_relevance(*args(sp, None, one, one)) == -1              # no token output
    sp.cfg_scale = 1.0
    assert lib.vaura_sample_relevance(*args(sp, one, one, one)) == -1               # no null-condition rows
    sp.cfg_scale, sp.input_is_probs = 3.0, 1
    assert lib.vaura_sample_relevance(*args(sp, one, one, one)) == -1               # probability rows
    assert lib.vaura_score_relevance(None, 4, one, one, None, one, None, one, one, None, one, one, None) == -1


def _descriptor(rows):
    """a descriptor that passes the shape checks of vaura_decode_step; its pointers are never dereferenced by a refused call"""
    x = L.DecoderExt()
    d = x.dec
    d.ext_bytes = 16
    d.dims.n_layer, d.dims.d_model, d.dims.n_head, d.dims.ffn_dim = 2, 1536, 16, 4096
    d.dims.n_codebooks, d.dims.vocab, d.dims.cond_dim, d.dims.tok_dim = 9, 1024, 768, 768
    d.batch, d.rows, d.max_len, d.timesteps, d.seq_len = 3, rows, 32, 12, 21
    layers = (L.LayerWeights * 2)()
    d.layers_host = C.cast(layers, C.POINTER(L.LayerWeights))
    for n in ("heads", "final_norm", "tok_emb", "tok_proj_w", "tok_proj_b", "tok_table", "empty_video", "rope", "cond_proj", "kcache",
              "vcache", "seq", "state", "ws_h", "ws_qkv", "ws_attn", "ws_ffn", "ws_logits"):
        setattr(d, n, 16)
    return x, d, layers


@pytest.mark.parametrize("cond,null,rows,cfg", [(16, 0, 6, 3.0), (0, 16, 6, 3.0), (16, 16, 3, 3.0), (16, 16, 6, 1.0)],
                         ids=["cond_only", "null_only", "no_null_rows", "scalar_scale_does_not_say_doubled"])
def test_descriptor_refusals(cond, null, rows, cfg):
    x, d, _keep = _descriptor(rows)
    x.logprobs_cond, x.logprobs_null = cond, null
    sp = L.Sampling(0, 1.0, 0, 0.0, cfg, 0, 0, 0, 0.0)
    assert L.lib().vaura_decode_step(C.byref(d), C.byref(sp), 1, None) == -1        # VAURA_ERR_ARG, nothing launched


def test_extension_of_another_size_is_refused():
    x, d, _keep = _descriptor(6)
    d.ext_bytes = 8
    sp = L.Sampling(0, 1.0, 0, 0.0, 3.0, 0, 0, 0, 0.0)
    assert L.lib().vaura_decode_step(C.byref(d), C.byref(sp), 1, None) == -1


# ---------------------------------------------------------------------------------------------------------------- plugin refusals
@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    from ckpt_fixture import write_checkpoint
    from vaura_amd.model import VAURAModel
    d = tmp_path_factory.mktemp("ckpt_relevance")
    ckpt, hp, _ = write_checkpoint(str(d), synth.tiny_sampler(2))
    return VAURAModel.load_from_checkpoint(ckpt, hparams_file=hp, map_location="cpu")


@pytest.mark.parametrize("kw,match", [
    (dict(rank_by="likelihood"), "rank_by must be"),
    (dict(rank_by=None, num_candidates=3), "rank_by must be"),
    (dict(rank_by="relevance"), "pointless"),
    (dict(rank_by="relevance", num_candidates=1, return_logprobs=True), "pointless"),
    (dict(rank_by="relevance", num_candidates=3, use_sampling=False), "identical"),
    (dict(rank_by="relevance", return_relevance=True, num_candidates=0), "at least 1"),
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


def test_check_candidates_keeps_its_old_signature_and_accepts_the_new_arguments():
    from vaura_amd.model import VAURAModel
    assert VAURAModel._check_candidates(3, False, True, 0.9) == 3                   # rank_by defaults to "logprob"
    assert VAURAModel._check_candidates(3, False, True, 0.9, "relevance") == 3
    assert VAURAModel._check_candidates(1, False, True, 0.9, "relevance", True) == 1
