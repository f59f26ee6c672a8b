"""Teacher-forced evaluation (VAURAModel.forward + _compute_loss, vaura_model.py:136-192, 240-280) on the host: the goldens the
reference itself produced (tests/golden/make_golden_eval.py) restated in numpy and by the CPU decoder oracle, the auto-set rule of
audio_tokens_per_video_frame, and what the plugin and the C ABI refuse without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle.decoder_oracle import DecoderOracle
from vaura_amd import _lib as L
from vaura_amd import synth
from vaura_amd.patterns import DelayedPatternProvider

SETS = ("delayed", "parallel", "even")


def _pattern_input(codes: np.ndarray, delays, special: int = 1024) -> np.ndarray:
    """build_pattern_sequence(codes[..., :-1]) against a pattern of Ta timesteps: S = Ta + max(d) + 1, step p of codebook q holds
    codes[..., p - 1 - d_q] when that is a timestep < Ta - 1, the special token otherwise."""
    B, K, Ta = codes.shape
    S = Ta + max(delays) + 1
    seq = np.full((B, K, S), special, dtype=np.int64)
    for q, d in enumerate(delays):
        for p in range(S):
            t = p - 1 - d
            if 0 <= t < Ta - 1:
                seq[:, q, p] = codes[:, q, t]
    return seq


def _nll(logits: np.ndarray, targets: np.ndarray) -> np.ndarray:
    """F.cross_entropy(reduction='none') over the last axis, float64."""
    x = logits.astype(np.float64)
    m = x.max(-1, keepdims=True)
    lse = (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))[..., 0]
    return lse - np.take_along_axis(x, targets[..., None].astype(np.int64), -1)[..., 0]


@pytest.mark.parametrize("name", SETS)
def test_numpy_restatement_reproduces_the_reference_loss(golden, name):
    g = golden("eval_tiny.npz")
    codes = g[f"{name}_codes"].astype(np.int64)
    keep = [int(t) for t in g["keep_t"]]
    nll = g[f"{name}_nll"].astype(np.float64)
    assert g[f"{name}_mask"].all()                               # delay patterns give every timestep a logit
    got = _nll(g[f"{name}_logits"], codes[:, :, keep])
    assert np.abs(got - nll[:, :, keep]).max() < 2e-5
    # _compute_loss: per-codebook mean over (b, t), then the mean over the codebooks
    lpc = nll.mean(axis=(0, 2))
    assert np.allclose(lpc, g[f"{name}_loss_per_codebook"], rtol=1e-5, atol=0)
    assert abs(lpc.mean() - float(g[f"{name}_loss"])) < 1e-5 * float(g[f"{name}_loss"])


@pytest.mark.parametrize("name", SETS)
def test_oracle_teacher_forced_logits_match_the_reference(golden, tiny_sampler_sd, name):
    g = golden("eval_tiny.npz")
    codes = g[f"{name}_codes"].astype(np.int64)
    delays = [int(d) for d in g[f"{name}_delays"]]
    keep = [int(t) for t in g["keep_t"]]
    B, K, Ta = codes.shape
    feats = synth.video_features(B, seed=int(g["feat_seed"]))
    orc = DecoderOracle(tiny_sampler_sd, num_layers=int(g["layers"]), nhead=16)
    seq = _pattern_input(codes, delays)
    out = orc.forward_full(torch.from_numpy(seq[..., :-1]), feats).numpy()    # positions [0, S - 1): the last one predicts nothing
    # revert_pattern_logits: model-output position s of codebook q predicts timestep t = s - d_q
    rev = np.stack([out[:, q, [t + delays[q] for t in keep]] for q in range(K)], axis=1)
    assert np.abs(rev - g[f"{name}_logits"]).max() < 3e-5


def test_full_golden_is_self_consistent(golden):
    g = golden("eval_full_raw_B2_T220.npz")
    ref = golden("full_greedy_raw_B2_T220.npz")
    keep = [int(t) for t in g["keep_t"]]
    for name, codes in (("greedy", ref["tokens"].astype(np.int64)), ("uniform", g["uniform_codes"].astype(np.int64))):
        nll = g[f"{name}_nll"].astype(np.float64)
        assert nll.shape == (2, 9, 220) and g[f"{name}_mask"].all()
        assert np.abs(_nll(g[f"{name}_logits"], codes[:, :, keep]) - nll[:, :, keep]).max() < 2e-5
        assert np.allclose(nll.mean(axis=(0, 2)), g[f"{name}_loss_per_codebook"], rtol=1e-5, atol=0)
    # greedy tokens are each row's argmax: the scored tokens are far more likely than uniform ones
    assert float(g["greedy_loss"]) < float(g["uniform_loss"])


def test_tokens_per_frame_auto_rule():
    from vaura_amd.model import VAURAModel
    rule = VAURAModel._auto_tokens_per_frame
    # llama.py:_set_audio_tokens_per_video_frame: S - K under a delayed pattern, S - 1 otherwise, over Tv, rounded up
    assert rule(220 + 9, 32, "DelayedPatternProvider", 9) == math.ceil(220 / 32) == 7
    assert rule(220 + 1, 32, "ParallelPatternProvider", 9) == math.ceil(220 / 32)
    assert rule(20 + 17, 4, "DelayedPatternProvider", 9) == math.ceil(28 / 4)     # delays 0,2,..,16: the rule still subtracts K
    assert rule(20 + 1, 4, None, 9) == 5


@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from ckpt_fixture import write_checkpoint
    from vaura_amd.model import VAURAModel
    d = tmp_path_factory.mktemp("ckpt_eval")
    ckpt, hp, _ = write_checkpoint(str(d), synth.tiny_sampler(2))
    return VAURAModel.load_from_checkpoint(ckpt, hparams_file=hp, map_location="cpu")


def test_scoring_refusals_on_the_host(cpu_model):
    m = cpu_model
    vis = torch.zeros(1, 32, 768)
    old, old_tpf = m.pattern_provider, m.sampler.audio_tokens_per_video_frame
    try:
        # Ta + max(d) + 1 > block_size (256): refused before the engine is touched
        m.pattern_provider = DelayedPatternProvider(9, delays=list(range(0, 18, 2)))
        with pytest.raises(L.VauraHipError, match="block_size"):
            m._score(torch.zeros(1, 9, 240, dtype=torch.long), vis)
        m.pattern_provider = DelayedPatternProvider(9)
        with pytest.raises(L.VauraHipError, match="block_size"):
            m._score(torch.zeros(1, 9, 250, dtype=torch.long), vis)

        class UnrolledPatternProvider:
            def get_pattern(self, timesteps):
                return object()
        m.pattern_provider = UnrolledPatternProvider()
        with pytest.raises(L.VauraHipError, match="not a delay pattern"):
            m._score(torch.zeros(1, 9, 20, dtype=torch.long), vis)
        # the refusals come first: audio_tokens_per_video_frame is not set by a refused call
        m.sampler.audio_tokens_per_video_frame = None
        m.pattern_provider = DelayedPatternProvider(9)
        with pytest.raises(L.VauraHipError, match="block_size"):
            m._score(torch.zeros(1, 9, 250, dtype=torch.long), vis)
        assert m.sampler.audio_tokens_per_video_frame is None
    finally:
        m.pattern_provider, m.sampler.audio_tokens_per_video_frame = old, old_tpf


def test_score_entry_points_check_their_arguments_without_a_gpu():
    lib = L.lib()
    assert lib.vaura_score(None, 10, 0, 0, 0, 0, 0, 0, 0, 0) == -1
    assert lib.vaura_score_logits(0, 0, 0, 1, 9, 1024, 20, 0, 0, 0, 0) == -1
    one = C.c_void_p(16)          # never dereferenced: the shape checks come first
    assert lib.vaura_score_logits(one, one, one, 1, 17, 1024, 20, one, one, one, 0) == -1      # K > 16
    assert lib.vaura_score_logits(one, one, one, 1, 9, 1000, 20, one, one, one, 0) == -2       # vocab not a multiple of 256
