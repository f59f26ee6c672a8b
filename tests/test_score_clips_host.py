"""Per-clip lengths in teacher-forced scoring, host side: what ``DecoderEngine.score_clips`` refuses before any device work
(clip_params.resolve_score_lengths / score_list_lengths), that ``score()`` still keeps one length per call, and a numpy restatement
of the masked means the device kernels produce (csrc/score.hip score_reduce_clips_kernel, vaura_sequence_logprob_clips)."""
import numpy as np
import pytest
import torch

from vaura_amd import _lib as L
from vaura_amd import clip_params, synth
from vaura_amd.engine import DecoderEngine


def test_resolve_score_lengths():
    assert clip_params.resolve_score_lengths(3, 20) == (None, None)
    assert clip_params.resolve_score_lengths(3, 20, [20, 13, 7], [32, 2, 1], 32) == ([20, 13, 7], [32, 2, 1])
    assert clip_params.resolve_score_lengths(2, 5, torch.tensor([2, 5]), None, 32) == ([2, 5], None)
    assert clip_params.resolve_score_lengths(2, 5, None, (1, 32), 32) == (None, [1, 32])
    for args, match in (((3, 20, [20, 13]), "2 values"), ((3, 20, [20, 13.0, 7]), "integers"), ((3, 20, [20, True, 7]), "integers"),
                        ((3, 20, [20, 13, 1]), "2 .. 20"), ((3, 20, [21, 13, 7]), "2 .. 20"), ((3, 20, 13), "one integer per clip"),
                        ((3, 20, torch.ones(3, 1, dtype=torch.int64)), "one-dimensional"),
                        ((3, 20, None, [32, 2], 32), "2 values"), ((3, 20, None, [32, 2, 0], 32), "video_lengths must lie"),
                        ((3, 20, None, [33, 2, 1], 32), "video_lengths must lie"), ((3, 20, None, [32, 2.5, 1], 32), "integers")):
        with pytest.raises(L.VauraHipError, match=match):
            clip_params.resolve_score_lengths(*args)


def test_score_list_lengths():
    a, b = torch.zeros(9, 12, dtype=torch.int64), torch.zeros(1, 9, 5, dtype=torch.int64)
    assert clip_params.score_list_lengths([a, b], 9) == [12, 5]
    for codes in ([a, torch.zeros(8, 5)], [a, torch.zeros(2, 9, 5)], [a, torch.zeros(5)], []):
        with pytest.raises(L.VauraHipError, match="codes"):
            clip_params.score_list_lengths(codes, 9)


def _bare_engine():
    eng = object.__new__(DecoderEngine)              # nothing but the configuration: whatever else is read raises AttributeError
    eng.cfg = synth.tiny_sampler(2)
    return eng


@pytest.mark.parametrize("lengths,kw,match", [
    ([12, 5], {}, "2 values"),                                             # wrong count
    ([12, 5.0, 7], {}, "integers"),                                        # non-integers
    ([12, 1, 7], {}, "2 .. 12"),                                           # Ta_b < 2
    ([12, 13, 7], {}, "2 .. 12"),                                          # Ta_b > Ta
    ([12, 5, 7], dict(video_lengths=[32, 0, 1]), "video_lengths must lie in 1 .. 32"),
    ([12, 5, 7], dict(video_lengths=[32, 33, 1]), "video_lengths must lie in 1 .. 32"),
    ([12, 5, 7], dict(video_lengths=[32, 2]), "2 values"),
    (None, dict(video_lengths=3), "one integer per clip"),
])
def test_score_clips_refuses_before_any_device_work(lengths, kw, match):
    eng = _bare_engine()
    codes, feats = torch.zeros(3, 9, 12, dtype=torch.int64), torch.zeros(3, 32, 768)
    with pytest.raises(L.VauraHipError, match=match):
        eng.score_clips(codes, feats, lengths, **kw)


def test_score_clips_refuses_a_bad_list_before_any_device_work():
    eng = _bare_engine()
    feats = torch.zeros(3, 32, 768)
    ok = [torch.zeros(9, 12, dtype=torch.int64), torch.zeros(1, 9, 5, dtype=torch.int64)]
    with pytest.raises(L.VauraHipError, match=r"codes of clip 2 must be \(9, Ta_b\)"):
        eng.score_clips(ok + [torch.zeros(8, 7, dtype=torch.int64)], feats)            # wrong K
    with pytest.raises(L.VauraHipError, match="2 .. 12"):
        eng.score_clips(ok + [torch.zeros(9, 1, dtype=torch.int64)], feats)            # a clip of one timestep
    with pytest.raises(L.VauraHipError, match="feats must be"):
        eng.score_clips(ok, feats)                                                     # two clips, three feature rows
    with pytest.raises(L.VauraHipError, match="shapes say"):
        eng.score_clips(ok + [torch.zeros(9, 7, dtype=torch.int64)], feats, [12, 5, 6])
    with pytest.raises(L.VauraHipError, match="codes must be"):
        eng.score_clips(torch.zeros(3, 8, 12, dtype=torch.int64), feats, [12, 5, 7])


def test_score_still_keeps_one_length_per_call():
    eng = _bare_engine()
    codes, feats = torch.zeros(2, 9, 12, dtype=torch.int64), torch.zeros(2, 32, 768)
    with pytest.raises(L.VauraHipError, match="one length for the whole call"):
        eng.score([codes[0], codes[1, :, :5]], feats)
    with pytest.raises(L.VauraHipError, match="one length for the whole call"):
        eng.score(codes, feats, video_lengths=[32, 2])


# ---------------------------------------------------------------------------------------------------------------- the masked means
def masked_means(nll, lengths, delays, n_scored):
    """What the device reports, restated with numpy in the kernels' own order.  nll (B, K, Ta) fp32 ->
    loss_per_codebook (K,): lane l of codebook q's wave adds its entries j = l, l + 64, .. of the flattened (b, t) one after the other
    (valid ones: t < Ta_b and t + d_q < n_scored), the 64 lanes are added pairwise at distance 1, 2, .., 32, the sum is divided by the
    count; loss: the K means added in codebook order, over K; nll_per_codebook (B, K): the same lane / butterfly scheme over clip b's
    t < Ta_b, over Ta_b; loss_per_clip (B,): those added in codebook order, over K."""
    f = np.float32
    B, K, Ta = nll.shape

    def butterfly(v):
        v = v.copy()
        for d in (1, 2, 4, 8, 16, 32):
            v = v + v[np.arange(64) ^ d]
        return v[0]

    lpc = np.zeros(K, f)
    for q in range(K):
        s, cnt = np.zeros(64, f), np.zeros(64, f)
        for j in range(B * Ta):
            b, t = divmod(j, Ta)
            if t < lengths[b] and t + delays[q] < n_scored:
                s[j % 64] += nll[b, q, t]
                cnt[j % 64] += f(1)
        lpc[q] = butterfly(s) / butterfly(cnt)
    loss = f(0)
    for q in range(K):
        loss = f(loss + lpc[q])
    loss = f(loss / f(K))
    pcb, clip = np.zeros((B, K), f), np.zeros(B, f)
    for b in range(B):
        tot = f(0)
        for q in range(K):
            s = np.zeros(64, f)
            for t in range(lengths[b]):
                s[t % 64] += nll[b, q, t]
            pcb[b, q] = butterfly(s) / f(lengths[b])
            tot = f(tot + pcb[b, q])
        clip[b] = f(tot / f(K))
    return lpc, loss, pcb, clip


def test_masked_means_restatement_agrees_with_plain_arithmetic():
    rng = np.random.default_rng(7)
    B, K, Ta = 3, 9, 70                               # more than 64 entries per clip: every lane, some twice
    lengths, delays = [70, 13, 2], [0, 2, 4, 6, 8, 10, 12, 14, 16]
    nll = (rng.random((B, K, Ta), dtype=np.float32) * 4 + 5).astype(np.float32)
    nll[1, :, 13:] = np.nan                           # behind a clip's end: never read
    nll[2, :, 2:] = np.nan
    lpc, loss, pcb, clip = masked_means(nll, lengths, delays, Ta + 16)
    valid = np.arange(Ta)[None, :] < np.asarray(lengths)[:, None]                     # (B, Ta)
    want_lpc = np.array([nll[:, q].astype(np.float64)[valid].mean() for q in range(K)])
    want_pcb = np.array([[nll[b, q, :lengths[b]].astype(np.float64).mean() for q in range(K)] for b in range(B)])
    # fp32 sums of at most 85 values near 7: a relative error of a few 2^-24 per addition
    assert np.abs(lpc - want_lpc).max() < 1e-5 and abs(loss - want_lpc.mean()) < 1e-5
    assert np.abs(pcb - want_pcb).max() < 1e-5 and np.abs(clip - want_pcb.mean(1)).max() < 1e-5
    assert np.isfinite(lpc).all() and np.isfinite(clip).all()
    # the pooled per-codebook mean is NOT the mean of the clips' means (the clips weigh by their lengths) ...
    assert np.abs(lpc - want_pcb.mean(0)).max() > 1e-3
    # ... and a scored range that ends early drops the delayed codebooks' tail: valid iff t + d_q < n_scored as well
    lpc_cut, _, _, _ = masked_means(nll, lengths, delays, 60)
    want_cut = np.array([nll[:, q].astype(np.float64)[valid & (np.arange(Ta)[None, :] + delays[q] < 60)].mean() for q in range(K)])
    assert np.abs(lpc_cut - want_cut).max() < 1e-5
    # every clip full: the same numbers as without lengths
    full = np.nan_to_num(nll, nan=6.0)
    a = masked_means(full, [Ta] * B, delays, Ta + 16)
    assert abs(a[1] - full.astype(np.float64).mean()) < 1e-5
