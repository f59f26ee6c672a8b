"""Pure-Python restatement of what the library does with token log-probabilities after the sampler has written them (csrc/step.hip:
pattern_revert_kernel<float>, sequence_logprob_kernel, select_candidates_kernel; include/vaura_hip.h vaura_pattern_revert_*_f32 /
vaura_sequence_logprob[_clips | _starts] / vaura_select_candidates: per-clip lengths and first frames are the same functions applied
to clip b's slice [:, :, :T_b] with t0 = t0_b) — every fp32 operation in the order the kernels perform it, so that GPU results can be compared bit for bit.
tests/test_logprobs_host.py pins these functions against hand-made cases."""
import numpy as np

F32 = np.float32


def revert(seq_layout: np.ndarray, delays, T: int, fill=0.0) -> np.ndarray:
    """(B, K, S) in the layout of the pattern sequence -> (B, K, T): frame t of codebook q sits at step t + 1 + d_q."""
    B, K, S = seq_layout.shape
    out = np.full((B, K, T), fill, dtype=seq_layout.dtype)
    for q in range(K):
        for t in range(T):
            s = t + 1 + int(delays[q])
            if s < S:
                out[:, q, t] = seq_layout[:, q, s]
    return out


def wave_sum(v: np.ndarray) -> np.float32:
    """64 lane values added pairwise at distance 1, 2, 4, 8, 16, 32 (csrc/common.h wave_sum); fp32 addition commutes, so the tree of
    neighbouring pairs gives every lane's bits."""
    v = np.asarray(v, dtype=F32)
    assert v.shape == (64,)
    while v.size > 1:
        v = (v[0::2] + v[1::2]).astype(F32)
    return F32(v[0])


def codebook_mean(lp_row: np.ndarray, t0: int) -> np.float32:
    """Mean of one codebook's frames t0 .. T - 1: lane l adds frames t0 + l, t0 + l + 64, .. in that order starting from 0, the lanes
    are added by ``wave_sum``, the sum is divided by T - t0."""
    T = lp_row.shape[0]
    lanes = np.zeros(64, dtype=F32)
    for lane in range(64):
        acc = F32(0.0)
        for t in range(t0 + lane, T, 64):
            acc = F32(acc + F32(lp_row[t]))
        lanes[lane] = acc
    with np.errstate(invalid="ignore"):
        return F32(wave_sum(lanes) / F32(T - t0))


def sequence_logprob(lp: np.ndarray, t0: int = 0):
    """lp (B, K, T) fp32, prompt frames [0, t0) excluded -> (per_codebook (B, K), per_clip (B,)): per_clip = (sum of the K means in
    codebook order, from 0) / K.  A NaN anywhere in frames t0 .. of a clip makes per_clip and all K per_codebook values of it NaN."""
    B, K, T = lp.shape
    per_cb = np.zeros((B, K), dtype=F32)
    per_clip = np.zeros(B, dtype=F32)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            for q in range(K):
                per_cb[b, q] = codebook_mean(lp[b, q], t0)
            tot = F32(0.0)
            for q in range(K):
                tot = F32(tot + per_cb[b, q])
            tot = F32(tot / F32(K))
            per_clip[b] = tot
            if np.isnan(tot):
                per_cb[b, :] = tot
    return per_cb, per_clip


def select_candidates(scores: np.ndarray) -> np.ndarray:
    """scores (B, N) -> winner (B,): the largest score, the first index on a tie; a NaN never beats a number; all NaN -> 0."""
    B, N = scores.shape
    win = np.zeros(B, dtype=np.int64)
    for b in range(B):
        best, sb = 0, scores[b, 0]
        for j in range(1, N):
            sj = scores[b, j]
            if sj > sb or (np.isnan(sb) and not np.isnan(sj)):
                best, sb = j, sj
        win[b] = best
    return win
