"""fp64 restatement of the video relevance the sampler reports in its third mode (csrc/step.hip sample_kernel<PC, true, SampleRelevance>,
include/vaura_hip.h vaura_decoder_ext.logprobs_cond / logprobs_null, vaura_sample_relevance), of the rule for what is stored where, and
— imported from tests/logprob_reference.py, the same kernels serve — of the fixed-order means and the selection rule.

For the token ``tok`` that the workgroup of (clip, codebook) chose, from the conditional row x_c and the null row x_u of the same prefix:

    lc = (x_c[tok] - max x_c) - log(sum exp(x_c - max x_c))
    lu = (x_u[tok] - max x_u) - log(sum exp(x_u - max x_u))          relevance r = lc - lu

over the full vocabulary of 1024, temperature 1, no CFG mix and no top-k / top-p cut.  Reduction order of the kernel, per row, the one
its mode-1 greedy branch uses: thread t of 256 owns candidates 4t .. 4t+3; MAXIMUM = its four values, then the wave's 64 threads, then
the four waves as max(max(w0, w1), max(w2, w3)); SUM = (e0 + e1) + (e2 + e3) per thread of e_j = exp(x_j - maximum), then the wave's
butterfly (neighbours at distance 1, 2, 4, .., 32), then the four waves as ((w0 + w1) + w2) + w3.  ``row_logprob`` follows that order
in fp64 (where the order moves the result by ~1e-16: it is restated, not needed); tests/test_relevance_host.py pins it against a plain
``torch.log_softmax`` in fp64."""
import numpy as np

from logprob_reference import F32, codebook_mean, revert, select_candidates, sequence_logprob, wave_sum  # noqa: F401  (re-exported)

V = 1024
THREADS = 256


def _tree(v: np.ndarray) -> float:
    """64 lane values added pairwise at distance 1, 2, .., 32 (the wave butterfly), in the dtype given"""
    while v.size > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def row_logprob(x: np.ndarray, tok: int) -> float:
    """log softmax(x)[tok] of one 1024-logit row in fp64, in the kernel's reduction order (block max, then block sum)."""
    x = np.asarray(x, dtype=np.float64).reshape(THREADS, 4)
    mt = np.maximum(np.maximum(x[:, 0], x[:, 1]), np.maximum(x[:, 2], x[:, 3]))           # thread
    mw = mt.reshape(4, 64).max(axis=1)                                                     # wave (max is order-free)
    m = max(max(mw[0], mw[1]), max(mw[2], mw[3]))                                          # the four waves
    e = np.exp(x - m)
    st = (e[:, 0] + e[:, 1]) + (e[:, 2] + e[:, 3])                                         # thread
    sw = [_tree(st[64 * w:64 * w + 64].copy()) for w in range(4)]                          # wave butterfly
    den = ((sw[0] + sw[1]) + sw[2]) + sw[3]                                                # the four waves
    return float((x.reshape(-1)[tok] - m) - np.log(den))


def token_relevance(x_c: np.ndarray, x_u: np.ndarray, tok: int):
    """(lc, lu) of the chosen token from the two rows; NaN in both when either row holds a non-finite value (the sampler raises
    VAURA_STATUS_NONFINITE_LOGITS for such a decision)."""
    if not (np.isfinite(x_c).all() and np.isfinite(x_u).all()):
        return float("nan"), float("nan")
    return row_logprob(x_c, tok), row_logprob(x_u, tok)


def stored(slot_before: int, t: int, T: int, value: float) -> float:
    """What the (batch, K, S) buffers hold at a slot after the step that decides it: the value only where the kernel writes a SAMPLED
    token — the slot held -1 (unknown) and its timestep t = s - 1 - d_q is a real one, 0 <= t < T; prompt / known tokens (slot >= 0) and
    special slots (t outside [0, T)) keep the 0 the host put there."""
    return value if (slot_before == -1 and 0 <= t < T) else 0.0


def sequence_relevance(lc: np.ndarray, lu: np.ndarray, t0: int = 0):
    """lc, lu (B, K, T) fp32 -> (r (B, K, T), per_codebook (B, K), per_clip (B,)): r = lc - lu is ONE fp32 subtraction per slot, the means
    are those of ``logprob_reference.sequence_logprob`` applied to r (fixed order: two runs give the same bits)."""
    with np.errstate(invalid="ignore"):
        r = (np.asarray(lc, dtype=F32) - np.asarray(lu, dtype=F32)).astype(F32)
    pcb, clip = sequence_logprob(r, t0)
    return r, pcb, clip
