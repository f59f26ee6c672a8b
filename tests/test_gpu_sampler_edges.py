"""csrc/step.hip sample_kernel on the adversarial rows of tests/sampler_edges_reference.py: shared top-k thresholds, radix-select byte
structure, the top-p order among ties, the strict top-p cut on its boundary, first-index ties of the greedy argmax, and the near-tie
detector's positive direction.  The rows of one parameter set share one launch; every launch goes through vaura_sample (scalars) and
vaura_sample_clips (records equal to the scalars), and the tokens EQUAL the expected ones — which tests/test_sampler_edges_host.py
has shown to be the reference's, with margins that leave fp32 rounding no say.

Rows that already are probabilities (groups 2 and 4, the dyadic row of 3) have one entry point only: vaura_sample_clips refuses
input_is_probs (include/vaura_hip.h), and that refusal is what the second call asserts there.

The documented order among equal probabilities under top-p, "lower id first", is the kernel's own; the reference project's
torch.sort(descending=True) defines none, so on rows with such ties the kernel is held to its contract, not to the oracle."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_edges_reference as E  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import synth  # noqa: E402

DEV = "cuda:0"
V = E.V
NEAR_TIE = 4             # VAURA_STATUS_NEAR_TIE


def stream():
    return L.current_stream(torch.device(DEV))


def sampling(p: E.Params, tie_eps: float = 0.0):
    return L.Sampling(int(p.use_sampling), p.temp, p.top_k, p.top_p, p.cfg_scale, 11, 0, int(p.input_is_probs), tie_eps)


def records(p: E.Params, B: int) -> torch.Tensor:
    one = struct.pack("<ififf3i", int(p.use_sampling), p.temp, p.top_k, p.top_p, p.cfg_scale, 0, 0, 0)
    return torch.frombuffer(bytearray(one * B), dtype=torch.int32).view(B, 8).to(DEV)


def run(p: E.Params, rows: torch.Tensor, noise: torch.Tensor, B: int, K: int, per_clip: bool):
    """one standalone launch -> (rc, tokens (B, K) on the CPU; -1 where nothing was written)"""
    rows_d, noise_d = rows.to(DEV), noise.to(DEV)
    tok = torch.full((B, K), -1, dtype=torch.int32, device=DEV)
    sp = sampling(p)
    if per_clip:
        rec = records(p, B)
        rc = L.lib().vaura_sample_clips(L.ptr(rows_d), B, K, V, C.byref(sp), L.ptr(rec), L.ptr(noise_d), 0, L.ptr(tok), None, 0, 0, None,
                                        stream())
    else:
        rc = L.lib().vaura_sample(L.ptr(rows_d), B, K, V, C.byref(sp), L.ptr(noise_d), 0, L.ptr(tok), stream())
    torch.cuda.synchronize()
    return rc, tok.cpu()


def check_launches(cases):
    n = 0
    for launch in E.launches(cases):
        p = launch[0].params
        rows, noise, expect = E.pack(launch)
        B, K = expect.shape
        for per_clip in (False, True):
            rc, tok = run(p, rows, noise, B, K, per_clip)
            if per_clip and p.input_is_probs:
                assert rc == -1 and bool((tok == -1).all()), launch[0].id       # VAURA_ERR_ARG, nothing launched
                continue
            assert rc == 0, (launch[0].id, per_clip)
            got, want = tok.flatten().tolist(), expect.flatten().tolist()
            wrong = [(c.id, g, w) for c, g, w in zip(launch, got, want) if g != w]
            assert not wrong, (f"{len(wrong)} of {len(launch)} rows", "records" if per_clip else "scalars", wrong[:8])
            assert got == want                                                   # (the padding rows as well)
        n += 1
    return n


def test_top_k_threshold_shared_by_several_tokens():
    """group 1: every token that ties with the k-th largest is kept ("p >= threshold"), the one 0.5 below is not; k = 2000 is k = V"""
    assert check_launches(E.topk_threshold_rows()) == 16


def test_radix_select_byte_structure():
    """group 2: keys that differ in one byte only / in random bits / in nothing, the k-th rank on the first and the last element of a
    histogram bin and inside a tie group"""
    assert check_launches(E.radix_rows()) == 12


def test_top_p_order_among_ties():
    """group 3: the bitonic network orders equal probabilities by id — the token at rank r is the stable sort's"""
    assert check_launches(E.topp_order_rows()) == 4


def test_top_p_cut_on_its_boundary():
    """group 4: cs - p == top_p is kept, the next rank is dropped; top_p = 1 drops nothing"""
    assert check_launches(E.topp_cut_rows()) == 5


@pytest.mark.parametrize("cfg_scale", [1.0, 6.0])
def test_greedy_first_index_ties(cfg_scale):
    """group 5: the lowest id among equal maxima, within a thread, a wave and across waves; with cfg_scale = 6 the tie exists only
    after the mix"""
    assert check_launches(E.greedy_rows(cfg_scale)) == 1


def test_golden_tie_rows_in_full(golden):
    """tests/golden/sampling.npz under top-p, ALL 27 rows against the stable reference — the two rows with exact ties included, which
    the comparison with the recorded tokens has to leave out"""
    g = golden("sampling.npz")
    logits = torch.from_numpy(g["logits"])
    noise = synth.exp_noise(1, 27, V, int(g["noise_seed"]))[0].contiguous()
    for name, top_k, top_p in E.GOLDEN_TOP_P:
        for temp in (1.0, 0.7):
            p = E.Params(True, temp, top_k, top_p)
            want = E.next_token(logits, use_sampling=True, temp=temp, top_k=top_k, top_p=top_p, noise=noise)[..., 0].int()
            keep = np.ones((3, 9), dtype=bool)
            for b, k in E.GOLDEN_TIE_ROWS:
                keep[b, k] = False
            assert np.array_equal(want.numpy()[keep], g[f"{name}_t{temp}_tok"][..., 0][keep])
            for per_clip in (False, True):
                rc, tok = run(p, logits, noise, 3, 9, per_clip)
                assert rc == 0 and torch.equal(tok, want), (name, temp, per_clip, torch.nonzero(tok != want).tolist())


@pytest.mark.parametrize("per_clip", [False, True], ids=["scalars", "records"])
def test_exact_ties_raise_the_near_tie_status(per_clip):
    """group 6, positive direction only: vaura_sample_seq with tie_eps = 2^-22 on launches whose every decision is an exact tie — the
    greedy rows, without and with the mix, and the k = 1 rows whose draw is a tie.  Every used slot counts once, the status bit is
    raised, the first flagged step is this one, and the tokens are the ones of the launches without the detector."""
    T, pos, step = 6, 3, 0
    for launch in E.near_tie_rows():
        p = launch[0].params
        rows, noise, expect = E.pack(launch)
        B, K = expect.shape
        delays = [0] * K                                     # slot pos + 1 holds timestep pos of every codebook: free and valid
        S = T + 1
        seq = torch.full((B, K, S), -1, dtype=torch.int32, device=DEV)
        seq[:, :, :pos + 1] = 5
        state = torch.zeros(8, dtype=torch.int32, device=DEV)
        state[0], state[2] = pos, step
        rows_d, noise_d = rows.to(DEV), noise.to(DEV)
        rec = records(p, B) if per_clip else None
        sp = sampling(p, E.TIE_EPS)
        rc = L.lib().vaura_sample_seq(L.ptr(rows_d), B, K, V, C.byref(sp), L.ptr(rec), L.ptr(noise_d), L.ptr(seq), T, S, L.ptr(state),
                                      L.delays_host(delays), None, None, None, None, stream())
        torch.cuda.synchronize()
        assert rc == 0, launch[0].id
        st = state.cpu().tolist()
        assert torch.equal(seq[:, :, pos + 1].cpu(), expect), launch[0].id
        assert st[4] & NEAR_TIE and st[6] == B * K and st[7] == step + 1, (launch[0].id, st)
        assert st[0] == pos + 1 and st[2] == step + 1 and not st[4] & ~NEAR_TIE, (launch[0].id, st)
