"""CPU-side checks (-m "not gpu") of delay patterns other than the default 0..K-1 (codebook_patterns.py:374-419): host metadata
against the reference's own values (tests/golden/patterns_delays.npz, tests/golden/make_golden_patterns.py), the checkpoint remap
of the reference's ParallelPatternProvider, refusals on the host, and the C ABI's new descriptor fields and argument checks
(answered without a GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch
import yaml

from vaura_amd import _lib as L
from vaura_amd import synth
from vaura_amd.patterns import DelayedPatternProvider, ParallelPatternProvider

SETS = ("parallel", "d011", "even", "unit")
SHAPES = ((4, 0), (20, 8), (55, 0), (220, 0), (221, 166))


@pytest.mark.parametrize("name", SETS)
def test_pattern_metadata_matches_reference(golden, name):
    g = golden("patterns_delays.npz")
    delays = [int(x) for x in g[name + "_delays"]]
    prov = ParallelPatternProvider(9) if name == "parallel" else DelayedPatternProvider(9, delays=delays)
    assert prov.delays == delays
    for T, Tp in SHAPES:
        k = f"{name}_T{T}_p{Tp}"
        pat = prov.get_pattern(T)
        S = g[k + "_seq"].shape[-1]
        assert pat.seq_steps == S == T + max(delays) + 1
        idx, mask = pat._build_indexes(T, "cpu")
        assert np.array_equal(idx.numpy(), g[k + "_idx"]) and np.array_equal(mask.numpy(), g[k + "_mask"]), k
        ridx, rmask = pat._revert_indexes(S, "cpu")
        assert np.array_equal(ridx.numpy(), g[k + "_ridx"]) and np.array_equal(rmask.numpy(), g[k + "_rmask"]), k
        assert pat.get_first_step_with_timesteps(Tp) == int(g[k + "_first"]) == Tp + 1 + delays[0], k


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from ckpt_fixture import write_checkpoint
    d = tmp_path_factory.mktemp("ckpt_parallel")
    ckpt, hp, _ = write_checkpoint(str(d), synth.tiny_sampler(2))
    with open(hp) as f:
        h = yaml.safe_load(f)
    # configs/modules/codebook_patterns/parallel_9cbs.yaml, as a training run's hparams.yaml names it
    h["pattern_provider_config"] = {"target": "models.modules.misc.codebook_patterns.ParallelPatternProvider", "params": {"n_q": 9}}
    hp_par = str(d / "hparams_parallel.yaml")
    with open(hp_par, "w") as f:
        yaml.safe_dump(h, f)
    return ckpt, hp_par


@pytest.fixture(scope="module")
def parallel_model(checkpoint):
    from vaura_amd.model import VAURAModel
    ckpt, hp = checkpoint
    return VAURAModel.load_from_checkpoint(ckpt, hparams_file=hp, map_location="cpu")


def test_checkpoint_naming_the_reference_parallel_provider_is_remapped(parallel_model):
    m = parallel_model
    assert type(m.pattern_provider) is ParallelPatternProvider
    assert m.pattern_provider.delays == [0] * 9
    assert m._pattern_delays(220) == [0] * 9
    pat = m.pattern_provider.get_pattern(220)
    assert pat.seq_steps == 221 and pat.get_first_step_with_timesteps(0) == 1


def test_host_refuses_what_the_loop_cannot_decode(parallel_model):
    m = parallel_model
    frames = torch.zeros(1, 4, 8, 768)
    # unsorted / negative delays: the provider itself (as the reference's asserts), and the kernels' argument check
    with pytest.raises(AssertionError):
        DelayedPatternProvider(9, delays=[0, 2, 1, 3, 4, 5, 6, 7, 8])
    for bad in ([0, 2, 1, 3, 4, 5, 6, 7, 8], [-1, 0, 0, 0, 0, 0, 0, 0, 0], [0] * 8):
        with pytest.raises(L.VauraHipError):
            L.check_delays(bad, 9)
    with pytest.raises(L.VauraHipError, match="16 codebooks"):
        L.check_delays([0] * 17, 17)
    # S = T + max(d) + 1 beyond the model's block_size (256): refused before any device work
    old = m.pattern_provider
    try:
        m.pattern_provider = DelayedPatternProvider(9, delays=list(range(0, 18, 2)))
        with pytest.raises(L.VauraHipError, match="block_size"):
            m.generate_tokens(frames=frames, max_new_tokens=240, prompt_is_encoded=True)

        # a provider whose pattern is not a pure delay pattern (the reference's Unrolled / VALLE / MusicLM kind): refused, not
        # decoded in another layout
        class UnrolledPatternProvider:
            def get_pattern(self, timesteps):
                return object()
        m.pattern_provider = UnrolledPatternProvider()
        with pytest.raises(L.VauraHipError, match="not a delay pattern"):
            m.generate_tokens(frames=frames, max_new_tokens=20, prompt_is_encoded=True)
    finally:
        m.pattern_provider = old


def test_decoder_descriptor_carries_the_delays():
    lib = L.lib()
    assert C.sizeof(L.Decoder) == lib.vaura_struct_size(3)
    assert L.Decoder.has_pattern_delays.offset == L.Decoder.ws_sync.offset + C.sizeof(C.c_void_p)   # appended after the last field
    assert L.Decoder.pattern_delays.offset == L.Decoder.has_pattern_delays.offset + 4
    d = L.Decoder()
    assert d.has_pattern_delays == 0 and list(d.pattern_delays) == [0] * 16          # zero-filled = the default pattern
    assert lib.vaura_struct_size(2) == 48                                            # vaura_sampling did not grow


def _fake_decoder(T, S, delays=None, K=9):
    d = L.Decoder()
    d.dims = L.Dims(24, 1536, 16, 4096, K, 1024, 512, 1024, 768, 8, 7, 1e-5)
    d.wdtype, d.batch, d.rows, d.max_len, d.timesteps, d.seq_len, d.n_cond_tokens = L.W_BF16, 2, 2, 256, T, S, 32
    lw = (L.LayerWeights * 24)()
    d._lw = lw
    d.layers_host = C.cast(lw, C.POINTER(L.LayerWeights))
    for name, typ in L.Decoder._fields_:
        if typ is C.c_void_p and name != "noise":
            setattr(d, name, 0x1000)        # never dereferenced: every call below fails on its arguments first
    if delays is not None:
        d.has_pattern_delays = 1
        for q, x in enumerate(delays):
            d.pattern_delays[q] = x
    return d


def test_decoder_checks_the_delays_without_a_gpu():
    lib = L.lib()
    sp = L.Sampling(0, 1.0, 0, 0.0, 1.0, 0, 0)

    def loop(d, n_prefill, n_steps):
        return lib.vaura_generate_loop(C.byref(d), C.byref(sp), n_prefill, n_steps, None, None)
    # parallel pattern: S = T + 1; the loop may not feed more than S - 1 positions
    assert loop(_fake_decoder(220, 221, [0] * 9), 0, 221) == -1
    # seq_len that does not match timesteps + max(d) + 1: VAURA_ERR_SHAPE
    assert loop(_fake_decoder(220, 229, [0] * 9), 0, 1) == -2
    assert loop(_fake_decoder(220, 221), 0, 1) == -2                      # zero-filled: d_q = q, S must be T + K
    assert loop(_fake_decoder(200, 217, list(range(0, 18, 2))), 0, 217) == -1
    # unsorted, negative, more than 16 codebooks, a flag other than 0 / 1: VAURA_ERR_ARG
    assert loop(_fake_decoder(220, 229, [0, 1, 2, 3, 4, 5, 6, 8, 7]), 0, 1) == -1
    assert loop(_fake_decoder(220, 221, [-1, 0, 0, 0, 0, 0, 0, 0, 0]), 0, 1) == -1
    assert loop(_fake_decoder(220, 221, [0] * 16, K=17), 0, 1) == -1
    d = _fake_decoder(220, 221, [0] * 9)
    d.has_pattern_delays = 2
    assert loop(d, 0, 1) == -1
    # S beyond the K/V capacity
    d = _fake_decoder(300, 301, [0] * 9)
    assert loop(d, 0, 1) == -1
    assert lib.vaura_decode_step(C.byref(_fake_decoder(220, 229, [0] * 9)), C.byref(sp), 1, None) == -2


def test_pattern_entry_points_check_their_arguments_without_a_gpu():
    lib = L.lib()
    build, revert = lib.vaura_pattern_build_delays, lib.vaura_pattern_revert_delays
    par, even = L.delays_host([0] * 9), L.delays_host(list(range(0, 18, 2)))
    P = 0x1000                                # never dereferenced: every call below fails on its arguments first
    assert build(0, 0, 1, 9, 4, 5, 1024, par, None) == -1                # null pointers
    assert revert(0, 0, 1, 9, 4, 5, -1, par, None) == -1
    assert build(P, P, 1, 9, 4, 5, 1024, None, None) == -1               # no delays
    assert revert(P, P, 1, 9, 4, 5, -1, None, None) == -1
    assert build(P, P, 1, 9, 4, 13, 1024, par, None) == -2               # S != T + max(d) + 1
    assert build(P, P, 1, 9, 4, 20, 1024, even, None) == -2
    assert revert(P, P, 1, 9, 4, 6, -1, par, None) == -2                 # longer than the pattern
    assert build(P, P, 1, 9, 4, 5, 1024, L.delays_host([0, 1, 0, 0, 0, 0, 0, 0, 0]), None) == -1     # unsorted
    assert revert(P, P, 1, 9, 4, 5, -1, L.delays_host([-1, 0, 0, 0, 0, 0, 0, 0, 0]), None) == -1   # negative
    assert build(P, P, 1, 17, 4, 5, 1024, L.delays_host([0] * 17), None) == -1                     # K > 16
    assert build(P, P, 0, 9, 4, 5, 1024, par, None) == -1 and revert(P, P, 1, 9, 0, 5, -1, par, None) == -1
