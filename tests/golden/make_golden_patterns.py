"""Goldens for delay patterns other than the default 0..K-1, made by running the REAL reference (build container only).

    python tests/golden/make_golden_patterns.py small    # pattern bookkeeping + a 2-layer model with delays 0,2,..,16 (seconds)
    python tests/golden/make_golden_patterns.py full     # 24-layer model, parallel pattern, B=2, T=220: greedy cfg 1 and
                                                         # cfg 6 top-k 250 sampled, un-rounded checkpoint (~7 min)

The reference model is built by ``ref_harness.build_reference_model`` (DelayedPatternProvider(9) by default); the pattern provider
is then swapped for the reference's own ``ParallelPatternProvider(9)`` / ``DelayedPatternProvider(9, delays=...)`` and
``sampler.codebook_pattern`` is set to match, which is what instantiating the model from ``parallel_9cbs.yaml`` does.
Inputs are regenerated from the seeds each fixture records (``vaura_amd.synth``), as in make_golden.py.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the repository on sys.path)
import ref_harness as rh  # noqa: E402
from vaura_amd import synth  # noqa: E402

DELAY_SETS = {"parallel": [0] * 9, "d011": [0] + [1] * 8, "even": list(range(0, 18, 2)), "unit": list(range(9))}
TINY_DELAYS = list(range(0, 18, 2))


def _provider(delays):
    rh.install()
    from models.modules.misc.codebook_patterns import DelayedPatternProvider, ParallelPatternProvider
    if delays == [0] * len(delays):
        return ParallelPatternProvider(len(delays))
    return DelayedPatternProvider(len(delays), delays=list(delays))


def _set_pattern(model, delays):
    model.pattern_provider = _provider(delays)
    model.sampler.codebook_pattern = model.pattern_provider.__class__.__name__
    return model


# ------------------------------------------------------------------------------------- pattern bookkeeping
def gold_patterns_delays():
    out = {}
    for name, delays in DELAY_SETS.items():
        prov = _provider(delays)
        out[name + "_delays"] = np.array(delays, dtype=np.int64)
        for T, Tp in [(4, 0), (20, 8), (55, 0), (220, 0), (221, 166)]:
            pat = prov.get_pattern(T)
            g = torch.Generator().manual_seed(300 + T)
            codes = torch.full((2, 9, T), -1, dtype=torch.long)
            if Tp:
                codes[..., :Tp] = torch.randint(0, 1024, (2, 9, Tp), generator=g)
            seq, idx, mask = pat.build_pattern_sequence(codes, 1024)
            filled = torch.where(seq == -1, torch.randint(0, 1024, seq.shape, generator=g), seq)
            filled = torch.where(mask[None], filled, torch.full_like(filled, 1024))
            rev, ridx, rmask = pat.revert_pattern_sequence(filled, special_token=-1)
            k = f"{name}_T{T}_p{Tp}"
            out[k + "_codes"] = codes.numpy().astype(np.int16)
            out[k + "_seq"] = seq.numpy().astype(np.int16)
            out[k + "_idx"] = idx.numpy().astype(np.int32)
            out[k + "_mask"] = mask.numpy()
            out[k + "_filled"] = filled.numpy().astype(np.int16)
            out[k + "_rev"] = rev.numpy().astype(np.int16)
            out[k + "_ridx"] = ridx.numpy().astype(np.int32)
            out[k + "_rmask"] = rmask.numpy()
            out[k + "_first"] = np.int64(pat.get_first_step_with_timesteps(Tp))
    out["sha1"] = np.array(mg.sha1(np.concatenate([out[k].reshape(-1).astype(np.int64) for k in sorted(out)])))
    mg.save("patterns_delays.npz", **out)


# ------------------------------------------------------------------------------------- tiny model, delays 0,2,..,16
def gold_tiny_delays():
    """2-layer model (the tiny_model.npz weights), delays 0,2,..,16 (S = T + 17), T=60 with a 40-frame prompt: greedy cfg 1 and
    top-k 250 cfg 6 sampled with the reference's noise stream."""
    cfg = synth.tiny_sampler(2)
    sd = synth.sampler_state_dict(cfg, seed=3)
    model = _set_pattern(rh.build_reference_model(cfg.yaml_params(), sd), TINY_DELAYS)
    B, T, Tp = 2, 60, 40
    feats = synth.video_features(B, seed=5)
    frames = feats.reshape(B, 4, 8, 768)
    prompt = torch.randint(0, 1024, (B, 9, Tp), generator=torch.Generator().manual_seed(41))
    out = {"layers": np.int64(2), "weight_seed": np.int64(3), "feat_seed": np.int64(5), "prompt_seed": np.int64(41),
           "delays": np.array(TINY_DELAYS, dtype=np.int64), "T": np.int64(T), "prompt": prompt.numpy().astype(np.int16)}
    r = model.generate(frames=frames, audio=prompt, max_new_tokens=T, return_sampled_indices=True, use_sampling=False,
                       prompt_is_encoded=True, cfg_scale=1.0, remove_prompts=False)
    out["greedy"] = r["sampled_indices"].numpy().astype(np.int16)
    torch.manual_seed(77)
    r = model.generate(frames=frames, audio=prompt, max_new_tokens=T, return_sampled_indices=True, use_sampling=True, temp=1.0,
                       top_k=250, top_p=0.0, prompt_is_encoded=True, cfg_scale=6.0, remove_prompts=False)
    out["topk250_cfg6"] = r["sampled_indices"].numpy().astype(np.int16)
    out["noise_seed"] = np.int64(77)
    out["sha1"] = np.array(mg.sha1(np.concatenate([out["greedy"], out["topk250_cfg6"]])))
    mg.save("tiny_delays_even.npz", **out)


# ------------------------------------------------------------------------------------- full depth, parallel pattern
def _run(model, name, delays, B, cfg_scale, use_sampling, top_k, noise_seed, keep, T=220, feat_seed=0):
    """make_golden._cfg_run for any delay pattern (one pass per sequence step up to T + max(d) + 1) and for cfg 1: every step's
    last-position logits captured; recorded per step, clip and codebook: the decision margin (greedy: top-1 - top-2 of the
    (mixed) logits; top-k sampled: the relative margin of argmax(p / Exp(1)) over the kept set) and, sampled, the relative
    gap at the top-k threshold."""
    feats = synth.video_features(B, seed=feat_seed)
    store = []
    h = mg._capture_logits(model, store)
    if use_sampling:
        torch.manual_seed(noise_seed)
    t = time.time()
    r = model.generate(frames=feats.reshape(B, 4, 8, 768), audio=None, max_new_tokens=T, return_sampled_indices=True,
                       use_sampling=use_sampling, temp=1.0, top_k=top_k, top_p=0.0, prompt_is_encoded=True, cfg_scale=cfg_scale)
    dt = time.time() - t
    h.remove()
    tok = r["sampled_indices"].numpy()
    S = T + max(delays) + 1
    assert [L for (L, _) in store] == list(range(1 + delays[0], S)), "one pass per sequence step"
    noise = synth.exp_noise(len(store), B * 9, 1024, noise_seed) if use_sampling else None
    margins, thr_gap = [], []
    for i, (L, lg) in enumerate(store):
        if cfg_scale > 1.0:
            assert lg.shape[0] == 2 * B
            c, u = lg[:B], lg[B:]
            mixed = u + (c - u) * cfg_scale                               # vaura_model.py:810-813
        else:
            mixed = lg
        if not use_sampling:
            top2 = torch.topk(mixed, 2, dim=-1).values
            margins.append((top2[..., 0] - top2[..., 1]).numpy())
            continue
        p = torch.softmax(mixed, -1)
        srt = torch.sort(p, dim=-1, descending=True).values
        thr = srt[..., top_k - 1:top_k]
        thr_gap.append(((srt[..., top_k - 1] - srt[..., top_k]) / srt[..., top_k - 1]).numpy())
        kept = torch.where(p >= thr, p, torch.zeros_like(p))
        ratio = kept / noise[i].reshape(B, 9, 1024)
        top2 = torch.topk(ratio, 2, dim=-1).values
        margins.append(((top2[..., 0] - top2[..., 1]) / top2[..., 0]).numpy())
    extra = {}
    if use_sampling:
        extra = dict(noise_seed=np.int64(noise_seed), threshold_rel_gap=np.stack(thr_gap).astype(np.float32))
    logits = {L: lg for (L, lg) in store}
    mg.save(name, tokens=tok.astype(np.int16), sha1=np.array(mg.sha1(tok.astype(np.int16))), delays=np.array(delays, dtype=np.int64),
            margins=np.stack(margins).astype(np.float32), logits_steps=np.array(keep),
            logits=np.stack([logits[L].numpy() for L in keep]), cfg_scale=np.float64(cfg_scale), top_k=np.int64(top_k),
            ref_seconds=np.float64(dt), weight_seed=np.int64(0), feat_seed=np.int64(feat_seed), round_bf16=np.int64(0), **extra)
    print(f"reference generate(): {dt:.1f}s  min margin {np.stack(margins).min():.3e}")


def gold_full_parallel():
    model = _set_pattern(mg._full_model(round_bf16=False), [0] * 9)
    keep = (1, 2, 100, 219, 220)
    _run(model, "full_parallel_greedy_raw_B2_T220.npz", [0] * 9, 2, 1.0, False, 0, 0, keep)
    _run(model, "full_parallel_topk250_cfg6_raw_B2_T220.npz", [0] * 9, 2, 6.0, True, 250, 2028, keep)


if __name__ == "__main__":
    torch.set_float32_matmul_precision("highest")
    what = sys.argv[1] if len(sys.argv) > 1 else "small"
    if what == "small":
        gold_patterns_delays(); gold_tiny_delays()
    elif what == "full":
        gold_full_parallel()
    else:
        raise SystemExit(f"unknown target {what}")
