"""Goldens of the teacher-forced evaluation path — the reference's own ``VAURAModel.forward`` + ``_compute_loss`` (build container only).

    python tests/golden/make_golden_eval.py small   # eval_tiny.npz: 2-layer model, B=3, Ta=20, delayed / parallel / even delays (seconds)
    python tests/golden/make_golden_eval.py full    # eval_full_raw_B2_T220.npz: 24 layers, un-rounded checkpoint (seed 0), B=2, Ta=220

The reference's ``DacModelWrapper.encode`` is a placeholder here (the ``dac`` package is absent): the model's audio encoder is given
an ``encode`` that returns recorded codes, so ``forward(frames, audio)`` scores exactly those codes.  ``model.pattern`` is reset before
every call (the reference caches the first call's pattern).  Recorded per code set: the reverted logits at a few timesteps only (the
whole (B, 9, Ta, 1024) tensor would not fit a fixture), ``nll`` (restated from the reference's full logits with F.cross_entropy,
reduction none), the mask, and ``loss`` / ``loss_per_codebook`` as ``_compute_loss`` returns them.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the repository on sys.path)
import make_golden_patterns as mp  # noqa: E402
import ref_harness as rh  # noqa: E402
from vaura_amd import synth  # noqa: E402

TINY_SETS = {"delayed": list(range(9)), "parallel": [0] * 9, "even": list(range(0, 18, 2))}
TINY_KEEP_T = (0, 19)
FULL_KEEP_T = (0, 1, 110, 219)


def _score(model, codes, frames, keep_t):
    """The reference's forward + _compute_loss on recorded codes; nll restated from the full reverted logits."""
    model.audio_encoder.encode = lambda audio: codes
    model.pattern = None
    with torch.no_grad():
        logits, mask, target = model.forward(frames, torch.zeros(codes.shape[0], 1, 512 * codes.shape[-1]))
        loss, lpc = model._compute_loss(logits, target[:, :9, :], mask)
        nll = F.cross_entropy(logits.permute(0, 3, 1, 2), target[:, :9, :], reduction="none")
    return dict(logits=logits[:, :, list(keep_t)].numpy().astype(np.float32), mask=mask.numpy(), nll=nll.numpy().astype(np.float32),
                loss=np.float32(loss.item()), loss_per_codebook=np.array([x.item() for x in lpc], dtype=np.float32),
                codes=codes.numpy().astype(np.int16))


def gold_eval_tiny():
    cfg = synth.tiny_sampler(2)
    sd = synth.sampler_state_dict(cfg, seed=3)
    model = rh.build_reference_model(cfg.yaml_params(), sd)
    B, Ta = 3, 20
    feats = synth.video_features(B, seed=5)
    frames = feats.reshape(B, 4, 8, 768)
    codes = torch.randint(0, 1024, (B, 9, Ta), generator=torch.Generator().manual_seed(61))
    out = {"layers": np.int64(2), "weight_seed": np.int64(3), "feat_seed": np.int64(5), "codes_seed": np.int64(61),
           "keep_t": np.array(TINY_KEEP_T, dtype=np.int64)}
    for name, delays in TINY_SETS.items():
        mp._set_pattern(model, delays)
        r = _score(model, codes, frames, TINY_KEEP_T)
        out[name + "_delays"] = np.array(delays, dtype=np.int64)
        for k, v in r.items():
            out[f"{name}_{k}"] = v
        print(f"{name}: loss {r['loss']:.6f}")
    mg.save("eval_tiny.npz", **out)


def gold_eval_full():
    """Delayed pattern (the shipped one), 24 layers on the un-rounded checkpoint: the greedy tokens of full_greedy_raw_B2_T220.npz under
    that run's condition (feat seed 0), and seeded uniform codes."""
    model = mg._full_model(round_bf16=False)
    B, Ta = 2, 220
    frames = synth.video_features(B, seed=0).reshape(B, 4, 8, 768)
    greedy = torch.from_numpy(np.load(os.path.join(HERE, "full_greedy_raw_B2_T220.npz"))["tokens"].astype(np.int64))
    uniform = torch.randint(0, 1024, (B, 9, Ta), generator=torch.Generator().manual_seed(62))
    out = {"weight_seed": np.int64(0), "feat_seed": np.int64(0), "round_bf16": np.int64(0), "uniform_seed": np.int64(62),
           "keep_t": np.array(FULL_KEEP_T, dtype=np.int64)}
    for name, codes in (("greedy", greedy), ("uniform", uniform)):
        r = _score(model, codes, frames, FULL_KEEP_T)
        for k, v in r.items():
            if name == "greedy" and k == "codes":
                continue                  # the fixture it came from holds them
            out[f"{name}_{k}"] = v
        print(f"{name}: loss {r['loss']:.6f}")
    mg.save("eval_full_raw_B2_T220.npz", **out)


if __name__ == "__main__":
    torch.set_float32_matmul_precision("highest")
    what = sys.argv[1] if len(sys.argv) > 1 else "small"
    if what == "small":
        gold_eval_tiny()
    elif what == "full":
        gold_eval_full()
    else:
        raise SystemExit(f"unknown target {what}")
