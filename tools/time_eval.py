#!/usr/bin/env python
"""Teacher-forced scoring at configs[1]'s shape (Ta = 220, delayed pattern: S - 1 = 228 positions, the un-rounded synthetic checkpoint,
storage h2), B = 8 and 16 clips, no CFG branch.  Reports ms per batch and scored tokens / s (B * 9 * 220 per batch) of
  score      DecoderEngine.score: prefill chunks with the heads at every position + NLL + reduction (vaura_score)
  per_pos    the existing per-position route, Transformer.forward -> DecoderEngine.logits_all_positions (one decode step with
             heads per position)
  heads_nll  the heads + NLL share of `score`: score minus the same chunks without heads and NLL (vaura_generate_loop's prefill)
HIP events on one stream, median of `rounds`.

    python tools/time_eval.py [rounds] > profiles/eval_score_timing.txt
"""
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import synth  # noqa: E402
from vaura_amd.engine import DecoderEngine  # noqa: E402


def _time(stream, fn, rounds):
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = torch.device("cuda:0")
    cfg = synth.FULL_SAMPLER
    eng = DecoderEngine(cfg, synth.sampler_state_dict(cfg, seed=0, round_bf16=False), dev, wdtype="h2")
    Ta, K = 220, cfg.num_codebooks
    stream = torch.cuda.Stream(dev)
    rec = {"shape": {"Ta": Ta, "S_minus_1": Ta + K - 1, "storage": eng.wdtype, "prefill_positions": eng.PREFILL_POSITIONS}, "rows": []}
    with torch.cuda.stream(stream):
        for B in (8, 16):
            feats = synth.video_features(B, seed=0).to(dev)
            codes = torch.randint(0, 1024, (B, K, Ta), generator=torch.Generator().manual_seed(7)).to(dev)
            eng.score(codes, feats)                                          # warm-up (workspaces)
            score = _time(stream, lambda: eng.score(codes, feats, checked=False), rounds)
            n = eng.S - 1

            def prefill_only():                                               # the same chunks, no heads / NLL
                eng._reset_state()
                sp = eng._sampling(False, 1.0, 0, 0.0, 1.0, 0, 0)
                L.check(eng.lib.vaura_generate_loop(C.byref(eng.dec), C.byref(sp), n, 0, None, L.current_stream(dev)), "loop")
            eng.score(codes, feats)                                          # leaves seq / condition of this shape in place
            pre = _time(stream, prefill_only, rounds)
            # the per-position route Transformer.forward takes (one decode step with heads per position)
            idx = eng.seq[:, :, :n].to(torch.int64).clone()
            eng.logits_all_positions(idx, feats)                             # warm-up
            per = _time(stream, lambda: eng.logits_all_positions(idx, feats), max(1, rounds // 2))
            tok = B * K * Ta
            row = {"B": B, "score_ms": score[0], "score_min_ms": score[1], "score_max_ms": score[2],
                   "per_position_ms": per[0], "prefill_without_heads_ms": pre[0], "heads_nll_ms": score[0] - pre[0],
                   "heads_nll_share": (score[0] - pre[0]) / score[0], "speedup_vs_per_position": per[0] / score[0],
                   "score_tokens_per_s": tok / (score[0] * 1e-3), "per_position_tokens_per_s": tok / (per[0] * 1e-3)}
            rec["rows"].append(row)
            print(f"B={B:2d}: score {score[0]:8.2f} ms/batch ({row['score_tokens_per_s']:10.0f} tok/s)  per-position {per[0]:8.2f} ms "
                  f"({row['per_position_tokens_per_s']:9.0f} tok/s)  speed-up {row['speedup_vs_per_position']:.2f}x  heads+NLL "
                  f"{row['heads_nll_ms']:.2f} ms ({100 * row['heads_nll_share']:.1f} %)", flush=True)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
