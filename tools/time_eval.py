#!/usr/bin/env python
"""Teacher-forced scoring at configs[1]'s shape (Ta = 220, delayed pattern: S - 1 = 228 positions, the un-rounded synthetic checkpoint,
storage h2), B = 8 and 16 clips, no CFG branch.  Reports ms per batch and scored tokens / s (B * 9 * 220 per batch) of
  score      DecoderEngine.score: prefill chunks with the heads at every position + NLL + reduction (vaura_score)
  per_pos    the existing per-position route, Transformer.forward -> DecoderEngine.logits_all_positions (one decode step with
             heads per position)
  heads_nll  the heads + NLL share of `score`: score minus the same chunks without heads and NLL (vaura_generate_loop's prefill)
HIP events on one stream, median of `rounds`.

    python tools/time_eval.py [rounds] > profiles/eval_score_timing.txt

Per-clip mode (``--clips``): 16 clips, Ta = 220, h2, the four routes taken in turn within every round (alternating: whatever else
shares the machine hits all of them alike), median / min / max over the rounds of
  a  score()                                          one length
  b  score_clips, every length 220                    the per-clip kernels on the same schedule: expected = a within a's spread
  c  score_clips, lengths 220 / 165 / 110 / 55 (four clips each) in one call
  d  the same clips as one score() call per distinct length (4 clips each): the only route without score_clips.  Two figures: on
     ONE engine, which re-prepares its workspaces for every new shape (d_one_engine), and on four engines that each keep their shape
     (d_prepared: the weights four times in memory, nothing re-prepared — the floor of this route)

    python tools/time_eval.py --clips [rounds] > profiles/eval_score_clips_timing.txt
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


def _stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def clips_mode(rounds):
    dev = torch.device("cuda:0")
    cfg = synth.FULL_SAMPLER
    sd = synth.sampler_state_dict(cfg, seed=0, round_bf16=False)
    B, Ta, K = 16, 220, cfg.num_codebooks
    distinct = [220, 165, 110, 55]
    lengths = [t for t in distinct for _ in range(B // len(distinct))]
    eng = DecoderEngine(cfg, sd, dev, wdtype="h2")
    per_len = [DecoderEngine(cfg, sd, dev, wdtype="h2") for _ in distinct]
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        feats = synth.video_features(B, seed=0).to(dev)
        codes = torch.randint(0, 1024, (B, K, Ta), generator=torch.Generator().manual_seed(7)).to(dev)
        groups = [(codes[i * 4:i * 4 + 4, :, :t].contiguous(), feats[i * 4:i * 4 + 4].contiguous()) for i, t in enumerate(distinct)]
        routes = {
            "a_score": lambda: eng.score(codes, feats, checked=False),
            "b_score_clips_equal": lambda: eng.score_clips(codes, feats, [Ta] * B, checked=False),
            "c_score_clips_mixed": lambda: eng.score_clips(codes, feats, lengths, checked=False),
            "d_one_engine": lambda: [eng.score(c, f, checked=False) for c, f in groups],
            "d_prepared": lambda: [e.score(c, f, checked=False) for e, (c, f) in zip(per_len, groups)],
        }
        for fn in routes.values():                                            # warm-up (workspaces of every shape)
            fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in routes}
        for _ in range(rounds):
            for k, fn in routes.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                torch.cuda.synchronize()
                ts[k].append(a.elapsed_time(b))
    rec = {"shape": {"B": B, "Ta": Ta, "storage": eng.wdtype, "lengths": lengths, "rounds": rounds}, "routes": {k: _stats(v) for k, v in ts.items()}}
    for k, v in rec["routes"].items():
        print(f"{k:22s} median {v['median_ms']:8.2f} ms   min {v['min_ms']:8.2f}   max {v['max_ms']:8.2f}", flush=True)
    m = {k: v["median_ms"] for k, v in rec["routes"].items()}
    print(f"b / a = {m['b_score_clips_equal'] / m['a_score']:.4f}   d_one_engine / c = {m['d_one_engine'] / m['c_score_clips_mixed']:.3f}   "
          f"d_prepared / c = {m['d_prepared'] / m['c_score_clips_mixed']:.3f}")
    print(json.dumps(rec))


def main():
    if "--clips" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--clips"]
        return clips_mode(int(rest[0]) if rest else 9)
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
