#!/usr/bin/env python
"""configs[1]'s decode workload (8 clips, cfg 6 -> 16 decoder rows, top-k 250 sampled, T = 220, the un-rounded synthetic
checkpoint, weight storage "auto") under the default delayed pattern (S = 229: 228 loop steps) and the parallel pattern
(ParallelPatternProvider, S = 221: 220 loop steps), alternating the two on ONE engine in one process.  Reports ms per batch of
generate_codes (condition MLP + pattern build + loop + revert; HIP events on the engine's stream) per pattern.

    python tools/time_patterns.py [rounds]
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaura_amd import synth  # noqa: E402
from vaura_amd.engine import DecoderEngine  # noqa: E402


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = torch.device("cuda:0")
    cfg = synth.FULL_SAMPLER
    eng = DecoderEngine(cfg, synth.sampler_state_dict(cfg, seed=0, round_bf16=False), dev)
    feats = synth.video_features(8, seed=0).to(dev)
    kw = dict(use_sampling=True, temp=1.0, top_k=250, cfg_scale=6.0, seed=1234, use_graph=True)
    patterns = {"delayed": None, "parallel": [0] * cfg.num_codebooks}
    stream = torch.cuda.Stream(dev)
    times = {k: [] for k in patterns}
    steps = {}
    with torch.cuda.stream(stream):
        for name, d in patterns.items():               # warm-up: graph capture of each shape
            eng.generate_codes(feats, 220, delays=d, **kw)
            torch.cuda.synchronize(dev)
            eng.check_status()
            steps[name] = eng.S - 1
        for _ in range(rounds):
            for name, d in patterns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                codes = eng.generate_codes(feats, 220, delays=d, **kw)
                b.record(stream)
                torch.cuda.synchronize(dev)
                eng.check_status()
                assert int(codes.min()) >= 0 and int(codes.max()) < 1024
                times[name].append(a.elapsed_time(b))
    for name in patterns:
        t = times[name]
        print(f"{name:9s} S-1 = {steps[name]} loop steps: {statistics.median(t):8.2f} ms / batch (median of {len(t)}; "
              f"min {min(t):.2f}, max {max(t):.2f}); {statistics.median(t) / steps[name] * 1e3:.1f} us / step")
    r = statistics.median(times["parallel"]) / statistics.median(times["delayed"])
    print(f"parallel / delayed: {r:.4f} (step-count ratio {steps['parallel'] / steps['delayed']:.4f})")


if __name__ == "__main__":
    main()
