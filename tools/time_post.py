#!/usr/bin/env python
"""The post stage on a ragged batch: ONE lengthed call (post.normalize_audio(wav, lengths=..) -> vaura_audio_*_clips) against the B
one-clip calls it replaces (slice each clip out, post.normalize_audio on it -> vaura_audio_normalize / vaura_audio_loudness).

8 clips of 8 distinct lengths in rows of 220 frames x 512 samples (2.55 s at 44.1 kHz, the bench's clip), strategies 'rms' and
'loudness'.  Both forms run on one side stream, alternating, after a warm-up of each; per form the median over the rounds of the
device time between two events on that stream (it includes the gaps the host leaves between launches: allocations, the slices, the
read-back of the lengths) and of the host's wall time around the same work ending in a synchronise.  The outputs of the two forms
are compared (bit equality over each clip's own samples) before anything is timed.

    python tools/time_post.py [rounds]
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaura_amd import post  # noqa: E402

SR = 44100
FRAMES = [220, 197, 173, 150, 126, 101, 77, 52]
HOP = 512


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    dev = torch.device("cuda:0")
    n = max(FRAMES) * HOP
    lens = [f * HOP for f in FRAMES]
    g = torch.Generator().manual_seed(0)
    wav = (0.1 * torch.randn(len(lens), 1, n, generator=g)).to(dev)
    for b, nb in enumerate(lens):
        wav[b, :, nb:] = 0.0
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    print(f"{len(lens)} clips, rows of {n} samples, lengths {lens}; {rounds} rounds, the forms alternating")
    for kw in (dict(strategy="rms"), dict(strategy="loudness", sample_rate=SR)):
        forms = {
            "one lengthed call (list)": lambda: post.normalize_audio(wav, lengths=lens, **kw),
            "one lengthed call (int32 on the device)": lambda: post.normalize_audio(wav, lengths=lens_dev, **kw),
            "8 one-clip calls": lambda: [post.normalize_audio(wav[b:b + 1, :, :nb].contiguous(), **kw) for b, nb in enumerate(lens)],
        }
        dev_ms = {k: [] for k in forms}
        wall_ms = {k: [] for k in forms}
        with torch.cuda.stream(stream):
            one = forms["one lengthed call (list)"]()
            many = forms["8 one-clip calls"]()
            torch.cuda.synchronize(dev)
            for b, nb in enumerate(lens):
                assert torch.equal(one[b:b + 1, :, :nb], many[b]) and bool((one[b, :, nb:] == 0).all()), b
            for _ in range(3):                              # warm-up of every form
                for f in forms.values():
                    f()
            torch.cuda.synchronize(dev)
            for _ in range(rounds):
                for name, f in forms.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    a.record(stream)
                    f()
                    b.record(stream)
                    torch.cuda.synchronize(dev)
                    wall_ms[name].append((time.perf_counter() - t0) * 1e3)
                    dev_ms[name].append(a.elapsed_time(b))
        print(f"strategy '{kw['strategy']}':")
        for name in forms:
            d, w = dev_ms[name], wall_ms[name]
            print(f"  {name:40s} events {statistics.median(d):8.3f} ms (min {min(d):.3f}, max {max(d):.3f})   "
                  f"wall {statistics.median(w):8.3f} ms (min {min(w):.3f}, max {max(w):.3f})")
        r = statistics.median(wall_ms["one lengthed call (list)"]) / statistics.median(wall_ms["8 one-clip calls"])
        print(f"  one lengthed call / 8 one-clip calls (wall medians): {r:.3f}")


if __name__ == "__main__":
    main()
