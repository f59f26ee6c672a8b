"""Cost of the attention maps on the decode loop: generate_codes(return_attention_weights=True) against the same call without the flag,
in ONE session, alternating.  The full-size synthetic sampler (24 layers), BASELINE configs[1]: 8 clips of 2.56 s (T = 220 frames, S =
229: 228 sampled steps), cfg 6 (16 decoder rows), top-k 128, Philox noise, default engine (auto storage), the captured step graph.

Per form: device-event time of `rounds` calls after a warm-up call of each (the loop and, with the flag, the buffer's zero fill and the
attention_map launch behind it), median / min / max.  The unflagged call is timed twice — before any flagged call has run and
interleaved with the flagged ones — so that the file shows whether the flag leaves anything behind; its kernels are the parent
commit's, byte for byte (profiles/attention_maps_device_code.txt).
    python tools/time_attention_maps.py [rounds] [out]        -> profiles/attention_maps_timing.txt"""
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vaura_amd import synth  # noqa: E402
from vaura_amd.engine import DecoderEngine  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "attention_maps_timing.txt")
DEV = "cuda:0"
B, T = 8, 220
KW = dict(use_sampling=True, temp=1.0, top_k=128, cfg_scale=6.0, seed=1234)

cfg = synth.FULL_SAMPLER
eng = DecoderEngine(cfg, synth.sampler_state_dict(cfg, seed=0, round_bf16=True), DEV)
feats = synth.video_features(B, 32, seed=0).to(DEV)


def timed(**kw):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    r = eng.generate_codes(feats, T, **KW, **kw)
    b.record()
    torch.cuda.synchronize()
    eng.check_status()
    return a.elapsed_time(b), r


def stats(v):
    return f"median {statistics.median(v):8.2f} ms   min {min(v):8.2f}   max {max(v):8.2f}   ({len(v)} calls)"


forms = {"mean, last layer": dict(return_attention_weights=True), "all heads, last layer": dict(return_attention_weights=True, attention_heads="all"),
         "mean, layer 0": dict(return_attention_weights=True, attention_layer=0)}
_, plain = timed()                                    # warm-up: builds the step graph
before = [timed()[0] for _ in range(ROUNDS)]          # no flagged call has run yet
times = {k: [] for k in ["no flag", *forms]}
for k, kw in forms.items():                           # warm-up of each form (its graph, its buffer)
    _, (codes, extra) = timed(**kw)
    assert torch.equal(codes, plain), k
shape = tuple(eng.attn_probs.shape)
for _ in range(ROUNDS):
    times["no flag"].append(timed()[0])
    for k, kw in forms.items():
        ms, (codes, extra) = timed(**kw)
        times[k].append(ms)
        assert torch.equal(codes, plain), k
base = statistics.median(times["no flag"])
lines = [
    "# Attention maps on the decode loop (tools/time_attention_maps.py): generate_codes() of BASELINE configs[1] — full-size sampler, 8 clips,",
    f"# T = {T} (228 sampled steps), cfg 6 (16 rows), top-k 128, Philox, storage {eng.wdtype}, step graph — with and without",
    "# return_attention_weights, alternating in one session; device events around the whole call.",
    f"# reported buffer: {shape} fp32 = {4 * eng.attn_probs.numel() / 1e6:.1f} MB, zeroed per call; map (8, 228, 228) fp32",
    f"no flag, before any flagged call   {stats(before)}",
    f"no flag, between flagged calls     {stats(times['no flag'])}",
]
for k in forms:
    d = statistics.median(times[k]) - base
    lines.append(f"{k:34s} {stats(times[k])}   + {d:6.2f} ms ({100 * d / base:+.1f} %) over the unflagged median")
spread = max(times["no flag"] + before) - min(times["no flag"] + before)
lines.append(f"# run-to-run spread of the unflagged call in this session: {spread:.2f} ms ({100 * spread / base:.1f} %); the two unflagged medians "
             f"differ by {abs(statistics.median(before) - base):.2f} ms")
print("\n".join(lines))
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
