#!/usr/bin/env python
"""The codec on a batch of clips of different lengths: ONE packed pass (CodecEngine.decode_clips / CodecEncoderEngine.encode_clips)
against the grouped route — decode() / encode() once per distinct length on the clips of that length, gathered and scattered into the
padded result, which is what VAURAModel.generate / _encode_clips did before.  Full-size synthetic codec, default precision (f16pair),
three batches each way:
  mixed16    16 clips, lengths 220 / 165 / 110 / 55 frames, four of each     (4 grouped passes at batch 4)
  distinct8   8 clips of eight distinct lengths from 55 to 220 frames         (8 grouped passes at batch 1: real data)
  equal8      8 clips of 220 frames against the plain batched decode() / encode(): what the packing itself costs
Encode takes the same batches in samples (frames * 512 - 37: no length is a multiple of the hop).  The routes of a batch are taken in
turn within every round (whatever else shares the machine hits both alike), `reps` calls per timed window between two HIP events on one
stream, median / min / max over the rounds of the time per call.  Both routes give the same bits, checked here before anything is timed.

    python tools/time_codec_clips.py [rounds] > profiles/codec_clips_timing.txt
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaura_amd import synth  # noqa: E402
from vaura_amd.engine import CodecEncoderEngine, CodecEngine  # noqa: E402

REPS = 5
BATCHES = {
    "mixed16": [t for t in (220, 165, 110, 55) for _ in range(4)],
    "distinct8": [55, 79, 102, 126, 149, 173, 196, 220],
    "equal8": [220] * 8,
}


def grouped_decode(eng, codes, lengths):
    hop = eng.cfg.hop
    wav = torch.zeros(codes.shape[0], 1, codes.shape[-1] * hop, device=codes.device)
    for t in sorted(set(lengths)):
        idx = torch.tensor([b for b, n in enumerate(lengths) if n == t], device=codes.device)
        wav[idx, :, :t * hop] = eng.decode(codes[idx][..., :t])
    return wav


def grouped_encode(enc, wav, n, hop):
    out = torch.zeros(wav.shape[0], enc.cfg.n_codebooks, -(-max(n) // hop), dtype=torch.int64, device=wav.device)
    for n_b in sorted(set(n)):
        idx = torch.tensor([b for b, v in enumerate(n) if v == n_b], device=wav.device)
        c = enc.encode(wav[idx][..., :n_b])
        out[idx, :, :c.shape[-1]] = c
    return out


def measure(stream, routes, rounds):
    outs = {k: fn() for k, fn in routes.items()}                       # warm-up: workspaces of every shape, code objects
    torch.cuda.synchronize()
    ref = next(iter(outs.values()))
    assert all(torch.equal(ref, o) for o in outs.values()), "the routes disagree"
    ts = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(REPS):
                fn()
            b.record(stream)
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) / REPS)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ts.items()}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    dev = torch.device("cuda:0")
    cfg = synth.FULL_CODEC
    sd = dict(synth.codec_state_dict(cfg, seed=0))
    sd.update(synth.codec_encoder_state_dict(cfg, seed=0))
    eng, enc = CodecEngine(cfg, sd, dev), CodecEncoderEngine(cfg, sd, dev)
    hop = cfg.hop
    stream = torch.cuda.Stream(dev)
    rec = {"precision": "f16pair", "rounds": rounds, "reps": REPS, "decode": {}, "encode": {}}
    with torch.cuda.stream(stream):
        for name, lengths in BATCHES.items():
            g = torch.Generator().manual_seed(7)
            codes = torch.randint(0, cfg.codebook_size, (len(lengths), cfg.n_codebooks, max(lengths)), generator=g).to(dev)
            n = [t * hop - 37 for t in lengths]
            wav = (torch.randn(len(n), 1, max(n), generator=g) * 0.3).to(dev)
            other = "plain" if name == "equal8" else "grouped"
            dec = {"one_pass": lambda: eng.decode_clips(codes, lengths),
                   other: (lambda: eng.decode(codes)) if name == "equal8" else (lambda: grouped_decode(eng, codes, lengths))}
            encr = {"one_pass": lambda: enc.encode_clips(wav, n),
                    other: (lambda: enc.encode(wav)) if name == "equal8" else (lambda: grouped_encode(enc, wav, n, hop))}
            for side, routes in (("decode", dec), ("encode", encr)):
                r = measure(stream, routes, rounds)
                r["lengths"] = lengths if side == "decode" else n
                r["ratio_other_over_one_pass"] = r[other]["median_ms"] / r["one_pass"]["median_ms"]
                rec[side][name] = r
                print(f"{side} {name:10s} one pass {r['one_pass']['median_ms']:8.3f} ms (min {r['one_pass']['min_ms']:.3f}, max {r['one_pass']['max_ms']:.3f})   "
                      f"{other:7s} {r[other]['median_ms']:8.3f} ms (min {r[other]['min_ms']:.3f}, max {r[other]['max_ms']:.3f})   "
                      f"{other} / one pass = {r['ratio_other_over_one_pass']:.3f}", flush=True)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
