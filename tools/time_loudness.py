#!/usr/bin/env python
"""Streaming loudness (csrc/loudness.hip), all in one run on the full-size model's batch: 8 clips, cfg 6, storage h1.
  one pass   post.measure_loudness (the parallel fp64 K-weighting, the meter) on 8 x 2.56 s and 8 x 30.72 s and on ONE clip of
             30.72 s, against vaura_audio_loudness (the one-thread-per-clip recursion and its gain launch) called directly on the
             same tensors with preallocated buffers, and against post.normalize_audio(strategy="loudness") around it: device time
             between two HIP events, `inner` calls back to back; post.normalize_loudness_causal (meter + gains applied) the same way
  streamed   the time to the first block's samples of generate_stream(block_frames=16) with and without stream_loudness (host clock,
             synchronised at the first block), and LoudnessStream.push per block of a live session (host time of the call; device time
             between two events)
Warm-up, then the median of `rounds` (min and max kept).

    python tools/time_loudness.py [rounds] [out file, default profiles/loudness_stream_timing.txt]
"""
import json
import os
import statistics
import sys
import time
import warnings

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import post, synth  # noqa: E402

B = 8
RATE = 44100


def _events(fn, rounds, inner):
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return statistics.median(ts), min(ts), max(ts)


def first_block_ms(make, rounds):
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it = make()
        blk = next(it)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
        for _ in it:                                                      # run the call to its end: the model is free again
            pass
        del blk
    return statistics.median(ts), min(ts), max(ts)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "loudness_stream_timing.txt")
    dev = torch.device("cuda:0")
    lines, rec = [], {"clips": B, "rounds": rounds}

    def say(line):
        print(line, flush=True)
        lines.append(line)

    lib = L.lib()
    target = post.LoudnessTarget()
    say(f"one workgroup of 256 threads per clip, {lib.vaura_audio_loudness_lds_bytes(RATE)} B of LDS; step {target.plan.step}, chunks of "
        f"{target.plan.L} samples")
    for name, clips, frames in (("8 x 2.56 s", B, 220), ("8 x 30.72 s", B, 2640), ("1 x 30.72 s", 1, 2640)):
        n = frames * 512
        wav = (torch.randn(clips, 1, n, generator=torch.Generator().manual_seed(0)) * 0.2).to(dev)
        inner = 20 if frames == 220 else 3

        p_out = torch.empty_like(wav)
        p_scratch = torch.empty(lib.vaura_audio_loudness_scratch_elems(clips), dtype=torch.float32, device=dev)
        st = L.current_stream(dev)

        def parent():                                                    # the C entry alone: its two launches, nothing allocated
            L.check(lib.vaura_audio_loudness(L.ptr(wav), L.ptr(p_out), clips, n, RATE, 12.0, 0, 2e-3, L.ptr(p_scratch), st),
                    "vaura_audio_loudness")

        def parent_call():
            return post.normalize_audio(wav, strategy="loudness", sample_rate=RATE)

        def meter():
            return post.measure_loudness(wav, sample_rate=RATE)

        def causal():
            return post.normalize_loudness_causal(wav, target)

        for _ in range(2):
            parent(), parent_call(), meter(), causal()
        torch.cuda.synchronize()
        got = meter()["integrated"]
        lk = -12.0 - 20.0 * torch.log10(parent_call().loudness_gains.double())
        diff = float((got.double() - lk).abs().max())
        r = {}
        for route, fn in (("parent", parent), ("parent_call", parent_call), ("meter", meter), ("causal", causal), ("parent_again", parent)):
            med, lo, hi = _events(fn, rounds, inner)
            r[route] = {"us": 1e3 * med, "min_us": 1e3 * lo, "max_us": 1e3 * hi}
        rec[name] = dict(r, max_abs_lkfs_diff=diff)
        say(f"  {name:>12}: vaura_audio_loudness alone (the serial kernel and its gain launch, buffers preallocated) {r['parent']['us']:9.1f} us (min "
            f"{r['parent']['min_us']:.1f}, max {r['parent']['max_us']:.1f}; again {r['parent_again']['us']:.1f}); normalize_audio(strategy=\"loudness\") "
            f"{r['parent_call']['us']:9.1f} us; measure_loudness {r['meter']['us']:9.1f} us (min {r['meter']['min_us']:.1f}, max "
            f"{r['meter']['max_us']:.1f}): {r['parent']['us'] / r['meter']['us']:.2f}x the entry alone; normalize_loudness_causal "
            f"{r['causal']['us']:9.1f} us; largest |LKFS difference| {diff:.2e} dB ({rounds} rounds of {inner})")

    # time to the first block with and without the loudness step; the per-push cost on the blocks of a live session
    from vaura_amd.model import VAURAModel
    cfg = synth.FULL_SAMPLER
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VAURAModel(
            feature_extractor_config={"target": "vaura_amd.feature_extractor.MotionFormer"},
            audio_encoder_config={"target": "vaura_amd.codec.DacModelWrapper", "params": {"model_sr": 44100, "synthetic": True}},
            sampler_config={"target": "vaura_amd.sampler.Transformer", "params": cfg.yaml_params()},
            visual_bridge_config={"target": "torch.nn.Identity"},
            pattern_provider_config={"target": "vaura_amd.patterns.DelayedPatternProvider", "params": {"n_q": 9}},
            flatten_vis_feats=True, freeze_feature_extractor=True, noise_mode="philox", seed=1234)
    m.sampler.load_state_dict(synth.sampler_state_dict(cfg, seed=0, round_bf16=True), strict=True)
    m.sampler.audio_tokens_per_video_frame = 7
    m = m.to(dev)
    frames = synth.video_features(B, 4 * 8, seed=0).reshape(B, 4, 8, cfg.cond_in).to(dev)
    kw = dict(frames=frames, max_new_tokens=220, prompt_is_encoded=True, use_sampling=True, temp=1.0, top_k=128, cfg_scale=6.0, block_frames=16)
    plain = lambda: m.generate_stream(**kw)                               # noqa: E731
    with_loud = lambda: post.stream_loudness(m.generate_stream(**kw), target)      # noqa: E731
    for _ in range(2):
        first_block_ms(plain, 1), first_block_ms(with_loud, 1)
    for name, make in (("generate_stream", plain), ("stream_loudness(generate_stream)", with_loud), ("generate_stream again", plain)):
        med, lo, hi = first_block_ms(make, max(3, rounds // 2))
        rec[name] = {"first_block_ms": med, "min_ms": lo, "max_ms": hi}
        say(f"  first block of {name:>34}: {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}); full-size model, {B} clips, cfg 6, 220 frames, "
            f"block_frames 16")

    feats = synth.video_features(B, tokens=6 * 8, seed=71).reshape(B, 6, 8, cfg.cond_in).to(dev)
    session = m.open_live(B, block_frames=16, use_sampling=True, temp=1.0, top_k=128, cfg_scale=6.0)
    blocks = []
    for i in range(6):
        blocks += session.push(features=feats[:, i])
    blocks += session.close()
    torch.cuda.synchronize()
    host_us, dev_us = [], []
    for r in range(max(3, rounds // 2) + 1):
        ls = post.LoudnessStream(target, B, dev)
        for blk in blocks:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            ls.push(blk["audio"], final=bool(blk["final"]))
            b.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if r:                                                         # the first pass warms the pinned ring and the table
                host_us.append(1e6 * (t1 - t0))
                dev_us.append(1e3 * a.elapsed_time(b))
    rec["live_push"] = {"blocks": len(blocks), "host_us": statistics.median(host_us), "host_max_us": max(host_us),
                        "device_us": statistics.median(dev_us), "device_max_us": max(dev_us)}
    say(f"  LoudnessStream.push per block of a live session ({len(blocks)} blocks of up to 16 frames, {B} clips, full-size model): host "
        f"{rec['live_push']['host_us']:.1f} us per call (max {max(host_us):.1f}), device {rec['live_push']['device_us']:.1f} us between two "
        f"events around it (max {max(dev_us):.1f}): the record copy, the allocations and the launch")
    say(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("# streaming loudness timing (tools/time_loudness.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
