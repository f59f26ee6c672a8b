#!/usr/bin/env python
"""Spectrogram at configs[1]'s batch: 8 clips of 2.56 s (8, 1, 112640) fp32 mono at 44.1 kHz -> (8, 220, 128) log-mel in dB, the default
format (n_fft 2048, hop 512: one column per codec frame).  Four routes:
  launch      vaura_spectrogram alone on a waveform already on the device: `inner` launches back to back between two HIP events
  call        post.audio_to_spectrogram (host checks, the record copy, the allocation and the launch), the same way
  torch_dev   the same picture with torch ops on the device: pad, torch.stft, |.|^2, a matmul with the dense filterbank, clamp, log10 —
              what a user can do today with torch alone (no per-clip lengths, no stream)
  torch_cpu   the same ops on the host with 16 threads, after the copy of the waveform (a host clock; the copy is inside)
then, on the tiny plugin model of the tests with the full-size synthetic codec (host clock, synchronised at the first block): the time
to the first block of stream_spectrogram(generate_stream(...)) against generate_stream alone in the same run, and the cost of
SpectrogramStream.push per block of a live session (host time of the call; device time between two events).
Warm-up, then the median of `rounds` (min and max kept).

    python tools/time_spectrogram.py [rounds] [out file, default profiles/spectrogram_timing.txt]
"""
import json
import os
import statistics
import sys
import time
import warnings

import torch
import torch.nn.functional as Fn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import post, synth  # noqa: E402
from vaura_amd import spectrogram as SG  # noqa: E402

B, COLS = 8, 220
N = COLS * 512
INNER = 50


def _events(stream, fn, rounds, inner):
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(inner):
            fn()
        b.record(stream)
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return statistics.median(ts), min(ts), max(ts)


def _host(fn, rounds):
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def torch_route(wav, fmt, win, fb, cols):
    """wav (B, 1, N) -> (B, cols, n_mels) in dB with torch ops on wav's device"""
    left = fmt.n_fft // 2 - fmt.hop // 2
    row = Fn.pad(wav[:, 0], (left, (cols - 1) * fmt.hop + fmt.n_fft - left - wav.shape[-1]))
    X = torch.stft(row, fmt.n_fft, hop_length=fmt.hop, window=win, center=False, return_complex=True)      # (B, bins, cols)
    P = X.real * X.real + X.imag * X.imag
    return 10.0 * torch.log10(torch.clamp(torch.matmul(fb, P), min=fmt.amin)).transpose(1, 2)


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
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "spectrogram_timing.txt")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    lines, rec = [], {"clips": B, "samples": N, "columns": COLS, "rounds": rounds, "launches_per_round": INNER}

    def say(line):
        print(line, flush=True)
        lines.append(line)

    fmt = post.SpectrogramFormat()
    lib = L.lib()
    say(f"{B} x {N} fp32 samples at 44.1 kHz -> {B} x {COLS} columns of {fmt.bins} mel bands in dB (n_fft {fmt.n_fft}, hop {fmt.hop}); "
        f"{B * COLS} workgroups of 256 threads, {lib.vaura_spectrogram_lds_bytes(fmt.n_fft, fmt.bins)} B of LDS each; "
        f"{(B * N * 4 + B * COLS * fmt.bins * 4) / 1e6:.2f} MB in and out; device {torch.cuda.get_device_name(0)}")
    host = torch.randn(B, 1, N, generator=torch.Generator().manual_seed(0)) * 0.3
    fb = SG.expand(fmt.mel, fmt.n_fft // 2 + 1)
    win_host = SG.window(fmt.n_fft)
    with torch.cuda.stream(stream):
        wav = host.to(dev)
        fb_dev, win_dev = fb.to(dev), win_host.to(dev)
        win, tw, bins, weights = post._spec_table(fmt, dev)
        records = torch.tensor([[0, N, 0, COLS, N]] * B, dtype=torch.int64, device=dev)
        out = torch.empty(B, COLS, fmt.bins, dtype=torch.float32, device=dev)
        st = L.current_stream(dev)

        def launch():
            L.check(lib.vaura_spectrogram(L.ptr(wav), B, N, L.ptr(records), 0, 0, 0, fmt.n_fft, fmt.hop, L.ptr(win), L.ptr(tw), L.ptr(bins),
                                          L.ptr(weights), weights.numel(), fmt.bins, SG.SCALES[fmt.scale], fmt.amin, L.ptr(out), COLS, st),
                    "vaura_spectrogram")

        def call():
            return post.audio_to_spectrogram(wav, fmt)

        def torch_dev():
            return torch_route(wav, fmt, win_dev, fb_dev, COLS)

        for _ in range(3):
            launch(), call(), torch_dev()
        torch.cuda.synchronize()
        got, ref = call()[0], torch_dev()
        launch()
        torch.cuda.synchronize()
        rec["launch_equals_call"] = bool(torch.equal(out, got))
        rec["max_abs_db_diff_to_torch_dev"] = float((got - ref).abs().max())
        for route, fn, inner in (("launch", launch, INNER), ("call", call, INNER), ("torch_dev", torch_dev, 10), ("launch_again", launch, INNER)):
            med, lo, hi = _events(stream, fn, rounds, inner)
            rec[route] = {"us": 1e3 * med, "min_us": 1e3 * lo, "max_us": 1e3 * hi}
            say(f"  {route:>12}: {1e3 * med:10.1f} us per batch (min {1e3 * lo:.1f}, max {1e3 * hi:.1f}; {rounds} rounds of {inner})")
    torch.set_num_threads(16)

    def torch_cpu():
        return torch_route(wav.cpu(), fmt, win_host, fb, COLS)
    torch_cpu()
    med, lo, hi = _host(torch_cpu, max(3, rounds // 4))
    rec["torch_cpu_16"] = {"us": 1e3 * med, "min_us": 1e3 * lo, "max_us": 1e3 * hi}
    say(f"  {'torch_cpu 16':>12}: {1e3 * med:10.1f} us per batch, copy included (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})")
    say(f"  torch on the device / launch: {rec['torch_dev']['us'] / rec['launch']['us']:.2f}x; torch on the device / call: "
        f"{rec['torch_dev']['us'] / rec['call']['us']:.2f}x; launch == call: {rec['launch_equals_call']}; max |call - torch_dev| "
        f"{rec['max_abs_db_diff_to_torch_dev']:.3e} dB")

    # time to the first block, with and without the spectrogram step; the per-push cost on the blocks of a live session
    from vaura_amd.model import VAURAModel
    cfg = synth.tiny_sampler(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VAURAModel(
            feature_extractor_config={"target": "vaura_amd.feature_extractor.MotionFormer"},
            audio_encoder_config={"target": "vaura_amd.codec.DacModelWrapper", "params": {"model_sr": 44100, "synthetic": True}},
            sampler_config={"target": "vaura_amd.sampler.Transformer", "params": cfg.yaml_params()},
            visual_bridge_config={"target": "torch.nn.Identity"},
            pattern_provider_config={"target": "vaura_amd.patterns.DelayedPatternProvider", "params": {"n_q": 9}},
            flatten_vis_feats=True, freeze_feature_extractor=True, noise_mode="philox")
    m.sampler.load_state_dict(synth.sampler_state_dict(cfg, seed=0), strict=True)
    m.sampler.audio_tokens_per_video_frame = 7
    m = m.to(dev)
    frames = synth.video_features(2, tokens=32, seed=31).reshape(2, 1, 32, 768).to(dev)
    kw = dict(frames=frames, max_new_tokens=128, prompt_is_encoded=True, use_sampling=False, cfg_scale=1.0, block_frames=16)
    plain = lambda: m.generate_stream(**kw)                               # noqa: E731
    with_spec = lambda: post.stream_spectrogram(m.generate_stream(**kw), fmt)      # noqa: E731
    for _ in range(2):
        first_block_ms(plain, 1), first_block_ms(with_spec, 1)
    for name, make in (("generate_stream", plain), ("stream_spectrogram(generate_stream)", with_spec), ("generate_stream again", plain)):
        med, lo, hi = first_block_ms(make, max(5, rounds // 2))
        rec[name] = {"first_block_ms": med, "min_ms": lo, "max_ms": hi}
        say(f"  first block of {name:>36}: {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}); tiny model, 2 clips, 128 frames, block_frames 16")

    feats = synth.video_features(2, tokens=6 * 8, seed=71).reshape(2, 6, 8, 768).to(dev)
    session = m.open_live(2, block_frames=16, use_sampling=False, cfg_scale=1.0)
    blocks = []
    for i in range(6):
        blocks += session.push(features=feats[:, i])
    blocks += session.close()
    torch.cuda.synchronize()
    host_us, dev_us = [], []
    for r in range(max(5, rounds // 2) + 1):
        sp = post.SpectrogramStream(fmt, 2, dev)
        for blk in blocks:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            sp.push(blk["audio"], final=bool(blk["final"]))
            b.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if r:                                                         # the first pass warms the pinned ring and the tables
                host_us.append(1e6 * (t1 - t0))
                dev_us.append(1e3 * a.elapsed_time(b))
    rec["live_push"] = {"blocks": len(blocks), "host_us": statistics.median(host_us), "host_max_us": max(host_us),
                        "device_us": statistics.median(dev_us), "device_max_us": max(dev_us)}
    say(f"  SpectrogramStream.push per block of a live session ({len(blocks)} blocks of up to 16 frames, 2 clips, tiny model): host "
        f"{rec['live_push']['host_us']:.1f} us per call (max {max(host_us):.1f}), device {rec['live_push']['device_us']:.1f} us between two "
        f"events around it (max {max(dev_us):.1f}): the record copy and the launch")
    say(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("# spectrogram timing (tools/time_spectrogram.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
