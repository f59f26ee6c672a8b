#!/usr/bin/env python
"""Audio output at configs[1]'s batch: 8 clips of 2.56 s (8, 1, 112896) fp32 mono at 44.1 kHz -> 48 kHz stereo int16, interleaved.
Four routes:
  launch      vaura_audio_output alone on a waveform already on the device: `inner` launches back to back between two HIP events
  call        post.audio_to_pcm (host checks, the record copy, the allocations and the launch), the same way
  torch_dev   the same arithmetic with torch ops on the device: torchaudio's strided conv1d over the full-form kernel, the gain, round,
              clamp, the cast and the channel copy — what a user can do today with torch alone
  torch_cpu   the same ops on the host with 16 threads, after the copy of the waveform (a host clock; the copy is inside)
and the time to the first PCM of stream_pcm(generate_stream(...)) against the first block of generate_stream alone, in the same run,
on the tiny plugin model of the tests with the full-size synthetic codec (host clock, synchronised at the first block).
Warm-up, then the median of `rounds` (min and max kept).  Bytes: the waveform read once plus the PCM written, over the launch time,
against the 6.29 TB/s copy rate measured on this part.

    python tools/time_audio_out.py [rounds] [out file, default profiles/audio_out_timing.txt]
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

COPY_RATE = 6.29e12
B, N, RATE = 8, 112896, 48000
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


def torch_route(wav, tab, full, n_out):
    """wav (B, 1, N) -> (B, n_out, 2) int16 with torch ops on wav's device"""
    o, w = tab["o"], tab["w"]
    y = Fn.conv1d(Fn.pad(wav, (w, w + o)), full, stride=o)              # (B, n, frames)
    y = y.transpose(1, 2).reshape(wav.shape[0], -1)[:, :n_out]
    q = torch.round(y * 32768.0).clamp(-32768, 32767).to(torch.int16)
    return q[:, :, None].expand(-1, -1, 2).contiguous()


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
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "audio_out_timing.txt")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    lines, rec = [], {"clips": B, "samples": N, "rate": RATE, "rounds": rounds, "launches_per_round": INNER}

    def say(line):
        print(line, flush=True)
        lines.append(line)

    fmt = post.PcmFormat(rate=RATE, dtype=torch.int16, channels=2, interleaved=True)
    pl, tab = fmt.plan, fmt.plan.table
    n_out = pl.output_total(N)
    host = torch.rand(B, 1, N, generator=torch.Generator().manual_seed(0)) * 1.6 - 0.8
    bytes_moved = B * N * 4 + B * n_out * 2 * 2
    say(f"{B} x {N} fp32 samples at 44.1 kHz -> {B} x {n_out} stereo int16 frames at {RATE} Hz; {pl.n} phases of {pl.T} taps, history "
        f"{pl.history()}; {bytes_moved / 1e6:.2f} MB moved, {B * -(-n_out // 1024)} workgroups")
    first64 = tab["first"].to(torch.int64)
    full = torch.zeros(pl.n, 2 * pl.w + pl.o + pl.T, dtype=torch.float32)
    full.scatter_(1, first64[:, None] + torch.arange(pl.T)[None, :], tab["weights"])
    full = full[:, None, :2 * pl.w + pl.o].contiguous()
    with torch.cuda.stream(stream):
        wav = host.to(dev)
        full_dev = full.to(dev)
        first, taps = post._pcm_table(pl, dev)
        records = torch.tensor([[0, N, 0, n_out, N]] * B, dtype=torch.int64, device=dev)
        gain = torch.ones(B, device=dev)
        out = torch.empty(B, n_out, 2, dtype=torch.int16, device=dev)
        clipped = torch.zeros(B, dtype=torch.int32, device=dev)
        lib, st = L.lib(), L.current_stream(dev)

        def launch():
            L.check(lib.vaura_audio_output(L.ptr(wav), B, N, L.ptr(records), 0, 0, 0, pl.o, pl.n, pl.w, L.ptr(first), L.ptr(taps), pl.n, pl.T,
                                           L.ptr(gain), 0, 1, 2, L.ptr(out), n_out, L.ptr(clipped), st), "vaura_audio_output")

        def call():
            return post.audio_to_pcm(wav, fmt)

        def torch_dev():
            return torch_route(wav, tab, full_dev, n_out)

        for _ in range(3):
            launch(), call(), torch_dev()
        torch.cuda.synchronize()
        got, ref = call()[0], torch_dev()
        launch()
        torch.cuda.synchronize()
        rec["launch_equals_call"] = bool(torch.equal(out, got))
        rec["max_abs_lsb_diff_to_torch_dev"] = int((got.to(torch.int32) - ref.to(torch.int32)).abs().max())
        for route, fn, inner in (("launch", launch, INNER), ("call", call, INNER), ("torch_dev", torch_dev, 5), ("launch_again", launch, INNER)):
            med, lo, hi = _events(stream, fn, rounds, inner)
            rec[route] = {"us": 1e3 * med, "min_us": 1e3 * lo, "max_us": 1e3 * hi}
            line = f"  {route:>12}: {1e3 * med:10.1f} us per batch (min {1e3 * lo:.1f}, max {1e3 * hi:.1f}; {rounds} rounds of {inner})"
            if route.startswith("launch"):
                line += f"  {bytes_moved / (med * 1e-3) / 1e12:.3f} TB/s = {100 * bytes_moved / (med * 1e-3) / COPY_RATE:.1f} % of the copy rate"
            say(line)
    torch.set_num_threads(16)

    def torch_cpu():
        return torch_route(wav.cpu(), tab, full, n_out)
    torch_cpu()
    med, lo, hi = _host(torch_cpu, max(3, rounds // 4))
    rec["torch_cpu_16"] = {"us": 1e3 * med, "min_us": 1e3 * lo, "max_us": 1e3 * hi}
    say(f"  {'torch_cpu 16':>12}: {1e3 * med:10.1f} us per batch, copy included (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})")
    say(f"  launch vs torch on the device: {rec['torch_dev']['us'] / rec['launch']['us']:.1f}x; call vs torch on the device: "
        f"{rec['torch_dev']['us'] / rec['call']['us']:.1f}x; launch == call: {rec['launch_equals_call']}; max |call - torch_dev| "
        f"{rec['max_abs_lsb_diff_to_torch_dev']} LSB")

    # time to the first block, with and without the PCM step
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
    with_pcm = lambda: post.stream_pcm(m.generate_stream(**kw), fmt)      # noqa: E731
    for _ in range(2):
        first_block_ms(plain, 1), first_block_ms(with_pcm, 1)
    for name, make in (("generate_stream", plain), ("stream_pcm(generate_stream)", with_pcm), ("generate_stream again", plain)):
        med, lo, hi = first_block_ms(make, max(5, rounds // 2))
        rec[name] = {"first_block_ms": med, "min_ms": lo, "max_ms": hi}
        say(f"  first block of {name:>28}: {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}); tiny model, 2 clips, 128 frames, block_frames 16")
    say(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("# audio output timing (tools/time_audio_out.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
