#!/usr/bin/env python
"""Audio preprocessing at configs[1]'s batch: 8 clips of 2.56 s -> (8, 1, 112896) fp32 mono at 44.1 kHz, for two sources:
48 kHz stereo int16 (interleaved, as a decoder hands it over, and planar) and 16 kHz mono float.  Three routes per source:
  launch      vaura_audio_preprocess alone on PCM already on the device: `inner` launches back to back between two HIP events
  call        AudioPreprocessor.__call__ (host checks, the allocation and the launch), the same way
  torch_dev   AudioPreprocessor.reference() on the same device: convert, mean, torchaudio's strided conv1d over the full-form kernel,
              one clip at a time as the data loader works — what a user can do today with torch alone
  torch_cpu   reference() on the host with 16 threads (a host clock)
Warm-up, then the median of `rounds` (min and max kept).  Bytes: the PCM read once plus the fp32 output, over the launch time, against
the 6.29 TB/s copy rate measured on this part; LDS: 4 bytes per tap and output sample, against the 75 TB/s of 4-byte LDS reads
(MI355X_MICROARCH.md).

    python tools/time_audio_pre.py [rounds] [out file, default profiles/audio_preprocess_timing.txt]
"""
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import audio_preprocess as AP  # noqa: E402

COPY_RATE, LDS_B32_RATE = 6.29e12, 75e12
B, SECONDS, NEW = 8, 2.56, 44100
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


def _pcm(dtype, C, N, interleaved):
    g = torch.Generator().manual_seed(0)
    shape = (B, N, C) if interleaved else (B, C, N)
    if dtype == torch.int16:
        return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16)
    return torch.rand(shape, generator=g) * 2 - 1


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "audio_preprocess_timing.txt")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    lines, rec = [], {"clips": B, "seconds": SECONDS, "rounds": rounds, "launches_per_round": INNER, "rows": {}}

    def say(line):
        print(line, flush=True)
        lines.append(line)

    sources = [("48 kHz stereo int16 interleaved", 48000, torch.int16, 2, True), ("48 kHz stereo int16 planar", 48000, torch.int16, 2, False),
               ("16 kHz mono float32", 16000, torch.float32, 1, False)]
    for name, orig, dtype, C, interleaved in sources:
        N = int(round(SECONDS * orig))
        host = _pcm(dtype, C, N, interleaved)
        pre = AP.AudioPreprocessor(duration=SECONDS, device=dev)
        tab = pre.table(orig)
        n_out = pre.output_length(N, orig)
        bytes_moved = host.numel() * host.element_size() + B * n_out * 4
        lds_bytes = B * n_out * tab["taps"] * 4
        row = {"source_rate": orig, "channels": C, "samples": N, "out_samples": n_out, "taps_per_phase": tab["taps"], "phases": tab["n"],
               "bytes_moved": bytes_moved, "lds_read_bytes": lds_bytes}
        say(f"{name}: {B} x {N} samples -> {B} x {n_out}; {tab['n']} phases of {tab['taps']} taps; {bytes_moved / 1e6:.2f} MB moved, "
            f"{lds_bytes / 1e6:.1f} MB of LDS reads, {B * -(-n_out // AP.TILE)} workgroups")
        with torch.cuda.stream(stream):
            on_dev = host.to(dev)
            first, taps = pre._device_table(orig, dev)
            d_in = torch.full((B,), N, dtype=torch.int32, device=dev)
            d_out = torch.full((B,), n_out, dtype=torch.int32, device=dev)
            out = torch.empty(B, 1, n_out, device=dev)
            lib, st = L.lib(), L.current_stream(dev)

            def launch():
                L.check(lib.vaura_audio_preprocess(L.ptr(on_dev), AP._FORMATS[dtype], int(interleaved), B, C, N, L.ptr(d_in), tab["o"], tab["n"],
                                                   tab["w"], L.ptr(first), L.ptr(taps), tab["n"], tab["taps"], L.ptr(out), n_out, L.ptr(d_out), st),
                        "vaura_audio_preprocess")

            def call():
                return pre(on_dev, sample_rate=orig, interleaved=interleaved)

            def torch_dev():
                return pre.reference(on_dev, sample_rate=orig, interleaved=interleaved)

            for _ in range(3):
                launch(), call(), torch_dev()
            torch.cuda.synchronize()
            got, ref = call()[0], torch_dev()[0]
            launch()
            torch.cuda.synchronize()
            row["max_abs_diff_to_torch_dev"] = float((got - ref).abs().max())
            row["launch_equals_call"] = bool(torch.equal(out, got))
            for route, fn, inner in (("launch", launch, INNER), ("call", call, INNER), ("torch_dev", torch_dev, 5), ("launch_again", launch, INNER)):
                med, lo, hi = _events(stream, fn, rounds, inner)
                row[route] = {"us": 1e3 * med, "min_us": 1e3 * lo, "max_us": 1e3 * hi}
                line = f"  {route:>12}: {1e3 * med:10.1f} us per batch (min {1e3 * lo:.1f}, max {1e3 * hi:.1f}; {rounds} rounds of {inner})"
                if route.startswith("launch"):
                    line += (f"  {bytes_moved / (med * 1e-3) / 1e12:.3f} TB/s = {100 * bytes_moved / (med * 1e-3) / COPY_RATE:.1f} % of the copy rate, "
                             f"LDS reads {100 * lds_bytes / (med * 1e-3) / LDS_B32_RATE:.1f} % of the 4-byte LDS rate")
                say(line)
        torch.set_num_threads(16)
        pre_cpu = AP.AudioPreprocessor(duration=SECONDS)
        pre_cpu.reference(host, sample_rate=orig, interleaved=interleaved)
        med, lo, hi = _host(lambda: pre_cpu.reference(host, sample_rate=orig, interleaved=interleaved), max(3, rounds // 4))
        row["torch_cpu_16"] = {"us": 1e3 * med, "min_us": 1e3 * lo, "max_us": 1e3 * hi}
        say(f"  {'torch_cpu 16':>12}: {1e3 * med:10.1f} us per batch (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})")
        say(f"  launch vs torch on the device: {row['torch_dev']['us'] / row['launch']['us']:.1f}x; call vs torch on the device: "
            f"{row['torch_dev']['us'] / row['call']['us']:.1f}x; max |launch - torch_dev| {row['max_abs_diff_to_torch_dev']:.2e}")
        rec["rows"][name] = row
    say(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("# audio preprocessing timing (tools/time_audio_pre.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
