#!/usr/bin/env python
"""Video preprocessing at configs[1]'s batch: 8 clips x 64 frames of 360 x 640 uint8 -> (8, 4, 3, 16, 224, 224) fp32.
  device   VideoPreprocessor on frames already on the device (the kernel alone: vaura_video_preprocess)
  pinned   the same from pinned host memory (one uint8 copy over the link + the kernel)
  cpu_N    the reference's route on this host with N threads: torch's antialiased uint8 interpolate + crop + /255 + normalise
HIP events on one stream for the device rows, a host clock for the CPU rows; warm-up, then the median of `rounds` (min and max kept).
Bytes: what the algorithm needs per frame (the source rows and columns that survive the crop, read once, plus the fp32 output) over the
kernel time, against the 6.29 TB/s copy rate measured on this part (MI355X_MICROARCH.md).

    python tools/time_preprocess.py [rounds] > profiles/preprocess_timing.txt

--yuv: the same batch as 4:2:0 decoder surfaces (input_format="nv12" / "i420": vaura_video_preprocess_yuv420, 1.5 bytes per pixel over
the link instead of 3) beside the RGB rows, which are the comparison: the RGB input is the host's conversion of the same planes, so all
six rows compute the same output (checked before timing).  The rows alternate inside every round, so they share clocks and neighbours.

    python tools/time_preprocess.py [rounds] --yuv > profiles/preprocess_yuv_timing.txt

--fps: video at its own frame rate (main_fps): the table launch beside the existing launch on the frames selected beforehand and
beside index_select + the existing launch, 60 and 30 fps, RGB and NV12, device and pinned; then a VideoFrameStream per push.

    python tools/time_preprocess.py [rounds] --fps > profiles/preprocess_fps_timing.txt
"""
import json
import os
import statistics
import subprocess
import sys
import time

import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaura_amd.preprocess import VideoPreprocessor, crop_offset, fps_plan, resized_size, yuv420_to_rgb_u8  # noqa: E402

COPY_RATE = 6.29e12
B, T, H, W = 8, 64, 360, 640


def _events(stream, fn, rounds):
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def _events_alternating(stream, fns, rounds):
    """Every row once per round, in turn: {name: (median, min, max)} ms."""
    ts = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            torch.cuda.synchronize()
            ts[name].append(a.elapsed_time(b))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in ts.items()}


def main_yuv(rounds):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    y = torch.randint(0, 256, (B, T, H, W), dtype=torch.uint8, generator=g)
    u = torch.randint(0, 256, (B, T, H // 2, W // 2), dtype=torch.uint8, generator=g)
    v = torch.randint(0, 256, (B, T, H // 2, W // 2), dtype=torch.uint8, generator=g)
    nv12 = torch.cat([y, torch.stack([u, v], dim=-1).reshape(B, T, H // 2, W)], dim=2)             # (B, T, 3H/2, W)
    i420 = torch.cat([y, u.reshape(B, T, H // 4, W), v.reshape(B, T, H // 4, W)], dim=2)
    rgb = torch.stack([yuv420_to_rgb_u8(y[b], u[b], v[b]) for b in range(B)])                       # (B, T, 3, H, W), clip by clip
    pres = {"rgb": VideoPreprocessor(device=dev), "nv12": VideoPreprocessor(device=dev, input_format="nv12"),
            "i420": VideoPreprocessor(device=dev, input_format="i420")}
    host = {"rgb": rgb, "nv12": nv12, "i420": i420}
    geo = pres["rgb"].geometry(H, W)
    rec = {"shape": {"clips": B, "frames": T, "H": H, "W": W, "out": [B, T // 16, 3, 16, 224, 224]},
           "input_bytes": {k: t.numel() for k, t in host.items()},
           "tiles": {"rgb": geo.tiles(False), "nv12": geo.tiles(False, "nv12"), "i420": geo.tiles(False, "i420")},
           "clocks_before": _clocks(), "rows": {}}
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        on_dev = {k: t.to(dev) for k, t in host.items()}
        pinned = {k: t.pin_memory() for k, t in host.items()}
        want = pres["rgb"](on_dev["rgb"])
        for k in ("nv12", "i420"):
            if not (torch.equal(pres[k](on_dev[k]), want) and torch.equal(pres[k](pinned[k]), want)):
                raise SystemExit(f"{k}: the output differs from the RGB kernel's on the converted frames")
        fns = {}
        for k, label in (("rgb", ""), ("nv12", " nv12"), ("i420", " i420")):
            fns["device" + label] = lambda k=k: pres[k](on_dev[k])
            fns["pinned" + label] = lambda k=k: pres[k](pinned[k])
        for _ in range(3):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        res = _events_alternating(stream, fns, rounds)
    rec["clocks_after"] = _clocks()
    print(f"# {B} x {T} frames of {H} x {W}: RGB {rgb.numel() / 1e6:.0f} MB, 4:2:0 {nv12.numel() / 1e6:.0f} MB; outputs equal to the bit; "
          f"{rounds} rounds, the six rows in turn inside each", flush=True)
    for name, (med, lo, hi) in res.items():
        rec["rows"][name] = {"ms": med, "min_ms": lo, "max_ms": hi}
        base = res["pinned" if name.startswith("pinned") else "device"]
        print(f"{name:>12}: {med:8.3f} ms per batch (min {lo:.3f}, max {hi:.3f})  {med / base[0]:.2f}x the RGB row "
              f"(whose min-max spread is {base[2] - base[1]:.3f} ms)", flush=True)
    print(json.dumps(rec))


def main_fps(rounds):
    """8 clips x 77 frames of 360 x 640 at 60 fps (32 output frames, 2 segments) and at 30 fps (64, 4 segments), RGB and NV12:
      table            the table launch on the source frames (vaura_video_preprocess_frames / _yuv420_frames)
      preselected      the existing launch on the same frames selected beforehand (the selection is not timed)
      select + plain   torch's index_select on the device, then the existing launch
    from device memory and (table, preselected) from pinned host memory; then a VideoFrameStream of the 30 fps clips pushed 1 and 16
    frames at a time: host time per push (the call returns without waiting for the kernel) and device time per push (events around
    each push: its map upload, launches and carry copy)."""
    dev = torch.device("cuda:0")
    n = 77
    g = torch.Generator().manual_seed(0)
    y = torch.randint(0, 256, (B, n, H, W), dtype=torch.uint8, generator=g)
    u = torch.randint(0, 256, (B, n, H // 2, W // 2), dtype=torch.uint8, generator=g)
    v = torch.randint(0, 256, (B, n, H // 2, W // 2), dtype=torch.uint8, generator=g)
    host = {"rgb": torch.randint(0, 256, (B, n, 3, H, W), dtype=torch.uint8, generator=g),
            "nv12": torch.cat([y, torch.stack([u, v], dim=-1).reshape(B, n, H // 2, W)], dim=2)}
    kw = {"rgb": {}, "nv12": {"input_format": "nv12"}}
    rec = {"shape": {"clips": B, "frames": n, "H": H, "W": W}, "clocks_before": _clocks(), "one_pass": {}, "stream": {}}
    stream = torch.cuda.Stream(dev)
    print(f"# {B} x {n} frames of {H} x {W}; {rounds} rounds, the rows of a block in turn inside each round", flush=True)
    with torch.cuda.stream(stream):
        on_dev = {k: t.to(dev) for k, t in host.items()}
        pinned = {k: t.pin_memory() for k, t in host.items()}
        for rate in (60, 30):
            table = fps_plan(n, rate).table
            idx = torch.from_numpy(table.astype("int64"))
            idx_dev = idx.to(dev)
            for fmt in ("rgb", "nv12"):
                plain, fps = VideoPreprocessor(device=dev, **kw[fmt]), VideoPreprocessor(device=dev, src_fps=rate, **kw[fmt])
                sel_dev = on_dev[fmt].index_select(1, idx_dev)
                sel_pin = host[fmt].index_select(1, idx).pin_memory()
                want = plain(sel_dev)
                if not (torch.equal(fps(on_dev[fmt]), want) and torch.equal(fps(pinned[fmt]), want)):
                    raise SystemExit(f"{fmt} at {rate} fps: the table launch differs from the existing launch on the selected frames")
                fns = {"device table": lambda: fps(on_dev[fmt]),
                       "device preselected": lambda: plain(sel_dev),
                       "device select + plain": lambda: plain(on_dev[fmt].index_select(1, idx_dev)),
                       "pinned table": lambda: fps(pinned[fmt]),
                       "pinned preselected": lambda: plain(sel_pin)}
                for _ in range(3):
                    for fn in fns.values():
                        fn()
                torch.cuda.synchronize()
                res = _events_alternating(stream, fns, rounds)
                key = f"{fmt} {rate} fps"
                rec["one_pass"][key] = {"frames_out": int(len(table)), "frames_named": int(len(set(table.tolist()))),
                                        "rows": {k: {"ms": m, "min_ms": lo, "max_ms": hi} for k, (m, lo, hi) in res.items()}}
                print(f"{key}: {len(table)} output frames from {len(set(table.tolist()))} of {n} source frames", flush=True)
                for name, (med, lo, hi) in res.items():
                    base = res["pinned preselected" if name.startswith("pinned") else "device preselected"]
                    print(f"{name:>24}: {med:8.3f} ms per batch (min {lo:.3f}, max {hi:.3f})  {med / base[0]:.2f}x the preselected row "
                          f"(whose min-max spread is {base[2] - base[1]:.3f} ms)", flush=True)
                del sel_dev, sel_pin, want
        # the stream: 30 fps, frames already on the device
        for fmt in ("rgb", "nv12"):
            pre = VideoPreprocessor(device=dev, **kw[fmt])
            for per_push in (1, 16):
                host_ms, dev_ms = [], []
                for r in range(rounds + 2):
                    vs = pre.open_stream(B, src_fps=30)
                    pushes, t_host, evs = 0, 0.0, []
                    for lo in range(0, n, per_push):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(stream)
                        t0 = time.perf_counter()
                        vs.push(on_dev[fmt][:, lo:lo + per_push])
                        t_host += time.perf_counter() - t0
                        b.record(stream)
                        evs.append((a, b))
                        pushes += 1
                    torch.cuda.synchronize()
                    vs.close()
                    if r >= 2:                                           # two warm-up passes
                        host_ms.append(1e3 * t_host / pushes)
                        dev_ms.append(sum(a.elapsed_time(b) for a, b in evs) / pushes)
                key = f"{fmt} {per_push} frame{'s' if per_push > 1 else ''} per push"
                rec["stream"][key] = {"pushes": pushes, "host_ms_per_push": statistics.median(host_ms), "device_ms_per_push": statistics.median(dev_ms)}
                print(f"stream {key:>24}: host {statistics.median(host_ms):7.3f} ms per push (min {min(host_ms):.3f}, max {max(host_ms):.3f}), "
                      f"device {statistics.median(dev_ms):7.3f} ms per push (min {min(dev_ms):.3f}, max {max(dev_ms):.3f}); {pushes} pushes, "
                      f"{B} clips", flush=True)
    rec["clocks_after"] = _clocks()
    print(json.dumps(rec))


def _cpu_route(video, threads, rounds):
    torch.set_num_threads(threads)
    oh, ow = resized_size(H, W, 256)
    top, left = crop_offset(oh, 224), crop_offset(ow, 224)

    def run():
        outs = []
        for clip in video:                                               # the loader transforms one clip at a time
            x = Fn.interpolate(clip, size=(oh, ow), mode="bilinear", antialias=True)[..., top:top + 224, left:left + 224]
            x = (x.to(torch.float32) / 255 - 0.5) / 0.5
            outs.append(x.view(T // 16, 16, 3, 224, 224).permute(0, 2, 1, 3, 4))
        return torch.stack(outs)
    run()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        run()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def _clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30)
        return [ln.strip() for ln in r.stdout.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:  # noqa: BLE001
        return [f"not read ({type(e).__name__})"]


def main():
    args = [a for a in sys.argv[1:] if a not in ("--yuv", "--fps")]
    rounds = int(args[0]) if args else 20
    if "--yuv" in sys.argv:
        return main_yuv(rounds)
    if "--fps" in sys.argv:
        return main_fps(rounds)
    dev = torch.device("cuda:0")
    video = torch.randint(0, 256, (B, T, 3, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    pre = VideoPreprocessor(device=dev)
    g = pre.geometry(H, W)
    rows = int(g.v["start"].max()) + g.v["taps"] - int(g.v["start"].min())
    bytes_in, bytes_out = 3 * rows * g.span, 3 * 224 * 224 * 4
    n_frames = B * T
    stream = torch.cuda.Stream(dev)
    rec = {"shape": {"clips": B, "frames": T, "H": H, "W": W, "out": [B, T // 16, 3, 16, 224, 224]},
           "bytes_per_frame": {"read": bytes_in, "written": bytes_out}, "clocks_before": _clocks(), "rows": {}}
    with torch.cuda.stream(stream):
        on_dev, pinned = video.to(dev), video.pin_memory()
        for _ in range(3):
            pre(on_dev), pre(pinned)
        torch.cuda.synchronize()
        for name, src in (("device", on_dev), ("pinned", pinned), ("device_again", on_dev)):
            med, lo, hi = _events(stream, lambda: pre(src), rounds)
            rec["rows"][name] = {"ms": med, "min_ms": lo, "max_ms": hi}
            line = f"{name:>12}: {med:8.3f} ms per batch (min {lo:.3f}, max {hi:.3f}; {rounds} rounds)"
            if name.startswith("device"):
                rate = n_frames * (bytes_in + bytes_out) / (med * 1e-3)
                rec["rows"][name].update(bytes_per_s=rate, share_of_copy_rate=rate / COPY_RATE)
                line += f"  {rate / 1e12:.3f} TB/s needed bytes = {100 * rate / COPY_RATE:.1f} % of the 6.29 TB/s copy rate"
            print(line, flush=True)
        # NHWC source (what a decoder hands over)
        nhwc = on_dev.permute(0, 1, 3, 4, 2).contiguous()
        pre_cl = VideoPreprocessor(device=dev, channels_last=True)
        for _ in range(3):
            pre_cl(nhwc)
        med, lo, hi = _events(stream, lambda: pre_cl(nhwc), rounds)
        rec["rows"]["device_channels_last"] = {"ms": med, "min_ms": lo, "max_ms": hi}
        print(f"{'device NHWC':>12}: {med:8.3f} ms per batch (min {lo:.3f}, max {hi:.3f})", flush=True)
    rec["clocks_after"] = _clocks()
    for threads in (4, 16):
        med, lo, hi = _cpu_route(video, threads, max(3, rounds // 5))
        rec["rows"][f"cpu_{threads}"] = {"ms": med, "min_ms": lo, "max_ms": hi}
        print(f"{'cpu ' + str(threads) + ' thr':>12}: {med:8.1f} ms per batch (min {lo:.1f}, max {hi:.1f})  torch interpolate(antialias) uint8 + crop + "
              f"normalise; device kernel is {med / rec['rows']['device']['ms']:.0f}x, from pinned memory {med / rec['rows']['pinned']['ms']:.0f}x faster",
              flush=True)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
