#!/usr/bin/env python
"""bench.py — V-AURA generation hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W          (N>1 from a plain shell: starts its own N ranks; under
                                                            torch.distributed.run it is one of them)

One "step" = one pass of the hot path over one batch of synthetic clips on each GPU:
video-feature MLP -> 228-step KV-cached decode loop (CFG + top-k sampling, delay pattern) ->
DAC decode to a 44.1 kHz waveform, with features / weights already resident in HBM.
Workload (BASELINE.json configs[1]): 8 clips per GPU of 2.56 s (T=220 frames, 9 codebooks),
top-k 250, temperature 1.0, cfg_scale 6.0 (the reference's default, configs/generate_vgg.yaml:27).
Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the line (`value`, `ms_per_step`, the split of the timed steps).
--full adds everything else the line can carry, each with runs of its own: the bf16-representable checkpoint and the exact-fp32
engine on the same job, per-kernel figures, the plugin surface, raw frames -> waveform, the other BASELINE configs and the CPU
baseline (the --no-* options below switch single legs of it off).
--dump-outputs DIR writes what the LAST timed step returned, as float32 .npy files: DIR/codes.npy (tokens, clips x 9 x T) and
DIR/waveform.npy (clips x 1 x samples); the inputs are seeded, so the same arguments give the same inputs on every run.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import dist as vdist  # noqa: E402
from vaura_amd import synth  # noqa: E402
from vaura_amd.engine import CodecEngine, DecoderEngine  # noqa: E402

HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: 8.0 TB/s spec
T_FRAMES, K_CB, TV = 220, 9, 32
HOP = 512
DUMP_CAP_BYTES = 60_000_000      # --dump-outputs: array data in all (under 64 MB with the .npy headers)


def dump_outputs(dirname: str, arrays) -> None:
    """name -> tensor, written as DIR/<name>.npy in float32 (token ids < 1024 are exact there).  An array that would take the total
    past DUMP_CAP_BYTES is replaced by a fixed, seeded sample of its elements (flattened, in index order)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    left = DUMP_CAP_BYTES
    for name, t in arrays.items():
        a = t.detach().to("cpu", torch.float32).numpy()
        if a.nbytes > left:
            idx = np.sort(np.random.default_rng(0).choice(a.size, left // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, f"{name}.npy"), a)
        left -= a.nbytes


def algorithmic_bytes_per_launch(kind: str, cfg: synth.SamplerCfg, wbytes: int, rows: int) -> float:
    """Weight bytes a launch of each GEMV kind must stream."""
    D, F = cfg.d_model, cfg.ffn_dim
    n = {"qkv": 3 * D * D, "wo": D * D, "w13": 2 * F * D, "w2": D * F, "heads": cfg.num_codebooks * cfg.d_codebook * D}[kind]
    return float(n * (2 if kind == "heads" and wbytes == 1 else wbytes))   # fp8 keeps the heads in bf16


def decode_loop_bytes(cfg: synth.SamplerCfg, wbytes: int, rows: int, steps: int, kvbytes: int = 4) -> float:
    """sum_L [ W*b_w + 24*2*Bs*1536*b_kv*(L+1) ]; b_kv = 4 (fp32 K/V: every parity configuration) or 2 (kv_dtype="f16")."""
    D, F = cfg.d_model, cfg.ffn_dim
    Wb = cfg.num_layers * (3 * D * D + D * D + 3 * F * D) * wbytes + \
        cfg.num_codebooks * cfg.d_codebook * D * (2 if wbytes == 1 else wbytes)
    tot = 0.0
    for Lc in range(1, steps + 1):
        tot += Wb + cfg.num_layers * 2 * rows * D * kvbytes * (Lc + 1)
    return tot


def extra_configs(args, dev, cfg, ccfg, sd, eng_h2, codec_pair, stream):
    """Short timed regions of the BASELINE configs the headline line does not run (all on the un-rounded synthetic checkpoint `sd`):
      rows32_h2          the reference's default batch (configs/generate_vgg.yaml:41: 16 clips, cfg 6 -> 32 decoder rows), h2
      c4                 BASELINE configs[3]: 10.24 s single pass (T=880, 128 video tokens, block_size_audio 1024), B=4, cfg 1, h2
      fp8h_kv16_mx8_rows32  BASELINE configs[4]'s per-GPU shape: fp8 weights against the hi activation plane (weight_dtype="fp8h"), fp16 K/V
                         cache, block-scaled fp8 codec, 16 clips, cfg 6 — with "tol vs bf16 reported": logits / tokens against the one-plane
                         ("h1" = the bf16-class) engine on the same checkpoint, waveform against the fp16-pair codec
      longform           row f1: 10.24 s clips through the sliding-window caller (scripts/generate.py:327-369), 8 clips, cfg 6, h2"""
    from vaura_amd.longform import COMPRESSION_MODEL_FRAME_RATE, chunk_schedule
    res = {}
    kw6 = dict(use_sampling=True, temp=1.0, top_k=args.top_k, top_p=0.0, cfg_scale=6.0, seed=1234, clip_base=0, use_graph=True)

    def region(e, cdc, feats, T, kw, wbytes, rows, cfgx, steps=3, warm=1, kvbytes=4):
        with torch.cuda.stream(stream):
            for _ in range(warm):
                cdc.decode(e.generate_codes(feats, T, **kw))
            torch.cuda.synchronize(dev)
            ev = []
            t0 = time.perf_counter()
            for _ in range(steps):
                a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                a.record(stream)
                codes = e.generate_codes(feats, T, **kw)
                b.record(stream)
                wav = cdc.decode(codes)
                c.record(stream)
                ev.append((a, b, c))
            torch.cuda.synchronize(dev)
            dt = (time.perf_counter() - t0) / steps
        e.check_status()                                  # a hand-off that gave up / non-finite logits FAIL the run
        assert int(codes.min()) >= 0 and int(codes.max()) < 1024 and bool(torch.isfinite(wav).all())
        tl = sum(a.elapsed_time(b) for a, b, _ in ev) / steps
        tc = sum(b.elapsed_time(c) for _, b, c in ev) / steps
        Bx = feats.shape[0]
        lb = decode_loop_bytes(cfgx, wbytes, rows, T + K_CB - 1, kvbytes)
        return {"value": round(Bx * K_CB * T / dt, 1), "unit": "codec tokens/s", "ms_per_step": round(1e3 * dt, 3), "steps": steps,
                "decode_loop_ms": round(tl, 3), "codec_ms": round(tc, 3), "rows": rows,
                "decode_loop_roofline": {"bound": "hbm", "achieved": round(lb / (tl * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                         "frac": round(lb / (tl * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "bytes": lb},
                "status_word": "clean", "near_tie_decisions_last_call": e.last_near_ties[0]}, codes

    # -- the reference's default batch on the headline storage
    f16 = synth.video_features(16, 32, cfg.cond_in, seed=0).to(dev)
    r, _ = region(eng_h2, codec_pair, f16, 220, kw6, 4, 32, cfg)
    r["workload"] = "16 clips x 2.56 s, cfg 6 (32 decoder rows: configs/generate_vgg.yaml:41 + :27), top-k 250, two fp16 planes, fp16-pair codec"
    res["rows32_h2"] = r

    # -- row f1: the sliding-window caller
    n_seg, dur = 16, 10.24
    fl = synth.video_features(8, n_seg * 8, seed=0).reshape(8, n_seg, 8, 768).to(dev)
    sched = chunk_schedule(dur, 2.56, 0.64, 25)
    stride_tokens = int(COMPRESSION_MODEL_FRAME_RATE * 0.64)

    def longform():
        toks, prompt = [], None
        for ch in sched:
            lo, hi = ch["positions"]
            sel = fl[:, torch.arange(lo, hi, device=dev) % n_seg].reshape(8, -1, 768)
            tok = eng_h2.generate_codes(sel, ch["max_gen_len"], prompt=prompt, **kw6)
            toks.append(tok if prompt is None else tok[:, :, prompt.shape[-1]:])
            prompt = tok[:, :, stride_tokens:]
        codes = torch.cat(toks, dim=-1)
        return codes, codec_pair.decode(codes)
    with torch.cuda.stream(stream):
        longform()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(2):
            codes, wav = longform()
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) / 2
    eng_h2.check_status()
    res["longform"] = {"value": round(8 * K_CB * codes.shape[-1] / dt, 1), "unit": "codec tokens/s", "ms_per_step": round(1e3 * dt, 3), "steps": 2,
                       "sec_audio_per_sec": round(8 * codes.shape[-1] * HOP / 44100 / dt, 2), "chunks": len(sched), "status_word": "clean",
                       "workload": f"8 clips x {dur} s through the sliding-window caller (2.56 s window, 0.64 s stride, prompt carry-over, one codec "
                                   "decode at the end: scripts/generate.py:327-369), cfg 6, top-k 250, two fp16 planes"}

    # -- configs[3]
    cfg4 = synth.SamplerCfg(block_size_audio=1024)
    e4 = DecoderEngine(cfg4, sd, dev)
    f4 = synth.video_features(4, 128, cfg.cond_in, seed=0).to(dev)
    kw1 = dict(kw6, cfg_scale=1.0)
    r, _ = region(e4, codec_pair, f4, 880, kw1, 4, 4, cfg4)
    r["workload"] = "configs[3]: 4 clips x 10.24 s single pass (T=880, Tv=128, block_size_audio 1024), cfg 1 (4 decoder rows), top-k 250, two fp16 planes"
    res["c4"] = r
    del e4
    torch.cuda.empty_cache()

    # -- configs[4]'s per-GPU shape + its tolerance report
    c8 = CodecEngine(ccfg, synth.codec_state_dict(ccfg, seed=0), dev, precision="mx8")
    e8f = DecoderEngine(cfg, sd, dev, wdtype="fp8h")                   # the same storage with the fp32 K/V cache of the parity configurations
    r32, _ = region(e8f, c8, f16, 220, kw6, 1, 32, cfg)
    del e8f
    torch.cuda.empty_cache()
    e8k = DecoderEngine(cfg, sd, dev, wdtype="fp8h", kv_dtype="f8")    # ... and with e4m3 K/V (unscaled, saturating): a ~4e-2-class option
    idx8 = torch.randint(0, 1024, (2, K_CB, 24), generator=torch.Generator().manual_seed(11)).to(dev)
    r8k, _ = region(e8k, c8, f16, 220, kw6, 1, 32, cfg, kvbytes=1)
    lg8k = e8k.logits_all_positions(idx8, f16[:2]).float().cpu()
    del e8k
    torch.cuda.empty_cache()
    e8 = DecoderEngine(cfg, sd, dev, wdtype="fp8h", kv_dtype="f16")
    r, codes8 = region(e8, c8, f16, 220, kw6, 1, 32, cfg, kvbytes=2)
    lg8h = e8.logits_all_positions(idx8, f16[:2]).float().cpu()
    r["with_fp32_kv_cache"] = {k: r32[k] for k in ("value", "ms_per_step", "decode_loop_ms", "decode_loop_roofline")}
    r["with_fp8_kv_cache"] = {k: r8k[k] for k in ("value", "ms_per_step", "decode_loop_ms", "decode_loop_roofline")}
    r["with_fp8_kv_cache"]["logits_rel_rms_vs_fp16_kv"] = round(float((lg8k - lg8h).pow(2).mean().sqrt() / lg8h.pow(2).mean().sqrt()), 5)
    r["workload"] = ("configs[4] per GPU: 16 clips x 2.56 s, cfg 6 (32 rows), top-k 250; per-layer matrices fp8 e4m3 + row scales multiplied against the "
                     "hi fp16 activation plane (weight_dtype='fp8h'), one-plane heads, fp16 K/V cache (kv_dtype='f16'); codec on the block-scaled "
                     "fp8 MFMA (mx8).  The roofline bytes count the K/V stream at 2 bytes per element")
    idx = codes8[:2, :, :24].contiguous()
    lg8 = e8.logits_all_positions(idx, f16[:2]).float().cpu()
    wav8 = c8.decode(codes8)
    wavp = codec_pair.decode(codes8)
    sig = float((wavp ** 2).mean().sqrt())
    wrms = float(((wav8 - wavp) ** 2).mean().sqrt())
    del e8, c8
    torch.cuda.empty_cache()
    eb = DecoderEngine(cfg, sd, dev, wdtype="h1")          # one fp16 plane forced on this checkpoint: the 16-bit-weight ("bf16-class") run
    with torch.cuda.stream(stream):
        codesb = eb.generate_codes(f16, 220, **kw6)
        torch.cuda.synchronize(dev)
    lgb = eb.logits_all_positions(idx, f16[:2]).float().cpu()
    eb.check_status()
    del eb
    torch.cuda.empty_cache()
    c8c, cbc = codes8.cpu(), codesb.cpu()
    steps_of = torch.arange(220)[None, :] + 1 + torch.arange(K_CB)[:, None]
    first = [int(steps_of[c8c[b] != cbc[b]].min()) if not torch.equal(c8c[b], cbc[b]) else 229 for b in range(16)]
    r["tolerance_vs_bf16"] = {
        "what": "fp8h + fp16-K/V engine against the one-plane fp16 ('h1', 16-bit weights, fp32 K/V) engine on the same checkpoint, same Philox noise; synthetic "
                "random-init weights: logits are nearly flat, so sampled sequences separate at the first near-tie and stay apart",
        "logits_rel_rms": round(float((lg8 - lgb).pow(2).mean().sqrt() / lgb.pow(2).mean().sqrt()), 5),
        "logits_max_abs": round(float((lg8 - lgb).abs().max()), 5), "logits_top1_agreement": round(float((lg8.argmax(-1) == lgb.argmax(-1)).float().mean()), 4),
        "sampled_token_agreement_220_frames": round(float((c8c == cbc).float().mean()), 4), "median_first_divergence_step": int(sorted(first)[8]),
        "waveform_rms_mx8_vs_f16pair_codec_same_tokens": round(wrms, 5), "waveform_signal_rms": round(sig, 5)}
    res["fp8h_kv16_mx8_rows32"] = r
    return res


def cpu_baseline(sd, feats_cpu, cfg_scale, n_clips, top_k, quick=False):
    """Oracle (CPU port of the reference path) on this box's host cores, as BASELINE.md §3 defines the baseline: real runs, no
    extrapolation.
      reference_faithful  ONE full run of the reference's own algorithm for one clip (configs[0] = C1: B=1, greedy, cfg 1): the whole
                          prefix re-fed every step, logits for every position, no cache (models/vaura_model.py:504-506) — 228 passes
                          of lengths 1..228 — plus the CPU DAC restatement's decode of its tokens: end to end, one run (flagged).
      cached              the same clip through the K/V-cached port: 1 warm-up + 3 full runs, median.
      value               the K/V-cached port at the GPU's OWN workload (all `n_clips` clips, CFG rows, top-k sampling): one full
                          228-step run + the codec (one clip timed, x clips), so that GPU / CPU is not just the 114x algorithmic gap.
    Thread counts are swept first (torch's default of one thread per core oversubscribes a 16-row GEMV 8x); `cores` = the
    count the `value` run used.  `quick` (bench.py --quick-cpu-baseline): the round-3 bounded sample instead of full runs."""
    from oracle import dac_oracle
    from oracle import generate_oracle as go
    from oracle.decoder_oracle import CachedDecoder, DecoderOracle
    cfg = synth.FULL_SAMPLER
    ccfg = synth.FULL_CODEC
    dec = DecoderOracle(sd, cfg.num_layers, cfg.nhead)
    g = torch.Generator().manual_seed(0)
    n_steps = T_FRAMES + K_CB - 1
    tokens_per_clip = K_CB * T_FRAMES
    with torch.no_grad():
        cond = feats_cpu[:n_clips]
        cond_all = torch.cat([cond, dec.null_condition(cond)], 0) if cfg_scale > 1 else cond
        rows = cond_all.shape[0]
        cd = CachedDecoder(dec, cond_all, n_steps + 1)
        tok = torch.randint(0, 1024, (rows, K_CB), generator=g)
        cd.step(tok)                      # warm-up (allocations, thread pool)
        default_threads = torch.get_num_threads()
        cand = [nt for nt in sorted({8, 16, 32, 64, max(1, default_threads // 2), default_threads}) if nt <= default_threads]
        sweep = {}
        for nt in cand:                   # the GPU batch's decode step (16 rows)
            torch.set_num_threads(nt)
            cd.pos = 1
            cd.step(tok)
            t0 = time.perf_counter()
            for _ in range(2):
                cd.step(tok)
            sweep[nt] = (time.perf_counter() - t0) / 2
        best = min(sweep, key=sweep.get)
        idx = torch.randint(0, 1024, (1, K_CB, 128), generator=g)
        sweep_full = {}
        for nt in cand:                   # the reference's cache-less pass (one clip, 128 positions)
            torch.set_num_threads(nt)
            dec.forward_full(idx[:, :, :8], cond[:1])
            t0 = time.perf_counter()
            dec.forward_full(idx, cond[:1])
            sweep_full[nt] = time.perf_counter() - t0
        best_full = min(sweep_full, key=sweep_full.get)
        out = {"unit": "codec tokens/s", "kind": "port", "logical_cpus": os.cpu_count(), "torch_default_threads": default_threads,
               "thread_sweep_ms_per_step": {str(k): round(1e3 * v, 1) for k, v in sweep.items()},
               "thread_sweep_ms_full_prefix_L128": {str(k): round(1e3 * v, 1) for k, v in sweep_full.items()}}
        if quick:
            torch.set_num_threads(best)
            ts = []
            for p0 in (1, n_steps - 7):
                cd.pos = p0
                t0 = time.perf_counter()
                for _ in range(6):
                    cd.step(tok)
                ts.append((time.perf_counter() - t0) / 6)
            cached_s = 0.5 * (ts[0] + ts[1]) * n_steps
            out.update({"value": round(n_clips * tokens_per_clip / cached_s, 2), "cores": best,
                        "sample": (f"QUICK: K/V-cached port at the GPU's batch ({n_clips} clips, rows={rows}): 6 steps at cache length ~1 "
                                   f"({ts[0] * 1e3:.0f} ms/step) and 6 at ~{n_steps - 7} ({ts[1] * 1e3:.0f} ms/step), mean x {n_steps}; "
                                   "decode loop only")})
            return out
        del cd
        # ---- codec: the CPU DAC restatement on one clip's tokens
        torch.set_num_threads(best_full)
        csd = synth.codec_state_dict(ccfg, seed=0)
        codes1 = torch.randint(0, 1024, (1, K_CB, T_FRAMES), generator=g)
        dac_oracle.decode(csd, codes1[:, :, :8], ccfg.decoder_rates)
        t0 = time.perf_counter()
        dac_oracle.decode(csd, codes1, ccfg.decoder_rates)
        codec_s = time.perf_counter() - t0
        # ---- the reference's own algorithm, one clip, ONE full run (C1)
        t0 = time.perf_counter()
        tk_full = go.generate(dec, cond[:1], T_FRAMES, mode="full")
        faithful_s = time.perf_counter() - t0
        # ---- the same clip through the K/V-cached port: warm-up + 3 runs, median
        torch.set_num_threads(best)
        runs = []
        for i in range(4):
            t0 = time.perf_counter()
            tk_c = go.generate(dec, cond[:1], T_FRAMES, mode="cached")
            runs.append(time.perf_counter() - t0)
        cached1 = sorted(runs[1:])[1]
        same = bool(torch.equal(tk_full, tk_c))
        # ---- the GPU's own workload through the K/V-cached port: ONE full run
        nz = synth.exp_noise(n_steps, n_clips * K_CB, 1024, 1234)
        t0 = time.perf_counter()
        go.generate(dec, cond, T_FRAMES, mode="cached", cfg_scale=cfg_scale, use_sampling=True, temp=1.0, top_k=top_k, noise=nz)
        cached_batch_s = time.perf_counter() - t0
    wall = cached_batch_s + n_clips * codec_s
    out.update({
        "value": round(n_clips * tokens_per_clip / wall, 2), "cores": best,
        "sample": (f"oracle/ fp32 torch-CPU port with a K/V cache on the GPU's own workload ({n_clips} clips, rows={rows}, cfg {cfg_scale}, "
                   f"top-k {top_k}): ONE full {n_steps}-step run = {cached_batch_s:.1f} s on {best} threads, + the CPU DAC restatement "
                   f"({codec_s:.2f} s for one clip on {best_full} threads, x {n_clips}) = {wall:.1f} s per batch, end to end"),
        "decode_loop_only_tok_s": round(n_clips * tokens_per_clip / cached_batch_s, 2),
        "codec_s": round(codec_s, 3),
        "reference_faithful_s_per_clip": round(faithful_s, 2),
        "reference_faithful": {
            "what": ("the reference's algorithm as it is (models/vaura_model.py:502-547: whole prefix re-fed every step, no cache, logits for "
                     f"every position), configs[0]: ONE clip, greedy, cfg 1.0, fp32, {best_full} threads — ONE full run of {n_steps} passes, "
                     "not an extrapolation"),
            "decode_loop_s": round(faithful_s, 2), "codec_s": round(codec_s, 3),
            "tok_s_end_to_end": round(tokens_per_clip / (faithful_s + codec_s), 2), "threads": best_full, "runs": 1,
            "tokens_equal_the_cached_port": same},
        "cached_tok_s": round(tokens_per_clip / cached1, 2),
        "cached": {"what": f"the same clip (configs[0]) through the K/V-cached port, {best} threads: 1 warm-up + 3 full runs, median",
                   "runs_s": [round(r, 2) for r in runs[1:]], "median_s": round(cached1, 2),
                   "tok_s_end_to_end": round(tokens_per_clip / (cached1 + codec_s), 2)},
    })
    return out


def launch_command(n: int, argv, port: int):
    """The child command of `python bench.py --gpus n` from a plain shell: one rank per GPU under torch.distributed.run, rendezvous on
    127.0.0.1 (the container hostname may not resolve), this script's own argv passed through."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__), *argv]


def self_launch(n: int, argv) -> int:
    """Run this script as `n` ranks under torch.distributed.run (child processes) and return their exit status."""
    import socket
    import subprocess
    have = vdist.count_gpus_without_hip()          # sysfs only: this parent never touches torch.cuda / HIP
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if have is not None and have < n and env.get("VAURA_BENCH_SHARE_GPU") != "1":
        print(f"bench.py: --gpus {n} but this box has {have} GPU(s); set VAURA_BENCH_SHARE_GPU=1 VAURA_BENCH_BACKEND=gloo to exercise "
              "the control flow on shared GPUs (never a reported number)", file=sys.stderr)
        return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return subprocess.run(launch_command(n, argv, port), env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=["c2", "c4"], default="c2",
                    help="c2 = BASELINE configs[1] (2.56 s clips, batch 8, cfg 6); c4 = configs[3] (10.24 s single pass, "
                         "batch 4, cfg 1, block_size_audio 1024, 128 video tokens)")
    ap.add_argument("--batch", type=int, default=None, help="clips per GPU (default: 8 for c2, 4 for c4)")
    ap.add_argument("--cfg-scale", type=float, default=None)
    ap.add_argument("--top-k", type=int, default=250)
    ap.add_argument("--weights", choices=["auto", "h1", "h2", "fp8", "fp8h", "f32"], default="auto",
                    help="storage of the streamed matrices (vaura_amd.engine.resolve_weight_dtype); auto = the plugin default: two fp16 "
                         "planes (h2) for the un-rounded checkpoint")
    ap.add_argument("--checkpoint", choices=["raw", "bf16repr"], default="raw",
                    help="synthetic checkpoint of the headline run: raw = un-rounded fp32 weights (what a real V-AURA checkpoint looks "
                         "like to the storage decision), bf16repr = every streamed weight bf16-representable (one fp16 plane is lossless)")
    ap.add_argument("--codec", choices=["f32", "f16pair", "f16", "f16pair_w8", "mx8"], default=None,
                    help="codec conv precision (default: f16pair; f16pair_w8 with --weights fp8).  mx8 = block-scaled fp8 on "
                         "the fp8 MFMA, BASELINE configs[4] together with --weights fp8 --batch 16")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--overlap", action="store_true", help="experiment: codec + gather of batch i on a second stream (slower)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--quick-cpu-baseline", action="store_true",
                    help="bounded 12-step sample of the K/V-cached CPU port instead of the full runs of BASELINE.md 3 (~2.5 min)")
    ap.add_argument("--no-second", "--no-f32", dest="no_second", action="store_true",
                    help="skip the second timed region (the bf16-representable checkpoint on one fp16 plane)")
    ap.add_argument("--no-plugin", action="store_true", help="skip timing VAURAModel.generate() through the plugin classes")
    ap.add_argument("--no-extras", action="store_true")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="skip the short timed regions of the other BASELINE configs (extra_configs: c4, rows32_h2, fp8h_kv16_mx8_rows32, longform)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline (second checkpoint, exact fp32, per-kernel figures, plugin surface, "
                         "extractor, other BASELINE configs, CPU baseline); a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's tokens and waveform to DIR/codes.npy and DIR/waveform.npy (float32)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` from a plain shell: start the N ranks as FRESH child processes (one per GPU, RCCL),
        # before anything in this process has touched the GPU (counting devices does not initialise HIP on this image; an
        # exec from a GPU-initialised process would not be allowed), relay rank 0's JSON line and exit with their status.
        sys.exit(self_launch(args.gpus, sys.argv[1:]))

    # VAURA_BENCH_BACKEND=gloo + VAURA_BENCH_SHARE_GPU=1: exercise the multi-rank control flow on a 1-GPU box
    # (all ranks on cuda:0, collectives on host copies).  Never used for reported numbers.
    share = os.environ.get("VAURA_BENCH_SHARE_GPU") == "1"
    rank, local, world = vdist.init(os.environ.get("VAURA_BENCH_BACKEND", "nccl"), device_index=0 if share else None)
    if share:
        local = 0
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    dev = torch.device(f"cuda:{local}")
    torch.cuda.set_device(dev)
    L.lib()  # fail loudly before doing anything expensive

    long_ctx = args.workload == "c4"
    global T_FRAMES, TV
    if long_ctx:
        T_FRAMES, TV = 880, 128
    if args.batch is None:
        args.batch = 4 if long_ctx else 8
    if args.cfg_scale is None:
        args.cfg_scale = 1.0 if long_ctx else 6.0   # the CFG null embedding is fixed at 32 tokens (vaura_model.py:790-793)
    cfg = synth.SamplerCfg(block_size_audio=1024) if long_ctx else synth.FULL_SAMPLER
    ccfg = synth.FULL_CODEC
    B = args.batch
    first, _ = vdist.shard(B * world, rank, world)
    # Two synthetic checkpoints (no network: weights are regenerated from seeds).  `value` runs on the UN-rounded one — fp32
    # weights 16 bits cannot hold, i.e. what a real V-AURA checkpoint looks like: the plugin default "auto" resolves to two fp16
    # planes (22 significand bits) there.  `value_h1_lossless_checkpoint` is the same job on a bf16-representable checkpoint,
    # which one fp16 plane holds exactly (half the weight bytes).
    sd = synth.sampler_state_dict(cfg, seed=0, round_bf16=(args.checkpoint == "bf16repr"))
    one_launch = not share                   # ranks sharing ONE GPU (control-flow test only): the in-launch hand-off needs the chip to itself
    eng = DecoderEngine(cfg, sd, dev, wdtype=args.weights, one_launch_mlp=one_launch)
    storage = eng.wdtype                     # what "auto" resolved to
    if args.codec is None:
        args.codec = "f16pair_w8" if storage in ("fp8", "fp8h") else "f16pair"
    codec = CodecEngine(ccfg, synth.codec_state_dict(ccfg, seed=0), dev, precision=args.codec)
    feats_cpu = synth.video_features(B, TV, cfg.cond_in, seed=0, first_clip=first)
    feats = feats_cpu.to(dev)
    kw = dict(use_sampling=True, temp=1.0, top_k=args.top_k, top_p=0.0, cfg_scale=args.cfg_scale, seed=1234,
              clip_base=first, use_graph=not args.no_graph)
    counts = [B] * world

    # Everything runs on one non-null HIP stream.  --overlap (experiment, measured SLOWER: 268 vs 255 ms per batch —
    # the codec's full-chip grids delay the latency-bound GEMVs of the next batch's decode loop) puts codec + gather
    # of batch i on a second stream next to the decode loop of batch i+1.
    s_loop = torch.cuda.Stream(dev)
    s_post = torch.cuda.Stream(dev) if args.overlap else s_loop

    marks = []      # (start, loop done, codec done) events of every step: the split of the TIMED steps themselves
    gathered = []   # N > 1: the whole node's (codes, waveform) of the latest step, what rank 0's caller receives

    def step():
        with torch.cuda.stream(s_loop):
            e_a = torch.cuda.Event(enable_timing=True)
            e_a.record(s_loop)
            codes = eng.generate_codes(feats, T_FRAMES, **kw)
            done = torch.cuda.Event(enable_timing=True)
            done.record(s_loop)
        with torch.cuda.stream(s_post):
            s_post.wait_event(done)
            codes.record_stream(s_post)
            wav = codec.decode(codes)
            e_c = torch.cuda.Event(enable_timing=True)
            e_c.record(s_post)
            marks.append((e_a, done, e_c))
            if world > 1:  # the single exchange of the job: final gather of tokens + waveform over RCCL
                gathered[:] = [vdist.gather_clips(codes.to(torch.int32), counts), vdist.gather_clips(wav, counts)]
        return codes, wav

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        vdist.barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            res = fn()
        torch.cuda.synchronize(dev)
        elapsed_local[0] = time.perf_counter() - t0          # this rank's own K steps (before the closing barrier)
        vdist.barrier()
        el = vdist.max_over_ranks(time.perf_counter() - t0, dev)
        # outside the timed region: the sticky device status word (a hand-off of the one-launch MLP that gave up makes every later
        # hand-off return at once — wrong tokens AND an optimistic time; non-finite logits = garbage tokens): the run FAILS on either
        eng.check_status()
        return el, res

    elapsed_local = [0.0]

    if world > 1:
        args.no_extras = True            # N > 1: the timed region, its split and who took part — nothing else
    seen = vdist.ranks_seen(dev)
    if not share:
        vdist.assert_distinct_devices(seen)          # --gpus N means N GPUs: two ranks on one device uuid is a launcher error, not a result
    elapsed, (codes, wav) = timed(step)
    per_rank_ms = vdist.gather_floats(1e3 * elapsed_local[0] / args.steps, dev)
    main_marks = marks[-args.steps:]
    t_loop = sum(a.elapsed_time(b) for a, b, _ in main_marks) / args.steps
    t_codec = sum(b.elapsed_time(c) for _, b, c in main_marks) / args.steps

    assert codes.shape == (B, K_CB, T_FRAMES) and int(codes.min()) >= 0 and int(codes.max()) < 1024
    assert wav.shape == (B, 1, T_FRAMES * HOP) and bool(torch.isfinite(wav).all())
    if args.dump_outputs and rank == 0:
        dump_codes, dump_wav = gathered if world > 1 else (codes, wav)
        dump_outputs(args.dump_outputs, {"codes": dump_codes, "waveform": dump_wav})

    tokens = world * B * K_CB * T_FRAMES * args.steps
    rows = 2 * B if args.cfg_scale > 1 else B
    wbytes = {"h1": 2, "h2": 4, "f32": 4, "fp8": 1, "fp8h": 1}[storage]
    out = {
        "metric": f"audio codec tokens/sec (whole node), {'10.24' if long_ctx else '2.56'} s clips",
        "value": round(tokens / elapsed, 1), "unit": "codec tokens/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None,
        # the arithmetic type the path computes in: exact products of (hi, lo) fp16 operand PAIRS (22 significand bits per operand, the
        # wlo*xlo term dropped) accumulated in fp32; `--weights f32` is bit-for-bit fp32 products on the fp32 MFMA (value_f32_exact below)
        "dtype": {"h2": "f16x2-split(22b)/f32-acc", "h1": "f16x2-split(22b act, 11b w)/f32-acc", "fp8": "fp8-w,f16x2-act/f32-acc",
                  "fp8h": "fp8-w,f16-act/f32-acc", "f32": "f32"}[storage], "data": "synthetic",
        "config": {"workload": (f"configs[{3 if long_ctx else (4 if storage in ('fp8', 'fp8h') and args.codec == 'mx8' else 1)}]: batch={B}/GPU x {'10.24' if long_ctx else '2.56'} s clips (T={T_FRAMES}, 9 codebooks, Tv={TV} AVCLIP-shaped features), "
                                f"top-k {args.top_k}, temp 1.0, cfg_scale {args.cfg_scale} (decoder rows={rows}), 24-layer "
                                "1536-d decoder + DAC-44k decode to waveform"),
                   "global_batch": B * world, "parallelism": f"clip-parallel x{world}, one final all_gather",
                   "weights": ({"h2": "two fp16 planes (hi, lo) + power-of-two row scales per streamed matrix: 22 significand bits, 4 bytes per weight",
                                "h1": "one fp16 plane + power-of-two row scales: lossless for this (bf16-representable) checkpoint, 2 bytes per weight",
                                "f32": "fp32 tiles on the exact-fp32-MFMA GEMVs (cross-check path)",
                                "fp8": "fp8 e4m3 + power-of-two row scales for the per-layer matrices and the codec's conv weights, "
                                       "one-plane heads (a different model: not the headline configuration)",
                                "fp8h": "fp8 e4m3 + power-of-two row scales for the per-layer matrices and the codec's conv weights, one-plane heads; "
                                        "the fp8 matrices multiply the HI fp16 activation plane only (11-bit activations: tolerance reported, configs[4])"}[storage]
                               + f" (requested: {args.weights}; checkpoint: {args.checkpoint})"
                               + "; activations as (hi, lo) fp16 planes between kernels, fp32 accumulate / residual stream / KV cache; codec: "
                               + {"f32": "fp32 MFMA", "f16pair": "activations and weights on (hi, lo) fp16 pairs, fp32 accumulate",
                                  "f16": "plain fp16 operands, fp32 accumulate (the reference's own codec precision class)",
                                  "f16pair_w8": "fp8 weights in one fp16 plane, activations on (hi, lo) fp16 pairs",
                                  "mx8": "fp8 weights and block-scaled fp8 activations on the fp8 MFMA (NOT inside the 1e-4 waveform "
                                         "budget: BASELINE configs[4] option)"}[args.codec]),
                   "hipgraph": not args.no_graph,
                   "streams": "decode loop of batch i+1 overlaps codec+gather of batch i (two HIP streams)" if args.overlap
                              else "one non-null HIP stream"},
        "sec_audio_per_sec": round(world * B * T_FRAMES * HOP / 44100.0 * args.steps / elapsed, 2),
        "value_storage": f"{storage} (weight_dtype={args.weights!r}) on the {'un-rounded (real-checkpoint-shaped)' if args.checkpoint == 'raw' else 'bf16-representable'} synthetic checkpoint",
        "ranks_seen": len(seen), "ranks": seen, "ms_per_step_per_rank": [round(v, 3) for v in per_rank_ms],
        "backend": (torch.distributed.get_backend() if world > 1 else None),
        # an in-launch hand-off that gave up would have FAILED the run above (check_status after the timed region): 0 by construction,
        # reported so that a silent switch to the separate launches can never hide in a number
        "handoff_fallbacks": eng.handoff_fallbacks,
        # near-tie detector (csrc/step.hip; engine.NEAR_TIE_EPS): used decisions of the LAST timed call whose own margin is inside the plane
        # arithmetic's noise bound.  Policy "report": counted, never re-run (near_tie="rerun" would run such a call again on the exact-fp32 engine)
        "near_tie": {"policy": eng.near_tie, "eps_rel": eng.near_tie_eps, "flagged_decisions_last_call": eng.last_near_ties[0],
                     "decisions_per_call": B * K_CB * T_FRAMES,
                     "first_flagged_step": eng.last_near_ties[1]},
    }
    if rank == 0 and world > 1:
        # the split of the timed steps on rank 0 (HIP events inside them); per-kernel rooflines / plugin / CPU legs are N=1 work
        lbN = decode_loop_bytes(cfg, wbytes, rows, T_FRAMES + K_CB - 1)
        out["split_ms"] = {"decode_loop": round(t_loop, 3), "codec": round(t_codec, 3)}
        out["decode_loop_roofline"] = {"bound": "hbm", "achieved": round(lbN / (t_loop * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS,
                                       "unit": "GB/s", "frac": round(lbN / (t_loop * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "bytes": lbN,
                                       "per": "GPU (rank 0)"}

    # ---- the same job on the bf16-representable checkpoint, where "auto" resolves to ONE fp16 plane (half the weight bytes,
    #      same real numbers).  Every rank runs it (same barriers).
    if args.full and not args.no_extras and args.weights == "auto" and args.checkpoint == "raw" and not args.no_second:
        eng_main = eng
        sd_b = synth.sampler_state_dict(cfg, seed=0, round_bf16=True)
        eng = DecoderEngine(cfg, sd_b, dev, one_launch_mlp=one_launch)                    # wdtype="auto"
        assert eng.wdtype == "h1", eng.wdtype
        del sd_b
        el1, (codes1, wav1) = timed(step)
        t_loop1 = sum(a.elapsed_time(b) for a, b, _ in marks[-args.steps:]) / args.steps
        assert int(codes1.min()) >= 0 and int(codes1.max()) < 1024 and bool(torch.isfinite(wav1).all())
        out["value_h1_lossless_checkpoint"] = round(tokens / el1, 1)
        out["ms_per_step_h1_lossless_checkpoint"] = round(1e3 * el1 / args.steps, 3)
        lb1 = decode_loop_bytes(cfg, 2, 2 * B if args.cfg_scale > 1 else B, T_FRAMES + K_CB - 1)
        out["decode_loop_roofline_h1_lossless_checkpoint"] = {"bound": "hbm", "achieved": round(lb1 / (t_loop1 * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS,
                                                              "unit": "GB/s", "frac": round(lb1 / (t_loop1 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                                              "bytes": lb1, "decode_loop_ms": round(t_loop1, 3)}
        out["h1_lossless_checkpoint"] = ("bf16-representable synthetic checkpoint: every streamed weight fits one fp16 plane exactly; storage chosen by "
                                         "weight_dtype='auto'")
        del eng
        torch.cuda.empty_cache()
        eng = eng_main

    # ---- the price of EXACT fp32: the same job, same checkpoint, on the exact-fp32-MFMA engine
    #      (`--weights f32`: fp32 tiles, v_mfma_f32_16x16x4_f32, fp32 activations between kernels) — one more timed region, driver-run
    if args.full and not args.no_extras and args.weights == "auto" and args.checkpoint == "raw" and not args.no_second and not long_ctx:
        eng_main = eng
        eng = DecoderEngine(cfg, sd, dev, wdtype="f32", one_launch_mlp=one_launch)
        elx, (codesx, wavx) = timed(step)
        t_loopx = sum(a.elapsed_time(b) for a, b, _ in marks[-args.steps:]) / args.steps
        assert int(codesx.min()) >= 0 and int(codesx.max()) < 1024 and bool(torch.isfinite(wavx).all())
        out["value_f32_exact"] = round(tokens / elx, 1)
        out["f32_exact"] = {"what": "same job and checkpoint with weight_dtype='f32': fp32 weight tiles and fp32 activations on the exact "
                                    "fp32 matrix instruction (bit-for-bit fp32 products; the cross-check engine of the parity tests)",
                            "ms_per_step": round(1e3 * elx / args.steps, 3), "decode_loop_ms": round(t_loopx, 3),
                            "value_over_value_f32_exact": round(out["value"] / (tokens / elx), 3)}
        out["near_tie"]["cost_of_policy_rerun"] = (
            f"a flagged call is run again on the exact-fp32 engine: + {1e3 * elx / args.steps:.0f} ms on top of {1e3 * elapsed / args.steps:.0f} ms "
            f"per batch; with {out['near_tie']['flagged_decisions_last_call']} flagged decision(s) in the last of these calls that is "
            + ("every such call: the default policy stays 'report'" if out["near_tie"]["flagged_decisions_last_call"] else "not this call"))
        del eng, codesx, wavx
        torch.cuda.empty_cache()
        eng = eng_main

    if rank == 0 and not args.no_extras:
        # ---- split of the timed steps (HIP events recorded inside them, on the streams the work ran on): arithmetic only
        n_steps = T_FRAMES + K_CB - 1
        lb = decode_loop_bytes(cfg, wbytes, rows, n_steps)
        out["split_ms"] = {"decode_loop": round(t_loop, 3), "codec": round(t_codec, 3)}
        out["decode_loop_roofline"] = {"bound": "hbm", "achieved": round(lb / (t_loop * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS,
                                       "unit": "GB/s", "frac": round(lb / (t_loop * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                       "bytes": lb}
        out["codec_tflops"] = round(B * 1.608e9 * T_FRAMES / (t_codec * 1e-3) / 1e12, 2)   # 1.608 GFLOP per codec frame
        # codec decode is MFMA-bound: matrix instructions actually issued per algorithmic product x algorithmic FLOP/s against the
        # dense peak of the instruction used (MI355X_MICROARCH.md: fp32-input MFMA 157 TF, fp16 2.5 PF, block-scaled fp8 5 PF)
        mpp, cpeak = {"f32": (1, 157.3), "f16pair": (3, 2500.0), "f16pair_w8": (2, 2500.0), "f16": (1, 2500.0), "mx8": (1, 5000.0)}[args.codec]
        out["codec_roofline"] = {"bound": "mfma", "achieved": round(mpp * out["codec_tflops"], 1), "peak": cpeak, "unit": "TFLOP/s",
                                 "frac": round(mpp * out["codec_tflops"] / cpeak, 4), "algorithmic_tflops": out["codec_tflops"],
                                 "matrix_instructions_per_product": mpp, "codec_ms": round(t_codec, 3),
                                 "counters": "profiles/r06_codec_mfma.json (tools/mfma_driver under rocprofv3 --pmc; builder: committed record, NOT measured by this run)"}

    if rank == 0 and not args.no_extras and args.full:
        # ---- per-kernel roofline and the other legs of --full, each with runs of its own
        torch.cuda.synchronize(dev)
        torch.cuda.set_stream(s_loop)    # same stream as the timed region; the per-launch events below are recorded on it
        reps = max(2, args.steps)

        # per-kernel, live: every launch of one eager 228-step pass carries its own start/stop events on the stream it is launched on
        # (hipExtLaunchKernelGGL via vaura_profile_loop): the kernel's execution alone.  rocprofv3's kernel trace of the replayed loop
        # reports, per dispatch, that PLUS the dispatch gap to its predecessor (its start stamp is taken when the packet is picked up,
        # before the barrier bit has waited the predecessor out: the sum of its durations over a step equals the step's wall time,
        # profiles/r03_bench_kernel_stats.csv: 1 002 of 1 016 us).  So the live figure that must agree with it is kernel-only + the
        # loop's average inter-kernel gap, measured here as (graph-replayed step time - sum of kernel-only intervals) / launches.
        # (Bracketing ONE kind per pass instead reads longer still — 19.8 vs 17.5 us on the MLP launch: the start stamp then sits
        # behind an undrained predecessor — and its sum over a step exceeds the step: not used.)
        eng.start_sequence(None)
        sp = eng._sampling(True, 1.0, args.top_k, 0.0, args.cfg_scale, 1234, first)
        eng.dec.noise = 0
        kinds = {"embed": 0, "qkv": 1, "attn": 2, "wo": 3, "w13": 4, "w2": 5, "heads": 6, "sample": 7}
        tot = (C.c_double * 8)()
        cnt = (C.c_int64 * 8)()
        eng.start_sequence(None)
        L.check(L.lib().vaura_profile_loop(C.byref(eng.dec), C.byref(sp), n_steps, 0xFF, tot, cnt,
                                           int(torch.cuda.current_stream().cuda_stream)), "vaura_profile_loop")
        eng.check_status()                       # vaura_profile_loop synchronised: a broken hand-off would make these intervals meaningless
        outl = (C.c_int64 * 8)()
        L.lib().vaura_profile_outliers(outl)     # intervals > 10x the kind's median (a stalled queue) are counted at the median
        n_out = int(sum(outl))
        per = {name: 1e3 * tot[bit] / max(1, cnt[bit]) for name, bit in kinds.items()}   # us per launch, kernel only
        launches = {name: int(cnt[bit]) for name, bit in kinds.items()}
        n_launch_step = sum(launches.values()) / n_steps
        gap_us = max(0.0, (1e3 * t_loop / n_steps - sum(per[k] * launches[k] for k in per) / n_steps) / n_launch_step)
        fused_mlp = launches["w2"] == 0 and launches["w13"] > 0     # csrc/mlp_engine.h: w1||w3 -> hand-off -> w2 in ONE launch, booked under w13
        if fused_mlp:
            per["mlp"], launches["mlp"] = per.pop("w13"), launches.pop("w13")
            per.pop("w2"), launches.pop("w2")
        total_us = {k: per[k] * launches[k] for k in per}
        # per-kind roofline fraction of the weight-streaming kernels; the DOMINANT kernel is the one with the largest total
        # time over the loop (launch count x average duration), not the largest per-launch byte count
        # ... and, in all layers but the last, the NEXT layer's qkv GEMV as its third phase (then qkv has one launch per step of its own)
        qkv_in_mlp = (1.0 - launches["qkv"] / launches["mlp"]) if fused_mlp and launches["qkv"] < launches["mlp"] else 0.0
        def alg_bytes(k):
            if k == "mlp":     # average over the step's launches
                return (algorithmic_bytes_per_launch("w13", cfg, wbytes, rows) + algorithmic_bytes_per_launch("w2", cfg, wbytes, rows)
                        + qkv_in_mlp * algorithmic_bytes_per_launch("qkv", cfg, wbytes, rows))
            return algorithmic_bytes_per_launch(k, cfg, wbytes, rows)
        gemv_kinds = ["qkv", "wo", "heads"] + (["mlp"] if fused_mlp else ["w13", "w2"])
        frac = {k: alg_bytes(k) / ((per[k] + gap_us) * 1e-6) / 1e9 / HBM_PEAK_GBS for k in gemv_kinds}
        kv_avg = 2.0 * rows * cfg.d_model * 4 * (n_steps + 1) / 2.0 + 2.0 * rows * cfg.d_model * 4     # K,V rows read (avg) + written
        frac["attn"] = kv_avg / ((per["attn"] + gap_us) * 1e-6) / 1e9 / HBM_PEAK_GBS
        dom = max(gemv_kinds + ["attn"], key=lambda k: total_us[k])
        ab = kv_avg if dom == "attn" else alg_bytes(dom)
        ach = ab / ((per[dom] + gap_us) * 1e-6) / 1e9          # dispatch-to-dispatch: what rocprofv3's kernel trace calls the duration
        names = json.load(open(os.path.join(REPO, "profiles", "kernel_names.json"))) if os.path.exists(
            os.path.join(REPO, "profiles", "kernel_names.json")) else {}
        nkey = "c4" if long_ctx else (f"{storage}_rows32" if rows > 16 and f"{storage}_rows32" in names else storage)
        kname = names.get(nkey, {}).get(dom, dom)
        if dom == "mlp" and not qkv_in_mlp:
            kname = names.get(nkey, {}).get("mlp_last", kname)
        # the committed rocprofv3 --kernel-trace --stats summary of this command (tools/profile_round.sh): its average duration of the
        # same kernel, quoted next to the live one so that the two can be seen to agree
        rocprof = None
        for cand in sorted((f for f in os.listdir(os.path.join(REPO, "profiles")) if f.endswith("_bench_kernel_stats.csv")), reverse=True):
            try:
                import csv
                for row in csv.DictReader(l for l in open(os.path.join(REPO, "profiles", cand)) if not l.startswith("#")):   # (the summary starts with a comment line)
                    if row.get("Name", "").replace("void ", "").split("(")[0].strip() == kname:
                        avg_us = float(row["AverageNs"]) * 1e-3
                        rocprof = {"source": f"profiles/{cand}", "measured_by": "builder: committed rocprofv3 summary, NOT measured by this run",
                                   "avg_us_per_launch": round(avg_us, 3), "calls": int(row["Calls"]),
                                   "frac": round(ab / (avg_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
                        break
            except Exception:
                continue
            if rocprof:
                break
        # HBM traffic of that kernel from the PMC passes over the SAME library (tools/pmc_driver.cpp + tools/profile_pmc.sh):
        # only quoted when the committed record is for this kernel instance and storage, else null
        traffic, tsrc = None, None
        for cand in sorted((f for f in os.listdir(os.path.join(REPO, "profiles"))
                            if f.endswith(f"_pmc_hbm_bytes_{storage}.json") or f.endswith(f"_pmc_hbm_bytes_{storage}_rows{rows}.json")), reverse=True):
            try:
                rec = json.load(open(os.path.join(REPO, "profiles", cand)))
                hit = rec.get("weights") == storage and rec.get("rows") == rows and rec.get("kernels", {}).get(kname)
                if hit:
                    traffic, tsrc = hit["hbm_bytes_per_launch"], f"profiles/{cand}"
                    break
            except Exception:
                continue
        out["roofline"] = {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": traffic,
                           "traffic_source": (f"{tsrc} (builder: committed PMC record, NOT measured by this run)" if tsrc else None),
                           "kernel": f"{kname} = {dom}", "dominant_by": "total time over the decode loop",
                           "stalled_intervals_counted_at_median": n_out, "rocprofv3_kernel_trace": rocprof,
                           "share_of_loop_kernel_time": round(total_us[dom] / sum(total_us.values()), 4),
                           "algorithmic_bytes_per_launch": ab, "avg_us_per_launch": round(per[dom] + gap_us, 3),
                           "avg_us_kernel_only": round(per[dom], 3), "inter_kernel_gap_us": round(gap_us, 3),
                           "launches_per_step": round(n_launch_step, 1),
                           "phases": (("w1||w3 + SwiGLU -> hand-off -> w2 + residual" + (" -> hand-off -> next layer's qkv (all layers but the last)" if qkv_in_mlp else "")
                                       + ", one launch (csrc/mlp_engine.h)") if dom == "mlp" else None),
                           "launches": launches[dom]}
        out["kernel_us"] = {k: round(v, 3) for k, v in per.items()}
        out["kernel_frac_of_hbm_peak"] = {k: round(v, 4) for k, v in frac.items()}

        # ---- the plugin surface (wall = generate() entry -> waveform): VAURAModel.generate() built from
        #      reference-style config dicts, same workload, next to the engine-level number above
        if not args.no_plugin and not long_ctx and args.weights == "auto":
            import warnings
            from vaura_amd.model import VAURAModel
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                model = VAURAModel(
                    feature_extractor_config={"target": "vaura_amd.feature_extractor.MotionFormer"},
                    audio_encoder_config={"target": "vaura_amd.codec.DacModelWrapper", "params": {"model_sr": 44100, "synthetic": True}},
                    sampler_config={"target": "vaura_amd.sampler.Transformer", "params": cfg.yaml_params()},
                    visual_bridge_config={"target": "torch.nn.Identity"},
                    pattern_provider_config={"target": "vaura_amd.patterns.DelayedPatternProvider", "params": {"n_q": 9}},
                    flatten_vis_feats=True, freeze_feature_extractor=True, noise_mode="philox", seed=1234)
            model.sampler.load_state_dict(sd, strict=True)
            model.sampler.audio_tokens_per_video_frame = 7
            model = model.to(dev)
            frames = feats.reshape(B, TV // 8, 8, cfg.cond_in)
            gkw = dict(frames=frames, audio=None, max_new_tokens=T_FRAMES, return_sampled_indices=True, use_sampling=True,
                       temp=1.0, top_k=args.top_k, top_p=0.0, prompt_is_encoded=True, cfg_scale=args.cfg_scale)
            for _ in range(2):
                r = model.generate(**gkw)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(reps):
                r = model.generate(**gkw)
            torch.cuda.synchronize(dev)
            t_plugin = (time.perf_counter() - t0) / reps
            assert r["generated_audio"].shape == (B, 1, T_FRAMES * HOP)
            out["plugin_surface"] = {"what": "vaura_amd.model.VAURAModel.generate() (plugin classes from config dicts), same workload, "
                                             f"storage {model.sampler.resolved_weight_dtype} (auto)",
                                     "ms_per_step": round(1e3 * t_plugin, 3),
                                     "tokens_per_s": round(B * K_CB * T_FRAMES / t_plugin, 1),
                                     "delta_ms_vs_engines": round(1e3 * t_plugin - (t_loop + t_codec), 3)}
            del model, r
            torch.cuda.empty_cache()

        # ---- the step BEFORE the hot path included (row f2): raw frames (B, 4, 3, 16, 224, 224) -> Segment-AVCLIP features ->
        #      decode loop -> codec, what scripts/generate.py:302-325 runs per batch.  Not in `value` (SURVEY.md 8d excludes
        #      feature extraction from the metric's wall time); reported beside it.
        if not long_ctx and not args.no_plugin:
            from vaura_amd.engine import AvclipEngine
            fx = AvclipEngine(synth.FULL_AVCLIP, synth.avclip_state_dict(seed=0), dev)
            frames = synth.video_frames(B, TV // 8, seed=0, first_clip=first).to(dev)

            def e2e():
                f = fx.forward(frames).reshape(B, TV, cfg.cond_in)
                return codec.decode(eng.generate_codes(f, T_FRAMES, **kw))
            for _ in range(2):
                e2e()
            torch.cuda.synchronize(dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            t0 = time.perf_counter()
            for _ in range(reps):
                ev[0].record()
                f = fx.forward(frames)
                ev[1].record()
                w = codec.decode(eng.generate_codes(f.reshape(B, TV, cfg.cond_in), T_FRAMES, **kw))
            ev[2].record()
            torch.cuda.synchronize(dev)
            t_e2e = (time.perf_counter() - t0) / reps
            eng.check_status()
            out["end_to_end_with_extractor"] = {"what": "raw frames -> Segment-AVCLIP (divided space-time ViT-B/16, 4 segments per clip) -> decode loop "
                                                        "-> DAC decode; engine level, same storage as `value`",
                                                "ms_per_step": round(1e3 * t_e2e, 3), "extractor_ms_last_step": round(ev[0].elapsed_time(ev[1]), 3),
                                                "tokens_per_s": round(B * K_CB * T_FRAMES / t_e2e, 1)}
            assert w.shape == (B, 1, T_FRAMES * HOP)
            del fx, frames, f, w
            torch.cuda.empty_cache()

        # ---- the OTHER BASELINE configs under the same clock: short timed regions (1 warm-up + 3 steps each, HIP events
        #      around loop and codec, status word checked after each), so that every headline bullet of README.md is a driver-run number.
        #      Each entry: value (tokens/s, loop + codec), ms_per_step, decode_loop_ms, codec_ms, decode_loop_roofline.frac.
        if world == 1 and not args.no_extra_configs and not long_ctx and args.weights == "auto" and args.checkpoint == "raw":
            out["extra_configs"] = extra_configs(args, dev, cfg, ccfg, sd, eng, codec, s_loop)

        if world == 1 and not args.no_cpu_baseline and not long_ctx:
            out["cpu_baseline"] = cpu_baseline(sd, feats_cpu, args.cfg_scale, B, args.top_k, quick=args.quick_cpu_baseline)
            out["gpu_over_cpu"] = round(out["value"] / out["cpu_baseline"]["value"], 1)

    if os.environ.get("VAURA_BENCH_SHARE_GPU") == "1" and world > 1:
        out["shared_gpu_control_flow_only"] = True      # ranks shared a GPU: the number says nothing about scaling
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        vdist.barrier()          # rank 0's extras above take a while: tear the group down together
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
