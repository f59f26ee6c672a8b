"""Windowed codec decode: longform.generate_long_stream (audio out chunk by chunk, one vaura_dac_decode_window pass per block) against
longform.generate_long (every token first, then ONE codec pass), whose default path this work does not change.
Production geometry (2.56 s window, 0.64 s stride, 25 video frames per second), the full-size synthetic model behind the plugin
surface (pass-through extractor, synthetic codec), 8 clips, cfg 6, top-k 128, default engine (auto storage), Philox noise: the shape of
tools/time_longform_clips.py.

Per duration: (a) host wall time to the first yielded block and to the last, at emit_chunks 1 and 4, against generate_long's single
return; (b) the codec alone: the stream's window calls summed against the one pass over the same tokens; (c) the codec workspace of
both routes (4 buffers of fp32).  Median of `rounds` after a warm-up of each form; the device is idle at every time stamp, so a
stream pays one host-device synchronisation per block here that a consumer overlapping its own work would not.
    python tools/time_codec_window.py [rounds]        -> profiles/codec_window_timing.txt"""
import ctypes as C
import os
import statistics
import sys
import time
import warnings

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vaura_amd import longform, synth  # noqa: E402
from vaura_amd.codec_clips import decode_halo  # noqa: E402
from vaura_amd.model import VAURAModel  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
DEV = "cuda:0"
B, N_SEG = 8, 16                              # 16 segments of 8 feature tokens = 10.24 s of video; longer durations wrap
DURATIONS = [10.24, 30.72]
KW = dict(use_sampling=True, temp=1.0, top_k=128, cfg_scale=6.0)

cfg = synth.FULL_SAMPLER
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    model = VAURAModel(
        feature_extractor_config={"target": "vaura_amd.feature_extractor.MotionFormer"},
        audio_encoder_config={"target": "vaura_amd.codec.DacModelWrapper", "params": {"model_sr": 44100, "synthetic": True}},
        sampler_config={"target": "vaura_amd.sampler.Transformer", "params": cfg.yaml_params()},
        visual_bridge_config={"target": "torch.nn.Identity"},
        pattern_provider_config={"target": "vaura_amd.patterns.DelayedPatternProvider", "params": {"n_q": 9}},
        flatten_vis_feats=True, freeze_feature_extractor=True, noise_mode="philox", seed=1234)
model.sampler.load_state_dict(synth.sampler_state_dict(cfg, seed=0, round_bf16=True), strict=True)
model.sampler.audio_tokens_per_video_frame = 7
model = model.to(DEV)
frames = synth.video_features(B, N_SEG * 8, seed=0).reshape(B, N_SEG, 8, cfg.cond_in).to(DEV)
K, H = model.num_codebooks, decode_halo(model.audio_encoder.cfg)


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def one_return(d):
    t0 = sync_time()
    r = longform.generate_long(model, frames, d, **KW)
    return sync_time() - t0, r


def stream(d, emit):
    """-> (seconds to the first block, seconds to the last, [(start_frame, frames)])"""
    t0 = sync_time()
    stamps, blocks = [], []
    for blk in longform.generate_long_stream(model, frames, d, emit_chunks=emit, **KW):
        stamps.append(sync_time() - t0)
        blocks.append((blk["start_frame"], blk["frames"]))
    return stamps[0], stamps[-1], blocks


def codec_only(tokens, blocks):
    """-> (seconds of the one pass, seconds of the window calls summed), each call timed with the device idle at both ends"""
    codec = model.audio_encoder
    codes = tokens[..., :K, :].contiguous()
    t0 = sync_time()
    codec.decode([(codes, None)])
    one = sync_time() - t0
    total = 0.0
    for s, n in blocks:
        t0 = sync_time()
        codec.decode_window(codes, [s] * B, [n] * B)
        total += sync_time() - t0
    return one, total


def workspace_bytes(T, blocks):
    eng = model.audio_encoder.engine()
    i32 = lambda v: (C.c_int32 * B)(*v)
    whole = eng.lib.vaura_dac_workspace_elems(C.byref(eng.c), B, T)
    window = max(eng.lib.vaura_dac_decode_window_workspace_elems(C.byref(eng.c), B, i32([T] * B), i32([s] * B), i32([n] * B)) for s, n in blocks)
    return 16 * whole, 16 * window


med = statistics.median
lines = [f"generate_long_stream against generate_long; {B} clips, cfg {KW['cfg_scale']}, top-k {KW['top_k']}, halo {H} frames, "
         f"median of {ROUNDS} after a warm-up, host wall time with the device idle at every stamp",
         f"device: {torch.cuda.get_device_name(0)}", ""]
for d in DURATIONS:
    n_chunks = len(longform.chunk_schedule(d))
    one_return(d), stream(d, 1), stream(d, 4)                  # warm-up: engines, graphs, workspaces
    t_ref, runs = [], {1: [], 4: []}
    for _ in range(ROUNDS):
        dt, ref = one_return(d)
        t_ref.append(dt)
        for emit in runs:
            runs[emit].append(stream(d, emit))
    model.sampler.engine().check_status()
    T = int(ref["sampled_indices"].shape[-1])
    lines += [f"duration {d} s: {T} frames, {n_chunks} chunks",
              f"  generate_long, single return          : {1e3 * med(t_ref):9.1f} ms"]
    for emit, rs in runs.items():
        blocks = rs[-1][2]
        frames_decoded = sum(min(T, s + n + H) - max(0, s - H) for s, n in blocks)
        codec = [codec_only(ref["sampled_indices"], blocks) for _ in range(ROUNDS + 1)][1:]
        one, win = med([c[0] for c in codec]), med([c[1] for c in codec])
        ws_whole, ws_window = workspace_bytes(T, blocks)
        first, last = med([r[0] for r in rs]), med([r[1] for r in rs])
        lines += [f"  stream, emit_chunks={emit}: {len(blocks)} blocks, first of {blocks[0][1]} frames",
                  f"    (a) time to the first block          : {1e3 * first:9.1f} ms   ({first / med(t_ref):.3f} of generate_long's return)",
                  f"        time to the last block           : {1e3 * last:9.1f} ms   ({last / med(t_ref):.3f}; {1e3 * (last - med(t_ref)):+.1f} ms)",
                  f"    (b) codec alone: one pass            : {1e3 * one:9.2f} ms   ({T} frames per clip)",
                  f"        codec alone: the windows, summed : {1e3 * win:9.2f} ms   ({frames_decoded} frames per clip = {frames_decoded / T:.3f} x; "
                  f"{win / one:.3f} x the time, {1e3 * (win - one):+.2f} ms)",
                  f"    (c) codec workspace: one pass        : {ws_whole / 2 ** 20:9.1f} MiB",
                  f"        codec workspace: widest window   : {ws_window / 2 ** 20:9.1f} MiB   ({ws_window / ws_whole:.4f})"]
    lines.append("")
text = "\n".join(lines)
print(text)
with open(os.path.join(REPO, "profiles", "codec_window_timing.txt"), "w") as f:
    f.write(text + "\n")
