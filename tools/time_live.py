"""Live video in: VAURAModel.open_live against longform.generate_long_stream(block_frames=16) on the same features.  The full-size
synthetic model behind the plugin surface (pass-through extractor, synthetic codec), 8 clips, cfg 6, top-k 128, default engine (auto
storage: h1 on this checkpoint), Philox noise, 16 segments (10.24 s of video) pushed as fast as the session takes them.

Per pushed segment: host wall time from push() to its last returned block being complete on the device (a synchronisation behind the
call); the time from the first push to the first block of the session; the same two stamps for generate_long_stream in the same run.
Real-time requirement: the mean time per pushed segment is below the 640 ms one segment lasts — the record says whether it is met.
With ``--parity FILE``: whether the extractor on (B, 1) segments gives the rows of its (B, 4) call at this batch, appended to FILE.
    python tools/time_live.py [rounds] [output file] [--parity FILE]        -> profiles/live_timing.txt"""
import os
import statistics
import sys
import time
import warnings

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vaura_amd import longform, synth  # noqa: E402
from vaura_amd.model import VAURAModel  # noqa: E402

argv = list(sys.argv[1:])
PARITY = None
if "--parity" in argv:
    i = argv.index("--parity")
    PARITY = argv[i + 1]
    del argv[i:i + 2]
ROUNDS = int(argv[0]) if argv else 3
OUT = argv[1] if len(argv) > 1 else os.path.join(REPO, "profiles", "live_timing.txt")
DEV = "cuda:0"
B, S, BF = 8, 16, 16
KW = dict(use_sampling=True, temp=1.0, top_k=128, cfg_scale=6.0)
SEGMENT_MS = 640.0

cfg = synth.FULL_SAMPLER
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    model = VAURAModel(
        feature_extractor_config={"target": "vaura_amd.feature_extractor.MotionFormer", "params": {"extract_features": True}},
        audio_encoder_config={"target": "vaura_amd.codec.DacModelWrapper", "params": {"model_sr": 44100, "synthetic": True}},
        sampler_config={"target": "vaura_amd.sampler.Transformer", "params": cfg.yaml_params()},
        visual_bridge_config={"target": "torch.nn.Identity"},
        pattern_provider_config={"target": "vaura_amd.patterns.DelayedPatternProvider", "params": {"n_q": 9}},
        flatten_vis_feats=True, freeze_feature_extractor=True, noise_mode="philox", seed=1234)
model.sampler.load_state_dict(synth.sampler_state_dict(cfg, seed=0, round_bf16=True), strict=True)
model.sampler.audio_tokens_per_video_frame = 7
model = model.to(DEV)
feats = synth.video_features(B, S * 8, seed=0).reshape(B, S, 8, cfg.cond_in).to(DEV)
med = statistics.median


def sync():
    torch.cuda.synchronize()


def run_live():
    """-> (ms per push, ms from the first push to the first block, ms of close(), the blocks, blocks per push)"""
    s = model.open_live(B, block_frames=BF, **KW)
    per_push, counts, blocks, first = [], [], [], None
    sync()
    t_open = time.perf_counter()
    for i in range(S):
        t0 = time.perf_counter()
        got = s.push(features=feats[:, i])
        sync()                                   # the last returned block is complete on the device
        t1 = time.perf_counter()
        per_push.append(1e3 * (t1 - t0))
        if got and first is None:
            first = 1e3 * (t1 - t_open)          # a consumer that waits for the push; the block itself was due earlier inside it
        counts.append(len(got))
        blocks += got
    t0 = time.perf_counter()
    blocks += s.close()
    sync()
    return per_push, first, 1e3 * (time.perf_counter() - t0), blocks, counts


def run_long_stream():
    """-> (ms to the first block, ms to the last, the blocks)"""
    sync()
    t0 = time.perf_counter()
    first, blocks = None, []
    for blk in longform.generate_long_stream(model, feats, 0.64 * S, block_frames=BF, **KW):
        sync()
        first = first if first is not None else 1e3 * (time.perf_counter() - t0)
        blocks.append(blk)
    return first, 1e3 * (time.perf_counter() - t0), blocks


ref = longform.generate_long(model, feats, 0.64 * S, **KW)
n_frames = int(ref["sampled_indices"].shape[-1])
_, _, _, blocks, _ = run_live()                     # warm-up, and the contract on this configuration
assert torch.equal(torch.cat([b["sampled_indices"] for b in blocks], -1), ref["sampled_indices"])
assert torch.equal(torch.cat([b["audio"] for b in blocks], -1), ref["generated_audio"])
_, _, long_blocks = run_long_stream()
assert torch.equal(torch.cat([b["audio"] for b in long_blocks], -1), ref["generated_audio"])
live_runs = [run_live() for _ in range(ROUNDS)]
long_runs = [run_long_stream() for _ in range(ROUNDS)]
model.sampler.engine().check_status()

per_push = [med([r[0][i] for r in live_runs]) for i in range(S)]
first = med([r[1] for r in live_runs])
close = med([r[2] for r in live_runs])
mean = sum(per_push) / S
lines = [f"live session against generate_long_stream(block_frames={BF}); {B} clips, cfg {KW['cfg_scale']}, top-k {KW['top_k']}, storage "
         f"{model.sampler.engine().wdtype}, {S} segments = {0.64 * S:.2f} s of video = {n_frames} frames, median of {ROUNDS} after a warm-up, "
         "host wall time with the device idle at every stamp; tokens and audio bit-equal to generate_long in this run",
         f"device: {torch.cuda.get_device_name(0)}", "",
         "push -> its last returned block complete on the device, per pushed segment (pushed as fast as the session takes them):"]
for i, ms in enumerate(per_push):
    what = "chunk 0, incrementally" if i < 4 else f"chunk {i - 3}"
    lines.append(f"  segment {i:2d} ({what:22s}): {ms:8.1f} ms   ({live_runs[0][4][i]} blocks)")
lines += [f"  close()                              : {close:8.1f} ms",
          f"mean per pushed segment                : {mean:8.1f} ms   (one segment lasts {SEGMENT_MS:.0f} ms: real-time requirement "
          f"{'MET' if mean < SEGMENT_MS else 'NOT MET'}, {mean / SEGMENT_MS:.3f} of real time; slowest push {max(per_push):.1f} ms)",
          f"first push -> first block of the session: {first:8.1f} ms   (after ONE segment of video; {len(live_runs[0][3])} blocks in all)", "",
          f"generate_long_stream(block_frames={BF}) on the same features, the whole video given up front:",
          f"  call -> first block                  : {med([r[0] for r in long_runs]):8.1f} ms",
          f"  call -> last block                   : {med([r[1] for r in long_runs]):8.1f} ms   ({len(long_runs[0][2])} blocks; the session's "
          f"pushes and close sum to {sum(per_push) + close:.1f} ms)"]
text = "\n".join(lines)
print(text)
with open(OUT, "w") as f:
    f.write(text + "\n")

if PARITY:
    fx = model.visual_feature_extractor
    fx.load_state_dict(synth.avclip_state_dict(seed=0), strict=True)
    fx.to(DEV)
    video = synth.video_frames(B, 4, seed=5).to(DEV)
    four, _ = fx(video)
    one, _ = fx(video[:, :1].contiguous())
    line = (f"extractor on (B={B}, 1) segment vs the slice of its (B={B}, 4) call, full-size configuration: "
            f"{'bit-equal' if torch.equal(four[:, :1], one) else 'NOT bit-equal'}, max |diff| = {float((four[:, :1] - one).abs().max()):.3e}")
    print("live_parity:", line)
    with open(PARITY, "a") as f:
        f.write(line + "\n")
