"""Sliding-window generation for clips of different durations: ONE longform.generate_long_clips call against what it replaces, one
longform.generate_long call per distinct duration on the clips that have it (the same code as before generate_long_clips existed).
Production geometry (2.56 s window, 0.64 s stride, 25 video frames per second), the full-size synthetic model behind the plugin
surface (pass-through extractor, synthetic codec), 8 clips, cfg 6, top-k 128, default engine (auto storage), Philox noise.

Three mixes: 8 distinct durations, 2 distinct durations, 8 equal durations.  The durations are 2.56 + 0.64 k seconds: under guidance
generate_long serves only durations whose every chunk selects the window's 4 segments (the null embedding has 32 tokens), and the
baseline has to run.  Per mix: median host wall time of `rounds` calls after a warm-up call of each form (alternating), and the
share of (clip, chunk) slots of the one-call form that are parked (clip_chunk_plan).
    python tools/time_longform_clips.py [rounds]        -> profiles/longform_clips_timing.txt"""
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

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
DEV = "cuda:0"
B, N_SEG = 8, 16                              # 16 segments of 8 feature tokens = 10.24 s of video
MIXES = {
    "8 distinct": [3.20, 3.84, 4.48, 5.12, 5.76, 7.04, 8.32, 9.60],
    "2 distinct": [3.84] * 4 + [9.60] * 4,
    "8 equal": [7.04] * 8,
}
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


def one_call(durations):
    return longform.generate_long_clips(model, frames, durations, **KW)


def per_duration(durations):
    out = {}
    for d in sorted(set(durations)):
        rows = [b for b, x in enumerate(durations) if x == d]
        out[d] = longform.generate_long(model, frames[rows], d, **KW)
    return out


def timed(fn, *a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn(*a)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


lines = [f"generate_long_clips (one call) against one generate_long per distinct duration; {B} clips, cfg {KW['cfg_scale']}, top-k {KW['top_k']}, "
         f"storage {model.sampler.resolved_weight_dtype if hasattr(model.sampler, 'resolved_weight_dtype') else 'auto'}, "
         f"median of {ROUNDS} after a warm-up, host wall time incl. the codec decode",
         f"device: {torch.cuda.get_device_name(0)}", ""]
for name, durations in MIXES.items():
    plan = longform.clip_chunk_plan(durations, None, N_SEG)
    slots = sum(len(ch["parked"]) for ch in plan["chunks"])
    parked = sum(sum(ch["parked"]) for ch in plan["chunks"])
    live_calls = sum(len(set(d for d, cl in zip(durations, plan["clips"]) if c < len(cl["schedule"]))) for c in range(len(plan["chunks"])))
    one_call(durations), per_duration(durations)            # warm-up: engines, graphs, codec plans
    t_one, t_per = [], []
    for _ in range(ROUNDS):
        dt, r = timed(one_call, durations)
        t_one.append(dt)
        dt, ref = timed(per_duration, durations)
        t_per.append(dt)
    model.sampler.engine().check_status()
    assert r["lengths"].tolist() == [cl["length"] for cl in plan["clips"]]
    assert all(ref[d]["sampled_indices"].shape[-1] == L for d, L in zip(durations, r["lengths"].tolist()))
    a, b = statistics.median(t_one), statistics.median(t_per)
    audio_s = sum(r["audio_lengths"].tolist()) / 44100
    lines += [f"{name}: durations {durations}",
              f"  one generate_long_clips call : {1e3 * a:9.1f} ms   ({len(plan['chunks'])} generate_tokens calls of {B} clips; {audio_s / a:.2f} s of audio per s)",
              f"  generate_long per duration   : {1e3 * b:9.1f} ms   ({len(set(durations))} calls, {live_calls} generate_tokens calls; {audio_s / b:.2f} s of audio per s)",
              f"  one call / per duration      : {a / b:9.3f}",
              f"  parked (clip, chunk) slots   : {parked} of {slots} = {100.0 * parked / slots:.1f} %", ""]
text = "\n".join(lines)
print(text)
with open(os.path.join(REPO, "profiles", "longform_clips_timing.txt"), "w") as f:
    f.write(text + "\n")
