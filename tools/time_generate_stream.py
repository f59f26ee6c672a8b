"""Audio out of one generate() call while its decode loop still runs: VAURAModel.generate_stream against generate(), and
longform.generate_long_stream with and without block_frames.  The full-size synthetic model behind the plugin surface (pass-through
extractor, synthetic codec), 8 clips, cfg 6, top-k 128, default engine (auto storage: h1 on this checkpoint), Philox noise, T = 220.

Per block_frames: host wall time from the call to the moment the first block's samples are ready on the device (a synchronisation
behind the block), the same for the last block, both against generate() returning with its audio ready, re-measured in the same run;
the codec time of the blocks' windows (decode_window_seq on the finished sequence, summed) against the one decode pass.  Then
generate_long_stream at 10.24 s: first and last block with and without block_frames=16, against generate_long.
    python tools/time_generate_stream.py [rounds] [output file]        -> profiles/generate_stream_timing.txt"""
import os
import statistics
import sys
import time
import warnings

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vaura_amd import clip_params, longform, synth  # noqa: E402
from vaura_amd.codec_clips import decode_halo  # noqa: E402
from vaura_amd.model import VAURAModel  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "generate_stream_timing.txt")
DEV = "cuda:0"
B, T, K = 8, 220, 9
KW = dict(use_sampling=True, temp=1.0, top_k=128, cfg_scale=6.0, prompt_is_encoded=True)
LONG_KW = dict(use_sampling=True, temp=1.0, top_k=128, cfg_scale=6.0)

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
frames = synth.video_features(B, 4 * 8, seed=0).reshape(B, 4, 8, cfg.cond_in).to(DEV)
long_frames = synth.video_features(B, 16 * 8, seed=0).reshape(B, 16, 8, cfg.cond_in).to(DEV)
H = decode_halo(model.audio_encoder.cfg)
codec = model.audio_encoder.engine()


def sync():
    torch.cuda.synchronize()


def time_blocks(make, wait_each=True):
    """-> (seconds to the first block, to the last, the blocks' frames).  ``wait_each``: the consumer waits for every block's samples
    before it asks for the next one (the device idles while the host enqueues the next piece); False: it waits for the first and the
    last only, as a consumer that hands the blocks to another stream would."""
    sync()
    t0 = time.perf_counter()
    first, n = None, []
    for blk in make():
        if wait_each or first is None:
            sync()                               # the block's samples are on the device
        first = first if first is not None else time.perf_counter() - t0
        n.append(blk["frames"])
    sync()
    return first, time.perf_counter() - t0, n


def time_call(fn):
    sync()
    t0 = time.perf_counter()
    r = fn()
    sync()
    return time.perf_counter() - t0, r


def device_ms(fn, reps=5):
    fn()
    sync()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        sync()
        out.append(ev[0].elapsed_time(ev[1]))
    return statistics.median(out)


med = statistics.median
lines = [f"generate_stream against generate; {B} clips, T = {T}, cfg {KW['cfg_scale']}, top-k {KW['top_k']}, storage "
         f"{model.sampler.engine().wdtype}, halo {H} frames, median of {ROUNDS} after a warm-up, host wall time with the device idle at every stamp",
         f"device: {torch.cuda.get_device_name(0)}", ""]
whole = lambda: model.generate(frames=frames, max_new_tokens=T, return_sampled_indices=True, **KW)
whole()
t_gen, ref = zip(*[time_call(whole) for _ in range(ROUNDS)])
t_gen, ref = med(t_gen), ref[-1]
eng = model.sampler.engine()
n_steps = eng.S - 1
lines += [f"generate(), return with the audio ready     : {1e3 * t_gen:8.1f} ms   ({n_steps} sampled steps + one codec pass over {T} frames per clip)"]
codes = ref["sampled_indices"][..., :K, :]
one_pass = device_ms(lambda: codec.decode(codes))
lines += [f"codec alone, the one pass                   : {one_pass:8.2f} ms", ""]
for bf in (8, 16, 32, 64):
    stream = lambda: model.generate_stream(frames=frames, max_new_tokens=T, block_frames=bf, **KW)
    blocks = list(stream())
    assert torch.equal(torch.cat([b["audio"] for b in blocks], -1), ref["generated_audio"]), bf
    assert torch.equal(torch.cat([b["sampled_indices"] for b in blocks], -1), ref["sampled_indices"]), bf
    runs = [time_blocks(stream) for _ in range(ROUNDS)]
    first, last, n = med([r[0] for r in runs]), med([r[1] for r in runs]), runs[0][2]
    free = med([time_blocks(stream, wait_each=False)[1] for _ in range(ROUNDS)])
    pieces = clip_params.stream_schedule(T, None, 1, None, H, bf, num_codebooks=K)
    # the codec's share: the blocks' windows on the finished sequence, one at a time
    windows = 0.0
    decoded = 0
    for _, r in pieces:
        lo, hi = r[0]
        windows += device_ms(lambda: codec.decode_window_seq(eng.seq, [lo] * B, [hi - lo] * B))
        decoded += min(T, hi + H) - max(0, lo - H)
    due = pieces[0][0] + (pieces[1][0] if len(pieces) > 1 else 0)
    lines += [f"block_frames = {bf}: {len(blocks)} blocks of {n[0]} .. {n[-1]} frames; the first is yielded behind {pieces[0][0]} sampled steps, with "
              f"{due} enqueued (the next piece runs in front of the block's window)",
              f"  time to the first block's samples         : {1e3 * first:8.1f} ms   ({first / t_gen:.3f} of generate()'s return)",
              f"  time to the last block's samples          : {1e3 * last:8.1f} ms   ({last / t_gen:.3f}; {1e3 * (last - t_gen):+.1f} ms)",
              f"    without a wait between the blocks       : {1e3 * free:8.1f} ms   ({free / t_gen:.3f}; {1e3 * (free - t_gen):+.1f} ms)",
              f"  codec alone: the windows, summed          : {windows:8.2f} ms   ({decoded} frames per clip = {decoded / T:.3f} x; "
              f"{windows / one_pass:.3f} x the one pass, {windows - one_pass:+.2f} ms)", ""]
eng.check_status()

D = 10.24
long_ref = longform.generate_long(model, long_frames, D, **LONG_KW)
t_long = med([time_call(lambda: longform.generate_long(model, long_frames, D, **LONG_KW))[0] for _ in range(ROUNDS)])
lines += [f"generate_long_stream, {D} s ({long_ref['sampled_indices'].shape[-1]} frames): generate_long returns after {1e3 * t_long:8.1f} ms"]
for name, extra in (("block_frames=None", {}), ("block_frames=16", dict(block_frames=16))):
    stream = lambda: longform.generate_long_stream(model, long_frames, D, **LONG_KW, **extra)
    blocks = list(stream())
    assert torch.equal(torch.cat([b["audio"] for b in blocks], -1), long_ref["generated_audio"]), name
    runs = [time_blocks(stream) for _ in range(ROUNDS)]
    first, last, n = med([r[0] for r in runs]), med([r[1] for r in runs]), runs[0][2]
    free = med([time_blocks(stream, wait_each=False)[1] for _ in range(ROUNDS)])
    lines += [f"  {name}: {len(blocks)} blocks, the first of {n[0]} frames",
              f"    time to the first block's samples       : {1e3 * first:8.1f} ms   ({first / t_long:.3f} of generate_long's return)",
              f"    time to the last block's samples        : {1e3 * last:8.1f} ms   ({last / t_long:.3f}; {1e3 * (last - t_long):+.1f} ms)",
              f"      without a wait between the blocks     : {1e3 * free:8.1f} ms   ({free / t_long:.3f}; {1e3 * (free - t_long):+.1f} ms)"]
model.sampler.engine().check_status()
text = "\n".join(lines)
print(text)
with open(OUT, "w") as f:
    f.write(text + "\n")
