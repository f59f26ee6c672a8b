"""Per-clip audio prompt lengths: ONE generate_tokens(prompt_lengths=[..]) call against what it replaces, one generate_tokens call per
distinct prompt length on the clips that have it (the same code as before the keyword existed).  The full-size synthetic model behind
the plugin surface (pass-through extractor), 8 clips, cfg 6, top-k 128, default engine (auto storage), Philox noise, T = 220 frames.

Three mixes: four distinct lengths (166 / 110 / 55 / 0, two clips each), eight distinct lengths, and all 166 (the scalar path: its
time must be the keyword-less call's).  Per mix: median host wall time of `rounds` calls after a warm-up call of each form
(alternating), the prefill positions the ragged call runs (sum over the groups of P_g + d_0) and their share of its time — the
groups' chunk sequences replayed alone on the finished sequence (vaura_prefill_rows, every group including the first, whose pass
inside the call is the loop's own prefill) between two events.
    python tools/time_prompt_lengths.py [rounds]        -> profiles/prompt_lengths_timing.txt"""
import ctypes as C
import os
import statistics
import sys
import time
import warnings

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import clip_params, synth  # noqa: E402
from vaura_amd.model import VAURAModel  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
DEV = "cuda:0"
B, T, K = 8, 220, 9
MIXES = {
    "4 distinct": [166, 166, 110, 110, 55, 55, 0, 0],
    "8 distinct": [166, 142, 118, 94, 70, 46, 22, 0],
    "8 equal": [166] * 8,
}
KW = dict(use_sampling=True, temp=1.0, top_k=128, cfg_scale=6.0, prompt_is_encoded=True, max_new_tokens=T)

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
frames = synth.video_features(B, 32, seed=0).reshape(B, 1, 32, cfg.cond_in).to(DEV)
prompt = torch.randint(0, cfg.d_codebook, (B, K, 166), generator=torch.Generator().manual_seed(1)).to(DEV)
eng = model.sampler.engine()


def one_call(P):
    return model.generate_tokens(frames=frames, audio=prompt, prompt_lengths=P, **KW)["tokens"]


def per_length(P):
    out = {}
    for p in sorted(set(P)):
        rows = [b for b, x in enumerate(P) if x == p]
        out[p] = model.generate_tokens(frames=frames[rows], audio=prompt[rows][..., :p] if p else None, **KW)
    return out


def timed(fn, *a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn(*a)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def passes_ms(P):
    """the groups' chunk sequences alone, on the sequence the ragged call left behind (every token known): device time between two events"""
    groups = sorted({p for p in P if p > 0})
    if not groups or eng.prompt_lengths is None or not eng.planes:
        return 0.0
    st = L.current_stream(eng.dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for n in groups:
        L.check(eng.lib.vaura_prefill_rows(C.byref(eng.dec), n, n, st), "vaura_prefill_rows")
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


lines = [f"generate_tokens(prompt_lengths=[..]) (one call) against one generate_tokens per distinct prompt length on its sub-batch; {B} clips, "
         f"T = {T}, cfg {KW['cfg_scale']}, top-k {KW['top_k']}, storage {eng.wdtype}, prefill chunks of {eng.PREFILL_POSITIONS} positions, "
         f"median of {ROUNDS} after a warm-up, host wall time, no codec",
         f"device: {torch.cuda.get_device_name(0)}", ""]
for name, P in MIXES.items():
    one_call(P), per_length(P)            # warm-up: engines, graphs
    t_one, t_per = [], []
    for _ in range(ROUNDS):
        dt, r = timed(one_call, P)
        t_one.append(dt)
        pre = passes_ms(P)
        dt, ref = timed(per_length, P)
        t_per.append(dt)
    eng.check_status()
    a, b = statistics.median(t_one), statistics.median(t_per)
    plan = clip_params.prompt_schedule(P, 0, T + K, cfg=True)
    npos = sum(e[1] for e in plan if e[0] == "prefill")
    steps = sum(e[1] for e in plan if e[0] == "steps")
    per_steps = sum(T + K - 1 - p for p in set(P))
    lines += [f"{name}: prompt lengths {P}",
              f"  one ragged call              : {1e3 * a:9.1f} ms   (1 loop of {steps} steps on {B} clips + {npos} prefill positions in {len(set(P)) - (0 in P)} passes)",
              f"  one call per distinct length : {1e3 * b:9.1f} ms   ({len(set(P))} calls, {per_steps} steps in all on {B // len(set(P))} clips each)",
              f"  ragged / per length          : {a / b:9.3f}"]
    if len(set(P)) == 1:
        lines += ["  (equal lengths take the scalar path: both forms are the keyword-less call on the whole batch)", ""]
    else:
        lines += [f"  prefill passes alone         : {pre:9.1f} ms = {100.0 * pre / (1e3 * a):.1f} % of the ragged call", ""]
text = "\n".join(lines)
print(text)
with open(os.path.join(REPO, "profiles", "prompt_lengths_timing.txt"), "w") as f:
    f.write(text + "\n")
