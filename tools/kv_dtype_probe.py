"""K/V cache types at configs[4]'s shape (16 clips, cfg 6, 32 rows, S = 229, full depth, fp8h weights): the 228-step loop time, the
per-layer attention launch time (per-launch events of one eager pass: vaura_profile_loop, kernel only) and teacher-forced logits against
the fp32 cache, all storages in one run.  GPU box.   python tools/kv_dtype_probe.py [--out FILE]"""
import argparse, ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, time
from vaura_amd import _lib as L, synth
from vaura_amd.engine import DecoderEngine
ap=argparse.ArgumentParser(); ap.add_argument("--out", default=None); ap.add_argument("--reps", type=int, default=5); args=ap.parse_args()
cfg=synth.FULL_SAMPLER; sd=synth.sampler_state_dict(cfg, seed=0, round_bf16=False)
f=synth.video_features(16, seed=0).cuda()
kw=dict(use_sampling=True, temp=1.0, top_k=250, cfg_scale=6.0, seed=1234)
s=torch.cuda.Stream()
idx=torch.randint(0,1024,(4,9,32)).cuda()
ref=None
lines=["# tools/kv_dtype_probe.py: 16 clips, cfg 6 (32 rows), T = 220 (S = 229, 228 steps), full depth; loop = graph-replayed generate_codes, mean of %d after a warm-up;" % args.reps,
       "# attn = mean kernel-only time of one attention launch (one per layer and step) over an eager pass; bytes = per cached vector"]
for wd,kv in (("fp8h","f32"),("fp8h","f16"),("fp8h","f8"),("fp8h","f8s"),("h2","f32")):
    e=DecoderEngine(cfg, sd, "cuda:0", wdtype=wd, kv_dtype=kv)
    with torch.cuda.stream(s):
        e.generate_codes(f,220,**kw); torch.cuda.synchronize()
        t0=time.perf_counter()
        for _ in range(args.reps): e.generate_codes(f,220,**kw)
        torch.cuda.synchronize()
        dt=(time.perf_counter()-t0)/args.reps*1e3
        e.check_status()
        # per-launch events on EVERY launch (mask 0xFF, as bench.py: bracketing one kind per pass reads longer), one eager pass of the same 228 steps
        e.start_sequence(None)
        sp=e._sampling(True, 1.0, 250, 0.0, 6.0, 1234, 0)
        e.dec.noise=0
        tot=(C.c_double*8)(); cnt=(C.c_int64*8)()
        L.check(L.lib().vaura_profile_loop(C.byref(e.dec), C.byref(sp), 228, 0xFF, tot, cnt, int(torch.cuda.current_stream().cuda_stream)), "vaura_profile_loop")
        e.check_status()
    attn_us=1e3*tot[2]/max(1,cnt[2])
    lg=e.logits_all_positions(idx, f[:4]).float().cpu()
    if ref is None: ref=lg
    line="%-5s kv %-4s bytes %3d  loop ms %8.2f  attn us/layer %6.2f (%d launches)  logits rel-rms vs fp8h/f32-KV %.3e" % (
        wd, kv, {"f32":384,"f16":192,"f8":96,"f8s":97}[kv], dt, attn_us, cnt[2], float((lg-ref).pow(2).mean().sqrt()/ref.pow(2).mean().sqrt()))
    print(line, flush=True); lines.append(line)
    del e; torch.cuda.empty_cache()
if args.out:
    with open(args.out,"w") as fh: fh.write("\n".join(lines)+"\n")
