"""Time of one sampler launch per mode (op-level vaura_sample, back to back on one stream): python tools/time_sampler.py

--clips B        clips per launch (default 8; the CFG modes carry 2 B rows: 8 -> 16 rows, 16 -> 32 rows)
--per-clip       time the per-clip instance (vaura_sample_clips, B records holding the same parameters) next to the scalar one,
                 both as 200 launches of one captured graph
--logprobs       add the LP column: the same launch through vaura_sample_logprobs (sample_kernel<PC, LP = true>: the token's log-probability
                 kept and stored), eager and, with --per-clip, inside the captured graph
--relevance      add the mode-2 column: the same launch through vaura_sample_relevance (sample_kernel<PC, true, SampleRelevance>: lp plus the
                 token's log-probability under the conditional and the null row); the cfg1 line has no null rows and shows none.  With
                 --package-root of a build without the entry point the column is left out (modes 0 and 1 of that build are the A/B)
--repeat R       print R lines per mode (run-to-run spread)
--package-root D import vaura_amd from D instead of this tree (A/B against another build of the library)"""
import argparse, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--clips", type=int, default=8)
ap.add_argument("--per-clip", action="store_true")
ap.add_argument("--logprobs", action="store_true")
ap.add_argument("--relevance", action="store_true")
ap.add_argument("--repeat", type=int, default=1)
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
import torch
sys.path.insert(0, os.path.abspath(args.package_root))
from vaura_amd import _lib as L
import ctypes as C
lib = L.lib()
dev = "cuda:0"
B, K, V = args.clips, 9, 1024
logits = torch.randn(2 * B, K * V, device=dev) * 3
tokens = torch.zeros(B * K, dtype=torch.int32, device=dev)
logprobs = torch.zeros(B * K, dtype=torch.float32, device=dev)
lcond, lnull = torch.zeros_like(logprobs), torch.zeros_like(logprobs)
has_rel = "vaura_sample_relevance" in L.SIGNATURES
def run(use_sampling, top_k, top_p, cfg, tie_eps=0.0, per_clip=False, graph=False, lp=False, rel=False):
    sp = L.Sampling()
    sp.use_sampling, sp.top_k, sp.temp, sp.top_p, sp.cfg_scale, sp.seed, sp.clip_base, sp.input_is_probs = use_sampling, top_k, 1.0, top_p, cfg, 1, 0, 0
    sp.tie_eps = tie_eps          # near-tie screen (round 6): 0 = off
    rec = None
    if per_clip:                  # the same parameters, from B device records (include/vaura_hip.h vaura_clip_sampling)
        from vaura_amd import clip_params
        rec = clip_params.pack_records(clip_params.resolve(B, [use_sampling] * B, 1.0, top_k, top_p, cfg))
        rec = torch.frombuffer(bytearray(rec), dtype=torch.int32).to(dev)
        launch = lambda i: lib.vaura_sample_clips(L.ptr(logits), B, K, V, C.byref(sp), L.ptr(rec), None, i, L.ptr(tokens), None, 0, 0, None, L.current_stream(torch.device(dev)))
    if lp:                        # LP = true instances (records or scalars)
        launch = lambda i: lib.vaura_sample_logprobs(L.ptr(logits), B, K, V, C.byref(sp), L.ptr(rec), None, i, L.ptr(tokens), None, 0, 0, None, L.ptr(logprobs), L.current_stream(torch.device(dev)))
    if rel:                       # mode 2 (records or scalars): lp, lc, lu
        launch = lambda i: lib.vaura_sample_relevance(L.ptr(logits), B, K, V, C.byref(sp), L.ptr(rec), None, i, L.ptr(tokens), None, 0, 0, None, L.ptr(logprobs), L.ptr(lcond), L.ptr(lnull), L.current_stream(torch.device(dev)))
    elif not lp and not per_clip:
        launch = lambda i: lib.vaura_sample(L.ptr(logits), B, K, V, C.byref(sp), None, i, L.ptr(tokens), L.current_stream(torch.device(dev)))
    s = torch.cuda.Stream()
    if graph:
        # vaura_sample_clips reads its records back before it launches (one copy + a wait per call), except while its stream is being
        # captured: the decode loop replays a captured step, so the per-clip INSTANCE is timed the same way, N launches in one graph
        with torch.cuda.stream(s):
            for _ in range(5):
                assert launch(0) == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for i in range(200):
                assert launch(i) == 0
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 2000 * 1000
    with torch.cuda.stream(s):
        for _ in range(50):
            assert launch(0) == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(2000):
            launch(i)
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 2000 * 1000
for _ in range(args.repeat):
    for name, a in (("greedy cfg6", (0, 0, 0.0, 6.0)), ("plain sampling cfg6", (1, 0, 0.0, 6.0)), ("top-k 250 cfg6", (1, 250, 0.0, 6.0)), ("top-p 0.9 cfg6", (1, 0, 0.9, 6.0)), ("top-k 250 cfg1", (1, 250, 0.0, 1.0))):
        line = f"{name}: {run(*a):.2f} us per launch (back to back, includes the dispatch gap); with the near-tie screen (tie_eps 1.5e-6): {run(*a, 1.5e-6):.2f}"
        if args.per_clip:
            line += (f"; 200 launches in one captured graph: scalar {run(*a, graph=True):.2f}, per-clip records {run(*a, per_clip=True, graph=True):.2f}"
                     f"; with the screen: scalar {run(*a, 1.5e-6, graph=True):.2f}, per-clip records {run(*a, 1.5e-6, True, True):.2f}")
        if args.logprobs:
            line += f"; LP (vaura_sample_logprobs): {run(*a, lp=True):.2f}"
            if args.per_clip:
                line += f", in the graph: scalar {run(*a, graph=True, lp=True):.2f}, per-clip records {run(*a, per_clip=True, graph=True, lp=True):.2f}"
        if args.relevance and has_rel and a[3] > 1.0:
            line += f"; relevance (vaura_sample_relevance): {run(*a, rel=True):.2f}"
            if args.per_clip:
                line += f", in the graph: scalar {run(*a, graph=True, rel=True):.2f}, per-clip records {run(*a, per_clip=True, graph=True, rel=True):.2f}"
        print(f"[{B} clips] {line}" if (args.clips != 8 or args.per_clip or args.repeat > 1) else line)
