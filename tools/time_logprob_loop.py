"""The 228-step decode loop of BASELINE configs[1] (8 clips x 2.56 s, T = 220, top-k 250, temperature 1, cfg 6, un-rounded checkpoint,
storage "auto") through DecoderEngine.generate_codes, timed with HIP events around 5 batches enqueued back to back (median of
--repeat such regions):    python tools/time_logprob_loop.py [--package-root D] [--repeat R] [--relevance]

  plain            return_logprobs=False: the sampler instances without log-probabilities
  logprobs         return_logprobs=True: sample_kernel<PC, LP = true> + the float revert + vaura_sequence_logprob
  candidates 2x4   num_candidates=4 at B = 2 (the same 8 sequences, 16 decoder rows; the condition MLP on 2 clips) with log-probabilities
  --relevance adds (where the tree has it):
  relevance        return_relevance=True at cfg 6: the mode-2 sampler + three float reverts, one subtraction, vaura_sequence_logprob
  both             return_logprobs and return_relevance
  relevance cfg1   return_relevance=True at cfg 1 next to "plain cfg1": the null rows are carried for the flag alone (twice the rows)

  --lengths adds (where the tree has them):
  lengths = T      max_new_tokens=[220] * 8, video_lengths=[32] * 8: the per-clip-length instances (sample_kernel<.., SampleLengths>,
                   embed_clips_kernel, the _clips pattern kernels) on the shape of "plain" — what the two integer loads per workgroup cost
  lengths ragged   max_new_tokens=[220, 110, 55, 220, 165, 28, 110, 220]: the same loop (a finished clip rides along to S)
  codec 1 / 2 / 4  CodecEngine.decode of 8 clips x 220 frames in one pass, and grouped as generate() groups a ragged batch: two lengths
                   (4 x 220 + 4 x 110) and four (2 x 220 + 2 x 165 + 2 x 110 + 2 x 55), median of 20 after 3 warm-ups

--package-root D imports vaura_amd from D (another build of the library, e.g. the parent commit): modes that tree does not have are
skipped, so the plain line of two trees can be taken in one session on one card."""
import argparse
import inspect
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--relevance", action="store_true")
ap.add_argument("--lengths", action="store_true")
args = ap.parse_args()
import torch  # noqa: E402
sys.path.insert(0, os.path.abspath(args.package_root))
from vaura_amd import synth  # noqa: E402
from vaura_amd.engine import DecoderEngine  # noqa: E402

dev = torch.device("cuda:0")
cfg = synth.FULL_SAMPLER
eng = DecoderEngine(cfg, synth.sampler_state_dict(cfg, seed=0, round_bf16=False), dev)
kw = dict(use_sampling=True, temp=1.0, top_k=250, cfg_scale=6.0, seed=1)
has_lp = "return_logprobs" in inspect.signature(eng.generate_codes).parameters
modes = [("plain", 8, {})]
if has_lp:
    modes += [("logprobs", 8, dict(return_logprobs=True)), ("candidates 2x4", 2, dict(return_logprobs=True, num_candidates=4))]
if args.relevance and "return_relevance" in inspect.signature(eng.generate_codes).parameters:
    modes += [("relevance", 8, dict(return_relevance=True)), ("both", 8, dict(return_logprobs=True, return_relevance=True)),
              ("plain cfg1", 8, dict(cfg_scale=1.0)), ("relevance cfg1", 8, dict(cfg_scale=1.0, return_relevance=True))]
has_len = args.lengths and "video_lengths" in inspect.signature(eng.generate_codes).parameters
if has_len:
    modes += [("lengths = T", 8, dict(T=[220] * 8, video_lengths=[32] * 8)), ("lengths ragged", 8, dict(T=[220, 110, 55, 220, 165, 28, 110, 220]))]
print(f"tree {os.path.abspath(args.package_root)}: storage {eng.wdtype}, 228 steps per batch, 5 batches per region, {args.repeat} regions")
s = torch.cuda.Stream(dev)
with torch.cuda.stream(s):
    for name, clips, extra in modes:
        feats = synth.video_features(clips, seed=0).to(dev)
        extra = dict(extra)
        T = extra.pop("T", 220)
        for _ in range(2):
            eng.generate_codes(feats, T, **dict(kw, **extra))
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                eng.generate_codes(feats, T, **dict(kw, **extra))
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / 5)
        eng.check_status()        # a broken hand-off / non-finite logits would make these times meaningless: fail instead
        ms.sort()
        print(f"{name:16s} {ms[len(ms) // 2]:8.3f} ms per batch (median; min {ms[0]:.3f}, max {ms[-1]:.3f}) = {ms[len(ms) // 2] / 228 * 1e3:7.2f} us per step")

if has_len:
    from vaura_amd.engine import CodecEngine  # noqa: E402
    ccfg = synth.FULL_CODEC
    codec = CodecEngine(ccfg, synth.codec_state_dict(ccfg, seed=0), dev)
    codes = torch.randint(0, 1024, (8, 9, 220), generator=torch.Generator().manual_seed(0)).to(dev)
    for name, groups in (("codec 1 length", [(8, 220)]), ("codec 2 lengths", [(4, 220), (4, 110)]),
                         ("codec 4 lengths", [(2, 220), (2, 165), (2, 110), (2, 55)])):
        ms = []
        with torch.cuda.stream(s):
            for i in range(23):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for n, Tg in groups:
                    codec.decode(codes[:n, :, :Tg])
                e1.record()
                torch.cuda.synchronize()
                if i >= 3:
                    ms.append(e0.elapsed_time(e1))
        ms.sort()
        print(f"{name:16s} {ms[len(ms) // 2]:8.3f} ms (median of 20; min {ms[0]:.3f}, max {ms[-1]:.3f})")
