"""Live video in: a session takes the video one segment at a time and hands out audio blocks while it does.

``generate()``, ``generate_stream()`` and ``longform.generate_long_stream()`` take the frames of the whole clip.  The model needs less:
the decoder reads video only in the embed of a step — position p takes condition token p // tokens_per_frame (csrc/step.hip) —, the
extractor works segment by segment (16 frames -> 8 tokens), and chunk c >= 1 of the sliding window needs the segments c .. c + 3 only.

    s = model.open_live(batch, block_frames=16, use_sampling=..., temp=..., top_k=..., top_p=..., cfg_scale=...)
    blocks = s.push(features=seg)      # (B, 1, 8, 768) or (B, 8, 768): one segment of extractor output
    blocks = s.push(frames=seg)        # (B, 1, C, 16, H, W): one segment of extractor input (model.frames_from_video of 16 frames)
    blocks = s.close()                 # the last blocks; "final" True on the last one

Frames that arrive one at a time, or at another rate than 25 fps, become such segments in ``model.open_video_stream(...)``
(``preprocess.VideoFrameStream``): ``for seg in vs.push(frames, pts): blocks += s.push(frames=seg)``.

A session runs the UNBOUNDED chunk schedule (``live_plan``): chunk 0 is a full window without a prompt over the segments 0 .. W - 1,
chunk c >= 1 starts ``stride_tokens`` frames later, is prompted with the tail of chunk c - 1 and reads the segments c .. c + W - 1 —
what ``longform.chunk_schedule`` gives for every duration of W + 1 segments or more, whose last chunk is again a full window.
Chunk 0 runs incrementally: with V condition tokens received the loop runs exactly the steps whose embed reads a token < V
(``clip_params.video_step_bound``), in the pieces of ``clip_params.live_schedule`` on the one captured step; the tokens that have not
arrived are NaN in the condition buffer, so a read ahead of the video would show in the status word.  Chunk c >= 1 runs when segment
c + W - 1 is pushed, as the call ``longform._stream_chunk`` makes for the long-form stream.  Frames leave by the long-form rule on
global frames: final in every codebook and one codec halo behind the last final frame (``longform._Held``).

Contract (tests/test_gpu_live.py; every comparison is ``torch.equal``): the blocks of a session closed after S >= W + 1 segments
concatenate to ``generate_long(model, feats[:, :S], stride * S)``'s tokens, relevance values and audio; for every close point the audio
is the codec's one decode of the session's own tokens; a session closed inside chunk 0 emits the prefix of
``generate_stream(max_new_tokens=T0)`` on the received segments followed by NaN segments that the bound gives.
Not built: the prompt prefill of chunk c + 1 overlapped with the wait for the next segment (it reads the segments c + 1 .. c + W - 1
only, so it is possible); per-clip lengths or prompts (all clips share the live clock); codec state carried across blocks; the
window's condition shifted in place for chunk c >= 1 (``DecoderEngine.append_condition(shift_tokens=...)`` does it, the chunk's call
projects its four segments again: 32 rows through the MLP); container or camera I/O.
"""
from __future__ import annotations

from math import ceil
from typing import List, Optional

import torch

from . import clip_params
from ._lib import VauraHipError
from .engine import off_null_stream
from .longform import COMPRESSION_MODEL_FRAME_RATE, REL, _Held, _decode_halo, _error, _stream_chunk, chunk_schedule


# ---- the unbounded chunk schedule: pure bookkeeping, no tensors
def live_plan(model_max_duration: float = 2.56, stride: float = 0.64, vfps: float = 25, segment_frames: int = 16) -> dict:
    """The chunk schedule of a session, read off ``chunk_schedule`` for W + 2 segments (three chunks; W = the segments of a full
    window): {"window": W, "first": frames of chunk 0, "full": frames of chunk c >= 1, "prompt": its prompt length, "stride_tokens":
    the frames it advances by, "new": the frames it generates}.  Refused unless that schedule IS one segment per chunk: chunk c at
    offset c * stride_tokens over the segments c .. c + W - 1, every chunk a full window."""
    W = ceil(model_max_duration * vfps) // int(segment_frames)
    if W < 1:
        raise _error(f"live_plan: a window of {model_max_duration} s at {vfps} fps holds no {segment_frames}-frame segment")
    sched = chunk_schedule(stride * (W + 2), model_max_duration, stride, vfps)
    st = int(COMPRESSION_MODEL_FRAME_RATE * stride)
    ok = len(sched) == 3 and sched[0]["prompt_len"] == 0 and sched[1]["max_gen_len"] == sched[2]["max_gen_len"] \
        and sched[1]["prompt_len"] == sched[2]["prompt_len"] == sched[0]["max_gen_len"] - st == sched[1]["max_gen_len"] - st \
        and all(ch["offset"] == c * st and ch["positions"] == (c, c + W) for c, ch in enumerate(sched))
    if not ok:
        raise _error(f"live_plan: a session advances by one {segment_frames}-frame segment per chunk; stride {stride} s at {vfps} fps under a "
                     f"window of {model_max_duration} s does not give that schedule ({sched})")
    return dict(window=W, first=sched[0]["max_gen_len"], full=sched[1]["max_gen_len"], prompt=sched[1]["prompt_len"], stride_tokens=st,
                new=sched[1]["new_tokens"])


def live_chunk(plan: dict, c: int) -> dict:
    """Chunk ``c`` of the unbounded schedule, in the form ``chunk_schedule`` lists its chunks."""
    if c == 0:
        return dict(offset=0, max_gen_len=plan["first"], prompt_len=0, positions=(0, plan["window"]), new_tokens=plan["first"])
    return dict(offset=c * plan["stride_tokens"], max_gen_len=plan["full"], prompt_len=plan["prompt"], positions=(c, c + plan["window"]),
                new_tokens=plan["new"])


def check_open(batch, block_frames, *, num_candidates=1, prompt_lengths=None, audio_lengths=None, max_new_tokens=None, video_lengths=None,
               near_tie=None) -> None:
    """What ``open_live`` refuses, on the host alone."""
    if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
        raise _error(f"open_live: batch must be a positive number of clips, got {batch!r}")
    clip_params.check_block_frames(block_frames)
    if isinstance(num_candidates, bool) or not isinstance(num_candidates, int) or num_candidates != 1:
        raise _error(f"a live session takes num_candidates = 1 (got {num_candidates!r}): the winning candidate is known only at the end of "
                     "a call, after audio has left")
    if prompt_lengths is not None or audio_lengths is not None or video_lengths is not None or max_new_tokens is not None:
        raise _error("a live session takes no prompt_lengths / audio_lengths, max_new_tokens or video_lengths: all clips of a session "
                     "share the live clock — one segment per push for every clip, until close()")
    if near_tie == "rerun":
        raise _error('a live session is refused on a sampler with near_tie="rerun": the re-run is decided at the end of a call, after '
                     'audio has left (use "report" or "off")')


def check_push(features, frames, batch: int, seg_tokens: int, cond_in: int, segment_frames: int, closed: bool) -> str:
    """What ``push`` refuses, from the shapes alone -> "features" | "frames"."""
    if closed:
        raise _error("push after close(): the session has handed out its last block")
    if (features is None) == (frames is None):
        raise _error("push takes one segment: either features= (extractor output) or frames= (extractor input), not both and not neither")
    if features is not None:
        shape = tuple(features.shape)
        if shape not in ((batch, 1, seg_tokens, cond_in), (batch, seg_tokens, cond_in)):
            raise _error(f"push(features=...): one segment is ({batch}, 1, {seg_tokens}, {cond_in}) or ({batch}, {seg_tokens}, {cond_in}), "
                         f"got {shape}")
        return "features"
    shape = tuple(frames.shape)
    if len(shape) != 6 or shape[0] != batch or shape[1] != 1 or shape[3] != segment_frames:
        raise _error(f"push(frames=...): one segment is ({batch}, 1, C, {segment_frames}, H, W), got {shape}")
    return "frames"


class LiveBook:
    """The host bookkeeping of a session — ints only, whatever the number of segments pushed: which work a push runs and which
    global frame ranges leave with it.  ``push()`` -> (work, releases): work = ("steps", [(n_steps, lo, hi), ...]) inside chunk 0
    (``clip_params.live_schedule``; possibly no piece) or ("chunk", c, ``live_chunk(plan, c)``); releases = [(lo, hi), ...], the
    blocks in order.  ``close()`` -> the last release or None."""

    def __init__(self, plan: dict, delays: List[int], block_frames: int, tokens_per_frame: int, seg_tokens: int, halo: int):
        self.plan, self.delays, self.block_frames, self.halo = plan, list(delays), int(block_frames), int(halo)
        self.first_step = 1 + self.delays[0]               # no prompt in chunk 0
        self.pieces = clip_params.live_schedule(plan["first"], self.first_step, self.delays, block_frames, tokens_per_frame,
                                                plan["window"] * seg_tokens, seg_tokens)
        assert len(self.pieces) == plan["window"]
        start = plan["prompt"] + 1 + self.delays[0]
        self.chunk_ranges = [r[0] for _, r in clip_params.stream_schedule(plan["full"], None, start, self.delays, 0, block_frames)
                             if r[0][1] > r[0][0]]
        self.segments = self.known = self.emitted = 0
        self.closed = False

    def _release(self, known: int, out: list):
        self.known = known
        if known - self.halo > self.emitted:
            out.append((self.emitted, known - self.halo))
            self.emitted = known - self.halo

    def push(self):
        if self.closed:
            raise _error("push after close(): the session has handed out its last block")
        self.segments += 1
        W, out = self.plan["window"], []
        if self.segments <= W:
            work = ("steps", [(n, lo, hi) for n, (lo, hi) in self.pieces[self.segments - 1]])
            for _, lo, hi in work[1]:
                if hi > lo:
                    self._release(hi, out)
            return work, out
        c = self.segments - W
        ch = live_chunk(self.plan, c)
        for _, hi in self.chunk_ranges:
            self._release(ch["offset"] + max(hi, ch["prompt_len"]), out)
        return ("chunk", c, ch), out

    def close(self):
        if self.closed:
            raise _error("close() after close(): the session has handed out its last block")
        self.closed = True
        if self.known > self.emitted:
            out = (self.emitted, self.known)
            self.emitted = self.known
            return out
        return None


# ---- the session
def open_live(model, batch: int, block_frames: int = 16, *, use_sampling: bool = True, temp: float = 1.0, top_k: int = 128, top_p: float = 0.0,
              cfg_scale: float = 1.0, return_relevance: bool = False, clip_indices=None, stride: float = 0.64, vfps: float = 25,
              model_max_duration: Optional[float] = None, num_candidates: int = 1, prompt_lengths=None, audio_lengths=None,
              max_new_tokens=None, video_lengths=None, return_attention_weights: bool = False) -> "LiveSession":
    """``VAURAModel.open_live``: the checks, then the session.  The sampling keywords take scalars or one value per clip, as
    ``generate_long_stream`` does.  Refused here: ``num_candidates`` > 1, any ``prompt_lengths`` / ``audio_lengths`` / ``max_new_tokens``
    / ``video_lengths``, a sampler with ``near_tie="rerun"``, a stride that is not one segment (``live_plan``), and a model without
    the flattened AVCLIP layout (only there is a video token part of one segment)."""
    clip_params.refuse_attention("a live session", return_attention_weights)
    check_open(batch, block_frames, num_candidates=num_candidates, prompt_lengths=prompt_lengths, audio_lengths=audio_lengths,
               max_new_tokens=max_new_tokens, video_lengths=video_lengths, near_tie=getattr(model.sampler, "near_tie", None))
    clip_params.check_lengths(batch, use_sampling=use_sampling, temp=temp, top_k=top_k, top_p=top_p, cfg_scale=cfg_scale)
    if not getattr(model, "flatten_vis_feats", False):
        raise _error("a live session needs the flattened AVCLIP layout (a MotionFormer extractor with flatten_vis_feats): only there is a "
                     "video token part of one segment")
    if model_max_duration is None:   # scripts/generate.py:221-226
        model_max_duration = 2.56 if model.sampler.config.block_size > 64 else 0.64
    ecfg = model.visual_feature_extractor.cfg
    plan = live_plan(model_max_duration, stride, vfps, ecfg.frames)
    sampling = dict(use_sampling=use_sampling, temp=temp, top_k=top_k, top_p=top_p, cfg_scale=cfg_scale)
    return LiveSession(model, int(batch), int(block_frames), plan, sampling, bool(return_relevance), clip_indices)


class LiveSession:
    """See the module docstring.  The state a session holds does not grow with the segments pushed: the last W segments' features,
    the prompt tokens of the next chunk (chunk 0's frames while it runs), and the ``_Held`` frames behind the last emitted one."""

    def __init__(self, model, batch, block_frames, plan, sampling, return_relevance, clip_indices):
        self.model, self.batch, self.block_frames, self.plan = model, batch, block_frames, plan
        self.sampling, self.return_relevance, self.clip_indices = sampling, return_relevance, clip_indices
        ecfg = model.visual_feature_extractor.cfg
        self.seg_tokens, self.segment_frames, self.cond_in = ecfg.t, ecfg.frames, ecfg.embed_dim
        # chunk 0 as generate_stream would resolve it: the host stage, then the engine's call record — before the engine is touched
        self._call = model._resolve_call(torch.empty(batch, 0), None, plan["first"], prompt_is_encoded=True, return_logprobs=False,
                                         return_relevance=return_relevance, video_lengths=None, prompt_lengths=None, audio_lengths=None,
                                         **sampling)
        kw = model._codes_keywords(self._call, batch, 0, None, None, None)
        self._noise_host = kw.pop("noise")
        kw.pop("prompt")
        self._codes_call = clip_params.resolve_codes_call(batch, plan["window"] * self.seg_tokens, plan["first"], None, **kw)
        self.book = LiveBook(plan, self._call.delays, block_frames, self._codes_call.tokens_per_frame, self.seg_tokens, _decode_halo(model))
        self._held = _Held(model, return_relevance)
        self._feats: List[torch.Tensor] = []       # extractor output of the last W segments, (B, t, cond_in) each
        self._chunk: List[torch.Tensor] = []       # chunk 0's frames as they become final
        self._prompt = None                        # the next chunk's prompt tokens (B, K, plan["prompt"])
        self._eng = None                           # the engine chunk 0 runs on (the sampler's; its fallback after a dirty status)
        self._steps = 0                            # sampled steps of chunk 0 that have run clean
        self._slot = 0
        self._dead = False
        self.closed = False

    # ------------------------------------------------------------------ public
    @property
    def frames_emitted(self) -> int:
        return self._held.emitted

    @torch.no_grad()
    def push(self, features=None, frames=None) -> List[dict]:
        kind = check_push(features, frames, self.batch, self.seg_tokens, self.cond_in, self.segment_frames, self.closed)
        if self._dead:
            raise _error("this session has raised after audio had left it: open a new one")
        model = self.model
        if kind == "frames":
            raw, _ = model.visual_feature_extractor(frames)
        else:
            raw = features.reshape(self.batch, 1, self.seg_tokens, self.cond_in)
        raw = raw.to(model.device).reshape(self.batch, self.seg_tokens, self.cond_in)
        self._feats = (self._feats + [raw])[-self.plan["window"]:]
        work, releases = self.book.push()
        if work[0] == "steps":
            blocks = self._run_steps(self._bridged(raw), work[1])
        else:
            blocks = self._run_chunk(work[2])
        assert [(b["start_frame"], b["start_frame"] + b["frames"]) for b in blocks] == releases, (blocks, releases)
        return blocks

    @torch.no_grad()
    def close(self) -> List[dict]:
        if self.closed:
            raise _error("close() after close(): the session has handed out its last block")
        self.closed = True
        last = self.book.close()
        if last is None or self._dead:
            return []
        return [self._held.release(last[1], True)]

    # ------------------------------------------------------------------ chunk 0: incrementally, on the video received so far
    def _begin(self, eng):
        """chunk 0 begun on ``eng``: the pattern sequence without a prompt and the NaN-filled condition buffer"""
        self._eng = eng
        with off_null_stream(eng.dev):
            self._start, self._sp, self._noise = eng.begin_live(self._codes_call, self._noise_host, owner=self)
        assert self._start == self.book.first_step
        self._begun = False                        # the teacher-forced positions in front of the first sampled step have not run

    def _bridged(self, raw):
        """one segment of extractor output (B, t, cond_in) as the sampler's condition takes it: the visual bridge, segment by segment"""
        return self.model.visual_bridge(raw.detach()).float()

    def _append(self, cond, index):
        with off_null_stream(self._eng.dev):
            self._eng.append_condition(cond, index * self.seg_tokens)

    def _run_steps(self, cond, pieces) -> List[dict]:
        if self._eng is None:
            self._begin(self.model.sampler.engine())
        if self._eng.live_owner is not self:       # chunk 0 lives in the engine's buffers between the pushes
            self._dead = True
            raise _error("another call has used the sampler's engine since this session's last push: until its first chunk is complete "
                         "(four segments) a session owns the engine — open a new session")
        self._append(cond, self.book.segments - 1)
        eng, events, blocks = self._eng, [], []
        use_graph = self._codes_call.use_graph

        def enqueue(k):                            # piece k, its state words behind it, its event behind those
            with off_null_stream(eng.dev):
                events.append((self._slot, eng.enqueue_piece(self._slot, 0 if self._begun else self._start - 1, pieces[k][0], self._sp,
                                                             self._noise, use_graph)))
            self._begun, self._slot = True, self._slot ^ 1
        if pieces:
            enqueue(0)
        for k, (n, lo, hi) in enumerate(pieces):
            if k + 1 < len(pieces):                # at most two pieces in flight, as in DecoderEngine._codes_stream
                enqueue(k + 1)
            slot, ev = events[k]
            ev.synchronize()
            st = eng._stream_status(eng._pinned_words()[slot])
            if st:
                err = eng.stream_error(st, events[-1][1])
                if self._held.emitted:
                    self._dead = True
                    err.frames_emitted = [self._held.emitted] * self.batch
                    err.args = (f"{err.args[0]} — after frames {err.frames_emitted} of the clips had been streamed out: they cannot be taken back",)
                    raise err
                # before any frame has left: what has run so far runs again on the engine generate() would fall back to, then on
                return blocks + self._restart(eng._status_fallback(st, err), pieces[k:])
            self._steps += n
            if hi > lo:
                self._final_frames(lo, hi, blocks)
        return blocks

    def _final_frames(self, lo, hi, blocks):
        """the frames [lo, hi) of chunk 0 have become final: into the held frames, and a block out when one is due"""
        blk = self.model._stream_block(self._eng, [(lo, hi)] * self.batch, self._call)
        self._chunk.append(blk["sampled_indices"])
        self._held.add(blk["sampled_indices"], {k: blk[k] for k in (REL if self.return_relevance else ())})
        upto = hi - self.book.halo
        if upto > self._held.emitted:
            blocks.append(self._held.release(upto, False))
        if hi == self.plan["first"]:               # chunk 0 is complete: the next chunk is prompted with its tail
            self._prompt = torch.cat(self._chunk, dim=-1)[:, :, self.plan["stride_tokens"]:]
            self._chunk = []

    def _restart(self, eng, rest) -> List[dict]:
        """A dirty status before the first block: chunk 0 again on ``eng`` (this engine on the separate launches, or the exact-fp32
        twin) — the received segments, the steps that had run as one piece, then the pieces that are left."""
        done, self._steps = self._steps, 0
        self._held, self._chunk = _Held(self.model, self.return_relevance), []
        self._begin(eng)
        for i, raw in enumerate(self._feats[:-1]):
            self._append(self._bridged(raw), i)
        cond = self._bridged(self._feats[-1])
        catch_up = [(done, 0, eng.final_frames(done, self._start))] if done else []
        return self._run_steps(cond, catch_up + list(rest))

    # ------------------------------------------------------------------ chunk c >= 1: the long-form stream's call
    def _run_chunk(self, ch) -> List[dict]:
        if self._prompt is None:
            raise _error("chunk 0 of this session did not complete")
        W = self.plan["window"]
        window = torch.stack(self._feats[-W:], dim=1)          # (B, W, t, cond_in): extractor output, passed through unchanged
        skw = dict(self.sampling, clip_indices=self.clip_indices, prompt_is_encoded=True)
        blocks = []
        try:
            it = _stream_chunk(self.model, self._held, window, self._prompt, ch["max_gen_len"], ch["offset"], False, self.block_frames,
                               self.return_relevance, skw)
            while True:
                try:
                    blocks.append(next(it))
                except StopIteration as stop:
                    self._prompt = stop.value[:, :, self.plan["stride_tokens"]:]
                    break
        except VauraHipError as e:
            if getattr(e, "status", None) is not None:       # a dirty status word: the session's frames, not the chunk's own
                self._dead = True
                e.frames_emitted = [self._held.emitted] * self.batch
            raise
        return blocks
