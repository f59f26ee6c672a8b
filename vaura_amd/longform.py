"""The caller on the input side of the hot path: single-chunk / sliding-window generation
as driven by the reference's script (/root/reference/scripts/generate.py:236-370).

Durations beyond what one pass covers (2.56 s for the released configuration, :222-224) are generated in chunks:
every later chunk is prompted with the tail of the previous one (``max_gen_len - stride_tokens`` tokens) and
produces ``stride_tokens`` new ones; the video segments of a chunk are ``positions % n_segments`` (:336-341).  The
prompt of a chunk is teacher-forced by the batched prefill pass of the engine (32 positions per weight stream),
the rest by the captured decode-step graph; the waveform of the whole clip is decoded once at the end (:366-369).

``generate_long`` keeps one duration per call.  ``generate_long_clips`` takes one duration per clip: clip b follows its own
``chunk_schedule``, and the schedules are merged into ONE ``generate_tokens`` call per chunk index (``clip_chunk_plan``) over the
per-clip lengths that call already serves; a clip whose schedule has ended stays in the batch, parked, until the longest is done.

``generate_long_stream`` / ``generate_long_clips_stream`` run the same loops as generators and hand out audio while the window slides:
after chunk c the tokens of the frames [0, N_c) are final, and the samples of a frame depend on ``codec_clips.decode_halo`` frames
either side, so [emitted, N_c - halo) is decoded then — one ``decode_window`` codec pass over that block and its halo — and the rest
on the last chunk.  The blocks are bit for bit the slices of the one decode at the end.
"""
from __future__ import annotations

from math import ceil
from typing import List, Optional

import torch

from . import clip_params

COMPRESSION_MODEL_FRAME_RATE = 86   # scripts/generate.py:30


def chunk_schedule(duration: float, model_max_duration: float = 2.56, stride: float = 0.64, vfps: float = 25) -> List[dict]:
    """The (offset, length, video positions, prompt length) of every model.generate() call the reference's loop makes
    (scripts/generate.py:236-237, 304-365) — pure bookkeeping, no tensors."""
    total_gen_len = int(duration * COMPRESSION_MODEL_FRAME_RATE)
    stride_tokens = int(COMPRESSION_MODEL_FRAME_RATE * stride)
    if duration <= model_max_duration:
        return [dict(offset=0, max_gen_len=total_gen_len, prompt_len=0, positions=None, new_tokens=total_gen_len)]
    assert stride is not None, "Stride should be defined to generate beyond max_duration"
    assert stride < model_max_duration, "Cannot stride by more than max generation duration."
    out, current_gen_offset, prompt_length = [], 0, 0
    while current_gen_offset + prompt_length < total_gen_len:
        time_offset = current_gen_offset / COMPRESSION_MODEL_FRAME_RATE
        chunk_duration = min(duration - time_offset, model_max_duration)
        max_gen_len = ceil(chunk_duration * COMPRESSION_MODEL_FRAME_RATE)
        initial_position = ceil(time_offset * vfps)
        video_target_length = ceil(chunk_duration * vfps)
        out.append(dict(offset=current_gen_offset, max_gen_len=max_gen_len, prompt_len=prompt_length,
                        positions=(initial_position // 16, (initial_position + video_target_length) // 16),
                        new_tokens=max_gen_len - prompt_length))
        prompt_length = max_gen_len - stride_tokens
        current_gen_offset += stride_tokens
    return out


REL = ("relevance", "logprob_cond", "logprob_null")


def _long_setup(model, frames, duration, stride, model_max_duration, vfps, clip_indices, use_sampling, temp, top_k, top_p, cfg_scale,
                video_lengths, who):
    """The checks of ``generate_long`` and what its loop needs: (schedule, keywords of every generate call)."""
    from .clip_params import check_lengths, refuse_lengths
    refuse_lengths(who, duration, video_lengths)
    check_lengths(frames.shape[0], use_sampling=use_sampling, temp=temp, top_k=top_k, top_p=top_p, cfg_scale=cfg_scale)
    if model_max_duration is None:   # scripts/generate.py:221-226
        model_max_duration = 2.56 if model.sampler.config.block_size > 64 else 0.64
    sched = chunk_schedule(duration, model_max_duration, stride, vfps)
    kw = dict(clip_indices=clip_indices, return_sampled_indices=True, use_sampling=use_sampling, temp=temp, top_k=top_k,
              top_p=top_p, remove_prompts=False, prompt_is_encoded=True, cfg_scale=cfg_scale)
    return sched, kw


def _long_chunks(model, frames, sched, stride_tokens, frame_step, kw, return_relevance):
    """The chunked generation of ``generate_long`` (:327-365), one ``generate_tokens`` call per step of the iteration: yields
    (chunk, the frames it generated (B, K, new_tokens), their relevance values or {})."""
    prompt_tokens = None
    for ch in sched:
        lo, hi = ch["positions"]
        positions = torch.arange(lo, hi, device=frames.device)
        selected = frames[:, positions % frames.shape[1], ...]
        if frame_step != 1:
            selected = selected[:, :, :, ::frame_step, ...]
        # tokens only: the reference decodes every chunk inside generate() and throws the audio away (:344-357)
        gen_tokens = model.generate_tokens(frames=selected, audio=prompt_tokens, max_new_tokens=ch["max_gen_len"],
                                           **(dict(kw, return_relevance=True) if return_relevance else kw))
        new_rel = {}
        if return_relevance:
            rel, gen_tokens = gen_tokens, gen_tokens["tokens"]
            new_rel = {k: rel[k] if prompt_tokens is None else rel[k][:, :, prompt_tokens.shape[-1]:] for k in REL}
        new = gen_tokens if prompt_tokens is None else gen_tokens[:, :, prompt_tokens.shape[-1]:]
        prompt_tokens = gen_tokens[:, :, stride_tokens:]
        yield ch, new, new_rel


def _check_codec_window(codec_window):
    if codec_window is not None and (isinstance(codec_window, bool) or not isinstance(codec_window, int) or codec_window < 1):
        raise _error(f"codec_window must be None or a positive number of frames, got {codec_window!r}")


def _check_emit_chunks(emit_chunks):
    if isinstance(emit_chunks, bool) or not isinstance(emit_chunks, int) or emit_chunks < 1:
        raise _error(f"emit_chunks must be a positive number of chunks, got {emit_chunks!r}")


@torch.no_grad()
def generate_long(model, frames: torch.Tensor, duration: float, *, stride: float = 0.64, model_max_duration: Optional[float] = None,
                  vfps: float = 25, frame_step: int = 1, clip_indices=None, use_sampling: bool = True, temp: float = 1.0,
                  top_k: int = 128, top_p: float = 0.0, cfg_scale: float = 1.0, return_relevance: bool = False, video_lengths=None,
                  codec_window: Optional[int] = None, return_attention_weights: bool = False) -> dict:
    """frames: whatever the feature-extractor plugin accepts, segments on dim 1 — raw (B, S, C, T, H, W) or, with the
    pass-through ``MotionFormer``, features (B, S, t, 768).  Returns {"generated_audio", "sampled_indices"}.
    ``use_sampling``, ``temp``, ``top_k``, ``top_p``, ``cfg_scale``: scalars, or one value per clip (length-B list / tuple / 1-D
    tensor) — every chunk of clip b is sampled with clip b's values (``VAURAModel.generate_tokens``).
    ``return_relevance``: passed to every chunk; the result gains "relevance", "logprob_cond" and "logprob_null" (B, K, T), the chunks'
    values concatenated with the prompt overlap removed the way the tokens are (every frame carries the values of the chunk that
    GENERATED it).  No sequence means are returned here: chunks overlap, and a mean per chunk is not a mean of the clip — reduce the
    (B, K, T) values as needed.
    ``codec_window``: None — the waveform is decoded in one codec pass, as always; an int — in successive windows of that many frames
    (``DacModelWrapper.decode_windowed``): the same bits, with codec workspaces that follow the window instead of the duration.
    One ``duration`` for the whole call: a per-clip sequence of durations, or ``video_lengths``, is refused (per-clip lengths are a
    feature of one ``generate()`` call; the chunk schedule here is shared by the batch)."""
    clip_params.refuse_attention("generate_long", return_attention_weights)
    _check_codec_window(codec_window)
    sched, kw = _long_setup(model, frames, duration, stride, model_max_duration, vfps, clip_indices, use_sampling, temp, top_k, top_p,
                            cfg_scale, video_lengths, "generate_long")
    if len(sched) == 1 and sched[0]["positions"] is None:     # single chunk (:309-324)
        selected = frames[:, :, ::frame_step, ...] if frame_step != 1 else frames
        item = model.generate(frames=selected, audio=None, max_new_tokens=sched[0]["max_gen_len"],
                              **(dict(kw, return_relevance=True) if return_relevance else kw))
        if codec_window is not None:
            item["generated_audio"] = model.audio_encoder.decode_windowed(item["sampled_indices"][..., : model.num_codebooks, :], codec_window)
        return {"generated_audio": item["generated_audio"], "sampled_indices": item["sampled_indices"],
                **({k: item[k] for k in REL} if return_relevance else {})}
    stride_tokens = int(COMPRESSION_MODEL_FRAME_RATE * stride)
    all_tokens = []
    all_rel = {k: [] for k in REL}
    for _, new, new_rel in _long_chunks(model, frames, sched, stride_tokens, frame_step, kw, return_relevance):   # chunked generation (:327-365)
        all_tokens.append(new)
        for k, v in new_rel.items():
            all_rel[k].append(v)
    gen_tokens = torch.cat(all_tokens, dim=-1)
    codes = gen_tokens[..., : model.num_codebooks, :]
    if codec_window is None:
        audio = model.audio_encoder.decode([(codes, None)])   # :366-369
    else:
        audio = model.audio_encoder.decode_windowed(codes, codec_window)
    return {"generated_audio": audio, "sampled_indices": gen_tokens,
            **({k: torch.cat(v, dim=-1) for k, v in all_rel.items()} if return_relevance else {})}


def _decode_halo(model) -> int:
    from .codec_clips import decode_halo
    return decode_halo(model.audio_encoder.cfg)


def generate_long_stream(model, frames: torch.Tensor, duration: float, *, emit_chunks: int = 1, stride: float = 0.64,
                         model_max_duration: Optional[float] = None, vfps: float = 25, frame_step: int = 1, clip_indices=None,
                         use_sampling: bool = True, temp: float = 1.0, top_k: int = 128, top_p: float = 0.0, cfg_scale: float = 1.0,
                         return_relevance: bool = False, video_lengths=None, block_frames: Optional[int] = None,
                         return_attention_weights: bool = False):
    """``generate_long`` as a generator of finished audio: the arguments are checked here, the returned iterator runs the chunks.
    After every ``emit_chunks`` chunks, and after the last one, it yields {"audio" (B, 1, n * hop), "start_frame", "frames" (n),
    "sampled_indices" (B, K, n), "final"} — with ``return_relevance`` also "relevance", "logprob_cond", "logprob_null" (B, K, n) — for
    the frames [start_frame, start_frame + n).  The blocks tile the clip without overlap, and their concatenation is, bit for bit,
    ``generate_long``'s "generated_audio" / "sampled_indices" / relevance values of the same call.
    After chunk c the tokens of the frames [0, N_c), N_c = offset_c + max_gen_len_c, are final: later chunks are prompted with them
    and generate behind them.  The samples of a frame depend on ``codec_clips.decode_halo`` = H frames either side, so the frames
    [emitted, N_c - H) are decoded then (``DacModelWrapper.decode_window``: one codec pass over that window and its halo), and on
    the last chunk everything up to N_c.  A single-chunk duration yields once, what ``generate_long`` returns.
    ``block_frames``: None — the generator above; an int — audio also leaves INSIDE a chunk: every chunk runs through
    ``VAURAModel.generate_stream(decode=False)`` (``DecoderEngine.generate_codes_stream``: the decode loop in pieces that end where
    ``block_frames`` more frames are final), and by the same rule on global frame indices — chunk offset + local frame; a chunk's prompt
    frames were final before it began — the frames [emitted, known - H) are decoded as soon as ``known`` frames are final, and at a
    chunk's end what the generator above releases there.  The first block of a call is then due after about ``block_frames`` + max(delay)
    decode steps and one small codec window instead of after the first whole chunk; a single-chunk duration streams as well.  The blocks
    still tile the clip and concatenate to the bits of ``generate_long``.  ``emit_chunks`` must stay 1 with it."""
    clip_params.refuse_attention("generate_long_stream", return_attention_weights)
    _check_emit_chunks(emit_chunks)
    if block_frames is not None:
        from .clip_params import check_block_frames
        check_block_frames(block_frames)
        if emit_chunks != 1:
            raise _error(f"block_frames releases audio inside every chunk: emit_chunks must stay 1, got {emit_chunks}")
    sched, kw = _long_setup(model, frames, duration, stride, model_max_duration, vfps, clip_indices, use_sampling, temp, top_k, top_p,
                            cfg_scale, video_lengths, "generate_long_stream")
    if block_frames is not None:
        return _long_stream_blocks(model, frames, sched, int(COMPRESSION_MODEL_FRAME_RATE * stride), frame_step, kw, return_relevance, block_frames)
    return _long_stream(model, frames, sched, int(COMPRESSION_MODEL_FRAME_RATE * stride), frame_step, kw, return_relevance, emit_chunks)


class _Held:
    """The frames of a long-form stream that are final and not yet dropped, [start, start + held), with their relevance values, and
    how many have been emitted: emitted - halo >= start, so the halo in front of the next block is always at hand."""

    def __init__(self, model, return_relevance):
        self.model, self.return_relevance = model, return_relevance
        self.tok, self.rel, self.start, self.emitted = [], {k: [] for k in REL}, 0, 0

    def add(self, tok, rel):
        self.tok.append(tok)
        for k, v in rel.items():
            self.rel[k].append(v)

    def release(self, upto: int, final: bool) -> dict:
        """The block of the frames [emitted, upto): ONE ``decode_window`` pass over them and their halo; one halo stays held."""
        H, K, at = _decode_halo(self.model), self.model.num_codebooks, self.start
        tok = torch.cat(self.tok, dim=-1)
        rel = {k: torch.cat(v, dim=-1) for k, v in self.rel.items()} if self.return_relevance else {}
        B, n = tok.shape[0], upto - self.emitted
        audio = self.model.audio_encoder.decode_window(tok[..., :K, :], [self.emitted - at] * B, [n] * B)
        blk = {"audio": audio, "start_frame": self.emitted, "frames": n, "sampled_indices": tok[..., self.emitted - at:upto - at],
               "final": final, **{k: v[..., self.emitted - at:upto - at] for k, v in rel.items()}}
        self.emitted = upto
        self.start = max(at, upto - H)                                      # the halo in front of the next block stays
        self.tok = [tok[..., self.start - at:]]
        self.rel = {k: [rel[k][..., self.start - at:]] if self.return_relevance else [] for k in REL}
        return blk


@torch.no_grad()
def _long_stream(model, frames, sched, stride_tokens, frame_step, kw, return_relevance, emit_chunks):
    if len(sched) == 1 and sched[0]["positions"] is None:
        selected = frames[:, :, ::frame_step, ...] if frame_step != 1 else frames
        item = model.generate(frames=selected, audio=None, max_new_tokens=sched[0]["max_gen_len"],
                              **(dict(kw, return_relevance=True) if return_relevance else kw))
        yield {"audio": item["generated_audio"], "start_frame": 0, "frames": int(item["sampled_indices"].shape[-1]),
               "sampled_indices": item["sampled_indices"], "final": True, **({k: item[k] for k in REL} if return_relevance else {})}
        return
    H, held = _decode_halo(model), _Held(model, return_relevance)            # generated and not yet emitted: frames [held.start, N_c)
    for c, (ch, new, new_rel) in enumerate(_long_chunks(model, frames, sched, stride_tokens, frame_step, kw, return_relevance)):
        held.add(new, new_rel)
        final = c + 1 == len(sched)
        N = ch["offset"] + ch["max_gen_len"]
        upto = N if final else N - H
        if final or not ((c + 1) % emit_chunks or upto <= held.emitted):
            yield held.release(upto, final)


@torch.no_grad()
def _long_stream_blocks(model, frames, sched, stride_tokens, frame_step, kw, return_relevance, block_frames):
    """``_long_stream`` with audio leaving inside the chunks (``generate_long_stream(block_frames=...)``)."""
    held = _Held(model, return_relevance)                                   # final and not yet dropped: frames [held.start, known)
    skw = {k: v for k, v in kw.items() if k not in ("return_sampled_indices", "remove_prompts")}      # generate_stream has neither
    prompt_tokens = None
    for c, ch in enumerate(sched):
        final = c + 1 == len(sched)
        if ch["positions"] is None:                                         # single chunk (:309-324)
            selected = frames[:, :, ::frame_step, ...] if frame_step != 1 else frames
        else:
            lo, hi = ch["positions"]
            selected = frames[:, torch.arange(lo, hi, device=frames.device) % frames.shape[1], ...]
            if frame_step != 1:
                selected = selected[:, :, :, ::frame_step, ...]
        chunk = yield from _stream_chunk(model, held, selected, prompt_tokens, ch["max_gen_len"], ch["offset"], final, block_frames,
                                         return_relevance, skw)
        prompt_tokens = chunk[:, :, stride_tokens:]


def _stream_chunk(model, held, selected, prompt_tokens, T, off, final, block_frames, return_relevance, skw):
    """One chunk of a long-form stream that releases inside its chunks (``_long_stream_blocks``; a live session's chunks c >= 1): the
    call ``generate_stream(decode=False)`` on the chunk's video ``selected`` and prompt, its generated frames added to ``held``, and
    the blocks that become due on global frames — chunk offset ``off`` + local frame — yielded.  Returns the chunk's tokens (B, K, T)."""
    H = _decode_halo(model)
    P = 0 if prompt_tokens is None else int(prompt_tokens.shape[-1])
    chunk = []
    for blk in model.generate_stream(frames=selected, audio=prompt_tokens, max_new_tokens=T, block_frames=block_frames, decode=False,
                                     return_relevance=return_relevance, **skw):
        lo, hi = blk["start_frame"], blk["start_frame"] + blk["frames"]
        chunk.append(blk["sampled_indices"])
        if hi > P:                                                      # frames this chunk GENERATED: the others are held already
            held.add(blk["sampled_indices"][..., max(lo, P) - lo:],
                     {k: blk[k][..., max(lo, P) - lo:] for k in (REL if return_relevance else ())})
        known = off + max(hi, P)
        upto = (known if final else known - H) if hi == T else known - H
        if upto > held.emitted:
            yield held.release(upto, final and hi == T)
    return torch.cat(chunk, dim=-1)


# ---- one duration per clip: the schedules of the clips merged into one call per chunk index
def _error(msg: str):
    from ._lib import VauraHipError
    return VauraHipError(msg)


def _clip_durations(durations, batch: Optional[int] = None) -> List[float]:
    """``durations`` as a list of ``batch`` finite floats > 0 that each give at least one frame; anything else is refused."""
    from .clip_params import is_per_clip
    if not is_per_clip(durations) or getattr(durations, "ndim", 1) != 1:
        raise _error(f"durations must be one duration per clip (a list, tuple or 1-D tensor), got {durations!r}")
    vals = durations.tolist() if hasattr(durations, "tolist") else list(durations)
    if batch is not None and len(vals) != batch:
        raise _error(f"durations has {len(vals)} values for a batch of {batch} clips")
    out = []
    for b, d in enumerate(vals):
        if isinstance(d, bool) or not isinstance(d, (int, float)):
            raise _error(f"the duration of clip {b} must be a number of seconds, got {d!r}")
        d = float(d)
        if d != d or d in (float("inf"), float("-inf")) or d <= 0.0:
            raise _error(f"the duration of clip {b} must be finite and positive, got {d!r}")
        if int(d * COMPRESSION_MODEL_FRAME_RATE) < 1:
            raise _error(f"the duration of clip {b} ({d!r} s) gives no frame at {COMPRESSION_MODEL_FRAME_RATE} frames per second")
        out.append(d)
    if not out:
        raise _error("durations is empty")
    return out


def _clip_segments(segments, batch: int, S: int) -> List[int]:
    """``segments`` as a list of ``batch`` ints in 1 .. S (None: every clip has all S)."""
    from .clip_params import _int_list, is_per_clip
    if segments is None:
        return [int(S)] * batch
    if not is_per_clip(segments):
        raise _error(f"segments must be one integer per clip (a list, tuple or 1-D tensor), got {segments!r}")
    vals = _int_list("segments", segments)
    if len(vals) != batch:
        raise _error(f"segments has {len(vals)} values for a batch of {batch} clips")
    if min(vals) < 1 or max(vals) > S:
        raise _error(f"segments must lie in 1 .. {S} (the segments of the padded batch), got {vals}")
    return vals


def clip_chunk_plan(durations, segments=None, S: Optional[int] = None, *, model_max_duration: float = 2.56, stride: float = 0.64,
                    vfps: float = 25) -> dict:
    """The ``chunk_schedule`` of every clip, merged by chunk index — pure bookkeeping, no tensors.  ``durations``: one per clip;
    ``segments``: the leading real segments S_b of every clip (None: all ``S``); ``S``: the segments of the padded batch.
    Returns {"stride_tokens", "clips": [per clip: "duration", "segments", "schedule" (its ``chunk_schedule``), "single" (the branch
    without positions, d_b <= model_max_duration), "length" L_b = offset + max_gen_len of its last chunk], "chunks": [per chunk index
    c: "prompt_len" (common), "lo" (common; None when no clip of the chunk has positions), and per clip "T" (max_gen_len), "hi",
    "indices" (the segments of frames[b] the call reads: arange(lo, hi_b) % S_b, or range(S_b) for a single-chunk clip),
    "n_segments" and "parked", and "width": the segments the call's video tensor holds per clip — the longest selection, and at least
    the window's (a full chunk's at offset 0), so that the last chunks, where every selection is shorter, still give the call the
    video tokens of a full window (guidance needs as many as the null embedding holds)]}.  A parked clip — its schedule ended before
    chunk c — has T = prompt_len + 1, hi None and the one segment [0]: it keeps its row, and what the call gives for it is thrown away.
    The merge rests on four facts of ``chunk_schedule`` (every chunk of a clip but its last has the full length; chunk c >= 1 starts
    at c * stride_tokens, has the prompt length full - stride_tokens, and generates at least one frame); they are checked here, and
    a set of schedules that breaks one is refused rather than merged."""
    from .clip_params import _int_list
    d = _clip_durations(durations)
    B = len(d)
    if S is None:                      # the batch is as wide as its longest clip
        if segments is None:
            raise _error("clip_chunk_plan needs S, the segments of the padded batch, or per-clip segments")
        S = max(_int_list("segments", segments), default=0)
    seg = _clip_segments(segments, B, int(S))
    stride_tokens = int(COMPRESSION_MODEL_FRAME_RATE * stride)
    full = ceil(model_max_duration * COMPRESSION_MODEL_FRAME_RATE)
    window = ceil(model_max_duration * vfps) // 16      # the segments of a full chunk at offset 0
    clips = []
    for b in range(B):
        sched = chunk_schedule(d[b], model_max_duration, stride, vfps)
        last = sched[-1]
        clips.append(dict(duration=d[b], segments=seg[b], schedule=sched, single=last["positions"] is None,
                          length=last["offset"] + last["max_gen_len"]))
    chunks = []
    for c in range(max(len(cl["schedule"]) for cl in clips)):
        live = [cl["schedule"][c] for cl in clips if c < len(cl["schedule"])]
        prompt_len = live[0]["prompt_len"]
        los = {ch["positions"][0] for ch in live if ch["positions"] is not None}
        if len({ch["prompt_len"] for ch in live}) != 1 or len(los) > 1 or any(ch["offset"] != c * stride_tokens for ch in live) \
                or any(ch["new_tokens"] < 1 for ch in live):
            raise _error(f"the chunk schedules of durations {d} cannot be merged at chunk {c}: the clips disagree on the prompt length, "
                         "the offset or the first video position, or a chunk generates no frame")
        lo = los.pop() if los else None
        T, hi, indices, parked = [], [], [], []
        for cl in clips:
            n = len(cl["schedule"])
            if c >= n:
                T.append(prompt_len + 1); hi.append(None); indices.append([0]); parked.append(True)
                continue
            ch = cl["schedule"][c]
            if c < n - 1 and ch["max_gen_len"] != full:
                raise _error(f"the chunk schedules of durations {d} cannot be merged at chunk {c}: a chunk that is not a clip's last "
                             f"has {ch['max_gen_len']} frames, the window has {full}")
            T.append(ch["max_gen_len"]); parked.append(False)
            if ch["positions"] is None:
                hi.append(None); indices.append(list(range(cl["segments"])))
            else:
                hi.append(ch["positions"][1])
                indices.append([p % cl["segments"] for p in range(ch["positions"][0], ch["positions"][1])])
                if not indices[-1]:
                    raise _error(f"chunk {c} of the clip of {cl['duration']} s covers no video segment (positions {ch['positions']})")
        chunks.append(dict(index=c, prompt_len=prompt_len, lo=lo, T=T, hi=hi, indices=indices, n_segments=[len(i) for i in indices],
                           width=max(window, max(len(i) for i in indices)), parked=parked))
    return dict(stride_tokens=stride_tokens, clips=clips, chunks=chunks)


@torch.no_grad()
def generate_long_clips(model, frames: torch.Tensor, durations, *, segments=None, stride: float = 0.64,
                        model_max_duration: Optional[float] = None, vfps: float = 25, frame_step: int = 1, clip_indices=None,
                        use_sampling: bool = True, temp: float = 1.0, top_k: int = 128, top_p: float = 0.0, cfg_scale: float = 1.0,
                        return_relevance: bool = False, video_lengths=None, num_candidates=None,
                        codec_window: Optional[int] = None, return_attention_weights: bool = False) -> dict:
    """``generate_long`` for a batch whose clips differ in duration, in one call: ``durations`` holds one positive float per clip
    (list / tuple / 1-D tensor of length B), and clip b's tokens, relevance values and waveform are, bit for bit (``noise_mode=
    "philox"`` or greedy decoding), those of ``generate_long(model, frames, durations[b], ...)`` on the same batch.
    ``segments``: one int per clip, 1 <= S_b <= frames.shape[1] — the leading segments of ``frames[b]`` that are real (the batch is
    padded on dim 1; a shorter video has fewer segments).  Clip b's positions wrap at S_b, and what lies behind is never read: the
    reference for clip b is then ``generate_long(model, frames[:, :S_b], durations[b], ...)``.
    The other keywords are ``generate_long``'s.  Clip b follows ``chunk_schedule(durations[b])``; chunk index c of every clip runs in
    ONE ``model.generate_tokens`` call on the full batch (``clip_chunk_plan``): per-clip ``max_new_tokens``, the clip's own video
    selection (shorter selections padded by repeating their last segment, hidden by ``video_segments``) and the common prompt.  A
    clip whose schedule has ended stays in the batch PARKED — one new frame after the prompt, one segment, result thrown away — so
    the batch, the captured step graph, the kernel instances chosen by row count and the Philox key ``clip_base + row`` stay what
    they are in the scalar call.  A parked row still goes through the prompt prefill.
    Returns "sampled_indices" (B, K, L_max) with the special id from frame L_b on, "lengths" (B,) = L_b = the offset plus the length
    of clip b's last chunk (``ceil`` in the schedule: it can exceed int(d_b * 86) by one, as in ``generate_long``), "generated_audio"
    (B, 1, L_max * hop) — ONE ``decode_clips`` pass, zeros past a clip's end; the plain ``decode`` when every L_b is the same — and
    "audio_lengths" (B,) = L_b * hop: ``post.normalize_audio(r["generated_audio"], ..., lengths=r["audio_lengths"])`` and
    ``post.save_wavs`` take it as it is.  ``return_relevance`` adds "relevance", "logprob_cond", "logprob_null" (B, K, L_max), zero past
    L_b (no sequence means, as in ``generate_long``).  Equal durations without ``segments``: ``generate_long`` itself (what it
    refuses included) plus the two lengths.  ``codec_window``: as in ``generate_long`` — an int decodes the waveform in successive windows
    of that many frames (``decode_windowed``, the same bits), None in the one pass.
    Refused before any device work: durations that are no per-clip sequence of length B, not finite, <= 0 or without a frame;
    ``segments`` out of range; ``video_lengths`` (a chunk's video length follows from the clip's duration) and ``num_candidates``;
    and ``frame_step`` != 1 for a batch that mixes single-chunk clips (d_b <= model_max_duration) with chunked ones — the two
    branches of ``generate_long`` stride different dimensions, which one tensor cannot hold.
    With ``cfg_scale`` > 1 or ``return_relevance`` the engine needs as many video tokens in a call as the null embedding holds, so
    ``generate_long`` refuses a duration whose last chunk selects fewer segments than a full window.  Here every call is as wide as
    a full window (``clip_chunk_plan``: "width"), and such a clip is served the way ``generate_tokens(video_lengths=...)`` serves a
    clip with fewer video tokens than the batch: it has no scalar ``generate_long`` to be compared with under guidance; its scalar
    counterpart is the one-duration loop over calls of the same width."""
    clip_params.refuse_attention("generate_long_clips", return_attention_weights)
    _check_codec_window(codec_window)
    d, seg, single, kw, sample_kw = _clips_setup(model, frames, durations, segments, stride, model_max_duration, vfps, frame_step, clip_indices,
                                                 use_sampling, temp, top_k, top_p, cfg_scale, video_lengths, num_candidates, "generate_long_clips")
    B, S = int(frames.shape[0]), int(frames.shape[1])
    if segments is None and len(set(d)) == 1:          # one duration after all: the scalar call, plus the lengths
        r = generate_long(model, frames, d[0], frame_step=frame_step, return_relevance=return_relevance, codec_window=codec_window,
                          **kw, **sample_kw)
        L_b = int(r["sampled_indices"].shape[-1])
        r["lengths"] = torch.full((B,), L_b, dtype=torch.int64, device=r["sampled_indices"].device)
        r["audio_lengths"] = r["lengths"] * (int(r["generated_audio"].shape[-1]) // L_b)
        return r
    plan = clip_chunk_plan(d, seg, S, **kw)
    K = model.num_codebooks
    lengths = [cl["length"] for cl in plan["clips"]]
    L_max = max(lengths)
    st = {}
    for _ in _clips_chunks(model, frames, plan, single, frame_step, sample_kw, return_relevance, st):
        pass
    tokens, rel = st["tokens"], st["rel"]
    if codec_window is not None:
        audio = model.audio_encoder.decode_windowed(tokens[..., :K, :], codec_window, None if len(set(lengths)) == 1 else lengths)
    elif len(set(lengths)) == 1:
        audio = model.audio_encoder.decode([(tokens[..., :K, :], None)])
    else:
        audio = model.audio_encoder.decode_clips(tokens[..., :K, :], lengths)
    lens = torch.tensor(lengths, dtype=torch.int64, device=tokens.device)
    return {"generated_audio": audio, "sampled_indices": tokens, "lengths": lens,
            "audio_lengths": lens * (int(audio.shape[-1]) // L_max), **rel}


def _clips_setup(model, frames, durations, segments, stride, model_max_duration, vfps, frame_step, clip_indices, use_sampling, temp, top_k,
                 top_p, cfg_scale, video_lengths, num_candidates, who):
    """The checks of ``generate_long_clips`` -> (durations, segments, which clips are single-chunk, schedule keywords, sampling keywords)."""
    from .clip_params import check_lengths
    if video_lengths is not None:
        raise _error(f"{who} takes no video_lengths: the video length of a chunk follows from the clip's duration "
                     "(pass `segments` for videos of different lengths)")
    if num_candidates is not None:
        raise _error(f"{who} takes no num_candidates: best-of-N is a feature of one generate() call")
    if not hasattr(frames, "shape") or len(frames.shape) < 2:
        raise _error("frames must carry the clips on dim 0 and the segments on dim 1")
    B, S = int(frames.shape[0]), int(frames.shape[1])
    d = _clip_durations(durations, B)
    seg = _clip_segments(segments, B, S)
    check_lengths(B, use_sampling=use_sampling, temp=temp, top_k=top_k, top_p=top_p, cfg_scale=cfg_scale)
    if model_max_duration is None:   # scripts/generate.py:221-226
        model_max_duration = 2.56 if model.sampler.config.block_size > 64 else 0.64
    single = [x <= model_max_duration for x in d]
    if frame_step != 1 and any(single) and not all(single):
        raise _error(f"frame_step = {frame_step} with a batch that mixes single-chunk clips (durations <= {model_max_duration} s) and "
                     "chunked ones: generate_long strides another dimension in each branch, and one tensor cannot hold both — call "
                     "the two groups separately")
    kw = dict(stride=stride, model_max_duration=model_max_duration, vfps=vfps)
    sample_kw = dict(clip_indices=clip_indices, use_sampling=use_sampling, temp=temp, top_k=top_k, top_p=top_p, cfg_scale=cfg_scale)
    return d, seg, single, kw, sample_kw


def _clips_chunks(model, frames, plan, single, frame_step, sample_kw, return_relevance, st):
    """The merged chunk loop of ``generate_long_clips``, one ``generate_tokens`` call per step of the iteration.  ``st`` receives
    "tokens" (B, K, L_max; the special id where nothing is generated yet) and "rel" (the relevance values, or {}), filled chunk by
    chunk; yields (chunk index, chunk of the plan) behind each call."""
    B = int(frames.shape[0])
    dev = frames.device
    special, stride_tokens = model.special_token_id, plan["stride_tokens"]
    L_max = max(cl["length"] for cl in plan["clips"])
    tokens = None
    rel = {}
    rows = torch.arange(B, device=dev)[:, None]
    gen_kw = dict(sample_kw, return_sampled_indices=True, remove_prompts=False, prompt_is_encoded=True,
                  **(dict(return_relevance=True) if return_relevance else {}))
    prompt = None
    for c, ch in enumerate(plan["chunks"]):
        idx = torch.tensor([i + [i[-1]] * (ch["width"] - len(i)) for i in ch["indices"]], device=dev)
        selected = frames[rows, idx]                        # (B, width, ...): clip b's own segments, its last one repeated behind them
        if frame_step != 1:                                 # in the branch the clips' schedules take (:309-324 / :336-341)
            selected = selected[:, :, ::frame_step, ...] if all(single) else selected[:, :, :, ::frame_step, ...]
        out = model.generate_tokens(frames=selected, audio=prompt, max_new_tokens=ch["T"], video_segments=ch["n_segments"], **gen_kw)
        tok, P = out["tokens"], ch["prompt_len"]
        if tokens is None:
            tokens = torch.full((B, tok.shape[1], L_max), special, dtype=tok.dtype, device=tok.device)
            rel = {k: torch.zeros(B, tok.shape[1], L_max, dtype=out[k].dtype, device=tok.device) for k in REL} if return_relevance else {}
            st["tokens"], st["rel"] = tokens, rel
        for b in range(B):                                  # every frame from the chunk that GENERATED it
            if not ch["parked"][b]:
                off, T_b = c * stride_tokens, ch["T"][b]
                tokens[b, :, off + P:off + T_b] = tok[b, :, P:T_b]
                for k in rel:
                    rel[k][b, :, off + P:off + T_b] = out[k][b, :, P:T_b]
        if c + 1 < len(plan["chunks"]):
            # the next prompt: a continuing clip's tokens from stride_tokens on (its chunk was full); a clip that is — or will be — parked
            # carries the last frames it holds (zeros in front of a track shorter than the prompt): valid ids, and nothing reads the result
            P_next = plan["chunks"][c + 1]["prompt_len"]
            prompt = torch.zeros(B, tok.shape[1], P_next, dtype=tok.dtype, device=tok.device)
            for b in range(B):
                T_b = ch["T"][b]
                n = min(T_b, P_next)
                prompt[b, :, P_next - n:] = tok[b, :, T_b - n:T_b]
        yield c, ch


def generate_long_clips_stream(model, frames: torch.Tensor, durations, segments=None, *, emit_chunks: int = 1, stride: float = 0.64,
                               model_max_duration: Optional[float] = None, vfps: float = 25, frame_step: int = 1, clip_indices=None,
                               use_sampling: bool = True, temp: float = 1.0, top_k: int = 128, top_p: float = 0.0, cfg_scale: float = 1.0,
                               return_relevance: bool = False, video_lengths=None, num_candidates=None,
                               return_attention_weights: bool = False):
    """``generate_long_clips`` as a generator of finished audio (``generate_long_stream`` for one duration per clip): the arguments are
    checked here, the returned iterator runs the chunks.  After every ``emit_chunks`` chunks, and after the last one, it yields
    {"audio" (B, 1, max(frames) * hop), "start_frames" and "frames" (one int per clip), "sampled_indices" (B, K, max(frames)), "final"},
    with ``return_relevance`` the three (B, K, max(frames)) values as well: clip b's frames [start_frames[b], start_frames[b] +
    frames[b]), left-aligned, with zeros (the special id in "sampled_indices") behind them.  Per clip the blocks tile [0, L_b) without
    overlap and concatenate to the bits of ``generate_long_clips``.  Clip b's last chunk releases everything up to L_b; a clip whose
    schedule has ended has frames[b] = 0 from then on (ONE ``decode_window`` pass per block, over the clips that have something).
    Audio leaves at chunk ends only: this generator has no ``block_frames`` (``generate_long_stream`` releases inside a chunk; the
    merged per-clip schedules stay as they are)."""
    clip_params.refuse_attention("generate_long_clips_stream", return_attention_weights)
    _check_emit_chunks(emit_chunks)
    d, seg, single, kw, sample_kw = _clips_setup(model, frames, durations, segments, stride, model_max_duration, vfps, frame_step, clip_indices,
                                                 use_sampling, temp, top_k, top_p, cfg_scale, video_lengths, num_candidates,
                                                 "generate_long_clips_stream")
    if segments is None and len(set(d)) == 1:          # one duration after all: the scalar stream with per-clip bookkeeping
        inner = generate_long_stream(model, frames, d[0], emit_chunks=emit_chunks, frame_step=frame_step, return_relevance=return_relevance,
                                     **kw, **sample_kw)
        return _same_for_every_clip(inner, int(frames.shape[0]))
    plan = clip_chunk_plan(d, seg, int(frames.shape[1]), **kw)
    return _clips_stream(model, frames, plan, single, frame_step, sample_kw, return_relevance, emit_chunks)


def _same_for_every_clip(blocks, B):
    for blk in blocks:
        blk["start_frames"], blk["frames"] = [blk.pop("start_frame")] * B, [blk["frames"]] * B
        yield blk


def clip_emission(plan, c: int, halo: int, emitted: List[int]) -> List[int]:
    """Per clip, the frame up to which audio can be released after chunk ``c`` of ``clip_chunk_plan``: L_b once the clip's last chunk
    has run, else c * stride_tokens + max_gen_len - halo (never below what is out already) — pure bookkeeping."""
    out = []
    for b, cl in enumerate(plan["clips"]):
        if c + 1 >= len(cl["schedule"]):
            out.append(cl["length"])
        else:
            out.append(max(emitted[b], c * plan["stride_tokens"] + plan["chunks"][c]["T"][b] - halo))
    return out


@torch.no_grad()
def _clips_stream(model, frames, plan, single, frame_step, sample_kw, return_relevance, emit_chunks):
    H, K, B = _decode_halo(model), model.num_codebooks, int(frames.shape[0])
    emitted = [0] * B
    st = {}
    for c, ch in _clips_chunks(model, frames, plan, single, frame_step, sample_kw, return_relevance, st):
        final = c + 1 == len(plan["chunks"])
        upto = clip_emission(plan, c, H, emitted)
        counts = [u - e for u, e in zip(upto, emitted)]
        if not final and ((c + 1) % emit_chunks or max(counts) < 1):
            continue
        if max(counts) < 1:                                  # cannot happen: the last chunk generates at least one frame of the longest clip
            raise _error("the last chunk released no frame")
        tokens, rel = st["tokens"], st["rel"]
        # the frames every clip holds by now, and the stretch of the token tensor that the windows and their halos lie in
        known = [cl["length"] if c + 1 >= len(cl["schedule"]) else c * plan["stride_tokens"] + ch["T"][b] for b, cl in enumerate(plan["clips"])]
        lo = min(max(0, e - H) for e, n in zip(emitted, counts) if n)
        hi = max(k for k, n in zip(known, counts) if n)
        starts = [e - lo if n else 0 for e, n in zip(emitted, counts)]
        lens = [min(k, hi) - lo if n else 1 for k, n in zip(known, counts)]
        audio = model.audio_encoder.decode_window(tokens[..., :K, lo:hi], starts, counts, lens)
        n_max = max(counts)
        blk_tok = torch.full((B, tokens.shape[1], n_max), model.special_token_id, dtype=tokens.dtype, device=tokens.device)
        blk_rel = {k: torch.zeros(B, v.shape[1], n_max, dtype=v.dtype, device=v.device) for k, v in rel.items()}
        for b in range(B):
            blk_tok[b, :, :counts[b]] = tokens[b, :, emitted[b]:upto[b]]
            for k, v in rel.items():
                blk_rel[k][b, :, :counts[b]] = v[b, :, emitted[b]:upto[b]]
        yield {"audio": audio, "start_frames": list(emitted), "frames": counts, "sampled_indices": blk_tok, "final": final, **blk_rel}
        emitted = upto
