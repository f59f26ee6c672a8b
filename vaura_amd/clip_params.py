"""Per-clip sampling parameters of one batched generate() call — host-side bookkeeping only (no device work, no HIP library).

``use_sampling``, ``temp``, ``top_k``, ``top_p`` and ``cfg_scale`` may each be a scalar (every clip) or a length-B sequence / 1-D
tensor (clip b gets element b).  Any non-scalar argument selects the per-clip path of the sampler (csrc/step.hip
``sample_kernel<true>``, include/vaura_hip.h ``vaura_clip_sampling``); scalars next to it are broadcast.  An all-scalar call stays
the scalar call it always was.
"""
from __future__ import annotations

import functools
import inspect
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

NAMES = ("use_sampling", "temp", "top_k", "top_p", "cfg_scale")
_CAST = {"use_sampling": lambda v: int(bool(v)), "temp": float, "top_k": int, "top_p": float, "cfg_scale": float}
RECORD_BYTES = 32            # sizeof(vaura_clip_sampling)


def _error(msg: str):
    from ._lib import VauraHipError
    return VauraHipError(msg)


def is_per_clip(v) -> bool:
    """A list / tuple / array / tensor with a clip dimension; Python and 0-d scalars are not."""
    if isinstance(v, (list, tuple, range)):
        return True
    return bool(getattr(v, "ndim", 0)) and hasattr(v, "tolist")


def _scalar(v):
    return v.item() if hasattr(v, "item") and not isinstance(v, (bool, int, float)) else v


def per_clip_length(**params) -> Optional[int]:
    """The common length of the non-scalar arguments (None: all scalars); sequences of different lengths are refused."""
    n = None
    for name, v in params.items():
        if not is_per_clip(v):
            continue
        if getattr(v, "ndim", 1) != 1:
            raise _error(f"per-clip {name} must be one-dimensional (one value per clip), got shape {tuple(v.shape)}")
        if n is not None and len(v) != n[1]:
            raise _error(f"per-clip {name} has {len(v)} values but {n[0]} has {n[1]}: one value per clip")
        n = n or (name, len(v))
    return None if n is None else n[1]


def resolve(batch: int, use_sampling, temp, top_k, top_p, cfg_scale) -> Optional[Dict[str, List]]:
    """None for an all-scalar call; otherwise every parameter as a list of ``batch`` plain Python values (scalars broadcast).
    A sequence whose length is not ``batch`` raises ``VauraHipError``."""
    given = dict(zip(NAMES, (use_sampling, temp, top_k, top_p, cfg_scale)))
    if per_clip_length(**given) is None:
        return None
    out = {}
    for name, v in given.items():
        if is_per_clip(v):
            vals = v.tolist() if hasattr(v, "tolist") else list(v)
            if len(vals) != batch:
                raise _error(f"per-clip {name} has {len(vals)} values for a batch of {batch} clips")
        else:
            vals = [_scalar(v)] * batch
        out[name] = [_CAST[name](x) for x in vals]
    return out


def check_lengths(batch: Optional[int], **params) -> None:
    """Refuse per-clip sequences that disagree with each other or with ``batch`` (when it is known) — cheap, before any device work."""
    n = per_clip_length(**params)
    if n is not None and batch is not None and n != batch:
        name = next(k for k, v in params.items() if is_per_clip(v))
        raise _error(f"per-clip {name} has {n} values for a batch of {batch} clips")


def any_cfg(cfg_scale) -> bool:
    """``use_cfg`` of a call: some clip's scale is above 1 (the null-condition rows are then carried for the whole batch)."""
    if is_per_clip(cfg_scale):
        return any(float(x) > 1.0 for x in (cfg_scale.tolist() if hasattr(cfg_scale, "tolist") else cfg_scale))
    return bool(_scalar(cfg_scale) > 1.0)


def any_sampled(use_sampling, temp) -> bool:
    """Does any clip draw (use_sampling and temp > 0)?  Noise is needed then; the rows of greedy clips stay unused."""
    n = per_clip_length(use_sampling=use_sampling, temp=temp)
    if n is None:
        return bool(_scalar(use_sampling) and _scalar(temp) > 0.0)
    us = use_sampling.tolist() if hasattr(use_sampling, "tolist") else (list(use_sampling) if is_per_clip(use_sampling) else [use_sampling] * n)
    tp = temp.tolist() if hasattr(temp, "tolist") else (list(temp) if is_per_clip(temp) else [temp] * n)
    return any(bool(u) and float(t) > 0.0 for u, t in zip(us, tp))


def take(v, first: int, count: int):
    """Clips [first, first + count) of one argument: a slice of a per-clip sequence, a scalar as it is."""
    return v[first:first + count] if is_per_clip(v) else v


def repeat(v, n: int):
    """One argument of a best-of-N call: every clip's value ``n`` times in a row (candidate j of clip b is row b * n + j); a scalar as it is."""
    if not is_per_clip(v):
        return v
    vals = v.tolist() if hasattr(v, "tolist") else list(v)
    return [x for x in vals for _ in range(n)]


def pack_records(p: Dict[str, List]) -> bytes:
    """``vaura_clip_sampling`` records, one per clip, as the device buffer holds them."""
    return b"".join(struct.pack("<ififf3i", p["use_sampling"][b], p["temp"][b], p["top_k"][b], p["top_p"][b], p["cfg_scale"][b], 0, 0, 0)
                    for b in range(len(p["temp"])))


# ---- per-clip lengths of one batched call: max_new_tokens as one int per clip (T_b) and video_lengths (Tv_b, the leading video tokens
# of clip b's features that are real).  Resolved and checked here, before any device work (include/vaura_hip.h vaura_decoder_ext2).
def _int_list(name: str, v) -> List[int]:
    if getattr(v, "ndim", 1) != 1:
        raise _error(f"per-clip {name} must be one-dimensional (one value per clip), got shape {tuple(v.shape)}")
    vals = v.tolist() if hasattr(v, "tolist") else list(v)
    for x in vals:
        if isinstance(x, bool) or not isinstance(x, int):
            raise _error(f"per-clip {name} must hold integers, got {x!r}")
    return vals


def max_tokens(max_new_tokens) -> int:
    """T_max of a call: the int itself, or the largest of a per-clip sequence (integers >= 1, checked)."""
    if not is_per_clip(max_new_tokens):
        return int(_scalar(max_new_tokens))
    vals = _int_list("max_new_tokens", max_new_tokens)
    if not vals or min(vals) < 1:
        raise _error(f"per-clip max_new_tokens must be at least 1 for every clip, got {vals}")
    return max(vals)


def resolve_lengths(batch: Optional[int], max_new_tokens, video_lengths=None, n_video_tokens: Optional[int] = None, prompt_len: int = 0):
    """(T_max, [T_b] or None, [Tv_b] or None) of a call.  ``max_new_tokens``: an int (None in the second place: every clip has it) or one
    int >= 1 per clip; ``video_lengths``: None or one int per clip, 1 <= Tv_b <= ``n_video_tokens`` (where that is known).  ``batch``
    and ``n_video_tokens`` None: not known yet, checked by a later call.  A common prompt must be shorter than every clip of a per-clip sequence."""
    t_max = max_tokens(max_new_tokens)
    lens = _int_list("max_new_tokens", max_new_tokens) if is_per_clip(max_new_tokens) else None
    if lens is not None and batch is not None and len(lens) != batch:
        raise _error(f"per-clip max_new_tokens has {len(lens)} values for a batch of {batch} clips")
    if lens is not None and prompt_len >= min(lens):     # (an int max_new_tokens keeps the callers' own check)
        raise _error(f"the audio prompt ({prompt_len} frames) must be shorter than every clip's max_new_tokens ({lens})")
    tv = None
    if video_lengths is not None:
        if not is_per_clip(video_lengths):
            raise _error(f"video_lengths must be one integer per clip (a list, tuple or 1-D tensor), got {video_lengths!r}")
        tv = _int_list("video_lengths", video_lengths)
        if batch is not None and len(tv) != batch:
            raise _error(f"video_lengths has {len(tv)} values for a batch of {batch} clips")
        if lens is not None and len(tv) != len(lens):
            raise _error(f"video_lengths has {len(tv)} values but max_new_tokens has {len(lens)}: one value per clip")
        if not tv or min(tv) < 1 or (n_video_tokens is not None and max(tv) > n_video_tokens):
            raise _error(f"video_lengths must lie in 1 .. {n_video_tokens if n_video_tokens is not None else 'Tv'} (the video tokens of the "
                         f"features), got {tv}")
    return t_max, lens, tv


def resolve_segments(batch: Optional[int], video_segments, video_lengths=None, n_segments: Optional[int] = None, flattened: bool = True,
                     lens: Optional[List[int]] = None) -> List[int]:
    """``video_segments`` of a call — the leading real segments of every clip, one int per clip in 1 .. ``n_segments`` (dim 1 of the
    frames) — as a list.  It stands in for ``video_lengths`` (both at once are refused) and counts in units that only the flattened
    AVCLIP layout has."""
    if video_lengths is not None:
        raise _error("video_segments and video_lengths both say how much of a clip's video is real: pass one of them")
    if not flattened:
        raise _error("video_segments needs the flattened AVCLIP layout (a MotionFormer extractor with flatten_vis_feats): only there "
                     "is a video token part of one segment")
    if not is_per_clip(video_segments):
        raise _error(f"video_segments must be one integer per clip (a list, tuple or 1-D tensor), got {video_segments!r}")
    seg = _int_list("video_segments", video_segments)
    if batch is not None and len(seg) != batch:
        raise _error(f"video_segments has {len(seg)} values for a batch of {batch} clips")
    if lens is not None and len(seg) != len(lens):
        raise _error(f"video_segments has {len(seg)} values but max_new_tokens has {len(lens)}: one value per clip")
    if not seg or min(seg) < 1 or (n_segments is not None and max(seg) > n_segments):
        raise _error(f"video_segments must lie in 1 .. {n_segments if n_segments is not None else 'S'} (the segments of the frames), got {seg}")
    return seg


def refuse_lengths(where: str, max_new_tokens=None, video_lengths=None) -> None:
    """Callers that keep one length per call (the sliding window, teacher-forced scoring) refuse a per-clip sequence with a message."""
    if is_per_clip(max_new_tokens) or video_lengths is not None:
        raise _error(f"{where} takes one length for the whole call: per-clip lengths (a max_new_tokens / duration sequence, video_lengths) "
                     "are served by generate() / generate_tokens() only")


# ---- per-clip lengths of one teacher-forced scoring call (DecoderEngine.score_clips): Ta_b timesteps of clip b's codes and Tv_b video
# tokens.  Scoring feeds codes[..., :Ta_b - 1], so a clip needs two timesteps.
def resolve_score_lengths(batch: int, timesteps: int, lengths=None, video_lengths=None, n_video_tokens: Optional[int] = None):
    """([Ta_b] or None, [Tv_b] or None) of a scoring call over ``batch`` clips padded to ``timesteps``.  ``lengths``: None (every clip
    has ``timesteps``) or one int per clip, 2 <= Ta_b <= ``timesteps``; ``video_lengths`` as in ``resolve_lengths``."""
    lens = None
    if lengths is not None:
        if not is_per_clip(lengths):
            raise _error(f"lengths must be one integer per clip (a list, tuple or 1-D tensor), got {lengths!r}")
        lens = _int_list("lengths", lengths)
        if len(lens) != batch:
            raise _error(f"per-clip lengths has {len(lens)} values for a batch of {batch} clips")
        if min(lens) < 2 or max(lens) > timesteps:
            raise _error(f"per-clip lengths must lie in 2 .. {timesteps} (scoring needs at least 2 timesteps: the input is "
                         f"codes[..., :-1]; the codes hold {timesteps}), got {lens}")
    _, _, tv = resolve_lengths(batch, timesteps, video_lengths, n_video_tokens)
    return lens, tv


def score_list_lengths(codes, num_codebooks: int) -> List[int]:
    """The lengths of a list of per-clip code tensors (K, Ta_b) / (1, K, Ta_b), from their shapes alone; another layout is refused."""
    if not isinstance(codes, (list, tuple)) or not codes:
        raise _error("codes must be one (B, K, Ta) tensor or a non-empty list of per-clip (K, Ta_b) tensors")
    lens = []
    for b, c in enumerate(codes):
        shape = tuple(getattr(c, "shape", ()))
        if len(shape) == 3 and shape[0] == 1:
            shape = shape[1:]
        if len(shape) != 2 or shape[0] != num_codebooks:
            raise _error(f"codes of clip {b} must be ({num_codebooks}, Ta_b) or (1, {num_codebooks}, Ta_b), got {tuple(getattr(c, 'shape', ()))}")
        lens.append(int(shape[1]))
    return lens


# ---- per-clip audio prompt lengths of one batched call: prompt_lengths = [P_0 .. P_{B-1}], 0 <= P_b < T_b, on a prompt (B, K, P_max).
# Resolved and checked here, before any device work (include/vaura_hip.h vaura_decoder_ext3).
def resolve_prompt_lengths(batch: Optional[int], prompt_lengths, prompt_len: Optional[int], t_max: int, lens: Optional[List[int]] = None):
    """[P_b] of a call, or None without the keyword.  ``prompt_lengths``: one int per clip (list / tuple / 1-D integer tensor), 0 <= P_b
    <= ``prompt_len`` (P_max, the prompt tensor's last dimension; None: there is no prompt, which is refused) and P_b < T_b, T_b =
    ``lens[b]`` or ``t_max``.  ``batch`` None: not known yet, checked by a later call."""
    if prompt_lengths is None:
        return None
    if prompt_len is None:
        raise _error("prompt_lengths needs an audio prompt: it says how many frames of each clip's prompt are real")
    if not is_per_clip(prompt_lengths):
        raise _error(f"prompt_lengths must be one integer per clip (a list, tuple or 1-D tensor), got {prompt_lengths!r}")
    P = _int_list("prompt_lengths", prompt_lengths)
    if batch is not None and len(P) != batch:
        raise _error(f"prompt_lengths has {len(P)} values for a batch of {batch} clips")
    if lens is not None and len(P) != len(lens):
        raise _error(f"prompt_lengths has {len(P)} values but max_new_tokens has {len(lens)}: one value per clip")
    if not P or min(P) < 0 or max(P) > prompt_len:
        raise _error(f"prompt_lengths must lie in 0 .. {prompt_len} (the frames of the prompt tensor), got {P}")
    for b, p in enumerate(P):
        T_b = lens[b] if lens is not None else t_max
        if p >= T_b:
            raise _error(f"the audio prompt of clip {b} ({p} frames) must be shorter than its max_new_tokens ({T_b})")
    return P


def prompt_rows(clips: List[int], batch: int, cfg: bool = False, num_candidates: int = 1) -> List[int]:
    """The decoder rows of the given clips of a call over ``batch`` clips: candidate j of clip b is row b * N + j, and with the
    null-condition rows its twin is row batch * N + b * N + j."""
    N = int(num_candidates)
    rows = [b * N + j for b in clips for j in range(N)]
    return rows + [batch * N + r for r in rows] if cfg else rows


def prompt_schedule(prompt_lengths: List[int], first_delay: int, seq_len: int, cfg: bool = False, num_candidates: int = 1) -> List[tuple]:
    """The order of work of a call with per-clip prompt lengths, as a list of ("prefill", n, rows) and ("steps", count) entries.
    n_b = P_b + ``first_delay`` positions of clip b are teacher-forced; n_(1) < .. < n_(G) are the distinct values.  Sampled steps run for
    the whole batch from position n_(1) to ``seq_len`` - 2 (the last one fills slot ``seq_len`` - 1); just before the step at position
    n_(g) comes group g's prefill pass over positions [0, n_(g)), whose K / V go to ``rows`` — the rows of the group's clips, their
    null-condition rows (``cfg``) and candidates — only.  At that moment every row holds a known token at every position below n_(g);
    no earlier.  A group with n = 0 has no pass.  Equal lengths give the scalar call's plan: at most one pass over every row, then
    ``seq_len`` - 1 - n steps."""
    B = len(prompt_lengths)
    n = [int(p) + int(first_delay) for p in prompt_lengths]
    if not n or min(n) < 0 or max(n) > seq_len - 1:
        raise _error(f"teacher-forced positions {n} must lie in 0 .. {seq_len - 1}")
    plan, at = [], min(n)
    for n_g in sorted(set(n)):
        if n_g > at:
            plan.append(("steps", n_g - at))
            at = n_g
        if n_g > 0:
            plan.append(("prefill", n_g, prompt_rows([b for b in range(B) if n[b] == n_g], B, cfg, num_candidates)))
    if seq_len - 1 > at:
        plan.append(("steps", seq_len - 1 - at))
    return plan


def prompt_row_steps(prompt_lengths: List[int], first_delay: int, cfg: bool = False, num_candidates: int = 1) -> List[int]:
    """n_r of every decoder row (``vaura_decoder_ext3.row_prompt_steps``): the clip's P_b + ``first_delay``, per candidate, then once more
    for the null-condition rows."""
    n = [int(p) + int(first_delay) for p in prompt_lengths for _ in range(int(num_candidates))]
    return n + n if cfg else n


# ---- one ``DecoderEngine.generate_codes`` call with every host argument resolved: what ``generate_codes`` and ``generate_codes_stream``
# both start from, and what the engine's private methods take instead of the arguments one by one.  No tensor, no device.
@dataclass(frozen=True)
class CodesCall:
    batch: int                              # B clips of the features; the decoder runs batch * num_candidates rows (x 2 with cfg_on)
    n_video_tokens: int                     # Tv of the features
    num_candidates: int                     # N: candidate j of clip b is row b * N + j
    t_max: int                              # the call runs to the longest clip
    lengths: Optional[List[int]]            # T_b per row (None: every row has t_max)
    tv_lengths: Optional[List[int]]         # Tv_b per row (None: every row has n_video_tokens)
    P: Optional[List[int]]                  # P_b per row, at least two distinct values (None: one prompt length, ``prompt_frames``)
    prompt_frames: int                      # the call's prompt is ``prompt[..., :prompt_frames]``; 0: no prompt
    cfg_on: bool                            # the null-condition rows are carried
    use_sampling: Union[bool, List]         # the five sampling values: a scalar, or one plain value per row
    temp: Union[float, List]
    top_k: Union[int, List]
    top_p: Union[float, List]
    cfg_scale: Union[float, List]
    want_logprobs: bool
    want_relevance: bool
    tokens_per_frame: int
    delays: Optional[Sequence[int]]
    seed: int
    clip_base: int
    use_graph: bool
    want_attention: bool = False            # per-step self-attention weights of one layer (``return_attention_weights``)
    attention_layer: int = -1               # as given: negative counts from the last layer (the engine knows how many there are)
    attention_heads: str = "mean"           # "mean" | "all"


# ---- attention maps of one call (return_attention_weights): what the reporting instance of the decode-step attention serves today.
ATTENTION_MAX_LEN = 256      # attention_step256_kernel: caches of at most 256 positions
ATTENTION_HEADS = ("mean", "all")


def attention_max_len(seq_len: int, block_size: Optional[int]) -> int:
    """The cache length ``DecoderEngine.prepare`` allocates for ``seq_len`` sequence steps under the model's ``block_size``."""
    return (max(int(seq_len), int(block_size or 0)) + 31) // 32 * 32


def check_attention_keywords(attention_layer, attention_heads, n_layer: Optional[int] = None) -> int:
    """The two keywords of a call that asks for attention maps -> the layer as an index in [0, n_layer) (as given while ``n_layer`` is
    not known).  Negative layers count from the last one, as in Python; out of range is refused."""
    if attention_heads not in ATTENTION_HEADS:
        raise _error(f'attention_heads must be "mean" or "all", got {attention_heads!r}')
    if isinstance(attention_layer, bool) or not isinstance(attention_layer, int):
        raise _error(f"attention_layer must be an int, got {attention_layer!r}")
    if n_layer is None:
        return attention_layer
    if not -n_layer <= attention_layer < n_layer:
        raise _error(f"attention_layer {attention_layer} is out of range for a decoder of {n_layer} layers")
    return attention_layer % n_layer


def check_attention_shape(seq_len: int, block_size: Optional[int]) -> None:
    """Attention maps come from the single-round-trip step kernel: refused where the cache has more than 256 positions."""
    if int(block_size or 0) > ATTENTION_MAX_LEN or attention_max_len(seq_len, block_size) > ATTENTION_MAX_LEN:
        raise _error(f"return_attention_weights is served for caches of at most {ATTENTION_MAX_LEN} positions (block_size <= "
                     f"{ATTENTION_MAX_LEN}); this call has block_size {block_size} and {seq_len} sequence steps")


def refuse_attention(where: str, return_attention_weights) -> None:
    """Callers that do not serve attention maps yet refuse the flag with a message."""
    if return_attention_weights:
        raise _error(f"{where} does not return attention weights in this version: generate() / generate_tokens() serve "
                     "return_attention_weights")


@functools.lru_cache(maxsize=None)
def _codes_signature() -> inspect.Signature:
    """The signature of ``DecoderEngine.generate_codes``: its keyword defaults are written there and nowhere else."""
    from .engine import DecoderEngine
    return inspect.signature(DecoderEngine.generate_codes)


def resolve_codes_call(batch: int, n_video_tokens: int, max_new_tokens, prompt_frames: Optional[int] = None, **kw) -> CodesCall:
    """The checks and the resolution of one ``generate_codes`` call, before any device work.  ``batch``, ``n_video_tokens``: the shape
    of the features; ``prompt_frames``: the last dimension of the prompt tensor (None: no prompt); ``kw``: the keywords of
    ``generate_codes`` (its two tensors, ``prompt`` and ``noise``, are not read) — one it does not have is a TypeError, one left out
    takes the default of its signature.  Lengths that disagree with the batch, with each other or with the prompt raise ``VauraHipError``."""
    a = _codes_signature().bind(None, None, max_new_tokens, **kw)
    a.apply_defaults()
    a = a.arguments
    B, N = batch, a["num_candidates"]
    if isinstance(N, bool) or not isinstance(N, int) or N < 1:
        raise _error(f"num_candidates must be an int >= 1, got {N!r}")
    sampling = {n: a[n] for n in NAMES}
    check_lengths(B, **sampling)
    prompt_lengths = a["prompt_lengths"]
    t_max, lengths, tv_lengths = resolve_lengths(B, max_new_tokens, a["video_lengths"], n_video_tokens,
                                                 0 if (prompt_frames is None or prompt_lengths is not None) else int(prompt_frames))
    P = resolve_prompt_lengths(B, prompt_lengths, prompt_frames, t_max, lengths)
    prompt_frames = int(prompt_frames or 0)
    if P is not None and len(set(P)) == 1:      # one length after all: the scalar call with prompt[..., :P], on its path
        prompt_frames, P = P[0], None
    if N > 1:                                   # candidate j of clip b is row b * N + j: it has clip b's lengths and values
        lengths, tv_lengths, P = (repeat(v, N) if v is not None else None for v in (lengths, tv_lengths, P))
    cfg_on = any_cfg(sampling["cfg_scale"])     # some clip mixes: the whole batch carries the null-condition rows
    sampling = {n: repeat(v, N) if is_per_clip(v) else _scalar(v) for n, v in sampling.items()}
    want_relevance = bool(a["return_relevance"])
    if want_relevance and not cfg_on:
        # relevance reads the null rows: carry them, and keep every clip un-mixed through its record (the scalar cfg_scale of the
        # call's vaura_sampling then only says that the rows exist)
        cfg_on = True
        if not is_per_clip(sampling["cfg_scale"]):
            sampling["cfg_scale"] = [float(sampling["cfg_scale"])] * (B * N)
    want_attention = bool(a["return_attention_weights"])
    if want_attention:
        check_attention_keywords(a["attention_layer"], a["attention_heads"])
        if N > 1:
            raise _error(f"return_attention_weights takes num_candidates = 1 in this version (got {N}): one map per clip")
        if lengths is not None or P is not None:
            raise _error("return_attention_weights takes one length for the whole call in this version: per-clip max_new_tokens / "
                         "prompt_lengths are not served together with it")
    return CodesCall(batch=B, n_video_tokens=n_video_tokens, num_candidates=N, t_max=t_max, lengths=lengths, tv_lengths=tv_lengths, P=P,
                     prompt_frames=prompt_frames, cfg_on=cfg_on, want_logprobs=bool(a["return_logprobs"]), want_relevance=want_relevance,
                     tokens_per_frame=a["tokens_per_frame"], delays=a["delays"], seed=a["seed"], clip_base=a["clip_base"],
                     use_graph=a["use_graph"], want_attention=want_attention, attention_layer=a["attention_layer"],
                     attention_heads=a["attention_heads"], **sampling)


# ---- audio out of one generate() call while its decode loop still runs (DecoderEngine.generate_codes_stream): which frames may leave
# after how many sampled steps.  Pure bookkeeping, no tensors.
def check_block_frames(block_frames) -> int:
    if isinstance(block_frames, bool) or not isinstance(block_frames, int) or block_frames < 1:
        raise _error(f"block_frames must be a positive number of frames, got {block_frames!r}")
    return block_frames


def final_frames(j: int, T: int, start: int, d_max: int) -> int:
    """F(j): frames of a T-frame clip that are final after ``j`` sampled steps of a loop that starts sampling at step ``start``.  Frame t
    of codebook q is written at step t + 1 + d_q, and steps [start, start + j) are filled: t is final once t + 1 + max(d) < start + j."""
    return max(0, min(T, start + j - 1 - d_max))


def releasable_frames(j: int, T_b: int, T: int, start: int, d_max: int, H: int) -> int:
    """Frames of clip b (T_b of the call's T) whose SAMPLES are final after ``j`` sampled steps: a frame's samples depend on ``H`` frames
    either side, so all but the last H of the F_b = min(F(j), T_b) final frames — and all T_b once the clip is complete."""
    F_b = min(final_frames(j, T, start, d_max), T_b)
    return T_b if F_b == T_b else max(0, F_b - H)


def stream_schedule(T: int, lengths: Optional[List[int]], start: int, delays: Optional[List[int]], H: int, block_frames: int,
                    num_codebooks: Optional[int] = None) -> List[tuple]:
    """The pieces a streaming call cuts its S - ``start`` sampled steps into, S = T + max(d) + 1: a list of (n_steps, [(lo_b, hi_b) per
    clip]) — after the piece's n_steps further steps the frames [lo_b, hi_b) of clip b have become releasable (``releasable_frames``;
    lo == hi: nothing for that clip in this piece).  ``lengths``: T_b per clip (None: one clip of T frames — every clip of the batch);
    ``delays``: the codebook delays (None: 0 .. ``num_codebooks`` - 1); ``H``: the codec's halo (``codec_clips.decode_halo``).
    A piece ends at the first step count at which the call's longest clip has ``block_frames`` more releasable frames than at the
    previous boundary's target — m = k * block_frames is releasable from j = m + H + 1 + max(d) - start on —, the last one at S - start,
    where every clip is complete.  Every piece has at least one step (a long prompt makes several targets due at once: one piece),
    so the steps sum to S - start and the ranges of a clip tile [0, T_b) in order."""
    block_frames = check_block_frames(block_frames)
    if delays is None:
        if num_codebooks is None:
            raise _error("stream_schedule needs the delays or the number of codebooks")
        delays = list(range(int(num_codebooks)))
    d_max = max(int(d) for d in delays)
    lens = [int(T)] if lengths is None else [int(n) for n in lengths]
    if T < 1 or not lens or min(lens) < 1 or max(lens) > T:
        raise _error(f"stream_schedule: clip lengths {lens} must lie in 1 .. T = {T}")
    total = T + d_max + 1 - int(start)
    if start < 1 or total < 1:
        raise _error(f"stream_schedule: the first sampled step {start} must lie in 1 .. {T + d_max}")
    bounds = []
    for m in range(block_frames, T, block_frames):
        j = min(total, max(1, m + H + 1 + d_max - start))
        if j < total and (not bounds or j > bounds[-1]):
            bounds.append(j)
    bounds.append(total)
    out, prev, done = [], 0, [0] * len(lens)
    for j in bounds:
        upto = [releasable_frames(j, n, T, start, d_max, H) for n in lens]
        out.append((j - prev, [(a, z) for a, z in zip(done, upto)]))
        prev, done = j, upto
    return out


# ---- video in while audio streams out (live.LiveSession): how far the decode loop may run on the video received so far.  The decoder
# reads video only in the embed of a step (csrc/step.hip embed_kernel, launched by va_launch_embed): the step at position p takes
# condition token p // tokens_per_frame when that is < Tv, and ``empty_video_emb`` otherwise.  Pure bookkeeping, no tensors.
def video_step_bound(n_tokens: int, Tv: int, tokens_per_frame: int, start: int, seq_len: int) -> int:
    """Sampled steps of a loop that starts sampling at step ``start`` (``start`` - 1 teacher-forced positions in front of them) that may
    run once the first ``n_tokens`` of the ``Tv`` condition tokens have arrived.  Sampled step j (0-based) embeds position ``start`` - 1 +
    j, so it reads token (start - 1 + j) // tokens_per_frame: allowed while that is < n_tokens, i.e. j < n_tokens * tokens_per_frame -
    (start - 1); positions from Tv * tokens_per_frame on read no video at all, so the whole window releases all ``seq_len`` - ``start``
    steps.  0 when not even the teacher-forced positions are covered."""
    n_tokens, Tv, tpf, start, seq_len = int(n_tokens), int(Tv), int(tokens_per_frame), int(start), int(seq_len)
    if tpf < 1 or Tv < 1 or start < 1 or seq_len < start or n_tokens < 0:
        raise _error(f"video_step_bound: tokens_per_frame {tpf}, Tv {Tv}, start {start}, seq_len {seq_len}, n_tokens {n_tokens}")
    total = seq_len - start
    if n_tokens >= Tv:
        return total
    return max(0, min(total, n_tokens * tpf - (start - 1)))


def live_schedule(T: int, start: int, delays: Optional[List[int]], block_frames: int, tokens_per_frame: int, Tv: int,
                  tokens_per_push: int, num_codebooks: Optional[int] = None) -> List[List[tuple]]:
    """The pieces of a live session's first chunk: ``stream_schedule`` (halo 0: a frame is released once its TOKENS are final; the codec
    halo is kept on global frames, ``longform._Held``) cut additionally at the video bound.  Entry i holds the pieces that may run once
    push i has brought the received tokens to min(Tv, (i + 1) * ``tokens_per_push``): a list of (n_steps, (lo, hi)) — after the piece's
    n_steps further sampled steps the frames [lo, hi) are final (``final_frames``; lo == hi: none).  ceil(Tv / tokens_per_push) entries;
    every piece has at least one step, the steps of all entries sum to S - ``start`` and the ranges tile [0, T) in order."""
    block_frames = check_block_frames(block_frames)
    if delays is None:
        if num_codebooks is None:
            raise _error("live_schedule needs the delays or the number of codebooks")
        delays = list(range(int(num_codebooks)))
    if isinstance(tokens_per_push, bool) or not isinstance(tokens_per_push, int) or tokens_per_push < 1:
        raise _error(f"tokens_per_push must be a positive number of condition tokens, got {tokens_per_push!r}")
    d_max = max(int(d) for d in delays)
    S = T + d_max + 1
    ends, j = [], 0
    for n, _ in stream_schedule(T, None, start, delays, 0, block_frames, num_codebooks):
        j += n
        ends.append(j)
    out, prev, done = [], 0, 0
    for i in range(-(-int(Tv) // tokens_per_push)):
        bound = video_step_bound(min(int(Tv), (i + 1) * tokens_per_push), Tv, tokens_per_frame, start, S)
        pieces = []
        for j in sorted({e for e in ends if prev < e < bound} | ({bound} if bound > prev else set())):
            upto = final_frames(j, T, start, d_max)
            pieces.append((j - prev, (done, upto)))
            prev, done = j, upto
        out.append(pieces)
    return out
