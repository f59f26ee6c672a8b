"""Generation-path mirror of the reference's ``VAURAModel`` (/root/reference/models/vaura_model.py).

Same plugin slots and constructor keywords (:28-120), same ``generate()`` keywords and result dict
(:410-597) and same ``_sample_next_token()`` signature (:775-827), so ``scripts/generate.py``-style
callers and ``configs/generate_*.yaml`` work once the ``target:`` strings point at ``vaura_amd``.
It is a plain ``nn.Module`` (inference only — the Lightning training half is out of scope) and it
does no arithmetic itself: conditioning, the 228-step decode loop, sampling, pattern bookkeeping and
codec decode all run in libvaura_hip.so.  The teacher-forced evaluation path (``forward``, ``_compute_loss``,
``validation_step`` / ``test_step``, :136-192, 240-295, 339-347) scores given audio under given video the same way.

What differs from the reference, on purpose:
  * the hot loop uses a K/V cache and runs entirely on the device (the reference re-feeds the whole
    prefix every step, :504-506); results are identical under causal masking;
  * ``noise_mode``: "philox" (default; device RNG keyed by (seed, clip index): invariant to batch
    sharding) or "torch_cpu" (Exp(1) draws taken from torch's global CPU generator in the
    reference's own order, which reproduces the reference CPU path token for token);
  * the codec decodes in fp32 (the reference casts DAC to fp16, :92).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import _lib as L
from . import clip_params
from .engine import off_null_stream
from .patterns import DelayedPatternProvider
from .utils import instantiate_from_config, sample_from_logits


def _disabled_train(self, mode: bool = True):
    return self


def _plain(o):
    """OmegaConf / Lightning AttributeDict containers -> plain dicts and lists (hyper-parameters out of a checkpoint)."""
    if hasattr(o, "items"):
        return {str(k): _plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)) or (hasattr(o, "__iter__") and not isinstance(o, (str, bytes)) and hasattr(o, "__len__")
                                        and not torch.is_tensor(o)):
        return [_plain(v) for v in o]
    return o


@dataclass(frozen=True)
class _GenerateCall:
    """One generate() / generate_tokens() / generate_stream() call as its host stage (``VAURAModel._resolve_call``) left it."""
    N: int                                   # candidates per clip
    t_max: int                               # the call runs to the longest clip
    lengths: Optional[List[int]]             # T_b (None: every clip has t_max)
    tv_lengths: Optional[List[int]]          # video_lengths, checked as far as the host stage can
    n_segments: Optional[List[int]]          # video_segments, turned into tv_lengths once the features exist
    delays: List[int]
    sampling: dict                           # use_sampling, temp, top_k, top_p, cfg_scale: each a scalar or one value per clip
    prompt_is_encoded: bool
    prompt_lengths: Any
    audio_lengths: Any
    return_logprobs: bool
    return_relevance: bool
    by_rel: bool                             # rank_by == "relevance"
    return_all_candidates: bool
    want_lp: bool                            # what the engine is asked for: the caller's flag, or the score the candidates are ranked by
    want_rel: bool
    remove_prompts: bool
    check: bool
    want_attn: bool = False                  # return_attention_weights: the call's keyword, or the constructor flag where it is None
    attention_layer: int = -1
    attention_heads: str = "mean"

    @property
    def ragged(self) -> bool:
        """Per-clip lengths of any kind: the result is then always a dict with "lengths"."""
        return any(v is not None for v in (self.lengths, self.tv_lengths, self.n_segments, self.prompt_lengths, self.audio_lengths))


class VAURAModel(nn.Module):
    def __init__(self, learning_rate: float = 5e-6, lr_scheduler: dict = None, weight_decay: float = 0.01,
                 betas: tuple = (0.9, 0.95), batch_size: int = 1, use_visual_conditioning: bool = True,
                 feature_extractor_config: dict = None, audio_encoder_config: dict = None, sampler_config: dict = None,
                 visual_bridge_config: dict = None, pattern_provider_config: dict = None,
                 predict_at_val_start: bool = False, return_attention_weights: bool = False,
                 plot_distr_of_pred_indices: bool = False, freeze_feature_extractor: bool = False,
                 files_to_track_during_training: List[str] = None, flatten_vis_feats: bool = False,
                 apply_per_video_frame_mask: bool = False, noise_mode: str = "philox", seed: int = 0):
        super().__init__()
        self.use_visual_conditioning = use_visual_conditioning
        self.visual_feature_extractor = instantiate_from_config(feature_extractor_config) if use_visual_conditioning else None
        if freeze_feature_extractor and self.visual_feature_extractor is not None:
            self.visual_feature_extractor.eval().requires_grad_(False)
        self.using_avclip = self.visual_feature_extractor.__class__.__name__ == "MotionFormer"
        self.flatten_vis_feats = self.using_avclip and flatten_vis_feats
        sampler_config = dict(sampler_config)
        sampler_config["params"] = dict(sampler_config.get("params", {}), use_visual_conditioning=use_visual_conditioning)
        self.sampler = instantiate_from_config(sampler_config)
        self.visual_bridge = instantiate_from_config(visual_bridge_config) if use_visual_conditioning else None
        self.audio_encoder = instantiate_from_config(audio_encoder_config)
        if hasattr(self.sampler, "initialize_embeddings") and self.audio_encoder.__class__.__name__ == "DacModelWrapper":
            self.sampler.initialize_embeddings(self.audio_encoder.model)
        self.audio_encoder.eval().requires_grad_(False)
        self.num_codebooks = self.sampler.num_codebooks
        if pattern_provider_config is not None:
            cfg = dict(pattern_provider_config)
            cfg["params"] = dict(cfg.get("params", {}), n_q=self.num_codebooks)  # :699-714
            self.pattern_provider = instantiate_from_config(cfg)
        else:
            self.pattern_provider = DelayedPatternProvider(n_q=self.num_codebooks)
        if hasattr(self.sampler, "codebook_pattern"):
            self.sampler.codebook_pattern = self.pattern_provider.__class__.__name__
        self.apply_per_video_frame_mask = apply_per_video_frame_mask
        self.return_attention_weights = return_attention_weights
        self.noise_mode = noise_mode
        self.seed = seed
        self.clip_base = 0  # global index of this rank's first clip (vaura_amd.dist)
        self.eval()

    # ------------------------------------------------------------------ checkpoint ingress (scripts/generate.py:208-212)
    # reference plugin classes -> their MI355X counterparts: a hparams.yaml written by the reference's training run names the
    # reference's classes; with `remap_targets` the reference's driver needs no config edit at all
    TARGET_MAP = {
        "models.modules.sampler.llama.Transformer": "vaura_amd.sampler.Transformer",
        "models.modules.dac.model.DacModelWrapper": "vaura_amd.codec.DacModelWrapper",
        "models.modules.feature_extractors.avclip.motionformer.MotionFormer": "vaura_amd.feature_extractor.MotionFormer",
        "models.modules.misc.codebook_patterns.DelayedPatternProvider": "vaura_amd.patterns.DelayedPatternProvider",
        "models.modules.misc.codebook_patterns.ParallelPatternProvider": "vaura_amd.patterns.ParallelPatternProvider",
    }
    # tensors of a reference checkpoint that nothing on the generation path reads: the extractor's 2-D patch embedding
    # (video_model_builder.py:246-248 builds it, forward_features uses patch_embed_3d)
    UNUSED_CHECKPOINT_KEYS = ("visual_feature_extractor.patch_embed.proj.weight", "visual_feature_extractor.patch_embed.proj.bias")

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None, hparams_file=None, strict: bool = True,
                             remap_targets: bool = True, **kwargs) -> "VAURAModel":
        """``LightningModule.load_from_checkpoint`` as ``scripts/generate.py:208-212`` calls it —
        ``VAURAModel.load_from_checkpoint(ckpt, hparams_file=hparams.yaml, map_location=device)`` — without Lightning:
        constructor arguments from ``hparams_file`` (the YAML ``save_hyperparameters()`` wrote, vaura_model.py:50; plain
        ``yaml.safe_load``) or, without one, from the checkpoint's own ``hyper_parameters``; then ``state_dict`` (keys
        ``sampler.*``, ``audio_encoder.model.*``, ``visual_feature_extractor.*``) loaded strictly; then ``.to(map_location)``.
        Keyword arguments override hyper-parameters, like Lightning's.  Plugin weights that the checkpoint itself carries
        need no file of their own: a codec without ``ckpt_path`` and an extractor whose ``ckpt_path`` does not exist on this
        machine (scripts/generate.py:31-35 points it at ./segment_avclip/...) are built empty and filled from ``state_dict``
        — if the checkpoint lacks them, the strict load fails loudly."""
        import inspect
        import os
        import warnings
        import yaml
        if callable(map_location) or isinstance(map_location, dict):
            raise L.VauraHipError("load_from_checkpoint: map_location must be a device (or None): tensors are read on the CPU and the model "
                                  "is moved afterwards; a callable / dict remapping is not supported")
        # With an hparams_file only `state_dict` is needed from the checkpoint: tensors only, no pickled objects executed.  Without one
        # the constructor arguments are the checkpoint's own pickled `hyper_parameters` (Lightning's AttributeDict / OmegaConf nodes):
        # that needs the full unpickler — the caller is trusting the file exactly as Lightning's own loader would.
        try:
            blob = torch.load(os.fspath(checkpoint_path), map_location="cpu", weights_only=True)
        except Exception:
            if hparams_file is not None:
                warnings.warn(f"{checkpoint_path}: not loadable with weights_only=True (pickled objects beside the tensors); falling back to "
                              "the full unpickler — only do this with checkpoints you trust", stacklevel=2)
            blob = torch.load(os.fspath(checkpoint_path), map_location="cpu", weights_only=False)
        if "state_dict" not in blob:
            raise L.VauraHipError(f"{checkpoint_path}: not a Lightning checkpoint (no 'state_dict')")
        sd = dict(blob["state_dict"])
        if hparams_file is not None:
            if not str(hparams_file).endswith((".yaml", ".yml")):
                raise L.VauraHipError("hparams_file must be the hparams.yaml of the run (csv is not read)")
            with open(os.fspath(hparams_file)) as f:
                hp = yaml.safe_load(f) or {}
        else:
            hp = blob.get("hyper_parameters") or {}
        hp = _plain(hp)
        hp.update(kwargs)
        accepted = set(inspect.signature(cls.__init__).parameters) - {"self"}
        dropped = sorted(k for k in hp if k not in accepted)
        if dropped:      # training-side hyper-parameters (optimizer, logging, ...) have no meaning here: say which ones were ignored
            warnings.warn(f"load_from_checkpoint: hyper-parameters without a counterpart on the generation path ignored: {dropped}", stacklevel=2)
        hp = {k: v for k, v in hp.items() if k in accepted}
        for key in ("feature_extractor_config", "audio_encoder_config", "sampler_config", "pattern_provider_config"):
            c = hp.get(key)
            if remap_targets and isinstance(c, dict) and c.get("target") in cls.TARGET_MAP:
                c["target"] = cls.TARGET_MAP[c["target"]]
        ae = hp.get("audio_encoder_config")
        if isinstance(ae, dict) and ae.get("target", "").startswith("vaura_amd.") and any(k.startswith("audio_encoder.model.") for k in sd):
            p = ae.setdefault("params", {})
            if not p.get("ckpt_path") and not p.get("synthetic"):
                p["weights_from_state_dict"] = True
        fe = hp.get("feature_extractor_config")
        if isinstance(fe, dict) and fe.get("target", "").startswith("vaura_amd.") and any(k.startswith("visual_feature_extractor.") for k in sd):
            p = fe.setdefault("params", {})
            if p.get("ckpt_path") and not os.path.exists(p["ckpt_path"]):
                warnings.warn(f"feature extractor ckpt_path {p['ckpt_path']!r} does not exist here: using the extractor tensors the "
                              "checkpoint itself carries (visual_feature_extractor.*)", stacklevel=2)
                p["ckpt_path"] = None
        model = cls(**hp)
        for k in cls.UNUSED_CHECKPOINT_KEYS:
            sd.pop(k, None)
        missing, unexpected = model.load_state_dict(sd, strict=False)
        if strict and (missing or unexpected):
            raise L.VauraHipError(f"{checkpoint_path}: state_dict does not fit the plugin modules: {len(missing)} missing "
                                  f"(e.g. {list(missing)[:3]}), {len(unexpected)} unexpected (e.g. {list(unexpected)[:3]})")
        fx = model.visual_feature_extractor
        if fx is not None and hasattr(fx, "_loaded") and not any(k.startswith("visual_feature_extractor.") for k in missing):
            fx._loaded = fx._loaded or any(k.startswith("visual_feature_extractor.") for k in sd)
        model.eval()
        if map_location is not None and not callable(map_location) and not isinstance(map_location, dict):
            model = model.to(map_location)
        return model

    # ------------------------------------------------------------------ small surface
    @property
    def special_token_id(self) -> int:
        return self.sampler.d_codebook

    @property
    def device(self):
        return next(self.sampler.parameters()).device

    def _handle_visual_conditioning(self, frames: torch.Tensor, clip_indices=None, B: int = None):
        if not self.use_visual_conditioning:
            return None
        assert frames is not None
        if self.using_avclip:
            vis_feats, _ = self.visual_feature_extractor(frames)
            if self.flatten_vis_feats:
                Bf, S, Tv, D = vis_feats.shape
                vis_feats = vis_feats.reshape(Bf, S * Tv, D)
        else:
            vis_feats = self.visual_feature_extractor(frames)
        return self.visual_bridge(vis_feats.detach())

    def frames_from_video(self, video, video_transforms=None, channels_last: bool = False, input_format: str = "rgb",
                          color_matrix: str = "bt601", color_range: str = "limited", size=None, chroma_row=None, src_fps=None,
                          pts=None, time_base=None, end=None, dst_fps=25, **segment_kw) -> torch.Tensor:
        """Decoded uint8 video -> what ``generate(frames=...)`` takes: (B, S, 3, 16, 224, 224) fp32 on the sampler's device.
        ``video``: uint8 (B, T, C, H, W), (T, C, H, W) or a list of per-clip tensors (``channels_last``: (.., H, W, C)).
        ``input_format`` "nv12" / "i420": decoder surfaces instead, uint8 (B, T, R, P), (T, R, P) or a list of them, converted with
        ``color_matrix`` ("bt601" / "bt709") and ``color_range`` ("limited" / "full") in the same launch; ``size=(H, W)`` and
        ``chroma_row`` describe a padded surface (VideoPreprocessor.__call__).
        ``video_transforms``: the ``video_transforms_test`` list of configs/generate_*.yaml (Resize -> CenterCrop -> ToFloat32DType ->
        Normalize); None = its values in generate_vgg.yaml:53-65.  ``segment_kw``: segment_size_vframes / n_segments / step_size_seg
        of GenerateMultipleSegments.  The preprocessor (tap tables, device copies) is built once per distinct configuration.
        Video that is not at ``dst_fps`` = 25: ``src_fps`` (an int, a Fraction, (num, den), a float; a list: one per clip) or ``pts``
        with ``time_base`` (and ``end``), see ``VideoPreprocessor.__call__`` — the frames are selected as ffmpeg's ``fps`` filter
        selects them, in the same launch."""
        pre = self._video_preprocessor(video_transforms, channels_last, input_format, color_matrix, color_range, src_fps, dst_fps,
                                       segment_kw)
        kw = {} if input_format == "rgb" else dict(size=size, chroma_row=chroma_row)
        if pts is not None or time_base is not None or end is not None:
            kw.update(pts=pts, time_base=time_base, end=end)
        return pre(video, **kw)

    def _video_preprocessor(self, video_transforms, channels_last, input_format, color_matrix, color_range, src_fps, dst_fps, segment_kw):
        """The cached ``VideoPreprocessor`` of one configuration, on the sampler's device."""
        from .preprocess import VideoPreprocessor, as_rate
        rate = None if src_fps is None else ([as_rate(r) for r in src_fps] if isinstance(src_fps, list) else as_rate(src_fps))
        key = (repr(_plain(video_transforms)) if video_transforms is not None else None, bool(channels_last),
               tuple(sorted(segment_kw.items())), input_format, color_matrix, color_range)
        if rate is not None or as_rate(dst_fps) != 25:
            key += (repr(rate), as_rate(dst_fps))
        cache = self.__dict__.setdefault("_video_preprocessors", {})
        if key not in cache:
            kw = dict(segment_kw, channels_last=channels_last, input_format=input_format, color_matrix=color_matrix,
                      color_range=color_range, src_fps=src_fps, dst_fps=dst_fps)
            cache[key] = (VideoPreprocessor(**kw) if video_transforms is None
                          else VideoPreprocessor.from_transforms_config(_plain(video_transforms), **kw))
        pre = cache[key]
        pre.device = self.device
        return pre

    def open_video_stream(self, batch: int, *, src_fps=None, time_base=None, dst_fps=25, video_transforms=None,
                          channels_last: bool = False, input_format: str = "rgb", color_matrix: str = "bt601",
                          color_range: str = "limited", size=None, chroma_row=None, **segment_kw):
        """Decoded frames at their own rate in, 25 fps segments out (``preprocess.VideoFrameStream``): ``vs.push(frames, pts)`` takes
        any number of frames (a camera's one, a decoder's block) and returns the complete (B, 1, 3, 16, 224, 224) segments, which
        are what ``LiveSession.push(frames=)`` takes; ``vs.close()`` returns what the end of the video completes.  ``src_fps`` for a
        constant rate, ``time_base`` for frames pushed with their pts; the other keywords are ``frames_from_video``'s."""
        if (src_fps is None) == (time_base is None):
            raise L.VauraHipError("open_video_stream takes src_fps (constant rate) or time_base (frames pushed with pts)")
        pre = self._video_preprocessor(video_transforms, channels_last, input_format, color_matrix, color_range, None, dst_fps, segment_kw)
        return pre.open_stream(batch, src_fps=src_fps, time_base=time_base, size=size, chroma_row=chroma_row)

    def audio_from_pcm(self, pcm, sample_rate: int, *, lengths=None, audio_transforms=None, duration: Optional[float] = None,
                       interleaved: bool = False):
        """Decoded PCM -> what ``forward`` / ``score_relevance`` / ``test_step`` batches / ``generate(audio=...)`` take: ``(audio (B, 1,
        N) fp32 mono at the codec's rate on the sampler's device, audio_lengths)``.  ``pcm``: int16, int32 or float32, (B, C, N) or
        (C, N) (``interleaved``: (B, N, C) / (N, C)) at ``sample_rate``; ``lengths``: the real samples of each row (None: whole rows —
        ``audio_lengths`` is then None too, every clip has N samples).  ``audio_transforms``: the ``audio_transforms_test`` list of
        configs/generate_vas.yaml:43-54 (AudioStereoToMono -> AudioResample -> AudioTrim); None = resample to the codec's rate, trim
        to ``duration`` seconds when given.  The preprocessor (tap tables, device copies) is built once per distinct configuration."""
        from .audio_preprocess import AudioPreprocessor
        key = (repr(_plain(audio_transforms)) if audio_transforms is not None else None, duration)
        cache = self.__dict__.setdefault("_audio_preprocessors", {})
        if key not in cache:
            if audio_transforms is None:
                cache[key] = AudioPreprocessor(target_sr=int(getattr(self.audio_encoder, "model_sr", 44100)), duration=duration)
            else:
                cache[key] = AudioPreprocessor.from_transforms_config(_plain(audio_transforms))
                if duration is not None:                                 # the call's own duration wins over the list's AudioTrim
                    cache[key].duration = float(duration)
        pre = cache[key]
        pre.device = self.device
        audio, out_lengths = pre(pcm, sample_rate=sample_rate, lengths=lengths, interleaved=interleaved)
        return audio, (None if lengths is None else out_lengths)

    def _pattern_delays(self, timesteps: int) -> List[int]:
        """The codebook delays of ``pattern_provider.get_pattern(timesteps)`` — the only layouts the decode loop implements
        (codebook_patterns.py:374-419: DelayedPatternProvider, ParallelPatternProvider).  Anything else — a pattern object without
        ``delays``, e.g. the reference's Unrolled / VALLE / MusicLM providers — is refused rather than decoded in another layout."""
        pattern = self.pattern_provider.get_pattern(timesteps)
        delays = getattr(pattern, "delays", None)
        if delays is None:
            raise L.VauraHipError(f"pattern provider {type(self.pattern_provider).__name__}: its pattern is not a delay pattern (no `delays`); "
                                  "the decode loop implements DelayedPatternProvider / ParallelPatternProvider layouts only")
        return list(L.check_delays(delays, self.num_codebooks))

    def _exp_noise(self, steps: int, rows: int, vocab: int) -> Optional[torch.Tensor]:
        if self.noise_mode == "philox":
            return None
        if self.noise_mode != "torch_cpu":
            raise ValueError(f"unknown noise_mode {self.noise_mode!r}")
        # one (rows, vocab) exponential draw per step from the global CPU generator: the stream the
        # reference's utils.multinomial -> torch.multinomial consumes on its CPU path
        return torch.stack([torch.empty(rows, vocab).exponential_(1) for _ in range(steps)])

    # ------------------------------------------------------------------ generate
    @staticmethod
    def _check_candidates(num_candidates, return_all_candidates, use_sampling, temp, rank_by="logprob", return_relevance=False) -> int:
        """The best-of-N arguments of generate() / generate_tokens(), checked on the host alone."""
        N = num_candidates
        if rank_by not in ("logprob", "relevance"):
            raise L.VauraHipError(f'rank_by must be "logprob" or "relevance", got {rank_by!r}')
        if isinstance(N, bool) or not isinstance(N, int):
            raise L.VauraHipError(f"num_candidates must be an int, got {N!r}")
        if N < 1:
            raise L.VauraHipError(f"num_candidates must be at least 1, got {N}")
        if return_all_candidates and N == 1:
            raise L.VauraHipError("return_all_candidates needs num_candidates > 1")
        if N > 1 and not clip_params.any_sampled(use_sampling, temp):
            raise L.VauraHipError(f"num_candidates = {N} with greedy decoding for every clip: the candidates would be identical "
                                  "(use_sampling with temp > 0 for at least one clip)")
        if rank_by == "relevance" and N == 1 and not return_relevance:
            raise L.VauraHipError('rank_by="relevance" with num_candidates = 1 and no return_relevance: nothing is ranked and nothing '
                                  "is returned (pointless: it would stream the null-condition rows for no result)")
        return N

    @staticmethod
    def _check_prompt_lengths(batch, audio, prompt_is_encoded, prompt_lengths, audio_lengths, t_max, lengths) -> None:
        """The per-clip prompt keywords of generate() / generate_tokens(), checked on the host alone with what is known before any
        device work (the batch of the frames, an encoded prompt's frames)."""
        if prompt_lengths is None and audio_lengths is None:
            return
        if prompt_lengths is not None and audio_lengths is not None:
            raise L.VauraHipError("prompt_lengths (frames of an encoded prompt) and audio_lengths (samples of raw audio) both say how long "
                                  "each clip's prompt is: pass one of them")
        if audio is None:
            raise L.VauraHipError("prompt_lengths / audio_lengths needs an audio prompt: it says how much of each clip's prompt is real")
        if audio_lengths is not None and prompt_is_encoded:
            raise L.VauraHipError("audio_lengths counts the samples of raw audio; an encoded prompt takes prompt_lengths (frames)")
        if prompt_lengths is not None:   # an encoded prompt: everything is known; raw audio: its frames are checked once it is encoded
            clip_params.resolve_prompt_lengths(batch, prompt_lengths, int(audio.shape[-1]) if prompt_is_encoded else t_max, t_max, lengths)

    def _resolve_call(self, frames, audio, max_new_tokens, *, use_sampling, temp, top_k, top_p, cfg_scale, prompt_is_encoded,
                      return_logprobs, return_relevance, video_lengths, prompt_lengths, audio_lengths, num_candidates=1,
                      return_all_candidates=False, rank_by="logprob", video_segments=None, return_attention_weights=False,
                      remove_prompts=False, check=False, attention_layer=-1, attention_heads="mean") -> "_GenerateCall":
        """The host stage of generate() / generate_tokens() / generate_stream(): everything that is known before any device work —
        the batch from the frames, an encoded prompt's frames — is checked and resolved here, once per call."""
        assert not self.training, "do not use generation in training mode"
        N = self._check_candidates(num_candidates, return_all_candidates, use_sampling, temp, rank_by, return_relevance)
        batch = frames.shape[0] if hasattr(frames, "shape") else None      # frames carry the batch on dim 0
        # per-clip parameter sequences of the wrong length, and the per-clip lengths
        sampling = dict(use_sampling=use_sampling, temp=temp, top_k=top_k, top_p=top_p, cfg_scale=cfg_scale)
        clip_params.check_lengths(batch, **sampling)
        per_clip_prompt = prompt_lengths is not None or audio_lengths is not None
        t_max, lengths, tv_lengths = clip_params.resolve_lengths(
            batch, max_new_tokens, video_lengths, None,
            int(audio.shape[-1]) if (audio is not None and prompt_is_encoded and not per_clip_prompt) else 0)
        self._check_prompt_lengths(batch, audio, prompt_is_encoded, prompt_lengths, audio_lengths, t_max, lengths)
        n_segments = None if video_segments is None else clip_params.resolve_segments(
            batch, video_segments, video_lengths, frames.shape[1] if batch is not None and len(frames.shape) > 1 else None,
            self.flatten_vis_feats, lengths)
        delays = self._pattern_delays(t_max)             # the layout the loop decodes; the call runs to the longest clip
        block = self.sampler.block_size
        # attention maps (the reference declares the switch, but its llama sampler
        # returns None for the weights, llama.py:520-539, and its generate() then fails on `sa_w[-1, -1, :]`): served by the decode
        # step's reporting attention instance; what that does not serve yet is refused here, before any device work
        want_attn = bool(return_attention_weights)
        if want_attn:
            attention_layer = clip_params.check_attention_keywords(attention_layer, attention_heads, getattr(self.sampler, "n_layer", None))
            clip_params.check_attention_shape(t_max + max(delays) + 1, block)
            if N > 1:
                raise L.VauraHipError(f"return_attention_weights takes num_candidates = 1 in this version (got {N}): one map per clip")
            if lengths is not None or per_clip_prompt:
                raise L.VauraHipError("return_attention_weights takes one length for the whole call in this version: per-clip "
                                      "max_new_tokens / prompt_lengths / audio_lengths are not served together with it")
        if delays != list(range(self.num_codebooks)) and t_max + max(delays) + 1 > block:   # (the engine refuses it too, before allocating)
            raise L.VauraHipError(f"{t_max} timesteps under the delays {delays} need {t_max + max(delays) + 1} sequence "
                                  f"steps; block_size is {block}")
        by_rel = rank_by == "relevance"
        return _GenerateCall(
            N=N, t_max=t_max, lengths=lengths, tv_lengths=tv_lengths, n_segments=n_segments, delays=delays, sampling=sampling, prompt_is_encoded=prompt_is_encoded,
            prompt_lengths=prompt_lengths, audio_lengths=audio_lengths, return_logprobs=bool(return_logprobs),
            return_relevance=bool(return_relevance), by_rel=by_rel, return_all_candidates=return_all_candidates,
            # candidates are ranked by their sequence log-probability by default
            want_lp=bool(return_logprobs) or (N > 1 and not by_rel), want_rel=bool(return_relevance) or (N > 1 and by_rel),
            remove_prompts=remove_prompts, check=check, want_attn=want_attn, attention_layer=attention_layer,
            attention_heads=attention_heads)

    def _bind_call(self, call: "_GenerateCall", frames, audio, clip_indices):
        """The second stage: the prompt is encoded and the features are extracted, then the call's lengths are resolved again with the
        batch, the video tokens and the prompt known — still before the engine is touched -> (features, B, Tp, P, lengths, tv_lengths,
        the keywords of ``DecoderEngine.generate_codes``)."""
        P = call.prompt_lengths
        if audio is not None and not call.prompt_is_encoded:
            # vaura_model.py:463-469 encodes the prompt here.  (Its unpacking `cat([encoded[0] for encoded in audio])`
            # expects EnCodec's frame list and breaks on DacModelWrapper's (B, 9, T) tensor; the tensor is used as is.)
            if call.audio_lengths is not None:    # one encoder pass over the clips, each cut to its own samples: P_b = the frames it returns
                audio, P = self._encode_clips(audio, call.audio_lengths)
            else:
                audio = self.audio_encoder.encode(audio)
        vis = self._handle_visual_conditioning(frames, clip_indices)
        if vis is None:
            # the reference's llama sampler refuses a missing condition itself: `raise Exception("Not implemented")` under
            # "we should always have audio and video" (llama.py:474-476) — channel-concat conditioning has no unconditional form
            raise NotImplementedError("unconditional generation: the llama sampler always needs video features "
                                      "(the reference raises here too, llama.py:474-476)")
        B, K, T, delays, lengths, tv_lengths = vis.shape[0], self.num_codebooks, call.t_max, call.delays, call.lengths, call.tv_lengths
        Tp = 0 if audio is None else int(audio.shape[-1])
        if P is not None:                    # the loop starts sampling behind the shortest prompt
            P = clip_params.resolve_prompt_lengths(B, P, Tp, T, lengths)
            Tp = min(P)
        if call.n_segments is not None:      # segments -> video tokens, from the features' own shape
            if int(vis.shape[1]) % int(frames.shape[1]):
                raise L.VauraHipError(f"video_segments: {int(vis.shape[1])} video tokens are no multiple of the {int(frames.shape[1])} segments")
            tv_lengths = [n * (int(vis.shape[1]) // int(frames.shape[1])) for n in call.n_segments]
        if call.ragged:
            _, lengths, tv_lengths = clip_params.resolve_lengths(B, lengths if lengths is not None else T, tv_lengths, int(vis.shape[1]),
                                                                 0 if P is not None else Tp)
        return vis.float(), B, Tp, P, lengths, tv_lengths, self._codes_keywords(call, B, Tp, P, tv_lengths, audio)

    def _codes_keywords(self, call: "_GenerateCall", B: int, Tp: int, P, tv_lengths, audio) -> dict:
        """The keywords of ``DecoderEngine.generate_codes`` for a bound call: B clips, the common (or shortest) prompt length Tp, the
        per-clip prompt lengths P or None, and the encoded prompt."""
        K, T, delays = self.num_codebooks, call.t_max, call.delays
        if self.sampler.audio_tokens_per_video_frame is None:
            raise L.VauraHipError("sampler.audio_tokens_per_video_frame must be set (scripts/generate.py:216 sets 7)")
        use_cfg = clip_params.any_cfg(call.sampling["cfg_scale"]) and self.sampler.__class__.__name__ == "Transformer"   # any clip's scale > 1
        S = T + max(delays) + 1
        start = Tp + 1 + delays[0]           # Pattern.get_first_step_with_timesteps(Tp) for sorted delays
        greedy = not clip_params.any_sampled(call.sampling["use_sampling"], call.sampling["temp"])     # per-clip: noise for the batch as soon as one clip draws
        noise = None if greedy else self._exp_noise(S - start, B * call.N * K, self.sampler.d_codebook)
        per_clip = P is not None and max(P) > 0      # (equal lengths: the engine takes the common prompt ``audio[..., :P]``, on its path)
        codes_kw = dict(call.sampling, cfg_scale=call.sampling["cfg_scale"] if use_cfg else 1.0, prompt=audio if (Tp or per_clip) else None,
                        prompt_lengths=P if per_clip else None, noise=noise, seed=self.seed, clip_base=self.clip_base,
                        tokens_per_frame=self.sampler.audio_tokens_per_video_frame, delays=None if delays == list(range(K)) else delays,
                        return_logprobs=call.want_lp, return_relevance=call.want_rel, num_candidates=call.N, video_lengths=tv_lengths)
        if call.want_attn:                       # (a call without the flag passes the keywords it always passed)
            codes_kw.update(return_attention_weights=True, attention_layer=call.attention_layer, attention_heads=call.attention_heads)
        return codes_kw

    @torch.no_grad()
    def generate_tokens(self, frames=None, audio: Union[torch.Tensor, None] = None, clip_indices=None,
                        max_new_tokens: int = 512, return_attention_weights: bool = False,
                        return_sampled_indices: bool = True, check: bool = False, use_sampling: bool = True,
                        temp: float = 1.0, top_k: int = 256, top_p: float = 0.0, remove_prompts: bool = False,
                        prompt_is_encoded: bool = False, cfg_scale: float = 1.0, return_logprobs: bool = False,
                        num_candidates: int = 1, return_all_candidates: bool = False, return_relevance: bool = False,
                        rank_by: str = "logprob", video_lengths=None, video_segments=None, prompt_lengths=None, audio_lengths=None,
                        attention_layer: int = -1, attention_heads: str = "mean"):
        """generate() up to and including revert_pattern_sequence (vaura_model.py:410-572): (B, K, T') int64 tokens on
        the device, no codec decode.  The sliding-window caller (vaura_amd.longform) uses this for every chunk and
        decodes the concatenated tokens once, as the reference's script does (scripts/generate.py:366-369).
        ``use_sampling``, ``temp``, ``top_k``, ``top_p`` and ``cfg_scale`` each take a scalar or one value per clip (a length-B list /
        tuple / 1-D tensor): clip b is decoded as the scalar call with its values would decode it, in the same batch
        (``DecoderEngine.generate_codes``).
        With ``return_logprobs`` or ``num_candidates`` > 1 the result is a dict instead of the tensor: "tokens" (B, K, T') plus
          * ``return_logprobs``: "logprobs" (B, K, T') — log-probability of every generated token under the distribution its decision
            was made from (CFG-mixed logits over the temperature where the clip samples, full vocabulary: before top-k / top-p),
            0 in prompt frames —, "logprob_per_codebook" (B, K) and "sequence_logprob" (B,): its mean over the generated frames, and
            the mean of that over the codebooks (prompt frames are not counted).  ``remove_prompts`` slices "logprobs" like the tokens;
          * ``num_candidates`` = N > 1: N takes per clip in one call — the extractor and the condition MLP run on the B clips — ranked on
            the device by "sequence_logprob": "tokens" holds each clip's winner, "selected_candidate" (B,) its index,
            "candidate_scores" (B, N) every take's score, "candidate_indices" (B * N, K, T') every take's tokens (candidate j of clip
            b is row b * N + j — the rows of a call on ``frames.repeat_interleave(N, 0)``);
          * ``return_all_candidates``: nothing is selected (for a caller with its own scorer): "tokens" and the log-probabilities are
            those of all B * N takes, in candidate order;
          * ``return_relevance`` (a dict as well): the video relevance of every generated token, "relevance" (B, K, T') = "logprob_cond"
            - "logprob_null", the token's log-probability given the video minus the one given the null video, both at temperature 1
            over the full vocabulary — a property of the model's two distributions, not of the sampling settings; 0 in prompt frames,
            sliced by ``remove_prompts`` like "logprobs" —, "relevance_per_codebook" (B, K) and "sequence_relevance" (B,), its
            fixed-order means over the generated frames and then the codebooks.  It reads the null-condition rows: a call in which no
            clip's ``cfg_scale`` exceeds 1 carries them anyway (twice the rows through the decode step; the tokens are unchanged);
          * ``rank_by`` = "logprob" (default: today's ranking) | "relevance": the score the N takes are ranked by — "sequence_logprob"
            or "sequence_relevance", same tie and NaN rules (``vaura_select_candidates``); "candidate_scores" holds the score that
            ranked.  "relevance" without candidates and without ``return_relevance`` is refused.
        Per-clip lengths: ``max_new_tokens`` also takes one int per clip (a length-B list / tuple / 1-D integer tensor) T_b >= 1, and
        ``video_lengths`` one int per clip, 1 <= Tv_b <= Tv: the leading video tokens of clip b that are real (positions behind them take
        ``empty_video_emb``, as a stand-alone call given only Tv_b tokens pads them; what the features hold behind them does not matter).
        The call runs to T_max = max T_b and the result is then always a dict: "tokens" (B, K, T_max) with the special id from frame
        T_b on, "lengths" (B,) = T_b (minus the prompt with ``remove_prompts``), and the entries above, zero past a clip's end, their
        means taken over the clip's own frames.  With ``noise_mode="philox"`` or greedy decoding, clip b's frames [0, T_b) — tokens and
        every reported value — are the bits of the same call with ``max_new_tokens=T_b`` (and the features cut to Tv_b): one batched
        call serves clips of different lengths.  ``noise_mode="torch_cpu"`` works but is not comparable (its draws are consumed per step
        of the call).  A common prompt must be shorter than every T_b.
        ``video_segments``: ``video_lengths`` counted in segments of ``frames`` (dim 1) instead of video tokens — one int per clip,
        1 <= n_b <= S, the leading segments of clip b that are real.  How many tokens a segment gives is known only once the extractor
        has run, so it is turned into ``video_lengths`` = n_b * (Tv // S) from the features' own shape.  It needs the flattened AVCLIP
        layout (``flatten_vis_feats``) and excludes ``video_lengths``; a call without it takes the path it always took.
        Per-clip prompt lengths: ``prompt_lengths`` = one int per clip, 0 <= P_b < T_b, on an encoded prompt (B, K, P_max) (or on raw audio,
        counted in the frames its plain encode gives): only the first P_b frames of clip b's prompt are its prompt, what lies behind them
        is never used.  ``audio_lengths`` = one int per clip for raw ``audio`` (B, 1, N), the real samples of each row (what
        ``audio_from_pcm(..., lengths=)`` returns): the clips are encoded in one pass, each cut to its own samples, and P_b is the frames
        the encoder gives clip b.  The two exclude each other.  The result is the dict of the per-clip lengths plus "prompt_lengths"
        (B,).  With ``noise_mode="philox"`` or greedy decoding clip b's frames [0, T_b) — tokens and every reported value, means taken
        over frames [P_b, T_b) — are the bits of the same call with the common prompt ``audio[..., :P_b]``: one batched call continues
        recordings of different lengths (``DecoderEngine.generate_codes``: one decode loop plus, on the plane storages, a prefill pass
        over P_g + d_0 positions for every further distinct length).  ``noise_mode="torch_cpu"`` works but is not comparable.  With
        ``remove_prompts`` clip b's frames [P_b, T_b) are left-aligned — "tokens" (B, K, T_max - min P) with the special id behind them,
        the per-token values with zeros — and "lengths" = T_b - P_b.
        ``return_attention_weights`` (a dict as well):
        "s_attn_weights", the self-attention weights of decoder layer ``attention_layer`` (default -1: the last; negative as in Python)
        at every sampled step — fp32 (B, S - start, S - 1) on the device, S the pattern sequence length and start the first sampled
        step: ``combine_attn_weights_to_tensor``'s layout, one map per clip.  Row i is the step that samples sequence slot start + i;
        columns 0 .. start + i - 1 hold its softmax weights over the cache positions (the mean over the 16 heads in fixed order, or with
        ``attention_heads="all"`` every head: (B, 16, S - start, S - 1)), everything to the right is exactly 0.  Position p carries video
        token p // audio_tokens_per_video_frame, so the map over positions is the map over video time.  Under CFG the conditional rows
        are reported.  Tokens and every other reported value are those of the call without the flag; ``remove_prompts`` does not cut
        the map.  Served for block_size <= 256, ``num_candidates`` = 1 and one length / prompt length per call (``VauraHipError``
        otherwise, at call time)."""
        return self._generate_tokens(self._resolve_call(
            frames, audio, max_new_tokens, use_sampling=use_sampling, temp=temp, top_k=top_k, top_p=top_p, cfg_scale=cfg_scale,
            prompt_is_encoded=prompt_is_encoded, return_logprobs=return_logprobs, return_relevance=return_relevance,
            video_lengths=video_lengths, prompt_lengths=prompt_lengths, audio_lengths=audio_lengths, num_candidates=num_candidates,
            return_all_candidates=return_all_candidates, rank_by=rank_by, video_segments=video_segments,
            return_attention_weights=return_attention_weights, remove_prompts=remove_prompts, check=check,
            attention_layer=attention_layer, attention_heads=attention_heads), frames, audio, clip_indices)

    def _generate_tokens(self, call: _GenerateCall, frames, audio, clip_indices):
        """``generate_tokens`` behind its host stage."""
        N, K, T = call.N, self.num_codebooks, call.t_max
        feats, B, Tp, P, lengths, tv_lengths, codes_kw = self._bind_call(call, frames, audio, clip_indices)
        assert lengths is not None or Tp < T, "gt audio prompt can not be longer than max_new_tokens"
        eng = self.sampler.engine()
        # decode loop + its status word in one synchronisation (the reference's own post-conditions, :550-572, synchronise too); an
        # activation beyond the fp16-plane range is re-run on the exact-fp32 engine instead of raising (engine.generate_codes_checked)
        codes = eng.generate_codes_checked(feats, lengths if lengths is not None else T, **codes_kw)
        lp = None
        if call.want_lp or call.want_rel or call.want_attn:
            codes, lp = codes
        bad = (codes < 0) | (codes > self.sampler.d_codebook)
        row_len = None
        if lengths is not None:              # the special id past a clip's own end, and only there
            row_len = torch.tensor(clip_params.repeat(lengths, N), device=codes.device)
            past = torch.arange(T, device=codes.device)[None, None, :] >= row_len[:, None, None]
            bad = torch.where(past, codes != self.special_token_id, bad | (codes == self.special_token_id))
        assert not bool(bad.any()), "generated sequence is incomplete or out of range"
        if call.check:
            # vaura_model.py:508-515 checks, every step, that the prefix is coherent with the pattern mask and holds no unknown
            # token; the device loop fills the sequence in place, so the same two properties are checked on the finished one
            # (they are monotone: a violation at any step is still there at the end).  :550-558 are these asserts, always on.
            seq = eng.seq[:B * N].to(torch.int64)
            if lengths is None:
                _, mask = self.pattern_provider.get_pattern(T)._build_indexes(T, seq.device)
                mask = mask[None].expand_as(seq)
            else:                            # every clip against its OWN pattern mask: steps behind its sequence hold the special token
                mask = torch.zeros_like(seq, dtype=torch.bool)
                for T_b in sorted(set(row_len.tolist())):
                    _, m = self.pattern_provider.get_pattern(T_b)._build_indexes(T_b, seq.device)
                    mask[row_len == T_b, :, :m.shape[-1]] = m
            special = torch.full_like(seq, self.special_token_id)
            assert not bool((seq == -1).any()), "unknown tokens left in the generated sequence"
            assert bool((seq == torch.where(mask, seq, special)).all()), "sequence and pattern mask disagree"
        lo = Tp if call.remove_prompts else 0
        if not (call.want_lp or call.want_rel or call.ragged or call.want_attn):
            return codes[..., lo:T]
        out = {}
        if call.ragged:
            out["lengths"] = torch.tensor(lengths if lengths is not None else [T] * B, device=codes.device) - lo
        cut = lambda x, fill: x[..., lo:T]
        if P is not None:
            out["prompt_lengths"] = torch.tensor(P, device=codes.device)
            if call.remove_prompts:          # clip b's frames [P_b, T_b) left-aligned
                out["lengths"] = out["lengths"] + lo - out["prompt_lengths"]
                cut = self._cut_without_prompts(P, lengths if lengths is not None else [T] * B, T, codes.device)
        return self._result_dict(call, out, codes, lp, cut, eng)

    @staticmethod
    def _cut_without_prompts(P, Tb, T, dev):
        """The ``cut`` of ``generate_tokens(prompt_lengths=..., remove_prompts=True)``: every per-frame entry holds clip b's frames
        [P_b, T_b) from column 0 on — (rows, K, T - min P) — with the special id (tokens) or zeros (values) behind them."""
        B, width = len(P), T - min(P)

        def cut(x, fill):
            n = x.shape[0] // B              # candidates per clip in this tensor
            first = torch.tensor(clip_params.repeat(P, n), device=dev)[:, None, None]
            end = torch.tensor(clip_params.repeat(Tb, n), device=dev)[:, None, None]
            src = torch.arange(width, device=dev)[None, None, :] + first
            got = torch.gather(x, 2, src.clamp(max=T - 1).expand(-1, x.shape[1], -1))
            return torch.where(src < end, got, torch.full_like(got, fill))
        return cut

    def _result_dict(self, call: _GenerateCall, out, codes, lp, cut, eng) -> dict:
        """The result dict of ``generate_tokens`` from the engine's codes (B * N, K, T) and per-token values ``lp``: the candidate
        selection, then every per-frame entry through ``cut(x, fill)`` — the slice ``[..., lo:T]``, or ``_cut_without_prompts``."""
        N, K, T = call.N, self.num_codebooks, call.t_max
        B, sp = codes.shape[0] // N, self.special_token_id
        if N > 1:
            rank = lp["sequence_relevance" if call.by_rel else "score"]
            out["candidate_indices"] = cut(codes, sp)
            out["candidate_scores"] = rank.view(B, N)
            if not call.return_all_candidates:
                c32 = codes.to(torch.int32).contiguous()
                won = torch.empty(B, K, T, dtype=torch.int32, device=codes.device)
                winner = torch.empty(B, dtype=torch.int32, device=codes.device)
                L.check(eng.lib.vaura_select_candidates(L.ptr(rank), L.ptr(c32), B, N, K, T, L.ptr(won), L.ptr(winner),
                                                        L.current_stream(eng.dev)), "vaura_select_candidates")
                rows = torch.arange(B, device=codes.device) * N + winner.to(torch.int64)
                codes = won.to(torch.int64)
                lp = {k: v[rows] for k, v in lp.items()}
                out["selected_candidate"] = winner.to(torch.int64)
        out["tokens"] = cut(codes, sp)
        if call.want_attn:
            out["s_attn_weights"] = lp["attention"]
        if call.return_logprobs:
            out["logprobs"] = cut(lp["logprobs"], 0.0)
            out["logprob_per_codebook"] = lp["per_codebook"]
            out["sequence_logprob"] = lp["score"]
        if call.return_relevance:
            for k in ("relevance", "logprob_cond", "logprob_null"):
                out[k] = cut(lp[k], 0.0)
            out["relevance_per_codebook"] = lp["relevance_per_codebook"]
            out["sequence_relevance"] = lp["sequence_relevance"]
        return out

    @torch.no_grad()
    def generate(self, frames=None, audio: Union[torch.Tensor, None] = None, clip_indices=None, max_new_tokens: int = 512,
                 return_attention_weights: Optional[bool] = None, return_sampled_indices: bool = False, check: bool = False,
                 use_sampling: bool = True, temp: float = 1.0, top_k: int = 256, top_p: float = 0.0,
                 remove_prompts: bool = False, prompt_is_encoded: bool = False, cfg_scale: float = 1.0,
                 return_logprobs: bool = False, num_candidates: int = 1, return_all_candidates: bool = False,
                 return_relevance: bool = False, rank_by: str = "logprob", video_lengths=None, prompt_lengths=None,
                 audio_lengths=None, attention_layer: int = -1, attention_heads: str = "mean") -> dict:
        """``return_logprobs`` / ``num_candidates`` / ``return_all_candidates`` / ``return_relevance`` / ``rank_by``: see ``generate_tokens`` — its extra entries are added
        to the result ("sampled_indices" takes "tokens"); the codec decodes the winners (B clips), or with ``return_all_candidates``
        all B * N takes.  With the defaults the result is the dict it always was.
        ``max_new_tokens`` as one int per clip and / or ``video_lengths`` (see ``generate_tokens``): the codec decodes the padded batch in
        one pass (``decode_clips``: the clips packed into one sequence; clips that all have one length: the plain ``decode``), "generated_audio" is (B, 1, T_max * hop) with zeros past each clip's end, and the result gains
        "lengths" (B,) in frames and "audio_lengths" (B,) in samples.  With an int and no ``video_lengths`` nothing is added.
        The post stage takes that batch in one call: ``post.normalize_audio(r["generated_audio"], ..., lengths=r["audio_lengths"])``,
        or ``post.scale_batch`` / ``post.save_wavs`` for the per-clip tensors and files.
        ``prompt_lengths`` / ``audio_lengths`` (see ``generate_tokens``): per-clip prompt lengths; the result gains "prompt_lengths" (B,) next
        to "lengths" / "audio_lengths", and with ``remove_prompts`` the codec decodes each clip's own T_b - P_b generated frames.
        ``return_attention_weights`` (None: the constructor's flag, as the reference's ``_log_predict_run`` passes it) /
        ``attention_layer`` / ``attention_heads`` (see ``generate_tokens``): "s_attn_weights" holds the
        per-step self-attention map, fp32 (B, S - start, S - 1) on the device; "mha_attn_weights" stays None (channel-concat
        conditioning has no cross-attention; the reference returns None there too)."""
        K = self.num_codebooks
        if return_attention_weights is None:
            return_attention_weights = self.return_attention_weights
        call = self._resolve_call(                                   # before the engine is touched
            frames, audio, max_new_tokens, use_sampling=use_sampling, temp=temp, top_k=top_k, top_p=top_p, cfg_scale=cfg_scale,
            prompt_is_encoded=prompt_is_encoded, return_logprobs=return_logprobs, return_relevance=return_relevance,
            video_lengths=video_lengths, prompt_lengths=prompt_lengths, audio_lengths=audio_lengths, num_candidates=num_candidates,
            return_all_candidates=return_all_candidates, rank_by=rank_by, return_attention_weights=return_attention_weights,
            remove_prompts=remove_prompts, check=check, attention_layer=attention_layer, attention_heads=attention_heads)
        extra = {}
        with off_null_stream(self.sampler.engine().dev) as caller:   # decode loop + codec leave HIP's null stream together
            out_codes = self._generate_tokens(call, frames, audio, clip_indices)
            if isinstance(out_codes, dict):
                extra = out_codes
                out_codes = extra.pop("tokens")
            if "lengths" not in extra:
                generated_audio = self.audio_encoder.decode([(out_codes[..., :K, :], None)])
            else:
                # ONE codec pass over the clips packed into a single sequence: a clip's waveform is, bit for bit, what decoding its own
                # T_b frames alone gives, zeros behind it (every take of a clip has the clip's length)
                rows = out_codes.shape[0]
                row_len = extra["lengths"].repeat_interleave(rows // extra["lengths"].shape[0])
                lens = row_len.tolist()
                if len(set(lens)) == 1:
                    # every clip has the same length: the plain batched pass gives the same bits without the gaps and the pack / clear /
                    # unpack launches, which cost 2.4 % at 8 clips of 220 frames
                    generated_audio = self.audio_encoder.decode([(out_codes[..., :K, :lens[0]], None)])
                    if lens[0] < out_codes.shape[-1]:
                        generated_audio = torch.nn.functional.pad(generated_audio, (0, generated_audio.shape[-1] // lens[0] * (out_codes.shape[-1] - lens[0])))
                else:
                    generated_audio = self.audio_encoder.decode_clips(out_codes[..., :K, :], lens)
                hop = generated_audio.shape[-1] // out_codes.shape[-1]
                extra["audio_lengths"] = extra["lengths"] * hop
        if caller is not None:
            out_codes.record_stream(caller)
            generated_audio.record_stream(caller)
            for t in extra.values():
                t.record_stream(caller)
        return {"generated_audio": generated_audio, "s_attn_weights": extra.pop("s_attn_weights", None), "mha_attn_weights": None,
                "sampled_indices": out_codes if return_sampled_indices else None, **extra}

    # ------------------------------------------------------------------ generate, audio out while the decode loop still runs
    def generate_stream(self, frames=None, audio: Union[torch.Tensor, None] = None, clip_indices=None, max_new_tokens: int = 512,
                        use_sampling: bool = True, temp: float = 1.0, top_k: int = 256, top_p: float = 0.0,
                        prompt_is_encoded: bool = False, cfg_scale: float = 1.0, return_logprobs: bool = False, num_candidates: int = 1,
                        return_relevance: bool = False, video_lengths=None, prompt_lengths=None, audio_lengths=None,
                        block_frames: int = 16, decode: bool = True, return_attention_weights: bool = False):
        """``generate`` as a generator of finished audio: the arguments are checked here, the returned iterator runs the call and yields
        {"audio" (B, 1, n * hop), "start_frame", "frames" (n), "sampled_indices" (B, K, n), "final"} for the frames [start_frame,
        start_frame + n) as soon as they can no longer change — about ``block_frames`` + ``decode_halo`` + max(delay) decode steps
        into the call for the first block instead of after all of them (``DecoderEngine.generate_codes_stream``: the loop runs in
        pieces; every block is ONE codec pass over its window and halo, gathered straight from the loop's pattern sequence,
        ``decode_window_seq``).  With per-clip lengths (``max_new_tokens`` as a sequence, ``video_lengths``) the dicts carry
        "start_frames" and "frames" as lists and clip b's samples / tokens are left-aligned with zeros / the special id behind them — the
        keys of the long-form streams.  ``return_logprobs`` adds "logprobs", ``return_relevance`` "relevance", "logprob_cond" and
        "logprob_null" (B, K, n): the per-token values travel with their frames (the sequence means exist only at the end of a call:
        ``generate``).  A block in which no clip releases a frame is skipped; a clip of at most ``decode_halo`` frames appears once.
        Contract: per clip the blocks tile [0, T_b) without overlap, and concatenated they are bit for bit ``generate``'s
        "generated_audio" (over the clip's own samples), "sampled_indices" and per-token values of the same call (``noise_mode=
        "philox"`` or greedy; ``"torch_cpu"`` draws the same tensor when the generator state is the same).  Prompt frames are part of
        the stream (there is no ``remove_prompts``).
        ``decode=False``: tokens only — no "audio" entry, no codec pass, and a frame is released as soon as its TOKENS are final (no halo
        held back): for a caller that decodes on frames of its own (``longform.generate_long_stream`` on global frame indices).
        Status rule: a non-finite logit or a hand-off give-up detected BEFORE the first block re-runs the call the way ``generate``
        does (separate launches / exact-fp32 twin) and streams from there; AFTER a block has left, ``VauraHipError`` with ``.status``
        and ``.frames_emitted`` — audio that has been handed out cannot be taken back.
        Refused here, before the engine is touched: ``num_candidates`` > 1 (the winner is known only at the end), more than one distinct
        prompt length (``prompt_lengths`` / ``audio_lengths``), a sampler with ``near_tie="rerun"`` (it decides at the end), and a
        ``block_frames`` that is no positive int.  Closing the iterator early leaves at most two pieces of the loop running and the
        model usable at once."""
        clip_params.check_block_frames(block_frames)
        clip_params.refuse_attention("generate_stream", return_attention_weights)
        if isinstance(num_candidates, bool) or not isinstance(num_candidates, int) or num_candidates != 1:
            raise L.VauraHipError(f"generate_stream takes num_candidates = 1 (got {num_candidates!r}): the winning candidate is known only "
                                  "at the end of the call")
        if getattr(self.sampler, "near_tie", None) == "rerun":
            raise L.VauraHipError('generate_stream is refused with near_tie="rerun": the re-run is decided at the end of the call, after '
                                  'audio has left (use "report" or "off")')
        P = None if prompt_lengths is None else clip_params._int_list("prompt_lengths", prompt_lengths)
        if P is None and clip_params.is_per_clip(audio_lengths):     # the frames the encoder gives each clip: known from the samples alone
            from .codec_clips import clip_layout
            P = list(clip_layout(clip_params._int_list("audio_lengths", audio_lengths), self.audio_encoder.cfg, "encode").frames)
        if P is not None and len(set(P)) > 1:
            raise L.VauraHipError(f"generate_stream takes one prompt length for the call, got {P} frames per clip: distinct lengths are not "
                                  "served by this version (generate() serves them)")
        call = self._resolve_call(
            frames, audio, max_new_tokens, use_sampling=use_sampling, temp=temp, top_k=top_k, top_p=top_p, cfg_scale=cfg_scale,
            prompt_is_encoded=prompt_is_encoded, return_logprobs=return_logprobs, return_relevance=return_relevance,
            video_lengths=video_lengths, prompt_lengths=prompt_lengths, audio_lengths=audio_lengths, return_attention_weights=False)
        return self._generate_stream(call, frames, audio, clip_indices, block_frames, bool(decode))

    @torch.no_grad()
    def _generate_stream(self, call: _GenerateCall, frames, audio, clip_indices, block_frames, decode):
        feats, B, _, _, lengths, tv_lengths, codes_kw = self._bind_call(call, frames, audio, clip_indices)
        ragged = lengths is not None or tv_lengths is not None
        codec, first = self.audio_encoder, self.sampler.engine()
        blocks = first.generate_codes_stream(feats, lengths if lengths is not None else call.t_max, block_frames=block_frames,
                                             halo=_codec_halo(codec) if decode else 0, **codes_kw)
        T_b = lengths if lengths is not None else [call.t_max] * B
        for ranges in blocks:
            eng = first.stream_engine          # the engine whose sequence these ranges refer to (the exact-fp32 twin after a range fallback)
            starts, counts = [lo for lo, _ in ranges], [hi - lo for lo, hi in ranges]
            blk = self._stream_block(eng, ranges, call, lengths if decode else False)
            if ragged:
                blk.update(start_frames=starts, frames=counts)
            else:
                blk.update(start_frame=starts[0], frames=counts[0])
            blk["final"] = all(hi == n for (_, hi), n in zip(ranges, T_b))
            yield blk

    def _stream_block(self, eng, ranges, call: _GenerateCall, lengths=False) -> dict:
        """The tensors of one block of a running loop: the frames ``ranges`` = [(lo_b, hi_b) per clip] out of ``eng``'s pattern
        sequence, and the per-token values the call asked for.  ``lengths`` not False (None, or T_b per clip): "audio" as well, ONE
        codec pass over the windows gathered straight from the sequence."""
        starts, counts = [lo for lo, _ in ranges], [hi - lo for lo, hi in ranges]
        with off_null_stream(eng.dev) as caller:
            blk = {"sampled_indices": eng.stream_frames(eng.seq, ranges, self.special_token_id).to(torch.int64)}
            if lengths is not False:
                blk["audio"] = self.audio_encoder.decode_window_seq(eng.seq, starts, counts, lengths, eng.delays)
            if call.want_lp:
                blk["logprobs"] = eng.stream_frames(eng.logprobs, ranges, 0.0)
            if call.want_rel:
                blk["logprob_cond"] = eng.stream_frames(eng.logprobs_cond, ranges, 0.0)
                blk["logprob_null"] = eng.stream_frames(eng.logprobs_null, ranges, 0.0)
                blk["relevance"] = blk["logprob_cond"] - blk["logprob_null"]
        if caller is not None:
            for t in blk.values():
                t.record_stream(caller)
        return blk

    # ------------------------------------------------------------------ video in, segment by segment, while audio streams out
    def open_live(self, batch: int, block_frames: int = 16, **kw):
        """A live session (``live.LiveSession``): ``s.push(features=seg)`` / ``s.push(frames=seg)`` take the video one 16-frame segment
        at a time and return the audio blocks that became due, ``s.close()`` the rest.  The keywords are ``live.open_live``'s."""
        from .live import open_live
        return open_live(self, batch, block_frames, **kw)

    # ------------------------------------------------------------------ a picture of the audio, one column per codec frame
    @staticmethod
    def audio_to_spectrogram(audio: torch.Tensor, fmt=None, lengths=None):
        """``post.audio_to_spectrogram``: the (B, 1, N) waveform of ``generate()`` (with its "audio_lengths" when the call was ragged)
        -> (spec (B, max columns, F) fp32 on the device, columns (B,) int64 on the host); ``fmt`` None: 128 log-mel bands in dB,
        n_fft 2048, hop 512 — column t is codec frame t."""
        from . import post
        return post.audio_to_spectrogram(audio, post.SpectrogramFormat() if fmt is None else fmt, lengths=lengths)

    @staticmethod
    def loudness_stream(blocks, target=None):
        """``post.stream_loudness``: the blocks of ``generate_stream`` / ``generate_long_stream`` / a live session with their audio
        normalised causally towards ``target`` (None: -12 LKFS at 44.1 kHz, ``post.LoudnessTarget()``); ``post.stream_pcm`` composes on top."""
        from . import post
        return post.stream_loudness(blocks, post.LoudnessTarget() if target is None else target)

    # ------------------------------------------------------------------ one step, reference signature
    @torch.no_grad()
    def _sample_next_token(self, sequence: torch.Tensor, condition: torch.Tensor, use_sampling: bool = False,
                           temp: float = 1.0, top_k: int = 0, top_p: float = 0.0, return_attention_weights: bool = False,
                           cfg_scale: float = 1.0) -> Tuple[torch.Tensor, Any, Any]:
        """sequence (B, K, L) int64, condition (B, Tv, 768) -> (next_token (B, K, 1), None, None).
        Stateless like the reference (the whole prefix is given), so it teacher-forces the prefix through
        the decode kernels; ``generate()`` does not go through here."""
        use_cfg = cfg_scale > 1.0 and self.sampler.__class__.__name__ == "Transformer"
        if use_cfg:
            null = torch.zeros_like(condition) + self.sampler.cls_embeddings.uncond_embedding.to(condition.device)
            condition = torch.cat([condition, null], dim=0)
            sequence = sequence.repeat(2, 1, 1)
        logits, _, _ = self.sampler(tgt=sequence, memory=condition, tgt_is_causal=True)
        last = logits[:, :, -1, :].contiguous()
        tok = sample_from_logits(last, use_sampling=use_sampling, temp=temp, top_k=top_k, top_p=top_p,
                                 cfg_scale=cfg_scale if use_cfg else 1.0)
        return tok, None, None

    # ------------------------------------------------------------------ teacher-forced evaluation (vaura_model.py:136-192, 240-295, 339-347)
    @staticmethod
    def _auto_tokens_per_frame(seq_len: int, n_video_tokens: int, codebook_pattern: Optional[str], num_codebooks: int) -> int:
        """llama.py:_set_audio_tokens_per_video_frame: ceil((S - K) / Tv) when the sampler's ``codebook_pattern`` names a delayed
        pattern, ceil((S - 1) / Tv) otherwise — S the length of the pattern sequence the sampler is fed."""
        import math
        n = seq_len - num_codebooks if "delayed" in str(codebook_pattern).lower() else seq_len - 1
        return int(math.ceil(n / n_video_tokens))

    @torch.no_grad()
    def forward(self, frames: torch.Tensor, audio: torch.Tensor, clip_indices: Optional[torch.Tensor] = None, *, audio_lengths=None,
                video_lengths=None):
        """Teacher-forced pass of the reference (vaura_model.py:136-192): frames (B, C, Tv, H, W) and mono audio (B, 1, N) ->
        (logits (B, K, Ta, card), logits_mask (B, K, Ta) bool, aud_feats (B, 9, Ta)).  ``audio_encoder.encode`` (the HIP DAC encode)
        gives the codes, the visual condition comes from ``_handle_visual_conditioning``, and ``DecoderEngine.score`` runs the
        sampler over ``build_pattern_sequence(codes[..., :-1])`` with the heads at every position and reverts the logits on the device
        (it does not go through ``Transformer.forward``).  Two differences from the reference, on purpose:
          * the reference caches the first call's pattern in ``self.pattern`` and reuses it for every later ``Ta``; here the delays
            are taken from ``pattern_provider.get_pattern(Ta)`` for each call's own ``Ta`` (``_pattern_delays``);
          * a ``sampler.audio_tokens_per_video_frame`` of None is set from the sequence as llama.py:_set_audio_tokens_per_video_frame
            does (and kept, as there); ``Transformer.forward`` itself still refuses None.
        Delay patterns give every timestep a logit, so the mask is all true and no reverted row is NaN.
        A padded batch of clips of different durations: ``audio_lengths`` — one int per clip, the samples of ``audio[b]`` that are real —
        and / or ``video_lengths`` (one int per clip, the leading video tokens that are real, as in ``generate``).  The audio is then
        encoded in one pass (``encode_clips``: every clip cut to its own samples, packed into one sequence), so clip b's codes are those of the clip encoded alone
        (``Ta_b`` = what the encoder returns for its samples; ``aud_feats`` is padded with 0 to the longest), the clips are scored in
        one ``DecoderEngine.score_clips`` call, and ``logits_mask[b, :, t]`` = t < Ta_b (the logits rows behind it are NaN):
        ``_compute_loss`` under that mask is the loss of the real frames.  With neither keyword every path is the one it was."""
        aud_feats, lengths = self._encode_clips(audio, audio_lengths)
        B, _, Ta = aud_feats.shape
        vis = self._handle_visual_conditioning(frames, clip_indices, B)
        if vis is None:
            raise NotImplementedError("unconditional scoring: the llama sampler always needs video features (llama.py:474-476)")
        r = self._score(aud_feats[:, :self.num_codebooks], vis, return_logits=True, lengths=lengths, video_lengths=video_lengths)
        return r["logits"], r["mask"], aud_feats

    def _encode_clips(self, audio: torch.Tensor, audio_lengths=None):
        """``audio_encoder.encode`` of a padded batch -> (codes (B, Kc, Ta_max), [Ta_b] or None).  ``audio_lengths`` None: one encode of
        the whole batch, as ever.  Otherwise ``audio_encoder.encode_clips``: one pass over the clips, each cut to its own samples — a clip encoded
        with zero padding behind it is not the clip — packed into one sequence, as ``generate`` decodes them; frames behind Ta_b hold 0."""
        if audio_lengths is None:
            return self.audio_encoder.encode(audio), None
        if not clip_params.is_per_clip(audio_lengths):
            raise L.VauraHipError(f"audio_lengths must be one integer per clip (a list, tuple or 1-D tensor), got {audio_lengths!r}")
        n = clip_params._int_list("audio_lengths", audio_lengths)
        if len(n) != audio.shape[0]:
            raise L.VauraHipError(f"audio_lengths has {len(n)} values for a batch of {audio.shape[0]} clips")
        if min(n) < 1 or max(n) > audio.shape[-1]:
            raise L.VauraHipError(f"audio_lengths must lie in 1 .. {audio.shape[-1]} (the samples of the padded batch), got {n}")
        from .codec_clips import clip_layout
        lengths = list(clip_layout(n, self.audio_encoder.cfg, "encode").frames)
        if len(set(n)) == 1:      # one length: the plain batched pass, the same bits for 2.3 % less
            codes = self.audio_encoder.encode(audio[..., :n[0]])
        else:
            codes = self.audio_encoder.encode_clips(audio[..., :max(n)], n)
        return codes, lengths

    @torch.no_grad()
    def score_relevance(self, frames: torch.Tensor, audio: torch.Tensor, clip_indices: Optional[torch.Tensor] = None, *,
                        audio_lengths=None, video_lengths=None) -> dict:
        """How much of GIVEN audio the video explains: ``forward``'s inputs (frames, mono audio (B, 1, N)) -> ``DecoderEngine.score(...,
        relevance=True)`` of the audio's codes: the teacher-forced cross-entropy under the video ("nll", "nll_per_codebook", "loss",
        "loss_per_codebook") and under the null condition ("nll_null", "nll_null_per_codebook", ...), "relevance_per_codebook" (B, K) =
        nll_null_per_codebook - nll_per_codebook and "relevance" (B,), its mean over the codebooks — nats per token; plus "codes"
        (B, K, Ta), the audio's codes.  ``forward`` / ``test_step`` do not go through here.
        ``audio_lengths`` / ``video_lengths``: a padded batch, as in ``forward`` — every per-clip entry then runs over clip b's own
        frames (``DecoderEngine.score_clips``), "codes" is padded with 0 and the result holds "lengths" (B,)."""
        aud_feats, lengths = self._encode_clips(audio, audio_lengths)
        vis = self._handle_visual_conditioning(frames, clip_indices, aud_feats.shape[0])
        if vis is None:
            raise NotImplementedError("unconditional scoring: the llama sampler always needs video features (llama.py:474-476)")
        codes = aud_feats[:, :self.num_codebooks]
        return dict(self._score(codes, vis, relevance=True, lengths=lengths, video_lengths=video_lengths), codes=codes)

    def _score(self, codes: torch.Tensor, vis: torch.Tensor, return_logits: bool = False, relevance: bool = False, lengths=None,
               video_lengths=None) -> dict:
        """DecoderEngine.score — with per-clip lengths ``score_clips`` — with this model's delays (per call) and tokens per video frame
        (auto-set rule when None)."""
        K = self.num_codebooks
        Ta = int(codes.shape[-1])
        delays = self._pattern_delays(Ta)
        S = Ta + max(delays) + 1
        if S > self.sampler.block_size:
            raise L.VauraHipError(f"{Ta} timesteps under the delays {delays} need {S} sequence steps; block_size is {self.sampler.block_size}")
        if self.sampler.audio_tokens_per_video_frame is None:
            self.sampler.audio_tokens_per_video_frame = self._auto_tokens_per_frame(
                S, int(vis.shape[1]), getattr(self.sampler, "codebook_pattern", None), K)
        eng = self.sampler.engine()
        kw = dict(delays=None if delays == list(range(K)) else delays, tokens_per_frame=self.sampler.audio_tokens_per_video_frame,
                  return_logits=return_logits, **(dict(relevance=True) if relevance else {}))
        if lengths is not None or video_lengths is not None:
            return eng.score_clips(codes, vis.float(), lengths, video_lengths=video_lengths, **kw)
        return eng.score(codes, vis.float(), **kw)

    @torch.no_grad()
    def _compute_loss(self, logits: torch.Tensor, targets: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, List[torch.Tensor]]:
        """vaura_model.py:240-280: per-codebook cross entropy over the valid (mask) entries, averaged over the codebooks ->
        (loss, [loss of codebook k]).  Runs the HIP NLL + fixed-order reduction kernels (``engine.score_logits``)."""
        from .engine import score_logits
        B, K, T = targets.shape
        assert logits.shape[:-1] == targets.shape
        assert mask.shape == targets.shape
        loss, lpc, _ = score_logits(logits, targets, mask)
        return loss, [lpc[k] for k in range(K)]

    @staticmethod
    def _stack_list_repr(list_repr, to_3dim: bool = False) -> torch.Tensor:
        """vaura_model.py:226-238."""
        tensor_repr = torch.stack([torch.stack(tensors) for tensors in list(list_repr)])
        if to_3dim:
            tensor_repr = tensor_repr.view(-1, *tensor_repr.shape[-2:])
        return tensor_repr

    def _shared_step(self, batch, batch_idx):
        """vaura_model.py:282-295 -> (logits, target codes, loss, loss_per_codebook)."""
        audio = batch["audio"] if self.flatten_vis_feats else self._stack_list_repr(batch["audio"], to_3dim=True)
        frames = batch["frames"]
        # a padded batch of clips of different durations says so: "audio_lengths" (samples) / "video_lengths" (video tokens) per clip
        ragged = {k: batch[k] for k in ("audio_lengths", "video_lengths") if batch.get(k) is not None}
        logits, logits_mask, target = self.forward(frames, audio, batch.get("meta", {}).get("clip_indices", None), **ragged)
        loss, loss_per_cb = self._compute_loss(logits, target[:, :self.num_codebooks, :], logits_mask)
        return logits, target, loss, loss_per_cb

    def _shared_log(self, stage: str, loss: torch.Tensor, loss_per_cb) -> None:
        """There is no Lightning logger here: the values the reference logs (``{stage}_loss``, ``{stage}_loss_per_codebook``,
        vaura_model.py:296-316) are kept in ``self.last_eval_log`` for the caller."""
        self.last_eval_log = {f"{stage}_loss": loss, f"{stage}_loss_per_codebook": list(loss_per_cb)}

    def validation_step(self, batch, batch_idx):
        _, _, loss, loss_per_cb = self._shared_step(batch, batch_idx)
        self._shared_log("val", loss, loss_per_cb)
        return loss

    def test_step(self, batch, batch_idx):
        _, _, loss, loss_per_cb = self._shared_step(batch, batch_idx)
        self._shared_log("test", loss, loss_per_cb)
        return loss



def _codec_halo(codec) -> int:
    """Frames of context either side that the samples of one frame depend on, for the codec plugin in use (``codec_clips.decode_halo``)."""
    from .codec_clips import decode_halo
    return decode_halo(codec.cfg)
