"""Host-side owners of device state for the HIP hot path (torch = memory + streams only).

``DecoderEngine``  packs a sampler state dict (reference key names) into the layouts of
                   include/vaura_hip.h, owns K/V cache + workspaces, and drives
                   vaura_prefill_cond / vaura_pattern_* / vaura_generate_loop.
``CodecEngine``    folds weight-norm of a DAC state dict and drives vaura_dac_decode.

Neither has a CPU path: construction fails if libvaura_hip.so cannot be loaded or the
tensors are not on a HIP device.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from typing import Dict, Optional, Sequence

import torch

from . import _lib as L
from . import clip_params
from . import ops
from .synth import CodecCfg, SamplerCfg, fold_weight_norm


def rope_table(n_pos: int, head_dim: int, base: int = 10000) -> torch.Tensor:
    """cos/sin table with the reference's own construction (llama.py:593-603) so that the
    table entries are bit-identical to what the reference multiplies by."""
    inv = 1.0 / (base ** (torch.arange(0, head_dim, 2)[: head_dim // 2].float() / head_dim))
    ang = torch.outer(torch.arange(n_pos), inv)
    z = torch.polar(torch.ones_like(ang), ang)
    return torch.stack([z.real, z.imag], dim=-1).contiguous()


_PRIVATE_STREAMS: Dict[torch.device, "torch.cuda.Stream"] = {}


@contextlib.contextmanager
def off_null_stream(dev: torch.device):
    """Run the enclosed enqueues on a private stream when the caller sits on HIP's legacy null stream.
    hipGraph capture is impossible there, and every launch on it synchronises implicitly with all blocking
    streams (measured: 268 -> 255 ms per configs[1] batch once the whole pass left the null stream).
    Ordered after the caller's pending work and before its later work.  Yields the caller's stream when a
    switch happened (results allocated inside must ``record_stream`` it), else None."""
    dev = torch.device(dev)
    cur = torch.cuda.current_stream(dev)
    if cur.cuda_stream != 0:
        yield None
        return
    side = _PRIVATE_STREAMS.get(dev)
    if side is None:
        side = _PRIVATE_STREAMS[dev] = torch.cuda.Stream(dev)
    side.wait_stream(cur)
    try:
        with torch.cuda.stream(side):
            yield cur
    finally:
        # also on an exception: kernels already enqueued on the side stream must still be ordered before later null-stream work
        cur.wait_stream(side)


def h_row_scales(w: torch.Tensor) -> torch.Tensor:
    """The power-of-two row scales of the fp16-plane storages (csrc/gemv3.hip h_row_scale_kernel): 2^(e - 14) with
    max|W[n, :]| = m * 2^e, m in [0.5, 1), i.e. max|W[n, :]| / scale in [2^13, 2^14); 1 for an all-zero row."""
    amax = w.detach().float().abs().amax(dim=1)
    _, e = torch.frexp(amax)
    return torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), e - 14), torch.ones_like(amax))


def h_effective_weight(w: torch.Tensor, planes: int) -> torch.Tensor:
    """The real-number matrix that ``planes`` fp16 planes hold: hi = fp16(W / scale), lo = fp16(W / scale - hi), times scale."""
    w = w.detach().float()
    sc = h_row_scales(w)[:, None]
    v = w / sc
    hi = v.half().float()
    q = hi if planes == 1 else hi + (v - hi).half().float()
    return q * sc


def h1_lossless(w: torch.Tensor) -> bool:
    """True when ONE fp16 plane (with its power-of-two row scale) holds every element of ``w``: half the HBM bytes, same real
    numbers.  bf16-representable weights qualify down to 2^-31 of their row's largest; a smaller element is held to 2^-39 of
    that maximum — below the resolution of any fp32 sum it enters — and does not disqualify the matrix."""
    w = w.detach().float()
    err = (h_effective_weight(w, 1) - w).abs()
    tol = w.abs().amax(dim=1, keepdim=True) * 2.0 ** -38
    return bool((err <= tol).all())


def fold_gain(g: torch.Tensor, plane_shift: int = 0):
    """(g 2^-E, 2^E) with E = max(0, ceil(log2 max|g|)) + plane_shift: the RMSNorm gain as the planes carry it and the factor its
    consuming matrix takes instead (both exact: powers of two)."""
    g = g.detach().float()
    m = float(g.abs().max())
    e = (max(0, math.ceil(math.log2(m))) if m > 0 and math.isfinite(m) else 0) + int(plane_shift)
    return g * (2.0 ** -e), 2.0 ** e


def streamed_matrices(sd: Dict[str, torch.Tensor]):
    """The matrices the decode loop streams every step (98 % of the bytes)."""
    from .synth import is_streamed_weight
    return [k for k in sd if is_streamed_weight(k)]


WEIGHT_DTYPES = ("h1", "h2", "fp8", "fp8h", "f32")
KV_DTYPES = ("f32", "f16", "f8", "f8s")      # K / V cache storages, in the order of vaura_decoder.kv_dtype


def resolve_weight_dtype(sd: Dict[str, torch.Tensor], wdtype: str) -> str:
    """Storage of the streamed matrices:
      "h2"   (hi, lo) fp16 planes, 22 significand bits, 4 bytes per weight: any fp32 checkpoint on the pair kernels — what
             "auto" picks for a real V-AURA checkpoint (fp32 master weights; the reference runs the sampler in fp32,
             configs/vaura_defaults.yaml `precision: 32`).  Logits within ~1e-5 of the fp32 reference, greedy tokens of every
             reference golden unchanged.
      "h1"   one fp16 plane, 2 bytes per weight — "auto" picks it when that loses nothing (``h1_lossless``: e.g. a
             bf16-representable checkpoint); forced on another checkpoint it ROUNDS the weights to 11 bits (not token-exact).
      "fp8"  e4m3 + row scales for the per-layer matrices (BASELINE configs[4]; a different model), multiplied against both
             activation planes: the "h1" arithmetic on ``quant.fp8_effective_state_dict(sd)``, token-exact against the oracle on it.
      "fp8h" (round 6) the same packed bytes against the HI activation plane only — 11-bit activations under 4-bit-significand
             weights, half the plane bytes each CU takes in: configs[4]'s measured configuration; tolerance against "fp8" / "h1"
             is REPORTED (tests, bench.py), not bit parity.
      "f32"  fp32 tiles on the exact-fp32-MFMA GEMVs (gemv_kernel.h): bit-for-bit fp32 products, 1/16 of the MFMA rate —
             the cross-check the pair kernels are tested against.
    ("bf16" is accepted as an alias of "h1": round 2's name for the 2-byte storage.)"""
    if wdtype == "bf16":
        wdtype = "h1"
    if wdtype != "auto":
        if wdtype not in WEIGHT_DTYPES:
            raise L.VauraHipError(f"weight_dtype must be auto | {' | '.join(WEIGHT_DTYPES)}, got {wdtype!r}")
        return wdtype
    return "h1" if all(h1_lossless(sd[k]) for k in streamed_matrices(sd)) else "h2"


def _require_cuda(dev: torch.device):
    if torch.device(dev).type != "cuda":
        raise L.VauraHipError(f"the V-AURA hot path runs on a HIP device only (got {dev}); there is no CPU fallback")
    L.lib()


# Near-tie detector (csrc/step.hip sample_kernel, include/vaura_hip.h vaura_sampling.tie_eps): relative bound on the error of a logit the
# plane storages deliver against the reference's fp32 (x the row's largest |logit|, x (2 cfg - 1) through the CFG mix).  Calibrated on
# the reference's own goldens (tools/near_tie_sweep.py -> profiles/r06_near_tie_sweep.txt; tests/test_gpu_generate.py::test_near_tie_*):
# bounds in [1.2e-6, 2e-6) flag the two literal near-ties the goldens hold (configs[3] step 578: margin 5.5e-6; the later chunk's step
# 175: 3.8e-6) and nothing else in any golden run (4 104 sampled + 4 104 greedy cfg-6 decisions, 7 920 + 1 134 greedy ones).
NEAR_TIE_EPS = 1.5e-6


class DecoderEngine:
    # hand-off epochs carry 10 bits of this counter (csrc/common.h va_handoff_epoch) and the arrival words of the in-launch hand-offs live
    # in LDS, which outlives processes: start every process somewhere else, so that two processes taking turns on one GPU do not
    # produce identical tag sequences
    _sequence_id = (os.getpid() * 0x9E37 + int.from_bytes(os.urandom(2), "little")) & 0x3FF

    def __init__(self, cfg: SamplerCfg, sd: Dict[str, torch.Tensor], device="cuda:0", wdtype: str = "auto",
                 one_launch_mlp: bool = True, range_fallback: bool = True, plane_shift: int = 0,
                 near_tie: str = "report", near_tie_eps: Optional[float] = None, kv_dtype: str = "f32"):
        """wdtype: storage of the streamed matrices — "auto" | "h1" | "h2" | "fp8" | "fp8h" | "f32" (``resolve_weight_dtype``).
        one_launch_mlp: let the library run w1||w3 -> w2 of a layer as ONE launch with an in-launch hand-off where the shape
        is eligible (1..16 decoder rows, fp16-plane weights, >= 256 CUs; csrc/mlp_engine.h: bit-identical results, -5..7 % on the
        decode loop).  Its consumers wait for producers of the SAME launch, so every workgroup must become resident: pass False
        when several processes share this GPU, or when several DecoderEngines of ONE process run on different streams at the same
        time (each launch wants all 256 CUs, one workgroup per CU: two such launches can starve each other until their bounded waits
        give up).  A give-up is reported by ``check_status`` — which callers of ``generate_codes`` / ``run`` must call themselves,
        ``VAURAModel.generate_tokens`` does.
        plane_shift: S in 0..24 (fp16-plane storages only).  EVERY activation plane set is stored times 2^-S and the matrix that consumes
        it times 2^S (h planes: through ``fold_gain``; attention output and SwiGLU output: ``vaura_decoder.plane_shift``) — the planes
        overflow at |activation| = 65504 * 2^S instead of 65504, at the same speed.  The price is at the other end of fp16: the lo
        plane's absolute resolution is 2^-24 * 2^S (its subnormal step), so S = 0 is what every parity number is quoted on, and a
        checkpoint KNOWN to carry massive activations is the reason to pass S = 4 .. 8 rather than pay the exact-fp32 twin on every call."""
        self.one_launch_mlp = bool(one_launch_mlp)
        self.handoff_fallbacks = 0           # calls re-run on the separate launches after an in-launch hand-off gave up (GPU shared)
        # near-tie detector: "off" | "report" (count decisions inside the arithmetic's noise: ``near_ties`` / ``last_near_ties``) |
        # "rerun" (``generate_codes_checked`` re-runs a flagged call on the exact-fp32 twin, like an overflow)
        if near_tie not in ("off", "report", "rerun"):
            raise L.VauraHipError(f"near_tie must be off | report | rerun, got {near_tie!r}")
        self.near_tie = near_tie
        self.near_tie_eps = float(NEAR_TIE_EPS if near_tie_eps is None else near_tie_eps)
        self.near_ties = 0                   # decisions flagged so far (all calls)
        self.last_near_ties = (0, None)      # (count, first flagged step) of the last checked call
        self.near_tie_reruns = 0
        # K / V cache: "f32" (every parity number) or "f16" (round 6; the low-precision serving configuration, BASELINE configs[4] together
        # with weight_dtype="fp8h": fp16(rotated k) / fp16(v), half the attention's stream; caches of at most 256 positions, plane storages)
        # "f8": OCP e4m3 bytes, unscaled and saturating — a quarter of the fp32 stream, a ~1e-2-class approximation of the attention (still an
        # order of magnitude below the fp8 weights' own error); an OPTION of that configuration, reported beside "f16"
        # "f8s": the same e4m3 bytes scaled per cached vector — one E8M0 exponent byte per 96-channel k or v (97 bytes against 96), chosen
        # so that the vector's largest |value| lands in (224, 448]: nothing saturates or drops to zero whatever the checkpoint's range,
        # and a non-finite k / v stays non-finite (include/vaura_hip.h, vaura_decoder.kv_dtype = 3): the range-safe fp8 option
        if kv_dtype not in KV_DTYPES:
            raise L.VauraHipError(f"kv_dtype must be {' | '.join(KV_DTYPES)}, got {kv_dtype!r}")
        self.kv_dtype = kv_dtype
        self.plane_shift = int(plane_shift)
        if not 0 <= self.plane_shift <= 24:
            raise L.VauraHipError(f"plane_shift must be in 0..24, got {plane_shift}")
        # Range safety (``generate_codes_checked``): the fp16-plane activation format ends at |x| = 65504; a call that overflows it is
        # DETECTED on the device (sticky status bit) and re-run from its start on a twin engine with weight_dtype="f32" (fp32
        # activations and weights on the exact-fp32 matrix instruction: no range limit, the reference's own arithmetic), built lazily
        # from the same state dict the first time it is needed.  The dict is kept by reference only (no copy).
        self._twin_sd = sd if range_fallback else None
        self._range_twin: Optional["DecoderEngine"] = None
        self.range_fallbacks = 0             # calls re-run on the exact-fp32 twin so far
        self._forward_on_twin = False        # forward_cached moved to the twin for good (the host's per-step calls)
        _require_cuda(device)
        self.cfg = cfg
        self.dev = torch.device(device)
        self.requested_wdtype = wdtype
        wdtype = resolve_weight_dtype(sd, wdtype)
        self.planes = wdtype != "f32"          # activations travel as (hi, lo) fp16 planes; "f32" = the exact-fp32-MFMA step
        if self.plane_shift and not self.planes:
            raise L.VauraHipError("plane_shift applies to the fp16-plane storages (h1 | h2 | fp8) only")
        S, pw = self.plane_shift, 2.0 ** self.plane_shift
        # "fp8": e4m3 + power-of-two row scales for the four per-layer matrices (BASELINE configs[4]); the codebook
        # heads stay one fp16 plane.  The model then IS the one with weights quant.fp8_effective_weight(W): same kernels,
        # same activation arithmetic.
        self.wd = {"f32": L.W_F32, "h1": L.W_H1, "h2": L.W_H2, "fp8": L.W_FP8, "fp8h": L.W_FP8H}[wdtype]
        head_wd = L.W_H1 if wdtype in ("fp8", "fp8h") else self.wd
        self.wdtype = wdtype
        # lossy storages (fp8 / fp8h; one plane FORCED on a checkpoint it cannot hold) are a different model than the state dict: their
        # exact-fp32 twin must hold the numbers the storage holds, or a call that falls back would be decoded by another model than
        # the other calls of the same job.  Resolved lazily in _twin().
        self._twin_lossy_cached: Optional[bool] = None
        self.lib = L.lib()
        D, F, K = cfg.d_model, cfg.ffn_dim, cfg.num_codebooks
        with torch.cuda.device(self.dev):
            self._keep = []  # device tensors referenced by raw pointers
            lw = (L.LayerWeights * cfg.num_layers)()
            for l in range(cfg.num_layers):
                p = f"layers.{l}."
                w1 = sd[p + "feed_forward.w1.weight"].float()
                w3 = sd[p + "feed_forward.w3.weight"].float()
                w13 = torch.stack([w1.view(F // 16, 16, D), w3.view(F // 16, 16, D)], dim=1).reshape(2 * F, D)
                # Norm gains leave the planes (range): rmsnorm's gain g multiplies the residual stream BEFORE it is split into fp16 planes
                # (the producer's epilogue), so a large gain eats the planes' range.  Fold a power of two out of it: the planes hold
                # (g 2^-E) * h with max |g 2^-E| <= 1 and the consuming matrix is stored as W 2^E — exact on both sides (its power-of-two
                # row scales absorb it; W (g * x) == (W 2^E) ((g 2^-E) * x) bit for bit), E = 0 for gains <= 1 (every golden).
                ga, ea = fold_gain(sd[p + "attention_norm.weight"], S)
                gf, ef = fold_gain(sd[p + "ffn_norm.weight"], S)
                lw[l].wqkv = L.ptr(self._pack(sd[p + "attention.wqkv.weight"].float() * ea, self.wd))
                lw[l].wo = L.ptr(self._pack(sd[p + "attention.wo.weight"].float() * pw, self.wd))
                lw[l].w13 = L.ptr(self._pack(w13 * ef, self.wd))
                lw[l].w2 = L.ptr(self._pack(sd[p + "feed_forward.w2.weight"].float() * pw, self.wd))
                lw[l].attn_norm = L.ptr(self._dev(ga))
                lw[l].ffn_norm = L.ptr(self._dev(gf))
            self.layers = lw
            gn, en = fold_gain(sd["norm.weight"], S)
            heads = torch.cat([sd[f"lm_heads.{k}.weight"].float() for k in range(K)], dim=0) * en
            self.heads = self._pack(heads, head_wd)
            self.final_norm = self._dev(gn)
            self.fc1 = self._pack(sd["cls_embeddings.projection.fc1.weight"], L.W_F32)
            self.fc2 = self._pack(sd["cls_embeddings.projection.fc2.weight"], L.W_F32)
            self.uncond = self._dev(sd["cls_embeddings.uncond_embedding"])
            self.empty_video = self._dev(sd["empty_video_emb"].reshape(-1))
            self.tok_emb = self._dev(torch.stack([sd[f"tok_embeddings.{k}.emb.weight"].float() for k in range(K)]))
            self.tok_w = self._dev(torch.stack([
                fold_weight_norm(sd[f"tok_embeddings.{k}.out_proj.weight_g"].float(),
                                 sd[f"tok_embeddings.{k}.out_proj.weight_v"].float())[:, :, 0] for k in range(K)]))
            self.tok_b = self._dev(torch.stack([sd[f"tok_embeddings.{k}.out_proj.bias"].float() for k in range(K)]))
            self.tok_table = torch.empty(K, cfg.d_codebook + 1, cfg.tok_dim, dtype=torch.float32, device=self.dev)
            self._keep.append(self.tok_table)
            L.check(self.lib.vaura_build_token_table(L.ptr(self.tok_emb), L.ptr(self.tok_w), L.ptr(self.tok_b),
                                                     L.ptr(self.tok_table), K, cfg.d_codebook + 1, cfg.codebook_dim,
                                                     cfg.tok_dim, L.current_stream(self.dev)), "vaura_build_token_table")
            torch.cuda.synchronize(self.dev)
        self.dims = L.Dims(cfg.num_layers, D, cfg.nhead, F, K, cfg.d_codebook, cfg.cond_dim, cfg.tok_dim, cfg.cond_in,
                           cfg.codebook_dim, 7, cfg.layer_norm_eps)
        self.dec: Optional[L.Decoder] = None
        self.state = None
        self._carried_status = 0             # status bits read off a state buffer that prepare() was about to replace
        self._shape = None
        self.delays: Optional[tuple] = None  # codebook delay pattern of the prepared shape (None = 0..K-1)
        self._graph, self._graph_key = None, None
        self.live_owner = None               # the live session whose first chunk is in the buffers (begin_live), until the next prepare()
        self.weight_bytes = sum(t.numel() * t.element_size() for t in self._keep)

    # ------------------------------------------------------------------ helpers
    def _dev(self, t: torch.Tensor) -> torch.Tensor:
        d = t.detach().to(self.dev, torch.float32).contiguous()
        self._keep.append(d)
        return d

    def _pack(self, w: torch.Tensor, wd: int) -> torch.Tensor:
        N, K = w.shape
        src = w.detach().to(self.dev, torch.float32).contiguous()
        dst = torch.empty(self.lib.vaura_packed_weight_bytes(N, K, wd), dtype=torch.uint8, device=self.dev)
        L.check(self.lib.vaura_pack_weight(L.ptr(src), L.ptr(dst), N, K, wd, L.current_stream(self.dev)), "vaura_pack_weight")
        torch.cuda.current_stream(self.dev).synchronize()  # src may be freed right after
        self._keep.append(dst)
        return dst

    @staticmethod
    def _rows_padded(r: int) -> int:
        return (r + 15) // 16 * 16

    # ------------------------------------------------------------------ per-call state
    # prompt positions teacher-forced per pass (bf16 / fp8 storage); the workspaces scale with it.  192 covers the
    # sliding-window caller's 166-token prompt in one GEMM pass (96 ms per chunk; 106 ms at 64, 120 ms at 32)
    PREFILL_POSITIONS = 192

    def pattern_delays(self, delays: Optional[Sequence[int]]) -> Optional[tuple]:
        """The codebook delay pattern as the engine keys it: None for the default (the zero-filled descriptor), otherwise the
        checked tuple (``_lib.check_delays``; an explicit 0..K-1 goes through the descriptor's delays and gives the same bits)."""
        return None if delays is None else L.check_delays(delays, self.cfg.num_codebooks)

    def prepare(self, batch: int, timesteps: int, n_cond_tokens: int, cfg_on: bool, tokens_per_frame: int = 7,
                block_size: Optional[int] = None, delays: Optional[Sequence[int]] = None):
        """delays: the codebook delay pattern (None = 0..K-1): S = timesteps + max(d) + 1 sequence steps."""
        c = self.cfg
        K = c.num_codebooks
        delays = self.pattern_delays(delays)
        S = timesteps + (K if delays is None else max(delays) + 1)
        if delays is not None and block_size and S > block_size:
            raise L.VauraHipError(f"delay pattern {list(delays)} with {timesteps} timesteps needs {S} sequence steps; the model's "
                                  f"block_size is {block_size}")
        rows = 2 * batch if cfg_on else batch
        max_len = (max(S, block_size or 0) + 31) // 32 * 32
        key = (batch, timesteps, n_cond_tokens, cfg_on, tokens_per_frame, max_len, delays)
        self._fc = None                       # whoever prepares the engine is about to overwrite the K/V cache
        self.live_owner = None                # ... and the sequence of a live session's first chunk (live.LiveSession checks before it goes on)
        if self._shape == key:
            return
        if getattr(self, "state", None) is not None:      # an unread status bit must survive the reallocation below
            self._carried_status |= int(self.state[4].item())
        with torch.cuda.device(self.dev):
            pp = min(self.PREFILL_POSITIONS, S) if self.planes else 1
            rp = self._rows_padded(rows) * pp     # decode uses the first position's worth of row blocks
            f32 = dict(dtype=torch.float32, device=self.dev)
            self.rope = rope_table(max_len, c.head_dim, c.rope_base).to(self.dev)
            if self.kv_dtype != "f32":
                if max_len > 256 or not self.planes:
                    raise L.VauraHipError(f"kv_dtype={self.kv_dtype!r} serves caches of at most 256 positions on the fp16-plane storages (got max_len "
                                          f"{max_len}, weights {self.wdtype})")
                self.kcache = torch.zeros(c.num_layers, rows, c.nhead, max_len, c.head_dim, device=self.dev,
                                          dtype=torch.float16 if self.kv_dtype == "f16" else torch.uint8)
            else:
                self.kcache = torch.zeros(c.num_layers, rows, c.nhead, max_len, c.head_dim, **f32)
            self.vcache = torch.zeros_like(self.kcache)
            self.kscale = self.vscale = None      # "f8s": the exponent byte of every cached vector
            if self.kv_dtype == "f8s":
                self.kscale = torch.zeros(c.num_layers, rows, c.nhead, max_len, device=self.dev, dtype=torch.uint8)
                self.vscale = torch.zeros_like(self.kscale)
            self.seq = torch.zeros(batch, K, S, dtype=torch.int32, device=self.dev)
            self.state = torch.zeros(8, dtype=torch.int32, device=self.dev)   # include/vaura_hip.h: position, arrivals, step, id, STATUS, spare
            self.ws_h = torch.zeros(rp * c.d_model, **f32)
            self.ws_qkv = torch.zeros(rp * 3 * c.d_model, **f32)
            self.ws_qkv2 = torch.zeros(self._rows_padded(rows) * 3 * c.d_model, **f32)   # decode step only
            self.ws_attn = torch.zeros(rp * c.d_model, **f32)
            self.ws_ffn = torch.zeros(rp * c.ffn_dim, **f32)
            self.ws_logits = torch.zeros(rows, K * c.d_codebook, **f32)
            self._prefill_positions = pp if pp > 1 else 0
            i16 = dict(dtype=torch.int16, device=self.dev)
            self.ws_h_split = torch.zeros(rp * 2 * c.d_model, **i16)       # (hi, lo) fp16 planes
            self.ws_attn_split = torch.zeros(rp * 2 * c.d_model, **i16)
            self.ws_ffn_split = torch.zeros(rp * 2 * c.ffn_dim, **i16)
            self.ws_ss = torch.zeros((rp // 16) * (c.d_model // 16) * 16, **f32)
            self.ws_attn_part = torch.zeros(rows * c.nhead * 8 * (c.d_model // c.nhead + 8), **f32)
            self.ws_sync = torch.zeros(768, dtype=torch.int32, device=self.dev)
            crp = self._rows_padded(rows * n_cond_tokens)
            self.cond_in = torch.zeros(crp * c.cond_in, **f32)
            self.cond_tmp = torch.zeros(crp * c.cond_dim, **f32)
            self.cond_proj = torch.zeros(crp * c.cond_dim, **f32)
            self.codes_i32 = torch.zeros(batch, K, timesteps, dtype=torch.int32, device=self.dev)
            self.clip_params = torch.zeros(batch, 8, dtype=torch.int32, device=self.dev)   # vaura_clip_sampling records (per-clip calls)
            self.logprobs = torch.zeros(batch, K, S, **f32)     # token log-probabilities in the layout of seq (return_logprobs calls)
            self.logprobs_cond = self.logprobs_null = None      # video relevance (return_relevance calls): allocated by the first such call
            # per-clip lengths of a ragged call (vaura_decoder_ext2): T_b and Tv_b.  Engine-owned like clip_params: the descriptor and a
            # captured step graph hold the POINTERS, _set_lengths() rewrites the values
            self.clip_T = torch.zeros(batch, dtype=torch.int32, device=self.dev)
            self.clip_Tv = torch.zeros(batch, dtype=torch.int32, device=self.dev)
            # per-clip prompt lengths (vaura_decoder_ext3): n_r = P_b + delays[0] of every row, and P_b of every clip (the first frame
            # of its means).  Engine-owned for the same reason: _set_prompt_lengths() rewrites the values
            self.row_n = torch.zeros(rows, dtype=torch.int32, device=self.dev)
            self.clip_P = torch.zeros(batch, dtype=torch.int32, device=self.dev)
        self.lengths = self.video_lengths = None      # the host lists of the call being run (None: every clip has T / Tv)
        self.prompt_lengths = None                    # likewise: P of every clip of the batch (None: one prompt length for the call)
        # the descriptor + the relevance pointers + the per-clip lengths + the prompt lengths + the attention-map request behind it (all
        # NULL: the descriptor alone).  ext_bytes says how much of it the library reads: the ext3 part, and the whole of it only in a call
        # that asks for attention maps (_set_attention)
        self.dec_ext4 = L.DecoderExt4()
        self.dec_ext3 = self.dec_ext4.ext3
        self.dec_ext2 = self.dec_ext3.ext2
        self.dec_ext = self.dec_ext2.ext   # views: byref(self.dec) points into dec_ext4
        self.attn_probs = None             # the reported weights of the call being run (return_attention_weights), else None
        d = self.dec_ext.dec
        d.ext_bytes = C.sizeof(L.DecoderExt3) - C.sizeof(L.Decoder)
        d.dims = self.dims
        d.dims.tokens_per_frame = tokens_per_frame
        d.wdtype, d.batch, d.rows, d.max_len = self.wd, batch, rows, max_len
        d.timesteps, d.seq_len, d.n_cond_tokens = timesteps, S, n_cond_tokens
        d.prefill_positions = self._prefill_positions
        d.plane_shift = self.plane_shift
        d.kv_dtype = KV_DTYPES.index(self.kv_dtype)
        d.kscale, d.vscale = L.ptr(self.kscale), L.ptr(self.vscale)
        d.clip_sampling = 0                # set per call by _sampling(): NULL = the scalars of the call's vaura_sampling
        d.logprobs = 0                     # set per call by generate_codes(return_logprobs=True): NULL = the sampler without them
        if delays is not None:             # zero-filled = the default pattern (include/vaura_hip.h)
            d.has_pattern_delays = 1
            for q, dq in enumerate(delays):
                d.pattern_delays[q] = dq
        d.layers_host = C.cast(self.layers, C.POINTER(L.LayerWeights))
        d.heads, d.final_norm = L.ptr(self.heads), L.ptr(self.final_norm)
        d.tok_emb, d.tok_proj_w, d.tok_proj_b = L.ptr(self.tok_emb), L.ptr(self.tok_w), L.ptr(self.tok_b)
        d.tok_table = L.ptr(self.tok_table)
        d.empty_video, d.rope, d.cond_proj = L.ptr(self.empty_video), L.ptr(self.rope), L.ptr(self.cond_proj)
        d.kcache, d.vcache, d.seq, d.state = L.ptr(self.kcache), L.ptr(self.vcache), L.ptr(self.seq), L.ptr(self.state)
        d.noise = 0
        d.ws_h, d.ws_qkv, d.ws_attn = L.ptr(self.ws_h), L.ptr(self.ws_qkv), L.ptr(self.ws_attn)
        d.ws_qkv2 = L.ptr(self.ws_qkv2) if self.planes else 0
        d.ws_ffn, d.ws_logits = L.ptr(self.ws_ffn), L.ptr(self.ws_logits)
        if self.planes:
            d.ws_h_split, d.ws_attn_split = L.ptr(self.ws_h_split), L.ptr(self.ws_attn_split)
            d.ws_ffn_split, d.ws_ss = L.ptr(self.ws_ffn_split), L.ptr(self.ws_ss)
        else:   # NULL split workspaces select the exact-fp32-MFMA step (api.hip enqueue_step)
            d.ws_h_split = d.ws_attn_split = d.ws_ffn_split = d.ws_ss = 0
        d.first_norm = self.layers[0].attn_norm
        d.ws_attn_part = L.ptr(self.ws_attn_part)
        d.ws_sync = L.ptr(self.ws_sync) if self.one_launch_mlp else 0      # producer flags of the one-launch MLP (csrc/mlp_engine.h); NULL -> two launches
        self.dec = d
        self._shape = key
        self._graph_key = None
        self.batch, self.rows, self.T, self.S, self.Tv, self.max_len = batch, rows, timesteps, S, n_cond_tokens, max_len
        self.delays = delays

    def kv_bytes_per_position(self) -> int:
        c = self.cfg
        return 2 * c.num_layers * self.rows * c.d_model * 4

    def set_condition(self, feats: torch.Tensor, replicate: int = 1):
        """feats (B, Tv, 768) fp32 on device.  Rows [B, 2B) get the CFG null embedding
        (models/vaura_model.py:790-793) when the engine was prepared with cfg_on.
        ``replicate`` = N > 1 (best-of-N): the engine is prepared for B * N clips, feats holds the B distinct ones.  The MLP runs on
        those B (+ B null) rows once; the projected rows are then copied N times each on the device (unpack, gather, pack), clip b
        to rows b * N .. b * N + N - 1 of its half.  A projected row depends on nothing but its own input row, so the copies are the
        bits that projecting the repeated features would give."""
        assert self.dec is not None
        self._fc = None
        B, Tv, Cin = feats.shape
        N = int(replicate)
        assert B * N == self.batch and Tv == self.Tv and Cin == self.cfg.cond_in
        doubled = self.rows == 2 * self.batch
        x = feats.to(self.dev, torch.float32)
        if doubled:
            if Tv != self.uncond.shape[0]:
                raise L.VauraHipError(f"CFG null embedding has {self.uncond.shape[0]} tokens, condition has {Tv}")
            x = torch.cat([x, torch.zeros_like(x) + self.uncond], dim=0)
        n = x.shape[0] * Tv                   # rows the MLP runs on: self.rows * Tv / N
        x = x.reshape(n, Cin).contiguous()
        st = L.current_stream(self.dev)
        L.check(self.lib.vaura_pack_rows(L.ptr(x), L.ptr(self.cond_in), n, Cin, st), "vaura_pack_rows")
        L.check(self.lib.vaura_prefill_cond(C.byref(self.dims), L.ptr(self.cond_in), L.ptr(self.fc1), L.ptr(self.fc2),
                                            L.W_F32, L.ptr(self.cond_tmp), L.ptr(self.cond_proj), n, st),
                "vaura_prefill_cond")
        self._cond_keepalive = x
        if N > 1:
            cd = self.cfg.cond_dim
            once = torch.empty(n, cd, dtype=torch.float32, device=self.dev)
            L.check(self.lib.vaura_unpack_rows(L.ptr(self.cond_proj), L.ptr(once), n, cd, st), "vaura_unpack_rows")
            rep = once.view(-1, Tv * cd).repeat_interleave(N, dim=0).reshape(self.rows * Tv, cd).contiguous()
            L.check(self.lib.vaura_pack_rows(L.ptr(rep), L.ptr(self.cond_proj), self.rows * Tv, cd, st), "vaura_pack_rows")
            self._cond_keepalive = (x, once, rep)

    def cond_projection(self) -> torch.Tensor:
        """(rows, Tv, cond_dim) row-major view of the hoisted video MLP output (tests)."""
        n = self.rows * self.Tv
        out = torch.empty(n, self.cfg.cond_dim, dtype=torch.float32, device=self.dev)
        L.check(self.lib.vaura_unpack_rows(L.ptr(self.cond_proj), L.ptr(out), n, self.cfg.cond_dim, L.current_stream(self.dev)),
                "vaura_unpack_rows")
        return out.view(self.rows, self.Tv, self.cfg.cond_dim)

    # ------------------------------------------------------------------ generation
    def _sampling(self, use_sampling, temp, top_k, top_p, cfg_scale, seed, clip_base) -> L.Sampling:
        """The call's ``vaura_sampling``.  Each of the five parameters is a scalar or a length-B sequence / tensor (clip_params.py):
        any sequence selects the per-clip path — the records go into the engine-owned device buffer the descriptor (and a captured
        step graph) points at, and the struct then only says whether the rows are doubled; an all-scalar call leaves the descriptor's
        pointer NULL and is the call it always was."""
        tie = self.near_tie_eps if (self.near_tie != "off" and self.planes) else 0.0      # the exact-fp32 engine IS the reference's arithmetic
        per_clip = clip_params.resolve(self.batch, use_sampling, temp, top_k, top_p, cfg_scale)
        if per_clip is not None:
            doubled = self.rows == 2 * self.batch
            for b in range(self.batch):
                us, tp, tk, pp, cs = (per_clip[n][b] for n in clip_params.NAMES)
                if us and tp > 0.0 and not pp > 0.0 and tk > self.cfg.d_codebook:
                    raise L.VauraHipError(f"top_k = {tk} of clip {b} exceeds the codebook size {self.cfg.d_codebook} (the reference's "
                                          "torch.topk raises as well)")
                if cs > 1.0 and not doubled:
                    raise L.VauraHipError(f"cfg_scale = {cs} of clip {b} needs the null-condition rows: prepare the engine with cfg_on "
                                          f"(rows = {self.rows}, batch = {self.batch})")
            host = torch.frombuffer(bytearray(clip_params.pack_records(per_clip)), dtype=torch.int32).view(self.batch, 8)
            self.clip_params.copy_(host)          # on the current stream, ahead of the loop that reads it
            self.dec.clip_sampling = L.ptr(self.clip_params)
            # scalars: unread by the per-clip sampler, except that cfg_scale > 1 states "rows [B, 2B) exist" (include/vaura_hip.h).
            # Nothing here depends on the values, so the bytes of this struct key ONE graph for every per-clip call of a shape.
            return L.Sampling(0, 1.0, 0, 0.0, 2.0 if doubled else 1.0, int(seed), int(clip_base), 0, float(tie))
        if self.dec is not None:
            self.dec.clip_sampling = 0
        use_sampling, temp, top_k, top_p, cfg_scale = (clip_params._scalar(v) for v in (use_sampling, temp, top_k, top_p, cfg_scale))
        if use_sampling and temp > 0.0 and not top_p > 0.0 and int(top_k) > self.cfg.d_codebook:
            # the reference's sample_top_k is torch.topk(probs, k) (utils/utils.py:172): k beyond the codebook raises there too
            raise L.VauraHipError(f"top_k = {top_k} exceeds the codebook size {self.cfg.d_codebook} (the reference's torch.topk raises as well)")
        return L.Sampling(int(bool(use_sampling)), float(temp), int(top_k), float(top_p),
                          float(cfg_scale if self.rows == 2 * self.batch else 1.0), int(seed), int(clip_base), 0, float(tie))

    def _set_lengths(self, lengths: Optional[Sequence[int]], video_lengths: Optional[Sequence[int]]):
        """The per-clip lengths of the call about to run (lists of ``batch`` ints, already checked by ``clip_params.resolve_lengths``;
        None: every clip has T / Tv): written into the engine-owned device arrays on the current stream, and the descriptor points
        at them or holds NULL."""
        for vals, buf, name in ((lengths, self.clip_T, "clip_timesteps"), (video_lengths, self.clip_Tv, "clip_cond_tokens")):
            if vals is not None:
                assert len(vals) == self.batch
                buf.copy_(torch.tensor(vals, dtype=torch.int32))
            setattr(self.dec_ext2, name, L.ptr(buf) if vals is not None else 0)
        self.lengths = None if lengths is None else list(lengths)
        self.video_lengths = None if video_lengths is None else list(video_lengths)
        self._set_prompt_lengths(None)     # a call has per-clip prompt lengths only where it says so right after this (generate_codes)
        self._set_attention(None, 0, 0)    # ... and attention maps likewise

    def _set_prompt_lengths(self, prompt_lengths: Optional[Sequence[int]]):
        """The per-clip prompt lengths of the call about to run (one int per clip of the prepared batch, candidates repeated; already
        checked by ``clip_params.resolve_prompt_lengths``; None: one prompt length for the whole call): n_r of every row and P_b of
        every clip go into the engine-owned device arrays on the current stream, and the descriptor points at the first or holds NULL."""
        if prompt_lengths is not None:
            assert len(prompt_lengths) == self.batch
            d0 = self.delays[0] if self.delays else 0
            self.row_n.copy_(torch.tensor(clip_params.prompt_row_steps(prompt_lengths, d0, self.rows == 2 * self.batch), dtype=torch.int32))
            self.clip_P.copy_(torch.tensor(list(prompt_lengths), dtype=torch.int32))
        self.dec_ext3.row_prompt_steps = L.ptr(self.row_n) if prompt_lengths is not None else 0
        self.prompt_lengths = None if prompt_lengths is None else list(prompt_lengths)

    def _set_attention(self, layer: Optional[int], pos0: int, n_steps: int):
        """The attention-map request of the call about to run (``layer`` None: none — the descriptor ends behind its ext3 part, as in
        every call before this keyword existed).  Otherwise layer ``layer`` reports the softmax weights of the ``n_steps`` decode steps
        from cache position ``pos0`` on, for the ``batch`` conditional rows: (n_steps, batch, n_head, max_len) fp32, zeroed here on the
        current stream — 4 * n_steps * batch * 16 * max_len bytes, 30 MB at 8 clips x 228 steps x 256 positions.  The buffer is kept
        while the shape of the request stays, so that such calls replay one captured graph."""
        x, d = self.dec_ext4, self.dec
        if layer is None:
            self.attn_probs = None
            x.attn_probs, x.attn_layer, x.attn_pos0, x.attn_steps, x.attn_rows = 0, 0, 0, 0, 0
            d.ext_bytes = C.sizeof(L.DecoderExt3) - C.sizeof(L.Decoder)
            return
        shape = (int(n_steps), self.batch, self.cfg.nhead, self.max_len)
        buf = getattr(self, "_attn_buf", None)
        if buf is None or tuple(buf.shape) != shape or buf.device != self.dev:
            self._attn_buf = None          # (freed before the new one is allocated)
            buf = self._attn_buf = torch.empty(shape, dtype=torch.float32, device=self.dev)
        buf.zero_()                        # entries behind a step's position are never written
        self.attn_probs = buf
        x.attn_probs, x.attn_layer, x.attn_pos0, x.attn_steps, x.attn_rows = L.ptr(buf), int(layer), int(pos0), int(n_steps), self.batch
        d.ext_bytes = C.sizeof(L.DecoderExt4) - C.sizeof(L.Decoder)

    def attention_map(self, heads: str = "mean") -> torch.Tensor:
        """The map of the finished call from ``attn_probs`` (``vaura_attention_map``): (batch, n_steps, S - 1), the fixed-order mean over
        the heads, or with ``heads="all"`` (batch, n_head, n_steps, S - 1).  Row i is the step that samples sequence slot start + i; its
        weights stand in columns 0 .. start + i - 1, exact zeros behind them."""
        n_steps, B, H, max_len = self.attn_probs.shape
        W = self.S - 1
        out = torch.empty((B, H, n_steps, W) if heads == "all" else (B, n_steps, W), dtype=torch.float32, device=self.dev)
        L.check(self.lib.vaura_attention_map(L.ptr(self.attn_probs), L.ptr(out), n_steps, B, H, max_len, W, int(heads == "all"),
                                             L.current_stream(self.dev)), "vaura_attention_map")
        return out

    def _delays_arg(self):
        return L.delays_host(self.delays) if self.delays is not None else None

    # The pattern ops (ops.pattern_build_into / pattern_revert_into) and the sequence scores (_means) come in three forms each, and a
    # call without lengths must not take the lengths' entry point.  The choice is stated once per op, there and below.
    def _pattern_build(self):
        """``codes_i32`` -> ``seq``; with per-clip lengths a slot past a clip's own end holds the special token, as in the sequence
        built for T_b."""
        ops.pattern_build_into(self.codes_i32, self.seq, self.cfg.d_codebook, self.delays,
                               self.clip_T if self.lengths is not None else None, L.current_stream(self.dev))

    def _pattern_revert(self, buf: torch.Tensor, out: torch.Tensor, fill, pad) -> torch.Tensor:
        """Tokens (int32) or fp32 values in the layout of seq -> ``out`` (batch, K, T): ``fill`` where the sequence holds no frame, ``pad``
        in the frames past a clip's own end (per-clip lengths only)."""
        ops.pattern_revert_into(buf, out, fill, pad, self.delays, self.clip_T if self.lengths is not None else None,
                                L.current_stream(self.dev))
        return out

    def _means(self, buf: torch.Tensor, S: int, delays, T: int, t0: Optional[int]):
        """Fixed-order means of fp32 values ``buf`` (batch, K, S) in the pattern layout of ``delays`` (None: the default) over frames
        t0 .. T - 1 — T_b - 1 with per-clip lengths; t0 = None: from every clip's own prompt length P_b — -> (per codebook (batch, K),
        per clip (batch,))."""
        Bn, K = self.batch, self.cfg.num_codebooks
        f32 = dict(dtype=torch.float32, device=self.dev)
        pcb, score = torch.empty(Bn, K, **f32), torch.empty(Bn, **f32)
        a = (L.ptr(buf), S, L.delays_host(delays) if delays is not None else None, Bn, K, T)
        clip_T = L.ptr(self.clip_T) if self.lengths is not None else None
        o = (L.ptr(pcb), L.ptr(score), L.current_stream(self.dev))
        if t0 is None:
            L.check(self.lib.vaura_sequence_logprob_starts(*a, L.ptr(self.clip_P), clip_T, *o), "vaura_sequence_logprob_starts")
        elif self.lengths is not None:
            L.check(self.lib.vaura_sequence_logprob_clips(*a, t0, clip_T, *o), "vaura_sequence_logprob_clips")
        else:
            L.check(self.lib.vaura_sequence_logprob(*a, t0, *o), "vaura_sequence_logprob")
        return pcb, score

    def start_sequence(self, prompt: Optional[torch.Tensor]):
        """codes = -1 everywhere but the prompt -> pattern sequence on device; returns Tp.  With per-clip prompt lengths
        (``_set_prompt_lengths``) clip b takes ``prompt[b, :, :P_b]`` and holds -1 behind it; Tp is then the shortest prompt."""
        T = self.T
        self.codes_i32.fill_(-1)
        Tp = 0
        if self.prompt_lengths is not None:
            Pm = prompt.shape[-1]
            real = torch.arange(Pm, device=self.dev)[None, None, :] < self.clip_P.to(torch.int64)[:, None, None]
            self.codes_i32[..., :Pm] = torch.where(real, prompt.to(self.dev, torch.int32), self.codes_i32[..., :Pm])
            Tp = min(self.prompt_lengths)
        elif prompt is not None and prompt.shape[-1] > 0:
            Tp = prompt.shape[-1]
            assert Tp < (min(self.lengths) if self.lengths else T), "gt audio prompt can not be longer than max_new_tokens"
            self.codes_i32[..., :Tp] = prompt.to(self.dev, torch.int32)
        self._pattern_build()
        self._reset_state()
        return Tp

    def run(self, n_prefill: int, n_steps: int, sp: L.Sampling, noise: Optional[torch.Tensor] = None,
            use_graph: bool = True, plan: Optional[list] = None):
        """Enqueue `n_prefill` teacher-forced positions and `n_steps` sampled ones (asynchronous).
        With `use_graph` one decode step is captured once into a hipGraph and replayed per step; HIP
        cannot capture on the legacy default stream, so the loop then runs on a private stream that is
        ordered after / before the caller's current stream.
        ``plan`` (per-clip prompt lengths, ``clip_params.prompt_schedule``; `n_prefill` / `n_steps` are then not read): its steps run
        through the same loop — one captured graph for all of them —, the first group's prefill is that loop's own, and every later
        group's pass is ``vaura_prefill_rows`` between two loops, on the plane storages; the tile storages need none (their prefill
        is the decode step without sampling, so the steps the rows were carried through already left the K / V of the scalar call)."""
        self.dec.noise = L.ptr(noise)
        self._noise_keepalive = noise
        calls = [("loop", n_prefill, n_steps)]
        if plan is not None:
            calls, first = [], 0
            for i, e in enumerate(plan):
                if e[0] == "steps":
                    calls.append(("loop", first, e[1]))
                    first = 0
                elif i == 0:
                    first = e[1]               # group 1: the existing prefill, with the loop's n_prefill
                elif self._prefill_positions:
                    calls.append(("rows", e[1]))
            if first:                          # (a plan without steps: cannot happen for P_b < T_b, kept whole anyway)
                calls.append(("loop", first, 0))
            n_steps = sum(c[2] for c in calls if c[0] == "loop")
        use_graph = bool(use_graph and n_steps > 0)
        with (off_null_stream(self.dev) if use_graph else contextlib.nullcontext()):
            st = L.current_stream(self.dev)
            if use_graph:
                # per-clip calls: the record POINTER and the canonical struct of _sampling() — "per-clip + row doubling", never the values
                key = (self._shape, L.ptr(noise), bytes(sp), int(self.dec.clip_sampling or 0), int(self.dec.logprobs or 0),
                       int(self.dec_ext.logprobs_cond or 0), int(self.dec_ext.logprobs_null or 0),
                       # per-clip lengths: the POINTERS (engine-owned arrays, rewritten per call) — other lengths replay the same graph
                       int(self.dec_ext2.clip_timesteps or 0), int(self.dec_ext2.clip_cond_tokens or 0),
                       # per-clip prompt lengths: the POINTER as well
                       int(self.dec_ext3.row_prompt_steps or 0),
                       # attention maps: the buffer, the layer and the first reported position (all 0 in a call without them)
                       int(self.dec_ext4.attn_probs or 0), int(self.dec_ext4.attn_layer), int(self.dec_ext4.attn_pos0),
                       int(self.dec_ext4.attn_steps))
                if self._graph_key != key:       # the captured step is tied to these buffers / parameters
                    self._free_graph()
                    handle = C.c_void_p()
                    L.check(self.lib.vaura_step_graph_build(C.byref(self.dec), C.byref(sp), st, C.byref(handle)),
                            "vaura_step_graph_build")
                    self._graph, self._graph_key = handle, key
            for c in calls:
                if c[0] == "rows":
                    L.check(self.lib.vaura_prefill_rows(C.byref(self.dec), c[1], c[1], st), "vaura_prefill_rows")
                else:
                    L.check(self.lib.vaura_generate_loop(C.byref(self.dec), C.byref(sp), c[1], c[2],
                                                         self._graph if (use_graph and c[2] > 0) else None, st), "vaura_generate_loop")

    def _free_graph(self):
        if getattr(self, "_graph", None):
            self.lib.vaura_step_graph_free(self._graph)
        self._graph, self._graph_key = None, None

    def __del__(self):
        try:
            self._free_graph()
        except Exception:
            pass

    @property
    def _twin_lossy(self) -> bool:
        if self._twin_lossy_cached is None:
            self._twin_lossy_cached = self.wdtype in ("fp8", "fp8h") or (
                self.wdtype == "h1" and self.requested_wdtype != "auto" and self._twin_sd is not None and
                not all(h1_lossless(self._twin_sd[k]) for k in streamed_matrices(self._twin_sd)))
        return self._twin_lossy_cached

    def _twin(self) -> "DecoderEngine":
        """The exact-fp32 engine of the SAME model: fp32 tiles of what this engine's storage holds (the state dict itself for the
        lossless storages; the dequantised matrices for fp8 / a forced single plane).  Built on first use: ~2.7 GB of weights."""
        if self._range_twin is None:
            sd = self._twin_sd
            if self._twin_lossy:
                from . import quant
                if self.wdtype in ("fp8", "fp8h"):
                    sd = quant.fp8_effective_state_dict(sd)
                else:
                    from .synth import is_streamed_weight
                    sd = {k: (h_effective_weight(v, 1) if is_streamed_weight(k) else v) for k, v in sd.items()}
            try:
                self._range_twin = DecoderEngine(self.cfg, sd, self.dev, wdtype="f32", range_fallback=False, near_tie="off")
            except torch.cuda.OutOfMemoryError as e:
                raise L.VauraHipError("the exact-fp32 twin engine (2.7 GB of fp32 tiles + its K/V cache) does not fit next to this engine: "
                                      f"{e}") from e
        return self._range_twin

    def _reset_state(self):
        """position / arrivals / step back to 0; state[3] carries a sequence id (reserved for in-launch hand-off epochs)."""
        self._fc = None                       # position 0 again: a cached forward() prefix no longer matches the K/V cache
        DecoderEngine._sequence_id = (DecoderEngine._sequence_id + 1) & 0x3FF      # 10 bits enter the hand-off epoch (csrc/common.h)
        self.state[:4].zero_()                               # tiny device fills: no host-device synchronisation
        self.state[3:4].fill_(DecoderEngine._sequence_id)    # state[4] (status bits) is sticky until check_status() reads it
        self.state[6:8].zero_()                              # near-tie count / first flagged step of THIS sequence

    def check_status(self):
        """Read AND clear the sticky device status word (one host-device synchronisation; ``VAURAModel.generate`` folds it into
        the reference's own post-condition checks, vaura_model.py:550-572) and raise ONE error naming every condition it holds:
        a non-finite logit at the sampler (what an activation beyond the fp16-plane range turns into — the tokens decoded after it
        are garbage), and / or a hand-off of the one-launch MLP that gave up (every later hand-off then returns at once: wrong
        tokens AND an optimistic time).  ``generate_codes`` / ``run`` are asynchronous and do NOT call this: whoever drives them
        directly (bench.py, tools/, tests) must call it after synchronising — ``VAURAModel.generate_tokens``, ``forward_cached`` and
        ``logits_all_positions`` do."""
        words = self.state.tolist()                       # ONE transfer: status word + the near-tie counters
        st = int(words[4]) | self._carried_status
        self._carried_status = 0
        if st:
            self.state[4:5].zero_()
        self.last_near_ties = (0, None)
        if st & 4:                                        # informational (csrc/step.hip near-tie detector): never an error
            self.last_near_ties = (int(words[6]), int(words[7]) - 1 if words[7] else None)
            self.near_ties += int(words[6])
            self.state[6:8].zero_()
            st &= ~4
        err = self._status_error(st)
        if err is not None:
            raise err

    @staticmethod
    def _status_error(st: int) -> Optional["L.VauraHipError"]:
        """The error of a status word whose bits 1 / 2 are set (None otherwise): ONE error naming every condition, carrying ``.status``."""
        msgs = []
        if st & 2:
            msgs.append(
                "a consumer of the one-launch MLP gave up waiting for its producers (csrc/mlp_engine.h: its 256 workgroups must all become "
                "resident — is another process, or a second DecoderEngine of this process on another stream, running the same kernels on "
                "this GPU?); every hand-off after the give-up returned without waiting, so the tokens of this call are not valid and its "
                "timing is meaningless.  DecoderEngine(..., one_launch_mlp=False) keeps the two-launch path")
        if st & 1:
            msgs.append(
                "non-finite logits reached the sampler — an activation left even the pre-scaled fp16-plane range, or the checkpoint holds "
                "non-finite weights; weight_dtype='f32' keeps fp32 activations (exact-fp32-MFMA path)")
        if msgs:
            err = L.VauraHipError(f"decode loop (status word {st:#x}): " + "; ALSO: ".join(msgs))
            err.status = st
            return err
        return None

    def revert(self) -> torch.Tensor:
        return self._pattern_revert(self.seq, self.codes_i32, -1, self.cfg.d_codebook)      # frames past a clip's own end: the special id

    @torch.no_grad()
    def generate_codes(self, feats: torch.Tensor, max_new_tokens, *, prompt: Optional[torch.Tensor] = None,
                       use_sampling=False, temp=1.0, top_k=0, top_p=0.0, cfg_scale=1.0, noise=None, seed=0,
                       clip_base=0, use_graph=True, tokens_per_frame=7, delays=None, return_logprobs=False, num_candidates=1,
                       return_relevance=False, video_lengths=None, prompt_lengths=None, return_attention_weights=False,
                       attention_layer=-1, attention_heads="mean"):
        """The hot loop of generate(): (B, Tv, 768) -> codes (B, K, T) int64 (device).  ``delays``: the codebook delay pattern
        (codebook_patterns.py:374-419; None = 0..K-1, ParallelPatternProvider = all zeros): S = T + max(d) + 1 sequence steps, the
        loop samples steps Tp + 1 + d_0 .. S - 1, and an explicit ``noise`` has S - (Tp + 1 + d_0) steps.
        ``use_sampling``, ``temp``, ``top_k``, ``top_p``, ``cfg_scale``: a scalar, or one value per clip (list / tuple / 1-D tensor of
        length B) — clip b is then decoded exactly as the scalar call with its values would decode it (``_sampling``).
        ``num_candidates`` = N > 1: N candidates per clip in one call, exactly the batch ``feats.repeat_interleave(N, 0)`` (candidate j
        of clip b is row b * N + j; per-clip values and the prompt are repeated per candidate; Philox noise is keyed by clip_base + row;
        an explicit ``noise`` has B * N * K rows) — but the condition MLP runs on the B distinct clips (``set_condition``).  Returns
        codes (B * N, K, T).
        ``return_logprobs``: returns ``(codes, {"logprobs": (B * N, K, T) fp32, "per_codebook": (B * N, K), "score": (B * N,)})`` — the
        log-probability of every sampled token under the distribution its decision was made from (include/vaura_hip.h
        ``vaura_decoder.logprobs``; prompt frames hold 0), its mean over the generated frames per codebook, and the mean of those over
        the codebooks (``vaura_sequence_logprob``: fixed order, a NaN anywhere makes the clip's scores NaN).  The tokens are the ones
        the call returns without it.
        ``return_relevance``: the dict (returned as with ``return_logprobs``; both flags give one dict) gains the video relevance of
        every sampled token, r = log p(token | prefix, video) - log p(token | prefix, null video), both at temperature 1 over the full
        vocabulary (include/vaura_hip.h ``vaura_decoder_ext.logprobs_cond``): "logprob_cond", "logprob_null", "relevance" (B * N, K, T)
        (0 in prompt frames), "relevance_per_codebook" (B * N, K) and "sequence_relevance" (B * N,), the fixed-order means of
        ``vaura_sequence_logprob`` applied to r.  It needs the null-condition rows: when no clip's ``cfg_scale`` exceeds 1 the engine
        prepares the doubled batch anyway and draws every clip un-mixed through the per-clip records (its own scale, <= 1) — the tokens
        are those of the call without the flag, but such a call streams TWICE the rows through the decode step.
        ``max_new_tokens``: an int, or one int per clip (list / tuple / 1-D integer tensor of length B) T_b >= 1 — the call runs to T_max =
        max T_b and returns codes (B * N, K, T_max), clip b padded with the special id from frame T_b on; ``video_lengths``: None, or
        one int per clip, 1 <= Tv_b <= Tv, the leading video tokens of clip b's features that are real (later positions take
        ``empty_video_emb``; what lies in ``feats[b, Tv_b:]`` does not matter).  With Philox noise or greedy decoding clip b's frames
        [0, T_b) — tokens, log-probabilities, relevance, and their means — are the bits of the scalar call at the same batch with
        ``max_new_tokens=T_b`` (and ``feats[:, :Tv_b]``).  A common prompt must be shorter than every T_b.  An explicit ``noise`` is
        consumed per step of the call, so such a call works but is not comparable with a stand-alone one.
        ``prompt_lengths``: None, or one int per clip, 0 <= P_b < T_b, on a ``prompt`` (B, K, P_max): only ``prompt[b, :, :P_b]`` is
        clip b's prompt (what lies behind it is never used).  With Philox noise or greedy decoding clip b's frames [0, T_b) — tokens,
        log-probabilities, relevance and their means — are the bits of the same call at the same batch with the common prompt
        ``prompt[..., :P_b]`` (no prompt for P_b = 0), on every storage.  The loop samples from the shortest prompt's end for the whole
        batch (one captured graph) and, on the plane storages, runs one prefill pass per further distinct length over positions
        [0, P_b + d_0) just before that group's first sampled step (``clip_params.prompt_schedule``): G distinct lengths cost one loop
        plus sum_g (P_g + d_0) prefill positions.  Lengths that are all equal are the scalar call with ``prompt[..., :P]``, on its path.
        An explicit ``noise`` starts at the shortest prompt's first step and is not comparable, as above.
        ``return_attention_weights``: the dict (one dict for all three flags) gains "attention": the self-attention weights of layer
        ``attention_layer`` (default -1: the last; negative as in Python) at every sampled step, fp32 (B, S - start, S - 1) — the mean over
        the 16 heads, added in index order in fp32 and multiplied once by 1/16 — or with ``attention_heads="all"`` (B, 16, S - start,
        S - 1).  Row i is the step that samples sequence slot start + i (cache position start + i - 1): columns 0 .. start + i - 1 hold
        softmax_j(q . k_j / sqrt(96)) over the keys as the cache stores them — the numbers the kernel's output is formed from
        (include/vaura_hip.h ``vaura_decoder_ext4``) —, everything to the right is exactly 0.  Position p carries video token p // 7, so
        the map over positions is also the map over video time.  The conditional rows are reported (never the null-condition rows), the
        tokens and every other reported value are those of the call without the flag.  It costs one fp32 buffer of (S - start, B, 16,
        max_len) per call — 30 MB at 8 clips x 228 steps — and a store per weight in one layer's attention launch.  Served for caches of
        at most 256 positions, ``num_candidates`` = 1 and one length / prompt length per call (``VauraHipError`` otherwise, before any
        device work)."""
        B, Tv, _ = feats.shape
        call = clip_params.resolve_codes_call(
            B, Tv, max_new_tokens, None if prompt is None else int(prompt.shape[-1]), use_sampling=use_sampling, temp=temp, top_k=top_k,
            top_p=top_p, cfg_scale=cfg_scale, seed=seed, clip_base=clip_base, use_graph=use_graph, tokens_per_frame=tokens_per_frame,
            delays=delays, return_logprobs=return_logprobs, num_candidates=num_candidates, return_relevance=return_relevance,
            video_lengths=video_lengths, prompt_lengths=prompt_lengths, return_attention_weights=return_attention_weights,
            attention_layer=attention_layer, attention_heads=attention_heads)
        self._check_attention(call)
        with off_null_stream(self.dev) as caller:
            Tp, start, plan, sp, noise = self._begin_sequence(call, feats, prompt, noise)
            self.run(start - 1, self.S - start, sp, noise, call.use_graph, plan)
            return self._finish_sequence(call, Tp, caller)

    def _check_attention(self, call: clip_params.CodesCall) -> Optional[int]:
        """What only the engine knows about a call that asks for attention maps, before any device work -> the reporting layer as an
        index (None: the call asks for none)."""
        if not call.want_attention:
            return None
        K = self.cfg.num_codebooks
        S = call.t_max + (K if call.delays is None else max(call.delays) + 1)
        clip_params.check_attention_shape(S, self.cfg.block_size)
        return clip_params.check_attention_keywords(call.attention_layer, call.attention_heads, self.cfg.num_layers)

    def _begin_sequence(self, call: clip_params.CodesCall, feats, prompt, noise):
        """Everything of a ``generate_codes`` call in front of its loop, on the resolved call, enqueued on the current stream: the
        prepared shape, the per-clip arrays, the condition, the pattern sequence, the sampling struct, and the log-probability /
        relevance buffers -> (Tp, first sampled step, prompt plan or None, vaura_sampling, noise on the device or None)."""
        N, K = call.num_candidates, self.cfg.num_codebooks
        prompt = prompt[..., :call.prompt_frames] if call.prompt_frames else None
        if prompt is not None and N > 1:
            prompt = prompt.repeat_interleave(N, dim=0)
        self.prepare(call.batch * N, call.t_max, call.n_video_tokens, call.cfg_on, call.tokens_per_frame, self.cfg.block_size, call.delays)
        self._set_lengths(call.lengths, call.tv_lengths)
        self._set_prompt_lengths(call.P)
        self.set_condition(feats, replicate=N)
        Tp = self.start_sequence(prompt)       # per-clip prompt lengths: the shortest — where the loop starts sampling
        start = Tp + 1 + (self.delays[0] if self.delays else 0)  # Pattern.get_first_step_with_timesteps(Tp), sorted delays
        plan = None if call.P is None else clip_params.prompt_schedule(call.P, self.delays[0] if self.delays else 0, self.S,
                                                                       self.rows == 2 * self.batch)
        sp = self._sampling(call.use_sampling, call.temp, call.top_k, call.top_p, call.cfg_scale, call.seed, call.clip_base)
        if noise is not None:
            noise = noise.to(self.dev, torch.float32).contiguous()
            assert noise.shape == (self.S - start, call.batch * N * K, self.cfg.d_codebook), noise.shape
        if call.want_logprobs:
            self.logprobs.zero_()         # slots the sampler does not fill (prompt, special) read 0
        self.dec.logprobs = L.ptr(self.logprobs) if call.want_logprobs else 0
        if call.want_relevance:
            if self.logprobs_cond is None:
                self.logprobs_cond, self.logprobs_null = torch.zeros_like(self.logprobs), torch.zeros_like(self.logprobs)
            else:
                self.logprobs_cond.zero_()
                self.logprobs_null.zero_()
        self.dec_ext.logprobs_cond = L.ptr(self.logprobs_cond) if call.want_relevance else 0
        self.dec_ext.logprobs_null = L.ptr(self.logprobs_null) if call.want_relevance else 0
        # attention maps: the step that samples slot start + i runs at cache position start + i - 1
        self._set_attention(self._check_attention(call), start - 1, self.S - start)
        return Tp, start, plan, sp, noise

    def _finish_sequence(self, call: clip_params.CodesCall, Tp: int, caller):
        """The end of a call whose loop is enqueued, on the current stream: the revert, the log-probabilities and the relevance that
        were asked for, all handed to the ``caller`` stream (``off_null_stream``) -> what ``generate_codes`` returns."""
        out = self.revert().to(torch.int64)
        extra = self._sequence_logprobs(Tp) if call.want_logprobs else None
        if call.want_relevance:
            extra = dict(extra or {}, **self._sequence_relevance(Tp))
        if call.want_attention:
            extra = dict(extra or {}, attention=self.attention_map(call.attention_heads))
        if caller is not None:
            out.record_stream(caller)
            for t in (extra or {}).values():
                t.record_stream(caller)
        return (out, extra) if (call.want_logprobs or call.want_relevance or call.want_attention) else out

    def _revert_f32(self, buf: torch.Tensor) -> torch.Tensor:
        """fp32 values in the layout of seq -> (batch, K, T), 0 where the sequence holds no frame."""
        out = torch.empty(self.batch, self.cfg.num_codebooks, self.T, dtype=torch.float32, device=self.dev)
        return self._pattern_revert(buf, out, 0.0, 0.0)

    def _sequence_means(self, buf: torch.Tensor, Tp: int):
        """Fixed-order means of values in the layout of seq over frames Tp .. T - 1 -> (per codebook (batch, K), per clip (batch,))."""
        # with per-clip prompt lengths: every clip's means over its own frames P_b .. T_b - 1
        return self._means(buf, self.S, self.delays, self.T, None if self.prompt_lengths is not None else Tp)

    def _sequence_logprobs(self, Tp: int) -> Dict[str, torch.Tensor]:
        """The finished call's log-probabilities, reverted to (batch, K, T), and their fixed-order means over frames Tp .. T - 1."""
        pcb, score = self._sequence_means(self.logprobs, Tp)
        return {"logprobs": self._revert_f32(self.logprobs), "per_codebook": pcb, "score": score}

    def _sequence_relevance(self, Tp: int) -> Dict[str, torch.Tensor]:
        """The finished call's relevance r = lc - lu (one fp32 subtraction per slot, in the layout of seq: 0 - 0 where nothing was
        sampled), the three reverted to (batch, K, T), and the fixed-order means of r (the log-probability's reduction kernel)."""
        r = self.logprobs_cond - self.logprobs_null
        pcb, score = self._sequence_means(r, Tp)
        return {"relevance": self._revert_f32(r), "logprob_cond": self._revert_f32(self.logprobs_cond),
                "logprob_null": self._revert_f32(self.logprobs_null), "relevance_per_codebook": pcb, "sequence_relevance": score}

    @torch.no_grad()
    def generate_codes_checked(self, feats: torch.Tensor, max_new_tokens: int, **kw):
        """``generate_codes`` + ``check_status`` (ONE host-device synchronisation) with range safety BY CONSTRUCTION: when — and only
        when — the status word reports non-finite logits (an activation left the fp16-plane range somewhere in the loop: every such
        overflow arrives at the sampler as NaN), the whole call is run again on the exact-fp32 twin engine
        (weight_dtype="f32": fp32 activations between kernels, the reference's own arithmetic and range), with the same condition,
        prompt, sampling parameters and noise (an explicit tensor, or Philox keyed by (seed, clip, codebook, step) — not by the engine), so
        the result is what the fp32 path would have produced from the start.  A checkpoint with massive activations therefore decodes
        correctly (at the f32 engine's speed) instead of raising.  Counted in ``range_fallbacks``.  The other status bit — a hand-off of
        the one-launch MLP that gave up because the GPU is shared — switches this engine to the separate launches and re-runs the
        call as well (``handoff_fallbacks``): a slower run, not an error.  Anything else still raises."""
        codes = self.generate_codes(feats, max_new_tokens, **kw)
        try:
            self.check_status()
        except L.VauraHipError as e:
            eng = self._status_fallback(getattr(e, "status", 0), e)
            return self.generate_codes_checked(feats, max_new_tokens, **kw) if eng is self else self._on_twin(feats, max_new_tokens, kw)
        if self.near_tie == "rerun" and self.last_near_ties[0] > 0 and self.wdtype != "f32" and self._twin_sd is not None:
            # >= 1 used decision of this call was inside the plane arithmetic's noise: the same call on the exact-fp32 twin, same noise
            self.near_tie_reruns += 1
            codes = self._on_twin(feats, max_new_tokens, kw)
        return codes

    def _on_twin(self, feats, max_new_tokens, kw):
        codes = self._twin().generate_codes(feats, max_new_tokens, **kw)
        self._range_twin.check_status()
        return codes

    def _status_fallback(self, st: int, err) -> "DecoderEngine":
        """What a call whose status word ``st`` gave the error ``err`` is run on again: this engine, switched to the separate launches
        (``handoff_fallbacks``), or the exact-fp32 twin (``range_fallbacks``).  Where neither helps, ``err`` is raised."""
        import warnings
        if (st & 2) and self.one_launch_mlp:
            # A consumer of the one-launch MLP gave up waiting: its 256 workgroups were not all resident — the GPU is shared
            # (another process / tenant, a CU mask, a second engine on another stream).  Not an error of the model: switch THIS
            # engine to the separate launches for good (no in-launch hand-off, nothing to starve; same bits) and run the call again.
            warnings.warn("vaura_amd: the one-launch MLP's in-launch hand-off timed out (GPU shared?); this engine now uses the "
                          "separate launches (slower by 5-7 %, same results)")
            self.one_launch_mlp = False
            self.handoff_fallbacks += 1
            if self.dec is not None:
                self.dec.ws_sync = 0
            self._free_graph()
            return self
        if st != 1 or self.wdtype == "f32" or self._twin_sd is None:       # nothing wider to fall back to
            raise err
        if self.range_fallbacks == 0:
            warnings.warn("vaura_amd: an activation left the fp16-plane range (non-finite logits at the sampler); this call is re-run "
                          "on the exact-fp32 twin engine (1.5 x slower, ~2.7 GB more)"
                          + (" — built from the DEQUANTISED matrices this lossy storage holds" if self._twin_lossy else "")
                          + ".  A checkpoint that does this on every call wants plane_shift=4..8 or weight_dtype='f32'")
        self.range_fallbacks += 1
        return self._twin()

    # ------------------------------------------------------------------ the loop in pieces: frames leave while it still runs
    def generate_codes_stream(self, feats: torch.Tensor, max_new_tokens, *, block_frames: int = 16, halo: int = 0, **kw):
        """``generate_codes`` as a generator that says which frames are final while the loop is still running.  The arguments are checked
        here, at call time; the returned generator runs the call.  ``kw``: the keywords of ``generate_codes``.
        The S - start sampled steps run in pieces (``clip_params.stream_schedule``): a piece ends where ``block_frames`` more frames of
        the longest clip have become RELEASABLE — final in every codebook (frame t of codebook q is written at step t + 1 + d_q and never
        changes afterwards) and at least ``halo`` frames in front of the last final one (the codec's ``decode_halo``: the samples of a
        frame depend on that many frames either side; 0 for a caller that wants tokens only); a complete clip releases everything.  The
        captured single step is the one ``generate_codes`` replays, and the position lives in the device state word, so the tokens are
        its tokens whatever the piece lengths (they need not be multiples of the loop's graph grouping).
        Each ``next()`` yields [(lo_b, hi_b) per clip]: the frames of ``self.seq`` (and of ``self.logprobs`` / ``logprobs_cond`` /
        ``logprobs_null`` when asked for — ``stream_frames`` reads them) that became releasable; the generator's return value
        (``StopIteration.value``) is what ``generate_codes`` returns.  At most two pieces are in flight: piece k + 1 is enqueued
        before the host waits for the event behind piece k, so the device does not idle on the host; whatever the consumer enqueues for
        block k (a codec window) therefore runs behind piece k + 1 on the stream.  Closing the generator early leaves at most those two
        pieces running; the engine is reusable at once (the next call is ordered behind them on the stream).
        Status word: behind every piece the state words are copied to pinned host memory in front of the piece's event — no extra
        stall.  Bit 1 (non-finite logits) or 2 (a hand-off gave up) BEFORE anything was yielded: what ``generate_codes_checked`` does —
        the separate launches, or the exact-fp32 twin, with the same noise — and the stream continues from there.  AFTER a block has
        gone out the audio cannot be taken back: ``VauraHipError`` with ``.status`` and ``.frames_emitted`` (per clip).
        Refused here, before the engine is touched: ``num_candidates`` > 1 (the winner is known only at the end), more than one distinct
        ``prompt_lengths`` value (that path interleaves prefill passes with the loop; not served by this version), ``near_tie="rerun"``
        (it decides at the end of the call), and a ``block_frames`` that is no positive int."""
        B, Tv, _ = feats.shape
        prompt, noise = kw.pop("prompt", None), kw.pop("noise", None)
        call = clip_params.resolve_codes_call(B, Tv, max_new_tokens, None if prompt is None else int(prompt.shape[-1]), **kw)
        clip_params.check_block_frames(block_frames)
        clip_params.refuse_attention("generate_codes_stream", call.want_attention)
        if call.num_candidates != 1:
            raise L.VauraHipError("streaming takes num_candidates = 1: the winning candidate is known only at the end of the call")
        if self.near_tie == "rerun":
            raise L.VauraHipError('streaming is refused on an engine with near_tie="rerun": the re-run is decided at the end of the call, '
                                  'after audio has left (use "report" or "off")')
        if isinstance(halo, bool) or not isinstance(halo, int) or halo < 0:
            raise L.VauraHipError(f"halo must be a non-negative number of frames, got {halo!r}")
        if call.P is not None:
            raise L.VauraHipError(f"streaming takes one prompt length for the call, got prompt_lengths {call.P}: distinct lengths interleave "
                                  "prefill passes with the loop and are not served by this version")
        if call.prompt_frames >= (min(call.lengths) if call.lengths else call.t_max):
            raise L.VauraHipError(f"the audio prompt ({call.prompt_frames} frames) must be shorter than max_new_tokens "
                                  f"({call.lengths or call.t_max})")
        return self._codes_stream(call, feats, prompt, noise, int(block_frames), int(halo))

    def _stream_status(self, words: torch.Tensor) -> int:
        """Bits 1 | 2 of the state words a piece left in pinned memory (its event has been waited for), with what ``prepare`` carried over."""
        return (int(words[4]) | self._carried_status) & 3

    def stream_frames(self, buf: torch.Tensor, ranges, fill) -> torch.Tensor:
        """The frames [lo_b, hi_b) of every clip out of ``buf`` in the layout of seq (tokens, or fp32 per-token values) -> (batch, K, max
        count), clip b's frames left-aligned with ``fill`` behind them: what the revert of the finished call holds there, bit for bit
        (frame t of codebook q sits at step t + 1 + d_q), read while the loop may still be filling later steps."""
        K = self.cfg.num_codebooks
        n = max(hi - lo for lo, hi in ranges)
        d = torch.tensor(self.delays if self.delays is not None else list(range(K)), device=self.dev)
        lo = torch.tensor([r[0] for r in ranges], device=self.dev)
        cnt = torch.tensor([r[1] - r[0] for r in ranges], device=self.dev)
        t = torch.arange(n, device=self.dev)
        step = (lo[:, None, None] + 1 + d[None, :, None] + t[None, None, :]).clamp(max=self.S - 1)
        got = torch.gather(buf, 2, step)
        return torch.where(t[None, None, :] < cnt[:, None, None], got, torch.full_like(got, fill))

    def _pinned_words(self):
        """The state words of the two pieces in flight, on the host."""
        if getattr(self, "_stream_pinned", None) is None:
            self._stream_pinned = [torch.zeros(8, dtype=torch.int32).pin_memory() for _ in range(2)]
        return self._stream_pinned

    def enqueue_piece(self, slot: int, n_prefill: int, n_steps: int, sp: L.Sampling, noise, use_graph: bool = True) -> "torch.cuda.Event":
        """A bounded number of steps of a begun sequence (``_begin_sequence`` / ``begin_live``), on the current stream: ``n_prefill``
        teacher-forced positions and ``n_steps`` sampled ones from where the device state word stands, the state words copied to the
        pinned host buffer ``slot`` (0 | 1) behind them, and the returned event behind those.  Once the event has been waited for,
        ``_stream_status(self._pinned_words()[slot])`` is the status of everything up to the end of this piece."""
        self.run(n_prefill, n_steps, sp, noise, use_graph)
        self._pinned_words()[slot].copy_(self.state, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        return ev

    def stream_error(self, st: int, last_event) -> "L.VauraHipError":
        """The error of a dirty status ``st`` read off a piece: waits for ``last_event`` (nothing of the call is running any more) and
        clears the device word and what ``prepare`` carried, so that the engine is reusable whatever the caller does with the error."""
        last_event.synchronize()
        self.state[4:5].zero_()
        self._carried_status = 0
        return self._status_error(st)

    # ------------------------------------------------------------------ video in while the loop runs (live.LiveSession)
    def begin_live(self, call: clip_params.CodesCall, noise=None, owner=None):
        """``_begin_sequence`` for a call whose video has not arrived yet, on the current stream -> (first sampled step, vaura_sampling,
        noise on the device or None).  The whole condition buffer is then filled with NaN: a step that reads a token ahead of the
        video gives non-finite logits, which the status word reports, instead of a wrong sample.  ``append_condition`` brings the
        tokens in; on an engine with the null-condition rows the null embedding is projected here, once.  ``owner``: kept in
        ``live_owner`` until the next ``prepare`` — any other call on this engine —, so that a session can tell that its sequence is
        still the one in the buffers."""
        if call.tv_lengths is not None or call.lengths is not None or call.P is not None or call.num_candidates != 1 or call.prompt_frames:
            raise L.VauraHipError("a live sequence takes one length for the whole call, no prompt and num_candidates = 1")
        clip_params.refuse_attention("a live sequence", call.want_attention)
        c = self.cfg
        zeros = torch.zeros(call.batch, call.n_video_tokens, c.cond_in, dtype=torch.float32, device=self.dev)
        _, start, _, sp, noise = self._begin_sequence(call, zeros, None, noise)
        self._live_null = None
        if self.rows == 2 * self.batch:
            self._live_null = self._project_rows(self.uncond.reshape(self.Tv, c.cond_in), "null")
        self.cond_proj.fill_(float("nan"))
        self.live_owner = owner
        return start, sp, noise

    def _project_rows(self, x: torch.Tensor, name: str) -> torch.Tensor:
        """``vaura_prefill_cond`` on the rows of ``x`` (n, cond_in) -> compact packed rows (n x cond_dim), in buffers of this size kept
        under ``name``.  A projected row depends on nothing but its own input row: these are the bits ``set_condition`` gives it."""
        c, n = self.cfg, int(x.shape[0])
        bufs = getattr(self, "_live_bufs", None)
        if bufs is None:
            bufs = self._live_bufs = {}
        if (name, n) not in bufs:
            rp = self._rows_padded(n)
            bufs[(name, n)] = tuple(torch.zeros(rp * w, dtype=torch.float32, device=self.dev) for w in (c.cond_in, c.cond_dim, c.cond_dim))
        inp, tmp, out = bufs[(name, n)]
        x = x.to(self.dev, torch.float32).contiguous()
        st = L.current_stream(self.dev)
        L.check(self.lib.vaura_pack_rows(L.ptr(x), L.ptr(inp), n, c.cond_in, st), "vaura_pack_rows")
        L.check(self.lib.vaura_prefill_cond(C.byref(self.dims), L.ptr(inp), L.ptr(self.fc1), L.ptr(self.fc2), L.W_F32, L.ptr(tmp),
                                            L.ptr(out), n, st), "vaura_prefill_cond")
        self._cond_keepalive = x
        return out

    def append_condition(self, feats: torch.Tensor, first_token: int, shift_tokens: int = 0):
        """``feats`` (B, n, cond_in): n fresh video tokens of every clip into the prepared condition buffer IN PLACE (it is baked into
        the captured step graph), on the current stream.  The MLP runs on the B * n new rows only; ``vaura_cond_window`` then moves
        tokens [shift_tokens, Tv) of the conditional rows down by ``shift_tokens`` and writes the new ones at ``first_token``; the
        null-condition rows take the projected null embedding at the same positions (``begin_live`` computed it; computed here for an
        engine that ``set_condition`` filled).  ``shift_tokens`` = 0 appends; ``set_condition`` stays the way to set a whole window."""
        assert self.dec is not None
        self._fc = None
        B, n, Cin = feats.shape
        if B != self.batch or Cin != self.cfg.cond_in or n < 1:
            raise L.VauraHipError(f"append_condition: features must be ({self.batch}, n, {self.cfg.cond_in}), got {tuple(feats.shape)}")
        null = None
        if self.rows == 2 * self.batch:
            if getattr(self, "_live_null", None) is None:
                self._live_null = self._project_rows(self.uncond.reshape(self.Tv, self.cfg.cond_in), "null")
            null = self._live_null
        new = self._project_rows(feats.reshape(B * n, Cin), "new")
        L.check(self.lib.vaura_cond_window(C.byref(self.dec), L.ptr(new), L.ptr(null), int(shift_tokens), int(first_token), n,
                                           L.current_stream(self.dev)), "vaura_cond_window")

    def final_frames(self, steps_run: int, start: int) -> int:
        """Frames of the begun sequence that are final in every codebook after ``steps_run`` sampled steps (``clip_params.final_frames``):
        what ``stream_frames`` may read."""
        return clip_params.final_frames(steps_run, self.T, start, max(self.delays) if self.delays is not None else self.cfg.num_codebooks - 1)

    @torch.no_grad()
    def _codes_stream(self, call: clip_params.CodesCall, feats, prompt, noise, block_frames: int, halo: int):
        self.stream_engine = self              # whose seq / per-token buffers the yielded ranges refer to (the twin after a range fallback)
        pinned = self._pinned_words()
        with off_null_stream(self.dev):
            Tp, start, _, sp, dev_noise = self._begin_sequence(call, feats, prompt, noise)
            pieces = clip_params.stream_schedule(self.T, self.lengths, start, self.delays, halo, block_frames, self.cfg.num_codebooks)
            if self.lengths is None:           # one length: every clip of the batch has the one range
                pieces = [(n, r * self.batch) for n, r in pieces]
            assert sum(n for n, _ in pieces) == self.S - start
            events = []

            def enqueue(k):                    # piece k, its state words behind it, its event behind those
                events.append(self.enqueue_piece(k % 2, start - 1 if k == 0 else 0, pieces[k][0], sp, dev_noise, call.use_graph))
            enqueue(0)
        emitted = [0] * self.batch
        for k, (_, ranges) in enumerate(pieces):
            if k + 1 < len(pieces):
                with off_null_stream(self.dev):
                    enqueue(k + 1)
            events[k].synchronize()
            st = self._stream_status(pinned[k % 2])
            if st:
                err = self.stream_error(st, events[-1])
                if any(emitted):
                    err.frames_emitted = list(emitted)
                    err.args = (f"{err.args[0]} — after frames {emitted} of the clips had been streamed out: they cannot be taken back",)
                    raise err
                # before any frame has left: ``generate_codes_checked``'s two ways out, as a stream.  Whoever reads seq / the per-token
                # buffers of the running stream reads those of the engine it continues on
                self.stream_engine = self._status_fallback(st, err)
                return (yield from self.stream_engine._codes_stream(call, feats, prompt, noise, block_frames, halo))
            if any(hi > lo for lo, hi in ranges):
                yield list(ranges)
                emitted = [hi for _, hi in ranges]
        with off_null_stream(self.dev) as caller:
            result = self._finish_sequence(call, Tp, caller)
        self.check_status()                    # the near-tie counters of the call (informational); the loop's bits were read piece by piece
        return result

    # ------------------------------------------------------------------ the reference host's call pattern, with a cache
    def forward_cached(self, idx: torch.Tensor, feats: torch.Tensor, tokens_per_frame: int = 7) -> torch.Tensor:
        """``Transformer.forward`` as the REFERENCE host calls it — the whole prefix, every step ("no caching is implemented :(",
        models/vaura_model.py:504-506) — served incrementally: when ``idx[..., :n]`` and ``feats`` equal what the previous call
        fed (compared on the device), only positions n.. are run through the decode kernels and their logits are appended to a
        cache; the result is the (Bs, K, L, V) view the contract asks for.  A call that does not extend the cached prefix (new
        clip, other batch, changed condition) starts over.  The host's 228-call loop thus costs 228 decode steps, not 26 106.
        ``self.cached_forward_steps`` counts the decode steps actually run (tests)."""
        Bs, K, Lq = idx.shape
        c = self.cfg
        cap = c.block_size                                   # positions the model supports (scripts/generate.py:221-224)
        if Lq > cap:
            raise L.VauraHipError(f"sequence of {Lq} positions exceeds block_size {cap}")
        if self._forward_on_twin:         # an earlier call overflowed the fp16 planes: this engine's forward() stays on fp32
            return self._range_twin.forward_cached(idx, feats, tokens_per_frame)
        idx = idx.to(self.dev)
        feats = feats.to(self.dev, torch.float32)
        st = getattr(self, "_fc", None)
        n0 = 0
        if (st is not None and st["key"] == (Bs, K, feats.shape[1], tokens_per_frame) and self._shape == st["shape"]
                and st["n"] < Lq and torch.equal(st["feats"], feats) and torch.equal(st["idx"][:, :, :st["n"]], idx[:, :, :st["n"]])):
            n0 = st["n"]
        else:
            self.prepare(Bs, cap - K, feats.shape[1], False, tokens_per_frame, block_size=cap)    # S = cap positions, K/V capacity = cap
            self._set_lengths(None, None)
            self.set_condition(feats)
            self.seq.zero_()
            self._reset_state()
            st = self._fc = {"key": (Bs, K, feats.shape[1], tokens_per_frame), "shape": self._shape, "feats": feats.clone(),
                             "idx": torch.zeros(Bs, K, cap, dtype=idx.dtype, device=self.dev), "n": 0,
                             "logits": torch.empty(Bs, K, cap, c.d_codebook, dtype=torch.float32, device=self.dev)}
        sp = self._sampling(False, 1.0, 0, 0.0, 1.0, 0, 0)
        stream = L.current_stream(self.dev)
        for p in range(n0, Lq):
            self.seq[:, :, p] = idx[:, :, p].to(torch.int32)       # teacher-forced input of position p (state[0] == p)
            L.check(self.lib.vaura_decode_step(C.byref(self.dec), C.byref(sp), 1, stream), "vaura_decode_step")
            st["logits"][:, :, p] = self.ws_logits.view(Bs, K, -1)
            self.cached_forward_steps = getattr(self, "cached_forward_steps", 0) + 1
        try:
            self.check_status()              # the caller consumes these logits on the host side anyway (one synchronisation)
            st["idx"][:, :, n0:Lq] = idx[:, :, n0:Lq]       # committed only once the status word is clean: a caller that
            st["n"] = Lq                                     # catches the error and goes on must not be served the invalid prefix
        except L.VauraHipError as e:
            self._fc = None
            # range safety for the reference host's call pattern too (see generate_codes_checked): non-finite logits = an activation left
            # the fp16-plane range -> this and every later forward() of the engine runs on the exact-fp32 twin (whole prefix recomputed once)
            if getattr(e, "status", 0) != 1 or self.wdtype == "f32" or self._twin_sd is None:
                raise
            self.range_fallbacks += 1
            self._forward_on_twin = True
            return self._twin().forward_cached(idx, feats, tokens_per_frame)
        return st["logits"][:, :, :Lq].clone()      # a copy: the cache must survive in-place edits by the caller

    # ------------------------------------------------------------------ op-level access (tests)
    def logits_all_positions(self, idx: torch.Tensor, feats: torch.Tensor, tokens_per_frame: int = 7) -> torch.Tensor:
        """Teacher-forced pass: idx (Bs, K, Lq) int64, feats (Bs, Tv, 768) -> logits (Bs, K, Lq, V).
        One decode step per position, heads evaluated every step (API-compat path of
        ``Transformer.forward``; the generate loop never materialises this tensor)."""
        Bs, K, Lq = idx.shape
        self._fc = None
        self.prepare(Bs, Lq, feats.shape[1], False, tokens_per_frame, block_size=self.cfg.block_size)
        self._set_lengths(None, None)
        self.set_condition(feats)
        self.seq.zero_()
        self.seq[:, :, :Lq] = idx.to(self.dev, torch.int32)
        self._reset_state()
        out = torch.empty(Bs, K, Lq, self.cfg.d_codebook, dtype=torch.float32, device=self.dev)
        sp = self._sampling(False, 1.0, 0, 0.0, 1.0, 0, 0)
        st = L.current_stream(self.dev)
        keep = self.seq.clone()
        for p in range(Lq):
            L.check(self.lib.vaura_decode_step(C.byref(self.dec), C.byref(sp), 1, st), "vaura_decode_step")
            out[:, :, p] = self.ws_logits.view(Bs, K, -1)
            self.seq.copy_(keep)  # the sampler only fills -1 slots, but keep the input pristine anyway
        self.check_status()
        return out

    # ------------------------------------------------------------------ teacher-forced scoring (VAURAModel.forward + _compute_loss)
    def _score_workspace(self) -> torch.Tensor:
        """(prefill_positions * rows_padded, K * vocab) fp32: the heads' output over one prefill chunk (vaura_score).  Allocated on
        first use and kept while the prepared shape stays (``_shape`` keys it), so the decode loop's memory is unchanged."""
        key = (self._shape, self._prefill_positions)
        if getattr(self, "_score_ws_key", None) != key:
            self._score_ws = None
            n = self._prefill_positions * self._rows_padded(self.rows) if self._prefill_positions else 0
            self._score_ws = (torch.empty(n, self.cfg.num_codebooks * self.cfg.d_codebook, dtype=torch.float32, device=self.dev)
                              if n else None)
            self._score_ws_key = key
        return self._score_ws

    @torch.no_grad()
    def score(self, codes: torch.Tensor, feats: torch.Tensor, *, delays: Optional[Sequence[int]] = None, tokens_per_frame: int = 7,
              return_logits: bool = False, checked: bool = True, relevance: bool = False, video_lengths=None) -> Dict[str, torch.Tensor]:
        """Teacher-forced cross-entropy of ``codes`` (B, K, Ta) under ``feats`` (B, Tv, 768): the reference's ``forward`` +
        ``_compute_loss`` (vaura_model.py:136-192, 240-280).  The input is ``build_pattern_sequence(codes[..., :-1])`` against a pattern
        of Ta timesteps (special token = vocab), S = Ta + max(d) + 1 (``delays`` None = 0..K-1); positions [0, S - 1) run without a CFG
        branch (rows = B) through the prefill chunks with the heads at every position (plane storages; one decode step with heads per
        position on "f32"), then the fused revert + log-softmax + NLL kernel and the fixed-order per-codebook mean (csrc/score.hip).
        Returns {"loss": (), "loss_per_codebook": (K,), "nll": (B, K, Ta), "mask": (B, K, Ta) bool, and with ``return_logits`` "logits":
        the reverted (B, K, Ta, vocab)}.  ``checked``: range safety as ``generate_codes_checked`` — a non-finite loss or a dirty status
        word re-runs the call on the exact-fp32 twin (one warning per engine).
        ``relevance``: the codes are prefilled under the video AND under the null condition (rows [B, 2B), the layout CFG uses: twice
        the rows in one pass), the NLL kernel and the reduction run on both row sets (``vaura_score_relevance``), and the result gains
        "nll_null" (B, K, Ta), "loss_null" / "loss_null_per_codebook", "nll_per_codebook" and "nll_null_per_codebook" (B, K) — the mean
        over the timesteps per clip and codebook, in the fixed order of ``vaura_sequence_logprob`` —, "relevance_per_codebook" (B, K)
        = nll_null_per_codebook - nll_per_codebook (how many nats per token the video explains) and "relevance" (B,), its mean over
        the codebooks.  Today's entries are the bits of the call without the flag.
        One length per call: a list of code tensors, or ``video_lengths``, is refused (``score_clips`` serves them)."""
        c = self.cfg
        if not torch.is_tensor(codes) or video_lengths is not None:      # one length per call here (a projected video row depends on its own input row only: pad the features)
            raise L.VauraHipError("score() takes one length for the whole call — one (B, K, Ta) tensor of codes, no video_lengths: per-clip "
                                  "lengths are served by score_clips() (and by generate() / generate_tokens())")
        return self._score(codes, feats, None, None, delays, tokens_per_frame, return_logits, checked, relevance, False)

    @torch.no_grad()
    def score_clips(self, codes, feats: torch.Tensor, lengths=None, *, video_lengths=None, delays: Optional[Sequence[int]] = None,
                    tokens_per_frame: int = 7, return_logits: bool = False, checked: bool = True,
                    relevance: bool = False) -> Dict[str, torch.Tensor]:
        """``score`` for clips of different lengths in ONE call: clip b is scored over its own ``Ta_b`` timesteps and its own ``Tv_b``
        video tokens, as ``score(codes[b:b + 1, :, :Ta_b], feats[b:b + 1, :Tv_b])`` scores it — attention is causal, so nothing behind a
        clip's end reaches a position before it: exact, not an approximation.
        ``codes``: a (B, K, Ta) tensor with ``lengths`` one int per clip, 2 <= Ta_b <= Ta (None: every clip has Ta), or a list of B
        tensors (K, Ta_b) / (1, K, Ta_b), padded here (``lengths`` then comes from the shapes).  What ``codes`` holds from timestep Ta_b
        on never matters (it is not range-checked either).  ``video_lengths``: as in ``generate_codes`` — positions whose frame is >=
        Tv_b take ``empty_video_emb``; ``feats[b, Tv_b:]`` does not matter.
        Clip b's input is ``build_pattern_sequence(codes_b[..., :Ta_b - 1])`` against a pattern of Ta_b timesteps
        (``vaura_pattern_build_clips``), the call runs the S_max - 1 positions of the longest clip, and the scoring kernels take Ta_b
        (csrc/score.hip ``score_nll_clips_kernel`` / ``score_reduce_clips_kernel``; a finished clip's rows are computed and ignored).
        Returns what ``score`` returns — "loss_per_codebook"[q] the mean over ALL valid (b, t), the reference's ``_compute_loss`` under
        the mask t < Ta_b, "loss" the mean of those; "nll" / "logits" NaN and "mask" False behind each clip's end — plus "lengths" (B,)
        int32, "nll_per_codebook" (B, K): the mean of clip b's codebook q over t < Ta_b, and "loss_per_clip" (B,): its mean over the
        codebooks, the loss clip b gets scored alone (``vaura_sequence_logprob_clips``: fixed order, two calls give the same bits).
        ``relevance``: the null-condition twins of ``score`` and "relevance_per_codebook" / "relevance", all over clip b's own frames.
        Everything wrong with the lengths is refused before any device work (``clip_params.resolve_score_lengths``)."""
        c = self.cfg
        K = c.num_codebooks
        if torch.is_tensor(codes):
            if codes.dim() != 3 or codes.shape[1] != K:
                raise L.VauraHipError(f"codes must be (B, {K}, Ta), got {tuple(codes.shape)}")
            B, Ta = int(codes.shape[0]), int(codes.shape[2])
        else:
            shapes = clip_params.score_list_lengths(codes, K)
            if lengths is not None and clip_params._int_list("lengths", lengths) != shapes:
                raise L.VauraHipError(f"lengths {list(lengths)} given next to a list of codes whose shapes say {shapes}")
            lengths, B, Ta = shapes, len(shapes), max(shapes)
        if feats.dim() != 3 or feats.shape[0] != B or feats.shape[2] != c.cond_in:
            raise L.VauraHipError(f"feats must be ({B}, Tv, {c.cond_in}), got {tuple(feats.shape)}")
        lens, tv = clip_params.resolve_score_lengths(B, Ta, lengths, video_lengths, int(feats.shape[1]))
        if not torch.is_tensor(codes):         # pad with a valid id: never read as a target, never fed (the special token stands there)
            padded = torch.zeros(B, K, Ta, dtype=torch.int64, device=self.dev)
            for b, cb in enumerate(codes):
                padded[b, :, :lens[b]] = cb.reshape(K, -1).to(self.dev)
            codes = padded
        return self._score(codes, feats, lens, tv, delays, tokens_per_frame, return_logits, checked, relevance, True)

    def _score(self, codes, feats, lengths, video_lengths, delays, tokens_per_frame, return_logits, checked, relevance, per_clip):
        """``score`` (lengths and video_lengths None, per_clip False: the launches and the bits it always had) and ``score_clips``
        (checked lists of per-clip lengths or None; per_clip: the per-clip entries of the result)."""
        c = self.cfg
        if codes.dim() != 3 or codes.shape[1] != c.num_codebooks:
            raise L.VauraHipError(f"codes must be (B, {c.num_codebooks}, Ta), got {tuple(codes.shape)}")
        B, K, Ta = codes.shape
        if feats.dim() != 3 or feats.shape[0] != B or feats.shape[2] != c.cond_in:
            raise L.VauraHipError(f"feats must be ({B}, Tv, {c.cond_in}), got {tuple(feats.shape)}")
        if Ta < 2:
            raise L.VauraHipError("scoring needs at least 2 timesteps (the input is codes[..., :-1])")
        dl = self.pattern_delays(delays)
        S = Ta + (K if dl is None else max(dl) + 1)
        if S > c.block_size:               # before any allocation (prepare() refuses only explicit delays)
            raise L.VauraHipError(f"{Ta} timesteps under the delays {list(dl) if dl else list(range(K))} need {S} sequence steps; the "
                                  f"model's block_size is {c.block_size}")
        codes_d = codes.to(self.dev)
        bad = (codes_d < 0) | (codes_d >= c.d_codebook)
        last = None                        # (B, 1, 1): the last timestep of every clip, Ta_b - 1
        if lengths is not None:            # only a clip's own Ta_b columns are its codes
            last = torch.tensor(lengths, device=self.dev).view(B, 1, 1) - 1
            bad &= torch.arange(Ta, device=self.dev).view(1, 1, Ta) <= last
        if bool(bad.any()):
            raise L.VauraHipError(f"codes must lie in [0, {c.d_codebook}) (the reference's cross_entropy refuses other targets)")
        targets = codes_d.to(torch.int32).contiguous()
        self._fc = None                    # the K/V cache is about to be reused: forward_cached must start over
        with off_null_stream(self.dev) as caller:
            self.prepare(B, Ta, feats.shape[1], bool(relevance), tokens_per_frame, block_size=c.block_size, delays=dl)
            self._set_lengths(lengths, video_lengths)      # score(): (None, None), one length per call
            self.set_condition(feats)
            if lengths is None:
                self.codes_i32[..., :Ta - 1] = targets[..., :Ta - 1]
                self.codes_i32[..., Ta - 1] = c.d_codebook             # build_pattern_sequence(codes[..., :-1]): no input beyond Ta - 2
            else:                          # clip b: build_pattern_sequence(codes_b[..., :Ta_b - 1]) — the special id from Ta_b - 1 on
                self.codes_i32.copy_(torch.where(torch.arange(Ta, device=self.dev).view(1, 1, Ta) < last, targets,
                                                 torch.full_like(targets, c.d_codebook)))
            self._pattern_build()
            self._reset_state()
            f32 = dict(dtype=torch.float32, device=self.dev)
            nll = torch.empty(B, K, Ta, **f32)
            mask = torch.empty(B, K, Ta, dtype=torch.uint8, device=self.dev)
            lpc = torch.empty(K, **f32)
            loss = torch.empty((), **f32)
            logits = torch.empty(B, K, Ta, c.d_codebook, **f32) if return_logits else None
            if relevance:
                nll0, lpc0, loss0 = torch.empty(B, K, Ta, **f32), torch.empty(K, **f32), torch.empty((), **f32)
                L.check(self.lib.vaura_score_relevance(C.byref(self.dec), self.S - 1, L.ptr(targets), L.ptr(self._score_workspace()),
                                                       L.ptr(logits), L.ptr(nll), L.ptr(mask), L.ptr(lpc), L.ptr(loss), L.ptr(nll0),
                                                       L.ptr(lpc0), L.ptr(loss0), L.current_stream(self.dev)), "vaura_score_relevance")
            else:
                L.check(self.lib.vaura_score(C.byref(self.dec), self.S - 1, L.ptr(targets), L.ptr(self._score_workspace()), L.ptr(logits),
                                             L.ptr(nll), L.ptr(mask), L.ptr(lpc), L.ptr(loss), L.current_stream(self.dev)), "vaura_score")
            out = {"loss": loss, "loss_per_codebook": lpc, "nll": nll, "mask": mask.bool()}
            if return_logits:
                out["logits"] = logits
            if per_clip:
                pcb, clip = self._clip_means(nll)
                out.update({"lengths": torch.tensor(lengths if lengths is not None else [Ta] * B, dtype=torch.int32, device=self.dev),
                            "nll_per_codebook": pcb, "loss_per_clip": clip})
            if relevance:
                pcb, pcb0 = out["nll_per_codebook"] if per_clip else self._clip_codebook_means(nll), self._clip_codebook_means(nll0)
                rpc = pcb0 - pcb
                out.update({"nll_null": nll0, "loss_null": loss0, "loss_null_per_codebook": lpc0, "nll_per_codebook": pcb,
                            "nll_null_per_codebook": pcb0, "relevance_per_codebook": rpc, "relevance": rpc.sum(-1) / K})
        if caller is not None:
            for t in out.values():
                t.record_stream(caller)
        if not checked:
            return out
        try:
            self.check_status()
            if not bool(torch.isfinite(loss)):
                err = L.VauraHipError("teacher-forced scoring: non-finite loss")
                err.status = 1
                raise err
        except L.VauraHipError as e:
            if getattr(e, "status", 0) != 1 or self.wdtype == "f32" or self._twin_sd is None:
                raise
            if self.range_fallbacks == 0:
                import warnings
                warnings.warn("vaura_amd: teacher-forced scoring gave a non-finite loss (an activation left the fp16-plane range); this "
                              "call is re-run on the exact-fp32 twin engine (slower, ~2.7 GB more)")
            self.range_fallbacks += 1
            if per_clip:                   # the twin scores the same clips: their lengths go with them
                return self._twin().score_clips(codes, feats, lengths, video_lengths=video_lengths, delays=delays,
                                                tokens_per_frame=tokens_per_frame, return_logits=return_logits, relevance=relevance)
            return self._twin().score(codes, feats, delays=delays, tokens_per_frame=tokens_per_frame, return_logits=return_logits,
                                      relevance=relevance)
        return out

    def _clip_codebook_means(self, nll: torch.Tensor) -> torch.Tensor:
        """(B, K, Ta) -> (B, K): the mean over the timesteps of every (clip, codebook) — ``_clip_means`` without the clip's own mean."""
        return self._clip_means(nll)[0]

    def _clip_means(self, nll: torch.Tensor):
        """(B, K, Ta) -> ((B, K), (B,)): the mean over the timesteps of every (clip, codebook) and the mean of those over the codebooks,
        by the fixed-order reduction of the token log-probabilities (``vaura_sequence_logprob``) — the tensor read as a pattern layout
        of zero delays, one unused leading step.  With per-clip lengths set (``score_clips``) the means of clip b run over its own
        t < Ta_b (``vaura_sequence_logprob_clips``), the NaN entries behind its end unread."""
        B, K, Ta = nll.shape
        lay = torch.zeros(B, K, Ta + 1, dtype=torch.float32, device=self.dev)
        lay[..., 1:] = nll
        return self._means(lay, Ta + 1, [0] * K, Ta, 0)


@torch.no_grad()
def score_logits(logits: torch.Tensor, targets: torch.Tensor, mask: torch.Tensor):
    """``VAURAModel._compute_loss`` on a given reverted logits tensor (vaura_model.py:240-280): logits (B, K, T, card) fp32, targets
    (B, K, T), mask (B, K, T) on one HIP device -> (loss (), loss_per_codebook (K,), nll (B, K, T)), through the same NLL and
    fixed-order reduction kernels as ``DecoderEngine.score`` (vaura_score_logits)."""
    if logits.dim() != 4 or targets.shape != logits.shape[:-1] or mask.shape != targets.shape:
        raise L.VauraHipError(f"logits (B, K, T, card), targets and mask (B, K, T) expected, got {tuple(logits.shape)}, "
                              f"{tuple(targets.shape)}, {tuple(mask.shape)}")
    dev = logits.device
    _require_cuda(dev)
    B, K, T, V = logits.shape
    lib = L.lib()
    x = logits.to(torch.float32).contiguous()
    tg = targets.to(dev, torch.int32).contiguous()
    mk = mask.to(dev, torch.uint8).contiguous()
    nll = torch.empty(B, K, T, dtype=torch.float32, device=dev)
    lpc = torch.empty(K, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    L.check(lib.vaura_score_logits(L.ptr(x), L.ptr(tg), L.ptr(mk), B, K, V, T, L.ptr(nll), L.ptr(lpc), L.ptr(loss),
                                   L.current_stream(dev)), "vaura_score_logits")
    return loss, lpc, nll


def _clip_lengths(name: str, lengths, batch: int, hi: int) -> list:
    """One int per clip in 1 .. ``hi`` as a list of Python ints; anything else is refused before any device work."""
    from . import clip_params
    if not clip_params.is_per_clip(lengths):
        raise L.VauraHipError(f"{name} must be one integer per clip (a list, tuple or 1-D tensor), got {lengths!r}")
    n = clip_params._int_list(name, lengths)
    if len(n) != batch:
        raise L.VauraHipError(f"{name} has {len(n)} values for a batch of {batch} clips")
    if min(n) < 1 or max(n) > hi:
        raise L.VauraHipError(f"{name} must lie in 1 .. {hi}, got {n}")
    return n


# codec precision name -> vaura_codec.precision (include/vaura_hip.h); CodecEngine's docstring says what each is
CODEC_PRECISIONS = {"f32": 0, "f16pair": 1, "f16pair_w8": 2, "mx8": 3, "f16": 4}


class CodecEngine:
    """DAC decode (codes -> waveform) on the HIP path; weights from a DAC-1.0.0-keyed state dict."""

    def __init__(self, cfg: CodecCfg, sd: Dict[str, torch.Tensor], device="cuda:0", precision: str = "f16pair"):
        """precision: "f16pair" (default; activations/weights as (hi, lo) fp16 pairs on the fp16 MFMA, error
        ~1e-6 RMS), "f32" (exact fp32 MFMA), "f16" (plain fp16 operands, fp32 accumulate — one matrix instruction per product:
        the arithmetic class the reference runs DAC in, vaura_model.py:92; error ~1e-4 of the signal), or "f16pair_w8" (BASELINE configs[4]: conv weights quantised to fp8 e4m3 with
        a power-of-two scale per output channel — a different model, ``quant.fp8_effective_codec_state_dict`` says which;
        such weights are exact in one fp16 plane, so a product costs two MFMAs instead of three), or "mx8" (configs[4] on the
        fp8 matrix instruction: those fp8 weights AND e4m3 activations with one power-of-two scale per 32 channels of a row,
        ``quant.mx8_effective_activation``; one block-scaled MFMA per 128 products — tolerance reported, not 1e-4)."""
        _require_cuda(device)
        self.cfg, self.dev, self.lib = cfg, torch.device(device), L.lib()
        self._keep = []
        self.pairs = CODEC_PRECISIONS[precision]
        if self.pairs in (2, 3):
            from .quant import fp8_effective_codec_state_dict
            sd = fp8_effective_codec_state_dict(sd)
        c = L.Codec()
        c.precision = self.pairs
        c.n_codebooks, c.codebook_size, c.codebook_dim, c.latent_dim = (cfg.n_codebooks, cfg.codebook_size,
                                                                        cfg.codebook_dim, cfg.latent_dim)
        nb = len(cfg.decoder_rates)
        assert nb <= 4 and len(cfg.dilations) == 3
        c.n_blocks, c.n_units = nb, 3
        for i, r in enumerate(cfg.decoder_rates):
            c.rates[i] = r
        K = cfg.n_codebooks
        f = lambda p: fold_weight_norm(sd[p + "weight_g"].float(), sd[p + "weight_v"].float())
        c.codebooks = L.ptr(self._dev(torch.stack([sd[f"quantizer.quantizers.{k}.codebook.weight"].float() for k in range(K)])))
        c.out_proj_w = L.ptr(self._dev(torch.stack([f(f"quantizer.quantizers.{k}.out_proj.")[:, :, 0] for k in range(K)])))
        c.out_proj_b = L.ptr(self._dev(torch.stack([sd[f"quantizer.quantizers.{k}.out_proj.bias"].float() for k in range(K)])))
        self._conv(c.conv_in, sd, "decoder.model.0.", 1, 1, mx8=False)
        for b, r in enumerate(cfg.decoder_rates):
            p = f"decoder.model.{b + 1}.block."
            c.alpha_up[b] = L.ptr(self._dev(sd[p + "0.alpha"].reshape(-1)))
            self._conv(c.up[b], sd, p + "1.", 1, r)
            for u, dil in enumerate(cfg.dilations):
                q = p + f"{u + 2}.block."
                c.alpha_res[b][u][0] = L.ptr(self._dev(sd[q + "0.alpha"].reshape(-1)))
                self._conv(c.res[b][u][0], sd, q + "1.", dil, 1)
                c.alpha_res[b][u][1] = L.ptr(self._dev(sd[q + "2.alpha"].reshape(-1)))
                self._conv(c.res[b][u][1], sd, q + "3.", 1, 1)
        n = nb + 1
        c.alpha_out = L.ptr(self._dev(sd[f"decoder.model.{n}.alpha"].reshape(-1)))
        self._conv(c.conv_out, sd, f"decoder.model.{n + 1}.", 1, 1)
        self.c = c
        self._ws_key = None

    def _dev(self, t):
        d = t.detach().to(self.dev, torch.float32).contiguous()
        self._keep.append(d)
        return d

    def _conv(self, cv: L.Conv, sd, prefix: str, dilation: int, stride: int, mx8: bool = True):
        w = fold_weight_norm(sd[prefix + "weight_g"].float(), sd[prefix + "weight_v"].float())
        self._pack_conv(cv, w, sd[prefix + "bias"], dilation, stride, mx8)

    def _pack_conv(self, cv: L.Conv, w: torch.Tensor, bias: torch.Tensor, dilation: int, stride: int, mx8: bool = True):
        """Folded Conv1d (Cout, Cin, k) / ConvTranspose1d (Cin, Cout, 2r) weight -> the layout of self.pairs (= vaura_codec.precision)."""
        if stride > 1:   # ConvTranspose1d weight (Cin, Cout, 2r) -> [phase][tap][Cout][Cin]
            cin, cout, k = w.shape
            assert k == 2 * stride
            wl = w.permute(2, 1, 0).reshape(2, stride, cout, cin).permute(1, 0, 2, 3)
            taps = 2
        else:            # Conv1d weight (Cout, Cin, k) -> [tap][Cout][Cin]
            cout, cin, k = w.shape
            wl = w.permute(2, 0, 1)
            taps = k
        if self.pairs == 3 and mx8 and cout > 1:   # packed e4m3 stream + per-output-channel scales (quant.mx8_pack_conv_weight)
            from .quant import mx8_pack_conv_weight
            wp = wl.reshape(stride, 2, cout, cin) if stride > 1 else wl.reshape(1, taps, cout, cin)
            stream, scale = mx8_pack_conv_weight(wp.contiguous().to(self.dev))
            self._keep.append(stream)
            cv.w = L.ptr(stream)
            cv.wscale = L.ptr(self._dev(scale))
        elif self.pairs and cout > 1:   # (hi, lo) fp16 pair layout [.., Cout][Cin/8][plane][8]
            wl = wl.contiguous()
            hi = wl.half()
            lo = (wl - hi.float()).half()
            pr = torch.stack([hi.reshape(*wl.shape[:-1], cin // 8, 8), lo.reshape(*wl.shape[:-1], cin // 8, 8)], dim=-2)
            keep = pr.contiguous().to(self.dev)
            self._keep.append(keep)
            cv.w = L.ptr(keep)
        else:
            cv.w = L.ptr(self._dev(wl))
        cv.bias = L.ptr(self._dev(bias))
        cv.cin, cv.cout, cv.taps, cv.dilation, cv.stride = cin, cout, taps, dilation, stride

    @torch.no_grad()
    def decode(self, codes: torch.Tensor) -> torch.Tensor:
        """codes (B, K, T) integer tensor on device -> wav (B, 1, T*hop) fp32."""
        B, K, T = codes.shape
        with off_null_stream(self.dev) as caller:
            ci = codes.to(self.dev, torch.int32).contiguous()
            need = self.lib.vaura_dac_workspace_elems(C.byref(self.c), B, T)
            if self._ws_key is None or self._ws_key < need:
                self._ws = [torch.empty(need, dtype=torch.float32, device=self.dev) for _ in range(4)]
                for i in range(4):
                    self.c.ws[i] = L.ptr(self._ws[i])
                self.c.ws_elems = need
                self._ws_key = need
            wav = torch.empty(B, 1, T * self.cfg.hop, dtype=torch.float32, device=self.dev)
            L.check(self.lib.vaura_dac_decode(C.byref(self.c), L.ptr(ci), B, T, L.ptr(wav), L.current_stream(self.dev)),
                    "vaura_dac_decode")
            self._codes_keepalive = ci
        if caller is not None:
            wav.record_stream(caller)
        return wav

    @torch.no_grad()
    def decode_clips(self, codes: torch.Tensor, lengths) -> torch.Tensor:
        """codes (B, K, T_max) on device, padded; ``lengths`` one int per clip (host values), 1 <= T_b <= T_max -> wav (B, 1, T_max*hop):
        ``wav[b, :, :T_b*hop]`` is bit for bit ``decode(codes[b:b+1, :, :T_b])``, zeros behind it.  ONE codec pass over the clips packed
        into a single sequence (``codec_clips.clip_layout``; vaura_dac_decode_clips), whatever the lengths."""
        from .codec_clips import clip_layout
        B, K, T = codes.shape
        n = _clip_lengths("lengths", lengths, B, T)
        lay = clip_layout(n, self.cfg, "decode")
        host = (C.c_int32 * B)(*n)
        with off_null_stream(self.dev) as caller:
            ci = codes.to(self.dev, torch.int32).contiguous()
            need = self.lib.vaura_dac_decode_clips_workspace_elems(C.byref(self.c), B, host)
            if need == 0:
                raise L.VauraHipError(f"decode_clips: a packed sequence of {lay.total} frames is beyond what one pass can index")
            if self._ws_key is None or self._ws_key < need:
                self._ws = [torch.empty(need, dtype=torch.float32, device=self.dev) for _ in range(4)]
                for i in range(4):
                    self.c.ws[i] = L.ptr(self._ws[i])
                self.c.ws_elems = need
                self._ws_key = need
            wav = torch.empty(B, 1, T * self.cfg.hop, dtype=torch.float32, device=self.dev)
            L.check(self.lib.vaura_dac_decode_clips(C.byref(self.c), L.ptr(ci), B, T, host, L.ptr(wav), L.current_stream(self.dev)),
                    "vaura_dac_decode_clips")
            self._codes_keepalive = ci
        if caller is not None:
            wav.record_stream(caller)
        return wav

    def _window_call(self, ci: torch.Tensor, n, starts, counts, seq_delays=False) -> torch.Tensor:
        """vaura_dac_decode_window on int32 codes of this device, inside the engine's stream context; grows the workspaces to the
        window's size when they are smaller.  ``seq_delays`` not False: ``ci`` is the decode loop's pattern sequence (B, K, S) under
        those delays (None: 0 .. K - 1) and the call is vaura_dac_decode_window_seq."""
        B, K, T = ci.shape
        host = [(C.c_int32 * B)(*v) for v in (n, starts, counts)]
        if seq_delays is False:
            name, src = "vaura_dac_decode_window", (B, T)
            need = self.lib.vaura_dac_decode_window_workspace_elems(C.byref(self.c), B, *host)
        else:
            name, src = "vaura_dac_decode_window_seq", (B, K, T, None if seq_delays is None else L.delays_host(seq_delays))
            need = self.lib.vaura_dac_decode_window_seq_workspace_elems(C.byref(self.c), *src, *host)
        if need == 0:
            raise L.VauraHipError(f"{name[10:]}: windows {list(zip(starts, counts))} of clips of {n} frames are beyond what one pass can index"
                                  + ("" if seq_delays is False else f", or not inside a pattern sequence of {T} steps"))
        if self._ws_key is None or self._ws_key < need:
            self._ws = [torch.empty(need, dtype=torch.float32, device=self.dev) for _ in range(4)]
            for i in range(4):
                self.c.ws[i] = L.ptr(self._ws[i])
            self.c.ws_elems = need
            self._ws_key = need
        N = max(counts)
        wav = torch.empty(B, 1, N * self.cfg.hop, dtype=torch.float32, device=self.dev)
        L.check(getattr(self.lib, name)(C.byref(self.c), L.ptr(ci), *src, *host, L.ptr(wav), N, L.current_stream(self.dev)), name)
        return wav

    @staticmethod
    def _window_args(B: int, n, starts, counts):
        from . import clip_params
        out = []
        for name, v in (("starts", starts), ("counts", counts)):
            if not clip_params.is_per_clip(v):
                raise L.VauraHipError(f"{name} must be one integer per clip (a list, tuple or 1-D tensor), got {v!r}")
            v = clip_params._int_list(name, v)
            if len(v) != B:
                raise L.VauraHipError(f"{name} has {len(v)} values for a batch of {B} clips")
            out.append(v)
        s, c = out
        if any(a < 0 or k < 0 or a + k > t for a, k, t in zip(s, c, n)):
            raise L.VauraHipError(f"every window must lie inside its clip: lengths {n}, starts {s}, counts {c}")
        if max(c) < 1:
            raise L.VauraHipError(f"decode_window: every count is 0, there is nothing to decode (counts {c})")
        return s, c

    @torch.no_grad()
    def decode_window(self, codes: torch.Tensor, starts, counts, lengths=None) -> torch.Tensor:
        """A window of every clip: codes (B, K, T_max) on device, the whole padded tensor; ``starts`` / ``counts`` one int per clip
        (host values), ``lengths`` as in ``decode_clips`` (None: T_max each) -> wav (B, 1, max(counts)*hop):
        ``wav[b, :, :counts[b]*hop]`` is bit for bit ``decode_clips(codes, lengths)[b, :, starts[b]*hop:(starts[b] + counts[b])*hop]``,
        zeros behind it.  A count of 0 (a finished clip) gives a row of zeros and reads nothing of the clip.  ONE codec pass over the
        windows, each with ``codec_clips.decode_halo`` frames of context either side (``codec_clips.window_layout``;
        vaura_dac_decode_window): its cost and its workspaces follow the windows, not T_max."""
        B, K, T = codes.shape
        n = [T] * B if lengths is None else _clip_lengths("lengths", lengths, B, T)
        s, c = self._window_args(B, n, starts, counts)
        with off_null_stream(self.dev) as caller:
            ci = codes.to(self.dev, torch.int32).contiguous()
            wav = self._window_call(ci, n, s, c)
            self._codes_keepalive = ci
        if caller is not None:
            wav.record_stream(caller)
        return wav

    @torch.no_grad()
    def decode_window_seq(self, seq: torch.Tensor, starts, counts, lengths=None, delays: Optional[Sequence[int]] = None) -> torch.Tensor:
        """``decode_window`` straight from the decode loop's pattern sequence: seq (B, K, S) int32 on this device (``DecoderEngine.seq``)
        under the codebook ``delays`` (None: 0 .. K - 1) holds T = S - 1 - max(d) frames per clip, frame t of codebook q at step
        t + 1 + d_q -> wav (B, 1, max(counts)*hop), bit for bit ``decode_window`` on the reverted codes (vaura_dac_decode_window_seq:
        the pack gathers from the sequence, everything else is that call).  No revert launch, no copy of ``seq``; it may be called
        while the sequence is still being filled, for windows whose frames AND halo are final (``clip_params.releasable_frames``):
        ``lengths`` stays every clip's whole length."""
        if seq.dim() != 3 or seq.dtype != torch.int32 or not seq.is_cuda or not seq.is_contiguous():
            raise L.VauraHipError(f"seq must be a contiguous (B, K, S) int32 tensor on {self.dev}, got {tuple(seq.shape)} {seq.dtype} on {seq.device}")
        B, K, S = seq.shape
        d = None if delays is None else L.check_delays(delays, K)
        T = S - 1 - (K - 1 if d is None else max(d))
        if K < self.cfg.n_codebooks or T < 1:
            raise L.VauraHipError(f"a pattern sequence of {K} codebooks and {S} steps under the delays {list(d) if d else list(range(K))} holds "
                                  f"no frame of the codec's {self.cfg.n_codebooks} codebooks")
        n = [T] * B if lengths is None else _clip_lengths("lengths", lengths, B, T)
        s, c = self._window_args(B, n, starts, counts)
        with off_null_stream(self.dev) as caller:
            wav = self._window_call(seq, n, s, c, seq_delays=d)
        if caller is not None:
            wav.record_stream(caller)
        return wav

    @torch.no_grad()
    def decode_windowed(self, codes: torch.Tensor, window: int, lengths=None) -> torch.Tensor:
        """``decode(codes)`` — with ``lengths``, ``decode_clips(codes, lengths)`` — bit for bit, as successive ``decode_window`` calls of
        ``window`` frames: codes (B, K, T) -> wav (B, 1, T*hop).  The workspaces are sized by the window (plus its halo), not by T.
        A clip that has ended gets count 0 in the later calls.  ``window`` >= T: the one pass itself."""
        B, K, T = codes.shape
        if isinstance(window, bool) or not isinstance(window, int) or window < 1:
            raise L.VauraHipError(f"window must be a positive number of frames, got {window!r}")
        n = [T] * B if lengths is None else _clip_lengths("lengths", lengths, B, T)
        if window >= T:
            return self.decode(codes) if lengths is None or min(n) == T else self.decode_clips(codes, n)
        hop = self.cfg.hop
        with off_null_stream(self.dev) as caller:
            ci = codes.to(self.dev, torch.int32).contiguous()
            wav = torch.zeros(B, 1, T * hop, dtype=torch.float32, device=self.dev)
            for s in range(0, max(n), window):
                counts = [max(0, min(window, t - s)) for t in n]
                part = self._window_call(ci, n, [min(s, t) for t in n], counts)
                wav[:, :, s * hop:s * hop + part.shape[-1]] = part
            self._codes_keepalive = ci
        if caller is not None:
            wav.record_stream(caller)
        return wav


class CodecConvOp:
    """ONE decoder convolution through ``vaura_dac_conv`` (op-level parity tests): folded Conv1d (Cout, Cin, k) or
    ConvTranspose1d (Cin, Cout, 2r; stride r) weight, in the arithmetic of a codec ``precision``.  For "f16pair_w8" / "mx8" the
    caller passes weights that are already fp8-representable (``quant.fp8_effective_weight``)."""

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, dilation: int = 1, stride: int = 1, precision: str = "f16pair",
                 device="cuda:0", mx8_weights: bool = True):
        _require_cuda(device)
        self.dev, self.lib, self._keep = torch.device(device), L.lib(), []
        self.pairs = CODEC_PRECISIONS[precision]
        self.cv = L.Conv()
        CodecEngine._pack_conv(self, self.cv, weight.float(), bias.float(), dilation, stride, mx8_weights)
        self.stride = stride

    _dev = CodecEngine._dev

    @torch.no_grad()
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """x (B, L, Cin) fp32, channels last, already activated -> (B, L * stride, Cout) fp32 = conv(x) + bias."""
        B, Lin, cin = x.shape
        assert cin == self.cv.cin
        with off_null_stream(self.dev) as caller:
            xi = x.to(self.dev, torch.float32).contiguous()
            out = torch.empty(B, Lin * self.stride, self.cv.cout, dtype=torch.float32, device=self.dev)
            scratch = torch.empty(B * Lin * cin + 64, dtype=torch.float32, device=self.dev)
            L.check(self.lib.vaura_dac_conv(C.byref(self.cv), self.pairs, L.ptr(xi), L.ptr(out), L.ptr(scratch), B, Lin,
                                            L.current_stream(self.dev)), "vaura_dac_conv")
            self._keepalive = (xi, scratch)
        if caller is not None:
            out.record_stream(caller)
        return out


    @torch.no_grad()
    def ex(self, x: torch.Tensor, res: Optional[torch.Tensor] = None, alpha: Optional[torch.Tensor] = None,
           out_raw: Optional[torch.Tensor] = None, out_act: Optional[torch.Tensor] = None) -> None:
        """The convolution with the epilogue of the decode path, through ``vaura_dac_conv_ex``: x (B, L, Cin) fp32, res (B, L * stride, Cout)
        fp32 or None, alpha (Cout) for out_act.  out_raw (fp32) / out_act (``codec_act_bytes`` bytes of any dtype, in the precision's own
        activation format) are contiguous device tensors the CALLER allocates — a view into a larger buffer with guard rows, in the
        parity tests — and the launch writes into."""
        B, Lin, cin = x.shape
        assert cin == self.cv.cin and (out_raw is not None or out_act is not None)
        _cuda_contiguous(res, alpha, out_raw, out_act)
        with off_null_stream(self.dev):
            xi = x.to(self.dev, torch.float32).contiguous()
            scratch = torch.empty(B * Lin * cin + 64, dtype=torch.float32, device=self.dev)
            L.check(self.lib.vaura_dac_conv_ex(C.byref(self.cv), self.pairs, L.ptr(xi), L.ptr(res), L.ptr(alpha), L.ptr(out_raw),
                                               L.ptr(out_act), L.ptr(scratch), B, Lin, L.current_stream(self.dev)), "vaura_dac_conv_ex")
            self._keepalive = (xi, scratch)


def _cuda_contiguous(*ts):
    for t in ts:
        if t is not None and not (t.is_cuda and t.is_contiguous()):
            raise L.VauraHipError("op-level codec entry: contiguous tensors on a HIP device expected")


def codec_act_bytes(precision: str, rows: int, Cc: int) -> int:
    """Bytes of an activated (rows, C) tensor in the activation format of a codec precision (include/vaura_hip.h, vaura_dac_conv_ex):
    fp32 or pair planes: 4 per element; "mx8": the e4m3 bytes, padded to 16, then one word of four E8M0 bytes per 128 channels of a row."""
    if precision != "mx8":
        return 4 * rows * Cc
    return ((rows * Cc + 15) & ~15) + rows * ((Cc + 127) // 128) * 4


class CodecUnitOp:
    """ONE residual unit of the decoder through ``vaura_dac_unit`` (op-level parity tests): 7-tap dilated conv (C, C, 7) -> Snake ->
    1 x 1 conv (C, C, 1) -> + residual, in the arithmetic of a codec ``precision``."""

    def __init__(self, w7: torch.Tensor, b7: torch.Tensor, dilation: int, w1: torch.Tensor, b1: torch.Tensor,
                 precision: str = "f16pair", device="cuda:0"):
        _require_cuda(device)
        self.dev, self.lib, self._keep = torch.device(device), L.lib(), []
        self.pairs = CODEC_PRECISIONS[precision]
        self.c7, self.c1 = L.Conv(), L.Conv()
        CodecEngine._pack_conv(self, self.c7, w7.float(), b7.float(), dilation, 1)
        CodecEngine._pack_conv(self, self.c1, w1.float(), b1.float(), 1, 1)

    _dev = CodecEngine._dev

    @torch.no_grad()
    def __call__(self, x: torch.Tensor, res: torch.Tensor, alpha_mid: torch.Tensor, alpha_next: torch.Tensor,
                 out_raw: Optional[torch.Tensor], out_act: torch.Tensor, mid: Optional[torch.Tensor] = None) -> bool:
        """x (B, L, C) fp32 = Snake of the unit's input, res (B, L, C) the input itself; out_raw / out_act / mid: device tensors of the
        caller as in ``CodecConvOp.ex`` (mid: ``codec_act_bytes`` bytes, the activated output of the first conv when two launches ran).
        True: the unit ran as ONE launch.  False: as two (mid given) or not at all (mid None)."""
        B, Ln, cin = x.shape
        assert cin == self.c7.cin and res.shape == x.shape
        _cuda_contiguous(res, alpha_mid, alpha_next, out_raw, out_act, mid)
        with off_null_stream(self.dev):
            xi = x.to(self.dev, torch.float32).contiguous()
            scratch = torch.empty(B * Ln * cin + 64, dtype=torch.float32, device=self.dev)
            rc = self.lib.vaura_dac_unit(C.byref(self.c7), C.byref(self.c1), self.pairs, L.ptr(xi), L.ptr(res), L.ptr(alpha_mid),
                                         L.ptr(alpha_next), L.ptr(out_raw), L.ptr(out_act), L.ptr(scratch), L.ptr(mid), B, Ln,
                                         L.current_stream(self.dev))
            self._keepalive = (xi, scratch)
        if rc == L.DAC_UNIT_TWO_LAUNCHES:
            return False
        L.check(rc, "vaura_dac_unit")
        return True


@torch.no_grad()
def codec_from_codes(codes: torch.Tensor, codebooks: torch.Tensor, out_proj_w: torch.Tensor, out_proj_b: torch.Tensor,
                     out: torch.Tensor, pairs: bool) -> None:
    """``quantizer.from_codes`` through ``vaura_dac_from_codes``: codes (B, K, T) int32, codebooks (K, size, dim), out_proj_w (K, latent,
    dim), out_proj_b (K, latent) fp32 -> out (B, T, latent), fp32 or (pairs) pair planes; every tensor the caller's, on one HIP device."""
    _cuda_contiguous(codes, codebooks, out_proj_w, out_proj_b, out)
    assert codes.dtype == torch.int32
    B, K, T = codes.shape
    _, size, dim = codebooks.shape
    latent = out_proj_w.shape[1]
    with off_null_stream(out.device):
        L.check(L.lib().vaura_dac_from_codes(L.ptr(codes), L.ptr(codebooks), L.ptr(out_proj_w), L.ptr(out_proj_b), L.ptr(out), B, K, T,
                                             size, dim, latent, 1 if pairs else 0, L.current_stream(out.device)), "vaura_dac_from_codes")


@torch.no_grad()
def codec_conv_out(w: torch.Tensor, bias: torch.Tensor, x: torch.Tensor, out: torch.Tensor, precision: str = "f16pair") -> None:
    """The decoder's last convolution through ``vaura_dac_conv_out``: w (1, C, 7) Conv1d weight, bias (1), x (B, L, C) fp32 (stored in the
    activation format of ``precision`` by the entry) -> out (B, L) fp32 = tanh(conv), the caller's tensor."""
    _cuda_contiguous(x, out)
    dev = x.device
    pairs = CODEC_PRECISIONS[precision]
    B, Ln, Cc = x.shape
    cv = L.Conv()
    wl = w.float()[0].t().contiguous().to(dev)          # [7][C]
    bl = bias.float().contiguous().to(dev)
    cv.w, cv.bias, cv.cin, cv.cout, cv.taps, cv.dilation, cv.stride = L.ptr(wl), L.ptr(bl), Cc, 1, 7, 1, 1
    with off_null_stream(dev):
        xi = x.float().contiguous()
        scratch = torch.empty(B * Ln * Cc + 64, dtype=torch.float32, device=dev)
        L.check(L.lib().vaura_dac_conv_out(C.byref(cv), pairs, L.ptr(xi), L.ptr(out), L.ptr(scratch), B, Ln, L.current_stream(dev)),
                "vaura_dac_conv_out")
        torch.cuda.current_stream(dev).synchronize()    # wl, bl, xi, scratch die with this frame


@torch.no_grad()
def codec_enc_conv_in(wav: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, alpha: torch.Tensor, out_raw: torch.Tensor,
                      out_act: torch.Tensor) -> None:
    """The encoder's first convolution through ``vaura_dac_enc_conv_in``: wav (B, L), w (7, C), bias (C), alpha (C) fp32 -> out_raw (B, L,
    C) fp32 and out_act, Snake(alpha) of it in pair planes; every tensor the caller's, on one HIP device."""
    _cuda_contiguous(wav, w, bias, alpha, out_raw, out_act)
    B, Ln = wav.shape
    with off_null_stream(wav.device):
        L.check(L.lib().vaura_dac_enc_conv_in(L.ptr(wav), L.ptr(w), L.ptr(bias), L.ptr(alpha), L.ptr(out_raw), L.ptr(out_act), B, Ln,
                                              w.shape[1], L.current_stream(wav.device)), "vaura_dac_enc_conv_in")


@torch.no_grad()
def codec_rvq_stage(residual: torch.Tensor, in_w: torch.Tensor, in_b: torch.Tensor, codebook: torch.Tensor, out_w: torch.Tensor,
                    out_b: torch.Tensor, codes: torch.Tensor, k: int) -> None:
    """ONE residual-VQ stage through ``vaura_dac_rvq_stage``: residual (B, T, latent) fp32 updated IN PLACE, the stage's in_w (dim, latent),
    in_b (dim), codebook (size, dim), out_w (latent, dim), out_b (latent); codes (B, K, T) int32 receives plane k."""
    _cuda_contiguous(residual, in_w, in_b, codebook, out_w, out_b, codes)
    assert codes.dtype == torch.int32
    B, T, latent = residual.shape
    size, dim = codebook.shape
    with off_null_stream(residual.device):
        L.check(L.lib().vaura_dac_rvq_stage(L.ptr(residual), L.ptr(in_w), L.ptr(in_b), L.ptr(codebook), L.ptr(out_w), L.ptr(out_b),
                                            L.ptr(codes), B, T, latent, dim, size, codes.shape[1], k,
                                            L.current_stream(residual.device)), "vaura_dac_rvq_stage")


def snake(x: torch.Tensor, alpha: torch.Tensor, device="cuda:0") -> torch.Tensor:
    """The codec's activation through ``vaura_snake`` (op-level parity tests): x (..., C) fp32 channels-last, alpha (C)."""
    _require_cuda(device)
    dev = torch.device(device)
    with off_null_stream(dev) as caller:
        xi = x.to(dev, torch.float32).contiguous()
        al = alpha.to(dev, torch.float32).contiguous()
        y = torch.empty_like(xi)
        L.check(L.lib().vaura_snake(L.ptr(xi), L.ptr(al), L.ptr(y), xi.numel() // xi.shape[-1], xi.shape[-1], L.current_stream(dev)),
                "vaura_snake")
    if caller is not None:
        y.record_stream(caller)
    return y


class CodecEncoderEngine:
    """DAC encode (waveform -> codes) on the HIP path; weights from a DAC-1.0.0-keyed state dict
    (``encoder.block.*``, ``quantizer.quantizers.N.{in_proj,codebook,out_proj}``).  Convolutions run on (hi, lo) fp16
    pairs like the decoder's default precision."""

    def __init__(self, cfg: CodecCfg, sd: Dict[str, torch.Tensor], device="cuda:0"):
        _require_cuda(device)
        self.cfg, self.dev, self.lib = cfg, torch.device(device), L.lib()
        self._keep = []
        c = L.CodecEncoder()
        c.n_codebooks, c.codebook_size, c.codebook_dim, c.latent_dim = (cfg.n_codebooks, cfg.codebook_size,
                                                                        cfg.codebook_dim, cfg.latent_dim)
        nb = len(cfg.encoder_rates)
        assert nb <= 4 and len(cfg.dilations) == 3
        c.n_blocks, c.n_units, c.enc_dim = nb, 3, cfg.encoder_dim
        for i, r in enumerate(cfg.encoder_rates):
            c.rates[i] = r
        K = cfg.n_codebooks
        f = lambda p: fold_weight_norm(sd[p + "weight_g"].float(), sd[p + "weight_v"].float())
        q = "quantizer.quantizers."
        c.in_proj_w = L.ptr(self._dev(torch.stack([f(f"{q}{k}.in_proj.")[:, :, 0] for k in range(K)])))
        c.in_proj_b = L.ptr(self._dev(torch.stack([sd[f"{q}{k}.in_proj.bias"].float() for k in range(K)])))
        c.codebooks = L.ptr(self._dev(torch.stack([sd[f"{q}{k}.codebook.weight"].float() for k in range(K)])))
        c.out_proj_w = L.ptr(self._dev(torch.stack([f(f"{q}{k}.out_proj.")[:, :, 0] for k in range(K)])))
        c.out_proj_b = L.ptr(self._dev(torch.stack([sd[f"{q}{k}.out_proj.bias"].float() for k in range(K)])))
        w0 = f("encoder.block.0.")                                   # (C, 1, 7) -> [tap][C]
        c.conv_in_w = L.ptr(self._dev(w0[:, 0, :].t()))
        c.conv_in_b = L.ptr(self._dev(sd["encoder.block.0.bias"]))
        d = cfg.encoder_dim
        for b, r in enumerate(cfg.encoder_rates):
            p = f"encoder.block.{b + 1}.block."
            for u, dil in enumerate(cfg.dilations):
                qq = p + f"{u}.block."
                c.alpha_res[b][u][0] = L.ptr(self._dev(sd[qq + "0.alpha"].reshape(-1)))
                self._conv(c.res[b][u][0], f(qq + "1.").permute(2, 0, 1), sd[qq + "1.bias"], dil)
                c.alpha_res[b][u][1] = L.ptr(self._dev(sd[qq + "2.alpha"].reshape(-1)))
                self._conv(c.res[b][u][1], f(qq + "3.").permute(2, 0, 1), sd[qq + "3.bias"], 1)
            c.alpha_down[b] = L.ptr(self._dev(sd[p + "3.alpha"].reshape(-1)))
            self._conv(c.down[b], self.strided_as_three_taps(f(p + "4."), r), sd[p + "4.bias"], 1)
            d *= 2
        n = nb + 1
        c.alpha_out = L.ptr(self._dev(sd[f"encoder.block.{n}.alpha"].reshape(-1)))
        self._conv(c.conv_out, f(f"encoder.block.{n + 1}.").permute(2, 0, 1), sd[f"encoder.block.{n + 1}.bias"], 1)
        self.c = c
        self._ws_key = None

    @staticmethod
    def strided_as_three_taps(w: torch.Tensor, r: int) -> torch.Tensor:
        """Conv1d weight (2C, C, 2r) with stride r, pad r/2  ->  [3][2C][r*C]: the same sum written over rows of r*C
        channels (input (L, C) read as (L/r, r*C)): w'[tau+1][co][q*C + ci] = w[co][ci][tau*r + q + r/2]."""
        cout, cin, k = w.shape
        assert k == 2 * r and r % 2 == 0
        out = torch.zeros(3, cout, r * cin, dtype=w.dtype)
        for tau in (-1, 0, 1):
            for qi in range(r):
                t = tau * r + qi + r // 2
                if 0 <= t < k:
                    out[tau + 1, :, qi * cin:(qi + 1) * cin] = w[:, :, t]
        return out

    def _dev(self, t):
        d = t.detach().to(self.dev, torch.float32).contiguous()
        self._keep.append(d)
        return d

    def _conv(self, cv: L.Conv, wl: torch.Tensor, bias: torch.Tensor, dilation: int):
        """wl: [taps][Cout][Cin] fp32 -> (hi, lo) fp16 pair layout [taps][Cout][Cin/8][plane][8]."""
        wl = wl.contiguous().float()
        taps, cout, cin = wl.shape
        hi = wl.half()
        lo = (wl - hi.float()).half()
        pr = torch.stack([hi.reshape(taps, cout, cin // 8, 8), lo.reshape(taps, cout, cin // 8, 8)], dim=-2)
        keep = pr.contiguous().to(self.dev)
        self._keep.append(keep)
        cv.w = L.ptr(keep)
        cv.bias = L.ptr(self._dev(bias))
        cv.cin, cv.cout, cv.taps, cv.dilation, cv.stride = cin, cout, taps, dilation, 1

    @torch.no_grad()
    def encode(self, wav: torch.Tensor) -> torch.Tensor:
        """wav (B, 1, N) / (B, N) / (N) on the device -> codes (B, K, ceil(N / hop)) int64.  The zero padding of
        ``DAC.preprocess`` is applied here."""
        if wav.dim() == 1:
            wav = wav[None]
        if wav.dim() == 3:
            wav = wav[:, 0]
        hop = int(math.prod(self.cfg.encoder_rates))
        B, N = wav.shape
        T = (N + hop - 1) // hop
        with off_null_stream(self.dev) as caller:
            x = torch.zeros(B, T * hop, dtype=torch.float32, device=self.dev)
            x[:, :N] = wav.to(self.dev, torch.float32)
            need = self.lib.vaura_dac_encode_workspace_elems(C.byref(self.c), B, T * hop)
            if self._ws_key is None or self._ws_key < need:
                self._ws = [torch.empty(need, dtype=torch.float32, device=self.dev) for _ in range(4)]
                for i in range(4):
                    self.c.ws[i] = L.ptr(self._ws[i])
                self.c.ws_elems = need
                self._ws_key = need
            codes = torch.empty(B, self.cfg.n_codebooks, T, dtype=torch.int32, device=self.dev)
            L.check(self.lib.vaura_dac_encode(C.byref(self.c), L.ptr(x), B, T * hop, L.ptr(codes), L.current_stream(self.dev)),
                    "vaura_dac_encode")
            out = codes.to(torch.int64)
        if caller is not None:
            out.record_stream(caller)
        return out

    @torch.no_grad()
    def encode_clips(self, wav: torch.Tensor, sample_lengths) -> torch.Tensor:
        """wav (B, 1, N) / (B, N) on the device, padded; ``sample_lengths`` one int per clip (host values), 1 <= n_b <= N -> codes
        (B, K, ceil(N / hop)) int64: ``codes[b, :, :ceil(n_b / hop)]`` is bit for bit ``encode(wav[b:b+1, ..., :n_b])``, 0 behind it.
        ONE encoder pass over the clips packed into a single sequence (``codec_clips.clip_layout``; vaura_dac_encode_clips)."""
        from .codec_clips import clip_layout
        if wav.dim() == 3:
            wav = wav[:, 0]
        if wav.dim() != 2:
            raise L.VauraHipError(f"encode_clips takes a (B, 1, N) or (B, N) batch, got shape {tuple(wav.shape)}")
        B, N = wav.shape
        n = _clip_lengths("sample_lengths", sample_lengths, B, N)
        lay = clip_layout(n, self.cfg, "encode")
        host = (C.c_int64 * B)(*n)
        T = (N + lay.hop - 1) // lay.hop
        with off_null_stream(self.dev) as caller:
            x = wav.to(self.dev, torch.float32).contiguous()
            need = self.lib.vaura_dac_encode_clips_workspace_elems(C.byref(self.c), B, host)
            if need == 0:
                raise L.VauraHipError(f"encode_clips: a packed sequence of {lay.total} frames is beyond what one pass can index")
            if self._ws_key is None or self._ws_key < need:
                self._ws = [torch.empty(need, dtype=torch.float32, device=self.dev) for _ in range(4)]
                for i in range(4):
                    self.c.ws[i] = L.ptr(self._ws[i])
                self.c.ws_elems = need
                self._ws_key = need
            codes = torch.empty(B, self.cfg.n_codebooks, T, dtype=torch.int32, device=self.dev)
            L.check(self.lib.vaura_dac_encode_clips(C.byref(self.c), L.ptr(x), B, N, host, L.ptr(codes), L.current_stream(self.dev)),
                    "vaura_dac_encode_clips")
            self._wav_keepalive = x
            out = codes.to(torch.int64)
        if caller is not None:
            out.record_stream(caller)
        return out


class AvclipEngine:
    """Segment-AVCLIP visual features on the HIP path: weights from a state dict with the reference
    MotionFormer's key names (``synth.avclip_state_dict`` lists them), frames (B, S, 3, 16, 224, 224) -> (B, S, 8, 768)."""

    def __init__(self, cfg, sd: Dict[str, torch.Tensor], device="cuda:0"):
        _require_cuda(device)
        self.cfg, self.dev, self.lib = cfg, torch.device(device), L.lib()
        self._keep = []
        D, Hd = cfg.embed_dim, cfg.embed_dim * cfg.mlp_ratio
        v = L.Vit()
        v.depth, v.dim, v.heads, v.hidden = cfg.depth, D, cfg.num_heads, Hd
        v.n_patches, v.n_frames = cfg.n, cfg.t
        v.in_chans, v.frames, v.img, v.patch, v.patch_t = cfg.in_chans, cfg.frames, cfg.img, cfg.patch, cfg.patch_t
        v.patch_k = cfg.in_chans * cfg.patch_t * cfg.patch * cfg.patch
        v.eps = 1e-6
        f, p = self._f32, self._pair
        v.pe_w, v.pe_b = p(sd["patch_embed_3d.proj.weight"].reshape(D, -1)), f(sd["patch_embed_3d.proj.bias"])
        v.cls_token, v.pos_embed, v.temp_embed = f(sd["cls_token"]), f(sd["pos_embed"]), f(sd["temp_embed"])
        blocks = (L.VitBlock * cfg.depth)()
        for i in range(cfg.depth):
            b, q = blocks[i], f"blocks.{i}."
            b.ln1_w, b.ln1_b = f(sd[q + "norm1.weight"]), f(sd[q + "norm1.bias"])
            b.ln2_w, b.ln2_b = f(sd[q + "norm2.weight"]), f(sd[q + "norm2.bias"])
            b.ln3_w, b.ln3_b = f(sd[q + "norm3.weight"]), f(sd[q + "norm3.bias"])
            for att, name in ((b.space, "attn."), (b.time, "timeattn.")):
                att.qkv_w, att.qkv_b = p(sd[q + name + "qkv.weight"]), f(sd[q + name + "qkv.bias"])
                att.proj_w, att.proj_b = p(sd[q + name + "proj.weight"]), f(sd[q + name + "proj.bias"])
            b.fc1_w, b.fc1_b = p(sd[q + "mlp.fc1.weight"]), f(sd[q + "mlp.fc1.bias"])
            b.fc2_w, b.fc2_b = p(sd[q + "mlp.fc2.weight"]), f(sd[q + "mlp.fc2.bias"])
        self._blocks = blocks
        v.blocks_host = C.cast(blocks, C.POINTER(L.VitBlock))
        v.norm_w, v.norm_b = f(sd["norm.weight"]), f(sd["norm.bias"])
        a = "spatial_attn_agg."
        v.agg_cls = f(sd[a + "cls_token"])
        v.agg_ln1_w, v.agg_ln1_b = f(sd[a + "norm1.weight"]), f(sd[a + "norm1.bias"])
        v.agg_ln2_w, v.agg_ln2_b = f(sd[a + "norm2.weight"]), f(sd[a + "norm2.bias"])
        v.agg_in_w, v.agg_in_b = p(sd[a + "self_attn.in_proj_weight"]), f(sd[a + "self_attn.in_proj_bias"])
        v.agg_out_w, v.agg_out_b = p(sd[a + "self_attn.out_proj.weight"]), f(sd[a + "self_attn.out_proj.bias"])
        v.agg_l1_w, v.agg_l1_b = p(sd[a + "linear1.weight"]), f(sd[a + "linear1.bias"])
        v.agg_l2_w, v.agg_l2_b = p(sd[a + "linear2.weight"]), f(sd[a + "linear2.bias"])
        self.v = v
        self._ws_segs = 0

    def _f32(self, t) -> int:
        d = t.detach().to(self.dev, torch.float32).contiguous()
        self._keep.append(d)
        return L.ptr(d)

    def _pair(self, w) -> int:
        """(Cout, Cin) fp32 -> (hi, lo) fp16 pair layout [Cout][Cin/8][plane][8] (the codec's weight layout, one tap)."""
        w = w.detach().to(self.dev, torch.float32).contiguous()
        cout, cin = w.shape
        hi = w.half()
        lo = (w - hi.float()).half()
        pr = torch.stack([hi.reshape(cout, cin // 8, 8), lo.reshape(cout, cin // 8, 8)], dim=-2).contiguous()
        self._keep.append(pr)
        return L.ptr(pr)

    # segments per pass: bounds the workspaces (a pass of 32 segments = 8 clips holds ~1.7 GB)
    MAX_SEGMENTS = 32

    def _workspaces(self, n_seg: int):
        if n_seg <= self._ws_segs:
            return
        names = ["ws_x", "ws_qkv", "ws_a", "ws_h", "ws_p", "ws_z", "ws_s"]
        self._ws = []
        for i, nm in enumerate(names):
            nbytes = self.lib.vaura_avclip_workspace_bytes(C.byref(self.v), n_seg, i)
            t = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
            self._ws.append(t)
            setattr(self.v, nm, L.ptr(t))
        self._ws_segs = n_seg

    @torch.no_grad()
    def forward(self, frames: torch.Tensor) -> torch.Tensor:
        """frames (B, S, 3, 16, 224, 224) on the device -> features (B, S, 8, 768) fp32."""
        c = self.cfg
        B, S = frames.shape[:2]
        if tuple(frames.shape[2:]) != (c.in_chans, c.frames, c.img, c.img):
            raise L.VauraHipError(f"AvclipEngine: segments must be ({c.in_chans}, {c.frames}, {c.img}, {c.img}), got {tuple(frames.shape[2:])}")
        with off_null_stream(self.dev) as caller:
            x = frames.to(self.dev, torch.float32).reshape(B * S, *frames.shape[2:]).contiguous()
            out = torch.empty(B * S, c.t, c.embed_dim, dtype=torch.float32, device=self.dev)
            step = min(self.MAX_SEGMENTS, B * S)
            self._workspaces(step)
            for s0 in range(0, B * S, step):
                n = min(step, B * S - s0)
                L.check(self.lib.vaura_avclip_forward(C.byref(self.v), L.ptr(x[s0:]), n, L.ptr(out[s0:]), L.current_stream(self.dev)),
                        "vaura_avclip_forward")
            self._frames_keepalive = x
        if caller is not None:
            out.record_stream(caller)
        return out.view(B, S, c.t, c.embed_dim)
