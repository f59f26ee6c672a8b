"""Thin torch-tensor wrappers over the C ABI (one function per entry point of include/vaura_hip.h).
All tensors must live on a HIP device; nothing here computes on the CPU."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib as L


def _cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.VauraHipError("HIP path only: tensor is not on a HIP device (no CPU fallback)")


def pack_weight(w: torch.Tensor, wdtype: int) -> torch.Tensor:
    _cuda(w)
    N, K = w.shape
    src = w.float().contiguous()
    dst = torch.empty(L.lib().vaura_packed_weight_bytes(N, K, wdtype), dtype=torch.uint8, device=w.device)
    L.check(L.lib().vaura_pack_weight(L.ptr(src), L.ptr(dst), N, K, wdtype, L.current_stream()), "vaura_pack_weight")
    torch.cuda.current_stream().synchronize()
    return dst


def pack_rows(x: torch.Tensor) -> torch.Tensor:
    _cuda(x)
    rows, Cc = x.shape
    src = x.float().contiguous()
    dst = torch.empty(((rows + 15) // 16 * 16) * Cc, dtype=torch.float32, device=x.device)
    L.check(L.lib().vaura_pack_rows(L.ptr(src), L.ptr(dst), rows, Cc, L.current_stream()), "vaura_pack_rows")
    torch.cuda.current_stream().synchronize()
    return dst


def unpack_rows(xp: torch.Tensor, rows: int, Cc: int) -> torch.Tensor:
    _cuda(xp)
    dst = torch.empty(rows, Cc, dtype=torch.float32, device=xp.device)
    L.check(L.lib().vaura_unpack_rows(L.ptr(xp), L.ptr(dst), rows, Cc, L.current_stream()), "vaura_unpack_rows")
    return dst


def gemv(wp: torch.Tensor, wdtype: int, xp: torch.Tensor, rows: int, N: int, K: int, epilogue: int = L.EPI_STORE,
         gain: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, eps: float = 1e-5) -> torch.Tensor:
    """Returns packed rows (rows x N') except for EPI_LOGITS (row-major (rows, N))."""
    _cuda(wp, xp, gain, residual)
    n_out = N // 2 if epilogue == L.EPI_SWIGLU else N
    rp = (rows + 15) // 16 * 16
    if epilogue == L.EPI_LOGITS:
        out = torch.zeros(rows, N, dtype=torch.float32, device=xp.device)
    else:
        out = torch.zeros(rp * n_out, dtype=torch.float32, device=xp.device)
    L.check(L.lib().vaura_gemv(L.ptr(wp), wdtype, L.ptr(xp), L.ptr(gain), L.ptr(residual), L.ptr(out), rows, N, K,
                               epilogue, eps, L.current_stream()), "vaura_gemv")
    return out


def attention_step(qkv_p: torch.Tensor, rope: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, rows: int,
                   n_head: int, head_dim: int, pos: int) -> torch.Tensor:
    _cuda(qkv_p, rope, kcache, vcache)
    max_len = kcache.shape[-2]
    out = torch.zeros(((rows + 15) // 16 * 16) * n_head * head_dim, dtype=torch.float32, device=qkv_p.device)
    L.check(L.lib().vaura_attention_step(L.ptr(qkv_p), L.ptr(rope), L.ptr(kcache), L.ptr(vcache), L.ptr(out), rows,
                                         n_head, head_dim, max_len, pos, L.current_stream()), "vaura_attention_step")
    return out


def attention_step_split(qkv_p: torch.Tensor, rope: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, rows: int,
                         n_head: int, head_dim: int, pos: int, n_split: int) -> torch.Tensor:
    """attention_step with the cached range of every (row, head) split over `n_split` workgroups + a combine pass."""
    _cuda(qkv_p, rope, kcache, vcache)
    max_len = kcache.shape[-2]
    out = torch.zeros(((rows + 15) // 16 * 16) * n_head * head_dim, dtype=torch.float32, device=qkv_p.device)
    part = torch.empty(rows * n_head * n_split * (head_dim + 8), dtype=torch.float32, device=qkv_p.device)
    L.check(L.lib().vaura_attention_step_split(L.ptr(qkv_p), L.ptr(rope), L.ptr(kcache), L.ptr(vcache), L.ptr(out),
                                               L.ptr(part), rows, n_head, head_dim, max_len, pos, n_split,
                                               L.current_stream()), "vaura_attention_step_split")
    return out


def attention_step_ex(qkv_p: torch.Tensor, rope: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, rows: int, n_head: int,
                      head_dim: int, pos: int, *, kv_dtype: int = 0, qkv2_p: Optional[torch.Tensor] = None, n_split: int = 1,
                      part: Optional[torch.Tensor] = None, arrivals: Optional[torch.Tensor] = None, want_split: bool = False,
                      plane_shift: int = 0, out: Optional[torch.Tensor] = None, out_split: Optional[torch.Tensor] = None):
    """vaura_attention_step_ex: ``attention_step_kv`` without the scaled storage (kv_dtype 0..2: fp32, fp16, e4m3), refused here as the C
    entry point refuses it."""
    if kv_dtype == 3:
        L.check(-1, "vaura_attention_step_ex")      # VAURA_ERR_ARG: it has nowhere to take the exponent bytes
    return attention_step_kv(qkv_p, rope, kcache, vcache, rows, n_head, head_dim, pos, kv_dtype=kv_dtype, qkv2_p=qkv2_p, n_split=n_split,
                             part=part, arrivals=arrivals, want_split=want_split, plane_shift=plane_shift, out=out, out_split=out_split)


def attention_step_kv(qkv_p: torch.Tensor, rope: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, rows: int, n_head: int,
                      head_dim: int, pos: int, *, kv_dtype: int = 0, kscale: Optional[torch.Tensor] = None,
                      vscale: Optional[torch.Tensor] = None, qkv2_p: Optional[torch.Tensor] = None, n_split: int = 1,
                      part: Optional[torch.Tensor] = None, arrivals: Optional[torch.Tensor] = None, want_split: bool = False,
                      plane_shift: int = 0, out: Optional[torch.Tensor] = None, out_split: Optional[torch.Tensor] = None):
    """vaura_attention_step_kv: one decode-step attention with every optional of the step.  kcache / vcache (rows, n_head, max_len,
    head_dim) in the storage of ``kv_dtype`` (fp32, fp16, e4m3, scaled e4m3).  kv_dtype = 3: kcache / vcache hold the bytes (uint8 or
    float8_e4m3fn), kscale / vscale (rows, n_head, max_len) uint8 the exponent byte of every cached vector.  Returns (out packed rows,
    out_split or None); ``out`` / ``out_split`` / ``part`` may be passed in (pre-filled) instead of allocated here."""
    _cuda(qkv_p, qkv2_p, rope, kcache, vcache, kscale, vscale, part, arrivals, out, out_split)
    max_len = kcache.shape[-2]
    rp = (rows + 15) // 16 * 16
    dev = qkv_p.device
    if out is None:
        out = torch.zeros(rp * n_head * head_dim, dtype=torch.float32, device=dev)
    if want_split and out_split is None:
        out_split = torch.zeros(rp * 2 * n_head * head_dim, dtype=torch.int16, device=dev)
    if n_split > 1 and part is None:
        part = torch.empty(rows * n_head * n_split * (head_dim + 8), dtype=torch.float32, device=dev)
    L.check(L.lib().vaura_attention_step_kv(L.ptr(qkv_p), L.ptr(qkv2_p), L.ptr(rope), L.ptr(kcache), L.ptr(vcache), L.ptr(kscale),
                                            L.ptr(vscale), L.ptr(out), L.ptr(out_split), L.ptr(part), L.ptr(arrivals), rows, n_head,
                                            head_dim, max_len, pos, n_split, plane_shift, kv_dtype, L.current_stream()),
            "vaura_attention_step_kv")
    return out, out_split


def attention_step_probs(qkv_p: torch.Tensor, rope: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, rows: int, n_head: int,
                         head_dim: int, pos: int, probs: torch.Tensor, pos0: int, *, kv_dtype: int = 0,
                         kscale: Optional[torch.Tensor] = None, vscale: Optional[torch.Tensor] = None,
                         qkv2_p: Optional[torch.Tensor] = None, n_split: int = 1, want_split: bool = False, plane_shift: int = 0,
                         out: Optional[torch.Tensor] = None, out_split: Optional[torch.Tensor] = None):
    """vaura_attention_step_probs: ``attention_step_kv`` that also reports the step's softmax weights into ``probs`` (n_steps, rows_out,
    n_head, max_len) fp32 — row (pos - pos0) of it, for rows < rows_out, when pos0 <= pos < pos0 + n_steps.  Returns (out, out_split)."""
    _cuda(qkv_p, qkv2_p, rope, kcache, vcache, kscale, vscale, out, out_split, probs)
    max_len = kcache.shape[-2]
    n_steps, rows_out = int(probs.shape[0]), int(probs.shape[1])
    assert probs.dtype == torch.float32 and probs.is_contiguous() and tuple(probs.shape[2:]) == (n_head, max_len)
    rp = (rows + 15) // 16 * 16
    dev = qkv_p.device
    if out is None:
        out = torch.zeros(rp * n_head * head_dim, dtype=torch.float32, device=dev)
    if want_split and out_split is None:
        out_split = torch.zeros(rp * 2 * n_head * head_dim, dtype=torch.int16, device=dev)
    part = torch.empty(rows * n_head * n_split * (head_dim + 8), dtype=torch.float32, device=dev) if n_split > 1 else None
    L.check(L.lib().vaura_attention_step_probs(L.ptr(qkv_p), L.ptr(qkv2_p), L.ptr(rope), L.ptr(kcache), L.ptr(vcache), L.ptr(kscale),
                                               L.ptr(vscale), L.ptr(out), L.ptr(out_split), L.ptr(part), None, rows, n_head, head_dim,
                                               max_len, pos, n_split, plane_shift, kv_dtype, L.ptr(probs), pos0, n_steps, rows_out,
                                               L.current_stream()), "vaura_attention_step_probs")
    return out, out_split


def attention_map(probs: torch.Tensor, width: int, heads: str = "mean") -> torch.Tensor:
    """vaura_attention_map: reported weights (n_steps, n_rows, n_head, max_len) -> (n_rows, n_steps, width), the fixed-order mean over
    the heads, or with ``heads="all"`` (n_rows, n_head, n_steps, width)."""
    _cuda(probs)
    n_steps, n_rows, H, max_len = probs.shape
    out = torch.empty((n_rows, H, n_steps, width) if heads == "all" else (n_rows, n_steps, width), dtype=torch.float32, device=probs.device)
    L.check(L.lib().vaura_attention_map(L.ptr(probs), L.ptr(out), n_steps, n_rows, H, max_len, width, int(heads == "all"),
                                        L.current_stream()), "vaura_attention_map")
    return out


def attention_prefill(qkv_p: torch.Tensor, rope: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, attn: torch.Tensor,
                      attn_split: Optional[torch.Tensor], rows: int, n_head: int, head_dim: int, p0: int, n_pos: int, *,
                      kv_dtype: int = 0, plane_shift: int = 0, kscale: Optional[torch.Tensor] = None,
                      vscale: Optional[torch.Tensor] = None) -> None:
    """vaura_attention_prefill on a one-layer descriptor: rope + K / V append of the chunk [p0, p0 + n_pos), then its causal attention.
    qkv_p: packed rows of (n_pos * rows16, 3 D), position z of the chunk in rows z * rows16 ..; its q columns are rotated in place.
    attn (packed rows of (n_pos * rows16, D)) and attn_split (its split rows, or None) receive the output.  kscale / vscale (rows, n_head,
    max_len) uint8: the exponent bytes of the scaled e4m3 cache (kv_dtype = 3)."""
    _cuda(qkv_p, rope, kcache, vcache, attn, attn_split, kscale, vscale)
    d = L.Decoder()
    d.dims.n_layer, d.dims.n_head, d.dims.d_model = 1, n_head, n_head * head_dim
    d.rows, d.max_len, d.kv_dtype, d.plane_shift = rows, kcache.shape[-2], kv_dtype, plane_shift
    d.rope, d.ws_qkv, d.kcache, d.vcache = L.ptr(rope), L.ptr(qkv_p), L.ptr(kcache), L.ptr(vcache)
    d.ws_attn, d.ws_attn_split = L.ptr(attn), L.ptr(attn_split)
    d.kscale, d.vscale = L.ptr(kscale), L.ptr(vscale)
    L.check(L.lib().vaura_attention_prefill(C.byref(d), 0, p0, n_pos, L.current_stream()), "vaura_attention_prefill")


def sample(logits: torch.Tensor, batch: int, *, use_sampling: bool, temp: float = 1.0, top_k: int = 0,
           top_p: float = 0.0, cfg_scale: float = 1.0, noise: Optional[torch.Tensor] = None, seed: int = 0,
           clip_base: int = 0, step: int = 0, input_is_probs: bool = False) -> torch.Tensor:
    """logits (rows, K, V) with rows = batch (or 2*batch when cfg_scale > 1) -> tokens (batch, K, 1) int64.
    ``input_is_probs``: the rows already are probabilities (no temperature / softmax / CFG mix)."""
    _cuda(logits, noise)
    rows, K, V = logits.shape
    lg = logits.float().contiguous()
    sp = L.Sampling(int(use_sampling), float(temp), int(top_k), float(top_p), float(cfg_scale), int(seed), int(clip_base),
                    int(bool(input_is_probs)), 0)
    out = torch.zeros(batch, K, dtype=torch.int32, device=logits.device)
    nz = None if noise is None else noise.float().contiguous()
    L.check(L.lib().vaura_sample(L.ptr(lg), batch, K, V, C.byref(sp), L.ptr(nz), step, L.ptr(out), L.current_stream()),
            "vaura_sample")
    torch.cuda.current_stream().synchronize()
    return out.to(torch.int64)[..., None]


# The pattern ops come in three forms — per-clip lengths / the default delays / explicit delays —, and a call without lengths must not
# take the lengths' entry point: that one reads the array back and waits on the stream.  The choice is stated once, in the two
# functions below (enqueue only: no allocation, no wait), for the ops behind them and for the engine.
def pattern_build_into(codes: torch.Tensor, seq: torch.Tensor, special: int, delays, clip_T: Optional[torch.Tensor], stream: int) -> None:
    """codes (B, K, T) int32 -> seq (B, K, S) int32; ``delays`` None = the default 0..K-1, ``clip_T`` (B,) int32 = per-clip lengths."""
    (B, K, T), S = codes.shape, seq.shape[-1]
    a = (L.ptr(codes), L.ptr(seq), B, K, T)
    dl = L.delays_host(delays) if delays is not None else None
    if clip_T is not None:
        L.check(L.lib().vaura_pattern_build_clips(*a, S, special, dl, L.ptr(clip_T), stream), "vaura_pattern_build_clips")
    elif delays is None:
        L.check(L.lib().vaura_pattern_build(*a, special, stream), "vaura_pattern_build")
    else:
        L.check(L.lib().vaura_pattern_build_delays(*a, S, special, dl, stream), "vaura_pattern_build_delays")


def pattern_revert_into(seq: torch.Tensor, out: torch.Tensor, fill, pad, delays, clip_T: Optional[torch.Tensor], stream: int) -> None:
    """seq (B, K, S) -> out (B, K, T), both int32 (tokens) or both fp32 (values in the layout of seq): ``fill`` where the sequence holds
    no frame, ``pad`` in the frames past a clip's own end (``clip_T`` only)."""
    (B, K, S), T, f32 = seq.shape, out.shape[-1], out.dtype == torch.float32
    a = (L.ptr(seq), L.ptr(out), B, K, T, S, fill)
    dl = L.delays_host(delays) if delays is not None else None
    if clip_T is not None:
        name = "vaura_pattern_revert_clips_f32" if f32 else "vaura_pattern_revert_clips"
        L.check(getattr(L.lib(), name)(*a, pad, dl, L.ptr(clip_T), stream), name)
    elif f32 or delays is not None:        # (fp32 has no default-delays entry point of its own: NULL delays there)
        name = "vaura_pattern_revert_delays_f32" if f32 else "vaura_pattern_revert_delays"
        L.check(getattr(L.lib(), name)(*a, dl, stream), name)
    else:
        L.check(L.lib().vaura_pattern_revert(*a, stream), "vaura_pattern_revert")


def pattern_build(codes: torch.Tensor, special: int, delays: Optional[Sequence[int]] = None) -> torch.Tensor:
    """codes (B, K, T) -> pattern sequence (B, K, T + max(d) + 1); ``delays`` None = the default 0..K-1."""
    _cuda(codes)
    B, K, T = codes.shape
    d = None if delays is None else L.check_delays(delays, K)
    seq = torch.empty(B, K, T + (K if d is None else max(d) + 1), dtype=torch.int32, device=codes.device)
    pattern_build_into(codes.to(torch.int32).contiguous(), seq, special, d, None, L.current_stream())
    torch.cuda.current_stream().synchronize()
    return seq.to(codes.dtype)


def pattern_revert(seq: torch.Tensor, timesteps: int, fill: int, delays: Optional[Sequence[int]] = None) -> torch.Tensor:
    """pattern sequence (B, K, S) -> codes (B, K, timesteps); ``delays`` None = the default 0..K-1."""
    _cuda(seq)
    B, K, S = seq.shape
    d = None if delays is None else L.check_delays(delays, K)
    codes = torch.empty(B, K, timesteps, dtype=torch.int32, device=seq.device)
    pattern_revert_into(seq.to(torch.int32).contiguous(), codes, fill, 0, d, None, L.current_stream())
    torch.cuda.current_stream().synchronize()
    return codes.to(seq.dtype)


def split_rows(xp: torch.Tensor, rows: int, Cc: int, gain: Optional[torch.Tensor] = None, want_ss: bool = False):
    """packed rows fp32 -> (split rows int16 tensor, partial sums of squares or None)."""
    _cuda(xp, gain)
    rp = (rows + 15) // 16 * 16
    dst = torch.zeros(rp * 2 * Cc, dtype=torch.int16, device=xp.device)
    ss = torch.zeros((rp // 16) * (Cc // 16) * 16, dtype=torch.float32, device=xp.device) if want_ss else None
    L.check(L.lib().vaura_split_rows(L.ptr(xp), L.ptr(dst), L.ptr(gain), L.ptr(ss), rows, Cc, L.current_stream()),
            "vaura_split_rows")
    return dst, ss


def unsplit_rows(sp: torch.Tensor, rows: int, Cc: int) -> torch.Tensor:
    """split rows -> (2, rows, C) fp32 values of the hi and lo fp16 planes (layout check helper; plain tensor ops on the device)."""
    rp = (rows + 15) // 16 * 16
    f = sp.view(torch.float16).view(rp // 16, 2, Cc // 8, 16, 8).float()
    return f.permute(1, 0, 3, 2, 4).reshape(2, rp, Cc)[:, :rows]


def gemv_pair(wp: torch.Tensor, x_split: torch.Tensor, rows: int, N: int, K: int, epilogue: int = L.EPI_STORE,
              ss_in: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
              gain_out: Optional[torch.Tensor] = None, want_split: bool = False, want_ss: bool = False, eps: float = 1e-5,
              wdtype: int = L.W_H1, out_khalf2: Optional[torch.Tensor] = None):
    """Returns (out, out_split, ss_out); out is packed rows, or row-major (rows, N) for EPI_LOGITS."""
    _cuda(wp, x_split, ss_in, residual, gain_out)
    n_out = N // 2 if epilogue == L.EPI_SWIGLU else N
    rp = (rows + 15) // 16 * 16
    dev = x_split.device
    out = torch.zeros(rows, N, dtype=torch.float32, device=dev) if epilogue == L.EPI_LOGITS else \
        torch.zeros(rp * n_out, dtype=torch.float32, device=dev)
    osp = torch.zeros(rp * 2 * n_out, dtype=torch.int16, device=dev) if want_split else None
    oss = torch.zeros((rp // 16) * (n_out // 16) * 16, dtype=torch.float32, device=dev) if want_ss else None
    n_ss = 0 if ss_in is None else K // 16
    L.check(L.lib().vaura_gemv_pair(L.ptr(wp), wdtype, L.ptr(x_split), L.ptr(ss_in), n_ss, L.ptr(residual), L.ptr(out), L.ptr(out_khalf2), L.ptr(osp),
                                    L.ptr(gain_out), L.ptr(oss), rows, N, K, epilogue, eps, L.current_stream()),
            "vaura_gemv_pair")
    return out, osp, oss
