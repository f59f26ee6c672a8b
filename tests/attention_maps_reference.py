"""CPU restatements for the attention maps of generate() (tests/test_attention_maps_host.py, tests/test_gpu_attention_maps.py): the
fixed-order head mean of csrc/step.hip ``attention_map_kernel`` in numpy, a teacher-forced restatement of every layer's self-attention
weights in fp64 or fp32 built from oracle.decoder_oracle's pieces, the plumbing-fault distance ``d_min`` computed from the fp64
restatement alone, and a greedy CPU decode that gives the host test tokens to compute it on.  Plain torch / numpy, no device."""
import copy
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.decoder_oracle import CachedDecoder, DecoderOracle, rmsnorm

SPECIAL = 1024


# ------------------------------------------------------------------------------------------------------- attention_map_kernel
def attention_map_np(probs: np.ndarray, width: int, heads: str = "mean") -> np.ndarray:
    """probs (n_steps, n_rows, H, max_len) fp32 -> (n_rows, n_steps, width): ((p_0 + p_1) + .. + p_{H-1}) * (1 / H), every operation
    in fp32 and in that order; heads="all": (n_rows, H, n_steps, width), a transposed copy."""
    probs = np.asarray(probs, dtype=np.float32)
    if heads == "all":
        return np.ascontiguousarray(probs[..., :width].transpose(1, 2, 0, 3))
    acc = probs[:, :, 0, :width].copy()
    for h in range(1, probs.shape[2]):
        acc = (acc + probs[:, :, h, :width]).astype(np.float32)
    return np.ascontiguousarray((acc * np.float32(1.0 / probs.shape[2])).astype(np.float32).transpose(1, 0, 2))


def mean_of_all_np(all_heads: np.ndarray) -> np.ndarray:
    """(B, H, n, W) fp32, the "all" map -> the "mean" map (B, n, W) in the kernel's order."""
    a = np.asarray(all_heads, dtype=np.float32)
    acc = a[:, 0].copy()
    for h in range(1, a.shape[1]):
        acc = (acc + a[:, h]).astype(np.float32)
    return (acc * np.float32(1.0 / a.shape[1])).astype(np.float32)


# ------------------------------------------------------------------------------------------------- teacher-forced restatement
def effective_sd(sd, wdtype: str):
    """The state dict whose streamed matrices hold the real numbers the storage ``wdtype`` holds ("f32": the dict itself)."""
    if wdtype == "f32":
        return sd
    from vaura_amd.engine import h_effective_weight
    from vaura_amd.synth import is_streamed_weight
    planes = {"h1": 1, "h2": 2}[wdtype]
    return {k: (h_effective_weight(v, planes) if is_streamed_weight(k) else v) for k, v in sd.items()}


def _oracle_in(orc: DecoderOracle, dtype) -> DecoderOracle:
    o = copy.copy(orc)
    o.sd = {k: v.to(dtype) for k, v in orc.sd.items()}
    o.tok_w, o.tok_b = [w.to(dtype) for w in orc.tok_w], [b.to(dtype) for b in orc.tok_b]
    o.head_w, o.rope = orc.head_w.to(dtype), orc.rope.to(dtype)       # the fp32 table, widened: what the kernels multiply by
    return o


def _rope(x, tab):
    """oracle.decoder_oracle.apply_rope in the dtype of x (that one computes in fp32): x (R, L, H, hd), tab (L, hd/2, 2)."""
    xs = x.reshape(*x.shape[:-1], -1, 2)
    c, s = tab[None, :, None, :, 0], tab[None, :, None, :, 1]
    return torch.stack([xs[..., 0] * c - xs[..., 1] * s, xs[..., 1] * c + xs[..., 0] * s], dim=-1).flatten(3)


def cache_values(x: torch.Tensor, kv_dtype: str) -> torch.Tensor:
    """x (..., 96): the numbers a K / V cache of storage ``kv_dtype`` hands back for the vectors x, in the dtype of x — the weights are
    DEFINED on the widened stored keys (include/vaura_hip.h vaura_decoder_ext4), and every later layer sees the stored values too.
    "f32": x; "f16": one rounding to fp16; "f8s": the scaled e4m3 rule of tests/kv_f8s_reference.py (the device stores its fp32 k / v)."""
    if kv_dtype == "f32":
        return x
    if kv_dtype == "f16":
        return x.float().half().to(x.dtype)
    if kv_dtype == "f8s":
        import kv_f8s_reference as F8
        return F8.cache64(x.float()).to(x.dtype)
    raise ValueError(kv_dtype)


@torch.no_grad()
def layer_probs(orc: DecoderOracle, seq_in: torch.Tensor, cond: torch.Tensor, dtype=torch.float64, kv_dtype: str = "f32") -> torch.Tensor:
    """The causal self-attention weights of every layer for the teacher-forced positions ``seq_in`` (R, K, L) int64 under ``cond``
    (R, Tv, 768): (n_layer, R, H, L, L) in ``dtype``, row i = query position i, exact zeros right of the diagonal.  The decoder of
    oracle.decoder_oracle (forward_full) with the weights widened to ``dtype``, keeping the weights of each layer on the way; rotated
    k and v pass through ``cache_values`` (the storage of the K / V cache), everything else stays in ``dtype``."""
    o = _oracle_in(orc, dtype)
    R, _, L = seq_in.shape
    tok = o.token_embedding(seq_in)
    cp = o.cond_for_positions(o.cond_projection(cond.to(dtype)), torch.arange(L))
    h = torch.cat([cp, tok], dim=-1)
    tab = o.rope[:L]
    mask = torch.ones(L, L, dtype=torch.bool).tril()
    out = []
    for l in range(o.L):
        p = f"layers.{l}."
        x = rmsnorm(h, o.sd[p + "attention_norm.weight"], o.eps)
        q, k, v = F.linear(x, o.sd[p + "attention.wqkv.weight"]).split([o.D, o.D, o.D], dim=-1)
        q = _rope(q.view(R, L, o.H, o.hd), tab).transpose(1, 2)
        k = _rope(k.view(R, L, o.H, o.hd), tab).transpose(1, 2)
        v = v.view(R, L, o.H, o.hd).transpose(1, 2)
        k, v = cache_values(k, kv_dtype), cache_values(v, kv_dtype)
        s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(o.hd)
        pr = torch.softmax(s.masked_fill(~mask, -math.inf), dim=-1)
        out.append(pr)
        a = torch.matmul(pr, v).transpose(1, 2).reshape(R, L, o.D)
        h = h + F.linear(a, o.sd[p + "attention.wo.weight"])
        h = h + o.feed_forward(rmsnorm(h, o.sd[p + "ffn_norm.weight"], o.eps), l)
    return torch.stack(out)


def map_all(probs_l: torch.Tensor, start: int) -> torch.Tensor:
    """One layer's weights (R, H, L, L), L = S - 1 -> the "all" map (R, H, S - start, S - 1): row i is the step at position start - 1 + i."""
    return probs_l[:, :, start - 1:, :]


def rel_err(got, ref) -> float:
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def d_min(cond_layers: torch.Tensor, null_layers, layer: int, start: int):
    """The smallest max |wrong - right| over the plumbing faults that matter, on the per-head ("all") map of ``layer`` — the object the
    error is measured on; the mean map is its exact fixed-order mean, where the 16 heads' differences partly cancel —, from the fp64
    restatement alone: another layer, the neighbouring step, another clip's row, the null-condition row.  Per clip, then the smallest.
    cond_layers / null_layers: ``layer_probs`` of the conditional / null rows (null_layers None: no such rows).  -> (d_min, {fault: d})"""
    right = map_all(cond_layers[layer], start)                          # (B, H, n, W)
    B = right.shape[0]
    per_clip = lambda wrong: float((wrong - right).abs().flatten(1).max(dim=1).values.min())
    faults = {"layer": min(per_clip(map_all(cond_layers[l], start)) for l in range(cond_layers.shape[0]) if l != layer),
              "step": float((right[:, :, 1:] - right[:, :, :-1]).abs().flatten(1).max(dim=1).values.min()),
              "clip": min(float((right[a] - right[b]).abs().max()) for a in range(B) for b in range(B) if a != b)}
    if null_layers is not None:
        faults["null"] = per_clip(map_all(null_layers[layer], start))
    return min(faults.values()), faults


# ------------------------------------------------------------------------------------------------------- tokens for the host test
@torch.no_grad()
def greedy_sequence(orc: DecoderOracle, feats: torch.Tensor, T: int, cfg_scale: float, delays, prompt=None) -> torch.Tensor:
    """A greedy CPU decode with the fp32 oracle: the pattern sequence (B, K, S) int64 of T timesteps under ``delays``, the special token
    in every slot without a timestep.  CFG as the reference mixes it (uncond + (cond - uncond) * scale) when cfg_scale > 1."""
    B, K = feats.shape[0], orc.K
    S = T + max(delays) + 1
    seq = torch.full((B, K, S), SPECIAL, dtype=torch.int64)
    Tp = 0 if prompt is None else prompt.shape[-1]
    for q, d in enumerate(delays):
        seq[:, q, 1 + d:1 + d + T] = -1
        if Tp:
            seq[:, q, 1 + d:1 + d + Tp] = prompt[:, q]
    cfg = cfg_scale > 1.0
    cond = torch.cat([feats, orc.null_condition(feats)]) if cfg else feats
    dec = CachedDecoder(orc, cond, S)
    for p in range(S - 1):
        tok = seq[:, :, p]
        assert int(tok.min()) >= 0
        x = dec.step(torch.cat([tok, tok]) if cfg else tok)
        if cfg:
            x = x[B:] + (x[:B] - x[B:]) * cfg_scale
        nxt = x.argmax(-1)
        seq[:, :, p + 1] = torch.where(seq[:, :, p + 1] == -1, nxt, seq[:, :, p + 1])
    return seq
