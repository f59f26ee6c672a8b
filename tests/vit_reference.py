"""fp64 restatement of every op of the Segment-AVCLIP extractor (oracle/avclip_oracle.py cites the reference's lines), the seeded input
builders and the acceptance bars of tests/test_gpu_avclip_ops.py.  Plain torch on the CPU: imported by the -m gpu module and by the CPU
self-checks in tests/test_vit_reference_host.py, which pin every function here to the fp32 oracle.

Every op takes the dtype of its input: called on `.double()` tensors it is the fp64 reference, on fp32 tensors the plain fp32 torch
restatement whose own error against fp64 (`e_ref`) scales the fp32-class bars.

Token rows of a sequence: row 0 = CLS, row 1 + f * n + i = patch (frame f, location i) — flatten(2) of the Conv3d output, order (f, h, w)
(video_model_builder.py:174-255).  QKV rows are [q | k | v], each (heads x 64) (vit_helper.py:98-119); q is scaled by 64^-0.5."""
import math

import torch

import parity_helpers as ph

D, HD, NF = 768, 64, 8
HEADS = D // HD
EPS = 1e-6            # video_model_builder.py:39, motionformer.py:177
U22, U23, U24, U25 = 2.0 ** -22, 2.0 ** -23, 2.0 ** -24, 2.0 ** -25
FLOOR = 3e-6          # tests/test_gpu_attention.py's floor for an fp32 kernel against fp64, relative to the case's scale
FACTOR = 4.0          # ... and its factor on e_ref


# ------------------------------------------------------------------------------------------------------------ pair planes
def split_pair(x32):
    """fp32 -> (hi, lo) fp16 with hi = fp16(x), lo = fp16(x - hi): the 22-bit operand format of every linear layer."""
    x32 = x32.float()
    hi = x32.half()
    return hi, (x32 - hi.float()).half()


def to_pair_planes(x32):
    """(rows, C) fp32 -> the pair layout as fp16 (rows, C/8, 2, 8): per row C/8 octets of [8 hi halves | 8 lo halves]."""
    rows, C = x32.shape
    hi, lo = split_pair(x32)
    return torch.stack([hi.reshape(rows, C // 8, 8), lo.reshape(rows, C // 8, 8)], dim=2).contiguous()


def pair_value64(x32):
    """The number a pair holds for x: hi + lo in fp64."""
    hi, lo = split_pair(x32)
    return hi.double() + lo.double()


def decode_pair(buf, rows, C):
    """Pair planes read back from the device -> fp64 values (rows, C)."""
    return ph.pair_planes_to_f64(buf, rows, C)[0]


def pair_repr_err(y64):
    """Representation error of y in (hi, lo) fp16 planes: 2^-22 |y| + 2^-25 (fp16 subnormal spacing 2^-24 on the lo plane)."""
    return U22 * y64.abs() + U25


# ---------------------------------------------------------------------------------------------------------------- tokens
def patch_gather(frames, pt, ps):
    """frames (n, C, T, H, W) -> (n * T/pt * H/ps * W/ps, C * pt * ps * ps): row = token (tf, ph, pw), column = (c, dt, dy, dx), the
    flattening order of the Conv3d weight (D, C, pt, ps, ps) — a stride == kernel convolution is this matrix times weight.reshape(D, -1)^T
    (vit_helper.py:543-548)."""
    n, C, T, H, W = frames.shape
    x = frames.reshape(n, C, T // pt, pt, H // ps, ps, W // ps, ps)
    return x.permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(n * (T // pt) * (H // ps) * (W // ps), C * pt * ps * ps)


def embed(x, cls, pos, temp, nf, n):
    """x (n_seg, 1 + nf n, D) with the patch embeddings in rows 1..; cls (D), pos (1 + n, D), temp (nf, D).  Row 0 = cls + pos[0], row
    1 + f n + i = x + (pos[1 + i] + temp[f]) ('separate' positional embedding, video_model_builder.py:240-249).  In fp32 this is the
    kernel's order of the two additions."""
    total = pos[1:].repeat(nf, 1) + temp.repeat_interleave(n, 0)
    out = x.clone()
    out[:, 0] = cls + pos[0]
    out[:, 1:] = x[:, 1:] + total
    return out


# ------------------------------------------------------------------------------------------------------------- LayerNorm
def layernorm(x, w, b, eps=EPS):
    """(x - mean) / sqrt(biased var + eps) * w + b over the last dim (F.layer_norm)."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w + b


LN_MEAN_ROUNDINGS = 22


def ln_constant_row_floor(x, w, eps=EPS):
    """A-priori error of an fp32 LayerNorm on a CONSTANT row x = c, per row (rows, 1), absolute.  The exact output is the bias.  The
    kernel's mean passes every value through at most 22 fp32 roundings — 15 additions in its lane (16 values, the first addition to 0 is
    exact), 6 butterfly steps across the wave, one division — each at most 2^-24 of a partial sum that is at most the total (all terms
    have one sign), so |mean - c| <= 22 x 2^-24 |c|.  x - mean is then the same nonzero value in every channel, the variance is its
    square (negligible against eps), and the output moves by |w| |mean - c| / sqrt(eps).  This replaces the 3e-6 floor on constant rows
    only: torch's pairwise sum of equal values can be exact (e_ref = 0 on a single row) where no other order is."""
    return LN_MEAN_ROUNDINGS * U24 * x.double().abs().amax(dim=1, keepdim=True) * float(w.abs().max()) / math.sqrt(eps)


def ln_map1_rows(n_seg, nf, n):
    """Row maps of the final norm (motionformer.py:311-330): (src, dst) index tensors — the patch rows of sequences of 1 + nf n rows, in
    order, and their rows in (segment, frame) sequences of 1 + n rows whose slot 0 is left for the aggregation CLS token."""
    seg = torch.arange(n_seg)[:, None, None]
    f = torch.arange(nf)[None, :, None]
    i = torch.arange(n)[None, None, :]
    src = seg * (1 + nf * n) + 1 + f * n + i
    dst = (seg * nf + f) * (n + 1) + 1 + i
    return src.reshape(-1), dst.reshape(-1)


# ------------------------------------------------------------------------------------------------------------- attention
def _heads(t):
    """(..., rows, H * 64) -> (..., H, rows, 64)"""
    return t.reshape(*t.shape[:-1], t.shape[-1] // HD, HD).transpose(-2, -3)


def _unheads(t):
    return t.transpose(-2, -3).reshape(*t.shape[:-3], t.shape[-2], t.shape[-3] * HD)


def qkv_attn(q, k, v):
    """softmax((q 64^-0.5) k^T) v (vit_helper.py:34-44, 119)."""
    return torch.softmax((q * 0.125) @ k.transpose(-1, -2), dim=-1) @ v


def cls_attention(qkv):
    """qkv (n_seq, Lseq, 3 D') -> (n_seq, D'): the query of row 0 of every sequence over all its rows."""
    q, k, v = (_heads(t) for t in qkv.chunk(3, dim=-1))            # (n_seq, H, L, 64)
    return _unheads(qkv_attn(q[:, :, :1], k, v))[:, 0]


def _pattern_kv(t, nf, n, mode):
    """t (n_seg, H, 1 + nf n, 64) -> keys / values of every patch query: (n_seg, H, groups, 1 + group size, 64), CLS first.
    'time': group = location i, members the nf frames; 'space': group = frame f, members the n locations."""
    ns, H = t.shape[:2]
    p = t[:, :, 1:].reshape(ns, H, nf, n, HD)
    if mode == "time":
        p = p.transpose(2, 3)
    c = t[:, :, :1, None].expand(ns, H, p.shape[2], 1, HD)
    return torch.cat((c, p), dim=3)


def pattern_attention(qkv, nf, n, mode):
    """qkv (n_seg, 1 + nf n, 3 D') -> (n_seg, nf n, D'): the outputs of the patch rows 1.. under DividedAttention's 'time' / 'space'
    pattern (vit_helper.py:98-172): keys = CLS + the tokens of the query's own location / frame."""
    q, k, v = (_heads(t) for t in qkv.chunk(3, dim=-1))
    ns, H = q.shape[:2]
    qg = q[:, :, 1:].reshape(ns, H, nf, n, HD)
    if mode == "time":
        qg = qg.transpose(2, 3)
    o = qkv_attn(qg, _pattern_kv(k, nf, n, mode), _pattern_kv(v, nf, n, mode))
    if mode == "time":
        o = o.transpose(2, 3)
    return _unheads(o.reshape(ns, H, nf * n, HD))


def cls_vscale(qkv):
    """max |v| over the keys of each output element of cls_attention: (n_seq, D'), constant over a head's 64 channels."""
    v = _heads(qkv.chunk(3, dim=-1)[2])
    return v.abs().amax(dim=(2, 3)).repeat_interleave(HD, dim=1)


def pattern_vscale(qkv, nf, n, mode):
    """... of pattern_attention: (n_seg, nf n, D')."""
    v = _pattern_kv(_heads(qkv.chunk(3, dim=-1)[2]), nf, n, mode)            # (ns, H, G, 1 + m, 64)
    ns, H, G = v.shape[:3]
    a = v.abs().amax(dim=(3, 4))[..., None].expand(ns, H, G, (nf * n) // G)
    a = a.transpose(2, 3) if mode == "time" else a
    return a.reshape(ns, H, nf * n).transpose(1, 2).repeat_interleave(HD, dim=2)


def pattern_abs_qk(qkv, nf, n, mode):
    """max over a query's keys of 0.125 sum_i |q_i| |k_i|: (n_seg, nf n, D'), constant over a head's channels.  The scale of a score's
    error when q and k carry 22 bits each."""
    q, k, _ = (_heads(t).abs() for t in qkv.double().chunk(3, dim=-1))
    ns, H = q.shape[:2]
    qg = q[:, :, 1:].reshape(ns, H, nf, n, HD)
    if mode == "time":
        qg = qg.transpose(2, 3)
    s = (0.125 * qg @ _pattern_kv(k, nf, n, mode).transpose(-1, -2)).amax(dim=-1)      # (ns, H, G, m)
    if mode == "time":
        s = s.transpose(2, 3)
    return s.reshape(ns, H, nf * n).transpose(1, 2).repeat_interleave(HD, dim=2)


def pair_attention_apriori(qkv, nf, n, mode):
    """A-priori error of attention computed on (hi, lo) fp16 operands, per output element, in units of the element's max |v|:
         2 x [3 x 2^-22 x 0.125 sum_i |q_i| |k_i|]  +  3 x 2^-22.
    A score is three fp16 products (hi hi + hi lo + lo hi, lo lo dropped) of two 22-bit operands: at most 3 x 2^-22 of its sum of
    magnitudes.  Scores all within +-e of the exact ones move every softmax weight by a factor inside exp(+-2 e), so an output by at most
    2 e max |v|.  The second term: p and v are 22-bit operands of the second product in the same three-product form."""
    return 2.0 * 3.0 * U22 * pattern_abs_qk(qkv, nf, n, mode) + 3.0 * U22


# ----------------------------------------------------------------------------------------------------------------- linear
def linear(x, w, b, res=None):
    y = x @ w.transpose(-1, -2) + b
    return y if res is None else y + res


def gelu(x):
    """Exact GELU x Phi(x) = 0.5 x (1 + erf(x / sqrt 2)) (nn.GELU, vit_helper.py:475-498), written 0.5 x erfc(-x / sqrt 2): the same
    function, without the cancellation of 1 + erf on the negative side."""
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


# ------------------------------------------------------------------------------------------------------------------ bars
def fp32_bar(e_ref, floor=FLOOR):
    """tests/test_gpu_attention.py's rule: err <= max(floor, 4 e_ref), both relative to the case's scale."""
    return max(floor, FACTOR * e_ref)


# -------------------------------------------------------------------------------------------------------- input builders
ATTN_FAMILIES = ("flat", "peak30", "first", "last", "big80", "ones")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def attention_inputs(n_seq, Lseq, family, seed, peak_rows=None, heads=HEADS):
    """qkv (n_seq, Lseq, 3 heads 64) fp32 for one softmax class.  Every query of a (sequence, head) is u + 0.05 noise with u a sign vector
    (0.125 u.u = 8), so a key c u / 8 scores c (+- 0.05 c) against ALL of them:
      flat     keys 0.05 N(0, 1): scores ~ 0.03, near-uniform weights (what synth.avclip_state_dict gives)
      peak30   flat, and the keys of `peak_rows` are 30 u / 8: one score of +30 in every key set that holds one such row
      first    flat, and row 0 (the CLS key, first of every key set) is 12 u / 8
      last     flat, and `peak_rows` (callers pass the LAST key of each key set) are 12 u / 8
      big80    keys c u / 8 with c uniform in [-80, 80]: scores of magnitude ~80, the maximum wherever it falls
      ones     flat with every v = 1 (the output must be 1)
    v = N(0, 1) (x 100 regions are applied by the caller with `scale_v`)."""
    g = gen(seed)
    Dd = heads * HD
    u = (torch.randint(0, 2, (n_seq, 1, Dd), generator=g) * 2 - 1).float()
    q = u + 0.05 * torch.randn(n_seq, Lseq, Dd, generator=g)
    k = 0.05 * torch.randn(n_seq, Lseq, Dd, generator=g)
    v = torch.randn(n_seq, Lseq, Dd, generator=g)
    if family == "peak30":
        k[:, peak_rows] = 30.0 / 8.0 * u
    elif family == "first":
        k[:, 0] = 12.0 / 8.0 * u[:, 0]
    elif family == "last":
        k[:, peak_rows] = 12.0 / 8.0 * u
    elif family == "big80":
        c = (torch.rand(n_seq, Lseq, heads, generator=g) * 160.0 - 80.0).repeat_interleave(HD, dim=2)
        k = c / 8.0 * u
    elif family == "ones":
        v = torch.ones_like(v)
    else:
        assert family == "flat", family
    return torch.cat((q, k, v), dim=-1).contiguous()


def scale_v(qkv, rows, factor=100.0):
    """v of `rows` (index or slice into dim 1, or a (seq index, row index) tuple) x factor, in place."""
    Dd = qkv.shape[-1] // 3
    if isinstance(rows, tuple):
        qkv[rows[0], rows[1], 2 * Dd:] *= factor
    else:
        qkv[:, rows, 2 * Dd:] *= factor
    return qkv


def last_key_rows(nf, n, mode):
    """Rows (of a 1 + nf n sequence) that are the LAST key of a key set: 'time' the last frame's, 'space' location n - 1 of every frame."""
    if mode == "time":
        return 1 + (nf - 1) * n + torch.arange(n)
    return 1 + torch.arange(nf) * n + (n - 1)


LN_FAMILIES = ("ordinary", "mean100", "constant", "outlier")


def ln_inputs(rows, family, seed, Dd=D):
    """x (rows, D) fp32: ordinary N(0, 1) rows of varying scale; mean 100 with std 1e-2; constant rows (variance 0: eps decides); one
    channel x 1e4.  Gain U(0.5, 1.5) with a few negative entries, bias N(0, 0.5)."""
    g = gen(seed)
    x = torch.randn(rows, Dd, generator=g)
    if family == "ordinary":
        x = x * (0.1 + 3.0 * torch.rand(rows, 1, generator=g)) + torch.randn(rows, 1, generator=g)
    elif family == "mean100":
        x = 100.0 + 1e-2 * x
    elif family == "constant":
        x = (torch.randn(rows, 1, generator=g) * 3.0).expand(rows, Dd).contiguous()
    elif family == "outlier":
        ch = torch.randint(0, Dd, (rows,), generator=g)
        x[torch.arange(rows), ch] *= 1e4
    else:
        raise AssertionError(family)
    w = 0.5 + torch.rand(Dd, generator=g)
    w[::97] *= -1.0
    b = 0.5 * torch.randn(Dd, generator=g)
    return x.contiguous(), w, b


def gelu_sweep():
    """fp32 arguments of the GELU check, a multiple of 3072 values: a dense grid on [-12, 12], +-0, the neighbourhood of -5.5 and below
    (where 0.5 x (1 + erff) rounds to 0), values past 6 (the end of the kernel's fit range in t = |x| / sqrt 2 is x = 8.49) up to 40."""
    parts = [torch.linspace(-12.0, 12.0, 20001), torch.tensor([0.0, -0.0]),
             torch.linspace(-6.5, -5.0, 3001), torch.linspace(-14.0, -5.5, 2001),
             torch.linspace(6.0, 9.0, 2001), torch.linspace(8.4, 8.6, 501), torch.tensor([10.0, 13.0, 20.0, 40.0, -20.0, -40.0])]
    x = torch.cat(parts).float()
    pad = (-x.numel()) % 3072
    return torch.cat((x, torch.linspace(-1.0, 1.0, pad).float())).contiguous()


def gelu_allowed(x64, y64):
    """The kernel's stated bound 1.3e-7 max(1, |x|) plus the pair planes' representation error 2^-22 |y| + 2^-25."""
    return 1.3e-7 * x64.abs().clamp(min=1.0) + U22 * y64.abs() + U25
