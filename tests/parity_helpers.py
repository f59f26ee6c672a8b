"""Helpers shared by the -m gpu parity tests (tests/ is on sys.path under pytest's rootdir conftest).

Token parity against a reference golden is STRICT (`assert_tokens_equal`): `torch.equal`, no exception.  The one golden that holds
a step whose reference margin is inside fp32 summation-order noise (configs[3], step 578, margin 5.5e-6) goes through
`assert_tokens_or_recorded_near_tie`, and what happened there is written down per storage.  Every comparison is recorded in the
session's `ParityReport` (conftest.py `parity_report`), which the session writes ONCE to gpurun_out/r06_parity.json."""
import json
import os

import torch


def _steps(K, T):
    """Sequence step that produced frame t of codebook k under the delay pattern (codebook_patterns.py:390-406): s = t + 1 + k."""
    return torch.arange(T)[None, :] + 1 + torch.arange(K)[:, None]


def token_diff_summary(tok, ref, margins=None, threshold_gap=None, first_step=1):
    """tok / ref (B, K, T).  `margins` (passes, B, K): the reference's own recorded decision margin per pass; pass i fills sequence
    step first_step + i (first_step = Tp + 1 with a prompt of Tp frames).  Returns a JSON-able dict."""
    B, K, T = ref.shape
    steps = _steps(K, T)
    out = {"tokens_equal": bool(torch.equal(tok, ref)), "clips": B, "clips_identical": 0, "frames": T,
           "token_agreement": float((tok == ref).float().mean()), "first_diff_step": None, "reference_margin_there": None,
           "threshold_gap_there": None, "identical_frames_before_first_diff": T}
    if margins is not None:
        out["reference_min_margin"] = float(margins.min())
    firsts = []
    for b in range(B):
        if torch.equal(tok[b], ref[b]):
            out["clips_identical"] += 1
            continue
        bad = tok[b] != ref[b]
        s = int(steps[bad].min())
        ks = [k for k in range(K) if bool((bad & (steps == s))[k].any())]
        m = min(float(margins[s - first_step, b, k]) for k in ks) if margins is not None else None
        g = min(float(threshold_gap[s - first_step, b, k]) for k in ks) if threshold_gap is not None else None
        firsts.append((s, b, ks, m, g))
    if firsts:
        s, b, ks, m, g = min(firsts)
        out.update(first_diff_step=s, first_diff_clip=b, first_diff_codebooks=ks, reference_margin_there=m, threshold_gap_there=g,
                   identical_frames_before_first_diff=max(0, s - K))
    return out


class ParityReport:
    """One entry per (golden, storage, launch shape) comparison of a session."""

    def __init__(self):
        self.entries = []

    def add(self, golden, storage, what, tok, ref, margins=None, threshold_gap=None, first_step=1, max_logit_err=None, **extra):
        e = {"golden": golden, "storage": storage, "what": what}
        e.update(token_diff_summary(tok, ref, margins, threshold_gap, first_step))
        if max_logit_err is not None:
            e["max_abs_logit_err"] = float(max_logit_err)
        e.update(extra)
        self.entries.append(e)
        return e

    def note_logit_err(self, golden, storage, err, **extra):
        for e in reversed(self.entries):
            if e["golden"] == golden and e["storage"] == storage:
                e["max_abs_logit_err"] = float(err)
                e.update(extra)
                return
        self.entries.append({"golden": golden, "storage": storage, "max_abs_logit_err": float(err), **extra})

    def summary_lines(self):
        for e in self.entries:
            yield (f"{e['golden']} [{e['storage']}] {e.get('what', '')}: tokens_equal={e.get('tokens_equal')} first_diff_step={e.get('first_diff_step')}"
                   f" margin_there={e.get('reference_margin_there')} max_abs_logit_err={e.get('max_abs_logit_err')}")

    def write(self, path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump({"what": "token / logit parity of the HIP decode loop against goldens produced by the reference itself "
                               "(tests/golden/make_golden.py), one entry per comparison of this pytest session",
                       "entries": self.entries}, f, indent=1)


def assert_tokens_equal(report, golden, storage, what, tok, ref, margins=None, threshold_gap=None, first_step=1, **extra):
    """STRICT: every token equals the reference's.  Recorded in the session report either way."""
    e = report.add(golden, storage, what, tok, ref, margins, threshold_gap, first_step, **extra)
    assert e["tokens_equal"], (f"{golden} [{storage}] {what}: first differs at step {e['first_diff_step']} (clip {e.get('first_diff_clip')}, "
                               f"codebooks {e.get('first_diff_codebooks')}); reference margin there {e['reference_margin_there']}, "
                               f"agreement {e['token_agreement']:.4f}")
    return e


def assert_tokens_or_recorded_near_tie(report, golden, storage, what, tok, ref, margins, tol, first_step=1, **extra):
    """For the ONE golden with a step inside summation-order noise (configs[3]: step 578, reference top-1 / top-2 margin 5.5e-6; the
    next smallest of its 888 steps is 6.2e-5): tokens must equal the reference's up to a first difference that sits on a step whose
    recorded reference margin is below `tol`.  Returns the report entry (identical_frames_before_first_diff = T when all equal)."""
    e = report.add(golden, storage, what, tok, ref, margins, None, first_step, near_tie_tolerance=tol, **extra)
    if not e["tokens_equal"]:
        m = e["reference_margin_there"]
        assert m is not None and m < tol, (f"{golden} [{storage}] {what}: first differs at step {e['first_diff_step']} where the reference's "
                                           f"margin is {m} >= {tol}")
        K, T = ref.shape[1], ref.shape[2]
        before = (_steps(K, T) < e["first_diff_step"])[None].expand_as(ref)
        assert torch.equal(tok[before], ref[before])
    return e


# ------------------------------------------------------------------------------------------------------------------
# Activation formats of the codec kernels (csrc/conv_kernels.h store_act_octet / store_pair4), decoded on the CPU for the op-level
# parity tests of tests/test_gpu_codec_stages.py.  tests/test_codec_stage_host.py checks these decoders themselves.

def pair_planes_to_f64(buf: torch.Tensor, rows: int, Cc: int):
    """(hi, lo) fp16 pair planes of a (rows, C) tensor -> (value = hi + lo, hi, lo), fp64 (rows, C) each.  Layout: per row C/8 octets
    of [plane hi | plane lo][8] halves — the half of channel c of row r sits at ((r * C/8 + c/8) * 2 + plane) * 8 + c % 8.  `buf`: any
    contiguous CPU tensor whose first rows * C * 4 bytes are the planes."""
    h = buf.contiguous().view(torch.uint8).reshape(-1)[: rows * Cc * 4].view(torch.float16).reshape(rows, Cc // 8, 2, 8).double()
    hi, lo = h[:, :, 0].reshape(rows, Cc), h[:, :, 1].reshape(rows, Cc)
    return hi + lo, hi, lo


def mx8_scale_offset(elems: int) -> int:
    return (elems + 15) & ~15


def mx8_to_f64(buf: torch.Tensor, rows: int, Cc: int):
    """Block-scaled e4m3 of a (rows, C) tensor -> (dequantised values fp64 (rows, C), scale bytes uint8 (rows, C/32)).  Layout: rows * C
    e4m3 bytes, row-major; at byte mx8_scale_offset(rows * C) one word of four E8M0 bytes per 128 channels of a row: the scale byte of
    the 32-channel block j of row r is byte (r * ceil(C/128) + j/4) * 4 + j % 4 there; value = e4m3 * 2^(byte - 127)."""
    raw = buf.contiguous().view(torch.uint8).reshape(-1)
    nsc = (Cc + 127) // 128
    off = mx8_scale_offset(rows * Cc)
    q = raw[: rows * Cc].view(torch.float8_e4m3fn).float().double().reshape(rows, Cc)
    sb = raw[off: off + rows * nsc * 4].reshape(rows, nsc * 4)[:, : Cc // 32].contiguous()
    scale = torch.ldexp(torch.ones(rows, Cc // 32, dtype=torch.float64), sb.to(torch.int32) - 127)
    return q * scale.repeat_interleave(32, dim=1), sb


def mx8_scale_bytes(x: torch.Tensor) -> torch.Tensor:
    """The E8M0 byte vaura_amd.quant's rule gives every 32-channel block of x (rows, C) fp32: the smallest power of two s = 2^(byte - 127)
    with amax <= 448 s, the byte clamped to [1, 253] -> uint8 (rows, C/32).  An all-zero block has no such smallest power: the kernel's
    integer form of the rule (mx8_scale_byte) lands on the clamp, byte 1, and so does this; every value of the block is 0 either way."""
    amax = x.detach().float().reshape(x.shape[0], -1, 32).abs().amax(dim=2)
    m, e = torch.frexp(amax)
    exp = torch.where(m <= 0.875, e - 9, e - 8).clamp(min=-126, max=126)
    return torch.where(amax > 0, exp + 127, torch.ones_like(exp)).to(torch.uint8)


def e4m3_step(q: torch.Tensor) -> torch.Tensor:
    """Spacing of the e4m3 grid at |q| (in units of the block scale): 2^-9 below 2^-6 (subnormals), else 2^(floor(log2 |q|) - 3)."""
    _, e = torch.frexp(q.abs().double().clamp(min=2.0 ** -6))        # |q| = m 2^e, m in [0.5, 1): floor(log2 |q|) = e - 1
    return torch.ldexp(torch.ones_like(q, dtype=torch.float64), e - 4)
