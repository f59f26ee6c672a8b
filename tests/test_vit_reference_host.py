"""CPU checks of tests/vit_reference.py, the fp64 reference of tests/test_gpu_avclip_ops.py: every op against the fp32 function of
oracle/avclip_oracle.py that restates the reference's lines, the input builders against what they claim, and the a-priori bars against
the size of the errors they are meant to catch.  No GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import parity_helpers as ph
import vit_reference as R
from oracle import avclip_oracle as ao

F32 = 2e-5        # fp32 evaluation against fp64 on O(1) values with sums over <= 1536 terms


def _close(a32, b64, tol=F32):
    scale = max(1.0, float(b64.abs().max()))
    err = float((a32.double() - b64).abs().max())
    assert err <= tol * scale, f"{err:.3e} > {tol * scale:.3e}"


def test_pair_planes_round_trip_and_layout():
    x = torch.randn(5, 32, generator=R.gen(1)) * torch.tensor([1e-6, 1e-3, 1.0, 100.0, 1e4])[:, None]
    planes = R.to_pair_planes(x)
    assert planes.shape == (5, 4, 2, 8) and planes.dtype == torch.float16
    val, hi, lo = ph.pair_planes_to_f64(planes, 5, 32)
    assert torch.equal(hi, x.half().double()) and torch.equal(val, R.pair_value64(x))
    assert bool(((val - x.double()).abs() <= R.pair_repr_err(x.double())).all())
    # channel c of row r sits at ((r * C/8 + c/8) * 2 + plane) * 8 + c % 8
    flat = planes.reshape(-1)
    assert float(flat[((3 * 4 + 2) * 2 + 0) * 8 + 5]) == float(x[3, 21].half())
    assert float(flat[((3 * 4 + 2) * 2 + 1) * 8 + 5]) == float((x[3, 21] - x[3, 21].half().float()).half())


def test_patch_gather_is_the_conv3d_of_the_oracle():
    g = R.gen(2)
    frames = torch.randn(2, 3, 4, 32, 32, generator=g)
    w = torch.randn(24, 3, 2, 16, 16, generator=g) * 0.02
    b = torch.randn(24, generator=g)
    conv = F.conv3d(frames, w, b, stride=(2, 16, 16)).flatten(2).transpose(1, 2)                 # avclip_oracle.tokens
    P = R.patch_gather(frames.double(), 2, 16)
    assert P.shape == (2 * 2 * 2 * 2, 1536)
    _close(conv.reshape(-1, 24), R.linear(P, w.reshape(24, -1).double(), b.double()))
    # one element by hand: segment 1, token (tf 1, ph 0, pw 1), column (c 2, dt 1, dy 3, dx 7)
    assert float(P[8 + 4 + 1, ((2 * 2 + 1) * 16 + 3) * 16 + 7]) == float(frames[1, 2, 3, 3, 16 + 7])


def test_embed_matches_the_oracle_tokens():
    g = R.gen(3)
    f, n, Dd = 2, 4, 24
    frames = torch.randn(2, 3, 4, 32, 32, generator=g)
    sd = {"patch_embed_3d.proj.weight": torch.randn(Dd, 3, 2, 16, 16, generator=g) * 0.02, "patch_embed_3d.proj.bias": torch.randn(Dd, generator=g),
          "cls_token": torch.randn(1, 1, Dd, generator=g), "pos_embed": torch.randn(1, n + 1, Dd, generator=g),
          "temp_embed": torch.randn(1, f, Dd, generator=g)}
    want, n_o = ao.tokens(frames, sd, f)
    assert n_o == n
    x = torch.zeros(2, 1 + f * n, Dd, dtype=torch.float64)
    x[:, 1:] = R.linear(R.patch_gather(frames.double(), 2, 16), sd["patch_embed_3d.proj.weight"].reshape(Dd, -1).double(),
                        sd["patch_embed_3d.proj.bias"].double()).reshape(2, f * n, Dd)
    _close(want, R.embed(x, sd["cls_token"][0, 0].double(), sd["pos_embed"][0].double(), sd["temp_embed"][0].double(), f, n))


@pytest.mark.parametrize("family", R.LN_FAMILIES)
def test_layernorm_matches_the_oracle(family):
    x, w, b = R.ln_inputs(7, family, 4, Dd=96)
    want = ao._ln(x, {"weight": w, "bias": b}, "")
    got = R.layernorm(x.double(), w.double(), b.double())
    # fp32 F.layer_norm of a row of mean m and deviation s carries ~2^-24 |m| / s of relative error: 1e-3 on the mean-100 rows
    tol = {"mean100": 5e-3, "outlier": 1e-4}.get(family, F32)
    _close(want, got, tol)
    if family == "constant":           # variance 0: the output is the bias exactly
        assert torch.equal(got, b.double().expand_as(got))


def test_ln_row_maps():
    src, dst = R.ln_map1_rows(2, 8, 5)
    assert src.numel() == dst.numel() == 80
    assert 0 not in src.tolist() and 41 not in src.tolist() and src.max() == 81             # the two CLS rows are never read
    assert sorted(set(range(2 * 8 * 6)) - set(dst.tolist())) == [6 * j for j in range(16)]     # slot 0 of the 16 sequences
    assert int(src[5 * 3 + 2]) == 1 + 17 and int(dst[5 * 3 + 2]) == 3 * 6 + 1 + 2
    assert int(src[40]) == 42 and int(dst[40]) == 8 * 6 + 1


def _divided(mode, seed):
    """ao.divided_attention with an identity projection against the three patterns of the reference on the same fp32 qkv."""
    g = R.gen(seed)
    b, f, n, heads = 2, 3, 4, 2
    Dd = heads * R.HD
    x = torch.randn(b, 1 + f * n, Dd, generator=g)
    sd = {"qkv.weight": torch.randn(3 * Dd, Dd, generator=g) * 0.15, "qkv.bias": torch.randn(3 * Dd, generator=g) * 0.1,
          "proj.weight": torch.eye(Dd), "proj.bias": torch.zeros(Dd)}
    want = ao.divided_attention(x, sd, "", heads, mode, n, f)
    qkv = ao._lin(x, sd, "qkv.").double()
    got = torch.cat((R.cls_attention(qkv)[:, None], R.pattern_attention(qkv, f, n, mode)), dim=1)
    return want, got, qkv


@pytest.mark.parametrize("mode", ["time", "space"])
def test_attention_patterns_match_the_oracle(mode):
    want, got, qkv = _divided(mode, 5)
    _close(want, got)
    # and the key sets by hand: patch (f 1, i 2) of sequence 1, head 1
    f, n = 3, 4
    q, k, v = (t[1, :, R.HD:2 * R.HD] for t in qkv.chunk(3, dim=-1))
    keys = [0] + ([1 + ff * n + 2 for ff in range(f)] if mode == "time" else [1 + 1 * n + i for i in range(n)])
    o = R.qkv_attn(q[1 + n + 2][None], k[keys], v[keys])[0]
    assert float((o - got[1, 1 + n + 2, R.HD:2 * R.HD]).abs().max()) < 1e-12
    # the scale helpers are per key set
    vs = R.pattern_vscale(qkv, f, n, mode)
    assert float(vs[1, n + 2, R.HD]) == float(v[keys].abs().max())
    aq = R.pattern_abs_qk(qkv, f, n, mode)
    assert abs(float(aq[1, n + 2, R.HD]) - float((0.125 * q[1 + n + 2].abs() @ k[keys].abs().T).max())) < 1e-12


def test_aggregation_attention_matches_the_oracle():
    """spatial_aggregate with unit norms, an identity out_proj and a zero MLP output returns cls + attention(CLS row)."""
    g = R.gen(6)
    b, n, heads = 3, 5, 2
    Dd = heads * R.HD
    p = "spatial_attn_agg."
    sd = {p + "cls_token": torch.randn(1, 1, Dd, generator=g), p + "norm1.weight": torch.ones(Dd), p + "norm1.bias": torch.zeros(Dd),
          p + "norm2.weight": torch.ones(Dd), p + "norm2.bias": torch.zeros(Dd),
          p + "self_attn.in_proj_weight": torch.randn(3 * Dd, Dd, generator=g) * 0.15, p + "self_attn.in_proj_bias": torch.randn(3 * Dd, generator=g) * 0.1,
          p + "self_attn.out_proj.weight": torch.eye(Dd), p + "self_attn.out_proj.bias": torch.zeros(Dd),
          p + "linear1.weight": torch.randn(8, Dd, generator=g), p + "linear1.bias": torch.zeros(8),
          p + "linear2.weight": torch.zeros(Dd, 8), p + "linear2.bias": torch.zeros(Dd)}
    y = torch.randn(b, n, Dd, generator=g)
    want = ao.spatial_aggregate(y, sd, heads) - sd[p + "cls_token"][0]
    x = torch.cat((sd[p + "cls_token"].expand(b, -1, -1), y), dim=1).double()
    z = R.layernorm(x, torch.ones(Dd, dtype=torch.float64), torch.zeros(Dd, dtype=torch.float64))
    qkv = R.linear(z, sd[p + "self_attn.in_proj_weight"].double(), sd[p + "self_attn.in_proj_bias"].double())
    _close(want, R.cls_attention(qkv))


def test_linear_and_gelu_match_torch():
    g = R.gen(7)
    x, w, b, r = torch.randn(9, 64, generator=g), torch.randn(96, 64, generator=g), torch.randn(96, generator=g), torch.randn(9, 96, generator=g)
    _close(F.linear(x, w, b) + r, R.linear(x.double(), w.double(), b.double(), r.double()))
    t = torch.linspace(-12, 12, 4001, dtype=torch.float64)
    y = R.gelu(t)
    _close(F.gelu(t.float()), y, 1e-6)
    direct = 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))
    assert float((direct - y).abs().max()) < 1e-14
    # the negative tail does not cancel: gelu(-8) = -8 Phi(-8) = -4.976e-15, to 1e-3 relative
    assert abs(float(R.gelu(torch.tensor(-8.0, dtype=torch.float64))) / -4.976e-15 - 1.0) < 1e-3
    assert float(R.gelu(torch.tensor(0.0, dtype=torch.float64))) == 0.0


def test_gelu_sweep_covers_what_it_claims():
    x = R.gelu_sweep()
    assert x.numel() % 3072 == 0 and x.dtype == torch.float32
    assert float(x.min()) == -40.0 and float(x.max()) == 40.0
    assert int(((x > -5.6) & (x < -5.4)).sum()) > 100 and int((x < -5.5).sum()) > 2000 and int((x > 6.0).sum()) > 2000
    z = x[x == 0]
    assert bool(torch.signbit(z).any()) and not bool(torch.signbit(z).all())
    # 0.5 x (1 + erff) is exactly 0 on part of the sweep where the pair planes can still hold the fp64 value
    y = R.gelu(x.double())
    lib = 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))
    assert int(((lib == 0) & (R.pair_value64(y.float()) != 0)).sum()) > 100
    assert bool((R.gelu_allowed(x.double(), y) < 2e-5).all())


@pytest.mark.parametrize("family", R.ATTN_FAMILIES)
def test_attention_inputs_produce_their_softmax_class(family):
    nf, n = 8, 5
    L = 1 + nf * n
    peak = R.last_key_rows(nf, n, "space") if family == "last" else torch.tensor([7])
    qkv = R.attention_inputs(2, L, family, 11, peak_rows=peak).double()
    q, k, v = (R._heads(t) for t in qkv.chunk(3, dim=-1))
    s = 0.125 * q[:, :, :1] @ k.transpose(-1, -2)                       # CLS scores (2, H, 1, L)
    arg = s.argmax(dim=-1)
    if family in ("flat", "ones"):
        assert float(s.abs().max()) < 0.5
        assert bool((v == 1).all()) == (family == "ones")
    elif family == "peak30":
        assert bool((arg == 7).all()) and 28.0 < float(s[..., 7].min()) and float(s[..., 7].max()) < 32.0
        assert float(s[..., :7].abs().max()) < 0.5
    elif family == "first":
        assert bool((arg == 0).all()) and float(s[..., 0].min()) > 11.0
    elif family == "last":
        sp = 0.125 * q[:, :, 1:n + 1] @ R._pattern_kv(k, nf, n, "space")[:, :, 0].transpose(-1, -2)       # frame 0's queries
        assert bool((sp.argmax(dim=-1) == n).all()) and float(sp[..., n].min()) > 11.0
    else:
        assert 70.0 < float(s.abs().max()) < 85.0 and float(s.abs().mean()) > 30.0


def test_scale_v_marks_regions():
    qkv = R.attention_inputs(2, 9, "ones", 12)
    R.scale_v(qkv, (1, slice(None)))
    R.scale_v(qkv, torch.tensor([2, 3]), 7.0)
    v = qkv[..., 2 * R.D:]
    assert bool((v[0, 0] == 1).all()) and bool((v[0, 2] == 7).all()) and bool((v[1, 0] == 100).all()) and bool((v[1, 3] == 700).all())
    assert bool((qkv[..., :2 * R.D].abs() < 2).all())


@pytest.mark.parametrize("mode", ["time", "space"])
def test_bars_are_finite_and_far_below_a_wrong_key(mode):
    """The a-priori pair bound and the fp32 floor, relative to max |v|, against the error of an attention that drops or swaps ONE key."""
    nf, n = 8, 15
    L = 1 + nf * n
    for family in R.ATTN_FAMILIES:
        peak = R.last_key_rows(nf, n, mode) if family == "last" else torch.tensor([1 + n + 3])
        qkv = R.attention_inputs(2, L, family, 13, peak_rows=peak)
        R.scale_v(qkv, (1, slice(None)))
        ap = R.pair_attention_apriori(qkv, nf, n, mode)
        assert bool(torch.isfinite(ap).all()) and float(ap.max()) < 5e-4, (family, float(ap.max()))
        ref = R.pattern_attention(qkv.double(), nf, n, mode)
        e_ref = float(((R.pattern_attention(qkv, nf, n, mode).double() - ref).abs() / R.pattern_vscale(qkv.double(), nf, n, mode)).max())
        assert R.fp32_bar(e_ref) < 1e-4, (family, e_ref)
        if family == "ones":
            continue
        # segment 1 reading segment 0's values: an error of the order of its own max |v|
        wrong = qkv.clone()
        wrong[1, :, 2 * R.D:] = qkv[0, :, 2 * R.D:]
        d = (R.pattern_attention(wrong.double(), nf, n, mode) - ref)[1].abs() / R.pattern_vscale(qkv.double(), nf, n, mode)[1]
        assert float(d.max()) > 1e-2 > 20 * (R.fp32_bar(e_ref) + float(ap.max())), (family, float(d.max()))


def test_constant_row_floor_bounds_a_sum_in_the_stated_number_of_roundings():
    """ln_constant_row_floor against an fp32 mean taken the way its derivation says (per lane 16 or 8 equal values left to right, six
    pairwise butterfly steps over 64 lanes, one division): the output error |w| |mean - c| / sqrt(eps) stays inside it, it is not
    vacuous (some rows do leave the bias), and it is far below an output of order 1."""
    c = (torch.randn(4096, generator=R.gen(14)) * 3.0).float()
    lanes = torch.zeros(4096, 64)
    for i in range(16):
        lanes[:, :32] = lanes[:, :32] + c[:, None]
        if i < 8:
            lanes[:, 32:] = lanes[:, 32:] + c[:, None]
    for step in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[:, torch.arange(64) ^ step]
    mean = lanes[:, 0] / 768.0
    w = torch.full((R.D,), 1.5)
    err = 1.5 * (c - mean).double().abs() / math.sqrt(R.EPS)
    floor = R.ln_constant_row_floor(c[:, None].expand(4096, R.D), w)[:, 0]
    assert bool((err <= floor).all()) and float(err.max()) > 0.0
    assert float((floor / c.double().abs().clamp(min=1e-3)).max()) < 3e-3          # 22 x 2^-24 x 1.5 x 1000 = 2e-3 per unit of |c|
