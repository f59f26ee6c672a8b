"""Exact-arithmetic reference of the decoder's linear kernels (csrc/gemv.hip, gemv3.hip, gemv3_kernel.h, gemv_kernel.h).  No GPU here.

The kernels multiply fp16 x fp16 on the MFMA (the pair path) or fp32 x fp32 (vaura_gemv) and sum in fp32, in an order that differs per
instantiation: k-slices per wave, batches, K halves, row halves, cross-wave and cross-lane reductions.  On the inputs below every product
is exact in fp32 and every partial sum of any subset of the products, in any order, is an fp32 number, so EVERY instantiation must return
the mathematically exact value bit for bit; a dropped, duplicated or misplaced product, plane, k-group, tile or row is an inequality.

The lattice
    activations  x = a + b 2^-13     a in {-1, 0, 1} (zero with probability 1/2), b in {-1, 0, 1}, b = 0 where a = 0
                                     -> fp16(x) = a, the lo plane is b 2^-13 exactly: both planes carry information.  (Where a = 0 a non-zero
                                     b would land in the HI plane and bring cross terms of granularity 2^-26.)
    weights      w = wa + wb 2^-13   wa in {-2..2} (K = 4096: {-1, 0, 1}), half of them zero; wb in {-1, 0, 1}, zero where wa = 0 and
                                     non-zero for the two-plane storage only: one plane / e4m3 hold w = wa exactly
    gains        powers of two in {1/2, 1, 2}, per column; residuals: multiples of 2^-13, |res| <= 64
    condition    every term is a multiple of the granule q (2^-13, times the smallest gain / scale in play) and
                 max (sum_k |x_k| |w_k| + |res|) < 2^24 q  -> every partial sum fits 24 bits (lattice_condition)
tests/test_linear_reference_host.py proves these statements on the CPU; tests/test_gpu_linear.py runs the kernels against them.

Where one rounding chain remains (fused norm, SwiGLU, GELU, ss_out) the bounds below are derived from the kernels' source, per element and
relative to the element's OWN exact value; none of them is measured on the code under test.
"""
import torch

U = 2.0 ** -24                   # unit roundoff of fp32: one correctly rounded operation has relative error <= U
LO = 2.0 ** -13
STORE, RESID, SWIGLU, GELU, LOGITS = 0, 1, 2, 3, 4
EPI_NAMES = {STORE: "STORE", RESID: "RESID", SWIGLU: "SWIGLU", GELU: "GELU", LOGITS: "LOGITS"}
STORAGES = ("h1", "h2", "fp8", "fp8h")
WT = {"h1": 0, "fp8": 1, "h2": 2, "fp8h": 3}         # storage tag of gemv3_kernel.h
EPS = float(torch.tensor(1e-5, dtype=torch.float32))   # eps as the float argument of the entry points holds it
SS_BASE = 600                   # mean square of row r as ss_partials states it: SS_BASE + 7 r (keeps |y1| <= 12 in the SwiGLU cases)

# ---------------------------------------------------------------------------------------------------------------- shapes and cases
# only these depths are compiled, so they are the smallest that exist
PAIR_SHAPES = {
    "qkv":        dict(K=1536, N=4608, epi=STORE, norm=True, ksplit=False),
    "qkv_ksplit": dict(K=1536, N=4608, epi=STORE, norm=True, ksplit=True),
    "store1536":  dict(K=1536, N=1536, epi=STORE, norm=False, ksplit=False),
    "resid1536":  dict(K=1536, N=1536, epi=RESID, norm=False, ksplit=False),
    "resid4096":  dict(K=4096, N=1536, epi=RESID, norm=False, ksplit=False),
    "store4096":  dict(K=4096, N=1536, epi=STORE, norm=False, ksplit=False),
    "swiglu":     dict(K=1536, N=8192, epi=SWIGLU, norm=True, ksplit=False),
    "logits":     dict(K=1536, N=9216, epi=LOGITS, norm=True, ksplit=False),
}
ROWS = (1, 8, 9, 16, 17, 32, 33)       # one live half, both halves, a ragged and a full second block, a two-block pass plus a tail block
EXTRA_ROWS = (250, 272)                # 16 and 17 row blocks: the GEMM tiling, live rows not a multiple of 16
EXTRA_SHAPES = ("resid4096", "swiglu", "logits")
EXTRA_STORAGES = ("h1", "h2", "fp8")
VARIANT_SHAPES = ("store1536", "resid1536", "resid4096", "store4096")
VARIANT_ROWS = (16, 32)


def n_out(shape):
    s = PAIR_SHAPES[shape]
    return s["N"] // 2 if s["epi"] == SWIGLU else s["N"]


def max_rows(shape):
    return EXTRA_ROWS[-1] if shape in EXTRA_SHAPES else ROWS[-1]


def pair_cases():
    """(shape, storage, rows, variant) of the exact half; variant '' = the product, else a switch of vaura_amd.variants."""
    out = []
    for shape in PAIR_SHAPES:
        for st in STORAGES:
            out += [(shape, st, r, "") for r in ROWS]
            if shape in EXTRA_SHAPES and st in EXTRA_STORAGES:
                out += [(shape, st, r, "") for r in EXTRA_ROWS]
            if shape in VARIANT_SHAPES:
                out += [(shape, st, r, "ROWSPLIT_OFF") for r in VARIANT_ROWS]
                if st in ("fp8", "fp8h"):
                    out += [(shape, st, r, "FP8_ROWSPLIT_OFF") for r in VARIANT_ROWS]
    return out


# ---------------------------------------------------------------------------------------------------------------- dispatch table
# What va_launch_gemv3 / dispatch3 (gemv3.hip) launch for vaura_gemv_pair, per (shape, storages, variant, row range): to be read
# against gemv3.hip dispatch3 and va_launch_gemv3.  {wt} = the storage tag (WT above).  gemv3_kernel<G, NW, T, EPI, NORM, XB, WT, KS, RBK>
# (ABL = 0 left out), gemv3h_kernel<G2, NW, EPI, XB, WT, NBF, RBK> with its `halves` argument, gemm3_kernel<EPI, NORM, WT, RBT, PF>,
# gemm4_kernel<EPI, NORM, WT, RBW, CT>.  Row ranges: 1..8 one live half of one row block, 9..16 one row block, 17..32 two row blocks (one
# pass of the RBK = 2 instances), 33..240 three to fifteen row blocks (RBK = 2 passes plus a tail), 241.. the GEMM tiling (R >= 16).
R_HALF, R_ONE, R_TWO, R_MANY, R_GEMM = (1, 8), (9, 16), (17, 32), (33, 240), (241, 1 << 30)
BELOW_GEMM = (R_HALF, R_ONE, R_TWO, R_MANY)
H12, F8, ALLST = ("h1", "h2"), ("fp8", "fp8h"), STORAGES
OFF, F8OFF = "ROWSPLIT_OFF", "FP8_ROWSPLIT_OFF"
PAIR_TABLE = [
    # shape, storages, variant, row ranges, instantiation
    # --- qkv: launch3<WT, 6, 8, 2, E3_STORE, true, XB2> (no two-row-block form: RB2 = false)
    ("qkv", ("h1", "fp8", "fp8h"), "", BELOW_GEMM, "gemv3_kernel<6,8,2,STORE,true,XB=1,WT={wt},KS=1,RBK=1>"),
    ("qkv", ("h2",), "", BELOW_GEMM, "gemv3_kernel<6,8,2,STORE,true,XB=3,WT=2,KS=1,RBK=1>"),
    # --- K-split qkv (out_khalf2): va_launch_gemv3, launch3<.., KS = 2, RB2 = true>
    ("qkv_ksplit", ("h1",), "", (R_HALF, R_ONE), "gemv3_kernel<3,8,3,STORE,true,XB=1,WT=0,KS=2,RBK=1>"),
    ("qkv_ksplit", ("h1",), "", (R_TWO, R_MANY), "gemv3_kernel<3,8,3,STORE,true,XB=1,WT=0,KS=2,RBK=2>"),
    ("qkv_ksplit", ("h2",), "", (R_HALF, R_ONE), "gemv3_kernel<3,8,3,STORE,true,XB=1,WT=2,KS=2,RBK=1>"),
    ("qkv_ksplit", ("h2",), "", (R_TWO, R_MANY), "gemv3_kernel<3,8,3,STORE,true,XB=3,WT=2,KS=2,RBK=2>"),
    ("qkv_ksplit", F8, "", (R_HALF, R_ONE), "gemv3_kernel<6,4,3,STORE,true,XB=1,WT={wt},KS=2,RBK=1>"),
    ("qkv_ksplit", F8, "", (R_TWO, R_MANY), "gemv3_kernel<6,4,3,STORE,true,XB=1,WT={wt},KS=2,RBK=2>"),
    # --- STORE without norm, K = 1536: fp16 planes on the row-split kernel (launch3h<WT, 3, E3_STORE, 1>), fp8 on launch3<WT, 6, 8, 1, E3_STORE, false>
    ("store1536", H12, "", (R_HALF,), "gemv3h_kernel<3,8,STORE,XB=1,WT={wt},NBF=2,RBK=1> halves=1"),
    ("store1536", H12, "", (R_ONE, R_TWO, R_MANY), "gemv3h_kernel<3,8,STORE,XB=1,WT={wt},NBF=2,RBK=1> halves=2"),
    ("store1536", F8, "", BELOW_GEMM, "gemv3_kernel<6,8,1,STORE,false,XB=1,WT={wt},KS=1,RBK=1>"),
    ("store1536", ALLST, OFF, (R_ONE, R_TWO), "gemv3_kernel<6,8,1,STORE,false,XB=1,WT={wt},KS=1,RBK=1>"),
    ("store1536", F8, F8OFF, (R_ONE, R_TWO), "gemv3_kernel<6,8,1,STORE,false,XB=1,WT={wt},KS=1,RBK=1>"),
    # --- RESID, K = 1536: launch3h<WT, 3, E3_RESID, 1, 2, 8, true>; fp8 with one row block and every ROWSPLIT_OFF: launch3<WT, 6, 8, 1, E3_RESID, false, 1, 1, true>
    ("resid1536", H12, "", (R_HALF,), "gemv3h_kernel<3,8,RESID,XB=1,WT={wt},NBF=2,RBK=1> halves=1"),
    ("resid1536", H12, "", (R_ONE,), "gemv3h_kernel<3,8,RESID,XB=1,WT={wt},NBF=2,RBK=1> halves=2"),
    ("resid1536", ALLST, "", (R_TWO, R_MANY), "gemv3h_kernel<3,8,RESID,XB=1,WT={wt},NBF=2,RBK=2> halves=2"),
    ("resid1536", F8, "", (R_HALF, R_ONE), "gemv3_kernel<6,8,1,RESID,false,XB=1,WT={wt},KS=1,RBK=1>"),
    ("resid1536", ALLST, OFF, (R_ONE,), "gemv3_kernel<6,8,1,RESID,false,XB=1,WT={wt},KS=1,RBK=1>"),
    ("resid1536", ALLST, OFF, (R_TWO,), "gemv3_kernel<6,8,1,RESID,false,XB=1,WT={wt},KS=1,RBK=2>"),
    ("resid1536", F8, F8OFF, (R_ONE,), "gemv3_kernel<6,8,1,RESID,false,XB=1,WT={wt},KS=1,RBK=1>"),
    ("resid1536", F8, F8OFF, (R_TWO,), "gemv3_kernel<6,8,1,RESID,false,XB=1,WT={wt},KS=1,RBK=2>"),
    # --- RESID, K = 4096: launch3h<WT, 8, E3_RESID, (WT == 2 ? 4 : 1), 2, 8, true>; else launch3<WT, 16, 8, 1, E3_RESID, false, 4, 1, true>
    ("resid4096", ("h1",), "", (R_HALF,), "gemv3h_kernel<8,8,RESID,XB=1,WT=0,NBF=2,RBK=1> halves=1"),
    ("resid4096", ("h1",), "", (R_ONE,), "gemv3h_kernel<8,8,RESID,XB=1,WT=0,NBF=2,RBK=1> halves=2"),
    ("resid4096", ("h1", "fp8", "fp8h"), "", (R_TWO, R_MANY), "gemv3h_kernel<8,8,RESID,XB=1,WT={wt},NBF=2,RBK=2> halves=2"),
    ("resid4096", ("h2",), "", (R_HALF,), "gemv3h_kernel<8,8,RESID,XB=4,WT=2,NBF=2,RBK=1> halves=1"),
    ("resid4096", ("h2",), "", (R_ONE,), "gemv3h_kernel<8,8,RESID,XB=4,WT=2,NBF=2,RBK=1> halves=2"),
    ("resid4096", ("h2",), "", (R_TWO, R_MANY), "gemv3h_kernel<8,8,RESID,XB=4,WT=2,NBF=2,RBK=2> halves=2"),
    ("resid4096", F8, "", (R_HALF, R_ONE), "gemv3_kernel<16,8,1,RESID,false,XB=4,WT={wt},KS=1,RBK=1>"),
    ("resid4096", ALLST, OFF, (R_ONE,), "gemv3_kernel<16,8,1,RESID,false,XB=4,WT={wt},KS=1,RBK=1>"),
    ("resid4096", ALLST, OFF, (R_TWO,), "gemv3_kernel<16,8,1,RESID,false,XB=4,WT={wt},KS=1,RBK=2>"),
    ("resid4096", F8, F8OFF, (R_ONE,), "gemv3_kernel<16,8,1,RESID,false,XB=4,WT={wt},KS=1,RBK=1>"),
    ("resid4096", F8, F8OFF, (R_TWO,), "gemv3_kernel<16,8,1,RESID,false,XB=4,WT={wt},KS=1,RBK=2>"),
    # (R >= 16, 6 column tiles of 256: launch_gemm4 picks 64-row workgroups; two planes then take the 128 x 128 form)
    ("resid4096", ("h1",), "", (R_GEMM,), "gemm4_kernel<RESID,false,WT=0,RBW=4,CT=16>"),
    ("resid4096", ("h2",), "", (R_GEMM,), "gemm4_kernel<RESID,false,WT=2,RBW=8,CT=8>"),
    ("resid4096", ("fp8",), "", (R_GEMM,), "gemm3_kernel<RESID,false,WT=1,RBT=4,PF=1>"),
    # --- STORE without norm, K = 4096: launch3h<WT, 8, E3_STORE, (WT == 2 ? 4 : 1)>; else launch3<WT, 16, 8, 1, E3_STORE, false, 4>
    ("store4096", ("h1",), "", (R_HALF,), "gemv3h_kernel<8,8,STORE,XB=1,WT=0,NBF=2,RBK=1> halves=1"),
    ("store4096", ("h1",), "", (R_ONE, R_TWO, R_MANY), "gemv3h_kernel<8,8,STORE,XB=1,WT=0,NBF=2,RBK=1> halves=2"),
    ("store4096", ("h2",), "", (R_HALF,), "gemv3h_kernel<8,8,STORE,XB=4,WT=2,NBF=2,RBK=1> halves=1"),
    ("store4096", ("h2",), "", (R_ONE, R_TWO, R_MANY), "gemv3h_kernel<8,8,STORE,XB=4,WT=2,NBF=2,RBK=1> halves=2"),
    ("store4096", F8, "", BELOW_GEMM, "gemv3_kernel<16,8,1,STORE,false,XB=4,WT={wt},KS=1,RBK=1>"),
    ("store4096", ALLST, OFF, (R_ONE, R_TWO), "gemv3_kernel<16,8,1,STORE,false,XB=4,WT={wt},KS=1,RBK=1>"),
    ("store4096", F8, F8OFF, (R_ONE, R_TWO), "gemv3_kernel<16,8,1,STORE,false,XB=4,WT={wt},KS=1,RBK=1>"),
    # --- SwiGLU: launch3<WT, 6, 8, 2, E3_SWIGLU, true, XB2, 1, true, 3>
    ("swiglu", ("h1", "fp8", "fp8h"), "", (R_HALF, R_ONE), "gemv3_kernel<6,8,2,SWIGLU,true,XB=1,WT={wt},KS=1,RBK=1>"),
    ("swiglu", ("h2",), "", (R_HALF, R_ONE), "gemv3_kernel<6,8,2,SWIGLU,true,XB=3,WT=2,KS=1,RBK=1>"),
    ("swiglu", ALLST, "", (R_TWO, R_MANY), "gemv3_kernel<6,8,2,SWIGLU,true,XB=3,WT={wt},KS=1,RBK=2>"),
    ("swiglu", ("h1",), "", (R_GEMM,), "gemm4_kernel<SWIGLU,true,WT=0,RBW=4,CT=16>"),
    ("swiglu", ("h2",), "", (R_GEMM,), "gemm4_kernel<SWIGLU,true,WT=2,RBW=8,CT=8>"),
    ("swiglu", ("fp8",), "", (R_GEMM,), "gemm3_kernel<SWIGLU,true,WT=1,RBT=4,PF=1>"),
    # --- logits: launch3<WT, 6, 8, 3, E3_LOGITS, true, XB2, 1, true, 3>
    ("logits", ("h1", "fp8", "fp8h"), "", (R_HALF, R_ONE), "gemv3_kernel<6,8,3,LOGITS,true,XB=1,WT={wt},KS=1,RBK=1>"),
    ("logits", ("h2",), "", (R_HALF, R_ONE), "gemv3_kernel<6,8,3,LOGITS,true,XB=3,WT=2,KS=1,RBK=1>"),
    ("logits", ALLST, "", (R_TWO, R_MANY), "gemv3_kernel<6,8,3,LOGITS,true,XB=3,WT={wt},KS=1,RBK=2>"),
    ("logits", ("h1",), "", (R_GEMM,), "gemm4_kernel<LOGITS,true,WT=0,RBW=4,CT=16>"),
    ("logits", ("h2",), "", (R_GEMM,), "gemm4_kernel<LOGITS,true,WT=2,RBW=8,CT=8>"),
    ("logits", ("fp8",), "", (R_GEMM,), "gemm3_kernel<LOGITS,true,WT=1,RBT=4,PF=1>"),
]


def pair_table_row(shape, storage, rows, variant=""):
    """Index of THE row of PAIR_TABLE a case runs (exactly one, else ValueError)."""
    hits = [i for i, (sh, sts, var, ranges, _) in enumerate(PAIR_TABLE)
            if sh == shape and storage in sts and var == variant and any(lo <= rows <= hi for lo, hi in ranges)]
    if len(hits) != 1:
        raise ValueError(f"{shape} {storage} rows={rows} {variant or 'product'}: {len(hits)} rows of PAIR_TABLE")
    return hits[0]


def pair_instance(shape, storage, rows, variant=""):
    return PAIR_TABLE[pair_table_row(shape, storage, rows, variant)][4].format(wt=WT[storage])


def gemm4_plan(R, gx, two_planes):
    """launch_gemm4's choice (gemv3.hip) restated: [(RBW, CT, first row block, row blocks)] per launch."""
    cand, eff = (8, 6, 4), (1.0, 1.03, 1.12 if two_planes else 0.95)

    def rounds(rb, h):
        return float((gx * ((rb + h - 1) // h) + 255) // 256)
    best, h1, h2, cut = 1e30, 4, 0, 0
    for i in range(3):
        c1 = rounds(R, cand[i]) * cand[i] * eff[i]
        if c1 < best:
            best, h1, h2, cut = c1, cand[i], 0, 0
        if cand[i] == 4 or not two_planes:
            continue
        full = gx * ((R + cand[i] - 1) // cand[i]) // 256
        gy1 = full * 256 // gx
        rb1 = gy1 * cand[i]
        if full < 1 or gy1 < 1 or rb1 >= R:
            continue
        for k in range(3):
            c2 = full * cand[i] * eff[i] + rounds(R - rb1, cand[k]) * cand[k] * eff[k] + 0.3
            if c2 < best:
                best, h1, h2, cut = c2, cand[i], cand[k], rb1
    if two_planes and h1 == 4 and not h2:
        return [(8, 8, 0, R)]
    return [(h1, 16, 0, cut if h2 else R)] + ([(h2, 16, cut, R - cut)] if h2 else [])


# vaura_gemv (gemv.hip dispatch<BF16>): every instance; N = 96 is six column tiles (three workgroups of the T = 2 instances)
GEMV_N = 96
GEMV_ROWS = (1, 16, 17, 40)
GEMV_TABLE = [
    # K, epilogue, norm, instantiation gemv_kernel<BF16, G, NW, T, EPI, NORM>
    (1536, STORE, True, "gemv_kernel<{bf},6,8,1,STORE,true>"),
    (1536, STORE, False, "gemv_kernel<{bf},6,8,1,STORE,false>"),
    (1536, RESID, False, "gemv_kernel<{bf},6,8,1,RESID,false>"),
    (1536, SWIGLU, True, "gemv_kernel<{bf},6,8,2,SWIGLU,true>"),
    (1536, LOGITS, True, "gemv_kernel<{bf},6,8,2,LOGITS,true>"),
    (1536, LOGITS, False, "gemv_kernel<{bf},6,8,2,LOGITS,false>"),
    (4096, RESID, False, "gemv_kernel<{bf},16,8,1,RESID,false>"),
    (4096, STORE, False, "gemv_kernel<{bf},16,8,1,STORE,false>"),
    (768, GELU, False, "gemv_kernel<{bf},6,4,1,GELU,false>"),
    (768, STORE, False, "gemv_kernel<{bf},6,4,1,STORE,false>"),
    (512, STORE, False, "gemv_kernel<{bf},4,4,1,STORE,false>"),
    (512, GELU, False, "gemv_kernel<{bf},4,4,1,GELU,false>"),
]


def gemv_cases():
    return [(K, epi, norm, bf16, rows) for (K, epi, norm, _) in GEMV_TABLE for bf16 in (False, True) for rows in GEMV_ROWS]


# ---------------------------------------------------------------------------------------------------------------- lattice generators
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def lattice_x(rows, K, seed, lo=True):
    """(a, b) int8-valued fp64 tensors (rows, K): x = a + b 2^-13."""
    g = _gen(seed)
    c = torch.randint(0, 4, (rows, K), generator=g)
    a = torch.where(c < 2, torch.zeros_like(c), 2 * c - 5)            # 0, 0, -1, 1
    b = torch.randint(-1, 2, (rows, K), generator=g) * (a != 0)
    if not lo:
        b = torch.zeros_like(b)
    return a.double(), b.double()


def lattice_w(N, K, seed, two_planes):
    """(wa, wb) fp32 tensors (N, K): w = wa + wb 2^-13; wa in {-2..2}, {-1, 0, 1} at K = 4096; wb != 0 only with two planes."""
    g = _gen(seed)
    nz = torch.randint(0, 2, (N, K), generator=g, dtype=torch.int8)
    if K >= 4096:
        mag = torch.randint(0, 2, (N, K), generator=g, dtype=torch.int8) * 2 - 1                       # -1, 1
    else:
        c = torch.randint(0, 4, (N, K), generator=g, dtype=torch.int8)
        mag = torch.where(c < 2, c - 2, c - 1)                                                        # -2, -1, 1, 2
    wa = nz * mag
    wb = (torch.randint(-1, 2, (N, K), generator=g, dtype=torch.int8) * (wa != 0)) if two_planes else torch.zeros_like(wa)
    return wa.float(), wb.float()


def pow2_gain(n, seed):
    """(n) fp32 in {1/2, 1, 2}, varying by column."""
    return torch.ldexp(torch.ones(n), torch.randint(-1, 2, (n,), generator=_gen(seed)))


def lattice_res(rows, N, seed):
    """multiples of 2^-13 with |res| <= 64, fp32 (rows, N)"""
    return (torch.randint(-(1 << 19), (1 << 19) + 1, (rows, N), generator=_gen(seed)).double() * LO).float()


def ss_partials(rows, n_ss, base=SS_BASE):
    """Integer partial sums of squares (rows, n_ss), different per row and per partial: row r sums to 16 n_ss (base + 7 r) + a little, an
    fp32 integer in any order (below 2^24 up to 272 rows of 96 partials)."""
    r = torch.arange(rows)[:, None]
    j = torch.arange(n_ss)[None, :]
    ss = 16 * (base + 7 * r) + ((r + 3) * j) % 13
    assert int(ss.sum(1).max()) < 1 << 24
    return ss.double()


def ss_device_layout(ss):
    """(rows, n_ss) -> the (R, n_ss, 16) fp32 buffer of Gemv3Args.ss_in, rows past the last one zero."""
    rows, n_ss = ss.shape
    rp = (rows + 15) // 16 * 16
    buf = torch.zeros(rp, n_ss)
    buf[:rows] = ss.float()
    return buf.view(rp // 16, 16, n_ss).permute(0, 2, 1).contiguous().reshape(-1)


def split2(v):
    """fp32 tensor -> (hi, lo) as split2 of gemv3_kernel.h forms them: hi = fp16(v), lo = fp16(v - hi); fp32 values."""
    v = v.float()
    hi = v.half().float()
    return hi, (v - hi).half().float()


class PairLattice:
    """Inputs of one shape of the pair path on the lattice, for max_rows(shape) rows (a case of fewer rows takes the first ones, so
    every row keeps its own values whatever the row count)."""

    def __init__(self, shape, two_planes, rows=None):
        s = PAIR_SHAPES[shape]
        K, N = s["K"], s["N"]
        seed = 1000 * (1 + list(PAIR_SHAPES).index(shape))
        self.shape, self.two_planes, self.K, self.N, self.epi, self.norm = shape, two_planes, K, N, s["epi"], s["norm"]
        self.rows = rows or max_rows(shape)
        self.a, self.b = lattice_x(self.rows, K, seed + 1)
        self.x = (self.a + self.b * LO).float()                       # what the producer (vaura_split_rows) is given
        self.gain_in = pow2_gain(K, seed + 2) if self.norm else None
        g = self.gain_in.double() if self.norm else 1.0
        self.xhi, self.xlo = self.a * g, self.b * g * LO               # the planes, as real numbers
        self.wa, self.wb = lattice_w(N, K, seed + 3, two_planes)
        self.w = self.wa + self.wb * float(LO)                         # fp32, exact (15 significand bits)
        no = n_out(shape)
        self.res = lattice_res(self.rows, no, seed + 4) if self.epi == RESID else None
        self.gain_out = pow2_gain(no, seed + 5) if self.epi in (STORE, RESID) and not s["ksplit"] else None
        self.ss = ss_partials(self.rows, K // 16) if self.norm else None
        self.granule = LO * (0.5 if self.norm else 1.0)


def pair_products(L, mode, k0=0, k1=None):
    """fp64 (rows, N) sums over k in [k0, k1) and the sum of |terms| next to them.
    mode 'full'  (one weight plane, e4m3):        sum (xhi + xlo) w
         'hi'    (e4m3 against the hi plane only): sum xhi w
         'three' (two weight planes):              sum whi xhi + whi xlo + wlo xhi   (gemv3_kernel.h: the wlo xlo term is dropped)
    Every operand is a small integer times a power of two and every sum is below 2^53 granules: the fp64 matmuls are exact."""
    k1 = L.K if k1 is None else k1
    xhi, xlo = L.xhi[:, k0:k1], L.xlo[:, k0:k1]
    whi, wlo = L.wa[:, k0:k1].double().t(), (L.wb[:, k0:k1].double() * LO).t()
    if mode == "hi":
        return xhi @ whi, xhi.abs() @ whi.abs()
    if mode == "full":
        assert not L.two_planes
        return (xhi + xlo) @ whi, (xhi.abs() + xlo.abs()) @ whi.abs()
    assert mode == "three"
    exact = (xhi + xlo) @ whi + xhi @ wlo
    return exact, (xhi.abs() + xlo.abs()) @ whi.abs() + xhi.abs() @ wlo.abs()


def dropped_term_bound(L):
    """sum |wlo| |xlo|: how far the three-term sum may lie from the full product (rows, N)."""
    return L.xlo.abs() @ (L.wb.double().abs() * LO).t()


def storage_mode(storage, rows):
    if storage == "h2":
        return "three"
    if storage == "fp8h" and (rows + 15) // 16 < 16:
        return "hi"
    return "full"


def lattice_condition(abs_sum, res, granule):
    """max (sum |x||w| + |res|) < 2^24 granule: any partial sum of the terms, in any order, is a multiple of the granule below 2^24 of
    them, i.e. an fp32 number.  (granule 2^-13: the bound is 2^11.)  Returns (largest, bound)."""
    worst = abs_sum if res is None else abs_sum + res.double().abs()
    return float(worst.max()), 2.0 ** 24 * granule


class GemvLattice:
    """Inputs of one instance of vaura_gemv (fp32 activations, fp32 / bf16 weights) on the lattice.  With the fused norm the kernel sums
    x^2 itself, so b = 0 there: the squares are 0 or 1 and the sum is exact.  GELU: x scaled by 2^-3 so that the sums land where
    the tanh moves; SwiGLU: w scaled by 2^-5 so that |y1| <= 12 (the norm divides any scale of x out again)."""

    def __init__(self, K, epi, norm, rows=GEMV_ROWS[-1], N=GEMV_N):
        seed = 50000 + 10 * K + epi + (5 if norm else 0)
        self.K, self.N, self.epi, self.norm, self.rows = K, N, epi, norm, rows
        xs = 0.125 if epi == GELU else 1.0
        ws = 0.03125 if epi == SWIGLU else 1.0
        a, b = lattice_x(rows, K, seed + 1, lo=not norm)
        self.x64 = (a + b * LO) * xs
        self.x = self.x64.float()
        self.gain = pow2_gain(K, seed + 2) if norm else None
        wa, _ = lattice_w(N, K, seed + 3, False)
        self.w = wa * ws
        self.res = lattice_res(rows, N, seed + 4) if epi == RESID else None
        xg = self.x64 * (self.gain.double() if norm else 1.0)
        self.exact = xg @ self.w.double().t()
        self.abs_sum = xg.abs() @ self.w.double().abs().t()
        self.ssq = (self.x64 * self.x64).sum(1) if norm else None      # integers: exact in fp32 in any order
        self.granule = LO * xs * ws * (0.5 if norm else 1.0)


# ---------------------------------------------------------------------------------------------------------------- bounds, from the code
# Fused norm (gemv3_kernel.h gemv3_kernel / gemm3_kernel / gemm4_kernel, gemv_kernel.h):
#     rinv = 1.0f / sqrtf(ssp * (1.0f / (float)K) + eps);   v = sacc * rinv          (built with -ffp-contract=off: no fused multiply-add;
# hipcc's default correctly rounded fp32 division and square root)
# ssp and sacc are exact on the lattice.  In units of U, to first order: the constant 1/K 1, the multiply 1, the add 1 (eps > 0: the sum is
# no smaller than its first operand) -> 3 under the square root = 1.5 behind it, + 1 for sqrtf, + 1 for the division = 3.5 on rinv, + 1 for
# the final multiply: 4.5.  C_NORM = 5 leaves the second-order terms (~ 10 U^2) room.  The bound is relative to the element's own value.
C_NORM = 5.0


def rinv64(ssq, K, eps=EPS):
    return 1.0 / torch.sqrt(ssq / K + eps)


def norm_bound(ref64):
    return C_NORM * U * ref64.abs()


# SwiGLU (gemv3_kernel.h silu3_f / gemv_kernel.h silu_f, gemv3_epilogue):   o = (y1 / (1.0f + expf(-y1))) * y3,   y = sacc * rinv
# y1 and y3 carry C_NORM U each.  silu(y) = y / (1 + e^-y) has condition |1 + y s(-y)| (s = logistic): y1's error arrives multiplied by
# it.  expf: 1 ulp (2 U) on e^-y1 (the negation is exact), weighted e / (1 + e) <= 1 in the denominator; the add 1, the division 1, the
# product with y3 1, y3's own C_NORM.
def swiglu_ref_and_bound(y1, y3):
    sig = torch.sigmoid(y1)
    ref = y1 * sig * y3
    cond = (1.0 + y1 * torch.sigmoid(-y1)).abs()
    e = torch.exp(-y1)
    rel = C_NORM * cond + 2.0 * e / (1.0 + e) + 1.0 + 1.0 + 1.0 + C_NORM
    return ref, rel * U * ref.abs() * (1.0 + 64 * U)


# GELU (gemv_kernel.h gelu_tanh_f):   inner = kBeta * (x + kKappa * (x * x * x));   o = 0.5f * x * (1.0f + tanhf(inner))
# x is exact on the lattice; the constants are the kernel's own fp32 values.  x*x*x 2, * kKappa 1 -> 3 on the cubic term, the add 1 (both
# operands have the sign of x: the term's share is <= 1) -> 4, * kBeta 1 -> 5 U on inner.  tanh' = 1 - t^2: an ABSOLUTE error
# (1 - t^2) |inner| 5 U on t; tanhf 2 ulp = 4 U |t|; the add 1.0f + t: U |1 + t|; 0.5f * x is exact; the last product U.  For x << 0
# the sum 1 + t cancels: the bound is absolute there, as the form the kernel uses makes it.
K_BETA = float(torch.tensor(0.7978845608028654, dtype=torch.float32))
K_KAPPA = float(torch.tensor(0.044715, dtype=torch.float32))


def gelu_ref_and_bound(x):
    inner = K_BETA * (x + K_KAPPA * (x * x * x))
    t = torch.tanh(inner)
    ref = 0.5 * x * (1.0 + t)
    err_sum = (1.0 - t * t) * inner.abs() * 5.0 * U + 4.0 * U * t.abs() + U * (1.0 + t).abs()
    return ref, (0.5 * x.abs() * err_sum + U * ref.abs()) * (1.0 + 64 * U)


# ss_out (gemv3_epilogue): s = ((o0 o0 + o1 o1) + o2 o2) + o3 o3, then two cross-lane adds; every term is non-negative, so the relative
# error of a sum is at most the largest of its operands' plus its own rounding: a square 1, three adds 3, two cross-lane adds 2.
C_SS = 6.0


def ss_out_ref_and_bound(out):
    """out (rows, n) fp32 as returned -> (rows, n/16) fp64 partial sums of squares and their bound"""
    o = out.double()
    ref = (o * o).view(o.shape[0], -1, 16).sum(2)
    return ref, C_SS * U * ref * (1.0 + 64 * U)


def ss_out_rows(buf, rows, n):
    """the (R, n/16, 16) buffer of Gemv3Args.ss_out -> (rows, n/16)"""
    rp = (rows + 15) // 16 * 16
    return buf[: (rp // 16) * (n // 16) * 16].view(rp // 16, n // 16, 16).permute(0, 2, 1).reshape(rp, n // 16)[:rows]


def swiglu_halves(y, N):
    """(rows, N) in the device's tile order (w1 tile, w3 tile, ...) -> (y1, y3) (rows, N/2)"""
    v = y.view(y.shape[0], N // 32, 2, 16)
    return v[:, :, 0].reshape(y.shape[0], N // 2), v[:, :, 1].reshape(y.shape[0], N // 2)
