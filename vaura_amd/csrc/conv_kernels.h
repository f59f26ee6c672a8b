// What the codec's conv kernels (dac.hip) and the extractor's linear-layer kernels (linear.hip) share: the argument structs and their
// tap / phase geometry, the Snake / GELU epilogue arithmetic, the activation formats' stores and the tile store.  Device helpers only —
// every kernel is emitted by exactly one unit.
#pragma once
#include "common.h"

#define BM 128  // positions per workgroup tile
#define BN 96    // output channels per workgroup tile (divides 1536, 768, 384, 192, 96)
#define BK 32    // input channels per k-tile

struct ConvArgs {
  const float* in;     // (B, Lin, Cin) already activated
  const float* w;      // [phase][tap][Cout][Cin]
  const float* bias;   // (Cout)
  const float* res;    // optional (B, Lout, Cout)
  const float* alpha;  // (Cout) Snake alpha for out_act
  float* out_raw;      // optional (B, Lout, Cout)
  float* out_act;      // optional (B, Lout, Cout)
  int Lin, Lout, Cin, Cout, NT;
  int off_base, off_step;   // off_t = off_base + t*off_step
  int ostride, oshift0;     // output row = j*ostride + oshift0 + phase
  int jcount;               // j in [0, jcount)
};

// mx8 activation buffers keep their scale words behind the e4m3 bytes of the whole (B, L, C) tensor
__host__ __device__ __forceinline__ size_t mx8_scale_offset(size_t elems) { return (elems + 15) & ~(size_t)15; }

// sin^2(x) for Snake.  The library sinf (Payne-Hanek path, sign / quadrant selects; inlined at every call site) was 2.3 ms of the 11.2 ms
// decode of 8 clips (profiles/r04_codec_ablations.txt: the activation, not the matrix pipe, was the codec's largest single cost).  Only
// the SQUARE is needed, and sin^2 has period pi and no sign: n = rint(x / pi), r = x - n pi in two fused steps (pi = PI_A + PI_B; the
// fma keeps n PI_A exact), sin r on [-pi/2, pi/2] as r + r t p(t), t = r^2 (degree-4 fit of sin(r)/r - 1: 7e-9 before rounding).
// Measured against fp64 over |x| <= 3e4: max abs error 2.5e-7, rms 3.7e-8 — the fp32 sinf squared gives 1.2e-7 / 2.9e-8; both are
// rounding noise of the final multiply.  The error stays at that level while n is exact (|x| < ~1e6; the fp16-plane activation
// format itself ends at 65504) and grows smoothly beyond.  tests/test_gpu_ops.py::test_snake_sine.
__device__ __forceinline__ float snake_sin2(float x) {
  const float n = __builtin_rintf(x * 0.318309886183790672f);
  float r = fmaf(-n, 3.14159274101257324f, x);
  r = fmaf(-n, -8.74227765734758577e-8f, r);
  const float t = r * r;
  float p = fmaf(t, 2.6051661734527443e-06f, -0.00019809046352747828f);
  p = fmaf(t, p, 0.008333050645887852f);
  p = fmaf(t, p, -0.16666658222675323f);
  const float sn = fmaf(r, t * p, r);
  return sn * sn;
}
// inv = 1.0f / (al + 1e-9f): one IEEE division per CHANNEL where a thread keeps its channels (the tile store, the fused unit), not per element
__device__ __forceinline__ float snake_fi(float v, float al, float inv) { return v + inv * snake_sin2(al * v); }
__device__ __forceinline__ float snake_f(float v, float al) { return snake_fi(v, al, 1.0f / (al + 1e-9f)); }

// ---------------------------------------------------------------------------------------------
// fp16-pair variant (codec precision 1): activations and weights travel as (hi, lo) fp16 pairs,
//   x = fp16(x) + fp16(x - fp16(x))   (22 significand bits; |rel err| <= 2^-22),
// and a product is three v_mfma_f32_16x16x32_f16: lo_w*hi_x + hi_w*lo_x + hi_w*hi_x (fp16 x fp16 products
// are exact in fp32; the dropped lo*lo term is < 2^-22).  5.3x fewer matrix-pipe cycles than the exact
// fp32 MFMA (conv_mfma_kernel, dac.hip) at an error far inside the codec's 1e-4 RMS budget (measured).
// "pair layout" of an activated (L x C) buffer / a weight tap (Cout x Cin): per row, C/8 octets of
// [plane hi|lo][8] halves = 32 B -> one row of 32 channels is still one 128-B line, same bytes as fp32.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct ConvPArgs {
  const uint16_t* in;    // pair layout (B, Lin, Cin)
  const uint16_t* w;     // pair layout [phase][tap][Cout][Cin]
  const float* bias;
  const float* res;      // fp32 (B, Lout, Cout)
  const float* alpha;
  float* out_raw;        // fp32
  uint16_t* out_act;     // pair layout, Snake applied
  int Lin, Lout, Cin, Cout, NT;
  int off_base, off_step, ostride, oshift0, jcount;
  int act;               // activation written to out_act: 0 Snake(alpha) (the codec), 1 exact GELU, 2 identity (row f2's linears)
  // --- block-scaled fp8 ("mx8") activations (codec precision 3, conv_mx8_kernel in dac.hip)
  int act_fmt;           // out_act format: 0 (hi, lo) fp16 pairs, 1 mx8 = e4m3 bytes (B, Lout, Cout) + out_scale
  uint8_t* out_scale;    // (B, Lout, ceil(Cout/128)) words of four E8M0 bytes: one power-of-two scale per 32 channels of a row
  const uint32_t* in_scale;   // the same for an mx8 input
  const float* wscale;   // (Cout) power-of-two scale of each output channel's e4m3 weights
  // --- residual unit in one launch (conv_pair_kernel<.., FUSE = true>): this conv (7 taps) -> Snake(alpha_mid) -> 1 x 1 conv (w2, bias2)
  //     -> + res -> out_raw / Snake(alpha) -> out_act.  bias / alpha_mid belong to the first conv, res / out_* / alpha to the second.
  const uint16_t* w2;    // pair layout [Cout][Cout]
  const float* bias2;
  const float* alpha_mid;
};

// The tap / phase geometry of a conv over Lin rows, into the fields ConvArgs and ConvPArgs share; returns the phase count (the launch
// has B * phases workgroups along z).  stride 1: `taps` taps `dilation` rows apart, centred.  stride r > 1: the transposed conv
// (k = 2r, pad = r / 2) as r two-tap problems over j in [0, Lin] — row j of phase ph is output row j r - r / 2 + ph, masked to [0, Lout).
template <class Args>
static inline int va_conv_geometry(Args& a, int taps, int dilation, int stride, int Lin) {
  if (stride > 1) {
    a.NT = 2; a.off_base = 0; a.off_step = -1; a.ostride = stride; a.oshift0 = -(stride / 2);
    a.Lout = Lin * stride; a.jcount = Lin + 1;
    return stride;
  }
  a.NT = taps; a.off_base = -((taps - 1) / 2) * dilation; a.off_step = dilation;
  a.ostride = 1; a.oshift0 = 0; a.Lout = Lin; a.jcount = Lin;
  return 1;
}

// conv_pair_kernel<3, false> (dac.hip) on a filled one-tap problem: the 128 x 96 tile of va_launch_linear_pair (linear.hip)
int va_launch_conv_pair_tile(const ConvPArgs& p, int B, hipStream_t s);

// Exact (erf) GELU, 0.5 x (1 + erf(x / sqrt 2)), as row f2's fc1 epilogue applies it 1.85 G times per 8 clips.  The library erff (inlined,
// branches) cost 1.2 ms of the extractor's 43.7 (profiles/r04_codec_ablations.txt).  Own form: with t = |x| / sqrt 2,
//   1 + erf(x / sqrt 2) = erfc(t) for x < 0, 2 - erfc(t) for x >= 0,   erfc(t) = exp(-t^2) k P(k),  k = 1 / (1 + 0.35 t),
// P a degree-8 fit of erfcx(t) / k on t in [0, 6] (3e-8 relative before rounding).  No cancellation on the negative side (the library
// form rounds 1 + erf to 0 below x = -5.5).  Against fp64: |error| <= 1.3e-7 max(1, |x|) — the rounding of the final products; the fp32
// 0.5 x (1 + erff(..)) form is at 4.5e-7.  tests/test_gpu_avclip.py keeps the features within 1e-4 of the reference's (observed 5e-6).
__device__ __forceinline__ float gelu_erf_f(float x) {
  const float t = fabsf(x) * 0.70710678118654752440f;
  const float k = __builtin_amdgcn_rcpf(fmaf(t, 0.35f, 1.0f));
  float p = 0.06797561794519424f;
  p = fmaf(p, k, -0.4044332206249237f);
  p = fmaf(p, k, 0.8392713069915771f);
  p = fmaf(p, k, -0.7225478887557983f);
  p = fmaf(p, k, 0.6403822898864746f);
  p = fmaf(p, k, -0.046077974140644073f);
  p = fmaf(p, k, 0.23748238384723663f);
  p = fmaf(p, k, 0.1900186985731125f);
  p = fmaf(p, k, 0.1979287713766098f);
  const float e = (k * p) * __builtin_amdgcn_exp2f(-(t * t) * 1.4426950408889634f);
  return (0.5f * x) * (x < 0.f ? e : 2.0f - e);
}

__device__ __forceinline__ void store_pair4(uint16_t* base, size_t row, int c0, int C, const f32x4 v) {
  // 4 consecutive channels c0..c0+3 (c0 % 4 == 0) of one row
  _Float16 h[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float x = v[i];
    h[i] = (_Float16)x;
    l[i] = (_Float16)(x - (float)h[i]);
  }
  typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
  f16x4* p = reinterpret_cast<f16x4*>(base + ((row * (size_t)(C >> 3) + (size_t)(c0 >> 3)) * 2) * 8 + (c0 & 7));
  p[0] = f16x4{h[0], h[1], h[2], h[3]};
  p[2] = f16x4{l[0], l[1], l[2], l[3]};   // +8 halves = the lo plane of the same octet
}

// E8M0 byte of the smallest power of two s with amax <= 448 * s (448 = 1.75 * 2^8 = the e4m3 maximum); same rule as
// vaura_amd/quant.py::fp8_row_scales, clamped to the bytes whose reciprocal is a normal float.
__device__ __forceinline__ int mx8_scale_byte(float amax) {
  const uint32_t bits = __builtin_bit_cast(uint32_t, amax);
  const int ea = (int)((bits >> 23) & 0xffu);
  const int e8 = ea - ((bits & 0x7fffffu) <= 0x600000u ? 8 : 7);
  return e8 < 1 ? 1 : (e8 > 253 ? 253 : e8);
}

// One octet (8 consecutive channels co..co+7 of global row `grow`) of an activated tensor in the next layer's input format.
// mx8: the 4 threads of a 32-channel block must be consecutive lanes, all active.
__device__ __forceinline__ void store_act_octet(void* out_act, uint8_t* out_scale, int fmt, size_t grow, int co, int C,
                                                const float (&sv)[8]) {
  if (fmt == 0) {
    f16x8 hi, lo;
#pragma unroll
    for (int r = 0; r < 8; ++r) { hi[r] = (_Float16)sv[r]; lo[r] = (_Float16)(sv[r] - (float)hi[r]); }
    f16x8* dst = reinterpret_cast<f16x8*>(reinterpret_cast<uint16_t*>(out_act) + ((grow * (size_t)(C >> 3) + (size_t)(co >> 3)) * 2) * 8);
    dst[0] = hi;
    dst[1] = lo;
  } else {
    float amax = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) amax = fmaxf(amax, fabsf(sv[r]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    const int e8 = mx8_scale_byte(amax);
    const float inv = __builtin_bit_cast(float, (uint32_t)(254 - e8) << 23);
    int q0 = 0, q1 = 0;
    q0 = __builtin_amdgcn_cvt_pk_fp8_f32(sv[0] * inv, sv[1] * inv, q0, false);
    q0 = __builtin_amdgcn_cvt_pk_fp8_f32(sv[2] * inv, sv[3] * inv, q0, true);
    q1 = __builtin_amdgcn_cvt_pk_fp8_f32(sv[4] * inv, sv[5] * inv, q1, false);
    q1 = __builtin_amdgcn_cvt_pk_fp8_f32(sv[6] * inv, sv[7] * inv, q1, true);
    typedef int i32x2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<i32x2*>(reinterpret_cast<uint8_t*>(out_act) + grow * (size_t)C + co) = i32x2{q0, q1};
    if (((co >> 3) & 3) == 0) out_scale[(grow * (size_t)((C + 127) >> 7) + (co >> 7)) * 4 + ((co >> 5) & 3)] = (uint8_t)e8;
  }
}

// Second half of the conv epilogue, shared by the pair and the mx8 kernel: `stage` holds the BM x BN_ fp32 tile (bias
// added), every thread owns whole octets of a row: + residual, raw store, activation, and the activated copy in the next
// layer's input format.
// Snake for an fp8 consumer: hardware sine (v_sin_f32, argument in revolutions) and reciprocal — absolute error ~1e-6 of a
// value that is about to be rounded to 3 mantissa bits; the library sinf (argument reduction + polynomial, ~10x the
// instructions) costs more than the layer's matrix instructions once those run at the fp8 rate.
__device__ __forceinline__ float snake_fast(float v, float al) {
  const float sn = __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(al * v * 0.15915494309189535f));   // v_sin_f32's domain is +-256 revolutions
  return v + __builtin_amdgcn_rcpf(al + 1e-9f) * (sn * sn);
}

template <int BN_, int SP, bool FAST = false, int ROWS = BM>
__device__ __forceinline__ void conv_tile_store(const ConvPArgs& a, const float* stage, int b, int ph, int j0, int n0, int tid) {
  constexpr int OCT = BN_ / 8;              // octets per tile row
  static_assert(OCT % 4 == 0, "a 32-channel scale block = 4 consecutive threads of one row");
  // a thread keeps ONE octet column and walks the rows (256 / OCT rows per sweep: 21 for 96 columns — threads 252..255 sit out, a whole
  // 4-thread scale group — 32 for 64): its eight Snake alphas and their inverses are loaded / divided once, not per element
  constexpr int RSTEP = 256 / OCT;
  if (tid >= RSTEP * OCT) return;
  const int oc = tid % OCT, row0 = tid / OCT;
  const int co = n0 + oc * 8;
  const size_t obase = (size_t)b * a.Lout;
  f32x4 al0 = f32x4{0.f, 0.f, 0.f, 0.f}, al1 = al0, iv0 = al0, iv1 = al0;
  if (a.out_act && a.act == 0) {
    al0 = *reinterpret_cast<const f32x4*>(a.alpha + co);
    al1 = *reinterpret_cast<const f32x4*>(a.alpha + co + 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) { iv0[r] = 1.0f / (al0[r] + 1e-9f); iv1[r] = 1.0f / (al1[r] + 1e-9f); }
  }
  for (int row = row0; row < ROWS; row += RSTEP) {
    const int jr = j0 + row;
    if (jr >= a.jcount) continue;
    const int orow = jr * a.ostride + a.oshift0 + ph;
    if (orow < 0 || orow >= a.Lout) continue;
    const size_t o = (obase + (size_t)orow) * a.Cout + co;
    f32x4 v0 = *reinterpret_cast<const f32x4*>(stage + row * SP + oc * 8);
    f32x4 v1 = *reinterpret_cast<const f32x4*>(stage + row * SP + oc * 8 + 4);
    if (a.res) {
      v0 = *reinterpret_cast<const f32x4*>(a.res + o) + v0;
      v1 = *reinterpret_cast<const f32x4*>(a.res + o + 4) + v1;
    }
    if (a.out_raw) {
      *reinterpret_cast<f32x4*>(a.out_raw + o) = v0;
      *reinterpret_cast<f32x4*>(a.out_raw + o + 4) = v1;
    }
    if (a.out_act) {
      float sv[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (FAST && a.act == 0) {
          sv[r] = snake_fast(v0[r], al0[r]);
          sv[r + 4] = snake_fast(v1[r], al1[r]);
        } else {
          sv[r] = a.act == 0 ? snake_fi(v0[r], al0[r], iv0[r]) : (a.act == 1 ? gelu_erf_f(v0[r]) : v0[r]);
          sv[r + 4] = a.act == 0 ? snake_fi(v1[r], al1[r], iv1[r]) : (a.act == 1 ? gelu_erf_f(v1[r]) : v1[r]);
        }
      }
      store_act_octet(a.out_act, a.out_scale, a.act_fmt, obase + (size_t)orow, co, a.Cout, sv);
    }
  }
}

