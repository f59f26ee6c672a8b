// Shared device helpers for libvaura_hip (gfx950 / CDNA4 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/vaura_hip.h"
#include "variants.h"      // va_variant / va_variant_field: the kernel-variant switches for A/B measurements

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define VA_CHECK_LAUNCH()                      \
  do {                                         \
    hipError_t e__ = hipGetLastError();        \
    if (e__ != hipSuccess) return (int)e__;    \
  } while (0)
// launch + check; the sticky per-thread error is cleared first so that a stale error left by some
// earlier, unrelated runtime call (observed: hipErrorNoDevice from a device probe) is not reported here.
// When vaura_profile_loop arms va_prof_start/stop the launch carries its own start/stop events
// (hipExtLaunchKernelGGL): they time exactly the kernel, like rocprofv3's kernel trace does.
extern thread_local int va_prof_kind;
void va_prof_events(hipEvent_t* start, hipEvent_t* stop);
#define VA_LAUNCH(kern, grid, block, smem, stream, ...)                                              \
  do {                                                                                               \
    (void)hipGetLastError();                                                                         \
    if (va_prof_kind >= 0) {                                                                         \
      hipEvent_t va_e0, va_e1;                                                                       \
      va_prof_events(&va_e0, &va_e1);                                                                \
      hipExtLaunchKernelGGL(kern, grid, block, smem, stream, va_e0, va_e1, 0, __VA_ARGS__);         \
    } else {                                                                                         \
      hipLaunchKernelGGL(kern, grid, block, smem, stream, __VA_ARGS__);                              \
    }                                                                                                \
    VA_CHECK_LAUNCH();                                                                               \
  } while (0)

// packed-rows index (see vaura_hip.h): float index of (row, col) in a (rows x C) matrix
__host__ __device__ __forceinline__ size_t packed_index(int row, int col, int C) {
  return ((((size_t)(row >> 4) * (size_t)(C >> 2) + (size_t)(col >> 2)) << 4) + (size_t)(row & 15)) * 4 + (size_t)(col & 3);
}
// float4 index of (row, 4-col quad cq) in packed rows
__host__ __device__ __forceinline__ size_t packed_quad(int row, int cq, int C) {
  return (((size_t)(row >> 4) * (size_t)(C >> 2) + (size_t)cq) << 4) + (size_t)(row & 15);
}

__device__ __forceinline__ float bf16_lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xffff0000u); }

// ---- cross-lane exchanges on the VALU (DPP modifiers + gfx950's v_permlane{16,32}_swap) instead of ds_bpermute: __shfl_xor
// compiles to an LDS-crossbar round trip (~60+ cycles of latency each, and the LDS pipe is shared by the 8 waves of a workgroup);
// the decode attention kernel issued ~50 of them per wave, the GEMV epilogues 4-8 on their post-barrier critical path.
template <int CTRL>
__device__ __forceinline__ float va_dpp(float x) {   // x as seen through DPP control CTRL (all rows / banks enabled)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}
#define VA_DPP_XOR1 0xB1    /* quad_perm [1,0,3,2] */
#define VA_DPP_XOR2 0x4E    /* quad_perm [2,3,0,1] */
#define VA_DPP_HALF_MIRROR 0x141   /* lane i <-> 7 - i of its 8: pairs the two quads (== xor 4 on quad-uniform values) */
#define VA_DPP_ROR8 0x128   /* rotate a 16-lane row by 8 == xor 8 */
// the value of lane ^ 16 / lane ^ 32.  v_permlane{16,32}_swap exchanges the odd rows of its first register with the even rows of
// its second.  PRECONDITION of va_xor16 / va_xor32 / wave_sum / wave_max: 1-D blocks whose size is a multiple of 64 (lane = threadIdx.x
// & 63: every kernel of this library is launched that way — the lane bit costs nothing, an mbcnt pair per call would) and the
// partner lane active (full waves at the call site).  tools/microbench/lane_exchange_probe.hip checks all six exchanges on device.
// The butterfly order of wave_sum / wave_max is 1, 2, 4, 8, 16, 32 since round 3 (round 2: 32 .. 1): fp32 sums round differently from
// round-2 records (LayerNorm in vit, the RVQ argmin distances, the sampler's softmax denominator, rinv) — bit-exactness claims against
// round-2 outputs do not carry over; the goldens (reference-generated) are what pins them.  Written as inline asm: with the builtin, hipcc 7.2 folds `select(lane bit, r[0], r[1])` of swap(x, x) to r[0] (and
// may give both operands one physical register) — tools/microbench/lane_exchange_probe.hip is the passing check of THIS form.  The
// s_nop covers the VALU-write -> permlane-read wait states the compiler would otherwise insert.
__device__ __forceinline__ float va_xor16(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return ((threadIdx.x >> 4) & 1) ? a : b;
}
__device__ __forceinline__ float va_xor32(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return ((threadIdx.x >> 5) & 1) ? a : b;
}
// all-reduce over the 64 lanes, butterfly order 1, 2, 4, 8, 16, 32 (after the xor-1 and xor-2 steps the values are uniform per quad,
// so the half-mirror pairs exactly what xor 4 would)
__device__ __forceinline__ float wave_sum(float v) {
  v += va_dpp<VA_DPP_XOR1>(v);
  v += va_dpp<VA_DPP_XOR2>(v);
  v += va_dpp<VA_DPP_HALF_MIRROR>(v);
  v += va_dpp<VA_DPP_ROR8>(v);
  v += va_xor16(v);
  v += va_xor32(v);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, va_dpp<VA_DPP_XOR1>(v));
  v = fmaxf(v, va_dpp<VA_DPP_XOR2>(v));
  v = fmaxf(v, va_dpp<VA_DPP_HALF_MIRROR>(v));
  v = fmaxf(v, va_dpp<VA_DPP_ROR8>(v));
  v = fmaxf(v, va_xor16(v));
  v = fmaxf(v, va_xor32(v));
  return v;
}

// round-to-nearest-even fp32 -> bf16 bits (inputs are finite weights)
__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

inline hipStream_t as_stream(vaura_stream_t s) { return (hipStream_t)s; }

// Opt a kernel into more than 64 KB of dynamic LDS — once per DEVICE (function attributes are per device: an engine on a second
// GPU of the same process needs its own call).  `done` is a per-call-site bit mask of devices already set up.
inline int va_big_lds_once(const void* fn, size_t bytes, unsigned long long* done) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return VAURA_ERR_STATE;
  if (!((*done >> dev) & 1ull)) {
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return VAURA_ERR_STATE;
    *done |= 1ull << dev;
  }
  return 0;
}


// ---- output stores of the decode-step kernels: write-through (sc0 sc1), so that a kernel leaves no dirty lines in its XCD's L2
// for the end-of-kernel release to write back (MI355X_MICROARCH.md: a release costs ~1.7 us clean, ~6.5 us behind freshly dirtied
// lines): -1 % on the decode loop.  Inline asm because no builtin takes a per-lane address with cache-policy bits; hipcc does not
// know the statement is a store of 4 registers, so the string itself ends with the wait state that keeps the next instruction from
// overwriting the data registers before the store has read them (cdna_hip_programming.md, inline asm: stores).
// -DVAURA_PLAIN_STORES (experiment build, python -m vaura_amd.csrc.build --plain-stores): ordinary stores, for the A/B.
#ifndef VAURA_PLAIN_STORES
__device__ __forceinline__ void va_st16(void* p, const f32x4 v) { asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void va_st8(void* p, const uint2 v) { asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void va_st4(void* p, const float v) { asm volatile("global_store_dword %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory"); }
#else
__device__ __forceinline__ void va_st16(void* p, const f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void va_st8(void* p, const uint2 v) { *reinterpret_cast<uint2*>(p) = v; }
__device__ __forceinline__ void va_st4(void* p, const float v) { *reinterpret_cast<float*>(p) = v; }
#endif

// ---- in-kernel time stamps: DIAGNOSTIC BUILD ONLY (python -m vaura_amd.csrc.build --stamps -> libvaura_hip_stamps.so; the product
// library is compiled without VAURA_STAMPS and contains none of this).  Every wave of the decode-step kernels reads
// s_memrealtime (100 MHz, one counter for the whole chip: comparable across CUs and across launches) at fixed points and writes
// ONE 128-byte record per wave to a side buffer that no kernel reads: {kind | block << 8 | xcc << 40 | wave << 48, t0 .. t6, t7}.  tools/pmc_driver --stamps
// collects them, tools/stamp_report.py turns them into the per-phase shares of profiles/r03_stage_stamps.json.  The stamps
// drain the memory pipeline where they wait, so this build's run TIME means nothing; its phase SHARES do.
#ifdef VAURA_STAMPS
static __device__ unsigned long long* va_stamp_ptr = nullptr;   // [0] = record counter, [1] = capacity, [2] = 1: every wave writes a record (0: wave 0 only), records from [8]
struct VaStamps { unsigned long long t[7]; };
__device__ __forceinline__ unsigned long long va_now() {
  unsigned long long t;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define VA_STAMP(st, i) do { __builtin_amdgcn_sched_barrier(0); (st).t[i] = va_now(); __builtin_amdgcn_sched_barrier(0); } while (0)
// wait until at most n vector-memory operations of this wave are outstanding (loads retire in order)
#define VA_WAIT_VM(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
__device__ __forceinline__ void va_stamp_flush(const VaStamps& st, int kind) {
  unsigned long long* p = va_stamp_ptr;
  if (!p || (threadIdx.x & 63) != 0) return;                 // lane 0: one 128-byte record per wave
  if (p[2] == 0 && threadIdx.x != 0) return;                 // [2] = 0: wave 0 only (least perturbation: read spans and gaps from this mode)
  const unsigned long long slot = atomicAdd(p, 1ull);
  const unsigned long long t7 = va_now();                    // the slot counter's round trip is over: what follows is fire-and-forget
  if (slot >= p[1]) return;
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  unsigned long long* r = p + 8 + slot * 16;
  r[0] = (unsigned long long)kind | ((unsigned long long)(blockIdx.x + gridDim.x * blockIdx.y) << 8) | ((unsigned long long)(xcc & 15u) << 40) |
         ((unsigned long long)(threadIdx.x >> 6) << 48);
#pragma unroll
  for (int i = 0; i < 7; ++i) r[1 + i] = st.t[i];
  r[8] = t7;
}
#define VA_STAMP_DECL(st) VaStamps st = {}
#define VA_STAMP_FLUSH(st, kind) va_stamp_flush(st, kind)
#define VA_STAMP_SETTER(name) extern "C" int name(unsigned long long* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(va_stamp_ptr), &p, sizeof p); }
#else
#define VA_STAMP(st, i) do { } while (0)
#define VA_WAIT_VM(n) do { } while (0)
#define VA_STAMP_DECL(st) do { } while (0)
#define VA_STAMP_FLUSH(st, kind) do { } while (0)
#define VA_STAMP_SETTER(name)
#endif

// ---- launchers implemented across the .hip files (host side, internal)
int va_launch_gemv(const void* w, int wdtype, const float* x, const float* gain, const float* residual, float* out,
                   int64_t rows, int64_t N, int64_t K, int epilogue, float eps, hipStream_t s);
int va_attention_splits(int rows, int n_head, int max_len);   // workgroups per (row, head) for this shape
// One layer's K / V cache as the attention launchers see it.  k / v are typed as the kernels take them (float* whatever the storage: same
// kernarg layout); the elements are fp32 or (dtype = vaura_decoder.kv_dtype = 1 / 2 / 3) fp16 / fp8 e4m3 / scaled e4m3.
struct VaKvCache {
  float *k = nullptr, *v = nullptr;             // (rows, n_head, max_len, 96) elements of the storage
  uint8_t *kscale = nullptr, *vscale = nullptr; // dtype = 3 only (NULL otherwise): one exponent byte per cached vector, (rows, n_head, max_len)
  int dtype = 0, max_len = 0;
};
// layer `layer` of a descriptor's cache: the layer stride in ELEMENTS of the storage (an out-of-range dtype is refused by va_kv_dispatch)
static inline VaKvCache va_kv_cache(const vaura_decoder* d, int layer) {
  const size_t vectors = (size_t)layer * d->rows * d->dims.n_head * (size_t)d->max_len;
  const size_t bytes = vectors * (size_t)(d->dims.d_model / d->dims.n_head) * (d->kv_dtype == 1 ? 2 : (d->kv_dtype == 2 || d->kv_dtype == 3) ? 1 : 4);
  VaKvCache c;
  c.k = reinterpret_cast<float*>(reinterpret_cast<char*>(d->kcache) + bytes);
  c.v = reinterpret_cast<float*>(reinterpret_cast<char*>(d->vcache) + bytes);
  if (d->kv_dtype == 3 && d->kscale && d->vscale) { c.kscale = d->kscale + vectors; c.vscale = d->vscale + vectors; }
  c.dtype = d->kv_dtype; c.max_len = d->max_len;
  return c;
}
// What every attention launcher refuses about a cache: head_dim != 96 and a narrow cache (dtype != 0) of more than 256 positions or under
// a range split are VAURA_ERR_SHAPE (fp16 / fp8 / scaled fp8 have the single-round-trip step kernel only: every 2.56 s configuration),
// scaled e4m3 without its exponent bytes is VAURA_ERR_ARG.  When two apply, the decode step's launcher has always reported the missing
// bytes (arg_first), the two prefill launchers the shape: each keeps its order.
static inline int va_kv_check(const VaKvCache& c, int head_dim, bool range_split, bool arg_first) {
  const bool no_scales = c.dtype == 3 && (!c.kscale || !c.vscale);
  if (arg_first && no_scales) return VAURA_ERR_ARG;
  if (head_dim != 96 || (c.dtype != 0 && (c.max_len > 256 || range_split))) return VAURA_ERR_SHAPE;
  return no_scales ? VAURA_ERR_ARG : 0;
}
// f(std::integral_constant<int, KVT>{}) for the storage `dtype`: the one place that maps vaura_decoder.kv_dtype to a KvT<> instance.
// f returns int: VA_LAUNCH inside a lambda returns the launch error from the lambda, and the launcher passes that on.
template <class F>
static inline int va_kv_dispatch(int dtype, F&& f) {
  switch (dtype) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
  }
  return VAURA_ERR_ARG;
}
struct VaAttentionStep {             // one decode-step attention: rope + cache append + softmax(qK^T)V of `rows` rows at one position
  const float *qkv = nullptr, *qkv2 = nullptr;   // qkv2: second K-half partial of qkv (added on load), or NULL
  const float* rope = nullptr;
  VaKvCache kv;
  float* out = nullptr;              // fp32 packed rows (rows x d_model)
  uint16_t* out_split = nullptr;     // planes for wo, or NULL
  int rows = 0, n_head = 0, head_dim = 0;
  const int32_t* pos_dev = nullptr;  // position on the device (state[0]), or NULL for pos_host
  int pos_host = 0;
  float* part = nullptr;             // partials of the range split (with n_split > 1), or NULL
  int n_split = 1;
  uint32_t* arrivals = nullptr;      // rows * n_head zeroed words: the last split to arrive merges; NULL: a combine launch follows
  float pscale = 1.f;                // scale of the out_split planes (2^-plane_shift)
  // softmax weights of the step (vaura_decoder_ext4): NULL = the instances without them.  (probs_steps, probs_rows, n_head, max_len)
  // fp32; written for rows < probs_rows when probs_pos0 <= position < probs_pos0 + probs_steps
  float* probs = nullptr;
  int probs_pos0 = 0, probs_steps = 0, probs_rows = 0;
};
int va_launch_attention(const VaAttentionStep& a, hipStream_t s);
struct Gemv3Args;
static inline bool va_is_fp8(int wdtype) { return wdtype == VAURA_W_FP8 || wdtype == VAURA_W_FP8H; }   // e4m3 tile pairs (both activation arithmetics)
int va_pack_weight_fp8(const float* src, void* dst, int64_t N, int64_t K, hipStream_t s);
int va_pack_weight_h(const float* src, void* dst, int64_t N, int64_t K, int planes, hipStream_t s);   // fp16 plane(s) + row scales
int va_launch_gemv3(const Gemv3Args& a, int64_t n_weight_rows, int64_t K, int epilogue, bool norm, hipStream_t s);
bool va_mlp_engine_eligible(const vaura_decoder* d);
int va_launch_mlp_engine(const Gemv3Args& a13, const Gemv3Args& a2, const Gemv3Args* aq_next, uint32_t* flags, int32_t* state, int layer,
                         hipStream_t s);
int va_launch_embed(const vaura_decoder* d, int pos_host, int n_pos, hipStream_t s);
// the relevance pointers behind a descriptor (vaura_decoder_ext), or NULL when the caller passed a plain vaura_decoder
inline const vaura_decoder_ext* va_decoder_ext(const vaura_decoder* d) {
  return (d->ext_bytes == (int32_t)(sizeof(vaura_decoder_ext) - sizeof(vaura_decoder)) ||
          d->ext_bytes == (int32_t)(sizeof(vaura_decoder_ext2) - sizeof(vaura_decoder)) ||
          d->ext_bytes == (int32_t)(sizeof(vaura_decoder_ext3) - sizeof(vaura_decoder)) ||
          d->ext_bytes == (int32_t)(sizeof(vaura_decoder_ext4) - sizeof(vaura_decoder)))
             ? reinterpret_cast<const vaura_decoder_ext*>(d) : nullptr;
}
// the per-clip lengths behind those (vaura_decoder_ext2), or NULL
inline const vaura_decoder_ext2* va_decoder_ext2(const vaura_decoder* d) {
  return (d->ext_bytes == (int32_t)(sizeof(vaura_decoder_ext2) - sizeof(vaura_decoder)) ||
          d->ext_bytes == (int32_t)(sizeof(vaura_decoder_ext3) - sizeof(vaura_decoder)) ||
          d->ext_bytes == (int32_t)(sizeof(vaura_decoder_ext4) - sizeof(vaura_decoder)))
             ? reinterpret_cast<const vaura_decoder_ext2*>(d) : nullptr;
}
inline const int32_t* va_clip_timesteps(const vaura_decoder* d) { const vaura_decoder_ext2* x = va_decoder_ext2(d); return x ? x->clip_timesteps : nullptr; }
inline const int32_t* va_clip_cond_tokens(const vaura_decoder* d) { const vaura_decoder_ext2* x = va_decoder_ext2(d); return x ? x->clip_cond_tokens : nullptr; }
// the per-clip prompt lengths behind those (vaura_decoder_ext3): n_r of every row, or NULL
inline const int32_t* va_row_prompt_steps(const vaura_decoder* d) {
  return (d->ext_bytes == (int32_t)(sizeof(vaura_decoder_ext3) - sizeof(vaura_decoder)) ||
          d->ext_bytes == (int32_t)(sizeof(vaura_decoder_ext4) - sizeof(vaura_decoder)))
             ? reinterpret_cast<const vaura_decoder_ext3*>(d)->row_prompt_steps : nullptr;
}
// the attention-map request behind those (vaura_decoder_ext4) when it asks for maps (attn_probs set), or NULL
inline const vaura_decoder_ext4* va_attention_maps(const vaura_decoder* d) {
  if (d->ext_bytes != (int32_t)(sizeof(vaura_decoder_ext4) - sizeof(vaura_decoder))) return nullptr;
  const vaura_decoder_ext4* x = reinterpret_cast<const vaura_decoder_ext4*>(d);
  return x->attn_probs ? x : nullptr;
}
struct VaSampleLaunch {              // one sampler launch over (B, K) rows of logits
  const float* logits = nullptr;
  int B = 0, K = 0, vocab = 0;
  const vaura_sampling* sp = nullptr;
  const vaura_clip_sampling* clips = nullptr;   // per-clip records (vaura_decoder.clip_sampling) or NULL for the scalars of `sp`
  const float* noise = nullptr;
  int32_t* state = nullptr;          // decoder state, or NULL (standalone: step_host).  Feeds the kernel's preloaded `state` argument,
  int64_t step_host = 0;             // SampleArgs.state (position, step: read) and SampleArgs.state_rw (arrivals, advance, status: written)
  int32_t *tokens_out = nullptr, *seq = nullptr;   // (B, K) tokens and / or the pattern sequence (B, K, S) of T timesteps
  int T = 0, S = 0;
  const int32_t* delays_host = nullptr;   // K delays, NULL = the default d_k = k
  float *lp_out = nullptr, *lp_seq = nullptr;     // (B, K) / (B, K, S); either non-NULL selects the LP instances
  // video relevance (mode 2 of step.hip's sampler): lc / lu of the chosen token, (B, K) and / or (B, K, S).  Any of them selects the
  // mode-2 instances; both values are needed, and null_rows = "logits has rows [B, 2B)" (VAURA_ERR_ARG otherwise, before the launch)
  float *cond_out = nullptr, *cond_seq = nullptr, *null_out = nullptr, *null_seq = nullptr;
  bool null_rows = false;
  const int32_t* clip_T = nullptr;        // per-clip timesteps T_b (vaura_decoder_ext2.clip_timesteps) or NULL: every clip has T
  const int32_t* clip_n = nullptr;        // per-clip first sampled positions n_b (vaura_decoder_ext3.row_prompt_steps) or NULL: the loop's step
};
int va_launch_sample(const VaSampleLaunch& a, hipStream_t s);
int va_check_clip_sampling(const vaura_sampling* sp, const vaura_clip_sampling* clips, int B, bool doubled, hipStream_t s);
// host side of the per-clip lengths' contract: B values of `lengths` (device; NULL passes) read back and held to lo .. hi
int va_check_clip_lengths(const int32_t* lengths, int B, int lo, int hi, hipStream_t s);
int va_launch_advance(int32_t* state, int set_to, hipStream_t s);
int va_launch_linear_pair(const uint16_t* in, const uint16_t* w, const float* bias, const float* res, float* out_raw,
                          uint16_t* out_act, int act, int B, int Lin, int Lout, int oshift, int Cin, int Cout, hipStream_t s);
int va_launch_rope_append(const vaura_decoder* d, int layer, int p0, int n_pos, hipStream_t s);
// the same with the K / V append held to the rows r with row_n[r] == n_sel (vaura_prefill_rows)
int va_launch_rope_append_rows(const vaura_decoder* d, int layer, int p0, int n_pos, const int32_t* row_n, int n_sel, hipStream_t s);
int va_launch_attention_prefill(const vaura_decoder* d, int layer, int p0, int n_pos, hipStream_t s);
// teacher-forced scoring (score.hip); clip_T: per-clip timesteps (vaura_decoder_ext2.clip_timesteps) or NULL: every clip has Ta
int va_launch_score_nll(const float* logits, int rows_per_pos, int p0, int n_pos, int B, int K, int V, int Ta, const int32_t* delays_host,
                        const int32_t* targets, float* nll, float* logits_out, const int32_t* clip_T, hipStream_t s);
int va_launch_score_reduce(float* nll, uint8_t* mask, float* logits_out, int B, int K, int V, int Ta, int n_scored, const int32_t* delays_host,
                           float* loss_per_cb, float* loss, const int32_t* clip_T, hipStream_t s);

// Epoch of an in-launch hand-off (mlp_engine.h): neither the flag words in global memory nor the arrival
// words in LDS are ever reset — a hand-off passes when every producer's word holds THIS launch's epoch — so no two launches that can
// see each other's words may share an epoch.  epoch = (sequence id state[3], 10 bits | launch-epoch counter state[5], 17 bits | layer)
// + 1.  state[5] is OWNED BY THE LIBRARY: bumped by whatever ends a decode step (the sampler's last workgroup, advance_kernel), never
// rewound — a caller that rewinds the position (state[0]) within a sequence still gets fresh epochs (round 4's epoch used state[0] and
// matched stale words when a (sequence, position) step was re-run).  state[3] is the CALLER's: a new value for every sequence start
// and for every decoder instance of the process — LDS keeps its words across launches and instances, so a state buffer that starts
// from zero again must come with a new sequence id (DecoderEngine._reset_state: a process-wide counter).
__device__ __forceinline__ uint32_t va_handoff_epoch(const int32_t* state, int layer) {
  return ((((uint32_t)state[3] & 0x3ffu) << 22) | (((uint32_t)state[5] & 0x1ffffu) << 5) | ((uint32_t)layer & 31u)) + 1u;
}
