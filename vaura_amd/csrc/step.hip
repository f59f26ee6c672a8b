// Per-step bookkeeping kernels around the layer stack: input embedding, next-token selection,
// delay-pattern build / revert.
//
//   embed    models/modules/sampler/llama.py:455-472, 555-586  (token projection sum + video concat)
//   sample   models/vaura_model.py:807-825, 536-544; utils/utils.py:139-196
//   pattern  models/modules/misc/codebook_patterns.py:137-285, 374-419 (delay patterns, closed form)
#include <vector>
#include "common.h"
#include "gemv3_kernel.h"

// ------------------------------------------------------------------------------------ embed
// Token projection table, built once per weight set with the arithmetic of the reference's
// DacEmbeddingProjection (llama.py:70-73): table[k][tok][c] = sum_i W_k[c][i] * emb_k[tok][i] + b_k[c]
__global__ void token_table_kernel(const float* __restrict__ tok_emb, const float* __restrict__ proj_w,
                                   const float* __restrict__ proj_b, float* __restrict__ table, int K, int vocab1,
                                   int cdim, int tok_dim) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)K * vocab1 * tok_dim;
  if (i >= total) return;
  const int c = (int)(i % tok_dim);
  const int tok = (int)((i / tok_dim) % vocab1);
  const int k = (int)(i / ((int64_t)tok_dim * vocab1));
  const float* e = tok_emb + ((size_t)k * vocab1 + tok) * cdim;
  const float* wr = proj_w + ((size_t)k * tok_dim + c) * cdim;
  float z = 0.f;
  for (int j = 0; j < cdim; ++j) z = fmaf(wr[j], e[j], z);
  table[i] = z + proj_b[(size_t)k * tok_dim + c];
}

// h0[row] = [ cond(row, pos // tpf) | sum_k table_k[tok(row % B, k, pos)] ]  -> packed rows (+ split rows
// of h0 * gain and per-16-column partial sums of squares for the first fused RMSNorm)
__global__ __launch_bounds__(64) void embed_kernel(
    const int32_t* __restrict__ seq, const int32_t* __restrict__ state, const float* __restrict__ cond_proj,
    const float* __restrict__ empty_video, const float* __restrict__ table, float* __restrict__ h,
    uint16_t* __restrict__ hsplit, const float* __restrict__ gain, float* __restrict__ ss, int B, int K, int S, int Tv,
    int tpf, int vocab1, int cond_dim, int tok_dim, int pos_host, int rows16) {
  const int row = blockIdx.x;
  const int cq = blockIdx.y * 64 + threadIdx.x;   // 4-column quad
  const int b = row % B;
  // decode: the position lives on the device; prefill: positions pos_host + blockIdx.z, one row block
  // (rows16 = padded row count) per position
  const int pos = pos_host >= 0 ? pos_host + (int)blockIdx.z : state[0];
  const int vrow = (int)blockIdx.z * rows16 + row;
  const int D = cond_dim + tok_dim;
  const int frame = pos / tpf;
  f32x4 o;
  if (cq < cond_dim / 4) {
    if (frame < Tv)
      o = reinterpret_cast<const f32x4*>(cond_proj)[packed_quad(row * Tv + frame, cq, cond_dim)];
    else
      o = reinterpret_cast<const f32x4*>(empty_video)[cq];
  } else {
    const int c0 = (cq - cond_dim / 4) * 4;
    o = f32x4{0.f, 0.f, 0.f, 0.f};
    int tok[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) tok[k] = (k < K) ? seq[((size_t)b * K + k) * S + pos] : 0;
    f32x4 e[16];
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < K) e[k] = *reinterpret_cast<const f32x4*>(table + ((size_t)k * vocab1 + tok[k]) * tok_dim + c0);
#pragma unroll
    for (int k = 0; k < 16; ++k)    // same left-to-right order as the reference's sum([...]) (llama.py:455-460)
      if (k < K) o += e[k];
  }
  va_st16(reinterpret_cast<f32x4*>(h) + packed_quad(vrow, cq, D), o);
  if (hsplit) {
    float s = ((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) + o[3] * o[3];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if ((threadIdx.x & 3) == 0) va_st4(ss + ((size_t)(vrow >> 4) * (D / 16) + (cq >> 2)) * 16 + (vrow & 15), s);
    const f32x4 u = o * *reinterpret_cast<const f32x4*>(gain + cq * 4);
    store_split4(hsplit, vrow, cq * 4, D, u);
  }
}

// embed_kernel with per-clip video lengths (vaura_decoder_ext2.clip_cond_tokens): only the first Tv_b = clip_tv[b] video tokens of clip
// b = row % B are real — the null-condition row of a clip follows its clip —, frames from Tv_b on take empty_video; the row stride of
// cond_proj stays Tv.  One vector load per workgroup (the host rewrites the array between replays of one captured graph: the vector
// path is the one that is coherent with those copies), clamped to Tv so that no value can send the gather out of its rows.  A copy
// of the kernel above and not a shared inlined body: that changed the operand order of embed_kernel's address arithmetic, and the
// kernel every existing call runs stays the instruction stream it was.
__global__ __launch_bounds__(64) void embed_clips_kernel(
    const int32_t* __restrict__ seq, const int32_t* __restrict__ state, const float* __restrict__ cond_proj,
    const float* __restrict__ empty_video, const float* __restrict__ table, float* __restrict__ h,
    uint16_t* __restrict__ hsplit, const float* __restrict__ gain, float* __restrict__ ss, int B, int K, int S, int Tv,
    int tpf, int vocab1, int cond_dim, int tok_dim, int pos_host, int rows16, const int32_t* __restrict__ clip_tv) {
  const int row = blockIdx.x;
  const int cq = blockIdx.y * 64 + threadIdx.x;   // 4-column quad
  const int b = row % B;
  int lane0 = 0;
  asm volatile("" : "+v"(lane0));
  const int tv_b = min(__builtin_amdgcn_readfirstlane(clip_tv[b + lane0]), Tv);
  // decode: the position lives on the device; prefill: positions pos_host + blockIdx.z, one row block
  // (rows16 = padded row count) per position
  const int pos = pos_host >= 0 ? pos_host + (int)blockIdx.z : state[0];
  const int vrow = (int)blockIdx.z * rows16 + row;
  const int D = cond_dim + tok_dim;
  const int frame = pos / tpf;
  f32x4 o;
  if (cq < cond_dim / 4) {
    if (frame < tv_b)
      o = reinterpret_cast<const f32x4*>(cond_proj)[packed_quad(row * Tv + frame, cq, cond_dim)];
    else
      o = reinterpret_cast<const f32x4*>(empty_video)[cq];
  } else {
    const int c0 = (cq - cond_dim / 4) * 4;
    o = f32x4{0.f, 0.f, 0.f, 0.f};
    int tok[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) tok[k] = (k < K) ? seq[((size_t)b * K + k) * S + pos] : 0;
    f32x4 e[16];
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < K) e[k] = *reinterpret_cast<const f32x4*>(table + ((size_t)k * vocab1 + tok[k]) * tok_dim + c0);
#pragma unroll
    for (int k = 0; k < 16; ++k)    // same left-to-right order as the reference's sum([...]) (llama.py:455-460)
      if (k < K) o += e[k];
  }
  va_st16(reinterpret_cast<f32x4*>(h) + packed_quad(vrow, cq, D), o);
  if (hsplit) {
    float s = ((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) + o[3] * o[3];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if ((threadIdx.x & 3) == 0) va_st4(ss + ((size_t)(vrow >> 4) * (D / 16) + (cq >> 2)) * 16 + (vrow & 15), s);
    const f32x4 u = o * *reinterpret_cast<const f32x4*>(gain + cq * 4);
    store_split4(hsplit, vrow, cq * 4, D, u);
  }
}

int va_launch_embed(const vaura_decoder* d, int pos_host, int n_pos, hipStream_t s) {
  const vaura_dims& m = d->dims;
  const int D = m.cond_dim + m.tok_dim;
  if (!d->tok_table || (D % 256)) return VAURA_ERR_SHAPE;
  const bool split = d->wdtype == VAURA_W_H1 || d->wdtype == VAURA_W_H2 || va_is_fp8(d->wdtype);   // pair path (api.hip enqueue_step)
  if (split && (!d->ws_h_split || !d->ws_ss || !d->first_norm)) return VAURA_ERR_ARG;
  if (const int32_t* clip_tv = va_clip_cond_tokens(d)) {
    VA_LAUNCH(embed_clips_kernel, dim3(d->rows, D / 256, n_pos), dim3(64), 0, s, d->seq, d->state, d->cond_proj, d->empty_video,
              d->tok_table, d->ws_h, split ? d->ws_h_split : nullptr, d->first_norm, d->ws_ss, d->batch, m.n_codebooks,
              d->seq_len, d->n_cond_tokens, m.tokens_per_frame, m.vocab + 1, m.cond_dim, m.tok_dim, pos_host,
              (d->rows + 15) / 16 * 16, clip_tv);
    return 0;
  }
  VA_LAUNCH(embed_kernel, dim3(d->rows, D / 256, n_pos), dim3(64), 0, s, d->seq, d->state, d->cond_proj, d->empty_video,
            d->tok_table, d->ws_h, split ? d->ws_h_split : nullptr, d->first_norm, d->ws_ss, d->batch, m.n_codebooks,
            d->seq_len, d->n_cond_tokens, m.tokens_per_frame, m.vocab + 1, m.cond_dim, m.tok_dim, pos_host,
            (d->rows + 15) / 16 * 16);
  return 0;
}

// ------------------------------------------------------------------------------------ live condition window
// The condition buffer of a live session (include/vaura_hip.h vaura_cond_window): cond_proj is baked into the captured step graph, so
// the window slides IN PLACE.  One work item per (decoder row, column quad), walking the tokens in ascending order: token j + shift is
// read before token j is written, and an item touches no address another item touches — no LDS, no barrier, no atomics.  A
// conditional row moves tokens [shift, Tv) down to [0, Tv - shift) and takes its n fresh tokens from new_rows (packed rows, row index
// row * n + t); a null-condition row (row >= B, CFG engines) does not move — the null embedding belongs to the window POSITION, not to
// the video's clock — and takes tokens [first, first + n) of null_rows (packed rows, row index = token).  16-byte loads and stores only.
__global__ __launch_bounds__(64) void cond_window_kernel(float* cond_proj, const float* __restrict__ new_rows,
                                                         const float* __restrict__ null_rows, int B, int Tv, int cond_dim, int shift,
                                                         int first, int n) {
  const int row = blockIdx.x;
  const int cq = blockIdx.y * 64 + threadIdx.x;   // 4-column quad
  if (cq >= cond_dim / 4) return;
  f32x4* dst = reinterpret_cast<f32x4*>(cond_proj);
  if (row >= B) {
    for (int t = 0; t < n; ++t)
      dst[packed_quad(row * Tv + first + t, cq, cond_dim)] = reinterpret_cast<const f32x4*>(null_rows)[packed_quad(first + t, cq, cond_dim)];
    return;
  }
  if (shift > 0)
    for (int j = 0; j + shift < Tv; ++j) {
      const f32x4 v = dst[packed_quad(row * Tv + j + shift, cq, cond_dim)];
      dst[packed_quad(row * Tv + j, cq, cond_dim)] = v;
    }
  for (int t = 0; t < n; ++t)
    dst[packed_quad(row * Tv + first + t, cq, cond_dim)] = reinterpret_cast<const f32x4*>(new_rows)[packed_quad(row * n + t, cq, cond_dim)];
}

extern "C" int vaura_cond_window(const vaura_decoder* d, const float* new_rows, const float* null_rows, int shift_tokens,
                                 int first_token, int n_tokens, vaura_stream_t s) {
  if (!d || !d->cond_proj || !new_rows) return VAURA_ERR_ARG;
  const int Tv = d->n_cond_tokens, cd = d->dims.cond_dim;
  if (d->batch <= 0 || Tv <= 0 || (d->rows != d->batch && d->rows != 2 * d->batch)) return VAURA_ERR_ARG;
  if (d->rows != d->batch && !null_rows) return VAURA_ERR_ARG;
  if (shift_tokens < 0 || first_token < 0 || n_tokens <= 0) return VAURA_ERR_ARG;
  if (shift_tokens > Tv || (int64_t)first_token + n_tokens > Tv) return VAURA_ERR_SHAPE;
  if (cd <= 0 || (cd % 4)) return VAURA_ERR_SHAPE;
  VA_LAUNCH(cond_window_kernel, dim3(d->rows, (cd / 4 + 63) / 64), dim3(64), 0, as_stream(s), const_cast<float*>(d->cond_proj), new_rows,
            null_rows, d->batch, Tv, cd, shift_tokens, first_token, n_tokens);
  return 0;
}

extern "C" int vaura_build_token_table(const float* tok_emb, const float* proj_w, const float* proj_b, float* table, int K,
                                       int vocab1, int cdim, int tok_dim, vaura_stream_t s) {
  if (!tok_emb || !proj_w || !proj_b || !table || K <= 0) return VAURA_ERR_ARG;
  const int64_t total = (int64_t)K * vocab1 * tok_dim;
  VA_LAUNCH(token_table_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(s), tok_emb, proj_w, proj_b,
            table, K, vocab1, cdim, tok_dim);
  return 0;
}

// ------------------------------------------------------------------------------------ sampling
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct SampleArgs {
  const float* logits;   // (rows, K*V) row-major
  const float* noise;    // (steps, B*K, V) or null
  const int32_t* state;  // device {pos, arrivals, step} or null
  int32_t* state_rw;     // same buffer, writable, or null (standalone)
  int32_t* tokens_out;   // (B, K) or null
  int32_t* seq;          // (B, K, S) or null
  int B, K, V, T, S;
  int32_t delays[16];    // pattern delay of codebook k < 16 (seq != null): step s of codebook k holds timestep s - 1 - delays[k]
  int use_sampling, top_k, probs_in;
  float temp, top_p, cfg_scale;
  float tie_eps;         // near-tie detector (vaura_sampling.tie_eps): relative bound on a logit's error, 0 = off
  uint64_t seed, clip_base;
  long long step_host;
};

#define SMP_THREADS 256

__device__ __forceinline__ void block_argmax(float v, int i, float* sv, int* si, float& bv, int& bi) {
  // first-index-wins argmax over the block (torch.argmax returns the first maximal index)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
  __syncthreads();
  bv = sv[0]; bi = si[0];
#pragma unroll
  for (int w = 1; w < SMP_THREADS / 64; ++w)
    if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
}

__device__ __forceinline__ float block_sum(float v, float* sv) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sv[0] + sv[1]) + sv[2]) + sv[3];
}
__device__ __forceinline__ float block_max(float v, float* sv) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
}
// two maxima with ONE barrier pair (the near-tie detector's scale next to the softmax's maximum)
__device__ __forceinline__ void block_max2(float& a, float& b, float* sv) {
  a = wave_max(a);
  b = wave_max(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = a; sv[4 + (threadIdx.x >> 6)] = b; }
  __syncthreads();
  a = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
  b = fmaxf(fmaxf(sv[4], sv[5]), fmaxf(sv[6], sv[7]));
}
// the near-tie screen's four quantities with ONE barrier pair: two maxima and two counts
__device__ __forceinline__ void block_tie4(float& m0, float& m1, int& c0, int& c1, float* sv, int* si) {
  m0 = wave_max(m0);
  m1 = wave_max(m1);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { c0 += __shfl_xor(c0, o, 64); c1 += __shfl_xor(c1, o, 64); }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    const int wv = threadIdx.x >> 6;
    sv[wv] = m0; sv[4 + wv] = m1; si[wv] = c0; si[4 + wv] = c1;
  }
  __syncthreads();
  m0 = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
  m1 = fmaxf(fmaxf(sv[4], sv[5]), fmaxf(sv[6], sv[7]));
  c0 = si[0] + si[1] + si[2] + si[3];
  c1 = si[4] + si[5] + si[6] + si[7];
}
__device__ __forceinline__ int block_count(int v, int* si) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) si[threadIdx.x >> 6] = v;
  __syncthreads();
  return si[0] + si[1] + si[2] + si[3];
}

// V == 1024 == 4 * SMP_THREADS: thread t owns candidates 4t .. 4t+3
// PC (per-clip parameters, vaura_decoder.clip_sampling): the workgroup of clip b = blockIdx.y takes use_sampling / temp / top_k / top_p /
// cfg_scale from record b of `clips` instead of the launch's scalars; everything below reads them through `a` either way.  PC = false
// is the scalar launch as it always was: the fetch is compiled out and `clips` (NULL) is never read.
// LP (token log-probabilities, vaura_decoder.logprobs / vaura_sample_logprobs): the kernel also reports log softmax(x / tau)[token] of the
// decision it made — x the CFG-mixed, sanitised logits, tau = temp where the clip samples and 1 where it is greedy, over the FULL
// vocabulary (before any top-k / top-p cut).  The sampled branch keeps the maximum and the denominator its draw used; the greedy branch
// pays one block_max and one block_sum more, same order.  The thread that owns the token's column does the epilogue (tid 0 otherwise) and
// stores the value next to the token.  LP = false compiles all of it out: those two instances are the kernels they were.
// The two output pointers travel as a trailing parameter PACK that is empty when LP = false: those instances keep the argument list, and
// with it the kernel-argument offsets, of the kernels they were (an extra pointer would move the hidden arguments behind it).
// The reporting MODE of an instance: 0 = none (LP = false, empty pack), 1 = the log-probability (LP = true, pack = SampleLogprobs), 2 = that
// plus the video relevance of the token (LP = true, pack = SampleRelevance; vaura_decoder_ext.logprobs_cond / logprobs_null,
// vaura_sample_relevance).  Mode 2 is told by the TYPE of the pack, not by a third template value: the four instances of modes 0 and 1
// keep their symbols, argument lists and instruction streams.  Mode 2 needs the null-condition rows [B, 2B) (refused on the host
// otherwise) and reports, for the token the workgroup chose, its log-probability under the model's two distributions, tau = 1:
//     lc = (x_c[tok] - max x_c) - logf(sum expf(x_c - max x_c))      x_c: the conditional row of (clip, codebook), as the mix reads it
//     lu = (x_u[tok] - max x_u) - logf(sum expf(x_u - max x_u))      x_u: the null row of the same prefix
// over the FULL vocabulary, no temperature, no top-k / top-p cut: a property of the model, not of the sampling settings.  Reduction
// order, per row, that of the mode-1 greedy branch: thread t takes the maximum of its candidates 4t .. 4t+3, block max (wave_max, then
// the four waves fmaxf(fmaxf(w0, w1), fmaxf(w2, w3))); thread t adds (e0 + e1) + (e2 + e3) of e_j = expf(x_j - max), block sum (wave_sum,
// then ((w0 + w1) + w2) + w3).  The two rows share each barrier pair (block_max2 / block_sum2: the same arithmetic).  A clip whose own
// scale is <= 1 still skips the mix for its token; its null row is read for lu only.  The thread that owns the token's column stores
// both values with ordinary vector stores, where — and only where — lp is stored.  NaN in both when either row (or their mix) holds a
// non-finite value; the status bit is raised for that as well (a null row the un-mixed draw never read is no draw error, but the
// values are not to be used).  The token never depends on the mode: everything of mode 2 happens after the draw.
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
struct SampleLogprobs {
  float* out;   // (B, K) next to tokens_out, or null
  float* seq;   // (B, K, S) in the layout of seq, or null
};
struct SampleRelevance {
  float* out;   // as SampleLogprobs
  float* seq;
  float* cond_out;   // lc: (B, K) or null
  float* cond_seq;   // lc: (B, K, S) in the layout of seq, or null
  float* null_out;   // lu: (B, K) or null
  float* null_seq;   // lu: (B, K, S) or null
};
// The per-clip LENGTHS of an instance (vaura_decoder_ext2.clip_timesteps): one more member of the pack, behind the reporting one where
// there is one — told by its type, like mode 2: the six instances without it keep their symbols, argument lists and instruction
// streams.  With it the workgroup of clip b takes T_b = T[b] for a.T, i.e. wherever a slot's validity is decided (the fix-up, the
// lp / lc / lu writes into the sequence layout, the near-tie count): a slot whose timestep is >= T_b gets the special token, and nothing
// of the clip is reported or counted there — the launch with a.T = T_b.  One vector load per workgroup, for the reason given at PC.
struct SampleLengths {
  const int32_t* T;   // (B) timesteps of every clip, 1 .. a.T (checked on the host; a larger value only keeps slots valid that a.S bounds anyway)
};
// The per-clip first sampled POSITIONS of an instance (vaura_decoder_ext3.row_prompt_steps): one more member of the pack, always its
// last — told by its type, like the lengths: the twelve instances without it keep their symbols, argument lists and instruction
// streams.  With it the workgroup of clip b keys its Philox counter by pos - n[b], the step index the call with that clip's prompt
// alone has at this position, instead of the loop's step; an explicit noise tensor and the near-tie detector's "first flagged step"
// keep the loop's step.  One vector load per workgroup, for the reason given at PC.
struct SampleStarts {
  const int32_t* n;   // (B) position of every clip's first sampled step, 0 .. a.S - 1 (checked on the host; the value only enters the counter)
};
template <typename T, typename... R>
__device__ __forceinline__ T va_first(T t, R...) { return t; }
// the member of a pack that has type W (the lengths and the first positions, wherever they stand behind the reporting member)
template <typename W, typename T, typename... R>
__device__ __forceinline__ W va_pick(T t, R... r) {
  if constexpr (std::is_same<T, W>::value) return t;
  else return va_pick<W>(r...);
}
// two sums with ONE barrier pair (block_sum's order for each)
__device__ __forceinline__ void block_sum2(float& a, float& b, float* sv) {
  a = wave_sum(a);
  b = wave_sum(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = a; sv[4 + (threadIdx.x >> 6)] = b; }
  __syncthreads();
  a = ((sv[0] + sv[1]) + sv[2]) + sv[3];
  b = ((sv[4] + sv[5]) + sv[6]) + sv[7];
}
template <bool PC, bool LP, typename... LpArgs>
__global__ __launch_bounds__(SMP_THREADS) void sample_kernel(const float* __restrict__ logits_q, const int32_t* __restrict__ state_q,
                                                             SampleArgs a, const int32_t* __restrict__ clips, LpArgs... lp_args) {
  constexpr bool REL = (std::is_same<LpArgs, SampleRelevance>::value || ...);      // mode 2
  constexpr bool CL = (std::is_same<LpArgs, SampleLengths>::value || ...);         // per-clip lengths
  constexpr bool ST = (std::is_same<LpArgs, SampleStarts>::value || ...);          // per-clip first sampled positions
  static_assert(sizeof...(LpArgs) == (LP ? 1 : 0) + (CL ? 1 : 0) + (ST ? 1 : 0),
                "LP instances take one SampleLogprobs / SampleRelevance, the others nothing; SampleLengths follows where the clips have lengths, SampleStarts last");
  [[maybe_unused]] float* lp_out = nullptr;
  [[maybe_unused]] float* lp_seq = nullptr;
  if constexpr (LP) { lp_out = va_first(lp_args...).out; lp_seq = va_first(lp_args...).seq; }
  a.logits = logits_q;   // explicit scalar copies: preloaded into SGPRs at wave launch (the struct is not)
  a.state = state_q;
  __shared__ float sv[8];
  __shared__ int si[8];
  __shared__ float sp[1024];   // top-p: sorted probabilities
  __shared__ int sidx[1024];   // top-p: their token ids
  __shared__ float skeep[1024];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_sel[2];
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int pos = a.state ? a.state[0] : 0;
  const long long step = a.state ? (long long)a.state[2] : a.step_host;
  const int V = a.V;

  const f32x4 lc = *reinterpret_cast<const f32x4*>(a.logits + ((size_t)b * a.K + k) * V + 4 * tid);
  if constexpr (PC) {
    // This clip's record, requested right behind its logits so that it waits under the same latency.  Two VECTOR loads, 16 + 4 bytes (five fields)
    // (the opaque lane offset keeps the address out of the scalar unit: the host rewrites the records between replays of one
    // captured graph, and the vector path is the one that is coherent with those copies); the fields are wave-uniform, so they go
    // back to SGPRs and every branch on them stays a scalar branch, as in the scalar instance.
    int lane0 = 0;
    asm volatile("" : "+v"(lane0));
    const int32_t* rec = clips + (size_t)b * (sizeof(vaura_clip_sampling) / 4) + lane0;
    const i32x4 r0 = *reinterpret_cast<const i32x4*>(rec);
    const int32_t r1 = rec[4];
    a.use_sampling = __builtin_amdgcn_readfirstlane(r0[0]);
    a.temp = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(r0[1]));
    a.top_k = __builtin_amdgcn_readfirstlane(r0[2]);
    a.top_p = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(r0[3]));
    const float cfg = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(r1));
    // the launch's scalar cfg_scale > 1 says that the null-condition rows [B, 2B) exist; a clip whose own scale is <= 1 skips the mix
    // (no lu + (x - lu) * 1: not the same bits), never reads them, and screens near-ties with factor 1 — the scalar path at
    // cfg_scale <= 1.  Without those rows no record can switch the mix on (refused on the host; clamped here: never out of bounds).
    a.cfg_scale = a.cfg_scale > 1.0f ? cfg : fminf(cfg, 1.0f);
  }
  if constexpr (CL) {      // this clip's timesteps: everything below reads them through `a`, like the per-clip parameters
    int lane0 = 0;
    asm volatile("" : "+v"(lane0));
    a.T = __builtin_amdgcn_readfirstlane(va_pick<SampleLengths>(lp_args...).T[b + lane0]);
  }
  [[maybe_unused]] long long cstep = 0;      // ST only: this clip's own step index, the Philox counter's
  if constexpr (ST) {
    int lane0 = 0;
    asm volatile("" : "+v"(lane0));
    cstep = (long long)pos - (long long)__builtin_amdgcn_readfirstlane(va_pick<SampleStarts>(lp_args...).n[b + lane0]);
  }
  float x[4] = {lc[0], lc[1], lc[2], lc[3]};
  // near-tie detector: magnitude of the rows this decision is made from (both branches, before the mix)
  float amax = fmaxf(fmaxf(fabsf(lc[0]), fabsf(lc[1])), fmaxf(fabsf(lc[2]), fabsf(lc[3])));
  if (a.cfg_scale > 1.0f) {  // models/vaura_model.py:810-813
    const f32x4 lu = *reinterpret_cast<const f32x4*>(a.logits + ((size_t)(a.B + b) * a.K + k) * V + 4 * tid);
    amax = fmaxf(amax, fmaxf(fmaxf(fabsf(lu[0]), fabsf(lu[1])), fmaxf(fabsf(lu[2]), fabsf(lu[3]))));
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = lu[j] + (x[j] - lu[j]) * a.cfg_scale;
  }
  // Near-tie detector (round 6).  The plane storages carry 22-bit operands where the reference computes fp32: a logit reaches the
  // sampler with an error of at most ~tie_eps x (the row's largest |logit|), and the CFG mix s lc - (s - 1) lu multiplies that by up
  // to 2 s - 1.  A decision whose own margin is inside twice that bound could have gone the other way in the reference's arithmetic
  // (or in ANY fp32 summation order: the reference's logits themselves move by ~3e-6 with the prefix length it re-feeds).  Such
  // decisions are COUNTED (state[6]; state[7] = first such step + 1) and raise the sticky VAURA_STATUS_NEAR_TIE bit; the token chosen
  // is never changed here.  What the host does with it is policy (engine.py near_tie: report | rerun on the exact-fp32 twin).
  bool near_tie = false;
  float tie_delta = 0.f;       // absolute bound on a mixed logit's error
  [[maybe_unused]] int lp_bad = 0;                         // LP only
  [[maybe_unused]] float lp_mx = 0.f, lp_den = 1.f;        // LP only: maximum and denominator of softmax(x / tau)
  const bool tie_on = a.tie_eps > 0.f && !a.probs_in;
  const float tie_mix = a.tie_eps * (a.cfg_scale > 1.0f ? 2.f * a.cfg_scale - 1.f : 1.f);
  if (tie_on && !(a.use_sampling && a.temp > 0.0f)) tie_delta = tie_mix * block_max(amax, sv);      // greedy: its own reduction; sampled: with the softmax's maximum
  // Range guard of the fp16-plane activation format (gemv3_kernel.h split2): an activation beyond fp16's 65504 becomes inf in its
  // hi plane, inf - inf = NaN in the lo plane, and from there NaN in the residual stream of that row for the rest of the clip —
  // so EVERY overflow anywhere in the step (or in a teacher-forced prefix, through the K/V cache) arrives here as a non-finite
  // logit.  Raise the sticky status bit the host checks after generate() instead of sampling from garbage.
  if (!(fabsf(x[0]) < INFINITY && fabsf(x[1]) < INFINITY && fabsf(x[2]) < INFINITY && fabsf(x[3]) < INFINITY)) {
    if (a.state_rw) __hip_atomic_fetch_or(&a.state_rw[4], VAURA_STATUS_NONFINITE_LOGITS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // ... and keep the rest of this launch on finite numbers: the selection networks below (radix select on the IEEE bits, the
    // bitonic sort, argmax of p / q) are written for ordered values; on NaN they can return an index outside the codebook, which
    // the NEXT step's embedding gather would follow out of its table (round 5: a memory fault, seen on the x3000 checkpoint under
    // top-k sampling).  The token drawn from the sanitised row is meaningless — the status bit says so — but it is a valid id.
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = fabsf(x[j]) < INFINITY ? x[j] : 0.f;
    if constexpr (LP) lp_bad = 1;
  }
  if constexpr (LP) lp_bad = __syncthreads_or(lp_bad);     // the row held an inf / NaN somewhere: its score is NaN, like its status bit

  int token;
  if (!(a.use_sampling && a.temp > 0.0f)) {
    float bv = x[0]; int bi = 4 * tid;
#pragma unroll
    for (int j = 1; j < 4; ++j) if (x[j] > bv) { bv = x[j]; bi = 4 * tid + j; }
    float rv; int ri;
    block_argmax(bv, bi, sv, si, rv, ri);
    token = ri;
    if (tie_delta > 0.f) {     // runner-up of the mixed logits: the argmax could flip when top-1 - top-2 < 2 delta
      float second = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) if (4 * tid + j != ri) second = fmaxf(second, x[j]);
      second = block_max(second, sv);
      near_tie = (rv - second) < 2.f * tie_delta;
    }
    if constexpr (LP) {        // tau = 1: the reductions of the sampled branch, in its order
      lp_mx = block_max(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), sv);
      float e[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = expf(x[j] - lp_mx);
      lp_den = block_sum((e[0] + e[1]) + (e[2] + e[3]), sv);
    }
  } else {
    // softmax(logits / temp) — or the input rows themselves when they already are probabilities (utils/utils.py:139-196)
    float p[4];
    if (a.probs_in) {
#pragma unroll
      for (int j = 0; j < 4; ++j) p[j] = x[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = x[j] / a.temp;
      float mx = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
      if (tie_on) {
        block_max2(mx, amax, sv);
        tie_delta = tie_mix * amax;
      } else {
        mx = block_max(mx, sv);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) p[j] = expf(x[j] - mx);
      const float den = block_sum((p[0] + p[1]) + (p[2] + p[3]), sv);
#pragma unroll
      for (int j = 0; j < 4; ++j) p[j] = p[j] / den;
      if constexpr (LP) { lp_mx = mx; lp_den = den; }      // the values the draw uses
    }

    // Exp(1) draws for this (clip, codebook, step)
    float q[4];
    if (a.noise) {
      const f32x4 nz = *reinterpret_cast<const f32x4*>(a.noise + (((size_t)step * a.B + b) * a.K + k) * V + 4 * tid);
      q[0] = nz[0]; q[1] = nz[1]; q[2] = nz[2]; q[3] = nz[3];
    } else {
      uint32_t r[4];
      const uint64_t clip = a.clip_base + (uint64_t)b;
      philox4x32_10((uint32_t)tid, ST ? (uint32_t)cstep : (uint32_t)step, (uint32_t)(clip * (uint64_t)a.K + k), (uint32_t)((clip * a.K + k) >> 32),
                    (uint32_t)a.seed, (uint32_t)(a.seed >> 32), r);
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = -logf(((float)r[j] + 0.5f) * 2.3283064365386963e-10f);
    }

    if (a.top_p > 0.0f) {
      // utils/utils.py:181-196 — sort descending (ties: lower id first), sequential cumsum, cut, renormalise,
      // draw in sorted space with the noise indexed by RANK, map back.
      // Bitonic network over the 1024 (probability, id) pairs, element 4 tid + j in thread tid's registers.  A stage of stride st compares
      // element i with i ^ st: strides 1, 2 stay inside a thread, 4 .. 128 are lane exchanges inside a wave (xor of the lane by st / 4),
      // only 256 and 512 (three of the 55 stages) cross waves and go through LDS with barriers.  Same comparisons as the LDS network
      // of rounds 1-3 (ties: lower id first): the same order, bit for bit (round 4: the top-p launch 52 -> 36.5 us; the network is ~20 us of
      // it, the sequential sum below ~10: tools/time_sampler.py).
      float sp_r[4];
      int id_r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { sp_r[j] = p[j]; id_r[j] = 4 * tid + j; }
      auto cmpx = [&](int j, float py, int idy, int st, int sz) {
        const int i = 4 * tid + j;
        const bool lower = (i & st) == 0;
        const bool desc = ((i & ~st) & sz) == 0;            // direction of the pair = that of its lower index
        const bool x_first = (sp_r[j] > py) || (sp_r[j] == py && id_r[j] < idy);
        const bool keep_x = (lower == desc) ? x_first : !x_first;
        if (!keep_x) { sp_r[j] = py; id_r[j] = idy; }
      };
      for (int sz = 2; sz <= 1024; sz <<= 1) {
        for (int st = sz >> 1; st > 0; st >>= 1) {
          if (st == 1) {           // (static register indices: a run-time `j ^ st` would send the arrays to scratch)
            const float py[4] = {sp_r[1], sp_r[0], sp_r[3], sp_r[2]};
            const int iy[4] = {id_r[1], id_r[0], id_r[3], id_r[2]};
#pragma unroll
            for (int j = 0; j < 4; ++j) cmpx(j, py[j], iy[j], 1, sz);
          } else if (st == 2) {
            const float py[4] = {sp_r[2], sp_r[3], sp_r[0], sp_r[1]};
            const int iy[4] = {id_r[2], id_r[3], id_r[0], id_r[1]};
#pragma unroll
            for (int j = 0; j < 4; ++j) cmpx(j, py[j], iy[j], 2, sz);
          } else if (st < 256) {
            float py[4]; int iy[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { py[j] = __shfl_xor(sp_r[j], st >> 2, 64); iy[j] = __shfl_xor(id_r[j], st >> 2, 64); }
            // stride >= 4: whether this thread's four elements are the lower ones of their pairs, and the pairs' direction, do not depend on j
            const bool want_first = (((4 * tid) & st) == 0) == ((((4 * tid) & ~st) & sz) == 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const bool x_first = (sp_r[j] > py[j]) || (sp_r[j] == py[j] && id_r[j] < iy[j]);
              if (x_first != want_first) { sp_r[j] = py[j]; id_r[j] = iy[j]; }
            }
          } else {
            __syncthreads();                                 // (the previous exchange's reads are done)
#pragma unroll
            for (int j = 0; j < 4; ++j) { sp[4 * tid + j] = sp_r[j]; sidx[4 * tid + j] = id_r[j]; }
            __syncthreads();
            float py[4]; int iy[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { py[j] = sp[(4 * tid + j) ^ st]; iy[j] = sidx[(4 * tid + j) ^ st]; }
#pragma unroll
            for (int j = 0; j < 4; ++j) cmpx(j, py[j], iy[j], st, sz);
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 4; ++j) { sp[4 * tid + j] = sp_r[j]; sidx[4 * tid + j] = id_r[j]; }
      __syncthreads();
      // torch.cumsum's order: one sequential chain of 1024 fp32 additions — kept in REGISTERS of wave 0 (lane l holds elements 16 l ..
      // 16 l + 15, the carry moves from lane to lane through an SGPR), not 1024 dependent LDS round trips of one thread
      if (tid < 64) {
        float v[16], keep[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 x = *reinterpret_cast<const f32x4*>(sp + 16 * tid + 4 * j);
          v[4 * j] = x[0]; v[4 * j + 1] = x[1]; v[4 * j + 2] = x[2]; v[4 * j + 3] = x[3];
        }
        float carry = 0.f;
        for (int l = 0; l < 64; ++l) {
          float cs = carry;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            cs += v[j];
            if (tid == l) keep[j] = (cs - v[j] > a.top_p) ? 0.f : 1.f;
          }
          carry = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cs), l));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          *reinterpret_cast<f32x4*>(skeep + 16 * tid + 4 * j) = f32x4{keep[4 * j], keep[4 * j + 1], keep[4 * j + 2], keep[4 * j + 3]};
      }
      __syncthreads();
      float ps[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) ps[j] = sp[4 * tid + j] * skeep[4 * tid + j];
      const float den2 = block_sum((ps[0] + ps[1]) + (ps[2] + ps[3]), sv);
      float bv = -1.f; int bi = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float r = (ps[j] / den2) / q[j];
        if (r > bv) { bv = r; bi = 4 * tid + j; }
      }
      float rv; int ri;
      block_argmax(bv, bi, sv, si, rv, ri);
      token = sidx[ri];
      if (tie_delta > 0.f) {   // the draw: argmax of p / q — a probability moves by a factor exp(+-delta / temp), the runner-up wins inside twice that
        float second = -1.f;   // (the nucleus cut itself is not screened: no shipped config samples with top-p)
#pragma unroll
        for (int j = 0; j < 4; ++j) if (4 * tid + j != ri) second = fmaxf(second, (ps[j] / den2) / q[j]);
        second = block_max(second, sv);
        near_tie = (rv - second) < rv * (2.f * tie_delta / a.temp);
      }
    } else {
      const float p_raw[4] = {p[0], p[1], p[2], p[3]};   // probabilities before the top-k mask (near-tie detector)
      float thr_keep = 0.f, den_keep = 1.f;
      if (a.top_k > 0) {
        // utils/utils.py:172-176 — threshold = k-th largest probability (bitwise binary search on the
        // IEEE bits: probabilities are >= 0 so integer order == float order), keep p >= threshold.
        const int kk = a.top_k < V ? a.top_k : V;
        uint32_t key[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) key[j] = __builtin_bit_cast(uint32_t, p[j]);
        // k-th largest key by radix-256 select: 4 passes of {LDS histogram of the next byte among the keys
        // that still match the chosen prefix, suffix-sum over the 256 bins, pick the byte holding rank `need`}
        uint32_t thr = 0;
        int need = kk;
#pragma unroll 1
        for (int pass = 0; pass < 4; ++pass) {
          const int shift = 24 - 8 * pass;
          hist[tid] = 0;
          __syncthreads();
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (pass == 0 || (key[j] >> (shift + 8)) == (thr >> (shift + 8))) atomicAdd(&hist[(key[j] >> shift) & 255u], 1u);
          __syncthreads();
          const int mine = (int)hist[255 - tid];       // reversed: an inclusive prefix scan gives suffix sums
          int scan = mine;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(scan, o, 64);
            if ((tid & 63) >= o) scan += up;
          }
          if ((tid & 63) == 63) si[tid >> 6] = scan;
          __syncthreads();
          for (int w2 = 0; w2 < (tid >> 6); ++w2) scan += si[w2];
          if (scan >= need && scan - mine < need) {    // exactly one bin holds the rank
            s_sel[0] = thr | ((uint32_t)(255 - tid) << shift);
            s_sel[1] = (uint32_t)(need - (scan - mine));
          }
          __syncthreads();
          thr = s_sel[0];
          need = (int)s_sel[1];
        }
        const float thrf = __builtin_bit_cast(float, thr);
        thr_keep = thrf;
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = p[j] * (p[j] >= thrf ? 1.0f : 0.0f);
        const float den2 = block_sum((p[0] + p[1]) + (p[2] + p[3]), sv);
        den_keep = den2;
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = p[j] / den2;
      }
      float bv = -1.f; int bi = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float r = p[j] / q[j];
        if (r > bv) { bv = r; bi = 4 * tid + j; }
      }
      float rv; int ri;
      block_argmax(bv, bi, sv, si, rv, ri);
      token = ri;
      if (tie_delta > 0.f) {
        // (1) the draw argmax(p / q): a probability moves by a factor exp(+-delta / temp) (the common normalisation cancels), so the
        //     runner-up wins when its ratio is within twice that of the winner's.  (2) the top-k threshold (keep p >= k-th largest):
        //     membership matters only through the draw — a candidate whose probability is within the band BELOW the threshold and whose
        //     ratio would have reached the winner's had it been kept, or a winner within the band ABOVE the threshold while such a
        //     candidate exists (it could have been the one left out).
        const float band = 2.f * tie_delta / a.temp;
        float second = -1.f, cand = -1.f;
        int nbelow = 0, wedge = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = 4 * tid + j;
          if (i != ri) second = fmaxf(second, p[j] / q[j]);
          if (thr_keep > 0.f) {
            if (p_raw[j] < thr_keep && p_raw[j] >= thr_keep * (1.f - band)) { ++nbelow; cand = fmaxf(cand, (p_raw[j] / den_keep) / q[j]); }
            if (i == ri && p_raw[j] <= thr_keep * (1.f + band)) wedge = 1;
          }
        }
        block_tie4(second, cand, nbelow, wedge, sv, si);             // one barrier pair for all four
        near_tie = (rv - second) < rv * band;
        if (thr_keep > 0.f && (cand >= rv * (1.f - band) || (nbelow > 0 && wedge > 0))) near_tie = true;
      }
    }
  }

  [[maybe_unused]] float lp = 0.f;
  if constexpr (LP) {          // (x holds x / tau here; static register indices)
    float xt = x[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) if ((token & 3) == j) xt = x[j];
    lp = lp_bad ? __builtin_nanf("") : (xt - lp_mx) - logf(lp_den);
  }
  if constexpr (REL) {
    // Mode 2, whole and apart (the instances of modes 0 and 1 see none of it): after the draw, before the fix-up below writes the slot.
    // The null row is read here whatever this clip's scale (the host guarantees rows [B, 2B)).
    const SampleRelevance r = va_first(lp_args...);
    const f32x4 un = *reinterpret_cast<const f32x4*>(a.logits + ((size_t)(a.B + b) * a.K + k) * V + 4 * tid);
    const float c[4] = {lc[0], lc[1], lc[2], lc[3]}, u[4] = {un[0], un[1], un[2], un[3]};
    bool mine = false;               // a non-finite value among this thread's eight: it poisons both sums below (no reduction of its own)
#pragma unroll
    for (int j = 0; j < 4; ++j) if (!(fabsf(c[j]) < INFINITY && fabsf(u[j]) < INFINITY)) mine = true;
    float mc = fmaxf(fmaxf(c[0], c[1]), fmaxf(c[2], c[3])), mu = fmaxf(fmaxf(u[0], u[1]), fmaxf(u[2], u[3]));
    block_max2(mc, mu, sv);
    float ec[4], eu[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { ec[j] = expf(c[j] - mc); eu[j] = expf(u[j] - mu); }
    float dc = (ec[0] + ec[1]) + (ec[2] + ec[3]), du = (eu[0] + eu[1]) + (eu[2] + eu[3]);
    if (mine) dc = du = __builtin_nanf("");
    block_sum2(dc, du, sv);
    const bool bad = lp_bad || dc != dc;      // block-uniform: the row's own status (mixed logits), or a NaN that reached the sums
    if (tid == (token >> 2)) {       // the thread that holds the token's two logits
      float ct = c[0], ut = u[0];
#pragma unroll
      for (int j = 1; j < 4; ++j) if ((token & 3) == j) { ct = c[j]; ut = u[j]; }
      const float rel_c = bad ? __builtin_nanf("") : (ct - mc) - logf(dc);
      const float rel_n = bad ? __builtin_nanf("") : (ut - mu) - logf(du);
      if (r.cond_out) r.cond_out[b * a.K + k] = rel_c;
      if (r.null_out) r.null_out[b * a.K + k] = rel_n;
      if (bad && a.state_rw) __hip_atomic_fetch_or(&a.state_rw[4], VAURA_STATUS_NONFINITE_LOGITS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a.seq && (r.cond_seq || r.null_seq)) {
        // the fix-up's own rule, evaluated by the thread that applies it next: a sampled token only (a valid slot that still holds -1)
        int dk = k;
#pragma unroll
        for (int j = 0; j < 16; ++j) if (j == k) dk = a.delays[j];
        const int offset = pos + 1, t = offset - 1 - dk;
        const size_t slot = ((size_t)b * a.K + k) * a.S + offset;
        if (offset < a.S && t >= 0 && t < a.T && a.seq[slot] == -1) {
          if (r.cond_seq) r.cond_seq[slot] = rel_c;
          if (r.null_seq) r.null_seq[slot] = rel_n;
        }
      }
    }
  }
  const int writer = LP ? (token >> 2) : 0;      // LP: the thread that holds the token's logit
  if (tid == writer) {
    if (a.tokens_out) a.tokens_out[b * a.K + k] = token;
    if constexpr (LP) if (lp_out) lp_out[b * a.K + k] = lp;
    if (a.seq) {
      // vaura_model.py:536-544 — invalid pattern slots become the special token; known tokens are kept
      int dk = k;                // this codebook's delay (static indices: k is uniform, a run-time index would go to scratch)
#pragma unroll
      for (int j = 0; j < 16; ++j) if (j == k) dk = a.delays[j];
      const int offset = pos + 1;
      const int t = offset - 1 - dk;
      const int tok = (t >= 0 && t < a.T) ? token : V;
      if (offset < a.S) {   // a step past the end of the sequence (refused by vaura_generate_loop) must not write
        int32_t* slot = a.seq + ((size_t)b * a.K + k) * a.S + offset;
        if (*slot == -1) {
          *slot = tok;
          if constexpr (LP) if (lp_seq && t >= 0 && t < a.T) lp_seq[((size_t)b * a.K + k) * a.S + offset] = lp;   // a sampled token only
          // near-tie detector: only decisions that are USED count (a valid pattern slot that was still unknown)
          if (near_tie && t >= 0 && t < a.T && a.state_rw) {
            __hip_atomic_fetch_or(&a.state_rw[4], VAURA_STATUS_NEAR_TIE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&a.state_rw[6], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int expect = 0;
            (void)__hip_atomic_compare_exchange_strong(&a.state_rw[7], &expect, (int)step + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
    }
    if (a.state_rw) {
      // No fences: nothing in THIS launch reads the token slots or the state written here; the next kernel sees them
      // because a kernel boundary publishes all stores.  The arrival counter is a device-scope atomic (coherent by
      // itself).  (An agent-scope release here costs an L2 write-back per workgroup: DESIGN.md §6.)
      const int arrived = __hip_atomic_fetch_add(&a.state_rw[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (arrived == (int)(gridDim.x * gridDim.y) - 1) {
        __hip_atomic_store(&a.state_rw[1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.state_rw[0] = pos + 1;
        a.state_rw[2] = (int)step + 1;
        a.state_rw[5] = a.state_rw[5] + 1;     // launch-epoch counter of the in-launch hand-offs (common.h va_handoff_epoch): never rewound
      }
    }
  }
}

// The read-back behind every host-side check of a per-clip array: capture query, one small copy, a wait on `s`.  While `s` is being
// captured nothing may wait: *captured is set and nothing is copied — the caller skips its check, the kernels' own clamps keep such
// a launch inside its rows.  captured = NULL does not ask: a capturing stream then answers with HIP's own error.
static int va_read_back(void* host, const void* dev, size_t bytes, hipStream_t s, bool* captured) {
  if (captured) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipError_t ce = hipStreamIsCapturing(s, &cs);
    if (ce != hipSuccess) { (void)hipGetLastError(); return (int)ce; }      // no answer: refuse, never skip silently
    *captured = cs != hipStreamCaptureStatusNone;
    if (*captured) return 0;
  }
  hipError_t e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return (int)e;
}

// Host side of the per-clip records' contract (the public entry points call it, never a captured launch): no records with probability
// rows, and no record may ask for the CFG mix unless the call carries the null-condition rows (`doubled`, and the scalar cfg_scale > 1
// that says so to the kernel).  Reads the B records back (va_read_back: skipped while `s` is being captured).
int va_check_clip_sampling(const vaura_sampling* sp, const vaura_clip_sampling* clips, int B, bool doubled, hipStream_t s) {
  if (!clips) return 0;
  if (!sp || B <= 0 || sp->input_is_probs) return VAURA_ERR_ARG;
  if (((uintptr_t)clips & 15u) != 0) return VAURA_ERR_ARG;
  std::vector<vaura_clip_sampling> host((size_t)B);
  bool captured = false;
  const int rc = va_read_back(host.data(), clips, host.size() * sizeof(vaura_clip_sampling), s, &captured);
  if (rc || captured) return rc;
  const bool rows = doubled && sp->cfg_scale > 1.0f;
  for (const vaura_clip_sampling& r : host)
    if (r.cfg_scale > 1.0f && !rows) return VAURA_ERR_ARG;
  return 0;
}

// Host side of the per-clip lengths' contract, under the rules of va_check_clip_sampling: the B values are read back and held to
// lo .. hi; skipped while `s` is being captured.
int va_check_clip_lengths(const int32_t* lengths, int B, int lo, int hi, hipStream_t s) {
  if (!lengths) return 0;
  if (B <= 0 || ((uintptr_t)lengths & 3u) != 0) return VAURA_ERR_ARG;
  std::vector<int32_t> host((size_t)B);
  bool captured = false;
  const int rc = va_read_back(host.data(), lengths, host.size() * sizeof(int32_t), s, &captured);
  if (rc || captured) return rc;
  for (const int32_t v : host)
    if (v < lo || v > hi) return VAURA_ERR_ARG;
  return 0;
}

int va_launch_sample(const VaSampleLaunch& l, hipStream_t s) {
  const vaura_sampling* sp = l.sp;
  const int B = l.B, K = l.K;
  if (!l.logits || !sp || B <= 0 || K <= 0) return VAURA_ERR_ARG;
  if (l.clips && sp->input_is_probs) return VAURA_ERR_ARG;
  const bool rel = l.cond_out || l.cond_seq || l.null_out || l.null_seq;
  const bool lp = l.lp_out || l.lp_seq || rel;
  if (lp && sp->input_is_probs) return VAURA_ERR_ARG;        // rows that already are probabilities: no log-probability to report
  // mode 2 reads rows [B, 2B) for every clip: both values or neither, and only when the call states that those rows exist
  if (rel && (!(l.cond_out || l.cond_seq) || !(l.null_out || l.null_seq) || !l.null_rows || !(sp->cfg_scale > 1.0f))) return VAURA_ERR_ARG;
  if (l.vocab != 1024) return VAURA_ERR_SHAPE;
  if (l.delays_host && K > 16) return VAURA_ERR_ARG;
  if (l.clip_T && !l.seq) return VAURA_ERR_ARG;                 // lengths decide the validity of sequence slots: nothing to decide without a sequence
  if (l.clip_n && (!l.seq || !l.state)) return VAURA_ERR_ARG;   // the counter step is position - n_b: the position lives in the state
  SampleArgs a;
  a.logits = l.logits; a.noise = l.noise; a.state = l.state; a.state_rw = l.state; a.tokens_out = l.tokens_out; a.seq = l.seq;
  a.B = B; a.K = K; a.V = l.vocab; a.T = l.T; a.S = l.S;
  for (int j = 0; j < 16; ++j) a.delays[j] = (l.delays_host && j < K) ? l.delays_host[j] : j;   // NULL: the default pattern, d_k = k
  a.use_sampling = sp->use_sampling; a.top_k = sp->top_k; a.temp = sp->temp; a.top_p = sp->top_p;
  a.cfg_scale = sp->input_is_probs ? 1.0f : sp->cfg_scale; a.seed = sp->seed; a.clip_base = sp->clip_base; a.step_host = l.step_host;
  a.probs_in = sp->input_is_probs;
  a.tie_eps = sp->tie_eps > 0.f ? sp->tie_eps : 0.f;
  const int32_t* rec = reinterpret_cast<const int32_t*>(l.clips);
  // The instance is told by the TYPES of its pack, in the fixed order [SampleLogprobs | SampleRelevance] [SampleLengths] [SampleStarts]:
  // each step below appends its member where the launch carries the array and hands the pack on; the last one derives LP from the
  // pack, picks PC by the records and launches.  3 x 2 x 2 packs x 2 values of PC: the 24 instances, each reached from one place.
  const dim3 grid(K, B), block(SMP_THREADS);
  const auto launch = [&](auto... pack) -> int {
    constexpr bool LP = ((std::is_same<decltype(pack), SampleLogprobs>::value || std::is_same<decltype(pack), SampleRelevance>::value) || ...);
    // (named outside the macro: the commas of the template arguments would split its argument list)
    const auto k_plain = sample_kernel<false, LP, decltype(pack)...>, k_pc = sample_kernel<true, LP, decltype(pack)...>;
    if (l.clips) VA_LAUNCH(k_pc, grid, block, 0, s, a.logits, a.state, a, rec, pack...);
    else VA_LAUNCH(k_plain, grid, block, 0, s, a.logits, a.state, a, rec, pack...);
    return 0;
  };
  const auto with_starts = [&](auto... pack) -> int { return l.clip_n ? launch(pack..., SampleStarts{l.clip_n}) : launch(pack...); };
  const auto with_lengths = [&](auto... pack) -> int { return l.clip_T ? with_starts(pack..., SampleLengths{l.clip_T}) : with_starts(pack...); };
  if (rel) return with_lengths(SampleRelevance{l.lp_out, l.lp_seq, l.cond_out, l.cond_seq, l.null_out, l.null_seq});
  if (lp) return with_lengths(SampleLogprobs{l.lp_out, l.lp_seq});
  return with_lengths();
}

__global__ void advance_kernel(int32_t* state, int set_to) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    state[0] = set_to >= 0 ? set_to : state[0] + 1;
    state[5] = state[5] + 1;                   // launch-epoch counter (common.h va_handoff_epoch)
  }
}
int va_launch_advance(int32_t* state, int set_to, hipStream_t s) {
  VA_LAUNCH(advance_kernel, dim3(1), dim3(64), 0, s, state, set_to);
  return 0;
}

// ------------------------------------------------------------------------------------ pattern
// delay pattern: sequence step s of codebook q holds timestep t = s - 1 - d_q; S = T + max(d) + 1 steps.  The delays travel by
// value; codebooks q >= 16 (default pattern only) keep d_q = q.
struct PatternDelays { int32_t d[16]; };

__device__ __forceinline__ int pattern_delay(const PatternDelays& pd, int q) {
  int dq = q;
#pragma unroll
  for (int j = 0; j < 16; ++j) if (j == q) dq = pd.d[j];     // static indices: a per-lane run-time index would go to scratch
  return dq;
}

// Per-clip lengths (clip_T, or NULL: every clip holds T frames): clip b holds T_b = clip_T[b] <= T frames.  build: a slot whose timestep
// is >= T_b holds the special token, as in the sequence built for T = T_b; revert (tokens or fp32 values in the layout of seq): frames
// from T_b on get `pad`.  T_b is clamped to T in build: no value can send a read out of the clip's rows.  One kernel each for every
// entry point: they run once or a handful of times per call, outside the decode loop.
__global__ void pattern_build_kernel(const int32_t* __restrict__ codes, int32_t* __restrict__ seq, int B, int K, int T, int S,
                                     int special, PatternDelays pd, const int32_t* __restrict__ clip_T) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * K * S) return;
  const int s = (int)(i % S), q = (int)((i / S) % K), b = (int)(i / ((int64_t)S * K));
  const int t = s - 1 - pattern_delay(pd, q);
  const int Tb = clip_T ? min(clip_T[b], T) : T;
  seq[i] = (t >= 0 && t < Tb) ? codes[((size_t)b * K + q) * T + t] : special;
}
template <typename E>      // tokens (int32_t) or their log-probabilities (float): the same index map
__global__ void pattern_revert_kernel(const E* __restrict__ seq, E* __restrict__ out, int B, int K, int T, int S, E fill, E pad,
                                      PatternDelays pd, const int32_t* __restrict__ clip_T) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * K * T) return;
  const int t = (int)(i % T), q = (int)((i / T) % K);
  const int64_t b = i / ((int64_t)T * K);
  const int s = t + 1 + pattern_delay(pd, q);
  out[i] = (!clip_T || t < clip_T[b]) ? ((s < S) ? seq[((size_t)b * K + q) * S + s] : fill) : pad;
}

// delays_host: K sorted, non-negative delays (K <= 16), or NULL for d_q = q.  Returns max(d) + 1 (K for NULL), or an error.
static int pattern_delays_arg(const int32_t* delays_host, int K, PatternDelays* pd) {
  for (int j = 0; j < 16; ++j) pd->d[j] = j;
  if (!delays_host) return K;
  if (K > 16) return VAURA_ERR_ARG;
  for (int q = 0; q < K; ++q) {
    if (delays_host[q] < 0 || (q > 0 && delays_host[q] < delays_host[q - 1])) return VAURA_ERR_ARG;
    pd->d[q] = delays_host[q];
  }
  return delays_host[K - 1] + 1;
}

// clip_T: the lengths (read back and held to 1 .. T) or NULL; an entry point that requires either array refuses its NULL itself
static int pattern_build(const int32_t* codes, int32_t* seq, int B, int K, int T, int S, int special, const int32_t* delays_host,
                         const int32_t* clip_T, hipStream_t s) {
  if (!codes || !seq || B <= 0 || K <= 0 || T <= 0) return VAURA_ERR_ARG;
  PatternDelays pd;
  const int span = pattern_delays_arg(delays_host, K, &pd);
  if (span < 0) return span;
  if (S != T + span) return VAURA_ERR_SHAPE;
  const int rc = va_check_clip_lengths(clip_T, B, 1, T, s);
  if (rc) return rc;
  const int64_t n = (int64_t)B * K * S;
  VA_LAUNCH(pattern_build_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, codes, seq, B, K, T, S, special, pd, clip_T);
  return 0;
}

template <typename E>
static int pattern_revert(const E* seq, E* out, int B, int K, int T, int S, E fill, E pad, const int32_t* delays_host,
                          const int32_t* clip_T, hipStream_t s) {
  if (!out || !seq || B <= 0 || K <= 0 || T <= 0 || S <= 0) return VAURA_ERR_ARG;
  PatternDelays pd;
  const int span = pattern_delays_arg(delays_host, K, &pd);
  if (span < 0) return span;
  if (delays_host && S > T + span) return VAURA_ERR_SHAPE;
  const int rc = va_check_clip_lengths(clip_T, B, 1, T, s);
  if (rc) return rc;
  const int64_t n = (int64_t)B * K * T;
  const auto kern = pattern_revert_kernel<E>;
  VA_LAUNCH(kern, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, seq, out, B, K, T, S, fill, pad, pd, clip_T);
  return 0;
}

// Sequence scores of token log-probabilities kept in the layout of seq.  One workgroup per clip, one wave per codebook (K <= 16), in a
// fixed order (the scheme of csrc/score.hip): lane l adds frames t0 + l, t0 + l + 64, .. of its codebook one after the other, the wave's
// fixed butterfly (wave_sum: neighbours at distance 1, 2, 4, .., 32) adds the lanes, the mean is sum / (T - t0); thread 0 then adds the K
// means in codebook order and divides by K.  Two runs give the same bits; a NaN anywhere in the clip reaches the clip's score through
// the sums (and every codebook's mean is then reported NaN as well: the clip's scores are not to be used).
// The means of clip b run over frames [t0_b, T_b): t0_b = clip_t0[b] (per-clip prompt lengths) or the scalar t0 where clip_t0 is NULL,
// T_b = clip_T[b] (per-clip lengths) or the scalar T where clip_T is NULL — the launch with t0 = t0_b and T = T_b.
__global__ __launch_bounds__(1024) void sequence_logprob_kernel(const float* __restrict__ lp, int B, int K, int T, int S, int t0,
                                                                PatternDelays pd, float* __restrict__ per_codebook,
                                                                float* __restrict__ per_clip, const int32_t* __restrict__ clip_t0,
                                                                const int32_t* __restrict__ clip_T) {
  __shared__ float means[16];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6, b = blockIdx.x;
  if (clip_T) T = clip_T[b];
  if (clip_t0) t0 = clip_t0[b];
  const int dq = pattern_delay(pd, q);
  const float* row = lp + ((size_t)b * K + q) * S + 1 + dq;
  float acc = 0.f;
  for (int t = t0 + lane; t < T; t += 64) acc += (t + 1 + dq < S) ? row[t] : 0.f;
  acc = wave_sum(acc);
  if (lane == 0) means[q] = acc / (float)(T - t0);
  __syncthreads();
  float tot = 0.f;
  for (int j = 0; j < K; ++j) tot += means[j];
  tot = tot / (float)K;
  if (lane == 0) per_codebook[(size_t)b * K + q] = (tot != tot) ? tot : means[q];
  if (threadIdx.x == 0) per_clip[b] = tot;
}

// The three vaura_sequence_logprob* entry points.  clip_t0 = NULL: the scalar t0, and clip_T (or NULL) is held to t0 + 1 .. T through
// va_check_clip_lengths — every clip has a frame behind the prompt; skipped while `s` is being captured.  With clip_t0 both arrays are
// read back without asking (a capturing stream gets HIP's error): 1 <= T_b <= T and 0 <= t0_b < T_b.
static int sequence_logprob(const float* logprobs, int seq_len, const int32_t* delays_host, int B, int K, int T, int t0,
                            const int32_t* clip_t0, const int32_t* clip_T, float* per_codebook, float* per_clip, hipStream_t s) {
  if (!logprobs || !per_codebook || !per_clip || B <= 0 || K <= 0 || T <= 0 || seq_len <= 0) return VAURA_ERR_ARG;
  if (!clip_t0 && (t0 < 0 || t0 >= T)) return VAURA_ERR_ARG;
  if (K > 16) return VAURA_ERR_SHAPE;
  PatternDelays pd;
  const int span = pattern_delays_arg(delays_host, K, &pd);
  if (span < 0) return span;
  if (seq_len != T + span) return VAURA_ERR_SHAPE;      // every frame of every codebook has its slot
  if (clip_t0) {
    if (((uintptr_t)clip_t0 & 3u) != 0 || ((uintptr_t)clip_T & 3u) != 0) return VAURA_ERR_ARG;
    std::vector<int32_t> h0((size_t)B), hT((size_t)B, T);
    int rc = va_read_back(h0.data(), clip_t0, h0.size() * sizeof(int32_t), s, nullptr);
    if (!rc && clip_T) rc = va_read_back(hT.data(), clip_T, hT.size() * sizeof(int32_t), s, nullptr);
    if (rc) return rc;
    for (int b = 0; b < B; ++b)
      if (hT[b] < 1 || hT[b] > T || h0[b] < 0 || h0[b] >= hT[b]) return VAURA_ERR_ARG;
  } else {
    const int rc = va_check_clip_lengths(clip_T, B, t0 + 1, T, s);
    if (rc) return rc;
  }
  VA_LAUNCH(sequence_logprob_kernel, dim3((unsigned)B), dim3(64 * K), 0, s, logprobs, B, K, T, seq_len, t0, pd, per_codebook, per_clip,
            clip_t0, clip_T);
  return 0;
}

// Best-of-N: one workgroup per clip picks the candidate with the largest score — the first index wins a tie, a NaN never beats a
// number, candidate 0 when every score is NaN — and copies its (K, T) codes.
__global__ __launch_bounds__(256) void select_candidates_kernel(const float* __restrict__ scores, const int32_t* __restrict__ codes, int N,
                                                                int KT, int32_t* __restrict__ codes_out, int32_t* __restrict__ winner) {
  const int b = blockIdx.x;
  int best = 0;
  float sb = scores[(size_t)b * N];
  for (int j = 1; j < N; ++j) {
    const float sj = scores[(size_t)b * N + j];
    if (sj > sb || (sb != sb && sj == sj)) { best = j; sb = sj; }
  }
  const int32_t* src = codes + ((size_t)b * N + best) * KT;
  int32_t* dst = codes_out + (size_t)b * KT;
  for (int i = threadIdx.x; i < KT; i += blockDim.x) dst[i] = src[i];
  if (threadIdx.x == 0) winner[b] = best;
}

// The attention map of a finished call from the weights its steps reported (vaura_decoder_ext4.attn_probs; csrc/attention.hip):
// probs (n_steps, n_rows, H, max_len) -> out (n_rows, n_steps, W), the mean over the heads — p_0 + p_1 + .. + p_{H-1} added in that
// order in fp32, times 1 / H once: nn.MultiheadAttention's averaged weights —, or with ALL out (n_rows, H, n_steps, W), a transposed
// copy.  One work item per output element; columns behind a step's position hold the zeros the caller put there.
template <bool ALL>
__global__ __launch_bounds__(256) void attention_map_kernel(const float* __restrict__ probs, float* __restrict__ out, int n_steps, int n_rows,
                                                            int H, int max_len, int W, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % W);
  long long r = i / W;
  const int step = (int)(r % n_steps);
  r /= n_steps;
  if constexpr (ALL) {
    const int h = (int)(r % H), b = (int)(r / H);
    out[i] = probs[(((size_t)step * n_rows + b) * H + h) * (size_t)max_len + j];
  } else {
    const float* src = probs + ((size_t)step * n_rows + (size_t)r) * H * (size_t)max_len + j;
    float acc = src[0];
    for (int h = 1; h < H; ++h) acc += src[(size_t)h * max_len];
    out[i] = acc * (1.0f / (float)H);
  }
}

extern "C" int vaura_attention_map(const float* probs, float* out, int n_steps, int n_rows, int n_head, int max_len, int W, int all_heads,
                                   vaura_stream_t s) {
  if (!probs || !out || n_steps < 1 || n_rows < 1 || n_head < 1 || max_len < 1 || W < 1 || W > max_len) return VAURA_ERR_ARG;
  const long long total = (long long)n_rows * (all_heads ? n_head : 1) * n_steps * W;
  if (total > 0x7fffffffLL * 256) return VAURA_ERR_SHAPE;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (all_heads) VA_LAUNCH(attention_map_kernel<true>, grid, dim3(256), 0, as_stream(s), probs, out, n_steps, n_rows, n_head, max_len, W, total);
  else VA_LAUNCH(attention_map_kernel<false>, grid, dim3(256), 0, as_stream(s), probs, out, n_steps, n_rows, n_head, max_len, W, total);
  return 0;
}

// What vaura_sample_clips / _logprobs / _relevance share: the rules of the standalone and the sequence form, the records' check, the
// launch.  Each entry point states its own required pointers first.
static int sample_step(const float* logits, int B, int K, int vocab, const vaura_sampling* sp, const vaura_clip_sampling* clips,
                       const float* noise, int64_t step, int32_t* tokens_out, int32_t* seq, int T, int S, int32_t* state,
                       float* logprobs_out, float* cond_out, float* null_out, hipStream_t s) {
  if (!logits || !sp || (!tokens_out && !seq) || B <= 0 || K <= 0) return VAURA_ERR_ARG;
  if (seq && (!state || T <= 0 || S <= 0)) return VAURA_ERR_ARG;
  const int rc = va_check_clip_sampling(sp, clips, B, sp->cfg_scale > 1.0f, s);
  if (rc) return rc;
  VaSampleLaunch a;
  a.logits = logits; a.B = B; a.K = K; a.vocab = vocab; a.sp = sp; a.clips = clips; a.noise = noise; a.step_host = step;
  a.tokens_out = tokens_out; a.seq = seq; a.T = T; a.S = S;
  a.state = seq ? state : nullptr;      // the standalone form keeps no state, like vaura_sample
  a.lp_out = logprobs_out;
  a.cond_out = cond_out; a.null_out = null_out; a.null_rows = cond_out || null_out;      // (vaura_sample_relevance has checked cfg_scale > 1)
  return va_launch_sample(a, s);
}

// vaura_sample_seq and vaura_sample_seq_starts: clip_first_steps = NULL is the former (its range check passes a NULL)
static int sample_seq(const float* logits, int B, int K, int vocab, const vaura_sampling* sp, const vaura_clip_sampling* clips,
                      const float* noise, int32_t* seq, int T, int S, int32_t* state, const int32_t* delays_host,
                      const int32_t* clip_timesteps, const int32_t* clip_first_steps, float* lp_seq, float* cond_seq, float* null_seq,
                      hipStream_t s) {
  if (!logits || !sp || !seq || !state || B <= 0 || K <= 0 || T <= 0 || S <= 0) return VAURA_ERR_ARG;
  if (sp->input_is_probs && (clips || lp_seq || cond_seq || null_seq)) return VAURA_ERR_ARG;
  if (!cond_seq != !null_seq) return VAURA_ERR_ARG;
  if (delays_host) {
    PatternDelays pd;
    const int span = pattern_delays_arg(delays_host, K, &pd);
    if (span < 0) return span;
  }
  int rc = va_check_clip_sampling(sp, clips, B, sp->cfg_scale > 1.0f, s);
  if (!rc) rc = va_check_clip_lengths(clip_timesteps, B, 1, T, s);
  if (!rc) rc = va_check_clip_lengths(clip_first_steps, B, 0, S - 1, s);
  if (rc) return rc;
  VaSampleLaunch a;
  a.logits = logits; a.B = B; a.K = K; a.vocab = vocab; a.sp = sp; a.clips = clips; a.noise = noise;
  a.seq = seq; a.T = T; a.S = S; a.state = state; a.delays_host = delays_host; a.clip_T = clip_timesteps; a.clip_n = clip_first_steps;
  a.lp_seq = lp_seq; a.cond_seq = cond_seq; a.null_seq = null_seq; a.null_rows = sp->cfg_scale > 1.0f;
  return va_launch_sample(a, s);
}

extern "C" {

int vaura_pattern_build(const int32_t* codes, int32_t* seq, int B, int K, int T, int special, vaura_stream_t s) {
  return pattern_build(codes, seq, B, K, T, T + K, special, nullptr, nullptr, as_stream(s));
}

int vaura_pattern_revert(const int32_t* seq, int32_t* codes, int B, int K, int T, int S, int fill, vaura_stream_t s) {
  return pattern_revert<int32_t>(seq, codes, B, K, T, S, fill, 0, nullptr, nullptr, as_stream(s));
}

int vaura_pattern_build_delays(const int32_t* codes, int32_t* seq, int B, int K, int T, int S, int special,
                               const int32_t* delays_host, vaura_stream_t s) {
  if (!delays_host) return VAURA_ERR_ARG;
  return pattern_build(codes, seq, B, K, T, S, special, delays_host, nullptr, as_stream(s));
}

int vaura_pattern_revert_delays(const int32_t* seq, int32_t* codes, int B, int K, int T, int S, int fill,
                                const int32_t* delays_host, vaura_stream_t s) {
  if (!delays_host) return VAURA_ERR_ARG;
  return pattern_revert<int32_t>(seq, codes, B, K, T, S, fill, 0, delays_host, nullptr, as_stream(s));
}

int vaura_pattern_revert_delays_f32(const float* seq, float* out, int B, int K, int T, int S, float fill, const int32_t* delays_host,
                                    vaura_stream_t s) {
  return pattern_revert<float>(seq, out, B, K, T, S, fill, 0.f, delays_host, nullptr, as_stream(s));
}

int vaura_pattern_build_clips(const int32_t* codes, int32_t* seq, int B, int K, int T, int S, int special, const int32_t* delays_host,
                              const int32_t* clip_timesteps, vaura_stream_t s) {
  if (!clip_timesteps) return VAURA_ERR_ARG;
  return pattern_build(codes, seq, B, K, T, S, special, delays_host, clip_timesteps, as_stream(s));
}

int vaura_pattern_revert_clips(const int32_t* seq, int32_t* codes, int B, int K, int T, int S, int fill, int pad,
                               const int32_t* delays_host, const int32_t* clip_timesteps, vaura_stream_t s) {
  if (!clip_timesteps) return VAURA_ERR_ARG;
  return pattern_revert<int32_t>(seq, codes, B, K, T, S, fill, pad, delays_host, clip_timesteps, as_stream(s));
}

int vaura_pattern_revert_clips_f32(const float* seq, float* out, int B, int K, int T, int S, float fill, float pad,
                                   const int32_t* delays_host, const int32_t* clip_timesteps, vaura_stream_t s) {
  if (!clip_timesteps) return VAURA_ERR_ARG;
  return pattern_revert<float>(seq, out, B, K, T, S, fill, pad, delays_host, clip_timesteps, as_stream(s));
}

int vaura_sample(const float* logits, int B, int K, int vocab, const vaura_sampling* sp, const float* noise,
                 int64_t step, int32_t* tokens_out, vaura_stream_t s) {
  if (!tokens_out) return VAURA_ERR_ARG;
  VaSampleLaunch a;      // no state: the step comes from the host
  a.logits = logits; a.B = B; a.K = K; a.vocab = vocab; a.sp = sp; a.noise = noise; a.step_host = step; a.tokens_out = tokens_out;
  return va_launch_sample(a, as_stream(s));
}

int vaura_sample_clips(const float* logits, int B, int K, int vocab, const vaura_sampling* sp, const vaura_clip_sampling* clips,
                       const float* noise, int64_t step, int32_t* tokens_out, int32_t* seq, int T, int S, int32_t* state,
                       vaura_stream_t s) {
  if (!clips) return VAURA_ERR_ARG;
  return sample_step(logits, B, K, vocab, sp, clips, noise, step, tokens_out, seq, T, S, state, nullptr, nullptr, nullptr, as_stream(s));
}

int vaura_sample_logprobs(const float* logits, int B, int K, int vocab, const vaura_sampling* sp, const vaura_clip_sampling* clips,
                          const float* noise, int64_t step, int32_t* tokens_out, int32_t* seq, int T, int S, int32_t* state,
                          float* logprobs_out, vaura_stream_t s) {
  if (!sp || !logprobs_out || sp->input_is_probs) return VAURA_ERR_ARG;
  return sample_step(logits, B, K, vocab, sp, clips, noise, step, tokens_out, seq, T, S, state, logprobs_out, nullptr, nullptr,
                     as_stream(s));
}

int vaura_sample_relevance(const float* logits, int B, int K, int vocab, const vaura_sampling* sp, const vaura_clip_sampling* clips,
                           const float* noise, int64_t step, int32_t* tokens_out, int32_t* seq, int T, int S, int32_t* state,
                           float* logprobs_out, float* cond_out, float* null_out, vaura_stream_t s) {
  if (!sp || !cond_out || !null_out || sp->input_is_probs) return VAURA_ERR_ARG;
  if (!(sp->cfg_scale > 1.0f)) return VAURA_ERR_ARG;      // no null-condition rows: nothing to compare the conditional row with
  // logprobs_out is optional here: NULL = lc and lu only
  return sample_step(logits, B, K, vocab, sp, clips, noise, step, tokens_out, seq, T, S, state, logprobs_out, cond_out, null_out,
                     as_stream(s));
}

int vaura_sample_seq(const float* logits, int B, int K, int vocab, const vaura_sampling* sp, const vaura_clip_sampling* clips,
                     const float* noise, int32_t* seq, int T, int S, int32_t* state, const int32_t* delays_host,
                     const int32_t* clip_timesteps, float* lp_seq, float* cond_seq, float* null_seq, vaura_stream_t s) {
  return sample_seq(logits, B, K, vocab, sp, clips, noise, seq, T, S, state, delays_host, clip_timesteps, nullptr, lp_seq, cond_seq,
                    null_seq, as_stream(s));
}

int vaura_sample_seq_starts(const float* logits, int B, int K, int vocab, const vaura_sampling* sp, const vaura_clip_sampling* clips,
                            const float* noise, int32_t* seq, int T, int S, int32_t* state, const int32_t* delays_host,
                            const int32_t* clip_timesteps, const int32_t* clip_first_steps, float* lp_seq, float* cond_seq,
                            float* null_seq, vaura_stream_t s) {
  if (!clip_first_steps) return VAURA_ERR_ARG;
  return sample_seq(logits, B, K, vocab, sp, clips, noise, seq, T, S, state, delays_host, clip_timesteps, clip_first_steps, lp_seq,
                    cond_seq, null_seq, as_stream(s));
}

int vaura_sequence_logprob(const float* logprobs, int seq_len, const int32_t* delays_host, int B, int K, int T, int t0,
                           float* per_codebook, float* per_clip, vaura_stream_t s) {
  return sequence_logprob(logprobs, seq_len, delays_host, B, K, T, t0, nullptr, nullptr, per_codebook, per_clip, as_stream(s));
}

int vaura_sequence_logprob_clips(const float* logprobs, int seq_len, const int32_t* delays_host, int B, int K, int T, int t0,
                                 const int32_t* clip_timesteps, float* per_codebook, float* per_clip, vaura_stream_t s) {
  if (!clip_timesteps) return VAURA_ERR_ARG;
  return sequence_logprob(logprobs, seq_len, delays_host, B, K, T, t0, nullptr, clip_timesteps, per_codebook, per_clip, as_stream(s));
}

int vaura_sequence_logprob_starts(const float* logprobs, int seq_len, const int32_t* delays_host, int B, int K, int T,
                                  const int32_t* clip_t0, const int32_t* clip_timesteps, float* per_codebook, float* per_clip,
                                  vaura_stream_t s) {
  if (!clip_t0) return VAURA_ERR_ARG;
  return sequence_logprob(logprobs, seq_len, delays_host, B, K, T, 0, clip_t0, clip_timesteps, per_codebook, per_clip, as_stream(s));
}

int vaura_select_candidates(const float* scores, const int32_t* codes, int B, int N, int K, int T, int32_t* codes_out, int32_t* winner,
                            vaura_stream_t s) {
  if (!scores || !codes || !codes_out || !winner || B <= 0 || N <= 0 || K <= 0 || T <= 0) return VAURA_ERR_ARG;
  if ((int64_t)K * T > 0x7fffffff) return VAURA_ERR_SHAPE;
  VA_LAUNCH(select_candidates_kernel, dim3((unsigned)B), dim3(256), 0, as_stream(s), scores, codes, N, K * T, codes_out, winner);
  return 0;
}

}  // extern "C"
