// Audio output: the codec's mono fp32 rows (44.1 kHz) -> PCM at the consumer's rate, format and channel layout, in one launch; the
// mirror image of audio_pre.hip.  One output sample, all fp32:
//   resample  m = q n + p:  acc = 0; acc = fmaf(k[p][j], x[q o + first[p] - w + j], acc) for j = 0 .. T - 1, in tap order (the table
//             of vaura_amd/audio_preprocess.py: resample_table(44100, rate), tap-major).  Explicit fmaf: every instance rounds alike.
//   gain      y = acc * gain[b]
//   format    S16 rint(y 32768) / S32 rint(y 2^31), half to even, saturated, NaN -> 0; F32 y itself.  clipped[b] counts the samples whose
//             y * scale lay outside the format's range ([-1, 1] for F32) or was NaN.
//   layout    the value goes to every one of C channels: planar (B, C, out_stride) or interleaved (B, out_stride, C).
// Stream position.  x[s] is indexed ABSOLUTELY: clip b's record says which samples this launch holds — the block [r0, r0 + L) and,
// in front of it, the carry row [r0 - H, r0) — and which outputs [m0, m0 + count) it forms, written to the row from its start.  x is
// 0 below 0 and, for a clip whose total length N is known (its last block), at and beyond N.  An output's value therefore depends
// on its absolute index and the samples around it, never on where a tile or a block starts: the blocks of a stream, concatenated, are
// the one-pass call (r0 = m0 = 0, no carry, every clip final) bit for bit.
//
//   grid  (tiles + (carry_out ? 1 : 0), B), tiles = ceil(out_stride / TILE): one workgroup per (tile of TILE output samples, clip); the
//         extra workgroup of a clip writes the NEXT carry row — the last H samples of carry ++ block — into the other buffer of the
//         caller's ping-pong pair, so no workgroup of the launch reads what another writes.
//   stage the tile's input span goes to LDS (from the carry below r0, from the block above, zeros outside the clip)
//   form  every thread takes TILE / 256 outputs as independent fmaf chains; plain vector stores; the clipped count is reduced per wave,
//         then per workgroup through LDS, and leaves as one atomic add per workgroup that counted any.
// o == n (44.1 kHz out) is the identity: no table, no staging.
#include "common.h"

#define AUDIO_OUT_TILE VAURA_AUDIO_OUT_TILE
#define AUDIO_OUT_THREADS 256
#define AUDIO_OUT_MAX_TAPS VAURA_AUDIO_PRE_MAX_TAPS
#define AUDIO_OUT_MAX_TABLE (1 << 20)
#define AUDIO_OUT_MAX_CHANNELS 8
#define AUDIO_OUT_LDS_LIMIT (64 * 1024)
#define AUDIO_OUT_RED_WORDS 4                 // one partial count per wave, in front of the staged span (16 bytes: the span stays aligned)

struct AudioOutArgs {
  const float* x;             // (B, in_stride): clip b's block
  const float* carry_in;      // (B, H): samples [r0 - H, r0) of clip b, or NULL with H == 0
  float* carry_out;           // (B, H) or NULL
  const long long* rec;       // (B, VAURA_AUDIO_OUT_RECORD): r0, L, m0, count, N (< 0: not the clip's last block)
  const int32_t* first;       // (n)
  const float* taps;          // (T, n)
  const float* gain;          // (B)
  void* out;
  int32_t* clipped;           // (B), added to
  long long in_stride, out_stride;
  int C, o, n, w, T, span, H, tiles;
};

struct AudioOutClip {
  const float *x, *carry;
  long long r0, L, N;
  int H;
  // x[s] of the stream: 0 outside the clip, the carry below r0, the block above; nothing is read behind r0 + L or outside the carry row
  __device__ __forceinline__ float sample(long long s) const {
    if (s < 0 || (N >= 0 && s >= N)) return 0.f;
    if (s < r0) return s >= r0 - H ? carry[s - (r0 - H)] : 0.f;
    return s - r0 < L ? x[s - r0] : 0.f;
  }
};

static size_t audio_out_span(int o, int n, int w, int T) {
  // as audio_pre_span: a tile's outputs advance TILE o / n samples, a run starts inside (-w, +w) of its centre and holds T taps
  return (size_t)(((long long)AUDIO_OUT_TILE * o + n - 1) / n) + 2 * (size_t)w + (size_t)T + 2;
}

template <typename T> struct AudioOutFormat;
template <> struct AudioOutFormat<int16_t> {
  static __device__ __forceinline__ int16_t quantise(float y, int& clip) {
    const float v = y * 32768.0f;
    clip += !(v >= -32768.0f && v <= 32767.0f);
    if (v != v) return 0;
    return (int16_t)(int)fminf(fmaxf(rintf(v), -32768.0f), 32767.0f);
  }
};
template <> struct AudioOutFormat<int32_t> {
  static __device__ __forceinline__ int32_t quantise(float y, int& clip) {
    const float v = y * 2147483648.0f;
    clip += !(v >= -2147483648.0f && v < 2147483648.0f);      // the fp32 values above 2^31 - 1 start at 2^31
    if (v != v) return 0;
    if (v >= 2147483648.0f) return INT32_MAX;
    if (v <= -2147483648.0f) return INT32_MIN;
    return (int32_t)rintf(v);                                  // |v| < 2^31: rint(v) is an integer an int32 holds
  }
};
template <> struct AudioOutFormat<float> {
  static __device__ __forceinline__ float quantise(float y, int& clip) {
    clip += !(y >= -1.0f && y <= 1.0f);
    return y;
  }
};

template <typename T>
struct alignas(2 * sizeof(T)) PcmOutPair { T a, b; };

// output i of the row, value v, to all C channels
template <typename T, bool INTERLEAVED>
__device__ __forceinline__ void put_frame(T* row, long long i, T v, int C, long long out_stride, bool pair_ok) {
  if (INTERLEAVED) {
    T* f = row + i * C;
    if (C == 2 && pair_ok) {
      PcmOutPair<T> pr;
      pr.a = v; pr.b = v;
      *reinterpret_cast<PcmOutPair<T>*>(f) = pr;               // one store per stereo frame
      return;
    }
    for (int c = 0; c < C; ++c) f[c] = v;
    return;
  }
  for (int c = 0; c < C; ++c) row[(long long)c * out_stride + i] = v;
}

template <typename T, bool INTERLEAVED>
__global__ __launch_bounds__(AUDIO_OUT_THREADS) void audio_output_kernel(const AudioOutArgs a) {
  extern __shared__ float lds[];
  int* red = reinterpret_cast<int*>(lds);                              // AUDIO_OUT_RED_WORDS partial counts
  float* xs = lds + AUDIO_OUT_RED_WORDS;                               // span samples
  const int tid = threadIdx.x, b = blockIdx.y;
  const long long* rec = a.rec + (long long)b * VAURA_AUDIO_OUT_RECORD;
  AudioOutClip clip;
  clip.H = a.H;
  clip.r0 = rec[0];
  clip.L = min(max(rec[1], 0ll), a.in_stride);                         // clamped: no record can make an index leave the clip's rows
  clip.N = rec[4];
  clip.x = a.x + (long long)b * a.in_stride;
  clip.carry = a.carry_in + (long long)b * a.H;
  if ((int)blockIdx.x >= a.tiles) {                                    // the next carry: the last H samples of carry ++ block
    float* next = a.carry_out + (long long)b * a.H;
    for (int i = tid; i < a.H; i += AUDIO_OUT_THREADS) {
      const long long j = clip.L - a.H + i;                            // relative to r0
      next[i] = j >= 0 ? clip.x[j] : clip.carry[a.H + j];
    }
    return;
  }
  const long long M0 = max(rec[2], 0ll);                               // a phase index is never negative
  const long long count = min(max(rec[3], 0ll), a.out_stride);
  const long long i0 = (long long)blockIdx.x * AUDIO_OUT_TILE;         // first output of the tile, relative to the row
  const long long iend = min(i0 + AUDIO_OUT_TILE, a.out_stride);
  T* row = reinterpret_cast<T*>(a.out) + (long long)b * a.C * a.out_stride;
  const bool pair_ok = (reinterpret_cast<uintptr_t>(a.out) & (2 * sizeof(T) - 1)) == 0;
  if (i0 >= count) {                                                   // behind the clip's outputs: zeros only
    for (long long i = i0 + tid; i < iend; i += AUDIO_OUT_THREADS) put_frame<T, INTERLEAVED>(row, i, (T)0, a.C, a.out_stride, pair_ok);
    return;
  }
  const float g = a.gain[b];
  constexpr int PER = AUDIO_OUT_TILE / AUDIO_OUT_THREADS;
  int clip_count = 0;
  if (a.T == 0) {                                                      // the codec's own rate
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const long long i = i0 + tid + e * AUDIO_OUT_THREADS;
      if (i < count) put_frame<T, INTERLEAVED>(row, i, AudioOutFormat<T>::quantise(clip.sample(M0 + i) * g, clip_count), a.C, a.out_stride, pair_ok);
      else if (i < iend) put_frame<T, INTERLEAVED>(row, i, (T)0, a.C, a.out_stride, pair_ok);
    }
  } else {
    const long long mt = M0 + i0;                                      // absolute index of the tile's first output
    const long long lo = (mt * a.o) / a.n - a.w;
    for (int i = tid; i < a.span; i += AUDIO_OUT_THREADS) xs[i] = clip.sample(lo + i);
    __syncthreads();
    float acc[PER];
    const float* xr[PER];
    const float* k[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const long long i = i0 + tid + e * AUDIO_OUT_THREADS;
      const long long m = i < count ? M0 + i : mt;                     // an output behind the clip computes the tile's first one and drops it
      const long long q = m / a.n;
      const int p = (int)(m - q * a.n);
      // first tap of this output in the staged span; clamped, so that no table content can index outside it
      xr[e] = xs + (int)min(max(q * a.o + a.first[p] - a.w - lo, 0ll), (long long)(a.span - a.T));
      k[e] = a.taps + p;
      acc[e] = 0.f;
    }
    for (int j = 0; j < a.T; ++j) {
#pragma unroll
      for (int e = 0; e < PER; ++e) acc[e] = fmaf(k[e][(size_t)j * a.n], xr[e][j], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const long long i = i0 + tid + e * AUDIO_OUT_THREADS;
      if (i < count) put_frame<T, INTERLEAVED>(row, i, AudioOutFormat<T>::quantise(acc[e] * g, clip_count), a.C, a.out_stride, pair_ok);
      else if (i < iend) put_frame<T, INTERLEAVED>(row, i, (T)0, a.C, a.out_stride, pair_ok);
    }
  }
  // the count: lanes -> wave (shuffles), waves -> workgroup (LDS), one atomic add per workgroup.  Integers: the order does not matter
  for (int d = 32; d > 0; d >>= 1) clip_count += __shfl_down(clip_count, d, 64);
  if ((tid & 63) == 0) red[tid >> 6] = clip_count;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int v = 0; v < AUDIO_OUT_THREADS / 64; ++v) total += red[v];
    if (total) atomicAdd(a.clipped + b, total);
  }
}

template <typename T>
static int audio_out_launch(const AudioOutArgs& a, int interleaved, dim3 grid, size_t lds, hipStream_t st) {
  if (interleaved) VA_LAUNCH((audio_output_kernel<T, true>), grid, dim3(AUDIO_OUT_THREADS), lds, st, a);
  else VA_LAUNCH((audio_output_kernel<T, false>), grid, dim3(AUDIO_OUT_THREADS), lds, st, a);
  return 0;
}

extern "C" {

int vaura_audio_output(const float* x, int B, int64_t in_stride, const int64_t* records, const float* carry_in, float* carry_out,
                       int history, int o, int n, int w, const int32_t* first, const float* taps, int phases, int taps_per_phase,
                       const float* gain, int format, int interleaved, int C_out, void* out, int64_t out_stride, int32_t* clipped,
                       vaura_stream_t s) {
  if (!x || !records || !gain || !clipped) return VAURA_ERR_ARG;
  if (in_stride < 0 || out_stride < 0 || history < 0) return VAURA_ERR_ARG;                   // negative lengths
  if (B <= 0 || in_stride == 0 || o <= 0 || n <= 0 || w < 0) return VAURA_ERR_ARG;
  if (out_stride > 0 && !out) return VAURA_ERR_ARG;
  if (history > 0 && !carry_in) return VAURA_ERR_ARG;
  if (carry_out && history == 0) return VAURA_ERR_ARG;
  if (carry_out && B <= 65535) {                                       // the ping-pong pair: the two (B, history) spans must not overlap
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(carry_in), out0 = reinterpret_cast<uintptr_t>(carry_out);
    const uintptr_t bytes = (uintptr_t)B * (uintptr_t)history * 4;
    if (in0 < out0 + bytes && out0 < in0 + bytes) return VAURA_ERR_ARG;
  }
  if (C_out < 1 || C_out > AUDIO_OUT_MAX_CHANNELS) return VAURA_ERR_SHAPE;
  if (format != VAURA_PCM_S16 && format != VAURA_PCM_S32 && format != VAURA_PCM_F32) return VAURA_ERR_DTYPE;
  if (in_stride > INT32_MAX || out_stride > INT32_MAX || history > INT32_MAX / 2) return VAURA_ERR_SHAPE;
  if (B > 65535) return VAURA_ERR_SHAPE;                               // gridDim.y
  const bool identity = o == n;
  if (!identity) {
    if (!first || !taps) return VAURA_ERR_ARG;
    if (phases != n || taps_per_phase <= 0) return VAURA_ERR_ARG;
    if (taps_per_phase > AUDIO_OUT_MAX_TAPS) return VAURA_ERR_SHAPE;
    if ((int64_t)phases * taps_per_phase > AUDIO_OUT_MAX_TABLE) return VAURA_ERR_SHAPE;
  }
  const size_t esize = format == VAURA_PCM_S16 ? 2 : 4;
  if ((reinterpret_cast<uintptr_t>(out) & (esize - 1)) || (reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(records) & 7) ||
      (reinterpret_cast<uintptr_t>(carry_in) & 3) || (reinterpret_cast<uintptr_t>(carry_out) & 3) || (reinterpret_cast<uintptr_t>(gain) & 3) ||
      (reinterpret_cast<uintptr_t>(clipped) & 3) || (reinterpret_cast<uintptr_t>(first) & 3) || (reinterpret_cast<uintptr_t>(taps) & 3))
    return VAURA_ERR_ARG;
  AudioOutArgs a;
  a.x = x; a.carry_in = carry_in; a.carry_out = carry_out; a.rec = reinterpret_cast<const long long*>(records); a.first = first; a.taps = taps;
  a.gain = gain; a.out = out; a.clipped = clipped; a.in_stride = in_stride; a.out_stride = out_stride;
  a.C = C_out; a.o = o; a.n = n; a.w = w; a.H = history;
  a.T = identity ? 0 : taps_per_phase;
  size_t lds = 4 * AUDIO_OUT_RED_WORDS;
  a.span = 0;
  if (!identity) {
    const size_t span = audio_out_span(o, n, w, taps_per_phase);
    lds += 4 * span;
    if (lds > AUDIO_OUT_LDS_LIMIT) return VAURA_ERR_SHAPE;
    a.span = (int)span;
  }
  a.tiles = (int)((out_stride + AUDIO_OUT_TILE - 1) / AUDIO_OUT_TILE);
  const unsigned gx = (unsigned)a.tiles + (carry_out ? 1u : 0u);
  if (gx == 0) return 0;                                               // no output and no carry to write
  const dim3 grid(gx, (unsigned)B);
  hipStream_t st = as_stream(s);
  switch (format) {
    case VAURA_PCM_S16: return audio_out_launch<int16_t>(a, interleaved, grid, lds, st);
    case VAURA_PCM_S32: return audio_out_launch<int32_t>(a, interleaved, grid, lds, st);
    default: return audio_out_launch<float>(a, interleaved, grid, lds, st);
  }
}

size_t vaura_audio_output_lds_bytes(int o, int n, int w, int taps_per_phase) {
  if (o <= 0 || n <= 0 || w < 0 || taps_per_phase <= 0) return 0;
  return 4 * (AUDIO_OUT_RED_WORDS + audio_out_span(o, n, w, taps_per_phase));
}

int vaura_audio_output_tile(void) { return AUDIO_OUT_TILE; }

}  // extern "C"
