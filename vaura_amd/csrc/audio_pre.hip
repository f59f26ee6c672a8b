// Audio preprocessing: decoded PCM -> the codec's padded mono input, in one launch.
//   AudioStereoToMono -> AudioResample(44100) -> AudioTrim        models/data/transforms/audio_transforms.py:162-192
//                                                               configs/generate_vas.yaml:43-54, data/demo/dataloader_config.yaml:13-20
// AudioResample is torchaudio.transforms.Resample at its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99): with
// o = orig / gcd, n = new / gcd, w = ceil(6 o / (0.99 min(o, n))), output sample m = q n + p is sum_j k[p][j] x[q o + j - w] over the
// 2 w + o taps of phase p, x = 0 outside the clip.  The window is zero outside |t| < 6, so only one run of taps per phase is non-zero
// in fp32; the host (vaura_amd/audio_preprocess.py: resample_table) hands over first[p] and that run, T taps per phase, stored tap-major
// (taps[j * n + p]: the lanes of a wave hold consecutive phases, so a tap load is one contiguous read).  The kernel does no filter
// geometry.
//
//   grid  (ceil(out_stride / TILE), B): one workgroup per (tile of TILE output samples, clip)
//   stage the tile's input span [lo, lo + len), lo = floor(m0 o / n) - w, goes to LDS as mono fp32: every thread loads the C channels
//         of its samples (planar: C reads of consecutive elements per wave; interleaved: the C elements of a frame, as one 4- or
//         8-byte word per lane for two channels), converts, adds them in channel order and divides by C.  Samples outside [0, n_b)
//         are written as 0 and never read from memory.
//   form  every thread takes TILE / 256 outputs (m = m0 + tid + 256 i): acc = sum over the T taps, in tap order, of tap * LDS sample;
//         one 4-byte store per output, 0 from the clip's output length to the row's end.
// o == n (after the gcd: the source is at the target rate) is the identity: the mono sample itself, no table, no LDS.
#include "common.h"

#define AUDIO_PRE_TILE VAURA_AUDIO_PRE_TILE
#define AUDIO_PRE_THREADS 256
#define AUDIO_PRE_MAX_TAPS VAURA_AUDIO_PRE_MAX_TAPS
#define AUDIO_PRE_MAX_TABLE (1 << 20)
#define AUDIO_PRE_MAX_CHANNELS 8
#define AUDIO_PRE_LDS_LIMIT (64 * 1024)

struct AudioPreArgs {
  const void* pcm;
  const int32_t* n_in;    // (B) real samples of clip b
  const int32_t* first;   // (n) first tap of phase p, as an index into the 2 w + o taps of the full form
  const float* taps;      // (T, n)
  const int32_t* n_out;   // (B) output samples of clip b
  float* out;             // (B, out_stride)
  long long in_stride, out_stride;
  int C, o, n, w, T, span;
};

__device__ __forceinline__ float pcm_to_float(int16_t v) { return (float)v * (1.0f / 32768.0f); }
__device__ __forceinline__ float pcm_to_float(int32_t v) { return (float)v * (1.0f / 2147483648.0f); }   // (float)v rounds; the scale is exact
__device__ __forceinline__ float pcm_to_float(float v) { return v; }

template <typename T>
struct alignas(2 * sizeof(T)) PcmPair { T a, b; };

// mono fp32 of sample i (0 <= i < n_b) of one clip: channels added in channel order, then divided by C
template <typename T, bool INTERLEAVED>
__device__ __forceinline__ float mono_sample(const T* clip, long long i, int C, long long in_stride, bool pair_ok) {
  if (INTERLEAVED) {
    const T* f = clip + i * C;
    if (C == 2 && pair_ok) {
      const PcmPair<T> v = *reinterpret_cast<const PcmPair<T>*>(f);
      return (pcm_to_float(v.a) + pcm_to_float(v.b)) / 2.0f;
    }
    float s = pcm_to_float(f[0]);
    for (int c = 1; c < C; ++c) s += pcm_to_float(f[c]);
    return s / (float)C;
  }
  float s = pcm_to_float(clip[i]);
  for (int c = 1; c < C; ++c) s += pcm_to_float(clip[(long long)c * in_stride + i]);
  return s / (float)C;
}

static size_t audio_pre_span(int o, int n, int w, int T) {
  // input samples one tile can touch: its outputs advance TILE o / n samples, a phase's run starts inside (-w, +w) of its centre and
  // holds T taps; + 2 for the two roundings of the ends
  return (size_t)(((long long)AUDIO_PRE_TILE * o + n - 1) / n) + 2 * (size_t)w + (size_t)T + 2;
}

template <typename T, bool INTERLEAVED>
__global__ __launch_bounds__(AUDIO_PRE_THREADS) void audio_preprocess_kernel(const AudioPreArgs a) {
  extern __shared__ float xs[];                                        // span mono samples
  const int tid = threadIdx.x, b = blockIdx.y;
  const long long m0 = (long long)blockIdx.x * AUDIO_PRE_TILE;
  // clamped: no length can make an index leave the clip's rows
  const long long nb = min(max((long long)a.n_in[b], 0ll), a.in_stride);
  const long long nout = min(max((long long)a.n_out[b], 0ll), a.out_stride);
  float* orow = a.out + (long long)b * a.out_stride;
  const long long mend = min(m0 + AUDIO_PRE_TILE, a.out_stride);
  if (m0 >= nout) {                                                    // behind the clip: zeros only
    for (long long m = m0 + tid; m < mend; m += AUDIO_PRE_THREADS) orow[m] = 0.f;
    return;
  }
  const T* clip = reinterpret_cast<const T*>(a.pcm) + (long long)b * a.C * a.in_stride;
  const bool pair_ok = (reinterpret_cast<uintptr_t>(a.pcm) & (2 * sizeof(T) - 1)) == 0;
  if (a.T == 0) {                                                      // source at the target rate
    for (long long m = m0 + tid; m < mend; m += AUDIO_PRE_THREADS)
      orow[m] = m < nout && m < nb ? mono_sample<T, INTERLEAVED>(clip, m, a.C, a.in_stride, pair_ok) : 0.f;
    return;
  }
  const long long lo = (m0 * a.o) / a.n - a.w;
  for (int i = tid; i < a.span; i += AUDIO_PRE_THREADS) {
    const long long s = lo + i;
    xs[i] = s >= 0 && s < nb ? mono_sample<T, INTERLEAVED>(clip, s, a.C, a.in_stride, pair_ok) : 0.f;
  }
  __syncthreads();
  // the thread's outputs side by side: PER independent chains of tap load, LDS read, multiply, add per tap
  constexpr int PER = AUDIO_PRE_TILE / AUDIO_PRE_THREADS;
  float acc[PER];
  const float* xr[PER];
  const float* k[PER];
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const long long m = m0 + tid + e * AUDIO_PRE_THREADS;
    const long long mm = m < nout ? m : m0;                            // an output behind the clip computes the tile's first one and drops it
    const long long q = mm / a.n;
    const int p = (int)(mm - q * a.n);
    // first tap of this output in the staged span; clamped, so that no table content can index outside it
    xr[e] = xs + (int)min(max(q * a.o + a.first[p] - a.w - lo, 0ll), (long long)(a.span - a.T));
    k[e] = a.taps + p;
    acc[e] = 0.f;
  }
  for (int j = 0; j < a.T; ++j) {
#pragma unroll
    for (int e = 0; e < PER; ++e) acc[e] += k[e][(size_t)j * a.n] * xr[e][j];
  }
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const long long m = m0 + tid + e * AUDIO_PRE_THREADS;
    if (m < mend) orow[m] = m < nout ? acc[e] : 0.f;
  }
}

template <typename T>
static int audio_pre_launch(const AudioPreArgs& a, int interleaved, dim3 grid, size_t lds, hipStream_t st) {
  if (interleaved) VA_LAUNCH((audio_preprocess_kernel<T, true>), grid, dim3(AUDIO_PRE_THREADS), lds, st, a);
  else VA_LAUNCH((audio_preprocess_kernel<T, false>), grid, dim3(AUDIO_PRE_THREADS), lds, st, a);
  return 0;
}

extern "C" {

int vaura_audio_preprocess(const void* pcm, int format, int interleaved, int B, int C, int64_t in_stride, const int32_t* n_in, int o, int n,
                           int w, const int32_t* first, const float* taps, int phases, int taps_per_phase, float* out, int64_t out_stride,
                           const int32_t* n_out, vaura_stream_t s) {
  if (!pcm || !n_in || !out || !n_out) return VAURA_ERR_ARG;
  if (B <= 0 || C <= 0 || in_stride <= 0 || out_stride <= 0 || o <= 0 || n <= 0 || w < 0) return VAURA_ERR_ARG;
  if (C > AUDIO_PRE_MAX_CHANNELS) return VAURA_ERR_SHAPE;
  if (format != VAURA_PCM_S16 && format != VAURA_PCM_S32 && format != VAURA_PCM_F32) return VAURA_ERR_DTYPE;
  if (in_stride > INT32_MAX || out_stride > INT32_MAX) return VAURA_ERR_SHAPE;
  if (B > 65535) return VAURA_ERR_SHAPE;                               // gridDim.y
  const bool identity = o == n;
  if (!identity) {
    if (!first || !taps) return VAURA_ERR_ARG;
    if (phases != n || taps_per_phase <= 0) return VAURA_ERR_ARG;
    if (taps_per_phase > AUDIO_PRE_MAX_TAPS) return VAURA_ERR_SHAPE;
    if ((int64_t)phases * taps_per_phase > AUDIO_PRE_MAX_TABLE) return VAURA_ERR_SHAPE;
  }
  const size_t esize = format == VAURA_PCM_S16 ? 2 : 4;
  if ((reinterpret_cast<uintptr_t>(pcm) & (esize - 1)) || (reinterpret_cast<uintptr_t>(out) & 3) || (reinterpret_cast<uintptr_t>(n_in) & 3) ||
      (reinterpret_cast<uintptr_t>(n_out) & 3) || (reinterpret_cast<uintptr_t>(first) & 3) || (reinterpret_cast<uintptr_t>(taps) & 3))
    return VAURA_ERR_ARG;
  AudioPreArgs a;
  a.pcm = pcm; a.n_in = n_in; a.first = first; a.taps = taps; a.n_out = n_out; a.out = out;
  a.in_stride = in_stride; a.out_stride = out_stride; a.C = C; a.o = o; a.n = n; a.w = w;
  a.T = identity ? 0 : taps_per_phase;
  size_t lds = 0;
  if (!identity) {
    const size_t span = audio_pre_span(o, n, w, taps_per_phase);
    lds = 4 * span;
    if (lds > AUDIO_PRE_LDS_LIMIT) return VAURA_ERR_SHAPE;
    a.span = (int)span;
  } else {
    a.span = 0;
  }
  const dim3 grid((unsigned)((out_stride + AUDIO_PRE_TILE - 1) / AUDIO_PRE_TILE), (unsigned)B);
  hipStream_t st = as_stream(s);
  switch (format) {
    case VAURA_PCM_S16: return audio_pre_launch<int16_t>(a, interleaved, grid, lds, st);
    case VAURA_PCM_S32: return audio_pre_launch<int32_t>(a, interleaved, grid, lds, st);
    default: return audio_pre_launch<float>(a, interleaved, grid, lds, st);
  }
}

size_t vaura_audio_preprocess_lds_bytes(int o, int n, int w, int taps_per_phase) {
  if (o <= 0 || n <= 0 || w < 0 || taps_per_phase <= 0) return 0;
  return 4 * audio_pre_span(o, n, w, taps_per_phase);
}

int vaura_audio_preprocess_tile(void) { return AUDIO_PRE_TILE; }

}  // extern "C"
