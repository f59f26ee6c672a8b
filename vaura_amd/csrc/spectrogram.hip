// Spectrogram: the codec's mono fp32 rows (44.1 kHz) -> power / log-mel columns, in one launch; one pass or block by block.  With hop 512
// (the codec's hop) column t is codec frame t.  One column, all fp32, for clip b with samples x[0 .. n_b) and x[s] = 0 outside:
//   columns   cols_b = ceil(n_b / hop); column t is centred on sample hop t + hop/2 and covers lo = hop t + hop/2 - n_fft/2 .. lo + n_fft - 1
//   frame     y[i] = w[i] * x[lo + i], one product; w is the periodic Hann window (vaura_amd/spectrogram.py: window(), float64 rounded once)
//   spectrum  X[k] = sum_i y[i] e^{-2 pi i ik / n_fft}, k = 0 .. n_fft/2;  P[k] = re * re + im * im (two products, one sum)
//   mel       M[m] = sum_k f[m][k] P[k] over the filter's contiguous support, ascending k: acc = 0, acc = fmaf(f, P[k], acc)
//   scale     POWER v;  DB 10 * log10f(v < amin ? amin : v);  LOG logf(v < amin ? amin : v)   (a NaN stays a NaN);  COMPLEX (linear
//             spectrum only): X[k] itself, (re, im) pairs — what the parity test measures the transform on
//   output    (B, out_stride, F) time-major — COMPLEX: (B, out_stride, F, 2) —: row i of clip b is column t0 + i, zeros from `count`
//             to the row's end
// Stream position.  x[s] is indexed ABSOLUTELY, as in audio_out.hip: clip b's record says which samples this launch holds — the block
// [r0, r0 + L) and, in front of it, the carry row [r0 - H, r0) — and which columns [t0, t0 + count) it forms.  A column's value depends
// on its absolute index and the samples of its window, never on where a block or a launch starts: the pushes of a stream, concatenated,
// are the one-pass call (r0 = t0 = 0, no carry, every clip final) bit for bit.
//
//   grid   (out_stride + (carry_out ? 1 : 0), B): one workgroup of 256 threads per (column, clip); a row behind the clip's count is
//          zero-filled and left.  The extra workgroup of a clip writes the NEXT carry row — the last H samples of carry ++ block —
//          into the other buffer of the caller's ping-pong pair, so no workgroup of the launch reads what another writes.
//   stage  the windowed frame goes to LDS packed as N = n_fft/2 complex points z[j] = y[2j] + i y[2j + 1]
//   FFT    Stockham autosort, decimation in frequency, between two LDS images: radix-4 stages with strides s = 1, 4, 16, .. and, for
//          N = 512, one closing radix-2 stage.  The plan is fixed per n_fft (a template instance per size): N = 256: 4 4 4 4,
//          N = 512: 4 4 4 4 2, N = 1024: 4 4 4 4 4.  Butterfly j of a stage reads the points j + k N/4 and writes q + s (4p + k),
//          p = j / s, q = j % s.  Twiddles come from ONE table built on the host in float64 and rounded once,
//          tw[t] = e^{-2 pi i t / n_fft}, t < 3 n_fft/4: a stage of sub-length n takes W_n^{kp} = tw[2 k p s].  No sincosf, no fast math.
//   post   X[k] = E + tw[k] O with E = (Z[k] + conj Z[N - k]) / 2, O = (Z[k] - conj Z[N - k]) / 2i, k = 0 .. N (Z[N] = Z[0]); P to LDS
//   mel    thread m forms M[m] in fixed order, scales, and the row leaves as plain contiguous vector stores
// LDS image.  Real and imaginary parts are separate fp32 arrays (every access is a 32-bit one: bank = word index mod 32, lanes
// conflict within a 32-lane half), the imaginary one 16 words further than N so the two halves of a wave's staging write fall on
// opposite halves of the banks.  Point i lives at word i ^ g(i), g = 5 * bit5(i) + 26 * bit6(i): bits 5 and 6 of the index are
// folded into the bank bits.  Reads of a stage are 32 consecutive points of one aligned block per half-wave: the fold is a constant
// there, a permutation of the banks — free.  Writes: at s = 1 the lanes of a half-wave differ in index bits 2 .. 6, at s = 4 in bits
// 0 1 4 5 6, at s = 16 in bits 0 .. 3 and 6 (linear, they would be 4-, 4- and 2-way conflicts); the fold makes each of these
// sets of 32 words distinct mod 32 (bit 5 goes to bank bits 0 and 2, bit 6 to 1, 3 and 4).  From s = 64 on a half-wave writes one
// aligned block.  The reversed read Z[N - k] of the post-pass straddles two blocks: at most one 2-way conflict per half-wave, once.
// Rounding count along one input-to-output path (the bar of tests/spectrogram_reference.py): window product 1; a radix-4 stage 2
// sums + twiddle entry 1 + product 1 + product sum 1 = 5 (its last instance multiplies by exactly 1: 2); the radix-2 stage 1; the
// post-pass sum 1 + twiddle entry 1 + product 1 + product sum 1 + final sum 1 = 5 (the halvings are exact).
//   n_fft 2048: 1 + 4 * 5 + 2 + 5 = 28;  n_fft 1024: 1 + 4 * 5 + 1 + 5 = 27;  n_fft 512: 1 + 3 * 5 + 2 + 5 = 23.
#include "common.h"

#define SPEC_THREADS 256
#define SPEC_MAX_MELS VAURA_SPECTROGRAM_MAX_MELS
#define SPEC_IM_GAP 16                        // the imaginary array starts at N + 16: opposite bank half from the real one

struct SpecArgs {
  const float* x;             // (B, in_stride): clip b's block
  const float* carry_in;      // (B, H): samples [r0 - H, r0) of clip b, or NULL with H == 0
  float* carry_out;           // (B, H) or NULL
  const long long* rec;       // (B, VAURA_SPECTROGRAM_RECORD): r0, L, t0, count, N (< 0: not the clip's last block)
  const float* window;        // (n_fft)
  const float2* tw;           // (3 n_fft / 4): e^{-2 pi i t / n_fft}
  const int32_t* mel_bins;    // (F, 3): first bin, count, offset into mel_weights; NULL: the linear spectrum
  const float* mel_weights;   // (mel_total)
  float* out;                 // (B, out_stride, F)
  long long in_stride, out_stride;
  int H, hop, F, scale, mel_total, cols;
  float amin;
};

struct SpecClip {
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

// word of point i inside one array of the image (i < N, N a multiple of 128: the result is below N too)
__device__ __forceinline__ int spec_word(int i) { return i ^ (((i >> 5) & 1) * 5) ^ (((i >> 6) & 1) * 26); }

__device__ __forceinline__ float2 spec_cmul(float2 a, float2 w) {
  return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

static size_t spec_lds_words(int n_fft) { return 2 * (size_t)(n_fft + 2 * SPEC_IM_GAP); }   // two images of N + (N + 16) + 16 words

__device__ __forceinline__ float spec_scale(float v, int scale, float amin) {
  if (scale == VAURA_SPEC_POWER) return v;
  const float c = v < amin ? amin : v;                                 // a NaN is not below amin: it stays
  return scale == VAURA_SPEC_DB ? 10.0f * log10f(c) : logf(c);
}

template <int NFFT>
__global__ __launch_bounds__(SPEC_THREADS) void spectrogram_kernel(const SpecArgs a) {
  constexpr int N = NFFT / 2, Q = N / 4, IMAGE = NFFT + 2 * SPEC_IM_GAP, IM = N + SPEC_IM_GAP;
  extern __shared__ float lds[];
  const int tid = threadIdx.x, b = blockIdx.y;
  const long long* rec = a.rec + (long long)b * VAURA_SPECTROGRAM_RECORD;
  SpecClip clip;
  clip.H = a.H;
  clip.r0 = rec[0];
  clip.L = min(max(rec[1], 0ll), a.in_stride);                         // clamped: no record can make an index leave the clip's rows
  clip.N = rec[4];
  clip.x = a.x + (long long)b * a.in_stride;
  clip.carry = a.carry_in + (long long)b * a.H;
  if ((int)blockIdx.x >= a.cols) {                                     // the next carry: the last H samples of carry ++ block
    float* next = a.carry_out + (long long)b * a.H;
    for (int i = tid; i < a.H; i += SPEC_THREADS) {
      const long long j = clip.L - a.H + i;                            // relative to r0
      next[i] = j >= 0 ? clip.x[j] : clip.carry[a.H + j];
    }
    return;
  }
  const long long count = min(max(rec[3], 0ll), a.out_stride);
  const int width = a.scale == VAURA_SPEC_COMPLEX ? 2 * a.F : a.F;     // values of one row
  float* row = a.out + ((long long)b * a.out_stride + blockIdx.x) * width;
  if ((long long)blockIdx.x >= count) {                                // behind the clip's columns: zeros only
    for (int m = tid; m < width; m += SPEC_THREADS) row[m] = 0.f;
    return;
  }
  const long long t = max(rec[2], 0ll) + blockIdx.x;                   // the column's absolute index
  const long long lo = t * a.hop + a.hop / 2 - N;
  float* src = lds;
  float* dst = lds + IMAGE;
  for (int i = tid; i < NFFT; i += SPEC_THREADS)                       // z[j] = y[2j] + i y[2j + 1]
    src[(i & 1) * IM + spec_word(i >> 1)] = a.window[i] * clip.sample(lo + i);
  __syncthreads();
  int s = 1;
#pragma unroll
  for (int n = N; n >= 4; n >>= 2, s <<= 2) {
    for (int j = tid; j < Q; j += SPEC_THREADS) {
      const int p = j / s, q = j - p * s;
      const int i0 = spec_word(j), i1 = spec_word(j + Q), i2 = spec_word(j + 2 * Q), i3 = spec_word(j + 3 * Q);
      const float2 A = make_float2(src[i0], src[IM + i0]), B = make_float2(src[i1], src[IM + i1]);
      const float2 C = make_float2(src[i2], src[IM + i2]), D = make_float2(src[i3], src[IM + i3]);
      const float2 apc = make_float2(A.x + C.x, A.y + C.y), amc = make_float2(A.x - C.x, A.y - C.y);
      const float2 bpd = make_float2(B.x + D.x, B.y + D.y);
      const float2 jbmd = make_float2(-(B.y - D.y), B.x - D.x);       // i (b - d)
      const int tw1 = 2 * p * s;                                       // W_n^p = tw[2 p s]; 3 tw1 < 3 n_fft / 4
      const float2 y0 = make_float2(apc.x + bpd.x, apc.y + bpd.y);
      const float2 y1 = spec_cmul(make_float2(amc.x - jbmd.x, amc.y - jbmd.y), a.tw[tw1]);
      const float2 y2 = spec_cmul(make_float2(apc.x - bpd.x, apc.y - bpd.y), a.tw[2 * tw1]);
      const float2 y3 = spec_cmul(make_float2(amc.x + jbmd.x, amc.y + jbmd.y), a.tw[3 * tw1]);
      const int o = q + 4 * s * p;
      const int o0 = spec_word(o), o1 = spec_word(o + s), o2 = spec_word(o + 2 * s), o3 = spec_word(o + 3 * s);
      dst[o0] = y0.x; dst[IM + o0] = y0.y;
      dst[o1] = y1.x; dst[IM + o1] = y1.y;
      dst[o2] = y2.x; dst[IM + o2] = y2.y;
      dst[o3] = y3.x; dst[IM + o3] = y3.y;
    }
    __syncthreads();
    float* sw = src; src = dst; dst = sw;
  }
  if (N == 512) {                                                      // the closing radix-2 stage: n = 2, s = N / 2, twiddle 1
    for (int j = tid; j < N / 2; j += SPEC_THREADS) {
      const int i0 = spec_word(j), i1 = spec_word(j + N / 2);
      const float2 A = make_float2(src[i0], src[IM + i0]), B = make_float2(src[i1], src[IM + i1]);
      dst[i0] = A.x + B.x; dst[IM + i0] = A.y + B.y;
      dst[i1] = A.x - B.x; dst[IM + i1] = A.y - B.y;
    }
    __syncthreads();
    float* sw = src; src = dst; dst = sw;
  }
  // the real-input post-pass: Z = src -> P[0 .. N] in the other image (plain words, no fold)
  float* P = dst;
  for (int k = tid; k <= N; k += SPEC_THREADS) {
    const int ik = spec_word(k & (N - 1)), im = spec_word((N - k) & (N - 1));
    const float zr = src[ik], zi = src[IM + ik], mr = src[im], mi = src[IM + im];
    const float er = (zr + mr) * 0.5f, ei = (zi - mi) * 0.5f;         // E = (Z[k] + conj Z[N - k]) / 2
    const float orr = (zi + mi) * 0.5f, oi = (mr - zr) * 0.5f;        // O = (Z[k] - conj Z[N - k]) / 2i
    const float2 w = a.tw[k];
    const float re = er + (orr * w.x - oi * w.y), imv = ei + (orr * w.y + oi * w.x);
    if (a.scale == VAURA_SPEC_COMPLEX) {
      row[2 * k] = re;
      row[2 * k + 1] = imv;
    }
    P[k] = re * re + imv * imv;
  }
  if (a.scale == VAURA_SPEC_COMPLEX) return;                           // uniform: the whole workgroup leaves
  __syncthreads();
  if (a.mel_bins) {
    for (int m = tid; m < a.F; m += SPEC_THREADS) {
      // held inside P and inside the packed weights: no table content can index outside either
      const int first = min(max(a.mel_bins[3 * m], 0), N);
      const int cnt = min(max(a.mel_bins[3 * m + 1], 0), min(N + 1 - first, a.mel_total));
      const float* f = a.mel_weights + min(max(a.mel_bins[3 * m + 2], 0), a.mel_total - cnt);
      float acc = 0.f;
      for (int k = 0; k < cnt; ++k) acc = fmaf(f[k], P[first + k], acc);
      row[m] = spec_scale(acc, a.scale, a.amin);
    }
  } else {
    for (int k = tid; k < a.F; k += SPEC_THREADS) row[k] = spec_scale(P[k], a.scale, a.amin);
  }
}

extern "C" {

int vaura_spectrogram(const float* x, int B, int64_t in_stride, const int64_t* records, const float* carry_in, float* carry_out,
                      int history, int n_fft, int hop, const float* window, const float* twiddles, const int32_t* mel_bins,
                      const float* mel_weights, int mel_total, int F, int scale, float amin, float* out, int64_t out_stride,
                      vaura_stream_t s) {
  if (!x || !records || !window || !twiddles) return VAURA_ERR_ARG;
  if (in_stride < 0 || out_stride < 0 || history < 0) return VAURA_ERR_ARG;                   // negative lengths
  if (B <= 0 || in_stride == 0) return VAURA_ERR_ARG;
  if (out_stride > 0 && !out) return VAURA_ERR_ARG;
  if (history > 0 && !carry_in) return VAURA_ERR_ARG;
  if (carry_out && history == 0) return VAURA_ERR_ARG;
  if ((mel_bins == nullptr) != (mel_weights == nullptr)) return VAURA_ERR_ARG;                // the table is there or it is not
  if (!(amin > 0.f)) return VAURA_ERR_ARG;                                                    // a NaN too
  if (carry_out && B <= 65535) {                                       // the ping-pong pair: the two (B, history) spans must not overlap
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(carry_in), out0 = reinterpret_cast<uintptr_t>(carry_out);
    const uintptr_t bytes = (uintptr_t)B * (uintptr_t)history * 4;
    if (in0 < out0 + bytes && out0 < in0 + bytes) return VAURA_ERR_ARG;
  }
  if (scale != VAURA_SPEC_POWER && scale != VAURA_SPEC_DB && scale != VAURA_SPEC_LOG && scale != VAURA_SPEC_COMPLEX) return VAURA_ERR_DTYPE;
  if (scale == VAURA_SPEC_COMPLEX && mel_bins) return VAURA_ERR_ARG;                          // the mel bands have no phase
  if (n_fft != 512 && n_fft != 1024 && n_fft != 2048) return VAURA_ERR_SHAPE;
  if (hop < 1 || hop > n_fft || (hop & (hop - 1))) return VAURA_ERR_SHAPE;
  if (mel_bins) {
    if (F < 1 || F > SPEC_MAX_MELS) return VAURA_ERR_SHAPE;
    // every filter holds at least one weight and none leaves the bins 0 .. n_fft/2
    if (mel_total < F || (int64_t)mel_total > (int64_t)F * (n_fft / 2 + 1)) return VAURA_ERR_SHAPE;
  } else if (F != n_fft / 2 + 1) {
    return VAURA_ERR_SHAPE;
  }
  if (in_stride > INT32_MAX || out_stride > INT32_MAX - 1 || history > INT32_MAX / 2) return VAURA_ERR_SHAPE;
  if (B > 65535) return VAURA_ERR_SHAPE;                               // gridDim.y
  if ((reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(records) & 7) || (reinterpret_cast<uintptr_t>(carry_in) & 3) ||
      (reinterpret_cast<uintptr_t>(carry_out) & 3) || (reinterpret_cast<uintptr_t>(window) & 3) || (reinterpret_cast<uintptr_t>(twiddles) & 7) ||
      (reinterpret_cast<uintptr_t>(mel_bins) & 3) || (reinterpret_cast<uintptr_t>(mel_weights) & 3) || (reinterpret_cast<uintptr_t>(out) & 3))
    return VAURA_ERR_ARG;
  SpecArgs a;
  a.x = x; a.carry_in = carry_in; a.carry_out = carry_out; a.rec = reinterpret_cast<const long long*>(records); a.window = window;
  a.tw = reinterpret_cast<const float2*>(twiddles); a.mel_bins = mel_bins; a.mel_weights = mel_weights; a.out = out;
  a.in_stride = in_stride; a.out_stride = out_stride; a.H = history; a.hop = hop; a.F = F; a.scale = scale;
  a.mel_total = mel_bins ? mel_total : 0; a.cols = (int)out_stride; a.amin = amin;
  const unsigned gx = (unsigned)out_stride + (carry_out ? 1u : 0u);
  if (gx == 0) return 0;                                               // no column and no carry to write
  const dim3 grid(gx, (unsigned)B);
  const size_t lds = 4 * spec_lds_words(n_fft);
  hipStream_t st = as_stream(s);
  switch (n_fft) {
    case 512: VA_LAUNCH((spectrogram_kernel<512>), grid, dim3(SPEC_THREADS), lds, st, a); break;
    case 1024: VA_LAUNCH((spectrogram_kernel<1024>), grid, dim3(SPEC_THREADS), lds, st, a); break;
    default: VA_LAUNCH((spectrogram_kernel<2048>), grid, dim3(SPEC_THREADS), lds, st, a); break;
  }
  return 0;
}

size_t vaura_spectrogram_lds_bytes(int n_fft, int F) {
  if ((n_fft != 512 && n_fft != 1024 && n_fft != 2048) || F < 1 || F > n_fft / 2 + 1) return 0;
  return 4 * spec_lds_words(n_fft);
}

}  // extern "C"
