// Streaming loudness: an ITU-R BS.1770 meter (K-weighting, 400 ms blocks every 100 ms, two gates) and a CAUSAL loudness normaliser on
// top of it, one pass or block by block.  The one-thread-per-clip recursion of post.hip (audio_loudness_gain_kernel) stays as it is and
// keeps its bits; nothing here replaces it.  With step = nearbyint(0.1 rate), gate = 4 step, for clip b with samples x[0 .. n_b):
//   K-weighting  the two biquads of post.hip (treble shelf, then 38 Hz high-pass), coefficients derived in double and KEPT in double,
//                each recursion in fp64, direct form I on its unclamped state:  y[i] = ((b0 x[i] + b1 x[i-1]) + b2 x[i-2]) - a1 y[i-1]
//                - a2 y[i-2];  the first stage's output is clamped to [-1, 1] before it enters the second, the second's is clamped and
//                rounded to fp32 once: w[i].  (The clamp is v < -1 ? -1 : v > 1 ? 1 : v: a NaN stays a NaN.)
//   parallel     a step is cut into C = ceil(step / L) lane chunks of L = ceil(step / 256) samples at ABSOLUTE indices (chunk c of step j
//                is always samples j step + c L ..).  Every lane runs its chunk from a zero y-state (the x-history is data); thread 0
//                chains the chunk end-states in chunk order, s' = zs_end + M s, M = the chunk's transition from the host's fp64 table
//                (one matrix for the full chunks, one for the last); every lane then adds h1[i] s1 + h2[i] s2, the homogeneous responses
//                of the same table.  Stage one is complete (and clamped) before stage two starts.
//   energies     S_j = sum of (double) w^2 over step j: every lane sums its chunk in ascending order, thread 0 sums the lanes in ascending
//                order; rounded to fp32 and kept in a ring of R = max(history_steps, 32) entries: S_j lives at j % R.
//   meter        energy(j) = (((S_j + S_j+1) + S_j+2) + S_j+3) / (float) gate, loudness l = -0.691f + 10 log10f(energy), both as post.hip
//                writes them.  Momentary M_j = l of block j; short-term = the same over 30 steps, / (float)(30 step).  Integrated at
//                boundary m (m steps complete, m >= 4): the blocks j in [max(0, m - history_steps), m - 4], absolute gate l > -70,
//                relative gate 10 LU below the mean of the absolutely gated; thread t sums the blocks lo + t, lo + t + 256, .. in ascending
//                order, the 256 partials are reduced in one fixed order (wave butterfly, then ((w0 + w1) + w2) + w3).  Undefined (NaN)
//                where no block exists, none passes a gate, or the result is not finite.
//   normaliser   d_m = clamp(target - I_m, +-max_gain_db), d_m = d_{m-1} where I_m is undefined, d_{-1} = initial_gain_db; with a slew
//                d_m = d_{m-1} + clamp(d_m - d_{m-1}, +-slew_step);  a_m = powf(10, d_m / 20).  Sample i, m = i / step, k = i - m step:
//                g = a_{m-1} + (a_m - a_{m-1}) * ((float)(k + 1) / (float) step), y = x g, clipped[b] counts |y| > 1, out = clip(y) or
//                clip(tanhf(y)).  a_m needs only the steps below m: every pushed sample leaves in the same push.
// One push: record (r0, n) per clip = samples received before and samples brought now.  The steps [r0 / step, (r0 + n) / step) become
// complete: their samples are the carry row (the raw tail shorter than one step) followed by the block.  Everything a value depends on is
// its absolute index and the clip's samples, never where a push starts: the pushes of a stream, concatenated, are the one-pass call.
//   grid   loudness_push_kernel: B workgroups of 256 threads, one per clip: per new step the two filter stages, S_j, the boundary j + 1.
//          One workgroup owns a clip's state (filter state fp64, d, a_{m-1}, a_m, I, the ring, the carry row): it is read and written in
//          place, no other workgroup touches it, so no second copy is needed.  Where no row brings more than LOUD_FUSE_MAX samples the
//          same workgroup applies the gains (one launch); otherwise loudness_apply_kernel does, on a (tiles, B) grid.
//   LDS    (step + 2) doubles (the step in place, two history slots in front) + 11.2 KB static.
#include "common.h"
#include <cmath>

#define LOUD_THREADS 256
#define LOUD_HEAD 24                       // words in front of the ring: 8 doubles of filter state, d, a_prev, a_cur, I, 4 spare
#define LOUD_RING_MIN 32                   // the short-term window is 30 steps
#define LOUD_FUSE_MAX 16384                // samples per row up to which the meter's workgroup applies the gains itself
#define LOUD_FUSE_GAINS (LOUD_FUSE_MAX / 800 + 4)   // step >= 800 (8 kHz): boundaries of such a push, + 2
#define LOUD_TABLE_MAX (10 + 2 * (2 * 19 + 8))   // the table at 48 kHz: L = ceil(4800 / 256) = 19
#define LOUD_APPLY_TILE (4 * LOUD_THREADS)  // samples per workgroup and pass of loudness_apply_kernel: four per thread

struct LoudArgs {
  const float* x;             // (B, in_stride): clip b's block
  float* out;                 // (B, in_stride) or NULL: only the meter runs
  const long long* rec;       // (B, VAURA_LOUDNESS_RECORD): r0, n
  float* state;               // (B, state_stride)
  const double* table;        // coefficients (10), then per stage h1 (L), h2 (L), M of a full chunk (4), M of the last chunk (4)
  float* gains;               // (B, mstride + 2): a_{M0 - 1}, a_{M0}, .., a_{M1}
  float* meter;               // (3, B, mstride): I at the new boundaries; the momentary and the short-term values they complete, NaN behind
  float* info;                // (B, 2): d and I at the last boundary
  int32_t* clipped;           // (B), added to
  long long in_stride, state_stride;
  int mstride, step, L, C, hist, R, has_slew, limiter, fused, B;
  float target, max_gain, slew_step, init_db;
};

__device__ __forceinline__ double loud_clamp(double v) { return v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v); }

// One biquad over the step held in buf[2 .. 2 + step) (buf[0], buf[1] = the inputs two and one sample before it), in place: clamped
// outputs replace the inputs.  s1, s2 (thread 0): the unclamped y-state in front of the step, replaced by the one behind it.  FINAL:
// returns the lane's sum of squares of the fp32-rounded outputs instead of leaving them for a next stage.
template <bool FINAL>
__device__ __forceinline__ double loud_stage(double* buf, double* es, double* ss, const double* __restrict__ co,
                                             const double* __restrict__ tab, int step, int L, int C, double& s1, double& s2) {
  const int tid = threadIdx.x, i0 = tid * L;
  const int len = tid < C ? min(L, step - i0) : 0;
  const double b0 = co[0], b1 = co[1], b2 = co[2], a1 = co[3], a2 = co[4];
  double x1 = 0.0, x2 = 0.0;
  if (len) { x1 = buf[i0 + 1]; x2 = buf[i0]; }                       // the two inputs in front of the chunk: another lane's, read first
  __syncthreads();
  double y1 = 0.0, y2 = 0.0;
  for (int k = 0; k < len; ++k) {
    const double xi = buf[2 + i0 + k];
    const double y = ((b0 * xi + b1 * x1) + b2 * x2) - a1 * y1 - a2 * y2;
    buf[2 + i0 + k] = y;
    x2 = x1; x1 = xi; y2 = y1; y1 = y;
  }
  es[2 * tid] = y1; es[2 * tid + 1] = y2;                            // zero-state end of the chunk (a one-sample chunk: y2 = 0)
  __syncthreads();
  if (tid == 0) {                                                    // the chain, in chunk order: ss[c] = the state in front of chunk c
    const double* Mf = tab + 2 * L;                                    // (read from es, written to ss: the loads do not wait for the stores)
    const double m0 = Mf[0], m1 = Mf[1], m2 = Mf[2], m3 = Mf[3];
    double p1 = s1, p2 = s2;
#pragma unroll 8
    for (int c = 0; c < C - 1; ++c) {
      const double e1 = es[2 * c], e2 = es[2 * c + 1];
      ss[2 * c] = p1; ss[2 * c + 1] = p2;
      const double n1 = e1 + (m0 * p1 + m1 * p2), n2 = e2 + (m2 * p1 + m3 * p2);
      p1 = n1; p2 = n2;
    }
    const double* Ml = Mf + 4;                                         // the step's last chunk has its own length
    ss[2 * (C - 1)] = p1; ss[2 * (C - 1) + 1] = p2;
    s1 = es[2 * (C - 1)] + (Ml[0] * p1 + Ml[1] * p2);
    s2 = es[2 * (C - 1) + 1] + (Ml[2] * p1 + Ml[3] * p2);
  }
  __syncthreads();
  const double c1 = ss[2 * tid], c2 = ss[2 * tid + 1];
  double acc = 0.0;
  for (int k = 0; k < len; ++k) {
    const double y = loud_clamp(buf[2 + i0 + k] + (tab[k] * c1 + tab[L + k] * c2));
    if (FINAL) {
      const float w = (float)y;
      acc += (double)w * (double)w;
    } else {
      buf[2 + i0 + k] = y;
    }
  }
  __syncthreads();
  return acc;
}

// (sum, count) of the workgroup in one fixed order; red: 8 floats
__device__ __forceinline__ void loud_block_sum(float& s, float& c, float* red) {
  s = wave_sum(s);
  c = wave_sum(c);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = s; red[4 + (threadIdx.x >> 6)] = c; }
  __syncthreads();
  s = ((red[0] + red[1]) + red[2]) + red[3];
  c = ((red[4] + red[5]) + red[6]) + red[7];
}

// the samples [0, n) of one row, from `first` in strides of `stride`: gains g[0] = a_{M0 - 1}, g[1] = a_{M0}, ..; zeros up to in_stride
__device__ __forceinline__ void loud_apply(const LoudArgs& a, int b, long long r0, long long n, long long M0, const float* g,
                                           long long first, long long stride) {
  // a record that promises more boundaries than the gains row holds is cut where the row ends
  n = min(n, max((M0 + a.mstride + 1) * (long long)a.step - r0, 0ll));
  const float* x = a.x + (long long)b * a.in_stride;
  float* o = a.out + (long long)b * a.in_stride;
  const bool vec = !(a.in_stride & 3) && !((reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.out)) & 15);
  const float fstep = (float)a.step;
  int over = 0;
  for (long long i = first; i < a.in_stride; i += stride) {           // i: a multiple of 4
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (i < n) {
      if (vec && i + 3 < n) {
        const float4 q = *reinterpret_cast<const float4*>(x + i);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
        for (int e = 0; e < 4; ++e) if (i + e < n) v[e] = x[i + e];  // nothing behind n is read
      }
      long long m = (r0 + i) / a.step;
      int k = (int)((r0 + i) - m * a.step);
      for (int e = 0; e < 4; ++e) {
        if (i + e < n) {
          const float a0 = g[m - M0], a1 = g[m - M0 + 1];
          const float gain = a0 + (a1 - a0) * ((float)(k + 1) / fstep);
          float y = v[e] * gain;
          if (fabsf(y) > 1.f) ++over;
          if (a.limiter) y = tanhf(y);
          v[e] = fminf(fmaxf(y, -1.f), 1.f);
        }
        if (++k == a.step) { k = 0; ++m; }
      }
    }
    if (vec) {
      *reinterpret_cast<float4*>(o + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int e = 0; e < 4; ++e) if (i + e < a.in_stride) o[i + e] = v[e];
    }
  }
  if (over) atomicAdd(a.clipped + b, over);                            // an integer count: the order of the additions does not show
}

__global__ __launch_bounds__(LOUD_THREADS) void loudness_push_kernel(const LoudArgs a) {
  extern __shared__ double loud_buf[];                                 // step + 2
  __shared__ double es[2 * LOUD_THREADS];
  __shared__ double ss[2 * LOUD_THREADS];
  __shared__ double tabs[LOUD_TABLE_MAX];
  __shared__ double part[LOUD_THREADS];
  __shared__ float red[8];
  __shared__ float gl[LOUD_FUSE_GAINS];
  const int tid = threadIdx.x, b = blockIdx.x, step = a.step, R = a.R;
  const long long r0 = max(a.rec[2 * b], 0ll);
  const long long n = min(max(a.rec[2 * b + 1], 0ll), a.in_stride);    // clamped: no record can make an index leave the clip's rows
  const long long M0 = r0 / step, M1 = (r0 + n) / step;
  const int nb = (int)min(M1 - M0, (long long)a.mstride);
  float* st = a.state + (long long)b * a.state_stride;
  double* fs = reinterpret_cast<double*>(st);                          // y1 y2 x1 x2 of the shelf, v1 v2 u1 u2 of the high-pass
  float* ring = st + LOUD_HEAD;
  float* carry = ring + R;
  const float* x = a.x + (long long)b * a.in_stride;
  const float gate = (float)(4 * step);
  const float nanv = __int_as_float(0x7fc00000);
  double f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float d = a.init_db, ap = powf(10.f, a.init_db / 20.f), ac = ap, Ilast = nanv;
  if (r0 > 0) {                                                        // a stream's first push reads no state: it may hold anything
    for (int i = 0; i < 8; ++i) f[i] = fs[i];
    d = st[16]; ap = st[17]; ac = st[18]; Ilast = st[19];
  }
  float* G = a.gains + (long long)b * (a.mstride + 2);
  float* mi = a.meter + (long long)b * a.mstride;
  float* mm = mi + (long long)a.B * a.mstride;
  float* ms = mm + (long long)a.B * a.mstride;
  if (tid == 0) { G[0] = ap; G[1] = ac; }
  if (a.fused && tid == 0) { gl[0] = ap; gl[1] = ac; }
  const long long mom0 = max(M0 + 1, 4ll), st0 = max(M0 + 1, 30ll);   // the first boundary of this push that completes a block / a 3 s window
  for (int i = tid; i < 10 + 2 * (2 * a.L + 8); i += LOUD_THREADS) tabs[i] = a.table[i];      // the table: read from LDS inside the loops
  const double* co = tabs;
  const double* tab0 = tabs + 10;
  const double* tab1 = tab0 + 2 * a.L + 8;
  for (int q = 0; q < nb; ++q) {
    const long long j = M0 + q, base = j * step;
    for (int i = tid; i < step; i += LOUD_THREADS) {
      const long long s = base + i;
      const float* src = s < r0 ? carry + (s - M0 * step) : x + (s - r0);       // one load behind a selected address
      loud_buf[2 + i] = (double)*src;
    }
    if (tid == 0) { loud_buf[0] = f[3]; loud_buf[1] = f[2]; }
    __syncthreads();
    const double lx1 = loud_buf[step + 1], lx2 = loud_buf[step];      // the raw inputs that end the step
    loud_stage<false>(loud_buf, es, ss, co, tab0, step, a.L, a.C, f[0], f[1]);
    f[2] = lx1; f[3] = lx2;
    if (tid == 0) { loud_buf[0] = f[7]; loud_buf[1] = f[6]; }
    __syncthreads();
    const double lu1 = loud_buf[step + 1], lu2 = loud_buf[step];      // the clamped shelf outputs that end the step
    part[tid] = loud_stage<true>(loud_buf, es, ss, co + 5, tab1, step, a.L, a.C, f[4], f[5]);
    f[6] = lu1; f[7] = lu2;
    __syncthreads();
    if (tid == 0) {
      double S = 0.0;
      for (int c = 0; c < a.C; ++c) S += part[c];
      ring[j % R] = (float)S;
    }
    __syncthreads();
    // boundary m: the steps below m are complete
    const long long m = j + 1;
    auto energy = [&](long long blk) { float e = 0.f; for (int p = 0; p < 4; ++p) e += ring[(blk + p) % R]; return e / gate; };
    float I = nanv;
    if (m >= 4) {
      const long long lo = max(0ll, m - a.hist), hi = m - 4;
      float s1 = 0.f, c1 = 0.f;
      for (long long blk = lo + tid; blk <= hi; blk += LOUD_THREADS) {
        const float e = energy(blk);
        if (-0.691f + 10.f * log10f(e) > -70.f) { s1 += e; c1 += 1.f; }
      }
      loud_block_sum(s1, c1, red);
      if (c1 > 0.f) {
        const float gamma_rel = -0.691f + 10.f * log10f(s1 / c1) - 10.f;
        float s2 = 0.f, c2 = 0.f;
        for (long long blk = lo + tid; blk <= hi; blk += LOUD_THREADS) {
          const float e = energy(blk);
          const float l = -0.691f + 10.f * log10f(e);
          if (l > -70.f && l > gamma_rel) { s2 += e; c2 += 1.f; }
        }
        loud_block_sum(s2, c2, red);
        if (c2 > 0.f) {
          const float lkfs = -0.691f + 10.f * log10f(s2 / c2);
          if (isfinite(lkfs)) I = lkfs;
        }
      }
    }
    float dn = d;
    if (I == I) dn = fminf(fmaxf(a.target - I, -a.max_gain), a.max_gain);
    if (a.has_slew) dn = d + fminf(fmaxf(dn - d, -a.slew_step), a.slew_step);
    d = dn; ap = ac; ac = powf(10.f, d / 20.f); Ilast = I;
    if (tid == 0) {
      G[q + 2] = ac;
      if (a.fused) gl[q + 2] = ac;
      mi[q] = I;
      if (m >= 4) mm[m - mom0] = -0.691f + 10.f * log10f(energy(m - 4));
      if (m >= 30) {
        float e = 0.f;
        for (int p = 0; p < 30; ++p) e += ring[(m - 30 + p) % R];
        ms[m - st0] = -0.691f + 10.f * log10f(e / (float)(30 * step));
      }
    }
    __syncthreads();                                                   // the ring is read before the next step writes it
  }
  // rows of the meter behind what this push completed
  const long long last = M0 + nb;
  const int cnt_m = (int)max(0ll, last - mom0 + 1), cnt_s = (int)max(0ll, last - st0 + 1);
  for (int i = tid; i < a.mstride; i += LOUD_THREADS) {
    if (i >= nb) mi[i] = nanv;
    if (i >= cnt_m) mm[i] = nanv;
    if (i >= cnt_s) ms[i] = nanv;
  }
  // the next carry row: the raw tail behind the last whole step
  if (M1 == M0) {
    const int tail0 = (int)(r0 - M0 * step);
    for (long long i = tid; i < n; i += LOUD_THREADS) carry[tail0 + i] = x[i];
  } else {
    const long long from = M1 * step - r0, tail1 = r0 + n - M1 * step;
    for (long long i = tid; i < tail1; i += LOUD_THREADS) carry[i] = x[from + i];
  }
  if (tid == 0) {
    for (int i = 0; i < 8; ++i) fs[i] = f[i];
    st[16] = d; st[17] = ap; st[18] = ac; st[19] = Ilast;
    a.info[2 * b] = d; a.info[2 * b + 1] = Ilast;
  }
  if (a.fused && a.out) {
    __syncthreads();
    loud_apply(a, b, r0, n, M0, gl, 4ll * tid, 4ll * LOUD_THREADS);
  }
}

__global__ __launch_bounds__(LOUD_THREADS) void loudness_apply_kernel(const LoudArgs a) {
  const int b = blockIdx.y;
  const long long r0 = max(a.rec[2 * b], 0ll);
  const long long n = min(max(a.rec[2 * b + 1], 0ll), a.in_stride);
  const float* g = a.gains + (long long)b * (a.mstride + 2);
  loud_apply(a, b, r0, n, r0 / a.step, g, (long long)blockIdx.x * LOUD_APPLY_TILE + 4ll * threadIdx.x,
             (long long)gridDim.x * LOUD_APPLY_TILE);
}

// step of a rate, or 0 where the rate is refused: outside 8 .. 48 kHz, or a gating block that is not four whole steps (11 025 Hz)
static int loud_step(int sample_rate) {
  if (sample_rate < 8000 || sample_rate > 48000) return 0;
  const int step = (int)nearbyint(0.1 * (double)sample_rate);
  return (int)nearbyint(0.4 * (double)sample_rate) == 4 * step ? step : 0;
}
static int loud_ring(int history_steps) { return history_steps > LOUD_RING_MIN ? history_steps : LOUD_RING_MIN; }
static size_t loud_state_stride(int step, int history_steps) { return ((size_t)LOUD_HEAD + loud_ring(history_steps) + step + 3) & ~(size_t)3; }

extern "C" {

size_t vaura_audio_loudness_state_elems(int n_clips, int sample_rate, int history_steps) {
  const int step = loud_step(sample_rate);
  if (n_clips <= 0 || !step || history_steps < VAURA_LOUDNESS_MIN_HISTORY || history_steps > VAURA_LOUDNESS_MAX_HISTORY) return 0;
  return (size_t)n_clips * loud_state_stride(step, history_steps);
}

size_t vaura_audio_loudness_table_elems(int sample_rate) {
  const int step = loud_step(sample_rate);
  if (!step) return 0;
  const int L = (step + LOUD_THREADS - 1) / LOUD_THREADS;
  return 10 + 2 * (2 * (size_t)L + 8);
}

size_t vaura_audio_loudness_lds_bytes(int sample_rate) {
  const int step = loud_step(sample_rate);
  if (!step) return 0;
  return (size_t)(step + 2) * 8 + (5 * LOUD_THREADS + LOUD_TABLE_MAX) * 8 + (8 + LOUD_FUSE_GAINS) * 4;
}

int vaura_audio_loudness_push(const float* x, float* out, int B, int64_t in_stride, const int64_t* records, float* state,
                              int sample_rate, int history_steps, const double* table, int64_t table_elems, float target_lkfs,
                              float max_gain_db, float slew_db_per_step, float initial_gain_db, int limiter, float* gains, float* meter,
                              int meter_stride, float* info, int32_t* clipped, vaura_stream_t s) {
  if (!x || !records || !state || !table || !gains || !meter || !info || !clipped) return VAURA_ERR_ARG;
  if (B <= 0 || in_stride <= 0 || meter_stride <= 0) return VAURA_ERR_ARG;
  if (!(max_gain_db >= 0.f) || !std::isfinite(max_gain_db) || !std::isfinite(target_lkfs) || !std::isfinite(initial_gain_db)) return VAURA_ERR_ARG;
  if (slew_db_per_step < 0.f || slew_db_per_step != slew_db_per_step) return VAURA_ERR_ARG;      // 0: no slew limit
  if (limiter != VAURA_LOUDNESS_CLIP && limiter != VAURA_LOUDNESS_TANH) return VAURA_ERR_DTYPE;
  const int step = loud_step(sample_rate);
  if (!step) return VAURA_ERR_SHAPE;
  if (history_steps < VAURA_LOUDNESS_MIN_HISTORY || history_steps > VAURA_LOUDNESS_MAX_HISTORY) return VAURA_ERR_SHAPE;
  if (in_stride > INT32_MAX || B > 65535) return VAURA_ERR_SHAPE;
  if ((uint64_t)table_elems != vaura_audio_loudness_table_elems(sample_rate)) return VAURA_ERR_ARG;
  if (out == x) return VAURA_ERR_ARG;                                  // not in place: a row's zeros would land on samples not yet read
  if ((reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(out) & 3) || (reinterpret_cast<uintptr_t>(records) & 7) ||
      (reinterpret_cast<uintptr_t>(state) & 7) || (reinterpret_cast<uintptr_t>(table) & 7) || (reinterpret_cast<uintptr_t>(gains) & 3) ||
      (reinterpret_cast<uintptr_t>(meter) & 3) || (reinterpret_cast<uintptr_t>(info) & 3) || (reinterpret_cast<uintptr_t>(clipped) & 3))
    return VAURA_ERR_ARG;
  LoudArgs a;
  a.x = x; a.out = out; a.rec = reinterpret_cast<const long long*>(records); a.state = state; a.table = table; a.gains = gains;
  a.meter = meter; a.info = info; a.clipped = clipped; a.in_stride = in_stride;
  a.state_stride = (long long)loud_state_stride(step, history_steps);
  a.mstride = meter_stride; a.step = step; a.L = (step + LOUD_THREADS - 1) / LOUD_THREADS; a.C = (step + a.L - 1) / a.L;
  a.hist = history_steps; a.R = loud_ring(history_steps); a.has_slew = slew_db_per_step > 0.f; a.limiter = limiter;
  a.fused = in_stride <= LOUD_FUSE_MAX; a.B = B;
  a.target = target_lkfs; a.max_gain = max_gain_db; a.slew_step = slew_db_per_step; a.init_db = initial_gain_db;
  hipStream_t st = as_stream(s);
  VA_LAUNCH(loudness_push_kernel, dim3((unsigned)B), dim3(LOUD_THREADS), (size_t)(step + 2) * 8, st, a);
  if (out && !a.fused) {
    const unsigned gx = (unsigned)((in_stride + LOUD_APPLY_TILE - 1) / LOUD_APPLY_TILE);
    VA_LAUNCH(loudness_apply_kernel, dim3(gx > 1024 ? 1024 : gx, (unsigned)B), dim3(LOUD_THREADS), 0, st, a);
  }
  return 0;
}

}  // extern "C"
