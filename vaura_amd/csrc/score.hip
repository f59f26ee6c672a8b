// Teacher-forced scoring: pattern revert + log-softmax + NLL of every scored logit row, and the per-codebook mean.
//   VAURAModel.forward (revert_pattern_logits)   models/vaura_model.py:136-192; codebook_patterns.py:287-313
//   VAURAModel._compute_loss                     models/vaura_model.py:240-280
// Model-output position s of codebook q predicts timestep t = s - d_q (the layout's step s + 1 holds (t, q) with t = s - d_q:
// revert_pattern_logits drops the first layout step, is_model_output=True).  Delay patterns cover every t < Ta, so the reference's
// mask is all true and its NaN fill never reaches a reverted row when every position is scored.
#include "common.h"

struct ScoreDelays { int32_t d[16]; };

__device__ __forceinline__ int score_delay(const ScoreDelays& pd, int q) {
  int dq = q;
#pragma unroll
  for (int j = 0; j < 16; ++j) if (j == q) dq = pd.d[j];     // static indices: a per-lane run-time index would go to scratch
  return dq;
}

// One wave per (position i, row b, codebook q): the 1024-logit row at logits + i * s_pos + b * s_row + q * s_cb, the head output of
// model-output position p0 + i.  The heads' row-major output over a chunk's row blocks is s_pos = rows_padded * K * V, s_row = K * V,
// s_cb = V; a reverted (B, K, Ta, V) tensor is read with p0 = 0, zero delays, s_pos = V, s_row = K * Ta * V, s_cb = Ta * V.
//   nll[b, q, t] = logsumexp(row) - row[target[b, q, t]]   (fp32; F.cross_entropy's log_softmax form: max, sum of exp(x - max))
//   logits_out[b, q, t, :] = row                            (optional: the reverted (B, K, Ta, V) tensor)
// A target outside [0, V) gives NaN (the reference's cross_entropy raises there; the engine checks the codes before the call).
__global__ __launch_bounds__(256) void score_nll_kernel(const float* __restrict__ logits, int64_t s_pos, int64_t s_row, int64_t s_cb, int p0,
                                                        int n_pos, int B, int K, int V, int Ta, ScoreDelays pd,
                                                        const int32_t* __restrict__ targets, float* __restrict__ nll,
                                                        float* __restrict__ logits_out) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (w >= (int64_t)n_pos * B * K) return;                   // wave-uniform
  const int q = (int)(w % K), b = (int)((w / K) % B), i = (int)(w / ((int64_t)K * B));
  const int t = p0 + i - score_delay(pd, q);
  if (t < 0 || t >= Ta) return;                              // no target: the reference drops these rows (wave-uniform)
  const float* row = logits + (size_t)i * s_pos + (size_t)b * s_row + (size_t)q * s_cb;
  const size_t bqt = ((size_t)b * K + q) * Ta + t;
  const int nq = V / 256;                                    // float4 per lane (V % 256 == 0: checked by the launcher)
  f32x4 x[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nq) x[j] = reinterpret_cast<const f32x4*>(row)[j * 64 + lane];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nq) m = fmaxf(m, fmaxf(fmaxf(x[j][0], x[j][1]), fmaxf(x[j][2], x[j][3])));
  m = wave_max(m);
  float se = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nq) se += ((expf(x[j][0] - m) + expf(x[j][1] - m)) + expf(x[j][2] - m)) + expf(x[j][3] - m);
  se = wave_sum(se);
  const int tg = targets[bqt];
  if (logits_out) {
    f32x4* o = reinterpret_cast<f32x4*>(logits_out + bqt * (size_t)V);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nq) va_st16(o + j * 64 + lane, x[j]);
  }
  if (lane == 0) {
    // NaN anywhere in the row survives: fmaxf drops it from m, but exp(NaN - m) carries it into the sum
    const float v = (tg >= 0 && tg < V) ? -((row[tg] - m) - logf(se)) : __builtin_nanf("");
    va_st4(nll + bqt, v);
  }
}

// score_nll_kernel with per-clip lengths (vaura_decoder_ext2.clip_timesteps): clip b holds Ta_b = clip_T[b] <= Ta timesteps, and a wave
// whose t >= Ta_b returns like one whose t >= Ta (wave-uniform: one vector load per wave, back to an SGPR; clamped to Ta, so no value can
// send a write out of the clip's rows).  What the finished clip's rows computed at such a position is ignored.  A copy of the kernel
// above, for the reason given at embed_clips_kernel (csrc/step.hip): the kernel every call without lengths runs stays untouched source.
__global__ __launch_bounds__(256) void score_nll_clips_kernel(const float* __restrict__ logits, int64_t s_pos, int64_t s_row, int64_t s_cb, int p0,
                                                              int n_pos, int B, int K, int V, int Ta, ScoreDelays pd,
                                                              const int32_t* __restrict__ targets, float* __restrict__ nll,
                                                              float* __restrict__ logits_out, const int32_t* __restrict__ clip_T) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (w >= (int64_t)n_pos * B * K) return;                   // wave-uniform
  const int q = (int)(w % K), b = (int)((w / K) % B), i = (int)(w / ((int64_t)K * B));
  const int t = p0 + i - score_delay(pd, q);
  int lane0 = 0;
  asm volatile("" : "+v"(lane0));
  const int Tb = min(__builtin_amdgcn_readfirstlane(clip_T[b + lane0]), Ta);
  if (t < 0 || t >= Tb) return;                              // no target, or behind the clip's own end (wave-uniform)
  const float* row = logits + (size_t)i * s_pos + (size_t)b * s_row + (size_t)q * s_cb;
  const size_t bqt = ((size_t)b * K + q) * Ta + t;
  const int nq = V / 256;                                    // float4 per lane (V % 256 == 0: checked by the launcher)
  f32x4 x[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nq) x[j] = reinterpret_cast<const f32x4*>(row)[j * 64 + lane];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nq) m = fmaxf(m, fmaxf(fmaxf(x[j][0], x[j][1]), fmaxf(x[j][2], x[j][3])));
  m = wave_max(m);
  float se = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nq) se += ((expf(x[j][0] - m) + expf(x[j][1] - m)) + expf(x[j][2] - m)) + expf(x[j][3] - m);
  se = wave_sum(se);
  const int tg = targets[bqt];
  if (logits_out) {
    f32x4* o = reinterpret_cast<f32x4*>(logits_out + bqt * (size_t)V);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nq) va_st16(o + j * 64 + lane, x[j]);
  }
  if (lane == 0) {
    const float v = (tg >= 0 && tg < V) ? -((row[tg] - m) - logf(se)) : __builtin_nanf("");
    va_st4(nll + bqt, v);
  }
}

// One workgroup, one wave per codebook (K <= 16): loss_per_cb[q] = mean of nll[:, q, t] over the valid t (t + d_q < n_scored), in a
// fixed order (each lane a fixed stride of (b, t), then the wave's fixed butterfly), so that two calls give the same bits; then thread
// 0 sums the K means in codebook order and divides by K (vaura_model.py:274-279).  Invalid entries — none when every position
// [0, S - 1) was scored — get mask 0, nll NaN and, when logits_out is given, a NaN row (revert_pattern_logits' fill).  With mask_in
// (a caller's (B, K, Ta) mask, _compute_loss) that mask decides, and nothing but loss_per_cb / loss is written.
__global__ __launch_bounds__(1024) void score_reduce_kernel(float* __restrict__ nll, const uint8_t* __restrict__ mask_in,
                                                            uint8_t* __restrict__ mask, float* __restrict__ logits_out,
                                                            int B, int K, int V, int Ta, int n_scored, ScoreDelays pd,
                                                            float* __restrict__ loss_per_cb, float* __restrict__ loss) {
  __shared__ float means[16];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  if (q < K) {
    const int dq = score_delay(pd, q);
    float s = 0.f, cnt = 0.f;
    const float qnan = __builtin_nanf("");
    for (int j = lane; j < B * Ta; j += 64) {
      const int b = j / Ta, t = j % Ta;
      const size_t bqt = ((size_t)b * K + q) * Ta + t;
      const bool ok = mask_in ? mask_in[bqt] != 0 : t + dq < n_scored;
      if (ok) { s += nll[bqt]; cnt += 1.f; }
      else if (!mask_in) va_st4(nll + bqt, qnan);
      if (mask) mask[bqt] = ok ? 1 : 0;
    }
    // rows of invalid entries in the reverted logits: the whole wave fills one row at a time
    if (logits_out && !mask_in && dq + Ta > n_scored) {
      const f32x4 nan4 = {qnan, qnan, qnan, qnan};
      for (int b = 0; b < B; ++b)
        for (int t = n_scored - dq < 0 ? 0 : n_scored - dq; t < Ta; ++t) {
          f32x4* o = reinterpret_cast<f32x4*>(logits_out + (((size_t)b * K + q) * Ta + t) * (size_t)V);
          for (int c = lane; c < V / 4; c += 64) va_st16(o + c, nan4);
        }
    }
    s = wave_sum(s);
    cnt = wave_sum(cnt);
    if (lane == 0) {
      const float mq = s / cnt;                               // 0 / 0 = NaN: a codebook without a valid entry (torch: mean of nothing)
      means[q] = mq;
      va_st4(loss_per_cb + q, mq);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int k = 0; k < K; ++k) tot += means[k];
    va_st4(loss, tot / (float)K);
  }
}

// score_reduce_kernel with per-clip lengths: an entry is valid iff t < Ta_b = clip_T[b] and t + d_q < n_scored — the reference's
// _compute_loss under the mask t < Ta_b.  loss_per_cb[q] is the mean over all valid (b, t) in the same fixed lane-strided order, loss
// the mean of the K means; invalid entries get mask 0, nll NaN and, with logits_out, a NaN row: per clip the suffix from
// min(Ta_b, n_scored - d_q) on, the whole wave filling one row at a time.  No caller's mask here (vaura_score_logits takes any mask
// already).  Ta_b is clamped to 0 .. Ta.
__global__ __launch_bounds__(1024) void score_reduce_clips_kernel(float* __restrict__ nll, uint8_t* __restrict__ mask,
                                                                  float* __restrict__ logits_out, int B, int K, int V, int Ta, int n_scored,
                                                                  ScoreDelays pd, float* __restrict__ loss_per_cb, float* __restrict__ loss,
                                                                  const int32_t* __restrict__ clip_T) {
  __shared__ float means[16];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  if (q < K) {
    const int dq = score_delay(pd, q);
    float s = 0.f, cnt = 0.f;
    const float qnan = __builtin_nanf("");
    for (int j = lane; j < B * Ta; j += 64) {
      const int b = j / Ta, t = j % Ta;
      const size_t bqt = ((size_t)b * K + q) * Ta + t;
      const bool ok = t < clip_T[b] && t + dq < n_scored;
      if (ok) { s += nll[bqt]; cnt += 1.f; }
      else va_st4(nll + bqt, qnan);
      if (mask) mask[bqt] = ok ? 1 : 0;
    }
    // rows of invalid entries in the reverted logits: the whole wave fills one row at a time
    if (logits_out) {
      const f32x4 nan4 = {qnan, qnan, qnan, qnan};
      int lane0 = 0;
      asm volatile("" : "+v"(lane0));
      for (int b = 0; b < B; ++b) {
        const int Tb = __builtin_amdgcn_readfirstlane(clip_T[b + lane0]);
        const int t0 = max(0, min(min(Tb, Ta), n_scored - dq));
        for (int t = t0; t < Ta; ++t) {
          f32x4* o = reinterpret_cast<f32x4*>(logits_out + (((size_t)b * K + q) * Ta + t) * (size_t)V);
          for (int c = lane; c < V / 4; c += 64) va_st16(o + c, nan4);
        }
      }
    }
    s = wave_sum(s);
    cnt = wave_sum(cnt);
    if (lane == 0) {
      const float mq = s / cnt;                               // 0 / 0 = NaN: a codebook without a valid entry (torch: mean of nothing)
      means[q] = mq;
      va_st4(loss_per_cb + q, mq);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int k = 0; k < K; ++k) tot += means[k];
    va_st4(loss, tot / (float)K);
  }
}

static ScoreDelays score_delays(const int32_t* delays_host, int K) {
  ScoreDelays pd;
  for (int j = 0; j < 16; ++j) pd.d[j] = (delays_host && j < K) ? delays_host[j] : j;
  return pd;
}

// one chunk of model-output positions [p0, p0 + n_pos), rows_per_pos rows each (row-major K * V logits per row); clip_T: per-clip
// timesteps (B int32 on the device, checked by the caller) or NULL — every clip has Ta, the kernel every call ran before
int va_launch_score_nll(const float* logits, int rows_per_pos, int p0, int n_pos, int B, int K, int V, int Ta, const int32_t* delays_host,
                        const int32_t* targets, float* nll, float* logits_out, const int32_t* clip_T, hipStream_t s) {
  if (!logits || !targets || !nll || n_pos <= 0 || B <= 0 || K <= 0 || K > 16 || Ta <= 0 || rows_per_pos < B) return VAURA_ERR_ARG;
  if (V % 256 || V > 1024) return VAURA_ERR_SHAPE;
  const ScoreDelays pd = score_delays(delays_host, K);
  const int64_t waves = (int64_t)n_pos * B * K, kv = (int64_t)K * V;
  if (clip_T) {
    VA_LAUNCH(score_nll_clips_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, logits, (int64_t)rows_per_pos * kv, kv, (int64_t)V,
              p0, n_pos, B, K, V, Ta, pd, targets, nll, logits_out, clip_T);
    return 0;
  }
  VA_LAUNCH(score_nll_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, logits, (int64_t)rows_per_pos * kv, kv, (int64_t)V, p0,
            n_pos, B, K, V, Ta, pd, targets, nll, logits_out);
  return 0;
}

int va_launch_score_reduce(float* nll, uint8_t* mask, float* logits_out, int B, int K, int V, int Ta, int n_scored, const int32_t* delays_host,
                           float* loss_per_cb, float* loss, const int32_t* clip_T, hipStream_t s) {
  if (!nll || !loss_per_cb || !loss || B <= 0 || K <= 0 || K > 16 || Ta <= 0 || V % 4) return VAURA_ERR_ARG;
  const ScoreDelays pd = score_delays(delays_host, K);
  if (clip_T) {
    VA_LAUNCH(score_reduce_clips_kernel, dim3(1), dim3(64 * K), 0, s, nll, mask, logits_out, B, K, V, Ta, n_scored, pd, loss_per_cb, loss, clip_T);
    return 0;
  }
  VA_LAUNCH(score_reduce_kernel, dim3(1), dim3(64 * K), 0, s, nll, (const uint8_t*)nullptr, mask, logits_out, B, K, V, Ta, n_scored, pd,
            loss_per_cb, loss);
  return 0;
}

extern "C" {

int vaura_score_logits(const float* logits, const int32_t* targets, const uint8_t* mask, int B, int K, int V, int Ta, float* nll,
                       float* loss_per_cb, float* loss, vaura_stream_t s) {
  if (!logits || !targets || !mask || !nll || !loss_per_cb || !loss || B <= 0 || K <= 0 || K > 16 || Ta <= 0) return VAURA_ERR_ARG;
  if (V % 256 || V > 1024) return VAURA_ERR_SHAPE;
  hipStream_t st = as_stream(s);
  ScoreDelays z;
  for (int j = 0; j < 16; ++j) z.d[j] = 0;
  // the reverted tensor as Ta one-row "positions" of zero delay: position t of row b, codebook q at ((b * K + q) * Ta + t) * V
  const int64_t waves = (int64_t)Ta * B * K;
  VA_LAUNCH(score_nll_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, logits, (int64_t)V, (int64_t)K * Ta * V, (int64_t)Ta * V,
            0, Ta, B, K, V, Ta, z, targets, nll, (float*)nullptr);
  VA_LAUNCH(score_reduce_kernel, dim3(1), dim3(64 * K), 0, st, nll, mask, (uint8_t*)nullptr, (float*)nullptr, B, K, V, Ta, Ta, z,
            loss_per_cb, loss);
  return 0;
}

}  // extern "C"
