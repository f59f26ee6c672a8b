// Clips and windows of clips in one codec pass (dac.hip only): the layouts of the packed sequence, the kernels that pack, unpack and clear
// its gaps, and the host arithmetic that plans it (gaps, offsets, the decoder's halo, windows).
#pragma once
#include "common.h"
#include <algorithm>
#include <vector>

// ---------------------------------------------------------------------------------------------
// Clips of different lengths in ONE pass (vaura_dac_decode_clips / vaura_dac_encode_clips).  The B clips lie behind one another
// on the time axis of a single sequence (B = 1 for every conv launch), `gap` latent frames of zeros between neighbours: clip b
// starts at latent row off[b], at row off[b] * rate on a level with `rate` rows per latent frame, at sample off[b] * hop.  No conv
// kernel knows about it.  A tap of a row of clip b lands inside the clip, in a gap — zeros, what the `jr >= 0 && jr < Lin` mask
// gives the clip decoded alone — or past an end of the sequence, where that mask applies.  Residual and raw rows are read at their own
// position only, a 1 x 1 conv is pointwise, and a transposed conv writes a row from one (j, phase).  A launch writes gap rows like
// any other (from the neighbours' edges), so the gap rows of every ACTIVATED buffer that a conv with more than one tap reads are
// cleared again behind the launch that wrote it (clips_zero_gaps_kernel).  The gap is the smallest number of latent frames that, on
// every level, covers the largest one-sided reach of the convs that run there (va_clips_gap_*).
#define VA_CLIP_CHUNK 64
struct ClipChunk {                    // up to VA_CLIP_CHUNK clips by value: a launch per chunk, no table on the device
  int n, b0;                          // clips in this chunk, index of the first
  int off[VA_CLIP_CHUNK];             // first latent row of the clip in the packed sequence
  int len[VA_CLIP_CHUNK];             // its latent frames
  int64_t aux[VA_CLIP_CHUNK];         // its samples (encode)
};
struct WindowLayout;
struct ClipLayout {
  int B, gap;
  int64_t total;                      // latent rows of the packed sequence: off[B - 1] + len[B - 1]
  const int* off;
  const int* len;
  const int64_t* aux;
  const WindowLayout* win = nullptr;  // vaura_dac_decode_window: the packed clips are windows of the caller's clips (see WindowLayout)
};
static ClipChunk va_clip_chunk(const ClipLayout& l, int b0, int bend) {
  ClipChunk k;
  k.b0 = b0; k.n = bend - b0 < VA_CLIP_CHUNK ? bend - b0 : VA_CLIP_CHUNK;
  for (int i = 0; i < k.n; ++i) { k.off[i] = l.off[b0 + i]; k.len[i] = l.len[b0 + i]; k.aux[i] = l.aux ? l.aux[b0 + i] : 0; }
  return k;
}

// the `gap` frames behind each clip of the chunk: unit = bytes of one latent frame of this buffer (rows per frame x bytes per row, a
// multiple of 16).  0 is all-zero bytes in fp32, in both fp16 planes and in e4m3; an mx8 buffer keeps the scale bytes its producer wrote
// (1 .. 253, mx8_scale_byte): 0 x 2^s is 0.
__global__ __launch_bounds__(256) void clips_zero_gaps_kernel(unsigned char* __restrict__ buf, ClipChunk k, size_t unit, int gap) {
  const int i = blockIdx.y;
  u32x4* p = reinterpret_cast<u32x4*>(buf + (size_t)(k.off[i] + k.len[i]) * unit);
  const size_t n16 = (size_t)gap * unit / 16;
  for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < n16; u += (size_t)gridDim.x * 256) p[u] = u32x4{0u, 0u, 0u, 0u};
}
// codes (B, K, Tmax) -> packed (K, total): a clip's own frames, code 0 on the `tail` frames behind it (the gap; 0 behind the last clip)
__global__ __launch_bounds__(256) void clips_pack_codes_kernel(const int32_t* __restrict__ codes, int32_t* __restrict__ packed, ClipChunk k,
                                                               int K, int Tmax, int64_t total, int gap, int B) {
  const int i = blockIdx.y, kk = blockIdx.z, b = k.b0 + i;
  const int n = k.len[i] + (b + 1 < B ? gap : 0);
  for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256)
    packed[(size_t)kk * total + k.off[i] + t] = t < k.len[i] ? codes[((size_t)b * K + kk) * Tmax + t] : 0;
}
// packed (K, total) -> codes (B, K, Tmax): 0 behind a clip's frames
__global__ __launch_bounds__(256) void clips_unpack_codes_kernel(const int32_t* __restrict__ packed, int32_t* __restrict__ codes, ClipChunk k,
                                                                 int K, int Tmax, int64_t total) {
  const int i = blockIdx.y, kk = blockIdx.z, b = k.b0 + i;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < Tmax; t += gridDim.x * 256)
    codes[((size_t)b * K + kk) * Tmax + t] = t < k.len[i] ? packed[(size_t)kk * total + k.off[i] + t] : 0;
}
// wav (B, n_max) -> packed samples: aux[i] samples of the clip, zeros up to the end of its last frame (DAC.preprocess) and through the gap
__global__ __launch_bounds__(256) void clips_pack_wav_kernel(const float* __restrict__ wav, float* __restrict__ packed, ClipChunk k,
                                                             int64_t n_max, int hop, int gap, int B) {
  const int i = blockIdx.y, b = k.b0 + i;
  const int64_t n = (int64_t)(k.len[i] + (b + 1 < B ? gap : 0)) * hop;
  float* dst = packed + (size_t)k.off[i] * hop;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < n; u += (int64_t)gridDim.x * 256)
    dst[u] = u < k.aux[i] ? wav[(size_t)b * n_max + u] : 0.f;
}
// packed samples -> wav (B, n_out): len[i] * hop samples of the clip, 0 behind them
__global__ __launch_bounds__(256) void clips_unpack_wav_kernel(const float* __restrict__ packed, float* __restrict__ wav, ClipChunk k,
                                                               int64_t n_out, int hop) {
  const int i = blockIdx.y, b = k.b0 + i;
  const int64_t n = (int64_t)k.len[i] * hop;
  const float* src = packed + (size_t)k.off[i] * hop;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < n_out; u += (int64_t)gridDim.x * 256)
    wav[(size_t)b * n_out + u] = u < n ? src[u] : 0.f;
}

// A window of every clip in ONE pass (vaura_dac_decode_window).  The decoder is a finite-support conv stack: the samples of latent
// frame f depend on the codes of frames f - H .. f + H only (H = va_decode_halo, from the conv descriptors).  So the frames
// [lo, hi) = [max(0, s - H), min(len, s + n + H)) of a clip, decoded as a clip of their own, give the samples of [s, s + n) exactly:
// a frame at least H from a cut end sees what it sees in the whole clip, and an end that is the clip's own (lo = 0, hi = len) has the
// zero padding the whole clip has there.  The windows are the clips of a ClipLayout (a clip with count 0 has none): packing reads
// from frame lo of the caller's tensor, unpacking skips the (s - lo) * hop samples in front.
struct WindowChunk {                  // up to VA_CLIP_CHUNK entries by value
  int n;
  int b[VA_CLIP_CHUNK];               // the caller's clip
  int off[VA_CLIP_CHUNK];             // pack: first latent row of the window in the packed sequence; unpack: of the frames asked for
  int len[VA_CLIP_CHUNK];             // pack: latent frames of the window (the gap behind it included); unpack: the frames asked for
  int src[VA_CLIP_CHUNK];             // pack: first frame of the window in the clip
  int aux[VA_CLIP_CHUNK];             // pack: the window's own frames (len without the gap)
};
struct WindowLayout {
  int B, n_max;                       // the caller's clips, the width of its output in frames
  const int* clip;                    // per window: the caller's clip
  const int* lo;                      // per window: its first frame in the clip
  const int* skip;                    // per window: halo frames in front of the frames asked for
  const int* window;                  // per caller's clip (B): index of its window, -1 for count 0
  const int* count;                   // per caller's clip (B)
  // vaura_dac_decode_window_seq: the caller's tensor is the decode loop's pattern sequence (B, seq_K, seq_S), not codes (seq_S = 0)
  int seq_K = 0, seq_S = 0;
  int seq_delays[16] = {0};
};
// codes (B, K, Tmax) -> packed (K, total): the window's frames from frame src[i] of clip b[i] on, code 0 on the gap frames behind it
__global__ __launch_bounds__(256) void window_pack_codes_kernel(const int32_t* __restrict__ codes, int32_t* __restrict__ packed, WindowChunk k,
                                                                int K, int Tmax, int64_t total) {
  const int i = blockIdx.y, kk = blockIdx.z;
  const int32_t* src = codes + ((size_t)k.b[i] * K + kk) * Tmax + k.src[i];
  for (int t = blockIdx.x * 256 + threadIdx.x; t < k.len[i]; t += gridDim.x * 256)
    packed[(size_t)kk * total + k.off[i] + t] = t < k.aux[i] ? src[t] : 0;
}
// The same pack from the decode loop's pattern sequence (vaura_dac_decode_window_seq): seq (B, K, S) holds frame t of codebook q at step
// t + 1 + d_q (vaura_pattern_build_delays), so the window's frames are gathered from there and no reverted tensor exists.  A value that
// is no code (an unknown slot, the special token: the host's checks keep every window off them) is packed as code 0, never used as an index.
struct SeqDelays { int d[16]; };
__global__ __launch_bounds__(256) void window_pack_seq_kernel(const int32_t* __restrict__ seq, int32_t* __restrict__ packed, WindowChunk k,
                                                              SeqDelays dl, int K, int S, int64_t total, int card) {
  const int i = blockIdx.y, kk = blockIdx.z;
  const int32_t* src = seq + ((size_t)k.b[i] * K + kk) * S + k.src[i] + 1 + dl.d[kk];
  for (int t = blockIdx.x * 256 + threadIdx.x; t < k.len[i]; t += gridDim.x * 256) {
    const int32_t v = t < k.aux[i] ? src[t] : 0;
    packed[(size_t)kk * total + k.off[i] + t] = (uint32_t)v < (uint32_t)card ? v : 0;
  }
}
// packed samples -> wav (B, n_out): the len[i] * hop samples from packed frame off[i] on, 0 behind them (len 0: a row of zeros, nothing read)
__global__ __launch_bounds__(256) void window_unpack_wav_kernel(const float* __restrict__ packed, float* __restrict__ wav, WindowChunk k,
                                                                int64_t n_out, int hop) {
  const int i = blockIdx.y, b = k.b[i];
  const int64_t n = (int64_t)k.len[i] * hop;
  const float* src = packed + (size_t)k.off[i] * hop;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < n_out; u += (int64_t)gridDim.x * 256)
    wav[(size_t)b * n_out + u] = u < n ? src[u] : 0.f;
}
// windows w0 .. of the layout: what window_pack_codes_kernel reads and where it writes
static WindowChunk va_window_pack_chunk(const ClipLayout& l, int w0) {
  WindowChunk k;
  k.n = l.B - w0 < VA_CLIP_CHUNK ? l.B - w0 : VA_CLIP_CHUNK;
  for (int i = 0; i < k.n; ++i) {
    const int w = w0 + i;
    k.b[i] = l.win->clip[w]; k.off[i] = l.off[w]; k.src[i] = l.win->lo[w]; k.aux[i] = l.len[w];
    k.len[i] = l.len[w] + (w + 1 < l.B ? l.gap : 0);
  }
  return k;
}
// the caller's clips b0 .. : where window_unpack_wav_kernel finds the frames asked for (a clip with count 0 has no window: len 0)
static WindowChunk va_window_unpack_chunk(const ClipLayout& l, int b0) {
  WindowChunk k;
  k.n = l.win->B - b0 < VA_CLIP_CHUNK ? l.win->B - b0 : VA_CLIP_CHUNK;
  for (int i = 0; i < k.n; ++i) {
    const int b = b0 + i, w = l.win->window[b];
    k.b[i] = b; k.len[i] = l.win->count[b]; k.off[i] = w < 0 ? 0 : l.off[w] + l.win->skip[w]; k.src[i] = k.aux[i] = 0;
  }
  return k;
}

static inline int va_ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int va_conv_reach(const vaura_conv& cv) { return cv.stride > 1 ? 1 : ((cv.taps - 1) / 2) * cv.dilation; }
// smallest gap (latent frames) with gap * rate(level) >= the one-sided reach of every conv on that level; -1: not a geometry of the pass
static int va_clips_gap_decode(const vaura_codec* c) {
  if (c->n_blocks < 1 || c->n_blocks > 4 || c->n_units != 3) return -1;
  int g = va_conv_reach(c->conv_in), rate = 1;
  for (int b = 0; b < c->n_blocks; ++b) {
    if (c->rates[b] < 1) return -1;
    g = std::max(g, va_ceil_div(va_conv_reach(c->up[b]), rate));     // reads rows j, j - 1 of its input level
    rate *= c->rates[b];
    for (int u = 0; u < 3; ++u)
      for (int i = 0; i < 2; ++i) g = std::max(g, va_ceil_div(va_conv_reach(c->res[b][u][i]), rate));
  }
  g = std::max(g, va_ceil_div(va_conv_reach(c->conv_out), rate));
  return g < 1 ? 1 : g;
}
static int va_clips_gap_encode(const vaura_codec_encoder* c, int64_t* hop_out) {
  if (c->n_blocks < 1 || c->n_blocks > 4 || c->n_units != 3) return -1;
  int64_t hop = 1;
  for (int b = 0; b < c->n_blocks; ++b) { if (c->rates[b] < 1) return -1; hop *= c->rates[b]; }
  if (hop_out) *hop_out = hop;
  int rate = (int)hop;
  int g = va_ceil_div(3, rate);                                  // the first conv: k = 7 on the samples
  for (int b = 0; b < c->n_blocks; ++b) {
    for (int u = 0; u < 3; ++u)
      for (int i = 0; i < 2; ++i) g = std::max(g, va_ceil_div(va_conv_reach(c->res[b][u][i]), rate));
    rate /= c->rates[b];
    g = std::max(g, va_ceil_div(va_conv_reach(c->down[b]), rate));   // 3 taps over rows of r * C channels = rows of its OUTPUT level
  }
  g = std::max(g, va_ceil_div(va_conv_reach(c->conv_out), rate));
  return g < 1 ? 1 : g;
}
// offsets of `B` clips of `frames[b]` latent frames; false when the packed sequence leaves the int range of the launch arithmetic
static bool va_clips_offsets(const int* frames, int B, int gap, int* off, int64_t* total) {
  int64_t o = 0;
  for (int b = 0; b < B; ++b) {
    if (o > 0x7fffffff) return false;
    off[b] = (int)o;
    o += frames[b] + (b + 1 < B ? gap : 0);
  }
  *total = o;
  return o <= 0x7fffffff;
}

static inline int64_t va_floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
// Frames of context either side that the samples of one latent frame depend on: the rows [0, hop) of the last level, taken backwards
// through the layers.  A k-tap conv of dilation d widens the interval by (k - 1) / 2 * d rows either side; a transposed conv (stride
// r, k = 2r, pad ceil(r / 2)) writes row o from the input rows j with o = j * r - pad + t, 0 <= t < k, so [lo, hi] comes from
// [ceil((lo + pad - k + 1) / r), floor((hi + pad) / r)].  At the latent level the frame itself is row 0.  -1: not such a geometry.
static int va_decode_halo(const vaura_codec* c) {
  if (va_clips_gap_decode(c) < 0) return -1;
  auto plain = [](const vaura_conv& cv) { return cv.stride == 1 && cv.taps >= 1 && (cv.taps & 1) && cv.dilation >= 1; };
  if (!plain(c->conv_in) || !plain(c->conv_out)) return -1;
  int64_t hop = 1;
  for (int b = 0; b < c->n_blocks; ++b) {
    if (c->up[b].stride != c->rates[b] || c->up[b].taps != 2 || hop > 0x7fffffff / c->rates[b]) return -1;
    hop *= c->rates[b];
    for (int u = 0; u < 3; ++u)
      for (int i = 0; i < 2; ++i) if (!plain(c->res[b][u][i])) return -1;
  }
  int64_t lo = -va_conv_reach(c->conv_out), hi = hop - 1 + va_conv_reach(c->conv_out);
  for (int b = c->n_blocks - 1; b >= 0; --b) {
    for (int u = 0; u < 3; ++u)
      for (int i = 0; i < 2; ++i) { lo -= va_conv_reach(c->res[b][u][i]); hi += va_conv_reach(c->res[b][u][i]); }
    const int64_t r = c->rates[b], pad = (r + 1) / 2, k = 2 * r;
    lo = -va_floor_div(-(lo + pad - k + 1), r);
    hi = va_floor_div(hi + pad, r);
  }
  lo -= va_conv_reach(c->conv_in); hi += va_conv_reach(c->conv_in);
  const int64_t h = std::max(-lo, hi);
  return h < 0 || h > 0x3fffffff ? -1 : (int)h;
}

// the windows of a decode_window call on the host: one per clip with count > 0
struct WindowPlan {
  std::vector<int> clip, lo, skip, len, off, window, count;
  int64_t total = 0;                  // latent rows of the packed windows; 0: refused arguments, -1: beyond the int range
  int gap = 0;
};
// T_max <= 0: lengths are checked against >= 1 only; lengths NULL: every clip has T_max frames (T_max <= 0: no end to clamp at, an
// upper bound of the window).  n_max <= 0: counts are not checked against it.
static WindowPlan va_window_plan(const vaura_codec* c, int B, int T_max, const int32_t* lengths, const int32_t* starts, const int32_t* counts,
                                 int n_max) {
  WindowPlan p;
  const int H = va_decode_halo(c);
  p.gap = va_clips_gap_decode(c);
  if (H < 0 || p.gap < 0) return p;
  p.window.assign((size_t)B, -1);
  p.count.assign(counts, counts + B);
  for (int b = 0; b < B; ++b) {
    const int64_t len = lengths ? lengths[b] : (T_max > 0 ? T_max : 0x7fffffff);
    const int64_t s = starts[b], n = counts[b];
    if (len < 1 || (T_max > 0 && len > T_max) || s < 0 || n < 0 || s + n > len || (n_max > 0 && n > n_max)) { p.clip.clear(); return p; }
    if (n == 0) continue;
    const int64_t lo = std::max<int64_t>(0, s - H), hi = std::min(len, s + n + H);
    p.window[(size_t)b] = (int)p.clip.size();
    p.clip.push_back(b); p.lo.push_back((int)lo); p.skip.push_back((int)(s - lo)); p.len.push_back((int)(hi - lo));
  }
  if (p.clip.empty()) return p;                        // every count is 0
  p.off.resize(p.clip.size());
  if (!va_clips_offsets(p.len.data(), (int)p.clip.size(), p.gap, p.off.data(), &p.total)) p.total = -1;
  return p;
}

// the pattern sequence of a window_seq call: K rows of S steps under `delays_host` (NULL: 0 .. K - 1) hold T = S - 1 - max(d) frames
struct SeqSource { int K, S, d_max; int delays[16]; };
static bool va_seq_source(const vaura_codec* c, int K, int S, const int32_t* delays_host, SeqSource* out) {
  if (!c || K < c->n_codebooks || K < 1 || K > 16 || S < 2) return false;
  out->K = K; out->S = S; out->d_max = 0;
  for (int q = 0; q < 16; ++q) {
    const int d = q < K ? (delays_host ? delays_host[q] : q) : 0;
    if (d < 0 || d > S - 2) return false;
    out->delays[q] = d;
    out->d_max = std::max(out->d_max, d);
  }
  return true;
}

