// Video preprocessing: decoded uint8 frames -> the feature extractor's input, in one launch.
//   torchvision.transforms.v2.Resize(256, antialias=True) -> CenterCrop([224, 224]) -> ToFloat32DType -> Normalize(0.5, 0.5)
//                                                       configs/generate_vgg.yaml:53-65
//   GenerateMultipleSegments(16) + permute               models/data/transforms/video_transforms.py:114-240, vggsound_dataset.py:273-275
// The resize is torch's separable antialiased triangle filter on uint8 (horizontal pass, rounded to uint8, then vertical pass, rounded
// to uint8), in its fixed-point form: int16 taps scaled by 2^prec, acc = 2^(prec-1) + sum(tap * pixel), clamp(acc >> prec, 0, 255).
// The taps, their start indices and both precisions are built on the host (vaura_amd/preprocess.py: tap_table) once per geometry;
// the kernel does no filter geometry.  Only what survives the crop is computed: the crop_w kept columns of the source rows that the
// kept output rows need.
//
// One kernel, both passes; the horizontally filtered rows of a tile live in LDS as uint8 and never touch memory.
//   grid  (ceil(crop_h / tile_rows), B * S * F): one workgroup per (tile of output rows, output frame), all three channels
//   phase 1 (per wave, one source row of one channel [NCHW] or of all three [NHWC] at a time): the row's needed byte range
//           [x0, x0 + span) is copied to the wave's LDS slab with aligned 4-byte loads (4 pixels per lane; the aligned words that
//           hold the first and last byte lie in the same pages as those bytes), then each lane filters 4 adjacent kept columns from
//           the slab and writes them as one 4-byte word of the tile
//   phase 2: each thread filters 4 adjacent columns of one output row vertically (one 4-byte LDS word per tap), maps the four uint8
//           levels through the 256-entry table lut[c][level] = ((level / 255) - mean[c]) / std[c] (built by the host in fp32, so the
//           device result is the host's to the bit) and stores 16 bytes.
// Bytes per 360 x 640 -> 224 x 224 frame: read 3 x 318 of 360 rows x 319 of 640 columns = 0.30 MB (+ the rows adjacent tiles share,
// which come from L2), write 3 x 224 x 224 x 4 = 0.60 MB.
//
// video_preprocess_yuv_kernel takes what a decoder hands over instead: 8-bit 4:2:0 surfaces (NV12: luma, then interleaved Cb,Cr rows at
// the same pitch; I420: luma, then the U and the V plane at half the pitch), 1.5 bytes per pixel.  Same grid, same phase 2; phase 1
// copies the needed bytes of one luma row and of its chroma row to the wave's slab, converts them ONCE to three planar uint8 rows in
// LDS (the host's integer formula: 2^14-scaled coefficients, chroma replicated over its 2 x 2 block, no interpolation) and filters
// each of the three as the NCHW instance filters a row.  yuv -> RGB uint8 -> the resize above: the same function as converting on the
// host first (vaura_amd/preprocess.py: yuv420_to_rgb_u8) and calling the RGB kernel.
//
// video_preprocess_frames_kernel / video_preprocess_yuv_frames_kernel are the same launches for video that is not at the model's 25
// frames per second (the reference re-encoded offline: scripts/reencode_videos.py:71, ffmpeg -vf fps=25): the source frame of every
// output frame comes from a device table the host builds (vaura_amd/preprocess.py: fps_plan, frames dropped and repeated as ffmpeg's
// fps filter does), so selecting frames costs no pass over the video.  See the comment in front of them.
#include "common.h"

#define PREPROC_MAX_TAPS VAURA_PREPROC_MAX_TAPS
#define PREPROC_WAVES 4
#define PREPROC_LDS_LIMIT (64 * 1024)

struct PreprocArgs {
  const uint8_t* src;
  const int32_t* h_rel;   // (crop_w) first tap of kept column x, relative to x0
  const int16_t* h_w;     // (crop_w, h_taps)
  const int32_t* v_start; // (crop_h) first source row of kept output row r
  const int16_t* v_w;     // (crop_h, v_taps)
  const float* lut;       // (3, 256)
  float* out;             // (B, S, 3, F, crop_h, crop_w)
  int T, H, W, S, F, seg_start, seg_stride;
  int crop_h, crop_w, h_taps, h_prec, v_taps, v_prec, x0, span, tile_rows, tile_src_rows, slab_dwords;
};

// acc >> prec as a uint8 level.  The taps are non-negative (the host builds triangle-filter taps only), so the accumulator never is
// negative and the clamp is the upper one alone, taken unsigned.  Written this way on purpose: from the signed form
// clamp(acc >> prec, 0, 255) of two neighbours hipcc 7.2 selects v_ashr_pk_u8_i32 for gfx950 and ORs the third byte into a
// register whose bits 16..23 still hold the first accumulator (seen on the device: every third column of a group of four wrong).
__device__ __forceinline__ uint32_t level_u8(int acc, int prec) {
  const uint32_t v = (uint32_t)acc >> prec;
  return v > 255u ? 255u : v;
}

// dynamic LDS of one workgroup: table (768 floats), first taps, horizontal taps, one row slab per wave, the tile
static size_t preproc_lds_bytes(int channels_last, int crop_w, int h_taps, int span, int tile_src_rows) {
  const size_t slab = (size_t)(((channels_last ? 3 : 1) * span + 3 + 3) >> 2);
  return 4 * ((size_t)768 + crop_w + (((size_t)crop_w * h_taps) >> 1) + (size_t)PREPROC_WAVES * slab + (size_t)3 * tile_src_rows * (crop_w >> 2));
}

template <bool NHWC>
__global__ __launch_bounds__(64 * PREPROC_WAVES) void video_preprocess_kernel(const PreprocArgs a) {
  extern __shared__ uint32_t smem[];
  const int nq = a.crop_w >> 2;                                       // 4-column groups per kept row
  float* lut = reinterpret_cast<float*>(smem);                         // 768 floats
  int32_t* hrel = reinterpret_cast<int32_t*>(smem + 768);              // crop_w
  int16_t* hw = reinterpret_cast<int16_t*>(smem + 768 + a.crop_w);     // crop_w * h_taps (an even count: crop_w % 4 == 0)
  uint32_t* slabs = smem + 768 + a.crop_w + ((a.crop_w * a.h_taps) >> 1);
  uint32_t* tile = slabs + PREPROC_WAVES * a.slab_dwords;              // [3][tile_src_rows][nq] words of 4 uint8
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  const int of = blockIdx.y;                                           // output frame (b, s, f)
  const int f = of % a.F, bs = of / a.F, s = bs % a.S, b = bs / a.S;
  const size_t n = (size_t)b * a.T + a.seg_start + s * a.seg_stride + f;   // source frame
  const int r0 = blockIdx.x * a.tile_rows;
  const int nr = min(a.tile_rows, a.crop_h - r0);
  // source rows [ylo, ylo + nrows): clamped so that no table content can index outside the frame or the tile
  const int ylo = min(max(a.v_start[r0], 0), a.H - a.v_taps);
  const int nrows = min(a.tile_src_rows, a.H - ylo);

  for (int i = tid; i < 768; i += 64 * PREPROC_WAVES) lut[i] = a.lut[i];
  for (int i = tid; i < a.crop_w; i += 64 * PREPROC_WAVES) hrel[i] = min(max(a.h_rel[i], 0), a.span - a.h_taps);
  for (int i = tid; i < a.crop_w * a.h_taps; i += 64 * PREPROC_WAVES) hw[i] = a.h_w[i];
  __syncthreads();

  // ---- phase 1: horizontal pass into the tile
  uint32_t* slab = slabs + wave * a.slab_dwords;
  const int jobs = NHWC ? nrows : 3 * nrows;
  const int hhalf = 1 << (a.h_prec - 1);
  for (int j0 = 0; j0 < jobs; j0 += PREPROC_WAVES) {
    const int j = j0 + wave;                                           // wave-uniform
    const int yy = NHWC ? j : j / 3, cj = NHWC ? 0 : j - 3 * yy;
    int shift = 0;
    if (j < jobs) {
      const size_t row = NHWC ? ((n * a.H + (ylo + yy)) * a.W + a.x0) * 3 : ((n * 3 + cj) * a.H + (ylo + yy)) * a.W + a.x0;
      const uintptr_t p = reinterpret_cast<uintptr_t>(a.src) + row;
      shift = (int)(p & 3);
      const uint32_t* pa = reinterpret_cast<const uint32_t*>(p - shift);
      const int ndw = (shift + (NHWC ? 3 : 1) * a.span + 3) >> 2;       // <= slab_dwords
      for (int i = lane; i < ndw; i += 64) slab[i] = pa[i];
    }
    __syncthreads();
    if (j < jobs) {
      const uint8_t* sb = reinterpret_cast<const uint8_t*>(slab) + shift;
#pragma unroll 1
      for (int c = NHWC ? 0 : cj; c < (NHWC ? 3 : cj + 1); ++c) {
        for (int q = lane; q < nq; q += 64) {
          uint32_t word = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int x = 4 * q + e;
            const uint8_t* t = NHWC ? sb + 3 * hrel[x] + c : sb + hrel[x];
            const int16_t* w = hw + x * a.h_taps;
            int acc = hhalf;
            for (int k = 0; k < a.h_taps; ++k) acc += (int)t[NHWC ? 3 * k : k] * (int)w[k];
            word |= level_u8(acc, a.h_prec) << (8 * e);
          }
          tile[((size_t)c * a.tile_src_rows + yy) * nq + q] = word;
        }
      }
    }
    __syncthreads();
  }

  // ---- phase 2: vertical pass, level -> fp32 table, 16-byte stores
  const int vhalf = 1 << (a.v_prec - 1);
  const int items = 3 * nr * nq;
  for (int it = tid; it < items; it += 64 * PREPROC_WAVES) {
    const int q = it % nq, rc = it / nq, rr = rc % nr, c = rc / nr;
    const int r = r0 + rr;
    const int ys = min(max(a.v_start[r] - ylo, 0), nrows - a.v_taps);
    const int16_t* w = a.v_w + (size_t)r * a.v_taps;
    const uint32_t* t = tile + ((size_t)c * a.tile_src_rows + ys) * nq + q;
    int a0 = vhalf, a1 = vhalf, a2 = vhalf, a3 = vhalf;
    for (int k = 0; k < a.v_taps; ++k) {
      const uint32_t d = t[(size_t)k * nq];
      const int wk = w[k];
      a0 += (int)(d & 255u) * wk;
      a1 += (int)((d >> 8) & 255u) * wk;
      a2 += (int)((d >> 16) & 255u) * wk;
      a3 += (int)(d >> 24) * wk;
    }
    const float* l = lut + 256 * c;
    const f32x4 o = {l[level_u8(a0, a.v_prec)], l[level_u8(a1, a.v_prec)], l[level_u8(a2, a.v_prec)], l[level_u8(a3, a.v_prec)]};
    float* dst = a.out + ((((size_t)bs * 3 + c) * a.F + f) * a.crop_h + r) * a.crop_w + 4 * q;
    *reinterpret_cast<f32x4*>(dst) = o;
  }
}

struct PreprocYuvArgs {
  const uint8_t* src;
  const int32_t* h_rel;
  const int16_t* h_w;
  const int32_t* v_start;
  const int16_t* v_w;
  const float* lut;
  float* out;
  int64_t pitch, chroma_offset, frame_stride;   // bytes: luma row to row, frame start to chroma plane, frame to frame
  int y_off, cy, crv, cgu, cgv, cbu;            // the host's colour formula, coefficients scaled by 2^14
  int T, H, W, S, F, seg_start, seg_stride;
  int crop_h, crop_w, h_taps, h_prec, v_taps, v_prec, x0, span, tile_rows, tile_src_rows, slab_dwords;
};

#define PREPROC_YUV_PREC 14

// one wave's slab: the luma bytes, the chroma bytes (NV12: one run of pairs; I420: the U run, then the V run), three planar RGB rows.
// Each raw run starts at an aligned word, so it holds up to 3 bytes in front of its first needed byte and ends on a whole word.
__host__ __device__ static inline int yuv_luma_dwords(int span) { return (span + 3 + 3) >> 2; }
__host__ __device__ static inline int yuv_plane_dwords(int span) { return ((span >> 1) + 1 + 3 + 3) >> 2; }    // I420: span / 2 + 1 samples at most
__host__ __device__ static inline int yuv_chroma_dwords(int span) { return (span + 16) >> 2; }                  // >= span + 2 + 3 bytes (NV12), >= 2 planes (I420)
__host__ __device__ static inline int yuv_rgb_dwords(int span) { return (span + 3) >> 2; }
__host__ __device__ static inline int yuv_slab_dwords(int span) { return yuv_luma_dwords(span) + yuv_chroma_dwords(span) + 3 * yuv_rgb_dwords(span); }

static size_t preproc_yuv_lds_bytes(int crop_w, int h_taps, int span, int tile_src_rows) {
  return 4 * ((size_t)768 + crop_w + (((size_t)crop_w * h_taps) >> 1) + (size_t)PREPROC_WAVES * yuv_slab_dwords(span) + (size_t)3 * tile_src_rows * (crop_w >> 2));
}

// The colour accumulators ARE negative for out-of-gamut input, so the lower clamp comes first and level_u8 (unsigned, see its comment)
// takes the upper one.
__device__ __forceinline__ uint32_t color_u8(int acc) { return level_u8(max(acc, 0), PREPROC_YUV_PREC); }

// copy `nbytes` bytes that start at `p` into `dst` with aligned 4-byte loads; returns where the first byte sits in dst (0..3)
__device__ __forceinline__ int stage_bytes(uint32_t* dst, const uint8_t* p, int nbytes, int lane) {
  const uintptr_t u = reinterpret_cast<uintptr_t>(p);
  const int shift = (int)(u & 3);
  const uint32_t* pa = reinterpret_cast<const uint32_t*>(u - shift);
  const int ndw = (shift + nbytes + 3) >> 2;
  for (int i = lane; i < ndw; i += 64) dst[i] = pa[i];
  return shift;
}

template <int LAYOUT>   // VAURA_YUV_NV12 / VAURA_YUV_I420
__global__ __launch_bounds__(64 * PREPROC_WAVES) void video_preprocess_yuv_kernel(const PreprocYuvArgs a) {
  extern __shared__ uint32_t smem[];
  const int nq = a.crop_w >> 2;                                       // 4-column groups per kept row
  float* lut = reinterpret_cast<float*>(smem);                         // 768 floats
  int32_t* hrel = reinterpret_cast<int32_t*>(smem + 768);              // crop_w
  int16_t* hw = reinterpret_cast<int16_t*>(smem + 768 + a.crop_w);     // crop_w * h_taps (an even count: crop_w % 4 == 0)
  uint32_t* slabs = smem + 768 + a.crop_w + ((a.crop_w * a.h_taps) >> 1);
  uint32_t* tile = slabs + PREPROC_WAVES * a.slab_dwords;              // [3][tile_src_rows][nq] words of 4 uint8
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  const int of = blockIdx.y;                                           // output frame (b, s, f)
  const int f = of % a.F, bs = of / a.F, s = bs % a.S, b = bs / a.S;
  const size_t n = (size_t)b * a.T + a.seg_start + s * a.seg_stride + f;   // source frame
  const int r0 = blockIdx.x * a.tile_rows;
  const int nr = min(a.tile_rows, a.crop_h - r0);
  // source rows [ylo, ylo + nrows): clamped so that no table content can index outside the frame or the tile
  const int ylo = min(max(a.v_start[r0], 0), a.H - a.v_taps);
  const int nrows = min(a.tile_src_rows, a.H - ylo);

  for (int i = tid; i < 768; i += 64 * PREPROC_WAVES) lut[i] = a.lut[i];
  for (int i = tid; i < a.crop_w; i += 64 * PREPROC_WAVES) hrel[i] = min(max(a.h_rel[i], 0), a.span - a.h_taps);
  for (int i = tid; i < a.crop_w * a.h_taps; i += 64 * PREPROC_WAVES) hw[i] = a.h_w[i];
  __syncthreads();

  // ---- phase 1: one source row per wave: stage luma + chroma, convert once, horizontal pass of the three channels into the tile
  uint32_t* luma = slabs + wave * a.slab_dwords;
  uint32_t* chroma = luma + yuv_luma_dwords(a.span);
  uint32_t* rgb = chroma + yuv_chroma_dwords(a.span);
  const int rgbw = yuv_rgb_dwords(a.span);
  const int c0 = a.x0 >> 1;                                            // first chroma sample of the span
  const int nc = ((a.x0 + a.span - 1) >> 1) - c0 + 1;                  // chroma samples the span touches (<= span / 2 + 1)
  const uint8_t* frame = a.src + n * (size_t)a.frame_stride;
  const int hhalf = 1 << (a.h_prec - 1);
  for (int j0 = 0; j0 < nrows; j0 += PREPROC_WAVES) {
    const int yy = j0 + wave;                                          // wave-uniform
    int ysh = 0, ush = 0, vsh = 0;
    if (yy < nrows) {
      const int y = ylo + yy;
      ysh = stage_bytes(luma, frame + (size_t)y * a.pitch + a.x0, a.span, lane);
      const uint8_t* cplane = frame + a.chroma_offset;
      if (LAYOUT == VAURA_YUV_NV12) {
        ush = stage_bytes(chroma, cplane + (size_t)(y >> 1) * a.pitch + 2 * c0, 2 * nc, lane);
      } else {
        const size_t cp = (size_t)(a.pitch >> 1);
        ush = stage_bytes(chroma, cplane + (size_t)(y >> 1) * cp + c0, nc, lane);
        vsh = stage_bytes(chroma + yuv_plane_dwords(a.span), cplane + ((size_t)(a.H >> 1) + (y >> 1)) * cp + c0, nc, lane);
      }
    }
    __syncthreads();
    if (yy < nrows) {
      const uint8_t* yb = reinterpret_cast<const uint8_t*>(luma) + ysh;
      const uint8_t* ub = reinterpret_cast<const uint8_t*>(chroma) + ush;
      const uint8_t* vb = reinterpret_cast<const uint8_t*>(chroma + yuv_plane_dwords(a.span)) + vsh;
      for (int m = lane; m < rgbw; m += 64) {                          // 4 pixels per lane, one word per channel
        uint32_t wr = 0, wg = 0, wb = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = min(4 * m + e, a.span - 1);                    // the last word may pass the span: its spare bytes are never read
          const int ci = ((a.x0 + i) >> 1) - c0;
          const int u = (LAYOUT == VAURA_YUV_NV12 ? (int)ub[2 * ci] : (int)ub[ci]) - 128;
          const int v = (LAYOUT == VAURA_YUV_NV12 ? (int)ub[2 * ci + 1] : (int)vb[ci]) - 128;
          const int yv = a.cy * ((int)yb[i] - a.y_off) + (1 << (PREPROC_YUV_PREC - 1));
          wr |= color_u8(yv + a.crv * v) << (8 * e);
          wg |= color_u8(yv + a.cgu * u + a.cgv * v) << (8 * e);
          wb |= color_u8(yv + a.cbu * u) << (8 * e);
        }
        rgb[m] = wr;
        rgb[rgbw + m] = wg;
        rgb[2 * rgbw + m] = wb;
      }
    }
    __syncthreads();
    if (yy < nrows) {
#pragma unroll 1
      for (int c = 0; c < 3; ++c) {
        const uint8_t* sb = reinterpret_cast<const uint8_t*>(rgb + c * rgbw);
        for (int q = lane; q < nq; q += 64) {
          uint32_t word = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int x = 4 * q + e;
            const uint8_t* t = sb + hrel[x];
            const int16_t* w = hw + x * a.h_taps;
            int acc = hhalf;
            for (int k = 0; k < a.h_taps; ++k) acc += (int)t[k] * (int)w[k];
            word |= level_u8(acc, a.h_prec) << (8 * e);
          }
          tile[((size_t)c * a.tile_src_rows + yy) * nq + q] = word;
        }
      }
    }
    __syncthreads();
  }

  // ---- phase 2: vertical pass, level -> fp32 table, 16-byte stores.  A copy of video_preprocess_kernel's phase 2 and not a shared
  // inlined body, for the reason given at embed_clips_kernel (csrc/step.hip): the kernels every RGB call runs stay untouched source.
  const int vhalf = 1 << (a.v_prec - 1);
  const int items = 3 * nr * nq;
  for (int it = tid; it < items; it += 64 * PREPROC_WAVES) {
    const int q = it % nq, rc = it / nq, rr = rc % nr, c = rc / nr;
    const int r = r0 + rr;
    const int ys = min(max(a.v_start[r] - ylo, 0), nrows - a.v_taps);
    const int16_t* w = a.v_w + (size_t)r * a.v_taps;
    const uint32_t* t = tile + ((size_t)c * a.tile_src_rows + ys) * nq + q;
    int a0 = vhalf, a1 = vhalf, a2 = vhalf, a3 = vhalf;
    for (int k = 0; k < a.v_taps; ++k) {
      const uint32_t d = t[(size_t)k * nq];
      const int wk = w[k];
      a0 += (int)(d & 255u) * wk;
      a1 += (int)((d >> 8) & 255u) * wk;
      a2 += (int)((d >> 16) & 255u) * wk;
      a3 += (int)(d >> 24) * wk;
    }
    const float* l = lut + 256 * c;
    const f32x4 o = {l[level_u8(a0, a.v_prec)], l[level_u8(a1, a.v_prec)], l[level_u8(a2, a.v_prec)], l[level_u8(a3, a.v_prec)]};
    float* dst = a.out + ((((size_t)bs * 3 + c) * a.F + f) * a.crop_h + r) * a.crop_w + 4 * q;
    *reinterpret_cast<f32x4*>(dst) = o;
  }
}

// ---- The same launches with every output frame's source frame read from a device table (video at its own frame rate: the host's
// fps plan names, per 25 fps tick, the source frame shown; vaura_amd/preprocess.py: fps_plan).  In the kernels above the source frame
// is `b * T + seg_start + s * seg_stride + f`; here it is frame_map[(b * S + s) * F + f], one wave-uniform read:
//   e >= 0  source frame e of the clip, clamped into [0, T)        -1  the output frame is left as it is (the workgroup returns)
//   -2      the clip's frame in `carry` (one frame per clip in the source layout: the last frame of an earlier block of a stream)
// They are kernels of their own so that the four functions above stay the source and the device code they were; the argument
// structs embed theirs, and the staging, filtering and store are restated once for these kernels (frames_prologue, frames_phase2).
struct PreprocFramesArgs {
  PreprocArgs p;
  const int32_t* frame_map;   // (n_clips, S * F)
  const uint8_t* carry;       // n_clips frames, or NULL
};

struct PreprocYuvFramesArgs {
  PreprocYuvArgs p;
  const int32_t* frame_map;
  const uint8_t* carry;       // clip b's surface at byte b * frame_stride, or NULL
};

// first byte of the source frame of output frame `of` (clip b), NULL where the output frame is left as it is; a -2 without a carry
// buffer is refused by the host and leaves the frame as it is here
template <class A>
__device__ __forceinline__ const uint8_t* mapped_frame(const A& a, int of, int b, size_t frame_bytes) {
  const int e = a.frame_map[of];
  if (e == -2 && a.carry) return a.carry + (size_t)b * frame_bytes;
  if (e == -1 || e == -2) return nullptr;
  return a.p.src + ((size_t)b * a.p.T + min(max(e, 0), a.p.T - 1)) * frame_bytes;
}

struct PreprocLds {
  float* lut;        // 768 floats
  int32_t* hrel;     // crop_w
  int16_t* hw;       // crop_w * h_taps
  uint32_t* slabs;   // PREPROC_WAVES slabs of slab_dwords
  uint32_t* tile;    // [3][tile_src_rows][crop_w / 4] words of 4 uint8
};

// the workgroup's LDS layout (that of the kernels above) with the three tables copied in; ends with a barrier
template <class P>
__device__ __forceinline__ PreprocLds frames_prologue(const P& a, uint32_t* smem, int tid) {
  PreprocLds l;
  l.lut = reinterpret_cast<float*>(smem);
  l.hrel = reinterpret_cast<int32_t*>(smem + 768);
  l.hw = reinterpret_cast<int16_t*>(smem + 768 + a.crop_w);
  l.slabs = smem + 768 + a.crop_w + ((a.crop_w * a.h_taps) >> 1);
  l.tile = l.slabs + PREPROC_WAVES * a.slab_dwords;
  for (int i = tid; i < 768; i += 64 * PREPROC_WAVES) l.lut[i] = a.lut[i];
  for (int i = tid; i < a.crop_w; i += 64 * PREPROC_WAVES) l.hrel[i] = min(max(a.h_rel[i], 0), a.span - a.h_taps);
  for (int i = tid; i < a.crop_w * a.h_taps; i += 64 * PREPROC_WAVES) l.hw[i] = a.h_w[i];
  __syncthreads();
  return l;
}

// horizontal pass of one planar uint8 row `sb` (pixel step PIX bytes) into row yy of channel c of the tile
template <int PIX, class P>
__device__ __forceinline__ void frames_filter_row(const P& a, const PreprocLds& l, const uint8_t* sb, int c, int yy, int lane) {
  const int nq = a.crop_w >> 2;
  const int hhalf = 1 << (a.h_prec - 1);
  for (int q = lane; q < nq; q += 64) {
    uint32_t word = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = 4 * q + e;
      const uint8_t* t = sb + PIX * l.hrel[x];
      const int16_t* w = l.hw + x * a.h_taps;
      int acc = hhalf;
      for (int k = 0; k < a.h_taps; ++k) acc += (int)t[PIX * k] * (int)w[k];
      word |= level_u8(acc, a.h_prec) << (8 * e);
    }
    l.tile[((size_t)c * a.tile_src_rows + yy) * nq + q] = word;
  }
}

// vertical pass, level -> fp32 table, 16-byte stores: phase 2 of the kernels above
template <class P>
__device__ __forceinline__ void frames_phase2(const P& a, const PreprocLds& l, int bs, int f, int r0, int nr, int ylo, int nrows, int tid) {
  const int nq = a.crop_w >> 2;
  const int vhalf = 1 << (a.v_prec - 1);
  const int items = 3 * nr * nq;
  for (int it = tid; it < items; it += 64 * PREPROC_WAVES) {
    const int q = it % nq, rc = it / nq, rr = rc % nr, c = rc / nr;
    const int r = r0 + rr;
    const int ys = min(max(a.v_start[r] - ylo, 0), nrows - a.v_taps);
    const int16_t* w = a.v_w + (size_t)r * a.v_taps;
    const uint32_t* t = l.tile + ((size_t)c * a.tile_src_rows + ys) * nq + q;
    int a0 = vhalf, a1 = vhalf, a2 = vhalf, a3 = vhalf;
    for (int k = 0; k < a.v_taps; ++k) {
      const uint32_t d = t[(size_t)k * nq];
      const int wk = w[k];
      a0 += (int)(d & 255u) * wk;
      a1 += (int)((d >> 8) & 255u) * wk;
      a2 += (int)((d >> 16) & 255u) * wk;
      a3 += (int)(d >> 24) * wk;
    }
    const float* lc = l.lut + 256 * c;
    const f32x4 o = {lc[level_u8(a0, a.v_prec)], lc[level_u8(a1, a.v_prec)], lc[level_u8(a2, a.v_prec)], lc[level_u8(a3, a.v_prec)]};
    float* dst = a.out + ((((size_t)bs * 3 + c) * a.F + f) * a.crop_h + r) * a.crop_w + 4 * q;
    *reinterpret_cast<f32x4*>(dst) = o;
  }
}

template <bool NHWC>
__global__ __launch_bounds__(64 * PREPROC_WAVES) void video_preprocess_frames_kernel(const PreprocFramesArgs fa) {
  extern __shared__ uint32_t smem[];
  const PreprocArgs& a = fa.p;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int of = blockIdx.y;                                           // output frame (b, s, f)
  const int f = of % a.F, bs = of / a.F, b = bs / a.S;
  const uint8_t* frame = mapped_frame(fa, of, b, (size_t)3 * a.H * a.W);   // the same for the whole workgroup
  if (!frame) return;
  const int r0 = blockIdx.x * a.tile_rows;
  const int nr = min(a.tile_rows, a.crop_h - r0);
  const int ylo = min(max(a.v_start[r0], 0), a.H - a.v_taps);
  const int nrows = min(a.tile_src_rows, a.H - ylo);
  const PreprocLds l = frames_prologue(a, smem, tid);

  // ---- phase 1: horizontal pass into the tile, one source row of one channel [NCHW] or of all three [NHWC] per wave
  uint32_t* slab = l.slabs + wave * a.slab_dwords;
  const int jobs = NHWC ? nrows : 3 * nrows;
  for (int j0 = 0; j0 < jobs; j0 += PREPROC_WAVES) {
    const int j = j0 + wave;                                           // wave-uniform
    const int yy = NHWC ? j : j / 3, cj = NHWC ? 0 : j - 3 * yy;
    int shift = 0;
    if (j < jobs) {
      const size_t row = NHWC ? ((size_t)(ylo + yy) * a.W + a.x0) * 3 : ((size_t)cj * a.H + (ylo + yy)) * a.W + a.x0;
      shift = stage_bytes(slab, frame + row, (NHWC ? 3 : 1) * a.span, lane);
    }
    __syncthreads();
    if (j < jobs) {
      const uint8_t* sb = reinterpret_cast<const uint8_t*>(slab) + shift;
      if (NHWC) {
#pragma unroll 1
        for (int c = 0; c < 3; ++c) frames_filter_row<3>(a, l, sb + c, c, yy, lane);
      } else {
        frames_filter_row<1>(a, l, sb, cj, yy, lane);
      }
    }
    __syncthreads();
  }
  frames_phase2(a, l, bs, f, r0, nr, ylo, nrows, tid);
}

template <int LAYOUT>   // VAURA_YUV_NV12 / VAURA_YUV_I420
__global__ __launch_bounds__(64 * PREPROC_WAVES) void video_preprocess_yuv_frames_kernel(const PreprocYuvFramesArgs fa) {
  extern __shared__ uint32_t smem[];
  const PreprocYuvArgs& a = fa.p;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int of = blockIdx.y;                                           // output frame (b, s, f)
  const int f = of % a.F, bs = of / a.F, b = bs / a.S;
  const uint8_t* frame = mapped_frame(fa, of, b, (size_t)a.frame_stride);
  if (!frame) return;
  const int r0 = blockIdx.x * a.tile_rows;
  const int nr = min(a.tile_rows, a.crop_h - r0);
  const int ylo = min(max(a.v_start[r0], 0), a.H - a.v_taps);
  const int nrows = min(a.tile_src_rows, a.H - ylo);
  const PreprocLds l = frames_prologue(a, smem, tid);

  // ---- phase 1: one source row per wave: stage luma + chroma, convert once, horizontal pass of the three channels into the tile
  uint32_t* luma = l.slabs + wave * a.slab_dwords;
  uint32_t* chroma = luma + yuv_luma_dwords(a.span);
  uint32_t* rgb = chroma + yuv_chroma_dwords(a.span);
  const int rgbw = yuv_rgb_dwords(a.span);
  const int c0 = a.x0 >> 1;                                            // first chroma sample of the span
  const int nc = ((a.x0 + a.span - 1) >> 1) - c0 + 1;                  // chroma samples the span touches (<= span / 2 + 1)
  for (int j0 = 0; j0 < nrows; j0 += PREPROC_WAVES) {
    const int yy = j0 + wave;                                          // wave-uniform
    int ysh = 0, ush = 0, vsh = 0;
    if (yy < nrows) {
      const int y = ylo + yy;
      ysh = stage_bytes(luma, frame + (size_t)y * a.pitch + a.x0, a.span, lane);
      const uint8_t* cplane = frame + a.chroma_offset;
      if (LAYOUT == VAURA_YUV_NV12) {
        ush = stage_bytes(chroma, cplane + (size_t)(y >> 1) * a.pitch + 2 * c0, 2 * nc, lane);
      } else {
        const size_t cp = (size_t)(a.pitch >> 1);
        ush = stage_bytes(chroma, cplane + (size_t)(y >> 1) * cp + c0, nc, lane);
        vsh = stage_bytes(chroma + yuv_plane_dwords(a.span), cplane + ((size_t)(a.H >> 1) + (y >> 1)) * cp + c0, nc, lane);
      }
    }
    __syncthreads();
    if (yy < nrows) {
      const uint8_t* yb = reinterpret_cast<const uint8_t*>(luma) + ysh;
      const uint8_t* ub = reinterpret_cast<const uint8_t*>(chroma) + ush;
      const uint8_t* vb = reinterpret_cast<const uint8_t*>(chroma + yuv_plane_dwords(a.span)) + vsh;
      for (int m = lane; m < rgbw; m += 64) {                          // 4 pixels per lane, one word per channel
        uint32_t wr = 0, wg = 0, wb = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = min(4 * m + e, a.span - 1);                    // the last word may pass the span: its spare bytes are never read
          const int ci = ((a.x0 + i) >> 1) - c0;
          const int u = (LAYOUT == VAURA_YUV_NV12 ? (int)ub[2 * ci] : (int)ub[ci]) - 128;
          const int v = (LAYOUT == VAURA_YUV_NV12 ? (int)ub[2 * ci + 1] : (int)vb[ci]) - 128;
          const int yv = a.cy * ((int)yb[i] - a.y_off) + (1 << (PREPROC_YUV_PREC - 1));
          wr |= color_u8(yv + a.crv * v) << (8 * e);
          wg |= color_u8(yv + a.cgu * u + a.cgv * v) << (8 * e);
          wb |= color_u8(yv + a.cbu * u) << (8 * e);
        }
        rgb[m] = wr;
        rgb[rgbw + m] = wg;
        rgb[2 * rgbw + m] = wb;
      }
    }
    __syncthreads();
    if (yy < nrows) {
#pragma unroll 1
      for (int c = 0; c < 3; ++c) frames_filter_row<1>(a, l, reinterpret_cast<const uint8_t*>(rgb + c * rgbw), c, yy, lane);
    }
    __syncthreads();
  }
  frames_phase2(a, l, bs, f, r0, nr, ylo, nrows, tid);
}

extern "C" {

// what both entry points refuse about the resize / crop / segments / tables, in vaura_video_preprocess's order
static int preproc_check(int n_clips, int T, int C, int H, int W, int resize, int crop_h, int crop_w, int F, int S, int seg_start,
                         int seg_stride, const int32_t* h_rel, const int16_t* h_w, int h_taps, int h_prec, const int32_t* v_start,
                         const int16_t* v_w, int v_taps, int v_prec, int x0, int span, int tile_rows, int tile_src_rows, const float* lut,
                         const float* out) {
  if (n_clips <= 0 || T <= 0 || H <= 0 || W <= 0 || resize <= 0 || crop_h <= 0 || crop_w <= 0 || F <= 0) return VAURA_ERR_ARG;
  if (C != 3) return VAURA_ERR_SHAPE;
  // torchvision's Resize(int): the short side to `resize`, the long side to int(resize * long / short)
  const int lng = H > W ? H : W, sht = H > W ? W : H;
  const int rl = (int)((double)resize * (double)lng / (double)sht);
  const int oh = H <= W ? resize : rl, ow = H <= W ? rl : resize;
  if (crop_h > oh || crop_w > ow || (crop_w & 3)) return VAURA_ERR_SHAPE;
  if (T < F) return VAURA_ERR_SHAPE;
  if (h_taps > PREPROC_MAX_TAPS || v_taps > PREPROC_MAX_TAPS) return VAURA_ERR_SHAPE;
  if (S <= 0 || seg_start < 0 || seg_stride <= 0 || (int64_t)seg_start + (int64_t)(S - 1) * seg_stride + F > T) return VAURA_ERR_SHAPE;
  if (h_taps <= 0 || v_taps <= 0 || h_prec <= 0 || h_prec > 22 || v_prec <= 0 || v_prec > 22) return VAURA_ERR_ARG;
  if (x0 < 0 || span < h_taps || (int64_t)x0 + span > W || v_taps > H) return VAURA_ERR_ARG;
  if (tile_rows <= 0 || tile_src_rows < v_taps || tile_src_rows > H) return VAURA_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(out) & 15) || (reinterpret_cast<uintptr_t>(h_rel) & 3) || (reinterpret_cast<uintptr_t>(v_start) & 3) ||
      (reinterpret_cast<uintptr_t>(h_w) & 1) || (reinterpret_cast<uintptr_t>(v_w) & 1) || (reinterpret_cast<uintptr_t>(lut) & 3))
    return VAURA_ERR_ARG;
  if ((int64_t)n_clips * S * F > 65535) return VAURA_ERR_SHAPE;       // gridDim.y
  return 0;
}

int vaura_video_preprocess(const uint8_t* video, int channels_last, int n_clips, int T, int C, int H, int W, int resize, int crop_h,
                           int crop_w, int F, int S, int seg_start, int seg_stride, const int32_t* h_rel, const int16_t* h_w, int h_taps,
                           int h_prec, const int32_t* v_start, const int16_t* v_w, int v_taps, int v_prec, int x0, int span,
                           int tile_rows, int tile_src_rows, const float* lut, float* out, vaura_stream_t s) {
  if (!video || !h_rel || !h_w || !v_start || !v_w || !lut || !out) return VAURA_ERR_ARG;
  if (const int st = preproc_check(n_clips, T, C, H, W, resize, crop_h, crop_w, F, S, seg_start, seg_stride, h_rel, h_w, h_taps, h_prec,
                                   v_start, v_w, v_taps, v_prec, x0, span, tile_rows, tile_src_rows, lut, out))
    return st;
  const int64_t frames_out = (int64_t)n_clips * S * F;
  PreprocArgs a;
  a.src = video; a.h_rel = h_rel; a.h_w = h_w; a.v_start = v_start; a.v_w = v_w; a.lut = lut; a.out = out;
  a.T = T; a.H = H; a.W = W; a.S = S; a.F = F; a.seg_start = seg_start; a.seg_stride = seg_stride;
  a.crop_h = crop_h; a.crop_w = crop_w; a.h_taps = h_taps; a.h_prec = h_prec; a.v_taps = v_taps; a.v_prec = v_prec;
  a.x0 = x0; a.span = span; a.tile_rows = tile_rows; a.tile_src_rows = tile_src_rows;
  a.slab_dwords = ((channels_last ? 3 : 1) * span + 3 + 3) >> 2;
  const size_t lds = preproc_lds_bytes(channels_last, crop_w, h_taps, span, tile_src_rows);
  if (lds > PREPROC_LDS_LIMIT) return VAURA_ERR_SHAPE;
  const dim3 grid((unsigned)((crop_h + tile_rows - 1) / tile_rows), (unsigned)frames_out);
  hipStream_t st = as_stream(s);
  if (channels_last) VA_LAUNCH(video_preprocess_kernel<true>, grid, dim3(64 * PREPROC_WAVES), lds, st, a);
  else VA_LAUNCH(video_preprocess_kernel<false>, grid, dim3(64 * PREPROC_WAVES), lds, st, a);
  return 0;
}

size_t vaura_video_preprocess_lds_bytes(int channels_last, int crop_w, int h_taps, int span, int tile_src_rows) {
  if (crop_w <= 0 || (crop_w & 3) || h_taps <= 0 || span <= 0 || tile_src_rows <= 0) return 0;
  return preproc_lds_bytes(channels_last, crop_w, h_taps, span, tile_src_rows);
}

// what both 4:2:0 entry points refuse about the surfaces and the colour formula, after preproc_check
static int preproc_yuv_check(int64_t video_bytes, int layout, int64_t pitch, int64_t chroma_offset, int64_t frame_stride, int n_clips, int T,
                             int H, int W, int y_off, int cy, int crv, int cgu, int cgv, int cbu) {
  if ((H & 1) || (W & 1)) return VAURA_ERR_SHAPE;                      // 4:2:0: one chroma sample per 2 x 2 luma block
  // |acc| <= 3 * 2^20 * 256 < 2^31 for any such coefficients (the host's are below 2^16)
  const int lim = 1 << 20;
  if (y_off < 0 || y_off > 255 || cy < -lim || cy > lim || crv < -lim || crv > lim || cgu < -lim || cgu > lim || cgv < -lim || cgv > lim ||
      cbu < -lim || cbu > lim)
    return VAURA_ERR_ARG;
  if (pitch < W || pitch > (int64_t)1 << 30 || (layout == VAURA_YUV_I420 && (pitch & 1))) return VAURA_ERR_ARG;
  // the planes of one frame, in bytes from its start: luma [0, luma_end), chroma [chroma_offset, frame_end)
  const int64_t luma_end = (int64_t)(H - 1) * pitch + W;
  const int64_t chroma_bytes = layout == VAURA_YUV_NV12 ? (int64_t)(H / 2 - 1) * pitch + W
                                                         : (int64_t)(H / 2) * (pitch / 2) + (int64_t)(H / 2 - 1) * (pitch / 2) + W / 2;
  if (chroma_offset < luma_end || chroma_offset > (int64_t)1 << 40) return VAURA_ERR_ARG;      // planes overlap
  const int64_t frame_end = chroma_offset + chroma_bytes;
  if (frame_stride < frame_end || frame_stride > (int64_t)1 << 40) return VAURA_ERR_ARG;       // frames overlap
  const int64_t n_frames = (int64_t)n_clips * T;
  if (video_bytes < 0 || n_frames - 1 > (video_bytes - frame_end) / frame_stride || video_bytes < frame_end) return VAURA_ERR_ARG;
  return 0;
}

int vaura_video_preprocess_yuv420(const uint8_t* video, int64_t video_bytes, int layout, int64_t pitch, int64_t chroma_offset,
                                  int64_t frame_stride, int n_clips, int T, int H, int W, int y_off, int cy, int crv, int cgu, int cgv,
                                  int cbu, int resize, int crop_h, int crop_w, int F, int S, int seg_start, int seg_stride,
                                  const int32_t* h_rel, const int16_t* h_w, int h_taps, int h_prec, const int32_t* v_start,
                                  const int16_t* v_w, int v_taps, int v_prec, int x0, int span, int tile_rows, int tile_src_rows,
                                  const float* lut, float* out, vaura_stream_t s) {
  if (!video || !h_rel || !h_w || !v_start || !v_w || !lut || !out) return VAURA_ERR_ARG;
  if (layout != VAURA_YUV_NV12 && layout != VAURA_YUV_I420) return VAURA_ERR_ARG;
  if (const int st = preproc_check(n_clips, T, 3, H, W, resize, crop_h, crop_w, F, S, seg_start, seg_stride, h_rel, h_w, h_taps, h_prec,
                                   v_start, v_w, v_taps, v_prec, x0, span, tile_rows, tile_src_rows, lut, out))
    return st;
  if (const int st = preproc_yuv_check(video_bytes, layout, pitch, chroma_offset, frame_stride, n_clips, T, H, W, y_off, cy, crv, cgu, cgv, cbu))
    return st;
  PreprocYuvArgs a;
  a.src = video; a.h_rel = h_rel; a.h_w = h_w; a.v_start = v_start; a.v_w = v_w; a.lut = lut; a.out = out;
  a.pitch = pitch; a.chroma_offset = chroma_offset; a.frame_stride = frame_stride;
  a.y_off = y_off; a.cy = cy; a.crv = crv; a.cgu = cgu; a.cgv = cgv; a.cbu = cbu;
  a.T = T; a.H = H; a.W = W; a.S = S; a.F = F; a.seg_start = seg_start; a.seg_stride = seg_stride;
  a.crop_h = crop_h; a.crop_w = crop_w; a.h_taps = h_taps; a.h_prec = h_prec; a.v_taps = v_taps; a.v_prec = v_prec;
  a.x0 = x0; a.span = span; a.tile_rows = tile_rows; a.tile_src_rows = tile_src_rows;
  a.slab_dwords = yuv_slab_dwords(span);
  const size_t lds = preproc_yuv_lds_bytes(crop_w, h_taps, span, tile_src_rows);
  if (lds > PREPROC_LDS_LIMIT) return VAURA_ERR_SHAPE;
  const dim3 grid((unsigned)((crop_h + tile_rows - 1) / tile_rows), (unsigned)((int64_t)n_clips * S * F));
  hipStream_t st = as_stream(s);
  if (layout == VAURA_YUV_NV12) VA_LAUNCH(video_preprocess_yuv_kernel<VAURA_YUV_NV12>, grid, dim3(64 * PREPROC_WAVES), lds, st, a);
  else VA_LAUNCH(video_preprocess_yuv_kernel<VAURA_YUV_I420>, grid, dim3(64 * PREPROC_WAVES), lds, st, a);
  return 0;
}

size_t vaura_video_preprocess_yuv420_lds_bytes(int layout, int crop_w, int h_taps, int span, int tile_src_rows) {
  if ((layout != VAURA_YUV_NV12 && layout != VAURA_YUV_I420) || crop_w <= 0 || (crop_w & 3) || h_taps <= 0 || span <= 0 || tile_src_rows <= 0)
    return 0;
  return preproc_yuv_lds_bytes(crop_w, h_taps, span, tile_src_rows);
}

// ---- the launches with a frame table.  The segment arguments of the siblings have no meaning here (the table names the source
// frame of every output frame), so they are not taken; what preproc_check says about segments is asked of the output sequence.
static int preproc_frames_check(const int32_t* frame_map, const uint8_t* carry, int carry_used, int T, int F, int S) {
  if (!frame_map || (reinterpret_cast<uintptr_t>(frame_map) & 3)) return VAURA_ERR_ARG;
  if (carry_used && !carry) return VAURA_ERR_ARG;
  if (T <= 0 || F <= 0) return VAURA_ERR_ARG;
  if (S <= 0 || S > 65535 || F > 65535) return VAURA_ERR_SHAPE;
  return 0;
}

int vaura_video_preprocess_frames(const uint8_t* video, int channels_last, int n_clips, int T, int C, int H, int W, int resize,
                                  int crop_h, int crop_w, int F, int S, const int32_t* h_rel, const int16_t* h_w, int h_taps, int h_prec,
                                  const int32_t* v_start, const int16_t* v_w, int v_taps, int v_prec, int x0, int span, int tile_rows,
                                  int tile_src_rows, const float* lut, float* out, const int32_t* frame_map, const uint8_t* carry,
                                  int carry_used, vaura_stream_t s) {
  if (!video || !h_rel || !h_w || !v_start || !v_w || !lut || !out) return VAURA_ERR_ARG;
  if (const int st = preproc_frames_check(frame_map, carry, carry_used, T, F, S)) return st;
  if (const int st = preproc_check(n_clips, S * F, C, H, W, resize, crop_h, crop_w, F, S, 0, F, h_rel, h_w, h_taps, h_prec, v_start, v_w,
                                   v_taps, v_prec, x0, span, tile_rows, tile_src_rows, lut, out))
    return st;
  PreprocFramesArgs fa;
  PreprocArgs& a = fa.p;
  a.src = video; a.h_rel = h_rel; a.h_w = h_w; a.v_start = v_start; a.v_w = v_w; a.lut = lut; a.out = out;
  a.T = T; a.H = H; a.W = W; a.S = S; a.F = F; a.seg_start = 0; a.seg_stride = F;
  a.crop_h = crop_h; a.crop_w = crop_w; a.h_taps = h_taps; a.h_prec = h_prec; a.v_taps = v_taps; a.v_prec = v_prec;
  a.x0 = x0; a.span = span; a.tile_rows = tile_rows; a.tile_src_rows = tile_src_rows;
  a.slab_dwords = ((channels_last ? 3 : 1) * span + 3 + 3) >> 2;
  fa.frame_map = frame_map; fa.carry = carry;
  const size_t lds = preproc_lds_bytes(channels_last, crop_w, h_taps, span, tile_src_rows);
  if (lds > PREPROC_LDS_LIMIT) return VAURA_ERR_SHAPE;
  const dim3 grid((unsigned)((crop_h + tile_rows - 1) / tile_rows), (unsigned)((int64_t)n_clips * S * F));
  hipStream_t st = as_stream(s);
  if (channels_last) VA_LAUNCH(video_preprocess_frames_kernel<true>, grid, dim3(64 * PREPROC_WAVES), lds, st, fa);
  else VA_LAUNCH(video_preprocess_frames_kernel<false>, grid, dim3(64 * PREPROC_WAVES), lds, st, fa);
  return 0;
}

int vaura_video_preprocess_yuv420_frames(const uint8_t* video, int64_t video_bytes, int layout, int64_t pitch, int64_t chroma_offset,
                                         int64_t frame_stride, int n_clips, int T, int H, int W, int y_off, int cy, int crv, int cgu,
                                         int cgv, int cbu, int resize, int crop_h, int crop_w, int F, int S, const int32_t* h_rel,
                                         const int16_t* h_w, int h_taps, int h_prec, const int32_t* v_start, const int16_t* v_w,
                                         int v_taps, int v_prec, int x0, int span, int tile_rows, int tile_src_rows, const float* lut,
                                         float* out, const int32_t* frame_map, const uint8_t* carry, int carry_used, vaura_stream_t s) {
  if (!video || !h_rel || !h_w || !v_start || !v_w || !lut || !out) return VAURA_ERR_ARG;
  if (layout != VAURA_YUV_NV12 && layout != VAURA_YUV_I420) return VAURA_ERR_ARG;
  if (const int st = preproc_frames_check(frame_map, carry, carry_used, T, F, S)) return st;
  if (const int st = preproc_check(n_clips, S * F, 3, H, W, resize, crop_h, crop_w, F, S, 0, F, h_rel, h_w, h_taps, h_prec, v_start, v_w,
                                   v_taps, v_prec, x0, span, tile_rows, tile_src_rows, lut, out))
    return st;
  if (const int st = preproc_yuv_check(video_bytes, layout, pitch, chroma_offset, frame_stride, n_clips, T, H, W, y_off, cy, crv, cgu, cgv, cbu))
    return st;
  PreprocYuvFramesArgs fa;
  PreprocYuvArgs& a = fa.p;
  a.src = video; a.h_rel = h_rel; a.h_w = h_w; a.v_start = v_start; a.v_w = v_w; a.lut = lut; a.out = out;
  a.pitch = pitch; a.chroma_offset = chroma_offset; a.frame_stride = frame_stride;
  a.y_off = y_off; a.cy = cy; a.crv = crv; a.cgu = cgu; a.cgv = cgv; a.cbu = cbu;
  a.T = T; a.H = H; a.W = W; a.S = S; a.F = F; a.seg_start = 0; a.seg_stride = F;
  a.crop_h = crop_h; a.crop_w = crop_w; a.h_taps = h_taps; a.h_prec = h_prec; a.v_taps = v_taps; a.v_prec = v_prec;
  a.x0 = x0; a.span = span; a.tile_rows = tile_rows; a.tile_src_rows = tile_src_rows;
  a.slab_dwords = yuv_slab_dwords(span);
  fa.frame_map = frame_map; fa.carry = carry;
  const size_t lds = preproc_yuv_lds_bytes(crop_w, h_taps, span, tile_src_rows);
  if (lds > PREPROC_LDS_LIMIT) return VAURA_ERR_SHAPE;
  const dim3 grid((unsigned)((crop_h + tile_rows - 1) / tile_rows), (unsigned)((int64_t)n_clips * S * F));
  hipStream_t st = as_stream(s);
  if (layout == VAURA_YUV_NV12) VA_LAUNCH(video_preprocess_yuv_frames_kernel<VAURA_YUV_NV12>, grid, dim3(64 * PREPROC_WAVES), lds, st, fa);
  else VA_LAUNCH(video_preprocess_yuv_frames_kernel<VAURA_YUV_I420>, grid, dim3(64 * PREPROC_WAVES), lds, st, fa);
  return 0;
}

}  // extern "C"
