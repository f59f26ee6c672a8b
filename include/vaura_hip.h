/*
 * vaura_hip.h — C ABI of libvaura_hip.so, the MI355X (gfx950) generation hot path of V-AURA.
 *
 * The reference (ilpoviertola/V-AURA) has no native code and no FFI: its hot path is the Python
 * call chain  VAURAModel.generate() -> _sample_next_token() -> llama.Transformer.forward()
 * -> sample_top_k/top_p -> DacModelWrapper.decode().  This header is the native boundary a
 * maintainer binds *under* those Python plugin classes (ctypes stub: INTEGRATION.md).  Each entry
 * point cites the reference interface it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - extern "C", plain pointers / sizes / a POD descriptor struct; no torch types.
 *   - every pointer is a DEVICE pointer unless its name ends in _host.
 *   - returns 0 on success, a negative vaura_status on an argument error, a positive value = hipError_t.
 *   - never allocates device memory, never synchronises the stream, never throws.
 *   - everything is enqueued on the hipStream_t that is passed in (pass torch's current stream).
 *   - one caller thread per device; re-entrant across devices, not within one descriptor.
 *
 * Activation layout ("packed rows"): a (rows x C) fp32 matrix is stored in blocks of 16 rows as
 *     [row_block][C/4][16 rows][4 cols]   ->  float index  ((rb*(C/4) + c/4)*16 + r%16)*4 + c%4
 *   so that one 64-lane wavefront reads/writes one 16x16 MFMA operand tile as a contiguous 1 KiB.
 *   rows beyond the live ones in the last block must be zero.
 *
 * Streamed-weight layout ("MFMA tiles"): an (N x K) matrix, N%16==0, K%32==0, is stored as
 *     [N/16][K/32][64 lanes][8]  with lane = (n%16) + 16*((k%32)/8), element j = k%8
 *   (VAURA_W_F32: [N/16][K/32][2 halves][64 lanes][4] fp32;  VAURA_W_BF16: 8 bf16 per lane;
 *    VAURA_W_H1:  8 fp16 per lane = W[n,k] / scale[n], followed by float scale[N] (power of two, max|W[n,:]| / scale in [2^13, 2^14));
 *    VAURA_W_H2:  [N/16][K/32][2 planes][64 lanes][8 fp16]: hi = fp16(W/scale), lo = fp16(W/scale - hi), followed by scale[N];
 *    VAURA_W_FP8: [N/16][K/64][64 lanes][16 bytes] = the lane's 8 values of the even then of the odd k-group, K%64==0,
 *          followed by float scale[N], scale[n] = smallest power of two with max|W[n,:]| <= 448*scale[n]);
 *   see vaura_pack_weight().
 */
#ifndef VAURA_HIP_H
#define VAURA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vaura_stream_t; /* hipStream_t */

typedef enum vaura_status {
  VAURA_OK = 0,
  VAURA_ERR_ARG = -1,       /* null pointer / size out of range            */
  VAURA_ERR_SHAPE = -2,     /* dims not supported by the compiled kernels  */
  VAURA_ERR_DTYPE = -3,
  VAURA_ERR_STATE = -4      /* e.g. step graph not built                   */
} vaura_status;

/* storage of the streamed matrices.
 *   VAURA_W_H2  (hi, lo) fp16 planes + power-of-two row scales: 22 significand bits, 4 bytes per weight — fp32 checkpoints on
 *               the fp16-pair decode kernels (gemv3_kernel.h); the default for real (fp32) checkpoints
 *   VAURA_W_H1  one fp16 plane + row scales, 2 bytes per weight: lossless for checkpoints whose weights fit 11 significand
 *               bits (bf16-representable ones: 8)
 *   VAURA_W_FP8 (BASELINE configs[4]; no reference counterpart): OCP e4m3 with one power-of-two scale per output row, for the
 *               four per-layer matrices; heads stay VAURA_W_H1.  Multiplied against BOTH activation planes: exactly the H1
 *               arithmetic on the dequantised checkpoint (tested as such)
 *   VAURA_W_FP8H (round 6, configs[4]'s measured configuration): the SAME packed bytes as VAURA_W_FP8, multiplied against the hi
 *               activation plane only (11-bit activations under 4-bit-significand weights): half the plane bytes through every CU,
 *               half the matrix instructions; tolerance against VAURA_W_FP8 / H1 reported by the tests and bench.py, not bit parity
 *   VAURA_W_F32 / VAURA_W_BF16: fp32 / bf16 MFMA tiles of the exact-fp32-MFMA GEMVs (gemv_kernel.h): the conditioning MLP, and
 *               the decode step when the split workspaces are NULL (an exact, slower cross-check)                        */
typedef enum vaura_wdtype { VAURA_W_F32 = 0, VAURA_W_BF16 = 1, VAURA_W_FP8 = 2, VAURA_W_H1 = 3, VAURA_W_H2 = 4, VAURA_W_FP8H = 5 } vaura_wdtype;

/* ---- model geometry: configs/modules/samplers/llama_9cbs.yaml:3-17 + sampler/llama.py:308-361 */
typedef struct vaura_dims {
  int32_t n_layer;      /* 24   */
  int32_t d_model;      /* 1536 */
  int32_t n_head;       /* 16   (head_dim = d_model / n_head = 96) */
  int32_t ffn_dim;      /* 4096 */
  int32_t n_codebooks;  /* 9    */
  int32_t vocab;        /* 1024 (special token id == vocab) */
  int32_t cond_dim;     /* 512  */
  int32_t tok_dim;      /* 1024 */
  int32_t cond_in;      /* 768  */
  int32_t codebook_dim; /* 8    */
  int32_t tokens_per_frame; /* 7, scripts/generate.py:216 */
  float   eps;          /* 1e-5 */
} vaura_dims;

/* ---- per-layer streamed weights, MFMA-tile layout, dtype = vaura_decoder.wdtype */
typedef struct vaura_layer_weights {
  const void*  wqkv;       /* (3*d_model x d_model)                       llama.py:211 */
  const void*  wo;         /* (d_model x d_model)                         llama.py:212 */
  const void*  w13;        /* (2*ffn x d_model): 16-row tiles interleaved w1,w3   llama.py:171-172 */
  const void*  w2;         /* (d_model x ffn)                             llama.py:173 */
  const float* attn_norm;  /* (d_model) gain                              llama.py:268 */
  const float* ffn_norm;   /* (d_model) gain                              llama.py:269 */
} vaura_layer_weights;

/* ---- sampling parameters: VAURAModel._sample_next_token, models/vaura_model.py:775-827 */
typedef struct vaura_sampling {
  int32_t use_sampling;   /* 0 -> greedy argmax of the logits (vaura_model.py:825) */
  float   temp;           /* <= 0 -> greedy                                        */
  int32_t top_k;          /* used when top_p <= 0 and top_k > 0 (utils/utils.py:163-178) */
  float   top_p;          /* > 0 wins over top_k (vaura_model.py:818-819; utils/utils.py:181-196) */
  float   cfg_scale;      /* > 1 -> rows [B,2B) are the null-condition branch (vaura_model.py:786-813) */
  uint64_t seed;          /* Philox key when noise == NULL                          */
  uint64_t clip_base;     /* global index of clip 0 (keeps draws invariant to batch sharding) */
  int32_t input_is_probs; /* 1: the input rows already are probabilities (utils/utils.py sample_top_k / sample_top_p / multinomial
                             take probs): no temperature, no softmax, no CFG mix.  0 in the decode loop                       */
  float   tie_eps;        /* near-tie detector (round 6), 0 = off: RELATIVE bound on the error of a logit as the plane storages deliver it
                             (x the row's largest |logit|, x (2 cfg_scale - 1) through the CFG mix).  A used decision whose own margin is
                             inside twice that bound — greedy: top-1 - top-2 of the mixed logits; sampled: the runner-up of argmax(p / q),
                             and the top-k threshold where it could change the draw — is counted in state[6] (state[7] = first such
                             step + 1) and raises VAURA_STATUS_NEAR_TIE.  The token chosen is never changed by the detector           */
} vaura_sampling;

/* ---- the same five parameters for ONE clip of a batched call: vaura_decoder.clip_sampling / vaura_sample_clips take B of these in
 * DEVICE memory, record b for clip b.  32 bytes, 16-byte aligned, plain 4-byte fields (the sampler's workgroup of clip b fetches its
 * record with two vector loads, 16 + 4 bytes).  Every field means what its namesake in vaura_sampling means. */
typedef struct vaura_clip_sampling {
  int32_t use_sampling;
  float   temp;
  int32_t top_k;
  float   top_p;
  float   cfg_scale;      /* > 1: this clip mixes in its null-condition row.  <= 1 inside a call that carries those rows: no mix at all —
                             the row is not read, no lu + (x - lu) * 1, near-tie factor 1: the bits of a cfg_scale <= 1 call */
  int32_t reserved[3];    /* 0 */
} vaura_clip_sampling;

/* ---- everything one decode step touches.  All buffers are owned by the caller (torch tensors). */
#define VAURA_STATUS_NONFINITE_LOGITS 1
#define VAURA_STATUS_HANDOFF_TIMEOUT 2    /* a consumer of the one-launch MLP (csrc/mlp_engine.h) gave up waiting for its producers */
#define VAURA_STATUS_NEAR_TIE 4           /* informational: >= 1 used decision of the sampler was inside the arithmetic's noise (vaura_sampling.tie_eps) */

typedef struct vaura_decoder {
  vaura_dims dims;
  int32_t wdtype;          /* vaura_wdtype of the streamed matrices                */
  int32_t batch;           /* B  = clips                                           */
  int32_t rows;            /* Bs = B, or 2B when cfg_scale > 1                     */
  int32_t max_len;         /* KV capacity in positions (>= S)                      */
  int32_t timesteps;       /* T  = max_new_tokens                                  */
  int32_t seq_len;         /* S  = T + max(delay) + 1 (T + n_codebooks for the default pattern) */
  int32_t n_cond_tokens;   /* Tv                                                   */
  int32_t prefill_positions; /* > 0: every ws_* buffer holds this many positions' worth of row blocks, so a
                                prompt is teacher-forced in chunks of that many positions per pass (bf16 path) */
  int32_t plane_shift;     /* S in [0, 24], pair path only (0 otherwise): the two activation plane sets that have no RMSNorm in front of
                              them — the attention output (ws_attn_split) and silu(w1 x) * (w3 x) (ws_ffn_split) — are stored times
                              2^-S, and the caller packed wo and w2 times 2^S (vaura_pack_weight of the scaled matrix: the row scales
                              are powers of two, so the tiles are the same bits).  Exact in both directions unless a plane value drops
                              into fp16's subnormals; buys 2^S of head-room before |activation| > 65504 raises
                              VAURA_STATUS_NONFINITE_LOGITS.  0 = the layout every parity number was taken on */
  int32_t kv_dtype;        /* 0: the K / V cache is fp32 (every parity number).  1 (round 6; the low-precision serving configuration, BASELINE
                              configs[4]): fp16 — kcache / vcache then point at (n_layer, rows, n_head, max_len, head_dim) HALVES holding
                              fp16(rotated k) / fp16(v); caches of at most 256 positions only (VAURA_ERR_SHAPE otherwise, from the descriptor check and from
                              the decode-step and prefill attention launchers alike); tolerance reported.
                              2: OCP e4m3 bytes of the same layout (unscaled, saturating at +-448): a quarter of the fp32 stream, ~1e-2 class.
                              3: scaled e4m3 — the bytes of 2 plus ONE E8M0 exponent byte per cached 96-channel vector in kscale / vscale
                              (below; 97 bytes per vector).  x -> amax = max |x_c|; e = the smallest integer with amax 2^-e <= 448, clamped to
                              [-127, 127] (amax = 0: -127); byte c = e4m3(x_c 2^-e), round to nearest even; exponent byte = e + 127; widened
                              as float(byte) 2^e.  Nothing saturates and the grid follows each vector's own range; a vector holding an inf or
                              NaN gets exponent byte 0xFF and widens to NaN in every channel.  Same shapes as 1 and 2 */

  const vaura_layer_weights* layers_host; /* HOST array [n_layer] of device pointers */
  const void*  heads;        /* (n_codebooks*vocab x d_model) MFMA tiles (VAURA_W_H1 when wdtype is FP8) llama.py:356-361 */
  const float* final_norm;   /* (d_model)                                          llama.py:355 */
  const float* tok_emb;      /* (K, vocab+1, codebook_dim)                         llama.py:392-404 */
  const float* tok_proj_w;   /* (K, tok_dim, codebook_dim) weight-norm folded      llama.py:405-409 */
  const float* tok_proj_b;   /* (K, tok_dim)                                                */
  const float* tok_table;    /* (K, vocab+1, tok_dim) = vaura_build_token_table(tok_emb, tok_proj_w, tok_proj_b) */
  const float* empty_video;  /* (cond_dim)                                         llama.py:336-338 */
  const float* rope;         /* (max_len, head_dim/2, 2) cos,sin                   llama.py:593-603 */
  const float* cond_proj;    /* packed rows (rows*Tv x cond_dim): vaura_prefill_cond output */

  float*   kcache;           /* (n_layer, rows, n_head, max_len, head_dim) fp32 (fp16 when kv_dtype = 1), rotated keys */
  float*   vcache;           /* same shape                                          */
  int32_t* seq;              /* (B, K, S) pattern sequence, -1 = unknown            vaura_model.py:485-493 */
  int32_t* state;            /* 8 words: [0]=position of the token being fed, [1]=arrival counter, [2]=step index, [3] sequence id,
                                [4]=STATUS bits, sticky until the caller clears them (VAURA_STATUS_*): the sampler raises
                                VAURA_STATUS_NONFINITE_LOGITS when a logit it is about to sample from is inf / NaN — which is
                                where every overflow of the fp16-plane activation format ends up (|activation| > 65504 -> inf
                                in the hi plane -> NaN in the residual stream).  [5]=launch-epoch counter of the in-launch hand-offs,
                                OWNED BY THE LIBRARY: whatever ends a decode step (sampler, teacher-forced advance) bumps it and
                                nothing rewinds it.  A hand-off epoch is (state[3] sequence id, state[5], layer): rewinding [0]
                                inside a sequence is safe; a NEW sequence, a state buffer that starts from zero again, or another
                                decoder instance in the same process must come with a new sequence id in [3] (10 bits are
                                used) — the arrival words of the hand-offs live in LDS and outlive launches.  [6] = near-tie decisions counted
                                since the caller last zeroed it, [7] = step index + 1 of the first of them (vaura_sampling.tie_eps) */
  const float* noise;        /* optional (n_steps, B*K, vocab) Exp(1) draws; NULL -> Philox */

  float* ws_h;               /* packed rows (rows x d_model) residual stream        */
  float* ws_qkv;             /* packed rows (rows x 3*d_model)                      */
  float* ws_qkv2;            /* optional, same shape (one position's worth): on the pair path the decode step's qkv GEMV
                                then runs as two K-half workgroup sets (ws_qkv, ws_qkv2) that attention adds on load   */
  float* ws_attn;            /* packed rows (rows x d_model)                        */
  float* ws_ffn;             /* packed rows (rows x ffn_dim)                        */
  float* ws_logits;          /* row-major (rows, K*vocab)                           */
  /* pair path (wdtype H1 / H2 / FP8): activations as (hi, lo) fp16 planes ("split rows", 2 * rows_padded * C fp16, see
   * vaura_amd/csrc/gemv3_kernel.h) and per-tile partial sums of squares for the fused RMSNorm.  NULL with wdtype F32 / BF16
   * selects the exact-fp32-MFMA step                                                                              */
  uint16_t* ws_h_split;      /* split rows (rows x d_model) of h * next_norm_gain   */
  uint16_t* ws_attn_split;   /* split rows (rows x d_model)                         */
  uint16_t* ws_ffn_split;    /* split rows (rows x ffn_dim)                         */
  float*    ws_ss;           /* (row_blocks, d_model/16, 16)                        */
  const float* first_norm;   /* layers[0].attn_norm (device), gain applied by the embed kernel */
  float*    ws_attn_part;    /* optional (rows, n_head, 8, head_dim + 8): partials of the range-split attention used when
                                rows*n_head < 256 and max_len > 256 (vaura_attention_splits); NULL -> never split       */
  uint32_t* ws_sync;         /* optional 768 words (zeroed once by the caller): producer flags of the launches that hand activations over INSIDE the
                                launch (csrc/mlp_engine.h: w1||w3 -> w2 -> next layer's qkv; csrc/attention.hip: attention -> wo), each phase's weight
                                stream running ahead of its hand-off; words 512 .. 767: arrival counts of the range-split attention (the last split
                                of a (row, head) merges the partials inside the launch; left at zero).  NULL -> every GEMV, the attention and its
                                merge are separate launches */
  /* codebook delay pattern (codebook_patterns.py:374-419: DelayedPatternProvider with any sorted `delays`, ParallelPatternProvider =
   * all zeros): sequence step s >= 1 of codebook q holds timestep t = s - 1 - d_q, and seq_len = timesteps + max(d) + 1.
   * has_pattern_delays = 0 (a zero-filled descriptor): d_q = q, the default delayed pattern.  1: pattern_delays[0 .. K-1] hold the
   * delays — sorted, >= 0, K <= 16 (VAURA_ERR_ARG otherwise).  The sampler's valid-slot fix-up and its near-tie count follow them. */
  int32_t has_pattern_delays;
  int32_t pattern_delays[16];
  /* Bytes of extension that FOLLOW this struct in the caller's memory: 0 (a zero-filled descriptor: none), or
   * sizeof(vaura_decoder_ext) - sizeof(vaura_decoder) when `dec` is the first member of a vaura_decoder_ext (below), or
   * sizeof(vaura_decoder_ext2) - sizeof(vaura_decoder) when that in turn is the first member of a vaura_decoder_ext2, or
   * sizeof(vaura_decoder_ext3) - sizeof(vaura_decoder) when that is the first member of a vaura_decoder_ext3, or
   * sizeof(vaura_decoder_ext4) - sizeof(vaura_decoder) when that is the first member of a vaura_decoder_ext4; anything else is
   * VAURA_ERR_ARG.  It occupies what was alignment padding in front of `kscale`: no field moved and the struct keeps its size, so a
   * caller compiled against the descriptor without it (and zero-filling it, as every field's default asks) runs unchanged. */
  int32_t ext_bytes;
  /* kv_dtype = 3 only (NULL otherwise): the exponent bytes of the scaled e4m3 cache, (n_layer, rows, n_head, max_len) each;
   * VAURA_ERR_ARG when kv_dtype = 3 and either is NULL */
  uint8_t* kscale;
  uint8_t* vscale;
  /* Per-clip sampling parameters (NULL: the scalars of the call's vaura_sampling hold for every clip): `batch` records in device
   * memory.  With it, use_sampling / temp / top_k / top_p / cfg_scale of vaura_sampling are not read, except that the scalar
   * cfg_scale > 1 together with rows == 2 batch still states that the null-condition rows exist (set both when any clip's scale is
   * above 1); seed, clip_base, tie_eps keep their meaning.  It lives here, next to `noise`, and not in vaura_sampling: that struct
   * keeps its 48 bytes for callers compiled against it.  The sampler reads the records at every step, and a captured step graph
   * holds the POINTER: rewrite the records between calls and replay the same graph.  vaura_decode_step, vaura_generate_loop and
   * vaura_step_graph_build return VAURA_ERR_ARG for records together with input_is_probs = 1, and for a record with cfg_scale > 1
   * when rows != 2 batch or the scalar cfg_scale <= 1 (they read the records back: one small copy and a wait on the stream, per
   * call — vaura_generate_loop only when it launches eagerly, graph == NULL: replays of a built graph stay asynchronous; not while
   * the stream is being captured either.  Where nothing is read back the kernel clamps such a record to 1).  vaura_score ignores it. */
  const vaura_clip_sampling* clip_sampling;
  /* Token log-probabilities (NULL: none — the sampler instances every earlier caller runs, unchanged): fp32 (batch, K, seq_len), the
   * layout of `seq`.  Where the sampler's fix-up writes a SAMPLED token (a valid pattern slot that held -1) it writes, at the same
   * index, the log-probability of that token under the distribution the decision was made from:
   *     lp = log softmax(x / tau)[token] = (x[token] / tau - mx) - logf(den),  mx = max x / tau,  den = sum expf(x / tau - mx)
   * with x the CFG-mixed, sanitised logits of (clip, codebook) and tau = temp where the clip samples (use_sampling && temp > 0), 1
   * where it is greedy.  The softmax runs over the FULL vocabulary — the probability before any top-k / top-p truncation — so the
   * values compare across candidates, across sampling settings and with vaura_score.  In the sampled branch mx and den are the very
   * values the draw used.  Prompt, known and special slots are not written: the caller zeroes the buffer first.  On a (clip, codebook)
   * row that raised VAURA_STATUS_NONFINITE_LOGITS the value is NaN.  The token drawn never depends on this pointer.  A captured step
   * graph holds it like every other buffer.  VAURA_ERR_ARG together with input_is_probs = 1.  vaura_score ignores it. */
  float* logprobs;
} vaura_decoder;

/* vaura_decoder with the video-relevance pointers appended behind its last field.  Every entry point takes `&ext.dec`; the library
 * reads the two pointers only when ext.dec.ext_bytes says that they are there.
 * Video relevance of the sampled tokens (both NULL: none — the sampler instances above, unchanged; exactly one NULL: VAURA_ERR_ARG):
 * two fp32 buffers (batch, K, seq_len) in the layout of `seq`, written where `logprobs` is written (a sampled token in a valid slot
 * that held -1; the caller zeroes them first).  For the token chosen, its log-probability under the model's two distributions,
 *     logprobs_cond = (x_c[tok] - max x_c) - logf(sum expf(x_c - max x_c))     x_c = the conditional row of (clip, codebook)
 *     logprobs_null = (x_u[tok] - max x_u) - logf(sum expf(x_u - max x_u))     x_u = the null-condition row of the same prefix
 * full vocabulary, NO temperature and no CFG mix: relevance = logprobs_cond - logprobs_null, the pointwise mutual information of
 * token and video, does not depend on the sampling settings.  Reduction order per row: block maximum, then block sum (csrc/step.hip).
 * Needs the null-condition rows: rows == 2 batch and the scalar cfg_scale > 1 (VAURA_ERR_ARG otherwise, before any launch).  A clip
 * whose own scale is <= 1 is still drawn un-mixed; its null row is read for logprobs_null only.  NaN in both on a row that raised
 * VAURA_STATUS_NONFINITE_LOGITS — which these pointers also raise for a non-finite value in either of the two rows.  The token drawn
 * never depends on them.  A captured step graph holds them like `logprobs`.  VAURA_ERR_ARG with input_is_probs = 1.  vaura_score
 * ignores them. */
typedef struct vaura_decoder_ext {
  vaura_decoder dec;        /* dec.ext_bytes = sizeof(vaura_decoder_ext) - sizeof(vaura_decoder) */
  float* logprobs_cond;
  float* logprobs_null;
} vaura_decoder_ext;

/* vaura_decoder_ext with the per-clip lengths of a ragged batch appended behind it.  Every entry point takes `&ext2.ext.dec`; the
 * library reads the two pointers only when ext.dec.ext_bytes = sizeof(vaura_decoder_ext2) - sizeof(vaura_decoder).  Both are `batch`
 * int32 in device memory, and either may be NULL (every clip then has dec.timesteps / dec.n_cond_tokens, as without this struct):
 *   clip_timesteps    T_b, 1 <= T_b <= dec.timesteps.  Clip b ends after T_b frames: the sampler's fix-up, its log-probability /
 *                     relevance writes and its near-tie count treat a slot whose timestep is >= T_b as invalid (the special token,
 *                     nothing reported, nothing counted), exactly as the call with timesteps = T_b treats it.  dec.timesteps and
 *                     dec.seq_len stay those of the longest clip; a finished clip rides along to the end of the loop.
 *   clip_cond_tokens  Tv_b, 1 <= Tv_b <= dec.n_cond_tokens.  Only the first Tv_b video tokens of clip b are real: a position whose
 *                     frame pos / tokens_per_frame is >= Tv_b takes empty_video, in the decode step and in the prefill pass, for the
 *                     clip's conditional row b and its null-condition row batch + b.  The row stride of cond_proj stays
 *                     dec.n_cond_tokens; what it holds behind token Tv_b - 1 of a clip is never read.
 * The kernels read the arrays at every step, and a captured step graph holds the POINTERS: rewrite the values between calls and
 * replay the same graph.  vaura_decode_step, vaura_generate_loop, vaura_step_graph_build and vaura_embed return VAURA_ERR_ARG for a
 * value outside its range (they read the arrays back: one small copy and a wait on the stream — under the rules of
 * vaura_decoder.clip_sampling: not for replays of a built graph, not while the stream is being captured; where nothing is read back
 * the kernels clamp a value to its upper bound, so nothing is read out of bounds).  vaura_score / vaura_score_relevance obey both
 * arrays (see there: 2 <= T_b, scoring needs two timesteps). */
typedef struct vaura_decoder_ext2 {
  vaura_decoder_ext ext;    /* ext.dec.ext_bytes = sizeof(vaura_decoder_ext2) - sizeof(vaura_decoder) */
  const int32_t* clip_timesteps;
  const int32_t* clip_cond_tokens;
} vaura_decoder_ext2;

/* vaura_decoder_ext2 with the per-clip audio PROMPT lengths of a batch appended behind it.  Every entry point takes
 * `&ext3.ext2.ext.dec`; the library reads the pointer only when dec.ext_bytes = sizeof(vaura_decoder_ext3) - sizeof(vaura_decoder).
 *   row_prompt_steps  `rows` int32 in device memory, or NULL (every clip starts where the loop starts, as without this struct).
 *                     Entry r is n_r = P_b + delays[0] for the clip b = r % batch of row r: the number of teacher-forced positions of
 *                     that clip, i.e. the position of its first sampled step.  0 <= n_r <= seq_len - 1.
 * With it the sampler keys clip b's Philox counter by (position - n_b) instead of the loop's step index — the step index the call
 * with the common prompt of P_b frames has at that position — so a clip draws what it draws in that call wherever the loop of this
 * call started.  An explicit `noise` tensor and the near-tie detector's "first flagged step" keep the loop's step.  Nothing else of
 * the step changes: a row that is still inside its prompt holds known tokens in every slot the sampler visits, and the fix-up
 * writes (and reports, and counts) only where a slot still holds -1.
 * vaura_prefill_rows (below) reads the same array to append K / V for one group of rows.
 * A captured step graph holds the POINTER; the host-side range check follows the rules of clip_timesteps. */
typedef struct vaura_decoder_ext3 {
  vaura_decoder_ext2 ext2;  /* ext2.ext.dec.ext_bytes = sizeof(vaura_decoder_ext3) - sizeof(vaura_decoder) */
  const int32_t* row_prompt_steps;
} vaura_decoder_ext3;

/* vaura_decoder_ext3 with the attention-map request of a call appended behind it.  Every entry point takes `&ext4.ext3.ext2.ext.dec`;
 * the library reads the fields only when dec.ext_bytes = sizeof(vaura_decoder_ext4) - sizeof(vaura_decoder) (64).
 *   attn_probs  NULL: no maps — every layer launches the attention instance it always launched.  Otherwise fp32
 *               (attn_steps, attn_rows, n_head, max_len) in device memory, zeroed by the caller: the decode step at cache position pos
 *               (the cache holds [0, pos), the new position is key pos) writes, for layer attn_layer, row r < attn_rows and head h, the
 *               softmax weights p[j] = softmax_j(q . k_j / sqrt(96)), j = 0 .. pos, to
 *                   attn_probs[((pos - attn_pos0) * attn_rows + r) * n_head + h][0 .. pos]
 *               and nothing behind them.  They are the numbers the kernel's output is formed from — expf(s_j - m_wave) *
 *               expf(m_wave - M) * (1 / denom) for a cached key, expf(s_new - M) * (1 / denom) for the new one (csrc/attention.hip) — on
 *               the fp32 scores of the keys AS STORED (widened fp16 / e4m3; the scaled e4m3 score carries the key's 2^e).  A step with
 *               pos outside [attn_pos0, attn_pos0 + attn_steps) — the teacher-forced positions in front of the loop — and rows >=
 *               attn_rows (the null-condition rows) write nothing.  The step's output, cache appends and tokens never depend on it.
 * Served by the single-round-trip step kernel only: max_len <= 256 (VAURA_ERR_SHAPE otherwise).  VAURA_ERR_ARG, with attn_probs set:
 * attn_layer outside [0, n_layer), attn_rows outside [1, rows], attn_steps < 1, attn_pos0 < 0.  All before any launch.  A captured step
 * graph holds the pointer and the four values. */
typedef struct vaura_decoder_ext4 {
  vaura_decoder_ext3 ext3;  /* ext3.ext2.ext.dec.ext_bytes = sizeof(vaura_decoder_ext4) - sizeof(vaura_decoder) */
  float* attn_probs;
  int32_t attn_layer, attn_pos0, attn_steps, attn_rows;
} vaura_decoder_ext4;

/* -------------------------------------------------------------------------------------------
 * Weight ingress (once, at load).  Replaces nn.Module.load_state_dict for the streamed matrices.
 * src: row-major fp32 (N x K) as stored in the reference checkpoint (nn.Linear.weight).          */
int vaura_pack_weight(const float* src, void* dst, int64_t N, int64_t K, int wdtype, vaura_stream_t s);
size_t vaura_packed_weight_bytes(int64_t N, int64_t K, int wdtype);

/* a4 DacEmbeddingProjection (llama.py:60-73) evaluated once for every (codebook, token):
 * table[k][tok][c] = sum_i w[k][c][i] * emb[k][tok][i] + b[k][c]   (K, vocab+1, tok_dim) fp32   */
int vaura_build_token_table(const float* tok_emb, const float* proj_w, const float* proj_b, float* table, int K,
                            int vocab1, int cdim, int tok_dim, vaura_stream_t s);

/* row-major (rows x C) fp32 <-> packed rows.  `rows_padded` = ceil(rows/16)*16 rows are written.   */
int vaura_pack_rows(const float* src, float* dst, int64_t rows, int64_t C, vaura_stream_t s);
int vaura_unpack_rows(const float* src, float* dst, int64_t rows, int64_t C, vaura_stream_t s);

/* -------------------------------------------------------------------------------------------
 * a5  AVCLIPEmbedder.forward / MLP (llama.py:79-92,136-141): fc2(gelu_tanh(fc1(x))), hoisted to
 * once per clip.  feats: packed rows (n_rows x 768); tmp: packed rows (n_rows x cond_dim);
 * out: packed rows (n_rows x cond_dim).  fc1/fc2: MFMA tiles, wdtype as given.                   */
int vaura_prefill_cond(const vaura_dims* d, const float* feats, const void* fc1, const void* fc2, int wdtype,
                       float* tmp, float* out, int64_t n_rows, vaura_stream_t s);

/* The condition buffer of a live session, updated in place (dec->cond_proj is baked into a captured step graph; row index
 * row * Tv + token, Tv = dec->n_cond_tokens).  ONE launch, for every decoder row:
 *   conditional rows [0, batch): tokens [shift_tokens, Tv) move down to [0, Tv - shift_tokens) (0: nothing moves), then tokens
 *     [first_token, first_token + n_tokens) are taken from new_rows — packed rows (batch * n_tokens x cond_dim), row index
 *     b * n_tokens + t: the output of vaura_prefill_cond on the clips' n_tokens fresh feature rows;
 *   null-condition rows [batch, 2 batch) (dec->rows == 2 dec->batch): nothing moves — the null embedding belongs to the window
 *     position —, tokens [first_token, first_token + n_tokens) are taken from null_rows, packed rows (Tv x cond_dim), row index =
 *     token: the projected null embedding, one copy for every clip.  Ignored (may be NULL) without those rows.
 * Tokens outside both ranges keep what they hold.  One work item per (row, 4-column quad) walks the tokens in ascending order and
 * reads token j + shift before it writes token j; items touch disjoint addresses.
 * VAURA_ERR_ARG: dec, dec->cond_proj or new_rows NULL, null_rows NULL with the null rows present, rows neither batch nor 2 batch, a
 * negative shift_tokens / first_token, n_tokens <= 0; VAURA_ERR_SHAPE: shift_tokens > Tv, first_token + n_tokens > Tv, cond_dim % 4.   */
int vaura_cond_window(const vaura_decoder* dec, const float* new_rows, const float* null_rows, int shift_tokens, int first_token,
                      int n_tokens, vaura_stream_t s);

/* -------------------------------------------------------------------------------------------
 * a14 Pattern.build_pattern_sequence (codebook_patterns.py:180-207) for DelayedPatternProvider
 * (:390-406).  codes (B,K,T) int32 with -1 = unknown -> seq (B,K,T+K); special = d_codebook.     */
int vaura_pattern_build(const int32_t* codes, int32_t* seq, int B, int K, int T, int special, vaura_stream_t s);
/* a14 Pattern.revert_pattern_sequence (codebook_patterns.py:260-285) + the [..., :T] slice
 * (vaura_model.py:568-569).  seq (B,K,S) -> codes (B,K,T); positions with no source get `fill`.  */
int vaura_pattern_revert(const int32_t* seq, int32_t* codes, int B, int K, int T, int S, int fill, vaura_stream_t s);
/* The same two for any delay pattern (codebook_patterns.py:374-419): delays_host = K ints, sorted, >= 0, K <= 16 (VAURA_ERR_ARG
 * otherwise).  build: S must be T + max(d) + 1 (VAURA_ERR_SHAPE otherwise); revert: any 0 < S <= T + max(d) + 1.  The two
 * entry points above are these with d_q = q.                                                     */
int vaura_pattern_build_delays(const int32_t* codes, int32_t* seq, int B, int K, int T, int S, int special,
                               const int32_t* delays_host, vaura_stream_t s);
int vaura_pattern_revert_delays(const int32_t* seq, int32_t* codes, int B, int K, int T, int S, int fill,
                                const int32_t* delays_host, vaura_stream_t s);

/* -------------------------------------------------------------------------------------------
 * a2/a13/a15  logits (rows, K*vocab) -> next tokens.  Standalone form of the sampler used inside
 * vaura_decode_step (same kernel).  noise: (B*K, vocab) Exp(1) draws or NULL (Philox, step index
 * `step`).  tokens_out (B,K) int32.                                                              */
int vaura_sample(const float* logits, int B, int K, int vocab, const vaura_sampling* sp, const float* noise,
                 int64_t step, int32_t* tokens_out, vaura_stream_t s);

/* vaura_sample with per-clip records (B of them, device memory; see vaura_decoder.clip_sampling): clip b is sampled with record b, and
 * the result equals, clip by clip, vaura_sample with that clip's parameters.  sp->cfg_scale > 1 states that logits has 2B rows.
 * seq == NULL: tokens_out (B,K) as vaura_sample.  seq != NULL: the sampler as the decode step runs it, on the caller's logits — seq
 * (B,K,S) pattern sequence (default delays) and `state` (8 words, vaura_decoder.state) are required, position and step index come
 * from state[0] / state[2] (`step` is not read), the slot state[0] + 1 is filled where it holds -1, the status bits and near-tie
 * counters are raised and the state advances; tokens_out may be NULL.
 * VAURA_ERR_ARG: clips == NULL, input_is_probs = 1, a record with cfg_scale > 1 while sp->cfg_scale <= 1.                        */
int vaura_sample_clips(const float* logits, int B, int K, int vocab, const vaura_sampling* sp, const vaura_clip_sampling* clips,
                       const float* noise, int64_t step, int32_t* tokens_out, int32_t* seq, int T, int S, int32_t* state,
                       vaura_stream_t s);

/* vaura_sample_clips (clips == NULL: the scalars of sp, i.e. vaura_sample; seq / T / S / state as there, NULL seq = the standalone
 * form) that also reports the log-probability of every token drawn: logprobs_out (B, K) fp32, defined at vaura_decoder.logprobs
 * (written for every (clip, codebook), whatever the slot held).  The tokens equal what vaura_sample / vaura_sample_clips return for
 * the same inputs.  VAURA_ERR_ARG: input_is_probs = 1 (rows that already are probabilities have no log-probability to report), a
 * NULL logprobs_out, and what vaura_sample_clips refuses.                                                                          */
int vaura_sample_logprobs(const float* logits, int B, int K, int vocab, const vaura_sampling* sp, const vaura_clip_sampling* clips,
                          const float* noise, int64_t step, int32_t* tokens_out, int32_t* seq, int T, int S, int32_t* state,
                          float* logprobs_out, vaura_stream_t s);
/* vaura_sample_logprobs that also reports the video relevance of every token drawn (vaura_decoder_ext.logprobs_cond / logprobs_null):
 * cond_out, null_out (B, K) fp32 = the token's log-probability under the conditional row and under the null row, tau = 1, full
 * vocabulary.  logits has 2B rows and sp->cfg_scale > 1 says so (scalar form: the clips are mixed with that scale; per-clip form: a
 * record with cfg_scale <= 1 draws un-mixed and its null row is read for null_out only).  logprobs_out may be NULL.  Tokens and
 * logprobs_out equal what vaura_sample_logprobs returns for the same inputs.  VAURA_ERR_ARG: sp->cfg_scale <= 1 (no null rows), a NULL
 * cond_out or null_out, and what vaura_sample_logprobs refuses.                                                                    */
int vaura_sample_relevance(const float* logits, int B, int K, int vocab, const vaura_sampling* sp, const vaura_clip_sampling* clips,
                           const float* noise, int64_t step, int32_t* tokens_out, int32_t* seq, int T, int S, int32_t* state,
                           float* logprobs_out, float* cond_out, float* null_out, vaura_stream_t s);
/* float twin of vaura_pattern_revert_delays: seq (B,K,S) fp32 -> out (B,K,T), frame t of codebook q from step t + 1 + d_q, `fill`
 * where S ends before it.  delays_host == NULL: d_q = q.                                                                           */
int vaura_pattern_revert_delays_f32(const float* seq, float* out, int B, int K, int T, int S, float fill, const int32_t* delays_host,
                                    vaura_stream_t s);
/* Sequence scores from token log-probabilities in the layout of seq (vaura_decoder.logprobs): logprobs (B, K, seq_len), seq_len =
 * T + max(d) + 1 (VAURA_ERR_SHAPE otherwise; delays_host NULL: d_q = q), K <= 16.  per_codebook (B, K) = mean over frames t0 .. T - 1
 * (t0 = prompt frames, excluded) of codebook q, per_clip (B) = mean of those K means.  Fixed summation order (one wave per codebook:
 * lane l adds frames t0 + l, t0 + l + 64, ..; lanes are added pairwise at distance 1, 2, 4, .. 32; the K means in codebook order):
 * two runs give the same bits.  A NaN anywhere in a clip makes per_clip AND all K per_codebook values of that clip NaN.            */
int vaura_sequence_logprob(const float* logprobs, int seq_len, const int32_t* delays_host, int B, int K, int T, int t0,
                           float* per_codebook, float* per_clip, vaura_stream_t s);
/* Best-of-N selection: scores (B * N), candidate j of clip b at b * N + j; codes (B * N, K, T) -> codes_out (B, K, T) = the codes of
 * the candidate with the largest score, winner (B) its index j.  The first index wins a tie; a NaN never beats a number; when every
 * score of a clip is NaN, candidate 0 wins.                                                                                        */
int vaura_select_candidates(const float* scores, const int32_t* codes, int B, int N, int K, int T, int32_t* codes_out, int32_t* winner,
                            vaura_stream_t s);

/* ---- per-clip lengths (vaura_decoder_ext2): the kernels above with T_b = clip_timesteps[b] (B int32, device memory) in place of T.
 * T stays the longest length (the row stride of codes / out, and S = T + max(d) + 1); delays_host NULL: d_q = q.  Each result equals,
 * clip by clip and over frames [0, T_b), what the entry point above gives for T = T_b.  VAURA_ERR_ARG: a NULL clip_timesteps, a value
 * outside 1 .. T (the values are read back: one small copy and a wait on the stream), and what the scalar form refuses.
 * build:  seq[b, q, s] = codes[b, q, t] for 0 <= t = s - 1 - d_q < T_b, else `special`.
 * revert: out[b, q, t] = seq[b, q, t + 1 + d_q] for t < T_b (`fill` where S ends before it), `pad` for t >= T_b.
 * sequence_logprob: the means run over frames t0 .. T_b - 1 of each clip (t0 < T_b for every clip), same order, same NaN rule.      */
int vaura_pattern_build_clips(const int32_t* codes, int32_t* seq, int B, int K, int T, int S, int special, const int32_t* delays_host,
                              const int32_t* clip_timesteps, vaura_stream_t s);
int vaura_pattern_revert_clips(const int32_t* seq, int32_t* codes, int B, int K, int T, int S, int fill, int pad,
                               const int32_t* delays_host, const int32_t* clip_timesteps, vaura_stream_t s);
int vaura_pattern_revert_clips_f32(const float* seq, float* out, int B, int K, int T, int S, float fill, float pad,
                                   const int32_t* delays_host, const int32_t* clip_timesteps, vaura_stream_t s);
int vaura_sequence_logprob_clips(const float* logprobs, int seq_len, const int32_t* delays_host, int B, int K, int T, int t0,
                                 const int32_t* clip_timesteps, float* per_codebook, float* per_clip, vaura_stream_t s);
/* The sampler exactly as the decode step runs it, on the caller's logits, with every option of the loop: seq (B, K, S) and `state` are
 * required (position state[0], step state[2]; the slot state[0] + 1 is filled where it holds -1; status bits and near-tie counters are
 * raised; the state advances).  clips: per-clip records or NULL; delays_host: K delays or NULL (d_q = q); clip_timesteps: B lengths
 * or NULL (every clip has T); lp_seq / cond_seq / null_seq: (B, K, S) fp32 in the layout of seq or NULL (vaura_decoder.logprobs,
 * vaura_decoder_ext.logprobs_cond / logprobs_null: cond_seq and null_seq together, with 2B rows of logits and sp->cfg_scale > 1).   */
int vaura_sample_seq(const float* logits, int B, int K, int vocab, const vaura_sampling* sp, const vaura_clip_sampling* clips,
                     const float* noise, int32_t* seq, int T, int S, int32_t* state, const int32_t* delays_host,
                     const int32_t* clip_timesteps, float* lp_seq, float* cond_seq, float* null_seq, vaura_stream_t s);
/* vaura_sample_seq with per-clip first sampled positions (vaura_decoder_ext3.row_prompt_steps; clip_first_steps: B int32 in device
 * memory, 0 <= n_b <= S - 1): clip b's Philox counter step is state[0] - n_b instead of state[2].  Clip by clip the result equals
 * vaura_sample_seq on a state whose step index state[2] is state[0] - n_b.  An explicit noise keeps state[2].  VAURA_ERR_ARG: a NULL
 * clip_first_steps, a value out of range (read back: one small copy and a wait on the stream), and what vaura_sample_seq refuses. */
int vaura_sample_seq_starts(const float* logits, int B, int K, int vocab, const vaura_sampling* sp, const vaura_clip_sampling* clips,
                            const float* noise, int32_t* seq, int T, int S, int32_t* state, const int32_t* delays_host,
                            const int32_t* clip_timesteps, const int32_t* clip_first_steps, float* lp_seq, float* cond_seq,
                            float* null_seq, vaura_stream_t s);
/* vaura_sequence_logprob / vaura_sequence_logprob_clips with a per-clip first frame: the means of clip b run over frames
 * clip_t0[b] .. T_b - 1 (clip_t0: B int32 in device memory; clip_timesteps: B lengths or NULL, every clip then has T).  Clip by clip
 * the bits of those entries called with t0 = clip_t0[b].  VAURA_ERR_ARG: a NULL clip_t0, a value outside 0 .. T_b - 1 (both arrays
 * are read back), and what the scalar forms refuse. */
int vaura_sequence_logprob_starts(const float* logprobs, int seq_len, const int32_t* delays_host, int B, int K, int T,
                                  const int32_t* clip_t0, const int32_t* clip_timesteps, float* per_codebook, float* per_clip,
                                  vaura_stream_t s);
/* The input embedding of the decode step (pos_host < 0, n_pos = 1: the position is state[0]) or of n_pos prefill positions from
 * pos_host on, alone: dec->ws_h (packed rows; prefill: one block of rows_padded rows per position) and, on the plane storages, the
 * planes and sums of squares behind it.  Obeys vaura_decoder_ext2.clip_cond_tokens.  Nothing advances.  Every token of dec->seq at the
 * embedded positions must be known (0 .. vocab): the kernel gathers table rows by token, as in the loop, where the sampler has filled
 * a slot before the step that embeds it — a slot that still holds -1 is the caller's error and is not checked.                              */
int vaura_embed(const vaura_decoder* dec, int pos_host, int n_pos, vaura_stream_t s);

/* -------------------------------------------------------------------------------------------
 * a3..a12 + a2/a13/a15 for ONE position: Transformer.inference (llama.py:445-504) restricted to the
 * position state[0] with a K/V cache, followed by _sample_next_token and the fix-up
 * (vaura_model.py:536-544) that writes seq[..., state[0]+1] and advances state.
 * sample == 0: teacher-forced step (prompt prefill): no heads, no sampling, state still advances. */
int vaura_decode_step(const vaura_decoder* dec, const vaura_sampling* sp, int sample, vaura_stream_t s);

/* a1  the hot loop of VAURAModel.generate (vaura_model.py:502-547): `n_prefill` teacher-forced
 * positions then `n_steps` sampled ones, all enqueued back-to-back.  graph != NULL replays a captured single-step
 * hipGraph per position (the position lives in dec->state); NULL launches every kernel eagerly.
 * vaura_step_graph_build captures one step of (dec, sp) on `s` (not the legacy null stream) into a handle the caller
 * owns: it is valid for exactly the buffers / shapes / sampling parameters it was built from.  The loop replays the step
 * `m` at a time where at least m steps remain (one graph launch per m steps; m = 4, or the GRAPH_STEPS field of vaura_set_debug_flags
 * at build time, 1..16): that longer graph is captured — same (dec, sp), on `s` — by the first vaura_generate_loop call with
 * n_steps >= m, so that call must use the dec / sp the handle was built from (it always must).  No process environment is read. */
typedef void* vaura_step_graph_t;
int vaura_generate_loop(const vaura_decoder* dec, const vaura_sampling* sp, int n_prefill, int n_steps,
                        vaura_step_graph_t graph, vaura_stream_t s);
int vaura_step_graph_build(const vaura_decoder* dec, const vaura_sampling* sp, vaura_stream_t s, vaura_step_graph_t* out);
/* The prefill pass of ONE group of rows of a call with per-clip prompt lengths (vaura_decoder_ext3.row_prompt_steps), on the plane
 * storages (prefill_positions > 0): exactly the chunk sequence vaura_generate_loop runs for n_prefill teacher-forced positions — from
 * position 0, in chunks of prefill_positions, every row computed, so every launch is the instance that call picks — except that K / V
 * (and the exponent bytes of kv_dtype 3) are appended only to the rows r with row_prompt_steps[r] == n_sel; the cache rows of every
 * other row keep their bytes.  It neither reads nor advances `state`: the caller runs it between two vaura_generate_loop calls, just
 * before the step at position n_sel.  Every token of dec->seq at positions [0, n_prefill) must be known for EVERY row (the embedding
 * gathers by token and does not clamp): that holds at that moment, and not earlier.
 * VAURA_ERR_ARG, before any launch: a descriptor without the array or without prefill workspaces, n_sel outside 1 .. seq_len - 1,
 * n_prefill outside 1 .. n_sel, a value of the array outside 0 .. seq_len - 1 (the array is read back: one small copy and a wait on
 * the stream). */
int vaura_prefill_rows(const vaura_decoder* dec, int n_prefill, int n_sel, vaura_stream_t s);
void vaura_step_graph_free(vaura_step_graph_t graph);

/* Measurement aid (bench.py): runs `n_steps` sampled steps eagerly on `s` with a hipEvent pair
 * around every launch of the kernel kinds selected by `kind_mask` (bit = vaura_kernel_kind), then
 * synchronises `s` and reports, per kind, the summed elapsed ms and the launch count (HOST arrays of
 * VAURA_K_COUNT entries).  A stage that is several launches (range-split attention) reports the sum of
 * its launches per stage.  The only entry point that creates events / synchronises.              */
typedef enum vaura_kernel_kind {
  VAURA_K_EMBED = 0, VAURA_K_QKV = 1, VAURA_K_ATTN = 2, VAURA_K_WO = 3, VAURA_K_W13 = 4, VAURA_K_W2 = 5,
  VAURA_K_HEADS = 6, VAURA_K_SAMPLE = 7, VAURA_K_COUNT = 8
} vaura_kernel_kind;
int vaura_profile_loop(const vaura_decoder* dec, const vaura_sampling* sp, int n_steps, unsigned kind_mask,
                       double* total_ms_host, int64_t* launches_host, vaura_stream_t s);
/* Launches of the calling thread's last vaura_profile_loop whose interval exceeded 10x their kind's median (a stalled queue, not
 * the kernel): they were counted at the median in total_ms_host; per kind, HOST array of VAURA_K_COUNT entries.               */
void vaura_profile_outliers(int64_t* per_kind);

/* -------------------------------------------------------------------------------------------
 * Teacher-forced scoring: VAURAModel.forward + _compute_loss (models/vaura_model.py:136-192, 240-280; test_step 339-347).
 * dec->seq holds the pattern sequence of the given codes (build_pattern_sequence(codes[..., :-1]) against a pattern of
 * dec->timesteps = Ta steps: vaura_pattern_build_delays of the codes with timestep Ta - 1 set to the special token), state zeroed,
 * dec->rows == dec->batch (no CFG branch).  Positions [0, n_pos) are run, n_pos <= seq_len - 1 and <= max_len (VAURA_ERR_ARG);
 * model-output position s of codebook q predicts timestep t = s - d_q, target targets[b, q, t] ((B, K, Ta) int32).
 *   plane storages with prefill workspaces: chunks of dec->prefill_positions positions through the prefill kernels, the heads
 *     (final RMSNorm fused) over every position of the chunk into ws_chunk_logits (prefill_positions * rows_padded * K * vocab
 *     floats), then the NLL kernel on the chunk;
 *   otherwise (VAURA_W_F32 / BF16): one decode step with heads per position (ws_logits), then the NLL kernel — the exact-fp32
 *     answer; ws_chunk_logits may be NULL.  The step's sampler leaves its status bits in state[4] as in the decode loop.
 * Outputs: nll (B, K, Ta) = logsumexp - target logit in fp32; mask_out (B, K, Ta) bytes (optional; 1 where t + d_q < n_pos, i.e.
 * all of them when n_pos = seq_len - 1 — delay patterns leave no timestep without a logit); logits_out (optional) the reverted
 * (B, K, Ta, vocab) logits, NaN rows where the mask is 0 (revert_pattern_logits' fill); loss_per_cb (K) = mean of the valid nll
 * of codebook q, loss (1) = sum_q loss_per_cb[q] / K.  Summation order is fixed: two calls give the same bits.
 * Per-clip lengths (the design chosen: this entry point and vaura_score_relevance are length-aware; there is no separate per-clip entry
 * point, and the per-clip means are one more call, below).  With vaura_decoder_ext2.clip_timesteps clip b holds Ta_b = clip_timesteps[b]
 * timesteps, 2 <= Ta_b <= dec->timesteps; dec->seq is vaura_pattern_build_clips of the codes with the special token from timestep
 * Ta_b - 1 on (build_pattern_sequence(codes_b[..., :Ta_b - 1]) against a pattern of Ta_b steps), n_pos the positions of the longest
 * clip.  An entry is valid iff t < Ta_b and t + d_q < n_pos: invalid entries get nll NaN, mask 0 and a NaN row of logits_out;
 * loss_per_cb[q] is the mean over all valid (b, t) in the same fixed order (_compute_loss under the mask t < Ta_b), loss the mean of
 * those.  targets behind Ta_b are not read.  Attention is causal, so clip b's valid entries are what the call on the clip alone gives;
 * the rows of a finished clip are computed and ignored.  With clip_cond_tokens the embed of either path takes Tv_b as in the decode
 * loop.  Both arrays are read back and range-checked once (one small copy and a wait on the stream; not while the stream is being
 * captured), before any launch: VAURA_ERR_ARG for a value outside its range.  Both NULL: the launches and the bits of the call
 * without the extension.
 * Per-clip means: vaura_sequence_logprob_clips(lay, Ta + 1, zero delays, B, K, Ta, 0, clip_timesteps, per_codebook, per_clip) on
 * lay (B, K, Ta + 1) = one unused leading step followed by nll — per_codebook (B, K) the mean of clip b's codebook q over t < Ta_b,
 * per_clip (B) the mean of those over the codebooks, the loss clip b gets scored alone; fixed order, the entries behind Ta_b unread. */
int vaura_score(const vaura_decoder* dec, int n_pos, const int32_t* targets, float* ws_chunk_logits, float* logits_out, float* nll,
                uint8_t* mask_out, float* loss_per_cb, float* loss, vaura_stream_t s);
/* vaura_score on a descriptor with the null-condition rows (dec->rows == 2 dec->batch; VAURA_ERR_ARG otherwise): the given codes are
 * prefilled under the video (rows [0, B)) and under the null condition (rows [B, 2B)) in one pass, the NLL kernel runs on both row sets
 * and the reduction on both nll tensors.  nll / loss_per_cb / loss as vaura_score; nll_null (B, K, Ta), loss_per_cb_null (K),
 * loss_null (1) the same quantities of the null rows (same mask, same fixed order).  nll_null - nll is how much the video explains
 * of every given token.                                                                                                            */
int vaura_score_relevance(const vaura_decoder* dec, int n_pos, const int32_t* targets, float* ws_chunk_logits, float* logits_out, float* nll,
                          uint8_t* mask_out, float* loss_per_cb, float* loss, float* nll_null, float* loss_per_cb_null, float* loss_null,
                          vaura_stream_t s);
/* _compute_loss on a given reverted logits tensor (B, K, Ta, vocab) fp32, targets (B, K, Ta) int32, mask (B, K, Ta) bytes: the same
 * NLL and reduction kernels (vocab % 256 == 0, <= 1024; K <= 16).  nll (B, K, Ta) is scratch + output (entries where mask is 0 are
 * not meaningful).                                                                                                                */
int vaura_score_logits(const float* logits, const int32_t* targets, const uint8_t* mask, int B, int K, int V, int Ta, float* nll,
                       float* loss_per_cb, float* loss, vaura_stream_t s);

/* -------------------------------------------------------------------------------------------
 * op-level entry points (parity tests call the same kernels the step uses)                      */
/* out = epilogue( W x (x*gain) * rinv ):  epi 0 store, 1 +residual, 2 SwiGLU pairs, 3 gelu_tanh,
 * 4 row-major logits.  K must be one of the compiled depths (512, 768, 1024, 1536, 4096).        */
int vaura_gemv(const void* w, int wdtype, const float* x, const float* gain, const float* residual, float* out,
               int64_t rows, int64_t N, int64_t K, int epilogue, float eps, vaura_stream_t s);
/* pair form of vaura_gemv: x as (hi, lo) fp16 planes ("split rows"), weights as fp16 plane(s) or fp8, products on
 * v_mfma_f32_16x16x32_f16.  ss_in (row_blocks, n_ss_in, 16): partial sums of squares of the raw input
 * (fused RMSNorm) or NULL.  Optional outputs: fp32 packed rows, split rows of out*gain_out, partial
 * sums of squares of out.  epilogue: 0 store, 1 +residual, 2 SwiGLU pairs, 4 row-major logits.       */
int vaura_gemv_pair(const void* w, int wdtype /* H1 | H2 | FP8 */, const uint16_t* x_split, const float* ss_in, int n_ss_in, const float* residual, float* out,
                    float* out_khalf2 /* NULL, or (K = 1536, fused norm, store): `out` gets the partial over the first half
                                         of K and this buffer the second half's; the consumer adds them */,
                    uint16_t* out_split, const float* gain_out, float* ss_out, int64_t rows, int64_t N, int64_t K, int epilogue,
                    float eps, vaura_stream_t s);
/* packed rows (rows x C) fp32 [* gain] -> split rows (2 * rows_padded * C fp16: hi plane, lo plane) [+ partial sums of squares] */
int vaura_split_rows(const float* src, uint16_t* dst, const float* gain, float* ss, int64_t rows, int64_t C, vaura_stream_t s);

/* a8/a9 for one layer at position `pos` (host value): rope(q,k), append, softmax(qK^T/sqrt(hd)) V. */
int vaura_attention_step(const float* qkv, const float* rope, float* kcache, float* vcache, float* out,
                         int rows, int n_head, int head_dim, int max_len, int pos, vaura_stream_t s);

/* same step with the cached range of every (row, head) split over n_split (2..8) workgroups + a combine
 * pass; part: (rows, n_head, n_split, head_dim + 8) floats of scratch.                              */
int vaura_attention_step_split(const float* qkv, const float* rope, float* kcache, float* vcache, float* out, float* part,
                               int rows, int n_head, int head_dim, int max_len, int pos, int n_split, vaura_stream_t s);
/* workgroups per (row, head) the decode step uses for this shape when ws_attn_part is given (1 = no split) */
int vaura_attention_splits(int rows, int n_head, int max_len);
/* Op-level access for parity tests: ONE decode-step attention with every optional the step passes, through the step's own launcher.
 * qkv2 (NULL ok): the second K-half partial of a split qkv GEMV, added to qkv on load.  out_split (NULL ok): split rows (hi, lo fp16 planes)
 * of out * 2^-plane_shift; the fp32 `out` is never scaled.  n_split 1..8: > 1 splits the cached range like vaura_attention_step_split
 * (`part` as there); with `arrivals` (rows * n_head zeroed words; left at zero) the last split to arrive merges inside the launch, with
 * NULL a combine launch follows.  kv_dtype as vaura_decoder.kv_dtype: kcache / vcache hold fp32, fp16 or e4m3 elements;
 * the narrow caches take max_len <= 256 and no split (VAURA_ERR_SHAPE otherwise, nothing is launched).                              */
int vaura_attention_step_ex(const float* qkv, const float* qkv2, const float* rope, float* kcache, float* vcache, float* out,
                            uint16_t* out_split, float* part, uint32_t* arrivals, int rows, int n_head, int head_dim, int max_len,
                            int pos, int n_split, int plane_shift, int kv_dtype, vaura_stream_t s);
/* vaura_attention_step_ex for every K / V storage: kv_dtype 0..3, with kscale / vscale (rows, n_head, max_len) the exponent bytes of the
 * scaled e4m3 cache (kv_dtype = 3: VAURA_ERR_ARG when either is NULL; ignored for 0..2).  vaura_attention_step_ex itself keeps refusing
 * kv_dtype = 3 (VAURA_ERR_ARG): it has nowhere to take them.  Storage 3 takes max_len <= 256 and no split, like 1 and 2.             */
int vaura_attention_step_kv(const float* qkv, const float* qkv2, const float* rope, float* kcache, float* vcache, uint8_t* kscale,
                            uint8_t* vscale, float* out, uint16_t* out_split, float* part, uint32_t* arrivals, int rows, int n_head,
                            int head_dim, int max_len, int pos, int n_split, int plane_shift, int kv_dtype, vaura_stream_t s);
/* vaura_attention_step_kv that also reports the softmax weights of the step (vaura_decoder_ext4.attn_probs, through the same launcher):
 * probs fp32 (n_steps, rows_out, n_head, max_len); the call at `pos` writes probs[((pos - pos0) * rows_out + r) * n_head + h][0 .. pos]
 * for rows r < rows_out when pos0 <= pos < pos0 + n_steps, and nothing otherwise.  out, out_split and the cache appends are the bits of
 * vaura_attention_step_kv.  VAURA_ERR_ARG: probs NULL, pos0 < 0, n_steps < 1, rows_out outside [1, rows], and what that entry refuses;
 * VAURA_ERR_SHAPE: max_len > 256 or n_split > 1 (the generic and range-split kernels report nothing).  Nothing is launched then.      */
int vaura_attention_step_probs(const float* qkv, const float* qkv2, const float* rope, float* kcache, float* vcache, uint8_t* kscale,
                               uint8_t* vscale, float* out, uint16_t* out_split, float* part, uint32_t* arrivals, int rows, int n_head,
                               int head_dim, int max_len, int pos, int n_split, int plane_shift, int kv_dtype, float* probs, int pos0,
                               int n_steps, int rows_out, vaura_stream_t s);
/* The attention map of a finished call from its reported weights: probs fp32 (n_steps, n_rows, n_head, max_len) ->
 *   all_heads = 0: out (n_rows, n_steps, W) = ((p_0 + p_1) + .. + p_{n_head-1}) * (1 / n_head), heads added in index order in fp32
 *   all_heads = 1: out (n_rows, n_head, n_steps, W), a transposed copy
 * over columns j < W <= max_len.  VAURA_ERR_ARG: NULL pointers, a count < 1, W > max_len.                                             */
int vaura_attention_map(const float* probs, float* out, int n_steps, int n_rows, int n_head, int max_len, int W, int all_heads,
                        vaura_stream_t s);
/* Op-level access for parity tests: the attention of a teacher-forced chunk [p0, p0 + n_pos) of one layer — rope(q, k) + K / V append of
 * the chunk, then its causal attention over cache positions [0, p0 + n_pos) — on a caller-filled descriptor.  Read: dims (n_layer, n_head,
 * d_model = 96 n_head), rows, max_len, kv_dtype, plane_shift, rope, ws_qkv (packed rows: position z of the chunk is row block(s)
 * z * rows16 .. ; q is rotated in place), kcache, vcache, ws_attn, ws_attn_split (NULL ok), with kv_dtype = 3 kscale and vscale.
 * VAURA_ERR_ARG: null pointers (kscale / vscale with kv_dtype = 3 included), p0 < 0,
 * n_pos <= 0, p0 + n_pos > max_len; VAURA_ERR_SHAPE: head_dim != 96, or a narrow cache (kv_dtype != 0) of more than 256 positions.
 * PREFILL_ATTN_PER_POSITION selects the per-position kernel (fp32).                                                                      */
int vaura_attention_prefill(const vaura_decoder* d, int layer, int p0, int n_pos, vaura_stream_t s);
/* Op-level access to the masked append of vaura_prefill_rows: rope of q (in place, EVERY row) and of k, and the K / V append of the
 * chunk [p0, p0 + n_pos) of one layer only for the rows r with row_n[r] == n_sel (row_n: d->rows int32 in device memory); the cache
 * rows and exponent bytes of every other row keep their bytes.  On the selected rows the bytes are those of the append that
 * vaura_attention_prefill starts with.  Reads of `d` as there (no ws_attn).  VAURA_ERR_ARG: a NULL row_n, and what that entry refuses. */
int vaura_rope_append_rows(const vaura_decoder* d, int layer, int p0, int n_pos, const int32_t* row_n, int n_sel, vaura_stream_t s);

/* -------------------------------------------------------------------------------------------
 * a16 DacModelWrapper.decode (models/modules/dac/model.py:41-48): quantizer.from_codes + DAC
 * decoder (descript-audio-codec 1.0.0, un-vendored).  Weight-norm is folded by the caller.      */
typedef struct vaura_conv {
  const float* w;     /* conv: [taps][Cout][Cin]; transposed (stride r, k = 2r, pad r/2): [r][2][Cout][Cin] */
  const float* bias;  /* (Cout) */
  const float* wscale;/* codec precision 3 only, else NULL: (Cout) power-of-two scale of the layer's e4m3 weights; `w` is then the
                         packed fp8 stream [phase][step][Cout][4][32] described at vaura_codec.precision */
  int32_t cin, cout, taps, dilation, stride, _pad;
} vaura_conv;

typedef struct vaura_codec {
  int32_t n_codebooks, codebook_size, codebook_dim, latent_dim;
  int32_t n_blocks, n_units;        /* 4 decoder blocks, 3 residual units each */
  int32_t rates[4];
  const float* codebooks;           /* (K, size, dim)                    quantizer.quantizers[k].codebook */
  const float* out_proj_w;          /* (K, latent, dim) weight-norm folded                     .out_proj   */
  const float* out_proj_b;          /* (K, latent) */
  vaura_conv conv_in;               /* latent -> C0, k7                                  decoder.model.0   */
  const float* alpha_up[4];         /* Snake in front of each transposed conv   decoder.model.{b+1}.block.0 */
  vaura_conv up[4];                 /*                                           decoder.model.{b+1}.block.1 */
  const float* alpha_res[4][3][2];  /* Snakes of each residual unit              ...block.{u+2}.block.{0,2} */
  vaura_conv res[4][3][2];          /* {k7 dilated, k1}                          ...block.{u+2}.block.{1,3} */
  const float* alpha_out;           /* final Snake                               decoder.model.{n+1}        */
  vaura_conv conv_out;              /* C_last -> 1, k7, w as [7][C_last]; tanh   decoder.model.{n+2}        */
  float* ws[4];                     /* activation buffers, channels-last (B, L, C), ws_elems x 4 bytes each */
  size_t ws_elems;
  int32_t precision;                /* 0: fp32 activations/weights, exact v_mfma_f32_16x16x4_f32;
                                       1: (hi, lo) fp16 pairs, 3 x v_mfma_f32_16x16x32_f16 per product: conv weights
                                          (not conv_out) must then be given in pair layout
                                          [.. Cout][Cin/8][hi|lo][8] halves instead of [.. Cout][Cin] floats;
                                       2: as 1 with single-plane weights (the caller guarantees every lo plane is zero, e.g.
                                          fp8-quantised weights: e4m3 x power-of-two scale is exact in fp16): the lo-plane
                                          product is skipped, 2 MFMAs per product (BASELINE configs[4] codec part);
                                       3: block-scaled fp8 on v_mfma_scale_f32_16x16x128_f8f6f4 (BASELINE configs[4]
                                          "fp8 MFMA ... codec conv"): activations are e4m3 with one power-of-two scale per
                                          32 channels of a row (quantised by the producing kernel), weights e4m3 with one
                                          power-of-two scale per output channel (`wscale`).  conv_in keeps the layout of 2
                                          (its input comes from the quantizer); conv_out stays fp32.  Weight stream of
                                          every other conv: per phase, input channels in super-chunks of 128 (the last may
                                          hold nch = 1..3 blocks of 32); inside a super-chunk the k-blocks kb = tap*nch + ch
                                          are taken four per step, so step s holds, for every output channel, 4 x 32 bytes
                                          (kb = 4s .. 4s+3; zeros past the last k-block): [phase][step][Cout][4][32].
                                       4: "f16": buffers and weights as in 1, but ONE matrix instruction per product — hi(w) x hi(x),
                                          plain fp16 operands with fp32 accumulate (the arithmetic class the reference runs DAC in,
                                          models/vaura_model.py:92); the lo planes are written but not read                      */
  int32_t _pad1;
} vaura_codec;

/* codes (B, K, T) int32 -> wav (B, 1, T*prod(rates)) fp32 */
int vaura_dac_decode(const vaura_codec* c, const int32_t* codes, int B, int T, float* wav, vaura_stream_t s);
/* floats each of the 4 workspaces must hold for (B, T) */
size_t vaura_dac_workspace_elems(const vaura_codec* c, int B, int T);
/* Clips of different lengths in ONE decode pass.  codes (B, K, T_max) int32, padded; lengths: B ints ON THE HOST, clip b has
 * lengths[b] frames, 1 .. T_max (codes behind them are not read) -> wav (B, 1, T_max*hop): wav[b, 0, :lengths[b]*hop] is bit for bit
 * what vaura_dac_decode gives for codes[b, :, :lengths[b]] alone, every sample behind it is 0.
 * How: the clips are laid out behind one another as ONE sequence with a gap of vaura_dac_clips_gap(c) latent frames of zeros
 * between neighbours — clip b at latent row o_b, at row o_b * rate on a level with `rate` rows per frame, at sample o_b * hop — and
 * every convolution runs on that sequence as a batch of one, through the kernels and the instance choice of vaura_dac_decode (the
 * grid is that of the whole batch, so short clips reach the 256-row and one-launch instances too).  A tap that leaves a clip reads a
 * gap row (zeros: what the row mask gives the clip alone); the gap rows of an activated buffer are cleared again behind the launch
 * that wrote it.  The gap is the smallest number of frames that covers, on every level, the one-sided reach ((taps - 1) / 2 *
 * dilation rows; 1 for a transposed conv) of the convs that run there: 4 for the 44.1 kHz geometry (27 rows at 8 rows per frame).
 * Nothing in the call waits for the device or copies from it; the lengths are read before it returns.
 * The 4 workspaces must hold vaura_dac_decode_clips_workspace_elems(c, B, lengths) floats each (0: c / lengths NULL, B <= 0, a
 * length < 1, or a sequence beyond the int range).
 * VAURA_ERR_ARG: NULL c / codes / wav / lengths (not dereferenced), B or T_max <= 0, a length outside 1 .. T_max, workspaces NULL or
 * too small; VAURA_ERR_SHAPE: as vaura_dac_decode, or the packed sequence's largest level (rows x channels) does not fit an int;
 * VAURA_ERR_DTYPE: precision.  All before any launch.                                                                               */
int vaura_dac_decode_clips(const vaura_codec* c, const int32_t* codes, int B, int T_max, const int32_t* lengths, float* wav,
                           vaura_stream_t s);
size_t vaura_dac_decode_clips_workspace_elems(const vaura_codec* c, int B, const int32_t* lengths);
/* gap (latent frames) of vaura_dac_decode_clips for this geometry, from the convs' taps, dilations and the rates; -1: c NULL or not a
 * geometry the decode pass takes.  Reads no device pointer.                                                                          */
int vaura_dac_clips_gap(const vaura_codec* c);
/* A WINDOW of every clip in one decode pass: the samples of clip b's frames [starts[b], starts[b] + counts[b]), bit for bit those of
 * the whole clip's decode (vaura_dac_decode / vaura_dac_decode_clips), at the cost and the workspace of the window.
 * codes (B, K, T_max) int32, the caller's padded tensor (read only); lengths, starts, counts: B ints each ON THE HOST; clip b has
 * lengths[b] frames, 1 .. T_max (lengths NULL: T_max each) -> wav (B, 1, N_max*hop): wav[b, 0, :counts[b]*hop] are the samples of
 * those frames, every sample behind them is 0.  counts[b] == 0 — a clip that is finished or parked — is allowed: nothing of the clip
 * is read or decoded, its row is 0.
 * How: the decoder is a finite-support conv stack, so the samples of a frame depend on the codes of H = vaura_dac_decode_halo(c)
 * frames either side and no further.  Per clip the frames [max(0, s - H), min(len, s + n + H)) are packed behind one another as
 * the clips of vaura_dac_decode_clips are (the same gap, the same pass, the same kernels and instance choice), and unpacking skips
 * the halo samples in front.  A window that reaches an end of its clip is clamped there, so the zero padding at that end is the
 * clip's own.  Nothing in the call waits for the device or copies from it; the host arrays are read before it returns.
 * The 4 workspaces must hold vaura_dac_decode_window_workspace_elems(c, B, lengths, starts, counts) floats each (0: c / starts /
 * counts NULL, B <= 0, arguments the call refuses, or a sequence beyond the int range; lengths NULL there: no window is clamped at
 * its clip's end, an upper bound).
 * VAURA_ERR_ARG: NULL c / codes / wav / starts / counts (not dereferenced), B, T_max or N_max <= 0, a length outside 1 .. T_max,
 * starts[b] < 0, counts[b] < 0, starts[b] + counts[b] > lengths[b], counts[b] > N_max, every count 0, workspaces NULL or too small;
 * VAURA_ERR_SHAPE: as vaura_dac_decode, a descriptor without a halo, or packed windows whose largest level (rows x channels) does
 * not fit an int; VAURA_ERR_DTYPE: precision.  All before any launch.                                                                */
int vaura_dac_decode_window(const vaura_codec* c, const int32_t* codes, int B, int T_max, const int32_t* lengths, const int32_t* starts,
                            const int32_t* counts, float* wav, int N_max, vaura_stream_t s);
size_t vaura_dac_decode_window_workspace_elems(const vaura_codec* c, int B, const int32_t* lengths, const int32_t* starts,
                                               const int32_t* counts);
/* H of vaura_dac_decode_window: the frames of context either side that the samples of one latent frame depend on, from the convs'
 * taps, dilations and strides (the sample interval of a frame taken backwards through the layers; a transposed conv has k = 2r and
 * pad ceil(r / 2)): 10 for the 44.1 kHz geometry.  -1: c NULL or not such a geometry.  Reads no device pointer.                      */
int vaura_dac_decode_halo(const vaura_codec* c);
/* vaura_dac_decode_window straight from the decode loop's pattern sequence: seq (B, K, S) int32 as vaura_pattern_build_delays lays it
 * out and the loop fills it — frame t of codebook q at step t + 1 + d_q, d = delays_host (K ints ON THE HOST, sorted as the pattern ops
 * take them; NULL: d_q = q), T = S - 1 - max(d) frames per clip, K >= c->n_codebooks (the first c->n_codebooks rows are decoded).
 * Only the pack differs: it gathers seq[b, q, t + 1 + d_q] where the window call reads codes[b, q, t]; the plan of the windows, the gap,
 * the pass, the kernels and the instance choice are vaura_dac_decode_window's with T_max = T, and so are the samples, bit for bit, of
 * the call on the reverted codes.  A caller that streams audio while the loop still runs needs no reverted tensor: the frames a window
 * and its halo cover must be FINAL in seq (every codebook's slot sampled), lengths[b] is the clip's whole length T_b, not what is final
 * so far.  A slot that holds no code (unknown, special token) is never used as an index: it is packed as code 0.
 * The 4 workspaces must hold vaura_dac_decode_window_seq_workspace_elems(...) floats each (0: arguments the call refuses).
 * VAURA_ERR_ARG: what vaura_dac_decode_window refuses, K < c->n_codebooks or > 16, S < 2, a delay < 0 or > S - 2, or a window whose
 * halo reaches a step >= S; VAURA_ERR_SHAPE / VAURA_ERR_DTYPE as there.  All before any launch.                                       */
int vaura_dac_decode_window_seq(const vaura_codec* c, const int32_t* seq, int B, int K, int S, const int32_t* delays_host,
                                const int32_t* lengths, const int32_t* starts, const int32_t* counts, float* wav, int N_max,
                                vaura_stream_t s);
size_t vaura_dac_decode_window_seq_workspace_elems(const vaura_codec* c, int B, int K, int S, const int32_t* delays_host,
                                                   const int32_t* lengths, const int32_t* starts, const int32_t* counts);
/* Op-level access for parity tests: ONE convolution of the decoder (WNConv1d / WNConvTranspose1d of descript-audio-codec's
 * DecoderBlock / ResidualUnit) in the arithmetic of `precision` (vaura_codec.precision; weights laid out for it).
 * in (B, Lin, Cin) fp32 channels-last, already activated -> out (B, Lout, Cout) fp32 = conv(in) + bias,
 * Lout = Lin * stride.  `scratch` (>= B*Lin*Cin floats) receives the input in the precision's activation format.   */
int vaura_dac_conv(const vaura_conv* cv, int precision, const float* in, float* out, float* scratch, int B, int Lin,
                   vaura_stream_t s);
/* Op-level access for parity tests: vaura_dac_conv with the epilogue of the decode path — exactly the launch vaura_dac_decode /
 * vaura_dac_encode make for one convolution.  in (B, Lin, Cin) fp32, already activated (converted into `scratch` as above; for
 * precision 0 scratch may be NULL).  res (B, Lout, Cout) fp32 or NULL: added to conv(in) + bias.  out_raw (B, Lout, Cout) fp32 or NULL:
 * that sum.  out_act or NULL (then alpha may be NULL): Snake(alpha) of it in the precision's own activation format: fp32 (B, Lout, Cout)
 * for precision 0; pair planes [row][Cout/8][hi|lo][8] halves for 1, 2 and 4; for 3 e4m3 bytes (B, Lout, Cout) followed, at byte
 * ((B*Lout*Cout + 15) & ~15), by (B * Lout, ceil(Cout/128)) words of four E8M0 bytes, one per 32 channels (4 * B*Lout*Cout bytes hold
 * both).  At least one of out_raw / out_act.  VAURA_ERR_ARG / VAURA_ERR_SHAPE as vaura_dac_conv; out_act without alpha: VAURA_ERR_ARG. */
int vaura_dac_conv_ex(const vaura_conv* cv, int precision, const float* in, const float* res, const float* alpha, float* out_raw,
                      void* out_act, float* scratch, int B, int Lin, vaura_stream_t s);
/* Returned by vaura_dac_unit when the unit is not eligible for the one-launch kernel (shape, precision, fewer than 384 workgroups, or
 * CODEC_128_ROWS / CODEC_UNIT_TWO_LAUNCHES): not an error.                                                                                       */
#define VAURA_DAC_UNIT_TWO_LAUNCHES (-100)
/* Op-level access for parity tests: ONE residual unit of the decoder, out = res + c1(Snake(alpha_mid)(c7(in))), as vaura_dac_decode runs
 * it.  in (B, L, C) fp32 = Snake of the unit's input, already applied; res (B, L, C) fp32 the unit's input; out_raw (NULL ok) and out_act
 * (required; Snake(alpha_next) of out) as for vaura_dac_conv_ex.  Returns 0 when the unit ran as ONE launch (vaura_debug_counter(1)
 * counts those).  Otherwise VAURA_DAC_UNIT_TWO_LAUNCHES: with `mid` (4 * B*L*C bytes; receives c7's activated output in the precision's
 * format) the two convolutions were launched one after the other and the outputs are valid, with mid = NULL nothing was launched.
 * out_act must not alias in / scratch.                                                                                                  */
int vaura_dac_unit(const vaura_conv* c7, const vaura_conv* c1, int precision, const float* in, const float* res,
                   const float* alpha_mid, const float* alpha_next, float* out_raw, void* out_act, float* scratch, float* mid, int B,
                   int L, vaura_stream_t s);
/* Op-level access for parity tests: quantizer.from_codes as vaura_dac_decode launches it.  codes (B, K, T) int32, codebooks (K, size,
 * dim), out_proj_w (K, latent, dim), out_proj_b (K, latent) -> z (B, T, latent): fp32 for pairs = 0, pair planes otherwise.
 * K <= 16, dim <= 8, latent % 8 == 0 (VAURA_ERR_SHAPE).  Codes are not range-checked.                                                  */
int vaura_dac_from_codes(const int32_t* codes, const float* codebooks, const float* out_proj_w, const float* out_proj_b, void* z,
                         int B, int K, int T, int size, int dim, int latent, int pairs, vaura_stream_t s);
/* Op-level access for parity tests: the decoder's last convolution (C -> 1, k = 7, tanh; cv->w fp32 [7][C]) with the dispatch of
 * vaura_dac_decode (CODEC_LAST_CONV_UNTILED: the untiled kernel).  in (B, L, C) fp32, converted into `scratch` (>= B*L*C floats) in the
 * activation format of `precision` (0: read as is; 1, 2, 4: pair planes; 3: mx8) -> wav (B, L) fp32.                                   */
int vaura_dac_conv_out(const vaura_conv* cv, int precision, const float* in, float* wav, float* scratch, int B, int L,
                       vaura_stream_t s);
/* Op-level access for parity tests: the codec's activation, Snake1d of descript-audio-codec 1.0.0 (dac/nn/layers.py: x + (alpha + 1e-9)^-1 *
 * sin(alpha x)^2), exactly as every conv epilogue of the decoder / encoder applies it.  x, y (rows, C) fp32 channels-last, alpha (C).
 * The sine is an own restatement (period-pi reduction of sin^2 + a degree-9 odd polynomial, csrc/conv_kernels.h::snake_sin2): max abs error
 * 2.5e-7 for |alpha x| < 1e6 — the library sinf was the largest single cost of the decode.                                             */
int vaura_snake(const float* x, const float* alpha, float* y, int64_t rows, int C, vaura_stream_t s);

/* -------------------------------------------------------------------------------------------
 * f4 DacModelWrapper.encode (models/modules/dac/model.py:30-39): DAC encoder + residual VQ (descript-audio-codec
 * 1.0.0, un-vendored: dac/model/dac.py Encoder, dac/nn/quantize.py).  Convolutions run on (hi, lo) fp16 pairs like the
 * decoder's precision 1: conv weights in pair layout, weight-norm folded by the caller.                           */
typedef struct vaura_codec_encoder {
  int32_t n_codebooks, codebook_size, codebook_dim, latent_dim;
  int32_t n_blocks, n_units;        /* 4 encoder blocks, 3 residual units each */
  int32_t rates[4];                 /* (2, 4, 8, 8) */
  int32_t enc_dim;                  /* 64: channels after the first conv; doubles per block */
  int32_t _pad0;
  const float* conv_in_w;           /* (7, enc_dim) fp32 = encoder.block.0 weight as [tap][Cout]          */
  const float* conv_in_b;           /* (enc_dim) */
  const float* alpha_res[4][3][2];  /* Snakes of each residual unit      encoder.block.{b+1}.block.{u}.block.{0,2} */
  vaura_conv res[4][3][2];          /* {k7 dilated, k1}                  ...block.{u}.block.{1,3}                   */
  const float* alpha_down[4];       /* Snake in front of each strided conv       encoder.block.{b+1}.block.3        */
  vaura_conv down[4];               /* encoder.block.{b+1}.block.4 (C -> 2C, k = 2r, stride r, pad r/2) restated as a
                                       3-tap stride-1 conv over rows of r*C channels (the (L, C) buffer read as
                                       (L/r, r*C)): cin = r*C, cout = 2C, taps = 3, dilation = 1, stride = 1,
                                       w'[tau+1][co][q*C + ci] = w[co][ci][tau*r + q + r/2] (0 outside [0, 2r))     */
  const float* alpha_out;           /* final Snake                               encoder.block.{n+1}                 */
  vaura_conv conv_out;              /* C_last -> latent, k3                      encoder.block.{n+2}                 */
  const float* in_proj_w;           /* (K, dim, latent) weight-norm folded       quantizer.quantizers[k].in_proj     */
  const float* in_proj_b;           /* (K, dim) */
  const float* codebooks;           /* (K, size, dim)                                                                */
  const float* out_proj_w;          /* (K, latent, dim)                                                              */
  const float* out_proj_b;          /* (K, latent) */
  float* ws[4];                     /* activation buffers, ws_elems x 4 bytes each */
  size_t ws_elems;
} vaura_codec_encoder;
/* wav (B, n_samples) fp32, n_samples a multiple of prod(rates) (DAC.preprocess zero-pads on the right; the caller does)
 * -> codes (B, K, n_samples / prod(rates)) int32 */
int vaura_dac_encode(const vaura_codec_encoder* c, const float* wav, int B, int64_t n_samples, int32_t* codes, vaura_stream_t s);
/* Op-level access for parity tests: the encoder's first convolution (1 -> C, k = 7, pad 3) as vaura_dac_encode launches it.  wav (B, L)
 * fp32, w (7, C), bias (C), alpha (C) -> out_raw (B, L, C) fp32 and out_act = Snake(alpha) of it in pair planes.  C % 32 == 0.           */
int vaura_dac_enc_conv_in(const float* wav, const float* w, const float* bias, const float* alpha, float* out_raw, void* out_act,
                          int B, int64_t L, int C, vaura_stream_t s);
/* Op-level access for parity tests: ONE stage of the residual vector quantiser as vaura_dac_encode launches it.  residual (B * T,
 * latent) fp32 is updated in place; in_w (dim, latent), in_b (dim), codebook (size, dim), out_w (latent, dim), out_b (latent) are the
 * stage's own; its codes go to codes[(b * K + k) * T + t] of a (B, K, T) int32 tensor.  dim <= 8, size <= 1024, latent <= 2048.       */
int vaura_dac_rvq_stage(float* residual, const float* in_w, const float* in_b, const float* codebook, const float* out_w,
                        const float* out_b, int32_t* codes, int B, int T, int latent, int dim, int size, int K, int k,
                        vaura_stream_t s);
size_t vaura_dac_encode_workspace_elems(const vaura_codec_encoder* c, int B, int64_t n_samples);
/* Clips of different lengths in ONE encode pass.  wav (B, n_max) fp32, padded (n_max need not be a multiple of the hop);
 * sample_lengths: B int64 ON THE HOST, clip b has sample_lengths[b] samples, 1 .. n_max (samples behind them are not read)
 * -> codes (B, K, T_max) int32, T_max = ceil(n_max / hop): codes[b, :, :ceil(n_b / hop)] is bit for bit what vaura_dac_encode gives for
 * clip b's own samples (zero-padded to a multiple of the hop, DAC.preprocess) alone, every frame behind them holds 0.
 * The packed sequence of vaura_dac_decode_clips, from the other side: clip b's samples at sample o_b * hop, zeros up to the end of
 * its last frame, then vaura_dac_encode_clips_gap(c) frames of zeros; the strided convs keep their view of r rows as one (every
 * offset is a multiple of the hop).  The gap covers the encoder's reaches per level: 4 for the 44.1 kHz geometry (27 rows in the
 * last block, at 8 rows per frame).  No wait for the device, no copy from it.
 * Workspaces: vaura_dac_encode_clips_workspace_elems(c, B, sample_lengths) floats each (0 as above).
 * VAURA_ERR_ARG: NULL c / wav / codes / sample_lengths (not dereferenced), B or n_max <= 0, a length outside 1 .. n_max, workspaces
 * NULL or too small; VAURA_ERR_SHAPE: as vaura_dac_encode, or the packed sequence does not fit an int.  All before any launch.       */
int vaura_dac_encode_clips(const vaura_codec_encoder* c, const float* wav, int B, int64_t n_max, const int64_t* sample_lengths,
                           int32_t* codes, vaura_stream_t s);
size_t vaura_dac_encode_clips_workspace_elems(const vaura_codec_encoder* c, int B, const int64_t* sample_lengths);
int vaura_dac_encode_clips_gap(const vaura_codec_encoder* c);

/* -------------------------------------------------------------------------------------------
 * f3 (the step after the path) post-codec scaling: normalize_audio (utils/data_utils.py:407-466) as called by
 * scale_audio / save_results (scripts/generate.py:404, 440-461), per clip.  wav/out: (n_clips, n_samples) fp32 (may
 * alias).  strategy: 0 'clip' (the generate_*.yaml default: clamp to +-10^(-db/20)), 1 'peak', 2 'rms' (then clamp
 * to +-1), 3 'none' (copy).  normalize: the reference's flag (rescale only when it would otherwise clip, if 0).
 * scratch: vaura_audio_scratch_elems(n_clips) floats (strategies 1, 2).  'loudness': vaura_audio_loudness below.   */
typedef enum vaura_audio_strategy { VAURA_AUDIO_CLIP = 0, VAURA_AUDIO_PEAK = 1, VAURA_AUDIO_RMS = 2, VAURA_AUDIO_NONE = 3 } vaura_audio_strategy;
int vaura_audio_normalize(const float* wav, float* out, int n_clips, int64_t n_samples, int strategy, int normalize,
                          float peak_clip_headroom_db, float rms_headroom_db, float* scratch, vaura_stream_t s);
size_t vaura_audio_scratch_elems(int n_clips);
/* f3, strategy 'loudness' (utils/data_utils.py:453-458 -> normalize_loudness :347-387 -> _clip_wav :389-404): per clip, gain to
 * -loudness_headroom_db LKFS (ITU-R BS.1770-4 integrated loudness as torchaudio 2.2.1's transforms.Loudness computes it — a
 * third-party dependency absent from the reference tree: restated from the published algorithm, PARITY UNPINNED), optional tanh
 * compressor, clamp to [-1, 1]; clips below energy_floor rms (reference: 2e-3) or shorter than one 400 ms gating block are only clamped.
 * scratch: vaura_audio_loudness_scratch_elems(n_clips) floats; its first n_clips floats hold the applied gains afterwards. */
int vaura_audio_loudness(const float* wav, float* out, int n_clips, int64_t n_samples, int sample_rate, float loudness_headroom_db,
                         int compressor, float energy_floor, float* scratch, vaura_stream_t s);
size_t vaura_audio_loudness_scratch_elems(int n_clips);
/* The two entry points above for the zero-padded waveform of a ragged batch (generate(max_new_tokens=[..]) -> "audio_lengths"): clip b
 * occupies wav[b * n_stride, b * n_stride + n_b), n_b = lengths[b] (device, n_clips int32, 4-byte aligned).  Its statistics and its
 * output samples [0, n_b) are the bits of a one-clip call of the entry point above with n_samples = n_b on those samples (everything
 * derived from the length — the partition of the sums, the rms divisor, the gating blocks, "shorter than one block" — is derived
 * from n_b); out[b, n_b:] is written as 0.0f; wav[b, n_b:] is never read (it may hold anything, NaN included).  Scratch: the same
 * *_scratch_elems(n_clips); the loudness gains are per clip as above.  VAURA_ERR_ARG before any launch: lengths NULL or misaligned, a
 * value outside 1 .. n_stride (the n_clips values are read back once; skipped while the stream is capturing).  VAURA_ERR_SHAPE for
 * 'loudness' as above, from n_stride.                                                                                              */
int vaura_audio_normalize_clips(const float* wav, float* out, int n_clips, int64_t n_stride, const int32_t* lengths, int strategy,
                                int normalize, float peak_clip_headroom_db, float rms_headroom_db, float* scratch, vaura_stream_t s);
int vaura_audio_loudness_clips(const float* wav, float* out, int n_clips, int64_t n_stride, const int32_t* lengths, int sample_rate,
                               float loudness_headroom_db, int compressor, float energy_floor, float* scratch, vaura_stream_t s);

/* -------------------------------------------------------------------------------------------
 * f2 (the step before the path) Segment-AVCLIP visual features: MotionFormer.forward
 * (models/modules/feature_extractors/avclip/motionformer.py:252-364) for the generate_*.yaml configuration: divided space-time
 * ViT-B/16 ('divided_224_16x4': motionformer_src/video_model_builder.py:174-268, vit_helper.py:392-472, 80-172, 523-557) + one
 * spatial nn.TransformerEncoderLayer per frame (motionformer.py:366-512), eval mode, no content mask.
 * Linear weights ("*_w") are in the codec's (hi, lo) fp16 PAIR layout [Cout][Cin/8][hi|lo][8] halves (row-major (Cout, Cin) of
 * nn.Linear.weight; the Conv3d weight flattened to (768, 1536)); everything else fp32.                                   */
typedef struct vaura_vit_attn {      /* DividedAttention (vit_helper.py:80-96) */
  const void* qkv_w; const float* qkv_b;      /* (3D, D) pair layout, (3D) */
  const void* proj_w; const float* proj_b;    /* (D, D) pair layout, (D)   */
} vaura_vit_attn;
typedef struct vaura_vit_block {     /* DividedSpaceTimeBlock (vit_helper.py:392-441) */
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *ln3_w, *ln3_b;      /* norm1 (space), norm2 (mlp), norm3 (time) */
  vaura_vit_attn space, time;                                       /* .attn, .timeattn */
  const void* fc1_w; const float* fc1_b; const void* fc2_w; const float* fc2_b;   /* mlp.fc1 (hidden, D), mlp.fc2 (D, hidden) */
} vaura_vit_block;
typedef struct vaura_vit {
  int32_t depth, dim, heads, hidden;           /* 12, 768, 12, 3072 */
  int32_t n_patches, n_frames;                 /* 196 tokens per frame, 8 token frames */
  int32_t in_chans, frames, img, patch, patch_t, patch_k;   /* 3, 16, 224, 16, 2, 1536 = 3*2*16*16 */
  float eps; int32_t _pad;                     /* 1e-6 */
  const void* pe_w; const float* pe_b;         /* patch_embed_3d.proj (D, patch_k) pair layout, (D) */
  const float *cls_token, *pos_embed, *temp_embed;     /* (D), (1 + n_patches, D), (n_frames, D) */
  const vaura_vit_block* blocks_host;          /* HOST array [depth] of device pointers */
  const float *norm_w, *norm_b;                /* final LayerNorm */
  const float* agg_cls;                        /* spatial_attn_agg.cls_token (D) */
  const float *agg_ln1_w, *agg_ln1_b, *agg_ln2_w, *agg_ln2_b;
  const void* agg_in_w; const float* agg_in_b;         /* self_attn.in_proj (3D, D) */
  const void* agg_out_w; const float* agg_out_b;       /* self_attn.out_proj (D, D) */
  const void* agg_l1_w; const float* agg_l1_b;         /* linear1 (hidden, D) */
  const void* agg_l2_w; const float* agg_l2_b;         /* linear2 (D, hidden) */
  /* workspaces, sizes from vaura_avclip_workspace_bytes(v, n_seg, i), i = 0..6 in this order */
  float* ws_x; float* ws_qkv; uint16_t* ws_a; uint16_t* ws_h; uint16_t* ws_p; float* ws_z; float* ws_s;
} vaura_vit;
/* frames (n_seg, 3, 16, 224, 224) fp32 (the (B, S) segments flattened) -> feats (n_seg, 8, 768) fp32 */
int vaura_avclip_forward(const vaura_vit* v, const float* frames, int n_seg, float* feats, vaura_stream_t s);
size_t vaura_avclip_workspace_bytes(const vaura_vit* v, int n_seg, int which);

/* Op-level entry points of the extractor: each runs ONE launcher of vaura_avclip_forward (the same static function the forward
 * calls) on caller-owned buffers, so the op-level parity tests (tests/test_gpu_avclip_ops.py) test the product path.  Those that
 * take a vaura_vit read only its dims, eps and the pointers named below (no workspace, no blocks) and apply the forward's own
 * shape gate first: dim == 768, heads * 64 == dim, n_frames == 8, 1 <= n_patches <= 255, hidden % 96 == 0, patch_k % 32 == 0
 * (VAURA_ERR_SHAPE otherwise; NULL pointers / counts <= 0: VAURA_ERR_ARG; nothing is launched in either case).
 * "pair" = the (hi, lo) fp16 pair layout [row][C/8][hi|lo][8] halves, 4 bytes per element.
 *   patchify       frames (n_seg, in_chans, frames_per_seg, img, img) fp32, 16-byte aligned -> patches (n_seg * T/pt * (img/patch)^2,
 *                  in_chans * pt * patch^2) pair, columns in the Conv3d weight's flattening order.  patch % 8, img % patch,
 *                  frames_per_seg % patch_t and columns % 32 must be 0 (VAURA_ERR_SHAPE).
 *   embed          x (n_seg, 1 + 8 n_patches, 768) fp32 in place: row 0 = cls_token + pos_embed[0]; row 1 + f n_patches + i +=
 *                  pos_embed[1 + i] + temp_embed[f] (v->cls_token, v->pos_embed, v->temp_embed).
 *   layernorm      `rows` rows of x (v->eps, biased variance) -> out_f32 and / or out_pair (either may be NULL, not both).  map 0: row r
 *                  -> row r.  map 1 (rows a multiple of 8 n_patches): source rows are the patch rows of sequences of 1 + 8 n_patches
 *                  rows (row 0 of each is never read), destination row (seg * 8 + f) * (n_patches + 1) + 1 + i (slot 0 not written).
 *   fill_rows      dst[i * stride] (768 floats each) = vec for i < n.
 *   cls_attention  qkv (n_seq * Lseq, 3 * 768) fp32 rows [q | k | v]: the query of row 0 of every sequence over its Lseq rows ->
 *                  out_pair row seq * out_stride.  part != NULL and Lseq > 512: 8 key splits and a combine launch, part >= n_seq *
 *                  heads * 8 * 66 floats.  Lseq <= 2041 (VAURA_ERR_SHAPE).
 *   time / space   qkv (n_seg * (1 + 8 n_patches), 3 * 768): every patch row over the CLS row and the 8 rows at its location / the
 *                  n_patches rows of its frame -> out_pair, same row; CLS rows of out_pair are not written.  n_patches > 207 takes
 *                  the generic fp32 kernel.
 *   linear_pair    out[b][row + oshift] = act(in[b][row] . w^T + bias (+ res[b][row + oshift])), in (B, Lin, Cin) pair, w (Cout, Cin)
 *                  pair, out_raw fp32 and / or out_act pair in sequences of Lout rows; res may be out_raw.  act 1: exact GELU
 *                  into out_act, 2: identity.  Cin % 32, Cout % 96 (VAURA_ERR_SHAPE); Lin + oshift <= Lout, act in {1, 2} (VAURA_ERR_ARG). */
int vaura_vit_patchify(const float* frames, void* patches, int n_seg, int in_chans, int frames_per_seg, int img, int patch_t, int patch,
                       vaura_stream_t s);
int vaura_vit_embed(const vaura_vit* v, float* x, int n_seg, vaura_stream_t s);
int vaura_vit_layernorm(const vaura_vit* v, const float* x, const float* w, const float* b, float* out_f32, void* out_pair, int64_t rows,
                        int map, vaura_stream_t s);
int vaura_vit_fill_rows(const vaura_vit* v, float* dst, const float* vec, int64_t n, int64_t stride, vaura_stream_t s);
int vaura_vit_cls_attention(const vaura_vit* v, const float* qkv, void* out_pair, float* part, int n_seq, int Lseq, int64_t out_stride,
                            vaura_stream_t s);
int vaura_vit_time_attention(const vaura_vit* v, const float* qkv, void* out_pair, int n_seg, vaura_stream_t s);
int vaura_vit_space_attention(const vaura_vit* v, const float* qkv, void* out_pair, int n_seg, vaura_stream_t s);
int vaura_linear_pair(const void* in, const void* w, const float* bias, const float* res, float* out_raw, void* out_act, int act, int B,
                      int Lin, int Lout, int oshift, int Cin, int Cout, vaura_stream_t s);

/* -------------------------------------------------------------------------------------------
 * Video preprocessing (csrc/preproc.hip): decoded uint8 frames -> the extractor's input.  The `video_transforms_test` list of
 * configs/generate_*.yaml (Resize(resize, antialias) -> CenterCrop -> ToFloat32DType -> Normalize) followed by
 * GenerateMultipleSegments (models/data/transforms/video_transforms.py:114-240) and the dataset's permute, in one launch.
 *   video     uint8, (n_clips, T, C, H, W) or, channels_last != 0, (n_clips, T, H, W, C); C must be 3
 *   out       fp32 (n_clips, S, C, F, crop_h, crop_w), 16-byte aligned: segment s, slot f = source frame seg_start + s * seg_stride + f
 *   tables    built by the host once per (H, W, resize, crop) (vaura_amd/preprocess.py): for kept column x the horizontal taps
 *             h_w[x * h_taps + k] (int16, scaled by 2^h_prec) start at source column x0 + h_rel[x]; all kept columns read inside
 *             [x0, x0 + span).  For kept row r the vertical taps v_w[r * v_taps + k] (2^v_prec) start at source row v_start[r].
 *             Every start + taps lies inside the source (short rows are shifted and zero-filled by the host).
 *             lut[c * 256 + level] = ((level / 255) - mean[c]) / std[c] in fp32.
 *   tile_rows output rows per workgroup; tile_src_rows = the most source rows any tile needs (v_start[last] + v_taps - v_start[first]).
 * Arithmetic: acc = 2^(prec-1) + sum(tap * pixel); level = clamp(acc >> prec, 0, 255) after each pass (torch's uint8 path).
 * VAURA_ERR_SHAPE, before any launch: C != 3; crop larger than the resized image (short side -> resize, long side ->
 * int(resize * long / short)); crop_w % 4 != 0; T < F or a segment outside [0, T); more than VAURA_PREPROC_MAX_TAPS taps per
 * output pixel (32: a short side of up to 15 x resize, 3840 lines at resize = 256 — 1080 x 1920 needs 11); a tile that does not
 * fit 64 KiB of LDS (vaura_video_preprocess_lds_bytes; lower tile_rows); more than 65535 output frames per call.                 */
#define VAURA_PREPROC_MAX_TAPS 32
int vaura_video_preprocess(const uint8_t* video, int channels_last, int n_clips, int T, int C, int H, int W, int resize, int crop_h,
                           int crop_w, int F, int S, int seg_start, int seg_stride, const int32_t* h_rel, const int16_t* h_w, int h_taps,
                           int h_prec, const int32_t* v_start, const int16_t* v_w, int v_taps, int v_prec, int x0, int span,
                           int tile_rows, int tile_src_rows, const float* lut, float* out, vaura_stream_t s);
/* dynamic LDS bytes of one workgroup for these table sizes (0 for sizes the kernel does not take) */
size_t vaura_video_preprocess_lds_bytes(int channels_last, int crop_w, int h_taps, int span, int tile_src_rows);

/* The same from decoder surfaces: 8-bit 4:2:0 YUV -> RGB uint8 -> the resize / crop / scale / normalise above, in one launch.
 *   video     uint8, n_clips * T frames, frame i at byte i * frame_stride; H and W even.  In a frame, luma row y starts at byte
 *             y * pitch; the chroma plane starts at byte chroma_offset:
 *               VAURA_YUV_NV12  H / 2 rows of W / 2 interleaved (Cb, Cr) pairs, row to row `pitch` bytes
 *               VAURA_YUV_I420  the U plane, H / 2 rows of W / 2 bytes, row to row pitch / 2 bytes, then the V plane at byte
 *                               chroma_offset + (H / 2) * (pitch / 2), laid out the same
 *             The base address needs no alignment.  Bytes outside the planes (the padding of a decoder surface) never reach the
 *             result; the aligned 4-byte word around a plane's first or last byte may be loaded.
 *   video_bytes  the bytes that may be read from `video` on; the last plane byte of the last frame must lie inside them
 *   colour    level = clamp((cy * (Y - y_off) + cu * (U - 128) + cv * (V - 128) + 2^13) >> 14, 0, 255), arithmetic shift, with
 *             (cu, cv) = (0, crv) for R, (cgu, cgv) for G, (cbu, 0) for B; the sample at (y >> 1, x >> 1) serves its 2 x 2 luma
 *             block (no interpolation).  The host decides the integers (vaura_amd/preprocess.py: yuv_coefficients — BT.601
 *             limited range is 16, 19077, 26149, -6419, -13320, 33050); the result is RGB uint8 before the resize, as if
 *             vaura_video_preprocess had been given the converted frames.
 *   the rest  as vaura_video_preprocess (C is 3).
 * VAURA_ERR_SHAPE, before any launch: odd H or W; everything vaura_video_preprocess lists (the LDS size is
 * vaura_video_preprocess_yuv420_lds_bytes).  VAURA_ERR_ARG: an unknown layout; pitch < W; an odd pitch with VAURA_YUV_I420;
 * chroma_offset inside the luma plane or frame_stride inside the chroma plane (planes or frames that overlap); a last plane byte
 * behind video_bytes; y_off outside 0..255 or a coefficient beyond +-2^20 (the accumulator is an int32); and what
 * vaura_video_preprocess answers with VAURA_ERR_ARG.                                                                              */
enum { VAURA_YUV_NV12 = 0, VAURA_YUV_I420 = 1 };
int vaura_video_preprocess_yuv420(const uint8_t* video, int64_t video_bytes, int layout, int64_t pitch, int64_t chroma_offset,
                                  int64_t frame_stride, int n_clips, int T, int H, int W, int y_off, int cy, int crv, int cgu, int cgv,
                                  int cbu, int resize, int crop_h, int crop_w, int F, int S, int seg_start, int seg_stride,
                                  const int32_t* h_rel, const int16_t* h_w, int h_taps, int h_prec, const int32_t* v_start,
                                  const int16_t* v_w, int v_taps, int v_prec, int x0, int span, int tile_rows, int tile_src_rows,
                                  const float* lut, float* out, vaura_stream_t s);
/* dynamic LDS bytes of one workgroup of that launch (0 for sizes the kernel does not take) */
size_t vaura_video_preprocess_yuv420_lds_bytes(int layout, int crop_w, int h_taps, int span, int tile_src_rows);

/* Both launches with the source frame of every output frame named by a table: video at its own frame rate, converted to the
 * model's 25 fps by dropping and repeating frames (vaura_amd/preprocess.py: fps_plan restates ffmpeg's `fps` filter at its defaults
 * — parity unpinned by the reference, which re-encoded its videos offline), in one pass or block by block (VideoFrameStream).
 *   frame_map  device, int32 (n_clips, S * F): output frame (b, s, f) shows
 *                e >= 0  source frame e of clip b (the kernel clamps e into [0, T); the host validates before the launch)
 *                -1      nothing: the output frame's bytes stay as they are
 *                -2      clip b's frame in `carry` (left as it is where carry is NULL)
 *   carry      NULL, or one frame per clip in the source layout: (n_clips, C, H, W) / (n_clips, H, W, C) bytes; for the 4:2:0
 *              entry clip b's surface at byte b * frame_stride.  carry_used != 0 says that the map holds a -2.
 *   T          the frames per clip that `video` holds; any T >= 1 (a block of a stream is shorter than a segment)
 * The siblings' seg_start / seg_stride are not taken: the table has them applied.  Everything else, the arithmetic and every
 * refusal are the sibling's (T < F and segments outside [0, T) excepted), and VAURA_ERR_ARG for a NULL or misaligned frame_map and
 * for carry_used with a NULL carry — all before any launch.                                                                        */
int vaura_video_preprocess_frames(const uint8_t* video, int channels_last, int n_clips, int T, int C, int H, int W, int resize,
                                  int crop_h, int crop_w, int F, int S, const int32_t* h_rel, const int16_t* h_w, int h_taps, int h_prec,
                                  const int32_t* v_start, const int16_t* v_w, int v_taps, int v_prec, int x0, int span, int tile_rows,
                                  int tile_src_rows, const float* lut, float* out, const int32_t* frame_map, const uint8_t* carry,
                                  int carry_used, vaura_stream_t s);
int vaura_video_preprocess_yuv420_frames(const uint8_t* video, int64_t video_bytes, int layout, int64_t pitch, int64_t chroma_offset,
                                         int64_t frame_stride, int n_clips, int T, int H, int W, int y_off, int cy, int crv, int cgu,
                                         int cgv, int cbu, int resize, int crop_h, int crop_w, int F, int S, const int32_t* h_rel,
                                         const int16_t* h_w, int h_taps, int h_prec, const int32_t* v_start, const int16_t* v_w,
                                         int v_taps, int v_prec, int x0, int span, int tile_rows, int tile_src_rows, const float* lut,
                                         float* out, const int32_t* frame_map, const uint8_t* carry, int carry_used, vaura_stream_t s);

/* -------------------------------------------------------------------------------------------
 * Audio preprocessing (csrc/audio_pre.hip): decoded PCM -> the codec's padded mono input.  The `audio_transforms_test` list of
 * configs/generate_vas.yaml:43-54 (AudioStereoToMono -> AudioResample(44100) -> AudioTrim; models/data/transforms/
 * audio_transforms.py:162-192, the resampler being torchaudio.transforms.Resample at its defaults) in one launch.  One source rate,
 * one channel count and one sample format per call; per-clip sample counts.
 *   pcm       B clips of C channels: planar (B, C, in_stride) or, interleaved != 0, (B, in_stride, C) as a decoder hands it over;
 *             format VAURA_PCM_S16 (x / 32768), VAURA_PCM_S32 (x / 2147483648) or VAURA_PCM_F32 (as is); aligned to its element
 *   n_in      device, (B) int32: the real samples of clip b (held to 0 .. in_stride); nothing at or behind them is read
 *   o, n, w   orig / gcd, new / gcd and the half width ceil(6 o / (0.99 min(o, n))) of the full form's 2 w + o taps per phase
 *   table     built by the host once per rate pair (vaura_amd/audio_preprocess.py: resample_table): for phase p the taps
 *             taps[j * phases + p], j < taps_per_phase (fp32, tap-major), are taps first[p] .. of the full form, the run outside of
 *             which every fp32 tap is exactly 0; phases == n.  o == n is the identity (the mono signal): the table is not read
 *             and may be NULL.
 *   out       fp32 (B, out_stride): clip b's n_out[b] samples (device int32, held to 0 .. out_stride; the host has applied the
 *             trim), 0 from there to the row's end.  Nothing outside the B rows is written.
 * Arithmetic, all fp32: channels added in channel order, divided by C; output m = q n + p is the sum over the taps, in tap order,
 * of tap * x[q o + first[p] + j - w], x = 0 outside [0, n_in[b]).
 * VAURA_ERR_ARG: a NULL or misaligned pointer, a size below 1, phases != n.  VAURA_ERR_DTYPE: an unknown format.  VAURA_ERR_SHAPE, before any
 * launch: C > 8; more than VAURA_AUDIO_PRE_MAX_TAPS (64) taps per phase; more than 2^20 table entries; a row of more than
 * 2^31 - 1 samples; more than 65535 clips; a tile whose input span does not fit 64 KiB of LDS (vaura_audio_preprocess_lds_bytes).   */
#define VAURA_AUDIO_PRE_TILE 1024
#define VAURA_AUDIO_PRE_MAX_TAPS 64
enum { VAURA_PCM_S16 = 0, VAURA_PCM_S32 = 1, VAURA_PCM_F32 = 2 };
int vaura_audio_preprocess(const void* pcm, int format, int interleaved, int B, int C, int64_t in_stride, const int32_t* n_in, int o, int n,
                           int w, const int32_t* first, const float* taps, int phases, int taps_per_phase, float* out, int64_t out_stride,
                           const int32_t* n_out, vaura_stream_t s);
/* dynamic LDS bytes of one workgroup: the mono input span of one tile (0 for sizes the kernel does not take) */
size_t vaura_audio_preprocess_lds_bytes(int o, int n, int w, int taps_per_phase);
/* output samples per workgroup (VAURA_AUDIO_PRE_TILE as the library was compiled) */
int vaura_audio_preprocess_tile(void);

/* -------------------------------------------------------------------------------------------
 * Audio output (csrc/audio_out.hip): the codec's mono fp32 rows at 44.1 kHz -> PCM at the consumer's rate, format and channel
 * layout, in one launch; one pass or block by block with the filter history carried, the blocks concatenated being the one-pass
 * result bit for bit.
 *   x         fp32 (B, in_stride): clip b's block of the stream, samples [r0, r0 + L) of the clip
 *   records   device, (B, VAURA_AUDIO_OUT_RECORD) int64, 8-byte aligned: r0, L (held to 0 .. in_stride), m0, count (held to
 *             0 .. out_stride), N.  The launch forms the outputs [m0, m0 + count) of clip b, absolute indices at the output rate, and
 *             writes them from the start of the clip's row.  N >= 0 is the clip's total input length (this is its last block); N < 0:
 *             not known yet.  x[s] is 0 for s < 0 and, when N >= 0, for s >= N; nothing at or behind r0 + L is read.
 *   carry_in  fp32 (B, history): samples [r0 - history, r0) of clip b (zeros in front of the stream's start); NULL with history == 0
 *   carry_out fp32 (B, history) or NULL: receives the last `history` samples of carry_in ++ block, written by extra workgroups of the
 *             same launch.  It must not overlap carry_in (a ping-pong pair; VAURA_ERR_ARG when the two (B, history) spans do).
 *   THE HOST RULE IS PART OF THE CONTRACT.  The kernel serves 0 for an index below the carry row and for one at or behind r0 + L of a
 *             block that is not final, and it holds the start of a tap run inside the span it staged: memory safety, not arithmetic.
 *             That no requested output ever needs such an index is the caller's to guarantee — `history` at least
 *             vaura_amd/audio_out.py: history() of the rate pair, and m0 + count at most releasable(r0 + L) for a block that is not
 *             final (output_total(N) for a final one).  A smaller history or a larger count gives wrong samples, silently.
 *             vaura_amd/post.py (audio_to_pcm, PcmStream) is the caller that keeps the rule.
 *   o, n, w, first, taps, phases, taps_per_phase   the table of the rate pair 44100 -> rate as for vaura_audio_preprocess
 *             (resample_table(44100, rate)); o == n is the identity, the table is not read and may be NULL.
 *   gain      device fp32 (B): one factor per clip
 *   out       format VAURA_PCM_S16 / S32 / F32, C_out (1 .. 8) copies of the mono value: planar (B, C_out, out_stride) or,
 *             interleaved != 0, (B, out_stride, C_out); zeros from `count` to the row's end; nothing outside the B rows is written.
 *             out_stride == 0 writes no output (out may be NULL): only the carry moves.
 *   clipped   device int32 (B), ADDED to (the caller zeroes it): samples whose y * scale lay outside the format's range or was NaN
 * Arithmetic, all fp32: acc = 0, then acc = fmaf(tap_j, x[q o + first[p] - w + j], acc) in tap order for output m = q n + p;
 * y = acc * gain[b]; S16 = rint(y * 32768), S32 = rint(y * 2^31) (half to even, saturated; NaN -> 0), F32 = y (counted outside
 * [-1, 1], not altered).
 * VAURA_ERR_ARG: a NULL required pointer or a misaligned one, B < 1, a negative length, in_stride == 0, phases != n.  VAURA_ERR_DTYPE: an
 * unknown format.  VAURA_ERR_SHAPE: C_out outside 1 .. 8; more than 64 taps per phase; more than 2^20 table entries; a row of more
 * than 2^31 - 1 samples; more than 65535 clips; a tile whose input span does not fit 64 KiB of LDS.  All before any launch and without
 * dereferencing anything.                                                                                                          */
#define VAURA_AUDIO_OUT_TILE 1024
#define VAURA_AUDIO_OUT_RECORD 5
int vaura_audio_output(const float* x, int B, int64_t in_stride, const int64_t* records, const float* carry_in, float* carry_out,
                       int history, int o, int n, int w, const int32_t* first, const float* taps, int phases, int taps_per_phase,
                       const float* gain, int format, int interleaved, int C_out, void* out, int64_t out_stride, int32_t* clipped,
                       vaura_stream_t s);
/* dynamic LDS bytes of one workgroup of that launch (0 for sizes the kernel does not take) */
size_t vaura_audio_output_lds_bytes(int o, int n, int w, int taps_per_phase);
/* output samples per workgroup (VAURA_AUDIO_OUT_TILE as the library was compiled) */
int vaura_audio_output_tile(void);

/* -------------------------------------------------------------------------------------------
 * Spectrogram (csrc/spectrogram.hip): the codec's mono fp32 rows at 44.1 kHz -> power, dB or log columns of the linear or the mel
 * spectrum, in one launch; one pass or block by block with the window history carried, the blocks concatenated being the one-pass
 * result bit for bit.  Column t of a clip is centred on sample hop t + hop/2 and covers lo = hop t + hop/2 - n_fft/2 ..
 * lo + n_fft - 1 (x is 0 outside the clip); with hop 512 it is codec frame t.  All fp32: y[i] = window[i] x[lo + i]; X = the
 * n_fft-point transform of y, bins 0 .. n_fft/2; P = re re + im im; M[m] = fmaf chain of f[m][k] P[k] over the filter's bins in
 * ascending order; then the scale: VAURA_SPEC_POWER v, VAURA_SPEC_DB 10 log10f(max(v, amin)), VAURA_SPEC_LOG logf(max(v, amin)); a
 * NaN stays a NaN.  VAURA_SPEC_COMPLEX (without a mel table only) gives X itself: out is (B, out_stride, F, 2), (re, im) pairs.
 *   x, records, carry_in, carry_out, history   as for vaura_audio_output, the record being r0, L, t0, count, N: the launch forms the
 *             columns [t0, t0 + count) of clip b and writes them from the start of the clip's rows.  The host rule is the same:
 *             `history` at least n_fft - 1 and t0 + count at most vaura_amd/spectrogram.py: releasable(r0 + L) for a block that is
 *             not final (columns(N) for a final one); vaura_amd/post.py (audio_to_spectrogram, SpectrogramStream) keeps it.
 *   n_fft     512, 1024 or 2048;  hop  a power of two, at most n_fft
 *   window    device fp32 (n_fft);  twiddles  device fp32 (3 n_fft / 4, 2), 8-byte aligned: cos and -sin of 2 pi t / n_fft
 *   mel_bins  device int32 (F, 3): first bin, count, offset into mel_weights of every filter (the kernel holds them inside
 *             0 .. n_fft/2 and inside the mel_total weights); mel_weights device fp32 (mel_total), the filters' weights packed in
 *             filter order.  Both NULL: the linear spectrum, F == n_fft/2 + 1.
 *   out       fp32 (B, out_stride, F), time-major: row i of clip b is column t0 + i, zeros from `count` to out_stride; nothing
 *             outside is written.  out_stride == 0 writes no column (out may be NULL): only the carry moves.
 * VAURA_ERR_ARG: a NULL required pointer or a misaligned one, one half of the mel table without the other, VAURA_SPEC_COMPLEX with a mel table, overlapping carry spans,
 * B < 1, a negative length, in_stride == 0, amin not above 0.  VAURA_ERR_DTYPE: an unknown scale.  VAURA_ERR_SHAPE: another n_fft; a
 * hop that is no power of two or exceeds n_fft; F above VAURA_SPECTROGRAM_MAX_MELS, or not n_fft/2 + 1 without a table; a table
 * with fewer than F or more than F (n_fft/2 + 1) weights (a filter without a bin, or a support that leaves 0 .. n_fft/2); a row of
 * more than 2^31 - 1 samples; more than 65535 clips.  All before any launch and without dereferencing anything.               */
#define VAURA_SPECTROGRAM_RECORD 5
#define VAURA_SPECTROGRAM_MAX_MELS 256
enum { VAURA_SPEC_POWER = 0, VAURA_SPEC_DB = 1, VAURA_SPEC_LOG = 2, VAURA_SPEC_COMPLEX = 3 };
int vaura_spectrogram(const float* x, int B, int64_t in_stride, const int64_t* records, const float* carry_in, float* carry_out,
                      int history, int n_fft, int hop, const float* window, const float* twiddles, const int32_t* mel_bins,
                      const float* mel_weights, int mel_total, int F, int scale, float amin, float* out, int64_t out_stride,
                      vaura_stream_t s);
/* dynamic LDS bytes of one workgroup of that launch: the two images of the transform (0 for sizes the kernel does not take) */
size_t vaura_spectrogram_lds_bytes(int n_fft, int F);

/* -------------------------------------------------------------------------------------------
 * Streaming loudness (csrc/loudness.hip): an ITU-R BS.1770 meter and a causal loudness normaliser over the codec's mono fp32 rows, one
 * pass or block by block, the blocks concatenated being the one-pass result bit for bit.  step = nearbyint(0.1 rate), gate = 4 step.
 * The K-weighting runs in fp64 (coefficients of vaura_audio_loudness's launcher, kept in double), parallel over 256 lane chunks per
 * step that are anchored at absolute sample indices; step energies S_j are fp32 in a ring of max(history_steps, 32) entries; the
 * momentary (4 steps), short-term (30 steps) and integrated (two gates, the blocks of the last history_steps steps) loudness use
 * post.hip's fp32 expressions.  At boundary m (m whole steps received) d_m = clamp(target_lkfs - I_m, +-max_gain_db), held where I_m
 * is undefined, slew-limited by slew_db_per_step where that is > 0; a_m = powf(10, d_m / 20); sample i of step m, offset k, leaves
 * as limiter(x (a_{m-1} + (a_m - a_{m-1}) (k + 1) / step)): every pushed sample leaves in the same push.
 *   x         device fp32 (B, in_stride): the next samples of every clip;  records  device int64 (B, VAURA_LOUDNESS_RECORD): r0 =
 *             samples the clip has brought before, n = samples it brings now (0 .. in_stride; nothing behind n is read).  The host
 *             keeps r0 (vaura_amd/loudness.py push_records); a clip's first push (r0 == 0) reads no state.
 *   out       device fp32 (B, in_stride), not x: the n normalised samples of every row, zeros behind them; NULL: the meter alone
 *   state     device, vaura_audio_loudness_state_elems(B, rate, history_steps) fp32 words, 8-byte aligned: per clip the filter
 *             state (8 doubles), d, a_{m-1}, a_m, I, the ring and the raw tail shorter than one step.  Owned by the stream.
 *   table     device fp64, vaura_audio_loudness_table_elems(rate) values (vaura_amd/loudness.py: table())
 *   gains     device fp32 (B, meter_stride + 2), written: a_{M0-1}, a_{M0}, .. a_{M1} with M0 = r0 / step, M1 = (r0 + n) / step
 *   meter     device fp32 (3, B, meter_stride), written: plane 0 I_m at the boundaries m = M0 + 1 .. M1; plane 1 the momentary
 *             loudness of the blocks those boundaries complete (block m - 4), left-aligned; plane 2 the short-term values (window
 *             m - 30) likewise; NaN where undefined and behind them.  meter_stride >= the largest M1 - M0 of the push, >= 1.
 *   info      device fp32 (B, 2), written: d and I at the clip's last boundary;  clipped  device int32 (B), ADDED to: |x g| > 1
 * One launch where in_stride <= 16384, two otherwise.  VAURA_ERR_ARG: a NULL or misaligned pointer, out == x, B < 1, in_stride < 1,
 * meter_stride < 1, a table of another size, a non-finite target / initial gain, max_gain_db negative or not finite, a negative or
 * NaN slew.  VAURA_ERR_DTYPE: an unknown limiter.  VAURA_ERR_SHAPE: a rate outside 8 .. 48 kHz or one whose gating block is not
 * four whole steps (11 025 Hz), history_steps outside 8 .. 4096, a row of more than 2^31 - 1 samples, more than 65535 clips.  All
 * before any launch.                                                                                                            */
#define VAURA_LOUDNESS_RECORD 2
#define VAURA_LOUDNESS_MIN_HISTORY 8
#define VAURA_LOUDNESS_MAX_HISTORY 4096
enum { VAURA_LOUDNESS_CLIP = 0, VAURA_LOUDNESS_TANH = 1 };
int vaura_audio_loudness_push(const float* x, float* out, int B, int64_t in_stride, const int64_t* records, float* state,
                              int sample_rate, int history_steps, const double* table, int64_t table_elems, float target_lkfs,
                              float max_gain_db, float slew_db_per_step, float initial_gain_db, int limiter, float* gains, float* meter,
                              int meter_stride, float* info, int32_t* clipped, vaura_stream_t s);
/* fp32 words of the state of n_clips clips (0 for a rate or a history the launcher refuses) */
size_t vaura_audio_loudness_state_elems(int n_clips, int sample_rate, int history_steps);
/* fp64 values of the chunk table of a rate (0 for a refused rate) */
size_t vaura_audio_loudness_table_elems(int sample_rate);
/* LDS bytes of one workgroup of the push kernel, dynamic and static (0 for a refused rate) */
size_t vaura_audio_loudness_lds_bytes(int sample_rate);

/* Measurement aid (tools/pmc_driver, A/B timing): selects kernel variants for launches enqueued (or graphs captured) afterwards.
 * vaura_amd/csrc/variants.h is the table of every bit of both words, by name (e.g. bit 0, ROWSPLIT_OFF: wo / w2 GEMVs as one workgroup
 * per column tile instead of the row-split pair); an entry never changes its value.  0 = the product configuration.   */
void vaura_set_debug_flags(unsigned flags);
/* A second word of the same kind, in the same table.  0 = the product. */
void vaura_set_debug_flags2(unsigned flags);
/* Host-side launch counters for tests that must know WHICH kernel instance a call took (read-and-clear; single caller thread):
 * 0 = codec conv launches on the 256-row workgroup instances (conv_pair_kernel<..., 8>, csrc/dac.hip) since the last read.
 * Unknown `which` -> -1. */
long long vaura_debug_counter(int which);

const char* vaura_version(void);
/* sizeof() of the descriptor structs as compiled into the library (0 dims, 1 layer_weights, 2 sampling, 3 decoder,
 * 4 conv, 5 codec, 6 codec_encoder, 7 vit, 8 vit_block, 9 clip_sampling, 10 decoder_ext, 11 decoder_ext2, 13 decoder_ext3; 12 is
 * unassigned and answers 0 like every unknown index): a binding checks its mirrored struct layouts against these before the first call.            */
size_t vaura_struct_size(int which);

#ifdef __cplusplus
}
#endif
#endif /* VAURA_HIP_H */
