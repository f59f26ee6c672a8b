// Kernel-variant switches: THE table of both words of vaura_set_debug_flags / vaura_set_debug_flags2 (A/B timing and the bit-identity
// tests; the product runs with both words 0).  Every host read of either word goes through va_variant / va_variant_field below;
// vaura_amd/variants.py mirrors names and values and tests/test_variants_host.py holds the two together.  The numeric values are what
// tools/pmc_driver --flags, VAURA_DEBUG_FLAGS / VAURA_DEBUG_FLAGS2 and the records under profiles/ use: an entry never moves.
// Free: word 1 bits 3, 6, 8, 12; word 2 bits 2, 7..11, 16..31.
#pragma once
#include "../../include/vaura_hip.h"

//  X(name, word, bit, effect)                                                                      one-bit switches
#define VA_VARIANTS(X)                                                                                                                 \
  X(ROWSPLIT_OFF, 1, 0, "wo / w2 on the one-workgroup-per-tile GEMV instead of the row-split pair")                                    \
  X(QKV_OWN_LAUNCH, 1, 1, "the next layer's qkv GEMV stays its own launch (not the MLP launch's third phase)")                         \
  X(MLP_TWO_LAUNCHES, 1, 2, "w1||w3 and w2 as two launches even where the one-launch MLP (mlp_engine.h) is eligible")                  \
  X(PREFILL_ATTN_PER_POSITION, 1, 4, "fp32 cache: per-position prefill attention instead of the MFMA kernel")                          \
  X(PREFILL_GEMM_64_ROWS, 1, 5, "64-row prefill GEMM workgroups only")                                                                 \
  X(VIT_SPACE_THREAD_PER_QUERY, 1, 7, "extractor space attention with one thread per query instead of the MFMA kernels")               \
  X(VIT_CLS_UNSPLIT, 1, 9, "extractor CLS attention on the one-workgroup-per-(sequence, head) kernel")                                 \
  X(VIT_TIME_THREAD_PER_HEAD_FRAME, 1, 10, "extractor time attention with one thread per (head, frame)")                               \
  X(VIT_SPACE_FP32_MFMA, 1, 11, "extractor space attention on the exact-fp32 MFMA instead of fp16 pairs")                              \
  X(CODEC_LAST_CONV_UNTILED, 1, 13, "the codec's last conv (C -> 1) without the LDS-staged window")                                    \
  X(GEMM3_ROUND2_TILE_RULE, 1, 14, "gemm3_kernel only: round 2's tile rule (128-row workgroups from 64 row blocks up)")                \
  X(PREFILL_GEMM_LAUNCH_ORDER, 1, 15, "prefill GEMM workgroups in launch order (no XCD tile order)")                                   \
  X(GEMM3_ONE_KGROUP, 1, 16, "gemm3_kernel only: one k-group of planes and weights in flight")                                         \
  X(PREFILL_GEMM_REGISTER_STAGED, 1, 17, "prefill GEMMs on the register-staged gemm3_kernel for every storage (fp8 always uses it)")   \
  X(GEMM4_NO_DMA, 1, 18, "gemm4_kernel ablation for tools/time_prefill_gemm.py: no DMA in the loop (WRONG RESULTS, timing only)")      \
  X(ATTN_MERGE_OWN_LAUNCH, 1, 19, "range-split attention: the merge of the partials as its own launch, not by the last split to arrive") \
  X(CODEC_128_ROWS, 1, 20, "codec convs in 128-row workgroups only (no 256-row instances, no one-launch residual units)")              \
  X(CODEC_UNIT_TWO_LAUNCHES, 1, 21, "codec residual units as two launches even where one workgroup holds every channel (C = 96, 192)") \
  X(PREFILL_GEMM_NO_CUT, 1, 22, "prefill GEMMs never cut into two launches of different workgroup heights")                            \
  X(PREFILL_GEMM_64x256, 1, 23, "two-plane prefill GEMMs with few column tiles (wo, w2) in 64 x 256 workgroups instead of 128 x 128")  \
  X(ROW_BLOCKS_WALK, 2, 0, "17..32 decoder rows: the GEMVs walk the two row blocks one after the other instead of both per weight pass") \
  X(ENGINE_MAX_16_ROWS, 2, 1, "the one-launch MLP refuses more than 16 rows (the separate two-row-block launches run instead)")        \
  X(FP8_ROWSPLIT_OFF, 2, 3, "fp8 weights, 17..32 rows: wo / w2 on one workgroup per tile instead of the fp8 row-split pair instances") \
  X(FP8_NO_ENGINE, 2, 4, "fp8 weights never take the one-launch MLP")                                                                  \
  X(LINEAR_REGISTER_STAGED, 2, 5, "extractor linear layers on the register-staged linear_pair_kernel, not linear_dma_kernel (bit-identical)") \
  X(LINEAR_DMA_LATE_FRAGMENTS, 2, 6, "extractor linear layers: LDS-DMA kernel with the fragments read beside their matrix instructions")

//  X(name, word, shift, width, effect)                                                             fields; 0 = the product's choice
#define VA_VARIANT_FIELDS(X)                                                                                                           \
  X(GRAPH_STEPS, 1, 24, 4, "decode steps per graph launch (1..15; 0 = the default VA_GRAPH_STEPS), read by vaura_step_graph_build")    \
  X(ENGINE_ABL, 1, 28, 4, "MlpEngineArgs::abl, timing only: 1 = no flag waits (WRONG RESULTS); 4: see the struct; 8 = no run-ahead throttle") \
  X(LINEAR_PANEL, 2, 12, 4, "extractor linear layers: column-tile panel of n tiles where n divides the tile count (15 = the whole width)")

enum VaVariant : unsigned {      // (word - 1) * 32 + bit
#define X(name, word, bit, effect) VV_##name = ((word) - 1) * 32 + (bit),
  VA_VARIANTS(X)
#undef X
};
enum VaVariantField : unsigned {      // (width << 8) | (word - 1) * 32 + shift
#define X(name, word, shift, width, effect) VF_##name = ((width) << 8) | (((word) - 1) * 32 + (shift)),
  VA_VARIANT_FIELDS(X)
#undef X
};

constexpr bool va_variants_disjoint() {
  unsigned seen[2] = {0u, 0u};
  bool ok = true;
#define X(name, word, bit, effect) ok = ok && (word) >= 1 && (word) <= 2 && (bit) < 32 && !(seen[(word) - 1] >> (bit) & 1u), seen[(word) - 1] |= 1u << (bit);
  VA_VARIANTS(X)
#undef X
#define X(name, word, shift, width, effect)                                                                                  \
  ok = ok && (word) >= 1 && (word) <= 2 && (width) >= 1 && (shift) + (width) <= 32 &&                                        \
       !(seen[(word) - 1] & (unsigned)(((1ull << (width)) - 1) << (shift))),                                                 \
  seen[(word) - 1] |= (unsigned)(((1ull << (width)) - 1) << (shift));
  VA_VARIANT_FIELDS(X)
#undef X
  return ok;
}
static_assert(va_variants_disjoint(), "two kernel-variant switches overlap within a word (or leave it)");

unsigned va_debug_flags_get();   // the words live in gemv3.hip, beside their exported setters (vaura_hip.h)
unsigned va_debug_flags2_get();

inline bool va_variant(VaVariant v) { return ((v < 32 ? va_debug_flags_get() : va_debug_flags2_get()) >> (v & 31u)) & 1u; }
inline unsigned va_variant_field(VaVariantField f) {
  return (((f & 255u) < 32 ? va_debug_flags_get() : va_debug_flags2_get()) >> (f & 31u)) & ((1u << (f >> 8)) - 1u);
}

// Both words as one value, and "run this scope as that variant": a handle built under one setting (StepGraph, api.hip) enqueues its
// later launches under the same one whatever the caller has set since, and every way out of the scope puts the caller's words back.
struct VaVariantWords {
  unsigned w1 = 0, w2 = 0;
  static VaVariantWords current() { return {va_debug_flags_get(), va_debug_flags2_get()}; }
  void set() const { vaura_set_debug_flags(w1); vaura_set_debug_flags2(w2); }
};
class VaVariantScope {
  const VaVariantWords saved = VaVariantWords::current();
 public:
  explicit VaVariantScope(const VaVariantWords& w) { w.set(); }
  ~VaVariantScope() { saved.set(); }
  VaVariantScope(const VaVariantScope&) = delete;
  VaVariantScope& operator=(const VaVariantScope&) = delete;
};
