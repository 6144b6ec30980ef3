// Which flash-attention kernel takes which layout, the plan of the backward
// and the tile bounds of the document mask: plain C++17 with no HIP call (the
// bounds constexpr, so device code may call them), so the kernel library and
// the stand-alone host programs (native/kernels/tests/) share it.
// Every launcher and dispatcher of attention_*.hip asks these predicates;
// pointer alignment, which a layout does not carry, stays at the entry points.
#pragma once

namespace {
constexpr int D = 128;      // head dim
constexpr int BQ = 128;     // query rows per workgroup of the 128-row kernels (4 waves x 32)
constexpr int KBLK = 256;   // keys per workgroup of the 256-key dK/dV kernel
constexpr int QW = 64;      // query rows per wave (and per head) of the 256-row dQ kernel
constexpr int QUAD = 4;     // query heads per workgroup of the 256-row dQ kernel
constexpr int QB = 256;     // query rows per workgroup of forward variant 10
// a buffer resource (LDS-DMA loads, buffer stores) addresses 32-bit byte offsets
constexpr long BUF_RANGE = 1L << 32;

// q / dq [B, S, Hq, 128], k / v / dk / dv [B, S, Hkv, 128] at token strides
// (elements); o, dout and the plain backward's dq are contiguous
struct AttnLayout {
  int B, S, Hq, Hkv;
  long q_tok, k_tok, v_tok, dq_tok, dk_tok, dv_tok;
  int causal;
};

// S rows of `tok` bf16 elements each stay inside one buffer resource
inline bool attn_fits(const AttnLayout& L, long tok) {
  return static_cast<long>(L.S) * tok * 2 < BUF_RANGE;
}
// what every kernel asks: whole blocks of `blk` rows, GQA groups, 16-B rows
inline bool attn_shape_ok(const AttnLayout& L, int blk) {
  return L.B >= 1 && L.S >= blk && L.S % blk == 0 && L.Hkv >= 1 && L.Hq % L.Hkv == 0 &&
         L.q_tok % 8 == 0 && L.k_tok % 8 == 0 && L.v_tok % 8 == 0;
}
inline bool attn_fwd_ok(const AttnLayout& L) { return attn_shape_ok(L, BQ); }
inline bool attn_bwd_ok(const AttnLayout& L) {
  return attn_shape_ok(L, BQ) && L.dk_tok % 4 == 0 && L.dv_tok % 4 == 0;
}
// K / V tiles by LDS-DMA (forward variants 1-4, the 128-row dQ kernel's DMA
// forms): the K/V span
inline bool attn_kv_dma_ok(const AttnLayout& L) {
  return attn_fits(L, L.k_tok > L.v_tok ? L.k_tok : L.v_tok);
}
// Q / dO tiles by LDS-DMA (the 16x16 dK/dV kernel's DMA forms): the Q span
inline bool attn_q_dma_ok(const AttnLayout& L) {
  const long o_tok = static_cast<long>(L.Hq) * D;
  return attn_fits(L, L.q_tok > o_tok ? L.q_tok : o_tok);
}
inline bool attn_fwd256_ok(const AttnLayout& L) {   // forward variant 10
  return attn_shape_ok(L, QB) && attn_fits(L, L.k_tok) && attn_fits(L, L.v_tok);
}
inline bool attn_dq256_ok(const AttnLayout& L) {   // 256-row dQ
  return attn_shape_ok(L, QW) && (L.Hq / L.Hkv) % QUAD == 0 && attn_fits(L, L.k_tok) &&
         attn_fits(L, L.v_tok);
}
inline bool attn_dq256_rope_ok(const AttnLayout& L) {   // ... with dQ at a token stride
  return attn_dq256_ok(L) && L.dq_tok >= static_cast<long>(L.Hq) * D && L.dq_tok % 8 == 0;
}
// 256-key dK/dV: the plain, the RoPE and the one-pass (dQ by atomics) forms
// take the same layouts
inline bool attn_dkdv256_ok(const AttnLayout& L) {
  return attn_shape_ok(L, KBLK) && L.dk_tok % 4 == 0 && L.dv_tok % 4 == 0 &&
         attn_fits(L, L.q_tok) && attn_fits(L, L.k_tok) &&
         attn_fits(L, static_cast<long>(L.Hq) * D);
}

// ---------------------------------------------------------------------------
// Packed sequences: causal attention within a document.  doc_start[b][i] is
// the first token of the document token i belongs to, doc_end[b][j] the
// (exclusive) end of j's document; both int32 [B, S] and non-decreasing along
// a row.  Query i sees key j iff doc_start[i] <= j <= i, which for j <= i is
// the same as i < doc_end[j].  The DOC forms of forward variant 4 and backward
// variant 5 (mxk_attn_fwd_doc / mxk_attn_bwd_doc) are the LDS-DMA kernels
// only: there is no register-staged fallback.
inline bool attn_doc_ok(const AttnLayout& L) {
  return L.causal && attn_bwd_ok(L) && attn_kv_dma_ok(L) && attn_q_dma_ok(L);
}
// The tile / slice bounds those kernels derive from the tables, constexpr so
// that the kernels and the host test share one definition.  Every result is
// clamped into the causal range, whatever the table holds: a malformed table
// gives wrong numbers, never an index outside the tensors.
constexpr int attn_clampi(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }
// forward / dQ: the first `tile`-key tile of the K / V walk of the query block
// at row q0 (ds_q0 = doc_start[q0], the smallest of the block), a multiple of
// `align` tiles (2 for a loop unrolled by two over static LDS buffers); the
// walk ends at the diagonal tile (q0 + BQ) / tile - 1 as without a table
constexpr int attn_doc_first_tile(int ds_q0, int q0, int tile, int align) {
  return attn_clampi(ds_q0, 0, q0) / (tile * align) * align;
}
// a wave whose first row's document starts at ds_first has a visible key in
// the tile at kv0 (the causal test is separate)
constexpr bool attn_doc_tile_active(int kv0, int tile, int ds_first) { return kv0 + tile > ds_first; }
// ... and needs the per-score mask key < doc_start[row] there (ds_last: of its last row)
constexpr bool attn_doc_tile_masked(int kv0, int ds_last) { return kv0 < ds_last; }
// dK / dV: `slice`-row query slices the key block at k0 walks from the
// diagonal (de_last = doc_end[k0 + BQ - 1], the largest of the block)
constexpr int attn_doc_slices(int de_last, int k0, int S, int slice) {
  return (attn_clampi(de_last, k0 + BQ, S) - k0 + slice - 1) / slice;
}
// a wave whose last key's document ends at de_last has a visible query row in
// the slice at qs0 (the causal test is separate)
constexpr bool attn_doc_slice_active(int qs0, int de_last) { return qs0 < de_last; }
// ... and needs the per-score mask row >= doc_end[key] there (de_first: of its first key)
constexpr bool attn_doc_slice_masked(int qs0, int slice, int de_first) {
  return qs0 + slice > de_first;
}

// ---------------------------------------------------------------------------
// Backward variants (MXK_ATTN_BWD_VARIANT, attn_bwd(variant=)), newest first.
// Timings are per Llama-3-8B layer at B 8.
//   9 (default): dQ by workgroups of the 4 query heads of a GQA quad x 64
//      rows, one wave per SIMD (attention_dq256.hip: Q / dO resident as MFMA
//      operands in the accumulator file, K / V by LDS-DMA shared by the four
//      heads, dO / O / Q staged through LDS, the delta pass folded in), then
//      variant 6's 256-key dK / dV: bit-identical to 6 and 1-3 % faster
//      (1.02-1.04 vs 1.045-1.057 ms, profiles/r6_dq256/SUMMARY.md).
//   8: one pass, dQ added by packed-bf16 atomics from the 256-key workgroups
//      (0.983 ms; dQ summed in bf16 in a nondeterministic order); 7: the same
//      with fp32 atomics and a convert pass (1.139 ms).
//   6: variant 5's dQ kernel (it also writes the row constants -lse/scale and
//      -delta), then dK / dV by the 256-key workgroups of attention_bwd256.hip
//      (one wave per SIMD, dK^T / dV^T in accumulators, S / dP of both key
//      tiles from one read of each Q / dO fragment, a key tile's softmax and
//      dK / dV pipelined into the next step): 1.018 vs 1.044 ms for 5,
//      deterministic (profiles/r5_attention/).
//   5: variant 3 with the delta pass (dO . O per query row) folded into the
//      dQ kernel, which then runs before dK/dV: no separate delta kernel,
//      1.042 vs 1.064 ms (profiles/r4_final/attention_b8.log).
//   4: 3 with the dQ loop unrolled by two (compile-time LDS buffer),
//      bit-identical and within noise (1.1487 vs 1.1525 ms).
//   3: variant 2 with explicitly software-pipelined dK/dV and dQ bodies (LDS
//      operands read a group ahead instead of one lgkmcnt(0) per MFMA),
//      bit-identical to 2 and 15 % faster (1.070 vs 1.262 ms,
//      profiles/r2_attention/).
//   2: dK/dV accumulated over the query-head group in one workgroup, bf16
//      out, K/V and Q/dO tiles by LDS-DMA (1.21 vs 1.31-1.36 ms,
//      profiles/r1_attention/); 1: the same with register-staged tiles.
//   0: per-query-head fp32 dK/dV partials + GQA reduce.
// A layout a variant's kernels do not take degrades: 9 -> 6 -> 5, 7 / 8 -> 5,
// and within 0-5 a kernel whose panel exceeds BUF_RANGE runs register-staged.
// ---------------------------------------------------------------------------
enum AttnDq : int {   // mxk_attn_bwd_dq_kernel<CAUSAL, ...> unless said otherwise
  DQ_REG,               // <C, false>
  DQ_DMA,               // <C, true>
  DQ_DMA_PIPE,          // <C, true, true>
  DQ_DMA_PIPE_UNROLL,   // <true, true, true, true>: causal only
  DQ_FOLD,              // <C, true, true, false, true>
  DQ_FOLD_ROWC,         // <C, true, true, false, true, true>
  DQ_256,               // mxk_attn_bwd_dq256
  DQ_ATOMICS,           // by the one-pass dK/dV kernel
};
enum AttnDkdv : int {   // mxk_attn_bwd_dkdv16_kernel<CAUSAL, ...> unless said otherwise
  DKDV_HEAD,           // <C, false>: per query head, B*Hq*(S/128) workgroups, fp32 partials
  DKDV_GQA,            // <C, true>
  DKDV_GQA_DMA,        // <C, true, true>
  DKDV_GQA_DMA_PIPE,   // <C, true, true, true>
  DKDV_256,            // mxk_attn_bwd_dkdv256
  DKDV_ONEPASS_F32,    // mxk_attn_bwd_onepass, fp32 atomics + convert
  DKDV_ONEPASS_BF16,   // mxk_attn_bwd_onepass, packed-bf16 atomics
};
// The stages in launch order: [delta] -> dQ if dq_first -> dK/dV -> dQ if not
// dq_first -> [reduce].
struct AttnBwdPlan {
  int variant;      // resolved; -1: arguments no variant takes
  int delta;        // the stand-alone delta kernel runs
  AttnDq dq;
  AttnDkdv dkdv;
  int reduce;       // GQA reduce of the per-head partials
  int dq_first;     // dQ writes delta / the rowc pairs dK/dV reads
  long workspace;   // bytes the resolved stages use
};

// delta [B*Hq*S] fp32, or {-lse/scale, -delta} rowc pairs for the 256-key
// kernel; + the fp32 dQ accumulator for 7, + 2 x dK/dV partials for 0
inline long attn_bwd_workspace(int B, int S, int Hq, int variant) {
  const long rows = static_cast<long>(B) * Hq * S;
  if (variant == 6 || variant == 8 || variant == 9) return rows * 8;
  if (variant == 7) return rows * 8 + rows * D * 4;
  return rows * 4 + (variant == 0 ? 2 * rows * D * 4 : 0);
}

inline AttnBwdPlan attn_bwd_plan(const AttnLayout& L, int variant) {
  AttnBwdPlan p{-1, 0, DQ_REG, DKDV_HEAD, 0, 0, 0};
  if (!attn_bwd_ok(L) || variant < 0 || variant > 9) return p;
  const bool kv_dma = attn_kv_dma_ok(L), q_dma = attn_q_dma_ok(L), k256 = attn_dkdv256_ok(L);
  if (variant == 7 || variant == 8) {
    if (k256)
      return {variant, 0, DQ_ATOMICS, variant == 8 ? DKDV_ONEPASS_BF16 : DKDV_ONEPASS_F32, 0, 0,
              attn_bwd_workspace(L.B, L.S, L.Hq, variant)};
    variant = 5;   // as 6 does, instead of failing
  }
  if (variant == 9 && !(attn_dq256_ok(L) && k256)) variant = 6;
  if (variant == 6 && !(kv_dma && k256)) variant = 5;
  p.variant = variant;
  p.workspace = attn_bwd_workspace(L.B, L.S, L.Hq, variant);
  if (variant >= 6) {
    p.dq = variant == 9 ? DQ_256 : DQ_FOLD_ROWC;
    p.dkdv = DKDV_256;
    p.dq_first = 1;
    return p;
  }
  p.dq_first = variant == 5 && kv_dma;
  p.delta = !p.dq_first;
  p.reduce = variant == 0;
  p.dkdv = variant >= 3 && q_dma ? DKDV_GQA_DMA_PIPE
           : variant >= 2 && q_dma ? DKDV_GQA_DMA
           : variant >= 1 ? DKDV_GQA : DKDV_HEAD;
  // a non-causal 4 runs 3's dQ instance: the unrolled body exists causal only
  p.dq = !(variant >= 2 && kv_dma) ? DQ_REG
         : variant == 5 ? DQ_FOLD
         : variant == 4 && L.causal ? DQ_DMA_PIPE_UNROLL
         : variant >= 3 ? DQ_DMA_PIPE : DQ_DMA;
  return p;
}
}  // namespace
