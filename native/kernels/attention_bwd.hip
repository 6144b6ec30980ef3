// Flash-attention backward for gfx950: the delta, 128-row dQ, 16x16 dK/dV and
// GQA-reduce kernels of variants 0-6, and the entry points of every variant
// (the plan: attention_plan.h; the 256-row dQ and 256-key dK/dV kernels of
// variants 6-9: attention_dq256.hip, attention_bwd256.hip).  Layouts as
// attention_fwd.hip.
#include "attention_common.h"

// ===========================================================================
// Backward.  Three passes, no atomics (deterministic):
//   1. delta[b][hq][q] = sum_d dO . O                       (mxk_attn_bwd_delta)
//   2. dQ, query-parallel, structured like the forward: per 64-key block
//      S^T = K.Q^T and dP^T = V.dO^T with the query on the lane, P^T from the
//      saved LSE (no max/sum), dS^T = P^T (dP^T - delta), dQ^T += K^T.dS^T
//      (K^T by ds_read_b64_tr_b16 from the same swizzled image).
//   3. dK/dV, key-parallel: one workgroup = 8 waves x 16 keys of one
//      (batch, q-head), sweeping 64-query slices: S = Q.K^T and dP = dO.V^T
//      with the KEY on the lane, so P and dS are already the B operands of
//      dV^T += dO^T.P and dK^T += Q^T.dS (dO^T, Q^T by transposed reads);
//      the accumulator init carries -LSE/scale and -delta, so
//      p = exp2(c * acc) and dS = p * acc' need no extra subtraction.
//      Per-q-head partial dK/dV (fp32) are summed over each GQA group by
//      mxk_attn_bwd_gqa_reduce.
// Recomputing S and dP in both passes costs 7 instead of 5 MFMA products
// per tile but removes the dQ atomics (1.3 TB/s chip-wide would bound the
// pass) and keeps every kernel deterministic.
// ===========================================================================
namespace {
constexpr int BQB = 64;   // queries per slice in the dK/dV kernel
}  // namespace

__global__ void __launch_bounds__(256)
mxk_attn_bwd_delta_kernel(const uint16_t* __restrict__ o, const uint16_t* __restrict__ dout,
                          float* __restrict__ delta, int S, int Hq, long rows) {
  // one 16-lane group per (b, q, hq) row of 128 dims: 8 bf16 per lane
  const long row = (static_cast<long>(blockIdx.x) * 256 + threadIdx.x) >> 4;
  const int sub = threadIdx.x & 15;
  if (row >= rows) return;
  const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(o + row * D + sub * 8);
  const bf16x8_t g = *reinterpret_cast<const bf16x8_t*>(dout + row * D + sub * 8);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e)
    s += mxk::bf2f(static_cast<uint16_t>(a[e])) * mxk::bf2f(static_cast<uint16_t>(g[e]));
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 16);
  if (sub == 0) {
    // row = (b * S + q) * Hq + hq  ->  delta[b][hq][q]
    const long bq = row / Hq;
    const int hq = static_cast<int>(row % Hq);
    const long b = bq / S, qi = bq % S;
    delta[(b * Hq + hq) * S + qi] = s;
  }
}

// DMA: K/V tiles by LDS-DMA straight into the swizzled image (the forward
// kernel's piece mapping, destinations bound to M0) instead of register
// staging - frees the 32 staging VGPRs that made this kernel spill at two
// waves per SIMD, and the ds_writes.  Requires S * token_stride * 2 < 2^32.
// FOLD (backward variant 5): the delta pass folded in - each query row's
// delta = dO . O is computed here from the row's own dO fragments and O (the
// two lanes of a row hold 64 columns each) and written to delta_w for the
// dK/dV kernel, which then runs after this one; no separate delta kernel.
// ROWC (with FOLD; backward variant 6): instead of delta, write the row
// pair {-lse/scale, -delta} that the 256-key dK/dV kernel
// (attention_bwd256.hip) loads as the initial S' / dP' accumulators.
// DOC (mxk_attn_bwd_doc; with CAUSAL, DMA, PIPE and not UNROLL): causal
// within a document, the forward's DOC form - the walk starts at the tile of
// doc_start[q0], a wave skips the tiles before its first row's document, and
// the tiles that begin before its last row's document zero P where
// key < doc_start[row].
template <bool CAUSAL, bool DMA = false, bool PIPE = false, bool UNROLL = false, bool FOLD = false,
          bool ROWC = false, bool DOC = false>
__global__ void __launch_bounds__(NT, 2)
mxk_attn_bwd_dq_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                       const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
                       const float* __restrict__ lse, const float* __restrict__ delta,
                       uint16_t* __restrict__ dq, int S, int Hq, int Hkv, long q_tok, long k_tok,
                       long v_tok, float scale, const uint16_t* __restrict__ o = nullptr,
                       float* __restrict__ delta_w = nullptr,
                       const int* __restrict__ doc_start = nullptr) {
  static_assert(!DOC || (CAUSAL && DMA && PIPE && !UNROLL), "the DOC form extends the FOLD instance");
  __shared__ __attribute__((aligned(16))) char smem[2][2 * TILE_BYTES];   // [buf][K | V]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31;
  const int h = lane >> 5;

  const int nqb = S / BQ;
  int bh, qb;
  map_block_xcd(blockIdx.x, gridDim.x, nqb, Hq / Hkv, CAUSAL, &bh, &qb);
  const int b = bh / Hq, hq = bh % Hq;
  const int hkv = hq / (Hq / Hkv);
  const int q0 = qb * BQ;
  const int qw0 = q0 + wave * 32;
  const int myq = qw0 + r32;

  const uint16_t* qb_ptr = q + static_cast<long>(b) * S * q_tok + static_cast<long>(hq) * D;
  const uint16_t* dob_ptr = dout + static_cast<long>(b) * S * Hq * D + static_cast<long>(hq) * D;
  const uint16_t* kb_ptr = k + static_cast<long>(b) * S * k_tok + static_cast<long>(hkv) * D;
  const uint16_t* vb_ptr = v + static_cast<long>(b) * S * v_tok + static_cast<long>(hkv) * D;

  bf16x8_t qf[8], dof[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8_t*>(qb_ptr + static_cast<long>(myq) * q_tok + 16 * s + 8 * h);
    dof[s] = *reinterpret_cast<const bf16x8_t*>(dob_ptr + static_cast<long>(myq) * Hq * D + 16 * s + 8 * h);
  }
  const float c = scale * 1.4426950408889634f;
  const long lrow = (static_cast<long>(b) * Hq + hq) * S + myq;
  const float lse2 = lse[lrow] * 1.4426950408889634f;
  float dlt;
  if constexpr (FOLD) {
    const uint16_t* ob_ptr = o + static_cast<long>(b) * S * Hq * D + static_cast<long>(hq) * D;
    float part = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bf16x8_t of = *reinterpret_cast<const bf16x8_t*>(ob_ptr + static_cast<long>(myq) * Hq * D +
                                                              16 * s + 8 * h);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        part += mxk::bf2f(static_cast<uint16_t>(dof[s][e])) * mxk::bf2f(static_cast<uint16_t>(of[e]));
    }
    dlt = part + __shfl_xor(part, 32);       // the row's other 64 columns
    if constexpr (ROWC) {
      if (h == 0)
        *reinterpret_cast<float2*>(delta_w + 2 * lrow) = make_float2(-lse[lrow] / scale, -dlt);
    } else {
      if (h == 0) delta_w[lrow] = dlt;
    }
  } else {
    dlt = delta[lrow];
  }

  const int kv_end = CAUSAL ? min(S, q0 + BQ) : S;
  const int nkv = kv_end / BKV;
  // DOC: the block's first tile and the wave's bounds through uniform
  // addresses (scalar loads), the lane's own row with its other row constants
  int j_lo = 0, ds_w0 = 0, ds_w1 = 0, ds_row = 0;
  if constexpr (DOC) {
    const int* ds_b = doc_start + static_cast<long>(b) * S;
    j_lo = attn_doc_first_tile(ds_b[q0], q0, BKV, 1);
    ds_w0 = ds_b[qw0];
    ds_w1 = ds_b[qw0 + 31];
    ds_row = ds_b[myq];
  }
  const int ld_row = tid >> 4, ld_ch = tid & 15;
  bf16x8_t kst[4], vst[4];
  auto load_tile = [&](int j) {
    const long r0 = static_cast<long>(j) * BKV + ld_row;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      kst[i] = *reinterpret_cast<const bf16x8_t*>(kb_ptr + (r0 + 16 * i) * k_tok + ld_ch * 8);
      vst[i] = *reinterpret_cast<const bf16x8_t*>(vb_ptr + (r0 + 16 * i) * v_tok + ld_ch * 8);
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = swz(ld_row + 16 * i, ld_ch);
      *reinterpret_cast<bf16x8_t*>(smem[buf] + off) = kst[i];
      *reinterpret_cast<bf16x8_t*>(smem[buf] + TILE_BYTES + off) = vst[i];
    }
  };
  // DMA pieces: wave w moves 1-KiB pieces g = 4w + p (rows 4g .. 4g+3) of K
  // and V, lane i at row 4g + (i >> 4), chunk (i & 15) ^ ((i >> 4) << 2 | p)
  mxk::u32x4 rk{}, rv{};
  uint32_t kvo[4] = {}, vvo[4] = {};
  const uint32_t sm32 = mxk::lds_addr32(&smem[0][0]);
  const uint32_t k_step = static_cast<uint32_t>(BKV * k_tok * 2);
  const uint32_t v_step = static_cast<uint32_t>(BKV * v_tok * 2);
  if constexpr (DMA) {
    rk = mxk::make_rsrc(kb_ptr, static_cast<unsigned>(S * k_tok * 2));
    rv = mxk::make_rsrc(vb_ptr, static_cast<unsigned>(S * v_tok * 2));
    const int prow = lane >> 4, pslot = lane & 15;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int r = 4 * (4 * wave + p) + prow;
      const int ch = pslot ^ ((prow << 2) | p);
      kvo[p] = static_cast<uint32_t>(r * k_tok * 2 + ch * 16);
      vvo[p] = static_cast<uint32_t>(r * v_tok * 2 + ch * 16);
    }
  }
  auto issue = [&](int j, int buf) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint32_t d = sm32 + buf * (2 * TILE_BYTES) + (4 * wave + p) * 1024;
      mxk::dma16m(rk, d, kvo[p], j * k_step);
      mxk::dma16m(rv, d + TILE_BYTES, vvo[p], j * v_step);
    }
  };
  if constexpr (DMA) {
    issue(j_lo, j_lo & 1);
    // consume the per-query loads here, so the compiler's vmcnt waits for
    // them sit before the loop and not inside it (where they would also wait
    // for the next tile's untracked DMA)
#pragma unroll
    for (int s = 0; s < 8; ++s) asm volatile("" ::"v"(qf[s]), "v"(dof[s]));
    asm volatile("" ::"v"(lse2), "v"(dlt));
    if constexpr (DOC) asm volatile("" ::"v"(ds_row));
    vm_wait<0>();
  } else {
    load_tile(0);
    store_tile(0);
  }
  __syncthreads();

  f32x16_t acc[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) zero16(acc[db]);
  const int G = lane >> 4, i16 = lane & 15;
  const int tr_key = 4 * h + (i16 >> 2);
  const int tr_ch = 2 * (G & 1) + ((i16 & 3) >> 1);
  const int tr_byte = 8 * (i16 & 1);

  // One loop body for both walks.  UNROLL: two tiles per trip of the outer
  // loop, so the buffer - and with it every LDS read address - is a
  // compile-time constant (as in the forward's variant 4).  The do / while is
  // no loop at all when UNROLL is false (the compiler's front end drops a
  // constant-false back edge, and every such instance keeps the instruction
  // stream of a plain `for (j)` around the body), and is unrolled in full
  // when it is true.  Neither a `for (u < NU)` around the body nor the body as
  // a lambda called from two loops does that: profiles/attention_dedup/.
  constexpr int NU = UNROLL ? 2 : 1;
  for (int j0 = j_lo; j0 < nkv; j0 += NU) {
    int u = 0;
#pragma unroll
    do {
      const int j = UNROLL ? j0 + u : j0;
      const int buf = UNROLL ? u : j & 1;
      if (!UNROLL || j < nkv) {
        // DMA: buffer buf^1 was last read in iteration j-1 (barrier-certified)
        if (j + 1 < nkv) {
          if constexpr (DMA) issue(j + 1, buf ^ 1);
          else load_tile(j + 1);
        }
        const int kv0 = j * BKV;
        bool active = !CAUSAL || kv0 <= qw0 + 31;
        if constexpr (DOC) active = active && attn_doc_tile_active(kv0, BKV, ds_w0);
        if (active) {
          const char* kt = smem[buf];
          const char* vt = smem[buf] + TILE_BYTES;
          const bool diag = CAUSAL && kv0 + BKV - 1 > qw0;
          if constexpr (PIPE) {
            // software-pipelined as the dK/dV kernel's PIPE body: S / dP operands
            // read a half (4 k-steps) ahead, dS-side transposed reads issued
            // under the exp, the next half's first operands under the dQ MFMAs
            bf16x8_t ka[2][2], va[2][2];    // ring of two k-step pairs
            auto read_p = [&](int kh, int pr, int slot) {
#pragma unroll
              for (int e = 0; e < 2; ++e) {
                const int s = 2 * pr + e;
                ka[slot][e] = lds_b128(kt + swz(32 * kh + r32, 2 * s + h));
                va[slot][e] = lds_b128(vt + swz(32 * kh + r32, 2 * s + h));
              }
            };
            auto read_t = [&](int kh, int db, int kk) {
              const int key = 32 * kh + 16 * kk + tr_key;
              const int ch = 4 * db + tr_ch;
              return cat8(lds_tr_b64(kt + swz(key, ch) + tr_byte),
                          lds_tr_b64(kt + swz(key + 8, ch) + tr_byte));
            };
            read_p(0, 0, 0);
#pragma unroll
            for (int kh = 0; kh < 2; ++kh) {
              __builtin_amdgcn_sched_barrier(0);
              f32x16_t s0, p0;
              zero16(s0);
              zero16(p0);
              bf16x8_t ta[8];
#pragma unroll
              for (int pr = 0; pr < 4; ++pr) {
                if (pr < 3) {
                  read_p(kh, pr + 1, (pr + 1) & 1);
                } else {
#pragma unroll
                  for (int x = 0; x < 4; ++x) ta[x] = read_t(kh, x >> 1, x & 1);
                }
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                  s0 = mfma32(ka[pr & 1][e], qf[2 * pr + e], s0);
                  p0 = mfma32(va[pr & 1][e], dof[2 * pr + e], p0);
                }
                __builtin_amdgcn_sched_barrier(0);
              }
#pragma unroll
              for (int x = 4; x < 8; ++x) ta[x] = read_t(kh, x >> 1, x & 1);
              // packed fp32 (v_pk_fma / v_pk_add / v_pk_mul): half the VALU issues
#pragma unroll
              for (int r = 0; r < 16; r += 2) {
                f32x2_t x = {s0[r], s0[r + 1]};
                x = __builtin_elementwise_fma(x, f32x2_t{c, c}, f32x2_t{-lse2, -lse2});
                s0[r] = fexp2(x[0]);   // P^T
                s0[r + 1] = fexp2(x[1]);
              }
              if (diag) {   // wave-uniform: only diagonal tiles pay for the mask
#pragma unroll
                for (int r = 0; r < 16; ++r)
                  if (kv0 + 32 * kh + crow(r, h) > myq) s0[r] = 0.f;
              }
              if constexpr (DOC) {
                if (attn_doc_tile_masked(kv0, ds_w1)) {   // wave-uniform
#pragma unroll
                  for (int r = 0; r < 16; ++r)
                    if (kv0 + 32 * kh + crow(r, h) < ds_row) s0[r] = 0.f;
                }
              }
#pragma unroll
              for (int r = 0; r < 16; r += 2) {
                const f32x2_t pp = f32x2_t{p0[r], p0[r + 1]} - f32x2_t{dlt, dlt};
                const f32x2_t d = f32x2_t{s0[r], s0[r + 1]} * pp;   // dS^T
                s0[r] = d[0];
                s0[r + 1] = d[1];
              }
              bf16x8_t df[2];
              df[0] = pack8(s0, 0);
              df[1] = pack8(s0, 8);
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int x = 0; x < 8; ++x) {
                acc[x >> 1] = mfma32(ta[x], df[x & 1], acc[x >> 1]);
                if (kh == 0 && x == 5) {
                  read_p(1, 0, 0);
                  __builtin_amdgcn_sched_barrier(0);
                }
              }
            }
          } else {
          // one 32-key half at a time keeps S^T / dP^T to 32 registers
#pragma unroll
          for (int kh = 0; kh < 2; ++kh) {
            f32x16_t s0, p0;
            zero16(s0);
            zero16(p0);
#pragma unroll
            for (int s = 0; s < 8; ++s) {
              const bf16x8_t kf = lds_b128(kt + swz(32 * kh + r32, 2 * s + h));
              const bf16x8_t vf = lds_b128(vt + swz(32 * kh + r32, 2 * s + h));
              s0 = mfma32(kf, qf[s], s0);
              p0 = mfma32(vf, dof[s], p0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              float e0 = fexp2(fmaf(s0[r], c, -lse2));
              if (diag && kv0 + 32 * kh + crow(r, h) > myq) e0 = 0.f;
              s0[r] = e0 * (p0[r] - dlt);   // dS^T
            }
            bf16x8_t df[2];
            df[0] = pack8(s0, 0);
            df[1] = pack8(s0, 8);
            // dQ^T += K^T . dS^T  (K^T by transposed reads of the K image)
#pragma unroll
            for (int db = 0; db < 4; ++db) {
#pragma unroll
              for (int kk = 0; kk < 2; ++kk) {
                const int key = 32 * kh + 16 * kk + tr_key;
                const int ch = 4 * db + tr_ch;
                const bf16x4_t lo = lds_tr_b64(kt + swz(key, ch) + tr_byte);
                const bf16x4_t hi = lds_tr_b64(kt + swz(key + 8, ch) + tr_byte);
                const bf16x8_t a = cat8(lo, hi);
                acc[db] = mfma32(a, df[kk], acc[db]);
              }
            }
          }
          }
        }
        if constexpr (DMA) {
          vm_wait<0>();   // own pieces of tile j+1
        } else {
          if (j + 1 < nkv) store_tile(buf ^ 1);
        }
        __syncthreads();
      }
    } while (UNROLL && ++u < NU);
  }
  uint16_t* row = dq + (static_cast<long>(b) * S + myq) * Hq * D + static_cast<long>(hq) * D;
  // 16-B stores, lane halves paired by v_permlane32_swap (as the forward's O)
#pragma unroll
  for (int db = 0; db < 4; ++db) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int g0 = 2 * kk, g1 = 2 * kk + 1;
      const uint32_t x0 = mxk::pack2bf(acc[db][4 * g0] * scale, acc[db][4 * g0 + 1] * scale);
      const uint32_t x1 = mxk::pack2bf(acc[db][4 * g0 + 2] * scale, acc[db][4 * g0 + 3] * scale);
      const uint32_t y0 = mxk::pack2bf(acc[db][4 * g1] * scale, acc[db][4 * g1 + 1] * scale);
      const uint32_t y1 = mxk::pack2bf(acc[db][4 * g1 + 2] * scale, acc[db][4 * g1 + 3] * scale);
      const auto p0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
      const auto p1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
      uint4 ov;
      ov.x = p0[0];
      ov.y = p1[0];
      ov.z = p0[1];
      ov.w = p1[1];
      *reinterpret_cast<uint4*>(row + 32 * db + 16 * kk + 8 * h) = ov;
    }
  }
}

// dK/dV with 16x16x32 MFMAs: one workgroup = 8 waves x 16 keys (128 keys of
// one (batch, q-head)), so a wave holds dK^T / dV^T of its keys in 64
// registers (32x32 tiles need 128) and two waves share each SIMD - a
// 32-key-per-wave kernel on 32x32x16 MFMAs (4 waves, one per SIMD; removed)
// left the matrix core idle through its exp / pack / LDS phases.  Per
// 32-query k-step:
//   S  = Q.K^T, dP = dO.V^T    (A: Q / dO rows, ds_read_b128; B: K / V in registers)
//   P  = exp2(c S'), dS = P dP' (accumulators pre-loaded with -LSE/scale, -delta)
//   dV^T += dO^T.P, dK^T += Q^T.dS  (A: transposed reads of the same images;
//   B: two 16x16 accumulator tiles = 8 consecutive-by-4 queries per lane)
// Q / dO image: 256-B rows, chunk c of row r at c ^ 2(r & 7) - conflict-free
// for the 16x16x32 row reads and the transposed reads (tests/test_attention_layout.py).
// Partials dk_p / dv_p (without GQA) are fp32 [B, S, Hq, 128], summed over the
// GQA group afterwards.
// Round-2 alternatives measured against the PIPE body of this kernel
// (profiles/r2_attention/): a four-buffer LDS ring with every load three
// items ahead (lse / delta rows by DMA too) 1.129 vs 1.099 ms per layer, and
// the 32-key-per-wave kernel pipelined (half the LDS operand traffic, dK / dV
// pinned to AGPRs, softmax overlapped in-wave) 1.182 vs 1.107 ms - two waves
// per SIMD hide more than the halved LDS traffic saves.  Also neutral:
// 128-query slices (half the barriers and pipeline drains; 1.1249 vs
// 1.1215 ms, bit-identical).  A staggered order for waves 4-7 (both S / dP
// groups first, so the SIMD partners' exp phases do not coincide) needs ~16
// more VGPRs than the 223 of this body and spilled (119 VGPRs, 4.17 ms).
namespace {
__device__ __forceinline__ int swz16(int row, int ch) {
  return row * 256 + ((ch ^ (2 * (row & 7))) << 4);
}
__device__ __forceinline__ f32x4_t mfma16(bf16x8_t a, bf16x8_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8_t pack2x4(const f32x4_t& lo, const f32x4_t& hi) {
  bf16x8_t o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[j] = static_cast<short>(mxk::f2bf(lo[j]));
    o[4 + j] = static_cast<short>(mxk::f2bf(hi[j]));
  }
  return o;
}
constexpr int NT16 = 512;
}  // namespace

// GQA: one workgroup per (batch, KV head, key block) walks every query head
// of the group, so dK^T / dV^T of its keys accumulate in registers over the
// whole group and are written once, in bf16, straight into dk / dv (token
// strides dk_tok / dv_tok).  Without it, one workgroup per query head writes
// fp32 partials that mxk_attn_bwd_gqa_reduce_kernel sums (4x the grid,
// ~1.1 GB more HBM traffic per Llama-3-8B layer at B = 8).
// DMA: Q / dO slices by LDS-DMA (wave w moves the 1-KiB pieces 2w, 2w + 1 of
// each), as in the dQ kernel; the lse / delta rows stay register-staged.
// DOC (mxk_attn_bwd_doc; with CAUSAL, GQA, DMA and PIPE): causal within a
// document, by the key's side of the rule - row i sees key j <= i iff
// i < doc_end[j].  The walk ends at the slice of doc_end[k0 + 127] instead of
// at S, a wave skips the slices that begin at or after its last key's
// doc_end, and the slices that reach past its first key's doc_end zero P
// where row >= doc_end[key].
template <bool CAUSAL, bool GQA = false, bool DMA = false, bool PIPE = false, bool DOC = false>
__global__ void __launch_bounds__(NT16, 1)
mxk_attn_bwd_dkdv16_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                           const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
                           const float* __restrict__ lse, const float* __restrict__ delta,
                           float* __restrict__ dk_p, float* __restrict__ dv_p, int S, int Hq,
                           int Hkv, long q_tok, long k_tok, long v_tok, float scale,
                           uint16_t* __restrict__ dk = nullptr, uint16_t* __restrict__ dv = nullptr,
                           long dk_tok = 0, long dv_tok = 0,
                           const int* __restrict__ doc_end = nullptr) {
  static_assert(!DOC || (CAUSAL && GQA && DMA && PIPE), "the DOC form extends the GQA DMA PIPE instance");
  __shared__ __attribute__((aligned(16))) char smem[2][2 * BQB * 256];   // [buf][Q | dO]
  __shared__ __attribute__((aligned(16))) float srow[2][2][BQB];       // [buf][-lse/scale | -delta]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15;
  const int G = lane >> 4;

  const int nkb = S / BQ;
  int bh, kb;
  {
    int qbi;
    map_block(blockIdx.x, gridDim.x / nkb, nkb, CAUSAL, &bh, &qbi);
    kb = CAUSAL ? nkb - 1 - qbi : qbi;
  }
  const int grp = Hq / Hkv;
  const int b = GQA ? bh / Hkv : bh / Hq;
  const int hq0 = GQA ? (bh % Hkv) * grp : bh % Hq;
  const int hkv = GQA ? bh % Hkv : hq0 / grp;
  const int k0 = kb * BQ;
  const int kw0 = k0 + wave * 16;
  const int mykey = kw0 + c16;
  const uint16_t* kb_ptr = k + static_cast<long>(b) * S * k_tok + static_cast<long>(hkv) * D;
  const uint16_t* vb_ptr = v + static_cast<long>(b) * S * v_tok + static_cast<long>(hkv) * D;

  // B operands of S / dP: lane holds K[mykey][32 s + 8 G .. +7]
  bf16x8_t kf[4], vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    kf[s] = *reinterpret_cast<const bf16x8_t*>(kb_ptr + static_cast<long>(mykey) * k_tok + 32 * s + 8 * G);
    vf[s] = *reinterpret_cast<const bf16x8_t*>(vb_ptr + static_cast<long>(mykey) * v_tok + 32 * s + 8 * G);
  }
  // DOC: the block's last slice and the wave's bounds through uniform
  // addresses (scalar loads), the lane's own key next to its K / V fragments
  int de_blk = S, de_w0 = S, de_w1 = S, de_key = S;
  if constexpr (DOC) {
    const int* de_b = doc_end + static_cast<long>(b) * S;
    de_blk = de_b[k0 + BQ - 1];
    de_w0 = de_b[kw0];
    de_w1 = de_b[kw0 + 15];
    de_key = de_b[mykey];
  }
  if constexpr (DMA) {
    // wait for the K / V fragments here, before the loops: a compiler wait
    // at their first use inside the slice loop would also wait for the
    // untracked DMA of the next slice
#pragma unroll
    for (int s = 0; s < 4; ++s) asm volatile("" ::"v"(kf[s]), "v"(vf[s]));
    if constexpr (DOC) asm volatile("" ::"v"(de_key));
  }
  const float c = scale * 1.4426950408889634f;
  const float inv_c = 1.f / c;

  f32x4_t dka[8], dva[8];
#pragma unroll
  for (int db = 0; db < 8; ++db) {
    dka[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    dva[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  // transposed-read lane constants: row 4G + (i >> 2), column block 4 (i & 3)
  const int tr_row = 4 * G + (c16 >> 2);
  const int tr_chb = (c16 & 3) >> 1;
  const int tr_byte = 8 * (c16 & 1);
  const int q_begin = CAUSAL ? k0 : 0;
  const int nsl = DOC ? attn_doc_slices(de_blk, k0, S, BQB) : (S - q_begin) / BQB;
  // Work items i = (query slice t, head gq of the group), head-outer, slices
  // ascending from the diagonal; pipelined across head boundaries.  (A
  // slice-outer walk from the last slice down, heads inner, which keeps the
  // key blocks of a group in lockstep on the same Q / dO slice, measured
  // neutral: 1.2417 vs 1.2468 ms per Llama-3-8B layer, profiles/r2_attention.)
  const int ngq = GQA ? grp : 1;
  const int niter = nsl * ngq;
  auto item = [&](int i, int* t, int* gq) {
    *gq = i / nsl;
    *t = i - *gq * nsl;
  };
  const uint16_t* qg_ptr = q + static_cast<long>(b) * S * q_tok + static_cast<long>(hq0) * D;
  const uint16_t* dog_ptr = dout + static_cast<long>(b) * S * Hq * D + static_cast<long>(hq0) * D;
  const float* lse_g = lse + (static_cast<long>(b) * Hq + hq0) * S;
  const float* dl_g = delta + (static_cast<long>(b) * Hq + hq0) * S;
  // loader: 512 threads x 2 chunks per tile (64 rows x 16 chunks)
  const int ld_row = tid >> 4, ld_ch = tid & 15;
  bf16x8_t qst[2], dst[2];
  float rst = 0.f;
  auto load_slice = [&](int i) {
    int t, gq;
    item(i, &t, &gq);
    const long r0 = q_begin + static_cast<long>(t) * BQB + ld_row;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      qst[j] = *reinterpret_cast<const bf16x8_t*>(qg_ptr + (r0 + 32 * j) * q_tok + gq * D + ld_ch * 8);
      dst[j] = *reinterpret_cast<const bf16x8_t*>(dog_ptr + (r0 + 32 * j) * Hq * D + gq * D + ld_ch * 8);
    }
    if (tid < 2 * BQB) {
      const long qi = q_begin + static_cast<long>(t) * BQB + (tid & (BQB - 1));
      rst = tid < BQB ? -lse_g[gq * S + qi] * 1.4426950408889634f * inv_c : -dl_g[gq * S + qi];
    }
  };
  auto store_slice = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int off = swz16(ld_row + 32 * j, ld_ch);
      *reinterpret_cast<bf16x8_t*>(smem[buf] + off) = qst[j];
      *reinterpret_cast<bf16x8_t*>(smem[buf] + BQB * 256 + off) = dst[j];
    }
    if (tid < 2 * BQB) srow[buf][tid / BQB][tid & (BQB - 1)] = rst;
  };
  // raw load at the top, arithmetic at the store: math right after the load
  // would put a vmcnt(0) there, which also waits for the slice DMA just issued
  auto load_row = [&](int i) {
    if (tid < 2 * BQB) {
      int t, gq;
      item(i, &t, &gq);
      const long qi = q_begin + static_cast<long>(t) * BQB + (tid & (BQB - 1));
      rst = (tid < BQB ? lse_g : dl_g)[gq * S + qi];
    }
  };
  auto store_row = [&](int buf) {
    if (tid < 2 * BQB)
      srow[buf][tid / BQB][tid & (BQB - 1)] = tid < BQB ? -rst * 1.4426950408889634f * inv_c : -rst;
  };
  mxk::u32x4 rq{}, rd{};
  uint32_t qvo[2] = {}, dvo[2] = {};
  const uint32_t sm32 = mxk::lds_addr32(&smem[0][0]);
  if constexpr (DMA) {
    // base at the group's first head; head gq is + 2 D gq bytes of soffset
    rq = mxk::make_rsrc(qg_ptr, static_cast<unsigned>(S * q_tok * 2));
    rd = mxk::make_rsrc(dog_ptr, static_cast<unsigned>(static_cast<long>(S) * Hq * D * 2));
    // lane i lands at row 4g + (i >> 4), slot i & 15 = chunk ^ 2 (row & 7)
    const int prow = lane >> 4, pslot = lane & 15;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int r = 4 * (2 * wave + p) + prow;
      const int ch = pslot ^ (2 * (r & 7));
      qvo[p] = static_cast<uint32_t>(r * q_tok * 2 + ch * 16);
      dvo[p] = static_cast<uint32_t>(r * Hq * D * 2 + ch * 16);
    }
  }
  auto issue = [&](int i, int buf) {
    int t, gq;
    item(i, &t, &gq);
    const long row0 = q_begin + static_cast<long>(t) * BQB;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const uint32_t d = sm32 + buf * (2 * BQB * 256) + (2 * wave + p) * 1024;
      mxk::dma16m(rq, d, qvo[p], static_cast<uint32_t>(row0 * q_tok * 2 + gq * D * 2));
      mxk::dma16m(rd, d + BQB * 256, dvo[p], static_cast<uint32_t>(row0 * Hq * D * 2 + gq * D * 2));
    }
  };
  if constexpr (DMA) {
    issue(0, 0);
    load_row(0);
    vm_wait<0>();
    store_row(0);
  } else {
    load_slice(0);
    store_slice(0);
  }
  __syncthreads();

  for (int i = 0; i < niter; ++i) {
    const int buf = i & 1;
    if (i + 1 < niter) {
      if constexpr (DMA) {
        issue(i + 1, buf ^ 1);   // buf ^ 1 last read in item i - 1 (barrier-certified)
        load_row(i + 1);
      } else {
        load_slice(i + 1);
      }
    }
    int t, gq_unused;
    item(i, &t, &gq_unused);
    const int qs0 = q_begin + t * BQB;
    bool active = !CAUSAL || qs0 + BQB - 1 >= kw0;
    if constexpr (DOC) active = active && attn_doc_slice_active(qs0, de_w1);
    if (active) {
      const char* qt = smem[buf];
      const char* dt = smem[buf] + BQB * 256;
      const bool diag = CAUSAL && qs0 < kw0 + 15;
      if constexpr (PIPE) {
        // Explicitly software-pipelined: every LDS operand is read one MFMA
        // group ahead of its use, and sched_barrier fences keep the compiler
        // from re-serialising read -> lgkmcnt(0) -> MFMA per instruction
        // (what it emits for the plain loop below: 64 waits per slice, each
        // exposing a full LDS latency).  The waitcnt pass then counts
        // lgkmcnt down through each group.
        bf16x8_t qa[8], da[8];          // S / dP A operands, [2 s + h]
        float4 l4[2], d4[2];            // -lse / -delta rows of the two halves
        auto read_a = [&](int ks) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int qr = 32 * ks + 16 * h + 4 * G;
            l4[h] = *reinterpret_cast<const float4*>(&srow[buf][0][qr]);
            d4[h] = *reinterpret_cast<const float4*>(&srow[buf][1][qr]);
          }
#pragma unroll
          for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int row = 32 * ks + 16 * h + c16;
              qa[2 * s + h] = *reinterpret_cast<const bf16x8_t*>(qt + swz16(row, 4 * s + G));
              da[2 * s + h] = *reinterpret_cast<const bf16x8_t*>(dt + swz16(row, 4 * s + G));
            }
          }
        };
        auto read_b = [&](int ks, int db, bf16x8_t* ao, bf16x8_t* aq) {
          const int row = 32 * ks + tr_row;
          const int ch = 2 * db + tr_chb;
          *ao = cat8(lds_tr_b64(dt + swz16(row, ch) + tr_byte),
                     lds_tr_b64(dt + swz16(row + 16, ch) + tr_byte));
          *aq = cat8(lds_tr_b64(qt + swz16(row, ch) + tr_byte),
                     lds_tr_b64(qt + swz16(row + 16, ch) + tr_byte));
        };
        read_a(0);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          __builtin_amdgcn_sched_barrier(0);
          f32x4_t st[2], pt[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            st[h] = f32x4_t{l4[h].x, l4[h].y, l4[h].z, l4[h].w};
            pt[h] = f32x4_t{d4[h].x, d4[h].y, d4[h].z, d4[h].w};
          }
#pragma unroll
          for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              st[h] = mfma16(qa[2 * s + h], kf[s], st[h]);
              pt[h] = mfma16(da[2 * s + h], vf[s], pt[h]);
            }
          }
          // first half of the dV / dK operands in flight under the exp
          bf16x8_t ob[8], qb[8];
#pragma unroll
          for (int db = 0; db < 4; ++db) read_b(ks, db, &ob[db], &qb[db]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
              const f32x2_t x = f32x2_t{st[h][r], st[h][r + 1]} * f32x2_t{c, c};
              st[h][r] = fexp2(x[0]);   // P
              st[h][r + 1] = fexp2(x[1]);
            }
          if (diag) {   // wave-uniform: only diagonal slices pay for the mask
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (mykey > qs0 + 32 * ks + 16 * h + 4 * G + r) st[h][r] = 0.f;
          }
          if constexpr (DOC) {
            if (attn_doc_slice_masked(qs0, BQB, de_w0)) {   // wave-uniform
#pragma unroll
              for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                  if (qs0 + 32 * ks + 16 * h + 4 * G + r >= de_key) st[h][r] = 0.f;
            }
          }
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
              const f32x2_t d = f32x2_t{pt[h][r], pt[h][r + 1]} * f32x2_t{st[h][r], st[h][r + 1]};
              pt[h][r] = d[0];   // dS
              pt[h][r + 1] = d[1];
            }
          const bf16x8_t pf = pack2x4(st[0], st[1]);
          const bf16x8_t sf = pack2x4(pt[0], pt[1]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int db = 0; db < 4; ++db) {
            dva[db] = mfma16(ob[db], pf, dva[db]);
            dka[db] = mfma16(qb[db], sf, dka[db]);
            read_b(ks, db + 4, &ob[db + 4], &qb[db + 4]);
            __builtin_amdgcn_sched_barrier(0);
          }
          if (ks == 0) read_a(1);       // next half's S / dP operands under the last MFMAs
#pragma unroll
          for (int db = 4; db < 8; ++db) {
            dva[db] = mfma16(ob[db], pf, dva[db]);
            dka[db] = mfma16(qb[db], sf, dka[db]);
          }
        }
      } else {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        f32x4_t st[2], pt[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int qr = 32 * ks + 16 * h + 4 * G;
          const float4 l4 = *reinterpret_cast<const float4*>(&srow[buf][0][qr]);
          const float4 d4 = *reinterpret_cast<const float4*>(&srow[buf][1][qr]);
          st[h] = f32x4_t{l4.x, l4.y, l4.z, l4.w};
          pt[h] = f32x4_t{d4.x, d4.y, d4.z, d4.w};
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int row = 32 * ks + 16 * h + c16;
            st[h] = mfma16(*reinterpret_cast<const bf16x8_t*>(qt + swz16(row, 4 * s + G)), kf[s], st[h]);
            pt[h] = mfma16(*reinterpret_cast<const bf16x8_t*>(dt + swz16(row, 4 * s + G)), vf[s], pt[h]);
          }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float e = fexp2(st[h][r] * c);
            if (diag && mykey > qs0 + 32 * ks + 16 * h + 4 * G + r) e = 0.f;
            st[h][r] = e;                  // P
            pt[h][r] = e * pt[h][r];       // dS
          }
        }
        const bf16x8_t pf = pack2x4(st[0], st[1]);
        const bf16x8_t sf = pack2x4(pt[0], pt[1]);
#pragma unroll
        for (int db = 0; db < 8; ++db) {
          const int row = 32 * ks + tr_row;
          const int ch = 2 * db + tr_chb;
          const bf16x8_t ao = cat8(lds_tr_b64(dt + swz16(row, ch) + tr_byte),
                                   lds_tr_b64(dt + swz16(row + 16, ch) + tr_byte));
          const bf16x8_t aq = cat8(lds_tr_b64(qt + swz16(row, ch) + tr_byte),
                                   lds_tr_b64(qt + swz16(row + 16, ch) + tr_byte));
          dva[db] = mfma16(ao, pf, dva[db]);
          dka[db] = mfma16(aq, sf, dka[db]);
        }
      }
      }
    }
    if constexpr (DMA) {
      vm_wait<0>();   // own pieces of item i+1
      if (i + 1 < niter) store_row(buf ^ 1);
    } else {
      if (i + 1 < niter) store_slice(buf ^ 1);
    }
    __syncthreads();
  }
  // lane = key, registers r: d = 16 db + 4 G + r
  if constexpr (GQA) {
    uint16_t* dkr = dk + (static_cast<long>(b) * S + mykey) * dk_tok + static_cast<long>(hkv) * D;
    uint16_t* dvr = dv + (static_cast<long>(b) * S + mykey) * dv_tok + static_cast<long>(hkv) * D;
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      const int d = 16 * db + 4 * G;
      uint2 pk;
      pk.x = mxk::pack2bf(dka[db][0] * scale, dka[db][1] * scale);
      pk.y = mxk::pack2bf(dka[db][2] * scale, dka[db][3] * scale);
      *reinterpret_cast<uint2*>(dkr + d) = pk;
      pk.x = mxk::pack2bf(dva[db][0], dva[db][1]);
      pk.y = mxk::pack2bf(dva[db][2], dva[db][3]);
      *reinterpret_cast<uint2*>(dvr + d) = pk;
    }
  } else {
    const long prow = ((static_cast<long>(b) * S + mykey) * Hq + hq0) * D;
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      const int d = 16 * db + 4 * G;
      *reinterpret_cast<float4*>(dk_p + prow + d) =
          make_float4(dka[db][0] * scale, dka[db][1] * scale, dka[db][2] * scale,
                      dka[db][3] * scale);
      *reinterpret_cast<float4*>(dv_p + prow + d) =
          make_float4(dva[db][0], dva[db][1], dva[db][2], dva[db][3]);
    }
  }
}

// dk[b][s][hkv][:] = sum over the group's q-heads of dk_p[b][s][hq][:] (bf16 out)
__global__ void __launch_bounds__(256)
mxk_attn_bwd_gqa_reduce_kernel(const float* __restrict__ dk_p, const float* __restrict__ dv_p,
                               uint16_t* __restrict__ dk, uint16_t* __restrict__ dv, long n_out,
                               int Hq, int Hkv, long dk_tok, long dv_tok) {
  const long i = (static_cast<long>(blockIdx.x) * 256 + threadIdx.x) * 4;   // 4 dims per thread
  if (i >= n_out) return;
  const int grp = Hq / Hkv;
  const int d = static_cast<int>(i % D);
  const long t = i / D;               // (b*S + s)*Hkv + hkv
  const int hkv = static_cast<int>(t % Hkv);
  const long bs = t / Hkv;
  float4 ak = make_float4(0.f, 0.f, 0.f, 0.f), av = ak;
  for (int gq = 0; gq < grp; ++gq) {
    const long src = (bs * Hq + hkv * grp + gq) * D + d;
    const float4 x = *reinterpret_cast<const float4*>(dk_p + src);
    const float4 y = *reinterpret_cast<const float4*>(dv_p + src);
    ak.x += x.x; ak.y += x.y; ak.z += x.z; ak.w += x.w;
    av.x += y.x; av.y += y.y; av.z += y.z; av.w += y.w;
  }
  uint2 pk;
  pk.x = mxk::pack2bf(ak.x, ak.y);
  pk.y = mxk::pack2bf(ak.z, ak.w);
  *reinterpret_cast<uint2*>(dk + bs * dk_tok + hkv * D + d) = pk;
  pk.x = mxk::pack2bf(av.x, av.y);
  pk.y = mxk::pack2bf(av.z, av.w);
  *reinterpret_cast<uint2*>(dv + bs * dv_tok + hkv * D + d) = pk;
}

MXK_API long mxk_attn_bwd_workspace_variant(int B, int S, int Hq, int variant) {
  return attn_bwd_workspace(B, S, Hq, variant);
}

// attn_bwd_plan (attention_plan.h) of a layout, for the host tests: out[0..6]
// = resolved variant, delta, AttnDq, AttnDkdv, reduce, dq_first, workspace
// bytes.  Host arithmetic only; launches nothing.
MXK_API int mxk_attn_bwd_plan(int B, int S, int Hq, int Hkv, long q_tok, long k_tok, long v_tok,
                              long dk_tok, long dv_tok, int causal, int variant, long* out) {
  const AttnLayout L{B, S, Hq, Hkv, q_tok, k_tok, v_tok, static_cast<long>(Hq) * D, dk_tok, dv_tok,
                     causal};
  const AttnBwdPlan p = attn_bwd_plan(L, variant);
  if (p.variant < 0 || !out) return static_cast<int>(hipErrorInvalidValue);
  const long f[7] = {p.variant, p.delta, p.dq, p.dkdv, p.reduce, p.dq_first, p.workspace};
  for (int i = 0; i < 7; ++i) out[i] = f[i];
  return 0;
}

// Backward variant 9 with the rotary-embedding backward fused into the dQ
// and dK stores: q / k are the ROTATED projections the forward ran on, and
// dq / dk come out as gradients of the un-rotated ones (rcos / rsin: the
// forward's [S][D/2] fp32 tables), so the fused-QKV projection's backward
// takes d(QKV) straight from here (dq / dk / dv at token strides, e.g.
// slices of one buffer).  Workspace: mxk_attn_bwd_workspace_variant(.., 9).
// hipErrorInvalidValue, with nothing launched, when either kernel does not
// take the layout (the caller then runs mxk_attn_bwd_variant and the
// stand-alone RoPE pass).
MXK_API int mxk_attn_bwd_rope(const void* q, const void* k, const void* v, const void* o,
                              const void* dout, const float* lse, void* dq, void* dk, void* dv,
                              void* workspace, int B, int S, int Hq, int Hkv, int head_dim,
                              long q_tok, long k_tok, long v_tok, long dq_tok, long dk_tok,
                              long dv_tok, const float* rcos, const float* rsin, float scale,
                              int causal, hipStream_t stream) {
  const AttnLayout L{B, S, Hq, Hkv, q_tok, k_tok, v_tok, dq_tok, dk_tok, dv_tok, causal};
  if (head_dim != D || !workspace || !rcos || !rsin || !attn_dq256_rope_ok(L) ||
      !attn_dkdv256_ok(L) || !attn_aligned(16, q, k, v, o, dout, dq, workspace, rcos, rsin) ||
      !attn_aligned(8, dk, dv))
    return static_cast<int>(hipErrorInvalidValue);
  float* rowc = static_cast<float*>(workspace);
  const int st = mxk_attn_bwd_dq256_rope(q, k, v, o, dout, lse, dq, rowc, B, S, Hq, Hkv, q_tok,
                                         k_tok, v_tok, dq_tok, rcos, rsin, scale, causal, stream);
  if (st) return st;
  return mxk_attn_bwd_dkdv256_rope(q, k, v, dout, rowc, dk, dv, B, S, Hq, Hkv, q_tok, k_tok, v_tok,
                                   dk_tok, dv_tok, rcos, rsin, scale, causal, stream);
}

namespace {
// the tensors of one backward, as the 128-row dQ and 16x16 dK/dV kernels take them
struct BwdArgs {
  const uint16_t *q, *k, *v, *o, *dout;
  const float* lse;
  uint16_t *dq, *dk, *dv;
  float *delta, *dk_p, *dv_p;   // workspace: delta (or rowc pairs), variant 0's partials
  float scale;
  hipStream_t stream;
};

// FOLD forms write delta (ROWC: the rowc pairs) from o and read none
int launch_dq(AttnDq kind, const AttnLayout& L, const BwdArgs& a) {
  if (kind == DQ_256)
    return mxk_attn_bwd_dq256(a.q, a.k, a.v, a.o, a.dout, a.lse, a.dq, a.delta, L.B, L.S, L.Hq,
                              L.Hkv, L.q_tok, L.k_tok, L.v_tok, a.scale, L.causal, a.stream);
  const bool fold = kind == DQ_FOLD || kind == DQ_FOLD_ROWC;
#define MXK_DQ(...)                                                                               \
  hipLaunchKernelGGL((mxk_attn_bwd_dq_kernel<__VA_ARGS__>), dim3(L.B * L.Hq * (L.S / BQ)),       \
                     dim3(NT), 0, a.stream, a.q, a.k, a.v, a.dout, a.lse,                        \
                     fold ? nullptr : a.delta, a.dq, L.S, L.Hq, L.Hkv, L.q_tok, L.k_tok, L.v_tok, \
                     a.scale, fold ? a.o : nullptr, fold ? a.delta : nullptr)
  switch (kind) {
    case DQ_REG: MXK_WITH_BOOL(C, L.causal, MXK_DQ(C, false)); break;
    case DQ_DMA: MXK_WITH_BOOL(C, L.causal, MXK_DQ(C, true)); break;
    case DQ_DMA_PIPE: MXK_WITH_BOOL(C, L.causal, MXK_DQ(C, true, true)); break;
    case DQ_DMA_PIPE_UNROLL: MXK_DQ(true, true, true, true); break;
    case DQ_FOLD: MXK_WITH_BOOL(C, L.causal, MXK_DQ(C, true, true, false, true)); break;
    case DQ_FOLD_ROWC: MXK_WITH_BOOL(C, L.causal, MXK_DQ(C, true, true, false, true, true)); break;
    default: return static_cast<int>(hipErrorInvalidValue);   // DQ_ATOMICS: no dQ stage
  }
#undef MXK_DQ
  MXK_RETURN_LAUNCH_STATUS();
}

int launch_dkdv(AttnDkdv kind, const AttnLayout& L, const BwdArgs& a) {
  if (kind == DKDV_256)
    return mxk_attn_bwd_dkdv256(a.q, a.k, a.v, a.dout, a.delta, a.dk, a.dv, L.B, L.S, L.Hq, L.Hkv,
                                L.q_tok, L.k_tok, L.v_tok, L.dk_tok, L.dv_tok, a.scale, L.causal,
                                a.stream);
  const bool gqa = kind != DKDV_HEAD;
#define MXK_DKDV16(...)                                                                          \
  MXK_WITH_BOOL(C, L.causal,                                                                     \
                hipLaunchKernelGGL((mxk_attn_bwd_dkdv16_kernel<C, __VA_ARGS__>),                 \
                                   dim3(L.B * (gqa ? L.Hkv : L.Hq) * (L.S / BQ)), dim3(NT16), 0, \
                                   a.stream, a.q, a.k, a.v, a.dout, a.lse, a.delta, a.dk_p,      \
                                   a.dv_p, L.S, L.Hq, L.Hkv, L.q_tok, L.k_tok, L.v_tok, a.scale, \
                                   gqa ? a.dk : nullptr, gqa ? a.dv : nullptr,                   \
                                   gqa ? L.dk_tok : 0L, gqa ? L.dv_tok : 0L))
  switch (kind) {
    case DKDV_HEAD: MXK_DKDV16(false); break;
    case DKDV_GQA: MXK_DKDV16(true); break;
    case DKDV_GQA_DMA: MXK_DKDV16(true, true); break;
    case DKDV_GQA_DMA_PIPE: MXK_DKDV16(true, true, true); break;
    default: return static_cast<int>(hipErrorInvalidValue);   // one-pass: its own entry point
  }
#undef MXK_DKDV16
  MXK_RETURN_LAUNCH_STATUS();
}
}  // namespace

// The backward of `variant` (attention_plan.h lists them), or of the variant
// the layout degrades to: check, plan, launch the plan's stages.
MXK_API int mxk_attn_bwd_variant(const void* q, const void* k, const void* v, const void* o,
                                 const void* dout, const float* lse, void* dq, void* dk, void* dv,
                                 void* workspace, int B, int S, int Hq, int Hkv, int head_dim,
                                 long q_tok, long k_tok, long v_tok, long dk_tok, long dv_tok,
                                 float scale, int causal, int variant, hipStream_t stream) {
  const AttnLayout L{B, S, Hq, Hkv, q_tok, k_tok, v_tok, static_cast<long>(Hq) * D, dk_tok, dv_tok,
                     causal};
  const AttnBwdPlan p = attn_bwd_plan(L, variant);
  if (head_dim != D || p.variant < 0 || !attn_aligned(16, q, k, v, o, dout, dq, workspace) ||
      !attn_aligned(8, dk, dv))
    return static_cast<int>(hipErrorInvalidValue);
  if (p.dq == DQ_ATOMICS)   // not bit-reproducible
    return mxk_attn_bwd_onepass(q, k, v, o, dout, lse, dq, dk, dv, workspace, B, S, Hq, Hkv, q_tok,
                                k_tok, v_tok, dk_tok, dv_tok, scale, causal,
                                p.dkdv == DKDV_ONEPASS_BF16, stream);
  const long rows = static_cast<long>(B) * Hq * S;
  float* ws = static_cast<float*>(workspace);
  const BwdArgs a{bf(q), bf(k), bf(v), bf(o), bf(dout), lse, bf(dq), bf(dk), bf(dv), ws,
                  p.reduce ? ws + rows : nullptr, p.reduce ? ws + rows + rows * D : nullptr, scale,
                  stream};
  if (p.delta)
    hipLaunchKernelGGL(mxk_attn_bwd_delta_kernel, dim3((rows * 16 + 255) / 256), dim3(256), 0,
                       stream, a.o, a.dout, a.delta, S, Hq, rows);
  int st = p.dq_first ? launch_dq(p.dq, L, a) : 0;
  if (!st) st = launch_dkdv(p.dkdv, L, a);
  if (!st && !p.dq_first) st = launch_dq(p.dq, L, a);
  if (st || !p.reduce) return st;
  const long n_out = static_cast<long>(B) * S * Hkv * D;
  hipLaunchKernelGGL(mxk_attn_bwd_gqa_reduce_kernel, dim3((n_out / 4 + 255) / 256), dim3(256), 0,
                     stream, a.dk_p, a.dv_p, a.dk, a.dv, n_out, Hq, Hkv, dk_tok, dv_tok);
  MXK_RETURN_LAUNCH_STATUS();
}

MXK_API long mxk_attn_bwd_doc_workspace(int B, int S, int Hq) {
  return attn_bwd_workspace(B, S, Hq, 5);   // delta
}

// Backward variant 5 with a per-document causal mask (attention_plan.h):
// the FOLD dQ kernel's DOC form, writing delta, then the GQA DMA PIPE dK / dV
// kernel's.  doc_start / doc_end int32 [B, S]; workspace:
// mxk_attn_bwd_doc_workspace bytes.  hipErrorInvalidValue, with nothing
// launched, for a layout attn_doc_ok does not take or a null / misaligned
// pointer.
MXK_API int mxk_attn_bwd_doc(const void* q, const void* k, const void* v, const void* o,
                             const void* dout, const float* lse, void* dq, void* dk, void* dv,
                             void* workspace, const int* doc_start, const int* doc_end, int B,
                             int S, int Hq, int Hkv, int head_dim, long q_tok, long k_tok,
                             long v_tok, long dk_tok, long dv_tok, float scale,
                             hipStream_t stream) {
  const AttnLayout L{B, S, Hq, Hkv, q_tok, k_tok, v_tok, static_cast<long>(Hq) * D, dk_tok, dv_tok, 1};
  if (head_dim != D || !attn_doc_ok(L) || !q || !k || !v || !o || !dout || !lse || !dq || !dk ||
      !dv || !workspace || !doc_start || !doc_end ||
      !attn_aligned(16, q, k, v, o, dout, dq, workspace) || !attn_aligned(8, dk, dv) ||
      !attn_aligned(4, lse, doc_start, doc_end))
    return static_cast<int>(hipErrorInvalidValue);
  float* delta = static_cast<float*>(workspace);
  hipLaunchKernelGGL((mxk_attn_bwd_dq_kernel<true, true, true, false, true, false, true>),
                     dim3(B * Hq * (S / BQ)), dim3(NT), 0, stream, bf(q), bf(k), bf(v), bf(dout),
                     lse, nullptr, bf(dq), S, Hq, Hkv, q_tok, k_tok, v_tok, scale, bf(o), delta,
                     doc_start);
  const int st = static_cast<int>(hipGetLastError());
  if (st) return st;
  hipLaunchKernelGGL((mxk_attn_bwd_dkdv16_kernel<true, true, true, true, true>),
                     dim3(B * Hkv * (S / BQ)), dim3(NT16), 0, stream, bf(q), bf(k), bf(v),
                     bf(dout), lse, delta, nullptr, nullptr, S, Hq, Hkv, q_tok, k_tok, v_tok, scale,
                     bf(dk), bf(dv), dk_tok, dv_tok, doc_end);
  MXK_RETURN_LAUNCH_STATUS();
}
