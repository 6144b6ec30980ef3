// Flash attention (causal / full, GQA, head_dim 128, bf16) for gfx950.
//
// The Llama-3-8B DDP validator step (BASELINE config 5) spends ~16 % of its
// time in attention; torch's SDPA backends on this image reach 140-150 TF/s.
// These kernels keep the S x S scores on chip (online softmax) and are
// written around CDNA4's 32x32x16 bf16 MFMA and 64-lane waves:
//
// Forward (mxk_attn_fwd_variant): one workgroup = 4 waves = 128 query rows of one
// (batch, q-head); each wave owns 32 query rows.  Per 64-key block:
//   * S^T = K . Q^T with the KEY as the MFMA row and the QUERY on the lane
//     ("swapped" QK^T): every lane holds 32 of its query's 64 scores, so the
//     row max / row sum are in-lane plus ONE permlane32_swap with the other
//     lane half - no LDS, no shuffles;
//   * P^T (bf16, straight from the accumulator registers) is the B operand
//     of O^T += V^T . P^T, whose A operand comes from LDS with the gfx950
//     transposed read ds_read_b64_tr_b16 - V is stored row-major as loaded;
//   * O^T accumulates with the query on the lane, so the online-softmax
//     rescale is a per-lane scalar multiply.
// K and V tiles are staged through registers into a double-buffered,
// XOR-swizzled LDS image (256-B rows, chunk c of row r at
// c ^ ((r&3)<<2 | (r>>2)&3)), conflict-free for both the row reads of K and
// the transposed reads of V (tests/test_attention_layout.py).
// Causal work is balanced by launching the heaviest query blocks first and
// pairing block i with block n-1-i across the two halves of the grid.
//
// Layouts: q [B, S, Hq, 128], k/v [B, S, Hkv, 128] with arbitrary token
// strides (so q/k/v can be views of the fused QKV projection), o
// [B, S, Hq, 128] contiguous, lse [B, Hq, S] fp32 (natural log of the row's
// sum of exp(scale * s)) for the backward pass.
#include "attention_common.h"

template <bool CAUSAL>
__global__ void __launch_bounds__(NT, 2)
mxk_attn_fwd_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                    const uint16_t* __restrict__ v, uint16_t* __restrict__ o,
                    float* __restrict__ lse, int S, int Hq, int Hkv, long q_tok, long k_tok,
                    long v_tok, float scale) {
  __shared__ __attribute__((aligned(16))) char smem[2][2 * TILE_BYTES];   // [buf][K | V]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31;
  const int h = lane >> 5;

  const int nqb = S / BQ;
  int bh, qb;
  map_block(blockIdx.x, gridDim.x / nqb, nqb, CAUSAL, &bh, &qb);
  const int b = bh / Hq, hq = bh % Hq;
  const int hkv = hq / (Hq / Hkv);
  const int q0 = qb * BQ;
  const int qw0 = q0 + wave * 32;
  const int myq = qw0 + r32;

  const uint16_t* qb_ptr = q + static_cast<long>(b) * S * q_tok + static_cast<long>(hq) * D;
  const uint16_t* kb_ptr = k + static_cast<long>(b) * S * k_tok + static_cast<long>(hkv) * D;
  const uint16_t* vb_ptr = v + static_cast<long>(b) * S * v_tok + static_cast<long>(hkv) * D;

  // Q^T fragments (B operand): lane holds Q[myq][16s + 8h .. +7]
  bf16x8_t qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s)
    qf[s] = *reinterpret_cast<const bf16x8_t*>(qb_ptr + static_cast<long>(myq) * q_tok + 16 * s + 8 * h);

  const int kv_end = CAUSAL ? min(S, q0 + BQ) : S;
  const int nkv = kv_end / BKV;

  // loader: thread t moves chunks t + 256 i (i = 0..3) of the 64 x 16-chunk tile
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
    char* kt = smem[buf];
    char* vt = smem[buf] + TILE_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = swz(ld_row + 16 * i, ld_ch);
      *reinterpret_cast<bf16x8_t*>(kt + off) = kst[i];
      *reinterpret_cast<bf16x8_t*>(vt + off) = vst[i];
    }
  };
  load_tile(0);
  store_tile(0);
  __syncthreads();

  const float c = scale * 1.4426950408889634f;   // scores -> log2 domain
  float m = -INFINITY, l = 0.f;
  f32x16_t acc[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[db][r] = 0.f;

  // per-lane parts of the transposed-read addresses of V (see header)
  const int G = lane >> 4, i16 = lane & 15;
  const int tr_key = 4 * h + (i16 >> 2);                          // + 32kb + 16s' + 8jh
  const int tr_ch = 2 * (G & 1) + ((i16 & 3) >> 1);               // + 4db
  const int tr_byte = 8 * (i16 & 1);

  for (int j = 0; j < nkv; ++j) {
    const int buf = j & 1;
    if (j + 1 < nkv) load_tile(j + 1);
    const int kv0 = j * BKV;
    const bool active = !CAUSAL || kv0 <= qw0 + 31;
    if (active) {
      const char* kt = smem[buf];
      const char* vt = smem[buf] + TILE_BYTES;
      // ---- S^T = K . Q^T : two 32-key halves
      f32x16_t s0, s1;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const bf16x8_t a0 = lds_b128(kt + swz(r32, 2 * s + h));
        const bf16x8_t a1 = lds_b128(kt + swz(32 + r32, 2 * s + h));
        s0 = mfma32(a0, qf[s], s0);
        s1 = mfma32(a1, qf[s], s1);
      }
      if (CAUSAL && kv0 + BKV - 1 > qw0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kv0 + crow(r, h);
          if (key > myq) s0[r] = -INFINITY;
          if (key + 32 > myq) s1[r] = -INFINITY;
        }
      }
      // ---- online softmax (query = lane, keys in registers + other half)
      float mx = s0[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s0[r]);
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s1[r]);
      mx = half_max(mx);
      const float m_new = fmaxf(m, mx);
      const float alpha = fexp2((m - m_new) * c);
      m = m_new;
      const float mc = m_new * c;
      float ls = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s0[r] = fexp2(fmaf(s0[r], c, -mc));
        s1[r] = fexp2(fmaf(s1[r], c, -mc));
        ls += s0[r] + s1[r];
      }
      l = l * alpha + ls;
      if (__builtin_amdgcn_ballot_w64(alpha != 1.f)) {   // wave-uniform: some row max moved
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[db][r] *= alpha;
      }
      // P^T fragments for the 4 16-key k-steps
      bf16x8_t pf[4];
      pf[0] = pack8(s0, 0);
      pf[1] = pack8(s0, 8);
      pf[2] = pack8(s1, 0);
      pf[3] = pack8(s1, 8);
      // ---- O^T += V^T . P^T
#pragma unroll
      for (int db = 0; db < 4; ++db) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int key = 16 * ks + tr_key;
          const int ch = 4 * db + tr_ch;
          const bf16x4_t lo = lds_tr_b64(vt + swz(key, ch) + tr_byte);
          const bf16x4_t hi = lds_tr_b64(vt + swz(key + 8, ch) + tr_byte);
          const bf16x8_t a = cat8(lo, hi);
          acc[db] = mfma32(a, pf[ks], acc[db]);
        }
      }
    }
    if (j + 1 < nkv) store_tile(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue: normalise, store O[b][myq][hq][:] and the row LSE
  const float lt = half_sum(l);
  const float inv = 1.f / lt;
  uint16_t* orow = o + (static_cast<long>(b) * S + myq) * Hq * D + static_cast<long>(hq) * D;
#pragma unroll
  for (int db = 0; db < 4; ++db) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = 32 * db + 8 * g + 4 * h;
      uint2 pk;
      pk.x = mxk::pack2bf(acc[db][4 * g] * inv, acc[db][4 * g + 1] * inv);
      pk.y = mxk::pack2bf(acc[db][4 * g + 2] * inv, acc[db][4 * g + 3] * inv);
      *reinterpret_cast<uint2*>(orow + d) = pk;
    }
  }
  if (h == 0) lse[(static_cast<long>(b) * Hq + hq) * S + myq] = m * scale + logf(lt);
}

// ---------------------------------------------------------------------------
// Forward, DMA-fed (the default): the same math and LDS image, but
//   * K/V tiles land in LDS by LDS-DMA (`buffer_load ... lds`, swizzle applied
//     on the source address) issued at the top of the iteration for the next
//     tile: no staging VGPRs, no ds_writes, and no 64-bit address arithmetic
//     per tile (one SGPR offset);
//   * the per-lane LDS read offsets of K (8) and V (8) are loop invariants;
//   * scale-and-shift and the row sum use packed fp32 (v_pk_fma_f32,
//     v_pk_add_f32), halving the softmax's full-rate VALU work.
// Requires S * token_stride * 2 < 2^32 for K and V (buffer offsets).

// DOC (mxk_attn_fwd_doc; with CAUSAL): causal within a document.  The walk
// starts at the tile of doc_start[q0] (rounded down to an even tile under
// UNROLL, so the LDS buffers stay compile-time), a wave skips the tiles that
// end before its first row's document, and the tiles that begin before its
// last row's document mask key < doc_start[row] per score.
template <bool CAUSAL, bool UNROLL, bool PIPE = false, bool DOC = false>
__global__ void __launch_bounds__(NT, 2)
mxk_attn_fwd_dma_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                        const uint16_t* __restrict__ v, uint16_t* __restrict__ o,
                        float* __restrict__ lse, int S, int Hq, int Hkv, long q_tok, long k_tok,
                        long v_tok, float scale, const int* __restrict__ doc_start = nullptr) {
  static_assert(!DOC || CAUSAL, "a document table masks causal attention only");
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
  const uint16_t* kb_ptr = k + static_cast<long>(b) * S * k_tok + static_cast<long>(hkv) * D;
  const uint16_t* vb_ptr = v + static_cast<long>(b) * S * v_tok + static_cast<long>(hkv) * D;

  bf16x8_t qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s)
    qf[s] = *reinterpret_cast<const bf16x8_t*>(qb_ptr + static_cast<long>(myq) * q_tok + 16 * s + 8 * h);

  const int kv_end = CAUSAL ? min(S, q0 + BQ) : S;
  const int nkv = kv_end / BKV;
  // DOC: the block's first tile and the wave's bounds through uniform
  // addresses (scalar loads), the lane's own row next to its Q fragments
  int j_lo = 0, ds_w0 = 0, ds_w1 = 0, ds_row = 0;
  if constexpr (DOC) {
    const int* ds_b = doc_start + static_cast<long>(b) * S;
    j_lo = attn_doc_first_tile(ds_b[q0], q0, BKV, UNROLL ? 2 : 1);
    ds_w0 = ds_b[qw0];
    ds_w1 = ds_b[qw0 + 31];
    ds_row = ds_b[myq];
  }

  // DMA: wave w moves the 1-KiB pieces g = 4w + p (rows 4g .. 4g+3) of K and
  // V; lane i lands at row 4g + (i >> 4), slot i & 15, so it fetches chunk
  // (i & 15) ^ f(row) with f(row) = (row & 3) << 2 | (row >> 2) & 3
  // = (i >> 4) << 2 | p.
  const mxk::u32x4 rk = mxk::make_rsrc(kb_ptr, static_cast<unsigned>(S * k_tok * 2));
  const mxk::u32x4 rv = mxk::make_rsrc(vb_ptr, static_cast<unsigned>(S * v_tok * 2));
  const int prow = lane >> 4, pslot = lane & 15;
  uint32_t kvo[4], vvo[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int row = 4 * (4 * wave + p) + prow;
    const int ch = pslot ^ ((prow << 2) | p);
    kvo[p] = static_cast<uint32_t>(row * k_tok * 2 + ch * 16);
    vvo[p] = static_cast<uint32_t>(row * v_tok * 2 + ch * 16);
  }
  const uint32_t k_step = static_cast<uint32_t>(BKV * k_tok * 2);
  const uint32_t v_step = static_cast<uint32_t>(BKV * v_tok * 2);
  // LDS destinations as scalar 32-bit addresses bound to M0 (mxk::dma16m)
  const uint32_t sm32 = mxk::lds_addr32(&smem[0][0]);
  auto issue = [&](int j, int buf) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint32_t d = sm32 + buf * (2 * TILE_BYTES) + (4 * wave + p) * 1024;
      mxk::dma16m(rk, d, kvo[p], j * k_step);
      mxk::dma16m(rv, d + TILE_BYTES, vvo[p], j * v_step);
    }
  };
  issue(j_lo, j_lo & 1);

  // loop-invariant LDS read offsets: K rows r32 (+32 rows = +8 KiB), chunk
  // 2s + h; V transposed reads at keys tr_key (+8), chunk 4db + tr_ch, with
  // +16 keys = +4 KiB per k-step
  int koff[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) koff[s] = swz(r32, 2 * s + h);
  const int G = lane >> 4, i16 = lane & 15;
  const int tr_key = 4 * h + (i16 >> 2);
  const int tr_ch = 2 * (G & 1) + ((i16 & 3) >> 1);
  const int tr_byte = 8 * (i16 & 1);
  int voff[4][2];
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    voff[db][0] = swz(tr_key, 4 * db + tr_ch) + tr_byte;
    voff[db][1] = swz(tr_key + 8, 4 * db + tr_ch) + tr_byte;
  }

  const float c = scale * 1.4426950408889634f;   // scores -> log2 domain
  const f32x2_t cc = {c, c};
  // DOC: a row whose document starts after an active tile has every score of
  // that tile at -inf.  With m = -inf the shift would be -inf + inf = NaN;
  // from a finite floor no score reaches, m_new stays the floor, the shift
  // m c is finite, P = exp2(-inf) = 0 and alpha = 1: the lane's m, l and acc
  // stay as they were.  The first visible score then rescales by
  // exp2(-huge) = 0, as it does from -inf.
  float m = DOC ? -1.7e38f / fmaxf(1.f, c) : -INFINITY, l = 0.f;
  f32x16_t acc[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[db][r] = 0.f;

  // Consume the Q fragments here: the compiler then waits for their loads
  // before the loop instead of placing vmcnt waits inside it, where they
  // would also wait for the next tile's (untracked) DMA.
#pragma unroll
  for (int s = 0; s < 8; ++s) asm volatile("" ::"v"(qf[s]));
  if constexpr (DOC) asm volatile("" ::"v"(ds_row));
  vm_wait<0>();   // tile 0 (DOC: tile j_lo)
  __syncthreads();

  // the loop body; UNROLL makes the LDS buffer a compile-time constant (read
  // addresses are then loop-invariant VGPRs + immediate offsets)
  auto step = [&](int j, int buf) {
    // buffer buf^1 was last read in iteration j-1 (barrier-certified)
    if (j + 1 < nkv) issue(j + 1, buf ^ 1);
    const int kv0 = j * BKV;
    bool active = !CAUSAL || kv0 <= qw0 + 31;
    if constexpr (DOC) active = active && attn_doc_tile_active(kv0, BKV, ds_w0);
    if (active) {
      const char* kt = smem[buf];
      const char* vt = smem[buf] + TILE_BYTES;
      f32x16_t s0, s1;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
      bf16x8_t vop[16];   // V^T operands [4 db + ks] (PIPE)
      auto read_v = [&](int x) {
        vop[x] = cat8(lds_tr_b64(vt + voff[x >> 2][0] + (x & 3) * 4096),
                      lds_tr_b64(vt + voff[x >> 2][1] + (x & 3) * 4096));
      };
      if constexpr (PIPE) {
        // K operands a k-step pair ahead (two-slot ring), the first V^T
        // operands under the last S MFMAs and the softmax, the rest one db
        // ahead of the PV MFMAs; sched_barrier fences keep the order (the
        // plain loop below gets read -> lgkmcnt(0) -> MFMA per instruction)
        bf16x8_t ka[2][4];
        auto read_k = [&](int pr, int slot) {
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            ka[slot][2 * e] = lds_b128(kt + koff[2 * pr + e]);
            ka[slot][2 * e + 1] = lds_b128(kt + koff[2 * pr + e] + 32 * 256);
          }
        };
        read_k(0, 0);
#pragma unroll
        for (int pr = 0; pr < 4; ++pr) {
          if (pr < 3) read_k(pr + 1, (pr + 1) & 1);
          else
#pragma unroll
            for (int x = 0; x < 4; ++x) read_v(x);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            s0 = mfma32(ka[pr & 1][2 * e], qf[2 * pr + e], s0);
            s1 = mfma32(ka[pr & 1][2 * e + 1], qf[2 * pr + e], s1);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int x = 4; x < 8; ++x) read_v(x);
      } else {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const bf16x8_t a0 = lds_b128(kt + koff[s]);
          const bf16x8_t a1 = lds_b128(kt + koff[s] + 32 * 256);
          s0 = mfma32(a0, qf[s], s0);
          s1 = mfma32(a1, qf[s], s1);
        }
      }
      if (CAUSAL && kv0 + BKV - 1 > qw0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kv0 + crow(r, h);
          if (key > myq) s0[r] = -INFINITY;
          if (key + 32 > myq) s1[r] = -INFINITY;
        }
      }
      if constexpr (DOC) {
        if (attn_doc_tile_masked(kv0, ds_w1)) {   // wave-uniform
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = kv0 + crow(r, h);
            if (key < ds_row) s0[r] = -INFINITY;
            if (key + 32 < ds_row) s1[r] = -INFINITY;
          }
        }
      }
      float mx = s0[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s0[r]);
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s1[r]);
      mx = half_max(mx);
      float m_new = fmaxf(m, mx);
      bool grow = true;
      if constexpr (PIPE) {
        // Lazy rescale: keep the stale row max unless the new one exceeds it
        // by more than 2^8 (log2 units).  P = exp2((s - m) c) then stays
        // <= 256 - exact in bf16's exponent range - and l / acc stay
        // consistent with the m they were built with (final o = acc / l,
        // lse = m scale + ln l).  On random data almost every block after the
        // first skips the 32 v_pk_mul of the accumulator rescale.
        grow = (m_new - m) * c > 8.f;
        if (!grow) m_new = m;
      }
      const float alpha = grow ? fexp2((m - m_new) * c) : 1.f;
      m = m_new;
      const f32x2_t nmc = {-m_new * c, -m_new * c};
      if constexpr (PIPE) {
        // P in four 16-key chunks: the exp of chunk ks + 1 runs on the VALU
        // while the four PV MFMAs of chunk ks run on the matrix core (one
        // wave overlaps its own softmax with its own MFMAs)
#pragma unroll
        for (int x = 8; x < 16; ++x) read_v(x);
        if (__builtin_amdgcn_ballot_w64(grow)) {
#pragma unroll
          for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[db][r] *= alpha;
        }
        f32x2_t ls2 = {0.f, 0.f};
        auto chunk = [&](int ks) {
          f32x16_t& x = ks < 2 ? s0 : s1;
          const int base = (ks & 1) * 8;
#pragma unroll
          for (int r = 0; r < 8; r += 2) {
            f32x2_t y = {x[base + r], x[base + r + 1]};
            y = __builtin_elementwise_fma(y, cc, nmc);
            y[0] = fexp2(y[0]);
            y[1] = fexp2(y[1]);
            ls2 += y;
            x[base + r] = y[0];
            x[base + r + 1] = y[1];
          }
          return pack8(x, base);
        };
        bf16x8_t pf[4];
        pf[0] = chunk(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
          for (int db = 0; db < 4; ++db) acc[db] = mfma32(vop[4 * db + ks], pf[ks], acc[db]);
          if (ks < 3) pf[ks + 1] = chunk(ks + 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        l = l * alpha + (ls2[0] + ls2[1]);
      } else {
        f32x2_t ls2 = {0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          f32x2_t x0 = {s0[r], s0[r + 1]};
          f32x2_t x1 = {s1[r], s1[r + 1]};
          x0 = __builtin_elementwise_fma(x0, cc, nmc);
          x1 = __builtin_elementwise_fma(x1, cc, nmc);
          x0[0] = fexp2(x0[0]);
          x0[1] = fexp2(x0[1]);
          x1[0] = fexp2(x1[0]);
          x1[1] = fexp2(x1[1]);
          ls2 += x0 + x1;
          s0[r] = x0[0];
          s0[r + 1] = x0[1];
          s1[r] = x1[0];
          s1[r + 1] = x1[1];
        }
        l = l * alpha + (ls2[0] + ls2[1]);
        if (__builtin_amdgcn_ballot_w64(alpha != 1.f)) {
#pragma unroll
          for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[db][r] *= alpha;
        }
        bf16x8_t pf[4];
        pf[0] = pack8(s0, 0);
        pf[1] = pack8(s0, 8);
        pf[2] = pack8(s1, 0);
        pf[3] = pack8(s1, 8);
#pragma unroll
        for (int db = 0; db < 4; ++db) {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const bf16x4_t lo = lds_tr_b64(vt + voff[db][0] + ks * 4096);
            const bf16x4_t hi = lds_tr_b64(vt + voff[db][1] + ks * 4096);
            acc[db] = mfma32(cat8(lo, hi), pf[ks], acc[db]);
          }
        }
      }
    }
    // tile j+1 (own pieces) landed; the barrier publishes every wave's pieces
    // and certifies that buffer buf is no longer read
    vm_wait<0>();
    __syncthreads();
  };
  if constexpr (UNROLL) {
    for (int j = j_lo; j < nkv; j += 2) {   // j_lo is even
      step(j, 0);
      if (j + 1 < nkv) step(j + 1, 1);
    }
  } else {
    for (int j = j_lo; j < nkv; ++j) step(j, j & 1);
  }

  const float lt = half_sum(l);
  const float inv = 1.f / lt;
  uint16_t* orow = o + (static_cast<long>(b) * S + myq) * Hq * D + static_cast<long>(hq) * D;
  // 16-B stores: v_permlane32_swap pairs groups g = 2k, 2k+1 across the lane
  // halves, so lane half h holds d = 32 db + 16 k + 8 h + 0..7 (half h of
  // group g holds 4 h + 0..3 of its 8)
#pragma unroll
  for (int db = 0; db < 4; ++db) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int g0 = 2 * kk, g1 = 2 * kk + 1;
      const uint32_t x0 = mxk::pack2bf(acc[db][4 * g0] * inv, acc[db][4 * g0 + 1] * inv);
      const uint32_t x1 = mxk::pack2bf(acc[db][4 * g0 + 2] * inv, acc[db][4 * g0 + 3] * inv);
      const uint32_t y0 = mxk::pack2bf(acc[db][4 * g1] * inv, acc[db][4 * g1 + 1] * inv);
      const uint32_t y1 = mxk::pack2bf(acc[db][4 * g1 + 2] * inv, acc[db][4 * g1 + 3] * inv);
      const auto p0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
      const auto p1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
      uint4 ov;
      ov.x = p0[0];
      ov.y = p1[0];
      ov.z = p0[1];
      ov.w = p1[1];
      *reinterpret_cast<uint4*>(orow + 32 * db + 16 * kk + 8 * h) = ov;
    }
  }
  if (h == 0) lse[(static_cast<long>(b) * Hq + hq) * S + myq] = m * scale + logf(lt);
}

// ---------------------------------------------------------------------------
// variant: 0 = register-staged K/V, 1 = LDS-DMA with the loop unrolled by 2
// (static LDS buffer), 2 = LDS-DMA, 3 = 2 with the PIPE body (operands read a
// group ahead, exp of P chunk ks+1 under the PV MFMAs of chunk ks, lazy
// rescale), 4 = 3 unrolled by 2 (default: the per-iteration v_or of the
// buffer base into 22 LDS addresses disappears).  1-4 fall back to 0 when a
// K/V panel exceeds the 32-bit buffer range.  B=8 Llama shape: 0.42 / 0.43 /
// 0.38 ms (profiles/r1_attention/); round 2: 2 / 3 / 4 = 0.3387 / 0.3218 /
// 0.3133 ms (profiles/r2_attention/fwd_lazy_rescale_unroll_ab.log).
#ifdef MXK_GEMM_EXPERIMENTS
int mxk_attn_fwd_exp_launch(int variant, const uint16_t* qp, const uint16_t* kp, const uint16_t* vp,
                            uint16_t* op, float* lse, int B, int S, int Hq, int Hkv, long q_tok,
                            long k_tok, long v_tok, float scale, int causal, hipStream_t stream);
#endif

MXK_API int mxk_attn_fwd_variant(const void* q, const void* k, const void* v, void* o, float* lse,
                                 int B, int S, int Hq, int Hkv, int head_dim, long q_tok,
                                 long k_tok, long v_tok, float scale, int causal, int variant,
                                 hipStream_t stream) {
  const AttnLayout L{B, S, Hq, Hkv, q_tok, k_tok, v_tok, 0, 0, 0, causal};
  if (head_dim != D || !attn_fwd_ok(L) || variant < 0 || variant > 10 ||
      !attn_aligned(16, q, k, v, o))
    return static_cast<int>(hipErrorInvalidValue);
  if (variant == 10) {
    // one wave per SIMD, two 32-row groups per wave (attention_fwd256.hip);
    // shapes it does not take (S % 256, 32-bit offsets) run variant 4
    if (attn_fwd256_ok(L))
      return mxk_attn_fwd256(q, k, v, o, lse, B, S, Hq, Hkv, q_tok, k_tok, v_tok, scale, causal,
                             stream);
    variant = 4;
  }
  const int nwg = B * Hq * (S / BQ);
  if (variant != 0 && !attn_kv_dma_ok(L)) variant = 0;
  const uint16_t *qp = bf(q), *kp = bf(k), *vp = bf(v);
  uint16_t* op = bf(o);
  if (variant >= 5) {
#ifdef MXK_GEMM_EXPERIMENTS
    // A/B records 5-9 (experiments/attention_fwd_exp.hip); -1: shape not
    // tiled by that variant, run variant 4
    const int st = mxk_attn_fwd_exp_launch(variant, qp, kp, vp, op, lse, B, S, Hq, Hkv, q_tok, k_tok,
                                           v_tok, scale, causal, stream);
    if (st >= 0) return st;
    variant = 4;
#else
    return static_cast<int>(hipErrorNotSupported);
#endif
  }
#define MXK_FWD(...)                                                                          \
  MXK_WITH_BOOL(C, causal,                                                                    \
                hipLaunchKernelGGL((__VA_ARGS__), dim3(nwg), dim3(NT), 0, stream, qp, kp, vp, \
                                   op, lse, S, Hq, Hkv, q_tok, k_tok, v_tok, scale))
  switch (variant) {   // mxk_attn_fwd_dma_kernel<CAUSAL, UNROLL, PIPE>
    case 4: MXK_FWD(mxk_attn_fwd_dma_kernel<C, true, true>); break;
    case 3: MXK_FWD(mxk_attn_fwd_dma_kernel<C, false, true>); break;
    case 2: MXK_FWD(mxk_attn_fwd_dma_kernel<C, false>); break;
    case 1: MXK_FWD(mxk_attn_fwd_dma_kernel<C, true>); break;
    default: MXK_FWD(mxk_attn_fwd_kernel<C>);
  }
#undef MXK_FWD
  MXK_RETURN_LAUNCH_STATUS();
}

// 1 if forward variant v is in this build (5-9 only in the experiments library)
MXK_API int mxk_attn_fwd_variant_built(int v) {
  if (v == 10) return 1;
#ifdef MXK_GEMM_EXPERIMENTS
  return v >= 0 && v <= 9;
#else
  return v >= 0 && v <= 4;
#endif
}

// Forward variant 4 with a per-document causal mask (attention_plan.h):
// doc_start int32 [B, S].  hipErrorInvalidValue, with nothing launched, for a
// layout attn_doc_ok does not take or a null / misaligned pointer.
MXK_API int mxk_attn_fwd_doc(const void* q, const void* k, const void* v, void* o, float* lse,
                             const int* doc_start, int B, int S, int Hq, int Hkv, int head_dim,
                             long q_tok, long k_tok, long v_tok, float scale, hipStream_t stream) {
  const AttnLayout L{B, S, Hq, Hkv, q_tok, k_tok, v_tok, static_cast<long>(Hq) * D,
                     static_cast<long>(Hkv) * D, static_cast<long>(Hkv) * D, 1};
  if (head_dim != D || !attn_doc_ok(L) || !q || !k || !v || !o || !lse || !doc_start ||
      !attn_aligned(16, q, k, v, o) || !attn_aligned(4, lse, doc_start))
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL((mxk_attn_fwd_dma_kernel<true, true, true, true>), dim3(B * Hq * (S / BQ)),
                     dim3(NT), 0, stream, bf(q), bf(k), bf(v), bf(o), lse, S, Hq, Hkv, q_tok, k_tok,
                     v_tok, scale, doc_start);
  MXK_RETURN_LAUNCH_STATUS();
}
