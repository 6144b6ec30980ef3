// attn_doc_ok against its definition over a sweep of layouts, and the tile /
// slice bounds the DOC kernels derive from a document table against a brute
// force over the mask, as a host program for the ASan + UBSan build
// (make test-attention-doc).
#include <climits>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "attention_plan.h"

namespace {
constexpr int TILE = 64, SLICE = 64, FWD_WAVE = 32, KEY_WAVE = 16;
long n_pts = 0, n_bad = 0;
void check(bool ok, const char* what, int a = 0, int b = 0, int c = 0) {
  ++n_pts;
  if (ok) return;
  if (++n_bad <= 20) std::printf("BAD %s (%d, %d, %d)\n", what, a, b, c);
}

void sweep_predicate() {
  for (int S : {64, 128, 192, 256, 384, 2048})
    for (int grp : {1, 2, 4})
      for (int spans = 0; spans < 4; ++spans)
        for (int causal = 0; causal < 2; ++causal)
          for (long dk_off : {0L, 2L, 4L}) {
            const long big = ((BUF_RANGE / 2 + S - 1) / S + 7) / 8 * 8;
            const int Hkv = 2, Hq = Hkv * grp;
            const long q_tok = spans & 2 ? big : Hq * D, kv_tok = spans & 1 ? big : Hkv * D;
            const AttnLayout L{1, S, Hq, Hkv, q_tok, kv_tok, kv_tok, Hq * D, Hkv * D + dk_off,
                               Hkv * D, causal};
            const bool want = causal && S >= BQ && S % BQ == 0 && dk_off % 4 == 0 && !(spans & 1) &&
                              !(spans & 2);
            check(attn_doc_ok(L) == want, "attn_doc_ok", S, spans, causal);
            check(attn_doc_ok(L) ==
                      (L.causal && attn_bwd_ok(L) && attn_kv_dma_ok(L) && attn_q_dma_ok(L)),
                  "attn_doc_ok definition", S, spans, causal);
          }
}

// visible(i, j): doc_start[i] <= j <= i
void sweep_table(int S, const std::vector<int>& given) {
  std::vector<int> starts;   // strictly increasing from 0, inside the row
  for (int x : given)
    if (x < S && (starts.empty() ? x == 0 : x > starts.back())) starts.push_back(x);
  std::vector<int> ds(S), de(S);
  for (size_t d = 0; d < starts.size(); ++d) {
    const int lo = starts[d], hi = d + 1 < starts.size() ? starts[d + 1] : S;
    for (int i = lo; i < hi; ++i) { ds[i] = lo; de[i] = hi; }
  }
  auto vis = [&](int i, int j) { return j <= i && j >= ds[i]; };
  // forward / dQ: query blocks of BQ rows, waves of 32 rows, tiles of 64 keys
  for (int q0 = 0; q0 < S; q0 += BQ)
    for (int align : {1, 2}) {
      const int j_lo = attn_doc_first_tile(ds[q0], q0, TILE, align), nkv = (q0 + BQ) / TILE;
      check(j_lo >= 0 && j_lo < nkv && j_lo % align == 0, "first tile range", S, q0, j_lo);
      for (int j = 0; j < nkv; ++j)
        for (int w = 0; w < BQ / FWD_WAVE; ++w) {
          const int qw0 = q0 + w * FWD_WAVE, kv0 = j * TILE;
          bool any = false, all = true;
          for (int i = qw0; i < qw0 + FWD_WAVE; ++i)
            for (int k = kv0; k < kv0 + TILE; ++k) {
              any = any || vis(i, k);
              all = all && (vis(i, k) || k > i);   // nothing for the lower mask to remove
            }
          const bool walked = j >= j_lo && kv0 <= qw0 + FWD_WAVE - 1 &&
                              attn_doc_tile_active(kv0, TILE, ds[qw0]);
          check(!any || walked, "visible key in a skipped tile", S, q0, j);
          // the skip is exact: a walked tile holds a visible key
          check(!walked || any, "walked tile without a visible key", S, q0, j);
          if (walked && !attn_doc_tile_masked(kv0, ds[qw0 + FWD_WAVE - 1]))
            check(all, "unmasked tile with a key before its row's document", S, q0, j);
        }
    }
  // dK / dV: key blocks of BQ keys, waves of 16 keys, slices of 64 query rows
  for (int k0 = 0; k0 < S; k0 += BQ) {
    const int nsl = attn_doc_slices(de[k0 + BQ - 1], k0, S, SLICE);
    check(nsl >= BQ / SLICE && k0 + nsl * SLICE <= S, "slice count range", S, k0, nsl);
    for (int t = 0; t < (S - k0) / SLICE; ++t)
      for (int w = 0; w < BQ / KEY_WAVE; ++w) {
        const int kw0 = k0 + w * KEY_WAVE, qs0 = k0 + t * SLICE;
        bool any = false, all = true;
        for (int k = kw0; k < kw0 + KEY_WAVE; ++k)
          for (int i = qs0; i < qs0 + SLICE; ++i) {
            any = any || vis(i, k);
            all = all && (vis(i, k) || k > i);
            // the key's side of the rule is the same mask
            check(vis(i, k) == (k <= i && i < de[k]), "doc_end form of the mask", S, i, k);
          }
        const bool walked = t < nsl && qs0 + SLICE - 1 >= kw0 &&
                            attn_doc_slice_active(qs0, de[kw0 + KEY_WAVE - 1]);
        check(!any || walked, "visible row in a skipped slice", S, k0, t);
        check(!walked || any, "walked slice without a visible row", S, k0, t);
        if (walked && !attn_doc_slice_masked(qs0, SLICE, de[kw0]))
          check(all, "unmasked slice with a row past its key's document", S, k0, t);
      }
  }
}

// whatever a table holds, the derived indices stay inside the causal range
void sweep_hardening() {
  for (int S : {128, 256, 1024})
    for (int blk = 0; blk < S; blk += BQ)
      for (int bad : {INT_MIN, INT_MIN + 1, -1, 0, 1, 63, 64, S - 1, S, S + 1, INT_MAX - 64, INT_MAX})
        for (int align : {1, 2}) {
          const int j_lo = attn_doc_first_tile(bad, blk, TILE, align);
          check(j_lo >= 0 && j_lo <= blk / TILE, "hardened first tile", S, blk, bad);
          const int nsl = attn_doc_slices(bad, blk, S, SLICE);
          check(nsl >= BQ / SLICE && blk + nsl * SLICE <= S, "hardened slice count", S, blk, bad);
        }
}
}  // namespace

int main() {
  sweep_predicate();
  for (int S : {128, 256, 384, 512}) {
    sweep_table(S, {0});
    sweep_table(S, {0, 64, 128, 192 < S ? 192 : S - 1});
    sweep_table(S, {0, 1, 37, 100, 129 < S ? 129 : 101, 200 < S ? 200 : 102, S - 1});
    sweep_table(S, {0, 100});
    sweep_table(S, {0, 96});
    sweep_table(S, {0, 127});
    sweep_table(S, {0, S - 64, S - 63});
    std::vector<int> every(S);
    for (int i = 0; i < S; ++i) every[i] = i;
    sweep_table(S, every);
  }
  sweep_hardening();
  std::printf("attention doc sweep: %ld points, %ld bad\n", n_pts, n_bad);
  return n_bad != 0;
}
