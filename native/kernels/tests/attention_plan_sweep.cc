// attn_bwd_plan over the sweep of tests/test_attention_plan.py, as a host
// program for the ASan + UBSan build (make test-attention-plan).
#include <cstdio>
#include <initializer_list>

#include "attention_plan.h"

int main() {
  long n = 0, bad = 0;
  for (int variant = -1; variant <= 10; ++variant)
    for (int S : {64, 128, 256, 384, 512, 2048})
      for (int grp : {1, 2, 4, 8})
        for (int spans = 0; spans < 4; ++spans)
          for (int causal = 0; causal < 2; ++causal, ++n) {
            const long big = ((BUF_RANGE / 2 + S - 1) / S + 7) / 8 * 8;
            const int Hkv = 2, Hq = Hkv * grp;
            const long q_tok = spans & 2 ? big : Hq * D, kv_tok = spans & 1 ? big : Hkv * D;
            const AttnLayout L{1, S, Hq, Hkv, q_tok, kv_tok, kv_tok, Hq * D, Hkv * D, Hkv * D, causal};
            const AttnBwdPlan p = attn_bwd_plan(L, variant);
            const bool valid = S >= BQ && variant >= 0 && variant <= 9;
            if ((p.variant >= 0) != valid) ++bad;
            if (valid && attn_bwd_workspace(1, S, Hq, variant) < p.workspace) ++bad;
            if (valid && p.dkdv >= DKDV_256 && !attn_dkdv256_ok(L)) ++bad;
            if (valid && p.dq == DQ_256 && !attn_dq256_ok(L)) ++bad;
          }
  std::printf("attention plan sweep: %ld points, %ld bad\n", n, bad);
  return bad != 0;
}
