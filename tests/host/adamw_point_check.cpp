// Host driver of 3dspa_code_amd/csrc/adamw_point.hpp (tests/test_adamw_groups_host.py): the header is plain C++, so the per-element arithmetic of
// the grouped optimizer kernels -- clip, both moments, bias corrections, the update, the weight EMA -- is compiled here with the host compiler.
// Input (stdin, little-endian): float32 sc, b1, b2, eps, t (updates applied + 1), d (EMA decay); int32 n; n records
//                               {float32 lr_g, wd_g, p, g, m, v, e}.
// Output: float32 bc1, bc2, then per record float32 p_new, m_new, v_new, e_new.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../3dspa_code_amd/csrc/adamw_point.hpp"

struct Rec { float lr_g, wd_g, p, g, m, v, e; };

template <typename V> static bool rd(V* p, size_t n) { return n == 0 || fread(p, sizeof(V), n, stdin) == n; }

int main() {
  float h[6]; int32_t n = 0;
  if (!rd(h, 6) || !rd(&n, 1) || n < 0 || n > (1 << 22)) return 2;
  std::vector<Rec> recs((size_t)n);
  if (!rd(recs.data(), recs.size())) return 3;
  AdamwCoef c;
  c.sc = h[0]; c.b1 = h[1]; c.b2 = h[2]; c.eps = h[3];
  c.bc1 = adamw_bias_correction(h[4], c.b1); c.bc2 = adamw_bias_correction(h[4], c.b2);
  const float d = h[5], omd = 1.f - d;
  std::vector<float> out = {c.bc1, c.bc2};
  for (const Rec& r : recs) {
    float m = r.m, v = r.v;
    const float pn = adamw_point(c, r.lr_g, r.wd_g, r.p, r.g, m, v);
    out.push_back(pn); out.push_back(m); out.push_back(v); out.push_back(adamw_ema_point(r.e, d, omd, pn));
  }
  return fwrite(out.data(), sizeof(float), out.size(), stdout) == out.size() ? 0 : 4;
}
