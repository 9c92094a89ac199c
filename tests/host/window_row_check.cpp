// Host driver of 3dspa_code_amd/csrc/window_row.hpp (tests/test_windows_host.py): the header is plain C++, so the plan check, the weights and the
// blend that the stitch kernel runs are compiled here with the host compiler and fed cases from a binary stream, walked as the kernel walks
// them: rows, then chunks of 64 frames with the chunk's window range, then frames.
// Input (stdin, little-endian): int32 cases, then per case: int32 W, N, Tw, TL, NC, blend, has_len; int32 t0[W]; int32 len[W] if has_len;
//   float32 src[W * N * Tw * NC].
// Output (stdout): per case int32 plan status (wr_plan_check) and where; if the plan is good: float32 out[N * TL * NC], float32 spread2[N * TL]
//   (the squared spread, before the square root), int32 count[N * TL] (contributing windows).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../3dspa_code_amd/csrc/window_row.hpp"

template <typename V> static bool rd(V* p, size_t n) { return n == 0 || fread(p, sizeof(V), n, stdin) == n; }
template <typename V> static bool wr(const V* p, size_t n) { return n == 0 || fwrite(p, sizeof(V), n, stdout) == n; }

int main() {
  int32_t cases = 0;
  if (!rd(&cases, 1) || cases < 0) return 2;
  for (int32_t k = 0; k < cases; ++k) {
    int32_t hdr[7];
    if (!rd(hdr, 7)) return 3;
    const int W = hdr[0], N = hdr[1], Tw = hdr[2], TL = hdr[3], NC = hdr[4], blend = hdr[5], has_len = hdr[6];
    if (W < 1 || W > WR_MAX_W || N < 1 || Tw < 1 || TL < 1 || NC < 1 || NC > 3) return 4;
    std::vector<int32_t> t0(W), len(W);
    if (!rd(t0.data(), W) || (has_len && !rd(len.data(), W))) return 5;
    std::vector<float> src((size_t)W * N * Tw * NC);
    if (!rd(src.data(), src.size())) return 6;
    int where = 0;
    const int32_t st[2] = {wr_plan_check(W, Tw, TL, t0.data(), has_len ? len.data() : nullptr, &where), where};
    if (!wr(st, 2)) return 7;
    if (st[0] != WR_PLAN_OK) continue;
    WrPlan p;
    p.W = W; p.Tw = Tw; p.TL = TL; p.blend = blend;
    for (int w = 0; w < W; ++w) { p.t0[w] = t0[w]; p.len[w] = has_len ? len[w] : wr_window_len(t0[w], Tw, TL); }
    std::vector<float> out((size_t)N * TL * NC), s2((size_t)N * TL);
    std::vector<int32_t> cnt((size_t)N * TL);
    for (int r = 0; r < N; ++r)
      for (int tc = 0; tc < TL; tc += 64) {
        int wlo, whi;
        wr_window_range(p, tc, tc + 63 < TL - 1 ? tc + 63 : TL - 1, wlo, whi);
        for (int t = tc; t < TL && t < tc + 64; ++t) {
          const size_t o = (size_t)r * TL + t;
          float* dst = out.data() + o * NC;
          cnt[o] = NC == 1 ? wr_point<1>(p, wlo, whi, src.data(), N, r, t, dst, &s2[o])
                           : (NC == 2 ? wr_point<2>(p, wlo, whi, src.data(), N, r, t, dst, &s2[o]) : wr_point<3>(p, wlo, whi, src.data(), N, r, t, dst, &s2[o]));
        }
      }
    if (!wr(out.data(), out.size()) || !wr(s2.data(), s2.size()) || !wr(cnt.data(), cnt.size())) return 8;
  }
  return 0;
}
