// Host driver of 3dspa_code_amd/csrc/score_row.hpp (tests/test_score_row_host.py): the header is plain C++, so the per-frame classification and the
// per-row accumulator that the GPU kernels run are compiled here with the host compiler and fed rows from a binary file.
// Input (stdin, little-endian): int32 rows, then per row: int32 T, NC, K; float32 scale; float32 thr[8]; float32 p[T*NC], l[T], g[T*NC], y[T].
// Output (stdout): per row float32 stats[8 + 4K], then float32 frame_err[T].
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../3dspa_code_amd/csrc/score_row.hpp"

template <typename V> static bool rd(V* p, size_t n) { return fread(p, sizeof(V), n, stdin) == n; }

int main() {
  int32_t rows = 0;
  if (!rd(&rows, 1) || rows < 0) return 2;
  for (int32_t r = 0; r < rows; ++r) {
    int32_t hdr[3];
    float scale = 1.f;
    ScoreThr thr;
    if (!rd(hdr, 3) || !rd(&scale, 1) || !rd(thr.t, SCORE_MAX_K)) return 3;
    const int T = hdr[0], NC = hdr[1];
    thr.K = hdr[2];
    if (T <= 0 || NC <= 0 || NC > 3 || thr.K < 0 || thr.K > SCORE_MAX_K) return 4;
    std::vector<float> p((size_t)T * NC), l(T), g((size_t)T * NC), y(T), stats(score_row_len(thr.K)), fe(T);
    if (!rd(p.data(), p.size()) || !rd(l.data(), l.size()) || !rd(g.data(), g.size()) || !rd(y.data(), y.size())) return 5;
    score_row_host(p.data(), l.data(), g.data(), y.data(), T, NC, thr, scale, stats.data(), fe.data());
    if (fwrite(stats.data(), 4, stats.size(), stdout) != stats.size() || fwrite(fe.data(), 4, fe.size(), stdout) != fe.size()) return 6;
  }
  return 0;
}
