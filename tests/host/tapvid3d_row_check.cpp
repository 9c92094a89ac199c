// Host driver of 3dspa_code_amd/csrc/tapvid3d_row.hpp (tests/test_tapvid3d_row_host.py): the header is plain C++, so the frame arithmetic, the
// per-row accumulator and the digit walk of the median select that the GPU kernels run are compiled here with the host compiler.
// Input (stdin, little-endian): int32 mode.
//   mode 0, rows:   int32 R, T, scaling, fixed; then per row float32 qt, s, fx, fy; p[T*3], l[T], g[T*3], y[T].
//                   Output per row: float32 stats[24], float32 scale used, float32 ratio[T].
//   mode 1, median: int32 sets; then per set int64 n, float32 x[n].  Output per set: float32 median.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../3dspa_code_amd/csrc/tapvid3d_row.hpp"

template <typename V> static bool rd(V* p, size_t n) { return n == 0 || fread(p, sizeof(V), n, stdin) == n; }
template <typename V> static bool wr(const V* p, size_t n) { return n == 0 || fwrite(p, sizeof(V), n, stdout) == n; }

int main() {
  int32_t mode = -1;
  if (!rd(&mode, 1)) return 2;
  if (mode == 0) {
    int32_t hdr[4];
    if (!rd(hdr, 4)) return 3;
    const int R = hdr[0], T = hdr[1], scaling = hdr[2], fixed = hdr[3];
    if (R < 0 || T <= 0 || scaling < 0 || scaling > 2) return 4;
    std::vector<float> p((size_t)T * 3), l(T), g((size_t)T * 3), y(T), ratio(T), stats(TV_S);
    for (int r = 0; r < R; ++r) {
      float q[4];
      if (!rd(q, 4) || !rd(p.data(), p.size()) || !rd(l.data(), l.size()) || !rd(g.data(), g.size()) || !rd(y.data(), y.size())) return 5;
      const float s = tv_row_host(p.data(), l.data(), g.data(), y.data(), T, q[0], scaling, q[1], q[2], q[3], fixed != 0, stats.data(), ratio.data());
      if (!wr(stats.data(), stats.size()) || !wr(&s, 1) || !wr(ratio.data(), ratio.size())) return 6;
    }
    return 0;
  }
  if (mode == 1) {
    int32_t sets = 0;
    if (!rd(&sets, 1) || sets < 0) return 3;
    for (int i = 0; i < sets; ++i) {
      int64_t n = 0;
      if (!rd(&n, 1) || n < 0) return 4;
      std::vector<float> x((size_t)n);
      if (!rd(x.data(), x.size())) return 5;
      const float m = tv_median_host(x.data(), n);
      if (!wr(&m, 1)) return 6;
    }
    return 0;
  }
  return 1;
}
