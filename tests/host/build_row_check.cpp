// Host driver over csrc/build_row.hpp (tests/test_build_row_host.py): the arithmetic the kernel of spa3d_build_batch runs, compiled with g++.
//   build_row_check sample   stdin: int32 N, T, D, Hp, Wp, H, W, has_intr; double intr[4]; f32 tracks [N,T,2], depth [T,H,W], dino [T,Hp,Wp,D]
//                            stdout: f32 lift [N,T,3], dino rows [N,T,D], depth-feature rows [N,T,256]
//   build_row_check round    stdin: int32 n; f32 x[n]                 stdout: u16 bf16[n], u16 f16[n]
//   build_row_check slot     stdin: int32 n_tracks, count, clip_T, n_index, n_probe; int32 index[n_index]; int32 (slot, t)[n_probe]
//                            stdout: int32 (br_slot_track, br_slot_source)[n_probe]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../3dspa_code_amd/csrc/build_row.hpp"

template <typename T> static bool rd(std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, stdin) == n;
}
template <typename T> static void wr(const std::vector<T>& v) {
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), stdout);
}

static int sample() {
  std::vector<int32_t> hd;
  std::vector<double> intr;
  if (!rd(hd, 8) || !rd(intr, 4)) return 2;
  const int N = hd[0], T = hd[1], D = hd[2], Hp = hd[3], Wp = hd[4], H = hd[5], W = hd[6];
  std::vector<float> tr, depth, dino;
  if (!rd(tr, (size_t)N * T * 2) || !rd(depth, (size_t)T * H * W) || !rd(dino, (size_t)T * Hp * Wp * D)) return 2;
  const BrIntr k = br_intrinsics(hd[7] ? intr.data() : nullptr, H, W);
  const float sw = br_map_scale(Wp, W), sh = br_map_scale(Hp, H);
  std::vector<float> lift((size_t)N * T * 3), drow((size_t)N * T * D), frow((size_t)N * T * 256);
  for (int n = 0; n < N; ++n)
    for (int t = 0; t < T; ++t) {
      const size_t p = (size_t)n * T + t;
      const float x = tr[p * 2], y = tr[p * 2 + 1];
      const float d = br_depth_at(depth.data() + (size_t)t * H * W, H, W, x, y);
      br_lift(x, y, d, k, &lift[p * 3]);
      const BrCorner c = br_corners(x * sw, y * sh, Wp, Hp);
      const float* base = dino.data() + (size_t)t * Hp * Wp * D;
      const float* r00 = base + ((size_t)c.y0 * Wp + c.x0) * D; const float* r01 = base + ((size_t)c.y0 * Wp + c.x1) * D;
      const float* r10 = base + ((size_t)c.y1 * Wp + c.x0) * D; const float* r11 = base + ((size_t)c.y1 * Wp + c.x1) * D;
      for (int ch = 0; ch < D; ++ch) drow[p * D + ch] = br_blend(r00[ch], r01[ch], r10[ch], r11[ch], c.wx, c.wy);
      float dp = 0.f;
      if (t > 0) dp = br_depth_at(depth.data() + (size_t)(t - 1) * H * W, H, W, tr[(p - 1) * 2], tr[(p - 1) * 2 + 1]);
      for (int ch = 0; ch < 256; ++ch) frow[p * 256 + ch] = br_depth_feature(ch, d, dp, t);
    }
  wr(lift); wr(drow); wr(frow);
  return 0;
}

static int round_() {
  std::vector<int32_t> hd;
  std::vector<float> x;
  if (!rd(hd, 1) || !rd(x, (size_t)hd[0])) return 2;
  std::vector<uint16_t> a(x.size()), b(x.size()), c(x.size()), d(x.size());
  for (size_t i = 0; i < x.size(); ++i) { a[i] = br_round_bf16(x[i]); b[i] = br_round_f16(x[i]); }
  // the store helpers round the same way
  for (size_t i = 0; i < x.size(); ++i) { br_store<BR_BF16>(c.data(), (int64_t)i, x[i]); br_store<BR_F16>(d.data(), (int64_t)i, x[i]); }
  if (a != c || b != d) return 3;
  for (size_t i = 0; i + 1 < x.size(); i += 2)
    if (br_pack2<BR_BF16>(x[i], x[i + 1]) != ((uint32_t)a[i] | ((uint32_t)a[i + 1] << 16)) || br_pack2<BR_F16>(x[i], x[i + 1]) != ((uint32_t)b[i] | ((uint32_t)b[i + 1] << 16))) return 3;
  wr(a); wr(b);
  return 0;
}

static int slot() {
  std::vector<int32_t> hd, index, probe;
  if (!rd(hd, 5) || !rd(index, (size_t)hd[3]) || !rd(probe, (size_t)hd[4] * 2)) return 2;
  std::vector<int32_t> out((size_t)hd[4] * 2);
  for (int i = 0; i < hd[4]; ++i) {
    out[(size_t)i * 2] = br_slot_track(index.data(), probe[(size_t)i * 2], hd[1], hd[0]);
    out[(size_t)i * 2 + 1] = br_slot_source(index.data(), probe[(size_t)i * 2], hd[1], hd[0], probe[(size_t)i * 2 + 1], hd[2]);
  }
  wr(out);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 1;
  if (!strcmp(argv[1], "sample")) return sample();
  if (!strcmp(argv[1], "round")) return round_();
  if (!strcmp(argv[1], "slot")) return slot();
  return 1;
}
