// Host driver of 3dspa_code_amd/csrc/heatmap_px.hpp (tests/test_heatmap_px_host.py): the header is plain C++, so the eligibility, the weights,
// the two sums, the division and the overlay that the GPU kernels run are compiled here with the host compiler and compute whole small clips
// on the CPU.
// Input (stdin, little-endian): int32 hdr[15] = N, T, H, W, coords, resize_h, resize_w, use_visibility, radius, power, have_visible,
//   have_video, normalize, alpha, colour_bgr; float32 lo, hi; float32 tracks[N*T*coords]; coords == 3: float64 K[T*9], E[T*16];
//   float32 values[N*T]; have_visible: float32 visible[N*T]; have_video: uint8 video[T*H*W*3].
// Output: float32 map[T*H*W], float32 weight[T*H*W], float64 num[T*H*W], uint64 den[T*H*W]; have_video: uint8 overlay[T*H*W*3].
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../3dspa_code_amd/csrc/heatmap_px.hpp"

template <typename V> static bool rd(V* p, size_t n) { return n == 0 || fread(p, sizeof(V), n, stdin) == n; }
template <typename V> static bool wr(const V* p, size_t n) { return n == 0 || fwrite(p, sizeof(V), n, stdout) == n; }

int main() {
  int32_t h[15];
  float range[2];
  if (!rd(h, 15) || !rd(range, 2)) return 2;
  HmScene s{};
  s.c = HmClip{h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9]};
  const HmClip& c = s.c;
  if (c.N < 1 || c.T < 1 || c.H < 1 || c.H > RP_MAX_DIM || c.W < 1 || c.W > RP_MAX_DIM || (c.coords != 2 && c.coords != 3) || c.radius < 1 ||
      c.radius > HM_MAX_RADIUS || (c.power != 1 && c.power != 2) || h[13] < 0 || h[13] > HM_MAX_ALPHA)
    return 3;
  const size_t n = (size_t)c.N * c.T, px = (size_t)c.T * c.H * c.W;
  std::vector<float> tracks(n * c.coords), values(n), visible(h[10] ? n : 0);
  std::vector<double> K(c.coords == 3 ? (size_t)c.T * 9 : 0), E(c.coords == 3 ? (size_t)c.T * 16 : 0);
  std::vector<uint8_t> video(h[11] ? px * 3 : 0);
  if (!rd(tracks.data(), tracks.size()) || !rd(K.data(), K.size()) || !rd(E.data(), E.size()) || !rd(values.data(), n) || !rd(visible.data(), visible.size()) ||
      !rd(video.data(), video.size()))
    return 4;
  s.tracks = tracks.data(); s.values = values.data(); s.visible = h[10] ? visible.data() : nullptr;
  s.K = c.coords == 3 ? K.data() : nullptr; s.E = c.coords == 3 ? E.data() : nullptr;
  std::vector<int32_t> pts(n);
  float lo, hi;
  hm_prepare_host(s, pts.data(), lo, hi);
  if (!h[12]) { lo = range[0]; hi = range[1]; }
  std::vector<float> map(px), weight(px);
  std::vector<double> num(px);
  std::vector<uint64_t> den(px);
  size_t o = 0;
  for (int t = 0; t < c.T; ++t)
    for (int Y = 0; Y < c.H; ++Y)
      for (int X = 0; X < c.W; ++X, ++o) {
        hm_pixel_host(s, pts.data(), t, X, Y, num[o], den[o]);
        map[o] = hm_value(num[o], den[o]);
        weight[o] = hm_weight_out(den[o]);
        if (h[11]) {
          int ch[3] = {video[3 * o], video[3 * o + 1], video[3 * o + 2]};
          hm_overlay(map[o], den[o], lo, hi, h[14] != 0, h[13], ch);
          for (int k = 0; k < 3; ++k) video[3 * o + k] = (uint8_t)ch[k];
        }
      }
  if (!wr(map.data(), px) || !wr(weight.data(), px) || !wr(num.data(), px) || !wr(den.data(), px) || !wr(video.data(), video.size())) return 5;
  return 0;
}
