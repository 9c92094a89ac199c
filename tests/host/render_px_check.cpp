// Host driver of 3dspa_code_amd/csrc/render_px.hpp (tests/test_render_px_host.py): the header is plain C++, so the projection, the colour map,
// the coverage tests, the blend and the compositing that the GPU kernels run are compiled here with the host compiler and rasterise whole
// small scenes on the CPU.
// Input (stdin, little-endian): int32 hdr[14] = N, T, H, W, coords, resize_h, resize_w, normalize, use_visibility, colour_bgr, trail,
//   point_size, have_visible, windows; float32 tracks[N*T*coords]; coords == 3: float64 K[T*9], E[T*16]; float32 scores[N*T];
//   have_visible: float32 visible[N*T].  windows == 0: uint8 video[T*H*W*3].  Else per window int32 t, y0, y1, x0, x1 (inclusive) and its
//   uint8 bytes [y1-y0+1][x1-x0+1][3] (a clip too large to hold is checked window by window).
// Output: int32 pixels[N*T*2], uint32 flags[N*T], then the painted video, or the painted windows in order.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../3dspa_code_amd/csrc/render_px.hpp"

template <typename V> static bool rd(V* p, size_t n) { return n == 0 || fread(p, sizeof(V), n, stdin) == n; }
template <typename V> static bool wr(const V* p, size_t n) { return n == 0 || fwrite(p, sizeof(V), n, stdout) == n; }

int main() {
  int32_t h[14];
  if (!rd(h, 14)) return 2;
  RpScene s{};
  s.c = RpClip{h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9], h[10], h[11]};
  const RpClip& c = s.c;
  if (c.N < 1 || c.T < 1 || c.H < 1 || c.H > RP_MAX_DIM || c.W < 1 || c.W > RP_MAX_DIM || (c.coords != 2 && c.coords != 3) || c.trail < 0 ||
      c.trail > RP_MAX_TRAIL || c.radius < 0 || c.radius > RP_MAX_RADIUS || h[13] < 0)
    return 3;
  const size_t n = (size_t)c.N * c.T;
  std::vector<float> tracks(n * c.coords), scores(n), visible(h[12] ? n : 0);
  std::vector<double> K(c.coords == 3 ? (size_t)c.T * 9 : 0), E(c.coords == 3 ? (size_t)c.T * 16 : 0);
  if (!rd(tracks.data(), tracks.size()) || !rd(K.data(), K.size()) || !rd(E.data(), E.size()) || !rd(scores.data(), n) || !rd(visible.data(), visible.size())) return 4;
  s.tracks = tracks.data(); s.scores = scores.data(); s.visible = h[12] ? visible.data() : nullptr;
  s.K = c.coords == 3 ? K.data() : nullptr; s.E = c.coords == 3 ? E.data() : nullptr;
  std::vector<int32_t> pos(n * 2);
  std::vector<uint32_t> fl(n);
  rp_prepare_host(s, pos.data(), fl.data());
  if (!wr(pos.data(), pos.size()) || !wr(fl.data(), fl.size())) return 5;
  auto paint = [&](std::vector<uint8_t>& px, int t, int y0, int y1, int x0, int x1) {
    size_t o = 0;
    for (int Y = y0; Y <= y1; ++Y)
      for (int X = x0; X <= x1; ++X, o += 3) {
        int ch[3] = {px[o], px[o + 1], px[o + 2]};
        rp_pixel_host(c, pos.data(), fl.data(), t, X, Y, ch);
        for (int k = 0; k < 3; ++k) px[o + k] = (uint8_t)ch[k];
      }
  };
  if (h[13] == 0) {
    std::vector<uint8_t> frame((size_t)c.H * c.W * 3);
    for (int t = 0; t < c.T; ++t) {
      if (!rd(frame.data(), frame.size())) return 6;
      paint(frame, t, 0, c.H - 1, 0, c.W - 1);
      if (!wr(frame.data(), frame.size())) return 7;
    }
    return 0;
  }
  for (int w = 0; w < h[13]; ++w) {
    int32_t q[5];
    if (!rd(q, 5) || q[0] < 0 || q[0] >= c.T || q[1] < 0 || q[2] >= c.H || q[1] > q[2] || q[3] < 0 || q[4] >= c.W || q[3] > q[4]) return 8;
    std::vector<uint8_t> px((size_t)(q[2] - q[1] + 1) * (q[4] - q[3] + 1) * 3);
    if (!rd(px.data(), px.size())) return 9;
    paint(px, q[0], q[1], q[2], q[3], q[4]);
    if (!wr(px.data(), px.size())) return 10;
  }
  return 0;
}
