// heatmap_px.hpp -- the arithmetic of spa3d_render_heatmap (include/spa3d.h states the contract): which point-frames contribute, the weight of a
// point for a pixel, the two sums, the map value and the overlay of one pixel.  Positions, colour, blend and the min / max are render_px.hpp's.
// Plain C++, host- and device-callable: the kernels of heatmap.hip and the g++ host test (tests/host/heatmap_px_check.cpp) run THIS code, and
// nothing else defines any of it.  Integers for the weights and their sum, double for the weighted sum, the division and the scaling; no fp32
// division.
#pragma once
#include "render_px.hpp"

constexpr int HM_MAX_RADIUS = 64, HM_MAX_ALPHA = 4096;
constexpr int32_t HM_NO_POINT = -1;  // a packed position (hm_pack) of a point-frame that does not contribute

struct HmClip { int32_t N, T, H, W, coords, resize_h, resize_w, use_visibility, radius, power; };

// One point-frame: trk = its coordinates, K / E = its frame's matrices (coords == 3), v = its value, vis = its visibility (have_vis false: absent).
// True when it contributes; pos is then its pixel, in bounds.
RP_HD bool hm_point_frame(const HmClip& c, const float* trk, const double* K, const double* E, float v, bool have_vis, float vis, int32_t pos[2]) {
  if (c.coords == 3) rp_project(trk, K, E, c.H, c.W, c.resize_h, c.resize_w, pos);
  else rp_pixel_2d(trk, pos);
  const bool seen = !c.use_visibility || (have_vis && vis > 0.5f);
  return seen && rp_finite(v) && pos[0] != RP_NO_POS && rp_in_bounds(pos, c.H, c.W);
}
// an in-bounds position in one word (x, y < 16384)
RP_HD int32_t hm_pack(const int32_t pos[2]) { return pos[0] | pos[1] << 16; }
RP_HD void hm_unpack(int32_t p, int& x, int& y) { x = p & 0xffff; y = p >> 16; }

// the weight of a point at offset (dx, dy) from the pixel; 0: out of reach.  |dx|, |dy| < 2^15, R2 = radius^2 <= 4096: w < 2^25
RP_HD uint32_t hm_weight(int dx, int dy, int R2, int power) {
  const int d2 = dx * dx + dy * dy;
  if (d2 > R2) return 0u;
  const uint32_t q = (uint32_t)(R2 + 1 - d2);
  return power == 2 ? q * q : q;
}
// one contributing point into a pixel's sums: the product is exact (25 + 24 bits), the addition rounds once
RP_HD void hm_add(double& num, uint64_t& den, uint32_t w, float v) {
  den += w;
  num += (double)w * (double)v;
}
RP_HD float hm_value(double num, uint64_t den) { return den ? (float)(num / (double)den) : NAN; }
RP_HD float hm_weight_out(uint64_t den) { return (float)den; }

// overlay: the scaled value of a map value, and one pixel's three bytes
RP_HD float hm_scale(float m, float lo, float hi) {
  const double dm = m, dl = lo, dh = hi;
  return (float)(dh > dl ? (dm - dl) / (dh - dl) : dm - dl);
}
RP_HD void hm_overlay(float m, uint64_t den, float lo, float hi, bool bgr, int alpha, int ch[3]) {
  if (!den) return;
  const float s1 = hm_scale(m, lo, hi);
  if (!rp_finite(s1)) return;
  const uint32_t col = rp_colour(s1, bgr);
  for (int c = 0; c < 3; ++c) ch[c] = rp_blend(ch[c], (int)(col >> (8 * c) & 255u), alpha);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole call on the host, in the kernels' steps.  Arrays as in spa3d_heatmap (host memory); pts [T][N] packed positions.
struct HmScene { HmClip c; const float* tracks; const double* K; const double* E; const float* values; const float* visible; };
inline void hm_prepare_host(const HmScene& s, int32_t* pts, float& mn, float& mx) {
  const HmClip& c = s.c;
  rp_minmax_init(mn, mx);
  for (int64_t j = 0; j < (int64_t)c.N * c.T; ++j) rp_minmax_add(mn, mx, s.values[j]);
  for (int i = 0; i < c.N; ++i)
    for (int t = 0; t < c.T; ++t) {
      const int64_t j = (int64_t)i * c.T + t;
      int32_t pos[2];
      const bool ok = hm_point_frame(c, s.tracks + j * c.coords, s.K ? s.K + (int64_t)t * 9 : nullptr, s.E ? s.E + (int64_t)t * 16 : nullptr, s.values[j],
                                     s.visible != nullptr, s.visible ? s.visible[j] : 0.f, pos);
      pts[(int64_t)t * c.N + i] = ok ? hm_pack(pos) : HM_NO_POINT;
    }
}
// the sums of pixel (X, Y) of frame t
inline void hm_pixel_host(const HmScene& s, const int32_t* pts, int t, int X, int Y, double& num, uint64_t& den) {
  const HmClip& c = s.c;
  num = 0.0; den = 0;
  for (int i = 0; i < c.N; ++i) {
    const int32_t p = pts[(int64_t)t * c.N + i];
    if (p == HM_NO_POINT) continue;
    int x, y;
    hm_unpack(p, x, y);
    const uint32_t w = hm_weight(X - x, Y - y, c.radius * c.radius, c.power);
    if (w) hm_add(num, den, w, s.values[(int64_t)i * c.T + t]);
  }
}
#endif
