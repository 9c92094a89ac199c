// render_px.hpp -- the arithmetic of spa3d_render_tracks (include/spa3d.h states the contract): the colour map, the projection of one point,
// the sample tests, the blend, the primitives of a point in a frame and their compositing into one pixel.
// Plain C++, host- and device-callable: the kernels of render.hip and the g++ host test (tests/host/render_px_check.cpp) run THIS code, and
// nothing else defines any of it.  Integer-only from the pixel positions on; double for projection and colour; fp32 for the normalisation.
//
// A point-frame (i, t) is prepared once into a position pos[2] (INT32_MIN: none) and a flag word:
//   bits 0..23  the colour's three bytes in the order they are written to a pixel (byte 0 first)
//   RP_COL_OK   the score gives a colour: point i draws in frame t
//   RP_END_OK   the position may carry a primitive: in bounds and, with use_visibility, visible
// The primitives of point i in frame t follow from the flag words and positions of frames max(0, t - trail) .. t (rp_for_each_prim).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RP_HD __host__ __device__ __forceinline__
#else
#define RP_HD inline
#endif

constexpr int RP_MAX_DIM = 16384, RP_MAX_TRAIL = 32, RP_MAX_RADIUS = 32;
constexpr int32_t RP_NO_POS = INT32_MIN;
constexpr uint32_t RP_COL_OK = 1u << 24, RP_END_OK = 1u << 25;
constexpr int RP_SEG = 0, RP_DOT = 1;
constexpr int RP_SEG_ALPHA = 179, RP_DOT_ALPHA = 256;  // of 256: 0.7 for a segment, 1 for a dot

struct RpClip { int32_t N, T, H, W, coords, resize_h, resize_w, normalize, use_visibility, colour_bgr, trail, radius; };
struct RpPrim { int32_t ax, ay, bx, by; uint32_t col; int32_t radius, kind; };  // a dot has b == a

RP_HD bool rp_finite(float v) { return fabsf(v) <= 3.402823466e38f; }  // false for NaN
RP_HD bool rp_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// ---- scores -> colour
RP_HD void rp_minmax_init(float& mn, float& mx) { mn = INFINITY; mx = -INFINITY; }
RP_HD void rp_minmax_add(float& mn, float& mx, float s) {
  if (rp_finite(s)) { mn = fminf(mn, s); mx = fmaxf(mx, s); }
}
RP_HD void rp_minmax_merge(float& mn, float& mx, float mn2, float mx2) { mn = fminf(mn, mn2); mx = fmaxf(mx, mx2); }
RP_HD float rp_normalize(float s, float mn, float mx) { return mx > mn ? (s - mn) / (mx - mn) : s - mn; }

// score_to_color_bgr (visualize.py:47-73) in double; the bytes in writing order
RP_HD uint32_t rp_colour(float s1, bool bgr) {
  const double q = fmin(fmax((double)s1, 0.0), 1.0);
  int r, g, b;
  if (q < 0.5) {
    const double ratio = q / 0.5;
    r = 255; g = (int)(255 * ratio); b = (int)(255 * ratio);
  } else {
    const double ratio = (q - 0.5) / 0.5;
    r = (int)(255 * (1 - ratio)); g = (int)(255 * (1 - ratio)); b = 255;
  }
  return bgr ? (uint32_t)b | (uint32_t)g << 8 | (uint32_t)r << 16 : (uint32_t)r | (uint32_t)g << 8 | (uint32_t)b << 16;
}

// ---- positions
// project_all_tracks + project_3d_to_2d (visualize.py:15-44,125-175) for one point of one frame; K [3][3], E [4][4] of that frame
RP_HD void rp_project(const float* p, const double* K, const double* E, int H, int W, int resize_h, int resize_w, int32_t pos[2]) {
  const double sx = (double)resize_w / (double)W, sy = (double)resize_h / (double)H;
  const double x = p[0], y = p[1], z = p[2];
  double c[3], h[3];
  for (int r = 0; r < 3; ++r) c[r] = ((E[r * 4] * x + E[r * 4 + 1] * y) + E[r * 4 + 2] * z) + E[r * 4 + 3];
  const double k[9] = {K[0] * sx, K[1], K[2] * sx, K[3], K[4] * sy, K[5] * sy, K[6], K[7], K[8]};
  for (int r = 0; r < 3; ++r) h[r] = (k[r * 3] * c[0] + k[r * 3 + 1] * c[1]) + k[r * 3 + 2] * c[2];
  double u = h[0] / (h[2] + 1e-8), v = h[1] / (h[2] + 1e-8);
  if (!rp_finite(u)) u = 0.0;
  if (!rp_finite(v)) v = 0.0;
  u = u / sx; v = v / sy;
  u = fmin(fmax(u, 0.0), (double)(W - 1)); v = fmin(fmax(v, 0.0), (double)(H - 1));
  pos[0] = (int32_t)u; pos[1] = (int32_t)v;
}
RP_HD void rp_pixel_2d(const float* p, int32_t pos[2]) {
  const bool ok = fabsf(p[0]) <= 1073741824.f && fabsf(p[1]) <= 1073741824.f;  // false for NaN and inf
  pos[0] = ok ? (int32_t)p[0] : RP_NO_POS; pos[1] = ok ? (int32_t)p[1] : RP_NO_POS;
}
RP_HD bool rp_in_bounds(const int32_t pos[2], int H, int W) { return pos[0] >= 0 && pos[0] < W && pos[1] >= 0 && pos[1] < H; }

// One point-frame: trk = its coordinates, K / E = its frame's matrices (coords == 3), s / vis = its score and visibility (have_* false: absent).
RP_HD uint32_t rp_point_frame(const RpClip& c, const float* trk, const double* K, const double* E, bool have_score, float s, float mn, float mx,
                              bool have_vis, float vis, int32_t pos[2]) {
  if (c.coords == 3) rp_project(trk, K, E, c.H, c.W, c.resize_h, c.resize_w, pos);
  else rp_pixel_2d(trk, pos);
  uint32_t fl = 0;
  if (have_score && rp_finite(s)) {
    const float s1 = c.normalize ? rp_normalize(s, mn, mx) : s;
    if (rp_finite(s1)) fl = rp_colour(s1, c.colour_bgr != 0) | RP_COL_OK;
  }
  const bool seen = !c.use_visibility || (have_vis && vis > 0.5f);
  if (seen && pos[0] != RP_NO_POS && rp_in_bounds(pos, c.H, c.W)) fl |= RP_END_OK;
  return fl;
}

// ---- coverage: units of 1/8 px, sample (a, b) of pixel (X, Y) at (8X + 2a + 1, 8Y + 2b + 1), position x at 8x + 4
RP_HD int rp_cover_dot(int X, int Y, int cx, int cy, int radius) {
  const int64_t R = 8 * (int64_t)radius + 4, R2 = R * R;
  const int64_t ox = 8 * ((int64_t)X - cx) - 3, oy = 8 * ((int64_t)Y - cy) - 3;
  int k = 0;
  for (int b = 0; b < 4; ++b)
    for (int a = 0; a < 4; ++a) {
      const int64_t px = ox + 2 * a, py = oy + 2 * b;
      k += px * px + py * py <= R2 ? 1 : 0;
    }
  return k;
}
RP_HD int rp_cover_seg(int X, int Y, int ax, int ay, int bx, int by) {
  const int64_t dx = 8 * ((int64_t)bx - ax), dy = 8 * ((int64_t)by - ay), L2 = dx * dx + dy * dy;
  const int64_t lim = 4 * ((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy));
  const int64_t ox = 8 * ((int64_t)X - ax) - 3, oy = 8 * ((int64_t)Y - ay) - 3;
  int k = 0;
  for (int b = 0; b < 4; ++b)
    for (int a = 0; a < 4; ++a) {
      const int64_t px = ox + 2 * a, py = oy + 2 * b;
      const int64_t u = px * dx + py * dy;
      bool in;
      if (L2 == 0 || u < 0) {
        in = px * px + py * py <= 16;
      } else if (u > L2) {
        const int64_t qx = px - dx, qy = py - dy;
        in = qx * qx + qy * qy <= 16;
      } else {
        const int64_t cr = px * dy - py * dx, ac = cr < 0 ? -cr : cr;
        in = ac <= lim && ac * ac <= 16 * L2;
      }
      k += in ? 1 : 0;
    }
  return k;
}

// ---- blend and compositing
RP_HD int rp_blend(int in, int col, int w) { return (in * (4096 - w) + col * w + 2048) >> 12; }

// The pixels a primitive can cover, exactly: the end points' box grown by the half-width.  A segment reaches 4 units from its axis, so samples
// within [8 min, 8 max + 8], which are those of the pixels min .. max; a dot reaches 8r + 4 from 8c + 4: the pixels c - r .. c + r.
RP_HD void rp_prim_box(const RpPrim& p, int& x0, int& y0, int& x1, int& y1) {
  const int g = p.kind == RP_DOT ? p.radius : 0;
  x0 = (p.ax < p.bx ? p.ax : p.bx) - g; x1 = (p.ax < p.bx ? p.bx : p.ax) + g;
  y0 = (p.ay < p.by ? p.ay : p.by) - g; y1 = (p.ay < p.by ? p.by : p.ay) + g;
}
// one primitive onto pixel (X, Y); ch = the pixel's three bytes
RP_HD void rp_apply(const RpPrim& p, int X, int Y, int ch[3]) {
  const int k = p.kind == RP_DOT ? rp_cover_dot(X, Y, p.ax, p.ay, p.radius) : rp_cover_seg(X, Y, p.ax, p.ay, p.bx, p.by);
  if (k == 0) return;
  const int w = k * (p.kind == RP_DOT ? RP_DOT_ALPHA : RP_SEG_ALPHA);
  for (int c = 0; c < 3; ++c) ch[c] = rp_blend(ch[c], (int)(p.col >> (8 * c) & 255u), w);
}
// an ordered list of primitives onto pixel (X, Y)
RP_HD void rp_composite(const RpPrim* prims, int n, int X, int Y, int ch[3]) {
  for (int j = 0; j < n; ++j) rp_apply(prims[j], X, Y, ch);
}

// The primitives of one point in frame t, in drawing order: pos [T][2] and fl [T] of THAT point.  f(const RpPrim&) is called for each.
template <typename F> RP_HD void rp_for_each_prim(const int32_t* pos, const uint32_t* fl, int t, int trail, int radius, F&& f) {
  const uint32_t ft = fl[t];
  if (!(ft & RP_COL_OK)) return;
  const uint32_t col = ft & 0xffffffu;
  for (int p = t - trail > 0 ? t - trail : 0; p < t; ++p)
    if (fl[p] & fl[p + 1] & RP_END_OK) f(RpPrim{pos[2 * p], pos[2 * p + 1], pos[2 * p + 2], pos[2 * p + 3], col, 0, RP_SEG});
  if (ft & RP_END_OK) f(RpPrim{pos[2 * t], pos[2 * t + 1], pos[2 * t], pos[2 * t + 1], col, radius, RP_DOT});
}
// the box of everything the point draws in frame t, cut to the image; empty: x0 > x1
RP_HD void rp_point_box(const int32_t* pos, const uint32_t* fl, int t, int trail, int radius, int H, int W, int& x0, int& y0, int& x1, int& y1) {
  int bx0 = W, by0 = H, bx1 = -1, by1 = -1;
  rp_for_each_prim(pos, fl, t, trail, radius, [&](const RpPrim& p) {
    int a0, b0, a1, b1;
    rp_prim_box(p, a0, b0, a1, b1);
    bx0 = a0 < bx0 ? a0 : bx0; by0 = b0 < by0 ? b0 : by0; bx1 = a1 > bx1 ? a1 : bx1; by1 = b1 > by1 ? b1 : by1;
  });
  x0 = bx0 < 0 ? 0 : bx0; y0 = by0 < 0 ? 0 : by0; x1 = bx1 > W - 1 ? W - 1 : bx1; y1 = by1 > H - 1 ? H - 1 : by1;
  if (x0 > x1 || y0 > y1) { x0 = 1; y0 = 1; x1 = 0; y1 = 0; }
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole call on the host, in the kernels' steps.  Arrays as in spa3d_render (host memory); pos [N][T][2], fl [N][T].
struct RpScene { RpClip c; const float* tracks; const double* K; const double* E; const float* scores; const float* visible; };
inline void rp_prepare_host(const RpScene& s, int32_t* pos, uint32_t* fl) {
  const RpClip& c = s.c;
  float mn, mx;
  rp_minmax_init(mn, mx);
  if (s.scores) for (int64_t j = 0; j < (int64_t)c.N * c.T; ++j) rp_minmax_add(mn, mx, s.scores[j]);
  for (int i = 0; i < c.N; ++i)
    for (int t = 0; t < c.T; ++t) {
      const int64_t j = (int64_t)i * c.T + t;
      fl[j] = rp_point_frame(c, s.tracks + j * c.coords, s.K ? s.K + (int64_t)t * 9 : nullptr, s.E ? s.E + (int64_t)t * 16 : nullptr, s.scores != nullptr,
                             s.scores ? s.scores[j] : 0.f, mn, mx, s.visible != nullptr, s.visible ? s.visible[j] : 0.f, pos + j * 2);
    }
}
// pixel (X, Y) of frame t: ch holds the input bytes on entry and the output bytes on return
inline void rp_pixel_host(const RpClip& c, const int32_t* pos, const uint32_t* fl, int t, int X, int Y, int ch[3]) {
  for (int i = 0; i < c.N; ++i) {
    const int64_t j = (int64_t)i * c.T;
    int x0, y0, x1, y1;
    rp_point_box(pos + j * 2, fl + j, t, c.trail, c.radius, c.H, c.W, x0, y0, x1, y1);
    if (X < x0 || X > x1 || Y < y0 || Y > y1) continue;
    rp_for_each_prim(pos + j * 2, fl + j, t, c.trail, c.radius, [&](const RpPrim& p) { rp_composite(&p, 1, X, Y, ch); });
  }
}
#endif
