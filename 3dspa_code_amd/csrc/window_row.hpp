// window_row.hpp -- the arithmetic of spa3d_stitch_windows (include/spa3d.h): a long clip cut into overlapping windows, and what one frame of
// the long time axis holds once the windows' values are merged back.  Plain C++, host- and device-callable: the kernel of windows.hip, the
// entry points' plan checks and the g++ host test (tests/host/window_row_check.cpp) run THIS code.
//
// Three things live here.
//   The plan: W windows, window w covers frames [t0[w], t0[w] + len[w]) of the TL-frame clip, starts strictly increasing, no frame uncovered.
//   The weight of window-relative frame j of a window with L live frames: 1 (mean), min(j + 1, L - j) (hat); "first" takes no weights.
//   The blend of one output element, in float32, plain operators (compiled with -ffp-contract=off, IEEE division): the contributions are taken
//     in increasing w; the first one starts num = float(wgt) * v and den = float(wgt), every later one adds to them, and the result is num / den
//     -- one division.  A frame under exactly one window, and every frame of the "first" blend, takes the lowest-numbered window's value
//     unchanged (3 * v / 3 is not v in float32, and NaN payloads and the sign of zero survive a copy).
//   spread^2 of a track point: the largest, over the contributing windows, of sum_c (p_w[c] - p_blend[c])^2 (c ascending, the first square starts
//     the sum); a NaN distance sticks; 0 under one window.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WR_HD __host__ __device__ __forceinline__
#else
#define WR_HD inline
#endif

enum { WR_BLEND_MEAN = 0, WR_BLEND_HAT = 1, WR_BLEND_FIRST = 2 };  // = SPA3D_BLEND_MEAN, SPA3D_BLEND_HAT, SPA3D_BLEND_FIRST
constexpr int WR_MAX_W = 256;                                        // starts and lengths travel by value

struct WrPlan {
  int32_t W, Tw, TL, blend;
  int32_t t0[WR_MAX_W], len[WR_MAX_W];
};

// ---- the plan ----
// live frames of a window of Tw frames that starts at t0 in a clip of TL
WR_HD int wr_window_len(int t0, int Tw, int TL) { return TL - t0 < Tw ? TL - t0 : Tw; }

// What is wrong with a plan, or WR_PLAN_OK; *where = the window it was found at.  len == NULL: every window has wr_window_len frames.
enum { WR_PLAN_OK = 0, WR_PLAN_START = 1, WR_PLAN_ORDER = 2, WR_PLAN_LEN = 3, WR_PLAN_GAP = 4 };
inline int wr_plan_check(int W, int Tw, int TL, const int32_t* t0, const int32_t* len, int* where) {
  int64_t end = 0;  // frames [0, end) are covered by the windows before w
  for (int w = 0; w < W; ++w) {
    *where = w;
    if (t0[w] < 0 || t0[w] >= TL) return WR_PLAN_START;
    if (w > 0 && t0[w] <= t0[w - 1]) return WR_PLAN_ORDER;
    const int L = len ? len[w] : wr_window_len(t0[w], Tw, TL);
    if (L < 1 || L > Tw || (int64_t)t0[w] + L > TL) return WR_PLAN_LEN;
    if (t0[w] > end) return WR_PLAN_GAP;
    if ((int64_t)t0[w] + L > end) end = (int64_t)t0[w] + L;
  }
  *where = W;
  return end == TL ? WR_PLAN_OK : WR_PLAN_GAP;
}

// The windows [wlo, whi) that can cover a frame of [tmin, tmax]: a window that starts at or before tmin - Tw ends before tmin, one that
// starts after tmax has not begun, and the starts increase.
WR_HD void wr_window_range(const WrPlan& p, int tmin, int tmax, int& wlo, int& whi) {
  int lo = 0, hi = 0;
  for (int w = 0; w < p.W; ++w) {
    if (p.t0[w] + p.Tw <= tmin) lo = w + 1;
    if (p.t0[w] <= tmax) hi = w + 1;
  }
  wlo = lo; whi = hi;
}

// ---- the weight ----
WR_HD int wr_weight(int blend, int j, int L) {
  if (blend != WR_BLEND_HAT) return 1;
  return j + 1 < L - j ? j + 1 : L - j;
}

// ---- the blend of one element ----
struct WrAcc { float num, den, first; int n; };
WR_HD void wr_acc_init(WrAcc& a) { a.num = 0.f; a.den = 0.f; a.first = 0.f; a.n = 0; }
WR_HD void wr_acc_add(WrAcc& a, int wgt, float v) {
  const float fw = (float)wgt;
  if (a.n == 0) { a.first = v; a.num = fw * v; a.den = fw; }
  else { a.num = a.num + fw * v; a.den = a.den + fw; }
  ++a.n;
}
WR_HD float wr_acc_result(const WrAcc& a, int blend) {
  if (a.n <= 1 || blend == WR_BLEND_FIRST) return a.first;
  return a.num / a.den;
}

// One frame t of one window row r: the blend of its NC (1..3) components over the windows of [wlo, whi) that cover t, and, when spread2 is
// given, the squared spread.  src is [W][N][Tw][NC]; out takes NC values.  Returns the number of contributing windows.  NC is a template
// parameter so that the accumulators stay in registers.
template <int NC> WR_HD int wr_point(const WrPlan& p, int wlo, int whi, const float* src, int64_t N, int64_t r, int t, float* out, float* spread2) {
  WrAcc acc[NC];
  for (int c = 0; c < NC; ++c) wr_acc_init(acc[c]);
  for (int w = wlo; w < whi; ++w) {
    const int j = t - p.t0[w];
    if (j < 0 || j >= p.len[w]) continue;
    const int wgt = wr_weight(p.blend, j, p.len[w]);
    const float* v = src + (((int64_t)w * N + r) * p.Tw + j) * NC;
    for (int c = 0; c < NC; ++c) wr_acc_add(acc[c], wgt, v[c]);
  }
  float res[NC];
  for (int c = 0; c < NC; ++c) out[c] = res[c] = wr_acc_result(acc[c], p.blend);
  if (spread2) {
    float m = 0.f;
    if (acc[0].n > 1) {
      for (int w = wlo; w < whi; ++w) {
        const int j = t - p.t0[w];
        if (j < 0 || j >= p.len[w]) continue;
        const float* v = src + (((int64_t)w * N + r) * p.Tw + j) * NC;
        float d2 = 0.f;
        for (int c = 0; c < NC; ++c) {
          const float d = v[c] - res[c];
          d2 = c == 0 ? d * d : d2 + d * d;
        }
        if (d2 > m || d2 != d2) m = d2;  // a NaN sticks: nothing compares greater than it afterwards
      }
    }
    *spread2 = m;
  }
  return acc[0].n;
}
