// tapvid3d_row.hpp -- the TAPVid-3D metric counts of one query row and the exact median select (spa3d_tapvid3d_from_preds, include/spa3d.h).
// Plain C++, host- and device-callable: the kernels of tapvid3d.hip and the g++ host test (tests/host/tapvid3d_row_check.cpp) run THIS code,
// frame by frame and digit by digit, in the same order.
//
// The definitions are restated from the published definition of the TAPVid-3D metrics (compute_tapvid3d_metrics of the tapnet package, which
// upstream does not vendor), parity unpinned: there is no tapnet on the machines this was written on, so include/spa3d.h is the contract.
//
// One row = one query track of T frames: predictions p[t][3], visibility logit l[t], targets g[t][3], target visibility y[t], the row's query
// frame tq.  fp32 throughout:
//   ew    = t != tq                                     the query frame is left out of every count
//   gn    = sqrtf(fmaxf(1e-12f, sum_c g^2)), pn alike;  ratio = gn / pn
//   ps    = p * s, rounded once per coordinate          s: 1, the sample's median of ratio over {vis and ew}, or the row's ratio at tq
//   e2    = sqrtf(sum_c (ps - g)^2)
//   thr_k = px_k * (g_z / f), f = sqrtf(fx fy + 1e-12f), px = 1, 2, 4, 8, 16    or the fixed metric table 0.01, 0.04, 0.16, 0.64, 2.56
//   within_k = e2 < thr_k (a non-positive threshold matches nothing), pv = l > 0, vis = y > 0.5
// Row of TV_S = 24 floats:
//   0 sum ew | 1 sum ew vis | 2 sum ew [pv == vis] | 3 sum ew pv
//   4 + 4k W = sum ew vis within | 5 + 4k TP = sum ew vis pv within | 6 + 4k FP = sum ew pv not (vis within) | 7 + 4k FN = sum ew vis not (pv within)
// so TP + FN = slot 1 and TP + FP = slot 3 on every row.  Counts are exact in fp32 (T < 2^24).
//
// Order of summation: as score_row.hpp -- lane j of 64 takes frames j, j + 64, ..., then the xor butterfly (32, 16, ..., 1).
//
// Median: non-NaN fp32 values >= 0 order as their bit patterns, so the k-th smallest is found by a most-significant-digit radix select over the
// 32-bit patterns, 8 bits a pass: histogram of the digit over the entries that carry the prefix found so far, walk the histogram to the digit
// that holds the rank, narrow.  Both middle ranks (m - 1) / 2 and m / 2 are carried through the same four passes; they share one histogram
// while their prefixes agree and split when a digit boundary falls between them, so duplicates across the middle need no special case: a
// rank is resolved through the counts alone.  NaN entries are not part of the set.  Integer counts only: the same input gives the same bits.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TV_HD __host__ __device__ __forceinline__
#define TV_UNROLL _Pragma("unroll")
#else
#define TV_HD inline
#define TV_UNROLL
#endif

constexpr int TV_K = 5;   // pixel thresholds 1, 2, 4, 8, 16
constexpr int TV_S = 24;  // 4 + 4 * TV_K
enum { TV_SCALE_NONE = 0, TV_SCALE_MEDIAN = 1, TV_SCALE_PER_TRAJECTORY = 2 };

TV_HD float tv_px(int k) { return k == 0 ? 1.f : k == 1 ? 2.f : k == 2 ? 4.f : k == 3 ? 8.f : 16.f; }
TV_HD float tv_fixed_thr(int k) { return k == 0 ? 0.01f : k == 1 ? 0.04f : k == 2 ? 0.16f : k == 3 ? 0.64f : 2.56f; }

// the row's query frame: clamp(lrintf(t), 0, T - 1); written so that a non-finite t never reaches lrintf
TV_HD int tv_query_frame(float t, int T) {
  if (!(t > 0.f)) return 0;
  if (t >= (float)(T - 1)) return T - 1;
  return (int)lrintf(t);
}
TV_HD float tv_focal(float fx, float fy) { return sqrtf(fx * fy + 1e-12f); }
TV_HD float tv_norm(const float* v) { return sqrtf(fmaxf(1e-12f, v[0] * v[0] + v[1] * v[1] + v[2] * v[2])); }
TV_HD float tv_ratio(const float* p, const float* g) { return tv_norm(g) / tv_norm(p); }

TV_HD uint32_t tv_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
TV_HD float tv_float(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }
TV_HD bool tv_is_nan_bits(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u; }
TV_HD float tv_nan() { return tv_float(0x7fc00000u); }

struct TvAcc {  // one lane's partial row
  float n_ew, n_vis, occ, n_pv;
  float w[TV_K], tp[TV_K], fp[TV_K], fn[TV_K];
};
TV_HD void tv_acc_init(TvAcc& a) {
  a.n_ew = a.n_vis = a.occ = a.n_pv = 0.f;
  for (int k = 0; k < TV_K; ++k) a.w[k] = a.tp[k] = a.fp[k] = a.fn[k] = 0.f;
}
// adds frame t of a row: p, g the frame's three coordinates; s the scale of the predictions; f the sample's focal length (tv_focal)
TV_HD void tv_acc_frame(TvAcc& a, const float* p, const float* g, float l, float y, float s, bool ew, float f, bool fixed) {
  if (!ew) return;
  float sq = 0.f;
  for (int c = 0; c < 3; ++c) {
    const float ps = p[c] * s;
    const float d = ps - g[c];
    sq += d * d;
  }
  const float e2 = sqrtf(sq);
  const bool pv = l > 0.f, vis = y > 0.5f;
  const float depth = g[2] / f;
  a.n_ew += 1.f;
  a.n_vis += vis ? 1.f : 0.f;
  a.occ += pv == vis ? 1.f : 0.f;
  a.n_pv += pv ? 1.f : 0.f;
  TV_UNROLL
  for (int k = 0; k < TV_K; ++k) {
    const float thr = fixed ? tv_fixed_thr(k) : tv_px(k) * depth;
    const bool within = vis && e2 < thr;
    a.w[k] += within ? 1.f : 0.f;
    a.tp[k] += (within && pv) ? 1.f : 0.f;
    a.fp[k] += (pv && !within) ? 1.f : 0.f;
    a.fn[k] += (vis && !(pv && within)) ? 1.f : 0.f;
  }
}
TV_HD void tv_acc_merge(TvAcc& a, const TvAcc& b) {
  a.n_ew += b.n_ew; a.n_vis += b.n_vis; a.occ += b.occ; a.n_pv += b.n_pv;
  TV_UNROLL
  for (int k = 0; k < TV_K; ++k) { a.w[k] += b.w[k]; a.tp[k] += b.tp[k]; a.fp[k] += b.fp[k]; a.fn[k] += b.fn[k]; }
}
TV_HD float tv_acc_slot(const TvAcc& a, int s) {
  float v = 0.f;
  if (s == 0) v = a.n_ew; else if (s == 1) v = a.n_vis; else if (s == 2) v = a.occ; else if (s == 3) v = a.n_pv;
  TV_UNROLL
  for (int k = 0; k < TV_K; ++k) {
    if (s == 4 + 4 * k) v = a.w[k];
    if (s == 5 + 4 * k) v = a.tp[k];
    if (s == 6 + 4 * k) v = a.fp[k];
    if (s == 7 + 4 * k) v = a.fn[k];
  }
  return v;
}

// ---- exact median select -------------------------------------------------------------------------------------------------------------
struct TvSelect {
  uint32_t prefix[2];  // the bits found so far of the two middle values (lower / upper)
  uint32_t rank[2];    // their ranks among the entries that carry the prefix
  uint32_t count;      // non-NaN entries of the set (known after pass 0)
};
TV_HD void tv_select_init(TvSelect& s) { s.prefix[0] = s.prefix[1] = 0u; s.rank[0] = s.rank[1] = 0u; s.count = 0u; }
TV_HD int tv_select_shift(int pass) { return 24 - 8 * pass; }
// does an entry take part in the histogram of middle value i in this pass?  (pass 0: every entry)
TV_HD bool tv_select_match(const TvSelect& s, int i, int pass, uint32_t bits) {
  return pass == 0 || (bits >> (tv_select_shift(pass) + 8)) == (s.prefix[i] >> (tv_select_shift(pass) + 8));
}
TV_HD uint32_t tv_select_digit(int pass, uint32_t bits) { return (bits >> tv_select_shift(pass)) & 255u; }
// whether the two middle values still share one histogram (call BEFORE tv_select_step of the pass)
TV_HD bool tv_select_shared(const TvSelect& s) { return s.prefix[0] == s.prefix[1]; }
// the digit walk of one pass: h0 / h1 are the 256-bin histograms of the entries matching prefix[0] / prefix[1] (h1 is not read while shared)
TV_HD void tv_select_step(TvSelect& s, const uint32_t* h0, const uint32_t* h1, int pass) {
  const bool shared = tv_select_shared(s);
  if (pass == 0) {
    uint32_t m = 0;
    for (int d = 0; d < 256; ++d) m += h0[d];
    s.count = m;
    if (m == 0) return;
    s.rank[0] = (m - 1) / 2; s.rank[1] = m / 2;
  }
  if (s.count == 0) return;
  for (int i = 0; i < 2; ++i) {
    const uint32_t* h = (i == 1 && !shared) ? h1 : h0;
    uint32_t below = 0; int d = 0;
    for (; d < 255; ++d) {  // the rank lies inside the matching entries, so the walk ends at the latest in bin 255
      if (s.rank[i] < below + h[d]) break;
      below += h[d];
    }
    s.rank[i] -= below;
    s.prefix[i] |= (uint32_t)d << tv_select_shift(pass);
  }
}
// after the four passes: the median (1 for an empty set)
TV_HD float tv_select_result(const TvSelect& s) {
  if (s.count == 0) return 1.f;
  const float a = tv_float(s.prefix[0]), b = tv_float(s.prefix[1]);
  return (s.count & 1u) ? a : 0.5f * a + 0.5f * b;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// the select on the host, pass by pass as the kernel does it
inline float tv_median_host(const float* x, int64_t n) {
  TvSelect s;
  tv_select_init(s);
  for (int pass = 0; pass < 4; ++pass) {
    uint32_t h[2][256];
    memset(h, 0, sizeof h);
    const bool shared = tv_select_shared(s);
    for (int64_t i = 0; i < n; ++i) {
      const uint32_t u = tv_bits(x[i]);
      if (tv_is_nan_bits(u)) continue;
      if (tv_select_match(s, 0, pass, u)) ++h[0][tv_select_digit(pass, u)];
      if (!shared && tv_select_match(s, 1, pass, u)) ++h[1][tv_select_digit(pass, u)];
    }
    tv_select_step(s, h[0], h[1], pass);
  }
  return tv_select_result(s);
}
// One row on the host in the kernel's order.  p, g [T][3]; l, y [T]; qt the row's query time (query_points[.., 0]); s the scale the row is
// scored with for `none` / `median`, ignored for per_trajectory (the row's own ratio at tq); stats [TV_S]; ratio [T] or null; returns the scale used
inline float tv_row_host(const float* p, const float* l, const float* g, const float* y, int T, float qt, int scaling, float s, float fx, float fy,
                         bool fixed, float* stats, float* ratio) {
  const int tq = tv_query_frame(qt, T);
  const float f = tv_focal(fx, fy);
  if (scaling == TV_SCALE_PER_TRAJECTORY) s = tv_ratio(p + 3 * tq, g + 3 * tq);
  TvAcc lane[64];
  for (int j = 0; j < 64; ++j) {
    tv_acc_init(lane[j]);
    for (int t = j; t < T; t += 64) {
      if (ratio) ratio[t] = tv_ratio(p + 3 * t, g + 3 * t);
      tv_acc_frame(lane[j], p + 3 * t, g + 3 * t, l[t], y[t], s, t != tq, f, fixed);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    TvAcc next[64];
    for (int j = 0; j < 64; ++j) { next[j] = lane[j]; tv_acc_merge(next[j], lane[j ^ o]); }
    for (int j = 0; j < 64; ++j) lane[j] = next[j];
  }
  for (int k = 0; k < TV_S; ++k) stats[k] = tv_acc_slot(lane[0], k);
  return s;
}
#endif
