// score_row.hpp -- per-track reconstruction scores of one query row (spa3d_score / spa3d_score_from_preds, include/spa3d.h).
// Plain C++, host- and device-callable: the fused kernel (head buffer), the from-predictions kernel (split tensors) and the g++ host test
// (tests/host/score_row_check.cpp) all run THIS code, frame by frame, in the same order.
//
// One row = one query track of T frames: predictions p[t][c], visibility logit l[t], targets g[t][c], target visibility y[t] in {0, 1},
// NC = 3 coordinates (2 for the 2-D model), K <= 8 distance thresholds tau_k, each multiplied by the row's sample scale.  Per frame, fp32:
//   e1  = sum_c |p - g|            the training loss's L1, summed in the order of head_loss_fwd_kernel (loss.hip)
//   e2  = sqrtf(sum_c (p - g)^2)   Euclidean distance
//   pv  = l > 0, vis = y > 0.5
//   bce = -y log_sigmoid(l) - (1 - y) log_sigmoid(-l), the expression of head_loss_fwd_kernel
// Stats row of S = 8 + 4K floats:
//   0 n_vis = sum vis | 1 sum y e1 | 2 sum y e2 | 3 max of e2 over vis frames (0 if none) | 4 sum bce | 5 sum [pv == vis] | 6 sum pv | 7 T
//   8 + 4k  W_k  = sum [vis and e2 < tau_k s]           9 + 4k  TP_k = sum [vis and pv and e2 < tau_k s]
//   10 + 4k FP_k = sum [pv and not (vis and e2 < tau_k s)]   11 + 4k FN_k = sum [vis and not (pv and e2 < tau_k s)]
// so TP_k + FN_k = n_vis and TP_k + FP_k = slot 6 on every row.  These are the TAP-Vid Jaccard counts with FIXED metric thresholds.
// This is NOT tapnet's TAPVid-3D metric: there is no depth-dependent threshold and no median rescaling of the predictions; a caller who
// wants scene-relative thresholds passes them through the per-sample scale.
//
// Order of summation: lane j of 64 takes frames j, j + 64, ... in increasing order, then the 64 partial rows are merged by the xor
// butterfly (distance 32, 16, ..., 1).  The kernel does that with wave shuffles, score_row_host below with a loop: the same additions.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SCORE_HD __host__ __device__ __forceinline__
#define SCORE_UNROLL _Pragma("unroll")  // the per-threshold arrays stay in registers
#else
#define SCORE_HD inline
#define SCORE_UNROLL
#endif

constexpr int SCORE_MAX_K = 8;
constexpr int SCORE_BASE = 8;  // slots before the per-threshold counts
SCORE_HD int score_row_len(int K) { return SCORE_BASE + 4 * K; }

struct ScoreThr { int K; float t[SCORE_MAX_K]; };  // travels by value in the kernel arguments

struct ScoreAcc {  // one lane's partial row (counts are exact in fp32: T < 2^24)
  float n_vis, s_e1, s_e2, mx, bce, occ, n_pv;
  float w[SCORE_MAX_K], tp[SCORE_MAX_K], fp[SCORE_MAX_K], fn[SCORE_MAX_K];
};

SCORE_HD float score_log_sigmoid(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }

SCORE_HD void score_acc_init(ScoreAcc& a) {
  a.n_vis = a.s_e1 = a.s_e2 = a.mx = a.bce = a.occ = a.n_pv = 0.f;
  for (int k = 0; k < SCORE_MAX_K; ++k) a.w[k] = a.tp[k] = a.fp[k] = a.fn[k] = 0.f;
}

// adds one frame; p / g: the frame's NC coordinates (stride sp / sg between coordinates); thr: tau_k * scale; returns e2
SCORE_HD float score_acc_frame(ScoreAcc& a, const float* p, long sp, const float* g, long sg, int NC, float l, float y, const ScoreThr& thr) {
  float e1 = 0.f, sq = 0.f;
  for (int c = 0; c < NC; ++c) {
    const float d = p[c * sp] - g[c * sg];
    e1 += fabsf(d);
    sq += d * d;
  }
  const float e2 = sqrtf(sq);
  const bool pv = l > 0.f, vis = y > 0.5f;
  a.n_vis += vis ? 1.f : 0.f;
  a.s_e1 += e1 * y;
  a.s_e2 += e2 * y;
  if (vis && e2 > a.mx) a.mx = e2;
  a.bce += -y * score_log_sigmoid(l) - (1.f - y) * score_log_sigmoid(-l);
  a.occ += pv == vis ? 1.f : 0.f;
  a.n_pv += pv ? 1.f : 0.f;
  SCORE_UNROLL
  for (int k = 0; k < SCORE_MAX_K; ++k) {
    if (k < thr.K) {
      const bool within = vis && e2 < thr.t[k];
      a.w[k] += within ? 1.f : 0.f;
      a.tp[k] += (within && pv) ? 1.f : 0.f;
      a.fp[k] += (pv && !within) ? 1.f : 0.f;
      a.fn[k] += (vis && !(pv && within)) ? 1.f : 0.f;
    }
  }
  return e2;
}

// a <- a merged with b (sums add, slot 3 is a max); commutative, so both partners of a butterfly step get the same bits
SCORE_HD void score_acc_merge(ScoreAcc& a, const ScoreAcc& b, int K) {
  a.n_vis += b.n_vis; a.s_e1 += b.s_e1; a.s_e2 += b.s_e2; a.mx = a.mx > b.mx ? a.mx : b.mx; a.bce += b.bce; a.occ += b.occ; a.n_pv += b.n_pv;
  SCORE_UNROLL
  for (int k = 0; k < SCORE_MAX_K; ++k)
    if (k < K) { a.w[k] += b.w[k]; a.tp[k] += b.tp[k]; a.fp[k] += b.fp[k]; a.fn[k] += b.fn[k]; }
}

// slot `s` of the finished row
SCORE_HD float score_acc_slot(const ScoreAcc& a, int s, int T) {
  float v = 0.f;
  if (s == 0) v = a.n_vis; else if (s == 1) v = a.s_e1; else if (s == 2) v = a.s_e2; else if (s == 3) v = a.mx;
  else if (s == 4) v = a.bce; else if (s == 5) v = a.occ; else if (s == 6) v = a.n_pv; else if (s == 7) v = (float)T;
  SCORE_UNROLL
  for (int k = 0; k < SCORE_MAX_K; ++k) {
    if (s == SCORE_BASE + 4 * k) v = a.w[k];
    if (s == SCORE_BASE + 4 * k + 1) v = a.tp[k];
    if (s == SCORE_BASE + 4 * k + 2) v = a.fp[k];
    if (s == SCORE_BASE + 4 * k + 3) v = a.fn[k];
  }
  return v;
}

// tau_k * scale, rounded once to fp32: what every comparison of the row uses
SCORE_HD ScoreThr score_thr_scaled(const ScoreThr& thr, float scale) {
  ScoreThr r = thr;
  for (int k = 0; k < SCORE_MAX_K; ++k) r.t[k] = k < thr.K ? thr.t[k] * scale : 0.f;
  return r;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole row on the host, in the kernel's order (64 lanes, then the butterfly).  p [T][NC], l [T], g [T][NC], y [T];
// stats [8 + 4K]; frame_err [T] or null.
inline void score_row_host(const float* p, const float* l, const float* g, const float* y, int T, int NC, const ScoreThr& thr, float scale,
                           float* stats, float* frame_err) {
  const ScoreThr ts = score_thr_scaled(thr, scale);
  ScoreAcc lane[64];
  for (int j = 0; j < 64; ++j) {
    score_acc_init(lane[j]);
    for (int t = j; t < T; t += 64) {
      const float e2 = score_acc_frame(lane[j], p + (long)t * NC, 1, g + (long)t * NC, 1, NC, l[t], y[t], ts);
      if (frame_err) frame_err[t] = e2;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    ScoreAcc next[64];
    for (int j = 0; j < 64; ++j) { next[j] = lane[j]; score_acc_merge(next[j], lane[j ^ o], ts.K); }
    for (int j = 0; j < 64; ++j) lane[j] = next[j];
  }
  for (int s = 0; s < score_row_len(ts.K); ++s) stats[s] = score_acc_slot(lane[0], s, T);
}
#endif
