// loss_point.hpp -- the training objective at one point (q, t) of a live query row (spa3d_loss_config, include/spa3d.h).
// Plain C++, host- and device-callable: the three loss kernels of loss.hip (head form, split form, backward) and the g++ host test
// (tests/host/loss_point_check.cpp) all run THIS code; there is no second implementation.  All fp32.
//
//   position term of one coordinate, d = prediction - target:
//     SPA3D_POS_L1     rho(d) = |d|                                        rho'(d) = sign(d), sign(0) = 0
//     SPA3D_POS_HUBER  rho(d) = d d / (2 delta) for |d| <= delta            rho'(d) = d / delta
//                               |d| - delta / 2  beyond                               sign(d)
//     (the Huber form with L1's slope in the tails, so l1_weight means the same for both)
//   visibility term, l = logit, y = target visibility, beta = bce_pos_weight (torch's pos_weight):
//     v(l)  = -beta y logsig(l) - (1 - y) logsig(-l)
//     v'(l) = beta y (sigmoid(l) - 1) + (1 - y) sigmoid(l);  with beta == 1 it is evaluated as sigmoid(l) - y, the expression the
//             loss has always used, so the default objective keeps its bits
// A multiplication by a weight that is exactly 1 (axis weight, point weight, beta) returns its other operand exactly: the default
// configuration computes what the fixed objective computed, bit for bit.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define LOSS_HD __host__ __device__ __forceinline__
#else
#define LOSS_HD inline
#endif

constexpr int LOSS_POS_L1 = 0, LOSS_POS_HUBER = 1;  // SPA3D_POS_L1 / SPA3D_POS_HUBER

LOSS_HD float loss_log_sigmoid(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }
LOSS_HD float loss_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

LOSS_HD float loss_pos_value(int kind, float delta, float d) {
  const float a = fabsf(d);
  if (kind == LOSS_POS_HUBER) return a <= delta ? d * d / (2.f * delta) : a - 0.5f * delta;
  return a;
}
LOSS_HD float loss_pos_deriv(int kind, float delta, float d) {
  if (kind == LOSS_POS_HUBER && fabsf(d) <= delta) return d / delta;
  return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
}
LOSS_HD float loss_vis_value(float beta, float y, float l) { return -(beta * y) * loss_log_sigmoid(l) - (1.f - y) * loss_log_sigmoid(-l); }
LOSS_HD float loss_vis_deriv(float beta, float y, float l) {
  const float s = loss_sigmoid(l);
  if (beta == 1.f) return s - y;
  return beta * y * (s - 1.f) + (1.f - y) * s;
}
