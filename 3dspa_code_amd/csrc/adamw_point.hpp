// adamw_point.hpp -- clip -> AdamW -> apply, and the weight EMA, at ONE element of the flat buffers (spa3d_adamw_step_groups, include/spa3d.h).
// Plain C++, host- and device-callable: the grouped optimizer kernels of loss.hip (16-byte body, scalar head and tail, scalar fall-back)
// and the g++ host test (tests/host/adamw_point_check.cpp) all run THIS code.  All fp32, one operation per line of the contract:
//
//   gi = g sc                                   sc = 1 below the clip norm, clip / norm above it (formed once per call)
//   m  = b1 m + (1 - b1) gi
//   v  = b2 v + (1 - b2) gi gi
//   mh = m / bc1,  vh = v / bc2                  bc = 1 - b^t at t = updates applied so far + 1 (adamw_bias_correction)
//   p  = p - lr_g (mh / (sqrt(vh) + eps) + wd_g p)
//   e  = d e + (1 - d) p                         (the EMA, after the update; 1 - d formed once per call)
//
// The expressions are those of adamw_kernel (loss.hip) in the same order, and the library is built with -ffp-contract=off: with
// lr_g = lr * 1 and wd_g = wd * 1 an element comes out bit for bit as spa3d_adamw_step leaves it.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define ADAMW_HD __host__ __device__ __forceinline__
#else
#define ADAMW_HD inline
#endif

// what every element of one call shares
struct AdamwCoef {
  float sc;        // clip factor
  float b1, b2;    // moment decays
  float bc1, bc2;  // bias corrections 1 - b1^t, 1 - b2^t
  float eps;
};

// 1 - b^t;  -expm1(t log b) keeps it accurate for b -> 1
ADAMW_HD float adamw_bias_correction(float t, float b) { return -expm1f(t * logf(b)); }

// one live element: the moments are written back through the references, the new parameter is returned
ADAMW_HD float adamw_point(const AdamwCoef& c, float lr_g, float wd_g, float p, float g, float& m, float& v) {
  const float gi = g * c.sc;
  const float mi = c.b1 * m + (1.f - c.b1) * gi;
  const float vi = c.b2 * v + (1.f - c.b2) * gi * gi;
  m = mi; v = vi;
  const float mh = mi / c.bc1, vh = vi / c.bc2;
  return p - lr_g * (mh / (sqrtf(vh) + c.eps) + wd_g * p);
}

// the weight EMA of one live element: d = decay, omd = 1 - d
ADAMW_HD float adamw_ema_point(float e, float d, float omd, float p_new) { return d * e + omd * p_new; }
