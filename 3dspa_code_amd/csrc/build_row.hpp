// build_row.hpp -- the arithmetic of spa3d_build_batch (include/spa3d.h): what one (clip, slot, frame) of a model batch holds.
// Plain C++, host- and device-callable: the kernel of batch_build.hip and the g++ host test (tests/host/build_row_check.cpp) run THIS code.
//
// Three things live here.
//   The sampler arithmetic (inference.py:287-447): the bilinear corner / weight / clamp rule, the four-term blend, the 2-D -> 3-D lift and the
//     depth-feature channel rule, in float32 and in the operation order of csrc/samplers.hip -- plain operators, compiled without contraction
//     (-ffp-contract=off) and with IEEE division, so the values are bit-identical to the reference functions run under NumPy >= 2
//     (tests/golden/sampler_golden.npz).  A coordinate that is NaN gives NaN values; a coordinate far outside the frame reads the clamped texels
//     with extrapolating weights, as the reference does.
//   The slot rule: which source track a batch slot reads, or that it is padding.
//   The single rounding of a float32 value to the batch's feature type: float32, bfloat16 or IEEE half, round to nearest even.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define BR_HD __host__ __device__ __forceinline__
#else
#define BR_HD inline
#endif

// ---- sampler arithmetic ----
struct BrCorner { int x0, y0, x1, y1; float wx, wy; };

// one axis: floor, the weight BEFORE clamping, then both texels clamped into [0, n - 1] (inference.py:305-316, :369-380, :415-425).  The floor is
// limited to [-2, n] before it becomes an integer: every value at or below -1 clamps to texels (0, 0) and every value at or above n - 1 to
// (n - 1, n - 1), so the limit changes no result and no float outside the int range is ever converted.
BR_HD void br_axis(float p, int n, int& i0, int& i1, float& w) {
  const float f = floorf(p);
  w = p - f;
  const int i = (int)fminf(fmaxf(f, -2.f), (float)n);
  const int a = i < 0 ? 0 : i, b = i + 1 < 0 ? 0 : i + 1;
  i0 = a > n - 1 ? n - 1 : a;
  i1 = b > n - 1 ? n - 1 : b;
}
BR_HD BrCorner br_corners(float px, float py, int Wm, int Hm) {
  BrCorner c;
  br_axis(px, Wm, c.x0, c.x1, c.wx);
  br_axis(py, Hm, c.y0, c.y1, c.wy);
  return c;
}
// f00 (1 - wx)(1 - wy) + f01 wx (1 - wy) + f10 (1 - wx) wy + f11 wx wy, each product left to right, the four terms added in that order
BR_HD float br_blend(float f00, float f01, float f10, float f11, float wx, float wy) {
  const float ax = 1.f - wx, ay = 1.f - wy;
  float r = (f00 * ax) * ay;
  r = r + (f01 * wx) * ay;
  r = r + (f10 * ax) * wy;
  r = r + (f11 * wx) * wy;
  return r;
}
// bilinear depth of one frame (frame = depth_map + t * H * W) at pixel (x, y)
BR_HD float br_depth_at(const float* frame, int H, int W, float x, float y) {
  const BrCorner c = br_corners(x, y, W, H);
  const float* r0 = frame + (int64_t)c.y0 * W;
  const float* r1 = frame + (int64_t)c.y1 * W;
  return br_blend(r0[c.x0], r0[c.x1], r1[c.x0], r1[c.x1], c.wx, c.wy);
}

// camera intrinsics as the lift uses them: the caller's doubles, or lift_2d_to_3d's default (inference.py:297-300), rounded once to float32
struct BrIntr { float fx, fy, cx, cy; };
inline BrIntr br_intrinsics(const double* intr, int H, int W) {
  double fx, fy, cx, cy;
  if (intr) { fx = intr[0]; fy = intr[1]; cx = intr[2]; cy = intr[3]; }
  else { fx = fy = (double)(H > W ? H : W); cx = W / 2.0; cy = H / 2.0; }
  return BrIntr{(float)fx, (float)fy, (float)cx, (float)cy};
}
// pixels of an H x W video -> texels of an Hp x Wp map: Python floats, weak against float32 (inference.py:359-360)
inline float br_map_scale(int map_size, int video_size) { return (float)((double)map_size / (double)video_size); }

// lift_2d_to_3d (inference.py:287-336): ((x - cx) z) / fx, ((y - cy) z) / fy, z
BR_HD void br_lift(float x, float y, float z, const BrIntr& k, float* out3) {
  out3[0] = ((x - k.cx) * z) / k.fx;
  out3[1] = ((y - k.cy) * z) / k.fy;
  out3[2] = z;
}
// sample_depth_features_for_tracks (inference.py:398-447): channel 0 = d, 1 = d / 10, 2 = d - d_prev for t > 0 (d_prev: the SAME track at frame
// t - 1, sampled at its own position there), every other channel 0
BR_HD float br_depth_feature(int ch, float d, float d_prev, int t) {
  if (ch == 0) return d;
  if (ch == 1) return d / 10.0f;
  if (ch == 2 && t > 0) return d - d_prev;
  return 0.f;
}

// ---- slot rule ----
// The source track of batch slot `slot` of a clip that picked `count` tracks out of a pool of `n_tracks`, or -1 for padding: a slot at or beyond
// the count, and an index outside [0, n_tracks).  index[slot] is read only for a slot below the count.
BR_HD int br_slot_track(const int32_t* index, int slot, int count, int n_tracks) {
  if (slot < 0 || slot >= count) return -1;
  const int32_t i = index[slot];
  return (i < 0 || i >= n_tracks) ? -1 : (int)i;
}
// a frame at or beyond the clip's own length is padding
BR_HD bool br_frame_live(int t, int clip_T) { return t >= 0 && t < clip_T; }
// both rules: the source track of (slot, frame t), or -1
BR_HD int br_slot_source(const int32_t* index, int slot, int count, int n_tracks, int t, int clip_T) {
  return br_frame_live(t, clip_T) ? br_slot_track(index, slot, count, n_tracks) : -1;
}

// ---- the single rounding ----
enum { BR_F32 = 0, BR_BF16 = 1, BR_F16 = 2 };  // = SPA3D_F32, SPA3D_BF16, SPA3D_F16

BR_HD uint32_t br_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
// float32 -> bfloat16, round to nearest even; NaN -> the quiet NaN 0x7fc0
BR_HD uint16_t br_round_bf16(float x) {
  const uint32_t u = br_bits(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
// float32 -> IEEE half, round to nearest even: 65520 and above become inf, magnitudes below 2^-14 become subnormals (2^-25 and below: zero),
// NaN -> the quiet NaN 0x7e00 with the sign kept
BR_HD uint16_t br_round_f16(float x) {
  const uint32_t u = br_bits(x);
  const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
  if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);
  if (a >= 0x38800000u) {  // a normal half: rebias the exponent, round at bit 13 (a carry walks into the exponent)
    uint32_t m = a - 0x38000000u;
    m += 0xfffu + ((m >> 13) & 1u);
    return (uint16_t)(sign | (m >> 13));
  }
  const uint32_t e = a >> 23;
  if (e < 102u) return (uint16_t)sign;  // below 2^-25
  const uint32_t mant = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;  // in units of 2^-24: mant >> shift, shift in 14..24
  uint32_t r = mant >> shift;
  const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
  if (rem > half || (rem == half && (r & 1u))) ++r;
  return (uint16_t)(sign | r);
}
// one value into the feature plane at element i
template <int OT> BR_HD void br_store(void* base, int64_t i, float v) {
  if (OT == BR_F32) ((float*)base)[i] = v;
  else if (OT == BR_BF16) ((uint16_t*)base)[i] = br_round_bf16(v);
  else ((uint16_t*)base)[i] = br_round_f16(v);
}
// two values as one dword of two 16-bit elements (low half = a)
template <int OT> BR_HD uint32_t br_pack2(float a, float b) {
  return OT == BR_BF16 ? ((uint32_t)br_round_bf16(a) | ((uint32_t)br_round_bf16(b) << 16)) : ((uint32_t)br_round_f16(a) | ((uint32_t)br_round_f16(b) << 16));
}
