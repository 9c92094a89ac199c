// batch_build.hip -- the kernel of spa3d_build_batch (include/spa3d.h): clips -> the padded model batch, in one launch per BB_CLIPS clips.
// One wave per (clip, frame, slot); a clip's N support slots come first, then its Q query slots.  The arithmetic is build_row.hpp's (the
// samplers' float32 operation order, the slot rule, one rounding to the feature type), which the g++ host test runs too.
//
// Walk order: frame-major inside a clip -- all slots of frame t, then t + 1 -- so the waves in flight read ONE frame's DINO map (4.2 MB at
// 37 x 37 x 768: the size of an XCD's L2, far inside the Infinity Cache) about 4 * N / (Hp * Wp) times per texel row while it is hot.
// Track-major order (sample_dino_kernel) spreads the same reads over all T frames of the map.  This follows the gather rates of the
// microarchitecture guide by where the rows are served from; it is not a measurement of this kernel.
//
// Every output element is written exactly once, by the one wave that owns it: padding slots and padding frames as zeros, a query_points
// row by the wave of its query frame (or, for a padded slot, of frame 0).  No atomics: two runs give the same bytes.
// The feature type is a template parameter and the 16-bit roundings are explicit (build_row.hpp): compiled once.
#include "common.hpp"

#include <algorithm>

namespace SPA_NS {

template <int OT> struct BbElem { typedef uint16_t type; };
template <> struct BbElem<BR_F32> { typedef float type; };

// four consecutive elements of a feature row at element offset i (a multiple of 4; the row is 16-byte aligned in float32, 8-byte in 16 bit)
template <int OT> __device__ __forceinline__ void bb_store4(void* base, int64_t i, float v0, float v1, float v2, float v3) {
  if constexpr (OT == BR_F32) *(float4*)((float*)base + i) = make_float4(v0, v1, v2, v3);
  else { uint2 u; u.x = br_pack2<OT>(v0, v1); u.y = br_pack2<OT>(v2, v3); *(uint2*)((uint16_t*)base + i) = u; }
}
template <int OT> __device__ __forceinline__ void bb_zero_row(void* base, int64_t off, int D, bool vec, int lane) {
  typedef typename BbElem<OT>::type E;
  if (vec) {
    for (int ch = lane * 4; ch < D; ch += 256) {
      if constexpr (OT == BR_F32) *(float4*)((float*)base + off + ch) = make_float4(0.f, 0.f, 0.f, 0.f);
      else *(uint2*)((uint16_t*)base + off + ch) = make_uint2(0u, 0u);
    }
  } else {
    for (int ch = lane; ch < D; ch += 64) ((E*)base)[off + ch] = (E)0;
  }
}
// a pool row (already in the feature type) copied
template <int OT> __device__ __forceinline__ void bb_copy_row(void* base, int64_t off, const void* src, int64_t soff, int D, bool vec, int lane) {
  typedef typename BbElem<OT>::type E;
  if (vec) {
    for (int ch = lane * 4; ch < D; ch += 256) {
      if constexpr (OT == BR_F32) *(float4*)((float*)base + off + ch) = *(const float4*)((const float*)src + soff + ch);
      else *(uint2*)((uint16_t*)base + off + ch) = *(const uint2*)((const uint16_t*)src + soff + ch);
    }
  } else {
    for (int ch = lane; ch < D; ch += 64) ((E*)base)[off + ch] = ((const E*)src)[soff + ch];
  }
}

template <int OT>
__global__ __launch_bounds__(256) void build_batch_kernel(const BbArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform: the clip descriptor is then read with scalar loads
  const int64_t S = (int64_t)a.N + a.Q;                                    // slots of one frame
  const int64_t per_clip = S * a.T, total = per_clip * a.nclips;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wv; w < total; w += (int64_t)gridDim.x * 4) {
    const int g = (int)(w / per_clip);
    const int64_t r = w - (int64_t)g * per_clip;
    const int t = (int)(r / S), slot = (int)(r - (int64_t)t * S);
    const BbClip& c = a.clip[g];
    const int b = a.b0 + g;
    const bool sup = slot < a.N;
    const int s = sup ? slot : slot - a.N;
    const int src = sup ? br_slot_track(c.sidx, s, c.n_support, c.n_tracks) : br_slot_track(c.qidx, s, c.n_query, c.n_tracks);
    const bool live = src >= 0 && br_frame_live(t, c.T);
    if (slot == 0 && t == 0 && lane == 0) a.bf[b] = c.T;
    const int64_t orow = ((int64_t)b * (sup ? a.N : a.Q) + s) * a.T + t;
    float* otr = (sup ? a.st : a.qt) + orow * 3;
    float* ovis = (sup ? a.sv : a.qv) + orow;
    bool write_qp = false;
    if (!sup) {  // the slot's query_points row: written at its query frame, or as zeros at frame 0 when the slot has none
      const int qf = src >= 0 ? c.qframe[s] : -1;
      const bool has = src >= 0 && br_frame_live(qf, c.T);
      if (t == 0 && !has && lane < 4) a.qp[((int64_t)b * a.Q + s) * 4 + lane] = 0.f;
      write_qp = has && t == qf;
    }
    if (!live) {
      if (lane < 3) otr[lane] = 0.f;
      if (lane == 3) *ovis = 0.f;
      if (sup && a.dino) bb_zero_row<OT>(a.dino, orow * a.D, a.D, (a.vec & 1) != 0, lane);
      if (sup && a.depthf) bb_zero_row<OT>(a.depthf, orow * a.DD, a.DD, (a.vec & 2) != 0, lane);
      continue;
    }
    const int64_t p = (int64_t)src * c.T + t;
    float x = 0.f, y = 0.f;
    if (c.tracks_2d) { x = c.tracks_2d[p * 2]; y = c.tracks_2d[p * 2 + 1]; }
    const bool depth_rows = sup && a.depthf && c.depth_feat;
    float d = 0.f;
    if (!c.tracks_3d || depth_rows) d = br_depth_at(c.depth + (int64_t)t * c.H * c.W, c.H, c.W, x, y);
    float xyz[3];
    if (c.tracks_3d) { xyz[0] = c.tracks_3d[p * 3]; xyz[1] = c.tracks_3d[p * 3 + 1]; xyz[2] = c.tracks_3d[p * 3 + 2]; }
    else br_lift(x, y, d, c.k, xyz);
    if (lane < 3) otr[lane] = lane == 0 ? xyz[0] : (lane == 1 ? xyz[1] : xyz[2]);
    if (lane == 3) *ovis = c.visible[p];
    if (write_qp && lane < 4) a.qp[((int64_t)b * a.Q + s) * 4 + lane] = lane == 0 ? (float)t : (lane == 1 ? xyz[0] : (lane == 2 ? xyz[1] : xyz[2]));
    if (!sup) continue;
    if (a.dino) {
      const int D = a.D;
      const int64_t o = orow * D;
      if (c.dino_pool) {
        bb_copy_row<OT>(a.dino, o, c.dino_pool, p * D, D, (a.vec & 1) != 0, lane);
      } else {
        const BrCorner k = br_corners(x * c.sw, y * c.sh, c.Wp, c.Hp);
        const float* base = c.dino_map + (int64_t)t * c.Hp * c.Wp * D;
        const float* r00 = base + ((int64_t)k.y0 * c.Wp + k.x0) * D; const float* r01 = base + ((int64_t)k.y0 * c.Wp + k.x1) * D;
        const float* r10 = base + ((int64_t)k.y1 * c.Wp + k.x0) * D; const float* r11 = base + ((int64_t)k.y1 * c.Wp + k.x1) * D;
        if (a.vec & 1) {
          for (int ch = lane * 4; ch < D; ch += 256) {
            const float4 f0 = *(const float4*)(r00 + ch), f1 = *(const float4*)(r01 + ch), f2 = *(const float4*)(r10 + ch), f3 = *(const float4*)(r11 + ch);
            bb_store4<OT>(a.dino, o + ch, br_blend(f0.x, f1.x, f2.x, f3.x, k.wx, k.wy), br_blend(f0.y, f1.y, f2.y, f3.y, k.wx, k.wy),
                          br_blend(f0.z, f1.z, f2.z, f3.z, k.wx, k.wy), br_blend(f0.w, f1.w, f2.w, f3.w, k.wx, k.wy));
          }
        } else {
          for (int ch = lane; ch < D; ch += 64) br_store<OT>(a.dino, o + ch, br_blend(r00[ch], r01[ch], r10[ch], r11[ch], k.wx, k.wy));
        }
      }
    }
    if (a.depthf) {
      const int DD = a.DD;
      const int64_t o = orow * DD;
      if (!c.depth_feat) {
        bb_copy_row<OT>(a.depthf, o, c.depth_pool, p * DD, DD, (a.vec & 2) != 0, lane);
      } else {
        float dp = 0.f;  // the same track one frame earlier, at its own position there
        if (t > 0) dp = br_depth_at(c.depth + (int64_t)(t - 1) * c.H * c.W, c.H, c.W, c.tracks_2d[(p - 1) * 2], c.tracks_2d[(p - 1) * 2 + 1]);
        if (a.vec & 2) {
          for (int ch = lane * 4; ch < DD; ch += 256)
            bb_store4<OT>(a.depthf, o + ch, br_depth_feature(ch, d, dp, t), br_depth_feature(ch + 1, d, dp, t), br_depth_feature(ch + 2, d, dp, t), br_depth_feature(ch + 3, d, dp, t));
        } else {
          for (int ch = lane; ch < DD; ch += 64) br_store<OT>(a.depthf, o + ch, br_depth_feature(ch, d, dp, t));
        }
      }
    }
  }
}

void k_build_batch(spa3d_ctx* c, const BbArgs& a, int out_type) {
  if (c->dry || a.nclips <= 0) return;
  const int64_t items = ((int64_t)a.N + a.Q) * a.T * a.nclips;
  const unsigned grid = (unsigned)std::min<int64_t>((items + 3) / 4, (int64_t)1 << 30);
  if (out_type == BR_F32) build_batch_kernel<BR_F32><<<grid, 256, 0, c->stream>>>(a);
  else if (out_type == BR_BF16) build_batch_kernel<BR_BF16><<<grid, 256, 0, c->stream>>>(a);
  else build_batch_kernel<BR_F16><<<grid, 256, 0, c->stream>>>(a);
  SPA_LAUNCH_CHECK(c);
}

}  // namespace SPA_NS
