// batch_build.hip -- spa3d_build_batch and spa3d_build_windows (include/spa3d.h), the kernel first, the entry points below it: clips -> the padded model batch, in one launch per BB_CLIPS clips.
// A window of a long clip (spa3d_build_windows) is a clip whose descriptor carries a frame offset t0 and the long arrays' row stride TL: the same kernel reads it in place.
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
#include "build_row.hpp"  // samplers, slot rule, the rounding to the feature type (host- and device-callable)

#include <algorithm>

// One launch of spa3d_build_batch: up to BB_CLIPS clips by value -- what fits in kernel arguments with room to spare -- and the
// batch's buffers.  Clip g of the launch fills sample b0 + g.  Every pointer is a device pointer; the intrinsics and the map scales are already float32.
constexpr int BB_CLIPS = 16;
struct BbClip {
  const float* tracks_2d; const float* tracks_3d; const float* visible; const float* depth; const float* dino_map;
  const void* dino_pool; const void* depth_pool;   // rows in the feature type, copied
  const int32_t* sidx; const int32_t* qidx; const int32_t* qframe;
  int32_t n_tracks, T, H, W, Hp, Wp, n_support, n_query;
  BrIntr k; float sw, sh;
  int32_t depth_feat;   // the depth-feature channels come from the depth map (0: from depth_pool, or there are none)
  int32_t t0, TL;       // the clip is frames [t0, t0 + T) of arrays that hold TL frames (spa3d_build_windows); spa3d_build_batch: 0 and T
};
struct BbArgs {
  BbClip clip[BB_CLIPS];
  float* st; float* sv; float* qp; float* qt; float* qv; int32_t* bf; void* dino; void* depthf;   // the batch: [B,N,T,3] [B,N,T] [B,Q,4] [B,Q,T,3] [B,Q,T] [B] [B,N,T,D] [B,N,T,DD]
  int32_t b0, nclips, N, Q, T, D, DD;
  int32_t vec;   // D % 4 == 0 and every DINO pointer 16-byte aligned: 16-byte accesses along the channel axis
};

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
    const int ts = c.t0 + t;                    // the frame of the source arrays
    const int64_t p = (int64_t)src * c.TL + ts;
    float x = 0.f, y = 0.f;
    if (c.tracks_2d) { x = c.tracks_2d[p * 2]; y = c.tracks_2d[p * 2 + 1]; }
    const bool depth_rows = sup && a.depthf && c.depth_feat;
    float d = 0.f;
    if (!c.tracks_3d || depth_rows) d = br_depth_at(c.depth + (int64_t)ts * c.H * c.W, c.H, c.W, x, y);
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
        const float* base = c.dino_map + (int64_t)ts * c.Hp * c.Wp * D;
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
        float dp = 0.f;  // the same track one frame earlier, at its own position there (t is the clip's frame: a window's first frame has no earlier one)
        if (t > 0) dp = br_depth_at(c.depth + (int64_t)(ts - 1) * c.H * c.W, c.H, c.W, c.tracks_2d[(p - 1) * 2], c.tracks_2d[(p - 1) * 2 + 1]);
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

// ---- the entry points ----
// Both entry points are this one walk.  t0 == nullptr: spa3d_build_batch, sample i is clips[i].  t0 given: spa3d_build_windows, sample w is
// frames [t0[w], t0[w] + out->T) of the ONE clip clips[0], addressed in place.
// Everything is checked for every clip before the first launch; then one launch per BB_CLIPS samples, their descriptors by value.
static int bb_build(spa3d_handle h, const spa3d_clip* clips, int32_t W, const int32_t* t0, spa3d_batch* out, void* stream, bool windows) {
  if (!h) return SPA3D_ERR_ARG;
  h->err.clear(); h->hip_err = 0;
  auto bad = [&](const std::string& m) { h->err = std::string(windows ? "build_windows: " : "build_batch: ") + m; return SPA3D_ERR_ARG; };
  if (h->cfg.model_kind == 1) return bad("the 2-D model (model_kind 1) has no depth coordinate");
  if (!clips) return bad(windows ? "clip is required" : "clips is required");
  if (!out) return bad("out is required");
  if (windows) {
    if (!t0) return bad("t0 is required");
    if (W < 1 || out->B != W) return bad("W = " + std::to_string(W) + ", out->B = " + std::to_string(out->B) + " (W >= 1 and out->B == W)");
  }
  if (out->B < 1 || out->N < 1 || out->Q < 0 || out->T < 1)
    return bad("out: B = " + std::to_string(out->B) + ", N = " + std::to_string(out->N) + ", Q = " + std::to_string(out->Q) + ", T = " + std::to_string(out->T) + " (B, N, T >= 1 and Q >= 0)");
  if (!out->support_tracks || !out->support_tracks_visible || !out->boundary_frame) return bad("out needs support_tracks, support_tracks_visible and boundary_frame");
  if (out->Q > 0 && (!out->query_points || !out->query_tracks || !out->query_tracks_visible)) return bad("out needs query_points, query_tracks and query_tracks_visible when Q > 0");
  const int D = h->cfg.dino_feature_dim, DD = h->cfg.depth_feature_dim;
  if (out->dino_features && D <= 0) return bad("out carries dino_features but the handle has no DINO feature (dino_feature_dim = 0)");
  if (out->depth_features && DD <= 0) return bad("out carries depth_features but the handle has no depth feature (depth_feature_dim = 0)");
  auto aligned = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
  bool vec_dino = (D & 3) == 0 && aligned(out->dino_features), vec_depth = (DD & 3) == 0 && aligned(out->depth_features);
  for (int i = 0; i < (windows ? 1 : out->B); ++i) {
    const spa3d_clip& k = clips[i];
    auto cbad = [&](const std::string& m) { return bad("clip " + std::to_string(i) + ": " + m); };
    if (k.n_tracks < 1) return cbad("n_tracks = " + std::to_string(k.n_tracks) + " must be positive");
    if (windows && k.T < 1) return cbad("T = " + std::to_string(k.T) + " must be positive");
    if (!windows && (k.T < 1 || k.T > out->T)) return cbad("T = " + std::to_string(k.T) + " is outside [1, " + std::to_string(out->T) + "] (the batch's T)");
    if (k.n_support < 1 || k.n_support > out->N) return cbad("n_support = " + std::to_string(k.n_support) + " is outside [1, " + std::to_string(out->N) + "]");
    if (k.n_query < 0 || k.n_query > out->Q) return cbad("n_query = " + std::to_string(k.n_query) + " is outside [0, " + std::to_string(out->Q) + "]");
    if (!k.visible) return cbad("visible is required");
    if (!k.support_index) return cbad("support_index is required");
    if (k.n_query > 0 && (!k.query_index || !k.query_frame)) return cbad("query_index and query_frame are required when n_query > 0");
    const bool depth_for_feature = out->depth_features && !k.depth_pool;
    const bool need_2d = !k.tracks_3d || k.dino_map || depth_for_feature;
    if (!k.tracks_3d && !k.depth_map) return cbad("a lift needs depth_map (or give tracks_3d)");
    if (need_2d && !k.tracks_2d) return cbad("tracks_2d is required to lift or to sample a map");
    if ((k.dino_map || !k.tracks_3d || depth_for_feature) && (k.H < 1 || k.W < 1)) return cbad("H = " + std::to_string(k.H) + ", W = " + std::to_string(k.W) + ": the video size must be positive");
    if (k.dino_map && k.dino_pool) return cbad("dino_map and dino_pool are both given");
    if (!out->dino_features && (k.dino_map || k.dino_pool)) return cbad("carries DINO but out->dino_features is NULL");
    if (out->dino_features && !k.dino_map && !k.dino_pool) return cbad("out carries dino_features: dino_map or dino_pool is required");
    if (k.dino_map && (k.Hp < 1 || k.Wp < 1)) return cbad("Hp = " + std::to_string(k.Hp) + ", Wp = " + std::to_string(k.Wp) + ": the map size must be positive");
    if (k.depth_pool && k.depth_map && k.tracks_3d) return cbad("depth_map and depth_pool are both given (and no lift needs the map)");
    if (!out->depth_features && k.depth_pool) return cbad("carries depth features but out->depth_features is NULL");
    if (depth_for_feature && !k.depth_map) return cbad("out carries depth_features: depth_map or depth_pool is required");
    vec_dino = vec_dino && aligned(k.dino_map) && aligned(k.dino_pool);
    vec_depth = vec_depth && aligned(k.depth_pool);
  }
  if (windows) {
    const int TL = clips[0].T;
    for (int w = 0; w < W; ++w) {
      if (t0[w] < 0 || t0[w] >= TL) return bad("t0[" + std::to_string(w) + "] = " + std::to_string(t0[w]) + " is outside [0, " + std::to_string(TL) + ") (the clip's T)");
      if (w > 0 && t0[w] <= t0[w - 1]) return bad("t0 must increase strictly (t0[" + std::to_string(w) + "] = " + std::to_string(t0[w]) + ")");
    }
  }
  h->stream = (hipStream_t)stream; h->dry = false;
  for (int b0 = 0; b0 < out->B; b0 += BB_CLIPS) {
    BbArgs a{};
    a.b0 = b0; a.nclips = std::min(BB_CLIPS, out->B - b0); a.N = out->N; a.Q = out->Q; a.T = out->T; a.D = D; a.DD = DD;
    a.st = (float*)out->support_tracks; a.sv = (float*)out->support_tracks_visible; a.qp = (float*)out->query_points; a.qt = (float*)out->query_tracks;
    a.qv = (float*)out->query_tracks_visible; a.bf = (int32_t*)out->boundary_frame; a.dino = (void*)out->dino_features; a.depthf = (void*)out->depth_features;
    a.vec = (vec_dino ? 1 : 0) | (vec_depth ? 2 : 0);
    for (int g = 0; g < a.nclips; ++g) {
      const spa3d_clip& k = clips[windows ? 0 : b0 + g];
      BbClip& c = a.clip[g];
      c.tracks_2d = k.tracks_2d; c.tracks_3d = k.tracks_3d; c.visible = k.visible; c.depth = k.depth_map; c.dino_map = k.dino_map;
      c.dino_pool = k.dino_pool; c.depth_pool = k.depth_pool; c.sidx = k.support_index; c.qidx = k.query_index; c.qframe = k.query_frame;
      c.n_tracks = k.n_tracks; c.T = k.T; c.H = k.H; c.W = k.W; c.Hp = k.Hp; c.Wp = k.Wp; c.n_support = k.n_support; c.n_query = k.n_query;
      c.k = br_intrinsics(k.intrinsics, k.H, k.W);
      c.sw = k.dino_map ? br_map_scale(k.Wp, k.W) : 0.f; c.sh = k.dino_map ? br_map_scale(k.Hp, k.H) : 0.f;
      c.depth_feat = (out->depth_features && !k.depth_pool) ? 1 : 0;
      c.t0 = 0; c.TL = k.T;
      if (windows) {  // a window is a clip that starts at t0[w]: its own length, its own row of window-relative query frames
        const int w = b0 + g;
        c.t0 = t0[w]; c.T = std::min(out->T, k.T - t0[w]);
        if (k.n_query > 0) c.qframe = k.query_frame + (int64_t)w * k.n_query;
      }
    }
    k_build_batch(h, a, h->cfg.precision);
  }
  return h->hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}

extern "C" {

int spa3d_build_batch(spa3d_handle h, const spa3d_clip* clips, spa3d_batch* out, void* stream) { return bb_build(h, clips, 0, nullptr, out, stream, false); }

int spa3d_build_windows(spa3d_handle h, const spa3d_clip* clip, int32_t W, const int32_t* t0, spa3d_batch* out, void* stream) {
  return bb_build(h, clip, W, t0, out, stream, true);
}

}  // extern "C"
