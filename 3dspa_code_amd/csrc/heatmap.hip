// heatmap.hip -- spa3d_render_heatmap (include/spa3d.h), kernels first, entry points below them: dense per-frame maps of a clip's track values
// and their overlay on the video.  All arithmetic is heatmap_px.hpp's and render_px.hpp's (shared with the g++ host test); this file only decides
// which thread runs it on what.  No 16-bit code: compiled once.
//
//   heatmap_minmax_kernel  partial (min, max) of the finite values, one pair per workgroup (at most HM_PARTS), fixed tree, no atomics
//   heatmap_range_kernel   one workgroup: the partials -> range[2]
//   heatmap_points_kernel  one thread per point-frame, in the order of its stores: pts[t][i] = (packed position or HM_NO_POINT, value) --
//                          frame-major, so the tile pass reads a chunk of points with one coalesced load
//   heatmap_tiles_kernel   one workgroup per (frame, 64 x 16 tile), 256 threads, thread = 4 neighbouring pixels of one row.  The N points are
//                          walked in chunks of HM_CHUNK: each thread tests one point's box (its position grown by radius) against the tile, the
//                          hits are compacted IN INDEX ORDER into an LDS list of (position, value) (ballot + popcount inside each 64-lane wave,
//                          the four wave totals prefix-summed through LDS), and the list is added into the four (num, den) pairs the thread
//                          keeps in registers -- every thread reads the same entry, a broadcast read -- before the next chunk.  LDS: the list
//                          of HM_CHUNK entries and four counters, whatever N is; no overflow case.  Every output element is stored once by its
//                          owner (16 bytes at a time where the four floats are aligned), a video pixel is loaded once and stored once, so
//                          out == video is legal; no atomics, no hand-off between workgroups.
#include <algorithm>

#include "common.hpp"
#include "heatmap_px.hpp"  // eligibility, weight, sums, map value, overlay (host- and device-callable)

// The launches of spa3d_render_heatmap: the caller's tensors and the workspace arrays of the preparation.
struct HeatmapArgs {
  HmClip c;
  const float* tracks; const double* K; const double* E; const float* values; const float* visible;
  float* map; float* weight; const uint8_t* video; uint8_t* out;
  float* part;         // [HM_PARTS][2]: partial (min, max) of the finite values
  const float* range;  // [2]: the clip's (min, max), or null: lo, hi below
  float* range_w;      // the same array, for the kernel that writes it
  int2* pts;           // [T][N]: (packed position or HM_NO_POINT, the value's bits)
  float lo, hi;
  int alpha, colour_bgr, nparts;
};
constexpr int HM_PARTS = 256;   // partial min / max pairs: one per workgroup of the reduction
constexpr int HM_CHUNK = 256;   // points culled and compacted per round of the tile pass (= its workgroup size)

namespace SPA_NS {

static inline int64_t hcdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

constexpr int HM_THREADS = 256;  // = HM_CHUNK: one point per thread in the cull
constexpr int HM_TILE_W = 64, HM_TILE_H = 16, HM_PX = 4;
static_assert(HM_THREADS == HM_CHUNK && HM_TILE_W * HM_TILE_H == HM_THREADS * HM_PX && HM_PARTS <= HM_THREADS, "thread <-> pixel / point / partial maps");

// (min, max) of a workgroup's values by a fixed tree; every thread returns the result
__device__ __forceinline__ void hm_block_minmax(float& mn, float& mx) {
  __shared__ float smn[HM_THREADS], smx[HM_THREADS];
  smn[threadIdx.x] = mn; smx[threadIdx.x] = mx;
  __syncthreads();
  for (int o = HM_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) rp_minmax_merge(smn[threadIdx.x], smx[threadIdx.x], smn[threadIdx.x + o], smx[threadIdx.x + o]);
    __syncthreads();
  }
  mn = smn[0]; mx = smx[0];
}

__global__ __launch_bounds__(HM_THREADS) void heatmap_minmax_kernel(const HeatmapArgs a) {
  const int64_t n = (int64_t)a.c.N * a.c.T;
  float mn, mx;
  rp_minmax_init(mn, mx);
  for (int64_t j = (int64_t)blockIdx.x * HM_THREADS + threadIdx.x; j < n; j += (int64_t)gridDim.x * HM_THREADS) rp_minmax_add(mn, mx, a.values[j]);
  hm_block_minmax(mn, mx);
  if (threadIdx.x == 0) { a.part[2 * blockIdx.x] = mn; a.part[2 * blockIdx.x + 1] = mx; }
}
__global__ __launch_bounds__(HM_THREADS) void heatmap_range_kernel(const HeatmapArgs a) {
  float mn, mx;
  rp_minmax_init(mn, mx);
  if ((int)threadIdx.x < a.nparts) { mn = a.part[2 * threadIdx.x]; mx = a.part[2 * threadIdx.x + 1]; }
  hm_block_minmax(mn, mx);
  if (threadIdx.x == 0) { a.range_w[0] = mn; a.range_w[1] = mx; }
}
void k_heatmap_range(spa3d_ctx* c, const HeatmapArgs& a) {
  if (c->dry) return;
  heatmap_minmax_kernel<<<(unsigned)a.nparts, HM_THREADS, 0, c->stream>>>(a);
  SPA_LAUNCH_CHECK(c);
  heatmap_range_kernel<<<1, HM_THREADS, 0, c->stream>>>(a);
  SPA_LAUNCH_CHECK(c);
}

__global__ __launch_bounds__(HM_THREADS) void heatmap_points_kernel(const HeatmapArgs a) {
  const int64_t j = (int64_t)blockIdx.x * HM_THREADS + threadIdx.x;  // j = t * N + i: the order of the stores
  if (j >= (int64_t)a.c.N * a.c.T) return;
  const int t = (int)(j / a.c.N), i = (int)(j % a.c.N);
  const int64_t s = (int64_t)i * a.c.T + t;
  const float v = a.values[s];
  int32_t pos[2];
  const bool ok = hm_point_frame(a.c, a.tracks + s * a.c.coords, a.K ? a.K + (int64_t)t * 9 : nullptr, a.E ? a.E + (int64_t)t * 16 : nullptr, v, a.visible != nullptr,
                                 a.visible ? a.visible[s] : 0.f, pos);
  a.pts[j] = make_int2(ok ? hm_pack(pos) : HM_NO_POINT, __float_as_int(v));
}
void k_heatmap_points(spa3d_ctx* c, const HeatmapArgs& a) {
  if (c->dry) return;
  heatmap_points_kernel<<<(unsigned)hcdiv((int64_t)a.c.N * a.c.T, HM_THREADS), HM_THREADS, 0, c->stream>>>(a);
  SPA_LAUNCH_CHECK(c);
}

__global__ __launch_bounds__(HM_THREADS) void heatmap_tiles_kernel(const HeatmapArgs a) {
  __shared__ int2 list[HM_CHUNK];
  __shared__ int wave_hits[HM_THREADS / 64];
  const int N = a.c.N, H = a.c.H, W = a.c.W, r = a.c.radius, R2 = r * r, power = a.c.power;
  const int tiles_x = (W + HM_TILE_W - 1) / HM_TILE_W, tiles_y = (H + HM_TILE_H - 1) / HM_TILE_H;
  const int t = (int)(blockIdx.x / ((unsigned)tiles_x * tiles_y));
  const int tile = (int)(blockIdx.x - (unsigned)t * tiles_x * tiles_y);
  const int tx0 = (tile % tiles_x) * HM_TILE_W, ty0 = (tile / tiles_x) * HM_TILE_H;          // the tile: [tx0, tx0 + 64) x [ty0, ty0 + 16)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Y = ty0 + tid / (HM_TILE_W / HM_PX), X0 = tx0 + (tid % (HM_TILE_W / HM_PX)) * HM_PX;
  const int npx = Y < H ? (W - X0 < 0 ? 0 : (W - X0 > HM_PX ? HM_PX : W - X0)) : 0;   // this thread's pixels inside the image: the tails

  double num[HM_PX];
  uint64_t den[HM_PX];
#pragma unroll
  for (int q = 0; q < HM_PX; ++q) { num[q] = 0.0; den[q] = 0; }

  const int2* pts = a.pts + (int64_t)t * N;
  for (int base = 0; base < N; base += HM_CHUNK) {
    const int i = base + tid;
    bool hit = false;
    int2 p = make_int2(HM_NO_POINT, 0);
    if (i < N) {
      p = pts[i];
      if (p.x != HM_NO_POINT) {
        int x, y;
        hm_unpack(p.x, x, y);
        hit = x + r >= tx0 && x - r < tx0 + HM_TILE_W && y + r >= ty0 && y - r < ty0 + HM_TILE_H;
      }
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wave_hits[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < HM_THREADS / 64; ++w) { const int h = wave_hits[w]; before += w < wave ? h : 0; total += h; }
    if (hit) list[before + __popcll(m & ((1ull << lane) - 1ull))] = p;   // index order: lanes in order inside a wave, waves in order
    __syncthreads();
    for (int k = 0; k < total; ++k) {
      const int2 e = list[k];  // the same entry for the whole workgroup
      int x, y;
      hm_unpack(e.x, x, y);
      const int dy = Y - y;
      if (dy * dy > R2) continue;
      const float v = __int_as_float(e.y);
#pragma unroll
      for (int q = 0; q < HM_PX; ++q) {
        const uint32_t w = hm_weight(X0 + q - x, dy, R2, power);
        if (w) hm_add(num[q], den[q], w, v);
      }
    }
    __syncthreads();  // the list and the counters are rewritten by the next chunk
  }

  if (npx == 0) return;
  const int64_t px = ((int64_t)t * H + Y) * W + X0;
  float mv[HM_PX], wv[HM_PX];
#pragma unroll
  for (int q = 0; q < HM_PX; ++q) { mv[q] = hm_value(num[q], den[q]); wv[q] = hm_weight_out(den[q]); }
  float* const outs[2] = {a.map, a.weight};
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    if (!outs[o]) continue;
    float* d = outs[o] + px;
    const float* s = o ? wv : mv;
    if (npx == HM_PX && ((uintptr_t)d & 15) == 0) {
      *reinterpret_cast<float4*>(d) = make_float4(s[0], s[1], s[2], s[3]);
    } else {
#pragma unroll
      for (int q = 0; q < HM_PX; ++q)
        if (q < npx) d[q] = s[q];
    }
  }
  if (!a.out) return;

  bool any = false;
#pragma unroll
  for (int q = 0; q < HM_PX; ++q) any |= q < npx && den[q] != 0;
  const uint8_t* src = a.video + px * 3;
  uint8_t* dst = a.out + px * 3;
  if (!any && dst == src) return;   // in place and nothing reaches these pixels: the bytes are already there
  const float lo = a.range ? a.range[0] : a.lo, hi = a.range ? a.range[1] : a.hi;
  int ch[HM_PX][3];
  if (npx == HM_PX && ((uintptr_t)src & 3) == 0) {   // 12 bytes as three dwords when whole and aligned
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
    const uint32_t w0 = s4[0], w1 = s4[1], w2 = s4[2];
#pragma unroll
    for (int q = 0; q < 12; ++q) ch[q / 3][q % 3] = (int)((q < 4 ? w0 : q < 8 ? w1 : w2) >> (8 * (q & 3)) & 255u);
  } else {
#pragma unroll
    for (int q = 0; q < HM_PX; ++q)
#pragma unroll
      for (int c = 0; c < 3; ++c) ch[q][c] = q < npx ? (int)src[q * 3 + c] : 0;
  }
#pragma unroll
  for (int q = 0; q < HM_PX; ++q)
    if (q < npx) hm_overlay(mv[q], den[q], lo, hi, a.colour_bgr != 0, a.alpha, ch[q]);
  if (npx == HM_PX && ((uintptr_t)dst & 3) == 0) {
    uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < 12; ++q) w[q >> 2] |= (uint32_t)ch[q / 3][q % 3] << (8 * (q & 3));
    uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
    d4[0] = w[0]; d4[1] = w[1]; d4[2] = w[2];
  } else {
#pragma unroll
    for (int q = 0; q < HM_PX; ++q)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (q < npx) dst[q * 3 + c] = (uint8_t)ch[q][c];
  }
}
void k_heatmap_tiles(spa3d_ctx* c, const HeatmapArgs& a) {
  if (c->dry) return;
  const int64_t blocks = (int64_t)a.c.T * hcdiv(a.c.W, HM_TILE_W) * hcdiv(a.c.H, HM_TILE_H);   // < 2^24: checked by the entry
  heatmap_tiles_kernel<<<(unsigned)blocks, HM_THREADS, 0, c->stream>>>(a);
  SPA_LAUNCH_CHECK(c);
}

}  // namespace SPA_NS

// ---- the entry points ----
// The launches of one call.  Runs twice: dry (no launch, a counting arena: the workspace the call needs) and for real.  Workspace: the partial
// min / max pairs and the range when the overlay is normalised, and the (position, value) pairs of the N x T point-frames.
static void heatmap_body(spa3d_ctx* c, const spa3d_heatmap* m) {
  const int64_t n = (int64_t)m->N * m->T;
  HeatmapArgs a{};
  a.c = HmClip{m->N, m->T, m->H, m->W, m->coords, m->resize_h, m->resize_w, m->use_visibility != 0, m->radius, m->power};
  a.tracks = m->tracks; a.K = m->coords == 3 ? m->intrinsics : nullptr; a.E = m->coords == 3 ? m->extrinsics : nullptr;
  a.values = m->values; a.visible = m->use_visibility ? m->visible : nullptr;
  a.map = m->map; a.weight = m->weight; a.video = m->video; a.out = m->out;
  a.lo = m->lo; a.hi = m->hi; a.alpha = m->alpha; a.colour_bgr = m->colour_bgr;
  a.nparts = (int)std::min<int64_t>(HM_PARTS, (n + HM_CHUNK - 1) / HM_CHUNK);
  if (m->out && m->normalize) {
    a.part = (float*)c->ar.alloc(HM_PARTS * 2 * 4);
    a.range_w = (float*)c->ar.alloc(2 * 4); a.range = a.range_w;
    SPA_NS::k_heatmap_range(c, a);
  }
  a.pts = (int2*)c->ar.alloc(n * 8);
  SPA_NS::k_heatmap_points(c, a);
  SPA_NS::k_heatmap_tiles(c, a);
}
static int64_t heatmap_need(spa3d_ctx* c, const spa3d_heatmap* m) {
  return arena_peak(c, [&] { heatmap_body(c, m); }) + 256;
}

extern "C" {

int64_t spa3d_heatmap_workspace_bytes(spa3d_handle h, int32_t N, int32_t T) {
  if (!h || N <= 0 || T <= 0) return -1;
  const int64_t n = (int64_t)N * T;
  auto up = [](int64_t b) { return (b + 255) & ~int64_t(255); };
  return up(HM_PARTS * 2 * 4) + up(2 * 4) + up(n * 8) + 256;
}
int spa3d_render_heatmap(spa3d_handle h, const spa3d_heatmap* m, void* ws, int64_t ws_bytes, void* stream) {
  if (!h) return SPA3D_ERR_ARG;
  h->err.clear(); h->hip_err = 0;
  auto bad = [&](const std::string& s) { h->err = "heatmap: " + s; return SPA3D_ERR_ARG; };
  if (!m) return bad("spa3d_heatmap is required");
  if (m->N < 1 || m->T < 1) return bad("N = " + std::to_string(m->N) + ", T = " + std::to_string(m->T) + ": both must be positive");
  if (m->H < 1 || m->H > RP_MAX_DIM || m->W < 1 || m->W > RP_MAX_DIM)
    return bad("H = " + std::to_string(m->H) + ", W = " + std::to_string(m->W) + " are outside [1, " + std::to_string(RP_MAX_DIM) + "]");
  if (!m->tracks) return bad("tracks is required");
  if (!m->values) return bad("values is required");
  if (m->coords != 2 && m->coords != 3) return bad("coords = " + std::to_string(m->coords) + " is neither 2 nor 3");
  if (m->coords == 3 && (!m->intrinsics || !m->extrinsics)) return bad("coords == 3 needs the camera matrices (intrinsics, extrinsics)");
  if (m->coords == 3 && (m->resize_h < 1 || m->resize_w < 1)) return bad("coords == 3 needs resize_h, resize_w >= 1");
  if (!m->map && !m->weight && !m->out) return bad("nothing to do: map, weight and out are all NULL");
  if (m->out && !m->video) return bad("the overlay (out) needs video");
  if (m->use_visibility && !m->visible) return bad("use_visibility needs visible");
  if (m->radius < 1 || m->radius > HM_MAX_RADIUS) return bad("radius = " + std::to_string(m->radius) + " is outside [1, " + std::to_string(HM_MAX_RADIUS) + "]");
  if (m->power != 1 && m->power != 2) return bad("power = " + std::to_string(m->power) + " is neither 1 nor 2");
  if (m->alpha < 0 || m->alpha > HM_MAX_ALPHA) return bad("alpha = " + std::to_string(m->alpha) + " is outside [0, " + std::to_string(HM_MAX_ALPHA) + "]");
  if (m->out && !m->normalize && !(rp_finite(m->lo) && rp_finite(m->hi))) return bad("normalize == 0 needs finite lo, hi");
  // a launch holds fewer than 2^32 threads: one thread per point-frame, 256 per (frame, tile)
  if ((int64_t)m->N * m->T > (int64_t)1 << 31) return bad("N x T = " + std::to_string((int64_t)m->N * m->T) + " point-frames exceed one launch (2^31)");
  if ((int64_t)m->T * ((m->W + 63) / 64) * ((m->H + 15) / 16) >= (int64_t)1 << 24) return bad("T x tiles reaches 2^24 workgroups: more than one launch holds");
  return sized_call(h, "heatmap", heatmap_need(h, m), ws, ws_bytes, stream, [&] { heatmap_body(h, m); });
}

}  // extern "C"
