// render.hip -- spa3d_render_tracks (include/spa3d.h), kernels first, entry points below them: score-coloured track overlays drawn into a clip's frames.
// All arithmetic is render_px.hpp's (shared with the g++ host test); this file only decides which thread runs it on what.  No 16-bit code:
// compiled once.
//
//   render_minmax_kernel  partial (min, max) of the finite scores, one pair per workgroup (at most RENDER_PARTS), fixed tree, no atomics
//   render_points_kernel  one thread per point-frame: finishes the min / max from the partials, then position, flag word, `pixels`
//   render_boxes_kernel   one thread per point-frame: the box of everything the point draws in that frame -> box[t][i] (frame-major, so
//                         the tile pass reads a chunk of points with one coalesced load)
//   render_tiles_kernel   one workgroup per (frame, 64 x 16 tile), 256 threads, thread = 4 neighbouring pixels of one row.  The N points are
//                         walked in chunks of RENDER_CHUNK: each thread tests one point's box against the tile, the hits are compacted IN INDEX
//                         ORDER into an LDS list (ballot + popcount inside each 64-lane wave, the four wave totals prefix-summed through LDS), and
//                         the list is composited into the registers that hold the thread's pixels before the next chunk.  LDS: the list of
//                         RENDER_CHUNK indices and four counters, whatever N is; no overflow case.  A pixel is loaded once and stored once by
//                         its owner, so out == video is legal; no atomics, no hand-off between workgroups.
#include <algorithm>

#include "common.hpp"
#include "render_px.hpp"  // colour, projection, coverage, blend (host- and device-callable)

// The launches of spa3d_render_tracks: the caller's tensors and the workspace arrays of the preparation.
struct RenderArgs {
  RpClip c;
  const uint8_t* video; uint8_t* out; const float* tracks; const double* K; const double* E; const float* scores; const float* visible;
  int32_t* pixels;     // caller's [N][T][2] or null
  float* part;         // [RENDER_PARTS][2]: partial (min, max) of the finite scores
  int32_t* pos;        // [N][T][2]
  uint32_t* fl;        // [N][T]: flag words (render_px.hpp)
  short* box;          // [T][N][4]: x0, y0, x1, y1 of everything point i draws in frame t (x0 > x1: nothing)
  int nparts;
};
constexpr int RENDER_PARTS = 256;   // partial min / max pairs: one per workgroup of the reduction
// RENDER_CHUNK, the points culled and compacted per round of the tile pass, is in common.hpp: tests/test_gpu_render.py reads it there

namespace SPA_NS {

static inline int64_t rcdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

constexpr int RENDER_THREADS = 256;  // = RENDER_CHUNK: one point per thread in the cull
constexpr int TILE_W = 64, TILE_H = 16, PX_PER_THREAD = 4;
static_assert(RENDER_THREADS == RENDER_CHUNK && TILE_W * TILE_H == RENDER_THREADS * PX_PER_THREAD, "thread <-> pixel / point maps");

// (min, max) of a workgroup's values by a fixed tree; every thread returns the result
__device__ __forceinline__ void block_minmax(float& mn, float& mx) {
  __shared__ float smn[RENDER_THREADS], smx[RENDER_THREADS];
  smn[threadIdx.x] = mn; smx[threadIdx.x] = mx;
  __syncthreads();
  for (int o = RENDER_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) rp_minmax_merge(smn[threadIdx.x], smx[threadIdx.x], smn[threadIdx.x + o], smx[threadIdx.x + o]);
    __syncthreads();
  }
  mn = smn[0]; mx = smx[0];
}

__global__ __launch_bounds__(RENDER_THREADS) void render_minmax_kernel(const RenderArgs a) {
  const int64_t n = (int64_t)a.c.N * a.c.T;
  float mn, mx;
  rp_minmax_init(mn, mx);
  for (int64_t j = (int64_t)blockIdx.x * RENDER_THREADS + threadIdx.x; j < n; j += (int64_t)gridDim.x * RENDER_THREADS) rp_minmax_add(mn, mx, a.scores[j]);
  block_minmax(mn, mx);
  if (threadIdx.x == 0) { a.part[2 * blockIdx.x] = mn; a.part[2 * blockIdx.x + 1] = mx; }
}
void k_render_minmax(spa3d_ctx* c, const RenderArgs& a) {
  if (c->dry) return;
  render_minmax_kernel<<<(unsigned)a.nparts, RENDER_THREADS, 0, c->stream>>>(a);
  SPA_LAUNCH_CHECK(c);
}

__global__ __launch_bounds__(RENDER_THREADS) void render_points_kernel(const RenderArgs a) {
  float mn, mx;
  rp_minmax_init(mn, mx);
  if (a.scores && a.c.normalize) {  // uniform: every thread reaches the barriers inside
    if ((int)threadIdx.x < a.nparts) { mn = a.part[2 * threadIdx.x]; mx = a.part[2 * threadIdx.x + 1]; }
    block_minmax(mn, mx);
  }
  const int64_t j = (int64_t)blockIdx.x * RENDER_THREADS + threadIdx.x;
  if (j >= (int64_t)a.c.N * a.c.T) return;
  const int t = (int)(j % a.c.T);
  int32_t pos[2];
  const uint32_t fl = rp_point_frame(a.c, a.tracks + j * a.c.coords, a.K ? a.K + (int64_t)t * 9 : nullptr, a.E ? a.E + (int64_t)t * 16 : nullptr, a.scores != nullptr,
                                     a.scores ? a.scores[j] : 0.f, mn, mx, a.visible != nullptr, a.visible ? a.visible[j] : 0.f, pos);
  if (a.pos) { a.pos[2 * j] = pos[0]; a.pos[2 * j + 1] = pos[1]; a.fl[j] = fl; }
  if (a.pixels) { a.pixels[2 * j] = pos[0]; a.pixels[2 * j + 1] = pos[1]; }
}
void k_render_points(spa3d_ctx* c, const RenderArgs& a) {
  if (c->dry) return;
  render_points_kernel<<<(unsigned)rcdiv((int64_t)a.c.N * a.c.T, RENDER_THREADS), RENDER_THREADS, 0, c->stream>>>(a);
  SPA_LAUNCH_CHECK(c);
}

__global__ __launch_bounds__(RENDER_THREADS) void render_boxes_kernel(const RenderArgs a) {
  const int64_t j = (int64_t)blockIdx.x * RENDER_THREADS + threadIdx.x;  // j = t * N + i: the order of the stores
  if (j >= (int64_t)a.c.N * a.c.T) return;
  const int t = (int)(j / a.c.N), i = (int)(j % a.c.N);
  int x0, y0, x1, y1;
  rp_point_box(a.pos + (int64_t)i * a.c.T * 2, a.fl + (int64_t)i * a.c.T, t, a.c.trail, a.c.radius, a.c.H, a.c.W, x0, y0, x1, y1);
  short4 b;  // 0 .. 16383 each
  b.x = (short)x0; b.y = (short)y0; b.z = (short)x1; b.w = (short)y1;
  reinterpret_cast<short4*>(a.box)[j] = b;
}
void k_render_boxes(spa3d_ctx* c, const RenderArgs& a) {
  if (c->dry) return;
  render_boxes_kernel<<<(unsigned)rcdiv((int64_t)a.c.N * a.c.T, RENDER_THREADS), RENDER_THREADS, 0, c->stream>>>(a);
  SPA_LAUNCH_CHECK(c);
}

__global__ __launch_bounds__(RENDER_THREADS) void render_tiles_kernel(const RenderArgs a) {
  __shared__ int list[RENDER_CHUNK];
  __shared__ int wave_hits[RENDER_THREADS / 64];
  const int N = a.c.N, T = a.c.T, H = a.c.H, W = a.c.W;
  const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (H + TILE_H - 1) / TILE_H;
  const int t = (int)(blockIdx.x / ((unsigned)tiles_x * tiles_y));
  const int tile = (int)(blockIdx.x - (unsigned)t * tiles_x * tiles_y);
  const int tx0 = (tile % tiles_x) * TILE_W, ty0 = (tile / tiles_x) * TILE_H;          // the tile: [tx0, tx0 + TILE_W) x [ty0, ty0 + TILE_H)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Y = ty0 + tid / (TILE_W / PX_PER_THREAD), X0 = tx0 + (tid % (TILE_W / PX_PER_THREAD)) * PX_PER_THREAD;
  const int npx = Y < H ? (W - X0 < 0 ? 0 : (W - X0 > PX_PER_THREAD ? PX_PER_THREAD : W - X0)) : 0;   // this thread's pixels inside the image: the tails
  const int64_t off = (((int64_t)t * H + (Y < H ? Y : 0)) * W + (npx ? X0 : 0)) * 3;
  const uint8_t* src = a.video + off;
  uint8_t* dst = a.out + off;

  int ch[PX_PER_THREAD][3];
  const bool wide_in = npx == PX_PER_THREAD && ((uintptr_t)src & 3) == 0;   // 12 bytes as three dwords when whole and aligned
  if (wide_in) {
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
    const uint32_t w0 = s4[0], w1 = s4[1], w2 = s4[2];
#pragma unroll
    for (int q = 0; q < 12; ++q) ch[q / 3][q % 3] = (int)((q < 4 ? w0 : q < 8 ? w1 : w2) >> (8 * (q & 3)) & 255u);
  } else {
#pragma unroll
    for (int q = 0; q < PX_PER_THREAD; ++q)
#pragma unroll
      for (int c = 0; c < 3; ++c) ch[q][c] = q < npx ? (int)src[q * 3 + c] : 0;
  }

  bool any = false;
  const short4* boxes = reinterpret_cast<const short4*>(a.box) + (int64_t)t * N;
  for (int base = 0; base < N; base += RENDER_CHUNK) {
    const int i = base + tid;
    bool hit = false;
    if (i < N) {
      const short4 b = boxes[i];
      hit = b.x <= b.z && b.z >= tx0 && b.x < tx0 + TILE_W && b.w >= ty0 && b.y < ty0 + TILE_H;
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wave_hits[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < RENDER_THREADS / 64; ++w) { const int h = wave_hits[w]; before += w < wave ? h : 0; total += h; }
    if (hit) list[before + __popcll(m & ((1ull << lane) - 1ull))] = i;   // index order: lanes in order inside a wave, waves in order
    __syncthreads();
    any |= total > 0;
    for (int k = 0; k < total; ++k) {
      const int pi = __builtin_amdgcn_readfirstlane(list[k]);  // the same point for the whole workgroup
      rp_for_each_prim(a.pos + (int64_t)pi * T * 2, a.fl + (int64_t)pi * T, t, a.c.trail, a.c.radius, [&](const RpPrim& p) {
        int x0, y0, x1, y1;
        rp_prim_box(p, x0, y0, x1, y1);
        if (x1 < tx0 || x0 >= tx0 + TILE_W || y1 < ty0 || y0 >= ty0 + TILE_H) return;   // not in this tile: the whole workgroup leaves
        if (Y < y0 || Y > y1 || X0 + PX_PER_THREAD - 1 < x0 || X0 > x1) return;
#pragma unroll
        for (int q = 0; q < PX_PER_THREAD; ++q)
          if (q < npx && X0 + q >= x0 && X0 + q <= x1) rp_apply(p, X0 + q, Y, ch[q]);
      });
    }
    __syncthreads();  // the list is rewritten by the next chunk
  }

  if (npx == 0 || (!any && dst == src)) return;   // in place and nothing near this tile: the bytes are already there
  if (npx == PX_PER_THREAD && ((uintptr_t)dst & 3) == 0) {
    uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < 12; ++q) w[q >> 2] |= (uint32_t)ch[q / 3][q % 3] << (8 * (q & 3));
    uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
    d4[0] = w[0]; d4[1] = w[1]; d4[2] = w[2];
  } else {
#pragma unroll
    for (int q = 0; q < PX_PER_THREAD; ++q)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (q < npx) dst[q * 3 + c] = (uint8_t)ch[q][c];
  }
}
void k_render_tiles(spa3d_ctx* c, const RenderArgs& a) {
  if (c->dry) return;
  const int64_t blocks = (int64_t)a.c.T * rcdiv(a.c.W, TILE_W) * rcdiv(a.c.H, TILE_H);   // < 2^31: checked by the entry
  render_tiles_kernel<<<(unsigned)blocks, RENDER_THREADS, 0, c->stream>>>(a);
  SPA_LAUNCH_CHECK(c);
}

}  // namespace SPA_NS

// ---- the entry points ----
// The launches of one call.  Runs twice: dry (no launch, a counting arena: the workspace the call needs) and for real.  Workspace: the partial
// min / max pairs, and -- when frames are drawn -- the positions, flag words and boxes of the N x T point-frames.
static void render_body(spa3d_ctx* c, const spa3d_render* r) {
  const int64_t n = (int64_t)r->N * r->T;
  RenderArgs a{};
  a.c = RpClip{r->N, r->T, r->H, r->W, r->coords, r->resize_h, r->resize_w, r->normalize != 0, r->use_visibility != 0, r->colour_bgr != 0, r->trail, r->point_size};
  a.video = r->video; a.out = r->out; a.tracks = r->tracks; a.K = r->coords == 3 ? r->intrinsics : nullptr; a.E = r->coords == 3 ? r->extrinsics : nullptr;
  a.scores = r->out ? r->scores : nullptr; a.visible = r->use_visibility ? r->visible : nullptr; a.pixels = r->pixels;
  a.nparts = (int)std::min<int64_t>(RENDER_PARTS, (n + RENDER_CHUNK - 1) / RENDER_CHUNK);
  const bool norm = a.scores && r->normalize;
  if (norm) { a.part = (float*)c->ar.alloc(RENDER_PARTS * 2 * 4); k_render_minmax(c, a); }
  if (r->out) {
    a.pos = (int32_t*)c->ar.alloc(n * 8); a.fl = (uint32_t*)c->ar.alloc(n * 4); a.box = (short*)c->ar.alloc(n * 8);
  }
  k_render_points(c, a);
  if (!r->out) return;
  k_render_boxes(c, a);
  k_render_tiles(c, a);
}
static int64_t render_need(spa3d_ctx* c, const spa3d_render* r) {
  return arena_peak(c, [&] { render_body(c, r); }) + 256;  // never 0: a call without a workspace is refused after the walk
}

extern "C" {

int64_t spa3d_render_workspace_bytes(spa3d_handle h, int32_t N, int32_t T) {
  if (!h || N <= 0 || T <= 0) return -1;
  const int64_t n = (int64_t)N * T;
  auto up = [](int64_t b) { return (b + 255) & ~int64_t(255); };
  return up(RENDER_PARTS * 2 * 4) + up(n * 8) + up(n * 4) + up(n * 8) + 256;
}
int spa3d_render_tracks(spa3d_handle h, const spa3d_render* r, void* ws, int64_t ws_bytes, void* stream) {
  if (!h) return SPA3D_ERR_ARG;
  h->err.clear(); h->hip_err = 0;
  auto bad = [&](const std::string& m) { h->err = "render: " + m; return SPA3D_ERR_ARG; };
  if (!r) return bad("spa3d_render is required");
  if (r->N < 1 || r->T < 1) return bad("N = " + std::to_string(r->N) + ", T = " + std::to_string(r->T) + ": both must be positive");
  if (r->H < 1 || r->H > RP_MAX_DIM || r->W < 1 || r->W > RP_MAX_DIM)
    return bad("H = " + std::to_string(r->H) + ", W = " + std::to_string(r->W) + " are outside [1, " + std::to_string(RP_MAX_DIM) + "]");
  if (!r->tracks) return bad("tracks is required");
  if (r->coords != 2 && r->coords != 3) return bad("coords = " + std::to_string(r->coords) + " is neither 2 nor 3");
  if (r->coords == 3 && (!r->intrinsics || !r->extrinsics)) return bad("coords == 3 needs the camera matrices (intrinsics, extrinsics)");
  if (r->coords == 3 && (r->resize_h < 1 || r->resize_w < 1)) return bad("coords == 3 needs resize_h, resize_w >= 1");
  if (!r->out && !r->pixels) return bad("nothing to do: out and pixels are both NULL");
  if (r->out && (!r->video || !r->scores)) return bad("drawing needs video and scores");
  if (r->use_visibility && !r->visible) return bad("use_visibility needs visible");
  if (r->trail < 0 || r->trail > RP_MAX_TRAIL) return bad("trail = " + std::to_string(r->trail) + " is outside [0, " + std::to_string(RP_MAX_TRAIL) + "]");
  if (r->point_size < 0 || r->point_size > RP_MAX_RADIUS)
    return bad("point_size = " + std::to_string(r->point_size) + " is outside [0, " + std::to_string(RP_MAX_RADIUS) + "]");
  // a launch holds fewer than 2^32 threads: one thread per point-frame, 256 per (frame, tile)
  if ((int64_t)r->N * r->T > (int64_t)1 << 31) return bad("N x T = " + std::to_string((int64_t)r->N * r->T) + " point-frames exceed one launch (2^31)");
  if (r->out && (int64_t)r->T * ((r->W + 63) / 64) * ((r->H + 15) / 16) >= (int64_t)1 << 24) return bad("T x tiles reaches 2^24 workgroups: more than one launch holds");
  return sized_call(h, "render", render_need(h, r), ws, ws_bytes, stream, [&] { render_body(h, r); });
}

}  // extern "C"
