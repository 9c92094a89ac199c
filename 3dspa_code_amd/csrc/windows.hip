// windows.hip -- spa3d_stitch_windows (include/spa3d.h), the kernel first, the entry point below it: the per-window predictions and errors of a
// long clip (spa3d_build_windows cut it, spa3d_score_folds scored the windows) merged back onto the clip's own time axis.
// One wave per window row, lanes along the long time axis in chunks of 64 frames: a window's row is contiguous in t, so the lanes of a chunk
// read consecutive addresses of every window that covers it.  The windows that can cover a chunk are found once per chunk from the plan, which
// travels by value (scalar loads).  The arithmetic is window_row.hpp's, which the g++ host test runs too.
// Every output element is written exactly once, by the wave that owns its row (row_track is a permutation): no atomics, two runs give the
// same bytes.  fp32 only: compiled once.  Plain loads and stores.
#include "common.hpp"
#include "window_row.hpp"  // the plan, the weights and the blend (host- and device-callable)

struct StArgs {
  WrPlan p;
  const int32_t* row_track;
  const float* tracks; const float* vlog; const float* ferr;   // [W,N,Tw,NC] [W,N,Tw] [W,N,Tw]; each may be null
  float* otracks; float* ovlog; float* oferr; float* ospread;  // [N,TL,NC] [N,TL] [N,TL] [N,TL]; null = not wanted
  int32_t N, NC;
};

namespace SPA_NS {

// the blended point of (window row r, frame t) and its spread, to element o = n * TL + t of the outputs that are wanted
template <int NC> __device__ __forceinline__ void st_tracks(const StArgs& a, int wlo, int whi, int64_t r, int t, int64_t o) {
  float v[NC], s2 = 0.f;
  if (a.ospread) wr_point<NC>(a.p, wlo, whi, a.tracks, a.N, r, t, v, &s2);
  else wr_point<NC>(a.p, wlo, whi, a.tracks, a.N, r, t, v, nullptr);
  if (a.otracks) {
#pragma unroll
    for (int c = 0; c < NC; ++c) a.otracks[o * NC + c] = v[c];
  }
  if (a.ospread) a.ospread[o] = sqrtf(s2);
}

__global__ __launch_bounds__(256) void stitch_windows_kernel(const StArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int TL = a.p.TL, NC = a.NC;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < a.N; r += (int64_t)gridDim.x * 4) {
    const int64_t n = a.row_track ? (int64_t)a.row_track[r] : r;
    if (n < 0 || n >= a.N) continue;  // not a permutation entry: nothing is written out of bounds
    for (int tc = 0; tc < TL; tc += 64) {
      int wlo, whi;
      wr_window_range(a.p, tc, min(tc + 63, TL - 1), wlo, whi);
      const int t = tc + lane;
      if (t >= TL) continue;
      const int64_t o = n * TL + t;
      if (a.otracks || a.ospread) {
        if (NC == 3) st_tracks<3>(a, wlo, whi, r, t, o);
        else st_tracks<2>(a, wlo, whi, r, t, o);
      }
      if (a.ovlog) wr_point<1>(a.p, wlo, whi, a.vlog, a.N, r, t, a.ovlog + o, nullptr);
      if (a.oferr) wr_point<1>(a.p, wlo, whi, a.ferr, a.N, r, t, a.oferr + o, nullptr);
    }
  }
}

void k_stitch_windows(spa3d_ctx* c, const StArgs& a) {
  if (c->dry) return;
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(a.N, 4), (int64_t)1 << 20);
  stitch_windows_kernel<<<grid, 256, 0, c->stream>>>(a);
  SPA_LAUNCH_CHECK(c);
}

}  // namespace SPA_NS

// ---- the entry point ----
extern "C" {

int spa3d_stitch_windows(spa3d_handle h, const spa3d_stitch* s, void* stream) {
  if (!h) return SPA3D_ERR_ARG;
  h->err.clear(); h->hip_err = 0;
  auto bad = [&](const std::string& m) { h->err = "stitch_windows: " + m; return SPA3D_ERR_ARG; };
  if (!s) return bad("the spa3d_stitch block is required");
  if (s->W < 1 || s->W > WR_MAX_W) return bad("W = " + std::to_string(s->W) + " is outside [1, " + std::to_string(WR_MAX_W) + "]");
  if (s->N < 1 || s->N > (1 << 24)) return bad("N = " + std::to_string(s->N) + " is outside [1, 2^24]");
  if (s->Tw < 1 || s->Tw > (1 << 20)) return bad("Tw = " + std::to_string(s->Tw) + " is outside [1, 2^20]");
  if (s->TL < 1 || s->TL > (1 << 24)) return bad("TL = " + std::to_string(s->TL) + " is outside [1, 2^24]");
  if (s->NC != 2 && s->NC != 3) return bad("NC = " + std::to_string(s->NC) + " must be 2 or 3");
  if (s->blend != SPA3D_BLEND_MEAN && s->blend != SPA3D_BLEND_HAT && s->blend != SPA3D_BLEND_FIRST)
    return bad("blend = " + std::to_string(s->blend) + " is none of SPA3D_BLEND_MEAN, SPA3D_BLEND_HAT, SPA3D_BLEND_FIRST");
  if (!s->t0) return bad("t0 is required");
  if (!s->out_tracks && !s->out_visible_logits && !s->out_frame_err && !s->out_spread) return bad("no output is wanted");
  if (s->out_tracks && !s->tracks) return bad("out_tracks needs tracks");
  if (s->out_spread && !s->tracks) return bad("out_spread needs tracks");
  if (s->out_visible_logits && !s->visible_logits) return bad("out_visible_logits needs visible_logits");
  if (s->out_frame_err && !s->frame_err) return bad("out_frame_err needs frame_err");
  int where = 0;
  switch (wr_plan_check(s->W, s->Tw, s->TL, s->t0, s->len, &where)) {
    case WR_PLAN_START: return bad("t0[" + std::to_string(where) + "] = " + std::to_string(s->t0[where]) + " is outside [0, TL = " + std::to_string(s->TL) + ")");
    case WR_PLAN_ORDER: return bad("t0 must increase strictly (t0[" + std::to_string(where) + "] = " + std::to_string(s->t0[where]) + ")");
    case WR_PLAN_LEN:
      return bad("len[" + std::to_string(where) + "] = " + std::to_string(s->len ? s->len[where] : wr_window_len(s->t0[where], s->Tw, s->TL)) +
                 " is outside [1, Tw = " + std::to_string(s->Tw) + "] or runs past TL");
    case WR_PLAN_GAP: return bad("the windows leave a gap in [0, TL = " + std::to_string(s->TL) + ") (found at window " + std::to_string(where) + ")");
    default: break;
  }
  StArgs a{};
  a.p.W = s->W; a.p.Tw = s->Tw; a.p.TL = s->TL; a.p.blend = s->blend;
  for (int w = 0; w < s->W; ++w) { a.p.t0[w] = s->t0[w]; a.p.len[w] = s->len ? s->len[w] : wr_window_len(s->t0[w], s->Tw, s->TL); }
  a.row_track = s->row_track; a.tracks = s->tracks; a.vlog = s->visible_logits; a.ferr = s->frame_err;
  a.otracks = s->out_tracks; a.ovlog = s->out_visible_logits; a.oferr = s->out_frame_err; a.ospread = s->out_spread;
  a.N = s->N; a.NC = s->NC;
  h->stream = (hipStream_t)stream; h->dry = false;
  k_stitch_windows(h, a);
  return h->hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}

}  // extern "C"
