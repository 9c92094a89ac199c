// tapvid3d.hip -- spa3d_tapvid3d_from_preds and spa3d_op_median_rows (include/spa3d.h), kernels first, entry points below them: the TAPVid-3D metric counts of every query
// row, with the predictions rescaled by the sample's exact median of |gt| / |pred| or by the row's ratio at its query frame.
// The definitions are restated from the published definition (compute_tapvid3d_metrics of the tapnet package), parity unpinned; the frame
// arithmetic and the digit walk of the select live in tapvid3d_row.hpp, which the g++ host test runs too.  fp32 only: compiled once.
//
//   tv_ratio_kernel     one wave per query row: ratio of every frame (optional output) and the median's set (NaN outside {vis and ew})
//   median_rows_kernel  one workgroup per row of values: exact median by a 4-pass radix select, integer LDS atomics only
//   tv_rows_kernel      one wave per query row: the 24 counts, lanes striding over frames, xor butterfly, lanes 0..23 store
//   tv_reduce_kernel    one workgroup per (sample, slot): the sample's rows pooled in double in a fixed order
// No float atomics anywhere: the same inputs give the same bits on every run.
#include <algorithm>

#include "common.hpp"
#include "tapvid3d_row.hpp"  // TAPVid-3D metric counts of a row and the exact median select (host- and device-callable)

// The launches of spa3d_tapvid3d_from_preds share this block: the caller's whole tensors, indexed by the global query row, and the
// rows [row0, row0 + nq) a launch covers.  ratio / sel / row_scale / scale may be null (see each kernel).
struct TvArgs {
  const float* tracks; const float* vlog; const float* tgt; const float* tvis; const float* qpts; const float* intr;  // intr: device [B][4] or null
  const float* scale;          // rows pass, median scaling: device [B]
  float* ratio; float* sel;    // ratio pass: ratio [B * Q][T] of every frame; sel: the same with NaN outside {vis and ew} (the median's set)
  float* row_scale; float* qstats;
  int64_t nq, row0; int Q, T, scaling, fixed;
};

namespace SPA_NS {

__global__ __launch_bounds__(256) void tv_ratio_kernel(const TvArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.nq) return;
  const int64_t gr = a.row0 + r;
  const int T = a.T;
  const float* p = a.tracks + gr * T * 3;
  const float* g = a.tgt + gr * T * 3;
  const float* y = a.tvis + gr * T;
  const int tq = tv_query_frame(a.qpts[gr * 4], T);
  for (int t = lane; t < T; t += 64) {
    const float ratio = tv_ratio(p + (long)t * 3, g + (long)t * 3);
    if (a.ratio) a.ratio[gr * T + t] = ratio;
    if (a.sel) a.sel[gr * T + t] = (y[t] > 0.5f && t != tq) ? ratio : tv_nan();
  }
}
void k_tv_ratio(spa3d_ctx* c, const TvArgs& a) {
  if (c->dry || a.nq <= 0) return;
  tv_ratio_kernel<<<(unsigned)cdiv(a.nq, 4), 256, 0, c->stream>>>(a);
  SPA_LAUNCH_CHECK(c);
}

// out[row] = median of the non-NaN entries of x[row * stride + 0 .. n) (1 if there is none); entries >= 0.  Four passes over the row, each:
// clear the two 256-bin histograms, count the digit of every entry that carries a middle value's prefix (integer LDS atomics: the counts do
// not depend on the order of arrival), then one thread walks the histograms (tv_select_step).
constexpr int MEDIAN_THREADS = 1024;
__global__ __launch_bounds__(MEDIAN_THREADS) void median_rows_kernel(const float* __restrict__ x, int64_t stride, int64_t n, float* __restrict__ out) {
  __shared__ uint32_t hist[2][256];
  __shared__ TvSelect sel;
  const float* xr = x + (int64_t)blockIdx.x * stride;
  if (threadIdx.x == 0) tv_select_init(sel);
  for (int pass = 0; pass < 4; ++pass) {
    if (threadIdx.x < 512) hist[threadIdx.x >> 8][threadIdx.x & 255] = 0u;
    __syncthreads();
    const TvSelect s = sel;
    const bool shared = tv_select_shared(s);
    for (int64_t i = threadIdx.x; i < n; i += MEDIAN_THREADS) {
      const uint32_t u = tv_bits(xr[i]);
      if (tv_is_nan_bits(u)) continue;
      const uint32_t d = tv_select_digit(pass, u);
      if (tv_select_match(s, 0, pass, u)) atomicAdd(&hist[0][d], 1u);
      if (!shared && tv_select_match(s, 1, pass, u)) atomicAdd(&hist[1][d], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) tv_select_step(sel, hist[0], hist[1], pass);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = tv_select_result(sel);
}
void k_median_rows(spa3d_ctx* c, const float* x, int64_t rows, int64_t stride, int64_t n, float* out) {
  if (c->dry || rows <= 0) return;
  median_rows_kernel<<<(unsigned)rows, MEDIAN_THREADS, 0, c->stream>>>(x, stride, n, out);
  SPA_LAUNCH_CHECK(c);
}

__device__ __forceinline__ void tv_acc_xor(TvAcc& a, int o) {
  TvAcc b;
  b.n_ew = __shfl_xor(a.n_ew, o, 64); b.n_vis = __shfl_xor(a.n_vis, o, 64); b.occ = __shfl_xor(a.occ, o, 64); b.n_pv = __shfl_xor(a.n_pv, o, 64);
#pragma unroll
  for (int k = 0; k < TV_K; ++k) {
    b.w[k] = __shfl_xor(a.w[k], o, 64); b.tp[k] = __shfl_xor(a.tp[k], o, 64); b.fp[k] = __shfl_xor(a.fp[k], o, 64); b.fn[k] = __shfl_xor(a.fn[k], o, 64);
  }
  tv_acc_merge(a, b);
}
__global__ __launch_bounds__(256) void tv_rows_kernel(const TvArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.nq) return;  // whole waves leave: no shuffle partner is lost
  const int64_t gr = a.row0 + r, b = gr / a.Q;
  const int T = a.T;
  const float* p = a.tracks + gr * T * 3;
  const float* g = a.tgt + gr * T * 3;
  const float* lg = a.vlog + gr * T;
  const float* y = a.tvis + gr * T;
  const int tq = tv_query_frame(a.qpts[gr * 4], T);
  const float f = a.intr ? tv_focal(a.intr[b * 4], a.intr[b * 4 + 1]) : tv_focal(256.f, 256.f);
  float s = 1.f;  // wave-uniform
  if (a.scaling == TV_SCALE_MEDIAN) s = a.scale[b];
  else if (a.scaling == TV_SCALE_PER_TRAJECTORY) s = tv_ratio(p + (long)tq * 3, g + (long)tq * 3);
  TvAcc acc;
  tv_acc_init(acc);
  for (int t = lane; t < T; t += 64) tv_acc_frame(acc, p + (long)t * 3, g + (long)t * 3, lg[t], y[t], s, t != tq, f, a.fixed != 0);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tv_acc_xor(acc, o);
  if (lane < TV_S) a.qstats[gr * TV_S + lane] = tv_acc_slot(acc, lane);
  if (lane == 0 && a.row_scale) a.row_scale[gr] = s;
}
void k_tv_rows(spa3d_ctx* c, const TvArgs& a) {
  if (c->dry || a.nq <= 0) return;
  tv_rows_kernel<<<(unsigned)cdiv(a.nq, 4), 256, 0, c->stream>>>(a);
  SPA_LAUNCH_CHECK(c);
}

// sample_stats[b][s] (double) = the sample's Q rows of query_stats summed in a fixed order: thread i takes rows i, i + 256, ..., then a tree
// over the 256 partials (the form of score_reduce_kernel, every slot a sum).  Padded rows hold zeros.
__global__ __launch_bounds__(256) void tv_reduce_kernel(const float* __restrict__ qstats, int Q, double* __restrict__ out) {
  __shared__ double red[256];
  const int64_t b = blockIdx.x / TV_S; const int s = (int)(blockIdx.x - b * TV_S);
  const float* base = qstats + b * Q * TV_S + s;
  double v = 0.0;
  for (int q = threadIdx.x; q < Q; q += 256) v += (double)base[(int64_t)q * TV_S];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}
void k_tv_reduce(spa3d_ctx* c, const float* qstats, int64_t B, int Q, double* out) {
  if (c->dry || B <= 0) return;
  tv_reduce_kernel<<<(unsigned)(B * TV_S), 256, 0, c->stream>>>(qstats, Q, out);
  SPA_LAUNCH_CHECK(c);
}

__global__ __launch_bounds__(256) void tv_fill_kernel(float* __restrict__ p, int64_t n, float v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}
void k_tv_fill(spa3d_ctx* c, float* p, int64_t n, float v) {
  if (c->dry || n <= 0) return;
  tv_fill_kernel<<<(unsigned)cdiv(n, 256), 256, 0, c->stream>>>(p, n, v);
  SPA_LAUNCH_CHECK(c);
}

}  // namespace SPA_NS

// ---- the entry points ----
// The launches of one call.  Runs twice: dry (no launch, a counting arena: the workspace the call needs) and for real.  Workspace: the median's
// set [B * Q][T_out] (median scaling only) and the per-sample factors [B] when the caller does not ask for them.
static void tapvid3d_body(spa3d_ctx* c, const spa3d_batch* b, const spa3d_outputs* preds, const spa3d_tapvid3d* m, const int32_t* cq) {
  const int To = c->cfg.num_output_frames;
  const int64_t B = b->B, Q = b->Q;
  const bool median = m->scaling == SPA3D_SCALE_MEDIAN;
  TvArgs a{};
  a.tracks = preds->tracks; a.vlog = preds->visible_logits; a.tgt = b->query_tracks; a.tvis = b->query_tracks_visible; a.qpts = b->query_points;
  a.intr = m->intrinsics; a.ratio = m->ratio; a.row_scale = m->row_scale; a.qstats = m->query_stats;
  a.Q = b->Q; a.T = To; a.scaling = m->scaling; a.fixed = m->fixed_thresholds != 0;
  a.sel = median ? (float*)c->ar.alloc(B * Q * To * 4) : nullptr;
  float* scale = m->scale ? m->scale : (median ? (float*)c->ar.alloc(B * 4) : nullptr);
  a.scale = scale;
  // rows of padded queries (spa3d_set_counts): every result reads 0, their inputs are never read and they are not part of the median
  auto zero_padded = [&](int64_t r0, int64_t nr) {
    if (c->dry || nr <= 0) return;
    (void)hipMemsetAsync(m->query_stats + r0 * TV_S, 0, (size_t)(nr * TV_S) * 4, c->stream);
    if (m->row_scale) (void)hipMemsetAsync(m->row_scale + r0, 0, (size_t)nr * 4, c->stream);
    if (m->ratio) (void)hipMemsetAsync(m->ratio + r0 * To, 0, (size_t)(nr * To) * 4, c->stream);
  };
  if (a.ratio || a.sel) for_each_live_span(cq, B, Q, [&](int64_t row0, int64_t nq) { a.row0 = row0; a.nq = nq; k_tv_ratio(c, a); });
  if (median) {
    if (!cq) k_median_rows(c, a.sel, B, Q * To, Q * To, scale);
    else for (int64_t i = 0; i < B; ++i) k_median_rows(c, a.sel + i * Q * To, 1, Q * To, (int64_t)cq[i] * To, scale + i);
  } else if (scale) {
    k_tv_fill(c, scale, B, 1.f);
  }
  for_each_live_span(cq, B, Q, [&](int64_t row0, int64_t nq) { a.row0 = row0; a.nq = nq; k_tv_rows(c, a); });
  if (cq) for_each_live_span(cq, B, Q, [&](int64_t row0, int64_t nq) { zero_padded(row0 + nq, Q - nq); });
  if (m->sample_stats) k_tv_reduce(c, m->query_stats, B, b->Q, m->sample_stats);
}
static int64_t tapvid3d_need(spa3d_ctx* c, const spa3d_batch* b, const spa3d_outputs* preds, const spa3d_tapvid3d* m, const int32_t* cq) {
  return arena_peak(c, [&] { tapvid3d_body(c, b, preds, m, cq); }) + 256;  // never 0: a call without a workspace is refused after the walk, whatever the scaling
}

extern "C" {

int64_t spa3d_tapvid3d_workspace_bytes(spa3d_handle h, int32_t B, int32_t Q, int32_t T) {
  if (!h || B <= 0 || Q <= 0 || T <= 0) return -1;
  const int64_t To = std::max(T, h->cfg.num_output_frames);  // the largest need of any scaling: the median's set and the factors, each 256-byte aligned
  return (((int64_t)B * Q * To * 4 + 255) & ~int64_t(255)) + (((int64_t)B * 4 + 255) & ~int64_t(255)) + 256;
}
int spa3d_tapvid3d_from_preds(spa3d_handle h, const spa3d_batch* b, const spa3d_outputs* preds, spa3d_tapvid3d* m, void* ws, int64_t ws_bytes, void* stream) {
  if (!h) return SPA3D_ERR_ARG;
  h->err.clear(); h->hip_err = 0;
  if (h->cfg.model_kind == 1) { h->err = "tapvid3d: the 2-D model (model_kind 1) has no depth coordinate"; return SPA3D_ERR_ARG; }
  if (!b || !b->query_tracks || !b->query_tracks_visible) { h->err = "tapvid3d: the batch needs its targets (query_tracks, query_tracks_visible)"; return SPA3D_ERR_ARG; }
  if (!b->query_points) { h->err = "tapvid3d: the batch needs query_points (the query frame is left out of every count)"; return SPA3D_ERR_ARG; }
  if (!preds || !preds->tracks || !preds->visible_logits) { h->err = "tapvid3d: predictions (tracks, visible_logits) are required"; return SPA3D_ERR_ARG; }
  if (!m || !m->query_stats) { h->err = "tapvid3d: spa3d_tapvid3d::query_stats is required"; return SPA3D_ERR_ARG; }
  if (m->scaling < SPA3D_SCALE_NONE || m->scaling > SPA3D_SCALE_PER_TRAJECTORY) { h->err = "tapvid3d: scaling = " + std::to_string(m->scaling) + " is outside [0, 2]"; return SPA3D_ERR_ARG; }
  if (b->B <= 0 || b->Q <= 0) { h->err = "batch: B,Q must be positive"; return SPA3D_ERR_ARG; }
  const int32_t* cq = nullptr;
  if (h->has_cnt_q && !(cq = checked_query_counts(h, b->B, b->Q))) return SPA3D_ERR_ARG;
  return sized_call(h, "tapvid3d", tapvid3d_need(h, b, preds, m, cq), ws, ws_bytes, stream, [&] { tapvid3d_body(h, b, preds, m, cq); });
}

int spa3d_op_median_rows(const float* x, int64_t rows, int64_t n, float* out, void* ws, int64_t ws_bytes, void* stream) {
  (void)ws; (void)ws_bytes;  // the select needs no scratch: its histograms live in LDS
  if (!x || !out || rows <= 0 || rows > 0x7fffffff || n < 0) return SPA3D_ERR_ARG;
  spa3d_ctx c; c.stream = (hipStream_t)stream;
  k_median_rows(&c, x, rows, n, n, out);
  return c.hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}

}  // extern "C"
