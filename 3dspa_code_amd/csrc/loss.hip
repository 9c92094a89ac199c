// loss.hip -- everything between the head and the parameter update (gfx950): latent discretisation, the loss (forward, backward, from
// split predictions), per-track scores, the loss scale of the 16-bit backward, AdamW with its gradient-norm and skip guard, the
// Threefry uniform noise, and the det_grads flush and unit.  Sums over the batch are fixed-order or fixed-point: no float atomics.
// T in {float, bf16_t} storage, fp32 math.  References such as attention.py:49 are to the reference implementation's files.
#include <algorithm>

#include "common.hpp"

namespace SPA_NS {

// ---------------------------------------------------------------------------------------------
// D1: clip, discretise, fixed noise, straight-through (track_autoencoder_3d.py:251-260)
// out = l - (l - q)  (same op order as the reference);  clipmask = 1[-1<=raw<=1] for the backward
// ---------------------------------------------------------------------------------------------
__global__ void discretize_kernel(const float* __restrict__ lat, const float* __restrict__ noise, int disc, float* __restrict__ out,
                                  float* __restrict__ clipmask, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float raw = lat[i];
    float l = raw != raw ? raw : fminf(fmaxf(raw, -1.f), 1.f);   // jnp.clip keeps a NaN a NaN (fmaxf / fminf would return the bound): a diverged latent must show
    if (clipmask) clipmask[i] = raw != raw ? raw : ((raw >= -1.f && raw <= 1.f) ? 1.f : 0.f);   // ... in the backward as well (jnp.clip's gradient of NaN is NaN)
    if (disc) {
      float q = rintf(__fmul_rn(l, 128.f)) / 128.f;
      q = __fsub_rn(__fadd_rn(q, noise[i] / 128.f), 1.0f / 256.0f);
      l = __fsub_rn(l, __fsub_rn(l, q));
    }
    out[i] = l;
  }
}
void k_discretize(spa3d_ctx* c, const float* lat, const float* noise, int discretize, float* out, float* clipmask, int64_t n) {
  if (c->dry || n == 0) return;
  discretize_kernel<<<GRID1D(n, 256), 256, 0, c->stream>>>(lat, noise, discretize, out, clipmask, n); SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// D8 head split + compute_loss_3d (track_autoencoder_3d.py:289-301, train.py:96-129)
// head[q][c*T+t], c<3 coords (coordinate-major), c==3 visibility logit
// ---------------------------------------------------------------------------------------------
// The objective is configurable per handle (spa3d_loss_config, include/spa3d.h): position term L1 or Huber with per-axis weights, BCE with a
// positive-class weight, and an optional per-point weight plane w[q][t] addressed like the visibility targets (null = 1).  The arithmetic of
// one point is loss_point.hpp; the numerators are P = sum w y e and V = sum w v, the denominator stays the unweighted visible count.
// (The axis weight is picked by selects: indexing the by-value argument with a per-thread index would move it to scratch memory.)
__device__ __forceinline__ float loss_axis(const spa3d_loss_config& lc, int c) { return c == 0 ? lc.axis_weight[0] : (c == 1 ? lc.axis_weight[1] : lc.axis_weight[2]); }
// The loss numerators and the visible count are summed over the whole batch by thousands of workgroups.  Float atomics make that sum depend
// on arrival order (the same batch gave 14089.21875 and 14089.216796875 in round 3), so two data-parallel replicas could log different
// losses and a test could not ask for bit-equal reruns.  Each workgroup reduces in a fixed order and adds its partial as a 64-bit FIXED-POINT
// integer (2^-24 units: exact, order-independent integer addition; quantisation 6e-8 per workgroup, far below fp32 resolution of the sums).
// Layout of the 10-float `sums` block: three 64-bit accumulators {position numerator, bce numerator, visible count} | denominator | loss scale | flag word.
// A partial that is not finite or beyond the fixed-point range sets a STICKY flag word (atomicOr) next to the accumulators and adds nothing; the sums then read as
// NaN.  (Round 4 added a marker value to the accumulator itself: k marked workgroups sum to k * 2^62 mod 2^64 = 0 for 4 | k, so a fully diverged forward reported loss 0.)
constexpr float LOSS_FIX = 16777216.f;                 // 2^24
__device__ __forceinline__ void loss_acc_add(unsigned long long* acc, unsigned* poison, float partial) {
  const float f = partial * LOSS_FIX;
  if (fabsf(f) < 1.0e15f) atomicAdd(acc, (unsigned long long)__float2ll_rn(f));   // NaN fails the comparison too
  else atomicOr(poison, 1u);
}
__device__ __forceinline__ float loss_acc_read(const unsigned long long* acc, const unsigned* poison) {
  if (*poison) return __int_as_float(0x7fc00000);
  return (float)((double)(long long)*acc * (1.0 / 16777216.0));
}
__global__ __launch_bounds__(256) void head_loss_fwd_kernel(const float* __restrict__ head, int64_t nq, int T_, const float* __restrict__ tgt,
                                                            const float* __restrict__ tvis, float* __restrict__ tracks,
                                                            float* __restrict__ vlog, float* __restrict__ clog, float* __restrict__ sums, unsigned* poison, int NC,
                                                            const spa3d_loss_config lc, const float* __restrict__ wgt) {
  // head row: NC coordinate blocks of T, then the visibility logits; the 2-D model (NC == 2) has a 4th block: certainty logits
  __shared__ float red[3][4];
  float pn = 0.f, bn = 0.f;
  const int64_t n = nq * T_;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int64_t q = i / T_; int t = (int)(i - q * T_);
    const float* hr = head + q * 4 * T_;
    const float lg = hr[NC * T_ + t];
    float perr = 0.f;
    for (int cdx = 0; cdx < NC; ++cdx) {
      const float pv = hr[cdx * T_ + t];
      if (tracks) tracks[i * NC + cdx] = pv;
      if (tgt) perr += loss_axis(lc, cdx) * loss_pos_value(lc.position_kind, lc.huber_delta, pv - tgt[i * NC + cdx]);
    }
    if (vlog) vlog[i] = lg;
    if (clog) clog[i] = NC == 2 ? hr[3 * T_ + t] : 0.f;  // 3DSPA: certain_logits = zeros (3d:301); TRAJAN: real head (ta:344)
    if (tgt) {
      const float y = tvis[i], w = wgt ? wgt[i] : 1.f;
      pn += perr * y * w;
      bn += loss_vis_value(lc.bce_pos_weight, y, lg) * w;
    }
  }
  if (!tgt) return;
  pn = wave_sum(pn); bn = wave_sum(bn);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = pn; red[1][w] = bn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    loss_acc_add((unsigned long long*)sums + 0, poison, red[0][0] + red[0][1] + red[0][2] + red[0][3]);
    loss_acc_add((unsigned long long*)sums + 1, poison, red[1][0] + red[1][1] + red[1][2] + red[1][3]);
  }
}
void k_loss_fwd(spa3d_ctx* c, const float* head, int64_t nq, int T_, const float* tgt, const float* tvis, float* tracks, float* vlog,
                float* clog, float* sums, unsigned* poison, int NC, const spa3d_loss_config& lc, const float* wgt) {
  if (c->dry || nq == 0) return;
  unsigned g = (unsigned)std::min<int64_t>(cdiv(nq * T_, 256), 4096);
  head_loss_fwd_kernel<<<g, 256, 0, c->stream>>>(head, nq, T_, tgt, tvis, tracks, vlog, clog, sums, poison, NC, lc, wgt);
  SPA_LAUNCH_CHECK(c);
}
// same numerators from already-split predictions (spa3d_loss entry point)
__global__ __launch_bounds__(256) void loss_from_preds_kernel(const float* __restrict__ tracks, const float* __restrict__ vlog, int64_t n,
                                                              const float* __restrict__ tgt, const float* __restrict__ tvis, float* sums, unsigned* poison, int NC,
                                                              const spa3d_loss_config lc, const float* __restrict__ wgt) {
  __shared__ float red[2][4];
  float pn = 0.f, bn = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float y = tvis[i], lg = vlog[i], w = wgt ? wgt[i] : 1.f;
    float perr = 0.f;
    for (int cdx = 0; cdx < NC; ++cdx) perr += loss_axis(lc, cdx) * loss_pos_value(lc.position_kind, lc.huber_delta, tracks[i * NC + cdx] - tgt[i * NC + cdx]);
    pn += perr * y * w;
    bn += loss_vis_value(lc.bce_pos_weight, y, lg) * w;
  }
  pn = wave_sum(pn); bn = wave_sum(bn);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = pn; red[1][w] = bn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    loss_acc_add((unsigned long long*)sums + 0, poison, red[0][0] + red[0][1] + red[0][2] + red[0][3]);
    loss_acc_add((unsigned long long*)sums + 1, poison, red[1][0] + red[1][1] + red[1][2] + red[1][3]);
  }
}
void k_loss_from_preds(spa3d_ctx* c, const float* tracks, const float* vlog, int64_t n, const float* tgt, const float* tvis, float* sums,
                       unsigned* poison, int NC, const spa3d_loss_config& lc, const float* wgt) {
  if (c->dry || n == 0) return;
  unsigned g = (unsigned)std::min<int64_t>(cdiv(n, 256), 4096);
  loss_from_preds_kernel<<<g, 256, 0, c->stream>>>(tracks, vlog, n, tgt, tvis, sums, poison, NC, lc, wgt);
  SPA_LAUNCH_CHECK(c);
}
// ---------------------------------------------------------------------------------------------
// Per-track scores (spa3d_score / spa3d_score_from_preds; arithmetic and summation order: score_row.hpp)
// One wave per query row, four rows per workgroup.  Lanes stride over the frames: in the head form every coordinate block of the row is read
// coalesced, in the split form a wave reads the row's contiguous [T][NC] span.  The row's sums are merged by the xor butterfly, so every lane
// ends with the same bits, and lanes 0 .. S-1 store one stat each.  No atomics: the same inputs give the same bits on every run, and the two
// input forms run the same instructions on the same values.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void score_acc_xor(ScoreAcc& a, int o, int K) {
  ScoreAcc b;
  b.n_vis = __shfl_xor(a.n_vis, o, 64); b.s_e1 = __shfl_xor(a.s_e1, o, 64); b.s_e2 = __shfl_xor(a.s_e2, o, 64); b.mx = __shfl_xor(a.mx, o, 64);
  b.bce = __shfl_xor(a.bce, o, 64); b.occ = __shfl_xor(a.occ, o, 64); b.n_pv = __shfl_xor(a.n_pv, o, 64);
#pragma unroll
  for (int k = 0; k < SCORE_MAX_K; ++k) {
    if (k < K) {  // wave-uniform
      b.w[k] = __shfl_xor(a.w[k], o, 64); b.tp[k] = __shfl_xor(a.tp[k], o, 64); b.fp[k] = __shfl_xor(a.fp[k], o, 64); b.fn[k] = __shfl_xor(a.fn[k], o, 64);
    } else {
      b.w[k] = b.tp[k] = b.fp[k] = b.fn[k] = 0.f;
    }
  }
  score_acc_merge(a, b, K);
}
__global__ __launch_bounds__(256) void score_rows_kernel(const ScoreArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.nq) return;  // whole waves leave: no shuffle partner is lost
  const int64_t gr = a.row0 + r;
  const int T = a.T, NC = a.NC;
  const ScoreThr thr = score_thr_scaled(a.thr, a.scale ? a.scale[gr / a.Q] : 1.f);
  const float *p, *lg; long sp, st;  // sp: stride between the coordinates of a frame, st: between frames
  if (a.head) { p = a.head + r * 4 * T; lg = p + (int64_t)NC * T; sp = T; st = 1; }
  else { p = a.tracks + gr * T * NC; lg = a.vlog + gr * T; sp = 1; st = NC; }
  const float* g = a.tgt + gr * T * NC;
  const float* y = a.tvis + gr * T;
  ScoreAcc acc;
  score_acc_init(acc);
  for (int t = lane; t < T; t += 64) {
    const float e2 = score_acc_frame(acc, p + (long)t * st, sp, g + (long)t * NC, 1, NC, lg[t], y[t], thr);
    if (a.frame_err) a.frame_err[gr * T + t] = e2;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) score_acc_xor(acc, o, thr.K);
  const int S = score_row_len(thr.K);
  if (lane < S) a.qstats[gr * S + lane] = score_acc_slot(acc, lane, T);
}
void k_score_rows(spa3d_ctx* c, const ScoreArgs& a) {
  if (c->dry || a.nq <= 0) return;
  score_rows_kernel<<<(unsigned)cdiv(a.nq, 4), 256, 0, c->stream>>>(a);
  SPA_LAUNCH_CHECK(c);
}
// sample_stats[b][s] (double) = the sample's Q rows of query_stats reduced in a fixed order: thread i takes rows i, i + 256, ..., then a tree
// over the 256 partials.  Slot 3 is a max; padded rows hold zeros and add nothing.  One workgroup per (sample, stat).
__global__ __launch_bounds__(256) void score_reduce_kernel(const float* __restrict__ qstats, int Q, int S, double* __restrict__ out) {
  __shared__ double red[256];
  const int64_t b = blockIdx.x / S; const int s = (int)(blockIdx.x - b * S);
  const float* base = qstats + b * Q * S + s;
  const bool is_max = s == 3;
  double v = 0.0;
  for (int q = threadIdx.x; q < Q; q += 256) {
    const double x = (double)base[(int64_t)q * S];
    v = is_max ? (x > v ? x : v) : v + x;
  }
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double x = red[threadIdx.x + o], w = red[threadIdx.x];
      red[threadIdx.x] = is_max ? (x > w ? x : w) : w + x;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}
void k_score_reduce(spa3d_ctx* c, const float* qstats, int64_t B, int Q, int K, double* out) {
  if (c->dry || B <= 0) return;
  const int S = score_row_len(K);
  score_reduce_kernel<<<(unsigned)(B * S), 256, 0, c->stream>>>(qstats, Q, S, out);
  SPA_LAUNCH_CHECK(c);
}

__global__ __launch_bounds__(256) void vis_count_kernel(const float* __restrict__ v, int64_t n, float* out, unsigned* poison) {
  __shared__ float red[4];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s += v[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss_acc_add((unsigned long long*)out, poison, red[0] + red[1] + red[2] + red[3]);
}
void k_vis_count(spa3d_ctx* c, const float* tvis, int64_t n, float* out, unsigned* poison) {
  if (c->dry || n == 0) return;
  unsigned g = (unsigned)std::min<int64_t>(cdiv(n, 256), 1024);
  vis_count_kernel<<<g, 256, 0, c->stream>>>(tvis, n, out, poison); SPA_LAUNCH_CHECK(c);
}
// sums = {pos_num, bce_num, vis_cnt} (fixed-point accumulators, see loss_acc_add); denom_dev = denom_host>0 ? denom_host : max(vis_cnt,1)
__global__ void set_denom_kernel(const float* sums, const unsigned* poison, float denom_host, float* denom_dev) {
  *denom_dev = denom_host > 0.f ? denom_host : fmaxf(loss_acc_read((const unsigned long long*)sums + 2, poison), 1.f);  // fmaxf(NaN, 1) = 1: the numerators carry the NaN
}
void k_set_denom(spa3d_ctx* c, const float* sums, const unsigned* poison, float denom_host, float* denom_dev) {
  if (c->dry) return;
  set_denom_kernel<<<1, 1, 0, c->stream>>>(sums, poison, denom_host, denom_dev); SPA_LAUNCH_CHECK(c);
}
__global__ void loss_finalize_kernel(const float* sums, const unsigned* poison, const float* denom_dev, float l1w, float bcew, float* loss3) {
  float d = *denom_dev;
  float pos = loss_acc_read((const unsigned long long*)sums + 0, poison) / d, vis = loss_acc_read((const unsigned long long*)sums + 1, poison) / d;
  loss3[0] = l1w * pos + bcew * vis; loss3[1] = pos; loss3[2] = vis;
}
void k_loss_finalize(spa3d_ctx* c, const float* sums, const unsigned* poison, const float* denom_dev, float l1w, float bcew, float* loss3) {
  if (c->dry) return;
  loss_finalize_kernel<<<1, 1, 0, c->stream>>>(sums, poison, denom_dev, l1w, bcew, loss3); SPA_LAUNCH_CHECK(c);
}
// d head (include/spa3d.h "Head cotangent"): l1w * w * y * a_c * rho'(pred - tgt) / denom ; bcew * w * v'(l) / denom.
// Default configuration, no weight plane: l1w*sign(pred-tgt)*vis/denom ; bcew*(sigmoid(l)-y)/denom ; sign(0)=0, in that order of operations.
template <typename T>
__global__ void loss_bwd_kernel(const float* __restrict__ head, int64_t nq, int T_, const float* __restrict__ tgt,
                                const float* __restrict__ tvis, const float* __restrict__ denom_dev, const spa3d_loss_config lc,
                                const float* __restrict__ wgt, T* __restrict__ dhead, int NC, const float* __restrict__ scale_dev) {
  const float inv = (scale_dev ? *scale_dev : 1.f) / *denom_dev;  // scale_dev: the fp16 mode's loss scale (a power of two)
  const int64_t n = nq * 4 * T_;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int64_t q = i / (4 * T_); int j = (int)(i - q * 4 * T_);
    int cc = j / T_, t = j - cc * T_;
    float y = tvis[q * T_ + t], g;
    const float w = (wgt && cc <= NC) ? wgt[q * T_ + t] : 1.f;
    if (cc < NC) {
      float df = head[i] - tgt[(q * T_ + t) * NC + cc];
      g = lc.l1_weight * (loss_axis(lc, cc) * loss_pos_deriv(lc.position_kind, lc.huber_delta, df)) * y * w * inv;
    } else if (cc == NC) {
      float l = head[i];
      g = lc.bce_weight * loss_vis_deriv(lc.bce_pos_weight, y, l) * w * inv;
    } else {
      g = 0.f;  // TRAJAN's certainty head carries no loss term in compute_loss_2d (train.py:60-93)
    }
    st(dhead + i, g);
  }
}
template <typename T>
void k_loss_bwd(spa3d_ctx* c, const float* head, int64_t nq, int T_, const float* tgt, const float* tvis, const float* denom_dev,
                const spa3d_loss_config& lc, const float* wgt, T* dhead, int NC, const float* scale_dev) {
  if (c->dry || nq == 0) return;
  loss_bwd_kernel<T><<<GRID1D(nq * 4 * T_, 256), 256, 0, c->stream>>>(head, nq, T_, tgt, tvis, denom_dev, lc, wgt, dhead, NC, scale_dev);
  SPA_LAUNCH_CHECK(c);
}
// Loss scale of the 16-bit backward (fp16 mode).  setting > 0: that value.  setting < 0: automatic -- the largest power of two that keeps
// the head gradient's magnitude gmax / denom at or below |setting| (16; gmax = the configured objective's largest head gradient per unit
// point weight, spa3d_loss_config: 5000 by default): activations' gradients then sit mid-range in fp16 for any batch
// size (at BASELINE cfg#3, denom = 4.4 M: 8192; a 100-element toy batch: 1).
// `state` (may be null): the caller's dynamic-scale state, state[0] = a power-of-two multiplier in (0, 1] that spa3d_adamw_step halves after
// a step with a non-finite gradient norm and grows back after 200 finite ones (0 or garbage-free zero memory = 1).
__global__ void set_loss_scale_kernel(const float* __restrict__ denom_dev, float gmax, float setting, const float* __restrict__ state,
                                      float* __restrict__ scale_dev) {
  float s = setting;
  if (setting < 0.f) s = fminf(fmaxf(exp2f(floorf(log2f(*denom_dev * (-setting) / gmax))), 1.f), 16777216.f);
  if (state) { const float m = state[0]; if (m > 0.f && m < 1.f) s = fmaxf(s * m, 5.9604645e-8f); }
  *scale_dev = s;
}
void k_set_loss_scale(spa3d_ctx* c, const float* denom_dev, float gmax, float setting, float* scale_dev) {
  if (c->dry) return;
  set_loss_scale_kernel<<<1, 1, 0, c->stream>>>(denom_dev, gmax, setting, c->loss_scale_state, scale_dev); SPA_LAUNCH_CHECK(c);
}
__global__ void unscale_kernel(float* __restrict__ a, const float* __restrict__ scale_dev, int64_t n) {
  const float s = 1.f / *scale_dev;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) a[i] *= s;
}
void k_unscale(spa3d_ctx* c, float* a, const float* scale_dev, int64_t n) {
  if (c->dry || n == 0) return;
  unscale_kernel<<<GRID1D(n, 256), 256, 0, c->stream>>>(a, scale_dev, n); SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// optimizer: clip_by_global_norm -> adamw -> apply_updates on flat buffers (train.py:239-242)
// ---------------------------------------------------------------------------------------------
// Global gradient norm, reproducible: every workgroup writes ITS partial sum of squares to scratch[SUMSQ_OFF + block] (fixed thread -> element
// map, fixed reduction tree) and adamw_guard_kernel adds the partials in index order.  A float atomicAdd here made the clip factor -- and so the
// whole AdamW update -- depend on arrival order: two data-parallel replicas holding bit-identical reduced gradients could drift apart.
constexpr int SUMSQ_MAXB = 512, SUMSQ_OFF = 256;  // partials live in floats [256, 768) of the >= 4 KiB scratch block
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, int64_t n, float* partial) {
  __shared__ float red[4];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s += g[i] * g[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t n, float lr, float tstep, float clip, float b1,
                                                    float b2, float eps, float wd, float* scratch) {
  // bias correction at the number of updates actually APPLIED: calls so far (tstep = step + 1) minus the steps skipped before this one
  // (scratch[3]; this kernel returns early when this step itself is skipped).  -expm1(t log b) keeps 1 - b^t accurate for b -> 1.
  const float teff = fmaxf(tstep - scratch[3], 1.f);
  const float bc1 = -expm1f(teff * logf(b1)), bc2 = -expm1f(teff * logf(b2));
  const float gn = sqrtf(scratch[1]);
  const float sc = gn < clip ? 1.f : clip / gn;
  if (blockIdx.x == 0 && threadIdx.x == 0) scratch[0] = gn;
  if (!(gn <= 3.0e38f)) return;  // inf / NaN gradient (an fp16 overflow): parameters and both moments stay as they are (adamw_guard_kernel reports it)
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float gi = g[i] * sc;
    float mi = b1 * m[i] + (1.f - b1) * gi;
    float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    float mh = mi / bc1, vh = vi / bc2;
    float pi = p[i];
    p[i] = pi - lr * (mh / (sqrtf(vh) + eps) + wd * pi);
  }
}
// scratch[2] := 1 if this step was skipped (non-finite gradient norm) else 0; scratch[3] += skipped steps; scratch[4] = dynamic loss-scale
// multiplier (0 = 1; halved on a skip, doubled up to 1 after 200 finite steps counted in scratch[5]) -- read by set_loss_scale_kernel when the
// caller registered it with spa3d_set_loss_scale_state.
__global__ __launch_bounds__(256) void adamw_guard_kernel(float* scratch, int nblocks) {
  __shared__ float red[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < nblocks; i += 256) s += scratch[SUMSQ_OFF + i];  // fixed order: thread t takes partials t, t + 256
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x != 0) return;
  scratch[1] = red[0];
  const bool bad = !(sqrtf(scratch[1]) <= 3.0e38f);
  scratch[2] = bad ? 1.f : 0.f;
  // the dynamic loss-scale multiplier must be a power of two in [2^-24, 1]; anything else (uninitialised scratch of a caller written against
  // the old contract, a stray value in (0,1]) reads as 1
  float m = scratch[4]; { int e; if (!(m >= 5.9604645e-8f && m <= 1.f && frexpf(m, &e) == 0.5f)) m = 1.f; }
  if (bad) { scratch[3] += 1.f; m = fmaxf(m * 0.5f, 5.9604645e-8f); scratch[5] = 0.f; }
  else if (m < 1.f) { scratch[5] += 1.f; if (scratch[5] >= 200.f) { m = fminf(2.f * m, 1.f); scratch[5] = 0.f; } }
  scratch[4] = m;
}
void k_adamw(spa3d_ctx* c, float* p, const float* g, float* m, float* v, int64_t n, float lr, int64_t step, float clip, float b1, float b2,
             float eps, float wd, float* scratch) {
  (void)hipMemsetAsync(scratch, 0, 12, c->stream);
  unsigned gr = (unsigned)std::min<int64_t>(cdiv(n, 256), 4096);
  const unsigned gs = (unsigned)std::min<int64_t>(cdiv(n, 256), SUMSQ_MAXB);
  sumsq_kernel<<<gs, 256, 0, c->stream>>>(g, n, scratch + SUMSQ_OFF);
  adamw_guard_kernel<<<1, 256, 0, c->stream>>>(scratch, (int)gs);
  adamw_kernel<<<gr, 256, 0, c->stream>>>(p, g, m, v, n, lr, (float)(step + 1), clip, b1, b2, eps, wd, scratch);
  SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// grouped AdamW + weight EMA (spa3d_adamw_step_groups, include/spa3d.h): the same three stages -- partial sums of squares, guard, update --
// with a table of ranges that scale the learning rate and the weight decay or freeze their elements (adamw_groups.hpp), and an optional
// exponential moving average of the new parameters written in the same pass.  The arithmetic of one element is adamw_point.hpp.
// ---------------------------------------------------------------------------------------------
// The table reaches the device BY VALUE in launch arguments, 160 ranges per launch, as k_set_i32 moves host offsets: no host-to-device copy,
// nothing borrowed from the caller once the call has returned.
constexpr int GROUPS_PER_LAUNCH = 160;
struct GroupWords { int32_t v[GROUPS_PER_LAUNCH * ADAMW_GROUP_WORDS]; };
__global__ __launch_bounds__(256) void set_groups_kernel(int32_t* __restrict__ dst, const GroupWords a, int nwords) {
  for (int i = threadIdx.x; i < nwords; i += 256) dst[i] = a.v[i];
}
// What a workgroup knows about the run of elements [t0, t1) it is about to process, found ONCE for the run: k = the first range that ends beyond
// t0, and, when one range covers the whole run or the run lies in a gap, the run's multipliers.  k is reached by walking forward from `k0` (any range
// index not beyond it: the result of adamw_group_find, or the k of an earlier run) through loads every lane shares.  A run that a range boundary cuts
// is not uniform: each of its elements walks forward from k on its own (adamw_group_at).
struct GroupRun { int k; bool uniform; float lr_scale, wd_scale; };
__device__ __forceinline__ GroupRun group_run(const AdamwGroup* __restrict__ tab, int num, int k0, int64_t t0, int64_t t1) {
  GroupRun r; r.uniform = true; r.lr_scale = 1.f; r.wd_scale = 1.f;
  r.k = k0;
  while (r.k < num && tab[r.k].end <= t0) ++r.k;
  if (r.k < num) {
    const int64_t b = tab[r.k].begin, e = tab[r.k].end;
    if (b <= t0 && e >= t1) { r.lr_scale = tab[r.k].lr_scale; r.wd_scale = tab[r.k].wd_scale; }
    else if (b < t1) r.uniform = false;   // (b >= t1: the whole run lies in the gap before range k)
  }
  return r;
}
// sumsq_kernel with the frozen elements left out: the same thread -> element map, the same tree, the same partial layout, and a frozen element adds
// +0.f -- its gradient is not even loaded, so a NaN or an inf there cannot reach the norm.  (The running sum is a sum of squares from +0.f: adding +0.f
// and not adding are the same bits.)  The map makes a workgroup's runs of 256 elements lie gridDim.x * 256 apart, so each run searches the table afresh.
// The host passes num = 0 for a table that freezes nothing.  Then every element counts, and the map's one 4-byte load per thread and round -- at most
// 512 workgroups, so 2 KiB in flight per CU -- is issued SUMSQ_AHEAD rounds at a time before the squares are added in the order of sumsq_kernel: the same
// bits at 16 times the loads in flight.
constexpr int SUMSQ_AHEAD = 16;
__global__ __launch_bounds__(256) void sumsq_groups_kernel(const float* __restrict__ g, int64_t n, const AdamwGroup* __restrict__ tab, int num,
                                                           float* partial) {
  __shared__ float red[4];
  float s = 0.f;
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t base = (int64_t)blockIdx.x * 256;
  if (num == 0) {
    for (; base + (SUMSQ_AHEAD - 1) * stride + 256 <= n; base += SUMSQ_AHEAD * stride) {   // SUMSQ_AHEAD whole runs
      float x[SUMSQ_AHEAD];
#pragma unroll
      for (int u = 0; u < SUMSQ_AHEAD; ++u) x[u] = g[base + u * stride + threadIdx.x];
#pragma unroll
      for (int u = 0; u < SUMSQ_AHEAD; ++u) s += x[u] * x[u];
    }
  }
  for (; base < n; base += stride) {
    const GroupRun r = group_run(tab, num, adamw_group_find(tab, num, base), base, std::min<int64_t>(base + 256, n));
    const int64_t i = base + threadIdx.x;
    if (i >= n) continue;
    float ls = r.lr_scale, ws = r.wd_scale;
    if (!r.uniform) { int k = r.k; adamw_group_at(tab, num, k, i, ls, ws); }
    if (ls != 0.f) s += g[i] * g[i];
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
struct AdamwGroupsArgs {
  float* p; const float* g; float* m; float* v; float* ema;
  int64_t n, head, nvec;   // elements [head, head + 4 nvec) are read and written 16 bytes at a time; what lies before and behind, one by one
  float lr, tstep, clip, b1, b2, eps, wd, ema_d, ema_omd;
  float* scratch;
};
template <bool EMA>
__device__ __forceinline__ void adamw_groups_one(const AdamwGroupsArgs& a, const AdamwCoef& c, int64_t i, float ls, float ws) {
  if (ls == 0.f) return;   // frozen: nothing is read, nothing is written
  float mi = a.m[i], vi = a.v[i];
  const float ei = EMA ? a.ema[i] : 0.f;
  const float pn = adamw_point(c, a.lr * ls, a.wd * ws, a.p[i], a.g[i], mi, vi);
  a.m[i] = mi; a.v[i] = vi; a.p[i] = pn;
  if (EMA) a.ema[i] = adamw_ema_point(ei, a.ema_d, a.ema_omd, pn);
}
// The runs of `len` elements that tile [s0, s1) are dealt out in contiguous blocks, workgroup b taking runs [b * per, (b + 1) * per): its runs ascend
// and adjoin, so the table is searched once and walked from there.  first / last = this workgroup's runs.
__device__ __forceinline__ void group_block_of_runs(int64_t s0, int64_t s1, int len, int64_t& first, int64_t& last) {
  const int64_t runs = (s1 - s0 + len - 1) / len, per = (runs + gridDim.x - 1) / gridDim.x;
  first = std::min<int64_t>((int64_t)blockIdx.x * per, runs); last = std::min<int64_t>(first + per, runs);
}
// elements [s0, s1) one at a time, in runs of 256
template <bool EMA>
__device__ __forceinline__ void adamw_groups_span(const AdamwGroupsArgs& a, const AdamwCoef& c, const AdamwGroup* __restrict__ tab, int num, int64_t s0, int64_t s1) {
  int64_t first, last;
  group_block_of_runs(s0, s1, 256, first, last);
  if (first >= last) return;
  int k = adamw_group_find(tab, num, s0 + first * 256);
  for (int64_t t = first; t < last; ++t) {
    const int64_t base = s0 + t * 256;
    const GroupRun r = group_run(tab, num, k, base, std::min<int64_t>(base + 256, s1));
    k = r.k;
    const int64_t i = base + threadIdx.x;
    if (i >= s1) continue;
    float ls = r.lr_scale, ws = r.wd_scale;
    if (!r.uniform) { int kk = r.k; adamw_group_at(tab, num, kk, i, ls, ws); }
    adamw_groups_one<EMA>(a, c, i, ls, ws);
  }
}
// The update: 28 bytes of traffic per element (36 with the EMA), no reuse -- a streaming pass.  A workgroup takes runs of 1024 elements, four per
// thread in one 16-byte load and store per stream; a run that one range covers (or none touches) resolves its multipliers once, a frozen run is
// skipped without a load, and a run that a range boundary cuts goes element by element through the same adamw_point.  Plain stores, no atomics:
// every element is written by one thread, from values that do not depend on the launch geometry.
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_groups_kernel(const AdamwGroupsArgs a, const AdamwGroup* __restrict__ tab, int num) {
  // (the prologue of adamw_kernel, expression for expression: the two must agree bit for bit)
  const float teff = fmaxf(a.tstep - a.scratch[3], 1.f);
  AdamwCoef c;
  c.b1 = a.b1; c.b2 = a.b2; c.eps = a.eps;
  c.bc1 = adamw_bias_correction(teff, a.b1); c.bc2 = adamw_bias_correction(teff, a.b2);
  const float gn = sqrtf(a.scratch[1]);
  c.sc = gn < a.clip ? 1.f : a.clip / gn;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.scratch[0] = gn;
  if (!(gn <= 3.0e38f)) return;  // non-finite norm over the live elements: the step is skipped, nothing but the scratch words is written
  const int64_t vend = a.head + 4 * a.nvec;
  int64_t first, last;
  group_block_of_runs(a.head, vend, 1024, first, last);
  int k = first < last ? adamw_group_find(tab, num, a.head + first * 1024) : 0;
  for (int64_t t = first; t < last; ++t) {
    const int64_t t0 = a.head + t * 1024;
    const GroupRun r = group_run(tab, num, k, t0, std::min<int64_t>(t0 + 1024, vend));
    k = r.k;
    const int64_t i = t0 + 4 * (int64_t)threadIdx.x;
    if (i >= vend) continue;
    if (!r.uniform) {
      int kk = r.k;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float ls, ws;
        adamw_group_at(tab, num, kk, i + j, ls, ws);
        adamw_groups_one<EMA>(a, c, i + j, ls, ws);
      }
      continue;
    }
    if (r.lr_scale == 0.f) continue;
    const float lr_g = a.lr * r.lr_scale, wd_g = a.wd * r.wd_scale;
    const float4 p4 = *reinterpret_cast<const float4*>(a.p + i), g4 = *reinterpret_cast<const float4*>(a.g + i);
    float4 m4 = *reinterpret_cast<const float4*>(a.m + i), v4 = *reinterpret_cast<const float4*>(a.v + i);
    float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (EMA) e4 = *reinterpret_cast<const float4*>(a.ema + i);
    float4 o4;
    o4.x = adamw_point(c, lr_g, wd_g, p4.x, g4.x, m4.x, v4.x);
    o4.y = adamw_point(c, lr_g, wd_g, p4.y, g4.y, m4.y, v4.y);
    o4.z = adamw_point(c, lr_g, wd_g, p4.z, g4.z, m4.z, v4.z);
    o4.w = adamw_point(c, lr_g, wd_g, p4.w, g4.w, m4.w, v4.w);
    *reinterpret_cast<float4*>(a.m + i) = m4; *reinterpret_cast<float4*>(a.v + i) = v4; *reinterpret_cast<float4*>(a.p + i) = o4;
    if (EMA) {
      e4.x = adamw_ema_point(e4.x, a.ema_d, a.ema_omd, o4.x); e4.y = adamw_ema_point(e4.y, a.ema_d, a.ema_omd, o4.y);
      e4.z = adamw_ema_point(e4.z, a.ema_d, a.ema_omd, o4.z); e4.w = adamw_ema_point(e4.w, a.ema_d, a.ema_omd, o4.w);
      *reinterpret_cast<float4*>(a.ema + i) = e4;
    }
  }
  adamw_groups_span<EMA>(a, c, tab, num, 0, a.head);
  adamw_groups_span<EMA>(a, c, tab, num, vend, a.n);
}
int64_t adamw_groups_ws_bytes(int num) { return num <= 0 ? 0 : ((int64_t)num * (int64_t)sizeof(AdamwGroup) + 255) / 256 * 256 + 256; }
// `groups`: HOST table, already validated (adamw_groups_check); `ws`: at least adamw_groups_ws_bytes(num) device bytes (unused with num == 0)
void k_adamw_groups(spa3d_ctx* c, float* p, const float* g, float* m, float* v, int64_t n, float lr, int64_t step, float clip, float b1, float b2,
                    float eps, float wd, const AdamwGroup* groups, int num, float* ema, float ema_decay, float* scratch, void* ws) {
  const AdamwGroup* tab = nullptr;
  if (num > 0) {
    int32_t* dst = reinterpret_cast<int32_t*>(((uintptr_t)ws + 255) / 256 * 256);
    tab = reinterpret_cast<const AdamwGroup*>(dst);
    const int32_t* src = reinterpret_cast<const int32_t*>(groups);
    for (int k0 = 0; k0 < num; k0 += GROUPS_PER_LAUNCH) {
      GroupWords w;
      const int nw = std::min(GROUPS_PER_LAUNCH, num - k0) * ADAMW_GROUP_WORDS;
      for (int i = 0; i < GROUPS_PER_LAUNCH * ADAMW_GROUP_WORDS; ++i) w.v[i] = i < nw ? src[(int64_t)k0 * ADAMW_GROUP_WORDS + i] : 0;
      set_groups_kernel<<<1, 256, 0, c->stream>>>(dst + (int64_t)k0 * ADAMW_GROUP_WORDS, w, nw);
    }
  }
  (void)hipMemsetAsync(scratch, 0, 12, c->stream);
  const unsigned gs = (unsigned)std::min<int64_t>(cdiv(n, 256), SUMSQ_MAXB);
  sumsq_groups_kernel<<<gs, 256, 0, c->stream>>>(g, n, tab, adamw_groups_any_frozen(groups, num) ? num : 0, scratch + SUMSQ_OFF);   // (a table that freezes nothing: every element counts)
  adamw_guard_kernel<<<1, 256, 0, c->stream>>>(scratch, (int)gs);
  AdamwGroupsArgs a;
  a.p = p; a.g = g; a.m = m; a.v = v; a.ema = ema; a.n = n;
  a.lr = lr; a.tstep = (float)(step + 1); a.clip = clip; a.b1 = b1; a.b2 = b2; a.eps = eps; a.wd = wd;
  a.ema_d = ema_decay; a.ema_omd = 1.f - ema_decay;
  a.scratch = scratch;
  // the 16-byte body needs every stream at the same offset from a 16-byte boundary; buffers that disagree go element by element throughout
  const uintptr_t ph = ((uintptr_t)p >> 2) & 3;
  const bool same = (((uintptr_t)g >> 2) & 3) == ph && (((uintptr_t)m >> 2) & 3) == ph && (((uintptr_t)v >> 2) & 3) == ph && (!ema || (((uintptr_t)ema >> 2) & 3) == ph);
  a.head = same ? std::min<int64_t>((int64_t)((4 - ph) & 3), n) : n;
  a.nvec = (n - a.head) / 4;
  const int64_t runs = std::max<int64_t>(cdiv(4 * a.nvec, 1024), cdiv(n - 4 * a.nvec, 256));
  const unsigned gr = (unsigned)std::min<int64_t>(std::max<int64_t>(runs, 1), 4096);
  if (ema) adamw_groups_kernel<true><<<gr, 256, 0, c->stream>>>(a, tab, num); else adamw_groups_kernel<false><<<gr, 256, 0, c->stream>>>(a, tab, num);
  SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// jax.random.uniform(PRNGKey(k0,k1), [n]) legacy threefry layout
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__device__ void threefry2x32(uint32_t k0, uint32_t k1, uint32_t& x0, uint32_t& x1) {
  const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
  const int R[2][4] = {{13, 15, 26, 6}, {17, 29, 16, 24}};
  x0 += ks[0]; x1 += ks[1];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { x0 += x1; x1 = rotl32(x1, R[i & 1][j]); x1 ^= x0; }
    x0 += ks[(i + 1) % 3]; x1 += ks[(i + 2) % 3] + (uint32_t)(i + 1);
  }
}
__global__ void uniform_noise_kernel(float* __restrict__ out, int64_t n, int64_t half, uint32_t k0, uint32_t k1) {
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < half; j += (int64_t)gridDim.x * 256) {
    uint32_t x0 = (uint32_t)j, x1 = (uint32_t)(half + j);
    threefry2x32(k0, k1, x0, x1);
    out[j] = __uint_as_float((x0 >> 9) | 0x3F800000u) - 1.0f;
    if (half + j < n) out[half + j] = __uint_as_float((x1 >> 9) | 0x3F800000u) - 1.0f;
  }
}
void k_uniform_noise(spa3d_ctx* c, float* out, int64_t n, uint32_t k0, uint32_t k1) {
  if (c->dry || n == 0) return;
  int64_t half = (n + (n & 1)) / 2;
  uniform_noise_kernel<<<GRID1D(half, 256), 256, 0, c->stream>>>(out, n, half, k0, k1); SPA_LAUNCH_CHECK(c);
}
// deterministic mode: fold the fixed-point shadow of a range of the gradient buffer into it (and clear the shadow: a later flush of the same range adds nothing).
// A sum of 2^62 units or more is overflow (common.hpp DetCfg): NaN, like the sticky flag -- a wrapped sum must never reach the buffer as a finite value.
__global__ __launch_bounds__(256) void det_flush_kernel(const DetCfg* __restrict__ det, int64_t lo, int64_t n) {
  const DetCfg d = *det;
  float* __restrict__ g = d.gbase + lo;
  long long* __restrict__ shadow = d.shadow + lo;
  const bool bad = *d.flag != 0;
  const double inv = 1.0 / (double)d.scale;   // a power of two: exact
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const long long q = shadow[i];
    if (q != 0 || bad) {
      const bool ovf = bad || q >= DET_SUM_MAX || q <= -DET_SUM_MAX;
      g[i] = ovf ? __int_as_float(0x7fc00000) : g[i] + (float)((double)q * inv); shadow[i] = 0;
    }
  }
}
void k_det_flush(spa3d_ctx* c, int64_t lo, int64_t n) {
  if (c->dry || n <= 0) return;
  det_flush_kernel<<<(unsigned)std::min<int64_t>(cdiv(n, 256), 8192), 256, 0, c->stream>>>(c->det, lo, n); SPA_LAUNCH_CHECK(c);
}
// the fixed-point unit of a det_grads call (common.hpp DetCfg): 2^(32 + e), e = floor(log2(denom / (n_vis * loss scale))) clamped to [-24, 40].  Inputs are the call's
// global denominator, its own visible count and its loss scale, so the unit is a function of the call's inputs alone (bit-equal run to run and whatever the
// all-reduce schedule).  -24 covers the fp16 mode at BASELINE configs[2] (e ~ -14); below it the unit stops coarsening and the range guards take over.
// gshift = floor(log2(gmax / 5000)) (host; 0 for the default objective): a gradient of the call also scales as the objective's largest head gradient gmax, so the
// unit follows it by that power of two -- e - gshift is what is clamped -- and a visibility-only objective is resolved as finely, relative to its size, as the default.
// Writes the call's DetCfg, with the unit as its scale, where the call's kernels read it.
__global__ void det_unit_kernel(const float* sums, const unsigned* poison, const float* denom_dev, const float* scale_dev, int gshift, DetCfg d, DetCfg* out) {
  const float nvis = fmaxf(loss_acc_read((const unsigned long long*)sums + 2, poison), 1.f);   // fmaxf(NaN, 1) = 1
  const float r = *denom_dev / (nvis * (scale_dev ? *scale_dev : 1.f));
  int e = 0;
  if (r > 0.f && r <= 3.0e38f) { (void)frexpf(r, &e); e = min(max(e - 1 - gshift, DET_E_MIN), DET_E_MAX); }   // r = m 2^e', m in [0.5, 1): floor(log2 r) = e' - 1, exactly
  d.scale = ldexpf(1.f, 32 + e);
  *out = d;
}
void k_det_unit(spa3d_ctx* c, const float* sums, const unsigned* poison, const float* denom_dev, const float* scale_dev, int gshift, const DetCfg& d, DetCfg* out) {
  if (c->dry) return;
  det_unit_kernel<<<1, 1, 0, c->stream>>>(sums, poison, denom_dev, scale_dev, gshift, d, out); SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// explicit instantiations
// ---------------------------------------------------------------------------------------------
#define INST_LOSS(T) \
  template void k_loss_bwd<T>(spa3d_ctx*, const float*, int64_t, int, const float*, const float*, const float*, const spa3d_loss_config&, const float*, T*, int, const float*);
INST_LOSS(float)
INST_LOSS(bf16_t)
}  // namespace SPA_NS
