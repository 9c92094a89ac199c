// attention.hip -- attention core of ImprovedMHDPAttention (attention.py:166-175): per-head RMSNorm of q,k,
// q/sqrt(Dh), key mask with finfo.min fill, softmax, PV -- forward and backward.
// The two front ends plan (attn_plan.hpp) and run the plan: the generic composition of the strided batched MFMA GEMM with the row-wise kernels
// below (RMSNorm, softmax) -- any Sq / Sk / Dh <= 128, both dtypes, the F32 parity path -- or the fused LDS-resident kernels (attention_fused.hip).
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace SPA_NS {

// ---------------------------------------------------------------------------------------------
// per-head RMSNorm over Dh (flax nn.RMSNorm eps 1e-6) attention.py:166-167.  one wave per (row, head)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void rms_heads_fwd_kernel(const T* __restrict__ x, int64_t ldx, const float* __restrict__ scale,
                                                            T* __restrict__ y, int64_t ldy, int64_t rows, int H, int Dh) {
  const int lane = threadIdx.x & 63;
  int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t n = rows * H, stride = (int64_t)gridDim.x * 4;
  for (; item < n; item += stride) {
    int64_t row = item / H; int h = (int)(item - row * H);
    const T* xr = x + row * ldx + h * Dh;
    float v0 = lane < Dh ? ld(xr + lane) : 0.f;
    float v1 = lane + 64 < Dh ? ld(xr + lane + 64) : 0.f;
    float ms = wave_sum(v0 * v0 + v1 * v1) / Dh;
    float r = rsqrtf(ms + 1e-6f);
    T* yr = y + row * ldy + h * Dh;
    if (lane < Dh) st(yr + lane, v0 * r * scale[lane]);
    if (lane + 64 < Dh) st(yr + lane + 64, v1 * r * scale[lane + 64]);
  }
}
template <typename T>
void k_rmsnorm_heads(spa3d_ctx* c, const T* x, int64_t ldx, const float* scale, T* y, int64_t ldy, int64_t rows, int H, int Dh) {
  if (c->dry || rows == 0) return;
  unsigned g = (unsigned)std::min<int64_t>(cdiv(rows * H, 4), 65536);
  rms_heads_fwd_kernel<T><<<g, 256, 0, c->stream>>>(x, ldx, scale, y, ldy, rows, H, Dh);
  SPA_LAUNCH_CHECK(c);
}
// dx = r*(g - xhat*mean(g*xhat)), g=dy*scale ; dscale += sum dy*xhat
template <typename T>
__global__ __launch_bounds__(256) void rms_heads_bwd_kernel(const T* __restrict__ x, int64_t ldx, const float* __restrict__ scale,
                                                            const T* __restrict__ dy, int64_t lddy, T* __restrict__ dx, int64_t lddx,
                                                            float* __restrict__ dscale, int64_t rows, int H, int Dh, const DetCfg* det) {
  __shared__ float red[4][128];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float a0 = 0.f, a1 = 0.f;
  int64_t item = (int64_t)blockIdx.x * 4 + w;
  const int64_t n = rows * H, stride = (int64_t)gridDim.x * 4;
  const float s0 = lane < Dh ? scale[lane] : 0.f, s1 = lane + 64 < Dh ? scale[lane + 64] : 0.f;
  for (; item < n; item += stride) {
    int64_t row = item / H; int h = (int)(item - row * H);
    const T* xr = x + row * ldx + h * Dh;
    const T* dyr = dy + row * lddy + h * Dh;
    float v0 = lane < Dh ? ld(xr + lane) : 0.f, v1 = lane + 64 < Dh ? ld(xr + lane + 64) : 0.f;
    float d0 = lane < Dh ? ld(dyr + lane) : 0.f, d1 = lane + 64 < Dh ? ld(dyr + lane + 64) : 0.f;
    float r = rsqrtf(wave_sum(v0 * v0 + v1 * v1) / Dh + 1e-6f);
    float xh0 = v0 * r, xh1 = v1 * r;
    float g0 = d0 * s0, g1 = d1 * s1;
    float mg = wave_sum(g0 * xh0 + g1 * xh1) / Dh;
    a0 += d0 * xh0; a1 += d1 * xh1;
    T* dxr = dx + row * lddx + h * Dh;
    if (lane < Dh) st(dxr + lane, r * (g0 - xh0 * mg));
    if (lane + 64 < Dh) st(dxr + lane + 64, r * (g1 - xh1 * mg));
  }
  red[w][lane] = a0; red[w][lane + 64] = a1;
  __syncthreads();
  if (w == 0) {
    if (lane < Dh) grad_add(det_read(det), dscale + lane, red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]);
    if (lane + 64 < Dh) grad_add(det_read(det), dscale + lane + 64, red[0][lane + 64] + red[1][lane + 64] + red[2][lane + 64] + red[3][lane + 64]);
  }
}
template <typename T>
void k_rmsnorm_heads_bwd(spa3d_ctx* c, const T* x, int64_t ldx, const float* scale, const T* dy, int64_t lddy, T* dx, int64_t lddx,
                         float* dscale, int64_t rows, int H, int Dh) {
  if (c->dry || rows == 0) return;
  unsigned g = (unsigned)std::min<int64_t>(cdiv(rows * H, 4), 2048);
  rms_heads_bwd_kernel<T><<<g, 256, 0, c->stream>>>(x, ldx, scale, dy, lddy, dx, lddx, dscale, rows, H, Dh, c->det);
  SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// softmax over keys with key mask: where(mask, logit, finfo.min) -> softmax (flax dot_product_attention)
// s: [nseq][H][Sq][Sk] in place.  one wave per row.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void softmax_kernel(T* __restrict__ s, const float* __restrict__ km, int64_t nseq, int H, int Sq, int Sk) {
  const int lane = threadIdx.x & 63;
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nrows = nseq * H * Sq, stride = (int64_t)gridDim.x * 4;
  for (; row < nrows; row += stride) {
    int64_t seq = row / ((int64_t)H * Sq);
    T* sr = s + row * Sk;
    const float* kmr = km ? km + seq * Sk : nullptr;
    float m = -3.4028234663852886e38f;
    for (int k = lane; k < Sk; k += 64) {
      float v = ld(sr + k);
      if (kmr && kmr[k] == 0.f) v = -3.4028234663852886e38f;
      m = fmaxf(m, v);
    }
    m = wave_max(m);
    float sum = 0.f;
    for (int k = lane; k < Sk; k += 64) {
      float v = ld(sr + k);
      if (kmr && kmr[k] == 0.f) v = -3.4028234663852886e38f;
      sum += expf(v - m);
    }
    sum = wave_sum(sum);
    float inv = 1.f / sum;
    for (int k = lane; k < Sk; k += 64) {
      float v = ld(sr + k);
      if (kmr && kmr[k] == 0.f) v = -3.4028234663852886e38f;
      st(sr + k, expf(v - m) * inv);
    }
  }
}
template <typename T>
void k_softmax(spa3d_ctx* c, T* s, const float* keymask, int64_t nseq, int H, int Sq, int Sk) {
  if (c->dry || nseq == 0) return;
  unsigned g = (unsigned)std::min<int64_t>(cdiv(nseq * H * Sq, 4), 65536);
  softmax_kernel<T><<<g, 256, 0, c->stream>>>(s, keymask, nseq, H, Sq, Sk);
  SPA_LAUNCH_CHECK(c);
}
// dS = P o (dP - rowsum(dP o P)), in place on dp; masked keys get exactly 0: where(mask, logit, min) passes them no gradient
// (this matters only for fully masked rows, where P is uniform instead of 0)
template <typename T>
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const T* __restrict__ p, T* __restrict__ dp, int64_t rows, int Sk,
                                                          const float* __restrict__ km, int64_t rows_per_seq) {
  const int lane = threadIdx.x & 63;
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (; row < rows; row += stride) {
    const T* pr = p + row * Sk; T* dr = dp + row * Sk;
    float s = 0.f;
    for (int k = lane; k < Sk; k += 64) s += ld(pr + k) * ld(dr + k);
    s = wave_sum(s);
    const float* kmr = km ? km + (row / rows_per_seq) * Sk : nullptr;
    for (int k = lane; k < Sk; k += 64) {
      float pv = ld(pr + k);
      float v = pv * (ld(dr + k) - s);
      if (kmr && kmr[k] == 0.f) v = 0.f;
      st(dr + k, v);
    }
  }
}
template <typename T>
void k_softmax_bwd(spa3d_ctx* c, const T* p, T* dp, int64_t rows, int Sk, const float* km, int64_t rows_per_seq) {
  if (c->dry || rows == 0) return;
  unsigned g = (unsigned)std::min<int64_t>(cdiv(rows, 4), 65536);
  softmax_bwd_kernel<T><<<g, 256, 0, c->stream>>>(p, dp, rows, Sk, km, rows_per_seq);
  SPA_LAUNCH_CHECK(c);
}

template <typename T> static T* aalloc(spa3d_ctx* c, int64_t n) { return (T*)c->ar.alloc(n * (int64_t)sizeof(T)); }

static int64_t attn_chunk(int64_t nseq, int Sq, int Sk, int H, int E, int esz) {
  int64_t per = (int64_t)H * Sq * Sk + (int64_t)(Sq + Sk) * E;
  int64_t cs = std::max<int64_t>(1, (int64_t)(768ll << 20) / (per * esz));
  return std::min(cs, nseq);
}
template <typename T>
static void scores(spa3d_ctx* c, const T* qn, const T* kn, T* s, int64_t ns, int Sq, int Sk, int H, int Dh) {
  const int E = H * Dh;
  GemmDesc d{};
  d.A = qn; d.B = kn; d.C = s; d.M = Sq; d.N = Sk; d.K = Dh;
  d.sAm = E; d.sAk = 1; d.sBk = 1; d.sBn = E; d.sCm = Sk;
  d.nb1 = (int)ns; d.nb2 = H; d.bA1 = (int64_t)Sq * E; d.bA2 = Dh; d.bB1 = (int64_t)Sk * E; d.bB2 = Dh;
  d.bC1 = (int64_t)H * Sq * Sk; d.bC2 = (int64_t)Sq * Sk;
  d.alpha = 1.0f / sqrtf((float)Dh);
  gemm_generic<T>(c, d);
}

// ---- a fused plan: its fp32 partials from the arena (the same in the dry run, which needed only the plan), then the launcher
void attn_launch(spa3d_ctx* c, const AttnDesc& d, const AttnPlan& pl) {
  const int64_t mk = c->ar.mark();
  float* part[2] = {nullptr, nullptr};
  for (int i = 0; i < 2; ++i)
    if (pl.part_bytes[i]) part[i] = (float*)c->ar.alloc(pl.part_bytes[i]);
  if (!c->dry) { if (pl.kernel == AttnKernel::QkvFwd) qkv_attn_launch(c, d); else attn_fused_launch(c, d, pl, part); }
  c->ar.release(mk);  // stream-ordered: whatever reuses the space is launched behind the route's kernels
}
static void attn_refuse(spa3d_ctx* c, AttnRefusal why, const char* dir) {
  if (c->hip_err) return;
  c->hip_err = -2;
  c->err = why == AttnRefusal::RaggedNeedsFused ? "ragged sequences need the fused attention kernels" : std::string("fused attention ") + dir + " does not cover this shape/dtype";
}
// sequence i of a RaggedKeys / Hole problem as a Dense problem of its own (Hole: over the compact key copy kc / vc of E-wide rows)
template <typename T>
static AttnDesc one_sequence(const AttnDesc& d, int64_t i, const T* kc = nullptr, const T* vc = nullptr) {
  const bool hole = d.layout == AttnLayout::Hole;
  const int64_t E = (int64_t)d.H * d.Dh, k0 = hole ? 0 : d.koff_host[i];
  AttnDesc s = d;
  s.layout = AttnLayout::Dense; s.nseq = 1; s.Sk = d.keys_of(i); s.km = nullptr;
  s.q = (const T*)d.q + i * d.Sq * d.ldq; s.o = d.o ? (T*)d.o + i * d.Sq * E : nullptr; s.lse = d.lse ? d.lse + i * d.H * d.Sq * 2 : nullptr;
  if (hole) { s.k = kc; s.v = vc; s.ldk = s.ldv = E; }
  else { s.k = (const T*)d.k + k0 * d.ldk; s.v = (const T*)d.v + k0 * d.ldv; }
  if (d.d_o) { s.d_o = (const T*)d.d_o + i * d.Sq * E; s.dq = (T*)d.dq + i * d.Sq * d.ldq; s.dk = (T*)d.dk + k0 * d.ldk; s.dv = (T*)d.dv + k0 * d.ldv; }
  return s;
}

template <typename T>
static void generic_fwd(spa3d_ctx* c, const AttnDesc& a) {
  const T *q = (const T*)a.q, *k = (const T*)a.k, *v = (const T*)a.v; T* o = (T*)a.o;
  const int64_t ldq = a.ldq, ldk = a.ldk, ldv = a.ldv, nseq = a.nseq; const float *sq = a.sq, *sk = a.sk, *km = a.km;
  const int Sq = a.Sq, Sk = a.Sk, H = a.H, Dh = a.Dh, E = H * Dh;
  const int64_t cs = attn_chunk(nseq, Sq, Sk, H, E, (int)sizeof(T));
  int64_t mk = c->ar.mark();
  T* qn = aalloc<T>(c, cs * Sq * E); T* kn = aalloc<T>(c, cs * Sk * E); T* s = aalloc<T>(c, cs * H * Sq * Sk);
  for (int64_t s0 = 0; s0 < nseq; s0 += cs) {
    const int64_t ns = std::min(cs, nseq - s0);
    k_rmsnorm_heads<T>(c, q + s0 * Sq * ldq, ldq, sq, qn, E, ns * Sq, H, Dh);
    k_rmsnorm_heads<T>(c, k + s0 * Sk * ldk, ldk, sk, kn, E, ns * Sk, H, Dh);
    scores<T>(c, qn, kn, s, ns, Sq, Sk, H, Dh);
    k_softmax<T>(c, s, km ? km + s0 * Sk : nullptr, ns, H, Sq, Sk);
    GemmDesc d{};  // O = P V
    d.A = s; d.B = v + s0 * Sk * ldv; d.C = o + s0 * Sq * E; d.M = Sq; d.N = Dh; d.K = Sk;
    d.sAm = Sk; d.sAk = 1; d.sBk = ldv; d.sBn = 1; d.sCm = E;
    d.nb1 = (int)ns; d.nb2 = H; d.bA1 = (int64_t)H * Sq * Sk; d.bA2 = (int64_t)Sq * Sk; d.bB1 = (int64_t)Sk * ldv; d.bB2 = Dh;
    d.bC1 = (int64_t)Sq * E; d.bC2 = Dh;
    gemm_generic<T>(c, d);
  }
  c->ar.release(mk);
}
// The generic route of a RaggedKeys / Hole problem: the sequences one by one, each planned again (a sequence the single launch declined may still run on the
// fused kernels).  Hole: on a compact copy of the two key segments, so sequence i gets the bits of attention_fwd on a compacted copy either way.
template <typename T>
static void per_sequence_fwd(spa3d_ctx* c, const AttnDesc& d) {
  if (d.layout == AttnLayout::RaggedKeys) {
    for (int64_t i = 0; i < d.nseq; ++i) attention_fwd<T>(c, one_sequence<T>(d, i));
    return;
  }
  const int E = d.H * d.Dh, Nk = d.Nk;
  const T *k = (const T*)d.k, *v = (const T*)d.v;
  const int64_t mk = c->ar.mark();
  T* kc = aalloc<T>(c, (int64_t)d.max_keys() * E); T* vc = aalloc<T>(c, (int64_t)d.max_keys() * E);
  auto seg = [&](T* dst, const T* src, int64_t ld_, int64_t r0, int64_t r1) {  // rows [r0, r1) of a strided [*, E] plane -> dense rows at dst
    if (c->dry || r1 <= r0) return;
    if (hipMemcpy2DAsync(dst, (size_t)E * sizeof(T), src + r0 * ld_, (size_t)ld_ * sizeof(T), (size_t)E * sizeof(T), (size_t)(r1 - r0), hipMemcpyDeviceToDevice,
                         c->stream) != hipSuccess && !c->hip_err) { c->hip_err = -8; c->err = "hold-out attention: compacting the keys failed"; }
  };
  for (int64_t i = 0; i < d.nseq; ++i) {
    const int lo = d.holes_host[2 * i], hi = d.holes_host[2 * i + 1];
    seg(kc, k, d.ldk, 0, lo); seg(kc + (int64_t)lo * E, k, d.ldk, hi, Nk);
    seg(vc, v, d.ldv, 0, lo); seg(vc + (int64_t)lo * E, v, d.ldv, hi, Nk);
    attention_fwd<T>(c, one_sequence<T>(d, i, kc, vc));
  }
  c->ar.release(mk);
}
template <typename T>
void attention_fwd(spa3d_ctx* c, const AttnDesc& d) {
  const AttnPlan pl = plan_attn_fwd(d, c->attn);
  if (pl.kernel == AttnKernel::Refuse) return attn_refuse(c, pl.why, "forward");
  if (pl.kernel == AttnKernel::Generic) return generic_fwd<T>(c, d);
  if (pl.kernel == AttnKernel::GenericPerSeq) return per_sequence_fwd<T>(c, d);
  attn_launch(c, d, pl);
}

template <typename T>
static void generic_bwd(spa3d_ctx* c, const AttnDesc& a) {
  const T *q = (const T*)a.q, *k = (const T*)a.k, *v = (const T*)a.v, *d_o = (const T*)a.d_o; T *dq = (T*)a.dq, *dk = (T*)a.dk, *dv = (T*)a.dv;
  const int64_t ldq = a.ldq, ldk = a.ldk, ldv = a.ldv, nseq = a.nseq; const float *sq = a.sq, *sk = a.sk, *km = a.km; float *dsq = a.dsq, *dsk = a.dsk;
  const int Sq = a.Sq, Sk = a.Sk, H = a.H, Dh = a.Dh, E = H * Dh;
  const int64_t cs = attn_chunk(nseq, Sq, Sk, H, E, (int)sizeof(T));
  int64_t mk = c->ar.mark();
  T* qn = aalloc<T>(c, cs * Sq * E); T* kn = aalloc<T>(c, cs * Sk * E); T* s = aalloc<T>(c, cs * H * Sq * Sk);
  T* dp = aalloc<T>(c, cs * H * Sq * Sk); T* dqn = aalloc<T>(c, cs * Sq * E); T* dkn = aalloc<T>(c, cs * Sk * E);
  const float alpha = 1.0f / sqrtf((float)Dh);
  for (int64_t s0 = 0; s0 < nseq; s0 += cs) {
    const int64_t ns = std::min(cs, nseq - s0);
    const T* q0 = q + s0 * Sq * ldq; const T* k0 = k + s0 * Sk * ldk; const T* v0 = v + s0 * Sk * ldv;
    const T* do0 = d_o + s0 * Sq * E;
    k_rmsnorm_heads<T>(c, q0, ldq, sq, qn, E, ns * Sq, H, Dh);
    k_rmsnorm_heads<T>(c, k0, ldk, sk, kn, E, ns * Sk, H, Dh);
    scores<T>(c, qn, kn, s, ns, Sq, Sk, H, Dh);
    k_softmax<T>(c, s, km ? km + s0 * Sk : nullptr, ns, H, Sq, Sk);
    const int64_t bS1 = (int64_t)H * Sq * Sk, bS2 = (int64_t)Sq * Sk;
    {  // dP = dO V^T
      GemmDesc d{};
      d.A = do0; d.B = v0; d.C = dp; d.M = Sq; d.N = Sk; d.K = Dh;
      d.sAm = E; d.sAk = 1; d.sBk = 1; d.sBn = ldv; d.sCm = Sk;
      d.nb1 = (int)ns; d.nb2 = H; d.bA1 = (int64_t)Sq * E; d.bA2 = Dh; d.bB1 = (int64_t)Sk * ldv; d.bB2 = Dh; d.bC1 = bS1; d.bC2 = bS2;
      gemm_generic<T>(c, d);
    }
    {  // dV = P^T dO
      GemmDesc d{};
      d.A = s; d.B = do0; d.C = dv + s0 * Sk * ldv; d.M = Sk; d.N = Dh; d.K = Sq;
      d.sAm = 1; d.sAk = Sk; d.sBk = E; d.sBn = 1; d.sCm = ldv;
      d.nb1 = (int)ns; d.nb2 = H; d.bA1 = bS1; d.bA2 = bS2; d.bB1 = (int64_t)Sq * E; d.bB2 = Dh; d.bC1 = (int64_t)Sk * ldv; d.bC2 = Dh;
      gemm_generic<T>(c, d);
    }
    k_softmax_bwd<T>(c, s, dp, ns * H * Sq, Sk, km ? km + s0 * Sk : nullptr, (int64_t)H * Sq);  // dp := dS
    {  // dQn = alpha dS Kn
      GemmDesc d{};
      d.A = dp; d.B = kn; d.C = dqn; d.M = Sq; d.N = Dh; d.K = Sk;
      d.sAm = Sk; d.sAk = 1; d.sBk = E; d.sBn = 1; d.sCm = E; d.alpha = alpha;
      d.nb1 = (int)ns; d.nb2 = H; d.bA1 = bS1; d.bA2 = bS2; d.bB1 = (int64_t)Sk * E; d.bB2 = Dh; d.bC1 = (int64_t)Sq * E; d.bC2 = Dh;
      gemm_generic<T>(c, d);
    }
    {  // dKn = alpha dS^T Qn
      GemmDesc d{};
      d.A = dp; d.B = qn; d.C = dkn; d.M = Sk; d.N = Dh; d.K = Sq;
      d.sAm = 1; d.sAk = Sk; d.sBk = E; d.sBn = 1; d.sCm = E; d.alpha = alpha;
      d.nb1 = (int)ns; d.nb2 = H; d.bA1 = bS1; d.bA2 = bS2; d.bB1 = (int64_t)Sq * E; d.bB2 = Dh; d.bC1 = (int64_t)Sk * E; d.bC2 = Dh;
      gemm_generic<T>(c, d);
    }
    k_rmsnorm_heads_bwd<T>(c, q0, ldq, sq, dqn, E, dq + s0 * Sq * ldq, ldq, dsq, ns * Sq, H, Dh);
    k_rmsnorm_heads_bwd<T>(c, k0, ldk, sk, dkn, E, dk + s0 * Sk * ldk, ldk, dsk, ns * Sk, H, Dh);
  }
  c->ar.release(mk);
}

template <typename T>
void attention_bwd(spa3d_ctx* c, const AttnDesc& d) {
  const AttnPlan pl = plan_attn_bwd(d, c->attn);
  if (pl.kernel == AttnKernel::Refuse) return attn_refuse(c, pl.why, "backward");
  if (pl.kernel == AttnKernel::Generic) return generic_bwd<T>(c, d);
  if (pl.kernel == AttnKernel::GenericPerSeq) {   // ragged keys, sequence by sequence
    for (int64_t i = 0; i < d.nseq; ++i) attention_bwd<T>(c, one_sequence<T>(d, i));
    return;
  }
  attn_launch(c, d, pl);
}

#define INST_ATTN(T)                                           \
  template void attention_fwd<T>(spa3d_ctx*, const AttnDesc&); \
  template void attention_bwd<T>(spa3d_ctx*, const AttnDesc&);
INST_ATTN(float)
INST_ATTN(bf16_t)
}  // namespace SPA_NS
