// embed.hip -- what turns the inputs and the parameters into the first token rows (gfx950): the sinusoidal, token and query embeddings,
// the row maps of the one-pass embedding, the readout rows, the key masks, the rank-K (depth) projection, and the weight shadows
// (pack / transpose).  Element-wise, HBM-bound kernels.
// T in {float, bf16_t} storage, fp32 math.  References such as attention.py:49 are to the reference implementation's files.
#include <algorithm>

#include "common.hpp"

namespace SPA_NS {

// ---------------------------------------------------------------------------------------------
// SinusoidalEmbedding (track_autoencoder.py:18-38): v = fl32(x*s_f); out = sin([v, fl32(v + fl32(pi/2))])
// layout "(coords d)": out[r][c*2nf + f] , out[r][c*2nf + nf + f].  Never fused to fma, never cos.
// ---------------------------------------------------------------------------------------------
struct SinScales { float s[64]; };
static SinScales make_scales(int nf) {
  SinScales sc;
  for (int i = 0; i < 64; ++i) sc.s[i] = i < nf ? (float)pow(2.0, (double)i / 3.0) : 0.f;
  return sc;
}
__device__ __forceinline__ float sin_feat(float x, float s, bool shifted) {
  float v = __fmul_rn(x, s);
  if (shifted) v = __fadd_rn(v, 1.57079637050628662109375f);  // fl32(0.5*pi)
  return sinf(v);
}
template <typename T>
__global__ __launch_bounds__(256) void sin_embed_kernel(const float* __restrict__ x, int64_t rows, int C, int nf, float prescale,
                                                        SinScales sc, T* __restrict__ out) {
  const int W = C * 2 * nf;
  const int64_t n = rows * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int64_t r = i / W; int j = (int)(i - r * W);
    int cc = j / (2 * nf); int f = j - cc * 2 * nf;
    float xv = x[r * C + cc] / prescale;
    st(out + i, sin_feat(xv, sc.s[f < nf ? f : f - nf], f >= nf));
  }
}
template <typename T>
void k_sin_embed(spa3d_ctx* c, const float* x, int64_t rows, int C, int nf, float prescale, T* out) {
  if (c->dry || rows == 0) return;
  sin_embed_kernel<T><<<GRID1D(rows * C * 2 * nf, 256), 256, 0, c->stream>>>(x, rows, C, nf, prescale, make_scales(nf), out);
  SPA_LAUNCH_CHECK(c);
}

// E1+E2 for the track tokens (track_autoencoder_3d.py:126-134): x4 = [x,y,z,t/T] -> sinbuf[nseq*T][4*2nf]
template <typename T>
__global__ __launch_bounds__(256) void embed_tokens_kernel(const float* __restrict__ tracks, int64_t nrows, int T_, int nf, float prescale,
                                                           SinScales sc, T* __restrict__ out, int NC) {
  const int W = (NC + 1) * 2 * nf;
  const int64_t n = nrows * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int64_t r = i / W; int j = (int)(i - r * W);
    int cc = j / (2 * nf); int f = j - cc * 2 * nf;
    float xv;
    if (cc < NC) xv = tracks[r * NC + cc];
    else xv = (float)(int)(r % T_) / (float)T_;  // jnp.arange(T)/T
    xv = xv / prescale;
    st(out + i, sin_feat(xv, sc.s[f < nf ? f : f - nf], f >= nf));
  }
}
// vectorised: 8 consecutive features (one coordinate, one sin/cos half) per thread, one 16-B store, 32-bit index math, the scale table
// in LDS (indexing the by-value kernel argument per lane went through scratch).  Same arithmetic as sin_feat(): results are identical.
template <typename T>
__global__ __launch_bounds__(256) void embed_tokens_vec_kernel(const float* __restrict__ tracks, unsigned nrows, int T_, int nf, float prescale,
                                                               SinScales sc, T* __restrict__ out, int NC) {
  constexpr int NV = VecOf<T>::N;
  __shared__ float ssc[64];
  if (threadIdx.x < 64) ssc[threadIdx.x] = sc.s[threadIdx.x];
  __syncthreads();
  const unsigned W = (unsigned)(NC + 1) * 2u * nf, gpr = W / NV;   // groups per row
  const unsigned total = nrows * gpr;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned r = i / gpr; const int j0 = (int)(i - r * gpr) * NV;
    const int cc = j0 / (2 * nf); const int f0 = j0 - cc * 2 * nf;
    const bool shifted = f0 >= nf; const int fb = shifted ? f0 - nf : f0;
    float xv;
    if (cc < NC) xv = tracks[(int64_t)r * NC + cc];
    else xv = (float)(int)(r % (unsigned)T_) / (float)T_;  // jnp.arange(T)/T
    xv = xv / prescale;
    float o[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) o[e] = sin_feat(xv, ssc[fb + e], shifted);
    store_vec<T, NV>(out + (int64_t)r * W + j0, o);
  }
}
template <typename T>
void k_embed_tokens(spa3d_ctx* c, const float* tracks, int64_t nrows, int T_, int nf, float prescale, T* sinbuf, int NC) {
  if (c->dry || nrows == 0) return;
  constexpr int NV = VecOf<T>::N;
  const int64_t W = (int64_t)(NC + 1) * 2 * nf;
  if (nf % NV == 0 && nf <= 64 && nrows * (W / NV) < 0x7fffffffLL && nrows < 0x7fffffffLL && (((uintptr_t)sinbuf) & 15) == 0) {
    embed_tokens_vec_kernel<T><<<GRID1D(nrows * (W / NV), 256), 256, 0, c->stream>>>(tracks, (unsigned)nrows, T_, nf, prescale, make_scales(nf), sinbuf, NC);
  } else {
    embed_tokens_kernel<T><<<GRID1D(nrows * W, 256), 256, 0, c->stream>>>(tracks, nrows, T_, nf, prescale, make_scales(nf), sinbuf, NC);
  }
  SPA_LAUNCH_CHECK(c);
}

// get_decoder_context + first-level query features (track_autoencoder_3d.py:209-233,265-272):
// feat[q][0:6nf] = sin-embed(xyz/track_scale); feat[q][6nf] = floor(round(t)/time_scale); qframe = round(t) (half-even)
__global__ __launch_bounds__(256) void query_embed1_kernel(const float* __restrict__ qp, int64_t nq, int nf, float track_scale,
                                                           float time_scale, SinScales sc, float* __restrict__ feat, int32_t* __restrict__ qframe,
                                                           int NC) {
  const int W = NC * 2 * nf + 1;
  const int64_t n = nq * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int64_t q = i / W; int j = (int)(i - q * W);
    if (j == NC * 2 * nf) {
      int32_t fr = (int32_t)rintf(qp[q * (NC + 1)]);
      qframe[q] = fr;
      feat[i] = floorf((float)fr / time_scale);
    } else {
      int cc = j / (2 * nf); int f = j - cc * 2 * nf;
      float xv = qp[q * (NC + 1) + 1 + cc] / track_scale;
      feat[i] = sin_feat(xv, sc.s[f < nf ? f : f - nf], f >= nf);
    }
  }
}
void k_query_embed1(spa3d_ctx* c, const float* qp, int64_t nq, int nf, float track_scale, float time_scale, float* feat, int32_t* qframe,
                    int NC) {
  if (c->dry || nq == 0) return;
  query_embed1_kernel<<<GRID1D(nq * (NC * 2 * nf + 1), 256), 256, 0, c->stream>>>(qp, nq, nf, track_scale, time_scale, make_scales(nf), feat, qframe, NC);
  SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// token bookkeeping
// ---------------------------------------------------------------------------------------------
// One-pass embedding (model.hip encode_tracks): row maps of the token rows the encoder keeps.  Row j of the (compact or dense) token buffer is dense
// token q = row_src[j] (or j) = (seq, s): a frame token (s >= 1) reads input row seq * T + s - 1 and is written to row j; the readout token (s == 0)
// has no input -- its GEMM row is dropped (crow = -1, arow = any valid row) and row j receives the readout parameter here (3d:161-165).
template <typename T>
__global__ void embed_maps_kernel(const int32_t* __restrict__ row_src, int64_t rows, int S, int T_, int32_t* __restrict__ arow, int32_t* __restrict__ crow,
                                  T* __restrict__ tok, const float* __restrict__ ro, int d) {
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < rows; j += (int64_t)gridDim.x * 256) {
    const int64_t q = row_src ? row_src[j] : j;
    const int64_t seq = q / S; const int s_ = (int)(q - seq * S);
    if (s_ == 0) {
      arow[j] = (int32_t)(seq * T_); crow[j] = -1;
      for (int k = 0; k < d; ++k) st(tok + j * d + k, ro[k]);
    } else { arow[j] = (int32_t)(seq * T_ + s_ - 1); crow[j] = (int32_t)j; }
  }
}
template <typename T>
void k_embed_maps(spa3d_ctx* c, const int32_t* row_src, int64_t rows, int S, int T_, int32_t* arow, int32_t* crow, T* tok, const float* readout, int d) {
  if (c->dry || rows == 0) return;
  embed_maps_kernel<T><<<GRID1D(rows, 256), 256, 0, c->stream>>>(row_src, rows, S, T_, arow, crow, tok, readout, d); SPA_LAUNCH_CHECK(c);
}
// tok[seq][0][:] = readout param (track_autoencoder_3d.py:161-165)
template <typename T>
__global__ void set_readout_kernel(T* tok, const float* __restrict__ ro, int64_t nseq, int S, int d) {
  const int64_t n = nseq * d;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int64_t s = i / d; int j = (int)(i - s * d);
    st(tok + s * S * d + j, ro[j]);
  }
}
template <typename T> void k_set_readout_rows(spa3d_ctx* c, T* tok, const float* readout, int64_t nseq, int S, int d) {
  if (c->dry || nseq == 0) return;
  set_readout_kernel<T><<<GRID1D(nseq * d, 256), 256, 0, c->stream>>>(tok, readout, nseq, S, d); SPA_LAUNCH_CHECK(c);
}
// key mask (repairs R2/R3): km[seq][0]=1 ; km[seq][1+t] = visible[seq][t]!=0 && t < boundary[b]
__global__ void keymask_kernel(const float* __restrict__ vis, const int32_t* __restrict__ boundary, int64_t nseq, int N, int T_, float* km) {
  const int S = T_ + 1;
  const int64_t n = nseq * S;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int64_t s = i / S; int k = (int)(i - s * S);
    float v = 1.f;
    if (k > 0) { int t = k - 1; v = (vis[s * T_ + t] != 0.f && t < boundary[s / N]) ? 1.f : 0.f; }
    km[i] = v;
  }
}
void k_keymask(spa3d_ctx* c, const float* visible, const int32_t* boundary, int64_t nseq, int N, int T_, float* km) {
  if (c->dry || nseq == 0) return;
  keymask_kernel<<<GRID1D(nseq * (T_ + 1), 256), 256, 0, c->stream>>>(visible, boundary, nseq, N, T_, km); SPA_LAUNCH_CHECK(c);
}
// key mask of the 2-D model (ta:217-223): km[seq][t] = visible & (t < boundary), no readout key
__global__ void keymask2d_kernel(const float* __restrict__ vis, const int32_t* __restrict__ boundary, int64_t nseq, int N, int T_, float* km) {
  const int64_t n = nseq * T_;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int64_t s_ = i / T_; int t = (int)(i - s_ * T_);
    km[i] = (vis[i] != 0.f && t < boundary[s_ / N]) ? 1.f : 0.f;
  }
}
void k_keymask2d(spa3d_ctx* c, const float* visible, const int32_t* boundary, int64_t nseq, int N, int T_, float* km) {
  if (c->dry || nseq == 0) return;
  keymask2d_kernel<<<GRID1D(nseq * T_, 256), 256, 0, c->stream>>>(visible, boundary, nseq, N, T_, km); SPA_LAUNCH_CHECK(c);
}
__global__ void sum3_kernel(const float* a, const float* b, const float* c3, float* out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (a ? a[i] : 0.f) + (b ? b[i] : 0.f) + (c3 ? c3[i] : 0.f);
}
void k_sum3(spa3d_ctx* c, const float* a, const float* b, const float* c3, float* out, int n) {
  if (c->dry) return;
  sum3_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(a, b, c3, out, n); SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// Dense layers with a tiny input width (K <= 4: the 1-channel depth feature, 3d:143-147).  As a GEMM this is a rank-K update of a
// 3.4 M x 384 tensor: pure streaming.  out[crow(m)][:] += x[m][:K] . w[K][N] + bias, crow(m) = m + (m / G + 1) * S (token rows
// 1..T of each sequence).  8 columns (16 B) per thread.
// ---------------------------------------------------------------------------------------------
template <typename T, int K>   // T: the 16-bit type only (see the instantiations)
__global__ void rank_fwd_kernel(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias, T* __restrict__ out,
                                int64_t M, int N, int64_t ldo, int rgroup, int rskip) {
  constexpr int NV = 8;
  const int cpr = N / NV;                   // column groups per row
  const int slots = 256 / cpr;              // rows per block iteration (5 at N = 384)
  const int slot = threadIdx.x / cpr, c = (threadIdx.x - slot * cpr) * NV;
  if (slot >= slots) return;
  float wv[K][NV], bvv[NV];                 // this thread's weight / bias columns: loaded once
#pragma unroll
  for (int j = 0; j < NV; ++j) { bvv[j] = bias ? bias[c + j] : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) wv[k][j] = ld(w + (int64_t)k * N + c + j); }
  // four rows per iteration, all loads first: one 16-B load in flight per thread is latency-bound (1.5 TB/s)
  constexpr int U = 4;
  const int64_t stride = (int64_t)gridDim.x * slots;
  for (int64_t m0 = (int64_t)blockIdx.x * slots + slot; m0 < M; m0 += stride * U) {
    float cur[U][NV]; float xv[U][K]; T* o[U]; bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t m = m0 + u * stride; ok[u] = m < M;
      const int64_t mm = ok[u] ? m : m0;
      const int64_t crow = rgroup > 0 ? mm + ((unsigned)mm / (unsigned)rgroup + 1) * (int64_t)rskip : mm;  // M < 2^31 (host)
      o[u] = out + crow * ldo + c;
      load_vec<T, NV>(o[u], cur[u]);
#pragma unroll
      for (int k = 0; k < K; ++k) xv[u][k] = ld(x + mm * K + k);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) acc = fmaf(xv[u][k], wv[k][j], acc);
        cur[u][j] += acc + bvv[j];
      }
      if (ok[u]) store_vec<T, NV>(o[u], cur[u]);
    }
  }
}
// gw[K][N] += x^T dY(rows remapped), gb[N] += colsum(dY): one pass over dY, per-block partials in registers, f32 atomics at the end
template <typename T, int K>
__global__ void rank_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy, int64_t M, int N, int64_t ldy, int rgroup, int rskip,
                                float* __restrict__ gw, float* __restrict__ gb, int64_t rows_per_block) {
  constexpr int NV = 8;
  const int cpr = N / NV;                       // column groups per row
  const int slots = 256 / cpr;                  // rows processed per block iteration
  const int slot = threadIdx.x / cpr, c = (threadIdx.x - slot * cpr) * NV;
  const int64_t m0 = (int64_t)blockIdx.x * rows_per_block; int64_t m1 = m0 + rows_per_block; if (m1 > M) m1 = M;
  if (slot >= slots) m1 = m0;  // idle threads: no rows, but they take part in the barriers below
  float aw[K][NV], ab[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) { ab[j] = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) aw[k][j] = 0.f; }
  constexpr int U = 4;  // four rows per iteration, loads first
  for (int64_t mb = m0 + slot; mb < m1; mb += (int64_t)slots * U) {
    float d[U][NV]; float xv[U][K];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t m = mb + (int64_t)u * slots;
      if (m < m1) {
        const int64_t row = rgroup > 0 ? m + ((unsigned)m / (unsigned)rgroup + 1) * (int64_t)rskip : m;
        load_vec<T, NV>(dy + row * ldy + c, d[u]);
#pragma unroll
        for (int k = 0; k < K; ++k) xv[u][k] = ld(x + m * K + k);
      } else {
#pragma unroll
        for (int j = 0; j < NV; ++j) d[u][j] = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) xv[u][k] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int j = 0; j < NV; ++j) ab[j] += d[u][j];
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < NV; ++j) aw[k][j] = fmaf(xv[u][k], d[u][j], aw[k][j]);
    }
  }
  // block-level reduction over the row slots in LDS, then ONE global atomic per column per block (all blocks hit the same 2 N addresses)
  __shared__ float red[(K + 1) * 2048];  // (K + 1) x N floats, N <= 2048 (N / 8 <= 256 column groups)
  float* rw = red; float* rb = red + (int64_t)K * N;
  __syncthreads();
  for (int t = threadIdx.x; t < (K + 1) * N; t += 256) red[t] = 0.f;
  __syncthreads();
  if (slot < slots) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      atomicAdd(rb + c + j, ab[j]);
#pragma unroll
      for (int k = 0; k < K; ++k) atomicAdd(rw + k * N + c + j, aw[k][j]);
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < N; t += 256) {
    if (gb) atomicAdd(gb + t, rb[t]);   // plain float atomics: k_rank_bwd refuses the deterministic mode
#pragma unroll
    for (int k = 0; k < K; ++k) atomicAdd(gw + (int64_t)k * N + t, rw[k * N + t]);
  }
}
template <typename T>
bool k_rank_fwd(spa3d_ctx* c, const T* x, const T* w, const float* bias, T* out, int64_t M, int N, int K, int64_t ldo, int rgroup, int rskip) {
  if (K < 1 || K > 4 || N % 8 || N / 8 > 256 || ldo % 8 || (((uintptr_t)out) & 15) || M >= 0x7fffffffLL) return false;
  if (c->dry || M == 0) return true;
  const dim3 g = GRID1D(cdiv(M, 4 * (256 / (N / 8))) * 256, 256);
  switch (K) {
    case 1: rank_fwd_kernel<T, 1><<<g, 256, 0, c->stream>>>(x, w, bias, out, M, N, ldo, rgroup, rskip); break;
    case 2: rank_fwd_kernel<T, 2><<<g, 256, 0, c->stream>>>(x, w, bias, out, M, N, ldo, rgroup, rskip); break;
    case 3: rank_fwd_kernel<T, 3><<<g, 256, 0, c->stream>>>(x, w, bias, out, M, N, ldo, rgroup, rskip); break;
    default: rank_fwd_kernel<T, 4><<<g, 256, 0, c->stream>>>(x, w, bias, out, M, N, ldo, rgroup, rskip); break;
  }
  SPA_LAUNCH_CHECK(c);
  return true;
}
template <typename T>
bool k_rank_bwd(spa3d_ctx* c, const T* x, const T* dy, int64_t M, int N, int K, int64_t ldy, int rgroup, int rskip, float* gw, float* gb) {
  if (c->det) return false;  // its workgroup-level reduction uses LDS float atomics (arrival order): the deterministic mode takes the GEMM path
  if (K < 1 || K > 4 || N % 8 || N / 8 > 256 || ldy % 8 || (((uintptr_t)dy) & 15) || M >= 0x7fffffffLL) return false;
  if (c->dry || M == 0) return true;
  const int64_t rpb = std::max<int64_t>(256, cdiv(M, 1024));
  const unsigned g = (unsigned)cdiv(M, rpb);
  switch (K) {
    case 1: rank_bwd_kernel<T, 1><<<g, 256, 0, c->stream>>>(x, dy, M, N, ldy, rgroup, rskip, gw, gb, rpb); break;
    case 2: rank_bwd_kernel<T, 2><<<g, 256, 0, c->stream>>>(x, dy, M, N, ldy, rgroup, rskip, gw, gb, rpb); break;
    case 3: rank_bwd_kernel<T, 3><<<g, 256, 0, c->stream>>>(x, dy, M, N, ldy, rgroup, rskip, gw, gb, rpb); break;
    default: rank_bwd_kernel<T, 4><<<g, 256, 0, c->stream>>>(x, dy, M, N, ldy, rgroup, rskip, gw, gb, rpb); break;
  }
  SPA_LAUNCH_CHECK(c);
  return true;
}

// weight shadows: src f32 [rows][cols] (row stride src_ld) -> native T [rows][ldn-strided], transposed T [cols][ldt-strided]
template <typename T>
__global__ void pack_kernel(const float* __restrict__ src, int64_t src_ld, int rows, int cols, T* dn, int64_t ldn, T* dt, int64_t ldt) {
  __shared__ float tile[32][33];
  int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    int r = r0 + i, cc = c0 + tx;
    float v = (r < rows && cc < cols) ? src[(int64_t)r * src_ld + cc] : 0.f;
    tile[i][tx] = v;
    if (dn && r < rows && cc < cols) st(dn + (int64_t)r * ldn + cc, v);
  }
  __syncthreads();
  if (dt)
    for (int i = ty; i < 32; i += 8) {
      int cc = c0 + i, r = r0 + tx;
      if (r < rows && cc < cols) st(dt + (int64_t)cc * ldt + r, tile[tx][i]);
    }
}
template <typename T>
void k_pack(spa3d_ctx* c, const float* src, int64_t src_ld, int rows, int cols, T* dn, int64_t ldn, T* dt, int64_t ldt) {
  if (c->dry) return;
  pack_kernel<T><<<dim3((unsigned)cdiv(cols, 32), (unsigned)cdiv(rows, 32)), 256, 0, c->stream>>>(src, src_ld, rows, cols, dn, ldn, dt, ldt);
  SPA_LAUNCH_CHECK(c);
}

template <typename T>
__global__ void transpose_kernel(const T* __restrict__ src, int rows, int cols, T* __restrict__ dst) {
  __shared__ T tile[32][33];
  int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) if (r0 + i < rows && c0 + tx < cols) tile[i][tx] = src[(int64_t)(r0 + i) * cols + c0 + tx];
  __syncthreads();
  for (int i = ty; i < 32; i += 8) if (c0 + i < cols && r0 + tx < rows) dst[(int64_t)(c0 + i) * rows + r0 + tx] = tile[tx][i];
}
template <typename T> void k_transpose(spa3d_ctx* c, const T* src, int rows, int cols, T* dst) {
  if (c->dry) return;
  transpose_kernel<T><<<dim3((unsigned)cdiv(cols, 32), (unsigned)cdiv(rows, 32)), 256, 0, c->stream>>>(src, rows, cols, dst);
  SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// explicit instantiations
// ---------------------------------------------------------------------------------------------
#define INST_EMBED(T) \
  template void k_sin_embed<T>(spa3d_ctx*, const float*, int64_t, int, int, float, T*);                                     \
  template void k_embed_tokens<T>(spa3d_ctx*, const float*, int64_t, int, int, float, T*, int);                             \
  template void k_embed_maps<T>(spa3d_ctx*, const int32_t*, int64_t, int, int, int32_t*, int32_t*, T*, const float*, int);  \
  template void k_set_readout_rows<T>(spa3d_ctx*, T*, const float*, int64_t, int, int);                                     \
  template void k_pack<T>(spa3d_ctx*, const float*, int64_t, int, int, T*, int64_t, T*, int64_t);                           \
  template void k_transpose<T>(spa3d_ctx*, const T*, int, int, T*);
INST_EMBED(float)
INST_EMBED(bf16_t)
// the rank-K kernels move 8 columns per thread in ONE 16-byte access: the 16-bit types only (in float that access is 4 columns wide; no caller ever had a float use)
template bool k_rank_fwd<bf16_t>(spa3d_ctx*, const bf16_t*, const bf16_t*, const float*, bf16_t*, int64_t, int, int, int64_t, int, int);
template bool k_rank_bwd<bf16_t>(spa3d_ctx*, const bf16_t*, const bf16_t*, int64_t, int, int, int64_t, int, int, float*, float*);
}  // namespace SPA_NS
