// layernorm.hip -- LayerNorm forward and backward (gfx950): the scalar kernels for any width, the 16-byte vectorised kernels, and the
// row-partitioned kernels of the two widths the step spends its LayerNorm time on (d = 384, d = 1280).  HBM-bound: a wave (or a part of
// one) per row, coalesced lane-contiguous access.
// T in {float, bf16_t} storage, fp32 math.  References such as attention.py:49 are to the reference implementation's files.
#include <algorithm>

#include "common.hpp"

namespace SPA_NS {

// ---------------------------------------------------------------------------------------------
// LayerNorm (flax nn.LayerNorm(use_bias=False), eps 1e-6, fast variance clamped at 0) attention.py:49,76,103
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const T* __restrict__ x, const float* __restrict__ scale, T* __restrict__ y,
                                                     float* __restrict__ stats, int64_t rows, int d) {
  const int lane = threadIdx.x & 63;
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (; row < rows; row += stride) {
    const T* xr = x + row * d;
    float s = 0.f, ss = 0.f;
    for (int i = lane; i < d; i += 64) { float v = ld(xr + i); s += v; ss += v * v; }
    s = wave_sum(s); ss = wave_sum(ss);
    float mu = s / d;
    float var = fmaxf(ss / d - mu * mu, 0.f);
    float r = rsqrtf(var + 1e-6f);
    if (stats && lane == 0) { stats[row * 2] = mu; stats[row * 2 + 1] = r; }
    T* yr = y + row * d;
    for (int i = lane; i < d; i += 64) st(yr + i, (ld(xr + i) - mu) * r * scale[i]);
  }
}
// dx = [add +] r*(g - mean(g) - xhat*mean(g*xhat)), g = dy*scale ; dscale += sum_rows dy*xhat   
#define LN_MAXJ 32  // d <= 2048
template <typename T>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                     const float* __restrict__ stats, const T* __restrict__ dy, const T* add,
                                                     T* dx, float* __restrict__ dscale, int64_t rows, int d, const DetCfg* det) {
  __shared__ float red[4][64 * LN_MAXJ / 4];  // reused per quarter below
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float acc[LN_MAXJ];
#pragma unroll
  for (int j = 0; j < LN_MAXJ; ++j) acc[j] = 0.f;
  int64_t row = (int64_t)blockIdx.x * 4 + w;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (; row < rows; row += stride) {
    const T* xr = x + row * d;
    const T* dyr = dy + row * d;
    const float mu = stats[row * 2], r = stats[row * 2 + 1];
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
      int i = lane + 64 * j;
      if (i < d) {
        float xh = (ld(xr + i) - mu) * r;
        float dyv = ld(dyr + i);
        float g = dyv * scale[i];
        sg += g; sgx += g * xh;
        acc[j] += dyv * xh;
      }
    }
    sg = wave_sum(sg) / d; sgx = wave_sum(sgx) / d;
    T* dxr = dx + row * d;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
      int i = lane + 64 * j;
      if (i < d) {
        float xh = (ld(xr + i) - mu) * r;
        float g = ld(dyr + i) * scale[i];
        float v = r * (g - sg - xh * sgx);
        if (add) v += ld(add + row * d + i);
        st(dxr + i, v);
      }
    }
  }
  // block reduce acc over the 4 waves, 8 columns-groups at a time to bound LDS
  for (int j0 = 0; j0 < LN_MAXJ; j0 += 8) {
    if (j0 * 64 >= d) break;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) red[w][j * 64 + lane] = acc[j0 + j];
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int i = lane + 64 * (j0 + j);
        if (i < d) {
          float s = red[0][j * 64 + lane] + red[1][j * 64 + lane] + red[2][j * 64 + lane] + red[3][j * 64 + lane];
          grad_add(det_read(det), dscale + i, s);
        }
      }
    }
  }
}
// vectorised variant: 16-byte loads (8 bf16 / 4 f32 per lane per step); lanes own fixed columns so the scale-gradient
// partials stay in registers across the rows a wave walks.  Needs d % VEC == 0 and d <= 2048.
// the 16 bytes of load_vec kept packed (half the registers of the unpacked floats while several rows are in flight)
template <typename T, int NV>
__device__ __forceinline__ void unpack_vec(const uint4& v, float (&f)[NV]) {
  if constexpr (sizeof(T) == 4) { f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w); }
  else { const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = unpack_lo(u[i]); f[2 * i + 1] = unpack_hi(u[i]); } }
}
// forward, vectorised: a wave per row, 16-byte loads held in registers between the statistics and the normalisation (the row is read
// once: the scalar kernel above reads it twice with 2-byte loads and measured 2.2 TB/s), two rows in flight per wave.
template <typename T, int STEPS, int U = 2>
__global__ __launch_bounds__(256) void ln_fwd_vec_kernel(const T* __restrict__ x, const float* __restrict__ scale, T* __restrict__ y,
                                                         float* __restrict__ stats, int64_t rows, int d) {
  constexpr int NV = VecOf<T>::N;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nch = d / NV;
  float sc[STEPS][NV];
#pragma unroll
  for (int s_ = 0; s_ < STEPS; ++s_) {
    const int c = lane + 64 * s_;
#pragma unroll
    for (int j = 0; j < NV; ++j) sc[s_][j] = c < nch ? scale[c * NV + j] : 0.f;
  }
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t row0 = (int64_t)blockIdx.x * 4 + w; row0 < rows; row0 += stride * U) {
    float xv[U][STEPS][NV];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = row0 + u * stride;
#pragma unroll
      for (int s_ = 0; s_ < STEPS; ++s_) {
        const int c = lane + 64 * s_;
        if (row < rows && c < nch) load_vec<T, NV>(x + row * d + c * NV, xv[u][s_]);
        else {
#pragma unroll
          for (int j = 0; j < NV; ++j) xv[u][s_][j] = 0.f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = row0 + u * stride;
      float s = 0.f, ss = 0.f;
#pragma unroll
      for (int s_ = 0; s_ < STEPS; ++s_)
#pragma unroll
        for (int j = 0; j < NV; ++j) { s += xv[u][s_][j]; ss += xv[u][s_][j] * xv[u][s_][j]; }
      s = wave_sum(s); ss = wave_sum(ss);
      const float mu = s / d;
      const float var = fmaxf(ss / d - mu * mu, 0.f);
      const float r = rsqrtf(var + 1e-6f);
      if (row < rows) {
        if (stats && lane == 0) { stats[row * 2] = mu; stats[row * 2 + 1] = r; }
#pragma unroll
        for (int s_ = 0; s_ < STEPS; ++s_) {
          const int c = lane + 64 * s_;
          if (c < nch) {
            float o[NV];
#pragma unroll
            for (int j = 0; j < NV; ++j) o[j] = (xv[u][s_][j] - mu) * r * sc[s_][j];
            store_vec<T, NV>(y + row * d + c * NV, o);
          }
        }
      }
    }
  }
}
// d = LPR * CH * NV: a row per LPR lanes (16 at d = 384, 32 at d = 1280 in 16-bit types), 64 / LPR consecutive rows per wave and step -- every lane
// works (a wave per 768-byte row leaves 16 of 64 lanes idle) and a wave keeps 64 / LPR rows in flight: 4.5 -> 5.2 TB/s at d = 384.
template <typename T, int LPR, int CH>
__global__ __launch_bounds__(256) void ln_fwd_part_kernel(const T* __restrict__ x, const float* __restrict__ scale, T* __restrict__ y,
                                                          float* __restrict__ stats, int64_t rows, int d) {
  constexpr int NV = VecOf<T>::N, RPB = 256 / LPR;
  const int sub = threadIdx.x & (LPR - 1);
  float sc[CH][NV];
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int j = 0; j < NV; ++j) sc[c][j] = scale[(sub + LPR * c) * NV + j];
  for (int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR; row < rows; row += (int64_t)gridDim.x * RPB) {
    uint4 xr[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) xr[c] = *(const uint4*)(x + row * d + (sub + LPR * c) * NV);
    float xv[CH][NV]; float s = 0.f, ss = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      unpack_vec<T, NV>(xr[c], xv[c]);
#pragma unroll
      for (int j = 0; j < NV; ++j) { s += xv[c][j]; ss += xv[c][j] * xv[c][j]; }
    }
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) { s += __shfl_xor(s, o, 64); ss += __shfl_xor(ss, o, 64); }
    const float mu = s / d;
    const float var = fmaxf(ss / d - mu * mu, 0.f);
    const float r = rsqrtf(var + 1e-6f);
    if (stats && sub == 0) { stats[row * 2] = mu; stats[row * 2 + 1] = r; }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      float o[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) o[j] = (xv[c][j] - mu) * r * sc[c][j];
      store_vec<T, NV>(y + row * d + (sub + LPR * c) * NV, o);
    }
  }
}
// backward in the same row partition (d = 384: LPR = 16, CH = 3)
template <typename T, int LPR, int CH>
__global__ __launch_bounds__(256) void ln_bwd_part_kernel(const T* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ stats,
                                                          const T* __restrict__ dy, const T* add, T* dx, float* __restrict__ dscale, int64_t rows, int d,
                                                          const DetCfg* det) {
  constexpr int NV = VecOf<T>::N, RPB = 256 / LPR, DV = LPR * CH * NV;
  __shared__ float red[4][DV];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, sub = threadIdx.x & (LPR - 1);
  float acc[CH][NV], sc[CH][NV];
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int j = 0; j < NV; ++j) { acc[c][j] = 0.f; sc[c][j] = scale[(sub + LPR * c) * NV + j]; }
  for (int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR; row < rows; row += (int64_t)gridDim.x * RPB) {
    uint4 xr[CH], dr[CH], ar[CH];
    const float mu = stats[row * 2], r = stats[row * 2 + 1];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int64_t o = row * d + (sub + LPR * c) * NV;
      xr[c] = *(const uint4*)(x + o); dr[c] = *(const uint4*)(dy + o);
      ar[c] = add ? *(const uint4*)(add + o) : make_uint4(0u, 0u, 0u, 0u);
    }
    float xh[CH][NV], gg[CH][NV]; float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      float xv[NV], dv[NV];
      unpack_vec<T, NV>(xr[c], xv); unpack_vec<T, NV>(dr[c], dv);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        xh[c][j] = (xv[j] - mu) * r; gg[c][j] = dv[j] * sc[c][j];
        sg += gg[c][j]; sgx += gg[c][j] * xh[c][j]; acc[c][j] += dv[j] * xh[c][j];
      }
    }
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) { sg += __shfl_xor(sg, o, 64); sgx += __shfl_xor(sgx, o, 64); }
    sg /= d; sgx /= d;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      float o[NV], av[NV];
      unpack_vec<T, NV>(ar[c], av);
#pragma unroll
      for (int j = 0; j < NV; ++j) o[j] = r * (gg[c][j] - sg - xh[c][j] * sgx) + av[j];
      store_vec<T, NV>(dx + row * d + (sub + LPR * c) * NV, o);
    }
  }
  // scale gradient: the 64 / LPR row groups of a wave, then the four waves, then one atomic per column and workgroup
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      float a = acc[c][j];
#pragma unroll
      for (int o = LPR; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
      if (lane < LPR) red[w][(sub + LPR * c) * NV + j] = a;
    }
  __syncthreads();
  for (int t = threadIdx.x; t < DV; t += 256) grad_add(det_read(det), dscale + t, red[0][t] + red[1][t] + red[2][t] + red[3][t]);
}
template <typename T>
void k_layernorm(spa3d_ctx* c, const T* x, const float* scale, T* y, float* stats, int64_t rows, int d) {
  if (c->dry || rows == 0) return;
  ProfScope ps(c, PROF_LN_FWD, 8.0 * (double)rows * d, (double)rows * d * 2.0 * sizeof(T) + rows * 8.0);  // read x, write y (+ stats)
  ps.tag(rows, d, 0, 0);
  constexpr int NV = VecOf<T>::N;
  const bool al = ((((uintptr_t)x) | ((uintptr_t)y)) & 15) == 0;
  if (d % NV == 0 && al && d <= 64 * NV * 4) {
    constexpr int gcap = 4096;  // measured (tools/bench_ln.py)
    const unsigned g = (unsigned)std::min<int64_t>(cdiv(rows, 8), gcap);
    const int steps = (d / NV + 63) / 64;
    if constexpr (sizeof(T) == 2) {  // the two widths of the step's large LayerNorms: row-partitioned kernels (4.6 -> 5.3 and 3.9 -> 5.2 TB/s)
      if (d == 384) { ln_fwd_part_kernel<T, 16, 3><<<(unsigned)std::min<int64_t>(cdiv(rows, 16), 2 * gcap), 256, 0, c->stream>>>(x, scale, y, stats, rows, d); SPA_LAUNCH_CHECK(c); return; }
      if (d == 1280) { ln_fwd_part_kernel<T, 32, 5><<<(unsigned)std::min<int64_t>(cdiv(rows, 8), 2 * gcap), 256, 0, c->stream>>>(x, scale, y, stats, rows, d); SPA_LAUNCH_CHECK(c); return; }
    }
    if (steps == 1) ln_fwd_vec_kernel<T, 1><<<g, 256, 0, c->stream>>>(x, scale, y, stats, rows, d);  // (four rows in flight per wave measured 3.5 vs 4.4 TB/s: occupancy)
    else if (steps == 2) ln_fwd_vec_kernel<T, 2><<<g, 256, 0, c->stream>>>(x, scale, y, stats, rows, d);
    else if (steps == 3) ln_fwd_vec_kernel<T, 3><<<g, 256, 0, c->stream>>>(x, scale, y, stats, rows, d);
    else ln_fwd_vec_kernel<T, 4><<<g, 256, 0, c->stream>>>(x, scale, y, stats, rows, d);
  } else {
    const unsigned g = (unsigned)std::min<int64_t>(cdiv(rows, 4), 65536);
    ln_fwd_kernel<T><<<g, 256, 0, c->stream>>>(x, scale, y, stats, rows, d);
  }
  SPA_LAUNCH_CHECK(c);
}

template <typename T, int STEPS, int U>
__global__ __launch_bounds__(256) void ln_bwd_vec_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                         const float* __restrict__ stats, const T* __restrict__ dy, const T* add, T* dx,
                                                         float* __restrict__ dscale, int64_t rows, int d, const DetCfg* det) {
  constexpr int NV = VecOf<T>::N;
  __shared__ float red[4][64 * NV];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nch = d / NV;
  float acc[STEPS][NV], sc[STEPS][NV];
#pragma unroll
  for (int s_ = 0; s_ < STEPS; ++s_) {
    const int c = lane + 64 * s_;
#pragma unroll
    for (int j = 0; j < NV; ++j) { acc[s_][j] = 0.f; sc[s_][j] = c < nch ? scale[c * NV + j] : 0.f; }
  }
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t row0 = (int64_t)blockIdx.x * 4 + w; row0 < rows; row0 += stride * U) {
    // every load of U rows (x, dy and the residual-path gradient) is requested before the first is used
    uint4 xr[U][STEPS], dr[U][STEPS], ar[U][STEPS]; float mu[U], r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = row0 + u * stride;
      const bool live = row < rows;
      mu[u] = live ? stats[row * 2] : 0.f; r[u] = live ? stats[row * 2 + 1] : 0.f;
#pragma unroll
      for (int s_ = 0; s_ < STEPS; ++s_) {
        const int c = lane + 64 * s_;
        xr[u][s_] = dr[u][s_] = ar[u][s_] = make_uint4(0u, 0u, 0u, 0u);
        if (live && c < nch) {
          xr[u][s_] = *(const uint4*)(x + row * d + c * NV); dr[u][s_] = *(const uint4*)(dy + row * d + c * NV);
          if (add) ar[u][s_] = *(const uint4*)(add + row * d + c * NV);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = row0 + u * stride;
      float xh[STEPS][NV], gg[STEPS][NV];
      float sg = 0.f, sgx = 0.f;
#pragma unroll
      for (int s_ = 0; s_ < STEPS; ++s_) {
        float xv[NV], dv[NV];
        unpack_vec<T, NV>(xr[u][s_], xv); unpack_vec<T, NV>(dr[u][s_], dv);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          xh[s_][j] = (xv[j] - mu[u]) * r[u]; gg[s_][j] = dv[j] * sc[s_][j];
          sg += gg[s_][j]; sgx += gg[s_][j] * xh[s_][j]; acc[s_][j] += dv[j] * xh[s_][j];
        }
      }
      sg = wave_sum(sg) / d; sgx = wave_sum(sgx) / d;
      if (row < rows) {
#pragma unroll
        for (int s_ = 0; s_ < STEPS; ++s_) {
          const int c = lane + 64 * s_;
          if (c < nch) {
            float o[NV], av[NV];
            unpack_vec<T, NV>(ar[u][s_], av);
#pragma unroll
            for (int j = 0; j < NV; ++j) o[j] = r[u] * (gg[s_][j] - sg - xh[s_][j] * sgx) + av[j];
            store_vec<T, NV>(dx + row * d + c * NV, o);
          }
        }
      }
    }
  }
#pragma unroll
  for (int s_ = 0; s_ < STEPS; ++s_) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV; ++j) red[w][lane * NV + j] = acc[s_][j];
    __syncthreads();
    if (w == 0) {
      const int c = lane + 64 * s_;
      if (c < nch)
#pragma unroll
        for (int j = 0; j < NV; ++j)
          grad_add(det_read(det), dscale + c * NV + j, red[0][lane * NV + j] + red[1][lane * NV + j] + red[2][lane * NV + j] + red[3][lane * NV + j]);
    }
  }
}
template <typename T>
void k_layernorm_bwd(spa3d_ctx* c, const T* x, const float* scale, const float* stats, const T* dy, T* dx, float* dscale,
                     int64_t rows, int d, const T* add) {
  if (c->dry || rows == 0) return;
  ProfScope ps(c, PROF_LN_BWD, 16.0 * (double)rows * d, (double)rows * d * (add ? 4.0 : 3.0) * sizeof(T) + rows * 8.0);  // x, dy, (add), dx
  ps.tag(rows, d, add ? 1 : 0, 0);
  constexpr int gcapb = 1024;
  unsigned g = (unsigned)std::min<int64_t>(cdiv(rows, 4), d <= 512 ? gcapb : 2 * gcapb);  // measured: 1024 blocks at d = 384, 2048 at d = 1280
  // few rows (the latent stacks: 1 408): one block per 4 rows means 352 blocks each adding its d partial sums into the SAME d addresses -- 103 us for 3 MB;
  // 32 rows per block there
  if (rows <= 16384) g = (unsigned)std::min<int64_t>(g, std::max<int64_t>(64, cdiv(rows, 32)));
  constexpr int NV = VecOf<T>::N;
  const bool al = ((((uintptr_t)x) | ((uintptr_t)dy) | ((uintptr_t)dx) | ((uintptr_t)add)) & 15) == 0;
  if (d % NV == 0 && al && d <= 64 * NV * 4) {
    const int steps = (d / NV + 63) / 64;
    if constexpr (sizeof(T) == 2) {  // row-partitioned kernels: 4.9 -> 5.2 TB/s at d = 384 (2.8 -> 5.3 below 0.5 M rows), 4.85 -> 5.45 at d = 1280
      if (d == 384) { ln_bwd_part_kernel<T, 16, 3><<<(unsigned)std::min<int64_t>(cdiv(rows, 16), 2 * gcapb), 256, 0, c->stream>>>(x, scale, stats, dy, add, dx, dscale, rows, d, c->det); SPA_LAUNCH_CHECK(c); return; }
      if (d == 1280) { ln_bwd_part_kernel<T, 32, 5><<<(unsigned)std::min<int64_t>(cdiv(rows, 8), 2 * gcapb), 256, 0, c->stream>>>(x, scale, stats, dy, add, dx, dscale, rows, d, c->det); SPA_LAUNCH_CHECK(c); return; }
    }
    if (steps == 1) ln_bwd_vec_kernel<T, 1, 1><<<g, 256, 0, c->stream>>>(x, scale, stats, dy, add, dx, dscale, rows, d, c->det);  // U = 4 measured 3.7 vs 4.7 TB/s
    else if (steps == 2) ln_bwd_vec_kernel<T, 2, 2><<<g, 256, 0, c->stream>>>(x, scale, stats, dy, add, dx, dscale, rows, d, c->det);
    else if (steps == 3) ln_bwd_vec_kernel<T, 3, 2><<<g, 256, 0, c->stream>>>(x, scale, stats, dy, add, dx, dscale, rows, d, c->det);
    else ln_bwd_vec_kernel<T, 4, 1><<<g, 256, 0, c->stream>>>(x, scale, stats, dy, add, dx, dscale, rows, d, c->det);
  } else {
    ln_bwd_kernel<T><<<g, 256, 0, c->stream>>>(x, scale, stats, dy, add, dx, dscale, rows, d, c->det);
  }
  SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// explicit instantiations
// ---------------------------------------------------------------------------------------------
#define INST_LN(T) \
  template void k_layernorm<T>(spa3d_ctx*, const T*, const float*, T*, float*, int64_t, int);                                        \
  template void k_layernorm_bwd<T>(spa3d_ctx*, const T*, const float*, const float*, const T*, T*, float*, int64_t, int, const T*);
INST_LN(float)
INST_LN(bf16_t)
}  // namespace SPA_NS
