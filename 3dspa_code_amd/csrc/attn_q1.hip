// attn_q1.hip -- single-query attention of a stack's last block, forward and backward (gfx950).
// T in {float, bf16_t} storage, fp32 math.  References such as attention.py:49 are to the reference implementation's files.
#include <algorithm>

#include "common.hpp"

namespace SPA_NS {

// ---------------------------------------------------------------------------------------------
// Single-query attention (last block of the track encoder / readout stack: only token 0 leaves the stack,
// track_autoencoder_3d.py:187-188,286, so only its query row is needed; K/V still come from every token).
// One wave per (sequence, head).  lane = 4*kgrp + part: 16 keys per pass, each key row split over 4 lanes.
// RMSNorm of q/k, 1/sqrt(Dh), key mask, softmax and PV fused; the probabilities are kept (fp32, tiny) for the
// backward.  HBM-bound (K and V are read once): scores live in LDS and the key loop is a runtime loop so the kernels
// stay near 100 VGPRs (the first version unrolled 20 passes over 32-wide arrays: 256 VGPRs, one wave per SIMD, spills).
// CC = channels per lane (Dh/4) at compile time; vec: 16-byte accesses with 16-byte chunk i of a lane = chunk 4*i+part
// of the row, so the 4 lanes of a key touch 64 contiguous bytes per instruction.
// ---------------------------------------------------------------------------------------------
#define Q1_MAXS 320
template <typename T, int CC>
__device__ __forceinline__ int q1_chan(int j, int part, bool vec) {
  constexpr int NV = VecOf<T>::N;
  return vec ? (j / NV) * (4 * NV) + part * NV + (j % NV) : part * CC + j;
}
template <typename T, int CC>
__device__ __forceinline__ void q1_load(const T* p, bool vec, float (&f)[CC], int part) {
  constexpr int NV = VecOf<T>::N;
  if (vec) {
#pragma unroll
    for (int i = 0; i < CC / NV; ++i) {
      float t[NV]; load_vec<T, NV>(p + (4 * i + part) * NV, t);
#pragma unroll
      for (int j = 0; j < NV; ++j) f[i * NV + j] = t[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < CC; ++j) f[j] = ld(p + part * CC + j);
  }
}
template <typename T, int CC>
__device__ __forceinline__ void q1_store(T* p, bool vec, const float (&f)[CC], int part) {
  constexpr int NV = VecOf<T>::N;
  if (vec) {
#pragma unroll
    for (int i = 0; i < CC / NV; ++i) {
      float t[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) t[j] = f[i * NV + j];
      store_vec<T, NV>(p + (4 * i + part) * NV, t);
    }
  } else {
#pragma unroll
    for (int j = 0; j < CC; ++j) st(p + part * CC + j, f[j]);
  }
}
__device__ __forceinline__ float quad_sum(float v) { v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); return v; }
__device__ __forceinline__ float kgrp_sum(float v) {
#pragma unroll
  for (int o = 4; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T, int CC>
__global__ __launch_bounds__(256) void attn_q1_fwd_kernel(const T* __restrict__ q0, int64_t ldq0, const T* __restrict__ k, const T* __restrict__ v,
                                                          int64_t ldk, int64_t ldv, const float* __restrict__ sq, const float* __restrict__ sk,
                                                          const float* __restrict__ km, int64_t nprob, int Smax, int H, T* __restrict__ o0,
                                                          float* __restrict__ p0, int vec_, const int32_t* __restrict__ seq_off) {
  __shared__ float scs[4][Q1_MAXS];
  constexpr int Dh = CC * 4;
  const int lane = threadIdx.x & 63, part = lane & 3, kg = lane >> 2, wv = threadIdx.x >> 6;
  const bool vec = vec_ != 0;
  float* sc = scs[wv];
  const float alpha = rsqrtf((float)Dh);
  float sqv[CC], skv[CC];
#pragma unroll
  for (int j = 0; j < CC; ++j) { const int ch = q1_chan<T, CC>(j, part, vec); sqv[j] = sq[ch]; skv[j] = sk[ch]; }
  for (int64_t prob = (int64_t)blockIdx.x * 4 + wv; prob < nprob; prob += (int64_t)gridDim.x * 4) {
    const int64_t seq = prob / H; const int h = (int)(prob - seq * H);
    // ragged sequences (token pruning): rows [seq_off[seq], seq_off[seq+1]) of the compact tensors; dense otherwise
    const int64_t rowbase = seq_off ? (int64_t)seq_off[seq] : seq * Smax;
    const int S = seq_off ? seq_off[seq + 1] - (int)rowbase : Smax;
    const int nit = (S + 15) / 16;
    float qh[CC];
    q1_load<T, CC>(q0 + seq * ldq0 + h * Dh, vec, qh, part);
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < CC; ++j) ss += qh[j] * qh[j];
    const float rq = rsqrtf(quad_sum(ss) / Dh + 1e-6f);
#pragma unroll
    for (int j = 0; j < CC; ++j) qh[j] *= rq * sqv[j];
    float m = -3.4028234663852886e38f;
#pragma unroll 2
    for (int it = 0; it < nit; ++it) {
      const int key = it * 16 + kg;
      const int kr_ = key < S ? key : S - 1;  // absent keys re-read the last row (keeps the quad shuffles convergent), result unused
      float kv_[CC];
      q1_load<T, CC>(k + (rowbase + kr_) * ldk + h * Dh, vec, kv_, part);
      float ks = 0.f, d = 0.f;
#pragma unroll
      for (int j = 0; j < CC; ++j) { ks += kv_[j] * kv_[j]; d += qh[j] * kv_[j] * skv[j]; }
      ks = quad_sum(ks); d = quad_sum(d);
      float lg = d * rsqrtf(ks / Dh + 1e-6f) * alpha;
      if (km && km[rowbase + kr_] == 0.f) lg = -3.4028234663852886e38f;
      if (key < S) { m = fmaxf(m, lg); if (part == 0) sc[key] = lg; }
    }
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float l = 0.f;
    for (int key = lane; key < S; key += 64) { const float e = expf(sc[key] - m); sc[key] = e; l += e; }  // own-wave LDS, program order
    l = wave_sum(l);
    const float inv = 1.f / l;
    float acc[CC];
#pragma unroll
    for (int j = 0; j < CC; ++j) acc[j] = 0.f;
#pragma unroll 2
    for (int it = 0; it < nit; ++it) {
      const int key = it * 16 + kg;
      if (key < S) {
        const float p = sc[key] * inv;
        if (part == 0) p0[prob * Smax + key] = p;
        float vv[CC];
        q1_load<T, CC>(v + (rowbase + key) * ldv + h * Dh, vec, vv, part);
#pragma unroll
        for (int j = 0; j < CC; ++j) acc[j] += p * vv[j];
      }
    }
#pragma unroll
    for (int j = 0; j < CC; ++j) acc[j] = kgrp_sum(acc[j]);
    if (kg == 0) q1_store<T, CC>(o0 + seq * (int64_t)H * Dh + h * Dh, vec, acc, part);
  }
}
template <typename T>
void k_attn_q1_fwd(spa3d_ctx* c, const T* q0, int64_t ldq0, const T* k, const T* v, int64_t ldk, int64_t ldv, const float* sq, const float* sk,
                   const float* km, int64_t nseq, int S, int H, int Dh, T* o0, float* p0, const int32_t* seq_off) {
  if (c->dry || nseq == 0) return;
  if (S > Q1_MAXS || Dh % 4 || Dh > 128) { if (!c->hip_err) { c->hip_err = -3; c->err = "attn_q1: S <= 320 and Dh % 4 == 0, Dh <= 128 required"; } return; }
  const int64_t nprob = nseq * H;
  ProfScope ps(c, PROF_ATTN_Q1, 4.0 * (double)nprob * S * Dh, (double)nprob * S * Dh * 2.0 * sizeof(T) + (double)nprob * S * 4.0);  // K, V once (+ p0)
  ps.tag(nseq, S, H, 0);
  unsigned g = (unsigned)std::min<int64_t>(cdiv(nprob, 4), 8192);
  constexpr int NV = VecOf<T>::N;
  const int vec = (Dh % (4 * NV) == 0 && ldk % NV == 0 && ldv % NV == 0 && ldq0 % NV == 0 &&
                   ((((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)q0) | ((uintptr_t)o0)) & 15) == 0) ? 1 : 0;
#define Q1F(CCv) attn_q1_fwd_kernel<T, CCv><<<g, 256, 0, c->stream>>>(q0, ldq0, k, v, ldk, ldv, sq, sk, km, nprob, S, H, o0, p0, vec, seq_off)
  switch (Dh / 4) { case 24: Q1F(24); break; case 16: Q1F(16); break; case 32: Q1F(32); break; case 8: Q1F(8); break; case 4: Q1F(4); break;
    case 2: Q1F(2); break; default: if (!c->hip_err) { c->hip_err = -3; c->err = "attn_q1: unsupported head width"; } return; }
#undef Q1F
  SPA_LAUNCH_CHECK(c);
}

// backward of the above: dq0 [nseq, H*Dh]; dk, dv for EVERY key row (overwritten); scale gradients accumulated.
// With x^ the RMS-normalised rows, q^ = x^_q*s_q, k^ = x^_k*s_k and ds_k = p_k (dp_k - sum p dp) / sqrt(Dh):
//   u = sum_k ds_k x^_k  gives both  dq^ = u*s_k  and  ds_k(scale) = q^*u;   dk^_k = ds_k q^;  dv_k = p_k dO.
// Registers: q^, dO, u (+ one key row); the scales and the scale-gradient accumulators live in LDS.
template <typename T, int CC, bool DET = false>  // DET: deterministic-gradient mode (common.hpp): the scale gradients accumulate as 64-bit fixed point, in LDS and in the shadow
__global__ __launch_bounds__(256) void attn_q1_bwd_kernel(const T* __restrict__ q0, int64_t ldq0, const T* __restrict__ k, const T* __restrict__ v,
                                                          int64_t ldk, int64_t ldv, const float* __restrict__ sq, const float* __restrict__ sk,
                                                          const float* __restrict__ km, int64_t nprob, int Smax, int H,
                                                          const float* __restrict__ p0, const T* __restrict__ d_o0, T* __restrict__ dq0,
                                                          T* __restrict__ dk, T* __restrict__ dv, float* __restrict__ dsq, float* __restrict__ dsk,
                                                          int vec_, const int32_t* __restrict__ seq_off, const DetCfg* det) {
  __shared__ float dps[4][Q1_MAXS];
  __shared__ float scl[2][4 * CC];  // s_q, s_k in lane-channel order [part][j]
  __shared__ float red[2][4 * CC];  // block accumulators of d s_q, d s_k
  __shared__ unsigned long long redq[DET ? 2 : 1][DET ? 4 * CC : 1];  // DET: the same in the shadow's fixed point (integer LDS atomics do not depend on arrival order)
  constexpr int Dh = CC * 4;
  constexpr int NV = VecOf<T>::N;
  constexpr int G = (CC % NV == 0) ? NV : 1;  // output chunk; vec implies G == NV
  const int lane = threadIdx.x & 63, part = lane & 3, kg = lane >> 2, wv = threadIdx.x >> 6;
  const bool vec = vec_ != 0;
  float* dp = dps[wv];
  const float* sql = scl[0] + part * CC;
  const float* skl = scl[1] + part * CC;
  const float alpha = rsqrtf((float)Dh);
  for (int t = threadIdx.x; t < 4 * CC; t += 256) {
    const int pt = t / CC, j = t - pt * CC;
    const int ch = q1_chan<T, CC>(j, pt, vec);
    scl[0][t] = sq[ch]; scl[1][t] = sk[ch]; red[0][t] = 0.f; red[1][t] = 0.f;
    if constexpr (DET) { redq[0][t] = 0ull; redq[1][t] = 0ull; }
  }
  DetCfg dc{};
  float qlim = 0.f;
  if constexpr (DET) {   // the unit and the overflow flag of the call (common.hpp DetCfg)
    dc = det_read(det);
    // one redq entry takes one addend per problem of this workgroup: bounding each by 2^62 / (that count) keeps the LDS sum below 2^62, so it cannot wrap
    const int64_t per = 4 * ((nprob + 4 * (int64_t)gridDim.x - 1) / (4 * (int64_t)gridDim.x));
    qlim = fminf(DET_ADDEND_MAX, 4.6116860184273879e18f / (float)(per > 0 ? per : 1));
  }
  __syncthreads();
  for (int64_t prob = (int64_t)blockIdx.x * 4 + wv; prob < nprob; prob += (int64_t)gridDim.x * 4) {
    const int64_t seq = prob / H; const int h = (int)(prob - seq * H);
    // ragged sequences (token pruning): rows [seq_off[seq], seq_off[seq+1]) of the compact tensors; dense otherwise
    const int64_t rowbase = seq_off ? (int64_t)seq_off[seq] : seq * Smax;
    const int S = seq_off ? seq_off[seq + 1] - (int)rowbase : Smax;
    const int nit = (S + 15) / 16;
    float qs[CC], dout[CC];
    q1_load<T, CC>(q0 + seq * ldq0 + h * Dh, vec, qs, part);
    q1_load<T, CC>(d_o0 + seq * (int64_t)H * Dh + h * Dh, vec, dout, part);
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < CC; ++j) ss += qs[j] * qs[j];
    const float rq = rsqrtf(quad_sum(ss) / Dh + 1e-6f);
#pragma unroll
    for (int j = 0; j < CC; ++j) qs[j] *= rq * sql[j];  // q^
    // pass 1: dp_k = dO . V_k (to LDS) and sum_k p_k dp_k
    float pd = 0.f;
#pragma unroll 2
    for (int it = 0; it < nit; ++it) {
      const int key = it * 16 + kg;
      const int kr_ = key < S ? key : S - 1;
      float vv[CC];
      q1_load<T, CC>(v + (rowbase + kr_) * ldv + h * Dh, vec, vv, part);
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < CC; ++j) d += dout[j] * vv[j];
      d = quad_sum(d);
      if (key < S && part == 0) { dp[key] = d; pd += p0[prob * Smax + key] * d; }
    }
    pd = wave_sum(pd);
    // pass 2: per key dv, dk (through the RMSNorm) and u
    float u[CC];
#pragma unroll
    for (int j = 0; j < CC; ++j) u[j] = 0.f;
    for (int it = 0; it < nit; ++it) {
      const int key = it * 16 + kg;
      const bool valid = key < S;
      const int kr_ = valid ? key : S - 1;
      const int64_t roff = rowbase + kr_;
      float xk[CC];
      q1_load<T, CC>(k + roff * ldk + h * Dh, vec, xk, part);
      float ks = 0.f;
#pragma unroll
      for (int j = 0; j < CC; ++j) ks += xk[j] * xk[j];
      const float rk = rsqrtf(quad_sum(ks) / Dh + 1e-6f);
      const float p = valid ? p0[prob * Smax + kr_] : 0.f;
      const bool keep = !(km && km[rowbase + kr_] == 0.f);
      const float ds = (valid && keep) ? p * (dp[kr_] - pd) * alpha : 0.f;  // where() passes no gradient to masked logits
      float gx = 0.f;
#pragma unroll
      for (int j = 0; j < CC; ++j) {
        xk[j] *= rk;                          // x^ of the key row
        u[j] += ds * xk[j];
        gx += qs[j] * skl[j] * xk[j];         // (dk^ * s_k) . x^ / ds
      }
      gx = quad_sum(gx) * ds / Dh;
      if (valid) {
        T* dkr = dk + roff * ldk + h * Dh;
        T* dvr = dv + roff * ldv + h * Dh;
#pragma unroll
        for (int i = 0; i < CC / G; ++i) {
          float ok[G], ov[G];
#pragma unroll
          for (int jj = 0; jj < G; ++jj) {
            const int j = i * G + jj;
            ok[jj] = rk * (ds * qs[j] * skl[j] - xk[j] * gx);
            ov[jj] = p * dout[j];
          }
          if (vec) {
            store_vec<T, G>(dkr + (4 * i + part) * G, ok);
            store_vec<T, G>(dvr + (4 * i + part) * G, ov);
          } else {
#pragma unroll
            for (int jj = 0; jj < G; ++jj) { st(dkr + part * CC + i * G + jj, ok[jj]); st(dvr + part * CC + i * G + jj, ov[jj]); }
          }
        }
      }
    }
    // query side: dq^ = u*s_k; d s_k += q^*u; d s_q += dq^ * x^_q; dq through the RMSNorm
    float xq[CC];
    q1_load<T, CC>(q0 + seq * ldq0 + h * Dh, vec, xq, part);
    float gq = 0.f;
#pragma unroll
    for (int j = 0; j < CC; ++j) {
      u[j] = kgrp_sum(u[j]);
      xq[j] *= rq;
      gq += u[j] * skl[j] * sql[j] * xq[j];
    }
    gq = quad_sum(gq) / Dh;
    if (kg == 0) {
#pragma unroll
      for (int j = 0; j < CC; ++j) {
        const float dqh = u[j] * skl[j];
        // (deterministic mode: LDS float atomics depend on arrival order too -- every contribution goes straight to the fixed-point shadow)
        if constexpr (DET) {
          const float fk = qs[j] * u[j] * dc.scale, fq = dqh * xq[j] * dc.scale;   // grad_add's per-addend bound, tightened to the workgroup's count (NaN fails it too)
          if (fabsf(fk) < qlim && fabsf(fq) < qlim) {
            atomicAdd(&redq[1][part * CC + j], (unsigned long long)__float2ll_rn(fk));
            atomicAdd(&redq[0][part * CC + j], (unsigned long long)__float2ll_rn(fq));
          } else atomicOr(dc.flag, 1u);
        } else { atomicAdd(&red[1][part * CC + j], qs[j] * u[j]); atomicAdd(&red[0][part * CC + j], dqh * xq[j]); }
        xq[j] = rq * (dqh * sql[j] - xq[j] * gq);
      }
      q1_store<T, CC>(dq0 + seq * (int64_t)H * Dh + h * Dh, vec, xq, part);
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 4 * CC; t += 256) {
    const int pt = t / CC, j = t - pt * CC;
    const int ch = q1_chan<T, CC>(j, pt, vec);
    if constexpr (DET) {  // the workgroup's exact integer sums go to the shadow as they are (|sum| >= 2^62: the flag)
      grad_add_q(dc, dsq + ch, (long long)redq[0][t]); grad_add_q(dc, dsk + ch, (long long)redq[1][t]);
    } else { atomicAdd(dsq + ch, red[0][t]); atomicAdd(dsk + ch, red[1][t]); }
  }
}
template <typename T>
void k_attn_q1_bwd(spa3d_ctx* c, const T* q0, int64_t ldq0, const T* k, const T* v, int64_t ldk, int64_t ldv, const float* sq, const float* sk,
                   const float* km, int64_t nseq, int S, int H, int Dh, const float* p0, const T* d_o0, T* dq0, T* dk, T* dv, float* dsq,
                   float* dsk, const int32_t* seq_off) {
  if (c->dry || nseq == 0) return;
  if (S > Q1_MAXS || Dh % 4 || Dh > 128) { if (!c->hip_err) { c->hip_err = -3; c->err = "attn_q1: S <= 320 and Dh % 4 == 0, Dh <= 128 required"; } return; }
  const int64_t nprob = nseq * H;
  ProfScope ps(c, PROF_ATTN_Q1, 8.0 * (double)nprob * S * Dh, (double)nprob * S * Dh * 4.0 * sizeof(T) + (double)nprob * S * 4.0);  // K, V read; dK, dV written
  ps.tag(nseq, S, H, 1);
  unsigned g = (unsigned)std::min<int64_t>(cdiv(nprob, 4), 4096);
  constexpr int NV = VecOf<T>::N;
  const int vec = (Dh % (4 * NV) == 0 && ldk % NV == 0 && ldv % NV == 0 && ldq0 % NV == 0 &&
                   ((((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)dk) | ((uintptr_t)dv) | ((uintptr_t)q0) | ((uintptr_t)d_o0) |
                     ((uintptr_t)dq0)) & 15) == 0) ? 1 : 0;
#define Q1B(CCv) do { if (c->det) attn_q1_bwd_kernel<T, CCv, true><<<g, 256, 0, c->stream>>>(q0, ldq0, k, v, ldk, ldv, sq, sk, km, nprob, S, H, p0, d_o0, dq0, dk, dv, dsq, dsk, vec, seq_off, c->det); \
                      else attn_q1_bwd_kernel<T, CCv, false><<<g, 256, 0, c->stream>>>(q0, ldq0, k, v, ldk, ldv, sq, sk, km, nprob, S, H, p0, d_o0, dq0, dk, dv, dsq, dsk, vec, seq_off, c->det); } while (0)
  switch (Dh / 4) { case 24: Q1B(24); break; case 16: Q1B(16); break; case 32: Q1B(32); break; case 8: Q1B(8); break; case 4: Q1B(4); break;
    case 2: Q1B(2); break; default: if (!c->hip_err) { c->hip_err = -3; c->err = "attn_q1: unsupported head width"; } return; }
#undef Q1B
  SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// explicit instantiations
// ---------------------------------------------------------------------------------------------
#define INST_Q1(T) \
  template void k_attn_q1_fwd<T>(spa3d_ctx*, const T*, int64_t, const T*, const T*, int64_t, int64_t, const float*, const float*,            \
                                 const float*, int64_t, int, int, int, T*, float*, const int32_t*);                                          \
  template void k_attn_q1_bwd<T>(spa3d_ctx*, const T*, int64_t, const T*, const T*, int64_t, int64_t, const float*, const float*,            \
                                 const float*, int64_t, int, int, int, const float*, const T*, T*, T*, T*, float*, float*, const int32_t*);
INST_Q1(float)
INST_Q1(bf16_t)
}  // namespace SPA_NS
