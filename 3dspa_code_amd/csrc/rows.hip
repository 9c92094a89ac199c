// rows.hip -- row plumbing of the hot path (gfx950): fills, casts, column sums, row movers (strided, by index), the token-pruning plan,
// the shared latent rows of the readout stack's first block, readout sequence assembly, the parameter-row broadcast and its gradient, and
// TRAJAN's visible-frame pooling.  Element-wise, HBM-bound kernels, 16 bytes per thread where the shape allows.
// T in {float, bf16_t} storage, fp32 math.  References such as attention.py:49 are to the reference implementation's files.
// Each launcher (fills and casts apart) is callable on its own -- spa3d_op_colsum, spa3d_op_rows, spa3d_op_prune_plan, spa3d_op_share_plan,
// spa3d_op_share_rows, spa3d_op_assemble_readout(_bwd), spa3d_op_broadcast_rows, spa3d_op_bcast_grad, spa3d_op_vis_mean_pool(_bwd) in ops.hip -- and
// tests/test_gpu_rows.py pins every branch below against tests/rows_util.py: copies bit for bit, plans integer for integer, sums element by element.
// Not reached there: the second grid-stride pass of the 1-D kernels (GRID1D caps a grid at 2^20 workgroups, 2^28 items a pass) and the
// nchunk >= 2^31 fallback of k_assemble_readout.  rows_idx mode 2 (scatter-add) is a plain read-modify-write: it is specified for UNIQUE indices only.
#include <algorithm>

#include "common.hpp"

namespace SPA_NS {

// ---------------------------------------------------------------------------------------------
// fills, products, casts, column sums
// ---------------------------------------------------------------------------------------------
void k_zero(spa3d_ctx* c, void* p, int64_t bytes) {
  if (c->dry || bytes == 0) return;
  hipError_t e = hipMemsetAsync(p, 0, (size_t)bytes, c->stream);
  if (e != hipSuccess && !c->hip_err) { c->hip_err = (int)e; c->err = std::string("hipMemsetAsync: ") + hipGetErrorString(e); }
}
// dst[0..n) = host values, passed BY VALUE in the launch arguments (32 per launch): no host-to-device copy, nothing borrowed from the caller
struct I32x32 { int32_t v[32]; };
__global__ void set_i32_kernel(int32_t* __restrict__ dst, I32x32 a, int n) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 32; ++i) if (t == i && i < n) dst[i] = a.v[i];
}
void k_set_i32(spa3d_ctx* c, int32_t* dst, const int32_t* host, int64_t n) {
  if (c->dry) return;
  for (int64_t i0 = 0; i0 < n; i0 += 32) {
    I32x32 a; const int m = (int)std::min<int64_t>(32, n - i0);
    for (int i = 0; i < 32; ++i) a.v[i] = i < m ? host[i0 + i] : 0;
    set_i32_kernel<<<1, 64, 0, c->stream>>>(dst + i0, a, m);
  }
  SPA_LAUNCH_CHECK(c);
}
__global__ void mul_kernel(float* __restrict__ a, const float* __restrict__ b, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) a[i] *= b[i];
}
void k_mul(spa3d_ctx* c, float* a, const float* b, int64_t n) {
  if (c->dry || n == 0) return;
  mul_kernel<<<GRID1D(n, 256), 256, 0, c->stream>>>(a, b, n); SPA_LAUNCH_CHECK(c);
}
template <typename T>
__global__ void cast_from_f32_kernel(const float* __restrict__ s, T* __restrict__ d, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) st(d + i, s[i]);
}
template <typename T> void k_cast_from_f32(spa3d_ctx* c, const float* s, T* d, int64_t n) {
  if (c->dry || n == 0) return;
  cast_from_f32_kernel<T><<<GRID1D(n, 256), 256, 0, c->stream>>>(s, d, n); SPA_LAUNCH_CHECK(c);
}
template <typename T>
__global__ void cast_to_f32_kernel(const T* __restrict__ s, float* __restrict__ d, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) d[i] = ld(s + i);
}
template <typename T> void k_cast_to_f32(spa3d_ctx* c, const T* s, float* d, int64_t n) {
  if (c->dry || n == 0) return;
  cast_to_f32_kernel<T><<<GRID1D(n, 256), 256, 0, c->stream>>>(s, d, n); SPA_LAUNCH_CHECK(c);
}
template <typename T>
__global__ void colsum_kernel(const T* __restrict__ x, int64_t rows, int n, int64_t ld_, float* __restrict__ out, int64_t rows_per_block,
                              int rgroup, int rskip, const DetCfg* det) {
  // block (64 cols x 4 row-lanes); grid (ceil(n/64), row_splits)
  __shared__ float red[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6;
  int64_t r0 = (int64_t)blockIdx.y * rows_per_block, r1 = std::min<int64_t>(rows, r0 + rows_per_block);
  float s = 0.f;
  if (col < n) for (int64_t r = r0 + w; r < r1; r += 4) {
    int64_t pr = r; if (rgroup > 0) pr = r + (r / rgroup + 1) * (int64_t)rskip;
    s += ld(x + pr * ld_ + col);
  }
  red[w][threadIdx.x & 63] = s;
  __syncthreads();
  if (w == 0 && col < n) grad_add(det_read(det), out + col, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}
// vectorised: a thread owns one 16-byte column chunk and walks rows; block = 32 chunks x 8 row lanes
template <typename T>
__global__ __launch_bounds__(256) void colsum_vec_kernel(const T* __restrict__ x, int64_t rows, int n, int64_t ld_, float* __restrict__ out,
                                                         int64_t rows_per_block, int rgroup, int rskip, const DetCfg* det) {
  constexpr int NV = VecOf<T>::N;
  __shared__ float red[8][32 * NV];
  const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
  const int ch = blockIdx.x * 32 + cx;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block, r1 = std::min<int64_t>(rows, r0 + rows_per_block);
  float a[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) a[j] = 0.f;
  if (ch * NV < n)
    for (int64_t r = r0 + ry; r < r1; r += 8) {
      int64_t pr = r; if (rgroup > 0) pr = r + (r / rgroup + 1) * (int64_t)rskip;
      float v[NV]; load_vec<T, NV>(x + pr * ld_ + ch * NV, v);
#pragma unroll
      for (int j = 0; j < NV; ++j) a[j] += v[j];
    }
#pragma unroll
  for (int j = 0; j < NV; ++j) red[ry][cx * NV + j] = a[j];
  __syncthreads();
  if (ry == 0 && ch * NV < n)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      float s_ = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) s_ += red[k][cx * NV + j];
      grad_add(det_read(det), out + ch * NV + j, s_);
    }
}
template <typename T>
void k_colsum(spa3d_ctx* c, const T* x, int64_t rows, int n, int64_t ld_, float* out, int rgroup, int rskip) {
  if (c->dry || rows == 0) return;
  constexpr int NV = VecOf<T>::N;
  if (n % NV == 0 && ld_ % NV == 0 && (((uintptr_t)x) & 15) == 0) {
    const int64_t gx = cdiv(n / NV, 32);
    int64_t sp = std::max<int64_t>(1, std::min<int64_t>(cdiv(rows, 64), 2048 / gx + 1));   // (was rows / 512: at 1 408 rows three row splits, 59 dependent loads per thread)
    int64_t rpb_ = cdiv(rows, sp);
    colsum_vec_kernel<T><<<dim3((unsigned)gx, (unsigned)cdiv(rows, rpb_)), 256, 0, c->stream>>>(x, rows, n, ld_, out, rpb_, rgroup, rskip, c->det);
    SPA_LAUNCH_CHECK(c);
    return;
  }
  int64_t splits = std::max<int64_t>(1, std::min<int64_t>(cdiv(rows, 256), 1024 / std::max<int64_t>(1, cdiv(n, 64)) + 1));
  int64_t rpb = cdiv(rows, splits);
  colsum_kernel<T><<<dim3((unsigned)cdiv(n, 64), (unsigned)cdiv(rows, rpb)), 256, 0, c->stream>>>(x, rows, n, ld_, out, rpb, rgroup, rskip, c->det);
  SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// row movers
// ---------------------------------------------------------------------------------------------
// dst[i][:] = src[i*stride_rows][:]
template <typename T>
__global__ void gather_rows_kernel(const T* __restrict__ src, int64_t srows, T* __restrict__ dst, int64_t n, int d) {
  const int64_t tot = n * d;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    int64_t r = i / d; int j = (int)(i - r * d);
    dst[i] = src[r * srows * d + j];
  }
}
template <typename T> void k_gather_rows(spa3d_ctx* c, const T* src, int64_t srows, T* dst, int64_t n, int d) {
  if (c->dry || n == 0) return;
  gather_rows_kernel<T><<<GRID1D(n * d, 256), 256, 0, c->stream>>>(src, srows, dst, n, d); SPA_LAUNCH_CHECK(c);
}
// rows by index, 16 bytes per thread: MODE 0 dst[i] = src[idx[i]] (gather), 1 dst[idx[i]] = src[i] (scatter), 2 dst[idx[i]] += src[i]
template <typename T, int MODE>
__global__ void rows_idx_kernel(const T* __restrict__ src, const int32_t* __restrict__ idx, T* __restrict__ dst, int64_t n, int d) {
  constexpr int NV = VecOf<T>::N;
  const int cpr = d / NV;  // 16-byte chunks per row (host: d % NV == 0)
  const int64_t tot = n * cpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cpr; const int ch = (int)(i - r * cpr);
    const int64_t other = idx[r];
    const int64_t so = (MODE == 0 ? other : r) * d + ch * NV, dofs = (MODE == 0 ? r : other) * d + ch * NV;
    if constexpr (MODE == 2) {
      float a[NV], b[NV];
      load_vec<T, NV>(src + so, a); load_vec<T, NV>(dst + dofs, b);
#pragma unroll
      for (int j = 0; j < NV; ++j) b[j] += a[j];
      store_vec<T, NV>(dst + dofs, b);
    } else {
      *(uint4*)(dst + dofs) = *(const uint4*)(src + so);
    }
  }
}
template <typename T> void k_rows_idx(spa3d_ctx* c, int mode, const T* src, const int32_t* idx, T* dst, int64_t n, int d) {
  if (c->dry || n == 0) return;
  constexpr int NV = VecOf<T>::N;
  if (d % NV) { if (!c->hip_err) { c->hip_err = -5; c->err = "rows_idx: row width must be a multiple of 16 bytes"; } return; }
  const dim3 g = GRID1D(n * (d / NV), 256);
  if (mode == 0) rows_idx_kernel<T, 0><<<g, 256, 0, c->stream>>>(src, idx, dst, n, d);
  else if (mode == 1) rows_idx_kernel<T, 1><<<g, 256, 0, c->stream>>>(src, idx, dst, n, d);
  else rows_idx_kernel<T, 2><<<g, 256, 0, c->stream>>>(src, idx, dst, n, d);
  SPA_LAUNCH_CHECK(c);
}
// dst[i*stride_rows][:] += src[i][:]
template <typename T>
__global__ void add_rows_strided_kernel(T* __restrict__ dst, const T* __restrict__ src, int64_t drows, int64_t n, int d) {
  const int64_t tot = n * d;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    int64_t r = i / d; int j = (int)(i - r * d);
    T* p = dst + r * drows * d + j;
    st(p, ld(p) + ld(src + i));
  }
}
template <typename T> void k_add_rows_strided(spa3d_ctx* c, T* dst, const T* src, int64_t drows, int64_t n, int d) {
  if (c->dry || n == 0) return;
  add_rows_strided_kernel<T><<<GRID1D(n * d, 256), 256, 0, c->stream>>>(dst, src, drows, n, d); SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// Token pruning of the track encoder (3DSPA model, 16-bit fused path).  A frame token whose key is masked (occluded, or at / past
// boundary_frame: track_autoencoder_3d.py:167-184) is never attended to, and only token 0 leaves the encoder (:187-188), so a masked
// token's own row influences nothing: the stack runs on COMPACTED, ragged sequences (token 0 + the visible frames, in time order).
//   seq_off [nseq + 1]  first compact row of every sequence (exclusive scan of the kept counts; seq_off[nseq] = kept rows in all)
//   row_src [kept]      dense row (seq * S + t) behind every compact row
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prune_count_kernel(const float* __restrict__ km, int64_t nseq, int S, int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  for (int64_t seq = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); seq < nseq; seq += (int64_t)gridDim.x * 4) {
    int n = 0;
    for (int t = lane; t < S; t += 64) n += km[seq * S + t] != 0.f ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) cnt[seq] = n;
  }
}
// exclusive scan of cnt[0..n) into off[0..n] by ONE workgroup (n <= a few hundred thousand sequences): per-thread chunk sums, a block
// scan of the 1024 partials, then the chunk is re-walked.  off may alias cnt only if they are the same buffer shifted: they are not.
__global__ __launch_bounds__(1024) void prune_scan_kernel(const int32_t* __restrict__ cnt, int64_t n, int32_t* __restrict__ off) {
  __shared__ int32_t part[1024];
  const int tid = threadIdx.x;
  const int64_t per = (n + 1023) / 1024, a = tid * per, b = a + per < n ? a + per : n;
  int32_t s = 0;
  for (int64_t i = a; i < b; ++i) s += cnt[i];
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int32_t v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int32_t run = tid ? part[tid - 1] : 0;
  for (int64_t i = a; i < b; ++i) { off[i] = run; run += cnt[i]; }
  if (tid == 1023) off[n] = part[1023];
}
__global__ __launch_bounds__(256) void prune_fill_kernel(const float* __restrict__ km, int64_t nseq, int S, const int32_t* __restrict__ off,
                                                         int32_t* __restrict__ row_src) {
  const int lane = threadIdx.x & 63;
  for (int64_t seq = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); seq < nseq; seq += (int64_t)gridDim.x * 4) {
    int base = off[seq];
    for (int t0 = 0; t0 < S; t0 += 64) {
      const int t = t0 + lane;
      const bool keep = t < S && km[seq * S + t] != 0.f;
      const unsigned long long m = __ballot(keep);
      if (keep) row_src[base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)(seq * S + t);
      base += __popcll(m);
    }
  }
}
// returns the number of kept rows (ONE stream synchronisation: the row count sizes every launch that follows); dense count when dry
int64_t k_prune_plan(spa3d_ctx* c, const float* km, int64_t nseq, int S, int32_t* cnt, int32_t* seq_off, int32_t* row_src) {
  if (c->dry) return nseq * S;
  if (nseq == 0) return 0;   // a grid of no workgroups is a launch error; no model call gets here (nseq = samples x tracks, both >= 1), spa3d_op_prune_plan does
  prune_count_kernel<<<(unsigned)std::min<int64_t>(cdiv(nseq, 4), 8192), 256, 0, c->stream>>>(km, nseq, S, cnt); SPA_LAUNCH_CHECK(c);
  prune_scan_kernel<<<1, 1024, 0, c->stream>>>(cnt, nseq, seq_off); SPA_LAUNCH_CHECK(c);
  prune_fill_kernel<<<(unsigned)std::min<int64_t>(cdiv(nseq, 4), 8192), 256, 0, c->stream>>>(km, nseq, S, seq_off, row_src); SPA_LAUNCH_CHECK(c);
  int32_t kept = 0;
  if (hipMemcpyAsync(&kept, seq_off + nseq, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    if (!c->hip_err) { c->hip_err = -4; c->err = "prune plan: reading the kept-row count failed"; }
    return nseq * S;
  }
  return kept;
}

// ---------------------------------------------------------------------------------------------
// Shared latent rows of the readout stack's first block (track_autoencoder_3d.py:276-285, 235-246): token n >= 1 of the sequence of
// query (b, q) is [lat[b][n] | lat[b][n][5 t_q : 5 t_q + 128]] -- a function of (b, n, t_q) only, so every query of a sample with the same
// frame t_q carries the same 128 latent rows into the block's LayerNorm and QKV projection.  A "slot" is a distinct (sample, frame)
// pair; the block runs LN1 / QKV (and their backward) once per slot and expands / reduces through the slot index (model.hip, Share).
// ---------------------------------------------------------------------------------------------
// per sample: slot_local[q] = rank of q's frame among the distinct frames of the sample (order of first occurrence); nslot_b[b] = their number
__global__ __launch_bounds__(256) void share_plan_kernel(const int32_t* __restrict__ qframe, int Q, int32_t* __restrict__ slot, int32_t* __restrict__ nslot_b,
                                                         int32_t* __restrict__ first_q) {
  extern __shared__ int32_t sh[];  // [Q] first occurrence of q's frame, then its rank
  const int b = blockIdx.x;
  const int32_t* fr = qframe + (int64_t)b * Q;
  for (int q = threadIdx.x; q < Q; q += 256) {
    const int32_t f = fr[q];
    int first = q;
    for (int p = 0; p < q; ++p) if (fr[p] == f) { first = p; break; }
    sh[q] = first;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int q = 0; q < Q; ++q) {
      if (sh[q] == q) { first_q[(int64_t)b * Q + n] = q; sh[q] = -(n + 1); ++n; }  // firsts carry -(rank + 1)
    }
    nslot_b[b] = n;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < Q; q += 256) {
    const int32_t v = sh[q];
    slot[(int64_t)b * Q + q] = v < 0 ? -v - 1 : -sh[v] - 1;  // local rank; made global by share_plan_finish_kernel
  }
}
// prefix over samples: slot -> global slot index; slot_b / slot_f / slot_q0: sample, frame and first member sequence of every slot; total[0] = number of slots
__global__ __launch_bounds__(256) void share_plan_finish_kernel(const int32_t* __restrict__ qframe, int B, int Q, int32_t* __restrict__ slot,
                                                                const int32_t* __restrict__ nslot_b, const int32_t* __restrict__ first_q,
                                                                int32_t* __restrict__ slot_b, int32_t* __restrict__ slot_f, int32_t* __restrict__ slot_q0,
                                                                int32_t* __restrict__ total) {
  __shared__ int32_t off[1025];
  if (threadIdx.x == 0) { int a = 0; for (int b = 0; b < B; ++b) { off[b] = a; a += nslot_b[b]; } off[B] = a; total[0] = a; }
  __syncthreads();
  for (int64_t i = threadIdx.x; i < (int64_t)B * Q; i += 256) {
    const int b = (int)(i / Q), j = (int)(i - (int64_t)b * Q);
    slot[i] += off[b];
    if (j < nslot_b[b]) { slot_b[off[b] + j] = b; slot_f[off[b] + j] = qframe[(int64_t)b * Q + first_q[i]]; slot_q0[off[b] + j] = b * Q + first_q[i]; }
  }
}
// returns the number of slots (ONE stream synchronisation); B * Q (every query its own slot) when dry
int64_t k_share_plan(spa3d_ctx* c, const int32_t* qframe, int64_t B, int Q, int32_t* slot, int32_t* slot_b, int32_t* slot_f, int32_t* slot_q0,
                     int32_t* scratch /*[B*Q + B + 1]*/) {
  if (c->dry) return B * Q;
  if (B > 1024 || Q > 12288) return B * Q;  // outside the plan kernels' LDS tables: every query its own slot, i.e. the caller keeps the dense path
  int32_t* first_q = scratch; int32_t* nslot_b = scratch + B * Q; int32_t* total = nslot_b + B;
  share_plan_kernel<<<(unsigned)B, 256, Q * sizeof(int32_t), c->stream>>>(qframe, Q, slot, nslot_b, first_q); SPA_LAUNCH_CHECK(c);
  share_plan_finish_kernel<<<1, 256, 0, c->stream>>>(qframe, (int)B, Q, slot, nslot_b, first_q, slot_b, slot_f, slot_q0, total); SPA_LAUNCH_CHECK(c);
  int32_t n = 0;
  if (hipMemcpyAsync(&n, total, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
    if (!c->hip_err) { c->hip_err = -4; c->err = "share plan: reading the slot count failed"; }
    return B * Q;
  }
  return n;
}
// xU = [nslot * L latent rows | B*Q query-token rows]: the distinct rows of the readout sequences (assemble_vec_kernel's values)
template <typename T>
__global__ void share_assemble_kernel(const T* __restrict__ qtok, const T* __restrict__ lat, const int32_t* __restrict__ slot_b,
                                      const int32_t* __restrict__ slot_f, int64_t nslot, int64_t BQ, int L, int Cl, int D, T* __restrict__ xU) {
  constexpr int NV = VecOf<T>::N;
  const int cpr = D / NV;
  const int64_t nlat = nslot * L, tot = (nlat + BQ) * cpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / cpr; const int j = (int)(i - row * cpr) * NV;
    float v[NV];
    if (row >= nlat) load_vec<T, NV>(qtok + (row - nlat) * D + j, v);
    else {
      const int64_t s_ = row / L; const int n = (int)(row - s_ * L);
      const T* lr = lat + ((int64_t)slot_b[s_] * L + n) * Cl;
      if (j < Cl) load_vec<T, NV>(lr + j, v);
      else {
        const int base = j - Cl + 5 * slot_f[s_];
#pragma unroll
        for (int e = 0; e < NV; ++e) { const int cc = base + e; v[e] = (cc >= 0 && cc < Cl) ? ld(lr + cc) : 0.f; }
      }
    }
    store_vec<T, NV>(xU + row * D + j, v);
  }
}
template <typename T>
void k_share_assemble(spa3d_ctx* c, const T* qtok, const T* lat, const int32_t* slot_b, const int32_t* slot_f, int64_t nslot, int64_t BQ, int L, int Cl,
                      int D, T* xU) {
  if (c->dry || BQ == 0) return;
  constexpr int NV = VecOf<T>::N;
  if (D % NV || Cl % NV) { if (!c->hip_err) { c->hip_err = -5; c->err = "share assemble: widths must be multiples of 16 bytes"; } return; }
  share_assemble_kernel<T><<<GRID1D((nslot * L + BQ) * (D / NV), 256), 256, 0, c->stream>>>(qtok, lat, slot_b, slot_f, nslot, BQ, L, Cl, D, xU);
  SPA_LAUNCH_CHECK(c);
}
// dense rows from slot rows.  Forward (add == nullptr): dst[(seq, tkn)] = src[tkn == 0 ? nslot*L + seq : slot[seq]*L + tkn - 1], a gather.
// Backward (add != nullptr): the slot row holds the SUM over the slot's member sequences (the LayerNorm backward is linear in its incoming
// gradient), so it is added to ONE member, the slot's first sequence slot_q0 -- every consumer downstream sums over the queries of a
// sample with the members' common frame (k_assemble_readout_bwd) --, and dst = add elsewhere.
template <typename T, bool ADD>
__global__ void share_expand_kernel(const T* __restrict__ src, const int32_t* __restrict__ slot, const int32_t* __restrict__ slot_q0, int64_t nslot,
                                    int64_t nseq, int S, int d, const T* add, T* dst) {
  constexpr int NV = VecOf<T>::N;
  const int cpr = d / NV, L = S - 1;
  const int64_t tot = nseq * S * cpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / cpr; const int ch = (int)(i - row * cpr);
    const int64_t seq = row / S; const int tkn = (int)(row - seq * S);
    const int32_t sl = slot[seq];
    const int64_t sr = tkn == 0 ? nslot * L + seq : (int64_t)sl * L + tkn - 1;
    if constexpr (ADD) {
      float b[NV];
      load_vec<T, NV>(add + row * d + ch * NV, b);
      if (tkn == 0 || slot_q0[sl] == (int32_t)seq) {
        float a[NV];
        load_vec<T, NV>(src + sr * d + ch * NV, a);
#pragma unroll
        for (int j = 0; j < NV; ++j) b[j] += a[j];
      }
      store_vec<T, NV>(dst + row * d + ch * NV, b);
    } else {
      *(uint4*)(dst + row * d + ch * NV) = *(const uint4*)(src + sr * d + ch * NV);
    }
  }
}
template <typename T>
void k_share_expand(spa3d_ctx* c, const T* src, const int32_t* slot, const int32_t* slot_q0, int64_t nslot, int64_t nseq, int S, int d, const T* add, T* dst) {
  if (c->dry || nseq == 0) return;
  constexpr int NV = VecOf<T>::N;
  if (d % NV) { if (!c->hip_err) { c->hip_err = -5; c->err = "share expand: row width must be a multiple of 16 bytes"; } return; }
  const dim3 g = GRID1D(nseq * S * (d / NV), 256);
  if (add) share_expand_kernel<T, true><<<g, 256, 0, c->stream>>>(src, slot, slot_q0, nslot, nseq, S, d, add, dst);
  else share_expand_kernel<T, false><<<g, 256, 0, c->stream>>>(src, slot, slot_q0, nslot, nseq, S, d, nullptr, dst);
  SPA_LAUNCH_CHECK(c);
}
// slot rows from dense rows (the transpose of the expansion): dstU[(s, n)] = sum over the sequences of slot s of src[(seq, 1 + n)] (fp32 sums);
// dstU[nslot*L + seq] = src[(seq, 0)].  One workgroup per slot: the member list is built once in LDS, then rows are walked 16 B per thread.
template <typename T>
__global__ __launch_bounds__(256) void share_reduce_kernel(const T* __restrict__ src, const int32_t* __restrict__ slot, const int32_t* __restrict__ slot_b,
                                                           int64_t nslot, int Q, int S, int d, T* __restrict__ dstU) {
  constexpr int NV = VecOf<T>::N;
  extern __shared__ int32_t members[];  // [Q]
  __shared__ int32_t wcnt[4], nmem;
  const int64_t s_ = blockIdx.x; const int L = S - 1, cpr = d / NV;
  const int b = slot_b[s_];
  // member list in ascending query order (ballot + prefix, as prune_fill_kernel): the fp32 sums below then have ONE order, run to run
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int base = 0;
  for (int q0 = 0; q0 < Q; q0 += 256) {
    const int q = q0 + threadIdx.x;
    const bool mine = q < Q && slot[(int64_t)b * Q + q] == (int32_t)s_;
    const unsigned long long m = __ballot(mine);
    if (lane == 0) wcnt[wv] = __popcll(m);
    __syncthreads();
    int pre = base;
    for (int w2 = 0; w2 < wv; ++w2) pre += wcnt[w2];
    if (mine) members[pre + __popcll(m & ((1ull << lane) - 1ull))] = q;
    base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) nmem = base;
  __syncthreads();
  const int nm = nmem;
  for (int i = threadIdx.x; i < L * cpr; i += 256) {
    const int n = i / cpr, ch = i - n * cpr;
    float acc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = 0.f;
    for (int m = 0; m < nm; ++m) {
      float v[NV];
      load_vec<T, NV>(src + (((int64_t)b * Q + members[m]) * S + 1 + n) * d + ch * NV, v);
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[j] += v[j];
    }
    store_vec<T, NV>(dstU + (s_ * L + n) * d + ch * NV, acc);
  }
}
template <typename T>
void k_share_reduce(spa3d_ctx* c, const T* src, const int32_t* slot, const int32_t* slot_b, int64_t nslot, int64_t nseq, int Q, int S, int d, T* dstU) {
  if (c->dry || nseq == 0) return;
  constexpr int NV = VecOf<T>::N;
  if (d % NV) { if (!c->hip_err) { c->hip_err = -5; c->err = "share reduce: row width must be a multiple of 16 bytes"; } return; }
  if (nslot > 0) share_reduce_kernel<T><<<(unsigned)nslot, 256, Q * sizeof(int32_t), c->stream>>>(src, slot, slot_b, nslot, Q, S, d, dstU);
  SPA_LAUNCH_CHECK(c);
  k_gather_rows<T>(c, src, S, dstU + nslot * (S - 1) * d, nseq, d);  // rows 0: one per sequence
}

// ---------------------------------------------------------------------------------------------
// D4-D6: readout sequence assembly without materialising tile/eye (track_autoencoder_3d.py:235-246,276-284)
// seq[b][q][0][:] = qtok[b][q][:] ; seq[b][q][1+n][c<Cl] = lat[b][n][c] ; seq[b][q][1+n][Cl+dd] = lat[b][n][dd+5*t_q] or 0
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void assemble_kernel(const T* __restrict__ qtok, const T* __restrict__ lat, const int32_t* __restrict__ qframe, int64_t BQ, int Q,
                                int L, int Cl, int D, T* __restrict__ seq) {
  const int64_t tot = BQ * (L + 1) * D;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    int64_t row = i / D; int j = (int)(i - row * D);
    int64_t bq = row / (L + 1); int tkn = (int)(row - bq * (L + 1));
    T v;
    if (tkn == 0) v = qtok[bq * D + j];
    else {
      int64_t b = bq / Q; int n = tkn - 1;
      const T* lr = lat + (b * L + n) * Cl;
      if (j < Cl) v = lr[j];
      else {
        int64_t cc = (int64_t)(j - Cl) + 5 * (int64_t)qframe[bq];
        if (cc >= 0 && cc < Cl) v = lr[cc]; else { T z; st(&z, 0.f); v = z; }
      }
    }
    seq[i] = v;
  }
}
// 8 elements per thread (one 16-B store), 32-bit index math; only the window part (Cl <= j, source shifted by 5 t_q elements, hence
// unaligned) gathers element-wise.  Needs D % 8 == 0, Cl % 8 == 0 and < 2^31 chunks (else the scalar kernel above).
template <typename T>
__global__ void assemble_vec_kernel(const T* __restrict__ qtok, const T* __restrict__ lat, const int32_t* __restrict__ qframe, unsigned nchunk,
                                    int Q, int L, int Cl, int D, T* __restrict__ seq) {
  constexpr int NV = VecOf<T>::N;
  const unsigned cpr = (unsigned)D / NV;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < nchunk; i += gridDim.x * 256u) {
    const unsigned row = i / cpr; const int j = (int)(i - row * cpr) * NV;
    const unsigned bq = row / (unsigned)(L + 1); const int tkn = (int)(row - bq * (unsigned)(L + 1));
    float v[NV];
    if (tkn == 0) load_vec<T, NV>(qtok + (int64_t)bq * D + j, v);
    else {
      const unsigned b = bq / (unsigned)Q;
      const T* lr = lat + ((int64_t)b * L + (tkn - 1)) * Cl;
      if (j < Cl) load_vec<T, NV>(lr + j, v);
      else {
        const int base = j - Cl + 5 * qframe[bq];
#pragma unroll
        for (int e = 0; e < NV; ++e) { const int cc = base + e; v[e] = (cc >= 0 && cc < Cl) ? ld(lr + cc) : 0.f; }
      }
    }
    store_vec<T, NV>(seq + (int64_t)row * D + j, v);
  }
}
template <typename T>
void k_assemble_readout(spa3d_ctx* c, const T* qtok, const T* lat, const int32_t* qframe, int64_t B, int Q, int L, int Cl, int D, T* seq) {
  if (c->dry || B == 0) return;
  constexpr int NV = VecOf<T>::N;
  const int64_t nchunk = B * Q * (L + 1) * (D / NV);
  if (D % NV == 0 && Cl % NV == 0 && nchunk < 0x7fffffffLL && ((((uintptr_t)qtok) | ((uintptr_t)lat) | ((uintptr_t)seq)) & 15) == 0) {
    assemble_vec_kernel<T><<<GRID1D(nchunk, 256), 256, 0, c->stream>>>(qtok, lat, qframe, (unsigned)nchunk, Q, L, Cl, D, seq);
  } else {
    assemble_kernel<T><<<GRID1D(B * Q * (L + 1) * D, 256), 256, 0, c->stream>>>(qtok, lat, qframe, B * Q, Q, L, Cl, D, seq);
  }
  SPA_LAUNCH_CHECK(c);
}
// backward: dqtok = dseq[:, :, 0, :] ; dlat[b][n][c] = sum_q dseq[b][q][1+n][c] + sum_q dseq[b][q][1+n][Cl + c-5t_q] 1[0<=c-5t_q<D-Cl]
// ACC: dlat += that sum instead (query chunks, model.hip: one plain fp32 add per element in stream order -- no atomics, fixed order)
template <typename T, bool ACC>
__global__ void assemble_bwd_lat_kernel(const T* __restrict__ dseq, const int32_t* __restrict__ qframe, int64_t B, int Q, int L, int Cl,
                                        int D, float* __restrict__ dlat) {
  const int64_t tot = B * L * Cl;
  const int Wd = D - Cl;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    int64_t bn = i / Cl; int cc = (int)(i - bn * Cl);
    int64_t b = bn / L; int n = (int)(bn - b * L);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;  // independent chains: 512 dependent strided loads were pure latency
    auto term = [&](int q) {
      const T* r = dseq + (((b * Q + q) * (L + 1)) + 1 + n) * D;
      float t = ld(r + cc);
      const int dd = cc - 5 * qframe[b * Q + q];
      if (dd >= 0 && dd < Wd) t += ld(r + Cl + dd);
      return t;
    };
    int q = 0;
    for (; q + 3 < Q; q += 4) { s0 += term(q); s1 += term(q + 1); s2 += term(q + 2); s3 += term(q + 3); }
    for (; q < Q; ++q) s0 += term(q);
    const float s = (s0 + s1) + (s2 + s3);
    if (ACC) dlat[i] += s; else dlat[i] = s;
  }
}
template <typename T>
void k_assemble_readout_bwd(spa3d_ctx* c, const T* dseq, const int32_t* qframe, int64_t B, int Q, int L, int Cl, int D, T* dqtok,
                            float* dlat, bool accumulate) {
  if (c->dry || B == 0) return;
  k_gather_rows<T>(c, dseq, L + 1, dqtok, B * Q, D);
  if (accumulate) assemble_bwd_lat_kernel<T, true><<<GRID1D(B * L * Cl, 256), 256, 0, c->stream>>>(dseq, qframe, B, Q, L, Cl, D, dlat);
  else assemble_bwd_lat_kernel<T, false><<<GRID1D(B * L * Cl, 256), 256, 0, c->stream>>>(dseq, qframe, B, Q, L, Cl, D, dlat);
  SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// parameter rows
// ---------------------------------------------------------------------------------------------
// ParamStateInit broadcast (track_autoencoder.py:41-53) and its gradient
template <typename T>
__global__ void bcast_rows_kernel(const float* __restrict__ src, int64_t per, T* __restrict__ dst, int64_t B) {
  const int64_t tot = per * B;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) st(dst + i, src[i % per]);
}
template <typename T> void k_broadcast_rows(spa3d_ctx* c, const float* src, int rows, int d, T* dst, int64_t B) {
  if (c->dry || B == 0) return;
  bcast_rows_kernel<T><<<GRID1D((int64_t)rows * d * B, 256), 256, 0, c->stream>>>(src, (int64_t)rows * d, dst, B); SPA_LAUNCH_CHECK(c);
}
template <typename T>
__global__ void bcast_grad_kernel(const T* __restrict__ dsrc, int64_t per, int64_t B, int64_t bstride, float* __restrict__ dparam, int64_t bchunk,
                                  const DetCfg* det) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  const int64_t b0 = (int64_t)blockIdx.y * bchunk; int64_t b1 = b0 + bchunk; if (b1 > B) b1 = B;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;  // four independent chains: the strided rows are latency, not bandwidth
  int64_t b = b0;
  for (; b + 3 < b1; b += 4) {
    s0 += ld(dsrc + b * bstride + i); s1 += ld(dsrc + (b + 1) * bstride + i);
    s2 += ld(dsrc + (b + 2) * bstride + i); s3 += ld(dsrc + (b + 3) * bstride + i);
  }
  for (; b < b1; ++b) s0 += ld(dsrc + b * bstride + i);
  const float s = (s0 + s1) + (s2 + s3);
  if (gridDim.y == 1) dparam[i] += s; else grad_add(det_read(det), dparam + i, s);
}
// dparam[per] += sum_b dsrc[b*bstride + :per]   (B up to ~10^5 strided rows: split over blockIdx.y, one f32 atomic per column per slice)
template <typename T> void k_bcast_grad(spa3d_ctx* c, const T* dsrc, int64_t per, int64_t B, int64_t bstride, float* dparam) {
  if (c->dry || B == 0) return;
  const int64_t gx = cdiv(per, 256);
  int64_t gy = std::max<int64_t>(1, std::min<int64_t>(B / 32, std::max<int64_t>(1, 2048 / gx)));
  const int64_t bchunk = cdiv(B, gy); gy = cdiv(B, bchunk);
  bcast_grad_kernel<T><<<dim3((unsigned)gx, (unsigned)gy), 256, 0, c->stream>>>(dsrc, per, B, bstride, dparam, bchunk, c->det); SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// TRAJAN track pooling (track_autoencoder.py:230-232): mean of the frame tokens over VISIBLE frames
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void vis_mean_pool_kernel(const T* __restrict__ tok, const float* __restrict__ vis, int64_t nseq, int T_, int d, T* __restrict__ out) {
  const int64_t tot = nseq * d;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    int64_t s_ = i / d; int j = (int)(i - s_ * d);
    float a = 0.f, cnt = 0.f;
    for (int t = 0; t < T_; ++t) { const float v = vis[s_ * T_ + t] != 0.f ? 1.f : 0.f; a += ld(tok + (s_ * T_ + t) * d + j) * v; cnt += v; }
    st(out + i, a / fmaxf(1.f, cnt));
  }
}
template <typename T> void k_vis_mean_pool(spa3d_ctx* c, const T* tok, const float* vis, int64_t nseq, int T_, int d, T* out) {
  if (c->dry || nseq == 0) return;
  vis_mean_pool_kernel<T><<<GRID1D(nseq * d, 256), 256, 0, c->stream>>>(tok, vis, nseq, T_, d, out); SPA_LAUNCH_CHECK(c);
}
template <typename T>
__global__ void vis_mean_pool_bwd_kernel(const T* __restrict__ dout, const float* __restrict__ vis, int64_t nseq, int T_, int d, T* __restrict__ dtok) {
  const int64_t tot = nseq * T_ * d;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    int64_t r = i / d; int j = (int)(i - r * d);
    int64_t s_ = r / T_;
    float cnt = 0.f;
    for (int t = 0; t < T_; ++t) cnt += vis[s_ * T_ + t] != 0.f ? 1.f : 0.f;
    const float v = vis[r] != 0.f ? 1.f : 0.f;
    st(dtok + i, ld(dout + s_ * d + j) * v / fmaxf(1.f, cnt));
  }
}
template <typename T> void k_vis_mean_pool_bwd(spa3d_ctx* c, const T* dout, const float* vis, int64_t nseq, int T_, int d, T* dtok) {
  if (c->dry || nseq == 0) return;
  vis_mean_pool_bwd_kernel<T><<<GRID1D(nseq * T_ * d, 256), 256, 0, c->stream>>>(dout, vis, nseq, T_, d, dtok); SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------
// explicit instantiations
// ---------------------------------------------------------------------------------------------
#define INST_ROWS(T) \
  template void k_cast_from_f32<T>(spa3d_ctx*, const float*, T*, int64_t);                                                                 \
  template void k_cast_to_f32<T>(spa3d_ctx*, const T*, float*, int64_t);                                                                   \
  template void k_colsum<T>(spa3d_ctx*, const T*, int64_t, int, int64_t, float*, int, int);                                                \
  template void k_gather_rows<T>(spa3d_ctx*, const T*, int64_t, T*, int64_t, int);                                                         \
  template void k_rows_idx<T>(spa3d_ctx*, int, const T*, const int32_t*, T*, int64_t, int);                                                \
  template void k_add_rows_strided<T>(spa3d_ctx*, T*, const T*, int64_t, int64_t, int);                                                    \
  template void k_share_assemble<T>(spa3d_ctx*, const T*, const T*, const int32_t*, const int32_t*, int64_t, int64_t, int, int, int, T*);  \
  template void k_share_expand<T>(spa3d_ctx*, const T*, const int32_t*, const int32_t*, int64_t, int64_t, int, int, const T*, T*);         \
  template void k_share_reduce<T>(spa3d_ctx*, const T*, const int32_t*, const int32_t*, int64_t, int64_t, int, int, int, T*);              \
  template void k_assemble_readout<T>(spa3d_ctx*, const T*, const T*, const int32_t*, int64_t, int, int, int, int, T*);                    \
  template void k_assemble_readout_bwd<T>(spa3d_ctx*, const T*, const int32_t*, int64_t, int, int, int, int, T*, float*, bool);            \
  template void k_broadcast_rows<T>(spa3d_ctx*, const float*, int, int, T*, int64_t);                                                      \
  template void k_bcast_grad<T>(spa3d_ctx*, const T*, int64_t, int64_t, int64_t, float*);                                                  \
  template void k_vis_mean_pool<T>(spa3d_ctx*, const T*, const float*, int64_t, int, int, T*);                                             \
  template void k_vis_mean_pool_bwd<T>(spa3d_ctx*, const T*, const float*, int64_t, int, int, T*);
INST_ROWS(float)
INST_ROWS(bf16_t)
}  // namespace SPA_NS
