// motion.hip -- the latent-set metrics' device side (include/spa3d.h), each kernel first, the entry points below them:
//   spa3d_motion_codes        latents -> the integer codes the decoder's quantiser rounds to (streaming, 16-byte loads);
//   spa3d_motion_moments_add  n, sum x, sum x x^T of token rows or of per-clip token sums, in 64-bit integers, ADDED into a caller-held state;
//   spa3d_motion_pdist        all pairwise dot products / squared distances of two code sets: a tiled NT GEMM on mfma_f32_16x16x32_bf16 whose
//                             fp32 accumulators are moved into int32 every MOTION_KCHUNK elements of K, so every result is an exact integer;
//   spa3d_motion_knn          the k nearest rows of b for every row of a, and
//   spa3d_motion_ball_hits    per-row and per-column counts of d(i, j) <= radius[i]: the pdist tile and K loop with a reducing epilogue in place
//                             of the store, so no [Ma, Mb] matrix exists anywhere;
//   spa3d_motion_kernel_sums  per-row and per-column sums of the polynomial kernel's numerator (a.b + C)^deg as 128-bit integers: the third such
//                             epilogue, what the unbiased MMD of two code sets (spa3d.kernel_distance) is made of.
// The code rounding, the state layout, the range checks and the chunk constant are motion_code.hpp's, which the g++ host test runs too.
// Nothing here adds floats across threads: the only atomics are integer adds, which commute, so two runs -- and any batching, chunking or
// rank split of the same clips -- give the same bits.  No 16-bit activations are touched: compiled once.  Plain loads and stores.
#include "common.hpp"
#include "motion_code.hpp"

namespace SPA_NS {

// ---------------------------------------------------------------------------------------------- codes
__device__ __forceinline__ int16_t mo_code_count(float x, int& nb) {
  bool nan = false;
  const int16_t c = mc_code(x, &nan);
  nb += nan ? 1 : 0;
  return c;
}

// VEC: latents 16-byte and codes 8-byte aligned -- four latents per load, the n % 4 tail by scalar loads
template <bool VEC> __global__ __launch_bounds__(256) void motion_codes_kernel(const float* __restrict__ lat, int64_t n, int16_t* __restrict__ codes, int32_t* bad) {
  int nb = 0;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  int64_t done = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    for (int64_t i = t0; i < n4; i += stride) {
      const float4 v = reinterpret_cast<const float4*>(lat)[i];
      short4 o;
      o.x = mo_code_count(v.x, nb); o.y = mo_code_count(v.y, nb); o.z = mo_code_count(v.z, nb); o.w = mo_code_count(v.w, nb);
      reinterpret_cast<short4*>(codes)[i] = o;
    }
    done = n4 << 2;
  }
  for (int64_t i = done + t0; i < n; i += stride) codes[i] = mo_code_count(lat[i], nb);
  // NaNs of the wave, one integer atomic per wave that saw any
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nb += __shfl_down(nb, off);
  if ((threadIdx.x & 63) == 0 && nb) atomicAdd(bad, nb);
}

void k_motion_codes(spa3d_ctx* c, const float* lat, int64_t n, int16_t* codes, int32_t* bad) {
  if (c->dry) return;
  hipError_t e = hipMemsetAsync(bad, 0, sizeof(int32_t), c->stream);
  if (e != hipSuccess && c->hip_err == 0) { c->hip_err = (int)e; c->err = std::string("motion_codes: hipMemsetAsync failed: ") + hipGetErrorString(e); }
  if (n == 0 || c->hip_err) return;
  const bool vec = ((uintptr_t)lat & 15) == 0 && ((uintptr_t)codes & 7) == 0;
  if (vec) motion_codes_kernel<true><<<GRID1D(cdiv(n, 4), 256), 256, 0, c->stream>>>(lat, n, codes, bad);
  else motion_codes_kernel<false><<<GRID1D(n, 256), 256, 0, c->stream>>>(lat, n, codes, bad);
  SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------- moments
// One workgroup per (slice of samples, 64 x 64 tile of S).  A batch of MM_S samples is staged in LDS as int32 -- columns [i0, i0 + 64) and
// [j0, j0 + 64), each a token row's code or, for the clip pool, the sum of the clip's R = L token rows -- and thread (ti, tj) adds its 4 x 4
// products into 64-bit registers.  The tiles of the first tile column also sum s, tile (0, 0) of slice 0 adds n.
constexpr int MM_TILE = 64, MM_S = 16, MM_SLICES = 64;

__global__ __launch_bounds__(256) void motion_moments_kernel(const int16_t* __restrict__ codes, int64_t nsamp, int R, int D, unsigned long long* state) {
  __shared__ __attribute__((aligned(16))) int32_t xi[MM_S][MM_TILE];
  __shared__ __attribute__((aligned(16))) int32_t xj[MM_S][MM_TILE];
  const int tiles = (D + MM_TILE - 1) / MM_TILE;
  const int i0 = ((int)blockIdx.y / tiles) * MM_TILE, j0 = ((int)blockIdx.y % tiles) * MM_TILE;
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  int64_t acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = 0;
  int64_t ssum = 0;
  for (int64_t base = (int64_t)blockIdx.x * MM_S; base < nsamp; base += (int64_t)gridDim.x * MM_S) {
    __syncthreads();   // the previous batch has been read
    for (int idx = threadIdx.x; idx < MM_S * 2 * MM_TILE; idx += 256) {
      const int s = idx >> 7, c = idx & 127;
      const int col = c < MM_TILE ? i0 + c : j0 + c - MM_TILE;
      const int64_t m = base + s;
      int32_t v = 0;
      if (m < nsamp && col < D) {
        const int16_t* p = codes + m * R * D + col;
        for (int l = 0; l < R; ++l) v += (int32_t)p[(int64_t)l * D];   // |v| <= 128 * 4096 = 2^19
      }
      if (c < MM_TILE) xi[s][c] = v; else xj[s][c - MM_TILE] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int s = 0; s < MM_S; ++s) {
      const int4 a = *reinterpret_cast<const int4*>(&xi[s][ti * 4]);
      const int4 b = *reinterpret_cast<const int4*>(&xj[s][tj * 4]);
      const int32_t av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] += (int64_t)av[p] * (int64_t)bv[q];
    }
    if (j0 == 0 && threadIdx.x < MM_TILE)
      for (int s = 0; s < MM_S; ++s) ssum += xi[s][threadIdx.x];
  }
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + ti * 4 + p, j = j0 + tj * 4 + q;
      if (i < D && j < D && acc[p][q] != 0) atomicAdd(&state[mc_state_S(D, i, j)], (unsigned long long)acc[p][q]);
    }
  if (j0 == 0 && threadIdx.x < MM_TILE && i0 + (int)threadIdx.x < D && ssum != 0) atomicAdd(&state[mc_state_s(i0 + threadIdx.x)], (unsigned long long)ssum);
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(&state[mc_state_n()], (unsigned long long)nsamp);
}

void k_motion_moments(spa3d_ctx* c, const int16_t* codes, int64_t M, int L, int D, int pool, int64_t* state) {
  if (c->dry) return;
  const int64_t nsamp = mc_samples(M, L, pool);
  const int tiles = (D + MM_TILE - 1) / MM_TILE;
  const dim3 grid((unsigned)std::min<int64_t>(cdiv(nsamp, MM_S), MM_SLICES), (unsigned)(tiles * tiles));
  motion_moments_kernel<<<grid, 256, 0, c->stream>>>(codes, nsamp, pool == MC_POOL_TOKEN ? 1 : L, D, reinterpret_cast<unsigned long long*>(state));
  SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------- pairwise distances
// out[i][j] = sum_e a[i][e] b[j][e]: an NT GEMM, K contiguous in both operands.  A workgroup of 4 waves owns a 128 x 128 tile, a wave 64 x 64 of
// it as 4 x 4 fragments of mfma_f32_16x16x32_bf16.  Per step of PD_BK = 64 elements of K each thread loads four 16-byte chunks (8 codes) of each
// operand, converts them to bf16 (exact: |code| <= 128) and stores them into the LDS image; the next step's loads are issued before this
// step's MFMAs.  LDS image: row-major, 8 chunks of 16 bytes per row, chunk s of row r at slot s ^ (r & 7) -- the 16 lanes ds_read_b128 serves
// together (8 rows of one chunk column, 8 of the next) then fall into 16 different 16-byte slots of the 256-byte bank row: conflict-free.
// A fragment is one ds_read_b128: lane l holds row l & 15, k = 8 (l >> 4) .. + 7 of the 32-wide step, for A and for B alike.
// Rows past Ma / Mb and the K tail are zeros in LDS; the store is guarded.  Squared norms are summed from the very integers that are staged.
constexpr int PD_BM = 128, PD_BN = 128, PD_BK = 64, PD_FLUSH = MOTION_KCHUNK / PD_BK;
static_assert(MOTION_KCHUNK % PD_BK == 0, "a flush falls on a step boundary");
typedef __attribute__((ext_vector_type(4))) float pd_f32x4;

// chunk (8 codes from element k) of row r: zeros past the rows or past E.  vec: E % 8 == 0 and a 16-byte aligned base, so a chunk is whole
__device__ __forceinline__ uint4 pd_load(const int16_t* __restrict__ base, int64_t rows, int E, int64_t r, int k, bool vec) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (r >= rows || k >= E) return v;
  const int16_t* p = base + r * E + k;
  if (vec) return *reinterpret_cast<const uint4*>(p);
  unsigned e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = k + j < E ? (unsigned)(unsigned short)p[j] : 0u;
  v.x = e[0] | (e[1] << 16); v.y = e[2] | (e[3] << 16); v.z = e[4] | (e[5] << 16); v.w = e[6] | (e[7] << 16);
  return v;
}
// two int16 codes of a dword -> two bf16; sq += their squares
__device__ __forceinline__ unsigned pd_cvt2(unsigned w, int& sq) {
  const int lo = (int)(short)(w & 0xffffu), hi = (int)w >> 16;
  sq += lo * lo + hi * hi;
  return f2bf_pack2((float)lo, (float)hi);
}
__device__ __forceinline__ uint4 pd_cvt8(uint4 v, int& sq) { return make_uint4(pd_cvt2(v.x, sq), pd_cvt2(v.y, sq), pd_cvt2(v.z, sq), pd_cvt2(v.w, sq)); }

// The K loop the three tile kernels share: the products of rows [i0, i0 + 128) of a with rows [j0, j0 + 128) of b over all of E, this wave's
// 64 x 64 of them ADDED into iacc as exact integers, and the parts of the rows' squared norms this thread staged added into na / nb.  The caller
// declares the three zero-initialised (zeroing them in here costs the pdist kernel 60 registers: hipcc then allocates 256 VGPR + 109 AGPR for it
// instead of 238 + 64).  sA and sB are the 16 KB operand images.  Starts with a barrier (whatever read or wrote the images before has finished);
// the last step's fragment reads are NOT followed by one.
__device__ __forceinline__ void pd_kloop(const int16_t* __restrict__ a, int64_t Ma, const int16_t* __restrict__ b, int64_t Mb, int E, int64_t i0, int64_t j0, bool vec,
                                         uint4* sA, uint4* sB, int32_t (&iacc)[4][4][4], int (&na)[4], int (&nb)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
  const int srow = tid >> 3, sslot = tid & 7;   // this thread stages chunk sslot of rows srow + 32 i, i = 0..3
  pd_f32x4 facc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) facc[m][n] = pd_f32x4{0.f, 0.f, 0.f, 0.f};
  uint4 ra[4], rb[4];
  const int nk = (E + PD_BK - 1) / PD_BK;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ra[i] = pd_load(a, Ma, E, i0 + srow + 32 * i, sslot * 8, vec);
    rb[i] = pd_load(b, Mb, E, j0 + srow + 32 * i, sslot * 8, vec);
  }
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();   // the previous step's fragments have been read
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = srow + 32 * i;
      sA[r * 8 + (sslot ^ (r & 7))] = pd_cvt8(ra[i], na[i]);
      sB[r * 8 + (sslot ^ (r & 7))] = pd_cvt8(rb[i], nb[i]);
    }
    __syncthreads();
    if (kt + 1 < nk) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ra[i] = pd_load(a, Ma, E, i0 + srow + 32 * i, (kt + 1) * PD_BK + sslot * 8, vec);
        rb[i] = pd_load(b, Mb, E, j0 + srow + 32 * i, (kt + 1) * PD_BK + sslot * 8, vec);
      }
    }
#pragma unroll
    for (int ks = 0; ks < PD_BK / 32; ++ks) {
      const int slot = ks * 4 + (lane >> 4);
      mfma16x8 fa[4], fb[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int rA = wm * 64 + f * 16 + (lane & 15), rB = wn * 64 + f * 16 + (lane & 15);
        fa[f] = __builtin_bit_cast(mfma16x8, sA[rA * 8 + (slot ^ (rA & 7))]);
        fb[f] = __builtin_bit_cast(mfma16x8, sB[rB * 8 + (slot ^ (rB & 7))]);
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) facc[m][n] = MFMA16(fa[m], fb[n], facc[m][n]);
    }
    // the chunk rule (motion_code.hpp): MOTION_KCHUNK elements of K have gone into the fp32 accumulators, every partial sum an integer of at
    // most 2^24 in magnitude; move them into the integers and start the next chunk from zero
    if ((kt + 1) % PD_FLUSH == 0 || kt + 1 == nk) {
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
#pragma unroll
          for (int r = 0; r < 4; ++r) iacc[m][n][r] += __float2int_rn(facc[m][n][r]);
          facc[m][n] = pd_f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
  }
}
// the squared norms of the tile's rows into sNa / sNb: the 8 threads that staged a row hold it in parts, lanes 8 q .. 8 q + 7 of a wave.  Ends
// with a barrier, after which every wave has also finished the K loop's last fragment reads.
__device__ __forceinline__ void pd_norms(int (&na)[4], int (&nb)[4], int32_t* sNa, int32_t* sNb) {
  const int srow = threadIdx.x >> 3, sslot = threadIdx.x & 7;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) { na[i] += __shfl_xor(na[i], off); nb[i] += __shfl_xor(nb[i], off); }
    if (sslot == 0) { sNa[srow + 32 * i] = na[i]; sNb[srow + 32 * i] = nb[i]; }
  }
  __syncthreads();
}

template <bool SQ> __global__ __launch_bounds__(256) void motion_pdist_kernel(const int16_t* __restrict__ a, int64_t Ma, const int16_t* __restrict__ b, int64_t Mb, int E,
                                                                              int32_t* __restrict__ out, int vec) {
  __shared__ uint4 sA[PD_BM * 8];
  __shared__ uint4 sB[PD_BN * 8];
  __shared__ int32_t sNa[PD_BM], sNb[PD_BN];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
  const int64_t i0 = (int64_t)blockIdx.y * PD_BM, j0 = (int64_t)blockIdx.x * PD_BN;
  int32_t iacc[4][4][4] = {};
  int na[4] = {0, 0, 0, 0}, nb[4] = {0, 0, 0, 0};
  pd_kloop(a, Ma, b, Mb, E, i0, j0, vec != 0, sA, sB, iacc, na, nb);
  if (SQ) pd_norms(na, nb, sNa, sNb);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int li = wm * 64 + m * 16 + (lane >> 4) * 4 + r, lj = wn * 64 + n * 16 + (lane & 15);   // C/D: col = lane & 15, row = 4 (lane >> 4) + r
        const int64_t i = i0 + li, j = j0 + lj;
        if (i < Ma && j < Mb) out[i * Mb + j] = SQ ? sNa[li] + sNb[lj] - 2 * iacc[m][n][r] : iacc[m][n][r];
      }
}

void k_motion_pdist(spa3d_ctx* c, const int16_t* a, int64_t Ma, const int16_t* b, int64_t Mb, int E, int kind, int32_t* out) {
  if (c->dry) return;
  const int vec = (E % 8 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0) ? 1 : 0;
  const dim3 grid((unsigned)cdiv(Mb, PD_BN), (unsigned)cdiv(Ma, PD_BM));
  if (kind == MC_PDIST_SQDIST) motion_pdist_kernel<true><<<grid, 256, 0, c->stream>>>(a, Ma, b, Mb, E, out, vec);
  else motion_pdist_kernel<false><<<grid, 256, 0, c->stream>>>(a, Ma, b, Mb, E, out, vec);
  SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------- streaming k-NN
// A row's list is its k smallest keys so far (mc_knn_key: distance, then column), ascending, in lanes 0 .. k - 1 of a wave; the other lanes
// hold MC_KNN_NONE.  knn_offer puts the keys the lanes bring (one each, MC_KNN_NONE for none) into it.  Only keys below the k-th one, thr, are
// looked at: a ballot finds them, the lowest such lane's key is broadcast, its position is the number of list entries below it (keys of a row
// are distinct), the entries from there move up one lane, and the ballot is taken again against the new k-th key.  Integer compares only.
__device__ __forceinline__ void knn_offer(unsigned long long key, unsigned long long& L, unsigned long long& thr, int k, int lane) {
  unsigned long long m = __ballot(key < thr);
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    const unsigned long long ck = __shfl(key, src);
    const int pos = __popcll(__ballot(L < ck));   // < k: ck is below the k-th entry
    const unsigned long long up = __shfl_up(L, 1);
    L = lane < pos ? L : (lane == pos ? ck : (lane < k ? up : MC_KNN_NONE));
    thr = __shfl(L, k - 1);
    m = (m & (m - 1)) & __ballot(key < thr);
  }
}

// Grid: (row tiles of 128) x (column ranges).  The workgroup walks the column tiles of its range (mc_knn_tile_range) with the pdist K loop and,
// after each, folds the tile's 128 x 128 distances into the rows' lists, which live in LDS between tiles (MC_KNN_MAX_K entries a row, 64 KB).  The
// distances pass through LDS 64 rows at a time, in the 32 KB the operand images no longer need: the waves that own the half write it (column
// XOR 16 on rows whose bit 2 is set: lanes l and l + 16 of a store hold rows 4 apart), then every wave folds 16 of its rows, the lanes taking
// columns lane and lane + 64.  A column past Mb (zeros in LDS: its "distance" is |a_i|^2) and the row's own column make no key.
// One range: the lists are the result.  More: range s writes its lists to ws[s][i][0 .. k), MC_KNN_NONE where it had fewer than k columns.
__global__ __launch_bounds__(256) void motion_knn_kernel(const int16_t* __restrict__ a, int64_t Ma, const int16_t* __restrict__ b, int64_t Mb, int E, int k,
                                                         int64_t self_offset, int32_t* __restrict__ dist, int32_t* __restrict__ idx, unsigned long long* __restrict__ ws, int vec) {
  __shared__ uint4 sAB[(PD_BM + PD_BN) * 8];
  __shared__ int32_t sNa[PD_BM], sNb[PD_BN];
  constexpr int KCAP = MC_KNN_MAX_K;
  __shared__ unsigned long long sL[PD_BM * KCAP];
  static_assert(64 * PD_BN * sizeof(int32_t) <= sizeof(sAB), "half a tile of distances fits the operand images");
  int32_t* sD = reinterpret_cast<int32_t*>(sAB);   // [64][PD_BN]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
  const int64_t i0 = (int64_t)blockIdx.x * PD_BM;
  for (int t = tid; t < PD_BM * KCAP; t += 256) sL[t] = MC_KNN_NONE;
  __syncthreads();
  int64_t t0, t1;
  mc_knn_tile_range(mc_knn_tiles(Mb), (int)gridDim.y, (int)blockIdx.y, &t0, &t1);
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t j0 = tile * PD_BN;
    int32_t iacc[4][4][4] = {};
    int na[4] = {0, 0, 0, 0}, nb[4] = {0, 0, 0, 0};
    pd_kloop(a, Ma, b, Mb, E, i0, j0, vec != 0, sAB, sAB + PD_BM * 8, iacc, na, nb);
    pd_norms(na, nb, sNa, sNb);   // and the images are free
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (wm == h) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int lr = m * 16 + (lane >> 4) * 4 + r, lj = wn * 64 + n * 16 + (lane & 15);
              sD[lr * PD_BN + (lj ^ (((lr >> 2) & 1) << 4))] = sNa[h * 64 + lr] + sNb[lj] - 2 * iacc[m][n][r];
            }
      }
      __syncthreads();
      for (int rr = 0; rr < 16; ++rr) {
        const int lr = wv * 16 + rr, li = h * 64 + lr;
        const int64_t i = i0 + li;
        if (i >= Ma) break;
        unsigned long long* lrow = sL + li * KCAP;
        unsigned long long thr = lrow[k - 1];
        const int64_t excl = mc_knn_excluded(i, self_offset);
        const int sw = ((lr >> 2) & 1) << 4;
        unsigned long long key[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int lj = lane + 64 * c;
          const int64_t j = j0 + lj;
          const int32_t d = sD[lr * PD_BN + (lj ^ sw)];
          key[c] = (j < Mb && j != excl) ? mc_knn_key(d, j) : MC_KNN_NONE;
        }
        if (!__any(key[0] < thr || key[1] < thr)) continue;   // after the first tiles: almost every row
        unsigned long long L = lane < k ? lrow[lane] : MC_KNN_NONE;
        knn_offer(key[0], L, thr, k, lane);
        knn_offer(key[1], L, thr, k, lane);
        if (lane < k) lrow[lane] = L;
      }
      __syncthreads();   // the half has been read: the other half, or the next tile's images, may be written
    }
  }
  // every wave writes the rows it folded
  for (int q = 0; q < 32; ++q) {
    const int li = (q >> 4) * 64 + wv * 16 + (q & 15);
    const int64_t i = i0 + li;
    if (i >= Ma || lane >= k) continue;
    const unsigned long long key = sL[li * KCAP + lane];
    if (gridDim.y == 1) {
      dist[i * k + lane] = mc_knn_key_dist(key);
      idx[i * k + lane] = mc_knn_key_idx(key);
    } else {
      ws[((int64_t)blockIdx.y * Ma + i) * k + lane] = key;
    }
  }
}

// one wave per row: the k smallest of the ranges' lists
__global__ __launch_bounds__(256) void motion_knn_merge_kernel(const unsigned long long* __restrict__ ws, int64_t Ma, int k, int splits, int32_t* __restrict__ dist,
                                                               int32_t* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= Ma) return;
  unsigned long long L = MC_KNN_NONE, thr = MC_KNN_NONE;
  for (int s = 0; s < splits; ++s) {
    const unsigned long long key = lane < k ? ws[((int64_t)s * Ma + i) * k + lane] : MC_KNN_NONE;
    knn_offer(key, L, thr, k, lane);
  }
  if (lane < k) {
    dist[i * k + lane] = mc_knn_key_dist(L);
    idx[i * k + lane] = mc_knn_key_idx(L);
  }
}

void k_motion_knn(spa3d_ctx* c, const int16_t* a, int64_t Ma, const int16_t* b, int64_t Mb, int E, int k, int64_t self_offset, int splits, int32_t* dist, int32_t* idx,
                  void* ws) {
  if (c->dry) return;
  const int vec = (E % 8 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0) ? 1 : 0;
  const dim3 grid((unsigned)cdiv(Ma, PD_BM), (unsigned)splits);
  unsigned long long* w = reinterpret_cast<unsigned long long*>(ws);
  motion_knn_kernel<<<grid, 256, 0, c->stream>>>(a, Ma, b, Mb, E, k, self_offset, dist, idx, w, vec);
  SPA_LAUNCH_CHECK(c);
  if (splits > 1 && c->hip_err == 0) {
    motion_knn_merge_kernel<<<(unsigned)cdiv(Ma, 4), 256, 0, c->stream>>>(w, Ma, k, splits, dist, idx);
    SPA_LAUNCH_CHECK(c);
  }
}

// ---------------------------------------------------------------------------------------------- ball hits
// The pdist grid and K loop; the store is replaced by counting.  hit(i, j) = d(i, j) <= radius[i] for a column inside b that is not the row's
// own.  A lane adds the hits of its 64 elements per row and per column in registers, the lanes that share a row (16) or a column (4) add theirs
// by shuffles, the two waves that share it by an LDS integer add, and one 32-bit integer atomic per row and per column of the tile with a hit
// adds the sum into global memory.  Integer adds commute: two runs give equal bits.
__global__ __launch_bounds__(256) void motion_ball_hits_kernel(const int16_t* __restrict__ a, int64_t Ma, const int16_t* __restrict__ b, int64_t Mb, int E,
                                                               const int32_t* __restrict__ radius, int64_t self_offset, int32_t* row_hits, int32_t* col_hits, int vec) {
  __shared__ uint4 sA[PD_BM * 8];
  __shared__ uint4 sB[PD_BN * 8];
  __shared__ int32_t sNa[PD_BM], sNb[PD_BN], sRad[PD_BM], sRow[PD_BM], sCol[PD_BN];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
  const int64_t i0 = (int64_t)blockIdx.y * PD_BM, j0 = (int64_t)blockIdx.x * PD_BN;
  if (tid < PD_BM) {
    sRad[tid] = i0 + tid < Ma ? radius[i0 + tid] : -1;
    sRow[tid] = 0;
    sCol[tid] = 0;
  }
  int32_t iacc[4][4][4] = {};
  int na[4] = {0, 0, 0, 0}, nb[4] = {0, 0, 0, 0};
  pd_kloop(a, Ma, b, Mb, E, i0, j0, vec != 0, sA, sB, iacc, na, nb);   // its barriers cover sRad, sRow and sCol
  pd_norms(na, nb, sNa, sNb);
  int ch[4] = {0, 0, 0, 0};
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int li = wm * 64 + m * 16 + (lane >> 4) * 4 + r;
      const int64_t i = i0 + li, excl = mc_knn_excluded(i, self_offset);
      const int32_t rad = sRad[li];
      int rh = 0;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int lj = wn * 64 + n * 16 + (lane & 15);
        const int64_t j = j0 + lj;
        const int hit = (i < Ma && j < Mb && j != excl && sNa[li] + sNb[lj] - 2 * iacc[m][n][r] <= rad) ? 1 : 0;
        rh += hit;
        ch[n] += hit;
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) rh += __shfl_xor(rh, off);
      if ((lane & 15) == 0 && rh) atomicAdd(&sRow[li], rh);
    }
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    ch[n] += __shfl_xor(ch[n], 16);
    ch[n] += __shfl_xor(ch[n], 32);
    if (lane < 16 && ch[n]) atomicAdd(&sCol[wn * 64 + n * 16 + lane], ch[n]);
  }
  __syncthreads();
  if (tid < PD_BM) {
    if (row_hits && i0 + tid < Ma && sRow[tid]) atomicAdd(&row_hits[i0 + tid], sRow[tid]);
  } else {
    const int t = tid - PD_BM;
    if (col_hits && j0 + t < Mb && sCol[t]) atomicAdd(&col_hits[j0 + t], sCol[t]);
  }
}

void k_motion_ball_hits(spa3d_ctx* c, const int16_t* a, int64_t Ma, const int16_t* b, int64_t Mb, int E, const int32_t* radius, int64_t self_offset, int32_t* row_hits,
                        int32_t* col_hits) {
  if (c->dry) return;
  hipError_t e = hipSuccess;
  if (row_hits) e = hipMemsetAsync(row_hits, 0, sizeof(int32_t) * Ma, c->stream);
  if (col_hits && e == hipSuccess) e = hipMemsetAsync(col_hits, 0, sizeof(int32_t) * Mb, c->stream);
  if (e != hipSuccess && c->hip_err == 0) { c->hip_err = (int)e; c->err = std::string("motion_ball_hits: hipMemsetAsync failed: ") + hipGetErrorString(e); }
  if (c->hip_err) return;
  const int vec = (E % 8 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0) ? 1 : 0;
  const dim3 grid((unsigned)cdiv(Mb, PD_BN), (unsigned)cdiv(Ma, PD_BM));
  motion_ball_hits_kernel<<<grid, 256, 0, c->stream>>>(a, Ma, b, Mb, E, radius, self_offset, row_hits, col_hits, vec);
  SPA_LAUNCH_CHECK(c);
}

// ---------------------------------------------------------------------------------------------- kernel sums
// The pdist grid and K loop; the store is replaced by 128-bit integer sums of p^DEG, p = a.b + C (mc_kernel_pow of motion_code.hpp), over the
// admitted pairs of the tile: a column inside b that is not the row's own, of a row inside a.  A padded row or column has p = C, not 0, so it is
// masked.  A lane adds its four column fragments of a row, the 16 lanes that share the row add theirs by shuffles of the limbs (mc_u128_add
// carries), the two waves that share it meet in LDS (plain writes, a barrier, one add), and the tile's sum goes into global memory by
// ks_atomic_add.  Columns likewise: 16 values in the lane, lanes ^ 16 and ^ 32, the two waves.
__device__ __forceinline__ mc_u128 ks_shfl_xor(mc_u128 v, int off) {
  mc_u128 r;
  r.lo = __shfl_xor((unsigned long long)v.lo, off);
  r.hi = __shfl_xor((unsigned long long)v.hi, off);
  return r;
}
// dst (two 64-bit words: lo, hi) += x as a 128-bit integer, by two 64-bit integer atomics.  The adder whose addend wrapped lo sees it in the value
// its own atomic returns and carries 1 into hi, so every wrap is carried exactly once: the final pair is the exact sum whatever the order of the
// adders, and two runs give equal bits.  The pair is only read after the kernel has finished.
__device__ __forceinline__ void ks_atomic_add(unsigned long long* dst, mc_u128 x) {
  if ((x.lo | x.hi) == 0) return;
  const unsigned long long old = atomicAdd(&dst[0], (unsigned long long)x.lo);
  const unsigned long long up = x.hi + ((old + x.lo) < x.lo ? 1u : 0u);
  if (up) atomicAdd(&dst[1], up);
}

template <int DEG> __global__ __launch_bounds__(256) void motion_kernel_sums_kernel(const int16_t* __restrict__ a, int64_t Ma, const int16_t* __restrict__ b, int64_t Mb, int E,
                                                                                    int64_t self_offset, unsigned long long* row_sums, unsigned long long* col_sums, int vec) {
  __shared__ uint4 sA[PD_BM * 8];
  __shared__ uint4 sB[PD_BN * 8];
  __shared__ mc_u128 sRow[2][PD_BM], sCol[2][PD_BN];   // [the wave column wn that summed it][row], [the wave row wm][column]: every slot written once
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
  const int64_t i0 = (int64_t)blockIdx.y * PD_BM, j0 = (int64_t)blockIdx.x * PD_BN;
  int32_t iacc[4][4][4] = {};
  int na[4] = {0, 0, 0, 0}, nb[4] = {0, 0, 0, 0};
  pd_kloop(a, Ma, b, Mb, E, i0, j0, vec != 0, sA, sB, iacc, na, nb);
  mc_u128 cs[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) cs[n] = mc_u128{0, 0};
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int li = wm * 64 + m * 16 + (lane >> 4) * 4 + r;
      const int64_t i = i0 + li, excl = mc_knn_excluded(i, self_offset);
      mc_u128 rs = mc_u128{0, 0};
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int64_t j = j0 + wn * 64 + n * 16 + (lane & 15);
        if (i < Ma && j < Mb && j != excl) {
          const mc_u128 v = mc_kernel_pow(mc_kernel_p(iacc[m][n][r], E), DEG);
          rs = mc_u128_add(rs, v);
          cs[n] = mc_u128_add(cs[n], v);
        }
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) rs = mc_u128_add(rs, ks_shfl_xor(rs, off));
      if ((lane & 15) == 0) sRow[wn][li] = rs;
    }
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    cs[n] = mc_u128_add(cs[n], ks_shfl_xor(cs[n], 16));
    cs[n] = mc_u128_add(cs[n], ks_shfl_xor(cs[n], 32));
    if (lane < 16) sCol[wm][wn * 64 + n * 16 + lane] = cs[n];
  }
  __syncthreads();
  if (tid < PD_BM) {
    if (row_sums && i0 + tid < Ma) ks_atomic_add(row_sums + 2 * (i0 + tid), mc_u128_add(sRow[0][tid], sRow[1][tid]));
  } else {
    const int t = tid - PD_BM;
    if (col_sums && j0 + t < Mb) ks_atomic_add(col_sums + 2 * (j0 + t), mc_u128_add(sCol[0][t], sCol[1][t]));
  }
}

void k_motion_kernel_sums(spa3d_ctx* c, const int16_t* a, int64_t Ma, const int16_t* b, int64_t Mb, int E, int degree, int64_t self_offset, uint64_t* row_sums,
                          uint64_t* col_sums) {
  if (c->dry) return;
  hipError_t e = hipSuccess;
  if (row_sums) e = hipMemsetAsync(row_sums, 0, sizeof(mc_u128) * Ma, c->stream);
  if (col_sums && e == hipSuccess) e = hipMemsetAsync(col_sums, 0, sizeof(mc_u128) * Mb, c->stream);
  if (e != hipSuccess && c->hip_err == 0) { c->hip_err = (int)e; c->err = std::string("motion_kernel_sums: hipMemsetAsync failed: ") + hipGetErrorString(e); }
  if (c->hip_err) return;
  const int vec = (E % 8 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0) ? 1 : 0;
  const dim3 grid((unsigned)cdiv(Mb, PD_BN), (unsigned)cdiv(Ma, PD_BM));
  unsigned long long* rs = reinterpret_cast<unsigned long long*>(row_sums);
  unsigned long long* cs = reinterpret_cast<unsigned long long*>(col_sums);
  if (degree == 1) motion_kernel_sums_kernel<1><<<grid, 256, 0, c->stream>>>(a, Ma, b, Mb, E, self_offset, rs, cs, vec);
  else if (degree == 2) motion_kernel_sums_kernel<2><<<grid, 256, 0, c->stream>>>(a, Ma, b, Mb, E, self_offset, rs, cs, vec);
  else motion_kernel_sums_kernel<3><<<grid, 256, 0, c->stream>>>(a, Ma, b, Mb, E, self_offset, rs, cs, vec);
  SPA_LAUNCH_CHECK(c);
}

}  // namespace SPA_NS

// ---- the entry points ----
static_assert(MC_POOL_TOKEN == SPA3D_POOL_TOKEN && MC_POOL_CLIP == SPA3D_POOL_CLIP && MC_PDIST_DOT == SPA3D_PDIST_DOT && MC_PDIST_SQDIST == SPA3D_PDIST_SQDIST,
              "motion_code.hpp and include/spa3d.h name the same values");
extern "C" {

int spa3d_motion_codes(spa3d_handle h, const float* latents, int64_t n, int16_t* codes, int32_t* bad, void* stream) {
  if (!h) return SPA3D_ERR_ARG;
  h->err.clear(); h->hip_err = 0;
  auto refuse = [&](const std::string& m) { h->err = "motion_codes: " + m; return SPA3D_ERR_ARG; };
  if (!latents) return refuse("latents is required");
  if (!codes) return refuse("codes is required");
  if (!bad) return refuse("bad is required");
  if (mc_codes_check(n) != MC_OK) return refuse("n = " + std::to_string(n) + " is negative");
  h->stream = (hipStream_t)stream; h->dry = false;
  SPA_NS::k_motion_codes(h, latents, n, codes, bad);
  return h->hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}

int spa3d_motion_moments_add(spa3d_handle h, const int16_t* codes, int64_t M, int32_t L, int32_t D, int32_t pool, int64_t* state, void* stream) {
  if (!h) return SPA3D_ERR_ARG;
  h->err.clear(); h->hip_err = 0;
  auto refuse = [&](const std::string& m) { h->err = "motion_moments_add: " + m; return SPA3D_ERR_ARG; };
  if (!codes) return refuse("codes is required");
  if (!state) return refuse("state is required");
  switch (mc_moments_check(M, L, D, pool)) {
    case MC_BAD_M: return refuse("M = " + std::to_string(M) + " is outside [1, 2^40]");
    case MC_BAD_L: return refuse("L = " + std::to_string(L) + " is outside [1, " + std::to_string(MC_MAX_L) + "]");
    case MC_BAD_D: return refuse("D = " + std::to_string(D) + " is outside [1, " + std::to_string(MC_MAX_D) + "]");
    case MC_BAD_POOL: return refuse("pool = " + std::to_string(pool) + " is neither SPA3D_POOL_TOKEN nor SPA3D_POOL_CLIP");
    default: break;
  }
  h->stream = (hipStream_t)stream; h->dry = false;
  SPA_NS::k_motion_moments(h, codes, M, L, D, pool, state);
  return h->hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}

int spa3d_motion_pdist(spa3d_handle h, const int16_t* a, int64_t Ma, const int16_t* b, int64_t Mb, int32_t E, int32_t kind, int32_t* out, void* stream) {
  if (!h) return SPA3D_ERR_ARG;
  h->err.clear(); h->hip_err = 0;
  auto refuse = [&](const std::string& m) { h->err = "motion_pdist: " + m; return SPA3D_ERR_ARG; };
  if (!a) return refuse("a is required");
  if (!b) return refuse("b is required");
  if (!out) return refuse("out is required");
  switch (mc_pdist_check(Ma, Mb, E, kind)) {
    case MC_BAD_M: return refuse("Ma = " + std::to_string(Ma) + " is outside [1, 2^22]");
    case MC_BAD_MB: return refuse("Mb = " + std::to_string(Mb) + " is outside [1, 2^22]");
    case MC_BAD_E: return refuse("E = " + std::to_string(E) + " is outside [1, " + std::to_string(MC_MAX_E) + "]");
    case MC_BAD_KIND: return refuse("kind = " + std::to_string(kind) + " is neither SPA3D_PDIST_DOT nor SPA3D_PDIST_SQDIST");
    default: break;
  }
  h->stream = (hipStream_t)stream; h->dry = false;
  SPA_NS::k_motion_pdist(h, a, Ma, b, Mb, E, kind, out);
  return h->hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}

// what the streaming entries say about the sizes they share with spa3d_motion_pdist and about self_offset; empty: not one of those
static std::string motion_set_refusal(int code, int64_t Ma, int64_t Mb, int32_t E, int64_t self_offset) {
  switch (code) {
    case MC_BAD_M: return "Ma = " + std::to_string(Ma) + " is outside [1, 2^22]";
    case MC_BAD_MB: return "Mb = " + std::to_string(Mb) + " is outside [1, 2^22]";
    case MC_BAD_E: return "E = " + std::to_string(E) + " is outside [1, " + std::to_string(MC_MAX_E) + "]";
    case MC_BAD_SELF: return "self_offset = " + std::to_string(self_offset) + " is below -1";
    default: return "";
  }
}

int64_t spa3d_motion_knn_workspace_bytes(int64_t Ma, int64_t Mb, int32_t k, int32_t splits) { return mc_knn_ws_bytes(Ma, Mb, k, splits); }

int spa3d_motion_knn(spa3d_handle h, const int16_t* a, int64_t Ma, const int16_t* b, int64_t Mb, int32_t E, int32_t k, int64_t self_offset, int32_t splits, int32_t* dist,
                     int32_t* idx, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!h) return SPA3D_ERR_ARG;
  h->err.clear(); h->hip_err = 0;
  auto refuse = [&](const std::string& m) { h->err = "motion_knn: " + m; return SPA3D_ERR_ARG; };
  if (!a) return refuse("a is required");
  if (!b) return refuse("b is required");
  if (!dist) return refuse("dist is required");
  if (!idx) return refuse("idx is required");
  const int code = mc_knn_check(Ma, Mb, E, k, self_offset, splits);
  if (code == MC_BAD_K)
    return refuse("k = " + std::to_string(k) + " is outside [1, " + std::to_string(std::min<int64_t>(MC_KNN_MAX_K, mc_knn_admissible(Mb, self_offset))) + "]: at most " +
                  std::to_string(MC_KNN_MAX_K) + ", and no more than the " + std::to_string(mc_knn_admissible(Mb, self_offset)) + " columns a row may take");
  if (code == MC_BAD_SPLITS) return refuse("splits = " + std::to_string(splits) + " is outside [0, " + std::to_string(MC_KNN_MAX_SPLITS) + "]");
  if (code != MC_OK) return refuse(motion_set_refusal(code, Ma, Mb, E, self_offset));
  const int n = splits == 0 ? mc_knn_splits(Ma, Mb) : splits;
  const int64_t need = mc_knn_ws_bytes(Ma, Mb, k, n);
  if (need > 0 && !workspace) return refuse("workspace is required with " + std::to_string(n) + " column ranges (" + std::to_string(need) + " bytes)");
  if (workspace_bytes < need) return refuse("workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(need) + " needed (spa3d_motion_knn_workspace_bytes)");
  if (need > 0 && ((uintptr_t)workspace & 7) != 0) return refuse("workspace is not 8-byte aligned");
  h->stream = (hipStream_t)stream; h->dry = false;
  SPA_NS::k_motion_knn(h, a, Ma, b, Mb, E, k, self_offset, n, dist, idx, workspace);
  return h->hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}

int spa3d_motion_ball_hits(spa3d_handle h, const int16_t* a, int64_t Ma, const int16_t* b, int64_t Mb, int32_t E, const int32_t* radius, int64_t self_offset, int32_t* row_hits,
                           int32_t* col_hits, void* stream) {
  if (!h) return SPA3D_ERR_ARG;
  h->err.clear(); h->hip_err = 0;
  auto refuse = [&](const std::string& m) { h->err = "motion_ball_hits: " + m; return SPA3D_ERR_ARG; };
  if (!a) return refuse("a is required");
  if (!b) return refuse("b is required");
  if (!radius) return refuse("radius is required");
  if (!row_hits && !col_hits) return refuse("one of row_hits and col_hits is required");
  const int code = mc_ball_check(Ma, Mb, E, self_offset);
  if (code != MC_OK) return refuse(motion_set_refusal(code, Ma, Mb, E, self_offset));
  h->stream = (hipStream_t)stream; h->dry = false;
  SPA_NS::k_motion_ball_hits(h, a, Ma, b, Mb, E, radius, self_offset, row_hits, col_hits);
  return h->hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}

int spa3d_motion_kernel_sums(spa3d_handle h, const int16_t* a, int64_t Ma, const int16_t* b, int64_t Mb, int32_t E, int32_t degree, int64_t self_offset, uint64_t* row_sums,
                             uint64_t* col_sums, void* stream) {
  if (!h) return SPA3D_ERR_ARG;
  h->err.clear(); h->hip_err = 0;
  auto refuse = [&](const std::string& m) { h->err = "motion_kernel_sums: " + m; return SPA3D_ERR_ARG; };
  if (!a) return refuse("a is required");
  if (!b) return refuse("b is required");
  if (!row_sums && !col_sums) return refuse("one of row_sums and col_sums is required");
  const int code = mc_ksum_check(Ma, Mb, E, degree, self_offset);
  if (code == MC_BAD_DEGREE) return refuse("degree = " + std::to_string(degree) + " is outside [1, " + std::to_string(MC_KERNEL_MAX_DEGREE) + "]");
  if (code != MC_OK) return refuse(motion_set_refusal(code, Ma, Mb, E, self_offset));
  if (((uintptr_t)row_sums & 7) != 0) return refuse("row_sums is not 8-byte aligned");
  if (((uintptr_t)col_sums & 7) != 0) return refuse("col_sums is not 8-byte aligned");
  h->stream = (hipStream_t)stream; h->dry = false;
  SPA_NS::k_motion_kernel_sums(h, a, Ma, b, Mb, E, degree, self_offset, row_sums, col_sums);
  return h->hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}

}  // extern "C"
