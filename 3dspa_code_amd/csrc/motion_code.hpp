// motion_code.hpp -- the integer side of the latent-set metrics (include/spa3d.h: spa3d_motion_codes, spa3d_motion_moments_add, spa3d_motion_pdist).
// Plain C++, host- and device-callable: the kernels of motion.hip, the entry points' range checks and the g++ host test
// (tests/host/motion_code_check.cpp) run THIS code.
//
// Six things live here.
//   The code of a latent: c = (int16) rintf(clip(x, -1, 1) * 128.f), an integer in [-128, 128] -- the integer discretize_kernel (loss.hip) rounds to
//     before it adds the dither.  The product is exact (a power of two), rintf rounds ties to even, +-inf clips to +-128, -0.0 gives 0.  A NaN has
//     no code: it gives 0 and is reported, and the callers count it.
//   The moment state of D-dimensional samples: int64 [1 + D + D * D] = n, s[D] = sum x, S[D][D] = sum x x^T (both triangles), with the index
//     helpers below.  A sample is a token row c[m][l][:] (MC_POOL_TOKEN, |x| <= 128) or a clip's token sum (MC_POOL_CLIP, |x| <= 128 L).
//   The chunk rule of the pairwise-distance GEMM: codes are exact in bf16 (integers up to 256 are), a product of two is at most 128 * 128 = 2^14,
//     and a sum of MOTION_KCHUNK = 1024 of them is at most 2^24 in magnitude, every partial sum an integer of at most that magnitude: exact in the
//     fp32 MFMA accumulator whatever the order.  So after every MOTION_KCHUNK elements of K the accumulator is moved into an int32 and cleared.
//   The range checks of the entries, as codes the entry points turn into messages.
//   The candidate order, the split plan and the workspace size of spa3d_motion_knn, and the checks it shares with spa3d_motion_ball_hits
//     (tests/host/motion_knn_check.cpp runs them under g++).
//   The integer side of spa3d_motion_kernel_sums: the polynomial kernel's numerator p^deg as a 128-bit integer of two 64-bit limbs, the limb add,
//     and the range check (tests/host/motion_kernel_check.cpp runs them under g++).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MC_HD __host__ __device__ __forceinline__
#else
#define MC_HD inline
#endif

constexpr int MC_CODE_MAX = 128;                       // |code| <= 128
constexpr int MOTION_KCHUNK = 1024;                    // K elements between two flushes of the fp32 accumulator
static_assert((int64_t)MOTION_KCHUNK * MC_CODE_MAX * MC_CODE_MAX == (int64_t)1 << 24, "a chunk's largest partial sum is the last integer run fp32 holds exactly");
enum { MC_POOL_TOKEN = 0, MC_POOL_CLIP = 1 };          // = SPA3D_POOL_TOKEN, SPA3D_POOL_CLIP
enum { MC_PDIST_DOT = 0, MC_PDIST_SQDIST = 1 };        // = SPA3D_PDIST_DOT, SPA3D_PDIST_SQDIST
constexpr int MC_MAX_L = 4096, MC_MAX_D = 256;         // moments: tokens per clip, token width
constexpr int MC_MAX_E = 32767;                        // pdist: E * 256^2 < 2^31, so |a|^2 + |b|^2 - 2 a.b fits an int32
constexpr int64_t MC_MAX_M = (int64_t)1 << 22;         // pdist: rows of either set (the launch grid)
static_assert((int64_t)MC_MAX_E * 256 * 256 < ((int64_t)1 << 31), "the squared distance fits an int32");

// ---- the code ----
// the code of x; a NaN gives 0 and sets *nan (left alone otherwise)
MC_HD int16_t mc_code(float x, bool* nan) {
  if (x != x) { *nan = true; return 0; }
  const float c = x < -1.f ? -1.f : (x > 1.f ? 1.f : x);
  return (int16_t)rintf(c * 128.f);
}

// ---- the moment state ----
MC_HD int64_t mc_state_len(int D) { return 1 + (int64_t)D + (int64_t)D * D; }
MC_HD int64_t mc_state_n() { return 0; }
MC_HD int64_t mc_state_s(int i) { return 1 + (int64_t)i; }
MC_HD int64_t mc_state_S(int D, int i, int j) { return 1 + (int64_t)D + (int64_t)i * D + j; }
// samples a call adds, and the largest |x_i x_j| of one sample
MC_HD int64_t mc_samples(int64_t M, int L, int pool) { return pool == MC_POOL_TOKEN ? M * L : M; }
MC_HD int64_t mc_sample_sq_max(int L, int pool) { return pool == MC_POOL_TOKEN ? (int64_t)MC_CODE_MAX * MC_CODE_MAX : (int64_t)MC_CODE_MAX * L * MC_CODE_MAX * L; }
// the largest n whose sums cannot pass 2^62: n * mc_sample_sq_max <= 2^62
MC_HD int64_t mc_samples_max(int L, int pool) { return ((int64_t)1 << 62) / mc_sample_sq_max(L, pool); }

// ---- the range checks ----
enum { MC_OK = 0, MC_BAD_M = 1, MC_BAD_L = 2, MC_BAD_D = 3, MC_BAD_POOL = 4, MC_BAD_E = 5, MC_BAD_KIND = 6, MC_BAD_MB = 7, MC_BAD_N = 8,
       MC_BAD_K = 9, MC_BAD_SELF = 10, MC_BAD_SPLITS = 11, MC_BAD_DEGREE = 12 };
MC_HD int mc_codes_check(int64_t n) { return n < 0 ? MC_BAD_N : MC_OK; }
MC_HD int mc_moments_check(int64_t M, int L, int D, int pool) {
  if (M < 1 || M > ((int64_t)1 << 40)) return MC_BAD_M;
  if (L < 1 || L > MC_MAX_L) return MC_BAD_L;
  if (D < 1 || D > MC_MAX_D) return MC_BAD_D;
  if (pool != MC_POOL_TOKEN && pool != MC_POOL_CLIP) return MC_BAD_POOL;
  return MC_OK;
}
MC_HD int mc_pdist_check(int64_t Ma, int64_t Mb, int E, int kind) {
  if (Ma < 1 || Ma > MC_MAX_M) return MC_BAD_M;
  if (Mb < 1 || Mb > MC_MAX_M) return MC_BAD_MB;
  if (E < 1 || E > MC_MAX_E) return MC_BAD_E;
  if (kind != MC_PDIST_DOT && kind != MC_PDIST_SQDIST) return MC_BAD_KIND;
  return MC_OK;
}

// ---- streaming k-NN and ball hits (spa3d_motion_knn, spa3d_motion_ball_hits) ----
// A candidate of row i is a column j with the squared distance d = d(i, j), 0 <= d < 2^31, and the ORDER of candidates is that of the 64-bit key
// d << 32 | j: by distance, equal distances by the lower column.  Keys of one row are distinct (the columns are), so the order is total and the
// k smallest keys are the same set, in the same order, however the columns were split.  All ones is no key: j never reaches 2^32 - 1.
constexpr int MC_KNN_MAX_K = 64;                         // a wave's lanes hold a row's list
constexpr int MC_KNN_TILE = 128;                         // columns (and rows) of one tile of the distance GEMM
constexpr int MC_KNN_MAX_SPLITS = 4096;                  // forced column ranges (the launch grid's second dimension)
constexpr int MC_KNN_TARGET_GROUPS = 512, MC_KNN_MIN_TILES = 4;   // the plan: two workgroups for each of the 256 CUs, no range below four tiles
constexpr uint64_t MC_KNN_NONE = ~(uint64_t)0;
MC_HD uint64_t mc_knn_key(int32_t d, int64_t j) { return ((uint64_t)(uint32_t)d << 32) | (uint64_t)(uint32_t)j; }
MC_HD int32_t mc_knn_key_dist(uint64_t key) { return (int32_t)(key >> 32); }
MC_HD int32_t mc_knn_key_idx(uint64_t key) { return (int32_t)(key & 0xffffffffu); }
// the column row i leaves out (self_offset >= 0: column i + self_offset; -1: none, returned as -1)
MC_HD int64_t mc_knn_excluded(int64_t i, int64_t self_offset) { return self_offset < 0 ? -1 : i + self_offset; }
// the fewest admissible columns any row has: row 0's own column self_offset lies inside b or no row's does
MC_HD int64_t mc_knn_admissible(int64_t Mb, int64_t self_offset) { return self_offset >= 0 && self_offset < Mb ? Mb - 1 : Mb; }
MC_HD int64_t mc_knn_tiles(int64_t M) { return (M + MC_KNN_TILE - 1) / MC_KNN_TILE; }
// the planned number of column ranges: enough workgroups to fill the chip, as long as every range keeps MC_KNN_MIN_TILES tiles.  Only time
// depends on it.
MC_HD int mc_knn_splits(int64_t Ma, int64_t Mb) {
  const int64_t rt = mc_knn_tiles(Ma), ct = mc_knn_tiles(Mb);
  const int64_t want = (MC_KNN_TARGET_GROUPS + rt - 1) / rt, most = ct / MC_KNN_MIN_TILES;
  const int64_t s = want < most ? want : most;
  return s < 1 ? 1 : (int)s;
}
// column tiles [*t0, *t1) of range s of `splits`: near-equal, in order, empty where there are more ranges than tiles
MC_HD void mc_knn_tile_range(int64_t tiles, int splits, int s, int64_t* t0, int64_t* t1) {
  *t0 = tiles * s / splits;
  *t1 = tiles * (s + 1) / splits;
}
MC_HD int mc_knn_check(int64_t Ma, int64_t Mb, int E, int k, int64_t self_offset, int splits) {
  const int r = mc_pdist_check(Ma, Mb, E, MC_PDIST_SQDIST);
  if (r != MC_OK) return r;
  if (self_offset < -1) return MC_BAD_SELF;
  if (k < 1 || k > MC_KNN_MAX_K || k > mc_knn_admissible(Mb, self_offset)) return MC_BAD_K;
  if (splits < 0 || splits > MC_KNN_MAX_SPLITS) return MC_BAD_SPLITS;
  return MC_OK;
}
// uint64 [splits][Ma][k] when there is more than one range (splits = 0: the plan's); -1 for sizes mc_knn_check refuses
MC_HD int64_t mc_knn_ws_bytes(int64_t Ma, int64_t Mb, int k, int splits) {
  if (Ma < 1 || Ma > MC_MAX_M || Mb < 1 || Mb > MC_MAX_M || k < 1 || k > MC_KNN_MAX_K || splits < 0 || splits > MC_KNN_MAX_SPLITS) return -1;
  const int n = splits == 0 ? mc_knn_splits(Ma, Mb) : splits;
  return n == 1 ? 0 : (int64_t)n * Ma * k * (int64_t)sizeof(uint64_t);
}
MC_HD int mc_ball_check(int64_t Ma, int64_t Mb, int E, int64_t self_offset) {
  const int r = mc_pdist_check(Ma, Mb, E, MC_PDIST_SQDIST);
  if (r != MC_OK) return r;
  return self_offset < -1 ? MC_BAD_SELF : MC_OK;
}

// ---- kernel sums (spa3d_motion_kernel_sums) ----
// The polynomial kernel (x.y / E + 1)^deg of x = a / 128 is p^deg / C^deg with C = 16384 E and p = a.b + C, an integer in [0, 2 C], 2 C < 2^30.
// p^deg < 2^90, and a sum of at most MC_MAX_M = 2^22 of them is below 2^112: an unsigned 128-bit integer, kept as two 64-bit limbs.
struct mc_u128 { uint64_t lo, hi; };
// a + b mod 2^128: lo wrapped exactly when the wrapped sum is below the addend's lo
MC_HD mc_u128 mc_u128_add(mc_u128 a, mc_u128 b) {
  mc_u128 r;
  r.lo = a.lo + b.lo;
  r.hi = a.hi + b.hi + (r.lo < b.lo ? 1u : 0u);
  return r;
}
constexpr int MC_KERNEL_MAX_DEGREE = 3;
MC_HD int64_t mc_kernel_base(int E) { return (int64_t)16384 * E; }
static_assert((int64_t)2 * 16384 * MC_MAX_E < ((int64_t)1 << 30), "p = a.b + C stays below 2^30");
// p of the exact dot product of two rows of codes, |dot| <= C
MC_HD uint32_t mc_kernel_p(int32_t dot, int E) { return (uint32_t)((int64_t)dot + mc_kernel_base(E)); }
// p^deg for p < 2^30, deg in {1, 2, 3}.  p^2 < 2^60 fits the low limb; p^3 = p^2 p is a 64 x 32 -> 96-bit product taken in two halves of p^2:
// q_lo p < 2^62 and q_hi p < 2^58 (q_hi < 2^28), the second shifted up 32 bits.
MC_HD mc_u128 mc_kernel_pow(uint32_t p, int deg) {
  mc_u128 r;
  r.hi = 0;
  if (deg == 1) { r.lo = p; return r; }
  const uint64_t q = (uint64_t)p * p;
  if (deg == 2) { r.lo = q; return r; }
  const uint64_t t0 = (q & 0xffffffffu) * p, t1 = (q >> 32) * p;
  r.lo = t0 + (t1 << 32);
  r.hi = (t1 >> 32) + (r.lo < t0 ? 1u : 0u);
  return r;
}
MC_HD int mc_ksum_check(int64_t Ma, int64_t Mb, int E, int deg, int64_t self_offset) {
  const int r = mc_pdist_check(Ma, Mb, E, MC_PDIST_DOT);
  if (r != MC_OK) return r;
  if (deg < 1 || deg > MC_KERNEL_MAX_DEGREE) return MC_BAD_DEGREE;
  return self_offset < -1 ? MC_BAD_SELF : MC_OK;
}
