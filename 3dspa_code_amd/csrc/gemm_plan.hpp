// gemm_plan.hpp -- which kernel runs a GEMM.  The one place that decides it: the launchers in gemm_fast.hip, gemm_rs.hip, gemm_ntb.hip,
// gemm_tnb.hip and mlp_fused.hip launch the kernel they are given, and the workspace-sizing dry run makes the same plan as the real run
// because the plan is a pure function of the descriptor, the policy and the operand pointers.  Host-only, no HIP headers: plain
// g++ -std=c++17 compiles it (tests/test_gemm_plan_host.py checks the decisions on the CPU).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <initializer_list>

// ------------------------------------------------------------------------------------------
// GEMM descriptor (generic, batched, strided).  C[b][m][n] (op)= alpha*sum_k A[b][m][k]*B[b][k][n]
// ------------------------------------------------------------------------------------------
enum { EPI_NONE = 0, EPI_GELU = 1, EPI_MUL_GELU_GRAD = 2 };
struct GemmDesc {
  const void* A; const void* B; void* C;
  int64_t M; int32_t N; int32_t K;
  int64_t sAm, sAk, sBk, sBn, sCm;   // element strides (C is n-contiguous)
  int32_t nb1 = 1, nb2 = 1;          // two-level batch: blockIdx.z = b1*nb2 + b2
  int64_t bA1 = 0, bA2 = 0, bB1 = 0, bB2 = 0, bC1 = 0, bC2 = 0;
  float alpha = 1.f;
  const float* bias = nullptr;       // [N] f32, added before act
  int epi = EPI_NONE;
  const void* aux = nullptr;         // residual (added after act) or pre-activation (EPI_MUL_GELU_GRAD); C layout, T
  int aux_is_residual = 1;
  int out_f32 = 0;                   // C is float regardless of T
  int accumulate = 0;                // C += (non-atomic)
  int atomic = 0;                    // C += via atomicAdd (f32 C only)
  float* colsum_out = nullptr;       // TN (dW) only: also accumulate the column sums of B (bias gradient) when the kernel can (gemm_tn_fuses_colsum)
  const void* Bt = nullptr;          // optional copy of B stored [N][K] (K contiguous, row stride ldBt) for the tiled kernels
  int64_t ldBt = 0;
  const void* rs_pk = nullptr;       // optional: B as the row-stationary kernel's fragment stream (gemm_rs_pack; K = 384)
  const void* ntb_pk = nullptr;      // optional: B as the large-register-tile NT kernel's fragment stream (gemm_ntb_pack)
  int32_t crow_group = 0, crow_skip = 0;  // C row m is stored at row m + (m/crow_group + 1)*crow_skip (token rows behind a readout row)
  int32_t brow_group = 0, brow_skip = 0;  // same remap on B's k index (dW over token rows that skip the readout row)
  void* pre_out = nullptr;                // with EPI_GELU: the pre-activation (T, C layout) is stored here as well
  const void* zero_page = nullptr;        // >= 16 B of zeros (tiled TN kernel: rows past the end of the reduction)
  // one-pass input embedding (tiled NT, N == 384, 16-bit): K columns [0, K1) from A, [K1, K) from A2 (row stride sA2m); input rows gathered through
  // arow_idx (both sources; also indexes r1_x), output rows scattered through crow_idx (< 0 = dropped); epilogue += r1_x[input row] * r1_w[n] in f32.
  // plan_nt refuses what it cannot honour (the caller then takes the multi-pass path)
  const void* A2 = nullptr; int64_t sA2m = 0; int32_t K1 = 0; const int32_t* arow_idx = nullptr; const int32_t* crow_idx = nullptr;
  const void* r1_x = nullptr; const float* r1_w = nullptr;
  int32_t seg_n = 0; void* C_seg[2] = {nullptr, nullptr};  // tiled TN (dW) only: output columns in seg_n-wide segments, segment s >= 1 in C_seg[s-1]
                                                          // (the q / k / v kernels of a fused projection are separate leaves); plan_tn refuses
                                                          // what it cannot honour
};

// every kernel a GEMM can run on.  Refuse: none the policy allows takes it (the model falls back, ops return SPA3D_ERR_ARG); Generic:
// gemm_generic_kernel<T>.  NT (C = A . B): gemm_rs_kernel<false / true (EPI_MUL_GELU_GRAD)> on rs_pk; gemm_ntb_kernel<4,6,.> (384 | N) / <6,4,.> on
// ntb_pk; mlp_fused_fwd_kernel (plan_mlp); gemm_nt8p_kernel<4,6,EMB=true> (one-pass embedding); gemm_nt8pp_kernel<8,4,..> / <4,6,..> (persistent
// 256 x 256 / 128 x 384); gemm_nt8p_kernel<8,4> / <4,6>; gemm_nt_occ_kernel; gemm_nt_kernel.  dW (C += A^T . B): gemm_tnb_kernel (+ gemm_tn_tail_kernel);
// gemm_tn8p_kernel<4,2> / <2,3> / <6,1> (256 x 256 / 128 x 384 / 384 x 128 tiles); gemm_tn_kernel.
enum class GemmKernel { Refuse, Generic, Rs, Ntb, MlpFused, NtEmbed, Nt8pp256, Nt8pp384, Nt8p256, Nt8p384, NtOcc, Nt,
                        Tnb, Tn8p256, Tn8p128x384, Tn8p384x128, Tn };
inline bool gemm_is_tn(GemmKernel k) { return k >= GemmKernel::Tnb; }

enum class Use { Off, BySize, Any };   // a kernel: never | at or above its row threshold | whatever the row count (test hooks)

// The kernel-choice switches behind "gemm_impl" (include/spa3d.h) and the `impl` of spa3d_op_linear*.
struct GemmPolicy {
  bool generic = false;                  // 1: the generic kernel only
  GemmKernel only = GemmKernel::Refuse;  // spa3d_op_linear 7 / 10: Rs / Ntb whatever the row count, or nothing (Refuse: no such restriction)
  bool rs = true;                        // row-stationary K = 384 kernel from 512 rows (6: off)
  Use ntb = Use::BySize;                 // large-register-tile NT kernel from 65 536 rows (9: any; 3, 4, 6, 8: off)
  Use tnb = Use::BySize;                 // large-register-tile dW kernel from 65 536 rows (same values)
  Use nt8p = Use::BySize;                // 8-phase NT kernels from 16 384 rows (3, 4, 9: any)
  Use tn8p = Use::BySize;                // 8-phase dW kernels from 65 536 rows and at most 25 % tile padding (3, 4, 9: any)
  bool nt8pp384 = true;                  // persistent form of the 128 x 384 NT kernel (4: off, the non-persistent kernel runs)
  bool nt_occ = true;                    // single-buffer short-K NT kernel (5: off, the double-buffered kernel runs)
  bool mlp_fused = true;                 // MLP forward as one kernel (6: off, two GEMMs)
  bool embed_fused = true;               // one-pass input embedding (6: off, the multi-pass path)
  // 0 product dispatch | 1 generic only | 2 tiled (the product dispatch; ops: an error when no tiled kernel takes the GEMM) | 3-6, 8, 9 test hooks
  // (include/spa3d.h "gemm_impl") | 7 / 10 one kernel or an error (spa3d_op_linear).  Every other value is the product dispatch.
  static GemmPolicy from_impl(int v) {
    GemmPolicy p;
    p.generic = v == 1;
    if (v == 3 || v == 4 || v == 9) p.nt8p = p.tn8p = Use::Any;
    if (v == 3 || v == 4 || v == 6 || v == 8) p.ntb = p.tnb = Use::Off;
    if (v == 9) p.ntb = p.tnb = Use::Any;
    p.nt8pp384 = v != 4; p.nt_occ = v != 5; p.rs = p.mlp_fused = p.embed_fused = v != 6;
    p.only = v == 7 ? GemmKernel::Rs : (v == 10 ? GemmKernel::Ntb : GemmKernel::Refuse);
    return p;
  }
};

inline bool gemm_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool gemm_on(Use u, int64_t rows, int64_t threshold) { return u == Use::Any || (u == Use::BySize && rows >= threshold); }

// ---- shape predicates of the packed-weight kernels.  gemm_rs.hip: the contraction it is built for, and bias rows in LDS (144 KiB ring + 9 KiB)
constexpr int RS_K = 384, RS_MAXN = 2304;
inline bool gemm_rs_ok(int K, int N) { return K == RS_K && N >= 256 && N <= RS_MAXN && N % 128 == 0; }
inline int ntb_wn(int N) { return N % 384 == 0 ? 6 : (N % 256 == 0 ? 4 : 0); }
// K >= 64: gemm_ntb_kernel's phase loop is a do-while behind the peeled first phase
inline bool gemm_ntb_ok(int K, int N) { return ntb_wn(N) != 0 && K % 32 == 0 && K >= 64; }

inline bool gemm_emb(const GemmDesc& d) { return d.A2 || d.arow_idx || d.crow_idx || d.r1_x; }
inline bool gemm_plain_nt(const GemmDesc& d) {   // a dense 16-bit C = A . B (+ bias): what the packed-weight kernels take (Rs also EPI_MUL_GELU_GRAD)
  return d.M >= 1 && d.sAk == 1 && d.nb1 == 1 && d.nb2 == 1 && d.alpha == 1.f && !d.out_f32 && !d.accumulate && !d.atomic && !d.crow_group && !d.pre_out &&
         !gemm_emb(d) && d.sAm % 8 == 0 && d.sCm % 8 == 0 && gemm_aligned16(d.A) && gemm_aligned16(d.C);
}
inline bool rs_takes(const GemmDesc& d) {
  const bool gelu = d.epi == EPI_MUL_GELU_GRAD;   // C = (A . B + bias) o gelu'(aux)
  if (!d.rs_pk || !gemm_rs_ok(d.K, d.N) || !gemm_plain_nt(d)) return false;
  return gelu ? d.aux && gemm_aligned16(d.aux) : d.epi == EPI_NONE && !d.aux;
}
inline bool ntb_takes(const GemmDesc& d) {
  if (!d.ntb_pk || !gemm_ntb_ok(d.K, d.N) || !gemm_plain_nt(d) || d.epi != EPI_NONE || d.aux || d.sAm > (1 << 20) || d.sCm > (1 << 20)) return false;
  if (!gemm_aligned16(d.ntb_pk) || !gemm_aligned16(d.bias)) return false;
  return ((d.M + 255) / 256) * (int64_t)(d.N / 256 + 1) <= (int64_t(1) << 30);   // the kernel's tile ids are 32-bit
}

// ---- C = A . B: the packed-weight kernels (when the descriptor carries their stream), else the tiled kernels; Refuse when none takes it
inline GemmKernel plan_nt_tiled(const GemmDesc& d, const GemmPolicy& p) {
  using K = GemmKernel;
  if (!d.Bt && d.sBk != 1) return K::Refuse;   // needs B as [N][K], K contiguous: the explicit transposed copy or B itself
  const void* Bt = d.Bt ? d.Bt : d.B; const int64_t ldb = d.Bt ? d.ldBt : d.sBn;
  if (d.sAk != 1 || d.nb1 != 1 || d.nb2 != 1 || d.atomic) return K::Refuse;
  if (d.K % 64 || d.N % 8 || d.M < 1 || d.K < 64) return K::Refuse;
  if (d.sAm % 8 || ldb % 8 || d.sCm % 8 || !gemm_aligned16(d.A) || !gemm_aligned16(Bt) || !gemm_aligned16(d.C)) return K::Refuse;
  if ((d.aux && (!gemm_aligned16(d.aux) || d.out_f32)) || !gemm_aligned16(d.bias) || (d.pre_out && (!gemm_aligned16(d.pre_out) || d.out_f32))) return K::Refuse;
  if ((int64_t)d.M * d.N < 128 * 128) return K::Refuse;  // tiny problems: the generic kernel has less tail waste
  if (((d.M + 127) / 128 + 7) / 8 * 8 * ((d.N + 127) / 128) > 0x7fffffffLL) return K::Refuse;   // 32-bit grid
  if (gemm_emb(d)) {  // one-pass input embedding: only the non-persistent 128 x 384 8-phase kernel carries these operands
    if (!p.embed_fused || d.N != 384 || d.out_f32 || d.accumulate || d.aux || d.pre_out || d.epi != EPI_NONE || d.crow_group) return K::Refuse;
    if ((d.A2 && (d.K1 % 64 || d.K1 <= 0 || d.K1 >= d.K || d.sA2m % 8 || !gemm_aligned16(d.A2))) || (d.r1_x && !d.r1_w)) return K::Refuse;
    return K::NtEmbed;
  }
  // 8-phase kernels: 256x256 when 256 | N, 128x384 when 384 | N (gemm_fast.hip has the measurements)
  if ((d.N % 256 == 0 || d.N % 384 == 0) && gemm_on(p.nt8p, d.M, 256 * 64)) {
    // persistent forms (accumulate would add loads to the counted wait)
    const bool pers_ok = d.K >= 128 && !d.accumulate && d.crow_group == 0 && d.M % 8 == 0 && (!d.aux || (!d.pre_out && !d.out_f32));
    if (pers_ok && d.N % 256 == 0) return K::Nt8pp256;
    if (pers_ok && p.nt8pp384 && !d.pre_out && !d.out_f32 && d.N % 384 == 0) return K::Nt8pp384;
    return d.N % 256 == 0 ? K::Nt8p256 : K::Nt8p384;
  }
  return p.nt_occ && d.K / 64 <= 8 ? K::NtOcc : K::Nt;   // short K: single LDS buffer, 4 workgroups/CU
}
inline GemmKernel plan_nt(const GemmDesc& d, const GemmPolicy& p) {
  using K = GemmKernel;
  if (p.generic) return K::Refuse;
  if (p.only == K::Rs) return rs_takes(d) ? K::Rs : K::Refuse;
  if (p.only == K::Ntb) return ntb_takes(d) ? K::Ntb : K::Refuse;
  if (p.rs && d.M >= 512 && rs_takes(d)) return K::Rs;
  if (gemm_on(p.ntb, d.M, 65536) && ntb_takes(d)) return K::Ntb;
  return plan_nt_tiled(d, p);
}

// ---- dW: C[Ki = d.M][N] += A^T . B over M = d.K rows (f32 C).  Refuse when no dW kernel takes it
inline bool tnb_takes(const GemmDesc& d) {   // gemm_tnb.hip; the caller has checked what every dW kernel needs
  const int Ki = (int)d.M, N = d.N;
  if (!((Ki % 384 == 0 && N % 256 == 0) || (Ki % 256 == 0 && N % 384 == 0))) return false;
  if (d.sAk > (1 << 24) || d.sBk > (1 << 24)) return false;   // 32-bit lane offsets
  // the skips a lane accumulates over a split stay in 32 bits
  return d.brow_group == 0 || (d.brow_group >= 16 && (d.K / d.brow_group + 2) * (int64_t)d.brow_skip * d.sBk * 2 < (int64_t(1) << 31));
}
// 8-phase dW tile with the least padding: 384 x 128 / 128 x 384 when one dimension is an odd multiple of 384, else 256 x 256; *waste = padded / real area
inline GemmKernel tn8p_tile(int Ki, int N, double* waste) {
  auto w = [&](int TI, int TNN) { return (double)((Ki + TI - 1) / TI * TI) * ((N + TNN - 1) / TNN * TNN) / ((double)Ki * N); };
  const double w0 = w(256, 256), w1 = w(128, 384), w2 = w(384, 128);
  *waste = std::min(w0, std::min(w1, w2));
  if (w0 <= *waste * 1.0001) return GemmKernel::Tn8p256;
  return w1 <= *waste * 1.0001 ? GemmKernel::Tn8p128x384 : GemmKernel::Tn8p384x128;
}
inline GemmKernel plan_tn(const GemmDesc& d, const GemmPolicy& p) {
  using K = GemmKernel;
  if (p.generic) return K::Refuse;
  // A[m'=i][k'=m] = X[m][i]: sAm == 1, sAk == lda ; B[k'=m][n]: sBn == 1, sBk == ldb ; f32 accumulate
  if (d.sAm != 1 || d.sBn != 1 || !d.out_f32 || !d.accumulate || d.nb1 != 1 || d.nb2 != 1) return K::Refuse;
  if (d.epi != EPI_NONE || d.aux || d.bias || d.alpha != 1.f || !d.zero_page) return K::Refuse;
  const int Ki = (int)d.M, N = d.N; const int64_t M = d.K;
  if (Ki % 8 || N % 8 || Ki < 8 || N < 8 || M < 256) return K::Refuse;
  if (d.sAk % 8 || d.sBk % 8 || !gemm_aligned16(d.A) || !gemm_aligned16(d.B)) return K::Refuse;
  // segmented outputs: a 32-column group never straddles a segment; at most three segments; no fused column sums
  if (d.seg_n > 0 && (d.seg_n % 32 || N % d.seg_n || N / d.seg_n > 3 || d.colsum_out)) return K::Refuse;
  if (gemm_on(p.tnb, M, 65536) && tnb_takes(d)) return K::Tnb;
  if (gemm_on(p.tn8p, M, 65536) && (d.brow_group == 0 || d.brow_group >= 16)) {
    double waste;
    const K k = tn8p_tile(Ki, N, &waste);
    if (waste <= 1.25 || p.tn8p == Use::Any) return k;
  }
  return d.seg_n > 0 ? K::Refuse : K::Tn;   // segmented outputs exist in the kernels above only: the caller runs one GEMM per segment
}
// the dW kernel also accumulates d.colsum_out (the bias gradient); otherwise the caller adds the column sums
inline bool gemm_tn_fuses_colsum(GemmKernel k, const GemmDesc& d) { return d.colsum_out && gemm_is_tn(k) && k != GemmKernel::Tn; }

// ---- any other 16-bit GEMM: NT, else dW, else the generic kernel (fp32 GEMMs always run on the generic kernel)
inline GemmKernel plan_gemm(const GemmDesc& d, const GemmPolicy& p) {
  GemmKernel k = plan_nt(d, p);
  if (k == GemmKernel::Refuse) k = plan_tn(d, p);
  return k == GemmKernel::Refuse ? GemmKernel::Generic : k;
}

// ---- packed weights: which streams to build
struct LinStreams { bool rs, rs_t, ntb, ntb_t; };
// for a weight W [K][N] of nseg column segments segw wide: rs / ntb for Y = X . W, rs_t / ntb_t for dX = dY . W^T (training only).  The large-tile
// streams only for a contraction >= 768, the shapes that kernel was measured ahead on (profiles/r05_gemm_ntb_*.log)
inline LinStreams plan_lin_streams(const GemmPolicy& p, int K, int N, int segw, int nseg, bool train) {
  const bool rs = p.rs && !p.generic, ntb = p.ntb != Use::Off && !p.generic;
  return {rs && gemm_rs_ok(K, N) && segw % 64 == 0, rs && train && nseg == 1 && gemm_rs_ok(N, K), ntb && K >= 768 && gemm_ntb_ok(K, N),
          ntb && train && N >= 768 && gemm_ntb_ok(N, K)};
}
// the fused MLP forward's weight stream, for a block of width d and MLP width mlp (the track encoder's self-attention blocks)
inline bool plan_mlp_pack(const GemmPolicy& p, bool cross, int d, int mlp) { return !p.generic && p.mlp_fused && !cross && d == 384 && mlp == 1536; }
// the one-pass input embedding's packed weights and summed biases
inline bool plan_embed_pack(const GemmPolicy& p, bool twoD, int d, int tok_K, int dino_dim, int depth_dim) {
  return !p.generic && p.embed_fused && !twoD && d == 384 && tok_K % 64 == 0 && (dino_dim == 0 || dino_dim % 64 == 0) && depth_dim <= 1;
}
// y = a + MLP(na) with h, hpre kept: MlpFused or Refuse (then two GEMMs).  16-byte vector loads / stores and LDS-DMA on every operand
inline GemmKernel plan_mlp(const GemmPolicy& p, int64_t M, int d, int mlp, const void* wpk, const float* b_in, const float* b_out,
                           const void* na, const void* a, const void* y, const void* h, const void* hpre) {
  if (p.generic || !p.mlp_fused || d != 384 || mlp != 1536 || M < 1 || !wpk || !b_in || !b_out) return GemmKernel::Refuse;
  for (const void* q : {na, a, y, h, hpre, wpk})
    if (!gemm_aligned16(q)) return GemmKernel::Refuse;
  return GemmKernel::MlpFused;
}

// ---- the flags word of the kernel's profiler record (ProfRec::tag[3]; tests/ and tools/ read it): the tiled NT kernels' epilogue bits,
// 512 / 518 row-stationary (plain / gelu'), 256 fused MLP, 1 << 21 | bias large-tile NT, 1 << 20 large-tile dW, 0 8-phase dW, the split count of gemm_tn_kernel
inline int64_t gemm_prof_flags(GemmKernel k, const GemmDesc& d, int64_t splits) {
  using K = GemmKernel;
  if (k == K::Rs) return d.epi == EPI_MUL_GELU_GRAD ? 512 + 6 : 512;
  if (k == K::MlpFused) return 256;
  if (k == K::Ntb) return (1 << 21) | (d.bias ? 1 : 0);
  if (k == K::Tnb) return 1 << 20;
  if (k == K::Tn) return splits;
  if (k < K::Rs || gemm_is_tn(k)) return 0;
  return d.epi | (d.aux ? 4 : 0) | (d.pre_out ? 8 : 0) | (d.out_f32 ? 16 : 0) | (d.accumulate ? 32 : 0) | (d.crow_group ? 64 : 0) | (d.sAm != d.K ? 128 : 0);
}
