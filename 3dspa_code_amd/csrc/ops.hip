// ops.hip -- single-op C-ABI entry points (spa3d_op_*): each building block of the hot path callable on
// its own so tests/ can compare every kernel with the oracle.  Thin wrappers over the same kernels the
// model orchestration uses.
#include <cmath>

#include "common.hpp"

namespace SPA_NS {
namespace {
struct OpCtx : spa3d_ctx {
  OpCtx(void* stream_, void* ws, int64_t ws_bytes) {  // (no environment switches: kernel choice comes from the entry point's `impl` argument)
    stream = (hipStream_t)stream_; ar.base = (char*)ws; ar.cap = ws_bytes;
  }
  template <typename U> U* alloc(int64_t n) { return (U*)ar.alloc(n * (int64_t)sizeof(U)); }
  int status() { return ar.overflow ? SPA3D_ERR_WORKSPACE : (hip_err ? SPA3D_ERR_HIP : SPA3D_OK); }
};

template <typename T>
int op_linear(OpCtx& c, const T* A, const T* B, const float* bias, const T* res, T* C, int64_t M, int N, int K, int act, int impl) {
  GemmDesc d{};
  d.A = A; d.B = B; d.C = C; d.M = M; d.N = N; d.K = K; d.sAm = K; d.sAk = 1; d.sBk = N; d.sBn = 1; d.sCm = N;
  d.bias = bias; d.epi = act == 1 ? EPI_GELU : (act == 2 ? EPI_MUL_GELU_GRAD : EPI_NONE); d.aux = res;  // act 2: C = (A.B + bias) o gelu'(residual)
  const GemmPolicy p = GemmPolicy::from_impl(impl & 15);
  if constexpr (sizeof(T) == 2) {
    if (p.only != GemmKernel::Refuse) {  // 7 / 10: the row-stationary K = 384 kernel (gemm_rs.hip) / the large-register-tile NT kernel (gemm_ntb.hip) or an error
      const bool rs = p.only == GemmKernel::Rs;
      const void*& pk = rs ? d.rs_pk : d.ntb_pk;
      pk = A;   // stand-in for the packed stream (A must be 16-byte aligned too): a wrong shape is an argument error whatever the workspace
      if (plan_nt(d, p) != p.only) return SPA3D_ERR_ARG;
      T* w = c.alloc<T>(rs ? gemm_rs_pack_elems(N) : gemm_ntb_pack_elems(K, N));
      if (c.ar.overflow) return SPA3D_ERR_WORKSPACE;
      if (rs) gemm_rs_pack<T>(&c, B, N, 1, N, w); else gemm_ntb_pack<T>(&c, B, N, 1, K, N, w);
      pk = w;
      if (plan_nt(d, p) != p.only) return SPA3D_ERR_ARG;   // (a misaligned workspace)
      gemm_launch<T>(&c, d, p.only);
      return c.status();
    }
    if (impl != 1) {
      // impl | 16 (benchmarks): the MLP-in form of the step -- a second output stream (the pre-activation) from the same epilogue
      if (impl & 16) { d.pre_out = c.alloc<T>(M * N); if (c.ar.overflow) return SPA3D_ERR_WORKSPACE; }
      T* Bt = c.alloc<T>((int64_t)K * N);
      if (c.ar.overflow) return SPA3D_ERR_WORKSPACE;
      k_transpose<T>(&c, B, K, N, Bt);
      d.Bt = Bt; d.ldBt = K;
      const GemmKernel k = plan_nt(d, GemmPolicy::from_impl((impl & 15) == 1 ? 0 : impl & 15));   // (17, 33 ...: the product dispatch, as always)
      if (k != GemmKernel::Refuse) { gemm_launch<T>(&c, d, k); return c.status(); }
    }
  }
  if ((impl & 15) >= 2) return SPA3D_ERR_ARG;   // tiled (or one kernel) or an error
  gemm_launch<T>(&c, d, GemmKernel::Generic);
  return c.status();
}

template <typename T>
int op_linear_bwd(OpCtx& c, const T* A, const T* B, const T* dC, T* dA, float* dB, float* dbias, int64_t M, int N, int K, int impl) {
  // 10: dA on the large-register-tile NT kernel or an error; 7 names no dA kernel here and is a tiled request like 2
  const GemmPolicy p = GemmPolicy::from_impl(impl == 7 ? 2 : impl);
  if (dA) {  // dA[M,K] = dC[M,N] . B[K,N]^T
    GemmDesc d{};
    d.A = dC; d.B = B; d.C = dA; d.M = M; d.N = K; d.K = N; d.sAm = N; d.sAk = 1; d.sBk = 1; d.sBn = N; d.sCm = K;
    d.Bt = B; d.ldBt = N;
    GemmKernel k = GemmKernel::Refuse;
    if constexpr (sizeof(T) == 2) {
      if (p.only == GemmKernel::Ntb) {  // element (k' = n, n' = k) of B^T is B[k * N + n]
        d.ntb_pk = dC;   // stand-in for the packed stream, as in op_linear
        if (plan_nt(d, p) != GemmKernel::Ntb) return SPA3D_ERR_ARG;
        T* pk = c.alloc<T>(gemm_ntb_pack_elems(N, K));
        if (c.ar.overflow) return SPA3D_ERR_WORKSPACE;
        gemm_ntb_pack<T>(&c, B, 1, N, N, K, pk);
        d.ntb_pk = pk;
      }
      k = plan_nt(d, p);
    }
    if (k == GemmKernel::Refuse) { if (impl >= 2) return SPA3D_ERR_ARG; k = GemmKernel::Generic; }
    gemm_launch<T>(&c, d, k);
  }
  if (dB) {  // dB[K,N] = A[M,K]^T . dC[M,N]
    k_zero(&c, dB, (int64_t)K * N * 4);
    GemmDesc d{};
    d.A = A; d.B = dC; d.C = dB; d.M = K; d.N = N; d.K = M; d.sAm = 1; d.sAk = K; d.sBk = N; d.sBn = 1; d.sCm = N;
    d.out_f32 = 1; d.accumulate = 1;
    void* zp = c.alloc<char>(256); k_zero(&c, zp, 256); d.zero_page = zp;
    GemmKernel k = GemmKernel::Refuse;
    if constexpr (sizeof(T) == 2) k = plan_tn(d, p);
    if (k == GemmKernel::Refuse) { if (impl >= 2) return SPA3D_ERR_ARG; k = GemmKernel::Generic; }
    gemm_launch<T>(&c, d, k);
  }
  if (dbias) { k_zero(&c, dbias, (int64_t)N * 4); k_colsum<T>(&c, dC, M, N, N, dbias); }
  return c.status();
}

// the header's kernel ids are GemmKernel's values (tests/test_gemm_desc_host.py compares the names as well)
#define OP_GEMM_ID(id, k) static_assert(id == (int)GemmKernel::k, #id)
OP_GEMM_ID(SPA3D_GEMM_REFUSE, Refuse); OP_GEMM_ID(SPA3D_GEMM_GENERIC, Generic); OP_GEMM_ID(SPA3D_GEMM_RS, Rs); OP_GEMM_ID(SPA3D_GEMM_NTB, Ntb);
OP_GEMM_ID(SPA3D_GEMM_MLP_FUSED, MlpFused); OP_GEMM_ID(SPA3D_GEMM_NT_EMBED, NtEmbed); OP_GEMM_ID(SPA3D_GEMM_NT8PP256, Nt8pp256);
OP_GEMM_ID(SPA3D_GEMM_NT8PP384, Nt8pp384); OP_GEMM_ID(SPA3D_GEMM_NT8P256, Nt8p256); OP_GEMM_ID(SPA3D_GEMM_NT8P384, Nt8p384);
OP_GEMM_ID(SPA3D_GEMM_NT_OCC, NtOcc); OP_GEMM_ID(SPA3D_GEMM_NT, Nt); OP_GEMM_ID(SPA3D_GEMM_TNB, Tnb); OP_GEMM_ID(SPA3D_GEMM_TN8P256, Tn8p256);
OP_GEMM_ID(SPA3D_GEMM_TN8P128X384, Tn8p128x384); OP_GEMM_ID(SPA3D_GEMM_TN8P384X128, Tn8p384x128); OP_GEMM_ID(SPA3D_GEMM_TN, Tn);
#undef OP_GEMM_ID
static_assert(SPA3D_EPI_NONE == EPI_NONE && SPA3D_EPI_GELU == EPI_GELU && SPA3D_EPI_MUL_GELU_GRAD == EPI_MUL_GELU_GRAD, "epilogue ids");

// spa3d_op_gemm: the descriptor as given, planned by plan_gemm (fp32: the generic kernel), launched on that kernel
template <typename T>
int op_gemm(OpCtx& c, const spa3d_gemm_args& a, int impl, int32_t* kernel_out) {
  GemmDesc d{};
  d.A = a.A; d.B = a.B; d.C = a.C; d.M = a.M; d.N = a.N; d.K = a.K; d.sAm = a.sAm; d.sAk = a.sAk; d.sBk = a.sBk; d.sBn = a.sBn; d.sCm = a.sCm;
  d.nb1 = a.nb1; d.nb2 = a.nb2; d.bA1 = a.bA1; d.bA2 = a.bA2; d.bB1 = a.bB1; d.bB2 = a.bB2; d.bC1 = a.bC1; d.bC2 = a.bC2;
  d.alpha = a.alpha; d.bias = a.bias; d.epi = a.epi; d.aux = a.aux; d.aux_is_residual = a.aux_is_residual; d.out_f32 = a.out_f32; d.accumulate = a.accumulate;
  d.pre_out = a.pre_out; d.crow_group = a.crow_group; d.crow_skip = a.crow_skip; d.brow_group = a.brow_group; d.brow_skip = a.brow_skip;
  d.seg_n = a.seg_n; d.C_seg[0] = a.C_seg[0]; d.C_seg[1] = a.C_seg[1]; d.colsum_out = a.colsum_out;
  d.A2 = a.A2; d.sA2m = a.sA2m; d.K1 = a.K1; d.arow_idx = a.arow_idx; d.crow_idx = a.crow_idx; d.r1_x = a.r1_x; d.r1_w = a.r1_w; d.Bt = a.Bt; d.ldBt = a.ldBt;
  const bool unbatched = d.nb1 == 1 && d.nb2 == 1;
  GemmKernel k = GemmKernel::Generic;
  void* zp = nullptr; T* own_bt = nullptr;   // workspace slots: carved and planned with first, written (zeroed, transposed into) once nothing is refused
  if constexpr (sizeof(T) == 2) {
    const GemmPolicy p = GemmPolicy::from_impl(impl);
    if (d.sAm == 1 && d.sBn == 1 && d.out_f32 && d.accumulate) {  // the dW form: the tiled kernels read rows past the reduction from a page of zeros
      zp = c.alloc<char>(256); d.zero_page = zp;
      if (c.ar.overflow) return SPA3D_ERR_WORKSPACE;
    }
    // the tiled NT kernels read B as [N][K]: a dense [K][N] B is transposed into the workspace when one of them takes the GEMM with such a copy (A stands
    // in for the copy while asking: 16-byte aligned, as every workspace slot is)
    if (!d.Bt && d.sBk != 1 && d.sBn == 1 && d.sBk == d.N && d.sAk == 1 && unbatched) {
      d.Bt = d.A; d.ldBt = d.K;
      if (plan_nt(d, p) != GemmKernel::Refuse) {
        own_bt = c.alloc<T>((int64_t)d.K * d.N); d.Bt = own_bt;
        if (c.ar.overflow) return SPA3D_ERR_WORKSPACE;
      } else { d.Bt = nullptr; d.ldBt = 0; }
    }
    k = plan_gemm(d, p);
    if (k == GemmKernel::Generic && impl >= 2) k = GemmKernel::Refuse;   // tiled or an error, as spa3d_op_linear
  }
  if (kernel_out) *kernel_out = (int32_t)k;
  if (k == GemmKernel::Refuse) return SPA3D_ERR_ARG;
  // what the generic kernel does not implement, and the column sums where the entry cannot add them
  const bool entry_colsum = d.colsum_out && !gemm_tn_fuses_colsum(k, d);
  if ((k == GemmKernel::Generic && (d.seg_n > 0 || gemm_emb(d))) || (entry_colsum && (sizeof(T) == 4 || d.sBn != 1 || !unbatched))) {
    if (kernel_out) *kernel_out = (int32_t)GemmKernel::Refuse;
    return SPA3D_ERR_ARG;
  }
  if (zp) k_zero(&c, zp, 256);
  if (own_bt) k_transpose<T>(&c, (const T*)d.B, d.K, d.N, own_bt);
  gemm_launch<T>(&c, d, k);
  if (entry_colsum) k_colsum<T>(&c, (const T*)d.B, d.K, d.N, d.sBk, d.colsum_out, d.brow_group, d.brow_skip);
  return c.status();
}

// the device copy of nseq + 1 host offsets at the front of the workspace, then `body` (which reads *dev) once dry for its peak and once for real
template <typename F> static int op_with_offsets(OpCtx& c, const int32_t* host, int64_t nseq, const int32_t** dev, F&& body) {
  int32_t* d = c.alloc<int32_t>(nseq + 1);
  if (c.ar.overflow) return SPA3D_ERR_WORKSPACE;
  *dev = d;
  const int64_t used = c.ar.off;
  if (used + arena_peak(&c, body) + 256 > c.ar.cap) return SPA3D_ERR_WORKSPACE;
  k_set_i32(&c, d, host, nseq + 1);
  body();
  return c.status();
}

// the attention entry points' descriptor (attn_plan.hpp): the operands every form shares; a form adds its layout, the backward its gradients
AttnDesc op_attn_desc(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv, const float* sq, const float* sk, const float* km,
                      int64_t nseq, int Sq, int Sk, int H, int Dh, const void* o, const float* lse, int32_t dtype) {
  AttnDesc a;
  a.q = q; a.k = k; a.v = v; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.sq = sq; a.sk = sk; a.km = km; a.o = const_cast<void*>(o); a.lse = const_cast<float*>(lse);
  a.nseq = nseq; a.Sq = Sq; a.Sk = Sk; a.H = H; a.Dh = Dh; a.esz = dtype == SPA3D_F32 ? 4 : 2;
  return a;
}
void op_attn_grads(AttnDesc& a, const void* d_o, void* dq, void* dk, void* dv, float* dsq, float* dsk) {
  a.d_o = d_o; a.dq = dq; a.dk = dk; a.dv = dv; a.dsq = dsq; a.dsk = dsk;
}
}  // namespace
}  // namespace SPA_NS

// An entry point with a `dtype` argument is compiled twice: as declared in include/spa3d.h (this build's 16-bit type is bf16) and, with -DSPA_F16=1,
// under a hidden `_f16` suffix with fp16 as the 16-bit type; the public function forwards dtype == SPA3D_F16 there (FWD16, its first statement).
// SPA3D_OP(name)(parameters) { ... } defines this build's one of the two.  The twin's type is the header's declaration of `name`, and the names have C
// linkage, so a parameter list that differs from the header does not compile in either build.
#define SPA3D_TWIN(name) __attribute__((visibility("hidden"))) decltype(name) name##_f16
#if SPA_F16
#define SPA3D_OP(name) SPA3D_TWIN(name); int name##_f16
#define FWD16(name, ...)
#define OP_DT16 SPA3D_F16
#else
#define SPA3D_OP(name) SPA3D_TWIN(name); int name
#define FWD16(name, ...) if (dtype == SPA3D_F16) return name##_f16(__VA_ARGS__);
#define OP_DT16 SPA3D_BF16
#endif
#define OP_DTYPE_OK(dtype) ((dtype) == SPA3D_F32 || (dtype) == OP_DT16)
// `body` with T the storage type of `dtype`: float for SPA3D_F32, this build's 16-bit type for every other value
#define OP_BY_DTYPE(dtype, body)                                            \
  do {                                                                      \
    if ((dtype) == SPA3D_F32) { using T = float; body; }                    \
    else { using T = bf16_t; body; }                                        \
  } while (0)
static bool op_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
static int op_nv(int32_t dtype) { return dtype == SPA3D_F32 ? 4 : 8; }   // elements per 16 bytes (VecOf<T>::N)

extern "C" {

SPA3D_OP(spa3d_op_sin_embed)(const float* x, int64_t rows, int32_t C, int32_t nf, void* out, int32_t dtype, void* stream) {
  FWD16(spa3d_op_sin_embed, x, rows, C, nf, out, dtype, stream)
  if (!x || !out || nf <= 0 || nf > 64) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_sin_embed<T>(&c, x, rows, C, nf, 1.0f, (T*)out));
  return c.status();
}

SPA3D_OP(spa3d_op_linear)(const void* A, const void* B, const float* bias, const void* residual, void* C, int64_t M, int32_t N, int32_t K,
                          int32_t act, int32_t dtype, int32_t impl, void* ws, int64_t ws_bytes, void* stream) {
  FWD16(spa3d_op_linear, A, B, bias, residual, C, M, N, K, act, dtype, impl, ws, ws_bytes, stream)
  if (!A || !B || !C) return SPA3D_ERR_ARG;
  OpCtx c(stream, ws, ws_bytes);
  OP_BY_DTYPE(dtype, return op_linear<T>(c, (const T*)A, (const T*)B, bias, (const T*)residual, (T*)C, M, N, K, act, impl));
}
SPA3D_OP(spa3d_op_linear_bwd)(const void* A, const void* B, const void* dC, void* dA, float* dB, float* dbias, int64_t M, int32_t N, int32_t K,
                              int32_t dtype, int32_t impl, void* ws, int64_t ws_bytes, void* stream) {
  FWD16(spa3d_op_linear_bwd, A, B, dC, dA, dB, dbias, M, N, K, dtype, impl, ws, ws_bytes, stream)
  if (!A || !B || !dC) return SPA3D_ERR_ARG;
  OpCtx c(stream, ws, ws_bytes);
  OP_BY_DTYPE(dtype, return op_linear_bwd<T>(c, (const T*)A, (const T*)B, (const T*)dC, (T*)dA, dB, dbias, M, N, K, impl));
}

SPA3D_OP(spa3d_op_gemm)(const spa3d_gemm_args* g, int32_t dtype, int32_t impl, int32_t* kernel_out, void* ws, int64_t ws_bytes, void* stream) {
  FWD16(spa3d_op_gemm, g, dtype, impl, kernel_out, ws, ws_bytes, stream)
  if (kernel_out) *kernel_out = SPA3D_GEMM_REFUSE;
  if (!g || !g->A || !g->B || !g->C || !OP_DTYPE_OK(dtype) || g->M < 1 || g->N < 1 || g->K < 1 || g->nb1 < 1 || g->nb2 < 1) return SPA3D_ERR_ARG;
  if (g->epi < SPA3D_EPI_NONE || g->epi > SPA3D_EPI_MUL_GELU_GRAD || (g->epi == SPA3D_EPI_MUL_GELU_GRAD && !g->aux)) return SPA3D_ERR_ARG;
  if (g->crow_group < 0 || g->crow_skip < 0 || g->brow_group < 0 || g->brow_skip < 0 || g->seg_n < 0 || g->K1 < 0) return SPA3D_ERR_ARG;
  if (g->seg_n > 0 && (g->N % g->seg_n || g->N / g->seg_n > 3 || (g->N / g->seg_n > 1 && !g->C_seg[0]) || (g->N / g->seg_n > 2 && !g->C_seg[1]))) return SPA3D_ERR_ARG;
  if ((g->A2 && (g->K1 < 1 || g->K1 >= g->K)) || (g->r1_x && !g->r1_w)) return SPA3D_ERR_ARG;
  if (dtype == SPA3D_F32 && (g->seg_n > 0 || g->colsum_out || g->A2 || g->arow_idx || g->crow_idx || g->r1_x)) return SPA3D_ERR_ARG;
  OpCtx c(stream, ws, ws_bytes);
  OP_BY_DTYPE(dtype, return op_gemm<T>(c, *g, impl, kernel_out));
}

SPA3D_OP(spa3d_op_mlp_fused)(const void* na, const void* a, const void* w_in, const float* b_in, const void* w_out, const float* b_out, void* y,
                             void* h, void* hpre, int64_t M, int32_t d, int32_t mlp, int32_t dtype, void* ws, int64_t ws_bytes, void* stream) {
  FWD16(spa3d_op_mlp_fused, na, a, w_in, b_in, w_out, b_out, y, h, hpre, M, d, mlp, dtype, ws, ws_bytes, stream)
  if (!na || !a || !w_in || !b_in || !w_out || !b_out || !y || !h || !hpre || dtype == SPA3D_F32) return SPA3D_ERR_ARG;
  if (d != 384 || mlp != 1536 || M < 1) return SPA3D_ERR_ARG;   // shape first: a wrong shape is an argument error whatever the workspace
  for (const void* p : {na, a, (const void*)y, (const void*)h, (const void*)hpre, w_in, w_out})
    if (!op_al16(p)) return SPA3D_ERR_ARG;                       // 16-byte vector / LDS-DMA accesses on every operand
  OpCtx c(stream, ws, ws_bytes);
  bf16_t* wpk = c.alloc<bf16_t>(mlp_fused_pack_elems());
  if (c.ar.overflow) return SPA3D_ERR_WORKSPACE;
  mlp_fused_pack<bf16_t>(&c, (const bf16_t*)w_in, (const bf16_t*)w_out, wpk);
  if (plan_mlp(GemmPolicy(), M, d, mlp, wpk, b_in, b_out, na, a, y, h, hpre) != GemmKernel::MlpFused) return SPA3D_ERR_ARG;
  mlp_fused_fwd(&c, (const bf16_t*)na, (const bf16_t*)a, (bf16_t*)y, (bf16_t*)h, (bf16_t*)hpre, M, wpk, b_in, b_out);
  return c.status();
}

SPA3D_OP(spa3d_op_qkv_attention)(const void* nq, int64_t ldn, const void* wq, const void* wk, const void* wv, const float* scale_q, const float* scale_k,
                                 const float* keymask, const int32_t* seq_off, int64_t nseq, int32_t S, int32_t H, void* qkv, void* o, float* lse,
                                 int32_t dtype, void* ws, int64_t ws_bytes, void* stream) {
  FWD16(spa3d_op_qkv_attention, nq, ldn, wq, wk, wv, scale_q, scale_k, keymask, seq_off, nseq, S, H, qkv, o, lse, dtype, ws, ws_bytes, stream)
  if (!nq || !wq || !wk || !wv || !scale_q || !scale_k || !qkv || !o || dtype == SPA3D_F32 || H < 1 || H > 64) return SPA3D_ERR_ARG;
  OpCtx c(stream, ws, ws_bytes);
  bf16_t* wpk = c.alloc<bf16_t>(qkv_attn_pack_elems(H));
  if (c.ar.overflow) return SPA3D_ERR_WORKSPACE;
  qkv_attn_pack<bf16_t>(&c, (const bf16_t*)wq, (const bf16_t*)wk, (const bf16_t*)wv, H * ATTN_DH, H, wpk);
  const int E = H * ATTN_DH;
  AttnDesc a = op_attn_desc(qkv, (const bf16_t*)qkv + E, (const bf16_t*)qkv + 2 * E, 3 * E, 3 * E, 3 * E, scale_q, scale_k, keymask, nseq, S, S, H, ATTN_DH, o, lse, dtype);
  if (seq_off) { a.layout = AttnLayout::RaggedRows; a.seq_off = seq_off; }
  a.x = nq; a.ldx = ldn; a.d = QKVA_D; a.qkv_pk = wpk;
  const AttnPlan pl = plan_qkv_attn(a, AttnPolicy::from_impl(6));
  if (pl.kernel != AttnKernel::QkvFwd) return SPA3D_ERR_ARG;
  attn_launch(&c, a, pl);
  return c.status();
}

SPA3D_OP(spa3d_op_layernorm)(const void* x, const float* scale, void* y, float* stats, int64_t rows, int32_t d, int32_t dtype, void* stream) {
  FWD16(spa3d_op_layernorm, x, scale, y, stats, rows, d, dtype, stream)
  if (!x || !scale || !y || d <= 0 || d > 2048) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_layernorm<T>(&c, (const T*)x, scale, (T*)y, stats, rows, d));
  return c.status();
}
SPA3D_OP(spa3d_op_layernorm_bwd)(const void* x, const float* scale, const float* stats, const void* dy, void* dx, float* dscale, int64_t rows,
                                 int32_t d, int32_t dtype, void* stream) {
  FWD16(spa3d_op_layernorm_bwd, x, scale, stats, dy, dx, dscale, rows, d, dtype, stream)
  if (!x || !scale || !stats || !dy || !dx || !dscale || d <= 0 || d > 2048) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_layernorm_bwd<T>(&c, (const T*)x, scale, stats, (const T*)dy, (T*)dx, dscale, rows, d, nullptr));
  return c.status();
}

SPA3D_OP(spa3d_op_attention)(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv, const float* scale_q,
                             const float* scale_k, const float* keymask, int64_t nseq, int32_t Sq, int32_t Sk, int32_t H, int32_t Dh, void* o,
                             float* lse, int32_t dtype, int32_t impl, void* ws, int64_t ws_bytes, void* stream) {
  FWD16(spa3d_op_attention, q, k, v, ldq, ldk, ldv, scale_q, scale_k, keymask, nseq, Sq, Sk, H, Dh, o, lse, dtype, impl, ws, ws_bytes, stream)
  if (!q || !k || !v || !o || !scale_q || !scale_k || Dh > 128) return SPA3D_ERR_ARG;
  OpCtx c(stream, ws, ws_bytes);
  c.attn = AttnPolicy::from_impl(impl);
  const AttnDesc a = op_attn_desc(q, k, v, ldq, ldk, ldv, scale_q, scale_k, keymask, nseq, Sq, Sk, H, Dh, o, lse, dtype);
  OP_BY_DTYPE(dtype, attention_fwd<T>(&c, a));
  return c.status();
}
SPA3D_OP(spa3d_op_attention_holdout)(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv, const float* scale_q,
                                     const float* scale_k, int64_t nseq, int32_t Sq, int32_t Nk, int32_t H, int32_t Dh, const int32_t* holes, void* o,
                                     float* lse, int32_t dtype, int32_t impl, void* ws, int64_t ws_bytes, void* stream) {
  FWD16(spa3d_op_attention_holdout, q, k, v, ldq, ldk, ldv, scale_q, scale_k, nseq, Sq, Nk, H, Dh, holes, o, lse, dtype, impl, ws, ws_bytes, stream)
  if (!q || !k || !v || !o || !scale_q || !scale_k || !holes || Dh < 1 || Dh > 128 || nseq < 1 || nseq > (1 << 20) || Sq < 1 || Nk < 1 || H < 1) return SPA3D_ERR_ARG;
  for (int64_t i = 0; i < nseq; ++i) {  // a hole outside [0, Nk], lo > hi, a sequence left without a key
    const int64_t lo = holes[2 * i], hi = holes[2 * i + 1];
    if (lo < 0 || hi > Nk || lo > hi || hi - lo >= Nk) return SPA3D_ERR_ARG;
  }
  OpCtx c(stream, ws, ws_bytes);
  c.attn = AttnPolicy::from_impl(impl);
  int32_t* hd = c.alloc<int32_t>(2 * nseq);
  if (c.ar.overflow) return SPA3D_ERR_WORKSPACE;
  k_set_i32(&c, hd, holes, 2 * nseq);
  AttnDesc a = op_attn_desc(q, k, v, ldq, ldk, ldv, scale_q, scale_k, nullptr, nseq, Sq, 0, H, Dh, o, lse, dtype);
  a.layout = AttnLayout::Hole; a.holes_host = holes; a.holes_dev = hd; a.Nk = Nk;
  OP_BY_DTYPE(dtype, attention_fwd<T>(&c, a));
  return c.status();
}
SPA3D_OP(spa3d_op_attention_bwd)(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv, const float* scale_q,
                                 const float* scale_k, const float* keymask, int64_t nseq, int32_t Sq, int32_t Sk, int32_t H, int32_t Dh,
                                 const void* o, const float* lse, const void* d_o, void* dq, void* dk, void* dv, float* dscale_q,
                                 float* dscale_k, int32_t dtype, int32_t impl, void* ws, int64_t ws_bytes, void* stream) {
  FWD16(spa3d_op_attention_bwd, q, k, v, ldq, ldk, ldv, scale_q, scale_k, keymask, nseq, Sq, Sk, H, Dh, o, lse, d_o, dq, dk, dv, dscale_q, dscale_k, dtype,
        impl, ws, ws_bytes, stream)
  if (!q || !k || !v || !d_o || !dq || !dk || !dv || !dscale_q || !dscale_k || Dh > 128) return SPA3D_ERR_ARG;
  OpCtx c(stream, ws, ws_bytes);
  c.attn = AttnPolicy::from_impl(impl);
  AttnDesc a = op_attn_desc(q, k, v, ldq, ldk, ldv, scale_q, scale_k, keymask, nseq, Sq, Sk, H, Dh, o, lse, dtype);
  op_attn_grads(a, d_o, dq, dk, dv, dscale_q, dscale_k);
  OP_BY_DTYPE(dtype, attention_bwd<T>(&c, a));
  return c.status();
}

// ---- The two ragged forms of the fused attention on their own (tests/test_gpu_attn_ragged.py).  Offsets are HOST arrays: checked first, then copied into the
// workspace (k_set_i32).  Whatever a launcher would record as a HIP-class error ("ragged sequences need the fused attention kernels", a shape the fused
// kernels decline under impl 2) is an argument error here and launches nothing; the workspace is sized by a dry walk before the first launch.
static bool ragged_args_ok(const void* const* ptrs, int np, const int32_t* seq_off, int64_t nseq, int64_t ldq, int64_t ldk, int64_t ldv, int32_t S, int32_t H,
                           int32_t Dh, int32_t dtype, int32_t impl) {
  if (!seq_off || dtype != OP_DT16 || Dh != ATTN_DH || S < 2 || S > ATTN_MAX_S || H < 1 || nseq < 1 || nseq > (1 << 20) || nseq * H > 0x7fffffffLL) return false;
  if (impl != 0 && impl != 2 && impl != 3 && impl != 4) return false;   // 1: no generic route for ragged rows; anything else names no kernel
  const int64_t E = (int64_t)H * Dh;   // a row stride below the row: rows of dq / dk / dv would overlap
  if (ldq < E || ldk < E || ldv < E || ldq % 8 || ldk % 8 || ldv % 8) return false;
  for (int i = 0; i < np; ++i)
    if (!ptrs[i] || !op_al16(ptrs[i])) return false;   // 16-byte vector accesses on every operand
  if (seq_off[0] < 0) return false;
  for (int64_t i = 0; i < nseq; ++i) {  // a length outside [1, S]: an empty or decreasing pair, a sequence longer than the instance (a sum past 2^31 wraps negative)
    const int64_t n = (int64_t)seq_off[i + 1] - seq_off[i];
    if (n < 1 || n > S) return false;
  }
  return true;
}
static bool varlen_args_ok(const int32_t* koff, int64_t nseq, int64_t ldq, int64_t ldk, int64_t ldv, int32_t Sq, int32_t H, int32_t Dh, int32_t dtype, int32_t impl) {
  if (!koff || !OP_DTYPE_OK(dtype) || nseq < 1 || nseq > (1 << 20) || Sq < 1 || H < 1 || Dh < 1 || Dh > 128 || impl < 0 || impl > 2) return false;
  if (ldq < (int64_t)H * Dh || ldk < (int64_t)H * Dh || ldv < (int64_t)H * Dh) return false;
  if (impl == 2 && (Dh != ATTN_DH || Sq > ATTN_XCHUNK || dtype == SPA3D_F32 || ldq % 8 || ldk % 8 || ldv % 8)) return false;   // what the chunked-key kernels take
  if (koff[0] != 0) return false;
  for (int64_t i = 0; i < nseq; ++i)
    if ((int64_t)koff[i + 1] - koff[i] < 1) return false;   // a sequence without a key
  return true;
}
SPA3D_OP(spa3d_op_attention_ragged)(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv, const float* scale_q,
                                    const float* scale_k, const float* keymask, const int32_t* seq_off, int64_t nseq, int32_t S, int32_t H, int32_t Dh,
                                    void* o, float* lse, int32_t dtype, int32_t impl, void* ws, int64_t ws_bytes, void* stream) {
  FWD16(spa3d_op_attention_ragged, q, k, v, ldq, ldk, ldv, scale_q, scale_k, keymask, seq_off, nseq, S, H, Dh, o, lse, dtype, impl, ws, ws_bytes, stream)
  const void* ptrs[] = {q, k, v, o, scale_q, scale_k};
  if (!ragged_args_ok(ptrs, 6, seq_off, nseq, ldq, ldk, ldv, S, H, Dh, dtype, impl)) return SPA3D_ERR_ARG;
  OpCtx c(stream, ws, ws_bytes);
  c.attn = AttnPolicy::from_impl(impl);
  AttnDesc a = op_attn_desc(q, k, v, ldq, ldk, ldv, scale_q, scale_k, keymask, nseq, S, S, H, Dh, o, lse, dtype);
  a.layout = AttnLayout::RaggedRows; a.total_rows = seq_off[nseq];
  return op_with_offsets(c, seq_off, nseq, &a.seq_off, [&] { attention_fwd<bf16_t>(&c, a); });
}
SPA3D_OP(spa3d_op_attention_ragged_bwd)(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv, const float* scale_q,
                                        const float* scale_k, const float* keymask, const int32_t* seq_off, int64_t nseq, int32_t S, int32_t H, int32_t Dh,
                                        const void* o, const float* lse, const void* d_o, void* dq, void* dk, void* dv, float* dscale_q, float* dscale_k,
                                        int32_t dtype, int32_t impl, void* ws, int64_t ws_bytes, void* stream) {
  FWD16(spa3d_op_attention_ragged_bwd, q, k, v, ldq, ldk, ldv, scale_q, scale_k, keymask, seq_off, nseq, S, H, Dh, o, lse, d_o, dq, dk, dv, dscale_q, dscale_k,
        dtype, impl, ws, ws_bytes, stream)
  const void* ptrs[] = {q, k, v, o, d_o, dq, dk, dv, scale_q, scale_k};
  if (!lse || !dscale_q || !dscale_k || !ragged_args_ok(ptrs, 10, seq_off, nseq, ldq, ldk, ldv, S, H, Dh, dtype, impl)) return SPA3D_ERR_ARG;
  OpCtx c(stream, ws, ws_bytes);
  c.attn = AttnPolicy::from_impl(impl);
  AttnDesc a = op_attn_desc(q, k, v, ldq, ldk, ldv, scale_q, scale_k, keymask, nseq, S, S, H, Dh, o, lse, dtype);
  a.layout = AttnLayout::RaggedRows; a.total_rows = seq_off[nseq];
  op_attn_grads(a, d_o, dq, dk, dv, dscale_q, dscale_k);
  return op_with_offsets(c, seq_off, nseq, &a.seq_off, [&] { attention_bwd<bf16_t>(&c, a); });
}

SPA3D_OP(spa3d_op_attention_varlen)(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv, const float* scale_q,
                                    const float* scale_k, const int32_t* koff, int64_t nseq, int32_t Sq, int32_t H, int32_t Dh, void* o, float* lse,
                                    int32_t dtype, int32_t impl, void* ws, int64_t ws_bytes, void* stream) {
  FWD16(spa3d_op_attention_varlen, q, k, v, ldq, ldk, ldv, scale_q, scale_k, koff, nseq, Sq, H, Dh, o, lse, dtype, impl, ws, ws_bytes, stream)
  if (!q || !k || !v || !o || !scale_q || !scale_k || !varlen_args_ok(koff, nseq, ldq, ldk, ldv, Sq, H, Dh, dtype, impl)) return SPA3D_ERR_ARG;
  if (impl == 2 && !(op_al16(q) && op_al16(k) && op_al16(v) && op_al16(o))) return SPA3D_ERR_ARG;
  OpCtx c(stream, ws, ws_bytes);
  c.attn = AttnPolicy::from_impl(impl);
  AttnDesc a = op_attn_desc(q, k, v, ldq, ldk, ldv, scale_q, scale_k, nullptr, nseq, Sq, 0, H, Dh, o, lse, dtype);
  a.layout = AttnLayout::RaggedKeys; a.koff_host = koff;
  OP_BY_DTYPE(dtype, return op_with_offsets(c, koff, nseq, &a.koff_dev, [&] { attention_fwd<T>(&c, a); }));
}
SPA3D_OP(spa3d_op_attention_varlen_bwd)(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv, const float* scale_q,
                                        const float* scale_k, const int32_t* koff, int64_t nseq, int32_t Sq, int32_t H, int32_t Dh, const void* o,
                                        const float* lse, const void* d_o, void* dq, void* dk, void* dv, float* dscale_q, float* dscale_k, int32_t dtype,
                                        int32_t impl, void* ws, int64_t ws_bytes, void* stream) {
  FWD16(spa3d_op_attention_varlen_bwd, q, k, v, ldq, ldk, ldv, scale_q, scale_k, koff, nseq, Sq, H, Dh, o, lse, d_o, dq, dk, dv, dscale_q, dscale_k, dtype, impl,
        ws, ws_bytes, stream)
  if (!q || !k || !v || !d_o || !dq || !dk || !dv || !scale_q || !scale_k || !dscale_q || !dscale_k || !varlen_args_ok(koff, nseq, ldq, ldk, ldv, Sq, H, Dh, dtype, impl))
    return SPA3D_ERR_ARG;
  // 16-bit, impl 0 / 2: the fused backward rebuilds P from the forward's o and lse, and a sequence the single launch declines is tried on the fused kernels
  // again -- a missing one of the two is refused here, not discovered there.  fp32 and impl 1 (the generic composition) read neither.
  if (dtype != SPA3D_F32 && impl != 1 && (!o || !lse)) return SPA3D_ERR_ARG;
  if (impl == 2) {
    for (const void* p : {q, k, v, o, d_o, (const void*)dq, (const void*)dk, (const void*)dv, (const void*)scale_q, (const void*)scale_k})
      if (!op_al16(p)) return SPA3D_ERR_ARG;
  }
  OpCtx c(stream, ws, ws_bytes);
  c.attn = AttnPolicy::from_impl(impl);
  AttnDesc a = op_attn_desc(q, k, v, ldq, ldk, ldv, scale_q, scale_k, nullptr, nseq, Sq, 0, H, Dh, o, lse, dtype);
  a.layout = AttnLayout::RaggedKeys; a.koff_host = koff;
  op_attn_grads(a, d_o, dq, dk, dv, dscale_q, dscale_k);
  OP_BY_DTYPE(dtype, return op_with_offsets(c, koff, nseq, &a.koff_dev, [&] { attention_bwd<T>(&c, a); }));
}

// Single-query attention and the rank-K projection: every shape their launchers would record as a HIP-class error (or decline) is an argument error here
static bool q1_shape_ok(int64_t nseq, int32_t S, int32_t H, int32_t Dh) {
  const bool width = Dh == 8 || Dh == 16 || Dh == 32 || Dh == 64 || Dh == 96 || Dh == 128;   // the instantiations of csrc/attn_q1.hip
  return width && S >= 1 && S <= 320 && H >= 1 && nseq >= 0;
}
SPA3D_OP(spa3d_op_attention_q1)(const void* q0, int64_t ldq0, const void* k, const void* v, int64_t ldk, int64_t ldv, const float* scale_q,
                                const float* scale_k, const float* keymask, const int32_t* seq_off, int64_t nseq, int32_t S, int32_t H, int32_t Dh,
                                void* o0, float* p0, int32_t dtype, void* stream) {
  FWD16(spa3d_op_attention_q1, q0, ldq0, k, v, ldk, ldv, scale_q, scale_k, keymask, seq_off, nseq, S, H, Dh, o0, p0, dtype, stream)
  if (!q0 || !k || !v || !scale_q || !scale_k || !o0 || !p0 || !q1_shape_ok(nseq, S, H, Dh)) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_attn_q1_fwd<T>(&c, (const T*)q0, ldq0, (const T*)k, (const T*)v, ldk, ldv, scale_q, scale_k, keymask, nseq, S, H, Dh, (T*)o0, p0, seq_off));
  return c.hip_err == -3 ? SPA3D_ERR_ARG : c.status();
}
SPA3D_OP(spa3d_op_attention_q1_bwd)(const void* q0, int64_t ldq0, const void* k, const void* v, int64_t ldk, int64_t ldv, const float* scale_q,
                                    const float* scale_k, const float* keymask, const int32_t* seq_off, int64_t nseq, int32_t S, int32_t H, int32_t Dh,
                                    const float* p0, const void* d_o0, void* dq0, void* dk, void* dv, float* dscale_q, float* dscale_k, int32_t dtype,
                                    void* stream) {
  FWD16(spa3d_op_attention_q1_bwd, q0, ldq0, k, v, ldk, ldv, scale_q, scale_k, keymask, seq_off, nseq, S, H, Dh, p0, d_o0, dq0, dk, dv, dscale_q, dscale_k,
        dtype, stream)
  if (!q0 || !k || !v || !scale_q || !scale_k || !p0 || !d_o0 || !dq0 || !dk || !dv || !dscale_q || !dscale_k || !q1_shape_ok(nseq, S, H, Dh))
    return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);   // c.det stays null: float atomics
  OP_BY_DTYPE(dtype, k_attn_q1_bwd<T>(&c, (const T*)q0, ldq0, (const T*)k, (const T*)v, ldk, ldv, scale_q, scale_k, keymask, nseq, S, H, Dh, p0, (const T*)d_o0,
                                      (T*)dq0, (T*)dk, (T*)dv, dscale_q, dscale_k, seq_off));
  return c.hip_err == -3 ? SPA3D_ERR_ARG : c.status();
}

SPA3D_OP(spa3d_op_rank_linear)(const void* x, const void* w, const float* bias, void* out, int64_t M, int32_t N, int32_t K, int64_t ldo, int32_t rgroup,
                               int32_t rskip, int32_t dtype, void* stream) {
  FWD16(spa3d_op_rank_linear, x, w, bias, out, M, N, K, ldo, rgroup, rskip, dtype, stream)
  if (!x || !w || !out || M < 0 || N < 8 || ldo < N || rgroup < 0 || rskip < 0 || dtype == SPA3D_F32) return SPA3D_ERR_ARG;   // (no float instantiation: embed.hip)
  OpCtx c(stream, nullptr, 0);
  // false: K outside 1..4, N % 8, N > 2048, ldo % 8, a misaligned out, M >= 2^31 (k_rank_fwd launches nothing then)
  const bool ok = k_rank_fwd<bf16_t>(&c, (const bf16_t*)x, (const bf16_t*)w, bias, (bf16_t*)out, M, N, K, ldo, rgroup, rskip);
  return ok ? c.status() : SPA3D_ERR_ARG;
}
SPA3D_OP(spa3d_op_rank_linear_bwd)(const void* x, const void* dy, int64_t M, int32_t N, int32_t K, int64_t ldy, int32_t rgroup, int32_t rskip, float* gw,
                                   float* gb, int32_t dtype, void* stream) {
  FWD16(spa3d_op_rank_linear_bwd, x, dy, M, N, K, ldy, rgroup, rskip, gw, gb, dtype, stream)
  if (!x || !dy || !gw || M < 0 || N < 8 || ldy < N || rgroup < 0 || rskip < 0 || dtype == SPA3D_F32) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  const bool ok = k_rank_bwd<bf16_t>(&c, (const bf16_t*)x, (const bf16_t*)dy, M, N, K, ldy, rgroup, rskip, gw, gb);
  return ok ? c.status() : SPA3D_ERR_ARG;
}

// ---- The row plumbing of csrc/rows.hip on its own (tests/test_gpu_rows.py).  Thin wrappers: every input a launcher would record as a HIP-class error
// (an empty grid, a row width that is not a multiple of 16 bytes) or mis-handle without a word (a 16-byte access through a pointer that is not 16-byte
// aligned, a negative count) is an argument error here and launches nothing.  c.det stays null: sums use float atomics.
SPA3D_OP(spa3d_op_colsum)(const void* x, int64_t rows, int32_t n, int64_t ld, int32_t rgroup, int32_t rskip, float* out, int32_t dtype, void* stream) {
  FWD16(spa3d_op_colsum, x, rows, n, ld, rgroup, rskip, out, dtype, stream)
  if (!x || !out || !OP_DTYPE_OK(dtype) || rows < 0 || n < 1 || ld < n || rgroup < 0 || rskip < 0) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_colsum<T>(&c, (const T*)x, rows, n, ld, out, rgroup, rskip));
  return c.status();
}

SPA3D_OP(spa3d_op_rows)(int32_t mode, const void* src, const int32_t* idx, int64_t stride_rows, void* dst, int64_t n, int32_t d, int32_t dtype, void* stream) {
  FWD16(spa3d_op_rows, mode, src, idx, stride_rows, dst, n, d, dtype, stream)
  if (!src || !dst || !OP_DTYPE_OK(dtype) || n < 0 || d < 1 || mode < SPA3D_ROWS_GATHER_STRIDED || mode > SPA3D_ROWS_ADD_STRIDED) return SPA3D_ERR_ARG;
  const bool by_idx = mode == SPA3D_ROWS_GATHER_IDX || mode == SPA3D_ROWS_SCATTER_IDX || mode == SPA3D_ROWS_SCATTER_ADD_IDX;
  if (by_idx && (!idx || d % op_nv(dtype) || !op_al16(src) || !op_al16(dst))) return SPA3D_ERR_ARG;   // 16-byte accesses: the launcher checks d only
  if (!by_idx && stride_rows < 1) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, {
    if (mode == SPA3D_ROWS_GATHER_STRIDED) k_gather_rows<T>(&c, (const T*)src, stride_rows, (T*)dst, n, d);
    else if (mode == SPA3D_ROWS_ADD_STRIDED) k_add_rows_strided<T>(&c, (T*)dst, (const T*)src, stride_rows, n, d);
    else k_rows_idx<T>(&c, mode - SPA3D_ROWS_GATHER_IDX, (const T*)src, idx, (T*)dst, n, d);
  });
  return c.status();
}

#if !SPA_F16   // the two plans have no storage type: one copy
int spa3d_op_prune_plan(const float* km, int64_t nseq, int32_t S, int32_t* cnt, int32_t* seq_off, int32_t* row_src, int64_t* kept, void* stream) {
  if (!km || !cnt || !seq_off || !row_src || !kept || nseq < 0 || S < 1 || nseq * (int64_t)S > 0x7fffffffLL) return SPA3D_ERR_ARG;   // row_src holds int32 rows
  OpCtx c(stream, nullptr, 0);
  *kept = k_prune_plan(&c, km, nseq, S, cnt, seq_off, row_src);
  return c.status();
}
int spa3d_op_share_plan(const int32_t* qframe, int64_t B, int32_t Q, int32_t* slot, int32_t* slot_b, int32_t* slot_f, int32_t* slot_q0, int32_t* scratch,
                        int64_t* nslot, void* stream) {
  if (!qframe || !slot || !slot_b || !slot_f || !slot_q0 || !scratch || !nslot || B < 0 || Q < 0 || B * (int64_t)Q > 0x7fffffffLL) return SPA3D_ERR_ARG;
  if (B == 0 || Q == 0) { *nslot = 0; return SPA3D_OK; }   // (k_share_plan would launch an empty grid)
  OpCtx c(stream, nullptr, 0);
  *nslot = k_share_plan(&c, qframe, B, Q, slot, slot_b, slot_f, slot_q0, scratch);
  return c.status();
}
#endif

SPA3D_OP(spa3d_op_share_rows)(int32_t which, const void* a, const void* b, const int32_t* slot, const int32_t* slot_b, const int32_t* slot_f,
                              const int32_t* slot_q0, int64_t nslot, int64_t B, int32_t Q, int32_t L, int32_t Cl, int32_t d, void* out, int32_t dtype, void* stream) {
  FWD16(spa3d_op_share_rows, which, a, b, slot, slot_b, slot_f, slot_q0, nslot, B, Q, L, Cl, d, out, dtype, stream)
  if (!a || !out || !OP_DTYPE_OK(dtype) || nslot < 0 || B < 0 || Q < 1 || L < 0 || d < 1 || which < SPA3D_SHARE_ASSEMBLE || which > SPA3D_SHARE_REDUCE)
    return SPA3D_ERR_ARG;
  const int nv = op_nv(dtype);
  if (d % nv || !op_al16(a) || !op_al16(out) || nslot > B * Q) return SPA3D_ERR_ARG;   // vector-only kernels
  const int64_t nseq = B * Q;
  OpCtx c(stream, nullptr, 0);
  if (which == SPA3D_SHARE_ASSEMBLE) {
    if (!b || !slot_b || !slot_f || Cl < 1 || Cl > d || Cl % nv || !op_al16(b)) return SPA3D_ERR_ARG;
    OP_BY_DTYPE(dtype, k_share_assemble<T>(&c, (const T*)a, (const T*)b, slot_b, slot_f, nslot, nseq, L, Cl, d, (T*)out));
  } else if (which == SPA3D_SHARE_EXPAND) {
    if (!slot || !slot_q0 || !op_al16(b)) return SPA3D_ERR_ARG;   // b = add, may be NULL
    OP_BY_DTYPE(dtype, k_share_expand<T>(&c, (const T*)a, slot, slot_q0, nslot, nseq, L + 1, d, (const T*)b, (T*)out));
  } else {
    if (!slot || !slot_b || Q > 12288) return SPA3D_ERR_ARG;         // the member list [Q] lives in LDS, as the plan's table
    OP_BY_DTYPE(dtype, k_share_reduce<T>(&c, (const T*)a, slot, slot_b, nslot, nseq, Q, L + 1, d, (T*)out));
  }
  return c.status();
}

SPA3D_OP(spa3d_op_assemble_readout)(const void* qtok, const void* lat, const int32_t* qframe, int64_t B, int32_t Q, int32_t L, int32_t Cl, int32_t D, void* seq,
                                    int32_t dtype, void* stream) {
  FWD16(spa3d_op_assemble_readout, qtok, lat, qframe, B, Q, L, Cl, D, seq, dtype, stream)
  if (!qtok || !lat || !qframe || !seq || !OP_DTYPE_OK(dtype) || B < 0 || Q < 1 || L < 0 || Cl < 1 || D < Cl) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_assemble_readout<T>(&c, (const T*)qtok, (const T*)lat, qframe, B, Q, L, Cl, D, (T*)seq));
  return c.status();
}
SPA3D_OP(spa3d_op_assemble_readout_bwd)(const void* dseq, const int32_t* qframe, int64_t B, int32_t Q, int32_t L, int32_t Cl, int32_t D, void* dqtok,
                                        float* dlat, int32_t accumulate, int32_t dtype, void* stream) {
  FWD16(spa3d_op_assemble_readout_bwd, dseq, qframe, B, Q, L, Cl, D, dqtok, dlat, accumulate, dtype, stream)
  if (!dseq || !qframe || !dqtok || !dlat || !OP_DTYPE_OK(dtype) || B < 0 || Q < 1 || L < 1 || Cl < 1 || D < Cl || (accumulate != 0 && accumulate != 1))
    return SPA3D_ERR_ARG;   // (L = 0: dlat is empty and its launch would have no workgroup)
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_assemble_readout_bwd<T>(&c, (const T*)dseq, qframe, B, Q, L, Cl, D, (T*)dqtok, dlat, accumulate != 0));
  return c.status();
}

SPA3D_OP(spa3d_op_broadcast_rows)(const float* src, int32_t rows, int32_t d, void* dst, int64_t B, int32_t dtype, void* stream) {
  FWD16(spa3d_op_broadcast_rows, src, rows, d, dst, B, dtype, stream)
  if (!src || !dst || !OP_DTYPE_OK(dtype) || rows < 1 || d < 1 || B < 0) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_broadcast_rows<T>(&c, src, rows, d, (T*)dst, B));
  return c.status();
}
SPA3D_OP(spa3d_op_bcast_grad)(const void* dsrc, int64_t per, int64_t B, int64_t bstride, float* dparam, int32_t dtype, void* stream) {
  FWD16(spa3d_op_bcast_grad, dsrc, per, B, bstride, dparam, dtype, stream)
  if (!dsrc || !dparam || !OP_DTYPE_OK(dtype) || per < 1 || per > 0x7fffffffLL || B < 0 || bstride < per) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_bcast_grad<T>(&c, (const T*)dsrc, per, B, bstride, dparam));
  return c.status();
}

SPA3D_OP(spa3d_op_vis_mean_pool)(const void* tok, const float* vis, int64_t nseq, int32_t T_, int32_t d, void* out, int32_t dtype, void* stream) {
  FWD16(spa3d_op_vis_mean_pool, tok, vis, nseq, T_, d, out, dtype, stream)
  if (!tok || !vis || !out || !OP_DTYPE_OK(dtype) || nseq < 0 || T_ < 1 || d < 1) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_vis_mean_pool<T>(&c, (const T*)tok, vis, nseq, T_, d, (T*)out));
  return c.status();
}
SPA3D_OP(spa3d_op_vis_mean_pool_bwd)(const void* dout, const float* vis, int64_t nseq, int32_t T_, int32_t d, void* dtok, int32_t dtype, void* stream) {
  FWD16(spa3d_op_vis_mean_pool_bwd, dout, vis, nseq, T_, d, dtok, dtype, stream)
  if (!dout || !vis || !dtok || !OP_DTYPE_OK(dtype) || nseq < 0 || T_ < 1 || d < 1) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_vis_mean_pool_bwd<T>(&c, (const T*)dout, vis, nseq, T_, d, (T*)dtok));
  return c.status();
}

// ---- The first mile of the model on its own (tests/test_gpu_embed.py): the embeddings, row maps, readout rows, key masks and weight shadows of csrc/embed.hip
// and the latent quantiser of csrc/loss.hip.  Same rules as the row plumbing above.  SinScales holds 64 entries and is indexed by the feature number: a width
// above 64 would read past the by-value kernel argument, so nf is checked here (spa3d_create checks num_frequencies; the launchers trust their caller).
static bool embed_nf_ok(int32_t nf) { return nf >= 1 && nf <= 64; }
static bool embed_scale_ok(float s) { return s != 0.f && s == s; }
static const int32_t kTileRowsMax = 65535 * 32;   // pack / transpose put the row tiles on gridDim.y

SPA3D_OP(spa3d_op_sin_embed_scaled)(const float* x, int64_t rows, int32_t C, int32_t nf, float prescale, void* out, int32_t dtype, void* stream) {
  FWD16(spa3d_op_sin_embed_scaled, x, rows, C, nf, prescale, out, dtype, stream)
  if (!x || !out || !OP_DTYPE_OK(dtype) || rows < 0 || C < 1 || C > 65536 || !embed_nf_ok(nf) || !embed_scale_ok(prescale)) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_sin_embed<T>(&c, x, rows, C, nf, prescale, (T*)out));
  return c.status();
}
SPA3D_OP(spa3d_op_embed_tokens)(const float* tracks, int64_t nrows, int32_t T_, int32_t NC, int32_t nf, float prescale, void* out, int32_t dtype, void* stream) {
  FWD16(spa3d_op_embed_tokens, tracks, nrows, T_, NC, nf, prescale, out, dtype, stream)
  if (!tracks || !out || !OP_DTYPE_OK(dtype) || nrows < 0 || T_ < 1 || (NC != 2 && NC != 3) || !embed_nf_ok(nf) || !embed_scale_ok(prescale)) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_embed_tokens<T>(&c, tracks, nrows, T_, nf, prescale, (T*)out, NC));
  return c.status();
}
SPA3D_OP(spa3d_op_embed_maps)(const int32_t* row_src, int64_t rows, int32_t S, int32_t T_, int32_t* arow, int32_t* crow, void* tok, const float* readout,
                              int32_t d, int32_t dtype, void* stream) {
  FWD16(spa3d_op_embed_maps, row_src, rows, S, T_, arow, crow, tok, readout, d, dtype, stream)
  if (!arow || !crow || !tok || !readout || !OP_DTYPE_OK(dtype) || rows < 0 || rows > 0x7fffffffLL || T_ < 1 || S != T_ + 1 || d < 1) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_embed_maps<T>(&c, row_src, rows, S, T_, arow, crow, (T*)tok, readout, d));
  return c.status();
}
SPA3D_OP(spa3d_op_set_readout_rows)(void* tok, const float* readout, int64_t nseq, int32_t S, int32_t d, int32_t dtype, void* stream) {
  FWD16(spa3d_op_set_readout_rows, tok, readout, nseq, S, d, dtype, stream)
  if (!tok || !readout || !OP_DTYPE_OK(dtype) || nseq < 0 || S < 1 || d < 1) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_set_readout_rows<T>(&c, (T*)tok, readout, nseq, S, d));
  return c.status();
}
SPA3D_OP(spa3d_op_pack)(const float* src, int64_t src_ld, int32_t rows, int32_t cols, void* dn, int64_t ldn, void* dt, int64_t ldt, int32_t dtype, void* stream) {
  FWD16(spa3d_op_pack, src, src_ld, rows, cols, dn, ldn, dt, ldt, dtype, stream)
  if (!src || (!dn && !dt) || !OP_DTYPE_OK(dtype) || rows < 0 || rows > kTileRowsMax || cols < 0 || src_ld < cols || (dn && ldn < cols) || (dt && ldt < rows))
    return SPA3D_ERR_ARG;
  if (rows == 0 || cols == 0) return SPA3D_OK;   // (k_pack would launch an empty grid)
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_pack<T>(&c, src, src_ld, rows, cols, (T*)dn, ldn, (T*)dt, ldt));
  return c.status();
}
SPA3D_OP(spa3d_op_transpose)(const void* src, int32_t rows, int32_t cols, void* dst, int32_t dtype, void* stream) {
  FWD16(spa3d_op_transpose, src, rows, cols, dst, dtype, stream)
  if (!src || !dst || !OP_DTYPE_OK(dtype) || rows < 0 || rows > kTileRowsMax || cols < 0) return SPA3D_ERR_ARG;
  if (rows == 0 || cols == 0) return SPA3D_OK;
  OpCtx c(stream, nullptr, 0);
  OP_BY_DTYPE(dtype, k_transpose<T>(&c, (const T*)src, rows, cols, (T*)dst));
  return c.status();
}

#if !SPA_F16   // fp32 and int32 tensors only: one copy
int spa3d_op_query_embed(const float* qp, int64_t nq, int32_t NC, int32_t nf, float track_scale, float time_scale, float* feat, int32_t* qframe, void* stream) {
  if (!qp || !feat || !qframe || nq < 0 || (NC != 2 && NC != 3) || !embed_nf_ok(nf) || !embed_scale_ok(track_scale) || !embed_scale_ok(time_scale)) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  k_query_embed1(&c, qp, nq, nf, track_scale, time_scale, feat, qframe, NC);
  return c.status();
}
int spa3d_op_keymask(const float* visible, const int32_t* boundary, int64_t nseq, int32_t N, int32_t T_, int32_t with_readout, float* km, void* stream) {
  if (!visible || !boundary || !km || nseq < 0 || N < 1 || nseq % N || T_ < 1 || (with_readout != 0 && with_readout != 1)) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  if (with_readout) k_keymask(&c, visible, boundary, nseq, N, T_, km);
  else k_keymask2d(&c, visible, boundary, nseq, N, T_, km);
  return c.status();
}
int spa3d_op_sum3(const float* a, const float* b, const float* c3, float* out, int32_t n, void* stream) {
  if (!out || (!a && !b && !c3) || n < 0) return SPA3D_ERR_ARG;
  if (n == 0) return SPA3D_OK;   // (k_sum3 would launch an empty grid)
  OpCtx c(stream, nullptr, 0);
  k_sum3(&c, a, b, c3, out, n);
  return c.status();
}
int spa3d_op_discretize(const float* lat, const float* noise, int32_t discretize, float* out, float* clipmask, int64_t n, void* stream) {
  if (!lat || !out || n < 0 || (discretize != 0 && discretize != 1) || (discretize && !noise)) return SPA3D_ERR_ARG;
  OpCtx c(stream, nullptr, 0);
  k_discretize(&c, lat, noise, discretize, out, clipmask, n);
  return c.status();
}
#endif

}  // extern "C"
