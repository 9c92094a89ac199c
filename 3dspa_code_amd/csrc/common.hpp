// common.hpp -- shared declarations for libspa3d_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/spa3d.h"
#include "ablate.inc"  // every work-skipping diagnostic mask, all 0 in libspa3d_hip.so
#include "gemm_plan.hpp"  // GemmDesc and the kernel choice (host-only)
#include "attn_plan.hpp"  // AttnDesc and the attention kernel choice (host-only)
#include "score_row.hpp"  // per-track score arithmetic (host- and device-callable)
#include "loss_point.hpp"  // the training objective at one point (host- and device-callable)
#include "adamw_point.hpp"   // clip -> AdamW -> EMA at one element (host- and device-callable)
#include "adamw_groups.hpp"  // the range table of the grouped optimizer: validation and lookup (host- and device-callable)

// One translation unit is compiled for exactly ONE 16-bit activation type: bf16 (default) or IEEE fp16 (-DSPA_F16=1, BASELINE
// cfg#5).  The raw 16-bit storage type is `bf16_t` (unsigned short) in both builds; what differs -- the two conversions, the MFMA
// instruction, the packed dot product -- is defined here, and everything device-side lives in a per-type namespace so the two builds
// of every source link into one library.  (No dual "platform" paths: both are gfx950-only code.)
#ifndef SPA_F16
#define SPA_F16 0
#endif
#if SPA_F16
#define SPA_NS h_f16
#else
#define SPA_NS h_bf16
#endif
typedef unsigned short bf16_t;  // raw 16-bit pattern (bf16, or fp16 in the SPA_F16 build); arithmetic is always done in f32

// ---- deterministic parameter gradients (spa3d_set_option "det_grads").  Every reduction INTO the flat gradient buffer (split-M dW tiles, bias / scale column sums,
// broadcast gradients) is a float atomic by default: fast, and its result depends on arrival order in the last bits.  In this mode the same call sites add 64-bit FIXED-POINT
// integers (exact, order-independent) into a shadow of the gradient buffer, which det_flush adds to the float buffer once a range is final.  The mode is per call: a
// det_grads train call writes its DetCfg into its own workspace (k_det_unit) and passes a pointer to it (spa3d_ctx::det) to every kernel that adds into the gradient
// buffer; nullptr = float atomics.  (A pointer, not the struct by value: kernel arguments are loaded at kernel entry, so the fields would stay live in SGPRs
// through the main loops -- SGPR spills in the LayerNorm backward, more VGPRs in the single-query attention backward; the struct is read where it is used.)
// Unit: one integer step is 1 / scale of the buffer's value, scale = 2^(32 + e) with e = floor(log2(denom / (n_vis * loss scale))) - floor(log2(gmax / 5000)) clamped to
// [DET_E_MIN, DET_E_MAX] (k_det_unit: a power of two, so the flush is exact; a gradient of this call scales as gmax * n_vis * loss scale / denom, gmax = the objective's
// largest head gradient per unit point weight, 5000 by default: the second term is then 0).  At a real batch n_vis ~ denom, so the unit is
// 2^-32 as it always was (2^-(32 + log2 ranks) data-parallel); it only gets finer when the denominator exceeds the call's own visible count.  Range: an addend of
// 2^55 units or more (or a NaN) sets the sticky flag instead of being added; a shadow sum of 2^62 units or more is taken as overflow by det_flush -- both flush NaN,
// never a wrapped finite value.  2^62 / 2^55 = 128 addends at the bound fit; a sum can only wrap past the flush check with 384 or more addends all near the bound.
// The single-query attention backward pre-sums in LDS and bounds its addends by 2^62 / (its problem count), so that sum cannot wrap either.
struct DetCfg { float* gbase; long long* shadow; long long n; unsigned* flag; float scale; };   // scale: the unit (k_det_unit)
constexpr float DET_ADDEND_MAX = 36028797018963968.f;   // 2^55 units
constexpr long long DET_SUM_MAX = 1ll << 62;
constexpr int DET_E_MIN = -24, DET_E_MAX = 40;   // the unit's exponent range (k_det_unit)

namespace SPA_NS {
#if SPA_F16
__device__ __forceinline__ float bf2f(bf16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
// round-to-nearest-even; overflows to inf beyond 65504 and flushes below 6e-8 (the fp16 mode scales the loss, model.hip)
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
typedef __attribute__((ext_vector_type(8))) _Float16 mfma16x8;
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)
#define MFMA32_ASM "v_mfma_f32_32x32x16_f16"
#define DOT2C_F32_16 "v_dot2c_f32_f16"
#define ONES2_16 0x3C003C00u  // (1.0, 1.0)
#else
__device__ __forceinline__ float bf2f(bf16_t h) { return __uint_as_float(((unsigned)h) << 16); }
// round-to-nearest-even; a plain cast emits v_cvt_pk_bf16_f32 and keeps NaN a NaN
// (MI355X_MICROARCH.md "Correctness boundaries")
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }
// the 16-bit activation type's MFMA operand vector and instructions (8 elements per lane)
typedef __attribute__((ext_vector_type(8))) __bf16 mfma16x8;
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)
#define MFMA32_ASM "v_mfma_f32_32x32x16_bf16"
#define DOT2C_F32_16 "v_dot2c_f32_bf16"
#define ONES2_16 0x3F803F80u  // (1.0, 1.0)
#endif
// two f32 -> one dword of two 16-bit values (low half = a): ONE v_cvt_pk_bf16_f32 (fp16 build: two converts + a pack).  The element-wise form
// (unsigned)f2bf(a) | ((unsigned)f2bf(b) << 16) compiles to a convert per element plus a shift / mask / or: three VALU operations per pair in every GEMM epilogue.
#if SPA_F16
typedef __attribute__((ext_vector_type(2))) _Float16 spa_h16x2;
#else
typedef __attribute__((ext_vector_type(2))) __bf16 spa_h16x2;
#endif
typedef __attribute__((ext_vector_type(2))) float spa_f32x2;
__device__ __forceinline__ unsigned f2bf_pack2(float a, float b) { return __builtin_bit_cast(unsigned, __builtin_convertvector(spa_f32x2{a, b}, spa_h16x2)); }
// the two 16-bit halves of a packed dword as f32
__device__ __forceinline__ float unpack_lo(unsigned u) { return bf2f((bf16_t)(u & 0xffffu)); }
__device__ __forceinline__ float unpack_hi(unsigned u) { return bf2f((bf16_t)(u >> 16)); }
template <typename T> __device__ __forceinline__ float ld(const T* p);
template <> __device__ __forceinline__ float ld<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ld<bf16_t>(const bf16_t* p) { return bf2f(*p); }
template <typename T> __device__ __forceinline__ void st(T* p, float v);
template <> __device__ __forceinline__ void st<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void st<bf16_t>(bf16_t* p, float v) { *p = f2bf(v); }

__device__ __forceinline__ float gelu_tanh_f(float x) {
  const float c = 0.7978845608028654f;  // sqrt(2/pi)
  float u = c * (x + 0.044715f * x * x * x);
  return 0.5f * x * (1.0f + tanhf(u));
}
__device__ __forceinline__ float gelu_tanh_grad_f(float x) {
  const float c = 0.7978845608028654f;
  float u = c * (x + 0.044715f * x * x * x);
  float t = tanhf(u);
  return 0.5f * (1.0f + t) + 0.5f * x * (1.0f - t * t) * c * (1.0f + 3.0f * 0.044715f * x * x);
}

// bf16-path variants (tiled GEMM epilogues only; the fp32 parity path keeps tanhf): gelu(x) = x*s, s = sigmoid(2u) = 1/(1+exp(-2u)),
// gelu'(x) = s*(1 + 2x(1-s)u'), one v_exp_f32 + one v_rcp_f32 (abs error ~1e-7, far below bf16 rounding).
__device__ __forceinline__ float gelu_sigmoid_2u(float x) {
  // exp(-2u) = 2^(x (A + B x^2)) with A = -2 sqrt(2/pi) log2(e), B = 0.044715 A: one fma and two multiplies feed v_exp_f32 directly
  constexpr float A = (float)(-2.0 * 0.7978845608028654 * 1.4426950408889634), B = (float)(-2.0 * 0.7978845608028654 * 1.4426950408889634 * 0.044715);
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * __builtin_fmaf(B, x * x, A)));
}
__device__ __forceinline__ float gelu_tanh_fast_f(float x) { return x * gelu_sigmoid_2u(x); }
__device__ __forceinline__ float gelu_tanh_grad_fast_f(float x) {
  const float s = gelu_sigmoid_2u(x);
  const float du = 0.7978845608028654f * (1.0f + 3.0f * 0.044715f * x * x);
  return s * (1.0f + 2.0f * x * (1.0f - s) * du);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// 16 bytes per lane and access: 4 f32 or 8 values of the 16-bit type, as floats in registers
template <typename T> struct VecOf;
template <> struct VecOf<float> { static constexpr int N = 4; };
template <> struct VecOf<bf16_t> { static constexpr int N = 8; };
template <typename T, int NV>
__device__ __forceinline__ void load_vec(const T* p, float (&f)[NV]) {
  if constexpr (sizeof(T) == 4) { const float4 v = *(const float4*)p; f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w; }
  else { const uint4 v = *(const uint4*)p; const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = unpack_lo(u[i]); f[2 * i + 1] = unpack_hi(u[i]); } }
}
template <typename T, int NV>
__device__ __forceinline__ void store_vec(T* p, const float (&f)[NV]) {
  if constexpr (sizeof(T) == 4) { *(float4*)p = make_float4(f[0], f[1], f[2], f[3]); }
  else { unsigned u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = f2bf_pack2(f[2 * i], f[2 * i + 1]);
    *(uint4*)p = make_uint4(u[0], u[1], u[2], u[3]); }
}

// A kernel with many additions reads the mode ONCE and passes it along; the cold sites (one addition per thread at a workgroup's end) read it at the addition.
__device__ __forceinline__ DetCfg det_read(const DetCfg* d) { return d ? *d : DetCfg{nullptr, nullptr, 0, nullptr, 4294967296.f}; }
__device__ __forceinline__ void grad_add(const DetCfg& dc, float* p, float v) {
  if (dc.shadow) {
    const long long i = p - dc.gbase;
    if ((unsigned long long)i < (unsigned long long)dc.n) {
      const float f = v * dc.scale;
      if (fabsf(f) < DET_ADDEND_MAX) atomicAdd((unsigned long long*)(dc.shadow + i), (unsigned long long)__float2ll_rn(f));   // NaN fails the comparison too
      else atomicOr(dc.flag, 1u);                                                                                              // sticky: det_flush then writes NaN
      return;
    }
  }
  atomicAdd(p, v);
}
// an addend already in fixed point (a workgroup's exact integer sum): straight into the shadow, no second rounding; |q| >= 2^62 is overflow
__device__ __forceinline__ void grad_add_q(const DetCfg& dc, float* p, long long q) {
  if (dc.shadow) {
    const long long i = p - dc.gbase;
    if ((unsigned long long)i < (unsigned long long)dc.n) {
      if (q < DET_SUM_MAX && q > -DET_SUM_MAX) atomicAdd((unsigned long long*)(dc.shadow + i), (unsigned long long)q);
      else atomicOr(dc.flag, 1u);
      return;
    }
  }
  atomicAdd(p, (float)((double)q / (double)dc.scale));
}
}  // namespace SPA_NS

// ------------------------------------------------------------------------------------------
// host-side context
// ------------------------------------------------------------------------------------------
// One launch of score_rows_kernel (loss.hip): rows [row0, row0 + nq) of the [B * Q] query rows.  Targets, sample scale, query_stats and frame_err are the
// caller's whole tensors, indexed by the global row; the predictions come either from this launch's head rows (head != null: [nq][4 * T], coordinate-major,
// row 0 = global row row0) or from the caller's split tensors (tracks [B * Q][T][NC], vlog [B * Q][T]).  The thresholds travel by value.
struct ScoreArgs {
  const float* head; const float* tracks; const float* vlog;
  const float* tgt; const float* tvis; const float* scale;  // scale: device [B] or null
  float* qstats; float* frame_err;                          // frame_err: [B * Q][T] or null
  int64_t nq, row0; int Q, T, NC; ScoreThr thr;
};

// render.hip's one constant that is read from outside it: tests/test_gpu_render.py sizes its compaction-order case by this line
constexpr int RENDER_CHUNK = 256;   // points culled and compacted per round of the tile pass (= its workgroup size)

struct Leaf {
  std::string name;
  int ndim;
  int64_t shape[4];
  int64_t offset;
  int64_t numel() const { int64_t n = 1; for (int i = 0; i < ndim; ++i) n *= shape[i]; return n; }
};

struct Arena {  // bump allocator over the caller's workspace; dry mode only counts
  char* base = nullptr;
  int64_t cap = 0, off = 0, peak = 0;
  bool dry = false, overflow = false;
  void* alloc(int64_t bytes) {
    int64_t a = (off + 255) & ~int64_t(255);
    off = a + bytes;
    if (off > peak) peak = off;
    if (dry) return (void*)(uintptr_t)(0x1000 + a);  // never dereferenced
    if (off > cap) { overflow = true; return base; }
    return base + a;
  }
  int64_t mark() const { return off; }
  void release(int64_t m) { off = m; }
};

// live per-kernel-class timing with HIP events on the launch stream (bench.py "roofline"; off by default)
enum { PROF_GEMM_NT = 0, PROF_GEMM_TN = 1, PROF_GEMM_GENERIC = 2, PROF_ATTN_FWD = 3, PROF_ATTN_BWD = 4, PROF_LN_FWD = 5, PROF_LN_BWD = 6,
       PROF_ATTN_Q1 = 7, PROF_EMBED = 8, PROF_NCLS = 9 };  // PROF_EMBED brackets the whole input-embedding stage (its GEMMs are also in PROF_GEMM_NT)
struct ProfRec { int cls; double flops, bytes; hipEvent_t e0, e1; int64_t tag[4] = {0, 0, 0, 0}; };  // tag: M, N, K, flags (GEMMs)
struct Prof {
  bool on = false;
  std::vector<hipEvent_t> pool; size_t used = 0;
  std::vector<ProfRec> recs;
  hipEvent_t get() {
    if (used == pool.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; pool.push_back(e); }
    return pool[used++];
  }
};

inline spa3d_loss_config loss_config_defaults() {  // train.py:96
  spa3d_loss_config d;
  d.l1_weight = 5000.0f; d.bce_weight = 1e-8f; d.position_kind = SPA3D_POS_L1; d.huber_delta = 1.f;
  d.axis_weight[0] = d.axis_weight[1] = d.axis_weight[2] = 1.f; d.bce_pos_weight = 1.f;
  return d;
}

struct spa3d_ctx {
  spa3d_config cfg;
  std::vector<Leaf> leaves;
  int64_t nparams = 0;
  std::string err;
  hipStream_t stream = nullptr;
  Arena ar;
  bool dry = false;   // orchestration runs without launching (workspace sizing)
  int hip_err = 0;
  GemmPolicy gemm;    // "gemm_impl": which kernels the GEMMs may run on (gemm_plan.hpp)
  AttnPolicy attn;    // "attn_impl": which kernels the attentions may run on (attn_plan.hpp)
  int chunk = 0;      // samples per chunk: 0 = as many as fit the workspace (spa3d_set_option "chunk")
  int query_chunk = 0;    // spa3d_set_option "query_chunk": readout over chunks of this many queries (0 = all Q at once); implies one sample per chunk
  int track_chunk = 0;    // spa3d_set_option "track_chunk": track encoder over chunks of this many tracks, recomputed in the backward (0 = off); one sample per chunk
  int ro_share = 1;       // readout block 1: LayerNorm / QKV once per distinct (sample, query frame) instead of per query (16-bit modes); SPA3D_RO_SHARE=0 disables
  int prune = 1;          // drop masked frame tokens from the track encoder (3DSPA model, fused 16-bit attention path); SPA3D_PRUNE=0 disables
  float loss_scale = 1.f;  // the 16-bit backward runs at loss x scale, parameter gradients are scaled back at the end: 1 = off (bf16 / fp32),
                           // > 0 a fixed scale, < 0 automatic with |loss_scale| the target head-gradient magnitude (fp16 mode: -16)
  void* grad_ev[2] = {nullptr, nullptr};  // spa3d_set_grad_events: recorded on the launch stream when a gradient segment is final (last chunk)
  int64_t grad_ev_gen[2] = {0, 0};  // how many times each event has been recorded (spa3d_grad_events_recorded)
  bool last_chunk = false;
  const float* loss_scale_state = nullptr;  // caller-owned device float (spa3d_set_loss_scale_state): dynamic multiplier of the loss scale
  double plan_stats[4] = {0, 0, 0, 0};  // last train call: encoder rows kept, encoder rows dense, readout slots, queries (spa3d_plan_stats)
  int det_grads = 0;      // spa3d_set_option "det_grads": order-independent parameter gradients (fixed-point shadow accumulation, DetCfg above); costs a few %
  const DetCfg* det = nullptr;  // the running det_grads train call's mode, in its workspace, passed to every kernel that adds into G; nullptr = float atomics
  // spa3d_set_counts: per-sample live support tracks / live queries of the next calls' batch (host copies; cnt_B entries each)
  std::vector<int32_t> cnt_n, cnt_q; bool has_cnt_n = false, has_cnt_q = false; int cnt_B = 0;
  // spa3d_set_loss: the objective of spa3d_loss_and_grads / spa3d_loss, with what follows from it -- gmax = max(l1_weight * max_c a_c, bce_weight * max(1, beta)),
  // the head gradient's bound per unit point weight (fp16 automatic loss scale), and gshift = floor(log2(gmax / 5000)) (det_grads unit)
  spa3d_loss_config loss = loss_config_defaults(); float loss_gmax = 5000.f; int loss_gshift = 0;
  // spa3d_set_point_weights: caller-owned device plane [B,Q,T_out] of the next calls' batch (null = every weight 1) and the B, Q it was stated for
  const float* pt_w = nullptr; int pt_B = 0, pt_Q = 0;
  int poison = 0;         // spa3d_set_option "poison": NaN-fill the workspace before every chunk and every op output before its launch (tests)
  int freeze = 0;         // spa3d_set_option "freeze": spa3d_loss_and_grads stops its backward at a stage boundary -- 1: [0, b1) of the flat buffer (embeddings,
                          // track encoder, state_init leaves) is frozen, 2: [0, b2) (the latent stacks too); run_chunk (model.hip) skips the stages whole
  Prof prof;
};

// ---- the scaffold of a call: sizing walk, sized call, query counts, live rows ----
// Peak arena bytes of `body` walked with launches off (c->dry) against a counting arena; the arena and the mode come back as they were.
// The caller adds its own slack.
template <typename F> inline int64_t arena_peak(spa3d_ctx* c, F&& body) {
  const Arena saved = c->ar; const bool sd = c->dry;
  c->ar = Arena(); c->ar.dry = true; c->dry = true;
  body();
  const int64_t peak = c->ar.peak;
  c->ar = saved; c->dry = sd;
  return peak;
}
// A call whose need is known: refused (SPA3D_ERR_ARG, "<what>: workspace too small: need N bytes") without a workspace of `need` bytes;
// else `body` runs on `stream` against the caller's workspace.
template <typename F> inline int sized_call(spa3d_ctx* c, const char* what, int64_t need, void* ws, int64_t ws_bytes, void* stream, F&& body) {
  if (!ws || ws_bytes < need) { c->err = std::string(what) + ": workspace too small: need " + std::to_string(need) + " bytes"; return SPA3D_ERR_ARG; }
  c->stream = (hipStream_t)stream; c->dry = false;
  c->ar = Arena(); c->ar.base = (char*)ws; c->ar.cap = ws_bytes;
  body();
  if (c->ar.overflow) { c->err = "internal: arena overflow"; return SPA3D_ERR_WORKSPACE; }
  return c->hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}
// spa3d_set_counts against a batch of B samples: false with c->err set when the counts were set for another B
inline bool counts_fit_batch(spa3d_ctx* c, int B) {
  if (c->cnt_B == B) return true;
  c->err = "counts were set for B = " + std::to_string(c->cnt_B) + ", this batch has B = " + std::to_string(B);
  return false;
}
// spa3d_set_point_weights against a batch of B samples of Q queries: false with c->err set when the plane was stated for another shape
inline bool weights_fit_batch(spa3d_ctx* c, int B, int Q) {
  if (!c->pt_w || (c->pt_B == B && c->pt_Q == Q)) return true;
  c->err = "point weights were set for B = " + std::to_string(c->pt_B) + ", Q = " + std::to_string(c->pt_Q) + ", this batch has B = " + std::to_string(B) +
           ", Q = " + std::to_string(Q);
  return false;
}
// The live-query counts [B] of a handle that has them (c->has_cnt_q), checked against a batch of B samples of Q queries; null with c->err
// set when they do not fit it.
inline const int32_t* checked_query_counts(spa3d_ctx* c, int B, int Q) {
  if (!counts_fit_batch(c, B)) return nullptr;
  for (int i = 0; i < B; ++i)
    if (c->cnt_q[i] < 0 || c->cnt_q[i] > Q) {
      c->err = "query_count[" + std::to_string(i) + "] = " + std::to_string(c->cnt_q[i]) + " is outside [0, Q = " + std::to_string(Q) + "]";
      return nullptr;
    }
  return c->cnt_q.data();
}
// f(row0, nq) over the live rows of the [B * Q] query rows: the whole batch at once without counts, else sample by sample, rows
// [i * Q, i * Q + cq[i]) -- the padded rows of sample i follow its span
template <typename F> inline void for_each_live_span(const int32_t* cq, int64_t B, int64_t Q, F&& f) {
  if (!cq) { f((int64_t)0, B * Q); return; }
  for (int64_t i = 0; i < B; ++i) f(i * Q, (int64_t)cq[i]);
}

struct ProfScope {  // records an event pair around the launches issued in its lifetime
  spa3d_ctx* c; ProfRec r; bool on;
  ProfScope(spa3d_ctx* c_, int cls, double flops, double bytes) : c(c_), on(c_->prof.on && !c_->dry) {
    if (!on) return;
    r.cls = cls; r.flops = flops; r.bytes = bytes; r.e0 = c->prof.get(); r.e1 = c->prof.get();
    if (!r.e0 || !r.e1) { on = false; return; }
    (void)hipEventRecord(r.e0, c->stream);
  }
  void tag(int64_t a, int64_t b, int64_t c2, int64_t d) { r.tag[0] = a; r.tag[1] = b; r.tag[2] = c2; r.tag[3] = d; }
  ~ProfScope() { if (on) { (void)hipEventRecord(r.e1, c->stream); c->prof.recs.push_back(r); } }
};

#define SPA_LAUNCH_CHECK(ctx)                                                     \
  do {                                                                            \
    hipError_t e__ = hipGetLastError();                                           \
    if (e__ != hipSuccess && (ctx)->hip_err == 0) {                               \
      (ctx)->hip_err = (int)e__;                                                  \
      (ctx)->err = std::string("HIP launch failed at ") + __FILE__ + ":" +        \
                   std::to_string(__LINE__) + ": " + hipGetErrorString(e__);      \
    }                                                                             \
  } while (0)

// launch geometry of the element-wise kernels: a 1-D grid of at most 2^20 workgroups of bs threads over n items (the kernels stride)
#define GRID1D(n, bs) dim3((unsigned)std::min<int64_t>(((n) + (bs)-1) / (bs), 1 << 20))
static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

namespace SPA_NS {
template <typename T> void gemm_generic(spa3d_ctx* c, const GemmDesc& d);
// The GEMM launchers: each launches the kernel gemm_plan.hpp chose for the descriptor (never a refused or dry-run plan: gemm_launch)
void gemm_nt_bf16(spa3d_ctx* c, const GemmDesc& d, GemmKernel k);   // the tiled NT kernels (gemm_fast.hip)
void gemm_tn_bf16(spa3d_ctx* c, const GemmDesc& d, GemmKernel k);   // the dW kernels (gemm_fast.hip, gemm_tnb.hip)
// large-register-tile NT GEMM (gemm_ntb.hip): C[M,N] (16-bit) = A[M,K] . W (+ bias), N a multiple of 384 (tile 256 x 384) or 256 (384 x 256), K % 32 == 0;
// W pre-packed by gemm_ntb_pack (element (k, n) of W at w[k*sk + n*sn]) as d.ntb_pk
int64_t gemm_ntb_pack_elems(int K, int N);
template <typename S> void gemm_ntb_pack(spa3d_ctx* c, const S* w, int64_t sk, int64_t sn, int K, int N, bf16_t* wpk);
void gemm_ntb(spa3d_ctx* c, const GemmDesc& d);
// row-stationary K = 384 GEMM (gemm_rs.hip): C[M,N] = A[M,384] . W (+ bias) with W pre-packed into the kernel's fragment stream (element (k, n) of W at w[k*sk + n*sn])
// as d.rs_pk; EPI_MUL_GELU_GRAD: C = (A . W + bias) o gelu'(d.aux) (C's layout): the MLP backward's dh
int64_t gemm_rs_pack_elems(int N);
template <typename S> void gemm_rs_pack(spa3d_ctx* c, const S* w, int64_t sk, int64_t sn, int N, bf16_t* wpk);
void gemm_rs(spa3d_ctx* c, const GemmDesc& d);
// QKV projection + attention forward of one (sequence, head) per workgroup pass (qkv_attn.hip): the weight stream, and the launcher of plan_qkv_attn's QkvFwd
int64_t qkv_attn_pack_elems(int H);
template <typename S> void qkv_attn_pack(spa3d_ctx* c, const S* wq, const S* wk, const S* wv /* [384][E] */, int E, int H, bf16_t* wpk);
void qkv_attn_launch(spa3d_ctx* c, const AttnDesc& d);
// the fused attention kernels (attention_fused.hip): launches a fused route of plan_attn_fwd / plan_attn_bwd; `part`: the plan's fp32 partials
void attn_fused_launch(spa3d_ctx* c, const AttnDesc& d, const AttnPlan& pl, float* const part[2]);
// sequence-resident MLP forward for d = 384, mlp = 1536 (mlp_fused.hip): y = a + MLP(na), h / hpre kept; launched when plan_mlp says MlpFused
template <typename S> void mlp_fused_pack(spa3d_ctx* c, const S* w_in /*[384][1536]*/, const S* w_out /*[1536][384]*/, bf16_t* wpk);
int64_t mlp_fused_pack_elems();
void mlp_fused_fwd(spa3d_ctx* c, const bf16_t* na, const bf16_t* a, bf16_t* y, bf16_t* h, bf16_t* hpre, int64_t M, const bf16_t* wpk,
                   const float* b_in, const float* b_out);
// runs a planned GEMM (not Refuse); nothing in the dry run, which only needed the plan
template <typename T> void gemm_launch(spa3d_ctx* c, const GemmDesc& d, GemmKernel k) {
  if (c->dry) return;
  if constexpr (sizeof(T) == 2) {
    if (k == GemmKernel::Rs) return gemm_rs(c, d);
    if (k == GemmKernel::Ntb) return gemm_ntb(c, d);
    if (gemm_is_tn(k)) return gemm_tn_bf16(c, d, k);
    if (k != GemmKernel::Generic) return gemm_nt_bf16(c, d, k);
  }
  gemm_generic<T>(c, d);
}

// ------------------------------------------------------------------------------------------
// launchers of the kernel units, grouped by file in each file's order; all asynchronous on c->stream; no-ops when c->dry
// ------------------------------------------------------------------------------------------
// layernorm.hip
template <typename T> void k_layernorm(spa3d_ctx*, const T* x, const float* scale, T* y, float* stats, int64_t rows, int d);
template <typename T> void k_layernorm_bwd(spa3d_ctx*, const T* x, const float* scale, const float* stats, const T* dy, T* dx,
                                           float* dscale, int64_t rows, int d, const T* add);
// attention.hip: the attention front ends -- plan (attn_plan.hpp), then the fused launchers, the generic composition (whole, or sequence by sequence for
// ragged keys / a hole) or the refusal's error; and the launch of a fused plan, which in the dry run only takes the plan's partials from the arena
template <typename T> void attention_fwd(spa3d_ctx* c, const AttnDesc& d);
template <typename T> void attention_bwd(spa3d_ctx* c, const AttnDesc& d);
void attn_launch(spa3d_ctx* c, const AttnDesc& d, const AttnPlan& pl);
// embed.hip
template <typename T> void k_sin_embed(spa3d_ctx*, const float* x, int64_t rows, int C, int nf, float prescale, T* out);
template <typename T> void k_embed_tokens(spa3d_ctx*, const float* tracks, int64_t nrows, int T_, int nf, float prescale, T* sinbuf, int NC = 3);
void k_query_embed1(spa3d_ctx*, const float* qp, int64_t nq, int nf, float track_scale, float time_scale, float* feat, int32_t* qframe,
                    int NC = 3);
template <typename T> void k_embed_maps(spa3d_ctx*, const int32_t* row_src, int64_t rows, int S, int T_, int32_t* arow, int32_t* crow, T* tok, const float* readout, int d);
template <typename T> void k_set_readout_rows(spa3d_ctx*, T* tok, const float* readout, int64_t nseq, int S, int d);
void k_keymask(spa3d_ctx*, const float* visible, const int32_t* boundary, int64_t nseq, int N, int T_, float* km);
void k_keymask2d(spa3d_ctx*, const float* visible, const int32_t* boundary, int64_t nseq, int N, int T_, float* km);  // 2-D TRAJAN twin (track_autoencoder.py:117-390)
void k_sum3(spa3d_ctx*, const float* a, const float* b, const float* c3, float* out, int n);
// Dense with input width K <= 4 as streaming kernels (false: shape not covered, use the GEMM path); instantiated for the 16-bit type only
template <typename T> bool k_rank_fwd(spa3d_ctx*, const T* x, const T* w /*[K][N]*/, const float* bias, T* out /*+=*/, int64_t M, int N, int K, int64_t ldo,
                                      int rgroup, int rskip);
template <typename T> bool k_rank_bwd(spa3d_ctx*, const T* x, const T* dy, int64_t M, int N, int K, int64_t ldy, int rgroup, int rskip, float* gw /*+=*/,
                                      float* gb /*+=, may be null*/);
template <typename T> void k_pack(spa3d_ctx*, const float* src, int64_t src_ld, int rows, int cols, T* dst_native, int64_t ldn, T* dst_T, int64_t ldt);
template <typename T> void k_transpose(spa3d_ctx*, const T* src, int rows, int cols, T* dst);  // dst[c][r] = src[r][c]
// rows.hip
void k_zero(spa3d_ctx*, void* p, int64_t bytes);
void k_set_i32(spa3d_ctx*, int32_t* dst, const int32_t* host, int64_t n);  // n host ints -> device, by value in the launch arguments
void k_mul(spa3d_ctx*, float* a, const float* b, int64_t n);
template <typename T> void k_cast_from_f32(spa3d_ctx*, const float* src, T* dst, int64_t n);
template <typename T> void k_cast_to_f32(spa3d_ctx*, const T* src, float* dst, int64_t n);
template <typename T> void k_colsum(spa3d_ctx*, const T* x, int64_t rows, int n, int64_t ld, float* out /*accumulated*/, int rgroup = 0,
                                    int rskip = 0);
template <typename T> void k_gather_rows(spa3d_ctx*, const T* src, int64_t src_stride_rows, T* dst, int64_t n, int d);
template <typename T> void k_rows_idx(spa3d_ctx*, int mode /*0 gather, 1 scatter, 2 scatter-add*/, const T* src, const int32_t* idx, T* dst, int64_t n, int d);
template <typename T> void k_add_rows_strided(spa3d_ctx*, T* dst, const T* src, int64_t dst_stride_rows, int64_t n, int d);
// token pruning of the track encoder: the plan (returns the kept-row count, one stream sync); k_rows_idx moves the rows
int64_t k_prune_plan(spa3d_ctx*, const float* km, int64_t nseq, int S, int32_t* cnt, int32_t* seq_off, int32_t* row_src);
// shared latent rows of the readout stack's first block (rows.hip "Shared latent rows"; model.hip Share)
int64_t k_share_plan(spa3d_ctx*, const int32_t* qframe, int64_t B, int Q, int32_t* slot, int32_t* slot_b, int32_t* slot_f, int32_t* slot_q0, int32_t* scratch);
template <typename T> void k_share_assemble(spa3d_ctx*, const T* qtok, const T* lat, const int32_t* slot_b, const int32_t* slot_f, int64_t nslot, int64_t BQ,
                                            int L, int Cl, int D, T* xU);
template <typename T> void k_share_expand(spa3d_ctx*, const T* srcU, const int32_t* slot, const int32_t* slot_q0, int64_t nslot, int64_t nseq, int S, int d,
                                          const T* add, T* dst);
template <typename T> void k_share_reduce(spa3d_ctx*, const T* src, const int32_t* slot, const int32_t* slot_b, int64_t nslot, int64_t nseq, int Q, int S, int d,
                                          T* dstU);
template <typename T> void k_assemble_readout(spa3d_ctx*, const T* qtok, const T* lat, const int32_t* qframe, int64_t B, int Q, int L, int Cl,
                                              int D, T* seq);
template <typename T> void k_assemble_readout_bwd(spa3d_ctx*, const T* dseq, const int32_t* qframe, int64_t B, int Q, int L, int Cl, int D,
                                                  T* dqtok, float* dlat, bool accumulate = false);
template <typename T> void k_broadcast_rows(spa3d_ctx*, const float* src, int rows, int d, T* dst, int64_t B);
template <typename T> void k_bcast_grad(spa3d_ctx*, const T* dsrc, int64_t per, int64_t B, int64_t bstride, float* dparam);
// 2-D TRAJAN twin (track_autoencoder.py:117-390)
template <typename T> void k_vis_mean_pool(spa3d_ctx*, const T* tok, const float* vis, int64_t nseq, int T_, int d, T* out);
template <typename T> void k_vis_mean_pool_bwd(spa3d_ctx*, const T* dout, const float* vis, int64_t nseq, int T_, int d, T* dtok);
// attn_q1.hip: single-query attention of the pruned last block
template <typename T> void k_attn_q1_fwd(spa3d_ctx*, const T* q0, int64_t ldq0, const T* k, const T* v, int64_t ldk, int64_t ldv,
                                         const float* sq, const float* sk, const float* km, int64_t nseq, int S, int H, int Dh, T* o0,
                                         float* p0, const int32_t* seq_off = nullptr);
template <typename T> void k_attn_q1_bwd(spa3d_ctx*, const T* q0, int64_t ldq0, const T* k, const T* v, int64_t ldk, int64_t ldv,
                                         const float* sq, const float* sk, const float* km, int64_t nseq, int S, int H, int Dh,
                                         const float* p0, const T* d_o0, T* dq0, T* dk, T* dv, float* dsq, float* dsk,
                                         const int32_t* seq_off = nullptr);
// loss.hip
void k_discretize(spa3d_ctx*, const float* lat, const float* noise, int discretize, float* out, float* clipmask, int64_t n);
void k_loss_fwd(spa3d_ctx*, const float* head, int64_t nq, int T_, const float* tgt, const float* tvis, float* tracks, float* vlog,
                float* clog, float* sums, unsigned* poison, int NC, const spa3d_loss_config& lc, const float* wgt);
void k_loss_from_preds(spa3d_ctx*, const float* tracks, const float* vlog, int64_t n, const float* tgt, const float* tvis, float* sums,
                       unsigned* poison, int NC, const spa3d_loss_config& lc, const float* wgt);
void k_score_rows(spa3d_ctx*, const ScoreArgs& a);
void k_score_reduce(spa3d_ctx*, const float* qstats, int64_t B, int Q, int K, double* out /*[B][8 + 4K]*/);
void k_vis_count(spa3d_ctx*, const float* tvis, int64_t n, float* out, unsigned* poison);
void k_set_denom(spa3d_ctx*, const float* sums, const unsigned* poison, float denom_host, float* denom_dev);
void k_loss_finalize(spa3d_ctx*, const float* sums, const unsigned* poison, const float* denom_dev, float l1w, float bcew, float* loss3);
template <typename T> void k_loss_bwd(spa3d_ctx*, const float* head, int64_t nq, int T_, const float* tgt, const float* tvis,
                                      const float* denom_dev, const spa3d_loss_config& lc, const float* wgt, T* dhead, int NC = 3,
                                      const float* scale_dev = nullptr);
void k_set_loss_scale(spa3d_ctx*, const float* denom_dev, float gmax, float setting, float* scale_dev);
void k_unscale(spa3d_ctx*, float* a, const float* scale_dev, int64_t n);
void k_adamw(spa3d_ctx*, float* p, const float* g, float* m, float* v, int64_t n, float lr, int64_t step, float clip, float b1, float b2,
             float eps, float wd, float* scratch);
// grouped AdamW + weight EMA (spa3d_adamw_step_groups): `groups` is a validated HOST table, `ws` holds adamw_groups_ws_bytes(num) device bytes
int64_t adamw_groups_ws_bytes(int num);
void k_adamw_groups(spa3d_ctx*, float* p, const float* g, float* m, float* v, int64_t n, float lr, int64_t step, float clip, float b1, float b2,
                    float eps, float wd, const AdamwGroup* groups, int num, float* ema, float ema_decay, float* scratch, void* ws);
void k_uniform_noise(spa3d_ctx*, float* out, int64_t n, uint32_t k0, uint32_t k1);
// over [lo, lo + n) of c->det: g[i] += shadow[i] / scale; shadow[i] = 0; NaN when *flag or |shadow[i]| >= 2^62
void k_det_flush(spa3d_ctx* c, int64_t lo, int64_t n);
// *out = d with the call's unit as its scale (DetCfg unit rule)
void k_det_unit(spa3d_ctx*, const float* sums, const unsigned* poison, const float* denom_dev, const float* scale_dev, int gshift, const DetCfg& d, DetCfg* out);
}  // namespace SPA_NS
using namespace SPA_NS;  // one 16-bit type per translation unit
