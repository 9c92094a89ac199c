// attn_plan.hpp -- which kernel runs an attention.  The one place that decides it: the launchers in attention_fused.hip and qkv_attn.hip launch
// the kernel they are given, the front ends in attention.hip turn a refusal into its error, and the workspace-sizing dry run makes the same plan
// as the real run because the plan is a pure function of the descriptor (its pointers' alignment included) and the policy.  Host-only, no HIP
// headers, no element type: plain g++ -std=c++17 compiles it (tests/test_attn_plan_host.py checks the decisions on the CPU).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <initializer_list>

// ---- what the fused kernels are built for (attention_fused.hip, qkv_attn.hip; their own constexprs restate these as tile arithmetic)
constexpr int ATTN_DH = 96;           // head width
constexpr int ATTN_MAX_S = 320;       // self attention: K^ and V of one head resident, 2 x 320 x 192 B = 120 KiB of the CU's 160 KiB
constexpr int ATTN_BWD4_MAX_S = 160;  // backward with four resident images + wave tiles: fits 160 KiB up to here
constexpr int ATTN_XCHUNK = 128;      // chunked-key (cross) attention: at most this many query rows, keys cut into chunks of this many
constexpr int QKVA_MAX_S = 160, QKVA_D = 384;   // fused QKV projection + attention forward: rows per sequence, model width

// ------------------------------------------------------------------------------------------
// One attention problem: nseq sequences of H heads, Dh wide; o = softmax(rms(q) rms(k)^T / sqrt(Dh), key mask) v   (attention.py:166-175)
// ------------------------------------------------------------------------------------------
enum class AttnLayout {
  Dense,        // sequence i: query rows [i Sq, (i + 1) Sq), key rows [i Sk, (i + 1) Sk)
  RaggedRows,   // self attention after token pruning: sequence i = rows [seq_off[i], seq_off[i + 1]) of q / k / v / o, at most Sq = Sk of them
  RaggedKeys,   // Sq query rows per sequence; the keys of sequence i are rows [koff[i], koff[i + 1]) of the packed k / v (Sk unused)
  Hole          // Sq query rows per sequence; ONE shared key set, rows [0, Nk) of k / v, sequence i leaving out [holes[2i], holes[2i + 1]) (forward only)
};
struct AttnDesc {
  const void *q = nullptr, *k = nullptr, *v = nullptr; int64_t ldq = 0, ldk = 0, ldv = 0;   // row strides in elements
  const float *sq = nullptr, *sk = nullptr;   // the two per-head RMSNorm scales [Dh]
  const float* km = nullptr;                  // key mask [nseq][Sk] or null (Dense / RaggedRows)
  void* o = nullptr; float* lse = nullptr;    // o [rows][H Dh]; lse [rows][H][2] = (row max, log row sum), may be null in the forward; both read by the backward
  int64_t nseq = 0; int Sq = 0, Sk = 0, H = 0, Dh = 0;
  int esz = 2;                                // element size: 2 (bf16 / fp16) or 4 (the fp32 parity mode: generic composition only)
  // backward
  const void* d_o = nullptr; void *dq = nullptr, *dk = nullptr, *dv = nullptr; float *dsq = nullptr, *dsk = nullptr;
  AttnLayout layout = AttnLayout::Dense;
  const int32_t* seq_off = nullptr; int64_t total_rows = 0;              // RaggedRows: device offsets [nseq + 1], the rows present
  const int32_t *koff_host = nullptr, *koff_dev = nullptr;               // RaggedKeys: the same nseq + 1 offsets on both sides
  const int32_t *holes_host = nullptr, *holes_dev = nullptr; int Nk = 0; // Hole: the same 2 nseq bounds on both sides
  // fused QKV projection + attention forward only (plan_qkv_attn): q | k | v above are its OUTPUT, x [rows][ldx] the LayerNorm-ed input of width d
  const void *x = nullptr, *qkv_pk = nullptr; int64_t ldx = 0; int d = 0;

  int keys_of(int64_t i) const {
    if (layout == AttnLayout::RaggedKeys) return koff_host[i + 1] - koff_host[i];
    if (layout == AttnLayout::Hole) return Nk - (holes_host[2 * i + 1] - holes_host[2 * i]);
    return Sk;
  }
  int max_keys() const {   // the longest sequence's key count
    if (layout == AttnLayout::Dense || layout == AttnLayout::RaggedRows) return Sk;
    int m = 0;
    for (int64_t i = 0; i < nseq; ++i) m = std::max(m, keys_of(i));
    return m;
  }
  int64_t total_keys() const {
    if (layout == AttnLayout::RaggedKeys) return koff_host[nseq];
    int64_t t = 0;
    for (int64_t i = 0; i < nseq; ++i) t += keys_of(i);
    return t;
  }
  double rows_present() const { return total_rows > 0 ? (double)total_rows : (double)nseq * Sq; }   // what the profiler prices
};

// The kernel-choice switches behind "attn_impl" (include/spa3d.h) and the `impl` of spa3d_op_attention*.
struct AttnPolicy {
  bool generic = false;     // 1: the generic composition only
  bool fused_only = false;  // every value >= 2: the fused kernels or a refusal, never the generic composition
  int bwd_split = 0;        // 3 / 4: the split-pass backward on 4 / 8 waves also where the four-image kernel would run (S <= 160; tests)
  bool qkv_fused = false;   // 6: the track encoder's QKV projection + attention forward as ONE kernel (measured 1.47x slower than the pair: opt-in)
  static AttnPolicy from_impl(int v) {
    AttnPolicy p;
    p.generic = v == 1; p.fused_only = v >= 2;
    p.bwd_split = v == 3 ? 4 : (v == 4 ? 8 : 0);
    p.qkv_fused = v == 6;
    return p;
  }
};

// every route an attention can take.  Generic: GEMMs + row kernels over the whole batch (attention.hip); GenericPerSeq: the front end runs the sequences
// of a RaggedKeys / Hole problem one by one, each planned again as a Dense problem of one sequence.  SelfFwd: attn_fwd_kernel<KT, NW>.  XFwd*:
// xattn_fwd_kernel<HOLE> + xattn_combine_kernel over nsplit key chunks.  Bwd4 / Bwd4Fast: attn_bwd8_kernel<KT> with / without a key mask; BwdSplit4 / 8:
// attn_bwd_split_kernel<KT, 4 / 8>.  XBwd*: attn_bwd8_kernel<8, true, false, ragged> + xattn_dq_finish_kernel.  QkvFwd: qkva_fwd_kernel.
enum class AttnKernel { Refuse, Generic, GenericPerSeq, SelfFwd, XFwd, XFwdRaggedKeys, XFwdHole, Bwd4, Bwd4Fast, BwdSplit4, BwdSplit8, XBwd, XBwdRaggedKeys,
                        QkvFwd };
enum class AttnRefusal { None, RaggedNeedsFused, NotCovered };   // the caller's error: ragged rows have no generic route | attn_impl >= 2 and no fused kernel
struct AttnPlan {
  AttnKernel kernel = AttnKernel::Refuse;
  int KT = 0, NW = 0, nsplit = 0;     // tiles of 16 keys, waves per workgroup, key chunks
  int64_t part_bytes[2] = {0, 0};     // fp32 partials the route takes from the arena, in this order (XFwd*: opart, mlpart; XBwd*: dqpart), dry run included
  AttnRefusal why = AttnRefusal::None;
};
inline bool attn_is_fused(AttnKernel k) { return k >= AttnKernel::SelfFwd; }

// the one alignment predicate: 16-byte vector loads / stores on every row, so strides in multiples of 8 elements and 16-byte aligned bases
inline bool attn_al16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if ((uintptr_t)p & 15) return false;
  return true;
}
inline bool attn_aligned(const AttnDesc& d, bool bwd) {
  if (d.ldq % 8 || d.ldk % 8 || d.ldv % 8 || !attn_al16({d.q, d.k, d.v, d.o})) return false;
  return !bwd || attn_al16({d.d_o, d.dq, d.dk, d.dv, d.sq, d.sk});
}

// will the fused kernels take ragged self attention (token pruning) at this shape?  The model asks before it prunes
inline bool attn_takes_ragged_self(const AttnPolicy& p, int S, int Dh, int esz) {
  return !p.generic && esz == 2 && Dh == ATTN_DH && S >= 2 && S <= ATTN_MAX_S;
}

// ---- the fused kernels' own coverage: Refuse = none of them takes the problem
inline AttnPlan attn_plan_chunked(const AttnDesc& d, bool bwd) {   // Sq <= 128 query rows against keys in chunks of 128
  AttnPlan pl;
  const int Sk = d.max_keys();
  const int64_t nsplit = ((int64_t)Sk + ATTN_XCHUNK - 1) / ATTN_XCHUNK, nprob = d.nseq * d.H;
  if (d.layout == AttnLayout::RaggedRows || d.Sq < 1 || d.Sq > ATTN_XCHUNK || Sk < 1 || nprob * nsplit > 0x7fffffffLL) return pl;   // 32-bit grid
  if (!attn_aligned(d, bwd)) return pl;
  const bool rk = d.layout == AttnLayout::RaggedKeys;
  pl.KT = ATTN_XCHUNK / 16; pl.NW = bwd ? 8 : 4; pl.nsplit = (int)nsplit;
  pl.part_bytes[0] = nprob * nsplit * d.Sq * ATTN_DH * 4;
  if (bwd) { pl.kernel = rk ? AttnKernel::XBwdRaggedKeys : AttnKernel::XBwd; return pl; }
  pl.part_bytes[1] = nprob * nsplit * d.Sq * 2 * 4;
  pl.kernel = d.layout == AttnLayout::Hole ? AttnKernel::XFwdHole : (rk ? AttnKernel::XFwdRaggedKeys : AttnKernel::XFwd);
  return pl;
}
inline bool attn_self_ok(const AttnDesc& d, bool bwd) {   // one workgroup per (sequence, head), every key resident
  if (d.Dh != ATTN_DH || d.Sq != d.Sk || d.Sk < 2 || d.Sk > ATTN_MAX_S) return false;
  return attn_aligned(d, bwd) && d.nseq * d.H <= 0x7fffffffLL;   // the kernels index problems in 32 bits
}
inline AttnPlan attn_plan_fused_fwd(const AttnDesc& d) {
  AttnPlan pl;
  if (d.layout == AttnLayout::RaggedKeys) return d.Dh == ATTN_DH ? attn_plan_chunked(d, false) : pl;
  if (d.layout == AttnLayout::Hole) { const int nmax = d.max_keys(); return d.Dh == ATTN_DH && nmax >= 1 && nmax <= d.Nk ? attn_plan_chunked(d, false) : pl; }
  if (d.Dh == ATTN_DH && d.Sq != d.Sk) return attn_plan_chunked(d, false);
  if (!attn_self_ok(d, false)) return pl;
  // key / query tiles of 16; odd counts pair up (the last pair half empty) except nine (S = 129, the readout stack: its own instance)
  pl.KT = (d.Sk + 15) / 16;
  if ((pl.KT & 1) && pl.KT != 9) pl.KT += 1;
  pl.NW = pl.KT >= 14 ? 8 : 4;   // > 80 KiB of LDS: one workgroup per CU, so eight waves
  pl.kernel = AttnKernel::SelfFwd;
  return pl;
}
inline AttnPlan attn_plan_fused_bwd(const AttnDesc& d, const AttnPolicy& p) {
  AttnPlan pl;
  if (!d.o || !d.lse) return pl;   // P is rebuilt from the forward's o and (row max, log row sum)
  if (d.layout == AttnLayout::RaggedKeys) return d.Dh == ATTN_DH ? attn_plan_chunked(d, true) : pl;
  if (d.Dh == ATTN_DH && d.Sq != d.Sk) return attn_plan_chunked(d, true);
  if (!attn_self_ok(d, true)) return pl;
  // even tile counts only: the tile routines take an odd KT (the last pair half empty, as in the forward's nine-tile instance), but at S = 129 the backward
  // measured the same with nine tiles as with ten (3.43 vs 3.44-3.6 ms: its third ROUND of tiles, not the tenth key tile, is what S = 129 pays for there)
  pl.KT = (d.Sk + 31) / 32 * 2;
  // four resident images with concurrent roles up to S_pad = 160 (without a key mask: the cheap score arithmetic), else split-pass on 8 waves
  if (pl.KT * 16 > ATTN_BWD4_MAX_S || p.bwd_split == 8) { pl.kernel = AttnKernel::BwdSplit8; pl.NW = 8; }
  else if (p.bwd_split == 4) { pl.kernel = AttnKernel::BwdSplit4; pl.NW = 4; }
  else { pl.kernel = d.km ? AttnKernel::Bwd4 : AttnKernel::Bwd4Fast; pl.NW = 8; }
  return pl;
}

// ---- fused where the policy and the element size allow and a fused kernel covers it; else the generic composition, or the refusal it cannot stand in for
inline AttnPlan attn_plan_or_generic(const AttnDesc& d, const AttnPolicy& p, AttnPlan fused) {
  if (!p.generic && d.esz == 2 && fused.kernel != AttnKernel::Refuse) return fused;
  AttnPlan pl;
  if (d.layout == AttnLayout::RaggedKeys || d.layout == AttnLayout::Hole) pl.kernel = AttnKernel::GenericPerSeq;
  else if (d.layout == AttnLayout::RaggedRows) pl.why = AttnRefusal::RaggedNeedsFused;
  else if (p.fused_only) pl.why = AttnRefusal::NotCovered;
  else pl.kernel = AttnKernel::Generic;
  return pl;
}
inline AttnPlan plan_attn_fwd(const AttnDesc& d, const AttnPolicy& p) { return attn_plan_or_generic(d, p, attn_plan_fused_fwd(d)); }
inline AttnPlan plan_attn_bwd(const AttnDesc& d, const AttnPolicy& p) {
  if (d.layout == AttnLayout::Hole) { AttnPlan pl; pl.why = AttnRefusal::NotCovered; return pl; }   // leave-fold-out scoring has no backward
  return attn_plan_or_generic(d, p, attn_plan_fused_bwd(d, p));
}

// ---- the track encoder's QKV projection + attention forward as one kernel (opt-in): QkvFwd, or Refuse (then the projection GEMM and plan_attn_fwd)
inline bool plan_qkv_pack(const AttnPolicy& p, bool gemm_generic, bool cross, int d, int Dh) {   // whether a block's weight stream is built
  return p.qkv_fused && !gemm_generic && !cross && d == QKVA_D && Dh == ATTN_DH;
}
inline AttnPlan plan_qkv_attn(const AttnDesc& d, const AttnPolicy& p) {
  AttnPlan pl;
  if (!p.qkv_fused || d.esz != 2 || !d.qkv_pk || d.Dh != ATTN_DH || d.d != QKVA_D || d.Sq != d.Sk || d.Sk < 2 || d.Sk > QKVA_MAX_S || d.H < 1 || d.nseq < 1) return pl;
  if (d.ldx % 8 || !attn_al16({d.x, d.q, d.o, d.qkv_pk}) || d.nseq * d.H > 0x7fffffffLL) return pl;
  pl.kernel = AttnKernel::QkvFwd; pl.KT = QKVA_MAX_S / 16; pl.NW = 4;
  return pl;
}
