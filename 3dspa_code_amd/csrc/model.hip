// model.hip -- host orchestration of the 3DSPA TrackAutoEncoder3D forward / loss / backward on gfx950
// and the C-ABI of include/spa3d.h that runs the network or reads its predictions (forward, score, loss,
// options).  A stand-alone API lives whole in the file of its kernels -- tapvid3d.hip, render.hip,
// batch_build.hip -- on the call scaffold of common.hpp.  The graph follows SURVEY.md 0.1 (E1-E7, L1-L3, D1-D8, LOSS) with
// repairs R2-R5; file:line references are to /root/reference.
//
// Memory plan: the batch is processed in chunks of `Bc` samples (every op is per-sample; the only
// batch-global quantity, the loss denominator, is computed from the targets up front).  Within a chunk
// all block intermediates needed by the backward are stashed in the caller's workspace (bump arena);
// parameter gradients accumulate in fp32 across chunks.
//
// Sequencing: run_body owns what belongs to the call (weight shadows, denominator, noise, det_grads, unscaling, the loss, the score reduction) and cuts
// the batch into chunks; run_chunk is the ONE route a chunk takes through the stages of Net -- encode_tracks, encode_latents, decode_latents,
// decode_queries, emit_outputs, backward_queries, backward_latents, backward_tracks -- whatever it is: uniform, one sample of a ragged batch, several
// packed, sliced by "track_chunk" / "query_chunk".  Only run_folds (spa3d_score_folds), whose chunk changes shape between the stages, sequences them itself.
// Every entry point that runs the network ends in sized_run: need at the least count, largest count that fits, run, status.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

#include "common.hpp"
#include <cstdio>

enum { MODE_FORWARD = 0, MODE_TRAIN = 1, MODE_ENCODE = 2, MODE_DECODE = 3 };

struct RunArgs {
  int mode; const float* P; const spa3d_batch* b; float denom; float* G; int accumulate; float* loss3; spa3d_outputs* out;
  const float* latents_in; float* latents_out; int chunk;  // chunk: fixed Bc (>0) or 0 = as large as fits
  const int32_t* cn; const int32_t* cq;  // ragged batch (spa3d_set_counts): host arrays [B] of live support tracks / live queries per sample; null = all N / all Q
  const spa3d_scores* score;  // spa3d_score: per-track scores of every emitted query row, straight from the head (emit_scores); null everywhere else
  const float* w;  // train: the point weights [B,Q,T_out] (spa3d_set_point_weights; run() has checked their shape), addressed with the visibility targets' offsets; null = 1
  int nfold; const int32_t* fold_off;  // spa3d_score_folds: the F folds of every clip (host, [nfold + 1]; validated by the entry point); 0 / null everywhere else
};

namespace SPA_NS {
// the point-weight plane at a row offset (null stays null: no arithmetic on a null pointer)
static inline const float* at_rows(const float* w, int64_t off) { return w ? w + off : nullptr; }

// ---------------------------------------------------------------------------------------------
// weights as the kernels want them
// ---------------------------------------------------------------------------------------------
template <typename T> struct Lin {
  T* wn = nullptr;            // [K][N]  (dX = dY . wn^T reads it K'-contiguous)
  T* wt = nullptr;            // [N][K]  (Y = X . W with K contiguous)
  T* wpk = nullptr;           // K = 384: W as the row-stationary kernel's fragment stream (gemm_rs.hip); null = not built
  T* wpk_t = nullptr;         // N = 384 (one segment): W^T as that stream, for dX = dY . W^T
  T* wnb = nullptr;           // contraction >= 768: W as the large-register-tile NT kernel's fragment stream (gemm_ntb.hip); null = not built
  T* wnb_t = nullptr;         // W^T as that stream, for dX = dY . W^T (training only)
  const float* bias = nullptr;
  int K = 0, N = 0, nseg = 1, segw = 0;
  int64_t ldn = 0;            // row stride of wn (== N except for column sub-views of a fused matrix)
  const float* src[3] = {nullptr, nullptr, nullptr};  // f32 leaves [K][segw]
  float* gw[3] = {nullptr, nullptr, nullptr};         // f32 grads  [K][segw]
  float* gb = nullptr;
};
template <typename T> struct BlockW {
  int d = 0, mlp = 0, dkv = 0; bool cross = false;
  const float *norm_q, *norm_attn, *sq, *sk, *csq = nullptr, *csk = nullptr;
  float *g_norm_q, *g_norm_attn, *g_sq, *g_sk, *g_csq = nullptr, *g_csk = nullptr;
  Lin<T> qkv, out, cq, ckv, cout, mlp_in, mlp_out;
  T* mlp_pk = nullptr;  // both MLP kernels as the fused forward kernel's weight stream (mlp_fused.hip; d = 384, mlp = 1536, 16-bit modes)
  T* qkv_pk = nullptr;  // the q | k | v kernels as the per-head fragment stream of the fused projection + attention forward (qkv_attn.hip; d = 384, 96-wide heads)
};
template <typename T> struct XfW { std::vector<BlockW<T>> blocks; const float* norm_enc; float* g_norm_enc; int d; };
template <typename T> struct BlockStash {
  T *x, *nq, *qkv, *o, *a, *na, *hpre, *h, *cq = nullptr, *ckv = nullptr, *co = nullptr;
  float *st1, *st2, *lse = nullptr, *clse = nullptr;
  bool shared = false;  // Share mode: x / nq / st1 hold the SLOT rows (xU, LN1(xU) and its statistics), not the dense ones
};

// Readout block 1 (track_autoencoder_3d.py:276-285): rows 1.. of the sequence of query (b, q) depend on (b, query frame) only, so LayerNorm 1 and
// the QKV projection (forward, dW, dX, LN backward) run once per "slot" = distinct (sample, frame) pair and are expanded to / reduced
// from the per-query rows through the slot index (rows.hip "Shared latent rows"); the block's dx carries a slot's LN-backward term on
// the slot's first sequence only (consumers sum over the queries of a sample).  xU = [nslot * (S-1) latent rows | one row 0 per
// sequence].  Same values as the dense computation up to summation order (dqkv rows of a slot are pre-summed in fp32).
template <typename T> struct Share {
  const int32_t *slot = nullptr, *slot_b = nullptr, *slot_q0 = nullptr; int64_t nslot = 0; int Q = 0; const T* xU = nullptr;
  bool probe = false;  // workspace-sizing pass: run the dense path (the larger stash) and add the Share backward's transients on top
  int64_t rows(int64_t nseq, int S) const { return nslot * (S - 1) + nseq; }
};
constexpr double SHARE_MAX_FRAC = 0.45;  // Share is used when slots <= 45 % of the queries (above, its stash would exceed the dense one)

// Ragged (token-pruned) sequences of the track encoder: compact row offsets [nseq + 1] and the exact kept-row count; off == nullptr: dense.
// NT GEMMs run on the row count rounded up to 8 (the persistent kernels want M % 8 == 0; rows are independent there and every compact
// buffer carries the slack); reductions over rows (dW, LayerNorm, attention) use the exact count.
struct Rag { const int32_t* off = nullptr; int64_t rows = 0; };
// Cross attention of a leave-fold-out round (spa3d_score_folds): the nseq sequences share ONE key set of Nk rows and sequence i leaves out the rows
// [lo_i, hi_i) = entries 2i, 2i + 1 of host / dev (the same 2 nseq values on both sides)
struct Holes { const int32_t* host = nullptr; const int32_t* dev = nullptr; int Nk = 0; };

template <typename T> struct Net {
  spa3d_ctx* c; const spa3d_config& g; const float* P; float* G;
  std::map<std::string, int64_t> off;
  int H, Dh, E, NC; bool twoD;
  Lin<T> tok, dino, depth, comp, decomp, qenc, pred;
  T* emb_wt = nullptr; float* emb_bias = nullptr; int emb_K = 0;  // one-pass embedding: [d][K_sin + K_dino] weights (K contiguous) and b_tok + b_dino + b_depth
  XfW<T> enc, t2l, dec, ro;
  const float *lat0, *readout; float *g_lat0, *g_readout;
  void* zero_page = nullptr;

  Net(spa3d_ctx* c_, const float* P_, float* G_) : c(c_), g(c_->cfg), P(P_), G(G_) {
    for (auto& l : c->leaves) off[l.name] = l.offset;
    H = g.num_heads; Dh = g.qkv_size / H; E = g.qkv_size;
    twoD = g.model_kind == 1; NC = twoD ? 2 : 3;
  }
  template <typename U> U* alloc(int64_t n) { return (U*)c->ar.alloc(n * (int64_t)sizeof(U)); }
  void copy_dd(void* dst, const void* src, int64_t bytes) {  // device-to-device on the launch stream
    if (c->dry || bytes <= 0) return;
    if (hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess && !c->hip_err) { c->hip_err = -7; c->err = "packing a ragged chunk: device copy failed"; }
  }
  const float* p(const std::string& n) { return P + off.at(n); }
  float* gr(const std::string& n) { return G ? G + off.at(n) : nullptr; }

  Lin<T> make_lin(std::initializer_list<std::string> kernels, const std::string& bias, int K, int segw) {
    Lin<T> l; l.K = K; l.segw = segw; l.nseg = (int)kernels.size(); l.N = segw * l.nseg; l.ldn = l.N;
    int i = 0;
    for (auto& k : kernels) { l.src[i] = p(k); l.gw[i] = gr(k); ++i; }
    if (!bias.empty()) { l.bias = p(bias); l.gb = gr(bias); }
    l.wn = alloc<T>((int64_t)K * l.N); l.wt = alloc<T>((int64_t)K * l.N);
    for (int s = 0; s < l.nseg; ++s)
      k_pack<T>(c, l.src[s], segw, K, segw, l.wn + (int64_t)s * segw, l.N, l.wt + (int64_t)s * segw * K, K);
    if constexpr (sizeof(T) == 2) {
      const LinStreams ps = plan_lin_streams(c->gemm, K, l.N, segw, l.nseg, G != nullptr);
      if (ps.rs) {
        l.wpk = alloc<T>(gemm_rs_pack_elems(l.N));
        for (int s = 0; s < l.nseg; ++s) gemm_rs_pack<float>(c, l.src[s], segw, 1, segw, l.wpk + gemm_rs_pack_elems(segw) * s);
      }
      if (ps.rs_t) {  // element (k' = n, n' = k) of W^T is src[k * N + n]
        l.wpk_t = alloc<T>(gemm_rs_pack_elems(K));
        gemm_rs_pack<float>(c, l.src[0], 1, l.N, K, l.wpk_t);
      }
      if (ps.ntb) { l.wnb = alloc<T>(gemm_ntb_pack_elems(K, l.N)); gemm_ntb_pack<T>(c, l.wn, l.ldn, 1, K, l.N, l.wnb); }
      if (ps.ntb_t) { l.wnb_t = alloc<T>(gemm_ntb_pack_elems(l.N, K)); gemm_ntb_pack<T>(c, l.wn, 1, l.ldn, l.N, K, l.wnb_t); }
    }
    return l;
  }
  // columns [seg0*segw, (seg0+nseg)*segw) of a fused matrix as a Lin of its own (no bias)
  static Lin<T> sub_lin(const Lin<T>& l, int seg0, int nseg) {
    Lin<T> r = l; r.nseg = nseg; r.N = nseg * l.segw; r.bias = nullptr; r.gb = nullptr; r.wnb = nullptr; r.wnb_t = nullptr;
    r.wpk = l.wpk && gemm_rs_ok(l.K, r.N) ? l.wpk + gemm_rs_pack_elems(l.segw) * seg0 : nullptr;  // the stream is column-segment-major
    r.wn = l.wn + (int64_t)seg0 * l.segw; r.wt = l.wt + (int64_t)seg0 * l.segw * l.K;
    for (int i = 0; i < 3; ++i) { r.src[i] = i < nseg ? l.src[seg0 + i] : nullptr; r.gw[i] = i < nseg ? l.gw[seg0 + i] : nullptr; }
    return r;
  }
  XfW<T> make_xf(const std::string& name, int d, int mlp, int L, int kv) {
    XfW<T> x; x.d = d;
    for (int i = 0; i < L; ++i) {
      std::string b = name + "/layer_" + std::to_string(i);
      BlockW<T> w; w.d = d; w.mlp = mlp; w.cross = kv > 0; w.dkv = kv;
      w.norm_q = p(b + "/norm_q/scale"); w.g_norm_q = gr(b + "/norm_q/scale");
      w.norm_attn = p(b + "/norm_attn/scale"); w.g_norm_attn = gr(b + "/norm_attn/scale");
      std::string s = b + "/self_att";
      w.qkv = make_lin({s + "/dense_query/kernel", s + "/dense_key/kernel", s + "/dense_value/kernel"}, "", d, E);
      w.sq = p(s + "/norm_query/scale"); w.g_sq = gr(s + "/norm_query/scale");
      w.sk = p(s + "/norm_key/scale"); w.g_sk = gr(s + "/norm_key/scale");
      w.out = make_lin({s + "/dense_out/kernel"}, s + "/dense_out/bias", E, d);
      if (kv) {
        std::string x2 = b + "/cross_att";
        w.cq = make_lin({x2 + "/dense_query/kernel"}, "", d, E);
        w.ckv = make_lin({x2 + "/dense_key/kernel", x2 + "/dense_value/kernel"}, "", kv, E);
        w.csq = p(x2 + "/norm_query/scale"); w.g_csq = gr(x2 + "/norm_query/scale");
        w.csk = p(x2 + "/norm_key/scale"); w.g_csk = gr(x2 + "/norm_key/scale");
        w.cout = make_lin({x2 + "/dense_out/kernel"}, x2 + "/dense_out/bias", E, d);
      }
      w.mlp_in = make_lin({b + "/MLP_in/kernel"}, b + "/MLP_in/bias", d, mlp);
      w.mlp_out = make_lin({b + "/MLP_out/kernel"}, b + "/MLP_out/bias", mlp, d);
      if constexpr (sizeof(T) == 2) {
        if (plan_mlp_pack(c->gemm, w.cross, d, mlp)) {
          w.mlp_pk = alloc<T>(mlp_fused_pack_elems());
          mlp_fused_pack<float>(c, w.mlp_in.src[0], w.mlp_out.src[0], w.mlp_pk);
        }
        if (plan_qkv_pack(c->attn, c->gemm.generic, w.cross, d, Dh)) {
          w.qkv_pk = alloc<T>(qkv_attn_pack_elems(H));
          qkv_attn_pack<float>(c, w.qkv.src[0], w.qkv.src[1], w.qkv.src[2], E, H, w.qkv_pk);
        }
      }
      x.blocks.push_back(w);
    }
    x.norm_enc = p(name + "/norm_encoder/scale"); x.g_norm_enc = gr(name + "/norm_encoder/scale");
    return x;
  }
  // builds all shadows at the current arena position (re-done every call: 0.9 GB of traffic, << 1 ms)
  void pack() {
    zero_page = c->ar.alloc(256); k_zero(c, zero_page, 256);
    const int d = g.track_token_dim, dl = g.encoder_latent_dim, dd = g.decoder_num_channels, nf = g.num_frequencies;
    lat0 = p("initializer/state_init"); g_lat0 = gr("initializer/state_init");
    readout = nullptr; g_readout = nullptr;
    if (!twoD) { readout = p("input_readout_token/state_init"); g_readout = gr("input_readout_token/state_init"); }
    tok = make_lin({"track_token_projection/kernel"}, "track_token_projection/bias", (NC + 1) * 2 * nf, d);
    if (g.dino_feature_dim > 0) dino = make_lin({"dino_projection/kernel"}, "dino_projection/bias", g.dino_feature_dim, d);
    if (g.depth_feature_dim > 0) depth = make_lin({"depth_projection/kernel"}, "depth_projection/bias", g.depth_feature_dim, d);
    if constexpr (sizeof(T) == 2) {
      if (plan_embed_pack(c->gemm, twoD, d, tok.K, g.dino_feature_dim, g.depth_feature_dim)) {
        emb_K = tok.K + (g.dino_feature_dim > 0 ? dino.K : 0);
        emb_wt = alloc<T>((int64_t)d * emb_K); emb_bias = alloc<float>(d);
        k_pack<T>(c, tok.src[0], d, tok.K, d, nullptr, 0, emb_wt, emb_K);
        if (g.dino_feature_dim > 0) k_pack<T>(c, dino.src[0], d, dino.K, d, nullptr, 0, emb_wt + tok.K, emb_K);
        k_sum3(c, tok.bias, g.dino_feature_dim > 0 ? dino.bias : nullptr, g.depth_feature_dim > 0 ? depth.bias : nullptr, emb_bias, d);
      }
    }
    enc = make_xf("input_track_transformer", d, g.enc_mlp, g.enc_layers, 0);
    t2l = make_xf("tracks_to_latents", dl, g.t2l_mlp, g.t2l_layers, d);
    comp = make_lin({"compressor/kernel"}, "compressor/bias", dl, g.latent_token_dim);
    decomp = make_lin({"decompressor/kernel"}, "decompressor/bias", g.latent_token_dim, dd - 128);
    dec = make_xf("decompress_attn", dd - 128, g.dec_mlp, g.dec_layers, 0);
    ro = make_xf("track_readout_attn", dd, g.ro_mlp, g.ro_layers, 0);
    qenc = make_lin({"query_encoder/kernel"}, "query_encoder/bias", (NC * 2 * nf + 1) * 2 * nf, dd);
    pred = make_lin({"track_predictor/kernel"}, "track_predictor/bias", dd, 4 * g.num_output_frames);
  }

  // ------------------------------------------------------------------ GEMM front ends: plan (gemm_plan.hpp), then launch (nothing when dry)
  GemmKernel plan(const GemmDesc& d) const { return sizeof(T) == 2 ? plan_gemm(d, c->gemm) : GemmKernel::Generic; }
  void gemm(const GemmDesc& d) { gemm_launch<T>(c, d, plan(d)); }
  // Y[M,N] = epi(X[M,K] W + b) (+ residual)
  void lin_fwd(const Lin<T>& l, const T* X, void* Y, int64_t M, int epi = EPI_NONE, const T* residual = nullptr, int out_f32 = 0,
               int accumulate = 0, int64_t ldx = 0, int64_t ldy = 0, int crow_group = 0, int crow_skip = 0, T* pre_out = nullptr) {
    GemmDesc d{};
    d.A = X; d.B = l.wn; d.C = Y; d.M = M; d.N = l.N; d.K = l.K;
    d.sAm = ldx ? ldx : l.K; d.sAk = 1; d.sBk = l.ldn; d.sBn = 1; d.sCm = ldy ? ldy : l.N;
    d.Bt = l.wt; d.ldBt = l.K; d.rs_pk = l.wpk; d.ntb_pk = l.wnb;
    d.crow_group = crow_group; d.crow_skip = crow_skip; d.pre_out = pre_out;
    d.bias = l.bias; d.epi = epi; d.aux = residual; d.out_f32 = out_f32; d.accumulate = accumulate;
    gemm(d);
  }
  // dX[M,K] (op)= dY[M,N] W^T, optionally * gelu'(pre)
  void lin_bwd_x(const Lin<T>& l, const T* dY, T* dX, int64_t M, const T* gelu_pre = nullptr, int accumulate = 0, int64_t lddx = 0) {
    GemmDesc d{};
    d.A = dY; d.B = l.wn; d.C = dX; d.M = M; d.N = l.K; d.K = l.N;
    d.sAm = l.N; d.sAk = 1; d.sBk = 1; d.sBn = l.ldn; d.sCm = lddx ? lddx : l.K;
    d.Bt = l.wn; d.ldBt = l.ldn; d.rs_pk = l.wpk_t; d.ntb_pk = l.wnb_t;
    if (gelu_pre) { d.epi = EPI_MUL_GELU_GRAD; d.aux = gelu_pre; }
    d.accumulate = accumulate;
    gemm(d);
  }
  // gw += X^T dY ; gb += colsum(dY)
  void lin_bwd_w(const Lin<T>& l, const T* X, const T* dY, int64_t M, int64_t ldx = 0, int brow_group = 0, int brow_skip = 0) {
    if constexpr (sizeof(T) == 2) {
      // fused projections (q | k | v): ONE dW GEMM over all segments -- X is read once instead of once per segment, a third of the launches --
      // with the output tiles routed to the segments' separate leaves (8-phase TN kernels; else the per-segment loop below)
      if (l.nseg > 1 && !l.gb && l.gw[0]) {
        GemmDesc d{};
        d.A = X; d.B = dY; d.C = l.gw[0]; d.M = l.K; d.N = l.N; d.K = M;
        d.sAm = 1; d.sAk = ldx ? ldx : l.K; d.sBk = l.N; d.sBn = 1; d.sCm = l.segw;
        d.out_f32 = 1; d.accumulate = 1; d.zero_page = zero_page; d.brow_group = brow_group; d.brow_skip = brow_skip;
        d.seg_n = l.segw; d.C_seg[0] = l.gw[1]; d.C_seg[1] = l.nseg > 2 ? l.gw[2] : nullptr;
        const GemmKernel k = plan_tn(d, c->gemm);
        if (k != GemmKernel::Refuse) { gemm_launch<T>(c, d, k); return; }
      }
    }
    for (int s = 0; s < l.nseg; ++s) {
      GemmDesc d{};
      d.A = X; d.B = dY + (int64_t)s * l.segw; d.C = l.gw[s]; d.M = l.K; d.N = l.segw; d.K = M;
      d.sAm = 1; d.sAk = ldx ? ldx : l.K; d.sBk = l.N; d.sBn = 1; d.sCm = l.segw;
      d.out_f32 = 1; d.accumulate = 1; d.zero_page = zero_page; d.brow_group = brow_group; d.brow_skip = brow_skip;
      d.colsum_out = l.gb ? l.gb + (int64_t)s * l.segw : nullptr;  // bias gradient rides along in the 8-phase and large-tile dW kernels
      const GemmKernel k = plan(d);
      gemm_launch<T>(c, d, k);
      if (l.gb && !gemm_tn_fuses_colsum(k, d)) k_colsum<T>(c, dY + (int64_t)s * l.segw, M, l.segw, l.N, l.gb + (int64_t)s * l.segw, brow_group, brow_skip);
    }
  }

  // ------------------------------------------------------------------ attention core (attention.hip): the descriptors of a block's two attentions
  // qkv [rows][3 E] = q | k | v; the backward adds d_o and dqkv in qkv's layout.  rg: ragged rows after token pruning
  AttnDesc self_desc(const BlockW<T>& w, const T* qkv, T* o, float* lse, const float* km, int64_t nseq, int S, const Rag& rg, const T* d_o = nullptr,
                     T* dqkv = nullptr) {
    AttnDesc a;
    a.q = qkv; a.k = qkv + E; a.v = qkv + 2 * E; a.ldq = a.ldk = a.ldv = 3 * E; a.sq = w.sq; a.sk = w.sk; a.km = km; a.o = o; a.lse = lse;
    a.nseq = nseq; a.Sq = a.Sk = S; a.H = H; a.Dh = Dh; a.esz = (int)sizeof(T);
    if (rg.off) { a.layout = AttnLayout::RaggedRows; a.seq_off = rg.off; a.total_rows = rg.rows; }
    if (d_o) { a.d_o = d_o; a.dq = dqkv; a.dk = dqkv + E; a.dv = dqkv + 2 * E; a.dsq = w.g_sq; a.dsk = w.g_sk; }
    return a;
  }
  // cq [rows][E], ckv [keys][2 E] = k | v: Skv keys per sequence, or ragged key sets (koff_h / koff_d), or one shared key set with a hole per sequence (hl)
  AttnDesc cross_desc(const BlockW<T>& w, const T* cq, const T* ckv, T* co, float* clse, int64_t nseq, int S, int Skv, const int32_t* koff_h,
                      const int32_t* koff_d, const Holes* hl, const T* d_o = nullptr, T* dcq = nullptr, T* dckv = nullptr) {
    AttnDesc a;
    a.q = cq; a.k = ckv; a.v = ckv + E; a.ldq = E; a.ldk = a.ldv = 2 * E; a.sq = w.csq; a.sk = w.csk; a.o = co; a.lse = clse;
    a.nseq = nseq; a.Sq = S; a.Sk = Skv; a.H = H; a.Dh = Dh; a.esz = (int)sizeof(T);
    if (hl) { a.layout = AttnLayout::Hole; a.holes_host = hl->host; a.holes_dev = hl->dev; a.Nk = hl->Nk; }
    else if (koff_h) { a.layout = AttnLayout::RaggedKeys; a.koff_host = koff_h; a.koff_dev = koff_d; }
    if (d_o) { a.d_o = d_o; a.dq = dcq; a.dk = dckv; a.dv = dckv + E; a.dsq = w.g_csq; a.dsk = w.g_csk; }
    return a;
  }

  // ------------------------------------------------------------------ ImprovedTransformerBlock (attention.py:67-108)
  // koff_h / koff_d (host / device, [nseq + 1]): cross attention against RAGGED key sets -- sequence i attends rows [koff[i], koff[i + 1]) of kv
  void block_fwd(const BlockW<T>& w, const T* x, T* y, int64_t nseq, int S, const float* km, const T* kv, int Skv, BlockStash<T>* st,
                 const Rag& rg = Rag(), const Share<T>* sh = nullptr, const int32_t* koff_h = nullptr, const int32_t* koff_d = nullptr,
                 const Holes* hl = nullptr) {  // hl: cross attention against ONE shared key set of hl->Nk rows of kv, a hole per sequence (forward only)
    const int64_t M = rg.off ? rg.rows : nseq * S, Mg = rg.off ? (M + 7) & ~int64_t(7) : M; const int d = w.d;  // Mg: NT-GEMM rows (see Rag)
    int64_t mk = c->ar.mark();
    T *nq, *qkv; float* st1;
    if (sh && sh->probe) sh = nullptr;
    if (sh) {  // LN1 + QKV once per slot row, then expanded to the per-query rows the attention kernel reads
      const int64_t MU = sh->rows(nseq, S), MUg = (MU + 7) & ~int64_t(7);
      nq = alloc<T>(MUg * d); st1 = alloc<float>(MU * 2);
      k_layernorm<T>(c, sh->xU, w.norm_q, nq, st1, MU, d);
      qkv = alloc<T>(Mg * 3 * E);
      const int64_t mk2 = c->ar.mark();
      T* qkvU = alloc<T>(MUg * 3 * E);
      lin_fwd(w.qkv, nq, qkvU, MUg);
      k_share_expand<T>(c, qkvU, sh->slot, sh->slot_q0, sh->nslot, nseq, S, 3 * E, nullptr, qkv);
      c->ar.release(mk2);
    } else {
      nq = alloc<T>(Mg * d); st1 = alloc<float>(M * 2);
      k_layernorm<T>(c, x, w.norm_q, nq, st1, M, d);                                    // :76-78
      qkv = alloc<T>(Mg * 3 * E);
    }
    T* o = alloc<T>(Mg * E); float* lse = alloc<float>(M * H * 2);
    AttnDesc sa = self_desc(w, qkv, o, lse, km, nseq, S, rg);
    if (!sh) { sa.x = nq; sa.ldx = d; sa.d = d; sa.qkv_pk = w.qkv_pk; }
    // :154-175 as ONE kernel per (sequence, head): q | k | v are written once and never read back by the forward (opt-in: attn_impl 6)
    const AttnPlan qa = plan_qkv_attn(sa, c->attn);
    if (qa.kernel == AttnKernel::QkvFwd) attn_launch(c, sa, qa);
    else {
      if (!sh) lin_fwd(w.qkv, nq, qkv, Mg);                                              // :154-173
      attention_fwd<T>(c, sa);                                                           // :166-175
    }
    T* a = alloc<T>(Mg * d);
    lin_fwd(w.out, o, a, Mg, EPI_NONE, x);                                              // :178-183 + residual :79,90
    T *cq = nullptr, *ckv = nullptr, *co = nullptr; float* clse = nullptr;
    if (w.cross) {                                                                      // :92-100
      cq = alloc<T>(M * E); lin_fwd(w.cq, nq, cq, M);
      const int64_t nkv = hl ? hl->Nk : (koff_h ? koff_h[nseq] : nseq * Skv);  // (shared keys: projected ONCE, not per sequence)
      ckv = alloc<T>(nkv * 2 * E); lin_fwd(w.ckv, kv, ckv, nkv);
      co = alloc<T>(M * E); clse = alloc<float>(M * H * 2);
      attention_fwd<T>(c, cross_desc(w, cq, ckv, co, clse, nseq, S, Skv, koff_h, koff_d, hl));
      lin_fwd(w.cout, co, a, M, EPI_NONE, a);
    }
    T* na = alloc<T>(Mg * d); float* st2 = alloc<float>(Mg * 2);
    k_layernorm<T>(c, a, w.norm_attn, na, st2, M, d);                                   // :103-105
    T* hpre = alloc<T>(Mg * w.mlp); T* h = alloc<T>(Mg * w.mlp);
    bool fused = false;
    if constexpr (sizeof(T) == 2) {  // :103-108 as one sequence-resident kernel (track encoder widths): h is never read back from HBM
      fused = plan_mlp(c->gemm, Mg, d, w.mlp, w.mlp_pk, w.mlp_in.bias, w.mlp_out.bias, na, a, y, h, hpre) == GemmKernel::MlpFused;
      if (fused && !c->dry) mlp_fused_fwd(c, na, a, y, h, hpre, Mg, w.mlp_pk, w.mlp_in.bias, w.mlp_out.bias);
    }
    if (!fused) {
      lin_fwd(w.mlp_in, na, h, Mg, EPI_GELU, nullptr, 0, 0, 0, 0, 0, 0, hpre);           // :106  h = gelu(hpre), both kept for the backward
      lin_fwd(w.mlp_out, h, y, Mg, EPI_NONE, a);                                         // :107-108
    }
    if (st) { st->x = const_cast<T*>(sh ? sh->xU : x); st->nq = nq; st->qkv = qkv; st->o = o; st->a = a; st->na = na; st->hpre = hpre; st->h = h;
              st->st1 = st1; st->st2 = st2; st->cq = cq; st->ckv = ckv; st->co = co; st->lse = lse; st->clse = clse; st->shared = sh != nullptr; }
    else c->ar.release(mk);
  }
  // dy -> dx (dx may alias dy); dkv accumulated (T) if cross
  void block_bwd(const BlockW<T>& w, const BlockStash<T>& s, const T* dy, T* dx, int64_t nseq, int S, const float* km, const T* kv,
                 int Skv, T* dkv, const Rag& rg = Rag(), const Share<T>* sh = nullptr, const int32_t* koff_h = nullptr, const int32_t* koff_d = nullptr) {
    const int64_t M = rg.off ? rg.rows : nseq * S, Mg = rg.off ? (M + 7) & ~int64_t(7) : M; const int d = w.d;
    int64_t mk = c->ar.mark();
    lin_bwd_w(w.mlp_out, s.h, dy, M);
    T* dh = alloc<T>(Mg * w.mlp);  // dh = dy Wout^T * gelu'(hpre)
    lin_bwd_x(w.mlp_out, dy, dh, Mg, s.hpre);
    lin_bwd_w(w.mlp_in, s.na, dh, M);
    T* dna = alloc<T>(Mg * d);
    lin_bwd_x(w.mlp_in, dh, dna, Mg);
    T* da = alloc<T>(Mg * d);
    k_layernorm_bwd<T>(c, s.a, w.norm_attn, s.st2, dna, da, w.g_norm_attn, M, d, dy);  // da = dy + LNbwd
    T* dnq = dna;  // reuse
    // self attention
    lin_bwd_w(w.out, s.o, da, M);
    T* d_o = alloc<T>(Mg * E);
    lin_bwd_x(w.out, da, d_o, Mg);
    T* dqkv = alloc<T>(Mg * 3 * E);
    attention_bwd<T>(c, self_desc(w, s.qkv, s.o, s.lse, km, nseq, S, rg, d_o, dqkv));
    if (sh && sh->probe) {  // sizing pass: the Share branch's transients at its largest admissible slot count, then the dense path
      const int64_t MUg = (sh->rows(nseq, S) + 7) & ~int64_t(7), mk2 = c->ar.mark();
      (void)alloc<T>(MUg * 3 * E); (void)alloc<T>(MUg * d); (void)alloc<T>(MUg * d);
      c->ar.release(mk2);
      sh = nullptr;
    }
    if (sh) {  // slot rows: dqkv pre-summed per slot, then dW / dX / LN1 backward on the slot rows and dx = da + expansion
      const int64_t MU = sh->rows(nseq, S), MUg = (MU + 7) & ~int64_t(7);
      T* dqkvU = alloc<T>(MUg * 3 * E);
      k_share_reduce<T>(c, dqkv, sh->slot, sh->slot_b, sh->nslot, nseq, sh->Q, S, 3 * E, dqkvU);
      lin_bwd_w(w.qkv, s.nq, dqkvU, MU);
      T* dnU = alloc<T>(MUg * d);
      lin_bwd_x(w.qkv, dqkvU, dnU, MUg);
      T* dxU = alloc<T>(MU * d);
      k_layernorm_bwd<T>(c, s.x, w.norm_q, s.st1, dnU, dxU, w.g_norm_q, MU, d, nullptr);
      k_share_expand<T>(c, dxU, sh->slot, sh->slot_q0, sh->nslot, nseq, S, d, da, dx);
      c->ar.release(mk);
      return;
    }
    lin_bwd_w(w.qkv, s.nq, dqkv, M);
    lin_bwd_x(w.qkv, dqkv, dnq, Mg);
    if (w.cross) {
      lin_bwd_w(w.cout, s.co, da, M);
      lin_bwd_x(w.cout, da, d_o, M);  // d_o := d co
      T* dcq = dqkv;                  // reuse [M,E]
      const int64_t nkv = koff_h ? koff_h[nseq] : nseq * Skv;
      T* dckv = alloc<T>(nkv * 2 * E);
      attention_bwd<T>(c, cross_desc(w, s.cq, s.ckv, s.co, s.clse, nseq, S, Skv, koff_h, koff_d, nullptr, d_o, dcq, dckv));
      // the backward writes dq with stride ldq = E into dcq: dense [M,E]
      lin_bwd_w(w.cq, s.nq, dcq, M);
      lin_bwd_x(w.cq, dcq, dnq, M, nullptr, 1);
      lin_bwd_w(w.ckv, kv, dckv, nkv);
      lin_bwd_x(w.ckv, dckv, dkv, nkv, nullptr, 1);
    }
    k_layernorm_bwd<T>(c, s.x, w.norm_q, s.st1, dnq, dx, w.g_norm_q, M, d, da);  // dx = da + LNbwd
    c->ar.release(mk);
  }


  // ------------------------------------------------------------------ last block of a stack whose output is token 0 only
  // (track_autoencoder_3d.py:187-188, 286).  K/V (and LN1) still cover every token; the query, attention output,
  // out-projection, LN2 and MLP are needed for row 0 of each sequence only: 25 % of a full block's GEMM work.
  struct LastStash { T *x, *nq, *kv, *q0, *o0, *x0, *a0, *na0, *hpre0, *h0, *nq0 = nullptr; float *st1, *st2, *p0; };
  void block_fwd_last(const BlockW<T>& w, const T* x, T* y0, int64_t nseq, int S, const float* km, LastStash* st, const Rag& rg = Rag()) {
    const int64_t M = rg.off ? rg.rows : nseq * S, Mg = rg.off ? (M + 7) & ~int64_t(7) : M; const int d = w.d;
    const int64_t mk = c->ar.mark();
    const Lin<T> wq = sub_lin(w.qkv, 0, 1), wkv = sub_lin(w.qkv, 1, 2);
    T* nq = alloc<T>(Mg * d); float* st1 = alloc<float>(M * 2);
    k_layernorm<T>(c, x, w.norm_q, nq, st1, M, d);
    T* kv = alloc<T>(Mg * 2 * E);
    lin_fwd(wkv, nq, kv, Mg);
    T* q0 = alloc<T>(nseq * E); T* nq0 = nullptr;
    if (rg.off) {  // rows 0 of the ragged sequences sit at seq_off[i]
      nq0 = alloc<T>(nseq * d);
      k_rows_idx<T>(c, 0, nq, rg.off, nq0, nseq, d);
      lin_fwd(wq, nq0, q0, nseq);
    } else {
      lin_fwd(wq, nq, q0, nseq, EPI_NONE, nullptr, 0, 0, (int64_t)S * d);          // rows 0 of every sequence
    }
    T* o0 = alloc<T>(nseq * E); float* p0 = alloc<float>(nseq * H * S);
    k_attn_q1_fwd<T>(c, q0, E, kv, kv + E, 2 * E, 2 * E, w.sq, w.sk, km, nseq, S, H, Dh, o0, p0, rg.off);
    T* x0 = alloc<T>(nseq * d);
    if (rg.off) k_rows_idx<T>(c, 0, x, rg.off, x0, nseq, d); else k_gather_rows<T>(c, x, S, x0, nseq, d);
    T* a0 = alloc<T>(nseq * d);
    lin_fwd(w.out, o0, a0, nseq, EPI_NONE, x0);
    T* na0 = alloc<T>(nseq * d); float* st2 = alloc<float>(nseq * 2);
    k_layernorm<T>(c, a0, w.norm_attn, na0, st2, nseq, d);
    T* hpre0 = alloc<T>(nseq * w.mlp); T* h0 = alloc<T>(nseq * w.mlp);
    lin_fwd(w.mlp_in, na0, h0, nseq, EPI_GELU, nullptr, 0, 0, 0, 0, 0, 0, hpre0);
    lin_fwd(w.mlp_out, h0, y0, nseq, EPI_NONE, a0);
    if (st) { st->x = const_cast<T*>(x); st->nq = nq; st->kv = kv; st->q0 = q0; st->o0 = o0; st->x0 = x0; st->a0 = a0; st->na0 = na0;
              st->hpre0 = hpre0; st->h0 = h0; st->st1 = st1; st->st2 = st2; st->p0 = p0; st->nq0 = nq0; }
    else c->ar.release(mk);
  }
  // dy0 [nseq,d] -> dx [rows of the stack input, d]
  void block_bwd_last(const BlockW<T>& w, const LastStash& s, const T* dy0, T* dx, int64_t nseq, int S, const float* km, const Rag& rg = Rag()) {
    const int64_t M = rg.off ? rg.rows : nseq * S, Mg = rg.off ? (M + 7) & ~int64_t(7) : M; const int d = w.d;
    const int64_t mk = c->ar.mark();
    const Lin<T> wq = sub_lin(w.qkv, 0, 1), wkv = sub_lin(w.qkv, 1, 2);
    lin_bwd_w(w.mlp_out, s.h0, dy0, nseq);
    T* dh = alloc<T>(nseq * w.mlp);
    lin_bwd_x(w.mlp_out, dy0, dh, nseq, s.hpre0);
    lin_bwd_w(w.mlp_in, s.na0, dh, nseq);
    T* dna = alloc<T>(nseq * d);
    lin_bwd_x(w.mlp_in, dh, dna, nseq);
    T* da0 = alloc<T>(nseq * d);
    k_layernorm_bwd<T>(c, s.a0, w.norm_attn, s.st2, dna, da0, w.g_norm_attn, nseq, d, dy0);
    lin_bwd_w(w.out, s.o0, da0, nseq);
    T* d_o0 = alloc<T>(nseq * E);
    lin_bwd_x(w.out, da0, d_o0, nseq);
    T* dq0 = alloc<T>(nseq * E); T* dkv = alloc<T>(Mg * 2 * E);
    k_attn_q1_bwd<T>(c, s.q0, E, s.kv, s.kv + E, 2 * E, 2 * E, w.sq, w.sk, km, nseq, S, H, Dh, s.p0, d_o0, dq0, dkv, dkv + E, w.g_sq, w.g_sk,
                     rg.off);
    lin_bwd_w(wkv, s.nq, dkv, M);
    T* dnq = alloc<T>(Mg * d);
    lin_bwd_x(wkv, dkv, dnq, Mg);
    if (rg.off) {
      lin_bwd_w(wq, s.nq0, dq0, nseq);
      T* dnq0 = alloc<T>(nseq * d);
      lin_bwd_x(wq, dq0, dnq0, nseq);
      k_rows_idx<T>(c, 2, dnq0, rg.off, dnq, nseq, d);                             // += into rows 0
    } else {
      lin_bwd_w(wq, s.nq, dq0, nseq, (int64_t)S * d);
      lin_bwd_x(wq, dq0, dnq, nseq, nullptr, 1, (int64_t)S * d);                  // += into rows 0
    }
    k_layernorm_bwd<T>(c, s.x, w.norm_q, s.st1, dnq, dx, w.g_norm_q, M, d, nullptr);
    if (rg.off) k_rows_idx<T>(c, 2, da0, rg.off, dx, nseq, d);                     // residual path of token 0
    else k_add_rows_strided<T>(c, dx, da0, S, nseq, d);
    c->ar.release(mk);
  }

  // ------------------------------------------------------------------ per-chunk state
  struct Chunk {
    int64_t Bc, nseq; int N, Q, T_, S;
    // intra-sample slices (run_chunk: "track_chunk" / "query_chunk", one sample per chunk): the track encoder runs on tracks [n_off, n_off + Nc) of the
    // sample (nseq = Bc * Nc; the cross attention of tracks_to_latents still sees all N), the readout on queries [q_off, q_off + Qc)
    bool ragged = false;  // sample(s) of a batch with per-sample counts (spa3d_set_counts)
    // packed: a chunk of SEVERAL samples of such a batch.  Their live tracks / queries are packed back to back -- the track encoder runs on
    // nseq = noff[Bc] sequences, the readout on qoff[Bc] -- and only the cheap per-sample kernels (key mask, sequence assembly, loss) loop over the samples
    bool packed = false; std::vector<int32_t> noff, qoff; int32_t* koff_dev = nullptr;
    // folds: ONE clip as F pseudo-samples (run_folds, spa3d_score_folds).  The track encoder runs once over the clip in place (Bc = 1); the latent stacks run
    // with Bc = F on the shared encoder rows, sequence f leaving out the rows holes_h[2f], holes_h[2f + 1]; the readout runs over a group of consecutive folds
    // as a packed chunk whose queries are rows [q_off, q_off + qoff[Bc]) of the clip IN PLACE (no packed copy) and read the latents of folds lat_f0, lat_f0 + 1, ..
    bool folds = false; std::vector<int32_t> holes_h; int32_t* holes_dev = nullptr; int lat_f0 = 0;
    int64_t nq() const { return packed ? (int64_t)qoff.back() : Bc * Qc; }
    // Which rows of the batch's [B * Q] query rows are the chunk's nq() query rows: f(chunk_row0, batch_row0, n, sample) once for the whole chunk
    // when its rows are consecutive in the batch (a uniform chunk, one ragged sample in place, a group of folds), else once per sample of the packed
    // chunk -- its live rows are the first of its Q (a sample without live queries gets its call too, with n = 0).  b0: the chunk's first sample.
    template <typename F> void for_each_query_span(int64_t b0, F&& f) const {
      if (!packed || folds) { f((int64_t)0, b0 * Q + q_off, nq(), (int64_t)0); return; }
      for (int64_t s = 0; s < Bc; ++s) f((int64_t)qoff[s], (b0 + s) * Q, (int64_t)(qoff[s + 1] - qoff[s]), s);
    }
    int Nk = 0;  // keys of the tracks_to_latents cross attention per sample: N, or the sample's live support tracks in a ragged batch
    int64_t n_off = 0, q_off = 0; int Nc = 0, Qc = 0; bool count_plan = true;  // count_plan: false for the backward's recompute (spa3d_plan_stats counts pass A only)
    // encoder
    T* sinbuf; const void* dino; const void* depthf; float* km; T* tok0; std::vector<BlockStash<T>> enc_st; T* enc_last; T* r0; float* st_r0;
    T* enc_out; LastStash enc_lst, ro_lst; T* enc_ln_all = nullptr; float* st_all = nullptr; const float* sup_vis = nullptr;
    Rag enc_rg; int32_t* row_src = nullptr;  // token pruning of the track encoder (encode_tracks)
    // t2l
    T* lat_in; std::vector<BlockStash<T>> t2l_st; T* t2l_last; float* st_t2l; T* t2l_n; float* latents;  // [Bc,L,Ld] f32
    // decode
    float* clipmask; float* lat_q; T* lat_qT; T* dec_in; std::vector<BlockStash<T>> dec_st; T* dec_last; float* st_dec; T* latd;
    float* feat; int32_t* qframe; T* sin2; T* qtok; T* seq0; Share<T> ro_sh; bool ro_share = false; std::vector<BlockStash<T>> ro_st; T* ro_last; T* q0; float* st_q0; T* q0n;
    float* head;
  };

  // E1-E7 (track_autoencoder_3d.py:123-188; with encode_latents: -204) on tracks [k.n_off, k.n_off + k.Nc) of samples [b0, b0 + k.Bc) -> k.enc_out [nseq, d] (written to enc_dst when given, else allocated here)
  void encode_tracks(Chunk& k, const spa3d_batch* b, int64_t b0, bool train, T* enc_dst = nullptr) {
    const int d = g.track_token_dim, nf = g.num_frequencies, T_ = k.T_, S = k.S;
    const int64_t nseq = k.nseq, trk0 = b0 * k.N + k.n_off;  // first track row of the slice (tracks of a sample chunk are contiguous when Nc < N: Bc = 1)
    const float* tracks = b->support_tracks + trk0 * T_ * NC;
    k.sup_vis = b->support_tracks_visible + trk0 * T_;
    const bool want_dino = !twoD && g.dino_feature_dim > 0 && b->dino_features, want_depth = !twoD && g.depth_feature_dim > 0 && b->depth_features;
    const T* dino_in = want_dino ? (const T*)b->dino_features + trk0 * T_ * g.dino_feature_dim : nullptr;
    const T* depth_in = want_depth ? (const T*)b->depth_features + trk0 * T_ * g.depth_feature_dim : nullptr;
    if (k.packed) {  // the live tracks of the chunk's samples, back to back (each sample's are the first rows of its slice: one copy per sample and tensor)
      float* pt = alloc<float>(nseq * T_ * NC); float* pv = alloc<float>(nseq * T_);
      T* pd = want_dino ? alloc<T>(nseq * T_ * g.dino_feature_dim) : nullptr; T* pz = want_depth ? alloc<T>(nseq * T_ * g.depth_feature_dim) : nullptr;
      for (int64_t s = 0; s < k.Bc; ++s) {
        const int64_t src = (b0 + s) * k.N * T_, dst = (int64_t)k.noff[s] * T_, n = (int64_t)(k.noff[s + 1] - k.noff[s]) * T_;
        copy_dd(pt + dst * NC, b->support_tracks + src * NC, n * NC * 4);
        copy_dd(pv + dst, b->support_tracks_visible + src, n * 4);
        if (pd) copy_dd(pd + dst * g.dino_feature_dim, (const T*)b->dino_features + src * g.dino_feature_dim, n * g.dino_feature_dim * (int64_t)sizeof(T));
        if (pz) copy_dd(pz + dst * g.depth_feature_dim, (const T*)b->depth_features + src * g.depth_feature_dim, n * g.depth_feature_dim * (int64_t)sizeof(T));
      }
      tracks = pt; k.sup_vis = pv; dino_in = pd; depth_in = pz;
    }
    // embed stage (3d:123-165) as one profile class: algorithmic bytes = what a single pass would move (xyz f32 + visibility + the 16-bit
    // dino / depth planes in, the kept token rows out); FLOPs of its projections
    ProfScope* eps = nullptr;
    {
      const double rows_in = (double)nseq * T_, kin = (double)(NC + 1) * 2 * nf + (b->dino_features ? g.dino_feature_dim : 0) + (b->depth_features ? g.depth_feature_dim : 0);
      const double by = rows_in * (NC * 4.0 + 4.0 + ((b->dino_features ? g.dino_feature_dim : 0) + (b->depth_features ? g.depth_feature_dim : 0)) * (double)sizeof(T)) + rows_in * d * (double)sizeof(T);
      eps = new ProfScope(c, PROF_EMBED, 2.0 * rows_in * kin * d, by);
    }
    k.sinbuf = alloc<T>(nseq * T_ * (NC + 1) * 2 * nf);
    k_embed_tokens<T>(c, tracks, nseq * T_, T_, nf, g.track_scale_factor, k.sinbuf, NC);             // 3d:126-134 / ta:186-199
    k.km = alloc<float>(nseq * S);
    if (k.packed) {  // boundary_frame is per sample
      for (int64_t s = 0; s < k.Bc; ++s) {
        const int n = k.noff[s + 1] - k.noff[s];
        k_keymask(c, k.sup_vis + (int64_t)k.noff[s] * T_, b->boundary_frame + b0 + s, n, n, T_, k.km + (int64_t)k.noff[s] * S);
      }
    }
    else if (twoD) k_keymask2d(c, k.sup_vis, b->boundary_frame + b0, nseq, k.Nc, T_, k.km);          // ta:213-223
    else k_keymask(c, k.sup_vis, b->boundary_frame + b0, nseq, k.Nc, T_, k.km);                      // 3d:167-180 (R2,R3)
    // Token pruning (3DSPA, fused 16-bit attention): a frame token whose key is masked is attended to by nobody, and only token 0 leaves
    // the stack (3d:187-188), so its row influences neither the output nor any gradient: the encoder runs on the kept rows only.
    k.enc_rg = Rag(); k.row_src = nullptr;
    const bool can_prune = !twoD && c->prune && attn_takes_ragged_self(c->attn, S, Dh, (int)sizeof(T));
    if (can_prune) {
      int32_t* cnt = alloc<int32_t>(nseq); int32_t* off = alloc<int32_t>(nseq + 1); k.row_src = alloc<int32_t>(nseq * S);
      const int64_t kept = k_prune_plan(c, k.km, nseq, S, cnt, off, k.row_src);
      if (!c->dry && k.count_plan) { c->plan_stats[0] += (double)kept; c->plan_stats[1] += (double)(nseq * S); }
      if (c->dry || kept < nseq * S) { k.enc_rg.off = off; k.enc_rg.rows = kept; }   // (the sizing dry run takes this branch at the dense count)
    }
    const Rag& rg = k.enc_rg;
    const int64_t rows = rg.off ? rg.rows : nseq * S, rows_g = rg.off ? (rows + 7) & ~int64_t(7) : rows;
    k.dino = dino_in; k.depthf = depth_in;
    bool emb_done = false;
    if constexpr (sizeof(T) == 2) {
      // K1: the three Denses are ONE Dense on the concatenated row (repair R4) -- one GEMM over K = 256 sin features + 768 DINO columns
      // (two A sources, no concatenated copy), depth as a rank-1 term and the summed biases in the f32 epilogue, every kept token row written
      // ONCE, straight into the compact (pruned) order; dropped frame tokens are neither computed nor gathered, readout rows come from k_embed_maps
      if (emb_wt && (g.dino_feature_dim > 0) == (k.dino != nullptr) && (g.depth_feature_dim > 0) == (k.depthf != nullptr) &&
          nseq * (int64_t)T_ < 0x7fffffffLL && rows < 0x7fffffffLL) {
        const int64_t mk_emb = c->ar.mark();
        T* out = alloc<T>(rows_g * d);
        int32_t* arow = alloc<int32_t>(rows); int32_t* crow = alloc<int32_t>(rows);
        k_embed_maps<T>(c, rg.off ? k.row_src : nullptr, rows, S, T_, arow, crow, out, readout, d);
        GemmDesc e{};
        e.A = k.sinbuf; e.sAm = tok.K; e.sAk = 1; e.B = emb_wt; e.sBk = 1; e.sBn = emb_K; e.Bt = emb_wt; e.ldBt = emb_K; e.C = out; e.sCm = d;
        e.M = rows; e.N = d; e.K = emb_K; e.bias = emb_bias; e.arow_idx = arow; e.crow_idx = crow;
        if (k.dino) { e.A2 = k.dino; e.sA2m = g.dino_feature_dim; e.K1 = tok.K; }
        if (k.depthf) { e.r1_x = k.depthf; e.r1_w = depth.src[0]; }
        emb_done = plan_nt(e, c->gemm) == GemmKernel::NtEmbed;
        if (emb_done) gemm_launch<T>(c, e, GemmKernel::NtEmbed);
        if (emb_done) k.tok0 = out;   // (the maps stay allocated for the chunk: the launch is asynchronous)
        else c->ar.release(mk_emb);   // refused: the multi-pass path below allocates its own buffers; k_embed_maps wrote only into what is released here
      }
    }
    T* tokc = (rg.off && !emb_done) ? alloc<T>(rows_g * d) : nullptr;
    const int64_t mk_dense = c->ar.mark();
    if (!emb_done) {
    k.tok0 = alloc<T>(nseq * S * d);
    // 3DSPA: rows 1..T of every sequence <- Dense(sin) [+ Dense(dino)] [+ Dense(depth)] (3d:137-147); TRAJAN: rows 0..T-1 (ta:211)
    const int cg = twoD ? 0 : T_, cs = twoD ? 0 : 1;
    lin_fwd(tok, k.sinbuf, k.tok0, nseq * T_, EPI_NONE, nullptr, 0, 0, 0, 0, cg, cs);
    if (k.dino) lin_fwd(dino, (const T*)k.dino, k.tok0, nseq * T_, EPI_NONE, nullptr, 0, 1, 0, 0, T_, 1);
    if (k.depthf) {
      // 1-channel input: a rank-1 update of the token tensor, streamed (as a K=1 GEMM it ran at 1 TB/s); bf16 path only
      bool streamed = false;
      if constexpr (sizeof(T) == 2) streamed = depth.ldn == depth.N && k_rank_fwd<T>(c, (const T*)k.depthf, depth.wn, depth.bias, k.tok0, nseq * T_, depth.N, depth.K, d, T_, 1);
      if (!streamed)
        lin_fwd(depth, (const T*)k.depthf, k.tok0, nseq * T_, EPI_NONE, nullptr, 0, 1, 0, 0, T_, 1);
    }
    if (!twoD) k_set_readout_rows<T>(c, k.tok0, readout, nseq, S, d);                                // 3d:161-165
    }
    const T* x = k.tok0;
    const float* km = k.km;
    if (rg.off) {  // compact, then the dense token tensor is dead (the backward rebuilds a dense gradient for the embed dW)
      if (!emb_done) {
        k_rows_idx<T>(c, 0, k.tok0, k.row_src, tokc, rows, d);
        c->ar.release(mk_dense);
        k.tok0 = tokc; x = tokc;
      }
      km = nullptr;  // every kept key is visible
    }
    delete eps;
    const int nenc = (int)enc.blocks.size();
    const int nfull = twoD ? nenc : nenc - 1;  // TRAJAN pools over every frame token: no pruned last block
    k.enc_st.resize(nenc);
    T* pp[2] = {nullptr, nullptr};
    if (!train && nfull > 0) { pp[0] = alloc<T>(rows_g * d); if (nfull > 1) pp[1] = alloc<T>(rows_g * d); }
    for (int i = 0; i < nfull; ++i) {
      T* y = train ? alloc<T>(rows_g * d) : pp[i & 1];
      block_fwd(enc.blocks[i], x, y, nseq, S, km, nullptr, 0, train ? &k.enc_st[i] : nullptr, rg);
      x = y;
    }
    k.enc_last = const_cast<T*>(x);
    k.enc_out = enc_dst ? enc_dst : alloc<T>(nseq * d);
    if (twoD) {
      k.enc_ln_all = alloc<T>(nseq * S * d); k.st_all = alloc<float>(nseq * S * 2);
      k_layernorm<T>(c, x, enc.norm_enc, k.enc_ln_all, k.st_all, nseq * S, d);                       // attention.py:49-51
      k_vis_mean_pool<T>(c, k.enc_ln_all, k.sup_vis, nseq, T_, d, k.enc_out);                        // ta:230-232
    } else {
      k.r0 = alloc<T>(nseq * d); k.st_r0 = alloc<float>(nseq * 2);
      block_fwd_last(enc.blocks[nenc - 1], x, k.r0, nseq, S, km, train ? &k.enc_lst : nullptr, rg);  // token 0 only: 3d:187-188
      k_layernorm<T>(c, k.r0, enc.norm_enc, k.enc_out, k.st_r0, nseq, d);                            // attention.py:49-51 (row 0 only)
    }
  }
  // L1-L3: k.enc_out holds all k.Bc * k.Nk encoder outputs -> k.latents [Bc,L,Ld] f32 (written to lat_dst when given, else allocated here)
  void encode_latents(Chunk& k, bool train, float* lat_dst = nullptr) {
    const int L = g.num_latent_tokens, dl = g.encoder_latent_dim;
    const T* x;
    if (k.packed) { k.koff_dev = alloc<int32_t>(k.Bc + 1); k_set_i32(c, k.koff_dev, k.noff.data(), k.Bc + 1); }
    const int32_t* koff_h = k.packed ? k.noff.data() : nullptr;
    Holes hl;
    if (k.folds) { k.holes_dev = alloc<int32_t>(2 * k.Bc); k_set_i32(c, k.holes_dev, k.holes_h.data(), 2 * k.Bc); hl.host = k.holes_h.data(); hl.dev = k.holes_dev; hl.Nk = k.Nk; }
    k.lat_in = alloc<T>(k.Bc * L * dl);
    k_broadcast_rows<T>(c, lat0, L, dl, k.lat_in, k.Bc);                                             // 3d:200
    x = k.lat_in;
    k.t2l_st.resize(t2l.blocks.size());
    for (size_t i = 0; i < t2l.blocks.size(); ++i) {
      T* y = alloc<T>(k.Bc * L * dl);
      block_fwd(t2l.blocks[i], x, y, k.Bc, L, nullptr, k.enc_out, k.Nk, train ? &k.t2l_st[i] : nullptr, Rag(), nullptr, koff_h, k.koff_dev,
                k.folds ? &hl : nullptr);  // 3d:201
      x = y;
    }
    k.t2l_last = const_cast<T*>(x);
    k.st_t2l = alloc<float>(k.Bc * L * 2); k.t2l_n = alloc<T>(k.Bc * L * dl);
    k_layernorm<T>(c, x, t2l.norm_enc, k.t2l_n, k.st_t2l, k.Bc * L, dl);
    k.latents = lat_dst ? lat_dst : alloc<float>(k.Bc * L * g.latent_token_dim);
    lin_fwd(comp, k.t2l_n, k.latents, k.Bc * L, EPI_NONE, nullptr, 1);                               // 3d:203
  }

  // D1-D7 (track_autoencoder_3d.py:206-263; with decode_queries, D8: -307): discretise, decompressor, decoder stack -> k.latd [Bc,L,Cl] (once per sample chunk).  latents_in: [Bc,L,Ld] f32
  void decode_latents(Chunk& k, const spa3d_batch* b, const float* latents_in, const float* noise, int64_t b0, bool train) {
    const int L = g.num_latent_tokens, Ld = g.latent_token_dim, dd = g.decoder_num_channels, Cl = dd - 128;
    const int64_t nl = k.Bc * L;
    k.clipmask = alloc<float>(nl * Ld); k.lat_q = alloc<float>(nl * Ld); k.lat_qT = alloc<T>(nl * Ld);
    k_discretize(c, latents_in, noise ? noise + b0 * L * Ld : nullptr, b->discretize, k.lat_q, k.clipmask, nl * Ld);  // 3d:251-260
    k_cast_from_f32<T>(c, k.lat_q, k.lat_qT, nl * Ld);
    k.dec_in = alloc<T>(nl * Cl);
    lin_fwd(decomp, k.lat_qT, k.dec_in, nl);                                                         // 3d:262
    const T* x = k.dec_in;
    k.dec_st.resize(dec.blocks.size());
    for (size_t i = 0; i < dec.blocks.size(); ++i) {
      T* y = alloc<T>(nl * Cl);
      block_fwd(dec.blocks[i], x, y, k.Bc, L, nullptr, nullptr, 0, train ? &k.dec_st[i] : nullptr);  // 3d:263
      x = y;
    }
    k.dec_last = const_cast<T*>(x);
    k.st_dec = alloc<float>(nl * 2); k.latd = alloc<T>(nl * Cl);
    k_layernorm<T>(c, x, dec.norm_enc, k.latd, k.st_dec, nl, Cl);
  }
  // D8: query tokens, readout stack and head of queries [k.q_off, k.q_off + k.Qc) of samples [b0, b0 + k.Bc) against k.latd
  void decode_queries(Chunk& k, const spa3d_batch* b, int64_t b0, bool train) {
    const int L = g.num_latent_tokens, dd = g.decoder_num_channels, Cl = dd - 128, nf = g.num_frequencies;
    const int64_t nq = k.nq();
    const T* x;
    // query tokens                                                                                     3d:209-233,265-275
    const int F = NC * 2 * nf + 1;
    k.feat = alloc<float>(nq * F); k.qframe = alloc<int32_t>(nq);
    // the chunk's query points where they lie in the batch, or -- a packed chunk -- the live ones of its samples copied back to back
    float* pq = k.packed && !k.folds ? alloc<float>(nq * (NC + 1)) : nullptr;
    const float* qp = pq;
    k.for_each_query_span(b0, [&](int64_t r, int64_t br, int64_t n, int64_t) {
      const float* src = b->query_points + br * (NC + 1);
      if (pq) copy_dd(pq + r * (NC + 1), src, n * (NC + 1) * 4); else qp = src;
    });
    k_query_embed1(c, qp, nq, nf, g.track_scale_factor, g.time_scale_factor, k.feat, k.qframe, NC);
    k.sin2 = alloc<T>(nq * F * 2 * nf);
    k_sin_embed<T>(c, k.feat, nq, F, nf, g.track_scale_factor, k.sin2);
    k.qtok = alloc<T>(nq * dd);
    lin_fwd(qenc, k.sin2, k.qtok, nq);
    // readout sequences                                                                                3d:276-285
    const int S = L + 1;
    k.seq0 = alloc<T>(nq * S * dd);
    if (k.packed) {  // a query's sample decides which latents it reads
      for (int64_t s = 0; s < k.Bc; ++s) {
        const int64_t q0 = k.qoff[s]; const int qs = k.qoff[s + 1] - k.qoff[s];
        if (qs > 0) k_assemble_readout<T>(c, k.qtok + q0 * dd, k.latd + (k.lat_f0 + s) * L * Cl, k.qframe + q0, 1, qs, L, Cl, dd, k.seq0 + q0 * S * dd);
      }
    }
    else k_assemble_readout<T>(c, k.qtok, k.latd, k.qframe, k.Bc, k.Qc, L, Cl, dd, k.seq0);
    x = k.seq0;
    const int nro = (int)ro.blocks.size();
    k.ro_st.resize(nro);
    // first block: LN1 / QKV once per distinct (sample, query frame) -- see Share.  One stream sync reads the slot count.
    k.ro_sh = Share<T>(); k.ro_share = false;
    const bool share_ok = sizeof(T) == 2 && c->ro_share && nro >= 2 && dd % 8 == 0 && Cl % 8 == 0;
    // a ragged sample too narrow for the slot plan still counts its queries; a packed chunk runs without the slot plan (its slots would have to be
    // planned per sample: not carried over yet) and counts them too
    if (share_ok && (k.packed || k.Qc < 8) && k.ragged && !c->dry) c->plan_stats[3] += (double)nq;
    if (share_ok && !k.packed && k.Qc >= 8) {
      int32_t* slot = alloc<int32_t>(nq); int32_t* slot_b = alloc<int32_t>(nq); int32_t* slot_f = alloc<int32_t>(nq);
      int32_t* slot_q0 = alloc<int32_t>(nq); int32_t* scratch = alloc<int32_t>(nq + k.Bc + 1);
      Share<T>& sh = k.ro_sh;
      sh.slot = slot; sh.slot_b = slot_b; sh.slot_q0 = slot_q0; sh.Q = k.Qc;
      if (c->dry) { sh.nslot = (int64_t)(SHARE_MAX_FRAC * (double)nq); sh.probe = true; k.ro_share = true; }
      else {
        sh.nslot = k_share_plan(c, k.qframe, k.Bc, k.Qc, slot, slot_b, slot_f, slot_q0, scratch);
        c->plan_stats[2] += (double)sh.nslot; c->plan_stats[3] += (double)nq;
        if ((double)sh.nslot <= SHARE_MAX_FRAC * (double)nq) {
          T* xU = alloc<T>(((sh.rows(nq, S) + 7) & ~int64_t(7)) * dd);
          k_share_assemble<T>(c, k.qtok, k.latd, slot_b, slot_f, sh.nslot, nq, L, Cl, dd, xU);
          sh.xU = xU; k.ro_share = true;
        }
      }
    }
    T* pp[2] = {nullptr, nullptr};
    if (!train && nro > 1) { pp[0] = alloc<T>(nq * S * dd); if (nro > 2) pp[1] = alloc<T>(nq * S * dd); }
    for (int i = 0; i + 1 < nro; ++i) {
      T* y = train ? alloc<T>(nq * S * dd) : pp[i & 1];
      block_fwd(ro.blocks[i], x, y, nq, S, nullptr, nullptr, 0, train ? &k.ro_st[i] : nullptr, Rag(), (i == 0 && k.ro_share) ? &k.ro_sh : nullptr);
      x = y;
    }
    k.ro_last = const_cast<T*>(x);
    k.q0 = alloc<T>(nq * dd); k.st_q0 = alloc<float>(nq * 2); k.q0n = alloc<T>(nq * dd);
    block_fwd_last(ro.blocks[nro - 1], x, k.q0, nq, S, nullptr, train ? &k.ro_lst : nullptr);       // token 0 only: 3d:286
    k_layernorm<T>(c, k.q0, ro.norm_enc, k.q0n, k.st_q0, nq, dd);
    k.head = alloc<float>(nq * 4 * g.num_output_frames);
    lin_fwd(pred, k.q0n, k.head, nq, EPI_NONE, nullptr, 1);                                           // 3d:287
  }


  // Overlap of the data-parallel gradient all-reduce with the backward: parameter gradients accumulate over the sample chunks, so
  // a leaf is final only in the LAST chunk's backward -- in reverse graph order.  The caller may register two events (spa3d_set_grad_events);
  // each is recorded on the launch stream when its segment of the flat gradient buffer (spa3d_grad_segments) has received its last
  // contribution; the third segment (embedding, track encoder, state_init leaves) is final when the call's work is.  With a loss scale (fp16) a
  // finished segment is unscaled right before its event; the rest of the buffer at the end of the call.
  int64_t seg_lo[2] = {0, 0}, seg_hi[2] = {0, 0};  // flat ranges of segment 0 ([b2, n): readout side) and 1 ([b1, b2): latent stacks), spa3d_grad_segments
  const float* scale_dev = nullptr;                  // fp16 mode: the call's loss scale (device)
  const float* ptw = nullptr;                        // the call's point weights (RunArgs::w)
  bool seg_unscaled[2] = {false, false};
  bool seg_frozen[2] = {false, false};               // "freeze": the segment lies in the frozen range -- nothing to flush or unscale, its event is still recorded
  void grad_segment_done(int i) {
    if (c->dry || !c->last_chunk || !c->grad_ev[i]) return;
    if (c->det && seg_hi[i] > seg_lo[i] && !seg_frozen[i]) k_det_flush(c, seg_lo[i], seg_hi[i] - seg_lo[i]);   // the segment's shadow sums are final too
    if (c->loss_scale != 1.f && !seg_frozen[i]) {  // fp16: bring the finished segment back to true scale NOW (a power of two: exact) so that its all-reduce can start behind the event
      if (!scale_dev || seg_hi[i] <= seg_lo[i]) return;
      k_unscale(c, G + seg_lo[i], scale_dev, seg_hi[i] - seg_lo[i]);
      seg_unscaled[i] = true;
    }
    if (hipEventRecord((hipEvent_t)c->grad_ev[i], c->stream) != hipSuccess && !c->hip_err) { c->hip_err = -6; c->err = "recording a gradient-segment event failed"; }
    else c->grad_ev_gen[i] += 1;
  }
  // The backward of a chunk in three stages; parameter gradients accumulate into G.
  // head, readout transformer, assembly, query encoder of queries [k.q_off, k.q_off + k.Qc): dlatd32 [Bc,L,Cl] = (accumulate ? += : =) the latent-side gradient
  void backward_queries(Chunk& k, const spa3d_batch* b, int64_t b0, const float* denom_dev, float* dlatd32, bool accumulate) {
    const int L = g.num_latent_tokens, dd = g.decoder_num_channels, Cl = dd - 128, To = g.num_output_frames;
    const int64_t nq = k.nq();
    {
      const int S = L + 1;
      const int64_t mk = c->ar.mark();
      T* dhead = alloc<T>(nq * 4 * To);
      k.for_each_query_span(b0, [&](int64_t r, int64_t br, int64_t n, int64_t) {  // targets stay in the batch's padded layout
        k_loss_bwd<T>(c, k.head + r * 4 * To, n, To, b->query_tracks + br * To * NC, b->query_tracks_visible + br * To, denom_dev,
                      c->loss, at_rows(ptw, br * To), dhead + r * 4 * To, NC, c->loss_scale != 1.f ? denom_dev + 1 : nullptr);  // + loss scale in fp16 mode
      });
      lin_bwd_w(pred, k.q0n, dhead, nq);
      T* dq0n = alloc<T>(nq * dd);
      lin_bwd_x(pred, dhead, dq0n, nq);
      T* dq0 = alloc<T>(nq * dd);
      k_layernorm_bwd<T>(c, k.q0, ro.norm_enc, k.st_q0, dq0n, dq0, ro.g_norm_enc, nq, dd, nullptr);
      T* dqtok = alloc<T>(nq * dd);
      T* dseq = alloc<T>(nq * S * dd);
      const int nro = (int)ro.blocks.size();
      block_bwd_last(ro.blocks[nro - 1], k.ro_lst, dq0, dseq, nq, S, nullptr);
      for (int i = nro - 2; i >= 0; --i)
        block_bwd(ro.blocks[i], k.ro_st[i], dseq, dseq, nq, S, nullptr, nullptr, 0, nullptr, Rag(), (i == 0 && k.ro_share) ? &k.ro_sh : nullptr);
      if (k.packed) {
        for (int64_t s = 0; s < k.Bc; ++s) {
          const int64_t q0 = k.qoff[s]; const int qs = k.qoff[s + 1] - k.qoff[s];
          if (qs > 0) k_assemble_readout_bwd<T>(c, dseq + q0 * S * dd, k.qframe + q0, 1, qs, L, Cl, dd, dqtok + q0 * dd, dlatd32 + s * L * Cl, accumulate);
          else if (!accumulate) k_zero(c, dlatd32 + s * L * Cl, (int64_t)L * Cl * 4);  // a sample without live queries sends no gradient to its latents
        }
      }
      else k_assemble_readout_bwd<T>(c, dseq, k.qframe, k.Bc, k.Qc, L, Cl, dd, dqtok, dlatd32, accumulate);
      lin_bwd_w(qenc, k.sin2, dqtok, nq);
      c->ar.release(mk);
    }
  }
  // decompress_attn, decompressor, straight-through clip, compressor, tracks_to_latents (+ state_init) from the latent-side gradient -> d enc_out [Bc * N, d]
  // lat0_trains = false ("freeze" 1): state_init lies in the frozen range [0, b1) although this stage consumes it -- its gradient is not added
  T* backward_latents(Chunk& k, const float* dlatd32, bool lat0_trains = true) {
    const int L = g.num_latent_tokens, Ld = g.latent_token_dim, dd = g.decoder_num_channels, Cl = dd - 128;
    const int d = g.track_token_dim, dl = g.encoder_latent_dim;
    const int64_t nl = k.Bc * L;
    T* ddec = alloc<T>(nl * Cl);
    {
      T* dlatd = alloc<T>(nl * Cl);
      k_cast_from_f32<T>(c, dlatd32, dlatd, nl * Cl);
      k_layernorm_bwd<T>(c, k.dec_last, dec.norm_enc, k.st_dec, dlatd, ddec, dec.g_norm_enc, nl, Cl, nullptr);
    }
    for (int i = (int)dec.blocks.size() - 1; i >= 0; --i)
      block_bwd(dec.blocks[i], k.dec_st[i], ddec, ddec, k.Bc, L, nullptr, nullptr, 0, nullptr);
    lin_bwd_w(decomp, k.lat_qT, ddec, nl);
    T* dlq = alloc<T>(nl * Ld);
    lin_bwd_x(decomp, ddec, dlq, nl);
    float* dl32 = alloc<float>(nl * Ld);
    k_cast_to_f32<T>(c, dlq, dl32, nl * Ld);
    k_mul(c, dl32, k.clipmask, nl * Ld);  // d/dl [l - stop_grad(l - q)] = 1, times the clip mask (3d:251,260)
    k_cast_from_f32<T>(c, dl32, dlq, nl * Ld);
    lin_bwd_w(comp, k.t2l_n, dlq, nl);
    T* dt2ln = alloc<T>(nl * dl);
    lin_bwd_x(comp, dlq, dt2ln, nl);
    T* dt2l = alloc<T>(nl * dl);
    k_layernorm_bwd<T>(c, k.t2l_last, t2l.norm_enc, k.st_t2l, dt2ln, dt2l, t2l.g_norm_enc, nl, dl, nullptr);
    const int64_t nkeys = k.packed ? (int64_t)k.noff.back() : k.Bc * k.Nk;
    T* denc_out = alloc<T>(nkeys * d);
    k_zero(c, denc_out, nkeys * d * (int64_t)sizeof(T));
    for (int i = (int)t2l.blocks.size() - 1; i >= 0; --i)
      block_bwd(t2l.blocks[i], k.t2l_st[i], dt2l, dt2l, k.Bc, L, nullptr, k.enc_out, k.Nk, denc_out, Rag(), nullptr, k.packed ? k.noff.data() : nullptr, k.koff_dev);
    grad_segment_done(1);  // tracks_to_latents, compressor, decompressor, decompress_attn
    if (lat0_trains) k_bcast_grad<T>(c, dt2l, (int64_t)L * dl, k.Bc, (int64_t)L * dl, g_lat0);
    return denc_out;
  }
  // track encoder (E7-E1) of the tracks of k (k.nseq sequences, stashed by encode_tracks(train = true)) against their rows denc_out [nseq, d]
  void backward_tracks(Chunk& k, const T* denc_out) {
    const int d = g.track_token_dim, T_ = k.T_;
    const int64_t nseq = k.nseq;
    const int S = k.S;
    const int64_t erows = k.enc_rg.off ? (k.enc_rg.rows + 7) & ~int64_t(7) : nseq * S;
    T* dtok = alloc<T>(erows * d);
    const int nenc = (int)enc.blocks.size();
    if (twoD) {
      T* dln = alloc<T>(nseq * S * d);
      k_vis_mean_pool_bwd<T>(c, denc_out, k.sup_vis, nseq, T_, d, dln);
      k_layernorm_bwd<T>(c, k.enc_last, enc.norm_enc, k.st_all, dln, dtok, enc.g_norm_enc, nseq * S, d, nullptr);
      for (int i = nenc - 1; i >= 0; --i)
        block_bwd(enc.blocks[i], k.enc_st[i], dtok, dtok, nseq, S, k.km, nullptr, 0, nullptr);
      lin_bwd_w(tok, k.sinbuf, dtok, nseq * T_);
    } else {
      T* dr0 = alloc<T>(nseq * d);
      k_layernorm_bwd<T>(c, k.r0, enc.norm_enc, k.st_r0, denc_out, dr0, enc.g_norm_enc, nseq, d, nullptr);
      const Rag& rg = k.enc_rg;
      const float* km = rg.off ? nullptr : k.km;
      block_bwd_last(enc.blocks[nenc - 1], k.enc_lst, dr0, dtok, nseq, S, km, rg);
      for (int i = nenc - 2; i >= 0; --i)
        block_bwd(enc.blocks[i], k.enc_st[i], dtok, dtok, nseq, S, km, nullptr, 0, nullptr, rg);
      const T* dtok_dense = dtok;
      if (rg.off) {
        T* d0 = alloc<T>(nseq * d);                                                    // rows 0 -> the readout token's gradient
        k_rows_idx<T>(c, 0, dtok, rg.off, d0, nseq, d);
        k_bcast_grad<T>(c, d0, d, nseq, d, g_readout);
        T* dd = alloc<T>(nseq * S * d);                                                // dense gradient for the embed dW (pruned rows: 0)
        k_zero(c, dd, nseq * S * d * (int64_t)sizeof(T));
        k_rows_idx<T>(c, 1, dtok, k.row_src, dd, rg.rows, d);
        dtok_dense = dd;
      } else {
        k_bcast_grad<T>(c, dtok, d, nseq, (int64_t)S * d, g_readout);
      }
      // token rows 1..T of every sequence (row remap on the reduction index: no compaction copy)
      lin_bwd_w(tok, k.sinbuf, dtok_dense, nseq * T_, 0, T_, 1);
      if (k.dino) lin_bwd_w(dino, (const T*)k.dino, dtok_dense, nseq * T_, 0, T_, 1);
      bool streamed = false;
      if constexpr (sizeof(T) == 2)
        streamed = k.depthf && depth.nseg == 1 && k_rank_bwd<T>(c, (const T*)k.depthf, dtok_dense, nseq * T_, depth.N, depth.K, d, T_, 1, depth.gw[0], depth.gb);
      if (k.depthf && !streamed)
        lin_bwd_w(depth, (const T*)k.depthf, dtok_dense, nseq * T_, 0, T_, 1);
    }
  }
};

// ---------------------------------------------------------------------------------------------
// drivers
// ---------------------------------------------------------------------------------------------
// test mode "poison": everything allocated from arena offset `mark` on starts as NaN (0xFFFF / 0xFFFFFFFF) instead of what an earlier
// chunk left there
static void poison_from(spa3d_ctx* c, int64_t mark) {
  if (!c->poison || c->dry) return;
  const int64_t o = (mark + 255) & ~int64_t(255);
  if (o < c->ar.cap) (void)hipMemsetAsync(c->ar.base + o, 0xFF, (size_t)(c->ar.cap - o), c->stream);
}

// the launch arguments every score launch of a call shares (the caller's whole tensors; the thresholds by value)
static ScoreArgs score_args(const spa3d_batch* b, const spa3d_scores* sc, int To, int NC) {
  ScoreArgs s{};
  s.tgt = b->query_tracks; s.tvis = b->query_tracks_visible; s.scale = sc->sample_scale; s.qstats = sc->query_stats; s.frame_err = sc->frame_err;
  s.Q = b->Q; s.T = To; s.NC = NC; s.thr.K = sc->num_thresholds;
  for (int i = 0; i < SCORE_MAX_K; ++i) s.thr.t[i] = i < sc->num_thresholds ? sc->thresholds[i] : 0.f;
  return s;
}
// query_stats / frame_err rows [r0, r0 + nr) of the padded queries of a ragged batch read as 0
static void score_zero_rows(spa3d_ctx* c, const spa3d_scores* sc, int64_t r0, int64_t nr, int To) {
  if (c->dry || nr <= 0) return;
  const int64_t S = score_row_len(sc->num_thresholds);
  (void)hipMemsetAsync(sc->query_stats + r0 * S, 0, (size_t)(nr * S) * 4, c->stream);
  if (sc->frame_err) (void)hipMemsetAsync(sc->frame_err + r0 * To, 0, (size_t)(nr * To) * 4, c->stream);
}
// The query rows [r0, r0 + nr) of the batch -- the padded queries of a sample of a ragged batch -- read as 0 in every tensor the call writes per query
static void zero_padded_rows(spa3d_ctx* c, const RunArgs& a, int NC, int64_t r0, int64_t nr) {
  if (c->dry || nr <= 0) return;
  const int To = c->cfg.num_output_frames;
  if (a.out && a.out->tracks) (void)hipMemsetAsync(a.out->tracks + r0 * To * NC, 0, (size_t)(nr * To * NC) * 4, c->stream);
  if (a.out && a.out->visible_logits) (void)hipMemsetAsync(a.out->visible_logits + r0 * To, 0, (size_t)(nr * To) * 4, c->stream);
  if (a.out && a.out->certain_logits) (void)hipMemsetAsync(a.out->certain_logits + r0 * To, 0, (size_t)(nr * To) * 4, c->stream);
  if (a.score) score_zero_rows(c, a.score, r0, nr, To);
}

// Per-track scores (spa3d_score), then outputs and loss sums, of the chunk's queries from k.head: one launch each per span of batch rows
// (Chunk::for_each_query_span).  Targets and results stay in the batch's padded layout.
template <typename T>
static void emit_outputs(spa3d_ctx* c, const RunArgs& a, Net<T>& net, typename Net<T>::Chunk& k, int64_t b0, float* sums, unsigned* poison) {
  const spa3d_batch* b = a.b; const int To = c->cfg.num_output_frames, NC = net.NC;
  const bool train = a.mode == MODE_TRAIN;
  if (a.score) {
    ScoreArgs s = score_args(b, a.score, To, NC);
    k.for_each_query_span(b0, [&](int64_t r, int64_t br, int64_t n, int64_t) { s.head = k.head + r * 4 * To; s.nq = n; s.row0 = br; k_score_rows(c, s); });
    if (!a.out) return;  // spa3d_score(out = NULL) writes no prediction tensor at all
  }
  k.for_each_query_span(b0, [&](int64_t r, int64_t br, int64_t n, int64_t) {
    float* tr = a.out && a.out->tracks ? a.out->tracks + br * To * NC : nullptr;
    float* vl = a.out && a.out->visible_logits ? a.out->visible_logits + br * To : nullptr;
    float* cl = a.out && a.out->certain_logits ? a.out->certain_logits + br * To : nullptr;
    k_loss_fwd(c, k.head + r * 4 * To, n, To, train ? b->query_tracks + br * To * NC : nullptr, train ? b->query_tracks_visible + br * To : nullptr,
               tr, vl, cl, sums, poison, NC, c->loss, train ? at_rows(a.w, br * To) : nullptr);
  });
}

// One chunk of k.Bc >= 1 samples [b0, b0 + k.Bc), in every mode: the one route a sample takes through the network, whether the chunk is uniform, one
// sample of a ragged batch (spa3d_set_counts) addressed in place at its own size -- its live rows are the first rows of its slice of the padded
// tensors, nothing at or beyond a count is read -- or several such samples packed back to back (Chunk::packed).
// Intra-sample chunks (spa3d_set_option "track_chunk" / "query_chunk"; run() has made k.Bc == 1):
//  track_chunk: pass A runs the track encoder over chunks of tracks without a stash (the no-stash ping-pong path) into one persistent
//    [N, d] enc_out; tracks_to_latents sees all N keys as before.  Pass B, after the latent-side backward has produced d enc_out for all N
//    tracks, re-runs each chunk's encoder forward WITH its stash and its backward against its rows (the reference's nn.remat idea, applied to
//    the largest stash).  Parameter gradients accumulate as they do across sample chunks.
//  query_chunk: readout rows depend on their query and the sample's latents only, and the loss denominator is batch-global and known up front,
//    so each chunk of queries runs embed -> readout -> head -> loss -> readout backward; the latent-side gradient dlatd32 is written by the
//    first chunk and accumulated (fp32, fixed order, no atomics) by the others.  Without query_chunk the loop below has one iteration.
template <typename T>
static void run_chunk(spa3d_ctx* c, const RunArgs& a, Net<T>& net, typename Net<T>::Chunk& k, int64_t b0, const float* noise, float* sums,
                      unsigned* poison, const float* denom_dev) {
  const spa3d_batch* b = a.b; const spa3d_config& g = c->cfg;
  const int L = g.num_latent_tokens, Ld = g.latent_token_dim, Cl = g.decoder_num_channels - 128, d = g.track_token_dim;
  const bool train = a.mode == MODE_TRAIN;
  // The readout stash of a query chunk is released when the chunk is done -- before backward_latents -- on the calls that have always done so:
  // intra-sample chunks, and a ragged sample alone in its chunk.  Every other chunk keeps it to its end, as it always has.  Releasing it everywhere
  // would lower the training need (and so raise the chunk size a workspace gives, and change the step time): a follow-up with a benchmark of its own.
  const bool release_each = c->query_chunk > 0 || c->track_chunk > 0 || (k.ragged && !k.packed);
  const int64_t ntrk = k.nseq, Qall = k.Qc;  // (track_chunk / query_chunk: k.Bc == 1)
  const int64_t tc = c->track_chunk > 0 ? std::min<int64_t>(c->track_chunk, ntrk) : ntrk, qc = c->query_chunk > 0 ? std::min<int64_t>(c->query_chunk, Qall) : Qall;
  auto track_slice = [&](int64_t n0) { k.n_off = n0; k.Nc = (int)std::min(tc, ntrk - n0); k.nseq = k.Nc; };
  // "freeze" (train only): the backward stops at a stage boundary.  The stages below it are skipped whole, and a stage the backward no longer enters runs
  // its forward without a stash: the same kernels (block_fwd and encode_tracks choose none by whether a stash is kept) into buffers released at once.
  const int fz = train ? c->freeze : 0;
  const bool stash_enc = train && fz < 1, stash_lat = train && fz < 2;
  if (a.mode != MODE_DECODE) {
    // freeze 2: no backward reads anything below the latents -- they are all that stays of the two encoder stages for the rest of the chunk
    float* lat_keep = fz >= 2 ? net.template alloc<float>(k.Bc * L * Ld) : nullptr;
    const int64_t mk_lat = c->ar.mark();
    if (c->track_chunk > 0) {  // pass A
      T* enc_all = net.template alloc<T>(ntrk * d);
      for (int64_t n0 = 0; n0 < ntrk; n0 += tc) {
        track_slice(n0);
        const int64_t mk = c->ar.mark();
        poison_from(c, mk);
        net.encode_tracks(k, b, b0, false, enc_all + n0 * d);
        c->ar.release(mk);
      }
      k.enc_out = enc_all; k.n_off = 0; k.Nc = (int)ntrk; k.nseq = ntrk;
    } else if (fz > 0) {
      // no encoder backward: enc_out is all backward_latents reads of this stage (with the packed key offsets, which encode_latents allocates), so the
      // ping-pong buffers, the token rows and the packed copies of a ragged chunk go now, not at the end of the chunk -- as pass A above does per slice
      T* enc_keep = net.template alloc<T>(ntrk * d);
      const int64_t mk = c->ar.mark();
      net.encode_tracks(k, b, b0, false, enc_keep);
      c->ar.release(mk);
    } else {
      net.encode_tracks(k, b, b0, stash_enc);
    }
    net.encode_latents(k, stash_lat, lat_keep);
    if (lat_keep) c->ar.release(mk_lat);
    float* lo = a.latents_out ? a.latents_out : (a.out && a.out->latents ? a.out->latents : nullptr);
    if (lo && !c->dry) (void)hipMemcpyAsync(lo + b0 * L * Ld, k.latents, (size_t)(k.Bc * L * Ld) * 4, hipMemcpyDeviceToDevice, c->stream);
  }
  if (a.mode == MODE_ENCODE) return;
  if (a.cq) for (int64_t s = 0; s < k.Bc; ++s) zero_padded_rows(c, a, net.NC, (b0 + s) * b->Q + a.cq[b0 + s], b->Q - a.cq[b0 + s]);
  if (k.nq() == 0) {  // no live query: no readout, no loss term, no gradient; the call's gradient segments may still end with this chunk
    if (train) { net.grad_segment_done(0); net.grad_segment_done(1); }
    return;
  }
  net.decode_latents(k, b, a.mode == MODE_DECODE ? a.latents_in + b0 * L * Ld : k.latents, noise, b0, stash_lat);
  float* dlatd32 = train ? net.template alloc<float>(k.Bc * L * Cl) : nullptr;
  for (int64_t q0 = 0; q0 < Qall; q0 += qc) {
    k.q_off = q0; k.Qc = (int)std::min(qc, Qall - q0);
    const int64_t mk = c->ar.mark();
    if (release_each) poison_from(c, mk);
    net.decode_queries(k, b, b0, train);
    emit_outputs<T>(c, a, net, k, b0, sums, poison);
    if (train) net.backward_queries(k, b, b0, denom_dev, dlatd32, q0 > 0);
    if (release_each) c->ar.release(mk);
  }
  if (!train) return;
  net.grad_segment_done(0);  // track_readout_attn, query_encoder, track_predictor: final after the last query chunk of the LAST sample chunk (grad_segment_done checks)
  if (fz >= 2) { net.grad_segment_done(1); return; }  // the backward ends here: the latents event follows the readout event directly, as for nq() == 0 above
  const T* denc_out = net.backward_latents(k, dlatd32, fz < 1);
  if (fz >= 1) return;  // the backward ends with the latent stacks (their event is recorded there); d enc_out is dead, and pass B with its recompute is dropped
  if (c->track_chunk <= 0) { net.backward_tracks(k, denc_out); return; }
  k.count_plan = false;  // pass B: recompute + backward per track chunk
  for (int64_t n0 = 0; n0 < ntrk; n0 += tc) {
    track_slice(n0);
    const int64_t mk = c->ar.mark();
    poison_from(c, mk);
    net.encode_tracks(k, b, b0, true);
    net.backward_tracks(k, denc_out + n0 * d);
    c->ar.release(mk);
  }
}

// spa3d_score_folds: a leave-fold-out round over every clip, one clip at a time.  The track encoder -- per track, and by far the largest stage -- runs ONCE
// over the clip's N tracks; the latent stacks run on F sequences that share its output rows (the K / V projection of tracks_to_latents once over the N
// rows, the cross attention with fold f's rows left out of sequence f: Holes); the readout decodes every track once, against the latents of its own fold,
// over groups of G consecutive folds (G: the most that fit the workspace), released between groups.  Forward only; nothing but the prune count is read back.
template <typename T>
static void run_folds(spa3d_ctx* c, const RunArgs& a, Net<T>& net, const float* noise, float* sums, unsigned* poison, int G) {
  const spa3d_batch* b = a.b; const spa3d_config& g = c->cfg;
  const int F = a.nfold; const int64_t LL = (int64_t)g.num_latent_tokens * g.latent_token_dim;
  for (int64_t b0 = 0; b0 < b->B; ++b0) {
    typename Net<T>::Chunk k{};
    c->last_chunk = b0 + 1 >= b->B;
    k.Bc = 1; k.N = b->N; k.Q = b->Q; k.T_ = b->T; k.S = b->T + 1; k.nseq = b->N; k.Nc = b->N; k.Qc = b->Q; k.Nk = b->N;
    k.folds = true;
    const int64_t mk = c->ar.mark();
    poison_from(c, mk);
    net.encode_tracks(k, b, b0, false);  // the clip in place: no packed copy
    k.Bc = F;
    for (int f = 0; f < F; ++f) { k.holes_h.push_back(a.fold_off[f]); k.holes_h.push_back(a.fold_off[f + 1]); }
    net.encode_latents(k, false);
    const float* nz = nullptr;
    if (noise) {  // every fold of the clip discretises with the clip's noise
      float* nb = net.template alloc<float>(F * LL);
      for (int f = 0; f < F; ++f) net.copy_dd(nb + f * LL, noise + b0 * LL, LL * 4);
      nz = nb;
    }
    net.decode_latents(k, b, k.latents, nz, 0, false);
    k.packed = k.ragged = true;
    for (int f0 = 0; f0 < F; f0 += G) {
      const int f1 = std::min(F, f0 + G);
      k.Bc = f1 - f0; k.lat_f0 = f0; k.q_off = a.fold_off[f0];
      k.qoff.clear();
      for (int f = f0; f <= f1; ++f) k.qoff.push_back(a.fold_off[f] - a.fold_off[f0]);
      const int64_t mq = c->ar.mark();
      poison_from(c, mq);
      net.decode_queries(k, b, b0, false);
      emit_outputs<T>(c, a, net, k, b0, sums, poison);
      c->ar.release(mq);
    }
    c->ar.release(mk);
  }
}

template <typename T>
void run_body(spa3d_ctx* c, const RunArgs& a, int Bc) {
  const spa3d_config& g = c->cfg; const spa3d_batch* b = a.b;
  const int L = g.num_latent_tokens, Ld = g.latent_token_dim, To = g.num_output_frames;
  const bool train = a.mode == MODE_TRAIN;
  Net<T> net(c, a.P, a.G);
  net.pack();
  net.ptw = train ? a.w : nullptr;
  float* sums = net.template alloc<float>(10);
  float* denom_dev = sums + 6;  // [0..5] three 64-bit fixed-point accumulators (loss.hip loss_acc_add), [6] denominator, [7] loss scale, [8] sticky non-finite flag
  unsigned* poison = (unsigned*)(sums + 8);
  k_zero(c, sums, 40);
  const float* noise = b->noise;
  if (a.mode != MODE_ENCODE && b->discretize && !noise) {
    float* nb = net.template alloc<float>((int64_t)b->B * L * Ld);
    k_uniform_noise(c, nb, (int64_t)b->B * L * Ld, 0u, 0u);  // PRNGKey(0), 3d:254
    noise = nb;
  }
  if (train) {
    if (a.cq) {  // live queries only: whatever sits in the padded target rows is never read
      for (int64_t s = 0; s < b->B; ++s) k_vis_count(c, b->query_tracks_visible + s * b->Q * To, (int64_t)a.cq[s] * To, sums + 4, poison);
    } else {
      k_vis_count(c, b->query_tracks_visible, (int64_t)b->B * b->Q * To, sums + 4, poison);
    }
    k_set_denom(c, sums, poison, a.denom, denom_dev);
    if (c->loss_scale != 1.f) k_set_loss_scale(c, denom_dev, c->loss_gmax, c->loss_scale, denom_dev + 1);  // sums[7]
    if (!a.accumulate) k_zero(c, a.G, c->nparams * 4);
  }
  if (train && (c->loss_scale != 1.f || c->det_grads)) {
    int64_t b4[4];
    if (spa3d_grad_segments(c, b4) == SPA3D_OK) { net.seg_lo[0] = b4[2]; net.seg_hi[0] = b4[3]; net.seg_lo[1] = b4[1]; net.seg_hi[1] = b4[2]; }
    if (c->loss_scale != 1.f) net.scale_dev = denom_dev + 1;
  }
  // "freeze": [0, lo) of G is frozen -- zeroed above or left as the caller's (accumulate), and no launch below writes there: not the stages run_chunk skips,
  // not the det_grads flush, not the unscaling
  int64_t lo_n[2] = {0, c->nparams};
  if (train) { (void)spa3d_trainable_range(c, lo_n); net.seg_frozen[1] = c->freeze >= 2; }
  const int64_t glo = lo_n[0];
  // deterministic parameter gradients: every reduction into G goes through a 64-bit fixed-point shadow (common.hpp DetCfg, grad_add).  c->det belongs to this
  // call alone: every launch that adds into G passes it, and it is null again before the call returns (the shadow lives in this call's workspace)
  if (train && c->det_grads) {
    long long* sh = net.template alloc<long long>(c->nparams); unsigned* fl = net.template alloc<unsigned>(64);
    k_zero(c, sh, c->nparams * 8); k_zero(c, fl, 256);
    DetCfg* dc = (DetCfg*)(fl + 2);   // fl[0]: the sticky overflow flag, fl[2...]: the DetCfg of this call, with its fixed-point unit
    k_det_unit(c, sums, poison, denom_dev, c->loss_scale != 1.f ? denom_dev + 1 : nullptr, c->loss_gshift, DetCfg{a.G, sh, (long long)c->nparams, fl, 0.f}, dc);
    c->det = dc;
  }
  const bool ragged = a.cn || a.cq;  // per-sample counts (spa3d_set_counts; run() has validated them)
  // The ragged chunk (B % Bc samples) runs FIRST, so the last chunk -- the one under whose track-encoder backward the gradient segments are all-reduced -- is a
  // full one (B = 64, Bc = 9: 9 samples of encoder backward to hide behind instead of 1)
  if (a.nfold > 0) run_folds<T>(c, a, net, noise, sums, poison, Bc);  // (Bc: folds per readout group)
  else for (int64_t b0 = 0, cur = 0; b0 < b->B; b0 += cur) {
    typename Net<T>::Chunk k{};
    cur = (b0 == 0 && b->B % Bc) ? b->B % Bc : std::min<int64_t>(Bc, b->B - b0);
    c->last_chunk = b0 + cur >= b->B;
    k.Bc = cur; k.N = b->N; k.Q = b->Q; k.T_ = b->T; k.S = b->T + (g.model_kind == 1 ? 0 : 1); k.nseq = k.Bc * b->N;
    k.Nc = b->N; k.Qc = b->Q; k.Nk = b->N;
    if (ragged && cur == 1) {  // one sample: addressed in place, at its own size
      k.ragged = true; k.Nc = k.Nk = a.cn ? a.cn[b0] : b->N; k.nseq = k.Nc; k.Qc = a.cq ? a.cq[b0] : b->Q;
    } else if (ragged) {  // several samples: their live rows packed back to back
      k.ragged = k.packed = true; k.noff.assign(1, 0); k.qoff.assign(1, 0);
      for (int64_t s = 0; s < cur; ++s) {
        k.noff.push_back(k.noff.back() + (a.cn ? a.cn[b0 + s] : b->N));
        k.qoff.push_back(k.qoff.back() + (a.cq ? a.cq[b0 + s] : b->Q));
      }
      k.nseq = k.noff.back();
    }
    const int64_t mk = c->ar.mark();
    poison_from(c, mk);
    run_chunk<T>(c, a, net, k, b0, noise, sums, poison, denom_dev);
    c->ar.release(mk);
  }
  if (c->det) {
    k_det_flush(c, glo, c->nparams - glo);   // what the segment flushes left (flushed ranges hold zeros)
    c->det = nullptr;   // no later launch of this handle (an op backward, its next call) may add into the dead shadow (tests/test_gpu_det_edges.py)
  }
  if (train && c->loss_scale != 1.f) {  // fp32 gradient buffer back to true scale (exact: power of two); segments already unscaled at their events are skipped
    const int64_t lo1 = std::max(net.seg_lo[1], glo), lo0 = std::max(net.seg_lo[0], glo);
    if (!net.seg_unscaled[0] && !net.seg_unscaled[1]) k_unscale(c, a.G + glo, denom_dev + 1, c->nparams - glo);
    else {
      k_unscale(c, a.G + glo, denom_dev + 1, lo1 - glo);
      if (!net.seg_unscaled[1]) k_unscale(c, a.G + lo1, denom_dev + 1, lo0 - lo1);
      if (!net.seg_unscaled[0]) k_unscale(c, a.G + lo0, denom_dev + 1, c->nparams - lo0);
    }
  }
  if (train && a.loss3) k_loss_finalize(c, sums, poison, denom_dev, c->loss.l1_weight, c->loss.bce_weight, a.loss3);
  // spa3d_score: the per-sample pooled stats, ONE launch once every (sample / query / track) chunk has written its rows of query_stats
  if (a.score && a.score->sample_stats) k_score_reduce(c, a.score->query_stats, b->B, b->Q, a.score->num_thresholds, a.score->sample_stats);
}

// entry points of this build's 16-bit type (and of the fp32 parity path, which lives in the bf16 build only)
void run_body16(spa3d_ctx* c, const RunArgs& a, int Bc) { run_body<bf16_t>(c, a, Bc); }
#if !SPA_F16
void run_body32(spa3d_ctx* c, const RunArgs& a, int Bc) { run_body<float>(c, a, Bc); }
#endif
}  // namespace SPA_NS

#if !SPA_F16  // everything below exists once: host-side tree / sizing / C-ABI, dispatching on spa3d_config::precision
namespace h_f16 { void run_body16(spa3d_ctx* c, const RunArgs& a, int Bc); }
namespace h_f16 {  // loss.hip's fp16 build instantiates it (spa3d_op_head_loss)
template <typename T> void k_loss_bwd(spa3d_ctx*, const float* head, int64_t nq, int T_, const float* tgt, const float* tvis, const float* denom_dev,
                                      const spa3d_loss_config& lc, const float* wgt, T* dhead, int NC, const float* scale_dev);
}

// ---------------------------------------------------------------------------------------------
// parameter tree: canonical leaf order = sorted Flax paths grouped per module
// ---------------------------------------------------------------------------------------------
static void add_leaf(spa3d_ctx* c, const std::string& name, std::initializer_list<int64_t> shape) {
  Leaf l; l.name = name; l.ndim = (int)shape.size(); int i = 0;
  for (auto s : shape) l.shape[i++] = s;
  l.offset = c->nparams;
  c->nparams += (l.numel() + 63) / 64 * 64;  // 256-B aligned leaves
  c->leaves.push_back(l);
}
static void add_attn(spa3d_ctx* c, const std::string& p, int dq, int dkv) {
  const int H = c->cfg.num_heads, Dh = c->cfg.qkv_size / H;
  add_leaf(c, p + "/dense_query/kernel", {dq, H, Dh});
  add_leaf(c, p + "/dense_key/kernel", {dkv, H, Dh});
  add_leaf(c, p + "/dense_value/kernel", {dkv, H, Dh});
  add_leaf(c, p + "/norm_query/scale", {Dh});
  add_leaf(c, p + "/norm_key/scale", {Dh});
  add_leaf(c, p + "/dense_out/kernel", {H, Dh, dq});
  add_leaf(c, p + "/dense_out/bias", {dq});
}
static void add_xf(spa3d_ctx* c, const std::string& p, int d, int mlp, int L, int kv) {
  for (int i = 0; i < L; ++i) {
    std::string b = p + "/layer_" + std::to_string(i);
    add_leaf(c, b + "/norm_q/scale", {d});
    add_attn(c, b + "/self_att", d, d);
    if (kv) add_attn(c, b + "/cross_att", d, kv);
    add_leaf(c, b + "/norm_attn/scale", {d});
    add_leaf(c, b + "/MLP_in/kernel", {d, mlp});
    add_leaf(c, b + "/MLP_in/bias", {mlp});
    add_leaf(c, b + "/MLP_out/kernel", {mlp, d});
    add_leaf(c, b + "/MLP_out/bias", {d});
  }
  add_leaf(c, p + "/norm_encoder/scale", {d});
}
static void build_leaves(spa3d_ctx* c) {
  const spa3d_config& g = c->cfg;
  const int d = g.track_token_dim, dl = g.encoder_latent_dim, dd = g.decoder_num_channels, nf = g.num_frequencies;
  const int NC = g.model_kind == 1 ? 2 : 3;
  add_leaf(c, "initializer/state_init", {g.num_latent_tokens, dl});
  // TRAJAN declares input_readout_token in setup() but never calls it (track_autoencoder.py:147), so Flax creates no parameter
  if (g.model_kind == 0) add_leaf(c, "input_readout_token/state_init", {1, d});
  add_leaf(c, "track_token_projection/kernel", {(NC + 1) * 2 * nf, d});
  add_leaf(c, "track_token_projection/bias", {d});
  if (g.dino_feature_dim > 0) {
    add_leaf(c, "dino_projection/kernel", {g.dino_feature_dim, d});  // repair R4
    add_leaf(c, "dino_projection/bias", {d});
  }
  if (g.depth_feature_dim > 0) {
    add_leaf(c, "depth_projection/kernel", {g.depth_feature_dim, d});  // repair R5
    add_leaf(c, "depth_projection/bias", {d});
  }
  add_xf(c, "input_track_transformer", d, g.enc_mlp, g.enc_layers, 0);
  add_xf(c, "tracks_to_latents", dl, g.t2l_mlp, g.t2l_layers, d);
  add_leaf(c, "compressor/kernel", {dl, g.latent_token_dim});
  add_leaf(c, "compressor/bias", {g.latent_token_dim});
  add_leaf(c, "decompressor/kernel", {g.latent_token_dim, dd - 128});
  add_leaf(c, "decompressor/bias", {dd - 128});
  add_xf(c, "decompress_attn", dd - 128, g.dec_mlp, g.dec_layers, 0);
  add_xf(c, "track_readout_attn", dd, g.ro_mlp, g.ro_layers, 0);
  const int qin = (NC * 2 * nf + 1) * 2 * nf;
  add_leaf(c, "query_encoder/kernel", {qin, dd});
  add_leaf(c, "query_encoder/bias", {dd});
  add_leaf(c, "track_predictor/kernel", {dd, 4 * g.num_output_frames});
  add_leaf(c, "track_predictor/bias", {4 * g.num_output_frames});
}

static void run_dispatch(spa3d_ctx* c, const RunArgs& a, int Bc) {
  if (c->cfg.precision == SPA3D_F32) h_bf16::run_body32(c, a, Bc);
  else if (c->cfg.precision == SPA3D_F16) h_f16::run_body16(c, a, Bc);
  else h_bf16::run_body16(c, a, Bc);
}

static int64_t dry_need(spa3d_ctx* c, const RunArgs& a, int Bc) {
  RunArgs d = a; d.P = (const float*)0x100000; d.G = a.G ? (float*)0x100000 : nullptr;
  return arena_peak(c, [&] { run_dispatch(c, d, Bc); }) + 4096;
}
// The batch of a sizing walk: sizes only.  Its pointers are never dereferenced (the dry run launches nothing), but the orchestration offsets them per
// chunk and arithmetic on a null pointer is undefined behaviour (UBSan, tests/test_host_sanitizers.py): they point at a fake non-null base
static spa3d_batch sizing_batch(const spa3d_ctx* c, int B, int N, int Q, int T) {
  spa3d_batch b{}; b.B = B; b.N = N; b.Q = Q; b.T = T; b.discretize = 1;
  const float* fake = (const float*)(uintptr_t)0x100000;
  b.support_tracks = fake; b.support_tracks_visible = fake; b.query_points = fake; b.boundary_frame = (const int32_t*)fake;
  b.query_tracks = fake; b.query_tracks_visible = fake;
  b.dino_features = c->cfg.dino_feature_dim > 0 ? (const void*)fake : nullptr;
  b.depth_features = c->cfg.depth_feature_dim > 0 ? (const void*)fake : nullptr;
  return b;
}
// The tail of every call that runs the network.  [lo, hi]: the counts the call may run with (samples per chunk, or folds per readout group).  The need at
// `lo` (at least `floor`) is checked first -- `refuse(need)` words the entry's message and gives its status (sized_call has one wording, the entries
// here two) --, then the largest count that fits is found by bisection over dry runs and the call runs in the caller's workspace.
template <typename R> static int sized_run(spa3d_ctx* c, const RunArgs& a, int lo, int hi, int64_t floor, void* ws, int64_t ws_bytes, void* stream, R&& refuse) {
  const int64_t need = std::max(floor, dry_need(c, a, lo));
  if (ws_bytes < need) return refuse(need);
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (dry_need(c, a, mid) <= ws_bytes) lo = mid; else hi = mid - 1;
  }
  c->stream = (hipStream_t)stream; c->dry = false;
  c->ar = Arena(); c->ar.base = (char*)ws; c->ar.cap = ws_bytes;
  for (double& v : c->plan_stats) v = 0;
  run_dispatch(c, a, lo);
  if (c->ar.overflow) { c->err = "internal: arena overflow"; return SPA3D_ERR_WORKSPACE; }
  return c->hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}

// "gemm_impl" of a handle: 7 and 10 are spa3d_op_linear's one-kernel hooks; on a handle they mean 2, the product dispatch
static void set_gemm_impl(spa3d_ctx* c, int v) { c->gemm = GemmPolicy::from_impl(v == 7 || v == 10 ? 2 : v); }

static int check_batch(spa3d_ctx* c, const spa3d_batch* b, int mode) {
  if (!b || b->B <= 0 || b->Q <= 0) { c->err = "batch: B,Q must be positive"; return SPA3D_ERR_ARG; }
  if (mode != MODE_DECODE && (b->N <= 0 || b->T <= 0 || !b->support_tracks || !b->support_tracks_visible || !b->boundary_frame)) {
    c->err = "batch: support_tracks / support_tracks_visible / boundary_frame required"; return SPA3D_ERR_ARG;
  }
  if (mode != MODE_ENCODE && !b->query_points) { c->err = "batch: query_points required (host builds the default grid)"; return SPA3D_ERR_ARG; }
  if (mode == MODE_TRAIN && (!b->query_tracks || !b->query_tracks_visible)) { c->err = "batch: targets required"; return SPA3D_ERR_ARG; }
  if (c->cfg.decoder_num_channels - 128 <= 0) { c->err = "decoder_num_channels must exceed 128"; return SPA3D_ERR_ARG; }
  return SPA3D_OK;
}

static int run(spa3d_ctx* c, RunArgs a, void* ws, int64_t ws_bytes, void* stream) {
  c->err.clear(); c->hip_err = 0;
  int rc = check_batch(c, a.b, a.mode);
  if (rc) return rc;
  int lo = 1, hi = a.b->B;
  if (a.chunk <= 0) a.chunk = c->chunk;  // spa3d_set_option "chunk" / SPA3D_CHUNK: fixed samples per chunk (tests: chunk-to-chunk reuse of the arena)
  if (c->query_chunk > 0 || c->track_chunk > 0) {  // intra-sample chunks: one sample per sample chunk
    if (a.chunk > 1) { c->err = "\"chunk\" > 1 cannot be combined with \"query_chunk\" / \"track_chunk\" (they imply one sample per chunk)"; return SPA3D_ERR_ARG; }
    a.chunk = 1;
  }
  // point weights (spa3d_set_point_weights): read by the train call only, refused for another batch shape before the first launch
  a.w = nullptr;
  if (a.mode == MODE_TRAIN) {
    if (!weights_fit_batch(c, a.b->B, a.b->Q)) return SPA3D_ERR_ARG;
    a.w = c->pt_w;
  }
  // per-sample counts (spa3d_set_counts): validated here, before the first launch; the sizing dry runs below walk the live counts
  a.cn = nullptr; a.cq = nullptr;
  if (c->has_cnt_n || c->has_cnt_q) {
    const spa3d_batch* b = a.b;
    if (!counts_fit_batch(c, b->B)) return SPA3D_ERR_ARG;  // first, and also when only support counts are set; checked_query_counts below repeats it, harmlessly
    if (c->cfg.model_kind == 1) { c->err = "per-sample counts are not supported by the 2-D model (model_kind 1)"; return SPA3D_ERR_ARG; }
    if (c->query_chunk > 0 || c->track_chunk > 0) { c->err = "per-sample counts cannot be combined with \"query_chunk\" / \"track_chunk\""; return SPA3D_ERR_ARG; }
    if (c->has_cnt_n && a.mode != MODE_DECODE) {  // spa3d_decode has no support tracks: it reads the query counts only
      for (int i = 0; i < b->B; ++i)
        if (c->cnt_n[i] < 1 || c->cnt_n[i] > b->N) { c->err = "support_count[" + std::to_string(i) + "] = " + std::to_string(c->cnt_n[i]) + " is outside [1, N = " + std::to_string(b->N) + "]"; return SPA3D_ERR_ARG; }
      a.cn = c->cnt_n.data();
    }
    if (c->has_cnt_q && a.mode != MODE_ENCODE && !(a.cq = checked_query_counts(c, b->B, b->Q))) return SPA3D_ERR_ARG;
    // counts that leave nothing out describe a uniform batch: it takes the batched path, bit for bit the call without counts
    bool full = true;
    for (int i = 0; i < b->B && full; ++i) full = (!a.cn || a.cn[i] == b->N) && (!a.cq || a.cq[i] == b->Q);
    if (full) { a.cn = nullptr; a.cq = nullptr; }
  }
  if (a.chunk > 0) { lo = hi = std::min(a.chunk, a.b->B); }
  return sized_run(c, a, lo, hi, 0, ws, ws_bytes, stream, [&](int64_t need) {
    c->err = "workspace too small: need " + std::to_string(need) + " bytes for chunk " + std::to_string(lo);
    return SPA3D_ERR_WORKSPACE;
  });
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

const char* spa3d_version(void) { return "spa3d-hip 0.1 (gfx950)"; }

int spa3d_create(const spa3d_config* cfg, spa3d_handle* out) {
  if (!cfg || !out) return SPA3D_ERR_ARG;
  if (cfg->num_heads <= 0 || cfg->qkv_size % cfg->num_heads) return SPA3D_ERR_ARG;  // attention.py:147-150
  if (cfg->qkv_size / cfg->num_heads > 128 || cfg->num_frequencies > 64 || cfg->num_frequencies <= 0) return SPA3D_ERR_ARG;
  // the readout stack's last block (block_fwd_last) runs the single-query attention in every precision, model kind and attn_impl: only the head widths
  // csrc/attn_q1.hip instantiates make a usable model (any other used to fail at the first forward, as a HIP-class error)
  { const int Dh = cfg->qkv_size / cfg->num_heads;
    if (Dh != 8 && Dh != 16 && Dh != 32 && Dh != 64 && Dh != 96 && Dh != 128) return SPA3D_ERR_ARG; }
  if (cfg->precision != SPA3D_F32 && cfg->precision != SPA3D_BF16 && cfg->precision != SPA3D_F16) return SPA3D_ERR_ARG;
  if (cfg->model_kind != 0 && cfg->model_kind != 1) return SPA3D_ERR_ARG;
  if (cfg->model_kind == 1 && (cfg->dino_feature_dim != 0 || cfg->depth_feature_dim != 0)) return SPA3D_ERR_ARG;
  if (cfg->track_token_dim > 2048 || cfg->decoder_num_channels > 2048 || cfg->encoder_latent_dim > 2048) return SPA3D_ERR_ARG;
  spa3d_ctx* c = new (std::nothrow) spa3d_ctx();
  if (!c) return SPA3D_ERR_ARG;
  c->cfg = *cfg;
  build_leaves(c);
  // fp16 gradients: activations' gradients of this loss sit at 1e-5..1e-7, below fp16's normal range (6.1e-5): the 16-bit backward runs
  // at loss x 2^k (k chosen per call from the loss denominator, k_set_loss_scale) and the fp32 parameter gradients are scaled back once
  // at the end (exact for powers of two)
  if (cfg->precision == SPA3D_F16) c->loss_scale = -16.f;
  // the ten switches (include/spa3d.h, spa3d_set_option) may be preset from the environment; nothing else is read from it
  const char* e = getenv("SPA3D_GEMM_IMPL"); if (e) set_gemm_impl(c, atoi(e));
  e = getenv("SPA3D_ATTN_IMPL"); if (e) c->attn = AttnPolicy::from_impl(atoi(e));
  e = getenv("SPA3D_LOSS_SCALE"); if (e && cfg->precision == SPA3D_F16) c->loss_scale = (float)atof(e);
  e = getenv("SPA3D_PRUNE"); if (e) c->prune = atoi(e);
  e = getenv("SPA3D_RO_SHARE"); if (e) c->ro_share = atoi(e);
  e = getenv("SPA3D_CHUNK"); if (e) c->chunk = atoi(e);
  e = getenv("SPA3D_DET_GRADS"); if (e) c->det_grads = atoi(e) != 0;
  e = getenv("SPA3D_QUERY_CHUNK"); if (e) c->query_chunk = std::max(0, atoi(e));
  e = getenv("SPA3D_TRACK_CHUNK"); if (e) c->track_chunk = std::max(0, atoi(e));
  e = getenv("SPA3D_FREEZE"); if (e && atoi(e) >= 0 && atoi(e) <= 2) c->freeze = atoi(e);
  *out = c;
  return SPA3D_OK;
}
int spa3d_destroy(spa3d_handle h) { delete h; return SPA3D_OK; }
const char* spa3d_last_error(spa3d_handle h) { return h ? h->err.c_str() : "null handle"; }
int64_t spa3d_param_elems(spa3d_handle h) { return h ? h->nparams : 0; }
int32_t spa3d_num_leaves(spa3d_handle h) { return h ? (int32_t)h->leaves.size() : 0; }
int spa3d_leaf_info(spa3d_handle h, int32_t i, char* name, int32_t* ndim, int64_t* shape, int64_t* offset) {
  if (!h || i < 0 || i >= (int32_t)h->leaves.size()) return SPA3D_ERR_ARG;
  const Leaf& l = h->leaves[i];
  if (name) { strncpy(name, l.name.c_str(), 159); name[159] = 0; }
  if (ndim) *ndim = l.ndim;
  if (shape) for (int k = 0; k < l.ndim; ++k) shape[k] = l.shape[k];
  if (offset) *offset = l.offset;
  return SPA3D_OK;
}

int64_t spa3d_workspace_bytes(spa3d_handle h, int32_t B, int32_t N, int32_t Q, int32_t T, int32_t chunk, int32_t train) {
  if (!h || B <= 0 || N <= 0 || Q <= 0 || T <= 0) return -1;
  const spa3d_batch b = sizing_batch(h, B, N, Q, T);
  RunArgs a{}; a.mode = train ? MODE_TRAIN : MODE_FORWARD; a.b = &b; a.G = train ? (float*)0x100000 : nullptr;
  if (h->query_chunk > 0 || h->track_chunk > 0) chunk = 1;  // intra-sample chunks process one sample at a time
  return dry_need(h, a, std::max(1, std::min(chunk, B)));
}

int spa3d_encode(spa3d_handle h, const float* params, const spa3d_batch* b, float* latents, void* ws, int64_t ws_bytes, void* stream) {
  if (!h || !params || !latents) return SPA3D_ERR_ARG;
  RunArgs a{}; a.mode = MODE_ENCODE; a.P = params; a.b = b; a.latents_out = latents;
  return run(h, a, ws, ws_bytes, stream);
}
int spa3d_decode(spa3d_handle h, const float* params, const spa3d_batch* b, const float* latents, spa3d_outputs* out, void* ws,
                 int64_t ws_bytes, void* stream) {
  if (!h || !params || !latents || !out) return SPA3D_ERR_ARG;
  RunArgs a{}; a.mode = MODE_DECODE; a.P = params; a.b = b; a.latents_in = latents; a.out = out;
  return run(h, a, ws, ws_bytes, stream);
}
int spa3d_forward(spa3d_handle h, const float* params, const spa3d_batch* b, spa3d_outputs* out, void* ws, int64_t ws_bytes, void* stream) {
  if (!h || !params || !out) return SPA3D_ERR_ARG;
  RunArgs a{}; a.mode = MODE_FORWARD; a.P = params; a.b = b; a.out = out;
  return run(h, a, ws, ws_bytes, stream);
}
// refusals of a spa3d_scores block, before any launch
static int check_scores(spa3d_ctx* c, const spa3d_batch* b, const spa3d_scores* sc) {
  c->err.clear();
  if (!b || !b->query_tracks || !b->query_tracks_visible) { c->err = "score: the batch needs its targets (query_tracks, query_tracks_visible)"; return SPA3D_ERR_ARG; }
  if (!sc || !sc->query_stats) { c->err = "score: spa3d_scores::query_stats is required"; return SPA3D_ERR_ARG; }
  if (sc->num_thresholds < 0 || sc->num_thresholds > SCORE_MAX_K) { c->err = "score: num_thresholds = " + std::to_string(sc->num_thresholds) + " is outside [0, 8]"; return SPA3D_ERR_ARG; }
  for (int i = 0; i < sc->num_thresholds; ++i)
    if (!(std::isfinite(sc->thresholds[i]) && sc->thresholds[i] > 0.f)) { c->err = "score: thresholds[" + std::to_string(i) + "] must be finite and positive"; return SPA3D_ERR_ARG; }
  return SPA3D_OK;
}
int spa3d_score(spa3d_handle h, const float* params, const spa3d_batch* b, spa3d_scores* scores, spa3d_outputs* out, void* ws, int64_t ws_bytes, void* stream) {
  if (!h || !params) return SPA3D_ERR_ARG;
  const int rc = check_scores(h, b, scores);
  if (rc) return rc;
  RunArgs a{}; a.mode = MODE_FORWARD; a.P = params; a.b = b; a.out = out; a.score = scores;  // the forward pass: no stash, no backward
  return run(h, a, ws, ws_bytes, stream);
}
// the near-equal split of N tracks into F folds, larger folds first (what spa3d.fold_offsets gives): what the workspace function sizes for
static std::vector<int32_t> equal_folds(int N, int F) {
  std::vector<int32_t> off(1, 0);
  for (int f = 0; f < F; ++f) off.push_back(off.back() + N / F + (f < N % F ? 1 : 0));
  return off;
}
int64_t spa3d_score_folds_workspace_bytes(spa3d_handle h, int32_t N, int32_t T, int32_t num_folds) {
  if (!h || h->cfg.model_kind != 0 || T <= 0 || num_folds < 2 || num_folds > 64 || N < num_folds) return -1;
  const std::vector<int32_t> off = equal_folds(N, num_folds);
  const spa3d_batch b = sizing_batch(h, 1, N, N, T);
  RunArgs a{}; a.mode = MODE_FORWARD; a.b = &b; a.nfold = num_folds; a.fold_off = off.data();
  return dry_need(h, a, 1);  // the readout one fold at a time: the least a call with these folds can run in
}
int spa3d_score_folds(spa3d_handle h, const float* params, const spa3d_batch* b, int32_t num_folds, const int32_t* fold_off, spa3d_scores* scores,
                      spa3d_outputs* out, void* ws, int64_t ws_bytes, void* stream) {
  if (!h || !params) return SPA3D_ERR_ARG;
  h->err.clear(); h->hip_err = 0;
  auto refuse = [&](const std::string& m) { h->err = "score_folds: " + m; return SPA3D_ERR_ARG; };
  int rc = check_batch(h, b, MODE_FORWARD);
  if (rc) return rc;
  if (b->Q != b->N) return refuse("the batch must have Q == N (query row q of a clip is its track q), got Q = " + std::to_string(b->Q) + ", N = " + std::to_string(b->N));
  if (num_folds < 2 || num_folds > 64) return refuse("num_folds = " + std::to_string(num_folds) + " is outside [2, 64]");
  if (!fold_off) return refuse("fold_off is required");
  if (fold_off[0] != 0 || fold_off[num_folds] != b->N) return refuse("fold_off must start at 0 and end at N = " + std::to_string(b->N));
  for (int f = 0; f < num_folds; ++f)
    if (fold_off[f + 1] <= fold_off[f]) return refuse("fold_off must be strictly increasing (fold_off[" + std::to_string(f + 1) + "] = " + std::to_string(fold_off[f + 1]) + ")");
  spa3d_batch bb = *b;
  if (!bb.query_tracks && !bb.query_tracks_visible) {  // the targets are the support tensors themselves: no copy
    if (b->T != h->cfg.num_output_frames) return refuse("targets left NULL need T == num_output_frames, got T = " + std::to_string(b->T) + ", num_output_frames = " + std::to_string(h->cfg.num_output_frames));
    bb.query_tracks = b->support_tracks; bb.query_tracks_visible = b->support_tracks_visible;
  }
  if (h->cfg.model_kind != 0) return refuse("not supported by the 2-D model (model_kind 1)");
  if (h->has_cnt_n || h->has_cnt_q) return refuse("per-sample counts (spa3d_set_counts) cannot be combined with folds");
  if (h->track_chunk > 0 || h->query_chunk > 0) return refuse("\"track_chunk\" / \"query_chunk\" cannot be combined with folds");
  rc = check_scores(h, &bb, scores);
  if (rc) return rc;
  RunArgs a{}; a.mode = MODE_FORWARD; a.P = params; a.b = &bb; a.out = out; a.score = scores; a.nfold = num_folds; a.fold_off = fold_off;
  // folds per readout group: the most that fit, at least one; never less than the workspace function promises for an even split (no workspace: 0 bytes)
  return sized_run(h, a, 1, num_folds, spa3d_score_folds_workspace_bytes(h, b->N, b->T, num_folds), ws, ws ? ws_bytes : 0, stream,
                   [&](int64_t need) { return refuse("workspace too small: need " + std::to_string(need) + " bytes"); });
}
int spa3d_score_from_preds(spa3d_handle h, const spa3d_batch* b, const spa3d_outputs* preds, spa3d_scores* scores, void* stream) {
  if (!h) return SPA3D_ERR_ARG;
  h->hip_err = 0;
  const int rc = check_scores(h, b, scores);
  if (rc) return rc;
  if (!preds || !preds->tracks || !preds->visible_logits) { h->err = "score: predictions (tracks, visible_logits) are required"; return SPA3D_ERR_ARG; }
  if (b->B <= 0 || b->Q <= 0) { h->err = "batch: B,Q must be positive"; return SPA3D_ERR_ARG; }
  const int32_t* cq = nullptr;
  if (h->has_cnt_q && !(cq = checked_query_counts(h, b->B, b->Q))) return SPA3D_ERR_ARG;
  h->stream = (hipStream_t)stream; h->dry = false;
  const int To = h->cfg.num_output_frames;
  ScoreArgs s = score_args(b, scores, To, h->cfg.model_kind == 1 ? 2 : 3);
  s.tracks = preds->tracks; s.vlog = preds->visible_logits;
  for_each_live_span(cq, b->B, b->Q, [&](int64_t row0, int64_t nq) {  // live queries only; a sample's padded rows read as 0
    s.nq = nq; s.row0 = row0;
    k_score_rows(h, s);
    if (cq) score_zero_rows(h, scores, row0 + nq, b->Q - nq, To);
  });
  if (scores->sample_stats) k_score_reduce(h, scores->query_stats, b->B, b->Q, scores->num_thresholds, scores->sample_stats);
  return h->hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}

int spa3d_loss_and_grads(spa3d_handle h, const float* params, const spa3d_batch* b, float denom, float* grads, int32_t accumulate,
                         float* loss3, spa3d_outputs* out, void* ws, int64_t ws_bytes, void* stream) {
  if (!h || !params || !grads) return SPA3D_ERR_ARG;
  if (accumulate && h->loss_scale != 1.f) { h->err = "accumulate=1 is not supported with a loss scale (fp16 mode)"; return SPA3D_ERR_ARG; }
  RunArgs a{}; a.mode = MODE_TRAIN; a.P = params; a.b = b; a.denom = denom; a.G = grads; a.accumulate = accumulate; a.loss3 = loss3; a.out = out;
  return run(h, a, ws, ws_bytes, stream);
}

int spa3d_loss(spa3d_handle h, const spa3d_batch* b, const spa3d_outputs* preds, float denom, float* loss3, void* stream) {
  if (!h || !b || !preds || !loss3 || !preds->tracks || !preds->visible_logits || !b->query_tracks || !b->query_tracks_visible)
    return SPA3D_ERR_ARG;
  h->err.clear(); h->hip_err = 0; h->stream = (hipStream_t)stream; h->dry = false;
  if (((uintptr_t)loss3) & 7) { h->err = "loss3 must be 8-byte aligned"; return SPA3D_ERR_ARG; }
  float* scratch = loss3 + 4;  // loss3 points at 12 floats: [0..2] results, [3] sticky non-finite flag, [4..9] three 64-bit fixed-point accumulators, [10] denominator
  unsigned* poison = (unsigned*)(loss3 + 3);
  const int To = h->cfg.num_output_frames, NC = h->cfg.model_kind == 1 ? 2 : 3;
  const int32_t* cq = nullptr;
  if (h->has_cnt_q && !(cq = checked_query_counts(h, b->B, b->Q))) return SPA3D_ERR_ARG;
  if (!weights_fit_batch(h, b->B, b->Q)) return SPA3D_ERR_ARG;
  k_zero(h, loss3 + 3, 36);
  // live queries only: the whole batch at once, or sample by sample (the sums are order-independent fixed-point sums)
  for_each_live_span(cq, b->B, b->Q, [&](int64_t row0, int64_t nq) { k_vis_count(h, b->query_tracks_visible + row0 * To, nq * To, scratch + 4, poison); });
  k_set_denom(h, scratch, poison, denom, scratch + 6);
  for_each_live_span(cq, b->B, b->Q, [&](int64_t row0, int64_t nq) {
    const int64_t r = row0 * To;
    k_loss_from_preds(h, preds->tracks + r * NC, preds->visible_logits + r, nq * To, b->query_tracks + r * NC, b->query_tracks_visible + r, scratch, poison, NC,
                      h->loss, at_rows(h->pt_w, r));
  });
  k_loss_finalize(h, scratch, poison, scratch + 6, h->loss.l1_weight, h->loss.bce_weight, loss3);
  return h->hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}

// The head loss of the train path on its own (tests/test_gpu_loss_ops.py): the launchers run_body / emit_outputs / backward_queries call, in their order,
// on one span of nq rows.  loss3[4..11] is laid out as run_body's `sums` block: accumulators, denominator, loss scale; [3] is the sticky flag.
int spa3d_op_head_loss(spa3d_handle h, const float* head, int64_t nq, const float* targets, const float* visible, float denom, const spa3d_outputs* out,
                       float* loss3, void* dhead, void* stream) {
  if (!h) return SPA3D_ERR_ARG;
  h->err.clear(); h->hip_err = 0;
  auto refuse = [&](const std::string& m) { h->err = "op_head_loss: " + m; return SPA3D_ERR_ARG; };
  if (!head || !targets || !visible || !loss3) return refuse("head, targets, visible and loss3 are required");
  if (nq < 0) return refuse("nq = " + std::to_string(nq) + " is negative");
  if (((uintptr_t)loss3) & 7) return refuse("loss3 must be 8-byte aligned");
  if (h->pt_w && (int64_t)h->pt_B * h->pt_Q != nq)
    return refuse("point weights were set for B = " + std::to_string(h->pt_B) + ", Q = " + std::to_string(h->pt_Q) + ", this call has nq = " + std::to_string(nq));
  if (nq == 0) return SPA3D_OK;
  h->stream = (hipStream_t)stream; h->dry = false;
  const int To = h->cfg.num_output_frames, NC = h->cfg.model_kind == 1 ? 2 : 3;
  float* sums = loss3 + 4; float* denom_dev = sums + 6;
  unsigned* poison = (unsigned*)(loss3 + 3);
  const bool scaled = h->loss_scale != 1.f;
  k_zero(h, loss3 + 3, 36);
  k_vis_count(h, visible, nq * To, sums + 4, poison);
  k_set_denom(h, sums, poison, denom, denom_dev);
  if (scaled) k_set_loss_scale(h, denom_dev, h->loss_gmax, h->loss_scale, denom_dev + 1);
  else if (hipMemsetD32Async((hipDeviceptr_t)(denom_dev + 1), 0x3f800000, 1, h->stream) != hipSuccess && !h->hip_err) { h->hip_err = -7; h->err = "op_head_loss: writing loss3[11] failed"; }
  k_loss_fwd(h, head, nq, To, targets, visible, out ? out->tracks : nullptr, out ? out->visible_logits : nullptr, out ? out->certain_logits : nullptr, sums, poison, NC,
             h->loss, h->pt_w);
  if (dhead) {
    const float* sc = scaled ? denom_dev + 1 : nullptr;
    if (h->cfg.precision == SPA3D_F32) k_loss_bwd<float>(h, head, nq, To, targets, visible, denom_dev, h->loss, h->pt_w, (float*)dhead, NC, sc);
    else if (h->cfg.precision == SPA3D_F16) h_f16::k_loss_bwd<bf16_t>(h, head, nq, To, targets, visible, denom_dev, h->loss, h->pt_w, (bf16_t*)dhead, NC, sc);
    else k_loss_bwd<bf16_t>(h, head, nq, To, targets, visible, denom_dev, h->loss, h->pt_w, (bf16_t*)dhead, NC, sc);
  }
  k_loss_finalize(h, sums, poison, denom_dev, h->loss.l1_weight, h->loss.bce_weight, loss3);
  return h->hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}

int spa3d_set_option(spa3d_handle h, const char* name, double value) {
  if (!h || !name) return SPA3D_ERR_ARG;
  const std::string n(name);
  if (n == "prune") h->prune = value != 0;
  else if (n == "ro_share") h->ro_share = value != 0;
  else if (n == "loss_scale") { if (h->cfg.precision != SPA3D_F16) { h->err = "loss_scale applies to SPA3D_F16 handles only"; return SPA3D_ERR_ARG; } h->loss_scale = (float)value; }
  else if (n == "attn_impl") h->attn = AttnPolicy::from_impl((int)value);
  else if (n == "gemm_impl") set_gemm_impl(h, (int)value);
  else if (n == "chunk") {
    if (value > 1 && (h->query_chunk > 0 || h->track_chunk > 0)) { h->err = "\"chunk\" > 1 cannot be combined with \"query_chunk\" / \"track_chunk\""; return SPA3D_ERR_ARG; }
    h->chunk = value > 0 ? (int)value : 0;
  }
  else if (n == "query_chunk" || n == "track_chunk") {
    if (!(value >= 0 && value <= 2147483647.0)) { h->err = n + " must be >= 0"; return SPA3D_ERR_ARG; }
    if (value >= 1 && h->chunk > 1) { h->err = "\"" + n + "\" cannot be combined with \"chunk\" > 1 (it implies one sample per chunk)"; return SPA3D_ERR_ARG; }
    (n == "query_chunk" ? h->query_chunk : h->track_chunk) = (int)value;
  }
  else if (n == "poison") h->poison = value != 0;
  else if (n == "det_grads") h->det_grads = value != 0;
  else if (n == "freeze") {
    if (value != 0 && value != 1 && value != 2) { h->err = "freeze must be 0 (nothing frozen), 1 (track encoder side) or 2 (the latent stacks too)"; return SPA3D_ERR_ARG; }
    h->freeze = (int)value;
  }
  else { h->err = "unknown option: " + n; return SPA3D_ERR_ARG; }
  return SPA3D_OK;
}
int spa3d_set_loss_scale_state(spa3d_handle h, const float* state) {
  if (!h) return SPA3D_ERR_ARG;
  h->loss_scale_state = state;
  return SPA3D_OK;
}
int spa3d_set_counts(spa3d_handle h, int32_t B, const int32_t* support_count, const int32_t* query_count) {
  if (!h) return SPA3D_ERR_ARG;
  h->has_cnt_n = h->has_cnt_q = false; h->cnt_n.clear(); h->cnt_q.clear(); h->cnt_B = 0;
  if (!support_count && !query_count) return SPA3D_OK;  // detach
  if (B <= 0) { h->err = "spa3d_set_counts: B must be positive"; return SPA3D_ERR_ARG; }
  h->cnt_B = B;
  if (support_count) { h->cnt_n.assign(support_count, support_count + B); h->has_cnt_n = true; }
  if (query_count) { h->cnt_q.assign(query_count, query_count + B); h->has_cnt_q = true; }
  return SPA3D_OK;
}
// the objective (include/spa3d.h "The training objective"): every refusal leaves the stored configuration as it was
int spa3d_set_loss(spa3d_handle h, const spa3d_loss_config* cfg) {
  if (!h) return SPA3D_ERR_ARG;
  const spa3d_loss_config d = cfg ? *cfg : loss_config_defaults();
  const int NC = h->cfg.model_kind == 1 ? 2 : 3;
  auto refuse = [&](const std::string& m) { h->err = "spa3d_set_loss: " + m; return SPA3D_ERR_ARG; };
  if (d.position_kind != SPA3D_POS_L1 && d.position_kind != SPA3D_POS_HUBER) return refuse("position_kind = " + std::to_string(d.position_kind) + " is neither SPA3D_POS_L1 nor SPA3D_POS_HUBER");
  const bool huber = d.position_kind == SPA3D_POS_HUBER;
  bool finite = std::isfinite(d.l1_weight) && std::isfinite(d.bce_weight) && std::isfinite(d.bce_pos_weight) && (!huber || std::isfinite(d.huber_delta));
  for (int i = 0; i < NC; ++i) finite = finite && std::isfinite(d.axis_weight[i]);
  if (!finite) return refuse("every field must be finite");
  bool negative = d.l1_weight < 0.f || d.bce_weight < 0.f || d.bce_pos_weight < 0.f;
  float amax = 0.f;
  for (int i = 0; i < NC; ++i) { negative = negative || d.axis_weight[i] < 0.f; amax = std::max(amax, d.axis_weight[i]); }
  if (negative) return refuse("l1_weight, bce_weight, axis_weight and bce_pos_weight must not be negative");
  if (huber && !(d.huber_delta > 0.f)) return refuse("huber_delta must be positive with SPA3D_POS_HUBER");
  if (d.l1_weight > 0.f && !(amax > 0.f)) return refuse("l1_weight > 0 needs a positive axis_weight among the model's " + std::to_string(NC) + " coordinates");
  const float gmax = std::max(d.l1_weight * amax, d.bce_weight * std::max(1.f, d.bce_pos_weight));
  if (!(gmax > 0.f && gmax <= 1073741824.f)) return refuse("the largest head gradient max(l1_weight * max axis_weight, bce_weight * max(1, bce_pos_weight)) must lie in (0, 2^30]");
  int e = 0;
  (void)frexp((double)gmax / 5000.0, &e);  // gmax / 5000 = m 2^e, m in [0.5, 1): floor(log2) = e - 1
  h->loss = d; h->loss_gmax = gmax; h->loss_gshift = e - 1;
  return SPA3D_OK;
}
int spa3d_get_loss(spa3d_handle h, spa3d_loss_config* out) {
  if (!h || !out) return SPA3D_ERR_ARG;
  *out = h->loss;
  return SPA3D_OK;
}
int spa3d_set_point_weights(spa3d_handle h, int32_t B, int32_t Q, const float* w) {
  if (!h) return SPA3D_ERR_ARG;
  h->pt_w = nullptr; h->pt_B = h->pt_Q = 0;
  if (!w) return SPA3D_OK;  // detach (B and Q are then ignored)
  if (B <= 0 || Q <= 0) { h->err = "spa3d_set_point_weights: B and Q must be positive"; return SPA3D_ERR_ARG; }
  h->pt_w = w; h->pt_B = B; h->pt_Q = Q;
  return SPA3D_OK;
}
int spa3d_grad_segments(spa3d_handle h, int64_t* bounds4) {
  if (!h || !bounds4) return SPA3D_ERR_ARG;
  int64_t b1 = -1, b2 = -1;
  for (auto& l : h->leaves) {
    if (b1 < 0 && l.name.rfind("tracks_to_latents/", 0) == 0) b1 = l.offset;
    if (b2 < 0 && l.name.rfind("track_readout_attn/", 0) == 0) b2 = l.offset;
  }
  if (b1 < 0 || b2 < b1) return SPA3D_ERR_ARG;
  bounds4[0] = 0; bounds4[1] = b1; bounds4[2] = b2; bounds4[3] = h->nparams;
  return SPA3D_OK;
}
int spa3d_trainable_range(spa3d_handle h, int64_t* lo_n) {
  int64_t b4[4];
  if (!h || !lo_n || spa3d_grad_segments(h, b4) != SPA3D_OK) return SPA3D_ERR_ARG;
  lo_n[0] = b4[h->freeze]; lo_n[1] = b4[3];
  return SPA3D_OK;
}
int spa3d_grad_events_recorded(spa3d_handle h, int64_t* out4) {
  if (!h || !out4) return SPA3D_ERR_ARG;
  out4[0] = h->grad_ev_gen[0]; out4[1] = h->grad_ev_gen[1]; out4[2] = (int64_t)(intptr_t)h->grad_ev[0]; out4[3] = (int64_t)(intptr_t)h->grad_ev[1];
  return SPA3D_OK;
}
int spa3d_detach(spa3d_handle h, void* ev_readout, void* ev_latents, const float* loss_scale_state) {
  if (!h) return SPA3D_ERR_ARG;
  if (ev_readout && h->grad_ev[0] == ev_readout && h->grad_ev[1] == ev_latents) { h->grad_ev[0] = nullptr; h->grad_ev[1] = nullptr; }
  if (loss_scale_state && h->loss_scale_state == loss_scale_state) h->loss_scale_state = nullptr;
  return SPA3D_OK;
}
int spa3d_set_grad_events(spa3d_handle h, void* ev_readout, void* ev_latents) {
  if (!h) return SPA3D_ERR_ARG;
  h->grad_ev[0] = ev_readout; h->grad_ev[1] = ev_latents;
  return SPA3D_OK;
}
int spa3d_plan_stats(spa3d_handle h, double* out4) {
  if (!h || !out4) return SPA3D_ERR_ARG;
  for (int i = 0; i < 4; ++i) out4[i] = h->plan_stats[i];
  return SPA3D_OK;
}

int spa3d_prof_enable(spa3d_handle h, int32_t on) {
  if (!h) return SPA3D_ERR_ARG;
  h->prof.on = on != 0; h->prof.used = 0; h->prof.recs.clear();
  return SPA3D_OK;
}
int spa3d_prof_read(spa3d_handle h, int32_t cls, double* out4) {
  if (!h || !out4 || cls < 0 || cls >= PROF_NCLS) return SPA3D_ERR_ARG;
  double n = 0, ms = 0, fl = 0, by = 0;
  for (auto& r : h->prof.recs) {
    if (r.cls != cls) continue;
    if (hipEventSynchronize(r.e1) != hipSuccess) return SPA3D_ERR_HIP;
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.e0, r.e1) != hipSuccess) return SPA3D_ERR_HIP;
    n += 1; ms += t; fl += r.flops; by += r.bytes;
  }
  out4[0] = n; out4[1] = ms; out4[2] = fl; out4[3] = by;
  return SPA3D_OK;
}

// one CSV line per profiled launch group: cls,ms,flops,bytes,tag0..3 (include/spa3d.h)
int spa3d_prof_dump(spa3d_handle h, const char* path) {
  if (!h || !path) return SPA3D_ERR_ARG;
  FILE* f = fopen(path, "w");
  if (!f) return SPA3D_ERR_ARG;
  for (auto& r : h->prof.recs) {
    float t = 0.f;
    if (hipEventSynchronize(r.e1) != hipSuccess || hipEventElapsedTime(&t, r.e0, r.e1) != hipSuccess) { fclose(f); return SPA3D_ERR_HIP; }
    fprintf(f, "%d,%.6f,%.6g,%.6g,%lld,%lld,%lld,%lld\n", r.cls, t, r.flops, r.bytes, (long long)r.tag[0], (long long)r.tag[1], (long long)r.tag[2], (long long)r.tag[3]);
  }
  fclose(f);
  return SPA3D_OK;
}

int spa3d_adamw_step(float* params, const float* grads, float* m, float* v, int64_t n, float lr, int64_t step, float clip, float b1,
                     float b2, float eps, float wd, float* scratch, void* stream) {
  if (!params || !grads || !m || !v || !scratch || n <= 0) return SPA3D_ERR_ARG;
  spa3d_ctx c; c.stream = (hipStream_t)stream;
  k_adamw(&c, params, grads, m, v, n, lr, step, clip, b1, b2, eps, wd, scratch);
  return c.hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}
int64_t spa3d_adamw_groups_workspace_bytes(int32_t num_groups) {
  if (num_groups < 0 || num_groups > ADAMW_MAX_GROUPS) return -1;
  return adamw_groups_ws_bytes(num_groups);
}
static_assert(sizeof(spa3d_param_group) == sizeof(AdamwGroup) && offsetof(spa3d_param_group, end) == offsetof(AdamwGroup, end) &&
              offsetof(spa3d_param_group, lr_scale) == offsetof(AdamwGroup, lr_scale) && offsetof(spa3d_param_group, wd_scale) == offsetof(AdamwGroup, wd_scale),
              "the kernels read the caller's table as AdamwGroup (adamw_groups.hpp)");
int spa3d_adamw_step_groups(float* params, const float* grads, float* m, float* v, int64_t n, float lr, int64_t step, float clip, float b1,
                            float b2, float eps, float wd, const spa3d_param_group* groups, int32_t num_groups, float* ema, float ema_decay,
                            float* scratch, void* ws, int64_t ws_bytes, void* stream) {
  // every refusal comes before the first launch (include/spa3d.h)
  if (!params || !grads || !m || !v || !scratch || n < 0) return SPA3D_ERR_ARG;
  if (adamw_groups_check(groups, num_groups, n) != ADAMW_G_OK) return SPA3D_ERR_ARG;
  if (ema && !(ema_decay >= 0.f && ema_decay < 1.f)) return SPA3D_ERR_ARG;   // (NaN fails both comparisons)
  if (num_groups > 0 && (!ws || ws_bytes < adamw_groups_ws_bytes(num_groups))) return SPA3D_ERR_WORKSPACE;
  if (n == 0) return SPA3D_OK;
  spa3d_ctx c; c.stream = (hipStream_t)stream;
  k_adamw_groups(&c, params, grads, m, v, n, lr, step, clip, b1, b2, eps, wd, reinterpret_cast<const AdamwGroup*>(groups), num_groups, ema, ema_decay, scratch, ws);
  return c.hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}
int spa3d_uniform_noise(float* out, int64_t n, uint32_t key0, uint32_t key1, void* stream) {
  if (!out || n <= 0) return SPA3D_ERR_ARG;
  spa3d_ctx c; c.stream = (hipStream_t)stream;
  k_uniform_noise(&c, out, n, key0, key1);
  return c.hip_err ? SPA3D_ERR_HIP : SPA3D_OK;
}

}  // extern "C"
#endif  // !SPA_F16
