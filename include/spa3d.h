/* spa3d.h -- C-ABI of libspa3d_hip.so: the MI355X (gfx950) implementation of the 3DSPA
 * TrackAutoEncoder3D train-step hot path.
 *
 * The reference (TheProParadox/3dspa_code) has no FFI: its boundary is the Flax module
 * protocol.  Each entry point below names the reference call it replaces:
 *
 *   spa3d_create / spa3d_leaf_*     TrackAutoEncoder3D(...) + model.init(rng, batch)['params']
 *                                   track_autoencoder_3d.py:43-115, train.py:221-233
 *   spa3d_encode                    TrackAutoEncoder3D.encode            track_autoencoder_3d.py:190-204
 *   spa3d_decode                    get_decoder_context + decode         track_autoencoder_3d.py:206-307
 *   spa3d_forward                   model.apply({'params': p}, batch)    track_autoencoder_3d.py:309-357
 *   spa3d_loss                      compute_loss_3d                      train.py:96-129
 *   spa3d_loss_and_grads            jax.value_and_grad(loss_fn)(params)  train.py:134-162
 *   spa3d_adamw_step                optax.chain(clip_by_global_norm(1.0), adamw(lr, 0.01)) + apply_updates
 *                                   train.py:164-165,239-242 (intended semantics, repair R6)
 *   spa3d_adamw_step_groups         the same chain with per-range learning-rate / weight-decay scales, frozen ranges and a weight EMA
 *                                   (optax.masked / multi_transform / ema; nothing in the reference: fine-tuning, product-only)
 *   spa3d_tapvid3d_from_preds      tapvid3d_metrics.compute_tapvid3d_metrics(...)  evaluate_tapvid3d.py:99-109,196-208
 *                                   (third-party arithmetic upstream: restated from the published definition, parity unpinned)
 *   spa3d_render_tracks             project_all_tracks + normalize_scores + paint_point_track_with_colors
 *                                   visualize.py:15-175, visualizer.py:23-45,149-200 (own integer rasteriser, not cv2's)
 *   spa3d_render_heatmap            dense per-frame maps of the track values (nothing in the reference: the library's own definition)
 *   spa3d_build_batch               split + lift_2d_to_3d + sample_*_features_for_tracks + batch dict, for many clips at once
 *                                   inference.py:541-590, data_loader.py:56-110
 *   spa3d_uniform_noise             jax.random.uniform(PRNGKey(0), shape) track_autoencoder_3d.py:254-257
 *   spa3d_op_*                      single building blocks (attention.py, track_autoencoder.py:18-38),
 *                                   exported so tests can check each kernel against the oracle.
 *
 * Rules: plain C; every function returns an int status (0 = ok) and never throws; no
 * allocation inside (the caller supplies one workspace from its own allocator); every call
 * is asynchronous on the hipStream_t passed as `void* stream` -- except that, in the 16-bit
 * modes, two 4-byte plan counts per sample chunk (kept frame tokens; distinct query frames) are
 * read back to the host, which synchronises the stream at those points (spa3d_set_option(h, "prune", 0) and
 * spa3d_set_option(h, "ro_share", 0) remove the reads together with the savings they size; no compute path reads the environment --
 * the ten options may only be PRESET from it when spa3d_create runs);
 * one handle per stream (thread-compatible, not thread-safe).  All tensors are row-major contiguous in the
 * reference's layouts.  Parameters and gradients are ONE flat float32 buffer each whose
 * leaf order / offsets the library defines (spa3d_leaf_*); names are the Flax paths of
 * SURVEY.md 0.3 and shapes are Flax shapes ([in,out] kernels, [in,H,Dh] / [H,Dh,out]).
 */
#ifndef SPA3D_H_
#define SPA3D_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPA3D_OK 0
#define SPA3D_ERR_ARG 1      /* bad argument / unsupported shape           */
#define SPA3D_ERR_WORKSPACE 2 /* workspace too small for even one sample    */
#define SPA3D_ERR_HIP 3      /* a HIP runtime call or launch failed        */

#define SPA3D_F32 0  /* exact-fp32 path: v_mfma_f32_16x16x4_f32, fp32 activations (parity runs) */
#define SPA3D_BF16 1 /* bf16 activations + bf16 MFMA, fp32 accumulate, fp32 master params/grads  */
#define SPA3D_F16 2  /* IEEE fp16 activations + fp16 MFMA (same rate), fp32 accumulate / master params/grads; the 16-bit backward
                        runs at loss x 2^k (k per call from the loss denominator), BASELINE.json configs[4] */

typedef struct spa3d_ctx* spa3d_handle;

/* Hyper-parameters: fields of TrackAutoEncoder3D (track_autoencoder_3d.py:53-67) plus the
 * transformer sizes hard-coded in setup() (:89-112) and the compute precision. */
typedef struct {
  int32_t num_output_frames;   /* 150 */
  int32_t num_latent_tokens;   /* 128 */
  int32_t latent_token_dim;    /* 96  */
  int32_t num_frequencies;     /* 32  */
  float track_scale_factor;    /* 1.0 */
  float time_scale_factor;     /* 150.0 */
  int32_t track_token_dim;     /* 384 */
  int32_t encoder_latent_dim;  /* 512 */
  int32_t decoder_num_channels;/* 1280 */
  int32_t dino_feature_dim;    /* 768; 0 = no dino_projection leaf (use_dino False / key absent) */
  int32_t depth_feature_dim;   /* channels of depth_features actually fed; 0 = no depth_projection */
  int32_t num_heads;           /* 8 */
  int32_t qkv_size;            /* 768; qkv_size / num_heads must be one of 8, 16, 32, 64, 96, 128 (spa3d_create: SPA3D_ERR_ARG otherwise) */
  int32_t enc_mlp, enc_layers; /* 1536, 3 */
  int32_t t2l_mlp, t2l_layers; /* 2048, 4 */
  int32_t dec_mlp, dec_layers; /* 2048, 4 */
  int32_t ro_mlp, ro_layers;   /* 1536, 4 */
  int32_t precision;           /* SPA3D_F32 | SPA3D_BF16 | SPA3D_F16 */
  int32_t model_kind;          /* 0 = TrackAutoEncoder3D (track_autoencoder_3d.py:43-357);
                                  1 = the 2-D TRAJAN twin TrackAutoEncoder (track_autoencoder.py:117-390): 2 coordinates, no readout
                                      token, visible-mean pooling, certainty head; dino/depth dims must be 0.  Tensors then carry 2
                                      coordinates ([..,2] tracks, [B,Q,3] query points) */
} spa3d_config;

/* One batch: TrackAutoEncoder3DInputs (track_autoencoder_3d.py:23-40) + the loss targets
 * read from the same dict (train.py:99-100).  Device pointers. */
typedef struct {
  int32_t B, N, Q, T;
  const float* support_tracks;          /* [B,N,T,3] f32 */
  const float* support_tracks_visible;  /* [B,N,T,1] f32, 0/1 */
  const float* query_points;            /* [B,Q,4] f32 (t,x,y,z); required (host builds the default grid) */
  const int32_t* boundary_frame;        /* [B] */
  const void* dino_features;            /* [B,N,T,dino_feature_dim] or NULL; f32 in F32 mode, bf16 in BF16 mode */
  const void* depth_features;           /* [B,N,T,depth_feature_dim] or NULL; same dtype rule */
  const float* noise;                   /* [B,L,latent_token_dim] uniform [0,1) or NULL */
  int32_t discretize;                   /* decode(discretize=...); with noise==NULL the library draws
                                           spa3d_uniform_noise (legacy threefry layout) itself */
  const float* query_tracks;            /* [B,Q,T,3] f32 targets (loss entry points only) */
  const float* query_tracks_visible;    /* [B,Q,T,1] f32 targets */
} spa3d_batch;

/* TrackAutoEncoderResults (track_autoencoder.py:72-91); certain_logits is identically 0. */
typedef struct {
  float* tracks;          /* [B,Q,T_out,3] f32 */
  float* visible_logits;  /* [B,Q,T_out,1] f32 */
  float* certain_logits;  /* [B,Q,T_out,1] f32 or NULL */
  float* latents;         /* [B,L,latent_token_dim] f32 or NULL: encode() output */
} spa3d_outputs;

const char* spa3d_version(void);
int spa3d_create(const spa3d_config* cfg, spa3d_handle* out);
int spa3d_destroy(spa3d_handle h);
const char* spa3d_last_error(spa3d_handle h);

/* parameter tree */
int64_t spa3d_param_elems(spa3d_handle h);
int32_t spa3d_num_leaves(spa3d_handle h);
/* name: >=160 bytes; shape: >=4 int64; offset in floats into the flat buffer */
int spa3d_leaf_info(spa3d_handle h, int32_t i, char* name, int32_t* ndim, int64_t* shape, int64_t* offset);

/* Bytes of workspace needed to process `chunk` samples at a time (1 <= chunk <= B) of a
 * [B,N,Q,T] batch; train!=0 sizes forward+backward, else forward only. */
int64_t spa3d_workspace_bytes(spa3d_handle h, int32_t B, int32_t N, int32_t Q, int32_t T, int32_t chunk, int32_t train);

int spa3d_encode(spa3d_handle h, const float* params, const spa3d_batch* b, float* latents,
                 void* ws, int64_t ws_bytes, void* stream);
int spa3d_decode(spa3d_handle h, const float* params, const spa3d_batch* b, const float* latents,
                 spa3d_outputs* out, void* ws, int64_t ws_bytes, void* stream);
int spa3d_forward(spa3d_handle h, const float* params, const spa3d_batch* b, spa3d_outputs* out,
                  void* ws, int64_t ws_bytes, void* stream);

/* loss3 (device, >= 12 floats, 8-byte aligned: [0..2] = total, position, visible; the rest is scratch -- [3] a sticky flag word
 * that any non-finite partial sum sets, after which all three results are NaN).
 * denom<=0: use max(sum(visible),1) of this batch.  The batch sums are order-independent (64-bit fixed-point accumulation): the same
 * inputs give the same bits on every run and on every data-parallel replica. */
int spa3d_loss(spa3d_handle h, const spa3d_batch* b, const spa3d_outputs* preds, float denom,
               float* loss3, void* stream);

/* The head loss of spa3d_loss_and_grads on its own: the launches that call makes between the head GEMM and the head's backward, in its order, on
 * nq query rows of head[q][c * T_out + t] (c < NC coordinates, then the visibility logit; the 2-D twin's 4th block: certainty logits).
 * Reads from the handle: num_output_frames, the model kind (NC), the precision, the objective (spa3d_set_loss), the point-weight plane
 * (spa3d_set_point_weights, stated for B * Q == nq), the "loss_scale" option and the loss-scale state (spa3d_set_loss_scale_state).
 * spa3d_set_counts is IGNORED: all nq rows are live.
 *   out    NULL, or the split predictions to write: tracks [nq,T_out,NC], visible_logits and certain_logits [nq,T_out] (zeros on the 3-D model);
 *          NULL members are not written, latents is not looked at.
 *   loss3  device, 12 floats, 8-byte aligned, as spa3d_loss; additionally [10] = the denominator used and [11] = the loss scale used (1 when the
 *          handle's "loss_scale" is 1, whatever the state: the train call then runs unscaled).
 *   dhead  NULL, or [nq, 4 * T_out] in the handle's storage type (fp32 / bf16 / fp16): the head cotangent times the loss scale.
 * SPA3D_ERR_ARG with a message, before the first launch: a NULL handle, head, targets, visible or loss3; nq < 0; loss3 not 8-byte aligned; a weight
 * plane with B * Q != nq.  nq == 0 is SPA3D_OK and launches nothing. */
int spa3d_op_head_loss(spa3d_handle h, const float* head /* [nq, 4*T_out] */, int64_t nq, const float* targets /* [nq,T_out,NC] */,
                       const float* visible /* [nq,T_out] */, float denom, const spa3d_outputs* out, float* loss3, void* dhead, void* stream);

/* Per-track reconstruction scores (no reference counterpart in the model code: upstream's tooling consumes per-point scores, and this is
 * what produces them).  For every query row, over its T_out frames, in fp32: e1 = sum_c |p - g| (the training loss's L1), e2 = the
 * Euclidean distance sqrtf(sum_c (p - g)^2), pv = visible_logit > 0, vis = target visibility y > 0.5, bce as in spa3d_loss.
 * query_stats row of S = 8 + 4K floats (K = num_thresholds):
 *   [0] n_vis = sum vis   [1] sum y e1   [2] sum y e2   [3] max of e2 over vis frames (0 if none)   [4] sum bce
 *   [5] sum [pv == vis] (occlusion-correct frames)   [6] sum pv   [7] T_out on a live row, 0 on a padded row
 *   [8 + 4k] W_k  = sum [vis and e2 < thresholds[k] * scale_b]        [9 + 4k]  TP_k = sum [vis and pv and e2 < thresholds[k] * scale_b]
 *   [10 + 4k] FP_k = sum [pv and not (vis and e2 < ...)]              [11 + 4k] FN_k = sum [vis and not (pv and e2 < ...)]
 * (TP_k + FN_k = [0] and TP_k + FP_k = [6] on every row.)  These are the TAP-Vid Jaccard counts with FIXED metric thresholds.  This is NOT
 * tapnet's TAPVid-3D metric (that is spa3d_tapvid3d_from_preds below): there is no depth-dependent threshold and no median rescaling;
 * sample_scale (one factor per sample on every threshold, default 1) is the hook for scene-relative thresholds.
 * sample_stats[b] = the sample's rows pooled in double (sums; [3] a max; [7] = T_out x live queries).  frame_err[q][t] = e2 of every frame,
 * whatever y is.  One wave per row and fixed-order reductions, no atomics: the same inputs give the same bits on every run, and
 * spa3d_score_from_preds on the predictions a spa3d_score call returned gives that call's bits.
 * With per-sample counts (spa3d_set_counts) the rows of padded queries are written as 0 in query_stats and frame_err, and targets at or
 * beyond a count are never read. */
typedef struct {
  int32_t num_thresholds;          /* 0..8 */
  float   thresholds[8];           /* finite, > 0 */
  const float* sample_scale;       /* device [B] or NULL */
  float*  query_stats;             /* device [B,Q,8+4K] f32, required */
  double* sample_stats;            /* device [B,8+4K] f64 or NULL */
  float*  frame_err;               /* device [B,Q,T_out] f32 or NULL */
} spa3d_scores;

/* spa3d_forward with the scores of its predictions against the batch's targets (required) computed on the way out, from the same head
 * buffer the outputs are split from.  No stash and no backward: spa3d_workspace_bytes(..., train = 0) is a sufficient workspace.  out may
 * be NULL: no [B,Q,T_out,.] prediction tensor is written then.  Works with every precision, model_kind, option and with per-sample counts
 * as spa3d_forward does (same refusals).  SPA3D_ERR_ARG with a message, before the first launch: missing targets, query_stats == NULL,
 * num_thresholds outside 0..8, a threshold that is not finite and positive. */
int spa3d_score(spa3d_handle h, const float* params, const spa3d_batch* b, spa3d_scores* scores, spa3d_outputs* out,
                void* ws, int64_t ws_bytes, void* stream);
/* The same scores from already-split predictions (as spa3d_loss): reads B, Q, the targets and the query counts only. */
int spa3d_score_from_preds(spa3d_handle h, const spa3d_batch* b, const spa3d_outputs* preds, spa3d_scores* scores, void* stream);

/* Scores for EVERY track of a clip in one call: a leave-fold-out round.  The clip's N tracks are cut into num_folds contiguous folds
 * [fold_off[f], fold_off[f + 1]); the tracks of fold f are reconstructed from the tracks outside it, and the per-point error is their score (what
 * upstream's visualiser paints as coords_score).  A caller who wants random folds shuffles the tracks beforehand (spa3d_build_batch with index
 * lists does that); the same fold_off (HOST, num_folds + 1 entries) applies to every clip of the batch.
 *   Batch: Q == N -- query row q of a clip IS its track q; query_points [B,N,4] required.  query_tracks and query_tracks_visible may both be
 * NULL: the targets are then support_tracks / support_tracks_visible themselves (no copy), which needs T == num_output_frames.
 *   Results: rows [fold_off[f], fold_off[f + 1]) of every output and of query_stats / frame_err are what spa3d_score gives on the batch whose
 * support tracks are the clip's tracks outside that range, in their order, and whose queries are the rows of that range (same noise[b],
 * boundary_frame[b] and options), up to the order of summation.  sample_stats[b] pools all N rows of the clip.  out may be NULL as in spa3d_score;
 * out->latents is not written (a clip has num_folds latent sets).  Two runs give the same bits: no float atomics.
 *   Work: the track encoder is per track, so it runs ONCE per clip over all N tracks, addressed in place (token pruning as usual) -- not num_folds
 * times over N (1 - 1 / num_folds).  The latent stacks run on num_folds sequences that share the encoder's output rows: the K / V projection of each
 * tracks_to_latents block runs once over the N rows, and its cross attention lets sequence f skip the rows of fold f (one launch of the chunked-key
 * kernel, keys addressed by logical position, so a sequence's result is bit for bit that of the kernel on a compacted copy of its keys; the
 * fp32 parity mode and attn_impl 1 run the sequences one by one on such a copy).  The readout decodes every track once against the latents of its
 * own fold, the first block dense as in a packed chunk, over groups of consecutive folds: as many folds per group as fit the workspace, released
 * between groups; the latent stages always run all folds at once.  spa3d_plan_stats reports out4[1] = sum over clips of N x (T + 1),
 * out4[3] = sum over clips of N.  "chunk" is ignored (clips are processed one at a time); "prune", "poison", "attn_impl", "gemm_impl" and the three
 * precisions work as elsewhere.  Asynchronous, allocates nothing, reads back nothing but the prune count.
 *   spa3d_score_folds_workspace_bytes: the bytes for the near-equal split of N into num_folds (sizes N / num_folds, the first N % num_folds one larger)
 * with the readout one fold at a time; -1 for arguments the call would refuse.  A larger workspace lets the readout take more folds per group.
 * (A call that leaves noise NULL with discretize set draws the noise of all B clips into the workspace first: B x L x latent_token_dim x 4 bytes more.)
 *   SPA3D_ERR_ARG with a message, before the first launch: Q != N; num_folds outside [2, 64], fold_off[0] != 0, fold_off not strictly increasing,
 * fold_off[num_folds] != N; NULL targets with T != num_output_frames; a model_kind 1 handle; stored per-sample counts (spa3d_set_counts);
 * "track_chunk" or "query_chunk" set; a workspace below what the workspace function returns, or below what this call's own folds need (the
 * message names the bytes); the spa3d_scores refusals of spa3d_score. */
int64_t spa3d_score_folds_workspace_bytes(spa3d_handle h, int32_t N, int32_t T, int32_t num_folds);
int spa3d_score_folds(spa3d_handle h, const float* params, const spa3d_batch* b,
                      int32_t num_folds, const int32_t* fold_off /* HOST [num_folds + 1] */,
                      spa3d_scores* scores, spa3d_outputs* out /* may be NULL */,
                      void* ws, int64_t ws_bytes, void* stream);

/* TAPVid-3D metrics of existing predictions against the batch's targets: occlusion accuracy, points-within and Jaccard counts at the pixel
 * thresholds 1, 2, 4, 8, 16, with the predictions rescaled first.  tapnet, whose compute_tapvid3d_metrics upstream calls, is not vendored by
 * the reference: what follows is restated from the published definition, parity unpinned, and is the contract.
 * fp32, per sample b, over the sample's live query rows; p, l = preds->tracks, preds->visible_logits, g, y = the batch's targets:
 *   tq    = clamp(lrintf(query_points[b,q,0]), 0, T_out - 1); ew[q][t] = (t != tq): the query frame is left out of every count
 *   gn    = sqrtf(fmaxf(1e-12f, sum_c g^2)), pn alike; ratio[q][t] = gn / pn, for every frame of a live row whatever y is
 *   scaling SPA3D_SCALE_NONE: s = 1.  SPA3D_SCALE_MEDIAN: s_b = the exact median of ratio over the sample's {y > 0.5 and ew} (the middle
 *   value; 0.5f a + 0.5f b of the two middle values for an even count; 1 for an empty set; a NaN ratio is not part of the set).
 *   SPA3D_SCALE_PER_TRAJECTORY: s_q = ratio[q][tq].  Scaled prediction ps = p * s, rounded once per coordinate.
 *   thr   = px * (g_z / f_b), f_b = sqrtf(fx fy + 1e-12f), px in {1, 2, 4, 8, 16}; intrinsics == NULL means (256, 256, 128, 128)
 *           (evaluate_tapvid3d.py:97); fixed_thresholds != 0 uses the metric table 0.01, 0.04, 0.16, 0.64, 2.56 instead
 *   within = sqrtf(sum_c (ps - g)^2) < thr (a non-positive threshold matches nothing); pv = l > 0; vis = y > 0.5
 * query_stats row of 24 floats (exact counts):
 *   [0] sum ew   [1] sum ew vis   [2] sum ew [pv == vis]   [3] sum ew pv
 *   [4 + 4k] W = sum ew vis within   [5 + 4k] TP = sum ew vis pv within   [6 + 4k] FP = sum ew pv not (vis within)   [7 + 4k] FN = sum ew vis not (pv within)
 * (TP + FN = [1] and TP + FP = [3] on every row.)  sample_stats[b] = the sample's rows summed in double in a fixed order.  The per-video
 * metrics are ratios of the pooled counts, taken by the caller: occlusion_accuracy = [2] / [0], pts_within_px = W / [1],
 * jaccard_px = TP / ([1] + FP), and the two averages over the five thresholds.
 * The median is a radix select over the bit patterns with integer counts, the rows are one wave each with fixed-order reductions: no float
 * atomics, the same inputs give the same bits on every run.  With per-sample counts (spa3d_set_counts) the rows of padded queries are written
 * as 0 in query_stats, row_scale and ratio, their inputs are never read, and they are not part of the median.
 * This differs from spa3d_scores, which has fixed per-sample thresholds, no rescaling, and counts the query frame. */
#define SPA3D_SCALE_NONE 0
#define SPA3D_SCALE_MEDIAN 1
#define SPA3D_SCALE_PER_TRAJECTORY 2
typedef struct {
  int32_t scaling, fixed_thresholds;
  const float* intrinsics;   /* device [B,4] (fx, fy, cx, cy) or NULL */
  float*  query_stats;       /* device [B,Q,24], required */
  double* sample_stats;      /* device [B,24] or NULL */
  float*  scale;             /* device [B] or NULL: the factor applied per sample (1 for none / per_trajectory) */
  float*  row_scale;         /* device [B,Q] or NULL: per_trajectory factors (else the sample's factor) */
  float*  ratio;             /* device [B,Q,T_out] or NULL */
} spa3d_tapvid3d;
/* a sufficient workspace for any scaling; T = T_out of the predictions */
int64_t spa3d_tapvid3d_workspace_bytes(spa3d_handle h, int32_t B, int32_t Q, int32_t T);
/* Reads B, Q, query_points, the targets and the query counts of the batch.  Asynchronous, allocates nothing, reads nothing back to the host.
 * SPA3D_ERR_ARG with a message, before the first launch: targets, query_points, predictions or query_stats missing; scaling outside 0..2;
 * a model_kind 1 handle (no depth coordinate); a workspace that is too small (the message names the bytes needed). */
int spa3d_tapvid3d_from_preds(spa3d_handle h, const spa3d_batch* b, const spa3d_outputs* preds, spa3d_tapvid3d* m, void* ws, int64_t ws_bytes,
                              void* stream);

/* Score-coloured track overlays drawn on the device: the counterpart of upstream's visualiser (project_all_tracks, normalize_scores,
 * score_to_color_bgr, paint_point_track_with_colors).  One clip per call; track-major layouts.  Kept from the reference: the primitives, their
 * order, the colours, the projection and the integer pixel positions.  NOT kept: cv2's rasteriser -- LINE_AA and addWeighted are third-party
 * arithmetic, parity with cv2 is not sought.  The rasteriser below is integer-only, so every output byte is defined and this comment is the
 * contract (csrc/render_px.hpp is its only implementation; tests/render_util.py restates it in NumPy).
 *
 * Position of point i in frame t (pixels[i][t], a function of the coordinates alone):
 *   coords == 3, in double, p = (x, y, z) of tracks[i][t] widened to double, K = intrinsics[t], E = extrinsics[t]:
 *     sx = resize_w / W, sy = resize_h / H;  K00 *= sx, K02 *= sx, K11 *= sy, K12 *= sy (the other entries as given)
 *     c_r = ((E[r][0] x + E[r][1] y) + E[r][2] z) + E[r][3]          r = 0..2, added left to right
 *     h_r = (K[r][0] c_0 + K[r][1] c_1) + K[r][2] c_2                r = 0..2
 *     u = h_0 / (h_2 + 1e-8), v = h_1 / (h_2 + 1e-8); NaN and +-inf become 0; u = u / sx, v = v / sy
 *     u clipped to [0, W - 1], v to [0, H - 1], then truncated towards zero
 *   coords == 2: each coordinate truncated towards zero (the reference's int()); a coordinate that is not finite or whose magnitude
 *     exceeds 2^30 leaves the point-frame without a position: pixels reads (INT32_MIN, INT32_MIN) and nothing is drawn from or to it.
 *   A position is in bounds when 0 <= x < W and 0 <= y < H.
 * Colour of (t, i), s = scores[i][t]:
 *   normalize != 0: min and max over the finite scores of the clip; fp32: s' = (s - min) / (max - min) if max > min, else s' = s - min.
 *   normalize == 0: s' = s.  If s or s' is not finite, point i draws nothing in frame t.
 *   score_to_color_bgr in double: q = s' clipped to [0, 1]; q < 0.5: ratio = q / 0.5, (b, g, r) = (int(255 ratio), int(255 ratio), 255);
 *   else ratio = (q - 0.5) / 0.5, (b, g, r) = (255, int(255 (1 - ratio)), int(255 (1 - ratio))).  The three bytes written per pixel are
 *   (b, g, r) when colour_bgr != 0, else (r, g, b).
 * Drawing frame t: points in index order i = 0 .. N-1.  For each point first its segments for p = max(0, t - trail) .. t - 1 in that order,
 *   segment p running from the position at frame p to the position at frame p + 1, each blended on its own; then its dot at the position of
 *   frame t.  Everything of point i in frame t has the colour of (t, i).  A segment is drawn only if both ends are in bounds, a dot only if its
 *   centre is.  visible is ignored unless use_visibility != 0 (upstream ignores it); then a dot needs visible[i][t] > 0.5 and a segment both
 *   ends visible.  Later primitives go over earlier ones.
 * Coverage, in units of 1/8 px: pixel (X, Y) has the 16 samples P = (8X + 2a + 1, 8Y + 2b + 1), a, b in 0..3; the integer position x is the
 *   centre 8x + 4.  Dot of radius r = point_size around C: a sample is inside when |P - C|^2 <= (8r + 4)^2.  Segment A -> B: d = B - A,
 *   L2 = d.d, u = (P - A).d;  u < 0 or L2 == 0: inside when |P - A|^2 <= 16;  u > L2: inside when |P - B|^2 <= 16;  otherwise, with
 *   c = (P - A)_x d_y - (P - A)_y d_x: inside when |c| <= 4 (|d_x| + |d_y|) and c^2 <= 16 L2 (the first test is an exact reject that keeps c^2
 *   within 64 bits at the size limit).  k = the number of inside samples, 0..16.
 * Blend, per channel: w = k a, a = 179 for a segment (0.7 x 256) and 256 for a dot; out = (in (4096 - w) + col w + 2048) >> 12.  A pixel no
 *   primitive touches keeps its input byte.
 * Every pixel is read once and written once by the one thread that owns it (out == video is legal), no atomics on pixels, the min / max is an
 * order-independent reduction: the same inputs give the same bytes on every run. */
typedef struct {
  int32_t N, T, H, W;              /* N, T >= 1; 1 <= H, W <= 16384 */
  const uint8_t* video;            /* device [T,H,W,3], channel order = the caller's; colour_bgr says which */
  uint8_t* out;                    /* device [T,H,W,3]; may be == video (in place).  NULL: only `pixels` is computed (video, scores not read) */
  const float* tracks;             /* device [N,T,3] camera/world points, or [N,T,2] pixel coordinates when coords == 2 */
  int32_t coords;                  /* 2 | 3 */
  const double* intrinsics;        /* device [T,3,3], coords == 3 only */
  const double* extrinsics;        /* device [T,4,4], coords == 3 only */
  int32_t resize_h, resize_w;      /* project_all_tracks' resize_height / resize_width (1024, 1024); >= 1, coords == 3 only */
  const float* scores;             /* device [N,T] */
  const float* visible;            /* device [N,T] or NULL */
  int32_t normalize, use_visibility, colour_bgr, trail, point_size;   /* trail 0..32, point_size 0..32 */
  int32_t* pixels;                 /* device [N,T,2] or NULL: the integer positions used (x, y), INT32_MIN for "no position" */
} spa3d_render;
/* a sufficient workspace for any option */
int64_t spa3d_render_workspace_bytes(spa3d_handle h, int32_t N, int32_t T);
/* Asynchronous, allocates nothing, reads nothing back to the host.  SPA3D_ERR_ARG with a message, before the first launch: a missing pointer
 * (tracks; video and scores when out is given; out and pixels both NULL; visible with use_visibility), coords outside {2, 3}, camera matrices
 * or resize missing with coords == 3, a size, trail or point_size out of range, a workspace that is too small (the message names the bytes
 * needed), more than 2^31 point-frames, or, when frames are drawn, 2^24 or more (frame, 64 x 16 tile) pairs: what one launch holds. */
int spa3d_render_tracks(spa3d_handle h, const spa3d_render* r, void* ws, int64_t ws_bytes, void* stream);

/* Dense per-frame score maps from track values: per pixel the kernel-weighted average of the values of the tracks around it, NaN where no
 * track is near, and optionally a translucent overlay of that map on the video.  The library's own definition -- the reference has no
 * counterpart (its visualiser paints dots, spa3d_render_tracks above); this comment is the contract, csrc/heatmap_px.hpp is its only
 * implementation and tests/heatmap_util.py restates it in NumPy.  One clip per call, track-major layouts, the inputs of spa3d_render.
 *
 * Position of point i in frame t: that of the track overlays -- coords == 3: the projection above; coords == 2: truncation, no position beyond
 *   2^30 or when not finite.  Point-frame (i, t) CONTRIBUTES when its position exists and is in bounds (0 <= x < W, 0 <= y < H), values[i][t]
 *   is finite and, with use_visibility != 0, visible[i][t] > 0.5.
 * Weight of a contributing point at (x, y) for pixel (X, Y): d2 = (X - x)^2 + (Y - y)^2, R2 = radius^2.  The point reaches the pixel iff
 *   d2 <= R2; then q = R2 + 1 - d2 and w = q (power == 1) or q q (power == 2): an integer, 1 <= w < 2^25 (radius <= 64).
 * Sums per pixel of frame t over the contributing points that reach it: den = sum of w, an unsigned 64-bit integer; num = sum of
 *   (double) w x (double) values[i][t] IN INCREASING i, starting from +0.0, one double addition per point (each product is exact in double).
 * map[t][Y][X] = (float) (num / (double) den) if den > 0, else NaN (0x7fc00000);  weight[t][Y][X] = (float) den.
 * Overlay (out given): a function of m = map[t][Y][X] widened to double, den and the input byte.  lo, hi: with normalize != 0 the min and max
 *   over the finite values[][] of the clip, else the caller's.  In double: s = (m - lo) / (hi - lo) if hi > lo, else m - lo;  s' = (float) s.
 *   If den == 0 or s' is not finite the pixel keeps its three bytes.  Otherwise the colour is score_to_color_bgr of s' as stated above for the
 *   track overlays, colour_bgr giving the byte order, and per channel out = (in (4096 - alpha) + col alpha + 2048) >> 12.
 * No fp32 division and no atomics anywhere; every output element is written once by the thread that owns its pixel (out == video is legal);
 * the sum has the fixed order above and the min / max is an order-independent reduction: the same inputs give the same bits on every run. */
typedef struct {
  int32_t N, T, H, W;              /* N, T >= 1; 1 <= H, W <= 16384 */
  const float* tracks;             /* device [N,T,3] camera/world points, or [N,T,2] pixel coordinates when coords == 2 */
  int32_t coords;                  /* 2 | 3 */
  const double* intrinsics;        /* device [T,3,3], coords == 3 only */
  const double* extrinsics;        /* device [T,4,4], coords == 3 only */
  int32_t resize_h, resize_w;      /* as in spa3d_render; >= 1, coords == 3 only */
  const float* values;             /* device [N,T] */
  const float* visible;            /* device [N,T] or NULL */
  int32_t use_visibility, radius, power;   /* radius 1..64, power 1 | 2 */
  float* map;                      /* device [T,H,W] or NULL */
  float* weight;                   /* device [T,H,W] or NULL */
  const uint8_t* video;            /* device [T,H,W,3]; required when out is given, not read otherwise */
  uint8_t* out;                    /* device [T,H,W,3] or NULL; may be == video (in place) */
  int32_t normalize;               /* overlay range: != 0 the clip's finite min / max of values, 0 the caller's lo, hi */
  float lo, hi;                    /* read when normalize == 0 and out is given; both finite */
  int32_t alpha, colour_bgr;       /* alpha 0..4096 (4096: the pure colour) */
} spa3d_heatmap;
/* a sufficient workspace for any option */
int64_t spa3d_heatmap_workspace_bytes(spa3d_handle h, int32_t N, int32_t T);
/* Asynchronous, allocates nothing, reads nothing back to the host.  SPA3D_ERR_ARG with a message, before the first launch: a missing pointer
 * (tracks, values; video when out is given; map, weight and out all NULL; visible with use_visibility), coords outside {2, 3}, camera matrices
 * or resize missing with coords == 3, N, T, H, W, radius, power or alpha out of range, lo or hi not finite when they are read, a workspace
 * that is too small (the message names the bytes needed), more than 2^31 point-frames, or 2^24 or more (frame, 64 x 16 tile) pairs: what one
 * launch holds. */
int spa3d_render_heatmap(spa3d_handle h, const spa3d_heatmap* m, void* ws, int64_t ws_bytes, void* stream);

/* Clips to model batches in one call: the support / query split, the 2-D -> 3-D lift, the DINO and depth-feature sampling and the padded,
 * ragged batch layout that spa3d_forward, spa3d_score, spa3d_loss_and_grads and spa3d_tapvid3d_from_preds read -- what inference.py:541-590 and
 * data_loader.py:56-110 do on the host, clip by clip, for every track of a clip.  Only the picked rows are computed, and they are written
 * straight into the batch, the feature planes in the handle's precision.
 *
 * A clip is a pool of n_tracks tracks over its own T frames (T <= the batch's T) and two index lists: batch slot i of the clip's sample reads
 * pool track support_index[i] (i < n_support) resp. query_index[i] (i < n_query); query_frame[i] is the frame of query i's query point.
 * Padding -- a slot at or beyond the clip's count, a frame at or beyond the clip's T, an index outside [0, n_tracks) -- is written as zeros,
 * so every byte of every output is defined.  The indices are not checked on the host (they are device arrays): validate them before the call.
 * Per live (slot, frame), with n the pool track and t the frame:
 *   position (support_tracks / query_tracks)   tracks_3d[n][t] if the clip has tracks_3d, else what spa3d_op_lift_2d_to_3d gives for
 *                                              tracks_2d[n][t] on depth_map with the clip's intrinsics
 *   visibility (..._visible)                   visible[n][t]
 *   dino_features (support slots)              the row dino_pool[n][t] copied, else what spa3d_op_sample_dino gives for the point on
 *                                              dino_map (Hp x Wp texels over the H x W video), rounded ONCE to the feature type
 *   depth_features (support slots)             the row depth_pool[n][t] copied, else the first depth_feature_dim channels of what
 *                                              spa3d_op_sample_depth_features gives (d, d / 10, d - d_prev for t > 0, zeros), rounded once
 *   query_points[q]                            (query_frame[q], x, y, z) of the query's position at that frame; zeros when query_frame[q] is
 *                                              outside the clip's [0, T)
 *   boundary_frame[b]                          the clip's T
 * The values are bit for bit those of the three spa3d_op_ samplers (float32, the reference's operation order; csrc/build_row.hpp is the only
 * implementation of the arithmetic and of the rounding: round to nearest even to bfloat16 or IEEE half).  One wave per (clip, frame, slot),
 * walked frame-major; no atomics: two calls give the same bytes.
 *
 * out: B, N, Q, T and the device buffers to fill (the const of spa3d_batch's pointers is cast away): support_tracks, support_tracks_visible,
 * boundary_frame always; query_points, query_tracks, query_tracks_visible when Q > 0.  dino_features == NULL: no clip may carry DINO (map or
 * pool); given: every clip carries one of the two.  The same holds for depth_features, where depth_map alone counts as the source (it also
 * serves the lift).  D = dino_feature_dim and the depth width = depth_feature_dim of the handle's config; noise and discretize are not touched.
 * Asynchronous on `stream`, allocates nothing, takes no workspace, reads nothing back; clips[0 .. B) (host) and each clip's intrinsics are
 * consumed before the call returns.  Up to 16 clips travel by value in one launch; a larger B takes several launches.
 * SPA3D_ERR_ARG with a message, before the first launch: a missing pointer; n_support outside [1, N] or n_query outside [0, Q]; a clip T
 * outside [1, out->T]; a map and a pool both given for one feature (for depth: depth_pool together with a depth_map that no lift needs); a
 * feature the handle or the batch does not have; neither tracks_3d nor a depth_map to lift with; a map without tracks_2d or sizes; a
 * model_kind 1 handle. */
typedef struct {            /* one clip; device pointers except intrinsics */
  int32_t n_tracks, T, H, W;               /* pool size, the clip's own frame count (<= batch T), video size */
  const float* tracks_2d;                  /* [n_tracks,T,2] pixels; needed to lift or to sample */
  const float* tracks_3d;                  /* [n_tracks,T,3] or NULL = lift from depth_map */
  const float* visible;                    /* [n_tracks,T] */
  const float* depth_map;                  /* [T,H,W] f32 or NULL */
  const float* dino_map; int32_t Hp, Wp;   /* [T,Hp,Wp,D] f32 or NULL */
  const void*  dino_pool;                  /* [n_tracks,T,D] in the output type, or NULL (prepare_3d_batch's layout) */
  const void*  depth_pool;                 /* [n_tracks,T,depth_feature_dim] in the output type, or NULL */
  const double* intrinsics;                /* host double[4] or NULL = lift_2d_to_3d's default */
  int32_t n_support, n_query;
  const int32_t *support_index, *query_index, *query_frame;   /* device */
} spa3d_clip;
int spa3d_build_batch(spa3d_handle h, const spa3d_clip* clips /* host [B] */, spa3d_batch* out, void* stream);

/* One LONG clip to W window samples in one call: the model is tied to num_output_frames frames (the head's width, the time embedding), so a clip
 * of clip->T = TL frames, which may exceed out->T = Tw, is scored window by window.  Sample w of the batch (out->B == W) is frames
 * [t0[w], min(t0[w] + Tw, TL)) of the clip; boundary_frame[w] is that length and the frames beyond it are zeros.  The support and query index
 * lists are shared by all windows; clip->query_frame, when n_query > 0, is [W, n_query] and window-relative.
 * Every output byte equals what spa3d_build_batch writes for W clips whose arrays are those frame slices of the long clip -- including channel
 * 2 of the sampled depth feature (d - d_prev), which is 0 at a window's first frame: a window is a clip that starts there.  The long clip is
 * addressed in place, no sliced copy of a pool or a map is made: pool rows are read at n * TL + t0 + t, maps at frame t0 + t.  The same kernel,
 * one wave per (window, frame, slot), frame-major; window descriptors travel by value, 16 per launch; no atomics.
 * SPA3D_ERR_ARG with a message, before the first launch: W < 1 or out->B != W; a t0[w] outside [0, TL); t0 not strictly increasing; and
 * everything spa3d_build_batch refuses, except a clip T above out->T. */
int spa3d_build_windows(spa3d_handle h, const spa3d_clip* clip, int32_t W, const int32_t* t0 /* HOST [W] */, spa3d_batch* out, void* stream);

/* The per-window results of a long clip merged back onto the clip's own time axis.  Window w covers frames [t0[w], t0[w] + len[w]); window row
 * r is row row_track[r] of every result (a permutation of [0, N); an entry outside that range writes nothing; not checked on the host: it is a
 * device array).  Per output element, in fp32, over the windows that cover its frame, in increasing w, with the integer weight of the
 * window-relative frame j of a window of L = len[w] frames -- SPA3D_BLEND_MEAN: 1, SPA3D_BLEND_HAT: min(j + 1, L - j):
 *   num = sum float(wgt) * v, den = sum float(wgt), each added left to right; the result is num / den, one division.
 *   A frame under exactly one window takes that window's value unchanged.  SPA3D_BLEND_FIRST: the lowest-numbered window that covers the
 *   frame supplies the value unchanged (targets carried onto the long axis exactly).
 *   out_spread[n][t] = sqrtf(max over the contributing windows of sum_c (p_w - p_blend)^2), 0 under one window, NaN if any distance is: the
 *   windows' disagreement about one track point.
 * csrc/window_row.hpp is the only implementation of the plan checks, the weights and the blend.  One wave per row, lanes along t; every output
 * is written once by its owner, no atomics: two runs give the same bytes.  Asynchronous, allocates nothing, takes no workspace, reads nothing
 * back; t0 and len are consumed before the call returns.
 * SPA3D_ERR_ARG with a message, before the first launch: no output wanted; a wanted output whose input is missing (out_spread needs tracks); W
 * outside [1, 256], N or TL outside [1, 2^24], Tw outside [1, 2^20], NC outside {2, 3}; blend outside the three values; a t0[w] outside [0, TL)
 * or t0 not strictly increasing; len[w] outside [1, Tw] or running past TL; a frame of [0, TL) that no window covers. */
#define SPA3D_BLEND_MEAN 0
#define SPA3D_BLEND_HAT 1
#define SPA3D_BLEND_FIRST 2
typedef struct {
  int32_t W, N, Tw, TL, NC, blend;           /* W <= 256: starts and lengths travel by value */
  const int32_t* t0;  const int32_t* len;     /* HOST [W]; len NULL = min(Tw, TL - t0[w]) */
  const int32_t* row_track;                   /* device [N] or NULL: window row r is row row_track[r] of the result (a permutation) */
  const float *tracks, *visible_logits, *frame_err;                        /* device [W,N,Tw,NC] / [W,N,Tw] / [W,N,Tw]; each may be NULL */
  float *out_tracks, *out_visible_logits, *out_frame_err, *out_spread;     /* device [N,TL,NC] / [N,TL] x 3; NULL = not wanted */
} spa3d_stitch;
int spa3d_stitch_windows(spa3d_handle h, const spa3d_stitch* s, void* stream);

/* ---- Latent-set metrics.  These are this library's own definitions: the reference stops at the predictions and has no counterpart. ----
 * The decoder sees a latent only through its quantiser, so the metrics are stated on what the quantiser keeps: the integer CODE
 *   c = (int16) rintf(clip(x, -1, 1) * 128.f)   in [-128, 128]
 * (the integer the latent quantiser rounds to before it adds the dither; ties to even, +-inf clips to +-128, -0.0 gives 0).  Sums of codes and of
 * code products are integers: exact, the same however the clips are batched, chunked or spread over ranks, and merged by integer addition.
 * csrc/motion_code.hpp is the only implementation of the rounding, the state layout, the range checks and the chunk constant.
 * In all three calls `h` serves the error message only; asynchronous on `stream`, no workspace, nothing read back.
 *
 * spa3d_motion_codes: codes[i] of latents[i], i < n (n == 0 only zeroes *bad).  A NaN has no code: it gives 0 and is counted in *bad, one
 *   device word the call itself zeroes first.  SPA3D_ERR_ARG with a message, before any launch: a NULL pointer, n < 0.
 *
 * spa3d_motion_moments_add: codes is [M][L][D].  state is a device array int64 [1 + D + D * D] = n, s[D], S[D][D] (both triangles), and the
 *   call ADDS the samples' count, sum and sum of outer products into it (zero it before the first call).  SPA3D_POOL_TOKEN: the samples are the
 *   M * L token rows c[m][l][:]; SPA3D_POOL_CLIP: the M per-clip token sums t[m][:] = sum_l c[m][l][:].  Exact 64-bit integer arithmetic, finished
 *   by 64-bit integer atomic adds (which commute): no float is added anywhere, the resulting bits do not depend on the order, on how clips were
 *   grouped into calls, or on which rank saw them.  The caller keeps n * 2^14 (token pool) or n * (128 L)^2 (clip pool) below 2^62.
 *   SPA3D_ERR_ARG with a message, before any launch: a NULL pointer, M < 1 (or above 2^40), L outside [1, 4096], D outside [1, 256], an unknown pool.
 *   In latent units a sample is x = c / 128 (token pool) or t / (128 L) (clip pool): mean mu = s / (n q), covariance Sigma = S / (n q^2) - mu mu^T
 *   (biased), q the divisor.  The Frechet distance of two such statistics, as the Python layer evaluates it in float64, is
 *     |mu_a - mu_b|^2 + tr Sigma_a + tr Sigma_b - 2 sum_i sqrt(max(lambda_i, 0)),
 *   lambda the eigenvalues of R Sigma_b R, R the symmetric square root of Sigma_a taken from its eigendecomposition with negative eigenvalues
 *   clipped to 0.  With fewer samples than dimensions the covariances are rank-deficient and the distance says little.
 *
 * spa3d_motion_pdist: a is [Ma][E], b is [Mb][E] (the same pointer is allowed), out is [Ma][Mb] int32.  SPA3D_PDIST_DOT: sum_e a_e b_e;
 *   SPA3D_PDIST_SQDIST: sum_e (a_e - b_e)^2, computed as |a|^2 + |b|^2 - 2 a.b in int32 (E <= 32767 keeps E * 256^2 below 2^31).  Every result
 *   is the exact integer: a tiled NT GEMM on the bf16 MFMA (codes are exact in bf16) whose fp32 accumulators are moved into int32 accumulators
 *   after every MOTION_KCHUNK = 1024 elements of E -- 1024 * 128 * 128 = 2^24, so no partial sum ever leaves the integers fp32 holds exactly.
 *   Every element of a and b must be a code, i.e. lie in [-128, 128]; this is the caller's contract (device data, not checked on the host), and
 *   other values give unspecified integers, never a store outside `out`.
 *   SPA3D_ERR_ARG with a message, before any launch: a NULL pointer, Ma or Mb outside [1, 2^22], E outside [1, 32767], an unknown kind.
 *
 * Streaming k-NN and ball hits.  spa3d_motion_knn and spa3d_motion_ball_hits run the tile and the K loop of spa3d_motion_pdist (SQDIST; the same
 *   contract on a, b, Ma, Mb and E, the same exact integers d(i, j) = sum_e (a_ie - b_je)^2) and reduce each tile where it was computed: no
 *   [Ma][Mb] matrix is written.  No float is compared or added.  Both take self_offset: >= 0 leaves column j == i + self_offset out of row i (0: a
 *   is b; s: a is the slice of b that starts at row s, so a large set is searched against itself in pieces); -1 leaves nothing out.  The columns
 *   left for a row are its ADMISSIBLE columns.
 *
 * spa3d_motion_knn: dist[i][0 .. k) and idx[i][0 .. k) (int32 [Ma][k] each) are the k nearest admissible rows of b for row i of a, ascending in
 *   the TOTAL order of the 64-bit key (uint64) d(i, j) << 32 | j: by distance, equal distances by the lower column index.  The order is part of
 *   the definition, so the result does not depend on how the work was split.  1 <= k <= 64, and k may not exceed the admissible columns of any
 *   row: Mb - 1 when self_offset lies in [0, Mb) (row 0's own column is then inside b), Mb otherwise.
 *   splits: the columns are searched in `splits` ranges of whole 128-column tiles by separate workgroups.  0 takes the library's plan
 *   (mc_knn_splits of csrc/motion_code.hpp), n >= 1 forces n ranges (at most 4096; ranges past the tiles are empty); only time depends on it.  One
 *   range writes dist / idx directly and needs no workspace (NULL, 0).  More write their k best keys per row to the workspace, uint64
 *   [splits][Ma][k] with all ones where a range had fewer than k admissible columns, and a merge kernel, one wave per row, writes the result.
 *   spa3d_motion_knn_workspace_bytes gives the bytes for the same Ma, Mb, k and splits (0 for one range, -1 for sizes the call refuses).
 *   SPA3D_ERR_ARG with a message, before any launch or store: a NULL a, b, dist or idx, Ma or Mb outside [1, 2^22], E outside [1, 32767],
 *   self_offset < -1, k out of range, splits outside [0, 4096], a workspace that is NULL, not 8-byte aligned or too small when one is needed.
 *
 * spa3d_motion_ball_hits: hit(i, j) = d(i, j) <= radius[i] (int32 [Ma]; <=, a negative radius hits nothing) over the admissible columns;
 *   row_hits[i] = sum_j hit(i, j) (int32 [Ma]), col_hits[j] = sum_i hit(i, j) (int32 [Mb]); either may be NULL, not both.  The call zeroes the
 *   outputs on the stream, then adds tile sums with 32-bit integer atomics, which commute: two runs give equal bits.
 *   SPA3D_ERR_ARG with a message, before any launch or store: a NULL a, b or radius, both outputs NULL, the size refusals above, self_offset < -1.
 *
 * The manifold estimates the Python layer builds from the two (spa3d.manifold_metrics; real set r [R], generated set g [G], k >= 1):
 *   radius of a sample = its k-th smallest distance to the OTHER samples of its own set (spa3d_motion_knn, self_offset 0, column k - 1);
 *   hits_r = ball_hits(a = r with the real radii, b = g), hits_g = ball_hits(a = g with the generated radii, b = r), nothing left out;
 *   precision = #{j : hits_r.col_hits[j] > 0} / G     recall   = #{i : hits_g.col_hits[i] > 0} / R     (as spa3d.precision_recall)
 *   density   = sum_j hits_r.col_hits[j] / (k G)       coverage = #{i : hits_r.row_hits[i] > 0} / R     (Naeem et al. 2020, with <=)
 *   each an integer count followed by one division.
 *
 * Kernel sums and the kernel distance.  The kernel is KID's (Binkowski et al. 2018: the unbiased MMD^2 with the cubic polynomial kernel); the
 *   features are the motion codes, not Inception's, so values are NOT comparable with published KID numbers.  On codes a[i][e], b[j][e] in
 *   [-128, 128] of flat width E, with C(E) = 16384 E and p(i, j) = sum_e a[i][e] b[j][e] + C -- an integer, 0 <= p <= 2 C < 2^30 -- the kernel is
 *     k_deg(i, j) = p(i, j)^deg / C^deg = (x.y / E + 1)^deg   for x = a / 128,   deg in {1, 2, 3} (3: KID's)
 *   so every sum of kernel values is an integer sum over C^deg: exact, and the same bits however the pairs were split over calls.
 *
 * spa3d_motion_kernel_sums: row_sums[i] = sum_j p(i, j)^degree over the admissible columns j of row i (self_offset as above: >= 0 leaves
 *   j == i + self_offset out, -1 nothing), col_sums[j] = sum_i p(i, j)^degree over the same admitted pairs.  Each sum is an unsigned 128-bit
 *   integer stored as uint64 [M][2] = {lo, hi}; the largest possible one is 2^22 (2^30)^3 = 2^112.  Either output may be NULL, not both.  The
 *   tile and K loop of spa3d_motion_pdist (DOT; the same contract on a, b, Ma, Mb and E); no [Ma][Mb] matrix is written.  The call zeroes the
 *   outputs on the stream, then adds tile sums as 128 bits by two 64-bit integer atomics, the carry taken by the one adder whose addend wrapped
 *   the low limb: the result is the exact sum whatever the order, two runs give equal bits, and the sums of disjoint column (row) ranges taken
 *   in separate calls add up to the one call's.  The limbs are complete when the call's work on the stream is.
 *   SPA3D_ERR_ARG with a message, before any launch or store: a NULL a or b, both outputs NULL, Ma or Mb outside [1, 2^22], E outside
 *   [1, 32767], degree outside [1, 3], self_offset < -1, an output that is not 8-byte aligned.
 *
 * The kernel distance the Python layer builds from three such calls (spa3d.kernel_distance; real set r [R], generated set g [G], R, G >= 2):
 *   A = sum_{i != i'} p(r_i, r_i')^deg  (r against r, self_offset 0),   B = sum_{j != j'} p(g_j, g_j')^deg,   X = sum_{i, j} p(g_j, r_i)^deg
 *   mmd2 = A / (R (R - 1) C^deg) + B / (G (G - 1) C^deg) - 2 X / (R G C^deg)
 *   formed as ONE exact rational and rounded to float64 once.  It is an unbiased estimate: small negative values are expected for equal sets.
 *   The witness, per sample, each element the float64 of its exact rational (rowsum_xy: row sums of x against y; colsum_gr: column sums of g
 *   against r):
 *     witness_gen[j]  = rowsum_gr[j] / (R C^deg) - rowsum_gg[j] / ((G - 1) C^deg)      mean kernel to the real set minus to its own set
 *     witness_real[i] = rowsum_rr[i] / ((R - 1) C^deg) - colsum_gr[i] / (G C^deg)      mean kernel to its own set minus to the generated set
 *   Sign convention: a large POSITIVE witness_gen[j] means generated clip j looks like the real set more than like its own; a large positive
 *   witness_real[i] means real clip i is far better covered by the real set than by the generated one.  mean_i witness_real[i] -
 *   mean_j witness_gen[j] = mmd2.
 *   subset_size = s: the estimate on the contiguous subsets real[t s : (t + 1) s] against gen[t s : (t + 1) s], t < min(R, G) / s (integer
 *   division), with the mean and the POPULATION standard deviation of the per-subset mmd2; shuffle first and the subsets are random ones. */
#define SPA3D_POOL_TOKEN 0
#define SPA3D_POOL_CLIP 1
#define SPA3D_PDIST_DOT 0
#define SPA3D_PDIST_SQDIST 1
int spa3d_motion_codes(spa3d_handle h, const float* latents, int64_t n, int16_t* codes, int32_t* bad, void* stream);
int spa3d_motion_moments_add(spa3d_handle h, const int16_t* codes, int64_t M, int32_t L, int32_t D, int32_t pool, int64_t* state, void* stream);
int spa3d_motion_pdist(spa3d_handle h, const int16_t* a, int64_t Ma, const int16_t* b, int64_t Mb, int32_t E, int32_t kind, int32_t* out, void* stream);
int64_t spa3d_motion_knn_workspace_bytes(int64_t Ma, int64_t Mb, int32_t k, int32_t splits);
int spa3d_motion_knn(spa3d_handle h, const int16_t* a, int64_t Ma, const int16_t* b, int64_t Mb, int32_t E, int32_t k, int64_t self_offset, int32_t splits, int32_t* dist,
                     int32_t* idx, void* workspace, int64_t workspace_bytes, void* stream);
int spa3d_motion_ball_hits(spa3d_handle h, const int16_t* a, int64_t Ma, const int16_t* b, int64_t Mb, int32_t E, const int32_t* radius, int64_t self_offset, int32_t* row_hits,
                           int32_t* col_hits, void* stream);
int spa3d_motion_kernel_sums(spa3d_handle h, const int16_t* a, int64_t Ma, const int16_t* b, int64_t Mb, int32_t E, int32_t degree, int64_t self_offset, uint64_t* row_sums,
                             uint64_t* col_sums, void* stream);

/* forward + loss + backward.  grads (flat f32, same layout as params) is OVERWRITTEN unless
 * accumulate!=0.  denom: global sum(query_tracks_visible) for data-parallel runs (the loss
 * normalisers are batch-global, train.py:111-113,119-121); <=0 = this batch's own.
 * loss3 (device): {total, position, visible} with that denominator.  out may be NULL.
 * The objective is the handle's (spa3d_set_loss, spa3d_set_point_weights below; the reference's by default). */
int spa3d_loss_and_grads(spa3d_handle h, const float* params, const spa3d_batch* b, float denom,
                         float* grads, int32_t accumulate, float* loss3, spa3d_outputs* out,
                         void* ws, int64_t ws_bytes, void* stream);

/* The training objective.  The reference trains one objective, L1 positions and BCE visibility with the weights 5000 and 1e-8 (train.py:96);
 * that is the default here, and a handle may be given another member of a small family.  Per live point (q, t) of a live query row, in fp32:
 *   p_c, g_c prediction and target, d_c = p_c - g_c, c < NC (3; 2 on the 2-D twin); l the visibility logit, y the target visibility;
 *   w the point weight (1 when no plane is attached); a_c = axis_weight[c]; beta = bce_pos_weight (the semantics of torch's pos_weight).
 *   position term   e = sum_c a_c rho(d_c)
 *     SPA3D_POS_L1     rho(d) = |d|,  rho' = sign(d) with sign(0) = 0
 *     SPA3D_POS_HUBER  rho(d) = d d / (2 delta) for |d| <= delta, else |d| - delta / 2;  rho' = d / delta, respectively sign(d)
 *                      (L1's slope in the tails, so l1_weight keeps its meaning)
 *   visibility term v = -beta y logsig(l) - (1 - y) logsig(-l)
 *   numerators      P = sum w y e,  V = sum w v  over the live points
 *   denominator     D = denom when denom > 0, else max(sum of y over the live rows, 1).  It is NOT weighted: a caller who wants a weighted
 *                   denominator passes it.
 *   loss3           {l1_weight P / D + bce_weight V / D,  P / D,  V / D}
 *   head cotangent  d/dp_c = l1_weight w y a_c rho'(d_c) / D
 *                   d/dl   = bce_weight w (beta y (sigmoid(l) - 1) + (1 - y) sigmoid(l)) / D;  with beta == 1 this is evaluated as
 *                            bce_weight w (sigmoid(l) - y) / D
 * With the default configuration and no weight plane every result is what the fixed objective gave, bit for bit, in all three precisions (the
 * extra multiplications are by exactly 1, in an order that leaves the old operations as they were).
 *   The configuration is per handle, like the options: spa3d_loss_and_grads and spa3d_loss read it; spa3d_score and the metrics do not.
 * spa3d_set_loss(h, NULL) restores the defaults.  It returns SPA3D_ERR_ARG with a message in spa3d_last_error, and leaves the stored
 * configuration untouched, for: a field that is not finite; a negative weight; position_kind outside {0, 1}; huber_delta <= 0 with HUBER;
 * l1_weight > 0 with no positive axis weight among the model's NC; g_max outside (0, 2^30], where
 *   g_max = max(l1_weight max_c a_c, bce_weight max(1, beta))
 * bounds the head gradient per unit point weight (and excludes the all-zero objective).  The fp16 automatic loss scale keeps g_max / D at or
 * below its target, and the det_grads unit follows g_max (see "det_grads" below); the defaults give g_max = 5000.
 *   Point weights: a caller-owned DEVICE plane [B,Q,T_out] of floats, one per point, addressed like query_tracks_visible; the handle keeps
 * the pointer (not a copy) until it is detached with w = NULL, and spa3d_loss_and_grads and spa3d_loss read it.  As with spa3d_set_counts a
 * later call whose batch has another B or Q is refused (SPA3D_ERR_ARG) before its first launch.  Rows at or beyond a sample's query_count are
 * never read (they may hold NaN).  Weights are expected in [0, 1]: the fp16 automatic loss scale and the det_grads unit are sized for that;
 * larger weights want a fixed "loss_scale". */
#define SPA3D_POS_L1 0
#define SPA3D_POS_HUBER 1
typedef struct {
  float l1_weight, bce_weight;   /* 5000, 1e-8 */
  int32_t position_kind;         /* SPA3D_POS_L1 */
  float huber_delta;             /* read with HUBER only; > 0 (default 1) */
  float axis_weight[3];          /* 1, 1, 1; the 2-D twin reads two */
  float bce_pos_weight;          /* 1 */
} spa3d_loss_config;
int spa3d_set_loss(spa3d_handle h, const spa3d_loss_config* cfg /* NULL = defaults */);
int spa3d_get_loss(spa3d_handle h, spa3d_loss_config* out);
int spa3d_set_point_weights(spa3d_handle h, int32_t B, int32_t Q, const float* w /* device [B,Q,T_out] or NULL = detach */);

/* clip_by_global_norm(clip) -> adamw(b1,b2,eps,wd) -> apply_updates on flat buffers, in place.
 * step = number of spa3d_adamw_step calls BEFORE this one; the bias correction uses step + 1 - scratch[3] (updates actually applied:
 * a skipped step leaves m and v untouched, so it does not count).
 * The global norm is a fixed-order two-stage reduction (no float atomics): bit-identical gradients give bit-identical updates on every replica.
 * scratch: >= 4 KiB device, zero-initialised once by the caller and then left alone between steps (floats [256, 768) are per-call partial sums;
 * a multiplier in [4] that is not a power of two in [2^-24, 1] reads as 1): scratch[0] returns the global grad norm,
 * [1] is internal, [2] = 1 when THIS step was skipped because the norm was inf/NaN (an fp16 overflow; params, m, v unchanged) else 0,
 * [3] counts skipped steps, [4] / [5] hold the dynamic loss-scale multiplier and its good-step counter (spa3d_set_loss_scale_state). */
int spa3d_adamw_step(float* params, const float* grads, float* m, float* v, int64_t n, float lr,
                     int64_t step, float clip, float b1, float b2, float eps, float wd,
                     float* scratch, void* stream);

/* spa3d_adamw_step with parameter groups and a weight EMA, in the same streaming pass: ranges of the buffers that scale the learning rate and
 * the weight decay or are frozen, and an exponential moving average of the new parameters for evaluation.  spa3d_adamw_step is unchanged.
 *
 * Table.  `groups` is a HOST array of `num_groups` ranges [begin, end) of the n elements handed to the call (NULL with 0).  It is validated, then
 *   carried to the device inside launch arguments into `ws` (>= spa3d_adamw_groups_workspace_bytes(num_groups) device bytes; may be NULL with
 *   num_groups == 0): the call allocates nothing, reads nothing back to the host, and has consumed the caller's array when it returns.
 *   0 <= num_groups <= 4096; the ranges are sorted ascending and disjoint; 0 <= begin < end <= n; lr_scale and wd_scale are finite and non-negative.
 *   An element in no range has both scales 1.  Ranges start and end at any element.
 * Frozen.  lr_scale == 0 freezes a range: its params, m, v and ema keep their bits, no weight decay reaches it, and its gradients are not read
 *   for the norm -- a NaN or an inf there neither poisons the norm nor skips the step.
 * Norm.  gn = sqrt(sum g^2) over the elements that are not frozen: the fixed-order two-stage reduction of spa3d_adamw_step, with the same
 *   thread-to-element map and the same partial layout in scratch[256, 768); a frozen element contributes +0.f.  scratch (>= 4 KiB device, same
 *   rules) means what it means there: [0] norm, [1] internal, [2] skipped-this-step, [3] skip count, [4] / [5] loss-scale multiplier and its
 *   counter.  A non-finite norm skips the whole step: nothing is written except the scratch words.
 * Update.  Per live element, in the order spa3d_adamw_step computes it: gi = g * sc (sc = 1 if gn < clip else clip / gn); m = b1 m + (1 - b1) gi;
 *   v = b2 v + (1 - b2) gi gi; mh = m / bc1, vh = v / bc2 with the bias corrections at step + 1 - scratch[3];
 *   p -= lr_g * (mh / (sqrtf(vh) + eps) + wd_g * p), where lr_g = lr * lr_scale and wd_g = wd * wd_scale are one fp32 product each.
 * EMA.  With ema != NULL (device [n]), after the update: e = d * e + (1 - d) * p_new in fp32, d = ema_decay in [0, 1), 1 - d formed once.  No
 *   bias correction: the caller initialises ema with a copy of the parameters.
 * Identity.  With num_groups == 0 and ema == NULL, params, m, v and scratch[0..5] are bit for bit those of spa3d_adamw_step on the same inputs;
 *   so they are with the single range [0, n) of scales (1, 1).  (Same expressions in the same order, and the library is built without
 *   floating-point contraction.)  The elements are moved 16 bytes at a time where the five buffers share their offset from a 16-byte boundary,
 *   one by one before and behind that and where they do not; both ways give the same bits, and two runs give the same bits (no atomics).
 * Refusals, each before the first launch with nothing written.  SPA3D_ERR_ARG: a NULL required pointer or n < 0; num_groups out of range, or
 *   groups == NULL with num_groups > 0; a range outside [0, n], empty, unsorted or overlapping; a scale that is negative or not finite;
 *   ema != NULL with ema_decay outside [0, 1) or not finite.  SPA3D_ERR_WORKSPACE: num_groups > 0 with ws NULL or ws_bytes too small.
 *   n == 0 (with a valid table, that is: none) returns SPA3D_OK and launches nothing.  The workspace query returns -1 for a count out of range. */
typedef struct {
  int64_t begin, end;  /* [begin, end) of the buffers handed to the call */
  float lr_scale;      /* multiplies lr; 0 freezes the range */
  float wd_scale;      /* multiplies wd */
} spa3d_param_group;
int64_t spa3d_adamw_groups_workspace_bytes(int32_t num_groups);
int spa3d_adamw_step_groups(float* params, const float* grads, float* m, float* v, int64_t n, float lr,
                            int64_t step, float clip, float b1, float b2, float eps, float wd,
                            const spa3d_param_group* groups /* HOST [num_groups], NULL with 0 */, int32_t num_groups,
                            float* ema /* device [n] or NULL */, float ema_decay,
                            float* scratch, void* ws, int64_t ws_bytes, void* stream);

/* Per-handle switches -- the only ones the library has (ten + one test mode); each may be preset at spa3d_create from the environment variable of the same name in
 * capitals with an SPA3D_ prefix (SPA3D_PRUNE, SPA3D_QUERY_CHUNK, SPA3D_TRACK_CHUNK, SPA3D_FREEZE ...).  Unknown names return SPA3D_ERR_ARG.
 *   "prune"      0/1  token pruning of the track encoder (16-bit modes)            } with both 0 every entry point is fully asynchronous
 *   "ro_share"   0/1  shared latent rows of the first readout block (16-bit modes) } (no plan count is read back)
 *   "loss_scale"      SPA3D_F16 handles: > 0 fixed, < 0 automatic with that head-gradient target
 *   "chunk"           samples processed at a time; 0 = as many as fit the workspace
 *   "query_chunk"  q  readout over chunks of q queries (0 = off, the default): per chunk the query embedding, readout stack, head, loss and (training)
 *                     the readout backward run and release their workspace; the latent stacks run once per sample and their gradient accumulates
 *                     over the chunks in fp32 in a fixed order.  The reference's decoder_scan_chunk_size (track_autoencoder_3d.py:312-349).  No recompute.
 *   "track_chunk"  n  track encoder over chunks of n tracks (0 = off, the default): the forward keeps only the [N, 384] encoder output, and the
 *                     backward re-runs each chunk's encoder forward with its stash before that chunk's backward -- one extra track-encoder forward
 *                     per training step, for a stash of n instead of N tracks (the reference's nn.remat, applied to the largest stash).
 *                     Either of the two > 0 processes ONE sample per sample chunk: "chunk" > 1 together with either is refused (SPA3D_ERR_ARG), and
 *                     spa3d_workspace_bytes then sizes one sample whatever its `chunk` argument.  A ragged last chunk is allowed.  Same values as
 *                     unchunked up to summation order; spa3d_plan_stats counts the forward pass only.
 *   "gemm_impl"       0 product dispatch | 1 generic strided MFMA kernel only | 2 tiled kernels | diagnostics that put small problems on the big
 *                     kernels: 3 every eligible GEMM on the 8-phase kernels, 4 the same with the non-persistent 128x384 kernel, 5 without the
 *                     single-buffer short-K kernel, 6 tiled GEMMs without the round-4 / round-5 kernels (MLP forward as two GEMMs, multi-pass input embedding, no row-stationary K = 384 kernel,
 *                     no large-register-tile kernels), 8 the product dispatch without the round-5 large-register-tile kernels (dW: csrc/gemm_tnb.hip; NT: csrc/gemm_ntb.hip), 9 = 3 with every
 *                     eligible dW / NT GEMM on those kernels whatever its row count.  (The `impl` argument of spa3d_op_linear* takes
 *                     the same values; spa3d_op_linear: | 16 = also write the pre-activation, the MLP-in form of the step.)  Decoded by
 *                     GemmPolicy::from_impl, and every kernel choice is made by the planner in csrc/gemm_plan.hpp.
 *   "attn_impl"       0 product dispatch | 1 generic composition | 2 fused kernels | 3, 4 fused with the split-pass backward on 4 / 8 waves (tests) |
 *                     6 fused kernels with the track encoder's QKV projection + attention forward as one launch (built in round 5, slower than the pair: opt-in)
 *   "det_grads"  0/1  order-independent parameter gradients: every reduction into the gradient buffer (split-M dW tiles, bias / scale column sums, broadcast
 *                     gradients) adds 64-bit fixed-point integers into a shadow of the buffer instead of float atomics, so two runs -- and two
 *                     data-parallel schedules -- give the same bits.  Unit: 2^-(32 + e) of the buffer's value with e = floor(log2(denom / (n_vis *
 *                     loss scale))) - floor(log2(g_max / 5000)), n_vis = this call's visible query points and g_max the objective's head-gradient
 *                     bound (spa3d_set_loss), clamped to [-24, 40]: a power of two chosen per call from its inputs and the handle's objective alone.
 *                     With the default objective the second term is 0, and with a real batch n_vis ~ denom, so the unit is 2^-32 as before
 *                     (2^-(32 + log2 ranks) data-parallel; fp16: follows the loss scale); it is finer when the denominator exceeds the call's own
 *                     visible count or the objective's gradients are smaller (g_max = 1, a visibility-only objective: 2^-45), and coarser by the
 *                     power of two below g_max / 5000 when they are larger -- gradients are resolved as finely, relative to their size, whatever
 *                     the objective.  Point weights are expected in [0, 1] and do not move the unit.  Range: an addend of 2^55 units or more, or a
 *                     shadow sum of 2^62 units or more, turns the whole gradient buffer of the call into NaN -- never a wrapped finite value.  The mode is
 *                     per handle and per train call: it travels with each launch of that call, so handles on other streams and the spa3d_op_*_bwd
 *                     entry points (always float atomics) never see it.
 *                     Costs 8 bytes of workspace per parameter and ~3.6 % of the step at BASELINE configs[2]
 *                     (1.82 -> 1.88 s: 64-bit atomics in the dW epilogues, the 1-channel depth gradient on the GEMM path); off by default.
 *   "freeze"     k    fine-tuning with the backward cut at a stage boundary of the flat parameter buffer (spa3d_grad_segments: {0, b1, b2, n}).  Read by
 *                     spa3d_loss_and_grads (and by spa3d_workspace_bytes(train = 1), which sizes that call); every other entry point ignores it.
 *                     0 (default) nothing is frozen: the call as it has always been, launch for launch.
 *                     1 [0, b1) is frozen -- embeddings, track encoder and the state_init leaves; the latent stacks and the readout train.
 *                     2 [0, b2) is frozen -- only track_readout_attn, query_encoder and track_predictor train.
 *                     Any other value (-1, 3, 0.5 ...) is refused with SPA3D_ERR_ARG and a message; the stored value stays.
 *                     initializer/state_init sits at offset 0, so it is frozen from 1 on although tracks_to_latents consumes it.
 *                     A call with k > 0: the forward results (outputs, loss3, latents, spa3d_plan_stats) are bit for bit those of k = 0 with the same
 *                     "chunk" -- the frozen stages run the same kernels, only without a stash; with lo = b1 or b2 (spa3d_trainable_range), [lo, n)
 *                     of `grads` receives what k = 0 gives, and [0, lo) is zero (accumulate == 0) or left untouched (accumulate != 0): no launch of the
 *                     call writes there.  Stages are skipped whole on the host: from 1 on the track-encoder backward is not run ("track_chunk": no
 *                     pass B, no recompute) and the encoder forward keeps only its [N, 384] output; with 2 the backward ends after the readout, and
 *                     the latent stacks keep no stash either.  The workspace need falls accordingly.  The two gradient events (spa3d_set_grad_events)
 *                     are still recorded once per call, in the last chunk, no later than where the shortened backward ends (2: the latents event
 *                     right behind the readout event).  Works with every precision, both model kinds, "chunk", "query_chunk", "track_chunk", "prune",
 *                     "ro_share", "det_grads", "poison", spa3d_set_counts, spa3d_set_point_weights and spa3d_set_loss.
 * and one test mode: "poison" 0/1 -- the workspace is filled with 16-bit NaN patterns before every sample chunk (and every track / query chunk), so a read of a row that this
 * call has not written (the rounded-up tails of pruned GEMMs, chunk-to-chunk reuse of the bump allocator) shows up as NaN instead of as a
 * plausible stale value (tests/test_gpu_poison.py). */
int spa3d_set_option(spa3d_handle h, const char* name, double value);

/* Dynamic loss scaling of the SPA3D_F16 backward.  `state` (device, caller-owned, may be NULL to detach) is one float: a power-of-two
 * multiplier in (0,1] applied on top of the per-call scale (0 reads as 1).  Point it at scratch + 4 of spa3d_adamw_step: that call skips the
 * update when the gradient norm is not finite (parameters and moments untouched), halves the multiplier, and doubles it back (up to 1)
 * after 200 finite steps. */
int spa3d_set_loss_scale_state(spa3d_handle h, const float* state);

/* Ragged batches: per-sample counts of live support tracks and live queries.  The tensors keep their padded layouts ([B,N,T,..], [B,Q,..]);
 * rows at or beyond a sample's count are padding: never read (they may hold NaN) and never contributing, in any entry point.
 * support_count / query_count: HOST arrays of B entries (they size launches: no device read-back, no extra synchronisation), copied into the
 * handle by this call (the caller may free them at once) and read by every later call on the handle; NULL = all N / all Q; both NULL detaches
 * (B is then ignored).  A call whose batch has another B than the stored one, 1 <= support_count[b] <= N or 0 <= query_count[b] <= Q violated,
 * counts together with "track_chunk" / "query_chunk", or counts on a model_kind 1 handle: SPA3D_ERR_ARG before the first launch, with a
 * message in spa3d_last_error.  spa3d_decode reads the query counts only, spa3d_encode the support counts only, spa3d_loss the query counts.
 *   Results: the live rows of every output and the latents are what the same handle gives for the sample alone, cropped to its counts (same
 * noise[b], boundary_frame[b]; bit for bit when the sample is alone in its chunk, up to the order of summation in a packed chunk, see below); output rows of padded queries are written as 0; loss and gradients are those of the live rows
 * (denom <= 0: max(sum of query_tracks_visible over the live queries, 1)) -- the sum over the samples of single-sample
 * spa3d_loss_and_grads(denom = D, accumulate = 1) calls.  A sample with query_count 0 is encoded and adds no loss and no gradient.
 *   Work follows the live counts, not B x N.  The samples of a sample chunk are PACKED: the track encoder runs once over the chunk's
 * sum n_b live tracks, the K/V projection of tracks_to_latents over those sum n_b rows and its cross attention over each sample's own n_b keys
 * (one launch of the chunked-key kernels with per-sample key offsets; the fp32 parity mode and attn_impl 1 run that attention sample by
 * sample), the latent stacks over the chunk's samples, the readout over the sum q_b live queries; only cheap per-row kernels (key mask,
 * sequence assembly, head / loss) are issued per sample.  The live rows of a chunk of several samples are copied once into packed buffers
 * in the workspace (tracks, visibility, DINO / depth planes, query points); a chunk of ONE sample addresses its rows in place.
 * spa3d_plan_stats reports the sums: out4[1] = sum n_b x (T + 1), out4[3] = sum q_b.  "chunk", "prune", "det_grads", "poison" and the fp16
 * loss scale work as in a uniform call (the chunk size that fits is found with the live counts); "ro_share" applies to chunks of one sample
 * only -- a packed chunk runs the first readout block densely (its slot plan is per (sample, frame) and is not carried over to packed
 * queries yet).  Counts that all equal (N, Q) are the uniform call, bit for bit.  Results of a packed chunk equal the single-sample ones up to
 * the order of summation (GEMM kernels are picked by row count).
 * spa3d_workspace_bytes of the padded shape (any chunk >= 1) stays a sufficient bound: the sizing pass of a ragged call walks the live
 * counts and takes the largest chunk that fits; a single sample needs no packed copy. */
int spa3d_set_counts(spa3d_handle h, int32_t B, const int32_t* support_count, const int32_t* query_count);

/* Overlapping the data-parallel gradient all-reduce with the backward (no reference counterpart: the reference is single-device, SURVEY 2;
 * the split is SURVEY 8(e)'s).  Parameter gradients accumulate over the call's sample chunks, so a leaf is final only in the LAST chunk's
 * backward, in reverse graph order.  spa3d_grad_segments: bounds4 = {0, b1, b2, n} (floats) cut the flat gradient buffer into
 *   [b2, n)  track_readout_attn, query_encoder, track_predictor            -- final first  (event ev_readout)
 *   [b1, b2) tracks_to_latents, compressor, decompressor, decompress_attn  -- final second (event ev_latents)
 *   [0, b1)  state_init leaves, token / dino / depth projections, input_track_transformer -- final when the call's work is.
 * spa3d_set_grad_events registers two hipEvent_t (or NULL to detach) that spa3d_loss_and_grads records on its stream at those two points of
 * the last chunk; a collective on a side stream that waits for an event may then run under the rest of the backward.  Nothing is recorded
 * on SPA3D_F16 handles (the loss-scaled buffer is rescaled as a whole at the end): use stream order there. */
int spa3d_grad_segments(spa3d_handle h, int64_t* bounds4);
/* The range of the flat buffer that spa3d_loss_and_grads trains under the stored "freeze" option: lo_n = {lo, n} with lo = 0, b1 or b2 of
 * spa3d_grad_segments for freeze 0, 1, 2.  [lo, n) is what the call writes gradients into; an optimiser step, a gradient norm or an all-reduce of a
 * fine-tuning run covers that range only (spa3d_adamw_step on params + lo, grads + lo, m + lo, v + lo with n - lo elements). */
int spa3d_trainable_range(spa3d_handle h, int64_t* lo_n /* [2] */);
int spa3d_set_grad_events(spa3d_handle h, void* ev_readout, void* ev_latents);
/* out4 = {records of the readout event so far, records of the latents event so far, the registered ev_readout, the registered ev_latents}
 * (host counters, bumped when a record is enqueued; the pointers as integers).  A caller about to wait on ITS events checks that they are
 * still the registered ones and that both counters advanced during its last spa3d_loss_and_grads, and otherwise falls back to stream order: waiting on an event that was NOT re-recorded (another owner re-registered or detached the events, an SPA3D_F16 handle)
 * would let the side-stream all-reduce start before the backward has produced the gradients. */
int spa3d_grad_events_recorded(spa3d_handle h, int64_t* out4);
/* Owner-aware detach: clears the registered events only if the handle still holds exactly (ev_readout, ev_latents), and the loss-scale
 * state only if it still is `loss_scale_state`; NULL arguments are skipped.  Lets a train state that is being destroyed release what IT
 * registered without tearing down what a newer state has registered on the same handle since. */
int spa3d_detach(spa3d_handle h, void* ev_readout, void* ev_latents, const float* loss_scale_state);

/* Data-dependent plan sizes of the last spa3d_loss_and_grads / forward call on this handle, summed over its sample chunks:
 * out4 = {track-encoder token rows kept, token rows before pruning, distinct (sample, query frame) slots, queries}; zeros when the
 * respective saving is off.  Host values (they are the counts the call read back to size its launches). */
int spa3d_plan_stats(spa3d_handle h, double* out4);

/* Live timing of the hot kernel classes with HIP event pairs recorded on the launch stream (bench.py's
 * "roofline" object).  cls: 0 tiled NT GEMM (incl. the fused MLP forward), 1 tiled TN GEMM (dW), 2 generic GEMM, 3 fused attention fwd,
 * 4 fused attention bwd, 5 / 6 LayerNorm fwd / bwd, 7 single-query attention, 8 the input-embedding stage as a whole (its GEMMs are also
 * counted in class 0).  out4 = {launches, total ms, algorithmic FLOPs, algorithmic bytes}. */
int spa3d_prof_enable(spa3d_handle h, int32_t on);
int spa3d_prof_read(spa3d_handle h, int32_t cls, double* out4);
/* One CSV line per profiled launch group since spa3d_prof_enable(h, 1): class, ms, algorithmic FLOPs, algorithmic bytes, M, N, K, flags
 * (tools/step_shapes.py aggregates it per GEMM shape).  Synchronises on the recorded events. */
int spa3d_prof_dump(spa3d_handle h, const char* path);

/* jax.random.uniform(PRNGKey(0),[n]) in the legacy (non-partitionable) threefry layout. */
int spa3d_uniform_noise(float* out, int64_t n, uint32_t key0, uint32_t key1, void* stream);

/* ---- single-op entry points (tests / benchmarks).  dtype: SPA3D_F32 | SPA3D_BF16 for the
 * activation tensors (void*); parameters, statistics and gradients of parameters are f32. ---- */

/* out[rows, C*2*nf] = SinusoidalEmbedding(x[rows,C]) (track_autoencoder.py:18-38) */
int spa3d_op_sin_embed(const float* x, int64_t rows, int32_t C, int32_t nf, void* out, int32_t dtype, void* stream);

/* C[M,N] = act(A[M,K] @ B[K,N] + bias) (+ residual); A,B,C,residual dense row-major `dtype`;
 * act: 0 none, 1 tanh-gelu, 2 = no activation and `residual` is not added but holds a pre-activation: C = (A @ B + bias) o gelu'(residual), the MLP backward's
 * dh = (dy . W_out^T) o gelu'(hpre).  impl: 0 auto, 1 generic kernel, 2 tiled bf16 kernel (error if unusable), ... as "gemm_impl" above; 7 = the row-stationary
 * K = 384 kernel (csrc/gemm_rs.hip: 16-bit, 128 | N <= 2304, act 0 or 2) or an error; 10 = the large-register-tile NT kernel (csrc/gemm_ntb.hip: 16-bit,
 * 384 | N or 256 | N, 32 | K >= 64, act 0, no residual) or an error -- spa3d_op_linear_bwd: its dA on that kernel. */
int spa3d_op_linear(const void* A, const void* B, const float* bias, const void* residual, void* C,
                    int64_t M, int32_t N, int32_t K, int32_t act, int32_t dtype, int32_t impl,
                    void* ws, int64_t ws_bytes, void* stream);
/* dA[M,K] = dC @ B^T ; dB[K,N] (f32, overwritten) = A^T @ dC ; dbias[N] (f32, overwritten) = colsum(dC) */
int spa3d_op_linear_bwd(const void* A, const void* B, const void* dC, void* dA, float* dB, float* dbias,
                        int64_t M, int32_t N, int32_t K, int32_t dtype, int32_t impl,
                        void* ws, int64_t ws_bytes, void* stream);

/* One GEMM as the model describes it to the planner (csrc/gemm_plan.hpp: the fields of GemmDesc, same names and meanings, without the packed-weight
 * streams):  C[b][m'][n] (op)= epi(alpha * sum_k A[b][m][k] * B[b][k'][n] + bias[n]) with element strides, a two-level batch, the row remaps
 * m' = m + (m / crow_group + 1) * crow_skip (C, aux and pre_out) and k' = k + (k / brow_group + 1) * brow_skip (B), column segments of a dW output
 * (columns [s seg_n, (s + 1) seg_n) in C_seg[s - 1] for s >= 1), the fused column sums of B and the one-pass input embedding operands (A2 .. r1_w).
 * Zero-initialise the struct, then set what the GEMM uses: alpha = 0 is a factor of zero, nb1 = nb2 = 0 is refused. */
typedef struct {
  const void* A; const void* B; void* C;
  int64_t M; int32_t N; int32_t K;
  int64_t sAm, sAk, sBk, sBn, sCm;           /* element strides; C is n-contiguous */
  int32_t nb1, nb2;                          /* two-level batch (>= 1 each) and its element strides */
  int64_t bA1, bA2, bB1, bB2, bC1, bC2;
  float alpha;
  const float* bias;                         /* f32[N] or NULL */
  int32_t epi;                               /* SPA3D_EPI_* */
  const void* aux; int32_t aux_is_residual;  /* C layout, `dtype`: residual, or the pre-activation of SPA3D_EPI_MUL_GELU_GRAD */
  int32_t out_f32, accumulate;               /* C is f32 whatever `dtype`; C += */
  void* pre_out;                             /* C layout, `dtype`: the value before the activation, or NULL */
  int32_t crow_group, crow_skip, brow_group, brow_skip;
  int32_t seg_n; void* C_seg[2];             /* dW kernels only */
  float* colsum_out;                         /* f32[N], accumulated into: the column sums of B's rows k' (the bias gradient of a dW GEMM) */
  const void* A2; int64_t sA2m; int32_t K1;  /* one-pass input embedding: K columns [0, K1) from A, [K1, K) from A2 */
  const int32_t* arow_idx;                   /* input row of output row m (A, A2 and r1_x) */
  const int32_t* crow_idx;                   /* row of C that output row m is stored at; < 0: dropped */
  const void* r1_x; const float* r1_w;       /* C[m][n] += r1_x[input row] * r1_w[n] in f32; r1_x in `dtype` */
  const void* Bt; int64_t ldBt;              /* optional copy of B stored [N][K], K contiguous, row stride ldBt */
} spa3d_gemm_args;
enum { SPA3D_EPI_NONE = 0, SPA3D_EPI_GELU = 1, SPA3D_EPI_MUL_GELU_GRAD = 2 };
/* the kernels a GEMM can run on (GemmKernel of csrc/gemm_plan.hpp, same order) */
enum { SPA3D_GEMM_REFUSE = 0, SPA3D_GEMM_GENERIC = 1, SPA3D_GEMM_RS = 2, SPA3D_GEMM_NTB = 3, SPA3D_GEMM_MLP_FUSED = 4, SPA3D_GEMM_NT_EMBED = 5,
       SPA3D_GEMM_NT8PP256 = 6, SPA3D_GEMM_NT8PP384 = 7, SPA3D_GEMM_NT8P256 = 8, SPA3D_GEMM_NT8P384 = 9, SPA3D_GEMM_NT_OCC = 10, SPA3D_GEMM_NT = 11,
       SPA3D_GEMM_TNB = 12, SPA3D_GEMM_TN8P256 = 13, SPA3D_GEMM_TN8P128X384 = 14, SPA3D_GEMM_TN8P384X128 = 15, SPA3D_GEMM_TN = 16 };
/* Plans the descriptor with the model's planner under the kernel-choice switches of `impl` ("gemm_impl" above), writes the chosen SPA3D_GEMM_* to
 * *kernel_out (may be NULL; SPA3D_GEMM_REFUSE when the call fails before or at its plan) and launches that kernel.  fp32 always runs
 * on the generic kernel.  From the workspace: 256 zero bytes for a dW descriptor (sAm = sBn = 1, out_f32, accumulate), and the [N][K] copy of B (K N
 * elements) when Bt is NULL, B is dense [K][N] and a tiled NT kernel takes the GEMM with it.
 * colsum_out: the 8-phase and large-tile dW kernels add the sums themselves; for every other 16-bit kernel (SPA3D_GEMM_TN, SPA3D_GEMM_GENERIC with
 * sBn = 1 and no batch) the entry adds them with the column-sum kernel after the GEMM, so the result does not depend on the kernel.
 * SPA3D_ERR_ARG, before any launch: A, B or C NULL; M, N or K < 1; nb1 or nb2 < 1; a dtype other than fp32 / bf16 / fp16; epi outside 0..2, or 2 without
 * aux; a negative group, skip, seg_n or K1; seg_n > 0 with N % seg_n, more than three segments or a missing C_seg; A2 with K1 outside (0, K); r1_x
 * without r1_w; impl >= 2 when no tiled kernel takes the GEMM; and what no kernel for the type implements -- fp32 with seg_n, colsum_out or an
 * embedding operand (A2, arow_idx, crow_idx, r1_x), 16-bit with seg_n or an embedding operand when the plan is the generic kernel, colsum_out on the
 * generic kernel with sBn != 1 or a batch.  SPA3D_ERR_WORKSPACE: a workspace too small for the two items above. */
int spa3d_op_gemm(const spa3d_gemm_args* g, int32_t dtype, int32_t impl, int32_t* kernel_out, void* ws, int64_t ws_bytes, void* stream);

/* The MLP of ImprovedTransformerBlock (attention.py:103-108) as ONE sequence-resident kernel, 16-bit dtypes, d = 384 and mlp = 1536 only
 * (the track encoder's widths; anything else returns SPA3D_ERR_ARG):  hpre = na @ w_in + b_in, h = tanh-gelu(hpre), y = a + h @ w_out + b_out.
 * na, a, y [M,d]; h, hpre [M,mlp]; w_in [d,mlp], w_out [mlp,d] in `dtype`; biases f32.  ws >= 4 MiB. */
int spa3d_op_mlp_fused(const void* na, const void* a, const void* w_in, const float* b_in, const void* w_out, const float* b_out,
                       void* y, void* h, void* hpre, int64_t M, int32_t d, int32_t mlp, int32_t dtype,
                       void* ws, int64_t ws_bytes, void* stream);

/* y = LayerNorm(x)*scale (no bias, eps 1e-6, fast variance); stats[rows,2] = (mean, rstd) */
int spa3d_op_layernorm(const void* x, const float* scale, void* y, float* stats, int64_t rows, int32_t d,
                       int32_t dtype, void* stream);
int spa3d_op_layernorm_bwd(const void* x, const float* scale, const float* stats, const void* dy, void* dx,
                           float* dscale /* f32[d], accumulated into */, int64_t rows, int32_t d, int32_t dtype, void* stream);

/* QKV projection + attention core of ImprovedMHDPAttention as ONE kernel (attention.py:154-175; round 5): q | k | v = nq . (Wq | Wk | Wv) (16-bit, stored:
 * qkv [rows, 3*H*96]), per-head RMSNorm of q and k, softmax, PV -> o [rows, H*96], lse [nseq, H, S, 2] (may be NULL).  nq [rows, 384] with row stride ldn;
 * wq / wk / wv [384, H*96] in the activation type; d = 384 and Dh = 96 only, S <= 160.  seq_off (int32 [nseq + 1], device) = ragged sequences (token pruning) or
 * NULL for nseq dense sequences of S rows; keymask as spa3d_op_attention.  16-bit dtypes only; SPA3D_ERR_ARG when the shape is not covered. */
int spa3d_op_qkv_attention(const void* nq, int64_t ldn, const void* wq, const void* wk, const void* wv, const float* scale_q, const float* scale_k,
                           const float* keymask, const int32_t* seq_off, int64_t nseq, int32_t S, int32_t H, void* qkv, void* o, float* lse,
                           int32_t dtype, void* ws, int64_t ws_bytes, void* stream);

/* Multi-head attention core of ImprovedMHDPAttention (attention.py:166-175): per-head RMSNorm of
 * q and k (scales f32[Dh]), q/sqrt(Dh), key mask (f32 [nseq,Sk] or NULL, non-zero = keep),
 * softmax, PV.  q [nseq,Sq,H*Dh] with row stride ldq (elements); k,v [nseq,Sk,H*Dh] strides ldk/ldv;
 * o [nseq,Sq,H*Dh] dense.  impl: 0 auto, 1 generic (GEMM+softmax kernels), 2 fused kernel. */
int spa3d_op_attention(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv,
                       const float* scale_q, const float* scale_k, const float* keymask,
                       int64_t nseq, int32_t Sq, int32_t Sk, int32_t H, int32_t Dh, void* o,
                       float* lse /* [nseq,H,Sq,2] = (row max, log row sum); written by the fused kernel only; may be NULL */,
                       int32_t dtype, int32_t impl, void* ws, int64_t ws_bytes, void* stream);
/* The cross attention of a leave-fold-out round (spa3d_score_folds) on its own: nseq sequences of Sq queries, q [nseq,Sq,H*Dh], over ONE shared key
 * set k, v [Nk,H*Dh]; sequence i leaves out the rows [lo_i, hi_i) = holes[2i], holes[2i + 1] and attends the rows outside, in row order.  No key
 * mask.  o, lse and impl as spa3d_op_attention; the result of sequence i is bit for bit spa3d_op_attention's on a compacted copy of its keys
 * (Sq queries against n_i = Nk - (hi_i - lo_i) keys, n_i != Sq).  ws holds the device copy of the holes, the fused kernel's partials or, on the
 * generic path, the compact copy.  SPA3D_ERR_ARG: a hole outside [0, Nk], lo > hi, a sequence left without a key. */
int spa3d_op_attention_holdout(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv,
                               const float* scale_q, const float* scale_k, int64_t nseq, int32_t Sq, int32_t Nk,
                               int32_t H, int32_t Dh, const int32_t* holes /* HOST [nseq][2] = lo, hi */,
                               void* o, float* lse, int32_t dtype, int32_t impl,
                               void* ws, int64_t ws_bytes, void* stream);
/* gradients of the above: dq,dk,dv dense-strided like q,k,v (same ld*); dscale_q/k f32[Dh] accumulated into */
int spa3d_op_attention_bwd(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv,
                           const float* scale_q, const float* scale_k, const float* keymask,
                           int64_t nseq, int32_t Sq, int32_t Sk, int32_t H, int32_t Dh,
                           const void* o, const float* lse /* forward outputs: needed by the fused kernel, NULL -> generic */,
                           const void* d_o, void* dq, void* dk, void* dv, float* dscale_q, float* dscale_k,
                           int32_t dtype, int32_t impl, void* ws, int64_t ws_bytes, void* stream);

/* The two ragged forms of the fused attention on their own (tests/test_gpu_attn_ragged.py).  The offsets are HOST arrays [nseq + 1], checked and then
 * copied into ws; ws also holds what the kernels carve (the chunked-key partials, the generic composition's intermediates) and is sized by a dry walk
 * before the first launch (SPA3D_ERR_WORKSPACE).  1 <= nseq <= 2^20.  Every refusal below is SPA3D_ERR_ARG and launches nothing.
 *
 * Ragged self-attention (token pruning in the track encoder): sequence i is rows [seq_off[i], seq_off[i + 1]) of the packed q, k, v, o (row strides
 * ldq / ldk / ldv, o dense), 1 <= its length S_i <= S, where S (2..320) picks the kernel instance as the longest length does in the model.  lse of
 * (sequence i, head h, token t) sits at ((seq_off[i] * H + h * S_i) + t) * 2, H * 2 floats per packed row in all.  keymask: NULL, or f32 [seq_off[nseq]]
 * indexed by PACKED row (non-zero = keep), not [nseq, S].  16-bit dtypes and Dh = 96 only, impl 0 / 2 (3 / 4 in the backward: the split-pass structures) --
 * there is no generic route for ragged rows, so SPA3D_F32, impl 1 and any other impl are refused, as are a NULL required pointer, H < 1, a row stride
 * below H*Dh or no multiple of 8, a pointer off 16 bytes, seq_off[0] < 0 and a length outside [1, S]. */
int spa3d_op_attention_ragged(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv,
                              const float* scale_q, const float* scale_k, const float* keymask,
                              const int32_t* seq_off /* HOST [nseq + 1] */, int64_t nseq, int32_t S, int32_t H, int32_t Dh, void* o,
                              float* lse /* may be NULL */, int32_t dtype, int32_t impl, void* ws, int64_t ws_bytes, void* stream);
/* gradients of the above from the forward's o and lse (both required); dq, dk, dv strided like q, k, v; dscale_q / dscale_k f32[Dh] accumulated into */
int spa3d_op_attention_ragged_bwd(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv,
                                  const float* scale_q, const float* scale_k, const float* keymask,
                                  const int32_t* seq_off /* HOST [nseq + 1] */, int64_t nseq, int32_t S, int32_t H, int32_t Dh,
                                  const void* o, const float* lse, const void* d_o, void* dq, void* dk, void* dv,
                                  float* dscale_q, float* dscale_k, int32_t dtype, int32_t impl, void* ws, int64_t ws_bytes, void* stream);
/* Cross attention against ragged key sets (tracks_to_latents on a batch with per-sample support counts): q, o [nseq,Sq,H*Dh]; the keys of sequence i are
 * rows [koff[i], koff[i + 1]) of the packed k, v; no key mask; lse [nseq,H,Sq,2].  impl 0 / 2: one launch of the chunked-key kernels (16-bit, Dh = 96,
 * Sq <= 128); impl 1, SPA3D_F32 or another shape: the sequences one by one through spa3d_op_attention's routes.  Refused: koff[0] != 0, a sequence
 * without a key, Sq < 1, H < 1, Dh outside 1..128, impl outside 0..2, a row stride below H*Dh, and impl 2 with a shape, dtype or alignment the fused
 * kernels do not take. */
int spa3d_op_attention_varlen(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv,
                              const float* scale_q, const float* scale_k, const int32_t* koff /* HOST [nseq + 1] */,
                              int64_t nseq, int32_t Sq, int32_t H, int32_t Dh, void* o, float* lse, int32_t dtype, int32_t impl,
                              void* ws, int64_t ws_bytes, void* stream);
/* gradients of the above from the forward's o and lse: both are required for a 16-bit dtype under impl 0 / 2 (a NULL one is refused); SPA3D_F32 and impl 1 run the
 * generic composition, which reads neither, and take NULL */
int spa3d_op_attention_varlen_bwd(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv,
                                  const float* scale_q, const float* scale_k, const int32_t* koff /* HOST [nseq + 1] */,
                                  int64_t nseq, int32_t Sq, int32_t H, int32_t Dh, const void* o, const float* lse, const void* d_o,
                                  void* dq, void* dk, void* dv, float* dscale_q, float* dscale_k, int32_t dtype, int32_t impl,
                                  void* ws, int64_t ws_bytes, void* stream);

/* Single-query attention of a stack's last block (csrc/attn_q1.hip; track_autoencoder_3d.py:187-188, 286): only token 0 of each sequence
 * queries, every token is a key.  q0 [nseq,H*Dh] with row stride ldq0; k, v [rows,H*Dh] with row strides ldk / ldv; o0 [nseq,H*Dh] dense;
 * p0 [nseq*H,S] f32 = the softmax row of every (sequence, head), kept for the backward.  Scales, key mask and arithmetic as
 * spa3d_op_attention (fp32 between load and store); keymask f32 [rows] or NULL.  seq_off (int32 [nseq + 1], device) = ragged sequences:
 * sequence i is rows [seq_off[i], seq_off[i + 1]) of k, v and keymask, 1 <= its length <= S, and only that many entries of its p0 rows
 * are written; NULL = nseq dense sequences of S rows.  Dh in {8, 16, 32, 64, 96, 128}, 1 <= S <= 320; anything else, or a NULL
 * required pointer, returns SPA3D_ERR_ARG and launches nothing. */
int spa3d_op_attention_q1(const void* q0, int64_t ldq0, const void* k, const void* v, int64_t ldk, int64_t ldv,
                          const float* scale_q, const float* scale_k, const float* keymask, const int32_t* seq_off,
                          int64_t nseq, int32_t S, int32_t H, int32_t Dh, void* o0, float* p0, int32_t dtype, void* stream);
/* gradients of the above from the forward's p0: dq0 [nseq,H*Dh] dense; dk, dv strided like k, v, every row of every sequence overwritten
 * (a masked key's rows with zeros); dscale_q / dscale_k f32[Dh] accumulated into.  Float atomics (the deterministic-gradient variant
 * runs inside spa3d_loss_and_grads only). */
int spa3d_op_attention_q1_bwd(const void* q0, int64_t ldq0, const void* k, const void* v, int64_t ldk, int64_t ldv,
                              const float* scale_q, const float* scale_k, const float* keymask, const int32_t* seq_off,
                              int64_t nseq, int32_t S, int32_t H, int32_t Dh, const float* p0, const void* d_o0,
                              void* dq0, void* dk, void* dv, float* dscale_q, float* dscale_k, int32_t dtype, void* stream);

/* Dense with an input width K <= 4 as a streaming kernel (csrc/embed.hip; the depth projection, track_autoencoder_3d.py:143-147):
 * out[crow(m)][0..N) += x[m][0..K) . w[K][N] + bias, m < M, crow(m) = m + (m / rgroup + 1) * rskip (rgroup > 0) or m (rgroup == 0).
 * x [M,K], w [K,N] and out (row stride ldo) in `dtype`; bias f32[N] or NULL.  16-bit dtypes only; 1 <= K <= 4, N a multiple of 8 up to
 * 2048, ldo a multiple of 8, out 16-byte aligned, M < 2^31; anything else returns SPA3D_ERR_ARG and launches nothing. */
int spa3d_op_rank_linear(const void* x, const void* w, const float* bias, void* out, int64_t M, int32_t N, int32_t K, int64_t ldo,
                         int32_t rgroup, int32_t rskip, int32_t dtype, void* stream);
/* gradients of the above: gw f32[K,N] += x^T . dy (rows of dy mapped by crow), gb f32[N] += column sums of those rows (NULL: skipped).
 * dy with row stride ldy; the same shape rules on N, K, ldy and dy's alignment. */
int spa3d_op_rank_linear_bwd(const void* x, const void* dy, int64_t M, int32_t N, int32_t K, int64_t ldy, int32_t rgroup, int32_t rskip,
                             float* gw, float* gb, int32_t dtype, void* stream);

/* ---- The row plumbing of csrc/rows.hip on its own (tests/test_gpu_rows.py).  `dtype` in {SPA3D_F32, SPA3D_BF16, SPA3D_F16} is the storage type of
 * every `void*` tensor; sums are fp32 (float atomics where a sum is split).  "16 bytes" below is 4 fp32 or 8 16-bit elements.  An empty input
 * (0 rows, 0 samples) returns SPA3D_OK and launches nothing; a NULL required pointer, a negative count or a shape outside what is stated
 * returns SPA3D_ERR_ARG and launches nothing. ---- */

/* out[j] += sum over r < rows of x[crow(r) * ld + j], j < n; crow as spa3d_op_rank_linear.  1 <= n <= ld.  16 bytes per thread when n and ld are
 * multiples of 16 bytes and x is 16-byte aligned, else element by element. */
int spa3d_op_colsum(const void* x, int64_t rows, int32_t n, int64_t ld, int32_t rgroup, int32_t rskip, float* out /* f32[n], accumulated into */,
                    int32_t dtype, void* stream);

/* Row movers, n rows of d elements:
 *   SPA3D_ROWS_GATHER_STRIDED   dst[i] = src[i * stride_rows]          SPA3D_ROWS_ADD_STRIDED      dst[i * stride_rows] += src[i]
 *   SPA3D_ROWS_GATHER_IDX       dst[i] = src[idx[i]]                   SPA3D_ROWS_SCATTER_IDX      dst[idx[i]] = src[i]
 *   SPA3D_ROWS_SCATTER_ADD_IDX  dst[idx[i]] += src[i]  -- for UNIQUE indices only (a plain read-modify-write: two rows with one index race)
 * The strided modes take any d >= 1 and stride_rows >= 1 (idx is not read); the index modes (idx int32 [n], device; stride_rows not read) move 16 bytes
 * per thread: d a multiple of 16 bytes, src and dst 16-byte aligned.  Copies are bit-exact; an add is one fp32 addition and one rounding to `dtype`. */
enum { SPA3D_ROWS_GATHER_STRIDED = 0, SPA3D_ROWS_GATHER_IDX = 1, SPA3D_ROWS_SCATTER_IDX = 2, SPA3D_ROWS_SCATTER_ADD_IDX = 3, SPA3D_ROWS_ADD_STRIDED = 4 };
int spa3d_op_rows(int32_t mode, const void* src, const int32_t* idx, int64_t stride_rows, void* dst, int64_t n, int32_t d, int32_t dtype, void* stream);

/* Token-pruning plan of the track encoder: km f32 [nseq, S] (non-zero = keep; -0.0 is dropped, NaN kept) -> cnt [nseq] kept tokens per sequence,
 * seq_off [nseq + 1] their exclusive prefix, row_src [*kept] the dense row seq * S + t behind every kept row, in order; *kept (host) = seq_off[nseq].
 * Synchronises the stream once.  S >= 1, nseq * S < 2^31; nseq = 0: *kept = 0, nothing written. */
int spa3d_op_prune_plan(const float* km, int64_t nseq, int32_t S, int32_t* cnt, int32_t* seq_off, int32_t* row_src, int64_t* kept, void* stream);

/* Shared-latent-row plan of the readout stack's first block: qframe int32 [B, Q] -> slot [B * Q] = the slot of every query, a slot being a distinct
 * (sample, frame) pair numbered sample by sample in order of first occurrence; slot_b / slot_f / slot_q0 [*nslot] = sample, frame and first member
 * query (b * Q + q) of every slot; *nslot (host) their number.  scratch int32 [B * Q + B + 1].  Synchronises the stream once.  B > 1024 or Q > 12288
 * is outside the plan's tables: *nslot = B * Q and nothing is written (the caller keeps the dense path). */
int spa3d_op_share_plan(const int32_t* qframe, int64_t B, int32_t Q, int32_t* slot, int32_t* slot_b, int32_t* slot_f, int32_t* slot_q0, int32_t* scratch,
                        int64_t* nslot, void* stream);

/* The rows behind that plan; S = L + 1 tokens per query sequence, nseq = B * Q, U = nslot * L + nseq rows:
 *   SPA3D_SHARE_ASSEMBLE  a = qtok [nseq, d], b = lat [B, L, Cl] -> out [U, d]: row (s, n) = [lat[slot_b[s]][n] | its window at frame slot_f[s]] (as
 *                         spa3d_op_assemble_readout), then the nseq query-token rows.  Reads slot_b, slot_f.  Cl <= d, a multiple of 16 bytes.
 *   SPA3D_SHARE_EXPAND    a = srcU [U, d] -> out [nseq, S, d]: token 0 = row nslot * L + seq, token 1 + n = row slot[seq] * L + n.  With b = add
 *                         [nseq, S, d] (the backward form): out = add, plus the source row at every token 0 and at the tokens of each slot's FIRST
 *                         member slot_q0 only.  Reads slot, slot_q0; Cl is not read.
 *   SPA3D_SHARE_REDUCE    a = src [nseq, S, d] -> out [U, d], the transpose of the expansion: row (s, n) = fp32 sum over the slot's members, in
 *                         ascending query order, of their token 1 + n; row nslot * L + seq = token 0 of seq.  Reads slot, slot_b; Q <= 12288.
 * Vector kernels only: d a multiple of 16 bytes and a, b, out 16-byte aligned.  Pointers a mode does not read may be NULL. */
enum { SPA3D_SHARE_ASSEMBLE = 0, SPA3D_SHARE_EXPAND = 1, SPA3D_SHARE_REDUCE = 2 };
int spa3d_op_share_rows(int32_t which, const void* a, const void* b, const int32_t* slot, const int32_t* slot_b, const int32_t* slot_f,
                        const int32_t* slot_q0, int64_t nslot, int64_t B, int32_t Q, int32_t L, int32_t Cl, int32_t d, void* out, int32_t dtype, void* stream);

/* Readout sequence assembly (track_autoencoder_3d.py:235-246, 276-284): seq [B, Q, 1 + L, D]; token 0 = qtok [B, Q, D]; token 1 + n =
 * [lat[b][n][0..Cl) | lat[b][n][dd + 5 qframe[b][q]] for dd < D - Cl, 0 outside [0, Cl)].  1 <= Cl <= D.  16 bytes per thread when Cl and D are multiples
 * of 16 bytes and the three tensors are 16-byte aligned, else element by element; both are copies, bit for bit. */
int spa3d_op_assemble_readout(const void* qtok, const void* lat, const int32_t* qframe, int64_t B, int32_t Q, int32_t L, int32_t Cl, int32_t D, void* seq,
                              int32_t dtype, void* stream);
/* its backward: dqtok [B, Q, D] = token 0 of dseq (a copy); dlat f32 [B, L, Cl] = (accumulate ? dlat : 0) + the sum over the sample's queries of
 * both parts, in a fixed order (no atomics).  L >= 1. */
int spa3d_op_assemble_readout_bwd(const void* dseq, const int32_t* qframe, int64_t B, int32_t Q, int32_t L, int32_t Cl, int32_t D, void* dqtok, float* dlat,
                                  int32_t accumulate, int32_t dtype, void* stream);

/* dst [B, rows, d] = src f32 [rows, d] rounded once to `dtype` (ParamStateInit, track_autoencoder.py:41-53) ... */
int spa3d_op_broadcast_rows(const float* src, int32_t rows, int32_t d, void* dst, int64_t B, int32_t dtype, void* stream);
/* ... and its gradient: dparam f32 [per] += sum over b < B of dsrc[b * bstride + 0..per).  1 <= per <= bstride. */
int spa3d_op_bcast_grad(const void* dsrc, int64_t per, int64_t B, int64_t bstride, float* dparam, int32_t dtype, void* stream);

/* TRAJAN's track pooling (track_autoencoder.py:230-232): out [nseq, d] = mean of tok [nseq, T, d] over the frames with vis f32 [nseq, T] != 0 (0 when
 * there is none); backward dtok [nseq, T, d] = dout [nseq, d] / max(1, visible frames) at the visible frames, 0 elsewhere.  T, d >= 1. */
int spa3d_op_vis_mean_pool(const void* tok, const float* vis, int64_t nseq, int32_t T, int32_t d, void* out, int32_t dtype, void* stream);
int spa3d_op_vis_mean_pool_bwd(const void* dout, const float* vis, int64_t nseq, int32_t T, int32_t d, void* dtok, int32_t dtype, void* stream);

/* ---- The first mile of the model on its own (tests/test_gpu_embed.py): the embeddings, row maps, readout rows, key masks and weight shadows of
 * csrc/embed.hip and the latent quantiser of csrc/loss.hip.  Rules as for the row plumbing: `dtype` in {SPA3D_F32, SPA3D_BF16, SPA3D_F16} is the storage
 * type of every `void*` tensor; an empty input returns SPA3D_OK and launches nothing; a NULL required pointer, a negative count or a shape outside what
 * is stated returns SPA3D_ERR_ARG and launches nothing.  Everywhere 1 <= nf <= 64 (the scale table of the kernels holds 64 entries), and a scale
 * that divides is neither 0 nor NaN. ---- */

/* spa3d_op_sin_embed with the division the model applies first: out[rows, C*2*nf] = SinusoidalEmbedding(x / prescale).  1 <= C <= 65536. */
int spa3d_op_sin_embed_scaled(const float* x, int64_t rows, int32_t C, int32_t nf, float prescale, void* out, int32_t dtype, void* stream);
/* Track tokens (track_autoencoder_3d.py:126-134): out[nrows, (NC+1)*2*nf] = SinusoidalEmbedding([tracks[r][0..NC), fl32(r % T) / fl32(T)] / prescale),
 * tracks f32 [nrows, NC], NC in {2, 3}, T >= 1.  16 bytes per thread when nf is a multiple of 16 bytes and out is 16-byte aligned, else element by
 * element (out need only be element-aligned); both give the same bits. */
int spa3d_op_embed_tokens(const float* tracks, int64_t nrows, int32_t T, int32_t NC, int32_t nf, float prescale, void* out, int32_t dtype, void* stream);
/* Decoder context (track_autoencoder_3d.py:209-233, 265-272): qp f32 [nq, NC+1] = (t, coordinates); qframe[q] = round-half-even(t);
 * feat f32 [nq, NC*2*nf + 1] = [SinusoidalEmbedding(coordinates / track_scale) | floor(fl32(qframe) / time_scale)].  NC in {2, 3}. */
int spa3d_op_query_embed(const float* qp, int64_t nq, int32_t NC, int32_t nf, float track_scale, float time_scale, float* feat, int32_t* qframe, void* stream);
/* Row maps of the one-pass embedding: row j of the token buffer is dense token q = row_src[j] (row_src NULL: j) = (seq, s) of nseq sequences of
 * S = T + 1 tokens.  s >= 1: arow[j] = seq * T + s - 1 (its input row), crow[j] = j, tok row j untouched.  s == 0: arow[j] = seq * T, crow[j] = -1,
 * tok[j][0..d) = readout f32 [d] rounded once.  rows < 2^31, T >= 1, S == T + 1, d >= 1. */
int spa3d_op_embed_maps(const int32_t* row_src, int64_t rows, int32_t S, int32_t T, int32_t* arow, int32_t* crow, void* tok, const float* readout, int32_t d,
                        int32_t dtype, void* stream);
/* tok [nseq, S, d]: row 0 of every sequence = readout f32 [d] rounded once (track_autoencoder_3d.py:161-165); the other rows untouched.  S, d >= 1. */
int spa3d_op_set_readout_rows(void* tok, const float* readout, int64_t nseq, int32_t S, int32_t d, int32_t dtype, void* stream);
/* Key masks: visible f32 [nseq, T], boundary int32 [nseq / N] (sequence s belongs to sample s / N); key t is kept when visible != 0 (-0.0 dropped,
 * NaN kept) and t < boundary.  with_readout = 1: km f32 [nseq, T + 1], key 0 (the readout token) always 1; with_readout = 0: km f32 [nseq, T], the 2-D
 * model's form.  N >= 1 divides nseq, T >= 1. */
int spa3d_op_keymask(const float* visible, const int32_t* boundary, int64_t nseq, int32_t N, int32_t T, int32_t with_readout, float* km, void* stream);
/* out[i] = fl32(fl32(a[i] + b[i]) + c[i]), i < n; a NULL operand counts as 0.f, at least one is given (the fused embedding bias). */
int spa3d_op_sum3(const float* a, const float* b, const float* c, float* out, int32_t n, void* stream);
/* Weight shadows: src f32 [rows, cols] with row stride src_ld -> dn [rows, cols] with row stride ldn and dt [cols, rows] with row stride ldt (the
 * transpose), both rounded once to `dtype`; either may be NULL, not both.  src_ld >= cols, ldn >= cols, ldt >= rows, rows <= 65535 * 32. */
int spa3d_op_pack(const float* src, int64_t src_ld, int32_t rows, int32_t cols, void* dn, int64_t ldn, void* dt, int64_t ldt, int32_t dtype, void* stream);
/* dst [cols, rows] = src [rows, cols] transposed, both dense, a copy.  rows <= 65535 * 32. */
int spa3d_op_transpose(const void* src, int32_t rows, int32_t cols, void* dst, int32_t dtype, void* stream);
/* Latent clip / quantise / straight-through (track_autoencoder_3d.py:251-260), f32 [n]: l = clip(lat, -1, 1); discretize = 1:
 * q = round-half-even(l * 128) / 128 + noise / 128 - 1 / 256 and out = l - (l - q), else out = l.  clipmask (may be NULL) = 1 where -1 <= lat <= 1,
 * else 0.  A NaN latent is a NaN in out and in clipmask.  noise may be NULL when discretize = 0. */
int spa3d_op_discretize(const float* lat, const float* noise, int32_t discretize, float* out, float* clipmask, int64_t n, void* stream);

/* ---- feature producers that build the hot path's inputs.  Host pointers: `intrinsics` only. ----
 * Float32 arithmetic in the reference's operation order: bit-identical to the reference functions under NumPy >= 2. */

/* sample_dino_features_for_tracks (inference.py:339-395): feat [T,Hp,Wp,D] f32, tracks_2d [N,T,2] f32 in pixels of an
 * H x W video -> out [N,T,D] (out_dtype SPA3D_F32 as the reference, or SPA3D_BF16 = the same values rounded once). */
int spa3d_op_sample_dino(const float* feat, const float* tracks_2d, int32_t N, int32_t T, int32_t Hp, int32_t Wp, int32_t D,
                         int32_t H, int32_t W, void* out, int32_t out_dtype, void* stream);
/* sample_depth_features_for_tracks (inference.py:398-447): depth [T,H,W,1] f32 -> out [N,T,256] f32 */
int spa3d_op_sample_depth_features(const float* depth, const float* tracks_2d, int32_t N, int32_t T, int32_t H, int32_t W,
                                   float* out, void* stream);
/* lift_2d_to_3d (inference.py:287-336): intrinsics = host double[4] {fx,fy,cx,cy} or NULL (fx=fy=max(H,W), cx=W/2, cy=H/2) */
int spa3d_op_lift_2d_to_3d(const float* tracks_2d, const float* depth, int32_t N, int32_t T, int32_t H, int32_t W,
                           const double* intrinsics, float* out, void* stream);
/* test entry of the metric's exact median select: out[r] = median of the non-NaN entries of x[r][0..n) (1 if none); entries >= 0.  Two middle
 * values of an even count are averaged as 0.5f a + 0.5f b.  ws is not used (the histograms live in LDS) and may be NULL. */
int spa3d_op_median_rows(const float* x, int64_t rows, int64_t n, float* out, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPA3D_H_ */
