"""Host-side mirror of the reference's Flax module protocol for the 3DSPA hot path.

Same names, argument meaning and error behaviour as the reference call sites
(train.py:137-146,194-199,221-233; evaluate_tapvid3d.py:70-77; inference.py:594-623):

    model  = TrackAutoEncoder3D(num_output_frames=..., use_dino=..., use_depth=...)
    params = model.init(rng, batch)['params']            # nested dict, Flax names/shapes
    preds  = model.apply({'params': params}, batch)      # TrackAutoEncoderResults
    losses = compute_loss_3d(preds, batch)               # {'total_loss','position_loss','visible_loss'}
    model.apply({'params': p}, batch, method=model.encode) etc.

Everything numeric happens in libspa3d_hip.so (hand-written HIP for gfx950) through the C-ABI in
include/spa3d.h; PyTorch only owns device memory and the stream.  There is no CPU fallback.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
import math
from typing import Any, Dict, Optional

import torch

from . import _lib
from .data import fold_offsets, validate_counts


# ------------------------------------------------------------------------------------------------
# result containers (track_autoencoder.py:72-114)
# ------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class TrackAutoEncoderResults:
  tracks: torch.Tensor  # [B,Q,T,3]
  visible_logits: torch.Tensor  # [B,Q,T,1]
  certain_logits: torch.Tensor  # [B,Q,T,1]  (identically zero, track_autoencoder_3d.py:301)

  @property
  def visible(self):  # ta:93-95
    return (self.visible_logits > 0).to(torch.float32)

  @property
  def certain(self):  # ta:97-99
    return (self.certain_logits > 0).to(torch.float32)

  @property
  def visible_and_certain(self):  # ta:101-105
    return ((torch.sigmoid(self.visible_logits) * torch.sigmoid(self.certain_logits)) > 0.5).to(torch.float32)


@dataclasses.dataclass
class TrackAutoEncoderDecoderContext:
  """get_decoder_context output.  The sinusoidal query identity itself is produced inside the fused
  decode kernels; the context carries what decode needs to rebuild it: the query points."""
  query_points: torch.Tensor  # [B,Q,4] (t,x,y,z)
  query_frame: torch.Tensor  # int32 [B,Q] = round(t)
  boundary_frame: Optional[torch.Tensor]
  query_count: Any = None  # ragged batch: live queries per sample ([B] ints), None = all Q

  @property
  def decoder_query(self):  # [B,Q,192] -- materialised on demand (ta:28-37)
    return sinusoidal_embedding(self.query_points[..., 1:].contiguous())


# ------------------------------------------------------------------------------------------------
# per-track reconstruction scores (include/spa3d.h, spa3d_scores)
# ------------------------------------------------------------------------------------------------
SCORE_BASE_SLOTS = 8  # stats row: [n_vis, sum y e1, sum y e2, max e2 (visible), sum bce, occlusion-correct frames, predicted-visible frames, frames] + 4 per threshold


class _ScoreProperties:
  """Ratios of a stats tensor [..., 8 + 4K]; every denominator is clamped at 1, so a row without visible frames (or a padded row) reads 0."""

  def _stats(self) -> torch.Tensor:
    raise NotImplementedError

  def _ratio(self, num, den):
    return num / torch.clamp(den, min=1.0)

  def _per_threshold(self, offset):  # [..., K]
    s = self._stats()
    return s[..., SCORE_BASE_SLOTS + offset::4]

  @property
  def num_visible(self):
    return self._stats()[..., 0]

  @property
  def position_l1(self):
    """Mean over the visible frames of sum_c |p - g|: the training loss's L1 term of this row."""
    s = self._stats()
    return self._ratio(s[..., 1], s[..., 0])

  @property
  def distance_mean(self):
    s = self._stats()
    return self._ratio(s[..., 2], s[..., 0])

  @property
  def distance_max(self):
    return self._stats()[..., 3]

  @property
  def visible_bce(self):
    s = self._stats()
    return self._ratio(s[..., 4], s[..., 7])

  @property
  def occlusion_accuracy(self):
    s = self._stats()
    return self._ratio(s[..., 5], s[..., 7])

  @property
  def pts_within(self):
    """[..., K]: share of the visible frames whose distance is below thresholds[k] (x the sample scale)."""
    return self._ratio(self._per_threshold(0), self._stats()[..., 0:1])

  @property
  def jaccard(self):
    """[..., K]: TP / (TP + FP + FN), the TAP-Vid Jaccard counts at fixed metric thresholds (not tapnet's TAPVid-3D metric)."""
    tp, fp, fn = self._per_threshold(1), self._per_threshold(2), self._per_threshold(3)
    return self._ratio(tp, tp + fp + fn)

  @property
  def average_jaccard(self):
    j = self.jaccard
    return j.mean(-1) if j.shape[-1] else torch.zeros(j.shape[:-1], dtype=j.dtype, device=j.device)

  @property
  def average_pts_within(self):
    w = self.pts_within
    return w.mean(-1) if w.shape[-1] else torch.zeros(w.shape[:-1], dtype=w.dtype, device=w.device)


@dataclasses.dataclass
class SampleScores(_ScoreProperties):
  """Per-sample scores from the pooled counts of the sample's live queries."""
  stats: torch.Tensor  # [B, 8 + 4K] f64
  thresholds: tuple = ()

  def _stats(self):
    return self.stats


@dataclasses.dataclass
class TrackScores(_ScoreProperties):
  """What TrackAutoEncoder3D.score / score_predictions return: the raw tensors of spa3d_scores and, as properties, the per-query ratios
  (position_l1, distance_mean, distance_max, occlusion_accuracy, pts_within[k], jaccard[k], average_jaccard); `.sample` gives the same per sample."""
  query_stats: torch.Tensor  # [B, Q, 8 + 4K] f32; rows of padded queries are 0
  sample_stats: Optional[torch.Tensor]  # [B, 8 + 4K] f64
  frame_err: Optional[torch.Tensor]  # [B, Q, T] f32 Euclidean error of every frame, or None
  thresholds: tuple = ()
  predictions: Optional['TrackAutoEncoderResults'] = None  # score(return_predictions=True)

  def _stats(self):
    return self.query_stats

  @property
  def sample(self) -> SampleScores:
    if self.sample_stats is None:
      raise ValueError('these scores carry no sample_stats')
    return SampleScores(self.sample_stats, self.thresholds)


@dataclasses.dataclass
class VideoScores:
  """What TrackAutoEncoder3D.score_video returns: one clip of n tracks over its own TL frames, in the clip's own track order."""
  tracks: Optional[torch.Tensor]  # [n, TL, 3] blended predictions (None without return_predictions)
  visible_logits: Optional[torch.Tensor]  # [n, TL]
  frame_err: torch.Tensor  # [n, TL] the windows' per-point errors, blended
  spread: torch.Tensor  # [n, TL] the windows' disagreement about the point (0 under one window)
  targets_tracks: torch.Tensor  # [n, TL, 3] the clip's own (lifted) tracks, as the windows held them
  targets_visible: torch.Tensor  # [n, TL]
  scores: TrackScores  # score_predictions of the blended predictions against the targets: [1, n, ..], over all TL frames
  window_start: Any  # np.int32 [W]
  perm: Any  # np.int64 [n]: track perm[r] was row r of every window

  @property
  def targets(self):
    """The targets as score_predictions takes them (a batch of one clip)."""
    return {'query_tracks': self.targets_tracks[None], 'query_tracks_visible': self.targets_visible[None, :, :, None]}


def _fold_offsets_of(folds, N):
  """score_all's `folds`: an int (fold_offsets) or an offsets array [F + 1]; the checked offsets, ValueError otherwise."""
  import numpy as np
  if isinstance(folds, (int, np.integer)) and not isinstance(folds, bool):
    return fold_offsets(N, int(folds))
  off = folds.detach().cpu().numpy() if isinstance(folds, torch.Tensor) else np.asarray(folds)
  if off.ndim != 1 or off.size < 3 or off.size > 65 or off.dtype.kind not in 'iu':
    raise ValueError('folds must be an int or an integer offsets array [F + 1] with 2 <= F <= 64')
  off = off.astype('int64')
  if off[0] != 0 or off[-1] != N or (off[1:] <= off[:-1]).any():
    raise ValueError(f'fold offsets must start at 0, increase strictly and end at N = {N}, got {off.tolist()}')
  return off


def _check_thresholds(thresholds):
  thr = tuple(float(t) for t in thresholds)
  if len(thr) > 8:
    raise ValueError(f'at most 8 thresholds, got {len(thr)}')
  for t in thr:
    if not (math.isfinite(t) and t > 0):
      raise ValueError(f'thresholds must be finite and positive, got {t!r}')
  return thr


def _alloc_scores(thr, B, Q, To, dev, sample_scale, frame_errors):
  """Result tensors and the spa3d_scores block that points at them; the second value keeps what the block references alive."""
  S = SCORE_BASE_SLOTS + 4 * len(thr)
  res = TrackScores(torch.empty(B, Q, S, dtype=torch.float32, device=dev), torch.empty(B, S, dtype=torch.float64, device=dev),
                    torch.empty(B, Q, To, dtype=torch.float32, device=dev) if frame_errors else None, thr)
  sc = _lib.Scores()
  sc.num_thresholds = len(thr)
  for i, t in enumerate(thr):
    sc.thresholds[i] = t
  keep = None
  if sample_scale is not None:
    keep = sample_scale if isinstance(sample_scale, torch.Tensor) else torch.as_tensor(sample_scale, dtype=torch.float32, device=dev)
    _require_cuda(keep, 'sample_scale')
    keep = keep.to(torch.float32).contiguous()
    if keep.numel() != B:
      raise ValueError(f'sample_scale must have one entry per sample (B = {B}), got {keep.numel()}')
    sc.sample_scale = keep.data_ptr()
  sc.query_stats, sc.sample_stats = res.query_stats.data_ptr(), res.sample_stats.data_ptr()
  sc.frame_err = res.frame_err.data_ptr() if frame_errors else None
  return res, sc, keep


# ------------------------------------------------------------------------------------------------
# TAPVid-3D metrics (include/spa3d.h, spa3d_tapvid3d): restated from the published definition, parity unpinned
# ------------------------------------------------------------------------------------------------
TAPVID3D_SLOTS = 24  # [evaluated frames, visible, occlusion-correct, predicted visible] + (W, TP, FP, FN) per pixel threshold
TAPVID3D_PIXELS = (1, 2, 4, 8, 16)
TAPVID3D_SCALINGS = {'none': 0, 'median': 1, 'per_trajectory': 2}


class _TapVid3DProperties:
  """Ratios of a stats tensor [..., 24]; a zero denominator gives 0, as _ScoreProperties does."""

  def _stats(self) -> torch.Tensor:
    raise NotImplementedError

  def _ratio(self, num, den):
    return num / torch.clamp(den, min=1.0)

  @property
  def occlusion_accuracy(self):
    s = self._stats()
    return self._ratio(s[..., 2], s[..., 0])

  @property
  def pts_within(self):
    """[..., 5]: share of the evaluated visible frames within the 1, 2, 4, 8, 16 pixel thresholds."""
    s = self._stats()
    return self._ratio(s[..., 4::4], s[..., 1:2])

  @property
  def jaccard(self):
    """[..., 5]: TP / (visible + FP) = TP / (TP + FN + FP)."""
    s = self._stats()
    return self._ratio(s[..., 5::4], s[..., 1:2] + s[..., 6::4])

  @property
  def average_jaccard(self):
    return self.jaccard.mean(-1)

  @property
  def average_pts_within_thresh(self):
    return self.pts_within.mean(-1)


@dataclasses.dataclass
class TapVid3DSampleScores(_TapVid3DProperties):
  """Per-clip metrics from the pooled counts of the clip's live queries: what the reference's evaluation reports per video."""
  stats: torch.Tensor  # [B, 24] f64 (or [24] after split_ragged)
  scaling: str = 'median'

  def _stats(self):
    return self.stats


@dataclasses.dataclass
class TapVid3DScores(_TapVid3DProperties):
  """What tapvid3d_predictions / TrackAutoEncoder3D.tapvid3d return: the raw tensors of spa3d_tapvid3d and, as properties, the per-query
  ratios (occlusion_accuracy, pts_within[k], jaccard[k], average_jaccard, average_pts_within_thresh); `.sample` gives the same per clip."""
  query_stats: torch.Tensor  # [B, Q, 24] f32; rows of padded queries are 0
  sample_stats: torch.Tensor  # [B, 24] f64
  scale: torch.Tensor  # [B] f32: the factor applied per sample (1 for none / per_trajectory)
  row_scale: torch.Tensor  # [B, Q] f32: the factor each row's predictions were multiplied by
  ratio: Optional[torch.Tensor] = None  # [B, Q, T] f32 |gt| / |pred| of every frame (ratios=True)
  scaling: str = 'median'
  fixed_thresholds: bool = False

  def _stats(self):
    return self.query_stats

  @property
  def sample(self) -> TapVid3DSampleScores:
    return TapVid3DSampleScores(self.sample_stats, self.scaling)

  def as_dict(self, b: int = 0) -> Dict[str, float]:
    """The 13 keys compute_tapvid3d_metrics returns, for clip b (one host read of the clip's 24 pooled counts)."""
    s = self.sample_stats if self.sample_stats.dim() == 1 else self.sample_stats[b]
    one = TapVid3DSampleScores(s.detach().to('cpu', torch.float64), self.scaling)
    out = {'occlusion_accuracy': float(one.occlusion_accuracy)}
    w, j = one.pts_within.tolist(), one.jaccard.tolist()
    for k, px in enumerate(TAPVID3D_PIXELS):
      out[f'pts_within_{px}'] = w[k]
      out[f'jaccard_{px}'] = j[k]
    out['average_jaccard'] = float(one.average_jaccard)
    out['average_pts_within_thresh'] = float(one.average_pts_within_thresh)
    return out


def _check_scaling(scaling) -> str:
  if scaling not in TAPVID3D_SCALINGS:
    raise ValueError(f"scaling must be one of {sorted(TAPVID3D_SCALINGS)} (tapnet's 'local_neighborhood' is not implemented), got {scaling!r}")
  return scaling


class ParamTree(dict):
  """Nested dict of parameter views; the root carries the flat fp32 buffer the views alias."""
  flat: Optional[torch.Tensor] = None


def sinusoidal_embedding(x: torch.Tensor, num_frequencies: int = 32) -> torch.Tensor:
  """SinusoidalEmbedding (track_autoencoder.py:18-38) on the GPU kernel."""
  lib = _lib.load()
  x = x.to(torch.float32).contiguous()
  rows = x.numel() // x.shape[-1]
  out = torch.empty(*x.shape[:-1], x.shape[-1] * 2 * num_frequencies, device=x.device, dtype=torch.float32)
  _lib.check(lib.spa3d_op_sin_embed(x.data_ptr(), rows, x.shape[-1], num_frequencies, out.data_ptr(), _lib.F32, _stream(x)),
             what='spa3d_op_sin_embed')
  return out


def _stream(t: torch.Tensor):
  return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


@contextlib.contextmanager
def _counts_on(h, b):
  """States the per-sample counts that _marshal found in the batch (b.counts) on the handle for the calls inside the block and detaches
  them afterwards, so that a later plain batch on the same handle is not affected."""
  cn, cq = getattr(b, 'counts', (None, None))
  if cn is None and cq is None:
    yield
    return
  lib = _lib.load()
  arr = lambda v: (C.c_int32 * len(v))(*v) if v is not None else None
  _lib.check(lib.spa3d_set_counts(h, b.B, arr(cn), arr(cq)), h, 'spa3d_set_counts')  # (the library copies the entries)
  try:
    yield
  finally:
    lib.spa3d_set_counts(h, 0, None, None)


# ------------------------------------------------------------------------------------------------
# the training objective (include/spa3d.h, spa3d_loss_config)
# ------------------------------------------------------------------------------------------------
POS_L1, POS_HUBER = 0, 1


@dataclasses.dataclass(frozen=True)
class LossConfig:
  """spa3d_loss_config: the objective of loss_and_grads / TrainState / compute_loss_3d(loss=...).  The defaults are the reference's
  (train.py:96).  position_kind POS_L1 or POS_HUBER (delta = huber_delta, L1's slope in the tails); axis_weight per coordinate (the 2-D model
  reads two); bce_pos_weight as torch's pos_weight.  Validated with the library's rules (ValueError here, SPA3D_ERR_ARG there)."""
  l1_weight: float = 5000.0
  bce_weight: float = 1e-8
  position_kind: int = POS_L1
  huber_delta: float = 1.0
  axis_weight: tuple = (1.0, 1.0, 1.0)
  bce_pos_weight: float = 1.0

  def __post_init__(self):
    self.validate(3)

  def validate(self, nc: int = 3):
    """The refusals of spa3d_set_loss for a model of `nc` coordinates, on the values as the library sees them (float32)."""
    f32 = lambda v: C.c_float(float(v)).value
    if isinstance(self.position_kind, bool) or self.position_kind not in (POS_L1, POS_HUBER):
      raise ValueError(f'position_kind must be POS_L1 (0) or POS_HUBER (1), got {self.position_kind!r}')
    ax = tuple(self.axis_weight)
    if len(ax) != 3:
      raise ValueError(f'axis_weight must have 3 entries (the 2-D model reads the first two), got {len(ax)}')
    huber = self.position_kind == POS_HUBER
    l1, bce, beta, delta = f32(self.l1_weight), f32(self.bce_weight), f32(self.bce_pos_weight), f32(self.huber_delta)
    ax = tuple(f32(a) for a in ax)
    if not all(math.isfinite(v) for v in (l1, bce, beta) + ax[:nc] + ((delta,) if huber else ())):
      raise ValueError('every field of a LossConfig must be finite')
    if l1 < 0 or bce < 0 or beta < 0 or any(a < 0 for a in ax[:nc]):
      raise ValueError('l1_weight, bce_weight, axis_weight and bce_pos_weight must not be negative')
    if huber and not delta > 0:
      raise ValueError(f'huber_delta must be positive with POS_HUBER, got {self.huber_delta!r}')
    amax = max(ax[:nc])
    if l1 > 0 and not amax > 0:
      raise ValueError(f"l1_weight > 0 needs a positive axis_weight among the model's {nc} coordinates")
    gmax = max(f32(l1 * amax), f32(bce * max(1.0, beta)))
    if not (0 < gmax <= 2.0 ** 30):
      raise ValueError(f'the largest head gradient max(l1_weight * max axis_weight, bce_weight * max(1, bce_pos_weight)) = {gmax!r} must lie in (0, 2^30]')
    return self

  def as_struct(self):
    s = _lib.LossConfig()
    s.l1_weight, s.bce_weight, s.position_kind, s.huber_delta, s.bce_pos_weight = self.l1_weight, self.bce_weight, int(self.position_kind), self.huber_delta, self.bce_pos_weight
    for i, a in enumerate(self.axis_weight):
      s.axis_weight[i] = a
    return s


def _point_weights(w, B, Q, To):
  """batch['query_weight'] ([B,Q,T] or [B,Q,T,1]) as the contiguous float32 plane the library reads; None stays None."""
  if w is None:
    return None
  _require_cuda(w, 'query_weight')
  if tuple(w.shape) not in ((B, Q, To), (B, Q, To, 1)):
    raise ValueError(f'query_weight must be {(B, Q, To)} or {(B, Q, To, 1)}, got {tuple(w.shape)}')
  return w if (w.dtype == torch.float32 and w.is_contiguous()) else w.to(torch.float32).contiguous()


@contextlib.contextmanager
def _loss_on(h, loss, weights, B, Q, nc):
  """States the objective and the point weights on the handle for the calls inside the block and takes both off afterwards (as _counts_on
  does with the counts): a handle shared by several owners never carries one owner's objective into another's call."""
  if loss is None and weights is None:
    yield
    return
  lib = _lib.load()
  if loss is not None:
    if not isinstance(loss, LossConfig):
      raise TypeError(f'loss must be a LossConfig or None, got {type(loss).__name__}')
    loss.validate(nc)
    cfg = loss.as_struct()
    _lib.check(lib.spa3d_set_loss(h, C.byref(cfg)), h, 'spa3d_set_loss')
  try:
    if weights is not None:
      _lib.check(lib.spa3d_set_point_weights(h, B, Q, weights.data_ptr()), h, 'spa3d_set_point_weights')
    yield
  finally:
    lib.spa3d_set_point_weights(h, 0, 0, None)
    if loss is not None:
      lib.spa3d_set_loss(h, None)


FREEZE_ALIASES = {'none': 0, 'encoder': 1, 'encoder+latents': 2}


def freeze_level(freeze) -> int:
  """0 | 1 | 2, or the aliases 'none' | 'encoder' | 'encoder+latents' (include/spa3d.h, spa3d_set_option "freeze")."""
  k = FREEZE_ALIASES.get(freeze, freeze) if isinstance(freeze, str) else freeze
  if isinstance(k, bool) or not isinstance(k, int) or k not in (0, 1, 2):
    raise ValueError(f"freeze must be 0, 1, 2 or one of {sorted(FREEZE_ALIASES)}, got {freeze!r}")
  return k


def trainable_range(h):
  """(lo, n) of the handle's stored "freeze" option: the range of the flat buffer a training call writes gradients into (spa3d_trainable_range)."""
  r = (C.c_int64 * 2)()
  _lib.check(_lib.load().spa3d_trainable_range(h, r), h, 'spa3d_trainable_range')
  return int(r[0]), int(r[1])


@contextlib.contextmanager
def _freeze_on(h, freeze):
  """States the "freeze" option on the handle for the calls inside the block (sizing included: spa3d_workspace_bytes follows it) and puts the value it
  found back afterwards, as _loss_on does with the objective: an SPA3D_FREEZE preset or another owner's setting survives the call."""
  k = freeze_level(freeze)
  lib = _lib.load()
  b4 = (C.c_int64 * 4)()
  _lib.check(lib.spa3d_grad_segments(h, b4), h, 'spa3d_grad_segments')
  prev = list(b4[:3]).index(trainable_range(h)[0])
  if prev == k:
    yield
    return
  _lib.check(lib.spa3d_set_option(h, b'freeze', float(k)), h, 'spa3d_set_option')
  try:
    yield
  finally:
    lib.spa3d_set_option(h, b'freeze', float(prev))


def _require_cuda(t: torch.Tensor, name: str):
  if not t.is_cuda:
    raise _lib.Spa3dError(f'{name} must live on the GPU: the 3DSPA hot path is HIP-only (no CPU fallback)')


# precision name -> (spa3d_config::precision, dtype of the DINO / depth feature planes handed to the library)
_PRECISIONS = {'fp32': (_lib.F32, torch.float32), 'bf16': (_lib.BF16, torch.bfloat16), 'fp16': (_lib.F16, torch.float16)}


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
class TrackAutoEncoder3D:
  """Drop-in for track_autoencoder_3d.TrackAutoEncoder3D (fields of 3d:53-67)."""

  def __init__(self, num_output_frames: int = 150, num_latent_tokens: int = 128, latent_token_dim: int = 96,
               num_frequencies: int = 32, track_scale_factor: float = 1.0, time_scale_factor: float = 150.0,
               track_token_dim: int = 384, encoder_latent_dim: int = 512, decoder_num_channels: int = 1280,
               dino_feature_dim: int = 768, depth_feature_dim: int = 256, use_dino: bool = True, use_depth: bool = True,
               decoder_scan_chunk_size: Optional[int] = None, precision: str = 'bf16',
               workspace_fraction: float = 0.80, track_chunk_size: Optional[int] = None):
    # track_chunk_size is NOT part of the reference's signature (product-only): the track encoder runs over chunks of that many tracks and is
    # recomputed chunk by chunk in the backward (spa3d_set_option "track_chunk"; one extra encoder forward per training step)
    if precision not in _PRECISIONS:
      raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}, got {precision!r}")
    self.num_output_frames = num_output_frames
    self.num_latent_tokens = num_latent_tokens
    self.latent_token_dim = latent_token_dim
    self.num_frequencies = num_frequencies
    self.track_scale_factor = track_scale_factor
    self.time_scale_factor = time_scale_factor
    self.track_token_dim = track_token_dim
    self.encoder_latent_dim = encoder_latent_dim
    self.decoder_num_channels = decoder_num_channels
    self.dino_feature_dim = dino_feature_dim
    self.depth_feature_dim = depth_feature_dim
    self.use_dino = use_dino
    self.use_depth = use_depth
    # 3d:312-349: the readout runs over chunks of this many queries (spa3d_set_option "query_chunk"); Q must be a multiple of it
    self.decoder_scan_chunk_size = decoder_scan_chunk_size
    self.track_chunk_size = track_chunk_size
    self.precision = precision
    self.workspace_fraction = workspace_fraction
    # transformer sizes of setup() (3d:89-112)
    self.num_heads, self.qkv_size = 8, 96 * 8
    self.enc_mlp, self.enc_layers = 1536, 3
    self.t2l_mlp, self.t2l_layers = 2048, 4
    self.dec_mlp, self.dec_layers = 2048, 4
    self.ro_mlp, self.ro_layers = 1536, 4
    if self.qkv_size % self.num_heads:  # attention.py:147-148
      raise ValueError(f'self.num_heads={self.num_heads} must divide self.qk_size={self.qkv_size}.')
    self._handles: Dict[Any, Any] = {}
    self._ws: Optional[torch.Tensor] = None
    self._kind, self._nc = 0, 3  # 0: 3DSPA (x,y,z); the 2-D TRAJAN subclass sets (1, 2)
    self._chunk_set: Dict[Any, Any] = {}  # handle -> (query_chunk, track_chunk) last stated by _chunk_options
    self._ws_cap = 0  # size of a budget-limited workspace (0: none / large enough for every request so far)

  # -------------------------------------------------------------------------------- handles / layout
  @property
  def act_dtype(self):
    return _PRECISIONS[self.precision][1]

  def _handle(self, dino_dim: int, depth_dim: int):
    key = (dino_dim, depth_dim)
    if key not in self._handles:
      # the last block of the readout stack runs the single-query attention kernels, which exist for these head widths only (SPA3D_ERR_ARG in spa3d_create)
      if self.num_heads > 0 and self.qkv_size % self.num_heads == 0 and self.qkv_size // self.num_heads not in (8, 16, 32, 64, 96, 128):
        raise ValueError(f'head width qkv_size / num_heads = {self.qkv_size // self.num_heads} must be one of 8, 16, 32, 64, 96, 128')
      lib = _lib.load()
      cfg = _lib.Config(self.num_output_frames, self.num_latent_tokens, self.latent_token_dim, self.num_frequencies,
                        self.track_scale_factor, self.time_scale_factor, self.track_token_dim, self.encoder_latent_dim,
                        self.decoder_num_channels, dino_dim, depth_dim, self.num_heads, self.qkv_size, self.enc_mlp,
                        self.enc_layers, self.t2l_mlp, self.t2l_layers, self.dec_mlp, self.dec_layers, self.ro_mlp,
                        self.ro_layers, _PRECISIONS[self.precision][0], self._kind)
      h = C.c_void_p()
      _lib.check(lib.spa3d_create(C.byref(cfg), C.byref(h)), what='spa3d_create')
      leaves = []
      name = C.create_string_buffer(160)
      nd = C.c_int32()
      shape = (C.c_int64 * 4)()
      off = C.c_int64()
      for i in range(lib.spa3d_num_leaves(h)):
        _lib.check(lib.spa3d_leaf_info(h, i, name, C.byref(nd), shape, C.byref(off)), h, 'spa3d_leaf_info')
        leaves.append((name.value.decode(), tuple(shape[k] for k in range(nd.value)), off.value))
      self._handles[key] = (h, leaves, lib.spa3d_param_elems(h))
    return self._handles[key]

  def _dims_from_batch(self, batch):
    dino = batch['dino_features'].shape[-1] if (self.use_dino and batch.get('dino_features') is not None) else 0
    depth = batch['depth_features'].shape[-1] if (self.use_depth and batch.get('depth_features') is not None) else 0
    return dino, depth

  @staticmethod
  def _dims_from_params(params):
    dino = params['dino_projection']['kernel'].shape[0] if 'dino_projection' in params else 0
    depth = params['depth_projection']['kernel'].shape[0] if 'depth_projection' in params else 0
    return dino, depth

  def tree_from_flat(self, flat: torch.Tensor, dino_dim: int, depth_dim: int) -> ParamTree:
    _, leaves, n = self._handle(dino_dim, depth_dim)
    assert flat.numel() == n and flat.dtype == torch.float32
    root = ParamTree()
    for name, shape, off in leaves:
      d = root
      parts = name.split('/')
      for q in parts[:-1]:
        d = d.setdefault(q, {})
      d[parts[-1]] = flat[off:off + math.prod(shape)].view(shape)
    root.flat = flat
    return root

  def flat_from_tree(self, params, device=None) -> torch.Tensor:
    """Returns the flat fp32 buffer behind `params` (zero-copy for a ParamTree, packed copy otherwise)."""
    if isinstance(params, ParamTree) and params.flat is not None:
      return params.flat
    dino, depth = self._dims_from_params(params)
    _, leaves, n = self._handle(dino, depth)
    first = params['initializer']['state_init']
    device = device or (first.device if isinstance(first, torch.Tensor) else 'cuda')
    flat = torch.zeros(n, dtype=torch.float32, device=device)
    for name, shape, off in leaves:
      d = params
      for q in name.split('/'):
        if q not in d:
          raise KeyError(f'parameter tree is missing {name!r}')  # cf. inference.py:608-619
        d = d[q]
      t = torch.as_tensor(d)
      if tuple(t.shape) != tuple(shape):
        raise ValueError(f'shape mismatch for {name}: expected {shape}, got {tuple(t.shape)}')
      flat[off:off + t.numel()] = t.to(device=device, dtype=torch.float32).reshape(-1)
    return flat

  # -------------------------------------------------------------------------------- init (train.py:233)
  def init(self, rng, batch, device=None):
    """model.init(rng, dummy_batch) -> {'params': tree}.  Flax default initialisers: lecun-normal (truncated)
    kernels, zero biases, unit norm scales, normal(1) `state_init`.  `rng`: int seed or torch.Generator.
    As in Flax, dino/depth projection leaves exist only if the batch carries those keys (3d:140,145)."""
    dino, depth = self._dims_from_batch(batch)
    _, leaves, n = self._handle(dino, depth)
    if device is None:
      st = batch.get('support_tracks')
      device = st.device if isinstance(st, torch.Tensor) and st.is_cuda else 'cuda'
    gen = rng if isinstance(rng, torch.Generator) else torch.Generator().manual_seed(int(rng))
    host = torch.zeros(n, dtype=torch.float32)
    for name, shape, off in leaves:
      numel = math.prod(shape)
      leaf = name.rsplit('/', 1)[-1]
      if leaf == 'kernel':
        fan_in = math.prod(shape[:-1]) if name.endswith('dense_out/kernel') else shape[0]
        std = math.sqrt(1.0 / fan_in) / 0.87962566103423978
        t = torch.empty(numel, dtype=torch.float32)
        torch.nn.init.trunc_normal_(t, 0.0, 1.0, -2.0, 2.0, generator=gen)
        host[off:off + numel] = t * std
      elif leaf == 'scale':
        host[off:off + numel] = 1.0
      elif leaf == 'state_init':
        host[off:off + numel] = torch.randn(numel, generator=gen)
      # bias: zeros
    flat = host.to(device)
    return {'params': self.tree_from_flat(flat, dino, depth)}

  # -------------------------------------------------------------------------------- batch marshalling
  def _f32(self, t, name):
    _require_cuda(t, name)
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()

  def _marshal(self, inputs, dino_dim, depth_dim, need_support=True, need_query=True, targets=False, discretize=True,
               noise=None, query_points=None, query_count=None):
    keep = []  # keeps converted tensors alive until the call was enqueued
    b = _lib.Batch()
    st = inputs.get('support_tracks')
    if need_support:
      if st is None or inputs.get('support_tracks_visible') is None or inputs.get('boundary_frame') is None:
        raise KeyError('inputs need support_tracks, support_tracks_visible and boundary_frame')
      st = self._f32(st, 'support_tracks')
      vis = self._f32(inputs['support_tracks_visible'], 'support_tracks_visible')
      if st.dim() != 4 or st.shape[-1] != self._nc:
        raise ValueError(f'support_tracks must be [B,N,T,{self._nc}], got {tuple(st.shape)}')
      if tuple(vis.shape[:3]) != tuple(st.shape[:3]):
        raise ValueError('support_tracks_visible must be [B,N,T,1]')
      bf = inputs['boundary_frame']
      _require_cuda(bf, 'boundary_frame')
      bf = bf.to(torch.int32).contiguous()
      B, N, T = st.shape[:3]
      keep += [st, vis, bf]
      b.B, b.N, b.T = B, N, T
      b.support_tracks, b.support_tracks_visible, b.boundary_frame = st.data_ptr(), vis.data_ptr(), bf.data_ptr()
      for key, dim, field in (('dino_features', dino_dim, 'dino_features'), ('depth_features', depth_dim, 'depth_features')):
        if dim > 0:
          f = inputs.get(key)
          if f is None:
            raise KeyError(f'parameters contain a {key[:-9]}_projection but the batch has no {key!r}')
          _require_cuda(f, key)
          if tuple(f.shape) != (B, N, T, dim):
            raise ValueError(f'{key} must be {(B, N, T, dim)}, got {tuple(f.shape)}')
          f = f if (f.dtype == self.act_dtype and f.is_contiguous()) else f.to(self.act_dtype).contiguous()
          keep.append(f)
          setattr(b, field, f.data_ptr())
    if need_query:
      qp = query_points if query_points is not None else inputs.get('query_points')
      if qp is None:
        qp = self.default_query_grid(inputs['support_tracks'])
      qp = self._f32(qp, 'query_points')
      if qp.dim() != 3 or qp.shape[-1] != self._nc + 1:
        raise ValueError(f'query_points must be [B,Q,{self._nc + 1}], got {tuple(qp.shape)}')
      if need_support and qp.shape[0] != b.B:
        raise ValueError('query_points batch dimension does not match support_tracks')
      keep.append(qp)
      b.B = qp.shape[0]
      b.Q = qp.shape[1]
      b.query_points = qp.data_ptr()
    else:
      b.Q = 1
    b.discretize = 1 if discretize else 0
    if noise is not None:
      nz = self._f32(noise, 'noise')
      if tuple(nz.shape) != (b.B, self.num_latent_tokens, self.latent_token_dim):
        raise ValueError('noise must be [B, num_latent_tokens, latent_token_dim]')
      keep.append(nz)
      b.noise = nz.data_ptr()
    if targets:
      To = self.num_output_frames
      qt = self._f32(inputs['query_tracks'], 'query_tracks')
      qv = self._f32(inputs['query_tracks_visible'], 'query_tracks_visible')
      if tuple(qt.shape) != (b.B, b.Q, To, self._nc) or tuple(qv.shape[:3]) != (b.B, b.Q, To):
        raise ValueError(f'query_tracks must be {(b.B, b.Q, To, self._nc)} and query_tracks_visible {(b.B, b.Q, To, 1)}')
      keep += [qt, qv]
      b.query_tracks, b.query_tracks_visible = qt.data_ptr(), qv.data_ptr()
      b.weights = _point_weights(inputs.get('query_weight'), b.B, b.Q, To)  # optional per-point loss weights; _loss_on states them
    # ragged batch: optional per-sample counts (rows at or beyond a count are padding the library never reads); _counts_on states them
    cn = validate_counts(inputs.get('support_count'), b.B, b.N, 'support_count', 1) if need_support else None
    cq = validate_counts(query_count if query_count is not None else inputs.get('query_count'), b.B, b.Q, 'query_count', 0) if need_query else None
    if (cn is not None or cq is not None) and self._kind == 1:
      raise ValueError('support_count / query_count are not supported by the 2-D model')
    b.counts = (cn, cq)
    return b, keep

  def default_query_grid(self, support_tracks):
    """32x32 grid with z=0 and frame 0 when no query_points are given (3d:215-226)."""
    dev = support_tracks.device
    g = torch.arange(32, dtype=torch.float32, device=dev) / 32.0 + 1.0 / 64.0
    qx, qy = torch.meshgrid(g, g, indexing='xy')
    cols = [torch.zeros_like(qx), qx, qy] + ([torch.zeros_like(qx)] if self._nc == 3 else [])  # z = 0 in 3-D (3d:218)
    q = torch.stack(cols, dim=-1).reshape(-1, self._nc + 1)
    return q[None].expand(support_tracks.shape[0], -1, -1).contiguous()

  def _chunk_options(self, h, Q: Optional[int]):
    """States the intra-sample chunk sizes on the handle before a call.  Q: the call's query count (None: no readout)."""
    qc, tc = self.decoder_scan_chunk_size, self.track_chunk_size
    for name, v in (('decoder_scan_chunk_size', qc), ('track_chunk_size', tc)):
      if v is not None and (not isinstance(v, int) or isinstance(v, bool) or v <= 0):
        raise ValueError(f'{name} must be a positive int or None, got {v!r}')
    if qc is not None and Q is not None and Q % qc:  # as the reference's rearrange('(Q H) ...') over the scan (3d:312-349)
      raise ValueError(f'decoder_scan_chunk_size={qc} must divide the number of queries Q={Q}')
    # a size left at None leaves the handle's option alone (an SPA3D_QUERY_CHUNK / SPA3D_TRACK_CHUNK preset stays in force) unless this model set it before
    lib = _lib.load()
    prev = self._chunk_set.get(h.value, (None, None))
    for name, v, p in ((b'query_chunk', qc, prev[0]), (b'track_chunk', tc, prev[1])):
      if v is not None or p is not None:
        _lib.check(lib.spa3d_set_option(h, name, float(v or 0)), h, 'spa3d_set_option')
    self._chunk_set[h.value] = (qc, tc)

  # -------------------------------------------------------------------------------- workspace
  def _workspace(self, h, B, N, Q, T, train, device):
    lib = _lib.load()
    want = lib.spa3d_workspace_bytes(h, B, max(N, 1), Q, max(T, 1), B, 1 if train else 0)
    floor = lib.spa3d_workspace_bytes(h, B, max(N, 1), Q, max(T, 1), 1, 1 if train else 0)
    have = self._ws.numel() if (self._ws is not None and self._ws.device == torch.device(device)) else 0
    if have >= want or (self._ws_cap > 0 and have >= max(floor, self._ws_cap)):
      return self._ws  # big enough for the whole batch, or a budget cap was hit before and this is already that large
    free, _total = torch.cuda.mem_get_info(device)
    budget = int((free + have) * self.workspace_fraction)
    size = min(want, max(budget, floor))
    if size > have:
      self._ws = None
      torch.cuda.empty_cache()
      self._ws = torch.empty(size, dtype=torch.uint8, device=device)
      self._ws_cap = size if size < want else 0
    return self._ws

  # -------------------------------------------------------------------------------- public methods
  def encode(self, variables, inputs):
    """TrackAutoEncoder3D.encode (3d:190-204) -> latents [B, 128, 96] (fp32)."""
    params = variables['params'] if 'params' in variables and isinstance(variables['params'], dict) else variables
    dino, depth = self._dims_from_params(params)
    h, _, _ = self._handle(dino, depth)
    b, keep = self._marshal(inputs, dino, depth, need_query=False)
    flat = self.flat_from_tree(params)
    dev = flat.device
    lat = torch.empty(b.B, self.num_latent_tokens, self.latent_token_dim, dtype=torch.float32, device=dev)
    self._chunk_options(h, None)
    ws = self._workspace(h, b.B, b.N, 1, b.T, False, dev)
    with _counts_on(h, b):
      _lib.check(_lib.load().spa3d_encode(h, flat.data_ptr(), C.byref(b), lat.data_ptr(), ws.data_ptr(), ws.numel(), _stream(flat)),
                 h, 'spa3d_encode')
    return lat

  def motion_codes(self, variables, inputs):
    """The integer codes of the batch's latents (include/spa3d.h, "Latent-set metrics"): `encode`, then spa3d_motion_codes -> int16
    [B, num_latent_tokens, latent_token_dim], what MotionStats.update, motion_pdist and precision_recall take.  ValueError on a NaN latent."""
    from .motion import motion_codes
    return motion_codes(self.encode(variables, inputs))

  def get_decoder_context(self, inputs):
    """3d:206-233."""
    qp = inputs.get('query_points')
    if qp is None:
      qp = self.default_query_grid(inputs['support_tracks'])
    qp = qp.to(torch.float32)
    return TrackAutoEncoderDecoderContext(qp, torch.round(qp[..., 0]).to(torch.int32), inputs.get('boundary_frame'), inputs.get('query_count'))

  def decode(self, variables, latents, decoder_context, discretize: bool = True, noise=None):
    """TrackAutoEncoder3D.decode (3d:248-307)."""
    params = variables['params'] if 'params' in variables and isinstance(variables['params'], dict) else variables
    dino, depth = self._dims_from_params(params)
    h, _, _ = self._handle(dino, depth)
    flat = self.flat_from_tree(params)
    dev = flat.device
    b, keep = self._marshal({}, dino, depth, need_support=False, discretize=discretize, noise=noise,
                            query_points=decoder_context.query_points, query_count=getattr(decoder_context, 'query_count', None))
    lat = self._f32(latents, 'latents')
    if tuple(lat.shape) != (b.B, self.num_latent_tokens, self.latent_token_dim):
      raise ValueError('latents must be [B, num_latent_tokens, latent_token_dim]')
    self._chunk_options(h, b.Q)
    res, out = self._alloc_outputs(b.B, b.Q, dev)
    ws = self._workspace(h, b.B, 1, b.Q, 1, False, dev)
    with _counts_on(h, b):
      _lib.check(_lib.load().spa3d_decode(h, flat.data_ptr(), C.byref(b), lat.data_ptr(), C.byref(out), ws.data_ptr(), ws.numel(),
                                          _stream(flat)), h, 'spa3d_decode')
    return res

  def _alloc_outputs(self, B, Q, dev):
    To = self.num_output_frames
    res = TrackAutoEncoderResults(
        torch.empty(B, Q, To, self._nc, dtype=torch.float32, device=dev), torch.empty(B, Q, To, 1, dtype=torch.float32, device=dev),
        torch.empty(B, Q, To, 1, dtype=torch.float32, device=dev))
    out = _lib.Outputs(res.tracks.data_ptr(), res.visible_logits.data_ptr(), res.certain_logits.data_ptr(), None)
    return res, out

  def __call__(self, variables, inputs, discretize: bool = True, noise=None):
    params = variables['params'] if 'params' in variables and isinstance(variables['params'], dict) else variables
    dino, depth = self._dims_from_params(params)
    h, _, _ = self._handle(dino, depth)
    flat = self.flat_from_tree(params)
    dev = flat.device
    b, keep = self._marshal(inputs, dino, depth, discretize=discretize, noise=noise)
    self._chunk_options(h, b.Q)
    res, out = self._alloc_outputs(b.B, b.Q, dev)
    ws = self._workspace(h, b.B, b.N, b.Q, b.T, False, dev)
    with _counts_on(h, b):
      _lib.check(_lib.load().spa3d_forward(h, flat.data_ptr(), C.byref(b), C.byref(out), ws.data_ptr(), ws.numel(), _stream(flat)),
                 h, 'spa3d_forward')
    return res

  def score(self, variables, batch, thresholds=(), sample_scale=None, return_predictions: bool = False, frame_errors: bool = False,
            discretize: bool = True, noise=None) -> TrackScores:
    """Forward pass + per-track reconstruction scores against the batch's targets in one call (spa3d_score): no [B,Q,T,.] prediction tensor is
    written unless return_predictions.  thresholds: up to 8 distances (in the units of the tracks); sample_scale: [B] factors on every
    threshold (scene-relative thresholds).  Fixed metric thresholds -- not tapnet's TAPVid-3D metric."""
    thr = _check_thresholds(thresholds)
    params = variables['params'] if 'params' in variables and isinstance(variables['params'], dict) else variables
    dino, depth = self._dims_from_params(params)
    h, _, _ = self._handle(dino, depth)
    flat = self.flat_from_tree(params)
    _require_cuda(flat, 'params')
    dev = flat.device
    b, keep = self._marshal(batch, dino, depth, targets=True, discretize=discretize, noise=noise)
    self._chunk_options(h, b.Q)
    res, sc, keep_scale = _alloc_scores(thr, b.B, b.Q, self.num_output_frames, dev, sample_scale, frame_errors)
    outp = None
    if return_predictions:
      res.predictions, out = self._alloc_outputs(b.B, b.Q, dev)
      outp = C.byref(out)
    ws = self._workspace(h, b.B, b.N, b.Q, b.T, False, dev)
    with _counts_on(h, b):
      _lib.check(_lib.load().spa3d_score(h, flat.data_ptr(), C.byref(b), C.byref(sc), outp, ws.data_ptr(), ws.numel(), _stream(flat)),
                 h, 'spa3d_score')
    return res

  def score_all(self, variables, batch, folds=8, thresholds=(), sample_scale=None, frame_errors: bool = False, return_predictions: bool = False,
                discretize: bool = True, noise=None) -> TrackScores:
    """Scores for EVERY track of every clip in one call (spa3d_score_folds): the tracks of each of `folds` contiguous folds are reconstructed from
    the clip's other tracks, and the result has [B, N, ..] shapes -- row n is track n.  The track encoder runs once per clip, not once per fold.
    folds: an int (fold_offsets(N, folds): near-equal sizes) or an offsets array [F + 1] from 0 to N, strictly increasing, 2 <= F <= 64; the same
    for every clip.  Contiguous folds are random folds when the tracks were shuffled beforehand.
    batch: the support keys (support_tracks [B,N,T,3], support_tracks_visible, boundary_frame, dino_features / depth_features as the parameters
    want) and either `query_frame` [B,N] ints -- track n is queried at its position in that frame -- or `query_points` [B,N,4].  The targets are
    `query_tracks` / `query_tracks_visible` when the batch carries them as [B,N,..]; otherwise (absent, or the [B,1,..] placeholders of a
    build_batch without queries) the support tensors themselves, which needs T == num_output_frames.  Everything is validated on the host
    (ValueError) before any device work.  Other arguments as `score`.

    One clip, every track coloured by its own reconstruction error:
      perm = np.random.permutation(n)                                                     # random folds = contiguous folds of a shuffled clip
      batch = spa3d.build_batch([clip], model, num_support_tracks=n, num_query_points=0, splits=[(perm, [], [])])
      batch['query_frame'] = torch.zeros(1, n, dtype=torch.int32, device='cuda')          # every track queried at frame 0
      sc = model.score_all(variables, batch, folds=8, frame_errors=True)
      err = torch.empty_like(sc.frame_err[0]); err[torch.as_tensor(perm, device=err.device)] = sc.frame_err[0]   # back to the clip's own track order
      spa3d.save_scores_npz('scores.npz', clip['tracks_3d'], err, clip['visible'], video=video, intrinsics=K, extrinsics=E)
      frames = spa3d.visualize_npz('scores.npz')                                          # RGB uint8 [T, H, W, 3]"""
    thr = _check_thresholds(thresholds)
    if self._kind == 1:
      raise ValueError('score_all is not available for the 2-D model')
    if self.decoder_scan_chunk_size is not None or self.track_chunk_size is not None:
      raise ValueError('score_all cannot be combined with decoder_scan_chunk_size / track_chunk_size')
    for key in ('support_tracks', 'support_tracks_visible', 'boundary_frame'):
      if batch.get(key) is None:
        raise ValueError(f'score_all needs support_tracks, support_tracks_visible and boundary_frame (no {key!r})')
    st = batch['support_tracks']
    if not isinstance(st, torch.Tensor) or st.dim() != 4 or st.shape[-1] != 3:
      raise ValueError(f'support_tracks must be a [B,N,T,3] tensor, got {tuple(getattr(st, "shape", ()))}')
    B, N, T = (int(v) for v in st.shape[:3])
    To = self.num_output_frames
    off = _fold_offsets_of(folds, N)
    F = len(off) - 1
    cn = validate_counts(batch.get('support_count'), B, N, 'support_count', 1)
    if cn is not None and any(c != N for c in cn):
      raise ValueError('score_all does not take ragged batches: every support_count must equal N')
    qf, qp = batch.get('query_frame'), batch.get('query_points')
    if qf is not None:
      qf = torch.as_tensor(qf)
      if tuple(qf.shape) != (B, N) or qf.dtype.is_floating_point or qf.dtype == torch.bool:
        raise ValueError(f'query_frame must be [B,N] = {(B, N)} ints, got {tuple(qf.shape)} {qf.dtype}')
      if qf.numel() and (int(qf.min()) < 0 or int(qf.max()) >= T):
        raise ValueError(f'query_frame has entries outside [0, T = {T})')
    elif qp is None or not isinstance(qp, torch.Tensor) or tuple(qp.shape) != (B, N, 4):
      raise ValueError(f'score_all needs query_frame [B,N] or query_points [B,N,4] = {(B, N, 4)}; got query_points {tuple(getattr(qp, "shape", ()))}')
    qt, qv = batch.get('query_tracks'), batch.get('query_tracks_visible')
    explicit = qt is not None and qv is not None and int(qt.shape[1]) == N
    if qt is not None and not explicit and int(qt.shape[1]) != 1:
      raise ValueError(f'query_tracks must be [B,N,T,3] targets (or absent), got {tuple(qt.shape)}')
    if explicit and (tuple(qt.shape) != (B, N, To, 3) or tuple(qv.shape[:3]) != (B, N, To)):
      raise ValueError(f'query_tracks must be {(B, N, To, 3)} and query_tracks_visible {(B, N, To, 1)}')
    if not explicit and T != To:
      raise ValueError(f'targets that default to the support tensors need T == num_output_frames, got T = {T}, num_output_frames = {To}')
    # ---- device work from here on
    params = variables['params'] if 'params' in variables and isinstance(variables['params'], dict) else variables
    dino, depth = self._dims_from_params(params)
    h, _, _ = self._handle(dino, depth)
    flat = self.flat_from_tree(params)
    _require_cuda(flat, 'params')
    dev = flat.device
    if qf is not None:  # the query point of track n: (frame, its position in that frame)
      _require_cuda(st, 'support_tracks')
      idx = qf.to(device=st.device, dtype=torch.int64)
      pos = torch.gather(st.to(torch.float32), 2, idx[:, :, None, None].expand(B, N, 1, 3))[:, :, 0]
      qp = torch.cat([idx[..., None].to(torch.float32), pos], dim=-1)
    inputs = {k: v for k, v in batch.items() if k not in ('support_count', 'query_count', 'query_points')}
    lib = _lib.load()
    if noise is None and discretize:  # the library's own draw, made here: the workspace need then does not depend on B
      noise = torch.empty(B, self.num_latent_tokens, self.latent_token_dim, dtype=torch.float32, device=dev)
      _lib.check(lib.spa3d_uniform_noise(noise.data_ptr(), noise.numel(), 0, 0, _stream(flat)), what='spa3d_uniform_noise')
    b, keep = self._marshal(inputs, dino, depth, discretize=discretize, noise=noise, query_points=qp)
    if explicit:
      qt, qv = self._f32(qt, 'query_tracks'), self._f32(qv, 'query_tracks_visible')
      keep += [qt, qv]
      b.query_tracks, b.query_tracks_visible = qt.data_ptr(), qv.data_ptr()
    self._chunk_options(h, None)
    res, sc, keep_scale = _alloc_scores(thr, B, N, To, dev, sample_scale, frame_errors)
    outp = None
    if return_predictions:
      res.predictions, out = self._alloc_outputs(B, N, dev)
      outp = C.byref(out)
    # workspace: at least what the call needs with the readout one fold at a time; up to one sample's forward more lets it take every fold at once
    floor = lib.spa3d_score_folds_workspace_bytes(h, N, T, F)
    if floor < 0:
      raise _lib.Spa3dError(f'spa3d_score_folds_workspace_bytes refused N = {N}, T = {T}, folds = {F}')
    want = floor + lib.spa3d_workspace_bytes(h, 1, N, N, T, 1, 0)
    have = self._ws.numel() if (self._ws is not None and self._ws.device == torch.device(dev)) else 0
    if have < want and not (self._ws_cap > 0 and have >= max(floor, self._ws_cap)):
      free, _total = torch.cuda.mem_get_info(dev)
      size = min(want, max(int((free + have) * self.workspace_fraction), floor))
      if size > have:
        self._ws = None
        torch.cuda.empty_cache()
        self._ws = torch.empty(size, dtype=torch.uint8, device=dev)
        self._ws_cap = size if size < want else 0
    ws = self._ws
    offs = (C.c_int32 * (F + 1))(*[int(v) for v in off])
    _lib.check(lib.spa3d_score_folds(h, flat.data_ptr(), C.byref(b), F, offs, C.byref(sc), outp, ws.data_ptr(), ws.numel(), _stream(flat)),
               h, 'spa3d_score_folds')
    return res

  def score_video(self, variables, clip, stride=None, folds=8, blend='hat', thresholds=(), perm=None, noise=None, windows_per_call=None,
                  return_predictions: bool = True, discretize: bool = True) -> 'VideoScores':
    """Scores for every track of a clip of ANY length.  The model is tied to num_output_frames frames, so the clip (the dict build_batch takes,
    with any number of frames TL) is cut into overlapping windows of that length (window_starts(TL, num_output_frames, stride), built in place
    by build_windows), every window goes through score_all, and the per-window predictions and errors are merged back onto the clip's own time
    axis by stitch_windows with the `blend` ('hat' | 'mean' | 'first') that include/spa3d.h defines.
      perm: the shuffle of the clip's n tracks that makes the contiguous folds random folds (np.random.permutation(n) when None); the same for
        every window.  Track perm[r] is row r of every window; the results are back in the clip's own track order.
      query frames: row r of window w is queried at the first frame of the window in which it is visible, frame 0 of the window if in none.
      noise: [W, num_latent_tokens, latent_token_dim], one draw per window; None draws it here, once for all windows.
      windows_per_call: at most this many windows per build_windows / score_all call (default: all).  score_all processes clips one at a
        time, so the grouping changes memory, not results.
    The targets are the windows' own support tracks carried onto the long axis by a 'first' stitch; `scores` is score_predictions of the
    stitched predictions against them, over all TL frames.  Forward only; the 3-D model; no ragged counts; no intra-sample chunk options.

      vs = model.score_video(variables, clip, stride=75)                         # clip: 4096 tracks x 600 frames, say
      spa3d.save_scores_npz('scores.npz', vs.targets_tracks, vs.frame_err, vs.targets_visible, video=video, intrinsics=K, extrinsics=E)
      frames = spa3d.render_tracks(video, vs.targets_tracks, vs.frame_err, vs.targets_visible, intrinsics=K, extrinsics=E)
      unsure = vs.spread > 0.1                                                   # the windows disagree about the point: model uncertainty"""
    import numpy as np
    from .data import BLENDS, MAX_WINDOWS, _clip_sources, build_windows, stitch_windows, window_starts
    thr = _check_thresholds(thresholds)
    if self._kind == 1:
      raise ValueError('score_video is not available for the 2-D model')
    if self.decoder_scan_chunk_size is not None or self.track_chunk_size is not None:
      raise ValueError('score_video cannot be combined with decoder_scan_chunk_size / track_chunk_size')
    if not isinstance(clip, dict):
      raise ValueError('score_video takes ONE clip dict')
    if clip.get('support_count') is not None or clip.get('query_count') is not None:
      raise ValueError('score_video does not take ragged counts')
    if blend not in BLENDS:
      raise ValueError(f'blend must be one of {sorted(BLENDS)}, got {blend!r}')
    plan, _, _ = _clip_sources(clip, self, lambda m: ValueError(f'clip: {m}'), None)
    n, TL, Tw = plan['n'], plan['Tc'], int(self.num_output_frames)
    starts = window_starts(TL, Tw, stride)
    W = len(starts)
    if W > MAX_WINDOWS:
      raise ValueError(f'{W} windows: a stitch takes at most {MAX_WINDOWS} (use a larger stride)')
    _fold_offsets_of(folds, n)  # refused here as score_all would
    if perm is None:
      perm = np.random.permutation(n)
    else:
      perm = perm.detach().cpu().numpy() if isinstance(perm, torch.Tensor) else np.asarray(perm)
      if perm.ndim != 1 or perm.dtype.kind not in 'iu' or len(perm) != n or not np.array_equal(np.sort(perm), np.arange(n)):
        raise ValueError(f'perm must be a permutation of range({n})')
    perm = perm.astype(np.int64)
    L, Ld = self.num_latent_tokens, self.latent_token_dim
    if noise is not None and (not isinstance(noise, torch.Tensor) or tuple(noise.shape) != (W, L, Ld)):
      raise ValueError(f'noise must be a [W, num_latent_tokens, latent_token_dim] = {(W, L, Ld)} tensor, got {tuple(getattr(noise, "shape", ()))}')
    if windows_per_call is None:
      windows_per_call = W
    if isinstance(windows_per_call, bool) or not isinstance(windows_per_call, (int, np.integer)) or windows_per_call < 1:
      raise ValueError(f'windows_per_call must be a positive int, got {windows_per_call!r}')
    # ---- device work from here on
    params = variables['params'] if 'params' in variables and isinstance(variables['params'], dict) else variables
    flat = self.flat_from_tree(params)
    _require_cuda(flat, 'params')
    dev = flat.device
    # the clip goes to the device once, whatever the grouping: build_windows takes device tensors of the right type as they are
    types = {'tracks_2d': torch.float32, 'visible': torch.float32, 'tracks_3d': torch.float32, 'depth': torch.float32, 'dino_map': torch.float32,
             'dino_features': self.act_dtype, 'depth_features': self.act_dtype}
    dclip = dict(clip)
    for k, dt in types.items():
      if clip.get(k) is not None:
        t = clip[k] if isinstance(clip[k], torch.Tensor) else torch.as_tensor(np.asarray(clip[k]))
        dclip[k] = t.to(device=dev, dtype=dt).contiguous()
    if noise is None and discretize:  # one draw for all windows: a window's noise does not depend on the grouping
      noise = torch.empty(W, L, Ld, dtype=torch.float32, device=dev)
      _lib.check(_lib.load().spa3d_uniform_noise(noise.data_ptr(), noise.numel(), 0, 0, _stream(flat)), what='spa3d_uniform_noise')
    parts = {k: [] for k in ('tracks', 'visible_logits', 'frame_err', 'support_tracks', 'support_tracks_visible')}
    for g0 in range(0, W, int(windows_per_call)):
      g1 = min(W, g0 + int(windows_per_call))
      batch = build_windows(dclip, self, starts=starts[g0:g1], order=perm, device=dev)
      vis = batch['support_tracks_visible'][..., 0] > 0.5
      batch['query_frame'] = vis.to(torch.int32).argmax(dim=2).to(torch.int32)  # the first visible frame; 0 when there is none
      sc = self.score_all(variables, batch, folds=folds, frame_errors=True, return_predictions=True, discretize=discretize,
                          noise=None if noise is None else noise[g0:g1])
      parts['tracks'].append(sc.predictions.tracks)
      parts['visible_logits'].append(sc.predictions.visible_logits[..., 0])
      parts['frame_err'].append(sc.frame_err)
      parts['support_tracks'].append(batch['support_tracks'])
      parts['support_tracks_visible'].append(batch['support_tracks_visible'][..., 0])
    cat = {k: (v[0] if len(v) == 1 else torch.cat(v, 0)) for k, v in parts.items()}
    out = stitch_windows(starts, TL, tracks=cat['tracks'], visible_logits=cat['visible_logits'], frame_err=cat['frame_err'], blend=blend, row_track=perm, spread=True)
    tgt = stitch_windows(starts, TL, tracks=cat['support_tracks'], visible_logits=cat['support_tracks_visible'], blend='first', row_track=perm)
    zeros = torch.zeros(1, n, TL, 1, dtype=torch.float32, device=dev)
    preds = TrackAutoEncoderResults(out['tracks'][None], out['visible_logits'][None, :, :, None], zeros)
    scores = score_predictions(preds, {'query_tracks': tgt['tracks'][None], 'query_tracks_visible': tgt['visible_logits'][None, :, :, None]}, thresholds=thr)
    return VideoScores(tracks=out['tracks'] if return_predictions else None, visible_logits=out['visible_logits'] if return_predictions else None,
                       frame_err=out['frame_err'], spread=out['spread'], targets_tracks=tgt['tracks'], targets_visible=tgt['visible_logits'], scores=scores,
                       window_start=starts, perm=perm)

  def tapvid3d(self, variables, batch, scalings=('median',), fixed_thresholds: bool = False, ratios: bool = False, discretize: bool = True, noise=None):
    """evaluate_tapvid3d.py:62-115 for one batch: ONE forward pass, then one TAPVid-3D metric call per scaling on that forward's
    predictions (tapvid3d_predictions).  Returns {scaling: TapVid3DScores}.  The batch carries its targets, may carry `intrinsics` [B, 4]
    (default (256, 256, 128, 128)) and, for a ragged batch, its counts (split_ragged cuts a TapVid3DScores per clip)."""
    scalings = tuple(_check_scaling(s) for s in scalings)
    preds = self(variables, batch, discretize=discretize, noise=noise)
    return {s: tapvid3d_predictions(preds, batch, scaling=s, intrinsics=batch.get('intrinsics'), fixed_thresholds=fixed_thresholds, ratios=ratios) for s in scalings}

  def apply(self, variables, *args, rngs=None, method=None, **kw):
    """Flax-style apply: model.apply({'params': p}, batch[, rngs=...][, method=model.encode])."""
    if method is None:
      return self(variables, *args, **kw)
    fn = getattr(self, method) if isinstance(method, str) else method
    name = getattr(fn, '__name__', '')
    if name == 'get_decoder_context':
      return self.get_decoder_context(*args, **kw)
    return fn(variables, *args, **kw)

  # -------------------------------------------------------------------------------- value_and_grad
  def loss_and_grads(self, variables, batch, grads_flat: Optional[torch.Tensor] = None, accumulate: bool = False,
                     denom: float = 0.0, discretize: bool = True, noise=None, return_predictions: bool = False, loss: Optional[LossConfig] = None,
                     freeze=0):
    """jax.value_and_grad(loss_fn)(params) of train.py:134-162 in one call.  Returns (loss_dict, grads_tree, preds|None).
    `freeze`: 0 | 1 ('encoder') | 2 ('encoder+latents') -- the backward stops at that stage boundary (spa3d_set_option "freeze"): the gradients of the
    frozen prefix [0, lo) of the flat buffer are zero (accumulate: left as they were), the rest and every forward result are those of freeze = 0.
    `denom`: the batch-GLOBAL sum(query_tracks_visible) under data parallelism (train.py:111-113).
    `loss`: the objective (LossConfig; None = the reference's); batch['query_weight'] ([B,Q,T] or [B,Q,T,1], in [0, 1]) weights single points."""
    params = variables['params'] if 'params' in variables and isinstance(variables['params'], dict) else variables
    dino, depth = self._dims_from_params(params)
    h, _, n = self._handle(dino, depth)
    flat = self.flat_from_tree(params)
    dev = flat.device
    b, keep = self._marshal(batch, dino, depth, targets=True, discretize=discretize, noise=noise)
    self._chunk_options(h, b.Q)
    if grads_flat is None:
      grads_flat = torch.empty(n, dtype=torch.float32, device=dev)
      accumulate = False
    loss3 = torch.empty(4, dtype=torch.float32, device=dev)
    res, out, outp = None, None, None
    if return_predictions:
      res, out = self._alloc_outputs(b.B, b.Q, dev)
      outp = C.byref(out)
    with _freeze_on(h, freeze), _counts_on(h, b), _loss_on(h, loss, b.weights, b.B, b.Q, self._nc):
      ws = self._workspace(h, b.B, b.N, b.Q, b.T, True, dev)
      _lib.check(_lib.load().spa3d_loss_and_grads(h, flat.data_ptr(), C.byref(b), float(denom), grads_flat.data_ptr(),
                                                  1 if accumulate else 0, loss3.data_ptr(), outp, ws.data_ptr(), ws.numel(),
                                                  _stream(flat)), h, 'spa3d_loss_and_grads')
    ld = {'total_loss': loss3[0], 'position_loss': loss3[1], 'visible_loss': loss3[2]}
    return ld, self.tree_from_flat(grads_flat, dino, depth), res


def compute_loss_3d(predictions: TrackAutoEncoderResults, targets, l1_weight: float = 5000.0, bce_weight: float = 1e-8,
                    denom: float = 0.0, loss: Optional[LossConfig] = None):
  """train.py:96-129 on the GPU kernels.  Needs any model handle only for its output-frame count.
  targets['query_weight'], when present, weights single points.  With `loss` (a LossConfig) the three numbers are what loss_and_grads reports
  under that objective for these predictions (l1_weight / bce_weight are then the configuration's, not the arguments)."""
  lib = _lib.load()
  tr = predictions.tracks
  _require_cuda(tr, 'predictions.tracks')
  B, Q, To = tr.shape[:3]
  h = _loss_handle(To, 1 if tr.shape[-1] == 2 else 0)
  b = _lib.Batch()
  b.B, b.Q = B, Q
  qt = targets['query_tracks'].to(torch.float32).contiguous()
  qv = targets['query_tracks_visible'].to(torch.float32).contiguous()
  if tuple(qt.shape) != tuple(tr.shape):
    raise ValueError(f'query_tracks {tuple(qt.shape)} does not match predictions {tuple(tr.shape)}')
  b.query_tracks, b.query_tracks_visible = qt.data_ptr(), qv.data_ptr()
  t32 = tr.to(torch.float32).contiguous()
  vl = predictions.visible_logits.to(torch.float32).contiguous()
  out = _lib.Outputs(t32.data_ptr(), vl.data_ptr(), None, None)
  b.counts = (None, validate_counts(targets.get('query_count'), B, Q, 'query_count', 0))  # ragged batch: live queries only
  qw = _point_weights(targets.get('query_weight'), B, Q, To)
  loss3 = torch.empty(12, dtype=torch.float32, device=tr.device)
  with _counts_on(h, b), _loss_on(h, loss, qw, B, Q, tr.shape[-1]):
    _lib.check(lib.spa3d_loss(h, C.byref(b), C.byref(out), float(denom), loss3.data_ptr(), _stream(tr)), h, 'spa3d_loss')
  pos, vis = loss3[1], loss3[2]
  if loss is not None:
    return {'total_loss': loss3[0], 'position_loss': pos, 'visible_loss': vis}
  return {'total_loss': l1_weight * pos + bce_weight * vis, 'position_loss': pos, 'visible_loss': vis}


def score_predictions(predictions: TrackAutoEncoderResults, targets, thresholds=(), sample_scale=None, frame_errors: bool = False) -> TrackScores:
  """The scores of TrackAutoEncoder3D.score from predictions that already exist (spa3d_score_from_preds): on the predictions a score call
  returned it gives that call's bits.  targets: query_tracks, query_tracks_visible and, for a ragged batch, query_count."""
  thr = _check_thresholds(thresholds)
  lib = _lib.load()
  tr = predictions.tracks
  _require_cuda(tr, 'predictions.tracks')
  B, Q, To = tr.shape[:3]
  h = _loss_handle(To, 1 if tr.shape[-1] == 2 else 0)
  b = _lib.Batch()
  b.B, b.Q = B, Q
  qt = targets['query_tracks'].to(torch.float32).contiguous()
  qv = targets['query_tracks_visible'].to(torch.float32).contiguous()
  _require_cuda(qt, 'query_tracks')
  _require_cuda(qv, 'query_tracks_visible')
  if tuple(qt.shape) != tuple(tr.shape):
    raise ValueError(f'query_tracks {tuple(qt.shape)} does not match predictions {tuple(tr.shape)}')
  b.query_tracks, b.query_tracks_visible = qt.data_ptr(), qv.data_ptr()
  t32 = tr.to(torch.float32).contiguous()
  vl = predictions.visible_logits.to(torch.float32).contiguous()
  out = _lib.Outputs(t32.data_ptr(), vl.data_ptr(), None, None)
  res, sc, keep_scale = _alloc_scores(thr, B, Q, To, tr.device, sample_scale, frame_errors)
  b.counts = (None, validate_counts(targets.get('query_count'), B, Q, 'query_count', 0))  # ragged batch: live queries only
  with _counts_on(h, b):
    _lib.check(lib.spa3d_score_from_preds(h, C.byref(b), C.byref(out), C.byref(sc), _stream(tr)), h, 'spa3d_score_from_preds')
  return res


def tapvid3d_predictions(predictions: TrackAutoEncoderResults, batch, scaling: str = 'median', intrinsics=None, fixed_thresholds: bool = False,
                         ratios: bool = False) -> TapVid3DScores:
  """TAPVid-3D metric counts of existing predictions (spa3d_tapvid3d_from_preds): the counterpart of
  tapvid3d_metrics.compute_tapvid3d_metrics(..., scaling=scaling) in evaluate_tapvid3d.py:99-109, for every clip of the batch at once and
  without a host copy.  batch: query_points, query_tracks, query_tracks_visible and, for a ragged batch, query_count.  intrinsics: [B, 4]
  or [4] (fx, fy, cx, cy), default (256, 256, 128, 128).  Restated from the published definition; parity with tapnet is unpinned."""
  _check_scaling(scaling)
  lib = _lib.load()
  tr = predictions.tracks
  _require_cuda(tr, 'predictions.tracks')
  if tr.dim() != 4 or tr.shape[-1] != 3:
    raise ValueError(f'TAPVid-3D metrics need 3-D tracks [B, Q, T, 3], got {tuple(tr.shape)}')
  B, Q, To = tr.shape[:3]
  dev = tr.device
  h = _loss_handle(To, 0)
  b = _lib.Batch()
  b.B, b.Q = B, Q
  qt = batch['query_tracks'].to(torch.float32).contiguous()
  qv = batch['query_tracks_visible'].to(torch.float32).contiguous()
  qp = batch['query_points'].to(torch.float32).contiguous()
  for t, name in ((qt, 'query_tracks'), (qv, 'query_tracks_visible'), (qp, 'query_points')):
    _require_cuda(t, name)
  if tuple(qt.shape) != tuple(tr.shape):
    raise ValueError(f'query_tracks {tuple(qt.shape)} does not match predictions {tuple(tr.shape)}')
  if qv.numel() != B * Q * To:
    raise ValueError(f'query_tracks_visible {tuple(qv.shape)} does not match predictions {tuple(tr.shape)}')
  if tuple(qp.shape) != (B, Q, 4):
    raise ValueError(f'query_points must be [B, Q, 4] (t, x, y, z), got {tuple(qp.shape)}')
  b.query_tracks, b.query_tracks_visible, b.query_points = qt.data_ptr(), qv.data_ptr(), qp.data_ptr()
  t32 = tr.to(torch.float32).contiguous()
  vl = predictions.visible_logits.to(torch.float32).contiguous()
  out = _lib.Outputs(t32.data_ptr(), vl.data_ptr(), None, None)
  res = TapVid3DScores(torch.empty(B, Q, TAPVID3D_SLOTS, dtype=torch.float32, device=dev), torch.empty(B, TAPVID3D_SLOTS, dtype=torch.float64, device=dev),
                       torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, Q, dtype=torch.float32, device=dev),
                       torch.empty(B, Q, To, dtype=torch.float32, device=dev) if ratios else None, scaling, bool(fixed_thresholds))
  m = _lib.TapVid3D()
  m.scaling, m.fixed_thresholds = TAPVID3D_SCALINGS[scaling], 1 if fixed_thresholds else 0
  k = None
  if intrinsics is not None:
    k = intrinsics if isinstance(intrinsics, torch.Tensor) else torch.as_tensor(intrinsics, dtype=torch.float32)
    k = k.to(device=dev, dtype=torch.float32)
    if k.dim() == 1:
      k = k.expand(B, -1)
    if tuple(k.shape) != (B, 4):
      raise ValueError(f'intrinsics must be [B, 4] or [4] (fx, fy, cx, cy), got {tuple(k.shape)}')
    k = k.contiguous()
    m.intrinsics = k.data_ptr()
  m.query_stats, m.sample_stats, m.scale, m.row_scale = res.query_stats.data_ptr(), res.sample_stats.data_ptr(), res.scale.data_ptr(), res.row_scale.data_ptr()
  m.ratio = res.ratio.data_ptr() if ratios else None
  ws = torch.empty(max(int(lib.spa3d_tapvid3d_workspace_bytes(h, B, Q, To)), 256), dtype=torch.uint8, device=dev)
  b.counts = (None, validate_counts(batch.get('query_count'), B, Q, 'query_count', 0))  # ragged batch: live queries only
  with _counts_on(h, b):
    _lib.check(lib.spa3d_tapvid3d_from_preds(h, C.byref(b), C.byref(out), C.byref(m), ws.data_ptr(), ws.numel(), _stream(tr)), h, 'spa3d_tapvid3d_from_preds')
  return res


def aggregate_tapvid3d(per_clip):
  """evaluate_tapvid3d.py:233-243: per_clip = a list of metric dicts (one per video); returns {key: mean, key_std: population std}."""
  out = {}
  if not per_clip:
    return out
  for key in per_clip[0]:
    vals = [float(c[key]) for c in per_clip]
    mean = sum(vals) / len(vals)
    out[key] = mean
    out[f'{key}_std'] = math.sqrt(sum((v - mean) ** 2 for v in vals) / len(vals))
  return out


def evaluate_tapvid3d(model, variables, batches, depth_scalings=('median',), fixed_thresholds: bool = False):
  """Counterpart of evaluate_model (evaluate_tapvid3d.py:144-244): every batch through model.tapvid3d (one forward, one metric call per
  scaling), every clip of every batch one video; returns {scaling: {key: mean over videos, key_std: std over videos}} with the reference's
  13 keys.  Batches may be ragged (collate_ragged) and may carry `intrinsics`."""
  depth_scalings = tuple(_check_scaling(s) for s in depth_scalings)
  per_clip = {s: [] for s in depth_scalings}
  for batch in batches:
    scores = model.tapvid3d(variables, batch, scalings=depth_scalings, fixed_thresholds=fixed_thresholds)
    for s in depth_scalings:
      per_clip[s] += [scores[s].as_dict(i) for i in range(scores[s].sample_stats.shape[0])]
  return {s: aggregate_tapvid3d(per_clip[s]) for s in depth_scalings}


# ------------------------------------------------------------------------------------------------
# track overlays (spa3d_render_tracks)
# ------------------------------------------------------------------------------------------------
def _video_u8(video: torch.Tensor) -> torch.Tensor:
  """uint8 [T, H, W, 3] as it is; a float [T, 3, H, W] in [0, 1] as prepare_video_for_visualization (visualize.py:219-240) converts it: clip,
  x 255, truncate."""
  if video.dtype == torch.uint8:
    if video.dim() != 4 or video.shape[-1] != 3:
      raise ValueError(f'a uint8 video must be [T, H, W, 3], got {tuple(video.shape)}')
    return video
  if not video.is_floating_point() or video.dim() != 4 or video.shape[1] != 3:
    raise ValueError(f'video must be uint8 [T, H, W, 3] or float [T, 3, H, W], got {video.dtype} {tuple(video.shape)}')
  return (video.permute(0, 2, 3, 1).clamp(0, 1) * 255).to(torch.uint8).contiguous()


def _camera(m, T, rows, name, dev):
  m = m if isinstance(m, torch.Tensor) else torch.as_tensor(m, dtype=torch.float64)
  m = m.to(device=dev, dtype=torch.float64)
  if m.dim() == 2:
    m = m.unsqueeze(0).expand(T, -1, -1)  # tiled over T, as project_all_tracks does
  if tuple(m.shape) != (T, rows, rows):
    raise ValueError(f'{name} must be [{rows}, {rows}] or [T, {rows}, {rows}], got {tuple(m.shape)}')
  return m.contiguous()


def _plane(t, N, T, name):
  t = t if isinstance(t, torch.Tensor) else torch.as_tensor(t)
  _require_cuda(t, name)
  if t.dim() == 3 and t.shape[-1] == 1:
    t = t[..., 0]
  if tuple(t.shape) != (N, T):
    raise ValueError(f'{name} must be [N, T] or [N, T, 1] = [{N}, {T}], got {tuple(t.shape)}')
  return t.to(torch.float32).contiguous()


def _render_call(r, tracks, intrinsics, extrinsics, resize, entry='spa3d_render_tracks', sizer='spa3d_render_workspace_bytes'):
  """Fills the coordinate fields of a _lib.Render (or a _lib.Heatmap: the same names), sizes the workspace and calls `entry` on tracks' stream.
  The converted tensors and the workspace live until the call is enqueued; the caching allocator orders any reuse of their memory after it on
  that stream."""
  lib = _lib.load()
  N, T, nc = tracks.shape
  dev = tracks.device
  r.N, r.T, r.coords = N, T, nc
  r.tracks = tracks.data_ptr()
  if nc == 3:
    if intrinsics is None or extrinsics is None:
      raise ValueError('3-D tracks need intrinsics and extrinsics')
    k, e = _camera(intrinsics, T, 3, 'intrinsics', dev), _camera(extrinsics, T, 4, 'extrinsics', dev)
    r.intrinsics, r.extrinsics = k.data_ptr(), e.data_ptr()
    r.resize_h, r.resize_w = int(resize[0]), int(resize[1])
  h = _render_handle()
  ws = torch.empty(max(int(getattr(lib, sizer)(h, N, T)), 256), dtype=torch.uint8, device=dev)
  _lib.check(getattr(lib, entry)(h, C.byref(r), ws.data_ptr(), ws.numel(), _stream(tracks)), h, entry)


_RENDER_HANDLE = []


def _render_handle():
  """A handle of the render calls' own: spa3d_render_tracks uses its handle for the error message, the stream and the workspace arena only, and
  must not reset those of a handle a model or the loss functions are using."""
  if not _RENDER_HANDLE:
    _RENDER_HANDLE.append(TrackAutoEncoder3D(num_output_frames=8, use_dino=False, use_depth=False, precision='fp32'))  # the model owns its handles
  return _RENDER_HANDLE[0]._handle(0, 0)[0]


def _tracks_f32(tracks):
  _require_cuda(tracks, 'tracks')
  if tracks.dim() != 3 or tracks.shape[-1] not in (2, 3):
    raise ValueError(f'tracks must be [N, T, 3] points or [N, T, 2] pixel coordinates, got {tuple(tracks.shape)}')
  return tracks.to(torch.float32).contiguous()


def render_tracks(video, tracks, scores, visibs=None, intrinsics=None, extrinsics=None, trail: int = 5, point_size: int = 2, normalize: bool = True,
                  resize=(1024, 1024), use_visibility: bool = False, colour_bgr: bool = False, out=None, return_pixels: bool = False):
  """Score-coloured dots and trails drawn into a clip's frames on the GPU (spa3d_render_tracks): the counterpart of project_all_tracks +
  normalize_scores + paint_point_track_with_colors (visualize.py:76-175, visualizer.py:23-45).  One clip, track-major: tracks [N, T, 3] with
  intrinsics [3, 3] / [T, 3, 3] and extrinsics [4, 4] / [T, 4, 4], or [N, T, 2] pixel coordinates; scores, visibs [N, T] or [N, T, 1]; video
  uint8 [T, H, W, 3] or float [T, 3, H, W] in [0, 1].  Returns uint8 [T, H, W, 3] (`out`, which may be the video itself, when given), and with
  return_pixels also the int32 [N, T, 2] positions used.  The rasteriser is the library's own integer one (include/spa3d.h), not cv2's."""
  _require_cuda(video, 'video')
  vid = _video_u8(video).contiguous()
  trk = _tracks_f32(tracks)
  N, T = trk.shape[:2]
  if vid.shape[0] != T:
    raise ValueError(f'video has {vid.shape[0]} frames, tracks have {T}')
  if out is None:
    out = torch.empty_like(vid)
  _require_cuda(out, 'out')
  if out.dtype != torch.uint8 or tuple(out.shape) != tuple(vid.shape) or not out.is_contiguous():
    raise ValueError(f'out must be a contiguous uint8 {tuple(vid.shape)} tensor')
  r = _lib.Render()
  r.H, r.W = vid.shape[1], vid.shape[2]
  r.video, r.out = vid.data_ptr(), out.data_ptr()
  sc = _plane(scores, N, T, 'scores')
  r.scores = sc.data_ptr()
  if visibs is not None:
    vs = _plane(visibs, N, T, 'visibs')
    r.visible = vs.data_ptr()
  elif use_visibility:
    raise ValueError('use_visibility needs visibs')
  r.normalize, r.use_visibility, r.colour_bgr, r.trail, r.point_size = int(bool(normalize)), int(bool(use_visibility)), int(bool(colour_bgr)), int(trail), int(point_size)
  pixels = torch.empty(N, T, 2, dtype=torch.int32, device=trk.device) if return_pixels else None
  r.pixels = pixels.data_ptr() if return_pixels else None
  _render_call(r, trk, intrinsics, extrinsics, resize)
  return (out, pixels) if return_pixels else out


def project_tracks(tracks_3d, intrinsics, extrinsics, H: int, W: int, resize=(1024, 1024)):
  """project_all_tracks (visualize.py:125-175) followed by the painter's int(): int32 [N, T, 2] pixel positions (x, y) of [N, T, 3] points,
  clipped to the image.  The same call as render_tracks with only the positions requested."""
  trk = _tracks_f32(tracks_3d)
  if trk.shape[-1] != 3:
    raise ValueError(f'tracks_3d must be [N, T, 3], got {tuple(trk.shape)}')
  r = _lib.Render()
  r.H, r.W = int(H), int(W)
  pixels = torch.empty(trk.shape[0], trk.shape[1], 2, dtype=torch.int32, device=trk.device)
  r.pixels = pixels.data_ptr()
  _render_call(r, trk, intrinsics, extrinsics, resize)
  return pixels


def render_heatmap(tracks, values, H: Optional[int] = None, W: Optional[int] = None, video=None, visibs=None, intrinsics=None, extrinsics=None, radius: int = 12,
                   power: int = 2, normalize: bool = True, value_range=None, alpha: float = 0.5, use_visibility: bool = False, colour_bgr: bool = False,
                   resize=(1024, 1024), out=None, return_weight: bool = False):
  """Dense per-frame maps of track values on the GPU (spa3d_render_heatmap; the library's own definition, include/spa3d.h): per pixel the
  average of the values of the tracks within `radius` of it, weighted by q = radius^2 + 1 - d^2 (power 1) or q^2 (power 2), NaN where no track is
  near.  One clip, track-major, the inputs of render_tracks: tracks [N, T, 3] with intrinsics / extrinsics, or [N, T, 2] pixel coordinates;
  values, visibs [N, T] or [N, T, 1].  Returns the float32 [T, H, W] map; with a video (uint8 [T, H, W, 3] or float [T, 3, H, W], which also
  gives H and W) also the uint8 overlay (`out`, which may be the video itself, when given); with return_weight also the float32 [T, H, W] sum of
  weights.  The overlay colours s = (map - lo) / (hi - lo) as render_tracks colours a score and blends it with weight alpha in [0, 1] (a
  multiple of 1 / 4096): (lo, hi) is value_range when given, else the min and max of the finite values (normalize) or (0, 1)."""
  a = float(alpha) * 4096
  if not (0 <= a <= 4096) or a != int(a):
    raise ValueError(f'alpha = {alpha} must be a multiple of 1 / 4096 in [0, 1]')
  if video is None and out is not None:
    raise ValueError('out needs video')
  if video is None and (H is None or W is None):
    raise ValueError('without a video H and W are required')
  if use_visibility and visibs is None:
    raise ValueError('use_visibility needs visibs')
  if value_range is not None and len(value_range) != 2:
    raise ValueError('value_range must be (lo, hi)')
  trk = _tracks_f32(tracks)
  N, T = trk.shape[:2]
  dev = trk.device
  m = _lib.Heatmap()
  if video is not None:
    _require_cuda(video, 'video')
    vid = _video_u8(video).contiguous()
    if vid.shape[0] != T:
      raise ValueError(f'video has {vid.shape[0]} frames, tracks have {T}')
    if (H is not None and int(H) != vid.shape[1]) or (W is not None and int(W) != vid.shape[2]):
      raise ValueError(f'H, W = {H}, {W} disagree with the video ({vid.shape[1]}, {vid.shape[2]})')
    H, W = vid.shape[1], vid.shape[2]
    if out is None:
      out = torch.empty_like(vid)
    _require_cuda(out, 'out')
    if out.dtype != torch.uint8 or tuple(out.shape) != tuple(vid.shape) or not out.is_contiguous():
      raise ValueError(f'out must be a contiguous uint8 {tuple(vid.shape)} tensor')
    m.video, m.out = vid.data_ptr(), out.data_ptr()
  m.H, m.W = int(H), int(W)
  val = _plane(values, N, T, 'values')
  m.values = val.data_ptr()
  if visibs is not None:
    vs = _plane(visibs, N, T, 'visibs')
    m.visible = vs.data_ptr()
  m.use_visibility, m.radius, m.power, m.alpha, m.colour_bgr = int(bool(use_visibility)), int(radius), int(power), int(a), int(bool(colour_bgr))
  if value_range is not None:
    m.normalize, m.lo, m.hi = 0, float(value_range[0]), float(value_range[1])
  else:
    m.normalize, m.lo, m.hi = int(bool(normalize)), 0.0, 1.0
  if m.H < 1 or m.W < 1:
    raise ValueError(f'H, W = {m.H}, {m.W} must be positive')
  hmap = torch.empty(T, m.H, m.W, dtype=torch.float32, device=dev)
  m.map = hmap.data_ptr()
  weight = torch.empty(T, m.H, m.W, dtype=torch.float32, device=dev) if return_weight else None
  m.weight = weight.data_ptr() if return_weight else None
  _render_call(m, trk, intrinsics, extrinsics, resize, 'spa3d_render_heatmap', 'spa3d_heatmap_workspace_bytes')
  res = (hmap,) + ((out,) if video is not None else ()) + ((weight,) if return_weight else ())
  return res if len(res) > 1 else hmap


def visualize_npz(path: str, device='cuda', mode: str = 'tracks', **options):
  """Counterpart of visualizer.py's main (:149-203) up to the painted frames: reads the TIME-major file data.save_scores_npz writes (coords
  [T, N, 3], coords_score [T, N] or [T, N, 1], video [T, 3, H, W] float or [T, H, W, 3] uint8, intrinsics, extrinsics, optional visibs),
  transposes to track-major, renders on `device` and returns RGB uint8 [T, H, W, 3].  mode 'tracks': dots and trails, options those of
  render_tracks; mode 'heatmap': the overlay of render_heatmap, options those of render_heatmap.  Encoding a video file is the caller's job."""
  if mode not in ('tracks', 'heatmap'):
    raise ValueError(f"mode must be 'tracks' or 'heatmap', got {mode!r}")
  import numpy as np
  d = np.load(path)
  coords, score = np.asarray(d['coords']), np.asarray(d['coords_score'])
  if score.ndim == 3:
    score = score[..., 0]
  to = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(device)
  visibs = None
  if 'visibs' in d.files:
    v = np.asarray(d['visibs'])
    visibs = to((v[..., 0] if v.ndim == 3 else v).T.astype(np.float32))
  cam = {}
  if coords.shape[-1] == 3:
    cam = dict(intrinsics=to(d['intrinsics'], torch.float64), extrinsics=to(d['extrinsics'], torch.float64))
  trk, sc = to(coords.transpose(1, 0, 2), torch.float32), to(score.T, torch.float32)
  if mode == 'heatmap':
    return render_heatmap(trk, sc, video=to(d['video']), visibs=visibs, **cam, **options)[1]
  return render_tracks(to(d['video']), trk, sc, visibs, **cam, **options)


_LOSS_HANDLES: Dict[Any, Any] = {}


def _loss_handle(num_output_frames, kind=0):
  if (num_output_frames, kind) not in _LOSS_HANDLES:
    cls = TrackAutoEncoder if kind else TrackAutoEncoder3D
    m = cls(num_output_frames=num_output_frames, precision='fp32') if kind else cls(num_output_frames=num_output_frames, use_dino=False,
                                                                                    use_depth=False, precision='fp32')
    _LOSS_HANDLES[(num_output_frames, kind)] = m._handle(0, 0)[0]
  return _LOSS_HANDLES[(num_output_frames, kind)]


def compute_loss_2d(predictions: TrackAutoEncoderResults, targets, l1_weight: float = 5000.0, bce_weight: float = 1e-8, denom: float = 0.0,
                    loss: Optional[LossConfig] = None):
  """train.py:60-93 (same arithmetic as compute_loss_3d on 2 coordinates)."""
  return compute_loss_3d(predictions, targets, l1_weight, bce_weight, denom, loss)


class TrackAutoEncoder(TrackAutoEncoder3D):
  """Drop-in for the 2-D TRAJAN twin track_autoencoder.TrackAutoEncoder (track_autoencoder.py:117-390): (x,y) tracks,
  no readout token (frame tokens are mean-pooled over visible frames, :230-232), a real certainty head (:344), no DINO /
  depth inputs.  Same kernels as the 3-D model; its 64-wide heads take the generic attention composition."""

  def __init__(self, num_output_frames: int = 150, num_latent_tokens: int = 128, latent_token_dim: int = 64, num_frequencies: int = 32,
               track_scale_factor: float = 1.0, time_scale_factor: float = 150.0, track_token_dim: int = 256,
               encoder_latent_dim: int = 512, decoder_num_channels: int = 1024, decoder_scan_chunk_size: Optional[int] = None,
               precision: str = 'bf16', workspace_fraction: float = 0.80, track_chunk_size: Optional[int] = None):
    # track_chunk_size: product-only, not part of the reference's signature (see TrackAutoEncoder3D)
    super().__init__(num_output_frames=num_output_frames, num_latent_tokens=num_latent_tokens, latent_token_dim=latent_token_dim,
                     num_frequencies=num_frequencies, track_scale_factor=track_scale_factor, time_scale_factor=time_scale_factor,
                     track_token_dim=track_token_dim, encoder_latent_dim=encoder_latent_dim, decoder_num_channels=decoder_num_channels,
                     dino_feature_dim=0, depth_feature_dim=0, use_dino=False, use_depth=False,
                     decoder_scan_chunk_size=decoder_scan_chunk_size, precision=precision, workspace_fraction=workspace_fraction,
                     track_chunk_size=track_chunk_size)
    self._kind, self._nc = 1, 2
    # transformer sizes of setup() (track_autoencoder.py:149-172)
    self.num_heads, self.qkv_size = 8, 64 * 8
    self.enc_mlp, self.enc_layers = 1024, 2
    self.t2l_mlp, self.t2l_layers = 2048, 6
    self.dec_mlp, self.dec_layers = 2048, 3
    self.ro_mlp, self.ro_layers = 1024, 4


PROF_CLASSES = ('gemm_nt_bf16 (tiled MFMA, Y=X.W / dX=dY.W^T)', 'gemm_tn_bf16 (tiled MFMA, dW=X^T.dY)', 'gemm_generic (strided MFMA)',
                'attention_fused_fwd', 'attention_fused_bwd', 'layernorm_fwd', 'layernorm_bwd', 'attention_single_query (pruned last block)',
                'embed (sin features + token / dino / depth projections + readout row + prune gather; its GEMMs also count in gemm_nt_bf16)')


def profile_summary(model, handle, peak_flops: float = 2.5e15):
  """Reads the live HIP-event timings (spa3d_prof_*): one row per instrumented kernel class with its launches, device ms,
  algorithmic FLOPs and algorithmic bytes (bench.py prices each class against its own roofline)."""
  lib = _lib.load()
  rows = []
  for cls, name in enumerate(PROF_CLASSES):
    o = (C.c_double * 4)()
    _lib.check(lib.spa3d_prof_read(handle, cls, o), handle, 'spa3d_prof_read')
    rows.append({'kernel': name, 'launches': int(o[0]), 'ms': o[1], 'flops': o[2], 'bytes': o[3]})
  if not any(r['launches'] for r in rows):
    return None
  return {'classes': rows, 'peak': peak_flops}
