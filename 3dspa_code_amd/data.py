"""Host-side steps either side of the hot path, with the reference's names:

  prepare_3d_batch                         data_loader.py:56-110   support/query split + query-point sampling
  draw_split / build_batch                 data_loader.py:67-81, inference.py:541-590 for many clips in one device call (spa3d_build_batch)
  convert_predictions_to_tapvid3d_format   evaluate_tapvid3d.py:39-59
  collate_ragged / split_ragged            evaluate_tapvid3d.py:318-348 as batches of clips with differing track / query counts
  load_checkpoint / save_checkpoint        inference.py:450-508, evaluate_tapvid3d.py:247-285 / train.py:389-393 (a stub upstream)

Plain NumPy / torch glue: no arithmetic worth a kernel -- except build_batch, whose host side only validates and marshals.  The metric arithmetic of TAPVid-3D is model.tapvid3d_predictions (upstream
it is the un-vendored `tapnet` package)."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from typing import Any, Dict, Optional

import numpy as np
import torch

from . import _lib


def prepare_3d_batch(example, num_support_tracks: int = 2048, num_query_tracks: int = 2048, num_frames: int = 150, use_dino: bool = True,
                     use_depth: bool = True, device='cuda', feature_dtype=torch.bfloat16):
  """data_loader.py:56-110.  Same RNG call sequence on NumPy's global generator as the reference
  (`np.random.permutation(num_total)` then one `np.random.randint(0, num_frames)` per query track), so a seeded
  reference run and a seeded run of this function pick the same tracks and frames."""
  tracks_3d = np.asarray(example['tracks_3d'])  # [N, T, 3]
  visible = np.asarray(example['visible'])  # [N, T, 1]
  num_total = tracks_3d.shape[0]
  indices = np.random.permutation(num_total)
  support_indices = indices[:num_support_tracks]
  query_indices = indices[num_support_tracks:num_support_tracks + num_query_tracks]
  if len(query_indices) < num_query_tracks:  # the reference would raise IndexError inside its sampling loop
    raise IndexError(f'example has {num_total} tracks, need {num_support_tracks} support + {num_query_tracks} query')
  query_tracks = tracks_3d[query_indices]
  ts = np.array([np.random.randint(0, num_frames) for _ in range(num_query_tracks)])
  xyz = query_tracks[np.arange(num_query_tracks), ts]
  query_points = np.concatenate([ts[:, None].astype(np.float64), xyz.astype(np.float64)], axis=1)  # np.array of python lists -> float64

  def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=dtype)[None]

  batch = {
      'support_tracks': dev(tracks_3d[support_indices]),
      'support_tracks_visible': dev(visible[support_indices]),
      'query_points': dev(query_points),
      'query_tracks': dev(query_tracks),
      'query_tracks_visible': dev(visible[query_indices]),
      'boundary_frame': torch.tensor([num_frames], dtype=torch.int32, device=device),
  }
  if use_dino and 'dino_features' in example:
    batch['dino_features'] = dev(np.asarray(example['dino_features'])[support_indices], feature_dtype)
  if use_depth and 'depth_features' in example:
    batch['depth_features'] = dev(np.asarray(example['depth_features'])[support_indices], feature_dtype)
  return batch


def draw_split(num_total: int, num_support: int, num_query: int, num_frames: int):
  """The support / query split of one clip: (support indices, query indices, query frames).  The RNG call sequence of data_loader.py:67-81 and
  inference.py:560-572 on NumPy's global generator -- one `permutation(num_total)`, then one `randint(0, num_frames)` per query -- so a seeded
  run picks what a seeded prepare_3d_batch (or the reference) picks.  IndexError when the clip has too few tracks, as prepare_3d_batch."""
  indices = np.random.permutation(num_total)
  support = indices[:num_support]
  query = indices[num_support:num_support + num_query]
  if len(support) < num_support or len(query) < num_query:
    raise IndexError(f'clip has {num_total} tracks, need {num_support} support + {num_query} query')
  frames = np.array([np.random.randint(0, num_frames) for _ in range(num_query)], dtype=np.int64)
  return support, query, frames


def _shape(x):
  return tuple(int(v) for v in (x.shape if hasattr(x, 'shape') else np.asarray(x).shape))


def _index_array(x, name, lo, hi, what):
  """A host int64 vector whose entries all lie in [lo, hi); ValueError otherwise (the device never sees an index that was not checked here)."""
  a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
  if a.ndim != 1:
    raise ValueError(f'{name} must be one-dimensional, got shape {a.shape}')
  if a.size and not np.issubdtype(a.dtype, np.integer):
    if not np.all(np.asarray(a, dtype=np.float64) == np.floor(np.asarray(a, dtype=np.float64))):
      raise ValueError(f'{name} must hold integers')
  a = a.astype(np.int64)
  if a.size and (a.min() < lo or a.max() >= hi):
    raise ValueError(f'{name} has entries outside [{lo}, {hi}) ({what})')
  return a


def _clip_sources(clip, model, bad, T):
  """The host checks of one clip dict (build_batch, build_windows): shapes and sources.  T: the most frames it may have (None = any).  Returns
  its plan (sizes, which source serves which output) and the DINO and depth-feature widths it carries (0 = none).  `bad` makes the exception."""
  if clip.get('tracks_2d') is None or clip.get('visible') is None:
    raise bad('tracks_2d and visible are required')
  s2 = _shape(clip['tracks_2d'])
  if len(s2) != 3 or s2[2] != 2 or s2[0] < 1 or s2[1] < 1:
    raise bad(f'tracks_2d must be [n,T,2], got {s2}')
  n, Tc = s2[:2]
  if T is not None and Tc > T:
    raise bad(f'has {Tc} frames, the batch has {T}')
  sv = _shape(clip['visible'])
  if sv not in ((n, Tc), (n, Tc, 1)):
    raise bad(f'visible must be {(n, Tc)} or {(n, Tc, 1)}, got {sv}')
  has3, depth = clip.get('tracks_3d') is not None, clip.get('depth')
  if has3 and _shape(clip['tracks_3d']) != (n, Tc, 3):
    raise bad(f'tracks_3d must be {(n, Tc, 3)}, got {_shape(clip["tracks_3d"])}')
  H = W = 0
  if depth is not None:
    sd = _shape(depth)
    if len(sd) == 4 and sd[3] == 1:
      sd = sd[:3]
    if len(sd) != 3 or sd[0] != Tc or sd[1] < 1 or sd[2] < 1:
      raise bad(f'depth must be [T,H,W] or [T,H,W,1] with T = {Tc}, got {_shape(depth)}')
    H, W = sd[1], sd[2]
  if not has3 and depth is None:
    raise bad('needs tracks_3d, or depth to lift tracks_2d with')
  if clip.get('video_shape') is not None:
    vs = tuple(int(v) for v in clip['video_shape'])
    if len(vs) != 4 or vs[1] < 1 or vs[2] < 1:
      raise bad(f'video_shape must be (T,H,W,3), got {vs}')
    if depth is not None and (vs[1], vs[2]) != (H, W):
      raise bad(f'video_shape {vs} and depth {(H, W)} disagree on the frame size')
    H, W = vs[1], vs[2]
  intr = None
  if clip.get('intrinsics') is not None:
    intr = [float(v) for v in np.asarray(clip['intrinsics'], dtype=np.float64).reshape(-1)]
    if len(intr) != 4:
      raise bad('intrinsics must be (fx, fy, cx, cy)')
  dino, dino_dim = None, 0
  if model.use_dino and (clip.get('dino_map') is not None or clip.get('dino_features') is not None):
    if clip.get('dino_map') is not None and clip.get('dino_features') is not None:
      raise bad('dino_map and dino_features are both given')
    if clip.get('dino_map') is not None:
      sm = _shape(clip['dino_map'])
      if len(sm) != 4 or sm[0] != Tc or min(sm) < 1:
        raise bad(f'dino_map must be [T,Hp,Wp,D] with T = {Tc}, got {sm}')
      if H < 1:
        raise bad('dino_map needs video_shape (or depth) for the frame size')
      dino = ('map', sm)
    else:
      sm = _shape(clip['dino_features'])
      if len(sm) != 3 or sm[:2] != (n, Tc) or sm[2] < 1:
        raise bad(f'dino_features must be [{n},{Tc},D], got {sm}')
      dino = ('pool', sm)
    dino_dim = sm[-1]
  dfeat, depth_dim = None, 0
  if model.use_depth and (clip.get('depth_features') is not None or depth is not None):
    if clip.get('depth_features') is not None:
      sm = _shape(clip['depth_features'])
      if len(sm) != 3 or sm[:2] != (n, Tc) or sm[2] < 1:
        raise bad(f'depth_features must be [{n},{Tc},C], got {sm}')
      if depth is not None and has3:
        raise bad('depth and depth_features are both given (and tracks_3d needs no lift)')
      dfeat = 'pool'
      depth_dim = sm[2]
    else:
      dfeat = 'map'
      depth_dim = int(model.depth_feature_dim)
  return dict(n=n, Tc=Tc, H=H, W=W, has3=has3, dino=dino, dfeat=dfeat, intr=intr), dino_dim, depth_dim


def _clip_upload(c, clip, p, up, act, keep):
  """The device side of one clip's descriptor: uploads what the plan reads (a tensor already on the device in the right type is used as it is),
  fills the sizes and pointers of the _lib.Clip `c`; what the pointers reference goes into `keep`."""
  c.n_tracks, c.T, c.H, c.W = p['n'], p['Tc'], p['H'], p['W']
  tens = {'tracks_2d': up(clip['tracks_2d']), 'visible': up(clip['visible'])}
  if p['has3']:
    tens['tracks_3d'] = up(clip['tracks_3d'])
  if clip.get('depth') is not None and (not p['has3'] or p['dfeat'] == 'map'):
    tens['depth_map'] = up(clip['depth'])
  if p['dino'] is not None and p['dino'][0] == 'map':
    tens['dino_map'] = up(clip['dino_map'])
    c.Hp, c.Wp = p['dino'][1][1], p['dino'][1][2]
  elif p['dino'] is not None:
    tens['dino_pool'] = up(clip['dino_features'], act)
  if p['dfeat'] == 'pool':
    tens['depth_pool'] = up(clip['depth_features'], act)
  for k, t in tens.items():
    setattr(c, k, t.data_ptr())
    keep.append(t)
  if p['intr'] is not None:
    intr = (C.c_double * 4)(*p['intr'])
    keep.append(intr)
    c.intrinsics = C.cast(intr, C.POINTER(C.c_double))


def build_batch(clips, model=None, num_support_tracks: int = 2048, num_query_points: int = 512, num_frames: Optional[int] = None, splits=None,
                device='cuda'):
  """Clips -> the batch dict that model.apply / model.score / model.tapvid3d / TrainState.train_step take, in ONE device call (spa3d_build_batch,
  include/spa3d.h): the split, the lift, the feature sampling and the padded ragged layout, only for the rows that were picked, the feature
  planes written in the model's activation type.  What inference.py:541-590 does per clip over ALL of its tracks, and prepare_3d_batch on the host.

  clips: a list of dicts (NumPy arrays or tensors).  Always `tracks_2d` [n,Tc,2] (pixels) and `visible` [n,Tc] or [n,Tc,1]; for the 3-D
  positions `tracks_3d` [n,Tc,3] or `depth` [Tc,H,W(,1)] to lift with (optional `intrinsics` (fx, fy, cx, cy)); optional DINO as `dino_map`
  [Tc,Hp,Wp,D] + `video_shape` (T,H,W,3) or as already-sampled `dino_features` [n,Tc,D]; optional `depth_features` [n,Tc,C] (without it, and
  with model.use_depth, the depth features are sampled from `depth`, model.depth_feature_dim channels).  Tc <= num_frames (default:
  model.num_output_frames); shorter clips are zero-padded and `boundary_frame` says where they end.
  splits: None = draw_split per clip with min(count, what the clip has), or one (support_index, query_index, query_frame) triple per clip.
  Everything is validated on the host first (ValueError; IndexError from the draw), the index arrays are uploaded once."""
  if model is None:
    raise ValueError('build_batch needs the model (precision and feature widths come from it)')
  if getattr(model, '_kind', 0) == 1:
    raise ValueError('build_batch is not available for the 2-D model')
  if not clips:
    raise ValueError('build_batch needs at least one clip')
  B = len(clips)
  if splits is not None and len(splits) != B:
    raise ValueError(f'splits must have one entry per clip ({B}), got {len(splits)}')
  T = int(num_frames) if num_frames is not None else int(model.num_output_frames)
  if T < 1 or num_support_tracks < 1 or num_query_points < 0:
    raise ValueError('num_frames and num_support_tracks must be positive, num_query_points non-negative')
  # ---- host pass: shapes, sources, splits.  Nothing touches the device before every clip has passed.
  plans, dino_dims, depth_dims = [], set(), set()
  for i, clip in enumerate(clips):
    bad = lambda m: ValueError(f'clip {i}: {m}')
    plan, dd, dpd = _clip_sources(clip, model, bad, T)
    dino_dims.add(dd)
    depth_dims.add(dpd)
    n, Tc = plan['n'], plan['Tc']
    if splits is None:
      ns = min(int(num_support_tracks), n)
      si, qi, qf = draw_split(n, ns, min(int(num_query_points), n - ns), Tc)
    else:
      if len(splits[i]) != 3:
        raise bad('a split is (support_index, query_index, query_frame)')
      si = _index_array(splits[i][0], f'clip {i}: support_index', 0, n, f'the clip has {n} tracks')
      qi = _index_array(splits[i][1], f'clip {i}: query_index', 0, n, f'the clip has {n} tracks')
      qf = _index_array(splits[i][2], f'clip {i}: query_frame', 0, Tc, f'the clip has {Tc} frames')
      if len(qf) != len(qi):
        raise bad(f'{len(qi)} query indices but {len(qf)} query frames')
    if len(si) < 1:
      raise bad('needs at least one support track')
    plans.append(dict(plan, si=si, qi=qi, qf=qf))
  if len(dino_dims) != 1 or len(depth_dims) != 1:
    raise ValueError('every clip of a batch must carry the same features with the same widths '
                     f'(DINO widths {sorted(dino_dims)}, depth widths {sorted(depth_dims)}; 0 = none)')
  D, DD = dino_dims.pop(), depth_dims.pop()
  if D and D != model.dino_feature_dim:
    raise ValueError(f'the clips carry {D} DINO channels, the model has dino_feature_dim = {model.dino_feature_dim}')
  N, Q = max(len(p['si']) for p in plans), max(max(len(p['qi']) for p in plans), 1)
  # ---- device pass
  dev = torch.device(device)
  if dev.type != 'cuda':
    raise _lib.Spa3dError('build_batch runs on the GPU: the 3DSPA hot path is HIP-only (no CPU fallback)')
  if dev.index is None:
    dev = torch.device('cuda', torch.cuda.current_device())
  h = model._handle(D, DD)[0]
  act = model.act_dtype

  def up(x, dtype=torch.float32):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(device=dev, dtype=dtype).contiguous()

  index = torch.from_numpy(np.concatenate([np.concatenate([p['si'], p['qi'], p['qf']]) for p in plans]).astype(np.int32)).to(dev)  # ONE upload
  batch = {
      'support_tracks': torch.empty(B, N, T, 3, dtype=torch.float32, device=dev), 'support_tracks_visible': torch.empty(B, N, T, 1, dtype=torch.float32, device=dev),
      'query_points': torch.empty(B, Q, 4, dtype=torch.float32, device=dev), 'query_tracks': torch.empty(B, Q, T, 3, dtype=torch.float32, device=dev),
      'query_tracks_visible': torch.empty(B, Q, T, 1, dtype=torch.float32, device=dev), 'boundary_frame': torch.empty(B, dtype=torch.int32, device=dev),
  }
  if D:
    batch['dino_features'] = torch.empty(B, N, T, D, dtype=act, device=dev)
  if DD:
    batch['depth_features'] = torch.empty(B, N, T, DD, dtype=act, device=dev)
  arr, keep, off = (_lib.Clip * B)(), [index], 0
  for i, (clip, p) in enumerate(zip(clips, plans)):
    c = arr[i]
    _clip_upload(c, clip, p, up, act, keep)
    ns, nq = len(p['si']), len(p['qi'])
    c.n_support, c.n_query = ns, nq
    c.support_index = index.data_ptr() + 4 * off
    c.query_index = index.data_ptr() + 4 * (off + ns)
    c.query_frame = index.data_ptr() + 4 * (off + ns + nq)
    off += ns + 2 * nq
  out = _lib.Batch()
  out.B, out.N, out.Q, out.T = B, N, Q, T
  for k in ('support_tracks', 'support_tracks_visible', 'query_points', 'query_tracks', 'query_tracks_visible', 'boundary_frame', 'dino_features', 'depth_features'):
    if k in batch:
      setattr(out, k, batch[k].data_ptr())
  with torch.cuda.device(dev):
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().spa3d_build_batch(h, arr, C.byref(out), stream), h, 'spa3d_build_batch')
  del keep  # the call is enqueued: the allocator recycles these on the same stream only
  batch['support_count'] = torch.tensor([len(p['si']) for p in plans], dtype=torch.int32, device=dev)
  batch['query_count'] = torch.tensor([len(p['qi']) for p in plans], dtype=torch.int32, device=dev)
  return batch


# ------------------------------------------------------------------------------------------------ long clips: windows
BLENDS = {'mean': _lib.BLEND_MEAN, 'hat': _lib.BLEND_HAT, 'first': _lib.BLEND_FIRST}
MAX_WINDOWS = 256  # what spa3d_stitch_windows carries by value


def window_starts(num_frames: int, window: int, stride: Optional[int] = None) -> np.ndarray:
  """The plan that cuts a clip of num_frames frames into overlapping windows of `window` frames: the start frames, int32 [W].
  stride defaults to window // 2 (at least 1); 1 <= stride <= window.  num_frames <= window: [0] (one, possibly short, window).  Otherwise
  W = 1 + ceil((num_frames - window) / stride), start w = w * stride for w < W - 1, and the LAST start is num_frames - window, so that the last
  window ends on the last frame.  The starts increase strictly, every frame is covered, none more than ceil(window / stride) + 1 times."""
  for name, v in (('num_frames', num_frames), ('window', window)) + ((('stride', stride),) if stride is not None else ()):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
      raise ValueError(f'{name} must be an int, got {v!r}')
  num_frames, window = int(num_frames), int(window)
  if num_frames < 1 or window < 1:
    raise ValueError(f'num_frames and window must be positive, got {num_frames}, {window}')
  stride = max(window // 2, 1) if stride is None else int(stride)
  if stride < 1 or stride > window:
    raise ValueError(f'stride must lie in [1, window = {window}], got {stride}')
  if num_frames <= window:
    return np.zeros(1, np.int32)
  W = 1 + -(-(num_frames - window) // stride)
  starts = np.arange(W, dtype=np.int64) * stride
  starts[-1] = num_frames - window
  return starts.astype(np.int32)


def _window_plan(starts, num_frames, window, stride, what):
  """`starts` checked (one-dimensional ints in [0, num_frames), strictly increasing), or window_starts when None: int32 [W]."""
  if starts is None:
    return window_starts(num_frames, window, stride)
  if stride is not None:
    raise ValueError(f'{what}: give starts or stride, not both')
  t0 = _index_array(starts, f'{what}: starts', 0, num_frames, f'the clip has {num_frames} frames')
  if len(t0) < 1:
    raise ValueError(f'{what}: needs at least one window')
  if (t0[1:] <= t0[:-1]).any():
    raise ValueError(f'{what}: starts must increase strictly, got {t0.tolist()}')
  return t0.astype(np.int32)


def build_windows(clip, model=None, starts=None, stride=None, order=None, device='cuda', queries=None):
  """One LONG clip -> the batch dict of its W windows (B = W), in one device call per 16 windows (spa3d_build_windows, include/spa3d.h): window w
  is frames [starts[w], starts[w] + model.num_output_frames) of the clip, cut in place -- no sliced copy of a pool or a map is made -- and holds
  what build_batch gives for a clip whose arrays are those frame slices, bit for bit.  The clip dict is the one build_batch takes, with ANY
  number of frames.  starts: window_starts(Tc, num_output_frames, stride) by default, or your own strictly increasing start frames.
  order: the support index list shared by all windows (row r of every window is pool track order[r]); default: all tracks in order.
  queries: None, or (query_index [nq], query_frame [W, nq]) with window-relative frames.  Returns the support keys, `boundary_frame` (the
  windows' live frames) and `window_start` (int32 [W]); with queries also the query keys.  Validated on the host first (ValueError)."""
  if model is None:
    raise ValueError('build_windows needs the model (precision and feature widths come from it)')
  if getattr(model, '_kind', 0) == 1:
    raise ValueError('build_windows is not available for the 2-D model')
  if not isinstance(clip, dict):
    raise ValueError('build_windows takes ONE clip dict')
  bad = lambda m: ValueError(f'clip: {m}')
  p, D, DD = _clip_sources(clip, model, bad, None)
  if D and D != model.dino_feature_dim:
    raise ValueError(f'the clip carries {D} DINO channels, the model has dino_feature_dim = {model.dino_feature_dim}')
  n, TL, Tw = p['n'], p['Tc'], int(model.num_output_frames)
  t0 = _window_plan(starts, TL, Tw, stride, 'build_windows')
  W = len(t0)
  lens = np.minimum(Tw, TL - t0.astype(np.int64))
  si = np.arange(n, dtype=np.int64) if order is None else _index_array(order, 'order', 0, n, f'the clip has {n} tracks')
  if len(si) < 1:
    raise bad('needs at least one support track')
  qi, qf = np.zeros(0, np.int64), np.zeros((W, 0), np.int64)
  if queries is not None:
    if len(queries) != 2:
      raise ValueError('queries is (query_index [nq], query_frame [W, nq])')
    qi = _index_array(queries[0], 'query_index', 0, n, f'the clip has {n} tracks')
    qf = queries[1].detach().cpu().numpy() if isinstance(queries[1], torch.Tensor) else np.asarray(queries[1])
    if qf.shape != (W, len(qi)) or qf.dtype.kind not in 'iu':
      raise ValueError(f'query_frame must be ints [W, nq] = {(W, len(qi))}, got {qf.shape} {qf.dtype}')
    qf = qf.astype(np.int64)
    if qf.size and ((qf < 0).any() or (qf >= lens[:, None]).any()):
      raise ValueError('query_frame has entries outside their window ([0, the window\'s live frames))')
  N, Q = len(si), len(qi)
  # ---- device pass
  dev = torch.device(device)
  if dev.type != 'cuda':
    raise _lib.Spa3dError('build_windows runs on the GPU: the 3DSPA hot path is HIP-only (no CPU fallback)')
  if dev.index is None:
    dev = torch.device('cuda', torch.cuda.current_device())
  h = model._handle(D, DD)[0]
  act = model.act_dtype

  def up(x, dtype=torch.float32):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(device=dev, dtype=dtype).contiguous()

  index = torch.from_numpy(np.concatenate([si, qi, qf.reshape(-1)]).astype(np.int32)).to(dev)  # ONE upload
  batch = {'support_tracks': torch.empty(W, N, Tw, 3, dtype=torch.float32, device=dev), 'support_tracks_visible': torch.empty(W, N, Tw, 1, dtype=torch.float32, device=dev),
           'boundary_frame': torch.empty(W, dtype=torch.int32, device=dev)}
  if Q:
    batch.update({'query_points': torch.empty(W, Q, 4, dtype=torch.float32, device=dev), 'query_tracks': torch.empty(W, Q, Tw, 3, dtype=torch.float32, device=dev),
                  'query_tracks_visible': torch.empty(W, Q, Tw, 1, dtype=torch.float32, device=dev)})
  if D:
    batch['dino_features'] = torch.empty(W, N, Tw, D, dtype=act, device=dev)
  if DD:
    batch['depth_features'] = torch.empty(W, N, Tw, DD, dtype=act, device=dev)
  c, keep = _lib.Clip(), [index]
  _clip_upload(c, clip, p, up, act, keep)
  c.n_support, c.n_query = N, Q
  c.support_index = index.data_ptr()
  c.query_index = index.data_ptr() + 4 * N
  c.query_frame = index.data_ptr() + 4 * (N + Q)
  out = _lib.Batch()
  out.B, out.N, out.Q, out.T = W, N, Q, Tw
  for k in ('support_tracks', 'support_tracks_visible', 'query_points', 'query_tracks', 'query_tracks_visible', 'boundary_frame', 'dino_features', 'depth_features'):
    if k in batch:
      setattr(out, k, batch[k].data_ptr())
  with torch.cuda.device(dev):
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().spa3d_build_windows(h, C.byref(c), W, (C.c_int32 * W)(*t0.tolist()), C.byref(out), stream), h, 'spa3d_build_windows')
  del keep  # the call is enqueued: the allocator recycles these on the same stream only
  batch['window_start'] = torch.from_numpy(t0.copy()).to(dev)
  return batch


_STITCH_HANDLE = []


def _stitch_handle():
  """A handle of the stitch calls' own: spa3d_stitch_windows uses its handle for the error message and the stream only, and must not reset
  those of a handle a model is using."""
  if not _STITCH_HANDLE:
    from .model import TrackAutoEncoder3D
    _STITCH_HANDLE.append(TrackAutoEncoder3D(num_output_frames=8, use_dino=False, use_depth=False, precision='fp32'))  # the model owns its handles
  return _STITCH_HANDLE[0]._handle(0, 0)[0]


def stitch_windows(starts, num_frames: int, tracks=None, visible_logits=None, frame_err=None, blend='hat', lengths=None, row_track=None, spread: bool = False):
  """Per-window results of a long clip merged onto the clip's own time axis (spa3d_stitch_windows, include/spa3d.h, which defines the blend).
  starts: int [W] window start frames; num_frames: TL; lengths: int [W] live frames per window (default min(Tw, TL - start)).
  tracks [W,N,Tw,3 or 2], visible_logits and frame_err [W,N,Tw] or [W,N,Tw,1]: device tensors, each optional.  blend: 'mean' | 'hat' | 'first'.
  row_track: None, or a permutation of range(N) (window row r is row row_track[r] of the results).  Returns a dict with the keys of the inputs
  given ([N,TL,NC] / [N,TL]) and, with spread=True, `spread` [N,TL].  The plan and the permutation are validated on the host (ValueError)."""
  if blend not in BLENDS:
    raise ValueError(f'blend must be one of {sorted(BLENDS)}, got {blend!r}')
  given = {k: v for k, v in (('tracks', tracks), ('visible_logits', visible_logits), ('frame_err', frame_err)) if v is not None}
  if not given:
    raise ValueError('stitch_windows needs tracks, visible_logits or frame_err')
  if spread and tracks is None:
    raise ValueError('spread needs tracks')
  for k, v in given.items():
    if not isinstance(v, torch.Tensor):
      raise ValueError(f'{k} must be a tensor')
  first = next(iter(given.values()))
  if first.dim() < 3:
    raise ValueError(f'inputs must be [W,N,Tw,...], got {tuple(first.shape)}')
  W, N, Tw = (int(v) for v in first.shape[:3])
  NC = 3
  for k, v in given.items():
    shp = tuple(int(x) for x in v.shape)
    if k == 'tracks':
      if len(shp) != 4 or shp[:3] != (W, N, Tw) or shp[3] not in (2, 3):
        raise ValueError(f'tracks must be [W,N,Tw,3] (or 2), got {shp}')
      NC = shp[3]
    elif shp not in ((W, N, Tw), (W, N, Tw, 1)):
      raise ValueError(f'{k} must be {(W, N, Tw)} or {(W, N, Tw, 1)}, got {shp}')
  if isinstance(num_frames, bool) or not isinstance(num_frames, (int, np.integer)) or num_frames < 1:
    raise ValueError(f'num_frames must be a positive int, got {num_frames!r}')
  TL = int(num_frames)
  if W < 1 or W > MAX_WINDOWS or N < 1 or Tw < 1:
    raise ValueError(f'W = {W} must lie in [1, {MAX_WINDOWS}] and N, Tw be positive')
  t0 = _window_plan(starts, TL, Tw, None, 'stitch_windows')
  if len(t0) != W:
    raise ValueError(f'{len(t0)} starts for W = {W} windows')
  if lengths is None:
    ln = np.minimum(Tw, TL - t0.astype(np.int64))
  else:
    ln = _index_array(lengths, 'lengths', 1, Tw + 1, f'a window has {Tw} frames')
    if len(ln) != W:
      raise ValueError(f'{len(ln)} lengths for W = {W} windows')
    if (t0 + ln > TL).any():
      raise ValueError(f'a window runs past num_frames = {TL}')
  end = 0
  for w in range(W):
    if t0[w] > end:
      raise ValueError(f'the windows leave a gap: frames [{end}, {int(t0[w])}) are covered by none')
    end = max(end, int(t0[w] + ln[w]))
  if end != TL:
    raise ValueError(f'the windows leave a gap: frames [{end}, {TL}) are covered by none')
  perm = None
  if row_track is not None:
    perm = _index_array(row_track, 'row_track', 0, N, f'there are {N} rows')
    if len(perm) != N or len(np.unique(perm)) != N:
      raise ValueError(f'row_track must be a permutation of range({N})')
  # ---- device pass
  dev = first.device
  if dev.type != 'cuda':
    raise _lib.Spa3dError('stitch_windows runs on the GPU: the 3DSPA hot path is HIP-only (no CPU fallback)')
  s = _lib.Stitch()
  s.W, s.N, s.Tw, s.TL, s.NC, s.blend = W, N, Tw, TL, NC, BLENDS[blend]
  t0c, lnc = (C.c_int32 * W)(*t0.tolist()), (C.c_int32 * W)(*[int(v) for v in ln])
  s.t0, s.len = t0c, lnc
  keep, res = [], {}
  if perm is not None:
    keep.append(torch.from_numpy(perm.astype(np.int32)).to(dev))
    s.row_track = keep[-1].data_ptr()
  for k, v in given.items():
    v = v.to(device=dev, dtype=torch.float32).contiguous()
    keep.append(v)
    setattr(s, k, v.data_ptr())
    res[k] = torch.empty((N, TL, NC) if k == 'tracks' else (N, TL), dtype=torch.float32, device=dev)
    setattr(s, 'out_' + k, res[k].data_ptr())
  if spread:
    res['spread'] = torch.empty(N, TL, dtype=torch.float32, device=dev)
    s.out_spread = res['spread'].data_ptr()
  h = _stitch_handle()
  with torch.cuda.device(dev):
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().spa3d_stitch_windows(h, C.byref(s), stream), h, 'spa3d_stitch_windows')
  del keep
  return res


def convert_predictions_to_tapvid3d_format(predictions, query_points=None):
  """evaluate_tapvid3d.py:39-59: [B,Q,T,3] -> pred_tracks [T,Q,3], pred_occluded [T,Q] (True = occluded, logit <= 0)."""
  pred_tracks = predictions.tracks.detach().float().cpu().numpy()[0]
  logits = predictions.visible_logits.detach().float().cpu().numpy()[0, :, :, 0]
  return np.transpose(pred_tracks, (1, 0, 2)), np.transpose(logits <= 0.0, (1, 0))


# ------------------------------------------------------------------------------------------------ ragged batches
# keys whose second dimension is the support-track axis / the query axis of a [B, ...] batch
SUPPORT_KEYS = ('support_tracks', 'support_tracks_visible', 'dino_features', 'depth_features')
QUERY_KEYS = ('query_points', 'query_tracks', 'query_tracks_visible', 'query_weight')


def validate_counts(counts, B: int, limit: int, name: str, minimum: int):
  """Per-sample counts of a ragged batch (include/spa3d.h, spa3d_set_counts) as a list of B ints in [minimum, limit]; None stays None.
  ValueError otherwise -- the library would refuse the same values with SPA3D_ERR_ARG."""
  if counts is None:
    return None
  vals = counts.detach().cpu().reshape(-1).tolist() if isinstance(counts, torch.Tensor) else list(np.asarray(counts).reshape(-1).tolist())
  if len(vals) != B:
    raise ValueError(f'{name} must have one entry per sample (B = {B}), got {len(vals)}')
  out = []
  for i, v in enumerate(vals):
    if int(v) != v:
      raise ValueError(f'{name}[{i}] = {v!r} is not an integer')
    v = int(v)
    if v < minimum or v > limit:
      raise ValueError(f'{name}[{i}] = {v} is outside [{minimum}, {limit}]')
    out.append(v)
  return out


def fold_offsets(num_tracks: int, folds: int) -> np.ndarray:
  """The offsets [folds + 1] (int32) that cut num_tracks tracks into `folds` contiguous folds of near-equal size, the larger folds first: what
  model.score_all(folds=int) uses and spa3d_score_folds_workspace_bytes sizes for.  Contiguous folds of a shuffled clip are random folds."""
  if isinstance(folds, bool) or not isinstance(folds, (int, np.integer)) or isinstance(num_tracks, bool) or not isinstance(num_tracks, (int, np.integer)):
    raise ValueError(f'num_tracks and folds must be ints, got {num_tracks!r}, {folds!r}')
  if folds < 2 or folds > 64:
    raise ValueError(f'folds must lie in [2, 64], got {folds}')
  if folds > num_tracks:
    raise ValueError(f'{folds} folds need at least as many tracks, got {num_tracks}')
  sizes = np.full(folds, num_tracks // folds, dtype=np.int64)
  sizes[:num_tracks % folds] += 1
  return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def collate_ragged(samples, pad_value: float = 0.0):
  """A list of per-clip dicts (support keys [n_b, T, ...], query keys [q_b, ...], `boundary_frame` a scalar or [1]; no batch axis) -> one
  padded batch ([B, max n_b, T, ...], [B, max q_b, ...]) with `support_count` / `query_count` (int32 [B]).  Rows at or beyond a count are
  padding (`pad_value`): the library never reads them.  Every clip carries the same keys and the same T; tensors stay on their device."""
  if not samples:
    raise ValueError('collate_ragged needs at least one sample')
  keys = [k for k in samples[0] if k not in ('support_count', 'query_count')]
  for s in samples:
    if sorted(k for k in s if k not in ('support_count', 'query_count')) != sorted(keys):
      raise ValueError('every sample of a ragged batch must carry the same keys')
  ns = [int(torch.as_tensor(s['support_tracks']).shape[0]) for s in samples] if 'support_tracks' in keys else None
  qs = [int(torch.as_tensor(s['query_points']).shape[0]) for s in samples] if 'query_points' in keys else None
  if ns is not None and min(ns) < 1:
    raise ValueError('every sample needs at least one support track')
  batch = {}
  for k in keys:
    ts = [torch.as_tensor(s[k]) for s in samples]
    if k == 'boundary_frame':
      batch[k] = torch.stack([t.reshape(()).to(torch.int32) for t in ts])
      continue
    counts = ns if k in SUPPORT_KEYS else (qs if k in QUERY_KEYS else None)
    if counts is None:
      batch[k] = torch.stack(ts)
      continue
    if any(int(t.shape[0]) != c for t, c in zip(ts, counts)) or any(t.shape[1:] != ts[0].shape[1:] for t in ts):
      raise ValueError(f'{k}: leading dimension must be the clip\'s own count and the remaining shape equal across clips')
    out = torch.full((len(ts), max(max(counts), 1)) + tuple(ts[0].shape[1:]), pad_value, dtype=ts[0].dtype, device=ts[0].device)
    for i, (t, c) in enumerate(zip(ts, counts)):
      out[i, :c] = t
    batch[k] = out
  dev = batch['support_tracks'].device if 'support_tracks' in batch else batch['query_points'].device
  if 'boundary_frame' in batch:
    batch['boundary_frame'] = batch['boundary_frame'].to(dev)  # per-clip scalars are often host values; the batch lives on one device
  if ns is not None:
    batch['support_count'] = torch.tensor(ns, dtype=torch.int32, device=dev)
  if qs is not None:
    batch['query_count'] = torch.tensor(qs, dtype=torch.int32, device=dev)
  return batch


def split_ragged(results, batch):
  """Back to per-clip views: `results` is a TrackAutoEncoderResults-like object (tensor attributes with leading [B, Q]) or a dict of
  such tensors; returns a list of B dicts whose tensors are the views [q_b, ...] of the live rows.  A TrackScores comes back as a list of B
  TrackScores (query_stats [q_b, S], sample_stats [S], frame_err [q_b, T]), a TapVid3DScores as a list of B TapVid3DScores."""
  if hasattr(results, 'query_stats') and hasattr(results, 'row_scale'):  # TapVid3DScores: one per clip, cut to its live rows
    B, Q = results.query_stats.shape[:2]
    qc = validate_counts(batch.get('query_count'), B, Q, 'query_count', 0) or [Q] * B
    return [dataclasses.replace(results, query_stats=results.query_stats[i, :qc[i]], sample_stats=results.sample_stats[i], scale=results.scale[i],
                                row_scale=results.row_scale[i, :qc[i]], ratio=None if results.ratio is None else results.ratio[i, :qc[i]]) for i in range(B)]
  if hasattr(results, 'query_stats') and hasattr(results, 'sample_stats'):  # TrackScores: one TrackScores per clip, cut to its live rows
    B, Q = results.query_stats.shape[:2]
    qc = validate_counts(batch.get('query_count'), B, Q, 'query_count', 0) or [Q] * B
    cut = lambda t, i: None if t is None else t[i, :qc[i]]
    preds = [None] * B if results.predictions is None else [
        dataclasses.replace(results.predictions, **{k: v[i, :qc[i]] for k, v in vars(results.predictions).items() if isinstance(v, torch.Tensor)}) for i in range(B)]
    return [dataclasses.replace(results, query_stats=cut(results.query_stats, i), sample_stats=None if results.sample_stats is None else results.sample_stats[i],
                                frame_err=cut(results.frame_err, i), predictions=preds[i]) for i in range(B)]
  if isinstance(results, dict):
    fields = {k: v for k, v in results.items() if isinstance(v, torch.Tensor)}
  else:
    fields = {k: v for k, v in vars(results).items() if isinstance(v, torch.Tensor)}
  B = next(iter(fields.values())).shape[0]
  Q = next(iter(fields.values())).shape[1]
  qc = validate_counts(batch.get('query_count'), B, Q, 'query_count', 0) or [Q] * B
  return [{k: v[i, :qc[i]] for k, v in fields.items()} for i in range(B)]


def save_scores_npz(path: str, coords, frame_scores, visibs, **extra):
  """Writes per-point scores in the layout upstream's visualiser reads: TIME-major `coords` [T, N, 3], `coords_score` [T, N], `visibs` [T, N]
  (plus whatever the caller owns: video, intrinsics, extrinsics, ...).  Inputs are the library's track-major tensors of ONE clip: coords
  [N, T, 3], frame_scores [N, T] (e.g. TrackScores.frame_err[b], or any score derived from it), visibs [N, T] or [N, T, 1]."""
  to_np = lambda t: t.detach().float().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float32)
  c, s, v = to_np(coords), to_np(frame_scores), to_np(visibs)
  if v.ndim == 3 and v.shape[-1] == 1:
    v = v[..., 0]
  if s.ndim == 3 and s.shape[-1] == 1:
    s = s[..., 0]
  if c.ndim != 3 or s.shape != c.shape[:2] or v.shape != c.shape[:2]:
    raise ValueError(f'coords must be [N, T, C] and frame_scores / visibs [N, T]; got {c.shape}, {s.shape}, {v.shape}')
  for k in ('coords', 'coords_score', 'visibs'):
    if k in extra:
      raise ValueError(f'{k!r} is written from the positional arguments')
  np.savez(path, coords=np.ascontiguousarray(c.transpose(1, 0, 2)), coords_score=np.ascontiguousarray(s.T), visibs=np.ascontiguousarray(v.T > 0.5),
           **{k: (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)) for k, t in extra.items()})


# ------------------------------------------------------------------------------------------------ checkpoints
def _flatten(tree, prefix=''):
  out = {}
  for k, v in tree.items():
    key = f'{prefix}/{k}' if prefix else k
    if isinstance(v, dict):
      out.update(_flatten(v, key))
    else:
      out[key] = v
  return out


def _unflatten_params(flat: Dict[str, Any]) -> Dict[str, Any]:
  """inference.py:450-461."""
  result: Dict[str, Any] = {}
  for key, value in flat.items():
    parts = key.split('/')
    d = result
    for part in parts[:-1]:
      d = d.setdefault(part, {})
    d[parts[-1]] = value
  return result


def save_checkpoint(path: str, params, state=None):
  """The save the reference leaves as a log line (train.py:389-393).  Flat 'a/b/c' keys -- the third layout its own
  loader accepts (inference.py:483-485) -- so the file loads in the reference too; optimizer moments and the step go
  under 'opt_m/...', 'opt_v/...', 'step' when a TrainState is given (resume), and its weight EMA, when it keeps one, under 'ema/...'."""
  flat = {k: v.detach().float().cpu().numpy() for k, v in _flatten(params).items()}
  if state is not None:
    names = list(_flatten(state.params).keys())
    m_tree = state.model.tree_from_flat(state.m, *state.model._dims_from_params(state.params))
    v_tree = state.model.tree_from_flat(state.v, *state.model._dims_from_params(state.params))
    flat.update({f'opt_m/{k}': t.detach().cpu().numpy() for k, t in _flatten(m_tree).items()})
    flat.update({f'opt_v/{k}': t.detach().cpu().numpy() for k, t in _flatten(v_tree).items()})
    flat['step'] = np.array(state.step, dtype=np.int64)
    # skipped-step counter, dynamic loss-scale multiplier and its good-step counter (spa3d_adamw_step scratch[3..5]) belong to the optimizer state
    flat['opt_scratch'] = state.scratch[3:6].detach().cpu().numpy()
    if getattr(state, 'ema', None) is not None:  # the weight EMA of a state created with ema_decay; a state without one writes the keys it always wrote
      e_tree = state.model.tree_from_flat(state.ema, *state.model._dims_from_params(state.params))
      flat.update({f'ema/{k}': t.detach().cpu().numpy() for k, t in _flatten(e_tree).items()})
    assert names
  if not path.endswith('.npz'):
    path = path + '.npz'
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  np.savez(path, **flat)
  return path


def load_checkpoint(checkpoint_path: str, model=None, allow_pickle: bool = False, ema: bool = False):
  """inference.py:464-508 for `.npz` files.  Flat-key files (and files written by save_checkpoint) load with
  allow_pickle=False; the two pickled layouts ('params' / 'optimizer' object arrays) execute code from the file when
  unpickled, so they need an explicit allow_pickle=True from the caller.  Returns the nested parameter dict (optimizer
  entries, if present, under the keys 'opt_m', 'opt_v', 'ema', 'step' are stripped -- use load_train_state for those).
  `ema=True` returns the weight EMA of a save_checkpoint file (its 'ema/...' entries) in place of the parameters."""
  if not os.path.exists(checkpoint_path):
    raise FileNotFoundError(f'Checkpoint not found: {checkpoint_path}')
  if ema:
    if not checkpoint_path.endswith('.npz'):
      raise ValueError('ema=True reads the flat-key .npz files of save_checkpoint')
    data = np.load(checkpoint_path, allow_pickle=False)
    flat = {k[len('ema/'):]: np.array(data[k]) for k in data.files if k.startswith('ema/')}
    if not flat:
      raise KeyError(f'{checkpoint_path} holds no weight EMA (no ema/ entries)')
    return _unflatten_params(flat)
  if not checkpoint_path.endswith('.npz'):  # Flax format (evaluate_tapvid3d.py:278-285, inference.py:490-503)
    state_dict = restore_flax_checkpoint(checkpoint_path)
    if 'params' in state_dict:
      return state_dict['params']
    if 'optimizer' in state_dict and isinstance(state_dict['optimizer'], dict) and 'target' in state_dict['optimizer']:
      return state_dict['optimizer']['target']
    return state_dict
  data = np.load(checkpoint_path, allow_pickle=allow_pickle)
  if 'params' in data.files:
    p = data['params']
    params = p.item() if p.ndim == 0 else dict(p)
  elif 'optimizer' in data.files:
    opt = data['optimizer']
    opt = opt.item() if opt.ndim == 0 else dict(opt)
    params = opt.get('target', opt) if isinstance(opt, dict) else opt
  else:
    flat = {k: np.array(data[k]) for k in data.files if not (k.startswith('opt_m/') or k.startswith('opt_v/') or k.startswith('ema/') or k in ('step', 'opt_scratch'))}
    params = _unflatten_params(flat)
  return params


# ------------------------------------------------------------------------------------------------ Flax msgpack checkpoints
# `flax.training.checkpoints.restore_checkpoint(path, target=None)` (evaluate_tapvid3d.py:278, inference.py:490) restated: Flax is not
# installed here and the reference holds no such file, so this follows Flax's documented serialization format -- PARITY UNPINNED:
#   file      = msgpack(state_dict)                                  nested dicts with str keys
#   ndarray   = ExtType(1, msgpack((shape, dtype_name, raw C-order bytes)))
#   complex   = ExtType(2, msgpack((real, imag)))          np scalar = ExtType(3, same tuple as ndarray)
#   arrays over 2**30 bytes are stored as {'__msgpack_chunked_array__': True, 'shape': [...], 'chunks': {'0': ndarray, '1': ...}}
#   a checkpoint DIRECTORY holds files `<prefix><step>`; the largest step wins (natural ordering).
_EXT_NDARRAY, _EXT_COMPLEX, _EXT_NPSCALAR = 1, 2, 3


def _nd_from_bytes(data: bytes):
  import msgpack
  shape, dtype_name, buf = msgpack.unpackb(data, raw=True)
  name = dtype_name.decode() if isinstance(dtype_name, bytes) else dtype_name
  if name == 'bfloat16':  # not a NumPy dtype: widen exactly to float32
    u16 = np.frombuffer(buf, dtype=np.uint16).astype(np.uint32) << 16
    return u16.view(np.float32).reshape(tuple(shape))
  return np.frombuffer(buf, dtype=np.dtype(name)).reshape(tuple(shape)).copy()


def _ext_hook(code, data):
  import msgpack
  if code == _EXT_NDARRAY:
    return _nd_from_bytes(data)
  if code == _EXT_COMPLEX:
    re_, im_ = msgpack.unpackb(data)
    return complex(re_, im_)
  if code == _EXT_NPSCALAR:
    return _nd_from_bytes(data)[()]
  return msgpack.ExtType(code, data)


def _unchunk(tree):
  if isinstance(tree, dict):
    if tree.get('__msgpack_chunked_array__'):
      # Flax writes both 'chunks' and 'shape' through _tuple_to_dict: {'0': .., '1': ..} with str keys (a plain list is accepted too).
      # Only the unchunked case has a round-trip here (msgpack_serialize refuses > 2**30-byte arrays); this branch is exercised by a
      # hand-built fixture (tests/test_data_host.py); parity unpinned: no Flax here, no msgpack file in the reference.
      def seq(v):
        return [v[str(i)] for i in range(len(v))] if isinstance(v, dict) else list(v)
      chunks = seq(tree['chunks'])
      return np.concatenate([np.asarray(c).reshape(-1) for c in chunks]).reshape(tuple(int(x) for x in seq(tree['shape'])))
    return {k: _unchunk(v) for k, v in tree.items()}
  return tree


def msgpack_restore(raw: bytes):
  """flax.serialization.msgpack_restore: bytes -> nested dict of NumPy arrays / scalars."""
  import msgpack
  return _unchunk(msgpack.unpackb(raw, ext_hook=_ext_hook, raw=False, strict_map_key=False))


def msgpack_serialize(tree) -> bytes:
  """flax.serialization.msgpack_serialize for nested dicts of arrays / Python scalars (arrays under 2**30 bytes)."""
  import msgpack

  def enc(o):
    if isinstance(o, torch.Tensor):
      o = o.detach().cpu().numpy()
    if isinstance(o, np.ndarray):
      if o.nbytes > 2**30:
        raise ValueError('chunked arrays are not written (every 3DSPA leaf is far below 2**30 bytes)')
      return msgpack.ExtType(_EXT_NDARRAY, msgpack.packb((list(o.shape), o.dtype.name, o.tobytes('C')), use_bin_type=True))
    if isinstance(o, np.generic):
      return msgpack.ExtType(_EXT_NPSCALAR, msgpack.packb(([], o.dtype.name, o.tobytes()), use_bin_type=True))
    if isinstance(o, complex):
      return msgpack.ExtType(_EXT_COMPLEX, msgpack.packb((o.real, o.imag)))
    raise TypeError(f'cannot serialize {type(o)}')

  return msgpack.packb(tree, default=enc, use_bin_type=True, strict_types=True)


def restore_flax_checkpoint(ckpt_dir: str, prefix: str = 'checkpoint_'):
  """checkpoints.restore_checkpoint(ckpt_dir, target=None): a file, or the newest `<prefix><step>` file of a directory."""
  import re
  path = ckpt_dir
  if os.path.isdir(ckpt_dir):
    def step_of(fn):
      m = re.fullmatch(re.escape(prefix) + r'(\d+(?:\.\d+)?)', fn)
      return float(m.group(1)) if m else None
    cands = [(step_of(f), f) for f in os.listdir(ckpt_dir)]
    cands = [c for c in cands if c[0] is not None]
    if not cands:
      raise ValueError(f'Checkpoint at {ckpt_dir} is empty or invalid')  # evaluate_tapvid3d.py:279-280
    path = os.path.join(ckpt_dir, max(cands)[1])
  with open(path, 'rb') as f:
    return msgpack_restore(f.read())


def _group_src(group, src: int = 0) -> int:
  """dist.broadcast takes a GLOBAL rank; `src` is a rank of `group` (a sub-group's rank 0 is generally not global rank 0)."""
  import torch.distributed as dist
  return dist.get_global_rank(group, src) if group is not None else src


def load_train_state(checkpoint_path: str, state, rank0_only: bool = False):
  """Resume: parameters, Adam moments and step back into a TrainState (in place).  Under data parallelism every replica ends
  with rank 0's state: with `rank0_only` only rank 0 reads the file and the buffers + step are broadcast."""
  import torch.distributed as dist
  multi = dist.is_available() and dist.is_initialized() and state.world > 1
  if multi and rank0_only and state.rank != 0:
    step = torch.zeros(1, dtype=torch.int64, device=state.flat.device)
    state.sync_from_rank0()
    dist.broadcast(step, src=_group_src(state.pg), group=state.pg)
    state.step = int(step.item())
    return state
  data = np.load(checkpoint_path, allow_pickle=False)
  model = state.model
  dims = model._dims_from_params(state.params)
  _, leaves, _ = model._handle(*dims)
  for name, shape, off in leaves:
    n = int(np.prod(shape))
    for buf, prefix in ((state.flat, ''), (state.m, 'opt_m/'), (state.v, 'opt_v/')):
      key = prefix + name
      if key not in data.files:
        raise KeyError(f'checkpoint is missing {key!r}')  # cf. check_params_structure, inference.py:608-619
      a = data[key]
      if tuple(a.shape) != tuple(shape):
        raise ValueError(f'shape mismatch for {key}: expected {shape}, got {a.shape}')
      buf[off:off + n] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(-1).to(buf.device)
  if getattr(state, 'ema', None) is not None:
    # the weight EMA: restored from 'ema/<leaf>'; a file without those keys (written by a state that kept none) starts it at the loaded parameters
    state.ema.copy_(state.flat)
    if any(k.startswith('ema/') for k in data.files):
      for name, shape, off in leaves:
        if 'ema/' + name not in data.files:
          raise KeyError(f"checkpoint is missing {'ema/' + name!r}")
        a = data['ema/' + name]
        if tuple(a.shape) != tuple(shape):
          raise ValueError(f'shape mismatch for ema/{name}: expected {shape}, got {a.shape}')
        state.ema[off:off + int(np.prod(shape))] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(-1).to(state.ema.device)
  state.step = int(data['step'])
  if 'opt_scratch' in data.files:  # absent in checkpoints written before round 4: counters start at 0, multiplier at 1
    state.scratch[3:6] = torch.from_numpy(np.asarray(data['opt_scratch'], dtype=np.float32)).to(state.scratch.device)
  if multi:
    state.sync_from_rank0()
    if rank0_only:
      dist.broadcast(torch.tensor([state.step], dtype=torch.int64, device=state.flat.device), src=_group_src(state.pg), group=state.pg)
  return state
