"""Long clips on the GPU: spa3d_build_windows, spa3d_stitch_windows and TrackAutoEncoder3D.score_video (include/spa3d.h).  Everything is compared
BIT FOR BIT except the spread, whose square root on the device is not promised correctly rounded (2 ulp of fp32).

  1. build_windows against build_batch on frame slices of the long clip: D = 40 and 30 (the vector and the scalar path), depth widths 1 and 3, the
     three precisions; stride 4, stride 8 with the last window moved back, stride 1; a clip shorter than the window; pools instead of maps and
     tracks_3d instead of a lift; more windows than one launch holds; window-relative queries.
  2. stitch_windows against the NumPy restatement (tests/windows_util.py): N = 5 and 70, Tw = 8 and 150, TL up to 400, the three blends, with
     and without a row permutation, a short last window, NaN in one window's row, two calls, outputs in canary-guarded allocations.
  3. score_video with one window against one score_all call.
  4. score_video with four windows against the by-hand route (build_batch on slices, score_all, the NumPy stitch), all windows per call and one.
  5. One full-width run: the default model in bf16."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity_util as PU
import windows_util as WU
from util import MINI, O, product_model

pytestmark = pytest.mark.gpu
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
LAUNCH_WINDOWS = 16  # BB_CLIPS of csrc/batch_build.hip: what one launch holds


def _bits(t):
  t = t.detach().cpu().contiguous()
  return t.view({4: torch.int32, 2: torch.int16}[t.element_size()]) if t.is_floating_point() else t


def _same(a, b, what=''):
  assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), f'{what}: {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}'
  assert torch.equal(_bits(a), _bits(b)), f'{what}: {int((_bits(a) != _bits(b)).sum())} of {a.numel()} elements differ'


def _model(spa3d, T, D, DD, precision):
  return spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=D, depth_feature_dim=DD, use_dino=D > 0, use_depth=DD > 0, precision=precision)


# ---------------------------------------------------------------------------------------------- 1. build_windows
FRAME_KEYS = ('depth', 'dino_map')                                                    # [T, ...]
TRACK_KEYS = ('tracks_2d', 'visible', 'tracks_3d', 'dino_features', 'depth_features')  # [n, T, ...]


def _long_clip(n, TL, D, H=28, W=42, Hp=2, Wp=3, seed=0):
  rng = np.random.default_rng(seed)
  tr = np.stack([rng.random((n, TL)) * (W + 6) - 3, rng.random((n, TL)) * (H + 6) - 3], -1).astype(np.float32)   # some points outside the frame
  tr[0, 0] = (0.0, 0.0)
  tr[1, TL - 1] = (W - 1.0, H - 1.0)  # integer coordinates: weights exactly 0
  return {'tracks_2d': tr, 'visible': (rng.random((n, TL, 1)) < 0.6).astype(np.float32), 'depth': (rng.random((TL, H, W, 1)) * 5 + 0.5).astype(np.float32),
          'dino_map': rng.standard_normal((TL, Hp, Wp, D)).astype(np.float32), 'video_shape': (TL, H, W, 3)}


def _slice(clip, a, b):
  """frames [a, b) of the clip as a clip of its own"""
  out = {}
  for k, v in clip.items():
    if k in FRAME_KEYS:
      out[k] = v[a:b]
    elif k in TRACK_KEYS:
      out[k] = v[:, a:b]
    elif k == 'video_shape':
      out[k] = (b - a,) + tuple(v[1:])
    else:
      out[k] = v
  return out


def _by_slices(spa3d, clip, model, starts, order, queries=None):
  TL, Tw = clip['tracks_2d'].shape[1], model.num_output_frames
  slices = [_slice(clip, int(a), min(int(a) + Tw, TL)) for a in starts]
  qi = np.zeros(0, np.int64) if queries is None else queries[0]
  splits = [(order, qi, np.zeros(0, np.int64) if queries is None else queries[1][w]) for w in range(len(starts))]
  return spa3d.build_batch(slices, model=model, splits=splits)


def _compare_windows(got, want, starts, queries=False):
  keys = ['support_tracks', 'support_tracks_visible', 'boundary_frame'] + [k for k in ('dino_features', 'depth_features') if k in want]
  if queries:
    keys += ['query_points', 'query_tracks', 'query_tracks_visible']
  assert sorted(got) == sorted(keys + ['window_start']), sorted(got)
  for k in keys:
    _same(got[k], want[k], k)
  assert got['window_start'].tolist() == [int(s) for s in starts] and got['window_start'].dtype == torch.int32


@pytest.mark.parametrize('D,DD,precision', [(40, 1, 'bf16'), (40, 3, 'fp32'), (40, 3, 'fp16'), (30, 1, 'fp32'), (30, 3, 'bf16'), (30, 1, 'fp16')])
def test_build_windows_equals_build_batch_on_slices(D, DD, precision):
  import spa3d
  n, TL, Tw = 24, 20, 8
  clip = _long_clip(n, TL, D, seed=D + DD)
  model = _model(spa3d, Tw, D, DD, precision)
  rng = np.random.default_rng(3)
  order = rng.permutation(n)[:17]
  for stride, starts in ((4, [0, 4, 8, 12]), (8, [0, 8, 12]), (1, list(range(13)))):
    assert spa3d.window_starts(TL, Tw, stride).tolist() == starts
    got = spa3d.build_windows(clip, model, stride=stride, order=order)
    want = _by_slices(spa3d, clip, model, starts, order)
    _compare_windows(got, want, starts)
    W = len(starts)
    assert got['support_tracks'].shape == (W, 17, Tw, 3) and got['boundary_frame'].tolist() == [Tw] * W and got['dino_features'].dtype == DTYPES[precision]
    assert got['dino_features'].shape == (W, 17, Tw, D) and got['depth_features'].shape == (W, 17, Tw, DD)
    # the comparison is not vacuous, and a window's first frame has no earlier frame: channel 2 of the depth feature is 0 there
    assert _bits(got['dino_features']).any() and _bits(got['depth_features'][..., 0]).all()
    if DD == 3:
      assert not _bits(got['depth_features'][:, :, 0, 2]).any() and _bits(got['depth_features'][:, :, 1:, 2]).any()
  # default order (every track) and explicit starts; window-relative queries
  starts = [0, 3, 12]
  queries = (np.array([5, 23, 0, 5]), rng.integers(0, Tw, (3, 4)))
  got = spa3d.build_windows(clip, model, starts=starts, queries=queries)
  _compare_windows(got, _by_slices(spa3d, clip, model, starts, np.arange(n), queries), starts, queries=True)
  assert got['query_points'].shape == (3, 4, 4) and got['query_points'][:, :, 0].cpu().long().tolist() == queries[1].tolist()
  # two calls give equal bytes
  again = spa3d.build_windows(clip, model, starts=starts, queries=queries)
  for k in got:
    _same(got[k], again[k], k)


def test_a_clip_shorter_than_the_window_is_one_padded_window():
  import spa3d
  n, TL, Tw, D, DD = 24, 5, 8, 40, 3
  clip = _long_clip(n, TL, D, seed=9)
  model = _model(spa3d, Tw, D, DD, 'bf16')
  got = spa3d.build_windows(clip, model)
  _compare_windows(got, spa3d.build_batch([clip], model=model, splits=[(np.arange(n), [], [])]), [0])
  assert got['boundary_frame'].tolist() == [5]
  for k in ('support_tracks', 'support_tracks_visible', 'dino_features', 'depth_features'):
    assert not _bits(got[k][:, :, TL:]).any() and _bits(got[k][:, :, :TL]).any(), k


@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_pools_and_tracks_3d_as_sources(precision):
  import spa3d
  rng = np.random.default_rng(11)
  n, TL, Tw, D, DD = 24, 20, 8, 40, 3
  pool = {'tracks_2d': rng.random((n, TL, 2)).astype(np.float32), 'visible': (rng.random((n, TL)) < 0.5).astype(np.float32),
          'tracks_3d': rng.standard_normal((n, TL, 3)).astype(np.float32), 'dino_features': rng.standard_normal((n, TL, D)).astype(np.float32),
          'depth_features': rng.standard_normal((n, TL, DD)).astype(np.float32)}
  model = _model(spa3d, Tw, D, DD, precision)
  order = rng.permutation(n)
  for stride in (4, 8):
    starts = spa3d.window_starts(TL, Tw, stride)
    got = spa3d.build_windows(pool, model, stride=stride, order=order)
    _compare_windows(got, _by_slices(spa3d, pool, model, starts, order), starts)
    # stated directly: torch indexing of the long pools
    for w, a in enumerate(starts.tolist()):
      _same(got['support_tracks'][w].cpu(), torch.from_numpy(pool['tracks_3d'])[order, a:a + Tw], 'tracks_3d pool')
      _same(got['dino_features'][w].cpu(), torch.from_numpy(pool['dino_features']).to(DTYPES[precision])[order, a:a + Tw], 'dino pool')
      _same(got['depth_features'][w].cpu(), torch.from_numpy(pool['depth_features']).to(DTYPES[precision])[order, a:a + Tw], 'depth pool')
  # tracks_3d given, both features sampled from maps; DINO from the map with a depth pool and a lift
  mapped = _long_clip(n, TL, D, seed=5)
  for clip in (dict(mapped, tracks_3d=pool['tracks_3d']), dict(mapped, depth_features=pool['depth_features'])):
    starts = spa3d.window_starts(TL, Tw, 4)
    _compare_windows(spa3d.build_windows(clip, model, stride=4, order=order), _by_slices(spa3d, clip, model, starts, order), starts)


def test_more_windows_than_one_launch_holds():
  import spa3d
  n, TL, Tw, D, DD = 24, 30, 8, 30, 1
  clip = _long_clip(n, TL, D, seed=4)
  model = _model(spa3d, Tw, D, DD, 'fp32')
  starts = spa3d.window_starts(TL, Tw, 1)
  assert len(starts) == 23 > LAUNCH_WINDOWS
  got = spa3d.build_windows(clip, model, stride=1)
  _compare_windows(got, _by_slices(spa3d, clip, model, starts, np.arange(n)), starts)
  assert _bits(got['support_tracks'][22]).any() and _bits(got['dino_features'][LAUNCH_WINDOWS]).any()


# ---------------------------------------------------------------------------------------------- 2. stitch_windows
def _stitch_c(spa3d, tracks, vlog, ferr, t0, ln, TL, blend, perm, spread=True):
  """spa3d_stitch_windows itself, every output in a canary-guarded allocation: NumPy (tracks [N,TL,NC], logits, errors, spread)"""
  lib = spa3d._lib.load()
  W, N, Tw, NC = tracks.shape
  dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
  s = spa3d._lib.Stitch()
  s.W, s.N, s.Tw, s.TL, s.NC, s.blend = W, N, Tw, TL, NC, WU.BLEND[blend]
  t0c = (C.c_int32 * W)(*[int(v) for v in t0])
  lnc = None if ln is None else (C.c_int32 * W)(*[int(v) for v in ln])
  s.t0, s.len = t0c, lnc
  keep = [dev(tracks), dev(vlog), dev(ferr)]
  s.tracks, s.visible_logits, s.frame_err = (k.data_ptr() for k in keep)
  if perm is not None:
    keep.append(dev(np.asarray(perm, np.int32)))
    s.row_track = keep[-1].data_ptr()
  outs = {'tracks': PU.guarded(N * TL, NC, torch.float32, name='out_tracks'), 'visible_logits': PU.guarded(N, TL, torch.float32, name='out_visible_logits'),
          'frame_err': PU.guarded(N, TL, torch.float32, name='out_frame_err')}
  if spread:
    outs['spread'] = PU.guarded(N, TL, torch.float32, name='out_spread')
  for k, v in outs.items():
    setattr(s, 'out_' + k, v.data_ptr())
  h = spa3d.data._stitch_handle()
  spa3d._lib.check(lib.spa3d_stitch_windows(h, C.byref(s), C.c_void_p(torch.cuda.current_stream().cuda_stream)), h, 'spa3d_stitch_windows')
  torch.cuda.synchronize()
  res = {k: v.cpu().numpy().copy() for k, v in outs.items()}
  PU.check_guards()
  res['tracks'] = res['tracks'].reshape(N, TL, NC)
  return res


def _check_stitch(got, tracks, vlog, ferr, t0, ln, TL, blend, perm, what):
  ln = WU.window_lengths(t0, tracks.shape[2], TL) if ln is None else ln
  b = WU.BLEND[blend]
  want_tr, want_s2 = WU.stitch(tracks, t0, ln, TL, b, perm, want_spread=True)
  for k, want in (('tracks', want_tr), ('visible_logits', WU.stitch(vlog, t0, ln, TL, b, perm)), ('frame_err', WU.stitch(ferr, t0, ln, TL, b, perm))):
    ok = WU.same_bits_or_both_nan(got[k], want)
    assert ok.all(), f'{what}: {k}: {int((~ok).sum())} of {ok.size} elements differ'
  if 'spread' in got:
    want = np.sqrt(want_s2)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got['spread']), nan), f'{what}: spread NaNs'
    d = WU.ulp_diff(got['spread'][~nan], want[~nan])
    assert d.size == 0 or d.max() <= 2, f'{what}: spread is {int(d.max())} ulp off'
    one = WU.coverage(t0, ln, TL) == 1
    assert not got['spread'][:, one].any()
  return want_tr


#          N, Tw, TL, t0, len
STITCH = [(5, 8, 20, [0, 4, 8, 12], None),
          (70, 8, 19, [0, 4, 8, 12, 16], None),            # more rows than one workgroup's waves; a short last window (3 frames)
          (5, 8, 12, [0, 3, 6], [8, 8, 6]),                # frames under 1, 2 and 3 windows
          (70, 8, 11, [0, 4, 9], [5, 6, 2]),               # len < Tw
          (5, 150, 400, [0, 75, 150, 225, 250], None),     # lanes over several 64-frame chunks
          (70, 150, 383, [0, 75, 150, 225, 300], None)]    # a short last window at Tw = 150


@pytest.mark.parametrize('blend', ['mean', 'hat', 'first'])
@pytest.mark.parametrize('case', range(len(STITCH)))
def test_stitch_matches_the_restatement(case, blend):
  import spa3d
  N, Tw, TL, t0, ln = STITCH[case]
  W = len(t0)
  rng = np.random.default_rng(10 * case + WU.BLEND[blend])
  tracks = (rng.standard_normal((W, N, Tw, 3)) * 10.0 ** rng.integers(-2, 3, (W, N, 1, 1))).astype(np.float32)
  vlog, ferr = (4 * rng.standard_normal((W, N, Tw))).astype(np.float32), np.abs(rng.standard_normal((W, N, Tw))).astype(np.float32)
  for perm in (None, rng.permutation(N)):
    got = _stitch_c(spa3d, tracks, vlog, ferr, t0, ln, TL, blend, perm)
    want_tr = _check_stitch(got, tracks, vlog, ferr, t0, ln, TL, blend, perm, f'case {case} {blend} perm={perm is not None}')
    assert np.isfinite(got['tracks']).all() and (got['spread'] > 0).any() == (W > 1)
    again = _stitch_c(spa3d, tracks, vlog, ferr, t0, ln, TL, blend, perm)
    for k in got:
      assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), k   # two calls give equal bytes
    # the Python wrapper is the same call
    dev = lambda a: torch.from_numpy(a).cuda()
    py = spa3d.stitch_windows(t0, TL, tracks=dev(tracks), visible_logits=dev(vlog)[..., None], frame_err=dev(ferr), blend=blend, lengths=ln, row_track=perm, spread=True)
    for k in got:
      assert np.array_equal(py[k].cpu().numpy().view(np.int32), got[k].view(np.int32)), k
  if blend == 'first' and ln is None:   # the lowest-numbered window that covers a frame supplies it: stated directly
    for t in range(TL):
      w = next(i for i, a in enumerate(t0) if a <= t < a + Tw)
      assert np.array_equal(want_tr[perm, t], tracks[w, :, t - t0[w]])


@pytest.mark.parametrize('blend', ['mean', 'hat', 'first'])
def test_nan_appears_exactly_where_its_window_contributes(blend):
  import spa3d
  N, Tw, TL, t0 = 5, 8, 20, [0, 4, 8, 12]
  rng = np.random.default_rng(2)
  tracks, vlog, ferr = (rng.standard_normal(s).astype(np.float32) for s in ((4, N, Tw, 3), (4, N, Tw), (4, N, Tw)))
  for a in (tracks, vlog, ferr):
    a[1, 2] = np.nan                                   # window 1 (frames 4..11), window row 2
    a[3, 4, 4:] = np.nan                               # window 3, row 4, its last four frames: 16..19, under one window -- copied
  perm = rng.permutation(N)
  got = _stitch_c(spa3d, tracks, vlog, ferr, t0, None, TL, blend, perm)
  _check_stitch(got, tracks, vlog, ferr, t0, None, TL, blend, perm, f'nan {blend}')
  frames = np.arange(TL)
  want = np.zeros((N, TL), bool)
  want[perm[2]] = (frames >= (8 if blend == 'first' else 4)) & (frames < 12)
  want[perm[4]] = frames >= 16
  for k in ('visible_logits', 'frame_err'):
    assert np.array_equal(np.isnan(got[k]), want), k
  assert np.array_equal(np.isnan(got['tracks']).all(-1), want) and np.array_equal(np.isnan(got['tracks']).any(-1), want)
  sp = np.zeros((N, TL), bool)
  sp[perm[2]] = (frames >= 4) & (frames < 12)          # window 1's distance is in the spread of every frame it covers; one-window frames read 0
  assert np.array_equal(np.isnan(got['spread']), sp)


# ---------------------------------------------------------------------------------------------- 3., 4. score_video
def _mini(spa3d, precision):
  cfg = O.Config(**MINI, use_dino=True, use_depth=True, dino_feature_dim=6, depth_feature_dim=2)
  return product_model(spa3d, cfg, precision)


def _mini_clip(n, TL, seed=21):
  rng = np.random.default_rng(seed)
  H, W = 12, 10
  return {'tracks_2d': np.stack([rng.random((n, TL)) * W, rng.random((n, TL)) * H], -1).astype(np.float32), 'visible': (rng.random((n, TL)) < 0.8).astype(np.float32),
          'depth': (rng.random((TL, H, W, 1)) + 0.5).astype(np.float32), 'dino_map': rng.standard_normal((TL, 3, 2, 6)).astype(np.float32), 'video_shape': (TL, H, W, 3)}


def _params(model, batch, seed=0):
  params = model.init(0, batch)['params']
  g = torch.Generator().manual_seed(seed)
  for k, v in O.tree_flatten(params).items():
    if k.endswith('bias') or k.endswith('scale'):
      v.add_((0.1 * torch.randn(v.shape, generator=g)).to(v.device))
  return params


def _first_visible(batch):
  """the query-frame rule of score_video, restated: the first frame of the window in which the row is visible, else 0"""
  vis = batch['support_tracks_visible'][..., 0].cpu().numpy() > 0.5
  qf = np.zeros(vis.shape[:2], np.int64)
  for w in range(vis.shape[0]):
    for r in range(vis.shape[1]):
      nz = np.nonzero(vis[w, r])[0]
      qf[w, r] = nz[0] if len(nz) else 0
  return torch.from_numpy(qf).to(torch.int32).cuda()


def _unpermute(t, perm):
  out = torch.empty_like(t)
  out[torch.as_tensor(perm, device=t.device)] = t
  return out


def test_score_video_with_one_window_is_one_score_all_call():
  import spa3d
  n, T = 14, 8
  model = _mini(spa3d, 'fp32')
  clip = _mini_clip(n, T)
  clip['visible'][3] = 0.0                              # a track that is never visible: queried at frame 0
  perm = np.random.default_rng(1).permutation(n)
  batch = spa3d.build_batch([clip], model=model, splits=[(perm, [], [])])
  params = _params(model, batch)
  noise = torch.rand(1, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(2)).cuda()
  vs = model.score_video({'params': params}, clip, folds=3, thresholds=(0.5, 2.0), perm=perm, noise=noise)
  hand = {k: batch[k] for k in ('support_tracks', 'support_tracks_visible', 'boundary_frame', 'dino_features', 'depth_features')}
  hand['query_frame'] = _first_visible(batch)
  assert int(hand['query_frame'][0, list(perm).index(3)]) == 0 and int(hand['query_frame'].max()) > 0
  sc = model.score_all({'params': params}, hand, folds=3, frame_errors=True, return_predictions=True, noise=noise)
  _same(vs.tracks, _unpermute(sc.predictions.tracks[0], perm), 'tracks')
  _same(vs.visible_logits, _unpermute(sc.predictions.visible_logits[0, :, :, 0], perm), 'visible_logits')
  _same(vs.frame_err, _unpermute(sc.frame_err[0], perm), 'frame_err')
  assert not _bits(vs.spread).any() and vs.spread.shape == (n, T)
  _same(vs.targets_tracks, _unpermute(batch['support_tracks'][0], perm), 'targets')
  _same(vs.targets_visible, _unpermute(batch['support_tracks_visible'][0, :, :, 0], perm), 'targets_visible')
  ref = spa3d.score_predictions(sc.predictions, {'query_tracks': batch['support_tracks'], 'query_tracks_visible': batch['support_tracks_visible']}, thresholds=(0.5, 2.0))
  _same(vs.scores.query_stats[0], _unpermute(ref.query_stats[0], perm), 'query_stats')
  assert bool(torch.isfinite(vs.tracks).all()) and float(vs.scores.sample_stats[0, 7]) == T * n
  assert vs.window_start.tolist() == [0] and np.array_equal(vs.perm, perm)
  # the targets are what save_scores_npz and render_tracks take
  assert tuple(vs.targets['query_tracks'].shape) == (1, n, T, 3) and tuple(vs.targets['query_tracks_visible'].shape) == (1, n, T, 1)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_score_video_equals_the_by_hand_route(precision, tmp_path):
  import spa3d
  n, TL, Tw, stride, folds = 24, 20, 8, 4, 3
  model = _mini(spa3d, precision)
  clip = _mini_clip(n, TL, seed=33)
  clip['visible'][5, 4:12] = 0.0                        # invisible throughout window 1 (frames 4..11)
  perm = np.random.default_rng(7).permutation(n)
  starts = spa3d.window_starts(TL, Tw, stride)
  W = len(starts)
  assert starts.tolist() == [0, 4, 8, 12]
  slices = [_slice(clip, int(a), int(a) + Tw) for a in starts]
  keys = ('support_tracks', 'support_tracks_visible', 'boundary_frame', 'dino_features', 'depth_features')
  params = _params(model, spa3d.build_batch(slices[:1], model=model, splits=[(perm, [], [])]))
  variables = {'params': params}
  noise = torch.rand(W, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(5)).cuda()
  results = {}
  for per_call in (W, 1):
    vs = model.score_video(variables, clip, stride=stride, folds=folds, blend='hat', perm=perm, noise=noise, windows_per_call=per_call)
    # by hand, with the same grouping: build_batch on slices, score_all, the NumPy stitch
    parts = {k: [] for k in ('tracks', 'visible_logits', 'frame_err', 'support_tracks', 'support_tracks_visible')}
    for g0 in range(0, W, per_call):
      b = spa3d.build_batch(slices[g0:g0 + per_call], model=model, splits=[(perm, [], [])] * len(slices[g0:g0 + per_call]))
      hand = {k: b[k] for k in keys}
      hand['query_frame'] = _first_visible(b)
      if g0 <= 1 < g0 + per_call:
        assert int(hand['query_frame'][1 - g0, list(perm).index(5)]) == 0
      sc = model.score_all(variables, hand, folds=folds, frame_errors=True, return_predictions=True, noise=noise[g0:g0 + per_call])
      for k, t in (('tracks', sc.predictions.tracks), ('visible_logits', sc.predictions.visible_logits[..., 0]), ('frame_err', sc.frame_err),
                   ('support_tracks', b['support_tracks']), ('support_tracks_visible', b['support_tracks_visible'][..., 0])):
        parts[k].append(t.float().cpu().numpy())
    cat = {k: np.concatenate(v, 0) for k, v in parts.items()}
    ln = WU.window_lengths(starts, Tw, TL)
    want_tr, want_s2 = WU.stitch(cat['tracks'], starts, ln, TL, WU.HAT, perm, want_spread=True)
    for k, want in (('tracks', want_tr), ('visible_logits', WU.stitch(cat['visible_logits'], starts, ln, TL, WU.HAT, perm)),
                    ('frame_err', WU.stitch(cat['frame_err'], starts, ln, TL, WU.HAT, perm)),
                    ('targets_tracks', WU.stitch(cat['support_tracks'], starts, ln, TL, WU.FIRST, perm)),
                    ('targets_visible', WU.stitch(cat['support_tracks_visible'], starts, ln, TL, WU.FIRST, perm))):
      got = getattr(vs, k).cpu().numpy()
      assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), f'{k} (windows_per_call = {per_call})'
      assert np.isfinite(got).all(), k
    sp = vs.spread.cpu().numpy()
    assert WU.ulp_diff(sp, np.sqrt(want_s2)).max() <= 2 and (sp[:, 4:16] > 0).any() and not sp[:, :4].any() and not sp[:, 16:].any()
    # the targets are the clip's own tracks, the scores cover the whole clip
    direct = spa3d.build_batch([_slice(clip, 0, Tw)], model=model, splits=[(np.arange(n), [], [])])
    _same(vs.targets_tracks[:, :Tw], direct['support_tracks'][0], 'targets, first window')
    _same(vs.targets_visible, torch.from_numpy(clip['visible']).cuda(), 'targets_visible')
    ref = spa3d.score_predictions(spa3d.TrackAutoEncoderResults(vs.tracks[None], vs.visible_logits[None, :, :, None], torch.zeros(1, n, TL, 1, device='cuda')), vs.targets)
    _same(vs.scores.query_stats, ref.query_stats, 'query_stats')
    assert float(vs.scores.sample_stats[0, 7]) == TL * n and vs.scores.query_stats.shape[:2] == (1, n)
    results[per_call] = vs
  # score_all processes clips one at a time: the grouping changes nothing
  for k in ('tracks', 'visible_logits', 'frame_err', 'spread', 'targets_tracks', 'targets_visible'):
    _same(getattr(results[W], k), getattr(results[1], k), f'{k}: all windows per call against one')
  # what save_scores_npz takes, as it is
  vs = results[W]
  path = str(tmp_path / 'scores.npz')
  spa3d.save_scores_npz(path, vs.targets_tracks, vs.frame_err, vs.targets_visible)
  z = np.load(path)
  assert z['coords'].shape == (TL, n, 3) and z['coords_score'].shape == (TL, n) and z['visibs'].shape == (TL, n)


def test_score_video_full_width_runs():
  import spa3d
  n, TL = 256, 225
  rng = np.random.default_rng(0)
  H, W = 28, 42
  clip = {'tracks_2d': np.stack([rng.random((n, TL)) * W, rng.random((n, TL)) * H], -1).astype(np.float32), 'visible': (rng.random((n, TL)) < 0.8).astype(np.float32),
          'depth': (rng.random((TL, H, W)) + 0.5).astype(np.float32), 'dino_map': rng.standard_normal((TL, 3, 4, 768)).astype(np.float32), 'video_shape': (TL, H, W, 3)}
  model = spa3d.TrackAutoEncoder3D(precision='bf16')
  first = spa3d.build_windows(clip, model, starts=[0])
  params = model.init(0, dict(first, query_points=torch.zeros(1, 1, 4, device='cuda')))['params']
  vs = model.score_video({'params': params}, clip, stride=75)
  assert vs.window_start.tolist() == [0, 75] and vs.tracks.shape == (n, TL, 3)
  for k in ('tracks', 'visible_logits', 'frame_err', 'spread', 'targets_tracks', 'targets_visible'):
    assert bool(torch.isfinite(getattr(vs, k)).all()), k
  assert float(vs.scores.sample_stats[0, 7]) == TL * n
  assert not bool(vs.spread[:, :75].any()) and not bool(vs.spread[:, 150:].any()) and bool((vs.spread[:, 75:150] > 0).any())
