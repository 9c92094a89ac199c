"""build_batch / spa3d_build_batch on the GPU (include/spa3d.h).  Everything is compared BIT FOR BIT: the kernel runs the samplers' arithmetic
(csrc/build_row.hpp, pinned to the reference's outputs by tests/golden/sampler_golden.npz) and rounds once, so there is no tolerance to set.

  1. the golden clip: every track as support, in order -> the fixture's arrays (fp32) and their torch roundings (bf16, fp16)
  2. a ragged batch of three clips that differ in track count, length, video and map size, against the existing per-clip route
     (lift_2d_to_3d / sample_*_features_for_tracks, indexing, collate_ragged), for D = 768, 40 and 30 (the scalar path) x depth widths 1 and 3
  3. pools (dino_features / depth_features / tracks_3d) as sources, and a clip that mixes a DINO map with a depth pool
  4. more clips than one launch holds
  5. plumbing: model.score on a build_batch dict equals model.score on the composed dict; TrainState.train_step accepts the dict
  6. determinism: two calls give equal bytes
No test hands an out-of-range index to the device: that guard is the header's slot rule, covered on the CPU (tests/test_build_row_host.py)."""
import os

import numpy as np
import pytest
import torch

from util import MINI, O, product_model

pytestmark = pytest.mark.gpu

Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sampler_golden.npz'), allow_pickle=False)
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
LAUNCH_CLIPS = 16  # BB_CLIPS of csrc/batch_build.hip: what one launch holds


def _bits(t):
  t = t.detach().cpu().contiguous()
  return t.view({4: torch.int32, 2: torch.int16}[t.element_size()]) if t.is_floating_point() else t


def _same(a, b, what=''):
  assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), f'{what}: {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}'
  assert torch.equal(_bits(a), _bits(b)), f'{what}: {int((_bits(a) != _bits(b)).sum())} of {a.numel()} elements differ'


def _model(spa3d, T, D, DD, precision):
  return spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=D, depth_feature_dim=DD, use_dino=D > 0, use_depth=DD > 0, precision=precision)


# ---------------------------------------------------------------------------------------------- 1. the golden clip
@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'fp16'])
def test_golden_clip(precision):
  import spa3d
  tr, dp, dn = Z['tracks_2d'], Z['depth'], Z['dino']
  N, T = tr.shape[:2]
  rng = np.random.default_rng(1)
  vis = (rng.random((N, T)) < 0.7).astype(np.float32)
  model = _model(spa3d, T, dn.shape[-1], 256, precision)
  qi, qf = np.array([3, 0, 22, 3]), np.array([3, 0, 4, 1])
  split = (np.arange(N), qi, qf)
  dt = DTYPES[precision]
  for intr, lift in ((None, Z['lift_default']), (tuple(Z['intrinsics']), Z['lift_intr'])):
    clip = {'tracks_2d': tr, 'visible': vis, 'depth': dp, 'dino_map': dn, 'video_shape': tuple(Z['video_shape']), 'intrinsics': intr}
    b = spa3d.build_batch([clip], model=model, splits=[split])
    lift = torch.from_numpy(lift)
    _same(b['support_tracks'][0], lift, 'support_tracks')
    _same(b['support_tracks_visible'][0, :, :, 0], torch.from_numpy(vis), 'visible')
    _same(b['dino_features'][0], torch.from_numpy(Z['dino_tracks']).to(dt), 'dino_features')
    _same(b['depth_features'][0], torch.from_numpy(Z['depth_tracks']).to(dt), 'depth_features')
    _same(b['query_tracks'][0], lift[qi], 'query_tracks')
    _same(b['query_tracks_visible'][0, :, :, 0], torch.from_numpy(vis[qi]), 'query_tracks_visible')
    _same(b['query_points'][0], torch.cat([torch.from_numpy(qf.astype(np.float32))[:, None], lift[qi, qf]], 1), 'query_points')
    assert b['boundary_frame'].tolist() == [T] and b['support_count'].tolist() == [N] and b['query_count'].tolist() == [4]
    assert b['dino_features'].dtype == dt and b['depth_features'].dtype == dt


# ---------------------------------------------------------------------------------------------- 2. ragged
#            n_tracks, T, H, W, Hp, Wp
RAGGED = [(90, 12, 28, 42, 2, 3), (40, 7, 37, 19, 5, 4), (30, 12, 16, 16, 1, 1)]
PICKS = [(70, 9), (33, 0), (1, 17)]
BATCH_T = 12


def _ragged_inputs(D, seed=0):
  rng = np.random.default_rng(seed)
  clips, splits = [], []
  for (n, T, H, W, Hp, Wp), (ns, nq) in zip(RAGGED, PICKS):
    tr = np.stack([rng.random((n, T)) * (W + 6) - 3, rng.random((n, T)) * (H + 6) - 3], -1).astype(np.float32)  # some points outside the frame
    tr[0, 0] = (0.0, 0.0)
    tr[min(1, n - 1), T - 1] = (W - 1.0, H - 1.0)  # integer coordinates: weights exactly 0
    assert (tr[..., 0] < 0).any() and (tr[..., 0] > W - 1).any() and (tr[..., 1] < 0).any() and (tr[..., 1] > H - 1).any()
    clips.append({'tracks_2d': tr, 'visible': (rng.random((n, T, 1)) < 0.6).astype(np.float32), 'depth': (rng.random((T, H, W, 1)) * 5 + 0.5).astype(np.float32),
                  'dino_map': rng.standard_normal((T, Hp, Wp, D)).astype(np.float32), 'video_shape': (T, H, W, 3)})
    perm = rng.permutation(n)
    splits.append((perm[:ns], perm[ns:ns + nq], rng.integers(0, T, nq)))
  return clips, splits


def _pad_t(t, T):
  """[n, Tc, ...] -> [n, T, ...] with zero frames behind the clip's own"""
  out = torch.zeros((t.shape[0], T) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)
  out[:, :t.shape[1]] = t
  return out


def _composed(spa3d, clips, splits, DD, dt, T):
  """The existing route: per clip the three sampler calls over ALL tracks, then indexing, then collate_ragged."""
  samples = []
  for clip, (si, qi, qf) in zip(clips, splits):
    tr = clip['tracks_2d']
    if 'tracks_3d' in clip:
      t3 = torch.as_tensor(clip['tracks_3d']).cuda()
    else:
      t3 = spa3d.lift_2d_to_3d(tr, clip['depth'], clip.get('intrinsics'))
    vis = torch.as_tensor(clip['visible']).cuda().reshape(tr.shape[0], tr.shape[1], 1)
    si_t, qi_t, qf_t = (torch.as_tensor(np.asarray(v)).long().cuda() for v in (si, qi, qf))
    s = {'support_tracks': _pad_t(t3[si_t], T), 'support_tracks_visible': _pad_t(vis[si_t], T), 'query_tracks': _pad_t(t3[qi_t], T),
         'query_tracks_visible': _pad_t(vis[qi_t], T), 'query_points': torch.cat([qf_t.float()[:, None], t3[qi_t, qf_t]], 1),
         'boundary_frame': torch.tensor(tr.shape[1])}
    if 'dino_features' in clip:
      s['dino_features'] = _pad_t(torch.as_tensor(clip['dino_features']).cuda().to(dt)[si_t], T)
    elif 'dino_map' in clip:
      s['dino_features'] = _pad_t(spa3d.sample_dino_features_for_tracks(clip['dino_map'], tr, clip['video_shape']).to(dt)[si_t], T)
    if DD:
      if 'depth_features' in clip:
        s['depth_features'] = _pad_t(torch.as_tensor(clip['depth_features']).cuda().to(dt)[si_t], T)
      else:
        s['depth_features'] = _pad_t(spa3d.sample_depth_features_for_tracks(clip['depth'], tr)[..., :DD].to(dt)[si_t], T)
    samples.append(s)
  return spa3d.collate_ragged(samples)


def _compare(got, want):
  assert sorted(got) == sorted(want)
  for k in want:
    _same(got[k], want[k], k)


@pytest.mark.parametrize('D,DD,precision', [(768, 1, 'bf16'), (768, 3, 'fp32'), (40, 1, 'fp16'), (40, 3, 'bf16'), (30, 1, 'fp32'), (30, 3, 'fp16')])
def test_ragged_batch_equals_the_per_clip_route(D, DD, precision):
  import spa3d
  dt = DTYPES[precision]
  clips, splits = _ragged_inputs(D, seed=D + DD)
  model = _model(spa3d, BATCH_T, D, DD, precision)
  got = spa3d.build_batch(clips, model=model, splits=splits)
  _compare(got, _composed(spa3d, clips, splits, DD, dt, BATCH_T))
  N, Q = 70, 17
  assert got['support_tracks'].shape == (3, N, BATCH_T, 3) and got['query_points'].shape == (3, Q, 4) and got['dino_features'].shape == (3, N, BATCH_T, D)
  assert got['depth_features'].shape == (3, N, BATCH_T, DD) and got['dino_features'].dtype == dt
  assert got['boundary_frame'].tolist() == [12, 7, 12] and got['support_count'].tolist() == [70, 33, 1] and got['query_count'].tolist() == [9, 0, 17]
  # padding slots and padding frames are zeros, in every tensor
  for b, ((_, Tc, *_), (ns, nq)) in enumerate(zip(RAGGED, PICKS)):
    for k in ('support_tracks', 'support_tracks_visible', 'dino_features', 'depth_features'):
      assert not _bits(got[k][b, ns:]).any() and not _bits(got[k][b, :, Tc:]).any(), (k, b)
    for k in ('query_tracks', 'query_tracks_visible'):
      assert not _bits(got[k][b, nq:]).any() and not _bits(got[k][b, :, Tc:]).any(), (k, b)
    assert not _bits(got['query_points'][b, nq:]).any()
    # the live frames are not all zeros: the comparison above is not vacuous
    assert _bits(got['dino_features'][b, :ns, :Tc]).any() and _bits(got['depth_features'][b, :ns, :Tc, 0]).all()
    # a query row is the lifted track at the drawn frame
    qf = torch.as_tensor(np.asarray(splits[b][2])).long()
    qp = got['query_points'][b, :nq].cpu()
    _same(qp[:, 0], qf.float(), 'query frame')
    _same(qp[:, 1:], got['query_tracks'][b, :nq].cpu()[torch.arange(nq), qf], 'query point')
    assert int(qf.max() if nq else 0) < Tc


# ---------------------------------------------------------------------------------------------- 3. pools
@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_pools_as_sources_and_a_clip_mixing_a_map_with_a_pool(precision):
  import spa3d
  dt = DTYPES[precision]
  rng = np.random.default_rng(11)
  D, DD, T = 40, 3, 12
  mapped = _ragged_inputs(D, seed=5)[0][0]
  n, Tm = mapped['tracks_2d'].shape[:2]
  assert Tm == T
  # clip 0: everything from pools (prepare_3d_batch's inputs); clip 1: DINO from the map, depth features from a pool, positions lifted
  pool = {'tracks_2d': rng.random((25, 8, 2)).astype(np.float32), 'visible': (rng.random((25, 8)) < 0.5).astype(np.float32),
          'tracks_3d': rng.standard_normal((25, 8, 3)).astype(np.float32), 'dino_features': rng.standard_normal((25, 8, D)).astype(np.float32),
          'depth_features': rng.standard_normal((25, 8, DD)).astype(np.float32)}
  mixed = dict(mapped, depth_features=rng.standard_normal((n, Tm, DD)).astype(np.float32))
  clips = [pool, mixed]
  splits = [(rng.permutation(25)[:20], np.array([1, 24, 7]), np.array([7, 0, 3])), (rng.permutation(n)[:11], np.array([5, 6]), np.array([11, 2]))]
  model = _model(spa3d, T, D, DD, precision)
  got = spa3d.build_batch(clips, model=model, splits=splits)
  _compare(got, _composed(spa3d, clips, splits, DD, dt, T))
  # torch indexing, stated directly for the pool clip
  si = torch.as_tensor(splits[0][0]).long()
  _same(got['support_tracks'][0, :20, :8].cpu(), torch.from_numpy(pool['tracks_3d'])[si], 'tracks_3d pool')
  _same(got['dino_features'][0, :20, :8].cpu(), torch.from_numpy(pool['dino_features']).to(dt)[si], 'dino pool')
  _same(got['depth_features'][0, :20, :8].cpu(), torch.from_numpy(pool['depth_features']).to(dt)[si], 'depth pool')
  # tracks_3d given and the depth features sampled from the map
  both = dict(mapped, tracks_3d=rng.standard_normal((n, Tm, 3)).astype(np.float32))
  got = spa3d.build_batch([both], model=model, splits=splits[1:])
  _compare(got, _composed(spa3d, [both], splits[1:], DD, dt, T))


# ---------------------------------------------------------------------------------------------- 4. more clips than one launch
def test_more_clips_than_one_launch_holds():
  import spa3d
  rng = np.random.default_rng(4)
  B, n, T, H, W = LAUNCH_CLIPS + 1, 3, 2, 4, 5
  clips = [{'tracks_2d': (rng.random((n, T, 2)) * 4).astype(np.float32), 'visible': np.ones((n, T), np.float32), 'depth': (rng.random((T, H, W)) + 1).astype(np.float32)[..., None]}
           for _ in range(B)]
  splits = [(np.array([2, 0]), np.array([1]), np.array([b % T])) for b in range(B)]
  model = _model(spa3d, T, 0, 0, 'fp32')
  got = spa3d.build_batch(clips, model=model, splits=splits)
  assert 'dino_features' not in got and 'depth_features' not in got and got['support_tracks'].shape == (B, 2, T, 3)
  _compare(got, _composed(spa3d, clips, splits, 0, torch.float32, T))
  assert _bits(got['support_tracks'][B - 1]).any() and got['boundary_frame'].tolist() == [T] * B


# ---------------------------------------------------------------------------------------------- 5. plumbing
def _mini_clips():
  rng = np.random.default_rng(21)
  clips = []
  for n, T, H, W in ((14, 8, 12, 10), (9, 5, 7, 9)):
    clips.append({'tracks_2d': np.stack([rng.random((n, T)) * W, rng.random((n, T)) * H], -1).astype(np.float32), 'visible': (rng.random((n, T)) < 0.8).astype(np.float32),
                  'depth': (rng.random((T, H, W, 1)) + 0.5).astype(np.float32), 'dino_map': rng.standard_normal((T, 3, 2, 6)).astype(np.float32), 'video_shape': (T, H, W, 3)})
  return clips


def test_model_score_and_train_step_take_the_dict():
  import spa3d
  cfg = O.Config(**MINI, use_dino=True, use_depth=True, dino_feature_dim=6, depth_feature_dim=2)
  model = product_model(spa3d, cfg, 'fp32')
  clips = _mini_clips()
  np.random.seed(7)
  splits = [spa3d.draw_split(14, 8, 4, 8), spa3d.draw_split(9, 5, 3, 5)]
  batch = spa3d.build_batch(clips, model=model, splits=splits)
  want = _composed(spa3d, clips, splits, 2, torch.float32, 8)
  _compare(batch, want)
  params = model.init(0, batch)['params']
  noise = torch.rand(2, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(2)).cuda()
  a = model.score({'params': params}, batch, thresholds=(0.5, 2.0), frame_errors=True, noise=noise)
  b = model.score({'params': params}, want, thresholds=(0.5, 2.0), frame_errors=True, noise=noise)
  _same(a.query_stats, b.query_stats, 'query_stats')
  _same(a.frame_err, b.frame_err, 'frame_err')
  assert torch.equal(a.sample_stats, b.sample_stats) and bool(torch.isfinite(a.query_stats).all()) and float(a.query_stats[0, 0, 7]) == 8.0
  st = spa3d.TrainState(model, params, learning_rate=1e-3, warmup_steps=0, total_steps=10)
  mt = st.train_step(batch, noise=noise)
  assert np.isfinite(float(mt['train/loss'])) and float(mt['train/loss']) > 0 and np.isfinite(float(mt['train/grad_norm']))


def test_drawn_splits_follow_the_seed():
  import spa3d
  cfg = O.Config(**MINI, use_dino=True, use_depth=True, dino_feature_dim=6, depth_feature_dim=2)
  model = product_model(spa3d, cfg, 'fp32')
  clips = _mini_clips()
  np.random.seed(9)
  drawn = spa3d.build_batch(clips, model=model, num_support_tracks=8, num_query_points=4)
  np.random.seed(9)
  splits = [spa3d.draw_split(14, 8, 4, 8), spa3d.draw_split(9, 8, 1, 5)]  # min(count, what the clip has): the second clip has 9 tracks
  _compare(drawn, spa3d.build_batch(clips, model=model, splits=splits))
  assert drawn['support_count'].tolist() == [8, 8] and drawn['query_count'].tolist() == [4, 1]


# ---------------------------------------------------------------------------------------------- 6. determinism
def test_two_calls_give_equal_bytes():
  import spa3d
  clips, splits = _ragged_inputs(768, seed=3)
  model = _model(spa3d, BATCH_T, 768, 3, 'bf16')
  a = spa3d.build_batch(clips, model=model, splits=splits)
  b = spa3d.build_batch(clips, model=model, splits=splits)
  _compare(a, b)
