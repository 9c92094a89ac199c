"""Host side of build_batch (3dspa_code_amd/data.py), no GPU: draw_split makes the RNG calls of prepare_3d_batch, so with one seed both pick the
same tracks and frames; and everything build_batch can refuse is refused on the host, before any device call (there is no device here)."""
import numpy as np
import pytest
import torch

import spa3d

N, T, H, W, D = 12, 6, 20, 30, 8


def test_draw_split_picks_what_prepare_3d_batch_picks():
  tracks = np.broadcast_to(np.arange(40, dtype=np.float32)[:, None, None], (40, 9, 3)).copy()  # a track's coordinates are its index
  tracks[..., 1] = np.arange(9, dtype=np.float32)[None]                                         # and y is the frame
  example = {'tracks_3d': tracks, 'visible': np.ones((40, 9, 1), np.float32)}
  for seed, (ns, nq) in enumerate([(16, 8), (30, 10), (1, 39), (39, 1)]):
    np.random.seed(seed)
    b = spa3d.prepare_3d_batch(example, num_support_tracks=ns, num_query_tracks=nq, num_frames=9, device='cpu')
    np.random.seed(seed)
    si, qi, qf = spa3d.draw_split(40, ns, nq, 9)
    assert np.array_equal(b['support_tracks'][0, :, 0, 0].numpy(), si.astype(np.float32))
    assert np.array_equal(b['query_tracks'][0, :, 0, 0].numpy(), qi.astype(np.float32))
    assert np.array_equal(b['query_points'][0, :, 0].numpy(), qf.astype(np.float32)) and np.array_equal(b['query_points'][0, :, 2].numpy(), qf.astype(np.float32))
    assert len(si) == ns and len(qi) == nq == len(qf) and len(set(si) | set(qi)) == ns + nq
    # and the generator is left in the same state
    state = np.random.get_state()[1].copy()
    np.random.seed(seed)
    spa3d.prepare_3d_batch(example, num_support_tracks=ns, num_query_tracks=nq, num_frames=9, device='cpu')
    assert np.array_equal(state, np.random.get_state()[1])


def test_draw_split_without_queries():
  np.random.seed(3)
  si, qi, qf = spa3d.draw_split(40, 40, 0, 9)
  np.random.seed(3)
  assert np.array_equal(si, np.random.permutation(40)) and len(qi) == 0 and len(qf) == 0


def test_draw_split_raises_index_error_on_a_small_clip():
  for total, ns, nq in ((10, 8, 3), (10, 11, 0), (0, 1, 0)):
    with pytest.raises(IndexError):
      spa3d.draw_split(total, ns, nq, 5)
    example = {'tracks_3d': np.zeros((total, 5, 3), np.float32), 'visible': np.zeros((total, 5, 1), np.float32)}
    if nq:
      with pytest.raises(IndexError):
        spa3d.prepare_3d_batch(example, num_support_tracks=ns, num_query_tracks=nq, num_frames=5, device='cpu')


def _model(**kw):
  return spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=D, depth_feature_dim=3, precision='bf16', **kw)


def _clip(rng=None, **over):
  rng = rng or np.random.default_rng(0)
  c = {'tracks_2d': rng.random((N, T, 2)).astype(np.float32) * 10, 'visible': np.ones((N, T), np.float32), 'depth': np.ones((T, H, W, 1), np.float32),
       'dino_map': rng.standard_normal((T, 2, 3, D)).astype(np.float32), 'video_shape': (T, H, W, 3)}
  c.update(over)
  return {k: v for k, v in c.items() if v is not None}


SPLIT = (np.arange(5), np.array([6, 7]), np.array([0, T - 1]))


def _refused(clips, exc=ValueError, match=None, **kw):
  kw.setdefault('model', _model())
  kw.setdefault('splits', [SPLIT] * len(clips))
  with pytest.raises(exc, match=match):
    spa3d.build_batch(clips, **kw)


def test_a_valid_call_gets_past_the_host_checks_and_only_then_asks_for_the_device():
  """The positive control of the refusals below: the same clip and split, unchanged, pass every host check; what stops the call here is the
  device alone (a CPU device is refused loudly, there is no fallback)."""
  with pytest.raises(spa3d._lib.Spa3dError, match='HIP-only'):
    spa3d.build_batch([_clip()], model=_model(), splits=[SPLIT], device='cpu')


def test_host_refusals():
  _refused([], match='at least one clip')
  _refused([_clip()], model=None, match='needs the model')
  _refused([_clip()], model=spa3d.TrackAutoEncoder(num_output_frames=T), match='2-D model')
  _refused([_clip()], splits=[SPLIT, SPLIT], match='one entry per clip')
  # missing inputs
  _refused([_clip(tracks_2d=None)], match='tracks_2d and visible')
  _refused([_clip(visible=None)], match='tracks_2d and visible')
  _refused([_clip(depth=None)], match='depth to lift')                                   # a lift without a depth map
  _refused([_clip(video_shape=None, depth=None, tracks_3d=np.zeros((N, T, 3), np.float32))], match='frame size')   # a map without the video size
  # shapes
  _refused([_clip(visible=np.ones((N, T + 1), np.float32))], match='visible must be')
  _refused([_clip(tracks_3d=np.zeros((N, T, 2), np.float32))], match='tracks_3d must be')
  _refused([_clip(depth=np.ones((T + 1, H, W), np.float32))], match='depth must be')
  _refused([_clip(dino_map=np.zeros((T, 2, 3), np.float32))], match='dino_map must be')
  _refused([_clip(dino_map=None, dino_features=np.zeros((N + 1, T, D), np.float32))], match='dino_features must be')
  _refused([_clip(depth_features=np.zeros((N, T), np.float32))], match='depth_features must be')
  _refused([_clip(video_shape=(T, H + 1, W, 3))], match='disagree')
  _refused([_clip(intrinsics=(1.0, 2.0, 3.0))], match='intrinsics')
  # a clip longer than the batch
  _refused([_clip()], num_frames=T - 1, match='frames')
  # a map and a pool for one feature
  _refused([_clip(dino_features=np.zeros((N, T, D), np.float32))], match='dino_map and dino_features are both given')
  _refused([_clip(tracks_3d=np.zeros((N, T, 3), np.float32), depth_features=np.zeros((N, T, 3), np.float32))], match='depth and depth_features are both given')
  # a feature the model does not have / clips that disagree
  _refused([_clip(dino_map=np.zeros((T, 2, 3, D + 4), np.float32))], match='dino_feature_dim')
  _refused([_clip(), _clip(dino_map=None)], match='same features')
  _refused([_clip(), _clip(depth_features=np.zeros((N, T, 2), np.float32))], match='same features')
  # counts: no support track, more frames than queries
  _refused([_clip()], splits=[(np.array([], np.int64), np.array([1]), np.array([0]))], match='at least one support track')
  _refused([_clip()], splits=[(np.arange(3), np.array([4, 5]), np.array([0]))], match='query frames')
  _refused([_clip()], splits=[(np.arange(3), np.array([4, 5]))], match='split is')
  # every index and frame is validated on the host
  for bad_split, word in (((np.array([0, N]), np.array([1]), np.array([0])), 'support_index'), ((np.array([-1]), np.array([1]), np.array([0])), 'support_index'),
                          ((np.array([0]), np.array([N]), np.array([0])), 'query_index'), ((np.array([0]), np.array([-3]), np.array([0])), 'query_index'),
                          ((np.array([0]), np.array([1]), np.array([T])), 'query_frame'), ((np.array([0]), np.array([1]), np.array([-1])), 'query_frame'),
                          ((np.array([0.5]), np.array([1]), np.array([0])), 'integers'), ((np.array([[0]]), np.array([1]), np.array([0])), 'one-dimensional'),
                          ((torch.tensor([0, 99]), torch.tensor([1]), torch.tensor([0])), 'support_index')):
    _refused([_clip()], splits=[bad_split], match=word)
  # a shorter clip: its frames are validated against ITS length, not the batch's
  short = _clip(tracks_2d=np.zeros((N, T - 2, 2), np.float32), visible=np.ones((N, T - 2), np.float32), depth=np.ones((T - 2, H, W), np.float32),
                dino_map=np.zeros((T - 2, 2, 3, D), np.float32), video_shape=(T - 2, H, W, 3))
  _refused([short], splits=[(np.array([0]), np.array([1]), np.array([T - 2]))], match='query_frame')
  # a drawn split on a clip that is too small for even one support track cannot happen (min(count, what the clip has)); a negative count is refused
  _refused([_clip()], splits=None, num_support_tracks=0, match='positive')
