"""The Python side of the score feature on the CPU (no compute call): TrackScores' derived properties against hand-made stats tensors, the
.npz layout of save_scores_npz, split_ragged on a TrackScores, and the refusals (CPU tensors, too many / bad thresholds)."""
import ctypes as C

import numpy as np
import pytest
import torch

from util import MINI, O, product_model


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


def _row(n_vis, s1, s2, mx, bce, occ, npv, T, per_k):
  return [n_vis, s1, s2, mx, bce, occ, npv, T] + [v for k in per_k for v in k]


def test_derived_properties_match_hand_made_stats(spa3d):
  # K = 2; rows: an ordinary row, a row without visible frames, a padded row (all zero)
  rows = [
      _row(4, 2.0, 1.0, 0.75, 6.0, 6, 5, 8, [(1, 1, 4, 3), (4, 3, 2, 1)]),
      _row(0, 0.0, 0.0, 0.0, 4.0, 8, 0, 8, [(0, 0, 0, 0), (0, 0, 0, 0)]),
      [0.0] * 16,
  ]
  qs = torch.tensor([rows], dtype=torch.float32)  # [1, 3, 16]
  ss = torch.tensor([[4, 2.0, 1.0, 0.75, 10.0, 14, 5, 16, 1, 1, 4, 3, 4, 3, 2, 1]], dtype=torch.float64)
  sc = spa3d.TrackScores(qs, ss, None, (0.1, 0.5))
  eq = lambda a, b: torch.testing.assert_close(a.double(), torch.tensor(b, dtype=torch.float64), rtol=1e-6, atol=0)
  eq(sc.position_l1, [[0.5, 0.0, 0.0]])
  eq(sc.distance_mean, [[0.25, 0.0, 0.0]])
  eq(sc.distance_max, [[0.75, 0.0, 0.0]])
  eq(sc.occlusion_accuracy, [[0.75, 1.0, 0.0]])  # the padded row's denominator (slot 7 = 0) is clamped at 1
  eq(sc.visible_bce, [[0.75, 0.5, 0.0]])
  eq(sc.pts_within, [[[0.25, 1.0], [0.0, 0.0], [0.0, 0.0]]])
  eq(sc.jaccard, [[[1 / 8, 3 / 6], [0.0, 0.0], [0.0, 0.0]]])
  eq(sc.average_jaccard, [[(1 / 8 + 3 / 6) / 2, 0.0, 0.0]])
  assert sc.pts_within.shape == (1, 3, 2) and sc.jaccard.shape == (1, 3, 2)
  s = sc.sample  # the same per sample, from the pooled counts
  eq(s.position_l1, [0.5])
  eq(s.distance_mean, [0.25])
  eq(s.distance_max, [0.75])
  eq(s.occlusion_accuracy, [14 / 16])
  eq(s.pts_within, [[0.25, 1.0]])
  eq(s.jaccard, [[1 / 8, 0.5]])
  eq(s.average_jaccard, [(1 / 8 + 0.5) / 2])
  assert s.stats.dtype == torch.float64 and s.thresholds == (0.1, 0.5)
  # K = 0: no per-threshold columns, the averages read 0
  sc0 = spa3d.TrackScores(qs[..., :8], ss[..., :8], None, ())
  assert sc0.pts_within.shape == (1, 3, 0) and sc0.jaccard.shape == (1, 3, 0)
  eq(sc0.average_jaccard, [[0.0, 0.0, 0.0]])
  eq(sc0.position_l1, [[0.5, 0.0, 0.0]])
  with pytest.raises(ValueError):
    spa3d.TrackScores(qs, None, None, (0.1, 0.5)).sample


def test_split_ragged_cuts_track_scores(spa3d):
  B, Q, T, S = 3, 5, 4, 12
  qs = torch.arange(B * Q * S, dtype=torch.float32).reshape(B, Q, S)
  ss = torch.arange(B * S, dtype=torch.float64).reshape(B, S)
  fe = torch.arange(B * Q * T, dtype=torch.float32).reshape(B, Q, T)
  preds = spa3d.TrackAutoEncoderResults(torch.zeros(B, Q, T, 3), torch.ones(B, Q, T, 1), torch.zeros(B, Q, T, 1))
  sc = spa3d.TrackScores(qs, ss, fe, (0.5,), preds)
  parts = spa3d.split_ragged(sc, {'query_count': torch.tensor([5, 0, 2])})
  assert [p.query_stats.shape[0] for p in parts] == [5, 0, 2]
  for i, p in enumerate(parts):
    q = [5, 0, 2][i]
    assert isinstance(p, spa3d.TrackScores) and p.thresholds == (0.5,)
    assert torch.equal(p.query_stats, qs[i, :q]) and torch.equal(p.sample_stats, ss[i]) and torch.equal(p.frame_err, fe[i, :q])
    assert p.predictions.tracks.shape == (q, T, 3) and p.predictions.visible_logits.shape == (q, T, 1)
    assert p.position_l1.shape == (q,) and p.sample.position_l1.shape == ()
  whole = spa3d.split_ragged(spa3d.TrackScores(qs, ss, None, (0.5,)), {})
  assert [p.query_stats.shape[0] for p in whole] == [Q] * B and all(p.frame_err is None and p.predictions is None for p in whole)
  # the existing behaviour on prediction objects is untouched
  d = spa3d.split_ragged(preds, {'query_count': [1, 2, 3]})
  assert [x['tracks'].shape[0] for x in d] == [1, 2, 3]


def test_save_scores_npz_layout(spa3d, tmp_path):
  N, T = 6, 9
  coords = torch.arange(N * T * 3, dtype=torch.float32).reshape(N, T, 3)
  scores = torch.arange(N * T, dtype=torch.float32).reshape(N, T)
  visibs = (torch.arange(N * T).reshape(N, T, 1) % 2).float()
  video = np.zeros((T, 4, 5, 3), np.uint8)
  path = str(tmp_path / 'scores.npz')
  spa3d.save_scores_npz(path, coords, scores, visibs, video=video, intrinsics=np.eye(3, dtype=np.float32), extrinsics=torch.eye(4).repeat(T, 1, 1))
  z = np.load(path)
  assert sorted(z.files) == ['coords', 'coords_score', 'extrinsics', 'intrinsics', 'video', 'visibs']
  assert z['coords'].shape == (T, N, 3) and z['coords_score'].shape == (T, N) and z['visibs'].shape == (T, N)  # time-major
  assert np.array_equal(z['coords'], coords.numpy().transpose(1, 0, 2)) and np.array_equal(z['coords_score'], scores.numpy().T)
  assert z['visibs'].dtype == np.bool_ and np.array_equal(z['visibs'], visibs.numpy()[..., 0].T > 0.5)
  assert z['video'].shape == (T, 4, 5, 3) and z['intrinsics'].shape == (3, 3) and z['extrinsics'].shape == (T, 4, 4)
  with pytest.raises(ValueError):
    spa3d.save_scores_npz(path, coords, scores[:, :-1], visibs)
  with pytest.raises(ValueError):
    spa3d.save_scores_npz(path, coords, scores, visibs, coords_score=scores)


def test_cpu_tensors_and_bad_thresholds_are_refused(spa3d):
  cfg = O.Config(**MINI, use_dino=False, use_depth=False)
  model = product_model(spa3d, cfg, 'fp32')
  batch = O.synthetic_batch(2, 4, 3, 8)
  _, _, n = model._handle(0, 0)
  params = model.tree_from_flat(torch.zeros(n), 0, 0)
  with pytest.raises(spa3d._lib.Spa3dError):
    model.score({'params': params}, batch, thresholds=(0.1,))
  preds = spa3d.TrackAutoEncoderResults(torch.zeros(2, 3, 8, 3), torch.zeros(2, 3, 8, 1), torch.zeros(2, 3, 8, 1))
  with pytest.raises(spa3d._lib.Spa3dError):
    spa3d.score_predictions(preds, batch, thresholds=(0.1,))
  with pytest.raises(ValueError):
    model.score({'params': params}, batch, thresholds=[0.01 * (i + 1) for i in range(9)])
  with pytest.raises(ValueError):
    spa3d.score_predictions(preds, batch, thresholds=[0.01 * (i + 1) for i in range(9)])
  for bad in ((0.0,), (-1.0,), (float('nan'),), (float('inf'),)):
    with pytest.raises(ValueError):
      model.score({'params': params}, batch, thresholds=bad)
  two_d = spa3d.TrackAutoEncoder(num_output_frames=8, precision='fp32')
  assert callable(two_d.score)


def test_scores_struct_matches_the_header(spa3d):
  """spa3d_scores as ctypes lays it out: int32, 8 floats, then four 8-byte pointers at offset 40."""
  S = spa3d._lib.Scores
  assert S.num_thresholds.offset == 0 and S.thresholds.offset == 4 and S.thresholds.size == 32
  assert (S.sample_scale.offset, S.query_stats.offset, S.sample_stats.offset, S.frame_err.offset) == (40, 48, 56, 64) and C.sizeof(S) == 72
  lib = spa3d._lib.load()
  m = spa3d.TrackAutoEncoder3D(num_output_frames=8, use_dino=False, use_depth=False, precision='fp32')
  h = m._handle(0, 0)[0]
  b = spa3d._lib.Batch()
  b.B, b.Q = 1, 1
  sc = S()
  sc.num_thresholds = 9
  out = spa3d._lib.Outputs()
  assert lib.spa3d_score_from_preds(h, C.byref(b), C.byref(out), C.byref(sc), None) == 1 and b'targets' in lib.spa3d_last_error(h)
  b.query_tracks, b.query_tracks_visible = 0x100000, 0x100000  # never dereferenced: the call is refused before any launch
  assert lib.spa3d_score_from_preds(h, C.byref(b), C.byref(out), C.byref(sc), None) == 1 and b'query_stats' in lib.spa3d_last_error(h)
  sc.query_stats = 0x100000
  assert lib.spa3d_score_from_preds(h, C.byref(b), C.byref(out), C.byref(sc), None) == 1 and b'num_thresholds' in lib.spa3d_last_error(h)
  sc.num_thresholds = 2
  sc.thresholds[0], sc.thresholds[1] = 0.5, -0.5
  assert lib.spa3d_score_from_preds(h, C.byref(b), C.byref(out), C.byref(sc), None) == 1 and b'thresholds[1]' in lib.spa3d_last_error(h)
