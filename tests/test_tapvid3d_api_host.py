"""The Python side of the TAPVid-3D metrics on the CPU (no compute call): TapVid3DScores' derived properties and as_dict against hand-made
counts, the aggregation of evaluate_tapvid3d against a hand-computed mean and standard deviation, split_ragged on a TapVid3DScores, the
ctypes layout of spa3d_tapvid3d, and the refusals (CPU tensors, unknown scaling, wrong shapes, the library's own argument checks)."""
import ctypes as C

import numpy as np
import pytest
import torch

import tapvid3d_util as TU
from util import MINI, O, product_model


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


#        ew vis occ pv | (W, TP, FP, FN) at 1, 2, 4, 8, 16 px
ROW_A = [9, 6, 7, 5, 1, 1, 4, 5, 2, 2, 3, 4, 3, 2, 3, 4, 4, 3, 2, 3, 6, 4, 1, 2]
ROW_B = [9, 0, 5, 4, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0, 4, 0]  # nothing visible
ROW_0 = [0] * 24                                                                   # a padded row


def _scores(spa3d):
  qs = torch.tensor([[ROW_A, ROW_B, ROW_0]], dtype=torch.float32)
  ss = qs.double().sum(1)
  return spa3d.TapVid3DScores(qs, ss, torch.ones(1), torch.ones(1, 3), None, 'median', False)


def test_derived_properties_and_as_dict_match_hand_made_counts(spa3d):
  sc = _scores(spa3d)
  eq = lambda a, b: torch.testing.assert_close(a.double(), torch.tensor(b, dtype=torch.float64), rtol=1e-6, atol=0)
  eq(sc.occlusion_accuracy, [[7 / 9, 5 / 9, 0.0]])
  eq(sc.pts_within, [[[1 / 6, 2 / 6, 3 / 6, 4 / 6, 1.0], [0.0] * 5, [0.0] * 5]])
  eq(sc.jaccard, [[[1 / 10, 2 / 9, 2 / 9, 3 / 8, 4 / 7], [0.0] * 5, [0.0] * 5]])
  eq(sc.average_jaccard, [[(1 / 10 + 2 / 9 + 2 / 9 + 3 / 8 + 4 / 7) / 5, 0.0, 0.0]])
  eq(sc.average_pts_within_thresh, [[(1 + 2 + 3 + 4 + 6) / 30, 0.0, 0.0]])
  s = sc.sample  # pooled: ew 18, vis 6, occ 12, pv 9; FP = 8, 7, 7, 6, 5
  assert s.stats.dtype == torch.float64 and s.scaling == 'median'
  eq(s.occlusion_accuracy, [12 / 18])
  eq(s.pts_within, [[1 / 6, 2 / 6, 3 / 6, 4 / 6, 1.0]])
  eq(s.jaccard, [[1 / 14, 2 / 13, 2 / 13, 3 / 12, 4 / 11]])
  d = sc.as_dict(0)
  assert list(d) == TU.KEYS and len(d) == 13
  want = TU.metrics(sc.sample_stats[0].numpy())
  assert all(isinstance(v, float) for v in d.values())
  assert d == pytest.approx(want, rel=1e-12)
  assert d['jaccard_16'] == pytest.approx(4 / 11) and d['occlusion_accuracy'] == pytest.approx(2 / 3)
  assert d['average_pts_within_thresh'] == pytest.approx((1 + 2 + 3 + 4 + 6) / 30)


def test_aggregation_is_mean_and_population_std_over_clips(spa3d):
  clips = [{'occlusion_accuracy': 0.5, 'average_jaccard': 0.2}, {'occlusion_accuracy': 1.0, 'average_jaccard': 0.4}, {'occlusion_accuracy': 0.75, 'average_jaccard': 0.9}]
  a = spa3d.aggregate_tapvid3d(clips)
  assert list(a) == ['occlusion_accuracy', 'occlusion_accuracy_std', 'average_jaccard', 'average_jaccard_std']
  assert a['occlusion_accuracy'] == pytest.approx(0.75) and a['occlusion_accuracy_std'] == pytest.approx((((0.25 ** 2) * 2 + 0.0) / 3) ** 0.5)
  assert a['average_jaccard'] == pytest.approx(0.5) and a['average_jaccard_std'] == pytest.approx(((0.09 + 0.01 + 0.16) / 3) ** 0.5)
  for k in ('occlusion_accuracy', 'average_jaccard'):  # np.mean / np.std as evaluate_tapvid3d.py:241-242
    assert a[k] == pytest.approx(np.mean([c[k] for c in clips])) and a[k + '_std'] == pytest.approx(np.std([c[k] for c in clips]))
  assert spa3d.aggregate_tapvid3d([]) == {}

  class FakeModel:  # evaluate_tapvid3d: every clip of every batch is one video, per scaling
    def __init__(self):
      self.calls = []

    def tapvid3d(self, variables, batch, scalings, fixed_thresholds=False):
      self.calls.append((batch['id'], scalings, fixed_thresholds))
      out = {}
      for s in scalings:
        rows = torch.tensor(batch['rows'], dtype=torch.float64) * (2 if s == 'none' else 1)
        out[s] = spa3d.TapVid3DScores(torch.zeros(rows.shape[0], 1, 24), rows, torch.ones(rows.shape[0]), torch.ones(rows.shape[0], 1), None, s, False)
      return out

  m = FakeModel()
  batches = [{'id': 0, 'rows': [ROW_A, ROW_B]}, {'id': 1, 'rows': [ROW_A]}]
  r = spa3d.evaluate_tapvid3d(m, {}, batches, depth_scalings=('median', 'none'))
  assert m.calls == [(0, ('median', 'none'), False), (1, ('median', 'none'), False)] and list(r) == ['median', 'none']
  per = [TU.metrics(ROW_A), TU.metrics(ROW_B), TU.metrics(ROW_A)]
  assert len(r['median']) == 26
  for k in TU.KEYS:
    assert r['median'][k] == pytest.approx(np.mean([c[k] for c in per])) and r['median'][k + '_std'] == pytest.approx(np.std([c[k] for c in per]))
    assert r['none'][k] == pytest.approx(r['median'][k])  # ratios of counts: doubling every count changes nothing
  with pytest.raises(ValueError):
    spa3d.evaluate_tapvid3d(m, {}, batches, depth_scalings=('local_neighborhood',))


def test_split_ragged_cuts_tapvid3d_scores(spa3d):
  B, Q, T = 3, 5, 4
  qs = torch.arange(B * Q * 24, dtype=torch.float32).reshape(B, Q, 24)
  sc = spa3d.TapVid3DScores(qs, qs.double().sum(1), torch.arange(B, dtype=torch.float32), torch.arange(B * Q, dtype=torch.float32).reshape(B, Q),
                            torch.arange(B * Q * T, dtype=torch.float32).reshape(B, Q, T), 'per_trajectory', True)
  parts = spa3d.split_ragged(sc, {'query_count': torch.tensor([5, 0, 2])})
  for i, (p, q) in enumerate(zip(parts, [5, 0, 2])):
    assert isinstance(p, spa3d.TapVid3DScores) and p.scaling == 'per_trajectory' and p.fixed_thresholds is True
    assert torch.equal(p.query_stats, qs[i, :q]) and torch.equal(p.sample_stats, sc.sample_stats[i]) and p.scale == i
    assert torch.equal(p.row_scale, sc.row_scale[i, :q]) and torch.equal(p.ratio, sc.ratio[i, :q])
    assert p.jaccard.shape == (q, 5) and p.sample.jaccard.shape == (5,)
    assert p.as_dict() == sc.as_dict(i)
  assert [p.query_stats.shape[0] for p in spa3d.split_ragged(sc, {})] == [Q] * B


def test_cpu_tensors_and_bad_arguments_are_refused(spa3d):
  preds = spa3d.TrackAutoEncoderResults(torch.zeros(2, 3, 8, 3), torch.zeros(2, 3, 8, 1), torch.zeros(2, 3, 8, 1))
  batch = O.synthetic_batch(2, 4, 3, 8)
  with pytest.raises(spa3d._lib.Spa3dError):
    spa3d.tapvid3d_predictions(preds, batch)
  for bad in ('local_neighborhood', 'Median', None, 1):
    with pytest.raises(ValueError):
      spa3d.tapvid3d_predictions(preds, batch, scaling=bad)
  cfg = O.Config(**MINI, use_dino=False, use_depth=False)
  model = product_model(spa3d, cfg, 'fp32')
  _, _, n = model._handle(0, 0)
  params = model.tree_from_flat(torch.zeros(n), 0, 0)
  with pytest.raises(ValueError):  # before any forward pass
    model.tapvid3d({'params': params}, batch, scalings=('median', 'nearest'))
  with pytest.raises(spa3d._lib.Spa3dError):
    model.tapvid3d({'params': params}, batch)


def test_struct_matches_the_header_and_the_library_refuses(spa3d):
  """spa3d_tapvid3d as ctypes lays it out (two int32, then six 8-byte pointers) and every refusal of the entry point, none of which launches."""
  S = spa3d._lib.TapVid3D
  assert (S.scaling.offset, S.fixed_thresholds.offset, S.intrinsics.offset, S.query_stats.offset, S.sample_stats.offset, S.scale.offset,
          S.row_scale.offset, S.ratio.offset) == (0, 4, 8, 16, 24, 32, 40, 48) and C.sizeof(S) == 56
  lib = spa3d._lib.load()
  h = spa3d.TrackAutoEncoder3D(num_output_frames=8, use_dino=False, use_depth=False, precision='fp32')._handle(0, 0)[0]
  fake = 0x100000  # never dereferenced: every call below is refused before its first launch
  b = spa3d._lib.Batch()
  b.B, b.Q = 2, 3
  out, m = spa3d._lib.Outputs(), S()
  call = lambda ws_bytes=0: lib.spa3d_tapvid3d_from_preds(h, C.byref(b), C.byref(out), C.byref(m), fake, ws_bytes, None)
  assert call() == 1 and b'targets' in lib.spa3d_last_error(h)
  b.query_tracks, b.query_tracks_visible = fake, fake
  assert call() == 1 and b'query_points' in lib.spa3d_last_error(h)
  b.query_points = fake
  assert call() == 1 and b'predictions' in lib.spa3d_last_error(h)
  out.tracks, out.visible_logits = fake, fake
  assert call() == 1 and b'query_stats' in lib.spa3d_last_error(h)
  m.query_stats = fake
  for bad in (-1, 3):
    m.scaling = bad
    assert call() == 1 and b'scaling' in lib.spa3d_last_error(h)
  m.scaling = 1
  need = lib.spa3d_tapvid3d_workspace_bytes(h, 2, 3, 8)
  assert need > 0 and call(0) == 1 and b'workspace too small' in lib.spa3d_last_error(h)
  asked = int(lib.spa3d_last_error(h).split(b'need ')[1].split()[0])
  assert 2 * 3 * 8 * 4 <= asked <= need
  assert lib.spa3d_tapvid3d_workspace_bytes(h, 0, 3, 8) == -1 and lib.spa3d_tapvid3d_workspace_bytes(None, 2, 3, 8) == -1
  two_d = spa3d.TrackAutoEncoder(num_output_frames=8, precision='fp32')._handle(0, 0)[0]
  m.scaling = 1
  assert lib.spa3d_tapvid3d_from_preds(two_d, C.byref(b), C.byref(out), C.byref(m), fake, 1 << 20, None) == 1 and b'model_kind 1' in lib.spa3d_last_error(two_d)
  assert lib.spa3d_tapvid3d_from_preds(None, C.byref(b), C.byref(out), C.byref(m), fake, 1 << 20, None) == 1
  assert lib.spa3d_op_median_rows(None, 1, 1, fake, None, 0, None) == 1 and lib.spa3d_op_median_rows(fake, 0, 1, fake, None, 0, None) == 1
