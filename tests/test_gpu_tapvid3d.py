"""TAPVid-3D metrics on the GPU (include/spa3d.h: spa3d_tapvid3d_from_preds, spa3d_op_median_rows; tapvid3d_predictions, TrackAutoEncoder3D.tapvid3d).

  1. spa3d_op_median_rows: exact against NumPy on ties, values that differ in their lowest mantissa bits only, 40 binades, and rows of
     n = 1, 63, 64, 65, 4097 and 76 800 with about 15 % NaN; several rows in one launch; two runs bit-equal.
  2. tapvid3d_predictions on generator data (tests/tapvid3d_util.py, no model): four shapes, three scalings, depth-dependent and fixed
     thresholds, default and explicit intrinsics, under the util's rules; a ragged batch with a query-less sample and NaN in everything
     padded; a sample without a visible frame.
  3. Model level (MINI, fp32 and bf16): model.tapvid3d equals tapvid3d_predictions(model.apply(...)) bit for bit, two runs are bit-equal, and
     with scaling 'none' and fixed thresholds the pooled counts equal spa3d_score's at the same thresholds once the query frames are taken
     out of both."""
import ctypes as C

import numpy as np
import pytest
import torch

import tapvid3d_util as TU
from util import MINI, O, batch_to, product_model

pytestmark = pytest.mark.gpu
FIELDS = ('query_stats', 'sample_stats', 'scale', 'row_scale', 'ratio')


def _median(spa3d, x, rows, n):
  xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda() if x.size else torch.zeros(1, device='cuda')
  out = torch.full((rows,), -7.0, device='cuda')
  rc = spa3d._lib.load().spa3d_op_median_rows(xt.data_ptr(), rows, n, out.data_ptr(), None, 0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
  assert rc == 0
  return out.cpu().numpy()


def test_median_rows_is_the_exact_median():
  import spa3d
  cases = {k: v for k, v in TU.median_cases().items() if k != 'zero and tiny'}  # (subnormals: the host test's business)
  rng = np.random.default_rng(17)
  for n in (1, 63, 64, 65, 4097, 76800):
    x = (1.3 * 2.0 ** rng.normal(0.0, 0.3, n)).astype(np.float32)
    x[rng.random(n) < 0.15] = np.nan
    cases[f'n = {n}, 15 % NaN'] = x
  for name, x in cases.items():
    got = _median(spa3d, x, 1, x.size)
    want = TU.median32(x)
    print(f'  median {name}: n {x.size}, non-NaN {int((~np.isnan(x)).sum())}: {got[0]!r} (NumPy {want!r})')
    assert got[0].tobytes() == np.float32(want).tobytes(), name
    assert _median(spa3d, x, 1, x.size).tobytes() == got.tobytes(), f'{name}: two runs differ'
  rows = np.stack([np.roll(cases['n = 4097, 15 % NaN'], 7 * r) * np.float32(1 + r) for r in range(5)])  # several rows, one launch
  rows[3] = np.nan
  got = _median(spa3d, rows, 5, 4097)
  assert got.tobytes() == np.array([TU.median32(r) for r in rows], np.float32).tobytes() and got[3] == 1.0


def _torch_inputs(spa3d, d):
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
  preds = spa3d.TrackAutoEncoderResults(t(d['p']), t(d['l'][..., None]), torch.zeros_like(t(d['l'][..., None])))
  batch = {'query_tracks': t(d['g']), 'query_tracks_visible': t(d['y'][..., None]), 'query_points': t(d['qp'])}
  return preds, batch


def _np(sc):
  return {k: getattr(sc, k).cpu().numpy() for k in FIELDS}


def _bit_equal(a, b, what):
  for k in FIELDS:
    x, y = getattr(a, k), getattr(b, k)
    assert (x is None) == (y is None) and (x is None or (x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else torch.int64),
                                                                                                                  y.view(torch.int32 if y.dtype == torch.float32 else torch.int64)))), f'{what}: {k} differs'


INTRINSICS = np.array([[300.0, 280.0, 160.0, 120.0], [200.0, 210.0, 100.0, 100.0], [256.0, 256.0, 128.0, 128.0]], np.float32)


@pytest.mark.parametrize('shape', [(3, 96, 24), (3, 37, 70), (3, 37, 150), (2, 512, 150)])
def test_predictions_on_generator_data(shape):
  import spa3d
  B, Q, T = shape
  d = TU.generate(B, Q, T)
  preds, batch = _torch_inputs(spa3d, d)
  for scaling in ('none', 'median', 'per_trajectory'):
    for fixed, k in ((False, None), (False, INTRINSICS[:B]), (True, None)):
      what = f'gpu {shape} {scaling} fixed={fixed} intrinsics={"given" if k is not None else "default"}'
      sc = spa3d.tapvid3d_predictions(preds, batch, scaling=scaling, intrinsics=k, fixed_thresholds=fixed, ratios=True)
      TU.check_call(d, _np(sc), scaling, k, fixed, what=what)
      _bit_equal(spa3d.tapvid3d_predictions(preds, batch, scaling=scaling, intrinsics=k, fixed_thresholds=fixed, ratios=True), sc, f'{what}: second run')
      lean = spa3d.tapvid3d_predictions(preds, batch, scaling=scaling, intrinsics=k, fixed_thresholds=fixed)  # without the ratio output
      assert lean.ratio is None and all(torch.equal(getattr(lean, f), getattr(sc, f)) for f in FIELDS[:4]), what
      if scaling == 'median':
        assert np.allclose(sc.scale.cpu().numpy(), d['s_b'], rtol=0.02)
        if not fixed:  # every threshold cuts the data: the generator aims at 0.25 / 0.38 / 0.50 / 0.63 / 0.75
          w = sc.sample.pts_within.cpu().numpy()
          print(f'  {what}: pts_within {np.round(w, 3).tolist()} average_jaccard {sc.sample.average_jaccard.tolist()}')
          assert (np.diff(w, axis=1) > 0.05).all() and 0.15 < w[:, 0].min() and w[:, 4].max() < 0.85
      for b in range(B):
        assert sc.as_dict(b) == pytest.approx(TU.metrics(sc.sample_stats[b].cpu().numpy()), rel=1e-12)
  one = spa3d.tapvid3d_predictions(preds, batch, scaling='median', intrinsics=INTRINSICS[0])  # one [4] row for every clip
  assert torch.equal(one.query_stats, spa3d.tapvid3d_predictions(preds, batch, scaling='median', intrinsics=np.tile(INTRINSICS[0], (B, 1))).query_stats)


def test_ragged_batch_with_a_query_less_sample_and_nan_padding():
  import spa3d
  B, Q, T = 3, 37, 70
  counts = [37, 0, 5]
  d = TU.generate(B, Q, T)
  clean = {k: v.copy() for k, v in d.items()}
  for b, n in enumerate(counts):  # everything the library must not read
    for k in ('p', 'l', 'g', 'y', 'qp'):
      d[k][b, n:] = np.nan
  preds, batch = _torch_inputs(spa3d, d)
  batch['query_count'] = torch.tensor(counts, dtype=torch.int32)
  cpreds, cbatch = _torch_inputs(spa3d, clean)
  for scaling in ('none', 'median', 'per_trajectory'):
    sc = spa3d.tapvid3d_predictions(preds, batch, scaling=scaling, ratios=True)
    out = _np(sc)
    assert all(np.isfinite(v).all() for v in out.values()), f'{scaling}: a padded NaN reached a result'
    TU.check_call(d, out, scaling, counts=counts, what=f'gpu ragged {scaling}')  # (padded rows all zero: checked there)
    assert out['scale'][1] == 1.0 and not out['sample_stats'][1].any()
    assert all(v == 0.0 for v in sc.as_dict(1).values())
    full = spa3d.tapvid3d_predictions(cpreds, cbatch, scaling=scaling, ratios=True)  # the batch without counts: sample 0 is whole in both
    for f in FIELDS:
      assert torch.equal(getattr(sc, f)[0], getattr(full, f)[0]), f'{scaling}: {f} of the whole sample differs from the uniform call'
    crop = lambda t: t[2:3, :5].contiguous()
    alone = spa3d.tapvid3d_predictions(spa3d.TrackAutoEncoderResults(crop(cpreds.tracks), crop(cpreds.visible_logits), crop(cpreds.certain_logits)),
                                       {k: crop(v) for k, v in cbatch.items()}, scaling=scaling, ratios=True)
    assert torch.equal(alone.query_stats[0], sc.query_stats[2, :5]) and torch.equal(alone.scale[0], sc.scale[2]) and torch.equal(alone.sample_stats[0], sc.sample_stats[2])
    parts = spa3d.split_ragged(sc, batch)
    assert [p.query_stats.shape[0] for p in parts] == counts and parts[2].as_dict() == sc.as_dict(2)


def test_sample_without_a_visible_frame():
  import spa3d
  d = TU.generate(2, 9, 70)
  d['y'][1] = 0.0
  preds, batch = _torch_inputs(spa3d, d)
  for scaling in ('none', 'median', 'per_trajectory'):
    sc = spa3d.tapvid3d_predictions(preds, batch, scaling=scaling, ratios=True)
    TU.check_call(d, _np(sc), scaling, what=f'gpu no visible frame {scaling}')
    m = sc.as_dict(1)
    assert float(sc.scale[1]) == 1.0 and float(sc.sample_stats[1, 1]) == 0.0 and not sc.sample_stats[1, 4::4].any() and not sc.sample_stats[1, 5::4].any()
    assert all(m[k] == 0.0 for k in TU.KEYS if k != 'occlusion_accuracy') and 0.0 < m['occlusion_accuracy'] < 1.0
    assert sc.as_dict(0)['average_jaccard'] > 0.0 or scaling == 'none'


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_model_level(precision):
  import spa3d
  B, N, Q, T = 3, 40, 96, 8
  cfg = O.Config(**MINI, use_dino=True, use_depth=True, dino_feature_dim=16, depth_feature_dim=1)
  model = product_model(spa3d, cfg, precision)
  batch = batch_to(O.synthetic_batch(B, N, Q, T, seed=11, dino_dim=16, depth_dim=1), 'cuda')
  batch['intrinsics'] = torch.from_numpy(INTRINSICS).cuda()
  v = {'params': model.init(0, batch)['params']}
  noise = torch.rand(B, cfg.num_latent_tokens, cfg.latent_token_dim, generator=torch.Generator().manual_seed(3)).cuda()
  scalings = ('median', 'per_trajectory', 'none')
  res = model.tapvid3d(v, batch, scalings=scalings, ratios=True, noise=noise)
  assert tuple(res) == scalings
  preds = model.apply(v, batch, noise=noise)
  for s in scalings:
    _bit_equal(res[s], spa3d.tapvid3d_predictions(preds, batch, scaling=s, intrinsics=batch['intrinsics'], ratios=True), f'{precision} {s}: model.tapvid3d vs tapvid3d_predictions(model.apply)')
    d = dict(p=preds.tracks.cpu().numpy(), l=preds.visible_logits[..., 0].cpu().numpy(), g=batch['query_tracks'].float().cpu().numpy(),
             y=batch['query_tracks_visible'].float().cpu().numpy().reshape(B, Q, T), qp=batch['query_points'].float().cpu().numpy())
    TU.check_call(d, _np(res[s]), s, INTRINSICS, False, what=f'model {precision} {s}')
  again = model.tapvid3d(v, batch, scalings=scalings, ratios=True, noise=noise)
  for s in scalings:
    _bit_equal(again[s], res[s], f'{precision} {s}: second run')
  # tie to spa3d_score: scaling 'none' + the fixed table are its thresholds; take the query frame out of both by y = 0 at tq
  tq = TU.query_frame(batch['query_points'].float().cpu().numpy(), T)
  moved = dict(batch)
  y = batch['query_tracks_visible'].clone()
  y.reshape(B, Q, T)[torch.arange(B)[:, None], torch.arange(Q)[None, :], torch.from_numpy(tq)] = 0
  moved['query_tracks_visible'] = y
  tv = model.tapvid3d(v, moved, scalings=('none',), fixed_thresholds=True, noise=noise)['none']
  sc = model.score(v, moved, thresholds=TU.FIXED, return_predictions=True, noise=noise)
  assert torch.equal(sc.predictions.tracks, preds.tracks)
  a, s = tv.sample_stats, sc.sample_stats
  print(f'  model {precision}: pooled W {a[:, 4::4].sum(0).tolist()} TP {a[:, 5::4].sum(0).tolist()} FP {a[:, 6::4].sum(0).tolist()} of {a[:, 1].sum().item()} visible evaluated frames')
  assert torch.equal(a[:, 1], s[:, 0]), 'visible frames'
  assert torch.equal(a[:, 4::4], s[:, 8::4]) and torch.equal(a[:, 5::4], s[:, 9::4]) and torch.equal(a[:, 7::4], s[:, 11::4]), 'W / TP / FN'
  # FP: spa3d_score still counts a predicted-visible query frame (y = 0 there: a false positive at every threshold); the metric leaves the frame out
  pv_tq = (np.take_along_axis(preds.visible_logits[..., 0].cpu().numpy(), tq[..., None], 2)[..., 0] > 0).sum(1).astype(np.float64)
  assert torch.equal(a[:, 6::4], s[:, 10::4] - torch.from_numpy(pv_tq).cuda()[:, None]), 'FP'
  assert torch.equal(a[:, 3], s[:, 6] - torch.from_numpy(pv_tq).cuda()) and torch.equal(a[:, 0], s[:, 7] - Q)
