"""Per-track scores on the GPU (include/spa3d.h: spa3d_score, spa3d_score_from_preds; TrackAutoEncoder3D.score, score_predictions).

  1. Same-call comparison: spa3d_score with predictions returned is compared with the NumPy float64 restatement (tests/score_util.py, the rules
     are stated there) computed from the predictions THAT CALL returned -- mini and full-width models, fp32 / bf16 / fp16, K = 0 and 5, with and
     without sample_scale, "chunk" 1 and 0, a query chunk dividing Q, a track chunk.  The predictions are bit-equal to spa3d_forward's on the
     same handle and options, spa3d_score_from_preds on them is bit-equal to the fused result, and two runs are bit-equal.
  2. Against existing behaviour: the pooled slots 1 / 0 and 4 / 0 equal spa3d_loss' position and visible loss within relative 1e-6.
  3. Ragged batches: live rows equal the single-sample calls (bit-equal when the sample is alone in its chunk, else against same-call
     predictions), padded rows are all zero, NaN in every padded row and in the padded targets leaves every result finite, split_ragged cuts.
  4. The 2-D twin (NC = 2) and the "poison" test mode."""
import numpy as np
import pytest
import torch

import score_util as SU
from ragged_util import crop, fill_padding
from util import MINI, O, batch_to, product_model

pytestmark = pytest.mark.gpu
CAST = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}


def _set(spa3d, h, **opts):
  lib = spa3d._lib.load()
  for k, v in opts.items():
    spa3d._lib.check(lib.spa3d_set_option(h, k.encode(), float(v)), h, k)


def _perturb(params, seed=0, amt=0.1):
  g = torch.Generator().manual_seed(seed)
  for k, v in O.tree_flatten(params).items():
    if k.endswith('bias') or k.endswith('scale'):
      v.add_((amt * torch.randn(v.shape, generator=g)).to(v.device))


def _mini(spa3d, precision, B=3, N=40, Q=96):
  cfg = O.Config(**MINI, use_dino=True, use_depth=True, dino_feature_dim=16, depth_feature_dim=1)
  model = product_model(spa3d, cfg, precision)
  batch = batch_to(O.synthetic_batch(B, N, Q, 8, seed=11, dino_dim=16, depth_dim=1), 'cuda')
  params = model.init(0, batch)['params']
  _perturb(params)
  noise = torch.rand(B, cfg.num_latent_tokens, cfg.latent_token_dim, generator=torch.Generator().manual_seed(3)).cuda()
  return model, (16, 1), batch, params, noise


def _full(spa3d, precision, B=3, N=300, Q=96):
  import bench
  dev = torch.device('cuda', 0)
  model = spa3d.TrackAutoEncoder3D(num_output_frames=150, dino_feature_dim=768, depth_feature_dim=1, precision=precision)
  batch = bench.synth_batch(B, N, Q, 150, 768, 1, dev, seed=31, feat_dtype=CAST[precision])
  batch['boundary_frame'] = torch.tensor(([150, 97, 150] * B)[:B], dtype=torch.int32, device=dev)
  params = model.init(0, batch)['params']
  noise = torch.rand(B, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(1)).to(dev)
  return model, (768, 1), batch, params, noise


def _thresholds(model, params, batch, noise):
  """Five thresholds at 0.25 / 0.5 / 1 / 2 / 4 x the median frame error of this model on this batch, rounded to three digits: every one of
  them cuts through the data."""
  fe = model.score({'params': params}, batch, frame_errors=True, noise=noise).frame_err
  med = float(fe.flatten().median())
  assert med > 0
  return tuple(float(f'{m * med:.3g}') for m in (0.25, 0.5, 1.0, 2.0, 4.0))


def _reference(preds, batch, thr, scale, rows=None):
  """float64 restatement from predictions; rows: optional (b, q_b) list = the live rows of a ragged batch, else all rows"""
  NC = preds.tracks.shape[-1]
  B, Q, T = preds.tracks.shape[:3]
  sel = [(b, Q) for b in range(B)] if rows is None else rows
  cat = lambda t, w: np.concatenate([t[b, :q].reshape(q, T, w) for b, q in sel]).astype(np.float64) if w else np.concatenate([t[b, :q].reshape(q, T) for b, q in sel]).astype(np.float64)
  p = cat(preds.tracks.cpu().numpy(), NC)
  g = cat(batch['query_tracks'].float().cpu().numpy(), NC)
  l = cat(preds.visible_logits.cpu().numpy(), 0)
  y = cat(batch['query_tracks_visible'].float().cpu().numpy(), 0)
  sc = None if scale is None else np.concatenate([np.full(q, float(scale[b]), np.float32) for b, q in sel])
  return SU.reference(p, l, g, y, thr, sc)


def _live(t, rows):
  return np.concatenate([t[b, :q].cpu().numpy() for b, q in rows])


def _bit_equal(a, b, what):
  for name in ('query_stats', 'sample_stats', 'frame_err'):
    x, y = getattr(a, name), getattr(b, name)
    assert (x is None) == (y is None), f'{what}: {name}'
    if x is not None:
      assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), f'{what}: {name} differs (max |d| {float((x.double() - y.double()).abs().max()):.3e})'


def _sample_stats_pool_the_rows(sc, what):
  qs, ss = sc.query_stats.double(), sc.sample_stats
  want = qs.sum(1)
  want[:, 3] = qs[:, :, 3].max(1).values
  assert ss.dtype == torch.float64
  torch.testing.assert_close(ss, want, rtol=1e-12, atol=0, msg=lambda m: f'{what}: sample_stats is not the pooled rows: {m}')
  cols = [0, 5, 6, 7] + list(range(8, qs.shape[-1]))  # counts: integers, exact in double whatever the order
  assert torch.equal(ss[:, cols], want[:, cols]), what


def _same_call_checks(spa3d, model, dims, params, batch, noise, thr, scale, what):
  """The full set of checks of item 1 for the handle's present options."""
  v = {'params': params}
  sc = model.score(v, batch, thresholds=thr, sample_scale=scale, return_predictions=True, frame_errors=True, noise=noise)
  fwd = model(v, batch, noise=noise)
  torch.cuda.synchronize()
  assert torch.equal(sc.predictions.tracks, fwd.tracks) and torch.equal(sc.predictions.visible_logits, fwd.visible_logits) and \
      torch.equal(sc.predictions.certain_logits, fwd.certain_logits), f'{what}: the predictions of spa3d_score differ from spa3d_forward'
  B, Q, T = fwd.tracks.shape[:3]
  assert sc.query_stats.shape == (B, Q, 8 + 4 * len(thr)) and sc.frame_err.shape == (B, Q, T)
  ref = _reference(sc.predictions, batch, thr, None if scale is None else scale.cpu().numpy())
  SU.check(sc.query_stats.reshape(B * Q, -1).cpu().numpy(), sc.frame_err.reshape(B * Q, T).cpu().numpy(), ref, what)
  _sample_stats_pool_the_rows(sc, what)
  again = model.score(v, batch, thresholds=thr, sample_scale=scale, frame_errors=True, noise=noise)  # out = NULL this time
  assert again.predictions is None
  _bit_equal(again, sc, f'{what}: second run (without predictions)')
  tg = {k: batch[k] for k in ('query_tracks', 'query_tracks_visible')}
  _bit_equal(spa3d.score_predictions(sc.predictions, tg, thresholds=thr, sample_scale=scale, frame_errors=True), sc, f'{what}: spa3d_score_from_preds')
  lean = model.score(v, batch, thresholds=thr, sample_scale=scale, noise=noise)  # no frame_err either
  assert lean.frame_err is None and torch.equal(lean.query_stats, sc.query_stats) and torch.equal(lean.sample_stats, sc.sample_stats)
  return sc


def _loss_cross_check(spa3d, sc, batch, what):
  ld = spa3d.compute_loss_3d(sc.predictions, batch)
  ss = sc.sample_stats
  den = max(float(ss[:, 0].sum()), 1.0)
  pos, vis = float(ss[:, 1].sum()) / den, float(ss[:, 4].sum()) / den
  e_p, e_v = abs(pos - float(ld['position_loss'])) / abs(float(ld['position_loss'])), abs(vis - float(ld['visible_loss'])) / abs(float(ld['visible_loss']))
  print(f'  {what}: position loss {float(ld["position_loss"]):.8e} vs pooled {pos:.8e} (rel {e_p:.2e}); visible loss {float(ld["visible_loss"]):.8e} vs {vis:.8e} (rel {e_v:.2e})')
  assert e_p <= 1e-6 and e_v <= 1e-6, what


# ---------------------------------------------------------------------------------------------- 1 + 2. same-call comparison
@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'fp16'])
def test_mini_same_call(precision):
  import spa3d
  model, dims, batch, params, noise = _mini(spa3d, precision)
  h = model._handle(*dims)[0]
  thr5 = _thresholds(model, params, batch, noise)
  scale = torch.tensor([0.5, 1.0, 1.7], device='cuda')
  for chunk in (1, 0):
    _set(spa3d, h, chunk=chunk)
    for thr in ((), thr5):
      for sc_ in (None, scale):
        s = _same_call_checks(spa3d, model, dims, params, batch, noise, thr, sc_, f'mini {precision} chunk={chunk} K={len(thr)} scale={sc_ is not None}')
    _loss_cross_check(spa3d, s, batch, f'mini {precision} chunk={chunk}')
  _set(spa3d, h, chunk=0)
  # with a scale, the counts at thresholds t x s_b equal the counts of a call with thresholds (t x s_b) and no scale, sample by sample
  a = model.score({'params': params}, batch, thresholds=thr5, sample_scale=scale, noise=noise)
  for b in range(3):
    tb = tuple(float(np.float32(t) * np.float32(float(scale[b]))) for t in thr5)
    one = model.score({'params': params}, batch, thresholds=tb, noise=noise)
    assert torch.equal(one.query_stats[b], a.query_stats[b])


@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'fp32'])
def test_full_width_same_call_and_intra_sample_chunks(precision):
  import spa3d
  model, dims, batch, params, noise = _full(spa3d, precision)
  h = model._handle(*dims)[0]
  thr5 = _thresholds(model, params, batch, noise)
  scale = torch.tensor([1.0, 0.6, 1.5], device='cuda')
  for chunk in (1, 0):
    _set(spa3d, h, chunk=chunk)
    s = _same_call_checks(spa3d, model, dims, params, batch, noise, thr5, scale, f'full {precision} chunk={chunk} K=5 scaled')
    _loss_cross_check(spa3d, s, batch, f'full {precision} chunk={chunk}')
  _set(spa3d, h, chunk=0)
  _same_call_checks(spa3d, model, dims, params, batch, noise, (), None, f'full {precision} K=0')
  base = model.score({'params': params}, batch, thresholds=thr5, noise=noise)
  for name, qc, tc in (('query_chunk 32', 32, None), ('track_chunk 128', None, 128), ('query_chunk 48 + track_chunk 100', 48, 100)):
    model.decoder_scan_chunk_size, model.track_chunk_size = qc, tc
    s = _same_call_checks(spa3d, model, dims, params, batch, noise, thr5, None, f'full {precision} {name}')
    _loss_cross_check(spa3d, s, batch, f'full {precision} {name}')
    if qc is not None and tc is None:  # query chunks alone leave every row's arithmetic alone up to the GEMM kernels picked by row count: fp32 is exact
      d = float((s.query_stats.double() - base.query_stats.double()).abs().max())
      print(f'  full {precision} {name}: max |stats - unchunked| = {d:.3e}')
  model.decoder_scan_chunk_size, model.track_chunk_size = None, None
  _bit_equal(model.score({'params': params}, batch, thresholds=thr5, noise=noise), base, f'full {precision}: back to unchunked')


# ---------------------------------------------------------------------------------------------- 3. ragged batches
def _ragged_checks(spa3d, model, dims, batch, params, noise, counts, thr, scale, what):
  B, Q = batch['query_points'].shape[:2]
  rows = [(b, q) for b, (n, q) in enumerate(counts)]
  h = model._handle(*dims)[0]
  v = {'params': params}
  rb = fill_padding(batch, counts, float('nan'))  # NaN in every padded support / query / TARGET row
  rb['support_count'] = torch.tensor([n for n, _ in counts], dtype=torch.int32)
  rb['query_count'] = torch.tensor([q for _, q in counts], dtype=torch.int32)
  got = {}
  for chunk in (1, 0):  # 1: every sample alone in its chunk; 0: packed chunks
    _set(spa3d, h, chunk=chunk)
    sc = model.score(v, rb, thresholds=thr, sample_scale=scale, return_predictions=True, frame_errors=True, noise=noise)
    torch.cuda.synchronize()
    got[chunk] = sc
    w = f'{what} chunk={chunk}'
    for t in (sc.query_stats, sc.sample_stats, sc.frame_err, sc.predictions.tracks, sc.predictions.visible_logits):
      assert bool(torch.isfinite(t).all()), f'{w}: non-finite results'
    for b, q in rows:  # padded rows: all zero, slot 7 included
      assert float(sc.query_stats[b, q:].abs().sum()) == 0.0 and float(sc.frame_err[b, q:].abs().sum()) == 0.0, f'{w}: padded rows of sample {b}'
      assert bool((sc.query_stats[b, :q, 7] == sc.frame_err.shape[-1]).all())
    ref = _reference(sc.predictions, batch, thr, scale.cpu().numpy(), rows)  # same-call predictions, live rows
    SU.check(_live(sc.query_stats, rows), _live(sc.frame_err, rows), ref, w)
    _sample_stats_pool_the_rows(sc, w)
    fwd = model(v, rb, noise=noise)
    assert torch.equal(fwd.tracks, sc.predictions.tracks) and torch.equal(fwd.visible_logits, sc.predictions.visible_logits), w
    tg = {'query_tracks': rb['query_tracks'], 'query_tracks_visible': rb['query_tracks_visible'], 'query_count': rb['query_count']}
    _bit_equal(spa3d.score_predictions(sc.predictions, tg, thresholds=thr, sample_scale=scale, frame_errors=True), sc, f'{w}: spa3d_score_from_preds with counts')
    _bit_equal(model.score(v, rb, thresholds=thr, sample_scale=scale, frame_errors=True, noise=noise), sc, f'{w}: second run')
    parts = spa3d.split_ragged(sc, rb)
    for (b, q), p in zip(rows, parts):
      assert p.query_stats.shape[0] == q and torch.equal(p.query_stats, sc.query_stats[b, :q]) and torch.equal(p.frame_err, sc.frame_err[b, :q])
      assert torch.equal(p.sample_stats, sc.sample_stats[b]) and p.predictions.tracks.shape[0] == q
  _set(spa3d, h, chunk=0)
  # the single-sample calls on the cropped samples: bit for bit the rows of the sample alone in its chunk
  for b, (n, q) in enumerate(counts):
    if q == 0:
      assert float(got[1].sample_stats[b].abs().sum()) == 0.0 and float(got[0].sample_stats[b].abs().sum()) == 0.0
      continue
    one = model.score(v, crop(batch, b, n, q), thresholds=thr, sample_scale=scale[b:b + 1], frame_errors=True, noise=noise[b:b + 1])
    assert torch.equal(one.query_stats[0], got[1].query_stats[b, :q]) and torch.equal(one.frame_err[0], got[1].frame_err[b, :q]), f'{what}: sample {b} alone in its chunk'
    assert torch.equal(one.sample_stats[0], got[1].sample_stats[b]), f'{what}: sample_stats of sample {b}'


def test_ragged_fp32_mini():
  import spa3d
  model, dims, batch, params, noise = _mini(spa3d, 'fp32', B=4, N=200, Q=96)
  batch['boundary_frame'] = torch.tensor([8, 7, 5, 8], dtype=torch.int32, device='cuda')
  counts = [(200, 96), (117, 40), (64, 1), (50, 0)]
  thr = _thresholds(model, params, batch, noise)
  _ragged_checks(spa3d, model, dims, batch, params, noise, counts, thr, torch.tensor([1.0, 0.5, 2.0, 1.0], device='cuda'), 'ragged mini fp32')


def test_ragged_bf16_full_width():
  import spa3d
  model, dims, batch, params, noise = _full(spa3d, 'bf16', B=4)
  counts = [(300, 96), (117, 40), (64, 1), (200, 0)]
  thr = _thresholds(model, params, batch, noise)
  _ragged_checks(spa3d, model, dims, batch, params, noise, counts, thr, torch.tensor([1.0, 0.5, 2.0, 1.0], device='cuda'), 'ragged full bf16')


# ---------------------------------------------------------------------------------------------- 4. the 2-D twin, poison
def test_2d_twin_same_call():
  import spa3d
  from test_trajan2d import MINI2D, _model
  for precision in ('fp32', 'bf16'):
    cfg = O.config_2d(**MINI2D)
    B, N, Q, T = 3, 12, 40, 8
    batch = batch_to(O.synthetic_batch_2d(B, N, Q, T, seed=5), 'cuda')
    model = _model(spa3d, cfg, precision)
    params = model.init(3, batch)['params']
    _perturb(params)
    noise = torch.rand(B, cfg.num_latent_tokens, cfg.latent_token_dim, generator=torch.Generator().manual_seed(0)).cuda()
    thr = _thresholds(model, params, batch, noise)
    s = _same_call_checks(spa3d, model, (0, 0), params, batch, noise, thr, torch.tensor([1.0, 0.7, 1.3], device='cuda'), f'2-D twin {precision}')
    assert s.predictions.tracks.shape == (B, Q, T, 2)
    ld = spa3d.compute_loss_2d(s.predictions, batch)
    den = max(float(s.sample_stats[:, 0].sum()), 1.0)
    assert abs(float(s.sample_stats[:, 1].sum()) / den - float(ld['position_loss'])) <= 1e-6 * abs(float(ld['position_loss']))
    with pytest.raises(ValueError):  # counts stay refused on the 2-D model
      model.score({'params': params}, dict(batch, query_count=torch.tensor([40, 3, 0])), thresholds=thr, noise=noise)


def test_poison_changes_nothing():
  import spa3d
  model, dims, batch, params, noise = _full(spa3d, 'bf16')
  h = model._handle(*dims)[0]
  thr = _thresholds(model, params, batch, noise)
  kw = dict(thresholds=thr, return_predictions=True, frame_errors=True, noise=noise)
  for chunk, qc in ((0, None), (1, None), (0, 32)):
    model.decoder_scan_chunk_size = qc
    _set(spa3d, h, chunk=chunk, poison=0)
    clean = model.score({'params': params}, batch, **kw)
    _set(spa3d, h, poison=1)
    dirty = model.score({'params': params}, batch, **kw)
    _set(spa3d, h, poison=0)
    _bit_equal(dirty, clean, f'poison, chunk={chunk} query_chunk={qc}')
    assert torch.equal(dirty.predictions.tracks, clean.predictions.tracks) and bool(torch.isfinite(dirty.query_stats).all())
  model.decoder_scan_chunk_size = None
  _set(spa3d, h, chunk=0)
