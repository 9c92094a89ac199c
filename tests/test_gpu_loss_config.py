"""The configurable training objective (include/spa3d.h, spa3d_loss_config / spa3d_set_point_weights) on the GPU: parity of loss and
gradients with the float64 oracle under torch autograd for five objectives and the 2-D twin, the defaults against the call without a
configuration (bit for bit), every place the weight plane is addressed (sample chunks, query chunks, track chunks, packed and single ragged
samples), the 16-bit modes, and det_grads under a visibility-only objective.

The objective is restated here in torch (`_objective`), on the oracle's float64 predictions: the reference the library is compared with is
the oracle's network plus this restatement, differentiated by autograd.  One case serves every test: the MINI network with DINO 24 and
depth 1 on B, N, Q, T = 3, 10, 6, 8 (tests/test_gpu_model.py::test_mini_forward_loss_grads_fp32's); its oracle forward runs once."""
import ctypes as C
import os
import sys

import pytest
import torch

from test_gpu_model import _noise, _params_to_oracle, _setup
from test_trajan2d import MINI2D, _model as _model2d
from util import MINI, Gates, O, batch_to, max_abs, product_model, rel_err

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_t150_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu

B, N, Q, T, DINO, DEPTH = 3, 10, 6, 8, 24, 1
COUNTS = [(10, 6), (4, 0), (7, 3)]   # the ragged batch: (support_count, query_count) per sample
LOSS_KEYS = ('total_loss', 'position_loss', 'visible_loss')


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


def _objectives(spa3d):
  """name -> (LossConfig, with the weight plane)"""
  L, H = spa3d.LossConfig, spa3d.POS_HUBER
  return {
      'a': (L(l1_weight=1.0, bce_weight=1.0), False),
      'b': (L(l1_weight=0.0, bce_weight=1.0, bce_pos_weight=3.0), False),                         # visibility only
      'c': (L(position_kind=H, huber_delta=1.0, axis_weight=(1.0, 0.5, 0.25)), False),
      'd': (L(), True),
      'e': (L(l1_weight=1.0, bce_weight=1.0, position_kind=H, huber_delta=1.0, axis_weight=(1.0, 0.5, 0.25), bce_pos_weight=3.0), True),
  }


def _weight_plane(shape, seed=77):
  """uniform in [0, 1], a quarter of the entries exactly 0"""
  g = torch.Generator().manual_seed(seed)
  w = torch.rand(shape, generator=g)
  w[torch.rand(shape, generator=g) < 0.25] = 0.0
  return w


def _objective(cfg, tracks, logits, batch, w=None, denom=None):
  """The objective of include/spa3d.h in torch, in the dtype of the predictions: {total, position, visible}."""
  tt, y = batch['query_tracks'].to(tracks.dtype), batch['query_tracks_visible'].to(tracks.dtype)
  nc = tracks.shape[-1]
  d = tracks - tt
  a = d.abs()
  if cfg.position_kind == 1:
    rho = torch.where(a <= cfg.huber_delta, d * d / (2 * cfg.huber_delta), a - cfg.huber_delta / 2)
  else:
    rho = a
  e = (rho * torch.tensor(cfg.axis_weight[:nc], dtype=tracks.dtype)).sum(-1, keepdim=True)
  ls = torch.nn.functional.logsigmoid
  v = -cfg.bce_pos_weight * y * ls(logits) - (1 - y) * ls(-logits)
  wt = torch.ones_like(y) if w is None else w.to(tracks.dtype).reshape(y.shape)
  D = torch.clamp(y.sum(), min=1.0) if denom is None else denom
  P, V = (wt * y * e).sum() / D, (wt * v).sum() / D
  return {'total_loss': cfg.l1_weight * P + cfg.bce_weight * V, 'position_loss': P, 'visible_loss': V}


def _oracle(om, p64, b64, noise, objectives, w):
  """One float64 forward; per objective the three losses and the gradient of the total by autograd."""
  leaves = {k: v.detach().clone().requires_grad_(True) for k, v in O.tree_flatten(p64).items()}
  preds = om(O.tree_unflatten(leaves), b64, discretize=True, noise=noise.double())
  out = {}
  names = sorted(leaves)
  for name, (cfg, weighted) in objectives.items():
    ld = _objective(cfg, preds.tracks, preds.visible_logits, b64, w if weighted else None)
    gs = torch.autograd.grad(ld['total_loss'], [leaves[k] for k in names], retain_graph=True, allow_unused=True)
    out[name] = ({k: float(v.detach()) for k, v in ld.items()}, {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(names, gs)})
  return preds, out


def _with_weights(gb, w, weighted):
  return dict(gb, query_weight=w.cuda()) if weighted else gb


def _assert_losses(ld, ref, what):
  for k in LOSS_KEYS:
    print(f'{what}: {k} {float(ld[k]):.9g} (oracle {ref[k]:.9g})')
    assert abs(float(ld[k]) - ref[k]) <= 1e-5 * abs(ref[k]) + 1e-7, (what, k, float(ld[k]), ref[k])


def _assert_grads(grads, grads_ref, what):
  gflat = O.tree_flatten(grads)
  assert set(gflat) == set(grads_ref)
  worst = (0.0, '')
  for k, gref in grads_ref.items():
    e = rel_err(gflat[k], gref) if float(gref.norm()) > 1e-12 else float(gflat[k].abs().max())
    worst = max(worst, (e, k))
    assert e < 2e-3, (what, k, e)
  print(f'{what}: worst gradient leaf {worst[0]:.3e} ({worst[1]})')


def _sides_of_delta(preds_ref, b64, delta):
  """shares of the visible coordinate errors below / above delta"""
  vis = b64['query_tracks_visible'].expand_as(preds_ref.tracks) > 0.5
  a = (preds_ref.tracks.detach() - b64['query_tracks']).abs()[vis]
  below = float((a <= delta).double().mean())
  return below, 1.0 - below


@pytest.fixture(scope='module')
def case(spa3d):
  """The shared case: parameters, batch, noise, weight plane, and the oracle's losses and gradients for every objective (computed once)."""
  cfg = O.Config(**MINI, use_dino=True, use_depth=True, dino_feature_dim=DINO, depth_feature_dim=DEPTH)
  model, params, batch, gb = _setup(spa3d, cfg, B, N, Q, T, 'fp32', DINO, DEPTH)
  batch['boundary_frame'] = torch.tensor([8, 5, 3], dtype=torch.int32)
  gb['boundary_frame'] = batch['boundary_frame'].cuda()
  noise = _noise(B, cfg)
  w = _weight_plane((B, Q, T))
  objectives = _objectives(spa3d)
  p64 = _params_to_oracle(params, torch.float64)
  b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
  preds_ref, ref = _oracle(O.TrackAutoEncoder3D(cfg), p64, b64, noise, objectives, w.double())
  return dict(cfg=cfg, model=model, params=params, batch=batch, gb=gb, noise=noise, w=w, objectives=objectives, b64=b64, preds_ref=preds_ref, ref=ref)


# ---------------------------------------------------------------------------------------------- parity with the oracle's autograd, fp32
@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd', 'e'])
def test_objective_matches_oracle_autograd_fp32(spa3d, case, name):
  cfg, weighted = case['objectives'][name]
  ld_ref, grads_ref = case['ref'][name]
  if cfg.position_kind == spa3d.POS_HUBER:   # both branches of the Huber term must carry weight
    below, above = _sides_of_delta(case['preds_ref'], case['b64'], cfg.huber_delta)
    print(f'objective {name}: {100 * below:.1f} % of the visible coordinate errors at or below delta = {cfg.huber_delta}, {100 * above:.1f} % above')
    assert below >= 0.2 and above >= 0.2
  gb = _with_weights(case['gb'], case['w'], weighted)
  ld, grads, preds = case['model'].loss_and_grads({'params': case['params']}, gb, noise=case['noise'].cuda(), return_predictions=True, loss=cfg)
  assert max_abs(preds.tracks, case['preds_ref'].tracks) < 1e-4
  _assert_losses(ld, ld_ref, f'objective {name}')
  _assert_grads(grads, grads_ref, f'objective {name}')
  _assert_losses(spa3d.compute_loss_3d(preds, gb, loss=cfg), ld_ref, f'objective {name}, compute_loss_3d')
  if name == 'b':
    enc = [k for k in grads_ref if k.startswith('input_track_transformer/')]
    gflat = O.tree_flatten(grads)
    assert enc and any(float(gflat[k].abs().max()) > 0 for k in enc), 'a visibility-only objective must reach the track encoder'
    assert float(ld['position_loss']) > 0 and abs(float(ld['total_loss']) - float(ld['visible_loss'])) <= 1e-6 * abs(float(ld['visible_loss']))
  # the objective was taken off the handle again: the next plain call is the default objective
  ld0, _, _ = case['model'].loss_and_grads({'params': case['params']}, case['gb'], noise=case['noise'].cuda())
  d_ref = _objective(spa3d.LossConfig(), case['preds_ref'].tracks.detach(), case['preds_ref'].visible_logits.detach(), case['b64'])
  _assert_losses(ld0, {k: float(v) for k, v in d_ref.items()}, 'default objective afterwards')


DELTA_2D = 1.0   # Huber threshold of the 2-D case: at least 20 % of its visible coordinate errors lie on each side (asserted below)


def test_2d_twin_huber_with_two_axis_weights(spa3d):
  cfg = O.config_2d(**MINI2D)
  B2, N2, Q2 = 3, 7, 5
  batch = O.synthetic_batch_2d(B2, N2, Q2, T, seed=5)
  batch['boundary_frame'] = torch.tensor([8, 6, 2], dtype=torch.int32)
  gb = batch_to(batch, 'cuda')
  model = _model2d(spa3d, cfg, 'fp32')
  params = model.init(3, gb)['params']
  g = torch.Generator().manual_seed(0)
  for k, v in O.tree_flatten(params).items():
    if k.endswith('bias') or k.endswith('scale'):
      v.add_((0.1 * torch.randn(v.shape, generator=g)).to(v.device))
  noise = torch.rand(B2, cfg.num_latent_tokens, cfg.latent_token_dim, generator=g)
  p64 = O.tree_unflatten({k: v.detach().cpu().double() for k, v in O.tree_flatten(params).items()})
  b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
  loss = spa3d.LossConfig(position_kind=spa3d.POS_HUBER, huber_delta=DELTA_2D, axis_weight=(1.0, 0.5, 0.25))
  preds_ref, ref = _oracle(O.TrackAutoEncoder2D(cfg), p64, b64, noise, {'c': (loss, False)}, None)
  below, above = _sides_of_delta(preds_ref, b64, loss.huber_delta)
  print(f'2-D twin: {100 * below:.1f} % of the visible coordinate errors at or below delta = {loss.huber_delta}, {100 * above:.1f} % above')
  assert below >= 0.2 and above >= 0.2
  ld, grads, preds = model.loss_and_grads({'params': params}, gb, noise=noise.cuda(), return_predictions=True, loss=loss)
  assert preds.tracks.shape == (B2, Q2, T, 2) and max_abs(preds.tracks, preds_ref.tracks) < 1e-4
  _assert_losses(ld, ref['c'][0], '2-D twin')
  _assert_grads(grads, ref['c'][1], '2-D twin')
  _assert_losses(spa3d.compute_loss_2d(preds, gb, loss=loss), ref['c'][0], '2-D twin, compute_loss_2d')


# ---------------------------------------------------------------------------------------------- the defaults are the old path
def _det(spa3d, model, params, on):
  h = model._handle(*model._dims_from_params(params))[0]
  spa3d._lib.check(spa3d._lib.load().spa3d_set_option(h, b'det_grads', float(on)), h, 'det_grads')
  return h


@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'fp16'])
def test_default_config_and_unit_weights_are_the_plain_call_bit_for_bit(spa3d, case, precision):
  model = product_model(spa3d, case['cfg'], precision)
  params, gb, noise = case['params'], case['gb'], case['noise'].cuda()
  _det(spa3d, model, params, 1)
  try:
    ld0, g0, p0 = model.loss_and_grads({'params': params}, gb, noise=noise, return_predictions=True)
    l0, f0, t0, v0 = torch.stack([ld0[k] for k in LOSS_KEYS]).clone(), g0.flat.clone(), p0.tracks.clone(), p0.visible_logits.clone()
    ld1, g1, p1 = model.loss_and_grads({'params': params}, dict(gb, query_weight=torch.ones(B, Q, T, 1, device='cuda')), noise=noise,
                                       return_predictions=True, loss=spa3d.LossConfig())
    l1 = torch.stack([ld1[k] for k in LOSS_KEYS])
  finally:
    _det(spa3d, model, params, 0)
  assert bool(torch.isfinite(f0).all()) and float(f0.abs().max()) > 0
  assert torch.equal(l1, l0) and torch.equal(g1.flat, f0) and torch.equal(p1.tracks, t0) and torch.equal(p1.visible_logits, v0)
  c0 = spa3d.compute_loss_3d(p0, gb)
  c1 = spa3d.compute_loss_3d(p0, dict(gb, query_weight=torch.ones(B, Q, T, device='cuda')), loss=spa3d.LossConfig())
  assert all(torch.equal(c0[k], c1[k]) for k in LOSS_KEYS)


# ---------------------------------------------------------------------------------------------- every addressing path, objective (e)
def _crop(batch, b, n, q):
  sup, qry = ('support_tracks', 'support_tracks_visible', 'dino_features', 'depth_features'), ('query_points', 'query_tracks', 'query_tracks_visible', 'query_weight')
  return {k: (v[b:b + 1, :n] if k in sup else (v[b:b + 1, :q] if k in qry else v[b:b + 1])).contiguous() for k, v in batch.items()}


def _set_chunk(spa3d, model, params, chunk):
  h = model._handle(*model._dims_from_params(params))[0]
  spa3d._lib.check(spa3d._lib.load().spa3d_set_option(h, b'chunk', float(chunk)), h, 'chunk')


def _close(got, ref, what):
  (ld, gflat, tracks, vlog), (ld_r, g_r, t_r, v_r) = got, ref
  e_t, e_v, e_g = max_abs(tracks, t_r), max_abs(vlog, v_r), rel_err(gflat, g_r)
  e_l = max(abs(float(ld[k]) - float(ld_r[k])) / abs(float(ld_r[k])) for k in LOSS_KEYS)
  print(f'{what}: tracks {e_t:.3e}, visible logits {e_v:.3e} (max-abs); flat gradient {e_g:.3e}, losses {e_l:.3e} (relative)')
  assert bool(torch.isfinite(gflat).all()) and bool(torch.isfinite(tracks).all())
  assert e_t < 1e-6 and e_v < 1e-6 and e_g < 1e-5 and e_l < 1e-5, what


def _train(model, params, gb, noise, loss, **kw):
  ld, grads, preds = model.loss_and_grads({'params': params}, gb, noise=noise, return_predictions=True, loss=loss, **kw)
  return {k: ld[k].clone() for k in LOSS_KEYS}, grads.flat.clone(), preds.tracks.clone(), preds.visible_logits.clone()


def test_every_addressing_path_carries_the_weight_plane(spa3d, case):
  loss, _ = case['objectives']['e']
  params, noise = case['params'], case['noise'].cuda()
  gb = _with_weights(case['gb'], case['w'], True)
  model = product_model(spa3d, case['cfg'], 'fp32')
  whole = _train(model, params, gb, noise, loss)
  _assert_losses(whole[0], case['ref']['e'][0], 'objective e, whole batch')
  _set_chunk(spa3d, model, params, 1)
  try:
    _close(_train(model, params, gb, noise, loss), whole, 'chunk = 1')
  finally:
    _set_chunk(spa3d, model, params, 0)
  for attr, size in (('decoder_scan_chunk_size', 2), ('track_chunk_size', 5)):
    setattr(model, attr, size)
    try:
      _close(_train(model, params, gb, noise, loss), whole, f'{attr} = {size}')
    finally:
      setattr(model, attr, None)
  _close(_train(model, params, gb, noise, loss), whole, 'chunk options off again')
  # the ragged batch: NaN in every padded row of the targets and of the weight plane
  rb = {k: v.clone() for k, v in gb.items()}
  for b, (n, q) in enumerate(COUNTS):
    for k in ('query_tracks', 'query_tracks_visible', 'query_weight'):
      rb[k][b, q:] = float('nan')
  D = max(float(sum(gb['query_tracks_visible'][b, :q].double().sum() for b, (n, q) in enumerate(COUNTS))), 1.0)
  Gsum, lsum = torch.zeros_like(whole[1]), {k: 0.0 for k in LOSS_KEYS}
  t_ref, v_ref = torch.zeros_like(whole[2]), torch.zeros_like(whole[3])
  first = True
  for b, (n, q) in enumerate(COUNTS):
    if q == 0:
      continue
    ld, grads, preds = model.loss_and_grads({'params': params}, _crop(gb, b, n, q), grads_flat=Gsum, accumulate=not first, denom=D, noise=noise[b:b + 1],
                                            return_predictions=True, loss=loss)
    first = False
    for k in LOSS_KEYS:
      lsum[k] += float(ld[k])
    t_ref[b, :q], v_ref[b, :q] = preds.tracks[0], preds.visible_logits[0]
  singles = (lsum, Gsum, t_ref, v_ref)
  rb['support_count'] = torch.tensor([n for n, _ in COUNTS], dtype=torch.int32)
  rb['query_count'] = torch.tensor([q for _, q in COUNTS], dtype=torch.int32)
  packed = _train(model, params, rb, noise, loss)
  _close(packed, singles, 'ragged, one packed chunk')
  _set_chunk(spa3d, model, params, 1)
  try:
    _close(_train(model, params, rb, noise, loss), singles, 'ragged, sample by sample')
  finally:
    _set_chunk(spa3d, model, params, 0)
  preds = spa3d.TrackAutoEncoderResults(packed[2], packed[3], torch.zeros_like(packed[3]))
  lr = spa3d.compute_loss_3d(preds, rb, loss=loss)
  assert all(abs(float(lr[k]) - lsum[k]) <= 1e-5 * abs(lsum[k]) for k in LOSS_KEYS), (lr, lsum)


# ---------------------------------------------------------------------------------------------- 16-bit modes
# 1 - cosine of the flat gradient against the float64 oracle, measured when the gates were set (profiles/r12_loss_config.log); bound = 1.5 x
ONE_MINUS_COS = {('bf16', 'b'): 3.7684e-05, ('bf16', 'e'): 5.0831e-05, ('fp16', 'b'): 6.4747e-06, ('fp16', 'e'): 1.0059e-05}


@pytest.mark.parametrize('name', ['b', 'e'])
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_16bit_modes(spa3d, case, precision, name):
  loss, weighted = case['objectives'][name]
  model = product_model(spa3d, case['cfg'], precision)
  params = case['params']
  gb = _with_weights(case['gb'], case['w'], weighted)
  ld, grads, _ = model.loss_and_grads({'params': params}, gb, noise=case['noise'].cuda(), loss=loss)
  gflat = grads.flat
  assert bool(torch.isfinite(gflat).all()) and float(gflat.abs().max()) > 0
  p, m, v = model.flat_from_tree(params).clone(), torch.zeros_like(gflat), torch.zeros_like(gflat)
  scratch = torch.zeros(1024, dtype=torch.float32, device='cuda')
  spa3d._lib.check(spa3d._lib.load().spa3d_adamw_step(p.data_ptr(), gflat.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), 1e-4, 0, 1.0, 0.9, 0.999, 1e-8, 0.01,
                                                       scratch.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), what='spa3d_adamw_step')
  assert float(scratch[2]) == 0.0, 'the step was skipped'
  grads_ref = case['ref'][name][1]
  gf = O.tree_flatten(grads)
  a = torch.cat([gf[k].double().cpu().reshape(-1) for k in sorted(grads_ref)])
  r = torch.cat([grads_ref[k].reshape(-1) for k in sorted(grads_ref)])
  omc = 1.0 - float((a @ r) / (a.norm() * r.norm()))
  measured = ONE_MINUS_COS[(precision, name)]
  g = Gates(f'{precision}, objective {name}: gradient direction against the float64 oracle')
  g.le('1 - cosine of the flat gradient', omc, 1.5 * measured, f'{measured:.3e}')
  g.check()


# ---------------------------------------------------------------------------------------------- det_grads, visibility-only objective
@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_det_grads_resolve_a_visibility_only_objective(spa3d, precision):
  cfg, p, batch, noise = G.make_inputs('c772')
  loss = _objectives(spa3d)['b'][0]
  model = product_model(spa3d, cfg, precision)
  gb = batch_to(batch, 'cuda')
  gp = O.tree_map(lambda t: t.cuda(), p)

  def run(det):
    _det(spa3d, model, gp, det)
    try:
      ld, grads, _ = model.loss_and_grads({'params': gp}, gb, noise=noise.cuda(), loss=loss)
      torch.cuda.synchronize()
    finally:
      _det(spa3d, model, gp, 0)
    return float(ld['total_loss']), {k: v.clone() for k, v in O.tree_flatten(grads).items()}

  a, b, c = run(1), run(1), run(0)
  assert a[0] == b[0] == c[0]
  diff = [k for k in a[1] if not torch.equal(a[1][k], b[1][k])]
  assert not diff, f'{precision}: {len(diff)} leaves differ between two det_grads runs, e.g. {diff[:3]}'
  assert all(bool(torch.isfinite(v).all()) for v in a[1].values()) and any(float(v.abs().max()) > 0 for v in a[1].values())
  worst = max((rel_err(a[1][k], c[1][k]), k) for k in a[1] if float(c[1][k].double().norm()) > 0)
  print(f'{precision}, visibility only: det_grads vs float atomics: worst leaf {worst}; loss {a[0]}')
  assert worst[0] < 5e-5
