"""Ragged batches on the GPU (include/spa3d.h, spa3d_set_counts; batch keys `support_count` / `query_count`): per-sample counts of live support
tracks and live queries in padded tensors whose padding is never read.

  1. fp32, MINI with DINO + depth, against the fp64 oracle run per sample on the cropped sample with the common denominator, summed
     (tests/ragged_util.py; the construction is pinned on the CPU by tests/test_ragged_host.py): the gates of tests/test_gpu_model.py.
  2. fp32, MINI and the full-size model at T = 150, against single-sample calls of the same handle on the cropped samples (the uniform path):
     the gates of tests/test_gpu_intra_chunk.py::_compare_exactish.
  3. bf16 / fp16, full size, prune + ro_share: (i) error against the fp32 parity mode's single-sample runs at most 1.5 x the error of the
     uniform 16-bit single-sample runs against the same reference; (ii) against the 16-bit single-sample runs (GATES16 below).
  4. NaN in every padded row of every input: bit-identical to zero padding, all finite, padded output rows exactly 0; once more under poison.
  5. spa3d_plan_stats follows the live counts; counts equal to (N, Q) are the uniform call, bit for bit.
  6. det_grads: two ragged train calls bit-equal; "chunk" 1 against 0.
  7. Refusals (SPA3D_ERR_ARG with a message, nothing launched) and the detach.
  8. TrainState.train_step on a ragged batch against the oracle's per-sample sum + AdamW.

Measured on one MI355X when the feature was added: profiles/r07_ragged.log."""
import ctypes as C

import pytest
import torch

from ragged_util import QUERY_KEYS, SUPPORT_KEYS, crop, fill_padding, live_visible, per_sample_sum
from util import MINI, Gates, O, batch_to, max_abs, product_model, rel_err

pytestmark = pytest.mark.gpu
CAST = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
COUNT_KEYS = ('support_count', 'query_count')


def _set(spa3d, h, **opts):
  lib = spa3d._lib.load()
  for k, v in opts.items():
    spa3d._lib.check(lib.spa3d_set_option(h, k.encode(), float(v)), h, k)


def _with_counts(batch, counts):
  out = dict(batch)
  out['support_count'] = torch.tensor([n for n, _ in counts], dtype=torch.int32)
  out['query_count'] = torch.tensor([q for _, q in counts], dtype=torch.int32)
  return out


def _plain(batch):
  return {k: v for k, v in batch.items() if k not in COUNT_KEYS}


def _mini(spa3d, precision='fp32'):
  cfg = O.Config(**MINI, use_dino=True, use_depth=True, dino_feature_dim=16, depth_feature_dim=1)
  model = product_model(spa3d, cfg, precision)
  batch = O.synthetic_batch(3, 200, 96, 8, seed=11, dino_dim=16, depth_dim=1)
  batch['boundary_frame'] = torch.tensor([8, 7, 5], dtype=torch.int32)
  return cfg, model, batch, [(200, 96), (117, 40), (64, 1)]


def _full(spa3d, precision='fp32', seed=31, feat=None):
  import bench
  dev = torch.device('cuda', 0)
  model = spa3d.TrackAutoEncoder3D(num_output_frames=150, dino_feature_dim=768, depth_feature_dim=1, precision=precision)
  batch = bench.synth_batch(3, 300, 96, 150, 768, 1, dev, seed=seed, feat_dtype=CAST[feat or precision])
  batch['boundary_frame'] = torch.tensor([150, 97, 150], dtype=torch.int32, device=dev)
  return model, batch, [(300, 96), (117, 40), (64, 1)]


def _assert_visible_live_points(batch, counts):
  for b, (n, q) in enumerate(counts):
    assert float(batch['query_tracks_visible'][b, :q].sum()) >= 1.0, f'sample {b} has no visible live query point'


def _perturb(params, seed=0, amt=0.1):
  g = torch.Generator().manual_seed(seed)
  for k, v in O.tree_flatten(params).items():
    if k.endswith('bias') or k.endswith('scale'):
      v.add_((amt * torch.randn(v.shape, generator=g)).to(v.device))


def _run(spa3d, model, dims, params, batch, noise, det=1, poison=0, chunk=0, modes=('train', 'forward', 'encode', 'decode')):
  """Every entry point once on `batch` (with or without count keys); results as clones."""
  h = model._handle(*dims)[0]
  _set(spa3d, h, poison=poison, chunk=chunk)
  v = {'params': params}
  r = {}
  if 'train' in modes:
    _set(spa3d, h, det_grads=det)
    ld, grads, preds = model.loss_and_grads(v, batch, noise=noise, return_predictions=True)
    r['loss'] = torch.stack([ld['total_loss'], ld['position_loss'], ld['visible_loss']]).clone()
    r['train.tracks'], r['train.visible'] = preds.tracks.clone(), preds.visible_logits.clone()
    r['grads'] = {k: g.clone() for k, g in O.tree_flatten(grads).items()}
    _set(spa3d, h, det_grads=0)
  if 'forward' in modes:
    out = model(v, batch, noise=noise)
    r['forward.tracks'], r['forward.visible'], r['forward.certain'] = out.tracks.clone(), out.visible_logits.clone(), out.certain_logits.clone()
  if 'encode' in modes or 'decode' in modes:
    lat = model.encode(v, batch)
    r['encode.latents'] = lat.clone()
    if 'decode' in modes:
      out = model.decode(v, lat, model.get_decoder_context(batch), noise=noise)
      r['decode.tracks'], r['decode.visible'] = out.tracks.clone(), out.visible_logits.clone()
  torch.cuda.synchronize()
  _set(spa3d, h, poison=0, chunk=0)
  return r


def _run_singles(spa3d, model, dims, params, batch, counts, noise, det=1, modes=('train', 'forward', 'encode', 'decode')):
  """The yardstick: one uniform call per sample on the cropped sample (no counts), denominator D, gradients summed over the samples;
  results laid out as a ragged call lays them out (padded output rows 0)."""
  plain = _plain(batch)
  D = max(live_visible(plain, counts), 1.0)
  B, Q = plain['query_points'].shape[:2]
  r = {}
  gsum, G = None, None
  for b, (n, q) in enumerate(counts):
    if q == 0:  # no live query: the sample is only encoded (a uniform call has no Q = 0)
      one = _run(spa3d, model, dims, params, crop(plain, b, n, 1), noise[b:b + 1], det=det, modes=('encode',)) if 'encode' in modes else {}
      for k, t in one.items():
        r.setdefault(k, torch.zeros((B,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device))[b] = t[0]
      continue
    one = _run(spa3d, model, dims, params, crop(plain, b, n, q), noise[b:b + 1], det=det, modes=tuple(m for m in modes if m != 'train'))
    if 'train' in modes:
      h = model._handle(*dims)[0]
      _set(spa3d, h, det_grads=det)
      if model.precision == 'fp16':  # accumulate = 1 is refused with a loss scale: sum the per-sample buffers here
        ld, grads, preds = model.loss_and_grads({'params': params}, crop(plain, b, n, q), denom=D, noise=noise[b:b + 1], return_predictions=True)
        gsum = grads.flat.double() if gsum is None else gsum + grads.flat.double()
        G = grads.flat
      else:
        first, G = G is None, (torch.zeros_like(model.flat_from_tree(params)) if G is None else G)
        ld, grads, preds = model.loss_and_grads({'params': params}, crop(plain, b, n, q), grads_flat=G, accumulate=not first, denom=D,
                                                noise=noise[b:b + 1], return_predictions=True)
      _set(spa3d, h, det_grads=0)
      one['loss'] = torch.stack([ld['total_loss'], ld['position_loss'], ld['visible_loss']]).clone()
      one['train.tracks'], one['train.visible'] = preds.tracks.clone(), preds.visible_logits.clone()
    for k, t in one.items():
      if k == 'loss':
        r[k] = t.double() if k not in r else r[k] + t.double()
      elif k == 'encode.latents':
        r.setdefault(k, torch.zeros((B,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device))[b] = t[0]
      else:
        r.setdefault(k, torch.zeros((B, Q) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device))[b, :q] = t[0]
  if 'train' in modes:
    flat = gsum.float() if gsum is not None else G
    r['grads'] = {k: g.clone() for k, g in O.tree_flatten(model.tree_from_flat(flat.clone(), *dims)).items()}
    r['loss'] = r['loss'].float()
  torch.cuda.synchronize()
  return r


def _finite(r):
  ts = [t for k, t in r.items() if k != 'grads'] + list(r.get('grads', {}).values())
  return all(bool(torch.isfinite(t).all()) for t in ts)


def _worst_leaf(a, ref, floor=1e-9):
  tot = float(torch.cat([g.double().reshape(-1) for g in ref.values()]).norm())
  return max((rel_err(a[k], ref[k]), k) for k in ref if float(ref[k].double().norm()) > floor * tot)


def _compare_exactish(a, ref, what, out_tol=1e-6, grad_tol=1e-5):
  assert _finite(a), f'{what}: non-finite values'
  for k in ref:
    if k == 'grads':
      continue
    e = rel_err(a[k], ref[k])
    print(f'{what}: {k} relative error {e:.3e}')
    assert e <= out_tol, f'{what}: {k} relative error {e:.3e} > {out_tol}'
  if 'grads' in ref:
    worst = _worst_leaf(a['grads'], ref['grads'])
    print(f'{what}: worst gradient leaf {worst[0]:.3e} ({worst[1]})')
    assert worst[0] <= grad_tol, f'{what}: gradient leaf {worst[1]} relative error {worst[0]:.3e} > {grad_tol}'


def _padded_rows_are_zero(r, counts):
  for k, t in r.items():
    if k in ('grads', 'loss', 'encode.latents'):
      continue
    for b, (n, q) in enumerate(counts):
      assert float(t[b, q:].abs().sum()) == 0.0, f'{k}: padded rows of sample {b} are not 0'


# ---------------------------------------------------------------------------------------------- 1. fp32 MINI against the fp64 oracle
def test_fp32_mini_ragged_vs_oracle_per_sample():
  import spa3d
  cfg, model, batch, counts = _mini(spa3d)
  _assert_visible_live_points(batch, counts)
  gb = batch_to(batch, 'cuda')
  params = model.init(0, gb)['params']
  _perturb(params)
  noise = torch.rand(3, cfg.num_latent_tokens, cfg.latent_token_dim, generator=torch.Generator().manual_seed(3))
  om = O.TrackAutoEncoder3D(cfg)
  p64 = O.tree_unflatten({k: v.detach().cpu().double() for k, v in O.tree_flatten(params).items()})
  b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
  ld_ref, preds_ref, grads_ref, D = per_sample_sum(lambda b, nz, d: O.loss_and_grads(om, p64, b, discretize=True, noise=nz, denom=d), b64, counts,
                                                    noise.double())
  lat_ref = [om.encode(p64, crop(b64, b, n, q)) for b, (n, q) in enumerate(counts)]
  rb = _with_counts(fill_padding(gb, counts, float('nan')), counts)  # the padding is never read: NaN there must not matter
  v = {'params': params}
  preds = model.apply(v, rb, discretize=True, noise=noise.cuda())
  lat = model.encode(v, rb)
  for b, (n, q) in enumerate(counts):
    e_t, e_v = max_abs(preds.tracks[b, :q], preds_ref[b].tracks[0].detach()), max_abs(preds.visible_logits[b, :q], preds_ref[b].visible_logits[0].detach())
    e_l = max_abs(lat[b], lat_ref[b][0].detach())
    print(f'sample {b} (n = {n}, q = {q}): max abs error tracks {e_t:.3e} visible logits {e_v:.3e} latents {e_l:.3e}')
    assert e_t < 1e-4 and e_v < 1e-4 and e_l < 1e-4
    assert float(preds.tracks[b, q:].abs().sum()) == 0.0 and float(preds.visible_logits[b, q:].abs().sum()) == 0.0
  assert float(preds.certain_logits.abs().max()) == 0.0
  ld = spa3d.compute_loss_3d(preds, rb)
  ld2, grads, preds2 = model.loss_and_grads(v, rb, discretize=True, noise=noise.cuda(), return_predictions=True)
  assert max_abs(preds2.tracks, preds.tracks) == 0.0
  for k in ('total_loss', 'position_loss', 'visible_loss'):
    print(f'{k}: compute_loss_3d {float(ld[k]):.9g} loss_and_grads {float(ld2[k]):.9g} oracle {float(ld_ref[k]):.9g}')
    assert abs(float(ld[k]) - float(ld_ref[k])) <= 1e-5 * abs(float(ld_ref[k])) + 1e-7, k
    assert abs(float(ld2[k]) - float(ld_ref[k])) <= 1e-5 * abs(float(ld_ref[k])) + 1e-7, k
  gflat = O.tree_flatten(grads)
  assert set(gflat) == set(grads_ref)
  worst = (0.0, '')
  for k, gref in grads_ref.items():
    e = rel_err(gflat[k], gref) if float(gref.norm()) > 1e-12 else float(gflat[k].abs().max())
    worst = max(worst, (e, k))
    assert e < 2e-3, (k, e)
  print('ragged fp32 mini: worst gradient leaf vs the oracle', worst)


# ---------------------------------------------------------------------------------------------- 2. fp32 against single-sample calls
@pytest.mark.parametrize('shape', ['mini', 'full'])
def test_fp32_ragged_equals_single_sample_calls(shape):
  import spa3d
  if shape == 'mini':
    _, model, batch, counts = _mini(spa3d)
    batch = batch_to(batch, 'cuda')
  else:
    model, batch, counts = _full(spa3d)
  _assert_visible_live_points(batch, counts)
  dims = model._dims_from_batch(batch)
  params = model.init(0, batch)['params']
  noise = torch.rand(3, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(3)).cuda()
  ref = _run_singles(spa3d, model, dims, params, batch, counts, noise)
  assert _finite(ref)
  got = _run(spa3d, model, dims, params, _with_counts(batch, counts), noise)
  _compare_exactish(got, ref, f'fp32 {shape} ragged vs single-sample calls')
  _padded_rows_are_zero(got, counts)


@pytest.mark.parametrize('case', ['fp32-mini', 'bf16-full', 'fp16-full'])
def test_a_sample_without_live_queries(case):
  """query_count 0 is allowed: the sample is encoded, its output rows are 0 and it adds neither loss nor gradient -- in a packed chunk
  (chunk = 0) and alone in its chunk (chunk = 1).  fp32: the gates of test 2 against single-sample calls (which skip the sample).  16-bit:
  the rule of test 3 (i) -- no further from the fp32 single-sample runs than 1.5 x what the uniform 16-bit single-sample runs are (a packed
  chunk's GEMMs see other row counts than a single sample's, so the planner may pick other kernels: measured 9e-7 on fp16 outputs)."""
  import spa3d
  precision, shape = case.split('-')
  if shape == 'mini':
    _, model, batch, counts = _mini(spa3d, precision)
    batch = batch_to(batch, 'cuda')
  else:
    model, batch, counts = _full(spa3d, precision, seed=36)
  counts = [counts[0], (counts[1][0], 0), counts[2]]
  dims = model._dims_from_batch(batch)
  params = model.init(0, batch)['params']
  noise = torch.rand(3, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(4)).cuda()
  rb = _with_counts(fill_padding(batch, counts, float('nan')), counts)
  if precision == 'fp32':
    ref = _run_singles(spa3d, model, dims, params, batch, counts, noise)
  else:
    m32 = spa3d.TrackAutoEncoder3D(num_output_frames=150, dino_feature_dim=768, depth_feature_dim=1, precision='fp32')
    b32 = dict(batch); b32['dino_features'] = batch['dino_features'].float(); b32['depth_features'] = batch['depth_features'].float()
    ref32 = _run_singles(spa3d, m32, dims, params, b32, counts, noise, modes=('train', 'encode'))
    del m32, b32
    torch.cuda.empty_cache()
    uni = _run_singles(spa3d, model, dims, params, batch, counts, noise, modes=('train', 'encode'))
    e_u, _ = _five(uni, ref32, counts)
    lat_u = rel_err(uni['encode.latents'], ref32['encode.latents'])
  for chunk in (0, 1):
    got = _run(spa3d, model, dims, params, rb, noise, chunk=chunk)
    assert _finite(got)
    _padded_rows_are_zero(got, counts)
    if precision == 'fp32':
      _compare_exactish(got, ref, f'{case} with a query-less sample, chunk={chunk}')
      continue
    e_r, _ = _five(got, ref32, counts)
    gt = Gates(f'{case} with a query-less sample, chunk={chunk}: vs the fp32 single-sample runs; bound = 1.5 x the uniform single-sample runs\' error')
    for nm, r_, u_ in zip(('tracks', 'visible logits', 'total loss', 'worst significant gradient leaf', '1 - cosine(whole gradient)'), e_r, e_u):
      gt.le(nm, r_, 1.5 * u_, f'uniform single-sample runs: {u_:.3e}')
    gt.le('latents (encode), relative Frobenius', rel_err(got['encode.latents'], ref32['encode.latents']), 1.5 * lat_u, f'uniform: {lat_u:.3e}')
    gt.check()


# ---------------------------------------------------------------------------------------------- 3. 16-bit modes
# (ii) ragged call against the single-sample calls of the same precision: bound = 1.5 x measured (util.Gates), measured on one MI355X when the
# feature was added (profiles/r07_ragged.log).  Outputs came out bit-identical (the forward of a packed chunk does per row what a single-sample
# call does; the chunked-key cross attention cuts each sample's keys at the same places); the gradients differ in summation order (packed dW
# reductions, one fixed-point shadow for the whole call against one flush per single-sample call), and the fp16 loss by the three fp32 losses
# the test adds up against the call's one sum
GATES16 = {
    'bf16': ((0.0, 0.0, 0.0, 2.15e-7), ('0', '0', '0', '1.43e-7: tracks_to_latents/layer_1/cross_att/dense_query/kernel')),
    'fp16': ((0.0, 0.0, 1.03e-7, 2.14e-7), ('0', '0', '6.85e-8', '1.42e-7: decompress_attn/layer_3/self_att/dense_key/kernel')),
}


def _five(got, ref, counts):
  """tracks, visible logits (live rows), total loss, worst significant gradient leaf, 1 - cosine of the whole gradient, against `ref`."""
  live = lambda t: torch.cat([t[b, :q].reshape(-1) for b, (n, q) in enumerate(counts)])
  names = sorted(ref['grads'])
  a = torch.cat([got['grads'][k].double().reshape(-1) for k in names]); b_ = torch.cat([ref['grads'][k].double().reshape(-1) for k in names])
  cos = float((a @ b_) / (a.norm() * b_.norm()))
  worst = _worst_leaf(got['grads'], ref['grads'], floor=1e-3)
  return (rel_err(live(got['train.tracks']), live(ref['train.tracks'])), rel_err(live(got['train.visible']), live(ref['train.visible'])),
          abs(float(got['loss'][0] - ref['loss'][0])) / abs(float(ref['loss'][0])), worst[0], 1.0 - cos), worst[1]


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_16bit_ragged_gates(precision):
  import spa3d
  model, batch, counts = _full(spa3d, precision, seed=32)
  _assert_visible_live_points(batch, counts)
  dims = model._dims_from_batch(batch)
  params = model.init(0, batch)['params']
  h = model._handle(*dims)[0]
  _set(spa3d, h, prune=1, ro_share=1)
  noise = torch.rand(3, 128, 96, generator=torch.Generator().manual_seed(7)).cuda()
  modes = ('train',)
  m32 = spa3d.TrackAutoEncoder3D(num_output_frames=150, dino_feature_dim=768, depth_feature_dim=1, precision='fp32')
  b32 = dict(batch); b32['dino_features'] = batch['dino_features'].float(); b32['depth_features'] = batch['depth_features'].float()
  ref32 = _run_singles(spa3d, m32, dims, params, b32, counts, noise, modes=modes)
  del m32, b32
  torch.cuda.empty_cache()
  uni = _run_singles(spa3d, model, dims, params, batch, counts, noise, modes=modes)
  got = _run(spa3d, model, dims, params, _with_counts(batch, counts), noise, modes=modes)
  assert _finite(got) and _finite(uni) and _finite(ref32)
  _padded_rows_are_zero(got, counts)
  (e_r, leaf_r), (e_u, leaf_u) = _five(got, ref32, counts), _five(uni, ref32, counts)
  names = ('tracks, relative Frobenius', 'visible logits, relative Frobenius', 'total loss, relative', 'worst significant gradient leaf',
           '1 - cosine(whole gradient)')
  gt = Gates(f'{precision} ragged call vs the fp32 parity mode\'s single-sample runs; bound = 1.5 x the uniform {precision} single-sample runs\' error')
  for nm, r_, u_ in zip(names, e_r, e_u):
    gt.le(nm, r_, 1.5 * u_, f'uniform single-sample runs: {u_:.3e}')
  gt.check()
  bounds, measured = GATES16[precision]
  worst = _worst_leaf(got['grads'], uni['grads'])
  live = lambda t: torch.cat([t[b, :q].reshape(-1) for b, (n, q) in enumerate(counts)])
  g2 = Gates(f'{precision} ragged call vs single-sample calls of the same precision (B = 3, N = 300, Q = 96, T = 150, prune + ro_share)')
  g2.le('tracks, relative Frobenius', rel_err(live(got['train.tracks']), live(uni['train.tracks'])), bounds[0], measured[0])
  g2.le('visible logits, relative Frobenius', rel_err(live(got['train.visible']), live(uni['train.visible'])), bounds[1], measured[1])
  g2.le('total loss, relative', abs(float(got['loss'][0] - uni['loss'][0])) / abs(float(uni['loss'][0])), bounds[2], measured[2])
  g2.le(f'worst gradient leaf ({worst[1]})', worst[0], bounds[3], measured[3])
  g2.check()


# ---------------------------------------------------------------------------------------------- 4. NaN padding
@pytest.mark.parametrize('case', ['fp32-mini', 'bf16-full', 'fp16-full'])
def test_nan_padding_is_never_read(case):
  import spa3d
  precision, shape = case.split('-')
  if shape == 'mini':
    _, model, batch, counts = _mini(spa3d, precision)
    batch = batch_to(batch, 'cuda')
  else:
    model, batch, counts = _full(spa3d, precision, seed=33)
  dims = model._dims_from_batch(batch)
  params = model.init(0, batch)['params']
  noise = torch.rand(3, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(5)).cuda()
  zero = _with_counts(fill_padding(batch, counts, 0.0), counts)
  nan = _with_counts(fill_padding(batch, counts, float('nan')), counts)
  for k in SUPPORT_KEYS + QUERY_KEYS:
    assert bool(torch.isnan(nan[k][1, counts[1][0 if k in SUPPORT_KEYS else 1]:]).all()), k
  clean = _run(spa3d, model, dims, params, zero, noise)
  assert _finite(clean)
  _padded_rows_are_zero(clean, counts)
  for poison in (0, 1):
    dirty = _run(spa3d, model, dims, params, nan, noise, poison=poison)
    assert _finite(dirty), f'poison={poison}: non-finite values'
    _padded_rows_are_zero(dirty, counts)
    for k in clean:
      if k == 'grads':
        assert all(torch.equal(dirty['grads'][g], clean['grads'][g]) for g in clean['grads']), f'poison={poison}: gradients changed with NaN padding'
      else:
        assert torch.equal(dirty[k], clean[k]), f'poison={poison}: {k} changed with NaN padding'


# ---------------------------------------------------------------------------------------------- 5. plan statistics, full counts
def test_plan_stats_follow_the_live_counts_and_full_counts_are_the_uniform_call():
  import spa3d
  model, batch, counts = _full(spa3d, 'bf16', seed=34)
  dims = model._dims_from_batch(batch)
  params = model.init(0, batch)['params']
  h = model._handle(*dims)[0]
  _set(spa3d, h, prune=1, ro_share=1)
  noise = torch.rand(3, 128, 96, generator=torch.Generator().manual_seed(6)).cuda()
  lib = spa3d._lib.load()
  st = (C.c_double * 4)()
  _run(spa3d, model, dims, params, _with_counts(batch, counts), noise, modes=('train',))
  spa3d._lib.check(lib.spa3d_plan_stats(h, st), h)
  T = batch['support_tracks'].shape[2]
  assert st[1] == sum(n for n, _ in counts) * (T + 1), list(st)
  assert st[3] == sum(q for _, q in counts), list(st)
  assert 0 < st[0] < st[1], list(st)  # boundary_frame 97 of sample 1: pruning ran
  ref = _run(spa3d, model, dims, params, _plain(batch), noise)
  B, N, Q = batch['support_tracks'].shape[0], batch['support_tracks'].shape[1], batch['query_points'].shape[1]
  got = _run(spa3d, model, dims, params, _with_counts(batch, [(N, Q)] * B), noise)
  for k in ref:
    if k == 'grads':
      assert all(torch.equal(got['grads'][g], ref['grads'][g]) for g in ref['grads'])
    else:
      assert torch.equal(got[k], ref[k]), k


# ---------------------------------------------------------------------------------------------- 6. det_grads, chunk
@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'fp32'])
def test_det_grads_bit_reproducible_and_chunk_option(precision):
  import spa3d
  if precision == 'fp32':
    _, model, batch, counts = _mini(spa3d)
    batch = batch_to(batch, 'cuda')
  else:
    model, batch, counts = _full(spa3d, precision, seed=35)
  dims = model._dims_from_batch(batch)
  params = model.init(0, batch)['params']
  noise = torch.rand(3, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(8)).cuda()
  rb = _with_counts(batch, counts)
  a = _run(spa3d, model, dims, params, rb, noise, det=1, modes=('train',))
  b = _run(spa3d, model, dims, params, rb, noise, det=1, modes=('train',))
  assert _finite(a)
  assert torch.equal(a['loss'], b['loss']) and torch.equal(a['train.tracks'], b['train.tracks'])
  assert all(torch.equal(a['grads'][k], b['grads'][k]) for k in a['grads']), 'det_grads on a ragged batch is not bit-reproducible'
  c1 = _run(spa3d, model, dims, params, rb, noise, det=1, chunk=1)
  c0 = _run(spa3d, model, dims, params, rb, noise, det=1, chunk=0)
  _compare_exactish(c1, c0, f'{precision} ragged chunk=1 vs chunk=0')


# ---------------------------------------------------------------------------------------------- 7. refusals and detach
def _raw_forward(spa3d, model, params, batch, B, cn, cq):
  """spa3d_set_counts + spa3d_forward through the C ABI, past the Python validation.  Returns (status, message, output tensor)."""
  lib = spa3d._lib.load()
  dims = model._dims_from_params(params)
  h = model._handle(*dims)[0]
  flat = model.flat_from_tree(params)
  b, keep = model._marshal(_plain(batch), *dims)
  res, out = model._alloc_outputs(b.B, b.Q, flat.device)
  res.tracks.fill_(7.0)
  ws = model._workspace(h, b.B, b.N, b.Q, b.T, False, flat.device)
  arr = lambda v: (C.c_int32 * len(v))(*v) if v is not None else None
  rc0 = lib.spa3d_set_counts(h, B, arr(cn), arr(cq))
  assert rc0 == 0
  rc = lib.spa3d_forward(h, flat.data_ptr(), C.byref(b), C.byref(out), ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
  msg = lib.spa3d_last_error(h).decode()
  assert lib.spa3d_set_counts(h, 0, None, None) == 0
  torch.cuda.synchronize()
  return rc, msg, res.tracks


def test_refusals_and_detach():
  import spa3d
  _, model, batch, counts = _mini(spa3d)
  batch = batch_to(batch, 'cuda')
  dims = model._dims_from_batch(batch)
  params = model.init(0, batch)['params']
  noise = torch.rand(3, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(9)).cuda()
  h = model._handle(*dims)[0]
  N, Q = 200, 96
  ok_n, ok_q = [n for n, _ in counts], [q for _, q in counts]
  bad = [('n_b = 0', 3, [200, 0, 64], ok_q), ('n_b > N', 3, [200, N + 1, 64], ok_q), ('q_b > Q', 3, ok_n, [96, Q + 1, 1]),
         ('q_b < 0', 3, ok_n, [96, -1, 1]), ('stored B differs', 2, ok_n[:2], ok_q[:2]), ('support counts alone, n_b = 0', 3, [0, 1, 1], None)]
  for what, B, cn, cq in bad:
    rc, msg, tr = _raw_forward(spa3d, model, params, batch, B, cn, cq)
    assert rc == 1 and len(msg) > 0, (what, rc, msg)
    assert bool((tr == 7.0).all()), f'{what}: the refused call wrote outputs'
  for opt in ('track_chunk', 'query_chunk'):
    _set(spa3d, h, **{opt: 32})
    rc, msg, tr = _raw_forward(spa3d, model, params, batch, 3, ok_n, ok_q)
    _set(spa3d, h, **{opt: 0})
    assert rc == 1 and 'chunk' in msg and bool((tr == 7.0).all()), (opt, rc, msg)
  rc, msg, tr = _raw_forward(spa3d, model, params, batch, 3, ok_n, ok_q)  # the accepted call, for contrast
  assert rc == 0 and not bool((tr == 7.0).any()), (rc, msg)
  # Python: the same values are ValueErrors before anything reaches the library
  for key, vals in (('support_count', [200, 0, 64]), ('support_count', [200, 201, 64]), ('query_count', [96, 97, 1]), ('support_count', [200, 64])):
    rb = _with_counts(batch, counts)
    rb[key] = torch.tensor(vals, dtype=torch.int32)
    with pytest.raises(ValueError):
      model({'params': params}, rb, noise=noise)
    with pytest.raises(ValueError):
      model.loss_and_grads({'params': params}, rb, noise=noise)
  # the 2-D twin refuses counts
  m2 = spa3d.TrackAutoEncoder(num_output_frames=24, precision='fp32')
  b2 = batch_to(O.synthetic_batch_2d(2, 20, 8, 24, seed=5), 'cuda')
  p2 = m2.init(0, b2)['params']
  rc, msg, tr = _raw_forward(spa3d, m2, p2, b2, 2, [20, 10], [8, 4])
  assert rc == 1 and len(msg) > 0 and bool((tr == 7.0).all()), (rc, msg)
  with pytest.raises(ValueError):
    m2({'params': p2}, _with_counts(b2, [(20, 8), (10, 4)]))
  # after a ragged call (the model detaches the counts) a uniform batch on the same handle is what a fresh handle gives
  model({'params': params}, _with_counts(batch, counts), noise=noise)
  after = _run(spa3d, model, dims, params, batch, noise)
  _, fresh_model, _, _ = _mini(spa3d)
  fresh = _run(spa3d, fresh_model, dims, params, batch, noise)
  for k in fresh:
    if k == 'grads':
      assert all(torch.equal(after['grads'][g], fresh['grads'][g]) for g in fresh['grads'])
    else:
      assert torch.equal(after[k], fresh[k]), k


def test_collate_ragged_feeds_the_model_and_split_ragged_cuts_the_results():
  """The evaluation-loop use: per-clip dicts -> collate_ragged -> one call -> split_ragged, against one call per clip."""
  import spa3d
  _, model, batch, counts = _mini(spa3d)
  gb = batch_to(batch, 'cuda')
  params = model.init(0, gb)['params']
  noise = torch.rand(3, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(12)).cuda()
  clips = []
  for b, (n, q) in enumerate(counts):
    c = {k: v[0] for k, v in crop(gb, b, n, q).items()}
    c['boundary_frame'] = torch.tensor(int(batch['boundary_frame'][b]))  # a host scalar, as a loader would hand it over
    clips.append(c)
  rb = spa3d.collate_ragged(clips, pad_value=float('nan'))
  assert rb['support_count'].tolist() == [n for n, _ in counts] and rb['query_count'].tolist() == [q for _, q in counts]
  preds = model.apply({'params': params}, rb, noise=noise)
  parts = spa3d.split_ragged(preds, rb)
  for b, (n, q) in enumerate(counts):
    one = model.apply({'params': params}, crop(gb, b, n, q), noise=noise[b:b + 1])
    assert parts[b]['tracks'].shape == (q, 8, 3)
    assert rel_err(parts[b]['tracks'], one.tracks[0]) <= 1e-6 and rel_err(parts[b]['visible_logits'], one.visible_logits[0]) <= 1e-6


# ---------------------------------------------------------------------------------------------- 8. train step
def test_train_step_on_a_ragged_batch_matches_oracle_adamw():
  import spa3d
  cfg, model, batch, counts = _mini(spa3d)
  _assert_visible_live_points(batch, counts)
  gb = batch_to(batch, 'cuda')
  params = model.init(0, gb)['params']
  _perturb(params)
  noise = torch.rand(3, cfg.num_latent_tokens, cfg.latent_token_dim, generator=torch.Generator().manual_seed(3))
  st = spa3d.TrainState(model, params, learning_rate=1e-2, warmup_steps=0, total_steps=10)  # no warm-up: the one step moves the parameters
  om = O.TrackAutoEncoder3D(cfg)
  flatP = O.tree_flatten(O.tree_unflatten({k: v.detach().cpu().double() for k, v in O.tree_flatten(params).items()}))
  M = {k: torch.zeros_like(v) for k, v in flatP.items()}
  V = {k: torch.zeros_like(v) for k, v in flatP.items()}
  b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
  rb = _with_counts(fill_padding(gb, counts, float('nan')), counts)
  mt = st.train_step(rb, noise=noise.cuda())
  ld, _, g, _ = per_sample_sum(lambda b, nz, d: O.loss_and_grads(om, O.tree_unflatten(flatP), b, noise=nz, denom=d), b64, counts, noise.double())
  lr = O.lr_schedule(0, 1e-2, 0, 10)
  gn = O.adamw_step(flatP, g, M, V, 0, lr)
  assert lr == 1e-2 and abs(mt['train/learning_rate'] - lr) < 1e-12
  print('ragged train step: loss', float(mt['train/loss']), 'oracle', float(ld['total_loss']), 'grad norm', float(mt['train/grad_norm']), 'oracle', gn)
  assert abs(float(mt['train/loss']) - float(ld['total_loss'])) < 1e-4 * abs(float(ld['total_loss']))
  assert abs(float(mt['train/grad_norm']) - gn) < 1e-3 * gn
  got = O.tree_flatten(st.params)
  for k, v in flatP.items():
    assert max_abs(got[k], v) < 2e-4, k
