"""Intra-sample chunking (spa3d_set_option "track_chunk" / "query_chunk", include/spa3d.h): the track encoder over chunks of tracks with its
recompute in the backward, and the readout over chunks of queries, against the same handle without chunks.

  * fp32, MINI (tests/util.py) and the full-size model at B = 2 with DINO and depth (only the full-size model reaches the fused attention, token
    pruning and shared-row paths: 96-wide heads), and the 2-D twin: outputs, losses, latents, forward / encode / decode and every gradient leaf
    against the unchunked run, ragged chunks included.  The gradients run under det_grads, so that what is compared is the chunking and not the
    float-atomic order of two runs.
  * bf16 / fp16 with token pruning and shared readout rows on: chunked against unchunked of the same precision under the util.Gates table
    (gradients under det_grads here too, so that the measured value the bounds derive from is not run-to-run atomic-order noise).
  * det_grads with both options: two runs bit-equal, loss equal to the unchunked loss.
  * poison with both options: the NaN-filled arena before every track / query chunk changes nothing.
  * decoder_scan_chunk_size that does not divide Q: ValueError before any launch.
  * BASELINE.json configs[4] at its full width (B = 1, N = 8192, Q = 2048, T = 300): the fp32 parity mode with track_chunk 1024 / query_chunk 256
    against the fp16 default dispatch -- the comparison tests/test_gpu_cfg5_width.py could make only at N = 4096, because one unchunked fp32
    sample (277 GB of workspace) does not fit the card.  The fp32 run took 6.2 s (32 GB workspace) on one MI355X, the fp16 one 4.3 s including
    its first-call setup (profiles/r06_intra_chunk.log).
"""
import time

import pytest
import torch

from util import MINI, Gates, O, batch_to, product_model, rel_err

pytestmark = pytest.mark.gpu
CAST = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}


def _set(spa3d, h, **opts):
  lib = spa3d._lib.load()
  for k, v in opts.items():
    spa3d._lib.check(lib.spa3d_set_option(h, k.encode(), float(v)), h, k)


def _run(spa3d, model, dims, params, batch, noise, tc=0, qc=0, det=1, poison=0, modes=('train', 'forward', 'encode', 'decode')):
  """Every entry point once with the given chunk options on the handle; returns the results as clones."""
  h = model._handle(*dims)[0]
  _set(spa3d, h, track_chunk=tc, query_chunk=qc, poison=poison)
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
  _set(spa3d, h, track_chunk=0, query_chunk=0, poison=0)
  return r


def _finite(r):
  ts = [t for k, t in r.items() if k != 'grads'] + list(r.get('grads', {}).values())
  return all(bool(torch.isfinite(t).all()) for t in ts)


def _worst_leaf(a, ref):
  tot = float(torch.cat([g.double().reshape(-1) for g in ref.values()]).norm())
  return max((rel_err(a[k], ref[k]), k) for k in ref if float(ref[k].double().norm()) > 1e-9 * tot)


def _compare_exactish(a, ref, what, out_tol=1e-6, grad_tol=1e-5):
  assert _finite(a), f'{what}: non-finite values'
  for k in ref:
    if k == 'grads':
      continue
    e = rel_err(a[k], ref[k])
    assert e <= out_tol, f'{what}: {k} relative error {e:.3e} > {out_tol}'
  if 'grads' in ref:
    worst = _worst_leaf(a['grads'], ref['grads'])
    print(f'{what}: worst gradient leaf {worst[0]:.3e} ({worst[1]})')
    assert worst[0] <= grad_tol, f'{what}: gradient leaf {worst[1]} relative error {worst[0]:.3e} > {grad_tol}'


def _mini(spa3d, precision='fp32'):
  cfg = O.Config(**MINI, use_dino=True, use_depth=True, dino_feature_dim=16, depth_feature_dim=1)
  model = product_model(spa3d, cfg, precision)
  batch = batch_to(O.synthetic_batch(2, 200, 96, 8, seed=11, dino_dim=16, depth_dim=1), 'cuda')
  return model, batch


def _full(spa3d, precision='fp32', seed=21):
  import bench
  dev = torch.device('cuda', 0)
  model = spa3d.TrackAutoEncoder3D(num_output_frames=150, dino_feature_dim=768, depth_feature_dim=1, precision=precision)
  batch = bench.synth_batch(2, 300, 96, 150, 768, 1, dev, seed=seed, feat_dtype=CAST[precision])
  batch['boundary_frame'] = torch.tensor([150, 97], dtype=torch.int32, device=dev)  # ragged key mask: pruning differs per sample
  return model, batch


CHUNKS = [(64, 32), (100, 40), (64, 0), (0, 40)]  # (track_chunk, query_chunk); 100 and 40 leave ragged last chunks of 200 / 300 tracks, 96 queries


@pytest.mark.parametrize('shape', ['mini', 'full'])
def test_fp32_chunked_equals_unchunked(shape):
  import spa3d
  model, batch = _mini(spa3d) if shape == 'mini' else _full(spa3d)
  dims = model._dims_from_batch(batch)
  params = model.init(0, batch)['params']
  noise = torch.rand(2, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(3)).cuda()
  ref = _run(spa3d, model, dims, params, batch, noise)
  assert _finite(ref)
  for tc, qc in CHUNKS:
    _compare_exactish(_run(spa3d, model, dims, params, batch, noise, tc, qc), ref, f'fp32 {shape} track_chunk={tc} query_chunk={qc}')


def test_fp32_2d_twin_chunked_equals_unchunked():
  import spa3d
  model = spa3d.TrackAutoEncoder(num_output_frames=24, precision='fp32')
  batch = batch_to(O.synthetic_batch_2d(2, 200, 96, 24, seed=5), 'cuda')
  batch['boundary_frame'] = torch.tensor([24, 17], dtype=torch.int32, device='cuda')
  params = model.init(0, batch)['params']
  noise = torch.rand(2, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(4)).cuda()
  ref = _run(spa3d, model, (0, 0), params, batch, noise)
  assert _finite(ref)
  for tc, qc in CHUNKS[:2]:
    _compare_exactish(_run(spa3d, model, (0, 0), params, batch, noise, tc, qc), ref, f'2-D twin track_chunk={tc} query_chunk={qc}')


# bound <= 1.5 x measured (util.Gates); measured on one MI355X when the options were added (profiles/r06_intra_chunk.log).  Outputs and losses
# came out bit-identical (the forward has no float atomics, the loss sums are fixed-point); the gradients differ by the summation order of the
# chunked latent-side gradient, which reaches fp16's small tracks_to_latents norm-scale leaves most
GATES16 = {
    'bf16': ((0.0, 0.0, 0.0, 2.3e-7), ('0', '0', '0', '1.51e-7: track_readout_attn/layer_0/self_att/dense_query/kernel')),
    'fp16': ((0.0, 0.0, 0.0, 1.0e-3), ('0', '0', '0', '6.73e-4: tracks_to_latents/layer_0/cross_att/norm_key/scale')),
}


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_16bit_chunked_vs_unchunked_gates(precision):
  import spa3d
  model, batch = _full(spa3d, precision, seed=22)
  dims = model._dims_from_batch(batch)
  params = model.init(0, batch)['params']
  h = model._handle(*dims)[0]
  _set(spa3d, h, prune=1, ro_share=1)
  noise = torch.rand(2, 128, 96, generator=torch.Generator().manual_seed(7)).cuda()
  modes = ('train',)
  ref = _run(spa3d, model, dims, params, batch, noise, det=1, modes=modes)
  lib = spa3d._lib.load()
  st = (spa3d._lib.C.c_double * 4)()
  spa3d._lib.check(lib.spa3d_plan_stats(h, st), h)
  ref_stats = list(st)
  got = _run(spa3d, model, dims, params, batch, noise, tc=100, qc=40, det=1, modes=modes)
  spa3d._lib.check(lib.spa3d_plan_stats(h, st), h)
  assert ref_stats[1] > ref_stats[0] > 0 and ref_stats[2] > 0, ref_stats  # pruning and shared rows both ran
  assert list(st)[:2] == ref_stats[:2], (list(st), ref_stats)  # plan stats count pass A once (the recompute does not add)
  assert _finite(got)
  bounds, measured = GATES16[precision]
  worst = _worst_leaf(got['grads'], ref['grads'])
  gt = Gates(f'{precision} track_chunk 100 / query_chunk 40 vs unchunked (B = 2, N = 300, Q = 96, T = 150, prune + ro_share)')
  gt.le('tracks, relative Frobenius', rel_err(got['train.tracks'], ref['train.tracks']), bounds[0], measured[0])
  gt.le('visible logits, relative Frobenius', rel_err(got['train.visible'], ref['train.visible']), bounds[1], measured[1])
  gt.le('total loss, relative', abs(float(got['loss'][0] - ref['loss'][0])) / abs(float(ref['loss'][0])), bounds[2], measured[2])
  gt.le(f'worst gradient leaf ({worst[1]})', worst[0], bounds[3], measured[3])
  gt.check()


def test_det_grads_with_both_options_is_bit_reproducible():
  import spa3d
  model, batch = _full(spa3d, 'bf16', seed=23)
  dims = model._dims_from_batch(batch)
  params = model.init(0, batch)['params']
  noise = torch.rand(2, 128, 96, generator=torch.Generator().manual_seed(8)).cuda()
  a = _run(spa3d, model, dims, params, batch, noise, tc=100, qc=40, det=1, modes=('train',))
  b = _run(spa3d, model, dims, params, batch, noise, tc=100, qc=40, det=1, modes=('train',))
  ref = _run(spa3d, model, dims, params, batch, noise, det=1, modes=('train',))
  assert _finite(a)
  assert torch.equal(a['loss'], b['loss']) and torch.equal(a['train.tracks'], b['train.tracks'])
  assert all(torch.equal(a['grads'][k], b['grads'][k]) for k in a['grads']), 'det_grads with intra-sample chunks is not bit-reproducible'
  e = abs(float(a['loss'][0] - ref['loss'][0])) / abs(float(ref['loss'][0]))
  assert e <= 1e-6, e


def test_poison_with_both_options_changes_nothing():
  import spa3d
  model, batch = _full(spa3d, 'bf16', seed=24)
  dims = model._dims_from_batch(batch)
  params = model.init(0, batch)['params']
  noise = torch.rand(2, 128, 96, generator=torch.Generator().manual_seed(9)).cuda()
  clean = _run(spa3d, model, dims, params, batch, noise, tc=100, qc=40, det=1)
  dirty = _run(spa3d, model, dims, params, batch, noise, tc=100, qc=40, det=1, poison=1)
  assert _finite(dirty)
  for k in clean:
    if k == 'grads':
      assert all(torch.equal(dirty['grads'][g], clean['grads'][g]) for g in clean['grads']), 'gradients changed under poison'
    else:
      assert torch.equal(dirty[k], clean[k]), f'{k} changed under poison'


def test_decoder_scan_chunk_size_is_real_and_must_divide_q():
  import spa3d
  model, batch = _mini(spa3d)
  dims = model._dims_from_batch(batch)
  params = model.init(0, batch)['params']
  noise = torch.rand(2, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(10)).cuda()
  ref = model({'params': params}, batch, noise=noise).tracks.clone()
  model.decoder_scan_chunk_size = 32   # 96 = 3 x 32: the handle now runs three query chunks
  model.track_chunk_size = 64
  got = model({'params': params}, batch, noise=noise).tracks.clone()
  h = model._handle(*dims)[0]
  assert rel_err(got, ref) <= 1e-6
  model.decoder_scan_chunk_size = 40   # does not divide 96
  torch.cuda.synchronize()
  with pytest.raises(ValueError):
    model({'params': params}, batch, noise=noise)
  with pytest.raises(ValueError):
    model.loss_and_grads({'params': params}, batch, noise=noise)
  model.decoder_scan_chunk_size = None
  model.track_chunk_size = None
  again = model({'params': params}, batch, noise=noise).tracks
  assert torch.equal(again, ref)  # back to the unchunked path
  del h


def test_cfg5_full_width_fp32_chunked_vs_fp16_default():
  """configs[4], one full sample: fp32 parity mode with track_chunk 1024 / query_chunk 256 against the fp16 default dispatch (gates of
  tests/test_gpu_cfg5_width.py's N = 4096 case, whose fp32 side could not run wider).  Fails without intra-sample chunking: the fp32 workspace
  request of one unchunked sample is refused."""
  import bench
  import spa3d
  Q, T = 2048, 300
  dev = torch.device('cuda', 0)
  batch = bench.synth_batch(1, 8192, Q, T, 768, 1, dev, seed=316, feat_dtype=torch.float16)
  noise = torch.rand(1, 128, 96, generator=torch.Generator().manual_seed(11)).to(dev)

  def run(precision, tc, qc):
    model = spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=768, depth_feature_dim=1, precision=precision,
                                     decoder_scan_chunk_size=qc, track_chunk_size=tc)
    b = dict(batch)
    b['dino_features'] = batch['dino_features'].to(CAST[precision]); b['depth_features'] = batch['depth_features'].to(CAST[precision])
    params = model.init(0, b)['params']
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ld, grads, preds = model.loss_and_grads({'params': params}, b, noise=noise, return_predictions=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = ([float(ld[k]) for k in ('total_loss', 'position_loss', 'visible_loss')], {k: v.clone() for k, v in O.tree_flatten(grads).items()},
           preds.tracks.clone(), preds.visible_logits.clone())
    print(f'configs[4] one sample, {precision} track_chunk={tc} query_chunk={qc}: {dt:.1f} s for loss_and_grads, workspace '
          f'{model._ws.numel() / 1e9:.1f} GB')
    del model, params, grads, preds, b
    torch.cuda.empty_cache()
    return out

  lo = run('fp16', None, None)
  ref = run('fp32', 1024, 256)
  (l16, g16, t16, v16), (l32, g32, t32, v32) = lo, ref
  assert all(bool(torch.isfinite(x).all()) for x in (t16, v16, t32, v32))
  assert all(bool(torch.isfinite(g32[k]).all()) for k in g32)
  names = sorted(g32)
  a = torch.cat([g16[k].double().reshape(-1) for k in names]); b_ = torch.cat([g32[k].double().reshape(-1) for k in names])
  cos = float((a @ b_) / (a.norm() * b_.norm()))
  tot = float(b_.norm())
  worst = max((rel_err(g16[k], g32[k]), k) for k in names if float(g32[k].double().norm()) > 1e-3 * tot)
  gt = Gates('cfg#5 FULL width (N = 8192, Q = 2048, T = 300): fp16 default dispatch vs the fp32 parity mode with intra-sample chunks')
  bounds, measured = (1.55e-3, 1.55e-3, 3.0e-5, 4.4e-2, 5.6e-6), ('1.03e-3 (N = 4096, round 5)', '1.03e-3', '2.0e-5', '2.9e-2', '3.7e-6')
  gt.le('tracks, relative Frobenius', rel_err(t16, t32), bounds[0], measured[0])
  gt.le('visible logits, relative Frobenius', rel_err(v16, v32), bounds[1], measured[1])
  gt.le('total loss, relative', abs(l16[0] - l32[0]) / abs(l32[0]), bounds[2], measured[2])
  gt.le(f'worst significant gradient leaf ({worst[1]})', worst[0], bounds[3], measured[3])
  gt.le('1 - cosine(whole gradient)', 1.0 - cos, bounds[4], measured[4])
  gt.check()
