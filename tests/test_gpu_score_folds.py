"""Leave-fold-out scoring on the GPU (include/spa3d.h: spa3d_score_folds, spa3d_op_attention_holdout; TrackAutoEncoder3D.score_all).

  1. The kernel: cross attention over shared keys with a per-sequence hole against spa3d_op_attention on a compacted copy of the keys, one sequence
     at a time -- o and lse bit for bit, bf16 / fp16 / fp32, holes at the start, across a chunk boundary, exactly one chunk, at the end, one row, empty.
  2. fp32 MINI against the fp64 oracle's forward on the cropped leave-out batch of every (clip, fold): max abs error below 1e-4 (the gate
     tests/test_gpu_ragged.py holds the fp32 mode to); score_predictions on the returned predictions gives the call's bits.
  3. Full width (T = 150, DINO 768 + depth, prune on) against model.score on the compacted batches -- the existing path.  fp32: the
     _compare_exactish gates of the ragged tests.  bf16 / fp16: no further from the fp32 mode's compacted calls than 1.5 x what the same-precision
     compacted calls are (measured inside the test); the direct difference is printed.
  4. The encoder ran once: spa3d_plan_stats.
  5. Invariants: two calls bit-equal, out = NULL, poison, NULL targets = explicit copies, query_frame = query_points, sample_stats = the pooled rows,
     F = 2 and F = N / 4, the smallest workspace (the readout one fold at a time) against all folds at once.
  6. Every refusal on a live handle, which still works afterwards.

Measured on one MI355X when the feature was added: profiles/r13_score_folds.log."""
import ctypes as C
import functools

import pytest
import torch

import folds_util as FU
import parity_util as PU
from util import MINI, Gates, O, batch_to, max_abs, product_model, rel_err

pytestmark = pytest.mark.gpu
CAST = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
CODE = {'fp32': 0, 'bf16': 1, 'fp16': 2}
FLOAT_SLOTS = (1, 2, 3, 4)   # of a query_stats row: sum y e1, sum y e2, max e2, sum bce (the others are integer counts)


def _s():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _set(spa3d, h, **opts):
  lib = spa3d._lib.load()
  for k, v in opts.items():
    spa3d._lib.check(lib.spa3d_set_option(h, k.encode(), float(v)), h, k)


def _perturb(params, seed=0, amt=0.1):
  g = torch.Generator().manual_seed(seed)
  for k, v in O.tree_flatten(params).items():
    if k.endswith('bias') or k.endswith('scale'):
      v.add_((amt * torch.randn(v.shape, generator=g)).to(v.device))


# ---------------------------------------------------------------------------------------------- 1. the kernel, bit for bit
HOLES = ((0, 37), (100, 140), (128, 256), (263, 300), (7, 8), (50, 50))


@pytest.mark.parametrize('Sq', [128, 5])
@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'fp32'])
def test_holdout_attention_is_the_compacted_call_bit_for_bit(precision, Sq):
  import spa3d
  lib = spa3d._lib.load()
  H, Dh, Nk, nseq = 2, 96, 300, len(HOLES)
  E, dt = H * Dh, CAST[precision]
  g = torch.Generator().manual_seed(17)
  q = torch.randn(nseq, Sq, E, generator=g).to(dt).cuda()
  k, v = torch.randn(Nk, E, generator=g).to(dt).cuda(), torch.randn(Nk, E, generator=g).to(dt).cuda()
  sq, sk = (1 + 0.2 * torch.randn(Dh, generator=g)).cuda(), (1 + 0.2 * torch.randn(Dh, generator=g)).cuda()
  o = PU.guarded(nseq * Sq, E, dt, name='o').view(nseq, Sq, E)
  lse = PU.guarded(nseq * H * Sq, 2, torch.float32, name='lse', fill=0.0).view(nseq, H, Sq, 2)
  ws = PU.poisoned_ws(32 << 20)
  holes = FU.i32([x for h in HOLES for x in h])
  assert lib.spa3d_op_attention_holdout(q.data_ptr(), k.data_ptr(), v.data_ptr(), E, E, E, sq.data_ptr(), sk.data_ptr(), nseq, Sq, Nk, H, Dh, holes,
                                        o.data_ptr(), lse.data_ptr(), CODE[precision], 0, ws.data_ptr(), ws.numel(), _s()) == 0
  bits = lambda t: t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)
  for i, (lo, hi) in enumerate(HOLES):
    n = Nk - (hi - lo)
    assert n != Sq   # the compacted call takes the chunked-key kernel too
    kc, vc = torch.cat([k[:lo], k[hi:]]).contiguous(), torch.cat([v[:lo], v[hi:]]).contiguous()
    o2 = PU.guarded(Sq, E, dt, name=f'o2[{i}]')
    lse2 = PU.guarded(H * Sq, 2, torch.float32, name=f'lse2[{i}]', fill=0.0).view(H, Sq, 2)
    ws.fill_(0xFF)
    assert lib.spa3d_op_attention(q[i].data_ptr(), kc.data_ptr(), vc.data_ptr(), E, E, E, sq.data_ptr(), sk.data_ptr(), None, 1, Sq, n, H, Dh, o2.data_ptr(),
                                  lse2.data_ptr(), CODE[precision], 0, ws.data_ptr(), ws.numel(), _s()) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(o2.float()).any(), f'hole {lo, hi}: the compacted call left NaN'
    assert torch.equal(bits(o[i]), bits(o2)), f'{precision} Sq = {Sq} hole [{lo}, {hi}): o differs, max |d| = {max_abs(o[i].float(), o2.float()):.3e}'
    assert torch.equal(bits(lse[i]), bits(lse2)), f'{precision} Sq = {Sq} hole [{lo}, {hi}): lse differs'
  if precision != 'fp32':   # (the generic composition does not write lse)
    assert bool(torch.isfinite(lse).all()) and float(lse.abs().sum()) > 0
  PU.check_guards()


# ---------------------------------------------------------------------------------------------- shared cases
@functools.lru_cache(maxsize=None)
def _mini(precision='fp32'):
  import spa3d
  cfg = O.Config(**MINI, use_dino=True, use_depth=True, dino_feature_dim=16, depth_feature_dim=1)
  model = product_model(spa3d, cfg, precision)
  raw = O.synthetic_batch(2, 200, 1, 8, seed=11, dino_dim=16, depth_dim=1)
  raw['boundary_frame'] = torch.tensor([8, 5], dtype=torch.int32)
  cpu, qf = FU.fold_batch(raw)
  batch = batch_to(cpu, 'cuda')
  params = model.init(0, batch)['params']
  _perturb(params)
  noise = torch.rand(2, cfg.num_latent_tokens, cfg.latent_token_dim, generator=torch.Generator().manual_seed(3))
  return cfg, model, cpu, batch, qf.cuda(), params, noise


@functools.lru_cache(maxsize=None)
def _full(precision):
  import bench
  import spa3d
  dev = torch.device('cuda', 0)
  model = spa3d.TrackAutoEncoder3D(num_output_frames=150, dino_feature_dim=768, depth_feature_dim=1, precision=precision)
  raw = bench.synth_batch(2, 300, 1, 150, 768, 1, dev, seed=41, feat_dtype=CAST[precision])
  raw['boundary_frame'] = torch.tensor([150, 97], dtype=torch.int32, device=dev)
  batch, qf = FU.fold_batch(raw)
  params = model.init(0, batch)['params']
  _set(spa3d, model._handle(768, 1)[0], prune=1)
  noise = torch.rand(2, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(1)).to(dev)
  return model, batch, qf, params, noise


def _compacted(model, params, batch, noise, off, thr=()):
  """The yardstick: model.score -- the existing path -- on the compacted leave-out batch of every (clip, fold), laid out as the fold call lays it out."""
  B, N = batch['support_tracks'].shape[:2]
  r = {}
  for b in range(B):
    for lo, hi in zip(off[:-1], off[1:]):
      sc = model.score({'params': params}, FU.leave_out(batch, b, lo, hi), thresholds=thr, return_predictions=True, frame_errors=True, noise=noise[b:b + 1])
      for key, t in (('tracks', sc.predictions.tracks), ('visible', sc.predictions.visible_logits), ('query_stats', sc.query_stats), ('frame_err', sc.frame_err)):
        r.setdefault(key, torch.zeros((B, N) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device))[b, lo:hi] = t[0]
  torch.cuda.synchronize()
  return r


def _as_dict(sc):
  return {'tracks': sc.predictions.tracks, 'visible': sc.predictions.visible_logits, 'query_stats': sc.query_stats, 'frame_err': sc.frame_err}


def _bit_equal(a, b, what):
  for name in ('query_stats', 'sample_stats', 'frame_err'):
    x, y = getattr(a, name), getattr(b, name)
    assert (x is None) == (y is None), f'{what}: {name}'
    if x is not None:
      assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), f'{what}: {name} differs (max |d| {float((x.double() - y.double()).abs().max()):.3e})'
  if a.predictions is not None and b.predictions is not None:
    assert torch.equal(a.predictions.tracks, b.predictions.tracks) and torch.equal(a.predictions.visible_logits, b.predictions.visible_logits), f'{what}: predictions differ'


def _pooled(sc, what):
  qs, ss = sc.query_stats.double(), sc.sample_stats
  want = qs.sum(1)
  want[:, 3] = qs[:, :, 3].max(1).values
  assert ss.dtype == torch.float64 and ss.shape == want.shape
  torch.testing.assert_close(ss, want, rtol=1e-12, atol=0, msg=lambda m: f'{what}: sample_stats is not the pooled rows: {m}')
  cols = [0, 5, 6, 7] + list(range(8, qs.shape[-1]))   # counts: integers, exact in double whatever the order
  assert torch.equal(ss[:, cols], want[:, cols]), what


# ---------------------------------------------------------------------------------------------- 2. fp32 MINI against the fp64 oracle
MINI_FOLDS = (0, 37, 165, 200)   # complements of 163, 72 and 165 keys: the hole at the start, in the middle, at the end; one complement is a single chunk


def test_fp32_mini_folds_vs_oracle_on_the_leave_out_batches():
  import spa3d
  cfg, model, cpu, batch, _, params, noise = _mini()
  thr = (0.05, 0.2)
  sc = model.score_all({'params': params}, batch, folds=list(MINI_FOLDS), thresholds=thr, frame_errors=True, return_predictions=True, noise=noise.cuda())
  torch.cuda.synchronize()
  B, N, T = 2, 200, 8
  assert sc.query_stats.shape == (B, N, 16) and sc.frame_err.shape == (B, N, T) and sc.predictions.tracks.shape == (B, N, T, 3)
  om = O.TrackAutoEncoder3D(cfg)
  p64 = O.tree_unflatten({k: v.detach().cpu().double() for k, v in O.tree_flatten(params).items()})
  b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in cpu.items()}
  for b in range(B):
    for lo, hi in zip(MINI_FOLDS[:-1], MINI_FOLDS[1:]):
      ref = om(p64, FU.leave_out(b64, b, lo, hi), discretize=True, noise=noise[b:b + 1].double())
      e_t = max_abs(sc.predictions.tracks[b, lo:hi], ref.tracks[0].detach())
      e_v = max_abs(sc.predictions.visible_logits[b, lo:hi], ref.visible_logits[0].detach())
      print(f'clip {b} fold [{lo}, {hi}) ({N - (hi - lo)} keys): max abs error tracks {e_t:.3e} visible logits {e_v:.3e}')
      assert e_t < 1e-4 and e_v < 1e-4
  assert float(sc.predictions.certain_logits.abs().max()) == 0.0
  tg = {'query_tracks': batch['support_tracks'], 'query_tracks_visible': batch['support_tracks_visible']}
  again = spa3d.score_predictions(sc.predictions, tg, thresholds=thr, frame_errors=True)
  _bit_equal(again, sc, 'score_predictions on the returned predictions')
  _pooled(sc, 'fp32 mini')


# ---------------------------------------------------------------------------------------------- 3. full width against the existing path
FULL_FOLDS = (0, 100, 140, 300)


@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'fp16'])
def test_full_width_folds_vs_score_on_the_compacted_batches(precision):
  import spa3d
  model, batch, _, params, noise = _full(precision)
  got = _as_dict(model.score_all({'params': params}, batch, folds=list(FULL_FOLDS), frame_errors=True, return_predictions=True, noise=noise))
  torch.cuda.synchronize()
  assert all(bool(torch.isfinite(t).all()) for t in got.values())
  uni = _compacted(model, params, batch, noise, FULL_FOLDS)
  fl = lambda r: r['query_stats'][..., list(FLOAT_SLOTS)]
  direct = {k: rel_err(got[k], uni[k]) for k in ('tracks', 'visible', 'frame_err')}
  direct['query_stats float slots'] = rel_err(fl(got), fl(uni))
  print(f'{precision}: score_all vs model.score on the compacted batches (B = 2, N = 300, T = 150, folds {FULL_FOLDS}), relative Frobenius: '
        + ', '.join(f'{k} {e:.3e}' for k, e in direct.items())
        + f'; bit-equal tracks: {torch.equal(got["tracks"], uni["tracks"])}, query_stats: {torch.equal(got["query_stats"], uni["query_stats"])}')
  if precision == 'fp32':
    assert direct['tracks'] <= 1e-6 and direct['visible'] <= 1e-6, direct
    a, b = fl(got).double(), fl(uni).double()
    worst = float(((a - b).abs() / b.abs().clamp_min(1e-30)).max())
    print(f'fp32: worst float slot of query_stats, relative: {worst:.3e}')
    assert bool(((a - b).abs() <= 1e-5 * b.abs()).all()), f'a float slot of query_stats is off by {worst:.3e} relative'
    return
  m32 = _full('fp32')[0]   # the same inputs: the feature planes as the 16-bit mode stores them, widened
  b32 = dict(batch, dino_features=batch['dino_features'].float(), depth_features=batch['depth_features'].float())
  ref32 = _compacted(m32, params, b32, noise, FULL_FOLDS)
  gt = Gates(f'{precision} score_all vs the fp32 parity mode\'s compacted calls; bound = 1.5 x the {precision} compacted calls\' error')
  for name, key in (('tracks, relative Frobenius', 'tracks'), ('visible logits, relative Frobenius', 'visible'), ('frame_err, relative Frobenius', 'frame_err')):
    e_u = rel_err(uni[key], ref32[key])
    gt.le(name, rel_err(got[key], ref32[key]), 1.5 * e_u, f'{precision} compacted calls: {e_u:.3e}')
  e_u = rel_err(fl(uni), fl(ref32))
  gt.le('query_stats float slots, relative Frobenius', rel_err(fl(got), fl(ref32)), 1.5 * e_u, f'{precision} compacted calls: {e_u:.3e}')
  gt.check()


# ---------------------------------------------------------------------------------------------- 4. the encoder ran once
def test_plan_stats_the_encoder_ran_once_per_clip():
  import spa3d
  model, batch, _, params, noise = _full('bf16')
  model.score_all({'params': params}, batch, folds=list(FULL_FOLDS), noise=noise)
  torch.cuda.synchronize()
  out4 = (C.c_double * 4)()
  assert spa3d._lib.load().spa3d_plan_stats(model._handle(768, 1)[0], out4) == 0
  B, N, T = 2, 300, 150
  print('plan stats after a fold call:', list(out4))
  assert out4[1] == B * N * (T + 1) and out4[3] == B * N
  assert 0 < out4[0] < out4[1]   # boundary_frame[1] = 97: pruning dropped the masked frame tokens


# ---------------------------------------------------------------------------------------------- 5. invariants
@pytest.mark.parametrize('case', ['fp32-mini', 'bf16-mini', 'bf16-full'])
def test_invariants(case):
  import spa3d
  precision, shape = case.split('-')
  if shape == 'mini':
    _, model, _, batch, qf, params, noise = _mini(precision)
    noise, dims, folds = noise.cuda(), (16, 1), list(MINI_FOLDS)
  else:
    model, batch, qf, params, noise = _full(precision)
    dims, folds = (768, 1), list(FULL_FOLDS)
  v = {'params': params}
  h = model._handle(*dims)[0]
  N = batch['support_tracks'].shape[1]
  thr = (0.05, 0.2)
  run = lambda b=batch, **kw: model.score_all(v, b, folds=kw.pop('folds', folds), thresholds=thr, frame_errors=True, noise=noise, **kw)
  first = run(return_predictions=True)
  torch.cuda.synchronize()
  assert all(bool(torch.isfinite(t).all()) for t in _as_dict(first).values())
  _pooled(first, case)
  _bit_equal(run(return_predictions=True), first, f'{case}: second call')
  lean = run()   # out = NULL
  assert lean.predictions is None
  _bit_equal(lean, first, f'{case}: out = NULL')
  _set(spa3d, h, poison=1)
  try:
    dirty = run(return_predictions=True)
    torch.cuda.synchronize()
  finally:
    _set(spa3d, h, poison=0)
  assert all(bool(torch.isfinite(t).all()) for t in _as_dict(dirty).values())
  _bit_equal(dirty, first, f'{case}: poison')
  explicit = dict(batch, query_tracks=batch['support_tracks'].clone(), query_tracks_visible=batch['support_tracks_visible'].clone())
  _bit_equal(run(explicit, return_predictions=True), first, f'{case}: explicit copies of the support tensors as targets')
  by_frame = {k: t for k, t in batch.items() if k != 'query_points'}
  by_frame['query_frame'] = qf
  _bit_equal(run(by_frame, return_predictions=True), first, f'{case}: query_frame instead of query_points')
  for F in (2, N // 4 if N // 4 <= 64 else 60):
    sc = run(folds=F, return_predictions=True)
    torch.cuda.synchronize()
    assert sc.query_stats.shape[:2] == (2, N) and all(bool(torch.isfinite(t).all()) for t in _as_dict(sc).values()), f'{case}: F = {F}'
    assert bool((sc.query_stats[..., 7] == model.num_output_frames).all()), f'{case}: F = {F}: a row was not scored'
    _pooled(sc, f'{case}: F = {F}')
  _bit_equal(run(return_predictions=True), first, f'{case}: after the other fold counts')
  if shape == 'mini':   # (the readout is the largest stage at this shape, so the smallest workspace forces one fold per readout group)
    lib = spa3d._lib.load()
    big = _as_dict(run(folds=3, return_predictions=True))
    floor = lib.spa3d_score_folds_workspace_bytes(h, N, 8, 3)
    assert 0 < floor < model._ws.numel()
    kept = model._ws, model._ws_cap
    model._ws, model._ws_cap = torch.empty(floor, dtype=torch.uint8, device='cuda'), floor   # score_all keeps a capped workspace that covers the floor
    try:
      small = _as_dict(run(folds=3, return_predictions=True))
      torch.cuda.synchronize()
      assert model._ws.numel() == floor
    finally:
      model._ws, model._ws_cap = kept
    # the same rows through GEMMs of other row counts: the fp32 gate of the ragged tests; 16-bit: at most one unit roundoff of the format
    tol = 1e-6 if precision == 'fp32' else PU.unit_roundoff(CAST[precision])
    for key in big:
      e = rel_err(small[key], big[key])
      print(f'{case}: readout one fold at a time ({floor} bytes) vs all folds at once ({kept[0].numel()} bytes): {key} relative Frobenius {e:.3e}')
      assert bool(torch.isfinite(small[key]).all()) and e <= tol, (key, e)


# ---------------------------------------------------------------------------------------------- 6. refusals on a live handle
def test_refusals_leave_the_handle_working():
  import spa3d
  cfg, model, _, batch, _, params, noise = _mini()
  v = {'params': params}
  before = model.score_all(v, batch, folds=list(MINI_FOLDS), frame_errors=True, noise=noise.cuda())
  h = model._handle(16, 1)[0]
  h2d = spa3d.TrackAutoEncoder(num_output_frames=8, precision='fp32')._handle(0, 0)[0]
  flat = model.flat_from_tree(params)
  N, T = 200, 8
  keep = []

  def make_batch():
    b, k = model._marshal({k: t for k, t in batch.items()}, 16, 1, noise=noise.cuda())
    keep.append(k)
    return b

  def make_scores():
    res, sc, _ = spa3d.model._alloc_scores((), 2, N, T, flat.device, None, False)
    keep.append(res)
    return sc

  ws = model._ws
  n = FU.check_refusals(spa3d, h, h2d, make_batch, make_scores, N, T, ws.data_ptr(), ws.numel(), flat.data_ptr())
  torch.cuda.synchronize()
  print(f'{n} refusals checked')
  after = model.score_all(v, batch, folds=list(MINI_FOLDS), frame_errors=True, noise=noise.cuda())
  _bit_equal(after, before, 'after the refusals')
