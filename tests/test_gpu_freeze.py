"""The "freeze" option of spa3d_loss_and_grads (include/spa3d.h, spa3d_set_option): the backward stops at a stage boundary of the flat parameter buffer.
Under det_grads every comparison with the unfrozen call is an identity: the forward results and the trainable gradients [lo, n) are the same bits, the
frozen prefix [0, lo) is zero -- or, with accumulate, exactly what the caller left there.

Two shapes: A, the mini config with B = 3, N = 6, Q = 5, T = 8 and chunk = 2 (a first chunk of one sample, a last chunk of two); B, the full-width model
(d = 384, eight 96-wide heads, default depths, DINO 768 + depth 1) with 16 output frames, B = 2, N = 32, Q = 16, T = 16, chunk = 1 and masked frames, where
token pruning, the shared readout rows and the fused kernels run."""
import ctypes as C

import pytest
import torch

from util import MINI, O, batch_to, product_model, rel_err

pytestmark = pytest.mark.gpu

COUNTS = ([6, 3, 5], [5, 0, 2])  # support_count, query_count of the ragged cases (shape A)
_cache = {}


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


def _perturbed(params, seed=0):
  g = torch.Generator().manual_seed(seed)
  for k, v in O.tree_flatten(params).items():
    if k.endswith('bias') or k.endswith('scale'):
      v.add_((0.1 * torch.randn(v.shape, generator=g)).to(v.device))
  return params


def _shape(name):
  """(cfg, batch on the CPU in fp32, noise, chunk, is 2-D) of a shape, built once"""
  if name in _cache:
    return _cache[name]
  if name == 'A':
    cfg = O.Config(**MINI, use_dino=True, use_depth=True, dino_feature_dim=24, depth_feature_dim=1)
    batch = O.synthetic_batch(3, 6, 5, 8, seed=1234, dino_dim=24, depth_dim=1)
    batch['boundary_frame'] = torch.tensor([8, 5, 3], dtype=torch.int32)
    chunk = 2
  elif name == 'B':
    cfg = O.Config(num_output_frames=16, use_dino=True, use_depth=True, dino_feature_dim=768, depth_feature_dim=1)
    batch = O.synthetic_batch(2, 32, 16, 16, seed=77, dino_dim=768, depth_dim=1)
    batch['boundary_frame'] = torch.tensor([16, 11], dtype=torch.int32)
    batch['support_tracks_visible'][:, ::3, 4:9] = 0  # masked frames inside the clip: their tokens are pruned
    batch['support_tracks_visible'][1, 5] = 0         # a track that is never visible
    chunk = 1
  else:  # the 2-D twin at mini size
    from test_trajan2d import MINI2D
    cfg = O.config_2d(**MINI2D)
    batch = O.synthetic_batch_2d(3, 6, 5, 8, seed=5)
    batch['boundary_frame'] = torch.tensor([8, 6, 2], dtype=torch.int32)
    chunk = 2
  g = torch.Generator().manual_seed(3)
  noise = torch.rand(batch['support_tracks'].shape[0], cfg.num_latent_tokens, cfg.latent_token_dim, generator=g)
  _cache[name] = (cfg, batch, noise, chunk, name == '2D')
  return _cache[name]


class Rig:
  """One model (one handle) on one shape in one precision, with det_grads on and its parameters on the device."""

  def __init__(self, spa3d, shape, precision):
    self.spa3d, self.lib = spa3d, spa3d._lib.load()
    cfg, batch, self.noise, self.chunk, twoD = _shape(shape)
    self.cfg = cfg
    if twoD:
      from test_trajan2d import _model
      self.model = _model(spa3d, cfg, precision)
    else:
      self.model = product_model(spa3d, cfg, precision)
    self.gb = batch_to(batch, 'cuda')
    if precision != 'fp32':
      for k in ('dino_features', 'depth_features'):
        if k in self.gb:
          self.gb[k] = self.gb[k].to(torch.bfloat16 if precision == 'bf16' else torch.float16)
    key = ('params', shape)
    if key not in _cache:  # the same parameters in every precision (fp32 leaves)
      _cache[key] = O.tree_map(lambda t: t.cpu(), _perturbed(self.model.init(0, self.gb)['params']))
    self.params = O.tree_map(lambda t: t.cuda(), _cache[key])
    self.dims = self.model._dims_from_params(self.params)
    self.h, self.leaves, self.n = self.model._handle(*self.dims)
    b4 = (C.c_int64 * 4)()
    assert self.lib.spa3d_grad_segments(self.h, b4) == 0
    self.seg = [int(x) for x in b4]
    self.noise = self.noise.cuda()

  def opt(self, **kw):
    for k, v in kw.items():
      self.spa3d._lib.check(self.lib.spa3d_set_option(self.h, k.encode(), float(v)), self.h, k)

  def run(self, k, grads_flat=None, accumulate=False, counts=None, **opts):
    """one training call at freeze = k -> (loss3 as floats, outputs, the flat gradient buffer, plan statistics)"""
    o = {'det_grads': 1, 'chunk': self.chunk, **opts}
    gb = dict(self.gb)
    if counts is not None:
      gb['support_count'] = torch.tensor(counts[0], dtype=torch.int32)
      gb['query_count'] = torch.tensor(counts[1], dtype=torch.int32)
    if grads_flat is None:
      grads_flat = torch.full((self.n,), float('nan'), device='cuda')  # whatever the call leaves unwritten shows
    self.opt(**o)
    try:
      ld, _, preds = self.model.loss_and_grads({'params': self.params}, gb, grads_flat=grads_flat, accumulate=accumulate, noise=self.noise,
                                               return_predictions=True, freeze=k)
      torch.cuda.synchronize()
      st = (C.c_double * 4)()
      assert self.lib.spa3d_plan_stats(self.h, st) == 0
    finally:
      self.opt(**{name: 0 for name in o})
    loss = tuple(float(ld[x]) for x in ('total_loss', 'position_loss', 'visible_loss'))
    outs = tuple(t.clone() for t in (preds.tracks, preds.visible_logits, preds.certain_logits))
    return loss, outs, grads_flat, tuple(st)

  def unit_abs_sum(self, counts=None, query_chunk=0):
    """(S, m): the launches of a training call that add into one element of the gradient buffer do so once per sample chunk (the latent stacks) or once per
    query chunk of a sample (the readout side).  The finest such units -- sample b cropped to its live tracks, with queries [q0, q1) -- are run alone here,
    unfrozen, against the batch's denominator; S = sum over the units of |gradient of the unit| bounds (triangle inequality) the sum of the magnitudes of
    whatever coarser groups of them a call adds, and m = the number of units bounds the number of additions an element receives."""
    B, N = self.gb['support_tracks'].shape[:2]
    Q = self.gb['query_tracks'].shape[1]
    live = [(counts[0][b] if counts else N, counts[1][b] if counts else Q) for b in range(B)]
    D = max(float(sum(self.gb['query_tracks_visible'][b, :q].double().sum() for b, (_, q) in enumerate(live))), 1.0)
    S, m = torch.zeros(self.n, device='cuda'), 0
    self.opt(det_grads=1, chunk=1)
    try:
      for b, (nb, q) in enumerate(live):
        for q0 in range(0, q, query_chunk or max(q, 1)):
          q1 = min(q, q0 + (query_chunk or q))
          unit = {}
          for name, v in self.gb.items():
            if name in ('support_tracks', 'support_tracks_visible', 'dino_features', 'depth_features'):
              unit[name] = v[b:b + 1, :nb].contiguous()
            elif name in ('query_points', 'query_tracks', 'query_tracks_visible'):
              unit[name] = v[b:b + 1, q0:q1].contiguous()
            else:
              unit[name] = v[b:b + 1].contiguous()
          g = torch.zeros(self.n, device='cuda')
          self.model.loss_and_grads({'params': self.params}, unit, grads_flat=g, denom=D, noise=self.noise[b:b + 1].contiguous())
          S += g.abs()
          m += 1
      torch.cuda.synchronize()
    finally:
      self.opt(det_grads=0, chunk=0)
    return S, m


def _rig(spa3d, shape, precision):
  key = ('rig', shape, precision)
  if key not in _cache:
    _cache[key] = Rig(spa3d, shape, precision)
  return _cache[key]


def _reference(rig, shape, precision, tag='', **kw):
  """the unfrozen call on the same handle with the same options: computed once, shared, never written to"""
  key = ('ref', shape, precision, tag)
  if key not in _cache:
    _cache[key] = rig.run(0, **kw)
  return _cache[key]


def _units(rig, shape, precision, tag='', counts=None, query_chunk=0):
  key = ('units', shape, precision, tag)
  if key not in _cache:
    _cache[key] = rig.unit_abs_sum(counts, query_chunk)
  return _cache[key]


def _bits(t):
  return t.contiguous().view(torch.int32)


def _pattern(n):
  return torch.sin(torch.arange(n, device='cuda', dtype=torch.float32)) * 3e-3 + 1e-3


def _check_against_unfrozen(rig, ref, k, what, accumulate=True, units=None, **kw):
  """test 5's checks of one frozen call against the unfrozen one.  units: (S, m) of Rig.unit_abs_sum for the call's batch and options"""
  lo, n = rig.seg[k], rig.n
  loss0, outs0, g0, stats0 = ref
  loss, outs, g, stats = rig.run(k, **kw)
  assert loss == loss0, (what, loss, loss0)
  for a, b in zip(outs, outs0):
    assert torch.equal(_bits(a), _bits(b)), f'{what}: outputs differ from the unfrozen call'
  assert stats == stats0, (what, stats, stats0)
  assert torch.isfinite(g0).all(), what
  assert torch.equal(_bits(g[lo:]), _bits(g0[lo:])), f'{what}: {int((_bits(g[lo:]) != _bits(g0[lo:])).sum())} trainable gradients differ'
  assert int(_bits(g[:lo]).count_nonzero()) == 0, f'{what}: the frozen range is not all zero bits'
  assert float(g0[:lo].abs().max()) > 0 and float(g0[lo:].abs().max()) > 0  # the comparison is not between zeros
  if not accumulate:
    return
  pattern = _pattern(n)
  _, _, acc, _ = rig.run(k, grads_flat=pattern.clone(), accumulate=True, **kw)
  assert torch.equal(_bits(acc[:lo]), _bits(pattern[:lo])), f'{what}: accumulate touched the frozen range'
  # "The pattern plus the gradient, within one fp32 addition".  The buffer receives the gradient in up to m additions per element -- the fixed-point sums in one,
  # when they are flushed, but a dW GEMM that owns its output tile adds its product straight into the buffer, once per chunk -- and each is ONE fp32 addition:
  # it rounds by at most 2^-24 of its result, which is at most |pattern| + S (S: the summed magnitudes of the addends, Rig.unit_abs_sum).  The unfrozen
  # gradient g0 went through the same m additions from zero, and pattern + g0 below is one more.  So |acc - (pattern + g0)| <= 2 m 2^-24 (|pattern| + S).
  S, m = units
  want = pattern[lo:] + g0[lo:]
  err = (acc[lo:] - want).abs()
  tol = m * 2.0 ** -23 * (pattern[lo:].abs() + S[lo:])
  worst = float((err / tol).max())
  print(f'{what}: accumulate: worst |acc - (pattern + gradient)| / bound = {worst:.3f} (m = {m} additions)')
  if not bool((err <= tol).all()):
    bad = (err > tol).nonzero().flatten() + lo
    names = sorted({next(nm for nm, _, off in reversed(rig.leaves) if off <= int(i)) for i in bad[:2000]})
    i = int(bad[int((err / tol)[bad - lo].argmax())])
    raise AssertionError(f'{what}: accumulate: {bad.numel()} elements beyond the bound in leaves {names[:12]}; worst at {i}: got {float(acc[i])!r}, '
                         f'pattern {float(pattern[i])!r} + gradient {float(g0[i])!r}, bound {float(tol[i - lo])!r}')


# ---------------------------------------------------------------------------------------------- 5: bit-equality under det_grads
@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'fp32'])
@pytest.mark.parametrize('shape', ['A', 'B'])
def test_frozen_call_equals_unfrozen_bit_for_bit(spa3d, shape, precision, k):
  rig = _rig(spa3d, shape, precision)
  ref = _reference(rig, shape, precision)
  if shape == 'B' and precision != 'fp32':  # the shape does what it is here for: masked frame tokens are pruned from the track encoder
    assert 0 < ref[3][0] < ref[3][1] and ref[3][3] > 0, ref[3]
  # accumulate = 1 is refused with a loss scale (fp16), as it is without the option
  acc = precision != 'fp16'
  _check_against_unfrozen(rig, ref, k, f'shape {shape} {precision} freeze {k}', accumulate=acc, units=_units(rig, shape, precision) if acc else None)


# ---------------------------------------------------------------------------------------------- 6: fp32 against the float64 oracle
@pytest.mark.parametrize('k', [1, 2])
def test_trainable_leaves_meet_the_oracle_gate_fp32(spa3d, k):
  """The gate of tests/test_gpu_model.py::_mini_fp32 for the full backward -- relative error of every leaf below 2e-3 against the float64 oracle under
  autograd -- on the leaves of the trainable range; the frozen leaves are zero."""
  rig = _rig(spa3d, 'A', 'fp32')
  cfg, batch, noise, _, _ = _shape('A')
  key = ('oracle', 'A')
  if key not in _cache:
    p64 = O.tree_unflatten({name: v.detach().cpu().double() for name, v in O.tree_flatten(rig.params).items()})
    b64 = {name: (v.double() if v.is_floating_point() else v) for name, v in batch.items()}
    _cache[key] = O.loss_and_grads(O.TrackAutoEncoder3D(cfg), p64, b64, discretize=True, noise=noise.double())
  ld_ref, _, grads_ref = _cache[key]
  loss, _, g, _ = rig.run(k)
  assert abs(loss[0] - float(ld_ref['total_loss'])) <= 1e-5 * abs(float(ld_ref['total_loss'])) + 1e-7
  lo, worst, trained = rig.seg[k], 0.0, 0
  for name, shape, off in rig.leaves:
    cnt = 1
    for s in shape:
      cnt *= int(s)
    got, gref = g[off:off + cnt].reshape(tuple(shape)), grads_ref[name]
    if off < lo:
      assert float(got.abs().max()) == 0.0, name
      continue
    e = rel_err(got, gref) if float(gref.norm()) > 1e-12 else float(got.abs().max())
    worst, trained = max(worst, e), trained + 1
    assert e < 2e-3, (name, e)
  assert 0 < trained < len(rig.leaves)
  print(f'freeze {k}: {trained} trainable leaves, worst relative error {worst:.3e} against the oracle (bound 2e-3)')


# ---------------------------------------------------------------------------------------------- 7: the options a training call accepts
MATRIX = {
    'query_chunk': dict(opts=dict(query_chunk=2, chunk=0)),
    'track_chunk': dict(opts=dict(track_chunk=4, chunk=0)),
    'ragged-packed': dict(counts=COUNTS, opts=dict(chunk=2)),
    'ragged-alone': dict(counts=COUNTS, opts=dict(chunk=1)),
    'poison': dict(opts=dict(poison=1)),
}


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
@pytest.mark.parametrize('case', sorted(MATRIX))
def test_options_matrix(spa3d, case, precision, k):
  rig = _rig(spa3d, 'A', precision)
  kw = dict(counts=MATRIX[case].get('counts'), **MATRIX[case]['opts'])
  ref = _reference(rig, 'A', precision, tag=case, **kw)
  units = _units(rig, 'A', precision, tag=case, counts=kw['counts'], query_chunk=kw.get('query_chunk', 0))
  _check_against_unfrozen(rig, ref, k, f'{case} {precision} freeze {k}', units=units, **kw)


def test_two_d_twin(spa3d):
  rig = _rig(spa3d, '2D', 'fp32')
  assert rig.seg[1] > 0
  _check_against_unfrozen(rig, _reference(rig, '2D', 'fp32'), 1, '2-D twin fp32 freeze 1', units=_units(rig, '2D', 'fp32'))


# ---------------------------------------------------------------------------------------------- 8: no stale state
def test_unfrozen_call_after_a_frozen_one_is_a_fresh_one(spa3d):
  used = Rig(spa3d, 'B', 'bf16')
  used.run(2)
  after = used.run(0)
  fresh = Rig(spa3d, 'B', 'bf16').run(0)
  assert after[0] == fresh[0] and after[3] == fresh[3]
  assert torch.equal(_bits(after[2]), _bits(fresh[2])), 'a freeze 2 call left something behind on the handle'


# ---------------------------------------------------------------------------------------------- 9: gradient-segment events
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_events_are_recorded_once_and_not_early(spa3d, precision):
  rig = _rig(spa3d, 'A', precision)
  lib, h = rig.lib, rig.h
  g0 = _reference(rig, 'A', precision)[2]  # no events registered: one flush / one unscaling at the end of the call
  evs = (torch.cuda.Event(), torch.cuda.Event())
  for e in evs:
    e.record()
  torch.cuda.synchronize()
  side = torch.cuda.Stream()
  assert lib.spa3d_set_grad_events(h, C.c_void_p(evs[0].cuda_event), C.c_void_p(evs[1].cuda_event)) == 0
  try:
    for k in (0, 1, 2):
      g4 = (C.c_int64 * 4)()
      assert lib.spa3d_grad_events_recorded(h, g4) == 0
      before = (int(g4[0]), int(g4[1]))
      rig.opt(det_grads=1, chunk=rig.chunk)
      grads = torch.full((rig.n,), float('nan'), device='cuda')
      rig.model.loss_and_grads({'params': rig.params}, rig.gb, grads_flat=grads, noise=rig.noise, freeze=k)
      # the call has enqueued its work and returned; behind the LATER event everything from the latent stacks' boundary up is final (k = 0: the
      # track encoder's segment is still being written), so a copy on a stream that waits for nothing else must already see the final bits
      lo = max(rig.seg[k], rig.seg[1])
      evs[1].synchronize()
      with torch.cuda.stream(side):
        snap = grads[lo:].clone()
      torch.cuda.synchronize()
      assert lib.spa3d_grad_events_recorded(h, g4) == 0
      assert (int(g4[0]), int(g4[1])) == (before[0] + 1, before[1] + 1), (k, before, tuple(g4))
      assert evs[0].query() and evs[1].query()
      assert torch.equal(_bits(snap), _bits(g0[lo:])), f'{precision} freeze {k}: the range behind the latents event was not final (fp16: not unscaled) at the event'
      assert torch.equal(_bits(grads[rig.seg[k]:]), _bits(g0[rig.seg[k]:])) and int(_bits(grads[:rig.seg[k]]).count_nonzero()) == 0
  finally:
    rig.opt(det_grads=0, chunk=0)
    lib.spa3d_set_grad_events(h, None, None)


# ---------------------------------------------------------------------------------------------- 10: TrainState on the device
def test_trainstate_freeze_1_equals_the_manual_route(spa3d):
  rig = Rig(spa3d, 'A', 'bf16')
  lib, model, b1, n = rig.lib, rig.model, rig.seg[1], rig.n
  hp = dict(learning_rate=1e-2, warmup_steps=1, total_steps=10)
  rig.opt(det_grads=1, chunk=rig.chunk)
  try:
    st = spa3d.TrainState(model, O.tree_map(lambda t: t.clone(), rig.params), freeze=1, **hp)
    st.m[:b1] = 0.25; st.v[:b1] = 0.5  # (a resumed state's moments: untouched is more than staying zero)
    start = [t.clone() for t in (st.flat, st.m, st.v)]
    flat, m, v = [t.clone() for t in start]
    g, scratch = torch.zeros(n, device='cuda'), torch.zeros(1024, device='cuda')
    sched = spa3d.create_learning_rate_schedule(hp['learning_rate'], hp['warmup_steps'], hp['total_steps'])
    stream = torch.cuda.current_stream().cuda_stream
    for step in range(3):
      mt = st.train_step(rig.gb, noise=rig.noise)
      # the manual route: the unfrozen gradient, its frozen part zeroed, AdamW on the slices
      model.loss_and_grads({'params': model.tree_from_flat(flat, *rig.dims)}, rig.gb, grads_flat=g, noise=rig.noise, freeze=0)
      assert float(g[:b1].abs().max()) > 0
      g[:b1] = 0
      assert lib.spa3d_adamw_step(flat[b1:].data_ptr(), g[b1:].data_ptr(), m[b1:].data_ptr(), v[b1:].data_ptr(), n - b1, sched(step), step, st.clip, st.b1,
                                  st.b2, st.eps, st.wd, scratch.data_ptr(), C.c_void_p(stream)) == 0
      torch.cuda.synchronize()
      assert float(mt['train/grad_norm']) == float(scratch[0]) > 0  # the norm of the trainable range
      for name, a, b in (('parameters', st.flat, flat), ('m', st.m, m), ('v', st.v, v)):
        assert torch.equal(_bits(a[b1:]), _bits(b[b1:])), f'step {step}: trainable {name} differ from the manual route'
    for name, a, b in zip(('parameters', 'm', 'v'), (st.flat, st.m, st.v), start):
      assert torch.equal(_bits(a[:b1]), _bits(b[:b1])), f'frozen {name} changed'
      assert not torch.equal(a[b1:], b[b1:]), f'trainable {name} did not move'
    st.close()
  finally:
    rig.opt(det_grads=0, chunk=0)
