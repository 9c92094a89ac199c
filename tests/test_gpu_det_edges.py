"""Edges of the deterministic-gradient mode (spa3d_set_option "det_grads", include/spa3d.h) that tests/test_gpu_det.py does not reach:

- the mode must not outlive the train call that used it: an op backward (spa3d_op_*_bwd) that runs after a det_grads call and writes into the range of that
  call's gradient buffer must still produce its full result (the caller's workspace, which held the shadow, stays alive here on purpose so that a shadow that
  outlived its call shows up as a wrong answer, never as a stray write);
- the mode belongs to one handle: two handles training at the same time on two streams of one process keep each its own mode (bit-equal det_grads gradients);
- a gradient beyond the fixed-point range must come out NaN, never as a finite value of the wrong sign or size (loss denominators far below the visible count
  drive every gradient up by the same factor, without touching the model);
- the fixed-point unit follows denom / (visible count of the call): a denominator far above the call's own visible count (a small batch under a large global
  denominator) must not round the small-norm leaves away.  At a real batch the two are about equal and the unit is 2^-32 as before (include/spa3d.h).

Every comparison is against the float-atomic run of the same call (det_grads 0) or against an fp64 reference of the op."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

from util import O, batch_to, product_model, rel_err

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_t150_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
Q1_LEAVES = ('track_readout_attn/layer_3/self_att/norm_query/scale', 'track_readout_attn/layer_3/self_att/norm_key/scale')  # single-query attention backward


def _s():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ws(nbytes=256 << 20):
  return torch.empty(nbytes, dtype=torch.uint8, device='cuda')


def _gpu_batch(batch, precision):
  gb = batch_to(batch, 'cuda')
  if precision != 'fp32':
    for k in ('dino_features', 'depth_features'):
      gb[k] = gb[k].to(torch.bfloat16 if precision == 'bf16' else torch.float16)
  return gb


@pytest.fixture(scope='module')
def c772():
  cfg, p, batch, noise = G.make_inputs('c772')
  return cfg, O.tree_map(lambda t: t.cuda(), p), batch, noise.cuda()


# ------------------------------------------------------------------------------------------------ A1: the mode does not outlive its train call
class DetCall:
  """One det_grads train call through the C ABI (model.loss_and_grads without the wrapper), with the gradient buffer G and the workspace owned here and kept
  alive until the test ends: when the mode was a device-side switch that a call cleared at its end, a stale shadow pointer pointed into this very workspace.
  run=False: handle, G and workspace only, calls issued with enqueue() (the mode stays set)."""

  def __init__(self, spa3d, inputs, precision='bf16', det=1, run=True):
    cfg, gp, batch, noise = inputs
    self.model = product_model(spa3d, cfg, precision)
    self.spa3d, self.lib = spa3d, spa3d._lib.load()
    dino, depth = self.model._dims_from_params(gp)
    self.h, self.leaves, n = self.model._handle(dino, depth)
    spa3d._lib.check(self.lib.spa3d_set_option(self.h, b'det_grads', float(det)), self.h)
    self.flat = self.model.flat_from_tree(gp)
    self.b, self.keep = self.model._marshal(_gpu_batch(batch, precision), dino, depth, targets=True, discretize=True, noise=noise)
    self.G = torch.zeros(n, dtype=torch.float32, device='cuda')
    self.loss3 = torch.empty(4, dtype=torch.float32, device='cuda')
    self.ws = self.model._workspace(self.h, self.b.B, self.b.N, self.b.Q, self.b.T, True, self.G.device)
    self.n = n
    if run:
      self.enqueue(_s())
      torch.cuda.synchronize()
      spa3d._lib.check(self.lib.spa3d_set_option(self.h, b'det_grads', 0.0), self.h)

  def enqueue(self, stream):
    self.spa3d._lib.check(self.lib.spa3d_loss_and_grads(self.h, self.flat.data_ptr(), C.byref(self.b), 0.0, self.G.data_ptr(), 0, self.loss3.data_ptr(), None,
                                                        self.ws.data_ptr(), self.ws.numel(), stream), self.h, 'spa3d_loss_and_grads')

  def view(self, offset, numel):
    assert 0 <= offset and offset + numel <= self.n
    return self.G[offset:offset + numel]


def _offsets(n, numel):
  return (0, (n // 2 - numel // 2) // 64 * 64)


def _linear_bwd_into(lib, call, M, N, K, impl):
  g = torch.Generator().manual_seed(12)
  A = torch.randn(M, K, generator=g).bfloat16()
  dC = torch.randn(M, N, generator=g).bfloat16()
  B = (torch.randn(K, N, generator=g) / math.sqrt(K)).bfloat16()
  Ad, Bd, dCd = A.cuda(), B.cuda(), dC.cuda()
  rB = A.double().T @ dC.double()
  rb = dC.double().sum(0)
  ws = _ws()
  for off in _offsets(call.n, K * N):
    dB = call.view(off, K * N)
    dB.fill_(float('nan'))
    rc = lib.spa3d_op_linear_bwd(Ad.data_ptr(), Bd.data_ptr(), dCd.data_ptr(), None, dB.data_ptr(), None, M, N, K, BF16, impl, ws.data_ptr(), ws.numel(), _s())
    assert rc == 0
    e = rel_err(dB.view(K, N), rB)
    print(f'linear_bwd impl {impl} {M}x{N}x{K}: dB at G+{off}: rel err {e:.3e}')
    assert e < 1e-5, f'dB written into the range of the last det_grads call lost contributions (offset {off}): rel err {e}'
    db = call.view(off, N)
    db.fill_(float('nan'))
    rc = lib.spa3d_op_linear_bwd(Ad.data_ptr(), Bd.data_ptr(), dCd.data_ptr(), None, None, db.data_ptr(), M, N, K, BF16, impl, ws.data_ptr(), ws.numel(), _s())
    assert rc == 0
    e = rel_err(db, rb)
    assert e < 1e-5, f'dbias written into the range of the last det_grads call lost contributions (offset {off}): rel err {e}'


@pytest.mark.parametrize('impl', [2, 3, 9])
@pytest.mark.parametrize('M,N,K', [(5000, 384, 256), (70001, 384, 768)])
def test_linear_bwd_after_a_det_grads_call(c772, M, N, K, impl):
  import spa3d
  call = DetCall(spa3d, c772)
  _linear_bwd_into(spa3d._lib.load(), call, M, N, K, impl)


@pytest.mark.parametrize('dtype,d', [(F32, 384), (F32, 1280), (BF16, 384), (BF16, 1152)])
def test_layernorm_bwd_after_a_det_grads_call(c772, dtype, d):
  import spa3d
  call = DetCall(spa3d, c772)
  lib = spa3d._lib.load()
  rows = 5000
  dt = torch.float32 if dtype == F32 else torch.bfloat16
  g = torch.Generator().manual_seed(3)
  x = (torch.randn(rows, d, generator=g) * 2 + 0.5).to(dt)
  scale = 1 + 0.1 * torch.randn(d, generator=g)
  dy = torch.randn(rows, d, generator=g).to(dt)
  xd, sd, dyd = x.cuda(), scale.cuda(), dy.cuda()
  y = torch.empty_like(xd)
  stats = torch.empty(rows, 2, device='cuda')
  assert lib.spa3d_op_layernorm(xd.data_ptr(), sd.data_ptr(), y.data_ptr(), stats.data_ptr(), rows, d, dtype, _s()) == 0
  sr = scale.double().requires_grad_(True)
  O.layer_norm(x.double(), sr).backward(dy.double())
  dx = torch.empty_like(xd)
  for off in _offsets(call.n, d):
    ds = call.view(off, d)
    ds.zero_()
    assert lib.spa3d_op_layernorm_bwd(xd.data_ptr(), sd.data_ptr(), stats.data_ptr(), dyd.data_ptr(), dx.data_ptr(), ds.data_ptr(), rows, d, dtype,
                                      _s()) == 0
    e = rel_err(ds, sr.grad)
    print(f'layernorm_bwd dtype {dtype} d {d}: dscale at G+{off}: rel err {e:.3e}')
    assert e < (1e-5 if dtype == F32 else 1e-2), f'dscale written into the range of the last det_grads call (offset {off}): rel err {e}'


def _attn_ref(q, k, v, sq, sk, km, H, Dh):
  nseq, Sq, _ = q.shape
  Sk = k.shape[1]
  qh = O.rms_norm(q.view(nseq, Sq, H, Dh), sq)
  kh = O.rms_norm(k.view(nseq, Sk, H, Dh), sk)
  vh = v.view(nseq, Sk, H, Dh)
  mask = None if km is None else km[:, None, None, :].expand(nseq, H, Sq, Sk)
  return O.dot_product_attention(qh, kh, vh, mask).reshape(nseq, Sq, H * Dh)


@pytest.mark.parametrize('dtype,impl,nseq,S,H', [(F32, 1, 5, 25, 8), (BF16, 1, 5, 25, 8), (BF16, 2, 17, 151, 8)])
def test_attention_bwd_scale_grads_after_a_det_grads_call(c772, dtype, impl, nseq, S, H):
  """The scale gradients d s_q, d s_k of the attention backward (generic impl 1, fused impl 2) written into the range of the last det_grads call."""
  import spa3d
  call = DetCall(spa3d, c772)
  lib = spa3d._lib.load()
  Dh = 96
  E = H * Dh
  dt = torch.float32 if dtype == F32 else torch.bfloat16
  g = torch.Generator().manual_seed(21)
  qkv = torch.randn(nseq, S, 3 * E, generator=g).to(dt)
  sq = 1 + 0.2 * torch.randn(Dh, generator=g)
  sk = 1 + 0.2 * torch.randn(Dh, generator=g)
  km = (torch.rand(nseq, S, generator=g) < 0.8).float()
  km[:, 0] = 1.0
  d_o = torch.randn(nseq, S, E, generator=g).to(dt)
  qkvd, sqd, skd, kmd, dod = qkv.cuda(), sq.cuda(), sk.cuda(), km.cuda(), d_o.cuda()
  o = torch.empty(nseq, S, E, device='cuda', dtype=dt)
  lse = torch.zeros(nseq, H, S, 2, device='cuda')
  ws = _ws(512 << 20)
  ptr = lambda t, i: t[..., i * E:(i + 1) * E].data_ptr()  # noqa: E731
  assert lib.spa3d_op_attention(ptr(qkvd, 0), ptr(qkvd, 1), ptr(qkvd, 2), 3 * E, 3 * E, 3 * E, sqd.data_ptr(), skd.data_ptr(), kmd.data_ptr(), nseq, S, S,
                                H, Dh, o.data_ptr(), lse.data_ptr(), dtype, impl, ws.data_ptr(), ws.numel(), _s()) == 0
  qr, kr, vr = (qkv[..., i * E:(i + 1) * E].double().contiguous() for i in range(3))
  sqr, skr = sq.double().requires_grad_(True), sk.double().requires_grad_(True)
  _attn_ref(qr, kr, vr, sqr, skr, km, H, Dh).backward(d_o.double())
  dqkv = torch.zeros(nseq, S, 3 * E, device='cuda', dtype=dt)
  bound = 1e-4 if dtype == F32 else 3e-2
  for off in _offsets(call.n, 2 * Dh):
    dsc = call.view(off, 2 * Dh)
    dsc.zero_()
    assert lib.spa3d_op_attention_bwd(ptr(qkvd, 0), ptr(qkvd, 1), ptr(qkvd, 2), 3 * E, 3 * E, 3 * E, sqd.data_ptr(), skd.data_ptr(), kmd.data_ptr(), nseq,
                                      S, S, H, Dh, o.data_ptr() if impl != 1 else None, lse.data_ptr() if impl != 1 else None, dod.data_ptr(),
                                      ptr(dqkv, 0), ptr(dqkv, 1), ptr(dqkv, 2), dsc[:Dh].data_ptr(), dsc[Dh:].data_ptr(), dtype, impl, ws.data_ptr(),
                                      ws.numel(), _s()) == 0
    e = (rel_err(dsc[:Dh], sqr.grad), rel_err(dsc[Dh:], skr.grad))
    print(f'attention_bwd dtype {dtype} impl {impl}: d s_q, d s_k at G+{off}: rel errs {e[0]:.3e} {e[1]:.3e}')
    assert max(e) < bound, f'scale gradients written into the range of the last det_grads call (offset {off}): rel errs {e}'


def test_op_after_a_det_call_and_a_plain_call_on_another_handle(c772):
  """det_grads train call on one handle, plain train call on a second one, then an op backward: the op sees float atomics whatever the order of the calls.
  A regression guard for the order independence, not a reproduction of the stale mode: when the mode was a device-side switch, the plain call stated it off
  at its start, so this passed before the switch was cleared at the end of a det_grads call too."""
  import spa3d
  call = DetCall(spa3d, c772, 'bf16', det=1)
  plain = DetCall(spa3d, c772, 'fp32', det=0)
  assert plain.model is not call.model
  _linear_bwd_into(spa3d._lib.load(), call, 5000, 384, 256, 2)


@pytest.mark.parametrize('prec_a,prec_b,det_b', [('fp32', 'fp32', 1), ('fp32', 'bf16', 1), ('fp32', 'fp32', 0)])
def test_two_handles_on_two_streams(c772, prec_a, prec_b, det_b):
  """Two handles train at the same time on two streams of one process (include/spa3d.h: one handle per stream), four calls each, alternating, with no host
  synchronisation in between: handle A (det_grads 1) must give the bits of its solo run in every call, handle B those of its solo run with det_grads 1, or
  stay within the float-atomic gate of tests/test_gpu_det.py with det_grads 0.  A is fp32, which reads nothing back mid-call, so the host runs whole calls
  ahead of the device and the two streams overlap.  When the mode was a process-wide device variable, B's call stated B's mode between A's kernels.
  A regression guard: whether calls overlap depends on timing."""
  import spa3d
  calls = (DetCall(spa3d, c772, prec_a, det=1, run=False), DetCall(spa3d, c772, prec_b, det=det_b, run=False))
  solo = []
  for call in calls:
    call.enqueue(_s())
    torch.cuda.synchronize()
    solo.append(call.G.clone())
  streams = (torch.cuda.Stream(), torch.cuda.Stream())
  got = ([], [])
  for _ in range(4):
    for call, st, out in zip(calls, streams, got):
      call.enqueue(C.c_void_p(st.cuda_stream))
      with torch.cuda.stream(st):
        out.append(call.G.clone())   # in stream order: after this call, before the next one zeroes G
  torch.cuda.synchronize()
  for name, call, det, ref, out in zip('AB', calls, (1, det_b), solo, got):
    for i, g in enumerate(out):
      if det:
        diff = [k for k, shape, off in call.leaves if not torch.equal(g[off:off + math.prod(shape)], ref[off:off + math.prod(shape)])]
        assert not diff, f'handle {name} ({call.model.precision}, det_grads) call {i}: {len(diff)} leaves differ from its solo run, e.g. {diff[:3]}'
      else:
        worst = max((rel_err(g[off:off + math.prod(shape)], ref[off:off + math.prod(shape)]), k) for k, shape, off in call.leaves
                    if float(ref[off:off + math.prod(shape)].double().norm()) > 0)
        print(f'handle {name} ({call.model.precision}, float atomics) call {i}: worst leaf vs its solo run {worst}')
        assert worst[0] < 5e-5, f'handle {name} call {i}: {worst}'


# ------------------------------------------------------------------------------------------------ A2 / A3: range and resolution of the fixed point
def _grads(spa3d, inputs, precision, det, denom, loss_scale=None):
  cfg, gp, batch, noise = inputs
  model = product_model(spa3d, cfg, precision)
  h = model._handle(*model._dims_from_params(gp))[0]
  lib = spa3d._lib.load()
  spa3d._lib.check(lib.spa3d_set_option(h, b'det_grads', float(det)), h)
  if loss_scale is not None:
    spa3d._lib.check(lib.spa3d_set_option(h, b'loss_scale', float(loss_scale)), h)
  _, grads, _ = model.loss_and_grads({'params': gp}, _gpu_batch(batch, precision), denom=float(denom), noise=noise)
  torch.cuda.synchronize()
  spa3d._lib.check(lib.spa3d_set_option(h, b'det_grads', 0.0), h)
  return O.tree_flatten(grads)


def _leaf_max(g):
  return max(float(v.abs().max()) for v in g.values() if torch.isfinite(v).all())


def _agree_or_nan(det, ref, what, leaves=None):
  """Per leaf: every element either NaN, or within 1e-3 |ref| + 1e-4 max|leaf| of the float-atomic result, and the finite part of the leaf within 5e-5
  relative.  Elements whose float-atomic reference is not finite (16-bit activation overflow) are not judged."""
  bad, nan_leaves = [], 0
  for k in (leaves or sorted(ref)):
    a, d = ref[k].double(), det[k].double()
    fin = torch.isfinite(a) & ~torch.isnan(d)
    if bool(torch.isnan(d).any()):
      nan_leaves += 1
    if not bool(fin.any()):
      continue
    a, d = a[fin], d[fin]
    amax = float(a.abs().max())
    err = (d - a).abs()
    worst = float((err - 1e-3 * a.abs()).max())
    rel = float((d - a).norm() / (a.norm() + 1e-300))
    if worst > 1e-4 * amax or rel >= 5e-5 or not bool(torch.isfinite(d).all()):
      bad.append((k, rel, float(err.max()), amax))
  print(f'{what}: {nan_leaves} NaN leaves, {len(bad)} finite leaves off the float-atomic result {bad[:3]}')
  assert not bad, f'{what}: a finite det_grads gradient disagrees with the float-atomic one (wrapped or rounded away): {bad[:5]}'


def _all_nan(g, leaves=None):
  return all(bool(torch.isnan(g[k]).any()) for k in (leaves or g))


@pytest.mark.parametrize('precision,loss_scale', [('fp32', None), ('bf16', None), ('fp16', 2.0 ** 8)])
def test_det_grads_overflow_is_nan_never_a_wrong_value(c772, precision, loss_scale):
  """denom far below the visible count scales every gradient up by the same factor.  1e8 ... 1e12 for the largest leaf element (steps of 10^0.5): the unit
  coarsens with the gradients (down to its floor 2^-(32-24)), every det_grads leaf must equal the float-atomic one.  1e18 and 1e21: past the floor, addends of
  2^55 units and more -- the whole buffer must come out NaN (the sticky flag), while the float-atomic reference is still finite in fp32 / bf16; bf16 checks the
  scale leaves of the single-query attention backward (its own guard) explicitly.  fp16 with a fixed loss scale 2^8 (targets for the scaled buffer): the
  16-bit activation gradients overflow to inf first, and an infinite addend must trip the same guard."""
  import spa3d
  cfg, gp, batch, noise = c772
  nvis = float(batch['query_tracks_visible'].sum())
  base = _grads(spa3d, c772, precision, 0, nvis, loss_scale)
  gmax = _leaf_max(base) * (loss_scale or 1.0)
  del base
  for target in (1e8, 3.16e8, 1e9, 3.16e9, 1e10, 3.16e10, 1e11, 3.16e11, 1e12, 1e18, 1e21):
    denom = nvis * gmax / target
    ref = _grads(spa3d, c772, precision, 0, denom, loss_scale)
    det = _grads(spa3d, c772, precision, 1, denom, loss_scale)
    what = f'{precision} denom {denom:.3e} (largest leaf element ~{target:.0e})'
    _agree_or_nan(det, ref, what)
    if precision == 'bf16':
      for k in Q1_LEAVES:
        assert float(ref[k].double().norm()) > 0, k
      _agree_or_nan(det, ref, what + ' single-query attention scale leaves', Q1_LEAVES)
    if target <= 1e12 and precision != 'fp16':
      assert not any(bool(torch.isnan(v).any()) for v in det.values()), f'{what}: in range, yet NaN'
    if target >= 1e18:
      if precision != 'fp16':
        assert all(bool(torch.isfinite(v).all()) for v in ref.values()), f'{what}: the float-atomic reference must stay finite for the test to mean anything'
      assert _all_nan(det), f'{what}: beyond the fixed-point range, yet some leaf came out finite'
      if precision == 'bf16':
        assert _all_nan(det, Q1_LEAVES)
    del ref, det


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('denom', [4.4e6, 4.4e8])
def test_det_grads_resolve_small_leaves_when_denom_exceeds_the_visible_count(c772, precision, denom):
  """A gradient sum below the fixed-point quantum rounds to zero.  The c772 batch (~1e3 visible points) under a denominator of 4.4e6 (the size of BASELINE
  configs[2]'s) and 4.4e8 has gradients 4e3 ... 4e5 times smaller than at its own count: the unit must follow (denom / visible count), so the 8 smallest-norm
  leaves keep |det - atomics| <= 1e-3 |atomics| + 1e-4 max|leaf| per element.  This is NOT the accuracy of a real configs[2] batch: there the visible count is
  the denominator and the unit is 2^-32 as before (NOTEBOOK: open)."""
  import spa3d
  ref = _grads(spa3d, c772, precision, 0, denom)
  det = _grads(spa3d, c772, precision, 1, denom)
  norms = sorted((float(v.double().norm()), k) for k, v in ref.items() if float(v.double().norm()) > 0)
  rows = []
  for nrm, k in norms[:8]:
    a, d = ref[k].double(), det[k].double()
    amax = float(a.abs().max())
    excess = float(((d - a).abs() - 1e-3 * a.abs()).max()) / amax
    rows.append((excess, k, nrm, rel_err(det[k], ref[k])))
  worst = max(rows)
  print(f'{precision} denom {denom:.1e}: worst small leaf {worst[1]} (norm {worst[2]:.3e}): (max |det-atomics| - 1e-3 |atomics|) / max|leaf| = '
        f'{worst[0]:.3e}, rel err {worst[3]:.3e}')
  bad = [r for r in rows if not r[0] <= 1e-4]
  assert not bad, f'{precision} denom {denom:.1e}: small leaves lost to the fixed-point quantum: {bad}'
