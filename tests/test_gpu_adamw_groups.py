"""spa3d_adamw_step_groups on the GPU (include/spa3d.h): bit identity with spa3d_adamw_step where the contract promises it, parameter groups against
the float64 restatement (tests/optim_util.py) at the project's AdamW gates, frozen ranges, the skip on a non-finite norm, the weight EMA, run-to-run
determinism, and TrainState(param_groups=..., ema_decay=...) on the mini model with and without `freeze`.  Every buffer the call writes sits in a
canary-guarded allocation (parity_util.guarded); input scales are those of test_adamw_step_matches_oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_util as OU
import parity_util as PU
from util import MINI, O, max_abs

pytestmark = pytest.mark.gpu

N = 100003
LR, WD, STEP = 3e-4, 0.01, 7
TABLE_A = [(0, 1), (1, 5), (7, 263), (263, 1000), (4097, 70001), (99999, 100003)]
TABLE_300 = [(50 + 333 * k, 50 + 333 * (k + 1)) for k in range(300)]
TABLE_4096 = [(7 + 24 * k, 27 + 24 * k) for k in range(4096)]


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


@pytest.fixture(scope='module')
def lib(spa3d):
  return spa3d._lib.load()


def _s():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, off, name):
  """t in a guarded device allocation, `off` floats beyond its 16-byte aligned start"""
  view = PU.guarded(1, t.numel() + off, torch.float32, name=name)[0]
  view[off:].copy_(t)
  return view[off:]


def _run(lib, spa3d, state, groups=None, ema=None, d=0.0, off=0, scratch3=0.0, entry='groups', step=STEP):
  """One optimizer call on copies of the host tensors `state` = (p, g, m, v).  entry = 'plain': spa3d_adamw_step.  Returns the CPU results."""
  p, g, m, v = (_dev(t, off, nm) for t, nm in zip(state, 'pgmv'))
  e = _dev(ema, off, 'ema') if ema is not None else None
  n = p.numel()
  scratch = PU.guarded(1, 1024, torch.float32, name='scratch', fill=0.0)[0]
  scratch[3] = scratch3
  if entry == 'plain':
    rc = lib.spa3d_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, step, 1.0, 0.9, 0.999, 1e-8, WD, scratch.data_ptr(), _s())
  else:
    groups = groups or []
    tab = (spa3d._lib.ParamGroup * max(len(groups), 1))(*[spa3d._lib.ParamGroup(*r) for r in groups])
    nb = lib.spa3d_adamw_groups_workspace_bytes(len(groups))
    ws = PU.guarded(1, max(nb, 4) // 4, torch.float32, name='ws')[0]
    rc = lib.spa3d_adamw_step_groups(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, step, 1.0, 0.9, 0.999, 1e-8, WD,
                                     tab if groups else None, len(groups), e.data_ptr() if e is not None else None, d, scratch.data_ptr(),
                                     ws.data_ptr() if groups else None, nb, _s())
  assert rc == 0
  torch.cuda.synchronize()
  out = dict(p=p.cpu(), g=g.cpu(), m=m.cpu(), v=v.cpu(), e=e.cpu() if e is not None else None, scratch=scratch[:6].cpu())
  PU.check_guards()
  return out


def _bits(a, b):
  return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _reference(state, groups, ema=None, d=0.0, skipped=0, step=STEP):
  P, G, M, V = (t.double().clone() for t in state)
  E = ema.double().clone() if ema is not None else None
  gn, skip = OU.adamw_groups_step(P, G, M, V, step, LR, wd=WD, groups=groups, ema=E, ema_decay=d, skipped=skipped)
  return P, M, V, E, gn, skip


# ------------------------------------------------------------------------------------------------ identity
@pytest.mark.parametrize('scratch3', [0.0, 3.0])
@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('n', [1, 255, 100003, 131073])
def test_identity_with_adamw_step(lib, spa3d, n, off, scratch3):
  """no table, and the single range [0, n) of scales (1, 1): p, m, v and scratch[0:6] are the bits of spa3d_adamw_step.  131073 = one element past 512
  workgroups of 256, where the grid cap of the norm's first stage binds; `off` = 1 moves every pointer off its 16-byte boundary (4 bytes on: the
  body still runs 16 bytes at a time behind a three-element head); scratch[3] = 3 moves the bias correction."""
  state = OU.draw_state(n, seed=5)
  want = _run(lib, spa3d, state, off=off, scratch3=scratch3, entry='plain')
  for groups in (None, [(0, n, 1.0, 1.0)]):
    got = _run(lib, spa3d, state, groups=groups, off=off, scratch3=scratch3)
    for k in ('p', 'm', 'v', 'scratch'):
      assert _bits(got[k], want[k]), (k, groups)
  assert float(want['scratch'][2]) == 0.0 and float(want['scratch'][0]) > 0 and not _bits(want['p'], state[0])


def test_identity_when_the_buffers_disagree_about_alignment(lib, spa3d):
  """p, m, v on a 16-byte boundary and g four bytes past one: no 16-byte body exists, every element goes one by one -- to the same bits"""
  n = 5000
  state = OU.draw_state(n, seed=6)
  want = _run(lib, spa3d, state, entry='plain')
  p, m, v = (_dev(t, 0, nm) for t, nm in zip((state[0], state[2], state[3]), 'pmv'))
  g = _dev(state[1], 1, 'g')
  scratch = PU.guarded(1, 1024, torch.float32, name='scratch', fill=0.0)[0]
  assert lib.spa3d_adamw_step_groups(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, STEP, 1.0, 0.9, 0.999, 1e-8, WD, None, 0, None, 0.0,
                                     scratch.data_ptr(), None, 0, _s()) == 0
  torch.cuda.synchronize()
  assert _bits(p.cpu(), want['p']) and _bits(m.cpu(), want['m']) and _bits(v.cpu(), want['v']) and _bits(scratch[:6].cpu(), want['scratch'])
  PU.check_guards()


# ------------------------------------------------------------------------------------------------ groups
def _check_against_reference(got, state, groups, ema=None, d=0.0):
  P, M, V, E, gn, skip = _reference(state, groups, ema, d)
  assert not skip
  ls, _ = OU.scale_vectors(state[0].numel(), groups)
  ep = ((got['p'].double() - P).abs() / ls.clamp(min=1.0)).max()
  em, ev = max_abs(got['m'], M), max_abs(got['v'], V)
  en = abs(float(got['scratch'][0]) - gn) / gn
  print(f'  {len(groups)} ranges: p / max(1, lr_scale) {float(ep):.3e} (gate 1e-6)  m {em:.3e} (1e-7)  v {ev:.3e} (1e-9)  norm rel {en:.3e} (1e-5)')
  assert float(ep) < 1e-6 and em < 1e-7 and ev < 1e-9 and en < 1e-5
  frozen = ls == 0
  for k, t in zip('pmv', (state[0], state[2], state[3])):
    assert _bits(got[k][frozen], t[frozen]), f'{k} moved inside a frozen range'
  if ema is not None:
    bound = 1e-6 * (1 - d) + 3 * 2.0 ** -24 * torch.maximum(ema.double().abs(), P.abs())
    assert bool(((got['e'].double() - E).abs() <= bound).all())
    assert _bits(got['e'][frozen], ema[frozen])


@pytest.mark.parametrize('name', ['six ranges', '300 ranges of 333', '4096 ranges'])
def test_groups_match_the_restatement(lib, spa3d, name):
  """Ranges that start and end anywhere -- one element, adjacent, with gaps, across workgroup runs, ending at n -- with scales from {0, 0.1, 1, 10} x
  {0, 1, 3}.  Gates: the project's AdamW gates (p 1e-6, m 1e-7, v 1e-9, norm 1e-5 relative), the p gate times max(1, lr_scale) because the update is
  linear in the rate."""
  bounds = {'six ranges': TABLE_A, '300 ranges of 333': TABLE_300, '4096 ranges': TABLE_4096}[name]
  groups = OU.draw_groups(bounds, seed=len(bounds))
  assert {g[2] for g in groups} == {0.0, 0.1, 1.0, 10.0} and {g[3] for g in groups} == {0.0, 1.0, 3.0}
  state = OU.draw_state(N, seed=5)
  got = _run(lib, spa3d, state, groups=groups)
  _check_against_reference(got, state, groups)
  if name == 'six ranges':   # and off the 16-byte boundary
    got1 = _run(lib, spa3d, state, groups=groups, off=1)
    for k in ('p', 'm', 'v', 'scratch'):
      assert _bits(got1[k], got[k]), k


# ------------------------------------------------------------------------------------------------ frozen
def test_frozen_ranges_keep_their_bits_and_their_gradients_are_not_read(lib, spa3d):
  groups = [(0, 1, 0.0, 1.0), (1, 5, 1.0, 1.0), (7, 263, 0.0, 3.0), (263, 1000, 0.1, 0.0), (4097, 70001, 0.0, 1.0), (99999, 100003, 0.0, 0.0)]
  p, g, m, v, e = OU.draw_state(N, seed=7, ema=True)
  ls, _ = OU.scale_vectors(N, groups)
  frozen = ls == 0
  clean = _run(lib, spa3d, (p, g, m, v), groups=groups, ema=e, d=0.9)
  bad = g.clone()
  bad[frozen] = float('nan')
  bad[0] = float('inf'); bad[262] = float('-inf'); bad[70000] = float('inf'); bad[100002] = float('inf')
  got = _run(lib, spa3d, (p, bad, m, v), groups=groups, ema=e, d=0.9)
  assert float(got['scratch'][2]) == 0.0 and float(got['scratch'][3]) == 0.0 and float(clean['scratch'][2]) == 0.0
  for k, t in zip('pmve', (p, m, v, e)):
    assert _bits(got[k][frozen], t[frozen]), f'{k} moved inside a frozen range'
    assert _bits(got[k], clean[k]), f'{k}: a frozen gradient reached a live element'
    assert not _bits(got[k][~frozen], t[~frozen])
  assert _bits(got['scratch'], clean['scratch'])
  _check_against_reference(clean, (p, g, m, v), groups, ema=e, d=0.9)


# ------------------------------------------------------------------------------------------------ skip
def test_a_non_finite_live_gradient_skips_the_whole_step(lib, spa3d):
  groups = [(0, 1000, 0.0, 1.0), (1000, 5000, 0.1, 3.0)]
  p, g, m, v, e = OU.draw_state(N, seed=8, ema=True)
  g = g.clone(); g[60000] = float('inf')
  got = _run(lib, spa3d, (p, g, m, v), groups=groups, ema=e, d=0.9, scratch3=2.0)
  for k, t in zip('pmve', (p, m, v, e)):
    assert _bits(got[k], t), k
  s = got['scratch']
  assert float(s[2]) == 1.0 and float(s[3]) == 3.0 and float(s[4]) == 0.5 and float(s[5]) == 0.0 and not np.isfinite(float(s[0]))


# ------------------------------------------------------------------------------------------------ EMA
@pytest.mark.parametrize('d', [0.0, 0.9, 0.999])
def test_ema(lib, spa3d, d):
  """e = d e + (1 - d) p_new in fp32, element by element within 1e-6 (1 - d) + 3 * 2^-24 max(|e|, |p|): three fp32 roundings plus the p gate carried
  through (1 - d).  d = 0: the EMA is the new parameter, bit for bit.  Without the EMA p, m and v come out the same bits."""
  groups = OU.draw_groups(TABLE_A, seed=3)
  p, g, m, v, e = OU.draw_state(N, seed=9, ema=True)
  got = _run(lib, spa3d, (p, g, m, v), groups=groups, ema=e, d=d)
  _check_against_reference(got, (p, g, m, v), groups, ema=e, d=d)
  ls, _ = OU.scale_vectors(N, groups)
  if d == 0.0:
    assert _bits(got['e'][ls != 0], got['p'][ls != 0])
  without = _run(lib, spa3d, (p, g, m, v), groups=groups)
  for k in ('p', 'm', 'v', 'scratch'):
    assert _bits(without[k], got[k]), k
  got1 = _run(lib, spa3d, (p, g, m, v), groups=groups, ema=e, d=d, off=1)   # and off the 16-byte boundary
  for k in ('p', 'm', 'v', 'e', 'scratch'):
    assert _bits(got1[k], got[k]), k


# ------------------------------------------------------------------------------------------------ determinism
def test_two_runs_give_the_same_bits(lib, spa3d):
  groups = OU.draw_groups(TABLE_300, seed=300)
  p, g, m, v, e = OU.draw_state(N, seed=10, ema=True)
  a = _run(lib, spa3d, (p, g, m, v), groups=groups, ema=e, d=0.99)
  b = _run(lib, spa3d, (p, g, m, v), groups=groups, ema=e, d=0.99)
  for k in ('p', 'm', 'v', 'e', 'scratch'):
    assert _bits(a[k], b[k]), k
  assert float(a['scratch'][0]) > 0


# ------------------------------------------------------------------------------------------------ TrainState on the mini model
@pytest.mark.parametrize('freeze', [0, 1])
def test_train_state_with_groups_and_ema_matches_the_restatement(spa3d, freeze):
  """Three fp32 steps with param_groups(no_decay=True, layer_decay=0.8) and ema_decay=0.99 (the pattern of test_train_step_matches_oracle_adamw): oracle
  gradients at the reference's own float64 parameters, the restatement as the optimizer.  freeze=1: the call covers [lo, n) with the ranges cut and
  shifted; the frozen prefix of flat, m, v and ema keeps its bits."""
  from test_gpu_model import _noise, _params_to_oracle, _setup
  cfg = O.Config(**MINI, use_dino=False, use_depth=False)
  B, Nt, Q, T = 2, 6, 4, 8
  model, params, batch, gb = _setup(spa3d, cfg, B, Nt, Q, T, 'fp32')
  noise = _noise(B, cfg)
  pg = spa3d.param_groups(model, params, no_decay=True, layer_decay=0.8)
  print(pg.describe().split('\n')[0])
  st = spa3d.TrainState(model, params, learning_rate=1e-2, warmup_steps=2, total_steps=10, param_groups=pg, ema_decay=0.99, freeze=freeze)
  _, leaves, n = model._handle(0, 0)
  lo = st.trainable_lo
  assert (lo > 0) == (freeze == 1) and st.groups == [(max(b, lo) - lo, e - lo, ls, ws) for b, e, ls, ws in pg.ranges if e > lo]
  st.m[:lo] = 0.25; st.v[:lo] = 0.5
  start = [t.clone() for t in (st.flat, st.m, st.v, st.ema)]
  om = O.TrackAutoEncoder3D(cfg)
  b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}

  def pack(tree_flat):
    out = torch.zeros(n, dtype=torch.float64)
    for name, shape, off in leaves:
      out[off:off + int(np.prod(shape))] = tree_flat[name].reshape(-1)
    return out

  def unpack(flat):
    return O.tree_unflatten({name: flat[off:off + int(np.prod(shape))].reshape(shape) for name, shape, off in leaves})

  P = pack(O.tree_flatten(_params_to_oracle(params, torch.float64)))
  M, V, E = st.m.double().cpu(), st.v.double().cpu(), P.clone()
  for step in range(3):
    mt = st.train_step(gb, noise=noise.cuda())
    ld, _, g = O.loss_and_grads(om, unpack(P), b64, noise=noise.double())
    G = pack(g)
    lr = O.lr_schedule(step, 1e-2, 2, 10)
    gn, skip = OU.adamw_groups_step(P[lo:], G[lo:], M[lo:], V[lo:], step, lr, groups=st.groups, ema=E[lo:], ema_decay=0.99)
    assert not skip and float(mt['train/skipped']) == 0.0
    assert abs(float(mt['train/loss']) - float(ld['total_loss'])) < 1e-4 * abs(float(ld['total_loss']))
    assert abs(float(mt['train/grad_norm']) - gn) < 1e-3 * gn
  # three Adam steps at lr 1e-2: sign-like updates amplify tiny gradient differences (the bound of test_train_step_matches_oracle_adamw)
  ep, ee = max_abs(st.flat, P), max_abs(st.ema, E)
  print(f'  freeze={freeze}: params {ep:.3e}, ema {ee:.3e} (bound 2e-4)')
  assert ep < 2e-4 and ee < 2e-4
  assert not torch.equal(st.ema, st.flat) and max_abs(st.ema, start[3]) > 0
  for a, b in zip(start, (st.flat, st.m, st.v, st.ema)):
    assert torch.equal(a[:lo], b[:lo])
  # evaluation on either set of weights
  m_p, _ = st.eval_step(gb, noise=noise.cuda())
  m_e, _ = st.eval_step(gb, noise=noise.cuda(), use_ema=True)
  assert float(m_p['eval/loss']) != float(m_e['eval/loss'])
