"""Grouped AdamW + weight EMA on the CPU (no compute call): the float64 restatement of the contract (tests/optim_util.py) against O.adamw_step and
against torch.optim.AdamW built from parameter groups; csrc/adamw_groups.hpp (table validation, element -> range lookup) and csrc/adamw_point.hpp
(the arithmetic of one element) compiled with the host compiler; every refusal of spa3d_adamw_step_groups, which comes before the first launch;
and spa3d.param_groups on the leaf tables of the default and the mini model."""
import ctypes as C
import math
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import optim_util as OU
from util import MINI, O, host_check_driver, product_model

F64 = torch.float64
INF, NAN = float('inf'), float('nan')


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


# ------------------------------------------------------------------------------------------------ the restatement
def _rel(a, b):
  return float((a - b).norm() / b.norm())


def test_restatement_with_an_empty_table_is_the_oracle_adamw():
  for scale, skipped in ((0.02, 0), (5.0, 0), (0.02, 2)):
    gen = torch.Generator().manual_seed(11)
    n = 777
    p0 = torch.randn(n, generator=gen, dtype=F64)
    grads = [scale * torch.randn(n, generator=gen, dtype=F64) for _ in range(3)]
    po, mo, vo = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    pr, mr, vr = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for t in range(3):
      gn = O.adamw_step({'a': po}, {'a': grads[t]}, {'a': mo}, {'a': vo}, max(t + 2 - skipped, 0), 3e-3)
      gr, skip = OU.adamw_groups_step(pr, grads[t], mr, vr, t + 2, 3e-3, skipped=skipped)
      assert not skip and abs(gr - gn) <= 1e-15 * gn
    for a, b in ((pr, po), (mr, mo), (vr, vo)):
      assert _rel(a, b) <= 1e-15


def _torch_groups_case(scale, steps=3):
  """three leaves plus a gap; one leaf frozen, one without decay at a tenth of the rate, one at ten times the rate with three times the decay"""
  gen = torch.Generator().manual_seed(5)
  sizes = [85, 5, 9, 40]          # leaf 1 frozen; leaf 3 is in no range
  offs = np.concatenate([[0], np.cumsum(sizes)])
  n = int(offs[-1])
  groups = [(0, 85, 0.1, 0.0), (85, 90, 0.0, 1.0), (90, 99, 10.0, 3.0)]
  lr, wd = 3e-3, 0.01
  p0 = torch.randn(n, generator=gen, dtype=F64)
  grads = [scale * torch.randn(n, generator=gen, dtype=F64) for _ in range(steps)]
  for g in grads:
    g[85:90] = NAN    # a frozen gradient is not read
  pr, mr, vr = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
  norms = []
  for t in range(steps):
    gn, skip = OU.adamw_groups_step(pr, grads[t], mr, vr, t, lr, wd=wd, groups=groups)
    assert not skip
    norms.append(gn)
  leaves = [torch.nn.Parameter(p0[offs[i]:offs[i + 1]].clone()) for i in range(4)]
  scales = [(0.1, 0.0), None, (10.0, 3.0), (1.0, 1.0)]
  opt = torch.optim.AdamW([{'params': [leaves[i]], 'lr': lr * scales[i][0], 'weight_decay': wd * scales[i][1]} for i in (0, 2, 3)], betas=(0.9, 0.999), eps=1e-8)
  live = [leaves[i] for i in (0, 2, 3)]
  tn = []
  for t in range(steps):
    for i in (0, 2, 3):
      leaves[i].grad = grads[t][offs[i]:offs[i + 1]].clone()
    tn.append(float(torch.nn.utils.clip_grad_norm_(live, 1.0)))
    opt.step()
  pt = torch.cat([l.detach() for l in leaves])
  assert torch.equal(pr[85:90], p0[85:90]) and torch.equal(pt[85:90], p0[85:90])
  assert float(mr[85:90].abs().max()) == 0 and float(vr[85:90].abs().max()) == 0
  return pr, pt, norms, tn, offs


def test_restatement_matches_torch_adamw_param_groups_without_clipping():
  pr, pt, norms, tn, offs = _torch_groups_case(0.02)
  assert max(norms) < 1.0
  for i in (0, 2, 3):
    assert _rel(pr[offs[i]:offs[i + 1]], pt[offs[i]:offs[i + 1]]) < 1e-13, i
  assert max(abs(a - b) for a, b in zip(norms, tn)) < 1e-12


def test_restatement_matches_torch_adamw_param_groups_with_clipping():
  pr, pt, norms, tn, offs = _torch_groups_case(5.0)
  assert min(norms) > 1.0
  for i in (0, 2, 3):
    assert _rel(pr[offs[i]:offs[i + 1]], pt[offs[i]:offs[i + 1]]) < 1e-9, i
  assert max(abs(a - b) for a, b in zip(norms, tn)) < 1e-10


def test_restatement_skip_and_ema():
  p, g, m, v, e = (t.double() for t in OU.draw_state(300, ema=True))
  groups = [(10, 20, 0.0, 1.0)]
  before = [t.clone() for t in (p, m, v, e)]
  g2 = g.clone(); g2[100] = INF
  gn, skip = OU.adamw_groups_step(p, g2, m, v, 3, 1e-3, groups=groups, ema=e, ema_decay=0.9)
  assert skip and not math.isfinite(gn) and all(torch.equal(a, b) for a, b in zip(before, (p, m, v, e)))
  g2 = g.clone(); g2[15] = NAN   # inside the frozen range: not read
  gn, skip = OU.adamw_groups_step(p, g2, m, v, 3, 1e-3, groups=groups, ema=e, ema_decay=0.9)
  assert not skip and math.isfinite(gn)
  assert all(torch.equal(a[10:20], b[10:20]) for a, b in zip(before, (p, m, v, e)))
  live = torch.ones(300, dtype=torch.bool); live[10:20] = False
  assert torch.allclose(e[live], 0.9 * before[3][live] + 0.1 * p[live], rtol=1e-15, atol=0)
  assert abs(gn - float(g[live].norm())) < 1e-15


# ------------------------------------------------------------------------------------------------ adamw_groups.hpp
ERR = dict(ok=0, count=1, null=2, bounds=3, empty=4, order=5, scale=6)


@pytest.fixture(scope='module')
def groups_driver(tmp_path_factory):
  return host_check_driver(tmp_path_factory, 'adamw_groups')


def _run_groups(driver, n, groups, num=None, null_table=False):
  num = len(groups) if num is None else num
  blob = struct.pack('<qqi', n, num, int(null_table)) + b''.join(struct.pack('<qqff', *g) for g in groups)
  out = subprocess.run([driver], input=blob, capture_output=True, timeout=120)
  assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
  err, bad, frozen = struct.unpack('<iii', out.stdout[:12])
  rest = out.stdout[12:]
  if err != 0:
    assert not rest
    return err, bad, frozen, None
  assert len(rest) == n * 20
  found = np.frombuffer(rest[:4 * n], np.int32)
  walk = np.frombuffer(rest[4 * n:12 * n], np.float32).reshape(n, 2)
  jump = np.frombuffer(rest[12 * n:], np.float32).reshape(n, 2)
  return err, bad, frozen, (found, walk, jump)


REFUSED_TABLES = [
    ('bounds', 100, [(-1, 5, 1.0, 1.0)], 0), ('bounds', 100, [(0, 5, 1.0, 1.0), (90, 101, 1.0, 1.0)], 1),
    ('empty', 100, [(5, 5, 1.0, 1.0)], 0), ('empty', 100, [(7, 5, 1.0, 1.0)], 0),
    ('order', 100, [(10, 20, 1.0, 1.0), (0, 5, 1.0, 1.0)], 1), ('order', 100, [(0, 10, 1.0, 1.0), (9, 20, 1.0, 1.0)], 1),
    ('scale', 100, [(0, 5, -1.0, 1.0)], 0), ('scale', 100, [(0, 5, 1.0, -1e-30)], 0), ('scale', 100, [(0, 5, NAN, 1.0)], 0),
    ('scale', 100, [(0, 5, 1.0, NAN)], 0), ('scale', 100, [(0, 5, INF, 1.0)], 0), ('scale', 100, [(0, 5, 1.0, 1.0), (5, 6, 1.0, INF)], 1),
    ('bounds', 0, [(0, 1, 1.0, 1.0)], 0),
]


@pytest.mark.parametrize('why,n,groups,bad', REFUSED_TABLES)
def test_groups_header_refuses(groups_driver, why, n, groups, bad):
  err, where, _, _ = _run_groups(groups_driver, n, groups)
  assert (err, where) == (ERR[why], bad)


def test_groups_header_refuses_counts_and_a_missing_table(groups_driver):
  assert _run_groups(groups_driver, 100, [], num=-1)[0] == ERR['count']
  assert _run_groups(groups_driver, 10 ** 6, [(i, i + 1, 1.0, 1.0) for i in range(4097)])[0] == ERR['count']   # one too many, nothing else wrong
  assert _run_groups(groups_driver, 100, [(0, 5, 1.0, 1.0)], null_table=True)[0] == ERR['null']
  assert _run_groups(groups_driver, 100, [], null_table=True)[0] == ERR['ok']     # NULL with 0
  assert _run_groups(groups_driver, 0, [])[0] == ERR['ok']


def _tables():
  t = {}
  t['one'] = (40, [(3, 4, 0.5, 2.0)])                                                         # a range of one element
  t['two adjacent'] = (40, [(0, 1, 0.0, 1.0), (1, 40, 2.0, 0.0)])                             # from element 0, adjacent, ending at n
  t['gaps'] = (300, [(0, 1, 0.0, 1.0), (1, 5, 0.1, 3.0), (7, 263, 1.0, 0.0), (263, 264, 10.0, 1.0), (290, 300, 0.0, 0.0)])
  t['4096 of one'] = (4096 + 50, [(i + 25, i + 26, float(i % 5), float(i % 3)) for i in range(4096)])
  t['4096 with gaps'] = (3 * 4096, [(3 * i + 1, 3 * i + 3, 0.25 * (i % 7), 1.0 + i % 2) for i in range(4096)])
  return t


@pytest.mark.parametrize('name', sorted(_tables()))
def test_groups_header_lookup_matches_a_linear_scan(groups_driver, name):
  n, groups = _tables()[name]
  err, _, frozen, (found, walk, jump) = _run_groups(groups_driver, n, groups)
  assert err == 0 and frozen == int(any(g[2] == 0.0 for g in groups))
  ends = np.array([g[1] for g in groups])
  ls, ws = OU.scale_vectors(n, groups, torch.float32)
  want = np.stack([ls.numpy(), ws.numpy()], 1)
  assert np.array_equal(found, np.searchsorted(ends, np.arange(n), side='right'))   # the first range that ends beyond i
  assert np.array_equal(walk, want) and np.array_equal(jump, want)
  for i in (0, n // 2, n - 1):   # and the scan itself, spot-checked
    assert OU.linear_lookup(groups, i)[1:] == (float(want[i, 0]), float(want[i, 1]))


# ------------------------------------------------------------------------------------------------ adamw_point.hpp
def test_point_header_matches_the_restatement(tmp_path_factory):
  """Inputs at the scales of test_adamw_step_matches_oracle (|p| < 6 in 4096 draws).  Gates: the project's AdamW gates -- p 1e-6 max(1, lr_scale) (the
  final subtraction rounds to half an ulp of p, <= 2.4e-7 below 4 and 4.8e-7 below 8; the update itself is ~1e-3 lr_scale with a few ulp of relative
  error), m 1e-7, v 1e-9 (values of 1e-3 and 1e-4: their half ulps are 6e-11 and 4e-12) -- and for the EMA 1e-6 (1 - d) + 3 * 2^-24 max(|e|, |p|):
  three fp32 roundings plus the p gate carried through (1 - d)."""
  driver = host_check_driver(tmp_path_factory, 'adamw_point')
  n = 4096
  p, g, m, v, e = OU.draw_state(n, seed=9, ema=True)
  lr, wd, b1, b2, eps = 3e-4, 0.01, 0.9, 0.999, 1e-8
  f = np.float32
  for (sc, t, d) in ((1.0, 8.0, 0.9), (0.37, 1.0, 0.999), (1.0, 5.0, 0.0)):
    gen = torch.Generator().manual_seed(3)
    lsc = torch.tensor([0.1, 1.0, 10.0])[torch.randint(3, (n,), generator=gen)]
    wsc = torch.tensor([0.0, 1.0, 3.0])[torch.randint(3, (n,), generator=gen)]
    lr_g, wd_g = (f(lr) * lsc.numpy()).astype(f), (f(wd) * wsc.numpy()).astype(f)
    blob = struct.pack('<6fi', sc, b1, b2, eps, t, d, n)
    blob += np.stack([lr_g, wd_g, p.numpy(), g.numpy(), m.numpy(), v.numpy(), e.numpy()], 1).astype('<f4').tobytes()
    out = subprocess.run([driver], input=blob, capture_output=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    a = np.frombuffer(out.stdout, np.float32)
    assert a.size == 2 + 4 * n
    bc, res = a[:2].astype(np.float64), a[2:].reshape(n, 4).astype(np.float64)
    b1f, b2f = float(f(b1)), float(f(b2))
    assert abs(bc[0] - (1 - b1f ** t)) < 4 * 2.0 ** -24 and abs(bc[1] - (1 - b2f ** t)) < 4 * 2.0 ** -24 * max(1 - b2f ** t, 2.0 ** -7)
    # the restatement with the call's clip factor: gradients pre-scaled, clip off
    P, G, M, V, E = p.double(), g.double() * sc, m.double().clone(), v.double().clone(), e.double().clone()
    P = P.clone()
    for scale_l in (0.1, 1.0, 10.0):
      for scale_w in (0.0, 1.0, 3.0):
        idx = (lsc == scale_l) & (wsc == scale_w)
        pp, mm, vv, ee = P[idx], M[idx], V[idx], E[idx]
        OU.adamw_groups_step(pp, G[idx], mm, vv, int(t) - 1, lr * scale_l, clip=INF, wd=wd * scale_w, ema=ee, ema_decay=d)
        P[idx], M[idx], V[idx], E[idx] = pp, mm, vv, ee
    ep = np.abs(res[:, 0] - P.numpy()) / np.maximum(1.0, lsc.double().numpy())
    em, ev = np.abs(res[:, 1] - M.numpy()), np.abs(res[:, 2] - V.numpy())
    ee_ = np.abs(res[:, 3] - E.numpy()) - 3 * 2.0 ** -24 * np.maximum(np.abs(e.double().numpy()), np.abs(P.numpy()))
    print(f'adamw_point sc={sc} t={t} d={d}: p {ep.max():.3e} (gate 1e-6)  m {em.max():.3e} (1e-7)  v {ev.max():.3e} (1e-9)  ema excess {ee_.max():.3e} ({1e-6 * (1 - d):.1e})')
    assert ep.max() < 1e-6 and em.max() < 1e-7 and ev.max() < 1e-9 and ee_.max() <= 1e-6 * (1 - d)
    if d == 0.0:
      assert np.array_equal(a[2:].reshape(n, 4)[:, 3], a[2:].reshape(n, 4)[:, 0])   # d = 0: the EMA is the new parameter, bit for bit


# ------------------------------------------------------------------------------------------------ the C entry point: refusals
FAKE = 0x100000   # never dereferenced: every call below returns before its first launch


def _call(spa3d, n=100, groups=((0, 5, 1.0, 1.0),), num=None, ema=None, d=0.0, ws=FAKE, ws_bytes=1 << 20, null=(), table=True):
  lib = spa3d._lib.load()
  tab = (spa3d._lib.ParamGroup * max(len(groups), 1))(*[spa3d._lib.ParamGroup(*g) for g in groups])
  ptr = {k: (None if k in null else FAKE) for k in ('p', 'g', 'm', 'v', 'scratch')}
  return lib.spa3d_adamw_step_groups(ptr['p'], ptr['g'], ptr['m'], ptr['v'], n, 3e-4, 0, 1.0, 0.9, 0.999, 1e-8, 0.01, tab if table else None,
                                     len(groups) if num is None else num, ema, d, ptr['scratch'], ws, ws_bytes, None)


def test_entry_point_refusals_come_before_any_launch(spa3d):
  lib = spa3d._lib.load()
  for k in ('p', 'g', 'm', 'v', 'scratch'):
    assert _call(spa3d, null=(k,)) == 1, k
  assert _call(spa3d, n=-1) == 1
  assert _call(spa3d, num=-1) == 1 and _call(spa3d, num=4097, n=10 ** 6) == 1
  assert _call(spa3d, table=False) == 1                       # groups == NULL with num_groups > 0
  for why, n, groups, _ in REFUSED_TABLES:
    assert _call(spa3d, n=n, groups=groups) == 1, (why, groups)
  for d in (-0.1, 1.0, 1.5, NAN, INF):
    assert _call(spa3d, ema=FAKE, d=d) == 1, d
  need = lib.spa3d_adamw_groups_workspace_bytes(1)
  assert need >= 24
  assert _call(spa3d, ws_bytes=need - 1) == 2 and _call(spa3d, ws=None) == 2
  assert _call(spa3d, n=100, groups=[(0, 5, 1.0, 1.0), (5, 4, 1.0, 1.0)], ws_bytes=0) == 1   # a bad table is an argument error whatever the workspace
  # n == 0: nothing to do, nothing launched -- with no table, which is the only valid one
  assert _call(spa3d, n=0, groups=(), ws=None, ws_bytes=0) == 0
  assert _call(spa3d, n=0, groups=(), ws=None, ws_bytes=0, ema=FAKE, d=0.5) == 0
  assert _call(spa3d, n=0, groups=(), table=False, ws=None, ws_bytes=0, null=('p',)) == 1


def test_workspace_query(spa3d):
  lib = spa3d._lib.load()
  assert lib.spa3d_adamw_groups_workspace_bytes(0) == 0
  assert lib.spa3d_adamw_groups_workspace_bytes(-1) == -1 and lib.spa3d_adamw_groups_workspace_bytes(4097) == -1
  sizes = [lib.spa3d_adamw_groups_workspace_bytes(k) for k in (1, 240, 4096)]
  assert all(s >= 24 * k for s, k in zip(sizes, (1, 240, 4096))) and sizes == sorted(sizes) and sizes[-1] < 1 << 20
  S = spa3d._lib.ParamGroup
  assert (S.begin.offset, S.end.offset, S.lr_scale.offset, S.wd_scale.offset, C.sizeof(S)) == (0, 8, 16, 20, 24)


# ------------------------------------------------------------------------------------------------ param_groups
def _models(spa3d):
  full = spa3d.TrackAutoEncoder3D(precision='bf16')
  _, leaves, n = full._handle(768, 1)
  pf = full.tree_from_flat(torch.zeros(n), 768, 1)
  cfg = O.Config(**MINI, use_dino=False, use_depth=False)
  mini = product_model(spa3d, cfg, 'fp32')
  _, ml, mn = mini._handle(0, 0)
  pm = mini.tree_from_flat(torch.zeros(mn), 0, 0)
  return [('default', full, pf, leaves, n), ('mini', mini, pm, ml, mn)]


def _check_table(ranges, leaves, n):
  offs = sorted(off for _, _, off in leaves) + [n]
  prev = 0
  for b, e, ls, ws in ranges:
    assert 0 <= b < e <= n and b >= prev and b in offs and e in offs   # sorted, disjoint, at leaf boundaries
    prev = e
  for a, b in zip(ranges, ranges[1:]):
    assert not (a[1] == b[0] and a[2:] == b[2:]), 'neighbours with equal scales are one range'
  assert all(r[2:] != (1.0, 1.0) for r in ranges)


def test_param_groups_on_the_leaf_tables(spa3d):
  for name, model, params, leaves, n in _models(spa3d):
    names = [l[0] for l in sorted(leaves, key=lambda l: l[2])]
    # nothing asked for: no range at all, every leaf described at (1, 1)
    pg = spa3d.param_groups(model, params)
    assert pg.ranges == [] and pg.n == n and [l[0] for l in pg.leaves] == names
    lines = pg.describe().split('\n')
    assert len(lines) == len(names) and all(ln.split()[0] == nm and 'lr_scale=1' in ln and 'wd_scale=1' in ln for ln, nm in zip(lines, names))
    # no_decay: exactly the leaves ending in /bias, /scale, /state_init
    pg = spa3d.param_groups(model, params, no_decay=True)
    _check_table(pg.ranges, leaves, n)
    got = {l[0] for l in pg.leaves if l[4] == 0.0}
    want = {nm for nm in names if re.search(r'/(bias|scale|state_init)$', nm)}
    assert got == want and want and len(want) < len(names)
    assert all(l[3] == 1.0 and l[4] in (0.0, 1.0) for l in pg.leaves)
    assert {nm.rsplit('/', 1)[1] for nm in names} == {'bias', 'scale', 'state_init', 'kernel'}   # ... and every other leaf is a kernel
    ls, ws = OU.scale_vectors(n, pg.ranges)
    for nm, b, e, l, w in pg.leaves:   # the table says what the leaves say, over each leaf and the padding behind it
      assert bool((ls[b:e] == l).all()) and bool((ws[b:e] == w).all()), nm
    # layer_decay: units follow the offsets, the last unit trains at the full rate, the first at r ** (U - 1)
    pg = spa3d.param_groups(model, params, layer_decay=0.8)
    _check_table(pg.ranges, leaves, n)
    lrs = [l[3] for l in pg.leaves]
    assert lrs == sorted(lrs) and lrs[-1] == 1.0 and pg.leaves[0][0] == 'initializer/state_init' and pg.leaves[0][1] == 0
    U = len(set(lrs))
    assert lrs[0] == 0.8 ** (U - 1) and sorted(set(lrs)) == sorted(0.8 ** (U - 1 - u) for u in range(U))
    unit_of = {l[0]: round(math.log(l[3]) / math.log(0.8)) for l in pg.leaves}
    stacks = sorted({nm.split('/')[0] for nm in names if '/layer_' in nm})
    assert stacks == ['decompress_attn', 'input_track_transformer', 'track_readout_attn', 'tracks_to_latents']
    n_layers = sum(len({nm.split('/')[1] for nm in names if nm.startswith(s + '/layer_')}) for s in stacks)
    assert U == n_layers + len({nm.split('/')[0] for nm in names}) - len(stacks)
    for s in stacks:
      last = max(int(nm.split('/')[1][6:]) for nm in names if nm.startswith(s + '/layer_'))
      assert unit_of[f'{s}/norm_encoder/scale'] == unit_of[f'{s}/layer_{last}/MLP_out/bias']    # the closing norm belongs to the last layer
      if last > 0:
        assert unit_of[f'{s}/layer_0/MLP_out/bias'] == unit_of[f'{s}/layer_1/norm_q/scale'] + 1
    assert unit_of['track_token_projection/kernel'] == unit_of['track_token_projection/bias']
    # rules: the first match wins, fixes both scales, and switches no_decay / layer_decay off for the leaf
    rules = [(r'^track_readout_attn/layer_0/', 0.5, 2.0), (r'^track_readout_attn/', 0.25, 1.0), (r'dense_out/bias$', 0.0, 0.0), (r'^initializer/', 0.0, 1.0)]
    pg = spa3d.param_groups(model, params, rules=rules, no_decay=True, layer_decay=0.8)
    _check_table(pg.ranges, leaves, n)
    by = {l[0]: l[3:] for l in pg.leaves}
    assert by['track_readout_attn/layer_0/self_att/dense_out/bias'] == (0.5, 2.0)
    assert by['track_readout_attn/layer_1/self_att/dense_out/bias'] == (0.25, 1.0)
    assert by['track_readout_attn/norm_encoder/scale'] == (0.25, 1.0)
    assert by['tracks_to_latents/layer_0/self_att/dense_out/bias'] == (0.0, 0.0)
    assert by['initializer/state_init'] == (0.0, 1.0)
    assert by['track_predictor/bias'] == (1.0, 0.0) and by['track_predictor/kernel'] == (1.0, 1.0)
    assert pg.ranges[0][:2] == (0, sorted(off for _, _, off in leaves)[1]) and pg.ranges[0][2:] == (0.0, 1.0)
    # coalescing: one rule over everything is one range over the whole buffer
    pg = spa3d.param_groups(model, params, rules=[(r'.', 0.5, 0.5)])
    assert pg.ranges == [(0, n, 0.5, 0.5)]
    pg = spa3d.param_groups(model, params, rules=[(r'^(tracks_to_latents|compressor)/', 0.0, 1.0)])
    assert len(pg.ranges) == 1 and pg.ranges[0][2:] == (0.0, 1.0)    # two modules that adjoin in the buffer: one frozen range
    for bad in (dict(rules=[('x', -1.0, 1.0)]), dict(rules=[('x', 1.0, NAN)]), dict(rules=[('x', INF, 1.0)]), dict(layer_decay=0.0), dict(layer_decay=NAN)):
      with pytest.raises(ValueError):
        spa3d.param_groups(model, params, **bad)
  # the per-leaf table of the default model fits the optimizer's limit with room to spare
  _, model, params, leaves, n = _models(spa3d)[0]
  pg = spa3d.param_groups(model, params, no_decay=True, layer_decay=0.8)
  print(f'default model: {len(leaves)} leaves, {len(pg.ranges)} ranges with no_decay + layer_decay')
  assert 100 < len(pg.ranges) <= len(leaves) < 4096
