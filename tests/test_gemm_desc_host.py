"""CPU side of tests/test_gpu_gemm_desc.py: the row-map formula against hand-written cases, the kernel ids of include/spa3d.h against the names the planner's
host program prints, the ctypes mirror of spa3d_gemm_args against the C struct, and for EVERY GPU case -- before any GPU run -- that the planner gives the kernel
the case names and that every expected value is exactly representable in the output type (so torch.equal is the right comparison).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import parity_util as PU
import test_gpu_gemm_desc as TD
from util import host_check_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT_ALL = TD.NT_EXACT + TD.NT_CROW_PRE + TD.NT_PRE + TD.NT_GELU_GRAD
TN_EVERY = TD.TN_ALL + TD.SEG_REFUSED


def test_row_map_hand_cases():
  assert PU.row_map(8, 3, 2).tolist() == [2, 3, 4, 7, 8, 9, 12, 13]
  assert PU.row_map(5, 1, 1).tolist() == [1, 3, 5, 7, 9]            # a readout row before every token row
  assert PU.row_map(5, 0, 3).tolist() == [0, 1, 2, 3, 4]            # group 0: no remap
  assert PU.row_map(7, 150, 1).tolist() == [1, 2, 3, 4, 5, 6, 7]    # one group: shifted by the first readout row
  m = PU.row_map(301, 150, 1)
  assert (int(m[149]), int(m[150]), int(m[299]), int(m[300])) == (150, 152, 301, 303)
  m = PU.row_map(20, 7, 3).tolist()
  assert m[:8] == [3, 4, 5, 6, 7, 8, 9, 13] and m[14] == 23          # rows 10 - 12 and 20 - 22 are skipped
  assert len(set(m)) == 20


def test_pattern_is_exact_and_outside_the_lane():
  p = PU.pattern(300, 400)
  for dt in (torch.bfloat16, torch.float16, torch.float32):
    PU.assert_exact_in(p, dt, 'pattern')
  assert float(p.max()) <= -512 and float(p.min()) >= -764
  assert not torch.equal(p[0], p[1]) and not torch.equal(p[:, 0], p[:, 1])
  with pytest.raises(AssertionError):
    PU.assert_exact_in(torch.tensor([257.0], dtype=torch.float64), torch.bfloat16)
  with pytest.raises(AssertionError):
    PU.assert_exact_in(torch.tensor([0.5], dtype=torch.float64), torch.float32)


@pytest.fixture(scope='module')
def plan_driver(tmp_path_factory):
  return host_check_driver(tmp_path_factory, 'gemm_plan', fp_contract_off=False)


def _norm(name):
  return name.replace('_', '').lower()


def test_kernel_ids_match_the_planner_names(plan_driver):
  """SPA3D_GEMM_* of the header, GEMM_KERNELS of the binding and the planner program's own table: same values, same names"""
  hdr = open(os.path.join(ROOT, 'include', 'spa3d.h')).read()
  ids = {m.group(1): int(m.group(2)) for m in re.finditer(r'\bSPA3D_GEMM_([A-Z0-9_]+)\s*=\s*(\d+)', hdr)}
  r = subprocess.run([plan_driver], input='kernels 0\n', capture_output=True, text=True, timeout=60)
  assert r.returncode == 0, r.stderr
  planner = {int(l.split()[0]): l.split()[1] for l in r.stdout.splitlines()}
  assert len(ids) == len(planner) == 17 and sorted(ids.values()) == sorted(planner) == list(range(17))
  for name, v in ids.items():
    assert _norm(name) == _norm(planner[v]), (name, v, planner[v])
  import spa3d
  assert list(spa3d._lib.GEMM_KERNELS) == [planner[i] for i in range(17)]
  epi = {m.group(1): int(m.group(2)) for m in re.finditer(r'\bSPA3D_EPI_([A-Z_]+)\s*=\s*(\d+)', hdr)}
  assert epi == {'NONE': spa3d._lib.EPI_NONE, 'GELU': spa3d._lib.EPI_GELU, 'MUL_GELU_GRAD': spa3d._lib.EPI_MUL_GELU_GRAD} == {'NONE': 0, 'GELU': 1, 'MUL_GELU_GRAD': 2}


def test_gemm_args_mirror_matches_the_c_struct(tmp_path_factory):
  import spa3d
  exe = host_check_driver(tmp_path_factory, 'gemm_args', fp_contract_off=False)
  r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
  assert r.returncode == 0, r.stderr
  want = [(l.split()[0], int(l.split()[1])) for l in r.stdout.splitlines()]
  G = spa3d._lib.GemmArgs
  assert want[0] == ('sizeof', C.sizeof(G))
  assert want[1:] == [(n, getattr(G, n).offset) for n, _ in G._fields_]


def test_every_gpu_case_runs_on_the_kernel_it_names(plan_driver):
  cases = NT_ALL + TN_EVERY
  r = subprocess.run([plan_driver], input='\n'.join(TD.plan_line(c) for c in cases) + '\n', capture_output=True, text=True, timeout=60)
  assert r.returncode == 0, r.stderr
  got = r.stdout.splitlines()
  assert len(got) == len(cases)
  bad = []
  for c, g in zip(cases, got):
    k = g.split()[0]
    fused = k.endswith('+colsum')
    k = k[:-7] if fused else k
    want = c['kernel']
    if want == 'Refuse':   # the entry's reading of the plan: the generic kernel under impl >= 2, or with segments, is a refusal
      ok = k == 'Generic' and (c['impl'] >= 2 or c['seg_n'] > 0)
    else:
      ok = k == want
    if c['kind'] == 'tn' and c['colsum'] and want != 'Refuse':
      ok = ok and fused == (want not in ('Tn', 'Generic'))
    if not ok:
      bad.append((c['id'], want, g))
  assert not bad, bad
  # every kernel / feature pair of the docstring's table is in the lists
  def ran(cases, **f):
    return {c['kernel'] for c in cases if all(c[k] == v if not callable(v) else v(c[k]) for k, v in f.items())}
  yes = lambda v: bool(v) and v != (0, 0)
  assert ran(TD.NT_CROW, crow=yes) == {'NtOcc', 'Nt', 'Nt8p256', 'Nt8p384', 'Generic'}
  assert ran(TD.NT_STRIDES) == {'NtOcc', 'Nt', 'Nt8p256', 'Nt8p384', 'Nt8pp256', 'Nt8pp384', 'Generic'}
  assert ran(TD.NT_OUT, out_f32=True, acc=False) == {'NtOcc', 'Nt', 'Nt8p256', 'Nt8p384', 'Nt8pp256', 'Generic'}
  assert ran(TD.NT_OUT, out_f32=False, acc=True) == ran(TD.NT_OUT, out_f32=True, acc=True) == {'NtOcc', 'Nt', 'Nt8p256', 'Nt8p384', 'Generic'}
  assert ran(TD.NT_GELU_GRAD) == {'NtOcc', 'Nt', 'Nt8p256', 'Nt8p384'}
  tiled = {'Tn8p256', 'Tn8p128x384', 'Tn8p384x128', 'Tnb'}
  assert ran(TD.TN_BROW, brow=yes) == tiled | {'Tn', 'Generic'} and ran(TD.TN_SEG) == tiled and ran(TD.TN_SEG, brow=yes) >= {'Tnb', 'Tn8p128x384'}
  assert ran(TD.TN_COLSUM, brow=yes) == ran(TD.TN_COLSUM, brow=(0, 0)) == tiled | {'Tn', 'Generic'} and ran(TD.TN_STRIDES) == tiled | {'Tn', 'Generic'}


@pytest.mark.parametrize('c', TD._ids([c for c in NT_ALL if c['epi'] != 2]))
def test_nt_references_are_exact(c):
  """every expected C and pre_out value of the case is exact in both 16-bit types (fp32 for an f32 output), operands included; and the gather reference equals
  a float64 matmul of the gathered operands scattered row by row"""
  o = TD.nt_build(c)
  for dt in (torch.bfloat16, torch.float16):
    PU.assert_exact_in(o['C'], torch.float32 if c['out_f32'] else dt, 'C')
    PU.assert_exact_in(o['P'], dt, 'pre_out')
    PU.assert_exact_in(o['C0'], dt, 'initial C')
    for k in ('A', 'A2', 'R', 'r1_x'):
      if o[k] is not None:
        PU.assert_exact_in(torch.nan_to_num(o[k], nan=0.0), dt, k)
  pre = c['alpha'] * (o['Aeff'] @ o['W'])
  if o['bias'] is not None:
    pre = pre + o['bias']
  if o['r1_x'] is not None:
    pre = pre + torch.outer(o['r1_x'][o['arow'].long()], o['r1_w'])
  assert torch.equal(pre, o['pre'])
  want = PU.pattern(o['rows'], c['N'])
  for m in range(c['M']):
    if o['cmap'][m] >= 0:
      want[o['cmap'][m]] = pre[m]
  assert torch.equal(want, o['P'])
  cm = o['cmap'][o['cmap'] >= 0]
  assert len(set(cm.tolist())) == cm.numel() and int(cm.max()) < o['rows']
  if c['emb']:
    assert o['cidx'][0] < 0 and o['cidx'][127] < 0 and o['cidx'][-1] < 0 and 0.1 < float((o['cidx'] < 0).float().mean()) < 0.4
    assert o['arow'].unique().numel() < c['M'] and int(o['arow'].max()) < c['emb']['src_rows']
    assert bool(torch.isnan(o['A']).any(1).any())   # rows nobody names are NaN


@pytest.mark.parametrize('c', TD._ids(TN_EVERY))
def test_dw_references_are_exact(c):
  o = TD.tn_build(c)   # asserts |dW|, |colsum| < 2^24 and integer
  X, dY = o['X'][:, :c['Ki']], o['dY']
  at = PU.row_map(c['M'], *c['brow'])
  assert bool(torch.isnan(dY[:, c['N']:]).all()) and bool(torch.isnan(o['X'][:, c['Ki']:]).all())
  skipped = torch.ones(dY.shape[0], dtype=torch.bool); skipped[at] = False
  assert bool(torch.isnan(dY[skipped]).all()) and int(skipped.sum()) == dY.shape[0] - c['M']
  dense = dY[at][:, :c['N']]
  assert torch.equal(o['C0'] + X.t() @ dense, o['dW']) and torch.equal(o['cs0'] + dense.sum(0), o['cs'])
  for dt in (torch.bfloat16, torch.float16):
    PU.assert_exact_in(X, dt, 'X')
    PU.assert_exact_in(dense, dt, 'dY')


def test_batch_reference_is_exact():
  A, B, Cx, st = TD.batch_build()
  for dt in (torch.bfloat16, torch.float16, torch.float32):
    PU.assert_exact_in(Cx, dt, 'C')
  b = TD.BATCH
  for b1 in range(b['nb1']):
    for b2 in range(b['nb2']):
      a = A[b1 * st['bA1'] + b2 * st['bA2']:][:b['M'] * b['K']].reshape(b['M'], b['K'])
      w = B[b1 * st['bB1'] + b2 * st['bB2']:][:b['K'] * b['N']].reshape(b['K'], b['N'])
      assert torch.equal(a @ w, Cx[b1 * st['bC1'] + b2 * st['bC2']:][:b['M'] * b['N']].reshape(b['M'], b['N']))
