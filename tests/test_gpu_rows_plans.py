"""GPU tests of the two integer plans of csrc/rows.hip -- the token-pruning plan (spa3d_op_prune_plan) and the shared-latent-row plan (spa3d_op_share_plan) --
and of what the row entry points refuse.  Plans are integers: every output, the returned count included, EQUALS the reference of tests/rows_util.py
(np.nonzero per sequence; the rank of each query's frame in order of first occurrence), and whatever lies past the count keeps its random fill.
Outputs live in parity_util.guarded() allocations, check_guards() after every call.  Companion of tests/test_gpu_rows.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity_util as PU
import rows_util as RU

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2
ERR_ARG = 1


@pytest.fixture(scope='module')
def lib():
  import spa3d
  return spa3d._lib.load()


def _s():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(dtype):
  return {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}[dtype]


def _ints(rows, cols, rng, name):
  """a guarded int32 [rows, cols] output filled with random negative values (no valid row, count or slot) -> (device view, the fill as numpy)"""
  fill = rng.integers(-9000, -1, (rows, cols)).astype(np.int32)
  out = PU.guarded(rows, cols, torch.int32, name=name, fill=0)
  out.copy_(torch.from_numpy(fill))
  return out, fill


# ================================================================================================ token-pruning plan
def _km(pattern, nseq, S, rng):
  if pattern == 'ones':
    return np.ones((nseq, S), np.float32)
  if pattern == 'col0':
    km = np.zeros((nseq, S), np.float32)
    km[:, 0] = 1.0
    return km
  km = (rng.random((nseq, S)) < 0.5).astype(np.float32)
  if pattern == 'zero-seq':
    km[nseq // 2] = 0.0
  if pattern == 'values':   # visible: 0.5, -1.0, NaN; invisible: -0.0
    r = rng.random((nseq, S))
    km = np.where(r < 0.2, 0.5, np.where(r < 0.4, -1.0, np.where(r < 0.45, np.nan, np.where(r < 0.7, -0.0, km)))).astype(np.float32)
  return km


def _prune_case(lib, nseq, S, pattern, rng):
  km = _km(pattern, nseq, S, rng)
  kmd = torch.from_numpy(km).cuda()
  cnt, _ = _ints(nseq, 1, rng, 'cnt')
  off, _ = _ints(nseq + 1, 1, rng, 'seq_off')
  row_src, fill = _ints(nseq, S, rng, 'row_src')
  kept = C.c_int64(-1)
  rc = lib.spa3d_op_prune_plan(kmd.data_ptr(), nseq, S, cnt.data_ptr(), off.data_ptr(), row_src.data_ptr(), C.byref(kept), _s())
  assert rc == 0
  PU.check_guards()
  rcnt, roff, rrows, rkept = RU.prune_plan_ref(km)
  tag = f'nseq {nseq} S {S} {pattern}'
  assert kept.value == rkept, f'kept {tag}: {kept.value} != {rkept}'
  assert np.array_equal(cnt.cpu().numpy()[:, 0], rcnt), f'cnt {tag}'
  assert np.array_equal(off.cpu().numpy()[:, 0], roff), f'seq_off {tag}'
  got = row_src.cpu().numpy().reshape(-1)
  assert np.array_equal(got[:rkept], rrows), f'row_src {tag}'
  assert np.array_equal(got[rkept:], fill.reshape(-1)[rkept:]), f'row_src past the kept rows changed {tag}'


PRUNE_NSEQ = [1, 3, 4, 5, 1023, 1024, 1025, 2049, 5000]
PRUNE_PATTERNS = ['ones', 'col0', 'bernoulli', 'zero-seq', 'values']


@pytest.mark.parametrize('S', [1, 2, 63, 64, 65, 129, 151, 320])
def test_prune_plan(lib, S):
  """S around the 64 lanes of a wave (one, two, three and five ballots per sequence); nseq around the four sequences of a workgroup and around the 1024 threads of
  the scan (1023, 1024: one count per thread; 1025, 2049, 5000: chunks of 2, 3 and 5 per thread); every visibility pattern at every size"""
  rng = np.random.default_rng(S)
  for nseq in PRUNE_NSEQ:
    for pattern in PRUNE_PATTERNS:
      _prune_case(lib, nseq, S, pattern, rng)
  print(f'  rows branch: prune plan S {S} -> ballots per sequence {(S + 63) // 64}; scan chunk per thread 1 (nseq <= 1024), 2, 3, 5')


def test_prune_plan_past_the_workgroup_cap(lib):
  """nseq = 40000 at S = 3: 10000 groups of four sequences against the cap of 8192 workgroups, so a wave takes a second sequence"""
  rng = np.random.default_rng(40000)
  for pattern in ('bernoulli', 'values'):
    _prune_case(lib, 40000, 3, pattern, rng)
  print('  rows branch: prune plan nseq 40000 -> grid capped at 8192 workgroups, second pass of the sequence loop')


def test_prune_plan_without_a_sequence(lib):
  """nseq = 0: kept = 0, nothing launched, every output at its fill (the launcher had no early return and asked for a grid of no workgroups)"""
  rng = np.random.default_rng(0)
  km = torch.ones(4, device='cuda')
  cnt, fc = _ints(2, 1, rng, 'cnt')
  off, fo = _ints(2, 1, rng, 'seq_off')
  row_src, fr = _ints(2, 4, rng, 'row_src')
  kept = C.c_int64(-1)
  assert lib.spa3d_op_prune_plan(km.data_ptr(), 0, 4, cnt.data_ptr(), off.data_ptr(), row_src.data_ptr(), C.byref(kept), _s()) == 0
  PU.check_guards()
  assert kept.value == 0
  assert np.array_equal(cnt.cpu().numpy(), fc) and np.array_equal(off.cpu().numpy(), fo) and np.array_equal(row_src.cpu().numpy(), fr)
  torch.cuda.synchronize()


# ================================================================================================ shared-latent-row plan
def _qframes(pattern, B, Q, rng):
  if pattern == 'equal':
    return np.full((B, Q), 7, np.int32)
  if pattern == 'distinct':
    return np.stack([rng.permutation(Q) for _ in range(B)]).astype(np.int32)
  return rng.integers(0, 3 if pattern == 'of3' else 40, (B, Q)).astype(np.int32)


def _plan_case(lib, B, Q, pattern, rng, fallback=False):
  qf = _qframes(pattern, B, Q, rng)
  qfd = torch.from_numpy(qf).cuda()
  n = B * Q
  outs = [_ints(n, 1, rng, name) for name in ('slot', 'slot_b', 'slot_f', 'slot_q0')]
  scratch, _ = _ints(n + B + 1, 1, rng, 'scratch')
  nslot = C.c_int64(-1)
  rc = lib.spa3d_op_share_plan(qfd.data_ptr(), B, Q, *[o.data_ptr() for o, _ in outs], scratch.data_ptr(), C.byref(nslot), _s())
  assert rc == 0
  PU.check_guards()
  tag = f'B {B} Q {Q} {pattern}'
  got = [o.cpu().numpy()[:, 0] for o, _ in outs]
  if fallback:
    assert nslot.value == n, f'fallback count {tag}'
    for a, (_, fill) in zip(got, outs):
      assert np.array_equal(a, fill[:, 0]), f'the fallback wrote an output {tag}'
    return
  ref = RU.slot_plan_ref(qf)
  assert nslot.value == ref[4], f'slot count {tag}: {nslot.value} != {ref[4]}'
  assert np.array_equal(got[0], ref[0]), f'slot {tag}'
  for name, a, r, (_, fill) in zip(('slot_b', 'slot_f', 'slot_q0'), got[1:], ref[1:4], outs[1:]):
    assert np.array_equal(a[:ref[4]], r), f'{name} {tag}'
    assert np.array_equal(a[ref[4]:], fill[ref[4]:, 0]), f'{name} past the slot count changed {tag}'


@pytest.mark.parametrize('B,Q', [(1, 1), (1, 8), (2, 255), (3, 256), (2, 257), (1, 600), (1024, 8)])
def test_share_plan(lib, B, Q):
  """Q around the 256 threads of the per-sample kernel, B up to the 1024 entries of the prefix table; frames all equal, all distinct, from 3 and from 40"""
  rng = np.random.default_rng(B * 100003 + Q)
  for pattern in ('equal', 'distinct', 'of3', 'of40'):
    _plan_case(lib, B, Q, pattern, rng)
  print(f'  rows branch: share plan B {B} Q {Q} -> plan kernels')


def test_share_plan_largest_table_and_fallback(lib):
  """(1, 12288) all distinct is the largest LDS table (48 KiB); (1025, 8) and (1, 12289) are outside the tables: the count is B Q and nothing is written"""
  rng = np.random.default_rng(12288)
  _plan_case(lib, 1, 12288, 'distinct', rng)
  print('  rows branch: share plan B 1 Q 12288 -> plan kernels (48 KiB table)')
  _plan_case(lib, 1025, 8, 'of3', rng, fallback=True)
  _plan_case(lib, 1, 12289, 'of40', rng, fallback=True)
  print('  rows branch: share plan (1025, 8), (1, 12289) -> fallback')


# ================================================================================================ refusals
def test_rows_entry_points_refuse(lib):
  """The calls of rows_util.plan_refusals / row_op_refusals (a NULL pointer once per argument, a width that is no multiple of 16 bytes where the kernel is
  vector-only, a pointer off by one element and by 8 bytes, negative counts, S < 1) against real buffers: SPA3D_ERR_ARG, every output still at its random
  fill, guards intact.  tests/test_rows_ref_host.py makes the same calls without a GPU, so a call that is not refused is seen there before it launches here"""
  rng = np.random.default_rng(5)
  ints = [_ints(64, 1, rng, f'int output {i}') for i in range(5)]
  idx = torch.arange(64, dtype=torch.int32, device='cuda') % 4
  km, vis, fsrc = torch.ones(64, device='cuda'), torch.ones(64, device='cuda'), torch.randn(4096, device='cuda')
  count = C.c_int64(-5)
  f32fill = torch.randn(64, 64, generator=torch.Generator().manual_seed(1))
  fout = PU.guarded(64, 64, torch.float32, name='f32 out', fill=0)
  fout.copy_(f32fill)
  bad = [f'{name}: status {rc}' for name, rc in RU.plan_refusals(lib, km.data_ptr(), idx.data_ptr(), [v.data_ptr() for v, _ in ints], C.byref(count), _s()) if rc != ERR_ARG]
  assert count.value == -5, 'a refused plan wrote its count'
  for dtype in (F32, BF16, F16):
    dt = _dt(dtype)
    fill = torch.randn(64, 64, generator=torch.Generator().manual_seed(2)).to(dt)
    out = PU.guarded(64, 64, dt, name='out', fill=0)
    out.copy_(fill)
    src = torch.randn(8192, device='cuda').to(dt)
    calls = RU.row_op_refusals(lib, dtype, src.data_ptr(), out.data_ptr(), fout.data_ptr(), fsrc.data_ptr(), idx.data_ptr(), vis.data_ptr(), _s())
    bad += [f'{dt} {name}: status {rc}' for name, rc in calls if rc != ERR_ARG]
    torch.cuda.synchronize()
    bits = torch.int32 if dtype == F32 else torch.int16
    assert torch.equal(out.cpu().view(bits), fill.view(bits)), f'a refused call wrote to an output ({dt})'
  assert not bad, 'not refused: ' + '; '.join(bad)
  assert torch.equal(fout.cpu(), f32fill), 'a refused call wrote to an fp32 output'
  for i, (v, fill) in enumerate(ints):
    assert np.array_equal(v.cpu().numpy(), fill), f'a refused call wrote to integer output {i}'
  PU.check_guards()
