"""The streaming k-NN, the ball hits and the manifold estimates on the GPU (include/spa3d.h "Streaming k-NN and ball hits", csrc/motion.hip):
every result is an integer and is compared with the NumPy restatement (tests/motion_knn_util.py) EXACTLY -- no tolerance anywhere.

  1. spa3d_motion_knn: shapes crossing the 128 tile in each direction and both, E with vector and scalar staging and a flush inside, k = 1 .. 64;
     the tie rule on sets whose distances collide; zero-padded columns that would win if they were admitted; the chunk-rule case; every form
     of self-exclusion; every split count gives the same bits.
  2. spa3d_motion_ball_hits: the same shapes with radii 0, -1, one equal to a distance of its row (the <=) and INT32_MAX; rows only, columns
     only, both; several workgroups adding into one count; two calls bit-equal.
  3. spa3d.manifold_metrics against the restatement and against spa3d.precision_recall; and, at 8192 x 8192, within a quarter of one matrix.
  4. Refused calls write nothing.
Outputs of the C calls sit in canary-guarded, poisoned allocations (parity_util.guarded)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import motion_knn_util as KU
import parity_util as PU

pytestmark = pytest.mark.gpu
POISON32 = -77777777
I32MAX = (1 << 31) - 1


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


def _stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _codes(shape, seed, lo=-128, hi=129):
  return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.int16)


def _knn_c(spa3d, a, b, k, self_offset, splits, expect=0):
  """spa3d_motion_knn itself on device tensors [Ma, E], [Mb, E]: (dist, idx) int32 NumPy [Ma, k], or the return code when it is not `expect`ed 0.
  The workspace is exactly the bytes the query names, zero-filled (a slot nobody wrote reads as "distance 0 to column 0" and wins), and guarded."""
  lib, h = spa3d._lib.load(), spa3d.motion._motion_handle()
  (Ma, E), Mb = a.shape, b.shape[0]
  dist = PU.guarded(Ma, k, torch.int32, name='dist', fill=POISON32)
  idx = PU.guarded(Ma, k, torch.int32, name='idx', fill=POISON32)
  need = int(lib.spa3d_motion_knn_workspace_bytes(Ma, Mb, k, splits))
  ws = PU.guarded(1, max(need, 0) // 4, torch.int32, name='workspace', fill=0) if need > 0 else None
  rc = lib.spa3d_motion_knn(h, a.data_ptr(), Ma, b.data_ptr(), Mb, E, k, self_offset, splits, dist.data_ptr(), idx.data_ptr(), ws.data_ptr() if need > 0 else None, max(need, 0), _stream())
  torch.cuda.synchronize()
  if expect != 0:
    assert rc == expect, (rc, lib.spa3d_last_error(h))
    assert bool((dist == POISON32).all()) and bool((idx == POISON32).all())
    PU.check_guards()
    return lib.spa3d_last_error(h).decode()
  spa3d._lib.check(rc, h, 'spa3d_motion_knn')
  res = dist.cpu().numpy().copy(), idx.cpu().numpy().copy()
  PU.check_guards()
  return res


def _same_knn(got, want, what):
  (gd, gi), (wd, wi) = got, want
  assert gd.dtype == np.int32 and gi.dtype == np.int32 and gd.shape == wd.shape and gi.shape == wi.shape
  bad = (gd.astype(np.int64) != wd) | (gi.astype(np.int64) != wi)
  assert not bad.any(), (f'{what}: {int(bad.sum())} of {wd.size} entries differ, first at {tuple(np.argwhere(bad)[0])}: '
                         f'(d, j) = ({gd[bad][0]}, {gi[bad][0]}) for ({wd[bad][0]}, {wi[bad][0]})')


def _check_knn(spa3d, a, b, k, self_offset, splits=1, what=''):
  got = _knn_c(spa3d, _dev(a), _dev(b), k, self_offset, splits)
  _same_knn(got, KU.knn(a, b, k, self_offset), what or f'{a.shape[0]} x {b.shape[0]}, E = {a.shape[1]}, k = {k}, self_offset = {self_offset}, splits = {splits}')
  return got


# ---------------------------------------------------------------------------------------------- 1. k-NN
GRID_M = [(1, 2), (16, 17), (130, 33), (33, 130), (130, 300)]
GRID_E = [96, 1000, 1056, 12288]          # two K steps; a K tail that is no multiple of 32; a flush inside; the model's 128 x 96 (E % 8 != 0: the test after this one)
GRID = [(Ma, Mb, E, k) for Ma, Mb in GRID_M for E in GRID_E for k in (1, 3, 8) if k <= Mb] + [(70, 200, 96, 64)]


@pytest.mark.parametrize('Ma,Mb,E,k', GRID)
def test_knn_equals_the_restatement(spa3d, Ma, Mb, E, k):
  a, b = _codes((Ma, E), Ma * 100003 + E), _codes((Mb, E), Mb * 7919 + E + 1)
  _check_knn(spa3d, a, b, k, -1)


@pytest.mark.parametrize('E', [1, 37, 1001])
def test_knn_of_rows_that_are_no_multiple_of_16_bytes(spa3d, E):
  """E % 8 != 0 stages by guarded scalar loads, as spa3d_motion_pdist does; a base 2 bytes off the grid does too"""
  a, b = _codes((19, E), E), _codes((130, E), E + 1)
  _check_knn(spa3d, a, b, 3, -1)
  buf = torch.zeros(19 * E + 1, dtype=torch.int16, device='cuda')
  buf[1:] = _dev(a).reshape(-1)
  _same_knn(_knn_c(spa3d, buf[1:].view(19, E), _dev(b), 3, -1, 1), KU.knn(a, b, 3, -1), f'E = {E}, a 2 bytes off')


@pytest.mark.parametrize('k', [1, 3, 8])
def test_the_tie_rule(spa3d, k):
  """equal distances go to the lower column: codes from {0, 1} at E = 8 (distances 0 .. 8 over 150 columns), duplicated rows, one row repeated"""
  x = _codes((150, 8), 11, 0, 2)
  x[40], x[141], x[3] = x[7], x[7], x[149]                 # duplicates across the tile edge: distance 0 to another sample
  d = KU.sqdist(x, x)
  assert d.max() <= 8 and (d == 0).sum() > 150
  for splits in (1, 2):
    _check_knn(spa3d, x, x, k, 0, splits)
    _check_knn(spa3d, x[30:140], x, k, -1, splits)
  same = np.tile(_codes((1, 8), 12), (140, 1))
  dist, idx = _check_knn(spa3d, same, same, k, 0, 2)
  assert not dist.any() and idx[0].tolist() == list(range(1, k + 1)) and idx[139].tolist() == list(range(k)) and idx[2, :2].tolist() == [0, 1][:k]


@pytest.mark.parametrize('Mb,k', [(129, 1), (129, 3), (1, 1), (260, 8)])
def test_padded_columns_never_become_candidates(spa3d, Mb, k):
  """a column past Mb is zeros in LDS: its "distance" |a_i|^2 = 128^2 E is below every real distance here (>= 255^2 E), so it would win"""
  E = 96
  a = np.full((5, E), 128, np.int16)
  b = (-128 + _codes((Mb, E), Mb, 0, 2)).astype(np.int16)
  assert KU.sqdist(a, b).min() >= 255 * 255 * E > 128 * 128 * E
  dist, idx = _check_knn(spa3d, a, b, k, -1)
  assert idx.max() < Mb and dist.min() >= 255 * 255 * E
  _check_knn(spa3d, a, b, k, -1, 3)


@pytest.mark.parametrize('Ma,Mb', [(16, 17), (130, 33)])
def test_the_chunk_rule_case(spa3d, Ma, Mb):
  """E = 12288, codes from {127, 128}: the dot products pass 2^24 with odd increments (tests/test_gpu_motion.py); the distances are small and collide"""
  E = 12288
  rng = np.random.default_rng(Ma)
  a, b = (127 + rng.integers(0, 2, (Ma, E))).astype(np.int16), (127 + rng.integers(0, 2, (Mb, E))).astype(np.int16)
  _check_knn(spa3d, a, b, 3, -1)
  dist, _ = _check_knn(spa3d, a, -b, 3, -1)
  assert dist.min() > 12288 * 254 * 254 - 1


def test_self_exclusion(spa3d):
  x = _codes((200, 96), 21)
  dist, idx = _check_knn(spa3d, x, x, 3, 0)
  assert (idx != np.arange(200)[:, None]).all() and dist.min() > 0
  # rows 5 .. 134 of the set, crossing a tile edge: each leaves its own column out ...
  dist, idx = _check_knn(spa3d, x[5:135], x, 3, 5)
  assert (idx != np.arange(5, 135)[:, None]).all()
  _same_knn((dist, idx), tuple(r[5:135] for r in KU.knn(x, x, 3, 0)), 'the slice of the whole set\'s result')
  # ... and with -1 finds itself first, at distance 0
  dist, idx = _check_knn(spa3d, x[5:135], x, 3, -1)
  assert idx[:, 0].tolist() == list(range(5, 135)) and not dist[:, 0].any() and dist[:, 1].min() > 0
  # the smallest sets k allows: Mb = k with nothing left out, Mb = k + 1 with the own column left out
  _check_knn(spa3d, x[:3], x[:8], 8, -1)
  dist, idx = _check_knn(spa3d, x[:9], x[:9], 8, 0)
  assert sorted(idx[4].tolist()) == [0, 1, 2, 3, 5, 6, 7, 8]
  # Mb = k with the own column left out: refused, nothing written
  assert 'the 7 columns' in _knn_c(spa3d, _dev(x[:8]), _dev(x[:8]), 8, 0, 1, expect=1)


def test_every_split_count_gives_the_same_bits(spa3d):
  """130 x 700, k = 8: six column tiles.  splits = 7 has a range without a tile; 130 x 645 with six ranges has one of five columns, fewer than k"""
  for Mb, counts in ((700, (1, 2, 3, 7, 0)), (645, (1, 6, 9))):
    a, b = _codes((130, 96), Mb), _codes((Mb, 96), Mb + 1)
    want = KU.knn(a, b, 8, -1)
    res = [_knn_c(spa3d, _dev(a), _dev(b), 8, -1, s) for s in counts]
    for s, got in zip(counts, res):
      _same_knn(got, want, f'130 x {Mb}, splits = {s}')
      assert np.array_equal(got[0], res[0][0]) and np.array_equal(got[1], res[0][1])
  # a set against itself over several ranges, and the Python call (the plan's splits, a workspace from torch, int64 indices)
  x = _codes((300, 4, 24), 5)
  flat = x.reshape(300, -1)
  want = KU.knn(flat, flat, 5, 0)
  _same_knn(_knn_c(spa3d, _dev(flat), _dev(flat), 5, 0, 3), want, 'self, 3 ranges')
  for splits in (0, 1, 3):
    dist, idx = spa3d.motion_knn(_dev(x), k=5, splits=splits)
    assert dist.dtype == torch.int32 and idx.dtype == torch.int64 and dist.is_cuda and tuple(dist.shape) == tuple(idx.shape) == (300, 5)
    assert np.array_equal(dist.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[1])
  dist, idx = spa3d.motion_knn(_dev(x[100:250]), _dev(x), k=2, query_offset=100)
  assert np.array_equal(idx.cpu().numpy(), KU.knn(flat, flat, 2, 0)[1][100:250])
  dist, idx = spa3d.motion_knn(_dev(x[:7]), _dev(x), k=5)                             # retrieval: nothing left out
  assert np.array_equal(idx.cpu().numpy(), KU.knn(flat[:7], flat, 5, -1)[1]) and idx[:, 0].tolist() == list(range(7))


# ---------------------------------------------------------------------------------------------- 2. ball hits
def _ball_c(spa3d, a, b, radius, self_offset, rows=True, cols=True):
  """spa3d_motion_ball_hits itself: (row_hits, col_hits) int32 NumPy, None for the one not asked for"""
  lib, h = spa3d._lib.load(), spa3d.motion._motion_handle()
  (Ma, E), Mb = a.shape, b.shape[0]
  rh = PU.guarded(1, Ma, torch.int32, name='row_hits', fill=POISON32) if rows else None
  ch = PU.guarded(1, Mb, torch.int32, name='col_hits', fill=POISON32) if cols else None
  spa3d._lib.check(lib.spa3d_motion_ball_hits(h, a.data_ptr(), Ma, b.data_ptr(), Mb, E, radius.data_ptr(), self_offset, rh.data_ptr() if rows else None,
                                              ch.data_ptr() if cols else None, _stream()), h, 'spa3d_motion_ball_hits')
  torch.cuda.synchronize()
  res = tuple(None if t is None else t.cpu().numpy().reshape(-1).copy() for t in (rh, ch))
  PU.check_guards()
  return res


def _radii(d, seed):
  """int32 [Ma]: by turns 0, -1, a distance of the row (so that <= and < differ), INT32_MAX, and the row's median"""
  rng = np.random.default_rng(seed)
  rad = np.empty(len(d), np.int64)
  for i in range(len(d)):
    rad[i] = (0, -1, d[i, rng.integers(0, d.shape[1])], I32MAX, int(np.median(d[i])))[(i + seed) % 5]
  return rad.astype(np.int32)


def _check_ball(spa3d, a, b, self_offset, seed):
  rad = _radii(KU.sqdist(a, b), seed)
  want = KU.ball_hits(a, b, rad, self_offset)
  da, db, dr = _dev(a), _dev(b), _dev(rad)
  both = _ball_c(spa3d, da, db, dr, self_offset)
  what = f'{a.shape[0]} x {b.shape[0]}, E = {a.shape[1]}, self_offset = {self_offset}'
  for got, w, name in zip(both, want, ('row_hits', 'col_hits')):
    assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64), w), f'{what}: {name} differs in {int((got != w).sum())} of {len(w)}'
  rows_only, cols_only = _ball_c(spa3d, da, db, dr, self_offset, cols=False), _ball_c(spa3d, da, db, dr, self_offset, rows=False)
  assert rows_only[1] is None and cols_only[0] is None and np.array_equal(rows_only[0], both[0]) and np.array_equal(cols_only[1], both[1])
  again = _ball_c(spa3d, da, db, dr, self_offset)
  assert np.array_equal(again[0], both[0]) and np.array_equal(again[1], both[1])
  return both, rad


@pytest.mark.parametrize('E', GRID_E)
@pytest.mark.parametrize('Ma,Mb', GRID_M + [(300, 140)])
def test_ball_hits_equal_the_restatement(spa3d, Ma, Mb, E):
  """300 x 140: three workgroups add into each column count, two into each row count"""
  a, b = _codes((Ma, E), Ma * 31 + E), _codes((Mb, E), Mb * 37 + E + 1)
  (rows, cols), rad = _check_ball(spa3d, a, b, -1, Ma + Mb)
  assert (rows[rad == I32MAX] == Mb).all() and not rows[rad <= 0].any() and rows.sum() == cols.sum()


def test_ball_hits_of_a_set_with_ties_and_padded_columns(spa3d):
  x = _codes((150, 8), 11, 0, 2)                            # distances 0 .. 8: most radii equal many distances of their row
  x[40], x[141] = x[7], x[7]
  for so in (0, -1):
    (rows, cols), rad = _check_ball(spa3d, x, x, so, 3)
    assert (rows[rad == I32MAX] == (149 if so == 0 else 150)).all() and (so == 0 or (rows[rad == 0] >= 1).all())
  _check_ball(spa3d, x[5:135], x, 5, 4)
  # rows of large norm against 129 columns and 1: a zero-padded column is inside every such ball and must not be counted
  a = np.full((5, 96), 128, np.int16)
  for Mb in (129, 1):
    b = (-128 + _codes((Mb, 96), Mb, 0, 2)).astype(np.int16)
    rad = np.array([I32MAX, 128 * 128 * 96, 255 * 255 * 96 - 1, 256 * 256 * 96, -1], np.int32)
    rows, cols = _ball_c(spa3d, _dev(a), _dev(b), _dev(rad), -1)
    want = KU.ball_hits(a, b, rad, -1)
    assert np.array_equal(rows, want[0]) and np.array_equal(cols, want[1]) and rows.tolist() == [Mb, 0, 0, Mb, 0] and cols.tolist() == [2] * Mb


# ---------------------------------------------------------------------------------------------- 3. the manifold estimates
def _same_metrics(m, want, k):
  for name in ('precision', 'recall', 'density', 'coverage'):
    assert isinstance(getattr(m, name), float) and getattr(m, name) == want[name], (name, getattr(m, name), want[name])
  for name in ('real_radius', 'gen_radius', 'gen_in_real_balls', 'real_in_gen_balls', 'real_ball_hits'):
    t = getattr(m, name)
    assert t.dtype == torch.int32 and t.is_cuda and np.array_equal(t.cpu().numpy().astype(np.int64), want[name]), name
  assert m.k == k


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('case', ['hand', 'random', 'ties'])
def test_manifold_metrics_equal_the_restatement_and_precision_recall(spa3d, case, k):
  if case == 'hand':
    real, gen = KU.HAND_REAL, KU.HAND_GEN
  elif case == 'random':
    # a generated sample is a real one plus noise of one of three sizes: well inside the real sample's ball, near its edge, well outside
    rng = np.random.default_rng(2)
    real = _codes((200, 128, 96), 1, -40, 41)
    amp = np.array([20.0, 57.0, 90.0])[rng.integers(0, 3, 150)]
    gen = np.clip(real[rng.integers(0, 200, 150)] + np.rint(rng.uniform(-1, 1, (150, 128, 96)) * amp[:, None, None]), -128, 128).astype(np.int16)
  else:
    real, gen = KU.tie_sets()
  m = spa3d.manifold_metrics(_dev(real), _dev(gen), k=k)
  want = KU.manifold(real, gen, k)
  _same_metrics(m, want, k)
  assert (m.precision, m.recall) == spa3d.precision_recall(_dev(real), _dev(gen), k=k)
  if case == 'hand' and k == 1:
    for name, w in KU.HAND.items():
      got = getattr(m, name)
      assert (got.tolist() if isinstance(got, torch.Tensor) else got) == w, name
  if case == 'random':
    assert 0 < m.precision < 1 and 0 < m.coverage < 1 and 0 < m.density


def test_manifold_metrics_at_8192_stay_within_a_quarter_of_one_matrix(spa3d):
  """what the streaming path is for: no [R, G] tensor.  Peak device memory of the call, the inputs included, stays below a quarter of the
  R * G * 4 bytes of ONE distance matrix (the matrix route holds three); the estimates equal the matrix route's.  torch's peak counts every
  live tensor of the process, so what earlier tests of a whole-suite run still hold (gigabytes: cached models and references) is read before
  this test allocates anything and taken off; in a process of its own that is zero and the condition is the peak itself."""
  R = G = 8192
  gc.collect()
  torch.cuda.synchronize()
  torch.cuda.empty_cache()
  held = torch.cuda.memory_allocated()       # other tests' tensors: before the inputs exist, so the inputs count towards the peak
  g = torch.Generator(device='cuda').manual_seed(0)
  real = torch.randint(-20, 21, (R, 96), generator=g, device='cuda', dtype=torch.int16)
  # a generated sample is a real one plus noise: a third each far inside the real sample's ball (noise variance 8 a coordinate against the
  # real set's 140), about as far from it as another real sample, and far outside (variance 675: past every real radius)
  amp = torch.tensor([5.0, 28.0, 45.0], device='cuda')[torch.arange(G, device='cuda') % 3]
  noise = torch.round((torch.rand(G, 96, generator=g, device='cuda') * 2 - 1) * amp[:, None]).to(torch.int16)
  gen = (real[torch.randint(0, R, (G,), generator=g, device='cuda')] + noise).contiguous()
  del amp, noise
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  m = spa3d.manifold_metrics(real, gen, k=3)
  torch.cuda.synchronize()
  peak = torch.cuda.max_memory_allocated() - held
  print(f'manifold_metrics at {R} x {G}: peak {peak / 2 ** 20:.1f} MiB allocated above the {held / 2 ** 20:.1f} MiB other tests hold, one matrix is {R * G * 4 / 2 ** 20:.0f} MiB')
  assert peak < R * G * 4 // 4, (peak, held)
  assert (m.precision, m.recall) == spa3d.precision_recall(real, gen, k=3)
  assert 0 < m.precision < 1 and 0 < m.recall <= 1 and 0 < m.coverage <= 1
  assert int(m.gen_in_real_balls.sum()) == int(m.real_ball_hits.sum()) and m.density == int(m.real_ball_hits.sum()) / (3 * G)


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_a_refused_call_writes_nothing(spa3d):
  lib, h = spa3d._lib.load(), spa3d.motion._motion_handle()
  codes = torch.zeros(130 * 96, dtype=torch.int16, device='cuda')
  word = torch.full((130 * 8,), POISON32, dtype=torch.int32, device='cuda')
  word2 = torch.full((130 * 8,), POISON32, dtype=torch.int32, device='cuda')
  ws = torch.full((7 * 130 * 8 * 2,), POISON32, dtype=torch.int32, device='cuda')
  s, cp, wp, w2p, wsp, wsb = _stream(), codes.data_ptr(), word.data_ptr(), word2.data_ptr(), ws.data_ptr(), ws.numel() * 4

  def refused(rc, text):
    assert rc == 1 and text in lib.spa3d_last_error(h).decode(), lib.spa3d_last_error(h)
  ok = dict(a=cp, Ma=130, b=cp, Mb=130, E=96, k=8, so=0, splits=7, dist=wp, idx=w2p, ws=wsp, wsb=wsb)

  def knn(**kw):
    q = dict(ok, **kw)
    return lib.spa3d_motion_knn(h, q['a'], q['Ma'], q['b'], q['Mb'], q['E'], q['k'], q['so'], q['splits'], q['dist'], q['idx'], q['ws'], q['wsb'], s)
  for kw, text in ((dict(a=None), 'a is required'), (dict(b=None), 'b is required'), (dict(dist=None), 'dist is required'), (dict(idx=None), 'idx is required'), (dict(Ma=0), 'Ma = 0'),
                   (dict(Mb=(1 << 22) + 1), 'Mb = 4194305'), (dict(E=0), 'E = 0'), (dict(E=32768), 'E = 32768'), (dict(so=-2), 'self_offset = -2'), (dict(k=0), 'k = 0'), (dict(k=65), 'k = 65'),
                   (dict(Mb=8), 'the 7 columns'), (dict(Mb=7, so=-1), 'the 7 columns'), (dict(splits=-1), 'splits = -1'), (dict(splits=4097), 'splits = 4097'),
                   (dict(ws=None), 'workspace is required'), (dict(wsb=7 * 130 * 8 * 8 - 1), '58240 needed'), (dict(wsb=0), 'needed'), (dict(ws=wsp + 4), '8-byte aligned')):
    refused(knn(**kw), text)

  def ball(a=cp, Ma=130, b=cp, Mb=130, E=96, radius=wp, so=-1, rows=w2p, cols=wsp):
    return lib.spa3d_motion_ball_hits(h, a, Ma, b, Mb, E, radius, so, rows, cols, s)
  for kw, text in ((dict(a=None), 'a is required'), (dict(b=None), 'b is required'), (dict(radius=None), 'radius is required'), (dict(rows=None, cols=None), 'one of row_hits and col_hits'),
                   (dict(Ma=0), 'Ma = 0'), (dict(Mb=0), 'Mb = 0'), (dict(E=32768), 'E = 32768'), (dict(so=-2), 'self_offset = -2')):
    refused(ball(**kw), text)
  assert lib.spa3d_motion_knn_workspace_bytes(130, 130, 8, -1) == -1 and lib.spa3d_motion_knn_workspace_bytes(130, 130, 65, 1) == -1
  torch.cuda.synchronize()
  assert bool((word == POISON32).all()) and bool((word2 == POISON32).all()) and bool((ws == POISON32).all()) and not codes.any()
  # the positive control: the same buffers, accepted -- all-zero codes, so every distance is 0 and the columns come in index order
  assert knn() == 0
  torch.cuda.synchronize()
  assert not word.any() and word2.view(130, 8)[0].tolist() == list(range(1, 9)) and word2.view(130, 8)[129].tolist() == list(range(8))
  assert not bool((ws == POISON32).any())                  # every range wrote its lists, the five without a tile as "no key"
  assert ball() == 0                                        # radius = the zeros just written: every column is a hit
  torch.cuda.synchronize()
  assert bool((word2[:130] == 130).all()) and bool((ws[:130] == 130).all()) and bool((ws[130:] != 130).any())
