"""The kernel sums and the kernel distance on the GPU (include/spa3d.h "Kernel sums and the kernel distance", csrc/motion.hip): every result is
an integer, or ONE rounding of an exact rational, and is compared with the restatement (tests/motion_kernel_util.py) EXACTLY -- no tolerance.

  1. spa3d_motion_kernel_sums: shapes crossing the 128 tile in each direction and both, E with vector and scalar staging, a K tail and a flush
     inside, degrees 1, 2, 3; padded rows and columns; sums whose high limb is set by one product, by a tile and by the global add; every form
     of self-exclusion; rows only, columns only, both; two calls bit-equal; degree 1 against spa3d.motion_pdist; additivity over column ranges.
  2. spa3d.kernel_distance against the restatement: the hand case, random sets at the model's width, subsets, a set against its copy; and at
     4096 x 4096 within a quarter of one matrix, the sums equal to an int64 matrix route that is exact at that width.
  3. Refused calls write nothing.
Outputs of the C calls sit in canary-guarded, poisoned allocations (parity_util.guarded)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import motion_kernel_util as KK
import parity_util as PU

pytestmark = pytest.mark.gpu
POISON32 = -77777777
POISON_LIMB = (POISON32 & 0xffffffff) | ((POISON32 & 0xffffffff) << 32)


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


def _limb_buffer(M, name):
  """uint64 [M][2] as a guarded int32 [M, 4] view filled with the poison; the view starts 4 KiB into its allocation, so it is 8-byte aligned"""
  t = PU.guarded(M, 4, torch.int32, name=name, fill=POISON32)
  assert t.data_ptr() % 8 == 0 and t.is_contiguous()
  return t


def _ints(t):
  return KK.from_limbs(t.cpu().numpy().reshape(-1, 4).view(np.int64))


def _sums_c(spa3d, a, b, degree, self_offset, rows=True, cols=True, expect=0):
  """spa3d_motion_kernel_sums itself on device tensors [Ma, E], [Mb, E]: (row_sums, col_sums) as lists of Python ints, None for the one not asked
  for.  Both buffers are allocated, guarded and poisoned whether or not they are passed: the one not passed must come back as poison.  With
  expect != 0: the refusal's message, after checking that nothing was written."""
  lib, h = spa3d._lib.load(), spa3d.motion._motion_handle()
  (Ma, E), Mb = a.shape, b.shape[0]
  rbuf, cbuf = _limb_buffer(max(Ma, 1), 'row_sums'), _limb_buffer(max(Mb, 1), 'col_sums')
  rc = lib.spa3d_motion_kernel_sums(h, a.data_ptr(), Ma, b.data_ptr(), Mb, E, degree, self_offset, rbuf.data_ptr() if rows else None, cbuf.data_ptr() if cols else None, _stream())
  torch.cuda.synchronize()
  if expect != 0:
    assert rc == expect, (rc, lib.spa3d_last_error(h))
    assert bool((rbuf == POISON32).all()) and bool((cbuf == POISON32).all())
    PU.check_guards()
    return lib.spa3d_last_error(h).decode()
  spa3d._lib.check(rc, h, 'spa3d_motion_kernel_sums')
  for asked, buf in ((rows, rbuf), (cols, cbuf)):
    assert asked or bool((buf == POISON32).all()), 'an output that was not asked for was written'
  res = (_ints(rbuf) if rows else None, _ints(cbuf) if cols else None)
  PU.check_guards()
  return res


def _first_diff(got, want):
  bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
  return f'{len(bad)} of {len(want)} differ, first at {bad[0]}: {got[bad[0]]} for {want[bad[0]]} (difference {got[bad[0]] - want[bad[0]]})' if bad else ''


def _check(spa3d, a, b, degree, self_offset, what=''):
  want = KK.kernel_sums(a, b, degree, self_offset)
  got = _sums_c(spa3d, _dev(a), _dev(b), degree, self_offset)
  what = what or f'{a.shape[0]} x {b.shape[0]}, E = {a.shape[1]}, degree = {degree}, self_offset = {self_offset}'
  for g, w, name in zip(got, want, ('row_sums', 'col_sums')):
    assert len(g) == len(w) and g == w, f'{what}: {name}: {_first_diff(g, w)}'
  assert sum(got[0]) == sum(got[1])
  return got, want


# ---------------------------------------------------------------------------------------------- 1. kernel sums
GRID_M = [(1, 2), (16, 17), (130, 33), (33, 130), (130, 300)]
GRID_E = [96, 1000, 1056, 12288, 1001]    # two K steps; a K tail that is no multiple of 32; a flush inside; the model's 128 x 96; E % 8 != 0: scalar staging


@pytest.mark.parametrize('degree', [1, 2, 3])
@pytest.mark.parametrize('E', GRID_E)
@pytest.mark.parametrize('Ma,Mb', GRID_M)
def test_kernel_sums_equal_the_restatement(spa3d, Ma, Mb, E, degree):
  a, b = _codes((Ma, E), Ma * 100003 + E), _codes((Mb, E), Mb * 7919 + E + 1)
  _check(spa3d, a, b, degree, -1)


@pytest.mark.parametrize('E', [1, 37])
def test_kernel_sums_of_rows_that_are_no_multiple_of_16_bytes(spa3d, E):
  """E % 8 != 0 stages by guarded scalar loads, as spa3d_motion_pdist does; a base 2 bytes off the grid does too"""
  a, b = _codes((19, E), E), _codes((130, E), E + 1)
  _check(spa3d, a, b, 3, -1)
  buf = torch.zeros(19 * 96 + 1, dtype=torch.int16, device='cuda')
  a96, b96 = _codes((19, 96), 5), _codes((130, 96), 6)
  buf[1:] = _dev(a96).reshape(-1)
  got = _sums_c(spa3d, buf[1:].view(19, 96), _dev(b96), 3, -1)
  assert got == KK.kernel_sums(a96, b96, 3, -1)


@pytest.mark.parametrize('degree', [1, 2, 3])
@pytest.mark.parametrize('Mb', [129, 1])
def test_padded_rows_and_columns_are_masked(spa3d, Mb, degree):
  """A padded row or column of a tile is zeros in LDS, so its p is C, not 0: an unmasked padded column adds C^degree to every row sum (127 of
  them here, for Mb = 129 and for Mb = 1), an unmasked padded row adds it to every column sum (126 of them: Ma = 130 fills 2 rows of its second
  tile).  So ANY size that is no multiple of 128 fails if the mask is missing -- every case of the grid above does; this one is the smallest."""
  E, Ma = 96, 130
  a, b = _codes((Ma, E), 40 + Mb), _codes((Mb, E), 41 + Mb)
  (rows, cols), _ = _check(spa3d, a, b, degree, -1)
  v = KK.powers(a, b, degree)
  assert rows == [int(x) for x in v.sum(1)] and cols == [int(x) for x in v.sum(0)]


def test_limbs_and_carries(spa3d):
  E = 12288
  plus, minus = np.full((130, E), 128, np.int16), np.full((33, E), -128, np.int16)
  # one product already needs the high limb: p = 2 C, p^3 = 27 * 2^81
  cube = (2 * KK.base(E)) ** 3
  assert cube == 27 << 81 and cube >> 64
  (rows, cols), _ = _check(spa3d, plus, -minus, 3, -1, 'all +128 against all +128')
  assert rows == [33 * cube] * 130 and cols == [130 * cube] * 33
  # p = 0 everywhere: every sum is 0 (and the outputs were zeroed, not left as poison)
  (rows, cols), _ = _check(spa3d, plus, minus, 3, -1, 'all +128 against all -128')
  assert rows == [0] * 130 and cols == [0] * 33
  # E = 96, random codes: one p^3 (about 3.9e18) stays under 2^64, a row's sum over 300 columns does not -- the three column tiles' sums are
  # added into the row's limbs by three workgroups, so the carry of the global add is exercised; the same at Ma = 300 for the column sums
  for Ma, Mb in ((16, 300), (300, 16), (300, 300)):
    a, b = _codes((Ma, 96), Ma + 1), _codes((Mb, 96), Mb + 2)
    assert int(KK.powers(a, b, 3).max()) < 1 << 64
    (rows, cols), want = _check(spa3d, a, b, 3, -1)
    if Mb == 300:
      assert any(r >> 64 for r in want[0])
    if Ma == 300:
      assert any(c >> 64 for c in want[1])
  # degree 2 at the widest E: p^2 up to 2^60, 300 of them pass 2^64
  a, b = _codes((20, 32767), 3, 100, 129), _codes((300, 32767), 4, 100, 129)
  (rows, _), want = _check(spa3d, a, b, 2, -1)
  assert any(r >> 64 for r in want[0])


def test_self_exclusion(spa3d):
  x = _codes((200, 96), 21)
  full = KK.powers(x, x, 3)
  (rows, cols), _ = _check(spa3d, x, x, 3, 0)
  assert rows == [int(full[i].sum() - full[i, i]) for i in range(200)] and rows == cols          # the kernel is symmetric
  # a slice of the set, crossing no tile edge and then one: each row leaves its own column out
  (rows, cols), _ = _check(spa3d, x[40:60], x, 3, 40)
  assert rows == [int(full[i].sum() - full[i, i]) for i in range(40, 60)]
  assert cols[39] == int(full[40:60, 39].sum()) and cols[40] == int(full[41:60, 40].sum())
  _check(spa3d, x[100:180], x, 2, 100)
  # -1 leaves nothing out
  (rows, _), _ = _check(spa3d, x[40:60], x, 3, -1)
  assert rows == [int(full[i].sum()) for i in range(40, 60)]
  # an offset that points past Mb excludes nothing; one that leaves only some rows' columns inside excludes those
  assert _check(spa3d, x[:20], x, 3, 200)[0] == _check(spa3d, x[:20], x, 3, -1)[0]
  (rows, _), _ = _check(spa3d, x[:20], x, 3, 190)
  assert rows[9] == int(full[9].sum() - full[9, 199]) and rows[10] == int(full[10].sum())


@pytest.mark.parametrize('degree', [1, 3])
def test_output_selection_and_repeatability(spa3d, degree):
  a, b = _codes((130, 1000), 8), _codes((300, 1000), 9)
  da, db = _dev(a), _dev(b)
  want = KK.kernel_sums(a, b, degree, -1)
  both = _sums_c(spa3d, da, db, degree, -1)
  rows_only, cols_only = _sums_c(spa3d, da, db, degree, -1, cols=False), _sums_c(spa3d, da, db, degree, -1, rows=False)
  assert both == want and rows_only == (want[0], None) and cols_only == (None, want[1])
  assert _sums_c(spa3d, da, db, degree, -1) == both
  # the Python call: int64 [M, 2] limb patterns on the device
  rs, cs = spa3d.motion_kernel_sums(da, db, degree=degree)
  assert rs.dtype == cs.dtype == torch.int64 and rs.is_cuda and tuple(rs.shape) == (130, 2) and tuple(cs.shape) == (300, 2)
  assert np.array_equal(rs.cpu().numpy(), KK.limbs(want[0])) and np.array_equal(cs.cpu().numpy(), KK.limbs(want[1]))
  assert spa3d.limbs_to_ints(rs) == want[0] and spa3d.limbs_to_ints(cs) == want[1]
  rs2, none = spa3d.motion_kernel_sums(da, db, degree=degree, cols=False)
  assert none is None and torch.equal(rs2, rs)
  none, cs2 = spa3d.motion_kernel_sums(da, db, degree=degree, rows=False)
  assert none is None and torch.equal(cs2, cs)
  # codes [M, L, D] are flattened; codes_ref=None leaves each sample out of its own row; query_offset names the slice
  x = _codes((150, 4, 24), 10)
  flat = x.reshape(150, -1)
  assert spa3d.limbs_to_ints(spa3d.motion_kernel_sums(_dev(x), degree=degree)[0]) == KK.kernel_sums(flat, flat, degree, 0)[0]
  assert spa3d.limbs_to_ints(spa3d.motion_kernel_sums(_dev(x[20:140]), _dev(x), degree=degree, query_offset=20)[1]) == KK.kernel_sums(flat[20:140], flat, degree, 20)[1]


@pytest.mark.parametrize('E', [96, 12288])
def test_degree_one_equals_the_summed_dot_products(spa3d, E):
  a, b = _codes((130, E), E + 3), _codes((300, E), E + 4)
  dot = spa3d.motion_pdist(_dev(a), _dev(b), kind='dot').to(torch.int64)
  C_ = KK.base(E)
  rows, cols = _sums_c(spa3d, _dev(a), _dev(b), 1, -1)
  assert rows == (dot.sum(1) + 300 * C_).tolist() and cols == (dot.sum(0) + 130 * C_).tolist()


def test_sums_over_column_ranges_add_up(spa3d):
  a, b = _codes((130, 96), 50), _codes((300, 96), 51)
  da = _dev(a)
  whole = _sums_c(spa3d, da, _dev(b), 3, -1)
  parts = [_sums_c(spa3d, da, _dev(b[lo:hi]), 3, -1) for lo, hi in ((0, 128), (128, 256), (256, 300))]
  assert [sum(p[0][i] for p in parts) for i in range(130)] == whole[0]
  assert parts[0][1] + parts[1][1] + parts[2][1] == whole[1]
  assert any(r >> 64 for r in whole[0])
  # row ranges of a set against itself, the self-exclusion carried by the offset: the rows concatenate, the column sums add up
  x = _codes((300, 96), 52)
  whole = _sums_c(spa3d, _dev(x), _dev(x), 3, 0)
  parts = [_sums_c(spa3d, _dev(x[lo:hi]), _dev(x), 3, lo) for lo, hi in ((0, 128), (128, 256), (256, 300))]
  assert parts[0][0] + parts[1][0] + parts[2][0] == whole[0]
  assert [sum(p[1][j] for p in parts) for j in range(300)] == whole[1]


# ---------------------------------------------------------------------------------------------- 2. the kernel distance
def _same_distance(d, want, subsets=False):
  assert isinstance(d.mmd2, float) and d.mmd2 == want['mmd2'], (d.mmd2, want['mmd2'])
  assert (d.degree, d.base, d.sum_rr, d.sum_gg, d.sum_rg) == (want['degree'], want['base'], want['sum_rr'], want['sum_gg'], want['sum_rg'])
  for name in ('witness_real', 'witness_gen'):
    got = getattr(d, name)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want[name].shape
    assert np.array_equal(got.view(np.int64), want[name].view(np.int64)), name          # bit for bit, the sign of a zero included
  if subsets:
    assert d.subset_values == want['subset_values'] and d.subset_mean == want['subset_mean'] and d.subset_std == want['subset_std']
  else:
    assert d.subset_values is None and d.subset_mean is None and d.subset_std is None


def test_kernel_distance_on_the_hand_case(spa3d):
  real, gen = np.array([[128], [128]], np.int16), np.array([[-128], [-128]], np.int16)
  d = spa3d.kernel_distance(_dev(real), _dev(gen))
  assert isinstance(d, spa3d.KernelDistance) and d.mmd2 == 16.0 and d.degree == 3 and d.base == 16384
  assert d.witness_gen.tolist() == [-8.0, -8.0] and d.witness_real.tolist() == [8.0, 8.0]
  _same_distance(d, KK.kernel_distance(real, gen, 3))
  real6, gen6 = np.array([128, 128, 128, 128, 0, 0], np.int16).reshape(-1, 1), np.array([-128, -128, 128, 128, 128, -128], np.int16).reshape(-1, 1)
  d = spa3d.kernel_distance(_dev(real6), _dev(gen6), subset_size=2)
  assert d.mmd2 == 1.0 and d.subset_values == [16.0, 0.0, -1.0] and d.subset_mean == 5.0
  _same_distance(d, KK.kernel_distance(real6, gen6, 3, subset_size=2), subsets=True)


@pytest.fixture(scope='module')
def model_width_sets():
  """200 real and 150 generated clips at the model's 128 x 96: a generated clip is a real one plus noise of one of three sizes"""
  rng = np.random.default_rng(2)
  real = _codes((200, 128, 96), 1, -40, 41)
  amp = np.array([20.0, 57.0, 90.0])[rng.integers(0, 3, 150)]
  gen = np.clip(real[rng.integers(0, 200, 150)] + np.rint(rng.uniform(-1, 1, (150, 128, 96)) * amp[:, None, None]), -128, 128).astype(np.int16)
  return real, gen


@pytest.mark.parametrize('degree,subset_size', [(3, None), (3, 50), (1, None), (2, 50)])
def test_kernel_distance_equals_the_restatement_at_the_models_width(spa3d, model_width_sets, degree, subset_size):
  """mmd2 and both witness vectors are the restatement's float64 bit for bit: both are one rounding of the same exact rational"""
  real, gen = model_width_sets
  want = KK.kernel_distance(real, gen, degree, subset_size)
  d = spa3d.kernel_distance(_dev(real), _dev(gen), degree=degree, subset_size=subset_size)
  _same_distance(d, want, subsets=subset_size is not None)
  assert (degree == 1 or d.sum_rr >> 64) and d.witness_gen.shape == (150,) and d.witness_real.shape == (200,)
  if subset_size:
    assert len(d.subset_values) == 3 and d.subset_std > 0


@pytest.mark.parametrize('degree', [1, 2, 3])
def test_a_set_against_its_copy_reproduces_the_closed_form(spa3d, degree):
  x = _codes((140, 4, 24), 30 + degree)
  d = spa3d.kernel_distance(_dev(x), _dev(x.copy()), degree=degree)
  want = KK.self_closed_form(x, degree)
  assert d.mmd2 == float(want) and d.mmd2 <= 0 and d.sum_rr == d.sum_gg
  _same_distance(d, KK.kernel_distance(x, x, degree))


def test_kernel_distance_at_4096_stays_within_a_quarter_of_one_matrix(spa3d):
  """No [R, G] tensor: the peak device memory of the call, the inputs included, stays below a quarter of the R * G * 4 bytes of ONE int32 matrix.
  What earlier tests of a whole-suite run still hold is read before this test allocates anything and taken off (as
  tests/test_gpu_motion_knn.py does).  Afterwards the sums are compared with an int64 matrix route that is exact at E = 96: p < 2^22, so with
  p^2 = q1 2^22 + q0 the row sums of p q0 and p q1 stay below 2^56 and p^3's row sum is their combination in Python ints."""
  R = G = 4096
  gc.collect()
  torch.cuda.synchronize()
  torch.cuda.empty_cache()
  held = torch.cuda.memory_allocated()
  g = torch.Generator(device='cuda').manual_seed(0)
  real = torch.randint(-128, 129, (R, 96), generator=g, device='cuda', dtype=torch.int16)
  gen = torch.randint(-100, 129, (G, 96), generator=g, device='cuda', dtype=torch.int16)
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  d = spa3d.kernel_distance(real, gen)
  torch.cuda.synchronize()
  peak = torch.cuda.max_memory_allocated() - held
  print(f'kernel_distance at {R} x {G}: peak {peak / 2 ** 20:.2f} MiB allocated above the {held / 2 ** 20:.1f} MiB other tests hold, one matrix is {R * G * 4 / 2 ** 20:.0f} MiB')
  assert peak < R * G * 4 // 4, (peak, held)
  C_ = KK.base(96)

  def cubes(a, b):
    """(row sums, column sums, diagonal sum) of p^3 as Python ints"""
    p = spa3d.motion_pdist(a, b, kind='dot').to(torch.int64) + C_
    assert int(p.max()) < 1 << 22 and int(p.min()) >= 0
    q = p * p
    s0, s1 = p * (q & ((1 << 22) - 1)), p * (q >> 22)
    join = lambda u, v: [x + (y << 22) for x, y in zip(u.tolist(), v.tolist())]
    return join(s0.sum(1), s1.sum(1)), join(s0.sum(0), s1.sum(0)), sum(join(s0.diagonal(), s1.diagonal()))
  want_rows, want_cols, _ = cubes(gen, real)
  rs, cs = spa3d.motion_kernel_sums(gen, real)
  assert spa3d.limbs_to_ints(rs) == want_rows and spa3d.limbs_to_ints(cs) == want_cols
  assert d.sum_rg == sum(want_rows) and min(want_rows) >> 64
  rr_rows, _, diag = cubes(real, real)
  assert d.sum_rr == sum(rr_rows) - diag
  assert d.mmd2 > 0 and d.witness_gen.shape == (G,)


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_a_refused_call_writes_nothing(spa3d):
  a, b = _dev(_codes((130, 96), 60)), _dev(_codes((130, 96), 61))
  lib, h = spa3d._lib.load(), spa3d.motion._motion_handle()
  assert 'degree = 0' in _sums_c(spa3d, a, b, 0, -1, expect=1)
  assert 'degree = 4' in _sums_c(spa3d, a, b, 4, -1, expect=1)
  assert 'self_offset = -2' in _sums_c(spa3d, a, b, 3, -2, expect=1)
  assert 'one of row_sums and col_sums' in _sums_c(spa3d, a, b, 3, -1, rows=False, cols=False, expect=1)
  rbuf, cbuf = _limb_buffer(130, 'row_sums'), _limb_buffer(130, 'col_sums')
  s, ap, bp, rp, cp = _stream(), a.data_ptr(), b.data_ptr(), rbuf.data_ptr(), cbuf.data_ptr()
  ok = dict(a=ap, Ma=130, b=bp, Mb=130, E=96, degree=3, so=0, rows=rp, cols=cp)

  def call(**kw):
    q = dict(ok, **kw)
    return lib.spa3d_motion_kernel_sums(h, q['a'], q['Ma'], q['b'], q['Mb'], q['E'], q['degree'], q['so'], q['rows'], q['cols'], s)
  for kw, text in ((dict(a=None), 'a is required'), (dict(b=None), 'b is required'), (dict(rows=None, cols=None), 'one of row_sums and col_sums'), (dict(Ma=0), 'Ma = 0'),
                   (dict(Ma=(1 << 22) + 1), 'Ma = 4194305'), (dict(Mb=0), 'Mb = 0'), (dict(Mb=(1 << 22) + 1), 'Mb = 4194305'), (dict(E=0), 'E = 0'), (dict(E=32768), 'E = 32768'),
                   (dict(degree=0), 'degree = 0'), (dict(degree=4), 'degree = 4'), (dict(degree=-1), 'degree = -1'), (dict(so=-2), 'self_offset = -2'),
                   (dict(rows=rp + 4), 'row_sums is not 8-byte aligned'), (dict(cols=cp + 4), 'col_sums is not 8-byte aligned'), (dict(rows=None, cols=cp + 2), 'col_sums is not 8-byte aligned')):
    assert call(**kw) == 1 and text in lib.spa3d_last_error(h).decode(), (kw, lib.spa3d_last_error(h))
  torch.cuda.synchronize()
  assert bool((rbuf == POISON32).all()) and bool((cbuf == POISON32).all())
  assert _ints(rbuf) == [POISON_LIMB | (POISON_LIMB << 64)] * 130
  # the positive control: the same buffers, accepted
  assert call() == 0
  torch.cuda.synchronize()
  want = KK.kernel_sums(a.cpu().numpy(), b.cpu().numpy(), 3, 0)
  assert (_ints(rbuf), _ints(cbuf)) == want
  PU.check_guards()
