"""Host side of the kernel sums and the kernel distance, no GPU: the restatement (tests/motion_kernel_util.py) against hand-computed cases and
closed forms; the helpers of csrc/motion_code.hpp built with the host compiler against Python ints BIT FOR BIT (the power in two limbs, the limb
add with its carry, the range check); and the Python refusals, which are raised before anything touches a device."""
import dataclasses
import math
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import motion_kernel_util as KK
import spa3d
from util import host_check_driver


def _col(*v):
  return np.array(v, np.int16).reshape(-1, 1)


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_restatement_on_the_two_set_hand_case():
  """E = 1, C = 16384: 128 * 128 + C = 2 C, so k = 8 inside either set; 128 * -128 + C = 0 across"""
  real, gen = _col(128, 128), _col(-128, -128)
  C = KK.base(1)
  assert C == 16384 == spa3d.motion.kernel_base(1)
  assert KK.kernel_sums(real, real, 3, 0) == ([(2 * C) ** 3] * 2, [(2 * C) ** 3] * 2)
  assert KK.kernel_sums(real, real, 3, -1)[0] == [2 * (2 * C) ** 3] * 2
  assert KK.kernel_sums(gen, real, 3, -1) == ([0, 0], [0, 0])
  d = KK.kernel_distance(real, gen, 3)
  assert d['mmd2_exact'] == 16 and d['mmd2'] == 16.0 and d['base'] == C and d['degree'] == 3
  assert (d['sum_rr'], d['sum_gg'], d['sum_rg']) == (2 * (2 * C) ** 3, 2 * (2 * C) ** 3, 0)
  assert d['witness_gen'].tolist() == [-8.0, -8.0] and d['witness_real'].tolist() == [8.0, 8.0]
  assert d['witness_gen'].dtype == np.float64
  # the means of the witness differ by the estimate, exactly
  assert sum(d['witness_real_exact']) / 2 - sum(d['witness_gen_exact']) / 2 == d['mmd2_exact']


@pytest.mark.parametrize('degree', [1, 2, 3])
def test_a_set_against_itself_gives_the_closed_form(degree):
  assert 1 <= degree <= spa3d.motion.MAX_DEGREE
  rng = np.random.default_rng(degree)
  for m, E in ((2, 1), (5, 3), (9, 96), (4, 12288)):
    x = rng.integers(-128, 129, (m, E)).astype(np.int16)
    d = KK.kernel_distance(x, x.copy(), degree)
    want = KK.self_closed_form(x, degree)
    assert d['mmd2_exact'] == want and d['mmd2'] == float(want)
    assert want <= 0      # A / (m (m - 1)) <= (A + D) / m^2 <=> A <= (m - 1) D: Cauchy-Schwarz in the kernel's feature space
  # written out for three codes at E = 1: p = x y + C
  x, C = _col(128, -128, 64), 16384
  p = lambda u, v: (u * v + C) ** degree
  A = 2 * (p(128, -128) + p(128, 64) + p(-128, 64))
  D = p(128, 128) + p(-128, -128) + p(64, 64)
  assert KK.self_closed_form(x, degree) == 2 * (Fraction(A, 6) - Fraction(A + D, 9)) / C ** degree == KK.kernel_distance(x, x, degree)['mmd2_exact']


def test_degree_one_is_the_sum_of_dots_plus_count_times_base():
  rng = np.random.default_rng(7)
  a, b = rng.integers(-128, 129, (7, 40)).astype(np.int16), rng.integers(-128, 129, (11, 40)).astype(np.int16)
  dot, C = a.astype(np.int64) @ b.astype(np.int64).T, KK.base(40)
  assert C == spa3d.motion.kernel_base(40)
  assert np.array_equal(KK.dots(a, b), dot)
  rows, cols = KK.kernel_sums(a, b, 1, -1)
  assert rows == (dot.sum(1) + 11 * C).tolist() and cols == (dot.sum(0) + 7 * C).tolist()
  rows, cols = KK.kernel_sums(a, b, 1, 2)          # row i leaves column i + 2 out: every row has 10 columns, columns 2 .. 8 have 6 rows
  keep = np.ones((7, 11), bool)
  keep[np.arange(7), np.arange(7) + 2] = False
  assert rows == ((dot * keep).sum(1) + 10 * C).tolist() and cols == ((dot * keep).sum(0) + keep.sum(0) * C).tolist()
  assert keep.sum(0).tolist() == [7, 7, 6, 6, 6, 6, 6, 6, 6, 7, 7]
  rows, cols = KK.kernel_sums(a, b, 1, 11)         # an offset past Mb leaves nothing out
  assert rows == (dot.sum(1) + 11 * C).tolist()


def test_subsets_of_a_six_plus_six_case_computed_by_hand():
  """E = 1: x y / C is 1, -1 or 0 for codes from {128, -128, 0}, so k is 8, 0 or 1.
  subset 0: real (128, 128), gen (-128, -128): 8 + 8 - 0 = 16.   subset 1: real = gen = (128, 128): 8 + 8 - 2 * 8 = 0.
  subset 2: real (0, 0), gen (128, -128): 1 + 0 - 2 * 1 = -1.   mean 5, population variance (11^2 + 5^2 + 6^2) / 3 = 182 / 3."""
  real, gen = _col(128, 128, 128, 128, 0, 0), _col(-128, -128, 128, 128, 128, -128)
  d = KK.kernel_distance(real, gen, 3, subset_size=2)
  assert {f.name for f in dataclasses.fields(spa3d.KernelDistance)} <= set(d)          # the restatement has every field of the result
  assert d['subset_values'] == [16.0, 0.0, -1.0] and d['subset_mean'] == 5.0 and d['subset_std'] == pytest.approx(math.sqrt(182 / 3), rel=1e-15)
  # the whole sets: real-real ordered pairs 12 of k = 8, 16 of k = 1 (a zero with anything), 2 of k = 1 (the zeros): A = 96 + 18 = 114 of 30;
  # gen-gen: +: {2, 3, 4}, -: {0, 1, 5}: 6 + 6 ordered pairs of k = 8 inside a sign, 18 of k = 0 across: B = 96 of 30;
  # cross: real + (4) with gen + (3): 12 of 8; real + with gen -: 0; real 0 (2) with anything (6): 12 of 1: X = 108 of 36
  assert d['mmd2_exact'] == Fraction(114, 30) + Fraction(96, 30) - Fraction(2 * 108, 36) == 1
  assert d['sum_rr'] == 114 * 16384 ** 3 and d['sum_gg'] == 96 * 16384 ** 3 and d['sum_rg'] == 108 * 16384 ** 3
  # subset_size = 4: one subset, the last two samples of either set left over; 6: the whole sets
  assert len(KK.kernel_distance(real, gen, 3, subset_size=4)['subset_values']) == 1
  d6 = KK.kernel_distance(real, gen, 3, subset_size=6)
  assert d6['subset_values'] == [1.0] and d6['subset_std'] == 0.0


def test_limbs_round_trip():
  ints = [0, 1, (1 << 63), (1 << 64) - 1, 1 << 64, (1 << 112), (1 << 128) - 1, 0xDEADBEEF << 70]
  arr = KK.limbs(ints)
  assert arr.dtype == np.int64 and arr.shape == (8, 2) and arr[2].tolist() == [-(1 << 63), 0] and arr[3].tolist() == [-1, 0] and arr[4].tolist() == [0, 1]
  assert KK.from_limbs(arr) == ints
  assert spa3d.limbs_to_ints(torch.from_numpy(arr)) == ints
  for bad in (torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64), arr):
    with pytest.raises(ValueError, match='limbs'):
      spa3d.limbs_to_ints(bad)


# ---------------------------------------------------------------------------------------------- the header against Python ints
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
  return host_check_driver(tmp_path_factory, 'motion_kernel')


def _ask(driver, lines):
  out = subprocess.run([driver], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=120)
  assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
  res = out.stdout.splitlines()
  assert len(res) == len(lines)
  return res


def _pairs(driver, lines):
  return [tuple(int(t) for t in r.split()) for r in _ask(driver, lines)]


def _split(x):
  return (x & KK.MASK64, x >> 64)


def test_header_power_in_two_limbs(driver):
  assert _ask(driver, ['consts']) == ['3 12 16']
  widths = (1, 96, 12288, 32767)
  assert [int(r) for r in _ask(driver, [f'base {E}' for E in widths])] == [KK.base(E) for E in widths]
  ps = [p for E in widths for p in (0, 1, KK.base(E), 2 * KK.base(E))] + np.random.default_rng(0).integers(0, 1 << 30, 1000).tolist() + [(1 << 30) - 1, 1 << 16, (1 << 16) + 1, 65535, 2642246]
  assert max(ps) < 1 << 30 and 2 * KK.base(32767) == max(ps[:16])
  for degree in (1, 2, 3):
    got = _pairs(driver, [f'pow {p} {degree}' for p in ps])
    assert got == [_split(p ** degree) for p in ps], degree
    assert (degree == 3) == any(hi for _, hi in got)
  # p itself: the exact dot product shifted by C, at both ends of its range
  q = [(-KK.base(E), E) for E in widths] + [(KK.base(E), E) for E in widths] + [(0, 96), (-1, 96), (12345, 12288)]
  assert [int(r) for r in _ask(driver, [f'p {d} {E}' for d, E in q])] == [d + KK.base(E) for d, E in q]


def test_header_limb_add_carries(driver):
  M = KK.MASK64
  rng = np.random.default_rng(1)
  cases = [((M, 0), (1, 0)),                      # lo sums to exactly 2^64
           ((M, 5), (M, 7)),                      # lo wraps, to M - 1
           ((1 << 63, 0), (1 << 63, 0)),          # exactly 2^64 again, from two equal halves
           ((123, 0), (456, 0)), ((0, 0), (0, 0)), ((M, 0), (0, 0)), ((0, 0), (M, 0)),       # hi = 0, no carry
           ((M, M >> 16), (M, 0)), ((7, 1 << 47), (M - 6, 1 << 47))]
  cases += [((int(a), int(b)), (int(c), int(d))) for a, b, c, d in zip(rng.integers(0, 1 << 64, 300, dtype=np.uint64), rng.integers(0, 1 << 48, 300, dtype=np.uint64),
                                                                      rng.integers(0, 1 << 64, 300, dtype=np.uint64), rng.integers(0, 1 << 48, 300, dtype=np.uint64))]
  got = _pairs(driver, [f'add {a[0]} {a[1]} {b[0]} {b[1]}' for a, b in cases])
  want = [_split((a[0] + (a[1] << 64) + b[0] + (b[1] << 64)) % (1 << 128)) for a, b in cases]
  assert got == want
  assert got[0] == (0, 1) and got[1] == (M - 1, 13) and got[2] == (0, 1) and got[3] == (579, 0)
  assert sum(1 for (a, b) in cases if a[0] + b[0] > M) > 100      # the carry is exercised
  # a running sum of powers, as the kernel keeps it: 5000 of the largest cube pass 2^97
  top = (2 * KK.base(32767)) ** 3
  acc = (0, 0)
  for n in (1, 2, 3):
    acc = _pairs(driver, [f'add {acc[0]} {acc[1]} {top & M} {top >> 64}'])[0]
    assert acc == _split(n * top)


def test_header_refusal_table(driver):
  OK, BAD_M, BAD_E, BAD_MB, BAD_SELF, BAD_DEGREE = 0, 1, 5, 7, 10, 12
  M = 1 << 22
  cases = [('ksum 1 1 1 1 -1', OK), ('ksum 130 300 12288 3 0', OK), (f'ksum {M} {M} 32767 3 {M}', OK), ('ksum 2 2 96 2 5', OK),
           ('ksum 0 2 96 3 0', BAD_M), ('ksum -1 2 96 3 0', BAD_M), (f'ksum {M + 1} 2 96 3 0', BAD_M),
           ('ksum 2 0 96 3 0', BAD_MB), (f'ksum 2 {M + 1} 96 3 0', BAD_MB),
           ('ksum 2 2 0 3 0', BAD_E), ('ksum 2 2 -5 3 0', BAD_E), ('ksum 2 2 32768 3 0', BAD_E),
           ('ksum 2 2 96 0 0', BAD_DEGREE), ('ksum 2 2 96 4 0', BAD_DEGREE), ('ksum 2 2 96 -3 0', BAD_DEGREE), ('ksum 2 2 96 2147483647 0', BAD_DEGREE),
           ('ksum 2 2 96 3 -2', BAD_SELF), ('ksum 2 2 96 3 -9223372036854775808', BAD_SELF),
           # the sizes are said first, then the degree, then the offset
           ('ksum 0 0 0 0 -2', BAD_M), ('ksum 2 0 0 0 -2', BAD_MB), ('ksum 2 2 0 0 -2', BAD_E), ('ksum 2 2 96 0 -2', BAD_DEGREE)]
  assert [int(v) for v in _ask(driver, [c for c, _ in cases])] == [w for _, w in cases]


# ---------------------------------------------------------------------------------------------- Python refusals
def test_cpu_tensors_and_bad_arguments_are_refused():
  c = torch.zeros(6, 4, 5, dtype=torch.int16)
  E = spa3d._lib.Spa3dError
  for call in (lambda: spa3d.motion_kernel_sums(c), lambda: spa3d.motion_kernel_sums(c, c, degree=2), lambda: spa3d.motion_kernel_sums(c[2:], c, query_offset=2, cols=False),
               lambda: spa3d.kernel_distance(c, c), lambda: spa3d.kernel_distance(c, c[:2], degree=1, subset_size=2)):
    with pytest.raises(E, match='HIP-only'):
      call()
  for degree in (0, 4, -1, True, 3.0, None):
    with pytest.raises(ValueError, match='degree'):
      spa3d.motion_kernel_sums(c, degree=degree)
    with pytest.raises(ValueError, match='degree'):
      spa3d.kernel_distance(c, c, degree=degree)
  for bad in (c.int(), c.float()):
    with pytest.raises(ValueError, match='int16'):
      spa3d.motion_kernel_sums(bad)
    with pytest.raises(ValueError, match='int16'):
      spa3d.motion_kernel_sums(c, bad)
    with pytest.raises(ValueError, match='int16'):
      spa3d.kernel_distance(c, bad)
    with pytest.raises(ValueError, match='int16'):
      spa3d.kernel_distance(bad, c)
  with pytest.raises(ValueError, match='elements per sample'):
    spa3d.motion_kernel_sums(c, c[:, :, :4])
  with pytest.raises(ValueError, match='elements per sample'):
    spa3d.kernel_distance(c, c[:, :3])
  with pytest.raises(ValueError, match='tensor'):
    spa3d.kernel_distance(np.zeros((3, 4), np.int16), c)
  with pytest.raises(ValueError, match='at least 2'):
    spa3d.kernel_distance(c[:1], c)
  with pytest.raises(ValueError, match='at least 2'):
    spa3d.kernel_distance(c, c[:1])
  for s in (1, 0, -2, True, 2.0):
    with pytest.raises(ValueError, match='subset_size'):
      spa3d.kernel_distance(c, c, subset_size=s)
  with pytest.raises(ValueError, match='subset_size = 7'):
    spa3d.kernel_distance(c, c, subset_size=7)
  with pytest.raises(ValueError, match='subset_size = 5'):
    spa3d.kernel_distance(c, c[:4], subset_size=5)
  with pytest.raises(ValueError, match='rows and cols'):
    spa3d.motion_kernel_sums(c, rows=False, cols=False)
  with pytest.raises(ValueError, match='needs codes_ref'):
    spa3d.motion_kernel_sums(c, query_offset=1)
  with pytest.raises(ValueError, match='runs past'):
    spa3d.motion_kernel_sums(c, c, query_offset=1)
