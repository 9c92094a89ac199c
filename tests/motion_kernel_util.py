"""Restatement of the kernel sums and the kernel distance (include/spa3d.h, "Kernel sums and the kernel distance"): what
spa3d_motion_kernel_sums and spa3d.kernel_distance must equal exactly.  The dot products are NumPy int64; everything that can pass 2^63 -- the
powers, their sums, the estimate -- is Python ints and fractions.Fraction.  Checked on the CPU by tests/test_motion_kernel_host.py."""
from fractions import Fraction

import numpy as np

import motion_knn_util as KU

MASK64 = (1 << 64) - 1


def base(E):
  """C = 16384 E"""
  return 16384 * int(E)


def dots(a, b):
  """int64 [Ma, Mb] dot products of flat codes, summed by the float64 BLAS: exact, every partial sum is an integer below 32767 * 2^14 < 2^53
  (as motion_knn_util.sqdist, whose note on NumPy's int64 matmul applies)"""
  a, b = np.asarray(a).reshape(len(a), -1).astype(np.int64), np.asarray(b).reshape(len(b), -1).astype(np.int64)
  assert max(np.abs(a).max(), np.abs(b).max()) <= 128 and a.shape[1] == b.shape[1] <= 32767
  return (a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)


def powers(a, b, degree):
  """object array [Ma, Mb] of Python ints p(i, j)^degree, p = a_i . b_j + C"""
  p = dots(a, b) + base(np.asarray(a).reshape(len(a), -1).shape[1])
  assert p.min() >= 0 and p.max() < 1 << 30
  return p.astype(object) ** int(degree)


def kernel_sums(a, b, degree, self_offset):
  """(row_sums, col_sums): lists of Python ints, the sums of p^degree over the admitted pairs (motion_knn_util.admissible)"""
  v = powers(a, b, degree)
  v = np.where(KU.admissible(v.shape[0], v.shape[1], self_offset), v, 0)
  return [int(x) for x in v.sum(1)], [int(x) for x in v.sum(0)]


def limbs(ints):
  """int64 NumPy [M, 2]: the {lo, hi} limb bit patterns of unsigned 128-bit integers, as spa3d.motion_kernel_sums returns them"""
  out = np.empty((len(ints), 2), np.uint64)
  for i, x in enumerate(ints):
    assert 0 <= x < 1 << 128
    out[i] = (x & MASK64, x >> 64)
  return out.view(np.int64)


def from_limbs(arr):
  """the inverse of limbs(): a list of Python ints"""
  u = np.asarray(arr).astype(np.int64).view(np.uint64).reshape(-1, 2)
  return [int(lo) | (int(hi) << 64) for lo, hi in u]


def _once(real, gen, degree):
  real, gen = np.asarray(real).reshape(len(real), -1), np.asarray(gen).reshape(len(gen), -1)
  R, G = len(real), len(gen)
  assert R >= 2 and G >= 2
  Cd = base(real.shape[1]) ** degree
  rr = kernel_sums(real, real, degree, 0)[0]
  gg = kernel_sums(gen, gen, degree, 0)[0]
  gr_rows, gr_cols = kernel_sums(gen, real, degree, -1)
  A, B, X = sum(rr), sum(gg), sum(gr_rows)
  assert X == sum(gr_cols)
  mmd2 = Fraction(A, R * (R - 1) * Cd) + Fraction(B, G * (G - 1) * Cd) - Fraction(2 * X, R * G * Cd)
  w_gen = [Fraction(x, R * Cd) - Fraction(s, (G - 1) * Cd) for x, s in zip(gr_rows, gg)]
  w_real = [Fraction(s, (R - 1) * Cd) - Fraction(x, G * Cd) for s, x in zip(rr, gr_cols)]
  return dict(mmd2_exact=mmd2, mmd2=float(mmd2), degree=degree, base=base(real.shape[1]), sum_rr=A, sum_gg=B, sum_rg=X, witness_gen_exact=w_gen, witness_real_exact=w_real,
              witness_gen=np.array([float(w) for w in w_gen], np.float64), witness_real=np.array([float(w) for w in w_real], np.float64))


def kernel_distance(real, gen, degree=3, subset_size=None):
  """the fields of spa3d.KernelDistance as a dict (plus the exact rationals mmd2_exact, witness_*_exact): mmd2 and the witness values are the
  float64 of their exact rationals; with subset_size the per-subset values, their mean and their population standard deviation (float64 NumPy)"""
  res = _once(real, gen, degree)
  if subset_size is not None:
    s = int(subset_size)
    assert 2 <= s <= min(len(real), len(gen))
    vals = [_once(real[t * s:(t + 1) * s], gen[t * s:(t + 1) * s], degree)['mmd2'] for t in range(min(len(real), len(gen)) // s)]
    res.update(subset_values=vals, subset_mean=float(np.mean(vals)), subset_std=float(np.std(vals)))
  return res


def self_closed_form(x, degree):
  """mmd2 of a set against a copy of itself, as an exact Fraction: 2 (A / (m (m - 1)) - (A + D) / m^2) / C^degree, A the off-diagonal and D the
  diagonal sum of p^degree"""
  x = np.asarray(x).reshape(len(x), -1)
  m = len(x)
  v = powers(x, x, degree)
  D = int(sum(v[i, i] for i in range(m)))
  A = int(v.sum()) - D
  return 2 * (Fraction(A, m * (m - 1)) - Fraction(A + D, m * m)) / base(x.shape[1]) ** degree
