"""NumPy int64 restatements of the streaming k-NN, the ball hits and the manifold estimates (include/spa3d.h, "Streaming k-NN and ball hits"):
what spa3d_motion_knn, spa3d_motion_ball_hits and spa3d.manifold_metrics must equal exactly.  Checked on the CPU by
tests/test_motion_knn_host.py."""
import numpy as np

import motion_util as MU

NONE = (1 << 64) - 1     # MC_KNN_NONE: no key


def sqdist(a, b):
  """int64 [Ma, Mb] squared distances of flat codes: MU.pdist(a, b, MU.SQDIST) to the bit, with the products summed by the float64 BLAS -- exact,
  every partial sum is an integer below 32767 * 2^14 < 2^53 -- because NumPy's int64 matmul takes seconds at E = 12288"""
  a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
  assert max(np.abs(a).max(), np.abs(b).max()) <= 128 and a.shape[1] <= 32767
  dot = (a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)
  return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * dot


def admissible(Ma, Mb, self_offset):
  """bool [Ma, Mb]: column j may be taken by row i (self_offset >= 0 leaves j == i + self_offset out, -1 nothing)"""
  ok = np.ones((Ma, Mb), bool)
  if self_offset >= 0:
    i = np.arange(Ma)
    j = i + self_offset
    ok[i[j < Mb], j[j < Mb]] = False
  return ok


def keys(a, b, self_offset):
  """uint64 [Ma, Mb]: d(i, j) << 32 | j, NONE where the column is not admissible"""
  d = sqdist(a, b)
  assert d.min() >= 0 and d.max() < 1 << 31
  key = (d.astype(np.uint64) << np.uint64(32)) | np.arange(d.shape[1], dtype=np.uint64)[None, :]
  return np.where(admissible(d.shape[0], d.shape[1], self_offset), key, np.uint64(NONE))


def knn(a, b, k, self_offset):
  """(dist int64 [Ma, k], idx int64 [Ma, k]): the k nearest admissible rows of b, by a STABLE sort on the distance (equal distances keep the
  order of the columns: the lower index first)"""
  d = sqdist(a, b)
  ok = admissible(d.shape[0], d.shape[1], self_offset)
  dist, idx = np.empty((len(d), k), np.int64), np.empty((len(d), k), np.int64)
  for i in range(len(d)):
    cols = np.flatnonzero(ok[i])
    assert len(cols) >= k
    order = cols[np.argsort(d[i, cols], kind='stable')][:k]
    dist[i], idx[i] = d[i, order], order
  return dist, idx


def ball_hits(a, b, radius, self_offset):
  """(row_hits int64 [Ma], col_hits int64 [Mb]) of hit(i, j) = d(i, j) <= radius[i] over the admissible columns"""
  d = sqdist(a, b)
  hit = (d <= np.asarray(radius).astype(np.int64)[:, None]) & admissible(d.shape[0], d.shape[1], self_offset)
  return hit.sum(1), hit.sum(0)


def manifold(real, gen, k):
  """the estimates and per-sample arrays of spa3d.manifold_metrics, as a dict"""
  real, gen = np.asarray(real).reshape(len(real), -1), np.asarray(gen).reshape(len(gen), -1)
  rad_r, rad_g = knn(real, real, k, 0)[0][:, k - 1], knn(gen, gen, k, 0)[0][:, k - 1]
  real_ball_hits, gen_in_real = ball_hits(real, gen, rad_r, -1)
  _, real_in_gen = ball_hits(gen, real, rad_g, -1)
  R, G = len(real), len(gen)
  return dict(precision=int((gen_in_real > 0).sum()) / G, recall=int((real_in_gen > 0).sum()) / R, density=int(gen_in_real.sum()) / (k * G),
              coverage=int((real_ball_hits > 0).sum()) / R, real_radius=rad_r, gen_radius=rad_g, gen_in_real_balls=gen_in_real, real_in_gen_balls=real_in_gen,
              real_ball_hits=real_ball_hits)


def tie_sets():
  """(real [6, 4, 6], gen [7, 4, 6]) int16: the hand-built sets of tests/test_gpu_motion.py's precision / recall test -- duplicates and exact ties"""
  L, D = 4, 6

  def clip(*moves):
    c = np.zeros(L * D, np.int16)
    for e, v in moves:
      c[e] += v
    return c.reshape(L, D)
  real = np.stack([clip(), clip(), clip((0, 3)), clip((1, 3)), clip((0, 3), (1, 4)), clip((5, 100))])
  gen = np.stack([clip(), clip((0, 3)), clip((0, 3)), clip((2, 5)), clip((1, -3)), clip((5, 128)), clip((5, -128))])
  return real, gen


HAND_REAL = np.array([0, 2, 4, 40, 120, 122], np.int16).reshape(-1, 1)
HAND_GEN = np.array([1, 3, 25, -100], np.int16).reshape(-1, 1)
HAND = dict(real_radius=[4, 4, 4, 1296, 4, 4], gen_radius=[4, 4, 484, 10201], gen_in_real_balls=[2, 2, 1, 0], real_ball_hits=[1, 2, 1, 1, 0, 0],
            precision=3 / 4, density=5 / 4, coverage=4 / 6, recall=4 / 6)
