"""NumPy int64 restatements of the latent-set metrics (include/spa3d.h, "Latent-set metrics"): what the kernels of csrc/motion.hip and the
selection of spa3d.precision_recall must equal bit for bit.  Checked on the CPU by tests/test_motion_host.py."""
import numpy as np

TOKEN, CLIP = 0, 1     # SPA3D_POOL_*
DOT, SQDIST = 0, 1     # SPA3D_PDIST_*


def codes(x):
  """(int16 codes, number of NaNs): np.rint (ties to even) of the float32 product clip(x, -1, 1) * 128; a NaN gives 0 and is counted"""
  x = np.asarray(x, np.float32)
  nan = np.isnan(x)
  c = np.clip(np.where(nan, np.float32(0), x), np.float32(-1), np.float32(1)).astype(np.float32) * np.float32(128)
  assert c.dtype == np.float32
  return np.rint(c).astype(np.int16), int(nan.sum())


def f32(bits):
  return np.array([bits], np.uint32).view(np.float32)[0]


def edge_values():
  """float32 inputs at which a rounding, clipping or NaN rule could go wrong, as one array: every tie k + 0.5 (in code units), +-1 and the floats
  next to them on both sides, +-0.0, +-inf, quiet and signalling NaNs of both signs, the smallest subnormal, the largest finite"""
  ties = (np.arange(-128, 128, dtype=np.float64) + 0.5) / 128.0
  near = [np.nextafter(np.float32(s), np.float32(t)) for s in (1.0, -1.0) for t in (0.0, 2.0 * s)]
  odd = [1.0, -1.0, 0.0, -0.0, np.inf, -np.inf, f32(0x7FC00000), f32(0xFFC00000), f32(0x7F800001), f32(0xFF800001), f32(0x00000001), f32(0x80000001),
         np.finfo(np.float32).max, -np.finfo(np.float32).max, 0.49999997 / 128, 127.5 / 128, -127.5 / 128, 1.5, -1.5, 0.00390625, 1e-8]
  return np.concatenate([ties.astype(np.float32), np.array(near, np.float32), np.array(odd, np.float32)])


def samples(c, pool):
  """int64 [n, D]: the token rows, or the per-clip token sums"""
  c = np.asarray(c).astype(np.int64)
  M, L, D = c.shape
  return c.reshape(M * L, D) if pool == TOKEN else c.sum(1)


def moments(c, pool):
  """int64 [1 + D + D * D] = n, s, S of codes [M, L, D]"""
  x = samples(c, pool)
  return np.concatenate([np.array([x.shape[0]], np.int64), x.sum(0), (x.T @ x).reshape(-1)])


def pdist(a, b, kind):
  """int64 [Ma, Mb] of flat codes a [Ma, E], b [Mb, E]"""
  a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
  dot = a @ b.T
  if kind == DOT:
    return dot
  return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * dot


def precision_recall(real, gen, k):
  """(precision, recall) by sorting: a sample's radius is its k-th smallest distance to the OTHER samples of its own set; <= throughout"""
  real, gen = np.asarray(real).reshape(len(real), -1), np.asarray(gen).reshape(len(gen), -1)

  def radii(x):
    d = pdist(x, x, SQDIST)
    out = np.empty(len(x), np.int64)
    for i in range(len(x)):
      out[i] = np.sort(np.delete(d[i], i))[k - 1]
    return out
  rr, rg = radii(real), radii(gen)
  d = pdist(real, gen, SQDIST)
  precision = sum(int((d[:, j] <= rr).any()) for j in range(len(gen))) / len(gen)
  recall = sum(int((d[i, :] <= rg).any()) for i in range(len(real))) / len(real)
  return precision, recall


def stats(state, D, divisor):
  """(n, mean, cov) in latent units from an int64 state, float64: the biased S / n - mu mu^T"""
  n = int(state[0])
  mu = state[1:1 + D].astype(np.float64) / (float(n) * divisor)
  S = state[1 + D:].reshape(D, D).astype(np.float64)
  return n, mu, S / (float(n) * float(divisor) ** 2) - np.outer(mu, mu)
