"""References and gates of the loss, loss-scale, AdamW-guard and AdamW kernels of csrc/loss.hip (tests/test_gpu_loss_ops.py), plain numpy: the
objective and the head cotangent of include/spa3d.h ("The training objective") with csrc/loss_point.hpp's formulas, in float64 (the reference) and in
float32 (the restatement, operation for operation); the loss scale; the guard's state machine as the header words it under spa3d_adamw_step; AdamW at one
call.  Every function takes the wrong variants the gates must reject (tests/test_loss_ref_host.py shows that they do).  No fixtures, no GPU."""
import collections
import math

import numpy as np

F32 = np.float32
CAP = 1 << 20   # 4096 workgroups x 256 threads: beyond this many elements head_loss_fwd, loss_from_preds and adamw_kernel take a second pass

Obj = collections.namedtuple('Obj', 'l1_weight bce_weight position_kind huber_delta axis_weight bce_pos_weight', defaults=(5000.0, 1e-8, 0, 1.0, (1.0, 1.0, 1.0), 1.0))


def gmax(o, nc=3):
  """spa3d_set_loss: the largest head gradient per unit point weight, in fp32 as the library forms it"""
  return max(F32(o.l1_weight) * max(F32(a) for a in o.axis_weight[:nc]), F32(o.bce_weight) * max(F32(1.0), F32(o.bce_pos_weight)))


# ------------------------------------------------------------------------------------------------ inputs
def draw_case(nq, T, nc, seed, weights=True):
  """head [nq, 4 T] (standard-normal coordinates, logits N(0, 4^2), a normal 4th block), targets [nq, T, nc], visible [nq, T] Bernoulli(0.7),
  weights [nq, T] from U[0, 2) or None; float32"""
  r = np.random.default_rng(seed)
  head = r.standard_normal((nq, 4, T)).astype(F32)
  head[:, nc] *= F32(4.0)
  tgt = r.standard_normal((nq, T, nc)).astype(F32)
  vis = (r.random((nq, T)) < 0.7).astype(F32)
  w = (r.random((nq, T)) * 2.0).astype(F32) if weights else None
  return head.reshape(nq, 4 * T), tgt, vis, w


def split_head(head, T, nc):
  """the head's blocks as the split predictions: tracks [nq, T, nc], visible logits [nq, T], certainty logits [nq, T] (zeros for nc == 3)"""
  h = head.reshape(-1, 4, T)
  return np.ascontiguousarray(h[:, :nc].transpose(0, 2, 1)), np.ascontiguousarray(h[:, nc]), (np.ascontiguousarray(h[:, 3]) if nc == 2 else np.zeros_like(h[:, 3]))


# ------------------------------------------------------------------------------------------------ one point (loss_point.hpp)
def _logsig(x):
  return np.minimum(x, x.dtype.type(0)) - np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
  one = x.dtype.type(1)
  return one / (one + np.exp(-x))


def pos_value(o, d, variant=None):
  a = np.abs(d)
  if o.position_kind == 1:
    dl = d.dtype.type(o.huber_delta)
    inside = (a < dl) if variant == 'huber_lt' else (a <= dl)
    return np.where(inside, d * d / (d.dtype.type(2) * dl), a - d.dtype.type(0.5) * dl)
  return a


def pos_deriv(o, d, variant=None):
  one = d.dtype.type(1)
  sgn = np.where(d > 0, one, np.where(d < 0, -one, one if variant == 'sign0' else d.dtype.type(0)))
  if o.position_kind == 1:
    dl = d.dtype.type(o.huber_delta)
    inside = (np.abs(d) < dl) if variant == 'huber_lt' else (np.abs(d) <= dl)
    return np.where(inside, d / dl, sgn)
  return sgn


def vis_value(o, y, l):
  dt = l.dtype.type
  return -(dt(o.bce_pos_weight) * y) * _logsig(l) - (dt(1) - y) * _logsig(-l)


def vis_deriv(o, y, l):
  dt = l.dtype.type
  s = _sigmoid(l)
  if F32(o.bce_pos_weight) == F32(1.0):
    return s - y
  return dt(o.bce_pos_weight) * y * (s - dt(1)) + (dt(1) - y) * s


# ------------------------------------------------------------------------------------------------ the objective
def point_terms(o, tracks, vlog, tgt, vis, w, dtype, variant=None):
  """(w y e, w v) of every point, [n] each, evaluated in `dtype` in the kernels' order of operations: float64 is the reference, float32 the restatement.
  variant 'swap_yw': the visibility target and the point weight change places; 'huber_lt': the Huber branch taken at < instead of <=."""
  nc = tracks.shape[-1]
  t, g, y, l = (np.asarray(x, dtype=dtype) for x in (tracks.reshape(-1, nc), tgt.reshape(-1, nc), vis.reshape(-1), vlog.reshape(-1)))
  wt = np.ones_like(y) if w is None else np.asarray(w, dtype=dtype).reshape(-1)
  if variant == 'swap_yw':
    y, wt = wt, y
  perr = np.zeros_like(y)
  for c in range(nc):
    perr = perr + dtype(F32(o.axis_weight[c])) * pos_value(o, t[:, c] - g[:, c], variant)
  return perr * y * wt, vis_value(o, y, l) * wt


def numerators(pt, vt, variant=None):
  """(P, V): the sums of the two term vectors in their own dtype -- float64: the reference (fsum, exact); float32: numpy's pairwise sum, one order a kernel may take.
  variant 'drop' / 'twice': the element at index CAP (the first one of the kernels' second pass) left out / counted twice."""
  out = []
  for x in (pt, vt):
    s = math.fsum(x.tolist()) if x.dtype == np.float64 else float(np.sum(x, dtype=F32))
    if variant in ('drop', 'twice') and x.size > CAP:
      s = s + (-1.0 if variant == 'drop' else 1.0) * float(x[CAP])
      s = s if x.dtype == np.float64 else float(F32(s))
    out.append(s)
  return tuple(out)


def numerator_bound(terms):
  """|got - ref64| allowed for a numerator: 16 2^-24 sum |terms| + 4096 2^-25.  At most 5 sequential adds per thread, a 6-level wave tree and 3 adds across
  the waves of a workgroup are 14 fp32 roundings on any path from a term to its workgroup's partial, a few ulp in expf / log1pf sit in the term itself (16 in all);
  each of at most 4096 workgroups rounds its partial once to the 2^-24 fixed-point unit (half a unit each)."""
  return 16.0 * 2.0 ** -24 * math.fsum(np.abs(terms.astype(np.float64)).tolist()) + 4096 * 2.0 ** -25


def denominator(vis, denom):
  return float(F32(denom)) if denom > 0 else max(float(np.asarray(vis, dtype=np.float64).sum()), 1.0)


def loss3_from(o, P, V, D):
  """{total, position, visible} as loss_finalize_kernel forms them in fp32 from the fp32 numerators and the denominator"""
  pos, v = F32(P) / F32(D), F32(V) / F32(D)
  return F32(F32(F32(o.l1_weight) * pos) + F32(F32(o.bce_weight) * v)), pos, v


def total_of(o, pos, vis):
  """loss3[0] from loss3[1] and loss3[2], in fp32, without contraction"""
  return F32(F32(F32(o.l1_weight) * F32(pos)) + F32(F32(o.bce_weight) * F32(vis)))


# ------------------------------------------------------------------------------------------------ the head cotangent
def head_cotangent(o, head, tgt, vis, w, T, nc, D, scale, dtype, variant=None):
  """d loss / d head times the loss scale, [nq, 4 T] in `dtype`, in loss_bwd_kernel's order of operations.  Also K [nq, 4 T] (float64): the magnitude at
  which an entry cancels -- bce_weight max(1, beta) w scale / D on the visibility block (sigmoid(l) - y loses what y had), 0 elsewhere.
  variant 'sign0': sign(0) = 1; 'certain': the certainty block carries the visibility gradient; 'huber_lt'."""
  h = np.asarray(head, dtype=dtype).reshape(-1, 4, T)
  g = np.asarray(tgt, dtype=dtype)
  y = np.asarray(vis, dtype=dtype)
  one = dtype(1)
  wt = np.ones_like(y) if w is None else np.asarray(w, dtype=dtype)
  inv = dtype(F32(scale)) / dtype(F32(D))
  out = np.zeros_like(h)
  for c in range(nc):
    out[:, c] = dtype(F32(o.l1_weight)) * (dtype(F32(o.axis_weight[c])) * pos_deriv(o, h[:, c] - g[:, :, c], variant)) * y * wt * inv
  vg = dtype(F32(o.bce_weight)) * vis_deriv(o, y, h[:, nc])
  out[:, nc] = vg * wt * inv
  if nc == 2 and variant == 'certain':
    out[:, 3] = vg * one * inv
  K = np.zeros(h.shape, dtype=np.float64)
  K[:, nc] = float(F32(o.bce_weight)) * max(1.0, float(F32(o.bce_pos_weight))) * wt.astype(np.float64) * float(F32(scale)) / float(F32(D))
  return out.reshape(-1, 4 * T), K.reshape(-1, 4 * T)


HALF_ULP = {'bf16': 2.0 ** -9, 'fp16': 2.0 ** -12}   # one rounding of the storage type, relative to the power of two above the value: half an ulp (8 / 11 significand bits)
E_MIN = {'bf16': -126, 'fp16': -14}                  # smallest normal exponent: below it the step stops shrinking


def rounding_allowance(ref64, precision):
  """What ONE round-to-nearest of `precision` may move a value near ref: half an ulp there, 2^-9 (bf16) / 2^-12 (fp16) of the power of two above |ref| -- half the
  subnormal step below the normal range; 0 for fp32.  The figures are relative to that power of two, not to |ref|: 2^-9 |ref| is half of what a correct
  rounding of a value just above a power of two costs (measured on the kernel and on torch's own cast: 1.98 x).  (|ref| is taken 2^-20 larger: the fp32 value being rounded may sit across a binade boundary from ref.)"""
  if precision == 'fp32':
    return np.zeros(np.shape(ref64))
  _, ex = np.frexp(np.abs(ref64) * (1.0 + 2.0 ** -20))   # |x| = m 2^ex with m in [0.5, 1): 2^ex is the power of two above |x|
  return HALF_ULP[precision] * np.exp2(np.maximum(ex, E_MIN[precision] + 1).astype(np.float64))


def cotangent_report(got, ref64, K, precision):
  """(entries over the gate, worst |got - ref| / bound): |got - ref| <= 8 2^-24 max(|ref|, K) + one rounding of the storage type (rounding_allowance).
  An entry whose value overflows fp16 must be +-inf, not a finite number."""
  got = np.asarray(got, dtype=np.float64)
  bound = 8.0 * 2.0 ** -24 * np.maximum(np.abs(ref64), K) + rounding_allowance(ref64, precision)
  over = np.abs(ref64) > 65520.0 if precision == 'fp16' else np.zeros(ref64.shape, dtype=bool)
  err = np.abs(np.where(over, 0.0, got) - np.where(over, 0.0, ref64))
  bad = ~(err <= bound)
  bad |= over & ~(np.isinf(got) & (np.sign(got) == np.sign(ref64)))
  ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
  return int(bad.sum()), float(np.nanmax(ratio)) if ratio.size else 0.0


# ------------------------------------------------------------------------------------------------ the exact lane
EXACT_OBJ = Obj(5000.0, 1e-8, 1, 0.125, (1.0, 2.0, 4.0), 4.0)   # Huber, delta 2^-3; every weight a power of two
P_GRID, V_GRID = 2.0 ** -6, 16.0


def exact_case(nq, T, nc, seed, extra=20000):
  """A case whose every intermediate is exactly representable, so the two numerators have one right answer bit for bit.
  Background points add exactly zero: (y = 0, logit -200), or (y = 1, logit +200, prediction == target).  Nonzero points: position error a multiple of 2^-4
  in [-2, 2] (both Huber branches: |d| <= 2^-3 gives 4 d^2, a multiple of 2^-6), point weight 1 or 2, and a logit on the side where the visibility term is
  exactly |l| (y = 1, l = -32 / -64: beta |l|; y = 0, l = +32 / +64: |l|) or exactly 0 (y = 1, l = +200).  They sit at every index within 512 of 0, of CAP and
  of n, and at `extra` random indices.  -> head, targets, visible, weights, P (exact), V (exact), the exact visible count."""
  o = EXACT_OBJ
  n = nq * T
  r = np.random.default_rng(seed)
  idx = np.unique(np.concatenate([np.arange(0, min(512, n)), np.arange(max(CAP - 512, 0), min(CAP + 512, n)) if n > CAP - 512 else np.arange(0),
                                  np.arange(max(n - 512, 0), n), r.integers(0, n, size=min(extra, n))]))
  k = idx.size
  y = np.zeros(n, dtype=F32)
  y[r.random(n) < 0.5] = 1.0        # background of both kinds
  lg = np.where(y > 0, F32(200.0), F32(-200.0)).astype(F32)
  tgt = (r.integers(-64, 65, size=(n, nc)) / 16.0).astype(F32)
  pred = tgt.copy()
  w = np.ones(n, dtype=F32)
  yk = (r.random(k) < 0.6).astype(F32)
  y[idx] = yk
  d = (r.integers(-32, 33, size=(k, nc)) / 16.0).astype(F32)
  d[r.random(k) < 0.15] = 0.0       # prediction == target at a nonzero point: gradient 0
  pred[idx] = tgt[idx] + d
  assert np.array_equal(pred[idx] - tgt[idx], d)   # multiples of 2^-4 below 8: the difference is exact
  w[idx] = r.choice(np.array([1.0, 2.0], dtype=F32), size=k)
  mag = r.choice(np.array([32.0, 64.0], dtype=F32), size=k)
  lk = np.where(yk > 0, -mag, mag).astype(F32)
  lk[(yk > 0) & (r.random(k) < 0.2)] = 200.0
  lg[idx] = lk
  head = np.zeros((nq, 4, T), dtype=F32)
  head[:, :nc] = pred.reshape(nq, T, nc).transpose(0, 2, 1)
  head[:, nc] = lg.reshape(nq, T)
  if nc == 2:
    head[:, 3] = r.standard_normal((nq, T)).astype(F32)
  # in fp32: -32 - log1p(exp(-32)) rounds to -32 there (and on the device, whatever its expf: the addend is 1e-14), not in float64
  pt, vt = (x.astype(np.float64) for x in point_terms(o, pred.reshape(nq, T, nc), lg, tgt.reshape(nq, T, nc), y, w, F32))
  P, V = float(pt.sum()), float(vt.sum())
  for terms, grid in ((pt, P_GRID), (vt, V_GRID)):
    q = terms / grid
    assert np.array_equal(q, np.round(q)) and np.abs(q).sum() < 2 ** 24, 'the lane must stay exact in fp32 in any order of summation'
  return head.reshape(nq, 4 * T), tgt.reshape(nq, T, nc), y.reshape(nq, T), w.reshape(nq, T), P, V, float(y.astype(np.float64).sum())


# ------------------------------------------------------------------------------------------------ the loss scale
def floor_log2(q):
  """floor(log2 q) of a positive finite float, exactly (frexp)"""
  m, e = math.frexp(float(q))
  return e - 1


def loss_scale_ref(denom, gm, setting, state=None, variant=None):
  """The scale set_loss_scale_kernel must produce: setting > 0 that value; setting < 0 the largest power of two with gm / denom * scale <= |setting|,
  taken on q = fl(fl(denom |setting|) / gm) in fp32 and clamped to [1, 2^24]; then times the state multiplier when that lies in (0, 1), floored at 2^-24.
  variant 'round': log2 rounded to nearest instead of floored."""
  s = float(F32(setting))
  if setting < 0:
    q = float(F32(F32(F32(denom) * F32(-setting)) / F32(gm)))
    e = floor_log2(q) if variant != 'round' else int(round(math.log2(q)))
    s = min(max(2.0 ** e, 1.0), 2.0 ** 24)
  if state is not None and 0.0 < float(F32(state)) < 1.0:
    s = max(float(F32(F32(s) * F32(state))), 2.0 ** -24)
  return s


def loss_scale_log2_route(denom, gm, setting):
  """exp2(floor(log2(q))) clamped, in numpy float32: set_loss_scale_kernel's expression.  numpy's log2 rounds to k an ulp or two below 2^k and this route is then a
  power of two too high (tests/test_loss_ref_host.py); the device's log2f does not: the kernel meets the frexp reference at every boundary
  (tests/test_gpu_loss_ops.py::test_loss_scale_at_every_power_of_two_boundary)"""
  q = F32(F32(F32(denom) * F32(-setting)) / F32(gm))
  return float(min(max(np.exp2(np.floor(np.log2(q))), F32(1.0)), F32(2.0 ** 24)))


def loss_scale_denoms(gm):
  """the denominators of the automatic-scale sweep at target 16: q = 2^k exactly (denom = gm 2^k / 16, when that is exact in fp32) for k = 0 .. 24, both fp32
  neighbours of each, and five everyday values"""
  out = []
  for k in range(25):
    d = F32(float(gm) * 2.0 ** k / 16.0)
    assert float(d) == float(gm) * 2.0 ** k / 16.0
    out += [float(np.nextafter(d, F32(0))), float(d), float(np.nextafter(d, F32(np.inf)))]
  return out + [1.0, 100.0, 313.0, 4.4e6, 1e12]


# ------------------------------------------------------------------------------------------------ the AdamW guard (include/spa3d.h, spa3d_adamw_step)
class Guard:
  """scratch[2..5] as the header words them: [2] this step skipped, [3] skipped steps, [4] the loss-scale multiplier -- a power of two in [2^-24, 1], anything
  else reads as 1; halved on a skip (floor 2^-24), doubled (up to 1) after 200 finite steps counted in [5]; a skip resets the counter."""

  def __init__(self, mult=0.0, count=0.0, skipped=0.0):
    self.s = [0.0, float(skipped), float(mult), float(count)]   # scratch[2], [3], [4], [5]

  @staticmethod
  def _read(m):
    ok = 2.0 ** -24 <= m <= 1.0 and math.frexp(m)[0] == 0.5
    return m if ok else 1.0

  def step(self, finite):
    m = self._read(self.s[2])
    if not finite:
      self.s[0] = 1.0
      self.s[1] += 1.0
      m = max(m * 0.5, 2.0 ** -24)
      self.s[3] = 0.0
    else:
      self.s[0] = 0.0
      if m < 1.0:
        self.s[3] += 1.0
        if self.s[3] >= 200.0:
          m = min(2.0 * m, 1.0)
          self.s[3] = 0.0
    self.s[2] = m
    return list(self.s)


# ------------------------------------------------------------------------------------------------ AdamW at one call
def adamw_ref(p, g, m, v, step, lr, clip=1.0, wd=0.01, b1=0.9, b2=0.999, eps=1e-8, skipped=0, dtype=np.float64, variant=None):
  """One spa3d_adamw_step in `dtype` -> (p, m, v, norm).  variant 'eps_inside': sqrt(v + eps); 'bias_at_step': bias correction at `step`, not at
  step + 1 - skipped; 'always_clip': the gradient scaled by clip / norm even when norm < clip."""
  p, g, m, v = (np.asarray(x, dtype=dtype) for x in (p, g, m, v))
  gn = math.sqrt(math.fsum((g.astype(np.float64) ** 2).tolist()))
  sc = 1.0 if (gn < clip and variant != 'always_clip') else clip / gn
  t = max(step, 1) if variant == 'bias_at_step' else max(step + 1 - skipped, 1)
  d = dtype
  gi = g * d(sc)
  mn = d(b1) * m + d(1 - b1) * gi
  vn = d(b2) * v + d(1 - b2) * gi * gi
  mh, vh = mn / d(1 - b1 ** t), vn / d(1 - b2 ** t)
  den = np.sqrt(vh + d(eps)) if variant == 'eps_inside' else np.sqrt(vh) + d(eps)
  return p - d(lr) * (mh / den + d(wd) * p), mn, vn, gn


ADAMW_GATES = dict(p=1e-6, m=1e-7, v=1e-9)   # max-abs, the project's (tests/test_gpu_ops.py::test_adamw_step_matches_oracle); the norm 1e-5 relative


def adamw_errs(got, ref):
  """max |got - ref| of (p, m, v)"""
  return tuple(float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))) for a, b in zip(got[:3], ref[:3]))


def adamw_passes(got, ref):
  e = adamw_errs(got, ref)
  return e[0] < ADAMW_GATES['p'] and e[1] < ADAMW_GATES['m'] and e[2] < ADAMW_GATES['v'] and abs(got[3] - ref[3]) <= 1e-5 * ref[3]


def small_state(n, seed):
  """g ~ 1e-9, m ~ 1e-9, v ~ 1e-18: eps = 1e-8 dominates sqrt(v) ~ 1e-9 in the denominator"""
  r = np.random.default_rng(seed)
  return (r.standard_normal(n).astype(F32), (r.standard_normal(n) * 1e-9).astype(F32), (r.standard_normal(n) * 1e-9).astype(F32), (r.random(n) * 1e-18).astype(F32))


def unit_norm_gradient(n):
  """a gradient whose norm is exactly 1 in any order of fp32 summation: 4^k entries of 2^-k (the largest 4^k <= n), spread over the vector, zeros elsewhere.
  Small entries on purpose: v's gate is absolute, and (1 - b2) g^2 carries the fp32 rounding of b2 = 0.999 (1.3e-8 relative to g^2)."""
  k = int(math.log(n, 4))
  g = np.zeros(n, dtype=F32)
  g[np.linspace(0, n - 1, 4 ** k).astype(np.int64)] = F32(2.0 ** -k)
  assert np.count_nonzero(g) == 4 ** k
  return g


# ------------------------------------------------------------------------------------------------ objectives and the Huber boundary
# a - e of tests/test_gpu_loss_config.py: L1, visibility only with beta = 3, Huber with unequal axis weights, the default, everything at once
OBJECTIVES = {
    'a': Obj(l1_weight=1.0, bce_weight=1.0),
    'b': Obj(l1_weight=0.0, bce_weight=1.0, bce_pos_weight=3.0),
    'c': Obj(position_kind=1, huber_delta=1.0, axis_weight=(1.0, 0.5, 0.25)),
    'd': Obj(),
    'e': Obj(l1_weight=1.0, bce_weight=1.0, position_kind=1, huber_delta=1.0, axis_weight=(1.0, 0.5, 0.25), bce_pos_weight=3.0),
}
UNIT_GMAX = Obj(l1_weight=1.0, bce_weight=1.0)   # g_max = 1


def huber_edge():
  """(objective, d): a Huber objective and an error with |d| == delta exactly, where the two branches -- equal in exact arithmetic, the function is continuous --
  round to DIFFERENT fp32 values, so which branch the kernel takes at |d| == delta shows in the bits of a one-point loss.  The header takes the quadratic one
  (|d| <= delta).  The axis weight 2^10 lifts the last bit of rho above the 2^-24 fixed-point unit."""
  for delta in (0.3, 0.7, 0.9, 1.1, 1.3, 1.7, 0.1, 0.6):
    o = Obj(l1_weight=1.0, bce_weight=1.0, position_kind=1, huber_delta=delta, axis_weight=(1024.0, 1.0, 1.0))
    d = np.array([F32(delta)], dtype=F32)
    if float(pos_value(o, d)[0]) != float(pos_value(o, d, 'huber_lt')[0]):
      return o, F32(delta)
  raise AssertionError('no candidate delta separates the two branches in fp32')
