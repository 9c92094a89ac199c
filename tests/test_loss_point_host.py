"""csrc/loss_point.hpp -- the per-point arithmetic of the configurable training objective, the code the three loss kernels run -- compiled
with the host compiler (tests/host/loss_point_check.cpp) and compared with float64 closed forms and with central differences taken in double.

Bound: 4 ulp of fp32.  For a value and for a derivative computed without a subtraction the ulp is the fp32 spacing at the float64 result (the
subnormal spacing 2^-149 at least).  The visibility derivative at y = 1 is sigmoid(l) - 1 (x beta): a difference of two numbers of size 1,
which the default objective must keep evaluating exactly as it always has (bit-equal defaults), so its error is that of its operands and is
measured in the spacing at 1 (2^-23) -- at l = 20 the fp32 sigmoid is exactly 1 and the difference 0 where the true value is -2.1e-9, 0.02 of
that spacing.  Measured figures: profiles/r12_loss_config.log."""
import struct
import subprocess

import numpy as np
import pytest

from util import host_check_driver

ULPS = 4.0
L1, HUBER = 0, 1
DELTAS = (1.0, 0.25, 3.0)
LOGITS = (0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0)
BETAS = (1.0, 3.0)


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
  return host_check_driver(tmp_path_factory, 'loss_point')


def _run(driver, pos, vis):
  blob = struct.pack('<i', len(pos)) + b''.join(struct.pack('<iff', k, dl, d) for k, dl, d in pos)
  blob += struct.pack('<i', len(vis)) + b''.join(struct.pack('<fff', b, y, l) for b, y, l in vis)
  out = subprocess.run([driver], input=blob, capture_output=True, timeout=60)
  assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
  a = np.frombuffer(out.stdout, np.float32)
  n, m = len(pos), len(vis)
  assert a.size == 2 * n + 3 * m
  return a[:n], a[n:2 * n], a[2 * n:2 * n + m], a[2 * n + m:2 * n + 2 * m], a[2 * n + 2 * m:]


def _spacing(ref):
  """fp32 spacing at |ref| (float64 array): 2^(floor(log2 |ref|) - 23), at least the subnormal spacing."""
  a = np.maximum(np.abs(ref), 2.0 ** -126)
  return np.maximum(2.0 ** (np.floor(np.log2(a)) - 23), 2.0 ** -149)


def _ulps(got, ref, at=None):
  return np.abs(got.astype(np.float64) - ref) / _spacing(ref if at is None else at)


def _pos_points():
  f = np.float32
  pts = []
  for kind in (L1, HUBER):
    for delta in DELTAS:
      dl = f(delta)
      ds = [f(0), dl, dl * f(1 + 2.0 ** -20), dl * f(1 - 2.0 ** -20), f(1e-6), f(50)]
      for d in ds:
        for s in (1, -1):
          pts.append((kind, float(dl), float(f(s) * d)))
  return pts


def _rho64(kind, delta, d):
  a = abs(d)
  if kind == HUBER:
    return d * d / (2 * delta) if a <= delta else a - delta / 2
  return a


def _drho64(kind, delta, d):
  if kind == HUBER and abs(d) <= delta:
    return d / delta
  return float(np.sign(d))


def _logsig64(x):
  return min(x, 0.0) - np.log1p(np.exp(-abs(x)))


def _v64(beta, y, l):
  return -beta * y * _logsig64(l) - (1 - y) * _logsig64(-l)


def _dv64(beta, y, l):
  # sigmoid(l) - 1 = -sigmoid(-l): no cancellation in the reference
  sig = lambda x: 1.0 / (1.0 + np.exp(-x)) if x >= 0 else np.exp(x) / (1.0 + np.exp(x))
  return -beta * y * sig(-l) + (1 - y) * sig(l)


def test_position_term_values_derivatives_and_identities(driver):
  pts = _pos_points()
  rho, drho, _, _, _ = _run(driver, pts, [])
  ref = np.array([_rho64(*p) for p in pts])
  dref = np.array([_drho64(*p) for p in pts])
  u, du = _ulps(rho, ref), _ulps(drho, dref)
  print(f'position term: worst value error {u.max():.3f} ulp, worst derivative error {du.max():.3f} ulp over {len(pts)} points')
  assert u.max() <= ULPS and du.max() <= ULPS
  # central differences of the float64 closed form: h = 1e-7 stays on one side of every kink but d = +-delta itself, where the value is C1 and the
  # difference quotient is off by h / (4 delta) <= 1e-7; roundoff 1e-16 / h = 1e-9; plus the 4 ulp of the fp32 derivative
  h = 1e-7
  cd = np.array([(_rho64(k, dl, d + h) - _rho64(k, dl, d - h)) / (2 * h) for k, dl, d in pts])
  err = np.abs(drho.astype(np.float64) - cd)
  print(f'position term: worst |derivative - central difference| {err.max():.3e}')
  assert err.max() <= 1e-7 + 1e-9 + ULPS * 2.0 ** -23
  f = np.float32
  for i, (k, dl, d) in enumerate(pts):
    j = i + 1 if i % 2 == 0 else i - 1   # the point's mirror image
    assert drho[i] == -drho[j], 'rho\' is odd'
    assert rho[i] == rho[j]
    if d == 0:
      assert rho[i] == 0 and drho[i] == 0
    if k == HUBER and abs(d) > dl:
      assert rho[i] == f(abs(f(d))) - f(dl) / f(2), 'Huber is |d| - delta / 2 beyond delta, exactly'
      assert abs(drho[i]) == 1
    if k == L1:
      assert rho[i] == abs(f(d))


def test_visibility_term_values_and_derivatives(driver):
  pts = [(b, y, l) for b in BETAS for y in (0.0, 1.0) for l in LOGITS]
  _, _, v, dv, ls = _run(driver, [], pts)
  ref = np.array([_v64(*p) for p in pts])
  dref = np.array([_dv64(*p) for p in pts])
  lref = np.array([_logsig64(p[2]) for p in pts])
  ul, uv = _ulps(ls, lref), _ulps(v, ref)
  y1 = np.array([p[1] == 1.0 for p in pts])
  # y = 0: v' = sigmoid(l), no subtraction: spacing at the result.  y = 1: sigmoid(l) - 1, operands of size 1: spacing at max(|result|, 1)
  ud = np.where(y1, _ulps(dv, dref, np.maximum(np.abs(dref), 1.0)), _ulps(dv, dref))
  for name, u in (('log_sigmoid', ul), ('visibility value', uv), ('visibility derivative', ud)):
    w = int(u.argmax())
    print(f'{name}: worst error {u.max():.3f} ulp at (beta, y, l) = {pts[w]}')
  big = np.array([abs(p[2]) == 88.0 for p in pts])
  print(f'log_sigmoid at |l| = 88: {ul[big].max():.3f} ulp; visibility value there: {uv[big].max():.3f} ulp')
  assert ul.max() <= ULPS and uv.max() <= ULPS and ud.max() <= ULPS
  rel1 = np.abs(dv.astype(np.float64) - dref)[y1] / np.abs(dref[y1])
  print(f'visibility derivative at y = 1, relative to its own size: worst {rel1.max():.3e} (the legacy sigmoid(l) - y expression loses it for l >= 17)')
  # central differences of the float64 closed form, h = 1e-6: truncation h^2 |v\'\'\'| / 6 < 1e-12 (|v\'\'\'| <= beta / 6 sqrt 3), roundoff 88 * 1e-16 / h = 1e-8
  h = 1e-6
  cd = np.array([(_v64(b, y, l + h) - _v64(b, y, l - h)) / (2 * h) for b, y, l in pts])
  err = np.abs(dv.astype(np.float64) - cd)
  print(f'visibility term: worst |derivative - central difference| {err.max():.3e}')
  assert err.max() <= 2e-8 + 3 * ULPS * 2.0 ** -23   # 3 = the largest beta: the derivative's range is [-beta, 1]
