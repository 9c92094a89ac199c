"""TAPVid-3D metric arithmetic (3dspa_code_amd/csrc/tapvid3d_row.hpp) on the CPU: the header is plain C++ shared by the kernels of tapvid3d.hip
and this test, so a small driver (tests/host/tapvid3d_row_check.cpp) is built with the host compiler.  Its rows on the generator's clips --
(3, 37, 70) and (2, 9, 150), the three scalings, depth-dependent and fixed thresholds, default and explicit intrinsics -- are compared with the
NumPy float64 restatement in tests/tapvid3d_util.py under the rules stated there, and its median select is compared bit for bit with NumPy's
on the cases a radix select can get wrong.  No GPU needed."""
import struct
import subprocess

import numpy as np
import pytest

import tapvid3d_util as TU
from util import host_check_driver


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
  return host_check_driver(tmp_path_factory, 'tapvid3d_row')


def host_rows(driver, d, b, scaling, s, intr, fixed):
  """Sample b of generator data through the host rows: stats [Q, 24], scale used [Q], ratio [Q, T]."""
  Q, T = d['l'].shape[1:]
  fx, fy = (256.0, 256.0) if intr is None else (float(intr[0]), float(intr[1]))
  blob = [struct.pack('<iiiii', 0, Q, T, TU.SCALINGS[scaling], int(fixed))]
  for q in range(Q):
    blob += [struct.pack('<ffff', float(d['qp'][b, q, 0]), float(s), fx, fy), d['p'][b, q].tobytes(), d['l'][b, q].tobytes(), d['g'][b, q].tobytes(), d['y'][b, q].tobytes()]
  out = subprocess.run([driver], input=b''.join(blob), capture_output=True, timeout=120)
  assert out.returncode == 0, out.stderr[-2000:]
  a = np.frombuffer(out.stdout, np.float32).reshape(Q, TU.S + 1 + T)
  return a[:, :TU.S], a[:, TU.S], a[:, TU.S + 1:]


def host_median(driver, sets):
  blob = [struct.pack('<ii', 1, len(sets))]
  for x in sets:
    x = np.ascontiguousarray(x, np.float32)
    blob += [struct.pack('<q', x.size), x.tobytes()]
  out = subprocess.run([driver], input=b''.join(blob), capture_output=True, timeout=120)
  assert out.returncode == 0, out.stderr[-2000:]
  return np.frombuffer(out.stdout, np.float32)


@pytest.mark.parametrize('shape', [(3, 37, 70), (2, 9, 150)])
@pytest.mark.parametrize('scaling', ['none', 'median', 'per_trajectory'])
def test_rows_match_float64_restatement(driver, shape, scaling):
  B, Q, T = shape
  d = TU.generate(B, Q, T)
  intr = np.array([[300.0, 280.0, 160.0, 120.0], [200.0, 210.0, 100.0, 100.0], [256.0, 256.0, 128.0, 128.0]], np.float32)
  for fixed, k in ((False, None), (False, intr), (True, None)):
    out = dict(query_stats=np.zeros((B, Q, TU.S), np.float32), sample_stats=np.zeros((B, TU.S)), scale=np.ones(B, np.float32),
               row_scale=np.zeros((B, Q), np.float32), ratio=np.zeros((B, Q, T), np.float32))
    for b in range(B):
      ki = None if k is None else k[b]
      _, _, ratio = host_rows(driver, d, b, 'none', 1.0, ki, fixed)
      s = 1.0
      if scaling == 'median':  # the sample's factor: the header's select over the set the ratio pass marks
        tq = TU.query_frame(d['qp'][b], T)
        sel = np.where((d['y'][b] > 0.5) & (np.arange(T)[None, :] != tq[:, None]), ratio, np.float32(np.nan))
        s = host_median(driver, [sel])[0]
        out['scale'][b] = s
      out['query_stats'][b], out['row_scale'][b], out['ratio'][b] = host_rows(driver, d, b, scaling, s, ki, fixed)
      out['sample_stats'][b] = out['query_stats'][b].astype(np.float64).sum(0)
    TU.check_call(d, out, scaling, k, fixed, what=f'host {shape} {scaling} fixed={fixed} intrinsics={"given" if k is not None else "default"}')
    if scaling == 'median':  # the generator's factors come back
      assert np.allclose(out['scale'], d['s_b'], rtol=0.02), out['scale']
    w = out['sample_stats'][:, 4::4] / out['sample_stats'][:, 1:2]
    if not fixed and scaling == 'median':  # every threshold cuts the data: the generator aims at 0.25 / 0.38 / 0.50 / 0.63 / 0.75
      assert (np.diff(w, axis=1) > 0.05).all() and 0.15 < w[:, 0].min() and w[:, 4].max() < 0.85, w
    if not fixed and scaling == 'per_trajectory':  # a row's factor carries its query frame's error, so fewer points fall within; still no vacuous threshold
      assert (np.diff(w, axis=1) > 0).all() and 0 < w[:, 0].min() and w[:, 4].max() < 1, w
    if not fixed and scaling == 'none':  # sample 0 is the one the generator left unscaled: there `none` cuts as the median does
      assert (np.diff(w[0]) > 0.05).all() and 0.15 < w[0, 0] and w[0, 4] < 0.85, w


def test_query_frame_is_left_out_and_clamped(driver):
  d = TU.generate(1, 4, 20, seed=11)
  d['qp'][0, :, 0] = [-3.0, 2.5, 3.5, 100.0]  # clamped to 0; ties to even: 2 and 4; clamped to T - 1
  stats, _, _ = host_rows(driver, d, 0, 'none', 1.0, None, False)
  ref = TU.reference(d['p'][0], d['l'][0], d['g'][0], d['y'][0], d['qp'][0], np.ones(4))
  assert ref['tq'].tolist() == [0, 2, 4, 19]
  TU.check_rows(stats, ref, 'query frames')
  assert (stats[:, 0] == 19).all()


def test_host_select_is_the_exact_median(driver):
  cases = TU.median_cases()
  got = host_median(driver, list(cases.values()))
  for (name, x), m in zip(cases.items(), got):
    want = TU.median32(x)
    assert m.tobytes() == np.float32(want).tobytes(), f'{name}: select gave {m!r}, the fp32 median is {want!r}'
    v = x[~np.isnan(x)]
    if v.size % 2 == 1:
      assert m == np.float32(np.median(v)), name
    elif v.size:
      assert abs(float(m) - float(np.median(v.astype(np.float64)))) <= 2.0 ** -23 * float(np.median(v.astype(np.float64))) + 1e-45, name
