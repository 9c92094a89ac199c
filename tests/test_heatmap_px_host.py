"""The arithmetic of spa3d_render_heatmap (3dspa_code_amd/csrc/heatmap_px.hpp) on the CPU: the header is plain C++ shared by the kernels of
heatmap.hip and this test, so a small driver (tests/host/heatmap_px_check.cpp) is built with the host compiler and computes whole small clips
through it.  map, weight, num, den and the overlay are compared bit for bit with the NumPy restatement of the contract
(tests/heatmap_util.py), and the restatement itself with cases worked out by hand.  No GPU needed."""
import os
import struct
import subprocess

import numpy as np
import pytest

import heatmap_util as HU
import render_util as RU
from util import host_check_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'visualize_golden.npz')


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
  return host_check_driver(tmp_path_factory, 'heatmap_px')


def host_heatmap(driver, tracks, values, H, W, radius, power, visible=None, use_visibility=False, video=None, normalize=True, rng=(0.0, 1.0), alpha=2048, bgr=False,
                 intrinsics=None, extrinsics=None, resize=(1024, 1024)):
  """The driver on one clip: (map, weight, num, den, overlay or None)."""
  N, T, C = tracks.shape
  blob = [struct.pack('<15i2f', N, T, H, W, C, resize[0], resize[1], int(use_visibility), radius, power, int(visible is not None), int(video is not None), int(normalize),
                      alpha, int(bgr), rng[0], rng[1]), np.ascontiguousarray(tracks, np.float32).tobytes()]
  if C == 3:
    blob += [np.ascontiguousarray(np.broadcast_to(intrinsics, (T, 3, 3)), np.float64).tobytes(), np.ascontiguousarray(np.broadcast_to(extrinsics, (T, 4, 4)), np.float64).tobytes()]
  blob.append(np.ascontiguousarray(values, np.float32).tobytes())
  if visible is not None:
    blob.append(np.ascontiguousarray(visible, np.float32).tobytes())
  if video is not None:
    blob.append(np.ascontiguousarray(video, np.uint8).tobytes())
  out = subprocess.run([driver], input=b''.join(blob), capture_output=True, timeout=120)
  assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
  n = T * H * W
  b = out.stdout
  m = np.frombuffer(b[:4 * n], np.float32).reshape(T, H, W)
  w = np.frombuffer(b[4 * n:8 * n], np.float32).reshape(T, H, W)
  num = np.frombuffer(b[8 * n:16 * n], np.float64).reshape(T, H, W)
  den = np.frombuffer(b[16 * n:24 * n], np.uint64).reshape(T, H, W)
  ov = np.frombuffer(b[24 * n:], np.uint8).reshape(T, H, W, 3) if video is not None else None
  return m, w, num, den, ov


def check(driver, tracks, values, H, W, radius, power, **kw):
  """driver == restatement, bit for bit; returns the restatement's (map, weight, overlay, den)"""
  m, w, num, den, ov = host_heatmap(driver, tracks, values, H, W, radius, power, **kw)
  pos = HU.positions(tracks, kw.get('intrinsics'), kw.get('extrinsics'), H, W, kw.get('resize', (1024, 1024)))
  ok = HU.contributes(pos, values, H, W, kw.get('visible'), kw.get('use_visibility', False))
  rnum, rden = HU.sums(pos, ok, values, H, W, radius, power)
  assert np.array_equal(den, rden) and np.array_equal(num.view(np.int64), rnum.view(np.int64))
  want = HU.heatmap(tracks, values, H, W, radius, power, **kw)
  assert HU.same_bits(m, want[0]) and HU.same_bits(w, want[1])
  if kw.get('video') is not None:
    assert np.array_equal(ov, want[2]), f'{int((ov != want[2]).sum())} overlay bytes differ'
  return want


# ---------------------------------------------------------------------------------------------- the restatement against hand cases
def test_restatement_hand_cases():
  H = W = 15
  one = np.array([[[7.0, 7.0]]], np.float32)
  # radius 5: R2 = 25.  Offset (3, 4): d2 = 25, q = 1.  Offset (4, 4): d2 = 32 > 25, nothing.  Centre: q = 26.
  for power in (1, 2):
    m, w, _, den = HU.heatmap(one, np.array([[2.0]], np.float32), H, W, 5, power)
    assert den[0, 7 + 4, 7 + 3] == 1 and den[0, 7 - 3, 7 + 4] == 1 and den[0, 7 + 4, 7 + 4] == 0 and den[0, 7, 7] == 26 ** power
    assert den[0, 7, 7 + 5] == 1 and den[0, 7, 7 + 6] == 0 and den[0, 7 + 1, 7 + 2] == 21 ** power
    inside = den[0] > 0
    assert inside.sum() == 81                                  # the lattice points of a disc of radius 5
    assert (m[0][inside] == 2.0).all() and np.isnan(m[0][~inside]).all() and m[0][~inside].view(np.int32).tolist() == [0x7fc00000] * int((~inside).sum())
    assert np.array_equal(w[0], den[0].astype(np.float32))
  # two points at mirrored offsets from a pixel: equal weights, the mean
  two = np.array([[[4.0, 7.0]], [[10.0, 7.0]]], np.float32)
  m, _, _, den = HU.heatmap(two, np.array([[1.0], [4.0]], np.float32), H, W, 5, 2)
  assert den[0, 7, 7] == 2 * 17 ** 2 and m[0, 7, 7] == 2.5
  assert m[0, 7, 4] == 1.0 and m[0, 7, 10] == 4.0               # 6 apart: neither reaches the other's pixel
  # unequal weights: pixel (6, 7) is 2 from the first (q = 22) and 4 from the second (q = 10)
  assert den[0, 7, 6] == 22 ** 2 + 10 ** 2 and m[0, 7, 6] == np.float32((484 * 1.0 + 100 * 4.0) / 584)
  # overlay: alpha 4096 is the pure colour, alpha 0 the input; lo == hi gives s = m - lo
  video = np.full((1, H, W, 3), 90, np.uint8)
  ov = HU.overlay(video, m, den, 1.0, 4.0, 4096)
  assert tuple(ov[0, 7, 4]) == (255, 0, 0) and tuple(ov[0, 7, 10]) == (0, 0, 255) and tuple(ov[0, 0, 0]) == (90, 90, 90)
  assert tuple(ov[0, 7, 7]) == (255, 255, 255)                  # s = 0.5: white
  assert np.array_equal(HU.overlay(video, m, den, 1.0, 4.0, 0), video)
  ov = HU.overlay(video, m, den, 1.0, 1.0, 2048, bgr=True)      # s = m - 1: 0 at the first point (red, written b g r), 3 -> 1 at the second (blue)
  assert tuple(ov[0, 7, 4]) == ((90 * 2048 + 0 * 2048 + 2048) >> 12, (90 * 2048 + 2048) >> 12, (90 * 2048 + 255 * 2048 + 2048) >> 12)
  assert tuple(ov[0, 7, 10]) == ((90 * 2048 + 255 * 2048 + 2048) >> 12, (90 * 2048 + 2048) >> 12, (90 * 2048 + 2048) >> 12)


def test_restatement_weight_bound_and_order():
  # the largest weight: radius 64, power 2, at the centre: (4096 + 1)^2 < 2^25
  m, w, _, den = HU.heatmap(np.array([[[3.0, 3.0]]], np.float32), np.array([[1.5]], np.float32), 8, 8, 64, 2)
  assert den[0, 3, 3] == 4097 ** 2 < 2 ** 25 and (den[0] > 0).all() and (m[0] == 1.5).all()
  # the order of the additions matters, and reverse=True is the other order
  rng = np.random.default_rng(0)
  tracks = rng.uniform(0, 8, (50, 1, 2)).astype(np.float32)
  values = (rng.choice([-1.0, 1.0], (50, 1)) * 2.0 ** rng.uniform(-20, 20, (50, 1))).astype(np.float32)
  pos = HU.positions(tracks)
  ok = HU.contributes(pos, values, 8, 8)
  a, da = HU.sums(pos, ok, values, 8, 8, 6, 2)
  b, db = HU.sums(pos, ok, values, 8, 8, 6, 2, reverse=True)
  assert np.array_equal(da, db) and (a != b).any()


# ---------------------------------------------------------------------------------------------- the header against the restatement
@pytest.mark.parametrize('radius,power', [(3, 2), (20, 1), (64, 2)])
def test_scene_matches_restatement(driver, radius, power):
  video, tracks, values, visible = RU.scene()   # 37 x 53, T = 7, N = 40
  H, W = video.shape[1:3]
  m, w, ov, den = check(driver, tracks, values, H, W, radius, power, video=video)
  assert (den > 0).any() and (ov != video).any()
  if radius == 64:
    assert (den > 0).all()
  if radius == 3:
    assert (den == 0).any() and np.array_equal(ov[den == 0], video[den == 0])
  # visible is ignored unless asked for
  assert HU.same_bits(check(driver, tracks, values, H, W, radius, power, visible=visible)[0], m)
  v = check(driver, tracks, values, H, W, radius, power, visible=visible, use_visibility=True)
  assert not HU.same_bits(v[0], m)


def test_rim_and_single_point(driver):
  H = W = 15
  one = np.array([[[7.9, 7.2]]], np.float32)                   # truncates to (7, 7)
  for power in (1, 2):
    m, w, _, den = check(driver, one, np.array([[2.0]], np.float32), H, W, 5, power)
    assert den[0, 11, 10] == 1 and den[0, 11, 11] == 0 and (m[0][den[0] > 0] == 2.0).all() and np.isnan(m[0][den[0] == 0]).all()
  two = np.array([[[4.0, 7.0]], [[10.0, 7.0]]], np.float32)
  m, _, _, _ = check(driver, two, np.array([[1.0], [4.0]], np.float32), H, W, 5, 2)
  assert m[0, 7, 7] == 2.5


def test_eligibility(driver):
  H, W, T = 12, 20, 3
  tracks = np.array([[(-0.5, -0.99), (3.9, 2.2), (6.5, 4.0)],          # -0.5 truncates to 0: in bounds
                     [(5.0, 6.0), (float(W), 6.0), (9.0, float(H))],    # x = W, y = H: out of bounds
                     [(2.0, 9.0), (np.inf, 9.0), (np.nan, 9.0)],
                     [(2.0 ** 31, 3.0), (12.0, 3.0), (13.0, -1.0)],
                     [(10.0, 10.0), (10.0, 10.0), (10.0, 10.0)]], np.float32)
  values = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], [np.nan, np.inf, -np.inf]], np.float32)
  visible = np.array([[1, 0, 1], [1, 1, 1], [0.5, 1, 1], [1, 0.51, 1], [1, 1, 1]], np.float32)
  ok = HU.contributes(HU.positions(tracks), values, H, W)
  assert ok.tolist() == [[True, True, True], [True, False, False], [True, False, False], [False, True, False], [False, False, False]]
  video = np.full((T, H, W, 3), 17, np.uint8)
  m, _, _, den = check(driver, tracks, values, H, W, 2, 2, video=video)
  assert den[0, 0, 0] == 25 and m[0, 0, 0] == 1.0 and (den[:, 10, 10] == 0).all()
  okv = HU.contributes(HU.positions(tracks), values, H, W, visible, True)
  assert okv.tolist() == [[True, False, True], [True, False, False], [False, False, False], [False, True, False], [False, False, False]]
  check(driver, tracks, values, H, W, 2, 2, video=video, visible=visible, use_visibility=True)


def test_overlay_options(driver):
  video, tracks, values, _ = RU.scene(T=3, N=20, H=20, W=30, seed=5)
  H, W = 20, 30
  base = check(driver, tracks, values, H, W, 4, 2, video=video)
  for kw in (dict(normalize=False, rng=(0.5, 2.5)), dict(normalize=False, rng=(1.0, 1.0)), dict(bgr=True), dict(alpha=0), dict(alpha=4096), dict(alpha=1),
             dict(normalize=False, rng=(2.0, 1.0))):
    got = check(driver, tracks, values, H, W, 4, 2, video=video, **kw)
    assert HU.same_bits(got[0], base[0])
    if kw.get('alpha') == 0:
      assert np.array_equal(got[2], video)
  weird = values.copy()
  weird[0, 1], weird[1, 2], weird[2, 0], weird[6] = np.nan, np.inf, -np.inf, np.nan
  check(driver, tracks, weird, H, W, 4, 2, video=video)
  allnan = np.full_like(values, np.nan)
  m, _, ov, _ = check(driver, tracks, allnan, H, W, 4, 2, video=video)
  assert np.isnan(m).all() and np.array_equal(ov, video)
  const = np.full_like(values, 0.75)                                   # max == min: s = m - lo = 0, red
  m, _, ov, den = check(driver, tracks, const, H, W, 4, 2, video=video, alpha=4096)
  assert (m[den > 0] == 0.75).all() and (ov[den > 0] == (255, 0, 0)).all()


def test_projected_points_of_the_golden_cameras(driver):
  g = dict(np.load(GOLDEN))
  H, W = (int(v) for v in g['hw'])
  for name in ('frames', 'single'):
    K, E, rs = g['intrinsics_' + name], g['extrinsics_' + name], tuple(int(v) for v in g['resize_' + name])
    pos = HU.positions(g['tracks'], K, E, H, W, rs)
    assert np.array_equal(pos, g['pixels_' + name])                     # the reference's int() of its own projection
    check(driver, g['tracks'], g['scores'], H, W, 6, 2, video=g['video'], intrinsics=K, extrinsics=E, resize=rs)
