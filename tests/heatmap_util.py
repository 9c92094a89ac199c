"""NumPy restatement of spa3d_render_heatmap, written from the contract in include/spa3d.h (not from csrc/heatmap_px.hpp): a loop over the
points in index order, vectorised over the pixels of a frame -- uint64 for the weights and their sum, float64 for the weighted sum, the division
and the scaling, float32 only where the contract rounds to it.  Every output bit is defined by the contract, so the tests compare with equality
(float outputs by their int32 view: NaN positions count).  Positions, colours and the scene come from tests/render_util.py."""
import numpy as np

import render_util as RU


def positions(tracks, intrinsics=None, extrinsics=None, H=None, W=None, resize=(1024, 1024)):
  """int32 [N, T, 2] (NO_POS: none) of [N, T, 2] pixel coordinates or of [N, T, 3] points with their cameras."""
  if tracks.shape[-1] == 2:
    return RU.pixels_2d(tracks)
  T = tracks.shape[1]
  return RU.project(tracks, np.broadcast_to(intrinsics, (T, 3, 3)), np.broadcast_to(extrinsics, (T, 4, 4)), H, W, resize)


def contributes(pos, values, H, W, visible=None, use_visibility=False):
  """bool [N, T]: the position exists and is in bounds, the value is finite and, when asked for, the point is visible."""
  p = pos.astype(np.int64)
  ok = (pos[..., 0] != RU.NO_POS) & (p[..., 0] >= 0) & (p[..., 0] < W) & (p[..., 1] >= 0) & (p[..., 1] < H) & np.isfinite(np.asarray(values, np.float32))
  if use_visibility:
    ok &= np.asarray(visible, np.float32) > np.float32(0.5)
  return ok


def sums(pos, ok, values, H, W, radius, power, reverse=False):
  """(num float64 [T, H, W], den uint64 [T, H, W]): the points in increasing index order (reverse: decreasing -- NOT the contract, for the
  test that shows the order matters)."""
  N, T = ok.shape
  R2 = radius * radius
  num, den = np.zeros((T, H, W), np.float64), np.zeros((T, H, W), np.uint64)
  ys, xs = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
  order = range(N - 1, -1, -1) if reverse else range(N)
  for t in range(T):
    for i in order:
      if not ok[i, t]:
        continue
      x, y = int(pos[i, t, 0]), int(pos[i, t, 1])
      y0, y1, x0, x1 = max(0, y - radius), min(H, y + radius + 1), max(0, x - radius), min(W, x + radius + 1)
      d2 = (xs[:, x0:x1] - x) ** 2 + (ys[y0:y1] - y) ** 2
      reach = d2 <= R2
      q = np.where(reach, R2 + 1 - d2, 0)
      w = (q * q if power == 2 else q).astype(np.uint64)
      den[t, y0:y1, x0:x1] += w
      add = num[t, y0:y1, x0:x1] + w.astype(np.float64) * np.float64(np.float32(values[i, t]))
      num[t, y0:y1, x0:x1] = np.where(reach, add, num[t, y0:y1, x0:x1])
  return num, den


def finish(num, den):
  """(map float32, weight float32) of the sums"""
  with np.errstate(all='ignore'):
    m = np.where(den > 0, (num / den.astype(np.float64)).astype(np.float32), np.float32(np.nan)).astype(np.float32)
  return m, den.astype(np.float32)


def value_range(values):
  """(lo, hi) float32 over the finite values; (inf, -inf) when there is none"""
  v = np.asarray(values, np.float32)
  fin = v[np.isfinite(v)]
  return (fin.min(), fin.max()) if fin.size else (np.float32(np.inf), np.float32(-np.inf))


def overlay(video, m, den, lo, hi, alpha, bgr=False):
  """video uint8 [T, H, W, 3], m float32 / den uint64 [T, H, W], alpha 0..4096 -> the blended copy"""
  dm, lo, hi = m.astype(np.float64), np.float64(np.float32(lo)), np.float64(np.float32(hi))
  with np.errstate(all='ignore'):
    s1 = ((dm - lo) / (hi - lo) if hi > lo else dm - lo).astype(np.float32)
    ok = (den > 0) & np.isfinite(s1)
    q = np.clip(np.where(ok, s1, 0).astype(np.float64), 0.0, 1.0)
  low = q < 0.5
  up = np.trunc(255 * (q / 0.5)).astype(np.int64)                  # q < 0.5: (b, g, r) = (up, up, 255)
  dn = np.trunc(255 * (1 - (q - 0.5) / 0.5)).astype(np.int64)      # else:     (b, g, r) = (255, dn, dn)
  b, g, r = np.where(low, up, 255), np.where(low, up, dn), np.where(low, 255, dn)
  col = np.stack([b, g, r] if bgr else [r, g, b], -1)
  new = (video.astype(np.int64) * (4096 - alpha) + col * alpha + 2048) >> 12
  return np.where(ok[..., None], new, video).astype(np.uint8)


def heatmap(tracks, values, H, W, radius, power, visible=None, use_visibility=False, video=None, normalize=True, rng=None, alpha=2048, bgr=False,
            intrinsics=None, extrinsics=None, resize=(1024, 1024)):
  """The whole call: (map, weight, overlay or None, den).  rng = (lo, hi) is read with normalize False."""
  pos = positions(tracks, intrinsics, extrinsics, H, W, resize)
  ok = contributes(pos, values, H, W, visible, use_visibility)
  num, den = sums(pos, ok, values, H, W, radius, power)
  m, w = finish(num, den)
  out = None
  if video is not None:
    lo, hi = value_range(values) if normalize else rng
    out = overlay(video, m, den, lo, hi, alpha, bgr)
  return m, w, out, den


def same_bits(a, b):
  """float32 arrays equal bit for bit"""
  a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
  return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
