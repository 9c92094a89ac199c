"""NumPy restatement of spa3d_render_tracks, written from the contract in include/spa3d.h (not from csrc/render_px.hpp): float64 for the
projection and the colour, float32 for the normalisation, Python / int64 integers for coverage and blend.  Every output byte is defined by the
contract, so the tests compare with equality.  Also the scene generators the host and GPU tests share."""
import numpy as np

NO_POS = -2 ** 31


def project(tracks, intrinsics, extrinsics, H, W, resize=(1024, 1024)):
  """tracks [N, T, 3] float32; intrinsics [T, 3, 3], extrinsics [T, 4, 4] float64 -> int32 [N, T, 2]."""
  N, T, _ = tracks.shape
  sx, sy = resize[1] / W, resize[0] / H
  out = np.zeros((N, T, 2), np.int32)
  p = tracks.astype(np.float64)
  with np.errstate(all='ignore'):
    for t in range(T):
      K = np.array(intrinsics[t], np.float64)
      E = np.asarray(extrinsics[t], np.float64)
      K[0, 0] *= sx; K[0, 2] *= sx; K[1, 1] *= sy; K[1, 2] *= sy
      x, y, z = p[:, t, 0], p[:, t, 1], p[:, t, 2]
      c = [((E[r, 0] * x + E[r, 1] * y) + E[r, 2] * z) + E[r, 3] for r in range(3)]
      h = [(K[r, 0] * c[0] + K[r, 1] * c[1]) + K[r, 2] * c[2] for r in range(3)]
      u, v = h[0] / (h[2] + 1e-8), h[1] / (h[2] + 1e-8)
      u = np.where(np.isfinite(u), u, 0.0) / sx
      v = np.where(np.isfinite(v), v, 0.0) / sy
      out[:, t, 0] = np.trunc(np.clip(u, 0, W - 1)).astype(np.int32)
      out[:, t, 1] = np.trunc(np.clip(v, 0, H - 1)).astype(np.int32)
  return out


def pixels_2d(tracks):
  """[N, T, 2] float32 pixel coordinates -> int32 [N, T, 2]; NO_POS where a coordinate is not finite or beyond 2^30."""
  t = tracks.astype(np.float32)
  with np.errstate(invalid='ignore'):
    ok = (np.abs(t) <= np.float32(2.0 ** 30)).all(-1)
  pos = np.trunc(np.where(ok[..., None], t, 0)).astype(np.int64)
  return np.where(ok[..., None], pos, NO_POS).astype(np.int32)


def colour_bgr(s1):
  """score_to_color_bgr in double."""
  q = min(max(float(s1), 0.0), 1.0)
  if q < 0.5:
    ratio = q / 0.5
    return int(255 * ratio), int(255 * ratio), 255
  ratio = (q - 0.5) / 0.5
  return 255, int(255 * (1 - ratio)), int(255 * (1 - ratio))


def colours(scores, normalize=True, bgr=False):
  """scores [N, T] float32 -> (bytes [N, T, 3] uint8 in writing order, ok [N, T] bool)."""
  s = np.asarray(scores, np.float32)
  fin = np.isfinite(s)
  with np.errstate(all='ignore'):
    if normalize and fin.any():
      mn, mx = s[fin].min(), s[fin].max()
      s1 = (s - mn) / (mx - mn) if mx > mn else s - mn
    else:
      s1 = s.copy()
    s1 = s1.astype(np.float32)
  ok = fin & np.isfinite(s1)
  col = np.zeros(s.shape + (3,), np.uint8)
  for idx in zip(*np.nonzero(ok)):
    b, g, r = colour_bgr(s1[idx])
    col[idx] = (b, g, r) if bgr else (r, g, b)
  return col, ok


_SA, _SB = np.meshgrid(np.arange(4, dtype=np.int64), np.arange(4, dtype=np.int64))  # sample offsets (a, b)


def _samples(xs, ys):
  """sample coordinates of the pixels xs x ys: int64 arrays [len(ys), len(xs), 4, 4] for x and y."""
  px = 8 * xs[None, :, None, None] + 2 * _SA[None, None] + 1
  py = 8 * ys[:, None, None, None] + 2 * _SB[None, None] + 1
  return np.broadcast_arrays(px, py)


def cover_dot(xs, ys, cx, cy, r):
  px, py = _samples(xs, ys)
  dx, dy = px - (8 * cx + 4), py - (8 * cy + 4)
  return (dx * dx + dy * dy <= (8 * r + 4) ** 2).sum((-1, -2))


def cover_seg(xs, ys, ax, ay, bx, by):
  px, py = _samples(xs, ys)
  px, py = px - (8 * ax + 4), py - (8 * ay + 4)
  dx, dy = 8 * (bx - ax), 8 * (by - ay)
  L2 = dx * dx + dy * dy
  u = px * dx + py * dy
  c = px * dy - py * dx
  near_a = px * px + py * py <= 16
  near_b = (px - dx) ** 2 + (py - dy) ** 2 <= 16
  body = (np.abs(c) <= 4 * (abs(dx) + abs(dy))) & (c * c <= 16 * L2)
  inside = np.where((u < 0) | (L2 == 0), near_a, np.where(u > L2, near_b, body))
  return inside.sum((-1, -2))


def _blend(frame, xs, ys, k, alpha, col):
  w = (k * alpha)[..., None].astype(np.int64)
  reg = frame[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1].astype(np.int64)
  new = (reg * (4096 - w) + np.asarray(col, np.int64)[None, None] * w + 2048) >> 12
  frame[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = np.where(w > 0, new, reg).astype(np.uint8)


def render(video, pos, scores, visible=None, trail=5, point_size=2, normalize=True, use_visibility=False, colour_bgr=False, only=None):
  """video uint8 [T, H, W, 3]; pos int32 [N, T, 2] (NO_POS: none); scores [N, T]; visible [N, T] or None.  Returns the painted copy.
  only: an optional window (t, y0, y1, x0, x1, H, W), bounds inclusive, of an H x W clip -- then video is just that window
  [y1 - y0 + 1, x1 - x0 + 1, 3] of frame t (how the 16384 x 16384 case is checked without its frames)."""
  N, T = pos.shape[:2]
  col, col_ok = colours(scores, normalize, colour_bgr)
  out = video.copy()
  if only is None:
    H, W = video.shape[1:3]
    frames = range(T)
  else:
    frames = [only[0]]
    H, W = only[5], only[6]
  p = pos.astype(np.int64)
  inb = (p[..., 0] >= 0) & (p[..., 0] < W) & (p[..., 1] >= 0) & (p[..., 1] < H) & (pos[..., 0] != NO_POS)
  end_ok = inb & ((np.asarray(visible, np.float32) > 0.5) if use_visibility else True)

  def paint(t, x_lo, x_hi, y_lo, y_hi, fn, alpha, c):
    """blend coverage fn over the pixel box, cut to the image (and to the window)"""
    wx0, wy0, wx1, wy1 = (0, 0, W - 1, H - 1) if only is None else (only[3], only[1], only[4], only[2])
    x_lo, x_hi, y_lo, y_hi = max(x_lo, wx0), min(x_hi, wx1), max(y_lo, wy0), min(y_hi, wy1)
    if x_lo > x_hi or y_lo > y_hi:
      return
    xs, ys = np.arange(x_lo, x_hi + 1, dtype=np.int64), np.arange(y_lo, y_hi + 1, dtype=np.int64)
    k = fn(xs, ys)
    frame = out[t] if only is None else out
    _blend(frame, xs - wx0, ys - wy0, k, alpha, c)

  for t in frames:
    for i in range(N):
      if not col_ok[i, t]:
        continue
      c = col[i, t]
      for q in range(max(0, t - trail), t):
        if end_ok[i, q] and end_ok[i, q + 1]:
          ax, ay, bx, by = (int(v) for v in (*p[i, q], *p[i, q + 1]))
          paint(t, min(ax, bx) - 2, max(ax, bx) + 2, min(ay, by) - 2, max(ay, by) + 2, lambda xs, ys: cover_seg(xs, ys, ax, ay, bx, by), 179, c)
      if end_ok[i, t]:
        cx, cy = int(p[i, t, 0]), int(p[i, t, 1])
        r = point_size
        paint(t, cx - r - 2, cx + r + 2, cy - r - 2, cy + r + 2, lambda xs, ys: cover_dot(xs, ys, cx, cy, r), 256, c)
  return out


# ---------------------------------------------------------------------------------------------- scenes
def scene(T=7, N=40, H=37, W=53, seed=0):
  """2-D scene: random-walk tracks, some crossing the 64 x 16 tile borders, one jumping across the image in one frame, some leaving the image,
  one with a NaN coordinate.  Returns video, tracks [N, T, 2] float32, scores [N, T] float32, visible [N, T] float32."""
  rng = np.random.default_rng(seed)
  video = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
  start = rng.uniform([0, 0], [W, H], (N, 1, 2))
  tracks = (start + np.cumsum(rng.normal(0, 2.5, (N, T, 2)), 1)).astype(np.float32)
  tracks[0, :, 1] = np.linspace(13.2, 18.9, T)   # walks across the border between tile rows 0 and 1 (y = 16)
  tracks[1, :, 0] = np.linspace(3.5, W - 2.5, T)   # sweeps the width
  tracks[2, T // 2:] = (W - 1.5, H - 1.5) - tracks[2, T // 2:]   # jumps across the image in one frame
  tracks[3, :, 0] += W   # outside: nothing drawn
  tracks[4, 1, 0] = np.nan
  tracks[5, :] = (10.7, 11.2)   # stands still: zero-length segments
  scores = rng.uniform(0, 3, (N, T)).astype(np.float32)
  visible = (rng.uniform(0, 1, (N, T)) > 0.3).astype(np.float32)
  return video, tracks, scores, visible
