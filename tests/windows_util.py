"""NumPy float32 restatement of the window plan, the blend weights and the stitch of spa3d_stitch_windows (include/spa3d.h), for the tests of
csrc/window_row.hpp and of the kernel.  The same operation order as the header: contributions in increasing window number, the first one
starts num = float(wgt) * v and den = float(wgt), later ones add; one division; a frame under one window, and the 'first' blend, copy the
lowest-numbered window's value.  Every array operation below is float32 (NumPy keeps float32 op float32 in float32)."""
import numpy as np

MEAN, HAT, FIRST = 0, 1, 2
BLEND = {'mean': MEAN, 'hat': HAT, 'first': FIRST}


def window_starts(num_frames, window, stride=None):
  stride = max(window // 2, 1) if stride is None else stride
  assert 1 <= stride <= window
  if num_frames <= window:
    return np.array([0], np.int32)
  W = 1 + (num_frames - window + stride - 1) // stride
  return np.array([w * stride for w in range(W - 1)] + [num_frames - window], np.int32)


def window_lengths(t0, Tw, TL):
  return np.minimum(Tw, TL - np.asarray(t0, np.int64)).astype(np.int32)


def weights(blend, L):
  j = np.arange(L)
  return (np.minimum(j + 1, L - j) if blend == HAT else np.ones(L)).astype(np.float32)


def coverage(t0, ln, TL):
  c = np.zeros(TL, np.int64)
  for a, l in zip(t0, ln):
    c[a:a + l] += 1
  return c


def stitch(src, t0, ln, TL, blend, row_track=None, want_spread=False):
  """src [W,N,Tw] or [W,N,Tw,NC] float32 -> blended [N,TL(,NC)] (and spread^2 [N,TL], BEFORE the square root, when asked; src must then have NC)."""
  src = np.asarray(src, np.float32)
  flat = src.ndim == 3
  if flat:
    src = src[..., None]
  W, N, Tw, NC = src.shape
  num, den, first = np.zeros((N, TL, NC), np.float32), np.zeros((TL,), np.float32), np.zeros((N, TL, NC), np.float32)
  cnt = np.zeros(TL, np.int64)
  for w in range(W):
    a, L = int(t0[w]), int(ln[w])
    v, wg = src[w, :, :L], weights(blend, L)
    fresh = cnt[a:a + L] == 0
    wv = wg[None, :, None] * v
    num[:, a:a + L] = np.where(fresh[None, :, None], wv, num[:, a:a + L] + wv)
    den[a:a + L] = np.where(fresh, wg, den[a:a + L] + wg)
    first[:, a:a + L] = np.where(fresh[None, :, None], v, first[:, a:a + L])
    cnt[a:a + L] += 1
  assert (cnt >= 1).all(), 'a gap in the plan'
  with np.errstate(invalid='ignore', divide='ignore'):
    blended = num / den[None, :, None]
  copy = (cnt <= 1) | (blend == FIRST)
  out = np.where(copy[None, :, None], first, blended).astype(np.float32)
  s2 = None
  if want_spread:
    s2 = np.zeros((N, TL), np.float32)
    for w in range(W):
      a, L = int(t0[w]), int(ln[w])
      with np.errstate(invalid='ignore', over='ignore'):
        d = src[w, :, :L] - out[:, a:a + L]
        d2 = d[..., 0] * d[..., 0]
        for c in range(1, NC):
          d2 = d2 + d[..., c] * d[..., c]
        m = s2[:, a:a + L]
        take = ((d2 > m) | (d2 != d2)) & (cnt[a:a + L] > 1)[None, :]
      s2[:, a:a + L] = np.where(take, d2, m)
  if row_track is not None:
    rt = np.asarray(row_track)
    o2 = np.empty_like(out)
    o2[rt] = out
    out = o2
    if s2 is not None:
      z = np.empty_like(s2)
      z[rt] = s2
      s2 = z
  if flat:
    out = out[..., 0]
  return (out, s2) if want_spread else out


def same_bits_or_both_nan(a, b):
  """elementwise: equal bit patterns, or both NaN (a blend that touches a NaN gives a NaN whose payload is the hardware's choice)"""
  a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
  return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))


def ulp_diff(a, b):
  """distance in float32 steps between two non-negative finite arrays"""
  a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
  return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
