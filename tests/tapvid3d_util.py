"""Helpers of the TAPVid-3D metric tests (tests/test_tapvid3d_row_host.py, tests/test_gpu_tapvid3d.py): a seeded generator of clips, a NumPy
float64 restatement of the definitions in include/spa3d.h (spa3d_tapvid3d) and the comparison rules.  tapnet is not vendored upstream and
is not a dependency here: the header's definitions are the contract (restated from the published definition, parity unpinned).

Rules (each derived from the number formats, not from what the code gives):
  * slots 0-3 (evaluated frames, visible, occlusion-correct, predicted visible) are exact, and so are TP + FN == slot 1, TP + FP == slot 3;
  * ratio is within relative 2^-21 of float64: two square roots of three-term sums and one division, at most 6 * 2^-24;
  * scale equals, bit for bit, the fp32 median of the ratios the call returned over {vis and ew} of the sample's live rows (the middle value,
    or np.float32(0.5) * a + np.float32(0.5) * b); row_scale equals ratio[q][tq] (per_trajectory) or the sample's scale;
  * threshold counts are compared with the reference evaluated AT THE SCALE THE CALL RETURNED, leaving out the (frame, threshold) pairs with
    |e2 - thr| <= 2^-21 (|ps| + |g|) + 1e-6 thr: the fp32 product p * s, the differences, the squares and the root are each a few 2^-24 of
    |ps| + |g|, and at the 1-px threshold thr is about |g| / 256, so those roundings are already 1e-5 of the threshold.  A count must lie
    between "all such pairs outside" and "all such pairs within".  At most 0.1 % of the pairs may be left out;
  * sample_stats equal the float64 sum of the sample's rows exactly (integers far below 2^53)."""
import numpy as np

S = 24
PX = (1, 2, 4, 8, 16)
FIXED = (0.01, 0.04, 0.16, 0.64, 2.56)
SCALINGS = {'none': 0, 'median': 1, 'per_trajectory': 2}
NEAR_MAX_FRACTION = 1e-3
RATIO_REL = 2.0 ** -21
KEYS = ['occlusion_accuracy'] + [f'{n}_{px}' for px in PX for n in ('pts_within', 'jaccard')] + ['average_jaccard', 'average_pts_within_thresh']


def generate(B, Q, T, seed=5):
  """A batch of B clips.  Depth z in about [0.5, 10], positions that drift, 85 % visible frames, predictions = (target + an error of
  (z / 256) * 2^u, u ~ U[-2, 6], in a random direction) / s_b with s_b = (1.0, 0.5, 2.0, 1.3)[b % 4]: the median scale recovers about s_b, and
  pts_within comes out near 0.25 / 0.38 / 0.50 / 0.63 / 0.75, so every pixel threshold cuts the data; sample 0 (s_b = 1) makes the `none`
  scaling cut too."""
  rng = np.random.default_rng(seed)
  z = np.clip(rng.uniform(1.0, 10.0, (B, Q, 1)) + np.cumsum(rng.normal(0.0, 0.05, (B, Q, T)), -1), 0.5, None)
  xy = (rng.uniform(-0.5, 0.5, (B, Q, 1, 2)) + np.cumsum(rng.normal(0.0, 0.01, (B, Q, T, 2)), -2)) * z[..., None]
  g = np.concatenate([xy, z[..., None]], -1)
  y = (rng.random((B, Q, T)) < 0.85).astype(np.float32)
  d = rng.normal(size=(B, Q, T, 3))
  d /= np.linalg.norm(d, axis=-1, keepdims=True)
  u = rng.uniform(-2.0, 6.0, (B, Q, T))
  delta = d * ((z / 256.0) * 2.0 ** u)[..., None]
  s_b = np.array([(1.0, 0.5, 2.0, 1.3)[b % 4] for b in range(B)])
  p = (g + delta) / s_b[:, None, None, None]
  l = rng.normal(size=(B, Q, T)) + (2.0 * y - 1.0)
  tq = rng.integers(0, T, (B, Q))
  g32 = g.astype(np.float32)
  qp = np.concatenate([tq[..., None].astype(np.float32), np.take_along_axis(g32, tq[:, :, None, None].repeat(3, -1), 2)[:, :, 0]], -1)
  return dict(p=p.astype(np.float32), l=l.astype(np.float32), g=g32, y=y, qp=qp.astype(np.float32), s_b=s_b.astype(np.float32))


def query_frame(qp, T):
  return np.clip(np.rint(np.asarray(qp, np.float64)[..., 0]), 0, T - 1).astype(np.int64)


def ratio64(p, g):
  n = lambda v: np.sqrt(np.maximum(1e-12, (np.asarray(v, np.float64) ** 2).sum(-1)))
  return n(g) / n(p)


def median32(values):
  """The fp32 median as the header defines it, on a float32 array (NaN entries are not part of the set); 1 for an empty set."""
  v = np.sort(np.asarray(values, np.float32).reshape(-1))
  v = v[~np.isnan(v)]
  m = v.size
  if m == 0:
    return np.float32(1.0)
  if m % 2:
    return v[m // 2]
  return np.float32(np.float32(0.5) * v[m // 2 - 1] + np.float32(0.5) * v[m // 2])


def median_cases():
  """Sets on which a radix select over bit patterns can go wrong, name -> float32 array (NaN entries are not part of a set)."""
  rng = np.random.default_rng(3)
  f = lambda a: np.asarray(a, np.float32)
  base = np.float32(1.2345)
  low_bits = (base.view(np.uint32) + rng.integers(0, 256, 1001).astype(np.uint32)).view(np.float32)  # differ only in the lowest 8 mantissa bits
  return {
      'empty': f([]), 'all nan': f([np.nan] * 5), 'one': f([3.5]), 'two': f([2.0, 5.0]), 'odd': f(rng.uniform(0.1, 9.0, 1001)), 'even': f(rng.uniform(0.1, 9.0, 1000)),
      'all equal': f([0.75] * 64), 'ties across the middle': f([1.0] * 10 + [2.0] * 10), 'ties below the middle': f([1.0] * 11 + [2.0] * 9),
      'three-way ties': f([1.0] * 4 + [1.5] * 2 + [2.0] * 4), 'tie on one side': f([1.0, 2.0, 2.0, 3.0, 3.0, 3.0]),
      'low 8 mantissa bits, odd': low_bits, 'low 8 mantissa bits, even': low_bits[:-1],
      '40 binades, odd': f(2.0 ** rng.uniform(-20, 20, 4097)), '40 binades, even': f(2.0 ** rng.uniform(-20, 20, 4096)),
      'middle across a binade': f([0.5, 0.9999999, 1.0, 1.0000001, 2.0, 4.0]), 'middle across the top digit': f([1e-30, 1e-20, 1e20, 1e30]),
      'with nan': f(np.where(rng.random(5000) < 0.15, np.nan, rng.uniform(0.5, 2.0, 5000))), 'zero and tiny': f([0.0, 1e-45, 1e-38, 1.0]),
  }


def reference(p, l, g, y, qp, row_scale, intrinsics=None, fixed=False):
  """p, g [R, T, 3]; l, y [R, T]; qp [R, 4]; row_scale [R]: the factor each row's predictions are multiplied by; intrinsics [R, 4] or None.
  float64 throughout.  Returns the exact slots, the count intervals and the left-out mask."""
  p, l, g, y, s = (np.asarray(a, dtype=np.float64) for a in (p, l, g, y, row_scale))
  R, T = l.shape
  tq = query_frame(qp, T)
  ew = np.arange(T)[None, :] != tq[:, None]
  pv, vis = l > 0, y > 0.5
  ps = p * s[:, None, None]
  e2 = np.sqrt(((ps - g) ** 2).sum(-1))
  if fixed:
    thr = np.broadcast_to(np.asarray(FIXED, np.float64), (R, T, 5))
  else:
    k = np.full((R, 4), (256.0, 256.0, 128.0, 128.0)) if intrinsics is None else np.asarray(intrinsics, np.float64)
    f = np.sqrt(k[:, 0] * k[:, 1] + 1e-12)
    thr = np.asarray(PX, np.float64)[None, None, :] * (g[..., 2] / f[:, None])[..., None]
  band = RATIO_REL * (np.linalg.norm(ps, axis=-1) + np.linalg.norm(g, axis=-1))[..., None] + 1e-6 * thr
  near = (np.abs(e2[..., None] - thr) <= band) & ew[..., None]
  ok = (ew & vis)[..., None]
  sure = ok & (e2[..., None] < thr) & ~near
  maybe = ok & near
  pv3 = pv[..., None]
  base = np.stack([ew.sum(-1), (ew & vis).sum(-1), (ew & (pv == vis)).sum(-1), (ew & pv).sum(-1)], -1).astype(np.float64)
  w = (sure.sum(1), (sure | maybe).sum(1))
  tp = ((sure & pv3).sum(1), ((sure | maybe) & pv3).sum(1))
  n_vis, n_pv = base[:, 1:2], base[:, 3:4]
  return dict(base=base, w=w, tp=tp, fp=(n_pv - tp[1], n_pv - tp[0]), fn=(n_vis - tp[1], n_vis - tp[0]), near=near, pairs=int(ew.sum()) * 5, tq=tq, ew=ew, vis=vis)


def check_rows(stats, ref, what='', assert_share=True):
  """stats [R, 24] as the code under test gave them against reference(...).  Prints each figure, then asserts; returns the left-out share."""
  stats = np.asarray(stats, np.float64)
  base = ref['base']
  assert stats.shape == (base.shape[0], S), stats.shape
  assert np.isfinite(stats).all(), f'{what}: non-finite stats'
  exact_bad = int((stats[:, :4] != base).sum())
  cnt_bad = 0
  for name, off in (('w', 0), ('tp', 1), ('fp', 2), ('fn', 3)):
    lo, hi = ref[name]
    got = stats[:, 4 + off::4]
    cnt_bad += int(((got < lo) | (got > hi) | (got != np.round(got))).sum())
  tp, fp, fn = (stats[:, 4 + o::4] for o in (1, 2, 3))
  ident_bad = int((tp + fn != stats[:, 1:2]).sum() + (tp + fp != stats[:, 3:4]).sum())
  left = float(ref['near'].sum()) / max(ref['pairs'], 1)
  print(f'  tapvid3d check {what}: rows {base.shape[0]}: exact-slot mismatches {exact_bad}, threshold-count mismatches {cnt_bad}, identity violations '
        f'{ident_bad}, pairs left out {left:.5%} (at most {NEAR_MAX_FRACTION:.1%})')
  assert not assert_share or left <= NEAR_MAX_FRACTION, f'{what}: {left:.4%} of the (frame, threshold) pairs lie in the rounding band of a threshold'
  assert exact_bad == 0 and cnt_bad == 0 and ident_bad == 0, what
  return left


def check_call(d, out, scaling, intrinsics=None, fixed=False, counts=None, what=''):
  """A whole call on generator data `d` (generate(...) or the same keys).  out: dict of NumPy arrays query_stats [B,Q,24], sample_stats
  [B,24], scale [B], row_scale [B,Q], ratio [B,Q,T].  counts: live queries per sample (None = all)."""
  B, Q, T = d['l'].shape
  qc = [Q] * B if counts is None else list(counts)
  qs, ss, scale, rs, ratio = (np.asarray(out[k]) for k in ('query_stats', 'sample_stats', 'scale', 'row_scale', 'ratio'))
  assert ratio.dtype == np.float32 and scale.dtype == np.float32 and rs.dtype == np.float32 and ss.dtype == np.float64
  worst_ratio, left = 0.0, []
  for b in range(B):
    n = qc[b]
    live = slice(0, n)
    assert not qs[b, n:].any() and not rs[b, n:].any() and not ratio[b, n:].any(), f'{what}: padded rows of sample {b} are not zero'
    tq = query_frame(d['qp'][b, live], T)
    ew = np.arange(T)[None, :] != tq[:, None]
    vis = d['y'][b, live] > 0.5
    if n:
      r64 = ratio64(d['p'][b, live], d['g'][b, live])
      worst_ratio = max(worst_ratio, float((np.abs(ratio[b, live] - r64) / r64).max()))
    if scaling == 'median':
      want = median32(ratio[b, live][vis & ew])
      assert scale[b].tobytes() == np.float32(want).tobytes(), f'{what}: sample {b} scale {scale[b]!r} is not the fp32 median {want!r} of the returned ratios'
      assert (rs[b, live] == scale[b]).all()
    else:
      assert scale[b] == 1.0
      if scaling == 'per_trajectory':
        assert (rs[b, live].view(np.uint32) == ratio[b, live][np.arange(n), tq].view(np.uint32)).all(), f'{what}: row_scale != ratio[q][tq]'
      else:
        assert (rs[b, live] == 1.0).all()
    if n:
      k = None if intrinsics is None else np.broadcast_to(np.asarray(intrinsics)[b], (n, 4))
      ref = reference(d['p'][b, live], d['l'][b, live], d['g'][b, live], d['y'][b, live], d['qp'][b, live], rs[b, live], k, fixed)
      left.append((float(ref['near'].sum()), ref['pairs']))
      check_rows(qs[b, live], ref, f'{what} sample {b}', assert_share=False)  # the share is asserted over the whole call below
    assert (ss[b] == qs[b].astype(np.float64).sum(0)).all(), f'{what}: sample_stats of sample {b} are not the sum of its rows'
  assert worst_ratio <= RATIO_REL, f'{what}: ratio rel err {worst_ratio:.3e} > {RATIO_REL:.3e}'
  share = sum(a for a, _ in left) / max(sum(b for _, b in left), 1)
  print(f'tapvid3d {what}: ratio rel err {worst_ratio:.3e} (bound {RATIO_REL:.3e}), pairs left out {share:.5%}, scale {np.asarray(scale).tolist()}')
  assert share <= NEAR_MAX_FRACTION
  return worst_ratio, share


def metrics(stats):
  """The 13 reference metrics of one stats row [24] (a pooled sample row or a query row), float64; zero denominators give 0."""
  s = np.asarray(stats, np.float64)
  div = lambda a, b: float(a / b) if b > 0 else 0.0
  m = {'occlusion_accuracy': div(s[2], s[0])}
  for k, px in enumerate(PX):
    m[f'pts_within_{px}'] = div(s[4 + 4 * k], s[1])
    m[f'jaccard_{px}'] = div(s[5 + 4 * k], s[1] + s[6 + 4 * k])
  m['average_jaccard'] = float(np.mean([m[f'jaccard_{px}'] for px in PX]))
  m['average_pts_within_thresh'] = float(np.mean([m[f'pts_within_{px}'] for px in PX]))
  return m
