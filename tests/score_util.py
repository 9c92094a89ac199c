"""Helpers of the score tests (tests/test_score_row_host.py, tests/test_gpu_score.py): a NumPy float64 restatement of the per-track score
definitions (include/spa3d.h, spa3d_scores) and the comparison rules.

Rules (each derived from the number formats, not from what the code gives):
  * counts that do not depend on a threshold (slots 0, 5, 6, 7) are exact: they come from comparisons of the inputs themselves;
  * threshold counts are exact once the (frame, threshold) pairs whose float64 e2 lies within relative 1e-5 of the threshold are left
    out: a row's count must lie between the reference count with every such pair classified "outside" and with every such pair classified
    "within".  At most 0.1 % of all pairs may be left out;
  * float sums (slots 1, 2, 4) match within relative (T + 8) * 2^-23: the worst case of a T-term fp32 sum of non-negative terms plus a few
    ulp of the per-term arithmetic (expf / log1pf, the squares and the square root);
  * slot 3 and frame_err match within relative 2^-22 per element: one sqrtf over at most three squared fp32 differences;
  * TP_k + FN_k == slot 0 and TP_k + FP_k == slot 6 hold exactly on every row."""
import numpy as np

NEAR_REL = 1e-5
NEAR_MAX_FRACTION = 1e-3


def log_sigmoid(x):
  return np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x)))


def reference(p, l, g, y, thresholds, scale=None):
  """p, g [R, T, NC]; l, y [R, T] (any float dtype; values are taken as they are, arithmetic in float64); thresholds: K floats;
  scale: [R] per-row factor or None.  Returns a dict of float64 arrays."""
  p, l, g, y = (np.asarray(a, dtype=np.float64) for a in (p, l, g, y))
  R, T = l.shape
  K = len(thresholds)
  d = p - g
  e1 = np.abs(d).sum(-1)
  e2 = np.sqrt((d * d).sum(-1))
  pv, vis = l > 0, y > 0.5
  bce = -y * log_sigmoid(l) - (1.0 - y) * log_sigmoid(-l)
  sc = np.ones(R, np.float32) if scale is None else np.asarray(scale, np.float32).reshape(R)
  thr = (np.asarray(thresholds, np.float32).reshape(1, K) * sc.reshape(R, 1)).astype(np.float64)  # tau_k * scale_b, rounded once to fp32
  base = np.stack([vis.sum(-1), (y * e1).sum(-1), (y * e2).sum(-1), np.where(vis, e2, 0.0).max(-1), bce.sum(-1), (pv == vis).sum(-1), pv.sum(-1),
                   np.full(R, T)], -1).astype(np.float64)
  near = np.abs(e2[:, :, None] - thr[:, None, :]) <= NEAR_REL * thr[:, None, :]  # [R, T, K]
  sure = vis[:, :, None] & (e2[:, :, None] < thr[:, None, :]) & ~near
  maybe = vis[:, :, None] & near
  pv3 = pv[:, :, None]
  w_lo, w_hi = sure.sum(1), (sure | maybe).sum(1)
  tp_lo, tp_hi = (sure & pv3).sum(1), ((sure | maybe) & pv3).sum(1)
  n_vis, n_pv = base[:, 0:1], base[:, 6:7]
  return dict(base=base, e2=e2, near=near, w=(w_lo, w_hi), tp=(tp_lo, tp_hi), fp=(n_pv - tp_hi, n_pv - tp_lo), fn=(n_vis - tp_hi, n_vis - tp_lo), K=K, T=T)


def check(stats, frame_err, ref, what=''):
  """stats [R, 8 + 4K] and frame_err [R, T] (or None) as the code under test gave them, against reference(...).  Prints each figure, then asserts."""
  stats = np.asarray(stats, dtype=np.float64)
  base, K, T = ref['base'], ref['K'], ref['T']
  assert stats.shape == (base.shape[0], 8 + 4 * K), (stats.shape, base.shape, K)
  assert np.isfinite(stats).all(), f'{what}: non-finite stats'
  near_frac = float(ref['near'].mean()) if K else 0.0
  sum_bound = (T + 8) * 2.0 ** -23
  rel = lambda got, want: float((np.abs(got - want) / np.maximum(np.abs(want), 1e-30)).max()) if got.size else 0.0
  sum_err = max(rel(stats[:, s], base[:, s]) for s in (1, 2, 4))
  max_err = rel(stats[:, 3], base[:, 3])
  fe_err = rel(np.asarray(frame_err, dtype=np.float64), ref['e2']) if frame_err is not None else 0.0
  exact_bad = int(sum((stats[:, s] != base[:, s]).sum() for s in (0, 5, 6, 7)))
  cnt_bad = 0
  for name, off in (('w', 0), ('tp', 1), ('fp', 2), ('fn', 3)):
    lo, hi = ref[name]
    got = stats[:, 8 + off::4][:, :K]
    cnt_bad += int(((got < lo) | (got > hi) | (got != np.round(got))).sum())
  tp, fp, fn = (stats[:, 8 + o::4][:, :K] for o in (1, 2, 3))
  ident_bad = int((tp + fn != stats[:, 0:1]).sum() + (tp + fp != stats[:, 6:7]).sum())
  print(f'  score check {what}: rows {base.shape[0]} T {T} K {K}: sum rel err {sum_err:.3e} (bound {sum_bound:.3e}), max-slot rel err {max_err:.3e} and '
        f'frame_err rel err {fe_err:.3e} (bound {2.0 ** -22:.3e}), exact-count mismatches {exact_bad}, threshold-count mismatches {cnt_bad}, '
        f'identity violations {ident_bad}, pairs left out {near_frac:.5%} (at most {NEAR_MAX_FRACTION:.1%})')
  assert near_frac <= NEAR_MAX_FRACTION, f'{what}: {near_frac:.4%} of the (frame, threshold) pairs lie within 1e-5 of a threshold'
  assert exact_bad == 0 and cnt_bad == 0 and ident_bad == 0, what
  assert sum_err <= sum_bound and max_err <= 2.0 ** -22 and fe_err <= 2.0 ** -22, what
