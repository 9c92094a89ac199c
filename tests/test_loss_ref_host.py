"""The references and gates of tests/test_gpu_loss_ops.py, on the CPU (tests/loss_util.py): for every gate the fp32 restatement of the operation passes it and
each wrong variant it is there for fails it -- a gate that nothing can fail is not a test (the pattern of tests/test_parity_gates_host.py).  The cap-crossing
shape is the GPU test's own: 2 x 2049 query rows of 257 frames, 1 053 186 points."""
import math

import numpy as np
import pytest

import loss_util as LU

F32 = np.float32
NQ, T = 2 * 2049, 257
N = NQ * T


@pytest.fixture(scope='module')
def big():
  head, tgt, vis, w = LU.draw_case(NQ, T, 3, seed=11)
  tracks, vlog, _ = LU.split_head(head, T, 3)
  return dict(head=head, tgt=tgt, vis=vis, w=w, tracks=tracks, vlog=vlog)


def _gate(o, c, variant_terms=None, variant_sum=None, w=True):
  """(position passes, visibility passes, ratios) of the fp32 restatement -- or a wrong variant of it -- at the numerator gate against float64"""
  wt = c['w'] if w else None
  r = LU.point_terms(o, c['tracks'], c['vlog'], c['tgt'], c['vis'], wt, np.float64)
  g = LU.point_terms(o, c['tracks'], c['vlog'], c['tgt'], c['vis'], wt, F32, variant_terms)
  ref, got = LU.numerators(*r), LU.numerators(*g, variant=variant_sum)
  res = []
  for k in range(2):
    res.append(abs(got[k] - ref[k]) / LU.numerator_bound(r[k]))
  return res[0] <= 1.0, res[1] <= 1.0, res


@pytest.mark.parametrize('name', sorted(LU.OBJECTIVES))
def test_fp32_restatement_passes_the_numerator_gate(big, name):
  assert N > LU.CAP
  for w in (True, False):
    okp, okv, ratio = _gate(LU.OBJECTIVES[name], big, w=w)
    print(f'objective {name}, weights {w}: fp32 pairwise sum at {ratio[0]:.4f} (position) and {ratio[1]:.4f} (visibility) of the bound')
    assert okp and okv
    assert ratio[0] < 0.25 and ratio[1] < 0.25, 'the reference alone must sit well inside its bound'


def test_numerator_gate_rejects_swapped_y_and_w(big):
  okp, okv, ratio = _gate(LU.OBJECTIVES['e'], big, variant_terms='swap_yw')
  print(f'y and w swapped: visibility numerator at {ratio[1]:.3g} x the bound')
  assert not okv


def test_huber_branch_at_the_boundary_shows_in_the_bits():
  """rho is continuous at |d| == delta, so no tolerance can tell <= from <: the two branches round differently in fp32, and a one-point loss is exact"""
  o, d = LU.huber_edge()
  z = np.zeros((1, 1, 3), dtype=F32)
  tr = z.copy(); tr[0, 0, 0] = d
  one, lg = np.ones((1, 1), dtype=F32), np.full((1, 1), 200.0, dtype=F32)
  good = LU.point_terms(o, tr, lg, z, one, None, F32)[0][0]
  bad = LU.point_terms(o, tr, lg, z, one, None, F32, 'huber_lt')[0][0]
  assert good != bad and abs(float(good) - float(bad)) >= 2.0 ** -24, 'the difference must survive the fixed-point unit'
  assert float(good) * 2 ** 24 == round(float(good) * 2 ** 24)
  # and on random data the variant is invisible, as it must be: no drawn error equals delta
  head, tgt, vis, w = LU.draw_case(64, T, 3, seed=3)
  tracks, vlog, _ = LU.split_head(head, T, 3)
  a = LU.point_terms(LU.OBJECTIVES['c'], tracks, vlog, tgt, vis, w, F32)
  b = LU.point_terms(LU.OBJECTIVES['c'], tracks, vlog, tgt, vis, w, F32, 'huber_lt')
  assert np.array_equal(a[0], b[0])


def test_exact_lane_rejects_an_element_dropped_or_counted_twice():
  head, tgt, vis, w, P, V, cnt = LU.exact_case(NQ, T, 3, seed=21)
  tracks, vlog, _ = LU.split_head(head, T, 3)
  pt, vt = LU.point_terms(LU.EXACT_OBJ, tracks, vlog, tgt, vis, w, F32)
  assert pt[LU.CAP] != 0 and vt[LU.CAP] != 0, 'the element at the cap must carry both terms'
  got = LU.numerators(pt, vt)
  assert (got[0], got[1]) == (P, V), 'the fp32 restatement is exact on the lane, in numpy\'s order as in any other'
  for order in (np.arange(N)[::-1], np.random.default_rng(0).permutation(N)):
    assert float(np.sum(pt[order], dtype=F32)) == P and float(np.sum(vt[order], dtype=F32)) == V
  for variant in ('drop', 'twice'):
    bad = LU.numerators(pt, vt, variant=variant)
    assert bad[0] != P and bad[1] != V, variant
  assert cnt == float(vis.sum(dtype=np.float64)) and cnt > 2 ** 18
  # both Huber branches, zero-gradient points and points with y = 0 are all there
  d = np.abs(tracks - tgt)
  assert (d[(d > 0)] <= 0.125).any() and (d > 0.125).any() and ((d.sum(-1) == 0) & (vis > 0) & (np.abs(vlog) < 100)).any() and ((vis == 0) & (vlog > 0)).any()
  # loss3[0] with the default weights is not an exact product: it is pinned as the fp32 expression
  D = 2.0 ** 18
  tot, pos, v = LU.loss3_from(LU.EXACT_OBJ, P, V, D)
  assert float(pos) == P / D and float(v) == V / D and tot == LU.total_of(LU.EXACT_OBJ, pos, v)
  assert float(tot) != 5000.0 * P / D + 1e-8 * V / D


# ------------------------------------------------------------------------------------------------ head cotangent
def _cot_case(nc, seed=5, nq=37):
  head, tgt, vis, w = LU.draw_case(nq, T, nc, seed=seed)
  h = head.reshape(nq, 4, T)
  h[::3, 0, ::5] = tgt[::3, ::5, 0]   # prediction == target on a grid of points: sign(0) = 0 there
  vis[::3, ::5] = 1.0
  w[::3, ::5] = np.maximum(w[::3, ::5], F32(0.5))
  return h.reshape(nq, 4 * T), tgt, vis, w


@pytest.mark.parametrize('nc', [3, 2])
@pytest.mark.parametrize('name', ['d', 'e'])
def test_cotangent_gate_accepts_the_restatement_and_rejects_its_variants(nc, name):
  o = LU.OBJECTIVES[name]
  head, tgt, vis, w = _cot_case(nc)
  D = LU.denominator(vis, 0.0)
  ref, K = LU.head_cotangent(o, head, tgt, vis, w, T, nc, D, 1.0, np.float64)
  got, _ = LU.head_cotangent(o, head, tgt, vis, w, T, nc, D, 1.0, F32)
  bad, ratio = LU.cotangent_report(got, ref, K, 'fp32')
  print(f'objective {name}, NC {nc}: fp32 restatement at {ratio:.3f} of the bound')
  assert bad == 0
  variants = (['sign0'] if o.position_kind == 0 else []) + (['certain'] if nc == 2 else [])   # (Huber's inner branch gives d / delta = 0 at d = 0 whatever sign(0) is)
  for v in variants:
    wrong, _ = LU.head_cotangent(o, head, tgt, vis, w, T, nc, D, 1.0, F32, v)
    nbad, r = LU.cotangent_report(wrong, ref, K, 'fp32')
    assert nbad > 0, v
  if nc == 2:
    assert not ref.reshape(-1, 4, T)[:, 3].any() and ref.reshape(-1, 4, T)[:, 2].any()
  # the 16-bit gates: one rounding of the type on top; an fp16 overflow must be an inf
  import torch
  for prec, dt in (('bf16', torch.bfloat16), ('fp16', torch.float16)):
    fac = 2.0 ** math.ceil(math.log2(2e5 / np.abs(ref).max())) if prec == 'fp16' else 1.0   # fp16: a loss scale that pushes the largest entries past 65504
    r16 = torch.from_numpy(got * F32(fac)).to(dt).double().numpy()
    ref16, K16 = ref * fac, K * fac
    if prec == 'fp16':
      assert (np.abs(ref16) > 65520).any() and np.isinf(r16).any()
      finite = np.where(np.isinf(r16), np.sign(r16) * 60000.0, r16)
      assert LU.cotangent_report(finite, ref16, K16, prec)[0] > 0, 'a finite number where the value overflows fp16 must be rejected'
    nbad, r = LU.cotangent_report(r16, ref16, K16, prec)
    print(f'{prec}: the fp32 restatement rounded once to the type at {r:.3f} of the bound')
    assert nbad == 0 and r > 0.9, (prec, r)   # half an ulp is what one rounding costs: the gate is tight
    # a store that truncates (the top 16 bits of the fp32 word, as a bf16 store without rounding would) is off by up to an ulp: rejected
    if prec == 'bf16':
      cut = (got.view(np.int32) & np.int32(-65536)).view(F32).astype(np.float64)
      assert LU.cotangent_report(cut, ref16, K16, prec)[0] > 0


# ------------------------------------------------------------------------------------------------ loss scale
def test_loss_scale_reference_values_and_the_round_variant():
  gm = float(LU.gmax(LU.Obj()))
  assert gm == 5000.0 and float(LU.gmax(LU.UNIT_GMAX)) == 1.0 and float(LU.gmax(LU.OBJECTIVES['b'])) == 3.0
  R = LU.loss_scale_ref
  assert R(2.56e6, gm, -16.0) == 8192.0 and R(4.4e6, gm, -16.0) == 8192.0 and R(312.5, gm, -16.0) == 1.0 and R(100.0, gm, -16.0) == 1.0 and R(1e12, gm, -16.0) == 2.0 ** 24
  assert R(1.0, gm, 1024.0) == 1024.0 and R(1.0, gm, 1024.0, 0.25) == 256.0
  assert all(R(1.0, gm, 1024.0, s) == 1024.0 for s in (0.0, 1.0, 2.0)) and R(1.0, gm, 1.0, 2.0 ** -30) == 2.0 ** -24
  differs, log2_off = 0, []
  for g in (gm, 1.0):
    for d in LU.loss_scale_denoms(g):
      want = R(d, g, -16.0)
      assert want == 2.0 ** LU.floor_log2(want) and 1.0 <= want <= 2.0 ** 24
      q = float(F32(F32(F32(d) * F32(16.0)) / F32(g)))
      assert want == 1.0 or want == 2.0 ** 24 or want <= q < 2.0 * want   # the largest power of two not above q
      differs += R(d, g, -16.0, variant='round') != want
      if LU.loss_scale_log2_route(d, g, -16.0) != want:
        log2_off.append((q, LU.loss_scale_log2_route(d, g, -16.0), want))
  assert differs >= 20, 'rounding the logarithm must show on the sweep (the upper neighbours of the powers of two)'
  # exp2(floor(log2 q)) in fp32 -- the expression the kernel uses -- is off IN NUMPY where q lies an ulp or two below 2^k: log2 q is then closer to k than fp32
  # resolves near k, rounds to k, and the route returns 2^k > q, one power of two too many.  Nowhere else on the sweep.  So the reference takes the exponent with
  # frexp, and whether the device's log2f has the same weakness is what the GPU test measures (it does not).
  assert len(log2_off) >= 20 and all(got == 2.0 * want and got * (1.0 - 2.0 ** -21) < q < got for q, got, want in log2_off)
  assert len(LU.loss_scale_denoms(gm)) == 80


# ------------------------------------------------------------------------------------------------ guard
def test_guard_state_machine():
  g = LU.Guard()
  assert g.step(True) == [0.0, 0.0, 1.0, 0.0]            # zero memory reads as 1 and stays there
  assert g.step(False) == [1.0, 1.0, 0.5, 0.0]
  for _ in range(199):
    s = g.step(True)
  assert s == [0.0, 1.0, 0.5, 199.0]
  assert g.step(True) == [0.0, 1.0, 1.0, 0.0]
  g.step(False); assert g.step(False) == [1.0, 3.0, 0.25, 0.0]
  for _ in range(200):
    s = g.step(True)
  assert s[2:] == [0.5, 0.0]
  for _ in range(200):
    s = g.step(True)
  assert s[2:] == [1.0, 0.0]
  for start in (0.3, 2.0 ** -25, 2.0, -0.5, float('nan')):
    assert LU.Guard(start).step(True)[2] == 1.0 and LU.Guard(start).step(False)[2] == 0.5
  assert LU.Guard(2.0 ** -24).step(False)[2] == 2.0 ** -24
  assert LU.Guard(0.5, count=150).step(False) == [1.0, 1.0, 0.25, 0.0]


# ------------------------------------------------------------------------------------------------ AdamW
def _state(n, seed=5):
  r = np.random.default_rng(seed)
  return (r.standard_normal(n).astype(F32), (r.standard_normal(n) * 0.01).astype(F32), (r.standard_normal(n) * 0.001).astype(F32), (r.random(n) * 1e-4).astype(F32))


def test_adamw_gates_accept_the_restatement_and_reject_the_variants():
  n = 4099
  p, g, m, v = _state(n)
  # clipped lane (norm ~ 0.64 against clip 0.1), two steps skipped before: the bias correction sits at step + 1 - skipped
  kw = dict(step=3, lr=3e-4, clip=0.1, skipped=2)
  ref = LU.adamw_ref(p, g, m, v, **kw)
  assert LU.adamw_passes(LU.adamw_ref(p, g, m, v, dtype=F32, **kw), ref)
  assert not LU.adamw_passes(LU.adamw_ref(p, g, m, v, dtype=F32, variant='bias_at_step', **kw), ref)
  # unclipped lane: norm < clip, the update is that of clip = inf
  gs = (g * F32(0.5 / ref[3])).astype(F32)
  kw = dict(step=7, lr=3e-4, clip=1.0)
  ref = LU.adamw_ref(p, gs, m, v, **kw)
  assert ref[3] < 1.0 and LU.adamw_errs(ref, LU.adamw_ref(p, gs, m, v, step=7, lr=3e-4, clip=float('inf'))) == (0.0, 0.0, 0.0)
  assert LU.adamw_passes(LU.adamw_ref(p, gs, m, v, dtype=F32, **kw), ref)
  assert not LU.adamw_passes(LU.adamw_ref(p, gs, m, v, dtype=F32, variant='always_clip', **kw), ref)
  # norm == clip exactly: sc = 1 exactly, whichever side of the comparison takes it
  gu = LU.unit_norm_gradient(n)
  assert float(np.sum(gu * gu, dtype=F32)) == 1.0 and LU.adamw_ref(p, gu, m, v, **kw)[3] == 1.0
  a, b = LU.adamw_ref(p, gu, m, v, **kw), LU.adamw_ref(p, gu, m, v, step=7, lr=3e-4, clip=float('inf'))
  assert LU.adamw_errs(a, b) == (0.0, 0.0, 0.0) and LU.adamw_passes(LU.adamw_ref(p, gu, m, v, dtype=F32, **kw), a)
  # small-state lane: eps dominates the denominator, and the p gate separates sqrt(v) + eps from sqrt(v + eps) by orders of magnitude
  ps, gsm, ms, vs = LU.small_state(n, seed=9)
  kw = dict(step=7, lr=1e-2, clip=1.0)
  ref = LU.adamw_ref(ps, gsm, ms, vs, **kw)
  assert LU.adamw_passes(LU.adamw_ref(ps, gsm, ms, vs, dtype=F32, **kw), ref)
  wrong = LU.adamw_ref(ps, gsm, ms, vs, dtype=F32, variant='eps_inside', **kw)
  e = LU.adamw_errs(wrong, ref)[0]
  print(f'small-state lane: eps inside the root moves p by {e:.3e} against the gate {LU.ADAMW_GATES["p"]:.0e}')
  assert e > 100 * LU.ADAMW_GATES['p']
  # ... which the everyday lane cannot see: sqrt(v) ~ 7e-3 there
  p, g, m, v = _state(n)
  big = LU.adamw_ref(p, g, m, v, step=7, lr=3e-4)
  assert LU.adamw_passes(LU.adamw_ref(p, g, m, v, step=7, lr=3e-4, dtype=F32, variant='eps_inside'), big)
  # v = 0 and g = 0: the update is exactly -lr wd p
  z = np.zeros(n, dtype=F32)
  out = LU.adamw_ref(p, z, z, z, step=0, lr=3e-4, dtype=F32)
  assert np.array_equal(out[0], p - F32(3e-4) * (F32(0.0) + F32(0.01) * p)) and not out[1].any() and not out[2].any()
