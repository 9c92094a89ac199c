"""The kernels of csrc/loss.hip between the head and the parameter update, on their own: the loss sums in head form (spa3d_op_head_loss) and split form
(spa3d_loss), the visible count, the head cotangent in all three storage types, the fp16 loss scale, AdamW with its guard, and the Threefry noise --
each against a plain reference (tests/loss_util.py; tests/test_loss_ref_host.py shows on the CPU that every gate used here accepts the fp32 restatement
and rejects the wrong variants it is there for).

Shapes: T_out = 257 (odd: rows straddle waves); nq = 4099, or B x Q = 2 x 2049, puts 1 053 443 / 1 053 186 points behind the loss kernels -- past the
4096-workgroup cap (1 048 576 points) and, for the count, past its 1024-workgroup cap; the small cases catch wave and workgroup tails.  Every output sits in a
parity_util.guarded allocation, checked after each call.  loss_bwd_kernel's own grid cap (2^20 workgroups) would need a 1 GiB output to bind: not covered."""
import contextlib
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import loss_util as LU
import optim_util as OU
import parity_util as PU

pytestmark = pytest.mark.gpu

F32 = np.float32
T = 257
NQ_HEAD, B_SPLIT, Q_SPLIT = 4099, 2, 2049
SMALL = [(1, 1), (9, 7), (1, 64), (5, 13), (255, 1), (4, 64), (1, 257)]   # (nq, T_out): 1, 63, 64, 65, 255, 256, 257 points
TORCH_DT = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


@pytest.fixture(scope='module')
def lib(spa3d):
  return spa3d._lib.load()


def _s():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_MODELS = {}


def _handle(spa3d, t_out, nc, precision='fp32'):
  key = (t_out, nc, precision)
  if key not in _MODELS:
    m = (spa3d.TrackAutoEncoder3D(num_output_frames=t_out, use_dino=False, use_depth=False, precision=precision) if nc == 3
         else spa3d.TrackAutoEncoder(num_output_frames=t_out, precision=precision))
    _MODELS[key] = (m, m._handle(0, 0)[0])
  return _MODELS[key][1]


def _dev(x):
  return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).cuda()


@contextlib.contextmanager
def _objective(lib, spa3d, h, o, w, B, Q):
  """the objective and the weight plane on the handle for the calls inside the block"""
  cfg = spa3d._lib.LossConfig(o.l1_weight, o.bce_weight, o.position_kind, o.huber_delta, (C.c_float * 3)(*o.axis_weight), o.bce_pos_weight)
  assert lib.spa3d_set_loss(h, C.byref(cfg)) == 0, lib.spa3d_last_error(h)
  wd = _dev(w) if w is not None else None
  try:
    if wd is not None:
      assert lib.spa3d_set_point_weights(h, B, Q, wd.data_ptr()) == 0
    yield
  finally:
    lib.spa3d_set_point_weights(h, 0, 0, None)
    lib.spa3d_set_loss(h, None)


def _parse(l3):
  """loss3 (12 floats, on the host): results, flag, the three fixed-point accumulators in 2^-24 units, denominator, loss scale"""
  l3 = l3.contiguous()
  acc = l3[4:10].view(torch.int64)
  return dict(out=l3[:3].numpy().copy(), flag=int(l3[3:4].view(torch.int32)), P=int(acc[0]) * 2.0 ** -24, V=int(acc[1]) * 2.0 ** -24, cnt=int(acc[2]) * 2.0 ** -24,
              denom=float(l3[10]), scale=float(l3[11]))


def _head_loss(lib, spa3d, h, head, tgt, vis, denom, nc, t_out, dt=None, outs=True):
  """one spa3d_op_head_loss into guarded outputs -> parsed loss3, the split predictions (device) and dhead (host, as stored)"""
  hd, td, vd = _dev(head), _dev(tgt), _dev(vis)
  nq = hd.shape[0]
  loss3 = PU.guarded(1, 12, torch.float32, name='loss3')[0]
  tr = vl = cl = dh = out = None
  if outs:
    tr, vl, cl = PU.guarded(nq, t_out * nc, torch.float32, name='tracks'), PU.guarded(nq, t_out, torch.float32, name='vlog'), PU.guarded(nq, t_out, torch.float32, name='clog')
    out = spa3d._lib.Outputs(tr.data_ptr(), vl.data_ptr(), cl.data_ptr(), None)
  if dt is not None:
    dh = PU.guarded(nq, 4 * t_out, dt, name='dhead')
  rc = lib.spa3d_op_head_loss(h, hd.data_ptr(), nq, td.data_ptr(), vd.data_ptr(), float(denom), C.byref(out) if out is not None else None, loss3.data_ptr(),
                              dh.data_ptr() if dh is not None else None, _s())
  assert rc == 0, lib.spa3d_last_error(h)
  torch.cuda.synchronize()
  res = _parse(loss3.cpu())
  res.update(tracks=tr, vlog=vl, clog=cl, dhead=dh.cpu() if dh is not None else None)
  PU.check_guards()
  return res


def _split_loss(lib, spa3d, h, tracks, vlog, tgt, vis, denom, B, Q, counts=None):
  """one spa3d_loss -> parsed loss3"""
  trd, vld, td, vd = _dev(tracks), _dev(vlog), _dev(tgt), _dev(vis)
  b = spa3d._lib.Batch()
  b.B, b.Q = B, Q
  b.query_tracks, b.query_tracks_visible = td.data_ptr(), vd.data_ptr()
  out = spa3d._lib.Outputs(trd.data_ptr(), vld.data_ptr(), None, None)
  loss3 = PU.guarded(1, 12, torch.float32, name='loss3')[0]
  if counts is not None:
    assert lib.spa3d_set_counts(h, B, None, (C.c_int32 * B)(*counts)) == 0
  try:
    rc = lib.spa3d_loss(h, C.byref(b), C.byref(out), float(denom), loss3.data_ptr(), _s())
  finally:
    lib.spa3d_set_counts(h, 0, None, None)
  assert rc == 0, lib.spa3d_last_error(h)
  torch.cuda.synchronize()
  res = _parse(loss3.cpu())
  PU.check_guards()
  return res


def _bits(x):
  return np.asarray(x, dtype=F32).view(np.int32)


def _same_bits(a, b):
  return np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _random_case(nq, t_out, nc, weighted, seed=11):
  return LU.draw_case(nq, t_out, nc, seed=seed, weights=weighted)


@functools.lru_cache(maxsize=None)
def _reference(nq, t_out, nc, weighted, name):
  """the float64 numerators, their bounds and the exact count of a random case under objective `name`: computed once, shared"""
  head, tgt, vis, w = _random_case(nq, t_out, nc, weighted)
  tracks, vlog, _ = LU.split_head(head, t_out, nc)
  pt, vt = LU.point_terms(LU.OBJECTIVES[name], tracks, vlog, tgt, vis, w, np.float64)
  P, V = LU.numerators(pt, vt)
  return P, V, LU.numerator_bound(pt), LU.numerator_bound(vt), float(vis.sum(dtype=np.float64))


def _check_numerators(res, ref, o, what):
  P, V, bp, bv, cnt = ref
  ep, ev = abs(res['P'] - P), abs(res['V'] - V)
  print(f'  {what}: position numerator |err| {ep:.3e} (bound {bp:.3e}, {ep / bp:.4f} x), visibility numerator |err| {ev:.3e} (bound {bv:.3e}, {ev / bv:.4f} x)')
  assert res['flag'] == 0 and ep <= bp and ev <= bv, what
  assert res['cnt'] == cnt and res['denom'] == max(cnt, 1.0), (what, res['cnt'], cnt)
  assert _same_bits(res['out'][0], LU.total_of(o, res['out'][1], res['out'][2])), what
  D = F32(res['denom'])
  assert _same_bits(res['out'][1], F32(res['P']) / D) and _same_bits(res['out'][2], F32(res['V']) / D), what
  return ep / bp, ev / bv


# ------------------------------------------------------------------------------------------------ (a) random lane, (c) head form = split form
CASES_A = [('a', False, 3), ('b', True, 3), ('c', True, 3), ('d', True, 3), ('d', False, 3), ('e', True, 3), ('e', True, 2), ('d', False, 2)]


@pytest.mark.parametrize('name,weighted,nc', CASES_A)
def test_head_loss_past_the_grid_cap_against_fp64_and_the_split_form(lib, spa3d, name, weighted, nc):
  """spa3d_op_head_loss at 1 053 443 points: both numerators within the derived bound of float64, the count exact, loss3[0] the fp32 expression of loss3[1..2];
  the predictions it writes are bit copies of the head's blocks, and spa3d_loss on them gives the same bits (both kernels run loss_point.hpp on the same values
  in the same order, without contraction)."""
  o = LU.OBJECTIVES[name]
  nq = NQ_HEAD
  assert nq * T > LU.CAP
  head, tgt, vis, w = _random_case(nq, T, nc, weighted)
  h = _handle(spa3d, T, nc)
  with _objective(lib, spa3d, h, o, w, 1, nq):
    res = _head_loss(lib, spa3d, h, head, tgt, vis, 0.0, nc, T)
    _check_numerators(res, _reference(nq, T, nc, weighted, name), o, f'head form, objective {name}, NC {nc}, weights {weighted}')
    assert res['scale'] == 1.0
    tracks, vlog, clog = LU.split_head(head, T, nc)
    assert _same_bits(res['tracks'].cpu().numpy().reshape(tracks.shape), tracks) and _same_bits(res['vlog'].cpu().numpy(), vlog)
    assert _same_bits(res['clog'].cpu().numpy(), clog) and (nc == 2) == bool(clog.any())
    split = _split_loss(lib, spa3d, h, res['tracks'], res['vlog'], tgt, vis, 0.0, 1, nq)
  same = _same_bits(split['out'], res['out']) and (split['P'], split['V'], split['cnt']) == (res['P'], res['V'], res['cnt'])
  print(f'  head form vs split form: {"equal bits" if same else "DIFFERENT bits"}: {res["out"]} / {split["out"]}')
  assert same


@pytest.mark.parametrize('name,weighted,nc', [('e', True, 3), ('d', False, 3), ('c', True, 2)])
def test_split_loss_past_the_grid_cap_against_fp64(lib, spa3d, name, weighted, nc):
  """spa3d_loss at B x Q = 2 x 2049 (1 053 186 points)"""
  o = LU.OBJECTIVES[name]
  nq = B_SPLIT * Q_SPLIT
  head, tgt, vis, w = _random_case(nq, T, nc, weighted)
  tracks, vlog, _ = LU.split_head(head, T, nc)
  h = _handle(spa3d, T, nc)
  with _objective(lib, spa3d, h, o, w, B_SPLIT, Q_SPLIT):
    res = _split_loss(lib, spa3d, h, tracks, vlog, tgt, vis, 0.0, B_SPLIT, Q_SPLIT)
  _check_numerators(res, _reference(nq, T, nc, weighted, name), o, f'split form, objective {name}, NC {nc}, weights {weighted}')


@pytest.mark.parametrize('nc', [3, 2])
def test_small_shapes_both_forms(lib, spa3d, nc):
  """1, 63, 64, 65, 255, 256 and 257 points: wave and workgroup tails"""
  o = LU.OBJECTIVES['e']
  for nq, t_out in SMALL:
    head, tgt, vis, w = _random_case(nq, t_out, nc, True, seed=100 + nq * t_out)
    tracks, vlog, clog = LU.split_head(head, t_out, nc)
    pt, vt = LU.point_terms(o, tracks, vlog, tgt, vis, w, np.float64)
    ref = LU.numerators(pt, vt) + (LU.numerator_bound(pt), LU.numerator_bound(vt), float(vis.sum(dtype=np.float64)))
    h = _handle(spa3d, t_out, nc)
    with _objective(lib, spa3d, h, o, w, nq, 1):
      res = _head_loss(lib, spa3d, h, head, tgt, vis, 0.0, nc, t_out, dt=torch.float32)
      _check_numerators(res, ref, o, f'head form, {nq} x {t_out}, NC {nc}')
      split = _split_loss(lib, spa3d, h, tracks, vlog, tgt, vis, 0.0, nq, 1)
      _check_numerators(split, ref, o, f'split form, {nq} x {t_out}, NC {nc}')
    assert _same_bits(split['out'], res['out']) and _same_bits(res['tracks'].cpu().numpy().reshape(tracks.shape), tracks) and _same_bits(res['clog'].cpu().numpy(), clog)
    ref64, K = LU.head_cotangent(o, head, tgt, vis, w, t_out, nc, res['denom'], 1.0, np.float64)
    bad, ratio = LU.cotangent_report(res['dhead'].numpy(), ref64, K, 'fp32')
    assert bad == 0, (nq, t_out, ratio)


def test_huber_branch_at_the_boundary(lib, spa3d):
  """one point with |d| == delta exactly: the quadratic branch (|d| <= delta), bit for bit -- the two branches round differently there (tests/loss_util.py huber_edge)"""
  o, d = LU.huber_edge()
  head = np.zeros((1, 4), dtype=F32); head[0, 0] = d; head[0, 3] = 200.0
  tgt, vis = np.zeros((1, 1, 3), dtype=F32), np.ones((1, 1), dtype=F32)
  want = LU.point_terms(o, head[:, :3].reshape(1, 1, 3), head[:, 3], tgt, vis, None, F32)[0][0]
  wrong = LU.point_terms(o, head[:, :3].reshape(1, 1, 3), head[:, 3], tgt, vis, None, F32, 'huber_lt')[0][0]
  h = _handle(spa3d, 1, 3)
  with _objective(lib, spa3d, h, o, None, 1, 1):
    res = _head_loss(lib, spa3d, h, head, tgt, vis, 1.0, 3, 1)
    split = _split_loss(lib, spa3d, h, head[:, :3].reshape(1, 1, 3), head[:, 3].reshape(1, 1), tgt, vis, 1.0, 1, 1)
  assert want != wrong
  assert _same_bits(res['out'][1], want) and _same_bits(split['out'][1], want) and res['out'][2] == 0.0


# ------------------------------------------------------------------------------------------------ (b) exact lane
@functools.lru_cache(maxsize=None)
def _exact(nq, nc):
  return LU.exact_case(nq, T, nc, seed=21 + nc)


@pytest.mark.parametrize('form', ['head', 'split'])
@pytest.mark.parametrize('nc', [3, 2])
def test_exact_lane_is_bit_equal_past_both_caps(lib, spa3d, form, nc):
  """Every intermediate exactly representable (tests/loss_util.py exact_case): the accumulators hold the exact integers, loss3[1..2] their quotients by a
  power-of-two denominator, loss3[0] the fp32 expression with the default weights.  With denom = 0 the denominator is vis_count_kernel's exact count over more
  than 262 144 entries (its own cap) and the quotients are one correctly rounded division."""
  o = LU.EXACT_OBJ
  nq = NQ_HEAD if form == 'head' else B_SPLIT * Q_SPLIT
  head, tgt, vis, w, P, V, cnt = _exact(nq, nc)
  tracks, vlog, _ = LU.split_head(head, T, nc)
  h = _handle(spa3d, T, nc)
  B, Q = (1, nq) if form == 'head' else (B_SPLIT, Q_SPLIT)
  with _objective(lib, spa3d, h, o, w, B, Q):
    for denom in (2.0 ** 18, 0.0):
      res = (_head_loss(lib, spa3d, h, head, tgt, vis, denom, nc, T, outs=False) if form == 'head'
             else _split_loss(lib, spa3d, h, tracks, vlog, tgt, vis, denom, B, Q))
      D = denom if denom > 0 else cnt
      tot, pos, v = LU.loss3_from(o, P, V, D)
      print(f'  exact lane, {form} form, NC {nc}, denom {denom}: P {res["P"]} (exact {P}), V {res["V"]} (exact {V}), count {res["cnt"]} (exact {cnt})')
      assert res['flag'] == 0 and (res['P'], res['V'], res['cnt'], res['denom']) == (P, V, cnt, D)
      assert _same_bits(res['out'][1], pos) and _same_bits(res['out'][2], v) and _same_bits(res['out'][0], tot)
  assert cnt > 262144 and nq * T > LU.CAP


# ------------------------------------------------------------------------------------------------ (d) ragged spa3d_loss
@pytest.mark.parametrize('counts', [(2049, 1000), (0, 2049)])
def test_ragged_split_loss(lib, spa3d, counts):
  """padded rows hold NaN and change no bit; a NaN in a live row makes all three results NaN; one error of 1e8 on a visible point gives NaN (the accumulator's
  range guard) or a value within the gate -- never another finite number"""
  o, nc = LU.OBJECTIVES['e'], 3
  B, Q = B_SPLIT, Q_SPLIT
  head, tgt, vis, w = _random_case(B * Q, T, nc, True)
  tracks, vlog, _ = LU.split_head(head, T, nc)
  live = np.zeros((B, Q), dtype=bool)
  for b, q in enumerate(counts):
    live[b, :q] = True
  live = live.reshape(-1)
  pt, vt = LU.point_terms(o, tracks[live], vlog[live], tgt[live], vis[live], w[live], np.float64)
  ref = LU.numerators(pt, vt) + (LU.numerator_bound(pt), LU.numerator_bound(vt), float(vis[live].sum(dtype=np.float64)))
  h = _handle(spa3d, T, nc)

  def run(fill, edit=None):
    arrs = [a.copy() for a in (tracks, vlog, tgt, vis, w)]
    if edit:
      edit(*arrs)
    terms = LU.point_terms(o, *(a[live] for a in arrs), np.float64) if edit else None
    for a in arrs:
      a[~live] = fill
    with _objective(lib, spa3d, h, o, arrs[4], B, Q):
      return _split_loss(lib, spa3d, h, arrs[0], arrs[1], arrs[2], arrs[3], 0.0, B, Q, counts=counts), terms

  res, _ = run(float('nan'))
  _check_numerators(res, ref, o, f'ragged {counts}')
  other, _ = run(7.0)
  assert _same_bits(other['out'], res['out']) and (other['P'], other['V'], other['cnt']) == (res['P'], res['V'], res['cnt'])
  first = int(np.flatnonzero(live)[0])
  last = int(np.flatnonzero(live)[-1])

  def nan_live(tr, vl, tg, vi, ww):
    tr[last, T - 1, 1] = float('nan')
  bad, _ = run(float('nan'), nan_live)
  assert np.isnan(bad['out']).all() and bad['flag'] != 0
  t_vis = int(np.flatnonzero(vis[first] > 0)[0])

  def huge(tr, vl, tg, vi, ww):
    tr[first, t_vis, 0] = tg[first, t_vis, 0] + F32(1e8)
  big, (pt, vt) = run(float('nan'), huge)
  if np.isnan(big['out']).any():
    assert np.isnan(big['out']).all() and big['flag'] != 0
    print(f'  ragged {counts}: an error of 1e8 (weight {w[first, t_vis]:.3f}) trips the range guard: NaN')
  else:
    err, bound = abs(big['P'] - LU.numerators(pt, vt)[0]), LU.numerator_bound(pt)   # the gate of the random lane, on the edited inputs
    print(f'  ragged {counts}: an error of 1e8 (weight {w[first, t_vis]:.3f}) stays finite: |err| {err:.3e} (bound {bound:.3e})')
    assert err <= bound


# ------------------------------------------------------------------------------------------------ (e) head cotangent
def _cot_case(nq, nc, seed=5):
  head, tgt, vis, w = LU.draw_case(nq, T, nc, seed=seed)
  h = head.reshape(nq, 4, T)
  h[::3, 0, ::5] = tgt[::3, ::5, 0]   # prediction == target: sign(0) = 0
  vis[::3, ::5] = 1.0
  w[::3, ::5] = np.maximum(w[::3, ::5], F32(0.5))
  return h.reshape(nq, 4 * T), tgt, vis, w


@pytest.mark.parametrize('name,nc,nq', [('d', 3, NQ_HEAD), ('e', 3, 37), ('d', 2, 37), ('e', 2, 37), ('b', 3, 37)])
def test_dhead_fp32_elementwise(lib, spa3d, name, nc, nq):
  """|got - ref64| <= 8 2^-24 max(|ref|, K) for every entry; K = bce_weight max(1, beta) w / D on the visibility block (where sigmoid - y cancels), 0 elsewhere.
  The certainty block of the 2-D twin is exactly 0, and the weight plane reaches the visibility block."""
  o = LU.OBJECTIVES[name]
  head, tgt, vis, w = _cot_case(nq, nc)
  h = _handle(spa3d, T, nc)
  with _objective(lib, spa3d, h, o, w, nq, 1):
    res = _head_loss(lib, spa3d, h, head, tgt, vis, 0.0, nc, T, dt=torch.float32, outs=False)
  got = res['dhead'].numpy()
  ref, K = LU.head_cotangent(o, head, tgt, vis, w, T, nc, res['denom'], 1.0, np.float64)
  bad, ratio = LU.cotangent_report(got, ref, K, 'fp32')
  print(f'  dhead fp32, objective {name}, NC {nc}, nq {nq}: worst |err| / bound = {ratio:.3f}')
  assert bad == 0 and res['scale'] == 1.0
  g3 = got.reshape(nq, 4, T)
  if nc == 2:
    assert not g3[:, 3].any(), 'the certainty block carries no gradient'
  else:
    assert bool(g3[:, 3].any())
  now, _ = LU.head_cotangent(o, head, tgt, vis, None, T, nc, res['denom'], 1.0, np.float64)
  assert LU.cotangent_report(got, now, K, 'fp32')[0] > 0, 'without the weight plane the reference must differ: the plane is in the gradient'
  if o.position_kind == 0 and o.l1_weight > 0:
    assert not g3[::3, 0, ::5].any(), 'sign(0) = 0'


def _run16(lib, spa3d, precision, o, case, nc, denom, setting=None):
  head, tgt, vis, w = case
  h = _handle(spa3d, T, nc, precision)
  if setting is not None:
    assert lib.spa3d_set_option(h, b'loss_scale', float(setting)) == 0
  try:
    with _objective(lib, spa3d, h, o, w, head.shape[0], 1):
      return _head_loss(lib, spa3d, h, head, tgt, vis, denom, nc, T, dt=TORCH_DT[precision], outs=False)
  finally:
    if precision == 'fp16':
      lib.spa3d_set_option(h, b'loss_scale', -16.0)


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
@pytest.mark.parametrize('name,nc', [('e', 3), ('d', 2)])
def test_dhead_16bit_within_one_rounding_of_the_format(lib, spa3d, precision, name, nc):
  """the fp32 gate plus ONE rounding of the storage type: half an ulp, 2^-9 (bf16) / 2^-12 (fp16) of the power of two above the value (tests/loss_util.py
  rounding_allowance); fp16 runs at the scale the call reports in loss3[11]; the certainty block is exactly 0"""
  o = LU.OBJECTIVES[name]
  case = _cot_case(37, nc)
  res = _run16(lib, spa3d, precision, o, case, nc, 0.0)
  got = res['dhead'].double().numpy()
  ref, K = LU.head_cotangent(o, case[0], case[1], case[2], case[3], T, nc, res['denom'], res['scale'], np.float64)
  bad, ratio = LU.cotangent_report(got, ref, K, precision)
  print(f'  dhead {precision}, objective {name}, NC {nc}: scale {res["scale"]}, worst |err| / bound = {ratio:.3f}')
  assert bad == 0
  assert res['scale'] == (LU.loss_scale_ref(res['denom'], float(LU.gmax(o, nc)), -16.0) if precision == 'fp16' else 1.0)
  if nc == 2:
    assert not got.reshape(-1, 4, T)[:, 3].any()


@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'fp16'])
def test_dhead_exact_sublane_and_fp16_overflow(lib, spa3d, precision):
  """default objective, no weights, power-of-two denominator and scale: position entries are +-5000 y scale / denom rounded once to the storage type, bit for
  bit, 0 where prediction == target or y = 0; an entry whose fp32 value overflows fp16 is +-inf"""
  nc, nq = 3, 37
  head, tgt, vis, _ = _cot_case(nq, nc)
  dt = TORCH_DT[precision]
  for denom, setting in ((1024.0, 64.0), (1.0, 1024.0)):
    res = _run16(lib, spa3d, precision, LU.Obj(), (head, tgt, vis, None), nc, denom, setting if precision == 'fp16' else None)
    scale = setting if precision == 'fp16' else 1.0
    assert res['scale'] == scale and res['denom'] == denom
    d = head.reshape(nq, 4, T)[:, :3] - tgt.transpose(0, 2, 1)
    want = torch.from_numpy((np.sign(d) * vis[:, None, :] * F32(5000.0 * scale / denom)).astype(F32)).to(dt)
    got = res['dhead'].reshape(nq, 4, T)[:, :3].contiguous()
    assert torch.equal(got.view(torch.int16) if dt != torch.float32 else got.view(torch.int32), want.view(torch.int16) if dt != torch.float32 else want.view(torch.int32))
    assert bool((want == 0).any()) and bool((want != 0).any())
    if precision == 'fp16' and 5000.0 * scale / denom > 65504:
      assert bool(torch.isinf(got[want != 0]).all()) and bool((got[want == 0] == 0).all())


# ------------------------------------------------------------------------------------------------ (f) loss scale
def _scale_of(lib, spa3d, h, denom):
  one = np.ones((1, 4), dtype=F32)
  return _head_loss(lib, spa3d, h, one, np.zeros((1, 1, 3), dtype=F32), np.ones((1, 1), dtype=F32), denom, 3, 1, outs=False)['scale']


def test_loss_scale_at_every_power_of_two_boundary(lib, spa3d):
  """fp16 handle, setting -16, the denominator passed: loss3[11] against the frexp reference at q = 2^k (k = 0 .. 24), at both fp32 neighbours of each and at
  five everyday denominators, for g_max = 5000 and g_max = 1"""
  h = _handle(spa3d, 1, 3, 'fp16')
  assert lib.spa3d_set_option(h, b'loss_scale', -16.0) == 0
  misses = []
  for o in (LU.Obj(), LU.UNIT_GMAX):
    gm = float(LU.gmax(o))
    with _objective(lib, spa3d, h, o, None, 1, 1):
      for d in LU.loss_scale_denoms(gm):
        got, want = _scale_of(lib, spa3d, h, d), LU.loss_scale_ref(d, gm, -16.0)
        if got != want:
          misses.append((gm, d, got, want))
  print(f'  loss scale: {len(misses)} of 160 points off the frexp reference' + ''.join(f'\n    g_max {g}: denom {d!r}: {a} (reference {b})' for g, d, a, b in misses))
  assert not misses


def test_loss_scale_fixed_setting_and_state(lib, spa3d):
  """a fixed setting is the scale; a registered state multiplies it when it lies in (0, 1), floored at 2^-24; 0, 1 and 2 are ignored.  A handle whose setting is
  exactly 1 runs unscaled whatever the state (the train call launches no scale kernel then): loss3[11] = 1."""
  h = _handle(spa3d, 1, 3, 'fp16')
  state = torch.zeros(1, device='cuda')
  try:
    assert lib.spa3d_set_option(h, b'loss_scale', 1024.0) == 0
    assert _scale_of(lib, spa3d, h, 100.0) == 1024.0
    assert lib.spa3d_set_loss_scale_state(h, state.data_ptr()) == 0
    for s, want in ((0.25, 256.0), (0.0, 1024.0), (1.0, 1024.0), (2.0, 1024.0), (2.0 ** -30, 2.0 ** -20)):
      state.fill_(s)
      assert _scale_of(lib, spa3d, h, 100.0) == want == LU.loss_scale_ref(100.0, 5000.0, 1024.0, s), (s, want)
    state.fill_(2.0 ** -30)
    assert lib.spa3d_set_option(h, b'loss_scale', 2.0) == 0
    assert _scale_of(lib, spa3d, h, 100.0) == 2.0 ** -24 == LU.loss_scale_ref(100.0, 5000.0, 2.0, 2.0 ** -30)
    assert lib.spa3d_set_option(h, b'loss_scale', 1.0) == 0
    assert _scale_of(lib, spa3d, h, 100.0) == 1.0
    assert lib.spa3d_set_option(h, b'loss_scale', -16.0) == 0
    state.fill_(0.5)
    assert _scale_of(lib, spa3d, h, 2.56e6) == 4096.0
  finally:
    lib.spa3d_set_loss_scale_state(h, None)
    lib.spa3d_set_option(h, b'loss_scale', -16.0)


# ------------------------------------------------------------------------------------------------ (g) AdamW
def _flat(n, name):
  """n floats in a guarded allocation, laid out as r rows for the largest divisor r <= 4096 of n: the guard's tail is 384 rows, and a [1, n] view of 2^20
  elements would carry 1.6 GB of canary"""
  rows = max(r for r in range(1, 4097) if n % r == 0)
  return PU.guarded(rows, n // rows, torch.float32, name=name).reshape(-1)


def _adamw(lib, spa3d, state, entry, step=7, lr=3e-4, clip=1.0, groups=None):
  """one optimizer call on guarded copies -> (p, m, v, scratch[:6]) on the host"""
  p, g, m, v = (_flat(t.size, nm) for t, nm in zip(state, 'pgmv'))
  for d, t in zip((p, g, m, v), state):
    d.copy_(torch.from_numpy(np.ascontiguousarray(t)))
  n = p.numel()
  scratch = PU.guarded(1, 1024, torch.float32, name='scratch', fill=0.0)[0]
  if entry == 'plain':
    rc = lib.spa3d_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, step, clip, 0.9, 0.999, 1e-8, 0.01, scratch.data_ptr(), _s())
  else:
    groups = groups or []
    tab = (spa3d._lib.ParamGroup * max(len(groups), 1))(*[spa3d._lib.ParamGroup(*r) for r in groups])
    nb = lib.spa3d_adamw_groups_workspace_bytes(len(groups))
    ws = PU.guarded(1, max(nb, 4) // 4, torch.float32, name='ws')[0]
    rc = lib.spa3d_adamw_step_groups(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, step, clip, 0.9, 0.999, 1e-8, 0.01, tab if groups else None,
                                     len(groups), None, 0.0, scratch.data_ptr(), ws.data_ptr() if groups else None, nb, _s())
  assert rc == 0
  torch.cuda.synchronize()
  out = (p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), scratch[:6].cpu().numpy())
  PU.check_guards()
  return out


def _six_ranges(n):
  """six ranges with gaps: two frozen ones (the first element, the last four), learning-rate scales 0.1 / 1 / 10, weight-decay scales 0 / 1 / 3; the fifth
  runs across index 2^20 when n does"""
  return [(0, 1, 0.0, 1.0), (1, 5, 0.1, 3.0), (7, 263, 1.0, 0.0), (263, 1000, 10.0, 1.0), (1003, n - 10, 0.1, 3.0), (n - 4, n, 0.0, 0.0)]


ENTRIES = ['plain', 'groups', 'table']


def _adamw_all(lib, spa3d, state, entries=ENTRIES, **kw):
  n = state[0].size
  return {e: _adamw(lib, spa3d, state, 'plain' if e == 'plain' else 'groups', groups=_six_ranges(n) if e == 'table' else None, **kw) for e in entries}


def _adamw_ref(state, entry, step=7, lr=3e-4, clip=1.0):
  """tests/optim_util.py's float64 restatement of the call -> (p, m, v, norm)"""
  P, G, M, V = (torch.from_numpy(np.ascontiguousarray(t)).double().clone() for t in state)
  gn, skip = OU.adamw_groups_step(P, G, M, V, step, lr, clip=clip, groups=_six_ranges(P.numel()) if entry == 'table' else ())
  assert not skip
  return P.numpy(), M.numpy(), V.numpy(), gn


def _adamw_gate(got, ref, what):
  e = LU.adamw_errs(got, ref)
  en = abs(float(got[3][0]) - ref[3]) / max(ref[3], 1e-300)
  print(f'  {what}: max |err| p {e[0]:.3e} (gate 1e-6), m {e[1]:.3e} (1e-7), v {e[2]:.3e} (1e-9), norm {en:.3e} relative (1e-5)')
  assert e[0] < 1e-6 and e[1] < 1e-7 and e[2] < 1e-9 and en <= 1e-5, what


def _state(n, seed=5):
  r = np.random.default_rng(seed)
  return (r.standard_normal(n).astype(F32), (r.standard_normal(n) * 0.01).astype(F32), (r.standard_normal(n) * 0.001).astype(F32), (r.random(n) * 1e-4).astype(F32))


def test_adamw_past_the_update_kernels_grid_cap(lib, spa3d):
  n = LU.CAP + 257
  state = _state(n)
  res = _adamw_all(lib, spa3d, state)
  for e in ENTRIES:
    _adamw_gate(res[e], _adamw_ref(state, e), f'n = 2^20 + 257, {e}')
    moved = res[e][1] != state[2]   # the first moment: 0.9 m + 0.1 g differs from m wherever the element was processed
    if e == 'table':
      assert moved[LU.CAP - 300:LU.CAP + 247].all() and not moved[-4:].any() and not moved[0], 'the range across index 2^20 moved, the frozen ends did not'
    else:
      assert moved[:LU.CAP].all() and moved[LU.CAP:].all(), 'elements on both sides of index 2^20 moved'
  assert max(LU.adamw_errs(_adamw_ref(state, 'plain'), LU.adamw_ref(*state, step=7, lr=3e-4))) < 1e-12   # the two float64 statements agree
  for k in range(4):
    assert _same_bits(res['groups'][k], res['plain'][k]), 'plain and groups (no table) are bit-equal'


def test_adamw_unclipped_and_norm_equal_to_clip(lib, spa3d):
  n = 4099
  p, g, m, v = _state(n)
  gs = (g * F32(0.5 / math.sqrt(float((g.astype(np.float64) ** 2).sum())))).astype(F32)
  for e, r in _adamw_all(lib, spa3d, (p, gs, m, v)).items():
    ref = _adamw_ref((p, gs, m, v), e, clip=float('inf'))   # the update must be that of clip = infinity
    assert ref[3] < 1.0
    _adamw_gate(r, ref, f'unclipped lane, {e}')
  gu = LU.unit_norm_gradient(n)
  ref = _adamw_ref((p, gu, m, v), 'plain', clip=float('inf'))
  for e, r in _adamw_all(lib, spa3d, (p, gu, m, v), entries=('plain', 'groups')).items():
    assert float(r[3][0]) == 1.0, 'the norm of 4^k entries of 2^-k is exactly 1'
    _adamw_gate(r, ref, f'norm == clip, {e}')
    mi = F32(0.9) * m + F32(F32(1.0) - F32(0.9)) * gu   # sc = 1 exactly: the first moment is that of the unscaled gradient, bit for bit
    assert _same_bits(r[1], mi)


def test_adamw_small_state_and_zero_state(lib, spa3d):
  n = 4099
  ps, gsm, ms, vs = LU.small_state(n, seed=9)
  wrong = LU.adamw_ref(ps, gsm, ms, vs, step=7, lr=1e-2, variant='eps_inside')
  assert LU.adamw_errs(wrong, _adamw_ref((ps, gsm, ms, vs), 'plain', lr=1e-2))[0] > 1e-4
  for e, r in _adamw_all(lib, spa3d, (ps, gsm, ms, vs), lr=1e-2).items():
    _adamw_gate(r, _adamw_ref((ps, gsm, ms, vs), e, lr=1e-2), f'small-state lane, {e}')
  z = np.zeros(n, dtype=F32)
  for e, r in _adamw_all(lib, spa3d, (ps, z, z, z), entries=('plain', 'groups'), step=0).items():
    assert _same_bits(r[0], ps - F32(3e-4) * (F32(0.0) + F32(0.01) * ps)) and not r[1].any() and not r[2].any() and float(r[3][0]) == 0.0, e


@pytest.mark.parametrize('entry', ['plain', 'groups'])
def test_adamw_guard_sequence(lib, spa3d, entry):
  """n = 1, call by call against the state machine restated from the header (tests/loss_util.py Guard): scratch[2..5] after every call; after a skipped call
  p, m, v keep their bits; every applied step is that of the float64 reference with the bias correction at step + 1 - skipped"""
  p, g, m, v = (PU.guarded(1, 1, torch.float32, name=nm, fill=0.0)[0] for nm in 'pgmv')
  scratch = PU.guarded(1, 1024, torch.float32, name='scratch', fill=0.0)[0]
  p.fill_(1.0)
  INF, FIN = float('inf'), 0.01

  def call(step, grad):
    g.fill_(grad)
    if entry == 'plain':
      rc = lib.spa3d_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 1, 3e-4, step, 1.0, 0.9, 0.999, 1e-8, 0.01, scratch.data_ptr(), _s())
    else:
      rc = lib.spa3d_adamw_step_groups(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 1, 3e-4, step, 1.0, 0.9, 0.999, 1e-8, 0.01, None, 0, None, 0.0,
                                       scratch.data_ptr(), None, 0, _s())
    assert rc == 0
    return [float(x) for x in scratch[:6].cpu()], (float(p), float(m), float(v))

  def run(seq, start=(0.0, 0.0)):
    scratch.zero_(); scratch[4], scratch[5] = start
    p.fill_(1.0); m.zero_(); v.zero_()
    guard = LU.Guard(*start)
    ref = [np.array([1.0]), np.array([0.0]), np.array([0.0])]
    skipped, trace = 0, []
    for step, fin in enumerate(seq):
      before = (float(p), float(m), float(v))
      s, after = call(step, FIN if fin else INF)
      want = guard.step(fin)
      assert s[2:] == want, (step, s, want)
      if fin:
        out = LU.adamw_ref(ref[0], np.array([FIN]), ref[1], ref[2], step=step, lr=3e-4, skipped=skipped)
        ref = list(out[:3])
        assert abs(after[0] - float(ref[0][0])) < 1e-6 and abs(after[1] - float(ref[1][0])) < 1e-7 and abs(after[2] - float(ref[2][0])) < 1e-9, (step, after, ref)
        assert abs(s[0] - FIN) <= 1e-5 * FIN
      else:
        skipped += 1
        assert after == before and s[0] == INF, 'a skipped call keeps p, m and v'
      trace.append(want[2])
    return trace

  tr = run([False] + [True] * 200 + [False, False] + [True] * 400)
  assert tr[0] == 0.5 and tr[199] == 0.5 and tr[200] == 1.0 and tr[202] == 0.25 and tr[402] == 0.5 and tr[401] == 0.25 and tr[602] == 1.0 and tr[601] == 0.5
  for start in (0.3, 2.0 ** -25):
    assert run([True], (start, 0.0)) == [1.0] and run([False], (start, 0.0)) == [0.5]
  assert run([False, False], (2.0 ** -24, 0.0)) == [2.0 ** -24, 2.0 ** -24]
  assert run([True, False, True], (0.5, 150.0)) == [0.5, 0.25, 0.25]   # a skip in the middle of counting resets the counter (compared call by call above)
  PU.check_guards()


# ------------------------------------------------------------------------------------------------ (h) noise
@pytest.mark.parametrize('key', [(0, 0), (1, 2), (0xFFFFFFFF, 0x9E3779B9)])
def test_uniform_noise_bits(lib, key):
  from oracle import np_blocks as NB
  for n in (1, 2, 255, 256, 65536, 65537):
    out = PU.guarded(1, n, torch.float32, name='noise')[0]
    assert lib.spa3d_uniform_noise(out.data_ptr(), n, key[0], key[1], _s()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    PU.check_guards()
    assert _same_bits(got, NB.jax_uniform_legacy((n,), key)), (n, key)
