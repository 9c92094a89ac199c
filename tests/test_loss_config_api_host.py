"""The configurable objective at the C-ABI and in the Python mirror, on the CPU (no compute call): struct layout, set / get / reset, every
refusal of spa3d_set_loss with its message and the stored configuration left in place, the shape check of spa3d_set_point_weights before any
launch, and LossConfig raising ValueError on the same inputs."""
import ctypes as C
import dataclasses
import math

import pytest
import torch

INF, NAN = float('inf'), float('nan')
# (fields that differ from the defaults, a word of the library's message); NC = 3
REFUSED = [
    (dict(l1_weight=NAN), b'finite'), (dict(bce_weight=INF), b'finite'), (dict(bce_pos_weight=NAN), b'finite'),
    (dict(axis_weight=(1.0, INF, 1.0)), b'finite'), (dict(position_kind=1, huber_delta=NAN), b'finite'),
    (dict(l1_weight=-1.0), b'negative'), (dict(bce_weight=-1e-8), b'negative'), (dict(axis_weight=(1.0, 1.0, -0.5)), b'negative'),
    (dict(bce_pos_weight=-1.0), b'negative'),
    (dict(position_kind=2), b'position_kind'), (dict(position_kind=-1), b'position_kind'),
    (dict(position_kind=1, huber_delta=0.0), b'huber_delta'), (dict(position_kind=1, huber_delta=-1.0), b'huber_delta'),
    (dict(axis_weight=(0.0, 0.0, 0.0)), b'axis_weight'),
    (dict(l1_weight=0.0, bce_weight=0.0), b'2^30'), (dict(l1_weight=2.0 ** 31), b'2^30'), (dict(l1_weight=0.0, bce_weight=2.0 ** 29, bce_pos_weight=4.0), b'2^30'),
]
ACCEPTED = [
    dict(l1_weight=1.0, bce_weight=1.0), dict(l1_weight=0.0, bce_weight=1.0, bce_pos_weight=3.0),
    dict(position_kind=1, huber_delta=1.0, axis_weight=(1.0, 0.5, 0.25)), dict(l1_weight=2.0 ** 30, bce_weight=0.0),
    dict(huber_delta=NAN),  # read with HUBER only
    dict(l1_weight=0.0, bce_weight=0.5, axis_weight=(0.0, 0.0, 0.0)),  # no position term: no axis weight is needed
]


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


def _struct(spa3d, **kw):
  s = spa3d._lib.LossConfig(5000.0, 1e-8, 0, 1.0, (C.c_float * 3)(1.0, 1.0, 1.0), 1.0)
  for k, v in kw.items():
    setattr(s, k, (C.c_float * 3)(*v) if k == 'axis_weight' else v)
  return s


def _fields(s):
  return (s.l1_weight, s.bce_weight, s.position_kind, s.huber_delta, tuple(s.axis_weight), s.bce_pos_weight)


def _same(a, b):
  return all((x == y) or (isinstance(x, float) and math.isnan(x) and math.isnan(y)) for x, y in zip(_fields(a)[:4] + _fields(a)[4] + _fields(a)[5:], _fields(b)[:4] + _fields(b)[4] + _fields(b)[5:]))


def _handle(spa3d, two_d=False):
  m = spa3d.TrackAutoEncoder(num_output_frames=8, precision='fp32') if two_d else spa3d.TrackAutoEncoder3D(num_output_frames=8, use_dino=False, use_depth=False, precision='fp32')
  return m, m._handle(0, 0)[0]


def test_struct_layout_matches_the_header(spa3d):
  S = spa3d._lib.LossConfig
  assert (S.l1_weight.offset, S.bce_weight.offset, S.position_kind.offset, S.huber_delta.offset, S.axis_weight.offset, S.bce_pos_weight.offset) == (0, 4, 8, 12, 16, 28)
  assert S.axis_weight.size == 12 and C.sizeof(S) == 32
  assert (spa3d.POS_L1, spa3d.POS_HUBER) == (0, 1)


def test_set_get_reset(spa3d):
  lib = spa3d._lib.load()
  _, h = _handle(spa3d)
  got = spa3d._lib.LossConfig()
  assert lib.spa3d_get_loss(h, C.byref(got)) == 0 and _same(got, _struct(spa3d))
  for kw in ACCEPTED:
    want = _struct(spa3d, **kw)
    assert lib.spa3d_set_loss(h, C.byref(want)) == 0, (kw, lib.spa3d_last_error(h))
    assert lib.spa3d_get_loss(h, C.byref(got)) == 0 and _same(got, want), kw
  assert lib.spa3d_set_loss(h, None) == 0
  assert lib.spa3d_get_loss(h, C.byref(got)) == 0 and _same(got, _struct(spa3d))
  assert lib.spa3d_set_loss(None, None) == 1 and lib.spa3d_get_loss(h, None) == 1 and lib.spa3d_get_loss(None, C.byref(got)) == 1


@pytest.mark.parametrize('kw,word', REFUSED)
def test_every_refusal_keeps_the_stored_configuration(spa3d, kw, word):
  lib = spa3d._lib.load()
  _, h = _handle(spa3d)
  kept = _struct(spa3d, l1_weight=2.0, bce_weight=0.5, position_kind=1, huber_delta=0.75, axis_weight=(1.0, 0.5, 0.25), bce_pos_weight=3.0)
  assert lib.spa3d_set_loss(h, C.byref(kept)) == 0
  bad = _struct(spa3d, **kw)
  assert lib.spa3d_set_loss(h, C.byref(bad)) == 1
  msg = lib.spa3d_last_error(h)
  assert msg.startswith(b'spa3d_set_loss') and word in msg, msg
  got = spa3d._lib.LossConfig()
  assert lib.spa3d_get_loss(h, C.byref(got)) == 0 and _same(got, kept)
  assert lib.spa3d_set_loss(h, None) == 0
  with pytest.raises(ValueError):
    spa3d.LossConfig(**kw)


def test_the_2d_twin_reads_two_axis_weights(spa3d):
  lib = spa3d._lib.load()
  _, h2 = _handle(spa3d, two_d=True)
  _, h3 = _handle(spa3d)
  only_z = _struct(spa3d, axis_weight=(0.0, 0.0, 1.0))
  assert lib.spa3d_set_loss(h3, C.byref(only_z)) == 0 and lib.spa3d_set_loss(h3, None) == 0
  assert lib.spa3d_set_loss(h2, C.byref(only_z)) == 1 and b'axis_weight' in lib.spa3d_last_error(h2)
  z_nan = _struct(spa3d, axis_weight=(1.0, 1.0, NAN))   # the third entry is not read
  assert lib.spa3d_set_loss(h2, C.byref(z_nan)) == 0 and lib.spa3d_set_loss(h2, None) == 0
  assert lib.spa3d_set_loss(h3, C.byref(z_nan)) == 1
  cfg = spa3d.LossConfig(axis_weight=(0.0, 0.0, 1.0))
  assert cfg.validate(3) is cfg
  with pytest.raises(ValueError):
    cfg.validate(2)


def test_loss_config_dataclass(spa3d):
  d = spa3d.LossConfig()
  assert dataclasses.astuple(d) == (5000.0, 1e-8, 0, 1.0, (1.0, 1.0, 1.0), 1.0)
  assert _same(d.as_struct(), _struct(spa3d))
  for kw in ACCEPTED:
    assert _same(spa3d.LossConfig(**kw).as_struct(), _struct(spa3d, **kw))
  with pytest.raises(ValueError):
    spa3d.LossConfig(axis_weight=(1.0, 1.0))
  with pytest.raises(ValueError):
    spa3d.LossConfig(l1_weight=1e39)   # finite in Python, not in the library's float32


def test_point_weights_for_another_shape_are_refused_before_any_launch(spa3d):
  lib = spa3d._lib.load()
  _, h = _handle(spa3d)
  fake = 0x100000  # never dereferenced: every call below returns before its first launch
  b = spa3d._lib.Batch()
  b.B, b.Q = 2, 3
  b.query_tracks, b.query_tracks_visible = fake, fake
  out = spa3d._lib.Outputs(fake, fake, None, None)
  assert lib.spa3d_set_point_weights(h, 0, 3, fake) == 1 and lib.spa3d_set_point_weights(h, 2, 0, fake) == 1
  assert lib.spa3d_set_point_weights(None, 2, 3, fake) == 1
  for B, Q in ((3, 3), (2, 4)):
    assert lib.spa3d_set_point_weights(h, B, Q, fake) == 0
    assert lib.spa3d_loss(h, C.byref(b), C.byref(out), 0.0, fake, None) == 1
    msg = lib.spa3d_last_error(h)
    assert b'point weights were set for' in msg and f'B = {B}, Q = {Q}'.encode() in msg, msg
    # the train call as well: refused before the batch's other tensors are looked at
    b.N, b.T = 4, 8
    b.support_tracks = b.support_tracks_visible = b.query_points = b.boundary_frame = fake
    assert lib.spa3d_loss_and_grads(h, fake, C.byref(b), 0.0, fake, 0, fake, None, fake, 0, None) == 1
    assert b'point weights were set for' in lib.spa3d_last_error(h)
  assert lib.spa3d_set_point_weights(h, 0, 0, None) == 0   # detach: B and Q are ignored
  assert lib.spa3d_loss_and_grads(h, fake, C.byref(b), 0.0, fake, 0, fake, None, fake, 0, None) == 2   # only the workspace is missing now


def test_op_head_loss_refusals_before_any_launch(spa3d):
  """spa3d_op_head_loss: a NULL required pointer, a negative row count, a misaligned loss3 and a weight plane stated for another row count are
  SPA3D_ERR_ARG with a message; nq == 0 is SPA3D_OK.  No call here reaches a launch."""
  lib = spa3d._lib.load()
  _, h = _handle(spa3d)
  fake = 0x100000  # never dereferenced
  out = spa3d._lib.Outputs(fake, fake, fake, None)
  call = lambda head=fake, nq=4, tgt=fake, vis=fake, loss3=fake, handle=h: lib.spa3d_op_head_loss(handle, head, nq, tgt, vis, 0.0, C.byref(out), loss3, fake, None)
  for kw in (dict(head=None), dict(tgt=None), dict(vis=None), dict(loss3=None)):
    assert call(**kw) == 1 and lib.spa3d_last_error(h).startswith(b'op_head_loss') and b'required' in lib.spa3d_last_error(h), kw
  assert call(handle=None) == 1
  assert call(nq=-1) == 1 and b'negative' in lib.spa3d_last_error(h)
  assert call(loss3=fake + 4) == 1 and b'8-byte aligned' in lib.spa3d_last_error(h)
  assert call(nq=0) == 0 and lib.spa3d_last_error(h) == b''
  assert lib.spa3d_op_head_loss(h, fake, 0, fake, fake, 0.0, None, fake, None, None) == 0   # out and dhead are optional
  assert lib.spa3d_set_point_weights(h, 2, 3, fake) == 0
  try:
    for nq in (5, 7, 0):
      assert call(nq=nq) == 1
      msg = lib.spa3d_last_error(h)
      assert b'point weights were set for B = 2, Q = 3' in msg and f'nq = {nq}'.encode() in msg, msg
  finally:
    assert lib.spa3d_set_point_weights(h, 0, 0, None) == 0
  assert call(nq=0) == 0
  # counts on the handle are ignored: the call does not look at them
  assert lib.spa3d_set_counts(h, 3, None, (C.c_int32 * 3)(1, 2, 3)) == 0
  try:
    assert call(nq=0) == 0 and call(nq=-2) == 1
  finally:
    assert lib.spa3d_set_counts(h, 0, None, None) == 0


def test_cpu_tensors_are_refused(spa3d):
  preds = spa3d.TrackAutoEncoderResults(torch.zeros(2, 3, 8, 3), torch.zeros(2, 3, 8, 1), torch.zeros(2, 3, 8, 1))
  batch = {'query_tracks': torch.zeros(2, 3, 8, 3), 'query_tracks_visible': torch.ones(2, 3, 8, 1), 'query_weight': torch.ones(2, 3, 8)}
  with pytest.raises(spa3d._lib.Spa3dError):
    spa3d.compute_loss_3d(preds, batch, loss=spa3d.LossConfig(l1_weight=1.0, bce_weight=1.0))
  with pytest.raises(spa3d._lib.Spa3dError):
    spa3d.compute_loss_2d(spa3d.TrackAutoEncoderResults(torch.zeros(2, 3, 8, 2), torch.zeros(2, 3, 8, 1), torch.zeros(2, 3, 8, 1)),
                          {'query_tracks': torch.zeros(2, 3, 8, 2), 'query_tracks_visible': torch.ones(2, 3, 8, 1)}, loss=spa3d.LossConfig())


def test_collate_ragged_pads_query_weight(spa3d):
  mk = lambda n, q: {'support_tracks': torch.zeros(n, 8, 3), 'support_tracks_visible': torch.ones(n, 8, 1), 'query_points': torch.zeros(q, 4),
                     'query_tracks': torch.zeros(q, 8, 3), 'query_tracks_visible': torch.ones(q, 8, 1), 'query_weight': torch.full((q, 8), 0.5), 'boundary_frame': 8}
  batch = spa3d.collate_ragged([mk(4, 3), mk(2, 1)], pad_value=NAN)
  w = batch['query_weight']
  assert w.shape == (2, 3, 8) and bool((w[0] == 0.5).all()) and bool((w[1, :1] == 0.5).all()) and bool(torch.isnan(w[1, 1:]).all())
  parts = spa3d.split_ragged({'query_weight': w}, batch)
  assert [p['query_weight'].shape[0] for p in parts] == [3, 1]
