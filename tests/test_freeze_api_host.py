"""CPU-side checks of the "freeze" option (include/spa3d.h, spa3d_set_option): which values are taken, the trainable range it implies against
spa3d_grad_segments for both model kinds, and the dry-run workspace sizing of a training call at B = 1, N = 2048, Q = 512, T = 150.
No compute call is made (no GPU here)."""
import ctypes as C

import pytest

from util import MINI, O, product_model

N, Q, T = 2048, 512, 150


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


def _segments(lib, h):
  b4 = (C.c_int64 * 4)()
  assert lib.spa3d_grad_segments(h, b4) == 0
  return [int(x) for x in b4]


def _range(lib, h):
  r = (C.c_int64 * 2)()
  assert lib.spa3d_trainable_range(h, r) == 0
  return [int(x) for x in r]


def _mini_handles(spa3d):
  m3 = product_model(spa3d, O.Config(**MINI, use_dino=False, use_depth=False), 'fp32')
  from test_trajan2d import MINI2D, _model
  m2 = _model(spa3d, O.config_2d(**MINI2D), 'fp32')
  return [('3-D mini', m3, m3._handle(0, 0)[0]), ('2-D twin', m2, m2._handle(0, 0)[0])]


def test_option_values(spa3d):
  lib = spa3d._lib.load()
  h = _mini_handles(spa3d)[0][2]
  for v in (0.0, 1.0, 2.0):
    assert lib.spa3d_set_option(h, b'freeze', v) == 0, lib.spa3d_last_error(h)
  seg = _segments(lib, h)
  assert _range(lib, h) == [seg[2], seg[3]]
  for v in (-1.0, 3.0, 0.5):
    assert lib.spa3d_set_option(h, b'freeze', v) == 1, v
    assert b'freeze' in lib.spa3d_last_error(h)
    assert _range(lib, h) == [seg[2], seg[3]], 'a refused value must leave the stored one alone'
  assert lib.spa3d_set_option(h, b'freeze', 0.0) == 0


def test_trainable_range_follows_the_option(spa3d):
  lib = spa3d._lib.load()
  for name, _, h in _mini_handles(spa3d):
    seg = _segments(lib, h)
    assert 0 < seg[1] < seg[2] < seg[3], (name, seg)
    assert _range(lib, h) == [0, seg[3]], name  # never set: nothing frozen
    for k in (0, 1, 2):
      assert lib.spa3d_set_option(h, b'freeze', float(k)) == 0
      assert _range(lib, h) == [seg[k], seg[3]], (name, k)
      assert spa3d.model.trainable_range(h) == (seg[k], seg[3])
    assert lib.spa3d_set_option(h, b'freeze', 0.0) == 0
    assert lib.spa3d_trainable_range(h, None) == 1 and lib.spa3d_trainable_range(None, (C.c_int64 * 2)()) == 1


def test_python_aliases_and_restore(spa3d):
  lib = spa3d._lib.load()
  _, m, h = _mini_handles(spa3d)[0]
  seg = _segments(lib, h)
  assert [spa3d.model.freeze_level(a) for a in ('none', 'encoder', 'encoder+latents', 0, 1, 2)] == [0, 1, 2, 0, 1, 2]
  for bad in (3, -1, 0.5, True, 'latents', None):
    with pytest.raises(ValueError):
      spa3d.model.freeze_level(bad)
  # the per-call statement puts back what it found: a preset survives a call made with another value
  assert lib.spa3d_set_option(h, b'freeze', 1.0) == 0
  with spa3d.model._freeze_on(h, 2):
    assert _range(lib, h)[0] == seg[2]
  assert _range(lib, h)[0] == seg[1]
  with spa3d.model._freeze_on(h, 'none'):
    assert _range(lib, h)[0] == 0
  assert _range(lib, h)[0] == seg[1]
  assert lib.spa3d_set_option(h, b'freeze', 0.0) == 0


@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_dry_run_workspace_falls_with_the_frozen_stages(spa3d, precision):
  lib = spa3d._lib.load()
  m = spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=768, depth_feature_dim=1, precision=precision)
  h = m._handle(768, 1)[0]

  def need(k, train=1):
    assert lib.spa3d_set_option(h, b'freeze', float(k)) == 0
    return lib.spa3d_workspace_bytes(h, 1, N, Q, T, 1, train)

  fwd = need(0, 0)
  w = [need(k) for k in (0, 1, 2)]
  print(f'{precision} B = 1, N = {N}, Q = {Q}, T = {T}: training need {w[0] / 1e9:.2f} GB unfrozen, {w[1] / 1e9:.2f} GB freeze 1, '
        f'{w[2] / 1e9:.2f} GB freeze 2; forward only {fwd / 1e9:.2f} GB')
  assert w[0] > w[1] > w[2] >= fwd > 0
  assert need(2, 0) == need(1, 0) == fwd, 'only the training call reads the option'
  # "track_chunk" already keeps no encoder stash in the forward: freezing the encoder drops pass B, never adds to the need
  assert lib.spa3d_set_option(h, b'track_chunk', 512.0) == 0
  tc = [need(k) for k in (0, 1, 2)]
  print(f'{precision} with track_chunk 512: {tc[0] / 1e9:.2f} / {tc[1] / 1e9:.2f} / {tc[2] / 1e9:.2f} GB')
  assert tc[1] <= tc[0] and tc[2] <= tc[1]
  assert lib.spa3d_set_option(h, b'track_chunk', 0.0) == 0
  # back at 0 the handle sizes as one that never froze
  h0 = spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=768, depth_feature_dim=1, precision=precision)._handle(768, 1)[0]
  assert need(0) == lib.spa3d_workspace_bytes(h0, 1, N, Q, T, 1, 1)
