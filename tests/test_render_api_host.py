"""The boundary of spa3d_render_tracks on the CPU (no compute call): the ctypes layout of spa3d_render against the header, every refusal of the
entry point -- each SPA3D_ERR_ARG with a message, before any launch -- the workspace sizing, and the Python wrappers' own refusals (CPU
tensors, shapes)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x100000  # never dereferenced: every call below is refused before its first launch


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


@pytest.fixture(scope='module')
def handle(spa3d):
  return spa3d.TrackAutoEncoder3D(num_output_frames=8, use_dino=False, use_depth=False, precision='fp32')._handle(0, 0)[0]


def good(spa3d, coords=2):
  r = spa3d._lib.Render()
  r.N, r.T, r.H, r.W, r.coords = 5, 4, 30, 40, coords
  r.video = r.out = r.tracks = r.scores = FAKE
  if coords == 3:
    r.intrinsics = r.extrinsics = FAKE
    r.resize_h = r.resize_w = 1024
  r.normalize, r.trail, r.point_size = 1, 5, 2
  return r


def test_struct_matches_the_header(spa3d):
  hdr = open(os.path.join(ROOT, 'include', 'spa3d.h')).read()
  body = re.search(r'typedef struct \{((?:(?!typedef struct).)*?)\} spa3d_render;', hdr, re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  names = []
  for decl in body.split(';'):
    decl = decl.strip()
    if not decl:
      continue
    first, *rest = decl.split(',')
    ptr = '*' in first
    ctype = 'ptr' if ptr else first.split()[0]
    for n in [first.split()[-1].lstrip('*')] + [x.strip() for x in rest]:
      names.append((n, ctype))
  fields = spa3d._lib.Render._fields_
  assert [n for n, _ in names] == [n for n, _ in fields]
  for (n, ctype), (_, ft) in zip(names, fields):
    assert ft is (C.c_void_p if ctype == 'ptr' else C.c_int32), n
  assert C.sizeof(spa3d._lib.Render) == 120 and spa3d._lib.Render.pixels.offset == 112


def test_every_refusal_is_err_arg_with_a_message(spa3d, handle):
  lib = spa3d._lib.load()
  need = lib.spa3d_render_workspace_bytes(handle, 5, 4)
  call = lambda r, ws=FAKE, nb=None: lib.spa3d_render_tracks(handle, C.byref(r) if r is not None else None, ws, need if nb is None else nb, None)
  err = lambda: lib.spa3d_last_error(handle)

  def refused(word, coords=2, **fields):
    r = good(spa3d, coords)
    for k, v in fields.items():
      setattr(r, k, v)
    assert call(r) == 1 and word in err(), (fields, err())

  refused(b'tracks', tracks=None)
  refused(b'video', video=None)
  refused(b'scores', scores=None)
  refused(b'both NULL', out=None)                       # nothing asked for
  refused(b'visible', use_visibility=1)
  for c in (0, 1, 4, -3):
    refused(b'coords', coords=c)
  refused(b'camera', coords=3, intrinsics=None)
  refused(b'camera', coords=3, extrinsics=None)
  refused(b'resize', coords=3, resize_h=0)
  refused(b'resize', coords=3, resize_w=-1)
  for k, v in (('N', 0), ('T', 0), ('N', -1)):
    refused(b'positive', **{k: v})
  for k, v in (('H', 0), ('W', 0), ('H', 16385), ('W', 16385)):
    refused(b'16384', **{k: v})
  for v in (-1, 33):
    refused(b'trail', trail=v)
    refused(b'point_size', point_size=v)
  assert call(None) == 1 and err()
  assert lib.spa3d_render_tracks(None, C.byref(good(spa3d)), FAKE, need, None) == 1
  # the workspace: a missing or short one names the bytes needed, and the need is within spa3d_render_workspace_bytes
  for coords in (2, 3):
    r = good(spa3d, coords)
    assert call(r, FAKE, 0) == 1 and b'workspace too small' in err()
    asked = int(err().split(b'need ')[1].split()[0])
    assert 0 < asked <= need
    assert call(r, None, need) == 1 and b'workspace too small' in err()
    assert call(r, FAKE, asked - 1) == 1 and int(err().split(b'need ')[1].split()[0]) == asked
  r = good(spa3d, 3)
  r.out = r.video = r.scores = None
  r.pixels = FAKE                                          # positions only: no frames, no scores
  assert call(r, FAKE, 0) == 1 and b'workspace too small' in err() and int(err().split(b'need ')[1].split()[0]) <= 256


def test_workspace_bytes_is_monotone(spa3d, handle):
  lib = spa3d._lib.load()
  f = lambda n, t: lib.spa3d_render_workspace_bytes(handle, n, t)
  sizes = [f(n, 150) for n in (1, 2, 64, 512, 2048, 65536)]
  assert all(0 < a < b for a, b in zip(sizes, sizes[1:]))
  sizes = [f(2048, t) for t in (1, 2, 24, 150, 300, 10000)]
  assert all(0 < a < b for a, b in zip(sizes, sizes[1:]))
  assert f(2048, 150) >= 2048 * 150 * 20 and f(1 << 20, 1 << 12) > 1 << 36   # 64-bit sizes
  assert f(0, 4) == -1 and f(4, 0) == -1 and f(-1, 4) == -1 and lib.spa3d_render_workspace_bytes(None, 4, 4) == -1


def test_python_wrappers_refuse_cpu_tensors_and_bad_shapes(spa3d):
  video, tracks, scores = torch.zeros(4, 8, 8, 3, dtype=torch.uint8), torch.zeros(5, 4, 2), torch.zeros(5, 4)
  with pytest.raises(spa3d._lib.Spa3dError):
    spa3d.render_tracks(video, tracks, scores)
  with pytest.raises(spa3d._lib.Spa3dError):
    spa3d.project_tracks(torch.zeros(5, 4, 3), np.eye(3), np.eye(4), 8, 8)
  assert set(('render_tracks', 'project_tracks', 'visualize_npz')) <= set(spa3d.__all__)
