"""The boundary of spa3d_render_heatmap on the CPU (no compute call): the ctypes layout of spa3d_heatmap against the header, every refusal of
the entry point -- each SPA3D_ERR_ARG with a message, before any launch -- the workspace sizing, and the Python wrapper's own refusals (CPU
tensors, shapes, options)."""
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
  m = spa3d._lib.Heatmap()
  m.N, m.T, m.H, m.W, m.coords = 5, 4, 30, 40, coords
  m.tracks = m.values = m.map = m.weight = m.video = m.out = FAKE
  if coords == 3:
    m.intrinsics = m.extrinsics = FAKE
    m.resize_h = m.resize_w = 1024
  m.radius, m.power, m.normalize, m.alpha = 12, 2, 1, 2048
  return m


def test_struct_matches_the_header(spa3d):
  hdr = open(os.path.join(ROOT, 'include', 'spa3d.h')).read()
  body = re.search(r'typedef struct \{((?:(?!typedef struct).)*?)\} spa3d_heatmap;', hdr, re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  names = []
  for decl in body.split(';'):
    decl = decl.strip()
    if not decl:
      continue
    first, *rest = decl.split(',')
    ctype = 'ptr' if '*' in first else first.split()[0]
    for n in [first.split()[-1].lstrip('*')] + [x.strip() for x in rest]:
      names.append((n, ctype))
  fields = spa3d._lib.Heatmap._fields_
  assert [n for n, _ in names] == [n for n, _ in fields]
  kinds = {'ptr': C.c_void_p, 'int32_t': C.c_int32, 'float': C.c_float}
  for (n, ctype), (_, ft) in zip(names, fields):
    assert ft is kinds[ctype], n
  H = spa3d._lib.Heatmap
  assert C.sizeof(H) == 144 and H.tracks.offset == 16 and H.values.offset == 56 and H.map.offset == 88 and H.out.offset == 112 and H.colour_bgr.offset == 136


def test_every_refusal_is_err_arg_with_a_message(spa3d, handle):
  lib = spa3d._lib.load()
  need = lib.spa3d_heatmap_workspace_bytes(handle, 5, 4)
  call = lambda m, ws=FAKE, nb=None: lib.spa3d_render_heatmap(handle, C.byref(m) if m is not None else None, ws, need if nb is None else nb, None)
  err = lambda: lib.spa3d_last_error(handle)

  def refused(word, coords=2, **fields):
    m = good(spa3d, coords)
    for k, v in fields.items():
      setattr(m, k, v)
    assert call(m) == 1 and word in err() and err().startswith(b'heatmap: '), (fields, err())

  refused(b'tracks', tracks=None)
  refused(b'values', values=None)
  refused(b'all NULL', map=None, weight=None, out=None)      # nothing asked for
  refused(b'video', video=None)                              # out without video
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
  for v in (0, -1, 65):
    refused(b'radius', radius=v)
  for v in (0, 3, -2):
    refused(b'power', power=v)
  for v in (-1, 4097):
    refused(b'alpha', alpha=v)
  for v in (float('nan'), float('inf'), float('-inf')):
    refused(b'finite lo, hi', normalize=0, lo=v, hi=1.0)
    refused(b'finite lo, hi', normalize=0, lo=0.0, hi=v)
  refused(b'2^31', N=1 << 20, T=(1 << 11) + 1)               # more point-frames than one launch holds
  refused(b'2^24', T=64, H=16384, W=16384)                    # 64 x 256 x 1024 (frame, tile) pairs
  assert call(None) == 1 and err()
  assert lib.spa3d_render_heatmap(None, C.byref(good(spa3d)), FAKE, need, None) == 1
  # lo, hi are not read unless the overlay uses them
  m = good(spa3d)
  m.normalize, m.lo, m.out, m.video = 0, float('nan'), None, None
  assert call(m, FAKE, 0) == 1 and b'workspace too small' in err()
  m = good(spa3d)
  m.lo = float('nan')                                          # normalize != 0: the clip's own range
  assert call(m, FAKE, 0) == 1 and b'workspace too small' in err()
  # the workspace: a missing or short one names the bytes needed, and the need is within spa3d_heatmap_workspace_bytes
  for coords in (2, 3):
    m = good(spa3d, coords)
    assert call(m, FAKE, 0) == 1 and b'workspace too small' in err()
    asked = int(err().split(b'need ')[1].split()[0])
    assert 0 < asked <= need
    assert call(m, None, need) == 1 and b'workspace too small' in err()
    assert call(m, FAKE, asked - 1) == 1 and int(err().split(b'need ')[1].split()[0]) == asked
  m = good(spa3d)
  m.out = m.video = None                                       # no overlay: no min / max arrays
  assert call(m, FAKE, 0) == 1 and int(err().split(b'need ')[1].split()[0]) < asked


def test_workspace_bytes_is_monotone(spa3d, handle):
  lib = spa3d._lib.load()
  f = lambda n, t: lib.spa3d_heatmap_workspace_bytes(handle, n, t)
  sizes = [f(n, 150) for n in (1, 2, 64, 512, 4096, 65536)]
  assert all(0 < a < b for a, b in zip(sizes, sizes[1:]))
  sizes = [f(4096, t) for t in (1, 2, 24, 150, 300, 10000)]
  assert all(0 < a < b for a, b in zip(sizes, sizes[1:]))
  assert f(4096, 150) >= 4096 * 150 * 8 and f(1 << 20, 1 << 12) > 1 << 34   # 64-bit sizes
  assert f(0, 4) == -1 and f(4, 0) == -1 and f(-1, 4) == -1 and lib.spa3d_heatmap_workspace_bytes(None, 4, 4) == -1


def test_python_wrapper_refuses_cpu_tensors_and_bad_shapes(spa3d):
  tracks, values, video = torch.zeros(5, 4, 2), torch.zeros(5, 4), torch.zeros(4, 8, 8, 3, dtype=torch.uint8)
  with pytest.raises(spa3d._lib.Spa3dError):
    spa3d.render_heatmap(tracks, values, 8, 8)                 # CPU tensors
  with pytest.raises(spa3d._lib.Spa3dError):
    spa3d.render_heatmap(tracks, values, video=video)
  for kw in (dict(), dict(H=8), dict(W=8), dict(H=8, W=8, alpha=1.5), dict(H=8, W=8, alpha=-0.1), dict(H=8, W=8, alpha=0.3), dict(H=8, W=8, out=video),
             dict(H=8, W=8, use_visibility=True), dict(H=8, W=8, value_range=(1.0,))):
    with pytest.raises(ValueError):                            # options are checked before any tensor is looked at
      spa3d.render_heatmap(tracks, values, **kw)
  with pytest.raises(ValueError, match="mode"):
    spa3d.visualize_npz('nothing.npz', mode='dots')
  assert 'render_heatmap' in spa3d.__all__
  import inspect
  sig = inspect.signature(spa3d.render_heatmap)
  assert list(sig.parameters) == ['tracks', 'values', 'H', 'W', 'video', 'visibs', 'intrinsics', 'extrinsics', 'radius', 'power', 'normalize', 'value_range', 'alpha',
                                  'use_visibility', 'colour_bgr', 'resize', 'out', 'return_weight']
  d = {k: p.default for k, p in sig.parameters.items()}
  assert (d['radius'], d['power'], d['normalize'], d['alpha'], d['resize'], d['return_weight']) == (12, 2, True, 0.5, (1024, 1024), False)
  assert inspect.signature(spa3d.visualize_npz).parameters['mode'].default == 'tracks'
