"""CPU-side checks of the intra-sample chunk options ("query_chunk", "track_chunk"; include/spa3d.h spa3d_set_option): the names are accepted,
the one-sample rule is enforced when the options are set, and the dry-run workspace sizing of BASELINE.json configs[4] (B = 1, N = 8192, Q = 2048,
T = 300, training) follows them.  No compute call is made (no GPU here)."""

import pytest

from util import MINI, O, product_model

N, Q, T = 8192, 2048, 300
CARD = 288e9


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


def _handle(spa3d, precision='fp32'):
  m = spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=768, depth_feature_dim=1, precision=precision)
  return m, m._handle(768, 1)[0]


def _ws(lib, h, tc=None, qc=None, B=1, chunk=1):
  if tc is not None:
    assert lib.spa3d_set_option(h, b'track_chunk', float(tc)) == 0
  if qc is not None:
    assert lib.spa3d_set_option(h, b'query_chunk', float(qc)) == 0
  return lib.spa3d_workspace_bytes(h, B, N, Q, T, chunk, 1)


def test_options_accepted_and_one_sample_rule(spa3d):
  lib = spa3d._lib.load()
  m = product_model(spa3d, O.Config(**MINI, use_dino=False, use_depth=False), 'fp32')
  h = m._handle(0, 0)[0]
  for name in (b'query_chunk', b'track_chunk'):
    assert lib.spa3d_set_option(h, name, 64.0) == 0, lib.spa3d_last_error(h)
    assert lib.spa3d_set_option(h, name, 0.0) == 0
    assert lib.spa3d_set_option(h, name, -1.0) == 1
  # "chunk" > 1 together with either option is refused, in either order, with a message that says why
  for name in (b'query_chunk', b'track_chunk'):
    assert lib.spa3d_set_option(h, name, 32.0) == 0
    assert lib.spa3d_set_option(h, b'chunk', 2.0) == 1
    assert b'chunk' in lib.spa3d_last_error(h)
    assert lib.spa3d_set_option(h, b'chunk', 1.0) == 0  # one sample per chunk is what the options imply anyway
    assert lib.spa3d_set_option(h, b'chunk', 0.0) == 0
    assert lib.spa3d_set_option(h, name, 0.0) == 0
  assert lib.spa3d_set_option(h, b'chunk', 2.0) == 0
  for name in (b'query_chunk', b'track_chunk'):
    assert lib.spa3d_set_option(h, name, 16.0) == 1
    assert b'chunk' in lib.spa3d_last_error(h)
  assert lib.spa3d_set_option(h, b'chunk', 0.0) == 0


def test_fp32_cfg5_sample_fits_with_the_options(spa3d):
  lib = spa3d._lib.load()
  _, h = _handle(spa3d, 'fp32')
  off = _ws(lib, h, 0, 0)
  on = _ws(lib, h, 1024, 256)
  print(f'fp32 configs[4] one sample, training: {off / 1e9:.1f} GB unchunked, {on / 1e9:.1f} GB with track_chunk 1024 / query_chunk 256')
  assert 0 < on < off
  assert on < 0.8 * CARD
  # the options imply one sample per chunk: the chunk argument no longer matters
  assert _ws(lib, h, chunk=1) == _ws(lib, h, chunk=4) == on


def test_workspace_does_not_grow_as_chunks_shrink(spa3d):
  lib = spa3d._lib.load()
  _, h = _handle(spa3d, 'fp32')
  prev = None
  for tc, qc in ((4096, 1024), (2048, 512), (1024, 256), (512, 128), (256, 64)):
    w = _ws(lib, h, tc, qc)
    assert prev is None or w <= prev, (tc, qc, w, prev)
    prev = w
  # each option on its own shrinks the request too
  off = _ws(lib, h, 0, 0)
  assert _ws(lib, h, 1024, 0) < off and _ws(lib, h, 0, 256) < off
  # a chunk at least as large as the sample is one chunk: the intra-sample loop with one iteration
  assert _ws(lib, h, N, Q) <= off


@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'fp16'])
def test_options_at_zero_size_exactly_as_never_set(spa3d, precision):
  lib = spa3d._lib.load()
  _, h0 = _handle(spa3d, precision)
  _, h1 = _handle(spa3d, precision)
  assert _ws(lib, h1, 512, 128) != _ws(lib, h0)
  _ws(lib, h1, 0, 0)  # set, then back to 0
  for B, chunk in ((1, 1), (2, 2), (3, 1)):
    assert lib.spa3d_workspace_bytes(h0, B, 1024, 256, T, chunk, 1) == lib.spa3d_workspace_bytes(h1, B, 1024, 256, T, chunk, 1)
    assert lib.spa3d_workspace_bytes(h0, B, 1024, 256, T, chunk, 0) == lib.spa3d_workspace_bytes(h1, B, 1024, 256, T, chunk, 0)


def test_decoder_scan_chunk_size_must_divide_q(spa3d):
  cfg = O.Config(**MINI, use_dino=False, use_depth=False)
  m = product_model(spa3d, cfg, 'fp32')
  m.decoder_scan_chunk_size = 5
  h = m._handle(0, 0)[0]
  with pytest.raises(ValueError):
    m._chunk_options(h, 12)
  m.decoder_scan_chunk_size = 4
  m._chunk_options(h, 12)
  m.decoder_scan_chunk_size = None
  m._chunk_options(h, 12)
  # back at None, the handle sizes as one that never chunked
  lib = spa3d._lib.load()
  h0 = product_model(spa3d, cfg, 'fp32')._handle(0, 0)[0]
  assert lib.spa3d_workspace_bytes(h, 2, 16, 12, 8, 2, 1) == lib.spa3d_workspace_bytes(h0, 2, 16, 12, 8, 2, 1)
