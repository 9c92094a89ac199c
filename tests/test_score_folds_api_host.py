"""The host side of the fold call (spa3d_score_folds; TrackAutoEncoder3D.score_all, fold_offsets) on the CPU, no compute call: the fold offsets,
score_all's validation (ValueError before any device work), the header against the binding table, and the C-ABI refusals -- every one of them
comes before the first launch, so they are reachable without a device (the pointers are fake and never dereferenced)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import folds_util as FU
from util import MINI, O, ROOT, product_model


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


def test_fold_offsets_values_and_errors(spa3d):
  assert spa3d.fold_offsets(10, 3).tolist() == [0, 4, 7, 10]          # larger folds first
  assert spa3d.fold_offsets(200, 3).tolist() == [0, 67, 134, 200]
  assert spa3d.fold_offsets(4096, 8).tolist() == [512 * i for i in range(9)]
  assert spa3d.fold_offsets(64, 64).tolist() == list(range(65))
  assert spa3d.fold_offsets(7, 2).tolist() == [0, 4, 7]
  off = spa3d.fold_offsets(1000, 7)
  assert off.dtype == np.int32 and off.shape == (8,) and off[0] == 0 and off[-1] == 1000
  sizes = np.diff(off)
  assert sizes.max() - sizes.min() == 1 and (np.diff(sizes) <= 0).all()
  for n, f in ((10, 1), (10, 0), (10, -3), (1000, 65), (5, 6), (1, 2)):
    with pytest.raises(ValueError):
      spa3d.fold_offsets(n, f)
  with pytest.raises(ValueError):
    spa3d.fold_offsets(10, 2.5)


def _cpu_case(spa3d, N=12, T=8):
  cfg = O.Config(**MINI, use_dino=False, use_depth=False)
  model = product_model(spa3d, cfg, 'fp32')
  batch, qf = FU.fold_batch(O.synthetic_batch(2, N, 1, T))
  _, _, n = model._handle(0, 0)
  return model, {'params': model.tree_from_flat(torch.zeros(n), 0, 0)}, batch, qf


def test_score_all_validates_on_the_host(spa3d):
  model, v, batch, qf = _cpu_case(spa3d)
  N = 12

  def bad(match, b=batch, m=model, **kw):
    with pytest.raises(ValueError, match=match):
      m.score_all(v, b, **kw)

  bad('folds', folds=1)
  bad('folds', folds=65)
  bad('folds', folds=13)                                  # more folds than tracks
  bad('offsets', folds=[0, 6])                            # F = 1
  bad('offsets', folds=np.array([0.0, 6.0, 12.0]))        # not integers
  bad('start at 0', folds=[1, 6, N])
  bad('start at 0', folds=[0, 6, N - 1])
  bad('start at 0', folds=[0, 6, 6, N])
  bad('start at 0', folds=torch.tensor([0, 7, 6, N]))
  bad('thresholds', thresholds=(0.0,))
  for key in ('support_tracks', 'support_tracks_visible', 'boundary_frame'):
    bad(key, b={k: t for k, t in batch.items() if k != key})
  bad('query_frame', b={k: t for k, t in batch.items() if k != 'query_points'})                  # neither query_points nor query_frame
  bad('query_points', b=dict(batch, query_points=batch['query_points'][:, :5]))                  # not [B,N,4]
  noq = {k: t for k, t in batch.items() if k != 'query_points'}
  bad('query_frame', b=dict(noq, query_frame=qf[:, :5]))
  bad('query_frame', b=dict(noq, query_frame=qf.float()))
  bad('outside', b=dict(noq, query_frame=torch.full_like(qf, 8)))
  bad('outside', b=dict(noq, query_frame=torch.full_like(qf, -1)))
  bad('support_count', b=dict(batch, support_count=torch.tensor([N, N - 1])))                    # ragged
  bad('query_tracks', b=dict(batch, query_tracks=torch.zeros(2, 5, 8, 3), query_tracks_visible=torch.zeros(2, 5, 8, 1)))
  bad('query_tracks', b=dict(batch, query_tracks=torch.zeros(2, N, 7, 3), query_tracks_visible=torch.zeros(2, N, 7, 1)))
  other = product_model(spa3d, O.Config(**dict(MINI, num_output_frames=6), use_dino=False, use_depth=False), 'fp32')
  bad('num_output_frames', m=other)                                                              # default targets need T == T_out
  chunked = product_model(spa3d, O.Config(**MINI, use_dino=False, use_depth=False), 'fp32')
  chunked.decoder_scan_chunk_size = 4
  bad('chunk', m=chunked)
  with pytest.raises(ValueError):
    spa3d.TrackAutoEncoder(num_output_frames=8, precision='fp32').score_all(v, batch)
  # everything valid, but on the CPU: refused as every compute call is, and only after the host checks
  for b in (batch, dict(noq, query_frame=qf), dict(batch, support_count=torch.tensor([N, N]), query_count=torch.tensor([1, 1]),
                                                  query_tracks=torch.zeros(2, 1, 8, 3), query_tracks_visible=torch.zeros(2, 1, 8, 1))):
    with pytest.raises(spa3d._lib.Spa3dError):
      model.score_all(v, b, folds=3)


def test_header_and_binding_table_agree(spa3d):
  text = open(os.path.join(ROOT, 'include', 'spa3d.h')).read()
  sigs = spa3d._lib._SIGS
  for name, nargs in (('spa3d_score_folds', 10), ('spa3d_score_folds_workspace_bytes', 4), ('spa3d_op_attention_holdout', 21)):
    m = re.search(r'\b' + name + r'\s*\(([^;]*?)\)\s*;', text, re.S)
    assert m, f'{name} is not declared in include/spa3d.h'
    args = [a for a in re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',') if a.strip()]
    assert len(args) == nargs == len(sigs[name][1]), (name, len(args), len(sigs[name][1]))
    assert hasattr(spa3d._lib.load(), name)
  assert sigs['spa3d_score_folds_workspace_bytes'][0] is C.c_int64 and sigs['spa3d_score_folds'][0] is C.c_int
  assert 'fold_offsets' in spa3d.__all__ and callable(spa3d.TrackAutoEncoder3D.score_all)


def test_c_abi_refusals_without_a_device(spa3d):
  N, T = 40, 8
  h = product_model(spa3d, O.Config(**MINI, use_dino=False, use_depth=False), 'fp32')._handle(0, 0)[0]
  h2d = spa3d.TrackAutoEncoder(num_output_frames=8, precision='fp32')._handle(0, 0)[0]
  fake = 0x100000

  def make_batch():
    b = spa3d._lib.Batch()
    b.B, b.N, b.Q, b.T, b.discretize = 2, N, N, T, 1
    b.support_tracks = b.support_tracks_visible = b.query_points = b.boundary_frame = b.noise = fake
    return b

  def make_scores():
    sc = spa3d._lib.Scores()
    sc.query_stats = fake
    return sc

  lib = spa3d._lib.load()
  need = lib.spa3d_score_folds_workspace_bytes(h, N, T, 3)
  assert need > 0
  assert lib.spa3d_score_folds_workspace_bytes(h, N, T, 3) == need   # a pure function of the handle's options and the shape
  assert FU.check_refusals(spa3d, h, h2d, make_batch, make_scores, N, T, fake, 2 * need, fake) == 18
  assert lib.spa3d_score_folds(None, fake, C.byref(make_batch()), 3, FU.i32([0, 14, 27, N]), C.byref(make_scores()), None, fake, 2 * need, None) == 1
  assert lib.spa3d_score_folds(h, None, C.byref(make_batch()), 3, FU.i32([0, 14, 27, N]), C.byref(make_scores()), None, fake, 2 * need, None) == 1
  # the kernel's test entry refuses a bad hole before it touches anything
  def holdout(holes, Nk=300):
    return lib.spa3d_op_attention_holdout(fake, fake, fake, 192, 192, 192, fake, fake, len(holes) // 2, 5, Nk, 2, 96, FU.i32(holes), fake, None, 1, 0,
                                          fake, 1 << 20, None)
  for holes in ([-1, 5], [290, 301], [9, 8], [0, 300], [0, 10, 300, 301]):
    assert holdout(holes) == 1, holes
