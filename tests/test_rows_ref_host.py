"""The references of tests/rows_util.py checked on the host, without a GPU: each against a second, independent statement of the same operation
(brute force, numpy's own routines, the oracle, autograd), so that tests/test_gpu_rows.py compares the kernels with something that is itself tested."""
import numpy as np
import torch

import rows_util as RU
from util import O


def test_prune_plan_reference_against_a_double_loop():
  rng = np.random.default_rng(0)
  for nseq, S in ((1, 1), (3, 2), (5, 65), (17, 151)):
    km = (rng.random((nseq, S)) < 0.5).astype(np.float32)
    km[rng.random((nseq, S)) < 0.1] = 0.5
    km[rng.random((nseq, S)) < 0.1] = -1.0
    km[rng.random((nseq, S)) < 0.1] = -0.0
    km[rng.random((nseq, S)) < 0.05] = np.nan
    if nseq > 1:
      km[1] = 0.0
    cnt, off, row_src, kept = RU.prune_plan_ref(km)
    rows, c2 = [], []
    for s in range(nseq):
      n = 0
      for t in range(S):
        v = float(km[s, t])
        if not v == 0.0:       # -0.0 == 0.0: dropped; NaN == 0.0 is false: kept
          rows.append(s * S + t); n += 1
      c2.append(n)
    assert kept == len(rows) and list(row_src) == rows and list(cnt) == c2
    assert off[0] == 0 and list(np.diff(off)) == c2 and off[-1] == kept
  km = np.array([[-0.0, np.nan, 0.0, 2.0]], np.float32)
  assert list(RU.prune_plan_ref(km)[2]) == [1, 3]
  cnt, off, row_src, kept = RU.prune_plan_ref(np.zeros((0, 4), np.float32))
  assert kept == 0 and len(row_src) == 0 and list(off) == [0]


def test_slot_plan_reference_against_numpy_unique():
  rng = np.random.default_rng(1)
  for B, Q, nf in ((1, 1, 1), (1, 8, 3), (2, 255, 40), (3, 17, 17), (4, 33, 1), (2, 40, 1000)):
    qf = rng.integers(0, nf, (B, Q)).astype(np.int32)
    slot, sb, sf, sq0, nslot = RU.slot_plan_ref(qf)
    base = 0
    for b in range(B):
      vals, first = np.unique(qf[b], return_index=True)
      order = np.argsort(first)                       # distinct frames in order of first occurrence
      vals, first = vals[order], first[order]
      n = len(vals)
      assert list(sf[base:base + n]) == list(vals) and list(sq0[base:base + n]) == list(b * Q + first) and list(sb[base:base + n]) == [b] * n
      rank = {int(v): i for i, v in enumerate(vals)}
      assert list(slot[b * Q:(b + 1) * Q]) == [base + rank[int(f)] for f in qf[b]]
      base += n
    assert nslot == base
    assert np.array_equal(sf[slot], qf.reshape(-1)) and np.array_equal(sb[slot], np.repeat(np.arange(B), Q))   # every query's slot has its sample and frame


def _frames(Cl, n, rng):
  last = (Cl - 1) // 5
  pool = [0, 1, 3, last, last + 1]
  return torch.tensor([pool[int(i)] for i in rng.integers(0, len(pool), n)], dtype=torch.int32)


def test_assembly_reference_is_the_oracles_at_a_window_of_128_and_its_autograd_is_the_backward_reference():
  rng = np.random.default_rng(2)
  cfg = O.Config()
  D, Cl = cfg.decoder_num_channels, cfg.decoder_num_channels - 128
  B, Q, L = 2, 3, 2
  g = torch.Generator().manual_seed(3)
  lat = torch.randn(B, L, Cl, generator=g, dtype=torch.float64)
  qtok = torch.randn(B, Q, D, generator=g, dtype=torch.float64)
  qf = _frames(Cl, B * Q, rng).reshape(B, Q)
  want = O.TrackAutoEncoder3D(cfg).append_time_feat(lat[:, None].expand(B, Q, L, Cl), qf)
  got = RU.assemble_ref(qtok, lat, qf, D)
  assert torch.equal(got[:, :, 1:], want) and torch.equal(got[:, :, 0], qtok)
  for Cl2, D2 in ((24, 40), (16, 24), (20, 27)):
    lat = torch.randn(B, L, Cl2, generator=g, dtype=torch.float64, requires_grad=True)
    qtok = torch.randn(B, Q, D2, generator=g, dtype=torch.float64, requires_grad=True)
    qf = _frames(Cl2, B * Q, rng).reshape(B, Q)
    seq = RU.assemble_ref(qtok, lat, qf, D2)
    # element by element: column Cl + dd of token 1 + n is lat[b][n][dd + 5 t] inside [0, Cl), else 0
    for b in range(B):
      for q in range(Q):
        for dd in range(D2 - Cl2):
          cc = dd + 5 * int(qf[b, q])
          exp = lat[b, :, cc] if cc < Cl2 else torch.zeros(L, dtype=torch.float64)
          assert torch.equal(seq[b, q, 1:, Cl2 + dd], exp)
    dseq = torch.randn(B, Q, 1 + L, D2, generator=g, dtype=torch.float64)
    gq, gl = torch.autograd.grad(seq, (qtok, lat), dseq)
    dq, dl = RU.assemble_bwd_ref(dseq, qf, Cl2)
    assert torch.equal(dq, gq) and float((dl - gl).abs().max()) < 1e-12
    add = RU.assemble_bwd_addends(dseq, qf, Cl2)
    assert add.shape == (2 * Q, B * L * Cl2) and float((add.sum(0).reshape(B, L, Cl2) - gl).abs().max()) < 1e-12


def test_shared_rows_references_compose_to_the_dense_assembly_and_reduce_is_the_transpose_of_expand():
  rng = np.random.default_rng(4)
  g = torch.Generator().manual_seed(5)
  for (Cl, D), B, Q, L in (((24, 40), 2, 9, 4), ((16, 24), 1, 1, 1), ((16, 24), 2, 60, 2)):
    qf = _frames(Cl, B * Q, rng).reshape(B, Q)
    plan = RU.slot_plan_ref(qf.numpy())
    slot, sb, sf, sq0, nslot = plan
    lat = torch.randn(B, L, Cl, generator=g).bfloat16()
    qtok = torch.randn(B * Q, D, generator=g).bfloat16()
    xU = RU.share_assemble_ref(qtok, lat, plan, D)
    dense = RU.assemble_ref(qtok.reshape(B, Q, D), lat, qf, D).reshape(B * Q, 1 + L, D)
    assert torch.equal(RU.share_expand_ref(xU, slot, nslot, L).view(torch.int16), dense.view(torch.int16))
    # <expand(u), v> == <u, reduce(v)> on small integers: every product and sum is exact in fp64
    U = nslot * L + B * Q
    u = torch.randint(-4, 5, (U, D), generator=g).double()
    v = torch.randint(-4, 5, (B * Q, 1 + L, D), generator=g).double()
    lhs = (RU.share_expand_ref(u, slot, nslot, L) * v).sum()
    rhs = (u * RU.share_reduce_ref(v, slot, nslot)).sum()
    assert float(lhs) == float(rhs)
    # the backward form adds the slot row to one member per slot: summed over a slot's members it equals adding it to all and reducing once
    add = torch.randint(-4, 5, (B * Q, 1 + L, D), generator=g).double()
    out, take = RU.share_expand_add_ref(u, add, slot, sq0, nslot, L)
    assert int(take[:, 1].sum()) == nslot and bool(take[:, 0].all())
    assert torch.equal(RU.share_reduce_ref(out, slot, nslot)[:nslot * L], RU.share_reduce_ref(add, slot, nslot)[:nslot * L] + u[:nslot * L])


def test_colsum_and_pooling_references_against_loops():
  g = torch.Generator().manual_seed(6)
  for rgroup, rskip in ((0, 0), (7, 1), (7, 3)):
    rows, n, ld = 19, 5, 8
    rmap = RU.crow(rows, rgroup, rskip)
    x = torch.randn(int(rmap[-1]) + 2, ld, generator=g)
    want = torch.zeros(n, dtype=torch.float64)
    for m in range(rows):
      pr = m + (m // rgroup + 1) * rskip if rgroup else m
      want += x[pr, :n].double()
    assert float((RU.colsum_ref(x, rows, n, rgroup, rskip) - want).abs().max()) < 1e-12
  tok = torch.randn(4, 6, 3, generator=g, dtype=torch.float64, requires_grad=True)
  vis = torch.tensor([[1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0], [0, 2.0, 0, -1.0, 0, 0], [0, 0, 0, 0, 1, 0]], dtype=torch.float32)
  out = RU.vis_mean_pool_ref(tok, vis)
  o, t = out.detach(), tok.detach()
  assert torch.equal(o[1], torch.zeros(3, dtype=torch.float64))
  assert float((o[2] - (t[2, 1] + t[2, 3]) / 2).abs().max()) < 1e-15 and float((o[0] - t[0].mean(0)).abs().max()) < 1e-15
  dout = torch.randn(4, 3, generator=g, dtype=torch.float64)
  (gt,) = torch.autograd.grad(out, tok, dout)
  assert float((RU.vis_mean_pool_bwd_ref(dout, vis) - gt).abs().max()) < 1e-15


def test_every_refusal_is_decided_before_anything_is_launched():
  """the calls of rows_util.plan_refusals / row_op_refusals with made-up (16-byte aligned) addresses and no GPU: every one returns SPA3D_ERR_ARG, so none of
  them reads a pointer or reaches a launch; tests/test_gpu_rows_plans.py repeats them against real buffers"""
  import ctypes as C
  import spa3d
  lib = spa3d._lib.load()
  count = C.c_int64(-5)
  base = 0x7f0000000000
  bad = [f'{n}: status {rc}' for n, rc in RU.plan_refusals(lib, base, base + 0x1000, [base + 0x2000 + 0x100 * i for i in range(5)], C.byref(count), None) if rc != 1]
  n = 0
  for dtype in (0, 1, 2):
    for name, rc in RU.row_op_refusals(lib, dtype, base + 0x10000, base + 0x20000, base + 0x30000, base + 0x40000, base + 0x1000, base + 0x50000, None):
      n += 1
      if rc != 1:
        bad.append(f'dtype {dtype} {name}: status {rc}')
  assert not bad, 'not refused: ' + '; '.join(bad)
  assert count.value == -5 and n > 400
