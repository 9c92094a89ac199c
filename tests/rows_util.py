"""Host references of the row plumbing (csrc/rows.hip) for tests/test_gpu_rows.py: plain numpy / torch, fp64 where there is arithmetic, written from the
statement of each operation and not from the kernels.  Checked on the CPU, against brute force and against the oracle, in tests/test_rows_ref_host.py.
Copies return the input's dtype (a selection moves bits); sums return float64."""
import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ row maps, column sums
def crow(M, rgroup, rskip):
  """the row map of the embedding stage: row m of the compact tensor is row m + (m // rgroup + 1) rskip of the padded one (rgroup == 0: m)"""
  m = torch.arange(M)
  return m + (m // rgroup + 1) * rskip if rgroup > 0 else m


def colsum_ref(x, rows, n, rgroup, rskip):
  """x [R, ld] -> float64 [n]: the sum of the mapped rows' first n columns"""
  return x[crow(rows, rgroup, rskip)][:, :n].double().sum(0)


# ------------------------------------------------------------------------------------------------ token-pruning plan
def prune_plan_ref(km):
  """km float32 numpy [nseq, S] -> (cnt [nseq], seq_off [nseq + 1], row_src [kept], kept), int32: per sequence the frames with km != 0 (-0.0 is dropped,
  NaN is kept), in time order; row_src holds the dense row seq * S + t"""
  nseq, S = km.shape
  cnt = np.zeros(nseq, np.int32)
  rows = []
  for s in range(nseq):
    t = np.nonzero(km[s] != 0)[0]
    cnt[s] = len(t)
    rows.append(s * S + t)
  seq_off = np.zeros(nseq + 1, np.int32)
  seq_off[1:] = np.cumsum(cnt)
  row_src = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
  return cnt, seq_off, row_src, int(seq_off[-1])


# ------------------------------------------------------------------------------------------------ shared-latent-row plan
def slot_plan_ref(qframe):
  """qframe int numpy [B, Q] -> (slot [B Q], slot_b, slot_f, slot_q0 [nslot], nslot), int32.  A slot is a distinct (sample, frame) pair; within a sample
  the slots are numbered by the first query that has the frame, samples follow one another; slot_q0 is that first query as b Q + q"""
  B, Q = qframe.shape
  slot = np.zeros(B * Q, np.int32)
  sb, sf, sq0 = [], [], []
  for b in range(B):
    rank = {}
    base = len(sb)
    for q in range(Q):
      f = int(qframe[b, q])
      if f not in rank:
        rank[f] = len(rank)
        sb.append(b); sf.append(f); sq0.append(b * Q + q)
      slot[b * Q + q] = base + rank[f]
  i32 = lambda a: np.asarray(a, np.int32)
  return slot, i32(sb), i32(sf), i32(sq0), len(sb)


# ------------------------------------------------------------------------------------------------ readout assembly
def window_eye(qframe, W, Cl):
  """[..., W, Cl] float64: eye(W, Cl, k = 5 t) per query, the literal form of track_autoencoder_3d.py:235-246 at a window of W columns"""
  d = torch.arange(W)[:, None]
  c = torch.arange(Cl)[None, :]
  return (c == d + 5 * qframe[..., None, None].to(torch.int64)).double()


def assemble_ref(qtok, lat, qframe, D):
  """qtok [B, Q, D], lat [B, L, Cl], qframe int [B, Q] -> seq [B, Q, 1 + L, D] in qtok's dtype: token 0 is the query token, token 1 + n is
  [lat[b][n] | einsum(lat[b][n], eye(W, Cl, 5 t))], W = D - Cl.  The einsum selects one value or none, so fp64 arithmetic moves the bits unchanged"""
  B, Q, _ = qtok.shape
  L, Cl = lat.shape[1], lat.shape[2]
  l64 = lat.double()[:, None].expand(B, Q, L, Cl)
  app = torch.einsum('bqnc,bqdc->bqnd', l64, window_eye(qframe, D - Cl, Cl))
  rows = torch.cat([l64, app], -1)
  return torch.cat([qtok.double()[:, :, None], rows], 2).to(qtok.dtype)


def assemble_bwd_ref(dseq, qframe, Cl):
  """dseq [B, Q, 1 + L, D] -> (dqtok [B, Q, D] in dseq's dtype, dlat float64 [B, L, Cl]): the transpose of assemble_ref"""
  D = dseq.shape[-1]
  g = dseq.double()[:, :, 1:]
  dlat = g[..., :Cl].sum(1) + torch.einsum('bqnd,bqdc->bnc', g[..., Cl:], window_eye(qframe, D - Cl, Cl))
  return dseq[:, :, 0].clone(), dlat


def assemble_bwd_addends(dseq, qframe, Cl):
  """the 2 Q addends of every dlat element, float64 [2 Q, B L Cl]: query q's direct column, then its window column (0 where the window misses it)"""
  B, Q = qframe.shape
  D = dseq.shape[-1]
  g = dseq.double()[:, :, 1:]
  direct = g[..., :Cl]                                                                    # [B, Q, L, Cl]
  win = torch.einsum('bqnd,bqdc->bqnc', g[..., Cl:], window_eye(qframe, D - Cl, Cl))
  return torch.stack([direct, win], 2).permute(1, 2, 0, 3, 4).reshape(2 * Q, -1)


# ------------------------------------------------------------------------------------------------ shared rows
def share_assemble_ref(qtok, lat, qframe_plan, D):
  """the distinct rows of the readout sequences: [nslot L latent rows | B Q query-token rows], from slot_plan_ref's (slot_b, slot_f).
  qtok [B Q, D], lat [B, L, Cl] -> [nslot L + B Q, D]"""
  _, slot_b, slot_f, _, nslot = qframe_plan
  L, Cl = lat.shape[1], lat.shape[2]
  if nslot:
    l64 = lat.double()[torch.as_tensor(slot_b, dtype=torch.int64)]                         # [nslot, L, Cl]
    app = torch.einsum('snc,sdc->snd', l64, window_eye(torch.as_tensor(slot_f), D - Cl, Cl))
    rows = torch.cat([l64, app], -1).reshape(nslot * L, D)
  else:
    rows = torch.zeros(0, D, dtype=torch.float64)
  return torch.cat([rows, qtok.double()], 0).to(qtok.dtype)


def _src_rows(slot, nslot, nseq, L):
  """[nseq, 1 + L] int64: the row of the slot tensor behind every (sequence, token)"""
  sl = torch.as_tensor(slot, dtype=torch.int64)
  tok0 = nslot * L + torch.arange(nseq)
  rest = sl[:, None] * L + torch.arange(L)[None, :]
  return torch.cat([tok0[:, None], rest], 1)


def share_expand_ref(srcU, slot, nslot, L):
  """srcU [nslot L + nseq, d] -> [nseq, 1 + L, d], a gather"""
  return srcU[_src_rows(slot, nslot, len(slot), L)]


def share_expand_add_ref(srcU, add, slot, slot_q0, nslot, L):
  """the backward form, float64: add everywhere, plus the source row at every token 0 and at the tokens of each slot's first member"""
  nseq = len(slot)
  first = torch.zeros(nseq, dtype=torch.bool)
  first[torch.as_tensor(slot_q0, dtype=torch.int64)] = True
  take = torch.cat([torch.ones(nseq, 1, dtype=torch.bool), first[:, None].expand(nseq, L)], 1)
  return add.double() + srcU.double()[_src_rows(slot, nslot, nseq, L)] * take[..., None], take


def share_reduce_ref(src, slot, nslot):
  """src [nseq, 1 + L, d] -> float64 [nslot L + nseq, d]: the sum of every slot's members' tokens 1.., then the tokens 0"""
  nseq, S, d = src.shape
  L = S - 1
  out = torch.zeros(nslot, L, d, dtype=torch.float64)
  out.index_add_(0, torch.as_tensor(slot, dtype=torch.int64), src.double()[:, 1:])
  return torch.cat([out.reshape(nslot * L, d), src.double()[:, 0]], 0)


# ------------------------------------------------------------------------------------------------ visible-frame pooling
def vis_mean_pool_ref(tok, vis):
  """tok [nseq, T, d], vis [nseq, T] -> float64 [nseq, d]: the mean over the frames with vis != 0, 0 without one (a non-unit visibility counts as 1)"""
  v = (vis != 0).double()
  return (tok.double() * v[..., None]).sum(1) / v.sum(1).clamp_min(1.0)[:, None]


def vis_mean_pool_bwd_ref(dout, vis):
  """dout [nseq, d] -> float64 [nseq, T, d]"""
  v = (vis != 0).double()
  return dout.double()[:, None, :] * (v / v.sum(1, keepdim=True).clamp_min(1.0))[..., None]


# ------------------------------------------------------------------------------------------------ what the entry points refuse
def plan_refusals(lib, km, idx, ints, count_ref, stream):
  """(name, status) of every call of the two plans that must return SPA3D_ERR_ARG: a NULL pointer once per argument, negative counts, S < 1.
  km, idx and the five `ints` are addresses; nothing is read through them when the calls are refused, as they must be"""
  P = lib.spa3d_op_prune_plan
  good = [km, 4, 8, ints[0], ints[1], ints[2], count_ref, stream]
  for i in (0, 3, 4, 5, 6):
    yield f'prune_plan NULL argument {i}', P(*[None if j == i else a for j, a in enumerate(good)])
  for label, i, v in (('nseq < 0', 1, -1), ('S = 0', 2, 0), ('S < 0', 2, -3)):
    yield f'prune_plan {label}', P(*[v if j == i else a for j, a in enumerate(good)])
  SP = lib.spa3d_op_share_plan
  good = [idx, 2, 4, ints[0], ints[1], ints[2], ints[3], ints[4], count_ref, stream]
  for i in (0, 3, 4, 5, 6, 7, 8):
    yield f'share_plan NULL argument {i}', SP(*[None if j == i else a for j, a in enumerate(good)])
  for label, i, v in (('B < 0', 1, -1), ('Q < 0', 2, -1)):
    yield f'share_plan {label}', SP(*[v if j == i else a for j, a in enumerate(good)])


def row_op_refusals(lib, dtype, a, o, f, fs, z, vis, stream):
  """(name, status) of every call of the dtype-carrying row entry points that must return SPA3D_ERR_ARG: a NULL pointer once per argument, a width that is
  no multiple of 16 bytes where the kernel is vector-only, a pointer off by one element and by 8 bytes, counts below their range, an unknown mode or dtype.
  a: input of `dtype`, o: output of `dtype`, f: fp32 output, fs: fp32 input, z: int32 input, vis: fp32 input -- 16-byte aligned addresses"""
  es, nv = (4, 4) if dtype == 0 else (2, 8)
  w = 2 * nv   # a width of 32 bytes
  s = stream

  def each(name, fn, good, ptrs, cases):
    for i in ptrs:
      yield f'{name} NULL argument {i}', fn(*[None if j == i else v for j, v in enumerate(good)])
    for label, i, v in cases:
      yield f'{name} {label}', fn(*[v if j == i else x for j, x in enumerate(good)])
    yield f'{name} dtype 3', fn(*[3 if j == len(good) - 2 else x for j, x in enumerate(good)])

  yield from each('colsum', lib.spa3d_op_colsum, [a, 4, w, w, 0, 0, f, dtype, s], (0, 6),
                  [('rows < 0', 1, -1), ('n = 0', 2, 0), ('n < 0', 2, -8), ('ld < n', 3, w - 1), ('rgroup < 0', 4, -1), ('rskip < 0', 5, -1)])
  for mode in (1, 2, 3):
    yield from each(f'rows mode {mode}', lib.spa3d_op_rows, [mode, a, z, 0, o, 4, w, dtype, s], (1, 2, 4),
                    [('n < 0', 5, -1), ('d = 0', 6, 0), ('d < 0', 6, -w), ('d + 1 element', 6, w + 1), ('d + half a vector', 6, w + nv // 2),
                     ('src + 1 element', 1, a + es), ('src + 8 bytes', 1, a + 8), ('dst + 1 element', 4, o + es), ('dst + 8 bytes', 4, o + 8)])
  for mode in (0, 4):
    yield from each(f'rows mode {mode}', lib.spa3d_op_rows, [mode, a, None, 1, o, 4, w, dtype, s], (1, 4),
                    [('n < 0', 5, -1), ('d = 0', 6, 0), ('d < 0', 6, -1), ('stride = 0', 3, 0), ('stride < 0', 3, -2)])
  yield 'rows mode 5', lib.spa3d_op_rows(5, a, z, 1, o, 4, w, dtype, s)
  yield 'rows mode -1', lib.spa3d_op_rows(-1, a, z, 1, o, 4, w, dtype, s)
  # share rows: (which, a, b, slot, slot_b, slot_f, slot_q0, nslot, B, Q, L, Cl, d, out, dtype, stream)
  shared = [('nslot < 0', 7, -1), ('B < 0', 8, -1), ('Q = 0', 9, 0), ('Q < 0', 9, -1), ('L < 0', 10, -1), ('d = 0', 12, 0), ('d < 0', 12, -w),
            ('d + 1 element', 12, w + 1), ('d + half a vector', 12, w + nv // 2), ('a + 1 element', 1, a + es), ('a + 8 bytes', 1, a + 8),
            ('out + 1 element', 13, o + es), ('out + 8 bytes', 13, o + 8), ('nslot > B Q', 7, 9)]
  yield from each('share assemble', lib.spa3d_op_share_rows, [0, a, a, None, z, z, None, 2, 1, 4, 2, nv, w, o, dtype, s], (1, 2, 4, 5, 13),
                  shared + [('Cl = 0', 11, 0), ('Cl + 1 element', 11, nv + 1), ('Cl > d', 11, 2 * w), ('lat + 1 element', 2, a + es), ('lat + 8 bytes', 2, a + 8)])
  yield from each('share expand', lib.spa3d_op_share_rows, [1, a, a, z, None, None, z, 2, 1, 4, 2, 0, w, o, dtype, s], (1, 3, 6, 13),
                  shared + [('add + 1 element', 2, a + es), ('add + 8 bytes', 2, a + 8)])
  yield from each('share reduce', lib.spa3d_op_share_rows, [2, a, None, z, z, None, None, 2, 1, 4, 2, 0, w, o, dtype, s], (1, 3, 4, 13),
                  shared + [('Q > 12288', 9, 12289)])
  yield 'share rows which 3', lib.spa3d_op_share_rows(3, a, a, z, z, z, z, 2, 1, 4, 2, nv, w, o, dtype, s)
  yield from each('assemble_readout', lib.spa3d_op_assemble_readout, [a, a, z, 1, 4, 2, nv, w, o, dtype, s], (0, 1, 2, 8),
                  [('B < 0', 3, -1), ('Q = 0', 4, 0), ('Q < 0', 4, -1), ('L < 0', 5, -1), ('Cl = 0', 6, 0), ('Cl < 0', 6, -nv), ('D < Cl', 7, nv - 1)])
  yield from each('assemble_readout_bwd', lib.spa3d_op_assemble_readout_bwd, [a, z, 1, 4, 2, nv, w, o, f, 0, dtype, s], (0, 1, 7, 8),
                  [('B < 0', 2, -1), ('Q = 0', 3, 0), ('Q < 0', 3, -1), ('L = 0', 4, 0), ('L < 0', 4, -1), ('Cl = 0', 5, 0), ('D < Cl', 6, nv - 1),
                   ('accumulate 2', 9, 2), ('accumulate -1', 9, -1)])
  yield from each('broadcast_rows', lib.spa3d_op_broadcast_rows, [fs, 2, w, o, 3, dtype, s], (0, 3),
                  [('rows = 0', 1, 0), ('rows < 0', 1, -1), ('d = 0', 2, 0), ('d < 0', 2, -1), ('B < 0', 4, -1)])
  yield from each('bcast_grad', lib.spa3d_op_bcast_grad, [a, w, 3, w, f, dtype, s], (0, 4),
                  [('per = 0', 1, 0), ('per < 0', 1, -1), ('B < 0', 2, -1), ('bstride < per', 3, w - 1), ('bstride < 0', 3, -w)])
  for name, fn in (('vis_mean_pool', lib.spa3d_op_vis_mean_pool), ('vis_mean_pool_bwd', lib.spa3d_op_vis_mean_pool_bwd)):
    yield from each(name, fn, [a, vis, 2, 4, w, o, dtype, s], (0, 1, 5), [('nseq < 0', 2, -1), ('T = 0', 3, 0), ('T < 0', 3, -1), ('d = 0', 4, 0), ('d < 0', 4, -1)])
