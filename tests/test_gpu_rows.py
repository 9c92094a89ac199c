"""GPU parity of the row plumbing of csrc/rows.hip on its own, through the spa3d_op_* entry points of csrc/ops.hip: column sums, the strided and indexed
row movers, readout sequence assembly and its backward, the shared-latent-row kernels, the parameter-row broadcast and its gradient, TRAJAN's visible-frame
pooling.  The two plans and the refusals are in tests/test_gpu_rows_plans.py.  References: tests/rows_util.py (checked in tests/test_rows_ref_host.py).

Every output lives in a parity_util.guarded() allocation and check_guards() runs after every call; inputs hold finite random values everywhere, the rows and
columns a kernel must not read included; a destination that is written in part or accumulated into is pre-filled with random values and whatever must stay
is compared with the fill bit for bit.  Every test runs in fp32, bf16 and fp16 (the fp16 twin of rows.hip has no other caller that isolates it).

  copies   bit-identical to the reference (int16 / int32 views)
  sums     element-wise.  fp32 results: 4 x the worst error of the float32 restatement against fp64, the restatement adding the addends one after the other
           (parity_util.sequential_sum) in the orders of parity_util.arrival_orders; 16-bit results: u_out |ref| on top of that.  One add and one rounding
           (scatter-add, strided add, expand with `add`, the pooling): parity_util.restated_bound.  The bound never comes from the kernel.

Shapes are the smallest at which each branch of each launcher is taken; `rows branch:` lines name the branch a case took (the launcher's own condition,
restated here), profiles/r15_rows_gates.log holds the table.  Added to the issue's lists because the code has the branch: n = 101 for the scalar column sum
(n = 100 is a multiple of 16 bytes in fp32 and takes the vector kernel there).  The strided movers run n = 5000 at stride 151 only up to d = 12 (a 0.6 GB
source otherwise).  Not reached: the second grid-stride pass of the 1-D kernels (GRID1D caps a grid at 2^20 workgroups, 2^28 items per pass) and the
nchunk >= 2^31 fallback of k_assemble_readout.  Scatter-add is specified for unique indices only and tested with nothing else."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity_util as PU
import rows_util as RU
from test_gpu_rank_linear import ROW_MAPS
from util import O

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2
DTYPES = [F32, BF16, F16]
GATHER_STRIDED, GATHER_IDX, SCATTER_IDX, SCATTER_ADD_IDX, ADD_STRIDED = range(5)
SHARE_ASSEMBLE, SHARE_EXPAND, SHARE_REDUCE = range(3)
MODEL_PAIR = (O.Config().decoder_num_channels - 128, O.Config().decoder_num_channels)   # (Cl, D) = (1152, 1280)
PAIRS = [(24, 40), (16, 24), MODEL_PAIR]


@pytest.fixture(scope='module')
def lib():
  import spa3d
  return spa3d._lib.load()


def _s():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(dtype):
  return {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}[dtype]


def _nv(dtype):
  return 4 if dtype == F32 else 8


def _bits(t):
  t = t.detach().cpu().contiguous()
  return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
  return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _gen(*key):
  return torch.Generator().manual_seed(sum(int(k) * m for k, m in zip(key, (1000003, 10007, 101, 7, 3, 1))) + 12345)


def _filled(rows, cols, dt, g, name, ld=None):
  """a guarded [rows, cols] output pre-filled with random values -> (device view, the fill on the host)"""
  fill = (torch.randn(rows, cols, generator=g) if dt.is_floating_point else torch.randint(-9000, -1, (rows, cols), generator=g, dtype=torch.int32)).to(dt)
  out = PU.guarded(rows, cols, dt, ld=ld, name=name, fill=0)
  out.copy_(fill)
  return out, fill


def _i32(a):
  return torch.as_tensor(np.asarray(a), dtype=torch.int32).cuda()


def _sum_gate(first, addends, ref64):
  """4 x the worst error against fp64 of `first` + the rows of `addends` added one after the other in float32, over parity_util.arrival_orders"""
  n, d = addends.shape
  e = 0.0
  for order in PU.arrival_orders(n, d):
    s32 = first.float().reshape(-1)
    for r0 in range(0, n, 1024):
      s32 = PU.sequential_sum(s32, addends[order[r0:r0 + 1024]].float(), torch.float32)
    e = max(e, float((s32.double() - ref64.reshape(-1)).abs().max()))
  return 4.0 * e


def _bound16(ref64, gate32, dt):
  """the sum gate behind one rounding to a 16-bit output"""
  if dt == torch.float32:
    return gate32
  u = PU.unit_roundoff(dt)
  return u * ref64.abs() + (1.0 + u) * gate32


# ================================================================================================ column sums
def _colsum_case(lib, dtype, rows, n, ld, rgroup, rskip, offset=0):
  dt = _dt(dtype)
  g = _gen(rows, n, ld, rgroup, rskip, offset)
  rmap = RU.crow(rows, rgroup, rskip)
  R = int(rmap[-1]) + 1 + 2
  x = torch.randn(R * ld + offset, generator=g).to(dt)      # rows outside the map and the columns past n hold values too: reading them shows
  xd = x.cuda()
  x2 = x[offset:].reshape(R, ld)
  out, fill = _filled(1, n, torch.float32, g, 'colsum out')
  ptr = xd.data_ptr() + offset * xd.element_size()
  vec = n % _nv(dtype) == 0 and ld % _nv(dtype) == 0 and ptr % 16 == 0
  rc = lib.spa3d_op_colsum(ptr, rows, n, ld, rgroup, rskip, out.data_ptr(), dtype, _s())
  assert rc == 0
  PU.check_guards()
  add = x2[rmap][:, :n]
  ref64 = fill[0].double() + RU.colsum_ref(x2, rows, n, rgroup, rskip)
  tag = f'rows {rows} n {n} ld {ld} map ({rgroup}, {rskip}) offset {offset}'
  print(f'  rows branch: colsum {dt} {tag} -> {"vector" if vec else "scalar"}')
  PU.assert_elementwise(out[0], ref64, _sum_gate(fill[0], add, ref64), f'GATE {dt} colsum {tag}')
  return vec


COLSUM_ROWS = [1, 7, 63, 64, 65, 1408, 5000]
COLSUM_N = [8, 48, 384, 392, 2048]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', COLSUM_N)
def test_colsum_vector(lib, dtype, n):
  """the 16-byte kernel: every width with every row count; the four row maps rotate so that every width meets every map; odd cases have ld = n + 8"""
  for i, rows in enumerate(COLSUM_ROWS):
    rgroup, rskip = ROW_MAPS[(i + COLSUM_N.index(n)) % 4]
    assert _colsum_case(lib, dtype, rows, n, n + 8 if i % 2 else n, rgroup, rskip)


@pytest.mark.parametrize('dtype', DTYPES)
def test_colsum_scalar(lib, dtype):
  """the element-wise kernel, taken three ways: a width that is no multiple of 16 bytes (n = 101; n = 100 in the 16-bit types), ld = n + 1, x offset by one
  element; the last two at a vector width"""
  for i, rows in enumerate((1, 7, 300, 5000)):
    rgroup, rskip = ROW_MAPS[i % 4]
    assert not _colsum_case(lib, dtype, rows, 101, 104, rgroup, rskip)
    assert _colsum_case(lib, dtype, rows, 100, 104, rgroup, rskip) == (dtype == F32)
    assert not _colsum_case(lib, dtype, rows, 48, 49, rgroup, rskip)
    assert not _colsum_case(lib, dtype, rows, 48, 56, rgroup, rskip, offset=1)


# ================================================================================================ row movers
MOVER_WIDTHS = [(F32, d) for d in (4, 12, 384)] + [(t, d) for t in (BF16, F16) for d in (8, 48, 384, 392)]
MOVER_N = [1, 7, 257, 5000]


@pytest.mark.parametrize('dtype,d', MOVER_WIDTHS)
def test_rows_by_index(lib, dtype, d):
  """gather, scatter and scatter-add through a seeded permutation into a tensor with five rows more than n"""
  dt = _dt(dtype)
  for n in MOVER_N:
    g = _gen(n, d, dtype)
    R = n + 5
    idx = torch.randperm(R, generator=g)[:n]
    idxd = _i32(idx.numpy())
    # gather: dst[i] = src[idx[i]]
    src = torch.randn(R, d, generator=g).to(dt)
    srcd = src.cuda()
    dst, _ = _filled(n, d, dt, g, 'gather dst')
    assert lib.spa3d_op_rows(GATHER_IDX, srcd.data_ptr(), idxd.data_ptr(), 0, dst.data_ptr(), n, d, dtype, _s()) == 0
    PU.check_guards()
    assert _same_bits(dst, src[idx]), f'gather by index n {n} d {d}'
    # scatter and scatter-add: dst[idx[i]] (+)= src[i]; the five rows outside the permutation keep the fill
    src = torch.randn(n, d, generator=g).to(dt)
    srcd = src.cuda()
    other = torch.ones(R, dtype=torch.bool)
    other[idx] = False
    dst, fill = _filled(R, d, dt, g, 'scatter dst')
    assert lib.spa3d_op_rows(SCATTER_IDX, srcd.data_ptr(), idxd.data_ptr(), 0, dst.data_ptr(), n, d, dtype, _s()) == 0
    PU.check_guards()
    got = dst.cpu()
    assert _same_bits(got[idx], src) and _same_bits(got[other], fill[other]), f'scatter by index n {n} d {d}'
    dst, fill = _filled(R, d, dt, g, 'scatter-add dst')
    assert lib.spa3d_op_rows(SCATTER_ADD_IDX, srcd.data_ptr(), idxd.data_ptr(), 0, dst.data_ptr(), n, d, dtype, _s()) == 0
    PU.check_guards()
    got = dst.cpu()
    ref64, ref32 = fill[idx].double() + src.double(), fill[idx].float() + src.float()
    PU.assert_elementwise(got[idx], ref64, PU.restated_bound(ref64, ref32, dt), f'GATE {dt} scatter_add n {n} d {d}')
    assert _same_bits(got[other], fill[other]), f'scatter-add touched a row outside the index n {n} d {d}'
  print(f'  rows branch: rows_idx {dt} d {d} -> vector (the only kernel)')


@pytest.mark.parametrize('dtype,d', MOVER_WIDTHS + [(t, d) for t in DTYPES for d in (5, 100)])
def test_rows_strided(lib, dtype, d):
  """strided gather and strided add (element-wise kernels, any width) at strides 1, 2 and 151"""
  dt = _dt(dtype)
  for n in MOVER_N:
    for stride in (1, 2, 151):
      if n == 5000 and stride == 151 and d > 12:
        continue
      g = _gen(n, d, dtype, stride)
      R = (n - 1) * stride + 2                                   # one row after the last one touched
      rows = torch.arange(n) * stride
      src = torch.randn(R, d, generator=g).to(dt)
      srcd = src.cuda()
      dst, _ = _filled(n, d, dt, g, 'strided gather dst')
      assert lib.spa3d_op_rows(GATHER_STRIDED, srcd.data_ptr(), None, stride, dst.data_ptr(), n, d, dtype, _s()) == 0
      PU.check_guards()
      assert _same_bits(dst, src[rows]), f'strided gather n {n} d {d} stride {stride}'
      add = torch.randn(n, d, generator=g).to(dt)
      addd = add.cuda()
      dst, fill = _filled(R, d, dt, g, 'strided add dst')
      assert lib.spa3d_op_rows(ADD_STRIDED, addd.data_ptr(), None, stride, dst.data_ptr(), n, d, dtype, _s()) == 0
      PU.check_guards()
      got = dst.cpu()
      ref64, ref32 = fill[rows].double() + add.double(), fill[rows].float() + add.float()
      PU.assert_elementwise(got[rows], ref64, PU.restated_bound(ref64, ref32, dt), f'GATE {dt} add_strided n {n} d {d} stride {stride}')
      other = torch.ones(R, dtype=torch.bool)
      other[rows] = False
      assert _same_bits(got[other], fill[other]), f'strided add touched a row between the strides n {n} d {d} stride {stride}'
  print(f'  rows branch: gather_rows / add_rows_strided {dt} d {d} -> scalar (the only kernel)')


@pytest.mark.parametrize('dtype', DTYPES)
def test_broadcast_rows(lib, dtype):
  """every copy equals the fp32 source rounded once"""
  dt = _dt(dtype)
  for rows, d, B in ((1, 8, 1), (3, 100, 5), (16, 384, 64)):
    g = _gen(rows, d, B)
    src = torch.randn(rows, d, generator=g)
    srcd = src.cuda()
    dst, _ = _filled(B * rows, d, dt, g, 'broadcast dst')
    assert lib.spa3d_op_broadcast_rows(srcd.data_ptr(), rows, d, dst.data_ptr(), B, dtype, _s()) == 0
    PU.check_guards()
    assert _same_bits(dst, src.to(dt).repeat(B, 1)), f'broadcast rows {rows} d {d} B {B}'


# ================================================================================================ readout assembly and the shared rows (copies)
def _frame_pool(Cl):
  last = (Cl - 1) // 5            # the last frame whose window [5 t, 5 t + W) still overlaps [0, Cl); one past it the window is all zeros
  return [0, 1, 3, last, last + 1]


def _frames(Cl, B, Q, k):
  pool = _frame_pool(Cl)
  return torch.tensor([pool[(2 * i + k) % 5] for i in range(B * Q)], dtype=torch.int32).reshape(B, Q)


def _assemble(lib, dtype, qtok_ptr, latd, qfd, B, Q, L, Cl, D, g):
  seq, _ = _filled(B * Q * (1 + L), D, _dt(dtype), g, 'seq')
  assert lib.spa3d_op_assemble_readout(qtok_ptr, latd.data_ptr(), qfd.data_ptr(), B, Q, L, Cl, D, seq.data_ptr(), dtype, _s()) == 0
  PU.check_guards()
  return seq.cpu().reshape(B, Q, 1 + L, D)


def _device_plan(lib, qfd, B, Q):
  n = B * Q
  bufs = [torch.full((n,), -7, dtype=torch.int32, device='cuda') for _ in range(4)]
  scratch = torch.zeros(n + B + 1, dtype=torch.int32, device='cuda')
  nslot = C.c_int64(-1)
  assert lib.spa3d_op_share_plan(qfd.data_ptr(), B, Q, *[b.data_ptr() for b in bufs], scratch.data_ptr(), C.byref(nslot), _s()) == 0
  return bufs, int(nslot.value)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('pair', PAIRS, ids=lambda p: f'{p[0]}-{p[1]}')
def test_assemble_and_shared_rows_are_copies(lib, dtype, pair):
  """assemble_readout (vector kernel), share_assemble and share_expand without `add` against the eye-einsum reference, bit for bit; then the composition on the
  device: expand(share_assemble(...)) under the device's own plan is assemble_readout(...)"""
  dt = _dt(dtype)
  Cl, D = pair
  k = 0
  for L in (1, 4):
    for B in (1, 2):
      for Q in (1, 9):
        g = _gen(Cl, L, B, Q, dtype)
        qf = _frames(Cl, B, Q, k); k += 1
        qtok = torch.randn(B * Q, D, generator=g).to(dt)
        lat = torch.randn(B, L, Cl, generator=g).to(dt)
        qtokd, latd, qfd = qtok.cuda(), lat.cuda(), qf.cuda()
        want = RU.assemble_ref(qtok.reshape(B, Q, D), lat, qf, D)
        seq = _assemble(lib, dtype, qtokd.data_ptr(), latd, qfd, B, Q, L, Cl, D, g)
        tag = f'(Cl, D) {pair} L {L} B {B} Q {Q} frames {qf.reshape(-1).tolist()}'
        assert _same_bits(seq, want), f'assemble_readout {tag}'
        plan = RU.slot_plan_ref(qf.numpy())
        (slot, slot_b, slot_f, slot_q0), nslot = _device_plan(lib, qfd, B, Q)
        assert nslot == plan[4] and np.array_equal(slot.cpu().numpy(), plan[0]) and np.array_equal(slot_b.cpu().numpy()[:nslot], plan[1])
        U = nslot * L + B * Q
        xU, _ = _filled(U, D, dt, g, 'xU')
        rc = lib.spa3d_op_share_rows(SHARE_ASSEMBLE, qtokd.data_ptr(), latd.data_ptr(), None, slot_b.data_ptr(), slot_f.data_ptr(), None, nslot, B, Q, L, Cl, D,
                                     xU.data_ptr(), dtype, _s())
        assert rc == 0
        PU.check_guards()
        assert _same_bits(xU, RU.share_assemble_ref(qtok, lat, plan, D)), f'share_assemble {tag}'
        out, _ = _filled(B * Q * (1 + L), D, dt, g, 'expanded')
        rc = lib.spa3d_op_share_rows(SHARE_EXPAND, xU.data_ptr(), None, slot.data_ptr(), None, None, slot_q0.data_ptr(), nslot, B, Q, L, 0, D, out.data_ptr(),
                                     dtype, _s())
        assert rc == 0
        PU.check_guards()
        assert _same_bits(out.cpu().reshape(B, Q, 1 + L, D), seq), f'expand(share_assemble) != assemble_readout {tag}'
        assert _same_bits(out.cpu().reshape(B, Q, 1 + L, D), want)
  print(f'  rows branch: assemble_readout {dt} (Cl, D) {pair} -> vector; share_assemble, share_expand -> vector (the only kernels)')


@pytest.mark.parametrize('dtype', DTYPES)
def test_assemble_scalar_kernel(lib, dtype):
  """assemble_kernel taken three ways: Cl no multiple of 16 bytes (18, 40), D no multiple (24, 42), qtok offset by one element at (24, 40) -- the last
  bit-identical to the vector kernel's result on the same data"""
  dt = _dt(dtype)
  k = 0
  for (Cl, D), off in (((18, 40), 0), ((24, 42), 0), ((24, 40), 1)):
    for L, B, Q in ((1, 1, 1), (4, 2, 9)):
      g = _gen(Cl, D, L, B, Q, off)
      qf = _frames(Cl, B, Q, k); k += 1
      raw = torch.randn(B * Q * D + off, generator=g).to(dt)
      lat = torch.randn(B, L, Cl, generator=g).to(dt)
      rawd, latd, qfd = raw.cuda(), lat.cuda(), qf.cuda()
      qtok = raw[off:].reshape(B * Q, D)
      ptr = rawd.data_ptr() + off * raw.element_size()
      assert Cl % _nv(dtype) or D % _nv(dtype) or ptr % 16, 'this case would take the vector kernel'
      seq = _assemble(lib, dtype, ptr, latd, qfd, B, Q, L, Cl, D, g)
      assert _same_bits(seq, RU.assemble_ref(qtok.reshape(B, Q, D), lat, qf, D)), f'scalar assemble (Cl, D) ({Cl}, {D}) offset {off} L {L} B {B} Q {Q}'
      if off:
        aligned = qtok.clone().cuda()
        assert aligned.data_ptr() % 16 == 0
        assert _same_bits(seq, _assemble(lib, dtype, aligned.data_ptr(), latd, qfd, B, Q, L, Cl, D, g)), 'scalar and vector kernels disagree on the same data'
      print(f'  rows branch: assemble_readout {dt} (Cl, D) ({Cl}, {D}) qtok offset {off} -> scalar')


# ================================================================================================ readout assembly backward
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('pair', PAIRS, ids=lambda p: f'{p[0]}-{p[1]}')
def test_assemble_backward(lib, dtype, pair):
  """dqtok is a copy; dlat (fp32) is the sum over the sample's queries of both parts, Q = 1, 3, 4, 5, 9 around the four-chain unroll; accumulate = 1 adds to the
  fill; two launches give the same bits (a fixed order, no atomics)"""
  dt = _dt(dtype)
  Cl, D = pair
  k = 0
  for L in (1, 4):
    for B in (1, 2):
      for Q in (1, 3, 4, 5, 9):
        g = _gen(Cl, L, B, Q, dtype, 1)
        qf = _frames(Cl, B, Q, k); k += 1
        dseq = torch.randn(B, Q, 1 + L, D, generator=g).to(dt)
        dseqd, qfd = dseq.cuda(), qf.cuda()
        dq_ref, dl_ref = RU.assemble_bwd_ref(dseq, qf, Cl)
        addends = RU.assemble_bwd_addends(dseq, qf, Cl)
        for acc in (0, 1):
          runs = []
          for _ in range(2):
            dqtok, _f = _filled(B * Q, D, dt, g, 'dqtok')
            dlat, fill = _filled(B * L, Cl, torch.float32, _gen(Cl, L, B, Q, acc), 'dlat')
            rc = lib.spa3d_op_assemble_readout_bwd(dseqd.data_ptr(), qfd.data_ptr(), B, Q, L, Cl, D, dqtok.data_ptr(), dlat.data_ptr(), acc, dtype, _s())
            assert rc == 0
            PU.check_guards()
            runs.append(dlat.cpu())
          tag = f'(Cl, D) {pair} L {L} B {B} Q {Q} accumulate {acc}'
          assert _same_bits(dqtok.cpu().reshape(B, Q, D), dq_ref), f'dqtok {tag}'
          first = fill.reshape(-1) if acc else torch.zeros(B * L * Cl)
          ref64 = first.double() + dl_ref.reshape(-1)
          PU.assert_elementwise(runs[0].reshape(-1), ref64, _sum_gate(first, addends, ref64), f'GATE {dt} assemble_bwd_dlat {tag}')
          assert _same_bits(runs[0], runs[1]), f'two launches of the dlat sum differ {tag}'


# ================================================================================================ shared rows: reduce, expand with add
def _slots(pattern, B, Q, g):
  """frames per query -> the plan; 'one': every query its own slot, 'all': one slot per sample, 'mix': a few frames, slots of 1 .. many members"""
  if pattern == 'one':
    qf = torch.stack([torch.randperm(Q, generator=g) for _ in range(B)])
  elif pattern == 'all':
    qf = torch.full((B, Q), 3)
  else:
    qf = torch.randint(0, max(2, min(7, Q // 2)), (B, Q), generator=g)
  return RU.slot_plan_ref(qf.numpy().astype(np.int32))


def _reduce_restated_err(src, slot, nslot, ref64):
  """worst error of the float32 restatement of the slot sums (members added one after the other, in ascending and in descending query order) against fp64"""
  L = src.shape[1] - 1
  idx = torch.as_tensor(slot, dtype=torch.int64)
  e = 0.0
  for flip in (False, True):
    s, i = (src.flip(0), idx.flip(0)) if flip else (src, idx)
    acc = torch.zeros(nslot, L, src.shape[2])
    for m in range(s.shape[0]):            # one member after the other: index_add_ leaves the order open
      acc[i[m]] += s[m, 1:].float()
    e = max(e, float((acc.double().reshape(nslot * L, -1) - ref64[:nslot * L]).abs().max()))
  return e


def _reduce(lib, dtype, srcd, slotd, slot_bd, nslot, B, Q, L, d, g):
  out, _ = _filled(nslot * L + B * Q, d, _dt(dtype), g, 'reduced')
  rc = lib.spa3d_op_share_rows(SHARE_REDUCE, srcd.data_ptr(), None, slotd.data_ptr(), slot_bd.data_ptr(), None, None, nslot, B, Q, L, 0, d, out.data_ptr(), dtype, _s())
  assert rc == 0
  PU.check_guards()
  return out.cpu()


def _expand(lib, dtype, srcUd, addd, slotd, slot_q0d, nslot, B, Q, L, d, g):
  out, _ = _filled(B * Q * (1 + L), d, _dt(dtype), g, 'expanded')
  rc = lib.spa3d_op_share_rows(SHARE_EXPAND, srcUd.data_ptr(), addd.data_ptr() if addd is not None else None, slotd.data_ptr(), None, None, slot_q0d.data_ptr(), nslot,
                               B, Q, L, 0, d, out.data_ptr(), dtype, _s())
  assert rc == 0
  PU.check_guards()
  return out.cpu().reshape(B * Q, 1 + L, d)


SHARE_WIDTHS = [(F32, 4), (F32, 1152)] + [(t, d) for t in (BF16, F16) for d in (8, 48, 1152)]


@pytest.mark.parametrize('dtype,d', SHARE_WIDTHS)
def test_share_reduce_and_expand_add(lib, dtype, d):
  """Q around the 256-query chunks of the member list (255, 256, 257, 600: one, two and three chunks), two samples (one at Q = 600); slots of one member, of every query of the
  sample, and a mix.  Reduce: fp32 sums in ascending member order, two launches bit-identical, the token-0 rows a copy.  Expand with add: rows of a slot's
  non-first members equal `add` bit for bit, the first member's and every token 0 equal add + src"""
  dt = _dt(dtype)
  for Q in (1, 8, 255, 256, 257, 600):
    B = 1 if Q == 600 else 2      # (the sample index b Q + q is exercised at every other Q; one sample keeps the largest case small)
    for L in (1, 4):
      for pattern in ('one', 'all', 'mix'):
        g = _gen(Q, L, d, dtype, ('one', 'all', 'mix').index(pattern))
        slot, slot_b, slot_f, slot_q0, nslot = _slots(pattern, B, Q, g)
        slotd, slot_bd, slot_q0d = _i32(slot), _i32(slot_b), _i32(slot_q0)
        nseq, U = B * Q, nslot * L + B * Q
        tag = f'Q {Q} L {L} d {d} slots {pattern} ({nslot})'
        src = torch.randn(nseq, 1 + L, d, generator=g).to(dt)
        srcd = src.cuda()
        ref64 = RU.share_reduce_ref(src, slot, nslot)
        got = _reduce(lib, dtype, srcd, slotd, slot_bd, nslot, B, Q, L, d, g)
        bound = _bound16(ref64[:nslot * L], 4.0 * _reduce_restated_err(src, slot, nslot, ref64), dt)
        PU.assert_elementwise(got[:nslot * L], ref64[:nslot * L], bound, f'GATE {dt} share_reduce {tag}')
        assert _same_bits(got[nslot * L:], src[:, 0]), f'share_reduce token-0 rows {tag}'
        assert _same_bits(got, _reduce(lib, dtype, srcd, slotd, slot_bd, nslot, B, Q, L, d, g)), f'two launches of share_reduce differ {tag}'
        srcU = torch.randn(U, d, generator=g).to(dt)
        add = torch.randn(nseq, 1 + L, d, generator=g).to(dt)
        out = _expand(lib, dtype, srcU.cuda(), add.cuda(), slotd, slot_q0d, nslot, B, Q, L, d, g)
        ref64, take = RU.share_expand_add_ref(srcU, add, slot, slot_q0, nslot, L)
        ref32 = add.float() + RU.share_expand_ref(srcU, slot, nslot, L).float() * take[..., None]
        assert _same_bits(out[~take], add[~take]), f'share_expand with add changed a non-first member {tag}'
        PU.assert_elementwise(out[take], ref64[take], PU.restated_bound(ref64[take], ref32[take], dt), f'GATE {dt} share_expand_add {tag}')
  print(f'  rows branch: share_reduce {dt} d {d} -> member-list chunks 1 (Q <= 256), 2 (257), 3 (600); share_expand ADD')


@pytest.mark.parametrize('dtype', DTYPES)
def test_share_reduce_is_the_transpose_of_expand_exactly(lib, dtype):
  """<expand(u), v> == <u, reduce(v)> on the device with |u|, |v| <= 4 and at most 60 members per slot: every sum is an integer below 256, exact in bf16, fp16
  and fp32, so both sides are computed from the device's outputs in int64 and must be EQUAL; expand and reduce equal their references bit for bit too"""
  dt = _dt(dtype)
  d, B = 8 * 3, 2
  for Q, L, pattern in ((8, 1, 'all'), (60, 4, 'all'), (60, 1, 'mix'), (9, 4, 'one')):
    g = _gen(Q, L, ('one', 'all', 'mix').index(pattern), dtype)
    slot, slot_b, slot_f, slot_q0, nslot = _slots(pattern, B, Q, g)
    slotd, slot_bd, slot_q0d = _i32(slot), _i32(slot_b), _i32(slot_q0)
    U = nslot * L + B * Q
    u = torch.randint(-4, 5, (U, d), generator=g).to(dt)
    v = torch.randint(-4, 5, (B * Q, 1 + L, d), generator=g).to(dt)
    eu = _expand(lib, dtype, u.cuda(), None, slotd, slot_q0d, nslot, B, Q, L, d, g)
    rv = _reduce(lib, dtype, v.cuda(), slotd, slot_bd, nslot, B, Q, L, d, g)
    assert _same_bits(eu, RU.share_expand_ref(u, slot, nslot, L)) and torch.equal(rv.double(), RU.share_reduce_ref(v, slot, nslot))
    lhs = int((eu.double() * v.double()).sum().to(torch.int64))
    rhs = int((u.double() * rv.double()).sum().to(torch.int64))
    assert lhs == rhs, f'adjoint identity Q {Q} L {L} slots {pattern}: {lhs} != {rhs}'


# ================================================================================================ parameter-row gradient
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('per', [1, 255, 256, 257, 6144])
def test_bcast_grad(lib, dtype, per):
  """B = 1 .. 63 is one slice of samples (a plain dparam += s), 64 is where the launcher splits and adds by float atomics; rows of `per` and of per + 40 elements
  (the gap holds values); dparam is pre-filled"""
  dt = _dt(dtype)
  for B in (1, 3, 4, 5, 63, 64, 65, 5000):
    g = _gen(B, per, dtype)
    vals = torch.randn(B, per, generator=g).to(dt)
    fill = torch.randn(per, generator=g)
    ref64 = fill.double() + vals.double().sum(0)
    gate = _sum_gate(fill, vals, ref64)
    for bstride in (per, per + 40):
      buf = torch.randn(B, bstride, generator=g).to(dt)
      buf[:, :per] = vals
      bufd = buf.cuda()
      dparam = PU.guarded(1, per, torch.float32, name='dparam', fill=0)
      dparam.copy_(fill[None])
      assert lib.spa3d_op_bcast_grad(bufd.data_ptr(), per, B, bstride, dparam.data_ptr(), dtype, _s()) == 0
      PU.check_guards()
      PU.assert_elementwise(dparam[0], ref64, gate, f'GATE {dt} bcast_grad B {B} per {per} bstride {bstride}')
    gy = max(1, min(B // 32, max(1, 2048 // ((per + 255) // 256))))
    print(f'  rows branch: bcast_grad {dt} B {B} per {per} -> {"single slice" if gy == 1 else "atomic"}')


# ================================================================================================ visible-frame pooling
def _vis(nseq, T, g, first):
  """pattern (first + s) % 5 for sequence s: all frames, none, one frame, Bernoulli(0.5), non-unit values (2.0 and -1.0 count as 1)"""
  vis = torch.zeros(nseq, T)
  for s in range(nseq):
    p = (first + s) % 5
    if p == 0:
      vis[s] = 1.0
    elif p == 2:
      vis[s, int(torch.randint(0, T, (1,), generator=g))] = 1.0
    elif p == 3:
      vis[s] = (torch.rand(T, generator=g) < 0.5).float()
    elif p == 4:
      m = torch.rand(T, generator=g)
      vis[s] = torch.where(m < 0.3, torch.tensor(2.0), torch.where(m < 0.6, torch.tensor(-1.0), torch.tensor(0.0)))
  return vis


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('T', [1, 24, 150])
def test_vis_mean_pool_and_backward(lib, dtype, T):
  """sequence s carries visibility pattern s % 5 (a single sequence runs the five one after the other); a sequence without a visible frame gives exactly 0 in the
  output and in the gradient; the float32 restatement adds the frames in time order"""
  dt = _dt(dtype)
  for d in (8, 100, 384):
    for nseq in (1, 5, 300):
      for first in (range(5) if nseq == 1 else (0,)):
        g = _gen(T, d, nseq, first, dtype)
        vis = _vis(nseq, T, g, first)
        tok = torch.randn(nseq, T, d, generator=g).to(dt)
        dout = torch.randn(nseq, d, generator=g)
        dout = (torch.sign(dout) * (0.05 + dout.abs())).to(dt)   # |dout| / T stays a normal fp16 number: the gate's u |ref| is a rounding, not an underflow
        tokd, visd, doutd = tok.cuda(), vis.cuda(), dout.cuda()
        keep = (vis != 0).float()
        cnt = keep.sum(1).clamp_min(1.0)
        none = keep.sum(1) == 0
        tag = f'T {T} d {d} nseq {nseq} first pattern {first}'
        out, _ = _filled(nseq, d, dt, g, 'pooled')
        assert lib.spa3d_op_vis_mean_pool(tokd.data_ptr(), visd.data_ptr(), nseq, T, d, out.data_ptr(), dtype, _s()) == 0
        PU.check_guards()
        ref64 = RU.vis_mean_pool_ref(tok, vis)
        terms = (tok.float() * keep[..., None]).permute(1, 0, 2).reshape(T, nseq * d)
        ref32 = PU.sequential_sum(torch.zeros(nseq * d), terms, torch.float32).reshape(nseq, d) / cnt[:, None]
        got = out.cpu()
        PU.assert_elementwise(got, ref64, PU.restated_bound(ref64, ref32, dt), f'GATE {dt} vis_mean_pool {tag}')
        assert torch.equal(got[none].float(), torch.zeros(int(none.sum()), d)), f'a sequence without a visible frame is not exactly 0 {tag}'
        dtok, _ = _filled(nseq * T, d, dt, g, 'dtok')
        assert lib.spa3d_op_vis_mean_pool_bwd(doutd.data_ptr(), visd.data_ptr(), nseq, T, d, dtok.data_ptr(), dtype, _s()) == 0
        PU.check_guards()
        ref64 = RU.vis_mean_pool_bwd_ref(dout, vis)
        ref32 = dout.float()[:, None, :] * keep[..., None] / cnt[:, None, None]
        got = dtok.cpu().reshape(nseq, T, d)
        PU.assert_elementwise(got, ref64, PU.restated_bound(ref64, ref32, dt), f'GATE {dt} vis_mean_pool_bwd {tag}')
        assert torch.equal(got[keep == 0].float(), torch.zeros(int((keep == 0).sum()), d)), f'an invisible frame has a gradient {tag}'
