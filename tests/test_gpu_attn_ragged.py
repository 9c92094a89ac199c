"""The two ragged forms of the fused attention on their own (csrc/attention_fused.hip), through spa3d_op_attention_ragged(_bwd) and
spa3d_op_attention_varlen(_bwd):

  * ragged self-attention (AttnArgs::seq_off / AttnBwdArgs::seq_off; the track encoder under token pruning): sequence i is rows [off[i], off[i + 1]) of the
    packed q | k | v, its lse at ((off[i] H + h S_i) + t) 2; the instance comes from the longest length S, the tile counts from S_i;
  * cross attention over ragged key sets (koff; tracks_to_latents with per-sample support counts): xattn_fwd_kernel with koff and its own backward instance
    attn_bwd8_kernel<8, true, false, true>, whose empty chunks leave the launcher's zeroed dq^ partials; fp32 / impl 1 loop over the sequences.

Every case: outputs in canary-guarded allocations of EXACTLY total_rows rows (PU.guarded: a store into the (rows + 7) & ~7 tail the model allocates trips a
canary), o / lse / dq / dk / dv NaN-filled (a slot nobody writes shows), dsq / dsk zero-filled, a poisoned workspace; the fp64 oracle (_attn_ref of
tests/test_gpu_ops.py) and the host emulations of the rounding contract (tests/parity_util.py) run one sequence at a time, rows concatenated, dsq / dsk summed
over the sequences in fp64; the row gates are the project's (2 x the emulation's worst, both against the oracle), the whole-tensor limits those of
test_attention_fused_fwd_bwd / test_attention_fused_cross (2e-2 / 3e-2 bf16, 4e-3 / 6e-3 fp16).

Dense comparison, per case family:
  * ragged self-attention forward, every case and both dtypes, masked or not: o and both lse slots of every sequence with S_i >= 2 are BIT-EQUAL to
    spa3d_op_attention(nseq = 1, Sq = Sk = S_i, impl 2) -- although the dense call runs another instance (KT from S_i, four or eight waves, the nine-tile or the
    WIDE store form).  What carries it: a key's logit is three k = 32 MFMAs over Dh whatever the instance; a padding key's bias is -inf, so exp gives an exact
    0 that adds nothing to the lane's l (same kt order, zeros appended) and its V row is stored as zeros, so the extra P.V products are 0 x 0 added to the
    accumulator; the nine-tile instance feeds tile 8 with zeros in the upper half of k, which is what the ten-tile instance's empty tile 9 is.
  * ragged-key cross attention forward: o and lse of sequence i BIT-EQUAL to spa3d_op_attention on that sequence's key slice (no count equals Sq, so the
    dense call takes the chunked kernel too: same 128-key chunks from the same first key, and a chunk past the keys is the neutral partial m = -inf, l = 0 that
    the combine step weighs with exp(-inf) = 0 -- it adds 0 to L and 0 x 0 to the sums); the uniform case also against ONE dense call over all sequences.
  * backward: no bit comparison (dsq / dsk are float atomics; rows are gated against the emulation).
The Gates tables of the first green run: profiles/r20_attn_ragged.log."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity_util as PU
from test_gpu_ops import _attn_ref
from util import Gates, max_abs, rel_err

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2
DH = 96
ALPHA = 0.10206207261596575


@pytest.fixture(scope='module')
def lib():
  import spa3d
  return spa3d._lib.load()


def _s():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(dtype):
  return {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}[dtype]


def _i32(v):
  a = np.ascontiguousarray(v, dtype=np.int32)
  return a.ctypes.data_as(C.POINTER(C.c_int32)), a


def _bits(t):
  return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
  return torch.equal(_bits(a), _bits(b))   # (NaN == NaN by bits: an unwritten slot on both sides is caught by the NaN checks, not here)


def _ptr(t):
  return None if t is None else t.data_ptr()


def _fwd_limit(dtype):
  return 2e-2 if dtype == BF16 else 4e-3


def _bwd_limit(dtype):
  return 3e-2 if dtype == BF16 else 6e-3


# ================================================================================================ ragged self-attention
SELF_CASES = {   # S (instance): (H, lengths)
    151: (8, (151, 1, 2, 16, 17, 33, 150, 97, 64)),    # KT 10, the T = 150 model; nseq = 9: the XCD-major map's tail
    129: (8, (129, 128, 113, 1, 16)),                  # the forward's nine-tile instance
    301: (2, (301, 1, 17, 160, 161, 300, 129, 2, 288)),   # KT 20, eight waves
    40: (2, (40, 3, 17)),
}
PROBE_LENS = (16, 17, 33, 151)
_cache = {}


class _SelfCase:
  """inputs, the fp64 oracle and the forward emulation of one ragged self-attention case, computed once and shared (never modified) by the tests"""

  def __init__(self, S, H, lens, dtype, masked=False, probe=False):
    self.S, self.H, self.lens, self.dtype, self.dt, self.masked = S, H, tuple(lens), dtype, _dt(dtype), masked
    self.E = E = H * DH
    self.off = [0]
    for n in lens:
      self.off.append(self.off[-1] + n)
    self.rows, self.nseq = self.off[-1], len(lens)
    g = torch.Generator().manual_seed(1000 * S + 10 * H + dtype + (5 if masked else 0))
    if probe:   # sequence 2j / 2j + 1 of length PROBE_LENS[j]: head 0 probes key 0 / S_i - 1, head 1 the other end
      parts = []
      for i, n in enumerate(lens):
        pos = [0, n - 1] if i % 2 == 0 else [n - 1, 0]
        q, k, v = PU.probe_inputs(1, n, n, H, DH, self.dt, [pos], seed=7 * n + i)
        parts.append(torch.cat([q[0], k[0], v[0]], dim=1))
      self.qkv = torch.cat(parts, dim=0)
    else:
      self.qkv = torch.randn(self.rows, 3 * E, generator=g).to(self.dt)
    self.sq = 1 + 0.2 * torch.randn(DH, generator=g)
    self.sk = 1 + 0.2 * torch.randn(DH, generator=g)
    self.d_o = torch.randn(self.rows, E, generator=g).to(self.dt)
    self.km = None
    if masked:   # PACKED key mask [rows]: first row of every sequence visible, about 80 % elsewhere, sequence 5 (33 rows) with only its first key
      self.km = (torch.rand(self.rows, generator=g) < 0.8).float()
      self.km[self.off[:-1]] = 1.0
      self.km[self.off[5] + 1:self.off[6]] = 0.0
    self.q, self.k, self.v = (self.qkv[:, j * E:(j + 1) * E].contiguous() for j in range(3))
    sqr, skr = self.sq.double().requires_grad_(True), self.sk.double().requires_grad_(True)
    o_ref, gq, gk, gv, emu = [], [], [], [], []
    for i in range(self.nseq):
      sl = self.seq(i)
      qr, kr, vr = (t[sl].double()[None].requires_grad_(True) for t in (self.q, self.k, self.v))
      ref = _attn_ref(qr, kr, vr, sqr, skr, self.km_of(i), H, DH)
      ref.backward(self.d_o[sl].double()[None])
      o_ref.append(ref.detach()[0]); gq.append(qr.grad[0]); gk.append(kr.grad[0]); gv.append(vr.grad[0])
      emu.append(PU.emulate_attention(self.q[sl][None], self.k[sl][None], self.v[sl][None], self.sq, self.sk, self.km_of(i), H, DH)[0])
    self.o_ref, self.o_emu = torch.cat(o_ref), torch.cat(emu)
    self.grads_ref = (torch.cat(gq), torch.cat(gk), torch.cat(gv), sqr.grad, skr.grad)
    self._emu_bwd = {}

  def seq(self, i):
    return slice(self.off[i], self.off[i + 1])

  def km_of(self, i):
    return None if self.km is None else self.km[self.seq(i)][None]

  def emu_bwd(self, fast):
    """emulate_attention_bwd one sequence at a time: rows concatenated, dsq / dsk summed over the sequences in fp64"""
    if fast not in self._emu_bwd:
      parts = [PU.emulate_attention_bwd(self.q[self.seq(i)][None], self.k[self.seq(i)][None], self.v[self.seq(i)][None], self.sq, self.sk, self.km_of(i), self.H,
                                        DH, self.d_o[self.seq(i)][None], fast=fast) for i in range(self.nseq)]
      self._emu_bwd[fast] = tuple(torch.cat([p[j][0] for p in parts]) for j in range(3)) + tuple(sum(p[j].double() for p in parts) for j in (3, 4))
    return self._emu_bwd[fast]


def _self_case(S, dtype, masked=False):
  key = (S, dtype, masked)
  if key not in _cache:
    H, lens = SELF_CASES[S]
    _cache[key] = _SelfCase(S, H, lens, dtype, masked)
  return _cache[key]


def _probe_case(dtype):
  key = ('probe', dtype)
  if key not in _cache:
    _cache[key] = _SelfCase(151, 2, [n for n in PROBE_LENS for _ in range(2)], dtype, probe=True)
  return _cache[key]


class _Dev:
  """device copies of a case's inputs; q | k | v packed (ld = 3 E) with exactly total_rows rows inside the guards"""

  def __init__(self, c, qkv=None, d_o=None):
    self.qkv = PU.guarded(c.rows, 3 * c.E, c.dt, name='qkv')
    self.qkv.copy_(c.qkv if qkv is None else qkv)
    self.d_o = PU.guarded(c.rows, c.E, c.dt, name='d_o')
    self.d_o.copy_(c.d_o if d_o is None else d_o)
    self.sq, self.sk = c.sq.cuda(), c.sk.cuda()
    self.km = None if c.km is None else c.km.cuda()
    self.ws = PU.poisoned_ws(1 << 20)   # the device copy of the offsets; the LDS-resident kernels carve nothing


def _ragged_fwd(lib, c, d, impl=2):
  E = c.E
  o = PU.guarded(c.rows, E, c.dt, name='o')
  lse = PU.guarded(c.rows * c.H, 2, torch.float32, name='lse')
  offp, _keep = _i32(c.off)
  rc = lib.spa3d_op_attention_ragged(d.qkv.data_ptr(), d.qkv[:, E:].data_ptr(), d.qkv[:, 2 * E:].data_ptr(), 3 * E, 3 * E, 3 * E, d.sq.data_ptr(), d.sk.data_ptr(),
                                     _ptr(d.km), offp, c.nseq, c.S, c.H, DH, o.data_ptr(), lse.data_ptr(), c.dtype, impl, d.ws.data_ptr(), d.ws.numel(), _s())
  assert rc == 0
  PU.check_guards()
  return o, lse


def _ragged_bwd(lib, c, d, o, lse, impl):
  E = c.E
  dqkv = PU.guarded(c.rows, 3 * E, c.dt, name='dqkv')
  dsq = PU.guarded(1, DH, torch.float32, name='dsq', fill=0.0)[0]
  dsk = PU.guarded(1, DH, torch.float32, name='dsk', fill=0.0)[0]
  offp, _keep = _i32(c.off)
  rc = lib.spa3d_op_attention_ragged_bwd(d.qkv.data_ptr(), d.qkv[:, E:].data_ptr(), d.qkv[:, 2 * E:].data_ptr(), 3 * E, 3 * E, 3 * E, d.sq.data_ptr(),
                                         d.sk.data_ptr(), _ptr(d.km), offp, c.nseq, c.S, c.H, DH, o.data_ptr(), lse.data_ptr(), d.d_o.data_ptr(), dqkv.data_ptr(),
                                         dqkv[:, E:].data_ptr(), dqkv[:, 2 * E:].data_ptr(), dsq.data_ptr(), dsk.data_ptr(), c.dtype, impl, d.ws.data_ptr(),
                                         d.ws.numel(), _s())
  assert rc == 0
  PU.check_guards()
  return dqkv[:, :E], dqkv[:, E:2 * E], dqkv[:, 2 * E:], dsq, dsk


def _lse_of(c, lse, i):
  """lse of sequence i as [H, S_i, 2]: the documented ragged position ((off[i] H + h S_i) + t) 2"""
  return lse.reshape(-1)[c.off[i] * c.H * 2:c.off[i + 1] * c.H * 2].view(c.H, c.lens[i], 2)


def _check_forward(lib, c, d, o, lse, title):
  """the forward's gates: nothing unwritten, the whole-tensor limit, the row gate, length-1 sequences exactly, every longer sequence against the dense entry"""
  H, E = c.H, c.E
  assert not torch.isnan(o.float()).any() and not torch.isnan(lse).any()   # every o row and every one of the rows x H x 2 lse slots was written
  e = rel_err(o.float(), c.o_ref)
  print(f'{title}: forward rel err {e:.3e}')
  assert e < _fwd_limit(c.dtype)
  gt = Gates(f'{title}, forward: kernel vs host emulation per sequence, both against the fp64 oracle')
  PU.attention_row_gate(gt, 'o', o, c.o_emu, c.o_ref, H, DH)
  gt.check()
  qn, kn = PU._rmsnorm16(c.q[None], c.sq, 1, H, DH)[0].double(), PU._rmsnorm16(c.k[None], c.sk, 1, H, DH)[0].double()   # [rows, H, Dh]
  differ = []
  for i, n in enumerate(c.lens):
    r0 = c.off[i]
    li = _lse_of(c, lse, i).cpu()
    if n == 1:
      # one key: P = 1 exactly, so o is the v row bit for bit; lse = (the logit, log 1 = 0 exactly).  The logit within what one 16-bit ulp per element of q^ and
      # k^ (the device's rsqrt against the host's) and an fp32 sum of 96 products allow: (4 u + 4 (96 + 2) 2^-24) alpha sum |q^ k^|
      assert _same_bits(o[r0], d.qkv[r0, 2 * E:]), f'{title}: o of the length-1 sequence {i} is not its v row'
      assert torch.equal(li[:, 0, 1], torch.zeros(H)), f'{title}: log l of the length-1 sequence {i}: {li[:, 0, 1].tolist()}'
      logit = (qn[r0] * kn[r0]).sum(-1) * ALPHA
      tol = (4 * PU.unit_roundoff(c.dt) + PU.C_MFMA * (DH + 2) * PU.U_F32) * ALPHA * (qn[r0] * kn[r0]).abs().sum(-1)
      assert bool(((li[:, 0, 0].double() - logit).abs() <= tol).all()), f'{title}: logit of the length-1 sequence {i}: {li[:, 0, 0].tolist()} vs {logit.tolist()}'
      continue
    o2 = PU.guarded(n, E, c.dt, name='o dense')
    lse2 = PU.guarded(H * n, 2, torch.float32, name='lse dense')
    rc = lib.spa3d_op_attention(d.qkv[r0:].data_ptr(), d.qkv[r0:, E:].data_ptr(), d.qkv[r0:, 2 * E:].data_ptr(), 3 * E, 3 * E, 3 * E, d.sq.data_ptr(), d.sk.data_ptr(),
                                None if d.km is None else d.km[r0:].data_ptr(), 1, n, n, H, DH, o2.data_ptr(), lse2.data_ptr(), c.dtype, 2, d.ws.data_ptr(),
                                d.ws.numel(), _s())
    assert rc == 0
    PU.check_guards()
    assert not torch.isnan(o2.float()).any() and not torch.isnan(lse2).any()
    if not (_same_bits(o2, o[r0:r0 + n]) and _same_bits(lse2.view(H, n, 2), _lse_of(c, lse, i))):
      differ.append((i, n, rel_err(o[r0:r0 + n].float(), o2.float()), max_abs(_lse_of(c, lse, i), lse2.view(H, n, 2))))
  print(f'{title}: sequences that differ from the dense entry (index, length, rel err of o, max |d lse|): {differ}')
  assert not differ, f'{title}: not bit-equal to spa3d_op_attention on the sequence alone: {differ}'


def _check_backward(c, got, mode, title):
  """nothing unwritten or NaN in dq, dk, dv, dsq, dsk; prints and returns their whole-tensor relative errors.  The caller asserts the limit (the probe test
  applies none, as _probe of tests/test_gpu_ops.py); the row gates and the length-1 checks are _gate_backward."""
  H = c.H
  for name, t in zip(('dq', 'dk', 'dv', 'dsq', 'dsk'), got):
    assert not torch.isnan(t.float()).any(), f'{title}: {name} has unwritten or NaN elements'
  errs = [rel_err(a.float(), b) for a, b in zip(got, c.grads_ref)]
  print(f'{title}: backward mode {mode} rel errs dq dk dv dsq dsk', errs)
  return errs


def _gate_backward(c, got, mode, title):
  gb = Gates(f'{title}, backward mode {mode}: kernel vs host emulation per sequence, both against the fp64 oracle')
  PU.attention_grad_gates(gb, got, c.emu_bwd(mode == '1' and c.km is None), c.grads_ref, c.H, DH, S=c.S)
  gb.check()
  # length-1 sequences: dv is the d_o row bit for bit (P = 16-bit(exp(~0)) = 1, one query); dq and dk are zero up to the floor of a typical row
  floor = PU.grad_row_floor(c.dt, DH, c.S)
  shp = (c.rows, c.H, DH)
  for i, n in enumerate(c.lens):
    if n == 1:
      r0 = c.off[i]
      assert _same_bits(got[2][r0], c.d_o[r0].cuda()), f'{title}: dv of the length-1 sequence {i} is not its d_o row'
      for name, g, r in (('dq', got[0], c.grads_ref[0]), ('dk', got[1], c.grads_ref[1])):
        assert float(r[r0].abs().max()) < 1e-12   # the oracle: one key passes no gradient to q or k
        z = float(PU.row_errs_floored(g.reshape(shp), r.reshape(shp), floor)[r0].max())
        print(f'{title}: {name} of the length-1 sequence {i}: {z:.3e} of the floor')
        assert z <= 1.0, f'{title}: {name} of the length-1 sequence {i} is {z:.3f} x the floor of a typical row'


def _modes(S):
  return [('1', 2), ('2', 3), ('3', 4)] if S <= 160 else [('3', 4)]


@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('S', sorted(SELF_CASES))
def test_ragged_self_attention_forward(lib, S, dtype):
  c = _self_case(S, dtype)
  d = _Dev(c)
  o, lse = _ragged_fwd(lib, c, d)
  _check_forward(lib, c, d, o, lse, f'ragged self-attention, {c.dt} S {S} H {c.H} lengths {c.lens}')


@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('S', sorted(SELF_CASES))
def test_ragged_self_attention_backward(lib, S, dtype):
  """every backward structure the length has: four resident images (impl 2), split-pass on 4 / 8 waves (impl 3 / 4) up to S = 160, the 8-wave split-pass above"""
  c = _self_case(S, dtype)
  d = _Dev(c)
  o, lse = _ragged_fwd(lib, c, d)
  title = f'ragged self-attention, {c.dt} S {S} H {c.H} lengths {c.lens}'
  for mode, impl in _modes(S):
    got = _ragged_bwd(lib, c, d, o, lse, impl)
    assert max(_check_backward(c, got, mode, title)) < _bwd_limit(dtype)
    _gate_backward(c, got, mode, title)


@pytest.mark.parametrize('dtype', [BF16, F16])
def test_ragged_self_attention_packed_key_mask(lib, dtype):
  """The key mask of the ragged form is indexed by PACKED row (km[row0 + t]); the model passes none when it prunes, so only this test reaches it."""
  c = _self_case(151, dtype, masked=True)
  d = _Dev(c)
  o, lse = _ragged_fwd(lib, c, d)
  title = f'ragged self-attention with a packed key mask, {c.dt} S 151 H {c.H} lengths {c.lens}'
  _check_forward(lib, c, d, o, lse, title)
  for mode, impl in _modes(151):
    got = _ragged_bwd(lib, c, d, o, lse, impl)
    assert max(_check_backward(c, got, mode, title)) < _bwd_limit(dtype)
    _gate_backward(c, got, mode, title)


@pytest.mark.parametrize('dtype', [BF16, F16])
def test_ragged_self_attention_sequences_are_isolated(lib, dtype):
  """Rerun with every q / k / v / d_o / o row OUTSIDE one sequence set to NaN: the sequence's own o, lse, dq, dk, dv keep their bits (dsq / dsk, sums over all
  sequences, are excluded).  A read one row past a sequence's end lands in its packed neighbour, and only this test sees it.  Sequences: the length-1, the
  length-17 and the last of the S = 151 case."""
  c = _self_case(151, dtype)
  d = _Dev(c)
  o, lse = _ragged_fwd(lib, c, d)
  base = {impl: _ragged_bwd(lib, c, d, o, lse, impl) for _, impl in _modes(151)}
  for i in (1, 4, c.nseq - 1):
    sl = c.seq(i)
    outside = torch.ones(c.rows, dtype=torch.bool)
    outside[sl] = False
    qkv_n, do_n = c.qkv.clone(), c.d_o.clone()
    qkv_n[outside] = float('nan')
    do_n[outside] = float('nan')
    dn = _Dev(c, qkv_n, do_n)
    o_n, lse_n = _ragged_fwd(lib, c, dn)
    assert _same_bits(o_n[sl], o[sl]), f'o of sequence {i} changed with its neighbours'
    assert _same_bits(_lse_of(c, lse_n, i), _lse_of(c, lse, i)), f'lse of sequence {i} changed with its neighbours'
    assert not torch.isnan(o_n[sl].float()).any()
    o_in = PU.guarded(c.rows, c.E, c.dt, name='o in')   # the forward's o as the backward reads it, NaN outside the sequence
    o_in.copy_(o)
    o_in[outside.cuda()] = float('nan')
    for impl, b in base.items():
      got = _ragged_bwd(lib, c, dn, o_in, lse, impl)
      for name, g, r in zip(('dq', 'dk', 'dv'), got, b):
        assert not torch.isnan(g[sl].float()).any(), f'{name} of sequence {i}, impl {impl}: NaN from a neighbour'
        assert _same_bits(g[sl], r[sl]), f'{name} of sequence {i}, impl {impl}, changed with its neighbours'


@pytest.mark.parametrize('dtype', [BF16, F16])
def test_ragged_self_attention_probe(lib, dtype):
  """Dominant-key probes (PU.probe_inputs) one sequence at a time: the lengths 16, 17, 33 and 151 twice each, the dominant key of head 0 / head 1 at
  0 / S_i - 1 and the other way round.  Losing the first or last key of a short sequence inside the long instance moves every row of the head by O(1).  The
  gates of _probe (tests/test_gpu_ops.py): the forward limit and row gate, the backward row gates without a whole-tensor limit."""
  c = _probe_case(dtype)
  d = _Dev(c)
  o, lse = _ragged_fwd(lib, c, d)
  title = f'ragged self-attention probe, {c.dt} lengths {c.lens}'
  _check_forward(lib, c, d, o, lse, title)
  for mode, impl in _modes(151):
    got = _ragged_bwd(lib, c, d, o, lse, impl)
    _check_backward(c, got, mode, title)
    _gate_backward(c, got, mode, title)


# ================================================================================================ ragged-key cross attention
COUNTS = (13, 300, 1, 129, 127, 256, 257, 200)   # Skmax = 300: three 128-key chunks; sequences with one and two chunks first, in the middle and last


class _CrossCase:
  def __init__(self, Sq, H, Dh, counts, dtype, seed=33):
    self.Sq, self.H, self.Dh, self.counts, self.dtype, self.dt = Sq, H, Dh, tuple(counts), dtype, _dt(dtype)
    self.E = E = H * Dh
    self.nseq = len(counts)
    self.koff = [0]
    for n in counts:
      self.koff.append(self.koff[-1] + n)
    self.keys = self.koff[-1]
    g = torch.Generator().manual_seed(seed + Sq + dtype)
    self.q = torch.randn(self.nseq, Sq, E, generator=g).to(self.dt)
    self.kv = torch.randn(self.keys, 2 * E, generator=g).to(self.dt)
    self.sq = 1 + 0.2 * torch.randn(Dh, generator=g)
    self.sk = 1 + 0.2 * torch.randn(Dh, generator=g)
    self.d_o = torch.randn(self.nseq, Sq, E, generator=g).to(self.dt)
    self.k, self.v = self.kv[:, :E].contiguous(), self.kv[:, E:].contiguous()
    sqr, skr = self.sq.double().requires_grad_(True), self.sk.double().requires_grad_(True)
    qr = self.q.double().requires_grad_(True)
    o_ref, gk, gv = [], [], []
    for i in range(self.nseq):
      sl = self.keys_of(i)
      kr, vr = self.k[sl].double()[None].requires_grad_(True), self.v[sl].double()[None].requires_grad_(True)
      ref = _attn_ref(qr[i:i + 1], kr, vr, sqr, skr, None, H, Dh)
      ref.backward(self.d_o[i:i + 1].double())
      o_ref.append(ref.detach()); gk.append(kr.grad[0]); gv.append(vr.grad[0])
    self.o_ref = torch.cat(o_ref)
    self.grads_ref = (qr.grad, torch.cat(gk), torch.cat(gv), sqr.grad, skr.grad)

  def keys_of(self, i):
    return slice(self.koff[i], self.koff[i + 1])

  def emulate(self):
    """emulate_attention / emulate_attention_bwd with chunk = 128, one sequence at a time"""
    fw = [PU.emulate_attention(self.q[i:i + 1], self.k[self.keys_of(i)][None], self.v[self.keys_of(i)][None], self.sq, self.sk, None, self.H, self.Dh, chunk=128)
          for i in range(self.nseq)]
    bw = [PU.emulate_attention_bwd(self.q[i:i + 1], self.k[self.keys_of(i)][None], self.v[self.keys_of(i)][None], self.sq, self.sk, None, self.H, self.Dh,
                                   self.d_o[i:i + 1], chunk=128) for i in range(self.nseq)]
    return torch.cat(fw), (torch.cat([p[0] for p in bw]), torch.cat([p[1][0] for p in bw]), torch.cat([p[2][0] for p in bw]),
                           sum(p[3].double() for p in bw), sum(p[4].double() for p in bw))


def _varlen_run(lib, c, impl, ws_bytes):
  """forward and backward through the ragged-key entries -> device inputs, o, lse, (dq, dk, dv, dsq, dsk)"""
  E, Sq, H, Dh = c.E, c.Sq, c.H, c.Dh
  qd, kvd, sqd, skd, dod = c.q.cuda(), PU.guarded(c.keys, 2 * E, c.dt, name='kv'), c.sq.cuda(), c.sk.cuda(), c.d_o.cuda()
  kvd.copy_(c.kv)
  o = PU.guarded(c.nseq * Sq, E, c.dt, name='o').view(c.nseq, Sq, E)
  lse = PU.guarded(c.nseq * H * Sq, 2, torch.float32, name='lse').view(c.nseq, H, Sq, 2)
  ws = PU.poisoned_ws(ws_bytes)
  koffp, _keep = _i32(c.koff)
  rc = lib.spa3d_op_attention_varlen(qd.data_ptr(), kvd.data_ptr(), kvd[:, E:].data_ptr(), E, 2 * E, 2 * E, sqd.data_ptr(), skd.data_ptr(), koffp, c.nseq, Sq, H, Dh,
                                     o.data_ptr(), lse.data_ptr(), c.dtype, impl, ws.data_ptr(), ws.numel(), _s())
  assert rc == 0
  PU.check_guards()
  dq = PU.guarded(c.nseq * Sq, E, c.dt, name='dq').view(c.nseq, Sq, E)
  dkv = PU.guarded(c.keys, 2 * E, c.dt, name='dkv')
  dsq = PU.guarded(1, Dh, torch.float32, name='dsq', fill=0.0)[0]
  dsk = PU.guarded(1, Dh, torch.float32, name='dsk', fill=0.0)[0]
  rc = lib.spa3d_op_attention_varlen_bwd(qd.data_ptr(), kvd.data_ptr(), kvd[:, E:].data_ptr(), E, 2 * E, 2 * E, sqd.data_ptr(), skd.data_ptr(), koffp, c.nseq, Sq, H,
                                         Dh, o.data_ptr(), lse.data_ptr(), dod.data_ptr(), dq.data_ptr(), dkv.data_ptr(), dkv[:, E:].data_ptr(), dsq.data_ptr(),
                                         dsk.data_ptr(), c.dtype, impl, ws.data_ptr(), ws.numel(), _s())
  assert rc == 0
  PU.check_guards()
  return (qd, kvd, sqd, skd, ws), o, lse, (dq, dkv[:, :E], dkv[:, E:], dsq, dsk)


def _varlen_fused(lib, Sq, counts, dtype):
  H = 2
  c = _CrossCase(Sq, H, DH, counts, dtype)
  E, Skmax = c.E, max(counts)
  (qd, kvd, sqd, skd, ws), o, lse, got = _varlen_run(lib, c, 2, PU.cross_attention_ws_bytes(c.nseq, H, Sq, Skmax) + 4096)   # + the offsets
  title = f'ragged-key cross attention, {c.dt} Sq {Sq} H {H} key counts {c.counts}'
  assert not torch.isnan(o.float()).any() and not torch.isnan(lse).any()
  for name, t in zip(('dq', 'dk', 'dv', 'dsq', 'dsk'), got):
    assert not torch.isnan(t.float()).any(), f'{title}: {name} has unwritten or NaN elements'
  e = rel_err(o.float(), c.o_ref)
  errs = [rel_err(a.float(), b) for a, b in zip(got, c.grads_ref)]
  print(f'{title}: forward rel err {e:.3e}; backward rel errs dq dk dv dsq dsk {errs}')
  assert e < _fwd_limit(dtype) and max(errs) < _bwd_limit(dtype)
  # forward: sequence i bit for bit against the dense entry on its key slice (no count equals Sq: the chunked kernel on both sides)
  for i, n in enumerate(counts):
    k0 = c.koff[i]
    o2 = PU.guarded(Sq, E, c.dt, name='o dense')
    lse2 = PU.guarded(H * Sq, 2, torch.float32, name='lse dense')
    rc = lib.spa3d_op_attention(qd[i].data_ptr(), kvd[k0:].data_ptr(), kvd[k0:, E:].data_ptr(), E, 2 * E, 2 * E, sqd.data_ptr(), skd.data_ptr(), None, 1, Sq, n, H, DH,
                                o2.data_ptr(), lse2.data_ptr(), dtype, 2, ws.data_ptr(), ws.numel(), _s())
    assert rc == 0
    PU.check_guards()
    assert _same_bits(o2, o[i]), f'{title}: o of sequence {i} ({n} keys) differs from the dense call on its keys, rel {rel_err(o[i].float(), o2.float()):.3e}'
    assert _same_bits(lse2.view(H, Sq, 2), lse[i]), f'{title}: lse of sequence {i} ({n} keys) differs from the dense call on its keys'
  if len(set(counts)) == 1:   # uniform offsets: also ONE dense call over all sequences
    n = counts[0]
    o2 = PU.guarded(c.nseq * Sq, E, c.dt, name='o dense').view(c.nseq, Sq, E)
    lse2 = PU.guarded(c.nseq * H * Sq, 2, torch.float32, name='lse dense').view(c.nseq, H, Sq, 2)
    rc = lib.spa3d_op_attention(qd.data_ptr(), kvd.data_ptr(), kvd[:, E:].data_ptr(), E, 2 * E, 2 * E, sqd.data_ptr(), skd.data_ptr(), None, c.nseq, Sq, n, H, DH,
                                o2.data_ptr(), lse2.data_ptr(), dtype, 2, ws.data_ptr(), ws.numel(), _s())
    assert rc == 0
    PU.check_guards()
    assert _same_bits(o2, o) and _same_bits(lse2, lse), f'{title}: differs from one dense call over all sequences'
  # the row gates, emulation per sequence
  o_emu, emu = c.emulate()
  gt = Gates(f'{title}, forward: kernel vs host emulation per sequence, both against the fp64 oracle')
  PU.attention_row_gate(gt, 'o', o, o_emu, c.o_ref, H, DH)
  gt.check()
  gb = Gates(f'{title}, backward: kernel vs host emulation per sequence, both against the fp64 oracle')
  PU.attention_grad_gates(gb, got, emu, c.grads_ref, H, DH, S=max(Sq, Skmax))
  gb.check()
  # a sequence with ONE key: the softmax passes no gradient to q, so its dq rows are zero up to the floor (its chunks 1 and 2 are the launcher's zeros: a
  # partial that is not zero shows here); P = 1, so its dv row is the head-wise sum of the d_o rows: one 16-bit rounding of an fp32 sum of Sq terms
  floor = PU.grad_row_floor(c.dt, DH, max(Sq, Skmax))
  for i, n in enumerate(counts):
    if n == 1:
      assert float(c.grads_ref[0][i].abs().max()) < 1e-12
      shp = (c.nseq, Sq, H, DH)
      z = float(PU.row_errs_floored(got[0].reshape(shp), c.grads_ref[0].reshape(shp), floor)[i].max())
      print(f'{title}: dq of the one-key sequence {i}: {z:.3e} of the floor')
      assert z <= 1.0
      want = c.d_o[i].double().sum(0)
      PU.assert_elementwise(got[2][c.koff[i]], want, PU.elementwise_bound(want, c.d_o[i].double().abs().sum(0), Sq, c.dt), 'dv of the one-key sequence')


@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('Sq', [128, 37])
def test_ragged_key_cross_attention_fused(lib, Sq, dtype):
  _varlen_fused(lib, Sq, COUNTS, dtype)


@pytest.mark.parametrize('dtype', [BF16, F16])
def test_ragged_key_cross_attention_uniform_offsets(lib, dtype):
  _varlen_fused(lib, 128, (200, 200, 200), dtype)


@pytest.mark.parametrize('dtype,impl', [(F32, 0), (F32, 1), (BF16, 1)])
def test_ragged_key_cross_attention_generic(lib, dtype, impl):
  """fp32 and impl 1 run the sequences one by one through the generic composition: against the oracle with the limits of test_attention_fwd_bwd_generic"""
  c = _CrossCase(16, 2, 16, (9, 1, 40), dtype)
  _, o, lse, got = _varlen_run(lib, c, impl, 16 << 20)
  assert not torch.isnan(o.float()).any()
  for t in got:
    assert not torch.isnan(t.float()).any()
  if dtype == F32:
    assert max_abs(o, c.o_ref) < 1e-5
    for g, r in zip(got, c.grads_ref):
      assert rel_err(g.float(), r) < 1e-4
  else:
    assert rel_err(o.float(), c.o_ref) < 2e-2
    for g, r in zip(got, c.grads_ref):
      assert rel_err(g.float(), r) < 3e-2


def test_ragged_key_cross_attention_refuses_a_short_workspace(lib):
  """The entry sizes the workspace by a dry walk before its first launch: one that holds the offsets but not the chunked-key partials is SPA3D_ERR_WORKSPACE,
  and nothing was written -- o and lse keep their NaN fill, the workspace its poison."""
  c = _CrossCase(37, 2, DH, COUNTS, BF16)
  E = c.E
  qd, kvd, sqd, skd = c.q.cuda(), c.kv.cuda(), c.sq.cuda(), c.sk.cuda()
  o = PU.guarded(c.nseq * 37, E, c.dt, name='o')
  lse = PU.guarded(c.nseq * 2 * 37, 2, torch.float32, name='lse')
  ws = PU.poisoned_ws(8192)
  koffp, _keep = _i32(c.koff)
  rc = lib.spa3d_op_attention_varlen(qd.data_ptr(), kvd.data_ptr(), kvd[:, E:].data_ptr(), E, 2 * E, 2 * E, sqd.data_ptr(), skd.data_ptr(), koffp, c.nseq, 37, 2, DH,
                                     o.data_ptr(), lse.data_ptr(), BF16, 2, ws.data_ptr(), ws.numel(), _s())
  assert rc == 2
  PU.check_guards()
  assert bool(torch.isnan(o.float()).all()) and bool(torch.isnan(lse).all())
  assert bool((ws == 0xFF).all())
