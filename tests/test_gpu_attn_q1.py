"""GPU parity of the single-query attention of every stack's last block (csrc/attn_q1.hip) on its own, through spa3d_op_attention_q1 / spa3d_op_attention_q1_bwd:
every head width the file instantiates (Dh = 8, 16, 32, 64, 96, 128) in fp32, bf16 and fp16, on the 16-byte "vec" lane layout and on the scalar one, sequence
lengths around the 16-key pass (1, 15, 16, 17) up to the 320-key limit, ragged sequences, problem counts that leave waves of a workgroup idle and problem
counts past the grid caps (8192 workgroups forward, 4096 backward: the stride loops).

Reference: the fp64 oracle of tests/test_gpu_ops.py::test_attention_fwd_bwd_generic (O.rms_norm, O.dot_product_attention, autograd) with the query restricted
to row 0 of each sequence, ragged input sequence by sequence.  Gates:
  fp32    o and p0 max-abs 1e-5, every gradient relative (Frobenius) 1e-4: the bounds of test_attention_fwd_bwd_generic;
  16-bit  the kernels round nowhere between load and store, so every element of o, dq0, dk, dv within u_out |ref| + 4 x max |fp32 host restatement - fp64|
          (parity_util.restated_bound; the restatement is parity_util.attn_q1_restated in float32 on the 16-bit inputs, pinned to the oracle in float64 by
          tests/test_parity_gates_host.py); p0 max-abs 1e-5 against the fp64 softmax;
  dscale_q / dscale_k (every dtype) element-wise within 4 x the restatement's own worst error, as the LayerNorm dscale: the restatement adds the problems'
          contributions to the pre-filled vector one after the other in float32, which is what a chain of float atomics does; their arrival order is
          not fixed, so narrow vectors take the worst over several orders (parity_util.arrival_orders).
Exact facts: p0, dk, dv of a masked key are 0; dk and dv start as NaN and every row of every live sequence is overwritten; rows past the last sequence and the
p0 entries past a ragged sequence's length keep their fill; the scale gradients are added to what the vectors held.  Outputs sit in guarded allocations."""
import ctypes as C

import pytest
import torch

import parity_util as PU
from util import O, max_abs, rel_err

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2
ERR_ARG = 1
WIDTHS = (8, 16, 32, 64, 96, 128)
EXTRA_ROWS = 3   # rows of dk / dv past the last sequence: never written


@pytest.fixture(scope='module')
def lib():
  import spa3d
  return spa3d._lib.load()


def _s():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(dtype):
  return {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}[dtype]


def _oracle(q0, k, v, sq, sk, km, H, Dh, d_o):
  """fp64 oracle of n equally long sequences: o [n, E], p [n, H, S] (the softmax the oracle's attention applies) and the gradients of sum(o d_o) into q0, k, v;
  the scale gradients accumulate in sq.grad / sk.grad (leaves shared between calls)."""
  n, S, _ = k.shape
  qr, kr, vr = (t.double().clone().requires_grad_(True) for t in (q0, k, v))
  qh = O.rms_norm(qr.view(n, 1, H, Dh), sq)
  kh = O.rms_norm(kr.view(n, S, H, Dh), sk)
  mask = None if km is None else km[:, None, None, :].expand(n, H, 1, S)
  o = O.dot_product_attention(qh, kh, vr.view(n, S, H, Dh), mask).reshape(n, H * Dh)
  o.backward(d_o.double())
  with torch.no_grad():
    lg = torch.einsum('nqhd,nkhd->nhqk', qh / Dh ** 0.5, kh)
    if mask is not None:
      lg = torch.where(mask != 0, lg, torch.full_like(lg, torch.finfo(torch.float64).min))
    p = torch.softmax(lg, -1)[:, :, 0, :]
  return o.detach(), p, qr.grad, kr.grad, vr.grad


def _vec_layout(dt, Dh, lds, ptrs):
  """the lane layout k_attn_q1_* picks (csrc/attn_q1.hip): for the record only, nothing is asserted on it"""
  nv = 16 // torch.empty(0, dtype=dt).element_size()
  return Dh % (4 * nv) == 0 and all(l % nv == 0 for l in lds) and all(p % 16 == 0 for p in ptrs)


def _run(lib, dtype, Dh, S, nseq, H, layout, masked, lens=None, seed=0, dark=False):
  """one forward + backward against the oracle.  layout: 'packed' = k | v in one [rows, 2 E] tensor, as the model passes it; 'separate' = two [rows, E]
  tensors; 'odd' = two tensors of row stride E + 1, which no vector width divides: the scalar lane layout at any head width.  lens: ragged sequence lengths
  (seq_off is passed and p0 is strided by S = max length); None = nseq dense sequences of S keys.  dark: the last sequence has NO visible key, key 0 included
  (where(mask, logit, finfo.min): it attends uniformly and passes no gradient through its logits)."""
  dt, E = _dt(dtype), H * Dh
  ragged = lens is not None
  lens = list(lens) if ragged else [S] * nseq
  assert len(lens) == nseq and max(lens) == S and min(lens) >= 1
  off = [0]
  for l in lens:
    off.append(off[-1] + l)
  total = off[-1]
  g = torch.Generator().manual_seed(1000 * Dh + S + seed)
  q0 = torch.randn(nseq, E, generator=g).to(dt)
  k = torch.randn(total, E, generator=g).to(dt)
  v = torch.randn(total, E, generator=g).to(dt)
  d_o = torch.randn(nseq, E, generator=g).to(dt)
  sq = 1 + 0.2 * torch.randn(Dh, generator=g)
  sk = 1 + 0.2 * torch.randn(Dh, generator=g)
  fill_q, fill_k = torch.randn(Dh, generator=g), torch.randn(Dh, generator=g)   # what dscale_q / dscale_k hold before the call
  km = None
  if masked:
    km = (torch.rand(total, generator=g) < 0.8).float()
    km[off[:-1]] = 1.0                                     # key 0 of every sequence is always visible
    lone = max(range(nseq), key=lambda i: (lens[i] > 1, -i))   # the first sequence with more than one key: only its key 0 stays visible
    km[off[lone] + 1:off[lone + 1]] = 0.0
    if dark:
      km[off[-2]:] = 0.0
  # ---- device tensors
  if layout == 'packed':
    kvd = torch.cat([k, v], 1).cuda()
    kd, vd, ld = kvd[:, :E], kvd[:, E:], 2 * E
    dkv = PU.guarded(total + EXTRA_ROWS, 2 * E, dt, name='dkv')
    dk, dv = dkv[:, :E], dkv[:, E:]
  else:
    ld = E if layout == 'separate' else E + 1
    kb, vb = torch.zeros(total, ld, dtype=dt, device='cuda'), torch.zeros(total, ld, dtype=dt, device='cuda')
    kd, vd = kb[:, :E], vb[:, :E]
    kd.copy_(k); vd.copy_(v)
    dk = PU.guarded(total + EXTRA_ROWS, E, dt, ld=ld, name='dk')
    dv = PU.guarded(total + EXTRA_ROWS, E, dt, ld=ld, name='dv')
  q0d, dod, sqd, skd = q0.cuda(), d_o.cuda(), sq.cuda(), sk.cuda()
  kmd = km.cuda() if masked else None
  offd = torch.tensor(off, dtype=torch.int32, device='cuda') if ragged else None
  o0 = PU.guarded(nseq, E, dt, name='o0')
  p0 = PU.guarded(nseq * H, S, torch.float32, name='p0')
  vec_f = _vec_layout(dt, Dh, (ld, ld, E), (kd.data_ptr(), vd.data_ptr(), q0d.data_ptr(), o0.data_ptr()))
  rc = lib.spa3d_op_attention_q1(q0d.data_ptr(), E, kd.data_ptr(), vd.data_ptr(), ld, ld, sqd.data_ptr(), skd.data_ptr(), kmd.data_ptr() if masked else None,
                                 offd.data_ptr() if ragged else None, nseq, S, H, Dh, o0.data_ptr(), p0.data_ptr(), dtype, _s())
  assert rc == 0
  PU.check_guards()
  dq0 = PU.guarded(nseq, E, dt, name='dq0')
  dsq = PU.guarded(1, Dh, torch.float32, name='dsq', fill=0.0)[0]
  dsk = PU.guarded(1, Dh, torch.float32, name='dsk', fill=0.0)[0]
  dsq.copy_(fill_q); dsk.copy_(fill_k)
  vec_b = vec_f and all(t.data_ptr() % 16 == 0 for t in (dk, dv, dod, dq0))
  rc = lib.spa3d_op_attention_q1_bwd(q0d.data_ptr(), E, kd.data_ptr(), vd.data_ptr(), ld, ld, sqd.data_ptr(), skd.data_ptr(), kmd.data_ptr() if masked else None,
                                     offd.data_ptr() if ragged else None, nseq, S, H, Dh, p0.data_ptr(), dod.data_ptr(), dq0.data_ptr(), dk.data_ptr(),
                                     dv.data_ptr(), dsq.data_ptr(), dsk.data_ptr(), dtype, _s())
  assert rc == 0
  PU.check_guards()
  print(f'  q1 instantiation: Dh {Dh} {dt} layout {layout}: forward {"vec" if vec_f else "scalar"}, backward {"vec" if vec_b else "scalar"}; S {S} nseq {nseq} H {H}'
        f'{" ragged " + str(lens) if ragged else ""}{" masked" if masked else ""}')
  # ---- references: sequences of one length together (fp64 oracle and the float32 restatement on the same stored inputs)
  sqr, skr = sq.double().requires_grad_(True), sk.double().requires_grad_(True)
  r64 = dict(o=torch.zeros(nseq, E, dtype=torch.float64), dq=torch.zeros(nseq, E, dtype=torch.float64), dk=torch.zeros(total, E, dtype=torch.float64),
             dv=torch.zeros(total, E, dtype=torch.float64), p=torch.zeros(nseq * H, S, dtype=torch.float64))
  r32 = {n: torch.zeros_like(t, dtype=torch.float32) for n, t in r64.items() if n != 'p'}
  c32q, c32k = torch.zeros(nseq * H, Dh), torch.zeros(nseq * H, Dh)
  offt = torch.tensor(off)
  for L in sorted(set(lens)):
    seqs = torch.tensor([i for i in range(nseq) if lens[i] == L])
    rows = (offt[seqs][:, None] + torch.arange(L)[None, :])                   # [n, L] rows of k / v
    kk, vv = k[rows], v[rows]
    kmm = km[rows] if masked else None
    probs = (seqs[:, None] * H + torch.arange(H)[None, :]).reshape(-1)        # problem = sequence x H + head
    o_, p_, dq_, dk_, dv_ = _oracle(q0[seqs], kk, vv, sqr, skr, kmm, H, Dh, d_o[seqs])
    r64['o'][seqs], r64['dq'][seqs], r64['dk'][rows], r64['dv'][rows] = o_, dq_, dk_, dv_
    r64['p'][probs, :L] = p_.reshape(-1, L)
    a = PU.attn_q1_restated(q0[seqs], kk, vv, sq, sk, kmm, H, Dh, d_o[seqs], torch.float32)
    r32['o'][seqs], r32['dq'][seqs], r32['dk'][rows], r32['dv'][rows] = a[0], a[2], a[3], a[4]
    c32q[probs], c32k[probs] = a[5], a[6]
  dsq64, dsk64 = fill_q.double() + sqr.grad, fill_k.double() + skr.grad
  e_sq = e_sk = 0.0   # the restatement's worst error: the problems' contributions added to the fill one after the other in float32, in each of the arrival orders
  for order in PU.arrival_orders(nseq * H, Dh):
    e_sq = max(e_sq, float((PU.sequential_sum(fill_q, c32q[order], torch.float32).double() - dsq64).abs().max()))
    e_sk = max(e_sk, float((PU.sequential_sum(fill_k, c32k[order], torch.float32).double() - dsk64).abs().max()))
  live = torch.zeros(nseq * H, S, dtype=torch.bool)
  for i, l in enumerate(lens):
    live[i * H:(i + 1) * H, :l] = True
  # ---- exact facts
  p0c, dkc, dvc = p0.cpu(), dk.float().cpu(), dv.float().cpu()
  assert not torch.isnan(p0c[live]).any(), 'a live p0 entry was not written'
  assert torch.isnan(p0c[~live]).all(), 'p0 past the length of a ragged sequence was written'
  assert not torch.isnan(dkc[:total]).any() and not torch.isnan(dvc[:total]).any(), 'a dk / dv row of a live sequence was not overwritten'
  assert torch.isnan(dkc[total:]).all() and torch.isnan(dvc[total:]).all(), 'rows past the last sequence were written'
  if masked:
    gone = km == 0
    zero_p = gone.clone()                 # keys whose probability is exactly 0: the masked keys of a sequence that has a visible one
    if dark:
      zero_p[off[-2]:] = False
      assert bool((dq0[-1].float().cpu() == 0).all()), 'a sequence without a visible key passes no gradient to its query'
    pm = torch.zeros(nseq * H, S, dtype=torch.bool)
    for i, l in enumerate(lens):
      pm[i * H:(i + 1) * H, :l] = zero_p[off[i]:off[i + 1]][None, :]
    assert bool((p0c[pm] == 0).all()) and bool((dvc[:total][zero_p] == 0).all()), 'p0 / dv of a masked key must be exactly 0'
    assert bool((dkc[:total][gone] == 0).all()), 'dk of a masked key must be exactly 0'
  # ---- gates
  e_p = max_abs(torch.where(live, p0c, torch.zeros(())), r64['p'])
  print(f'  GATE {dt} p0 max-abs {e_p:.3e} bound 1e-05')
  assert e_p < 1e-5
  got = dict(o=o0, dq=dq0, dk=dk[:total], dv=dv[:total])
  if dtype == F32:
    e_o = max_abs(o0, r64['o'])
    print(f'  GATE {dt} o max-abs {e_o:.3e} bound 1e-05')
    assert e_o < 1e-5
    for n, a, b in (('dq', dq0, r64['dq']), ('dk', dk[:total], r64['dk']), ('dv', dv[:total], r64['dv']), ('dsq', dsq, dsq64), ('dsk', dsk, dsk64)):
      e = rel_err(a.float(), b)
      print(f'  GATE {dt} {n} rel {e:.3e} bound 1e-04')
      assert e < 1e-4, n
  else:
    for n in ('o', 'dq', 'dk', 'dv'):
      PU.assert_elementwise(got[n], r64[n], PU.restated_bound(r64[n], r32[n], dt), f'GATE {dt} {n}')
  PU.assert_elementwise(dsq, dsq64, 4.0 * e_sq, f'GATE {dt} dsq')
  PU.assert_elementwise(dsk, dsk64, 4.0 * e_sk, f'GATE {dt} dsk')


DTYPES = [F32, BF16, F16]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Dh', WIDTHS)
def test_q1_every_width_s17_packed(lib, dtype, Dh):
  """S = 17: one key into the second 16-key pass.  nseq x H = 3 x 3 = 9 problems: the last workgroup has three idle waves, which still take the backward's
  barriers.  k | v packed as the model passes them, key mask."""
  _run(lib, dtype, Dh, 17, 3, 3, 'packed', True)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Dh', WIDTHS)
def test_q1_every_width_s151_separate(lib, dtype, Dh):
  """S = 151 (the model's 150 frames + readout token), k and v in tensors of their own; 3 x 1 = 3 problems: fewer than one workgroup's four waves.
  The mask alternates with the width."""
  _run(lib, dtype, Dh, 151, 3, 1, 'separate', Dh in (8, 32, 96))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Dh', [96, 32])
@pytest.mark.parametrize('S', [1, 15, 16, 320])
def test_q1_pass_boundaries(lib, dtype, Dh, S):
  """the other lengths around the 16-key pass and the 320-key limit, at the model's width and at a second one; 5 x 2 = 10 problems"""
  _run(lib, dtype, Dh, S, 5, 2, 'packed', True)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Dh', [16, 32, 64, 96, 128])
def test_q1_scalar_layout_at_vec_widths(lib, dtype, Dh):
  """row stride E + 1: the scalar lane layout at every width that can also run the vec one (16: fp32 only), against the reference, not against the vec result
  (the two sum in different orders).  S = 33: two full passes and one key."""
  _run(lib, dtype, Dh, 33, 2, 2, 'odd', True)


@pytest.mark.parametrize('dtype', DTYPES)
def test_q1_past_the_grid_caps(lib, dtype):
  """10925 x 3 = 32775 problems at S = 17, Dh = 8: more than 4 x 8192 (forward) and 4 x 4096 (backward), so workgroups stride to a second problem, and not a
  multiple of 4"""
  _run(lib, dtype, 8, 17, 10925, 3, 'packed', True)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Dh,layout,masked', [(96, 'packed', True), (32, 'packed', False), (8, 'separate', True), (64, 'odd', True)])
def test_q1_ragged(lib, dtype, Dh, layout, masked):
  """seq_off with lengths 1, 16, 17 and Smax = 40 packed compactly; p0 strided by Smax"""
  _run(lib, dtype, Dh, 40, 4, 2, layout, masked, lens=(1, 16, 17, 40))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Dh,layout', [(32, 'packed'), (8, 'separate')])
def test_q1_sequence_without_a_visible_key(lib, dtype, Dh, layout):
  """The model never masks key 0, and with a visible key the probability of a masked key is exactly 0, so its logit gets no gradient whether or not the
  backward looks at the mask.  The one input on which the backward's own mask test decides anything is a sequence with no visible key: every logit is
  finfo.min, the softmax is uniform over ALL keys, and where() passes no gradient to q or k (tests/test_gpu_ops.py::test_attention_fully_masked_sequence
  pins the same rule for the full-attention kernels).  S = 17, the last of 3 sequences dark."""
  _run(lib, dtype, Dh, 17, 3, 2, layout, True, dark=True)


def test_q1_refusals(lib):
  """every shape the launchers would record as a HIP-class error, and every missing pointer, is SPA3D_ERR_ARG with nothing launched: the outputs keep their fill"""
  H, Dh, S, nseq = 2, 32, 20, 3
  E = H * Dh
  dt = torch.bfloat16
  z = lambda *s: torch.ones(*s, dtype=dt, device='cuda')
  q0, k, v, d_o = z(nseq, E), z(nseq * 320, E), z(nseq * 320, E), z(nseq, E)
  sq, sk = torch.ones(128, device='cuda'), torch.ones(128, device='cuda')
  o0 = PU.guarded(nseq, 128 * H, dt, name='o0')
  p0 = PU.guarded(nseq * H, 321, torch.float32, name='p0')
  dq0 = PU.guarded(nseq, 128 * H, dt, name='dq0')
  dk = PU.guarded(nseq * 320, 128 * H, dt, name='dk')
  dv = PU.guarded(nseq * 320, 128 * H, dt, name='dv')
  dsq = PU.guarded(1, 128, torch.float32, name='dsq')[0]
  dsk = PU.guarded(1, 128, torch.float32, name='dsk')[0]
  pin = torch.zeros(nseq * H, 321, device='cuda')

  def fwd(S=S, Dh=Dh, H=H, nseq=nseq, dtype=BF16, **null):
    a = dict(q0=q0.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), sq=sq.data_ptr(), sk=sk.data_ptr(), o0=o0.data_ptr(), p0=p0.data_ptr())
    a.update(null)
    return lib.spa3d_op_attention_q1(a['q0'], E, a['k'], a['v'], E, E, a['sq'], a['sk'], None, None, nseq, S, H, Dh, a['o0'], a['p0'], dtype, _s())

  def bwd(S=S, Dh=Dh, H=H, nseq=nseq, dtype=BF16, **null):
    a = dict(q0=q0.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), sq=sq.data_ptr(), sk=sk.data_ptr(), p0=pin.data_ptr(), d_o=d_o.data_ptr(), dq0=dq0.data_ptr(),
             dk=dk.data_ptr(), dv=dv.data_ptr(), dsq=dsq.data_ptr(), dsk=dsk.data_ptr())
    a.update(null)
    return lib.spa3d_op_attention_q1_bwd(a['q0'], E, a['k'], a['v'], E, E, a['sq'], a['sk'], None, None, nseq, S, H, Dh, a['p0'], a['d_o'], a['dq0'], a['dk'],
                                         a['dv'], a['dsq'], a['dsk'], dtype, _s())

  for dtype in (F32, BF16, F16):
    for f in (fwd, bwd):
      assert f(S=321, dtype=dtype) == ERR_ARG and f(S=0, dtype=dtype) == ERR_ARG
      for w in (0, 4, 12, 24, 40, 48, 100, 132, 256):
        assert f(Dh=w, dtype=dtype) == ERR_ARG, w
      assert f(H=0, dtype=dtype) == ERR_ARG and f(nseq=-1, dtype=dtype) == ERR_ARG
  for name in ('q0', 'k', 'v', 'sq', 'sk', 'o0', 'p0'):
    assert fwd(**{name: None}) == ERR_ARG, name
  for name in ('q0', 'k', 'v', 'sq', 'sk', 'p0', 'd_o', 'dq0', 'dk', 'dv', 'dsq', 'dsk'):
    assert bwd(**{name: None}) == ERR_ARG, name
  torch.cuda.synchronize()
  for t in (o0, p0, dq0, dk, dv, dsq, dsk):
    assert torch.isnan(t.float()).all(), 'a refused call wrote to an output'
  PU.check_guards()
