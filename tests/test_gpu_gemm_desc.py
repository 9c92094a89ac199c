"""The GEMM kernels behind their descriptor (csrc/gemm_plan.hpp GemmDesc) through spa3d_op_gemm, one kernel at a time: what spa3d_op_linear(_bwd) cannot
state -- row remaps, gather / scatter maps, column segments, fused column sums, padded strides, f32 / accumulating outputs, alpha, the pre-activation output.
Everything that can be is on the exact-integer lane (tests/parity_util.py desc_nt_case / desc_tn_case): compared with torch.equal, the destination
pre-filled with pattern() and compared whole (rows and columns the kernel must not touch included), NaN wherever the kernel must not read, outputs in
guarded allocations, a poisoned workspace.  Every case names its kernel and asserts the kernel_out the entry reports; tests/test_gemm_desc_host.py checks on
the CPU that the planner gives that kernel for the case and that every expected value is exact in the output type.  impl forces kernels at small M as in
tests/test_gpu_gemm_exact.py: 2 tiled, 5 without the single-buffer NT kernel, 3 the 8-phase kernels at any row count, 9 also the large-tile dW kernel, 1 generic.

Feature -> kernels it runs on here (NT: C = A . W):
  crow remap (+ residual)         NtOcc, Nt, Nt8p256, Nt8p384, Generic.  Never the persistent kernels or NtEmbed: plan_nt_tiled takes crow_group != 0 off both
  crow remap + pre_out (GELU)     NtOcc, Nt8p384
  padded sAm / sCm (+ residual)   NtOcc, Nt, Nt8p256, Nt8p384, Nt8pp256, Nt8pp384, Generic
  out_f32                         NtOcc, Nt, Nt8p256, Nt8p384, Nt8pp256, Generic.  Not Nt8pp384: plan_nt_tiled gives it no f32 output (asserted: Nt8p384 runs)
  accumulate, out_f32 + accumulate  NtOcc, Nt, Nt8p256, Nt8p384, Generic.  Never persistent (asserted at shapes the persistent kernels would take)
  pre_out without a remap         Nt8pp256; at N = 384 the planner leaves Nt8pp384 for Nt8p384 (asserted)
  EPI_MUL_GELU_GRAD               NtOcc, Nt, Nt8p256, Nt8p384 (the gate of tests/test_gpu_gemm_rs.py)
  alpha 0.5, 2                    NtOcc, Generic
  two-level batch                 Generic, 16-bit and fp32 (no tiled kernel is batched: plan_nt_tiled)
  one-pass embedding              NtEmbed (the only kernel with these operands)
dW (C += X^T . dY):
  brow remap, NaN skipped rows    Tn8p256, Tn8p128x384, Tn8p384x128, Tnb (both tile shapes, with its tail kernel), Generic; group 15 lands on Tn (asserted)
  seg_n / C_seg                   Tn8p256, Tn8p128x384, Tn8p384x128, Tnb.  Tn and Generic have no segments: plan_tn refuses, the entry returns SPA3D_ERR_ARG (asserted)
  fused colsum_out                Tn8p256, Tn8p128x384, Tn8p384x128, Tnb with two and three row tiles; on Tn and Generic the entry adds the sums itself (asserted equal)
  padded sAk / sBk / sCm          Tn, Tn8p256, Tn8p128x384, Tn8p384x128, Tnb, Generic
Shapes are the issue's; where the planner sends one elsewhere the nearest it takes is used: the 8-phase dW tile follows (Ki, N) -- 256 x 256 -> Tn8p256,
256 x 384 -> Tn8p128x384, 384 x 256 -> Tn8p384x128 (tn8p_tile) -- and Tnb takes 384 x 256 and 256 x 384 only (tnb_takes)."""
import ctypes as C
import math

import pytest
import torch

import parity_util as PU
from test_gpu_gemm_exact import _same
from test_gpu_gemm_rs import _gelu_grad64

pytestmark = pytest.mark.gpu
BF16, F16, F32 = 1, 2, 0
TYPES = ((BF16, torch.bfloat16), (F16, torch.float16))
ERR_ARG, ERR_WORKSPACE = 1, 2


@pytest.fixture(scope='module')
def lib():
  import spa3d
  return spa3d._lib.load()


def _L():
  import spa3d
  return spa3d._lib


def _s():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(x, dt):
  return None if x is None else x.to(dt).cuda().contiguous()


def _ptr(t):
  return None if t is None else t.data_ptr()


def _args(**kw):
  a = _L().GemmArgs()
  a.nb1 = a.nb2 = 1
  a.alpha = 1.0
  a.aux_is_residual = 1
  for k, v in kw.items():
    setattr(a, k, v)
  return a


def _call(lib, a, code, impl, ws_bytes=64 << 10):
  ws = PU.poisoned_ws(ws_bytes)
  k = C.c_int32(-1)
  rc = lib.spa3d_op_gemm(C.byref(a), code, impl, C.byref(k), ws.data_ptr(), ws.numel(), _s())
  torch.cuda.synchronize()
  return rc, _L().GEMM_KERNELS[k.value]


# ------------------------------------------------------------------------------------------------ case tables (also read by tests/test_gemm_desc_host.py)
def nt(kernel, impl, M, N, K, **kw):
  """one NT case: the kernel it must run on, the impl that sends it there, desc_nt_case's arguments, and out_f32 / pre / epi for the call"""
  c = dict(kind='nt', kernel=kernel, impl=impl, M=M, N=N, K=K, lda=K, ldc=N, crow=(0, 0), res=False, bias=True, alpha=1.0, acc=False, emb=None, out_f32=False, pre=False, epi=0)
  c.update(kw)
  c['id'] = '-'.join([kernel, f'{M}x{N}x{K}'] + [f'{k}={v}'.replace(' ', '') for k, v in sorted(kw.items()) if k != 'emb'] + (['emb'] if c['emb'] else []))
  return c


def tn(kernel, impl, M, Ki, N, **kw):
  """one dW case: reduction length M (the descriptor's K), output Ki x N (the descriptor's M x N)"""
  c = dict(kind='tn', kernel=kernel, impl=impl, M=M, Ki=Ki, N=N, lda=Ki, ldb=N, ldc=None, brow=(0, 0), seg_n=0, colsum=False)
  c.update(kw)
  c['id'] = '-'.join([kernel, f'{M}:{Ki}x{N}'] + [f'{k}={v}'.replace(' ', '') for k, v in sorted(kw.items())])
  return c


def nt_build(c):
  return PU.desc_nt_case(c['M'], c['N'], c['K'], seed=c['M'] + 3 * c['N'] + 7 * c['K'] + c['impl'], lda=c['lda'], ldc=c['ldc'], crow=c['crow'], res=c['res'],
                         bias=c['bias'], alpha=c['alpha'], acc=c['acc'], emb=c['emb'])


def tn_build(c):
  return PU.desc_tn_case(c['M'], c['N'], c['Ki'], seed=c['M'] + 13 * c['N'] + 3 * c['Ki'], lda=c['lda'], ldb=c['ldb'], brow=c['brow'])


def plan_line(c):
  """the case as a line for tests/host/gemm_plan_check.cpp (pointers: any 16-byte aligned addresses; the entry supplies Bt and the zero page)"""
  if c['kind'] == 'nt':
    f = dict(M=c['M'], N=c['N'], K=c['K'], sAm=c['lda'], sCm=c['ldc'], Bt='0x500000', ldBt=c['K'], epi=c['epi'], out_f32=int(c['out_f32']), accumulate=int(c['acc']),
             crow_group=c['crow'][0], alpha=int(c['alpha']) if c['alpha'] >= 1 else 0)
    if c['bias']: f['bias'] = '0x720000'
    if c['res'] or c['epi'] == 2: f['aux'] = '0x900000'
    if c['pre']: f['pre_out'] = '0xd00000'
    e = c['emb']
    if e:
      f.update(arow='0x700000', crow='0x710000')
      if e['K1']: f.update(A2='0x600000', sA2m=e['lda2'], K1=e['K1'])
      if e['r1']: f.update(r1_x='0x730000', r1_w='0x740000')
  else:
    f = dict(M=c['Ki'], N=c['N'], K=c['M'], sAm=1, sAk=c['lda'], sBk=c['ldb'], sBn=1, sCm=c['seg_n'] or c['ldc'] or c['N'], out_f32=1, accumulate=1, zero_page='0xb00000',
             brow_group=c['brow'][0], brow_skip=c['brow'][1], seg_n=c['seg_n'])
    if c['colsum']: f['colsum'] = '0xc00000'
  return f'gemm {c["impl"]} ' + ' '.join(f'{k}={v}' for k, v in f.items())


# ---- NT: crow remap.  M is no multiple of the group (the last group is partial) except group 1; group 1 puts a boundary on every tile edge, 7 and 150 inside tiles
def _crow(kernel, impl, N1, N2):
  return [nt(kernel, impl, 257, N1, 64, crow=(150, 1)), nt(kernel, impl, 300, N2, 192, crow=(7, 3), res=True), nt(kernel, impl, 300, N2, 64, crow=(1, 1), res=True)]


NT_CROW = (_crow('NtOcc', 2, 256, 384) + _crow('Nt', 5, 256, 384) + _crow('Nt8p256', 3, 256, 256) + _crow('Nt8p384', 3, 384, 384) + _crow('Generic', 1, 256, 384))
NT_CROW_PRE = [nt('NtOcc', 2, 300, 384, 192, crow=(7, 3), res=True, pre=True, epi=1), nt('Nt8p384', 3, 257, 384, 64, crow=(150, 1), res=True, pre=True, epi=1)]
# ---- NT: padded strides, the residual at C's stride.  The persistent kernels need 8 | M and K >= 128; an odd M keeps impl 3 off them
NT_STRIDES = [nt('NtOcc', 2, 257, 256, 64, lda=72, ldc=264, res=True), nt('Nt', 5, 257, 384, 192, lda=256, ldc=392, res=True),
              nt('Nt8p256', 3, 257, 256, 128, lda=136, ldc=264), nt('Nt8p384', 3, 129, 384, 192, lda=256, ldc=392, res=True),
              nt('Nt8pp256', 3, 264, 256, 128, lda=192, ldc=264, res=True), nt('Nt8pp256', 3, 264, 256, 192, lda=200, ldc=264),
              nt('Nt8pp384', 3, 136, 384, 192, lda=200, ldc=392, res=True), nt('Nt8pp384', 3, 136, 384, 128, lda=192, ldc=392),
              nt('Generic', 1, 300, 130, 70, lda=78, ldc=138, res=True)]
# ---- NT: f32 output, accumulate, both.  264 x 256 x 128 and 136 x 384 x 128 are shapes impl 3 gives the persistent kernels: with accumulate it must not
_OUT = [dict(out_f32=True), dict(acc=True), dict(out_f32=True, acc=True)]
NT_OUT = ([nt(k, i, M, N, K, **f) for f in _OUT for k, i, M, N, K in (('NtOcc', 2, 257, 256, 64), ('Nt', 5, 129, 384, 128), ('Generic', 1, 65, 40, 72))]
          + [nt('Nt8p256', 3, 264, 256, 128, **f) for f in _OUT[1:]] + [nt('Nt8p384', 3, 136, 384, 128, **f) for f in _OUT]
          + [nt('Nt8pp256', 3, 264, 256, 128, out_f32=True), nt('Nt8p256', 3, 257, 256, 128, out_f32=True)])
# ---- NT: the pre-activation output without a remap: the persistent 256 x 256 kernel takes it (no aux), the persistent 128 x 384 kernel does not
NT_PRE = [nt('Nt8pp256', 3, 264, 256, 128, pre=True, epi=1), nt('Nt8p384', 3, 136, 384, 128, pre=True, epi=1)]
NT_ALPHA = [nt(k, i, M, N, K, alpha=al) for al in (0.5, 2.0) for k, i, M, N, K in (('NtOcc', 2, 257, 256, 64), ('Generic', 1, 65, 40, 72))]
NT_GELU_GRAD = [nt('NtOcc', 2, 257, 256, 128, bias=False, epi=2), nt('Nt', 5, 257, 384, 64, bias=False, epi=2), nt('Nt8p256', 3, 257, 256, 128, bias=False, epi=2),
                nt('Nt8p384', 3, 129, 384, 192, bias=False, epi=2)]
# ---- NT: the one-pass input embedding (N = 384).  Row strides differ from K1 and K - K1
def _emb(M, K, K1, r1, bias):
  return nt('NtEmbed', 2, M, 384, K, lda=(K1 or K) + 8, bias=bias, emb=dict(K1=K1, src_rows=M + 37, lda2=K - K1 + 16, r1=r1))


NT_EMBED = [_emb(128, 256, 64, True, True), _emb(129, 256, 192, True, False), _emb(300, 256, 64, False, True), _emb(300, 64, 0, True, True), _emb(129, 256, 192, False, False)]
NT_EXACT = NT_CROW + NT_STRIDES + NT_OUT + NT_ALPHA + NT_EMBED

# ---- dW.  The 8-phase tile follows (Ki, N); Tnb has two tile shapes
TN_TILED = [('Tn8p256', 3, 256, 256), ('Tn8p128x384', 3, 256, 384), ('Tn8p384x128', 3, 384, 256), ('Tnb', 9, 384, 256), ('Tnb', 9, 256, 384)]
# reduction lengths per (group, skip): one below, at and one above a multiple of the group, all with M % 32 != 0 (the large-tile kernel's tail kernel runs with the
# remap) and one with M % 32 == 0; 8267 = 8192 + 75: the 8-phase kernels take two M-splits of 4160 rows (launch_tn8p), and 4160 is inside a group of 150 and of 151
TN_BROW_M = {(16, 1): (271, 272, 273, 288), (150, 1): (299, 300, 301, 8267), (151, 3): (301, 302, 303, 8267)}
TN_BROW = [tn(k, i, M, Ki, N, brow=b) for k, i, Ki, N in TN_TILED for b, Ms in TN_BROW_M.items() for M in Ms]
TN_BROW += [tn('Tn', 3, M, 256, 256, brow=(15, 1)) for M in (299, 300, 301, 8267)] + [tn('Tn', 9, 300, 384, 256, brow=(15, 1)), tn('Generic', 1, 300, 40, 24, brow=(7, 3))]
TN_SEG = [tn('Tn8p128x384', 3, 300, 384, 768, seg_n=384), tn('Tnb', 9, 300, 384, 768, seg_n=384), tn('Tn8p128x384', 3, 300, 384, 1152, seg_n=384),
          tn('Tnb', 9, 300, 256, 1152, seg_n=384), tn('Tn8p128x384', 3, 300, 384, 384, seg_n=128), tn('Tnb', 9, 300, 256, 384, seg_n=128),
          tn('Tn8p256', 3, 300, 256, 768, seg_n=256), tn('Tnb', 9, 300, 384, 768, seg_n=256), tn('Tn8p384x128', 3, 300, 384, 256, seg_n=128),
          tn('Tn8p128x384', 3, 301, 384, 1152, seg_n=384, brow=(150, 1)), tn('Tnb', 9, 301, 256, 1152, seg_n=384, brow=(16, 1))]
# Ki of two and three row tiles: tiles with ti > 0 exist and must not add the column sums
_CS = [('Tn8p256', 3, 512, 256), ('Tn8p256', 3, 768, 256), ('Tn8p128x384', 3, 256, 384), ('Tn8p128x384', 3, 384, 384), ('Tn8p384x128', 3, 768, 128),
       ('Tn8p384x128', 3, 1152, 128), ('Tnb', 9, 768, 256), ('Tnb', 9, 1152, 256), ('Tnb', 9, 512, 384), ('Tnb', 9, 768, 384), ('Tn', 2, 256, 256), ('Generic', 1, 40, 24)]
TN_COLSUM = [tn(k, i, 300, Ki, N, colsum=True, brow=b) for k, i, Ki, N in _CS for b in ((0, 0), (150, 1))]
TN_STRIDES = [tn(k, i, 300, Ki, N, lda=Ki + 8, ldb=N + 8, ldc=N + 8) for k, i, Ki, N in TN_TILED + [('Tn', 2, 256, 256), ('Generic', 1, 40, 24)]]
TN_ALL = TN_BROW + TN_SEG + TN_COLSUM + TN_STRIDES


def _ids(cases):
  return [pytest.param(c, id=c['id']) for c in cases]


# ------------------------------------------------------------------------------------------------ NT
def _run_nt(lib, c, o, code, dt, aux=None):
  """the call of one NT case in one type -> (C view, pre_out view or None); kernel and guards asserted"""
  out_dt = torch.float32 if c['out_f32'] else dt
  Cd = PU.guarded(o['rows'], c['N'], out_dt, ld=o['ldc'], name='C')
  Cd.copy_(o['C0'].to(out_dt))
  Pd = None
  if c['pre']:
    Pd = PU.guarded(o['rows'], c['N'], dt, ld=o['ldc'], name='pre_out')
    Pd.copy_(PU.pattern(o['rows'], c['N']).to(dt))
  keep = {k: _dev(o[k], dt) for k in ('A', 'A2', 'W', 'R', 'r1_x')}
  keep.update(bias=_dev(o['bias'], torch.float32), r1_w=_dev(o['r1_w'], torch.float32), arow=_dev(o['arow'], torch.int32), cidx=_dev(o['cidx'], torch.int32))
  if aux is not None:
    keep['R'] = aux
  e = c['emb'] or {}
  a = _args(A=_ptr(keep['A']), B=_ptr(keep['W']), C=Cd.data_ptr(), M=c['M'], N=c['N'], K=c['K'], sAm=o['lda'], sAk=1, sBk=c['N'], sBn=1, sCm=o['ldc'],
            alpha=c['alpha'], bias=_ptr(keep['bias']), epi=c['epi'], aux=_ptr(keep['R']), aux_is_residual=int(c['epi'] != 2), out_f32=int(c['out_f32']),
            accumulate=int(c['acc']), pre_out=_ptr(Pd), crow_group=c['crow'][0], crow_skip=c['crow'][1], A2=_ptr(keep['A2']), sA2m=e.get('lda2', 0), K1=e.get('K1', 0),
            arow_idx=_ptr(keep['arow']), crow_idx=_ptr(keep['cidx']), r1_x=_ptr(keep['r1_x']), r1_w=_ptr(keep['r1_w']))
  rc, k = _call(lib, a, code, c['impl'], c['K'] * c['N'] * 2 + (64 << 10))
  print(f'  {c["id"]} {dt}: rc {rc}, kernel {k}')
  assert rc == 0 and k == c['kernel'], (rc, k, c['kernel'])
  PU.check_guards()
  return Cd, Pd


@pytest.mark.parametrize('c', _ids(NT_EXACT))
def test_nt_exact(lib, c):
  """C compared whole with the exact integers: the image of the row map holds the sums, every other row still holds pattern()"""
  o = nt_build(c)
  for code, dt in TYPES:
    Cd, _ = _run_nt(lib, c, o, code, dt)
    _same(Cd, o['C'].float(), f'C {dt}')


@pytest.mark.parametrize('c', _ids(NT_CROW_PRE + NT_PRE))
def test_nt_pre_out(lib, c):
  """EPI_GELU with the pre-activation output: pre_out on the exact lane (whole buffer, remapped like C), C = gelu(pre) + R through the element-wise gate"""
  o = nt_build(c)
  keep = o['cmap'] >= 0
  R = o['R'][o['cmap'], :c['N']] if c['res'] else None
  ref = PU.gelu_tanh(o['pre']) + (R if c['res'] else 0.0)
  for code, dt in TYPES:
    Cd, Pd = _run_nt(lib, c, o, code, dt)
    _same(Pd, o['P'].float(), f'pre_out {dt}')
    got = Cd.float().cpu()
    bound = PU.linear_bound(o['Aeff'].float(), o['W'].float(), o['bias'], R, 1, ref, o['pre'], dt)
    PU.assert_elementwise(got[o['cmap']], ref, bound, f'C {dt}')
    rest = torch.ones(o['rows'], dtype=torch.bool); rest[o['cmap'][keep]] = False
    _same(got[rest], o['C0'][rest].float(), f'rows of C outside the row map {dt}')


@pytest.mark.parametrize('c', _ids(NT_GELU_GRAD))
def test_nt_gelu_grad(lib, c):
  """C = (A . W) o gelu'(aux) on the tiled kernels, operands and gate of tests/test_gpu_gemm_rs.py::test_gemm_rs_gelu_grad_epilogue_matches_fp64"""
  M, N, K = c['M'], c['N'], c['K']
  g = torch.Generator().manual_seed(7 * M + N)
  for code, dt in TYPES:
    A = torch.randn(M, K, generator=g).to(dt)
    B = (torch.randn(K, N, generator=g) / math.sqrt(K)).to(dt)
    pre = (torch.randn(M, N, generator=g) * 1.5).to(dt)
    o = dict(A=A, W=B, A2=None, R=None, r1_x=None, r1_w=None, bias=None, arow=None, cidx=None, rows=M, lda=K, ldc=N, C0=PU.pattern(M, N))
    Cd, _ = _run_nt(lib, c, o, code, dt, aux=pre.cuda())
    gg = _gelu_grad64(pre.double())
    ref = (A.double() @ B.double()) * gg
    gerr = 4.0 * float((_gelu_grad64(pre.float()).double() - gg).abs().max())
    ap = PU.abs_product(A, B)
    PU.assert_elementwise(Cd.cpu(), ref, PU.elementwise_bound(ref, ap * gg.abs(), K, dt) + (1 + PU.unit_roundoff(dt)) * gerr * ap, f'dh {dt}')


BATCH = dict(nb1=2, nb2=3, M=33, N=40, K=24)


def batch_build():
  """two-level batch with six distinct batch strides: flat NaN operand buffers, C a flat pattern(); -> (A, B, expected C, strides, per-batch references)"""
  b = BATCH
  M, N, K, nb1, nb2 = b['M'], b['N'], b['K'], b['nb1'], b['nb2']
  st = dict(bA2=M * K + 8, bB2=K * N + 24, bC2=M * N + 40)
  st.update(bA1=nb2 * st['bA2'] + 16, bB1=nb2 * st['bB2'] + 32, bC1=nb2 * st['bC2'] + 48)
  assert len(set(st.values())) == 6
  A = torch.full((nb1 * st['bA1'],), float('nan'), dtype=torch.float64)
  B = torch.full((nb1 * st['bB1'],), float('nan'), dtype=torch.float64)
  Cx = PU.pattern(1, nb1 * st['bC1'])[0]
  for b1 in range(nb1):
    for b2 in range(nb2):
      o = PU.desc_nt_case(M, N, K, seed=100 + 10 * b1 + b2, bias=False)
      ia, ib, ic = b1 * st['bA1'] + b2 * st['bA2'], b1 * st['bB1'] + b2 * st['bB2'], b1 * st['bC1'] + b2 * st['bC2']
      A[ia:ia + M * K] = o['A'].reshape(-1)
      B[ib:ib + K * N] = o['W'].reshape(-1)
      Cx[ic:ic + M * N] = o['pre'].reshape(-1)
  return A, B, Cx, st


@pytest.mark.parametrize('code,dt', TYPES + ((F32, torch.float32),))
def test_generic_two_level_batch(lib, code, dt):
  b = BATCH
  A, B, Cx, st = batch_build()
  Ad, Bd = _dev(A, dt), _dev(B, dt)
  Cd = PU.guarded(1, Cx.numel(), dt, name='C')
  Cd.copy_(PU.pattern(1, Cx.numel()).to(dt))
  a = _args(A=Ad.data_ptr(), B=Bd.data_ptr(), C=Cd.data_ptr(), M=b['M'], N=b['N'], K=b['K'], sAm=b['K'], sAk=1, sBk=b['N'], sBn=1, sCm=b['N'], nb1=b['nb1'], nb2=b['nb2'], **st)
  rc, k = _call(lib, a, code, 1 if code != F32 else 0)
  print(f'  batch {dt}: rc {rc}, kernel {k}')
  assert rc == 0 and k == 'Generic'
  PU.check_guards()
  _same(Cd[0], Cx.float(), f'C {dt}')


# ------------------------------------------------------------------------------------------------ dW
def _run_tn(lib, c, o, code, dt, expect_rc=0):
  """the call of one dW case in one type -> (segment views, colsum view); C and the column sums start from the case's integers"""
  Ki, N, seg = c['Ki'], c['N'], c['seg_n']
  w = seg or N
  ldc = w if seg else (c['ldc'] or N)
  Cs = []
  for s in range(N // w):
    Cs.append(PU.guarded(Ki, w, torch.float32, ld=ldc, name=f'dW segment {s}'))
    Cs[-1].copy_(o['C0'][:, s * w:(s + 1) * w].float())
  cs = PU.guarded(1, N, torch.float32, name='colsum')
  cs.copy_(o['cs0'].float()[None])
  Xd, Yd = _dev(o['X'], dt), _dev(o['dY'], dt)
  a = _args(A=Xd.data_ptr(), B=Yd.data_ptr(), C=Cs[0].data_ptr(), M=Ki, N=N, K=c['M'], sAm=1, sAk=o['lda'], sBk=o['ldb'], sBn=1, sCm=ldc, out_f32=1, accumulate=1,
            brow_group=c['brow'][0], brow_skip=c['brow'][1], seg_n=seg, colsum_out=cs.data_ptr() if c['colsum'] else None)
  for s, t in enumerate(Cs[1:3]):
    a.C_seg[s] = t.data_ptr()
  rc, k = _call(lib, a, code, c['impl'])
  print(f'  {c["id"]} {dt}: rc {rc}, kernel {k}')
  assert rc == expect_rc and k == (c['kernel'] if expect_rc == 0 else 'Refuse'), (rc, k, c['kernel'])
  PU.check_guards()
  return Cs, cs


@pytest.mark.parametrize('c', _ids(TN_ALL))
def test_dw_exact(lib, c):
  """every segment of dW and the column sums (the initial integers when the case has none: untouched) equal the exact integers"""
  o = tn_build(c)
  w = c['seg_n'] or c['N']
  for code, dt in TYPES:
    Cs, cs = _run_tn(lib, c, o, code, dt)
    for s, t in enumerate(Cs):
      _same(t, o['dW'][:, s * w:(s + 1) * w].float(), f'dW segment {s} {dt}')
    _same(cs[0], (o['cs'] if c['colsum'] else o['cs0']).float(), f'colsum {dt}')


# what plan_tn refuses with segments: a reduction under 256 rows, more than three segments, seg_n % 32, segments with fused column sums, and kernels without segments
SEG_REFUSED = [tn('Refuse', 3, 255, 384, 768, seg_n=384), tn('Refuse', 3, 300, 384, 384, seg_n=96), tn('Refuse', 3, 300, 384, 96, seg_n=48),
               tn('Refuse', 3, 300, 384, 768, seg_n=384, colsum=True), tn('Refuse', 2, 300, 384, 768, seg_n=384), tn('Refuse', 1, 300, 384, 768, seg_n=384),
               tn('Refuse', 0, 300, 384, 768, seg_n=384)]


@pytest.mark.parametrize('c', _ids(SEG_REFUSED))
def test_dw_segments_refused(lib, c):
  o = tn_build(c)
  w = c['seg_n']
  Cs, cs = _run_tn(lib, c, o, BF16, torch.bfloat16, expect_rc=ERR_ARG)
  for s, t in enumerate(Cs):
    _same(t, o['C0'][:, s * w:(s + 1) * w].float(), f'dW segment {s} after a refusal')
  _same(cs[0], o['cs0'].float(), 'colsum after a refusal')


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(lib):
  """refused before any launch: the output still holds its fill"""
  c = nt('Generic', 1, 33, 40, 24)
  o = nt_build(c)
  dt = torch.bfloat16
  Ad, Wd = _dev(o['A'], dt), _dev(o['W'], dt)
  Cd = PU.guarded(o['rows'], 40, dt, name='C')
  Cd.copy_(o['C0'].to(dt))
  f32 = torch.zeros(64, device='cuda')
  i32 = torch.zeros(64, dtype=torch.int32, device='cuda')
  base = dict(A=Ad.data_ptr(), B=Wd.data_ptr(), C=Cd.data_ptr(), M=33, N=40, K=24, sAm=24, sAk=1, sBk=40, sBn=1, sCm=40)
  bad = [dict(A=None), dict(B=None), dict(C=None), dict(M=0), dict(N=0), dict(K=-1), dict(nb1=0), dict(nb2=0), dict(epi=3), dict(epi=2), dict(crow_group=-1),
         dict(brow_skip=-1), dict(seg_n=-8), dict(seg_n=16), dict(seg_n=8, N=40), dict(A2=Ad.data_ptr(), K1=0), dict(A2=Ad.data_ptr(), K1=24), dict(r1_x=Ad.data_ptr())]
  for kw in bad:
    for code in (BF16, F16, F32):
      rc, k = _call(lib, _args(**{**base, **kw}), code, 0)
      assert rc == ERR_ARG and k == 'Refuse', (kw, code, rc, k)
  # fp32 has the generic kernel only: what that kernel does not implement is refused, not dropped
  A32, W32 = _dev(o['A'], torch.float32), _dev(o['W'], torch.float32)
  b32 = dict(base, A=A32.data_ptr(), B=W32.data_ptr())
  for kw in (dict(seg_n=20, C_seg=(C.c_void_p * 2)(f32.data_ptr(), None)), dict(colsum_out=f32.data_ptr()), dict(arow_idx=i32.data_ptr()), dict(crow_idx=i32.data_ptr()),
             dict(A2=A32.data_ptr(), K1=8, sA2m=24), dict(r1_x=A32.data_ptr(), r1_w=f32.data_ptr())):
    rc, k = _call(lib, _args(**{**b32, **kw}), F32, 0)
    assert rc == ERR_ARG and k == 'Refuse', (kw, rc, k)
  # 16-bit: the same operands where the plan is the generic kernel (33 x 40 is below every tiled kernel), and a tiled request nothing takes
  for kw in (dict(arow_idx=i32.data_ptr()), dict(crow_idx=i32.data_ptr()), dict(r1_x=Ad.data_ptr(), r1_w=f32.data_ptr())):
    rc, k = _call(lib, _args(**{**base, **kw}), BF16, 0)
    assert rc == ERR_ARG, (kw, rc, k)
  rc, k = _call(lib, _args(**base), BF16, 2)
  assert rc == ERR_ARG and k == 'Refuse'
  # a workspace too small for the transposed copy of B (a tiled NT plan) or for the zero page (a dW descriptor)
  big = nt('NtOcc', 2, 257, 256, 64)
  ob = nt_build(big)
  Ab, Wb = _dev(ob['A'], dt), _dev(ob['W'], dt)
  Cb = PU.guarded(ob['rows'], 256, dt, name='Cb')
  Cb.copy_(ob['C0'].to(dt))
  a = _args(A=Ab.data_ptr(), B=Wb.data_ptr(), C=Cb.data_ptr(), M=257, N=256, K=64, sAm=64, sAk=1, sBk=256, sBn=1, sCm=256)
  rc, _ = _call(lib, a, BF16, 2, ws_bytes=1024)
  assert rc == ERR_WORKSPACE
  torch.cuda.synchronize()
  PU.check_guards()
  _same(Cd, o['C0'].float(), 'C after the refusals')
  _same(Cb, ob['C0'].float(), 'C after a workspace refusal')
