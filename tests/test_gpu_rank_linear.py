"""GPU parity of the rank-K projection kernels (rank_fwd_kernel / rank_bwd_kernel in csrc/embed.hip: the depth projection for depth_feature_dim <= 4) on
their own, through spa3d_op_rank_linear / spa3d_op_rank_linear_bwd: every K in 1..4 in bf16 and fp16, output widths whose column groups divide the 256
threads (8, 2048), leave threads idle (48, 384, 392: 240 or 245 of 256 at work; 1032: 129) or fill the workgroup with one row (2048), row counts around the 4-row
unroll and around the backward's rows per workgroup, and row maps other than the model's (T, 1).

Reference: fp64 matmul on the stored inputs with the row map crow(m) = m + (m / rgroup + 1) rskip applied on the host.
Forward: out is pre-filled with random values; mapped rows equal fill + x . w + bias within u_out |ref| + 4 x max |fp32 host restatement - fp64|
(parity_util.restated_bound), skipped rows are bit-identical to the fill and the columns past N are guard bytes.
Backward: gw and gb are pre-filled; the result is the fill plus the gradient, element-wise within 4 x the float32 restatement's own worst error against fp64,
as the LayerNorm dscale.  The restatement adds the rows to the fill one after the other in float32 (parity_util.sequential_sum): the kernel's sums are
per-thread chains, LDS float atomics and one global float atomic per workgroup, i.e. fp32 additions in an order that is not fixed -- so the restatement is
taken in several row orders where the result is narrow (parity_util.arrival_orders) and its worst error is the worst over all of them.
fp32: the kernels' float instantiation moved 8 columns per thread with 4-column (16-byte) loads and stores, so it never updated every other group of four
columns (profiles/r14_q1_rank_gates.log); no model path called it.  It is no longer instantiated and the op refuses SPA3D_F32."""
import ctypes as C

import pytest
import torch

import parity_util as PU

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2
ERR_ARG = 1
ROW_MAPS = [(0, 0), (7, 1), (150, 1), (7, 3)]
WIDTHS = [8, 48, 384, 392, 1032, 2048]


@pytest.fixture(scope='module')
def lib():
  import spa3d
  return spa3d._lib.load()


def _s():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(dtype):
  return {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}[dtype]


def _crow(M, rgroup, rskip):
  m = torch.arange(M)
  return m + (m // rgroup + 1) * rskip if rgroup > 0 else m


def _bits(t):
  return t.contiguous().view(torch.int16)


def _fwd_case(lib, dtype, K, N, M, rgroup, rskip, ldo, bias=True):
  dt = _dt(dtype)
  g = torch.Generator().manual_seed(K * 100003 + N * 17 + M)
  x = torch.randn(M, K, generator=g).to(dt)
  w = torch.randn(K, N, generator=g).to(dt)
  b = torch.randn(N, generator=g) if bias else None
  crow = _crow(M, rgroup, rskip)
  R = int(crow[-1]) + 1 + 2                       # two more rows after the last mapped one
  fill = torch.randn(R, N, generator=g).to(dt)
  out = PU.guarded(R, N, dt, ld=ldo, name='out')
  out.copy_(fill)
  xd, wd = x.cuda(), w.cuda()
  bd = b.cuda() if bias else None
  rc = lib.spa3d_op_rank_linear(xd.data_ptr(), wd.data_ptr(), bd.data_ptr() if bias else None, out.data_ptr(), M, N, K, ldo, rgroup, rskip, dtype, _s())
  assert rc == 0
  PU.check_guards()                               # the columns past N of every row among them
  got = out.cpu()
  add64 = x.double() @ w.double() + (b.double() if bias else 0.0)
  ref64 = fill.double()[crow] + add64
  add32 = x.float() @ w.float()
  ref32 = fill.float()[crow] + ((add32 + b) if bias else add32)
  PU.assert_elementwise(got[crow], ref64, PU.restated_bound(ref64, ref32, dt), f'GATE {dt} out K {K} N {N} M {M} map ({rgroup}, {rskip})')
  skipped = torch.ones(R, dtype=torch.bool)
  skipped[crow] = False
  assert torch.equal(_bits(got[skipped]), _bits(fill[skipped])), 'a row outside the row map changed'


@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('K', [1, 2, 3, 4])
@pytest.mark.parametrize('N', WIDTHS)
def test_rank_linear_forward(lib, dtype, K, N):
  """M = 1, 19, 257, 5000 (fewer rows than one pass of a workgroup, an odd count, one past 256, many workgroups); the four row maps rotate over M, K and N so
  that every width and every K meets every map; M = 19 has ldo = N + 8; M = 257 runs without a bias"""
  for i, M in enumerate((1, 19, 257, 5000)):
    rgroup, rskip = ROW_MAPS[(i + K + WIDTHS.index(N)) % 4]
    _fwd_case(lib, dtype, K, N, M, rgroup, rskip, N + 8 if M == 19 else N, bias=M != 257)
  print(f'  rank instantiation: forward K {K} N {N} {_dt(dtype)}')


def _bwd_case(lib, dtype, K, N, M, rgroup, rskip, ldy):
  dt = _dt(dtype)
  g = torch.Generator().manual_seed(K * 100003 + N * 17 + M + 1)
  x = torch.randn(M, K, generator=g).to(dt)
  crow = _crow(M, rgroup, rskip)
  R = int(crow[-1]) + 1
  dy = torch.randn(R, ldy, generator=g).to(dt)    # the rows outside the map and the columns past N hold values too: reading them shows
  fw, fb = torch.randn(K, N, generator=g), torch.randn(N, generator=g)
  xd, dyd = x.cuda(), dy.cuda()
  d = dy[crow][:, :N]
  gw64 = fw.double() + x.double().t() @ d.double()
  gb64 = fb.double() + d.double().sum(0)
  e_w = e_b = 0.0   # the restatement's worst error: rows added to the fill one after the other in float32, in each of parity_util.arrival_orders
  for order in PU.arrival_orders(M, N):
    s32 = torch.cat([fw.reshape(-1), fb])
    for r0 in range(0, M, 4096):   # row m's addends to gw (K N) and gb (N), 4096 rows at a time to bound the host memory
      xs, ds = x[order[r0:r0 + 4096]].float(), d[order[r0:r0 + 4096]].float()
      s32 = PU.sequential_sum(s32, torch.cat([(xs[:, :, None] * ds[:, None, :]).reshape(-1, K * N), ds], 1), torch.float32)
    e_w = max(e_w, float((s32[:K * N].reshape(K, N).double() - gw64).abs().max()))
    e_b = max(e_b, float((s32[K * N:].double() - gb64).abs().max()))
  for with_gb in (True, False):
    gw = PU.guarded(K, N, torch.float32, name='gw', fill=0.0)
    gb = PU.guarded(1, N, torch.float32, name='gb', fill=0.0)[0]
    gw.copy_(fw); gb.copy_(fb)
    rc = lib.spa3d_op_rank_linear_bwd(xd.data_ptr(), dyd.data_ptr(), M, N, K, ldy, rgroup, rskip, gw.data_ptr(), gb.data_ptr() if with_gb else None, dtype, _s())
    assert rc == 0
    PU.check_guards()
    tag = f'K {K} N {N} M {M} map ({rgroup}, {rskip}){"" if with_gb else " gb = NULL"}'
    PU.assert_elementwise(gw, gw64, 4.0 * e_w, f'GATE {dt} gw {tag}')
    if with_gb:
      PU.assert_elementwise(gb, gb64, 4.0 * e_b, f'GATE {dt} gb {tag}')
    else:
      assert torch.equal(gb.cpu(), fb), 'gb was written although NULL was passed'


@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('K', [1, 2, 3, 4])
@pytest.mark.parametrize('N', WIDTHS)
def test_rank_linear_backward(lib, dtype, K, N):
  """M as in the forward plus 255, 256, 257 around the 256 rows a workgroup takes at least; row maps and the wider row stride (M = 19) as in the forward"""
  for i, M in enumerate((1, 19, 255, 256, 257, 5000)):
    rgroup, rskip = ROW_MAPS[(i + K + WIDTHS.index(N)) % 4]
    _bwd_case(lib, dtype, K, N, M, rgroup, rskip, N + 8 if M == 19 else N)
  print(f'  rank instantiation: backward K {K} N {N} {_dt(dtype)}')


@pytest.mark.parametrize('dtype,K', [(BF16, 2), (F16, 3)])
def test_rank_linear_backward_rows_per_block_above_its_floor(lib, dtype, K):
  """M = 1024 x 256 + 300 at N = 48: a workgroup takes ceil(M / 1024) = 257 rows, more than the floor of 256; the model's row map (150, 1)"""
  _bwd_case(lib, dtype, K, 48, 1024 * 256 + 300, 150, 1, 48)


def test_rank_linear_refusals(lib):
  """K outside 1..4, N % 8 != 0, N > 2048, ld % 8 != 0, a misaligned out / dy, a missing pointer and the float dtype: SPA3D_ERR_ARG, nothing launched"""
  M, N, K = 40, 48, 2
  for dtype in (BF16, F16):
    dt = _dt(dtype)
    x = torch.ones(M, 4, dtype=dt, device='cuda')
    w = torch.ones(4, 4096, dtype=dt, device='cuda')
    b = torch.ones(4096, device='cuda')
    dy = torch.ones(M + 1, 4096, dtype=dt, device='cuda')
    out = PU.guarded(M + 1, 4096, dt, name='out')
    gw = PU.guarded(4, 4096, torch.float32, name='gw')
    gb = PU.guarded(1, 4096, torch.float32, name='gb')[0]
    es = out.element_size()

    def fwd(N=N, K=K, ldo=None, dtype=dtype, M=M, **a):
      p = dict(x=x.data_ptr(), w=w.data_ptr(), out=out.data_ptr())
      p.update(a)
      return lib.spa3d_op_rank_linear(p['x'], p['w'], b.data_ptr(), p['out'], M, N, K, N if ldo is None else ldo, 0, 0, dtype, _s())

    def bwd(N=N, K=K, ldo=None, dtype=dtype, M=M, **a):
      p = dict(x=x.data_ptr(), out=dy.data_ptr(), gw=gw.data_ptr())
      p.update(a)
      return lib.spa3d_op_rank_linear_bwd(p['x'], p['out'], M, N, K, N if ldo is None else ldo, 0, 0, p['gw'], gb.data_ptr(), dtype, _s())

    for f, buf in ((fwd, out), (bwd, dy)):
      assert f(K=0) == ERR_ARG and f(K=5) == ERR_ARG
      assert f(N=44) == ERR_ARG and f(N=2056) == ERR_ARG and f(N=4096) == ERR_ARG and f(N=0) == ERR_ARG
      assert f(ldo=52) == ERR_ARG and f(ldo=60) == ERR_ARG
      assert f(out=buf.data_ptr() + es) == ERR_ARG and f(out=buf.data_ptr() + 8) == ERR_ARG   # one element, and half a 16-byte group
      assert f(dtype=F32) == ERR_ARG
      assert f(x=None) == ERR_ARG and f(out=None) == ERR_ARG
    assert fwd(w=None) == ERR_ARG and bwd(gw=None) == ERR_ARG
    torch.cuda.synchronize()
    for t in (out, gw, gb):
      assert torch.isnan(t.float()).all(), 'a refused call wrote to an output'
    PU.check_guards()
