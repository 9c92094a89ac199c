"""Exact-integer lane of every GEMM kernel: operands whose every partial sum is a small integer (tests/parity_util.py: int_lane_nt, int_lane_tn), so
the right output does not depend on tiling, summation order or atomics and is compared with torch.equal.  A dropped, doubled or permuted k-slice,
row or column changes some integer: the sparse +-1 operand touches every k in every aligned group of 64 columns, with a column-dependent offset.
The reference is a signed gather / index_add_ on the host, not a matmul.

Shapes: the lists of tests/test_gpu_ops.py, test_gpu_fp16.py and test_gpu_gemm_rs.py (chosen for path coverage) without their GELU cases, plus per
kernel the small ones those lists lack: M = 1, M = one tile, one tile + 1, and K of 1, 2 and 3 K-tiles -- where the kernel takes them:
  * the tiled NT kernels need M N >= 128 x 128 (csrc/gemm_plan.hpp plan_nt_tiled), so their M = 1 case is 1 x 16384, and 1 x 16512 = 43 x 384 (384 | N, 256 does not divide N) for the 128 x 384 tile;
  * the persistent 8-phase kernels need 8 | M and K >= 128: M = 8 is their smallest row count and K = 128, 192, 256 their 2, 3, 4 K-tiles;
  * the large-register-tile NT kernel needs 32 | K >= 64: K = 64, 96, 128 are 2, 3, 4 of its 32-wide phases;
  * the row-stationary kernel has K = 384 only;
  * every tiled dW kernel needs a reduction of >= 256 rows (plan_tn): M = 1 runs on the generic kernel only, and 256, 257 are the smallest there.
Both 16-bit types run in every case.  Outputs sit in guarded allocations and the workspace is poisoned.  spa3d_op_linear_bwd runs with the
context's default gradient mode (float atomics); the entry has no switch for the fixed-point det_grads path, so that path is not reached from here
(tests/test_gpu_det_edges.py covers it in-model)."""
import ctypes as C

import pytest
import torch

import parity_util as PU
import test_gpu_fp16 as TF
import test_gpu_gemm_rs as TR
import test_gpu_ops as TO

pytestmark = pytest.mark.gpu
BF16, F16 = 1, 2
TYPES = ((BF16, torch.bfloat16), (F16, torch.float16))


@pytest.fixture(scope='module')
def lib():
  import spa3d
  return spa3d._lib.load()


def _s():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _no_gelu(cases):
  """(M, N, K, res, bias) of the (M, N, K, act, res, bias) cases without an activation"""
  return [(M, N, K, res, bias) for M, N, K, act, res, bias in cases if act == 0]


def _same(got, ref, what):
  got = got.float().cpu()
  if not torch.equal(got, ref):
    bad = (got != ref).nonzero()
    i = tuple(int(x) for x in bad[0])
    pytest.fail(f'{what}: {bad.shape[0]} of {ref.numel()} elements differ from the exact integers, first at {i}: got {float(got[i])}, want {float(ref[i])}')


def _nt_case(lib, impl, M, N, K, res, bias):
  A, W, b, R, ref = PU.int_lane_nt(M, N, K, seed=M + 3 * N + 7 * K, bias=bias, res=res)
  bd = b.cuda() if bias else None
  for code, dt in TYPES:
    Ad, Wd = A.to(dt).cuda(), W.to(dt).cuda()
    Rd = R.to(dt).cuda() if res else None
    Cd = PU.guarded(M, N, dt, name='C')
    ws = PU.poisoned_ws(PU.linear_ws_bytes(N, K))
    rc = lib.spa3d_op_linear(Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr() if bias else None, Rd.data_ptr() if res else None, Cd.data_ptr(), M, N, K, 0,
                             code, impl, ws.data_ptr(), ws.numel(), _s())
    assert rc == 0, (rc, dt)
    PU.check_guards()
    _same(Cd, ref, f'C {dt}')


def _dx_case(lib, impl, M, N, K):
  """dA[M, K] = dC[M, N] . B[K, N]^T: the contraction is N, and B^T is the sparse +-1 operand"""
  dC, Wt, _, _, ref = PU.int_lane_nt(M, K, N, seed=5 * M + N + 11 * K, bias=False, res=False)   # Wt [N, K]
  B = Wt.t().contiguous()
  for code, dt in TYPES:
    dCd, Bd = dC.to(dt).cuda(), B.to(dt).cuda()
    Ad = torch.zeros(8, K, dtype=dt, device='cuda')   # unused by the dA path
    dA = PU.guarded(M, K, dt, name='dA')
    ws = PU.poisoned_ws(PU.linear_ws_bytes(N, K))
    rc = lib.spa3d_op_linear_bwd(Ad.data_ptr(), Bd.data_ptr(), dCd.data_ptr(), dA.data_ptr(), None, None, M, N, K, code, impl, ws.data_ptr(), ws.numel(), _s())
    assert rc == 0, (rc, dt)
    PU.check_guards()
    _same(dA, ref, f'dA {dt}')


def _tn_case(lib, impl, M, N, K):
  A, dC, rW, rb = PU.int_lane_tn(M, N, K, seed=M + 13 * N + 3 * K)
  for code, dt in TYPES:
    Ad, dCd = A.to(dt).cuda(), dC.to(dt).cuda()
    Bd = torch.zeros(K, N, dtype=dt, device='cuda')   # unused by the dB / dbias paths
    dB = PU.guarded(K, N, torch.float32, name='dB')
    db = PU.guarded(1, N, torch.float32, name='dbias')
    ws = PU.poisoned_ws(PU.linear_ws_bytes(N, K))
    rc = lib.spa3d_op_linear_bwd(Ad.data_ptr(), Bd.data_ptr(), dCd.data_ptr(), None, dB.data_ptr(), db.data_ptr(), M, N, K, code, impl, ws.data_ptr(), ws.numel(), _s())
    assert rc == 0, (rc, dt)
    PU.check_guards()
    _same(dB, rW, f'dB {dt}')
    _same(db[0], rb, f'dbias {dt}')


# ------------------------------------------------------------------------------------------------ NT: C = A . W (+ bias)(+ R)
# 128 x 128 x 64 tiles (gemm_nt_occ_kernel up to 8 K-tiles, gemm_nt_kernel beyond): impl 2; gemm_nt_kernel for every K: impl 5
SMALL_128 = [(1, 16384, 64, False, True), (128, 128, 64, False, False), (129, 128, 128, True, True), (128, 128, 192, False, True)]


@pytest.mark.parametrize('M,N,K,res,bias', _no_gelu(TO.TILED_NT) + SMALL_128 + [(129, 128, 640, True, True)])
def test_exact_tiled_nt(lib, M, N, K, res, bias):
  _nt_case(lib, 2, M, N, K, res, bias)


@pytest.mark.parametrize('M,N,K,res,bias', _no_gelu(TO.NT_DOUBLE_BUFFERED) + SMALL_128)
def test_exact_tiled_nt_double_buffered(lib, M, N, K, res, bias):
  _nt_case(lib, 5, M, N, K, res, bias)


# 8-phase kernels, 256 x 256 (256 | N) and 128 x 384 (384 | N), K-tile 64; odd M or K = 64 keeps impl 4 off the persistent 256 x 256 form
@pytest.mark.parametrize('M,N,K,res,bias', _no_gelu(TO.NT_8PHASE) + [(1, 16384, 64, False, True), (256, 256, 64, True, False), (257, 256, 128, False, True),
                                                                    (257, 256, 192, True, True), (1, 16512, 64, False, False), (128, 384, 64, False, True),
                                                                    (129, 384, 128, True, True), (128, 384, 192, False, False)])
def test_exact_tiled_nt_8phase(lib, M, N, K, res, bias):
  _nt_case(lib, 4, M, N, K, res, bias)


@pytest.mark.parametrize('M,N,K,res,bias', _no_gelu(TO.NT_8PHASE_PERSISTENT) + [(8, 2048, 128, False, True), (256, 256, 128, True, True), (264, 256, 192, False, False),
                                                                               (256, 256, 256, False, True), (48, 384, 128, True, False), (128, 384, 128, False, True),
                                                                               (136, 384, 192, True, True), (128, 384, 256, False, False)])
def test_exact_tiled_nt_8phase_persistent(lib, M, N, K, res, bias):
  _nt_case(lib, 3, M, N, K, res, bias)


@pytest.mark.parametrize('M,N,K,bias', TO.NT_LARGE_TILE + [(256, 384, 64, True), (257, 384, 96, False), (256, 384, 128, True), (1, 256, 96, True),
                                                           (384, 256, 64, False), (385, 256, 128, True)])
def test_exact_large_register_tile_nt(lib, M, N, K, bias):
  _nt_case(lib, 10, M, N, K, False, bias)


@pytest.mark.parametrize('M,N,with_bias', [c for c in TR.RS_SHAPES] + [(1, 256, True), (257, 256, False), (512, 384, True)])
def test_exact_row_stationary(lib, M, N, with_bias):
  _nt_case(lib, 7, M, N, 384, False, with_bias)


@pytest.mark.parametrize('M,N,K,res', [(M, N, K, res) for M, N, K, act, res in TO.GENERIC_NT if act == 0] + [(1, 50, 33, True), (1, 8, 64, False), (65, 33, 128, True),
                                                                                                        (64, 64, 192, False), (300, 130, 70, True)])
def test_exact_generic_16bit(lib, M, N, K, res):
  _nt_case(lib, 1, M, N, K, res, True)


@pytest.mark.parametrize('force8p', [False, True])
@pytest.mark.parametrize('M,N,K,res,bias', _no_gelu(TF.FP16_TILED))
def test_exact_fp16_list(lib, force8p, M, N, K, res, bias):
  _nt_case(lib, 3 if force8p else 2, M, N, K, res, bias)


# ------------------------------------------------------------------------------------------------ dX = dC . B^T on the NT kernels
def _dx_impl(impl, M, N, K):
  return impl if (N % 64 == 0 and M * K >= 128 * 128) else 0   # as tests/test_gpu_ops.py::test_linear_bwd_tiled: else the generic kernel


@pytest.mark.parametrize('impl', [2, 3])
@pytest.mark.parametrize('M,N,K', TO.TILED_BWD + [(128, 64, 128), (129, 128, 128), (256, 192, 256), (1, 64, 16384)])
def test_exact_dx_tiled(lib, impl, M, N, K):
  _dx_case(lib, _dx_impl(impl, M, N, K), M, N, K)


@pytest.mark.parametrize('M,N,K', TO.DX_LARGE_TILE + [(1, 64, 384), (256, 96, 384), (257, 128, 384), (384, 64, 256), (385, 96, 256)])
def test_exact_dx_large_register_tile(lib, M, N, K):
  _dx_case(lib, 10, M, N, K)


@pytest.mark.parametrize('M,N,K', TO.GENERIC_BWD + [(1, 33, 50)])
def test_exact_dx_generic_16bit(lib, M, N, K):
  _dx_case(lib, 1, M, N, K)


# ------------------------------------------------------------------------------------------------ dW = A^T . dC, dbias = colsum(dC)
@pytest.mark.parametrize('M,N,K', TO.TILED_BWD + [(256, 128, 128), (257, 128, 128), (320, 129 * 8, 136), (384, 256, 64)])
def test_exact_dw_tiled(lib, M, N, K):
  """gemm_tn_kernel (impl 2 below 65 536 rows): 128 x 128 output tiles, 64 reduction rows per LDS tile, M split across workgroups, float atomics"""
  _tn_case(lib, 2, M, N, K)


@pytest.mark.parametrize('M,N,K', TO.TN_8PHASE + [(256, 256, 256), (257, 256, 256), (272, 384, 128), (320, 128, 384), (1040, 256, 256)])
def test_exact_dw_8phase(lib, M, N, K):
  """the 8-phase dW kernels (impl 3): 256 x 256, 128 x 384 and 384 x 128 tiles, ring of 16-row quarters"""
  _tn_case(lib, 3, M, N, K)


@pytest.mark.parametrize('M,N,K', TO.TN_LARGE_TILE + [(256, 256, 384), (257, 256, 384), (288, 384, 256), (289, 384, 256), (320, 256, 384)])
def test_exact_dw_large_register_tile(lib, M, N, K):
  """gemm_tnb_kernel + gemm_tn_tail_kernel (impl 9): 384 x 256 / 256 x 384 tiles, M % 32 rows through the tail kernel"""
  _tn_case(lib, 9, M, N, K)


@pytest.mark.parametrize('M,N,K', TO.GENERIC_BWD + [(1, 40, 24), (255, 96, 64), (257, 50, 33)])
def test_exact_dw_generic_16bit(lib, M, N, K):
  _tn_case(lib, 1, M, N, K)
