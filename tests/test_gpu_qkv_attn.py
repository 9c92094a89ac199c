"""Fused QKV projection + attention forward (csrc/qkv_attn.hip; /root/reference/attention.py:154-175 = three DenseGeneral, two RMSNorm, dot_product_attention as ONE
kernel per (sequence, head)) against (a) the fp64 oracle and (b) the two-kernel path it replaces (projection GEMM + fused attention kernel), which has the same
rounding points: q | k | v rounded to 16 bits, normalised from the rounded values, P rounded before P.V."""
import ctypes as C
import math

import pytest
import torch

from util import O, max_abs, rel_err

pytestmark = pytest.mark.gpu
BF16, F16 = 1, 2


@pytest.fixture(scope='module')
def lib():
  import spa3d
  return spa3d._lib.load()


def _s():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _case(nseq, S, H, dtype, ragged, masked, seed=3):
  g = torch.Generator().manual_seed(seed)
  tdt = torch.bfloat16 if dtype == BF16 else torch.float16
  E = H * 96
  lens = [S] * nseq
  if ragged:
    lens = [max(2, S - int(x)) for x in torch.randint(0, 40, (nseq,), generator=g)]
    lens[0] = S; lens[-1] = 17 if nseq > 1 else S
  off = [0]
  for n in lens:
    off.append(off[-1] + n)
  rows = off[-1]
  nq = torch.randn(rows, 384, generator=g).to(tdt)
  w = [(torch.randn(384, E, generator=g) / math.sqrt(384)).to(tdt) for _ in range(3)]
  sq = 1 + 0.2 * torch.randn(96, generator=g); sk = 1 + 0.2 * torch.randn(96, generator=g)
  km = None
  if masked and not ragged:
    km = (torch.rand(nseq, S, generator=g) < 0.8).float(); km[:, 0] = 1.0
  return lens, off, nq, w, sq, sk, km


def _oracle(lens, off, nq, w, sq, sk, km, H):
  q = (nq.double() @ w[0].double()).to(nq.dtype).double()   # the projection output is stored in 16 bits; everything downstream starts from it
  k = (nq.double() @ w[1].double()).to(nq.dtype).double()
  v = (nq.double() @ w[2].double()).to(nq.dtype).double()
  outs = []
  for i, n in enumerate(lens):
    sl = slice(off[i], off[i + 1])
    qq = O.rms_norm(q[sl].view(1, n, H, 96), sq.double()); kk = O.rms_norm(k[sl].view(1, n, H, 96), sk.double())
    mask = None if km is None else km[i].view(1, 1, 1, n)
    outs.append(O.dot_product_attention(qq, kk, v[sl].view(1, n, H, 96), mask).reshape(n, H * 96))
  return torch.cat([q, k, v], dim=1), torch.cat(outs, dim=0)


@pytest.mark.parametrize('nseq,S,H,dtype,ragged,masked', [(3, 151, 8, BF16, False, False), (5, 151, 8, BF16, True, False), (4, 151, 8, BF16, False, True),
                                                          (9, 129, 8, BF16, False, False), (2, 160, 8, F16, False, True), (17, 151, 8, F16, True, False),
                                                          (3, 40, 2, BF16, False, True), (300, 151, 8, BF16, True, False)])
def test_qkv_attention_fused_vs_oracle_and_two_kernel_path(lib, nseq, S, H, dtype, ragged, masked):
  """Ragged cases take the two-kernel comparison through spa3d_op_attention_ragged (same offsets, from the host), under the dense cases' three assertions.
  The first time it ran, [300-151-8-1-True-False] (bf16, 39 717 rows, 635 472 lse slots) missed |d lse| < 1e-3 with 3.13e-3 (29 slots above 1e-3): the fused
  kernel summed x^2 for the two RMSNorms in another order than the attention kernels, its rsqrt argument differed by an fp32 ulp now and then, and about one
  element of q^ / k^ in 10^5 rounded to the other bf16 neighbour.  qkva_fwd_kernel now sums in the attention kernels' order (csrc/qkv_attn.hip); measured
  since: bf16 max |d lse| 1.2e-6 in every case, no slot above 1e-5.  The fp16 cases measure 1.1e-4 (dense) and 4.7e-4 (ragged), as before that change."""
  lens, off, nq, w, sq, sk, km = _case(nseq, S, H, dtype, ragged, masked)
  E, rows = H * 96, off[-1]
  tdt = nq.dtype
  d = lambda t: None if t is None else t.cuda()
  nqd, wd, sqd, skd, kmd = d(nq), [d(x) for x in w], d(sq), d(sk), d(km)
  offd = torch.tensor(off, dtype=torch.int32, device='cuda') if ragged else None
  qkv = torch.full((rows, 3 * E), float('nan'), device='cuda', dtype=tdt)
  o = torch.full((rows, E), float('nan'), device='cuda', dtype=tdt)
  lse = torch.full((rows * H * 2,), float('nan'), device='cuda')
  ws = torch.empty(64 << 20, dtype=torch.uint8, device='cuda')
  rc = lib.spa3d_op_qkv_attention(nqd.data_ptr(), 384, wd[0].data_ptr(), wd[1].data_ptr(), wd[2].data_ptr(), sqd.data_ptr(), skd.data_ptr(),
                                  None if kmd is None else kmd.data_ptr(), None if offd is None else offd.data_ptr(), nseq, S, H, qkv.data_ptr(), o.data_ptr(),
                                  lse.data_ptr(), dtype, ws.data_ptr(), ws.numel(), _s())
  assert rc == 0
  torch.cuda.synchronize()
  qkv_ref, o_ref = _oracle(lens, off, nq, w, sq, sk, km, H)
  assert not torch.isnan(qkv.float()).any() and not torch.isnan(o.float()).any()
  eps = 2.0 ** -8 if dtype == BF16 else 2.0 ** -11
  # q | k | v: the fp32-accumulated product rounded once -- a handful of elements may fall on the other side of a rounding boundary than the fp64 product's rounding
  assert rel_err(qkv.float(), qkv_ref) < 1.5 * eps / math.sqrt(3)
  assert max_abs(qkv.float(), qkv_ref) <= eps * float(qkv_ref.abs().max())
  assert rel_err(o.float(), o_ref) < (1.2e-2 if dtype == BF16 else 1.6e-3)   # the fused attention kernel's own bound (tests/test_gpu_ops.py)
  # against the two-kernel path on the SAME stored q | k | v: identical rounding points -> equal up to fp32 summation order of the two MFMA contractions
  # (ragged: the same offsets through spa3d_op_attention_ragged, which takes them from the host; both kernels put lse at the same ragged position)
  o2 = torch.empty_like(o); lse2 = torch.full((rows * H * 2,), float('nan'), device='cuda')
  if ragged:
    rc = lib.spa3d_op_attention_ragged(qkv.data_ptr(), qkv[:, E:].data_ptr(), qkv[:, 2 * E:].data_ptr(), 3 * E, 3 * E, 3 * E, sqd.data_ptr(), skd.data_ptr(),
                                       None, (C.c_int32 * len(off))(*off), nseq, S, H, 96, o2.data_ptr(), lse2.data_ptr(), dtype, 2, ws.data_ptr(), ws.numel(), _s())
  else:
    rc = lib.spa3d_op_attention(qkv.data_ptr(), qkv[:, E:].data_ptr(), qkv[:, 2 * E:].data_ptr(), 3 * E, 3 * E, 3 * E, sqd.data_ptr(), skd.data_ptr(),
                                None if kmd is None else kmd.data_ptr(), nseq, S, S, H, 96, o2.data_ptr(), lse2.data_ptr(), dtype, 2, ws.data_ptr(), ws.numel(), _s())
  assert rc == 0
  torch.cuda.synchronize()
  frac = float((o2.view(torch.int16) != o.view(torch.int16)).float().mean())
  print(f'fused vs two kernels: o differs in {frac:.2e} of the elements; lse max abs diff {float((lse2 - lse).abs().max()):.2e}')
  assert rel_err(o.float(), o2.float()) < 2 * eps and frac < 0.05
  assert float((lse2 - lse).abs().max()) < 1e-3


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_qkv_attention_fused_in_model_equals_the_two_kernel_path(precision, tmp_path):
  """attn_impl 6 (the fused kernel in the track encoder's blocks, ragged pruned sequences included) against the default dispatch on the full-size T = 150 model:
  same rounding points, a different projection kernel (fp32 summation order), so the two runs differ like any two 16-bit paths of the suite do."""
  import os, sys
  import spa3d
  from util import batch_to, product_model
  sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
  import make_t150_golden as G
  cfg, p, batch, noise = G.make_inputs('c772')
  outs = {}
  for impl in (0, 6):
    model = product_model(spa3d, cfg, precision)
    gb = batch_to(batch, 'cuda')
    for k in ('dino_features', 'depth_features'):
      gb[k] = gb[k].to(torch.bfloat16 if precision == 'bf16' else torch.float16)
    gp = O.tree_map(lambda t: t.cuda(), p)
    h = model._handle(*model._dims_from_params(gp))[0]
    lib_ = spa3d._lib.load()
    spa3d._lib.check(lib_.spa3d_set_option(h, b'attn_impl', float(impl)), h)
    lib_.spa3d_prof_enable(h, 1)
    ld, grads, preds = model.loss_and_grads({'params': gp}, gb, noise=noise.cuda(), return_predictions=True)
    torch.cuda.synchronize()
    lib_.spa3d_prof_dump.restype = C.c_int; lib_.spa3d_prof_dump.argtypes = [C.c_void_p, C.c_char_p]
    path = str(tmp_path / f'qa_prof_{precision}_{impl}.csv')
    assert lib_.spa3d_prof_dump(h, path.encode()) == 0
    lib_.spa3d_prof_enable(h, 0)
    spa3d._lib.check(lib_.spa3d_set_option(h, b'attn_impl', 0.0), h)
    fused = sum(1 for line in open(path) if line.split(',')[0] == '3' and int(line.strip().split(',')[7]) == 2)   # class attention forward, tag[3] = 2: qkv_attn_launch
    outs[impl] = (float(ld['total_loss']), preds.tracks.clone(), {k: v.clone() for k, v in O.tree_flatten(grads).items()}, fused)
  assert outs[6][3] >= 2 and outs[0][3] == 0, (outs[6][3], outs[0][3])   # the two full encoder blocks ran fused under 6, none by default
  e_t = rel_err(outs[6][1], outs[0][1])
  worst = max((rel_err(outs[6][2][k], outs[0][2][k]), k) for k in outs[0][2] if float(outs[0][2][k].double().norm()) > 1e-3 * max(float(v.double().norm()) for v in outs[0][2].values()))
  print(f'{precision}: fused QKV + attention in model vs the default dispatch: tracks rel {e_t:.3e}, worst significant gradient leaf {worst}')
  # two 16-bit paths whose q | k | v come from different GEMM kernels (fp32 summation order -> different 16-bit roundings, amplified by the layers behind):
  # the bounds of tests/test_gpu_round4_ab.py; measured here 6.0e-3 / 0.18 (bf16)
  assert e_t < (9.5e-3 if precision == 'bf16' else 1.2e-3)
  assert worst[0] < (0.28 if precision == 'bf16' else 3.6e-2)   # fp16 measured 2.4e-2
