"""fp16 mode (BASELINE.json configs[4]: "... T=300, C=772, fp16"): the same kernels compiled for IEEE fp16 as the 16-bit activation
type (common.hpp, -DSPA_F16=1), selected by precision='fp16' / dtype SPA3D_F16.  Op-level checks against the fp64 oracle on
fp16-rounded inputs (a build that ran the bf16 MFMA on fp16 bit patterns would be off by orders of magnitude), model-level checks
against the oracle directly and against the frozen T=150 / T=300 goldens.

Tolerances: fp16 keeps 11 significand bits (bf16: 8), so forward values are ~8x closer to the oracle than bf16's; the 16-bit backward
runs at loss x 2^k (k chosen per call so the head gradient's magnitude is <= 16, model.hip) and smaller contributions flush -- the BCE term at weight
1e-8 (train.py:96) is such a contribution; leaves it alone feeds are compared by norm against a floor."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import parity_util as PU
from util import MINI, O, batch_to, max_abs, product_model, rel_err

pytestmark = pytest.mark.gpu
F16 = 2


@pytest.fixture(scope='module')
def lib():
  import spa3d
  return spa3d._lib.load()


def _s():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ws(nbytes=256 << 20):
  return torch.empty(nbytes, dtype=torch.uint8, device='cuda')


FP16_TILED = [(4133, 2304, 384, 0, False, False), (777, 1536, 384, 1, False, True), (2050, 384, 1536, 0, True, True), (300, 600, 1280, 0, False, True),
              (70008, 512, 256, 0, True, True)]


@pytest.mark.parametrize('force8p', [False, True])
@pytest.mark.parametrize('M,N,K,act,res,bias', FP16_TILED)
def test_fp16_linear_tiled(lib, force8p, M, N, K, act, res, bias):
  IMPL = 3 if force8p else 2  # 3: the 8-phase kernels for any M
  g = torch.Generator().manual_seed(11)
  A = torch.randn(M, K, generator=g).half()
  B = (torch.randn(K, N, generator=g) / math.sqrt(K)).half()
  bs = torch.randn(N, generator=g) if bias else None
  R = torch.randn(M, N, generator=g).half() if res else None
  Ad, Bd = A.cuda(), B.cuda()
  bd = bs.cuda() if bias else None
  Rd = R.cuda() if res else None
  Cd = PU.guarded(M, N, torch.float16)
  ws = PU.poisoned_ws(PU.linear_ws_bytes(N, K))
  assert lib.spa3d_op_linear(Ad.data_ptr(), Bd.data_ptr(), bd.data_ptr() if bias else None, Rd.data_ptr() if res else None, Cd.data_ptr(),
                             M, N, K, act, F16, IMPL, ws.data_ptr(), ws.numel(), _s()) == 0
  PU.check_guards()
  ref = A.double() @ B.double()
  if bias:
    ref = ref + bs.double()
  pre = ref
  if act:
    ref = O.gelu_tanh(ref)
  if res:
    ref = ref + R.double()
  assert not torch.isnan(Cd.float()).any()
  assert rel_err(Cd.float(), ref) < 6e-4  # fp16 output rounding only (2^-12); accumulation is fp32
  PU.assert_elementwise(Cd, ref, PU.linear_bound(A, B, bs, R, act, ref, pre, torch.float16), 'C')


@pytest.mark.parametrize('M,N,K', [(5000, 384, 256), (3333, 2304, 384), (70001, 384, 768)])
def test_fp16_linear_bwd_tiled(lib, M, N, K):
  IMPL = 3  # the 8-phase TN kernels for any M
  g = torch.Generator().manual_seed(12)
  A = torch.randn(M, K, generator=g).half()
  B = (torch.randn(K, N, generator=g) / math.sqrt(K)).half()
  dC = torch.randn(M, N, generator=g).half()
  Ad, Bd, dCd = A.cuda(), B.cuda(), dC.cuda()
  dA = PU.guarded(M, K, torch.float16, name='dA')
  dB = PU.guarded(K, N, torch.float32, name='dB')
  db = PU.guarded(1, N, torch.float32, name='dbias')[0]
  ws = PU.poisoned_ws(PU.linear_ws_bytes(N, K))
  assert lib.spa3d_op_linear_bwd(Ad.data_ptr(), Bd.data_ptr(), dCd.data_ptr(), dA.data_ptr(), dB.data_ptr(), db.data_ptr(), M, N, K, F16, IMPL,
                                 ws.data_ptr(), ws.numel(), _s()) == 0
  PU.check_guards()
  rA, rB, rb = dC.double() @ B.double().T, A.double().T @ dC.double(), dC.double().sum(0)
  assert rel_err(dA.float(), rA) < 6e-4
  assert rel_err(dB, rB) < 1e-5  # exact fp16 products, fp32 accumulate + fp32 atomics
  assert rel_err(db, rb) < 1e-5
  PU.gate_linear_bwd(A, B, dC, dA, dB, db, rA, rB, rb, torch.float16)


@pytest.mark.parametrize('d', [384, 1280, 512, 1152, 100])
def test_fp16_layernorm(lib, d):
  """384 / 1280: the part kernels; 512 / 1152: the vectorised kernels in 1 / 3 steps; 100 (8 does not divide it): the plain kernels -- forward and backward, as
  tests/test_gpu_ops.py::test_layernorm_fwd_bwd lists them; rows 1, 3, 257 beside the 777 the test had.  Element-wise gates on y, dx and dscale."""
  for rows in (777, 1, 3, 257):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(rows, d, generator=g) * 3 + 1).half()
    sc = 1 + 0.1 * torch.randn(d, generator=g)
    dy = torch.randn(rows, d, generator=g).half()
    xd, scd, dyd = x.cuda(), sc.cuda(), dy.cuda()
    y = PU.guarded(rows, d, torch.float16, name='y'); st = PU.guarded(rows, 2, torch.float32, name='stats')
    assert lib.spa3d_op_layernorm(xd.data_ptr(), scd.data_ptr(), y.data_ptr(), st.data_ptr(), rows, d, F16, _s()) == 0
    PU.check_guards()
    assert rel_err(y.float(), O.layer_norm(x.double(), sc.double())) < 6e-4
    dx = PU.guarded(rows, d, torch.float16, name='dx'); ds = PU.guarded(1, d, torch.float32, name='dscale', fill=0.0)[0]
    assert lib.spa3d_op_layernorm_bwd(xd.data_ptr(), scd.data_ptr(), st.data_ptr(), dyd.data_ptr(), dx.data_ptr(), ds.data_ptr(), rows, d, F16, _s()) == 0
    PU.check_guards()
    y64, dx64, ds64 = PU.layernorm_restated(x, sc, dy, torch.float64)
    y32, dx32, ds32 = PU.layernorm_restated(x, sc, dy, torch.float32)
    PU.assert_elementwise(y, y64, PU.restated_bound(y64, y32, torch.float16), 'y')
    PU.assert_elementwise(dx, dx64, PU.restated_bound(dx64, dx32, torch.float16), 'dx')
    PU.assert_elementwise(ds, ds64, PU.restated_bound(ds64, ds32, torch.float32), 'dscale')


@pytest.mark.parametrize('bwd_mode', ['1', '3'])
@pytest.mark.parametrize('nseq,S,H,masked', [(9, 151, 8, True), (3, 129, 8, False), (3, 301, 8, True)])
def test_fp16_attention_fused(lib, nseq, S, H, masked, bwd_mode):
  import test_gpu_ops as TO
  if S > 192 and bwd_mode != '3':
    pytest.skip('S > 192 has one backward structure')
  BWD_IMPL = {'1': 2, '3': 4}[bwd_mode]
  Dh, E = 96, H * 96
  g = torch.Generator().manual_seed(21)
  qkv = torch.randn(nseq, S, 3 * E, generator=g).half()
  sq = 1 + 0.2 * torch.randn(Dh, generator=g); sk = 1 + 0.2 * torch.randn(Dh, generator=g)
  km = None
  if masked:
    km = (torch.rand(nseq, S, generator=g) < 0.8).float(); km[:, 0] = 1.0; km[0, 1:] = 0.0
  qkvd = qkv.cuda()
  o = PU.guarded(nseq * S, E, torch.float16, name='o').view(nseq, S, E)
  lse = PU.guarded(nseq * H * S, 2, torch.float32, name='lse', fill=0.0).view(nseq, H, S, 2)
  ws = PU.poisoned_ws(1 << 20)   # the LDS-resident kernels carve nothing from it
  sqd, skd = sq.cuda(), sk.cuda()
  kmd = km.cuda() if masked else None
  assert lib.spa3d_op_attention(qkvd[..., :E].data_ptr(), qkvd[..., E:2 * E].data_ptr(), qkvd[..., 2 * E:].data_ptr(), 3 * E, 3 * E, 3 * E,
                                sqd.data_ptr(), skd.data_ptr(), kmd.data_ptr() if masked else None, nseq, S, S, H, Dh, o.data_ptr(),
                                lse.data_ptr(), F16, 2, ws.data_ptr(), ws.numel(), _s()) == 0
  PU.check_guards()
  qr = qkv[..., :E].double().contiguous().requires_grad_(True)
  kr = qkv[..., E:2 * E].double().contiguous().requires_grad_(True)
  vr = qkv[..., 2 * E:].double().contiguous().requires_grad_(True)
  sqr, skr = sq.double().requires_grad_(True), sk.double().requires_grad_(True)
  ref = TO._attn_ref(qr, kr, vr, sqr, skr, km, H, Dh)
  e = rel_err(o.float(), ref.detach())
  print('fp16 fused attention fwd rel err', e)
  assert e < 3e-3  # bf16: 2e-2
  from util import Gates
  gt = Gates(f'fp16 fused self-attention forward, nseq {nseq} S {S} H {H} masked {masked}: kernel vs host emulation, both against the fp64 oracle')
  PU.attention_row_gate(gt, 'o', o, PU.emulate_attention(qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:], sq, sk, km, H, Dh), ref.detach(), H, Dh)
  gt.check()
  d_o = torch.randn(nseq, S, E, generator=g).half()
  ref.backward(d_o.double())
  dod = d_o.cuda()
  dqkv = PU.guarded(nseq * S, 3 * E, torch.float16, name='dqkv').view(nseq, S, 3 * E)
  dsq = PU.guarded(1, Dh, torch.float32, name='dsq', fill=0.0)[0]; dsk = PU.guarded(1, Dh, torch.float32, name='dsk', fill=0.0)[0]
  assert lib.spa3d_op_attention_bwd(qkvd[..., :E].data_ptr(), qkvd[..., E:2 * E].data_ptr(), qkvd[..., 2 * E:].data_ptr(), 3 * E, 3 * E, 3 * E,
                                    sqd.data_ptr(), skd.data_ptr(), kmd.data_ptr() if masked else None, nseq, S, S, H, Dh, o.data_ptr(),
                                    lse.data_ptr(), dod.data_ptr(), dqkv[..., :E].data_ptr(), dqkv[..., E:2 * E].data_ptr(),
                                    dqkv[..., 2 * E:].data_ptr(), dsq.data_ptr(), dsk.data_ptr(), F16, BWD_IMPL, ws.data_ptr(), ws.numel(), _s()) == 0
  PU.check_guards()
  errs = [rel_err(dqkv[..., :E].float(), qr.grad), rel_err(dqkv[..., E:2 * E].float(), kr.grad), rel_err(dqkv[..., 2 * E:].float(), vr.grad),
          rel_err(dsq, sqr.grad), rel_err(dsk, skr.grad)]
  print('fp16 fused attention bwd rel errs dq dk dv dsq dsk', errs)
  assert max(errs) < 5e-3  # bf16: 3e-2
  gb = Gates(f'fp16 fused self-attention backward, mode {bwd_mode} nseq {nseq} S {S} H {H} masked {masked}: kernel vs host emulation, both against the fp64 oracle')
  emu = PU.emulate_attention_bwd(qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:], sq, sk, km, H, Dh, d_o, fast=bwd_mode == '1' and not masked)
  PU.attention_grad_gates(gb, (dqkv[..., :E], dqkv[..., E:2 * E], dqkv[..., 2 * E:], dsq, dsk), emu, (qr.grad, kr.grad, vr.grad, sqr.grad, skr.grad), H, Dh)
  gb.check()


def _params_to_oracle(params, dtype):
  return O.tree_unflatten({k: v.detach().cpu().to(dtype) for k, v in O.tree_flatten(params).items()})


def test_fp16_mini_model_vs_oracle():
  import spa3d
  cfg = O.Config(**MINI, use_dino=True, use_depth=True, dino_feature_dim=24, depth_feature_dim=1)
  B, N, Q, T = 2, 12, 6, 8
  batch = O.synthetic_batch(B, N, Q, T, seed=1234, dino_dim=24, depth_dim=1)
  model = product_model(spa3d, cfg, 'fp16')
  gb = batch_to(batch, 'cuda')
  params = model.init(0, gb)['params']
  noise = torch.rand(B, cfg.num_latent_tokens, cfg.latent_token_dim, generator=torch.Generator().manual_seed(3))
  p64 = _params_to_oracle(params, torch.float64)
  b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
  b64['dino_features'] = batch['dino_features'].half().double()
  b64['depth_features'] = batch['depth_features'].half().double()
  ld_ref, preds_ref, grads_ref = O.loss_and_grads(O.TrackAutoEncoder3D(cfg), p64, b64, discretize=True, noise=noise.double())
  ld, grads, preds = model.loss_and_grads({'params': params}, gb, noise=noise.cuda(), return_predictions=True)
  e = rel_err(preds.tracks, preds_ref.tracks)
  print('fp16 mini tracks rel err', e)
  assert e < 1e-2  # bf16 mini test: 5e-2
  assert abs(float(ld['total_loss']) - float(ld_ref['total_loss'])) < 1e-2 * abs(float(ld_ref['total_loss']))
  gf = O.tree_flatten(grads)
  a = torch.cat([gf[k].double().cpu().reshape(-1) for k in sorted(grads_ref)])
  b = torch.cat([grads_ref[k].reshape(-1) for k in sorted(grads_ref)])
  cos = float((a @ b) / (a.norm() * b.norm()))
  print('fp16 mini grad cosine', cos)
  assert cos > 0.995 and bool(torch.isfinite(a).all())


@pytest.mark.parametrize('case', ['c772', 'c772_t300'])
def test_fp16_full_size_vs_oracle_golden(case):
  """Full-size model in fp16 at T=150 and at BASELINE configs[4]'s T = T_out = 300 (S = 301 fused attention forward + split-pass
  backward in-model, floor(t/150) in {0,1}, decoder window past the 1152 latent channels) against the frozen fp64 oracle outputs."""
  import spa3d
  import test_gpu_t150 as T150
  cfg, p, batch, noise, exp = T150._case(case)
  model = product_model(spa3d, cfg, 'fp16')
  gb = batch_to(batch, 'cuda')
  for k in ('dino_features', 'depth_features'):
    gb[k] = gb[k].half()  # exact: bf16-representable values of |x| < 65504 with 8 significand bits
  gp = O.tree_map(lambda t: t.cuda(), p)
  ld, grads, preds = model.loss_and_grads({'params': gp}, gb, noise=noise.cuda(), return_predictions=True)
  gf = O.tree_flatten(grads)
  e_t = rel_err(preds.tracks, torch.from_numpy(exp['tracks']))
  got = [float(ld[k]) for k in ('total_loss', 'position_loss', 'visible_loss')]
  print(f'{case} fp16: tracks rel {e_t:.3e} losses {got} vs {exp["losses"].tolist()}')
  names, rel, leaf = T150._leaf_report(gf, exp, f'{case} fp16')
  from util import Gates
  t300 = case == 'c772_t300'
  gt = Gates(f'{case} fp16 vs the fp64 oracle golden')
  gt.le('tracks, relative Frobenius', e_t, 1.9e-3, '1.0e-3 (T=150), 1.25e-3 (T=300); bf16: 7e-3')
  gt.le('total loss, relative', abs(got[0] - exp['losses'][0]) / abs(exp['losses'][0]), 9e-5, '6.5e-7 (T=150), 5.9e-5 (T=300)')
  gt.le('worst gradient-leaf norm, relative', float(rel.max()), 4.2e-2 if t300 else 6.5e-3, '2.8e-2 (T=300), 4.2e-3 (T=150)')
  gt.le('worst stored gradient leaf, relative', max(leaf.values()), 4.2e-2 if t300 else 6.5e-3, '2.8e-2 (T=300), 3.7e-3 (T=150)')
  gt.check()
  assert all(bool(torch.isfinite(gf[k]).all()) for k in names)
