"""The latent-set metrics on the GPU (include/spa3d.h "Latent-set metrics", csrc/motion.hip): every result is an integer and is compared with the
NumPy int64 restatement (tests/motion_util.py) EXACTLY -- no tolerance anywhere.

  1. spa3d_motion_codes: sizes with and without a vector body and tail, an unaligned base, the host test's table of edge values, the NaN count,
     and model.motion_codes of the mini model.
  2. spa3d_motion_moments_add: both pools; one tile and several, D not a multiple of the tile or of 4; random codes and all +-128; the call ADDS;
     70 clips in one call, in three, and in the reverse order give the same bits; two runs are bit-equal.
  3. spa3d_motion_pdist: one tile and several with ragged edges; E below, at and above the chunk, tails that are no multiple of 32 (and, beyond the
     listed sizes, no multiple of 8: the scalar staging path); both kinds; the chunk-rule case at E = 12288 on codes from {127, 128}.
  4. precision_recall on hand-built sets with exact ties.
  5. Refused calls write nothing.
Outputs of the C calls sit in canary-guarded allocations (parity_util.guarded)."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_util as MU
import parity_util as PU
from util import MINI, O, batch_to, product_model

pytestmark = pytest.mark.gpu
POISON16, POISON32 = -9999, -77777777


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


def _stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guard1d(n, dtype, fill, name):
  """n elements of a 2- or 4-byte type inside a canary-guarded allocation, as a flat contiguous view"""
  rows, cols = (n // 96, 96) if n % 96 == 0 and n >= 96 else (1, n)
  return PU.guarded(rows, cols, dtype, name=name, fill=fill).reshape(-1)


def _guard_state(D):
  """a zeroed int64 [1 + D + D * D] moment state inside a guarded allocation (the guards know 2- and 4-byte types: an int32 view of twice the length)"""
  n = 1 + D + D * D
  return _guard1d(2 * n, torch.int32, 0, 'state').view(torch.int64)


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------- 1. codes
def _codes_c(spa3d, lat):
  """spa3d_motion_codes itself on a float32 device tensor (any alignment): (codes int16 NumPy, bad)"""
  lib, h = spa3d._lib.load(), spa3d.motion._motion_handle()
  n = lat.numel()
  codes = _guard1d(n, torch.int16, POISON16, 'codes')
  bad = _guard1d(1, torch.int32, POISON32, 'bad')
  spa3d._lib.check(lib.spa3d_motion_codes(h, lat.data_ptr(), n, codes.data_ptr(), bad.data_ptr(), _stream()), h, 'spa3d_motion_codes')
  torch.cuda.synchronize()
  res = codes.cpu().numpy().copy(), int(bad.item())
  PU.check_guards()
  return res


def _latents(n, seed):
  rng = np.random.default_rng(seed)
  x = (rng.standard_normal(n) * 0.7).astype(np.float32)          # about 15 % beyond +-1
  x[rng.integers(0, n, max(1, n // 50))] = rng.integers(-128, 128, max(1, n // 50)).astype(np.float32) / 128 + np.float32(0.5 / 128)   # exact ties
  return x


@pytest.mark.parametrize('n', [1, 63, 4097, 128 * 96 * 3])
def test_codes_equal_the_restatement(spa3d, n):
  x = _latents(n, n)
  want, _ = MU.codes(x)
  got, bad = _codes_c(spa3d, _dev(x))
  assert bad == 0 and np.array_equal(got, want) and np.abs(got).max() <= 128
  # a base that is 4 bytes off the 16-byte grid takes the scalar kernel: the same codes
  buf = torch.zeros(n + 1, dtype=torch.float32, device='cuda')
  buf[1:] = _dev(x)
  assert buf[1:].data_ptr() % 16 == 4
  got, bad = _codes_c(spa3d, buf[1:])
  assert bad == 0 and np.array_equal(got, want)
  # the Python wrapper is the same call and keeps the shape
  py = spa3d.motion_codes(_dev(x).reshape(1, -1))
  assert py.dtype == torch.int16 and tuple(py.shape) == (1, n) and np.array_equal(py.cpu().numpy().reshape(-1), want)


def test_codes_of_the_edge_table(spa3d):
  x = MU.edge_values()
  want, nbad = MU.codes(x)
  got, bad = _codes_c(spa3d, _dev(x))
  assert nbad == 4 == bad and np.array_equal(got, want)
  assert got[np.isnan(x)].tolist() == [0] * 4 and got[np.isinf(x)].tolist() == [128, -128]
  with pytest.raises(ValueError, match='4 of .* NaN'):
    spa3d.motion_codes(_dev(x))


@pytest.mark.parametrize('nans', [0, 1, 37])
def test_bad_counts_the_nans_exactly(spa3d, nans):
  n = 4097
  x = _latents(n, 7)
  where = np.random.default_rng(nans).permutation(n)[:nans]
  if nans:
    where[0] = n - 1                                             # one in the scalar tail
  x[where] = np.nan
  want, nbad = MU.codes(x)
  got, bad = _codes_c(spa3d, _dev(x))
  assert bad == nbad == nans and np.array_equal(got, want) and not got[where].any()


def test_model_motion_codes_is_the_code_of_encode(spa3d):
  cfg = O.Config(**MINI, use_dino=False, use_depth=False)
  model = product_model(spa3d, cfg, 'fp32')
  gb = batch_to(O.synthetic_batch(3, 6, 5, 8, seed=1234), 'cuda')
  params = model.init(0, gb)['params']
  g = torch.Generator().manual_seed(0)
  for k, v in O.tree_flatten(params).items():
    if k.endswith('bias') or k.endswith('scale'):
      v.add_((0.1 * torch.randn(v.shape, generator=g)).to(v.device))
  lat = model.encode({'params': params}, gb)
  codes = model.motion_codes({'params': params}, gb)
  want, nbad = MU.codes(lat.cpu().numpy())
  assert nbad == 0 and codes.dtype == torch.int16 and tuple(codes.shape) == (3, cfg.num_latent_tokens, cfg.latent_token_dim)
  assert np.array_equal(codes.cpu().numpy(), want) and len(np.unique(want)) > 1
  # and the codes feed the statistics and the distances as they are
  st = spa3d.MotionStats(cfg.latent_token_dim, cfg.num_latent_tokens, 'token').update(codes)
  assert np.array_equal(st.state.cpu().numpy(), MU.moments(want, MU.TOKEN))
  assert np.array_equal(spa3d.motion_pdist(codes).cpu().numpy(), MU.pdist(want.reshape(3, -1), want.reshape(3, -1), MU.SQDIST))


# ---------------------------------------------------------------------------------------------- 2. moments
def _moments_c(spa3d, codes, pool, state=None):
  lib, h = spa3d._lib.load(), spa3d.motion._motion_handle()
  M, L, D = codes.shape
  state = _guard_state(D) if state is None else state
  dc = _dev(codes)
  spa3d._lib.check(lib.spa3d_motion_moments_add(h, dc.data_ptr(), M, L, D, pool, state.data_ptr(), _stream()), h, 'spa3d_motion_moments_add')
  torch.cuda.synchronize()
  return state


def _codes_of(kind, shape, seed):
  rng = np.random.default_rng(seed)
  if kind == 'random':
    return rng.integers(-128, 129, shape).astype(np.int16)
  return (128 * (2 * rng.integers(0, 2, shape) - 1)).astype(np.int16)


MOMENT_SHAPES = [(1, 4, 8), (3, 128, 96), (70, 128, 96), (5, 7, 24), (2, 3, 100)]


@pytest.mark.parametrize('kind', ['random', 'pm128'])
@pytest.mark.parametrize('pool', [MU.TOKEN, MU.CLIP])
@pytest.mark.parametrize('shape', MOMENT_SHAPES)
def test_moments_equal_the_restatement(spa3d, shape, pool, kind):
  codes = _codes_of(kind, shape, sum(shape) + pool)
  want = torch.from_numpy(MU.moments(codes, pool))
  state = _moments_c(spa3d, codes, pool)
  got = state.cpu().clone()
  assert torch.equal(got, want), f'{int((got != want).sum())} of {want.numel()} entries differ'
  assert int(got[0]) == (shape[0] * shape[1] if pool == MU.TOKEN else shape[0])
  # the call ADDS: once more into the same state doubles every entry; and two runs are bit-equal
  _moments_c(spa3d, codes, pool, state)
  assert torch.equal(state.cpu(), 2 * want)
  PU.check_guards()
  assert torch.equal(_moments_c(spa3d, codes, pool).cpu(), got)
  PU.check_guards()


def test_all_plus_128_reaches_the_largest_sums(spa3d):
  codes = np.full((70, 128, 96), 128, np.int16)
  for pool, n, x in ((MU.TOKEN, 70 * 128, 128), (MU.CLIP, 70, 128 * 128)):
    got = _moments_c(spa3d, codes, pool).cpu().numpy()
    PU.check_guards()
    assert got[0] == n and (got[1:97] == n * x).all() and (got[97:] == n * x * x).all()


@pytest.mark.parametrize('pool', ['token', 'clip'])
def test_seventy_clips_in_one_call_in_three_and_reversed_give_the_same_bits(spa3d, pool):
  codes = _codes_of('random', (70, 128, 96), 70)
  dc = _dev(codes)
  want = torch.from_numpy(MU.moments(codes, MU.TOKEN if pool == 'token' else MU.CLIP))
  one = spa3d.MotionStats(96, 128, pool).update(dc)
  parts = (dc[:1], dc[1:6], dc[6:])
  assert [int(p.shape[0]) for p in parts] == [1, 5, 64]
  three, rev = spa3d.MotionStats(96, 128, pool), spa3d.MotionStats(96, 128, pool)
  for p in parts:
    three.update(p)
  for p in reversed(parts):
    rev.update(p)
  for s in (one, three, rev):
    assert s.state.is_cuda and s.n == int(want[0]) and torch.equal(s.state.cpu(), want)
  # two states merged are the state of all the clips; mean and cov in latent units
  a, b = spa3d.MotionStats(96, 128, pool).update(dc[:30]), spa3d.MotionStats(96, 128, pool).update(dc[30:])
  assert torch.equal(a.merge(b).state.cpu(), want)
  n, mu, cov = MU.stats(want.numpy(), 96, 128 if pool == 'token' else 128 * 128)
  assert a.n == n and np.array_equal(a.mean, mu) and np.array_equal(a.cov, cov)
  fd = spa3d.frechet_distance(one, a)
  assert abs(fd) <= 1e-7 * 2 * np.trace(cov)


def test_update_refusals(spa3d):
  st = spa3d.MotionStats(8, 4, 'clip')
  ok = torch.zeros(2, 4, 8, dtype=torch.int16, device='cuda')
  for bad in (ok[:, :3], ok[:, :, :7], ok[0], ok[:0]):
    with pytest.raises(ValueError, match='codes must be'):
      st.update(bad)
  with pytest.raises(ValueError, match='int16'):
    st.update(ok.int())
  assert st.n == 0 and not st.state.any()
  # the overflow refusal comes before the launch: the state keeps its bits
  big = spa3d.MotionStats(2, 4096, 'clip')
  full = torch.zeros(7, dtype=torch.int64)
  full[0] = 1 << 24
  big.load_state_dict({'D': 2, 'L': 4096, 'pool': 'clip', 'state': full})
  with pytest.raises(OverflowError, match='2\\^62'):
    big.update(torch.full((1, 4096, 2), 128, dtype=torch.int16, device='cuda'))
  assert torch.equal(big.state.cpu(), full) and big.n == 1 << 24


# ---------------------------------------------------------------------------------------------- 3. pairwise distances
def _pdist_c(spa3d, a, b, kind):
  """spa3d_motion_pdist itself on device tensors [Ma, E], [Mb, E]: int32 NumPy [Ma, Mb]"""
  lib, h = spa3d._lib.load(), spa3d.motion._motion_handle()
  Ma, E = a.shape
  Mb = b.shape[0]
  out = PU.guarded(Ma, Mb, torch.int32, name='out', fill=POISON32)
  spa3d._lib.check(lib.spa3d_motion_pdist(h, a.data_ptr(), Ma, b.data_ptr(), Mb, E, kind, out.data_ptr(), _stream()), h, 'spa3d_motion_pdist')
  torch.cuda.synchronize()
  res = out.cpu().numpy().copy()
  PU.check_guards()
  return res


def _same_ints(got, want, what):
  assert got.dtype == np.int32 and got.shape == want.shape
  bad = got.astype(np.int64) != want
  assert not bad.any(), f'{what}: {int(bad.sum())} of {want.size} entries differ, first at {tuple(np.argwhere(bad)[0])}: {got[bad][0]} for {want[bad][0]}'


PDIST_M = [(1, 1), (16, 17), (130, 33)]
PDIST_E = [96, 1000, 1024, 1056, 12288]


@pytest.mark.parametrize('kind', [MU.DOT, MU.SQDIST])
@pytest.mark.parametrize('E', PDIST_E)
@pytest.mark.parametrize('Ma,Mb', PDIST_M)
def test_pdist_equals_the_restatement(spa3d, Ma, Mb, E, kind):
  rng = np.random.default_rng(Ma * 100003 + E + kind)
  a, b = rng.integers(-128, 129, (Ma, E)).astype(np.int16), rng.integers(-128, 129, (Mb, E)).astype(np.int16)
  _same_ints(_pdist_c(spa3d, _dev(a), _dev(b), kind), MU.pdist(a, b, kind), f'{Ma} x {Mb}, E = {E}')


@pytest.mark.parametrize('E', [1, 37, 1001, 1031])
def test_pdist_of_rows_that_are_no_multiple_of_16_bytes(spa3d, E):
  """E % 8 != 0 (or a base off the 16-byte grid) stages by guarded scalar loads; the tail of the last K step is zeros"""
  rng = np.random.default_rng(E)
  a, b = rng.integers(-128, 129, (19, E)).astype(np.int16), rng.integers(-128, 129, (130, E)).astype(np.int16)
  for kind in (MU.DOT, MU.SQDIST):
    _same_ints(_pdist_c(spa3d, _dev(a), _dev(b), kind), MU.pdist(a, b, kind), f'E = {E}')
  buf = torch.zeros(19 * E + 1, dtype=torch.int16, device='cuda')
  buf[1:] = _dev(a).reshape(-1)
  _same_ints(_pdist_c(spa3d, buf[1:].view(19, E), _dev(b), MU.SQDIST), MU.pdist(a, b, MU.SQDIST), f'E = {E}, a 2 bytes off')


@pytest.mark.parametrize('Ma,Mb', PDIST_M)
def test_the_chunk_rule_case(spa3d, Ma, Mb):
  """E = 12288, codes drawn from {127, 128}: every product is 16 129, 16 256 or 16 384 with random parity, so the partial sums pass 2^24 with odd
  increments and an fp32 accumulator flushed less often than every MOTION_KCHUNK = 1024 elements rounds some of them: a wrong integer."""
  E = 12288
  rng = np.random.default_rng(Ma)
  a, b = (127 + rng.integers(0, 2, (Ma, E))).astype(np.int16), (127 + rng.integers(0, 2, (Mb, E))).astype(np.int16)
  want = MU.pdist(a, b, MU.DOT)
  assert want.min() > 11 * (1 << 24) and (want.size == 1 or ((want % 2).any() and (want % 2 == 0).any()))
  _same_ints(_pdist_c(spa3d, _dev(a), _dev(b), MU.DOT), want, 'dot')
  _same_ints(_pdist_c(spa3d, _dev(a), _dev(-b), MU.DOT), -want, 'dot, b negated')
  _same_ints(_pdist_c(spa3d, _dev(a), _dev(b), MU.SQDIST), MU.pdist(a, b, MU.SQDIST), 'sqdist')
  far = MU.pdist(a, -b, MU.SQDIST)
  assert far.max() < 1 << 31 and far.min() > 12288 * 254 * 254 - 1
  _same_ints(_pdist_c(spa3d, _dev(a), _dev(-b), MU.SQDIST), far, 'sqdist, b negated')
  # the extreme: all +128 against all -128
  p, m = np.full((Ma, E), 128, np.int16), np.full((Mb, E), -128, np.int16)
  got = _pdist_c(spa3d, _dev(p), _dev(m), MU.SQDIST)
  assert (got == 805306368).all() and 805306368 == 12288 * 256 * 256
  assert (_pdist_c(spa3d, _dev(p), _dev(m), MU.DOT) == -12288 * 128 * 128).all()


@pytest.mark.parametrize('kind', ['sqdist', 'dot'])
def test_motion_pdist_of_one_set_is_symmetric_with_a_zero_diagonal(spa3d, kind):
  codes = _codes_of('random', (33, 8, 16), 5)
  codes[7] = codes[2]                                              # a duplicated clip: an exact zero off the diagonal
  d = spa3d.motion_pdist(_dev(codes), kind=kind)
  assert d.dtype == torch.int32 and d.is_cuda and tuple(d.shape) == (33, 33)
  flat = codes.reshape(33, -1)
  _same_ints(d.cpu().numpy(), MU.pdist(flat, flat, MU.SQDIST if kind == 'sqdist' else MU.DOT), kind)
  assert torch.equal(d, d.t())
  if kind == 'sqdist':
    assert not d.diagonal().any() and int(d[7, 2]) == 0 and int((d == 0).sum()) == 35
  # two sets; and the two calls give equal bytes
  other = _codes_of('random', (5, 8, 16), 6)
  d2 = spa3d.motion_pdist(_dev(codes), _dev(other), kind=kind)
  _same_ints(d2.cpu().numpy(), MU.pdist(flat, other.reshape(5, -1), MU.SQDIST if kind == 'sqdist' else MU.DOT), kind)
  assert torch.equal(d2, spa3d.motion_pdist(_dev(codes), _dev(other), kind=kind))
  with pytest.raises(ValueError, match='elements per sample'):
    spa3d.motion_pdist(_dev(codes), _dev(other)[:, :, :8])
  with pytest.raises(ValueError, match='32767'):
    spa3d.motion_pdist(torch.zeros(2, 32768, dtype=torch.int16, device='cuda'))


# ---------------------------------------------------------------------------------------------- 4. precision / recall
@pytest.mark.parametrize('k', [1, 3])
def test_precision_recall_on_hand_built_sets_with_ties(spa3d, k):
  L, D = 4, 6
  base = np.zeros((L, D), np.int16)

  def clip(*moves):   # the base clip with element e moved by v codes: squared distance to the base = sum v^2
    c = base.copy().reshape(-1)
    for e, v in moves:
      c[e] += v
    return c.reshape(L, D)
  real = np.stack([clip(), clip(), clip((0, 3)), clip((1, 3)), clip((0, 3), (1, 4)), clip((5, 100))])               # 6 clips, two identical
  gen = np.stack([clip(), clip((0, 3)), clip((0, 3)), clip((2, 5)), clip((1, -3)), clip((5, 128)), clip((5, -128))])   # 7 clips, two identical, exact ties
  want = MU.precision_recall(real, gen, k)
  got = spa3d.precision_recall(_dev(real), _dev(gen), k=k)
  assert got == want and 0 < want[0] < 1 and 0 < want[1] <= 1
  # mirrored sets mirror the two numbers
  assert spa3d.precision_recall(_dev(gen), _dev(real), k=k) == want[::-1]
  with pytest.raises(ValueError, match='at least'):
    spa3d.precision_recall(_dev(real)[:k], _dev(gen), k=k)


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_a_refused_call_writes_nothing(spa3d):
  lib, h = spa3d._lib.load(), spa3d.motion._motion_handle()
  lat = torch.zeros(64, device='cuda')
  codes = torch.full((64 * 130,), POISON16, dtype=torch.int16, device='cuda')
  word = torch.full((130 * 130,), POISON32, dtype=torch.int32, device='cuda')
  state = torch.full((1 + 8 + 64,), POISON32, dtype=torch.int64, device='cuda')
  s = _stream()

  def refused(rc, text):
    assert rc == 1 and text in lib.spa3d_last_error(h).decode(), lib.spa3d_last_error(h)
  refused(lib.spa3d_motion_codes(h, lat.data_ptr(), -1, codes.data_ptr(), word.data_ptr(), s), 'n = -1')
  refused(lib.spa3d_motion_codes(h, None, 64, codes.data_ptr(), word.data_ptr(), s), 'latents')
  refused(lib.spa3d_motion_codes(h, lat.data_ptr(), 64, codes.data_ptr(), None, s), 'bad is required')
  for M, L, D, pool, text in ((0, 8, 8, 0, 'M = 0'), (4, 0, 8, 1, 'L = 0'), (4, 4097, 8, 0, 'L = 4097'), (4, 8, 0, 0, 'D = 0'), (4, 8, 257, 1, 'D = 257'), (4, 8, 8, 2, 'pool = 2')):
    refused(lib.spa3d_motion_moments_add(h, codes.data_ptr(), M, L, D, pool, state.data_ptr(), s), text)
  refused(lib.spa3d_motion_moments_add(h, codes.data_ptr(), 4, 8, 8, 0, None, s), 'state is required')
  for Ma, Mb, E, kind, text in ((0, 4, 64, 0, 'Ma = 0'), (4, 0, 64, 1, 'Mb = 0'), (4, 4, 0, 1, 'E = 0'), (4, 4, 32768, 0, 'E = 32768'), (4, 4, 64, 2, 'kind = 2'), (4, 4, 64, -1, 'kind = -1')):
    refused(lib.spa3d_motion_pdist(h, codes.data_ptr(), Ma, codes.data_ptr(), Mb, E, kind, word.data_ptr(), s), text)
  refused(lib.spa3d_motion_pdist(h, codes.data_ptr(), 4, None, 4, 64, 0, word.data_ptr(), s), 'b is required')
  torch.cuda.synchronize()
  assert bool((codes == POISON16).all()) and bool((word == POISON32).all()) and bool((state == POISON32).all())
  # the positive control: the same buffers, accepted
  assert lib.spa3d_motion_codes(h, lat.data_ptr(), 64, codes.data_ptr(), word.data_ptr(), s) == 0
  torch.cuda.synchronize()
  assert not codes[:64].any() and int(word[0]) == 0 and bool((codes[64:] == POISON16).all()) and bool((word[1:] == POISON32).all())
