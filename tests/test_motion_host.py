"""Host side of the latent-set metrics, no GPU: the NumPy restatements (tests/motion_util.py) against hand-computed values; csrc/motion_code.hpp built
with the host compiler against the restatement BIT FOR BIT (codes at every tie and edge, the state index helpers, every refusal bound);
spa3d.frechet_distance against closed forms; MotionStats' host side (merge, state dict, npz, overflow refusal, mean / cov); the precision / recall
selection against the sorting restatement; and the Python refusals.

Frechet gates.  Errors are stated relative to tr Sigma_a + tr Sigma_b.  The gates come from a CPU measurement of exactly this formula (D = 96, NumPy
float64): full-rank cases (n = 500, 9000) measured <= 5.3e-16 on uncorrelated codes, gate 1e-12 -- the correlated sets used here measure 1.8e-16 ..
1.4e-14, the diagonal cases 0; rank-deficient cases (n = 70 < D) measured 4.8e-9 .. 5.0e-9 (here 6.4e-10 .. 5.6e-9) -- the square roots of
round-off-sized eigenvalues -- gate 1e-7, a 20 x margin because that term depends on the LAPACK build.  The values a run measures are printed,
stand in every failure message, and those of one run are kept in profiles/r24_motion.log."""
import subprocess

import numpy as np
import pytest
import torch

import motion_util as MU
import spa3d
from util import host_check_driver

D96 = 96


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_restatement_on_hand_computed_values():
  c, bad = MU.codes(np.array([0.0, 1.0, -1.0, 0.5, 0.5 / 128, 1.5 / 128, 2.5 / 128, -0.5 / 128, -1.5 / 128, 3.0, -3.0, np.nan, np.inf, -np.inf, 0.3], np.float32))
  assert c.tolist() == [0, 128, -128, 64, 0, 2, 2, 0, -2, 128, -128, 0, 128, -128, 38] and bad == 1 and c.dtype == np.int16
  codes = np.array([[[1, -2], [3, 4]], [[-128, 128], [128, 128]]], np.int16)   # [M = 2, L = 2, D = 2]
  assert MU.moments(codes, MU.TOKEN).tolist() == [4, 4, 258, 1 + 9 + 2 * 128 * 128, -2 + 12, -2 + 12, 4 + 16 + 2 * 128 * 128]
  assert MU.moments(codes, MU.CLIP).tolist() == [2, 4, 258, 16, 8, 8, 4 + 256 * 256]
  a, b = np.array([[1, 2, 3], [-128, -128, -128]], np.int16), np.array([[3, 2, 1], [128, 128, 128], [0, 0, 0]], np.int16)
  assert MU.pdist(a, b, MU.DOT).tolist() == [[10, 768, 0], [-768, -3 * 128 * 128, 0]]
  assert MU.pdist(a, b, MU.SQDIST).tolist() == [[8, 127 ** 2 + 126 ** 2 + 125 ** 2, 14], [131 ** 2 + 130 ** 2 + 129 ** 2, 3 * 256 * 256, 3 * 128 * 128]]
  # four real points on a line, three generated: radii by hand (k = 1: the nearest other sample)
  real, gen = np.array([[0], [1], [3], [10]], np.int16), np.array([[2], [2], [20]], np.int16)
  # real radii^2 1, 1, 4, 49; generated radii^2 0, 0, 324.  gen 2 is within 1 of real 1 (and real 3's ball), gen 20 is 100 > 49 from real 10.
  # recall: real 0 -> (0 - 20)^2 = 400 > 324 and 4 > 0: out; 1 -> 361 out; 3 -> 289 <= 324 in; 10 -> 100 in
  assert MU.precision_recall(real, gen, 1) == (2 / 3, 0.5)


# ---------------------------------------------------------------------------------------------- the header against the restatement
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
  return host_check_driver(tmp_path_factory, 'motion_code')


def _ask(driver, lines):
  out = subprocess.run([driver], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=120)
  assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
  res = out.stdout.splitlines()
  assert len(res) == len(lines)
  return res


def test_header_codes_match_the_restatement_bit_for_bit(driver):
  rng = np.random.default_rng(0)
  x = np.concatenate([MU.edge_values(), (rng.standard_normal(4000) * 0.7).astype(np.float32), rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
  want, nbad = MU.codes(x)
  got = [tuple(int(t) for t in r.split()) for r in _ask(driver, [f'code {int(b):x}' for b in x.view(np.uint32)])]
  assert [g[0] for g in got] == want.tolist()
  assert [g[1] for g in got] == np.isnan(x).astype(int).tolist() and sum(g[1] for g in got) == nbad > 4
  # what the table is for: every tie went to the even code, the clip and the zeros
  ties = (np.arange(-128, 128) + 0.5) / 128.0
  tie_codes, _ = MU.codes(ties.astype(np.float32))
  assert (tie_codes % 2 == 0).all() and (np.abs(tie_codes - ties * 128) == 0.5).all()
  assert MU.codes(np.array([np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0)), -0.0, np.inf, -np.inf], np.float32))[0].tolist() == [128, 128, 0, 128, -128]
  assert np.abs(want).max() == 128


def test_header_state_helpers_and_constants(driver):
  assert _ask(driver, ['consts']) == [f'128 1024 4096 256 32767 {1 << 22}']
  assert 1024 * 128 * 128 == 1 << 24 and 32767 * 256 * 256 < 1 << 31 <= 32768 * 256 * 256
  for D in (1, 8, 96, 256):
    q = [f'len {D}', 's 0', f's {D - 1}', f'S {D} 0 0', f'S {D} {D - 1} {D - 1}', f'S {D} {D // 2} {D // 3}']
    want = [1 + D + D * D, 1, D, 1 + D, D + D * D, 1 + D + (D // 2) * D + D // 3]
    assert [int(v) for v in _ask(driver, q)] == want
    # the layout moments() of the restatement writes: n, s, S row-major
    st = MU.moments(np.arange(2 * 3 * D).reshape(2, 3, D) % 7 - 3, MU.TOKEN)
    assert st.shape == (want[0],)
  got = [int(v) for v in _ask(driver, ['samples 70 128 0', 'samples 70 128 1', 'sqmax 128 0', 'sqmax 128 1', 'nmax 128 0', 'nmax 128 1', 'nmax 4096 1', 'nmax 1 1'])]
  assert got == [70 * 128, 70, 1 << 14, (128 * 128) ** 2, 1 << 48, 1 << 34, 1 << 24, 1 << 48]
  for L in (1, 7, 128, 4096):
    for pool, name in ((0, 'token'), (1, 'clip')):
      assert int(_ask(driver, [f'nmax {L} {pool}'])[0]) == spa3d.motion.samples_max(L, name)


def test_header_refusal_bounds(driver):
  OK, BAD_M, BAD_L, BAD_D, BAD_POOL, BAD_E, BAD_KIND, BAD_MB, BAD_N = range(9)
  cases = [('codes 0', OK), ('codes 1', OK), ('codes -1', BAD_N), (f'codes {1 << 40}', OK),
           ('mom 1 1 1 0', OK), ('mom 70 128 96 1', OK), ('mom 1 4096 256 1', OK), ('mom 0 128 96 0', BAD_M), ('mom -5 128 96 0', BAD_M), (f'mom {(1 << 40) + 1} 1 1 0', BAD_M),
           ('mom 1 0 96 0', BAD_L), ('mom 1 4097 96 0', BAD_L), ('mom 1 -1 96 1', BAD_L), ('mom 1 128 0 0', BAD_D), ('mom 1 128 257 0', BAD_D), ('mom 1 128 -3 1', BAD_D),
           ('mom 1 128 96 2', BAD_POOL), ('mom 1 128 96 -1', BAD_POOL),
           ('pd 1 1 1 0', OK), ('pd 130 33 12288 1', OK), (f'pd {1 << 22} {1 << 22} 32767 1', OK), ('pd 0 1 96 0', BAD_M), (f'pd {(1 << 22) + 1} 1 96 0', BAD_M),
           ('pd 1 0 96 0', BAD_MB), ('pd 1 -1 96 0', BAD_MB), (f'pd 1 {(1 << 22) + 1} 96 0', BAD_MB), ('pd 1 1 0 0', BAD_E), ('pd 1 1 32768 1', BAD_E), ('pd 1 1 -7 1', BAD_E),
           ('pd 1 1 96 2', BAD_KIND), ('pd 1 1 96 -1', BAD_KIND)]
  assert [int(v) for v in _ask(driver, [c for c, _ in cases])] == [w for _, w in cases]


# ---------------------------------------------------------------------------------------------- Frechet distance
def _stats_of(codes, pool):
  M, L, D = codes.shape
  st = spa3d.MotionStats(D, L, pool)
  st.load_state_dict({'D': D, 'L': L, 'pool': pool, 'state': torch.from_numpy(MU.moments(codes, MU.TOKEN if pool == 'token' else MU.CLIP))})
  return st


def _hadamard(n):
  H = np.array([[1]], np.int64)
  while H.shape[0] < n:
    H = np.block([[H, H], [H, -H]])
  return H


def _gate(what, err, scale, gate):
  rel = abs(err) / scale
  line = f'frechet {what}: |error| / (tr Sa + tr Sb) = {rel:.3e} (gate {gate:.0e})'
  print(line)
  assert rel <= gate, line


#                    n,  M,   L, pool,   gate
FRECHET_SETS = [(500, 125, 4, 'token', 1e-12), (9000, 2250, 4, 'token', 1e-12), (70, 70, 4, 'clip', 1e-7)]


@pytest.mark.parametrize('n,M,L,pool,gate', FRECHET_SETS)
def test_frechet_identical_shifted_and_symmetric(n, M, L, pool, gate):
  rng = np.random.default_rng(n)
  mix = rng.integers(-3, 4, (D96, D96))
  ca = np.clip((rng.integers(-20, 21, (M, L, D96)) @ mix) // 8, -100, 100).astype(np.int16)   # correlated coordinates, room for the shift
  a = _stats_of(ca, pool)
  assert a.n == n and (np.linalg.matrix_rank(a.cov) == D96) == (n > D96)
  tr = 2.0 * float(np.trace(a.cov))
  # identical statistics: 0
  _gate(f'n = {n} identical', spa3d.frechet_distance(a, a), tr, gate)
  # one coordinate shifted by 20 codes in every token: the covariance is unchanged, the means differ by 20 / 128 in that coordinate
  cb = ca.copy()
  cb[:, :, 5] += 20
  b = _stats_of(cb, pool)
  assert np.abs(b.mean - a.mean).max() == abs(b.mean[5] - a.mean[5]) and abs((b.mean[5] - a.mean[5]) - 20 / 128) < 1e-15
  _gate(f'n = {n} shifted by 20 codes', spa3d.frechet_distance(a, b) - (20 / 128) ** 2, tr, gate)
  # symmetry in the arguments, on two unrelated sets
  cc = np.clip((rng.integers(-20, 21, (M, L, D96)) @ rng.integers(-3, 4, (D96, D96))) // 8, -128, 128).astype(np.int16)
  c = _stats_of(cc, pool)
  ab, ba = spa3d.frechet_distance(a, c), spa3d.frechet_distance(c, a)
  assert ab > 0
  _gate(f'n = {n} symmetry', ab - ba, float(np.trace(a.cov) + np.trace(c.cov)), gate)
  # (mean, cov) pairs are taken as they are
  assert spa3d.frechet_distance((a.mean, a.cov), (c.mean, c.cov)) == ab


@pytest.mark.parametrize('reps', [1, 8])
def test_frechet_of_two_diagonal_covariances(reps):
  """column d of the samples is amplitude[d] times row d + 1 of a 128 x 128 Hadamard matrix: zero mean, mutually orthogonal, so the covariance is
  exactly diag((amplitude / 128)^2) and the distance is sum_d (sigma_a - sigma_b)^2"""
  H = _hadamard(128)[1:D96 + 1].T                      # [128 samples, 96]
  rng = np.random.default_rng(reps)
  amp_a, amp_b = rng.integers(1, 129, D96), rng.integers(1, 129, D96)
  ca = np.tile(H * amp_a, (reps, 1)).astype(np.int16)[:, None, :]
  cb = np.tile(H * amp_b, (reps, 1)).astype(np.int16)[:, None, :]
  a, b = _stats_of(ca, 'token'), _stats_of(cb, 'token')
  assert a.n == 128 * reps and not a.mean.any() and np.array_equal(a.cov, np.diag((amp_a / 128.0) ** 2))
  want = float((((amp_a - amp_b) / 128.0) ** 2).sum())
  _gate(f'n = {128 * reps} diagonal', spa3d.frechet_distance(a, b) - want, float(np.trace(a.cov) + np.trace(b.cov)), 1e-12)


def test_frechet_refuses_mismatched_statistics():
  with pytest.raises(ValueError):
    spa3d.frechet_distance((np.zeros(3), np.eye(3)), (np.zeros(4), np.eye(4)))
  with pytest.raises(ValueError):
    spa3d.frechet_distance((np.zeros(3), np.eye(4)), (np.zeros(3), np.eye(3)))
  with pytest.raises(ValueError, match='no samples'):
    spa3d.frechet_distance(spa3d.MotionStats(4, 2), spa3d.MotionStats(4, 2))


# ---------------------------------------------------------------------------------------------- MotionStats, host side
@pytest.mark.parametrize('pool', ['token', 'clip'])
def test_merge_equals_the_concatenated_update_and_round_trips(pool, tmp_path):
  rng = np.random.default_rng(3)
  c1, c2 = (rng.integers(-128, 129, (m, 5, 7)).astype(np.int16) for m in (3, 4))
  a, b = _stats_of(c1, pool), _stats_of(c2, pool)
  both = _stats_of(np.concatenate([c1, c2]), pool)
  assert a.merge(b) is a and torch.equal(a.state, both.state) and a.n == both.n == (35 if pool == 'token' else 7) and a.state.dtype == torch.int64
  # mean and cov in latent units: numpy's biased covariance of the samples
  x = MU.samples(np.concatenate([c1, c2]), MU.TOKEN if pool == 'token' else MU.CLIP) / float(128 if pool == 'token' else 128 * 5)
  assert a.divisor == (128 if pool == 'token' else 640)
  assert np.allclose(a.mean, x.mean(0), rtol=0, atol=1e-15) and np.allclose(a.cov, np.cov(x.T, bias=True), rtol=0, atol=1e-14) and a.cov.dtype == np.float64
  # state dict and npz
  sd = a.state_dict()
  sd['state'][0] += 0
  fresh = spa3d.MotionStats(7, 5, pool).load_state_dict(sd)
  assert torch.equal(fresh.state, a.state) and fresh.n == a.n and fresh.state.data_ptr() != sd['state'].data_ptr()
  back = spa3d.MotionStats.load(a.save(str(tmp_path / 'stats')))
  assert (back.D, back.L, back.pool, back.n) == (7, 5, pool, a.n) and torch.equal(back.state, a.state)
  # all_reduce without a process group leaves the state alone
  assert torch.equal(back.all_reduce().state, a.state)
  for bad in (spa3d.MotionStats(7, 4, pool), spa3d.MotionStats(6, 5, pool), spa3d.MotionStats(7, 5, 'clip' if pool == 'token' else 'token'), 'x'):
    with pytest.raises(ValueError, match='another kind'):
      a.merge(bad)
  with pytest.raises(ValueError, match='another kind'):
    spa3d.MotionStats(7, 4, pool).load_state_dict(sd)
  with pytest.raises(ValueError, match='int64'):
    fresh.load_state_dict(dict(sd, state=sd['state'][:-1]))
  with pytest.raises(ValueError, match='int64'):
    fresh.load_state_dict(dict(sd, state=sd['state'].to(torch.int32)))


def test_overflow_refusal_and_constructor_refusals():
  lim = spa3d.motion.samples_max(4096, 'clip')
  assert lim == 1 << 24 and spa3d.motion.samples_max(128, 'token') == 1 << 48
  def full(n):
    st = torch.zeros(1 + 2 + 4, dtype=torch.int64)
    st[0] = n
    return {'D': 2, 'L': 4096, 'pool': 'clip', 'state': st}
  a = spa3d.MotionStats(2, 4096, 'clip').load_state_dict(full(lim))
  assert a.n == lim
  with pytest.raises(OverflowError, match='2\\^62'):
    spa3d.MotionStats(2, 4096, 'clip').load_state_dict(full(lim + 1))
  one = spa3d.MotionStats(2, 4096, 'clip').load_state_dict(full(1))
  before = a.state.clone()
  with pytest.raises(OverflowError, match='2\\^62'):
    a.merge(one)
  assert torch.equal(a.state, before) and a.n == lim      # a refused merge adds nothing
  for args in ((0, 4), (257, 4), (4, 0), (4, 4097), (4.0, 4), (True, 4)):
    with pytest.raises(ValueError):
      spa3d.MotionStats(*args)
  with pytest.raises(ValueError, match='pool'):
    spa3d.MotionStats(4, 4, 'frame')


# ---------------------------------------------------------------------------------------------- precision / recall: the selection
@pytest.mark.parametrize('k', [1, 2, 3])
def test_knn_selection_equals_the_sorting_restatement(k):
  rng = np.random.default_rng(k)
  for trial in range(20):
    real = rng.integers(-3, 4, (int(rng.integers(k + 1, 9)), 3)).astype(np.int16)   # a small range: many exact ties and duplicates
    gen = rng.integers(-3, 4, (int(rng.integers(k + 1, 9)), 3)).astype(np.int16)
    if trial % 3 == 0:
      gen[0] = real[0]
      real[-1] = real[0]
    d = lambda a, b: torch.from_numpy(MU.pdist(a, b, MU.SQDIST))
    got = spa3d.motion.knn_precision_recall(d(real, real), d(gen, gen), d(real, gen), k)
    assert got == MU.precision_recall(real, gen, k), (trial, real.tolist(), gen.tolist())
  with pytest.raises(ValueError, match='at least'):
    spa3d.motion.knn_precision_recall(torch.zeros(k, k), torch.zeros(k + 1, k + 1), torch.zeros(k, k + 1), k)


# ---------------------------------------------------------------------------------------------- Python refusals
def test_cpu_tensors_and_bad_arguments_are_refused():
  c = torch.zeros(3, 4, 5, dtype=torch.int16)
  E = spa3d._lib.Spa3dError
  for call in (lambda: spa3d.motion_codes(torch.zeros(2, 4, 5)), lambda: spa3d.MotionStats(5, 4).update(c), lambda: spa3d.motion_pdist(c), lambda: spa3d.motion_pdist(c, c, kind='dot'),
               lambda: spa3d.precision_recall(torch.zeros(4, 2, dtype=torch.int16), torch.zeros(5, 2, dtype=torch.int16), k=3)):
    with pytest.raises(E, match='HIP-only'):
      call()
  with pytest.raises(ValueError, match='kind'):
    spa3d.motion_pdist(c, kind='l1')
  with pytest.raises(ValueError, match='tensor'):
    spa3d.motion_pdist(np.zeros((3, 4), np.int16))
  with pytest.raises(ValueError, match='at least 4'):
    spa3d.precision_recall(torch.zeros(3, 2, dtype=torch.int16), torch.zeros(5, 2, dtype=torch.int16), k=3)
  with pytest.raises(ValueError, match='at least 4'):
    spa3d.precision_recall(torch.zeros(5, 2, dtype=torch.int16), torch.zeros(3, 2, dtype=torch.int16), k=3)
  with pytest.raises(ValueError, match='positive int'):
    spa3d.precision_recall(c, c, k=0)
  assert hasattr(spa3d.TrackAutoEncoder3D, 'motion_codes')
