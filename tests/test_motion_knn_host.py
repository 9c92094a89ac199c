"""Host side of the streaming k-NN, the ball hits and the manifold estimates, no GPU: the NumPy restatements (tests/motion_knn_util.py) against a
hand-computed case and against motion_util.precision_recall; the k-NN helpers of csrc/motion_code.hpp built with the host compiler against NumPy
BIT FOR BIT (key packing and order, the excluded column, the admissible count, the split plan and the tile ranges, the range checks, the
workspace size); and the Python refusals."""
import subprocess

import numpy as np
import pytest
import torch

import motion_knn_util as KU
import motion_util as MU
import spa3d
from util import host_check_driver


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_restatement_on_the_hand_computed_case():
  real, gen = KU.HAND_REAL, KU.HAND_GEN
  assert KU.knn(real, real, 1, 0)[0][:, 0].tolist() == KU.HAND['real_radius']
  assert KU.knn(gen, gen, 1, 0)[0][:, 0].tolist() == KU.HAND['gen_radius']
  assert KU.knn(real, real, 1, 0)[1][:, 0].tolist() == [1, 0, 1, 2, 5, 4]              # 2 is 2 away from 0 and from 4: the lower index
  rows, cols = KU.ball_hits(real, gen, KU.HAND['real_radius'], -1)
  assert cols.tolist() == KU.HAND['gen_in_real_balls'] and rows.tolist() == KU.HAND['real_ball_hits']
  m = KU.manifold(real, gen, 1)
  for name, want in KU.HAND.items():
    got = m[name]
    assert (got.tolist() if isinstance(got, np.ndarray) else got) == want, name
  # real 0: 1 from 1, and 10 000 <= 10 201 from -100; 2: 1 from 1 and from 3; 4: 1 from 3, 441 <= 484 from 25; 40: 225 from 25; 120, 122: none
  assert m['real_in_gen_balls'].tolist() == [2, 2, 2, 1, 0, 0]
  # self-exclusion by offset: rows 2.. of the set against the set leave out their own column, -1 leaves nothing out
  d, i = KU.knn(real[2:], real, 2, 2)
  assert i.tolist() == [[1, 0], [2, 1], [5, 3], [4, 3]] and d[:, 0].tolist() == [4, 1296, 4, 4]
  d, i = KU.knn(real[2:], real, 1, -1)
  assert i[:, 0].tolist() == [2, 3, 4, 5] and not d.any()
  # the distances the restatement sorts are motion_util's, to the bit, at the extremes too
  rng = np.random.default_rng(0)
  for Ma, Mb, E in ((7, 9, 1), (19, 33, 1001), (5, 6, 12288)):
    a, b = rng.integers(-128, 129, (Ma, E)).astype(np.int16), rng.integers(-128, 129, (Mb, E)).astype(np.int16)
    assert np.array_equal(KU.sqdist(a, b), MU.pdist(a, b, MU.SQDIST)) and KU.sqdist(a, b).dtype == np.int64
  p, m = np.full((2, 32767), 128, np.int16), np.full((3, 32767), -128, np.int16)
  assert (KU.sqdist(p, m) == 32767 * 256 * 256).all() and not KU.sqdist(p, p).any()
  # the keys order as the stable sort does
  key = KU.keys(real, real, 0)
  assert (key.diagonal() == np.uint64(KU.NONE)).all() and np.array_equal(np.argsort(key, axis=1)[:, :3], KU.knn(real, real, 3, 0)[1])


@pytest.mark.parametrize('k', [1, 2, 3])
def test_precision_and_recall_equal_the_matrix_restatement(k):
  rng = np.random.default_rng(k)
  for trial in range(20):
    lo, hi = (-3, 4) if trial % 2 else (-128, 129)                                     # a small range: many exact ties and duplicates
    real = rng.integers(lo, hi, (int(rng.integers(k + 1, 12)), 3)).astype(np.int16)
    gen = rng.integers(lo, hi, (int(rng.integers(k + 1, 12)), 3)).astype(np.int16)
    if trial % 3 == 0:
      gen[0] = real[0]
      real[-1] = real[0]
    m = KU.manifold(real, gen, k)
    assert (m['precision'], m['recall']) == MU.precision_recall(real, gen, k), (trial, real.tolist(), gen.tolist())
    assert 0 <= m['coverage'] <= 1 and m['density'] >= m['precision'] / k
  real, gen = KU.tie_sets()
  m = KU.manifold(real, gen, k)
  assert (m['precision'], m['recall']) == MU.precision_recall(real, gen, k)


# ---------------------------------------------------------------------------------------------- the header against NumPy
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
  return host_check_driver(tmp_path_factory, 'motion_knn')


def _ask(driver, lines):
  out = subprocess.run([driver], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=120)
  assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
  res = out.stdout.splitlines()
  assert len(res) == len(lines)
  return res


def test_header_keys_pack_and_order_as_numpy_does(driver):
  assert _ask(driver, ['consts']) == [f'64 128 4096 512 4 {KU.NONE}']
  rng = np.random.default_rng(0)
  d = np.concatenate([[0, 0, 1, (1 << 31) - 1, (1 << 31) - 1, 805306368], rng.integers(0, 1 << 31, 500)]).astype(np.int64)
  j = np.concatenate([[0, (1 << 22) - 1, 0, 0, (1 << 22) - 1, 77], rng.integers(0, 1 << 22, 500)]).astype(np.int64)
  want = (d.astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64)
  got = [[int(t) for t in r.split()] for r in _ask(driver, [f'key {a} {b}' for a, b in zip(d, j)])]
  assert [g[0] for g in got] == want.tolist() and [g[1] for g in got] == d.tolist() and [g[2] for g in got] == j.tolist()
  assert max(g[0] for g in got) < KU.NONE
  # the order: by distance, equal distances by the lower index -- the lexicographic order of (d, j)
  pairs = [(int(d[p]), int(j[p]), int(d[q]), int(j[q])) for p, q in rng.integers(0, len(d), (300, 2))] + [(5, 9, 5, 10), (5, 10, 5, 9), (5, 9, 5, 9), (4, 4000000, 5, 0), (5, 0, 4, 4000000)]
  got = [int(r) for r in _ask(driver, ['less %d %d %d %d' % p for p in pairs])]
  assert got == [int((p[0], p[1]) < (p[2], p[3])) for p in pairs]


def test_header_exclusion_and_admissible_counts(driver):
  q = ['excl 0 0', 'excl 7 0', 'excl 7 5', 'excl 7 -1', f'excl {(1 << 22) - 1} {1 << 22}', 'adm 10 0', 'adm 10 -1', 'adm 10 9', 'adm 10 10', 'adm 1 0', 'adm 1 -1', 'adm 10 4000000']
  assert [int(r) for r in _ask(driver, q)] == [0, 7, 12, -1, (1 << 23) - 1, 9, 10, 9, 10, 0, 1, 10]
  # against the restatement's mask: the smallest row count of admissible columns
  for Ma, Mb, so in ((5, 9, 0), (5, 9, -1), (5, 9, 8), (5, 9, 9), (3, 3, 0), (1, 1, 0)):
    assert int(_ask(driver, [f'adm {Mb} {so}'])[0]) == KU.admissible(Ma, Mb, so).sum(1).min()


def _plan(Ma, Mb):
  rt, ct = -(-Ma // 128), -(-Mb // 128)
  return max(1, min(-(-512 // rt), ct // 4))


def test_header_split_plan_and_tile_ranges(driver):
  sizes = [(1, 1), (1, 2), (130, 700), (4096, 4096), (64, 262144), (50000, 50000), (1 << 22, 1 << 22), (1, 1 << 22), (1 << 22, 1), (128, 512), (129, 511), (70000, 1024)]
  got = [int(r) for r in _ask(driver, [f'splits {a} {b}' for a, b in sizes])]
  assert got == [_plan(a, b) for a, b in sizes]
  assert got[:5] == [1, 1, 1, 8, 512] and max(got) <= 512 and min(got) >= 1
  # the ranges: in order, disjoint, covering every tile once; empty ones where there are more ranges than tiles
  for tiles, splits in ((6, 1), (6, 2), (6, 3), (6, 7), (1, 4), (2048, 512), (32768, 4096), (5, 5)):
    r = [tuple(int(t) for t in line.split()) for line in _ask(driver, [f'range {tiles} {splits} {s}' for s in range(splits)])]
    assert r == [(tiles * s // splits, tiles * (s + 1) // splits) for s in range(splits)]
    assert r[0][0] == 0 and r[-1][1] == tiles and all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(a <= b for a, b in r)
    if splits > tiles:
      assert any(a == b for a, b in r)


def test_header_refusal_bounds_and_workspace(driver):
  OK, BAD_M, BAD_E, BAD_MB, BAD_K, BAD_SELF, BAD_SPLITS = 0, 1, 5, 7, 9, 10, 11
  M = 1 << 22
  cases = [('knn 1 2 96 1 0 0', OK), ('knn 130 700 96 8 0 7', OK), (f'knn {M} {M} 32767 64 -1 4096', OK), ('knn 0 2 96 1 0 0', BAD_M), (f'knn {M + 1} 2 96 1 0 0', BAD_M),
           ('knn 1 0 96 1 -1 0', BAD_MB), (f'knn 1 {M + 1} 96 1 -1 0', BAD_MB), ('knn 1 2 0 1 0 0', BAD_E), ('knn 1 2 32768 1 0 0', BAD_E), ('knn 1 2 96 1 -2 0', BAD_SELF),
           ('knn 1 2 96 0 0 0', BAD_K), ('knn 1 2 96 -1 0 0', BAD_K), ('knn 1 200 96 65 -1 0', BAD_K), ('knn 1 200 96 64 -1 0', OK),
           # k against the admissible columns: Mb = k with nothing left out, Mb = k + 1 with the own column left out; Mb = k with it left out is refused
           ('knn 8 8 96 8 -1 1', OK), ('knn 8 9 96 8 0 1', OK), ('knn 8 8 96 8 0 1', BAD_K), ('knn 3 8 96 8 5 1', BAD_K), ('knn 3 8 96 8 7 1', BAD_K), ('knn 3 8 96 8 8 1', OK),
           ('knn 1 1 96 1 0 0', BAD_K), ('knn 1 1 96 1 -1 0', OK),
           ('knn 1 2 96 1 0 -1', BAD_SPLITS), ('knn 1 2 96 1 0 4097', BAD_SPLITS), ('knn 1 2 96 1 0 4096', OK),
           ('ball 1 1 1 -1', OK), ('ball 130 33 12288 0', OK), (f'ball {M} {M} 32767 {M}', OK), ('ball 0 1 96 0', BAD_M), ('ball 1 0 96 0', BAD_MB), (f'ball 1 {M + 1} 96 0', BAD_MB),
           ('ball 1 1 0 0', BAD_E), ('ball 1 1 32768 0', BAD_E), ('ball 1 1 96 -2', BAD_SELF), ('ball 1 1 96 -100', BAD_SELF)]
  assert [int(v) for v in _ask(driver, [c for c, _ in cases])] == [w for _, w in cases]
  ws = [('ws 130 700 8 1', 0), ('ws 130 700 8 2', 2 * 130 * 8 * 8), ('ws 130 700 8 7', 7 * 130 * 8 * 8), ('ws 130 700 8 0', 0), ('ws 4096 4096 3 0', 8 * 4096 * 3 * 8),
        ('ws 64 262144 5 0', 512 * 64 * 5 * 8), (f'ws {M} {M} 64 4096', 4096 * M * 64 * 8), ('ws 8192 8192 3 0', 8 * 8192 * 3 * 8),
        ('ws 0 700 8 1', -1), ('ws 130 0 8 1', -1), ('ws 130 700 0 1', -1), ('ws 130 700 65 1', -1), ('ws 130 700 8 -1', -1), ('ws 130 700 8 4097', -1), (f'ws {M + 1} 700 8 1', -1)]
  assert [int(v) for v in _ask(driver, [c for c, _ in ws])] == [w for _, w in ws]
  # the library's own C entry answers the same, without a GPU
  lib = spa3d._lib.load()
  for q, want in ws:
    assert int(lib.spa3d_motion_knn_workspace_bytes(*[int(t) for t in q.split()[1:]])) == want


# ---------------------------------------------------------------------------------------------- Python refusals
def test_cpu_tensors_and_bad_arguments_are_refused():
  c = torch.zeros(6, 4, 5, dtype=torch.int16)
  rad = torch.zeros(6, dtype=torch.int32)
  E = spa3d._lib.Spa3dError
  for call in (lambda: spa3d.motion_knn(c), lambda: spa3d.motion_knn(c, c, k=2), lambda: spa3d.motion_knn(c[2:], c, k=2, query_offset=2), lambda: spa3d.motion_ball_hits(c, c, rad),
               lambda: spa3d.manifold_metrics(c, c, k=3)):
    with pytest.raises(E, match='HIP-only'):
      call()
  for k in (0, -1, 65, 1.0, True, None):
    with pytest.raises(ValueError, match='k'):
      spa3d.motion_knn(c, k=k)
    with pytest.raises(ValueError, match='k'):
      spa3d.manifold_metrics(c, c, k=k)
  with pytest.raises(ValueError, match='k = 6'):          # six samples, each left out of its own row: five to choose from
    spa3d.motion_knn(c, k=6)
  with pytest.raises(ValueError, match='k = 7'):
    spa3d.motion_knn(c, c, k=7)
  with pytest.raises(ValueError, match='k = 6'):
    spa3d.motion_knn(c[:2], c, k=6, query_offset=3)
  with pytest.raises(ValueError, match='at least 4'):
    spa3d.manifold_metrics(c[:3], c, k=3)
  with pytest.raises(ValueError, match='at least 4'):
    spa3d.manifold_metrics(c, c[:3], k=3)
  for bad in (c.int(), c.float()):
    with pytest.raises(ValueError, match='int16'):
      spa3d.motion_knn(bad)
    with pytest.raises(ValueError, match='int16'):
      spa3d.motion_knn(c, bad)
    with pytest.raises(ValueError, match='int16'):
      spa3d.manifold_metrics(c, bad, k=1)
  with pytest.raises(ValueError, match='elements per sample'):
    spa3d.motion_knn(c, c[:, :, :4])
  with pytest.raises(ValueError, match='elements per sample'):
    spa3d.manifold_metrics(c, c[:, :3], k=1)
  with pytest.raises(ValueError, match='tensor'):
    spa3d.motion_knn(np.zeros((3, 4), np.int16))
  with pytest.raises(ValueError, match='needs codes_ref'):
    spa3d.motion_knn(c, query_offset=1)
  with pytest.raises(ValueError, match='runs past'):
    spa3d.motion_knn(c, c, query_offset=1)
  with pytest.raises(ValueError, match='query_offset'):
    spa3d.motion_knn(c[:2], c, query_offset=-1)
  with pytest.raises(ValueError, match='splits'):
    spa3d.motion_knn(c, splits=-1)
  with pytest.raises(ValueError, match='rows and cols'):
    spa3d.motion_ball_hits(c, c, rad, rows=False, cols=False)
