"""The arithmetic of spa3d_build_batch (3dspa_code_amd/csrc/build_row.hpp) on the CPU: the header is plain C++ shared by the kernel and this
test, so a small driver (tests/host/build_row_check.cpp) is built with the host compiler (-ffp-contract=off, as the library) and run on the
inputs of tests/golden/sampler_golden.npz.  Expected, bit for bit: the reference's own outputs stored there.  The two 16-bit roundings are
compared with torch's, and the slot rule is probed at its edges.  No GPU needed."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch
from util import host_check_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, 'tests', 'golden', 'sampler_golden.npz'), allow_pickle=False)


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
  return host_check_driver(tmp_path_factory, 'build_row')


def _run(driver, mode, blob):
  out = subprocess.run([driver, mode], input=blob, capture_output=True, timeout=120)
  assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
  return out.stdout


def _sample(driver, intrinsics):
  tr, dp, dn = Z['tracks_2d'], Z['depth'], Z['dino']
  N, T = tr.shape[:2]
  _, Hp, Wp, D = dn.shape
  H, W = dp.shape[1:3]
  assert (N, T, D, Hp, Wp, H, W) == (23, 5, 40, 2, 3, 28, 42)
  intr = np.zeros(4) if intrinsics is None else np.asarray(intrinsics, np.float64)
  blob = struct.pack('<8i', N, T, D, Hp, Wp, H, W, int(intrinsics is not None)) + intr.tobytes() + tr.astype(np.float32).tobytes() + \
      dp.astype(np.float32).tobytes() + dn.astype(np.float32).tobytes()
  a = np.frombuffer(_run(driver, 'sample', blob), np.float32)
  n3, nd = N * T * 3, N * T * D
  return a[:n3].reshape(N, T, 3), a[n3:n3 + nd].reshape(N, T, D), a[n3 + nd:].reshape(N, T, 256)


def test_sampler_arithmetic_is_bit_identical_to_the_reference_outputs(driver):
  lift, dino, depth = _sample(driver, None)
  assert np.array_equal(lift.view(np.uint32), Z['lift_default'].view(np.uint32))
  assert np.array_equal(dino.view(np.uint32), Z['dino_tracks'].view(np.uint32))
  assert np.array_equal(depth.view(np.uint32), Z['depth_tracks'].view(np.uint32))
  lift_i, _, _ = _sample(driver, Z['intrinsics'])
  assert np.array_equal(lift_i.view(np.uint32), Z['lift_intr'].view(np.uint32))
  # the fixture does exercise the clamp: points outside the frame and on integer coordinates
  tr = Z['tracks_2d']
  assert (tr[..., 0] < 0).any() and (tr[..., 0] > 41).any() and (tr[..., 1] < 0).any() and (tr[..., 1] > 27).any() and (tr == np.floor(tr)).all(-1).any()


def _round_inputs():
  rng = np.random.default_rng(5)
  bits = rng.integers(0, 2**32, 200000, dtype=np.uint64).astype(np.uint32)
  x = bits.view(np.float32)
  x = x[~np.isnan(x)]
  edge = np.array([0.0, -0.0, 1.0, -1.0, 65504.0, 65519.99, 65520.0, 65536.0, -65520.0, 1e38, -1e38, np.inf, -np.inf, 2.0**-14, 2.0**-14 * (1 - 2.0**-11),
                   2.0**-24, 2.0**-25, 2.0**-25 * (1 + 2.0**-20), 2.0**-26, 1.5 * 2.0**-24, 2.5 * 2.0**-24, 3.0 * 2.0**-25, 1.0 + 2.0**-8, 1.0 + 2.0**-9, 1.0 + 3 * 2.0**-9,
                   1.0 + 2.0**-11, 1.0 + 3 * 2.0**-11, 1.0 + 2.0**-12, 3.3895314e38, 1e-45, 2047.0, 2049.0, 2051.0], np.float32)
  # values in the half range, where its rounding and its subnormals matter
  mid = (rng.standard_normal(100000) * np.exp(rng.uniform(-20, 12, 100000))).astype(np.float32)
  return np.concatenate([x, edge, -edge, mid])


def test_roundings_equal_torch(driver):
  x = _round_inputs()
  out = np.frombuffer(_run(driver, 'round', struct.pack('<i', len(x)) + x.tobytes()), np.uint16)
  bf, f16 = out[:len(x)], out[len(x):]
  t = torch.from_numpy(x.copy())
  assert np.array_equal(bf, t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
  assert np.array_equal(f16, t.to(torch.float16).view(torch.int16).numpy().view(np.uint16))
  nan = np.array([np.nan, -np.nan], np.float32)
  out = np.frombuffer(_run(driver, 'round', struct.pack('<i', 2) + nan.tobytes()), np.uint16)
  assert torch.from_numpy(out[:2].view(np.int16).copy()).view(torch.bfloat16).isnan().all() and torch.from_numpy(out[2:].view(np.int16).copy()).view(torch.float16).isnan().all()


def test_slot_rule_pads_past_the_count_past_the_clip_and_bad_indices(driver):
  n_tracks, count, clip_T = 10, 6, 4
  index = np.array([3, -1, 9, n_tracks, 0, 2**31 - 1], np.int32)  # exactly `count` entries: a slot past the count must not be looked up
  probes = np.array([[0, 0], [0, 3], [0, 4], [0, 11], [1, 0], [2, 3], [3, 0], [4, 2], [5, 0], [6, 0], [7, 1], [-1, 0], [2, -1], [1000000, 0]], np.int32)
  blob = struct.pack('<5i', n_tracks, count, clip_T, len(index), len(probes)) + index.tobytes() + probes.tobytes()
  got = np.frombuffer(_run(driver, 'slot', blob), np.int32).reshape(-1, 2)
  #                    live    live   frame = clip T   beyond    index -1  live   index = n_tracks  live    huge     slot = count  beyond   slot < 0  t < 0   far
  want = np.array([[3, 3], [3, 3], [3, -1], [3, -1], [-1, -1], [9, 9], [-1, -1], [0, 0], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [9, -1], [-1, -1]], np.int32)
  assert np.array_equal(got, want)
