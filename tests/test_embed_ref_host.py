"""The references of tests/embed_util.py checked on the host, without a GPU: each against a second, independent statement of the same operation (the
oracle where it reaches, a brute-force loop where it does not), so that tests/test_gpu_embed.py compares the kernels with something that is itself
tested.  The last test makes every refusal call of the new entry points: they return before anything is launched."""
import math

import numpy as np
import torch

import embed_util as EU
import rows_util as RU
from util import O

f32 = np.float32


def _tracks(nrows, NC, seed):
  return (np.random.default_rng(seed).random((nrows, NC)) * 2 - 0.5).astype(f32)


def test_token_embedding_reference_is_the_oracles_sinusoidal_input():
  """embed_track_pos_visible up to its Dense: the 2-D model returns the embedding itself; the 3-D model is given an identity projection.  In float64 with a
  track scale of 1 the oracle takes the same float32 arguments and a float64 sine: equal to the last bit or two of the sine.  In float32 with a scale of 3
  it divides in float32 as the kernel does and takes a float32 sine: within the rounding of that sine"""
  for NC, nf, (B, N, T) in ((2, 32, (2, 3, 7)), (3, 32, (1, 2, 150)), (3, 5, (2, 2, 129)), (2, 12, (1, 1, 1)), (3, 64, (1, 3, 5))):
    tr = _tracks(B * N * T, NC, NC * 100 + nf)
    W = (NC + 1) * 2 * nf
    for scale, dt, tol in ((1.0, torch.float64, 4e-16), (3.0, torch.float32, 1.3e-7)):
      cfg = O.Config(num_frequencies=nf, track_scale_factor=scale, num_output_frames=T)
      t4 = torch.from_numpy(tr).reshape(B, N, T, NC).to(dt)
      vis = torch.ones(B, N, T, 1, dtype=dt)
      if NC == 2:
        want = O.TrackAutoEncoder2D(cfg).embed_track_pos_visible(None, t4, vis)
      else:
        p = {'track_token_projection': {'kernel': torch.eye(W, dtype=dt), 'bias': torch.zeros(W, dtype=dt)}}
        want = O.TrackAutoEncoder3D(cfg).embed_track_pos_visible(p, t4, vis)
      got = EU.embed_tokens_ref(tr, T, nf, scale)
      assert got.shape == (B * N * T, W)
      assert float(np.abs(got - want.reshape(-1, W).double().numpy()).max()) <= tol, (NC, nf, T, scale)


def test_time_coordinate_and_zero_pattern():
  for T in (1, 7, 129, 150):
    tc = EU.time_coord(3 * T + 2, T)
    assert tc.dtype == f32
    for r in range(3 * T + 2):
      assert tc[r] == f32(f32(r % T) / f32(T))
    want = (torch.arange(T, dtype=torch.float32) / T).numpy()      # the oracle's fr_id
    assert np.array_equal(tc[T:2 * T], want) and np.array_equal(tc[:T], want)
  out = EU.embed_tokens_ref(np.zeros((4, 3), f32), 2, 8, 3.0)
  one = math.sin(float(EU.HALF_PI))
  row = out[0].reshape(4, 16)
  assert np.all(row[:, :8] == 0) and np.all(row[:, 8:] == one) and abs(one - 1.0) < 1e-14
  assert np.array_equal(out[0], out[2]) and not np.array_equal(out[0, 48:], out[1, 48:])   # rows 0 and 2 are t = 0, row 1 is t = 1 / 2
  assert float(EU.HALF_PI) == 1.57079637050628662109375
  # a NaN or an infinity poisons its own coordinate's columns and nothing else
  x = np.array([[0.25, np.nan, np.inf]], f32)
  nan = np.isnan(EU.sin_embed_ref(x, 5)).reshape(3, 10)
  assert not nan[0].any() and nan[1].all() and nan[2].all()


def test_query_reference_is_the_oracles_decoder_context():
  times = np.array([0.5, 1.5, 2.5, 3.5, -0.5, 2.4999998, 2.5000002, 149.0, 6.0, 0.0, 7.49, 148.5], f32)
  for NC, nf in ((3, 32), (2, 5)):
    for tscale, time_scale in ((1.0, 1.0), (1.0, 4.0), (1.0, 3.0), (3.0, 150.0)):
      rng = np.random.default_rng(7)
      qp = np.concatenate([times[:, None], (rng.random((len(times), NC)) * 2 - 0.5).astype(f32)], 1)
      sin, tfeat, qframe = EU.query_embed_ref(qp, nf, tscale, time_scale)
      cfg = O.Config(num_frequencies=nf, track_scale_factor=tscale, time_scale_factor=time_scale)
      m = (O.TrackAutoEncoder3D if NC == 3 else O.TrackAutoEncoder2D)(cfg)
      ctx = m.get_decoder_context({'query_points': torch.from_numpy(qp)[None], 'boundary_frame': torch.zeros(1, dtype=torch.int32)})
      assert np.array_equal(qframe, ctx.query_frame[0].numpy())
      assert float(np.abs(sin - ctx.decoder_query[0].double().numpy()).max()) <= 1.3e-7       # the oracle's float32 sine
      want = torch.floor(ctx.query_frame[..., None].to(torch.float32) / cfg.time_scale_factor)  # the tfeat line of decode
      assert np.array_equal(tfeat, want[0, :, 0].numpy())
  # half to even, not half away from zero; floor, not truncation; an exact quotient stays exact
  _, tfeat, qframe = EU.query_embed_ref(np.concatenate([times[:, None], np.zeros((len(times), 2), f32)], 1), 4, 1.0, 3.0)
  assert list(qframe[:9]) == [0, 2, 2, 4, 0, 2, 3, 149, 6] and list(tfeat[:9]) == [0, 0, 0, 1, 0, 0, 1, 49, 2]
  _, tfeat, qframe = EU.query_embed_ref(np.array([[-0.6, 0, 0], [-2.5, 0, 0], [-3.5, 0, 0]], f32), 4, 1.0, 4.0)
  assert list(qframe) == [-1, -2, -4] and list(tfeat) == [-1, -1, -1]


def test_map_reference_against_closed_forms_and_a_pruning_plan():
  for T, nseq in ((1, 5), (7, 3), (150, 2)):
    S = T + 1
    arow, crow, ro = EU.embed_maps_ref(None, nseq * S, S, T)
    j = np.arange(nseq * S)
    assert np.array_equal(ro, j % S == 0) and np.array_equal(crow, np.where(j % S == 0, -1, j))
    assert np.array_equal(arow, (j // S) * T + np.maximum(j % S - 1, 0))
    rng = np.random.default_rng(T)
    km = (rng.random((nseq, S)) < 0.5).astype(f32)
    km[:, 0] = 1.0
    km[nseq - 1, 1:] = 0.0                      # one sequence keeps its readout token and nothing else
    _, _, row_src, kept = RU.prune_plan_ref(km)
    arow, crow, ro = EU.embed_maps_ref(row_src, kept, S, T)
    assert int(ro.sum()) == nseq and ro[-1]
    vis_rows = np.nonzero(km[:, 1:].reshape(-1) != 0)[0]      # the kept frame tokens are the input rows with a visible frame, in order
    assert np.array_equal(arow[~ro], vis_rows) and np.array_equal(crow[~ro], np.nonzero(~ro)[0]) and np.all(crow[ro] == -1)
    assert np.array_equal(arow[ro], np.arange(nseq) * T)


def test_keymask_reference_against_the_oracle_and_the_special_values():
  rng = np.random.default_rng(3)
  for B, N, T in ((3, 1, 1), (3, 3, 7), (3, 10, 150), (2, 4, 9)):
    vis = (rng.random((B * N, T)) < 0.6).astype(f32)
    for boundary in ([0, T, T + 5][:B], [-1, T // 2, T][:B]):
      b = torch.tensor(boundary, dtype=torch.int32)
      v5 = torch.from_numpy(vis).reshape(B, N, T, 1)
      want = O.TrackAutoEncoder3D.key_mask(v5, b).reshape(B * N, T + 1).float().numpy()
      assert np.array_equal(EU.keymask_ref(vis, boundary, N, 1), want)
      want2 = ((torch.arange(T)[None, None, :] < b[:, None, None]) & (v5[..., 0] != 0)).reshape(B * N, T).float().numpy()   # the 2-D model's mask
      assert np.array_equal(EU.keymask_ref(vis, boundary, N, 0), want2)
  vis = np.array([[0.0, 1.0, -0.0, 0.5, -1.0, np.nan]], f32)
  assert list(EU.keymask_ref(vis, [6], 1, 0)[0]) == [0, 1, 0, 1, 1, 1]
  assert list(EU.keymask_ref(vis, [4], 1, 1)[0]) == [1, 0, 1, 0, 1, 0, 0]
  assert list(EU.keymask_ref(vis, [0], 1, 1)[0]) == [1, 0, 0, 0, 0, 0, 0] and list(EU.keymask_ref(vis, [-1], 1, 0)[0]) == [0] * 6
  two = EU.keymask_ref(np.ones((4, 3), f32), [1, 3], 2, 0)    # sequences 0, 1 belong to sample 0, sequences 2, 3 to sample 1
  assert two.tolist() == [[1, 0, 0], [1, 0, 0], [1, 1, 1], [1, 1, 1]]


def test_pack_and_sum3_references_against_loops():
  g = torch.Generator().manual_seed(0)
  for dt in (torch.bfloat16, torch.float16):
    src = torch.randn(5, 9, generator=g)
    n, t = EU.pack_ref(src, 6, dt)
    assert n.shape == (5, 6) and t.shape == (6, 5)
    for r in range(5):
      for c in range(6):
        assert float(n[r, c]) == float(src[r, c].to(dt)) == float(t[c, r])
  # torch's cast is round to nearest even: a value halfway between two neighbours goes to the even one
  assert float(torch.tensor(1.0 + 2.0 ** -8).to(torch.bfloat16)) == 1.0 and float(torch.tensor(1.0 + 3 * 2.0 ** -8).to(torch.bfloat16)) == 1.0 + 2.0 ** -6
  assert float(torch.tensor(1.0 + 2.0 ** -11).half()) == 1.0 and float(torch.tensor(1.0 + 3 * 2.0 ** -11).half()) == 1.0 + 2.0 ** -9
  assert math.isinf(float(torch.tensor(65520.0).half())) and float(torch.tensor(65519.0).half()) == 65504.0
  a, b, c = (np.random.default_rng(i).standard_normal(7).astype(f32) for i in range(3))
  s = EU.sum3_ref(a, b, c)
  assert all(s[i] == f32(f32(a[i] + b[i]) + c[i]) for i in range(7)) and s.dtype == f32
  assert np.array_equal(EU.sum3_ref(None, b, None), b) and np.array_equal(EU.sum3_ref(a, None, c), a + c)


def test_discretize_reference_against_scalar_arithmetic_and_the_oracle_in_float64():
  rng = np.random.default_rng(5)
  planted = EU.discretize_planted()
  lat = np.concatenate([planted, planted, planted, (rng.random(2000) * 3 - 1.5).astype(f32)])
  top = np.nextafter(f32(1), f32(0))
  noise = rng.random(len(lat)).astype(f32)
  noise[:len(planted)] = 0.0
  noise[len(planted):2 * len(planted)] = top
  for disc in (0, 1):
    out, mask = EU.discretize_ref(lat, noise, disc)
    for i in range(len(lat)):
      o, m = EU.discretize_scalar(lat[i], noise[i], disc)
      assert (o == out[i] or (o != o and out[i] != out[i])) and (m == mask[i] or (m != m and mask[i] != mask[i])), (disc, i, lat[i])
    nan = np.isnan(lat)
    assert np.array_equal(np.isnan(out), nan) and np.array_equal(np.isnan(mask), nan)
    want = EU.discretize_oracle64(lat, noise, disc)
    assert float(np.abs(out[~nan].astype(np.float64) - want[~nan]).max()) <= 2.0 ** -23
  # the edges: the mask is closed at +-1, ties go to the even multiple, and the result is q up to the rounding of l - (l - q)
  _, mask = EU.discretize_ref(np.array([1.0, -1.0, 1.0 + 2.0 ** -23, -1.0 - 2.0 ** -23, np.inf, 0.0, -0.0], f32), None, 0)
  assert mask.tolist() == [1, 1, 0, 0, 0, 1, 1]
  out, _ = EU.discretize_ref(np.array([0.5 / 128, 1.5 / 128, 2.5 / 128, -0.5 / 128, -1.5 / 128], f32), np.full(5, 0.5, f32), 1)
  assert np.allclose(out * 128, [0, 2, 2, 0, -2], atol=1e-4)


def test_every_refusal_is_decided_before_anything_is_launched():
  """the calls of embed_util.refusals with made-up addresses and no GPU: every one returns SPA3D_ERR_ARG, so none of them reads a pointer or reaches a
  launch.  Empty inputs return SPA3D_OK the same way"""
  import spa3d
  lib = spa3d._lib.load()
  base = 0x7f0000000000
  a, o, f, z = base + 0x10000, base + 0x20000, base + 0x30000, base + 0x40000
  bad, n = [], 0
  for dtype in (0, 1, 2):
    for name, rc in EU.refusals(lib, dtype, a, o, f, z, None):
      n += 1
      if rc != 1:
        bad.append(f'dtype {dtype} {name}: status {rc}')
  assert not bad, 'not refused: ' + '; '.join(bad)
  assert n > 240
  empty = []
  for dtype in (0, 1, 2):
    empty += [('sin_embed_scaled', lib.spa3d_op_sin_embed_scaled(a, 0, 3, 32, 1.0, o, dtype, None)),
              ('embed_tokens', lib.spa3d_op_embed_tokens(a, 0, 2, 3, 32, 1.0, o, dtype, None)),
              ('embed_maps', lib.spa3d_op_embed_maps(None, 0, 3, 2, z, z, o, a, 8, dtype, None)),
              ('set_readout_rows', lib.spa3d_op_set_readout_rows(o, a, 0, 3, 8, dtype, None)),
              ('pack rows = 0', lib.spa3d_op_pack(a, 8, 0, 8, o, 8, None, 0, dtype, None)),
              ('pack cols = 0', lib.spa3d_op_pack(a, 8, 4, 0, o, 8, o, 4, dtype, None)),
              ('transpose', lib.spa3d_op_transpose(o, 0, 8, o, dtype, None))]
  empty += [('query_embed', lib.spa3d_op_query_embed(a, 0, 3, 32, 1.0, 150.0, f, z, None)), ('keymask', lib.spa3d_op_keymask(a, z, 0, 3, 4, 1, f, None)),
            ('sum3', lib.spa3d_op_sum3(a, None, None, f, 0, None)), ('discretize', lib.spa3d_op_discretize(a, None, 0, f, None, 0, None))]
  assert all(rc == 0 for _, rc in empty), [e for e in empty if e[1] != 0]
