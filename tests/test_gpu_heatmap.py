"""Dense score maps on the GPU (include/spa3d.h: spa3d_render_heatmap; spa3d.render_heatmap, visualize_npz(mode='heatmap')).  Every comparison
is exact against the NumPy restatement of the contract (tests/heatmap_util.py): torch.equal on uint8, and on the int32 view of the float outputs,
so that NaN positions count.

  1. The 37 x 53, T = 7, N = 40 scene of render_util (neither side a multiple of the 64 x 16 tile or of the 4-pixel packing) at radius 3 / power 2,
     radius 20 / power 1 (a point reaches three tile rows) and radius 64 / power 2 (every point reaches the whole image): map, weight, overlay;
     a frame whose values are all NaN; two runs; in place; a view at an odd byte offset.
  2. Order across compaction chunks: 3 x HM_CHUNK + 5 points inside one tile, values of random sign over 2^+-20 -- after showing on the CPU that
     the other order gives other bits.
  3. The rim: radius 5, offset (3, 4) has q = 1 and (4, 4) nothing; one point of value 2.0; two points with equal weights.
  4. Eligibility: out-of-bounds positions, NaN / inf / 2^31 coordinates, NaN and +-inf values, use_visibility on and off.
  5. coords == 3 with the cameras of tests/golden/visualize_golden.npz: the positions are those of project_tracks.
  6. Overlay options: normalize, value_range (lo == hi too), colour_bgr, alpha 0 and 1, a float [T, 3, H, W] video, a 20 x 200 image (several
     tile columns, the aligned store path, more points than one chunk).
  7. 64-bit den: 2000 points on one pixel at radius 64 / power 2.
  8. Memory safety: outputs and workspace in canary-guarded, NaN-poisoned allocations, a map that is not 16-byte aligned; refused calls write
     nothing.
  9. The real use: model.score(frame_errors, return_predictions) -> render_heatmap; save_scores_npz -> visualize_npz(mode='heatmap')."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import heatmap_util as HU
import parity_util as PU
import render_util as RU
from util import MINI, O, batch_to, product_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = int(re.search(r'constexpr int HM_CHUNK = (\d+);', open(os.path.join(ROOT, '3dspa_code_amd', 'csrc', 'heatmap.hip')).read()).group(1))
SETTINGS = [(3, 2), (20, 1), (64, 2)]


def cu(a, dtype=None):
  return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def bits(got, want):
  """a float32 device tensor against a float32 array, bit for bit"""
  return torch.equal(got.cpu().contiguous().view(torch.int32), torch.as_tensor(np.ascontiguousarray(want, np.float32)).view(torch.int32))


def same(got, want):
  return torch.equal(got.cpu(), torch.as_tensor(np.ascontiguousarray(want)))


def gpu_heatmap(spa3d, tracks, values, H=None, W=None, video=None, visible=None, alpha=2048, **kw):
  """(map, weight, overlay or None) of spa3d.render_heatmap; alpha in 4096ths, as the restatement takes it"""
  res = spa3d.render_heatmap(cu(tracks), cu(values), H, W, video=None if video is None else cu(video), visibs=None if visible is None else cu(visible),
                             alpha=alpha / 4096, return_weight=True, **kw)
  torch.cuda.synchronize()
  return (res[0], res[2], res[1]) if video is not None else (res[0], res[1], None)


def agree(spa3d, tracks, values, H, W, radius, power, video=None, visible=None, use_visibility=False, normalize=True, rng=None, alpha=2048, bgr=False, cam=None):
  """the call against the restatement: map, weight and (with a video) the overlay, bit for bit; returns the restatement's (map, weight, overlay, den)"""
  cam = cam or {}
  # the wrapper's rule: value_range when given, else the clip's own range (normalize) or (0, 1)
  want = HU.heatmap(tracks, values, H, W, radius, power, visible=visible, use_visibility=use_visibility, video=video, normalize=normalize and rng is None,
                    rng=rng if rng is not None else (0.0, 1.0), alpha=alpha, bgr=bgr, **cam)
  m, w, ov = gpu_heatmap(spa3d, tracks, values, H if video is None else None, W if video is None else None, video, visible, alpha, radius=radius, power=power,
                         use_visibility=use_visibility, normalize=normalize, value_range=rng, colour_bgr=bgr, **cam)
  assert m.dtype == torch.float32 and tuple(m.shape) == want[0].shape and tuple(w.shape) == want[1].shape
  bad = m.cpu().numpy().view(np.int32) != want[0].view(np.int32)
  assert not bad.any(), f'{int(bad.sum())} map values differ, first at {np.argwhere(bad)[0].tolist()}'
  assert bits(w, want[1])
  if video is not None:
    bad = ov.cpu().numpy() != want[2]
    assert not bad.any(), f'{int(bad.sum())} overlay bytes differ, first at {np.argwhere(bad)[0].tolist()}'
  return want


@pytest.fixture(scope='module')
def scene():
  video, tracks, values, visible = RU.scene()
  return dict(video=video, tracks=tracks, values=values, visible=visible, H=video.shape[1], W=video.shape[2])


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('radius,power', SETTINGS)
def test_scene_is_the_restatement(scene, radius, power):
  import spa3d
  s = scene
  m, w, ov, den = agree(spa3d, s['tracks'], s['values'], s['H'], s['W'], radius, power, video=s['video'])
  assert (den > 0).any() and (ov != s['video']).any()
  assert (den > 0).all() if radius == 64 else (den == 0).any() or radius == 20
  # without a video: the map alone, the same bits
  m2, w2, _ = gpu_heatmap(spa3d, s['tracks'], s['values'], s['H'], s['W'], radius=radius, power=power)
  assert bits(m2, m) and bits(w2, w)


def test_nan_frame_two_runs_in_place_and_an_odd_offset(scene):
  import spa3d
  s = scene
  values = s['values'].copy()
  values[:, 3] = np.nan   # no point contributes in frame 3
  for radius, power in SETTINGS:
    want = agree(spa3d, s['tracks'], values, s['H'], s['W'], radius, power, video=s['video'])
    assert np.isnan(want[0][3]).all() and np.array_equal(want[2][3], s['video'][3]) and not np.array_equal(want[2][2], s['video'][2])
  video, tracks, val = cu(s['video']), cu(s['tracks']), cu(values)
  a = spa3d.render_heatmap(tracks, val, video=video, radius=20, power=1, return_weight=True)
  b = spa3d.render_heatmap(tracks, val, video=video, radius=20, power=1, return_weight=True)
  assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))
  assert torch.equal(video.cpu(), torch.as_tensor(s['video']))                  # the input is not written
  assert bool(torch.isnan(a[0][3]).all()) and torch.equal(a[1][3], video[3]) and bool((a[2][3] == 0).all())
  inplace = video.clone()
  r = spa3d.render_heatmap(tracks, val, video=inplace, out=inplace, radius=20, power=1)
  assert r[1] is inplace and torch.equal(inplace, a[1]) and torch.equal(r[0].view(torch.int32), a[0].view(torch.int32))
  # a view that starts at an odd byte offset (and an odd width): the unaligned byte path
  buf = torch.zeros(video.numel() + 1, dtype=torch.uint8, device='cuda')
  odd = buf[1:].view(video.shape)
  odd.copy_(video)
  spa3d.render_heatmap(tracks, val, video=odd, out=odd, radius=20, power=1)
  assert torch.equal(odd, a[1])


# ---------------------------------------------------------------------------------------------- 2
def test_order_across_compaction_chunks():
  import spa3d
  N, T, H, W = 3 * CHUNK + 5, 2, 16, 64   # one tile: one workgroup sees every point of a frame, in four chunks
  rng = np.random.default_rng(7)
  tracks = np.stack([rng.uniform(0, W, (N, T)), rng.uniform(0, H, (N, T))], -1).astype(np.float32)
  values = (rng.choice([-1.0, 1.0], (N, T)) * 2.0 ** rng.uniform(-20, -8, (N, T))).astype(np.float32)
  # six pairs of magnitude 2^19 .. 2^20 that cancel exactly, the two of a pair on one pixel and in different chunks: what is left of the small
  # values after a large one has come and gone depends on when it came
  for a, b in ((0, CHUNK + 3), (5, 2 * CHUNK + 7), (CHUNK - 1, 3 * CHUNK + 4), (CHUNK, 2 * CHUNK), (7, 3 * CHUNK), (2 * CHUNK - 2, 3 * CHUNK + 1)):
    tracks[b] = tracks[a]
    values[a] = (rng.choice([-1.0, 1.0], T) * 2.0 ** rng.uniform(19, 20, T)).astype(np.float32)
    values[b] = -values[a]
  pos = HU.positions(tracks)
  ok = HU.contributes(pos, values, H, W)
  assert ok.all()
  fwd, den = HU.sums(pos, ok, values, H, W, 20, 2)
  rev, den2 = HU.sums(pos, ok, values, H, W, 20, 2, reverse=True)
  assert np.array_equal(den, den2)
  assert (HU.finish(fwd, den)[0].view(np.int32) != HU.finish(rev, den)[0].view(np.int32)).any(), 'the order does not show in this case: it proves nothing'
  agree(spa3d, tracks, values, H, W, 20, 2)


# ---------------------------------------------------------------------------------------------- 3
def test_the_rim_a_single_point_and_the_mean_of_two():
  import spa3d
  H = W = 15
  one = np.array([[[7.9, 7.2]]], np.float32)                    # truncates to (7, 7)
  for power in (1, 2):
    m, w, _ = gpu_heatmap(spa3d, one, np.array([[2.0]], np.float32), H, W, radius=5, power=power)
    m, w = m.cpu().numpy()[0], w.cpu().numpy()[0]
    assert w[7 + 4, 7 + 3] == 1 and w[7 - 3, 7 - 4] == 1 and w[7 + 4, 7 + 4] == 0 and w[7, 7] == 26 ** power and w[7, 7 + 5] == 1 and w[7, 7 + 6] == 0
    assert (w > 0).sum() == 81 and (m[w > 0] == 2.0).all() and (m[w == 0].view(np.int32) == 0x7fc00000).all()
    agree(spa3d, one, np.array([[2.0]], np.float32), H, W, 5, power)
  two = np.array([[[4.0, 7.0]], [[10.0, 7.0]]], np.float32)
  vals = np.array([[1.0], [4.0]], np.float32)
  m, w, _ = gpu_heatmap(spa3d, two, vals, H, W, radius=5, power=2)
  assert float(m[0, 7, 7]) == 2.5 and float(w[0, 7, 7]) == 2 * 17 ** 2 and float(m[0, 7, 4]) == 1.0 and float(m[0, 7, 10]) == 4.0
  agree(spa3d, two, vals, H, W, 5, 2)


# ---------------------------------------------------------------------------------------------- 4
def test_eligibility():
  import spa3d
  H, W, T = 12, 20, 3
  tracks = np.array([[(-0.5, -0.99), (3.9, 2.2), (6.5, 4.0)],          # -0.5 truncates to 0: in bounds
                     [(5.0, 6.0), (float(W), 6.0), (9.0, float(H))],    # x = W, y = H: out of bounds
                     [(2.0, 9.0), (np.inf, 9.0), (np.nan, 9.0)],
                     [(2.0 ** 31, 3.0), (12.0, 3.0), (13.0, -1.0)],
                     [(10.0, 10.0), (10.0, 10.0), (10.0, 10.0)],
                     [(-3.0e9, 5.0), (15.0, -2.0 ** 31), (17.0, 8.0)]], np.float32)
  values = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], [np.nan, np.inf, -np.inf], [13, 14, 15]], np.float32)
  visible = np.array([[1, 0, 1], [1, 1, 1], [0.5, 1, 1], [1, 0.51, 1], [1, 1, 1], [1, 1, 0]], np.float32)
  ok = HU.contributes(HU.positions(tracks), values, H, W)
  assert ok.tolist() == [[True, True, True], [True, False, False], [True, False, False], [False, True, False], [False, False, False], [False, False, True]]
  video = np.full((T, H, W, 3), 17, np.uint8)
  for radius, power in ((2, 2), (64, 1)):
    off = agree(spa3d, tracks, values, H, W, radius, power, video=video)
    if radius == 2:
      assert off[3][:, 10, 10].tolist() == [0, 0, 0]                                                # the point with non-finite values contributes nothing
    on = agree(spa3d, tracks, values, H, W, radius, power, video=video, visible=visible, use_visibility=True)
    ign = agree(spa3d, tracks, values, H, W, radius, power, video=video, visible=visible)          # ignored unless asked for
    assert HU.same_bits(ign[0], off[0]) and not HU.same_bits(on[1], off[1])


# ---------------------------------------------------------------------------------------------- 5
def test_projected_points_with_the_golden_cameras():
  import spa3d
  g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'visualize_golden.npz')))
  H, W = (int(v) for v in g['hw'])
  for name in ('frames', 'single'):
    K, E, rs = g['intrinsics_' + name], g['extrinsics_' + name], tuple(int(v) for v in g['resize_' + name])
    px = spa3d.project_tracks(cu(g['tracks']), cu(K), cu(E), H, W, resize=rs)
    assert same(px, HU.positions(g['tracks'], K, E, H, W, rs)) and same(px, g['pixels_' + name])
    want = agree(spa3d, g['tracks'], g['scores'], H, W, 6, 2, video=g['video'], cam=dict(intrinsics=K, extrinsics=E, resize=rs))
    # the same map from the projected pixels taken as 2-D coordinates
    m2, w2, _ = gpu_heatmap(spa3d, g['pixels_' + name].astype(np.float32), g['scores'], H, W, radius=6, power=2)
    assert bits(m2, want[0]) and bits(w2, want[1]) and (want[3] > 0).any()


# ---------------------------------------------------------------------------------------------- 6
def test_overlay_options(scene):
  import spa3d
  s = scene
  tracks, values, video, H, W = s['tracks'], s['values'], s['video'], s['H'], s['W']
  base = agree(spa3d, tracks, values, H, W, 6, 2, video=video)
  for kw in (dict(normalize=False), dict(rng=(0.5, 2.5)), dict(normalize=False, rng=(0.5, 2.5)), dict(rng=(1.0, 1.0)), dict(rng=(2.0, 1.0)), dict(bgr=True), dict(alpha=1),
             dict(alpha=4095)):
    got = agree(spa3d, tracks, values, H, W, 6, 2, video=video, **kw)
    assert HU.same_bits(got[0], base[0]) and not np.array_equal(got[2], base[2])
  assert np.array_equal(agree(spa3d, tracks, values, H, W, 6, 2, video=video, alpha=0)[2], video)             # alpha 0: the bytes stay
  pure = agree(spa3d, tracks, values, H, W, 6, 2, video=video, alpha=4096)                                    # alpha 4096: the pure colour
  lo, hi = HU.value_range(values)
  s1 = ((base[0].astype(np.float64) - lo) / (np.float64(hi) - lo)).astype(np.float32)
  t, y, x = (int(v) for v in np.argwhere(base[3] > 0)[0])
  b, g, r = RU.colour_bgr(s1[t, y, x])
  assert tuple(pure[2][t, y, x]) == (r, g, b)
  bgr = agree(spa3d, tracks, values, H, W, 6, 2, video=video[..., ::-1], bgr=True)
  assert np.array_equal(bgr[2][..., ::-1], base[2])
  weird = values.copy()
  weird[0, 1], weird[1, 2], weird[2, 0], weird[6] = np.nan, np.inf, -np.inf, np.nan
  agree(spa3d, tracks, weird, H, W, 6, 2, video=video)
  agree(spa3d, tracks, np.full_like(values, 0.75), H, W, 6, 2, video=video)                                   # max == min: s = m - lo
  f = np.random.default_rng(2).uniform(-0.2, 1.2, (video.shape[0], 3, H, W)).astype(np.float32)
  u8 = (np.clip(np.transpose(f, (0, 2, 3, 1)), 0, 1) * 255).astype(np.uint8)                                  # prepare_video_for_visualization
  _, _, ov = gpu_heatmap(spa3d, tracks, values, video=f, radius=6, power=2)
  assert same(ov, HU.heatmap(tracks, values, H, W, 6, 2, video=u8)[2])


def test_wide_image_many_tiles_aligned_stores():
  """200 x 20: four tile columns with a tail, two tile rows with a tail, a width that is a multiple of 4 (16-byte stores, dword pixels), more
  points than one chunk spread over all tiles, radius 9."""
  import spa3d
  T, H, W, N = 3, 20, 200, CHUNK + 37
  rng = np.random.default_rng(9)
  video = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
  tracks = np.stack([rng.uniform(-2, W + 2, (N, T)), rng.uniform(-2, H + 2, (N, T))], -1).astype(np.float32)
  values = rng.normal(0, 1, (N, T)).astype(np.float32)
  want = agree(spa3d, tracks, values, H, W, 9, 2, video=video)
  assert (want[3] > 0).all()
  agree(spa3d, tracks[:60], values[:60], H, W, 3, 1, video=video)   # sparse: tiles and pixels nothing reaches


# ---------------------------------------------------------------------------------------------- 7
def test_den_needs_64_bits():
  import spa3d
  N, S = 2000, 16
  tracks = np.full((N, 1, 2), 8.3, np.float32)
  values = np.random.default_rng(3).normal(0, 1, (N, 1)).astype(np.float32)
  want = agree(spa3d, tracks, values, S, S, 64, 2)
  den = want[3]
  assert int(den[0, 8, 8]) == N * 4097 ** 2 > 2 ** 32 and (den > 2 ** 32).all()
  exact = np.array([[float(np.float32(int(d))) for d in row] for row in den[0]])       # Python int -> one rounding to float32
  assert np.array_equal(want[1][0].astype(np.float64), exact) and (exact != den[0].astype(np.float64)).any()


# ---------------------------------------------------------------------------------------------- 8
def test_guarded_outputs_poisoned_workspace_and_refusals(scene):
  import spa3d
  lib = spa3d._lib.load()
  h = spa3d.model._render_handle()
  T, H, W, N = 2, 20, 200, 90
  rng = np.random.default_rng(11)
  video = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
  tracks = np.stack([rng.uniform(0, W, (N, T)), rng.uniform(0, H, (N, T))], -1).astype(np.float32)
  values = rng.normal(0, 1, (N, T)).astype(np.float32)
  want = HU.heatmap(tracks, values, H, W, 7, 2, video=video)
  d_tracks, d_values, d_video = cu(tracks), cu(values), cu(video)
  cap = int(lib.spa3d_heatmap_workspace_bytes(h, N, T))
  stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

  def fresh(shift):
    """guarded, NaN-filled map and weight (the map `shift` floats into its view: 16-byte aligned or not), a guarded overlay, a guarded NaN workspace"""
    mp = PU.guarded(1, T * H * W + shift, torch.float32, name='map')[0, shift:]
    wt = PU.guarded(T * H, W, torch.float32, name='weight')
    ov = PU.guarded(T * H, W * 3 // 2, torch.int16, name='overlay', fill=0)
    ws = PU.guarded(1, cap // 4, torch.float32, name='workspace')
    return mp, wt, ov, ws

  def call(mp, wt, ov, ws, **fields):
    m = spa3d._lib.Heatmap()
    m.N, m.T, m.H, m.W, m.coords = N, T, H, W, 2
    m.tracks, m.values, m.video = d_tracks.data_ptr(), d_values.data_ptr(), d_video.data_ptr()
    m.map, m.weight, m.out = mp.data_ptr(), wt.data_ptr(), ov.data_ptr()
    m.radius, m.power, m.normalize, m.alpha = 7, 2, 1, 2048
    for k, v in fields.items():
      setattr(m, k, v)
    rc = lib.spa3d_render_heatmap(h, C.byref(m), ws.data_ptr(), cap, stream)
    torch.cuda.synchronize()
    return rc

  for shift in (0, 1):
    mp, wt, ov, ws = fresh(shift)
    assert mp.data_ptr() % 16 == (4 * shift) % 16
    assert call(mp, wt, ov, ws) == 0, lib.spa3d_last_error(h)
    assert bits(mp.view(T, H, W), want[0]) and bits(wt.view(T, H, W), want[1]) and same(ov.contiguous().view(torch.uint8).view(T, H, W, 3), want[2])
    PU.check_guards()
  # refused calls write nothing: outputs and workspace keep their fill, the guards their canary
  mp, wt, ov, ws = fresh(0)
  for fields, word in ((dict(radius=0), b'radius'), (dict(radius=65), b'radius'), (dict(power=3), b'power'), (dict(alpha=4097), b'alpha'), (dict(coords=4), b'coords'),
                       (dict(use_visibility=1), b'visible'), (dict(video=None), b'video'), (dict(normalize=0, lo=float('nan')), b'finite'), (dict(H=16385), b'16384')):
    assert call(mp, wt, ov, ws, **fields) == 1 and word in lib.spa3d_last_error(h), fields
  assert bool(torch.isnan(mp).all()) and bool(torch.isnan(wt).all()) and bool((ov == 0).all()) and bool(torch.isnan(ws).all())
  PU.check_guards()


# ---------------------------------------------------------------------------------------------- 9
def test_score_then_heatmap_and_the_npz_round_trip(tmp_path):
  import spa3d
  cfg = O.Config(**MINI, use_dino=False, use_depth=False)
  model = product_model(spa3d, cfg, 'fp32')
  batch = batch_to(O.synthetic_batch(2, 12, 10, 8, seed=5), 'cuda')
  params = model.init(0, batch)['params']
  sc = model.score({'params': params}, batch, frame_errors=True, return_predictions=True)
  T, S = sc.frame_err.shape[-1], 64
  xy = sc.predictions.tracks[0, :, :, :2]                                       # [Q, T, 2]
  lo, hi = xy.amin(), xy.amax()
  xy = ((xy - lo) / (hi - lo) * (S - 1)).contiguous()                           # spread over the canvas
  video = torch.rand(T, 3, S, S, generator=torch.Generator().manual_seed(1)).cuda()
  vis = batch['query_tracks_visible'][0]
  hm, direct, weight = spa3d.render_heatmap(xy, sc.frame_err[0], video=video, visibs=vis, return_weight=True)
  torch.cuda.synchronize()
  assert hm.shape == (T, S, S) and hm.dtype == torch.float32 and direct.shape == (T, S, S, 3) and direct.dtype == torch.uint8
  u8 = (np.clip(np.transpose(video.cpu().numpy(), (0, 2, 3, 1)), 0, 1) * 255).astype(np.uint8)
  want = HU.heatmap(xy.cpu().numpy(), sc.frame_err[0].cpu().numpy(), S, S, 12, 2, video=u8)
  assert bits(hm, want[0]) and bits(weight, want[1]) and same(direct, want[2]) and (want[2] != u8).any()
  fin = torch.isfinite(hm)
  assert bool(fin.any()) and float(hm[fin].min()) >= float(sc.frame_err[0].min()) and float(hm[fin].max()) <= float(sc.frame_err[0].max())   # an average of the errors
  path = str(tmp_path / 'scores.npz')
  spa3d.save_scores_npz(path, xy, sc.frame_err[0], vis, video=video)
  assert torch.equal(spa3d.visualize_npz(path, mode='heatmap'), direct)
  assert torch.equal(spa3d.visualize_npz(path), spa3d.render_tracks(video, xy, sc.frame_err[0], vis))   # the default mode is unchanged
