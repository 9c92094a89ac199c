"""Track overlays on the GPU (include/spa3d.h: spa3d_render_tracks; spa3d.render_tracks, project_tracks, visualize_npz).  Every comparison is
torch.equal on uint8 / int32 against the NumPy restatement of the contract (tests/render_util.py); projection and colours are also compared
with what the reference's own functions gave (tests/golden/visualize_golden.npz -- the fixture travels, the reference does not).

  1. The 37 x 53, T = 7, N = 40 scene (neither side a multiple of the 64 x 16 tile or of the 4-pixel packing; tracks crossing tile borders, one
     jumping across the image in a frame), trail 5 / radius 2 and trail 0 / radius 0; in place; two runs; a frame no point touches.
  2. Ordering across compaction chunks: 3 x RENDER_CHUNK + 5 points inside one tile, distinct colours.
  3. The golden scene through project_tracks and render_tracks(coords = 3); the golden colour list through full-coverage dot centres.
  4. Score handling, use_visibility, colour_bgr, float [T, 3, H, W] input, a wide image (several tile columns, aligned dword path).
  5. The real use: model.score(frame_errors, return_predictions) -> render; save_scores_npz -> visualize_npz gives the same bytes."""
import os
import re

import numpy as np
import pytest
import torch

import render_util as RU
from util import MINI, O, batch_to, product_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = int(re.search(r'constexpr int RENDER_CHUNK = (\d+);', open(os.path.join(ROOT, '3dspa_code_amd', 'csrc', 'common.hpp')).read()).group(1))


def cu(a, dtype=None):
  return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


@pytest.fixture(scope='module')
def golden():
  return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'visualize_golden.npz')))


@pytest.fixture(scope='module')
def scene():
  """The scene and its references, computed once: {(trail, radius): painted video}."""
  video, tracks, scores, visible = RU.scene()
  pos = RU.pixels_2d(tracks)
  refs = {(tr, r): RU.render(video, pos, scores, trail=tr, point_size=r) for tr, r in ((5, 2), (0, 0))}
  return dict(video=video, tracks=tracks, scores=scores, visible=visible, pos=pos, refs=refs)


def gpu_render(spa3d, video, tracks, scores, visible=None, **kw):
  out = spa3d.render_tracks(cu(video), cu(tracks), cu(scores), None if visible is None else cu(visible), **kw)
  torch.cuda.synchronize()
  return out


def same(got, want):
  return torch.equal(got.cpu(), torch.as_tensor(np.ascontiguousarray(want)))


@pytest.mark.parametrize('trail,radius', [(5, 2), (0, 0)])
def test_scene_is_the_restatement(scene, trail, radius):
  import spa3d
  s = scene
  out, pixels = gpu_render(spa3d, s['video'], s['tracks'], s['scores'], trail=trail, point_size=radius, return_pixels=True)
  assert same(pixels, s['pos'])
  want = s['refs'][(trail, radius)]
  bad = (out.cpu().numpy() != want)
  assert not bad.any(), f'{int(bad.sum())} bytes differ, first at {np.argwhere(bad)[0].tolist()}'
  assert (want != s['video']).any()


def test_in_place_two_runs_and_an_untouched_frame(scene):
  import spa3d
  s = scene
  video, tracks = cu(s['video']), cu(s['tracks'])
  scores = s['scores'].copy()
  scores[:, 3] = np.nan   # nothing is drawn in frame 3: it stays byte-identical
  sc = cu(scores)
  a = spa3d.render_tracks(video, tracks, sc)
  b = spa3d.render_tracks(video, tracks, sc)
  assert torch.equal(a, b) and torch.equal(video.cpu(), torch.as_tensor(s['video']))   # two runs; the input is not written
  assert torch.equal(a[3], video[3]) and not torch.equal(a[2], video[2])
  assert same(a, RU.render(s['video'], s['pos'], scores))
  inplace = video.clone()
  r = spa3d.render_tracks(inplace, tracks, sc, out=inplace)
  assert r is inplace and torch.equal(inplace, a)
  # a view that starts at an odd byte offset and an odd width: the unaligned path
  buf = torch.zeros(video.numel() + 1, dtype=torch.uint8, device='cuda')
  odd = buf[1:].view(video.shape)
  odd.copy_(video)
  spa3d.render_tracks(odd, tracks, sc, out=odd)
  assert torch.equal(odd, a)


def test_order_across_compaction_chunks():
  import spa3d
  N, T, S = 3 * CHUNK + 5, 2, 32
  rng = np.random.default_rng(7)
  video = rng.integers(0, 256, (T, S, S, 3), dtype=np.uint8)
  tracks = rng.uniform(3, 13, (N, T, 2)).astype(np.float32)   # all inside the tile [0, 64) x [0, 16): one workgroup sees every point
  tracks[:, 1] += rng.uniform(-2, 2, (N, 2)).astype(np.float32)
  scores = rng.permutation(N * T).reshape(N, T).astype(np.float32)   # distinct scores: distinct colours up to the 8-bit ramp
  out, pixels = gpu_render(spa3d, video, tracks, scores, trail=1, point_size=1, return_pixels=True)
  pos = RU.pixels_2d(tracks)
  assert same(pixels, pos)
  want = RU.render(video, pos, scores, trail=1, point_size=1)
  assert same(out, want)
  # the picture depends on the order: the same points in reverse index order paint something else
  rev = RU.render(video, pos[::-1], scores[::-1], trail=1, point_size=1)
  assert (rev != want).any()


def test_golden_projection_and_scene(golden):
  import spa3d
  g = golden
  H, W = (int(v) for v in g['hw'])
  for name in ('frames', 'single'):
    K, E, rs = cu(g['intrinsics_' + name]), cu(g['extrinsics_' + name]), tuple(int(v) for v in g['resize_' + name])
    px = spa3d.project_tracks(cu(g['tracks']), K, E, H, W, resize=rs)
    assert px.dtype == torch.int32 and same(px, g['pixels_' + name])   # the reference's int() of its own project_all_tracks
    out, px2 = spa3d.render_tracks(cu(g['video']), cu(g['tracks']), cu(g['scores']), intrinsics=K, extrinsics=E, resize=rs, return_pixels=True)
    assert torch.equal(px, px2)
    assert same(out, RU.render(g['video'], g['pixels_' + name], g['scores']))


def test_golden_colour_list(golden):
  """A radius-1 dot covers its centre pixel with all 16 samples, so that pixel IS the colour: the reference's score_to_color_bgr of
  -0.3, 0, 0.5, 1, 1.7 and every k / 510 with their fp32 neighbours."""
  import spa3d
  cs, want = golden['colour_scores'], golden['colour_bgr']
  n, S = cs.size, 120
  assert n <= (S // 3) ** 2
  idx = np.arange(n)
  xy = np.stack([1 + 3 * (idx % (S // 3)), 1 + 3 * (idx // (S // 3))], -1)
  out = gpu_render(spa3d, np.zeros((1, S, S, 3), np.uint8), xy.reshape(n, 1, 2).astype(np.float32), cs.reshape(n, 1), trail=0, point_size=1, normalize=False, colour_bgr=True)
  assert np.array_equal(out.cpu().numpy()[0][xy[:, 1], xy[:, 0]], want)


def test_scores_visibility_bgr_float_video(scene):
  import spa3d
  s = scene
  video, tracks, visible, pos = s['video'], s['tracks'], s['visible'], s['pos']
  const = np.full_like(s['scores'], 0.75)
  assert same(gpu_render(spa3d, video, tracks, const), RU.render(video, pos, const))                       # max == min: s - min
  weird = s['scores'].copy()
  weird[0, 1], weird[1, 2], weird[2, 0], weird[6] = np.nan, np.inf, -np.inf, np.nan
  for normalize in (True, False):
    assert same(gpu_render(spa3d, video, tracks, weird, normalize=normalize), RU.render(video, pos, weird, normalize=normalize))
  assert same(gpu_render(spa3d, video, tracks, np.full_like(const, np.nan)), video)
  vis = gpu_render(spa3d, video, tracks, s['scores'], visible, use_visibility=True)
  assert same(vis, RU.render(video, pos, s['scores'], visible, use_visibility=True)) and not same(vis, s['refs'][(5, 2)])
  assert same(gpu_render(spa3d, video, tracks, s['scores'], visible[..., None]), s['refs'][(5, 2)])         # ignored unless asked for; [N, T, 1]
  bgr = gpu_render(spa3d, video[..., ::-1], tracks, s['scores'], colour_bgr=True)
  assert same(bgr, s['refs'][(5, 2)][..., ::-1])
  f = np.random.default_rng(2).uniform(-0.2, 1.2, (video.shape[0], 3) + video.shape[1:3]).astype(np.float32)
  u8 = (np.clip(np.transpose(f, (0, 2, 3, 1)), 0, 1) * 255).astype(np.uint8)                              # prepare_video_for_visualization
  assert same(gpu_render(spa3d, f, tracks, s['scores']), RU.render(u8, pos, s['scores']))


@pytest.mark.parametrize('T,H,W,N,step', [(3, 21, 200, 12, None), (2, 35, 1300, 10, 600)])
def test_wide_image_many_tiles(T, H, W, N, step):
  """200 x 21: four tile columns with a tail, two tile rows with a tail, a width that is a multiple of 4 (the dword path) -- long segments
  that cross several tiles, radius 7.  1300 x 35: segments of 511 to 1290 px across twenty tile columns."""
  import spa3d
  rng = np.random.default_rng(9)
  video = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
  tracks = np.stack([rng.uniform(0, W, (N, T)), rng.uniform(0, H, (N, T))], -1).astype(np.float32)
  if step:
    tracks[:4, 0, 0] = (2, 3, 4, 5)
    tracks[:4, 1, 0] = tracks[:4, 0, 0] + (511, 512, 513, 1290)
  scores = rng.uniform(0, 1, (N, T)).astype(np.float32)
  out = gpu_render(spa3d, video, tracks, scores, trail=2, point_size=7)
  assert same(out, RU.render(video, RU.pixels_2d(tracks), scores, trail=2, point_size=7))


def test_refusals_on_the_device_side():
  import spa3d
  video, tracks, scores = torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(3, 2, 2), torch.zeros(3, 2)
  with pytest.raises(spa3d._lib.Spa3dError):
    spa3d.render_tracks(video, tracks.cuda(), scores.cuda())        # CPU video
  with pytest.raises(spa3d._lib.Spa3dError):
    spa3d.render_tracks(video.cuda(), tracks, scores.cuda())        # CPU tracks
  with pytest.raises(spa3d._lib.Spa3dError, match='trail'):
    spa3d.render_tracks(video.cuda(), tracks.cuda(), scores.cuda(), trail=33)


def test_score_then_render_and_the_npz_round_trip(tmp_path):
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
  direct, pixels = spa3d.render_tracks(video, xy, sc.frame_err[0], vis, return_pixels=True)
  torch.cuda.synchronize()
  assert direct.shape == (T, S, S, 3) and direct.dtype == torch.uint8
  u8 = (np.clip(np.transpose(video.cpu().numpy(), (0, 2, 3, 1)), 0, 1) * 255).astype(np.uint8)
  pos = RU.pixels_2d(xy.cpu().numpy())
  assert same(pixels, pos) and same(direct, RU.render(u8, pos, sc.frame_err[0].cpu().numpy())) and (direct.cpu().numpy() != u8).any()
  path = str(tmp_path / 'scores.npz')
  spa3d.save_scores_npz(path, xy, sc.frame_err[0], vis, video=video)
  assert torch.equal(spa3d.visualize_npz(path), direct)
