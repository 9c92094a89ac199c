"""Host side of the long-clip path, no GPU: the window plan (spa3d.window_starts), the blend arithmetic of csrc/window_row.hpp built with the host
compiler and compared BIT FOR BIT with the NumPy restatement (tests/windows_util.py), and every ValueError of build_windows, stitch_windows and
score_video, raised before any device call (there is no device here)."""
import struct
import subprocess

import numpy as np
import pytest
import torch

import spa3d
import windows_util as WU
from util import host_check_driver


# ---------------------------------------------------------------------------------------------- the plan
def test_window_starts_properties_over_a_grid():
  for window in range(1, 20):
    for stride in range(1, window + 1):
      for num_frames in range(1, 90):
        s = spa3d.window_starts(num_frames, window, stride)
        assert s.dtype == np.int32 and np.array_equal(s, WU.window_starts(num_frames, window, stride)), (num_frames, window, stride)
        if num_frames <= window:
          assert s.tolist() == [0]
          continue
        assert len(s) == 1 + -(-(num_frames - window) // stride)
        assert s[0] == 0 and (np.diff(s) > 0).all()                       # strictly increasing
        assert s[:-1].tolist() == [w * stride for w in range(len(s) - 1)]
        assert s[-1] == num_frames - window                               # the last window is flush with the end
        cov = WU.coverage(s, WU.window_lengths(s, window, num_frames), num_frames)
        assert cov.min() >= 1 and cov.max() <= -(-window // stride) + 1, (num_frames, window, stride, cov.max())


def test_window_starts_default_stride_and_refusals():
  assert spa3d.window_starts(600, 150).tolist() == [0, 75, 150, 225, 300, 375, 450]
  assert spa3d.window_starts(20, 8, 8).tolist() == [0, 8, 12] and spa3d.window_starts(20, 8, 4).tolist() == [0, 4, 8, 12]
  assert spa3d.window_starts(5, 8).tolist() == [0] and spa3d.window_starts(3, 1).tolist() == [0, 1, 2]
  for bad in (0, -1, 9):
    with pytest.raises(ValueError, match='stride'):
      spa3d.window_starts(20, 8, bad)
  for args in ((0, 8), (20, 0), (20.0, 8), (20, 8, 2.0), (True, 8)):
    with pytest.raises(ValueError):
      spa3d.window_starts(*args)


# ---------------------------------------------------------------------------------------------- the header against the restatement
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
  return host_check_driver(tmp_path_factory, 'window_row')


def _run(driver, cases):
  blob = [struct.pack('<i', len(cases))]
  for src, t0, ln, TL, blend in cases:
    W, N, Tw, NC = src.shape
    blob += [struct.pack('<7i', W, N, Tw, TL, NC, blend, int(ln is not None)), np.asarray(t0, np.int32).tobytes()]
    if ln is not None:
      blob.append(np.asarray(ln, np.int32).tobytes())
    blob.append(np.ascontiguousarray(src, np.float32).tobytes())
  out = subprocess.run([driver], input=b''.join(blob), capture_output=True, timeout=120)
  assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
  res, pos = [], 0
  for src, t0, ln, TL, blend in cases:
    W, N, Tw, NC = src.shape
    status, where = struct.unpack_from('<2i', out.stdout, pos)
    pos += 8
    if status != 0:
      res.append((status, where))
      continue
    o = np.frombuffer(out.stdout, np.float32, N * TL * NC, pos).reshape(N, TL, NC)
    pos += o.nbytes
    s2 = np.frombuffer(out.stdout, np.float32, N * TL, pos).reshape(N, TL)
    pos += s2.nbytes
    cnt = np.frombuffer(out.stdout, np.int32, N * TL, pos).reshape(N, TL)
    pos += cnt.nbytes
    res.append((o, s2, cnt))
  assert pos == len(out.stdout)
  return res


#        Tw, TL, t0, len (None = min(Tw, TL - t0))
PLANS = [(8, 20, [0, 4, 8, 12], None),                 # stride 4: frames under 1, 2 windows
         (8, 20, [0, 8, 12], None),                    # stride 8, the last window moved back
         (8, 14, list(range(7)), None),                # stride 1: up to 7 windows per frame
         (8, 12, [0, 3, 6], [8, 8, 6]),                # frames under 1, 2 and 3 windows; 6 + 6 = TL
         (8, 5, [0], None),                            # one short window
         (8, 11, [0, 4, 9], [5, 6, 2]),                # len < Tw everywhere, a short last window
         (150, 400, [0, 75, 150, 225, 250], None),     # more than one 64-frame chunk
         (3, 70, list(range(0, 68, 1)), None)]         # many windows, chunk borders inside windows


@pytest.mark.parametrize('blend', ['mean', 'hat', 'first'])
def test_header_matches_the_restatement_bit_for_bit(driver, blend):
  rng = np.random.default_rng(WU.BLEND[blend])
  cases = []
  for Tw, TL, t0, ln in PLANS:
    for NC in (1, 2, 3):
      W, N = len(t0), 3
      src = (rng.standard_normal((W, N, Tw, NC)) * 10.0 ** rng.integers(-3, 4, (W, N, 1, 1))).astype(np.float32)
      src[0, 0, 0] = -0.0   # the sign of zero survives a copy
      cases.append((src, t0, ln, TL, WU.BLEND[blend]))
  for (src, t0, ln, TL, b), (out, s2, cnt) in zip(cases, _run(driver, cases)):
    ln = WU.window_lengths(t0, src.shape[2], TL) if ln is None else ln
    want, want_s2 = WU.stitch(src, t0, ln, TL, b, want_spread=True)
    assert np.array_equal(cnt, np.broadcast_to(WU.coverage(t0, ln, TL), cnt.shape))
    assert np.array_equal(out.view(np.int32), want.view(np.int32)), (t0, TL, src.shape)
    assert np.array_equal(s2.view(np.int32), want_s2.view(np.int32)), (t0, TL, src.shape)
    one = WU.coverage(t0, ln, TL) == 1
    assert not s2[:, one].any() and (len(t0) == 1 or s2[:, ~one].any())
    assert np.signbit(out[0, 0]).all()


def test_weights_and_single_window_copy(driver):
  # one frame under three windows with hand-computed weights: window-relative frames 6, 3, 0 of 8-frame windows -> hat weights 2, 4, 1
  src = np.zeros((3, 1, 8, 1), np.float32)
  vals = np.array([0.1, 0.7, 0.3], np.float32)
  src[0, 0, 6, 0], src[1, 0, 3, 0], src[2, 0, 0, 0] = vals
  (hat, _, cnt), (mean, _, _), (first, _, _) = _run(driver, [(src, [0, 3, 6], [8, 8, 6], 12, b) for b in (WU.HAT, WU.MEAN, WU.FIRST)])
  assert cnt[0, 6] == 3
  w = np.array([2, 4, 1], np.float32)
  num = w[0] * vals[0]
  num = num + w[1] * vals[1]
  num = num + w[2] * vals[2]
  assert hat[0, 6, 0] == np.float32(num) / np.float32(7) and mean[0, 6, 0] == ((vals[0] + vals[1]) + vals[2]) / np.float32(3) and first[0, 6, 0] == vals[0]
  # 3 * v / 3 is not v for this v: a frame under one window must be a copy, whatever its weight
  v = next(x for x in (np.float32(k) / np.float32(7) for k in range(1, 99)) if (np.float32(3) * x) / np.float32(3) != x)
  src = np.full((2, 1, 8, 1), v, np.float32)
  (out, s2, cnt), = _run(driver, [(src, [0, 6], None, 14, WU.HAT)])
  assert cnt[0].tolist() == [1] * 6 + [2] * 2 + [1] * 6 and (out[0, cnt[0] == 1, 0] == v).all() and WU.weights(WU.HAT, 8)[2] == 3


def test_nan_stays_where_its_window_contributes(driver):
  rng = np.random.default_rng(5)
  src = rng.standard_normal((4, 2, 8, 3)).astype(np.float32)
  src[1, 0] = np.nan                                     # window 1 (frames 4..11), row 0
  frames = np.arange(20)
  for b in (WU.MEAN, WU.HAT, WU.FIRST):
    (out, s2, _), = _run(driver, [(src, [0, 4, 8, 12], None, 20, b)])
    # mean, hat: every frame window 1 contributes to.  first: frames 4..7 come from window 0, frames 8..11 from window 1.
    want = (frames >= (8 if b == WU.FIRST else 4)) & (frames < 12)
    assert np.array_equal(np.isnan(out[0]).all(-1), want) and np.array_equal(np.isnan(out[0]).any(-1), want) and not np.isnan(out[1]).any()
    # the spread of frames 4..11 has window 1's distance in it under every blend
    assert np.array_equal(np.isnan(s2[0]), (frames >= 4) & (frames < 12)) and not np.isnan(s2[1]).any()


def test_bad_plans_are_named(driver):
  src = np.zeros((3, 1, 8, 1), np.float32)
  res = _run(driver, [(src, [0, 4, 20], None, 20, 0), (src, [0, 4, 4], None, 20, 0), (src, [0, 4, 8], [8, 9, 8], 20, 0), (src, [0, 4, 8], [8, 8, 0], 20, 0),
                      (src, [0, 9, 12], None, 20, 0), (src, [0, 4, 8], None, 20, 0), (src, [1, 4, 12], None, 20, 0), (src, [0, 8, 12], [8, 8, 9], 20, 0)])
  assert res == [(1, 2), (2, 2), (3, 1), (3, 2), (4, 1), (4, 3), (4, 0), (3, 2)]


# ---------------------------------------------------------------------------------------------- Python refusals
N, T, TL, H, W_, D = 12, 6, 15, 20, 30, 8


def _model(**kw):
  return spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=D, depth_feature_dim=3, precision='bf16', **kw)


def _clip(**over):
  rng = np.random.default_rng(0)
  c = {'tracks_2d': rng.random((N, TL, 2)).astype(np.float32) * 10, 'visible': np.ones((N, TL), np.float32), 'depth': np.ones((TL, H, W_, 1), np.float32),
       'dino_map': rng.standard_normal((TL, 2, 3, D)).astype(np.float32), 'video_shape': (TL, H, W_, 3)}
  c.update(over)
  return {k: v for k, v in c.items() if v is not None}


def test_a_valid_build_windows_call_only_then_asks_for_the_device():
  with pytest.raises(spa3d._lib.Spa3dError, match='HIP-only'):
    spa3d.build_windows(_clip(), _model(), device='cpu')
  with pytest.raises(spa3d._lib.Spa3dError, match='HIP-only'):
    spa3d.build_windows(_clip(), _model(), starts=[0, 2, 9], order=np.arange(N)[::-1], queries=(np.array([1, 2]), np.zeros((3, 2), np.int64)), device='cpu')


def test_build_windows_refusals():
  def refused(match, clip=None, model=_model(), **kw):
    with pytest.raises(ValueError, match=match):
      spa3d.build_windows(_clip() if clip is None else clip, model, device='cpu', **kw)
  refused('needs the model', model=None)
  refused('2-D model', model=spa3d.TrackAutoEncoder(num_output_frames=T))
  refused('ONE clip', clip=[_clip()])
  refused('tracks_2d and visible', clip=_clip(visible=None))
  refused('depth to lift', clip=_clip(depth=None))
  refused('depth must be', clip=_clip(depth=np.ones((TL + 1, H, W_), np.float32)))
  refused('dino_map must be', clip=_clip(dino_map=np.zeros((TL - 1, 2, 3, D), np.float32)))
  refused('dino_feature_dim', clip=_clip(dino_map=np.zeros((TL, 2, 3, D + 4), np.float32)))
  refused('not both', starts=[0, 9], stride=3)
  refused('stride', stride=0)
  refused('stride', stride=T + 1)
  refused('starts', starts=[0, TL])
  refused('starts', starts=[-1, 3])
  refused('increase strictly', starts=[0, 5, 5])
  refused('at least one window', starts=[])
  refused('order', order=[0, N])
  refused('order', order=[[0, 1]])
  refused('at least one support', order=[])
  refused('queries is', queries=(np.array([1]),))
  refused('query_index', queries=(np.array([N]), np.zeros((3, 1), np.int64)))
  refused('query_frame must be', queries=(np.array([1]), np.zeros((2, 1), np.int64)))
  refused('query_frame has entries', queries=(np.array([1]), np.array([[0], [0], [0], [T]])))       # the default plan has 4 windows
  refused('query_frame has entries', starts=[0, 6, 12], queries=(np.array([1]), np.array([[0], [0], [3]])))   # the last window has 3 live frames


def test_stitch_windows_refusals():
  x = torch.zeros(4, 5, 8, 3)
  y = torch.zeros(4, 5, 8)
  ok = dict(starts=[0, 4, 8, 12], num_frames=20, tracks=x, visible_logits=y, frame_err=y[..., None])
  with pytest.raises(spa3d._lib.Spa3dError, match='HIP-only'):   # the positive control: a valid call is stopped by the device alone
    spa3d.stitch_windows(**ok, row_track=np.arange(5)[::-1].copy(), spread=True)

  def refused(match, **kw):
    with pytest.raises(ValueError, match=match):
      spa3d.stitch_windows(**dict(ok, **kw))
  refused('blend', blend='max')
  refused('needs tracks, visible_logits or frame_err', tracks=None, visible_logits=None, frame_err=None)
  refused('spread needs tracks', tracks=None, spread=True)
  refused('must be a tensor', frame_err=np.zeros((4, 5, 8), np.float32))
  refused('tracks must be', tracks=torch.zeros(4, 5, 8, 4))
  refused('visible_logits must be', visible_logits=torch.zeros(4, 5, 7))
  refused('num_frames', num_frames=0)
  refused('starts', starts=[0, 4, 8, 20])
  refused('increase strictly', starts=[0, 4, 4, 12])
  refused('4 windows', starts=[0, 4, 8])
  refused('gap', starts=[0, 4, 8, 11])                      # frame 19 is covered by none
  refused('gap', starts=[1, 4, 8, 12])
  refused('gap', starts=[0, 4, 8, 12], lengths=[3, 8, 8, 8])
  refused('lengths', lengths=[8, 8, 8, 9])
  refused('lengths', lengths=[8, 8, 8, 0])
  refused('lengths', lengths=[8, 8, 8])
  refused('runs past', starts=[0, 4, 8, 13], lengths=[8, 8, 8, 8])
  refused('permutation', row_track=[0, 1, 2, 3, 3])
  refused('permutation', row_track=[0, 1, 2, 3])
  refused('row_track', row_track=[0, 1, 2, 3, 5])
  with pytest.raises(ValueError, match=r'\[1, 256\]'):
    spa3d.stitch_windows(np.arange(257), 257 + 7, frame_err=torch.zeros(257, 1, 8))


def test_score_video_refusals():
  variables = {'params': {}}

  def refused(match, model=None, clip=None, **kw):
    with pytest.raises(ValueError, match=match):
      (model or _model()).score_video(variables, _clip() if clip is None else clip, **kw)
  refused('2-D model', model=spa3d.TrackAutoEncoder(num_output_frames=T))
  refused('decoder_scan_chunk_size', model=_model(decoder_scan_chunk_size=4))
  refused('decoder_scan_chunk_size', model=_model(track_chunk_size=4))
  refused('ragged', clip=dict(_clip(), support_count=[N]))
  refused('ONE clip', clip=[_clip()])
  refused('blend', blend='median')
  refused('thresholds', thresholds=(0.0,))
  refused('tracks_2d and visible', clip=_clip(tracks_2d=None))
  refused('stride', stride=T + 1)
  refused('folds', folds=1)
  refused('folds', folds=N + 1)
  refused('fold offsets', folds=np.array([0, 3, N + 1]))
  refused('permutation', perm=np.arange(N - 1))
  refused('permutation', perm=np.zeros(N, np.int64))
  refused('noise must be', noise=torch.zeros(2, 3, 4))
  refused('windows_per_call', windows_per_call=0)
  refused('256', stride=1, clip=_clip(tracks_2d=np.zeros((N, 300, 2), np.float32), visible=np.ones((N, 300), np.float32), depth=np.ones((300, 2, 2), np.float32),
                                      dino_map=None, video_shape=None))
