"""The two device steps score_video adds around score_all, each against what a caller would do by hand, on one GPU, in one process, timed with HIP
events in ALTERNATING order (a, b, a, b, ...), the first `--warmup` rounds dropped.

  build    a  build_windows   one spa3d.build_windows call: W windows cut out of the long clip's arrays in place
           b  build_batch_xW  W spa3d.build_batch calls on torch slices of the same clip (the per-track arrays of a slice are not contiguous:
                              build_batch copies them; the maps of a slice are views)
  stitch   a  stitch_windows  one spa3d.stitch_windows call: tracks, visibility logits, frame errors and the spread, un-permuted
           b  torch           the hat blend restated with torch slices (accumulate weight * value and weight per window, one division, one
                              index_copy for the permutation; no spread, no single-window copy rule -- so it is not bit-equal, the largest difference is printed)

The workload: the inference-size clip -- 64 x 64 = 4096 tracks, TL = 600 frames, a 518 x 518 video, DINOv2-base 37 x 37 x 768 maps, a depth map
per frame -- in windows of 150 frames at stride 75 (7 windows), bf16, depth features of width --depth-dim.  The inputs are on the device before
the clock starts.  The two builds are compared bit for bit once.  Prints one JSON line per kind (event ms: median / min / max; host wall ms) and
one summary line.  Nothing is gated.

  python tools/bench_score_video.py --reps 7"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--tracks', type=int, default=4096)
  ap.add_argument('--frames', type=int, default=600)
  ap.add_argument('--window', type=int, default=150)
  ap.add_argument('--stride', type=int, default=75)
  ap.add_argument('--depth-dim', type=int, default=1)
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=2)
  args = ap.parse_args()
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import numpy as np
  import torch
  import spa3d
  assert torch.cuda.is_available(), 'bench_score_video needs the GPU: there is no CPU fallback and a CPU time would say nothing'
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  n, TL, Tw, H, W, Hp, Wp, D, DD = args.tracks, args.frames, args.window, 518, 518, 37, 37, 768, args.depth_dim
  model = spa3d.TrackAutoEncoder3D(num_output_frames=Tw, dino_feature_dim=D, depth_feature_dim=DD, precision='bf16')
  gen = torch.Generator(device=dev).manual_seed(5)
  xy = torch.rand(n, TL, 2, generator=gen, device=dev) * torch.tensor([W + 20.0, H + 20.0], device=dev) - 10.0  # a few points outside the frame
  clip = {'tracks_2d': xy, 'visible': (torch.rand(n, TL, generator=gen, device=dev) < 0.8).float(), 'depth': torch.rand(TL, H, W, 1, generator=gen, device=dev) * 9 + 0.1,
          'dino_map': torch.randn(TL, Hp, Wp, D, generator=gen, device=dev), 'video_shape': (TL, H, W, 3)}
  starts = spa3d.window_starts(TL, Tw, args.stride)
  nw = len(starts)
  perm = np.random.default_rng(0).permutation(n)

  def by_slices():
    out = []
    for a in starts.tolist():
      b = min(a + Tw, TL)
      sl = {'tracks_2d': clip['tracks_2d'][:, a:b], 'visible': clip['visible'][:, a:b], 'depth': clip['depth'][a:b], 'dino_map': clip['dino_map'][a:b],
            'video_shape': (b - a, H, W, 3)}
      out.append(spa3d.build_batch([sl], model=model, splits=[(perm, [], [])]))
    return out

  keys = ('support_tracks', 'support_tracks_visible', 'boundary_frame', 'dino_features', 'depth_features')
  a, b = spa3d.build_windows(clip, model, stride=args.stride, order=perm), by_slices()
  bits = lambda t: t.view(torch.int16) if t.dtype == torch.bfloat16 else t
  equal = all(torch.equal(bits(a[k][w]), bits(b[w][k][0])) for k in keys for w in range(nw))
  del a, b
  # per-window results as score_all leaves them
  tracks = torch.randn(nw, n, Tw, 3, generator=gen, device=dev)
  vlog, ferr = torch.randn(nw, n, Tw, generator=gen, device=dev), torch.rand(nw, n, Tw, generator=gen, device=dev)
  perm_t = torch.as_tensor(perm, device=dev)
  lens = [min(Tw, TL - s) for s in starts.tolist()]
  hats = [torch.minimum(torch.arange(1, L + 1, device=dev), torch.arange(L, 0, -1, device=dev)).float() for L in lens]

  def torch_stitch():
    res = {}
    den = torch.zeros(TL, device=dev)
    for w, (s, L) in enumerate(zip(starts.tolist(), lens)):
      den[s:s + L] += hats[w]
    for name, src in (('tracks', tracks), ('visible_logits', vlog[..., None]), ('frame_err', ferr[..., None])):
      num = torch.zeros(n, TL, src.shape[-1], device=dev)
      for w, (s, L) in enumerate(zip(starts.tolist(), lens)):
        num[:, s:s + L] += hats[w][None, :, None] * src[w, :, :L]
      res[name] = torch.empty_like(num).index_copy_(0, perm_t, num / den[None, :, None])
    return res

  lib_stitch = lambda: spa3d.stitch_windows(starts, TL, tracks=tracks, visible_logits=vlog, frame_err=ferr, blend='hat', row_track=perm, spread=True)
  x, y = lib_stitch(), torch_stitch()
  diff = max(float((x[k] - y[k].reshape(x[k].shape)).abs().max()) for k in ('tracks', 'visible_logits', 'frame_err'))
  del x, y
  pairs = [('build', [('build_windows', lambda: spa3d.build_windows(clip, model, stride=args.stride, order=perm)), ('build_batch_xW', by_slices)]),
           ('stitch', [('stitch_windows', lib_stitch), ('torch', torch_stitch)])]
  med = {}
  for step, kinds in pairs:
    ms = {name: [] for name, _ in kinds}
    wall = {name: [] for name, _ in kinds}
    for i in range(args.warmup + args.reps):
      for name, fn in kinds:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        del out
        if i >= args.warmup:
          ms[name].append(e0.elapsed_time(e1))
          wall[name].append((t1 - t0) * 1e3)
    for name, _ in kinds:
      med[name] = statistics.median(ms[name])
      print(json.dumps({'tool': 'bench_score_video', 'step': step, 'kind': name, 'tracks': n, 'frames': TL, 'window': Tw, 'stride': args.stride, 'windows': nw, 'dino': [Hp, Wp, D],
                        'depth_dim': DD, 'precision': 'bf16', 'event_ms': [round(v, 3) for v in ms[name]], 'median_ms': round(med[name], 3), 'min_ms': round(min(ms[name]), 3),
                        'max_ms': round(max(ms[name]), 3), 'host_wall_median_ms': round(statistics.median(wall[name]), 3)}), flush=True)
  print(json.dumps({'tool': 'bench_score_video', 'summary': 'HIP-event time per long clip; ratios are by-hand route / library call', 'builds_bit_equal': bool(equal),
                    'build_batch_xW_over_build_windows': round(med['build_batch_xW'] / med['build_windows'], 3), 'torch_over_stitch_windows': round(med['torch'] / med['stitch_windows'], 3),
                    'stitch_max_abs_diff_vs_torch': diff}), flush=True)


if __name__ == '__main__':
  main()
