"""spa3d.render_tracks against a plain device copy of the same video, on one GPU, in one process.  The copy, out.copy_(video), reads and
writes every pixel once: the floor for any renderer that produces a new clip.  The two are timed in ALTERNATING order (render, copy, render,
copy, ...) with device events around `--inner` back-to-back renders or `--copy-inner` back-to-back copies (the copy is short: more of them
make a window worth timing), the first `--warmup` rounds dropped.  What the floor includes: the clip and its copy (2 x 118 MB at the default
size) fit the 256 MiB Infinity Cache together and `out` has just been written by the render, so the copy runs largely from cache; it is a
lower bound on the floor from HBM, and the ratio printed is an upper bound on the distance from it.

The clip: 150 frames of 512 x 512, uint8; N = 2048 and 512 tracks of pixel coordinates (coords = 2), trail 5, radius 2, in two layouts:
  scattered   random walks started anywhere in the image
  clustered   every track inside a 96 x 40 window: all N points land in a few 64 x 16 tiles, the worst case for the tile pass

Prints one JSON line per (layout, N) -- ms per call: median / min / max for both, and their ratio -- nothing is gated.

  python tools/bench_render.py --reps 9"""
import argparse
import json
import os
import statistics
import sys


def tracks_for(layout, N, T, H, W, gen, torch):
  if layout == 'scattered':
    start = torch.rand(N, 1, 2, generator=gen) * torch.tensor([W, H], dtype=torch.float32)
  else:
    start = torch.rand(N, 1, 2, generator=gen) * torch.tensor([96.0, 40.0]) + torch.tensor([200.0, 230.0])
  walk = torch.cumsum(torch.randn(N, T, 2, generator=gen) * (2.0 if layout == 'scattered' else 0.3), 1)
  return (start + walk).float()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--frames', type=int, default=150)
  ap.add_argument('--size', type=int, default=512)
  ap.add_argument('--trail', type=int, default=5)
  ap.add_argument('--radius', type=int, default=2)
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--inner', type=int, default=10)
  ap.add_argument('--copy-inner', type=int, default=200)
  args = ap.parse_args()
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import torch
  import spa3d
  assert torch.cuda.is_available(), 'bench_render needs the GPU: there is no CPU fallback and a CPU time would say nothing'
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  T, H, W = args.frames, args.size, args.size
  gen = torch.Generator().manual_seed(5)
  video = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, generator=gen).to(dev)
  out = torch.empty_like(video)

  def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
      fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner

  for layout in ('scattered', 'clustered'):
    for N in (2048, 512):
      tracks = tracks_for(layout, N, T, H, W, gen, torch).to(dev)
      scores = torch.rand(N, T, generator=gen).to(dev)
      kinds = [('render', lambda: spa3d.render_tracks(video, tracks, scores, trail=args.trail, point_size=args.radius, out=out)), ('copy', lambda: out.copy_(video))]
      ms = {name: [] for name, _ in kinds}
      for i in range(args.warmup + args.reps):
        for name, fn in kinds:
          t = timed(fn, args.inner if name == 'render' else args.copy_inner)
          if i >= args.warmup:
            ms[name].append(t)
      spa3d.render_tracks(video, tracks, scores, trail=args.trail, point_size=args.radius, out=out)
      torch.cuda.synchronize()
      changed = int((out != video).any(-1).sum())
      stat = lambda v: {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4)}
      print(json.dumps({'tool': 'bench_render', 'layout': layout, 'N': N, 'frames': T, 'H': H, 'W': W, 'trail': args.trail, 'radius': args.radius, 'inner': args.inner, 'copy_inner': args.copy_inner,
                        'video_MB': round(video.numel() / 1e6, 1), 'pixels_changed': changed, 'render': stat(ms['render']), 'copy': stat(ms['copy']),
                        'render_over_copy': round(statistics.median(ms['render']) / statistics.median(ms['copy']), 2)}), flush=True)


if __name__ == '__main__':
  main()
