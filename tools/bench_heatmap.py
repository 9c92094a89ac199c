"""spa3d.render_heatmap at inference size, on one GPU, in one process, against the two things it can be held to:

  stamp   the torch route: every point-frame's (2 radius + 1)^2 stamp scattered into fp32 num / den planes with index_add_ (float atomics), a
          chunk of frames at a time (all 150 frames at once would need 0.67 G indices), then num / den.  Not the same arithmetic -- fp32 sums
          in arrival order -- so it is also run twice and the map values that differ between its own two runs are counted.
  copy    out.copy_(src) of a float32 [T, H, W] tensor: reads and writes one map once, the floor for anything that produces one.

The kinds are timed in ALTERNATING order (map, map + overlay, stamp, copy, map, ...) with device events around `inner` back-to-back calls of
each, the first `--warmup` rounds dropped.  Prints one JSON line: ms per call, median / min / max of `--reps` rounds -- nothing is gated.

  python tools/bench_heatmap.py --reps 7"""
import argparse
import json
import os
import statistics
import sys


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--tracks', type=int, default=4096)
  ap.add_argument('--frames', type=int, default=150)
  ap.add_argument('--size', type=int, default=518)
  ap.add_argument('--radius', type=int, default=16)
  ap.add_argument('--power', type=int, default=2)
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--inner', type=int, default=5)
  ap.add_argument('--copy-inner', type=int, default=50)
  ap.add_argument('--stamp-frames', type=int, default=10, help='frames per index_add_ of the stamp route')
  args = ap.parse_args()
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import torch
  import spa3d
  assert torch.cuda.is_available(), 'bench_heatmap needs the GPU: there is no CPU fallback and a CPU time would say nothing'
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  N, T, H, W, R, P = args.tracks, args.frames, args.size, args.size, args.radius, args.power
  gen = torch.Generator().manual_seed(5)
  start = torch.rand(N, 1, 2, generator=gen) * torch.tensor([W, H], dtype=torch.float32)
  tracks = (start + torch.cumsum(torch.randn(N, T, 2, generator=gen) * 2.0, 1)).float().to(dev)
  values = torch.rand(N, T, generator=gen).to(dev)
  video = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, generator=gen).to(dev)
  out = torch.empty_like(video)
  src, dst = torch.rand(T, H, W, generator=gen).to(dev), torch.empty(T, H, W, device=dev)

  d = torch.arange(-R, R + 1, device=dev)
  dy, dx = d.view(-1, 1).expand(2 * R + 1, 2 * R + 1).reshape(-1), d.view(1, -1).expand(2 * R + 1, 2 * R + 1).reshape(-1)
  q = (R * R + 1 - (dx * dx + dy * dy)).clamp(min=0).float()
  stamp_w = q * q if P == 2 else q                                   # 0 outside the disc

  def stamp():
    """the scatter route: [T, H, W] map"""
    num, den = torch.zeros(T * H * W, device=dev), torch.zeros(T * H * W, device=dev)
    pos = tracks.to(torch.int64)                                     # truncation, as the call does
    for t0 in range(0, T, args.stamp_frames):
      t1 = min(T, t0 + args.stamp_frames)
      x, y = pos[:, t0:t1, 0, None] + dx, pos[:, t0:t1, 1, None] + dy  # [N, t, S]
      ok = (pos[:, t0:t1, 0, None] >= 0) & (pos[:, t0:t1, 0, None] < W) & (pos[:, t0:t1, 1, None] >= 0) & (pos[:, t0:t1, 1, None] < H)
      ok = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H) & (stamp_w > 0)
      tt = torch.arange(t0, t1, device=dev).view(1, -1, 1)
      idx = ((tt * H + y) * W + x)[ok]
      w = stamp_w.expand_as(ok)[ok]
      den.index_add_(0, idx, w)
      num.index_add_(0, idx, w * values[:, t0:t1, None].expand_as(ok)[ok])
    return (num / den).view(T, H, W)                                  # 0 / 0 = NaN where nothing reaches

  def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
      fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner

  kinds = [('map', lambda: spa3d.render_heatmap(tracks, values, H, W, radius=R, power=P), args.inner),
           ('map_overlay', lambda: spa3d.render_heatmap(tracks, values, video=video, out=out, radius=R, power=P), args.inner),
           ('stamp', stamp, 1), ('copy', lambda: dst.copy_(src), args.copy_inner)]
  ms = {name: [] for name, _, _ in kinds}
  for i in range(args.warmup + args.reps):
    for name, fn, inner in kinds:
      t = timed(fn, inner)
      if i >= args.warmup:
        ms[name].append(t)
  a, b = stamp(), stamp()
  m1, m2 = spa3d.render_heatmap(tracks, values, H, W, radius=R, power=P), spa3d.render_heatmap(tracks, values, H, W, radius=R, power=P)
  torch.cuda.synchronize()
  ai, bi = a.view(torch.int32), b.view(torch.int32)
  fin = torch.isfinite(m1)
  stat = lambda v: {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4)}
  print(json.dumps({'tool': 'bench_heatmap', 'N': N, 'frames': T, 'H': H, 'W': W, 'radius': R, 'power': P, 'inner': args.inner, 'copy_inner': args.copy_inner,
                    'map_MB': round(src.numel() * 4 / 1e6, 1), 'video_MB': round(video.numel() / 1e6, 1), **{k: stat(v) for k, v in ms.items()},
                    'map_over_copy': round(statistics.median(ms['map']) / statistics.median(ms['copy']), 2),
                    'stamp_over_map': round(statistics.median(ms['stamp']) / statistics.median(ms['map']), 2),
                    'pixels_reached': int(fin.sum()), 'pixels': int(fin.numel()),
                    'stamp_values_differing_between_its_two_runs': int(((ai != bi) & ~(torch.isnan(a) & torch.isnan(b))).sum()),
                    'call_values_differing_between_its_two_runs': int((m1.view(torch.int32) != m2.view(torch.int32)).sum()),
                    'stamp_max_abs_diff_to_call': float((a - m1)[fin & torch.isfinite(a)].abs().max())}), flush=True)


if __name__ == '__main__':
  main()
