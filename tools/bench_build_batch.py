"""build_batch (one spa3d_build_batch call for all clips) against the same batch from the existing per-clip calls, on one GPU, in one process,
timed with HIP events in ALTERNATING order (a, b, c, a, b, c, ...), the first `--warmup` rounds dropped.

  a  build_batch     spa3d.build_batch(clips, splits=...): only the picked rows, written straight into the padded batch in bf16
  b  per_clip_bf16   per clip: lift_2d_to_3d, sample_dino_features_for_tracks(out_dtype=bf16) and sample_depth_features_for_tracks over ALL tracks,
                     then indexing, then collate_ragged -- the cheapest route the library had
  c  per_clip_f32    the same with the DINO sampler writing fp32 and a cast afterwards: inference.py's recipe as it stands

The workload: 8 clips of the inference.py shape -- 64 x 64 = 4096 tracks, T = 150, a 518 x 518 video, DINOv2-base 37 x 37 x 768 maps, a
depth map per frame -- 2048 support + 512 query tracks picked per clip, bf16, depth features of width --depth-dim.  The inputs are on the
device before the clock starts and the splits are the same for the three kinds; the results of a and b are compared bit for bit once.
Prints one JSON line per kind (event ms: median / min / max; host wall ms) and one summary line.  Nothing is gated.

  python tools/bench_build_batch.py --reps 7"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--clips', type=int, default=8)
  ap.add_argument('--tracks', type=int, default=4096)
  ap.add_argument('--frames', type=int, default=150)
  ap.add_argument('--support', type=int, default=2048)
  ap.add_argument('--queries', type=int, default=512)
  ap.add_argument('--depth-dim', type=int, default=1)
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=2)
  args = ap.parse_args()
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import numpy as np
  import torch
  import spa3d
  assert torch.cuda.is_available(), 'bench_build_batch needs the GPU: there is no CPU fallback and a CPU time would say nothing'
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  B, n, T, H, W, Hp, Wp, D, DD = args.clips, args.tracks, args.frames, 518, 518, 37, 37, 768, args.depth_dim
  model = spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=D, depth_feature_dim=DD, precision='bf16')
  gen = torch.Generator(device=dev).manual_seed(5)
  clips = []
  for _ in range(B):
    xy = torch.rand(n, T, 2, generator=gen, device=dev) * torch.tensor([W + 20.0, H + 20.0], device=dev) - 10.0  # a few points outside the frame
    clips.append({'tracks_2d': xy, 'visible': (torch.rand(n, T, generator=gen, device=dev) < 0.8).float(),
                  'depth': torch.rand(T, H, W, 1, generator=gen, device=dev) * 9 + 0.1, 'dino_map': torch.randn(T, Hp, Wp, D, generator=gen, device=dev),
                  'video_shape': (T, H, W, 3)})
  np.random.seed(0)
  splits = [spa3d.draw_split(n, args.support, args.queries, T) for _ in range(B)]
  dsplits = [tuple(torch.as_tensor(v).long().to(dev) for v in s) for s in splits]

  def per_clip(dino_dtype):
    samples = []
    for clip, (si, qi, qf) in zip(clips, dsplits):
      tr = clip['tracks_2d']
      t3 = spa3d.lift_2d_to_3d(tr, clip['depth'])
      dino = spa3d.sample_dino_features_for_tracks(clip['dino_map'], tr, clip['video_shape'], out_dtype=dino_dtype)
      depth = spa3d.sample_depth_features_for_tracks(clip['depth'], tr)
      vis = clip['visible'][..., None]
      samples.append({'support_tracks': t3[si], 'support_tracks_visible': vis[si], 'query_tracks': t3[qi], 'query_tracks_visible': vis[qi],
                      'query_points': torch.cat([qf.float()[:, None], t3[qi, qf]], 1), 'boundary_frame': torch.tensor(T),
                      'dino_features': dino[si].to(torch.bfloat16), 'depth_features': depth[si][..., :DD].to(torch.bfloat16)})
    return spa3d.collate_ragged(samples)

  kinds = [('build_batch', lambda: spa3d.build_batch(clips, model=model, splits=splits)), ('per_clip_bf16', lambda: per_clip(torch.bfloat16)),
           ('per_clip_f32', lambda: per_clip(torch.float32))]
  a, b = kinds[0][1](), kinds[1][1]()
  equal = sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.int16) if a[k].dtype == torch.bfloat16 else a[k],
                                                                                  b[k].view(torch.int16) if b[k].dtype == torch.bfloat16 else b[k]) for k in a)
  del a, b
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
  med = {name: statistics.median(ms[name]) for name, _ in kinds}
  for name, _ in kinds:
    print(json.dumps({'tool': 'bench_build_batch', 'kind': name, 'clips': B, 'tracks': n, 'frames': T, 'support': args.support, 'queries': args.queries, 'dino': [Hp, Wp, D],
                      'depth_dim': DD, 'precision': 'bf16', 'event_ms': [round(x, 3) for x in ms[name]], 'median_ms': round(med[name], 3), 'min_ms': round(min(ms[name]), 3),
                      'max_ms': round(max(ms[name]), 3), 'host_wall_median_ms': round(statistics.median(wall[name]), 3)}), flush=True)
  out_bytes = B * args.support * T * D * 2
  print(json.dumps({'tool': 'bench_build_batch', 'summary': 'HIP-event time of one batch of clips; ratios are per-clip route / build_batch', 'results_bit_equal': bool(equal),
                    'build_batch_median_ms': round(med['build_batch'], 3), 'per_clip_bf16_over_build_batch': round(med['per_clip_bf16'] / med['build_batch'], 3),
                    'per_clip_f32_over_build_batch': round(med['per_clip_f32'] / med['build_batch'], 3),
                    'dino_plane_GB': round(out_bytes / 1e9, 3), 'dino_plane_write_GBps': round(out_bytes / 1e6 / med['build_batch'], 1)}), flush=True)


if __name__ == '__main__':
  main()
