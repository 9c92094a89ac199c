"""The TAPVid-3D metric call against the forward pass whose predictions it scores, on one GPU, in one process: the kinds are timed in
ALTERNATING order (a, b, c, d, a, b, c, d, ...), every repetition ending in a device synchronise, the first `--warmup` rounds dropped.

  a  forward          spa3d_forward (predictions written)
  b  median           spa3d_tapvid3d_from_preds on those predictions, scaling = median (ratio pass, radix select, rows, pool)
  c  per_trajectory   the same, scaling = per_trajectory (rows, pool)
  d  none             the same, scaling = none

The headline width: B = 1 clip, N = 2048 support tracks, Q = 512 queries, T = 150 frames (76 800 ratios in the median's set), DINO 768 +
depth 1, bf16; --queries 2048 --frames 300 is the cfg#5 width (614 400).  Prints one JSON line per kind (ms: median / min / max) and one
summary line: each metric call as a share of the forward pass.  Nothing is gated.

  python tools/bench_tapvid3d.py --reps 9"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=1)
  ap.add_argument('--tracks', type=int, default=2048)
  ap.add_argument('--queries', type=int, default=512)
  ap.add_argument('--frames', type=int, default=150)
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--warmup', type=int, default=2)
  args = ap.parse_args()
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import torch
  import bench  # synth_batch
  import spa3d
  assert torch.cuda.is_available(), 'bench_tapvid3d needs the GPU: there is no CPU fallback and a CPU time would say nothing'
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  B, N, Q, T = args.batch, args.tracks, args.queries, args.frames
  model = spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=768, depth_feature_dim=1, precision='bf16')
  batch = bench.synth_batch(B, N, Q, T, 768, 1, dev, seed=77, feat_dtype=torch.bfloat16)
  v = {'params': model.init(0, batch)['params']}
  noise = torch.rand(B, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(1)).to(dev)
  preds = model(v, batch, noise=noise)
  kinds = [('forward', lambda: model(v, batch, noise=noise))] + \
          [(s, (lambda s=s: spa3d.tapvid3d_predictions(preds, batch, scaling=s))) for s in ('median', 'per_trajectory', 'none')]
  ms = {name: [] for name, _ in kinds}
  for i in range(args.warmup + args.reps):
    for name, fn in kinds:
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      fn()
      torch.cuda.synchronize()
      if i >= args.warmup:
        ms[name].append((time.perf_counter() - t0) * 1e3)
  med = {name: statistics.median(ms[name]) for name, _ in kinds}
  for name, _ in kinds:
    print(json.dumps({'tool': 'bench_tapvid3d', 'kind': name, 'B': B, 'N': N, 'Q': Q, 'frames': T, 'median_set': Q * T, 'precision': 'bf16',
                      'ms': [round(x, 3) for x in ms[name]], 'median_ms': round(med[name], 3), 'min_ms': round(min(ms[name]), 3), 'max_ms': round(max(ms[name]), 3)}), flush=True)
  print(json.dumps({'tool': 'bench_tapvid3d', 'summary': 'metric call (host wall time, allocation of its results included) as a share of the forward pass',
                    'forward_median_ms': round(med['forward'], 3), **{f'{s}_share': round(med[s] / med['forward'], 5) for s in ('median', 'per_trajectory', 'none')}}), flush=True)


if __name__ == '__main__':
  main()
