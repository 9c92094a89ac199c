"""Per-track scores against the two calls they replace, on one GPU, in one process: four kinds timed in ALTERNATING order
(a, b, c, d, a, b, c, d, ...), every repetition ending in a device synchronise, the first `--warmup` rounds dropped.

  a  forward                 spa3d_forward (predictions written)
  b  forward + loss          spa3d_forward, then spa3d_loss on its predictions -- what a user had for a quality number
  c  score                   spa3d_score(out = NULL): K = 5 thresholds, query_stats + sample_stats, no prediction tensor written
  d  score + preds + frames  spa3d_score with predictions and frame_err

  --shape uniform   B = 8, N = 2048, Q = 2048, T = 150, DINO 768 + depth 1, bf16
  --shape ragged    the 32-clip ragged batch of tools/bench_ragged.py (n_b = q_b in [64, 1024], one ragged call per kind)

Prints one JSON line per kind (times in ms, median / min / max, spread = (max - min) / median) and one summary line: c against b, with the
run-to-run spread of b next to it.  c moves strictly fewer bytes than b, so it gets no margin beyond that spread.

  python tools/bench_score.py --shape uniform --reps 7"""
import argparse
import json
import os
import random
import statistics
import sys
import time


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shape', choices=('uniform', 'ragged'), required=True)
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--seed', type=int, default=0)
  args = ap.parse_args()
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import torch
  import bench  # synth_batch
  import spa3d
  assert torch.cuda.is_available(), 'bench_score needs the GPU: there is no CPU fallback and a CPU time would say nothing'
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  T = 150
  model = spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=768, depth_feature_dim=1, precision='bf16')
  if args.shape == 'uniform':
    B, N, Q = 8, 2048, 2048
    batch = bench.synth_batch(B, N, Q, T, 768, 1, dev, seed=77, feat_dtype=torch.bfloat16)
    live_q = B * Q
  else:
    rng = random.Random(args.seed)
    counts = [rng.randint(64, 1024) for _ in range(32)]
    B, N, Q = 32, 1024, 1024
    batch = bench.synth_batch(B, N, Q, T, 768, 1, dev, seed=77, feat_dtype=torch.bfloat16)
    for b, n in enumerate(counts):
      for k in ('support_tracks', 'support_tracks_visible', 'dino_features', 'depth_features', 'query_points', 'query_tracks', 'query_tracks_visible'):
        batch[k][b, n:] = 0
    batch['support_count'] = torch.tensor(counts, dtype=torch.int32)
    batch['query_count'] = torch.tensor(counts, dtype=torch.int32)
    live_q = sum(counts)
  params = model.init(0, batch)['params']
  v = {'params': params}
  noise = torch.rand(B, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(1)).to(dev)
  thr = (0.02, 0.05, 0.1, 0.2, 0.4)
  targets = {k: batch[k] for k in ('query_tracks', 'query_tracks_visible', 'query_count') if k in batch}

  def fwd_loss():
    return spa3d.compute_loss_3d(model(v, batch, noise=noise), targets)

  kinds = (('forward', lambda: model(v, batch, noise=noise)),
           ('forward+loss', fwd_loss),
           ('score', lambda: model.score(v, batch, thresholds=thr, noise=noise)),
           ('score+preds+frames', lambda: model.score(v, batch, thresholds=thr, return_predictions=True, frame_errors=True, noise=noise)))
  ms = {name: [] for name, _ in kinds}
  for i in range(args.warmup + args.reps):
    for name, fn in kinds:
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      fn()
      torch.cuda.synchronize()
      if i >= args.warmup:
        ms[name].append((time.perf_counter() - t0) * 1e3)
  med = {}
  for name, _ in kinds:
    m = statistics.median(ms[name])
    med[name] = m
    print(json.dumps({'tool': 'bench_score', 'shape': args.shape, 'kind': name, 'B': B, 'N': N, 'Q': Q, 'frames': T, 'live_queries': live_q, 'precision': 'bf16',
                      'thresholds': len(thr), 'ms': [round(x, 2) for x in ms[name]], 'median_ms': round(m, 2), 'min_ms': round(min(ms[name]), 2),
                      'max_ms': round(max(ms[name]), 2), 'spread': round((max(ms[name]) - min(ms[name])) / m, 4)}), flush=True)
  pair = ms['forward+loss']
  print(json.dumps({'tool': 'bench_score', 'shape': args.shape, 'summary': 'score (out = NULL) against forward + loss', 'score_median_ms': round(med['score'], 2),
                    'pair_median_ms': round(med['forward+loss'], 2), 'score_over_pair': round(med['score'] / med['forward+loss'], 4),
                    'pair_spread': round((max(pair) - min(pair)) / med['forward+loss'], 4), 'score_wins': med['score'] <= med['forward+loss']}), flush=True)


if __name__ == '__main__':
  main()
