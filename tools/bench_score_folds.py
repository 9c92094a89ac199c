"""Scores for every track of a clip: one spa3d_score_folds call against the leave-out round it replaces, on one GPU, in one process.

  a  score_all          model.score_all(folds = F): the track encoder once over the clip's N tracks
  b  F x model.score    one model.score call per fold on a PRE-BUILT compacted batch (support = the other folds, queries = the fold): the
                        track encoder F times over N (1 - 1 / F) tracks.  Building those batches is not timed.

Workload: one clip of the inference.py shape -- N = 4096 tracks, T = 150, DINO 768 + depth 1, bf16, F = 8 (512 queries per fold), every track
queried at a random frame, frame errors on, no prediction tensor.  The two kinds are timed with HIP events in ALTERNATING order (a, b, a, b, ...;
every other round b first), the first `--warmup` rounds dropped.  Prints one JSON line per kind (ms: median / min / max, spread = (max - min) /
median), the largest difference between the two results (they are the same numbers up to the order of summation), and one summary line.

  python tools/bench_score_folds.py --reps 7"""
import argparse
import json
import os
import statistics
import sys


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--tracks', type=int, default=4096)
  ap.add_argument('--folds', type=int, default=8)
  ap.add_argument('--frames', type=int, default=150)
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=2)
  args = ap.parse_args()
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import torch
  import bench  # synth_batch
  import spa3d
  assert torch.cuda.is_available(), 'bench_score_folds needs the GPU: there is no CPU fallback and a CPU time would say nothing'
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  N, F, T = args.tracks, args.folds, args.frames
  model = spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=768, depth_feature_dim=1, precision='bf16')
  raw = bench.synth_batch(1, N, 1, T, 768, 1, dev, seed=77, feat_dtype=torch.bfloat16)
  support = ('support_tracks', 'support_tracks_visible', 'dino_features', 'depth_features')
  batch = {k: raw[k] for k in support + ('boundary_frame',)}
  qf = torch.randint(0, T, (1, N), generator=torch.Generator().manual_seed(5)).to(dev)
  pos = torch.gather(batch['support_tracks'], 2, qf[:, :, None, None].expand(1, N, 1, 3))[:, :, 0]
  batch['query_points'] = torch.cat([qf[..., None].float(), pos], dim=-1)
  off = [int(x) for x in spa3d.fold_offsets(N, F)]
  compacted = []
  for lo, hi in zip(off[:-1], off[1:]):
    c = {k: torch.cat([batch[k][0, :lo], batch[k][0, hi:]])[None].contiguous() for k in support}
    c['boundary_frame'] = batch['boundary_frame']
    c['query_points'] = batch['query_points'][:, lo:hi].contiguous()
    c['query_tracks'] = batch['support_tracks'][:, lo:hi].contiguous()
    c['query_tracks_visible'] = batch['support_tracks_visible'][:, lo:hi].contiguous()
    compacted.append(c)
  params = model.init(0, batch)['params']
  v = {'params': params}
  noise = torch.rand(1, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(1)).to(dev)

  def folds_call():
    return model.score_all(v, batch, folds=F, frame_errors=True, noise=noise).frame_err

  def round_by_hand():
    return torch.cat([model.score(v, c, frame_errors=True, noise=noise).frame_err for c in compacted], dim=1)

  kinds = (('score_all', folds_call), (f'{F} x model.score', round_by_hand))
  ms = {name: [] for name, _ in kinds}
  last = {}
  for i in range(args.warmup + args.reps):
    for name, fn in (kinds if i % 2 == 0 else kinds[::-1]):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      torch.cuda.synchronize()
      e0.record()
      last[name] = fn()
      e1.record()
      e1.synchronize()
      if i >= args.warmup:
        ms[name].append(e0.elapsed_time(e1))
  a, b = last[kinds[0][0]], last[kinds[1][0]]
  assert a.shape == b.shape == (1, N, T) and bool(torch.isfinite(a).all())
  diff = float((a.double() - b.double()).norm() / b.double().norm())
  med = {}
  for name, _ in kinds:
    m = statistics.median(ms[name])
    med[name] = m
    print(json.dumps({'tool': 'bench_score_folds', 'kind': name, 'N': N, 'folds': F, 'frames': T, 'precision': 'bf16', 'ms': [round(x, 2) for x in ms[name]],
                      'median_ms': round(m, 2), 'min_ms': round(min(ms[name]), 2), 'max_ms': round(max(ms[name]), 2),
                      'spread': round((max(ms[name]) - min(ms[name])) / m, 4)}), flush=True)
  ws = model._ws.numel() if model._ws is not None else 0
  print(json.dumps({'tool': 'bench_score_folds', 'summary': f'score_all against {F} model.score calls on pre-built compacted batches',
                    'score_all_median_ms': round(med[kinds[0][0]], 2), 'by_hand_median_ms': round(med[kinds[1][0]], 2),
                    'by_hand_over_score_all': round(med[kinds[1][0]] / med[kinds[0][0]], 3), 'frame_err_relative_difference': diff,
                    'frame_err_bit_equal': bool(torch.equal(a, b)), 'workspace_GiB': round(ws / 2 ** 30, 2)}), flush=True)


if __name__ == '__main__':
  main()
