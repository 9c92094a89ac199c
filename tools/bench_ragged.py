"""Ragged batches against the two ways a user had before them: 32 clips whose track counts differ (n_b = q_b drawn once from a seeded list in
[64, 1024], T = 150, DINO 768 + depth 1, bf16), forward and train step.

  --mode a   one ragged call (batch keys support_count / query_count; needs a build with spa3d_set_counts)
  --mode b   32 single-sample calls on the cropped clips, gradients accumulated -- the only correct way without counts
  --mode c   one call zero-padded to 1024 with visible = 0 -- WRONG answers (tests/test_ragged_host.py); it bounds the padded work

Modes b and c use only the interface every commit has, so `--root DIR` may point at another checkout's built tree (the parent commit's) and
a job script can alternate processes of this tool: a (this tree), b and c (the other tree), each under its own timeout.  Every repetition ends
in a device synchronise; the first `--warmup` repetitions of each kind are dropped.  Prints one JSON line per kind (forward, train) with the
times in ms, their median / min / max and the live tracks per second at the median.

  python tools/bench_ragged.py --mode a --reps 7
  python tools/bench_ragged.py --mode b --reps 7 --root ../parent_checkout"""
import argparse
import json
import os
import random
import statistics
import sys
import time


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--mode', choices=('a', 'b', 'c'), required=True)
  ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='checkout whose built package is measured')
  ap.add_argument('--clips', type=int, default=32)
  ap.add_argument('--lo', type=int, default=64)
  ap.add_argument('--hi', type=int, default=1024)
  ap.add_argument('--frames', type=int, default=150)
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--seed', type=int, default=0)
  ap.add_argument('--tag', default='')
  args = ap.parse_args()
  sys.path.insert(0, os.path.abspath(args.root))
  import torch
  import bench  # synth_batch of the measured tree
  import spa3d
  assert torch.cuda.is_available(), 'bench_ragged needs the GPU: there is no CPU fallback and a CPU time would say nothing'
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  rng = random.Random(args.seed)
  counts = [rng.randint(args.lo, args.hi) for _ in range(args.clips)]
  B, N, T = args.clips, args.hi, args.frames
  model = spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=768, depth_feature_dim=1, precision='bf16')
  full = bench.synth_batch(B, N, N, T, 768, 1, dev, seed=77, feat_dtype=torch.bfloat16)
  sup = ('support_tracks', 'support_tracks_visible', 'dino_features', 'depth_features')
  qry = ('query_points', 'query_tracks', 'query_tracks_visible')
  for b, n in enumerate(counts):  # padding: zeros with visible = 0 (what mode c feeds; modes a and b never read it)
    for k in sup + qry:
      full[k][b, n:] = 0
  params = model.init(0, full)['params']
  v = {'params': params}
  noise = torch.rand(B, model.num_latent_tokens, model.latent_token_dim, generator=torch.Generator().manual_seed(1)).to(dev)
  grads = torch.zeros_like(params.flat)
  denom = float(max(sum(float(full['query_tracks_visible'][b, :n].sum()) for b, n in enumerate(counts)), 1.0))
  if args.mode == 'a':
    batch = dict(full)
    batch['support_count'] = torch.tensor(counts, dtype=torch.int32)
    batch['query_count'] = torch.tensor(counts, dtype=torch.int32)
    fwd = lambda: model(v, batch, noise=noise)
    trn = lambda: model.loss_and_grads(v, batch, grads_flat=grads, denom=denom, noise=noise)
  elif args.mode == 'c':
    fwd = lambda: model(v, full, noise=noise)
    trn = lambda: model.loss_and_grads(v, full, grads_flat=grads, denom=denom, noise=noise)
  else:
    clips = []
    for b, n in enumerate(counts):
      clips.append({k: (t[b:b + 1, :n].contiguous() if k in sup + qry else t[b:b + 1].contiguous()) for k, t in full.items()})
    del full
    torch.cuda.empty_cache()
    # one workspace for all clips, sized once for the widest single-sample train call: otherwise it would grow clip by clip inside the timed loop,
    # and a single-sample forward whose workspace is exactly its own estimate returned "arena overflow" at one of these widths (NOTEBOOK.md, open)
    model._workspace(model._handle(768, 1)[0], 1, N, N, T, True, dev)

    def fwd():
      for b, c in enumerate(clips):
        model(v, c, noise=noise[b:b + 1])

    def trn():
      for b, c in enumerate(clips):
        model.loss_and_grads(v, c, grads_flat=grads, accumulate=b > 0, denom=denom, noise=noise[b:b + 1])
  live = sum(counts)
  for kind, fn in (('forward', fwd), ('train', trn)):
    ms = []
    for i in range(args.warmup + args.reps):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      fn()
      torch.cuda.synchronize()
      if i >= args.warmup:
        ms.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(ms)
    print(json.dumps({'tool': 'bench_ragged', 'mode': args.mode, 'tag': args.tag, 'kind': kind, 'clips': B, 'live_tracks': live, 'padded_tracks': B * N,
                      'frames': T, 'precision': 'bf16', 'ms': [round(x, 2) for x in ms], 'median_ms': round(med, 2), 'min_ms': round(min(ms), 2),
                      'max_ms': round(max(ms), 2), 'live_tracks_per_s': round(live / (med * 1e-3), 1), 'root': os.path.abspath(args.root)}), flush=True)


if __name__ == '__main__':
  main()
