"""What the "freeze" option (include/spa3d.h, spa3d_set_option) buys at the headline shape of bench.py: B = 64 clips of 2048 support + 512 query tracks,
T = 150, DINO 768 + depth 1, bf16.

  python tools/bench_freeze.py [--repeats 3] [--batch 64] [--log profiles/rNN_freeze.log]

Per freeze level 0 / 1 / 2: ms per model.loss_and_grads call (HIP events around the call on its stream, after one warm-up call per level), the samples per
chunk the workspace gives (the largest chunk whose dry-run need fits the workspace, the rule the library applies) and the one-sample workspace need.
The three levels share one model, one workspace (the one the unfrozen call asks for) and one batch, and are timed in alternating order -- 0 1 2, 2 1 0,
0 1 2, ... -- so that a drift of the machine does not land on one level.  Needs the GPU: it fails without one."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, Q, T, DINO, DEPTH = 2048, 512, 150, 768, 1
LEVELS = (0, 1, 2)
NAMES = {0: 'none', 1: 'encoder', 2: 'encoder+latents'}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=3)
  ap.add_argument('--batch', type=int, default=64)
  ap.add_argument('--log', default=None)
  args = ap.parse_args()
  if args.repeats < 3:
    ap.error('--repeats must be at least 3')
  import torch
  if not torch.cuda.is_available():
    sys.exit('bench_freeze.py: no GPU -- a time measured anywhere else says nothing about the MI355X')
  import bench
  import spa3d
  lib = spa3d._lib.load()
  dev = torch.device('cuda', 0)
  B = args.batch
  model = spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=DINO, depth_feature_dim=DEPTH, precision='bf16')
  batch = bench.synth_batch(B, N, Q, T, DINO, DEPTH, dev, seed=1234, feat_dtype=torch.bfloat16)
  params = model.init(0, batch)['params']
  h, _, n = model._handle(DINO, DEPTH)
  grads = torch.empty(n, dtype=torch.float32, device=dev)
  lines = []

  def say(s):
    print(s, flush=True)
    lines.append(s)

  def call(k):
    ld, _, _ = model.loss_and_grads({'params': params}, batch, grads_flat=grads, freeze=k)
    return ld

  say(f'bench_freeze: B = {B}, N = {N}, Q = {Q}, T = {T}, dino {DINO}, depth {DEPTH}, bf16; {torch.cuda.get_device_name(0)}')
  losses = {}
  for k in LEVELS:  # warm-up, level 0 first: it sizes the workspace all three run in
    losses[k] = float(call(k)['total_loss'])
  torch.cuda.synchronize()
  ws = model._ws.numel()
  need, chunk, lo = {}, {}, {}
  for k in LEVELS:
    with spa3d.model._freeze_on(h, k):
      need[k] = lib.spa3d_workspace_bytes(h, 1, N, Q, T, 1, 1)
      chunk[k] = max([c for c in range(1, B + 1) if lib.spa3d_workspace_bytes(h, B, N, Q, T, c, 1) <= ws] or [0])
      lo[k] = spa3d.model.trainable_range(h)[0]
  ms = {k: [] for k in LEVELS}
  for r in range(args.repeats):
    for k in (LEVELS if r % 2 == 0 else LEVELS[::-1]):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      call(k)
      e1.record()
      e1.synchronize()
      ms[k].append(e0.elapsed_time(e1))
  say(f'workspace {ws / 1e9:.1f} GB (shared by the three levels); {args.repeats} timed calls per level in alternating order, one warm-up each')
  say(f'{"freeze":20s} {"trainable":>12s} {"ms/call median":>15s} {"min":>9s} {"max":>9s} {"vs 0":>7s} {"chunk":>6s} {"1-sample need GB":>17s}   loss')
  base = statistics.median(ms[0])
  for k in LEVELS:
    med = statistics.median(ms[k])
    say(f'{str(k) + " (" + NAMES[k] + ")":20s} {n - lo[k]:12d} {med:15.1f} {min(ms[k]):9.1f} {max(ms[k]):9.1f} {med / base:7.3f} {chunk[k]:6d} {need[k] / 1e9:17.2f}   '
        f'{losses[k]:.6e}')
  say('every call: ' + json.dumps({str(k): [round(x, 1) for x in ms[k]] for k in LEVELS}))
  if args.log:
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
