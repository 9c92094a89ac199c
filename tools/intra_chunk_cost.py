"""What the intra-sample chunk options (spa3d_set_option "track_chunk" / "query_chunk") cost and buy at BASELINE.json configs[4]
(N = 8192 support tracks, Q = 2048 queries, T = 300, DINO 768 + depth 1, training).

  python tools/intra_chunk_cost.py            dry-run workspace bytes (no GPU needed) and the largest batch per step that fits one card
  python tools/intra_chunk_cost.py --gpu      also s/step of one fp16 sample with and without the options (loss_and_grads, synchronised)

The largest batch: the inputs of B samples (support tracks, visibility, fp16 DINO / depth planes, queries and targets) plus the workspace the
library asks for must fit the card's 288 GB with the model's own 0.8 workspace fraction applied to what the inputs leave free.  Without the
options the library already walks the batch one sample at a time when it must, so both modes are bounded by their one-sample workspace."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, Q, T, DINO, DEPTH = 8192, 2048, 300, 768, 1
CARD = 288e9
MODES = (('off', 0, 0), ('track_chunk 1024', 1024, 0), ('query_chunk 256', 0, 256), ('track_chunk 1024 + query_chunk 256', 1024, 256),
         ('track_chunk 512 + query_chunk 128', 512, 128))


def input_bytes(B):
  per = N * T * (3 * 4 + 4 + 2 * (DINO + DEPTH)) + Q * (4 * 4 + T * (3 * 4 + 4)) + 4
  return B * per


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--gpu', action='store_true')
  ap.add_argument('--steps', type=int, default=3)
  args = ap.parse_args()
  import spa3d
  lib = spa3d._lib.load()
  print(f'configs[4]: N = {N}, Q = {Q}, T = {T}, dino {DINO}, depth {DEPTH}; training; one sample per chunk')
  print(f'{"precision":9s} {"mode":38s} {"workspace GB":>12s} {"largest B":>9s}')
  for precision in ('fp32', 'fp16'):
    m = spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=DINO, depth_feature_dim=DEPTH, precision=precision)
    h = m._handle(DINO, DEPTH)[0]
    for name, tc, qc in MODES:
      spa3d._lib.check(lib.spa3d_set_option(h, b'track_chunk', float(tc)), h)
      spa3d._lib.check(lib.spa3d_set_option(h, b'query_chunk', float(qc)), h)
      ws = lib.spa3d_workspace_bytes(h, 1, N, Q, T, 1, 1)
      bmax = 0
      while lib.spa3d_workspace_bytes(h, bmax + 1, N, Q, T, 1, 1) <= 0.8 * (CARD - input_bytes(bmax + 1)):
        bmax += 1
      print(f'{precision:9s} {name:38s} {ws / 1e9:12.2f} {bmax:9d}')
  if not args.gpu:
    return
  import torch
  import bench
  dev = torch.device('cuda', 0)
  batch = bench.synth_batch(1, N, Q, T, DINO, DEPTH, dev, seed=316, feat_dtype=torch.float16)
  noise = torch.rand(1, 128, 96, generator=torch.Generator().manual_seed(11)).to(dev)
  print(f'fp16, one sample, loss_and_grads, 1 warm-up + {args.steps} timed calls each')
  for name, tc, qc in MODES[:4]:
    model = spa3d.TrackAutoEncoder3D(num_output_frames=T, dino_feature_dim=DINO, depth_feature_dim=DEPTH, precision='fp16',
                                     decoder_scan_chunk_size=qc or None, track_chunk_size=tc or None)
    params = model.init(0, batch)['params']
    model.loss_and_grads({'params': params}, batch, noise=noise)
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.steps):
      t0 = time.perf_counter()
      ld, _, _ = model.loss_and_grads({'params': params}, batch, noise=noise)
      torch.cuda.synchronize()
      ts.append(time.perf_counter() - t0)
    ts.sort()
    print(f'  {name:38s} median {ts[len(ts) // 2]:.3f} s/step (min {ts[0]:.3f}, max {ts[-1]:.3f}); loss {float(ld["total_loss"]):.6e}; '
          f'workspace {model._ws.numel() / 1e9:.1f} GB')
    del model, params
    torch.cuda.empty_cache()


if __name__ == '__main__':
  main()
