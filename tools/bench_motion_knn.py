"""The streaming k-NN and the manifold estimates against the matrix route they replace, on one GPU, in one process, timed with HIP events in
ALTERNATING order (a, b, c, a, b, c, ...), the first `--warmup` rounds dropped, `--reps` kept (as tools/bench_motion.py).

  knn       a  motion_knn        spa3d.motion_knn(a, k=3): the set against itself, each sample left out (rows x rows, E = 12288)
            b  pdist+topk        spa3d.motion_pdist(a) with the diagonal set to INT32_MAX, then torch.topk(k, largest=False): the matrix route
            c  motion_pdist      spa3d.motion_pdist(a) alone: the bare GEMM, the floor the reducing epilogue is judged by
  manifold  a  manifold_metrics  spa3d.manifold_metrics(real, gen, k=3) at R = G = rows
            b  precision_recall  spa3d.precision_recall(real, gen, k=3): three matrices, kthvalue and any (two of the four estimates)
  retrieve  a  motion_knn        spa3d.motion_knn(queries, gallery, k=5): --queries against --gallery rows with the planned splits
            (no matrix route is timed: at the default sizes it is the same GEMM plus a top-k over queries x gallery)

Before anything is timed the k-NN result is compared with the matrix route's (distances must be equal; indices may differ only where
distances tie, where torch.topk's order is unspecified and the library's is the lower index) and the estimates with precision_recall.
Prints one JSON line per kind and one summary line.  Nothing is gated.

  python tools/bench_motion_knn.py --reps 7"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rows', type=int, default=4096)
  ap.add_argument('--tokens', type=int, default=128)
  ap.add_argument('--dim', type=int, default=96)
  ap.add_argument('--queries', type=int, default=64)
  ap.add_argument('--gallery', type=int, default=262144)
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=2)
  args = ap.parse_args()
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import torch
  import spa3d
  assert torch.cuda.is_available(), 'bench_motion_knn needs the GPU: there is no CPU fallback and a CPU time would say nothing'
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  M, L, D = args.rows, args.tokens, args.dim
  E = L * D
  gen = torch.Generator(device=dev).manual_seed(11)
  real = spa3d.motion_codes(torch.randn(M, L, D, generator=gen, device=dev) * 0.6)
  # generated samples: real ones plus noise of three sizes
  amp = torch.tensor([0.1, 0.45, 0.9], device=dev)[torch.randint(0, 3, (M,), generator=gen, device=dev)]
  fake = spa3d.motion_codes(real[torch.randint(0, M, (M,), generator=gen, device=dev)].float() / 128.0 + torch.randn(M, L, D, generator=gen, device=dev) * amp[:, None, None])
  gallery = torch.randint(-128, 129, (args.gallery, E), generator=gen, device=dev, dtype=torch.int16)   # 6 GB at the default size
  queries = gallery[torch.randint(0, args.gallery, (args.queries,), generator=gen, device=dev)].clone()
  queries[:, ::7] += 1
  queries.clamp_(-128, 128)
  I32MAX = (1 << 31) - 1

  def matrix_topk():
    d = spa3d.motion_pdist(real)
    d.fill_diagonal_(I32MAX)
    return torch.topk(d, 3, dim=1, largest=False, sorted=True)

  lib_knn = lambda: spa3d.motion_knn(real, k=3)
  (kd, ki), (td, ti) = lib_knn(), matrix_topk()
  dist_equal = bool(torch.equal(kd, td))
  idx_differ = int((ki != ti).sum())
  flat = real.reshape(M, E)
  rows = torch.arange(M, device=dev)[:, None].expand(M, 3)
  idx_differ_only_at_ties = bool(((ki == ti) | (((flat[rows] - flat[ti]).int() ** 2).sum(-1) == kd)).all())
  m = spa3d.manifold_metrics(real, fake, k=3)
  pr = spa3d.precision_recall(real, fake, k=3)
  estimates = {'precision': m.precision, 'recall': m.recall, 'density': m.density, 'coverage': m.coverage, 'equal_precision_recall': (m.precision, m.recall) == pr}
  rd, ri = spa3d.motion_knn(queries, gallery, k=5)
  splits = int(spa3d._lib.load().spa3d_motion_knn_workspace_bytes(args.queries, args.gallery, 5, 0)) // (args.queries * 5 * 8) or 1
  del kd, ki, td, ti, rows

  steps = [('knn', M, M, [('motion_knn', lib_knn), ('pdist+topk', matrix_topk), ('motion_pdist', lambda: spa3d.motion_pdist(real))]),
           ('manifold', M, M, [('manifold_metrics', lambda: spa3d.manifold_metrics(real, fake, k=3)), ('precision_recall', lambda: spa3d.precision_recall(real, fake, k=3))]),
           ('retrieve', args.queries, args.gallery, [('motion_knn', lambda: spa3d.motion_knn(queries, gallery, k=5))])]
  med = {}
  for step, Ma, Mb, kinds in steps:
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
      med[(step, name)] = statistics.median(ms[name])
      rec = {'tool': 'bench_motion_knn', 'step': step, 'kind': name, 'Ma': Ma, 'Mb': Mb, 'E': E, 'event_ms': [round(v, 4) for v in ms[name]], 'median_ms': round(med[(step, name)], 4),
             'min_ms': round(min(ms[name]), 4), 'max_ms': round(max(ms[name]), 4), 'host_wall_median_ms': round(statistics.median(wall[name]), 4)}
      if name in ('motion_knn', 'motion_pdist'):
        rec['mfma_tflops_median'] = round(2.0 * Ma * Mb * E / (med[(step, name)] * 1e-3) / 1e12, 1)
      if step == 'retrieve':
        rec['planned_splits'] = splits
        rec['gallery_gbytes_per_s'] = round(Mb * E * 2 / (med[(step, name)] * 1e-3) / 1e9, 1)
      print(json.dumps(rec), flush=True)
  print(json.dumps({'tool': 'bench_motion_knn', 'summary': 'HIP-event time per call', 'knn_distances_equal_matrix_route': dist_equal, 'knn_indices_differing_from_torch_topk': idx_differ,
                    'those_differ_only_where_distances_tie': idx_differ_only_at_ties, 'estimates': estimates,
                    'motion_knn_over_motion_pdist': round(med[('knn', 'motion_knn')] / med[('knn', 'motion_pdist')], 3),
                    'pdist_topk_over_motion_knn': round(med[('knn', 'pdist+topk')] / med[('knn', 'motion_knn')], 3),
                    'precision_recall_over_manifold_metrics': round(med[('manifold', 'precision_recall')] / med[('manifold', 'manifold_metrics')], 3)}), flush=True)


if __name__ == '__main__':
  main()
