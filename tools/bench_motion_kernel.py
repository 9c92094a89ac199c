"""The kernel sums against the bare GEMM and against the matrix route they replace, on one GPU, in one process, timed with HIP events in
ALTERNATING order (a, b, c, a, b, c, ...), the first `--warmup` rounds dropped, `--reps` kept (as tools/bench_motion_knn.py).

  sums      a  kernel_sums       spa3d.motion_kernel_sums(a, b, degree=3): row and column sums, rows x rows at E = tokens * dim, nothing left out
            b  motion_pdist      spa3d.motion_pdist(a, b, kind='dot'): the same K loop with a plain store -- the difference is the epilogue's price
            c  matrix_route      motion_pdist('dot'), then (d.double() + C) ** 3 and .sum(1) in torch: row sums only, and not exact
  distance  a  kernel_distance   spa3d.kernel_distance(real, gen) end to end at R = G = rows: three calls, the read-back and the exact rationals
                                 on the host (the host wall time is the figure that counts: the Fractions run after the last kernel)

`sums` runs at every size of --rows (default 4096 and 512).  Before anything is timed the library's row sums are compared with the matrix
route's float64 ones: how many differ from the exact integers and by how much, relative.  Prints one JSON line per kind and size and one summary
line.  Nothing is gated.

  python tools/bench_motion_kernel.py --reps 7"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rows', type=int, nargs='+', default=[4096, 512])
  ap.add_argument('--tokens', type=int, default=128)
  ap.add_argument('--dim', type=int, default=96)
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=2)
  args = ap.parse_args()
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import torch
  import spa3d
  assert torch.cuda.is_available(), 'bench_motion_kernel needs the GPU: there is no CPU fallback and a CPU time would say nothing'
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  L, D = args.tokens, args.dim
  E = L * D
  C = 16384 * E
  gen = torch.Generator(device=dev).manual_seed(11)
  Mmax = max(args.rows)
  real = spa3d.motion_codes(torch.randn(Mmax, L, D, generator=gen, device=dev) * 0.6)
  amp = torch.tensor([0.1, 0.45, 0.9], device=dev)[torch.randint(0, 3, (Mmax,), generator=gen, device=dev)]
  fake = spa3d.motion_codes(real[torch.randint(0, Mmax, (Mmax,), generator=gen, device=dev)].float() / 128.0 + torch.randn(Mmax, L, D, generator=gen, device=dev) * amp[:, None, None])

  def timed(kinds):
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
    return ms, wall

  summary = {}
  for M in args.rows:
    a, b = real[:M].reshape(M, E), fake[:M].reshape(M, E)

    def matrix_route():
      d = spa3d.motion_pdist(a, b, kind='dot')
      return ((d.double() + float(C)) ** 3).sum(1)

    exact = spa3d.limbs_to_ints(spa3d.motion_kernel_sums(a, b, degree=3, cols=False)[0])
    approx = matrix_route().tolist()
    rel = [abs(int(x) - y) / y for x, y in zip(approx, exact)]
    differ = sum(1 for x, y in zip(approx, exact) if int(x) != y)
    kinds = [('kernel_sums', lambda: spa3d.motion_kernel_sums(a, b, degree=3)), ('motion_pdist', lambda: spa3d.motion_pdist(a, b, kind='dot')), ('matrix_route', matrix_route)]
    ms, wall = timed(kinds)
    med = {name: statistics.median(ms[name]) for name, _ in kinds}
    for name, _ in kinds:
      rec = {'tool': 'bench_motion_kernel', 'step': 'sums', 'kind': name, 'Ma': M, 'Mb': M, 'E': E, 'event_ms': [round(v, 4) for v in ms[name]], 'median_ms': round(med[name], 4),
             'min_ms': round(min(ms[name]), 4), 'max_ms': round(max(ms[name]), 4), 'host_wall_median_ms': round(statistics.median(wall[name]), 4)}
      if name != 'matrix_route':
        rec['mfma_tflops_median'] = round(2.0 * M * M * E / (med[name] * 1e-3) / 1e12, 1)
      print(json.dumps(rec), flush=True)
    summary[f'rows_{M}'] = {'kernel_sums_over_motion_pdist': round(med['kernel_sums'] / med['motion_pdist'], 3), 'matrix_route_over_kernel_sums': round(med['matrix_route'] / med['kernel_sums'], 3),
                            'matrix_route_row_sums_differing_from_the_exact_integers': differ, 'of': M, 'matrix_route_max_relative_error': max(rel), 'largest_exact_row_sum_bits': max(exact).bit_length()}
  M = Mmax
  ms, wall = timed([('kernel_distance', lambda: spa3d.kernel_distance(real, fake))])
  kd = spa3d.kernel_distance(real, fake)
  print(json.dumps({'tool': 'bench_motion_kernel', 'step': 'distance', 'kind': 'kernel_distance', 'R': M, 'G': M, 'E': E, 'event_ms': [round(v, 4) for v in ms['kernel_distance']],
                    'median_ms': round(statistics.median(ms['kernel_distance']), 4), 'min_ms': round(min(ms['kernel_distance']), 4), 'max_ms': round(max(ms['kernel_distance']), 4),
                    'host_wall_ms': [round(v, 3) for v in wall['kernel_distance']], 'host_wall_median_ms': round(statistics.median(wall['kernel_distance']), 3), 'mmd2': kd.mmd2}), flush=True)
  summary['tool'] = 'bench_motion_kernel'
  summary['summary'] = 'HIP-event time per call'
  print(json.dumps(summary), flush=True)


if __name__ == '__main__':
  main()
