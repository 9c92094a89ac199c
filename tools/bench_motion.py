"""The two device steps of the latent-set metrics that do arithmetic, each against the torch route a caller would write, on one GPU, in one process,
timed with HIP events in ALTERNATING order (a, b, a, b, ...), the first `--warmup` rounds dropped.

  pdist    a  motion_pdist   spa3d.motion_pdist(a, b): Ma x Mb exact int32 squared distances of flat codes (E = 12288 = 128 tokens x 96)
           b  torch          a.float() @ b.float().T in fp32 plus the row norms, rounded to int32.  Whether that result is exact is checked against
                             the library's and printed: an fp32 sum of 12288 products of up to 2^14 passes 2^24, so it need not be.
  moments  a  moments_add    one MotionStats.update of --clips clips (both pools)
           b  torch.cov      torch.cov of the same rows in float32 (token rows, or the per-clip token means), plus their mean: floating-point
                             statistics whose bits depend on the batch; the largest relative difference to the exact covariance is printed.

The MFMA rate of the pdist kernel is 2 Ma Mb E / time, against the 2.5 PFLOP/s dense bf16 peak of the MI355X.  A 64 x 64 corner of the library's
matrix is checked against NumPy int64 before anything is timed.  Prints one JSON line per kind and one summary line.  Nothing is gated.

  python tools/bench_motion.py --reps 7"""
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
  ap.add_argument('--clips', type=int, default=64)
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=2)
  args = ap.parse_args()
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import numpy as np
  import torch
  import spa3d
  assert torch.cuda.is_available(), 'bench_motion needs the GPU: there is no CPU fallback and a CPU time would say nothing'
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  torch.backends.cuda.matmul.allow_tf32 = False
  M, L, D = args.rows, args.tokens, args.dim
  E = L * D
  gen = torch.Generator(device=dev).manual_seed(11)
  # codes of latents that fill the range: a clipped normal, so +-128 is common
  a = spa3d.motion_codes((torch.randn(M, L, D, generator=gen, device=dev) * 0.6))
  b = spa3d.motion_codes((torch.randn(M, L, D, generator=gen, device=dev) * 0.6))
  fa, fb = a.reshape(M, E), b.reshape(M, E)

  def torch_pdist():
    x, y = fa.float(), fb.float()
    return ((x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * (x @ y.t())).to(torch.int32)

  lib_pdist = lambda: spa3d.motion_pdist(a, b)
  ours, theirs = lib_pdist(), torch_pdist()
  corner = ours[:64, :64].cpu().numpy().astype(np.int64)
  x, y = fa[:64].cpu().numpy().astype(np.int64), fb[:64].cpu().numpy().astype(np.int64)
  corner_exact = bool(np.array_equal(corner, (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2 * (x @ y.T)))
  torch_wrong = int((ours != theirs).sum())
  torch_worst = int((ours.long() - theirs.long()).abs().max())
  del ours, theirs

  clips = a[:args.clips].contiguous()

  def lib_moments(pool):
    st = spa3d.MotionStats(D, L, pool).update(clips)   # the state is on the device from here on: a timed call is one spa3d_motion_moments_add
    return lambda: st.update(clips).state

  def torch_cov(pool):
    def f():
      rows = clips.reshape(-1, D).float() / 128.0 if pool == 'token' else clips.float().sum(1) / (128.0 * L)
      return torch.cov(rows.t(), correction=0), rows.mean(0)
    return f

  cov_diff = {}
  for pool in ('token', 'clip'):
    st = spa3d.MotionStats(D, L, pool).update(clips)
    exact = torch.from_numpy(st.cov)
    got = torch_cov(pool)()[0].double().cpu()
    cov_diff[pool] = float((got - exact).abs().max() / exact.abs().max())

  pairs = [('pdist', [('motion_pdist', lib_pdist), ('torch', torch_pdist)]),
           ('moments_token', [('moments_add', lib_moments('token')), ('torch.cov', torch_cov('token'))]),
           ('moments_clip', [('moments_add', lib_moments('clip')), ('torch.cov', torch_cov('clip'))])]
  med = {}
  for step, kinds in pairs:
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
      rec = {'tool': 'bench_motion', 'step': step, 'kind': name, 'rows': M, 'E': E, 'clips': args.clips, 'event_ms': [round(v, 4) for v in ms[name]],
             'median_ms': round(med[(step, name)], 4), 'min_ms': round(min(ms[name]), 4), 'max_ms': round(max(ms[name]), 4), 'host_wall_median_ms': round(statistics.median(wall[name]), 4)}
      if (step, name) == ('pdist', 'motion_pdist'):
        rec['mfma_tflops_median'] = round(2.0 * M * M * E / (med[(step, name)] * 1e-3) / 1e12, 1)
        rec['share_of_2.5_PF_bf16_peak'] = round(rec['mfma_tflops_median'] / 2500.0, 4)
      print(json.dumps(rec), flush=True)
  print(json.dumps({'tool': 'bench_motion', 'summary': 'HIP-event time per call; ratios are torch route / library call', 'library_corner_64x64_equals_int64': corner_exact,
                    'torch_pdist_entries_differing_from_exact': torch_wrong, 'of': M * M, 'torch_pdist_worst_abs_difference': torch_worst, 'torch_pdist_is_exact': torch_wrong == 0,
                    'torch_over_motion_pdist': round(med[('pdist', 'torch')] / med[('pdist', 'motion_pdist')], 3),
                    'torch_cov_over_moments_add_token': round(med[('moments_token', 'torch.cov')] / med[('moments_token', 'moments_add')], 3),
                    'torch_cov_over_moments_add_clip': round(med[('moments_clip', 'torch.cov')] / med[('moments_clip', 'moments_add')], 3),
                    'torch_cov_max_rel_difference_to_exact': cov_diff}), flush=True)


if __name__ == '__main__':
  main()
