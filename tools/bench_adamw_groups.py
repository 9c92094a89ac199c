"""Grouped AdamW + weight EMA against the plain optimizer step, at the parameter count of the full model (spa3d_param_elems):

  (a) spa3d_adamw_step
  (b) spa3d_adamw_step_groups with no table
  (c) ... with the per-leaf table of param_groups(no_decay=True, layer_decay=0.8)
  (d) (c) with the EMA
  (e) the workaround without the entry point: one spa3d_adamw_step per range of (c) and per gap between them
      (wrong as an optimizer -- every call clips by its own slice's norm -- and three launches per slice)

HIP events around every call, warm-up, REPEATS rounds with the order of the configurations alternating from round to round; reports the median and
the spread of each, and the achieved bytes/s at 28 B per element for the update (36 with the EMA) plus 4 B for the norm pass, beside the 6.29 TB/s that a
float4 copy reaches on this part.  Needs a GPU: there is no fall-back.

  python tools/bench_adamw_groups.py [--repeats 9] [--out profiles/r22_adamw_groups.log]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spa3d  # noqa: E402

COPY_TBS = 6.29


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=9)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--inner', type=int, default=5, help='calls per timed window')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert args.repeats >= 7
  assert torch.cuda.is_available(), 'bench_adamw_groups needs a GPU'
  lib = spa3d._lib.load()
  model = spa3d.TrackAutoEncoder3D(precision='bf16')
  h, leaves, n = model._handle(768, 1)
  assert n == lib.spa3d_param_elems(h)
  params = model.tree_from_flat(torch.zeros(n), 768, 1)   # (the table needs names and offsets only)
  pg = spa3d.param_groups(model, params, no_decay=True, layer_decay=0.8)
  ranges = pg.ranges
  # (e): every range, and every gap between ranges, as a slice of its own
  slices, prev = [], 0
  for b, e, _, _ in ranges:
    if b > prev:
      slices.append((prev, b))
    slices.append((b, e))
    prev = e
  if prev < n:
    slices.append((prev, n))

  gen = torch.Generator(device='cuda').manual_seed(0)
  p = torch.randn(n, device='cuda', generator=gen)
  g = torch.randn(n, device='cuda', generator=gen) * 1e-4
  m = torch.zeros(n, device='cuda'); v = torch.zeros(n, device='cuda'); ema = p.clone()
  scratch = torch.zeros(1024, device='cuda')
  tab = (spa3d._lib.ParamGroup * len(ranges))(*[spa3d._lib.ParamGroup(*r) for r in ranges])
  nb = lib.spa3d_adamw_groups_workspace_bytes(len(ranges))
  ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
  s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  hyper = (3e-4, 7, 1.0, 0.9, 0.999, 1e-8, 0.01)
  P, G, M, V, E, S, W = (t.data_ptr() for t in (p, g, m, v, ema, scratch, ws))

  def plain():
    assert lib.spa3d_adamw_step(P, G, M, V, n, *hyper, S, s) == 0

  def groups(table, k, e):
    assert lib.spa3d_adamw_step_groups(P, G, M, V, n, *hyper, table, k, e, 0.999, S, W if k else None, nb if k else 0, s) == 0

  def per_slice():
    for b, e in slices:
      assert lib.spa3d_adamw_step(P + 4 * b, G + 4 * b, M + 4 * b, V + 4 * b, e - b, *hyper, S, s) == 0

  configs = [('a', 'spa3d_adamw_step', plain, 28), ('b', 'groups entry, no table', lambda: groups(None, 0, None), 28),
             ('c', f'per-leaf table, {len(ranges)} ranges', lambda: groups(tab, len(ranges), None), 28),
             ('d', '(c) + EMA', lambda: groups(tab, len(ranges), E), 36), ('e', f'one spa3d_adamw_step per slice, {len(slices)} slices', per_slice, 28)]
  times = {k: [] for k, _, _, _ in configs}
  for r in range(args.warmup + args.repeats):
    order = configs if r % 2 == 0 else configs[::-1]
    for k, _, fn, _ in order:
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(args.inner):
        fn()
      e1.record()
      torch.cuda.synchronize()
      if r >= args.warmup:
        times[k].append(e0.elapsed_time(e1) / args.inner)
  lines = [f'bench_adamw_groups: n = {n} elements ({len(leaves)} leaves), {args.repeats} repeats of {args.inner} calls after {args.warmup} warm-up rounds, order alternating',
           f'  bytes per element: 28 update (36 with EMA) + 4 norm; float4 copy on this part: {COPY_TBS} TB/s']
  med = {}
  for k, name, _, bpe in configs:
    t = sorted(times[k])
    med[k] = statistics.median(t)
    tbs = (bpe + 4) * n / (med[k] * 1e-3) / 1e12
    lines.append(f'  ({k}) {name:48s} median {med[k]:8.4f} ms  min {t[0]:8.4f}  max {t[-1]:8.4f}   {tbs:5.2f} TB/s = {100 * tbs / COPY_TBS:5.1f}% of the copy rate')
  spread = (max(times['a']) - min(times['a'])) / med['a']
  lines.append(f'  (b) / (a) = {med["b"] / med["a"]:.4f}   run-to-run spread of (a): {100 * spread:.2f}% of its median')
  lines.append(f'  (c) / (a) = {med["c"] / med["a"]:.4f}   (d) / (c) = {med["d"] / med["c"]:.4f} (36 + 4 over 28 + 4 bytes = 1.25)   (e) / (c) = {med["e"] / med["c"]:.4f}')
  lines.append(f'  (c) < (e): {med["c"] < med["e"]}')
  text = '\n'.join(lines)
  print(text, flush=True)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
