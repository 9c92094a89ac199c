"""The contract of spa3d_adamw_step_groups (include/spa3d.h) restated in float64 on torch tensors: parameter groups, frozen ranges, the clip norm
over the live elements, the skip on a non-finite norm, the bias correction at the number of applied updates, and the weight EMA.  With an empty
table and no EMA it is O.adamw_step, operation for operation (tests/test_adamw_groups_host.py pins both that and the agreement with
torch.optim.AdamW built from parameter groups).  Plain functions, no fixtures."""
import math

import torch


def scale_vectors(n, groups, dtype=torch.float64):
  """(lr_scale[n], wd_scale[n]) of a table [(begin, end, lr_scale, wd_scale)]: an element in no range has both scales 1"""
  ls, ws = torch.ones(n, dtype=dtype), torch.ones(n, dtype=dtype)
  for b, e, l, w in groups:
    ls[b:e] = l
    ws[b:e] = w
  return ls, ws


def linear_lookup(groups, i):
  """(range index or -1, lr_scale, wd_scale) of element i by a linear scan"""
  for k, (b, e, l, w) in enumerate(groups):
    if b <= i < e:
      return k, l, w
  return -1, 1.0, 1.0


def adamw_groups_step(p, g, m, v, step, lr, clip=1.0, wd=0.01, b1=0.9, b2=0.999, eps=1e-8, groups=(), ema=None, ema_decay=0.0, skipped=0):
  """One call on flat float64 tensors, in place.  `step` = calls before this one, `skipped` = updates skipped so far (scratch[3]).
  Returns (norm over the live elements, True when the step was skipped: nothing was written)."""
  n = p.numel()
  ls, ws = scale_vectors(n, groups, p.dtype)
  live = ls != 0
  gl = g[live]   # a frozen gradient is never read as a number
  gn = math.sqrt(float((gl.double() ** 2).sum()))
  if not math.isfinite(gn):
    return gn, True
  sc = 1.0 if gn < clip else clip / gn
  t = max(step + 1 - skipped, 1)
  gi = gl * sc
  ml = m[live].mul(b1).add(gi, alpha=1 - b1)
  vl = v[live].mul(b2).addcmul(gi, gi, value=1 - b2)
  mh = ml / (1 - b1 ** t)
  vh = vl / (1 - b2 ** t)
  pl = p[live]
  pl = pl.sub((lr * ls[live]) * (mh / (vh.sqrt() + eps) + (wd * ws[live]) * pl))
  m[live] = ml
  v[live] = vl
  p[live] = pl
  if ema is not None:
    ema[live] = ema_decay * ema[live] + (1 - ema_decay) * pl
  return gn, False


def draw_state(n, seed=5, ema=False):
  """p, g, m, v (and e) at the scales of test_adamw_step_matches_oracle, fp32 values"""
  gen = torch.Generator().manual_seed(seed)
  p = torch.randn(n, generator=gen)
  g = torch.randn(n, generator=gen) * 0.01
  m = torch.randn(n, generator=gen) * 0.001
  v = torch.rand(n, generator=gen) * 1e-4
  if not ema:
    return p, g, m, v
  return p, g, m, v, p + torch.randn(n, generator=gen) * 0.01


def draw_groups(bounds, seed=0):
  """a table over the given [(begin, end)] with scales drawn from {0, 0.1, 1, 10} x {0, 1, 3}; every value of both sets occurs once there are 12 ranges"""
  gen = torch.Generator().manual_seed(seed)
  L, W = (0.0, 0.1, 1.0, 10.0), (0.0, 1.0, 3.0)
  out = []
  for k, (b, e) in enumerate(bounds):
    if k < 12:
      l, w = L[k % 4], W[(k // 4 + k) % 3]
    else:
      l, w = L[int(torch.randint(4, (1,), generator=gen))], W[int(torch.randint(3, (1,), generator=gen))]
    out.append((b, e, l, w))
  return out
