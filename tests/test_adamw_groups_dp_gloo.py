"""TrainState(param_groups=..., ema_decay=...) on the CPU with stand-in compute / AdamW (the pattern of tests/test_freeze_dp_gloo.py), at world size 1
(no process group) and at world size 2 over gloo: the adamw hook keeps its twelve positional arguments when nothing is set; with groups or an EMA it
also receives groups= (cut to the trainable range and shifted under `freeze`), ema= and ema_decay=; the EMA starts as rank 0's parameters on every
rank; frozen ranges and the frozen prefix keep their bits; and checkpoints round-trip exactly with and without the EMA."""
import os
import tempfile
import traceback

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import optim_util as OU
from test_dp_gloo import _free_port
from util import MINI, O


def _scenario(rank, world):
  import ctypes as C
  import spa3d
  from util import product_model
  cfg = O.Config(**MINI, use_dino=False, use_depth=False)
  model = product_model(spa3d, cfg, 'fp32')
  h, leaves, n = model._handle(0, 0)
  b4 = (C.c_int64 * 4)()
  assert spa3d._lib.load().spa3d_grad_segments(h, b4) == 0
  b1 = int(b4[1])
  params = O.init_params(cfg, seed=5 + rank, dtype=torch.float32, with_dino=False, with_depth=False, perturb=0.1)   # every rank its own: rank 0's must win
  batch = O.synthetic_batch(2, 5, 4, 8, seed=17)

  def compute(params_, batch_, grads_flat, denom, discretize, noise):
    grads_flat.copy_(torch.linspace(-1.0, 1.0, grads_flat.numel()) * (rank + 1) * 1e-3)
    z = torch.zeros(())
    return {'total_loss': z + 1.0 + rank, 'position_loss': z, 'visible_loss': z}

  common = dict(learning_rate=1e-2, warmup_steps=1, total_steps=10, grad_bucket_bytes=4000, compute=compute, noise_fn=lambda k, dev: torch.zeros(k), weight_decay=0.1)

  # ---- nothing set: the hook is called exactly as before -- a stand-in without keywords would raise on any
  calls = []

  def adamw_old(flat, grads, mm, vv, lr, step, clip, b1_, b2_, eps, wd, scratch):
    calls.append(flat.numel())
    scratch[0] = O.adamw_step({'p': flat}, {'p': grads}, {'p': mm}, {'p': vv}, step, lr, clip=clip, wd=wd, b1=b1_, b2=b2_, eps=eps)

  st0 = spa3d.TrainState(model, params, adamw=adamw_old, **common)
  assert st0.ema is None and st0.ema_params is None and st0.groups is None
  st0.train_step(batch, discretize=False)
  assert calls == [n]
  try:
    st0.eval_step(batch, use_ema=True)
    raise AssertionError('eval_step(use_ema=True) without an EMA must raise')
  except ValueError:
    pass

  # ---- groups + EMA under freeze=1
  pg = spa3d.param_groups(model, params, rules=[(r'^track_readout_attn/layer_0/', 0.0, 1.0)], no_decay=True, layer_decay=0.8)
  full = pg.ranges
  assert any(b < b1 < e for b, e, _, _ in full) or any(e <= b1 for _, e, _, _ in full), 'the table must reach below the frozen boundary for the cut to show'
  want = [(max(b, b1) - b1, e - b1, ls, ws) for b, e, ls, ws in full if e > b1]
  seen = []

  def adamw_new(flat, grads, mm, vv, lr, step, clip, b1_, b2_, eps, wd, scratch, groups=None, ema=None, ema_decay=None):
    seen.append((flat.numel(), list(groups), None if ema is None else ema.numel(), ema_decay, ema is not None and ema.data_ptr() == st.ema.data_ptr() + 4 * b1))
    gn, _ = OU.adamw_groups_step(flat, grads, mm, vv, step, lr, clip=clip, wd=wd, b1=b1_, b2=b2_, eps=eps, groups=groups, ema=ema, ema_decay=ema_decay or 0.0)
    scratch[0] = gn

  st = spa3d.TrainState(model, params, adamw=adamw_new, freeze='encoder', param_groups=pg, ema_decay=0.9, **common)
  assert st.groups == want and st.ema_decay == 0.9
  assert st.ema.data_ptr() != st.flat.data_ptr() and torch.equal(st.ema, st.flat)           # a copy of the (rank 0) parameters
  assert st.ema_params.flat is st.ema and set(O.tree_flatten(st.ema_params)) == set(O.tree_flatten(st.params))
  ref0 = O.init_params(cfg, seed=5, dtype=torch.float32, with_dino=False, with_depth=False, perturb=0.1)
  ema_is_rank0 = bool(torch.equal(st.ema, model.flat_from_tree(ref0, device='cpu')))
  st.m[:b1] = 0.25; st.v[:b1] = 0.5
  start = [t.clone() for t in (st.flat, st.m, st.v, st.ema)]
  outs = [st.train_step(batch, discretize=False) for _ in range(3)]
  assert len(seen) == 3 and all(s == (n - b1, want, n - b1, 0.9, True) for s in seen), seen[0][:1]
  now = (st.flat, st.m, st.v, st.ema)
  assert all(torch.equal(a[:b1], b[:b1]) for a, b in zip(start, now)), 'the frozen prefix moved'
  ls, _ = OU.scale_vectors(n, full)
  frozen = (ls == 0) & (torch.arange(n) >= b1)
  live = (ls != 0) & (torch.arange(n) >= b1)
  assert int(frozen.sum()) > 0 and all(torch.equal(a[frozen], b[frozen]) for a, b in zip(start, now)), 'a frozen range moved'
  assert all(float((a[live] != b[live]).float().mean()) > 0.9 for a, b in zip(start, now)), 'part of the live elements did not move'
  # 'train/grad_norm': the norm of the rank-summed gradient over the live elements
  g = torch.linspace(-1.0, 1.0, n) * 1e-3 * sum(r + 1 for r in range(world))
  gn = float(outs[-1]['train/grad_norm'])
  assert abs(gn - float(g[live].double().norm())) < 1e-6 * gn
  # eval_step evaluates either set of weights
  got = []
  st._evaluate = lambda p_, batch_, denom, discretize, noise: (got.append(p_) or {'total_loss': torch.zeros(()), 'position_loss': torch.zeros(()), 'visible_loss': torch.zeros(())}, None)
  st.eval_step(batch); st.eval_step(batch, use_ema=True)
  assert got[0] is st.params and got[1] is st.ema_params

  # ---- EMA alone, no freeze: an empty table, the whole buffers
  seen2 = []

  def adamw_ema(flat, grads, mm, vv, lr, step, clip, b1_, b2_, eps, wd, scratch, groups=None, ema=None, ema_decay=None):
    seen2.append((flat.numel(), list(groups), ema.numel(), ema_decay))
    scratch[0] = 0.0

  st_e = spa3d.TrainState(model, params, adamw=adamw_ema, ema_decay=0.5, **common)
  st_e.train_step(batch, discretize=False)
  assert seen2 == [(n, [], n, 0.5)]

  # ---- checkpoints (each rank its own file)
  with tempfile.TemporaryDirectory() as d:
    path = spa3d.save_checkpoint(os.path.join(d, f'with_ema_{rank}'), st.params, st)
    keys = set(np.load(path).files)
    names = {nm for nm, _, _ in leaves}
    base = names | {f'opt_m/{k}' for k in names} | {f'opt_v/{k}' for k in names} | {'step', 'opt_scratch'}
    assert keys == base | {f'ema/{k}' for k in names}
    st2 = spa3d.TrainState(model, O.init_params(cfg, seed=99, dtype=torch.float32, with_dino=False, with_depth=False), adamw=adamw_new, freeze='encoder',
                           param_groups=pg, ema_decay=0.9, **common)
    spa3d.load_train_state(path, st2)
    in_leaf = torch.zeros(n, dtype=torch.bool)   # a checkpoint holds the leaves, not the alignment padding between them
    for _, shape, off in leaves:
      in_leaf[off:off + int(np.prod(shape))] = True
    assert all(torch.equal(a[in_leaf], b[in_leaf]) for a, b in zip((st2.flat, st2.m, st2.v, st2.ema), now)) and st2.step == st.step == 3
    assert not torch.equal(st2.ema[in_leaf], st2.flat[in_leaf])
    tree = O.tree_flatten(spa3d.load_checkpoint(path, ema=True))
    assert set(tree) == names and all(np.array_equal(tree[k], v.numpy()) for k, v in O.tree_flatten(st.ema_params).items())
    plain = O.tree_flatten(spa3d.load_checkpoint(path))
    assert set(plain) == names and all(np.array_equal(plain[k], v.numpy()) for k, v in O.tree_flatten(st.params).items())
    # a state without an EMA writes the keys it always wrote; loaded into a state that keeps one, the EMA starts at the loaded parameters
    path0 = spa3d.save_checkpoint(os.path.join(d, f'without_ema_{rank}'), st0.params, st0)
    assert set(np.load(path0).files) == base
    spa3d.load_train_state(path0, st2)
    assert torch.equal(st2.flat[in_leaf], st0.flat[in_leaf]) and torch.equal(st2.ema, st2.flat) and st2.step == 1
    try:
      spa3d.load_checkpoint(path0, ema=True)
      raise AssertionError('load_checkpoint(ema=True) of a file without an EMA must raise')
    except KeyError:
      pass
    # ... and a file with an EMA loads into a state without one
    spa3d.load_train_state(path, st0)
    assert torch.equal(st0.flat[in_leaf], st.flat[in_leaf]) and st0.ema is None
  return ema_is_rank0, gn


def _worker(rank, world, port, q):
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  dist.init_process_group('gloo', rank=rank, world_size=world)
  torch.set_num_threads(2)   # (in the spawned workers only: the in-process case must leave the suite's thread count alone)
  try:
    q.put((rank, 'ok') + _scenario(rank, world))
  except BaseException:
    q.put((rank, traceback.format_exc(), False, 0.0))
  finally:
    dist.destroy_process_group()


def test_trainstate_groups_and_ema_world_size_1():
  ema_is_rank0, gn = _scenario(0, 1)
  assert ema_is_rank0 and gn > 0


def test_trainstate_groups_and_ema_world_size_2_gloo():
  ctx = mp.get_context('spawn')
  q = ctx.SimpleQueue()
  port = _free_port()
  procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
  for p in procs:
    p.start()
  for p in procs:
    p.join(300)
    if p.is_alive():
      p.kill()
    assert p.exitcode == 0, f'worker exit code {p.exitcode}'
  res = sorted([q.get(), q.get()], key=lambda r: r[0])
  for rank, status, ema_is_rank0, gn in res:
    assert status == 'ok', f'rank {rank}:\n{status}'
    assert ema_is_rank0, f'rank {rank}: the EMA is not rank 0\'s parameters'
  assert res[0][3] == res[1][3] > 0
