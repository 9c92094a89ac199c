"""TrainState(freeze=1) at world size 2 over gloo on the CPU, with stand-in compute / AdamW (the pattern of tests/test_dp_gloo.py): the optimiser and the
gradient all-reduce see the trainable range [b1, n) of the flat buffers only, and the frozen prefix of the parameters and of both moments keeps its bits."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_dp_gloo import _free_port
from util import MINI, O


def _worker(rank, world, port, q):
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  dist.init_process_group('gloo', rank=rank, world_size=world)
  try:
    import ctypes as C
    import spa3d
    from util import product_model
    torch.set_num_threads(2)
    cfg = O.Config(**MINI, use_dino=False, use_depth=False)
    model = product_model(spa3d, cfg, 'fp32')
    h, _, n = model._handle(0, 0)
    b4 = (C.c_int64 * 4)()
    assert spa3d._lib.load().spa3d_grad_segments(h, b4) == 0
    b1 = int(b4[1])
    params = O.init_params(cfg, seed=5, dtype=torch.float32, with_dino=False, with_depth=False, perturb=0.1)
    seen = {'adamw': [], 'allreduce': []}

    def compute(params_, batch, grads_flat, denom, discretize, noise):  # a full, rank-dependent gradient: a stand-in knows nothing of the option
      grads_flat.copy_(torch.linspace(-1.0, 1.0, grads_flat.numel()) * (rank + 1))
      z = torch.zeros(())
      return {'total_loss': z + 1.0 + rank, 'position_loss': z, 'visible_loss': z}

    def adamw(flat, grads, mm, vv, lr, step, clip, b1_, b2_, eps, wd, scratch):  # moves every element it is handed (weight decay included)
      seen['adamw'].append((flat.numel(), grads.numel(), mm.numel(), vv.numel()))
      scratch[0] = O.adamw_step({'p': flat}, {'p': grads}, {'p': mm}, {'p': vv}, step, lr, clip=clip, wd=wd, b1=b1_, b2=b2_, eps=eps)

    st = spa3d.TrainState(model, params, learning_rate=1e-2, warmup_steps=1, total_steps=10, grad_bucket_bytes=4000, compute=compute, adamw=adamw,
                          noise_fn=lambda k, dev: torch.zeros(k), freeze='encoder', weight_decay=0.1)
    assert st.freeze == 1 and st.trainable_lo == b1
    st.m[:b1] = 0.25; st.v[:b1] = 0.5  # moments of a resumed state: they must come through untouched, not merely stay zero
    start = [t.clone() for t in (st.flat, st.m, st.v)]

    real = dist.all_reduce

    def all_reduce(t, *a, **kw):  # stand-in: notes which elements of the gradient buffer travel, then reduces them
      g0, g1 = st.grads.data_ptr(), st.grads.data_ptr() + 4 * n
      if g0 <= t.data_ptr() < g1:
        seen['allreduce'].append(((t.data_ptr() - g0) // 4, t.numel()))
      return real(t, *a, **kw)

    dist.all_reduce = all_reduce
    try:
      batch = O.synthetic_batch(2, 5, 4, 8, seed=17)
      outs = [st.train_step(batch, discretize=False) for _ in range(3)]
    finally:
      dist.all_reduce = real
    frozen_same = all(bool(torch.equal(a[:b1], b[:b1])) for a, b in zip(start, (st.flat, st.m, st.v)))
    moved = all(float((a[b1:] != b[b1:]).float().mean()) > 0.99 for a, b in zip(start, (st.flat, st.m, st.v)))
    # the reduced trainable gradients are the SUM over the ranks; the frozen ones are this rank's own, never reduced
    base = torch.linspace(-1.0, 1.0, n)
    sum_ok = bool(torch.equal(st.grads[b1:], (base * 1 + base * 2)[b1:])) and bool(torch.equal(st.grads[:b1], (base * (rank + 1))[:b1]))
    q.put((rank, b1, n, frozen_same, moved, sum_ok, seen['adamw'], seen['allreduce'], float(outs[-1]['train/loss']), float(outs[-1]['train/grad_norm'])))
  finally:
    dist.destroy_process_group()


def test_trainstate_freeze_slices_adamw_and_allreduce():
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
  norms = []
  for rank, b1, n, frozen_same, moved, sum_ok, adamw_seen, ar_seen, loss, gn in res:
    assert 0 < b1 < n
    assert frozen_same, f'rank {rank}: frozen parameters or moments changed'
    assert moved, f'rank {rank}: part of the trainable range did not move'
    assert sum_ok, f'rank {rank}: the trainable gradients are not the rank sum, or a frozen gradient was reduced'
    assert adamw_seen == [(n - b1,) * 4] * 3, adamw_seen
    # per step: buckets of 1000 floats that tile [b1, n) exactly, nothing below b1
    assert len(ar_seen) % 3 == 0
    per = ar_seen[:len(ar_seen) // 3]
    assert ar_seen == per * 3
    assert per[0][0] == b1 and all(a[0] + a[1] == b[0] for a, b in zip(per, per[1:])) and per[-1][0] + per[-1][1] == n, per
    assert all(cnt <= 1000 for _, cnt in per)
    assert loss == 3.0  # the loss scalars still ride along: 1 + 2
    norms.append(gn)
  assert norms[0] == norms[1] > 0
