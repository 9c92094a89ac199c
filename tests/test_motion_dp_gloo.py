"""MotionStats.all_reduce at world size 2 over gloo, on the CPU (the pattern of tests/test_adamw_groups_dp_gloo.py): each rank holds a different
hand-built state, the reduction is an int64 SUM, and both ranks end with the same bits -- those of one state built from both ranks' clips.  The
entries are large enough (beyond 2^53) that a sum taken in floating point would not give them."""
import os
import traceback

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import motion_util as MU
from test_dp_gloo import _free_port

D, L = 6, 5
BIG = (1 << 60) + 12345   # an entry only integer addition keeps: BIG + BIG + 1 is not a float64


def _rank_codes(rank):
  return np.random.default_rng(40 + rank).integers(-128, 129, (3 + rank, L, D)).astype(np.int16)


def _rank_state(rank, pool):
  st = torch.from_numpy(MU.moments(_rank_codes(rank), pool))
  st[1 + D + 7] += BIG + rank
  return st


def _scenario(rank, world):
  import spa3d
  out = {}
  for name, pool in (('token', MU.TOKEN), ('clip', MU.CLIP)):
    s = spa3d.MotionStats(D, L, name).load_state_dict({'D': D, 'L': L, 'pool': name, 'state': _rank_state(rank, pool)})
    assert s.n == ((3 + rank) * L if name == 'token' else 3 + rank)
    assert s.all_reduce() is s
    want = sum(_rank_state(r, pool) for r in range(world))
    assert torch.equal(s.state, want) and s.state.dtype == torch.int64, f'rank {rank} {name}'
    assert s.n == int(want[0]) == sum((3 + r) * (L if name == 'token' else 1) for r in range(world))
    if world == 2:   # apart from the planted entry, the state of both ranks' clips in one update
      both = torch.from_numpy(MU.moments(np.concatenate([_rank_codes(0), _rank_codes(1)]), pool))
      both[1 + D + 7] += 2 * BIG + 1
      assert torch.equal(s.state, both)
      assert int(float(2 * BIG + 1)) != 2 * BIG + 1   # the planted sum is not a float64: only integer addition gives it
    out[name] = s.state.clone()
  return out


def _worker(rank, world, port, q):
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  dist.init_process_group('gloo', rank=rank, world_size=world)
  torch.set_num_threads(2)
  try:
    res = _scenario(rank, world)
    q.put((rank, 'ok', res['token'].numpy(), res['clip'].numpy()))
  except BaseException:
    q.put((rank, traceback.format_exc(), None, None))
  finally:
    dist.destroy_process_group()


def test_all_reduce_without_a_group_is_a_no_op():
  res = _scenario(0, 1)
  assert torch.equal(res['token'], _rank_state(0, MU.TOKEN))


def test_all_reduce_world_size_2_gloo_gives_both_ranks_the_integer_sum():
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
  for rank, status, _, _ in res:
    assert status == 'ok', f'rank {rank}:\n{status}'
  assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])   # every rank holds the same bits
  assert int(res[0][2][1 + D + 7]) - int(MU.moments(np.concatenate([_rank_codes(0), _rank_codes(1)]), MU.TOKEN)[1 + D + 7]) == 2 * BIG + 1
