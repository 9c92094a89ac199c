"""bench.py's own N-rank launcher (`python bench.py --gpus N`, as the driver invokes it) on a CPU-only host: --launch-check makes every
rank join a gloo group and exit before any GPU call.  BASELINE.json configs[3] (no reference counterpart: SURVEY 2, no multi-device code)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=300):
  env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
  env.update(env_extra or {})
  return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_plain_invocation_spawns_n_ranks():
  r = _run(['--gpus', '2', '--launch-check'])
  assert r.returncode == 0, r.stderr[-2000:]
  lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
  assert len(lines) == 1, r.stdout  # rank 0 only
  j = json.loads(lines[0])
  assert j['launch_check'] is True and j['n_gpus'] == 2 and j['ranks_verified'] == 2 and j['requested_gpus'] == 2


def test_single_rank_launch_check():
  r = _run(['--gpus', '1', '--launch-check'])
  assert r.returncode == 0, r.stderr[-2000:]
  assert json.loads(r.stdout.strip().splitlines()[-1])['n_gpus'] == 1


def test_world_size_mismatch_is_refused():
  # a torchrun-style environment of the wrong size must not produce a number
  r = _run(['--gpus', '4', '--launch-check'], env_extra={'WORLD_SIZE': '1', 'RANK': '0', 'LOCAL_RANK': '0'})
  assert r.returncode == 2 and 'refusing' in r.stderr
  assert not [l for l in r.stdout.splitlines() if l.startswith('{')]


def test_config5_argument_path_and_whole_step_hbm_fields():
  """BASELINE.json configs[4] is reachable from the driver's command (`bench.py --config 5 [--batch B]`), and the whole-step HBM figure comes
  from the committed PMC passes with their round tag (a warning field when they are older than the round this tree is built in)."""
  sys.path.insert(0, ROOT)
  import bench
  c5 = bench.CONFIGS[5]
  assert (c5['N'], c5['Q'], c5['T'], c5['dino'], c5['depth'], c5['precision']) == (8192, 2048, 300, 768, 1, 'fp16') and c5['B'] >= 1
  r = _run(['--gpus', '1', '--config', '5', '--batch', '2', '--launch-check'])
  assert r.returncode == 0, r.stderr[-2000:]
  r = _run(['--gpus', '1', '--config', '4', '--launch-check'])
  assert r.returncode != 0  # configs[3] is --gpus 8 of config 3, not a config of its own
  rows, src, tag, warn = bench.pmc_tables()
  assert rows and tag and src.startswith('profiles/' + tag)
  by = bench.pmc_step_bytes(rows)
  assert 1e12 < by < 2e13  # TB per step: the activations of every op round-trip through HBM
  assert (warn is None) == (int(tag[1:]) >= bench.current_round())
  assert 'embed' in bench.CLASS_INFO


def test_dump_outputs_whole_and_sampled(tmp_path):
  """--dump-outputs: the metrics and the four parameter-sized vectors of the state, float32 / float64, within the 64 MB budget; a state too large for
  the budget is written as the same seeded sample of positions from each vector, identical from call to call."""
  import types
  import numpy as np
  import torch
  sys.path.insert(0, ROOT)
  import bench
  metrics = {'train/loss': torch.tensor(1.5), 'train/learning_rate': 1e-4, 'train/grad_norm': torch.tensor(2.0)}

  def state(n):
    g = torch.Generator().manual_seed(n)
    return types.SimpleNamespace(**{k: torch.randn(n, generator=g) for k in ('flat', 'grads', 'm', 'v')})

  small = state(1000)
  names, nbytes = bench.dump_outputs(str(tmp_path / 'small'), small, metrics)
  assert 'sample_index' not in names and nbytes <= bench.DUMP_BUDGET
  assert np.array_equal(np.load(tmp_path / 'small' / 'grads.npy'), small.grads.numpy())
  assert float(np.load(tmp_path / 'small' / 'train_loss.npy')) == 1.5

  n = bench.DUMP_BUDGET // 16 + 1  # four fp32 vectors one element over the budget
  big = state(n)
  for d in ('a', 'b'):
    names, nbytes = bench.dump_outputs(str(tmp_path / d), big, metrics)
    assert 'sample_index' in names and nbytes <= bench.DUMP_BUDGET
  total = 0
  for f in os.listdir(tmp_path / 'a'):
    a, b = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
    assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
    total += os.path.getsize(tmp_path / 'a' / f)
  assert total <= bench.DUMP_BUDGET
  idx = np.load(tmp_path / 'a' / 'sample_index.npy').astype(np.int64)
  assert np.all(np.diff(idx) > 0) and idx[-1] < n
  assert np.array_equal(np.load(tmp_path / 'a' / 'adam_v.npy'), big.v.numpy()[idx])


def test_steps_must_be_positive():
  r = _run(['--gpus', '1', '--steps', '0', '--launch-check'])
  assert r.returncode == 2 and '--steps' in r.stderr
