"""SURVEY.md 5 "ASAN on the host shim": the host code of libspa3d_hip.so -- csrc/model.hip and csrc/ops.hip (leaf tree, bump arena, the dry run
that sizes the workspace by executing the whole forward / backward orchestration with launches disabled) and the three stand-alone APIs that live
next to their kernels (csrc/tapvid3d.hip, csrc/render.hip, csrc/batch_build.hip) -- compiled with -fsanitize=address,undefined (host only:
-fno-gpu-sanitize; GPU sanitizers are not available on this pool) and driven through the C-ABI by plain C++ programs with their own main
(tests/host/spa3d_host_*.cpp).  Every entry validates its arguments and sizes its workspace before its first launch, so calls with a
zero-byte workspace, and every refusal, walk the orchestration without a GPU.  Nothing is preloaded; no GPU call is made; runs on the CPU box."""
import importlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAN = ['-fsanitize=address,undefined', '-fno-gpu-sanitize', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g']
# sanitised units: the network's orchestration in both precisions, each stand-alone API once; their regular objects stay out of the link
SANITISED = [('model.hip', True), ('ops.hip', True), ('tapvid3d.hip', False), ('render.hip', False), ('batch_build.hip', False)]
# driver (tests/host/spa3d_host_<name>.cpp) -> the token it prints when every CHECK held.  What each walks is told at the top of its source.
DRIVERS = {'dryrun': 'HOST_DRYRUN_OK',            # the five BASELINE.json shapes, the 2-D twin, the refused configurations
           'score': 'HOST_SCORE_OK',              # spa3d_score / spa3d_score_from_preds: need <= spa3d_workspace_bytes(train = 0), refusals
           'tapvid3d': 'HOST_TAPVID3D_OK',        # spa3d_tapvid3d_from_preds: need <= spa3d_tapvid3d_workspace_bytes, refusals
           'render': 'HOST_RENDER_OK',            # spa3d_render_tracks: need <= spa3d_render_workspace_bytes, refusals
           'build_batch': 'HOST_BUILD_BATCH_OK',  # spa3d_build_batch: every refusal, the bad clip beyond the first launch's 16
           'ragged': 'HOST_RAGGED_OK'}            # spa3d_set_counts: packed chunks, samples without queries, the count refusals of every entry


def _build():
  """The objects every driver links: the sanitised units (rebuilt when their source or any header of build.HEADERS is newer) and the regular rest."""
  b = importlib.import_module('3dspa_code_amd.build')
  b.build(verbose=False)
  out = os.path.join(b.HERE, 'build', 'asan')
  os.makedirs(out, exist_ok=True)
  flags = [f for f in b.FLAGS if f != '-O3'] + ['-O1'] + SAN
  jobs, objs = [], []
  for src, both in SANITISED:
    variants = [('', []), ('_f16', ['-DSPA_F16=1'])] if both else [('', [])]
    for suffix, extra in variants:
      obj = os.path.join(out, src.replace('.hip', suffix + '.o'))
      objs.append(obj)
      if b._stale(obj, [os.path.join(b.CSRC, src)] + b.HEADERS):
        jobs.append(subprocess.Popen([b._hipcc()] + flags + extra + ['-c', os.path.join(b.CSRC, src), '-o', obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
  for j in jobs:
    o, _ = j.communicate()
    assert j.returncode == 0, o[-3000:]
  skip = tuple(src[:-len('.hip')] for src, _ in SANITISED)
  return objs + [os.path.join(b.HERE, 'build', o) for o in sorted(os.listdir(os.path.join(b.HERE, 'build'))) if o.endswith('.o') and not o.startswith(skip)]


def build_driver(name):
  """tests/host/spa3d_host_<name>.cpp, sanitised, linked against the objects of _build(): the program's path."""
  objs = _build()
  b = importlib.import_module('3dspa_code_amd.build')
  exe = os.path.join(b.HERE, 'build', 'asan', 'spa3d_host_' + name)
  drv = os.path.join(ROOT, 'tests', 'host', f'spa3d_host_{name}.cpp')
  cmd = [b._hipcc(), '--offload-arch=gfx950', '-x', 'hip'] + SAN + ['-O1', '-I', os.path.join(ROOT, 'include'), drv, '-x', 'none'] + objs + ['-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
  return exe


def run_driver(exe, token, tmp_path):
  supp = tmp_path / 'lsan.supp'
  supp.write_text('leak:libamdhip64\nleak:libhsa-runtime64\nleak:libamd_comgr\nleak:librocprofiler\n')
  env = {k: v for k, v in os.environ.items() if not k.startswith('SPA3D_')}  # no option of the caller's shell reaches the handles
  env.update(ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1',
             LSAN_OPTIONS=f'suppressions={supp}:print_suppressions=0')
  r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
  print(r.stdout[-4000:], r.stderr[-4000:])
  assert r.returncode == 0 and token in r.stdout
  assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr and 'LeakSanitizer' not in r.stderr


def test_host_orchestration_dry_runs_under_asan_and_ubsan(tmp_path):
  run_driver(build_driver('dryrun'), DRIVERS['dryrun'], tmp_path)


@pytest.mark.parametrize('name', [n for n in DRIVERS if n != 'dryrun'])
def test_api_driver_dry_runs_under_asan_and_ubsan(name, tmp_path):
  run_driver(build_driver(name), DRIVERS[name], tmp_path)


def test_every_driver_source_is_run():
  have = {f[len('spa3d_host_'):-len('.cpp')] for f in os.listdir(os.path.join(ROOT, 'tests', 'host')) if f.startswith('spa3d_host_')}
  assert have == set(DRIVERS)
