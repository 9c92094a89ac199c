"""spa3d_build_batch's refusals walked on the CPU under AddressSanitizer + UndefinedBehaviorSanitizer: tests/host/spa3d_host_build_batch.cpp linked
against the sanitised host orchestration that tests/test_host_sanitizers.py builds (the entry lives in csrc/model.hip).  The entry checks every
clip before its first launch, so each refused call -- a missing pointer, counts above N or Q, a clip without support tracks or longer than the
batch, a map and a pool for one feature, a feature the handle or the batch does not have, a lift without a depth map, the 2-D model -- returns
SPA3D_ERR_ARG with a message and launches nothing; the bad clip is the 20th of 20, beyond the first launch's 16."""
import importlib
import os
import subprocess

import test_host_sanitizers as ths

ROOT = ths.ROOT


def test_build_batch_refusals_under_asan_and_ubsan(tmp_path):
  ths._build()  # the sanitised model / ops objects and the regular kernel objects
  b = importlib.import_module('3dspa_code_amd.build')
  out = os.path.join(b.HERE, 'build', 'asan')
  san = ['-fsanitize=address,undefined', '-fno-gpu-sanitize', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g']
  regular = [os.path.join(b.HERE, 'build', o) for o in sorted(os.listdir(os.path.join(b.HERE, 'build')))
             if o.endswith('.o') and not o.startswith(('model', 'ops'))]
  exe = os.path.join(out, 'spa3d_host_build_batch')
  drv = os.path.join(ROOT, 'tests', 'host', 'spa3d_host_build_batch.cpp')
  cmd = [b._hipcc(), '--offload-arch=gfx950', '-x', 'hip'] + san + ['-O1', '-I', os.path.join(ROOT, 'include'), drv, '-x', 'none'] + \
        [os.path.join(out, o) for o in ('model.o', 'model_f16.o', 'ops.o', 'ops_f16.o')] + regular + ['-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
  supp = tmp_path / 'lsan.supp'
  supp.write_text('leak:libamdhip64\nleak:libhsa-runtime64\nleak:libamd_comgr\nleak:librocprofiler\n')
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1',
             LSAN_OPTIONS=f'suppressions={supp}:print_suppressions=0')
  for k in ('SPA3D_GEMM_IMPL', 'SPA3D_ATTN_IMPL', 'SPA3D_PRUNE', 'SPA3D_RO_SHARE', 'SPA3D_CHUNK', 'SPA3D_LOSS_SCALE', 'SPA3D_QUERY_CHUNK', 'SPA3D_TRACK_CHUNK'):
    env.pop(k, None)
  r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
  print(r.stdout[-4000:], r.stderr[-4000:])
  assert r.returncode == 0 and 'HOST_BUILD_BATCH_OK' in r.stdout
  assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr and 'LeakSanitizer' not in r.stderr
