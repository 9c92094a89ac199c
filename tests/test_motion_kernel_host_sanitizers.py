"""The refusals of spa3d_motion_kernel_sums, walked under AddressSanitizer + UndefinedBehaviorSanitizer by a stand-alone program with its own main
(tests/host/motion_kernel_host_walk.cpp; what it walks is told at the top of its source).  Built and run exactly as
tests/test_motion_knn_host_sanitizers.py builds its walk: host code only, no GPU, nothing preloaded, not through Python; csrc/motion.hip is
sanitised in place of its regular object, and that object is shared with the other walks."""
import importlib
import os
import subprocess

from test_host_sanitizers import ROOT, SAN, _build, run_driver


def test_motion_kernel_walk_under_asan_and_ubsan(tmp_path):
  objs = _build()
  b = importlib.import_module('3dspa_code_amd.build')
  asan = os.path.join(b.HERE, 'build', 'asan')
  src, obj = os.path.join(b.CSRC, 'motion.hip'), os.path.join(asan, 'motion.o')
  if b._stale(obj, [src] + b.HEADERS):
    r = subprocess.run([b._hipcc()] + [f for f in b.FLAGS if f != '-O3'] + ['-O1'] + SAN + ['-c', src, '-o', obj], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
  regular = os.path.join(b.HERE, 'build', 'motion.o')
  assert regular in objs
  objs = [obj if o == regular else o for o in objs]
  exe = os.path.join(asan, 'motion_kernel_host_walk')
  drv = os.path.join(ROOT, 'tests', 'host', 'motion_kernel_host_walk.cpp')
  cmd = [b._hipcc(), '--offload-arch=gfx950', '-x', 'hip'] + SAN + ['-O1', '-I', os.path.join(ROOT, 'include'), drv, '-x', 'none'] + objs + ['-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
  run_driver(exe, 'HOST_MOTION_KERNEL_OK', tmp_path)
