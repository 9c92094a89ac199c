"""The host orchestration of a training call under the "freeze" option, walked dry under AddressSanitizer + UndefinedBehaviorSanitizer by a stand-alone
program (tests/host/freeze_host_walk.cpp; what it walks is told at the top of its source).  Built and run as the drivers of tests/test_host_sanitizers.py
are: host code only, no GPU, the sanitised objects shared with them."""
import importlib
import os
import subprocess

from test_host_sanitizers import ROOT, SAN, _build, run_driver


def test_freeze_walk_under_asan_and_ubsan(tmp_path):
  objs = _build()
  b = importlib.import_module('3dspa_code_amd.build')
  exe = os.path.join(b.HERE, 'build', 'asan', 'freeze_host_walk')
  drv = os.path.join(ROOT, 'tests', 'host', 'freeze_host_walk.cpp')
  cmd = [b._hipcc(), '--offload-arch=gfx950', '-x', 'hip'] + SAN + ['-O1', '-I', os.path.join(ROOT, 'include'), drv, '-x', 'none'] + objs + ['-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
  run_driver(exe, 'HOST_FREEZE_OK', tmp_path)
