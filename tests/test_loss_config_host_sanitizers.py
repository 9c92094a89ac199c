"""The host code of the configurable objective under AddressSanitizer + UndefinedBehaviorSanitizer: tests/host/loss_config_host.cpp, a plain
C++ program with its own main, linked against the sanitised objects that tests/test_host_sanitizers.py builds.  It walks a train call with a
configuration and a weight plane at zero workspace, a packed ragged call, a query-chunked call and every refusal.  Nothing is preloaded; no GPU
call is made."""
import importlib
import os
import subprocess

from test_host_sanitizers import ROOT, SAN, _build, run_driver


def test_loss_config_driver_is_clean_under_asan_and_ubsan(tmp_path):
  objs = _build()
  b = importlib.import_module('3dspa_code_amd.build')
  exe = os.path.join(b.HERE, 'build', 'asan', 'loss_config_host')
  drv = os.path.join(ROOT, 'tests', 'host', 'loss_config_host.cpp')
  cmd = [b._hipcc(), '--offload-arch=gfx950', '-x', 'hip'] + SAN + ['-O1', '-I', os.path.join(ROOT, 'include'), drv, '-x', 'none'] + objs + ['-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
  run_driver(exe, 'HOST_LOSS_CONFIG_OK', tmp_path)
