"""The refusals and the workspace sizing of spa3d_render_heatmap, walked under AddressSanitizer + UndefinedBehaviorSanitizer by a stand-alone
program with its own main (tests/host/heatmap_host_walk.cpp; what it walks is told at the top of its source).  Built and run as the drivers of
tests/test_host_sanitizers.py are: host code only, no GPU, nothing preloaded; the sanitised objects are shared with them, and csrc/heatmap.hip
is sanitised here in place of its regular object."""
import importlib
import os
import subprocess

from test_host_sanitizers import ROOT, SAN, _build, run_driver


def test_heatmap_walk_under_asan_and_ubsan(tmp_path):
  objs = _build()
  b = importlib.import_module('3dspa_code_amd.build')
  asan = os.path.join(b.HERE, 'build', 'asan')
  src, obj = os.path.join(b.CSRC, 'heatmap.hip'), os.path.join(asan, 'heatmap.o')
  if b._stale(obj, [src] + b.HEADERS):
    r = subprocess.run([b._hipcc()] + [f for f in b.FLAGS if f != '-O3'] + ['-O1'] + SAN + ['-c', src, '-o', obj], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
  regular = os.path.join(b.HERE, 'build', 'heatmap.o')
  assert regular in objs
  objs = [obj if o == regular else o for o in objs]
  exe = os.path.join(asan, 'heatmap_host_walk')
  drv = os.path.join(ROOT, 'tests', 'host', 'heatmap_host_walk.cpp')
  cmd = [b._hipcc(), '--offload-arch=gfx950', '-x', 'hip'] + SAN + ['-O1', '-I', os.path.join(ROOT, 'include'), drv, '-x', 'none'] + objs + ['-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
  run_driver(exe, 'HOST_HEATMAP_OK', tmp_path)
