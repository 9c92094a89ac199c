"""Workspace need of the model calls over a table of shapes and options, one line each.  Needs no GPU: spa3d_workspace_bytes and
spa3d_score_folds_workspace_bytes walk the orchestration with launches off, and a ragged call (spa3d_set_counts) given a zero-byte workspace is
refused with the bytes its first chunk size needs before anything is launched.  Prints, asserts nothing: diff the output of two commits to see
whether a change of the host sequencing moved any need.

  python tools/ws_table.py > table.txt"""
import ctypes as C
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spa3d  # noqa: E402

L = spa3d._lib
lib = L.load()
FAKE = 0x100000  # never dereferenced: every call below returns before its first launch
SHAPES = [(8, 64, 16), (150, 2048, 512), (300, 8192, 2048)]  # (T, N, Q)
RAGGED = {'uniform': [(300, 96)] * 3, 'full': [(300, 96), (117, 40), (64, 1)], 'full_q0': [(300, 96), (117, 0), (64, 1)],
          'alone_q0': [(117, 0), (300, 96), (64, 1)]}


def handle(precision, twin=False):
  if twin:
    return spa3d.TrackAutoEncoder(precision=precision)._handle(0, 0)[0]
  return spa3d.TrackAutoEncoder3D(precision=precision, dino_feature_dim=768, depth_feature_dim=1)._handle(768, 1)[0]


def opt(h, **kw):
  for k, v in kw.items():
    assert lib.spa3d_set_option(h, k.encode(), float(v)) == 0, (k, v)


def refused_need(h, B, N, Q, T, train, feats):
  """The 'need N bytes for chunk K' of a call with a zero-byte workspace."""
  b = L.Batch(B, N, Q, T, FAKE, FAKE, FAKE, FAKE, FAKE if feats else None, FAKE if feats else None, FAKE, 1, FAKE, FAKE)
  out = L.Outputs(FAKE, FAKE, FAKE, FAKE)
  if train:
    lib.spa3d_loss_and_grads(h, FAKE, C.byref(b), 0.0, FAKE, 0, FAKE, C.byref(out), FAKE, 0, None)
  else:
    lib.spa3d_forward(h, FAKE, C.byref(b), C.byref(out), FAKE, 0, None)
  m = re.search(r'need (\d+) bytes for chunk (\d+)', lib.spa3d_last_error(h).decode())
  return (int(m.group(1)), int(m.group(2))) if m else (-1, -1)


def main():
  models = [(p, False) for p in ('fp32', 'bf16', 'fp16')] + [('bf16', True)]
  for precision, twin in models:
    h = handle(precision, twin)
    tag = f'{precision}{"/2d" if twin else ""}'
    for T, N, Q in SHAPES:
      for train in (1, 0):
        for chunk in (1, 4, 9):
          print(f'{tag} T={T} N={N} Q={Q} train={train} B=9 chunk={chunk}: {lib.spa3d_workspace_bytes(h, 9, N, Q, T, chunk, train)}')
        for qc in (0, 256, Q):
          for tc in (0, 1024):
            opt(h, query_chunk=qc, track_chunk=tc)
            print(f'{tag} T={T} N={N} Q={Q} train={train} B=9 chunk=1 query_chunk={qc} track_chunk={tc}: {lib.spa3d_workspace_bytes(h, 9, N, Q, T, 1, train)}')
        opt(h, query_chunk=0, track_chunk=0)
    if twin:
      continue
    for name, counts in RAGGED.items():
      n = (C.c_int32 * 3)(*[c[0] for c in counts])
      q = (C.c_int32 * 3)(*[c[1] for c in counts])
      assert lib.spa3d_set_counts(h, 3, n, q) == 0
      for train in (1, 0):
        for chunk in (0, 1, 2, 3):
          opt(h, chunk=chunk)
          need, at = refused_need(h, 3, 300, 96, 150, train, True)
          print(f'{tag} ragged {name} T=150 N=300 Q=96 train={train} B=3 chunk={chunk}: {need} (chunk {at})')
      opt(h, chunk=0)
    assert lib.spa3d_set_counts(h, 0, None, None) == 0
    for N in (300, 4096):
      for F in (2, 8, 64):
        print(f'{tag} score_folds T=150 N={N} F={F}: {lib.spa3d_score_folds_workspace_bytes(h, N, 150, F)}')


if __name__ == '__main__':
  main()
