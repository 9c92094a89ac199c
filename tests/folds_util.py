"""Helpers shared by the spa3d_score_folds tests (tests/test_score_folds_api_host.py, tests/test_gpu_score_folds.py): the batch a fold call takes, the
compacted leave-out batch that defines its result, and the list of refusals of include/spa3d.h with the call that provokes each."""
import ctypes as C

import torch

SUPPORT_KEYS = ('support_tracks', 'support_tracks_visible', 'dino_features', 'depth_features')


def fold_batch(batch, seed=5):
  """A batch for score_all from a synthetic one: the support keys and boundary_frame, and query_points [B,N,4] = every track at a random frame
  (frame, its own position there).  No targets: they default to the support tensors."""
  st = batch['support_tracks']
  B, N, T = st.shape[:3]
  qf = torch.randint(0, T, (B, N), generator=torch.Generator().manual_seed(seed)).to(st.device)
  pos = torch.gather(st.float(), 2, qf[:, :, None, None].expand(B, N, 1, 3))[:, :, 0]
  out = {k: batch[k] for k in SUPPORT_KEYS + ('boundary_frame',) if k in batch}
  out['query_points'] = torch.cat([qf[..., None].float(), pos], dim=-1)
  return out, qf.to(torch.int32)


def leave_out(batch, b, lo, hi):
  """What rows [lo, hi) of clip b are defined by: the single-sample batch whose support tracks are the clip's tracks outside [lo, hi), in their order,
  whose queries are the rows of that range, and whose targets are those tracks themselves."""
  keep = lambda t: torch.cat([t[b, :lo], t[b, hi:]])[None].contiguous()
  out = {k: keep(batch[k]) for k in SUPPORT_KEYS if k in batch}
  out['boundary_frame'] = batch['boundary_frame'][b:b + 1]
  out['query_points'] = batch['query_points'][b:b + 1, lo:hi].contiguous()
  out['query_tracks'] = batch['support_tracks'][b:b + 1, lo:hi].contiguous()
  out['query_tracks_visible'] = batch['support_tracks_visible'][b:b + 1, lo:hi].contiguous()
  return out


def i32(values):
  return (C.c_int32 * len(values))(*[int(v) for v in values])


def check_refusals(spa3d, h, h2d, make_batch, make_scores, N, T, ws_ptr, ws_bytes, params_ptr):
  """Every refusal of spa3d_score_folds (include/spa3d.h), each with its message; nothing is launched by any of them, so the pointers may be fake.
  h: a model_kind 0 handle whose num_output_frames is T; h2d: a model_kind 1 handle; make_batch() / make_scores(): fresh valid blocks
  (B = 2, Q = N, NULL targets) for h.  Returns the number of refusals checked."""
  lib = spa3d._lib.load()
  off = spa3d.fold_offsets(N, 3)
  n = [0]

  def refused(word, handle=h, b=None, F=3, fo=None, sc=None, ws=ws_ptr, wb=ws_bytes, code=1):
    b = make_batch() if b is None else b
    sc = make_scores() if sc is None else sc
    rc = lib.spa3d_score_folds(handle, params_ptr, C.byref(b), F, i32(off if fo is None else fo), C.byref(sc), None, ws, wb, None)
    msg = lib.spa3d_last_error(handle).decode()
    assert rc == code and word in msg, (word, rc, msg)
    n[0] += 1

  b = make_batch(); b.Q = N - 1
  refused('Q == N', b=b)
  refused('num_folds', F=1, fo=[0, N])
  refused('num_folds', F=65, fo=list(range(65)) + [N])
  refused('start at 0', fo=[1, 5, 9, N])
  refused('end at N', fo=[0, 5, 9, N - 1])
  refused('strictly increasing', fo=[0, 9, 9, N])
  refused('strictly increasing', fo=[0, 9, 5, N])
  b = make_batch(); b.T = T - 1
  refused('num_output_frames', b=b)
  b = make_batch(); b.query_tracks, b.query_tracks_visible = b.support_tracks, b.support_tracks_visible   # (the 2-D model has its own target width: explicit)
  refused('model_kind 1', handle=h2d, b=b)
  assert lib.spa3d_set_counts(h, 2, i32([N, N - 1]), None) == 0
  refused('counts')
  assert lib.spa3d_set_counts(h, 0, None, None) == 0
  for opt in (b'track_chunk', b'query_chunk'):
    assert lib.spa3d_set_option(h, opt, 16.0) == 0
    refused('chunk')
    assert lib.spa3d_set_option(h, opt, 0.0) == 0
  need = lib.spa3d_score_folds_workspace_bytes(h, N, T, 3)
  assert 0 < need <= ws_bytes
  refused(f'need {need} bytes', wb=need - 1)
  refused(f'need {need} bytes', ws=None)
  sc = make_scores(); sc.query_stats = None
  refused('query_stats', sc=sc)
  sc = make_scores(); sc.num_thresholds = 9
  refused('num_thresholds', sc=sc)
  sc = make_scores(); sc.num_thresholds = 2; sc.thresholds[0], sc.thresholds[1] = 0.5, float('nan')
  refused('thresholds[1]', sc=sc)
  b = make_batch(); b.query_tracks = b.support_tracks   # one target without the other
  refused('targets', b=b)
  # the sizing function refuses what the call refuses
  assert lib.spa3d_score_folds_workspace_bytes(h, N, T, 1) == -1 and lib.spa3d_score_folds_workspace_bytes(h, N, T, 65) == -1
  assert lib.spa3d_score_folds_workspace_bytes(h, 2, T, 3) == -1 and lib.spa3d_score_folds_workspace_bytes(h2d, N, T, 3) == -1
  return n[0]
