"""Helpers of the ragged-batch tests (tests/test_ragged_host.py, tests/test_gpu_ragged.py): cropping a padded batch to one sample's live rows,
filling the padding, and the expected values of a ragged call built from per-sample runs.

The expected-value construction (include/spa3d.h, spa3d_set_counts): outputs of sample b are those of the sample run alone, cropped to
(n_b, q_b); loss and gradients are the SUM over the samples of single-sample runs that all use the common denominator
D = max(sum of query_tracks_visible over the live queries of the whole batch, 1)."""
import torch

SUPPORT_KEYS = ('support_tracks', 'support_tracks_visible', 'dino_features', 'depth_features')
QUERY_KEYS = ('query_points', 'query_tracks', 'query_tracks_visible')


def crop(batch, b, n, q):
  """Sample b alone with its first n support tracks and first q queries (a batch of one)."""
  out = {}
  for k, v in batch.items():
    if k in ('support_count', 'query_count'):
      continue
    if k in SUPPORT_KEYS:
      out[k] = v[b:b + 1, :n].contiguous()
    elif k in QUERY_KEYS:
      out[k] = v[b:b + 1, :q].contiguous()
    else:
      out[k] = v[b:b + 1].contiguous()
  return out


def fill_padding(batch, counts, value):
  """A copy of the batch whose rows at or beyond the counts hold `value` in every support / query tensor."""
  out = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
  for b, (n, q) in enumerate(counts):
    for k in SUPPORT_KEYS:
      if k in out:
        out[k][b, n:] = value
    for k in QUERY_KEYS:
      if k in out:
        out[k][b, q:] = value
  return out


def live_visible(batch, counts):
  return float(sum(batch['query_tracks_visible'][b, :q].double().sum() for b, (n, q) in enumerate(counts)))


def per_sample_sum(run_one, batch, counts, noise, denom=None):
  """run_one(cropped_batch, noise_b, denom) -> (loss dict, preds, grads dict).  Returns (summed loss dict, list of per-sample preds,
  summed grads dict, D)."""
  D = max(live_visible(batch, counts), 1.0) if denom is None else denom
  loss, grads, preds = None, None, []
  for b, (n, q) in enumerate(counts):
    ld, p, g = run_one(crop(batch, b, n, q), noise[b:b + 1], D)
    preds.append(p)
    loss = {k: v.clone() for k, v in ld.items()} if loss is None else {k: loss[k] + ld[k] for k in loss}
    grads = {k: v.clone() for k, v in g.items()} if grads is None else {k: grads[k] + g[k] for k in grads}
  return loss, preds, grads, D
