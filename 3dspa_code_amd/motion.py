"""Latent-set metrics on the integer codes of the bottleneck (include/spa3d.h, "Latent-set metrics": the library's own definitions, the
reference has no counterpart).  The device work is csrc/motion.hip -- codes, exact integer moments, exact integer pairwise distances, and the
streaming k-NN, ball hits and kernel sums that reduce those products tile by tile; what is left here is plumbing: the moment state and its
merges, the Frechet distance in float64 NumPy, the k-NN precision / recall selection on the matrix route, the counts-to-ratios of
manifold_metrics, and the exact rationals of kernel_distance."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import torch

from . import _lib

CODE_MAX = 128          # |code| <= 128 (csrc/motion_code.hpp)
MAX_L, MAX_D, MAX_E = 4096, 256, 32767
POOLS = {'token': _lib.POOL_TOKEN, 'clip': _lib.POOL_CLIP}
KINDS = {'dot': _lib.PDIST_DOT, 'sqdist': _lib.PDIST_SQDIST}

_MOTION_HANDLE = []


def _motion_handle():
  """A handle of the motion calls' own: they use it for the error message and the stream only, and must not reset those of a handle a model
  is using."""
  if not _MOTION_HANDLE:
    from .model import TrackAutoEncoder3D
    _MOTION_HANDLE.append(TrackAutoEncoder3D(num_output_frames=8, use_dino=False, use_depth=False, precision='fp32'))  # the model owns its handles
  return _MOTION_HANDLE[0]._handle(0, 0)[0]


def _on_device(t, name, what):
  if not isinstance(t, torch.Tensor):
    raise ValueError(f'{name} must be a tensor')
  if t.device.type != 'cuda':
    raise _lib.Spa3dError(f'{what} runs on the GPU: the 3DSPA hot path is HIP-only (no CPU fallback)')


def _stream(t):
  return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _codes_arg(codes, name, what):
  _on_device(codes, name, what)
  if codes.dtype != torch.int16:
    raise ValueError(f'{name} must be int16 codes (motion_codes), got {codes.dtype}')
  return codes.contiguous()


# ------------------------------------------------------------------------------------------------ codes
def motion_codes(latents):
  """The integer codes of latents the caller already has (spa3d_motion_codes): c = rint(clip(x, -1, 1) * 128) as int16, the shape of the input.
  ValueError when a latent is NaN (it has no code)."""
  _on_device(latents, 'latents', 'motion_codes')
  lat = latents.to(torch.float32).contiguous()
  codes = torch.empty(lat.shape, dtype=torch.int16, device=lat.device)
  bad = torch.empty(1, dtype=torch.int32, device=lat.device)
  h = _motion_handle()
  with torch.cuda.device(lat.device):
    _lib.check(_lib.load().spa3d_motion_codes(h, lat.data_ptr(), lat.numel(), codes.data_ptr(), bad.data_ptr(), _stream(lat)), h, 'spa3d_motion_codes')
  nbad = int(bad.item())
  if nbad > 0:
    raise ValueError(f'{nbad} of {lat.numel()} latents are NaN: they have no code')
  return codes


# ------------------------------------------------------------------------------------------------ moments
def samples_max(L: int, pool: str) -> int:
  """the largest sample count whose integer sums cannot pass 2^62 (mc_samples_max of csrc/motion_code.hpp): n * 2^14 (token pool) or
  n * (128 L)^2 (clip pool) stays at or below 2^62"""
  return (1 << 62) // (CODE_MAX * CODE_MAX if pool == 'token' else (CODE_MAX * L) ** 2)


class MotionStats:
  """Count, sum and sum of outer products of D-dimensional latent samples, as exact integers: one int64 tensor [1 + D + D * D] = n, s, S
  (spa3d_motion_moments_add adds into it).  pool='token': every token row of every clip is a sample (x = c / 128); pool='clip': every clip's
  mean token (x = sum_l c[l] / (128 L)).  The state is the same bits however the clips were batched, and two states merge by integer addition
  (merge, all_reduce).  n, mean and cov are float64 on the host, in latent units; cov is the biased S / n - mu mu^T."""

  def __init__(self, D: int, L: int, pool: str = 'clip'):
    if pool not in POOLS:
      raise ValueError(f'pool must be one of {sorted(POOLS)}, got {pool!r}')
    for name, v, hi in (('D', D, MAX_D), ('L', L, MAX_L)):
      if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 or v > hi:
        raise ValueError(f'{name} = {v!r} is outside [1, {hi}]')
    self.D, self.L, self.pool = int(D), int(L), pool
    self.state = torch.zeros(1 + self.D + self.D * self.D, dtype=torch.int64)
    self._n = 0   # tracked on the host: update() needs no read-back

  # ---- sizes
  @property
  def n(self) -> int:
    return self._n

  @property
  def divisor(self) -> int:
    """codes per latent unit of one sample coordinate"""
    return CODE_MAX if self.pool == 'token' else CODE_MAX * self.L

  def _check_n(self, n):
    if n > samples_max(self.L, self.pool):
      raise OverflowError(f'{n} samples of the {self.pool} pool (L = {self.L}) could carry a sum past 2^62; the limit is {samples_max(self.L, self.pool)}')

  # ---- adding samples
  def update(self, codes):
    """codes: int16 device tensor [M, L, D] (motion_codes).  Adds its samples into the state, which moves to the codes' device."""
    codes = _codes_arg(codes, 'codes', 'MotionStats.update')
    if codes.dim() != 3 or tuple(codes.shape[1:]) != (self.L, self.D) or codes.shape[0] < 1:
      raise ValueError(f'codes must be [M >= 1, L = {self.L}, D = {self.D}], got {tuple(codes.shape)}')
    M = int(codes.shape[0])
    self._check_n(self._n + (M * self.L if self.pool == 'token' else M))
    if self.state.device != codes.device:
      self.state = self.state.to(codes.device)
    h = _motion_handle()
    with torch.cuda.device(codes.device):
      _lib.check(_lib.load().spa3d_motion_moments_add(h, codes.data_ptr(), M, self.L, self.D, POOLS[self.pool], self.state.data_ptr(), _stream(codes)),
                 h, 'spa3d_motion_moments_add')
    self._n += M * self.L if self.pool == 'token' else M
    return self

  def _same_kind(self, other):
    if not isinstance(other, MotionStats) or (other.D, other.L, other.pool) != (self.D, self.L, self.pool):
      raise ValueError(f'statistics of another kind: D, L, pool = {(self.D, self.L, self.pool)} here')

  def merge(self, other):
    """adds another state of the same D, L and pool: integer addition, equal to one state updated with both sets of clips"""
    self._same_kind(other)
    self._check_n(self._n + other._n)
    self.state += other.state.to(self.state.device)
    self._n += other._n
    return self

  def all_reduce(self, group=None):
    """int64 SUM over the process group: every rank ends with the same bits.  Without an initialised process group: nothing to do."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
      dist.all_reduce(self.state, op=dist.ReduceOp.SUM, group=group)
      self._n = int(self.state[0].item())
      self._check_n(self._n)
    return self

  # ---- persistence
  def state_dict(self):
    return {'D': self.D, 'L': self.L, 'pool': self.pool, 'state': self.state.detach().cpu().clone()}

  def load_state_dict(self, sd):
    state = torch.as_tensor(np.asarray(sd['state'])) if not isinstance(sd['state'], torch.Tensor) else sd['state']
    if (int(sd['D']), int(sd['L']), str(sd['pool'])) != (self.D, self.L, self.pool):
      raise ValueError(f'state of another kind: D, L, pool = {(int(sd["D"]), int(sd["L"]), str(sd["pool"]))}, here {(self.D, self.L, self.pool)}')
    if state.dtype != torch.int64 or tuple(state.shape) != (1 + self.D + self.D * self.D,):
      raise ValueError(f'state must be int64 [{1 + self.D + self.D * self.D}], got {state.dtype} {tuple(state.shape)}')
    n = int(state[0].item())
    if n < 0:
      raise ValueError(f'state holds a negative count {n}')
    self._check_n(n)
    self.state = state.detach().clone().to(self.state.device)
    self._n = n
    return self

  def save(self, path):
    sd = self.state_dict()
    np.savez(path, D=np.int64(sd['D']), L=np.int64(sd['L']), pool=np.str_(sd['pool']), state=sd['state'].numpy())
    return path if str(path).endswith('.npz') else str(path) + '.npz'

  @classmethod
  def load(cls, path):
    z = np.load(path)
    return cls(int(z['D']), int(z['L']), str(z['pool'])).load_state_dict({'D': z['D'], 'L': z['L'], 'pool': str(z['pool']), 'state': z['state']})

  # ---- the statistics, float64 on the host
  def _host(self):
    if self._n < 1:
      raise ValueError('no samples yet')
    st = self.state.detach().cpu().numpy()
    D = self.D
    return st[1:1 + D].astype(np.float64), st[1 + D:].reshape(D, D).astype(np.float64)

  @property
  def mean(self):
    s, _ = self._host()
    return s / (float(self._n) * self.divisor)

  @property
  def cov(self):
    s, S = self._host()
    mu = s / (float(self._n) * self.divisor)
    return S / (float(self._n) * float(self.divisor) ** 2) - np.outer(mu, mu)


def _mean_cov(x):
  if isinstance(x, MotionStats):
    return x.mean, x.cov
  mu, cov = x
  mu, cov = np.asarray(mu, np.float64), np.asarray(cov, np.float64)
  if mu.ndim != 1 or cov.shape != (mu.shape[0], mu.shape[0]):
    raise ValueError(f'statistics must be (mean [D], cov [D, D]), got {mu.shape} and {cov.shape}')
  return mu, cov


def frechet_distance(a, b) -> float:
  """The Frechet distance of two Gaussians with the statistics a and b (MotionStats, or (mean, cov) pairs), as include/spa3d.h states it:
      |mu_a - mu_b|^2 + tr Sigma_a + tr Sigma_b - 2 sum_i sqrt(max(lambda_i, 0)),
  lambda the eigenvalues of R Sigma_b R, R the symmetric square root of Sigma_a (eigh, negative eigenvalues clipped to 0).  R Sigma_b R is
  symmetric positive semi-definite and has the eigenvalues of Sigma_a Sigma_b, so no general matrix square root is needed.  float64 NumPy."""
  mu_a, cov_a = _mean_cov(a)
  mu_b, cov_b = _mean_cov(b)
  if mu_a.shape != mu_b.shape:
    raise ValueError(f'statistics of {mu_a.shape[0]} and {mu_b.shape[0]} dimensions')
  w, V = np.linalg.eigh((cov_a + cov_a.T) * 0.5)
  R = (V * np.sqrt(np.maximum(w, 0.0))) @ V.T
  G = R @ ((cov_b + cov_b.T) * 0.5) @ R
  lam = np.linalg.eigvalsh((G + G.T) * 0.5)
  d = mu_a - mu_b
  return float(d @ d + np.trace(cov_a) + np.trace(cov_b) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


# ------------------------------------------------------------------------------------------------ pairwise distances
def _flat_codes(codes, name):
  codes = _codes_arg(codes, name, 'motion_pdist')
  if codes.dim() < 2 or codes.shape[0] < 1:
    raise ValueError(f'{name} must be [M >= 1, ...], got {tuple(codes.shape)}')
  return codes.reshape(codes.shape[0], -1)


def motion_pdist(codes_a, codes_b=None, kind='sqdist'):
  """All pairwise integer distances of two sets of codes (spa3d_motion_pdist): an int32 device tensor [Ma, Mb], every entry exact.  Codes
  [M, L, D] are flattened to [M, L * D]; codes_b=None compares the set with itself.  kind: 'sqdist' (sum of squared differences) | 'dot'.
  The flat distance compares token l of one clip with token l of the other; the latent tokens are index-aligned across clips because they all
  start from the learned `initializer`.  The entries must be codes (|c| <= 128): that is the caller's contract."""
  if kind not in KINDS:
    raise ValueError(f'kind must be one of {sorted(KINDS)}, got {kind!r}')
  a = _flat_codes(codes_a, 'codes_a')
  b = a if codes_b is None else _flat_codes(codes_b, 'codes_b')
  if b.device != a.device:
    raise ValueError(f'codes_a is on {a.device}, codes_b on {b.device}')
  E = int(a.shape[1])
  if int(b.shape[1]) != E:
    raise ValueError(f'codes_a has {E} elements per sample, codes_b {int(b.shape[1])}')
  if E < 1 or E > MAX_E:
    raise ValueError(f'E = {E} elements per sample is outside [1, {MAX_E}]')
  out = torch.empty(a.shape[0], b.shape[0], dtype=torch.int32, device=a.device)
  h = _motion_handle()
  with torch.cuda.device(a.device):
    _lib.check(_lib.load().spa3d_motion_pdist(h, a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], E, KINDS[kind], out.data_ptr(), _stream(a)), h, 'spa3d_motion_pdist')
  return out


# ------------------------------------------------------------------------------------------------ streaming k-NN, ball hits, manifold metrics
MAX_K = 64              # MC_KNN_MAX_K (csrc/motion_code.hpp): a wave's lanes hold a row's list


def _int_arg(v, name, lo):
  if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
    raise ValueError(f'{name} must be an int >= {lo}, got {v!r}')
  return int(v)


def _same_width(named):
  """two named code sets are int16 tensors [M >= 1, ...] with the same number E of elements per sample, 1 <= E <= MAX_E; no device is asked for"""
  for name, t in named:
    if not isinstance(t, torch.Tensor):
      raise ValueError(f'{name} must be a tensor')
    if t.dtype != torch.int16:
      raise ValueError(f'{name} must be int16 codes (motion_codes), got {t.dtype}')
    if t.dim() < 2 or t.shape[0] < 1:
      raise ValueError(f'{name} must be [M >= 1, ...], got {tuple(t.shape)}')
  (na, a), (nb, b) = named
  E, Eb = a[0].numel(), b[0].numel()
  if Eb != E:
    raise ValueError(f'{na} has {E} elements per sample, {nb} {Eb}')
  if E < 1 or E > MAX_E:
    raise ValueError(f'E = {E} elements per sample is outside [1, {MAX_E}]')


def _set_pair(codes, codes_ref, query_offset, what):
  """(a, b, self_offset) of a query set against a reference set.  codes_ref=None: the set against itself, every sample left out of its own
  row; query_offset=s: codes is codes_ref[s : s + M], each sample again left out; otherwise nothing is left out (-1)."""
  # what is wrong with the arguments themselves is said first (ValueError), where they live after that
  if codes_ref is None and query_offset is not None:
    raise ValueError('query_offset names the slice of codes_ref the queries are: it needs codes_ref')
  ref = codes if codes_ref is None else codes_ref
  _same_width((('codes', codes), ('codes_ref', ref)))
  self_offset = 0 if codes_ref is None else (-1 if query_offset is None else _int_arg(query_offset, 'query_offset', 0))
  if self_offset > 0 and self_offset + codes.shape[0] > ref.shape[0]:
    raise ValueError(f'query_offset = {self_offset} with {codes.shape[0]} queries runs past the {ref.shape[0]} samples of codes_ref')
  if ref.device != codes.device:
    raise ValueError(f'codes is on {codes.device}, codes_ref on {ref.device}')
  _on_device(codes, 'codes', what)
  a = codes.contiguous().reshape(codes.shape[0], -1)
  b = a if codes_ref is None else codes_ref.contiguous().reshape(codes_ref.shape[0], -1)
  return a, b, self_offset


def motion_knn(codes, codes_ref=None, k: int = 1, query_offset=None, splits: int = 0):
  """The k nearest samples of codes_ref for every sample of codes, on the exact integer squared distances of the flat codes
  (spa3d_motion_knn): (dist int32 [M, k], idx int64 [M, k]), ascending by (distance, index) -- equal distances go to the lower index, so the
  result is the same however the search was split.  No [M, Mref] matrix is built: the distance tiles are reduced where they are computed.
  codes_ref=None searches the set itself with each sample left out; query_offset=s says codes is codes_ref[s : s + M], each sample again
  left out (a large set against itself, in pieces).  Retrieval: dist, idx = motion_knn(codes_gen, codes_real, k=5).
  k <= 64 and at most the samples a row may take; splits: 0 = the library's plan, n = n column ranges (only time depends on it)."""
  k = _int_arg(k, 'k', 1)
  splits = _int_arg(splits, 'splits', 0)
  if k > MAX_K:
    raise ValueError(f'k = {k} is above {MAX_K}')
  ref = codes if codes_ref is None else codes_ref
  if isinstance(ref, torch.Tensor) and ref.dim() >= 1:
    own = 0 if codes_ref is None else (query_offset if isinstance(query_offset, (int, np.integer)) else -1)
    most = int(ref.shape[0]) - 1 if 0 <= own < ref.shape[0] else int(ref.shape[0])
    if k > most:
      raise ValueError(f'k = {k} needs at least {k} samples a row may take, there are {most}')
  a, b, self_offset = _set_pair(codes, codes_ref, query_offset, 'motion_knn')
  Ma, Mb, E = int(a.shape[0]), int(b.shape[0]), int(a.shape[1])
  lib, h = _lib.load(), _motion_handle()
  need = int(lib.spa3d_motion_knn_workspace_bytes(Ma, Mb, k, splits))
  if need < 0:
    raise ValueError(f'sizes out of range: {Ma} x {Mb} samples, k = {k}, splits = {splits}')
  dist = torch.empty(Ma, k, dtype=torch.int32, device=a.device)
  idx = torch.empty(Ma, k, dtype=torch.int32, device=a.device)
  ws = torch.empty(need // 8, dtype=torch.int64, device=a.device) if need else None
  with torch.cuda.device(a.device):
    _lib.check(lib.spa3d_motion_knn(h, a.data_ptr(), Ma, b.data_ptr(), Mb, E, k, self_offset, splits, dist.data_ptr(), idx.data_ptr(),
                                    ws.data_ptr() if need else None, need, _stream(a)), h, 'spa3d_motion_knn')
  return dist, idx.to(torch.int64)


def motion_ball_hits(codes, codes_ref, radius, query_offset=None, rows: bool = True, cols: bool = True):
  """Counts of hit(i, j) = d(codes[i], codes_ref[j]) <= radius[i] on the exact integer squared distances (spa3d_motion_ball_hits):
  (row_hits int32 [M] = hits of sample i's ball, col_hits int32 [Mref] = balls reference sample j lies in); the one not asked for is None.
  radius: int32 [M]; <= throughout, a negative radius hits nothing.  codes_ref=None / query_offset as motion_knn.  No [M, Mref] matrix."""
  if not rows and not cols:
    raise ValueError('one of rows and cols must be asked for')
  a, b, self_offset = _set_pair(codes, codes_ref, query_offset, 'motion_ball_hits')
  _on_device(radius, 'radius', 'motion_ball_hits')
  if radius.dtype != torch.int32 or tuple(radius.shape) != (a.shape[0],) or radius.device != a.device:
    raise ValueError(f'radius must be int32 [{a.shape[0]}] on {a.device}, got {radius.dtype} {tuple(radius.shape)} on {radius.device}')
  radius = radius.contiguous()
  row_hits = torch.empty(a.shape[0], dtype=torch.int32, device=a.device) if rows else None
  col_hits = torch.empty(b.shape[0], dtype=torch.int32, device=a.device) if cols else None
  h = _motion_handle()
  with torch.cuda.device(a.device):
    _lib.check(_lib.load().spa3d_motion_ball_hits(h, a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], int(a.shape[1]), radius.data_ptr(), self_offset,
                                                  row_hits.data_ptr() if rows else None, col_hits.data_ptr() if cols else None, _stream(a)), h, 'spa3d_motion_ball_hits')
  return row_hits, col_hits


@dataclasses.dataclass
class ManifoldMetrics:
  """manifold_metrics' result.  The four estimates are integer counts followed by one division; the tensors are per sample, on the device."""
  precision: float
  recall: float
  density: float
  coverage: float
  k: int
  real_radius: torch.Tensor          # int32 [R]: squared distance to the k-th nearest other real sample
  gen_radius: torch.Tensor           # int32 [G]
  gen_in_real_balls: torch.Tensor    # int32 [G]: real balls generated sample j lies in; 0 = outside the real manifold
  real_in_gen_balls: torch.Tensor    # int32 [R]: generated balls real sample i lies in
  real_ball_hits: torch.Tensor       # int32 [R]: generated samples inside real sample i's ball


def manifold_metrics(codes_real, codes_gen, k: int = 3) -> ManifoldMetrics:
  """Precision, recall (as precision_recall, to the bit), density and coverage (Naeem et al. 2020, with <=) of a generated set against a real
  one, on the exact integer squared distances of the flat codes, as include/spa3d.h states them.  A sample's radius is its k-th smallest
  distance to the other samples of its own set (two motion_knn calls); the counts come from two ball-hits calls.  No [R, G] matrix is built,
  so the set size is bounded by time, not by memory."""
  k = _int_arg(k, 'k', 1)
  if k > MAX_K:
    raise ValueError(f'k = {k} is above {MAX_K}')
  _same_width((('codes_real', codes_real), ('codes_gen', codes_gen)))
  for name, c in (('codes_real', codes_real), ('codes_gen', codes_gen)):
    if c.shape[0] < k + 1:
      raise ValueError(f'{name} has {c.shape[0]} samples, k = {k} needs at least {k + 1}')
  rad_r = motion_knn(codes_real, k=k)[0][:, k - 1].contiguous()
  rad_g = motion_knn(codes_gen, k=k)[0][:, k - 1].contiguous()
  real_ball_hits, gen_in_real = motion_ball_hits(codes_real, codes_gen, rad_r)
  _, real_in_gen = motion_ball_hits(codes_gen, codes_real, rad_g, rows=False)
  R, G = int(rad_r.shape[0]), int(rad_g.shape[0])
  counts = torch.stack([(gen_in_real > 0).sum(), (real_in_gen > 0).sum(), gen_in_real.sum(dtype=torch.int64), (real_ball_hits > 0).sum()]).tolist()   # one read-back
  return ManifoldMetrics(precision=counts[0] / G, recall=counts[1] / R, density=counts[2] / (k * G), coverage=counts[3] / R, k=k, real_radius=rad_r, gen_radius=rad_g,
                         gen_in_real_balls=gen_in_real, real_in_gen_balls=real_in_gen, real_ball_hits=real_ball_hits)


# ------------------------------------------------------------------------------------------------ kernel sums and the kernel distance
MAX_DEGREE = 3          # MC_KERNEL_MAX_DEGREE (csrc/motion_code.hpp)


def kernel_base(E: int) -> int:
  """C = 16384 E (mc_kernel_base): the kernel (x.y / E + 1)^deg of x = codes / 128 is (a.b + C)^deg / C^deg"""
  return 16384 * int(E)


def _degree_arg(degree):
  if isinstance(degree, bool) or not isinstance(degree, (int, np.integer)) or degree < 1 or degree > MAX_DEGREE:
    raise ValueError(f'degree must be 1, 2 or {MAX_DEGREE}, got {degree!r}')
  return int(degree)


def motion_kernel_sums(codes, codes_ref=None, degree: int = 3, query_offset=None, rows: bool = True, cols: bool = True):
  """Per-row and per-column sums of p(i, j)^degree, p = codes[i] . codes_ref[j] + C with C = 16384 E, over the admitted pairs
  (spa3d_motion_kernel_sums): (row_sums int64 [M, 2], col_sums int64 [Mref, 2]) on the device, each row the BIT PATTERNS of the {lo, hi} limbs of
  an unsigned 128-bit integer (limbs_to_ints reads them); the one not asked for is None.  Exact, and additive over disjoint column or row
  ranges.  codes_ref=None / query_offset as motion_knn.  No [M, Mref] matrix."""
  degree = _degree_arg(degree)
  if not rows and not cols:
    raise ValueError('one of rows and cols must be asked for')
  a, b, self_offset = _set_pair(codes, codes_ref, query_offset, 'motion_kernel_sums')
  row_sums = torch.empty(a.shape[0], 2, dtype=torch.int64, device=a.device) if rows else None
  col_sums = torch.empty(b.shape[0], 2, dtype=torch.int64, device=a.device) if cols else None
  h = _motion_handle()
  with torch.cuda.device(a.device):
    _lib.check(_lib.load().spa3d_motion_kernel_sums(h, a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], int(a.shape[1]), degree, self_offset,
                                                    row_sums.data_ptr() if rows else None, col_sums.data_ptr() if cols else None, _stream(a)), h, 'spa3d_motion_kernel_sums')
  return row_sums, col_sums


def limbs_to_ints(t):
  """int64 [M, 2] limb bit patterns (motion_kernel_sums) -> a list of M Python ints: lo & (2^64 - 1) | hi << 64"""
  if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != 2:
    raise ValueError('limbs must be an int64 tensor [M, 2]')
  mask = (1 << 64) - 1
  return [(lo & mask) | ((hi & mask) << 64) for lo, hi in t.detach().cpu().tolist()]


@dataclasses.dataclass
class KernelDistance:
  """kernel_distance's result.  mmd2 and the witness values are each ONE rounding of an exact rational; the sums are exact Python ints."""
  mmd2: float
  degree: int
  base: int                          # C = 16384 E
  sum_rr: int                        # A = sum over ordered pairs i != i' of p(r_i, r_i')^degree
  sum_gg: int                        # B, likewise for the generated set
  sum_rg: int                        # X = sum over every (generated, real) pair
  witness_real: np.ndarray           # float64 [R]: mean kernel to the other real samples minus mean kernel to the generated set
  witness_gen: np.ndarray            # float64 [G]: mean kernel to the real set minus to the other generated samples; > 0: looks real
  subset_mean: float | None = None   # with subset_size: mean, population standard deviation and values of the per-subset mmd2
  subset_std: float | None = None
  subset_values: list | None = None


def _kernel_distance_once(real, gen, degree):
  from fractions import Fraction
  R, G = int(real.shape[0]), int(gen.shape[0])
  C = kernel_base(real[0].numel())
  rr = motion_kernel_sums(real, degree=degree, cols=False)[0]
  gg = motion_kernel_sums(gen, degree=degree, cols=False)[0]
  gr_rows, gr_cols = motion_kernel_sums(gen, real, degree=degree)
  rr, gg, gr_rows, gr_cols = (limbs_to_ints(t) for t in (rr, gg, gr_rows, gr_cols))
  A, B, X = sum(rr), sum(gg), sum(gr_rows)
  Cd = C ** degree
  mmd2 = float(Fraction(A, R * (R - 1) * Cd) + Fraction(B, G * (G - 1) * Cd) - Fraction(2 * X, R * G * Cd))
  # a witness value x / (R Cd) - s / ((G - 1) Cd) is the ONE rational (x (G - 1) - s R) / (R (G - 1) Cd); Python's int / int is the correctly
  # rounded float64 of the quotient, as float(Fraction) is, without a gcd per element
  den_g, den_r = R * (G - 1) * Cd, (R - 1) * G * Cd
  w_gen = np.array([(x * (G - 1) - s * R) / den_g for x, s in zip(gr_rows, gg)], np.float64)
  w_real = np.array([(s * G - x * (R - 1)) / den_r for s, x in zip(rr, gr_cols)], np.float64)
  return KernelDistance(mmd2=mmd2, degree=degree, base=C, sum_rr=A, sum_gg=B, sum_rg=X, witness_real=w_real, witness_gen=w_gen)


def kernel_distance(codes_real, codes_gen, degree: int = 3, subset_size=None) -> KernelDistance:
  """The kernel distance of a generated set against a real one as include/spa3d.h states it: the unbiased MMD^2 with the polynomial kernel
  (x.y / E + 1)^degree on the flat codes x = c / 128 (degree 3: KID's kernel, Binkowski et al. 2018 -- on motion codes, not Inception features, so
  not comparable with published KID values).  Three motion_kernel_sums calls give exact integer sums; mmd2 is one exact rational rounded once.
  It needs no covariance and is unbiased at any set size, where the Frechet distance of fewer samples than dimensions says little.  The witness
  says which samples pull the sets apart (KernelDistance).  subset_size=s adds the mean and population standard deviation of the estimate over
  the contiguous subsets real[t s : (t + 1) s] against gen[t s : (t + 1) s], t < min(R, G) // s (shuffle first for random subsets).  No
  [R, G] matrix is built."""
  degree = _degree_arg(degree)
  _same_width((('codes_real', codes_real), ('codes_gen', codes_gen)))
  R, G = int(codes_real.shape[0]), int(codes_gen.shape[0])
  for name, m in (('codes_real', R), ('codes_gen', G)):
    if m < 2:
      raise ValueError(f'{name} has {m} sample, the unbiased estimate needs at least 2')
  if subset_size is not None:
    s = _int_arg(subset_size, 'subset_size', 2)
    if s > min(R, G):
      raise ValueError(f'subset_size = {s} is above the smaller set\'s {min(R, G)} samples')
  res = _kernel_distance_once(codes_real, codes_gen, degree)
  if subset_size is not None:
    vals = [_kernel_distance_once(codes_real[t * s:(t + 1) * s], codes_gen[t * s:(t + 1) * s], degree).mmd2 for t in range(min(R, G) // s)]
    res.subset_values = vals
    res.subset_mean = float(np.mean(vals))
    res.subset_std = float(np.std(vals))
  return res


def knn_precision_recall(d_rr, d_gg, d_rg, k: int):
  """The selection of precision_recall on the three distance matrices (real-real [R, R], generated-generated [G, G], real-generated [R, G]),
  any integer or float tensors: (precision, recall) as Python floats.  <= throughout."""
  R, G = int(d_rr.shape[0]), int(d_gg.shape[0])
  for name, m in (('real', R), ('generated', G)):
    if m < k + 1:
      raise ValueError(f'the {name} set has {m} samples, k = {k} needs at least {k + 1}')
  # a sample's radius: its k-th smallest distance to the OTHER samples of its own set -- the (k + 1)-th smallest of its row with the diagonal
  # (its distance to itself, the row's minimum 0) left in
  rad_r = torch.kthvalue(d_rr, k + 1, dim=1).values
  rad_g = torch.kthvalue(d_gg, k + 1, dim=1).values
  inside_real = int((d_rg <= rad_r[:, None]).any(dim=0).sum().item())   # generated samples inside some real sample's ball
  inside_gen = int((d_rg <= rad_g[None, :]).any(dim=1).sum().item())     # real samples inside some generated sample's ball
  return inside_real / G, inside_gen / R   # integer counts, one division each: the same float on every device


def precision_recall(codes_real, codes_gen, k: int = 3):
  """The k-NN manifold estimate of precision and recall on the exact integer squared distances of the flat codes.  A sample's radius is its
  k-th smallest distance to the other samples of its own set; precision is the share of generated samples within (<=) the radius of at least
  one real sample, recall the share of real samples within the radius of at least one generated sample.  Integer distances make ties exact
  and the estimate reproducible.  -> (precision, recall)"""
  if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
    raise ValueError(f'k must be a positive int, got {k!r}')
  for name, c in (('codes_real', codes_real), ('codes_gen', codes_gen)):
    if isinstance(c, torch.Tensor) and c.dim() >= 1 and c.shape[0] < k + 1:
      raise ValueError(f'{name} has {c.shape[0]} samples, k = {k} needs at least {k + 1}')
  d_rr = motion_pdist(codes_real)
  d_gg = motion_pdist(codes_gen)
  d_rg = motion_pdist(codes_real, codes_gen)
  return knn_precision_recall(d_rr, d_gg, d_rg, int(k))
