"""Host references of the first mile of the model (csrc/embed.hip, discretize_kernel of csrc/loss.hip) for tests/test_gpu_embed.py: plain numpy / torch,
written from the statement of each operation.  Where the operation is arithmetic the argument arithmetic is float32 in the kernel's order (numpy float32
operations round after every step) and the sine is taken in float64 on those float32 arguments.  Checked on the CPU, against the oracle and against brute
force, in tests/test_embed_ref_host.py."""
import numpy as np
import torch

from util import O

f32 = np.float32
HALF_PI = f32(0.5 * np.pi)   # fl32(pi / 2) = 1.57079637050628662109375
SENTINEL = -1280.0           # exact in fp32, bf16 and fp16; no operation here produces it (|sin| <= 1, masks are 0 / 1, maps are >= -1)


# ------------------------------------------------------------------------------------------------ sinusoidal embeddings
def sin_args(x, nf, prescale=1.0):
  """x float32 [rows, C] -> the float32 sine arguments [rows, C, 2 nf]: xv = x / prescale, v = fl32(xv s_f), [v | fl32(v + fl32(pi / 2))]"""
  x = np.asarray(x, f32)
  with np.errstate(invalid='ignore', over='ignore'):
    xv = x / f32(prescale)
    v = xv[..., None] * O.sin_scales(nf)
    a = np.concatenate([v, v + HALF_PI], -1)
  assert a.dtype == f32
  return a


def sin_embed_ref(x, nf, prescale=1.0):
  """SinusoidalEmbedding(x / prescale), layout "(coords d)": float64 [rows, C 2 nf]; a NaN or an infinity in x gives NaN in its coordinate's 2 nf columns"""
  a = sin_args(x, nf, prescale)
  with np.errstate(invalid='ignore'):
    return np.sin(a.astype(np.float64)).reshape(a.shape[0], -1)


def time_coord(nrows, T):
  """fl32(fl32(r % T) / fl32(T)) of every row: jnp.arange(T) / T tiled over the sequences"""
  return (np.arange(nrows) % T).astype(f32) / f32(T)


def embed_tokens_ref(tracks, T, nf, prescale=1.0):
  """tracks float32 [nrows, NC] -> float64 [nrows, (NC + 1) 2 nf]: the embedding of [tracks | time_coord]"""
  tracks = np.asarray(tracks, f32)
  x = np.concatenate([tracks, time_coord(tracks.shape[0], T)[:, None]], 1)
  return sin_embed_ref(x, nf, prescale)


def query_embed_ref(qp, nf, track_scale, time_scale):
  """qp float32 [nq, NC + 1] = (t, coordinates) -> (sin float64 [nq, NC 2 nf], tfeat float32 [nq], qframe int32 [nq]):
  qframe = rint(t) (half to even), tfeat = floor(fl32(qframe) / fl32(time_scale))"""
  qp = np.asarray(qp, f32)
  qframe = np.rint(qp[:, 0]).astype(np.int32)
  tfeat = np.floor(qframe.astype(f32) / f32(time_scale))
  assert tfeat.dtype == f32
  return sin_embed_ref(qp[:, 1:], nf, track_scale), tfeat, qframe


# ------------------------------------------------------------------------------------------------ row maps, readout rows, key masks
def embed_maps_ref(row_src, rows, S, T):
  """-> (arow, crow int32 [rows], readout bool [rows]): row j is dense token q = row_src[j] (None: j) = (seq, s); a frame token reads input row
  seq T + s - 1 and keeps its row, a readout token (s == 0) drops its GEMM row (crow -1, arow the sequence's first input row)"""
  assert S == T + 1
  arow, crow, ro = np.zeros(rows, np.int32), np.zeros(rows, np.int32), np.zeros(rows, bool)
  j = 0
  src = iter(row_src) if row_src is not None else None
  while j < rows:
    q = int(next(src)) if src is not None else j
    seq, s = divmod(q, S)
    if s == 0:
      arow[j], crow[j], ro[j] = seq * T, -1, True
    else:
      arow[j], crow[j] = seq * T + s - 1, j
    j += 1
  return arow, crow, ro


def keymask_ref(vis, boundary, N, with_readout):
  """vis float32 [nseq, T], boundary int [nseq / N] -> float32 [nseq, T + 1] (key 0 = the readout token, always 1) or [nseq, T]: key t is kept when
  vis != 0 (so -0.0 is dropped, NaN and fractions are kept) and t < boundary of the sequence's sample"""
  nseq, T = vis.shape
  km = np.zeros((nseq, T + 1 if with_readout else T), f32)
  for s in range(nseq):
    b = int(boundary[s // N])
    if with_readout:
      km[s, 0] = 1.0
    for t in range(T):
      v = float(vis[s, t])
      if v != 0 and t < b:
        km[s, t + 1 if with_readout else t] = 1.0
  return km


# ------------------------------------------------------------------------------------------------ weight shadows
def sum3_ref(a, b, c):
  """fl32(fl32(a + b) + c), a missing operand is 0.f"""
  n = len(next(x for x in (a, b, c) if x is not None))
  z = np.zeros(n, f32)
  a, b, c = (z if x is None else np.asarray(x, f32) for x in (a, b, c))
  return (a + b) + c


def pack_ref(src, cols, dt):
  """src float32 torch [rows, src_ld] -> (native [rows, cols], transposed [cols, rows]) in dt: torch's cast rounds to nearest even"""
  n = src[:, :cols].to(dt)
  return n, n.T.contiguous()


# ------------------------------------------------------------------------------------------------ latent quantiser
def discretize_ref(lat, noise, discretize):
  """float32 arrays -> (out, clipmask) float32, every step rounded to float32 in the source's order: l = clip(lat, -1, 1);
  q = rint(l 128) / 128; q = (q + noise / 128) - 1 / 256; out = l - (l - q).  clipmask = 1 where -1 <= lat <= 1.  NaN passes through to both"""
  raw = np.asarray(lat, f32)
  nan = np.isnan(raw)
  with np.errstate(invalid='ignore'):
    l = np.where(nan, raw, np.minimum(np.maximum(raw, f32(-1)), f32(1)))
    mask = np.where(nan, raw, ((raw >= f32(-1)) & (raw <= f32(1))).astype(f32))
    if discretize:
      q = np.rint(l * f32(128)) / f32(128)
      q = (q + np.asarray(noise, f32) / f32(128)) - f32(1.0 / 256.0)
      l = l - (l - q)
  assert l.dtype == f32 and mask.dtype == f32
  return l, mask


def discretize_scalar(raw, u, discretize):
  """one element of discretize_ref in numpy float32 scalar arithmetic"""
  raw = f32(raw)
  if raw != raw:
    return raw, raw
  l = min(max(raw, f32(-1)), f32(1))
  mask = f32(1) if f32(-1) <= raw <= f32(1) else f32(0)
  if discretize:
    q = f32(np.rint(f32(l * f32(128)))) / f32(128)
    q = f32(f32(q + f32(f32(u) / f32(128))) - f32(1.0 / 256.0))
    l = f32(l - f32(l - q))
  return f32(l), mask


def discretize_oracle64(lat, noise, discretize):
  """the clip / round / noise / straight-through lines of the oracle's decode in float64 (torch.round is half to even)"""
  l = torch.clamp(torch.as_tensor(np.asarray(lat, np.float64)), -1.0, 1.0)
  if discretize:
    d = torch.round(l * 128.0) / 128.0
    d = d + torch.as_tensor(np.asarray(noise, np.float64)) / 128.0 - 1.0 / 256.0
    l = l - (l - d)
  return l.numpy()


def discretize_planted():
  """latents at every edge of the quantiser: the clip bounds and their neighbours, both zeros, ties of rint at (k + 0.5) / 128 for even and odd k of both
  signs, NaN and the infinities"""
  eps = 2.0 ** -23
  ties = [(k + 0.5) / 128.0 for k in (0, 1, 2, 3, 64, 65, 126, 127, -1, -2, -3, -4, -65, -66, -127, -128)]
  return np.array([1.0, -1.0, 1.0 + eps, -1.0 - eps, 1.0 - eps / 2, -1.0 + eps / 2, 1.5, -1.5, 0.0, -0.0] + ties + [np.nan, np.inf, -np.inf], f32)


# ------------------------------------------------------------------------------------------------ what the entry points refuse
def refusals(lib, dtype, a, o, f, z, stream):
  """(name, status) of every call of the embedding entry points that must return SPA3D_ERR_ARG: a NULL pointer once per required argument, negative counts,
  nf = 0 and 65, NC = 1 and 4, S != T + 1, N not dividing nseq, leading dimensions below the width, both pack outputs NULL, discretize = 1 without noise,
  a zero or NaN scale, an unknown dtype.  a: fp32 input, o: output of `dtype`, f: fp32 output, z: int32 buffer -- addresses; nothing is read through them"""
  s = stream
  nan = float('nan')

  def each(name, fn, good, ptrs, cases, dtype_at=None):
    for i in ptrs:
      yield f'{name} NULL argument {i}', fn(*[None if j == i else v for j, v in enumerate(good)])
    for label, i, v in cases:
      yield f'{name} {label}', fn(*[v if j == i else x for j, x in enumerate(good)])
    if dtype_at is not None:
      for bad in (3, -1):
        yield f'{name} dtype {bad}', fn(*[bad if j == dtype_at else x for j, x in enumerate(good)])

  nfs = lambda i: [('nf = 0', i, 0), ('nf = 65', i, 65), ('nf < 0', i, -32)]
  ncs = lambda i: [('NC = 1', i, 1), ('NC = 4', i, 4), ('NC = 0', i, 0)]
  yield from each('sin_embed_scaled', lib.spa3d_op_sin_embed_scaled, [a, 4, 3, 32, 1.0, o, dtype, s], (0, 5),
                  [('rows < 0', 1, -1), ('C = 0', 2, 0), ('C < 0', 2, -1), ('prescale = 0', 4, 0.0), ('prescale NaN', 4, nan)] + nfs(3), 6)
  if dtype == 0:
    yield from each('sin_embed', lib.spa3d_op_sin_embed, [a, 4, 3, 32, o, dtype, s], (0, 4), nfs(3))
  yield from each('embed_tokens', lib.spa3d_op_embed_tokens, [a, 4, 2, 3, 32, 1.0, o, dtype, s], (0, 6),
                  [('nrows < 0', 1, -1), ('T = 0', 2, 0), ('T < 0', 2, -1), ('prescale = 0', 5, 0.0), ('prescale NaN', 5, nan)] + ncs(3) + nfs(4), 7)
  yield from each('embed_maps', lib.spa3d_op_embed_maps, [z, 4, 3, 2, z + 0x100, z + 0x200, o, a, 8, dtype, s], (4, 5, 6, 7),
                  [('rows < 0', 1, -1), ('S = T', 2, 2), ('S = T + 2', 2, 4), ('T = 0', 3, 0), ('T < 0', 3, -1), ('d = 0', 8, 0), ('d < 0', 8, -8)], 9)
  yield from each('set_readout_rows', lib.spa3d_op_set_readout_rows, [o, a, 4, 3, 8, dtype, s], (0, 1),
                  [('nseq < 0', 2, -1), ('S = 0', 3, 0), ('S < 0', 3, -1), ('d = 0', 4, 0), ('d < 0', 4, -8)], 5)
  yield from each('pack', lib.spa3d_op_pack, [a, 10, 4, 8, o, 8, o + 0x1000, 4, dtype, s], (0,),
                  [('rows < 0', 2, -1), ('cols < 0', 3, -1), ('src_ld < cols', 1, 7), ('ldn < cols', 5, 7), ('ldt < rows', 7, 3), ('ldn < 0', 5, -8),
                   ('rows past the grid', 2, 65535 * 32 + 1)], 8)
  yield 'pack both outputs NULL', lib.spa3d_op_pack(a, 10, 4, 8, None, 8, None, 4, dtype, s)
  yield 'pack ldn < cols, transposed given', lib.spa3d_op_pack(a, 10, 4, 8, o, 7, o + 0x1000, 4, dtype, s)
  yield 'pack ldt < rows, native NULL', lib.spa3d_op_pack(a, 10, 4, 8, None, 0, o, 3, dtype, s)
  yield from each('transpose', lib.spa3d_op_transpose, [o, 4, 8, o + 0x1000, dtype, s], (0, 3),
                  [('rows < 0', 1, -1), ('cols < 0', 2, -1), ('rows past the grid', 1, 65535 * 32 + 1)], 4)
  if dtype == 0:   # the entry points without a storage type: once
    yield from each('query_embed', lib.spa3d_op_query_embed, [a, 4, 3, 32, 1.0, 150.0, f, z, s], (0, 6, 7),
                    [('nq < 0', 1, -1), ('track_scale = 0', 4, 0.0), ('time_scale = 0', 5, 0.0), ('time_scale NaN', 5, nan)] + ncs(2) + nfs(3))
    yield from each('keymask', lib.spa3d_op_keymask, [a, z, 6, 3, 4, 1, f, s], (0, 1, 6),
                    [('nseq < 0', 2, -3), ('N = 0', 3, 0), ('N < 0', 3, -3), ('N = 4 does not divide nseq = 6', 3, 4), ('N = 7 > nseq', 3, 7), ('T = 0', 4, 0),
                     ('T < 0', 4, -1), ('with_readout = 2', 5, 2), ('with_readout = -1', 5, -1)])
    yield 'keymask 2-D, N does not divide nseq', lib.spa3d_op_keymask(a, z, 6, 4, 4, 0, f, s)
    yield from each('sum3', lib.spa3d_op_sum3, [a, a, a, f, 8, s], (3,), [('n < 0', 4, -1)])
    yield 'sum3 without an operand', lib.spa3d_op_sum3(None, None, None, f, 8, s)
    yield from each('discretize', lib.spa3d_op_discretize, [a, a + 0x1000, 1, f, f + 0x1000, 8, s], (0, 1, 3),
                    [('n < 0', 5, -1), ('discretize = 2', 2, 2), ('discretize = -1', 2, -1)])
    yield 'discretize = 0, NULL latents', lib.spa3d_op_discretize(None, None, 0, f, None, 8, s)
