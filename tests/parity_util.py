"""Helpers of the per-kernel parity tests: outputs inside canary-guarded allocations, poisoned workspaces, an element-wise error bound
derived from the number formats, per-row errors, and the exact-integer GEMM operands whose products have one right answer bit for bit.
Plain functions, no fixtures.  Everything except guarded() / poisoned_ws() runs on the host (tests/test_parity_gates_host.py)."""
import math
import os

import torch

# ------------------------------------------------------------------------------------------------ number formats
U_F32, U_BF16, U_F16 = 2.0 ** -24, 2.0 ** -8, 2.0 ** -11   # unit roundoff (round to nearest even, st() in csrc/common.hpp): half an ulp of 1.0


def unit_roundoff(dtype):
  return {torch.float32: U_F32, torch.bfloat16: U_BF16, torch.float16: U_F16}[dtype]


# ------------------------------------------------------------------------------------------------ guarded outputs
CANARY16 = -91      # int16 0xFFA5: a NaN as bf16 and as fp16, and 0xFFA5FFA5 is a NaN as fp32; not the NaN torch.full(nan) writes
GUARD_FRONT_BYTES = 4096
GUARD_TAIL_ROWS = 384   # the tallest workgroup tile in csrc/ (gemm_ntb 384 x 256, gemm_tnb 384 x 256, gemm_tn8p 384 x 128)
_guards = []            # (test id, name, int16 canary views)


def _current_test():
  return os.environ.get('PYTEST_CURRENT_TEST', '')


def guarded(rows, cols, dtype, ld=None, device='cuda', name='out', fill=float('nan')):
  """A [rows, cols] view (row stride ld elements, default cols) of `dtype` inside a larger allocation whose every other byte holds the canary:
  >= 4 KiB before the view, 384 rows x ld after it, and the ld - cols gap of every row.  The view itself is filled with `fill` (NaN: an element the
  kernel does not write stays visible).  The view starts 4 KiB into the allocation, so it keeps the 16-byte alignment the kernels ask for.
  check_guards() later asserts that no canary byte changed."""
  ld = cols if ld is None else ld
  assert ld >= cols and rows >= 0
  es = torch.empty(0, dtype=dtype).element_size()
  assert es in (2, 4) and GUARD_FRONT_BYTES % es == 0
  front = GUARD_FRONT_BYTES // es
  n = front + (rows + GUARD_TAIL_ROWS) * ld
  raw = torch.full((n * es // 2,), CANARY16, dtype=torch.int16, device=device)
  buf = raw.view(dtype)
  body = buf[front:front + rows * ld].view(rows, ld)
  view = body[:, :cols]
  view.fill_(fill)
  regions = [raw[:front * es // 2], raw[(front + rows * ld) * es // 2:]]
  if ld > cols:
    regions.append(body[:, cols:])
  me = _current_test()
  _guards[:] = [g for g in _guards if g[0] == me]   # a test that failed before its check leaves nothing behind for the next one
  _guards.append((me, name, regions, raw))
  return view


def canary_intact(region):
  """every byte of `region` (any dtype, any strides) still holds the canary"""
  r = region.contiguous().view(torch.int16) if region.dtype != torch.int16 else region
  return torch.equal(r.contiguous().view(torch.uint8), torch.full_like(r, CANARY16).contiguous().view(torch.uint8))


def check_guards():
  """assert that every canary byte of every guarded() allocation of this test is bit-unchanged, then forget them"""
  if _guards and _guards[0][2][0].is_cuda:
    torch.cuda.synchronize()
  bad = []
  for _, name, regions, _raw in _guards:
    for where, r in zip(('before the view', 'after the last row', 'in the row gaps'), regions):
      if not canary_intact(r):
        r16 = r.contiguous().view(torch.int16).reshape(-1)
        hit = (r16 != CANARY16).nonzero().reshape(-1)
        bad.append(f'{name}: {hit.numel()} 16-bit words changed {where}, first at word {int(hit[0])}')
  _guards.clear()
  assert not bad, 'stray stores outside the output view: ' + '; '.join(bad)


def poisoned_ws(nbytes, device='cuda'):
  """a workspace of 0xFF bytes (a NaN in fp32, bf16 and fp16): a kernel that reads a slot nobody wrote computes NaNs instead of passing on zeros"""
  return torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device=device)


def linear_ws_bytes(N, K, elem_size=2):
  """what spa3d_op_linear / spa3d_op_linear_bwd carve from their workspace (csrc/ops.hip): one K x N copy of the weight (transposed or packed as a
  fragment stream: gemm_ntb_pack_elems = K N, gemm_rs_pack_elems = 384 N) and a 256-byte zero page, each rounded up by the arena"""
  return K * N * elem_size + (64 << 10)


# ------------------------------------------------------------------------------------------------ element-wise gate
C_MFMA = 4.0   # the one factor that is not derived: MFMA's accumulation inside a block is not documented as IEEE


def abs_product(A, B):
  """an upper bound of |A| . |B| in fp64, from an fp32 matmul: every term is >= 0, so the fp32 sum is within K 2^-24 (1 + ...) relative of the exact
  one whatever its order; inflating by K 2^-23 makes it an upper bound without an fp64 matmul of the test's largest shapes"""
  K = A.shape[1]
  return (A.float().abs() @ B.float().abs()).double() * (1.0 + K * 2.0 ** -23)


def elementwise_bound(ref64, absprod, K, out_dtype, bias=None, R=None, act_err=0.0, lipschitz=1.0, c=C_MFMA):
  """|got - ref| allowed per element for a result that is ONE round-to-nearest-even (to out_dtype) of an fp32 accumulation:

      u_out |ref| + (1 + u_out) [ lipschitz c (K + 2) 2^-24 (|A|.|B| + |bias|) + c (K + 2) 2^-24 |R| + act_err ]

  u_out |ref|: the output rounding (absent for fp32 output).  c (K + 2) 2^-24 (...): the any-order fp32 summation bound of K products (exact: 16-bit
  operands) plus the bias and the residual, times c = 4 for MFMA's undocumented in-block accumulation -- it holds for every tiling and for atomics.
  With an activation between the sum and the store, the sum's error passes through it (lipschitz = max |act'|, 1.13 for tanh-gelu) and act_err is
  added: 4 x the measured |fp32 host evaluation - fp64| of the activation on the test's own pre-activations."""
  u = unit_roundoff(out_dtype)
  g = c * (K + 2) * U_F32
  pre = absprod.double().clone()
  if bias is not None:
    pre = pre + bias.double().abs()
  acc = lipschitz * g * pre
  if R is not None:
    acc = acc + g * R.double().abs()
  out_round = 0.0 if out_dtype == torch.float32 else u * ref64.abs()
  return out_round + (1.0 + u) * (acc + act_err)


GELU_LIPSCHITZ = 1.13   # max |d/dx tanh-gelu(x)| = 1.1290 (at x = 1.46)


def gelu_tanh(x):
  return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_act_err(pre64):
  """4 x max |tanh-gelu evaluated in fp32 on the host - fp64| over these pre-activations (the factor covers the device's exp / tanh
  differing from the host's by a few ulp; tests/test_gpu_ops.py::test_sin_embed argues the same way for sinf)"""
  return 4.0 * float((gelu_tanh(pre64.float()).double() - gelu_tanh(pre64)).abs().max())


def elementwise_report(got, ref64, bound):
  """(number of elements over the bound, index of the worst, worst |got - ref| / bound)"""
  err = (got.detach().double().cpu() - ref64.double()).abs()
  bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
  bad = ~(err <= bound)   # a NaN in got is over any bound
  ratio = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err / bound.clamp_min(1e-300))
  worst = int(ratio.reshape(-1).argmax()) if err.numel() else 0
  idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), err.shape)) if err.numel() else ()
  return int(bad.sum()), idx, float(ratio.reshape(-1)[worst]) if err.numel() else 0.0


def assert_elementwise(got, ref64, bound, what='output'):
  """|got - ref| <= bound for EVERY element; on failure the count, the worst index and the worst error / bound"""
  n, idx, ratio = elementwise_report(got, ref64, bound)
  print(f'  elementwise {what}: worst |err| / bound = {ratio:.3f} at {idx}')
  assert n == 0, f'{what}: {n} of {ref64.numel()} elements over the bound, worst at {idx}: |err| = {ratio:.3f} x bound'


def row_errs(got, ref64, dim=-1):
  """relative L2 error of every row along `dim`: ||got - ref|| / ||ref||"""
  g, r = got.detach().double().cpu(), ref64.double()
  return (g - r).norm(dim=dim) / (r.norm(dim=dim) + 1e-30)


# ------------------------------------------------------------------------------------------------ exact-integer GEMM lane
def sparse_sign_matrix(K, N):
  """W [K, N] with exactly r = ceil(K / 64) entries of +-1 per column, at deterministic positions: column n has one entry in every block of 64
  consecutive k (the last block may be shorter), at offset (37 (n % 64) + 7 (n // 64) + 3 j) % 64 of block j (folded into a short last block).
  37 is odd, so the 64 columns of an aligned group hit the 64 offsets of every block once each: every aligned group of 64 columns touches every k.
  Returns (W float32, idx int64 [r, N], sgn float32 [r, N]) with W[idx[j, n], n] = sgn[j, n]."""
  r = (K + 63) // 64
  n = torch.arange(N)
  j = torch.arange(r)[:, None]
  off = (37 * (n % 64) + 7 * (n // 64))[None, :] + 3 * j
  width = torch.full((r, 1), 64)
  width[-1, 0] = K - 64 * (r - 1)
  idx = 64 * j + (off % 64) % width
  h = (n[None, :] * 2654435761 + j * 40503 + 12345) >> 7
  sgn = (1 - 2 * (h & 1)).float()
  W = torch.zeros(K, N)
  W[idx, n[None, :].expand(r, N)] = sgn
  return W, idx, sgn


def int_lane_nt(M, N, K, seed, bias=True, res=False):
  """Operands of C = A . W (+ bias)(+ R) whose every partial sum is an integer of magnitude <= 256, exact in bf16 and fp16: A dense in [-a, a],
  W = sparse_sign_matrix(K, N), bias in [-3, 3], R in [-5, 5], a = (256 - 3 - 5) // r.  The reference is a signed gather of A's columns (float32
  arithmetic on small integers: exact), not a matmul.  Returns (A, W, bias, R, ref), all float32, bias / R None when not asked for."""
  r = (K + 63) // 64
  a = (256 - 3 - 5) // r
  assert a >= 1, 'K too long for the exact lane'
  g = torch.Generator().manual_seed(seed)
  A = torch.randint(-a, a + 1, (M, K), generator=g).float()
  W, idx, sgn = sparse_sign_matrix(K, N)
  b = torch.randint(-3, 4, (N,), generator=g).float() if bias else None
  R = torch.randint(-5, 6, (M, N), generator=g).float() if res else None
  ref = torch.zeros(M, N)
  for j in range(r):
    ref += A[:, idx[j]] * sgn[j]
  if bias:
    ref += b
  if res:
    ref += R
  assert float(ref.abs().max()) <= 256
  return A, W, b, R, ref


def int_lane_tn(M, N, K, seed):
  """Operands of dW = A^T . dC and dbias = colsum(dC) with exact fp32 sums: A [M, K] with r = ceil(K / 64) entries of +-1 per ROW (the transpose of
  sparse_sign_matrix(K, M): every aligned group of 64 rows touches every column), dC dense in [-4, 4]; |sum| <= 4 M < 2^24 for M <= 100 003.  The
  reference is an index_add_ of dC's rows.  Returns (A, dC, dW_ref, dbias_ref), float32."""
  assert 4 * M < 2 ** 24
  g = torch.Generator().manual_seed(seed)
  Wt, idx, sgn = sparse_sign_matrix(K, M)   # idx [r, M]: the columns row m touches
  dC = torch.randint(-4, 5, (M, N), generator=g).float()
  ref = torch.zeros(K, N)
  for j in range(idx.shape[0]):
    ref.index_add_(0, idx[j], dC * sgn[j][:, None])
  return Wt.t().contiguous(), dC, ref, dC.sum(0)


# ------------------------------------------------------------------------------------------------ exact-integer lane of a GEMM descriptor
# spa3d_op_gemm (tests/test_gpu_gemm_desc.py): the lane above with everything that changes an address -- padded strides, the crow / brow row remaps,
# gather and scatter maps, two A sources, a rank-1 term, an initial C, an initial column sum, alpha a power of two.  Host only; the references are
# gathers / index_add_ in float64 built from the index maps (tests/test_gemm_desc_host.py checks the maps and that every expected value is exact).
def row_map(n, group, skip):
  """Where rows 0 .. n - 1 of a remapped operand sit: row m at m + (m // group + 1) * skip -- behind every `group` rows `skip` rows that do not belong
  to the GEMM (the readout rows), the first of them before row 0.  group 0: no remap.  The one place in tests/ where the formula is written."""
  m = torch.arange(n)
  return m if group == 0 else m + (m // group + 1) * skip


def pattern(rows, cols):
  """The recognisable fill of a destination: -(512 + 4 ((7 row + 3 col) % 64)), multiples of 4 in [-764, -512] -- exact in bf16, fp16 and fp32, outside the
  lane's results (|.| <= 256), and different in neighbouring rows and columns, so a row stored in the wrong place is not mistaken for an untouched one."""
  return -(512.0 + 4.0 * ((7 * torch.arange(rows)[:, None] + 3 * torch.arange(cols)[None, :]) % 64)).double()


def assert_exact_in(ref, dtype, what='reference'):
  """every value of `ref` (float64) is exactly representable in `dtype`: the lane compares with torch.equal, so this is a condition, not a tolerance"""
  assert bool(torch.isfinite(ref).all()), what
  if dtype == torch.float32:
    assert float(ref.abs().max()) < 2 ** 24 and torch.equal(ref, ref.round()), f'{what}: not an integer below 2^24'
  else:
    assert torch.equal(ref.to(dtype).double(), ref), f'{what}: not exact in {dtype}'


def padded(x, ld, rows=None, at=None, fill=float('nan')):
  """x [m, n] inside a [rows, ld] buffer of `fill` (NaN: what the kernel must not read): row i of x at buffer row at[i] (default i), columns [0, n)"""
  m, n = x.shape
  rows = m if rows is None else rows
  buf = torch.full((rows, ld), fill, dtype=torch.float64)
  buf[torch.arange(m) if at is None else at, :n] = x.double()
  return buf


def desc_nt_case(M, N, K, seed, lda=None, ldc=None, crow=(0, 0), res=False, bias=True, alpha=1.0, acc=False, emb=None):
  """C = alpha A . W (+ bias)(+ rank-1)(+ R)(+ C0) on the integer lane, as a dict of float64 host tensors.
  A in [-a, a] (x 1 / alpha for alpha < 1, so alpha A stays an integer), W = sparse_sign_matrix(K, N), bias in [-3, 3], R in [-5, 5], C0 (the initial C of
  `acc`) in [-7, 7], rank-1 term r1_x in [-2, 2] times r1_w in [-3, 3]: a = min(100, 235 // (r max(alpha, 1))) keeps every sum within 256.
  crow = (group, skip): C, R and pre_out rows through row_map.  emb = dict(K1, src_rows, lda2, r1): the one-pass embedding -- input rows gathered through
  `arow` (with repeats, from src_rows > M rows; rows it never names are NaN), columns [0, K1) from A and [K1, K) from A2 (K1 = 0: one source), output
  rows scattered through `cidx`, an injective map into M + M // 2 rows with about a quarter dropped (-1), rows 0 and 127 (first and last of a tile) and
  the last row among them.
  Keys: A, A2 (padded buffers, NaN in the pad columns and unnamed rows), W [K, N], bias, r1_x [src_rows], r1_w [N], arow, cidx (int32), cmap (row of C per output
  row, -1 dropped), rows (of C), R (padded [rows, ldc], NaN outside the image), C0 [rows, N] (pattern(); the integers of `acc` in the image), pre [M, N] (before R / C0),
  C [rows, N] and P [rows, N] (the expected C and pre_out: pattern() outside the image)."""
  lda = K if lda is None else lda
  ldc = N if ldc is None else ldc
  r = (K + 63) // 64
  a = min(100, 235 // int(r * max(alpha, 1.0)))
  assert a >= 1
  g = torch.Generator().manual_seed(seed)
  W, idx, sgn = sparse_sign_matrix(K, N)
  o = dict(W=W.double(), bias=None, A2=None, r1_x=None, r1_w=None, arow=None, cidx=None)
  scale = 1.0 if alpha >= 1.0 else 1.0 / alpha
  if emb is None:
    Aeff = torch.randint(-a, a + 1, (M, K), generator=g).double() * scale
    o['A'] = padded(Aeff, lda)
    src = torch.arange(M)
  else:
    S, K1 = emb['src_rows'], emb['K1']
    assert S > M
    src = torch.randint(0, S, (M,), generator=g)
    src[1] = src[0]                                   # a repeat for sure
    named = torch.zeros(S, dtype=torch.bool); named[src] = True
    full = torch.randint(-a, a + 1, (S, K), generator=g).double() * scale
    full[~named] = float('nan')
    if K1:
      o['A'], o['A2'] = padded(full[:, :K1], lda), padded(full[:, K1:], emb['lda2'])
      Aeff = torch.cat([o['A'][src, :K1], o['A2'][src, :K - K1]], 1)   # gather, then concatenate: the multi-pass form
    else:
      o['A'] = padded(full, lda)
      Aeff = o['A'][src, :K]
    o['arow'] = src.int()
  pre = torch.zeros(M, N, dtype=torch.float64)
  for j in range(r):
    pre += Aeff[:, idx[j]] * sgn[j].double()
  pre *= alpha
  if bias:
    o['bias'] = torch.randint(-3, 4, (N,), generator=g).double()
    pre += o['bias']
  if emb is not None and emb.get('r1'):
    x = torch.randint(-2, 3, (emb['src_rows'],), generator=g).double()
    x[~named] = float('nan')
    o['r1_x'], o['r1_w'] = x, torch.randint(-3, 4, (N,), generator=g).double()
    pre += x[src][:, None] * o['r1_w'][None, :]
  if emb is None:
    cmap = row_map(M, *crow)
    rows = int(cmap[-1]) + 1 + crow[1] + 2            # the rows behind the last one stay untouched too
  else:
    rows = M + M // 2
    cmap = torch.randperm(rows, generator=g)[:M]
    drop = torch.rand(M, generator=g) < 0.25
    drop[[0, 127, M - 1]] = True
    drop[[1, 126]] = False
    cmap[drop] = -1
    o['cidx'] = cmap.int()
  keep = cmap >= 0
  out = pre.clone()
  o['R'] = None
  if res:
    R = torch.randint(-5, 6, (M, N), generator=g).double()
    o['R'] = padded(R[keep], ldc, rows, cmap[keep])
    out += R
  o['C0'] = pattern(rows, N)
  if acc:
    c0 = torch.randint(-7, 8, (M, N), generator=g).double()
    o['C0'][cmap[keep]] = c0[keep]
    out += c0
  o['C'], o['P'] = pattern(rows, N), pattern(rows, N)
  o['C'][cmap[keep]] = out[keep]
  o['P'][cmap[keep]] = pre[keep]
  assert float(out[keep].abs().max()) <= 256 and float(pre[keep].abs().max()) <= 256
  o.update(pre=pre, cmap=cmap, rows=rows, Aeff=Aeff, lda=lda, ldc=ldc)
  return o


def desc_tn_case(M, N, Ki, seed, lda=None, ldb=None, brow=(0, 0)):
  """dW[Ki, N] = C0 + X^T . dY and colsum = cs0 + colsum(dY) over M rows on the integer lane (int_lane_tn), float64 host tensors: X [M, Ki] with +-1 entries,
  dY in [-4, 4], C0 in [-7, 7], cs0 in [-9, 9]; every sum is an integer below 2^24.  brow = (group, skip): dY's rows sit at row_map() of a taller buffer
  whose other rows (the skipped ones and two behind the last) are NaN, as are the pad columns of both operands.  The references are an index_add_ and a
  column sum of the COMPACT dY: the map enters only where the buffer is laid out.
  Keys: X (padded [M, lda]), dY (padded [rows, ldb]), C0, dW [Ki, N], cs0, cs [N]."""
  lda = Ki if lda is None else lda
  ldb = N if ldb is None else ldb
  X, dC, ref, cs = int_lane_tn(M, N, Ki, seed)
  g = torch.Generator().manual_seed(seed + 1)
  C0 = torch.randint(-7, 8, (Ki, N), generator=g).double()
  cs0 = torch.randint(-9, 10, (N,), generator=g).double()
  at = row_map(M, *brow)
  o = dict(X=padded(X, lda), dY=padded(dC, ldb, int(at[-1]) + 3, at), C0=C0, dW=C0 + ref.double(), cs0=cs0, cs=cs0 + cs.double(), lda=lda, ldb=ldb)
  assert_exact_in(o['dW'], torch.float32, 'dW')
  assert_exact_in(o['cs'], torch.float32, 'colsum')
  return o


def linear_bound(A, B, bias, R, act, ref64, pre64, out_dtype):
  """elementwise_bound of C = act(A . B + bias) + R for a test's own operands (act: 0 none, 1 tanh-gelu; pre64 = the fp64 pre-activation)"""
  ap = abs_product(A, B)
  if act:
    return elementwise_bound(ref64, ap, A.shape[1], out_dtype, bias, R, act_err=gelu_act_err(pre64), lipschitz=GELU_LIPSCHITZ)
  return elementwise_bound(ref64, ap, A.shape[1], out_dtype, bias, R)


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_restated(x, scale, dy, dtype):
  """The LayerNorm kernels' arithmetic (csrc/layernorm.hip: mean and E[x^2] - mean^2 clamped at 0, eps 1e-6, r = rsqrt; dx = r (g - mean(g) - xhat mean(g xhat)),
  g = dy scale; dscale = sum over rows of dy xhat) in `dtype` on the host: float32 restates the kernels, float64 is the reference.  -> (y, dx, dscale)"""
  x, scale, dy = x.to(dtype), scale.to(dtype), dy.to(dtype)
  d = x.shape[1]
  mu = x.sum(1, keepdim=True) / d
  var = ((x * x).sum(1, keepdim=True) / d - mu * mu).clamp_min(0)
  r = torch.rsqrt(var + 1e-6)
  xh = (x - mu) * r
  g = dy * scale
  dx = r * (g - g.sum(1, keepdim=True) / d - xh * ((g * xh).sum(1, keepdim=True) / d))
  return xh * scale, dx, (dy * xh).sum(0)


def restated_bound(ref64, host32, out_dtype):
  """u_out |ref| + 4 x max |fp32 host restatement - fp64|: one output rounding (absent for fp32) on top of fp32 arithmetic whose order and rsqrt / division differ
  from the host's by a few ulp"""
  e = 4.0 * float((host32.double() - ref64).abs().max())
  return e if out_dtype == torch.float32 else unit_roundoff(out_dtype) * ref64.abs() + (1.0 + unit_roundoff(out_dtype)) * e


# ------------------------------------------------------------------------------------------------ fused attention forward: host emulation
NEG_BIG = -3.4028234663852886e38   # csrc/attn_common.hpp:14
PROBE_POSITIONS = (0, 1, 15, 16, 31, 32, 63, 64, 127, 128, 159, 160)   # + Sk - 2, Sk - 1 (cross: + 255, 256 and the ragged last chunk's first / last key)


def emulate_attention(q, k, v, sq, sk, km, H, Dh, chunk=None):
  """The fused forward kernels' rounding contract on the host (csrc/attention_fused.hip), everything between two rounding points in fp32 with the sums
  taken exactly (fp64) and rounded once -- an idealised order-free fp32 accumulation:
    * 16-bit q, k, v as given;
    * q^ = 16-bit(x * rsqrt(sum x^2 / Dh + 1e-6) * scale), fp32 inside: frag_norm, lines 91-105 (queries); rows_store<NORM>, lines 69-81 (keys);
    * logits in fp32: the MFMA sum of q^ k^ (lines 158-167), * 1/sqrt(Dh) + key bias (line 174; masked key: + finfo.min, line 142; cross: 294, 321);
    * softmax in fp32: p = exp(s - max), l = sum p (lines 176-183; cross per 128-key chunk: 323-329);
    * self-attention (chunk=None): P = 16-bit(p / l) (line 191), o = 16-bit(fp32 sum of P v) (lines 218-225);
    * cross attention (chunk=128, xattn_fwd_kernel + xattn_combine_kernel): per chunk P_c = 16-bit(p) UNnormalised (line 337), O_c = fp32 sum P_c v
      (line 356), then o = 16-bit((sum_c e^(m_c - M) O_c) / L), L = sum_c e^(m_c - M) l_c (lines 373-391): one output rounding.
  q [nseq, Sq, H Dh], k, v [nseq, Sk, H Dh] in the 16-bit type, scales fp32 [Dh], km [nseq, Sk] or None.  -> o [nseq, Sq, H Dh] in the 16-bit type."""
  dt = q.dtype
  nseq, Sq, _ = q.shape
  Sk = k.shape[1]

  def norm(x, scale):
    f = x.float().reshape(nseq, -1, H, Dh)
    rr = torch.rsqrt((f * f).sum(-1, keepdim=True) / Dh + 1e-6)
    return (f * rr * scale.float()).to(dt)
  qn, kn, vh = norm(q, sq), norm(k, sk), v.reshape(nseq, Sk, H, Dh)
  s = torch.einsum('nqhd,nkhd->nhqk', qn.double(), kn.double()).float() * torch.tensor(0.10206207261596575, dtype=torch.float32)
  if km is not None:
    s = s + torch.where(km == 0, torch.tensor(NEG_BIG, dtype=torch.float32), torch.tensor(0.0))[:, None, None, :]
  vd = vh.double().permute(0, 2, 1, 3)   # [nseq, H, Sk, Dh]
  if chunk is None:
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    P = (p * (1.0 / p.sum(-1, keepdim=True))).to(dt)
    o = (P.double() @ vd).float().to(dt)
  else:
    ms, ls, os_ = [], [], []
    for c0 in range(0, Sk, chunk):
      sc = s[..., c0:c0 + chunk]
      m = sc.max(-1, keepdim=True).values
      p = torch.exp(sc - m)
      ms.append(m); ls.append(p.sum(-1, keepdim=True)); os_.append((p.to(dt).double() @ vd[:, :, c0:c0 + chunk]).float())
    M = torch.stack(ms).max(0).values
    L = sum(l * torch.exp(m - M) for m, l in zip(ms, ls))
    o = (sum(torch.exp(m - M) * oc for m, oc in zip(ms, os_)) * (1.0 / L)).to(dt)
  return o.permute(0, 2, 1, 3).reshape(nseq, Sq, H * Dh)


def attention_row_gate(gates, name, got, emu, ref64, H, Dh):
  """every (sequence, token, head) row of `got` within 2 x the WORST row of the host emulation, both against the fp64 oracle: the kernel differs from the
  emulation only in summation order and in its exp, so its row errors are another sample of the same distribution, and the maximum over thousands of
  rows is a stable statistic.  The bound is the emulation's value, never the kernel's.  Adds one row to the util.Gates table."""
  shp = ref64.shape[:-1] + (H, Dh)
  ke = row_errs(got.reshape(shp), ref64.reshape(shp), -1)
  ee = row_errs(emu.reshape(shp), ref64.reshape(shp), -1)
  worst = tuple(int(i) for i in torch.unravel_index(ke.reshape(-1).argmax(), ke.shape))
  gates.le(f'{name}: worst row error (row {worst})', float(ke.max()), 2.0 * float(ee.max()), f'emulation worst row {float(ee.max()):.3e}')


def probe_positions(Sk, cross=False):
  ps = list(PROBE_POSITIONS) + [Sk - 2, Sk - 1]
  if cross:
    ps += [255, 256, (Sk - 1) // 128 * 128, Sk - 1]
  return sorted({p for p in ps if 0 <= p < Sk})


def probe_inputs(nseq, Sq, Sk, H, Dh, dt, pos, seed):
  """Dominant-key probe: head h of sequence s probes key pos[s][h].  In that head every raw query is a common vector w + 1 % noise and k[pos] = w, so after
  the RMSNorm the probed logit is about sqrt(Dh) = 9.8 against N(0, 1) for the other keys and takes over 90 % of every row's probability; v[pos] is 8 x
  the scale of the other values.  Losing or misplacing that key moves every forward row of the head by O(1).  -> q [nseq, Sq, E], k, v [nseq, Sk, E]"""
  g = torch.Generator().manual_seed(seed)
  w = torch.randn(nseq, 1, H, Dh, generator=g)
  q = w + 0.01 * torch.randn(nseq, Sq, H, Dh, generator=g)
  k = torch.randn(nseq, Sk, H, Dh, generator=g)
  v = torch.randn(nseq, Sk, H, Dh, generator=g)
  for s in range(nseq):
    for h in range(H):
      k[s, pos[s][h], h] = w[s, 0, h]
      v[s, pos[s][h], h] *= 8.0
  E = H * Dh
  return q.reshape(nseq, Sq, E).to(dt), k.reshape(nseq, Sk, E).to(dt), v.reshape(nseq, Sk, E).to(dt)


def cross_attention_ws_bytes(nseq, H, Sq, Sk):
  """what the fused cross attention carves from its workspace (csrc/attn_plan.hpp: AttnPlan::part_bytes of the XFwd* / XBwd* routes): per (sequence, head, 128-key chunk) an
  fp32 [Sq, 96] partial and an [Sq, 2] (max, sum) pair in the forward, an fp32 [Sq, 96] dq^ partial in the backward; each released before the next call"""
  return nseq * H * ((Sk + 127) // 128) * Sq * (96 + 2) * 4 + (64 << 10)


def gate_linear_bwd(A, B, dC, dA, dB, db, rA, rB, rb, dt):
  """element-wise gates of a Dense backward (tests/parity_util.py): dA = dC . B^T is one rounding to `dt` of an fp32 sum over N; dB = A^T . dC and
  dbias = colsum(dC) are fp32 sums over M in any order (tiles, splits, atomics)"""
  if dA is not None:
    assert_elementwise(dA, rA, elementwise_bound(rA, abs_product(dC, B.t()), dC.shape[1], dt), 'dA')
  if dB is not None:
    assert_elementwise(dB, rB, elementwise_bound(rB, abs_product(A.t(), dC), A.shape[0], torch.float32), 'dB')
  if db is not None:
    assert_elementwise(db, rb, elementwise_bound(rb, dC.double().abs().sum(0), dC.shape[0], torch.float32), 'dbias')


# ------------------------------------------------------------------------------------------------ fused attention backward: host emulation
def _rmsnorm16(x, scale, nseq, H, Dh):
  f = x.float().reshape(nseq, -1, H, Dh)
  rr = torch.rsqrt((f * f).sum(-1, keepdim=True) / Dh + 1e-6)
  return (f * rr * scale.float()).to(x.dtype)


def _rmsnorm_bwd(x, scale, g, Dh, dt):
  """RMSNorm backward as the kernels state it (csrc/attention_fused.hip:626-656 for q, 736-766 for k, 411-419 for the cross dq): x the raw 16-bit row, g the fp32
  gradient of the normalised row.  rr = rsqrt(sum x^2 / Dh + 1e-6), xh = x rr, gx = sum(g scale xh) / Dh, dx = 16-bit(rr (g scale - xh gx)); the row's
  contribution to dscale is g xh (fp32).  x, g [..., Dh] -> (dx in dt, dscale fp32 [Dh] summed over every row, exactly)"""
  f = x.float()
  rr = torch.rsqrt((f * f).sum(-1, keepdim=True) / Dh + 1e-6)
  xh = f * rr
  sc = scale.float()
  gx = (g * sc * xh).double().sum(-1, keepdim=True).float() / Dh
  dx = (rr * (g * sc - xh * gx)).to(dt)
  return dx, (g * xh).double().reshape(-1, Dh).sum(0).float()


def emulate_attention_bwd(q, k, v, sq, sk, km, H, Dh, d_o, chunk=None, fast=False):
  """The fused backward kernels' rounding contract on the host (csrc/attention_fused.hip), sums taken exactly and rounded once to fp32 as in emulate_attention.
  All three self-attention structures (attn_bwd8_kernel, attn_bwd_split_kernel on 4 / 8 waves) and the cross form run the same two tile routines:
    * q^, k^ = 16-bit RMSNorm rows as in the forward (rows_store<NORM>, lines 69-81; frag_norm, 91-105); v, dO and the forward's o in 16 bits;
    * row statistics from the forward: m and log l in fp32 (lse, lines 184 / 392; read at 900-903, 1082); delta = fp32 sum(dO o) over the 16-bit o
      (store_do_delta, lines 784-793);
    * S = fp32 sum q^ k^ and dP = fp32 sum dO v (lines 580-581, 690-691);
    * masked arithmetic (a key mask, every split-pass launch, the cross form): p = exp((S alpha + bias - m) - log l) (lines 590, 706),
      dS = 16-bit(p (dP - delta) alpha) for a visible key, 0 for a masked one (lines 591-592, 708), P = 16-bit(p) (line 707);
    * fast arithmetic (fast=True: attn_bwd8_kernel without a key mask, lines 1131-1132): S starts at -(m + log l) / alpha and dP at -delta (lines 575, 685, 902),
      p = exp2(S alpha log2 e) (lines 587, 696), dS = 16-bit(p (dP - delta)) WITHOUT alpha (lines 588, 698), alpha applied to the fp32 sums (lines 632, 742);
    * dq^ = fp32 sum_keys dS k^ (lines 599-618; cross: fp32 partials per 128-key chunk, line 622, summed in xattn_dq_finish_kernel, line 410),
      dk^ = fp32 sum_queries dS q^ and dv = 16-bit(fp32 sum_queries P dO) (lines 729-730, 771);
    * dq, dk = 16-bit RMSNorm backward of dq^, dk^ on the raw rows, dscale_q / dscale_k += dq^ xh, dk^ xh in fp32 (lines 626-656, 736-766, 411-419).
  `chunk` only selects the forward emulation that supplies o.  -> (dq, dk, dv in the 16-bit type, dsq, dsk fp32 [Dh])"""
  dt = q.dtype
  nseq, Sq, _ = q.shape
  Sk = k.shape[1]
  alpha = torch.tensor(0.10206207261596575, dtype=torch.float32)
  qn, kn = _rmsnorm16(q, sq, nseq, H, Dh), _rmsnorm16(k, sk, nseq, H, Dh)            # [nseq, S, H, Dh]
  qd, kd = qn.double().permute(0, 2, 1, 3), kn.double().permute(0, 2, 1, 3)          # [nseq, H, S, Dh]
  vd = v.reshape(nseq, Sk, H, Dh).double().permute(0, 2, 1, 3)
  dod = d_o.reshape(nseq, Sq, H, Dh).double().permute(0, 2, 1, 3)
  o = emulate_attention(q, k, v, sq, sk, km, H, Dh, chunk).reshape(nseq, Sq, H, Dh).double().permute(0, 2, 1, 3)
  s = (qd @ kd.transpose(-1, -2)).float()
  bias = torch.zeros(nseq, 1, 1, Sk)
  if km is not None:
    bias = torch.where(km == 0, torch.tensor(NEG_BIG, dtype=torch.float32), torch.tensor(0.0))[:, None, None, :]
  sl = s * alpha + bias
  m = sl.max(-1, keepdim=True).values
  logl = torch.log(torch.exp(sl - m).sum(-1, keepdim=True))
  delta = (dod * o).sum(-1, keepdim=True).float()
  dp = (dod @ vd.transpose(-1, -2)).float()
  if fast:
    assert km is None
    p = torch.exp2((s - (m + logl) * torch.tensor(9.797958971132712, dtype=torch.float32)) * (alpha * torch.tensor(1.4426950408889634, dtype=torch.float32)))
    ds = (p * (dp - delta)).to(dt).double()
    post = alpha
  else:
    p = torch.exp((sl - m) - logl)
    ds = torch.where(bias == 0, p * (dp - delta) * alpha, torch.zeros(())).to(dt).double()
    post = torch.tensor(1.0)
  dqh = (ds @ kd).float() * post                      # [nseq, H, Sq, Dh]
  dkh = (ds.transpose(-1, -2) @ qd).float() * post    # [nseq, H, Sk, Dh]
  dv = (p.to(dt).double().transpose(-1, -2) @ dod).float().to(dt)
  E = H * Dh
  dq, dsq = _rmsnorm_bwd(q.reshape(nseq, Sq, H, Dh), sq, dqh.permute(0, 2, 1, 3), Dh, dt)
  dk, dsk = _rmsnorm_bwd(k.reshape(nseq, Sk, H, Dh), sk, dkh.permute(0, 2, 1, 3), Dh, dt)
  return dq.reshape(nseq, Sq, E), dk.reshape(nseq, Sk, E), dv.permute(0, 2, 1, 3).reshape(nseq, Sk, E), dsq, dsk


def grad_row_floor(dtype, Dh, S, c=C_MFMA):
  """The fraction of a typical row below which a gradient row is judged absolutely (row_errs_floored): c sqrt(2 Dh S) 2^-24 / u_out.  A row whose reference
  is zero (a query or key of a sequence with one visible key: the softmax passes no gradient) is not an exact zero in a kernel: dP - delta is the difference of two
  fp32 sums of the same Dh products taken in different orders, and S such residues (one per query, or per key) add into the row -- a random walk of 2 Dh S fp32
  roundings of terms the size of a typical row's, i.e. an absolute noise of about sqrt(2 Dh S) 2^-24 typical rows, c = 4 as in elementwise_bound.  The gate resolves
  relative errors of about u_out, so rows smaller than noise / u_out of a typical row cannot be judged relatively.  bf16, S = 301: 1.5 %; fp16: 12 %."""
  return c * math.sqrt(2.0 * Dh * S) * U_F32 / unit_roundoff(dtype)


def row_errs_floored(got, ref64, floor, dim=-1):
  """row_errs with the denominator max(||ref row||, floor x the RMS row norm of the tensor): a gradient row whose reference is zero or nearly so (a query with
  one visible key has dq = 0 exactly in the oracle) is judged absolutely, against `floor` (grad_row_floor) of a typical row, instead of dividing by nothing.
  The emulation takes its sums exactly and has none of the kernels' fp32 cancellation noise there, so its own error in such a row is 0 and cannot serve as the
  yardstick; a typical row can"""
  g, r = got.detach().double().cpu(), ref64.double()
  n = r.norm(dim=dim)
  return (g - r).norm(dim=dim) / torch.clamp(n, min=floor * float((n * n).mean().sqrt()) + 1e-300)


def attention_grad_gates(gates, got, emu, ref, H, Dh, S=None):
  """The backward half of the row gate.  got / emu / ref: (dq, dk, dv, dsq, dsk) of the kernel, of emulate_attention_bwd and of the fp64 oracle.  Every
  (sequence, token, head) row of dq, dk, dv and the whole vectors dsq, dsk within 2 x the emulation's worst, rows by row_errs_floored.  S: the longest
  sequence (queries or keys) where the tensors are ragged sequences' rows concatenated [rows, E] and their shape does not say it."""
  floor = grad_row_floor(emu[0].dtype, Dh, max(ref[0].shape[1], ref[1].shape[1]) if S is None else S)
  for name, g, e, r in zip(('dq', 'dk', 'dv'), got[:3], emu[:3], ref[:3]):
    shp = r.shape[:-1] + (H, Dh)
    ke = row_errs_floored(g.reshape(shp), r.reshape(shp), floor)
    ee = row_errs_floored(e.reshape(shp), r.reshape(shp), floor)
    worst = tuple(int(i) for i in torch.unravel_index(ke.reshape(-1).argmax(), ke.shape))
    gates.le(f'{name}: worst row error (row {worst})', float(ke.max()), 2.0 * float(ee.max()), f'emulation worst row {float(ee.max()):.3e}')
  for name, g, e, r in zip(('dsq', 'dsk'), got[3:], emu[3:], ref[3:]):
    ke, ee = float(row_errs(g.reshape(1, -1), r.reshape(1, -1))[0]), float(row_errs(e.reshape(1, -1), r.reshape(1, -1))[0])
    gates.le(f'{name}: error of the whole vector', ke, 2.0 * ee, f'emulation {ee:.3e}')


# ------------------------------------------------------------------------------------------------ generic 16-bit attention composition: host emulation
def emulate_attention_generic(q, k, v, sq, sk, km, H, Dh, d_o):
  """The generic composition in a 16-bit type (csrc/attention.hip:42-129: GEMM + row kernels, every intermediate stored in 16 bits), sums exact and rounded once:
    * q^, k^ = 16-bit(x r scale) (rms_heads_fwd_kernel, csrc/attention.hip);
    * S = 16-bit(alpha fp32 sum q^ k^) (scores(), attention.hip:31-40, alpha = 1 / sqrtf(Dh) in the GEMM epilogue);
    * P = 16-bit(exp(S - max) / sum) in fp32 on the stored S, a masked key read as finfo.min (softmax_kernel, attention.hip);
    * o = 16-bit(fp32 sum P v) (attention.hip:61-66);
    * dP = 16-bit(fp32 sum dO v) (attention.hip:96-102), dv = 16-bit(fp32 sum P dO) (103-109);
    * dS = 16-bit(P (dP - fp32 sum(P dP))), 0 for a masked key (softmax_bwd_kernel, attention.hip);
    * dq^ = 16-bit(alpha fp32 sum dS k^), dk^ = 16-bit(alpha fp32 sum dS q^) (attention.hip:111-124);
    * dq, dk = 16-bit(r (g - xh mean(g xh))), g = dq^ scale, and dscale += dq^ xh in fp32 (rms_heads_bwd_kernel, attention.hip).
  -> (o, dq, dk, dv in the 16-bit type, dsq, dsk fp32 [Dh])"""
  dt = q.dtype
  nseq, Sq, _ = q.shape
  Sk = k.shape[1]
  alpha = torch.tensor(1.0 / math.sqrt(Dh), dtype=torch.float32)
  qn, kn = _rmsnorm16(q, sq, nseq, H, Dh), _rmsnorm16(k, sk, nseq, H, Dh)
  qd, kd = qn.double().permute(0, 2, 1, 3), kn.double().permute(0, 2, 1, 3)
  vd = v.reshape(nseq, Sk, H, Dh).double().permute(0, 2, 1, 3)
  dod = d_o.reshape(nseq, Sq, H, Dh).double().permute(0, 2, 1, 3)
  s = ((qd @ kd.transpose(-1, -2)).float() * alpha).to(dt).float()
  vis = torch.ones(nseq, 1, 1, Sk, dtype=torch.bool) if km is None else (km != 0)[:, None, None, :]
  s = torch.where(vis, s, torch.tensor(NEG_BIG, dtype=torch.float32))
  e = torch.exp(s - s.max(-1, keepdim=True).values)
  P = (e * (1.0 / e.sum(-1, keepdim=True))).to(dt).double()
  o = (P @ vd).float().to(dt)
  dP = (dod @ vd.transpose(-1, -2)).float().to(dt).float()
  dv = (P.transpose(-1, -2) @ dod).float().to(dt)
  rs = (P * dP.double()).sum(-1, keepdim=True).float()
  dS = torch.where(vis, P.float() * (dP - rs), torch.zeros(())).to(dt).double()
  dqh = ((dS @ kd).float() * alpha).to(dt).float().permute(0, 2, 1, 3)
  dkh = ((dS.transpose(-1, -2) @ qd).float() * alpha).to(dt).float().permute(0, 2, 1, 3)
  dq, dsq = _rmsnorm_bwd(q.reshape(nseq, Sq, H, Dh), sq, dqh, Dh, dt)
  dk, dsk = _rmsnorm_bwd(k.reshape(nseq, Sk, H, Dh), sk, dkh, Dh, dt)
  E = H * Dh
  back = lambda t, S: t.permute(0, 2, 1, 3).reshape(nseq, S, E)
  return back(o, Sq), dq.reshape(nseq, Sq, E), dk.reshape(nseq, Sk, E), back(dv, Sk), dsq, dsk


# ------------------------------------------------------------------------------------------------ single-query attention and sums by float atomics
def sequential_sum(first, addends, dtype):
  """first + addends[0] + addends[1] + ... taken one addend after the other in `dtype` (float32: what a chain of float atomics does, in one of its possible
  orders; numpy's accumulate neither widens nor sums pairwise, torch's cumsum would accumulate float32 in double).  first [d], addends [n, d] -> [d]"""
  import numpy as np
  npdt = {torch.float32: np.float32, torch.float64: np.float64}[dtype]
  a = np.concatenate([first.detach().cpu().numpy().astype(npdt)[None], addends.detach().cpu().numpy().astype(npdt)], 0)
  return torch.from_numpy(np.add.accumulate(a, axis=0)[-1].copy())


def arrival_orders(n, d, samples=128):
  """Row orders in which to restate a sum of n addends that a kernel takes by float atomics, for a result of d elements: the given order, its reverse, then
  seeded random permutations -- ceil(samples / d) orders in all.  The atomics' arrival order is not fixed, so every order is as much the restatement as any
  other, and "the restatement's own worst error" (the gate is 4 x that) is the worst over the elements of all of them.  One order is enough for a wide result;
  for a narrow one (8 columns) the worst of 8 rounding-noise samples is itself noise -- it falls below a quarter of the typical worst about once in a hundred
  draws, and a correct kernel then fails -- so narrow results take more orders until at least `samples` = 128 elements enter the maximum."""
  count = max(1, -(-samples // d))
  yield torch.arange(n)
  if count > 1:
    yield torch.arange(n - 1, -1, -1)
  for i in range(2, count):
    yield torch.randperm(n, generator=torch.Generator().manual_seed(i))


def attn_q1_restated(q0, k, v, sq, sk, km, H, Dh, d_o, dtype):
  """Single-query attention (track_autoencoder_3d.py:187-188, 286: token 0 of each sequence queries, every token is a key) and its gradients, written out in
  `dtype` on the host: float32 is the restatement that sets the 16-bit gates, float64 must equal the oracle's autograd (tests/test_parity_gates_host.py).
  x^ = x rsqrt(mean x^2 + 1e-6); q^ = x^_q s_q; logit_j = q^ . (x^_j s_k) / sqrt(Dh), finfo.min for a masked key; p = softmax; o = sum p_j v_j.
  Backward: dp_j = dO . v_j; ds_j = p_j (dp_j - sum p dp) / sqrt(Dh), 0 for a masked key; dv_j = p_j dO; dk^_j = ds_j q^ and u = sum ds_j x^_j give
  dq^ = u s_k, ds_k = q^ u, ds_q = dq^ x^_q; a row's gradient through the RMSNorm is r (g - x^ mean(g x^)) with g = d(normalised row) x scale.
  q0, d_o [n, H Dh]; k, v [n, S, H Dh]; km [n, S] or None.  -> o [n, H Dh], p [n, H, S], dq [n, H Dh], dk, dv [n, S, H Dh] and the scale gradients of every
  (sequence, head) problem, csq, csk [n H, Dh] in problem order (to be summed as the kernel's atomics sum them: sequential_sum)."""
  n, S = k.shape[0], k.shape[1]
  x = q0.to(dtype).reshape(n, H, Dh)
  kk, vv = k.to(dtype).reshape(n, S, H, Dh), v.to(dtype).reshape(n, S, H, Dh)
  do = d_o.to(dtype).reshape(n, H, Dh)
  sq, sk = sq.to(dtype), sk.to(dtype)
  alpha = torch.tensor(1.0 / math.sqrt(Dh), dtype=dtype)
  rq = torch.rsqrt((x * x).sum(-1, keepdim=True) / Dh + 1e-6)
  xq = x * rq
  qh = xq * sq
  rk = torch.rsqrt((kk * kk).sum(-1, keepdim=True) / Dh + 1e-6)
  xk = kk * rk
  lg = torch.einsum('nhd,nshd->nhs', qh, xk * sk) * alpha
  keep = torch.ones(n, 1, S, dtype=torch.bool) if km is None else (km != 0)[:, None, :]
  lg = torch.where(keep, lg, torch.full_like(lg, torch.finfo(dtype).min))
  p = torch.softmax(lg, -1)
  o = torch.einsum('nhs,nshd->nhd', p, vv)
  dp = torch.einsum('nhd,nshd->nhs', do, vv)
  ds = torch.where(keep, p * (dp - (p * dp).sum(-1, keepdim=True)) * alpha, torch.zeros((), dtype=dtype))
  dv = torch.einsum('nhs,nhd->nshd', p, do)
  u = torch.einsum('nhs,nshd->nhd', ds, xk)
  gk = torch.einsum('nhs,nhd->nshd', ds, qh) * sk
  dk = rk * (gk - xk * ((gk * xk).sum(-1, keepdim=True) / Dh))
  dqh = u * sk
  gq = dqh * sq
  dq = rq * (gq - xq * ((gq * xq).sum(-1, keepdim=True) / Dh))
  E = H * Dh
  return o.reshape(n, E), p, dq.reshape(n, E), dk.reshape(n, S, E), dv.reshape(n, S, E), (dqh * xq).reshape(n * H, Dh), (qh * u).reshape(n * H, Dh)
