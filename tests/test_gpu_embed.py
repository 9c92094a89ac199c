"""GPU parity of the first mile of the model on its own, through the spa3d_op_* entry points of csrc/ops.hip: the sinusoidal, token and query embeddings, the
row maps of the one-pass embedding, the readout rows, both key masks, the weight shadows (sum3, pack, transpose) of csrc/embed.hip and the latent quantiser of
csrc/loss.hip.  References: tests/embed_util.py (checked in tests/test_embed_ref_host.py, where the refusals are made too).

Every output lives in a parity_util.guarded() allocation pre-filled with embed_util.SENTINEL and check_guards() runs after every case; whatever an
operation does not own inside its output (the element before an offset output, the token rows embed_maps and set_readout_rows skip) must still hold the
sentinel, and the padding between a row's width and its leading dimension is canary checked by the guards.

  embeddings   fp32 within 5e-7 of the float64 sine of the float32 arguments (the bound of test_gpu_ops.py::test_sin_embed_matches_oracle_and_kat for two
               libm sinf's); 16-bit within u |ref| + 5e-7, plus fp16's subnormal spacing where |ref| < 2^-14; NaN exactly where the reference has one
  integers, masks, copies, casts, sum3, the quantiser   bit for bit

`embed branch:` lines name the kernel a token-embedding case took (the launcher's own condition, restated here).  Added to the issue's lists because no
listed case reaches the branch: query times -2.5 and -7 (floor differs from truncation only below zero), and pack in fp32 (the entry point takes it)."""
import ctypes as C

import numpy as np
import pytest
import torch

import embed_util as EU
import parity_util as PU
import rows_util as RU
from util import O

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2
DTYPES = [F32, BF16, F16]
f32 = np.float32


@pytest.fixture(scope='module')
def lib():
  import spa3d
  return spa3d._lib.load()


def _s():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(dtype):
  return {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}[dtype]


def _bits(t):
  t = t.detach().cpu().contiguous()
  return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
  return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _out(rows, cols, dt, name, ld=None):
  return PU.guarded(rows, cols, dt, ld=ld, name=name, fill=EU.SENTINEL)


def _is_sentinel(t):
  return bool(torch.all(_bits(t) == _bits(torch.full((1,), EU.SENTINEL).to(t.dtype))[0])) if t.numel() else True


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sin_gate(got, ref64, dt, what):
  """NaN exactly where the reference has one; elsewhere the bound of the module docstring"""
  got = got.detach().cpu()
  ref = torch.from_numpy(np.ascontiguousarray(ref64)).reshape(got.shape)
  nan = torch.isnan(ref)
  assert torch.equal(torch.isnan(got.float()), nan), f'{what}: NaN positions differ from the reference'
  ref = torch.where(nan, 0.0, ref)      # the NaN positions are settled: they take no part in the bound
  bound = torch.full_like(ref, 5e-7)
  if dt != torch.float32:
    bound = bound + PU.unit_roundoff(dt) * ref.abs()
  if dt == torch.float16:
    bound = bound + torch.where(ref.abs() < 2.0 ** -14, 2.0 ** -24, 0.0)
  PU.assert_elementwise(torch.where(nan, 0.0, got.double()), ref, bound, what)


# ================================================================================================ token and sinusoidal embeddings
TOKEN_SHAPES = [(1, 1), (5, 7), (3, 150), (2, 129)]   # (nseq, T): T does not divide 256, the vector groups of a row straddle workgroups


def _tracks(nrows, NC, seed):
  x = (np.random.default_rng(seed).random((nrows, NC)) * 2 - 0.5).astype(f32)
  if nrows >= 3:
    x[1] = 0.0
    x[2, 0], x[2, 1] = np.nan, np.inf
  return x


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nf', [32, 8, 64, 12, 5])
def test_embed_tokens(lib, dtype, nf):
  dt = _dt(dtype)
  es = 4 if dtype == F32 else 2
  nv = 16 // es
  assert (nf % nv == 0) == {32: True, 8: True, 64: True, 12: dtype == F32, 5: False}[nf]   # the path the aligned call takes
  for NC in (2, 3):
    for prescale in (1.0, 3.0):
      for nseq, T in TOKEN_SHAPES:
        nrows, W = nseq * T, (NC + 1) * 2 * nf
        x = _tracks(nrows, NC, 1000 * nf + 10 * NC + T)
        xd = _dev(x)
        ref = EU.embed_tokens_ref(x, T, nf, prescale)
        out = _out(nrows, W, dt, 'embed_tokens out')
        assert out.data_ptr() % 16 == 0
        assert lib.spa3d_op_embed_tokens(xd.data_ptr(), nrows, T, NC, nf, prescale, out.data_ptr(), dtype, _s()) == 0
        off = _out(1, nrows * W + 1, dt, 'embed_tokens out + 1 element')
        assert lib.spa3d_op_embed_tokens(xd.data_ptr(), nrows, T, NC, nf, prescale, off.data_ptr() + es, dtype, _s()) == 0
        PU.check_guards()
        tag = f'{dt} NC {NC} nf {nf} prescale {prescale} nseq {nseq} T {T}'
        print(f'  embed branch: embed_tokens {tag} -> {"vector" if nf % nv == 0 else "scalar"}; offset by one element -> scalar')
        got = out.cpu()
        _sin_gate(got, ref, dt, f'GATE embed_tokens {tag}')
        # the source's claim: both kernels give the same bits
        offc = off.cpu()
        assert _is_sentinel(offc[0, :1]), f'the element before the offset output was written: {tag}'
        assert _same_bits(offc[0, 1:].reshape(nrows, W), got), f'scalar and vector kernels differ: {tag}'
        # the time coordinate depends on r % T alone, and t = 0 is the zero-input pattern
        tcol = got[:, NC * 2 * nf:]
        if nseq > 1:
          assert _same_bits(tcol[:nrows - T], tcol[T:]), f'time columns of rows r and r + T differ: {tag}'
        for r in range(0, nrows, T):
          assert bool(torch.all(tcol[r, :nf] == 0)) and _same_bits(tcol[r, nf:], tcol[0, nf:].clone()), f'time columns at t = 0: {tag}'
        one = float(np.sin(np.float64(EU.HALF_PI)))
        assert float((tcol[0, nf:].double() - one).abs().max()) <= 5e-7 + (0 if dtype == F32 else PU.unit_roundoff(dt))
        if nrows >= 3:   # the all-zero track row: zeros and sin(fl32(pi / 2)) in every track coordinate
          z = got[1, :NC * 2 * nf].reshape(NC, 2 * nf)
          assert bool(torch.all(z[:, :nf] == 0)) and _same_bits(z[:, nf:], tcol[0, nf:].expand(NC, nf).contiguous())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nf', [32, 5])
def test_sin_embed_16_bit_outputs_and_prescale(lib, dtype, nf):
  """spa3d_op_sin_embed in the 16-bit types (its fp32 test is test_gpu_ops.py's), and its sibling with the model's division in all three"""
  dt = _dt(dtype)
  for Cc in (1, 3):
    for rows in (1, 257):
      x = (np.random.default_rng(rows + Cc + nf).random((rows, Cc)) * 2 - 0.5).astype(f32)
      x[0] = 0.0
      xd = _dev(x)
      W = Cc * 2 * nf
      if dtype != F32:
        out = _out(rows, W, dt, 'sin_embed out')
        assert lib.spa3d_op_sin_embed(xd.data_ptr(), rows, Cc, nf, out.data_ptr(), dtype, _s()) == 0
        PU.check_guards()
        _sin_gate(out, EU.sin_embed_ref(x, nf), dt, f'GATE sin_embed {dt} C {Cc} nf {nf} rows {rows}')
        row = out[0].cpu().reshape(Cc, 2 * nf)
        assert bool(torch.all(row[:, :nf] == 0)) and float((row[:, nf:].double() - 1.0).abs().max()) <= PU.unit_roundoff(dt)
      for prescale in (3.0, 0.7):
        out = _out(rows, W, dt, 'sin_embed_scaled out')
        assert lib.spa3d_op_sin_embed_scaled(xd.data_ptr(), rows, Cc, nf, prescale, out.data_ptr(), dtype, _s()) == 0
        PU.check_guards()
        _sin_gate(out, EU.sin_embed_ref(x, nf, prescale), dt, f'GATE sin_embed_scaled {dt} C {Cc} nf {nf} rows {rows} prescale {prescale}')


# ================================================================================================ query embedding
QUERY_TIMES = [0.5, 1.5, 2.5, 3.5, -0.5, 2.4999998, 2.5000002, 149.0, 6.0, -2.5, -7.0, 0.0, 7.49, 148.5, 3.0]


@pytest.mark.parametrize('NC', [2, 3])
@pytest.mark.parametrize('nf', [32, 5])
def test_query_embed(lib, NC, nf):
  for nq in (1, 255, 257, 1000):
    for k, time_scale in enumerate((1.0, 4.0, 3.0)):
      track_scale = (1.0, 3.0)[k % 2]
      rng = np.random.default_rng(nq + k)
      qp = (rng.random((nq, NC + 1)) * 2 - 0.5).astype(f32)
      qp[:, 0] = np.array([QUERY_TIMES[(i + k) % len(QUERY_TIMES)] for i in range(nq)], f32)
      if nq > 20:
        qp[20:, 0] += rng.integers(0, 140, nq - 20).astype(f32)     # the same fractions at other frames
      W = NC * 2 * nf + 1
      feat = _out(nq, W, torch.float32, 'query feat')
      qframe = _out(nq, 1, torch.int32, 'query frame')
      qd = _dev(qp)
      assert lib.spa3d_op_query_embed(qd.data_ptr(), nq, NC, nf, track_scale, time_scale, feat.data_ptr(), qframe.data_ptr(), _s()) == 0
      PU.check_guards()
      sin, tfeat, qf = EU.query_embed_ref(qp, nf, track_scale, time_scale)
      tag = f'NC {NC} nf {nf} nq {nq} time_scale {time_scale} track_scale {track_scale}'
      got = feat.cpu()
      assert np.array_equal(qframe.cpu().numpy()[:, 0], qf), f'query frames: {tag}'
      assert _same_bits(got[:, W - 1], torch.from_numpy(tfeat)), f'time feature: {tag}'
      _sin_gate(got[:, :W - 1], sin, torch.float32, f'GATE query_embed {tag}')


# ================================================================================================ row maps and readout rows
def _pruned_plan(target, T, seed):
  """row_src of a random mask that keeps every readout token and, in sequence 1, nothing else; cut to `target` rows (a prefix of a plan is a plan)"""
  S = T + 1
  nseq = target // max(1, T // 2) + 3
  while True:
    rng = np.random.default_rng(seed + nseq)
    km = (rng.random((nseq, S)) < 0.5).astype(f32)
    km[:, 0] = 1.0
    km[1, 1:] = 0.0
    _, _, row_src, kept = RU.prune_plan_ref(km)
    if kept >= target:
      return row_src[:target].copy()
    nseq += 1


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('d', [384, 40])
def test_embed_maps(lib, dtype, d):
  dt = _dt(dtype)
  ro = torch.randn(d, generator=torch.Generator().manual_seed(d))
  rod = ro.cuda()
  for T in (1, 7, 150):
    S = T + 1
    for rows in (1, 255, 257, 1001):
      for pruned in (False, True):
        row_src = _pruned_plan(rows, T, 7 * T + rows) if pruned else None
        src_d = _dev(row_src) if pruned else None
        arow = _out(rows, 1, torch.int32, 'arow')
        crow = _out(rows, 1, torch.int32, 'crow')
        tok = _out(rows, d, dt, 'tok')
        assert lib.spa3d_op_embed_maps(src_d.data_ptr() if pruned else None, rows, S, T, arow.data_ptr(), crow.data_ptr(), tok.data_ptr(), rod.data_ptr(), d,
                                       dtype, _s()) == 0
        PU.check_guards()
        ra, rc, is_ro = EU.embed_maps_ref(row_src, rows, S, T)
        tag = f'{dt} d {d} T {T} rows {rows} {"pruned" if pruned else "dense"}'
        assert np.array_equal(arow.cpu().numpy()[:, 0], ra), f'arow: {tag}'
        assert np.array_equal(crow.cpu().numpy()[:, 0], rc), f'crow: {tag}'
        got = tok.cpu()
        m = torch.from_numpy(is_ro)
        assert _same_bits(got[m], ro.to(dt).expand(int(m.sum()), d).contiguous()), f'readout rows: {tag}'
        assert _is_sentinel(got[~m]), f'a frame token row was written: {tag}'


@pytest.mark.parametrize('dtype', DTYPES)
def test_set_readout_rows(lib, dtype):
  dt = _dt(dtype)
  for nseq, S, d in ((1, 2, 384), (5, 8, 40), (37, 151, 384)):
    ro = torch.randn(d, generator=torch.Generator().manual_seed(S))
    rod = ro.cuda()
    tok = _out(nseq * S, d, dt, 'tok')
    assert lib.spa3d_op_set_readout_rows(tok.data_ptr(), rod.data_ptr(), nseq, S, d, dtype, _s()) == 0
    PU.check_guards()
    got = tok.cpu().reshape(nseq, S, d)
    assert _same_bits(got[:, 0], ro.to(dt).expand(nseq, d).contiguous()), f'readout rows {dt} {(nseq, S, d)}'
    assert _is_sentinel(got[:, 1:]), f'a row after the readout row was written {dt} {(nseq, S, d)}'


# ================================================================================================ key masks
VIS_VALUES = np.array([0.0, 1.0, -0.0, 0.5, -1.0, np.nan], f32)


@pytest.mark.parametrize('N', [1, 3, 10])
@pytest.mark.parametrize('T', [1, 7, 150])
def test_keymask_both_forms(lib, N, T):
  B = 3
  nseq = B * N
  rng = np.random.default_rng(100 * N + T)
  special = VIS_VALUES[rng.integers(0, len(VIS_VALUES), (nseq, T))]
  binary = (rng.random((nseq, T)) < 0.6).astype(f32)
  for vis in (special, binary):
    for boundary in ([0, T, T + 5], [-1, max(T // 2, 1), T], [T // 3, 0, T - 1]):
      vd, bd = _dev(vis), _dev(np.array(boundary, np.int32))
      for with_readout in (1, 0):
        cols = T + 1 if with_readout else T
        km = _out(nseq, cols, torch.float32, 'km')
        assert lib.spa3d_op_keymask(vd.data_ptr(), bd.data_ptr(), nseq, N, T, with_readout, km.data_ptr(), _s()) == 0
        PU.check_guards()
        got = km.cpu()
        tag = f'N {N} T {T} boundary {boundary} with_readout {with_readout}'
        assert _same_bits(got, torch.from_numpy(EU.keymask_ref(vis, boundary, N, with_readout))), f'key mask: {tag}'
        if vis is binary:
          v5, b = torch.from_numpy(vis).reshape(B, N, T, 1), torch.tensor(boundary, dtype=torch.int32)
          want = O.TrackAutoEncoder3D.key_mask(v5, b).reshape(nseq, T + 1).float()
          assert torch.equal(got, want if with_readout else want[:, 1:].contiguous()), f'key mask against the oracle: {tag}'


# ================================================================================================ weight shadows
@pytest.mark.parametrize('n', [1, 255, 257, 384])
def test_sum3_every_null_pattern(lib, n):
  rng = np.random.default_rng(n)
  ops = [rng.standard_normal(n).astype(f32) * f32(10.0 ** (i - 1)) for i in range(3)]
  devs = [_dev(o) for o in ops]
  for pat in range(1, 8):
    use = [bool(pat >> i & 1) for i in range(3)]
    out = _out(1, n, torch.float32, 'sum3 out')
    assert lib.spa3d_op_sum3(*[dv.data_ptr() if u else None for dv, u in zip(devs, use)], out.data_ptr(), n, _s()) == 0
    PU.check_guards()
    ref = EU.sum3_ref(*[o if u else None for o, u in zip(ops, use)])
    assert _same_bits(out.cpu()[0], torch.from_numpy(ref)), f'sum3 n {n} operands {use}'


def _planted(dt):
  """values exactly halfway between two neighbours of the 16-bit type, the lower neighbour even (ties to it) and odd (ties away from it), both signs;
  fp16: the overflow threshold 65520 (halfway between the largest finite value and 2^16: to infinity), its neighbour below, subnormal ties"""
  h = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11      # half a spacing at 1.0
  v = [1.0 + h, 1.0 + 3 * h, -1.0 - h, -1.0 - 3 * h, 2.0 + 2 * h, 0.5 + 1.5 * h, 1.0 + h * (1 + 2.0 ** -12), 1.0 + h * (1 - 2.0 ** -12)]
  if dt == torch.float16:
    v += [65520.0, -65520.0, 65519.996, 2.0 ** -25, 3 * 2.0 ** -25, 5 * 2.0 ** -25, -3 * 2.0 ** -25, 2.0 ** -24, 1.5 * 2.0 ** -14]
  return torch.tensor(v, dtype=torch.float32)


PACK_SHAPES = [(1, 1), (31, 33), (32, 32), (33, 31), (65, 130), (4, 384)]


def _pack_src(rows, cols, src_ld, dt, seed):
  g = torch.Generator().manual_seed(seed)
  src = torch.randn(rows, src_ld, generator=g)
  if dt != torch.float32:
    p = _planted(dt)
    idx = torch.randperm(rows * cols, generator=g)[:len(p)]
    src[idx // cols, idx % cols] = p[:len(idx)]
  return src


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows,cols', PACK_SHAPES)
def test_pack(lib, dtype, rows, cols):
  dt = _dt(dtype)
  for src_ld in (cols, cols + 3):
    src = _pack_src(rows, cols, src_ld, dt, rows * 1000 + cols + src_ld)
    srcd = src.cuda()
    want_n, want_t = EU.pack_ref(src, cols, dt)
    for ldn in (cols, cols + 8):
      for ldt in (rows, rows + 8):
        for native, transposed in ((True, False), (False, True), (True, True)):
          dn = _out(rows, cols, dt, 'pack native', ld=ldn)
          dT = _out(cols, rows, dt, 'pack transposed', ld=ldt)
          assert lib.spa3d_op_pack(srcd.data_ptr(), src_ld, rows, cols, dn.data_ptr() if native else None, ldn, dT.data_ptr() if transposed else None, ldt,
                                   dtype, _s()) == 0
          PU.check_guards()
          tag = f'{dt} {rows} x {cols} src_ld {src_ld} ldn {ldn} ldt {ldt} native {native} transposed {transposed}'
          assert _same_bits(dn.cpu(), want_n) if native else _is_sentinel(dn.cpu()), f'pack native: {tag}'
          assert _same_bits(dT.cpu(), want_t) if transposed else _is_sentinel(dT.cpu()), f'pack transposed: {tag}'


@pytest.mark.parametrize('dtype', DTYPES)
def test_transpose(lib, dtype):
  dt = _dt(dtype)
  for rows, cols in PACK_SHAPES:
    src = _pack_src(rows, cols, cols, dt, rows + cols).to(dt)
    srcd = src.cuda()
    dst = _out(cols, rows, dt, 'transpose dst')
    assert lib.spa3d_op_transpose(srcd.data_ptr(), rows, cols, dst.data_ptr(), dtype, _s()) == 0
    PU.check_guards()
    assert _same_bits(dst.cpu(), src.T.contiguous()), f'transpose {dt} {rows} x {cols}'


# ================================================================================================ latent quantiser
@pytest.mark.parametrize('n', [1, 255, 257, 70001])
def test_discretize(lib, n):
  planted = EU.discretize_planted()
  k = len(planted)
  rng = np.random.default_rng(n)
  lat = np.concatenate([planted, planted, planted, (rng.random(n) * 3 - 1.5).astype(f32)])[:n]
  noise_d = torch.empty(n, device='cuda')
  assert lib.spa3d_uniform_noise(noise_d.data_ptr(), n, 0, 0, _s()) == 0
  noise = noise_d.cpu().numpy()
  assert noise.min() >= 0.0 and noise.max() < 1.0
  noise[:k] = 0.0                                           # the first copy of the planted latents meets the smallest noise,
  noise[k:2 * k] = np.nextafter(f32(1), f32(0))             # the second the largest value below 1, the third whatever the generator gave
  noise_d = _dev(noise)
  latd = _dev(lat)
  nan = np.isnan(lat)
  for disc in (0, 1):
    ref, mask = EU.discretize_ref(lat, noise, disc)
    want64 = EU.discretize_oracle64(lat, noise, disc)
    for with_mask in (True, False):
      for with_noise in ((True,) if disc else (True, False)):
        out = _out(1, n, torch.float32, 'discretize out')
        cm = _out(1, n, torch.float32, 'discretize clipmask')
        assert lib.spa3d_op_discretize(latd.data_ptr(), noise_d.data_ptr() if with_noise else None, disc, out.data_ptr(), cm.data_ptr() if with_mask else None,
                                       n, _s()) == 0
        PU.check_guards()
        tag = f'n {n} discretize {disc} clipmask {with_mask} noise {with_noise}'
        got, gm = out.cpu()[0], cm.cpu()[0]
        # NaN at the reference's positions and nowhere else; every other element bit for bit (the reference's NaN is the input's own, passed through)
        assert np.array_equal(np.isnan(got.numpy()), nan) and _same_bits(got[~torch.from_numpy(nan)], torch.from_numpy(ref[~nan])), f'discretize out: {tag}'
        if with_mask:
          assert np.array_equal(np.isnan(gm.numpy()), nan) and _same_bits(gm[~torch.from_numpy(nan)], torch.from_numpy(mask[~nan])), f'clip mask: {tag}'
        else:
          assert _is_sentinel(gm), f'clip mask written without being asked for: {tag}'
        assert float(np.abs(got.numpy()[~nan].astype(np.float64) - want64[~nan]).max(initial=0.0)) <= 2.0 ** -23, f'against the float64 formula: {tag}'
