"""The refusals of the four ragged attention entry points (include/spa3d.h: spa3d_op_attention_ragged(_bwd), spa3d_op_attention_varlen(_bwd)) on the CPU.
Every one of them comes before the first launch and before the workspace is touched, so they are reachable without a device: the tensor pointers are fake
and never dereferenced, the offsets are real host arrays.  Each refused call differs in ONE argument from a call that passes the argument checks -- shown
by that call's SPA3D_ERR_WORKSPACE with an empty workspace, which is also answered before anything is launched."""
import ctypes as C

import numpy as np
import pytest

F32, BF16, F16 = 0, 1, 2
OK, ERR_ARG, ERR_WORKSPACE = 0, 1, 2
FAKE = 0x100000   # 16-byte aligned


@pytest.fixture(scope='module')
def lib():
  import spa3d
  return spa3d._lib.load()


def _i32(v):
  a = np.ascontiguousarray(v, dtype=np.int32)
  return a.ctypes.data_as(C.POINTER(C.c_int32)), a


RAGGED = dict(q=FAKE, k=FAKE, v=FAKE, ldq=576, ldk=576, ldv=576, sq=FAKE, sk=FAKE, km=None, off=[0, 151, 152, 169], nseq=None, S=151, H=2, Dh=96, o=FAKE, lse=FAKE,
              d_o=FAKE, dq=FAKE, dk=FAKE, dv=FAKE, dsq=FAKE, dsk=FAKE, dtype=BF16, impl=2, ws=FAKE, ws_bytes=0)
VARLEN = dict(q=FAKE, k=FAKE, v=FAKE, ldq=192, ldk=384, ldv=384, sq=FAKE, sk=FAKE, off=[0, 13, 313, 314], nseq=None, Sq=37, H=2, Dh=96, o=FAKE, lse=FAKE,
              d_o=FAKE, dq=FAKE, dk=FAKE, dv=FAKE, dsq=FAKE, dsk=FAKE, dtype=BF16, impl=2, ws=FAKE, ws_bytes=0)


def _ragged(lib, bwd, **kw):
  a = dict(RAGGED, **kw)
  off, keep = (None, None) if a['off'] is None else _i32(a['off'])
  nseq = a['nseq'] if a['nseq'] is not None else len(a['off']) - 1
  head = (a['q'], a['k'], a['v'], a['ldq'], a['ldk'], a['ldv'], a['sq'], a['sk'], a['km'], off, nseq, a['S'], a['H'], a['Dh'])
  tail = (a['dtype'], a['impl'], a['ws'], a['ws_bytes'], None)
  if bwd:
    return lib.spa3d_op_attention_ragged_bwd(*head, a['o'], a['lse'], a['d_o'], a['dq'], a['dk'], a['dv'], a['dsq'], a['dsk'], *tail)
  return lib.spa3d_op_attention_ragged(*head, a['o'], a['lse'], *tail)


def _varlen(lib, bwd, **kw):
  a = dict(VARLEN, **kw)
  off, keep = (None, None) if a['off'] is None else _i32(a['off'])
  nseq = a['nseq'] if a['nseq'] is not None else len(a['off']) - 1
  head = (a['q'], a['k'], a['v'], a['ldq'], a['ldk'], a['ldv'], a['sq'], a['sk'], off, nseq, a['Sq'], a['H'], a['Dh'])
  tail = (a['dtype'], a['impl'], a['ws'], a['ws_bytes'], None)
  if bwd:
    return lib.spa3d_op_attention_varlen_bwd(*head, a['o'], a['lse'], a['d_o'], a['dq'], a['dk'], a['dv'], a['dsq'], a['dsk'], *tail)
  return lib.spa3d_op_attention_varlen(*head, a['o'], a['lse'], *tail)


RAGGED_REFUSALS = [
    ('q', dict(q=None)), ('k', dict(k=None)), ('v', dict(v=None)), ('o', dict(o=None)), ('scale_q', dict(sq=None)), ('scale_k', dict(sk=None)),
    ('seq_off', dict(off=None, nseq=3)),
    ('fp32', dict(dtype=F32)), ('fp32, auto dispatch', dict(dtype=F32, impl=0)), ('an unknown dtype', dict(dtype=3)),
    ('impl 1', dict(impl=1)), ('impl 1, fp16', dict(impl=1, dtype=F16)), ('impl -5', dict(impl=-5)), ('impl 5', dict(impl=5)), ('impl 6', dict(impl=6)), ('impl 7', dict(impl=7)),
    ('Dh 64', dict(Dh=64)), ('Dh 128', dict(Dh=128)),
    ('S 1', dict(S=1, off=[0, 1, 2])), ('S 321', dict(S=321)), ('S 0', dict(S=0)), ('H 0', dict(H=0)), ('H -1', dict(H=-1)),
    ('nseq 0', dict(nseq=0)), ('nseq -1', dict(nseq=-1)), ('nseq 2^20 + 1', dict(off=np.arange(0, (1 << 20) + 2), nseq=(1 << 20) + 1)),
    ('seq_off[0] < 0', dict(off=[-1, 150, 151, 168])),
    ('a zero-length sequence', dict(off=[0, 151, 151, 168])),
    ('a length S + 1', dict(off=[0, 152, 153, 170])),
    ('a length S + 1 in the last sequence', dict(off=[0, 17, 18, 170])),
    ('decreasing offsets', dict(off=[0, 151, 140, 157])),
    ('offsets past 2^31', dict(off=[0x7fffff00, 0x7fffff80, -0x7fffff00, -0x7ffffe80])),
    ('a row stride that is no multiple of 8', dict(ldq=580)), ('a k stride of 0', dict(ldk=0)),
    ('row strides of 8, below H Dh', dict(ldq=8, ldk=8, ldv=8)), ('a q stride below H Dh', dict(ldq=184)), ('a v stride below H Dh', dict(ldv=96)),
    ('a misaligned v', dict(v=FAKE + 2)), ('a misaligned o', dict(o=FAKE + 8)),
]


@pytest.mark.parametrize('bwd', [False, True])
def test_ragged_self_attention_refusals_without_a_device(lib, bwd):
  for dtype in (BF16, F16):
    for impl in (0, 2, 3, 4):
      assert _ragged(lib, bwd, dtype=dtype, impl=impl) == ERR_WORKSPACE   # the arguments pass; the empty workspace is answered before any launch
  assert _ragged(lib, bwd, off=[5, 6, 157, 159]) == ERR_WORKSPACE          # a first offset above 0 and the lengths 1, S, 2 are fine
  assert _ragged(lib, bwd, km=FAKE) == ERR_WORKSPACE
  assert _ragged(lib, bwd, ldq=192, ldk=192, ldv=192) == ERR_WORKSPACE       # separate q, k, v planes of exactly H Dh columns
  for what, kw in RAGGED_REFUSALS:
    for dtype in ((BF16, F16) if 'dtype' not in kw else (kw['dtype'],)):
      assert _ragged(lib, bwd, **dict(kw, dtype=dtype)) == ERR_ARG, (what, dtype)
  if bwd:
    for name in ('lse', 'd_o', 'dq', 'dk', 'dv', 'dsq', 'dsk'):
      assert _ragged(lib, True, **{name: None}) == ERR_ARG, name
  else:
    assert _ragged(lib, False, lse=None) == ERR_WORKSPACE                  # lse is optional in the forward


VARLEN_REFUSALS = [
    ('q', dict(q=None)), ('k', dict(k=None)), ('v', dict(v=None)), ('o', dict(o=None)), ('scale_q', dict(sq=None)), ('scale_k', dict(sk=None)),
    ('koff', dict(off=None, nseq=3)),
    ('koff[0] != 0', dict(off=[1, 14, 314, 315])), ('koff[0] < 0', dict(off=[-1, 13, 313, 314])),
    ('a sequence without a key', dict(off=[0, 13, 13, 314])), ('a first sequence without a key', dict(off=[0, 0, 300, 301])),
    ('decreasing offsets', dict(off=[0, 300, 13, 314])),
    ('Sq 0', dict(Sq=0)), ('H 0', dict(H=0)), ('Dh 0', dict(Dh=0)), ('Dh 129', dict(Dh=129, ldq=258, ldk=258, ldv=258, impl=0)),
    ('nseq 0', dict(nseq=0)), ('nseq 2^20 + 1', dict(off=np.arange(0, (1 << 20) + 2), nseq=(1 << 20) + 1)),
    ('impl 3', dict(impl=3)), ('impl -1', dict(impl=-1)), ('an unknown dtype', dict(dtype=3)),
    ('impl 2 with Dh 64', dict(Dh=64)), ('impl 2 with Sq 129', dict(Sq=129)), ('impl 2 with fp32', dict(dtype=F32)),
    ('impl 2 with a row stride that is no multiple of 8', dict(ldk=388)), ('impl 2 with a misaligned k', dict(k=FAKE + 2)),
    ('a row stride below H Dh', dict(ldq=96)),
]


@pytest.mark.parametrize('bwd', [False, True])
def test_ragged_key_cross_attention_refusals_without_a_device(lib, bwd):
  for dtype, impl in ((BF16, 0), (BF16, 1), (BF16, 2), (F16, 0), (F16, 1), (F16, 2), (F32, 0), (F32, 1)):
    assert _varlen(lib, bwd, dtype=dtype, impl=impl) == ERR_WORKSPACE
  # every shape the generic route takes passes under impl 0 / 1
  for kw in (dict(Dh=64, ldq=128, ldk=128, ldv=128), dict(Sq=129), dict(Dh=16, H=2, Sq=16, dtype=F32, ldq=32, ldk=64, ldv=64)):
    for impl in (0, 1):
      assert _varlen(lib, bwd, **dict(kw, impl=impl)) == ERR_WORKSPACE, (kw, impl)
  for what, kw in VARLEN_REFUSALS:
    assert _varlen(lib, bwd, **kw) == ERR_ARG, what
  if bwd:
    for name in ('d_o', 'dq', 'dk', 'dv', 'dsq', 'dsk'):
      assert _varlen(lib, True, **{name: None}) == ERR_ARG, name
    # the fused backward rebuilds P from o and lse: for a 16-bit dtype both are required under impl 0 and 2 alike (with only one of them the sequences would
    # be tried on the fused kernels one by one); impl 1 and fp32 run the generic composition, which reads neither
    for dtype in (BF16, F16):
      for impl in (0, 2):
        for kw in (dict(o=None), dict(lse=None), dict(o=None, lse=None)):
          assert _varlen(lib, True, **dict(kw, dtype=dtype, impl=impl)) == ERR_ARG, (dtype, impl, kw)
      for kw in (dict(o=None), dict(lse=None), dict(o=None, lse=None)):
        assert _varlen(lib, True, **dict(kw, dtype=dtype, impl=1)) == ERR_WORKSPACE, (dtype, kw)
    for impl in (0, 1):
      for kw in (dict(o=None), dict(lse=None), dict(o=None, lse=None)):
        assert _varlen(lib, True, **dict(kw, dtype=F32, impl=impl)) == ERR_WORKSPACE, (impl, kw)
  else:
    assert _varlen(lib, False, lse=None) == ERR_WORKSPACE
