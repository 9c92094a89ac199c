"""Attention kernel selection (3dspa_code_amd/csrc/attn_plan.hpp) on the CPU: the planner is host-only code, so a small driver
(tests/host/attn_plan_check.cpp) is built with the host compiler and fed a table of (descriptor, pointers, attn_impl) -> route with its tile count KT,
waves, key splits and the bytes of fp32 partials it takes from the arena.  The rows pin every `attn_impl` value, every route of the catalogue, both
sides of each shape threshold, the layouts, every operand of the alignment lists one at a time, the 32-bit problem counts and the refusal reasons.
Expected values are worked out from the kernels' coverage (attention_fused.hip, qkv_attn.hip), not read back from the planner.  The planner has no
dry mode: a row holds for the sizing pass and the real pass alike.  No GPU needed."""
import subprocess

import pytest
from util import host_check_driver


def R(route, KT=0, NW=0, nsplit=0, part=(0, 0), why=''):
  return f'{route} KT={KT} NW={NW} nsplit={nsplit} part={part[0]},{part[1]}' + (f' why={why}' if why else '')


GENERIC, PER_SEQ = R('Generic'), R('GenericPerSeq')
NOT_COVERED, RAGGED = R('Refuse', why='not-covered'), R('Refuse', why='ragged')
KM = 'km=0xf00000'
# defaults of the driver: nseq = 4, H = 4, Dh = 96, 16-bit, no key mask, row strides H * Dh, every operand 16-byte aligned
X = 'Sq=128 Sk=2048'                                    # cross attention: 16 problems x 16 chunks of 128 keys
X_OPART, X_MLPART = 16 * 16 * 128 * 96 * 4, 16 * 16 * 128 * 2 * 4
XFWD, XBWD = R('XFwd', 8, 4, 16, (X_OPART, X_MLPART)), R('XBwd', 8, 8, 16, (X_OPART, 0))
RK = 'layout=keys keys=300,117,64 Sq=128'               # ragged keys: 3 sequences, the longest 300 keys = 3 chunks; 12 problems
RK_OPART, RK_MLPART = 12 * 3 * 128 * 96 * 4, 12 * 3 * 128 * 2 * 4
HOLE = 'layout=hole Nk=300 Sq=128'                      # 2 sequences over 300 shared rows; 8 problems x 3 chunks
HOLE_PART = (8 * 3 * 128 * 96 * 4, 8 * 3 * 128 * 2 * 4)
BIG = 2**31 - 1

CASES = [
  # ---- attn_impl: 0 product dispatch | 1 generic | every value >= 2 the fused kernels or a refusal | 3 / 4 split-pass backward on 4 / 8 waves | 6 fused QKV
  ('fwd 0 S=151', R('SelfFwd', 10, 4)),
  ('fwd -1 S=151', R('SelfFwd', 10, 4)),
  ('fwd 1 S=151', GENERIC),
  ('fwd 2 S=151', R('SelfFwd', 10, 4)),
  ('fwd 3 S=151', R('SelfFwd', 10, 4)),
  ('fwd 4 S=151', R('SelfFwd', 10, 4)),
  ('fwd 6 S=151', R('SelfFwd', 10, 4)),
  ('fwd 7 S=151', R('SelfFwd', 10, 4)),
  ('bwd 0 S=151', R('Bwd4Fast', 10, 8)),
  ('bwd 1 S=151', GENERIC),
  ('bwd 2 S=151', R('Bwd4Fast', 10, 8)),
  ('bwd 3 S=151', R('BwdSplit4', 10, 4)),
  ('bwd 4 S=151', R('BwdSplit8', 10, 8)),
  ('bwd 6 S=151', R('Bwd4Fast', 10, 8)),
  ('bwd 7 S=151', R('Bwd4Fast', 10, 8)),
  ('bwd 3 S=160', R('BwdSplit4', 10, 4)),
  ('bwd 4 S=160', R('BwdSplit8', 10, 8)),
  ('bwd 3 S=161', R('BwdSplit8', 12, 8)),               # above S = 160 only the 8-wave split-pass kernel exists
  ('bwd 4 S=161', R('BwdSplit8', 12, 8)),
  ('fwd 7 S=321', NOT_COVERED),                          # >= 2: never the generic composition
  ('bwd 7 S=321', NOT_COVERED),
  # ---- forward, self attention: tiles of 16 keys, odd counts pair up except nine; 8 waves from 14 tiles
  ('fwd 0 S=1', GENERIC),
  ('fwd 2 S=1', NOT_COVERED),
  ('fwd 0 S=2', R('SelfFwd', 2, 4)),
  ('fwd 0 S=128', R('SelfFwd', 8, 4)),
  ('fwd 0 S=129', R('SelfFwd', 9, 4)),
  ('fwd 0 S=144', R('SelfFwd', 9, 4)),
  ('fwd 0 S=145', R('SelfFwd', 10, 4)),
  ('fwd 0 S=192', R('SelfFwd', 12, 4)),
  ('fwd 0 S=193', R('SelfFwd', 14, 8)),                 # 13 tiles pair up to 14: the first 8-wave instance
  ('fwd 0 S=208', R('SelfFwd', 14, 8)),
  ('fwd 0 S=209', R('SelfFwd', 14, 8)),
  ('fwd 0 S=320', R('SelfFwd', 20, 8)),
  ('fwd 0 S=321', GENERIC),
  ('fwd 2 S=321', NOT_COVERED),
  ('fwd 0 S=151 ' + KM, R('SelfFwd', 10, 4)),
  # ---- backward, self attention: even tile counts; four images up to S_pad = 160 (fast path without a key mask), else split-pass on 8 waves
  ('bwd 0 S=1', GENERIC),
  ('bwd 0 S=2', R('Bwd4Fast', 2, 8)),
  ('bwd 0 S=128', R('Bwd4Fast', 8, 8)),
  ('bwd 0 S=129', R('Bwd4Fast', 10, 8)),
  ('bwd 0 S=160', R('Bwd4Fast', 10, 8)),
  ('bwd 0 S=161', R('BwdSplit8', 12, 8)),
  ('bwd 0 S=320', R('BwdSplit8', 20, 8)),
  ('bwd 0 S=321', GENERIC),
  ('bwd 2 S=321', NOT_COVERED),
  ('bwd 0 S=151 ' + KM, R('Bwd4', 10, 8)),
  ('bwd 0 S=161 ' + KM, R('BwdSplit8', 12, 8)),
  ('bwd 3 S=151 ' + KM, R('BwdSplit4', 10, 4)),
  ('bwd 0 S=151 o=0', GENERIC),                          # the fused backward rebuilds P from the forward's o and lse
  ('bwd 0 S=151 lse=0', GENERIC),
  ('bwd 2 S=151 lse=0', NOT_COVERED),
  # ---- Sq != Sk: chunked keys, at most 128 query rows
  ('fwd 0 ' + X, XFWD),
  ('fwd 0 Sq=129 Sk=2048', GENERIC),
  ('fwd 2 Sq=129 Sk=2048', NOT_COVERED),
  ('fwd 0 Sq=1 Sk=1', GENERIC),                          # Sq == Sk is self attention, and below its two rows
  ('fwd 0 Sq=128 Sk=129', R('XFwd', 8, 4, 2, (16 * 2 * 128 * 96 * 4, 16 * 2 * 128 * 2 * 4))),
  ('fwd 0 ' + X + ' ' + KM, XFWD),
  ('fwd 1 ' + X, GENERIC),
  ('bwd 0 ' + X, XBWD),
  ('bwd 0 Sq=129 Sk=2048', GENERIC),
  ('bwd 3 ' + X, XBWD),
  ('bwd 0 ' + X + ' lse=0', GENERIC),
  # ---- ragged key sets: one launch over the longest sequence's chunks, else the sequences one by one
  ('fwd 0 ' + RK, R('XFwdRaggedKeys', 8, 4, 3, (RK_OPART, RK_MLPART))),
  ('bwd 0 ' + RK, R('XBwdRaggedKeys', 8, 8, 3, (RK_OPART, 0))),
  ('fwd 2 ' + RK, R('XFwdRaggedKeys', 8, 4, 3, (RK_OPART, RK_MLPART))),
  ('fwd 0 layout=keys keys=128,128 Sq=128', R('XFwdRaggedKeys', 8, 4, 1, (8 * 128 * 96 * 4, 8 * 128 * 2 * 4))),   # Sq = the key count: still chunked
  ('fwd 1 ' + RK, PER_SEQ),
  ('bwd 1 ' + RK, PER_SEQ),
  ('fwd 0 ' + RK + ' Dh=64', PER_SEQ),
  ('fwd 2 ' + RK + ' Dh=64', PER_SEQ),                   # (each sequence is then refused on its own)
  ('fwd 0 ' + RK + ' esz=4', PER_SEQ),
  ('fwd 0 layout=keys keys=300,117,64 Sq=129', PER_SEQ),
  ('bwd 0 layout=keys keys=300,117,64 Sq=129', PER_SEQ),
  ('bwd 0 ' + RK + ' o=0', PER_SEQ),
  ('bwd 0 ' + RK + ' dk=0x900008', PER_SEQ),
  # ---- one shared key set with a hole per sequence (forward only)
  ('fwd 0 ' + HOLE + ' holes=0:0,100:150', R('XFwdHole', 8, 4, 3, HOLE_PART)),     # nmax = Nk: an empty hole
  ('fwd 0 ' + HOLE + ' holes=0:150,100:150', R('XFwdHole', 8, 4, 2, (8 * 2 * 128 * 96 * 4, 8 * 2 * 128 * 2 * 4))),
  ('fwd 0 ' + HOLE + ' holes=10:5,100:150', PER_SEQ),                              # nmax > Nk
  ('fwd 1 ' + HOLE + ' holes=0:0,100:150', PER_SEQ),
  ('fwd 0 ' + HOLE + ' holes=0:0,100:150 esz=4', PER_SEQ),
  ('fwd 0 ' + HOLE + ' holes=0:0,100:150 Dh=64', PER_SEQ),
  ('fwd 0 ' + HOLE + ' holes=0:0,100:150 v=0x300008', PER_SEQ),
  ('bwd 0 ' + HOLE + ' holes=0:0,100:150', NOT_COVERED),
  # ---- ragged query rows (token pruning): the fused self-attention kernels or an error, never the generic composition
  ('fwd 0 layout=rows S=151', R('SelfFwd', 10, 4)),
  ('bwd 0 layout=rows S=151', R('Bwd4Fast', 10, 8)),
  ('bwd 0 layout=rows S=301 ' + KM, R('BwdSplit8', 20, 8)),
  ('fwd 1 layout=rows S=151', RAGGED),
  ('bwd 1 layout=rows S=151', RAGGED),
  ('fwd 0 layout=rows S=151 Dh=64', RAGGED),
  ('fwd 2 layout=rows S=151 Dh=64', RAGGED),
  ('bwd 0 layout=rows S=151 Dh=64', RAGGED),
  ('fwd 0 layout=rows S=321', RAGGED),
  ('fwd 0 layout=rows Sq=128 Sk=256', RAGGED),
  ('bwd 0 layout=rows S=151 lse=0', RAGGED),
  # ---- the fp32 parity mode and other head widths: the generic composition
  ('fwd 0 S=151 esz=4', GENERIC),
  ('bwd 0 S=151 esz=4', GENERIC),
  ('fwd 2 S=151 esz=4', NOT_COVERED),
  ('bwd 2 S=151 esz=4', NOT_COVERED),
  ('fwd 0 ' + X + ' esz=4', GENERIC),
  ('fwd 0 S=151 Dh=64', GENERIC),
  ('bwd 0 S=151 Dh=64', GENERIC),
  ('fwd 2 S=151 Dh=64', NOT_COVERED),
  ('bwd 2 S=151 Dh=64', NOT_COVERED),
  ('fwd 0 ' + X + ' Dh=64', GENERIC),
  ('bwd 0 ' + X + ' Dh=64', GENERIC),
  # ---- 32-bit problem counts: nseq * H, and nseq * H * key chunks
  (f'fwd 0 S=151 H=1 nseq={BIG}', R('SelfFwd', 10, 4)),
  (f'fwd 0 S=151 H=1 nseq={BIG + 1}', GENERIC),
  (f'bwd 0 S=151 H=1 nseq={BIG}', R('Bwd4Fast', 10, 8)),
  (f'bwd 0 S=151 H=1 nseq={BIG + 1}', GENERIC),
  (f'fwd 0 Sq=128 Sk=256 H=1 nseq={2**30 - 1}', R('XFwd', 8, 4, 2, ((2**31 - 2) * 128 * 96 * 4, (2**31 - 2) * 128 * 2 * 4))),
  (f'fwd 0 Sq=128 Sk=256 H=1 nseq={2**30}', GENERIC),
  (f'bwd 0 Sq=128 Sk=256 H=1 nseq={2**30 - 1}', R('XBwd', 8, 8, 2, ((2**31 - 2) * 128 * 96 * 4, 0))),
  (f'bwd 0 Sq=128 Sk=256 H=1 nseq={2**30}', GENERIC),
]
# ---- alignment: row strides in multiples of 8 elements; q, k, v, o 16-byte aligned in the forward, and d_o, dq, dk, dv, sq, sk as well in the backward
FWD_PTRS = {'q': 0x100000, 'k': 0x200000, 'v': 0x300000, 'o': 0x400000}
BWD_ONLY_PTRS = {'d_o': 0x700000, 'dq': 0x800000, 'dk': 0x900000, 'dv': 0xa00000, 'sq': 0x600000, 'sk': 0x610000}
for shape in ('S=151', X):
  for ld in ('ldq', 'ldk', 'ldv'):
    CASES += [(f'fwd 0 {shape} {ld}=388', GENERIC), (f'bwd 0 {shape} {ld}=388', GENERIC), (f'fwd 2 {shape} {ld}=388', NOT_COVERED)]
  CASES += [(f'fwd 0 {shape} ldq=1152 ldk=1152 ldv=1152', XFWD if shape == X else R('SelfFwd', 10, 4))]
  for name, addr in FWD_PTRS.items():
    CASES += [(f'fwd 0 {shape} {name}={addr + 8:#x}', GENERIC), (f'bwd 0 {shape} {name}={addr + 8:#x}', GENERIC)]
  for name, addr in BWD_ONLY_PTRS.items():
    CASES += [(f'bwd 0 {shape} {name}={addr + 4:#x}', GENERIC), (f'bwd 2 {shape} {name}={addr + 4:#x}', NOT_COVERED),
              (f'fwd 0 {shape} {name}={addr + 4:#x}', XFWD if shape == X else R('SelfFwd', 10, 4))]   # the forward reads the scales element by element
CASES += [
  # ---- fused QKV projection + attention forward (attn_impl 6 only): d = 384, 96-wide heads, 2 <= S <= 160, a packed weight stream
  ('qkv 6 S=151', R('QkvFwd', 10, 4)),
  ('qkv 6 S=160', R('QkvFwd', 10, 4)),
  ('qkv 6 S=161', R('Refuse')),
  ('qkv 6 S=2', R('QkvFwd', 10, 4)),
  ('qkv 6 S=1', R('Refuse')),
  ('qkv 6 S=151 layout=rows', R('QkvFwd', 10, 4)),
  ('qkv 6 S=151 ' + KM, R('QkvFwd', 10, 4)),
  ('qkv 6 S=151 d=256', R('Refuse')),
  ('qkv 6 S=151 pk=0', R('Refuse')),                    # a missing pack (shared readout rows; a cross block)
  ('qkv 6 S=151 Dh=64', R('Refuse')),
  ('qkv 6 S=151 esz=4', R('Refuse')),
  ('qkv 6 S=151 ldx=388', R('Refuse')),
  ('qkv 6 S=151 x=0xd00008', R('Refuse')),
  ('qkv 6 S=151 q=0x100008', R('Refuse')),
  ('qkv 6 S=151 o=0x400008', R('Refuse')),
  ('qkv 6 S=151 pk=0xe00008', R('Refuse')),
  (f'qkv 6 S=151 H=1 nseq={BIG}', R('QkvFwd', 10, 4)),
  (f'qkv 6 S=151 H=1 nseq={BIG + 1}', R('Refuse')),
  ('qkv 0 S=151', R('Refuse')),
  ('qkv 2 S=151', R('Refuse')),
  ('pack 6', '1'),
  ('pack 0', '0'),
  ('pack 2', '0'),
  ('pack 6 cross=1', '0'),
  ('pack 6 d=256', '0'),
  ('pack 6 Dh=64', '0'),
  ('pack 6 gemm_generic=1', '0'),
  # ---- what the model asks before it prunes: ragged self attention on the fused kernels
  ('prune 0 S=151', '1'),
  ('prune 2 S=151', '1'),
  ('prune 6 S=151', '1'),
  ('prune 1 S=151', '0'),
  ('prune 0 S=320', '1'),
  ('prune 0 S=321', '0'),
  ('prune 0 S=2', '1'),
  ('prune 0 S=1', '0'),
  ('prune 0 S=151 Dh=64', '0'),
  ('prune 0 S=151 esz=4', '0'),
]


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
  return host_check_driver(tmp_path_factory, 'attn_plan', fp_contract_off=False)


def test_attn_plan_table(driver):
  r = subprocess.run([driver], input='\n'.join(c for c, _ in CASES) + '\n', capture_output=True, text=True, timeout=60)
  assert r.returncode == 0, r.stderr
  got = r.stdout.splitlines()
  assert len(got) == len(CASES)
  bad = [(case, want, g) for (case, want), g in zip(CASES, got) if g != want]
  assert not bad, '\n'.join(f'{c}\n  want {w}\n  got  {g}' for c, w, g in bad)


def test_prune_predicate_agrees_with_the_planner(driver):
  """Whatever the predicate admits, plan_attn_fwd / plan_attn_bwd take as ragged rows (aligned operands); what it declines at 16-bit Dh = 96 they refuse."""
  cases = [(impl, S) for impl in (0, 1, 2, 3, 4, 6) for S in (1, 2, 151, 160, 161, 320, 321)]
  lines = [f'prune {i} S={S}' for i, S in cases] + [f'fwd {i} layout=rows S={S}' for i, S in cases] + [f'bwd {i} layout=rows S={S}' for i, S in cases]
  r = subprocess.run([driver], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=60)
  assert r.returncode == 0, r.stderr
  got = r.stdout.splitlines()
  n = len(cases)
  assert len(got) == 3 * n
  for j, case in enumerate(cases):
    admitted = got[j] == '1'
    assert admitted == (not got[n + j].startswith('Refuse')) == (not got[2 * n + j].startswith('Refuse')), (case, got[j], got[n + j], got[2 * n + j])
