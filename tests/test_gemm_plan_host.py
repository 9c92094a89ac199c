"""GEMM kernel selection (3dspa_code_amd/csrc/gemm_plan.hpp) on the CPU: the planner is host-only code, so a small driver
(tests/host/gemm_plan_check.cpp) is built with the host compiler and fed a table of (descriptor, pointers, policy) -> kernel.  The rows pin
every `gemm_impl` value, every kernel of the catalogue and both sides of each threshold (rows 512 / 16 384 / 65 536, K <= 512, M.N < 128^2,
8-phase dW tile waste <= 1.25, brow_group >= 16), the operand refusals and the fused column sums.  The planner has no dry mode: a row holds
for the sizing pass and the real pass alike.  No GPU needed."""
import subprocess

import pytest
from util import host_check_driver

BT = 'Bt=0x500000'
# dW descriptor: C[Ki = M][N] += A^T B over K rows
TN = 'sAm=1 sBn=1 out_f32=1 accumulate=1 zero_page=0xb00000'


def tn(ki, n, m, extra=''):
  return f'M={ki} N={n} K={m} sAk={ki} sBk={n} sCm={n} {TN} {extra}'


CASES = [
  # ---- gemm_impl 1: generic only; tiny problems and non-tiled layouts fall back to the generic kernel
  ('gemm 1 M=65536 N=384 K=384 ' + BT + ' ldBt=384', 'Generic flags=0'),
  ('gemm 0 M=127 N=128 K=64 ' + BT + ' ldBt=64', 'Generic flags=0'),             # M.N < 128^2
  ('nt 0 M=128 N=128 K=64 ' + BT + ' ldBt=64', 'NtOcc flags=0'),
  ('nt 0 M=1024 N=128 K=64 sBk=1 sBn=64', 'NtOcc flags=0'),                      # B itself K-contiguous
  ('nt 0 M=1024 N=128 K=64', 'Refuse flags=0'),                                  # no [N][K] copy of B
  ('nt 0 M=1024 N=128 K=96 ' + BT + ' ldBt=96', 'Refuse flags=0'),               # K % 64
  ('nt 0 M=1024 N=128 K=64 atomic=1 ' + BT + ' ldBt=64', 'Refuse flags=0'),
  ('nt 0 M=1024 N=128 K=64 C=0x300008 ' + BT + ' ldBt=64', 'Refuse flags=0'),    # misaligned C
  ('nt 0 M=1024 N=128 K=64 bias=0x720004 ' + BT + ' ldBt=64', 'Refuse flags=0'),
  ('nt 0 M=1024 N=128 K=64 out_f32=1 aux=0x900000 ' + BT + ' ldBt=64', 'Refuse flags=0'),
  ('nt 0 M=274877906944 N=128 K=64 ' + BT + ' ldBt=64', 'Refuse flags=0'),       # grid past 2^31 workgroups
  ('nt 0 M=137438953472 N=128 K=64 ' + BT + ' ldBt=64', 'NtOcc flags=0'),
  ('gemm 1 ' + tn(384, 1536, 65536), 'Generic flags=0'),
  ('gemm 0 ' + tn(384, 1536, 255), 'Generic flags=0'),                           # dW over < 256 rows
  # ---- short K (<= 512) single-buffer kernel; 5 turns it off
  ('nt 0 M=1024 N=136 K=512 ' + BT + ' ldBt=512', 'NtOcc flags=0'),
  ('nt 0 M=1024 N=136 K=576 ' + BT + ' ldBt=576', 'Nt flags=0'),
  ('nt 5 M=1024 N=136 K=512 ' + BT + ' ldBt=512', 'Nt flags=0'),
  ('nt 2 M=1024 N=136 K=512 ' + BT + ' ldBt=512', 'NtOcc flags=0'),
  # ---- 8-phase NT kernels from 16 384 rows; 3 / 4 / 9 any row count, 4 without the persistent 128 x 384 kernel
  ('nt 0 M=16384 N=256 K=256 ' + BT + ' ldBt=256', 'Nt8pp256 flags=0'),
  ('nt 0 M=16383 N=256 K=256 ' + BT + ' ldBt=256', 'NtOcc flags=0'),
  ('nt 0 M=16384 N=384 K=768 ' + BT + ' ldBt=768', 'Nt8pp384 flags=0'),
  ('nt 0 M=16384 N=384 K=768 aux=0x900000 ' + BT + ' ldBt=768', 'Nt8pp384 flags=4'),
  ('nt 4 M=16384 N=384 K=768 ' + BT + ' ldBt=768', 'Nt8p384 flags=0'),
  ('nt 4 M=1024 N=256 K=256 ' + BT + ' ldBt=256', 'Nt8pp256 flags=0'),
  ('nt 3 M=1024 N=384 K=384 ' + BT + ' ldBt=384', 'Nt8pp384 flags=0'),
  ('nt 9 M=1024 N=384 K=384 ' + BT + ' ldBt=384', 'Nt8pp384 flags=0'),
  ('nt 0 M=16384 N=384 K=768 accumulate=1 ' + BT + ' ldBt=768', 'Nt8p384 flags=32'),
  ('nt 0 M=16384 N=256 K=768 crow_group=8 ' + BT + ' ldBt=768', 'Nt8p256 flags=64'),
  ('nt 0 M=16388 N=256 K=256 ' + BT + ' ldBt=256', 'Nt8p256 flags=0'),           # M % 8: not persistent
  ('nt 0 M=16384 N=256 K=64 ' + BT + ' ldBt=64', 'Nt8p256 flags=0'),             # K < 128: not persistent
  ('nt 0 M=16384 N=384 K=384 epi=1 pre_out=0xd00000 ' + BT + ' ldBt=384', 'Nt8p384 flags=9'),
  ('nt 0 M=16384 N=768 K=384 epi=1 pre_out=0xd00000 ' + BT + ' ldBt=384', 'Nt8pp256 flags=9'),
  ('nt 0 M=16384 N=384 K=384 sAm=1152 ' + BT + ' ldBt=384', 'Nt8pp384 flags=128'),
  # ---- one-pass input embedding (the 8-phase 128 x 384 kernel with gathered / scattered rows); 6 and 1 refuse it
  ('nt 0 M=4096 N=384 K=1024 sAm=256 A2=0x600000 sA2m=768 K1=256 arow=0x700000 crow=0x710000 bias=0x720000 ' + BT + ' ldBt=1024', 'NtEmbed flags=128'),
  ('nt 0 M=4096 N=384 K=1024 sAm=256 A2=0x600002 sA2m=768 K1=256 arow=0x700000 crow=0x710000 ' + BT + ' ldBt=1024', 'Refuse flags=0'),  # A2 misaligned
  ('nt 0 M=4096 N=384 K=1024 sAm=256 A2=0x600000 sA2m=768 K1=192 arow=0x700000 crow=0x710000 ' + BT + ' ldBt=1024', 'NtEmbed flags=128'),
  ('nt 0 M=4096 N=384 K=1024 sAm=256 A2=0x600000 sA2m=768 K1=200 arow=0x700000 crow=0x710000 ' + BT + ' ldBt=1024', 'Refuse flags=0'),  # K1 % 64
  ('nt 0 M=4096 N=384 K=1024 sAm=256 A2=0x600000 sA2m=768 K1=1024 arow=0x700000 crow=0x710000 ' + BT + ' ldBt=1024', 'Refuse flags=0'), # K1 >= K
  ('nt 0 M=4096 N=384 K=1024 sAm=256 A2=0x600000 sA2m=772 K1=256 arow=0x700000 crow=0x710000 ' + BT + ' ldBt=1024', 'Refuse flags=0'),  # sA2m % 8
  ('nt 0 M=4096 N=384 K=256 arow=0x700000 crow=0x710000 r1_x=0x730000 ' + BT + ' ldBt=256', 'Refuse flags=0'),                        # r1_x without r1_w
  ('nt 0 M=4096 N=384 K=256 arow=0x700000 crow=0x710000 r1_x=0x730000 r1_w=0x740000 ' + BT + ' ldBt=256', 'NtEmbed flags=0'),
  ('nt 0 M=4096 N=768 K=256 arow=0x700000 crow=0x710000 ' + BT + ' ldBt=256', 'Refuse flags=0'),                                      # N != 384
  ('nt 0 M=4096 N=384 K=256 arow=0x700000 crow=0x710000 accumulate=1 ' + BT + ' ldBt=256', 'Refuse flags=0'),
  ('nt 6 M=4096 N=384 K=256 arow=0x700000 crow=0x710000 ' + BT + ' ldBt=256', 'Refuse flags=0'),
  ('nt 1 M=4096 N=384 K=256 arow=0x700000 crow=0x710000 ' + BT + ' ldBt=256', 'Refuse flags=0'),
  # ---- row-stationary K = 384 kernel from 512 rows; 6 off; 7 (ops) any row count or nothing
  ('nt 0 M=512 N=1152 K=384 rs_pk=0x800000 ' + BT + ' ldBt=384', 'Rs flags=512'),
  ('nt 0 M=511 N=1152 K=384 rs_pk=0x800000 ' + BT + ' ldBt=384', 'NtOcc flags=0'),
  ('nt 0 M=512 N=384 K=1536 sAm=1536 epi=2 aux=0x900000 rs_pk=0x800000 ' + BT + ' ldBt=1536', 'Nt flags=6'),  # K != 384
  ('nt 0 M=512 N=1536 K=384 epi=2 aux=0x900000 rs_pk=0x800000 ' + BT + ' ldBt=384', 'Rs flags=518'),
  ('nt 0 M=512 N=1152 K=384 aux=0x900000 rs_pk=0x800000 ' + BT + ' ldBt=384', 'NtOcc flags=4'),                # residual: tiled
  ('nt 0 M=512 N=1152 K=384 accumulate=1 rs_pk=0x800000 ' + BT + ' ldBt=384', 'NtOcc flags=32'),
  ('nt 6 M=4096 N=1152 K=384 rs_pk=0x800000 ' + BT + ' ldBt=384', 'NtOcc flags=0'),
  ('nt 7 M=1 N=1152 K=384 rs_pk=0x800000', 'Rs flags=512'),
  ('nt 7 M=64 N=2304 K=384 rs_pk=0x800000', 'Rs flags=512'),
  ('nt 7 M=64 N=2432 K=384 rs_pk=0x800000', 'Refuse flags=0'),                  # N > 2304
  ('nt 7 M=64 N=192 K=384 rs_pk=0x800000', 'Refuse flags=0'),                   # N < 256
  ('nt 7 M=64 N=1152 K=384 epi=1 rs_pk=0x800000', 'Refuse flags=0'),            # gelu forward
  ('nt 7 M=64 N=1152 K=384 aux=0x900000 rs_pk=0x800000', 'Refuse flags=0'),     # residual
  ('nt 7 M=64 N=1152 K=384 epi=2 rs_pk=0x800000', 'Refuse flags=0'),            # gelu' without its pre-activation
  ('nt 7 M=64 N=1152 K=384 A=0x100008 rs_pk=0x800000', 'Refuse flags=0'),
  ('nt 7 M=64 N=1152 K=384 ' + BT + ' ldBt=384', 'Refuse flags=0'),             # no stream
  # ---- large-register-tile NT kernel from 65 536 rows; 9 any; 3, 4, 6, 8 off; 10 (ops) any row count or nothing
  ('nt 0 M=65536 N=384 K=1536 ntb_pk=0xa00000 ' + BT + ' ldBt=1536', 'Ntb flags=2097152'),
  ('nt 0 M=65536 N=384 K=1536 bias=0x720000 ntb_pk=0xa00000 ' + BT + ' ldBt=1536', 'Ntb flags=2097153'),
  ('nt 0 M=65528 N=384 K=1536 ntb_pk=0xa00000 ' + BT + ' ldBt=1536', 'Nt8pp384 flags=0'),
  ('nt 9 M=1024 N=384 K=1536 ntb_pk=0xa00000 ' + BT + ' ldBt=1536', 'Ntb flags=2097152'),
  ('nt 8 M=65536 N=384 K=1536 ntb_pk=0xa00000 ' + BT + ' ldBt=1536', 'Nt8pp384 flags=0'),
  ('nt 3 M=65536 N=384 K=1536 ntb_pk=0xa00000 ' + BT + ' ldBt=1536', 'Nt8pp384 flags=0'),
  ('nt 6 M=65536 N=384 K=1536 ntb_pk=0xa00000 ' + BT + ' ldBt=1536', 'Nt8pp384 flags=0'),
  ('nt 0 M=65536 N=384 K=1536 aux=0x900000 ntb_pk=0xa00000 ' + BT + ' ldBt=1536', 'Nt8pp384 flags=4'),
  ('nt 0 M=65536 N=384 K=1536 bias=0x720004 ntb_pk=0xa00000 ' + BT + ' ldBt=1536', 'Refuse flags=0'),
  ('nt 10 M=8 N=256 K=3072 ntb_pk=0xa00000', 'Ntb flags=2097152'),
  ('nt 10 M=8 N=320 K=3072 ntb_pk=0xa00000', 'Refuse flags=0'),                 # neither 384 | N nor 256 | N
  ('nt 10 M=8 N=384 K=32 ntb_pk=0xa00000', 'Refuse flags=0'),                   # K < 64
  ('nt 10 M=8 N=384 K=96 epi=1 ntb_pk=0xa00000', 'Refuse flags=0'),
  ('nt 10 M=8 N=384 K=96 ntb_pk=0xa00008', 'Refuse flags=0'),                   # misaligned stream
  ('nt 10 M=8 N=384 K=96 sAm=2097152 ntb_pk=0xa00000', 'Refuse flags=0'),       # lda > 2^20
  # ---- dW: large-tile kernel from 65 536 rows, else the 8-phase kernels (65 536 rows, tile waste <= 1.25), else gemm_tn_kernel
  ('tn 0 ' + tn(384, 1536, 65536), 'Tnb flags=1048576'),
  ('tn 0 ' + tn(384, 1536, 65536, 'colsum=0xc00000'), 'Tnb+colsum flags=1048576'),
  ('tn 0 ' + tn(768, 1152, 65536), 'Tnb flags=1048576'),                        # 256 | Ki, 384 | N
  ('tn 0 ' + tn(384, 1536, 65535, 'colsum=0xc00000'), 'Tn flags=7'),
  ('gemm 0 ' + tn(384, 1536, 65535), 'Tn flags=7'),
  ('tn 9 ' + tn(384, 1536, 1024), 'Tnb flags=1048576'),
  ('tn 8 ' + tn(384, 1536, 65536, 'colsum=0xc00000'), 'Tn8p128x384+colsum flags=0'),
  ('tn 6 ' + tn(384, 1536, 65536), 'Tn8p128x384 flags=0'),
  ('tn 3 ' + tn(384, 1536, 1024), 'Tn8p128x384 flags=0'),
  ('tn 4 ' + tn(512, 512, 1024), 'Tn8p256 flags=0'),
  ('tn 8 ' + tn(512, 512, 65536), 'Tn8p256 flags=0'),
  ('tn 8 ' + tn(1152, 640, 65536), 'Tn8p384x128 flags=0'),
  ('tn 8 ' + tn(320, 256, 65536), 'Tn8p384x128 flags=0'),                       # least waste 1.2
  ('tn 8 ' + tn(288, 256, 65536), 'Tn flags=7'),                                # least waste 1.33
  ('tn 9 ' + tn(288, 256, 1024), 'Tn8p384x128 flags=0'),
  ('tn 0 ' + tn(384, 1536, 65536, 'brow_group=15 brow_skip=1'), 'Tn flags=7'),
  ('tn 0 ' + tn(384, 1536, 65536, 'brow_group=16 brow_skip=1'), 'Tnb flags=1048576'),
  ('tn 0 ' + tn(384, 1536, 65536, 'brow_group=16 brow_skip=16384'), 'Tn8p128x384 flags=0'),   # skips past 32 bits
  ('tn 8 ' + tn(512, 512, 65536, 'brow_group=15 brow_skip=1'), 'Tn flags=7'),
  ('tn 8 ' + tn(512, 512, 65536, 'brow_group=16 brow_skip=1'), 'Tn8p256 flags=0'),
  ('tn 0 ' + tn(384, 1536, 65536, 'A=0x100008'), 'Refuse flags=0'),
  ('tn 0 ' + tn(384, 1536, 65536, 'bias=0x720000'), 'Refuse flags=0'),
  ('tn 0 ' + tn(384, 1536, 65536, 'zero_page=0'), 'Refuse flags=0'),
  ('tn 0 ' + tn(12, 1536, 65536), 'Refuse flags=0'),                            # Ki % 8
  # ---- fused q | k | v dW: segments routed to separate leaves, 8-phase / large-tile kernels only (else one GEMM per segment)
  ('tn 0 ' + tn(384, 1152, 65536, 'seg_n=384 sCm=384'), 'Tn8p128x384 flags=0'),
  ('tn 0 ' + tn(384, 768, 65536, 'seg_n=384 sCm=384'), 'Tnb flags=1048576'),
  ('tn 0 ' + tn(384, 1152, 1024, 'seg_n=384 sCm=384'), 'Refuse flags=0'),
  ('tn 0 ' + tn(384, 1152, 65536, 'seg_n=96 sCm=96'), 'Refuse flags=0'),       # > 3 segments
  ('tn 0 ' + tn(384, 1152, 65536, 'seg_n=48 sCm=48'), 'Refuse flags=0'),       # seg_n % 32
  ('tn 0 ' + tn(384, 1152, 65536, 'seg_n=384 sCm=384 colsum=0xc00000'), 'Refuse flags=0'),
  ('tn 1 ' + tn(384, 1152, 65536, 'seg_n=384 sCm=384'), 'Refuse flags=0'),
  # ---- packed weight streams of a Lin
  ('lin 0 K=384 N=1152 segw=384 nseg=3', 'rs=1 rs_t=0 ntb=0 ntb_t=1'),
  ('lin 0 K=384 N=384', 'rs=1 rs_t=1 ntb=0 ntb_t=0'),
  ('lin 0 K=1536 N=384', 'rs=0 rs_t=1 ntb=1 ntb_t=0'),
  ('lin 0 K=1536 N=384 train=0', 'rs=0 rs_t=0 ntb=1 ntb_t=0'),
  ('lin 0 K=384 N=1536', 'rs=1 rs_t=0 ntb=0 ntb_t=1'),
  ('lin 0 K=384 N=384 segw=96 nseg=4', 'rs=0 rs_t=0 ntb=0 ntb_t=0'),
  ('lin 0 K=640 N=384', 'rs=0 rs_t=1 ntb=0 ntb_t=0'),
  ('lin 0 K=640 N=320', 'rs=0 rs_t=0 ntb=0 ntb_t=0'),
  ('lin 9 K=1536 N=384', 'rs=0 rs_t=1 ntb=1 ntb_t=0'),
  ('lin 8 K=1536 N=384', 'rs=0 rs_t=1 ntb=0 ntb_t=0'),
  ('lin 6 K=1536 N=384', 'rs=0 rs_t=0 ntb=0 ntb_t=0'),
  ('lin 1 K=384 N=1536', 'rs=0 rs_t=0 ntb=0 ntb_t=0'),
  # ---- fused MLP forward (and whether its stream is built)
  ('mlp 0', 'MlpFused 1'),
  ('mlp 2', 'MlpFused 1'),
  ('mlp 6', 'Refuse 0'),
  ('mlp 0 M=0', 'Refuse 1'),
  ('mlp 0 h=0x400008', 'Refuse 1'),
  ('mlp 0 wpk=0', 'Refuse 1'),
  ('mlp 0 b_out=0', 'Refuse 1'),
  ('mlp 0 d=256', 'Refuse 0'),
  ('mlp 0 cross=1', 'MlpFused 0'),
  # ---- one-pass embedding weights
  ('embed 0', '1'),
  ('embed 0 dino=0', '1'),
  ('embed 0 tokK=200', '0'),
  ('embed 0 dino=100', '0'),
  ('embed 0 depth=2', '0'),
  ('embed 0 twoD=1', '0'),
  ('embed 6', '0'),
]


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
  return host_check_driver(tmp_path_factory, 'gemm_plan', fp_contract_off=False)


def test_gemm_plan_table(driver):
  r = subprocess.run([driver], input='\n'.join(c for c, _ in CASES) + '\n', capture_output=True, text=True, timeout=60)
  assert r.returncode == 0, r.stderr
  got = r.stdout.splitlines()
  assert len(got) == len(CASES)
  bad = [(case, want, g) for (case, want), g in zip(CASES, got) if g != want]
  assert not bad, '\n'.join(f'{c}\n  want {w}\n  got  {g}' for c, w, g in bad)
