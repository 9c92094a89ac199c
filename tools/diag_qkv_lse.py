"""Where do the fused QKV kernel (spa3d_op_qkv_attention) and the attention kernel on the stored q | k | v (spa3d_op_attention_ragged) disagree on lse, and which of
the two is nearer fp64?  The ragged cases of tests/test_gpu_qkv_attn.py: counts of slots above 1e-3 / 1e-4 / 1e-5 and the worst six slots, each against (m, log l)
computed in fp64 from host-normalised 16-bit q^, k^.  Needs a GPU.  python tools/diag_qkv_lse.py   (figures: profiles/r20_attn_ragged.log, section B)"""
import ctypes as C, sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import torch
import test_gpu_qkv_attn as Q
import parity_util as PU
import spa3d
lib = spa3d._lib.load()
for (nseq, S, H, dtype) in ((300, 151, 8, 1), (17, 151, 8, 2), (5, 151, 8, 1)):
  lens, off, nq, w, sq, sk, km = Q._case(nseq, S, H, dtype, True, False)
  E, rows = H * 96, off[-1]
  tdt = nq.dtype
  nqd, wd, sqd, skd = nq.cuda(), [x.cuda() for x in w], sq.cuda(), sk.cuda()
  offd = torch.tensor(off, dtype=torch.int32, device='cuda')
  qkv = torch.full((rows, 3 * E), float('nan'), device='cuda', dtype=tdt)
  o = torch.full((rows, E), float('nan'), device='cuda', dtype=tdt)
  lse = torch.full((rows * H * 2,), float('nan'), device='cuda')
  ws = torch.empty(64 << 20, dtype=torch.uint8, device='cuda')
  s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  rc = lib.spa3d_op_qkv_attention(nqd.data_ptr(), 384, wd[0].data_ptr(), wd[1].data_ptr(), wd[2].data_ptr(), sqd.data_ptr(), skd.data_ptr(), None, offd.data_ptr(), nseq, S, H,
                                  qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), dtype, ws.data_ptr(), ws.numel(), s)
  assert rc == 0
  o2 = torch.empty_like(o); lse2 = torch.full((rows * H * 2,), float('nan'), device='cuda')
  rc = lib.spa3d_op_attention_ragged(qkv.data_ptr(), qkv[:, E:].data_ptr(), qkv[:, 2 * E:].data_ptr(), 3 * E, 3 * E, 3 * E, sqd.data_ptr(), skd.data_ptr(), None,
                                     (C.c_int32 * len(off))(*off), nseq, S, H, 96, o2.data_ptr(), lse2.data_ptr(), dtype, 2, ws.data_ptr(), ws.numel(), s)
  assert rc == 0
  torch.cuda.synchronize()
  d = (lse2 - lse).abs().cpu()
  print(f'case {nseq} x {S} x {H} dtype {dtype}: rows {rows}, lse slots {d.numel()}, NaN {int(torch.isnan(d).sum())}, max {float(d.max()):.3e}, '
        f'> 1e-3: {int((d > 1e-3).sum())}, > 1e-4: {int((d > 1e-4).sum())}, > 1e-5: {int((d > 1e-5).sum())}; in m (even) > 1e-4: {int((d[0::2] > 1e-4).sum())}, in log l (odd): {int((d[1::2] > 1e-4).sum())}')
  qkvh = qkv.cpu()
  l1, l2 = lse.cpu(), lse2.cpu()
  worst = torch.argsort(d, descending=True)[:6].tolist()
  for idx in worst:
    slot = idx // 2
    i = max(j for j in range(nseq) if off[j] * H <= slot)
    n = lens[i]; r = slot - off[i] * H; h, t = r // n, r % n
    sl = slice(off[i], off[i + 1])
    q = qkvh[sl, h * 96:(h + 1) * 96]; k = qkvh[sl, E + h * 96:E + (h + 1) * 96]
    qn = PU._rmsnorm16(q[None], sq, 1, 1, 96)[0, :, 0].double(); kn = PU._rmsnorm16(k[None], sk, 1, 1, 96)[0, :, 0].double()
    lg = (qn[t] * kn).sum(-1) * 0.10206207261596575
    m64 = float(lg.max()); ll64 = float(torch.log(torch.exp(lg - lg.max()).sum()))
    # sensitivity: what one 16-bit ulp on every element of q^[t] could move the max logit by
    kmax = kn[int(lg.argmax())]
    sens = float((qn[t].abs() * kmax.abs()).sum()) * 0.10206207261596575 * 2 * PU.unit_roundoff(tdt)
    print(f'  slot {slot} ({"m" if idx % 2 == 0 else "log l"}) seq {i} len {n} head {h} t {t}: qkv kernel ({float(l1[2*slot]):.6f}, {float(l1[2*slot+1]):.6f}) ragged kernel ({float(l2[2*slot]):.6f}, {float(l2[2*slot+1]):.6f}) '
          f'fp64 from host q^ k^ ({m64:.6f}, {ll64:.6f}); m + log l: {float(l1[2*slot]+l1[2*slot+1]):.6f} / {float(l2[2*slot]+l2[2*slot+1]):.6f} / {m64+ll64:.6f}; one-ulp-per-element bound on m {sens:.3e}')
