// Host driver for tests/test_gemm_desc_host.py: the size of spa3d_gemm_args (include/spa3d.h) and the offset of every field, one "<name> <offset>" line each,
// for the comparison with the ctypes mirror in 3dspa_code_amd/_lib.py.  The header is C: included as the callers of the library see it.
#include <cstddef>
#include <cstdio>

#include "../../include/spa3d.h"

#define F(f) std::printf(#f " %zu\n", offsetof(spa3d_gemm_args, f));

int main() {
  std::printf("sizeof %zu\n", sizeof(spa3d_gemm_args));
  F(A) F(B) F(C) F(M) F(N) F(K) F(sAm) F(sAk) F(sBk) F(sBn) F(sCm) F(nb1) F(nb2) F(bA1) F(bA2) F(bB1) F(bB2) F(bC1) F(bC2) F(alpha) F(bias) F(epi) F(aux)
  F(aux_is_residual) F(out_f32) F(accumulate) F(pre_out) F(crow_group) F(crow_skip) F(brow_group) F(brow_skip) F(seg_n) F(C_seg) F(colsum_out) F(A2) F(sA2m) F(K1)
  F(arow_idx) F(crow_idx) F(r1_x) F(r1_w) F(Bt) F(ldBt)
  return 0;
}
