// The kernel-sum helpers of csrc/motion_code.hpp built with the host compiler and driven by tests/test_motion_kernel_host.py: one query per input
// line, one answer line each.
//   consts                       -> "MC_KERNEL_MAX_DEGREE MC_BAD_DEGREE sizeof(mc_u128)"
//   base E                       -> C = 16384 E
//   p DOT E                      -> DOT + C
//   pow P DEG                    -> "<lo> <hi>" of P^DEG
//   add ALO AHI BLO BHI          -> "<lo> <hi>" of the 128-bit sum (unsigned decimal limbs)
//   ksum MA MB E DEG SO          -> the range check's result
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../3dspa_code_amd/csrc/motion_code.hpp"

int main() {
  char line[512], op[32];
  while (fgets(line, sizeof line, stdin)) {
    if (sscanf(line, "%31s", op) != 1) continue;
    const char* rest = line + strlen(op);
    if (!strcmp(op, "add")) {
      unsigned long long u[4];
      if (sscanf(rest, "%llu %llu %llu %llu", &u[0], &u[1], &u[2], &u[3]) != 4) return 3;
      const mc_u128 r = mc_u128_add(mc_u128{u[0], u[1]}, mc_u128{u[2], u[3]});
      printf("%" PRIu64 " %" PRIu64 "\n", r.lo, r.hi);
      continue;
    }
    long long v[5] = {0, 0, 0, 0, 0};
    const int got = sscanf(rest, "%lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4]);
    if (!strcmp(op, "consts")) printf("%d %d %zu\n", MC_KERNEL_MAX_DEGREE, (int)MC_BAD_DEGREE, sizeof(mc_u128));
    else if (!strcmp(op, "base") && got == 1) printf("%" PRId64 "\n", mc_kernel_base((int)v[0]));
    else if (!strcmp(op, "p") && got == 2) printf("%" PRIu32 "\n", mc_kernel_p((int32_t)v[0], (int)v[1]));
    else if (!strcmp(op, "pow") && got == 2) {
      const mc_u128 r = mc_kernel_pow((uint32_t)v[0], (int)v[1]);
      printf("%" PRIu64 " %" PRIu64 "\n", r.lo, r.hi);
    } else if (!strcmp(op, "ksum") && got == 5) printf("%d\n", mc_ksum_check(v[0], v[1], (int)v[2], (int)v[3], v[4]));
    else return 3;
  }
  return 0;
}
