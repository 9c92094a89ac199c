// csrc/motion_code.hpp built with the host compiler and driven by tests/test_motion_host.py: one query per input line, one answer line each.
//   code <hex bits of a float32>   -> "<code> <1 if NaN else 0>"
//   len D | s I | S D I J          -> the state length / index
//   samples M L POOL | sqmax L POOL | nmax L POOL
//   codes N | mom M L D POOL | pd MA MB E KIND   -> the range check's result
//   consts                         -> "MC_CODE_MAX MOTION_KCHUNK MC_MAX_L MC_MAX_D MC_MAX_E MC_MAX_M"
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../3dspa_code_amd/csrc/motion_code.hpp"

int main() {
  char line[256], op[32];
  while (fgets(line, sizeof line, stdin)) {
    long long v[4] = {0, 0, 0, 0};
    unsigned bits = 0;
    if (sscanf(line, "%31s", op) != 1) continue;
    const char* rest = line + strlen(op);
    if (!strcmp(op, "code")) {
      if (sscanf(rest, "%x", &bits) != 1) return 2;
      float x;
      memcpy(&x, &bits, 4);
      bool nan = false;
      const int c = mc_code(x, &nan);
      printf("%d %d\n", c, nan ? 1 : 0);
      continue;
    }
    const int got = sscanf(rest, "%lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3]);
    if (!strcmp(op, "consts")) printf("%d %d %d %d %d %" PRId64 "\n", MC_CODE_MAX, MOTION_KCHUNK, MC_MAX_L, MC_MAX_D, MC_MAX_E, MC_MAX_M);
    else if (!strcmp(op, "len") && got == 1) printf("%" PRId64 "\n", mc_state_len((int)v[0]));
    else if (!strcmp(op, "s") && got == 1) printf("%" PRId64 "\n", mc_state_s((int)v[0]));
    else if (!strcmp(op, "S") && got == 3) printf("%" PRId64 "\n", mc_state_S((int)v[0], (int)v[1], (int)v[2]));
    else if (!strcmp(op, "samples") && got == 3) printf("%" PRId64 "\n", mc_samples(v[0], (int)v[1], (int)v[2]));
    else if (!strcmp(op, "sqmax") && got == 2) printf("%" PRId64 "\n", mc_sample_sq_max((int)v[0], (int)v[1]));
    else if (!strcmp(op, "nmax") && got == 2) printf("%" PRId64 "\n", mc_samples_max((int)v[0], (int)v[1]));
    else if (!strcmp(op, "codes") && got == 1) printf("%d\n", mc_codes_check(v[0]));
    else if (!strcmp(op, "mom") && got == 4) printf("%d\n", mc_moments_check(v[0], (int)v[1], (int)v[2], (int)v[3]));
    else if (!strcmp(op, "pd") && got == 4) printf("%d\n", mc_pdist_check(v[0], v[1], (int)v[2], (int)v[3]));
    else return 3;
  }
  return 0;
}
