// The k-NN helpers of csrc/motion_code.hpp built with the host compiler and driven by tests/test_motion_knn_host.py: one query per input line, one
// answer line each.
//   consts                       -> "MC_KNN_MAX_K MC_KNN_TILE MC_KNN_MAX_SPLITS MC_KNN_TARGET_GROUPS MC_KNN_MIN_TILES MC_KNN_NONE"
//   key D J                      -> "<key> <distance read back> <index read back>"
//   less D1 J1 D2 J2             -> 1 if key(D1, J1) < key(D2, J2) else 0
//   excl I SO | adm MB SO        -> the column row I leaves out / the fewest admissible columns of a row
//   splits MA MB                 -> the planned number of column ranges
//   range TILES SPLITS S         -> "<t0> <t1>"
//   knn MA MB E K SO SPLITS | ball MA MB E SO   -> the range check's result
//   ws MA MB K SPLITS            -> the workspace bytes
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../3dspa_code_amd/csrc/motion_code.hpp"

int main() {
  char line[256], op[32];
  while (fgets(line, sizeof line, stdin)) {
    long long v[6] = {0, 0, 0, 0, 0, 0};
    if (sscanf(line, "%31s", op) != 1) continue;
    const char* rest = line + strlen(op);
    const int got = sscanf(rest, "%lld %lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]);
    if (!strcmp(op, "consts")) printf("%d %d %d %d %d %" PRIu64 "\n", MC_KNN_MAX_K, MC_KNN_TILE, MC_KNN_MAX_SPLITS, MC_KNN_TARGET_GROUPS, MC_KNN_MIN_TILES, MC_KNN_NONE);
    else if (!strcmp(op, "key") && got == 2) {
      const uint64_t key = mc_knn_key((int32_t)v[0], v[1]);
      printf("%" PRIu64 " %d %d\n", key, mc_knn_key_dist(key), mc_knn_key_idx(key));
    } else if (!strcmp(op, "less") && got == 4) printf("%d\n", mc_knn_key((int32_t)v[0], v[1]) < mc_knn_key((int32_t)v[2], v[3]) ? 1 : 0);
    else if (!strcmp(op, "excl") && got == 2) printf("%" PRId64 "\n", mc_knn_excluded(v[0], v[1]));
    else if (!strcmp(op, "adm") && got == 2) printf("%" PRId64 "\n", mc_knn_admissible(v[0], v[1]));
    else if (!strcmp(op, "splits") && got == 2) printf("%d\n", mc_knn_splits(v[0], v[1]));
    else if (!strcmp(op, "range") && got == 3) {
      int64_t t0 = -1, t1 = -1;
      mc_knn_tile_range(v[0], (int)v[1], (int)v[2], &t0, &t1);
      printf("%" PRId64 " %" PRId64 "\n", t0, t1);
    } else if (!strcmp(op, "knn") && got == 6) printf("%d\n", mc_knn_check(v[0], v[1], (int)v[2], (int)v[3], v[4], (int)v[5]));
    else if (!strcmp(op, "ball") && got == 4) printf("%d\n", mc_ball_check(v[0], v[1], (int)v[2], v[3]));
    else if (!strcmp(op, "ws") && got == 4) printf("%" PRId64 "\n", mc_knn_ws_bytes(v[0], v[1], (int)v[2], (int)v[3]));
    else return 3;
  }
  return 0;
}
