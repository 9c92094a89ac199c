// Host driver of 3dspa_code_amd/csrc/adamw_groups.hpp (tests/test_adamw_groups_host.py): the header is plain C++, so the validation of the range
// table of spa3d_adamw_step_groups and the element -> range lookup that its kernels run are compiled here with the host compiler.
// Input (stdin, little-endian): int64 n, int64 num, int32 null_table, then num records {int64 begin, int64 end, float32 lr_scale, float32 wd_scale}.
// Output: int32 error code (AdamwGroupsError), int32 index of the offending range (-1: none), int32 any_frozen; then, for a valid table, per element
// i of [0, n): int32 adamw_group_find(i); float32 lr_scale, wd_scale by adamw_group_at from one cursor walked over all elements in order; and
// float32 lr_scale, wd_scale by adamw_group_at from the cursor adamw_group_find(i - i % 7) (a run that starts a few elements earlier).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../3dspa_code_amd/csrc/adamw_groups.hpp"

template <typename V> static bool rd(V* p, size_t n) { return n == 0 || fread(p, sizeof(V), n, stdin) == n; }
template <typename V> static bool wr(const std::vector<V>& v) { return v.empty() || fwrite(v.data(), sizeof(V), v.size(), stdout) == v.size(); }

int main() {
  int64_t n = 0, num = 0; int32_t null_table = 0;
  if (!rd(&n, 1) || !rd(&num, 1) || !rd(&null_table, 1)) return 2;
  const int64_t stored = num < 0 || num > (1 << 16) ? 0 : num;   // an out-of-range count comes with no records
  std::vector<AdamwGroup> g((size_t)stored);
  if (!rd(g.data(), g.size())) return 3;
  int bad = -2;
  const AdamwGroup* tab = null_table ? nullptr : g.data();
  const AdamwGroupsError err = adamw_groups_check(tab, num, n, &bad);
  std::vector<int32_t> head = {(int32_t)err, (int32_t)bad, err == ADAMW_G_OK && adamw_groups_any_frozen(tab, (int)num) ? 1 : 0};
  if (!wr(head)) return 4;
  if (err != ADAMW_G_OK || n > (1 << 24)) return 0;
  std::vector<int32_t> found((size_t)n);
  std::vector<float> walk(2 * (size_t)n), jump(2 * (size_t)n);
  int k = adamw_group_find(tab, (int)num, 0);
  for (int64_t i = 0; i < n; ++i) {
    found[i] = adamw_group_find(tab, (int)num, i);
    adamw_group_at(tab, (int)num, k, i, walk[2 * i], walk[2 * i + 1]);
    int kk = adamw_group_find(tab, (int)num, i - i % 7);
    adamw_group_at(tab, (int)num, kk, i, jump[2 * i], jump[2 * i + 1]);
  }
  return wr(found) && wr(walk) && wr(jump) ? 0 : 5;
}
