// Host driver of 3dspa_code_amd/csrc/loss_point.hpp (tests/test_loss_point_host.py): the header is plain C++, so the per-point arithmetic of
// the training objective that the three loss kernels run is compiled here with the host compiler and evaluated on lists of points.
// Input (stdin, little-endian): int32 n_pos, then n_pos records {int32 kind, float32 delta, float32 d};
//                               int32 n_vis, then n_vis records {float32 beta, float32 y, float32 l}.
// Output: float32 rho[n_pos], rho'[n_pos], v[n_vis], v'[n_vis], logsig(l)[n_vis].
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../3dspa_code_amd/csrc/loss_point.hpp"

struct PosRec { int32_t kind; float delta, d; };
struct VisRec { float beta, y, l; };

template <typename V> static bool rd(V* p, size_t n) { return n == 0 || fread(p, sizeof(V), n, stdin) == n; }
template <typename V> static bool wr(const std::vector<V>& v) { return v.empty() || fwrite(v.data(), sizeof(V), v.size(), stdout) == v.size(); }

int main() {
  int32_t np = 0, nv = 0;
  if (!rd(&np, 1) || np < 0 || np > (1 << 20)) return 2;
  std::vector<PosRec> pos((size_t)np);
  if (!rd(pos.data(), pos.size())) return 3;
  if (!rd(&nv, 1) || nv < 0 || nv > (1 << 20)) return 4;
  std::vector<VisRec> vis((size_t)nv);
  if (!rd(vis.data(), vis.size())) return 5;
  std::vector<float> rho, drho, v, dv, ls;
  for (const PosRec& r : pos) { rho.push_back(loss_pos_value(r.kind, r.delta, r.d)); drho.push_back(loss_pos_deriv(r.kind, r.delta, r.d)); }
  for (const VisRec& r : vis) { v.push_back(loss_vis_value(r.beta, r.y, r.l)); dv.push_back(loss_vis_deriv(r.beta, r.y, r.l)); ls.push_back(loss_log_sigmoid(r.l)); }
  return wr(rho) && wr(drho) && wr(v) && wr(dv) && wr(ls) ? 0 : 6;
}
