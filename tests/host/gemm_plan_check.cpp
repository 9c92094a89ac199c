// Host driver for tests/test_gemm_plan_host.py: reads one case per line from stdin and prints what 3dspa_code_amd/csrc/gemm_plan.hpp decides.
//   <fn> <impl> [field=value ...]      fn: gemm | nt | tn | mlp | lin | embed | kernels      impl: GemmPolicy::from_impl's argument
// Descriptor fields take integers (pointers as addresses; A, B, C default to 16-byte aligned addresses).  Output per line: the kernel name,
// and for tn / gemm "+colsum" when the dW plan fuses the column sums; lin prints its four stream flags, embed 0 / 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../../3dspa_code_amd/csrc/gemm_plan.hpp"

static const char* name(GemmKernel k) {
  static const char* n[] = {"Refuse", "Generic", "Rs", "Ntb", "MlpFused", "NtEmbed", "Nt8pp256", "Nt8pp384", "Nt8p256", "Nt8p384", "NtOcc", "Nt",
                            "Tnb", "Tn8p256", "Tn8p128x384", "Tn8p384x128", "Tn"};
  return n[(int)k];
}
static const void* P(long long v) { return (const void*)(uintptr_t)v; }

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string fn; int impl = 0;
    if (!(in >> fn >> impl)) continue;
    std::map<std::string, long long> f;
    for (std::string kv; in >> kv;) { const size_t e = kv.find('='); f[kv.substr(0, e)] = std::strtoll(kv.c_str() + e + 1, nullptr, 0); }
    auto get = [&](const char* k, long long dflt) { auto it = f.find(k); return it == f.end() ? dflt : it->second; };
    const GemmPolicy p = GemmPolicy::from_impl(impl);
    GemmDesc d{};
    d.A = P(get("A", 0x100000)); d.B = P(get("B", 0x200000)); d.C = (void*)P(get("C", 0x300000));
    d.M = get("M", 0); d.N = (int32_t)get("N", 0); d.K = (int32_t)get("K", 0);
    d.sAm = get("sAm", d.K); d.sAk = get("sAk", 1); d.sBk = get("sBk", d.N); d.sBn = get("sBn", 1); d.sCm = get("sCm", d.N);
    d.nb1 = (int32_t)get("nb1", 1); d.alpha = (float)get("alpha", 1);
    d.bias = (const float*)P(get("bias", 0)); d.epi = (int)get("epi", EPI_NONE); d.aux = P(get("aux", 0));
    d.out_f32 = (int)get("out_f32", 0); d.accumulate = (int)get("accumulate", 0); d.atomic = (int)get("atomic", 0);
    d.colsum_out = (float*)P(get("colsum", 0)); d.Bt = P(get("Bt", 0)); d.ldBt = get("ldBt", 0);
    d.rs_pk = P(get("rs_pk", 0)); d.ntb_pk = P(get("ntb_pk", 0));
    d.crow_group = (int32_t)get("crow_group", 0); d.brow_group = (int32_t)get("brow_group", 0); d.brow_skip = (int32_t)get("brow_skip", 0);
    d.pre_out = (void*)P(get("pre_out", 0)); d.zero_page = P(get("zero_page", 0));
    d.A2 = P(get("A2", 0)); d.sA2m = get("sA2m", 0); d.K1 = (int32_t)get("K1", 0);
    d.arow_idx = (const int32_t*)P(get("arow", 0)); d.crow_idx = (const int32_t*)P(get("crow", 0));
    d.r1_x = P(get("r1_x", 0)); d.r1_w = (const float*)P(get("r1_w", 0)); d.seg_n = (int32_t)get("seg_n", 0);
    if (fn == "kernels") {  // the catalogue: one "<GemmKernel value> <name>" line per kernel
      for (int i = 0; i <= (int)GemmKernel::Tn; ++i) std::printf("%d %s\n", i, name((GemmKernel)i));
      continue;
    }
    if (fn == "lin") {
      const LinStreams s = plan_lin_streams(p, (int)get("K", 0), (int)get("N", 0), (int)get("segw", get("N", 0)), (int)get("nseg", 1), get("train", 1) != 0);
      std::printf("rs=%d rs_t=%d ntb=%d ntb_t=%d\n", s.rs, s.rs_t, s.ntb, s.ntb_t);
      continue;
    }
    if (fn == "embed") {
      std::printf("%d\n", plan_embed_pack(p, get("twoD", 0) != 0, (int)get("d", 384), (int)get("tokK", 256), (int)get("dino", 768), (int)get("depth", 1)));
      continue;
    }
    GemmKernel k;
    if (fn == "mlp") {
      const long long al = 0x400000;
      k = plan_mlp(p, get("M", 4096), (int)get("d", 384), (int)get("mlp", 1536), P(get("wpk", al)), (const float*)P(get("b_in", al)),
                   (const float*)P(get("b_out", al)), P(get("na", al)), P(get("a", al)), P(get("y", al)), P(get("h", al)), P(get("hpre", al)));
      std::printf("%s %d\n", name(k), plan_mlp_pack(p, get("cross", 0) != 0, (int)get("d", 384), (int)get("mlp", 1536)));
      continue;
    }
    if (fn == "nt") k = plan_nt(d, p);
    else if (fn == "tn") k = plan_tn(d, p);
    else if (fn == "gemm") k = plan_gemm(d, p);
    else { std::printf("bad fn %s\n", fn.c_str()); return 2; }
    std::printf("%s%s flags=%lld\n", name(k), gemm_tn_fuses_colsum(k, d) ? "+colsum" : "", (long long)gemm_prof_flags(k, d, 7));
  }
  return 0;
}
