// Host driver for tests/test_attn_plan_host.py: reads one case per line from stdin and prints what 3dspa_code_amd/csrc/attn_plan.hpp decides.
//   <fn> <impl> [field=value ...]      fn: fwd | bwd | qkv | prune | pack      impl: AttnPolicy::from_impl's argument
// Descriptor fields take integers (pointers as addresses; every operand defaults to a 16-byte aligned address, km and the qkv operands to null).
// layout=rows | keys | hole picks the layout; keys=a,b,.. are the sequences' key counts (ragged keys), holes=lo:hi,.. the holes (with Nk).
// Output per line: the route, KT, waves and splits, the partials' bytes, and the refusal's reason; prune / pack print 0 / 1.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../3dspa_code_amd/csrc/attn_plan.hpp"

static const char* name(AttnKernel k) {
  static const char* n[] = {"Refuse", "Generic", "GenericPerSeq", "SelfFwd", "XFwd", "XFwdRaggedKeys", "XFwdHole", "Bwd4", "Bwd4Fast", "BwdSplit4", "BwdSplit8",
                            "XBwd", "XBwdRaggedKeys", "QkvFwd"};
  return n[(int)k];
}
static const char* name(AttnRefusal r) { return r == AttnRefusal::None ? "" : (r == AttnRefusal::RaggedNeedsFused ? " why=ragged" : " why=not-covered"); }
static const void* P(long long v) { return (const void*)(uintptr_t)v; }

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string fn; int impl = 0;
    if (!(in >> fn >> impl)) continue;
    std::map<std::string, std::string> f;
    for (std::string kv; in >> kv;) { const size_t e = kv.find('='); f[kv.substr(0, e)] = kv.substr(e + 1); }
    auto get = [&](const char* k, long long dflt) { auto it = f.find(k); return it == f.end() ? dflt : std::strtoll(it->second.c_str(), nullptr, 0); };
    const AttnPolicy p = AttnPolicy::from_impl(impl);
    if (fn == "prune") { std::printf("%d\n", attn_takes_ragged_self(p, (int)get("S", 151), (int)get("Dh", 96), (int)get("esz", 2))); continue; }
    if (fn == "pack") { std::printf("%d\n", plan_qkv_pack(p, get("gemm_generic", 0) != 0, get("cross", 0) != 0, (int)get("d", 384), (int)get("Dh", 96))); continue; }
    AttnDesc d;
    d.q = P(get("q", 0x100000)); d.k = P(get("k", 0x200000)); d.v = P(get("v", 0x300000)); d.o = (void*)P(get("o", 0x400000)); d.lse = (float*)P(get("lse", 0x500000));
    d.sq = (const float*)P(get("sq", 0x600000)); d.sk = (const float*)P(get("sk", 0x610000)); d.km = (const float*)P(get("km", 0));
    d.nseq = get("nseq", 4); d.Sq = (int)get("Sq", get("S", 0)); d.Sk = (int)get("Sk", get("S", 0)); d.H = (int)get("H", 4); d.Dh = (int)get("Dh", 96);
    d.esz = (int)get("esz", 2);
    const int64_t E = (int64_t)d.H * d.Dh;
    d.ldq = get("ldq", E); d.ldk = get("ldk", E); d.ldv = get("ldv", E);
    d.d_o = P(get("d_o", 0x700000)); d.dq = (void*)P(get("dq", 0x800000)); d.dk = (void*)P(get("dk", 0x900000)); d.dv = (void*)P(get("dv", 0xa00000));
    d.dsq = (float*)P(0xb00000); d.dsk = (float*)P(0xb10000);
    std::vector<int32_t> host;
    const std::string layout = f.count("layout") ? f["layout"] : "dense";
    if (layout == "rows") { d.layout = AttnLayout::RaggedRows; d.seq_off = (const int32_t*)P(0xc00000); d.total_rows = get("total_rows", d.nseq * d.Sq - 3); }
    else if (layout == "keys") {
      d.layout = AttnLayout::RaggedKeys; host.push_back(0);
      std::istringstream ks(f["keys"]);
      for (std::string t; std::getline(ks, t, ',');) host.push_back(host.back() + (int32_t)std::atoi(t.c_str()));
      d.nseq = (int64_t)host.size() - 1; d.koff_host = host.data(); d.koff_dev = (const int32_t*)P(0xc00000);
    } else if (layout == "hole") {
      d.layout = AttnLayout::Hole; d.Nk = (int)get("Nk", 0);
      std::istringstream hs(f["holes"]);
      for (std::string t; std::getline(hs, t, ',');) { host.push_back((int32_t)std::atoi(t.c_str())); host.push_back((int32_t)std::atoi(t.c_str() + t.find(':') + 1)); }
      d.nseq = (int64_t)host.size() / 2; d.holes_host = host.data(); d.holes_dev = (const int32_t*)P(0xc00000);
    } else if (layout != "dense") { std::printf("bad layout %s\n", layout.c_str()); return 2; }
    if (f.count("nseq") && layout != "dense" && layout != "rows") { std::printf("nseq follows from keys= / holes=\n"); return 2; }
    AttnPlan pl;
    if (fn == "qkv") {
      d.x = P(get("x", 0xd00000)); d.ldx = get("ldx", 384); d.d = (int)get("d", 384); d.qkv_pk = P(get("pk", 0xe00000)); d.ldq = d.ldk = d.ldv = 3 * E;
      pl = plan_qkv_attn(d, p);
    } else if (fn == "fwd") pl = plan_attn_fwd(d, p);
    else if (fn == "bwd") pl = plan_attn_bwd(d, p);
    else { std::printf("bad fn %s\n", fn.c_str()); return 2; }
    std::printf("%s KT=%d NW=%d nsplit=%d part=%lld,%lld%s\n", name(pl.kernel), pl.KT, pl.NW, pl.nsplit, (long long)pl.part_bytes[0], (long long)pl.part_bytes[1],
                name(pl.why));
  }
  return 0;
}
