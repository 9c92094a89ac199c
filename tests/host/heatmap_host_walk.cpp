// Host-side walk of spa3d_render_heatmap under AddressSanitizer + UndefinedBehaviorSanitizer, built like windows_host_walk.cpp
// (tests/test_heatmap_host_sanitizers.py).  No GPU is touched: the entry checks everything and sizes its workspace (a dry walk of its launches
// against a counting arena) before its first launch, so each call below returns SPA3D_ERR_ARG with a message and launches nothing.  The device
// pointers are fakes that are never dereferenced; a call that got past the checks would try to launch and come back with another status, which
// fails the CHECK.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "spa3d.h"

static spa3d_config base(int T) {
  spa3d_config c;
  memset(&c, 0, sizeof c);
  c.num_output_frames = T; c.num_latent_tokens = 128; c.latent_token_dim = 96; c.num_frequencies = 32; c.track_scale_factor = 1.f;
  c.time_scale_factor = 150.f; c.track_token_dim = 384; c.encoder_latent_dim = 512; c.decoder_num_channels = 1280;
  c.num_heads = 8; c.qkv_size = 768; c.enc_mlp = 1536; c.enc_layers = 3; c.t2l_mlp = 2048; c.t2l_layers = 4; c.dec_mlp = 2048; c.dec_layers = 4;
  c.ro_mlp = 1536; c.ro_layers = 4; c.precision = SPA3D_F32; c.model_kind = 0;
  return c;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed: %s (line %d): %s\n", #x, __LINE__, h ? spa3d_last_error(h) : ""); return 1; } } while (0)

static float* const fake = (float*)(uintptr_t)0x100000;  // never dereferenced: every call below returns before its first launch
static uint8_t* const bfake = (uint8_t*)(uintptr_t)0x200000;
static const double* const dfake = (const double*)(uintptr_t)0x300000;

static spa3d_heatmap good_of(int N, int T, int H, int W, int coords) {
  spa3d_heatmap m; memset(&m, 0, sizeof m);
  m.N = N; m.T = T; m.H = H; m.W = W; m.coords = coords; m.tracks = fake; m.values = fake; m.map = fake; m.weight = fake; m.video = bfake; m.out = bfake;
  if (coords == 3) { m.intrinsics = dfake; m.extrinsics = dfake; m.resize_h = m.resize_w = 1024; }
  m.radius = 16; m.power = 2; m.normalize = 1; m.alpha = 2048;
  return m;
}
static bool refused(spa3d_handle h, const spa3d_heatmap* m, void* ws, int64_t bytes, const char* word) {
  const int rc = spa3d_render_heatmap(h, m, ws, bytes, nullptr);
  const char* e = spa3d_last_error(h);
  if (rc != SPA3D_ERR_ARG || (m && !strstr(e, "heatmap")) || !strstr(e, word)) { fprintf(stderr, "rc = %d, message '%s', wanted '%s'\n", rc, e, word); return false; }
  return true;
}
static int64_t need_of(spa3d_handle h) {
  const char* p = strstr(spa3d_last_error(h), "need ");
  return p ? atoll(p + 5) : -1;
}

int main() {
  spa3d_config cfg = base(150);
  spa3d_handle h = nullptr;
  CHECK(spa3d_create(&cfg, &h) == SPA3D_OK && h);
  const int64_t big = (int64_t)1 << 40;
  // the inference-size clip, both coordinate kinds, with and without the overlay: the dry walk sizes the workspace, and the need is within
  // spa3d_heatmap_workspace_bytes
  for (int coords : {2, 3}) {
    spa3d_heatmap m = good_of(4096, 150, 518, 518, coords);
    const int64_t cap = spa3d_heatmap_workspace_bytes(h, m.N, m.T);
    CHECK(cap > (int64_t)m.N * m.T * 8);
    CHECK(refused(h, &m, fake, 0, "workspace too small"));
    const int64_t need = need_of(h);
    CHECK(need > 0 && need <= cap);
    CHECK(refused(h, &m, nullptr, big, "workspace too small") && need_of(h) == need);
    CHECK(refused(h, &m, fake, need - 1, "workspace too small") && need_of(h) == need);
    m.out = nullptr; m.video = nullptr;
    CHECK(refused(h, &m, fake, 0, "workspace too small") && need_of(h) < need && need_of(h) > (int64_t)m.N * m.T * 8);
    m.map = nullptr;
    CHECK(refused(h, &m, fake, 0, "workspace too small"));
    m.weight = nullptr;
    CHECK(refused(h, &m, fake, big, "all NULL"));
  }
  const spa3d_heatmap good = good_of(64, 8, 37, 53, 3);
  spa3d_heatmap m;
  CHECK(refused(h, nullptr, fake, big, "required"));
  m = good; m.tracks = nullptr; CHECK(refused(h, &m, fake, big, "tracks"));
  m = good; m.values = nullptr; CHECK(refused(h, &m, fake, big, "values"));
  m = good; m.video = nullptr; CHECK(refused(h, &m, fake, big, "needs video"));
  m = good; m.use_visibility = 1; CHECK(refused(h, &m, fake, big, "needs visible"));
  for (int c : {0, 1, 4, -3}) { m = good; m.coords = c; CHECK(refused(h, &m, fake, big, "coords")); }
  m = good; m.intrinsics = nullptr; CHECK(refused(h, &m, fake, big, "camera"));
  m = good; m.extrinsics = nullptr; CHECK(refused(h, &m, fake, big, "camera"));
  m = good; m.resize_h = 0; CHECK(refused(h, &m, fake, big, "resize"));
  m = good; m.resize_w = -5; CHECK(refused(h, &m, fake, big, "resize"));
  m = good; m.N = 0; CHECK(refused(h, &m, fake, big, "positive"));
  m = good; m.T = -1; CHECK(refused(h, &m, fake, big, "positive"));
  m = good; m.N = INT32_MAX; m.T = INT32_MAX; CHECK(refused(h, &m, fake, big, "2^31"));
  m = good; m.N = 1 << 20; m.T = (1 << 11) + 1; CHECK(refused(h, &m, fake, big, "2^31"));
  m = good; m.H = 0; CHECK(refused(h, &m, fake, big, "16384"));
  m = good; m.W = 16385; CHECK(refused(h, &m, fake, big, "16384"));
  m = good; m.H = INT32_MAX; CHECK(refused(h, &m, fake, big, "16384"));
  m = good; m.T = 64; m.H = 16384; m.W = 16384; CHECK(refused(h, &m, fake, big, "2^24"));
  for (int r : {0, -1, 65, INT32_MAX, INT32_MIN}) { m = good; m.radius = r; CHECK(refused(h, &m, fake, big, "radius")); }
  for (int p : {0, 3, -2, INT32_MAX}) { m = good; m.power = p; CHECK(refused(h, &m, fake, big, "power")); }
  for (int a : {-1, 4097, INT32_MIN}) { m = good; m.alpha = a; CHECK(refused(h, &m, fake, big, "alpha")); }
  for (float v : {NAN, INFINITY, -INFINITY}) {
    m = good; m.normalize = 0; m.lo = v; m.hi = 1.f; CHECK(refused(h, &m, fake, big, "finite lo, hi"));
    m = good; m.normalize = 0; m.lo = 0.f; m.hi = v; CHECK(refused(h, &m, fake, big, "finite lo, hi"));
    m = good; m.lo = v; m.hi = v; CHECK(refused(h, &m, fake, 0, "workspace too small"));                                     // not read: the clip's own range
    m = good; m.normalize = 0; m.lo = v; m.out = nullptr; CHECK(refused(h, &m, fake, 0, "workspace too small"));              // not read: no overlay
  }
  // the largest clip one launch holds is sized without overflow: 2^31 point-frames of 8 bytes
  m = good_of(1 << 20, 1 << 11, 16384, 64, 2); m.T = 1 << 11;
  CHECK(spa3d_heatmap_workspace_bytes(h, m.N, m.T) > (int64_t)1 << 34);
  CHECK(refused(h, &m, fake, 0, "workspace too small") && need_of(h) > (int64_t)1 << 34 && need_of(h) <= spa3d_heatmap_workspace_bytes(h, m.N, m.T));
  CHECK(spa3d_heatmap_workspace_bytes(h, 0, 4) == -1 && spa3d_heatmap_workspace_bytes(h, 4, -1) == -1 && spa3d_heatmap_workspace_bytes(nullptr, 4, 4) == -1);
  CHECK(spa3d_render_heatmap(nullptr, &good, fake, big, nullptr) == SPA3D_ERR_ARG);
  CHECK(spa3d_destroy(h) == SPA3D_OK);
  puts("HOST_HEATMAP_OK");
  return 0;
}
