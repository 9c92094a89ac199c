// Host-side walk of spa3d_render_tracks under AddressSanitizer + UndefinedBehaviorSanitizer, built like spa3d_host_tapvid3d.cpp
// (tests/test_host_sanitizers.py).  No GPU is touched: the entry validates its arguments and sizes its workspace with a dry run of its
// launches BEFORE the first real one, so a call with a zero-byte workspace walks every launch site -- small and large clips, both coordinate
// forms, with and without normalisation, visibility, `pixels`, and the positions-only form -- and returns SPA3D_ERR_ARG with the bytes it
// needs.  Checked here: that need never exceeds spa3d_render_workspace_bytes, and every refusal returns SPA3D_ERR_ARG with a message.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "spa3d.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

static long long need_of(spa3d_handle h) {  // "render: workspace too small: need N bytes"
  const char* m = spa3d_last_error(h);
  const char* p = strstr(m, "need ");
  return p ? atoll(p + 5) : -1;
}

static void* const fake = (void*)(uintptr_t)0x100000;  // never dereferenced: every call below returns before its first launch

static spa3d_render clip(int N, int T, int H, int W, int coords) {
  spa3d_render r; memset(&r, 0, sizeof r);
  r.N = N; r.T = T; r.H = H; r.W = W; r.coords = coords;
  r.video = (const uint8_t*)fake; r.out = (uint8_t*)fake; r.tracks = (const float*)fake; r.scores = (const float*)fake;
  if (coords == 3) { r.intrinsics = (const double*)fake; r.extrinsics = (const double*)fake; r.resize_h = 1024; r.resize_w = 1024; }
  r.normalize = 1; r.trail = 5; r.point_size = 2;
  return r;
}

int main() {
  spa3d_config c; memset(&c, 0, sizeof c);
  c.num_output_frames = 8; c.num_latent_tokens = 128; c.latent_token_dim = 96; c.num_frequencies = 32; c.track_scale_factor = 1.f; c.time_scale_factor = 150.f;
  c.track_token_dim = 384; c.encoder_latent_dim = 512; c.decoder_num_channels = 1280; c.num_heads = 8; c.qkv_size = 768; c.enc_mlp = 1536; c.enc_layers = 3;
  c.t2l_mlp = 2048; c.t2l_layers = 4; c.dec_mlp = 2048; c.dec_layers = 4; c.ro_mlp = 1536; c.ro_layers = 4; c.precision = SPA3D_F32; c.model_kind = 0;
  spa3d_handle h = nullptr;
  CHECK(spa3d_create(&c, &h) == SPA3D_OK && h);
  struct Shape { const char* name; int N, T, H, W; };
  const Shape shapes[] = {{"one point, one frame, one pixel", 1, 1, 1, 1}, {"test scene 40 x 7, 37 x 53", 40, 7, 37, 53}, {"2048 x 150, 512 x 512", 2048, 150, 512, 512},
                          {"65536 x 300, 4096 x 4096", 65536, 300, 4096, 4096}, {"1024 x 60, 16384 x 16384", 1024, 60, 16384, 16384}};
  for (const Shape& s : shapes) {
    const long long bound = spa3d_render_workspace_bytes(h, s.N, s.T);
    CHECK(bound > 0);
    long long most = 0;
    for (int coords : {2, 3})
      for (int normalize : {0, 1})
        for (int vis : {0, 1})
          for (int px : {0, 1})
            for (int draw : {0, 1}) {
              spa3d_render r = clip(s.N, s.T, s.H, s.W, coords);
              r.normalize = normalize;
              if (vis) { r.visible = (const float*)fake; r.use_visibility = 1; }
              if (px) r.pixels = (int32_t*)fake;
              if (!draw) { r.out = nullptr; r.video = nullptr; r.scores = nullptr; }
              if (!draw && !px) { CHECK(spa3d_render_tracks(h, &r, fake, bound, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "both NULL")); continue; }
              CHECK(spa3d_render_tracks(h, &r, fake, 0, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "workspace too small"));
              const long long need = need_of(h);
              CHECK(need > 0 && need <= bound);
              CHECK(spa3d_render_tracks(h, &r, nullptr, bound, nullptr) == SPA3D_ERR_ARG);
              CHECK(spa3d_render_tracks(h, &r, fake, need - 1, nullptr) == SPA3D_ERR_ARG && need_of(h) == need);
              if (draw) CHECK(need >= (long long)s.N * s.T * 20);  // positions, flag words, boxes
              if (need > most) most = need;
            }
    printf("%-36s spa3d_render_tracks walks; needs at most %lld of the %lld bytes spa3d_render_workspace_bytes gives\n", s.name, most, bound);
  }
  {  // refusals: SPA3D_ERR_ARG with a message, before anything else happens
    const long long bound = spa3d_render_workspace_bytes(h, 40, 7);
    spa3d_render r = clip(40, 7, 37, 53, 3);
    auto refused = [&](const spa3d_render& x, const char* word) { return spa3d_render_tracks(h, &x, fake, bound, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), word); };
    spa3d_render x = r; x.tracks = nullptr; CHECK(refused(x, "tracks"));
    x = r; x.video = nullptr; CHECK(refused(x, "video"));
    x = r; x.scores = nullptr; CHECK(refused(x, "scores"));
    x = r; x.out = nullptr; CHECK(refused(x, "both NULL"));
    x = r; x.intrinsics = nullptr; CHECK(refused(x, "camera"));
    x = r; x.extrinsics = nullptr; CHECK(refused(x, "camera"));
    x = r; x.resize_w = 0; CHECK(refused(x, "resize"));
    x = r; x.use_visibility = 1; CHECK(refused(x, "visible"));
    for (int co : {-1, 0, 1, 4}) { x = r; x.coords = co; CHECK(refused(x, "coords")); }
    for (int v : {0, -5}) { x = r; x.N = v; CHECK(refused(x, "positive")); x = r; x.T = v; CHECK(refused(x, "positive")); }
    for (int v : {0, 16385, -1}) { x = r; x.H = v; CHECK(refused(x, "16384")); x = r; x.W = v; CHECK(refused(x, "16384")); }
    for (int v : {-1, 33, 1 << 30}) { x = r; x.trail = v; CHECK(refused(x, "trail")); x = r; x.point_size = v; CHECK(refused(x, "point_size")); }
    x = r; x.N = 1 << 22; x.T = (1 << 9) + 1; CHECK(refused(x, "point-frames"));
    x = r; x.T = 64; x.H = 16384; x.W = 16384; CHECK(refused(x, "2^24"));  // 64 x 256 x 1024 tiles
    x = r; x.T = 64; x.H = 16384; x.W = 16384; x.out = nullptr; x.video = nullptr; x.scores = nullptr; x.pixels = (int32_t*)fake;
    CHECK(spa3d_render_tracks(h, &x, fake, 0, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "workspace too small"));
    CHECK(spa3d_render_tracks(h, nullptr, fake, bound, nullptr) == SPA3D_ERR_ARG && strlen(spa3d_last_error(h)) > 0);
    CHECK(spa3d_render_tracks(nullptr, &r, fake, bound, nullptr) == SPA3D_ERR_ARG);
    CHECK(spa3d_render_workspace_bytes(h, 0, 7) == -1 && spa3d_render_workspace_bytes(h, 40, 0) == -1 && spa3d_render_workspace_bytes(nullptr, 40, 7) == -1);
    puts("refusals return SPA3D_ERR_ARG with a message");
  }
  CHECK(spa3d_destroy(h) == SPA3D_OK);
  puts("HOST_RENDER_OK");
  return 0;
}
