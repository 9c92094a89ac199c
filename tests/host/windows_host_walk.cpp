// Host-side walk of the refusals of spa3d_build_windows and spa3d_stitch_windows under AddressSanitizer + UndefinedBehaviorSanitizer, built like
// spa3d_host_build_batch.cpp (tests/test_windows_host_sanitizers.py).  No GPU is touched: both entries check everything before their first
// launch, so each call below returns SPA3D_ERR_ARG with a message and launches nothing.  The device pointers are fakes that are never
// dereferenced; a call that got past the checks would try to launch and come back with another status, which fails the CHECK.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "spa3d.h"

static spa3d_config base(int T, int dino, int depth, int precision, int kind) {
  spa3d_config c;
  memset(&c, 0, sizeof c);
  c.num_output_frames = T; c.num_latent_tokens = 128; c.latent_token_dim = 96; c.num_frequencies = 32; c.track_scale_factor = 1.f;
  c.time_scale_factor = 150.f; c.track_token_dim = kind ? 256 : 384; c.encoder_latent_dim = 512; c.decoder_num_channels = kind ? 1024 : 1280;
  c.dino_feature_dim = dino; c.depth_feature_dim = depth; c.num_heads = 8; c.qkv_size = kind ? 512 : 768; c.enc_mlp = kind ? 1024 : 1536;
  c.enc_layers = kind ? 2 : 3; c.t2l_mlp = 2048; c.t2l_layers = kind ? 3 : 4; c.dec_mlp = 2048; c.dec_layers = kind ? 3 : 4;
  c.ro_mlp = kind ? 1024 : 1536; c.ro_layers = 4; c.precision = precision; c.model_kind = kind;
  return c;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed: %s (line %d): %s\n", #x, __LINE__, h ? spa3d_last_error(h) : ""); return 1; } } while (0)

static float* const fake = (float*)(uintptr_t)0x100000;  // never dereferenced: every call below returns before its first launch
static const int32_t* const ifake = (const int32_t*)(uintptr_t)0x200000;

static spa3d_batch out_of(int B, int N, int Q, int T, bool dino, bool depth) {
  spa3d_batch b; memset(&b, 0, sizeof b);
  b.B = B; b.N = N; b.Q = Q; b.T = T;
  b.support_tracks = fake; b.support_tracks_visible = fake; b.query_points = fake; b.boundary_frame = ifake; b.query_tracks = fake; b.query_tracks_visible = fake;
  if (dino) b.dino_features = fake;
  if (depth) b.depth_features = fake;
  return b;
}
// a long clip that lifts from its depth map and samples both features from maps
static spa3d_clip clip_of(int n, int T, int ns, int nq) {
  spa3d_clip c; memset(&c, 0, sizeof c);
  c.n_tracks = n; c.T = T; c.H = 518; c.W = 518; c.tracks_2d = fake; c.visible = fake; c.depth_map = fake; c.dino_map = fake; c.Hp = 37; c.Wp = 37;
  c.n_support = ns; c.n_query = nq; c.support_index = ifake; c.query_index = ifake; c.query_frame = ifake;
  return c;
}

static bool refused_build(spa3d_handle h, const spa3d_clip* clip, int W, const int32_t* t0, spa3d_batch* out, const char* word) {
  const int rc = spa3d_build_windows(h, clip, W, t0, out, nullptr);
  const char* m = spa3d_last_error(h);
  if (rc != SPA3D_ERR_ARG || !strstr(m, "build_windows") || !strstr(m, word)) { fprintf(stderr, "rc = %d, message '%s', wanted '%s'\n", rc, m, word); return false; }
  return true;
}
static bool refused_stitch(spa3d_handle h, const spa3d_stitch* s, const char* word) {
  const int rc = spa3d_stitch_windows(h, s, nullptr);
  const char* m = spa3d_last_error(h);
  if (rc != SPA3D_ERR_ARG || !strstr(m, "stitch_windows") || !strstr(m, word)) { fprintf(stderr, "rc = %d, message '%s', wanted '%s'\n", rc, m, word); return false; }
  return true;
}

int main() {
  for (int prec : {SPA3D_F32, SPA3D_BF16, SPA3D_F16}) {
    spa3d_config cfg = base(150, 768, 1, prec, 0);
    spa3d_handle h = nullptr;
    CHECK(spa3d_create(&cfg, &h) == SPA3D_OK && h);
    // 600 frames at stride 25: 19 windows, more than one launch holds; the LAST start is the bad one, and still nothing is launched
    const int W = 19, N = 4096, Q = 16, Tw = 150, TL = 600;
    int32_t t0[W];
    for (int w = 0; w < W; ++w) t0[w] = 25 * w;
    spa3d_clip clip = clip_of(4096, TL, N, Q);
    const spa3d_clip good = clip;
    spa3d_batch out = out_of(W, N, Q, Tw, true, true);
    // the plan
    CHECK(refused_build(h, &clip, 0, t0, &out, "W = 0"));
    CHECK(refused_build(h, &clip, W - 1, t0, &out, "out->B = 19"));
    CHECK(refused_build(h, &clip, W, nullptr, &out, "t0 is required"));
    { int32_t t[W]; memcpy(t, t0, sizeof t); t[W - 1] = TL; CHECK(refused_build(h, &clip, W, t, &out, "t0[18] = 600")); }
    { int32_t t[W]; memcpy(t, t0, sizeof t); t[0] = -1; CHECK(refused_build(h, &clip, W, t, &out, "t0[0] = -1")); }
    { int32_t t[W]; memcpy(t, t0, sizeof t); t[W - 1] = t[W - 2]; CHECK(refused_build(h, &clip, W, t, &out, "increase strictly")); }
    { int32_t t[W]; memcpy(t, t0, sizeof t); t[3] = 10; CHECK(refused_build(h, &clip, W, t, &out, "increase strictly")); }
    // what spa3d_build_batch refuses, except a clip longer than the batch
    CHECK(refused_build(h, nullptr, W, t0, &out, "clip is required"));
    CHECK(refused_build(h, &clip, W, t0, nullptr, "out is required"));
    { spa3d_batch o = out; o.support_tracks = nullptr; CHECK(refused_build(h, &clip, W, t0, &o, "support_tracks")); }
    { spa3d_batch o = out; o.boundary_frame = nullptr; CHECK(refused_build(h, &clip, W, t0, &o, "boundary_frame")); }
    { spa3d_batch o = out; o.query_points = nullptr; CHECK(refused_build(h, &clip, W, t0, &o, "query_points")); }
    { spa3d_batch o = out; o.N = 0; CHECK(refused_build(h, &clip, W, t0, &o, "N = 0")); }
    { spa3d_batch o = out; o.T = 0; CHECK(refused_build(h, &clip, W, t0, &o, "T = 0")); }
    clip = good; clip.T = 0; CHECK(refused_build(h, &clip, W, t0, &out, "T = 0 must be positive"));
    clip = good; clip.n_tracks = 0; CHECK(refused_build(h, &clip, W, t0, &out, "n_tracks = 0"));
    clip = good; clip.n_support = N + 1; CHECK(refused_build(h, &clip, W, t0, &out, "n_support = 4097"));
    clip = good; clip.n_query = Q + 1; CHECK(refused_build(h, &clip, W, t0, &out, "n_query = 17"));
    clip = good; clip.visible = nullptr; CHECK(refused_build(h, &clip, W, t0, &out, "visible"));
    clip = good; clip.support_index = nullptr; CHECK(refused_build(h, &clip, W, t0, &out, "support_index"));
    clip = good; clip.query_frame = nullptr; CHECK(refused_build(h, &clip, W, t0, &out, "query_frame"));
    clip = good; clip.tracks_2d = nullptr; CHECK(refused_build(h, &clip, W, t0, &out, "tracks_2d"));
    clip = good; clip.depth_map = nullptr; CHECK(refused_build(h, &clip, W, t0, &out, "a lift needs depth_map"));
    clip = good; clip.dino_map = nullptr; CHECK(refused_build(h, &clip, W, t0, &out, "dino_map or dino_pool"));
    clip = good; clip.dino_pool = fake; CHECK(refused_build(h, &clip, W, t0, &out, "dino_map and dino_pool are both given"));
    clip = good; clip.tracks_3d = fake; clip.depth_pool = fake; CHECK(refused_build(h, &clip, W, t0, &out, "depth_map and depth_pool are both given"));
    clip = good; clip.H = 0; CHECK(refused_build(h, &clip, W, t0, &out, "video size"));
    clip = good; clip.Wp = 0; CHECK(refused_build(h, &clip, W, t0, &out, "map size"));
    { clip = good; spa3d_batch o = out; o.dino_features = nullptr; CHECK(refused_build(h, &clip, W, t0, &o, "out->dino_features is NULL")); }
    clip = good;
    CHECK(spa3d_build_windows(nullptr, &clip, W, t0, &out, nullptr) == SPA3D_ERR_ARG);
    // spa3d_build_batch still refuses the long clip
    { spa3d_batch o = out_of(1, N, Q, Tw, true, true); CHECK(spa3d_build_batch(h, &clip, &o, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "T = 600")); }
    CHECK(spa3d_destroy(h) == SPA3D_OK);
  }
  {  // the 2-D twin has no depth coordinate
    spa3d_config cfg = base(150, 0, 0, SPA3D_BF16, 1);
    spa3d_handle h = nullptr;
    CHECK(spa3d_create(&cfg, &h) == SPA3D_OK && h);
    spa3d_clip c = clip_of(100, 300, 64, 0);
    c.dino_map = nullptr;
    const int32_t t0[2] = {0, 150};
    spa3d_batch o = out_of(2, 64, 0, 150, false, false);
    CHECK(refused_build(h, &c, 2, t0, &o, "model_kind 1"));
    CHECK(spa3d_destroy(h) == SPA3D_OK);
  }
  {  // spa3d_stitch_windows
    spa3d_config cfg = base(150, 0, 0, SPA3D_F32, 0);
    spa3d_handle h = nullptr;
    CHECK(spa3d_create(&cfg, &h) == SPA3D_OK && h);
    const int32_t t0[7] = {0, 75, 150, 225, 300, 375, 450};
    spa3d_stitch good; memset(&good, 0, sizeof good);
    good.W = 7; good.N = 4096; good.Tw = 150; good.TL = 600; good.NC = 3; good.blend = SPA3D_BLEND_HAT; good.t0 = t0;
    good.row_track = ifake; good.tracks = fake; good.visible_logits = fake; good.frame_err = fake;
    good.out_tracks = fake; good.out_visible_logits = fake; good.out_frame_err = fake; good.out_spread = fake;
    spa3d_stitch s;
    CHECK(refused_stitch(h, nullptr, "required"));
    s = good; s.out_tracks = s.out_visible_logits = s.out_frame_err = s.out_spread = nullptr; CHECK(refused_stitch(h, &s, "no output"));
    s = good; s.tracks = nullptr; s.out_spread = nullptr; CHECK(refused_stitch(h, &s, "out_tracks needs tracks"));
    s = good; s.tracks = nullptr; s.out_tracks = nullptr; CHECK(refused_stitch(h, &s, "out_spread needs tracks"));
    s = good; s.visible_logits = nullptr; CHECK(refused_stitch(h, &s, "out_visible_logits needs visible_logits"));
    s = good; s.frame_err = nullptr; CHECK(refused_stitch(h, &s, "out_frame_err needs frame_err"));
    s = good; s.t0 = nullptr; CHECK(refused_stitch(h, &s, "t0 is required"));
    s = good; s.W = 0; CHECK(refused_stitch(h, &s, "W = 0"));
    s = good; s.W = 257; CHECK(refused_stitch(h, &s, "W = 257"));
    s = good; s.N = 0; CHECK(refused_stitch(h, &s, "N = 0"));
    s = good; s.N = (1 << 24) + 1; CHECK(refused_stitch(h, &s, "N = 16777217"));
    s = good; s.Tw = 0; CHECK(refused_stitch(h, &s, "Tw = 0"));
    s = good; s.TL = 0; CHECK(refused_stitch(h, &s, "TL = 0"));
    s = good; s.NC = 1; CHECK(refused_stitch(h, &s, "NC = 1"));
    s = good; s.NC = 4; CHECK(refused_stitch(h, &s, "NC = 4"));
    s = good; s.blend = 3; CHECK(refused_stitch(h, &s, "blend = 3"));
    s = good; s.blend = -1; CHECK(refused_stitch(h, &s, "blend = -1"));
    { int32_t t[7]; memcpy(t, t0, sizeof t); t[6] = 600; s = good; s.t0 = t; CHECK(refused_stitch(h, &s, "t0[6] = 600")); }
    { int32_t t[7]; memcpy(t, t0, sizeof t); t[2] = 75; s = good; s.t0 = t; CHECK(refused_stitch(h, &s, "increase strictly")); }
    { int32_t t[7]; memcpy(t, t0, sizeof t); t[3] = 301; t[4] = 302; s = good; s.t0 = t; CHECK(refused_stitch(h, &s, "gap")); }   // frame 300 is covered by none
    { int32_t t[7]; memcpy(t, t0, sizeof t); t[0] = 1; s = good; s.t0 = t; CHECK(refused_stitch(h, &s, "gap")); }
    s = good; s.W = 6; CHECK(refused_stitch(h, &s, "gap"));                                                                    // frames 525.. are covered by none
    { const int32_t len[7] = {150, 150, 150, 150, 150, 150, 151}; s = good; s.len = len; CHECK(refused_stitch(h, &s, "len[6] = 151")); }
    { const int32_t len[7] = {150, 150, 0, 150, 150, 150, 150}; s = good; s.len = len; CHECK(refused_stitch(h, &s, "len[2] = 0")); }
    { const int32_t len[7] = {150, 150, 150, 150, 150, 150, 149}; s = good; s.len = len; CHECK(refused_stitch(h, &s, "gap")); }
    CHECK(spa3d_stitch_windows(nullptr, &good, nullptr) == SPA3D_ERR_ARG);
    // the largest plan: 256 windows by value
    std::vector<int32_t> many(257);
    for (int w = 0; w < 257; ++w) many[w] = w;
    s = good; s.W = 256; s.t0 = many.data(); s.TL = 255 + 150 + 1; CHECK(refused_stitch(h, &s, "gap"));
    CHECK(spa3d_destroy(h) == SPA3D_OK);
  }
  puts("HOST_WINDOWS_OK");
  return 0;
}
