// Host-side walk of spa3d_build_batch's refusals under AddressSanitizer + UndefinedBehaviorSanitizer, built like spa3d_host_tapvid3d.cpp
// (tests/test_host_sanitizers.py).  No GPU is touched: the entry checks every clip before its first launch, so each call below returns
// SPA3D_ERR_ARG with a message and launches nothing.  The pointers are fakes that are never dereferenced; a call that got past the checks would
// try to launch and come back with another status, which fails the CHECK.
#include <cstdio>
#include <cstdlib>
#include <cstring>

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
// a clip that lifts from its depth map and samples both features from maps
static spa3d_clip clip_of(int n, int T, int ns, int nq) {
  spa3d_clip c; memset(&c, 0, sizeof c);
  c.n_tracks = n; c.T = T; c.H = 518; c.W = 518; c.tracks_2d = fake; c.visible = fake; c.depth_map = fake; c.dino_map = fake; c.Hp = 37; c.Wp = 37;
  c.n_support = ns; c.n_query = nq; c.support_index = ifake; c.query_index = ifake; c.query_frame = ifake;
  return c;
}

// the call is refused with SPA3D_ERR_ARG and a message that holds `word`
static bool refused(spa3d_handle h, const spa3d_clip* clips, spa3d_batch* out, const char* word) {
  const int rc = spa3d_build_batch(h, clips, out, nullptr);
  const char* m = spa3d_last_error(h);
  if (rc != SPA3D_ERR_ARG || !strstr(m, "build_batch") || !strstr(m, word)) { fprintf(stderr, "rc = %d, message '%s', wanted '%s'\n", rc, m, word); return false; }
  return true;
}

int main() {
  for (int prec : {SPA3D_F32, SPA3D_BF16, SPA3D_F16}) {
    spa3d_config cfg = base(150, 768, 1, prec, 0);
    spa3d_handle h = nullptr;
    CHECK(spa3d_create(&cfg, &h) == SPA3D_OK && h);
    const int B = 20, N = 2048, Q = 512, T = 150;  // more clips than one launch holds: the LAST clip is the bad one, and still nothing is launched
    spa3d_clip clips[B];
    for (int i = 0; i < B; ++i) clips[i] = clip_of(4096, 150 - i, 2048, 512);
    spa3d_batch out = out_of(B, N, Q, T, true, true);
    spa3d_clip& k = clips[B - 1];
    const spa3d_clip good = k;
    // missing pointers
    CHECK(refused(h, nullptr, &out, "clips"));
    CHECK(refused(h, clips, nullptr, "out"));
    { spa3d_batch o = out; o.support_tracks = nullptr; CHECK(refused(h, clips, &o, "support_tracks")); }
    { spa3d_batch o = out; o.support_tracks_visible = nullptr; CHECK(refused(h, clips, &o, "support_tracks_visible")); }
    { spa3d_batch o = out; o.boundary_frame = nullptr; CHECK(refused(h, clips, &o, "boundary_frame")); }
    { spa3d_batch o = out; o.query_points = nullptr; CHECK(refused(h, clips, &o, "query_points")); }
    { spa3d_batch o = out; o.query_tracks = nullptr; CHECK(refused(h, clips, &o, "query_tracks")); }
    { spa3d_batch o = out; o.query_tracks_visible = nullptr; CHECK(refused(h, clips, &o, "query_tracks_visible")); }
    k = good; k.visible = nullptr; CHECK(refused(h, clips, &out, "clip 19: visible"));
    k = good; k.support_index = nullptr; CHECK(refused(h, clips, &out, "support_index"));
    k = good; k.query_index = nullptr; CHECK(refused(h, clips, &out, "query_index"));
    k = good; k.query_frame = nullptr; CHECK(refused(h, clips, &out, "query_frame"));
    k = good; k.tracks_2d = nullptr; CHECK(refused(h, clips, &out, "tracks_2d"));
    k = good; k.tracks_2d = nullptr; k.tracks_3d = fake; CHECK(refused(h, clips, &out, "tracks_2d"));  // still samples maps
    k = good; k.dino_map = nullptr; CHECK(refused(h, clips, &out, "dino_map or dino_pool"));
    k = good; k.tracks_3d = fake; k.depth_map = nullptr; CHECK(refused(h, clips, &out, "depth_map or depth_pool"));
    // sizes of the batch and counts above N or Q, a clip without support tracks, a clip longer than the batch
    { spa3d_batch o = out; o.B = 0; CHECK(refused(h, clips, &o, "B = 0")); }
    { spa3d_batch o = out; o.N = 0; CHECK(refused(h, clips, &o, "N = 0")); }
    { spa3d_batch o = out; o.T = 0; CHECK(refused(h, clips, &o, "T = 0")); }
    { spa3d_batch o = out; o.Q = -1; CHECK(refused(h, clips, &o, "Q = -1")); }
    k = good; k.n_support = N + 1; CHECK(refused(h, clips, &out, "n_support = 2049"));
    k = good; k.n_query = Q + 1; CHECK(refused(h, clips, &out, "n_query = 513"));
    k = good; k.n_query = -1; CHECK(refused(h, clips, &out, "n_query = -1"));
    k = good; k.n_support = 0; CHECK(refused(h, clips, &out, "n_support = 0"));
    k = good; k.T = T + 1; CHECK(refused(h, clips, &out, "T = 151"));
    k = good; k.T = 0; CHECK(refused(h, clips, &out, "T = 0"));
    k = good; k.n_tracks = 0; CHECK(refused(h, clips, &out, "n_tracks = 0"));
    k = good; k.H = 0; CHECK(refused(h, clips, &out, "video size"));
    k = good; k.Wp = 0; CHECK(refused(h, clips, &out, "map size"));
    // a map and a pool for one feature
    k = good; k.dino_pool = fake; CHECK(refused(h, clips, &out, "dino_map and dino_pool are both given"));
    k = good; k.tracks_3d = fake; k.depth_pool = fake; CHECK(refused(h, clips, &out, "depth_map and depth_pool are both given"));
    // a lift without a depth map
    k = good; k.depth_map = nullptr; CHECK(refused(h, clips, &out, "a lift needs depth_map"));
    // a feature the batch does not have
    { k = good; spa3d_batch o = out; o.dino_features = nullptr; CHECK(refused(h, clips, &o, "out->dino_features is NULL")); }
    { k = good; k.dino_map = nullptr; k.dino_pool = fake; spa3d_batch o = out; o.dino_features = nullptr; CHECK(refused(h, clips, &o, "out->dino_features is NULL")); }
    { k = good; k.depth_pool = fake; spa3d_batch o = out; o.depth_features = nullptr; CHECK(refused(h, clips, &o, "out->depth_features is NULL")); }
    k = good;
    CHECK(spa3d_build_batch(nullptr, clips, &out, nullptr) == SPA3D_ERR_ARG);
    CHECK(spa3d_destroy(h) == SPA3D_OK);
  }
  {  // features the handle does not have
    spa3d_config cfg = base(150, 0, 0, SPA3D_BF16, 0);
    spa3d_handle h = nullptr;
    CHECK(spa3d_create(&cfg, &h) == SPA3D_OK && h);
    spa3d_clip c = clip_of(100, 150, 64, 16);
    spa3d_batch o = out_of(1, 64, 16, 150, true, false);
    CHECK(refused(h, &c, &o, "the handle has no DINO feature"));
    c.dino_map = nullptr;
    o = out_of(1, 64, 16, 150, false, true);
    CHECK(refused(h, &c, &o, "the handle has no depth feature"));
    CHECK(spa3d_destroy(h) == SPA3D_OK);
  }
  {  // the 2-D twin has no depth coordinate
    spa3d_config cfg = base(150, 0, 0, SPA3D_BF16, 1);
    spa3d_handle h = nullptr;
    CHECK(spa3d_create(&cfg, &h) == SPA3D_OK && h);
    spa3d_clip c = clip_of(100, 150, 64, 16);
    c.dino_map = nullptr;
    spa3d_batch o = out_of(1, 64, 16, 150, false, false);
    CHECK(refused(h, &c, &o, "model_kind 1"));
    CHECK(spa3d_destroy(h) == SPA3D_OK);
  }
  puts("HOST_BUILD_BATCH_OK");
  return 0;
}
