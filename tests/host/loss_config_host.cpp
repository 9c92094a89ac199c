// Host-side walk of the configurable objective (spa3d_set_loss, spa3d_set_point_weights) under AddressSanitizer + UndefinedBehaviorSanitizer,
// built like the spa3d_host_*.cpp drivers (tests/test_loss_config_host_sanitizers.py).  No GPU is touched: every entry point validates its
// arguments and sizes its workspace with a dry run of the orchestration BEFORE its first launch, so a train call with a zero-byte workspace
// walks the whole orchestration -- with the weight plane offset at every place the targets are -- and returns SPA3D_ERR_WORKSPACE.  Walked
// here: a train call with a configuration and a weight plane, a packed ragged call, a query-chunked call, det_grads, and every refusal.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

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
static spa3d_loss_config defaults() {
  spa3d_loss_config d;
  d.l1_weight = 5000.f; d.bce_weight = 1e-8f; d.position_kind = SPA3D_POS_L1; d.huber_delta = 1.f;
  d.axis_weight[0] = d.axis_weight[1] = d.axis_weight[2] = 1.f; d.bce_pos_weight = 1.f;
  return d;
}
static bool same(const spa3d_loss_config& a, const spa3d_loss_config& b) { return memcmp(&a, &b, sizeof a) == 0; }

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

static long long need_of(spa3d_handle h) {  // "workspace too small: need N bytes for chunk 1"
  const char* m = spa3d_last_error(h);
  const char* p = strstr(m, "need ");
  return p ? atoll(p + 5) : -1;
}

int main() {
  const int B = 4, N = 256, Q = 64, T = 150;
  float* fake = (float*)(uintptr_t)0x100000;  // never dereferenced: every call below returns before its first launch
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  spa3d_loss_config e = defaults();   // Huber, axis weights, weighted BCE
  e.l1_weight = 1.f; e.bce_weight = 1.f; e.position_kind = SPA3D_POS_HUBER; e.huber_delta = 1.f; e.axis_weight[1] = 0.5f; e.axis_weight[2] = 0.25f; e.bce_pos_weight = 3.f;
  for (int prec : {SPA3D_BF16, SPA3D_F16, SPA3D_F32}) {
    spa3d_config c = base(T, 768, 1, prec, 0);
    spa3d_handle h = nullptr;
    CHECK(spa3d_create(&c, &h) == SPA3D_OK && h);
    spa3d_batch b; memset(&b, 0, sizeof b);
    b.B = B; b.N = N; b.Q = Q; b.T = T; b.discretize = 1;
    b.support_tracks = fake; b.support_tracks_visible = fake; b.query_points = fake; b.boundary_frame = (const int32_t*)fake;
    b.dino_features = fake; b.depth_features = fake; b.noise = fake; b.query_tracks = fake; b.query_tracks_visible = fake;
    spa3d_outputs out; out.tracks = fake; out.visible_logits = fake; out.certain_logits = fake; out.latents = fake;
    spa3d_loss_config got;
    CHECK(spa3d_get_loss(h, &got) == SPA3D_OK && same(got, defaults()));
    CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE);
    const long long plain = need_of(h);
    CHECK(plain > 0);
    // a configuration and a weight plane cost no workspace
    CHECK(spa3d_set_loss(h, &e) == SPA3D_OK && spa3d_get_loss(h, &got) == SPA3D_OK && same(got, e));
    CHECK(spa3d_set_point_weights(h, B, Q, fake) == SPA3D_OK);
    CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) == plain);
    CHECK(spa3d_set_option(h, "det_grads", 1) == SPA3D_OK);
    CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) > plain);
    CHECK(spa3d_set_option(h, "det_grads", 0) == SPA3D_OK);
    // a packed ragged call (one chunk of 1, one of 3) and its single-sample form
    const int32_t cn[4] = {256, 100, 64, 200}, cq[4] = {64, 0, 1, 30};
    CHECK(spa3d_set_counts(h, B, cn, cq) == SPA3D_OK && spa3d_set_option(h, "chunk", 3) == SPA3D_OK);
    CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) > 0);
    CHECK(spa3d_set_option(h, "chunk", 1) == SPA3D_OK);
    CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) > 0);
    CHECK(spa3d_set_option(h, "chunk", 0) == SPA3D_OK && spa3d_set_counts(h, 0, nullptr, nullptr) == SPA3D_OK);
    // a query-chunked and a track-chunked call
    CHECK(spa3d_set_option(h, "query_chunk", 16) == SPA3D_OK);
    CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) > 0 && need_of(h) < plain);
    CHECK(spa3d_set_option(h, "track_chunk", 100) == SPA3D_OK);
    CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) > 0);
    CHECK(spa3d_set_option(h, "query_chunk", 0) == SPA3D_OK && spa3d_set_option(h, "track_chunk", 0) == SPA3D_OK);
    // the forward pass and the scores read neither
    CHECK(spa3d_forward(h, fake, &b, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE);
    // a weight plane stated for another shape: the train call and spa3d_loss refuse before a launch, the forward pass does not look
    for (int k = 0; k < 2; ++k) {
      CHECK(spa3d_set_point_weights(h, B + (k == 0), Q + (k == 1), fake) == SPA3D_OK);
      CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "point weights were set for"));
      CHECK(spa3d_loss(h, &b, &out, 0.f, fake, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "point weights were set for"));
      CHECK(spa3d_forward(h, fake, &b, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE);
    }
    CHECK(spa3d_set_point_weights(h, 0, Q, fake) == SPA3D_ERR_ARG && spa3d_set_point_weights(h, B, -1, fake) == SPA3D_ERR_ARG);
    CHECK(spa3d_set_point_weights(h, 0, 0, nullptr) == SPA3D_OK);
    CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) == plain);
    // every refusal of spa3d_set_loss, each leaving the stored configuration (e) in place
    spa3d_loss_config bad[16]; int nb = 0;
    for (auto& x : bad) x = defaults();
    bad[nb++].l1_weight = nan; bad[nb++].bce_weight = inf; bad[nb++].bce_pos_weight = nan; bad[nb++].axis_weight[2] = inf;
    bad[nb].position_kind = SPA3D_POS_HUBER; bad[nb++].huber_delta = nan;
    bad[nb++].l1_weight = -1.f; bad[nb++].bce_weight = -1.f; bad[nb++].axis_weight[0] = -1.f; bad[nb++].bce_pos_weight = -1.f;
    bad[nb++].position_kind = 2; bad[nb++].position_kind = -1;
    bad[nb].position_kind = SPA3D_POS_HUBER; bad[nb++].huber_delta = 0.f;
    bad[nb].axis_weight[0] = bad[nb].axis_weight[1] = bad[nb].axis_weight[2] = 0.f; ++nb;
    bad[nb].l1_weight = 0.f; bad[nb++].bce_weight = 0.f;
    bad[nb++].l1_weight = 2147483648.f;
    bad[nb].l1_weight = 0.f; bad[nb].bce_weight = 1073741824.f; bad[nb++].bce_pos_weight = 2.f;
    CHECK(nb == 16);
    for (int i = 0; i < nb; ++i) {
      CHECK(spa3d_set_loss(h, &bad[i]) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "spa3d_set_loss") == spa3d_last_error(h));
      CHECK(spa3d_get_loss(h, &got) == SPA3D_OK && same(got, e));
    }
    spa3d_loss_config edge = defaults(); edge.l1_weight = 1073741824.f;   // g_max = 2^30 is allowed
    CHECK(spa3d_set_loss(h, &edge) == SPA3D_OK);
    CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE);
    CHECK(spa3d_set_loss(h, nullptr) == SPA3D_OK && spa3d_get_loss(h, &got) == SPA3D_OK && same(got, defaults()));
    CHECK(spa3d_get_loss(h, nullptr) == SPA3D_ERR_ARG);
    CHECK(spa3d_destroy(h) == SPA3D_OK);
  }
  {  // the 2-D twin reads two axis weights
    spa3d_config c = base(150, 0, 0, SPA3D_BF16, 1);
    spa3d_handle h = nullptr;
    CHECK(spa3d_create(&c, &h) == SPA3D_OK && h);
    spa3d_loss_config z = defaults(); z.axis_weight[0] = z.axis_weight[1] = 0.f;
    CHECK(spa3d_set_loss(h, &z) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "axis_weight"));
    z = defaults(); z.axis_weight[2] = nan;
    CHECK(spa3d_set_loss(h, &z) == SPA3D_OK);
    spa3d_batch b; memset(&b, 0, sizeof b);
    b.B = 2; b.N = 64; b.Q = 16; b.T = 150; b.discretize = 1;
    b.support_tracks = fake; b.support_tracks_visible = fake; b.query_points = fake; b.boundary_frame = (const int32_t*)fake; b.noise = fake;
    b.query_tracks = fake; b.query_tracks_visible = fake;
    CHECK(spa3d_set_point_weights(h, 2, 16, fake) == SPA3D_OK);
    CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, nullptr, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) > 0);
    CHECK(spa3d_destroy(h) == SPA3D_OK);
  }
  CHECK(spa3d_set_loss(nullptr, nullptr) == SPA3D_ERR_ARG && spa3d_set_point_weights(nullptr, 1, 1, fake) == SPA3D_ERR_ARG);
  puts("HOST_LOSS_CONFIG_OK");
  return 0;
}
