// Host-side walk of RAGGED calls (spa3d_set_counts) under AddressSanitizer + UndefinedBehaviorSanitizer, built like spa3d_host_dryrun.cpp
// (tests/test_host_sanitizers.py).  No GPU is touched: every entry point validates the counts and sizes its workspace with a dry run of the
// orchestration BEFORE its first launch, so a call with a zero-byte workspace walks the whole ragged orchestration -- packed chunks,
// per-sample loops, samples without queries -- and returns SPA3D_ERR_WORKSPACE with the bytes one sample chunk needs.  Checked here:
// that need never exceeds spa3d_workspace_bytes of the padded shape (include/spa3d.h promises the bound), and every refusal.
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

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

static long long need_of(spa3d_handle h) {  // "workspace too small: need N bytes for chunk 1"
  const char* m = spa3d_last_error(h);
  const char* p = strstr(m, "need ");
  return p ? atoll(p + 5) : -1;
}

int main() {
  const int B = 4, N = 512, Q = 128, T = 150;
  float* fake = (float*)(uintptr_t)0x100000;  // never dereferenced: every call below returns before its first launch
  for (int prec : {SPA3D_BF16, SPA3D_F16, SPA3D_F32}) {
    spa3d_config c = base(T, 768, 1, prec, 0);
    spa3d_handle h = nullptr;
    CHECK(spa3d_create(&c, &h) == SPA3D_OK && h);
    spa3d_batch b; memset(&b, 0, sizeof b);
    b.B = B; b.N = N; b.Q = Q; b.T = T; b.discretize = 1;
    b.support_tracks = fake; b.support_tracks_visible = fake; b.query_points = fake; b.boundary_frame = (const int32_t*)fake;
    b.dino_features = fake; b.depth_features = fake; b.noise = fake; b.query_tracks = fake; b.query_tracks_visible = fake;
    spa3d_outputs out; out.tracks = fake; out.visible_logits = fake; out.certain_logits = fake; out.latents = fake;
    const long long bound_train = spa3d_workspace_bytes(h, B, N, Q, T, 1, 1), bound_fwd = spa3d_workspace_bytes(h, B, N, Q, T, 1, 0);
    CHECK(bound_train > 0 && bound_fwd > 0);
    const int32_t sets[][2][4] = {
        {{512, 100, 64, 300}, {128, 0, 1, 50}},     // a sample without queries, a sample with one
        {{512, 512, 512, 511}, {128, 128, 128, 127}},  // all but one row live
        {{1, 1, 1, 1}, {0, 0, 0, 0}},                  // the least of everything
        {{512, 512, 512, 512}, {128, 128, 128, 128}},  // nothing left out: the uniform call
    };
    for (auto& s : sets) {
      CHECK(spa3d_set_counts(h, B, s[0], s[1]) == SPA3D_OK);
      CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE);
      const long long need_t = need_of(h);
      CHECK(need_t > 0 && need_t <= bound_train);
      CHECK(spa3d_forward(h, fake, &b, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE);
      const long long need_f = need_of(h);
      CHECK(need_f > 0 && need_f <= bound_fwd && need_f <= need_t);
      CHECK(spa3d_encode(h, fake, &b, fake, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) <= bound_fwd);
      CHECK(spa3d_decode(h, fake, &b, fake, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) <= bound_fwd);
      printf("precision %d counts (%d %d %d %d | %d %d %d %d): one-sample need train %.3f GB (padded bound %.3f), forward %.3f GB (%.3f)\n", prec,
             s[0][0], s[0][1], s[0][2], s[0][3], s[1][0], s[1][1], s[1][2], s[1][3], need_t / 1e9, bound_train / 1e9, need_f / 1e9, bound_fwd / 1e9);
      // support counts alone, query counts alone
      CHECK(spa3d_set_counts(h, B, s[0], nullptr) == SPA3D_OK && spa3d_forward(h, fake, &b, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE);
      CHECK(spa3d_set_counts(h, B, nullptr, s[1]) == SPA3D_OK && spa3d_forward(h, fake, &b, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE);
    }
    // with a workspace that holds several samples the sizing pass packs them: walk it with chunk = 3 (one chunk of 1, one of 3)
    CHECK(spa3d_set_counts(h, B, sets[0][0], sets[0][1]) == SPA3D_OK && spa3d_set_option(h, "chunk", 3) == SPA3D_OK);
    CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) > 0);
    CHECK(need_of(h) <= spa3d_workspace_bytes(h, B, N, Q, T, 3, 1));
    // One sample alone in the first chunk and three packed in the second (B = 4, chunk = 3: B % chunk = 1) go through the same chunk driver.  The
    // sample without live queries sits alone in its chunk, then inside the packed chunk; training and forward.  The sizing walk decides the call:
    // one byte below the need it reports the call is refused with that same need (at the need it would go on to launch, which needs a device), and
    // the need of samples at their own size stays within the padded bound.
    const int32_t alone[2][4] = {{100, 512, 64, 300}, {0, 128, 1, 50}}, inside[2][4] = {{512, 100, 64, 300}, {128, 0, 1, 50}};
    for (auto s : {alone, inside}) {
      CHECK(spa3d_set_counts(h, B, s[0], s[1]) == SPA3D_OK);
      CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && strstr(spa3d_last_error(h), "for chunk 3"));
      const long long need_t = need_of(h);
      CHECK(need_t > 0 && need_t <= spa3d_workspace_bytes(h, B, N, Q, T, 3, 1));
      CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, need_t - 1, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) == need_t);
      CHECK(spa3d_forward(h, fake, &b, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && strstr(spa3d_last_error(h), "for chunk 3"));
      const long long need_f = need_of(h);
      CHECK(need_f > 0 && need_f <= need_t && need_f <= spa3d_workspace_bytes(h, B, N, Q, T, 3, 0));
      CHECK(spa3d_forward(h, fake, &b, &out, fake, need_f - 1, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) == need_f);
      printf("precision %d chunk 3 of 4, query-less sample %s: need train %.3f GB, forward %.3f GB\n", prec, s == alone ? "alone" : "packed", need_t / 1e9, need_f / 1e9);
    }
    CHECK(spa3d_set_option(h, "chunk", 0) == SPA3D_OK);
    // refusals: SPA3D_ERR_ARG with a message, before anything else happens
    const int32_t ok_n[4] = {512, 100, 64, 300}, ok_q[4] = {128, 0, 1, 50};
    const int32_t n0[4] = {512, 0, 64, 300}, nbig[4] = {512, 513, 64, 300}, qbig[4] = {128, 129, 1, 50}, qneg[4] = {128, -1, 1, 50};
    struct { const int32_t* n; const int32_t* q; int B; } bad[] = {{n0, ok_q, B}, {nbig, ok_q, B}, {ok_n, qbig, B}, {ok_n, qneg, B}, {ok_n, ok_q, B - 1}, {n0, nullptr, B}};
    for (auto& r : bad) {
      CHECK(spa3d_set_counts(h, r.B, r.n, r.q) == SPA3D_OK);
      CHECK(spa3d_forward(h, fake, &b, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && strlen(spa3d_last_error(h)) > 0);
      CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_ARG);
    }
    // every entry that reads query_count refuses counts set for another B and a count above Q, by name, before a launch
    spa3d_scores sc; memset(&sc, 0, sizeof sc); sc.query_stats = fake;
    spa3d_tapvid3d tv; memset(&tv, 0, sizeof tv); tv.query_stats = fake;
    struct { int B; const int32_t* q; const char* msg; } refused[] = {{B - 1, ok_q, "counts were set"}, {B, qbig, "query_count"}};
    for (auto& r : refused) {
      CHECK(spa3d_set_counts(h, r.B, nullptr, r.q) == SPA3D_OK);
      CHECK(spa3d_forward(h, fake, &b, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), r.msg));
      CHECK(spa3d_score_from_preds(h, &b, &out, &sc, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), r.msg));
      CHECK(spa3d_tapvid3d_from_preds(h, &b, &out, &tv, fake, 0, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), r.msg));
      CHECK(spa3d_loss(h, &b, &out, 0.f, fake, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), r.msg));
    }
    CHECK(spa3d_set_counts(h, B, ok_n, ok_q) == SPA3D_OK);
    for (const char* o : {"track_chunk", "query_chunk"}) {
      CHECK(spa3d_set_option(h, o, 32) == SPA3D_OK);
      CHECK(spa3d_forward(h, fake, &b, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "chunk"));
      CHECK(spa3d_set_option(h, o, 0) == SPA3D_OK);
    }
    CHECK(spa3d_loss(h, &b, &out, 0.f, fake + 1, nullptr) == SPA3D_ERR_ARG);  // (misaligned loss3: refused before the counts are looked at)
    CHECK(spa3d_set_counts(h, 0, ok_n, ok_q) == SPA3D_ERR_ARG);
    CHECK(spa3d_set_counts(h, 0, nullptr, nullptr) == SPA3D_OK);  // detach: the uniform call again
    CHECK(spa3d_forward(h, fake, &b, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) > 0 && need_of(h) <= bound_fwd);
    CHECK(spa3d_destroy(h) == SPA3D_OK);
  }
  {  // the 2-D twin refuses counts
    spa3d_config c = base(150, 0, 0, SPA3D_BF16, 1);
    spa3d_handle h = nullptr;
    CHECK(spa3d_create(&c, &h) == SPA3D_OK && h);
    spa3d_batch b; memset(&b, 0, sizeof b);
    b.B = 2; b.N = 64; b.Q = 16; b.T = 150; b.discretize = 1;
    b.support_tracks = fake; b.support_tracks_visible = fake; b.query_points = fake; b.boundary_frame = (const int32_t*)fake; b.noise = fake;
    spa3d_outputs out; out.tracks = fake; out.visible_logits = fake; out.certain_logits = fake; out.latents = nullptr;
    const int32_t n[2] = {64, 10}, q[2] = {16, 4};
    CHECK(spa3d_set_counts(h, 2, n, q) == SPA3D_OK);
    CHECK(spa3d_forward(h, fake, &b, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && strlen(spa3d_last_error(h)) > 0);
    CHECK(spa3d_destroy(h) == SPA3D_OK);
  }
  CHECK(spa3d_set_counts(nullptr, 1, nullptr, nullptr) == SPA3D_ERR_ARG);
  puts("HOST_RAGGED_OK");
  return 0;
}
