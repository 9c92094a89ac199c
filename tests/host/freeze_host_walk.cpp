// Host-side walk of training calls under the "freeze" option (include/spa3d.h, spa3d_set_option) under AddressSanitizer + UndefinedBehaviorSanitizer,
// built like spa3d_host_ragged.cpp (tests/test_freeze_host_sanitizers.py).  No GPU is touched: spa3d_loss_and_grads sizes its workspace with a dry run
// of the orchestration before its first launch, so a call with a zero-byte workspace walks the shortened route of run_chunk (csrc/model.hip) -- the
// no-stash stages, their early releases, the skipped backward stages -- and returns SPA3D_ERR_WORKSPACE with the bytes one chunk needs.  Checked here:
// the need falls with the frozen stages, stays at or above the forward's, stays within spa3d_workspace_bytes(train = 1) of the stored option, and the walk holds
// for uniform, ragged (alone and packed) and intra-sample-chunked calls of both model kinds in every precision.
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

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

static long long need_of(spa3d_handle h) {  // "workspace too small: need N bytes for chunk 1"
  const char* m = spa3d_last_error(h);
  const char* p = strstr(m, "need ");
  return p ? atoll(p + 5) : -1;
}

int main() {
  const int B = 4, N = 512, Q = 128, T = 150;
  float* fake = (float*)(uintptr_t)0x100000;  // never dereferenced: every call below returns before its first launch
  for (int kind : {0, 1})
    for (int prec : {SPA3D_BF16, SPA3D_F16, SPA3D_F32}) {
      spa3d_config c = base(T, kind ? 0 : 768, kind ? 0 : 1, prec, kind);
      spa3d_handle h = nullptr;
      CHECK(spa3d_create(&c, &h) == SPA3D_OK && h);
      spa3d_batch b; memset(&b, 0, sizeof b);
      b.B = B; b.N = N; b.Q = Q; b.T = T; b.discretize = 1;
      b.support_tracks = fake; b.support_tracks_visible = fake; b.query_points = fake; b.boundary_frame = (const int32_t*)fake;
      if (!kind) { b.dino_features = fake; b.depth_features = fake; }
      b.noise = fake; b.query_tracks = fake; b.query_tracks_visible = fake;
      spa3d_outputs out; out.tracks = fake; out.visible_logits = fake; out.certain_logits = fake; out.latents = fake;
      int64_t seg[4], r[2];
      CHECK(spa3d_grad_segments(h, seg) == SPA3D_OK && spa3d_trainable_range(h, r) == SPA3D_OK && r[0] == 0 && r[1] == seg[3]);
      auto train_need = [&]() -> long long {
        return spa3d_loss_and_grads(h, fake, &b, 0.f, fake, 0, fake, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE ? need_of(h) : -1;
      };
      CHECK(spa3d_forward(h, fake, &b, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE);
      const long long fwd = need_of(h);
      long long w[3];
      for (int k = 0; k < 3; ++k) {
        CHECK(spa3d_set_option(h, "freeze", k) == SPA3D_OK && spa3d_trainable_range(h, r) == SPA3D_OK && r[0] == seg[k] && r[1] == seg[3]);
        w[k] = train_need();
        CHECK(w[k] > 0 && w[k] <= spa3d_workspace_bytes(h, B, N, Q, T, 1, 1));  // (the sizing batch also holds the noise the call was given)
        CHECK(spa3d_forward(h, fake, &b, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) == fwd);  // every other entry ignores the option
        // one byte below the need the call is refused with that same need; accumulate walks the same route
        CHECK(spa3d_loss_and_grads(h, fake, &b, 0.f, fake, prec != SPA3D_F16, fake, &out, fake, w[k] - 1, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) == w[k]);
      }
      CHECK(w[0] > w[1] && w[1] > w[2] && w[2] >= fwd);
      for (double bad : {-1.0, 3.0, 0.5}) {
        CHECK(spa3d_set_option(h, "freeze", bad) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "freeze"));
        CHECK(spa3d_trainable_range(h, r) == SPA3D_OK && r[0] == seg[2]);
      }
      printf("kind %d precision %d: one-sample need train %.3f / %.3f / %.3f GB at freeze 0 / 1 / 2, forward %.3f GB\n", kind, prec, w[0] / 1e9, w[1] / 1e9,
             w[2] / 1e9, fwd / 1e9);
      for (int k = 1; k < 3; ++k) {
        CHECK(spa3d_set_option(h, "freeze", k) == SPA3D_OK);
        // several samples per chunk (one chunk of 1, one of 3)
        CHECK(spa3d_set_option(h, "chunk", 3) == SPA3D_OK);
        const long long w3 = train_need();
        CHECK(w3 >= w[k] && w3 <= spa3d_workspace_bytes(h, B, N, Q, T, 3, 1));
        if (!kind) {  // ragged: the query-less sample alone in the first chunk, then inside the packed one
          const int32_t alone[2][4] = {{100, 512, 64, 300}, {0, 128, 1, 50}}, inside[2][4] = {{512, 100, 64, 300}, {128, 0, 1, 50}};
          for (auto s : {alone, inside}) {
            CHECK(spa3d_set_counts(h, B, s[0], s[1]) == SPA3D_OK);
            const long long wr = train_need();
            CHECK(wr > 0 && wr <= w3);
          }
          CHECK(spa3d_set_option(h, "chunk", 1) == SPA3D_OK);
          const long long wr1 = train_need();
          CHECK(wr1 > 0 && wr1 <= w[k]);
          CHECK(spa3d_set_counts(h, 0, nullptr, nullptr) == SPA3D_OK);
        }
        CHECK(spa3d_set_option(h, "chunk", 0) == SPA3D_OK);
        // intra-sample chunks: pass A keeps no encoder stash already, pass B is dropped -- never more than the unfrozen call
        CHECK(spa3d_set_option(h, "freeze", 0) == SPA3D_OK && spa3d_set_option(h, "track_chunk", 128) == SPA3D_OK && spa3d_set_option(h, "query_chunk", 32) == SPA3D_OK);
        const long long c0 = train_need();
        CHECK(spa3d_set_option(h, "freeze", k) == SPA3D_OK);
        const long long ck = train_need();
        CHECK(c0 > 0 && ck > 0 && ck <= c0);
        CHECK(spa3d_set_option(h, "track_chunk", 0) == SPA3D_OK && spa3d_set_option(h, "query_chunk", 0) == SPA3D_OK);
      }
      // back at 0 the call sizes as it did before the option was ever set
      CHECK(spa3d_set_option(h, "freeze", 0) == SPA3D_OK && train_need() == w[0]);
      CHECK(spa3d_destroy(h) == SPA3D_OK);
    }
  int64_t r[2];
  CHECK(spa3d_trainable_range(nullptr, r) == SPA3D_ERR_ARG);
  puts("HOST_FREEZE_OK");
  return 0;
}
