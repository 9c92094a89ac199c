// Host-side walk of spa3d_score / spa3d_score_from_preds under AddressSanitizer + UndefinedBehaviorSanitizer, built like spa3d_host_ragged.cpp
// (tests/test_host_sanitizers.py).  No GPU is touched: spa3d_score validates its arguments and sizes its workspace with a dry run of the
// orchestration BEFORE its first launch, so a call with a zero-byte workspace walks the whole score orchestration -- the BASELINE shapes, a
// ragged batch with a sample without queries, query chunks, the 2-D twin -- and returns SPA3D_ERR_WORKSPACE with the bytes it needs.
// Checked here: that need never exceeds spa3d_workspace_bytes(train = 0), and every refusal returns SPA3D_ERR_ARG with a message.
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

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

static long long need_of(spa3d_handle h) {  // "workspace too small: need N bytes for chunk 1"
  const char* m = spa3d_last_error(h);
  const char* p = strstr(m, "need ");
  return p ? atoll(p + 5) : -1;
}

static float* const fake = (float*)(uintptr_t)0x100000;  // never dereferenced: every call below returns before its first launch

static spa3d_batch batch_of(int B, int N, int Q, int T, bool features) {
  spa3d_batch b; memset(&b, 0, sizeof b);
  b.B = B; b.N = N; b.Q = Q; b.T = T; b.discretize = 1;
  b.support_tracks = fake; b.support_tracks_visible = fake; b.query_points = fake; b.boundary_frame = (const int32_t*)fake; b.noise = fake;
  if (features) { b.dino_features = fake; b.depth_features = fake; }
  b.query_tracks = fake; b.query_tracks_visible = fake;
  return b;
}
static spa3d_scores scores_of(int K) {
  spa3d_scores s; memset(&s, 0, sizeof s);
  s.num_thresholds = K;
  for (int i = 0; i < K && i < 8; ++i) s.thresholds[i] = 0.01f * (float)(i + 1);
  s.sample_scale = fake; s.query_stats = fake; s.sample_stats = (double*)fake; s.frame_err = fake;
  return s;
}

int main() {
  spa3d_outputs out; out.tracks = fake; out.visible_logits = fake; out.certain_logits = fake; out.latents = nullptr;
  struct Shape { const char* name; int B, N, Q, T, dino, depth, prec, kind; };
  const Shape shapes[] = {
      {"cfg#1 B=2 64+16 T=24 xyz fp32", 2, 64, 16, 24, 0, 0, SPA3D_F32, 0},
      {"cfg#2 B=64 2048+512 T=150 C=4 bf16", 64, 2048, 512, 150, 0, 1, SPA3D_BF16, 0},
      {"cfg#3 B=64 2048+512 T=150 C=772 bf16", 64, 2048, 512, 150, 768, 1, SPA3D_BF16, 0},
      {"cfg#5 B=8 8192+2048 T=300 C=772 fp16", 8, 8192, 2048, 300, 768, 1, SPA3D_F16, 0},
      {"2-D TRAJAN twin", 4, 256, 64, 150, 0, 0, SPA3D_BF16, 1},
  };
  for (const Shape& s : shapes) {
    spa3d_config c = base(s.T, s.dino, s.depth, s.prec, s.kind);
    spa3d_handle h = nullptr;
    CHECK(spa3d_create(&c, &h) == SPA3D_OK && h);
    spa3d_batch b = batch_of(s.B, s.N, s.Q, s.T, s.dino > 0);
    if (s.dino == 0 && s.depth > 0) b.depth_features = fake;
    const long long bound = spa3d_workspace_bytes(h, s.B, s.N, s.Q, s.T, 1, 0);
    CHECK(bound > 0);
    for (int K : {0, 5, 8}) {
      spa3d_scores sc = scores_of(K);
      CHECK(spa3d_score(h, fake, &b, &sc, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE);
      const long long need = need_of(h);
      CHECK(need > 0 && need <= bound);
      CHECK(spa3d_score(h, fake, &b, &sc, nullptr, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) == need);  // out = NULL: the same walk
      CHECK(spa3d_forward(h, fake, &b, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) == need);       // and the forward's workspace exactly
    }
    {  // query chunks: one sample per chunk, the readout released chunk by chunk
      spa3d_scores sc = scores_of(5);
      CHECK(spa3d_set_option(h, "query_chunk", s.Q / 4) == SPA3D_OK);
      CHECK(spa3d_score(h, fake, &b, &sc, nullptr, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE);
      CHECK(need_of(h) > 0 && need_of(h) <= spa3d_workspace_bytes(h, s.B, s.N, s.Q, s.T, 1, 0) && need_of(h) <= bound);
      CHECK(spa3d_set_option(h, "chunk", 2) == SPA3D_ERR_ARG);  // refused with intra-sample chunks, as everywhere
      CHECK(spa3d_set_option(h, "query_chunk", 0) == SPA3D_OK && spa3d_set_option(h, "track_chunk", s.N / 2) == SPA3D_OK);
      CHECK(spa3d_score(h, fake, &b, &sc, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) > 0 && need_of(h) <= bound);
      CHECK(spa3d_set_option(h, "track_chunk", 0) == SPA3D_OK);
    }
    printf("%-44s spa3d_score walks; forward-only workspace bound %.3f GB\n", s.name, bound / 1e9);
    // refusals: SPA3D_ERR_ARG with a message, before anything else happens
    {
      spa3d_scores sc = scores_of(5);
      spa3d_batch nb = b; nb.query_tracks = nullptr;
      CHECK(spa3d_score(h, fake, &nb, &sc, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "targets"));
      CHECK(spa3d_score_from_preds(h, &nb, &out, &sc, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "targets"));
      nb = b; nb.query_tracks_visible = nullptr;
      CHECK(spa3d_score(h, fake, &nb, &sc, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "targets"));
      spa3d_scores bad = sc; bad.query_stats = nullptr;
      CHECK(spa3d_score(h, fake, &b, &bad, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "query_stats"));
      CHECK(spa3d_score_from_preds(h, &b, &out, &bad, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "query_stats"));
      CHECK(spa3d_score(h, fake, &b, nullptr, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && strlen(spa3d_last_error(h)) > 0);
      for (int K : {-1, 9, 1 << 20}) {
        bad = sc; bad.num_thresholds = K;
        CHECK(spa3d_score(h, fake, &b, &bad, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "num_thresholds"));
        CHECK(spa3d_score_from_preds(h, &b, &out, &bad, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "num_thresholds"));
      }
      const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
      for (float v : {0.f, -1.f, inf, -inf, nan}) {
        bad = sc; bad.thresholds[3] = v;
        CHECK(spa3d_score(h, fake, &b, &bad, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "thresholds[3]"));
        CHECK(spa3d_score_from_preds(h, &b, &out, &bad, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "thresholds[3]"));
      }
      bad = sc; bad.num_thresholds = 3; bad.thresholds[3] = nan;  // beyond num_thresholds: not looked at
      CHECK(spa3d_score(h, fake, &b, &bad, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE);
      spa3d_outputs np = out; np.tracks = nullptr;
      CHECK(spa3d_score_from_preds(h, &b, &np, &sc, nullptr) == SPA3D_ERR_ARG && strlen(spa3d_last_error(h)) > 0);
      CHECK(spa3d_score_from_preds(h, &b, nullptr, &sc, nullptr) == SPA3D_ERR_ARG);
      CHECK(spa3d_score(nullptr, fake, &b, &sc, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && spa3d_score(h, nullptr, &b, &sc, &out, fake, 0, nullptr) == SPA3D_ERR_ARG);
    }
    if (s.kind == 1) {  // the 2-D twin refuses counts here as in every entry point
      const int32_t n[4] = {256, 10, 256, 256}, q[4] = {64, 4, 0, 64};
      spa3d_scores sc = scores_of(5);
      CHECK(spa3d_set_counts(h, s.B, n, q) == SPA3D_OK);
      CHECK(spa3d_score(h, fake, &b, &sc, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && strlen(spa3d_last_error(h)) > 0);
    }
    CHECK(spa3d_destroy(h) == SPA3D_OK);
  }
  {  // a ragged batch: a sample without queries, a sample with one; single-sample chunks and a packed chunk of three
    const int B = 4, N = 512, Q = 128, T = 150;
    for (int prec : {SPA3D_BF16, SPA3D_F32}) {
      spa3d_config c = base(T, 768, 1, prec, 0);
      spa3d_handle h = nullptr;
      CHECK(spa3d_create(&c, &h) == SPA3D_OK && h);
      spa3d_batch b = batch_of(B, N, Q, T, true);
      spa3d_scores sc = scores_of(5);
      const long long bound = spa3d_workspace_bytes(h, B, N, Q, T, 1, 0);
      const int32_t n[4] = {512, 100, 64, 300}, q[4] = {128, 0, 1, 50};
      CHECK(spa3d_set_counts(h, B, n, q) == SPA3D_OK);
      CHECK(spa3d_score(h, fake, &b, &sc, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) > 0 && need_of(h) <= bound);
      CHECK(spa3d_score(h, fake, &b, &sc, nullptr, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) <= bound);
      CHECK(spa3d_set_option(h, "chunk", 3) == SPA3D_OK);
      CHECK(spa3d_score(h, fake, &b, &sc, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) > 0 && need_of(h) <= spa3d_workspace_bytes(h, B, N, Q, T, 3, 0));
      CHECK(spa3d_set_option(h, "chunk", 0) == SPA3D_OK);
      // inherited refusals: counts with intra-sample chunks, counts that do not fit the batch
      CHECK(spa3d_set_option(h, "query_chunk", 32) == SPA3D_OK);
      CHECK(spa3d_score(h, fake, &b, &sc, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "chunk"));
      CHECK(spa3d_set_option(h, "query_chunk", 0) == SPA3D_OK);
      const int32_t qbig[4] = {128, 129, 1, 50};
      CHECK(spa3d_set_counts(h, B, n, qbig) == SPA3D_OK);
      CHECK(spa3d_score(h, fake, &b, &sc, &out, fake, 0, nullptr) == SPA3D_ERR_ARG && strlen(spa3d_last_error(h)) > 0);
      CHECK(spa3d_score_from_preds(h, &b, &out, &sc, nullptr) == SPA3D_ERR_ARG && strlen(spa3d_last_error(h)) > 0);
      CHECK(spa3d_set_counts(h, B - 1, n, q) == SPA3D_OK);
      CHECK(spa3d_score_from_preds(h, &b, &out, &sc, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "counts"));
      CHECK(spa3d_set_counts(h, 0, nullptr, nullptr) == SPA3D_OK);
      CHECK(spa3d_score(h, fake, &b, &sc, &out, fake, 0, nullptr) == SPA3D_ERR_WORKSPACE && need_of(h) <= bound);
      CHECK(spa3d_destroy(h) == SPA3D_OK);
    }
  }
  puts("HOST_SCORE_OK");
  return 0;
}
