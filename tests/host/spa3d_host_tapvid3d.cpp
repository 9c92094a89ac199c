// Host-side walk of spa3d_tapvid3d_from_preds under AddressSanitizer + UndefinedBehaviorSanitizer, built like spa3d_host_score.cpp
// (tests/test_host_sanitizers.py).  No GPU is touched: the entry validates its arguments and sizes its workspace with a dry run of its
// orchestration BEFORE its first launch, so a call with a zero-byte workspace walks every launch site -- the BASELINE shapes, the three
// scalings, with and without the optional outputs, a ragged batch with a query-less sample -- and returns SPA3D_ERR_ARG with the bytes it
// needs.  Checked here: that need never exceeds spa3d_tapvid3d_workspace_bytes, and every refusal returns SPA3D_ERR_ARG with a message.
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

static long long need_of(spa3d_handle h) {  // "tapvid3d: workspace too small: need N bytes"
  const char* m = spa3d_last_error(h);
  const char* p = strstr(m, "need ");
  return p ? atoll(p + 5) : -1;
}

static float* const fake = (float*)(uintptr_t)0x100000;  // never dereferenced: every call below returns before its first launch

static spa3d_batch batch_of(int B, int Q) {
  spa3d_batch b; memset(&b, 0, sizeof b);
  b.B = B; b.Q = Q;  // the entry reads B, Q, query_points and the targets only
  b.query_points = fake; b.query_tracks = fake; b.query_tracks_visible = fake;
  return b;
}
static spa3d_tapvid3d metric_of(int scaling, bool all_outputs) {
  spa3d_tapvid3d m; memset(&m, 0, sizeof m);
  m.scaling = scaling; m.query_stats = fake;
  if (all_outputs) { m.intrinsics = fake; m.sample_stats = (double*)fake; m.scale = fake; m.row_scale = fake; m.ratio = fake; }
  return m;
}

int main() {
  spa3d_outputs out; out.tracks = fake; out.visible_logits = fake; out.certain_logits = nullptr; out.latents = nullptr;
  struct Shape { const char* name; int B, Q, T, prec; };
  const Shape shapes[] = {
      {"cfg#1 B=2 Q=16 T=24 fp32", 2, 16, 24, SPA3D_F32},
      {"cfg#2/#3 B=64 Q=512 T=150 bf16", 64, 512, 150, SPA3D_BF16},
      {"headline width B=1 Q=512 T=150 bf16", 1, 512, 150, SPA3D_BF16},
      {"cfg#5 B=8 Q=2048 T=300 fp16", 8, 2048, 300, SPA3D_F16},
  };
  for (const Shape& s : shapes) {
    spa3d_config c = base(s.T, 768, 1, s.prec, 0);
    spa3d_handle h = nullptr;
    CHECK(spa3d_create(&c, &h) == SPA3D_OK && h);
    spa3d_batch b = batch_of(s.B, s.Q);
    const long long bound = spa3d_tapvid3d_workspace_bytes(h, s.B, s.Q, s.T);
    CHECK(bound > 0);
    long long most = 0;
    for (int scaling : {SPA3D_SCALE_NONE, SPA3D_SCALE_MEDIAN, SPA3D_SCALE_PER_TRAJECTORY})
      for (bool all : {false, true})
        for (int fixed : {0, 1}) {
          spa3d_tapvid3d m = metric_of(scaling, all); m.fixed_thresholds = fixed;
          CHECK(spa3d_tapvid3d_from_preds(h, &b, &out, &m, fake, 0, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "workspace too small"));
          const long long need = need_of(h);
          CHECK(need > 0 && need <= bound);
          CHECK(spa3d_tapvid3d_from_preds(h, &b, &out, &m, nullptr, bound, nullptr) == SPA3D_ERR_ARG);          // no workspace at all
          CHECK(spa3d_tapvid3d_from_preds(h, &b, &out, &m, fake, need - 1, nullptr) == SPA3D_ERR_ARG && need_of(h) == need);
          if (scaling == SPA3D_SCALE_MEDIAN) CHECK(need >= (long long)s.B * s.Q * s.T * 4);                       // the median's set
          if (need > most) most = need;
        }
    CHECK(spa3d_tapvid3d_workspace_bytes(h, 0, s.Q, s.T) == -1 && spa3d_tapvid3d_workspace_bytes(h, s.B, 0, s.T) == -1 &&
          spa3d_tapvid3d_workspace_bytes(h, s.B, s.Q, 0) == -1 && spa3d_tapvid3d_workspace_bytes(nullptr, s.B, s.Q, s.T) == -1);
    printf("%-40s spa3d_tapvid3d_from_preds walks; needs at most %lld of the %lld bytes spa3d_tapvid3d_workspace_bytes gives\n", s.name, most, bound);
    // refusals: SPA3D_ERR_ARG with a message, before anything else happens
    {
      spa3d_tapvid3d m = metric_of(SPA3D_SCALE_MEDIAN, true);
      spa3d_batch nb = b; nb.query_tracks = nullptr;
      CHECK(spa3d_tapvid3d_from_preds(h, &nb, &out, &m, fake, bound, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "targets"));
      nb = b; nb.query_tracks_visible = nullptr;
      CHECK(spa3d_tapvid3d_from_preds(h, &nb, &out, &m, fake, bound, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "targets"));
      nb = b; nb.query_points = nullptr;
      CHECK(spa3d_tapvid3d_from_preds(h, &nb, &out, &m, fake, bound, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "query_points"));
      CHECK(spa3d_tapvid3d_from_preds(h, nullptr, &out, &m, fake, bound, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "targets"));
      spa3d_outputs np = out; np.tracks = nullptr;
      CHECK(spa3d_tapvid3d_from_preds(h, &b, &np, &m, fake, bound, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "predictions"));
      np = out; np.visible_logits = nullptr;
      CHECK(spa3d_tapvid3d_from_preds(h, &b, &np, &m, fake, bound, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "predictions"));
      CHECK(spa3d_tapvid3d_from_preds(h, &b, nullptr, &m, fake, bound, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "predictions"));
      spa3d_tapvid3d bad = m; bad.query_stats = nullptr;
      CHECK(spa3d_tapvid3d_from_preds(h, &b, &out, &bad, fake, bound, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "query_stats"));
      CHECK(spa3d_tapvid3d_from_preds(h, &b, &out, nullptr, fake, bound, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "query_stats"));
      for (int sc : {-1, 3, 1 << 20}) {
        bad = m; bad.scaling = sc;
        CHECK(spa3d_tapvid3d_from_preds(h, &b, &out, &bad, fake, bound, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "scaling"));
      }
      nb = b; nb.Q = 0;
      CHECK(spa3d_tapvid3d_from_preds(h, &nb, &out, &m, fake, bound, nullptr) == SPA3D_ERR_ARG && strlen(spa3d_last_error(h)) > 0);
      CHECK(spa3d_tapvid3d_from_preds(nullptr, &b, &out, &m, fake, bound, nullptr) == SPA3D_ERR_ARG);
    }
    CHECK(spa3d_destroy(h) == SPA3D_OK);
  }
  {  // a ragged batch: a sample without queries, a sample with one
    const int B = 4, Q = 128, T = 150;
    spa3d_config c = base(T, 768, 1, SPA3D_BF16, 0);
    spa3d_handle h = nullptr;
    CHECK(spa3d_create(&c, &h) == SPA3D_OK && h);
    spa3d_batch b = batch_of(B, Q);
    const long long bound = spa3d_tapvid3d_workspace_bytes(h, B, Q, T);
    const int32_t n[4] = {512, 100, 64, 300}, q[4] = {128, 0, 1, 50};
    CHECK(spa3d_set_counts(h, B, n, q) == SPA3D_OK);
    for (int scaling : {SPA3D_SCALE_NONE, SPA3D_SCALE_MEDIAN, SPA3D_SCALE_PER_TRAJECTORY})
      for (bool all : {false, true}) {
        spa3d_tapvid3d m = metric_of(scaling, all);
        CHECK(spa3d_tapvid3d_from_preds(h, &b, &out, &m, fake, 0, nullptr) == SPA3D_ERR_ARG && need_of(h) > 0 && need_of(h) <= bound);
      }
    spa3d_tapvid3d m = metric_of(SPA3D_SCALE_MEDIAN, true);
    const int32_t qbig[4] = {128, 129, 1, 50};
    CHECK(spa3d_set_counts(h, B, n, qbig) == SPA3D_OK);
    CHECK(spa3d_tapvid3d_from_preds(h, &b, &out, &m, fake, bound, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "query_count"));
    CHECK(spa3d_set_counts(h, B - 1, n, q) == SPA3D_OK);
    CHECK(spa3d_tapvid3d_from_preds(h, &b, &out, &m, fake, bound, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "counts"));
    CHECK(spa3d_set_counts(h, 0, nullptr, nullptr) == SPA3D_OK);
    CHECK(spa3d_tapvid3d_from_preds(h, &b, &out, &m, fake, 0, nullptr) == SPA3D_ERR_ARG && need_of(h) > 0 && need_of(h) <= bound);
    CHECK(spa3d_destroy(h) == SPA3D_OK);
    puts("ragged batch with a query-less sample walks");
  }
  {  // the 2-D twin has no depth coordinate
    spa3d_config c = base(150, 0, 0, SPA3D_BF16, 1);
    spa3d_handle h = nullptr;
    CHECK(spa3d_create(&c, &h) == SPA3D_OK && h);
    spa3d_batch b = batch_of(4, 64);
    spa3d_tapvid3d m = metric_of(SPA3D_SCALE_MEDIAN, true);
    CHECK(spa3d_tapvid3d_from_preds(h, &b, &out, &m, fake, 1 << 24, nullptr) == SPA3D_ERR_ARG && strstr(spa3d_last_error(h), "model_kind 1"));
    CHECK(spa3d_destroy(h) == SPA3D_OK);
  }
  puts("HOST_TAPVID3D_OK");
  return 0;
}
