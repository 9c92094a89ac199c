// Host-side walk of the refusals of spa3d_motion_codes, spa3d_motion_moments_add and spa3d_motion_pdist under AddressSanitizer +
// UndefinedBehaviorSanitizer, built like windows_host_walk.cpp (tests/test_motion_host_sanitizers.py).  No GPU is touched: the three entries check
// everything before their first launch, so each call below returns SPA3D_ERR_ARG with a message and launches nothing.  The device pointers are
// fakes that are never dereferenced; a call that got past the checks would try to launch and come back with another status, which fails the CHECK.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "spa3d.h"

static spa3d_config base() {
  spa3d_config c;
  memset(&c, 0, sizeof c);
  c.num_output_frames = 8; c.num_latent_tokens = 128; c.latent_token_dim = 96; c.num_frequencies = 32; c.track_scale_factor = 1.f;
  c.time_scale_factor = 150.f; c.track_token_dim = 384; c.encoder_latent_dim = 512; c.decoder_num_channels = 1280;
  c.dino_feature_dim = 0; c.depth_feature_dim = 0; c.num_heads = 8; c.qkv_size = 768; c.enc_mlp = 1536;
  c.enc_layers = 3; c.t2l_mlp = 2048; c.t2l_layers = 4; c.dec_mlp = 2048; c.dec_layers = 4;
  c.ro_mlp = 1536; c.ro_layers = 4; c.precision = SPA3D_F32; c.model_kind = 0;
  return c;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed: %s (line %d): %s\n", #x, __LINE__, h ? spa3d_last_error(h) : ""); return 1; } } while (0)

static float* const ffake = (float*)(uintptr_t)0x100000;        // never dereferenced: every call below returns before its first launch
static int16_t* const cfake = (int16_t*)(uintptr_t)0x200000;
static int32_t* const ifake = (int32_t*)(uintptr_t)0x300000;
static int64_t* const sfake = (int64_t*)(uintptr_t)0x400000;

static bool said(spa3d_handle h, int rc, const char* entry, const char* word) {
  const char* m = spa3d_last_error(h);
  if (rc != SPA3D_ERR_ARG || !strstr(m, entry) || !strstr(m, word)) { fprintf(stderr, "rc = %d, message '%s', wanted '%s: ... %s'\n", rc, m, entry, word); return false; }
  return true;
}
static bool refused_codes(spa3d_handle h, const float* lat, int64_t n, int16_t* codes, int32_t* bad, const char* word) {
  return said(h, spa3d_motion_codes(h, lat, n, codes, bad, nullptr), "motion_codes", word);
}
static bool refused_moments(spa3d_handle h, const int16_t* codes, int64_t M, int32_t L, int32_t D, int32_t pool, int64_t* state, const char* word) {
  return said(h, spa3d_motion_moments_add(h, codes, M, L, D, pool, state, nullptr), "motion_moments_add", word);
}
static bool refused_pdist(spa3d_handle h, const int16_t* a, int64_t Ma, const int16_t* b, int64_t Mb, int32_t E, int32_t kind, int32_t* out, const char* word) {
  return said(h, spa3d_motion_pdist(h, a, Ma, b, Mb, E, kind, out, nullptr), "motion_pdist", word);
}

int main() {
  spa3d_config cfg = base();
  spa3d_handle h = nullptr;
  CHECK(spa3d_create(&cfg, &h) == SPA3D_OK && h);
  // spa3d_motion_codes
  CHECK(refused_codes(h, nullptr, 12288, cfake, ifake, "latents is required"));
  CHECK(refused_codes(h, ffake, 12288, nullptr, ifake, "codes is required"));
  CHECK(refused_codes(h, ffake, 12288, cfake, nullptr, "bad is required"));
  CHECK(refused_codes(h, ffake, -1, cfake, ifake, "n = -1"));
  CHECK(refused_codes(h, ffake, INT64_MIN, cfake, ifake, "negative"));
  CHECK(spa3d_motion_codes(nullptr, ffake, 4, cfake, ifake, nullptr) == SPA3D_ERR_ARG);
  // spa3d_motion_moments_add
  for (int pool : {SPA3D_POOL_TOKEN, SPA3D_POOL_CLIP}) {
    CHECK(refused_moments(h, nullptr, 70, 128, 96, pool, sfake, "codes is required"));
    CHECK(refused_moments(h, cfake, 70, 128, 96, pool, nullptr, "state is required"));
    CHECK(refused_moments(h, cfake, 0, 128, 96, pool, sfake, "M = 0"));
    CHECK(refused_moments(h, cfake, -3, 128, 96, pool, sfake, "M = -3"));
    CHECK(refused_moments(h, cfake, INT64_MAX, 128, 96, pool, sfake, "M = 9223372036854775807"));
    CHECK(refused_moments(h, cfake, ((int64_t)1 << 40) + 1, 128, 96, pool, sfake, "2^40"));
    CHECK(refused_moments(h, cfake, 70, 0, 96, pool, sfake, "L = 0"));
    CHECK(refused_moments(h, cfake, 70, 4097, 96, pool, sfake, "L = 4097"));
    CHECK(refused_moments(h, cfake, 70, -1, 96, pool, sfake, "L = -1"));
    CHECK(refused_moments(h, cfake, 70, INT32_MAX, 96, pool, sfake, "L = 2147483647"));
    CHECK(refused_moments(h, cfake, 70, 128, 0, pool, sfake, "D = 0"));
    CHECK(refused_moments(h, cfake, 70, 128, 257, pool, sfake, "D = 257"));
    CHECK(refused_moments(h, cfake, 70, 128, INT32_MIN, pool, sfake, "D = -2147483648"));
  }
  CHECK(refused_moments(h, cfake, 70, 128, 96, 2, sfake, "pool = 2"));
  CHECK(refused_moments(h, cfake, 70, 128, 96, -1, sfake, "pool = -1"));
  CHECK(spa3d_motion_moments_add(nullptr, cfake, 70, 128, 96, SPA3D_POOL_CLIP, sfake, nullptr) == SPA3D_ERR_ARG);
  // spa3d_motion_pdist
  for (int kind : {SPA3D_PDIST_DOT, SPA3D_PDIST_SQDIST}) {
    CHECK(refused_pdist(h, nullptr, 16, cfake, 17, 12288, kind, ifake, "a is required"));
    CHECK(refused_pdist(h, cfake, 16, nullptr, 17, 12288, kind, ifake, "b is required"));
    CHECK(refused_pdist(h, cfake, 16, cfake, 17, 12288, kind, nullptr, "out is required"));
    CHECK(refused_pdist(h, cfake, 0, cfake, 17, 12288, kind, ifake, "Ma = 0"));
    CHECK(refused_pdist(h, cfake, -1, cfake, 17, 12288, kind, ifake, "Ma = -1"));
    CHECK(refused_pdist(h, cfake, ((int64_t)1 << 22) + 1, cfake, 17, 12288, kind, ifake, "Ma = 4194305"));
    CHECK(refused_pdist(h, cfake, INT64_MAX, cfake, 17, 12288, kind, ifake, "Ma = "));
    CHECK(refused_pdist(h, cfake, 16, cfake, 0, 12288, kind, ifake, "Mb = 0"));
    CHECK(refused_pdist(h, cfake, 16, cfake, INT64_MIN, 12288, kind, ifake, "Mb = -"));
    CHECK(refused_pdist(h, cfake, 16, cfake, ((int64_t)1 << 22) + 1, 12288, kind, ifake, "Mb = 4194305"));
    CHECK(refused_pdist(h, cfake, 16, cfake, 17, 0, kind, ifake, "E = 0"));
    CHECK(refused_pdist(h, cfake, 16, cfake, 17, -8, kind, ifake, "E = -8"));
    CHECK(refused_pdist(h, cfake, 16, cfake, 17, 32768, kind, ifake, "E = 32768"));
    CHECK(refused_pdist(h, cfake, 16, cfake, 17, INT32_MAX, kind, ifake, "E = 2147483647"));
  }
  CHECK(refused_pdist(h, cfake, 16, cfake, 17, 12288, 2, ifake, "kind = 2"));
  CHECK(refused_pdist(h, cfake, 16, cfake, 17, 12288, -1, ifake, "kind = -1"));
  CHECK(spa3d_motion_pdist(nullptr, cfake, 16, cfake, 17, 12288, SPA3D_PDIST_DOT, ifake, nullptr) == SPA3D_ERR_ARG);
  // a refusal leaves a message of its own: the last one read back names the last call
  CHECK(strstr(spa3d_last_error(h), "motion_pdist: kind = -1"));
  CHECK(spa3d_destroy(h) == SPA3D_OK);
  puts("HOST_MOTION_OK");
  return 0;
}
