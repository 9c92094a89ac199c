// Host-side walk of the refusals of spa3d_motion_knn, spa3d_motion_ball_hits and spa3d_motion_knn_workspace_bytes under AddressSanitizer +
// UndefinedBehaviorSanitizer, built like motion_host_walk.cpp (tests/test_motion_knn_host_sanitizers.py).  No GPU is touched: the entries check
// everything before their first launch or store, so each call below returns SPA3D_ERR_ARG with a message and launches nothing.  The device
// pointers are fakes that are never dereferenced; a call that got past the checks would try to launch and come back with another status, which
// fails the CHECK.
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

static int16_t* const cfake = (int16_t*)(uintptr_t)0x200000;     // never dereferenced: every call below returns before its first launch
static int32_t* const ifake = (int32_t*)(uintptr_t)0x300000;
static int32_t* const jfake = (int32_t*)(uintptr_t)0x380000;
static void* const wfake = (void*)(uintptr_t)0x400000;

static bool said(spa3d_handle h, int rc, const char* entry, const char* word) {
  const char* m = spa3d_last_error(h);
  if (rc != SPA3D_ERR_ARG || !strstr(m, entry) || !strstr(m, word)) { fprintf(stderr, "rc = %d, message '%s', wanted '%s: ... %s'\n", rc, m, entry, word); return false; }
  return true;
}
struct Knn {   // an accepted call's arguments; each refusal changes one
  const int16_t* a = cfake; int64_t Ma = 130; const int16_t* b = cfake; int64_t Mb = 700; int32_t E = 12288, k = 8; int64_t so = 0; int32_t splits = 7;
  int32_t* dist = ifake; int32_t* idx = jfake; void* ws = wfake; int64_t wsb = 7 * 130 * 8 * 8;
};
static bool refused_knn(spa3d_handle h, const Knn& q, const char* word) {
  return said(h, spa3d_motion_knn(h, q.a, q.Ma, q.b, q.Mb, q.E, q.k, q.so, q.splits, q.dist, q.idx, q.ws, q.wsb, nullptr), "motion_knn", word);
}
struct Ball {
  const int16_t* a = cfake; int64_t Ma = 130; const int16_t* b = cfake; int64_t Mb = 700; int32_t E = 12288; const int32_t* radius = ifake; int64_t so = -1;
  int32_t* rows = jfake; int32_t* cols = jfake;
};
static bool refused_ball(spa3d_handle h, const Ball& q, const char* word) {
  return said(h, spa3d_motion_ball_hits(h, q.a, q.Ma, q.b, q.Mb, q.E, q.radius, q.so, q.rows, q.cols, nullptr), "motion_ball_hits", word);
}

int main() {
  spa3d_config cfg = base();
  spa3d_handle h = nullptr;
  CHECK(spa3d_create(&cfg, &h) == SPA3D_OK && h);
  const int64_t M22 = (int64_t)1 << 22;
  // spa3d_motion_knn_workspace_bytes
  CHECK(spa3d_motion_knn_workspace_bytes(130, 700, 8, 1) == 0);
  CHECK(spa3d_motion_knn_workspace_bytes(130, 700, 8, 0) == 0);
  CHECK(spa3d_motion_knn_workspace_bytes(130, 700, 8, 7) == 7 * 130 * 8 * 8);
  CHECK(spa3d_motion_knn_workspace_bytes(64, 262144, 5, 0) == (int64_t)512 * 64 * 5 * 8);
  CHECK(spa3d_motion_knn_workspace_bytes(M22, M22, 64, 4096) == (int64_t)4096 * M22 * 64 * 8);
  CHECK(spa3d_motion_knn_workspace_bytes(0, 700, 8, 1) == -1 && spa3d_motion_knn_workspace_bytes(INT64_MIN, 700, 8, 1) == -1 && spa3d_motion_knn_workspace_bytes(M22 + 1, 700, 8, 1) == -1);
  CHECK(spa3d_motion_knn_workspace_bytes(130, 0, 8, 1) == -1 && spa3d_motion_knn_workspace_bytes(130, INT64_MAX, 8, 1) == -1);
  CHECK(spa3d_motion_knn_workspace_bytes(130, 700, 0, 1) == -1 && spa3d_motion_knn_workspace_bytes(130, 700, 65, 1) == -1 && spa3d_motion_knn_workspace_bytes(130, 700, INT32_MIN, 1) == -1);
  CHECK(spa3d_motion_knn_workspace_bytes(130, 700, 8, -1) == -1 && spa3d_motion_knn_workspace_bytes(130, 700, 8, 4097) == -1 && spa3d_motion_knn_workspace_bytes(130, 700, 8, INT32_MAX) == -1);
  // spa3d_motion_knn
  { Knn q; q.a = nullptr; CHECK(refused_knn(h, q, "a is required")); }
  { Knn q; q.b = nullptr; CHECK(refused_knn(h, q, "b is required")); }
  { Knn q; q.dist = nullptr; CHECK(refused_knn(h, q, "dist is required")); }
  { Knn q; q.idx = nullptr; CHECK(refused_knn(h, q, "idx is required")); }
  { Knn q; q.Ma = 0; CHECK(refused_knn(h, q, "Ma = 0")); }
  { Knn q; q.Ma = -1; CHECK(refused_knn(h, q, "Ma = -1")); }
  { Knn q; q.Ma = M22 + 1; CHECK(refused_knn(h, q, "Ma = 4194305")); }
  { Knn q; q.Ma = INT64_MAX; CHECK(refused_knn(h, q, "Ma = ")); }
  { Knn q; q.Mb = 0; CHECK(refused_knn(h, q, "Mb = 0")); }
  { Knn q; q.Mb = INT64_MIN; CHECK(refused_knn(h, q, "Mb = -")); }
  { Knn q; q.Mb = M22 + 1; CHECK(refused_knn(h, q, "Mb = 4194305")); }
  { Knn q; q.E = 0; CHECK(refused_knn(h, q, "E = 0")); }
  { Knn q; q.E = -8; CHECK(refused_knn(h, q, "E = -8")); }
  { Knn q; q.E = 32768; CHECK(refused_knn(h, q, "E = 32768")); }
  { Knn q; q.E = INT32_MAX; CHECK(refused_knn(h, q, "E = 2147483647")); }
  { Knn q; q.so = -2; CHECK(refused_knn(h, q, "self_offset = -2")); }
  { Knn q; q.so = INT64_MIN; CHECK(refused_knn(h, q, "self_offset = -")); }
  { Knn q; q.k = 0; CHECK(refused_knn(h, q, "k = 0")); }
  { Knn q; q.k = -3; CHECK(refused_knn(h, q, "k = -3")); }
  { Knn q; q.k = 65; CHECK(refused_knn(h, q, "k = 65")); }
  { Knn q; q.k = INT32_MAX; CHECK(refused_knn(h, q, "k = 2147483647")); }
  { Knn q; q.Mb = 8; CHECK(refused_knn(h, q, "the 7 columns")); }                       // Mb = k with the own column left out
  { Knn q; q.Mb = 8; q.Ma = 3; q.so = 7; CHECK(refused_knn(h, q, "the 7 columns")); }   // row 0's own column is the last one
  { Knn q; q.Mb = 7; q.so = -1; CHECK(refused_knn(h, q, "the 7 columns")); }
  { Knn q; q.Mb = 1; q.k = 1; CHECK(refused_knn(h, q, "the 0 columns")); }
  { Knn q; q.splits = -1; CHECK(refused_knn(h, q, "splits = -1")); }
  { Knn q; q.splits = 4097; CHECK(refused_knn(h, q, "splits = 4097")); }
  { Knn q; q.splits = INT32_MIN; CHECK(refused_knn(h, q, "splits = -2147483648")); }
  { Knn q; q.ws = nullptr; CHECK(refused_knn(h, q, "workspace is required")); }
  { Knn q; q.wsb -= 1; CHECK(refused_knn(h, q, "58240 needed")); }
  { Knn q; q.wsb = 0; CHECK(refused_knn(h, q, "workspace of 0 bytes")); }
  { Knn q; q.wsb = -1; CHECK(refused_knn(h, q, "workspace of -1 bytes")); }
  { Knn q; q.wsb = INT64_MIN; CHECK(refused_knn(h, q, "needed")); }
  { Knn q; q.ws = (void*)(uintptr_t)0x400004; CHECK(refused_knn(h, q, "8-byte aligned")); }
  { Knn q; q.Ma = 64; q.Mb = 262144; q.k = 5; q.so = -1; q.splits = 0; q.wsb = (int64_t)512 * 64 * 5 * 8 - 8; CHECK(refused_knn(h, q, "needed")); }   // the plan's 512 ranges
  { Knn q; CHECK(spa3d_motion_knn(nullptr, q.a, q.Ma, q.b, q.Mb, q.E, q.k, q.so, q.splits, q.dist, q.idx, q.ws, q.wsb, nullptr) == SPA3D_ERR_ARG); }
  // spa3d_motion_ball_hits
  { Ball q; q.a = nullptr; CHECK(refused_ball(h, q, "a is required")); }
  { Ball q; q.b = nullptr; CHECK(refused_ball(h, q, "b is required")); }
  { Ball q; q.radius = nullptr; CHECK(refused_ball(h, q, "radius is required")); }
  { Ball q; q.rows = nullptr; q.cols = nullptr; CHECK(refused_ball(h, q, "one of row_hits and col_hits")); }
  { Ball q; q.Ma = 0; CHECK(refused_ball(h, q, "Ma = 0")); }
  { Ball q; q.Ma = M22 + 1; CHECK(refused_ball(h, q, "Ma = 4194305")); }
  { Ball q; q.Ma = INT64_MIN; CHECK(refused_ball(h, q, "Ma = -")); }
  { Ball q; q.Mb = 0; CHECK(refused_ball(h, q, "Mb = 0")); }
  { Ball q; q.Mb = -5; CHECK(refused_ball(h, q, "Mb = -5")); }
  { Ball q; q.Mb = INT64_MAX; CHECK(refused_ball(h, q, "Mb = 9223372036854775807")); }
  { Ball q; q.E = 0; CHECK(refused_ball(h, q, "E = 0")); }
  { Ball q; q.E = 32768; CHECK(refused_ball(h, q, "E = 32768")); }
  { Ball q; q.E = INT32_MIN; CHECK(refused_ball(h, q, "E = -2147483648")); }
  { Ball q; q.so = -2; CHECK(refused_ball(h, q, "self_offset = -2")); }
  { Ball q; q.so = INT64_MIN; CHECK(refused_ball(h, q, "self_offset = -9223372036854775808")); }
  { Ball q; CHECK(spa3d_motion_ball_hits(nullptr, q.a, q.Ma, q.b, q.Mb, q.E, q.radius, q.so, q.rows, q.cols, nullptr) == SPA3D_ERR_ARG); }
  // a refusal leaves a message of its own: the last one read back names the last call
  CHECK(strstr(spa3d_last_error(h), "motion_ball_hits: self_offset"));
  CHECK(spa3d_destroy(h) == SPA3D_OK);
  puts("HOST_MOTION_KNN_OK");
  return 0;
}
