// Host-side walk of the refusals of spa3d_motion_kernel_sums under AddressSanitizer + UndefinedBehaviorSanitizer, built like
// motion_knn_host_walk.cpp (tests/test_motion_kernel_host_sanitizers.py).  No GPU is touched: the entry checks everything before its first store
// or launch, so each call below returns SPA3D_ERR_ARG with a message.  The device pointers are fakes that are never dereferenced; a call that got
// past the checks would try to zero its outputs and launch and come back with another status, which fails the CHECK.
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

static int16_t* const cfake = (int16_t*)(uintptr_t)0x200000;     // never dereferenced: every call below returns before its first store or launch
static uint64_t* const rfake = (uint64_t*)(uintptr_t)0x300000;
static uint64_t* const kfake = (uint64_t*)(uintptr_t)0x380000;

static bool said(spa3d_handle h, int rc, const char* word) {
  const char* m = spa3d_last_error(h);
  if (rc != SPA3D_ERR_ARG || !strstr(m, "motion_kernel_sums: ") || !strstr(m, word)) { fprintf(stderr, "rc = %d, message '%s', wanted 'motion_kernel_sums: ... %s'\n", rc, m, word); return false; }
  return true;
}
struct Sums {   // an accepted call's arguments; each refusal changes one
  const int16_t* a = cfake; int64_t Ma = 130; const int16_t* b = cfake; int64_t Mb = 700; int32_t E = 12288, degree = 3; int64_t so = 0;
  uint64_t* rows = rfake; uint64_t* cols = kfake;
};
static bool refused(spa3d_handle h, const Sums& q, const char* word) {
  return said(h, spa3d_motion_kernel_sums(h, q.a, q.Ma, q.b, q.Mb, q.E, q.degree, q.so, q.rows, q.cols, nullptr), word);
}

int main() {
  spa3d_config cfg = base();
  spa3d_handle h = nullptr;
  CHECK(spa3d_create(&cfg, &h) == SPA3D_OK && h);
  const int64_t M22 = (int64_t)1 << 22;
  { Sums q; q.a = nullptr; CHECK(refused(h, q, "a is required")); }
  { Sums q; q.b = nullptr; CHECK(refused(h, q, "b is required")); }
  { Sums q; q.rows = nullptr; q.cols = nullptr; CHECK(refused(h, q, "one of row_sums and col_sums")); }
  { Sums q; q.Ma = 0; CHECK(refused(h, q, "Ma = 0")); }
  { Sums q; q.Ma = -1; CHECK(refused(h, q, "Ma = -1")); }
  { Sums q; q.Ma = M22 + 1; CHECK(refused(h, q, "Ma = 4194305")); }
  { Sums q; q.Ma = INT64_MAX; CHECK(refused(h, q, "Ma = 9223372036854775807")); }
  { Sums q; q.Ma = INT64_MIN; CHECK(refused(h, q, "Ma = -")); }
  { Sums q; q.Mb = 0; CHECK(refused(h, q, "Mb = 0")); }
  { Sums q; q.Mb = -5; CHECK(refused(h, q, "Mb = -5")); }
  { Sums q; q.Mb = M22 + 1; CHECK(refused(h, q, "Mb = 4194305")); }
  { Sums q; q.Mb = INT64_MAX; CHECK(refused(h, q, "Mb = 9223372036854775807")); }
  { Sums q; q.E = 0; CHECK(refused(h, q, "E = 0")); }
  { Sums q; q.E = -8; CHECK(refused(h, q, "E = -8")); }
  { Sums q; q.E = 32768; CHECK(refused(h, q, "E = 32768")); }
  { Sums q; q.E = INT32_MAX; CHECK(refused(h, q, "E = 2147483647")); }
  { Sums q; q.E = INT32_MIN; CHECK(refused(h, q, "E = -2147483648")); }
  { Sums q; q.degree = 0; CHECK(refused(h, q, "degree = 0")); }
  { Sums q; q.degree = 4; CHECK(refused(h, q, "degree = 4")); }
  { Sums q; q.degree = -1; CHECK(refused(h, q, "degree = -1")); }
  { Sums q; q.degree = INT32_MAX; CHECK(refused(h, q, "degree = 2147483647")); }
  { Sums q; q.degree = INT32_MIN; CHECK(refused(h, q, "degree = -2147483648")); }
  { Sums q; q.so = -2; CHECK(refused(h, q, "self_offset = -2")); }
  { Sums q; q.so = INT64_MIN; CHECK(refused(h, q, "self_offset = -9223372036854775808")); }
  { Sums q; q.rows = (uint64_t*)(uintptr_t)0x300004; CHECK(refused(h, q, "row_sums is not 8-byte aligned")); }
  { Sums q; q.cols = (uint64_t*)(uintptr_t)0x380001; CHECK(refused(h, q, "col_sums is not 8-byte aligned")); }
  { Sums q; q.rows = nullptr; q.cols = (uint64_t*)(uintptr_t)0x380004; CHECK(refused(h, q, "col_sums is not 8-byte aligned")); }
  { Sums q; q.cols = nullptr; q.rows = (uint64_t*)(uintptr_t)0x300002; CHECK(refused(h, q, "row_sums is not 8-byte aligned")); }
  // what is said first: the pointers, then the sizes, the degree, the offset, the alignment
  { Sums q; q.Ma = 0; q.degree = 9; q.so = -7; q.rows = (uint64_t*)(uintptr_t)0x300004; CHECK(refused(h, q, "Ma = 0")); }
  { Sums q; q.degree = 9; q.so = -7; q.rows = (uint64_t*)(uintptr_t)0x300004; CHECK(refused(h, q, "degree = 9")); }
  { Sums q; q.so = -7; q.rows = (uint64_t*)(uintptr_t)0x300004; CHECK(refused(h, q, "self_offset = -7")); }
  { Sums q; CHECK(spa3d_motion_kernel_sums(nullptr, q.a, q.Ma, q.b, q.Mb, q.E, q.degree, q.so, q.rows, q.cols, nullptr) == SPA3D_ERR_ARG); }
  // a refusal leaves a message of its own: the last one read back names the last call
  { Sums q; q.so = -3; CHECK(refused(h, q, "self_offset = -3")); }
  CHECK(strstr(spa3d_last_error(h), "motion_kernel_sums: self_offset = -3"));
  CHECK(spa3d_destroy(h) == SPA3D_OK);
  puts("HOST_MOTION_KERNEL_OK");
  return 0;
}
