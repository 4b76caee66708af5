/*
 * GPU test of the client half on the plain C ABI (include/mosfhet_hip.h): create a key handle, encrypt, open, destroy -- no host-struct layer.
 *   - N = 1024, n = 70, binary keys made here; 3 TLWE and 2 TRLWE samples of four-bit messages at sigma 2^-25 decode to their messages through the phase calls at
 *     msg_bits = 4, and the phases lie within 2^45 of the messages (sigma 2^64 = 2^39: more than 60 sigma);
 *   - a TRGSW batch of 2 samples at (l, Bg_bit) = (2, 8): with both outputs asked for, the torus rows are TRLWE samples whose phase is the gadget term within 2^45;
 *   - the refusals an embedding program meets first: a call that needs the key the handle lacks, msg_bits = 64.
 * Run by tests/test_client_samples.py; exit status = number of failed checks.
 */
#include <math.h>
#include <mosfhet_hip.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* the three HIP runtime calls this program needs (the library links the runtime; the HIP headers need a C++ compiler) */
int hipMalloc(void **ptr, size_t size);
int hipMemcpy(void *dst, const void *src, size_t bytes, int kind);
int hipFree(void *ptr);
enum { H2D = 1, D2H = 2 };

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __func__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

enum { N = 1024, n = 70, L = 2, BG = 8, TLWES = 3, TRLWES = 2, TRGSWS = 2, ROWS = TRGSWS * 2 * L };

static uint64_t tdist(uint64_t a, uint64_t b) { int64_t d = (int64_t)(a - b); return (uint64_t)(d < 0 ? -d : d); }

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  const double sigma = 2.9802322387695312e-08;   /* 2^-25 */
  static uint64_t s_rlwe[N], s_lwe[n], msg_t[TLWES], msg_r[TRLWES * N], got_t[TLWES], got_r[TRLWES * N], ph[ROWS * N];
  static unsigned char secret[32];
  uint64_t x = 0x9E3779B97F4A7C15ULL;
  for (int i = 0; i < N; i++) { x = x * 6364136223846793005ULL + 1442695040888963407ULL; s_rlwe[i] = (x >> 40) & 1; }
  for (int i = 0; i < n; i++) { x = x * 6364136223846793005ULL + 1442695040888963407ULL; s_lwe[i] = (x >> 40) & 1; }
  for (int i = 0; i < TLWES; i++) msg_t[i] = (uint64_t)((5 * i + 3) % 16) << 60;
  for (int i = 0; i < TRLWES * N; i++) msg_r[i] = (uint64_t)((7 * i + 1) % 16) << 60;
  for (int i = 0; i < 32; i++) secret[i] = (unsigned char)(i * 3 + 1);
  const int32_t m[TRGSWS] = {1, -1}, e[TRGSWS] = {0, N + 2};

  mosfhet_hip_ctx_t ctx = NULL;
  mosfhet_hip_client_key_t key = NULL, lwe_only = NULL;
  CHECK(mosfhet_hip_ctx_create(&ctx, 0) == 0, "ctx_create: %s", mosfhet_hip_last_error());
  if (failures) return failures;
  CHECK(mosfhet_hip_set_keygen_secret(secret) == 0, "set_keygen_secret");
  CHECK(mosfhet_hip_client_key_create(&key, s_rlwe, N, s_lwe, n) == 0, "client_key_create: %s", mosfhet_hip_last_error());
  CHECK(mosfhet_hip_client_key_create(&lwe_only, NULL, 0, s_lwe, n) == 0, "client_key_create (LWE only): %s", mosfhet_hip_last_error());
  int64_t info[6];
  CHECK(mosfhet_hip_client_key_info(key, info) == 0 && info[0] == N && info[1] == n && info[3] == 1 && info[5] == 1, "client_key_info");

  /* one device buffer: messages, samples, opened words */
  const size_t w_mt = TLWES, w_ct = (size_t)TLWES * (n + 1), w_mr = (size_t)TRLWES * N, w_cr = (size_t)TRLWES * 2 * N, w_g = (size_t)ROWS * 2 * N, w_ph = (size_t)ROWS * N;
  const size_t o_mt = 0, o_ct = o_mt + w_mt, o_mr = o_ct + w_ct, o_cr = o_mr + w_mr, o_g = o_cr + w_cr, o_gd = o_g + w_g, o_ph = o_gd + w_g, o_lists = o_ph + w_ph;
  uint64_t *d = NULL;
  CHECK(hipMalloc((void **)&d, sizeof(uint64_t) * (o_lists + 2)) == 0, "hipMalloc");
  if (failures) return failures;
  CHECK(hipMemcpy(d + o_mt, msg_t, sizeof(msg_t), H2D) == 0 && hipMemcpy(d + o_mr, msg_r, sizeof(msg_r), H2D) == 0, "hipMemcpy to the device");
  CHECK(hipMemcpy(d + o_lists, m, sizeof(m), H2D) == 0 && hipMemcpy(d + o_lists + 1, e, sizeof(e), H2D) == 0, "hipMemcpy to the device");

  /* TLWE and TRLWE: encrypt, open at four bits */
  CHECK(mosfhet_hip_tlwe_encrypt_batch(ctx, key, d + o_ct, d + o_mt, sigma, TLWES, NULL) == 0, "tlwe_encrypt: %s", mosfhet_hip_last_error());
  CHECK(mosfhet_hip_tlwe_phase_batch(ctx, lwe_only, d + o_ph, d + o_ct, 4, TLWES, NULL) == 0, "tlwe_phase: %s", mosfhet_hip_last_error());
  CHECK(mosfhet_hip_ctx_sync(ctx, NULL) == 0, "sync");
  CHECK(hipMemcpy(got_t, d + o_ph, sizeof(got_t), D2H) == 0, "hipMemcpy from the device");
  for (int i = 0; i < TLWES; i++) CHECK(got_t[i] == msg_t[i] >> 60, "TLWE sample %d decodes to %llu", i, (unsigned long long)got_t[i]);
  CHECK(mosfhet_hip_tlwe_phase_batch(ctx, key, d + o_ph, d + o_ct, 0, TLWES, NULL) == 0, "tlwe_phase: %s", mosfhet_hip_last_error());
  CHECK(mosfhet_hip_ctx_sync(ctx, NULL) == 0, "sync");
  CHECK(hipMemcpy(got_t, d + o_ph, sizeof(got_t), D2H) == 0, "hipMemcpy from the device");
  uint64_t worst = 0;
  for (int i = 0; i < TLWES; i++) { const uint64_t w = tdist(got_t[i], msg_t[i]); if (w > worst) worst = w; }
  CHECK(worst < (1ULL << 45), "a TLWE phase lies 2^%.1f from its message", log2((double)worst + 1.0));
  CHECK(mosfhet_hip_trlwe_encrypt_batch(ctx, key, d + o_cr, d + o_mr, sigma, TRLWES, NULL) == 0, "trlwe_encrypt: %s", mosfhet_hip_last_error());
  CHECK(mosfhet_hip_trlwe_phase_batch(ctx, key, d + o_ph, d + o_cr, 4, TRLWES, NULL) == 0, "trlwe_phase: %s", mosfhet_hip_last_error());
  CHECK(mosfhet_hip_ctx_sync(ctx, NULL) == 0, "sync");
  CHECK(hipMemcpy(got_r, d + o_ph, sizeof(got_r), D2H) == 0, "hipMemcpy from the device");
  int wrong = 0;
  for (int i = 0; i < TRLWES * N; i++) wrong += got_r[i] != msg_r[i] >> 60;
  CHECK(wrong == 0, "%d of %d TRLWE coefficients decode to another message", wrong, TRLWES * N);
  printf("TLWE and TRLWE round trips: %d failures so far (worst TLWE phase error 2^%.1f)\n", failures, log2((double)worst + 1.0));

  /* TRGSW: both outputs; every torus row opens to its gadget term */
  CHECK(mosfhet_hip_trgsw_encrypt_batch(ctx, key, (double *)(d + o_gd), d + o_g, (const int32_t *)(d + o_lists), (const int32_t *)(d + o_lists + 1), L, BG, sigma, TRGSWS, NULL) == 0,
        "trgsw_encrypt: %s", mosfhet_hip_last_error());
  CHECK(mosfhet_hip_trlwe_phase_batch(ctx, key, d + o_ph, d + o_g, 0, ROWS, NULL) == 0, "trlwe_phase of the TRGSW rows: %s", mosfhet_hip_last_error());
  CHECK(mosfhet_hip_ctx_sync(ctx, NULL) == 0, "sync");
  CHECK(hipMemcpy(ph, d + o_ph, sizeof(ph), D2H) == 0, "hipMemcpy from the device");
  worst = 0;
  for (int u = 0; u < TRGSWS; u++)
    for (int q = 0; q < 2 * L; q++) {
      const int c = q / L, j = q % L, ex = e[u] & (2 * N - 1);
      uint64_t h = (uint64_t)(int64_t)m[u] << (64 - (j + 1) * BG);
      if (ex & N) h = 0 - h;
      /* the gadget on the mask (c = 0) shows in the phase as -h X^e s, on the body (c = 1) as h X^e */
      for (int i = 0; i < N; i++) {
        uint64_t want = 0;
        if (c == 1) want = i == (ex & (N - 1)) ? h : 0;
        else {
          const int src = i - (ex & (N - 1));
          const uint64_t sv = s_rlwe[src & (N - 1)] * h;
          want = src < 0 ? sv : 0 - sv;
        }
        const uint64_t w = tdist(ph[((size_t)u * 2 * L + q) * N + i], want);
        if (w > worst) worst = w;
      }
    }
  CHECK(worst < (1ULL << 45), "a TRGSW row's phase lies 2^%.1f from its gadget term", log2((double)worst + 1.0));
  printf("TRGSW rows: worst phase error 2^%.1f (bound 2^45)\n", log2((double)worst + 1.0));

  /* refusals */
  CHECK(mosfhet_hip_trlwe_encrypt_batch(ctx, lwe_only, d + o_cr, NULL, sigma, 1, NULL) == MOSFHET_HIP_EINVAL && strstr(mosfhet_hip_last_error(), "h_s_rlwe"), "the missing key is not refused");
  CHECK(mosfhet_hip_tlwe_phase_batch(ctx, key, d + o_ph, d + o_ct, 64, TLWES, NULL) == MOSFHET_HIP_EINVAL && strstr(mosfhet_hip_last_error(), "msg_bits"), "msg_bits = 64 is not refused");

  CHECK(hipFree(d) == 0, "hipFree");
  CHECK(mosfhet_hip_client_key_destroy(key) == 0 && mosfhet_hip_client_key_destroy(lwe_only) == 0, "client_key_destroy");
  CHECK(mosfhet_hip_ctx_destroy(ctx) == 0, "ctx_destroy");
  if (!failures) printf("client_samples ok\n");
  return failures;
}
