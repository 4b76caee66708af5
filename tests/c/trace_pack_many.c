/*
 * GPU test of mosfhet_tlwe_trace_pack_many on host structs (include/mosfhet_compat.h): N = 1024, key t = 4, base_bit = 9, ring noise 2^-45, 2^2 samples per output.
 *   - 9 samples under the extracted ring key give 3 outputs (the last holds one sample); the phase of output o is N m_j at coefficient j N / 4 and 0 elsewhere within
 *     2^58, the reference's own bound for the trace (test/tests.c:850); the worst is printed;
 *   - the outputs equal, word for word, what mosfhet_hip_tlwe_trace_pack_many_batch writes for the same samples laid out flat on the device;
 *   - log_per = 0 gives the words of mosfhet_tlwe_trace_pack.
 * Run by tests/test_trace_pack_many.py; exit status = number of failed checks.
 */
#include <math.h>
#include <mosfhet.h>
#include <mosfhet_hip.h>

/* the three HIP runtime calls this program needs (the library links the runtime; the HIP headers need a C++ compiler) */
int hipMalloc(void **ptr, size_t size);
int hipMemcpy(void *dst, const void *src, size_t bytes, int kind);
int hipFree(void *ptr);
enum { H2D = 1, D2H = 2 };

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __func__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

enum { N = 1024, T = 4, BASE_BIT = 9, TOTAL = 9, LOG_PER = 2, PER = 1 << LOG_PER, OUTPUTS = (TOTAL + PER - 1) / PER };

static double dist(Torus a, Torus b) { return fabs((double)(int64_t)(a - b)); }
static double lg(double x) { return log2(x > 1 ? x : 1); }

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_seed(0x4D414E59);
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, 1, 2.842170943040401e-14);    /* 2^-45 */
  TLWE_Key extracted = tlwe_alloc_key(N, rlwe_key->sigma);
  trlwe_extract_tlwe_key(extracted, rlwe_key);
  TRLWE_KS_Key *trace_key = trlwe_new_packing1_KS_key_CDKS21(rlwe_key, extracted, T, BASE_BIT);
  TorusPolynomial ph = polynomial_new_torus_polynomial(N);

  Torus msg[TOTAL];
  TLWE *in = tlwe_alloc_sample_array(TOTAL, N);
  for (int j = 0; j < TOTAL; j++) {
    msg[j] = (Torus)((j * 7 + 3) % 16) << (60 - 10);     /* mu / (16 N): N m stays on multiples of 1/16 */
    TLWE c = tlwe_new_sample(msg[j], extracted);
    tlwe_copy(in[j], c);
    free_tlwe(c);
  }
  TRLWE packed[OUTPUTS], single[TOTAL], one[TOTAL];
  for (int o = 0; o < OUTPUTS; o++) packed[o] = trlwe_alloc_new_sample(1, N);
  for (int j = 0; j < TOTAL; j++) { single[j] = trlwe_alloc_new_sample(1, N); one[j] = trlwe_alloc_new_sample(1, N); }
  mosfhet_tlwe_trace_pack_many(packed, in, TOTAL, LOG_PER, trace_key);
  double worst = 0;
  for (int o = 0; o < OUTPUTS; o++) {
    trlwe_phase(ph, packed[o], rlwe_key);
    for (int i = 0; i < N; i++) {
      const int j = o * PER + i / (N / PER);
      const Torus want = i % (N / PER) == 0 && j < TOTAL ? msg[j] * (Torus)N : 0;
      const double e = dist(ph->coeffs[i], want);
      if (e > worst) worst = e;
    }
  }
  printf("trace_pack_many: worst phase 2^%.1f from N m_j at j N / %d (bound 2^58)\n", lg(worst), PER);
  CHECK(worst <= 0x1p58, "a packed output does not decrypt (2^%.1f)", lg(worst));

  /* log_per = 0 is the trace call */
  mosfhet_tlwe_trace_pack_many(one, in, TOTAL, 0, trace_key);
  mosfhet_tlwe_trace_pack(single, in, TOTAL, trace_key);
  int differ = 0;
  for (int j = 0; j < TOTAL; j++)
    differ += memcmp(one[j]->a[0]->coeffs, single[j]->a[0]->coeffs, sizeof(Torus) * N) != 0 || memcmp(one[j]->b->coeffs, single[j]->b->coeffs, sizeof(Torus) * N) != 0;
  CHECK(differ == 0, "log_per = 0: %d of %d outputs differ from mosfhet_tlwe_trace_pack", differ, TOTAL);

  /* the same samples flat on the device, through the C ABI */
  const size_t in_w = (size_t)TOTAL * (N + 1), out_w = (size_t)OUTPUTS * 2 * N;
  Torus *h_in = (Torus *)malloc(sizeof(Torus) * in_w), *h_out = (Torus *)malloc(sizeof(Torus) * out_w), *d = NULL;
  for (int j = 0; j < TOTAL; j++) {
    memcpy(h_in + (size_t)j * (N + 1), in[j]->a, sizeof(Torus) * N);
    h_in[(size_t)j * (N + 1) + N] = in[j]->b;
  }
  CHECK(hipMalloc((void **)&d, sizeof(Torus) * (in_w + out_w)) == 0, "hipMalloc");
  if (failures) return failures;
  CHECK(hipMemcpy(d, h_in, sizeof(Torus) * in_w, H2D) == 0, "hipMemcpy to the device");
  mosfhet_hip_ctx_t ctx = (mosfhet_hip_ctx_t)mosfhet_engine_ctx();
  const int rc = mosfhet_hip_tlwe_trace_pack_many_batch(ctx, (mosfhet_hip_gak_t)trace_key[0]->device, 0, d + in_w, d, TOTAL, LOG_PER, NULL);
  CHECK(rc == 0, "mosfhet_hip_tlwe_trace_pack_many_batch: %s", mosfhet_hip_last_error());
  CHECK(mosfhet_hip_ctx_sync(ctx, NULL) == 0, "sync");
  CHECK(hipMemcpy(h_out, d + in_w, sizeof(Torus) * out_w, D2H) == 0, "hipMemcpy from the device");
  differ = 0;
  for (int o = 0; o < OUTPUTS; o++)
    differ += memcmp(packed[o]->a[0]->coeffs, h_out + (size_t)o * 2 * N, sizeof(Torus) * N) != 0 || memcmp(packed[o]->b->coeffs, h_out + (size_t)o * 2 * N + N, sizeof(Torus) * N) != 0;
  CHECK(differ == 0, "%d of %d outputs differ from mosfhet_hip_tlwe_trace_pack_many_batch", differ, OUTPUTS);
  CHECK(mosfhet_hip_tlwe_trace_pack_many_batch(ctx, (mosfhet_hip_gak_t)trace_key[0]->device, 1, d + in_w, d, TOTAL, LOG_PER, NULL) == MOSFHET_HIP_EINVAL,
        "entry0 = 1 on a set of log2 N entries was accepted");
  CHECK(mosfhet_hip_tlwe_trace_pack_many_batch(ctx, (mosfhet_hip_gak_t)trace_key[0]->device, 0, d + in_w, d, TOTAL, 11, NULL) == MOSFHET_HIP_EINVAL, "log_per = 11 at N = 1024 was accepted");
  hipFree(d);
  free(h_in);
  free(h_out);
  if (!failures) printf("trace_pack_many ok\n");
  return failures;
}
