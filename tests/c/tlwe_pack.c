/*
 * GPU test of mosfhet_tlwe_pack (include/mosfhet_compat.h): N = 1024, n_in = 16, t = 4, base_bit = 6, 70 samples packed 64 per output (a full output and a short
 * one), messages on multiples of 1/16, on host structs.
 *   - the outputs equal, word for word, what mosfhet_hip_tlwe_pack_batch writes for the same samples laid out flat on the device, at split = 1 and split = 3;
 *   - every packed coefficient decrypts to its message within half a slot (2^59), the coefficients past the last sample of the short output to 0;
 *   - the phases lie within 2^40 of those of the drop-in layer's trlwe_full_packing_keyswitch loop on the same inputs and key: the two differ by the n_in roundings
 *     of the loop against the one of the new call, and by FFT rounding.  Measured: 2^27.5 (split 1), 2^27.6 (split 3); printed by every run.
 * Run by tests/test_tlwe_pack.py; exit status = number of failed checks.
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

enum { n = 16, N = 1024, T = 4, BASE_BIT = 6, TOTAL = 70, PER = 64, OUTPUTS = 2 };

static double dist(Torus a, Torus b) { return fabs((double)(int64_t)(a - b)); }

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_seed(0x5041434B);
  TLWE_Key lwe_key = tlwe_new_binary_key(n, 9.313225746154785e-10);          /* 2^-30 */
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, 1, 5.684341886080802e-14);    /* 2^-44 */
  TRLWE_KS_Key key = trlwe_new_full_packing_KS_key(rlwe_key, lwe_key, T, BASE_BIT);

  Torus msg[TOTAL];
  TLWE *in = tlwe_alloc_sample_array(TOTAL, n);
  for (int j = 0; j < TOTAL; j++) {
    msg[j] = (Torus)((j * 7 + 3) % 16) << 60;
    TLWE c = tlwe_new_sample(msg[j], lwe_key);
    tlwe_copy(in[j], c);
    free_tlwe(c);
  }
  TRLWE got[OUTPUTS], loop[OUTPUTS];
  for (int o = 0; o < OUTPUTS; o++) { got[o] = trlwe_alloc_new_sample(1, N); loop[o] = trlwe_alloc_new_sample(1, N); }

  /* the same samples flat on the device, through the C ABI */
  const size_t in_w = (size_t)TOTAL * (n + 1), out_w = (size_t)OUTPUTS * 2 * N;
  Torus *h_in = (Torus *)malloc(sizeof(Torus) * in_w), *h_out = (Torus *)malloc(sizeof(Torus) * out_w), *d = NULL;
  for (int j = 0; j < TOTAL; j++) {
    memcpy(h_in + (size_t)j * (n + 1), in[j]->a, sizeof(Torus) * n);
    h_in[(size_t)j * (n + 1) + n] = in[j]->b;
  }
  CHECK(hipMalloc((void **)&d, sizeof(Torus) * (in_w + out_w)) == 0, "hipMalloc");
  if (failures) return failures;
  CHECK(hipMemcpy(d, h_in, sizeof(Torus) * in_w, H2D) == 0, "hipMemcpy to the device");
  mosfhet_hip_ctx_t ctx = (mosfhet_hip_ctx_t)mosfhet_engine_ctx();

  const int splits[2] = {1, 3};
  for (int s = 0; s < 2; s++) {
    mosfhet_tlwe_pack(got, in, TOTAL, PER, key, splits[s]);
    const int rc = mosfhet_hip_tlwe_pack_batch(ctx, (mosfhet_hip_gak_t)key->device, d + in_w, d, TOTAL, PER, splits[s], NULL);
    CHECK(rc == 0, "mosfhet_hip_tlwe_pack_batch: %s", mosfhet_hip_last_error());
    CHECK(mosfhet_hip_ctx_sync(ctx, NULL) == 0, "sync");
    CHECK(hipMemcpy(h_out, d + in_w, sizeof(Torus) * out_w, D2H) == 0, "hipMemcpy from the device");
    int differ = 0;
    for (int o = 0; o < OUTPUTS; o++)
      differ += memcmp(got[o]->a[0]->coeffs, h_out + (size_t)o * 2 * N, sizeof(Torus) * N) != 0 || memcmp(got[o]->b->coeffs, h_out + (size_t)o * 2 * N + N, sizeof(Torus) * N) != 0;
    printf("split %d: %d of %d outputs of mosfhet_tlwe_pack differ from the C-ABI call as words\n", splits[s], differ, OUTPUTS);
    CHECK(differ == 0, "split %d: %d of %d outputs differ from mosfhet_hip_tlwe_pack_batch", splits[s], differ, OUTPUTS);

    /* decryption, and the distance from the drop-in layer's loop */
    TorusPolynomial ph = polynomial_new_torus_polynomial(N), ph_loop = polynomial_new_torus_polynomial(N);
    double worst = 0, apart = 0;
    for (int o = 0; o < OUTPUTS; o++) {
      const int have = TOTAL - o * PER < PER ? TOTAL - o * PER : PER;
      trlwe_full_packing_keyswitch(loop[o], in + (size_t)o * PER, (uint64_t)have, key);
      trlwe_phase(ph, got[o], rlwe_key);
      trlwe_phase(ph_loop, loop[o], rlwe_key);
      for (int j = 0; j < N; j++) {
        const double e = dist(ph->coeffs[j], j < have ? msg[o * PER + j] : 0), a = dist(ph->coeffs[j], ph_loop->coeffs[j]);
        if (e > worst) worst = e;
        if (a > apart) apart = a;
      }
    }
    printf("split %d: worst distance from the messages 2^%.1f (half a slot: 2^59); from the phases of the trlwe_full_packing_keyswitch loop 2^%.1f (bound 2^40)\n", splits[s],
           log2(worst > 1 ? worst : 1), log2(apart > 1 ? apart : 1));
    CHECK(worst < 0x1p59, "split %d: an output does not decrypt (2^%.1f)", splits[s], log2(worst > 1 ? worst : 1));
    CHECK(apart < 0x1p40, "split %d: phases 2^%.1f from the existing loop's", splits[s], log2(apart > 1 ? apart : 1));
    free_polynomial(ph);
    free_polynomial(ph_loop);
  }
  hipFree(d);
  free(h_in);
  free(h_out);
  if (!failures) printf("tlwe_pack ok\n");
  return failures;
}
