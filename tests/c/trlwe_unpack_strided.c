/*
 * GPU test of mosfhet_trlwe_unpack_strided and mosfhet_trlwe_unpack_strided_keyswitch (include/mosfhet_compat.h): N = 1024, 70 samples opened 40 per input (a whole
 * input and a partly opened one) at the coefficients 24 + 25 j, messages on multiples of 1/16 at every coefficient, on host structs; the switch goes to n = 24 with
 * t = 4, base_bit = 4.
 *   - mosfhet_trlwe_unpack_strided equals, word for word, the drop-in layer's trlwe_extract_tlwe(in[o], 24 + 25 j) of every (input, j) and what
 *     mosfhet_hip_trlwe_unpack_strided_batch writes for the same inputs laid out flat on the device;
 *   - mosfhet_trlwe_unpack_strided_keyswitch equals, word for word, the drop-in layer's tlwe_keyswitch of every extracted sample and
 *     mosfhet_hip_trlwe_unpack_strided_keyswitch_batch;
 *   - every extracted and every switched sample decrypts to its message within half a slot (2^59);
 *   - (first 0, stride 1) gives the words of mosfhet_trlwe_unpack.
 * Run by tests/test_trlwe_unpack_strided.py; exit status = number of failed checks.
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

enum { n = 24, N = 1024, T = 4, BASE_BIT = 4, TOTAL = 70, PER = 40, INPUTS = 2, FIRST = 24, STRIDE = 25 };

static double dist(Torus a, Torus b) { return fabs((double)(int64_t)(a - b)); }

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_seed(0x53545244);
  TLWE_Key lwe_key = tlwe_new_binary_key(n, 9.094947017729282e-13);            /* 2^-40 */
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, 1, 9.094947017729282e-13);
  TLWE_Key extracted = tlwe_alloc_key(N, 9.094947017729282e-13);
  trlwe_extract_tlwe_key(extracted, rlwe_key);
  TLWE_KS_Key ksk = tlwe_new_KS_key(lwe_key, extracted, T, BASE_BIT);

  Torus msg[TOTAL];
  TRLWE in[INPUTS];
  TorusPolynomial m = polynomial_new_torus_polynomial(N);
  for (int o = 0; o < INPUTS; o++) {
    for (int j = 0; j < N; j++) m->coeffs[j] = (Torus)((o * 5 + j * 7 + 3) % 16) << 60;
    for (int j = 0; j < PER && o * PER + j < TOTAL; j++) msg[o * PER + j] = m->coeffs[FIRST + j * STRIDE];
    in[o] = trlwe_new_sample(m, rlwe_key);
  }
  TLWE *wide = tlwe_alloc_sample_array(TOTAL, N), *narrow = tlwe_alloc_sample_array(TOTAL, n);
  TLWE ext = tlwe_alloc_sample(N), sw = tlwe_alloc_sample(n);

  /* the same inputs flat on the device, through the C ABI */
  const size_t in_w = (size_t)INPUTS * 2 * N, wide_w = (size_t)TOTAL * (N + 1), narrow_w = (size_t)TOTAL * (n + 1);
  Torus *h_in = (Torus *)malloc(sizeof(Torus) * in_w), *h_out = (Torus *)malloc(sizeof(Torus) * wide_w), *d = NULL;
  for (int o = 0; o < INPUTS; o++) {
    memcpy(h_in + (size_t)o * 2 * N, in[o]->a[0]->coeffs, sizeof(Torus) * N);
    memcpy(h_in + (size_t)o * 2 * N + N, in[o]->b->coeffs, sizeof(Torus) * N);
  }
  CHECK(hipMalloc((void **)&d, sizeof(Torus) * (in_w + wide_w)) == 0, "hipMalloc");
  if (failures) return failures;
  CHECK(hipMemcpy(d, h_in, sizeof(Torus) * in_w, H2D) == 0, "hipMemcpy to the device");
  mosfhet_hip_ctx_t ctx = (mosfhet_hip_ctx_t)mosfhet_engine_ctx();

  /* part 1 */
  mosfhet_trlwe_unpack_strided(wide, in, TOTAL, PER, FIRST, STRIDE);
  int rc = mosfhet_hip_trlwe_unpack_strided_batch(ctx, d + in_w, d, N, TOTAL, PER, FIRST, STRIDE, NULL);
  CHECK(rc == 0, "mosfhet_hip_trlwe_unpack_strided_batch: %s", mosfhet_hip_last_error());
  CHECK(mosfhet_hip_ctx_sync(ctx, NULL) == 0, "sync");
  CHECK(hipMemcpy(h_out, d + in_w, sizeof(Torus) * wide_w, D2H) == 0, "hipMemcpy from the device");
  int differ_abi = 0, differ_loop = 0;
  double worst = 0;
  for (int j = 0; j < TOTAL; j++) {
    const Torus *w = h_out + (size_t)j * (N + 1);
    differ_abi += memcmp(wide[j]->a, w, sizeof(Torus) * N) != 0 || wide[j]->b != w[N];
    trlwe_extract_tlwe(ext, in[j / PER], FIRST + (j % PER) * STRIDE);
    differ_loop += memcmp(wide[j]->a, ext->a, sizeof(Torus) * N) != 0 || wide[j]->b != ext->b;
    const double e = dist(tlwe_phase(wide[j], extracted), msg[j]);
    if (e > worst) worst = e;
  }
  printf("strided unpack: %d of %d samples differ from the C-ABI call, %d from the trlwe_extract_tlwe loop; worst distance from the messages 2^%.1f (half a slot: 2^59)\n", differ_abi, TOTAL,
         differ_loop, log2(worst > 1 ? worst : 1));
  CHECK(differ_abi == 0, "%d samples of mosfhet_trlwe_unpack_strided differ from mosfhet_hip_trlwe_unpack_strided_batch", differ_abi);
  CHECK(differ_loop == 0, "%d samples of mosfhet_trlwe_unpack_strided differ from trlwe_extract_tlwe", differ_loop);
  CHECK(worst < 0x1p59, "an extracted sample does not decrypt (2^%.1f)", log2(worst > 1 ? worst : 1));

  /* part 2 */
  mosfhet_trlwe_unpack_strided_keyswitch(narrow, in, TOTAL, PER, FIRST, STRIDE, ksk);
  rc = mosfhet_hip_trlwe_unpack_strided_keyswitch_batch(ctx, (mosfhet_hip_ksk_t)ksk->device, d + in_w, d, TOTAL, PER, FIRST, STRIDE, NULL);
  CHECK(rc == 0, "mosfhet_hip_trlwe_unpack_strided_keyswitch_batch: %s", mosfhet_hip_last_error());
  CHECK(mosfhet_hip_ctx_sync(ctx, NULL) == 0, "sync");
  CHECK(hipMemcpy(h_out, d + in_w, sizeof(Torus) * narrow_w, D2H) == 0, "hipMemcpy from the device");
  differ_abi = differ_loop = 0;
  worst = 0;
  for (int j = 0; j < TOTAL; j++) {
    const Torus *w = h_out + (size_t)j * (n + 1);
    differ_abi += memcmp(narrow[j]->a, w, sizeof(Torus) * n) != 0 || narrow[j]->b != w[n];
    tlwe_keyswitch(sw, wide[j], ksk);
    differ_loop += memcmp(narrow[j]->a, sw->a, sizeof(Torus) * n) != 0 || narrow[j]->b != sw->b;
    const double e = dist(tlwe_phase(narrow[j], lwe_key), msg[j]);
    if (e > worst) worst = e;
  }
  printf("strided unpack + key switch: %d of %d samples differ from the C-ABI call, %d from the tlwe_keyswitch loop; worst distance from the messages 2^%.1f (half a slot: 2^59)\n",
         differ_abi, TOTAL, differ_loop, log2(worst > 1 ? worst : 1));
  CHECK(differ_abi == 0, "%d samples of mosfhet_trlwe_unpack_strided_keyswitch differ from mosfhet_hip_trlwe_unpack_strided_keyswitch_batch", differ_abi);
  CHECK(differ_loop == 0, "%d samples of mosfhet_trlwe_unpack_strided_keyswitch differ from tlwe_keyswitch of the extracted samples", differ_loop);
  CHECK(worst < 0x1p59, "a switched sample does not decrypt (2^%.1f)", log2(worst > 1 ? worst : 1));

  /* (first 0, stride 1) is the call without a geometry */
  TLWE *plain = tlwe_alloc_sample_array(TOTAL, N);
  mosfhet_trlwe_unpack(plain, in, TOTAL, PER);
  mosfhet_trlwe_unpack_strided(wide, in, TOTAL, PER, 0, 1);
  int differ_plain = 0;
  for (int j = 0; j < TOTAL; j++) differ_plain += memcmp(wide[j]->a, plain[j]->a, sizeof(Torus) * N) != 0 || wide[j]->b != plain[j]->b;
  CHECK(differ_plain == 0, "%d samples of mosfhet_trlwe_unpack_strided at (0, 1) differ from mosfhet_trlwe_unpack", differ_plain);

  hipFree(d);
  free(h_in);
  free(h_out);
  if (!failures) printf("trlwe_unpack_strided ok\n");
  return failures;
}
