/*
 * GPU test of the trace switch and the gadget -> TRGSW conversion on host structs (include/mosfhet_compat.h): N = 1024, key t = 4, base_bit = 9, ring noise 2^-45.
 *   - mosfhet_tlwe_trace_pack of 5 samples under the extracted ring key equals five single trlwe_packing1_keyswitch_CDKS21 calls word for word;
 *   - the phases are N m at coefficient 0 and 0 elsewhere within 2^58, the reference's own bound (test/tests.c:850); the worst is printed;
 *   - the outputs equal, word for word, what mosfhet_hip_tlwe_trace_pack_batch writes for the same samples laid out flat on the device;
 *   - trlwe_RLWE_priv_keyswitch with the gadget key turns TRLWE(m) into TRLWE(-s m): within 2^52 of it, the tolerance of the reference's private-switch test;
 *   - trgsw_from_gadget (l = 2, Bg_bit = 8) of the gadget rows of the bits 0 and 1 gives TRGSWs whose external product with a TRLWE sample on multiples of 1/16
 *     decrypts to bit x message within 2^57 (half a slot less two bits).
 * Run by tests/test_trace_conversions.py; exit status = number of failed checks.
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

enum { N = 1024, T = 4, BASE_BIT = 9, COUNT = 5, L = 2, BG_BIT = 8 };

static double dist(Torus a, Torus b) { return fabs((double)(int64_t)(a - b)); }
static double lg(double x) { return log2(x > 1 ? x : 1); }

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_seed(0x54524143);
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, 1, 2.842170943040401e-14);    /* 2^-45 */
  TLWE_Key extracted = tlwe_alloc_key(N, rlwe_key->sigma);
  trlwe_extract_tlwe_key(extracted, rlwe_key);
  TRLWE_KS_Key *trace_key = trlwe_new_packing1_KS_key_CDKS21(rlwe_key, extracted, T, BASE_BIT);
  TorusPolynomial ph = polynomial_new_torus_polynomial(N);

  /* ---- the trace ---- */
  Torus msg[COUNT];
  TLWE *in = tlwe_alloc_sample_array(COUNT, N);
  TRLWE batch[COUNT], single[COUNT];
  for (int j = 0; j < COUNT; j++) {
    msg[j] = (Torus)((j * 7 + 3) % 16) << 60;
    TLWE c = tlwe_new_sample(msg[j], extracted);
    tlwe_copy(in[j], c);
    free_tlwe(c);
    batch[j] = trlwe_alloc_new_sample(1, N);
    single[j] = trlwe_alloc_new_sample(1, N);
  }
  mosfhet_tlwe_trace_pack(batch, in, COUNT, trace_key);
  int differ = 0;
  double worst = 0;
  for (int j = 0; j < COUNT; j++) {
    trlwe_packing1_keyswitch_CDKS21(single[j], in[j], trace_key);
    differ += memcmp(batch[j]->a[0]->coeffs, single[j]->a[0]->coeffs, sizeof(Torus) * N) != 0 || memcmp(batch[j]->b->coeffs, single[j]->b->coeffs, sizeof(Torus) * N) != 0;
    trlwe_phase(ph, batch[j], rlwe_key);
    for (int i = 0; i < N; i++) {
      const double e = dist(ph->coeffs[i], i == 0 ? msg[j] * (Torus)N : 0);
      if (e > worst) worst = e;
    }
  }
  printf("trace: %d of %d outputs of mosfhet_tlwe_trace_pack differ from single trlwe_packing1_keyswitch_CDKS21 calls; worst phase 2^%.1f from N m (bound 2^58)\n", differ, COUNT,
         lg(worst));
  CHECK(differ == 0, "%d of %d outputs differ from the single calls", differ, COUNT);
  CHECK(worst <= 0x1p58, "a trace does not decrypt to N m (2^%.1f)", lg(worst));

  /* the same samples flat on the device, through the C ABI */
  const size_t in_w = (size_t)COUNT * (N + 1), out_w = (size_t)COUNT * 2 * N;
  Torus *h_in = (Torus *)malloc(sizeof(Torus) * in_w), *h_out = (Torus *)malloc(sizeof(Torus) * out_w), *d = NULL;
  for (int j = 0; j < COUNT; j++) {
    memcpy(h_in + (size_t)j * (N + 1), in[j]->a, sizeof(Torus) * N);
    h_in[(size_t)j * (N + 1) + N] = in[j]->b;
  }
  CHECK(hipMalloc((void **)&d, sizeof(Torus) * (in_w + out_w)) == 0, "hipMalloc");
  if (failures) return failures;
  CHECK(hipMemcpy(d, h_in, sizeof(Torus) * in_w, H2D) == 0, "hipMemcpy to the device");
  mosfhet_hip_ctx_t ctx = (mosfhet_hip_ctx_t)mosfhet_engine_ctx();
  const int rc = mosfhet_hip_tlwe_trace_pack_batch(ctx, (mosfhet_hip_gak_t)trace_key[0]->device, 0, d + in_w, d, COUNT, NULL);
  CHECK(rc == 0, "mosfhet_hip_tlwe_trace_pack_batch: %s", mosfhet_hip_last_error());
  CHECK(mosfhet_hip_ctx_sync(ctx, NULL) == 0, "sync");
  CHECK(hipMemcpy(h_out, d + in_w, sizeof(Torus) * out_w, D2H) == 0, "hipMemcpy from the device");
  differ = 0;
  for (int j = 0; j < COUNT; j++)
    differ += memcmp(batch[j]->a[0]->coeffs, h_out + (size_t)j * 2 * N, sizeof(Torus) * N) != 0 || memcmp(batch[j]->b->coeffs, h_out + (size_t)j * 2 * N + N, sizeof(Torus) * N) != 0;
  CHECK(differ == 0, "%d of %d outputs differ from mosfhet_hip_tlwe_trace_pack_batch", differ, COUNT);
  CHECK(mosfhet_hip_tlwe_trace_pack_batch(ctx, (mosfhet_hip_gak_t)trace_key[0]->device, 1, d + in_w, d, COUNT, NULL) == MOSFHET_HIP_EINVAL, "entry0 = 1 on a set of log2 N entries was accepted");

  /* ---- the private switch and the gadget conversion ---- */
  TRLWE_KS_Key *gadget_key = trlwe_new_gadget_to_RGSW_KS(rlwe_key, T, BASE_BIT);
  TorusPolynomial m = polynomial_new_torus_polynomial(N), sm = polynomial_new_torus_polynomial(N);
  for (int i = 0; i < N; i++) m->coeffs[i] = (Torus)((i * 5 + 1) % 16) << 60;
  TRLWE ct = trlwe_new_sample(m, rlwe_key), sw = trlwe_alloc_new_sample(1, N);
  trlwe_RLWE_priv_keyswitch(sw, ct, gadget_key[0]);
  polynomial_naive_mul_torus(sm, m, rlwe_key->s[0]);
  trlwe_phase(ph, sw, rlwe_key);
  worst = 0;
  for (int i = 0; i < N; i++) { const double e = dist(ph->coeffs[i], (Torus)0 - sm->coeffs[i]); if (e > worst) worst = e; }
  printf("private switch: 2^%.1f from -s m (bound 2^52)\n", lg(worst));
  CHECK(worst < 0x1p52, "trlwe_RLWE_priv_keyswitch: 2^%.1f from -s m", lg(worst));

  TRLWE_DFT prod_dft = trlwe_alloc_new_DFT_sample(1, N);
  TRLWE prod = trlwe_alloc_new_sample(1, N);
  for (int bit = 0; bit < 2; bit++) {
    TRLWE rows[L];
    for (int i = 0; i < L; i++) {
      TorusPolynomial g = polynomial_new_torus_polynomial(N);
      memset(g->coeffs, 0, sizeof(Torus) * N);
      g->coeffs[0] = (Torus)bit << (64 - (i + 1) * BG_BIT);
      rows[i] = trlwe_new_sample(g, rlwe_key);
      free_polynomial(g);
    }
    TRGSW_DFT sel = trgsw_alloc_new_DFT_sample(L, BG_BIT, 1, N);
    trgsw_from_gadget(sel, rows, gadget_key);
    trgsw_mul_trlwe_DFT(prod_dft, ct, sel);
    trlwe_from_DFT(prod, prod_dft);
    trlwe_phase(ph, prod, rlwe_key);
    worst = 0;
    for (int i = 0; i < N; i++) { const double e = dist(ph->coeffs[i], bit ? m->coeffs[i] : 0); if (e > worst) worst = e; }
    printf("trgsw_from_gadget, bit %d: external product 2^%.1f from bit x message (bound 2^57)\n", bit, lg(worst));
    CHECK(worst < 0x1p57, "bit %d: the TRGSW from the gadget rows does not select (2^%.1f)", bit, lg(worst));
    for (int i = 0; i < L; i++) free_trlwe(rows[i]);
  }
  hipFree(d);
  free(h_in);
  free(h_out);
  if (!failures) printf("trace_conversions ok\n");
  return failures;
}
