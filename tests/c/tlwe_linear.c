/*
 * GPU test of mosfhet_tlwe_linear_inputs and mosfhet_tlwe_linear_bootstrap_inputs (include/mosfhet_compat.h) at the reference's SET_1 (n = 585, N = 1024, l = 2,
 * Bg = 2^8, key switch t = 5, base_bit = 2): a 4 -> 3 layer on 2 inputs given as host structs.
 *   - out[b][j] word for word equal to a loop of tlwe_scale_addto (src/tlwe.c:143-191) over the row's weights, written here against include/mosfhet.h, starting from
 *     the trivial sample of the bias (or of 0 without one): with narrow weights, and with weights that need all 64 bits;
 *   - the fused call word for word equal to that loop followed by tlwe_keyswitch and functional_bootstrap, one sample at a time;
 *   - the fused result decrypts: inputs +-1/16, weights in [-2, 2] with an odd sum of magnitudes per row, bias -1/16 (the slots of torus_base 4 are centred on
 *     m / 8, so the sign changes at -1/16), the constant table 1/16: out = sign(W x) / 16 within 2^60 (half a slot).
 * The bootstrap key's product order is set, so that no word depends on how many samples a launch holds.
 * Run by tests/test_tlwe_linear.py; exit status = number of failed checks.
 */
#include <math.h>
#include <mosfhet.h>
#include <mosfhet_hip.h>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __func__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static int same_tlwe(TLWE a, TLWE b) { return a->n == b->n && a->b == b->b && !memcmp(a->a, b->a, sizeof(Torus) * (size_t)a->n); }

enum { n = 585, N = 1024, k = 1, l = 2, Bg_bit = 8, COUNT = 2, ROWS_IN = 4, ROWS_OUT = 3 };

/* want = (0, bias) + sum_i W[i] in[i] by the reference's own calls */
static void row_by_scale_addto(TLWE want, TLWE *in, const int64_t *W, Torus bias) {
  tlwe_noiseless_trivial_sample(want, bias);
  for (int i = 0; i < ROWS_IN; i++) tlwe_scale_addto(want, in[i], (Torus)W[i]);
}

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_seed(0x4C494E);
  TLWE_Key lwe_key = tlwe_new_binary_key(n, 9.141776004202573e-5);
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, k, 2.989040792967434e-8);
  TLWE_Key extracted = tlwe_alloc_key(N, rlwe_key->sigma);
  trlwe_extract_tlwe_key(extracted, rlwe_key);
  TRGSW_Key gkey = trgsw_new_key(rlwe_key, l, Bg_bit);
  Bootstrap_Key bk = new_bootstrap_key(gkey, lwe_key, 1);
  mosfhet_bootstrap_key_set_product_order(bk, MOSFHET_HIP_ORDER_REFERENCE);
  TLWE_KS_Key ksk = tlwe_new_KS_key(lwe_key, extracted, 5, 2);

  static const int64_t W_toy[ROWS_OUT][ROWS_IN] = {{2, -1, 1, -1}, {1, 1, -1, 0}, {-2, 1, 0, 2}};
  static const int64_t W_wide[ROWS_OUT][ROWS_IN] = {{(int64_t)1 << 40, -1, INT64_MIN, 3}, {INT64_MAX, ((int64_t)1 << 32) + 1, 0, -((int64_t)1 << 32)}, {(int64_t)1 << 31, -((int64_t)1 << 31), 1, 7}};
  static const int signs[COUNT][ROWS_IN] = {{1, 1, 1, 1}, {-1, 1, -1, 1}};
  const Torus sixteenth = double2torus(1. / 16), bias_toy[ROWS_OUT] = {-sixteenth, -sixteenth, -sixteenth};
  const Torus bias_wide[ROWS_OUT] = {0xFFFFFFFFFFFFFFFFULL, 1, 0x123456789ABCDEF0ULL};

  TLWE *in[COUNT], *got[COUNT], *want[COUNT];
  for (int b = 0; b < COUNT; b++) {
    in[b] = tlwe_alloc_sample_array(ROWS_IN, N);
    got[b] = tlwe_alloc_sample_array(ROWS_OUT, N);
    want[b] = tlwe_alloc_sample_array(ROWS_OUT, N);
    for (int i = 0; i < ROWS_IN; i++) {
      TLWE c = tlwe_new_sample(signs[b][i] > 0 ? sixteenth : -sixteenth, extracted);
      tlwe_copy(in[b][i], c);
      free_tlwe(c);
    }
  }

  /* the linear map alone */
  const struct { const char *name; const int64_t *W; const Torus *bias; } cases[] = {
      {"narrow weights, bias", &W_toy[0][0], bias_toy}, {"narrow weights, no bias", &W_toy[0][0], NULL}, {"wide weights, bias", &W_wide[0][0], bias_wide},
      {"wide weights, no bias", &W_wide[0][0], NULL}};
  for (size_t c = 0; c < sizeof(cases) / sizeof(cases[0]); c++) {
    mosfhet_tlwe_linear_inputs(got, in, cases[c].W, cases[c].bias, ROWS_OUT, ROWS_IN, COUNT);
    int differ = 0;
    for (int b = 0; b < COUNT; b++)
      for (int j = 0; j < ROWS_OUT; j++) {
        row_by_scale_addto(want[b][j], in[b], cases[c].W + (size_t)j * ROWS_IN, cases[c].bias ? cases[c].bias[j] : 0);
        differ += !same_tlwe(got[b][j], want[b][j]);
      }
    printf("%s: %d of %d outputs differ from the loop of tlwe_scale_addto as words\n", cases[c].name, differ, COUNT * ROWS_OUT);
    CHECK(differ == 0, "%s: %d of %d outputs of mosfhet_tlwe_linear_inputs differ from the loop of tlwe_scale_addto", cases[c].name, differ, COUNT * ROWS_OUT);
  }

  /* the layer and its activation */
  Torus table[4] = {sixteenth, sixteenth, sixteenth, sixteenth};
  TRLWE tv = trlwe_alloc_new_sample(k, N);
  trlwe_torus_packing(tv, table, 4);
  mosfhet_tlwe_linear_bootstrap_inputs(got, in, &W_toy[0][0], bias_toy, ROWS_OUT, ROWS_IN, COUNT, tv, bk, ksk, 4);
  TLWE sum = tlwe_alloc_sample(N), switched = tlwe_alloc_sample(n), res = tlwe_alloc_sample(N);
  int differ = 0, wrong = 0;
  double worst = 0;
  for (int b = 0; b < COUNT; b++)
    for (int j = 0; j < ROWS_OUT; j++) {
      row_by_scale_addto(sum, in[b], W_toy[j], bias_toy[j]);
      tlwe_keyswitch(switched, sum, ksk);
      functional_bootstrap(res, tv, switched, bk, 4);
      differ += !same_tlwe(got[b][j], res);
      int s = 0;
      for (int i = 0; i < ROWS_IN; i++) s += (int)W_toy[j][i] * signs[b][i];
      const Torus expect = s > 0 ? sixteenth : -sixteenth;
      const double dist = fabs((double)(int64_t)(tlwe_phase(got[b][j], extracted) - expect));
      if (dist > worst) worst = dist;
      wrong += !(dist < 0x1p60);
    }
  printf("layer + activation: %d of %d outputs differ from scale_addto + tlwe_keyswitch + functional_bootstrap as words; worst distance from sign(W x) / 16: 2^%.1f\n", differ,
         COUNT * ROWS_OUT, log2(worst > 1 ? worst : 1));
  CHECK(differ == 0, "%d of %d outputs of mosfhet_tlwe_linear_bootstrap_inputs differ from the loop", differ, COUNT * ROWS_OUT);
  CHECK(wrong == 0, "%d of %d outputs of mosfhet_tlwe_linear_bootstrap_inputs do not decrypt to sign(W x) / 16 within 2^60", wrong, COUNT * ROWS_OUT);

  if (!failures) printf("tlwe_linear ok\n");
  return failures;
}
