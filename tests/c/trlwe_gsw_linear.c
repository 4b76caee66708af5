/*
 * GPU test of mosfhet_trlwe_gsw_linear and mosfhet_trlwe_gsw_linear_extract (include/mosfhet_compat.h) on host structs: N = 2048, gadget l = 4, Bg_bit = 9, noise 2^-44.
 * Every input packs 32 four-bit values at coefficients 0 .. 31 (slots of 1/16); a weight is the TRGSW sample of mosfhet_polylinear_dot_layout of 32 values in [-8, 8):
 * 2l zero TRLWE samples plus mu 2^(64 - (i + 1) Bg_bit) on the row's own component.
 *   - at rows_in = 1 (2 output rows, 2 batch elements) mosfhet_trlwe_gsw_linear equals, word for word, the drop-in layer's trgsw_to_DFT, trgsw_mul_trlwe_DFT and
 *     trlwe_from_DFT (+ the bias on component b), with and without bias, and mosfhet_trlwe_gsw_linear_extract at idx 0 and 5 equals trlwe_extract_tlwe of those;
 *   - at rows_in = 2 coefficient 0 of output (b, j) decrypts to the inner product of the row's 64 weights with the 64 packed values within half a slot (2^59), through
 *     both faces.
 * Run by tests/test_trlwe_gsw_linear.py; exit status = number of failed checks.
 */
#include <math.h>
#include <mosfhet.h>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __func__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

enum { N = 2048, L = 4, BG_BIT = 9, ROWS_OUT = 2, ROWS_IN = 2, COUNT = 2, PER = 32 };

static double dist(Torus a, Torus b) { return fabs((double)(int64_t)(a - b)); }

static int differs(TRLWE x, TRLWE y) { return memcmp(x->a[0]->coeffs, y->a[0]->coeffs, sizeof(Torus) * N) != 0 || memcmp(x->b->coeffs, y->b->coeffs, sizeof(Torus) * N) != 0; }

/* TRGSW(mu): rows 0 .. l - 1 carry mu g_i on component a, rows l .. 2l - 1 on component b */
static TRGSW trgsw_of_polynomial(const int64_t *mu, TRLWE_Key key, TorusPolynomial zero) {
  TRGSW g = trgsw_alloc_new_sample(L, BG_BIT, 1, N);
  for (int c = 0; c < 2; c++)
    for (int i = 0; i < L; i++) {
      TRLWE row = g->samples[c * L + i];
      trlwe_sample(row, zero, key);
      Torus *dst = c ? row->b->coeffs : row->a[0]->coeffs;
      for (int x = 0; x < N; x++) dst[x] += (Torus)mu[x] << (64 - (i + 1) * BG_BIT);
    }
  return g;
}

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_seed(0x47535731);
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, 1, 5.684341886080802e-14);            /* 2^-44 */
  TLWE_Key extracted = tlwe_alloc_key(N, 5.684341886080802e-14);
  trlwe_extract_tlwe_key(extracted, rlwe_key);
  TorusPolynomial m = polynomial_new_torus_polynomial(N), zero = polynomial_new_torus_polynomial(N);
  memset(zero->coeffs, 0, sizeof(Torus) * N);

  /* the packed inputs and their cleartext values */
  int x[COUNT][ROWS_IN][PER];
  TRLWE in[COUNT * ROWS_IN];
  for (int b = 0; b < COUNT; b++)
    for (int i = 0; i < ROWS_IN; i++) {
      memset(m->coeffs, 0, sizeof(Torus) * N);
      for (int c = 0; c < PER; c++) {
        x[b][i][c] = (b * 5 + i * 11 + c * 7 + 3) % 16;
        m->coeffs[c] = (Torus)x[b][i][c] << 60;
      }
      in[b * ROWS_IN + i] = trlwe_new_sample(m, rlwe_key);
    }

  /* the weights: W [ROWS_OUT][ROWS_IN] TRGSW samples of dot_layout polynomials, bias [ROWS_OUT][N] */
  static int64_t poly[N];
  static Torus bias[ROWS_OUT][N];
  int64_t w[ROWS_OUT][ROWS_IN][PER];
  TRGSW W[ROWS_OUT * ROWS_IN];
  for (int j = 0; j < ROWS_OUT; j++)
    for (int i = 0; i < ROWS_IN; i++) {
      for (int c = 0; c < PER; c++) w[j][i][c] = (j * 3 + i * 5 + c * 2) % 16 - 8;
      CHECK(mosfhet_polylinear_dot_layout(poly, w[j][i], PER, N, 1) == 0, "dot_layout");
      W[j * ROWS_IN + i] = trgsw_of_polynomial(poly, rlwe_key, zero);
    }
  for (int j = 0; j < ROWS_OUT; j++)
    for (int c = 0; c < N; c++) bias[j][c] = (Torus)((j + 1 + c) % 16) << 60;

  /* part 1, rows_in = 1: the layer of the weights W[j][0] on the inputs in[b][0] against the drop-in layer's external product */
  TRGSW W1[ROWS_OUT];
  TRLWE in1[COUNT], want[COUNT * ROWS_OUT], want_b[COUNT * ROWS_OUT], got[COUNT * ROWS_OUT];
  TRGSW_DFT w_dft = trgsw_alloc_new_DFT_sample(L, BG_BIT, 1, N);
  TRLWE_DFT acc = trlwe_alloc_new_DFT_sample(1, N);
  for (int j = 0; j < ROWS_OUT; j++) W1[j] = W[j * ROWS_IN];
  for (int b = 0; b < COUNT; b++) in1[b] = in[b * ROWS_IN];
  for (int j = 0; j < ROWS_OUT; j++) {
    trgsw_to_DFT(w_dft, W1[j]);
    for (int b = 0; b < COUNT; b++) {
      const int o = b * ROWS_OUT + j;
      want[o] = trlwe_alloc_new_sample(1, N);
      want_b[o] = trlwe_alloc_new_sample(1, N);
      got[o] = trlwe_alloc_new_sample(1, N);
      trgsw_mul_trlwe_DFT(acc, in1[b], w_dft);
      trlwe_from_DFT(want[o], acc);
      trlwe_copy(want_b[o], want[o]);
      for (int c = 0; c < N; c++) want_b[o]->b->coeffs[c] += bias[j][c];
    }
  }
  int differ = 0, differ_b = 0;
  mosfhet_trlwe_gsw_linear(got, in1, W1, NULL, ROWS_OUT, 1, COUNT);
  for (int o = 0; o < COUNT * ROWS_OUT; o++) differ += differs(got[o], want[o]);
  mosfhet_trlwe_gsw_linear(got, in1, W1, &bias[0][0], ROWS_OUT, 1, COUNT);
  for (int o = 0; o < COUNT * ROWS_OUT; o++) differ_b += differs(got[o], want_b[o]);
  printf("trlwe_gsw_linear at rows_in = 1: %d of %d outputs differ from trgsw_mul_trlwe_DFT + trlwe_from_DFT without bias, %d with\n", differ, COUNT * ROWS_OUT, differ_b);
  CHECK(differ == 0, "%d outputs of mosfhet_trlwe_gsw_linear differ from trgsw_mul_trlwe_DFT + trlwe_from_DFT", differ);
  CHECK(differ_b == 0, "%d outputs of mosfhet_trlwe_gsw_linear with bias differ", differ_b);
  TLWE *ext = tlwe_alloc_sample_array(COUNT * ROWS_OUT, N);
  TLWE one = tlwe_alloc_sample(N);
  const int idxs[2] = {0, 5};
  for (int q = 0; q < 2; q++) {
    differ = 0;
    mosfhet_trlwe_gsw_linear_extract(ext, in1, W1, &bias[0][0], ROWS_OUT, 1, COUNT, idxs[q]);
    for (int o = 0; o < COUNT * ROWS_OUT; o++) {
      trlwe_extract_tlwe(one, want_b[o], idxs[q]);
      differ += memcmp(ext[o]->a, one->a, sizeof(Torus) * N) != 0 || ext[o]->b != one->b;
    }
    CHECK(differ == 0, "%d outputs of mosfhet_trlwe_gsw_linear_extract at idx %d differ from trlwe_extract_tlwe of the product", differ, idxs[q]);
  }

  /* part 2, rows_in = 2: what the layer decrypts to, through both faces */
  double worst = 0, worst_ext = 0;
  mosfhet_trlwe_gsw_linear(got, in, W, &bias[0][0], ROWS_OUT, ROWS_IN, COUNT);
  mosfhet_trlwe_gsw_linear_extract(ext, in, W, &bias[0][0], ROWS_OUT, ROWS_IN, COUNT, 0);
  for (int o = 0; o < COUNT * ROWS_OUT; o++) {
    const int b = o / ROWS_OUT, j = o % ROWS_OUT;
    int sum = j + 1;                                        /* bias[j][0] */
    for (int i = 0; i < ROWS_IN; i++)
      for (int c = 0; c < PER; c++) sum += (int)w[j][i][c] * x[b][i][c];
    const Torus target = (Torus)(int64_t)sum << 60;
    trlwe_phase(m, got[o], rlwe_key);
    const double e = dist(m->coeffs[0], target), e_ext = dist(tlwe_phase(ext[o], extracted), target);
    if (e > worst) worst = e;
    if (e_ext > worst_ext) worst_ext = e_ext;
  }
  printf("trlwe_gsw_linear at rows_in = 2: worst distance of the inner products from bias + sum w x: 2^%.1f, extracted 2^%.1f (half a slot: 2^59)\n",
         log2(worst > 1 ? worst : 1), log2(worst_ext > 1 ? worst_ext : 1));
  CHECK(worst < 0x1p59, "an inner product does not decrypt (2^%.1f)", log2(worst > 1 ? worst : 1));
  CHECK(worst_ext < 0x1p59, "an extracted inner product does not decrypt (2^%.1f)", log2(worst_ext > 1 ? worst_ext : 1));

  if (!failures) printf("trlwe_gsw_linear ok\n");
  return failures;
}
