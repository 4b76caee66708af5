/*
 * GPU test of mosfhet_trlwe_linear, mosfhet_trlwe_linear_extract and mosfhet_polylinear_dot_layout (include/mosfhet_compat.h) on host structs: N = 1024, a 2 x 2 layer
 * of weight polynomials over 2 batch elements.  Every input packs 16 four-bit values at coefficients 0 .. 15 (slots of 1/16); row j's weight polynomials are
 * mosfhet_polylinear_dot_layout of weights in [-3, 3], so coefficient 0 of output (b, j) is the inner product of the row's 32 weights with the 32 packed values.
 *   - mosfhet_trlwe_linear equals, word for word, the drop-in layer's loop trlwe_to_DFT, trlwe_DFT_mul_by_polynomial / trlwe_DFT_mul_addto_by_polynomial,
 *     trlwe_from_DFT (+ the bias on component b), with and without bias;
 *   - mosfhet_trlwe_linear_extract at idx 0 and 5 equals trlwe_extract_tlwe of those;
 *   - the sample extracted at 0 decrypts to bias + sum w x mod 16 within half a slot (2^59);
 *   - mosfhet_polylinear_dot_layout refuses per * stride > N.
 * Run by tests/test_trlwe_linear.py; exit status = number of failed checks.
 */
#include <math.h>
#include <mosfhet.h>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __func__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

enum { N = 1024, ROWS_OUT = 2, ROWS_IN = 2, COUNT = 2, PER = 16 };

static double dist(Torus a, Torus b) { return fabs((double)(int64_t)(a - b)); }

static int differs(TRLWE x, TRLWE y) { return memcmp(x->a[0]->coeffs, y->a[0]->coeffs, sizeof(Torus) * N) != 0 || memcmp(x->b->coeffs, y->b->coeffs, sizeof(Torus) * N) != 0; }

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_seed(0x504C494E);
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, 1, 9.094947017729282e-13);            /* 2^-40 */
  TLWE_Key extracted = tlwe_alloc_key(N, 9.094947017729282e-13);
  trlwe_extract_tlwe_key(extracted, rlwe_key);

  /* the packed inputs and their cleartext values */
  int x[COUNT][ROWS_IN][PER];
  TRLWE in[COUNT * ROWS_IN];
  TorusPolynomial m = polynomial_new_torus_polynomial(N);
  for (int b = 0; b < COUNT; b++)
    for (int i = 0; i < ROWS_IN; i++) {
      memset(m->coeffs, 0, sizeof(Torus) * N);
      for (int c = 0; c < PER; c++) {
        x[b][i][c] = (b * 5 + i * 11 + c * 7 + 3) % 16;
        m->coeffs[c] = (Torus)x[b][i][c] << 60;
      }
      in[b * ROWS_IN + i] = trlwe_new_sample(m, rlwe_key);
    }

  /* the weights: W [ROWS_OUT][ROWS_IN][N] through dot_layout, bias [ROWS_OUT][N] */
  static int64_t W[ROWS_OUT][ROWS_IN][N];
  static Torus bias[ROWS_OUT][N];
  int64_t w[ROWS_OUT][ROWS_IN][PER];
  for (int j = 0; j < ROWS_OUT; j++)
    for (int i = 0; i < ROWS_IN; i++) {
      for (int c = 0; c < PER; c++) w[j][i][c] = (j * 3 + i * 5 + c * 2) % 7 - 3;
      CHECK(mosfhet_polylinear_dot_layout(W[j][i], w[j][i], PER, N, 1) == 0, "dot_layout");
    }
  for (int j = 0; j < ROWS_OUT; j++)
    for (int c = 0; c < N; c++) bias[j][c] = (Torus)((j + 1 + c) % 16) << 60;
  int64_t scratch[N];
  CHECK(mosfhet_polylinear_dot_layout(scratch, w[0][0], PER, N, N / PER + 1) == -1, "dot_layout accepted per * stride > N");
  CHECK(mosfhet_polylinear_dot_layout(scratch, w[0][0], PER, N, N / PER) == 0 && scratch[0] == w[0][0][0] && scratch[N - N / PER] == -w[0][0][1] && scratch[1] == 0,
        "dot_layout at stride N / per");

  /* the loop of the drop-in layer */
  TRLWE want[COUNT * ROWS_OUT], want_b[COUNT * ROWS_OUT], got[COUNT * ROWS_OUT];
  TRLWE_DFT x_dft[ROWS_IN], acc = trlwe_alloc_new_DFT_sample(1, N);
  DFT_Polynomial w_dft[ROWS_OUT][ROWS_IN];
  for (int i = 0; i < ROWS_IN; i++) x_dft[i] = trlwe_alloc_new_DFT_sample(1, N);
  for (int j = 0; j < ROWS_OUT; j++)
    for (int i = 0; i < ROWS_IN; i++) {
      for (int c = 0; c < N; c++) m->coeffs[c] = (Torus)W[j][i][c];
      w_dft[j][i] = polynomial_new_DFT_polynomial(N);
      polynomial_torus_to_DFT(w_dft[j][i], m);
    }
  for (int b = 0; b < COUNT; b++) {
    for (int i = 0; i < ROWS_IN; i++) trlwe_to_DFT(x_dft[i], in[b * ROWS_IN + i]);
    for (int j = 0; j < ROWS_OUT; j++) {
      const int o = b * ROWS_OUT + j;
      trlwe_DFT_mul_by_polynomial(acc, x_dft[0], w_dft[j][0]);
      for (int i = 1; i < ROWS_IN; i++) trlwe_DFT_mul_addto_by_polynomial(acc, x_dft[i], w_dft[j][i]);
      want[o] = trlwe_alloc_new_sample(1, N);
      want_b[o] = trlwe_alloc_new_sample(1, N);
      got[o] = trlwe_alloc_new_sample(1, N);
      trlwe_from_DFT(want[o], acc);
      trlwe_copy(want_b[o], want[o]);
      for (int c = 0; c < N; c++) want_b[o]->b->coeffs[c] += bias[j][c];
    }
  }

  /* part 1: the TRLWE face */
  int differ = 0, differ_b = 0;
  mosfhet_trlwe_linear(got, in, &W[0][0][0], NULL, ROWS_OUT, ROWS_IN, COUNT);
  for (int o = 0; o < COUNT * ROWS_OUT; o++) differ += differs(got[o], want[o]);
  mosfhet_trlwe_linear(got, in, &W[0][0][0], &bias[0][0], ROWS_OUT, ROWS_IN, COUNT);
  for (int o = 0; o < COUNT * ROWS_OUT; o++) differ_b += differs(got[o], want_b[o]);
  printf("trlwe_linear: %d of %d outputs differ from the loop without bias, %d with\n", differ, COUNT * ROWS_OUT, differ_b);
  CHECK(differ == 0, "%d outputs of mosfhet_trlwe_linear differ from the loop of trlwe_DFT_mul_addto_by_polynomial", differ);
  CHECK(differ_b == 0, "%d outputs of mosfhet_trlwe_linear with bias differ from the loop", differ_b);

  /* part 2: the extracting face, and what it decrypts to */
  TLWE *ext = tlwe_alloc_sample_array(COUNT * ROWS_OUT, N);
  TLWE one = tlwe_alloc_sample(N);
  const int idxs[2] = {0, 5};
  double worst = 0;
  for (int q = 0; q < 2; q++) {
    differ = 0;
    mosfhet_trlwe_linear_extract(ext, in, &W[0][0][0], &bias[0][0], ROWS_OUT, ROWS_IN, COUNT, idxs[q]);
    for (int o = 0; o < COUNT * ROWS_OUT; o++) {
      trlwe_extract_tlwe(one, want_b[o], idxs[q]);
      differ += memcmp(ext[o]->a, one->a, sizeof(Torus) * N) != 0 || ext[o]->b != one->b;
      if (idxs[q] == 0) {
        const int b = o / ROWS_OUT, j = o % ROWS_OUT;
        int sum = j + 1;                                        /* bias[j][0] */
        for (int i = 0; i < ROWS_IN; i++)
          for (int c = 0; c < PER; c++) sum += (int)w[j][i][c] * x[b][i][c];
        const double e = dist(tlwe_phase(ext[o], extracted), (Torus)(int64_t)sum << 60);
        if (e > worst) worst = e;
      }
    }
    CHECK(differ == 0, "%d outputs of mosfhet_trlwe_linear_extract at idx %d differ from trlwe_extract_tlwe of the loop", differ, idxs[q]);
  }
  printf("trlwe_linear_extract: worst distance of the inner products from bias + sum w x: 2^%.1f (half a slot: 2^59)\n", log2(worst > 1 ? worst : 1));
  CHECK(worst < 0x1p59, "an inner product does not decrypt (2^%.1f)", log2(worst > 1 ? worst : 1));

  if (!failures) printf("trlwe_linear ok\n");
  return failures;
}
