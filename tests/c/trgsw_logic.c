/*
 * GPU test of mosfhet_trgsw_logic (include/mosfhet_compat.h) at the lvl2 ring and gadget (N = 2048, l = 4, Bg = 2^9, sigma = 2^-44), the gadget at which a gate's
 * output is usable:
 *   - one AND gate on 2 batch elements equals the drop-in layer's own trgsw_mul_DFT2 word for word.  trgsw_mul_DFT2 leaves the product's accumulators in the DFT
 *     domain, the gate leaves F(G(accumulators)) -- a selector like any other -- so trgsw_mul_DFT2's result goes through trgsw_from_DFT and trgsw_to_DFT first, and
 *     both sides are compared as the torus words trgsw_from_DFT gives;
 *   - the 4-bit incrementer (s_0 = NOT a_0; s_i = c_i XOR a_i, c_{i+1} = c_i AND a_i, the carry in x) on the values {0, 5, 7, 15, 11} in one batch: the external
 *     product of every sum selector with a sample of four-bit messages decrypts to bit x message within 2^57.
 * Run by tests/test_trgsw_logic.py; exit status = number of failed checks.
 */
#include <math.h>
#include <mosfhet.h>
#include <mosfhet_hip.h>   /* MOSFHET_HIP_SEL_* */

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __func__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

enum { N = 2048, k = 1, l = 4, Bg_bit = 9, BITS = 4, COUNT = 5, INC_GATES = 2 * BITS - 2 };

static uint64_t tdist(Torus a, Torus b) { int64_t d = (int64_t)(a - b); return (uint64_t)(d < 0 ? -d : d); }

static int same_words(TRGSW a, TRGSW b) {
  const size_t bytes = sizeof(Torus) * (size_t)N;
  for (int r = 0; r < 2 * l; r++)
    if (memcmp(a->samples[r]->a[0]->coeffs, b->samples[r]->a[0]->coeffs, bytes) || memcmp(a->samples[r]->b->coeffs, b->samples[r]->b->coeffs, bytes)) return 0;
  return 1;
}

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_seed(0x5E110);
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, k, 5.684341886080802e-14);   /* 2^-44 */
  TRGSW_Key key = trgsw_new_key(rlwe_key, l, Bg_bit);
  TRGSW tmp = trgsw_alloc_new_sample(l, Bg_bit, k, N), got_w = trgsw_alloc_new_sample(l, Bg_bit, k, N), want_w = trgsw_alloc_new_sample(l, Bg_bit, k, N);

  /* one AND gate against trgsw_mul_DFT2 */
  {
    const int and_gate[4] = {MOSFHET_HIP_SEL_AND, 0, 1, -1};
    TRGSW_DFT *in[2], *out[2];
    for (int b = 0; b < 2; b++) {
      in[b] = trgsw_alloc_new_DFT_sample_array(2, l, Bg_bit, k, N);
      out[b] = trgsw_alloc_new_DFT_sample_array(1, l, Bg_bit, k, N);
      for (int i = 0; i < 2; i++) {
        trgsw_monomial_sample(tmp, (b + i) & 1, 0, key);
        trgsw_to_DFT(in[b][i], tmp);
      }
    }
    mosfhet_trgsw_logic(out, in, and_gate, 1, 2, 2);
    TRGSW_DFT prod = trgsw_alloc_new_DFT_sample(l, Bg_bit, k, N), want = trgsw_alloc_new_DFT_sample(l, Bg_bit, k, N);
    for (int b = 0; b < 2; b++) {
      trgsw_mul_DFT2(prod, in[b][0], in[b][1]);
      trgsw_from_DFT(tmp, prod);
      trgsw_to_DFT(want, tmp);
      trgsw_from_DFT(want_w, want);
      trgsw_from_DFT(got_w, out[b][0]);
      CHECK(same_words(got_w, want_w), "batch element %d: the AND gate differs from trgsw_mul_DFT2", b);
    }
    printf("one AND gate against trgsw_mul_DFT2: %d failures so far\n", failures);
    free_trgsw(prod);
    free_trgsw(want);
    for (int b = 0; b < 2; b++) {
      free_trgsw_array(in[b], 2);
      free_trgsw_array(out[b], 1);
    }
  }

  /* the incrementer */
  {
    int gates[INC_GATES][4], sums[BITS], n = 0, carry = 0;
    gates[n][0] = MOSFHET_HIP_SEL_NOT; gates[n][1] = 0; gates[n][2] = -1; gates[n][3] = -1;
    sums[0] = n++;
    for (int i = 1; i < BITS; i++) {
      gates[n][0] = MOSFHET_HIP_SEL_XOR; gates[n][1] = carry; gates[n][2] = i; gates[n][3] = -1;
      sums[i] = n++;
      if (i + 1 < BITS) {
        gates[n][0] = MOSFHET_HIP_SEL_AND; gates[n][1] = carry; gates[n][2] = i; gates[n][3] = -1;
        carry = BITS + n++;
      }
    }
    CHECK(n == INC_GATES, "%d gates", n);
    const int values[COUNT] = {0, 5, 7, 15, 11};
    TRGSW_DFT *in[COUNT], *out[COUNT];
    for (int b = 0; b < COUNT; b++) {
      in[b] = trgsw_alloc_new_DFT_sample_array(BITS, l, Bg_bit, k, N);
      out[b] = trgsw_alloc_new_DFT_sample_array(INC_GATES, l, Bg_bit, k, N);
      for (int i = 0; i < BITS; i++) {
        trgsw_monomial_sample(tmp, (values[b] >> i) & 1, 0, key);
        trgsw_to_DFT(in[b][i], tmp);
      }
    }
    mosfhet_trgsw_logic(out, in, &gates[0][0], INC_GATES, BITS, COUNT);
    static Torus msg[N];
    TorusPolynomial m = polynomial_new_torus_polynomial(N), ph = polynomial_new_torus_polynomial(N);
    uint64_t x = 0x9E3779B97F4A7C15ULL, worst = 0;
    for (int j = 0; j < N; j++) {
      x = x * 6364136223846793005ULL + 1442695040888963407ULL;
      msg[j] = m->coeffs[j] = (Torus)((x >> 40) & 15) << 60;
    }
    TRLWE probe = trlwe_alloc_new_sample(k, N), res = trlwe_alloc_new_sample(k, N);
    TRLWE_DFT acc = trlwe_alloc_new_DFT_sample(k, N);
    trlwe_sample(probe, m, rlwe_key);
    for (int b = 0; b < COUNT; b++)
      for (int i = 0; i < BITS; i++) {
        const int bit = (((values[b] + 1) & 15) >> i) & 1;
        trgsw_mul_trlwe_DFT(acc, probe, out[b][sums[i]]);
        trlwe_from_DFT(res, acc);
        trlwe_phase(ph, res, rlwe_key);
        uint64_t w = 0;
        for (int j = 0; j < N; j++) {
          const uint64_t d = tdist(ph->coeffs[j], bit ? msg[j] : 0);
          if (d > w) w = d;
        }
        if (w > worst) worst = w;
        CHECK(w < (1ULL << 57), "%d + 1, sum bit %d: 2^%.1f from bit x message", values[b], i, log2((double)w + 1.0));
      }
    printf("incrementer: worst distance from bit x message 2^%.1f (bound 2^57)\n", log2((double)worst + 1.0));
    free_trlwe(probe);
    free_trlwe(res);
    free_trlwe(acc);
    free_polynomial(m);
    free_polynomial(ph);
    for (int b = 0; b < COUNT; b++) {
      free_trgsw_array(in[b], BITS);
      free_trgsw_array(out[b], INC_GATES);
    }
  }

  free_trgsw(tmp);
  free_trgsw(got_w);
  free_trgsw(want_w);
  if (!failures) printf("trgsw_logic ok\n");
  return failures;
}
