/*
 * GPU test of mosfhet_trlwe_automaton (include/mosfhet_compat.h): 3 inputs with words of STEPS encrypted bits at SET_1's ring and gadget (N = 1024, l = 2,
 * Bg = 2^8; 2-bit messages on every coefficient), the 3-state machine "ones-counter in the exponent + parity pair":
 *   state 0: stays, a 1 multiplies by X; state 1 (even) and state 2 (odd) swap on a 1.
 *   - every state of V_0 equals, word for word, the backward chain of CMUXes written against include/mosfhet.h (trlwe_mul_by_xai / trlwe_sub /
 *     trgsw_mul_trlwe_DFT / trlwe_from_DFT / trlwe_add), per input and with one shared initial vector; start = 2 gives that row; a batch of one the same words;
 *   - every state decrypts: state 0 to X^ones m_0, states 1 and 2 to m_1 / m_2, swapped on odd parity; the initial vector is left as it was.
 * Run by tests/test_trlwe_automaton.py; exit status = number of failed checks.
 */
#include <math.h>
#include <mosfhet.h>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __func__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

enum { N = 1024, k = 1, l = 2, Bg_bit = 8, STEPS = 5, STATES = 3, PREC = 2, COUNT = 3 };

static const int next0[STATES] = {0, 1, 2}, next1[STATES] = {0, 2, 1}, rot0[STATES] = {0, 0, 0}, rot1[STATES] = {1, 0, 0};

static uint64_t tdist(Torus a, Torus b) { int64_t d = (int64_t)(a - b); return (uint64_t)(d < 0 ? -d : d); }
static int same_trlwe(TRLWE a, TRLWE b) {
  const size_t bytes = sizeof(Torus) * (size_t)N;
  return !memcmp(a->a[0]->coeffs, b->a[0]->coeffs, bytes) && !memcmp(a->b->coeffs, b->b->coeffs, bytes);
}

/* out = in1 + selector (.) (in2 - in1) */
static void cmux(TRLWE out, TRLWE in1, TRLWE in2, TRGSW_DFT selector) {
  TRLWE_DFT tmp = trlwe_alloc_new_DFT_sample(k, N);
  TRLWE tmp2 = trlwe_alloc_new_sample(k, N);
  trlwe_sub(tmp2, in2, in1);
  trgsw_mul_trlwe_DFT(tmp, tmp2, selector);
  trlwe_from_DFT(tmp2, tmp);
  trlwe_add(out, tmp2, in1);
  free_trlwe(tmp);
  free_trlwe(tmp2);
}

/* V <- V_0 of the machine over `word`, backwards from V = the initial vector */
static void run(TRLWE *V, TRGSW_DFT *word) {
  TRLWE *W = trlwe_alloc_new_sample_array(STATES, k, N);
  TRLWE r0 = trlwe_alloc_new_sample(k, N), r1 = trlwe_alloc_new_sample(k, N);
  for (int t = STEPS - 1; t >= 0; t--) {
    for (int q = 0; q < STATES; q++) {
      trlwe_mul_by_xai(r0, V[next0[q]], rot0[q]);
      trlwe_mul_by_xai(r1, V[next1[q]], rot1[q]);
      cmux(W[q], r0, r1, word[t]);
    }
    for (int q = 0; q < STATES; q++) trlwe_copy(V[q], W[q]);
  }
  free_trlwe(r0);
  free_trlwe(r1);
  free_trlwe_array(W, STATES);
}

static uint64_t worst = 0;
static void check_decrypts(TRLWE c, const Torus *msg, int ones, TRLWE_Key key, int b, int q) {
  TorusPolynomial ph = polynomial_new_torus_polynomial(N);
  trlwe_phase(ph, c, key);
  uint64_t w = 0;
  for (int j = 0; j < N; j++) {
    const int src = j - ones;                       /* coefficient j of X^ones m (ones < N) */
    const Torus want = src < 0 ? (Torus)0 - msg[src + N] : msg[src];
    const uint64_t d = tdist(ph->coeffs[j], want);
    if (d > w) w = d;
  }
  if (w > worst) worst = w;
  CHECK(w < (1ULL << (64 - PREC - 1)), "input %d, state %d: 2^%.1f from the message", b, q, log2((double)w + 1.0));
  free_polynomial(ph);
}

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_seed(0x4155544F);
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, k, 2.9802322387695312e-08);   /* 2^-25 */
  TRGSW_Key key = trgsw_new_key(rlwe_key, l, Bg_bit);

  static Torus msg[COUNT][STATES][N];
  const int bits[COUNT] = {0x00, 0x1F, 0x0D};       /* the words, symbol t = bit t: 0, 5 and 3 ones */
  uint64_t x = 0x9E3779B97F4A7C15ULL;
  TRLWE *init[COUNT], *before[COUNT], *want[COUNT], *out[COUNT], *one[COUNT];
  TRGSW_DFT *word[COUNT];
  TorusPolynomial m = polynomial_new_torus_polynomial(N);
  TRGSW tmp = trgsw_alloc_new_sample(l, Bg_bit, k, N);
  for (int b = 0; b < COUNT; b++) {
    init[b] = trlwe_alloc_new_sample_array(STATES, k, N);
    before[b] = trlwe_alloc_new_sample_array(STATES, k, N);
    want[b] = trlwe_alloc_new_sample_array(STATES, k, N);
    out[b] = trlwe_alloc_new_sample_array(STATES, k, N);
    one[b] = trlwe_alloc_new_sample_array(1, k, N);
    for (int q = 0; q < STATES; q++) {
      for (int j = 0; j < N; j++) {
        x = x * 6364136223846793005ULL + 1442695040888963407ULL;
        msg[b][q][j] = m->coeffs[j] = (Torus)((x >> 40) & ((1u << PREC) - 1)) << (64 - PREC);
      }
      trlwe_sample(init[b][q], m, rlwe_key);
      trlwe_copy(before[b][q], init[b][q]);
      trlwe_copy(want[b][q], init[b][q]);
    }
    word[b] = trgsw_alloc_new_DFT_sample_array(STEPS, l, Bg_bit, k, N);
    for (int t = 0; t < STEPS; t++) {
      trgsw_monomial_sample(tmp, (bits[b] >> t) & 1, 0, key);
      trgsw_to_DFT(word[b][t], tmp);
    }
  }

  /* every state, every input its own initial vector */
  mosfhet_trlwe_automaton(out, word, STEPS, init, 0, next0, next1, rot0, rot1, STATES, 1, -1, COUNT);
  int differ = 0;
  for (int b = 0; b < COUNT; b++) {
    run(want[b], word[b]);
    const int ones = __builtin_popcount(bits[b]);
    for (int q = 0; q < STATES; q++) {
      differ += !same_trlwe(out[b][q], want[b][q]);
      CHECK(same_trlwe(init[b][q], before[b][q]), "the call changed state %d of input %d's initial vector", q, b);
      const int from = q == 0 ? 0 : (ones & 1) ? 3 - q : q;      /* the state the machine started in q ends in */
      check_decrypts(out[b][q], msg[b][from], q == 0 ? ones : 0, rlwe_key, b, q);
    }
  }
  CHECK(differ == 0, "%d of %d states differ from the CMUX chain", differ, COUNT * STATES);
  printf("all states: %d of %d differ from the CMUX chain as words; worst distance from the message 2^%.1f (bound 2^%d)\n", differ, COUNT * STATES,
         log2((double)worst + 1.0), 64 - PREC - 1);

  /* one state: that row */
  mosfhet_trlwe_automaton(one, word, STEPS, init, 0, next0, next1, rot0, rot1, STATES, 1, 2, COUNT);
  for (int b = 0; b < COUNT; b++) CHECK(same_trlwe(one[b][0], want[b][2]), "start = 2: input %d differs from state 2 of the full result", b);

  /* a batch of one: the same words */
  mosfhet_trlwe_automaton(out + 1, word + 1, STEPS, init + 1, 0, next0, next1, rot0, rot1, STATES, 1, -1, 1);
  for (int q = 0; q < STATES; q++) CHECK(same_trlwe(out[1][q], want[1][q]), "a batch of one differs in state %d", q);

  /* one initial vector for the whole batch: input 1's */
  mosfhet_trlwe_automaton(out, word, STEPS, init + 1, 1, next0, next1, rot0, rot1, STATES, 1, -1, COUNT);
  for (int b = 0; b < COUNT; b++) {
    for (int q = 0; q < STATES; q++) trlwe_copy(want[b][q], init[1][q]);
    run(want[b], word[b]);
    for (int q = 0; q < STATES; q++) CHECK(same_trlwe(out[b][q], want[b][q]), "shared initial vector: state %d of input %d differs from the CMUX chain", q, b);
  }

  for (int b = 0; b < COUNT; b++) {
    free_trgsw_array(word[b], STEPS);
    free_trlwe_array(init[b], STATES);
    free_trlwe_array(before[b], STATES);
    free_trlwe_array(want[b], STATES);
    free_trlwe_array(out[b], STATES);
    free_trlwe_array(one[b], 1);
  }
  free_trgsw(tmp);
  free_polynomial(m);
  if (!failures) printf("trlwe_automaton ok\n");
  return failures;
}
