/*
 * GPU test of mosfhet_eval_LUT_inputs (include/mosfhet_compat.h): a shared 2^13-entry table evaluated on 8 independent inputs, each encrypted bit by bit as
 * TRGSW_DFT samples, at the reference application's ring and gadget (N = 2048, l = 1, Bg = 2^23; 4 output bits).
 *   - word for word equal to the reference's own eval_LUT loop (applications/leveled_lut/vertical_packing.c:24-52) written against include/mosfhet.h:
 *     trlwe_sub / trgsw_mul_trlwe_DFT / trlwe_from_DFT / trlwe_add per tree node, blind_rotate with a[i] = int2torus(2N - 2^i), trlwe_extract_tlwe, one input
 *     at a time on a copy of the table (that loop destroys its table);
 *   - every output decrypts to the table entry of its input;
 *   - LUT is left as it was.
 * Run by tests/test_leveled_lut.py; exit status = number of failed checks.
 */
#include <math.h>
#include <mosfhet.h>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __func__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static int same_tlwe(TLWE a, TLWE b) { return a->b == b->b && !memcmp(a->a, b->a, sizeof(Torus) * (size_t)a->n); }
static uint64_t tdist(Torus a, Torus b) { int64_t d = (int64_t)(a - b); return (uint64_t)(d < 0 ? -d : d); }
static int same_trlwe(TRLWE a, TRLWE b) {
  const size_t bytes = sizeof(Torus) * (size_t)a->b->N;
  return !memcmp(a->a[0]->coeffs, b->a[0]->coeffs, bytes) && !memcmp(a->b->coeffs, b->b->coeffs, bytes);
}

enum { N = 2048, LOG_N = 11, k = 1, l = 1, Bg_bit = 23, SIZE = 13, PREC = 4, COUNT = 8, N_LUTS = 1 << (SIZE - LOG_N) };

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

/* destroys `table` */
static void eval_one(TLWE output, TRGSW_DFT *input, int size, TRLWE *table) {
  for (int i = 0; i < size - LOG_N; i++) {
    const int half = 1 << (size - LOG_N - i - 1);
    for (int j = 0; j < half; j++) cmux(table[j], table[j], table[j + half], input[size - i - 1]);
  }
  if (size > LOG_N) size = LOG_N;
  Torus a[32];
  for (int i = 0; i < size; i++) a[i] = int2torus((uint64_t)(2 * N - (1 << i)), LOG_N + 1);
  blind_rotate(table[0], a, input, size);
  trlwe_extract_tlwe(output, table[0], 0);
}

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_seed(0x4C5554);
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, k, 2.220446049250313e-16);   /* 2^-52 */
  TRGSW_Key key = trgsw_new_key(rlwe_key, l, Bg_bit);
  TLWE_Key out_key = tlwe_alloc_key(N, rlwe_key->sigma);
  trlwe_extract_tlwe_key(out_key, rlwe_key);

  /* the table: 2^13 entries of 4 bits, 4 trivial TRLWEs */
  static Torus entries[1 << SIZE];
  uint64_t x = 0x9E3779B97F4A7C15ULL;
  for (int i = 0; i < (1 << SIZE); i++) {
    x = x * 6364136223846793005ULL + 1442695040888963407ULL;
    entries[i] = (Torus)((x >> 40) & ((1u << PREC) - 1)) << (64 - PREC);
  }
  TRLWE *LUT = trlwe_alloc_new_sample_array(N_LUTS, k, N), *before = trlwe_alloc_new_sample_array(N_LUTS, k, N), *work = trlwe_alloc_new_sample_array(N_LUTS, k, N);
  for (int j = 0; j < N_LUTS; j++) {
    trlwe_torus_packing(LUT[j], entries + (size_t)j * N, N);
    trlwe_copy(before[j], LUT[j]);
  }

  /* the inputs, bit by bit (vertical_packing.c:8-22) */
  int m[COUNT];
  TRGSW_DFT *inputs[COUNT];
  TRGSW tmp = trgsw_alloc_new_sample(l, Bg_bit, k, N);
  for (int b = 0; b < COUNT; b++) {
    x = x * 6364136223846793005ULL + 1442695040888963407ULL;
    m[b] = (int)((x >> 33) & ((1u << SIZE) - 1));
    inputs[b] = trgsw_alloc_new_DFT_sample_array(SIZE, l, Bg_bit, k, N);
    for (int i = 0; i < SIZE; i++) {
      trgsw_monomial_sample(tmp, (m[b] >> i) & 1, 0, key);
      trgsw_to_DFT(inputs[b][i], tmp);
    }
  }

  TLWE *got = tlwe_alloc_sample_array(COUNT, N), *want = tlwe_alloc_sample_array(COUNT, N);
  mosfhet_eval_LUT_inputs(got, inputs, SIZE, LUT, COUNT);
  int changed = 0;
  for (int j = 0; j < N_LUTS; j++) changed += !same_trlwe(LUT[j], before[j]);
  CHECK(changed == 0, "mosfhet_eval_LUT_inputs changed %d of %d table rows", changed, N_LUTS);

  int differ = 0;
  uint64_t worst = 0;
  for (int b = 0; b < COUNT; b++) {
    for (int j = 0; j < N_LUTS; j++) trlwe_copy(work[j], before[j]);
    eval_one(want[b], inputs[b], SIZE, work);
    differ += !same_tlwe(got[b], want[b]);
    const uint64_t d = tdist(tlwe_phase(got[b], out_key), entries[m[b]]);
    if (d > worst) worst = d;
    CHECK(d < (1ULL << (64 - PREC - 1)), "input %d (index %d) does not decrypt to its table entry: 2^%.1f away", b, m[b], log2((double)d + 1.0));
  }
  printf("%d of %d outputs differ from the reference loop as words; worst distance from the table entry 2^%.1f (bound 2^%d)\n", differ, COUNT, log2((double)worst + 1.0),
         64 - PREC - 1);
  CHECK(differ == 0, "%d of %d outputs of mosfhet_eval_LUT_inputs differ from the eval_LUT loop", differ, COUNT);

  /* one input alone, and inputs whose device blocks do not follow each other (reversed order): the same words */
  TLWE *again = tlwe_alloc_sample_array(COUNT, N);
  TRGSW_DFT *reversed[COUNT];
  for (int b = 0; b < COUNT; b++) reversed[b] = inputs[COUNT - 1 - b];
  mosfhet_eval_LUT_inputs(again, reversed, SIZE, LUT, COUNT);
  for (int b = 0; b < COUNT; b++) CHECK(same_tlwe(again[b], want[COUNT - 1 - b]), "reversed inputs: output %d differs", b);
  mosfhet_eval_LUT_inputs(again, inputs + 3, SIZE, LUT, 1);
  CHECK(same_tlwe(again[0], want[3]), "a batch of one differs");

  for (int b = 0; b < COUNT; b++) free_trgsw_array(inputs[b], SIZE);
  free_trgsw(tmp);
  free_tlwe_array(got, COUNT);
  free_tlwe_array(want, COUNT);
  free_tlwe_array(again, COUNT);
  free_trlwe_array(LUT, N_LUTS);
  free_trlwe_array(before, N_LUTS);
  free_trlwe_array(work, N_LUTS);
  if (!failures) printf("leveled_lut_inputs ok\n");
  return failures;
}
