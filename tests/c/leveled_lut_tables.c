/*
 * GPU test of mosfhet_eval_LUTs_inputs (include/mosfhet_compat.h): 4 shared 2^13-entry tables evaluated on 4 independent inputs, each encrypted bit by bit as
 * TRGSW_DFT samples, at the reference application's ring and gadget (N = 2048, l = 1, Bg = 2^23; 4 output bits per table) -- set B of tests/test_leveled_lut.py.
 *   - out[b][tb] word for word equal to the reference's own eval_LUT loop (applications/leveled_lut/vertical_packing.c:24-52) written against include/mosfhet.h:
 *     trlwe_sub / trgsw_mul_trlwe_DFT / trlwe_from_DFT / trlwe_add per tree node, blind_rotate with a[i] = int2torus(2N - 2^i), trlwe_extract_tlwe, one input
 *     and one table at a time on a copy of the table (that loop destroys its table);
 *   - every output decrypts to the entry of its table at its input;
 *   - every table is left as it was;
 *   - one table through the new call equals mosfhet_eval_LUT_inputs on that table.
 * Run by tests/test_leveled_lut_tables.py; exit status = number of failed checks.
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

enum { N = 2048, LOG_N = 11, k = 1, l = 1, Bg_bit = 23, SIZE = 13, PREC = 4, COUNT = 4, TABLES = 4, N_LUTS = 1 << (SIZE - LOG_N) };

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
  mosfhet_seed(0x4C555453);
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, k, 2.220446049250313e-16);   /* 2^-52 */
  TRGSW_Key key = trgsw_new_key(rlwe_key, l, Bg_bit);
  TLWE_Key out_key = tlwe_alloc_key(N, rlwe_key->sigma);
  trlwe_extract_tlwe_key(out_key, rlwe_key);

  /* the tables: 4 x 2^13 entries of 4 bits, each 4 trivial TRLWEs */
  static Torus entries[TABLES][1 << SIZE];
  uint64_t x = 0x9E3779B97F4A7C15ULL;
  TRLWE *LUTs[TABLES], *before[TABLES], *work = trlwe_alloc_new_sample_array(N_LUTS, k, N);
  for (int tb = 0; tb < TABLES; tb++) {
    for (int i = 0; i < (1 << SIZE); i++) {
      x = x * 6364136223846793005ULL + 1442695040888963407ULL;
      entries[tb][i] = (Torus)((x >> 40) & ((1u << PREC) - 1)) << (64 - PREC);
    }
    LUTs[tb] = trlwe_alloc_new_sample_array(N_LUTS, k, N);
    before[tb] = trlwe_alloc_new_sample_array(N_LUTS, k, N);
    for (int j = 0; j < N_LUTS; j++) {
      trlwe_torus_packing(LUTs[tb][j], entries[tb] + (size_t)j * N, N);
      trlwe_copy(before[tb][j], LUTs[tb][j]);
    }
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

  TLWE *got[COUNT], *want[COUNT];
  for (int b = 0; b < COUNT; b++) {
    got[b] = tlwe_alloc_sample_array(TABLES, N);
    want[b] = tlwe_alloc_sample_array(TABLES, N);
  }
  mosfhet_eval_LUTs_inputs(got, inputs, SIZE, LUTs, TABLES, COUNT);
  int changed = 0;
  for (int tb = 0; tb < TABLES; tb++)
    for (int j = 0; j < N_LUTS; j++) changed += !same_trlwe(LUTs[tb][j], before[tb][j]);
  CHECK(changed == 0, "mosfhet_eval_LUTs_inputs changed %d of %d table rows", changed, TABLES * N_LUTS);

  int differ = 0;
  uint64_t worst = 0;
  for (int b = 0; b < COUNT; b++)
    for (int tb = 0; tb < TABLES; tb++) {
      for (int j = 0; j < N_LUTS; j++) trlwe_copy(work[j], before[tb][j]);
      eval_one(want[b][tb], inputs[b], SIZE, work);
      differ += !same_tlwe(got[b][tb], want[b][tb]);
      const uint64_t d = tdist(tlwe_phase(got[b][tb], out_key), entries[tb][m[b]]);
      if (d > worst) worst = d;
      CHECK(d < (1ULL << (64 - PREC - 1)), "input %d (index %d), table %d does not decrypt to its table entry: 2^%.1f away", b, m[b], tb, log2((double)d + 1.0));
    }
  printf("%d of %d outputs differ from the reference loop as words; worst distance from the table entry 2^%.1f (bound 2^%d)\n", differ, COUNT * TABLES,
         log2((double)worst + 1.0), 64 - PREC - 1);
  CHECK(differ == 0, "%d of %d outputs of mosfhet_eval_LUTs_inputs differ from the eval_LUT loop", differ, COUNT * TABLES);

  /* one table through the new call, and the one-table call on the same table: the same words */
  TLWE *one = tlwe_alloc_sample_array(COUNT, N), *rows[COUNT];
  for (int b = 0; b < COUNT; b++) rows[b] = &one[b];
  mosfhet_eval_LUTs_inputs(rows, inputs, SIZE, &LUTs[2], 1, COUNT);
  for (int b = 0; b < COUNT; b++) CHECK(same_tlwe(one[b], want[b][2]), "one table through the several-table call: input %d differs", b);
  mosfhet_eval_LUT_inputs(one, inputs, SIZE, LUTs[2], COUNT);
  for (int b = 0; b < COUNT; b++) CHECK(same_tlwe(one[b], want[b][2]), "the one-table call: input %d differs", b);

  for (int b = 0; b < COUNT; b++) {
    free_trgsw_array(inputs[b], SIZE);
    free_tlwe_array(got[b], TABLES);
    free_tlwe_array(want[b], TABLES);
  }
  free_trgsw(tmp);
  free_tlwe_array(one, COUNT);
  for (int tb = 0; tb < TABLES; tb++) {
    free_trlwe_array(LUTs[tb], N_LUTS);
    free_trlwe_array(before[tb], N_LUTS);
  }
  free_trlwe_array(work, N_LUTS);
  if (!failures) printf("leveled_lut_tables ok\n");
  return failures;
}
