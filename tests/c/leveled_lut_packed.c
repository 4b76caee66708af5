/*
 * GPU test of mosfhet_eval_LUTs_packed_inputs (include/mosfhet_compat.h): tables whose entries hold m = 2^pack_log output values in adjacent coefficients, evaluated
 * on 5 independent inputs, each encrypted bit by bit as TRGSW_DFT samples, at N = 1024, l = 3, Bg = 2^10 -- the shapes P1 and P2 of tests/test_leveled_lut_packed.py:
 *   P1  size 5, pack_log 3, one trivial table of 256 coefficients (shorter than N: the coefficients behind it are filled too and never selected), no tree;
 *   P2  size 9, pack_log 2, two ENCRYPTED tables of two TRLWEs each: one tree level, 8 rotate steps.
 *   - out[b][tb * m + t] word for word equal to the same evaluation written against include/mosfhet.h: the CMUX tree of the reference's eval_LUT
 *     (applications/leveled_lut/vertical_packing.c:24-52) over the top selectors, blind_rotate with a[i] = int2torus(2N - 2^(i + pack_log)), then
 *     trlwe_extract_tlwe at idx t for t < m, one input and one table at a time on a copy of the table;
 *   - every output decrypts to value t of the entry of its table at its input; the inputs hold the indices 2^size - 1 and 0;
 *   - every table is left as it was.
 * Run by tests/test_leveled_lut_packed.py; exit status = number of failed checks.
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

enum { N = 1024, LOG_N = 10, k = 1, l = 3, Bg_bit = 10, PREC = 4, COUNT = 5, MAX_TABLES = 2, MAX_LUTS = 2, MAX_OUTS = 8 };

static uint64_t rnd = 0x9E3779B97F4A7C15ULL;
static uint64_t next(void) { rnd = rnd * 6364136223846793005ULL + 1442695040888963407ULL; return rnd >> 33; }

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

/* destroys `table`; output[t] for t < 2^pack_log */
static void eval_one(TLWE *output, TRGSW_DFT *input, int size, int pack_log, TRLWE *table) {
  const int rot = LOG_N - pack_log;
  for (int i = 0; i < size - rot; i++) {
    const int half = 1 << (size - rot - i - 1);
    for (int j = 0; j < half; j++) cmux(table[j], table[j], table[j + half], input[size - i - 1]);
  }
  const int steps = size > rot ? rot : size;
  Torus a[32];
  for (int i = 0; i < steps; i++) a[i] = int2torus((uint64_t)(2 * N - (1 << (i + pack_log))), LOG_N + 1);
  blind_rotate(table[0], a, input, steps);
  for (int t = 0; t < (1 << pack_log); t++) trlwe_extract_tlwe(output[t], table[0], t);
}

static void run(const char *name, int size, int pack_log, int tables, int encrypted, TRLWE_Key rlwe_key, TRGSW_Key key, TLWE_Key out_key) {
  const int m = 1 << pack_log, outs = tables * m;
  const int n_luts = size + pack_log > LOG_N ? 1 << (size + pack_log - LOG_N) : 1;
  static Torus entries[MAX_TABLES][MAX_LUTS * N];
  TRLWE *LUTs[MAX_TABLES], *before[MAX_TABLES], *work = trlwe_alloc_new_sample_array(n_luts, k, N);
  TorusPolynomial msg = polynomial_new_torus_polynomial(N);
  for (int tb = 0; tb < tables; tb++) {
    for (int i = 0; i < n_luts * N; i++) entries[tb][i] = (Torus)(next() & ((1u << PREC) - 1)) << (64 - PREC);
    LUTs[tb] = trlwe_alloc_new_sample_array(n_luts, k, N);
    before[tb] = trlwe_alloc_new_sample_array(n_luts, k, N);
    for (int j = 0; j < n_luts; j++) {
      if (encrypted) {
        memcpy(msg->coeffs, entries[tb] + (size_t)j * N, sizeof(Torus) * N);
        trlwe_sample(LUTs[tb][j], msg, rlwe_key);
      } else {
        trlwe_torus_packing(LUTs[tb][j], entries[tb] + (size_t)j * N, N);
      }
      trlwe_copy(before[tb][j], LUTs[tb][j]);
    }
  }

  /* the inputs, bit by bit (vertical_packing.c:8-22): the extreme rotations first */
  int x[COUNT];
  TRGSW_DFT *inputs[COUNT];
  TRGSW tmp = trgsw_alloc_new_sample(l, Bg_bit, k, N);
  for (int b = 0; b < COUNT; b++) {
    x[b] = b == 0 ? (1 << size) - 1 : b == 1 ? 0 : (int)(next() & ((1u << size) - 1));
    inputs[b] = trgsw_alloc_new_DFT_sample_array(size, l, Bg_bit, k, N);
    for (int i = 0; i < size; i++) {
      trgsw_monomial_sample(tmp, (x[b] >> i) & 1, 0, key);
      trgsw_to_DFT(inputs[b][i], tmp);
    }
  }

  TLWE *got[COUNT], *want = tlwe_alloc_sample_array(MAX_OUTS, N);
  for (int b = 0; b < COUNT; b++) got[b] = tlwe_alloc_sample_array(outs, N);
  mosfhet_eval_LUTs_packed_inputs(got, inputs, size, LUTs, tables, pack_log, COUNT);
  int changed = 0;
  for (int tb = 0; tb < tables; tb++)
    for (int j = 0; j < n_luts; j++) changed += !same_trlwe(LUTs[tb][j], before[tb][j]);
  CHECK(changed == 0, "%s: mosfhet_eval_LUTs_packed_inputs changed %d of %d table rows", name, changed, tables * n_luts);

  int differ = 0;
  uint64_t worst = 0;
  for (int b = 0; b < COUNT; b++)
    for (int tb = 0; tb < tables; tb++) {
      for (int j = 0; j < n_luts; j++) trlwe_copy(work[j], before[tb][j]);
      eval_one(want, inputs[b], size, pack_log, work);
      for (int t = 0; t < m; t++) {
        differ += !same_tlwe(got[b][tb * m + t], want[t]);
        const uint64_t d = tdist(tlwe_phase(got[b][tb * m + t], out_key), entries[tb][x[b] * m + t]);
        if (d > worst) worst = d;
        CHECK(d < (1ULL << (64 - PREC - 1)), "%s: input %d (index %d), table %d, output %d does not decrypt to its table entry: 2^%.1f away", name, b, x[b], tb, t,
              log2((double)d + 1.0));
      }
    }
  printf("%s: %d of %d outputs differ from the loop against mosfhet.h as words; worst distance from the table entry 2^%.1f (bound 2^%d)\n", name, differ, COUNT * outs,
         log2((double)worst + 1.0), 64 - PREC - 1);
  CHECK(differ == 0, "%s: %d of %d outputs of mosfhet_eval_LUTs_packed_inputs differ from the loop", name, differ, COUNT * outs);

  for (int b = 0; b < COUNT; b++) {
    free_trgsw_array(inputs[b], size);
    free_tlwe_array(got[b], outs);
  }
  free_tlwe_array(want, MAX_OUTS);
  free_trgsw(tmp);
  free_polynomial(msg);
  for (int tb = 0; tb < tables; tb++) {
    free_trlwe_array(LUTs[tb], n_luts);
    free_trlwe_array(before[tb], n_luts);
  }
  free_trlwe_array(work, n_luts);
}

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_seed(0x5041434B);
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, k, 5.684341886080802e-14);   /* 2^-44 */
  TRGSW_Key key = trgsw_new_key(rlwe_key, l, Bg_bit);
  TLWE_Key out_key = tlwe_alloc_key(N, rlwe_key->sigma);
  trlwe_extract_tlwe_key(out_key, rlwe_key);
  run("P1", 5, 3, 1, 0, rlwe_key, key, out_key);
  run("P2", 9, 2, 2, 1, rlwe_key, key, out_key);
  if (!failures) printf("leveled_lut_packed ok\n");
  return failures;
}
