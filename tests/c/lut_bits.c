/*
 * GPU test of mosfhet_eval_LUTs_bits (include/mosfhet_compat.h): 3 shared one-bit tables evaluated on 2 inputs of 4 LWE-encrypted bits each, at N = 1024, l = 2,
 * Bg = 2^8 with short keys (words are compared, nothing is decrypted).
 *   - out[b][tb] word for word equal to the same loop written against include/mosfhet.h, one sample at a time: circuit_bootstrap_3 and trgsw_to_DFT of every
 *     input bit, the reference's eval_LUT (applications/leveled_lut/vertical_packing.c:36-52: blind_rotate with a[i] = int2torus(2N - 2^i), trlwe_extract_tlwe) on
 *     a copy of each table, tlwe_keyswitch N -> n of every output;
 *   - without the output key the outputs are the eval_LUT results themselves;
 *   - every table is left as it was.
 * The bootstrap key's product order is set, so that no word depends on how many bits a launch holds.
 * Run by tests/test_lut_bits.py; exit status = number of failed checks.
 */
#include <math.h>
#include <mosfhet.h>
#include <mosfhet_hip.h>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __func__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static int same_tlwe(TLWE a, TLWE b) { return a->n == b->n && a->b == b->b && !memcmp(a->a, b->a, sizeof(Torus) * (size_t)a->n); }
static int same_trlwe(TRLWE a, TRLWE b) {
  const size_t bytes = sizeof(Torus) * (size_t)a->b->N;
  return !memcmp(a->a[0]->coeffs, b->a[0]->coeffs, bytes) && !memcmp(a->b->coeffs, b->b->coeffs, bytes);
}

enum { n = 64, N = 1024, LOG_N = 10, k = 1, l = 2, Bg_bit = 8, SIZE = 4, COUNT = 2, TABLES = 3 };

/* destroys `table` (SIZE <= LOG_N: no tree) */
static void eval_one(TLWE output, TRGSW_DFT *input, TRLWE table) {
  Torus a[SIZE];
  for (int i = 0; i < SIZE; i++) a[i] = int2torus((uint64_t)(2 * N - (1 << i)), LOG_N + 1);
  blind_rotate(table, a, input, SIZE);
  trlwe_extract_tlwe(output, table, 0);
}

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_seed(0x42495453);
  TLWE_Key lwe_key = tlwe_new_binary_key(n, 3.0517578125e-05);
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, k, 5.684341886080802e-14);
  TLWE_Key extracted = tlwe_alloc_key(N, rlwe_key->sigma);
  trlwe_extract_tlwe_key(extracted, rlwe_key);
  TRGSW_Key gkey = trgsw_new_key(rlwe_key, l, Bg_bit);
  Bootstrap_Key bk = new_bootstrap_key(gkey, lwe_key, 1);
  mosfhet_bootstrap_key_set_product_order(bk, MOSFHET_HIP_ORDER_REFERENCE);
  TRLWE_KS_Key *kska = trlwe_new_priv_KS_key(rlwe_key, rlwe_key, 20, 2);
  Generic_KS_Key kskb = trlwe_new_packing1_KS_key(rlwe_key, extracted, 1, 2);
  TLWE_KS_Key ksk_out = tlwe_new_KS_key(lwe_key, extracted, 4, 4);

  /* the tables: one bit per entry, 0 or 1/4 (the message a circuit bootstrap takes) */
  static Torus entries[TABLES][N];
  uint64_t x = 0x9E3779B97F4A7C15ULL;
  TRLWE LUTs_row[TABLES], before[TABLES], *LUTs[TABLES], work = trlwe_alloc_new_sample(k, N);
  for (int tb = 0; tb < TABLES; tb++) {
    for (int i = 0; i < N; i++) {
      x = x * 6364136223846793005ULL + 1442695040888963407ULL;
      entries[tb][i] = (Torus)((x >> 40) & 1) << 62;
    }
    LUTs_row[tb] = trlwe_alloc_new_sample(k, N);
    before[tb] = trlwe_alloc_new_sample(k, N);
    trlwe_torus_packing(LUTs_row[tb], entries[tb], N);
    trlwe_copy(before[tb], LUTs_row[tb]);
    LUTs[tb] = &LUTs_row[tb];
  }

  /* the inputs, bit by bit */
  TLWE *in[COUNT], *got[COUNT], *got_N[COUNT], *want[COUNT], *want_N[COUNT];
  for (int b = 0; b < COUNT; b++) {
    x = x * 6364136223846793005ULL + 1442695040888963407ULL;
    const int m = (int)((x >> 33) & ((1u << SIZE) - 1));
    in[b] = tlwe_alloc_sample_array(SIZE, n);
    for (int i = 0; i < SIZE; i++) {
      TLWE c = tlwe_new_sample(double2torus(0.25 * ((m >> i) & 1)), lwe_key);
      tlwe_copy(in[b][i], c);
      free_tlwe(c);
    }
    got[b] = tlwe_alloc_sample_array(TABLES, n);
    want[b] = tlwe_alloc_sample_array(TABLES, n);
    got_N[b] = tlwe_alloc_sample_array(TABLES, N);
    want_N[b] = tlwe_alloc_sample_array(TABLES, N);
  }

  mosfhet_eval_LUTs_bits(got, in, SIZE, LUTs, TABLES, COUNT, bk, kska, kskb, ksk_out);
  mosfhet_eval_LUTs_bits(got_N, in, SIZE, LUTs, TABLES, COUNT, bk, kska, kskb, NULL);
  int changed = 0;
  for (int tb = 0; tb < TABLES; tb++) changed += !same_trlwe(LUTs_row[tb], before[tb]);
  CHECK(changed == 0, "mosfhet_eval_LUTs_bits changed %d of %d tables", changed, TABLES);

  /* the same loop, one sample at a time */
  TRGSW sel = trgsw_alloc_new_sample(l, Bg_bit, k, N);
  TRGSW_DFT *sel_dft = trgsw_alloc_new_DFT_sample_array(SIZE, l, Bg_bit, k, N);
  int differ = 0, differ_N = 0;
  for (int b = 0; b < COUNT; b++) {
    for (int i = 0; i < SIZE; i++) {
      circuit_bootstrap_3(sel, in[b][i], bk, kska, kskb);
      trgsw_to_DFT(sel_dft[i], sel);
    }
    for (int tb = 0; tb < TABLES; tb++) {
      trlwe_copy(work, before[tb]);
      eval_one(want_N[b][tb], sel_dft, work);
      tlwe_keyswitch(want[b][tb], want_N[b][tb], ksk_out);
      differ_N += !same_tlwe(got_N[b][tb], want_N[b][tb]);
      differ += !same_tlwe(got[b][tb], want[b][tb]);
    }
  }
  printf("%d of %d outputs without the output key and %d of %d with it differ from the loop as words\n", differ_N, COUNT * TABLES, differ, COUNT * TABLES);
  CHECK(differ_N == 0, "%d of %d outputs of mosfhet_eval_LUTs_bits (no output key) differ from circuit_bootstrap_3 + trgsw_to_DFT + eval_LUT", differ_N, COUNT * TABLES);
  CHECK(differ == 0, "%d of %d outputs of mosfhet_eval_LUTs_bits differ from circuit_bootstrap_3 + trgsw_to_DFT + eval_LUT + tlwe_keyswitch", differ, COUNT * TABLES);

  for (int b = 0; b < COUNT; b++) {
    free_tlwe_array(in[b], SIZE);
    free_tlwe_array(got[b], TABLES);
    free_tlwe_array(want[b], TABLES);
    free_tlwe_array(got_N[b], TABLES);
    free_tlwe_array(want_N[b], TABLES);
  }
  free_trgsw_array(sel_dft, SIZE);
  free_trgsw(sel);
  free_trlwe(work);
  for (int tb = 0; tb < TABLES; tb++) {
    free_trlwe(LUTs_row[tb]);
    free_trlwe(before[tb]);
  }
  if (!failures) printf("lut_bits ok\n");
  return failures;
}
