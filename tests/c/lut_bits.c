/*
 * GPU test of mosfhet_eval_LUTs_bits (include/mosfhet_compat.h): 3 shared one-bit tables evaluated on 2 inputs of 4 LWE-encrypted bits each, at N = 1024, l = 2,
 * Bg = 2^8 with short keys (words are compared, nothing is decrypted).
 *   - out[b][tb] word for word equal to the same loop written against include/mosfhet.h, one sample at a time: circuit_bootstrap_3 and trgsw_to_DFT of every
 *     input bit, the reference's eval_LUT (applications/leveled_lut/vertical_packing.c:36-52: blind_rotate with a[i] = int2torus(2N - 2^i), trlwe_extract_tlwe) on
 *     a copy of each table, tlwe_keyswitch N -> n of every output;
 *   - without the output key the outputs are the eval_LUT results themselves;
 *   - every table is left as it was;
 *   - mosfhet_eval_LUTs_packed_bits at pack_log = 0 gives the same words on the same tables, with and without the output key;
 *   - at pack_log = 1, on one packed table whose entry x holds its two output bits at coefficients 2x and 2x + 1 (2^(4+1) < N: one TRLWE, no tree), it equals the
 *     same loop with a[i] = int2torus(2N - 2^(i+1)) and trlwe_extract_tlwe at 0 and 1, with and without the output key; the table is left as it was.
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

enum { n = 64, N = 1024, LOG_N = 10, k = 1, l = 2, Bg_bit = 8, SIZE = 4, COUNT = 2, TABLES = 3, PACK_LOG = 1, PACK = 1 << PACK_LOG };

/* destroys `table` (SIZE <= LOG_N: no tree) */
static void eval_one(TLWE output, TRGSW_DFT *input, TRLWE table) {
  Torus a[SIZE];
  for (int i = 0; i < SIZE; i++) a[i] = int2torus((uint64_t)(2 * N - (1 << i)), LOG_N + 1);
  blind_rotate(table, a, input, SIZE);
  trlwe_extract_tlwe(output, table, 0);
}

/* the same for a table of PACK output bits per entry: output[t] for t < PACK; destroys `table` (SIZE + PACK_LOG <= LOG_N: no tree) */
static void eval_one_packed(TLWE *output, TRGSW_DFT *input, TRLWE table) {
  Torus a[SIZE];
  for (int i = 0; i < SIZE; i++) a[i] = int2torus((uint64_t)(2 * N - (1 << (i + PACK_LOG))), LOG_N + 1);
  blind_rotate(table, a, input, SIZE);
  for (int t = 0; t < PACK; t++) trlwe_extract_tlwe(output[t], table, t);
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

  /* the packed table: entry x holds its PACK output bits, each 0 or 1/4, at coefficients PACK x .. PACK x + PACK - 1 */
  static Torus packed_entries[N];
  for (int i = 0; i < N; i++) {
    x = x * 6364136223846793005ULL + 1442695040888963407ULL;
    packed_entries[i] = (Torus)((x >> 40) & 1) << 62;
  }
  TRLWE packed_row = trlwe_alloc_new_sample(k, N), packed_before = trlwe_alloc_new_sample(k, N), *packed_LUTs[1] = {&packed_row};
  trlwe_torus_packing(packed_row, packed_entries, N);
  trlwe_copy(packed_before, packed_row);

  /* the inputs, bit by bit */
  TLWE *in[COUNT], *got[COUNT], *got_N[COUNT], *want[COUNT], *want_N[COUNT];
  TLWE *got0[COUNT], *got0_N[COUNT], *gotp[COUNT], *gotp_N[COUNT], *wantp[COUNT], *wantp_N[COUNT];
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
    got0[b] = tlwe_alloc_sample_array(TABLES, n);
    got0_N[b] = tlwe_alloc_sample_array(TABLES, N);
    gotp[b] = tlwe_alloc_sample_array(PACK, n);
    wantp[b] = tlwe_alloc_sample_array(PACK, n);
    gotp_N[b] = tlwe_alloc_sample_array(PACK, N);
    wantp_N[b] = tlwe_alloc_sample_array(PACK, N);
  }

  mosfhet_eval_LUTs_bits(got, in, SIZE, LUTs, TABLES, COUNT, bk, kska, kskb, ksk_out);
  mosfhet_eval_LUTs_bits(got_N, in, SIZE, LUTs, TABLES, COUNT, bk, kska, kskb, NULL);
  int changed = 0;
  for (int tb = 0; tb < TABLES; tb++) changed += !same_trlwe(LUTs_row[tb], before[tb]);
  CHECK(changed == 0, "mosfhet_eval_LUTs_bits changed %d of %d tables", changed, TABLES);

  /* one output per entry through the packed call: the same words */
  mosfhet_eval_LUTs_packed_bits(got0, in, SIZE, LUTs, TABLES, 0, COUNT, bk, kska, kskb, ksk_out);
  mosfhet_eval_LUTs_packed_bits(got0_N, in, SIZE, LUTs, TABLES, 0, COUNT, bk, kska, kskb, NULL);
  int differ0 = 0, differ0_N = 0;
  for (int b = 0; b < COUNT; b++)
    for (int tb = 0; tb < TABLES; tb++) {
      differ0 += !same_tlwe(got0[b][tb], got[b][tb]);
      differ0_N += !same_tlwe(got0_N[b][tb], got_N[b][tb]);
    }
  changed = 0;
  for (int tb = 0; tb < TABLES; tb++) changed += !same_trlwe(LUTs_row[tb], before[tb]);
  CHECK(changed == 0, "mosfhet_eval_LUTs_packed_bits (pack_log 0) changed %d of %d tables", changed, TABLES);
  printf("pack_log 0: %d of %d outputs without the output key and %d of %d with it differ from mosfhet_eval_LUTs_bits as words\n", differ0_N, COUNT * TABLES, differ0,
         COUNT * TABLES);
  CHECK(differ0_N == 0, "%d of %d outputs of mosfhet_eval_LUTs_packed_bits (pack_log 0, no output key) differ from mosfhet_eval_LUTs_bits", differ0_N, COUNT * TABLES);
  CHECK(differ0 == 0, "%d of %d outputs of mosfhet_eval_LUTs_packed_bits (pack_log 0) differ from mosfhet_eval_LUTs_bits", differ0, COUNT * TABLES);

  /* PACK output bits per entry, one table */
  mosfhet_eval_LUTs_packed_bits(gotp, in, SIZE, packed_LUTs, 1, PACK_LOG, COUNT, bk, kska, kskb, ksk_out);
  mosfhet_eval_LUTs_packed_bits(gotp_N, in, SIZE, packed_LUTs, 1, PACK_LOG, COUNT, bk, kska, kskb, NULL);
  CHECK(same_trlwe(packed_row, packed_before), "mosfhet_eval_LUTs_packed_bits (pack_log %d) changed its table", PACK_LOG);

  /* the same loop, one sample at a time */
  TRGSW sel = trgsw_alloc_new_sample(l, Bg_bit, k, N);
  TRGSW_DFT *sel_dft = trgsw_alloc_new_DFT_sample_array(SIZE, l, Bg_bit, k, N);
  int differ = 0, differ_N = 0, differp = 0, differp_N = 0;
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
    trlwe_copy(work, packed_before);
    eval_one_packed(wantp_N[b], sel_dft, work);
    for (int t = 0; t < PACK; t++) {
      tlwe_keyswitch(wantp[b][t], wantp_N[b][t], ksk_out);
      differp_N += !same_tlwe(gotp_N[b][t], wantp_N[b][t]);
      differp += !same_tlwe(gotp[b][t], wantp[b][t]);
    }
  }
  printf("%d of %d outputs without the output key and %d of %d with it differ from the loop as words\n", differ_N, COUNT * TABLES, differ, COUNT * TABLES);
  CHECK(differ_N == 0, "%d of %d outputs of mosfhet_eval_LUTs_bits (no output key) differ from circuit_bootstrap_3 + trgsw_to_DFT + eval_LUT", differ_N, COUNT * TABLES);
  CHECK(differ == 0, "%d of %d outputs of mosfhet_eval_LUTs_bits differ from circuit_bootstrap_3 + trgsw_to_DFT + eval_LUT + tlwe_keyswitch", differ, COUNT * TABLES);
  printf("pack_log %d: %d of %d outputs without the output key and %d of %d with it differ from the loop as words\n", PACK_LOG, differp_N, COUNT * PACK, differp,
         COUNT * PACK);
  CHECK(differp_N == 0, "%d of %d outputs of mosfhet_eval_LUTs_packed_bits (pack_log %d, no output key) differ from circuit_bootstrap_3 + trgsw_to_DFT + blind_rotate + extraction",
        differp_N, COUNT * PACK, PACK_LOG);
  CHECK(differp == 0, "%d of %d outputs of mosfhet_eval_LUTs_packed_bits (pack_log %d) differ from circuit_bootstrap_3 + trgsw_to_DFT + blind_rotate + extraction + tlwe_keyswitch",
        differp, COUNT * PACK, PACK_LOG);

  for (int b = 0; b < COUNT; b++) {
    free_tlwe_array(in[b], SIZE);
    free_tlwe_array(got[b], TABLES);
    free_tlwe_array(want[b], TABLES);
    free_tlwe_array(got_N[b], TABLES);
    free_tlwe_array(want_N[b], TABLES);
    free_tlwe_array(got0[b], TABLES);
    free_tlwe_array(got0_N[b], TABLES);
    free_tlwe_array(gotp[b], PACK);
    free_tlwe_array(wantp[b], PACK);
    free_tlwe_array(gotp_N[b], PACK);
    free_tlwe_array(wantp_N[b], PACK);
  }
  free_trgsw_array(sel_dft, SIZE);
  free_trgsw(sel);
  free_trlwe(work);
  for (int tb = 0; tb < TABLES; tb++) {
    free_trlwe(LUTs_row[tb]);
    free_trlwe(before[tb]);
  }
  free_trlwe(packed_row);
  free_trlwe(packed_before);
  if (!failures) printf("lut_bits ok\n");
  return failures;
}
