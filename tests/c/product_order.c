/*
 * GPU test of mosfhet_bootstrap_key_set_product_order through the MOSFHET-compatible API at the TFHEpp lvl2 set (N = 2048, l = 4, Bg = 2^9, n = 632), the one
 * ring where the summation order of the external products depends on the kernel (include/mosfhet_hip.h: MOSFHET_HIP_ORDER_*).  The device list names GPU 0 twice
 * (argument 2: two contexts, two host threads, a replicated key) or once (argument 1: the host-struct pipeline alone cuts the batch).
 *   BY_COMPONENT, then REFERENCE: programmable_bootstrap_batch and full_domain_functional_bootstrap_batch of 300 host structs equal the 300 single calls on the
 *     primary context WORD FOR WORD -- a slice of 150 is beyond the two-CU kernel's batches (half the CUs), a single call is inside them.
 *   AUTO: the slices sum in the reference's order and the single calls by component, so the two are compared by phase: within 2^47 of each other and within 2^58 of
 *     the message (the bounds of tests/test_gpu_parity.py::test_split_kernel_batch_sizes_pairs_and_alone for this pair of orders at this key set).
 *   blind_rotate(tv, a, key->s, n) -- the reference's entry point that takes the key's TRGSW_DFT array, not the key -- sums as the key does: with a body chosen so that
 *     the initial rotation is the identity it equals functional_bootstrap_wo_extract of the same key word for word under both fixed orders, and the two orders differ.
 * The order is set AFTER the first sharded call, so the setter has to reach a replica that exists already; the replicas of later keys copy it when they are made.
 * Run by tests/test_product_order.py; exit status = number of failed checks.
 */
#include <math.h>
#include <mosfhet.h>
#include <mosfhet_hip.h>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __func__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static int same_tlwe(TLWE a, TLWE b) { return a->b == b->b && !memcmp(a->a, b->a, sizeof(Torus) * (size_t)a->n); }
static uint64_t tdist(Torus a, Torus b) { int64_t d = (int64_t)(a - b); return (uint64_t)(d < 0 ? -d : d); }
static double log2u(uint64_t x) { return log2((double)x + 1.0); }

enum { n = 632, N = 2048, k = 1, l = 4, Bg_bit = 9, COUNT = 300 };

/* batch against single calls: words (exact) or phases */
static void compare(const char *what, const char *order, int exact, TLWE *batch, TLWE *single, const Torus *expect, int modulus, TLWE_Key extracted) {
  int differ = 0;
  uint64_t apart = 0, off_batch = 0, off_single = 0;
  for (int i = 0; i < COUNT; i++) {
    differ += !same_tlwe(batch[i], single[i]);
    const Torus pb = tlwe_phase(batch[i], extracted), ps = tlwe_phase(single[i], extracted);
    if (tdist(pb, ps) > apart) apart = tdist(pb, ps);
    if (tdist(pb, expect[i % modulus]) > off_batch) off_batch = tdist(pb, expect[i % modulus]);
    if (tdist(ps, expect[i % modulus]) > off_single) off_single = tdist(ps, expect[i % modulus]);
  }
  printf("%-40s %-13s %3d of %d outputs differ as words; phases 2^%.1f apart; from the message: batch 2^%.1f, single calls 2^%.1f\n", what, order, differ, COUNT, log2u(apart),
         log2u(off_batch), log2u(off_single));
  if (exact) CHECK(differ == 0, "%s, %s key: %d of %d outputs of the sharded batch differ from their single calls", what, order, differ, COUNT);
  else CHECK(apart < (1ULL << 47), "%s, %s key: phases of the batch and of the single calls 2^%.1f apart", what, order, log2u(apart));
  CHECK(off_batch < (1ULL << 58) && off_single < (1ULL << 58), "%s, %s key: does not decrypt (2^%.1f, 2^%.1f)", what, order, log2u(off_batch), log2u(off_single));
}

int main(int argc, char **argv) {
  int devs[2] = {0, 0};
  const int n_dev = argc > 1 ? atoi(argv[1]) : 2;
  if (n_dev < 1 || n_dev > 2) { printf("usage: product_order [1 | 2]\n"); return 255; }
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_set_devices(n_dev, devs);
  mosfhet_seed(0x4D4F5346);
  TLWE_Key lwe_key = tlwe_new_binary_key(n, 3.0517578125e-05);                 /* 2^-15 */
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, k, 5.684341886080802e-14);      /* 2^-44 */
  TRGSW_Key trgsw_key = trgsw_new_key(rlwe_key, l, Bg_bit);
  TLWE_Key extracted = tlwe_alloc_key(N, rlwe_key->sigma);
  trlwe_extract_tlwe_key(extracted, rlwe_key);
  Bootstrap_Key bk = new_bootstrap_key(trgsw_key, lwe_key, 1);
  TLWE_KS_Key ks = tlwe_new_KS_key(lwe_key, extracted, 8, 2);
  Torus lut[4] = {int2torus(3, 4), int2torus(7, 4), int2torus(11, 4), int2torus(15, 4)}, lut8[8];
  for (int i = 0; i < 8; i++) lut8[i] = int2torus((uint64_t)((3 * i + 1) & 7), 3);
  TRLWE tv = trlwe_alloc_new_sample(k, N), tv8 = trlwe_alloc_new_sample(k, N);
  trlwe_torus_packing(tv, lut, 4);
  trlwe_torus_packing_many_LUT(tv8, lut8, 4, 2);   /* test_FDFB_new (test/tests.c:1095-1127): 2 interleaved tables of 4 */
  TLWE *in = tlwe_alloc_sample_array(COUNT, n), *fin = tlwe_alloc_sample_array(COUNT, n);
  TLWE *batch = tlwe_alloc_sample_array(COUNT, N), *single = tlwe_alloc_sample_array(COUNT, N);
  TLWE probe = tlwe_alloc_sample(n);
  tlwe_sample(probe, double2torus(1. / 8.), lwe_key);
  TRLWE rot[2] = {trlwe_alloc_new_sample(k, N), trlwe_alloc_new_sample(k, N)}, acc = trlwe_alloc_new_sample(k, N);
  for (int i = 0; i < COUNT; i++) {
    tlwe_sample(in[i], double2torus((i % 4) / 8.), lwe_key);
    tlwe_sample(fin[i], int2torus((uint64_t)(i % 8), 3), lwe_key);
  }
  /* a first sharded call: the key's replica on the second context exists before any order is set */
  programmable_bootstrap_batch(batch, tv, in, COUNT, bk, 3, 0, 0);

  static const struct { int order; const char *name; } orders[3] = {{MOSFHET_HIP_ORDER_BY_COMPONENT, "BY_COMPONENT"}, {MOSFHET_HIP_ORDER_REFERENCE, "REFERENCE"},
                                                                    {MOSFHET_HIP_ORDER_AUTO, "AUTO"}};
  for (int q = 0; q < 3; q++) {
    mosfhet_bootstrap_key_set_product_order(bk, orders[q].order);
    int got = -1;
    CHECK(mosfhet_hip_bsk_get_product_order((mosfhet_hip_bsk_t)mosfhet_bootstrap_key_device(bk), &got) == MOSFHET_HIP_OK && got == orders[q].order, "order %d not stored", orders[q].order);
    const int exact = orders[q].order != MOSFHET_HIP_ORDER_AUTO;
    programmable_bootstrap_batch(batch, tv, in, COUNT, bk, 3, 0, 0);
    for (int i = 0; i < COUNT; i++) programmable_bootstrap(single[i], tv, in[i], bk, 3, 0, 0);
    compare("programmable_bootstrap", orders[q].name, exact, batch, single, lut, 4, extracted);
    full_domain_functional_bootstrap_batch(batch, tv8, fin, COUNT, bk, ks, 3);
    for (int i = 0; i < COUNT; i++) full_domain_functional_bootstrap(single[i], tv8, fin[i], bk, ks, 3);
    compare("full_domain_functional_bootstrap", orders[q].name, exact, batch, single, lut8, 8, extracted);
    if (exact) {   /* key->s handed to blind_rotate: a temporary key view, which takes the key's order */
      probe->b = (Torus)0 - double2torus(1. / (4 * 4));   /* src/bootstrap.c:194: acc = tv * X^-round(2N (b + 1 / (4 torus_base))) = tv */
      functional_bootstrap_wo_extract(rot[q], tv, probe, bk, 4);
      trlwe_copy(acc, tv);
      blind_rotate(acc, probe->a, bk->s, n);
      const int same = !memcmp(acc->a[0]->coeffs, rot[q]->a[0]->coeffs, sizeof(Torus) * N) && !memcmp(acc->b->coeffs, rot[q]->b->coeffs, sizeof(Torus) * N);
      printf("%-40s %-13s %s functional_bootstrap_wo_extract of the key\n", "blind_rotate(tv, a, key->s, n)", orders[q].name, same ? "equals" : "DIFFERS FROM");
      CHECK(same, "blind_rotate over key->s, %s key: differs from the key's own functional_bootstrap_wo_extract", orders[q].name);
    }
  }
  CHECK(memcmp(rot[0]->b->coeffs, rot[1]->b->coeffs, sizeof(Torus) * N) != 0, "the two fixed orders gave the same words");
  printf("product_order (%d contexts): %s\n", n_dev, failures ? "FAILED" : "ok");
  free_tlwe_array(in, COUNT); free_tlwe_array(fin, COUNT); free_tlwe_array(batch, COUNT); free_tlwe_array(single, COUNT); free_trlwe(tv); free_trlwe(tv8); free_trlwe(rot[0]); free_trlwe(rot[1]); free_trlwe(acc); free_tlwe(probe);
  free_tlwe_ks_key(ks); free_bootstrap_key(bk); free_trgsw_key(trgsw_key); free_trlwe_key(rlwe_key); free_tlwe_key(lwe_key); free_tlwe_key(extracted);
  return failures > 255 ? 255 : failures;
}
