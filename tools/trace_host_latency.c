/*
 * Single-call times of the host functions behind DESIGN 4.17: trlwe_packing1_keyswitch_CDKS21, trlwe_RLWE_priv_keyswitch and trgsw_from_gadget (l = 4) at N = 2048,
 * key t = 4, base_bit = 9, on host structs as the reference's callers hold them.  Wall-clock median, minimum and maximum of 15 calls after two warm-up calls.
 *   gcc -O2 -std=gnu11 -Iinclude tools/trace_host_latency.c -o trace_host_latency -Lmosfhet_amd -lmosfhet_hip -L/opt/rocm/lib -lamdhip64 -lm -Wl,-rpath,<dir of the library>
 * Linked against a library built from the parent commit it times the loops of batch-1 device calls these functions were.
 */
#include <mosfhet.h>
#include <time.h>

enum { N = 2048, T = 4, BASE_BIT = 9, L = 4, BG_BIT = 8, REPS = 15 };

static double now_ms(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
static int cmp(const void *a, const void *b) { return (*(const double *)a > *(const double *)b) - (*(const double *)a < *(const double *)b); }
static void report(const char *what, double *ms) {
  qsort(ms, REPS, sizeof(double), cmp);
  printf("%-36s ms per call: median %.3f  min %.3f  max %.3f  (%d calls)\n", what, ms[REPS / 2], ms[0], ms[REPS - 1], REPS);
}

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_seed(0x4C4154);
  TRLWE_Key key = trlwe_new_binary_key(N, 1, 8.881784197001252e-16);   /* 2^-50 */
  TLWE_Key extracted = tlwe_alloc_key(N, key->sigma);
  trlwe_extract_tlwe_key(extracted, key);
  TRLWE_KS_Key *trace_key = trlwe_new_packing1_KS_key_CDKS21(key, extracted, T, BASE_BIT);
  TRLWE_KS_Key *gadget_key = trlwe_new_gadget_to_RGSW_KS(key, T, BASE_BIT);
  TLWE in = tlwe_new_sample((Torus)3 << 60, extracted);
  TRLWE out = trlwe_alloc_new_sample(1, N), rows[L];
  TorusPolynomial g = polynomial_new_torus_polynomial(N);
  for (int i = 0; i < L; i++) {
    memset(g->coeffs, 0, sizeof(Torus) * N);
    g->coeffs[0] = (Torus)1 << (64 - (i + 1) * BG_BIT);
    rows[i] = trlwe_new_sample(g, key);
  }
  TRGSW_DFT sel = trgsw_alloc_new_DFT_sample(L, BG_BIT, 1, N);
  double ms[REPS];
  for (int r = -2; r < REPS; r++) {
    const double t0 = now_ms();
    trlwe_packing1_keyswitch_CDKS21(out, in, trace_key);
    if (r >= 0) ms[r] = now_ms() - t0;
  }
  report("trlwe_packing1_keyswitch_CDKS21", ms);
  for (int r = -2; r < REPS; r++) {
    const double t0 = now_ms();
    trlwe_RLWE_priv_keyswitch(out, rows[0], gadget_key[0]);
    if (r >= 0) ms[r] = now_ms() - t0;
  }
  report("trlwe_RLWE_priv_keyswitch", ms);
  for (int r = -2; r < REPS; r++) {
    const double t0 = now_ms();
    trgsw_from_gadget(sel, rows, gadget_key);
    if (r >= 0) ms[r] = now_ms() - t0;
  }
  report("trgsw_from_gadget, l = 4", ms);
  return 0;
}
