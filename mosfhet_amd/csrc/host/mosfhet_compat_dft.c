/*
 * mosfhet_compat_dft.c -- the reference's DFT-level API (SURVEY.md 8(b) "must-keep" signatures) on device-resident objects.
 *
 * DFT_Polynomial / TRLWE_DFT / TRGSW_DFT keep the reference's struct shapes (include/mosfhet.h:37-40,78-81,111-114 of the reference), but every
 * `coeffs` of a DFT-domain polynomial points to DEVICE memory in the engine's slot order.  One object = one device block:
 *     TRLWE_DFT      [k+1][N/2] complex            a[0] owns the block, b is a view at + N doubles
 *     TRGSW_DFT      [(k+1) l][k+1][N/2] complex   samples[0]->a[0] owns it; the layout of one bootstrap-key entry
 *     arrays of them one block for the whole array (every element holds a reference: elements may be freed one by one, in any order, or through
 *                    the *_array functions), so an array of TRGSW_DFT is directly a key for blind_rotate
 * Every function stages its torus-domain arguments through the calling thread's staging buffers and waits for its result; nothing here computes
 * on the host.  k = 1 (every parameter set of the reference, test/tests.c:37-62).
 */
#define _GNU_SOURCE
#include <stdlib.h>
#include <string.h>

#include "compat_internal.h"

static mosfhet_hip_ctx_t ectx(void) { return (mosfhet_hip_ctx_t)mosfhet_engine_ctx(); }
static void check_rc(int rc, const char *what) {
  if (rc || mosfhet_hip_ctx_sync(ectx(), NULL)) mc_die(what);
}
static void need(int cond, const char *what) {
  if (cond) return;
  fprintf(stderr, "mosfhet_amd: %s\n", what);
  abort();
}

void init_fft(int N) { /* src/polynomial.c:341-356 builds the per-thread FFT plans; here: start the engine (twiddle tables of every ring live in the context) */
  need(N == 1024 || N == 2048 || N == 4096, "init_fft: ring degree must be 1024, 2048 or 4096");
  (void)mosfhet_engine_ctx();
}

uint16_t inverse_mod_2N(uint16_t x, uint16_t N) { /* src/misc.c:142-159: inverse of odd x modulo 2N (a power of two), here by Newton iteration */
  const uint32_t mask = 2u * N - 1;
  uint32_t inv = x;
  for (int i = 0; i < 4; i++) inv = (inv * (2u - x * inv)) & mask;
  return (uint16_t)inv;
}

/* ------------------------------------------------------------------ DFT polynomials */
DFT_Polynomial polynomial_new_DFT_polynomial(int N) {
  return (DFT_Polynomial)mc_poly_shell(MC_POLY_DFT_OWNER, mc_dev_alloc(sizeof(double) * (size_t)N), N);
}

DFT_Polynomial *polynomial_new_array_of_polynomials_DFT(int N, int size) {
  DFT_Polynomial *r = (DFT_Polynomial *)mc_xmalloc(sizeof(DFT_Polynomial) * (size_t)(size > 0 ? size : 1));
  double *block = (double *)mc_dev_alloc(sizeof(double) * (size_t)N * (size_t)(size > 0 ? size : 1));
  McShare *share = mc_share_new(block, size);
  for (int i = 0; i < size; i++) r[i] = (DFT_Polynomial)mc_poly_shell_shared(share, block + (size_t)i * N, N);
  if (size <= 0) free(share);
  return r;
}

void free_array_of_polynomials(void *p, int size) {
  if (!p) return;
  for (int i = 0; i < size; i++) free_polynomial(((void **)p)[i]);
  free(p);
}

void polynomial_torus_to_DFT(DFT_Polynomial out, TorusPolynomial in) {
  const int N = in->N;
  Torus *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (size_t)N);
  mc_dev_copy(d, in->coeffs, sizeof(Torus) * (size_t)N, HIP_H2D);
  check_rc(mosfhet_hip_torus_to_dft_batch(ectx(), out->coeffs, d, N, 1, NULL), "polynomial_torus_to_DFT");
}

void polynomial_DFT_to_torus(TorusPolynomial out, const DFT_Polynomial in) {
  const int N = in->N;
  Torus *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (size_t)N);
  check_rc(mosfhet_hip_dft_to_torus_batch(ectx(), d, in->coeffs, N, 1, NULL), "polynomial_DFT_to_torus");
  mc_dev_copy(out->coeffs, d, sizeof(Torus) * (size_t)N, HIP_D2H);
}

void polynomial_mul_DFT(DFT_Polynomial out, DFT_Polynomial in1, DFT_Polynomial in2) {
  check_rc(mosfhet_hip_dft_mul_batch(ectx(), out->coeffs, in1->coeffs, in2->coeffs, in1->N, 1, 0, NULL), "polynomial_mul_DFT");
}

void polynomial_mul_addto_DFT(DFT_Polynomial out, DFT_Polynomial in1, DFT_Polynomial in2) {
  check_rc(mosfhet_hip_dft_mul_batch(ectx(), out->coeffs, in1->coeffs, in2->coeffs, in1->N, 1, 1, NULL), "polynomial_mul_addto_DFT");
}

void polynomial_copy_DFT_polynomial(DFT_Polynomial out, DFT_Polynomial in) {
  mc_use_device();
  mc_dev_copy(out->coeffs, in->coeffs, sizeof(double) * (size_t)in->N, HIP_D2D);
}

/* ------------------------------------------------------------------ TRLWE_DFT */
/* owner: 1 = the object owns its block, 0 = a view; share != NULL: the object holds one reference to an array's block */
static TRLWE_DFT trlwe_dft_shell(double *base, int N, int owner, McShare *share) {
  TRLWE_DFT c = (TRLWE_DFT)mc_xmalloc(sizeof(*c));
  c->a = (DFT_Polynomial *)mc_xmalloc(sizeof(DFT_Polynomial));
  c->a[0] = share ? (DFT_Polynomial)mc_poly_shell_shared(share, base, N) : (DFT_Polynomial)mc_poly_shell(owner ? MC_POLY_DFT_OWNER : MC_POLY_DFT_VIEW, base, N);
  c->b = (DFT_Polynomial)mc_poly_shell(MC_POLY_DFT_VIEW, base + N, N);
  c->k = 1;
  return c;
}

/* device block of a TRLWE_DFT made here ([2][N/2] complex); aborts on anything else */
static double *trlwe_dft_base(TRLWE_DFT c, const char *who) {
  need(c && c->k == 1 && c->b->coeffs == c->a[0]->coeffs + c->b->N, who);
  return c->a[0]->coeffs;
}

TRLWE_DFT trlwe_alloc_new_DFT_sample(int k, int N) {
  need(k == 1, "trlwe_alloc_new_DFT_sample: k = 1 only");
  return trlwe_dft_shell((double *)mc_dev_alloc(sizeof(double) * 2 * (size_t)N), N, 1, NULL);
}

TRLWE_DFT *trlwe_alloc_new_DFT_sample_array(int count, int k, int N) {
  need(k == 1, "trlwe_alloc_new_DFT_sample_array: k = 1 only");
  TRLWE_DFT *r = (TRLWE_DFT *)mc_xmalloc(sizeof(TRLWE_DFT) * (size_t)(count > 0 ? count : 1));
  double *block = (double *)mc_dev_alloc(sizeof(double) * 2 * (size_t)N * (size_t)(count > 0 ? count : 1));
  McShare *share = mc_share_new(block, count);
  for (int i = 0; i < count; i++) r[i] = trlwe_dft_shell(block + (size_t)i * 2 * N, N, 0, share);
  if (count <= 0) free(share);
  return r;
}

void trlwe_to_DFT(TRLWE_DFT out, TRLWE in) {
  const int N = in->b->N;
  double *dst = trlwe_dft_base(out, "trlwe_to_DFT: `out` was not made by trlwe_alloc_new_DFT_sample");
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * 2 * (size_t)N), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * 2 * (size_t)N);
  mc_trlwe_to_flat(h, in);
  mc_dev_copy(d, h, sizeof(Torus) * 2 * (size_t)N, HIP_H2D);
  check_rc(mosfhet_hip_torus_to_dft_batch(ectx(), dst, d, N, 2, NULL), "trlwe_to_DFT");
  mc_hstage_free(h);
}

void trlwe_from_DFT(TRLWE out, TRLWE_DFT in) {
  const int N = out->b->N;
  const double *src = trlwe_dft_base(in, "trlwe_from_DFT: `in` was not made by trlwe_alloc_new_DFT_sample");
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * 2 * (size_t)N), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * 2 * (size_t)N);
  check_rc(mosfhet_hip_dft_to_torus_batch(ectx(), d, src, N, 2, NULL), "trlwe_from_DFT");
  mc_dev_copy(h, d, sizeof(Torus) * 2 * (size_t)N, HIP_D2H);
  mc_trlwe_from_flat(out, h);
  mc_hstage_free(h);
}

/* ------------------------------------------------------------------ TRGSW_DFT */
static TRGSW_DFT trgsw_dft_shell(double *base, int l, int Bg_bit, int N, int owner, McShare *share) {
  TRGSW_DFT g = (TRGSW_DFT)mc_xmalloc(sizeof(*g));
  g->samples = (TRLWE_DFT *)mc_xmalloc(sizeof(TRLWE_DFT) * (size_t)2 * l);
  for (int r = 0; r < 2 * l; r++) g->samples[r] = trlwe_dft_shell(base + (size_t)r * 2 * N, N, owner && r == 0, r == 0 ? share : NULL);
  g->l = l;
  g->Bg_bit = Bg_bit;
  return g;
}

static size_t trgsw_dft_doubles(int l, int N) { return (size_t)2 * l * 2 * N; }

static double *trgsw_dft_base(TRGSW_DFT g, const char *who) {
  need(g && g->samples && g->l >= 1, who);
  double *base = trlwe_dft_base(g->samples[0], who);
  const int N = g->samples[0]->b->N;
  for (int r = 1; r < 2 * g->l; r++) need(trlwe_dft_base(g->samples[r], who) == base + (size_t)r * 2 * N, who);
  return base;
}

TRGSW_DFT *mc_trgsw_dft_views(double *base, int n, int l, int Bg_bit, int N) {
  TRGSW_DFT *r = (TRGSW_DFT *)mc_xmalloc(sizeof(TRGSW_DFT) * (size_t)n);
  for (int i = 0; i < n; i++) r[i] = trgsw_dft_shell(base + (size_t)i * trgsw_dft_doubles(l, N), l, Bg_bit, N, 0, NULL);
  return r;
}

void mc_trgsw_dft_views_free(TRGSW_DFT *views, int n) {
  for (int i = 0; i < n; i++) free_trgsw(views[i]);
  free(views);
}

TRGSW_DFT trgsw_alloc_new_DFT_sample(int l, int Bg_bit, int k, int N) {
  need(k == 1, "trgsw_alloc_new_DFT_sample: k = 1 only");
  return trgsw_dft_shell((double *)mc_dev_alloc(sizeof(double) * trgsw_dft_doubles(l, N)), l, Bg_bit, N, 1, NULL);
}

TRGSW_DFT *trgsw_alloc_new_DFT_sample_array(int count, int l, int Bg_bit, int k, int N) {
  need(k == 1, "trgsw_alloc_new_DFT_sample_array: k = 1 only");
  TRGSW_DFT *r = (TRGSW_DFT *)mc_xmalloc(sizeof(TRGSW_DFT) * (size_t)(count > 0 ? count : 1));
  double *block = (double *)mc_dev_alloc(sizeof(double) * trgsw_dft_doubles(l, N) * (size_t)(count > 0 ? count : 1));
  McShare *share = mc_share_new(block, count);
  for (int i = 0; i < count; i++) r[i] = trgsw_dft_shell(block + (size_t)i * trgsw_dft_doubles(l, N), l, Bg_bit, N, 0, share);
  if (count <= 0) free(share);
  return r;
}

void trgsw_to_DFT(TRGSW_DFT out, TRGSW in) {
  const int l = in->l, N = in->samples[0]->b->N, rows = 2 * l;
  need(out->l == l, "trgsw_to_DFT: gadget sizes differ");
  double *dst = trgsw_dft_base(out, "trgsw_to_DFT: `out` was not made by trgsw_alloc_new_DFT_sample");
  const size_t words = (size_t)rows * 2 * N;
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * words), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * words);
  for (int r = 0; r < rows; r++) mc_trlwe_to_flat(h + (size_t)r * 2 * N, in->samples[r]);
  mc_dev_copy(d, h, sizeof(Torus) * words, HIP_H2D);
  check_rc(mosfhet_hip_torus_to_dft_batch(ectx(), dst, d, N, rows * 2, NULL), "trgsw_to_DFT");
  out->Bg_bit = in->Bg_bit;
  mc_hstage_free(h);
}

void trgsw_mul_trlwe_DFT(TRLWE_DFT out, TRLWE in1, TRGSW_DFT in2) {
  const int N = in1->b->N;
  const double *g = trgsw_dft_base(in2, "trgsw_mul_trlwe_DFT: `in2` was not made by this library");
  double *dst = trlwe_dft_base(out, "trgsw_mul_trlwe_DFT: `out` was not made by trlwe_alloc_new_DFT_sample");
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * 2 * (size_t)N), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * 2 * (size_t)N);
  mc_trlwe_to_flat(h, in1);
  mc_dev_copy(d, h, sizeof(Torus) * 2 * (size_t)N, HIP_H2D);
  check_rc(mosfhet_hip_external_product_dft_batch(ectx(), g, 0, dst, d, N, in2->l, in2->Bg_bit, 1, NULL), "trgsw_mul_trlwe_DFT");
  mc_hstage_free(h);
}

/* An array of TRGSW_DFT as one device key: the array's own block when its entries are consecutive (Bootstrap_Key.s, trgsw_alloc_new_DFT_sample_array),
 * else a gathered copy (*owned is set and the caller frees it). */
static double *key_block(TRGSW_DFT *s, int size, int *l, int *Bg_bit, int *N, int *owned, const char *who) {
  need(s && size >= 1, who);
  double *base = trgsw_dft_base(s[0], who);
  *l = s[0]->l; *Bg_bit = s[0]->Bg_bit; *N = s[0]->samples[0]->b->N; *owned = 0;
  const size_t esz = trgsw_dft_doubles(*l, *N);
  int contiguous = 1;
  for (int i = 1; i < size; i++) {
    need(s[i]->l == *l && s[i]->Bg_bit == *Bg_bit && s[i]->samples[0]->b->N == *N, who);
    if (trgsw_dft_base(s[i], who) != base + (size_t)i * esz) contiguous = 0;
  }
  if (contiguous) return base;
  double *blk = (double *)mc_dev_alloc(sizeof(double) * esz * (size_t)size);
  for (int i = 0; i < size; i++) mc_dev_copy(blk + (size_t)i * esz, trgsw_dft_base(s[i], who), sizeof(double) * esz, HIP_D2D);
  *owned = 1;
  return blk;
}

/* src/bootstrap.c:107-122: tv <- tv * X^{sum a_i s_i} by `size` CMUX steps with the selectors s[0..size) */
void blind_rotate(TRLWE tv, Torus *a, TRGSW_DFT *s, int size) {
  int l, Bg_bit, N, owned;
  double *blk = key_block(s, size, &l, &Bg_bit, &N, &owned, "blind_rotate: `s` must be TRGSW_DFT samples made by this library (one ring, one gadget)");
  need(tv->b->N == N, "blind_rotate: ring degrees of tv and s differ");
  mosfhet_hip_bsk_t view = NULL;
  if (mosfhet_hip_bsk_view_create(ectx(), &view, blk, size, 1, N, l, Bg_bit)) mc_die("blind_rotate");
  if (!owned && mosfhet_hip_bsk_set_product_order(view, mc_order_of_block(blk))) mc_die("blind_rotate");   /* Bootstrap_Key.s: the view sums as its key does */
  const size_t acc_w = (size_t)2 * N;
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * (acc_w + size + 1)), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (acc_w + size + 1));
  mc_trlwe_to_flat(h, tv);
  memcpy(h + acc_w, a, sizeof(Torus) * (size_t)size);
  h[acc_w + size] = 0;
  mc_dev_copy(d, h, sizeof(Torus) * (acc_w + size + 1), HIP_H2D);
  check_rc(mosfhet_hip_blind_rotate_batch(ectx(), view, d, d + acc_w, 1, NULL), "blind_rotate");
  mc_dev_copy(h, d, sizeof(Torus) * acc_w, HIP_D2H);
  mc_trlwe_from_flat(tv, h);
  mc_hstage_free(h);
  mosfhet_hip_bsk_destroy(view);
  if (owned) hipFree(blk);
}

/* src/bootstrap_ga.c:35-60.  `ak` must be the automorphism key set of a Bootstrap_GA_Key (entry j <-> generator 2j + 1, one device key set).  The header of entry 0
 * of a SHORTER set (packing, trace, private keys) passes the check below; mosfhet_hip_blind_rotate_ga_batch refuses it (entries < N) and check_rc ends the program. */
void blind_rotate_ga(TRLWE tv, Torus *a, TRGSW_DFT *s, TRLWE_KS_Key *ak, int size) {
  int l, Bg_bit, N, owned;
  double *blk = key_block(s, size, &l, &Bg_bit, &N, &owned, "blind_rotate_ga: `s` must be TRGSW_DFT samples made by this library (one ring, one gadget)");
  need(ak && ak[0] && ak[0]->device && ak[0]->entry == 0, "blind_rotate_ga: `ak` must be the .ak of a Bootstrap_GA_Key");
  mosfhet_hip_bsk_t view = NULL;
  if (mosfhet_hip_bsk_view_create(ectx(), &view, blk, size, 1, N, l, Bg_bit)) mc_die("blind_rotate_ga");
  if (!owned && mosfhet_hip_bsk_set_product_order(view, mc_order_of_block(blk))) mc_die("blind_rotate_ga");   /* Bootstrap_Key.s: the view sums as its key does */
  const size_t acc_w = (size_t)2 * N;
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * (acc_w + size + 1)), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (acc_w + size + 1));
  mc_trlwe_to_flat(h, tv);
  memcpy(h + acc_w, a, sizeof(Torus) * (size_t)size);
  h[acc_w + size] = 0;
  mc_dev_copy(d, h, sizeof(Torus) * (acc_w + size + 1), HIP_H2D);
  check_rc(mosfhet_hip_blind_rotate_ga_batch(ectx(), view, (mosfhet_hip_gak_t)ak[0]->device, d, d + acc_w, 1, NULL), "blind_rotate_ga");
  mc_dev_copy(h, d, sizeof(Torus) * acc_w, HIP_D2H);
  mc_trlwe_from_flat(tv, h);
  mc_hstage_free(h);
  mosfhet_hip_bsk_destroy(view);
  if (owned) hipFree(blk);
}

/* ------------------------------------------------------------------ leveled LUT evaluation on host structs: the shared pieces of the five calls below */
static void need_of(int cond, const char *name, const char *what) {
  if (cond) return;
  fprintf(stderr, "mosfhet_amd: %s: %s\n", name, what);
  abort();
}

/* The selectors of `count` inputs as one device block [count][size] of TRGSW_DFT: the inputs' own blocks where they are when they follow each other in memory, else
 * gathered into one block first (*gathered is set and the caller frees it). */
static double *lut_selectors(TRGSW_DFT **inputs, int size, int count, int *l, int *Bg_bit, int *N, int *gathered, const char *name) {
  char who[192];
  snprintf(who, sizeof who, "%s: every input must be `size` TRGSW_DFT samples made by this library (one ring, one gadget)", name);
  double **blk = (double **)mc_xmalloc(sizeof(double *) * (size_t)count);
  int *owned = (int *)mc_xmalloc(sizeof(int) * (size_t)count);
  *gathered = 0;
  for (int b = 0; b < count; b++) {
    int lb, Bb, Nb;
    blk[b] = key_block(inputs[b], size, &lb, &Bb, &Nb, &owned[b], who);
    if (b == 0) { *l = lb; *Bg_bit = Bb; *N = Nb; }
    need(lb == *l && Bb == *Bg_bit && Nb == *N, who);
    if (owned[b]) *gathered = 1;   /* a copy key_block made: it moves into the block and is released here */
  }
  const size_t in_doubles = trgsw_dft_doubles(*l, *N) * (size_t)size;
  for (int b = 1; b < count; b++)
    if (blk[b] != blk[0] + (size_t)b * in_doubles) *gathered = 1;
  double *sel = blk[0];
  if (*gathered) {
    sel = (double *)mc_dev_alloc(sizeof(double) * in_doubles * (size_t)count);
    for (int b = 0; b < count; b++) {
      mc_dev_copy(sel + (size_t)b * in_doubles, blk[b], sizeof(double) * in_doubles, HIP_D2D);
      if (owned[b]) hipFree(blk[b]);
    }
  }
  free(owned);
  free(blk);
  return sel;
}

/* TRLWEs per table: max(1, 2^(size + pack_log) / N), after the checks on the ring and on what it holds */
static size_t lut_rows_per_table(int N, int size, int pack_log, const char *name) {
  need_of(N == 1024 || N == 2048, name, "ring degree must be 1024 or 2048");
  int log_N = 0;
  while ((1 << log_N) < N) log_N++;
  need_of(pack_log <= log_N - 1, name, "pack_log must be at most log2 N - 1");
  need_of(size + pack_log <= log_N + MOSFHET_HIP_LUT_MAX_LEVELS, name, "size + pack_log must be at most log2 N + MOSFHET_HIP_LUT_MAX_LEVELS");
  return size + pack_log > log_N ? (size_t)1 << (size + pack_log - log_N) : 1;
}

static void lut_stage_tables(Torus *h, TRLWE **LUTs, int tables, size_t n_luts, int N) {
  for (int tb = 0; tb < tables; tb++)
    for (size_t j = 0; j < n_luts; j++) mc_trlwe_to_flat(h + ((size_t)tb * n_luts + j) * 2 * (size_t)N, LUTs[tb][j]);
}

static void lut_stage_bits(Torus *h, TLWE **in, int size, int count, int n, const char *name) {
  for (int b = 0; b < count; b++)
    for (int i = 0; i < size; i++) {
      Torus *w = h + ((size_t)b * (size_t)size + (size_t)i) * ((size_t)n + 1);
      need_of(in[b][i]->n == n, name, "an input bit is not an LWE sample of the bootstrap key's dimension");
      memcpy(w, in[b][i]->a, sizeof(Torus) * (size_t)n);
      w[n] = in[b][i]->b;
    }
}

/* out[b][o] <- sample b * outs + o of h, samples of dimension n_res */
static void lut_unstage_outputs(TLWE **out, const Torus *h, int count, int outs, int n_res, const char *name, const char *what) {
  for (int b = 0; b < count; b++)
    for (int o = 0; o < outs; o++) {
      const Torus *w = h + ((size_t)b * (size_t)outs + (size_t)o) * ((size_t)n_res + 1);
      need_of(out[b][o]->n == n_res, name, what);
      memcpy(out[b][o]->a, w, sizeof(Torus) * (size_t)n_res);
      out[b][o]->b = w[n_res];
    }
}

/* The three calls on TRGSW_DFT inputs: out[b][tb * m + t], LUTs[tb] an array of max(1, 2^(size + pack_log) / N) host TRLWEs.  `one`: the one-table entry point. */
static void eval_LUTs_inputs(const char *name, TLWE **out, TRGSW_DFT **inputs, int size, TRLWE **LUTs, int tables, int pack_log, int one, int count) {
  int l, Bg_bit, N, gathered;
  double *sel = lut_selectors(inputs, size, count, &l, &Bg_bit, &N, &gathered, name);
  const int outs = tables << pack_log;
  const size_t n_luts = lut_rows_per_table(N, size, pack_log, name);
  const size_t lut_w = (size_t)tables * n_luts * 2 * (size_t)N, out_w = (size_t)count * (size_t)outs * ((size_t)N + 1);
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * (lut_w > out_w ? lut_w : out_w)), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (lut_w + out_w));
  lut_stage_tables(h, LUTs, tables, n_luts, N);
  mc_dev_copy(d, h, sizeof(Torus) * lut_w, HIP_H2D);
  check_rc(one ? mosfhet_hip_leveled_lut_batch(ectx(), d + lut_w, sel, d, size, N, l, Bg_bit, count, NULL)
               : mosfhet_hip_leveled_lut_packed_batch(ectx(), d + lut_w, sel, d, size, N, l, Bg_bit, tables, pack_log, count, NULL),
           name);
  mc_dev_copy(h, d + lut_w, sizeof(Torus) * out_w, HIP_D2H);
  lut_unstage_outputs(out, h, count, outs, N, name, "an output sample has the wrong dimension (the ring degree N)");
  mc_hstage_free(h);
  if (gathered) hipFree(sel);
}

/* The two calls on LWE-encrypted bits: in[b][i] is bit i of input b; out[b][tb * m + t], switched to the input dimension when ksk_out is given. */
static void eval_LUTs_bits(const char *name, TLWE **out, TLWE **in, int size, TRLWE **LUTs, int tables, int pack_log, int count, Bootstrap_Key key, TRLWE_KS_Key *kska,
                           Generic_KS_Key kskb, TLWE_KS_Key ksk_out) {
  const int n = key->n, N = key->N, outs = tables << pack_log;
  const size_t n_luts = lut_rows_per_table(N, size, pack_log, name);
  const int n_res = ksk_out ? out[0][0]->n : N;
  const size_t lut_w = (size_t)tables * n_luts * 2 * (size_t)N, in_w = (size_t)count * (size_t)size * ((size_t)n + 1), out_w = (size_t)count * (size_t)outs * ((size_t)n_res + 1);
  const size_t up_w = lut_w + in_w;
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * (up_w > out_w ? up_w : out_w)), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (up_w + out_w));
  lut_stage_tables(h, LUTs, tables, n_luts, N);
  lut_stage_bits(h + lut_w, in, size, count, n, name);
  mc_dev_copy(d, h, sizeof(Torus) * up_w, HIP_H2D);
  check_rc(mosfhet_hip_lut_bits_packed_batch(ectx(), (mosfhet_hip_bsk_t)mc_key_here(key->device, MC_KEY_BSK), (mosfhet_hip_gak_t)mc_key_here(kska[0]->device, MC_KEY_GAK),
                                             (mosfhet_hip_ksk_t)mc_key_here(kskb->device, MC_KEY_KSK),
                                             ksk_out ? (mosfhet_hip_ksk_t)mc_key_here(ksk_out->device, MC_KEY_KSK) : NULL, d + up_w, d, d + lut_w, size, tables, pack_log, count,
                                             NULL),
           name);
  mc_dev_copy(h, d + up_w, sizeof(Torus) * out_w, HIP_D2H);
  lut_unstage_outputs(out, h, count, outs, n_res, name, "an output sample has the wrong dimension (n with ksk_out, N without)");
  mc_hstage_free(h);
}

/* eval_LUT (applications/leveled_lut/vertical_packing.c:36-52) for `count` independent inputs against one shared table (mosfhet_hip_leveled_lut_batch):
 * inputs[b] is an array of `size` TRGSW_DFT selectors (bit i of input b's index at inputs[b][i]), LUT the array of max(1, 2^size / N) host TRLWEs, left
 * unchanged.  (out[b] is row b's only output, LUT the only table.) */
void mosfhet_eval_LUT_inputs(TLWE *out, TRGSW_DFT **inputs, int size, TRLWE *LUT, int count) {
  need(out && inputs && LUT && size >= 1 && count >= 1, "mosfhet_eval_LUT_inputs: bad argument");
  TLWE **rows = (TLWE **)mc_xmalloc(sizeof(TLWE *) * (size_t)count);
  for (int b = 0; b < count; b++) rows[b] = out + b;
  eval_LUTs_inputs("mosfhet_eval_LUT_inputs", rows, inputs, size, &LUT, 1, 0, 1, count);
  free(rows);
}

/* The same for `tables` shared tables over the same inputs (mosfhet_hip_leveled_lut_tables_batch, here as the packed call at pack_log = 0): LUTs[tb] is table tb,
 * an array of max(1, 2^size / N) host TRLWEs, left unchanged; out[b][tb] receives what eval_LUT gives for input b on table tb.  One call, the selectors fetched once
 * for all tables. */
void mosfhet_eval_LUTs_inputs(TLWE **out, TRGSW_DFT **inputs, int size, TRLWE **LUTs, int tables, int count) {
  need(out && inputs && LUTs && size >= 1 && count >= 1 && tables >= 1 && tables <= MOSFHET_HIP_LUT_MAX_TABLES, "mosfhet_eval_LUTs_inputs: bad argument");
  eval_LUTs_inputs("mosfhet_eval_LUTs_inputs", out, inputs, size, LUTs, tables, 0, 0, count);
}

/* Several outputs packed into one table (mosfhet_hip_leveled_lut_packed_batch): an entry is m = 2^pack_log adjacent coefficients; LUTs[tb] is an array of
 * max(1, 2^(size + pack_log) / N) host TRLWEs, left unchanged; out[b][tb * m + t] receives output t of the entry input b selects in table tb. */
void mosfhet_eval_LUTs_packed_inputs(TLWE **out, TRGSW_DFT **inputs, int size, TRLWE **LUTs, int tables, int pack_log, int count) {
  need(out && inputs && LUTs && size >= 1 && count >= 1 && tables >= 1 && tables <= MOSFHET_HIP_LUT_MAX_TABLES && pack_log >= 0 && pack_log <= 10 &&
           size + pack_log <= 11 + MOSFHET_HIP_LUT_MAX_LEVELS,
       "mosfhet_eval_LUTs_packed_inputs: bad argument");
  eval_LUTs_inputs("mosfhet_eval_LUTs_packed_inputs", out, inputs, size, LUTs, tables, pack_log, 0, count);
}

/* The leveled application's loop (applications/leveled_lut/main.c: circuit_bootstrap_3 src/bootstrap.c:346-366, trgsw_to_DFT src/trgsw.c:345-349, eval_LUT
 * vertical_packing.c:36-52, tlwe_keyswitch src/tlwe.c:289-320) for `count` inputs given as LWE-encrypted bits (mosfhet_hip_lut_bits_batch, here as the packed call
 * at pack_log = 0): in[b][i] is bit i of input b, LUTs[tb] table tb (an array of max(1, 2^size / N) host TRLWEs, left unchanged); out[b][tb] receives the output of
 * table tb for input b, switched to the input dimension when ksk_out is given. */
void mosfhet_eval_LUTs_bits(TLWE **out, TLWE **in, int size, TRLWE **LUTs, int tables, int count, Bootstrap_Key key, TRLWE_KS_Key *kska, Generic_KS_Key kskb,
                            TLWE_KS_Key ksk_out) {
  need(out && in && LUTs && key && kska && kska[0] && kskb && size >= 1 && count >= 1 && tables >= 1 && tables <= MOSFHET_HIP_LUT_MAX_TABLES, "mosfhet_eval_LUTs_bits: bad argument");
  eval_LUTs_bits("mosfhet_eval_LUTs_bits", out, in, size, LUTs, tables, 0, count, key, kska, kskb, ksk_out);
}

/* mosfhet_eval_LUTs_bits with packed tables (mosfhet_hip_lut_bits_packed_batch): out[b][tb * m + t], switched to the input dimension when ksk_out is given. */
void mosfhet_eval_LUTs_packed_bits(TLWE **out, TLWE **in, int size, TRLWE **LUTs, int tables, int pack_log, int count, Bootstrap_Key key, TRLWE_KS_Key *kska,
                                   Generic_KS_Key kskb, TLWE_KS_Key ksk_out) {
  need(out && in && LUTs && key && kska && kska[0] && kskb && size >= 1 && count >= 1 && tables >= 1 && tables <= MOSFHET_HIP_LUT_MAX_TABLES && pack_log >= 0 && pack_log <= 10 &&
           size + pack_log <= 11 + MOSFHET_HIP_LUT_MAX_LEVELS,
       "mosfhet_eval_LUTs_packed_bits: bad argument");
  eval_LUTs_bits("mosfhet_eval_LUTs_packed_bits", out, in, size, LUTs, tables, pack_log, count, key, kska, kskb, ksk_out);
}

/* Encrypted memory (mosfhet_hip_trlwe_ram_read_batch / _write_batch): mem[b] is input b's array of 2^size host TRLWEs, addr[b] its array of `size` TRGSW_DFT
 * selectors (address bit i at addr[b][i]), other[b] the output of a read or the value of a write.  One upload, one call, one download. */
static void trlwe_ram(const char *name, TRLWE *other, TRGSW_DFT **addr, int size, TRLWE **mem, int write, int count) {
  int l, Bg_bit, N, gathered;
  double *sel = lut_selectors(addr, size, count, &l, &Bg_bit, &N, &gathered, name);
  need_of(N == 1024 || N == 2048, name, "ring degree must be 1024 or 2048");
  need_of(size <= MOSFHET_HIP_LUT_MAX_LEVELS, name, "size must be at most MOSFHET_HIP_LUT_MAX_LEVELS");
  const size_t cells = (size_t)1 << size, row = 2 * (size_t)N;
  const size_t mem_w = (size_t)count * cells * row, other_w = (size_t)count * row;
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * (mem_w + other_w)), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (mem_w + other_w));
  for (int b = 0; b < count; b++)
    for (size_t i = 0; i < cells; i++) mc_trlwe_to_flat(h + ((size_t)b * cells + i) * row, mem[b][i]);
  if (write)
    for (int b = 0; b < count; b++) mc_trlwe_to_flat(h + mem_w + (size_t)b * row, other[b]);
  mc_dev_copy(d, h, sizeof(Torus) * (write ? mem_w + other_w : mem_w), HIP_H2D);
  if (write) {
    check_rc(mosfhet_hip_trlwe_ram_write_batch(ectx(), d, sel, d + mem_w, size, N, l, Bg_bit, count, NULL), name);
    mc_dev_copy(h, d, sizeof(Torus) * mem_w, HIP_D2H);
    for (int b = 0; b < count; b++)
      for (size_t i = 0; i < cells; i++) mc_trlwe_from_flat(mem[b][i], h + ((size_t)b * cells + i) * row);
  } else {
    check_rc(mosfhet_hip_trlwe_ram_read_batch(ectx(), d + mem_w, sel, d, size, N, l, Bg_bit, count, NULL), name);
    mc_dev_copy(h, d + mem_w, sizeof(Torus) * other_w, HIP_D2H);
    for (int b = 0; b < count; b++) mc_trlwe_from_flat(other[b], h + (size_t)b * row);
  }
  mc_hstage_free(h);
  if (gathered) hipFree(sel);
}

/* out[b] <- the cell of mem[b] at the address addr[b] encrypts: the CMUX tree over the 2^size cells, top address bit first.  mem is left unchanged. */
void mosfhet_trlwe_ram_read(TRLWE *out, TRGSW_DFT **addr, int size, TRLWE **mem, int count) {
  need(out && addr && mem && size >= 1 && count >= 1, "mosfhet_trlwe_ram_read: bad argument");
  trlwe_ram("mosfhet_trlwe_ram_read", out, addr, size, mem, 0, count);
}

/* Every cell i of mem[b] <- the chain of `size` CMUXes between the cell and val[b]: val[b] where i is the address addr[b] encrypts, the old cell elsewhere. */
void mosfhet_trlwe_ram_write(TRLWE **mem, TRGSW_DFT **addr, int size, TRLWE *val, int count) {
  need(mem && addr && val && size >= 1 && count >= 1, "mosfhet_trlwe_ram_write: bad argument");
  trlwe_ram("mosfhet_trlwe_ram_write", val, addr, size, mem, 1, count);
}

/* Encrypted automata (mosfhet_hip_trlwe_automaton_batch): word[b] is input b's array of `steps` TRGSW_DFT selectors (symbol t at word[b][t]), init[b] its state
 * vector of `states` host TRLWEs (init[0] for every input with init_shared), the tables int [layers][states].  out[b] receives V_0[b]: `states` samples with
 * start < 0, the one sample V_0[b][start] else.  One upload, one call, one download; the handle lives for the call. */
void mosfhet_trlwe_automaton(TRLWE **out, TRGSW_DFT **word, int steps, TRLWE **init, int init_shared, const int *next0, const int *next1, const int *rot0, const int *rot1,
                             int states, int layers, int start, int count) {
  const char *name = "mosfhet_trlwe_automaton";
  need(out && word && init && next0 && next1 && rot0 && rot1 && steps >= 1 && states >= 1 && layers >= 1 && count >= 1, "mosfhet_trlwe_automaton: bad argument");
  need_of(steps <= MOSFHET_HIP_AUTOMATON_MAX_STEPS && states <= MOSFHET_HIP_AUTOMATON_MAX_STATES && start < states, name, "steps, states or start out of range");
  int l, Bg_bit, N, gathered;
  double *sel = lut_selectors(word, steps, count, &l, &Bg_bit, &N, &gathered, name);
  need_of(N == 1024 || N == 2048, name, "ring degree must be 1024 or 2048");
  mosfhet_hip_automaton_t a = NULL;
  check_rc(mosfhet_hip_automaton_create(&a, next0, next1, rot0, rot1, states, layers, N), name);
  const size_t row = 2 * (size_t)N, vecs = init_shared ? 1 : (size_t)count, out_rows = start < 0 ? (size_t)states : 1;
  const size_t init_w = vecs * (size_t)states * row, out_w = (size_t)count * out_rows * row;
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * (init_w + out_w)), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (init_w + out_w));
  for (size_t b = 0; b < vecs; b++)
    for (int q = 0; q < states; q++) mc_trlwe_to_flat(h + (b * (size_t)states + (size_t)q) * row, init[b][q]);
  mc_dev_copy(d, h, sizeof(Torus) * init_w, HIP_H2D);
  check_rc(mosfhet_hip_trlwe_automaton_batch(ectx(), d + init_w, a, sel, d, init_shared, steps, start, l, Bg_bit, count, NULL), name);
  mc_dev_copy(h, d + init_w, sizeof(Torus) * out_w, HIP_D2H);
  for (size_t b = 0; b < (size_t)count; b++)
    for (size_t q = 0; q < out_rows; q++) mc_trlwe_from_flat(out[b][q], h + (b * out_rows + q) * row);
  mc_hstage_free(h);
  mosfhet_hip_automaton_destroy(a);
  if (gathered) hipFree(sel);
}

/* Selector logic (mosfhet_hip_trgsw_logic_batch): in[b] is batch element b's array of n_in TRGSW_DFT selectors, out[b] its array of n_gates selectors, gate g's
 * output at out[b][g]; gates is int [n_gates][4] = {op, x, y, z}.  The samples live on the device: the call reads and writes their blocks where the arrays follow each
 * other in memory, else through one gathered block each.  The handle is made from the samples' N and lives for the call. */
void mosfhet_trgsw_logic(TRGSW_DFT **out, TRGSW_DFT **in, const int *gates, int n_gates, int n_in, int count) {
  const char *name = "mosfhet_trgsw_logic";
  need(out && in && gates && n_gates >= 1 && n_in >= 1 && count >= 1, "mosfhet_trgsw_logic: bad argument");
  need_of(n_gates <= MOSFHET_HIP_SELLOGIC_MAX_WIRES && n_in <= MOSFHET_HIP_SELLOGIC_MAX_WIRES, name, "n_gates or n_in out of range");
  int l, Bg_bit, N, gathered, lo, Bo, No, scattered;
  double *src = lut_selectors(in, n_in, count, &l, &Bg_bit, &N, &gathered, name);
  double *dst = lut_selectors(out, n_gates, count, &lo, &Bo, &No, &scattered, name);
  need_of(lo == l && No == N, name, "the outputs' ring or gadget length differs from the inputs'");
  need_of(N == 1024 || N == 2048, name, "ring degree must be 1024 or 2048");
  mosfhet_hip_sellogic_t c = NULL;
  check_rc(mosfhet_hip_sellogic_create(&c, gates, n_gates, n_in, N), name);
  check_rc(mosfhet_hip_trgsw_logic_batch(ectx(), dst, c, src, l, Bg_bit, count, NULL), name);
  need_of(hipStreamSynchronize(NULL) == 0, name, "the device reported an error");
  const size_t esz = trgsw_dft_doubles(l, N);
  for (int b = 0; b < count; b++)
    for (int g = 0; g < n_gates; g++) {
      if (scattered) mc_dev_copy(trgsw_dft_base(out[b][g], name), dst + ((size_t)b * n_gates + g) * esz, sizeof(double) * esz, HIP_D2D);
      out[b][g]->Bg_bit = Bg_bit;
    }
  mosfhet_hip_sellogic_destroy(c);
  if (gathered) hipFree(src);
  if (scattered) hipFree(dst);
}

/* y = W x + bias with cleartext weights on `count` independent inputs (mosfhet_hip_tlwe_linear_batch; tlwe_scale_addto of src/tlwe.c:143-191 row by row):
 * in[b][i] input i of instance b, W [rows_out][rows_in], bias [rows_out] or NULL, out[b][j] of the inputs' dimension.  With a bootstrap key: the linear map, then
 * tlwe_keyswitch, then functional_bootstrap (mosfhet_hip_linear_keyswitch_functional_bootstrap_batch), out[b][j] of dimension N. */
static void tlwe_linear(const char *name, TLWE **out, TLWE **in, const int64_t *W, const Torus *bias, int rows_out, int rows_in, int count, TRLWE tv, Bootstrap_Key key,
                        TLWE_KS_Key ksk, int torus_base) {
  const int n = in[0][0]->n, n_res = key ? key->N : n, N = key ? key->N : 0;
  if (key) need_of(n == key->k * key->N, name, "the inputs must have the dimension k N of the bootstrap key's ring (the key switch's input dimension)");
  const size_t tv_w = key ? (size_t)2 * N : 0, in_w = (size_t)count * (size_t)rows_in * ((size_t)n + 1), out_w = (size_t)count * (size_t)rows_out * ((size_t)n_res + 1);
  const size_t up_w = tv_w + in_w;
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * (up_w > out_w ? up_w : out_w)), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (up_w + out_w));
  if (key) mc_trlwe_to_flat(h, tv);
  lut_stage_bits(h + tv_w, in, rows_in, count, n, name);
  mc_dev_copy(d, h, sizeof(Torus) * up_w, HIP_H2D);
  mosfhet_hip_linear_t lin = NULL;
  check_rc(mosfhet_hip_linear_create_dense(ectx(), &lin, W, bias, rows_out, rows_in), name);
  if (key)
    check_rc(mosfhet_hip_linear_keyswitch_functional_bootstrap_batch(ectx(), lin, (mosfhet_hip_ksk_t)mc_key_here(ksk->device, MC_KEY_KSK),
                                                                     (mosfhet_hip_bsk_t)mc_key_here(key->device, MC_KEY_BSK), d + up_w, d, 1, d + tv_w, count, torus_base, 1, NULL),
             name);
  else
    check_rc(mosfhet_hip_tlwe_linear_batch(ectx(), lin, d + up_w, d + tv_w, n, count, NULL), name);
  mc_dev_copy(h, d + up_w, sizeof(Torus) * out_w, HIP_D2H);   /* (synchronous: the handle is idle when it is destroyed) */
  mosfhet_hip_linear_destroy(lin);
  lut_unstage_outputs(out, h, count, rows_out, n_res, name, "an output sample has the wrong dimension (the inputs' without a bootstrap key, N with one)");
  mc_hstage_free(h);
}

void mosfhet_tlwe_linear_inputs(TLWE **out, TLWE **in, const int64_t *W, const Torus *bias, int rows_out, int rows_in, int count) {
  need(out && in && W && rows_out >= 1 && rows_in >= 1 && count >= 1, "mosfhet_tlwe_linear_inputs: bad argument");
  tlwe_linear("mosfhet_tlwe_linear_inputs", out, in, W, bias, rows_out, rows_in, count, NULL, NULL, NULL, 0);
}

void mosfhet_tlwe_linear_bootstrap_inputs(TLWE **out, TLWE **in, const int64_t *W, const Torus *bias, int rows_out, int rows_in, int count, TRLWE tv, Bootstrap_Key key,
                                          TLWE_KS_Key ksk, int torus_base) {
  need(out && in && W && tv && key && ksk && rows_out >= 1 && rows_in >= 1 && count >= 1, "mosfhet_tlwe_linear_bootstrap_inputs: bad argument");
  tlwe_linear("mosfhet_tlwe_linear_bootstrap_inputs", out, in, W, bias, rows_out, rows_in, count, tv, key, ksk, torus_base);
}

/* trlwe_full_packing_keyswitch (src/keyswitch.c:195-227) over a batch in one call (mosfhet_hip_tlwe_pack_batch): out[o] packs in[o per .. min(total, (o + 1) per) - 1],
 * sample j of it at coefficient j; key from trlwe_new_full_packing_KS_key; split = 1 gives the reference's summation, split = P cuts the key entries into P parts. */
void mosfhet_tlwe_pack(TRLWE *out, TLWE *in, uint64_t total, uint64_t per, TRLWE_KS_Key key, int split) {
  const char *name = "mosfhet_tlwe_pack";
  need(out && in && key && key->device && total >= 1 && total <= 0x7fffffffu && per >= 1 && per <= 4096, "mosfhet_tlwe_pack: bad argument");
  const int n = key->k, N = out[0]->b->N;
  const size_t outputs = (size_t)((total + per - 1) / per);
  const size_t in_w = (size_t)total * ((size_t)n + 1), out_w = outputs * 2 * (size_t)N;
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * (in_w > out_w ? in_w : out_w)), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (in_w + out_w));
  for (uint64_t j = 0; j < total; j++) {
    Torus *w = h + (size_t)j * ((size_t)n + 1);
    need_of(in[j]->n == n, name, "an input is not an LWE sample of the key's input dimension");
    memcpy(w, in[j]->a, sizeof(Torus) * (size_t)n);
    w[n] = in[j]->b;
  }
  mc_dev_copy(d, h, sizeof(Torus) * in_w, HIP_H2D);
  check_rc(mosfhet_hip_tlwe_pack_batch(ectx(), (mosfhet_hip_gak_t)mc_key_here(key->device, MC_KEY_GAK), d + in_w, d, (int)total, (int)per, split, NULL), name);
  mc_dev_copy(h, d + in_w, sizeof(Torus) * out_w, HIP_D2H);
  for (size_t o = 0; o < outputs; o++) {
    need_of(out[o]->k == 1 && out[o]->b->N == N, name, "an output is not a k = 1 TRLWE sample of the key's ring");
    mc_trlwe_from_flat(out[o], h + o * 2 * (size_t)N);
  }
  mc_hstage_free(h);
}

/* trlwe_extract_tlwe (src/trlwe.c:540-552) over a batch in one call (mosfhet_hip_trlwe_unpack_batch), the inverse layout of mosfhet_tlwe_pack: out[o per + j] =
 * extract(in[o], j); with a key, tlwe_keyswitch of every extracted sample as well (mosfhet_hip_trlwe_unpack_keyswitch_batch: the batch of N + 1 words per sample is
 * never written).  (first, stride): sample j of an input is the coefficient first + j stride; (0, 1) for the calls without a geometry. */
static void trlwe_unpack(const char *name, TLWE *out, TRLWE *in, uint64_t total, uint64_t per, uint64_t first, uint64_t stride, TLWE_KS_Key ksk) {
  const int N = in[0]->b->N, n_res = ksk ? out[0]->n : N;
  const size_t inputs = (size_t)((total + per - 1) / per);
  const size_t in_w = inputs * 2 * (size_t)N, out_w = (size_t)total * ((size_t)n_res + 1);
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * (in_w > out_w ? in_w : out_w)), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (in_w + out_w));
  for (size_t o = 0; o < inputs; o++) {
    need_of(in[o]->k == 1 && in[o]->b->N == N, name, "an input is not a k = 1 TRLWE sample of the first input's ring");
    mc_trlwe_to_flat(h + o * 2 * (size_t)N, in[o]);
  }
  mc_dev_copy(d, h, sizeof(Torus) * in_w, HIP_H2D);
  if (ksk)
    check_rc(mosfhet_hip_trlwe_unpack_strided_keyswitch_batch(ectx(), (mosfhet_hip_ksk_t)mc_key_here(ksk->device, MC_KEY_KSK), d + in_w, d, (int)total, (int)per, (int)first, (int)stride,
                                                              NULL), name);
  else
    check_rc(mosfhet_hip_trlwe_unpack_strided_batch(ectx(), d + in_w, d, N, (int)total, (int)per, (int)first, (int)stride, NULL), name);
  mc_dev_copy(h, d + in_w, sizeof(Torus) * out_w, HIP_D2H);
  for (uint64_t j = 0; j < total; j++) {
    const Torus *w = h + (size_t)j * ((size_t)n_res + 1);
    need_of(out[j]->n == n_res, name, "an output sample has the wrong dimension (N without a key, the key's output dimension with one)");
    memcpy(out[j]->a, w, sizeof(Torus) * (size_t)n_res);
    out[j]->b = w[n_res];
  }
  mc_hstage_free(h);
}

void mosfhet_trlwe_unpack(TLWE *out, TRLWE *in, uint64_t total, uint64_t per) {
  need(out && in && total >= 1 && total <= 0x7fffffffu && per >= 1 && per <= 4096, "mosfhet_trlwe_unpack: bad argument");
  trlwe_unpack("mosfhet_trlwe_unpack", out, in, total, per, 0, 1, NULL);
}

void mosfhet_trlwe_unpack_keyswitch(TLWE *out, TRLWE *in, uint64_t total, uint64_t per, TLWE_KS_Key ksk) {
  need(out && in && ksk && ksk->device && total >= 1 && total <= 0x7fffffffu && per >= 1 && per <= 4096, "mosfhet_trlwe_unpack_keyswitch: bad argument");
  trlwe_unpack("mosfhet_trlwe_unpack_keyswitch", out, in, total, per, 0, 1, ksk);
}

/* ... with a geometry: out[o per + j] = extract(in[o], first + j stride); the ranges are the device call's (mosfhet_hip_trlwe_unpack_strided_batch), which names what it
 * refuses */
void mosfhet_trlwe_unpack_strided(TLWE *out, TRLWE *in, uint64_t total, uint64_t per, uint64_t first, uint64_t stride) {
  need(out && in && total >= 1 && total <= 0x7fffffffu && per >= 1 && per <= 4096 && first < 4096 && stride >= 1 && stride <= 0x7fffffffu,
       "mosfhet_trlwe_unpack_strided: bad argument");
  trlwe_unpack("mosfhet_trlwe_unpack_strided", out, in, total, per, first, stride, NULL);
}

void mosfhet_trlwe_unpack_strided_keyswitch(TLWE *out, TRLWE *in, uint64_t total, uint64_t per, uint64_t first, uint64_t stride, TLWE_KS_Key ksk) {
  need(out && in && ksk && ksk->device && total >= 1 && total <= 0x7fffffffu && per >= 1 && per <= 4096 && first < 4096 && stride >= 1 && stride <= 0x7fffffffu,
       "mosfhet_trlwe_unpack_strided_keyswitch: bad argument");
  trlwe_unpack("mosfhet_trlwe_unpack_strided_keyswitch", out, in, total, per, first, stride, ksk);
}

/* src/trlwe.c:775-781: out = KeySwitch_{ks_key}(in(X^gen)); ks_key switches from key(X^gen) back to key (any entry of a key set) */
void trlwe_eval_automorphism(TRLWE out, TRLWE in, uint64_t gen, TRLWE_KS_Key ks_key) {
  const int N = in->b->N;
  const size_t row = (size_t)2 * N;
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * 2 * row), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * 2 * row);
  mc_trlwe_to_flat(h, in);
  mc_dev_copy(d, h, sizeof(Torus) * row, HIP_H2D);
  check_rc(mosfhet_hip_trlwe_eval_automorphism_entry_batch(ectx(), (mosfhet_hip_gak_t)ks_key->device, ks_key->entry, d + row, d, (int)(gen & (uint64_t)(2 * N - 1)), 1, NULL),
           "trlwe_eval_automorphism");
  mc_dev_copy(h + row, d + row, sizeof(Torus) * row, HIP_D2H);
  mc_trlwe_from_flat(out, h + row);
  mc_hstage_free(h);
}

/* src/bootstrap.c:369-389: out = (0, p0) + sum_i selector[i] (.) digit_i(p1 - p0); the l selector rows are TRLWE_DFT (trlwe_to_DFT of the packed samples) */
void public_mux(TRLWE out, TorusPolynomial p0, TorusPolynomial p1, TRLWE_DFT *selector, int l, int Bg_bit) {
  const int N = out->b->N;
  const size_t row = (size_t)2 * N;
  const char *who = "public_mux: `selector` must be TRLWE_DFT samples made by this library";
  double *sel = trlwe_dft_base(selector[0], who);
  int owned = 0;
  for (int i = 1; i < l; i++)
    if (trlwe_dft_base(selector[i], who) != sel + (size_t)i * row) owned = 1;
  if (owned) {   /* selector rows allocated one by one: gather them */
    sel = (double *)mc_dev_alloc(sizeof(double) * row * (size_t)l);
    for (int i = 0; i < l; i++) mc_dev_copy(sel + (size_t)i * row, trlwe_dft_base(selector[i], who), sizeof(double) * row, HIP_D2D);
  }
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * (2 * (size_t)N + row)), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (2 * (size_t)N + row));
  memcpy(h, p0->coeffs, sizeof(Torus) * (size_t)N);
  memcpy(h + N, p1->coeffs, sizeof(Torus) * (size_t)N);
  mc_dev_copy(d, h, sizeof(Torus) * 2 * (size_t)N, HIP_H2D);
  check_rc(mosfhet_hip_public_mux_dft_batch(ectx(), d + 2 * N, d, d + N, sel, N, l, Bg_bit, 1, NULL), "public_mux");
  mc_dev_copy(h + 2 * N, d + 2 * N, sizeof(Torus) * row, HIP_D2H);
  mc_trlwe_from_flat(out, h + 2 * N);
  mc_hstage_free(h);
  if (owned) hipFree(sel);
}

/* ------------------------------------------------------------------ TRGSW-accumulator bootstrap (src/bootstrap.c:267-306) */
void functional_bootstrap_trgsw_phase1(TRGSW_DFT out, TLWE in, Bootstrap_Key key, int torus_base) {
  const int n = key->n;
  double *dst = trgsw_dft_base(out, "functional_bootstrap_trgsw_phase1: `out` was not made by trgsw_alloc_new_DFT_sample");
  need(out->l == key->l && out->samples[0]->b->N == key->N, "functional_bootstrap_trgsw_phase1: `out` and the key differ in ring or gadget");
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * ((size_t)n + 1)), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * ((size_t)n + 1));
  memcpy(h, in->a, sizeof(Torus) * (size_t)n);
  h[n] = in->b;
  mc_dev_copy(d, h, sizeof(Torus) * ((size_t)n + 1), HIP_H2D);
  check_rc(mosfhet_hip_functional_bootstrap_trgsw_phase1_batch(ectx(), (mosfhet_hip_bsk_t)key->device, dst, d, 1, torus_base, NULL), "functional_bootstrap_trgsw_phase1");
  out->Bg_bit = key->Bg_bit;
  mc_hstage_free(h);
}

void functional_bootstrap_trgsw_phase2(TLWE out, TRGSW_DFT in, TRLWE tv) {
  const int N = tv->b->N;
  const size_t row = (size_t)2 * N;
  const double *g = trgsw_dft_base(in, "functional_bootstrap_trgsw_phase2: `in` was not made by this library");
  mosfhet_hip_bsk_t view = NULL;   /* the selector is its own one-entry key: ring and gadget come from the sample, as in the reference (src/bootstrap.c:297-306) */
  if (mosfhet_hip_bsk_view_create(ectx(), &view, g, 1, 1, N, in->l, in->Bg_bit)) mc_die("functional_bootstrap_trgsw_phase2");
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * (row + N + 1)), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (row + N + 1));
  mc_trlwe_to_flat(h, tv);
  mc_dev_copy(d, h, sizeof(Torus) * row, HIP_H2D);
  check_rc(mosfhet_hip_functional_bootstrap_trgsw_phase2_batch(ectx(), view, d + row, g, d, 1, 1, NULL), "functional_bootstrap_trgsw_phase2");
  mc_dev_copy(h + row, d + row, sizeof(Torus) * ((size_t)N + 1), HIP_D2H);
  memcpy(out->a, h + row, sizeof(Torus) * (size_t)N);
  out->b = h[row + N];
  mc_hstage_free(h);
  mosfhet_hip_bsk_destroy(view);
}

/* ------------------------------------------------------------------ arrays and convenience constructors (src/trlwe.c:15-21,96-102,318-322, src/trgsw.c:82-88,137-143) */
TRLWE *trlwe_alloc_new_sample_array(int count, int k, int N) {
  TRLWE *r = (TRLWE *)mc_xmalloc(sizeof(TRLWE) * (size_t)(count > 0 ? count : 1));
  for (int i = 0; i < count; i++) r[i] = trlwe_alloc_new_sample(k, N);
  return r;
}

void free_trlwe_array(void *p, int count) {
  if (!p) return;
  for (int i = 0; i < count; i++) free_trlwe(((void **)p)[i]);
  free(p);
}

TRLWE trlwe_new_sample(TorusPolynomial m, TRLWE_Key key) {
  TRLWE c = trlwe_alloc_new_sample(key->k, key->s[0]->N);
  trlwe_sample(c, m, key);
  return c;
}

TRGSW *trgsw_alloc_new_sample_array(int count, int l, int Bg_bit, int k, int N) {
  TRGSW *r = (TRGSW *)mc_xmalloc(sizeof(TRGSW) * (size_t)(count > 0 ? count : 1));
  for (int i = 0; i < count; i++) r[i] = trgsw_alloc_new_sample(l, Bg_bit, k, N);
  return r;
}

void free_trgsw_array(void *p, int count) {
  if (!p) return;
  for (int i = 0; i < count; i++) free_trgsw(((void **)p)[i]);
  free(p);
}

/* y = W x + bias with cleartext POLYNOMIAL weights on `count` independent packed inputs (mosfhet_hip_trlwe_linear_batch / _extract_batch; trlwe_DFT_mul_by_polynomial and
 * trlwe_DFT_mul_addto_by_polynomial of src/trlwe.c:491-505 row by row): idx < 0: out_trlwe[b rows_out + j]; else out_tlwe[b rows_out + j] = trlwe_extract_tlwe(., idx). */
static void trlwe_linear(const char *name, TRLWE *out_trlwe, TLWE *out_tlwe, TRLWE *in, const int64_t *W, const Torus *bias, int rows_out, int rows_in, int count, int idx) {
  const int N = in[0]->b->N;
  const size_t ins = (size_t)count * (size_t)rows_in, outs = (size_t)count * (size_t)rows_out, one = idx < 0 ? (size_t)2 * N : (size_t)N + 1;
  const size_t in_w = ins * 2 * (size_t)N, out_w = outs * one;
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * (in_w > out_w ? in_w : out_w)), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (in_w + out_w));
  for (size_t o = 0; o < ins; o++) {
    need_of(in[o]->k == 1 && in[o]->b->N == N, name, "an input is not a k = 1 TRLWE sample of the first input's ring");
    mc_trlwe_to_flat(h + o * 2 * (size_t)N, in[o]);
  }
  mc_dev_copy(d, h, sizeof(Torus) * in_w, HIP_H2D);
  mosfhet_hip_polylinear_t lin = NULL;
  check_rc(mosfhet_hip_polylinear_create_dense(ectx(), &lin, W, bias, rows_out, rows_in, N), name);
  if (idx < 0)
    check_rc(mosfhet_hip_trlwe_linear_batch(ectx(), lin, d + in_w, d, count, NULL), name);
  else
    check_rc(mosfhet_hip_trlwe_linear_extract_batch(ectx(), lin, d + in_w, d, idx, count, NULL), name);
  mc_dev_copy(h, d + in_w, sizeof(Torus) * out_w, HIP_D2H);   /* (synchronous: the handle is idle when it is destroyed) */
  mosfhet_hip_polylinear_destroy(lin);
  for (size_t o = 0; o < outs; o++) {
    const Torus *w = h + o * one;
    if (idx < 0) {
      need_of(out_trlwe[o]->k == 1 && out_trlwe[o]->b->N == N, name, "an output is not a k = 1 TRLWE sample of the inputs' ring");
      mc_trlwe_from_flat(out_trlwe[o], w);
    } else {
      need_of(out_tlwe[o]->n == N, name, "an output sample has the wrong dimension (N)");
      memcpy(out_tlwe[o]->a, w, sizeof(Torus) * (size_t)N);
      out_tlwe[o]->b = w[N];
    }
  }
  mc_hstage_free(h);
}

void mosfhet_trlwe_linear(TRLWE *out, TRLWE *in, const int64_t *W, const Torus *bias, int rows_out, int rows_in, int count) {
  need(out && in && W && rows_out >= 1 && rows_in >= 1 && count >= 1, "mosfhet_trlwe_linear: bad argument");
  trlwe_linear("mosfhet_trlwe_linear", out, NULL, in, W, bias, rows_out, rows_in, count, -1);
}

void mosfhet_trlwe_linear_extract(TLWE *out, TRLWE *in, const int64_t *W, const Torus *bias, int rows_out, int rows_in, int count, int idx) {
  need(out && in && W && rows_out >= 1 && rows_in >= 1 && count >= 1 && idx >= 0, "mosfhet_trlwe_linear_extract: bad argument");
  trlwe_linear("mosfhet_trlwe_linear_extract", NULL, out, in, W, bias, rows_out, rows_in, count, idx);
}

/* y = W x + bias with ENCRYPTED polynomial weights (TRGSW samples, W[j rows_in + i]) on `count` independent packed inputs (mosfhet_hip_trlwe_gsw_linear_batch /
 * _extract_batch: a sum of trgsw_mul_trlwe_DFT, src/trgsw.c:385-423, with one rounding per row): idx < 0: out_trlwe[b rows_out + j]; else out_tlwe[b rows_out + j] =
 * trlwe_extract_tlwe(., idx).  One upload, one call, one download. */
static void trlwe_gsw_linear(const char *name, TRLWE *out_trlwe, TLWE *out_tlwe, TRLWE *in, TRGSW *W, const Torus *bias, int rows_out, int rows_in, int count, int idx) {
  const int N = in[0]->b->N, l = W[0]->l, Bg_bit = W[0]->Bg_bit, rows = 2 * l;
  const size_t ins = (size_t)count * (size_t)rows_in, outs = (size_t)count * (size_t)rows_out, one = idx < 0 ? (size_t)2 * N : (size_t)N + 1;
  const size_t in_w = ins * 2 * (size_t)N, out_w = outs * one, entries = (size_t)rows_out * (size_t)rows_in, esz = (size_t)rows * 2 * (size_t)N;
  Torus *h = (Torus *)mc_hstage_alloc(sizeof(Torus) * (in_w > out_w ? in_w : out_w)), *d = (Torus *)mc_stage_alloc(sizeof(Torus) * (in_w + out_w));
  Torus *w = (Torus *)mc_xmalloc(sizeof(Torus) * entries * esz);
  for (size_t e = 0; e < entries; e++) {
    need_of(W[e]->l == l && W[e]->Bg_bit == Bg_bit, name, "a weight has another gadget than the first weight");
    for (int r = 0; r < rows; r++) {
      need_of(W[e]->samples[r]->k == 1 && W[e]->samples[r]->b->N == N, name, "a weight is not a k = 1 TRGSW sample of the inputs' ring");
      mc_trlwe_to_flat(w + e * esz + (size_t)r * 2 * (size_t)N, W[e]->samples[r]);
    }
  }
  for (size_t o = 0; o < ins; o++) {
    need_of(in[o]->k == 1 && in[o]->b->N == N, name, "an input is not a k = 1 TRLWE sample of the first input's ring");
    mc_trlwe_to_flat(h + o * 2 * (size_t)N, in[o]);
  }
  mc_dev_copy(d, h, sizeof(Torus) * in_w, HIP_H2D);
  mosfhet_hip_gswlinear_t lin = NULL;
  check_rc(mosfhet_hip_gswlinear_create_dense(ectx(), &lin, w, bias, rows_out, rows_in, N, l, Bg_bit), name);
  free(w);
  if (idx < 0)
    check_rc(mosfhet_hip_trlwe_gsw_linear_batch(ectx(), lin, d + in_w, d, count, NULL), name);
  else
    check_rc(mosfhet_hip_trlwe_gsw_linear_extract_batch(ectx(), lin, d + in_w, d, idx, count, NULL), name);
  mc_dev_copy(h, d + in_w, sizeof(Torus) * out_w, HIP_D2H);   /* (synchronous: the handle is idle when it is destroyed) */
  mosfhet_hip_gswlinear_destroy(lin);
  for (size_t o = 0; o < outs; o++) {
    const Torus *r = h + o * one;
    if (idx < 0) {
      need_of(out_trlwe[o]->k == 1 && out_trlwe[o]->b->N == N, name, "an output is not a k = 1 TRLWE sample of the inputs' ring");
      mc_trlwe_from_flat(out_trlwe[o], r);
    } else {
      need_of(out_tlwe[o]->n == N, name, "an output sample has the wrong dimension (N)");
      memcpy(out_tlwe[o]->a, r, sizeof(Torus) * (size_t)N);
      out_tlwe[o]->b = r[N];
    }
  }
  mc_hstage_free(h);
}

void mosfhet_trlwe_gsw_linear(TRLWE *out, TRLWE *in, TRGSW *W, const Torus *bias, int rows_out, int rows_in, int count) {
  need(out && in && W && rows_out >= 1 && rows_in >= 1 && count >= 1, "mosfhet_trlwe_gsw_linear: bad argument");
  trlwe_gsw_linear("mosfhet_trlwe_gsw_linear", out, NULL, in, W, bias, rows_out, rows_in, count, -1);
}

void mosfhet_trlwe_gsw_linear_extract(TLWE *out, TRLWE *in, TRGSW *W, const Torus *bias, int rows_out, int rows_in, int count, int idx) {
  need(out && in && W && rows_out >= 1 && rows_in >= 1 && count >= 1 && idx >= 0, "mosfhet_trlwe_gsw_linear_extract: bad argument");
  trlwe_gsw_linear("mosfhet_trlwe_gsw_linear_extract", NULL, out, in, W, bias, rows_out, rows_in, count, idx);
}

/* pure host integer code: X^(N - c stride) * X^(c stride) = X^N = -1, so the entry at N - c stride is negated */
int mosfhet_polylinear_dot_layout(int64_t *poly, const int64_t *w, int per, int N, int stride) {
  if (!poly || !w || per < 1 || stride < 1 || N < 1 || (N & (N - 1)) || (long long)per * stride > N) return -1;
  memset(poly, 0, sizeof(int64_t) * (size_t)N);
  poly[0] = w[0];
  for (int c = 1; c < per; c++) poly[N - c * stride] = (int64_t)(0 - (uint64_t)w[c]);
  return 0;
}
