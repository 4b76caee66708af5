/*
 * mosfhet_hip.h -- C ABI of the MI355X (gfx950) TFHE bootstrap engine.
 *
 * This is the thin device layer that a MOSFHET build links instead of its CPU hot path
 * (src/bootstrap.c, src/trgsw.c, src/polynomial.c with the src/fft back-ends, src/tlwe.c key switch).  Plain C: opaque
 * handles, raw pointers and sizes, no C++ / torch types.  Each entry point names the reference
 * function(s) of antoniocgj/MOSFHET it replaces (file:line in that repository); INTEGRATION.md shows
 * the reference-side binding.  The MOSFHET-compatible struct API (TLWE, TRLWE, Bootstrap_Key,
 * functional_bootstrap(), ...) built on top of this layer is declared in mosfhet_compat.h.
 *
 * Conventions
 *   Torus            uint64_t, arithmetic mod 2^64                         (include/mosfhet.h:27)
 *   TLWE(n)          Torus[n+1]:  a[0..n-1], b                             (mosfhet.h:51-54, flattened)
 *   TRLWE(k,N)       Torus[k+1][N]: a[0..k-1], b                           (mosfhet.h:73-76, flattened)
 *   TRGSW(k,N,l)     Torus[(k+1)l][k+1][N], row p*l+j                      (mosfhet.h:106-109, src/trgsw.c:152-168)
 *   batches          arrays of the above, densely packed, batch index outermost
 *   d_* parameters   DEVICE pointers (hipMalloc / torch CUDA storage); h_* parameters host pointers
 *   stream           a hipStream_t passed as void*; NULL = HIP's default (null) stream, as in every HIP API
 *                    (torch's default stream is that NULL handle).  Calls are asynchronous on the stream
 *                    and never synchronise the device unless documented
 *   return value     0 on success, a negative MOSFHET_HIP_E* code otherwise; mosfhet_hip_last_error()
 *                    returns a thread-local message.  The legacy void API of mosfhet_compat.h aborts on
 *                    error, like the reference's assert/exit behaviour (src/misc.c:104-128).
 *   supported        tuned kernels: k = 1; N = 1024, 2048, 4096 (all ring degrees of the reference's parameter sets, test/tests.c:37-62);
 *                    l <= 6 with l*Bg_bit < 64 (compile-time specialisations for 2x8, 4x9, 1x23); any n.  Every entry point.
 *                    general path (csrc/general_kernels.h; the reference is generic in k and N, src/trgsw.c:385-423): k <= 3 and any power-of-two
 *                    N in 256 .. 16384 -- a correctness path, one workgroup per ciphertext, bit-identical to the same oracle.  A bootstrap key with such
 *                    parameters (mosfhet_hip_bsk_create[_from_device]) serves programmable / functional bootstraps (+ wo_extract), blind_rotate, the
 *                    full-domain bootstrap, key switch + bootstrap, external products, CMUX and multivalue_bootstrap_CLOT21; the other entry points
 *                    return MOSFHET_HIP_EINVAL for it.
 *                    mosfhet_hip_torus_to_dft_batch / _dft_to_torus_batch take any such N (natural slot order outside 1024 / 2048 / 4096).
 *   threading        re-entrant, like the reference (thread-local scratch there, src/polynomial.c:269-352): a context and its key
 *                    handles are read-only after creation and may be shared by any number of host threads; device temporaries of
 *                    the compositions and of the table key switches belong to the CALLING THREAD (grown on demand, released at
 *                    thread exit).  A thread that spreads compositions over several streams must order them itself (its
 *                    temporaries are shared between its own launches); create / destroy of a handle must not race with its use.
 * DFT-domain data (bootstrap key) is device-resident in the engine's own slot order and never leaves it,
 * as in the reference where the element order is private to the FFT back-end (src/polynomial.c:336-357).
 */
#ifndef MOSFHET_HIP_H
#define MOSFHET_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MOSFHET_HIP_OK 0
#define MOSFHET_HIP_EINVAL (-1)      /* bad argument / unsupported parameter set */
#define MOSFHET_HIP_EHIP (-2)        /* a HIP runtime call failed (message has the hipError string) */
#define MOSFHET_HIP_ENODEV (-3)      /* no usable gfx950 device */

typedef struct mosfhet_hip_ctx *mosfhet_hip_ctx_t;     /* one per (process, device) */
typedef struct mosfhet_hip_bsk *mosfhet_hip_bsk_t;     /* device-resident DFT bootstrap key */
typedef struct mosfhet_hip_ksk *mosfhet_hip_ksk_t;     /* device-resident LWE key-switch key */
typedef struct mosfhet_hip_gak *mosfhet_hip_gak_t;     /* device-resident automorphism (TRLWE key-switch) key set */

const char *mosfhet_hip_last_error(void);
const char *mosfhet_hip_version(void);

/* Context: selects `device` and creates the twiddle tables (replaces the lazy per-thread
 * FFT-processor set-up of init_fft, src/polynomial.c:336-357). */
int mosfhet_hip_ctx_create(mosfhet_hip_ctx_t *out, int device);
int mosfhet_hip_ctx_destroy(mosfhet_hip_ctx_t ctx);
int mosfhet_hip_ctx_sync(mosfhet_hip_ctx_t ctx, void *stream);          /* hipStreamSynchronize */
int mosfhet_hip_device_count(void);

/* The twiddle table the engine uses for ring degree N: (re, im) pairs, N/2 - 1 of them (host copy;
 * lets tests check it is bit-identical to the oracle's). */
int mosfhet_hip_twiddles(int N, double *h_out);

/* Bootstrap key.  Takes the key in the TORUS domain, h_bk = Torus[n][(k+1)l][k+1][N] with
 * BK_i = TRGSW(s_i) -- what new_bootstrap_key holds in `tmp` before trgsw_to_DFT (src/bootstrap.c:14-18)
 * -- uploads it and runs the engine's own forward transform over every polynomial
 * (replaces trgsw_to_DFT, src/trgsw.c:345-349).  Synchronous. */
int mosfhet_hip_bsk_create(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t *out, const uint64_t *h_bk,
                           int n, int k, int N, int l, int Bg_bit);
/* Same from a device-resident torus-domain key (e.g. generated on the GPU or received over xGMI). */
int mosfhet_hip_bsk_create_from_device(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t *out, const uint64_t *d_bk,
                                       int n, int k, int N, int l, int Bg_bit, void *stream);
int mosfhet_hip_bsk_destroy(mosfhet_hip_bsk_t bsk);
size_t mosfhet_hip_bsk_bytes(mosfhet_hip_bsk_t bsk);                     /* device bytes of the DFT key */
/* Copy the DFT-domain key back in ORACLE slot order (natural recursion index, interleaved re/im),
 * double[n][(k+1)l][k+1][N]; test hook only. */
int mosfhet_hip_bsk_export_dft(mosfhet_hip_bsk_t bsk, double *h_out);

/* programmable_bootstrap over a batch (src/bootstrap.c:208-220): for every b < count
 *   d_out[b] = TLWE(kN) = SampleExtract_0( BlindRotate( tv_b * X^{-round(2N b'/2^64)}, a', BK ) )
 * with (a', b') = ((x << kappa) + 2^(63-log2(2N)+theta)) & ~(2^(64-log2(2N)+theta) - 1) and
 * torus_base = 2^(precision-1).  Ranges: 1 <= precision <= 30, 0 <= kappa <= 63 and
 * 0 <= theta <= log2(2N) - 1 (from theta = log2(2N) on the mask's shift would be 64 or more);
 * anything else fails with MOSFHET_HIP_EINVAL.  d_tv holds tv_count test vectors; tv_count == 1 shares one test
 * vector across the batch (the reference's callers pass one LUT per call), tv_count == count gives
 * each ciphertext its own. */
int mosfhet_hip_programmable_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk,
                                             uint64_t *d_out /*[count][kN+1]*/, const uint64_t *d_tv /*[tv_count][k+1][N]*/,
                                             int tv_count, const uint64_t *d_in /*[count][n+1]*/, int count,
                                             int precision, int kappa, int theta, void *stream);

/* functional_bootstrap over a batch (src/bootstrap.c:200-206). */
int mosfhet_hip_functional_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk,
                                           uint64_t *d_out /*[count][kN+1]*/, const uint64_t *d_tv, int tv_count,
                                           const uint64_t *d_in /*[count][n+1]*/, int count, int torus_base, void *stream);

/* functional_bootstrap_wo_extract over a batch (src/bootstrap.c:192-198): writes the rotated TRLWE. */
int mosfhet_hip_functional_bootstrap_wo_extract_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk,
                                                      uint64_t *d_out /*[count][k+1][N]*/, const uint64_t *d_tv, int tv_count,
                                                      const uint64_t *d_in, int count, int torus_base, void *stream);

/* blind_rotate over a batch (src/bootstrap.c:107-122): d_acc[b] is rotated IN PLACE by the n mask
 * words of d_in[b] (the b word of d_in is ignored). */
int mosfhet_hip_blind_rotate_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, uint64_t *d_acc /*[count][k+1][N]*/,
                                   const uint64_t *d_in /*[count][n+1]*/, int count, void *stream);

/* trgsw_mul_trlwe_DFT + trlwe_from_DFT over a batch (src/trgsw.c:385-423, src/trlwe.c:629-634):
 * d_out[b] = BK[key_index] (.) d_in[b], result back in the torus domain. */
int mosfhet_hip_external_product_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, int key_index,
                                       uint64_t *d_out /*[count][k+1][N]*/, const uint64_t *d_in /*[count][k+1][N]*/,
                                       int count, void *stream);

/* polynomial_torus_to_DFT / polynomial_DFT_to_torus / polynomial_mul_DFT / polynomial_mul_addto_DFT over
 * flat arrays of polynomials (src/polynomial.c:359-426).  DFT polynomials are N doubles (N/2 complex,
 * interleaved, engine slot order). */
int mosfhet_hip_torus_to_dft_batch(mosfhet_hip_ctx_t ctx, double *d_out, const uint64_t *d_in, int N, int count, void *stream);
int mosfhet_hip_dft_to_torus_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const double *d_in, int N, int count, void *stream);
int mosfhet_hip_dft_mul_batch(mosfhet_hip_ctx_t ctx, double *d_out, const double *d_a, const double *d_b,
                              int N, int count, int addto, void *stream);

/* LWE key switch.  Key layout Torus[n_in][t][2^base_bit - 1][n_out + 1], entry [i][j][v-1] =
 * TLWE_out(s_in[i] * v * 2^(64-(j+1)base_bit)) -- tlwe_new_KS_key's table (src/tlwe.c:193-212) flattened. */
int mosfhet_hip_ksk_create(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, const uint64_t *h_ksk,
                           int n_in, int n_out, int t, int base_bit);
int mosfhet_hip_ksk_destroy(mosfhet_hip_ksk_t ksk);
/* tlwe_keyswitch over a batch (src/tlwe.c:289-303), bit-exact. */
int mosfhet_hip_tlwe_keyswitch_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, uint64_t *d_out /*[count][n_out+1]*/,
                                     const uint64_t *d_in /*[count][n_in+1]*/, int count, void *stream);

/* trlwe_extract_tlwe at coefficient idx over a batch (src/trlwe.c:540-552), k = 1. */
int mosfhet_hip_trlwe_extract_tlwe_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out /*[count][N+1]*/, const uint64_t *d_in /*[count][2][N]*/,
                                         int N, int idx, int count, void *stream);
/* ... for any k >= 1 (the loop over the k mask polynomials of src/trlwe.c:540-552) */
int mosfhet_hip_trlwe_extract_tlwe_k_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out /*[count][kN+1]*/, const uint64_t *d_in /*[count][k+1][N]*/,
                                           int k, int N, int idx, int count, void *stream);
/* tlwe_addto over a batch (src/tlwe.c:170-173): d_out[b] += d_in[b], samples of n+1 words. */
int mosfhet_hip_tlwe_addto_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const uint64_t *d_in, int n, int count, void *stream);

/* full_domain_functional_bootstrap over a batch (src/bootstrap.c:519-538): sign bootstrap with the constant test
 * vector 2^62 - 2^(62-precision) at torus_base 2^(precision-1), b -= sign, LWE key switch (ksk: kN -> n), += input,
 * second bootstrap with d_tv at torus_base 2^precision.  Scratch buffers live in the bsk handle. */
int mosfhet_hip_full_domain_functional_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_ksk_t ksk,
                                                       uint64_t *d_out /*[count][kN+1]*/, const uint64_t *d_tv, int tv_count,
                                                       const uint64_t *d_in /*[count][n+1]*/, int count, int precision, void *stream);

/* multivalue_bootstrap_CLOT21 over a batch (src/bootstrap.c:222-230): one blind rotation at torus_base * n_luts,
 * then n_luts sample extractions N / (n_luts * torus_base) coefficients apart. */
int mosfhet_hip_multivalue_bootstrap_CLOT21_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, uint64_t *d_out /*[count][n_luts][kN+1]*/,
                                                  const uint64_t *d_tv, int tv_count, const uint64_t *d_in, int count,
                                                  int torus_base, int n_luts, void *stream);

/* Automorphism key set (Bootstrap_GA_Key.ak, src/bootstrap_ga.c:10, src/keyswitch.c:500-511 with skip_even): N FFT-based
 * TRLWE key-switch keys, entry j switching from s(X^(2j+1)) back to s(X).  h_ak = Torus[N][t][k+1][N] in the TORUS
 * domain (rows KS[j] = TRLWE(s_in(X) 2^(64-(j+1) base_bit)), src/keyswitch.c:12-37); transformed on upload. k = 1. */
int mosfhet_hip_gak_create(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t *out, const uint64_t *h_ak, int N, int t, int base_bit);
int mosfhet_hip_gak_destroy(mosfhet_hip_gak_t gak);
/* trlwe_eval_automorphism over a batch (src/trlwe.c:775-781 = polynomial_permute, src/polynomial.c:442-450, followed by the
 * FFT-based trlwe_keyswitch, src/keyswitch.c:162-193): d_out[b] = KeySwitch_{ak[(gen-1)/2]}(d_in[b](X^gen)); gen odd, < 2N.
 * With gen = 1 this is trlwe_keyswitch itself (entry 0 switches from s to s).  gak may be any FFT key-switch key set
 * (mosfhet_hip_trlwe_ksk_create) that HAS that entry: (gen - 1) / 2 >= entries returns MOSFHET_HIP_EINVAL before any HIP call. */
int mosfhet_hip_trlwe_eval_automorphism_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t gak, uint64_t *d_out /*[count][2][N]*/,
                                              const uint64_t *d_in /*[count][2][N]*/, int gen, int count, void *stream);
/* functional_bootstrap_ga / functional_bootstrap_wo_extract_ga over a batch (src/bootstrap_ga.c:62-76).  bsk must hold
 * BK_i = TRGSW(X^{s_i}) (new_bootstrap_key_ga, :17-20); gak must have t = l and base_bit = Bg_bit (:10).
 * extract != 0: d_out = TLWE [count][N+1]; else the rotated TRLWE [count][2][N].  The generators come from the mask words and
 * reach 2N - 1, so gak must be the full set: entries < N returns MOSFHET_HIP_EINVAL before any HIP call. */
int mosfhet_hip_functional_bootstrap_ga_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_gak_t gak, uint64_t *d_out,
                                              const uint64_t *d_tv, int tv_count, const uint64_t *d_in /*[count][n+1]*/, int count,
                                              int torus_base, int extract, void *stream);

/* Generic set of FFT-based TRLWE key-switch keys (TRLWE_KS_Key, src/keyswitch.c:12-37): `entries` keys of t rows each,
 * h_rows = Torus[entries][t][2][N] in the torus domain.  (mosfhet_hip_gak_create is this with entries = N.) */
int mosfhet_hip_trlwe_ksk_create(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t *out, const uint64_t *h_rows, int entries, int N, int t,
                                 int base_bit);
/* trlwe_keyswitch over a batch (src/keyswitch.c:162-193) with key `entry` of the set; any t. */
int mosfhet_hip_trlwe_keyswitch_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t tks, int entry, uint64_t *d_out /*[count][2][N]*/,
                                      const uint64_t *d_in, int count, void *stream);
/* trlwe_priv_keyswitch_2 over a batch (src/keyswitch.c:52-63); tks = the two keys of trlwe_new_priv_KS_key (:39-50). */
int mosfhet_hip_trlwe_priv_keyswitch_2_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t tks, uint64_t *d_out, const uint64_t *d_in,
                                             int count, void *stream);
/* LWE -> TRLWE packing key (Generic_KS_Key of trlwe_new_packing1_KS_key, src/keyswitch.c:368-390), rows UNcompressed:
 * h_rows = Torus[n][t][2^base_bit - 1][2][N]; and trlwe_packing1_keyswitch over a batch (src/keyswitch.c:458-475). */
int mosfhet_hip_packing1_ksk_create(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, const uint64_t *h_rows, int n, int N, int t,
                                    int base_bit);
int mosfhet_hip_trlwe_packing1_keyswitch_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, uint64_t *d_out /*[count][2][N]*/,
                                               const uint64_t *d_in /*[count][n+1]*/, int count, void *stream);
/* circuit_bootstrap_3 over a batch (src/bootstrap.c:346-366): d_out[b] = TRGSW = Torus[2l][2][N], rows i < l from the private
 * key switch, rows l + i from the packing key switch.  kska = 2-entry key set, kskb = packing key (n = N). */
int mosfhet_hip_circuit_bootstrap_3_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_gak_t kska, mosfhet_hip_ksk_t kskb,
                                          uint64_t *d_out /*[count][2l][2][N]*/, const uint64_t *d_in /*[count][n+1]*/, int count,
                                          void *stream);
/* The same with progress events: level_done = l caller-created hipEvent_t (as void *, entries may be NULL) or NULL; level_done[i] is recorded on the
 * launch stream when gadget level i is finished, i.e. rows i and l + i of EVERY output are final -- a host that wants the TRGSWs back can copy a level
 * out (hipMemcpy2DAsync on a stream that waits for the event) while the next level's key switches run: 268 MB per 1024 outputs at lvl2. */
int mosfhet_hip_circuit_bootstrap_3_batch_ev(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_gak_t kska, mosfhet_hip_ksk_t kskb,
                                             uint64_t *d_out, const uint64_t *d_in, int count, void *stream, void *const *level_done);

/* ---- callers either side of the bootstrap ---- */
/* public_mux over a batch (src/bootstrap.c:369-389): d_out[b] = (0, p0) + sum_i sel[b][i] * dec_i(p1 - p0); selector rows are
 * torus-domain TRLWEs [count][l][2][N] (the reference takes TRLWE_DFT; the transform is fused); p0, p1 shared by the batch. */
int mosfhet_hip_public_mux_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out /*[count][2][N]*/, const uint64_t *d_p0 /*[N]*/, const uint64_t *d_p1,
                                 const uint64_t *d_sel, int N, int l, int Bg_bit, int count, void *stream);
/* full_domain_functional_bootstrap_KS21 (variant 0, src/bootstrap.c:391-432) / _KS21_2 (variant 1, :434-463) over a batch;
 * d_tv = the 2N-coefficient cleartext test polynomial, pksk = packing key N -> TRLWE(N). */
int mosfhet_hip_full_domain_functional_bootstrap_KS21_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_ksk_t pksk,
                                                            uint64_t *d_out /*[count][N+1]*/, const uint64_t *d_tv /*[2N]*/,
                                                            const uint64_t *d_in, int count, int torus_base, int variant, void *stream);

/* multivalue_bootstrap_phase1 (src/bootstrap.c:232-243): d_out[b] = torus_base + 1 rotated accumulators [2][N]. */
int mosfhet_hip_multivalue_bootstrap_phase1_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, uint64_t *d_out /*[count][torus_base+1][2][N]*/,
                                                  const uint64_t *d_in, int count, int torus_base, void *stream);
/* multivalue_bootstrap_phase2 (src/bootstrap.c:245-265) for a batch sharing one cleartext LUT h_lut[torus_base] (HOST ints). */
int mosfhet_hip_multivalue_bootstrap_phase2_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out /*[count][N+1]*/, const int *h_lut,
                                                  const uint64_t *d_rotated, int N, int torus_base, int log_torus_base, int count, void *stream);
/* Table-lookup private key switch LWE(m) -> TRLWE(-s m): key of trlwe_new_priv_SK_KS_key_N2 (src/keyswitch.c:611-637), rows
 * uncompressed, h_rows = Torus[n+1][t][2^base_bit-1][2][N] (entry n belongs to the b word); trlwe_priv_keyswitch (:639-656). */
int mosfhet_hip_priv_ksk_create(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, const uint64_t *h_rows, int n, int N, int t, int base_bit);
int mosfhet_hip_trlwe_priv_keyswitch_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, uint64_t *d_out /*[count][2][N]*/,
                                           const uint64_t *d_in /*[count][n+1]*/, int count, void *stream);
/* circuit_bootstrap (variant 0, src/bootstrap.c:309-322) / circuit_bootstrap_2 (variant 1, :324-344): kska = private key-switch
 * key (priv_ksk_create, n = N), kskb = packing key. */
int mosfhet_hip_circuit_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_ksk_t kska, mosfhet_hip_ksk_t kskb,
                                        uint64_t *d_out /*[count][2l][2][N]*/, const uint64_t *d_in, int count, int variant, void *stream);
int mosfhet_hip_circuit_bootstrap_batch_ev(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_ksk_t kska, mosfhet_hip_ksk_t kskb,
                                           uint64_t *d_out, const uint64_t *d_in, int count, int variant, void *stream,
                                           void *const *level_done /* as in mosfhet_hip_circuit_bootstrap_3_batch_ev */);

/* functional_bootstrap_trgsw_phase1 (src/bootstrap.c:284-295): blind rotation with a TRGSW accumulator; d_out_dft[b] = TRGSW_DFT(X^-phase)
 * as [2l][2][N/2] complex in the engine's slot order (the layout of one bootstrap-key entry).  phase2 (:297-306): d_out[b] =
 * SampleExtract_0(tv (.) d_in_dft[b]); tv_count = 1 (shared) or count.  bsk supplies N, l, Bg_bit in phase 2. */
int mosfhet_hip_functional_bootstrap_trgsw_phase1_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, double *d_out_dft, const uint64_t *d_in,
                                                        int count, int torus_base, void *stream);
int mosfhet_hip_functional_bootstrap_trgsw_phase2_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, uint64_t *d_out /*[count][N+1]*/,
                                                        const double *d_in_dft, const uint64_t *d_tv, int tv_count, int count, void *stream);

/* trlwe_tensor_prod_FFT (src/trlwe.c:727-771) over a batch of pairs; rlk = 1-entry key set (mosfhet_hip_trlwe_ksk_create) holding the rows of
 * trlwe_new_RL_key (src/keyswitch.c:3-10).  tlwe_mul (src/tlwe.c:322-332): LWE x LWE under the extracted key, pksk = packing key. */
int mosfhet_hip_trlwe_tensor_prod_FFT_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t rlk, uint64_t *d_out /*[count][2][N]*/, const uint64_t *d_in1,
                                            const uint64_t *d_in2, int precision, int count, void *stream);
int mosfhet_hip_tlwe_mul_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t pksk, mosfhet_hip_gak_t rlk, uint64_t *d_out /*[count][N+1]*/, const uint64_t *d_in1,
                               const uint64_t *d_in2, int precision, int count, void *stream);
/* full_domain_functional_bootstrap_CLOT21 (variant 0, src/bootstrap.c:465-491: d_tv = two TRLWE test vectors [2][2][N]) and _CLOT21_2
 * (variant 1, :493-517: d_tv = 2^(precision-1) cleartext LUT words, on the device). */
int mosfhet_hip_full_domain_functional_bootstrap_CLOT21_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_ksk_t pksk, mosfhet_hip_gak_t rlk,
                                                              uint64_t *d_out /*[count][N+1]*/, const uint64_t *d_tv, const uint64_t *d_in, int count,
                                                              int precision, int variant, void *stream);

/* Bootstrap key with blind-rotate unfolding u = 2, 4 or 8 (new_bootstrap_key(.., unfolding), src/bootstrap.c:23-48; the reference's group
 * stride 2^u / u is an integer quotient, :34-45, so other factors make overlapping groups there and are rejected here): h_su =
 * Torus[n 2^u / u][2l][2][N], torus domain; n divisible by u.  The handle works with functional_bootstrap[_wo_extract]_batch and the
 * compositions built on them (they take the blind_rotate_unfolded branch, src/bootstrap.c:124-149,196-197). */
int mosfhet_hip_bsk_unfolded_create(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t *out, const uint64_t *h_su, int n, int N, int l, int Bg_bit,
                                    int unfolding);

/* Bootstraps of few ciphertexts with an unfolded key assemble the selectors of all key groups side by side first (two launches per chunk of `max_batch`
 * ciphertexts, up to 8 chunks; same results bit for bit); larger batches run one fused kernel.  -1: default (64, capped by 2 GiB of selectors), 0: never. */
int mosfhet_hip_set_unfold_split_max(int max_batch);
/* Unfolding 2 rotates with the per-group TRGSW assembled in the DFT domain (the key's samples are transformed once, when the handle is made; per step
 * and ciphertext the transforms of ONE CMUX for two mask words: mosfhet_amd/csrc/unfold_kernels.h).  Same mathematics as src/bootstrap.c:124-149, another
 * order of floating-point operations (oracle/oracle_ext.c:orc_blind_rotate_unfolded2_dft mirrors it bit for bit; it agrees with the reference's own
 * results to FFT rounding).  on = 0 (or MOSFHET_HIP_UNFOLD2_DFT=0) selects the torus-domain assembly, as for u = 4 and 8. */
int mosfhet_hip_set_unfold2_dft(int on);
/* the same key encrypted on the device (torus-domain samples, generator and secrets as mosfhet_hip_bsk_generate) */
int mosfhet_hip_bsk_unfolded_generate(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t *out, const uint64_t *h_s_rlwe /*[N]*/, int N, const uint64_t *h_s_lwe /*[n]*/, int n,
                                      int l, int Bg_bit, double sigma, uint64_t seed, int unfolding);

/* multivalue_bootstrap_UBR_phase1 / phase2 (src/bootstrap.c:151-190) with an unfolded key: d_sa = [count][n/u][2l][2][N/2] complex
 * (the per-group TRGSW_DFT of each input); phase 2 evaluates tv_count shared test vectors per ciphertext: d_out = [count][tv_count][N+1]. */
int mosfhet_hip_multivalue_bootstrap_UBR_phase1_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, double *d_sa, const uint64_t *d_in, int count,
                                                      void *stream);
int mosfhet_hip_multivalue_bootstrap_UBR_phase2_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, uint64_t *d_out, const uint64_t *d_tvs,
                                                      int tv_count, const uint64_t *d_in, const double *d_sa, int count, int torus_base,
                                                      void *stream);

/* trlwe_mv_extract_tlwe (mode 0: d_out = [count][amount][N+1]), _scaling (1), _scaling_addto (2), _scaling_subto (3: d_out = [count][N+1])
 * (src/trlwe.c:580-622); `amount` is the reference's amount / scale argument. */
int mosfhet_hip_trlwe_mv_extract_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const uint64_t *d_in /*[count][2][N]*/, int N, int mode, int amount,
                                       int count, void *stream);

/* On-device generation of a table-lookup TRLWE key (the 6 GB packing key of config 4 in milliseconds): kind 0 = packing key
 * (trlwe_new_packing1_KS_key, src/keyswitch.c:368-390), kind 1 = private key (trlwe_new_priv_SK_KS_key_N2, :611-637); rows are fresh
 * TRLWE encryptions under the binary key h_s_out[N] (exact a * s, Gaussian noise sigma, counter-based generator seeded by `seed`).
 * ksk_export_rows copies rows [first_row, first_row + count) back for inspection. */
int mosfhet_hip_trlwe_table_ksk_generate(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, int kind, const uint64_t *h_s_out, int N,
                                         const uint64_t *h_s_in, int n, int t, int base_bit, double sigma, uint64_t seed);
int mosfhet_hip_ksk_export_rows(mosfhet_hip_ksk_t ksk, size_t first_row, size_t count, uint64_t *h_out);
/* Seed-compressed form (the reference's USE_COMPRESSED_TRLWE key rows, src/keyswitch.c:231-241, regenerated by
 * trlwe_compressed_subto, src/trlwe_compressed_vaes.c:139-160): the same rows as mosfhet_hip_trlwe_table_ksk_generate makes for this seed, but
 * only the b halves stay in HBM (mosfhet_hip_ksk_bytes: half); every key switch that takes the handle regenerates the mask words inside the
 * kernel from (seed, row, word).  Results are bit-identical to the uncompressed key's.  ksk_export_rows expands the rows. */
int mosfhet_hip_trlwe_table_ksk_generate_compressed(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, int kind, const uint64_t *h_s_out, int N,
                                                    const uint64_t *h_s_in, int n, int t, int base_bit, double sigma, uint64_t seed);
/* tlwe_keyswitch_no_precomp (src/tlwe.c:305-320): key = plain device rows [n_in][t][n_out + 1], one sample per (input word, digit position), multiplied by the
 * digit in the kernel (the reference's double rounding offset included).  count <= 65535 (MOSFHET_HIP_EINVAL beyond it, before any device call). */
int mosfhet_hip_tlwe_keyswitch_no_precomp_batch(mosfhet_hip_ctx_t ctx, const uint64_t *d_rows, uint64_t *d_out, const uint64_t *d_in, int count, int n_in, int n_out,
                                                int t, int base_bit, void *stream);
/* LUT-packing key switch (trlwe_new_packing_KS_key / trlwe_packing_keyswitch, src/keyswitch.c:214-241,346-366): `torus_base` LWE samples into the `torus_base`
 * slots of one TRLWE sample.  The key is a table key with n * torus_base digit sources (ksk kind 2: export / import / alloc as such);
 * d_in [count][torus_base][n + 1], d_out [count][2][N]. */
int mosfhet_hip_trlwe_lut_packing_ksk_generate(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, const uint64_t *h_s_out /*[N]*/, int N, const uint64_t *h_s_in /*[n]*/,
                                               int n, int t, int base_bit, int torus_base, double sigma, uint64_t seed);
int mosfhet_hip_trlwe_lut_packing_keyswitch_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, int torus_base, uint64_t *d_out, const uint64_t *d_in, int count,
                                                  void *stream);
size_t mosfhet_hip_ksk_bytes(mosfhet_hip_ksk_t ksk);                     /* device bytes of a key-switch table */
/* On-device generation of the bootstrap key (new_bootstrap_key without unfolding, src/bootstrap.c:3-21: BK_i = TRGSW(s_i); ga != 0: the
 * TRGSW(X^{s_i}) samples of new_bootstrap_key_ga, src/bootstrap_ga.c:5-24) from the binary TRLWE key h_s_rlwe[N] and LWE key h_s_lwe[n]:
 * encrypted in the torus domain by the counter-based generator (exact a * s, Gaussian noise sigma), then transformed -- no host key, no upload. */
int mosfhet_hip_bsk_generate(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t *out, const uint64_t *h_s_rlwe, int N, const uint64_t *h_s_lwe, int n, int l, int Bg_bit,
                             double sigma, uint64_t seed, int ga);
/* ... for any k <= 3 and any ring the engine serves up to N = 8192 (keys of the general-ring path): h_s_rlwe = the k key polynomials [k][N]; the k + 1 components of a
 * row as trgsw_monomial_sample makes them (src/trgsw.c:152-168).  k = 1 on a tuned ring is mosfhet_hip_bsk_generate(.., ga = 0). */
int mosfhet_hip_bsk_generate_k(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t *out, const uint64_t *h_s_rlwe /*[k][N]*/, int k, int N, const uint64_t *h_s_lwe, int n, int l,
                               int Bg_bit, double sigma, uint64_t seed);
/* On-device generation of FFT-based TRLWE key-switch keys: entry e, row r < t = TRLWE_{s_out}(h_msgs[e](X) * 2^(64 - (r+1) base_bit)), then the
 * engine's forward transform.  h_msgs = Torus[entries][N] holds the polynomial each entry switches FROM: the other key (trlwe_new_KS_key,
 * src/keyswitch.c:12-37), its Galois images s(X^(2e+1)) for e < N (trlwe_new_automorphism_KS_keyset, :500-511), (-s * s_in, -s) (trlwe_new_priv_KS_key,
 * :39-50) or s^2 (trlwe_new_RL_key, :3-10). */
int mosfhet_hip_trlwe_ksk_generate(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t *out, const uint64_t *h_s_out, int N, const uint64_t *h_msgs, int entries, int t,
                                   int base_bit, double sigma, uint64_t seed);
/* On-device generation of the LWE -> LWE key-switch table of tlwe_new_KS_key (src/tlwe.c:193-212) from the two binary keys: rows
 * TLWE_{s_out}(s_in[i] v 2^(64 - (j+1) base_bit)), masks from the counter-based generator, Gaussian noise sigma.  compressed != 0 stores one word
 * per row (b) and tlwe_keyswitch regenerates the masks inside the kernel: lvl2's 1.2 GB table becomes 2 MB, results are bit-identical to the
 * uncompressed key of the same seed.  The handle works with every entry point that takes an LWE key-switch key. */
int mosfhet_hip_tlwe_ksk_generate(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, const uint64_t *h_s_out, int n_out, const uint64_t *h_s_in, int n_in, int t,
                                  int base_bit, double sigma, uint64_t seed, int compressed);

/* Kernel selection for the N = 1024 bootstraps: batches of at most `max_batch` ciphertexts run the latency-oriented kernel (one workgroup
 * of 2l wavefronts per ciphertext, ~1/3 of the latency), larger ones the throughput kernel (one wavefront per ciphertext).  Results are
 * bit-identical.  Default 512 (or env MOSFHET_HIP_TEAM_MAX); 0 disables the latency kernel. */
int mosfhet_hip_set_team_max_batch(int max_batch);
/* The throughput kernel at N = 1024 with the 2 x 2^8 gadget (SET_1): workgroups of four ciphertexts whose wavefronts stay within a key row of each other and share the
 * bootstrap-key lines in the CU's vector L1, instead of one ciphertext per workgroup.  Results are bit-identical.  mode 0 = never, 1 = for batches of at least one
 * residency round of the device (8 per CU), 4 = at any batch size, also in place of the latency kernel (for tests).  -1 = back to the default: env MOSFHET_HIP_PBS_GROUP, else the built-in choice (capi.hip: PBS_GROUP_DEFAULT; docs/SWITCHES.md). */
int mosfhet_hip_set_pbs_group(int mode);
/* ciphertexts per workgroup (1 or 4) of the throughput-kernel launch the calling thread's most recent bootstrap call made; 0 if it made none.  For tests. */
int mosfhet_hip_last_pbs_group(void);
/* the same switch-over for N = 2048 and, at half the value, N = 4096 (one workgroup of two transform teams per ciphertext; default 512, MOSFHET_HIP_WIDE_TEAM_MAX; 0 disables) */
int mosfhet_hip_set_wide_team_max_batch(int max_batch);
/* N = 2048, l = 2, 4 or 6 (l = 4: the TFHEpp lvl2 set of BASELINE.json configs[2..4]; l = 6: the radix-integer application's): batches of at most `max_batch` bootstraps take TWO CUs each (pbs_split_kernel: one workgroup per
 * accumulator component, one 16 KiB exchange per CMUX step) -- the share one GPU gets when a config's batch is sharded over eight leaves half its CUs idle otherwise.
 * -1 = half the device's CUs (default, MOSFHET_HIP_SPLIT_MAX), 0 = never.  The ONE selection that changes bits: that kernel adds the external product's rows per
 * accumulator component and then the two partial sums (src/trgsw.c:393-419 is one chain over all rows); the results differ from every other kernel's by FFT-level
 * rounding -- the tolerance the reference's own tests accept between its two FFT back-ends -- and are bit-identical to the oracle's restatement of that order
 * (oracle/oracle_tfhe.c: orc_set_product_order). */
int mosfhet_hip_set_split_max_batch(int max_batch);
/* Table key switches (tlwe_keyswitch, trlwe_packing1_keyswitch, trlwe_priv_keyswitch: src/tlwe.c:289-303, src/keyswitch.c:458-475,639-656) with 2 - 4 digit bits:
 * from `min_count` ciphertexts on they run with OUTPUT WORDS on the lanes (wave-uniform digits pick the candidate by register-relative addressing: one scalar move and
 * one 64-bit add per ciphertext, input word, digit position and output word) instead of ciphertexts on the lanes (a per-lane LDS gather).  Integer sums: the same
 * bits either way.  Default 17 = every batch the direct kernels of up to 16 ciphertexts leave (MOSFHET_HIP_KS_WORDS); 0 = never. */
int mosfhet_hip_set_ks_words(int min_count);
/* wavefronts of that kernel whose bounded wait on their workgroup's counters ran out since the library was loaded (synchronises the device): 0 unless something is broken */
int mosfhet_hip_ks_words_gave_up(mosfhet_hip_ctx_t ctx, unsigned int *count);
/* its launch plan for a shape, without a device (tests): plan = { taken at the current setting, digit positions per stage, stages per input word, LDS-DMA requests per wavefront
 * and stage, LDS bytes per workgroup, workgroups, ciphertext groups of 512, input-word splits }; compressed_lwe: seed-compressed LWE rows (they stay with the other form) */
int mosfhet_hip_ks_words_plan(int count, int n_in, int row, int t, int base_bit, int compressed_lwe, long long plan[8]);
/* how long (10 ns ticks; default 200000 = 2 ms, MOSFHET_HIP_SPLIT_LIMIT) the first workgroup of such a pair waits for its partner before it takes the whole bootstrap
 * alone (same summation order, same bits); 0 = always alone (test switch) */
int mosfhet_hip_set_split_wait_limit(int ticks);
/* of the calling host thread's last split launch (synchronises its stream): bootstraps taken by a pair of workgroups / alone */
int mosfhet_hip_split_last_launch(int *count, int *paired, int *alone);   /* (the one-CU and throughput by-component launches of a BY_COMPONENT key are no split launches and do not update it) */

/* Summation order of a bootstrap key's external products -- a property of the KEY, so that the same key and ciphertext give the same words at every batch
 * size, on every device and on every shard of a batch.
 *   AUTO          (every new key) the kernel chosen for the batch size decides: by component on the split kernels, the reference's one chain elsewhere
 *   REFERENCE     one fma chain over all 2 l rows (src/trgsw.c:393-419): the split kernels are never taken for this key, whatever
 *                 MOSFHET_HIP_SPLIT_MAX / mosfhet_hip_set_split_max_batch say
 *   BY_COMPONENT  the split kernels' order (rows 0 .. l-1 chained from zero, rows l .. 2l-1 chained from zero, one IEEE addition of the two sums) at EVERY
 *                 batch size: batches of at most split_max_batch bootstraps still take two CUs each (a matter of speed only), larger ones and launches that
 *                 find no exchange slots take the one-CU by-component kernel (the split kernel's alone path with a launch shape of its own), batches beyond
 *                 wide_team_max_batch the by-component form of the throughput kernel (pbs_kernel<.., BYC = true>; the Galois family: the one-CU kernel in residency
 *                 rounds of one workgroup per CU).  The split switches are pure performance switches for such a key.
 * Rule: the property governs every launcher family in which AUTO can pick a by-component kernel for SOME batch size: the plain bootstrap family at N = 2048
 * with l = 2, 4, 6 (programmable / functional bootstrap with and without extract, blind_rotate, row mode and every composition built on them: FDFB and its
 * KS21 / CLOT21 forms, multi-value CLOT21, key switch + bootstrap, circuit bootstraps, the vec_* callers) and the Galois family at N = 2048 with l = 4.
 * Everywhere else (other rings, odd l, Galois at l != 4, unfolded keys, the general-ring path, stand-alone external products and CMUX) results do not depend
 * on the batch size already: the setter accepts any valid value there and it changes nothing.
 * The field is read by the launchers: setting it while another thread issues launches on the key is the caller's race; keys stay read-only otherwise.
 * mosfhet_hip_bsk_clone copies it (replicas on other GPUs sum alike).  Key images and on-disk formats do not carry it (formats unchanged): set it after loading.
 * Unknown values: MOSFHET_HIP_EINVAL. */
#define MOSFHET_HIP_ORDER_AUTO          0
#define MOSFHET_HIP_ORDER_REFERENCE     1
#define MOSFHET_HIP_ORDER_BY_COMPONENT  2
int mosfhet_hip_bsk_set_product_order(mosfhet_hip_bsk_t bsk, int order);
int mosfhet_hip_bsk_get_product_order(mosfhet_hip_bsk_t bsk, int *order);
/* Which kernel family a bootstrap launch of a tuned, folded key takes, without a device: the function the launchers themselves decide with, at the current values
 * of the batch-threshold setters (team / wide_team / split max_batch, MOSFHET_HIP_ROUND_CHUNK), with `cus` in place of the device's CU count.
 * count: bootstraps of the launch (ciphertexts x rows in row mode); rows: accumulator rows per ciphertext (1 = plain); galois: 0 plain family, 1 Galois family.
 *   plan[0]  kernel family (below)      plan[1]  1 = that kernel sums by component
 *   plan[2]  launches (residency rounds) of a key that does not fit the L2s      plan[3]  reserved, 0
 * (SPLIT: a BY_COMPONENT key whose launch finds no exchange slots runs LATENCY_BY_COMPONENT instead, an AUTO key LATENCY.) */
#define MOSFHET_HIP_FAMILY_THROUGHPUT               0   /* one team per bootstrap, several per CU (pbs_kernel, pbs_ga_kernel) */
#define MOSFHET_HIP_FAMILY_LATENCY                  1   /* one workgroup of several teams per bootstrap (pbs_team / wide_team / wide_pair, pbs_ga_wide) */
#define MOSFHET_HIP_FAMILY_SPLIT                    2   /* two CUs per bootstrap (pbs_split_kernel, pbs_ga_split_kernel): by component */
#define MOSFHET_HIP_FAMILY_LATENCY_BY_COMPONENT     3   /* the one-CU by-component kernel, one launch */
#define MOSFHET_HIP_FAMILY_THROUGHPUT_BY_COMPONENT  4   /* pbs_kernel<.., BYC = true> (plain family); Galois family: the one-CU by-component kernel in rounds of one workgroup per CU */
int mosfhet_hip_bootstrap_plan(int N, int l, int Bg_bit, int count, int rows, int galois, int order, int cus, int plan[4]);
/* The throughput by-component kernel parks one partial sum per workgroup in device memory (32 KiB each, at most 128 MiB per host thread and stream, allocated at the
 * first such launch -- outside a stream capture).  When that memory is refused the launch runs the one-CU by-component kernel in residency rounds instead: the same
 * bits at about 1.8 x the time.  set_bycomp_parking(0) takes that path always (tests, and the yardstick of tools/product_order_ab.py); 1 = default. */
int mosfhet_hip_set_bycomp_parking(int on);

/* Unit-loop form of the external-product kernel on rings of two wavefronts per team (N = 2048, l = 4; trgsw_mul_trlwe_DFT, src/trgsw.c:385-423).  The
 * software-pipelined loop is taken only by the instantiation that has been soaked clean and only while its build has no scratch (capi.hip: ep_go); the plain
 * loop gives the same bits 11 % slower.  set_ep_plain_loop(1) forces the plain loop for every multi-wavefront instantiation (tests run both in one
 * process; MOSFHET_HIP_EP_PAIRS=0 does the same for a whole process).  ep_kernel_info(i, ...) reports, for the i-th such instantiation launched so far,
 * its name, the scratch bytes per lane of its pipelined build and whether the launcher takes that build; MOSFHET_HIP_EINVAL past the end. */
int mosfhet_hip_set_ep_plain_loop(int on);
int mosfhet_hip_ep_kernel_info(int i, const char **name, int *scratch_bytes, int *takes_pipelined);
/* N >= 2048 bootstraps re-align their teams per XCD every few CMUX steps (a bounded wait: timing only).  A launch whose wait ran out (the chip was shared
 * with another launch) makes the next MOSFHET_HIP_PACE_SKIP (16) paced launches of the device skip the rendezvous; this returns how many are still to skip. */
int mosfhet_hip_pace_skip_credit(mosfhet_hip_ctx_t ctx, int *credit);

/* Digit-parallel forms of the radix-integer callers of applications/multi-ciphertext-arith for M INDEPENDENT integers: the gate sequences of
 * ufhe_sl_add_integer / ufhe_sub_integer (src/integer.c:79-107,136-156), ufhe_relu_integer (src/ml.c:4-20) and ufhe_encrypted_tlwe_lut (src/lut.c:6-20), one
 * key-switch / packing-switch / bootstrap LAUNCH per carry step or tree level instead of one gate per digit and integer.  Integers are digit-major on the device:
 * [d][M][N+1] torus words, digit / (2 torus_base) per sample under the extracted TRLWE key (ufhe_encrypt_integer).  The handle borrows the keys (bootstrap key
 * n -> N, LWE key switch N -> n, LUT-packing key of torus_base slots N -> TRLWE(N); pksk may be NULL for add / sub only) and is read-only after creation.
 *   addsub: c = a + b (subtract = 0) or a - b (1) over all d digits, the carry out of the top digit dropped (equal-width operands); c must not alias a, b
 *   relu: out = in > 0 ? in : 0 for signed integers; out may alias in
 *   encrypted_lut: table[0][m] = table[selector_m][m]; d_table [size][M][N+1] is consumed, d_sel [log_B size][M][N+1] = selector digits, least significant first
 *   cmp: c[m] = 0 / 1 / 2 for a[m] < / = / > b[m] (ufhe_cmp_integer, src/integer.c:205-264); d_c [M][N+1] is the one result digit
 *   lut_cleartext: out[m] = h_lut[selector_m] for a CLEARTEXT table (ufhe_lut_integer, src/lut.c:23-47): one multi-value rotation per selector, then the tree */
typedef struct mosfhet_hip_vec *mosfhet_hip_vec_t;
int mosfhet_hip_vec_create(mosfhet_hip_ctx_t ctx, mosfhet_hip_vec_t *out, mosfhet_hip_bsk_t bsk, mosfhet_hip_ksk_t ksk, mosfhet_hip_ksk_t pksk, int torus_base);
int mosfhet_hip_vec_destroy(mosfhet_hip_vec_t vec);
int mosfhet_hip_vec_addsub(mosfhet_hip_vec_t vec, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, int M, int d, int subtract, void *stream);
int mosfhet_hip_vec_relu(mosfhet_hip_vec_t vec, uint64_t *d_out, const uint64_t *d_in, int M, int d, void *stream);
int mosfhet_hip_vec_encrypted_lut(mosfhet_hip_vec_t vec, uint64_t *d_table, const uint64_t *d_sel, int size, int M, void *stream);
int mosfhet_hip_vec_cmp(mosfhet_hip_vec_t vec, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, int M, int d, int a_signed, int b_signed, void *stream);
/*   mul: c = a * b (ufhe_mul_integer, src/integer.c:166-203): schoolbook over a's digits -- per digit one multi-value rotation, two packed product tables per integer,
 *        two bootstrap launches over all digits of b, a shifted addition and a shifted accumulation; a [da][M][N+1], b [db][M][N+1], c [dc][M][N+1], no aliasing */
/*   mux_array: out[m] = vec[selector_m][m] over arrays of `size` integers of d digits (ufhe_mux_integer_array, src/lut.c:49-64): all d trees of all M instances as ONE
 *        tree over d M instances; d_tables [size][d][M][N+1] is consumed, d_sel [log_B size][M][N+1], d_out [d][M][N+1] */
int mosfhet_hip_vec_mux_array(mosfhet_hip_vec_t vec, uint64_t *d_out, uint64_t *d_tables, const uint64_t *d_sel, int size, int d, int M, void *stream);
int mosfhet_hip_vec_sl_add(mosfhet_hip_vec_t vec, uint64_t *d_c, int dc, const uint64_t *d_a, int da, int g, const uint64_t *d_b, int db, int h, int is_signed, int M,
                           void *stream);   /* c = a B^g + b B^h (ufhe_sl_add_integer, src/integer.c:79-107) */
int mosfhet_hip_vec_extend(mosfhet_hip_vec_t vec, uint64_t *d_c, int dc, int d_ini, int is_signed, int M, void *stream);   /* digits [d_ini, dc) <- zero or sign (ufhe_extend_integer, :62-77) */
int mosfhet_hip_vec_mul(mosfhet_hip_vec_t vec, uint64_t *d_c, int dc, const uint64_t *d_a, int da, const uint64_t *d_b, int db, int is_signed, int M, void *stream);
int mosfhet_hip_vec_lut_cleartext(mosfhet_hip_vec_t vec, uint64_t *d_out, const uint64_t *d_sel, const uint64_t *h_lut, int size, int d_out_digits, int M, void *stream);

/* The canonical caller pattern in one call (applications/multi-ciphertext-arith/src/integer.c:94-95): tlwe_keyswitch kN -> n, then
 * functional_bootstrap (extract = 1: d_out [count][kN+1]) or functional_bootstrap_wo_extract (extract = 0: d_out [count][k+1][N]);
 * same stream, no host synchronisation in between. */
int mosfhet_hip_keyswitch_functional_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, mosfhet_hip_bsk_t bsk, uint64_t *d_out,
                                                     const uint64_t *d_tv, int tv_count, const uint64_t *d_in /*[count][kN+1]*/, int count,
                                                     int torus_base, int extract, void *stream);

/* ---- cleartext-weight linear layers on LWE batches, y = W x + bias (capi_linear.inc, linear_kernels.h) ----
 * The reference's tlwe_scale, tlwe_scale_addto, tlwe_scale_subto, tlwe_add and tlwe_sub (src/tlwe.c:143-191) with cleartext weights, for `count` independent
 * inferences or circuit instances at once.  Samples are n + 1 torus words, the b word last, any 1 <= n <= 65535:
 *     out[b][j][c] = (c == n ? bias[j] : 0) + sum_i W[j][i] in[b][i][c]   (mod 2^64);   d_in [count][rows_in][n+1], d_out [count][rows_out][n+1]
 * W[j][i] is the multiplier tlwe_scale takes, read as a signed 64-bit number, shared by the whole batch; bias[j] is a torus word (a trivially encrypted constant).
 * Exact integer arithmetic: no word depends on count, tiling, form (dense / sparse) or path.
 * A handle holds the weights on the device and is read-only after creation.  `narrow` (info[3], set at creation iff every weight lies in [-2^31, 2^31)) selects
 * the cheaper multiply sequence and changes no word. */
typedef struct mosfhet_hip_linear *mosfhet_hip_linear_t;
/* src/tlwe.c:143-191 as a dense layer: h_W [rows_out][rows_in], h_bias [rows_out] or NULL */
int mosfhet_hip_linear_create_dense(mosfhet_hip_ctx_t ctx, mosfhet_hip_linear_t *out, const int64_t *h_W, const uint64_t *h_bias, int rows_out, int rows_in);
/* src/tlwe.c:143-191 as a sparse map (a netlist level, a convolution, a gather): CSR, h_row_ptr [rows_out+1] (row_ptr[0] = 0, monotone), h_col / h_val [nnz];
 * columns may be unsorted and may repeat within a row (they add), rows may be empty (bias alone); columns outside [0, rows_in) are refused. */
int mosfhet_hip_linear_create_sparse(mosfhet_hip_ctx_t ctx, mosfhet_hip_linear_t *out, const int *h_row_ptr, const int *h_col, const int64_t *h_val,
                                     const uint64_t *h_bias, int rows_out, int rows_in);
int mosfhet_hip_linear_destroy(mosfhet_hip_linear_t lin);
/* info: rows_out, rows_in, nnz (-1 dense), narrow, device bytes, form (0 dense, 1 sparse) */
int mosfhet_hip_linear_info(mosfhet_hip_linear_t lin, long long info[6]);
/* a copy for another context (device), after the pattern of mosfhet_hip_ksk_clone; a handle serves the context it was made or cloned for */
int mosfhet_hip_linear_clone(mosfhet_hip_ctx_t ctx_other, mosfhet_hip_linear_t lin, mosfhet_hip_linear_t *out);
/* src/tlwe.c:143-191 over a batch: d_out = W d_in + bias.  d_out must not overlap d_in.  Queues on `stream`, never synchronises; temporaries (sparse rows of
 * more than 64 entries only) live in the calling thread's pool, so the call is capturable once a call of the same size has run. */
int mosfhet_hip_tlwe_linear_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_linear_t lin, uint64_t *d_out, const uint64_t *d_in, int n, int count, void *stream);
/* What a call of src/tlwe.c:143-191 over a batch will do (pure; no device; the function the launcher decides with).  `cus` is reserved for sizing grids: it is
 * checked (>= 1) and sizes nothing today, every unit of work being one wavefront of a flat grid.
 * plan = { form (0 dense, 1 sparse), TJ = output rows per wavefront, words per lane, workgroups, grid folds (gridDim.y; gridDim.x = ceil(workgroups / folds)),
 *          passes over the input = ceil(rows_out / TJ), input bytes read by the model = passes * count * rows_in * (n+1) * 8, multiply sequence (0 narrow, 1 wide) } */
int mosfhet_hip_tlwe_linear_plan(int rows_out, int rows_in, long long nnz /* -1 dense */, int narrow, int n, int count, int cus, long long plan[8]);
/* src/tlwe.c:143-191, then the body of mosfhet_hip_keyswitch_functional_bootstrap_batch on the count * rows_out results: d_in [count][rows_in][kN+1], d_out
 * [count * rows_out][kN+1] (extract = 1) or [count * rows_out][k+1][N] (0); tv_count is 1 or count * rows_out.  The linear map's output lives in the calling
 * thread's pool, the switched samples in the bootstrap key's scratch as in that call: one stream per host thread. */
int mosfhet_hip_linear_keyswitch_functional_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_linear_t lin, mosfhet_hip_ksk_t ksk, mosfhet_hip_bsk_t bsk,
                                                            uint64_t *d_out, const uint64_t *d_tv, int tv_count, const uint64_t *d_in /*[count][rows_in][kN+1]*/,
                                                            int count, int torus_base, int extract, void *stream);

/* ---- cleartext polynomial-weight linear layers on batches of PACKED TRLWE samples (capi_polylinear.inc; kernel: polylinear_body, trace_kernels.h) ----
 * The reference's trlwe_to_DFT, trlwe_DFT_mul_by_polynomial / trlwe_DFT_mul_addto_by_polynomial (src/trlwe.c:491-505), trlwe_from_DFT and trlwe_extract_tlwe
 * (:540-552) for `count` independent inferences at once.  One negacyclic product with the right weight polynomial is an inner product over up to N packed values,
 * a 1-D convolution, a rotation or a slot sum (mosfhet_polylinear_dot_layout, mosfhet_compat.h, lays out the first).  Ring N in {1024, 2048, 4096}, k = 1.
 * A handle holds, per output row j, an ordered list of entries (col_e, val_e) -- val_e a cleartext polynomial of N signed 64-bit coefficients -- and an optional
 * bias polynomial of N torus words.  With F = polynomial_torus_to_DFT (a weight is converted as (double)(int64_t), exactly as a torus word is),
 * G = polynomial_DFT_to_torus with the general rounding (exact for every double) and mul_addto = polynomial_mul_addto_DFT (two FMAs per part, input first):
 *     acc_a = acc_b = +0.0
 *     for e in the entries of row j, in the stored order:   acc_a = mul_addto(acc_a, F(in[b][col_e].a), F(val_e));   acc_b likewise with .b
 *     out[b][j] = (G(acc_a), G(acc_b) + bias[j])           (mod 2^64)
 * Any int64 weight is accepted.  No word depends on count, a sample's position in the batch, the workspace, the rounds, the device, the launch geometry or on whether
 * the handle was made dense or sparse with the same ordered entries.  The weights are transformed on the device at creation and kept in the engine's slot order,
 * read-only afterwards; no DFT-domain data crosses this interface. */
typedef struct mosfhet_hip_polylinear *mosfhet_hip_polylinear_t;
/* src/trlwe.c:491-505 as a dense layer: h_W [rows_out][rows_in][N], h_bias [rows_out][N] or NULL; row j's entries are col = 0 .. rows_in - 1 ascending, zero
 * polynomials are not skipped */
int mosfhet_hip_polylinear_create_dense(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t *out, const int64_t *h_W, const uint64_t *h_bias, int rows_out, int rows_in, int N);
/* src/trlwe.c:491-505 as a sparse map: CSR over polynomial blocks, h_row_ptr [rows_out+1] (row_ptr[0] = 0, monotone), h_col [nnz], h_val [nnz][N]; the rules of
 * mosfhet_hip_linear_create_sparse: columns may be unsorted and may repeat within a row (they add, in the stored order), rows may be empty ((0, bias)), columns outside
 * [0, rows_in) are refused */
int mosfhet_hip_polylinear_create_sparse(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t *out, const int *h_row_ptr, const int *h_col, const int64_t *h_val,
                                         const uint64_t *h_bias, int rows_out, int rows_in, int N);
int mosfhet_hip_polylinear_destroy(mosfhet_hip_polylinear_t lin);
/* info: rows_out, rows_in, nnz (-1 dense), N, device bytes, form (0 dense, 1 sparse) */
int mosfhet_hip_polylinear_info(mosfhet_hip_polylinear_t lin, long long info[6]);
/* a copy for another context (device), after the pattern of mosfhet_hip_linear_clone */
int mosfhet_hip_polylinear_clone(mosfhet_hip_ctx_t ctx_other, mosfhet_hip_polylinear_t lin, mosfhet_hip_polylinear_t *out);
/* src/trlwe.c:491-505 between trlwe_to_DFT and trlwe_from_DFT over a batch: d_in [count][rows_in][2][N] -> d_out [count][rows_out][2][N].  Asynchronous on `stream`,
 * never synchronises; the transformed inputs of a round live in the calling thread's pool (one stream per host thread; capturable once a call of the same size has run),
 * bounded by mosfhet_hip_set_tlwe_pack_workspace: a larger batch runs in rounds of whole batch elements.  count == 0 is OK.  MOSFHET_HIP_EINVAL, before any HIP call: null
 * ctx / lin, count < 0, null buffers with count > 0, lin of another context, d_out overlapping d_in, a round whose teams do not fit one launch, a workspace bound below
 * one batch element. */
int mosfhet_hip_trlwe_linear_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t lin, uint64_t *d_out /*[count][rows_out][2][N]*/,
                                   const uint64_t *d_in /*[count][rows_in][2][N]*/, int count, void *stream);
/* The same words followed by trlwe_extract_tlwe(., idx) (src/trlwe.c:540-552), 0 <= idx < N (else MOSFHET_HIP_EINVAL): a[i] = out.a[idx - i] for i <= idx,
 * -out.a[N + idx - i] above, b = out.b[idx].  The TRLWE result is never written; d_out is the [..][N+1] layout the key switch takes next.  count == 0 returns before
 * the handle is read: idx < 0 is refused at every count, idx >= N where there is something to do. */
int mosfhet_hip_trlwe_linear_extract_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t lin, uint64_t *d_out /*[count][rows_out][N+1]*/, const uint64_t *d_in, int idx,
                                           int count, void *stream);
/* src/trlwe.c:491-505 and :540-552 into the calling thread's pool, then the body of mosfhet_hip_keyswitch_functional_bootstrap_batch on the count * rows_out samples:
 * the same words as the two calls one after the other.  d_out [count * rows_out][N+1] (extract = 1) or [count * rows_out][2][N] (0); tv_count is 1 or
 * count * rows_out.  The handle's ring must be the key-switch key's input (else MOSFHET_HIP_EINVAL).  One stream per host thread. */
int mosfhet_hip_trlwe_linear_keyswitch_functional_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t lin, mosfhet_hip_ksk_t ksk, mosfhet_hip_bsk_t bsk,
                                                                  uint64_t *d_out, const uint64_t *d_tv, int tv_count, const uint64_t *d_in /*[count][rows_in][2][N]*/,
                                                                  int idx, int count, int torus_base, int extract, void *stream);
/* What a call of src/trlwe.c:491-505 over a batch will do (pure; no device; the function the launcher decides with).  nnz = -1: dense.  `cus` is reserved (checked >= 1).
 * workspace_bytes = 0: the current setting.  plan = { teams of the main launch of a round, batch elements per round, rounds, pool bytes per round, forward transforms
 * per call = count * rows_in * 2, inverse transforms per call = count * rows_out * 2, weight bytes one team reads, input bytes one team reads (sparse: of the mean row,
 * rounded up) } */
int mosfhet_hip_trlwe_linear_plan(int N, int rows_out, int rows_in, long long nnz, int count, int extract, int cus, long long workspace_bytes, long long plan[8]);

/* ---- ENCRYPTED polynomial-weight linear layers on batches of PACKED TRLWE samples (capi_gswlinear.inc; kernels: gsw_digits_body, gsw_sum_body, trace_kernels.h) ----
 * The layer above with the operands' roles exchanged: every weight is a TRGSW sample (private-model inference; encrypted filters, rotations and selections of packed
 * slots; products with the selectors mosfhet_hip_trgsw_from_gadget_batch and mosfhet_hip_circuit_bootstrap_3_dft_batch leave on the device), and a row of the layer
 * is a SUM of the reference's trgsw_mul_trlwe_DFT (src/trgsw.c:385-423) with one rounding.  Ring N in {1024, 2048, 4096}, k = 1, gadget (l, Bg_bit) given at creation.
 * A handle holds, per output row j, an ordered list of entries (col_e, W_e) -- W_e a TRGSW_DFT sample [2l][2][N/2] complex in the engine's slot order, rows 0 .. l - 1
 * multiplying the digits of component a and rows l .. 2l - 1 those of component b, the row order of trgsw_mul_trlwe_DFT -- and an optional bias polynomial of N torus
 * words.  With F = polynomial_torus_to_DFT, G = polynomial_DFT_to_torus with the general rounding, dec_i = polynomial_decompose_i and mul_addto =
 * polynomial_mul_addto_DFT (two FMAs per part, digit first, row second):
 *     acc_a = acc_b = +0.0
 *     for e in the entries of row j, in the stored order:   for c in (a, b):   for i in 0 .. l - 1:
 *         d = F(dec_i(in[b][col_e].c, Bg_bit, l, i));   acc_a = mul_addto(acc_a, d, W_e[c l + i].a);   acc_b = mul_addto(acc_b, d, W_e[c l + i].b)
 *     out[b][j] = (G(acc_a), G(acc_b) + bias[j])           (mod 2^64)
 * With one entry and no bias that is trgsw_mul_trlwe_DFT followed by trlwe_from_DFT, word for word (mosfhet_hip_external_product_batch at MOSFHET_HIP_ORDER_REFERENCE).
 * No word depends on count, a sample's position in the batch, the workspace, the rounds, the device, the launch geometry or on whether the handle was made dense, sparse
 * or from selectors with the same ordered entries.
 * The gadget: 1 <= l <= 6, 1 <= Bg_bit <= 31 and l * Bg_bit <= 63, else MOSFHET_HIP_EINVAL -- the range on which the digit rule of the kernels is exact: a digit is the
 * 32-bit field (uint32_t)(word >> (64 - (i + 1) Bg_bit)) & (2^Bg_bit - 1) of the word plus the gadget offset, re-centred by 2^(Bg_bit - 1) as an int, and the offset's
 * rounding term is 2^(63 - l Bg_bit). */
typedef struct mosfhet_hip_gswlinear *mosfhet_hip_gswlinear_t;
/* a dense layer: h_W [rows_out][rows_in][2l][2][N] torus words (TRGSW samples as trgsw_sample writes them), h_bias [rows_out][N] or NULL; row j's entries are col =
 * 0 .. rows_in - 1 ascending.  The rows are transformed on the device at creation exactly as mosfhet_hip_torus_to_dft_batch transforms them. */
int mosfhet_hip_gswlinear_create_dense(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t *out, const uint64_t *h_W, const uint64_t *h_bias, int rows_out, int rows_in, int N,
                                       int l, int Bg_bit);
/* a sparse map: CSR over TRGSW blocks, h_row_ptr [rows_out+1] (row_ptr[0] = 0, monotone), h_col [nnz], h_W [nnz][2l][2][N]; the rules of
 * mosfhet_hip_polylinear_create_sparse: columns may be unsorted and may repeat within a row (they add, in the stored order), rows may be empty ((0, bias)), columns outside
 * [0, rows_in) are refused */
int mosfhet_hip_gswlinear_create_sparse(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t *out, const int *h_row_ptr, const int *h_col, const uint64_t *h_W,
                                        const uint64_t *h_bias, int rows_out, int rows_in, int N, int l, int Bg_bit);
/* the same map over weights that are already on the device: d_sel_dft [nnz][2l][2][N/2] complex as mosfhet_hip_trgsw_from_gadget_batch,
 * mosfhet_hip_circuit_bootstrap_3_dft_batch or mosfhet_hip_torus_to_dft_batch wrote them; they are copied into the handle's own image (synchronises the device's null
 * stream: work that writes the selectors on another stream must have finished) */
int mosfhet_hip_gswlinear_create_from_selectors(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t *out, const double *d_sel_dft, const int *h_row_ptr, const int *h_col,
                                                const uint64_t *h_bias, int rows_out, int rows_in, int N, int l, int Bg_bit);
int mosfhet_hip_gswlinear_destroy(mosfhet_hip_gswlinear_t lin);
/* info: rows_out, rows_in, nnz (-1 dense), N, l, Bg_bit, device bytes, form (0 dense, 1 sparse, 2 from selectors) */
int mosfhet_hip_gswlinear_info(mosfhet_hip_gswlinear_t lin, long long info[8]);
/* a copy for another context (device), after the pattern of mosfhet_hip_polylinear_clone */
int mosfhet_hip_gswlinear_clone(mosfhet_hip_ctx_t ctx_other, mosfhet_hip_gswlinear_t lin, mosfhet_hip_gswlinear_t *out);
/* d_in [count][rows_in][2][N] -> d_out [count][rows_out][2][N].  Asynchronous on `stream`, never synchronises; the digit transforms of a round ([rows_in][2l][N/2]
 * complex per batch element: made once, read by all rows_out teams) live in the calling thread's pool (one stream per host thread; capturable once a call of the same
 * size has run), bounded by mosfhet_hip_set_tlwe_pack_workspace: a larger batch runs in rounds of whole batch elements.  count == 0 is OK.  MOSFHET_HIP_EINVAL, before any
 * HIP call: null ctx / lin, count < 0, null buffers with count > 0, lin of another context, d_out overlapping d_in, a round whose teams do not fit one launch, a workspace
 * bound below one batch element. */
int mosfhet_hip_trlwe_gsw_linear_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t lin, uint64_t *d_out /*[count][rows_out][2][N]*/,
                                       const uint64_t *d_in /*[count][rows_in][2][N]*/, int count, void *stream);
/* The same words followed by trlwe_extract_tlwe(., idx) (src/trlwe.c:540-552), 0 <= idx < N (else MOSFHET_HIP_EINVAL).  The TRLWE result is never written; d_out is the
 * [..][N+1] layout mosfhet_hip_keyswitch_functional_bootstrap_batch takes next on the same stream. */
int mosfhet_hip_trlwe_gsw_linear_extract_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t lin, uint64_t *d_out /*[count][rows_out][N+1]*/, const uint64_t *d_in, int idx,
                                               int count, void *stream);
/* What a call will do (pure; no device; the function the launcher decides with).  nnz = -1: dense.  `cus` is reserved (checked >= 1).  workspace_bytes = 0: the current
 * setting.  plan = { teams of the main launch of a round, batch elements per round, rounds, pool bytes per round, forward transforms per call = count * rows_in * 2l,
 * inverse transforms per call = count * rows_out * 2, weight bytes one team reads, digit bytes one team reads (sparse: of the mean row, rounded up) } */
int mosfhet_hip_trlwe_gsw_linear_plan(int N, int l, int rows_out, int rows_in, long long nnz, int count, int extract, int cus, long long workspace_bytes, long long plan[8]);

/* ---- batches of LWE samples packed into TRLWE samples: trlwe_full_packing_keyswitch over a batch (src/keyswitch.c:195-227) ----
 * pk: an FFT key-switch key set with entries = n_in (mosfhet_hip_trlwe_ksk_create / _generate; entry i switches from the constant polynomial s_in[i] -- the key
 * trlwe_new_full_packing_KS_key makes), any t and base_bit, N in {1024, 2048, 4096}.
 *   d_in [total][n_in + 1] -> d_out [outputs][2][N], outputs = ceil(total / per), 1 <= per <= N: output o packs samples o per .. min(total, (o + 1) per) - 1, sample j
 *   of it at coefficient j; coefficients from the number of samples upward carry no b word and a zero mask column; the last output may be short.
 * split = 1: output o is the reference's, word for word -- one accumulator pair over the entries i ascending and the rows j < t ascending, digits by the rounded
 * rule of polynomial_decompose_i, one inverse transform and rounding per component, out.a = -as.a, out.b[j] = in[j].b - as.b[j].  split = P > 1 (at most
 * min(n_in, 64)): the entries are cut into P consecutive parts of ceil(n_in / P) (the last one shorter), each with its own accumulator pair and rounding; the
 * rounded parts are subtracted as 64-bit integers, so that P teams work on one output.  The words depend on the inputs, the key and P only -- never on total, on
 * the position of an output in the batch, on the workspace, on the device or on the launch geometry; the call never chooses P itself.
 * Asynchronous on `stream`, never synchronises; temporaries in the calling thread's pool (ONE STREAM PER HOST THREAD at a time); capturable once a call of the same
 * size has run.  total == 0 is OK.  d_out must not overlap d_in.
 * The transposed staging ([outputs of a round][n_in][N] words) is bounded by mosfhet_hip_set_tlwe_pack_workspace (default 256 MiB, 0 restores it); a larger batch
 * runs in rounds of whole outputs.  mosfhet_hip_tlwe_pack_plan says what the launcher will do, as a pure function (no GPU):
 * plan = { outputs, split used, entries per part, outputs per round, rounds, teams of the main launch (per round), transposed-staging bytes per round, key bytes
 *          one team reads }.  split = 0 asks it to recommend one for `cus` CUs: enough parts to fill cus x (teams resident per CU at one wavefront per SIMD), never
 * fewer than 8 entries per part, never above min(n_in, 64), and 1 as soon as the outputs alone fill the chip.  workspace_bytes = 0: the current setting. */
int mosfhet_hip_tlwe_pack_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t pk, uint64_t *d_out /*[outputs][2][N]*/, const uint64_t *d_in /*[total][n_in+1]*/,
                                int total, int per, int split, void *stream);
int mosfhet_hip_tlwe_pack_plan(int N, int n_in, int t, int total, int per, int split /*0: recommend*/, int cus, long long workspace_bytes, long long plan[8]);
int mosfhet_hip_set_tlwe_pack_workspace(long long bytes);

/* ---- packed TRLWE samples opened into batches of LWE samples: trlwe_extract_tlwe (src/trlwe.c:540-552, k = 1) over a batch, the inverse layout of tlwe_pack ----
 *   d_in [outputs][2][N] -> [total] samples, outputs = ceil(total / per), 1 <= per <= N, N a power of two in 256 .. 4096: sample o per + j is
 *   trlwe_extract_tlwe(in[o], j), word for word: a[i] = in[o].a[j - i] for i <= j, -in[o].a[N + j - i] above, b = in[o].b[j].  The last input may be opened in part.
 * Pure integer work: the words depend on d_in, per and the index only.
 * mosfhet_hip_trlwe_unpack_batch writes the batch d_out [total][N + 1]; rows from `total` on are not touched.  Asynchronous on `stream`, never synchronises, allocates
 * nothing, capturable from the first call.
 * mosfhet_hip_trlwe_unpack_keyswitch_batch: every word equals mosfhet_hip_tlwe_keyswitch_batch applied to that batch, which is never written -- the pre-pass of the
 * table key switch (the transposition of the tiles, the digit entries of the word-lane form) reads the packed words directly.  ksk: an LWE -> LWE key with n_in == N
 * (stored or seed-compressed); a packing key, a key of another ring or of another context is refused.  No word depends on the form that ran, on total, on the piece
 * boundaries or on mosfhet_hip_set_ks_words.  Up to 16 samples are unpacked into the calling thread's pool and take the direct kernels.
 * mosfhet_hip_unpack_keyswitch_functional_bootstrap_batch: that call followed by the body of mosfhet_hip_keyswitch_functional_bootstrap_batch on the `total` switched
 * samples (k = 1) -- the same scratch, the same words as the two calls one after the other.
 * Both: asynchronous, temporaries in the key-switch workspace of the calling thread (ONE STREAM PER HOST THREAD at a time), capturable once a call of the same size
 * has run.  total == 0 is OK.  d_out must not overlap d_in.
 * mosfhet_hip_trlwe_unpack_plan says what the launchers will do, as a pure function (no GPU; n_out = 0 asks about mosfhet_hip_trlwe_unpack_batch alone):
 * plan = { outputs, form of the switch (0: up to 16 samples, unpacked first; 1: word-lane; 2: tiles of 256; 3: tiles of 512 -- launch_tlwe_keyswitch's own decision at
 *          the current mosfhet_hip_set_ks_words), pieces (word-lane: ceil(total / 8192)), workgroups of the source pre-pass, bytes the pre-pass writes, bytes of the
 *          [total][N + 1] batch that is not written, pool bytes used, samples per workgroup of mosfhet_hip_trlwe_unpack_batch's kernel }. */
int mosfhet_hip_trlwe_unpack_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out /*[total][N+1]*/, const uint64_t *d_in /*[outputs][2][N]*/, int N, int total, int per, void *stream);
int mosfhet_hip_trlwe_unpack_keyswitch_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, uint64_t *d_out /*[total][n_out+1]*/, const uint64_t *d_in /*[outputs][2][N]*/,
                                             int total, int per, void *stream);
int mosfhet_hip_unpack_keyswitch_functional_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, mosfhet_hip_bsk_t bsk, uint64_t *d_out, const uint64_t *d_tv,
                                                            int tv_count, const uint64_t *d_in /*[outputs][2][N]*/, int total, int per, int torus_base, int extract,
                                                            void *stream);
int mosfhet_hip_trlwe_unpack_plan(int N, int n_out, int t, int base_bit, int compressed, int total, int per, int cus, long long plan[8]);
/* The same three calls and the plan with a geometry (per, first, stride): sample o per + j is trlwe_extract_tlwe(in[o], first + j stride), word for word -- what
 * opens the samples mosfhet_hip_tlwe_trace_pack_many_batch puts at coefficients j N / 2^L (first 0, stride N / 2^L) and the valid outputs of a packed convolution.
 * 1 <= per, 0 <= first < N, 1 <= stride and first + (per - 1) stride <= N - 1, evaluated in 64 bits: coefficient indices do not wrap; anything else returns
 * MOSFHET_HIP_EINVAL with a message naming the argument, before any HIP call.  The calls above are (first 0, stride 1) of the same bodies.  Same contracts as their
 * twins: asynchronous, the same pool slots and ONE STREAM PER HOST THREAD, the same refusals, the same capturability, total == 0 is OK.  The words depend on d_in, the
 * geometry and the sample index only.  The plan's fields do not depend on first or stride: it equals mosfhet_hip_trlwe_unpack_plan at the same (total, per)
 * whenever the geometry is accepted. */
int mosfhet_hip_trlwe_unpack_strided_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out /*[total][N+1]*/, const uint64_t *d_in /*[outputs][2][N]*/, int N, int total, int per,
                                           int first, int stride, void *stream);
int mosfhet_hip_trlwe_unpack_strided_keyswitch_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, uint64_t *d_out /*[total][n_out+1]*/,
                                                     const uint64_t *d_in /*[outputs][2][N]*/, int total, int per, int first, int stride, void *stream);
int mosfhet_hip_unpack_strided_keyswitch_functional_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, mosfhet_hip_bsk_t bsk, uint64_t *d_out,
                                                                    const uint64_t *d_tv, int tv_count, const uint64_t *d_in /*[outputs][2][N]*/, int total, int per,
                                                                    int first, int stride, int torus_base, int extract, void *stream);
int mosfhet_hip_trlwe_unpack_strided_plan(int N, int n_out, int t, int base_bit, int compressed, int total, int per, int first, int stride, int cus, long long plan[8]);
/* mosfhet_hip_trlwe_linear_batch into the calling thread's pool, then mosfhet_hip_unpack_strided_keyswitch_functional_bootstrap_batch on its count * rows_out results,
 * `per` samples of each: the same words as the two calls one after the other.  d_out [count * rows_out * per][N+1] (extract = 1) or [..][2][N] (0); tv_count is 1
 * or count * rows_out * per.  The handle's ring must be the key-switch key's input ring (else MOSFHET_HIP_EINVAL).  One stream per host thread. */
int mosfhet_hip_trlwe_linear_unpack_keyswitch_functional_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t lin, mosfhet_hip_ksk_t ksk, mosfhet_hip_bsk_t bsk,
                                                                         uint64_t *d_out, const uint64_t *d_tv, int tv_count,
                                                                         const uint64_t *d_in /*[count][rows_in][2][N]*/, int per, int first, int stride, int count,
                                                                         int torus_base, int extract, void *stream);

/* ---- the LWE -> TRLWE switch by the trace and the gadget -> TRGSW conversion over batches (src/keyswitch.c:526-546, 65-97, 559-572) ----
 * tks: an FFT key-switch key set (mosfhet_hip_trlwe_ksk_create / _generate), any t and base_bit, k = 1, N in {1024, 2048, 4096}; `entry0` names the first entry a call
 * uses, so that one set can hold several keys.  All three: one launch, asynchronous on `stream`, no allocation, no synchronisation, capturable from the first call;
 * count == 0 is OK; bad arguments return MOSFHET_HIP_EINVAL before any HIP call.
 *
 * mosfhet_hip_tlwe_trace_pack_batch: trlwe_packing1_keyswitch_CDKS21 over a batch, d_in [count][N + 1] -> d_out [count][2][N].  Entries entry0 + j, j < log2 N, switch
 * from s(X^(N / 2^j + 1)) to s (the order of trlwe_new_packing1_KS_key_CDKS21); the set must hold entry0 + log2 N entries.  Per sample: out = (a', in.b X^0) with
 * a'[0] = in.a[0], a'[N - i] = -in.a[i]; then for j = 0 .. log2 N - 1: out += KeySwitch_j(out(X^(N / 2^j + 1))), KeySwitch = trlwe_keyswitch.  Every word equals that
 * sequence made of polynomial_permute, mosfhet_hip_trlwe_keyswitch_batch and an addition (rows 0 .. t - 1 in one chain, one rounding per component and step).
 * THE INPUT MUST LIE UNDER THE EXTRACTED RING KEY (trlwe_extract_tlwe_key of the key the set switches to) -- what bootstraps write: the trace adds the un-switched
 * accumulator to its switched image, so a sample under an independent LWE key decrypts to noise.  The phase of the result is N m at coefficient 0 (the trace
 * multiplies by N) and 0 elsewhere, up to the key-switch noise.  d_out must not overlap d_in.
 *
 * mosfhet_hip_trlwe_rlwe_priv_keyswitch_batch: trlwe_RLWE_priv_keyswitch over a batch, [count][2][N] -> [count][2][N]: TRLWE(m) -> TRLWE(m v).  Entry entry0 switches
 * from s_in v, entry entry0 + 1 from v (trlwe_new_RLWE_priv_KS_key).  out = sum_j dec_j(in.b) KS1_j - sum_j dec_j(in.a) KS0_j: two passes, each with its own
 * accumulators, inverse transforms and rounding -- the two trlwe_keyswitch calls, the negation and the addition of the reference, word for word.  d_out may be d_in.
 *
 * mosfhet_hip_trgsw_from_gadget_batch: trgsw_from_gadget over a batch: d_gadget [count][l][2][N], row i = TRLWE(m 2^(64 - (i + 1) Bg_bit)), -> d_out_dft
 * [count][2l][2][N/2] complex in the engine's slot order -- the d_sel_dft of the leveled-LUT calls, an entry of a bootstrap key (what mosfhet_hip_bsk_create_from_device makes of the same rows in the torus domain;
 * mosfhet_hip_bsk_view_create takes it as it is).  Row i < l is
 * the forward transform of the private switch of gadget row i (the key of v = -s: trlwe_new_gadget_to_RGSW_KS), row l + i that of gadget row i itself, both exactly
 * as mosfhet_hip_torus_to_dft_batch transforms the torus words; no torus-domain word is written.  1 <= l <= 6; count * l teams.
 *
 * mosfhet_hip_trace_plan checks a shape as the calls do, as a pure function (no GPU): kind 0 trace pack, 1 private switch, 2 TRGSW from gadget (l is read for kind 2
 * only), `entries` what the set holds.  plan = { key entries a team reads, teams of the launch, threads per team, forward transforms per team, inverse transforms per
 * team, key bytes a team reads }. */
int mosfhet_hip_tlwe_trace_pack_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t tks, int entry0, uint64_t *d_out /*[count][2][N]*/, const uint64_t *d_in /*[count][N+1]*/,
                                      int count, void *stream);
int mosfhet_hip_trlwe_rlwe_priv_keyswitch_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t tks, int entry0, uint64_t *d_out /*[count][2][N]*/, const uint64_t *d_in, int count,
                                                void *stream);
int mosfhet_hip_trgsw_from_gadget_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t tks, int entry0, double *d_out_dft /*[count][2l][2][N/2] complex*/,
                                        const uint64_t *d_gadget /*[count][l][2][N]*/, int l, int count, void *stream);
int mosfhet_hip_trace_plan(int kind, int N, int t, int base_bit, int entries, int entry0, int l, int count, long long plan[6]);

/* ---- many LWE samples packed into one TRLWE sample by the trace (PackLWEs of the paper trlwe_packing1_keyswitch_CDKS21 comes from) ----
 * Same key set as mosfhet_hip_tlwe_trace_pack_batch (log2 N entries from entry0 on, k = 1, N in {1024, 2048, 4096}, any t), no other key material.
 * d_in [total][N + 1], n = 2^log_per, L = log_per, 0 <= L <= log2 N, outputs = ceil(total / n), d_out [outputs][2][N]; output o takes samples o n .. o n + n - 1, a sample
 * index >= total stands for the all-zero sample (the last output only).  With embed the embedding of the trace call (a'[0] = a[0], a'[N - i] = -a[i], b X^0),
 * KeySwitch_e = trlwe_keyswitch with entry entry0 + e (rows 0 .. t - 1 in one chain, one rounding per component), X^s p the exact negacyclic shift of both components
 * and every addition mod 2^64:
 *
 *   P_0[j] = embed(in[o n + j])                                    j < n
 *   for lvl = 1 .. L:                                              n / 2^lvl results per output
 *       E = P_{lvl-1}[r],   O = X^(N / 2^lvl) * P_{lvl-1}[r + n / 2^lvl]        r < n / 2^lvl
 *       U = E + O,  V = E - O
 *       P_lvl[r] = U + KeySwitch_{log2 N - lvl}( V(X^(2^lvl + 1)) )
 *   acc = P_L[0]
 *   for j = 0 .. log2 N - L - 1:   acc += KeySwitch_j( acc(X^(N / 2^j + 1)) )   -- the trace step
 *   out[o] = acc
 *
 * Every call uses each of the log2 N entries once (level lvl entry log2 N - lvl, the tail entries 0 .. log2 N - L - 1).  The phase N m_j of sample j lands at coefficient
 * j N / n, every other coefficient has phase 0 up to the key-switch noise.  log_per = 0 is mosfhet_hip_tlwe_trace_pack_batch word for word.  THE INPUTS MUST LIE UNDER THE
 * EXTRACTED RING KEY, as there.  n - 1 merges and log2 N - L trace steps per output, each one automorphism and one FFT key switch: one launch per level, one team per
 * merge, the last level's launch runs the tail with the accumulator on chip; at level 1 the two leaves are embedded as they are read.
 *
 * Asynchronous on `stream`, never synchronises.  Levels 1 .. L - 1 live in the calling thread's pool (one stream per host thread; capturable once a call of the same size
 * has run), bounded by mosfhet_hip_set_tlwe_pack_workspace: level 1 holds n / 2 TRLWE samples per output, level 2 n / 4 beside it, later levels reuse the two regions;
 * a larger batch runs in rounds of whole outputs.  No word depends on total, on an output's position, on the rounds or on what the pool held.  MOSFHET_HIP_EINVAL, before
 * any HIP call: null ctx / tks, total < 0, entry0 < 0, log_per outside 0 .. log2 N, a set shorter than entry0 + log2 N, null buffers with total > 0, d_out overlapping
 * d_in, tks of another context, a workspace bound below one output's levels, a level whose teams do not fit one launch.  total == 0 is OK.
 *
 * mosfhet_hip_tlwe_trace_pack_many_plan: the launcher's own decision as a pure function (no GPU); workspace_bytes = 0: the current setting.  plan = { outputs, launches
 * per round, teams of the first launch of a round, merge steps per output (n - 1), tail steps (log2 N - L), outputs per round, rounds, pool bytes per round }. */
int mosfhet_hip_tlwe_trace_pack_many_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t tks, int entry0, uint64_t *d_out /*[outputs][2][N]*/, const uint64_t *d_in /*[total][N+1]*/,
                                           int total, int log_per, void *stream);
int mosfhet_hip_tlwe_trace_pack_many_plan(int N, int t, int base_bit, int entries, int entry0, int total, int log_per, long long workspace_bytes /*0: current setting*/,
                                          long long plan[8]);

/* CMUX over a batch with one shared selector = entry `key_index` of a key handle (e.g. circuit-bootstrap outputs turned into a handle by
 * mosfhet_hip_bsk_create_from_device): d_out[b] = d_in0[b] + key (.) (d_in1[b] - d_in0[b]); d_out may alias d_in0.  The leveled caller of
 * the path (applications/leveled_lut/vertical_packing.c:24-52: CMUX tree, then blind_rotate with the selectors as key). */
int mosfhet_hip_cmux_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, int key_index, uint64_t *d_out /*[count][2][N]*/, const uint64_t *d_in0,
                           const uint64_t *d_in1, int count, void *stream);

/* Leveled look-up-table evaluation for a batch of INDEPENDENT inputs against ONE shared table: eval_LUT of the reference's leveled application
 * (applications/leveled_lut/vertical_packing.c:36-52) with input = the selectors of input b, for b < count.  (mosfhet_hip_cmux_batch and
 * mosfhet_hip_blind_rotate_batch share one selector / one key over their batch: one encrypted input, many table copies.)
 *   d_sel_dft  [count][size][2l][2][N/2] complex, engine slot order: selector i of input b encrypts bit i (least significant first, vertical_packing.c:16-20)
 *              of b's index -- the layout of `size` consecutive bootstrap-key entries, i.e. what mosfhet_hip_torus_to_dft_batch makes of
 *              mosfhet_hip_circuit_bootstrap_3_batch's [count * size][2l][2][N]
 *   d_lut      [n_luts][2][N] torus-domain TRLWEs, n_luts = max(1, 2^size / N), trivial or encrypted; READ ONLY (the reference destroys its table, a batch
 *              needs it for every input)
 *   d_out      [count][N + 1]: SampleExtract_0 of the rotated survivor
 * Per input: tree level i = 0 .. size - log2(N) - 1 halves the table with selector size - i - 1, T[j] <- T[j] + sel (.) (T[j + half] - T[j]); then blind_rotate of
 * T[0] with a[i] = int2torus(2N - 2^i, log2(2N)) and the first min(size, log2 N) selectors as key; then trlwe_extract_tlwe(.., 0).  Level 0's differences, their
 * gadget digits and forward transforms are the same for every input and are made once per call.
 * k = 1, N in {1024, 2048}, 1 <= l <= 6, Bg_bit <= 31, l * Bg_bit < 64, 1 <= size <= log2(N) + MOSFHET_HIP_LUT_MAX_LEVELS; anything else MOSFHET_HIP_EINVAL with a
 * message, before any HIP call.
 * Summation order: every external product is one chain over rows 0 .. 2l-1, the reference's order, rounded with the reduction mod 1 (the selectors are
 * caller-held DFT content without a magnitude bound).  These launches consult no key handle, so the by-component order (MOSFHET_HIP_ORDER_BY_COMPONENT) never
 * applies here.  No output word depends on count or on the chunking below.
 * Asynchronous on `stream`.  The prepared table rows and the tree's intermediates live in the CALLING THREAD's pool (one set of buffers per host thread and
 * device): no allocation and no synchronisation from the second call of a shape on -- and therefore ONE STREAM PER HOST THREAD at a time for this call: a thread
 * that queues two calls on two streams that may overlap must wait for the first before it issues the second.  (The first call of a larger shape allocates, which
 * synchronises the device and cannot run inside a stream capture.)
 * A batch whose intermediates ([count][2^(levels-1)][2][N] words) exceed the workspace bound (1 GiB; mosfhet_hip_set_leveled_lut_workspace, 0 = default; results
 * do not depend on it) is cut into chunks of whole inputs.  mosfhet_hip_leveled_lut_plan says what the launcher will do, as a pure function (no GPU):
 * plan = {tree levels = max(0, size - log2 N), first-level nodes = 2^(levels - 1) (0 without a tree), inputs per chunk, workspace bytes}; `cus` (the device's
 * CU count) sizes the grids only and changes none of the four. */
#define MOSFHET_HIP_LUT_MAX_LEVELS 10
int mosfhet_hip_leveled_lut_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const double *d_sel_dft, const uint64_t *d_lut, int size, int N, int l, int Bg_bit,
                                  int count, void *stream);
int mosfhet_hip_leveled_lut_plan(int N, int l, int size, int count, int cus, long long *plan /*[4]*/);
int mosfhet_hip_set_leveled_lut_workspace(long long bytes);

/* The same evaluation for SEVERAL shared tables over the same selectors: an n-bit -> m-bit function is m tables, more precision than one table carries is
 * several, and feeding a result back into the leveled pipeline takes one LWE sample per output bit.  One call fetches the selectors -- the expensive operand,
 * 2l * 2 * N/2 complex per bit of every input -- once for all tables where `tables` calls of mosfhet_hip_leveled_lut_batch fetch them `tables` times.
 *   d_sel_dft  [count][size][2l][2][N/2] complex: exactly the layout of mosfhet_hip_leveled_lut_batch
 *   d_luts     [tables][n_luts][2][N], n_luts = max(1, 2^size / N), trivial or encrypted; READ ONLY
 *   d_out      [count][tables][N + 1], input-major: as [count * tables][N + 1] it is the batch mosfhet_hip_tlwe_keyswitch_batch and then
 *              mosfhet_hip_circuit_bootstrap_3_batch take as "bit tb of input b", with no repacking
 * d_out[b][tb] is word for word what mosfhet_hip_leveled_lut_batch writes to d_out[b] when given table tb alone: the same summation order (one chain over rows
 * 0 .. 2l-1, the reference's, rounded with the reduction mod 1), no key handle consulted, and no word depends on count, on tables or on the passes, chunks and
 * groups below.  Arguments as for mosfhet_hip_leveled_lut_batch plus 1 <= tables <= MOSFHET_HIP_LUT_MAX_TABLES; anything else MOSFHET_HIP_EINVAL with a message
 * naming the argument, before any HIP call; count == 0 returns MOSFHET_HIP_OK.
 * Asynchronous on `stream`.  The workspace comes from the CALLING THREAD's pool, the one mosfhet_hip_leveled_lut_batch draws from: ONE STREAM PER HOST THREAD at a
 * time for these two calls together -- a thread that queues two of them on two streams that may overlap must wait for the first before it issues the second.
 * Workspace bound: the one of mosfhet_hip_set_leveled_lut_workspace.  Per table the prepared rows [nodes][2l][N/2] complex and the intermediates
 * [chunk][nodes][2][N] as in the one-table call; when all tables do not fit beside one input the call runs in passes over groups of tables (each pass reads the
 * selectors again), within a pass in chunks of whole inputs; it refuses only when one table with one input does not fit.
 * The finish runs one workgroup per (input, group of G tables) with the G accumulators in LDS; G comes from mosfhet_hip_set_leveled_lut_tables_group (0 = the
 * default), capped by what the LDS of a CU holds (8 at N = 1024, 3 at N = 2048) and by the tables of a pass.  Results do not depend on it.
 * mosfhet_hip_leveled_lut_tables_plan says what the launcher will do, as a pure function (no GPU): plan = {tree levels, first-level nodes per table, inputs per
 * chunk, tables per pass, workspace bytes = tables per pass * (prepared rows + chunk * intermediates), tables per finishing workgroup}; `cus` sizes grids only. */
#define MOSFHET_HIP_LUT_MAX_TABLES 64
int mosfhet_hip_leveled_lut_tables_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const double *d_sel_dft, const uint64_t *d_luts, int size, int N, int l, int Bg_bit,
                                         int tables, int count, void *stream);
int mosfhet_hip_leveled_lut_tables_plan(int N, int l, int size, int tables, int count, int cus, long long *plan /*[6]*/);
int mosfhet_hip_set_leveled_lut_tables_group(int group);

/* circuit_bootstrap_3 followed by trgsw_to_DFT (src/bootstrap.c:346-366, src/trgsw.c:345-349) in one call, the TRGSWs never written in the torus domain:
 * d_out_dft [count][2l][2][N/2] complex is word for word mosfhet_hip_torus_to_dft_batch of mosfhet_hip_circuit_bootstrap_3_batch's [count][2l][2][N]; as
 * [count / size][size][2l][2][N/2] it is the d_sel_dft of the leveled LUT calls.  Arguments, refusals, bootstrap launch (the key's product order governs it
 * exactly as there) and the choice between one packing switch for all levels and one per level are those of mosfhet_hip_circuit_bootstrap_3_batch; the private key
 * switch transforms its result (rows i < l) and its input (rows l + i) itself.  N in {1024, 2048, 4096}.  Asynchronous on `stream`; temporaries in the calling
 * thread's pool as for mosfhet_hip_circuit_bootstrap_3_batch. */
int mosfhet_hip_circuit_bootstrap_3_dft_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_gak_t kska, mosfhet_hip_ksk_t kskb,
                                              double *d_out_dft /*[count][2l][2][N/2] complex*/, const uint64_t *d_in /*[count][n+1]*/, int count, void *stream);

/* An n-bit -> m-bit function on inputs given as LWE-encrypted bits, LWE-encrypted bits out: circuit bootstrap + vertical packing, the loop of the reference's
 * leveled application (applications/leveled_lut/main.c: circuit_bootstrap_3 src/bootstrap.c:346-366, trgsw_to_DFT src/trgsw.c:345-349, eval_LUT
 * vertical_packing.c:36-52, tlwe_keyswitch src/tlwe.c:289-320) for `count` inputs in one call.  An S-box is size = tables = 8.
 *   d_in     [count][size][n + 1]: bit i of input b, least significant first, encoded as the circuit bootstrap takes it
 *   d_luts   [tables][n_luts][2][N], n_luts = max(1, 2^size / N), as for mosfhet_hip_leveled_lut_tables_batch; READ ONLY
 *   ksk_out  an LWE -> LWE key N -> n (mosfhet_hip_ksk_create with n_in = N, n_out = bsk's n), or NULL
 *   d_out    with ksk_out [count][tables][n + 1] -- exactly the d_in of the next call when tables == size; without it [count][tables][N + 1]
 * Ring and gadget come from bsk (the selectors a circuit bootstrap makes carry the bootstrap key's l, Bg_bit); kska / kskb as for
 * mosfhet_hip_circuit_bootstrap_3_batch.  Per chunk of whole inputs: mosfhet_hip_circuit_bootstrap_3_dft_batch on the chunk's chunk * size bits into the selector
 * workspace, mosfhet_hip_leveled_lut_tables_batch on those selectors, and with ksk_out mosfhet_hip_tlwe_keyswitch_batch of the chunk's [chunk * tables][N + 1].
 * N in {1024, 2048}; size, tables, l, Bg_bit as in mosfhet_hip_leveled_lut_tables_batch; anything else MOSFHET_HIP_EINVAL with a message naming the argument.  Null
 * handles and the ranges of size (1 .. 21), tables and count are checked before any handle is read and before any HIP call; count == 0 returns MOSFHET_HIP_OK.
 * Words: for a key whose product order is MOSFHET_HIP_ORDER_REFERENCE or _BY_COMPONENT no output word depends on count, on the bound below or on the chunking,
 * and every word equals the four calls above made one after the other on the whole batch.  For an AUTO key the kernel chosen for the launched batch -- here: the
 * bits of one chunk -- decides, as for every AUTO launch: a caller who wants chunk-independent words sets the order.
 * Asynchronous on `stream`: no synchronisation, and no allocation from the second call of a shape on.  The selector workspace [chunk][size][2l][2][N/2] complex
 * (and, with ksk_out, the chunk's [chunk * tables][N + 1]) lives in the CALLING THREAD's pool beside the leveled LUT's: ONE STREAM PER HOST THREAD at a time for
 * this call and the leveled LUT calls together.  The first call of a larger shape allocates, which synchronises the device and cannot run inside a stream capture.
 * Bound of the selector workspace: 2 GiB (mosfhet_hip_set_lut_bits_workspace, 0 = default) -- 8192 bits at lvl2's gadget; `chunk` is the largest number of whole
 * inputs whose selectors fit (at most 2^20 bits per launch), and at least 1: one input always runs.  The LUT call inside a chunk keeps its own bound, passes and
 * chunks.  mosfhet_hip_lut_bits_plan is the function the launcher uses, pure (no GPU), `cus` sizes grids only: plan = {inputs per chunk, chunks, selector bytes per
 * chunk, bits per circuit-bootstrap launch, then the six fields of mosfhet_hip_leveled_lut_tables_plan for a chunk}. */
int mosfhet_hip_lut_bits_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_gak_t kska, mosfhet_hip_ksk_t kskb, mosfhet_hip_ksk_t ksk_out /* or NULL */,
                               uint64_t *d_out, const uint64_t *d_luts, const uint64_t *d_in, int size, int tables, int count, void *stream);
int mosfhet_hip_lut_bits_plan(int N, int l, int size, int tables, int count, int cus, long long *plan /*[10]*/);
int mosfhet_hip_set_lut_bits_workspace(long long bytes);

/* Several OUTPUTS packed into one table (CGGI's other packing): a table entry occupies m = 2^pack_log adjacent coefficients, the m output bits of that entry, so an
 * n-bit -> m-bit function is ONE table with ONE rotation chain where the calls above run m tables with m chains.  An S-box at N = 2048 is exactly one TRLWE
 * (256 entries x 8 bits): no tree, 8 rotate steps, 8 extractions.
 *   d_sel_dft  [count][size][2l][2][N/2] complex: exactly the layout of mosfhet_hip_leveled_lut_batch
 *   d_luts     [tables][n_luts][2][N], n_luts = max(1, 2^(size + pack_log) / N): output t of entry x of table tb is coefficient (x m + t) mod N of TRLWE
 *              (x m + t) / N; trivial or encrypted; READ ONLY.  When 2^(size + pack_log) < N the coefficients behind the table are never selected.
 *   d_out      [count][tables][m][N + 1]: as [count * tables * m][N + 1] it is "bit tb m + t of input b", the batch mosfhet_hip_tlwe_keyswitch_batch takes next
 * Per input: tree levels i = 0 .. levels - 1, levels = max(0, size - (log2 N - pack_log)), level i with selector size - i - 1 over 2^(levels - i - 1) nodes; then
 * blind_rotate of node 0 with a[i] = int2torus(2N - 2^(i + pack_log), log2(2N)) and the first steps = min(size, log2 N - pack_log) selectors; then
 * trlwe_extract_tlwe(.., t) (src/trlwe.c:540-552) for t < m.  Summation order and rounding are those of the calls above; no key handle is consulted; no word
 * depends on count, tables, passes, chunks or groups.  pack_log == 0 IS mosfhet_hip_leveled_lut_tables_batch.
 * Arguments as for mosfhet_hip_leveled_lut_tables_batch, with 0 <= pack_log <= log2 N - 1 and size + pack_log <= log2 N + MOSFHET_HIP_LUT_MAX_LEVELS; anything else
 * MOSFHET_HIP_EINVAL with a message naming the argument, before any HIP call; count == 0 returns MOSFHET_HIP_OK.  Stream, pool, workspace bound, passes, chunks and
 * groups are those of mosfhet_hip_leveled_lut_tables_batch at the packed number of levels.
 * mosfhet_hip_leveled_lut_packed_plan is the function the launcher uses, pure (no GPU), `cus` sizes grids only: plan = {the six fields of
 * mosfhet_hip_leveled_lut_tables_plan at the packed levels and nodes, rotate steps, outputs per input = tables * m}. */
int mosfhet_hip_leveled_lut_packed_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const double *d_sel_dft, const uint64_t *d_luts, int size, int N, int l, int Bg_bit,
                                         int tables, int pack_log, int count, void *stream);
int mosfhet_hip_leveled_lut_packed_plan(int N, int l, int size, int tables, int pack_log, int count, int cus, long long *plan /*[8]*/);
/* mosfhet_hip_lut_bits_batch with the packed call as its middle: tables * m output bits per input.  d_luts as above; d_out with ksk_out [count][tables * m][n + 1]
 * -- the d_in of the next call when tables * m == size -- and without it [count][tables * m][N + 1].  Everything else (keys, chunks, selector workspace of `size`
 * selectors per input, words, stream) as for mosfhet_hip_lut_bits_batch; the staging in front of the output key switch is [chunk][tables * m][N + 1].  Null handles
 * and the ranges of size, pack_log (0 .. 10, size + pack_log <= 21), tables and count are checked before any handle is read; pack_log == 0 IS
 * mosfhet_hip_lut_bits_batch.  A round is still almost all circuit bootstrap: this variant closes the interface, it does not shorten the round.
 * plan = {the four fields of mosfhet_hip_lut_bits_plan, then the eight of mosfhet_hip_leveled_lut_packed_plan for a chunk}. */
int mosfhet_hip_lut_bits_packed_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_gak_t kska, mosfhet_hip_ksk_t kskb, mosfhet_hip_ksk_t ksk_out /* or NULL */,
                                      uint64_t *d_out, const uint64_t *d_luts, const uint64_t *d_in, int size, int tables, int pack_log, int count, void *stream);
int mosfhet_hip_lut_bits_packed_plan(int N, int l, int size, int tables, int pack_log, int count, int cus, long long *plan /*[12]*/);

/* Encrypted memory (the leveled RAM of the TFHE papers): every input b owns cells = 2^size TRLWE samples, read and written at an ENCRYPTED address.
 *   d_mem      [count][cells][2][N] torus words
 *   d_sel_dft  [count][size][2l][2][N/2] complex: exactly the layout of mosfhet_hip_leveled_lut_batch; selector j of input b encrypts bit j of b's address,
 *              least significant first
 * (.) below is the external product of mosfhet_hip_leveled_lut_batch: one chain over rows 0 .. 2l-1, rounded with the reduction mod 1.
 * READ: d_out[b] is [2][N]; d_mem is never written.
 *     T = mem[b];  for t = 0 .. size-1, half = 2^(size-1-t):  T[j] = T[j] + sel[b][size-1-t] (.) (T[j + half] - T[j]) for j < half;  out[b] = T[0]
 *   The phase of out[b] is that of mem[b][address of b].  `size` launches per chunk of inputs: the first level reads the memory and writes a workspace of
 *   [chunk][cells / 2][2][N] words, the last writes d_out (size = 1: one launch, no workspace).
 * WRITE: d_val is [count][2][N]; d_mem is updated in place, every cell i of every input independently:
 *     v = val[b];  for j = 0 .. size-1:  bit j of i set:  v = mem[b][i] + sel[b][j] (.) (v - mem[b][i]);  else:  v = v + sel[b][j] (.) (mem[b][i] - v);  mem[b][i] = v
 *   The phase of the cell is that of val[b] where i is b's address and that of the old cell elsewhere, both with the noise of `size` products added.  One launch,
 *   one workgroup per (input, cell), no workspace.  (Computed as e = v - mem[b][i], which gives the same words: e = sel (.) e, or e = e + sel (.) (-e).)
 * No word depends on count, on a sample's position in the batch, on the chunking or on the workspace bound.
 * k = 1, N in {1024, 2048}, 1 <= l <= 6, Bg_bit <= 31, l * Bg_bit < 64, 1 <= size <= MOSFHET_HIP_LUT_MAX_LEVELS, count >= 0 (0: nothing is done); d_out and d_val
 * must not overlap d_mem as address ranges; a workspace bound (mosfhet_hip_set_leveled_lut_workspace) below one input's intermediates is refused: anything else
 * MOSFHET_HIP_EINVAL with a message naming the argument, before any HIP call.
 * Asynchronous on `stream`.  The read's workspace lives in the CALLING THREAD's pool: no allocation and no synchronisation from the second call of a shape on
 * (capturable from then on) -- and therefore ONE STREAM PER HOST THREAD at a time, as for mosfhet_hip_leveled_lut_batch.  A batch whose intermediates exceed the
 * bound runs in chunks of whole inputs.
 * mosfhet_hip_trlwe_ram_plan says what the launchers will do, as a pure function (no GPU; `cus` sizes grids only): plan = {cells, launches, inputs per chunk,
 * workspace bytes (chunk * cells / 2 * 2N * 8 for a read of size > 1, else 0), external products (read: count * (cells - 1); write: count * cells * size)}. */
int mosfhet_hip_trlwe_ram_read_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out /*[count][2][N]*/, const double *d_sel_dft, const uint64_t *d_mem, int size, int N, int l,
                                     int Bg_bit, int count, void *stream);
int mosfhet_hip_trlwe_ram_write_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_mem, const double *d_sel_dft, const uint64_t *d_val /*[count][2][N]*/, int size, int N, int l,
                                      int Bg_bit, int count, void *stream);
int mosfhet_hip_trlwe_ram_plan(int N, int l, int size, int count, int write, int cus, long long *plan /*[5]*/);

/* Encrypted automata: a deterministic weighted finite automaton -- more generally a layered branching program -- run over a word whose symbols are ENCRYPTED bits
 * (the third leveled primitive of the TFHE papers, next to the look-up table and the memory above).  Cost: `states` CMUXes per symbol.
 * Ring and gadget: N in {1024, 2048}, k = 1; the gadget is a run-time argument: 1 <= l <= 6, Bg_bit <= 31, l * Bg_bit < 64.
 * THE AUTOMATON is a handle made from host arrays and shared by the batch: states S in 1 .. MOSFHET_HIP_AUTOMATON_MAX_STATES, layers L in
 * 1 .. MOSFHET_HIP_AUTOMATON_MAX_STEPS; per layer and state next0, next1 in [0, S) and rot0, rot1 in [0, 2N), each int32 [L][S].  Position t of the word uses
 * layer t mod L: L = 1 is a time-invariant automaton, L = steps a branching program, anything between is periodic.  Creation checks and packs the tables on the host
 * (no device is needed); the packed table is copied to a device the first time a call runs there (one allocation, one synchronous copy) and stays for the handle's life.
 *   d_sel_dft  [count][steps][2l][2][N/2] complex in slot order: selector t of input b encrypts symbol t of b's word -- the layout of mosfhet_hip_leveled_lut_batch
 *              with size = steps, hence what mosfhet_hip_circuit_bootstrap_3_dft_batch and mosfhet_hip_trgsw_from_gadget_batch leave on the device;
 *              1 <= steps <= MOSFHET_HIP_AUTOMATON_MAX_STEPS
 *   d_init     [count][S][2][N] torus words, the state vector behind the last symbol; with init_shared != 0 [S][2][N], one vector for the whole batch (for example
 *              trivial samples of the final weights)
 * THE EVALUATION runs backwards, as in the papers:  V_steps = init;  for t = steps-1 .. 0, with lambda = t mod L, for every state q
 *     V_t[b][q] = R0 + sel[b][t] (.) (R1 - R0),   R0 = X^rot0[lambda][q] V_{t+1}[b][next0[lambda][q]],   R1 = X^rot1[lambda][q] V_{t+1}[b][next1[lambda][q]]
 * X^a is the exact negacyclic rotation of both components (torus_polynomial_mul_by_xai, src/polynomial.c:184-199); (.) is the external product of the calls above:
 * one chain over rows 0 .. 2l-1 from zero, rounded with the reduction mod 1.  V_0[b][q] is what the automaton started in q accumulates over b's word.
 *   start < 0        d_out is [count][S][2][N] = V_0: a long word is streamed chunk by chunk, LAST CHUNK FIRST, by feeding the output back in as d_init
 *   0 <= start < S   d_out is [count][2][N] = V_0[b][start], and step 0 computes that state only
 * No word depends on count, on a sample's position in the batch, on the chunking or on the workspace bound.
 * MOSFHET_HIP_EINVAL with a message naming the argument, before any HIP call: null pointers; N, gadget, states, layers, steps or start out of range; a table entry out
 * of range (at creation); count < 0; d_out overlapping d_init as address ranges; a workspace bound (mosfhet_hip_set_leveled_lut_workspace) below one input's state
 * vectors.  N is the handle's: the batch call takes no ring degree of its own, and the callers that know one from their arguments (Engine.trlwe_automaton,
 * mosfhet_trlwe_automaton) refuse a handle made for another N.  count == 0 does nothing.
 * One launch per step and chunk of inputs: the first reads d_init, the last writes d_out, those between alternate between two buffers [chunk][S][2][N] (steps = 1: none,
 * steps = 2: one) in the CALLING THREAD's pool: no allocation and no synchronisation from the second call of a shape on (capturable from then on) -- and therefore ONE
 * STREAM PER HOST THREAD at a time, as for mosfhet_hip_leveled_lut_batch.  A batch whose buffers exceed the bound runs in chunks of whole inputs.
 * mosfhet_hip_trlwe_automaton_plan says what the launcher will do, as a pure function (no GPU; `cus` sizes grids only): plan = {launches, inputs per chunk, workspace
 * bytes (buffers * chunk * S * 2N * 8), external products (count * (S * (steps - 1) + (start < 0 ? S : 1))), buffers}. */
#define MOSFHET_HIP_AUTOMATON_MAX_STATES 4096
#define MOSFHET_HIP_AUTOMATON_MAX_STEPS 4096
typedef struct mosfhet_hip_automaton *mosfhet_hip_automaton_t;
int mosfhet_hip_automaton_create(mosfhet_hip_automaton_t *out, const int *h_next0, const int *h_next1, const int *h_rot0, const int *h_rot1 /* each [layers][states] */,
                                 int states, int layers, int N);
int mosfhet_hip_automaton_destroy(mosfhet_hip_automaton_t automaton);
int mosfhet_hip_automaton_info(mosfhet_hip_automaton_t automaton, long long info[3] /* N, states, layers */);
int mosfhet_hip_trlwe_automaton_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, mosfhet_hip_automaton_t automaton, const double *d_sel_dft, const uint64_t *d_init,
                                      int init_shared, int steps, int start, int l, int Bg_bit, int count, void *stream);
int mosfhet_hip_trlwe_automaton_plan(int N, int l, int states, int layers, int steps, int start, int count, int cus, long long *plan /*[5]*/);

/* Selector logic: circuits of gates over TRGSW-encrypted bits, computed on the device FROM selectors (the reference's trgsw_mul_DFT / trgsw_mul_DFT2,
 * src/trgsw.c:425-442, are the AND gate).  The look-up tables, memories, automata and encrypted-weight layers above consume TRGSW_DFT selectors; this call makes new
 * ones from them without a bootstrap: an address is incremented, two address bits become a one-hot line, an automaton's symbol is the XOR of two encrypted bits.
 * Ring and gadget: N in {1024, 2048}, k = 1; the gadget is a run-time argument: 1 <= l <= 6, Bg_bit <= 31, l * Bg_bit < 64.
 * WIRES 0 .. n_in - 1 are a batch element's input selectors; wire n_in + g is the output of gate g.
 * THE CIRCUIT is a handle made from a host array int32 [n_gates][4] = {op, x, y, z} and shared by the batch.  Every operand a gate uses is a wire index below n_in + g
 * (inputs or EARLIER gates only; x = y is allowed); every operand field a gate does not use must be -1; 1 <= n_in, n_gates <= MOSFHET_HIP_SELLOGIC_MAX_WIRES.
 * X, Y, Z are the TRGSW_DFT samples on a gate's wires, r = c l + i a row (c = 0: component a, c = 1: component b):
 *   T(S)_r   = (G(S[r].a), G(S[r].b)), G = polynomial_DFT_to_torus, nearest mod 2^64: the words mosfhet_hip_dft_to_torus_batch writes
 *   E(L, W)  = the external product of the TRLWE sample L with W: one chain from +0.0 over W's rows 0 .. 2l-1 (the digits of L.a levels first, then L.b;
 *              polynomial_decompose_i, polynomial_torus_to_DFT, the two-FMA mul_addto with the digit first and the row second), then G of both accumulators
 *   H_r      = row r of the trivial sample of 1: 2^(64 - (i + 1) Bg_bit) at coefficient 0 of component c, zero elsewhere
 *   F        = polynomial_torus_to_DFT exactly as mosfhet_hip_torus_to_dft_batch makes it;  P_r = E(T(X)_r, Y);  all integer arithmetic mod 2^64
 *   op  name    operands   row r of the output, before F
 *   0   NOT     x          H_r - T(X)_r
 *   1   AND     x, y       P_r                                   trgsw_mul_DFT2(out, X, Y) row for row
 *   2   NAND    x, y       H_r - P_r
 *   3   OR      x, y       T(X)_r + T(Y)_r - P_r
 *   4   NOR     x, y       H_r - T(X)_r - T(Y)_r + P_r
 *   5   XOR     x, y       T(X)_r + T(Y)_r - 2 P_r
 *   6   XNOR    x, y       H_r - T(X)_r - T(Y)_r + 2 P_r
 *   7   ANDNOT  x, y       T(X)_r - P_r                          x and not y
 *   8   MUX     x, y, z    T(Y)_r + E(T(X)_r - T(Y)_r, Z)        z ? x : y
 * out[r] = (F(row.a), F(row.b)).  These are ring identities: the same gates multiply, add and select selectors of monomials or other small polynomials.
 * No word depends on count, on a batch element's position, on the launch geometry or on how levels are grouped.  AND is NOT commutative, in its words or in its noise:
 * THE DEEPER WIRE GOES IN x.  The left operand's noise is added; the right operand's row noise and the gadget's approximation error are multiplied by the digit norm
 * once in the gate and once more when the result is used.  At (N, l, Bg_bit) = (2048, 4, 9) with sigma 2^-44 a gate output's external product with a sample of 4-bit
 * messages in slots of 2^60 errs by about 2^50 - 2^52, and a chain with the accumulated wire in x grows by about 0.2 bit per gate; with the accumulated wire in y the
 * result is lost at depth 2.  A GATE'S OUTPUT IS USABLE ONLY AT SUCH A FINE GADGET WITH SUCH NOISE: at (1024, 2, 8), (1024, 3, 10), (1024, 6, 7) with sigma 2.989e-8
 * and at (2048, 1, 23) nothing survives one product (tests/test_trgsw_logic.py measures both), and selectors of mosfhet_hip_circuit_bootstrap_3_dft_batch are not
 * expected to survive one either.  The words are defined and tested at every gadget all the same.
 *   d_in_dft   [count][n_in][2l][2][N/2] complex in slot order: the layout of d_sel_dft of the leveled calls with size = n_in
 *   d_out_dft  [count][n_gates][2l][2][N/2] complex: EVERY gate's output, row g of a batch element = wire n_in + g (a d_sel_dft with size = n_gates: the caller picks
 *              its outputs by index); later levels read earlier rows of it
 * Creation checks every entry, computes level(g) = 1 + the highest level of g's operands (inputs: 0) and packs the gates sorted by level -- on the host, no device is
 * needed; the packed table is copied to a device the first time a call runs there (one allocation, one synchronous copy) and stays for the handle's life.  The call is
 * one launch per level, teams = count x gates of the level x 2l (a batch whose widest level exceeds one grid runs in chunks of whole batch elements); no pool, no
 * workspace; asynchronous on `stream`, never synchronises, capturable from the first call after the table is on the device.
 * MOSFHET_HIP_EINVAL with a message naming the argument, before any HIP call: null pointers; N, gadget, n_in or n_gates out of range; a gate entry that is no op, uses
 * a wire that is not earlier or sets an unused field (at creation); count < 0; d_out_dft overlapping d_in_dft as address ranges.  N is the handle's (Engine.trgsw_logic
 * refuses tensors of another N).  count == 0 does nothing.
 * mosfhet_hip_sellogic_info: info = {N, n_in, n_gates, levels, product gates (every op but NOT: 2l external products per batch element each)}.
 * mosfhet_hip_trgsw_logic_plan says what the launcher will do, as a pure function (no GPU; `cus` is reserved): plan = {launches, teams of the widest launch, external
 * products, inverse transforms, forward transforms}; the last three are those of n_gates AND gates (count x 2l x n_gates products; a handle's own count is
 * count x 2l x info[4]). */
#define MOSFHET_HIP_SELLOGIC_MAX_WIRES 4096
#define MOSFHET_HIP_SEL_NOT 0
#define MOSFHET_HIP_SEL_AND 1
#define MOSFHET_HIP_SEL_NAND 2
#define MOSFHET_HIP_SEL_OR 3
#define MOSFHET_HIP_SEL_NOR 4
#define MOSFHET_HIP_SEL_XOR 5
#define MOSFHET_HIP_SEL_XNOR 6
#define MOSFHET_HIP_SEL_ANDNOT 7
#define MOSFHET_HIP_SEL_MUX 8
typedef struct mosfhet_hip_sellogic *mosfhet_hip_sellogic_t;
int mosfhet_hip_sellogic_create(mosfhet_hip_sellogic_t *out, const int *h_gates /*[n_gates][4]*/, int n_gates, int n_in, int N);
int mosfhet_hip_sellogic_destroy(mosfhet_hip_sellogic_t c);
int mosfhet_hip_sellogic_info(mosfhet_hip_sellogic_t c, long long info[5] /* N, n_in, n_gates, levels, product gates */);
int mosfhet_hip_trgsw_logic_batch(mosfhet_hip_ctx_t ctx, double *d_out_dft /*[count][n_gates][2l][2][N/2] complex*/, mosfhet_hip_sellogic_t c,
                                  const double *d_in_dft /*[count][n_in][2l][2][N/2] complex*/, int l, int Bg_bit, int count, void *stream);
int mosfhet_hip_trgsw_logic_plan(int N, int l, int n_in, int n_gates, int levels, int widest_level, int count, int cus, long long *plan /*[5]*/);

/* ---- The client half on the device: encrypting and opening batches of samples under a secret key (csrc/capi_client.inc, csrc/client_kernels.h; the reference's
 * tlwe_new_sample / tlwe_phase, src/tlwe.c, trlwe_new_sample / trlwe_phase, src/trlwe.c:296-331, trgsw_new_monomial_sample + trgsw_to_DFT, src/trgsw.c:152-168).
 * For a user who keeps key and data on one trusted box: selectors for the leveled calls are made, and their results opened, without a host round trip.  k = 1.
 *
 * mosfhet_hip_client_key_create makes the key handle ON THE HOST (no device needed): h_s_rlwe [N] with N a power of two in 256 .. 4096, h_s_lwe [n] with
 * 1 <= n <= 65536, either may be NULL (not both); every coefficient must fit int16 as a signed word (binary keys and the bounded keys of tlwe / trlwe_new_bounded_key).
 * Creation packs the TRLWE key's nonzero coefficients as a list of (position, value) and the LWE key as one int per coefficient; the image is copied to a device the
 * first time a call runs there (one allocation, one synchronous copy, under the handle's lock) and stays for the handle's life.  Any number of host threads and
 * contexts may share a handle.  A call that needs the key the handle lacks returns MOSFHET_HIP_EINVAL.
 * mosfhet_hip_client_key_info: info = {N, n, nonzero coefficients of s_rlwe, s_rlwe binary (every coefficient 0 or 1)?, nonzero coefficients of s_lwe, s_lwe binary?}
 * (N = 0 / n = 0: that key is missing).
 *
 * Samples, word for word (all arithmetic mod 2^64):
 *   TLWE    out[i] = a_i for i < n, out[n] = sum_i a_i s_i + e + msg
 *   TRLWE   out[0] = a uniform, out[1] = b = a * s + e + msg; the product is exact and negacyclic (X^N = -1); d_msg NULL = the zero polynomial
 *   TRGSW   row q = c l + j (c < 2, j < l) of sample u is a fresh TRLWE(0); then m[u] 2^(64 - (j+1) Bg_bit) is added to coefficient e of component c -- AFTER b was formed
 *           from the plain mask -- where X^exp[u] = +-X^e: exponent taken mod 2N (two's complement: -3 is 2N - 3), sign flipped for N <= exp mod 2N
 *           (trgsw_new_monomial_sample; tests/client_reference.py).  d_exp NULL = all 0.  Gadget: 1 <= l <= 6, 1 <= Bg_bit <= 31, l * Bg_bit < 64, the rule of the
 *           RAM and automaton calls.  d_out_torus [count][2l][2][N] words and / or d_out_dft [count][2l][2][N/2] complex in slot order: the selector layout of the
 *           leveled calls, so `count` here is their count x size.  At least one output; with both, the doubles are the engine's forward transform
 *           (mosfhet_hip_torus_to_dft_batch) of exactly the words in d_out_torus.  d_out_dft needs N in {1024, 2048, 4096}.
 *
 * Randomness: MASKS AND NOISE both come from ChaCha20 under the secret of mosfhet_hip_set_keygen_secret (below) -- unlike the key generators, whose masks come from a
 * public seed: two encrypt calls that shared masks would publish the difference of their MESSAGES.  One block per (row, coefficient x), parameterised as the
 * generators' noise: counter = (row << 16) | x, nonce = (call index << 8) | kind with kind 6: TLWE, 7: TRLWE, 8: TRGSW; the call index is the generators' counter, so
 * no two calls of any kind share a nonce.  Output words 0 - 3 give the noise term exactly as the generators compute theirs; words 4 - 5 of the SAME block are the mask
 * word (low word first).  TLWE: row = the sample's index, mask word i from block x = i, the one noise term from block x = 0.  TRLWE: row = the sample's index.  TRGSW: row =
 * u 2l + q.  Launches are chunks of at most 2^20 rows; no word depends on the chunking, on the launch geometry, on count or on which outputs were asked for.  Like the
 * generators' noise this is reproducible under an installed secret WITHIN a release (known answers: tests/test_client_samples.py).
 * NO ENCRYPTION UNDER STREAM CAPTURE: the nonce is drawn when the call is made, so a replayed graph would encrypt again with the same masks and noise -- two samples
 * whose difference is the bare difference of their messages.  The three encrypt calls query hipStreamIsCapturing and return MOSFHET_HIP_EINVAL ("capture") before
 * anything is launched.
 *
 * Phases are exact, no transform: phase = b - sum_i a_i s_i, respectively b - a * s (tlwe_phase, trlwe_phase).  msg_bits = 0 returns the phases, msg_bits in 1 .. 63
 * returns (phase + 2^(63 - msg_bits)) >> (64 - msg_bits), the message of msg_bits bits nearest to the phase; anything else is refused.  One launch, no pool, never
 * synchronises: capturable from the first call after the key image is on the device.
 *
 * Every call: asynchronous on `stream` (the encrypt calls of a DFT-only TRGSW batch keep torus rows in the calling thread's pool, at most 1 GiB, chunk by chunk);
 * count == 0 does nothing.  MOSFHET_HIP_EINVAL with a message naming the argument, before any launch: null ctx, key or buffer; the handle lacks the key; count < 0;
 * gadget or msg_bits out of range; both TRGSW outputs NULL; an output overlapping an input (or the other output) as address ranges; a stream in capture (encryption).
 * mosfhet_hip_trgsw_encrypt_plan says what the launcher will do, as a pure function (no GPU): with_torus_out 0 = d_out_dft only, 1 = both outputs, 2 = d_out_torus
 * only; info = {launches, workgroups of the widest launch, workspace bytes (pool), chunks}. */
typedef struct mosfhet_hip_client_key *mosfhet_hip_client_key_t;
int mosfhet_hip_client_key_create(mosfhet_hip_client_key_t *out, const uint64_t *h_s_rlwe /*[N] or NULL*/, int N, const uint64_t *h_s_lwe /*[n] or NULL*/, int n);
int mosfhet_hip_client_key_destroy(mosfhet_hip_client_key_t key);
int mosfhet_hip_client_key_info(mosfhet_hip_client_key_t key, int64_t info[6]);
int mosfhet_hip_tlwe_encrypt_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_client_key_t key, uint64_t *d_out /*[count][n+1]*/, const uint64_t *d_msg /*[count]*/, double sigma,
                                   int count, void *stream);
int mosfhet_hip_trlwe_encrypt_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_client_key_t key, uint64_t *d_out /*[count][2][N]*/, const uint64_t *d_msg /*[count][N] or NULL*/,
                                    double sigma, int count, void *stream);
int mosfhet_hip_trgsw_encrypt_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_client_key_t key, double *d_out_dft /*[count][2l][2][N/2] complex or NULL*/,
                                    uint64_t *d_out_torus /*[count][2l][2][N] or NULL*/, const int32_t *d_m /*[count]*/, const int32_t *d_exp /*[count] or NULL*/, int l,
                                    int Bg_bit, double sigma, int count, void *stream);
int mosfhet_hip_trgsw_encrypt_plan(int N, int l, int count, int with_torus_out, int64_t info[4]);
int mosfhet_hip_tlwe_phase_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_client_key_t key, uint64_t *d_out /*[count]*/, const uint64_t *d_in /*[count][n+1]*/, int msg_bits,
                                 int count, void *stream);
int mosfhet_hip_trlwe_phase_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_client_key_t key, uint64_t *d_out /*[count][N]*/, const uint64_t *d_in /*[count][2][N]*/, int msg_bits,
                                  int count, void *stream);

/* Key images for the on-disk formats (save_bootstrap_key / load_new_bootstrap_key src/bootstrap.c:63-104, trlwe_save_KS_key /
 * trlwe_load_new_KS_key src/keyswitch.c:122-160, tlwe_save_KS_key / tlwe_load_new_KS_key src/tlwe.c:247-287, trlwe_save_generic_ks_key /
 * trlwe_load_new_generic_ks_key src/keyswitch.c:409-455).  DFT-domain contents are backend-defined in the reference too (src/polynomial.c:336-357):
 * an image is the engine's own layout (tag mosfhet_hip_dft_layout_id), mosfhet_hip_bsk_bytes / mosfhet_hip_trlwe_ksk_bytes long, and exact -- an
 * exported and re-imported key gives bit-identical results.  An unfolded bootstrap key's image is its torus-domain samples.  Table keys are the
 * reference's uncompressed row order and stream row-wise (ksk_export_rows / ksk_alloc + ksk_import_rows), 2N or n_out + 1 words per row.
 * info arrays: bsk {n, k, N, l, Bg_bit, unfolding}; trlwe_ksk {entries, N, t, base_bit}; ksk {n_in, row words, b_word, t, base_bit, kind}
 * with kind 0 = LWE -> LWE, 1 = packing, 2 = private (n_in counts the b entry). */
unsigned mosfhet_hip_dft_layout_id(void);
int mosfhet_hip_bsk_info(mosfhet_hip_bsk_t bsk, int *out6);
int mosfhet_hip_bsk_export(mosfhet_hip_bsk_t bsk, void *h_out);
int mosfhet_hip_bsk_import(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t *out, const void *h_image, int n, int k, int N, int l, int Bg_bit, int unfolding);
int mosfhet_hip_trlwe_ksk_info(mosfhet_hip_gak_t tks, int *out4);
size_t mosfhet_hip_trlwe_ksk_bytes(mosfhet_hip_gak_t tks);
int mosfhet_hip_trlwe_ksk_export(mosfhet_hip_gak_t tks, void *h_out);
int mosfhet_hip_trlwe_ksk_import(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t *out, const void *h_image, int entries, int N, int t, int base_bit);
int mosfhet_hip_ksk_info(mosfhet_hip_ksk_t ksk, int *out6);
int mosfhet_hip_ksk_alloc(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, int kind, int n, int n_out_or_N, int t, int base_bit);
int mosfhet_hip_ksk_import_rows(mosfhet_hip_ksk_t ksk, size_t first_row, size_t count, const uint64_t *h_in);

/* Key replication for several GPUs (keys replicated per GPU, optionally by hipMemcpyPeer over xGMI instead of host copies): a copy of
 * `src` on the device of `dst_ctx`, DEVICE TO DEVICE -- hipMemcpyPeer with peer access enabled where the two devices allow it (xGMI on an MI355X node),
 * HIP's own staged copy otherwise, and a pinned 64 MiB host bounce buffer when even that is refused.  Every field travels as it is: a seed-compressed
 * table key stays compressed (3 GB instead of the 6 GB its exported rows take at BASELINE configs[3]), an unfolded key keeps its torus-domain samples.
 * Same bits on both devices, so results do not depend on which replica serves a slice.  The source key's device need not be the caller's current one.
 * mosfhet_hip_last_clone_route(): how the calling thread's last clone travelled -- 0 same device, 1 peer to peer, 2 device to device without peer
 * access (HIP stages it), 3 host bounce buffer. */
int mosfhet_hip_bsk_clone(mosfhet_hip_ctx_t dst_ctx, mosfhet_hip_bsk_t *out, mosfhet_hip_bsk_t src);
int mosfhet_hip_ksk_clone(mosfhet_hip_ctx_t dst_ctx, mosfhet_hip_ksk_t *out, mosfhet_hip_ksk_t src);
int mosfhet_hip_gak_clone(mosfhet_hip_ctx_t dst_ctx, mosfhet_hip_gak_t *out, mosfhet_hip_gak_t src);
int mosfhet_hip_last_clone_route(void);
size_t mosfhet_hip_gak_bytes(mosfhet_hip_gak_t gak);                     /* device bytes of an FFT key-switch key set (= mosfhet_hip_trlwe_ksk_bytes) */

/* Timing hook for bench.py: runs `reps` launches of the programmable-bootstrap kernel on `stream`
 * bracketed by hipEvents ON THAT STREAM and returns the average kernel time in milliseconds
 * (synchronises the stream). */
int mosfhet_hip_time_programmable_bootstrap(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, uint64_t *d_out,
                                            const uint64_t *d_tv, int tv_count, const uint64_t *d_in, int count,
                                            int precision, int reps, void *stream, float *ms_per_launch);

/* Secret of the on-device key generators (bsk_generate, *_ksk_generate): the 256-bit ChaCha20 key their NOISE terms are drawn under.  It is independent
 * of the public 64-bit mask seed those calls take (masks are public and regenerable from that seed; noise is not).  Drawn from the operating system at
 * first use unless set here (32 bytes); process-wide.
 * Every generate call draws its noise under a ChaCha20 nonce no other call under this secret gets (a call counter and the generator kind), so the
 * `seed` arguments need NOT be unique: two keys made with the same seed share their masks, never their noise.  Setting the secret restarts that
 * sequence -- the same secret followed by the same generate calls reproduces the same keys (reproducible test runs; the host layer does this under
 * mosfhet_seed).  Never install one secret twice for keys that go to different parties.
 * The contract (known answers: tests/test_keygen_known_answers.py):
 *   - MASKS are a file format and STABLE: word idx of row `row` under `seed` (mask polynomial m of a k > 1 row: stream m, else 0) is
 *       z = seed + 0x9E3779B97F4A7C15 * (row * 0x100000001B3 + idx * 4 + stream + 1);  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *       z = (z ^ z >> 27) * 0x94D049BB133111EB;  word = z ^ z >> 31          (all mod 2^64)
 *     Stored seed-compressed keys regenerate their masks with it, so it does not change between releases.
 *   - NOISE is reproducible under an installed secret WITHIN a release, not across releases.  Today: the ChaCha20 block function of RFC 8439 with a
 *     64-bit block counter (state words 12 - 13) and a 64-bit nonce (words 14 - 15), key = the 32 bytes as eight little-endian words,
 *     counter = (row << 16) | coefficient, nonce = (call index << 8) | kind -- the call index counts generate calls from 1 after the secret was installed;
 *     kind 1: table keys (packing, private, LUT packing), 2: bootstrap keys, 3: unfolded bootstrap keys, 4: FFT key-switch key sets, 5: LWE tables.
 *     Output words 0 - 3 are two 64-bit uniforms (low word first), u = ((w >> 11) + 0.5) 2^-53, the term is cos(2 pi u1) sqrt(-2 ln u2) sigma 2^64
 *     truncated towards zero (evaluated in double: within 2^-48 sigma of the exact value).
 *   - The ENCRYPT calls of the client half (mosfhet_hip_tlwe_encrypt_batch, _trlwe_, _trgsw_, above) draw on the same secret and the same call counter with kinds 6
 *     (TLWE), 7 (TRLWE) and 8 (TRGSW): noise from words 0 - 3 as here, and -- unlike the generators -- their MASKS from words 4 - 5 of the same block (low word
 *     first), so their masks are secret-derived and never repeat between calls.  TLWE: row = sample, mask word i from coefficient i, the noise term from coefficient 0;
 *     TRLWE: row = sample; TRGSW: row = sample * 2l + c * l + j.  Reproducible within a release, like the noise. */
int mosfhet_hip_set_keygen_secret(const void *key32);

/* ---- DFT-level entry points behind the reference's legacy signatures (mosfhet.h:179-182,263-264,342-344,454,296 of the reference; csrc/capi_dft.inc).
 * DFT-domain objects are device arrays of doubles in the engine's slot order ([polynomial][N/2] complex). ---- */
/* non-owning key handle over n consecutive TRGSW_DFT entries ([(k+1)l][k+1][N/2] complex each) already on the device; destroy with mosfhet_hip_bsk_destroy */
int mosfhet_hip_bsk_view_create(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t *out, const double *d_dft, int n, int k, int N, int l, int Bg_bit);
const double *mosfhet_hip_bsk_device_dft(mosfhet_hip_bsk_t bsk);          /* device address of entry 0 (NULL: unfolded key) */
/* trgsw_mul_trlwe_DFT (src/trgsw.c:385-423), result left in the DFT domain: d_out_dft [count][k+1][N/2] complex; key_stride in doubles, 0 = shared TRGSW */
int mosfhet_hip_external_product_dft_batch(mosfhet_hip_ctx_t ctx, const double *d_trgsw_dft, size_t key_stride, double *d_out_dft,
                                           const uint64_t *d_in /*[count][k+1][N]*/, int N, int l, int Bg_bit, int count, void *stream);
/* public_mux (src/bootstrap.c:369-389) with the selector rows in the DFT domain: d_sel_dft [count][l][2][N/2] complex */
int mosfhet_hip_public_mux_dft_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out /*[count][2][N]*/, const uint64_t *d_p0 /*[N]*/, const uint64_t *d_p1,
                                     const double *d_sel_dft, int N, int l, int Bg_bit, int count, void *stream);
/* blind_rotate_ga (src/bootstrap_ga.c:35-60) in place on d_acc [count][2][N]; d_in [count][n+1] (mask words).  gak: the full automorphism key set with t = l and
 * base_bit = Bg_bit; entries < N returns MOSFHET_HIP_EINVAL before any HIP call (the generators reach 2N - 1, entry N - 1). */
int mosfhet_hip_blind_rotate_ga_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_gak_t gak, uint64_t *d_acc, const uint64_t *d_in, int count,
                                      void *stream);
/* polynomial_add_DFT_polynomials / _sub_ / _scale_and_add_ (src/polynomial.c:102-128) and the TRLWE_DFT / TRGSW_DFT sums built on them, over flat
 * device arrays: d_out[i] = (d_a ? d_a[i] : 0) + cb * d_b[i] (d_out may alias d_a or d_b) */
int mosfhet_hip_dft_lincomb_batch(mosfhet_hip_ctx_t ctx, double *d_out, const double *d_a, const double *d_b, double cb, size_t n_doubles, void *stream);
/* trlwe_eval_automorphism (src/trlwe.c:775-781) with key-set entry `entry` (the batch entry point above uses entry (gen - 1) / 2) */
int mosfhet_hip_trlwe_eval_automorphism_entry_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t gak, int entry, uint64_t *d_out, const uint64_t *d_in, int gen,
                                                    int count, void *stream);

#ifdef __cplusplus
}
#endif
#endif
