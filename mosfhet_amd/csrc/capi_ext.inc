// capi_ext.inc -- C-ABI entry points of the callers either side of the bootstrap (SURVEY section 8 rows a20-a22, a24, a25, a28).
// Included at the end of capi.hip (shares its handle types and helpers).  Every entry point is a composition of launches on
// one stream; temporaries live in the calling thread's pool (capi.hip: ThreadPool), grown on demand.

static int ctx_scratch(mosfhet_hip_ctx_t ctx, int slot, size_t words, uint64_t **out) { return pool_get(ctx->device, POOL_CTX0 + slot, words, out); }
static int ext_scratch(mosfhet_hip_bsk_t bsk, int slot, size_t words, uint64_t **out) { return pool_get(bsk->device, POOL_EXT0 + slot, words, out); }

// ---- secret of the on-device key generators (csrc/keygen_kernels.h): the ChaCha20 key of the NOISE terms.  Independent of the public mask seeds the
// generate calls take; drawn from the operating system at first use unless the caller installs one (the host layer hands over 32 bytes of its own
// ChaCha20 stream, which makes runs under mosfhet_seed reproducible).  Process-wide, set once before keys are generated.
#include <sys/random.h>
#include <mutex>
static NoiseKey g_noise_key;
static bool g_noise_key_set = false;
static uint64_t g_noise_calls = 0;   // generate calls made under the current key: every call gets its own ChaCha20 nonce
static std::mutex g_noise_key_lock;

extern "C" int mosfhet_hip_set_keygen_secret(const void *key32) {
  if (!key32) return fail(MOSFHET_HIP_EINVAL, "set_keygen_secret: null key");
  std::lock_guard<std::mutex> hold(g_noise_key_lock);
  memcpy(g_noise_key.k, key32, sizeof(g_noise_key.k));
  g_noise_key_set = true;
  g_noise_calls = 0;   // a new key starts a new sequence (installing the same key again reproduces the same keys: mosfhet_seed)
  return MOSFHET_HIP_OK;
}

// The noise stream of ONE generate call: the process-wide key with a nonce no other call under that key gets (call counter, generator kind in the low
// byte).  Masks come from the caller's public seed and repeat when the seed repeats; the noise never does (see keygen_kernels.h).
enum { NOISE_TABLE = 1, NOISE_BSK = 2, NOISE_BSK_UNFOLDED = 3, NOISE_TRLWE_KSK = 4, NOISE_TLWE_KSK = 5 };
static NoiseKey noise_key_for_call(int kind) {
  std::lock_guard<std::mutex> hold(g_noise_key_lock);
  if (!g_noise_key_set) {
    size_t got = 0;
    while (got < sizeof(g_noise_key.k)) {
      const ssize_t r = getrandom((char *)g_noise_key.k + got, sizeof(g_noise_key.k) - got, 0);
      if (r <= 0) break;
      got += (size_t)r;
    }
    if (got < sizeof(g_noise_key.k)) {
      FILE *f = fopen("/dev/urandom", "rb");
      if (!f || fread(g_noise_key.k, sizeof(g_noise_key.k), 1, f) != 1) {
        fprintf(stderr, "mosfhet_amd: no entropy source for key generation (getrandom and /dev/urandom failed)\n");
        abort();
      }
      fclose(f);
    }
    g_noise_key_set = true;
  }
  NoiseKey k = g_noise_key;
  k.nonce = (++g_noise_calls << 8) | (uint64_t)(kind & 0xff);
  return k;
}

static int is_packing_key(mosfhet_hip_ksk_t k, int N) { return k->row == 2 * N && k->b_word == N && k->n_in == N; }

// ---- public_mux ----
static int launch_public_mux(mosfhet_hip_ctx_t ctx, uint64_t *d_out, size_t out_stride, const uint64_t *d_p0, const uint64_t *d_p1, const uint64_t *d_sel,
                             size_t sel_stride, uint64_t *dec /*[l][N] words*/, d2 *pdec /*[l][N/2]*/, int N, int l, int Bg_bit, int count, hipStream_t s) {
  hipLaunchKernelGGL(public_mux_digits_kernel, dim3((N + 255) / 256), dim3(256), 0, s, d_p0, d_p1, dec, N, l, Bg_bit);
  RING_DISPATCH(ctx, N, {
    hipLaunchKernelGGL(torus_to_dft_kernel<F>, dim3(l), dim3(F::THREADS), 0, s, dec, pdec, TW);
    hipLaunchKernelGGL(public_mux_kernel<F>, dim3(count), dim3(F::THREADS), 0, s, d_sel, sel_stride, pdec, d_p0, TW, d_out, out_stride, l);
  });
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_public_mux_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const uint64_t *d_p0, const uint64_t *d_p1, const uint64_t *d_sel, int N,
                                            int l, int Bg_bit, int count, void *stream) {
  if (!ctx || (count > 0 && !d_out) || (count > 0 && !d_p0) || (count > 0 && !d_p1) || (count > 0 && !d_sel) || count < 0 || l < 1 || l * Bg_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "public_mux: bad argument");
  if (!ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "public_mux: N = %d not supported (1024, 2048, 4096)", N);
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  uint64_t *tmp = nullptr;
  HIP_TRY(hipMalloc((void **)&tmp, (size_t)2 * l * N * sizeof(uint64_t)));
  int rc = launch_public_mux(ctx, d_out, (size_t)2 * N, d_p0, d_p1, d_sel, (size_t)l * 2 * N, tmp, (d2 *)(tmp + (size_t)l * N), N, l, Bg_bit, count,
                             pick(ctx, stream));
  hipFree(tmp);  // synchronises
  return rc;
}

// ---- full_domain_functional_bootstrap_KS21 / _KS21_2 ----
extern "C" int mosfhet_hip_full_domain_functional_bootstrap_KS21_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_ksk_t pksk, uint64_t *d_out,
                                                                       const uint64_t *d_tv, const uint64_t *d_in, int count, int torus_base, int variant,
                                                                       void *stream) {
  TUNED_ONLY(bsk, "full_domain_functional_bootstrap_KS21");
  if (!ctx || !bsk || !pksk || (count > 0 && !d_out) || (count > 0 && !d_tv) || (count > 0 && !d_in) || count < 0 || torus_base < 2 || (torus_base & 1)) return fail(MOSFHET_HIP_EINVAL, "fdfb_KS21: bad argument");
  const int N = bsk->N, l = bsk->l, Bg = bsk->Bg_bit, half_base = torus_base / 2;
  if (!is_packing_key(pksk, N)) return fail(MOSFHET_HIP_EINVAL, "fdfb_KS21: ksk must be a packing key N -> TRLWE(N)");
  if (variant == 0 && l * half_base > N) return fail(MOSFHET_HIP_EINVAL, "fdfb_KS21: l * torus_base / 2 exceeds N");
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t row = (size_t)2 * N;
  // Few ciphertexts: the l levels' samples are laid out input-major (sample b l + i) and go through the packing table TOGETHER -- one switch of l count samples, whose
  // output order IS the selector layout [count][l] -- instead of l switches that each sweep the table for a fraction of a tile (capi.hip: cb_levels_together); and the l
  // bootstraps per input of _KS21_2, which differ in the test vector only, run as one row-mode launch (cb_bootstraps_together).  Same operations on the same words.
  const bool together = cb_levels_together(count, l), rows_together = variant == 1 && cb_bootstraps_together(bsk, count, l);
  const bool wide_ext = together || rows_together;
  const size_t w_tv = row * (rows_together ? l : 1), w_acc = (size_t)count * row, w_ext = ((size_t)count * (N + 1) * (wide_ext ? l : 1) + 1) & ~(size_t)1, w_sel = (size_t)count * l * row,
               w_dec = (size_t)l * N, w_p = (size_t)2 * N, w_tv2 = (size_t)count * row;
  uint64_t *base = nullptr;
  int rc = ext_scratch(bsk, 0, w_tv + w_acc + w_ext + w_sel + 2 * w_dec + w_p + w_tv2, &base);
  if (rc) return rc;
  uint64_t *tv_sign = base, *acc = tv_sign + w_tv, *ext = acc + w_acc, *sel = ext + w_ext, *dec = sel + w_sel, *pdec = dec + w_dec, *p0 = pdec + w_dec,
           *p1 = p0 + N, *tv2 = p0 + w_p;
  hipStream_t s = pick(ctx, stream);
  // sample (b, i) of the level loop: input-major in the wide layout, one level at a time otherwise
  const size_t e_stride = wide_ext ? (size_t)l * (N + 1) : (size_t)N + 1;
  auto e_level = [&](int i) { return wide_ext ? ext + (size_t)i * (N + 1) : ext; };
  auto switch_level = [&](int i) -> int {   // level i's samples -> selector rows i (one switch per level)
    HIP_TRY(launch_tlwe_keyswitch(pksk->d_ksk, sel + (size_t)i * row, (size_t)l * row, e_level(i), e_stride, count, N, 2 * N, N, pksk->t, pksk->base_bit, tl_ws(ctx->device), s,
                                  pksk->compressed, pksk->seed));
    return MOSFHET_HIP_OK;
  };
  if (variant == 0) {
    const int slot_size = N / (l * half_base);
    hipLaunchKernelGGL(ks21_sign_lut_kernel, dim3((N + 255) / 256), dim3(256), 0, s, tv_sign, N, l, Bg, half_base, (uint64_t *)nullptr, (uint64_t *)nullptr);
    if ((rc = mosfhet_hip_functional_bootstrap_wo_extract_batch(ctx, bsk, acc, tv_sign, 1, d_in, count, l * half_base, stream))) return rc;
    for (int i = 0; i < l; i++) {
      const uint64_t sign = ~0ull << (64 - (i + 1) * Bg - 1);
      hipLaunchKernelGGL(trlwe_extract_kernel, dim3((N + 255) / 256, count), dim3(256), 0, s, e_level(i), e_stride, acc, row, N, 1, i * slot_size);
      hipLaunchKernelGGL(tlwe_add_to_word_kernel, dim3((count + 255) / 256), dim3(256), 0, s, e_level(i), count, e_stride, (size_t)N, (uint64_t)0 - sign);
      if (!together && (rc = switch_level(i))) return rc;
    }
  } else {
    if (rows_together) {
      for (int i = 0; i < l; i++)
        hipLaunchKernelGGL(torus_packing_kernel, dim3((N + 255) / 256), dim3(256), 0, s, tv_sign + (size_t)i * row, N, (const uint64_t *)nullptr, 1, ~0ull << (64 - (i + 1) * Bg - 1), ~0ull << (64 - (i + 1) * Bg - 1));
      if ((rc = bootstrap_common("full_domain_functional_bootstrap_KS21_2", ctx, bsk, ext, tv_sign, l, d_in, count * l, 0, 0, 0, half_base, 1, 0, stream, l))) return rc;
    }
    for (int i = 0; i < l; i++) {
      const uint64_t sign = ~0ull << (64 - (i + 1) * Bg - 1);
      if (!rows_together) {
        hipLaunchKernelGGL(torus_packing_kernel, dim3((N + 255) / 256), dim3(256), 0, s, tv_sign, N, (const uint64_t *)nullptr, 1, sign, sign);
        // (wide layout without the row-mode launch: the bootstrap writes level i's samples contiguously; they are spread to their input-major places afterwards)
        if ((rc = mosfhet_hip_functional_bootstrap_batch(ctx, bsk, wide_ext ? acc : ext, tv_sign, 1, d_in, count, half_base, stream))) return rc;
        if (wide_ext)
          HIP_TRY(hipMemcpy2DAsync(e_level(i), e_stride * sizeof(uint64_t), acc, (size_t)(N + 1) * sizeof(uint64_t), (size_t)(N + 1) * sizeof(uint64_t), (size_t)count,
                                   hipMemcpyDeviceToDevice, s));
      }
      hipLaunchKernelGGL(tlwe_add_to_word_kernel, dim3((count + 255) / 256), dim3(256), 0, s, e_level(i), count, e_stride, (size_t)N, (uint64_t)0 - sign);
      if (!together && (rc = switch_level(i))) return rc;
    }
  }
  if (together)   // all l count samples at once: sample b l + i lands on selector row (b, i)
    HIP_TRY(launch_tlwe_keyswitch(pksk->d_ksk, sel, row, ext, (size_t)N + 1, l * count, N, 2 * N, N, pksk->t, pksk->base_bit, tl_ws(ctx->device), s, pksk->compressed, pksk->seed));
  hipLaunchKernelGGL(ks21_sign_lut_kernel, dim3((N + 255) / 256), dim3(256), 0, s, const_cast<uint64_t *>(d_tv), N, l, Bg, half_base, p0, p1);   // (p0 given: d_tv is only read)
  if ((rc = launch_public_mux(ctx, tv2, row, p0, p1, sel, (size_t)l * row, dec, (d2 *)pdec, N, l, Bg, count, s))) return rc;
  return mosfhet_hip_functional_bootstrap_batch(ctx, bsk, d_out, tv2, count, d_in, count, half_base, stream);
}

// ---- multivalue_bootstrap_phase1 / phase2 ----
extern "C" int mosfhet_hip_multivalue_bootstrap_phase1_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, uint64_t *d_out, const uint64_t *d_in, int count,
                                                             int torus_base, void *stream) {
  TUNED_ONLY(bsk, "multivalue_bootstrap_phase1");
  if (!ctx || !bsk || (count > 0 && !d_out) || (count > 0 && !d_in) || count < 0 || torus_base < 1) return fail(MOSFHET_HIP_EINVAL, "multivalue_phase1: bad argument");
  const int N = bsk->N;
  if (torus_base >= N) return fail(MOSFHET_HIP_EINVAL, "multivalue_phase1: torus_base must be < N");
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  uint64_t *base = nullptr;
  int rc = ext_scratch(bsk, 0, (size_t)2 * N + (size_t)count * 2 * N, &base);
  if (rc) return rc;
  uint64_t *tv = base, *acc = base + 2 * N;
  hipStream_t s = pick(ctx, stream);
  // constant test vector 1 / (4 torus_base)  (double2torus, src/misc.c:13-15)
  const uint64_t c = (uint64_t)(int64_t)(18446744073709551616.0 * (1. / (4 * torus_base)));
  hipLaunchKernelGGL(torus_packing_kernel, dim3((N + 255) / 256), dim3(256), 0, s, tv, N, (const uint64_t *)nullptr, 1, c, c);
  if ((rc = mosfhet_hip_functional_bootstrap_wo_extract_batch(ctx, bsk, acc, tv, 1, d_in, count, torus_base, stream))) return rc;
  hipLaunchKernelGGL(mv_phase1_rotate_kernel, dim3((2 * N + 255) / 256, torus_base + 1, count), dim3(256), 0, s, acc, d_out, N, torus_base);
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_multivalue_bootstrap_phase2_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const int *h_lut, const uint64_t *d_rotated, int N,
                                                             int torus_base, int log_torus_base, int count, void *stream) {
  if (!ctx || (count > 0 && !d_out) || !h_lut || (count > 0 && !d_rotated) || count < 0) return fail(MOSFHET_HIP_EINVAL, "multivalue_phase2: bad argument");
  if (torus_base < 1 || torus_base > 64 || log_torus_base < 0 || log_torus_base > 6 || N > 4096 || (N & (N - 1)))
    return fail(MOSFHET_HIP_EINVAL, "multivalue_phase2: torus_base <= 64, log_torus_base <= 6, N <= 4096 supported");
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  MvCoef coef;
  memset(&coef, 0, sizeof(coef));
  for (int j = 0; j < log_torus_base; j++) {   // src/bootstrap.c:251-262
    const int over0 = ((h_lut[0] >> j) & 1) + ((h_lut[torus_base - 1] >> j) & 1);
    if (over0 == 2) coef.c[j][torus_base] = 1;
    else if (over0 == 1) coef.c[j][0] = 1;
    for (int i = 1; i < torus_base; i++) coef.c[j][i] = (signed char)(((h_lut[i] >> j) & 1) - ((h_lut[i - 1] >> j) & 1));
  }
  hipLaunchKernelGGL(mv_phase2_kernel, dim3(count), dim3(256), (size_t)2 * N * sizeof(uint64_t), pick(ctx, stream), d_rotated, d_out, coef, N, torus_base,
                     log_torus_base);
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// ---- table-lookup private key switch: LWE(m) -> TRLWE(-s m) ----
extern "C" int mosfhet_hip_priv_ksk_create(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, const uint64_t *h_rows, int n, int N, int t, int base_bit) {
  // rows of 2N words, n + 1 digit sources (the b word is the last one, key -1), nothing copied to the output
  int rc = mosfhet_hip_ksk_create(ctx, out, h_rows, n + 1, 2 * N - 1, t, base_bit);
  if (rc) return rc;
  (*out)->b_word = -1;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_trlwe_priv_keyswitch_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, uint64_t *d_out, const uint64_t *d_in, int count,
                                                      void *stream) {
  if (!ctx || !ksk || (count > 0 && !d_out) || (count > 0 && !d_in) || count < 0 || ksk->b_word != -1) return fail(MOSFHET_HIP_EINVAL, "priv_keyswitch: needs a key from priv_ksk_create");
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(launch_tlwe_keyswitch(ksk->d_ksk, d_out, (size_t)ksk->row, d_in, (size_t)ksk->n_in, count, ksk->n_in, ksk->row, -1, ksk->t, ksk->base_bit, tl_ws(ctx->device),
                                pick(ctx, stream), ksk->compressed, ksk->seed));
  return MOSFHET_HIP_OK;
}

// ---- circuit_bootstrap (variant 0) / circuit_bootstrap_2 (variant 1) ----
extern "C" int mosfhet_hip_circuit_bootstrap_batch_ev(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_ksk_t kska, mosfhet_hip_ksk_t kskb, uint64_t *d_out,
                                                      const uint64_t *d_in, int count, int variant, void *stream, void *const *level_done) {
  TUNED_ONLY(bsk, "circuit_bootstrap");
  if (!ctx || !bsk || !kska || !kskb || (count > 0 && !d_out) || (count > 0 && !d_in) || count < 0) return fail(MOSFHET_HIP_EINVAL, "circuit_bootstrap: bad argument");
  const int N = bsk->N, l = bsk->l;
  if (kska->b_word != -1 || kska->row != 2 * N || kska->n_in != N + 1) return fail(MOSFHET_HIP_EINVAL, "circuit_bootstrap: kska must be a private key-switch key N -> TRLWE(N)");
  if (!is_packing_key(kskb, N)) return fail(MOSFHET_HIP_EINVAL, "circuit_bootstrap: kskb must be a packing key N -> TRLWE(N)");
  if (variant == 1 && N % (2 * l)) return fail(MOSFHET_HIP_EINVAL, "circuit_bootstrap_2: N not divisible by 2l");
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t row = (size_t)2 * N, trgsw = (size_t)2 * l * row;
  // circuit_bootstrap_2 on few ciphertexts: the l levels' samples go through each table switch TOGETHER (capi.hip: cb_levels_together) -- two switches of l count samples
  // instead of 2 l switches of count, ceil(l count / 512) sweeps of each table instead of l; results land in a staging block and are copied into their TRGSW rows.
  const bool together = variant == 1 && cb_levels_together(count, l);
  const size_t w_ext = ((size_t)count * (N + 1) * (together ? l : 1) + 1) & ~(size_t)1, w_stage = together ? (size_t)l * count * row : 0;
  uint64_t *base = nullptr;
  int rc = ext_scratch(bsk, 0, row + (size_t)count * row + w_ext + w_stage, &base);
  if (rc) return rc;
  uint64_t *tv = base, *acc = tv + row, *ext = acc + (size_t)count * row, *stage = ext + w_ext;
  hipStream_t s = pick(ctx, stream);
  if (variant == 1) {
    hipLaunchKernelGGL(circuit_bootstrap_lut_kernel, dim3((N + 255) / 256), dim3(256), 0, s, tv, N, l, bsk->Bg_bit);
    if ((rc = mosfhet_hip_functional_bootstrap_wo_extract_batch(ctx, bsk, acc, tv, 1, d_in, count, 2 * l, stream))) return rc;
  }
  if (variant == 0 && cb_bootstraps_together(bsk, count, l)) {
    // circuit_bootstrap on few ciphertexts: its l bootstraps per input differ in the test vector only (src/bootstrap.c:313-317), so they run as ONE launch in row mode
    // (PbsParams.rows = l: block b takes input b / l and test vector b % l; a single call is l bootstraps side by side instead of one after the other; beyond one
    // residency round launch_pbs cuts the row blocks into rounds of whole inputs), and the l count
    // samples -- input-major: sample b l + i -- go through each table switch together.  Same operations on the same words: same bits.
    uint64_t *tvs = nullptr, *ext0 = nullptr, *stage0 = nullptr;
    const size_t w_tvs = (size_t)l * row, w_e = ((size_t)l * count * (N + 1) + 1) & ~(size_t)1;
    if ((rc = ext_scratch(bsk, 1, w_tvs + w_e + (size_t)l * count * row, &tvs))) return rc;
    ext0 = tvs + w_tvs;
    stage0 = ext0 + w_e;
    for (int i = 0; i < l; i++)
      hipLaunchKernelGGL(torus_packing_kernel, dim3((N + 255) / 256), dim3(256), 0, s, tvs + (size_t)i * row, N, (const uint64_t *)nullptr, 1, 1ull << (64 - (i + 1) * bsk->Bg_bit), (uint64_t)0);
    if ((rc = bootstrap_common("circuit_bootstrap", ctx, bsk, ext0, tvs, l, d_in, count * l, 0, 0, 0, 2, 1, 0, stream, l))) return rc;
    for (int half = 0; half < 2; half++) {
      const mosfhet_hip_ksk_t key = half ? kskb : kska;
      HIP_TRY(launch_tlwe_keyswitch(key->d_ksk, stage0, row, ext0, (size_t)N + 1, l * count, half ? N : N + 1, 2 * N, half ? N : -1, key->t, key->base_bit, tl_ws(ctx->device), s,
                                    key->compressed, key->seed));
      // TRGSW b takes samples b l .. b l + l - 1 as its rows half l .. half l + l - 1: l rows wide, one TRGSW apart
      HIP_TRY(hipMemcpy2DAsync(d_out + (size_t)half * l * row, trgsw * sizeof(uint64_t), stage0, (size_t)l * row * sizeof(uint64_t), (size_t)l * row * sizeof(uint64_t), (size_t)count,
                               hipMemcpyDeviceToDevice, s));
    }
    if (level_done)
      for (int i = 0; i < l; i++)
        if (level_done[i]) HIP_TRY(hipEventRecord((hipEvent_t)level_done[i], s));
    HIP_TRY(hipGetLastError());
    return MOSFHET_HIP_OK;
  }
  if (together) {
    for (int i = 0; i < l; i++)
      hipLaunchKernelGGL(trlwe_extract_kernel, dim3((N + 255) / 256, count), dim3(256), 0, s, ext + (size_t)i * count * (N + 1), (size_t)N + 1, acc, row, N, 1, i * (N / (2 * l)));
    for (int half = 0; half < 2; half++) {   // rows i < l from the private table, rows l + i from the packing table
      const mosfhet_hip_ksk_t key = half ? kskb : kska;
      HIP_TRY(launch_tlwe_keyswitch(key->d_ksk, stage, row, ext, (size_t)N + 1, l * count, half ? N : N + 1, 2 * N, half ? N : -1, key->t, key->base_bit, tl_ws(ctx->device), s,
                                    key->compressed, key->seed));
      for (int i = 0; i < l; i++)
        HIP_TRY(hipMemcpy2DAsync(d_out + (size_t)(half * l + i) * row, trgsw * sizeof(uint64_t), stage + (size_t)i * count * row, row * sizeof(uint64_t), row * sizeof(uint64_t),
                                 (size_t)count, hipMemcpyDeviceToDevice, s));
    }
    if (level_done)
      for (int i = 0; i < l; i++)
        if (level_done[i]) HIP_TRY(hipEventRecord((hipEvent_t)level_done[i], s));   // (all levels are final together here)
    HIP_TRY(hipGetLastError());
    return MOSFHET_HIP_OK;
  }
  for (int i = 0; i < l; i++) {
    if (variant == 0) {
      hipLaunchKernelGGL(torus_packing_kernel, dim3((N + 255) / 256), dim3(256), 0, s, tv, N, (const uint64_t *)nullptr, 1, 1ull << (64 - (i + 1) * bsk->Bg_bit), (uint64_t)0);
      if ((rc = mosfhet_hip_functional_bootstrap_batch(ctx, bsk, ext, tv, 1, d_in, count, 2, stream))) return rc;
    } else {
      hipLaunchKernelGGL(trlwe_extract_kernel, dim3((N + 255) / 256, count), dim3(256), 0, s, ext, (size_t)N + 1, acc, row, N, 1, i * (N / (2 * l)));
    }
    HIP_TRY(launch_tlwe_keyswitch(kska->d_ksk, d_out + (size_t)i * row, trgsw, ext, (size_t)N + 1, count, N + 1, 2 * N, -1, kska->t, kska->base_bit, tl_ws(ctx->device), s, kska->compressed, kska->seed));
    HIP_TRY(launch_tlwe_keyswitch(kskb->d_ksk, d_out + (size_t)(l + i) * row, trgsw, ext, (size_t)N + 1, count, N, 2 * N, N, kskb->t, kskb->base_bit, tl_ws(ctx->device), s, kskb->compressed, kskb->seed));
    if (level_done && level_done[i]) HIP_TRY(hipEventRecord((hipEvent_t)level_done[i], s));   // rows i and l + i of every output are final
  }
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_circuit_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_ksk_t kska, mosfhet_hip_ksk_t kskb, uint64_t *d_out,
                                                   const uint64_t *d_in, int count, int variant, void *stream) {
  return mosfhet_hip_circuit_bootstrap_batch_ev(ctx, bsk, kska, kskb, d_out, d_in, count, variant, stream, nullptr);
}

// ---- TRGSW-accumulator bootstrap ("full TRGSW bootstrap") ----
// phase 1 [src/bootstrap.c:284-295]: the 2l rows of the trivial TRGSW(1) are blind-rotated independently (trgsw_mul_DFT is row-wise,
// src/trgsw.c:425-431) by pbs_kernel with rows = 2l, then transformed (trgsw_to_DFT).  d_out_dft: [count][2l][2][N/2] complex,
// the engine's slot order = the layout of one bootstrap-key entry.
extern "C" int mosfhet_hip_functional_bootstrap_trgsw_phase1_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, double *d_out_dft, const uint64_t *d_in, int count,
                                                                   int torus_base, void *stream) {
  TUNED_ONLY(bsk, "functional_bootstrap_trgsw_phase1");
  if (!ctx || !bsk || (count > 0 && !d_out_dft) || (count > 0 && !d_in) || count < 0 || torus_base < 1) return fail(MOSFHET_HIP_EINVAL, "trgsw_phase1: bad argument");
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const int N = bsk->N, l = bsk->l, rows = 2 * l;
  const size_t row = (size_t)2 * N;
  uint64_t *base = nullptr;
  int rc = ext_scratch(bsk, 0, rows * row + (size_t)count * rows * row, &base);
  if (rc) return rc;
  uint64_t *tv = base, *acc = base + rows * row;
  hipStream_t s = pick(ctx, stream);
  hipLaunchKernelGGL(trgsw_trivial_one_kernel, dim3((2 * N + 255) / 256, rows), dim3(256), 0, s, tv, N, l, bsk->Bg_bit);
  if ((rc = bootstrap_common("functional_bootstrap_trgsw_phase1", ctx, bsk, acc, tv, rows, d_in, count * rows, 0, 0, 0, torus_base, 0, 0, stream, rows))) return rc;
  return mosfhet_hip_torus_to_dft_batch(ctx, d_out_dft, acc, N, count * rows * 2, stream);
}

// phase 2 [src/bootstrap.c:297-306]: d_out[b] = SampleExtract_0( tv (.) TRGSW_b ); tv shared (tv_count = 1) or one per ciphertext
extern "C" int mosfhet_hip_functional_bootstrap_trgsw_phase2_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, uint64_t *d_out, const double *d_in_dft,
                                                                   const uint64_t *d_tv, int tv_count, int count, void *stream) {
  TUNED_ONLY(bsk, "functional_bootstrap_trgsw_phase2");
  if (!ctx || !bsk || (count > 0 && !d_out) || (count > 0 && !d_in_dft) || (count > 0 && !d_tv) || count < 0 || (tv_count != 1 && tv_count != count)) return fail(MOSFHET_HIP_EINVAL, "trgsw_phase2: bad argument");
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const int N = bsk->N, l = bsk->l;
  uint64_t *tmp = nullptr;
  int rc = ext_scratch(bsk, 0, (size_t)count * 2 * N, &tmp);
  if (rc) return rc;
  hipStream_t s = pick(ctx, stream);
  const size_t key_stride = (size_t)2 * l * 2 * (N / 2), in_stride = tv_count == 1 ? 0 : (size_t)2 * N;
  const d2 *g = (const d2 *)d_in_dft;
  RING_DISPATCH(ctx, N, rc = launch_external_product<F>(l, bsk->Bg_bit, s, g, TW, d_tv, tmp, count, key_stride, in_stride, nullptr, nullptr, false));
  if (rc) return rc;
  hipLaunchKernelGGL(trlwe_extract_kernel, dim3((N + 255) / 256, count), dim3(256), 0, s, d_out, (size_t)N + 1, tmp, (size_t)2 * N, N, 1, 0);
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// ---- FFT tensor product, tlwe_mul, CLOT21 full-domain bootstraps ----
// trlwe_tensor_prod_FFT [src/trlwe.c:727-771]; rlk = 1-entry key set made from trlwe_new_RL_key rows (src/keyswitch.c:3-10)
extern "C" int mosfhet_hip_trlwe_tensor_prod_FFT_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t rlk, uint64_t *d_out, const uint64_t *d_in1, const uint64_t *d_in2,
                                                       int precision, int count, void *stream) {
  if (!ctx || !rlk || (count > 0 && !d_out) || (count > 0 && !d_in1) || (count > 0 && !d_in2) || count < 0 || precision < 1 || precision > 62) return fail(MOSFHET_HIP_EINVAL, "tensor_prod: bad argument");
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const int N = rlk->N;
  const size_t row = (size_t)2 * N;
  uint64_t *base = nullptr;
  int rc = ctx_scratch(ctx, 2, 2 * (size_t)count * row, &base);
  if (rc) return rc;
  uint64_t *res = base, *t2 = base + (size_t)count * row;
  hipStream_t s = pick(ctx, stream);
  RING_DISPATCH(ctx, N, {
    hipLaunchKernelGGL(trlwe_tensor_prod_kernel<F>, dim3(count), dim3(F::THREADS), 0, s, d_in1, row, d_in2, row, TW, res, t2, precision);
    hipLaunchKernelGGL(trlwe_fft_keyswitch_kernel<F>, dim3(count), dim3(F::THREADS), 0, s, rlk->d_ak, rlk->d_ak, TW, t2, row, d_out, row, rlk->t, rlk->base_bit, 2, res, row);
  });
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// tlwe_mul [src/tlwe.c:322-332]: both operands packed into TRLWEs, tensor product, sample extract at 0.  in/out strides in words.
static int tlwe_mul_strided(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t pksk, mosfhet_hip_gak_t rlk, uint64_t *d_out, const uint64_t *d_in1, const uint64_t *d_in2,
                            int precision, int count, void *stream) {
  const int N = rlk->N;
  if (!is_packing_key(pksk, N)) return fail(MOSFHET_HIP_EINVAL, "tlwe_mul: ksk must be a packing key N -> TRLWE(N)");
  const size_t row = (size_t)2 * N, lwe = (size_t)count * (N + 1);
  // few ciphertexts: both operands through the packing table in ONE switch (their samples copied side by side; tmp1 and tmp2 are contiguous) -- one table sweep
  // instead of two (capi.hip: cb_levels_together)
  const bool together = cb_levels_together(count, 2);
  uint64_t *base = nullptr;
  int rc = ctx_scratch(ctx, 1, 3 * (size_t)count * row + (together ? 2 * lwe : 0), &base);
  if (rc) return rc;
  uint64_t *tmp1 = base, *tmp2 = tmp1 + (size_t)count * row, *prod = tmp2 + (size_t)count * row, *both = prod + (size_t)count * row;
  hipStream_t s = pick(ctx, stream);
  if (together) {
    HIP_TRY(hipMemcpyAsync(both, d_in1, lwe * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(both + lwe, d_in2, lwe * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    HIP_TRY(launch_tlwe_keyswitch(pksk->d_ksk, tmp1, row, both, (size_t)N + 1, 2 * count, N, 2 * N, N, pksk->t, pksk->base_bit, tl_ws(ctx->device), s, pksk->compressed, pksk->seed));
  } else {
    HIP_TRY(launch_tlwe_keyswitch(pksk->d_ksk, tmp1, row, d_in1, (size_t)N + 1, count, N, 2 * N, N, pksk->t, pksk->base_bit, tl_ws(ctx->device), s, pksk->compressed, pksk->seed));
    HIP_TRY(launch_tlwe_keyswitch(pksk->d_ksk, tmp2, row, d_in2, (size_t)N + 1, count, N, 2 * N, N, pksk->t, pksk->base_bit, tl_ws(ctx->device), s, pksk->compressed, pksk->seed));
  }
  if ((rc = mosfhet_hip_trlwe_tensor_prod_FFT_batch(ctx, rlk, prod, tmp1, tmp2, precision, count, stream))) return rc;
  hipLaunchKernelGGL(trlwe_extract_kernel, dim3((N + 255) / 256, count), dim3(256), 0, s, d_out, (size_t)N + 1, prod, row, N, 1, 0);
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_tlwe_mul_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t pksk, mosfhet_hip_gak_t rlk, uint64_t *d_out, const uint64_t *d_in1,
                                          const uint64_t *d_in2, int precision, int count, void *stream) {
  if (!ctx || !pksk || !rlk || (count > 0 && !d_out) || (count > 0 && !d_in1) || (count > 0 && !d_in2) || count < 0 || precision < 1 || precision > 62) return fail(MOSFHET_HIP_EINVAL, "tlwe_mul: bad argument");
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  return tlwe_mul_strided(ctx, pksk, rlk, d_out, d_in1, d_in2, precision, count, stream);
}

// full_domain_functional_bootstrap_CLOT21 (variant 0, src/bootstrap.c:465-491; d_tv = two TRLWE test vectors [2][2][N]) and _CLOT21_2
// (variant 1, :493-517; d_tv = 2 * 2^(precision-2) cleartext LUT words)
extern "C" int mosfhet_hip_full_domain_functional_bootstrap_CLOT21_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_ksk_t pksk, mosfhet_hip_gak_t rlk,
                                                                         uint64_t *d_out, const uint64_t *d_tv, const uint64_t *d_in, int count, int precision,
                                                                         int variant, void *stream) {
  TUNED_ONLY(bsk, "full_domain_functional_bootstrap_CLOT21");
  if (!ctx || !bsk || !pksk || !rlk || (count > 0 && !d_out) || (count > 0 && !d_tv) || (count > 0 && !d_in) || count < 0 || precision < 2 || precision > 30) return fail(MOSFHET_HIP_EINVAL, "fdfb_CLOT21: bad argument");
  const int N = bsk->N;
  if (rlk->N != N || !is_packing_key(pksk, N)) return fail(MOSFHET_HIP_EINVAL, "fdfb_CLOT21: keys do not match the bootstrap key's ring");
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t row = (size_t)2 * N, lwe = (size_t)count * (N + 1);
  // _CLOT21's three bootstraps per input differ in the test vector only (src/bootstrap.c:476-478): side by side in row mode for batches below a residency round's
  // worth of inputs, like circuit_bootstrap's (capi.hip: cb_bootstraps_together) -- one call is one bootstrap's latency instead of three
  const bool rows3 = variant == 0 && cb_bootstraps_together(bsk, count, 3);
  uint64_t *base = nullptr;
  int rc = ext_scratch(bsk, 0, row + (size_t)count * row + 3 * lwe + (rows3 ? 3 * row + 3 * lwe : 0), &base);
  if (rc) return rc;
  uint64_t *tv = base, *acc = tv + row, *ct_sign = acc + (size_t)count * row, *ct_f0 = ct_sign + lwe, *ct_f1 = ct_f0 + lwe, *tv3 = ct_f1 + lwe, *ext3 = tv3 + 3 * row;
  hipStream_t s = pick(ctx, stream);
  const uint64_t sign = 1ull << (64 - precision - 1);
  if (variant == 0) {
    const int tb = 1 << (precision - 1);
    if (rows3) {
      HIP_TRY(hipMemcpyAsync(tv3, d_tv, 2 * row * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
      hipLaunchKernelGGL(torus_packing_kernel, dim3((N + 255) / 256), dim3(256), 0, s, tv3 + 2 * row, N, (const uint64_t *)nullptr, 1, sign, sign);
      if ((rc = bootstrap_common("full_domain_functional_bootstrap_CLOT21", ctx, bsk, ext3, tv3, 3, d_in, count * 3, 0, 0, 0, tb, 1, 0, stream, 3))) return rc;
      uint64_t *dst[3] = {ct_f0, ct_f1, ct_sign};   // sample 3 b + j is input b under test vector j
      for (int j = 0; j < 3; j++)
        HIP_TRY(hipMemcpy2DAsync(dst[j], (size_t)(N + 1) * sizeof(uint64_t), ext3 + (size_t)j * (N + 1), (size_t)3 * (N + 1) * sizeof(uint64_t), (size_t)(N + 1) * sizeof(uint64_t),
                                 (size_t)count, hipMemcpyDeviceToDevice, s));
    } else {
      hipLaunchKernelGGL(torus_packing_kernel, dim3((N + 255) / 256), dim3(256), 0, s, tv, N, (const uint64_t *)nullptr, 1, sign, sign);
      if ((rc = mosfhet_hip_functional_bootstrap_batch(ctx, bsk, ct_f0, d_tv, 1, d_in, count, tb, stream))) return rc;
      if ((rc = mosfhet_hip_functional_bootstrap_batch(ctx, bsk, ct_f1, d_tv + row, 1, d_in, count, tb, stream))) return rc;
      if ((rc = mosfhet_hip_functional_bootstrap_batch(ctx, bsk, ct_sign, tv, 1, d_in, count, tb, stream))) return rc;
    }
  } else {
    const int tb = 1 << (precision - 2), slot = N / (4 * tb);
    if (N % (4 * tb)) return fail(MOSFHET_HIP_EINVAL, "fdfb_CLOT21_2: N not divisible by 4 * torus_base");
    hipLaunchKernelGGL(clot21_lut_kernel, dim3((N + 255) / 256), dim3(256), 0, s, tv, d_tv, sign, N, tb);
    if ((rc = mosfhet_hip_functional_bootstrap_wo_extract_batch(ctx, bsk, acc, tv, 1, d_in, count, 4 * tb, stream))) return rc;
    hipLaunchKernelGGL(trlwe_extract_kernel, dim3((N + 255) / 256, count), dim3(256), 0, s, ct_f0, (size_t)N + 1, acc, row, N, 1, 0);
    hipLaunchKernelGGL(trlwe_extract_kernel, dim3((N + 255) / 256, count), dim3(256), 0, s, ct_f1, (size_t)N + 1, acc, row, N, 1, slot);
    hipLaunchKernelGGL(trlwe_extract_kernel, dim3((N + 255) / 256, count), dim3(256), 0, s, ct_sign, (size_t)N + 1, acc, row, N, 1, 2 * slot);
  }
  hipLaunchKernelGGL(tlwe_add_to_word_kernel, dim3((count + 255) / 256), dim3(256), 0, s, ct_sign, count, (size_t)N + 1, ((size_t)N + 1) - 1, (uint64_t)0 - sign);
  if ((rc = tlwe_mul_strided(ctx, pksk, rlk, ct_f1, ct_f1, ct_sign, precision, count, stream))) return rc;
  hipLaunchKernelGGL(tlwe_add_to_word_kernel, dim3((count + 255) / 256), dim3(256), 0, s, ct_sign, count, (size_t)N + 1, ((size_t)N + 1) - 1, 2 * sign);
  if ((rc = tlwe_mul_strided(ctx, pksk, rlk, ct_f0, ct_f0, ct_sign, precision, count, stream))) return rc;
  HIP_TRY(hipMemcpyAsync(d_out, ct_f0, lwe * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
  return mosfhet_hip_tlwe_addto_batch(ctx, d_out, ct_f1, N, count, stream);
}

// ---- blind-rotate unfolding ----
// Key of new_bootstrap_key(out_key, in_key, unfolding > 1) [src/bootstrap.c:23-48]: h_su = Torus[n 2^u / u][2l][2][N], torus domain.
// The handle is an ordinary bootstrap-key handle: every bootstrap entry point dispatches on it as the reference dispatches on
// key->unfolding (src/bootstrap.c:196-197).
// Unfolding 2: the rotation multiplies in the DFT domain (unfold_kernels.h), so the samples are transformed once, here.  The torus-domain samples stay:
// they are the key's exported form and what multivalue_bootstrap_UBR_phase1 assembles its selectors from.
// Made when the key is created or cloned (a replica on another GPU transforms its own), so that a bootstrap launch never allocates, never touches the
// null stream and cannot run into a stream capture or a first-call stall.  The copy doubles the key's device footprint (lvl2, u = 2: 2 x 330 MB): a process
// that keeps the torus-domain assembly (MOSFHET_HIP_UNFOLD2_DFT=0 at creation) does not pay for it; should it switch the DFT path on later
// (mosfhet_hip_set_unfold2_dft), the first rotation makes the copy under the handle's lock -- that one call must be outside any capture.
static bool unfold2_dft_enabled();
static bool unfold2_capable(const mosfhet_hip_bsk *b) { return b->unfolding == 2 && b->l <= 6; }   // (pbs_unfold2_kernel is instantiated for l <= 6; longer gadgets keep the run-time-l torus-domain kernels)
static int unfold2_ready(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk *b) {
  if (b->su_dft_ready.load(std::memory_order_acquire)) return MOSFHET_HIP_OK;
  std::lock_guard<std::mutex> hold(b->su_dft_lock);
  if (b->su_dft_ready.load(std::memory_order_relaxed)) return MOSFHET_HIP_OK;
  int caller_dev = -1;
  (void)hipGetDevice(&caller_dev);
  struct Restore { int d; ~Restore() { if (d >= 0) (void)hipSetDevice(d); } } restore{caller_dev};   // the caller's current device stays what it was
  HIP_TRY(hipSetDevice(b->device));
  d2 *dft = nullptr;
  HIP_TRY(hipMalloc((void **)&dft, b->bytes));
  const size_t polys = (size_t)b->n / 2 * 4 * 2 * b->l * 2;
  (void)ctx;   // the key's own context: its device holds the samples and the twiddle table that transforms them
  RING_DISPATCH(b->ctx, b->N, hipLaunchKernelGGL(torus_to_dft_kernel<F>, dim3((unsigned)polys), dim3(F::THREADS), 0, nullptr, b->d_su, dft, TW));
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) { (void)hipFree(dft); return fail(MOSFHET_HIP_EHIP, "unfolding 2: transforming the key samples: %s", hipGetErrorString(e)); }
  b->d_su_dft = dft;
  b->su_dft_ready.store(1, std::memory_order_release);
  return MOSFHET_HIP_OK;
}

// pbs_unfold2_kernel: the reference gadgets; run-time gadgets l = 1 .. 6
constexpr bool unfold2_gadgets(int N, int L, int BG) { return BG == 0 || reference_gadget(N, L, BG); }

// bounded = true below: unfolding-2 keys are always samples this library transformed itself (unfold2_ready); no key view reaches this launcher.
template <class F>
static int launch_unfold2_f(int l, int Bg_bit, const Unfold2Params &u, int count, hipStream_t s) {
  // N = 2048: the transformed samples (1.5 x a plain key) do not fit the L2s either -- one launch per residency round, like launch_pbs (4096 at lvl2: 120.9 -> 99.7 ms)
  // (the per-XCD rendezvous of the plain kernel was tried here too: 100.8 against 99.7 ms per 4096 without it -- not adopted)
  const int round = F::N == 2048 ? round_chunk(F::THREADS) : 0;
  return gadget_dispatch<F::N, unfold2_gadgets>(l, Bg_bit, true, [&](auto L, auto BG) {
    launch_rounds<F::N>(pbs_unfold2_kernel<F, L, BG>, F::THREADS, u, count, round, false, s);
    return launched();
  });
}

extern "C" int mosfhet_hip_bsk_unfolded_create(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t *out, const uint64_t *h_su, int n, int N, int l, int Bg_bit,
                                               int unfolding) {
  if (!ctx || !out || !h_su) return fail(MOSFHET_HIP_EINVAL, "bsk_unfolded_create: bad argument");
  if (!ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "bsk_unfolded_create: N = %d not supported (1024, 2048, 4096)", N);
  // src/bootstrap.c:34-45 places group i at su[i * (2^u / u)] with an INTEGER quotient: for u = 3, 5, 6, 7 consecutive groups overlap (and the
  // reference writes past its own allocation), so only powers of two describe a usable key
  if ((unfolding != 2 && unfolding != 4 && unfolding != 8) || n % unfolding)
    return fail(MOSFHET_HIP_EINVAL, "bsk_unfolded_create: unfolding must be 2, 4 or 8 with n divisible by it (test/tests.c:34; the reference's key layout, "
                                    "src/bootstrap.c:34-45, is only consistent for powers of two)");
  if (l < 1 || Bg_bit < 1 || l * Bg_bit >= 64 || Bg_bit > 31) return fail(MOSFHET_HIP_EINVAL, "bsk_unfolded_create: bad gadget");
  HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<mosfhet_hip_bsk> b_owner(new mosfhet_hip_bsk());
  mosfhet_hip_bsk *b = b_owner.get();
  b->ctx = ctx; b->device = ctx->device; b->d_bk = nullptr; b->n = n; b->k = 1; b->N = N; b->l = l; b->Bg_bit = Bg_bit; b->unfolding = unfolding;
  b->bytes = (size_t)n * ((size_t)1 << unfolding) / unfolding * 2 * l * 2 * N * sizeof(uint64_t);
  HIP_TRY(hipMalloc((void **)&b->d_su, b->bytes));
  HIP_TRY(hipMemcpy(b->d_su, h_su, b->bytes, hipMemcpyHostToDevice));
  if (unfold2_capable(b) && unfold2_dft_enabled()) {
    const int rc = unfold2_ready(ctx, b);
    if (rc) return rc;
  }
  *out = b_owner.release();
  return MOSFHET_HIP_OK;
}

// programmable_bootstrap's input scaling (src/bootstrap.c:213-217) as its own pass, for the kernels that do not fuse it
__global__ void pbs_pre_kernel(uint64_t *__restrict__ out, const uint64_t *__restrict__ in, size_t words, int kappa, int theta, int log2N2) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= words) return;
  const uint64_t rnd = 1ull << (64 - log2N2 + theta - 1), msk = ~((1ull << (64 - log2N2 + theta)) - 1);
  out[i] = ((in[i] << kappa) + rnd) & msk;
}

// ciphertexts per chunk of the two-phase unfolded bootstrap (-1: the default of 64, capped by 2 GiB of selectors; 0: always the fused kernel)
static std::atomic<int> g_unfold_split_max{-2};
static int unfold_split_max() {
  if (g_unfold_split_max == -2) {
    const char *e = getenv("MOSFHET_HIP_UNFOLD_SPLIT_MAX");
    g_unfold_split_max = e ? atoi(e) : -1;
  }
  return g_unfold_split_max;
}
extern "C" int mosfhet_hip_set_unfold_split_max(int max_batch) {
  g_unfold_split_max = max_batch < -1 ? -1 : max_batch;
  return MOSFHET_HIP_OK;
}

// phase 2 of the unfolded rotation: one team per (ciphertext, test vector); few units on N = 1024 / 2048: two transform teams each (ubr_phase2_wide_kernel,
// bit-identical; the switch-overs of pbs_team_kernel / pbs_wide_team_kernel)
static int launch_ubr_phase2(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, hipStream_t s, const d2 *sa, const uint64_t *d_in, const uint64_t *d_tvs, uint64_t *acc, int units,
                             int tv_count, uint64_t prec, long long tv_stride_b = 0) {
  const int N = bsk->N, groups = bsk->n / bsk->unfolding;
  if (N == 2048 && units <= wide_team_max_batch()) {
    using F = Fft2048;
    return launch_dyn_lds(ubr_phase2_wide_kernel<F>, dim3(units), dim3(2 * F::THREADS), kWideLds<F>, s, sa, ctx->tw2048, d_in, d_tvs, acc, bsk->n, bsk->l, bsk->Bg_bit, groups,
                          tv_count, prec, tv_stride_b);
  } else if (N == 1024 && units <= team_max_batch()) {
    using F = Fft1024;   // (< 48 KiB of LDS: no attribute needed)
    hipLaunchKernelGGL(ubr_phase2_wide_kernel<F>, dim3(units), dim3(2 * F::THREADS), kWideLds<F>, s, sa, ctx->tw1024, d_in, d_tvs, acc, bsk->n, bsk->l, bsk->Bg_bit, groups, tv_count, prec,
                       tv_stride_b);
  } else {
    RING_DISPATCH(ctx, N, hipLaunchKernelGGL(ubr_phase2_kernel<F>, dim3(units), dim3(F::THREADS), 0, s, sa, TW, d_in, d_tvs, acc, bsk->n, bsk->l, bsk->Bg_bit, groups, tv_count, prec, tv_stride_b));
  }
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// MOSFHET_HIP_UNFOLD2_DFT=0 / mosfhet_hip_set_unfold2_dft(0): unfolding-2 keys rotate through the torus-domain assembly like u = 4 and 8 (the order of
// operations of oracle_ext.c:orc_blind_rotate_unfolded instead of orc_blind_rotate_unfolded2_dft)
static std::atomic<int> g_unfold2_dft{-1};
static bool unfold2_dft_enabled() {
  if (g_unfold2_dft < 0) {
    const char *e = getenv("MOSFHET_HIP_UNFOLD2_DFT");
    g_unfold2_dft = e ? (atoi(e) != 0) : 1;
  }
  return g_unfold2_dft != 0;
}
extern "C" int mosfhet_hip_set_unfold2_dft(int on) {
  g_unfold2_dft = on ? 1 : 0;
  return MOSFHET_HIP_OK;
}

static int bootstrap_unfolded(const char *who, mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, uint64_t *d_out, const uint64_t *d_tv, int tv_count,
                              const uint64_t *d_in, int count, int pre, int kappa, int theta, int torus_base, int extract, int skip_init, void *stream, int rows) {
  if (skip_init || rows != 1) return fail(MOSFHET_HIP_EINVAL, "%s: not available with an unfolded key", who);
  const int N = bsk->N;
  hipStream_t s = pick(ctx, stream);
  bool dft2 = false;
  if (unfold2_capable(bsk) && unfold2_dft_enabled()) {
    const int rc2 = unfold2_ready(ctx, bsk);
    if (rc2) return rc2;
    dft2 = true;
  }
  // Few ciphertexts: the per-group selectors of ALL groups are made side by side first (torus domain: ubr_phase1_kernel assembles  sum_j X^(rot_j) su_j  and
  // transforms it, one team per polynomial, (k+1)^2 l n/u of them per ciphertext; unfolding 2: unfold2_select_kernel forms them from the transformed
  // samples), then one team per ciphertext walks the n/u external products (ubr_phase2_kernel).  The same sums, transforms and fma chains as the
  // one-kernel forms -- bit-identical -- but a single bootstrap at lvl2 takes 6 / 3 / 4 ms at u = 2 / 4 / 8 instead of 147 / 286 / 2365 ms (torus domain) or
  // 23 ms (unfold2), where one team streams the 2^u samples of every group on its own.  Large batches take one kernel: it needs no selector storage (n/u
  // TRGSW_DFT per ciphertext) and the chip is full either way.  Switch-over: 8 chunks of 64 (torus domain: its fused kernel is slow), 48 ciphertexts
  // (unfolding 2, measured at lvl2: 6 / 9 / ~20 ms for 1 / 16 / 64 against 21 - 23 ms flat up to ~500); MOSFHET_HIP_UNFOLD_SPLIT_MAX /
  // mosfhet_hip_set_unfold_split_max override it (0: never).
  const int split_env = unfold_split_max();
  const int groups = bsk->n / bsk->unfolding;
  const size_t sa_words = (size_t)groups * 2 * bsk->l * 2 * N;                  // doubles per ciphertext
  static const size_t budget_gib = getenv("MOSFHET_HIP_UNFOLD_BUDGET_GIB") ? (size_t)atoi(getenv("MOSFHET_HIP_UNFOLD_BUDGET_GIB")) : 2;
  const size_t budget = budget_gib << 27;                                        // words: 2 GiB of selectors unless told otherwise
  int split_max = split_env >= 0 ? split_env : (dft2 ? 48 : 64);
  const int split_upto = dft2 ? split_max : 8 * split_max;                       // largest batch that goes selectors-first
  if ((size_t)split_max * sa_words > budget) split_max = (int)(budget / sa_words);
  const bool split = split_max > 0 && count <= split_upto;
  if (dft2 && !split) {
    // no temporaries; the input scaling of programmable_bootstrap is applied as the words are read
    Unfold2Params u;
    u.p.bk = bsk->d_su_dft;
    u.p.tw = N == 1024 ? ctx->tw1024 : (N == 2048 ? ctx->tw2048 : ctx->tw4096);
    u.p.in = d_in; u.p.tv = d_tv; u.p.out = d_out;
    u.p.tv_stride = tv_count == 1 ? 0 : (long long)2 * N;
    u.p.n = bsk->n; u.p.Bg_bit = bsk->Bg_bit;
    u.p.pre = pre; u.p.kappa = kappa; u.p.theta = theta;
    u.p.prec_offset = (uint64_t)((int64_t)(18446744073709551616.0 * (1. / (4 * (double)torus_base))));
    u.p.extract = extract; u.p.skip_init = 0;
    u.wtab = ctx->wtab[N == 1024 ? 0 : (N == 2048 ? 1 : 2)];
    int rc_u = MOSFHET_HIP_OK;
    RING_DISPATCH(ctx, N, rc_u = launch_unfold2_f<F>(bsk->l, bsk->Bg_bit, u, count, s));
    return rc_u;
  }
  uint64_t *acc = d_out;
  const size_t w_acc = extract ? (size_t)count * 2 * N : 0, w_in = pre ? (size_t)count * (bsk->n + 1) : 0;
  if (w_acc + w_in) {
    // temporaries of the calling thread: callers that spread unfolded bootstraps over several streams order them themselves (mosfhet_hip.h)
    uint64_t *tmp = nullptr;
    int rc = ext_scratch(bsk, 1, w_acc + w_in, &tmp);
    if (rc) return rc;
    if (extract) acc = tmp;
    if (pre) {
      // programmable_bootstrap = scaled input + functional_bootstrap, which dispatches on key->unfolding (src/bootstrap.c:208-219,196-197)
      int log2N2 = 1;
      while ((1 << log2N2) < 2 * N) log2N2++;
      uint64_t *scaled = tmp + w_acc;
      hipLaunchKernelGGL(pbs_pre_kernel, dim3((unsigned)((w_in + 255) / 256)), dim3(256), 0, s, scaled, d_in, w_in, kappa, theta, log2N2);
      d_in = scaled;
    }
  }
  {
    if (split) {
      const int chunk = count < split_max ? count : split_max;
      uint64_t *sa = nullptr;
      int rc = pool_get(ctx->device, POOL_UNFOLD, (size_t)chunk * sa_words, &sa);
      if (rc) return rc;
      const uint64_t prec = (uint64_t)((int64_t)(18446744073709551616.0 * (1. / (4 * (double)torus_base))));
      for (int lo = 0; lo < count; lo += chunk) {
        const int c = count - lo < chunk ? count - lo : chunk;
        const uint64_t *in_c = d_in + (size_t)lo * (bsk->n + 1);
        const dim3 grid1(2 * bsk->l * 2, groups, c);
        RING_DISPATCH(ctx, N, {
          if (dft2) hipLaunchKernelGGL(unfold2_select_kernel<F>, grid1, dim3(F::THREADS), 0, s, bsk->d_su_dft, ctx->wtab[N == 1024 ? 0 : (N == 2048 ? 1 : 2)], in_c, (d2 *)sa, bsk->n, bsk->l);
          else hipLaunchKernelGGL(ubr_phase1_kernel<F>, grid1, dim3(F::THREADS), 0, s, bsk->d_su, TW, in_c, (d2 *)sa, bsk->n, bsk->l, bsk->unfolding);
        });
        const long long tv_stride_b = tv_count == 1 ? 0 : (long long)2 * N;   // one test vector per ciphertext: the chunk's first
        if ((rc = launch_ubr_phase2(ctx, bsk, s, (const d2 *)sa, in_c, d_tv + (size_t)lo * (size_t)tv_stride_b, acc + (size_t)lo * 2 * N, c, 1, prec, tv_stride_b))) return rc;
      }
      if (extract) hipLaunchKernelGGL(trlwe_extract_kernel, dim3((N + 255) / 256, count), dim3(256), 0, s, d_out, (size_t)N + 1, acc, (size_t)2 * N, N, 1, 0);
      HIP_TRY(hipGetLastError());
      return MOSFHET_HIP_OK;
    }
  }
  UnfoldParams p;
  p.su = bsk->d_su;
  p.tw = N == 1024 ? ctx->tw1024 : (N == 2048 ? ctx->tw2048 : ctx->tw4096);
  p.in = d_in;
  p.tv = d_tv;
  p.out = acc;
  p.tv_stride = tv_count == 1 ? 0 : (long long)2 * N;
  p.n = bsk->n; p.l = bsk->l; p.Bg_bit = bsk->Bg_bit; p.unfolding = bsk->unfolding;
  p.prec_offset = (uint64_t)((int64_t)(18446744073709551616.0 * (1. / (4 * (double)torus_base))));
  RING_DISPATCH(ctx, N, hipLaunchKernelGGL(pbs_unfolded_kernel<F>, dim3(count), dim3(F::THREADS), 0, s, p));
  if (extract) hipLaunchKernelGGL(trlwe_extract_kernel, dim3((N + 255) / 256, count), dim3(256), 0, s, d_out, (size_t)N + 1, acc, (size_t)2 * N, N, 1, 0);
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// multivalue_bootstrap_UBR_phase1 / phase2 [src/bootstrap.c:151-190] with an unfolded key: phase 1 depends on the input's mask only and
// yields n / u TRGSW_DFT per ciphertext (d_sa: [count][n/u][2l][2][N/2] complex, slot order); phase 2 evaluates tv_count test vectors
// (shared by the batch) per ciphertext against them: d_out[b][v] = TLWE.
extern "C" int mosfhet_hip_multivalue_bootstrap_UBR_phase1_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, double *d_sa, const uint64_t *d_in, int count,
                                                                 void *stream) {
  TUNED_ONLY(bsk, "multivalue_bootstrap_UBR_phase1");
  if (!ctx || !bsk || (count > 0 && !d_sa) || (count > 0 && !d_in) || count < 0 || bsk->unfolding < 2) return fail(MOSFHET_HIP_EINVAL, "UBR_phase1: needs an unfolded key");
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const dim3 grid(2 * bsk->l * 2, bsk->n / bsk->unfolding, count);
  RING_DISPATCH(ctx, bsk->N, hipLaunchKernelGGL(ubr_phase1_kernel<F>, grid, dim3(F::THREADS), 0, pick(ctx, stream), bsk->d_su, TW, d_in, (d2 *)d_sa, bsk->n, bsk->l,
                                                bsk->unfolding));
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_multivalue_bootstrap_UBR_phase2_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, uint64_t *d_out, const uint64_t *d_tvs, int tv_count,
                                                                 const uint64_t *d_in, const double *d_sa, int count, int torus_base, void *stream) {
  TUNED_ONLY(bsk, "multivalue_bootstrap_UBR_phase2");
  if (!ctx || !bsk || (count > 0 && !d_out) || (count > 0 && !d_tvs) || (count > 0 && !d_in) || (count > 0 && !d_sa) || count < 0 || tv_count < 1 || torus_base < 1 || bsk->unfolding < 2)
    return fail(MOSFHET_HIP_EINVAL, "UBR_phase2: bad argument (needs an unfolded key)");
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const int N = bsk->N, units = count * tv_count;
  uint64_t *acc = nullptr;
  int rc = ext_scratch(bsk, 1, (size_t)units * 2 * N, &acc);
  if (rc) return rc;
  const uint64_t prec = (uint64_t)((int64_t)(18446744073709551616.0 * (1. / (4 * (double)torus_base))));
  hipStream_t s = pick(ctx, stream);
  if ((rc = launch_ubr_phase2(ctx, bsk, s, (const d2 *)d_sa, d_in, d_tvs, acc, units, tv_count, prec))) return rc;
  hipLaunchKernelGGL(trlwe_extract_kernel, dim3((N + 255) / 256, units), dim3(256), 0, s, d_out, (size_t)N + 1, acc, (size_t)2 * N, N, 1, 0);
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// trlwe_mv_extract_tlwe (mode 0: d_out = [count][amount][N+1]) / _scaling (1) / _scaling_addto (2) / _scaling_subto (3: d_out = [count][N+1])
extern "C" int mosfhet_hip_trlwe_mv_extract_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const uint64_t *d_in, int N, int mode, int amount, int count,
                                                  void *stream) {
  if (!ctx || (count > 0 && !d_out) || (count > 0 && !d_in) || count < 0 || mode < 0 || mode > 3 || amount < 1 || amount > N) return fail(MOSFHET_HIP_EINVAL, "mv_extract: bad argument");
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(mv_extract_kernel, dim3((N + 255) / 256, mode == 0 ? amount : 1, count), dim3(256), 0, pick(ctx, stream), d_in, d_out, N, mode, amount);
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// the key generators keep the TRLWE key's nonzero coefficients as 16-bit integers (binary, ternary, bounded and narrow Gaussian keys all fit)
static bool trlwe_key_fits(const uint64_t *h_s, int N) {
  for (int i = 0; i < N; i++) {
    const int64_t v = (int64_t)h_s[i];
    if (v > 32767 || v < -32768) return false;
  }
  return true;
}

// ---- on-device generation of the table-lookup TRLWE keys (SURVEY 8(f).1) ----
// kind 0: packing key (trlwe_new_packing1_KS_key, src/keyswitch.c:368-390); kind 1: private key (trlwe_new_priv_SK_KS_key_N2, :611-637).
// h_s_out: the N words of the binary TRLWE key, h_s_in: the n words of the LWE key being switched from.
static int table_ksk_generate(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, int kind, const uint64_t *h_s_out, int N, const uint64_t *h_s_in, int n, int t,
                              int base_bit, double sigma, uint64_t seed, int compressed, int slots = 1) {
  if (!ctx || !out || !h_s_out || !h_s_in || kind < 0 || kind > 2 || slots < 1 || (kind == 2 && (N % slots || compressed)) || n < 1 || t < 1 || base_bit < 1 || base_bit > 8 || t * base_bit >= 64)
    return fail(MOSFHET_HIP_EINVAL, "table_ksk_generate: bad argument");
  if (N < 256 || N > 4096 || (N & (N - 1))) return fail(MOSFHET_HIP_EINVAL, "table_ksk_generate: N must be a power of two in 256..4096");
  if (!trlwe_key_fits(h_s_out, N)) return fail(MOSFHET_HIP_EINVAL, "table_ksk_generate: TRLWE key coefficients must fit 16 bits");
  HIP_TRY(hipSetDevice(ctx->device));
  const int entries = kind == 2 ? n * slots : n + kind, cands = (1 << base_bit) - 1;
  const size_t n_rows = (size_t)entries * t * cands;
  std::unique_ptr<mosfhet_hip_ksk> k_owner(new mosfhet_hip_ksk());
  mosfhet_hip_ksk *k = k_owner.get();
  k->ctx = ctx; k->device = ctx->device; k->n_in = entries; k->n_out = 2 * N - 1; k->t = t; k->base_bit = base_bit;
  k->row = 2 * N; k->b_word = kind == 0 ? N : -1;
  k->compressed = compressed != 0; k->seed = seed;
  k->bytes = n_rows * (compressed ? 1 : 2) * N * sizeof(uint64_t);
  DevBuf keys;                                     // the two secret keys on the device, released on every way out
  HIP_TRY(hipMalloc((void **)&k->d_ksk, k->bytes + ksw_slack_bytes(k->row)));   // (+ slack: the word-lane key switch reads past the last row, keyswitch_words_kernels.h)
  HIP_TRY(keys.alloc(((size_t)N + n) * sizeof(uint64_t)));
  uint64_t *d_keys = keys.as<uint64_t>();
  HIP_TRY(hipMemcpy(d_keys, h_s_out, (size_t)N * sizeof(uint64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_keys + N, h_s_in, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
  const size_t lds = (size_t)N * sizeof(uint64_t) + (size_t)N * 2 * sizeof(uint16_t);
  const NoiseKey nkey = noise_key_for_call(NOISE_TABLE);
  for (size_t first = 0; first < n_rows; first += 1u << 20) {   // grid.x stays far below 2^31
    const size_t chunk = n_rows - first < (1u << 20) ? n_rows - first : (1u << 20);
    hipLaunchKernelGGL(trlwe_table_keygen_kernel, dim3((unsigned)chunk), dim3(256), lds, nullptr, k->d_ksk, d_keys, d_keys + N, n, N, t, base_bit, sigma, seed, kind,
                       first, compressed, nkey, slots);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  *out = k_owner.release();
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_trlwe_table_ksk_generate(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, int kind, const uint64_t *h_s_out, int N, const uint64_t *h_s_in,
                                                    int n, int t, int base_bit, double sigma, uint64_t seed) {
  return table_ksk_generate(ctx, out, kind, h_s_out, N, h_s_in, n, t, base_bit, sigma, seed, 0);
}

// Seed-compressed form of the same key (SURVEY 8(f).2; the reference's USE_COMPRESSED_TRLWE rows, src/keyswitch.c:231-241): identical rows for the
// same seed, but only the b halves are kept in HBM; the key switches regenerate the masks (keyswitch_kernels.h, MASKGEN).
extern "C" int mosfhet_hip_trlwe_table_ksk_generate_compressed(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, int kind, const uint64_t *h_s_out, int N,
                                                               const uint64_t *h_s_in, int n, int t, int base_bit, double sigma, uint64_t seed) {
  return table_ksk_generate(ctx, out, kind, h_s_out, N, h_s_in, n, t, base_bit, sigma, seed, 1);
}

// tlwe_keyswitch_no_precomp (src/tlwe.c:305-320) on a key held as plain device rows [n_in][t][n_out + 1] (one TLWE sample per input word and digit
// position, scaled by the digit in the kernel): d_in [count][n_in + 1] -> d_out [count][n_out + 1]
extern "C" int mosfhet_hip_tlwe_keyswitch_no_precomp_batch(mosfhet_hip_ctx_t ctx, const uint64_t *d_rows, uint64_t *d_out, const uint64_t *d_in, int count, int n_in,
                                                           int n_out, int t, int base_bit, void *stream) {
  if (!ctx || count < 0 || n_in < 1 || n_out < 1 || t < 1 || base_bit < 1 || base_bit > 16 || t * base_bit >= 63) return fail(MOSFHET_HIP_EINVAL, "keyswitch_no_precomp: bad argument");
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_rows || !d_out || !d_in) return fail(MOSFHET_HIP_EINVAL, "keyswitch_no_precomp: null buffer");
  if (count > 65535) return fail(MOSFHET_HIP_EINVAL, "keyswitch_no_precomp: count = %d (at most 65535 samples per call: the kernels index the batch by gridDim.z and gridDim.y)", count);
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(launch_tlwe_keyswitch_scaled(d_rows, d_out, (size_t)n_out + 1, d_in, (size_t)n_in + 1, count, n_in, n_out + 1, t, base_bit, tl_ws(ctx->device), pick(ctx, stream)));
  return MOSFHET_HIP_OK;
}

// LUT-packing key (trlwe_new_packing_KS_key, src/keyswitch.c:214-241): the table of trlwe_packing_keyswitch, which packs `torus_base` LWE samples into the
// `torus_base` slots of one TRLWE sample.  Entry (i, e) = i * torus_base + e; a key with n * torus_base digit sources and no b word (ksk kind 2).
extern "C" int mosfhet_hip_trlwe_lut_packing_ksk_generate(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, const uint64_t *h_s_out, int N, const uint64_t *h_s_in, int n,
                                                          int t, int base_bit, int torus_base, double sigma, uint64_t seed) {
  return table_ksk_generate(ctx, out, 2, h_s_out, N, h_s_in, n, t, base_bit, sigma, seed, 0, torus_base);
}

// trlwe_packing_keyswitch (src/keyswitch.c:346-366) for a batch: d_in [count][torus_base][n + 1] (the LWE samples of one packing next to each other),
// d_out [count][2][N]:  out = (0, b_e on slot e) - sum_{i, e, j} KS[i][e][j][digit_j(in_e.a_i)]
namespace mosfhet {
__global__ void lut_packing_gather_kernel(uint64_t *__restrict__ words, const uint64_t *__restrict__ in, int n, int slots, size_t total) {
  const size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // word (b, i, e) of the digit-source vectors
  if (x >= total) return;
  const size_t per = (size_t)n * slots, b = x / per, w = x % per;
  const int i = (int)(w / slots), e = (int)(w % slots);
  words[x] = in[(b * slots + e) * (size_t)(n + 1) + i];
}
__global__ void lut_packing_addb_kernel(uint64_t *__restrict__ out, const uint64_t *__restrict__ in, int n, int N, int slots, size_t total) {
  const size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // coefficient (b, q) of the b polynomials
  if (x >= total) return;
  const size_t b = x / N;
  const int q = (int)(x % N), e = q / (N / slots);
  out[b * 2 * (size_t)N + N + q] += in[(b * slots + e) * (size_t)(n + 1) + n];
}
}  // namespace mosfhet

extern "C" int mosfhet_hip_trlwe_lut_packing_keyswitch_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, int torus_base, uint64_t *d_out, const uint64_t *d_in,
                                                             int count, void *stream) {
  if (!ctx || !ksk || count < 0 || torus_base < 1) return fail(MOSFHET_HIP_EINVAL, "lut_packing_keyswitch: bad argument");
  if (ksk->b_word >= 0 || ksk->n_in % torus_base || (ksk->row / 2) % torus_base) return fail(MOSFHET_HIP_EINVAL, "lut_packing_keyswitch: not a LUT-packing key for this torus_base");
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_in) return fail(MOSFHET_HIP_EINVAL, "lut_packing_keyswitch: null buffer");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  const int N = ksk->row / 2, n = ksk->n_in / torus_base;
  uint64_t *words = nullptr;
  int rc = pool_get(ctx->device, POOL_PACK, (size_t)count * ksk->n_in, &words);
  if (rc) return rc;
  const size_t total = (size_t)count * ksk->n_in, totb = (size_t)count * N;
  hipLaunchKernelGGL(lut_packing_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, words, d_in, n, torus_base, total);
  HIP_TRY(launch_tlwe_keyswitch(ksk->d_ksk, d_out, (size_t)ksk->row, words, (size_t)ksk->n_in, count, ksk->n_in, ksk->row, -1, ksk->t, ksk->base_bit, tl_ws(ctx->device), s,
                                ksk->compressed, ksk->seed));
  hipLaunchKernelGGL(lut_packing_addb_kernel, dim3((unsigned)((totb + 255) / 256)), dim3(256), 0, s, d_out, d_in, n, N, torus_base, totb);
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

extern "C" size_t mosfhet_hip_ksk_bytes(mosfhet_hip_ksk_t ksk) { return ksk ? ksk->bytes : 0; }

// On-device generation of the bootstrap key itself (new_bootstrap_key, src/bootstrap.c:3-21; ga != 0: the TRGSW(X^{s_i}) samples of
// new_bootstrap_key_ga, src/bootstrap_ga.c:5-24): encrypt in the torus domain, then the engine's own forward transform -- no host key, no upload.
extern "C" int mosfhet_hip_bsk_generate(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t *out, const uint64_t *h_s_rlwe, int N, const uint64_t *h_s_lwe, int n, int l,
                                        int Bg_bit, double sigma, uint64_t seed, int ga) {
  if (!ctx || !out || !h_s_rlwe || !h_s_lwe || n < 1) return fail(MOSFHET_HIP_EINVAL, "bsk_generate: bad argument");
  int rc = check_params("bsk_generate", 1, N, l, Bg_bit);
  if (rc) return rc;
  if (!trlwe_key_fits(h_s_rlwe, N)) return fail(MOSFHET_HIP_EINVAL, "bsk_generate: TRLWE key coefficients must fit 16 bits");
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n_rows = (size_t)n * 2 * l, words = n_rows * 2 * N;
  uint64_t *d_bk = nullptr, *d_keys = nullptr;
  hipError_t e = hipMalloc((void **)&d_bk, words * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMalloc((void **)&d_keys, ((size_t)N + n) * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMemcpy(d_keys, h_s_rlwe, (size_t)N * sizeof(uint64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_keys + N, h_s_lwe, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(trgsw_bk_keygen_kernel, dim3((unsigned)n_rows), dim3(256), (size_t)N * sizeof(uint64_t) + (size_t)N * 2 * sizeof(uint16_t), nullptr, d_bk, d_keys,
                       d_keys + N, N, l, Bg_bit, sigma, seed, ga, noise_key_for_call(NOISE_BSK));
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    if (d_bk) hipFree(d_bk);
    if (d_keys) hipFree(d_keys);
    return fail(MOSFHET_HIP_EHIP, "bsk_generate: %s", hipGetErrorString(e));
  }
  rc = mosfhet_hip_bsk_create_from_device(ctx, out, d_bk, n, 1, N, l, Bg_bit, nullptr);
  hipStreamSynchronize(nullptr);
  hipFree(d_bk);
  hipFree(d_keys);
  return rc;
}

// ... for any k <= 3 and power-of-two ring the engine serves (the general-ring path too): h_s_rlwe = the k key polynomials [k][N].  k = 1 on a tuned ring is
// mosfhet_hip_bsk_generate.  N <= 8192 (the generator keeps one mask and the key's support in LDS: 12 N bytes).
extern "C" int mosfhet_hip_bsk_generate_k(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t *out, const uint64_t *h_s_rlwe, int k, int N, const uint64_t *h_s_lwe, int n, int l,
                                          int Bg_bit, double sigma, uint64_t seed) {
  if (!ctx || !out || !h_s_rlwe || !h_s_lwe || n < 1) return fail(MOSFHET_HIP_EINVAL, "bsk_generate_k: bad argument");
  int rc = check_params("bsk_generate_k", k, N, l, Bg_bit, true);
  if (rc) return rc;
  if (!general_ring(k, N)) return mosfhet_hip_bsk_generate(ctx, out, h_s_rlwe, N, h_s_lwe, n, l, Bg_bit, sigma, seed, 0);
  if (N > 8192) return fail(MOSFHET_HIP_EINVAL, "bsk_generate_k: N = %d: the device generator serves rings up to 8192 (upload a host-made key with mosfhet_hip_bsk_create)", N);
  for (int m = 0; m < k; m++)
    if (!trlwe_key_fits(h_s_rlwe + (size_t)m * N, N)) return fail(MOSFHET_HIP_EINVAL, "bsk_generate_k: TRLWE key coefficients must fit 16 bits");
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n_rows = (size_t)n * (k + 1) * l, words = n_rows * (k + 1) * N, lds = (size_t)N * 12;
  DevBuf bk, keys;
  HIP_TRY(bk.alloc(words * sizeof(uint64_t)));
  HIP_TRY(keys.alloc(((size_t)k * N + n) * sizeof(uint64_t)));
  uint64_t *d_keys = keys.as<uint64_t>();
  HIP_TRY(hipMemcpy(d_keys, h_s_rlwe, (size_t)k * N * sizeof(uint64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_keys + (size_t)k * N, h_s_lwe, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
  if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(trgsw_bk_keygen_k_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(trgsw_bk_keygen_k_kernel, dim3((unsigned)n_rows), dim3(256), lds, nullptr, bk.as<uint64_t>(), d_keys, d_keys + (size_t)k * N, k, N, l, Bg_bit, sigma, seed,
                     noise_key_for_call(NOISE_BSK));
  HIP_TRY(hipGetLastError());
  rc = mosfhet_hip_bsk_create_from_device(ctx, out, bk.as<uint64_t>(), n, k, N, l, Bg_bit, nullptr);
  HIP_TRY(hipStreamSynchronize(nullptr));
  return rc;
}

// On-device generation of an UNFOLDED bootstrap key (new_bootstrap_key(.., unfolding > 1), src/bootstrap.c:23-48): per group of u key bits the 2^u
// torus-domain samples su[g 2^u + j] = TRGSW(1 if the group's bits spell j else 0), encrypted by the same kernel as the plain key (the message of entry e
// is one 0/1 word) and left in the torus domain, where the unfolded rotation wants them.  u = 8 at lvl2 is 20,224 samples = 5 GB: seconds here, minutes of
// schoolbook products on the host.
extern "C" int mosfhet_hip_bsk_unfolded_generate(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t *out, const uint64_t *h_s_rlwe, int N, const uint64_t *h_s_lwe, int n, int l,
                                                 int Bg_bit, double sigma, uint64_t seed, int unfolding) {
  if (!ctx || !out || !h_s_rlwe || !h_s_lwe || n < 1) return fail(MOSFHET_HIP_EINVAL, "bsk_unfolded_generate: bad argument");
  if (!ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "bsk_unfolded_generate: N = %d not supported (1024, 2048, 4096)", N);
  if ((unfolding != 2 && unfolding != 4 && unfolding != 8) || n % unfolding)
    return fail(MOSFHET_HIP_EINVAL, "bsk_unfolded_generate: unfolding must be 2, 4 or 8 with n divisible by it");
  if (l < 1 || Bg_bit < 1 || l * Bg_bit >= 64 || Bg_bit > 31) return fail(MOSFHET_HIP_EINVAL, "bsk_unfolded_generate: bad gadget");
  if (!trlwe_key_fits(h_s_rlwe, N)) return fail(MOSFHET_HIP_EINVAL, "bsk_unfolded_generate: TRLWE key coefficients must fit 16 bits");
  HIP_TRY(hipSetDevice(ctx->device));
  const int key_exp = 1 << unfolding;
  const size_t entries = (size_t)n / unfolding * key_exp;
  std::vector<uint64_t> msgs(entries);
  for (int g = 0; g < n / unfolding; g++)
    for (int j = 0; j < key_exp; j++) {
      uint64_t v = 1;
      for (int b = 0; b < unfolding; b++) v *= ((j >> b) & 1) ? h_s_lwe[g * unfolding + b] : 1 - h_s_lwe[g * unfolding + b];
      msgs[(size_t)g * key_exp + j] = v;
    }
  std::unique_ptr<mosfhet_hip_bsk> b_owner(new mosfhet_hip_bsk());
  mosfhet_hip_bsk *b = b_owner.get();
  b->ctx = ctx; b->device = ctx->device; b->d_bk = nullptr; b->n = n; b->k = 1; b->N = N; b->l = l; b->Bg_bit = Bg_bit; b->unfolding = unfolding;
  const size_t n_rows = entries * 2 * l;
  b->bytes = n_rows * 2 * N * sizeof(uint64_t);
  HIP_TRY(hipMalloc((void **)&b->d_su, b->bytes));
  DevBuf keys;
  HIP_TRY(keys.alloc(((size_t)N + entries) * sizeof(uint64_t)));
  uint64_t *d_keys = (uint64_t *)keys.p;
  HIP_TRY(hipMemcpy(d_keys, h_s_rlwe, (size_t)N * sizeof(uint64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_keys + N, msgs.data(), entries * sizeof(uint64_t), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(trgsw_bk_keygen_kernel, dim3((unsigned)n_rows), dim3(256), (size_t)N * sizeof(uint64_t) + (size_t)N * 2 * sizeof(uint16_t), nullptr, b->d_su, d_keys,
                     d_keys + N, N, l, Bg_bit, sigma, seed, 0, noise_key_for_call(NOISE_BSK_UNFOLDED));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  if (unfold2_capable(b) && unfold2_dft_enabled()) {   // the transformed samples of unfolding 2: now, not at the first bootstrap (unfold2_ready)
    const int rc2 = unfold2_ready(ctx, b);
    if (rc2) return rc2;
  }
  *out = b_owner.release();
  return MOSFHET_HIP_OK;
}

// On-device generation of a set of FFT-based TRLWE key-switch keys: entry e switches from the polynomial h_msgs[e] (the key being switched from,
// a Galois image of the key, -s, -s * s_in, s^2 ...) to s_out.  Encrypt in the torus domain, transform, hand out a gak handle.
extern "C" int mosfhet_hip_trlwe_ksk_generate(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t *out, const uint64_t *h_s_out, int N, const uint64_t *h_msgs, int entries, int t,
                                              int base_bit, double sigma, uint64_t seed) {
  if (!ctx || !out || !h_s_out || !h_msgs || entries < 1) return fail(MOSFHET_HIP_EINVAL, "trlwe_ksk_generate: bad argument");
  if (!ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "trlwe_ksk_generate: N = %d not supported (1024, 2048, 4096)", N);
  if (t < 1 || base_bit < 1 || t * base_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "trlwe_ksk_generate: bad t = %d base_bit = %d", t, base_bit);
  if (!trlwe_key_fits(h_s_out, N)) return fail(MOSFHET_HIP_EINVAL, "trlwe_ksk_generate: TRLWE key coefficients must fit 16 bits");
  HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<mosfhet_hip_gak> g_owner(new mosfhet_hip_gak());
  mosfhet_hip_gak *g = g_owner.get();
  g->ctx = ctx; g->device = ctx->device; g->N = N; g->t = t; g->base_bit = base_bit; g->entries = entries;
  const size_t n_rows = (size_t)entries * t, polys = n_rows * 2;
  g->bytes = polys * N * sizeof(double);
  DevBuf rows, keys;
  HIP_TRY(rows.alloc(g->bytes));
  HIP_TRY(keys.alloc(((size_t)N + (size_t)entries * N) * sizeof(uint64_t)));
  HIP_TRY(hipMalloc((void **)&g->d_ak, g->bytes));
  uint64_t *d_keys = keys.as<uint64_t>();
  HIP_TRY(hipMemcpy(d_keys, h_s_out, (size_t)N * sizeof(uint64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_keys + N, h_msgs, (size_t)entries * N * sizeof(uint64_t), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(trlwe_poly_keygen_kernel, dim3((unsigned)n_rows), dim3(256), (size_t)N * sizeof(uint64_t) + (size_t)N * 2 * sizeof(uint16_t), nullptr,
                     rows.as<uint64_t>(), d_keys, d_keys + N, N, t, base_bit, sigma, seed, noise_key_for_call(NOISE_TRLWE_KSK), ClientParams{});
  RING_DISPATCH(ctx, N, hipLaunchKernelGGL(torus_to_dft_kernel<F>, dim3((unsigned)polys), dim3(F::THREADS), 0, nullptr, rows.as<uint64_t>(), g->d_ak, TW));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  *out = g_owner.release();
  return MOSFHET_HIP_OK;
}

// On-device generation of the LWE -> LWE key-switch table (tlwe_new_KS_key, src/tlwe.c:193-212): rows TLWE_{s_out}(s_in[i] v 2^(64-(j+1)bb)).
// compressed != 0 keeps one word per row (b): the 1.2 GB table of lvl2 becomes 2 MB and tlwe_keyswitch regenerates every mask word it stages.
extern "C" int mosfhet_hip_tlwe_ksk_generate(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, const uint64_t *h_s_out, int n_out, const uint64_t *h_s_in, int n_in,
                                             int t, int base_bit, double sigma, uint64_t seed, int compressed) {
  if (!ctx || !out || !h_s_out || !h_s_in || n_out < 1 || n_in < 1 || t < 1 || base_bit < 1 || base_bit > 8 || t * base_bit >= 64)
    return fail(MOSFHET_HIP_EINVAL, "tlwe_ksk_generate: bad argument");
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n_rows = (size_t)n_in * t * ((1u << base_bit) - 1);
  std::unique_ptr<mosfhet_hip_ksk> k_owner(new mosfhet_hip_ksk());
  mosfhet_hip_ksk *k = k_owner.get();
  k->ctx = ctx; k->device = ctx->device; k->n_in = n_in; k->n_out = n_out; k->t = t; k->base_bit = base_bit;
  k->row = n_out + 1; k->b_word = n_out;
  k->compressed = compressed != 0; k->seed = seed;
  k->bytes = n_rows * (compressed ? 1 : (size_t)n_out + 1) * sizeof(uint64_t);
  DevBuf keys;
  HIP_TRY(hipMalloc((void **)&k->d_ksk, k->bytes + ksw_slack_bytes(k->row)));   // (+ slack: the word-lane key switch reads past the last row, keyswitch_words_kernels.h)
  HIP_TRY(keys.alloc(((size_t)n_out + n_in) * sizeof(uint64_t)));
  uint64_t *d_keys = keys.as<uint64_t>();
  HIP_TRY(hipMemcpy(d_keys, h_s_out, (size_t)n_out * sizeof(uint64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_keys + n_out, h_s_in, (size_t)n_in * sizeof(uint64_t), hipMemcpyHostToDevice));
  const NoiseKey nkey = noise_key_for_call(NOISE_TLWE_KSK);
  for (size_t first = 0; first < n_rows; first += 1u << 20) {
    const size_t chunk = n_rows - first < (1u << 20) ? n_rows - first : (1u << 20);
    hipLaunchKernelGGL(tlwe_ksk_keygen_kernel, dim3((unsigned)chunk), dim3(64), 0, nullptr, k->d_ksk, d_keys, d_keys + n_out, n_out, t, base_bit, sigma, seed, first,
                       compressed, nkey, ClientParams{});
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  *out = k_owner.release();
  return MOSFHET_HIP_OK;
}

// copy `count` rows of a table key back to the host (verification of generated keys, key files); compressed keys are expanded on the way
extern "C" int mosfhet_hip_ksk_export_rows(mosfhet_hip_ksk_t ksk, size_t first_row, size_t count, uint64_t *h_out) {
  if (!ksk || !h_out) return fail(MOSFHET_HIP_EINVAL, "ksk_export_rows: bad argument");
  const size_t row_bytes = (size_t)ksk->row * sizeof(uint64_t);
  if (ksk->compressed) {
    const int mask_words = ksk->b_word == ksk->row - 1 ? ksk->row - 1 : ksk->row / 2;     // LWE rows keep one b word, TRLWE rows their b polynomial
    if ((first_row + count) * (size_t)(ksk->row - mask_words) * sizeof(uint64_t) > ksk->bytes) return fail(MOSFHET_HIP_EINVAL, "ksk_export_rows: out of range");
    if (count == 0) return MOSFHET_HIP_OK;
    HIP_TRY(hipSetDevice(ksk->device));
    uint64_t *tmp = nullptr;
    HIP_TRY(hipMalloc((void **)&tmp, count * row_bytes));
    hipLaunchKernelGGL(table_expand_kernel, dim3((unsigned)count), dim3(256), 0, nullptr, tmp, ksk->d_ksk, ksk->row, mask_words, ksk->seed, first_row);
    hipError_t e = hipMemcpy(h_out, tmp, count * row_bytes, hipMemcpyDeviceToHost);
    hipFree(tmp);
    if (e != hipSuccess) return fail(MOSFHET_HIP_EHIP, "ksk_export_rows: %s", hipGetErrorString(e));
    return MOSFHET_HIP_OK;
  }
  if ((first_row + count) * row_bytes > ksk->bytes) return fail(MOSFHET_HIP_EINVAL, "ksk_export_rows: out of range");
  HIP_TRY(hipSetDevice(ksk->device));
  HIP_TRY(hipMemcpy(h_out, (const char *)ksk->d_ksk + first_row * row_bytes, count * row_bytes, hipMemcpyDeviceToHost));
  return MOSFHET_HIP_OK;
}

// ---- the canonical caller pattern: key switch N -> n, then bootstrap (applications/multi-ciphertext-arith/src/integer.c:94-95) ----
// d_in: [count][kN+1] ciphertexts under the extracted key; the switched ciphertexts live in the handle's scratch, one stream, no host sync.
extern "C" int mosfhet_hip_keyswitch_functional_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, mosfhet_hip_bsk_t bsk, uint64_t *d_out,
                                                                const uint64_t *d_tv, int tv_count, const uint64_t *d_in, int count, int torus_base, int extract,
                                                                void *stream) {
  if (!ctx || !ksk || !bsk || count < 0) return fail(MOSFHET_HIP_EINVAL, "keyswitch_bootstrap: bad argument");
  if (int rk = ks_bootstrap_keys_match("keyswitch_bootstrap", ksk, bsk)) return rk;
  if (count == 0) return MOSFHET_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  uint64_t *tmp = nullptr;
  int rc = ext_scratch(bsk, 1, (size_t)count * (bsk->n + 1), &tmp);
  if (rc) return rc;
  if ((rc = mosfhet_hip_tlwe_keyswitch_batch(ctx, ksk, tmp, d_in, count, stream))) return rc;
  return extract ? mosfhet_hip_functional_bootstrap_batch(ctx, bsk, d_out, d_tv, tv_count, tmp, count, torus_base, stream)
                 : mosfhet_hip_functional_bootstrap_wo_extract_batch(ctx, bsk, d_out, d_tv, tv_count, tmp, count, torus_base, stream);
}

// ---- CMUX over a batch with one shared selector (key entry `key_index` of a key handle, e.g. one made from circuit-bootstrapped TRGSW
// samples by mosfhet_hip_bsk_create_from_device): out[b] = in0[b] + key (.) (in1[b] - in0[b]).  d_out may alias d_in0.
// (CMUX of applications/leveled_lut/vertical_packing.c:24-33 = trlwe_sub + trgsw_mul_trlwe_DFT + trlwe_from_DFT + trlwe_add, fused.)
extern "C" int mosfhet_hip_cmux_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, int key_index, uint64_t *d_out, const uint64_t *d_in0, const uint64_t *d_in1,
                                      int count, void *stream) {
  if (!ctx || !bsk || count < 0 || key_index < 0 || key_index >= bsk->n) return fail(MOSFHET_HIP_EINVAL, "cmux: bad argument");
  if (bsk->unfolding > 1) return fail(MOSFHET_HIP_EINVAL, "cmux: an unfolded key has no DFT entries");
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_in0 || !d_in1) return fail(MOSFHET_HIP_EINVAL, "cmux: null buffer");
  HIP_TRY(hipSetDevice(ctx->device));
  if (bsk->general) return external_product_general(ctx, bsk, key_index, d_out, d_in1, d_in0, count, stream);
  const d2 *row = bsk->d_bk + (size_t)key_index * (2 * bsk->l * 2 * (bsk->N / 2));
  hipStream_t s = pick(ctx, stream);
  int rc = MOSFHET_HIP_OK;
  RING_DISPATCH(ctx, bsk->N, rc = launch_external_product<F>(bsk->l, bsk->Bg_bit, s, row, TW, d_in1, d_out, count, (size_t)0, (size_t)2 * F::N, d_in0, nullptr, bsk->owns));
  return rc;
}

// ---- key images for the on-disk formats (SURVEY 8(f).2; save_bootstrap_key / load_new_bootstrap_key src/bootstrap.c:63-104,
// trlwe_save_KS_key / trlwe_load_new_KS_key src/keyswitch.c:122-160, trlwe_save_generic_ks_key / _load_ :409-455) ----
// DFT-domain contents are backend-defined in the reference as well (element order depends on the FFT library, src/polynomial.c:336-357): an image is
// the engine's own layout, stamped with mosfhet_hip_dft_layout_id() by the callers that write files.  Images are exact: a key that went through
// export -> import produces bit-identical results.
extern "C" unsigned mosfhet_hip_dft_layout_id(void) { return 0x4D414631u; }  // "MAF1": [poly][8 or 16 values per thread][threads] slot order of negacyclic_fft.h

extern "C" int mosfhet_hip_bsk_info(mosfhet_hip_bsk_t bsk, int *out6) {
  if (!bsk || !out6) return fail(MOSFHET_HIP_EINVAL, "bsk_info: bad argument");
  out6[0] = bsk->n; out6[1] = bsk->k; out6[2] = bsk->N; out6[3] = bsk->l; out6[4] = bsk->Bg_bit; out6[5] = bsk->unfolding;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_bsk_export(mosfhet_hip_bsk_t bsk, void *h_out) {
  if (!bsk || !h_out) return fail(MOSFHET_HIP_EINVAL, "bsk_export: bad argument");
  HIP_TRY(hipSetDevice(bsk->device));
  HIP_TRY(hipMemcpy(h_out, bsk->unfolding > 1 ? (const void *)bsk->d_su : (const void *)bsk->d_bk, bsk->bytes, hipMemcpyDeviceToHost));
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_bsk_import(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t *out, const void *h_image, int n, int k, int N, int l, int Bg_bit, int unfolding) {
  if (!ctx || !out || !h_image || n < 1) return fail(MOSFHET_HIP_EINVAL, "bsk_import: bad argument");
  if (unfolding > 1) {
    if (k != 1) return fail(MOSFHET_HIP_EINVAL, "bsk_import: unfolded keys have k = 1");
    return mosfhet_hip_bsk_unfolded_create(ctx, out, (const uint64_t *)h_image, n, N, l, Bg_bit, unfolding);
  }
  int rc = check_params("bsk_import", k, N, l, Bg_bit, true);   // general rings too: their images are the natural slot order of general_kernels.h, copied as they are
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<mosfhet_hip_bsk> b_owner(new mosfhet_hip_bsk());
  mosfhet_hip_bsk *b = b_owner.get();
  b->ctx = ctx; b->device = ctx->device; b->n = n; b->k = k; b->N = N; b->l = l; b->Bg_bit = Bg_bit;
  b->general = general_ring(k, N);
  b->bytes = (size_t)n * (k + 1) * l * (k + 1) * N * sizeof(double);
  hipError_t e = hipMalloc((void **)&b->d_bk, b->bytes);
  if (e == hipSuccess) e = hipMemcpy(b->d_bk, h_image, b->bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(MOSFHET_HIP_EHIP, "bsk_import: %s", hipGetErrorString(e));
  *out = b_owner.release();
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_trlwe_ksk_info(mosfhet_hip_gak_t tks, int *out4) {
  if (!tks || !out4) return fail(MOSFHET_HIP_EINVAL, "trlwe_ksk_info: bad argument");
  out4[0] = tks->entries; out4[1] = tks->N; out4[2] = tks->t; out4[3] = tks->base_bit;
  return MOSFHET_HIP_OK;
}

extern "C" size_t mosfhet_hip_trlwe_ksk_bytes(mosfhet_hip_gak_t tks) { return tks ? tks->bytes : 0; }

extern "C" int mosfhet_hip_trlwe_ksk_export(mosfhet_hip_gak_t tks, void *h_out) {
  if (!tks || !h_out) return fail(MOSFHET_HIP_EINVAL, "trlwe_ksk_export: bad argument");
  HIP_TRY(hipSetDevice(tks->device));
  HIP_TRY(hipMemcpy(h_out, tks->d_ak, tks->bytes, hipMemcpyDeviceToHost));
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_trlwe_ksk_import(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t *out, const void *h_image, int entries, int N, int t, int base_bit) {
  if (!ctx || !out || !h_image || entries < 1) return fail(MOSFHET_HIP_EINVAL, "trlwe_ksk_import: bad argument");
  if (!ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "trlwe_ksk_import: N = %d not supported (1024, 2048, 4096)", N);
  if (t < 1 || base_bit < 1 || t * base_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "trlwe_ksk_import: bad t = %d base_bit = %d", t, base_bit);
  HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<mosfhet_hip_gak> g_owner(new mosfhet_hip_gak());
  mosfhet_hip_gak *g = g_owner.get();
  g->ctx = ctx; g->device = ctx->device; g->N = N; g->t = t; g->base_bit = base_bit; g->entries = entries;
  g->bytes = (size_t)entries * t * 2 * N * sizeof(double);
  hipError_t e = hipMalloc((void **)&g->d_ak, g->bytes);
  if (e == hipSuccess) e = hipMemcpy(g->d_ak, h_image, g->bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(MOSFHET_HIP_EHIP, "trlwe_ksk_import: %s", hipGetErrorString(e));
  *out = g_owner.release();
  return MOSFHET_HIP_OK;
}

// table keys (LWE -> LWE, packing, private): the device table IS the reference's uncompressed row order [n_in][t][2^bb - 1][row], so files are
// streamed row-wise: ksk_info, ksk_export_rows on the way out; ksk_alloc (kind 0 LWE -> LWE with n_out, 1 packing, 2 private with N) and
// ksk_import_rows on the way in.
extern "C" int mosfhet_hip_ksk_info(mosfhet_hip_ksk_t ksk, int *out6) {
  if (!ksk || !out6) return fail(MOSFHET_HIP_EINVAL, "ksk_info: bad argument");
  out6[0] = ksk->n_in; out6[1] = ksk->row; out6[2] = ksk->b_word; out6[3] = ksk->t; out6[4] = ksk->base_bit;
  out6[5] = ksk->b_word == ksk->n_out ? 0 : (ksk->b_word < 0 ? 2 : 1);
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_ksk_alloc(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t *out, int kind, int n, int n_out_or_N, int t, int base_bit) {
  if (!ctx || !out || kind < 0 || kind > 2 || n < 1 || n_out_or_N < 1 || t < 1 || base_bit < 1 || base_bit > 8 || t * base_bit >= 64)
    return fail(MOSFHET_HIP_EINVAL, "ksk_alloc: bad argument");
  HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<mosfhet_hip_ksk> k_owner(new mosfhet_hip_ksk());
  mosfhet_hip_ksk *k = k_owner.get();
  k->ctx = ctx; k->device = ctx->device; k->t = t; k->base_bit = base_bit;
  k->n_in = n + (kind == 2);
  k->n_out = kind == 0 ? n_out_or_N : 2 * n_out_or_N - 1;
  k->row = k->n_out + 1;
  k->b_word = kind == 0 ? k->n_out : (kind == 1 ? n_out_or_N : -1);
  k->bytes = (size_t)k->n_in * t * ((1u << base_bit) - 1) * k->row * sizeof(uint64_t);
  hipError_t e = hipMalloc((void **)&k->d_ksk, k->bytes + ksw_slack_bytes(k->row));   // (+ slack: keyswitch_words_kernels.h)
  if (e != hipSuccess) return fail(MOSFHET_HIP_EHIP, "ksk_alloc: %s", hipGetErrorString(e));
  *out = k_owner.release();
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_ksk_import_rows(mosfhet_hip_ksk_t ksk, size_t first_row, size_t count, const uint64_t *h_in) {
  if (!ksk || !h_in) return fail(MOSFHET_HIP_EINVAL, "ksk_import_rows: bad argument");
  if (ksk->compressed) return fail(MOSFHET_HIP_EINVAL, "ksk_import_rows: a seed-compressed key has no mask rows to import");
  const size_t row_bytes = (size_t)ksk->row * sizeof(uint64_t);
  if ((first_row + count) * row_bytes > ksk->bytes) return fail(MOSFHET_HIP_EINVAL, "ksk_import_rows: out of range");
  HIP_TRY(hipSetDevice(ksk->device));
  HIP_TRY(hipMemcpy((char *)ksk->d_ksk + first_row * row_bytes, h_in, count * row_bytes, hipMemcpyHostToDevice));
  return MOSFHET_HIP_OK;
}

// ---- key replication, device to device (SURVEY.md 8(e)) ----
static thread_local int t_clone_route = 0;
extern "C" int mosfhet_hip_last_clone_route(void) { return t_clone_route; }
extern "C" size_t mosfhet_hip_gak_bytes(mosfhet_hip_gak_t gak) { return gak ? gak->bytes : 0; }

// dst (on dst_dev, which is the current device) <- src (on src_dev)
static int copy_across(void *dst, int dst_dev, const void *src, int src_dev, size_t bytes) {
  if (bytes == 0) return MOSFHET_HIP_OK;
  const char *no_peer = getenv("MOSFHET_HIP_NO_PEER");   // test switch: 1 = skip peer access, 2 = skip every device-to-device copy (host bounce, same device included)
  const int skip = no_peer ? atoi(no_peer) : 0;
  if (dst_dev == src_dev && skip < 2) {
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice));
    HIP_TRY(hipDeviceSynchronize());   // (a device-to-device copy returns before it has run; the replica is used from other streams)
    t_clone_route = 0;
    return MOSFHET_HIP_OK;
  }
  int can = 0;
  if (skip < 1 && dst_dev != src_dev && hipDeviceCanAccessPeer(&can, dst_dev, src_dev) == hipSuccess && can) {
    const hipError_t e = hipDeviceEnablePeerAccess(src_dev, 0);   // current device = dst_dev
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) can = 0;
    (void)hipGetLastError();
  } else {
    can = 0;
  }
  if (skip < 2) {
    const hipError_t e = hipMemcpyPeer(dst, dst_dev, src, src_dev, bytes);
    if (e == hipSuccess) {
      HIP_TRY(hipDeviceSynchronize());
      t_clone_route = can ? 1 : 2;
      return MOSFHET_HIP_OK;
    }
    (void)hipGetLastError();
  }
  // last resort: a pinned bounce buffer, 64 MiB at a time
  const size_t chunk = (size_t)64 << 20;
  void *h = nullptr;
  HIP_TRY(hipHostMalloc(&h, bytes < chunk ? bytes : chunk, 0));
  hipError_t e = hipSuccess;
  for (size_t off = 0; off < bytes && e == hipSuccess; off += chunk) {
    const size_t c = bytes - off < chunk ? bytes - off : chunk;
    if ((e = hipSetDevice(src_dev)) != hipSuccess) break;
    if ((e = hipMemcpy(h, (const char *)src + off, c, hipMemcpyDeviceToHost)) != hipSuccess) break;
    if ((e = hipSetDevice(dst_dev)) != hipSuccess) break;
    e = hipMemcpy((char *)dst + off, h, c, hipMemcpyHostToDevice);
  }
  (void)hipSetDevice(dst_dev);
  (void)hipHostFree(h);
  if (e != hipSuccess) return fail(MOSFHET_HIP_EHIP, "key replication: %s", hipGetErrorString(e));
  t_clone_route = 3;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_bsk_clone(mosfhet_hip_ctx_t dst_ctx, mosfhet_hip_bsk_t *out, mosfhet_hip_bsk_t src) {
  if (!dst_ctx || !out || !src) return fail(MOSFHET_HIP_EINVAL, "bsk_clone: bad argument");
  if (!src->owns) return fail(MOSFHET_HIP_EINVAL, "bsk_clone: a key view does not own its entries");
  HIP_TRY(hipSetDevice(src->device));
  HIP_TRY(hipDeviceSynchronize());   // the key may still be in the making on a stream of its own device
  HIP_TRY(hipSetDevice(dst_ctx->device));
  std::unique_ptr<mosfhet_hip_bsk> b_owner(new mosfhet_hip_bsk());
  mosfhet_hip_bsk *b = b_owner.get();
  b->ctx = dst_ctx; b->device = dst_ctx->device; b->n = src->n; b->k = src->k; b->N = src->N; b->l = src->l; b->Bg_bit = src->Bg_bit;
  b->unfolding = src->unfolding; b->bytes = src->bytes; b->general = src->general;
  b->order = src->order;   // replicas sum alike (mosfhet_hip_bsk_set_product_order)
  int rc;
  if (src->unfolding > 1) {
    HIP_TRY(hipMalloc((void **)&b->d_su, b->bytes));
    if ((rc = copy_across(b->d_su, dst_ctx->device, src->d_su, src->device, b->bytes))) return rc;
    if (unfold2_capable(b) && unfold2_dft_enabled() && (rc = unfold2_ready(dst_ctx, b))) return rc;   // the replica transforms its own samples, now
  } else {
    HIP_TRY(hipMalloc((void **)&b->d_bk, b->bytes));
    if ((rc = copy_across(b->d_bk, dst_ctx->device, src->d_bk, src->device, b->bytes))) return rc;
  }
  *out = b_owner.release();
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_ksk_clone(mosfhet_hip_ctx_t dst_ctx, mosfhet_hip_ksk_t *out, mosfhet_hip_ksk_t src) {
  if (!dst_ctx || !out || !src) return fail(MOSFHET_HIP_EINVAL, "ksk_clone: bad argument");
  HIP_TRY(hipSetDevice(src->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipSetDevice(dst_ctx->device));
  std::unique_ptr<mosfhet_hip_ksk> k_owner(new mosfhet_hip_ksk());
  mosfhet_hip_ksk *k = k_owner.get();
  k->ctx = dst_ctx; k->device = dst_ctx->device; k->n_in = src->n_in; k->n_out = src->n_out; k->t = src->t; k->base_bit = src->base_bit; k->row = src->row; k->b_word = src->b_word;
  k->compressed = src->compressed; k->seed = src->seed; k->bytes = src->bytes;
  HIP_TRY(hipMalloc((void **)&k->d_ksk, k->bytes + ksw_slack_bytes(k->row)));   // (+ slack: the word-lane key switch reads past the last row, keyswitch_words_kernels.h)
  const int rc = copy_across(k->d_ksk, dst_ctx->device, src->d_ksk, src->device, k->bytes);
  if (rc) return rc;
  *out = k_owner.release();
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_gak_clone(mosfhet_hip_ctx_t dst_ctx, mosfhet_hip_gak_t *out, mosfhet_hip_gak_t src) {
  if (!dst_ctx || !out || !src) return fail(MOSFHET_HIP_EINVAL, "gak_clone: bad argument");
  HIP_TRY(hipSetDevice(src->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipSetDevice(dst_ctx->device));
  std::unique_ptr<mosfhet_hip_gak> g_owner(new mosfhet_hip_gak());
  mosfhet_hip_gak *g = g_owner.get();
  g->ctx = dst_ctx; g->device = dst_ctx->device; g->N = src->N; g->t = src->t; g->base_bit = src->base_bit; g->entries = src->entries; g->bytes = src->bytes;
  HIP_TRY(hipMalloc((void **)&g->d_ak, g->bytes));
  const int rc = copy_across(g->d_ak, dst_ctx->device, src->d_ak, src->device, g->bytes);
  if (rc) return rc;
  *out = g_owner.release();
  return MOSFHET_HIP_OK;
}
