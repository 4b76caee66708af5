// capi_dft.inc -- C-ABI entry points behind the reference's DFT-level functions (include/mosfhet.h:179-182,263-264,342-344,454,296 of the
// reference): the legacy signatures pass TRGSW_DFT / TRLWE_DFT / DFT_Polynomial objects around, which this engine keeps device resident in its own
// slot order (negacyclic_fft.h).  The host layer (csrc/host/mosfhet_compat_dft.c) hands their device pointers to the calls below.
// Included at the end of capi.hip.

// A non-owning key handle over `n` consecutive TRGSW_DFT entries already in device memory in the engine's layout ([entry][(k+1)l][k+1][N/2] complex,
// slot order: what torus_to_dft_batch writes for the entries' polynomials in that order).  Lets blind_rotate(tv, a, TRGSW_DFT *s, size) and the CMUX of
// applications/leveled_lut/vertical_packing.c run on selectors the caller transformed with trgsw_to_DFT.  Destroy with mosfhet_hip_bsk_destroy.
extern "C" int mosfhet_hip_bsk_view_create(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t *out, const double *d_dft, int n, int k, int N, int l, int Bg_bit) {
  if (!ctx || !out || !d_dft || n < 1) return fail(MOSFHET_HIP_EINVAL, "bsk_view_create: bad argument");
  int rc = check_params("bsk_view_create", k, N, l, Bg_bit);
  if (rc) return rc;
  std::unique_ptr<mosfhet_hip_bsk> b(new mosfhet_hip_bsk());
  b->ctx = ctx; b->device = ctx->device; b->n = n; b->k = k; b->N = N; b->l = l; b->Bg_bit = Bg_bit;
  b->d_bk = (d2 *)d_dft;
  b->owns = false;
  b->bytes = (size_t)n * (k + 1) * l * (k + 1) * N * sizeof(double);
  *out = b.release();
  return MOSFHET_HIP_OK;
}

// device address of a key's DFT entries (NULL for an unfolded key): entry i starts at + i * (k+1) l (k+1) N doubles
extern "C" const double *mosfhet_hip_bsk_device_dft(mosfhet_hip_bsk_t bsk) { return bsk ? (const double *)bsk->d_bk : nullptr; }

// trgsw_mul_trlwe_DFT (src/trgsw.c:385-423) with the result LEFT in the DFT domain, as the reference declares it:
// d_out_dft[b] ([k+1][N/2] complex) = sum over rows of DFT(digit_j(d_in[b].p)) (.) d_trgsw_dft rows.  key_stride (doubles): 0 = one TRGSW for the batch.
extern "C" int mosfhet_hip_external_product_dft_batch(mosfhet_hip_ctx_t ctx, const double *d_trgsw_dft, size_t key_stride, double *d_out_dft,
                                                      const uint64_t *d_in, int N, int l, int Bg_bit, int count, void *stream) {
  if (!ctx || count < 0) return fail(MOSFHET_HIP_EINVAL, "external_product_dft: bad argument");
  int rc = check_params("external_product_dft", 1, N, l, Bg_bit);
  if (rc) return rc;
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_trgsw_dft || !d_out_dft || !d_in) return fail(MOSFHET_HIP_EINVAL, "external_product_dft: null buffer");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  const d2 *row = (const d2 *)d_trgsw_dft;
  RING_DISPATCH(ctx, N, launch_external_product<F>(l, Bg_bit, s, row, TW, d_in, (uint64_t *)nullptr, count, key_stride / 2, (size_t)2 * F::N, nullptr, (d2 *)d_out_dft, false));
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// public_mux with the selector in the DFT domain, the reference's signature (src/bootstrap.c:369-389: TRLWE_DFT *selector): d_sel_dft [count][l][2][N/2] complex
extern "C" int mosfhet_hip_public_mux_dft_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const uint64_t *d_p0, const uint64_t *d_p1, const double *d_sel_dft, int N,
                                                int l, int Bg_bit, int count, void *stream) {
  if (!ctx || count < 0 || l < 1 || l * Bg_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "public_mux_dft: bad argument");
  if (!ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "public_mux_dft: N = %d not supported (1024, 2048, 4096)", N);
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_p0 || !d_p1 || !d_sel_dft) return fail(MOSFHET_HIP_EINVAL, "public_mux_dft: null buffer");
  HIP_TRY(hipSetDevice(ctx->device));
  uint64_t *tmp = nullptr;
  int rc = ctx_scratch(ctx, 2, (size_t)2 * l * N, &tmp);
  if (rc) return rc;
  hipStream_t s = pick(ctx, stream);
  d2 *pdec = (d2 *)(tmp + (size_t)l * N);
  hipLaunchKernelGGL(public_mux_digits_kernel, dim3((N + 255) / 256), dim3(256), 0, s, d_p0, d_p1, tmp, N, l, Bg_bit);
  RING_DISPATCH(ctx, N, {
    hipLaunchKernelGGL(torus_to_dft_kernel<F>, dim3(l), dim3(F::THREADS), 0, s, tmp, pdec, TW);
    hipLaunchKernelGGL(public_mux_kernel<F>, dim3(count), dim3(F::THREADS), 0, s, (const uint64_t *)nullptr, (size_t)0, pdec, d_p0, TW, d_out, (size_t)2 * N, l,
                       (const d2 *)d_sel_dft);
  });
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// blind_rotate_ga (src/bootstrap_ga.c:35-60) on caller-supplied accumulators: d_acc [count][2][N] in place, d_in [count][n+1] (only the n mask words are read)
extern "C" int mosfhet_hip_blind_rotate_ga_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_gak_t gak, uint64_t *d_acc, const uint64_t *d_in, int count,
                                                 void *stream) {
  TUNED_ONLY(bsk, "blind_rotate_ga");
  if (!ctx || !bsk || !gak || count < 0) return fail(MOSFHET_HIP_EINVAL, "blind_rotate_ga: bad argument");
  if (bsk->unfolding > 1) return fail(MOSFHET_HIP_EINVAL, "blind_rotate_ga: needs a key without unfolding");
  if (gak->N != bsk->N || gak->t != bsk->l || gak->base_bit != bsk->Bg_bit)
    return fail(MOSFHET_HIP_EINVAL, "blind_rotate_ga: automorphism keys must use the bootstrap key's N, l, Bg_bit");
  // the generators come from the mask words and reach 2N - 1: entry N - 1
  if (gak->entries < gak->N)
    return fail(MOSFHET_HIP_EINVAL, "blind_rotate_ga: needs the full automorphism key set, entries = %d < N = %d", gak->entries, gak->N);
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_acc || !d_in) return fail(MOSFHET_HIP_EINVAL, "blind_rotate_ga: null buffer");
  HIP_TRY(hipSetDevice(ctx->device));
  GaParams g;
  memset(&g, 0, sizeof(g));
  g.p.bk = bsk->d_bk;
  g.p.tw = bsk->N == 1024 ? ctx->tw1024 : (bsk->N == 2048 ? ctx->tw2048 : ctx->tw4096);
  g.p.in = d_in;
  g.p.out = d_acc;
  g.p.n = bsk->n;
  g.p.Bg_bit = bsk->Bg_bit;
  g.p.skip_init = 1;
  g.p.extract = 0;
  g.ak = gak->d_ak;
  g.mode = 0;
  g.entry = -1;
  int rc_ga = MOSFHET_HIP_OK;
  RING_DISPATCH(ctx, bsk->N, rc_ga = launch_ga_f<F>(bsk->l, bsk->Bg_bit, g, count, pick(ctx, stream), bsk->order));
  return rc_ga;
}

// trlwe_eval_automorphism (src/trlwe.c:775-781) with the key the CALLER names (entry of a key set) instead of entry (gen - 1) / 2
extern "C" int mosfhet_hip_trlwe_eval_automorphism_entry_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t gak, int entry, uint64_t *d_out, const uint64_t *d_in, int gen,
                                                               int count, void *stream) {
  if (!ctx || !gak || count < 0 || entry < 0 || entry >= gak->entries) return fail(MOSFHET_HIP_EINVAL, "eval_automorphism: bad argument");
  if (gen < 1 || gen >= 2 * gak->N || !(gen & 1)) return fail(MOSFHET_HIP_EINVAL, "eval_automorphism: generator %d must be odd and < 2N", gen);
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_in) return fail(MOSFHET_HIP_EINVAL, "eval_automorphism: null buffer");
  HIP_TRY(hipSetDevice(ctx->device));
  GaParams g;
  memset(&g, 0, sizeof(g));
  g.p.tw = gak->N == 1024 ? ctx->tw1024 : (gak->N == 2048 ? ctx->tw2048 : ctx->tw4096);
  g.p.in = d_in;
  g.p.out = d_out;
  g.p.Bg_bit = gak->base_bit;
  g.ak = gak->d_ak;
  g.mode = 1;
  g.gen = gen;
  g.entry = entry;
  int rc_ga = MOSFHET_HIP_OK;
  RING_DISPATCH(ctx, gak->N, rc_ga = launch_ga_f<F>(gak->t, gak->base_bit, g, count, pick(ctx, stream), MOSFHET_HIP_ORDER_AUTO));   // (mode 1: no external product)
  return rc_ga;
}

// polynomial_add_DFT_polynomials / _sub_ / _scale_and_add_ (src/polynomial.c:102-128) and their TRLWE_DFT / TRGSW_DFT callers (src/trlwe.c, src/trgsw.c:
// trlwe_DFT_add / _sub / _addto, trgsw_DFT_add / _sub) over flat device arrays: d_out[i] = (d_a ? d_a[i] : 0) + cb * d_b[i], one fma per element
// (cb = 1 / -1: plain add / subtract); d_out may alias either input.  Linear and elementwise, so the slot order does not matter.
namespace mosfhet {
__global__ void dft_lincomb_kernel(double *out, const double *a, const double *b, double cb, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = __builtin_fma(cb, b[i], a ? a[i] : 0.0);
}
}  // namespace mosfhet

extern "C" int mosfhet_hip_dft_lincomb_batch(mosfhet_hip_ctx_t ctx, double *d_out, const double *d_a, const double *d_b, double cb, size_t n_doubles, void *stream) {
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "dft_lincomb: null ctx");
  if (n_doubles == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_b) return fail(MOSFHET_HIP_EINVAL, "dft_lincomb: null buffer");
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t blocks = (n_doubles + 255) / 256;
  hipLaunchKernelGGL(mosfhet::dft_lincomb_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, pick(ctx, stream), d_out, d_a, d_b, cb, n_doubles);
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}
