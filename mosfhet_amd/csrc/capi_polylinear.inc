// capi_polylinear.inc -- cleartext polynomial-weight linear layers on batches of packed TRLWE samples: the reference's trlwe_to_DFT, trlwe_DFT_mul_by_polynomial /
// trlwe_DFT_mul_addto_by_polynomial (src/trlwe.c:491-505), trlwe_from_DFT and trlwe_extract_tlwe (:540-552) as ONE call over a batch, dense and sparse (CSR over
// polynomial blocks), alone or in front of key switch + bootstrap.  Own code: nothing of the reference is compiled in.  Kernel: polylinear_body, trace_kernels.h.
//
//   acc_a = acc_b = +0.0;  for e in row j's entries, in the stored order:  acc_c = mul_addto(acc_c, F(in[b][col_e].c), F(val_e))
//   out[b][j] = (G(acc_a), G(acc_b) + bias[j])          F = polynomial_torus_to_DFT, G = polynomial_DFT_to_torus with the general rounding, k = 1
//
// The handle holds the weight polynomials TRANSFORMED (torus_to_dft_kernel at creation, slot order), the lists and the bias in one device image, read-only after
// creation.  A call is two launches per round: torus_to_dft_kernel over the round's inputs into the calling thread's pool (slot POOL_POLYLINEAR, [round][rows_in][2][N/2]
// complex: every transform is made once and read by all rows_out teams), then trace_conversions_kernel kind 4, one team per (batch element, output row).  The pool is
// bounded by mosfhet_hip_set_tlwe_pack_workspace; a larger batch runs in rounds of whole batch elements, which changes no word.  The handle's image and clone, the plan,
// the checks of the compute calls and the loop over rounds are the packed families' shared ones: capi_linear_common.inc.
struct mosfhet_hip_polylinear : PackedLinear {};   // l = Bg_bit = 0; form: PLIN_DENSE or PLIN_SPARSE
static const PackedFamily POLYLINEAR = {false, 2, POOL_POLYLINEAR, "weight polynomials", "transformed inputs", "mosfhet_hip_polylinear_clone"};

extern "C" int mosfhet_hip_trlwe_linear_plan(int N, int rows_out, int rows_in, long long nnz, int count, int extract, int cus, long long workspace_bytes, long long plan[8]) {
  return packed_linear_plan_out("trlwe_linear_plan", POLYLINEAR, N, 0, rows_out, rows_in, nnz, count, extract, cus, workspace_bytes, plan);
}

// Every check of the two creation calls that needs no device, then the image: lists and bias uploaded, the weights uploaded as torus words and transformed in place of
// their slot by the forward-transform launcher every key of this library goes through.
static int polylinear_create(const char *who, mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t *out, const int *h_row_ptr, const int *h_col, const int64_t *h_val,
                             const uint64_t *h_bias, int rows_out, int rows_in, int N, bool sparse) {
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!out) return fail(MOSFHET_HIP_EINVAL, "%s: null out", who);
  if (rows_out < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_out = %d", who, rows_out);
  if (rows_in < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_in = %d", who, rows_in);
  if (!ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (1024, 2048, 4096)", who, N);
  std::vector<int> ptr, col;
  const char *missing = nullptr;   // what packed_linear_lists refuses where there are entries: sparse, "null h_col or h_val"; dense, "null h_W"
  if (sparse ? !h_col || !h_val : !h_val) missing = sparse ? "h_col or h_val" : "h_W";
  int rc = packed_linear_lists(who, POLYLINEAR, sparse, h_row_ptr, h_col, missing, rows_out, rows_in, ptr, col);
  if (rc) return rc;
  const long long entries = (long long)col.size();
  std::unique_ptr<mosfhet_hip_polylinear> h(new mosfhet_hip_polylinear());
  h->rows_out = rows_out; h->rows_in = rows_in; h->N = N; h->form = sparse; h->has_bias = h_bias != nullptr;
  h->nnz = sparse ? entries : -1; h->entries = entries;
  const size_t weight_bytes = (size_t)entries * N * sizeof(double);
  if ((rc = packed_linear_image(h.get(), ctx, weight_bytes, h_bias, ptr, col))) return rc;
  if (entries) {
    DevBuf words;   // (double)(int64_t): a weight is converted exactly as a torus word is
    HIP_TRY(words.alloc(weight_bytes));
    HIP_TRY(hipMemcpy(words.p, h_val, weight_bytes, hipMemcpyHostToDevice));
    RING_DISPATCH(ctx, N, hipLaunchKernelGGL(torus_to_dft_kernel<F>, dim3((unsigned)entries), dim3(F::THREADS), 0, nullptr, words.p, (void *)(h->d + h->off[PLIN_W]), TW));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
  }
  *out = h.release();
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_polylinear_create_dense(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t *out, const int64_t *h_W, const uint64_t *h_bias, int rows_out, int rows_in,
                                                   int N) {
  return polylinear_create("polylinear_create_dense", ctx, out, nullptr, nullptr, h_W, h_bias, rows_out, rows_in, N, false);
}

extern "C" int mosfhet_hip_polylinear_create_sparse(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t *out, const int *h_row_ptr, const int *h_col, const int64_t *h_val,
                                                    const uint64_t *h_bias, int rows_out, int rows_in, int N) {
  return polylinear_create("polylinear_create_sparse", ctx, out, h_row_ptr, h_col, h_val, h_bias, rows_out, rows_in, N, true);
}

extern "C" int mosfhet_hip_polylinear_destroy(mosfhet_hip_polylinear_t lin) {
  delete lin;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_polylinear_info(mosfhet_hip_polylinear_t lin, long long info[6]) {
  if (!lin || !info) return fail(MOSFHET_HIP_EINVAL, "polylinear_info: null %s", lin ? "info" : "lin");
  info[0] = lin->rows_out; info[1] = lin->rows_in; info[2] = lin->nnz; info[3] = lin->N; info[4] = (long long)lin->bytes; info[5] = lin->form;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_polylinear_clone(mosfhet_hip_ctx_t ctx_other, mosfhet_hip_polylinear_t lin, mosfhet_hip_polylinear_t *out) {
  return clone_image("polylinear_clone", ctx_other, lin, out);
}

// the body of the compute calls, after the argument checks: per round one forward launch over the inputs and one launch of trace_conversions_kernel kind 4
static int polylinear_run(mosfhet_hip_ctx_t ctx, const PackedLinear *lin, const PackedPlan &plan, uint64_t *d_out, const uint64_t *d_in, int idx, int count, hipStream_t s) {
  TraceParams p = {};
  p.kind = TRACE_KIND_POLYLINEAR;
  p.key = lin->at<d2>(PLIN_W); p.row_ptr = lin->at<int>(PLIN_PTR); p.col = lin->at<int>(PLIN_COL); p.bias = lin->has_bias ? lin->at<uint64_t>(PLIN_BIAS) : nullptr;
  p.rows_out = lin->rows_out; p.rows_in = lin->rows_in; p.idx = idx;
  return packed_linear_rounds(ctx, POLYLINEAR, lin, plan, d_out, d_in, idx, count, [&](uint64_t *pool, const uint64_t *src, uint64_t *out, long long n) {
    p.xin = reinterpret_cast<const d2 *>(pool); p.out = out;
    RING_DISPATCH(ctx, lin->N, p.tw = TW;
                  hipLaunchKernelGGL(torus_to_dft_kernel<F>, dim3((unsigned)(n * lin->rows_in * 2)), dim3(F::THREADS), 0, s, (const void *)src, (void *)pool, TW, 0);
                  hipLaunchKernelGGL(trace_conversions_kernel<F>, dim3((unsigned)(n * lin->rows_out)), dim3(F::THREADS), 0, s, p));
  });
}

// src/trlwe.c:491-505 between trlwe_to_DFT and trlwe_from_DFT, over a batch
extern "C" int mosfhet_hip_trlwe_linear_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t lin, uint64_t *d_out, const uint64_t *d_in, int count, void *stream) {
  return packed_linear_call("trlwe_linear", POLYLINEAR, polylinear_run, ctx, lin, d_out, d_in, -1, false, count, stream);
}

// ... followed by trlwe_extract_tlwe(., idx) (src/trlwe.c:540-552); the TRLWE result is never written
extern "C" int mosfhet_hip_trlwe_linear_extract_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t lin, uint64_t *d_out, const uint64_t *d_in, int idx, int count,
                                                      void *stream) {
  return packed_linear_call("trlwe_linear_extract", POLYLINEAR, polylinear_run, ctx, lin, d_out, d_in, idx, true, count, stream);
}

// The extract call into the calling thread's pool (slot POOL_POLYLINEAR_OUT: a slot of its own, as POOL_LINEAR_OUT is), then the body of
// mosfhet_hip_keyswitch_functional_bootstrap_batch on the count * rows_out samples.  No bootstrap or key-switch kernel, launcher or kernel choice differs from that call's.
extern "C" int mosfhet_hip_trlwe_linear_keyswitch_functional_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t lin, mosfhet_hip_ksk_t ksk, mosfhet_hip_bsk_t bsk,
                                                                             uint64_t *d_out, const uint64_t *d_tv, int tv_count, const uint64_t *d_in, int idx, int count,
                                                                             int torus_base, int extract, void *stream) {
  const char *who = "trlwe_linear_keyswitch_bootstrap";
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!lin) return fail(MOSFHET_HIP_EINVAL, "%s: null lin", who);
  if (!ksk) return fail(MOSFHET_HIP_EINVAL, "%s: null ksk", who);
  if (!bsk) return fail(MOSFHET_HIP_EINVAL, "%s: null bsk", who);
  PackedPlan plan;
  bool run;
  int rc = packed_linear_check(who, POLYLINEAR, ctx, lin, nullptr, d_in, idx, true, count, false, &plan, &run);
  if (rc || !run) return rc;
  if (!d_out || !d_tv) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  // the checks of the body below on the two keys, BEFORE anything is queued: the extracted samples are lin->N + 1 words
  if ((rc = ks_bootstrap_keys_match(who, ksk, bsk))) return rc;
  if (ksk->n_in != lin->N) return fail(MOSFHET_HIP_EINVAL, "%s: the handle's ring is N = %d, the key-switch key takes samples of %d words + 1", who, lin->N, ksk->n_in);
  long long samples;
  if ((rc = ks_bootstrap_samples(who, count, lin->rows_out, 0, tv_count, &samples))) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  uint64_t *y = nullptr;
  if ((rc = pool_get(ctx->device, POOL_POLYLINEAR_OUT, (size_t)samples * ((size_t)lin->N + 1), &y))) return rc;
  if ((rc = polylinear_run(ctx, lin, plan, y, d_in, idx, count, pick(ctx, stream)))) return rc;
  return mosfhet_hip_keyswitch_functional_bootstrap_batch(ctx, ksk, bsk, d_out, d_tv, tv_count, y, (int)samples, torus_base, extract, stream);
}

// mosfhet_hip_trlwe_linear_batch into the calling thread's pool (slot POOL_POLYLINEAR_OUT, here [count][rows_out][2][N]), then the body of
// mosfhet_hip_unpack_strided_keyswitch_functional_bootstrap_batch on the count * rows_out results, `per` samples of each: pure composition, the words of the two calls
// one after the other.
extern "C" int mosfhet_hip_trlwe_linear_unpack_keyswitch_functional_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t lin, mosfhet_hip_ksk_t ksk,
                                                                                    mosfhet_hip_bsk_t bsk, uint64_t *d_out, const uint64_t *d_tv, int tv_count,
                                                                                    const uint64_t *d_in, int per, int first, int stride, int count, int torus_base,
                                                                                    int extract, void *stream) {
  const char *who = "trlwe_linear_unpack_keyswitch_bootstrap";
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!lin) return fail(MOSFHET_HIP_EINVAL, "%s: null lin", who);
  if (!ksk) return fail(MOSFHET_HIP_EINVAL, "%s: null ksk", who);
  if (!bsk) return fail(MOSFHET_HIP_EINVAL, "%s: null bsk", who);
  int rc = unpack_scalars(who, 0, per, first, stride);
  if (rc) return rc;
  PackedPlan plan;
  bool run;
  rc = packed_linear_check(who, POLYLINEAR, ctx, lin, nullptr, d_in, -1, false, count, false, &plan, &run);
  if (rc || !run) return rc;
  if (!d_out || !d_tv) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  // the checks of the body below on the two keys and the geometry, BEFORE anything is queued
  if ((rc = ks_bootstrap_keys_match(who, ksk, bsk))) return rc;
  if (bsk->k != 1) return fail(MOSFHET_HIP_EINVAL, "%s: packed inputs have one mask polynomial (k = 1), the bootstrap key has k = %d", who, bsk->k);
  if (ksk->n_in != lin->N) return fail(MOSFHET_HIP_EINVAL, "%s: the handle's ring is N = %d, the key-switch key opens samples of a ring of %d", who, lin->N, ksk->n_in);
  if (ksk->ctx != ctx) return fail(MOSFHET_HIP_EINVAL, "%s: ksk belongs to another context (device %d)", who, ksk->device);
  if (per > lin->N) return fail(MOSFHET_HIP_EINVAL, "%s: per = %d (1 .. N = %d)", who, per, lin->N);
  if ((rc = unpack_geometry(who, lin->N, per, first, stride))) return rc;
  long long samples;
  if ((rc = ks_bootstrap_samples(who, count, lin->rows_out, per, tv_count, &samples))) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  uint64_t *y = nullptr;
  if ((rc = pool_get(ctx->device, POOL_POLYLINEAR_OUT, (size_t)count * lin->rows_out * 2 * (size_t)lin->N, &y))) return rc;
  if ((rc = polylinear_run(ctx, lin, plan, y, d_in, -1, count, pick(ctx, stream)))) return rc;
  return unpack_keyswitch_bootstrap_body(who, ctx, ksk, bsk, d_out, d_tv, tv_count, y, (int)samples, per, first, stride, torus_base, extract, stream);
}
