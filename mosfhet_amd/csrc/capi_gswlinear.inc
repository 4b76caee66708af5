// capi_gswlinear.inc -- ENCRYPTED polynomial-weight linear layers on batches of packed TRLWE samples: sums of the reference's trgsw_mul_trlwe_DFT (src/trgsw.c:385-423)
// with ONE rounding per output component, then trlwe_from_DFT or trlwe_extract_tlwe (src/trlwe.c:540-552), as one call over a batch, dense, sparse (CSR over TRGSW
// blocks) or over selectors already on the device.  Own code: nothing of the reference is compiled in.  Kernels: gsw_digits_body and gsw_sum_body, trace_kernels.h.
//
//   acc_a = acc_b = +0.0
//   for e in row j's entries, in the stored order:  for c in (a, b):  for i < l:
//       d = F(dec_i(in[b][col_e].c));  acc_a = mul_addto(acc_a, d, W_e[c l + i].a);  acc_b = mul_addto(acc_b, d, W_e[c l + i].b)
//   out[b][j] = (G(acc_a), G(acc_b) + bias[j])
//
// The handle holds the weights as TRGSW_DFT samples [entries][2l][2][N/2] complex in slot order (torus rows transformed by torus_to_dft_kernel at creation, or selectors
// copied device to device), the lists and the bias in one device image, read-only after creation.  A call is two launches per round: trace_conversions_kernel kind 5
// over the round's inputs into the calling thread's pool (slot POOL_GSWLINEAR, [round][rows_in][2l][N/2] complex: every digit transform is made once and read by all
// rows_out teams), then kind 6, one team per (batch element, output row).  The pool is bounded by mosfhet_hip_set_tlwe_pack_workspace; a larger batch runs in rounds of
// whole batch elements, which changes no word.  The handle's image and clone, the plan, the checks of the compute calls and the loop over rounds are the packed
// families' shared ones: capi_linear_common.inc.
struct mosfhet_hip_gswlinear : PackedLinear {};   // form: PLIN_DENSE, PLIN_SPARSE or PLIN_SELECTORS
static const PackedFamily GSWLINEAR = {true, 1, POOL_GSWLINEAR, "weight samples", "digit transforms", "mosfhet_hip_gswlinear_clone"};

// The gadget the digit rule of ks_rows_rt is exact on: the field (uint32_t)(word >> shift) & ((1u << Bg_bit) - 1) and its half 1 << (Bg_bit - 1) are 32-bit, so
// 1 <= Bg_bit <= 31; GADGET_OFFSET's rounding term 2^(63 - l Bg_bit) needs l Bg_bit <= 63; l = 1 .. 6 as everywhere in this library (check_params).
static int gswlinear_gadget(const char *who, int N, int l, int Bg_bit) { return check_params(who, 1, N, l, Bg_bit); }

extern "C" int mosfhet_hip_trlwe_gsw_linear_plan(int N, int l, int rows_out, int rows_in, long long nnz, int count, int extract, int cus, long long workspace_bytes,
                                                 long long plan[8]) {
  return packed_linear_plan_out("trlwe_gsw_linear_plan", GSWLINEAR, N, l, rows_out, rows_in, nnz, count, extract, cus, workspace_bytes, plan);
}

// Every check of the three creation calls that needs no device, then the image: lists and bias uploaded; the weights uploaded as torus words and transformed into their
// slot by the forward-transform launcher every key of this library goes through (h_W), or copied device to device (d_sel: already TRGSW_DFT samples in slot order).
static int gswlinear_create(const char *who, mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t *out, const int *h_row_ptr, const int *h_col, const uint64_t *h_W,
                            const double *d_sel, const uint64_t *h_bias, int rows_out, int rows_in, int N, int l, int Bg_bit, int form) {
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!out) return fail(MOSFHET_HIP_EINVAL, "%s: null out", who);
  if (rows_out < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_out = %d", who, rows_out);
  if (rows_in < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_in = %d", who, rows_in);
  int rc = gswlinear_gadget(who, N, l, Bg_bit);
  if (rc) return rc;
  std::vector<int> ptr, col;
  // The null array that packed_linear_lists refuses where there are entries ("null h_col", else "null h_W" or "null d_sel_dft": one message, the order of the
  // three checks this stands for).  The second assignment overrides the first: a null h_col is named before a null weight array.
  const char *missing = nullptr;
  if (form == PLIN_SELECTORS ? !d_sel : !h_W) missing = form == PLIN_SELECTORS ? "d_sel_dft" : "h_W";
  if (form != PLIN_DENSE && !h_col) missing = "h_col";
  if ((rc = packed_linear_lists(who, GSWLINEAR, form != PLIN_DENSE, h_row_ptr, h_col, missing, rows_out, rows_in, ptr, col))) return rc;
  const long long entries = (long long)col.size();
  const long long polys = entries * 4 * l;   // one team of the creation's transform launch per polynomial
  if (polys > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: %lld weight samples x 4 l = %d polynomials do not fit one launch", who, entries, 4 * l);
  std::unique_ptr<mosfhet_hip_gswlinear> h(new mosfhet_hip_gswlinear());
  h->rows_out = rows_out; h->rows_in = rows_in; h->N = N; h->l = l; h->Bg_bit = Bg_bit; h->form = form; h->has_bias = h_bias != nullptr;
  h->nnz = form == PLIN_DENSE ? -1 : entries; h->entries = entries;
  const size_t weight_bytes = (size_t)polys * N * sizeof(double);
  if ((rc = packed_linear_image(h.get(), ctx, weight_bytes, h_bias, ptr, col))) return rc;
  if (entries && form == PLIN_SELECTORS) {
    HIP_TRY(hipMemcpy(h->d + h->off[PLIN_W], d_sel, weight_bytes, hipMemcpyDeviceToDevice));   // (synchronous on the null stream: the image is complete on return)
    HIP_TRY(hipStreamSynchronize(nullptr));
  } else if (entries) {
    DevBuf words;
    HIP_TRY(words.alloc(weight_bytes));
    HIP_TRY(hipMemcpy(words.p, h_W, weight_bytes, hipMemcpyHostToDevice));
    RING_DISPATCH(ctx, N, hipLaunchKernelGGL(torus_to_dft_kernel<F>, dim3((unsigned)polys), dim3(F::THREADS), 0, nullptr, (const void *)words.p,
                                             (void *)(h->d + h->off[PLIN_W]), TW, 0));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
  }
  *out = h.release();
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_gswlinear_create_dense(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t *out, const uint64_t *h_W, const uint64_t *h_bias, int rows_out, int rows_in,
                                                  int N, int l, int Bg_bit) {
  return gswlinear_create("gswlinear_create_dense", ctx, out, nullptr, nullptr, h_W, nullptr, h_bias, rows_out, rows_in, N, l, Bg_bit, PLIN_DENSE);
}

extern "C" int mosfhet_hip_gswlinear_create_sparse(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t *out, const int *h_row_ptr, const int *h_col, const uint64_t *h_W,
                                                   const uint64_t *h_bias, int rows_out, int rows_in, int N, int l, int Bg_bit) {
  return gswlinear_create("gswlinear_create_sparse", ctx, out, h_row_ptr, h_col, h_W, nullptr, h_bias, rows_out, rows_in, N, l, Bg_bit, PLIN_SPARSE);
}

extern "C" int mosfhet_hip_gswlinear_create_from_selectors(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t *out, const double *d_sel_dft, const int *h_row_ptr, const int *h_col,
                                                           const uint64_t *h_bias, int rows_out, int rows_in, int N, int l, int Bg_bit) {
  return gswlinear_create("gswlinear_create_from_selectors", ctx, out, h_row_ptr, h_col, nullptr, d_sel_dft, h_bias, rows_out, rows_in, N, l, Bg_bit, PLIN_SELECTORS);
}

extern "C" int mosfhet_hip_gswlinear_destroy(mosfhet_hip_gswlinear_t lin) {
  delete lin;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_gswlinear_info(mosfhet_hip_gswlinear_t lin, long long info[8]) {
  if (!lin || !info) return fail(MOSFHET_HIP_EINVAL, "gswlinear_info: null %s", lin ? "info" : "lin");
  info[0] = lin->rows_out; info[1] = lin->rows_in; info[2] = lin->nnz; info[3] = lin->N; info[4] = lin->l; info[5] = lin->Bg_bit; info[6] = (long long)lin->bytes;
  info[7] = lin->form;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_gswlinear_clone(mosfhet_hip_ctx_t ctx_other, mosfhet_hip_gswlinear_t lin, mosfhet_hip_gswlinear_t *out) {
  return clone_image("gswlinear_clone", ctx_other, lin, out);
}

// the body of the compute calls, after the argument checks: per round one launch of trace_conversions_kernel kind 5 over the inputs and one of kind 6
static int gswlinear_run(mosfhet_hip_ctx_t ctx, const PackedLinear *lin, const PackedPlan &plan, uint64_t *d_out, const uint64_t *d_in, int idx, int count, hipStream_t s) {
  TraceParams dg = {}, p = {};
  dg.kind = TRACE_KIND_GSW_DIGITS;
  dg.l = lin->l; dg.base_bit = lin->Bg_bit;
  p.kind = TRACE_KIND_GSW_SUM;
  p.key = lin->at<d2>(PLIN_W); p.row_ptr = lin->at<int>(PLIN_PTR); p.col = lin->at<int>(PLIN_COL); p.bias = lin->has_bias ? lin->at<uint64_t>(PLIN_BIAS) : nullptr;
  p.l = lin->l; p.rows_out = lin->rows_out; p.rows_in = lin->rows_in; p.idx = idx;
  return packed_linear_rounds(ctx, GSWLINEAR, lin, plan, d_out, d_in, idx, count, [&](uint64_t *pool, const uint64_t *src, uint64_t *out, long long n) {
    dg.sel = reinterpret_cast<d2 *>(pool); dg.in = src;
    p.xin = reinterpret_cast<const d2 *>(pool); p.out = out;
    RING_DISPATCH(ctx, lin->N, dg.tw = p.tw = TW;
                  hipLaunchKernelGGL(trace_conversions_kernel<F>, dim3((unsigned)(n * lin->rows_in)), dim3(F::THREADS), 0, s, dg);
                  hipLaunchKernelGGL(trace_conversions_kernel<F>, dim3((unsigned)(n * lin->rows_out)), dim3(F::THREADS), 0, s, p));
  });
}

// sums of src/trgsw.c:385-423 with one rounding, over a batch
extern "C" int mosfhet_hip_trlwe_gsw_linear_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t lin, uint64_t *d_out, const uint64_t *d_in, int count, void *stream) {
  return packed_linear_call("trlwe_gsw_linear", GSWLINEAR, gswlinear_run, ctx, lin, d_out, d_in, -1, false, count, stream);
}

// ... followed by trlwe_extract_tlwe(., idx) (src/trlwe.c:540-552); the TRLWE result is never written
extern "C" int mosfhet_hip_trlwe_gsw_linear_extract_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t lin, uint64_t *d_out, const uint64_t *d_in, int idx, int count,
                                                          void *stream) {
  return packed_linear_call("trlwe_gsw_linear_extract", GSWLINEAR, gswlinear_run, ctx, lin, d_out, d_in, idx, true, count, stream);
}
