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
// whole batch elements, which changes no word.  One place decides the shape of a call (gswlinear_plan: for the launcher and for mosfhet_hip_trlwe_gsw_linear_plan).
struct mosfhet_hip_gswlinear {
  mosfhet_hip_ctx_t ctx = nullptr;   // compared, never read: the context may already be destroyed when the handle is freed or cloned
  int device = 0;
  int rows_out = 0, rows_in = 0, N = 0, l = 0, Bg_bit = 0, form = 0, has_bias = 0;
  long long nnz = -1, entries = 0;
  size_t off[4] = {}, bytes = 0;     // offsets of the arrays in the one device image
  char *d = nullptr;
  ~mosfhet_hip_gswlinear() {
    if (ctx) (void)hipSetDevice(device);
    if (d) (void)hipFree(d);
  }
  template <class T> const T *at(int k) const { return reinterpret_cast<const T *>(d + off[k]); }
};
enum { GLIN_W = 0, GLIN_BIAS, GLIN_PTR, GLIN_COL };
enum { GLIN_DENSE = 0, GLIN_SPARSE = 1, GLIN_SELECTORS = 2 };

struct GswLinearPlan { long long teams, round, rounds, pool_bytes, forwards, inverses, weight_bytes, digit_bytes; };

// The gadget the digit rule of ks_rows_rt is exact on: the field (uint32_t)(word >> shift) & ((1u << Bg_bit) - 1) and its half 1 << (Bg_bit - 1) are 32-bit, so
// 1 <= Bg_bit <= 31; GADGET_OFFSET's rounding term 2^(63 - l Bg_bit) needs l Bg_bit <= 63; l = 1 .. 6 as everywhere in this library (check_params).
static int gswlinear_gadget(const char *who, int N, int l, int Bg_bit) { return check_params(who, 1, N, l, Bg_bit); }

// The one place that decides the shape of a call.  `cus` is RESERVED, as in polylinear_plan: checked, sizes nothing today (one team per output sample, a flat grid).
static int gswlinear_plan(const char *who, int N, int l, int rows_out, int rows_in, long long nnz, int count, int extract, int cus, long long workspace, GswLinearPlan *r) {
  if (!ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (1024, 2048, 4096)", who, N);
  if (l < 1 || l > 6) return fail(MOSFHET_HIP_EINVAL, "%s: l = %d (1 .. 6)", who, l);
  if (rows_out < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_out = %d", who, rows_out);
  if (rows_in < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_in = %d", who, rows_in);
  if (nnz < -1 || nnz > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: nnz = %lld (-1 dense, at most 2^31 - 1)", who, nnz);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (extract != 0 && extract != 1) return fail(MOSFHET_HIP_EINVAL, "%s: extract = %d (0 or 1)", who, extract);
  if (cus < 1) return fail(MOSFHET_HIP_EINVAL, "%s: cus = %d", who, cus);
  if (workspace < 0) return fail(MOSFHET_HIP_EINVAL, "%s: workspace_bytes = %lld (0: the current setting)", who, workspace);
  if (workspace == 0) workspace = g_pack_workspace.load(std::memory_order_relaxed);
  const long long entries = nnz < 0 ? (long long)rows_out * rows_in : nnz;
  if (entries > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: rows_out = %d x rows_in = %d weight samples do not fit 2^31 - 1", who, rows_out, rows_in);
  const long long one = (long long)rows_in * 2 * l * N * 8;   // the digit transforms of one batch element: 2l polynomials of N / 2 complex per input
  if (one > workspace)
    return fail(MOSFHET_HIP_EINVAL, "%s: the workspace bound of %lld bytes does not hold the digit transforms of one batch element (%lld): mosfhet_hip_set_tlwe_pack_workspace",
                who, workspace, one);
  const long long fit = workspace / one;
  r->round = count < fit ? count : fit;
  r->rounds = count ? (count + r->round - 1) / r->round : 0;
  r->teams = r->round * rows_out;
  if (r->teams > 0x7fffffffLL || r->round * rows_in > 0x7fffffffLL)
    return fail(MOSFHET_HIP_EINVAL, "%s: %lld batch elements x rows_out = %d (or x rows_in = %d) teams do not fit one launch", who, r->round, rows_out, rows_in);
  r->pool_bytes = r->round * one;
  r->forwards = (long long)count * rows_in * 2 * l;
  r->inverses = (long long)count * rows_out * 2;
  const long long per_team = (entries + rows_out - 1) / rows_out;   // dense: rows_in; sparse: the mean row, rounded up
  r->weight_bytes = per_team * 2 * l * 2 * N * 8;
  r->digit_bytes = per_team * 2 * l * N * 8;
  return MOSFHET_HIP_OK;
}

// plan = { teams of the main launch, batch elements per round, rounds, pool bytes per round, forward transforms per call, inverse transforms per call, weight bytes one
//          team reads, digit bytes one team reads }
extern "C" int mosfhet_hip_trlwe_gsw_linear_plan(int N, int l, int rows_out, int rows_in, long long nnz, int count, int extract, int cus, long long workspace_bytes,
                                                 long long plan[8]) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "trlwe_gsw_linear_plan: null plan");
  GswLinearPlan r;
  const int rc = gswlinear_plan("trlwe_gsw_linear_plan", N, l, rows_out, rows_in, nnz, count, extract, cus, workspace_bytes, &r);
  if (rc) return rc;
  plan[0] = r.teams; plan[1] = r.round; plan[2] = r.rounds; plan[3] = r.pool_bytes; plan[4] = r.forwards; plan[5] = r.inverses; plan[6] = r.weight_bytes;
  plan[7] = r.digit_bytes;
  return MOSFHET_HIP_OK;
}

// Every check of the three creation calls that needs no device, then the image: lists and bias uploaded; the weights uploaded as torus words and transformed into their
// slot by the forward-transform launcher every key of this library goes through (h_W), or copied device to device (d_sel: already TRGSW_DFT samples in slot order).
static int gswlinear_create(const char *who, mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t *out, const int *h_row_ptr, const int *h_col, const uint64_t *h_W,
                            const double *d_sel, const uint64_t *h_bias, int rows_out, int rows_in, int N, int l, int Bg_bit, int form) {
  const bool dense = form == GLIN_DENSE;
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!out) return fail(MOSFHET_HIP_EINVAL, "%s: null out", who);
  if (rows_out < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_out = %d", who, rows_out);
  if (rows_in < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_in = %d", who, rows_in);
  int rc = gswlinear_gadget(who, N, l, Bg_bit);
  if (rc) return rc;
  std::vector<int> ptr((size_t)rows_out + 1, 0), col;
  long long entries;
  if (!dense) {
    if (!h_row_ptr) return fail(MOSFHET_HIP_EINVAL, "%s: null h_row_ptr", who);
    if (h_row_ptr[0] != 0) return fail(MOSFHET_HIP_EINVAL, "%s: row_ptr[0] = %d (must be 0)", who, h_row_ptr[0]);
    for (int j = 0; j < rows_out; j++)
      if (h_row_ptr[j + 1] < h_row_ptr[j]) return fail(MOSFHET_HIP_EINVAL, "%s: row_ptr[%d] = %d is below row_ptr[%d] = %d", who, j + 1, h_row_ptr[j + 1], j, h_row_ptr[j]);
    entries = h_row_ptr[rows_out];
    if (entries && !h_col) return fail(MOSFHET_HIP_EINVAL, "%s: null h_col", who);
    if (entries && form == GLIN_SPARSE && !h_W) return fail(MOSFHET_HIP_EINVAL, "%s: null h_W", who);
    if (entries && form == GLIN_SELECTORS && !d_sel) return fail(MOSFHET_HIP_EINVAL, "%s: null d_sel_dft", who);
    for (long long q = 0; q < entries; q++)
      if (h_col[q] < 0 || h_col[q] >= rows_in) return fail(MOSFHET_HIP_EINVAL, "%s: col[%lld] = %d (rows_in = %d)", who, q, h_col[q], rows_in);
    ptr.assign(h_row_ptr, h_row_ptr + rows_out + 1);
    col.assign(h_col, h_col + entries);
  } else {
    if (!h_W) return fail(MOSFHET_HIP_EINVAL, "%s: null h_W", who);
    entries = (long long)rows_out * rows_in;
    if (entries > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: rows_out = %d x rows_in = %d weight samples do not fit 2^31 - 1", who, rows_out, rows_in);
    col.resize((size_t)entries);
    for (int j = 0; j < rows_out; j++) {
      ptr[j + 1] = (j + 1) * rows_in;
      for (int i = 0; i < rows_in; i++) col[(size_t)j * rows_in + i] = i;
    }
  }
  const long long polys = entries * 4 * l;   // one team of the creation's transform launch per polynomial
  if (polys > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: %lld weight samples x 4 l = %d polynomials do not fit one launch", who, entries, 4 * l);
  std::unique_ptr<mosfhet_hip_gswlinear> h(new mosfhet_hip_gswlinear());
  h->ctx = ctx; h->device = ctx->device; h->rows_out = rows_out; h->rows_in = rows_in; h->N = N; h->l = l; h->Bg_bit = Bg_bit; h->form = form; h->has_bias = h_bias != nullptr;
  h->nnz = dense ? -1 : entries; h->entries = entries;
  const size_t len[4] = {(size_t)polys * N * sizeof(double), h_bias ? (size_t)rows_out * N * sizeof(uint64_t) : 0, ptr.size() * sizeof(int), col.size() * sizeof(int)};
  const void *src[4] = {nullptr, h_bias, ptr.data(), col.data()};
  size_t total = 0;
  for (int k = 0; k < 4; k++) { h->off[k] = total; total += (len[k] + 15) & ~(size_t)15; }
  h->bytes = total;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMalloc((void **)&h->d, h->bytes));
  for (int k = 1; k < 4; k++)
    if (len[k]) HIP_TRY(hipMemcpy(h->d + h->off[k], src[k], len[k], hipMemcpyHostToDevice));
  if (entries && form == GLIN_SELECTORS) {
    HIP_TRY(hipMemcpy(h->d + h->off[GLIN_W], d_sel, len[GLIN_W], hipMemcpyDeviceToDevice));   // (synchronous on the null stream: the image is complete on return)
    HIP_TRY(hipStreamSynchronize(nullptr));
  } else if (entries) {
    DevBuf words;
    HIP_TRY(words.alloc(len[GLIN_W]));
    HIP_TRY(hipMemcpy(words.p, h_W, len[GLIN_W], hipMemcpyHostToDevice));
    RING_DISPATCH(ctx, N, hipLaunchKernelGGL(torus_to_dft_kernel<F>, dim3((unsigned)polys), dim3(F::THREADS), 0, nullptr, (const void *)words.p,
                                             (void *)(h->d + h->off[GLIN_W]), TW, 0));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
  }
  *out = h.release();
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_gswlinear_create_dense(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t *out, const uint64_t *h_W, const uint64_t *h_bias, int rows_out, int rows_in,
                                                  int N, int l, int Bg_bit) {
  return gswlinear_create("gswlinear_create_dense", ctx, out, nullptr, nullptr, h_W, nullptr, h_bias, rows_out, rows_in, N, l, Bg_bit, GLIN_DENSE);
}

extern "C" int mosfhet_hip_gswlinear_create_sparse(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t *out, const int *h_row_ptr, const int *h_col, const uint64_t *h_W,
                                                   const uint64_t *h_bias, int rows_out, int rows_in, int N, int l, int Bg_bit) {
  return gswlinear_create("gswlinear_create_sparse", ctx, out, h_row_ptr, h_col, h_W, nullptr, h_bias, rows_out, rows_in, N, l, Bg_bit, GLIN_SPARSE);
}

extern "C" int mosfhet_hip_gswlinear_create_from_selectors(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t *out, const double *d_sel_dft, const int *h_row_ptr, const int *h_col,
                                                           const uint64_t *h_bias, int rows_out, int rows_in, int N, int l, int Bg_bit) {
  return gswlinear_create("gswlinear_create_from_selectors", ctx, out, h_row_ptr, h_col, nullptr, d_sel_dft, h_bias, rows_out, rows_in, N, l, Bg_bit, GLIN_SELECTORS);
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

// after the pattern of mosfhet_hip_polylinear_clone: a copy of the handle on the device of ctx_other, device to device
extern "C" int mosfhet_hip_gswlinear_clone(mosfhet_hip_ctx_t ctx_other, mosfhet_hip_gswlinear_t lin, mosfhet_hip_gswlinear_t *out) {
  if (!ctx_other) return fail(MOSFHET_HIP_EINVAL, "gswlinear_clone: null ctx_other");
  if (!lin) return fail(MOSFHET_HIP_EINVAL, "gswlinear_clone: null lin");
  if (!out) return fail(MOSFHET_HIP_EINVAL, "gswlinear_clone: null out");
  HIP_TRY(hipSetDevice(lin->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipSetDevice(ctx_other->device));
  std::unique_ptr<mosfhet_hip_gswlinear> h(new mosfhet_hip_gswlinear());
  h->ctx = ctx_other; h->device = ctx_other->device;
  h->rows_out = lin->rows_out; h->rows_in = lin->rows_in; h->N = lin->N; h->l = lin->l; h->Bg_bit = lin->Bg_bit; h->form = lin->form; h->has_bias = lin->has_bias;
  h->nnz = lin->nnz; h->entries = lin->entries; h->bytes = lin->bytes;
  memcpy(h->off, lin->off, sizeof(h->off));
  HIP_TRY(hipMalloc((void **)&h->d, h->bytes));
  const int rc = copy_across(h->d, ctx_other->device, lin->d, lin->device, h->bytes);
  if (rc) return rc;
  *out = h.release();
  return MOSFHET_HIP_OK;
}

// the body of the compute calls, after the argument checks: per round one launch of trace_conversions_kernel kind 5 over the inputs and one of kind 6.
// idx < 0: d_out [count][rows_out][2][N]; else [count][rows_out][N + 1]
static int gswlinear_run(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t lin, const GswLinearPlan &plan, uint64_t *d_out, const uint64_t *d_in, int idx, int count,
                         hipStream_t s) {
  const int N = lin->N;
  uint64_t *pool = nullptr;
  const int rc = pool_get(ctx->device, POOL_GSWLINEAR, (size_t)(plan.pool_bytes / (long long)sizeof(uint64_t)), &pool);
  if (rc) return rc;
  TraceParams dg = {}, p = {};
  dg.kind = TRACE_KIND_GSW_DIGITS;
  dg.sel = reinterpret_cast<d2 *>(pool);
  dg.l = lin->l; dg.base_bit = lin->Bg_bit;
  p.kind = TRACE_KIND_GSW_SUM;
  p.key = lin->at<d2>(GLIN_W); p.row_ptr = lin->at<int>(GLIN_PTR); p.col = lin->at<int>(GLIN_COL); p.bias = lin->has_bias ? lin->at<uint64_t>(GLIN_BIAS) : nullptr;
  p.xin = reinterpret_cast<const d2 *>(pool);
  p.l = lin->l; p.rows_out = lin->rows_out; p.rows_in = lin->rows_in; p.idx = idx;
  const size_t out_words = idx < 0 ? (size_t)2 * N : (size_t)N + 1;
  for (long long b0 = 0; b0 < count; b0 += plan.round) {
    const long long n = count - b0 < plan.round ? count - b0 : plan.round;
    dg.in = d_in + (size_t)b0 * lin->rows_in * 2 * N;
    p.out = d_out + (size_t)b0 * lin->rows_out * out_words;
    RING_DISPATCH(ctx, N, dg.tw = p.tw = TW;
                  hipLaunchKernelGGL(trace_conversions_kernel<F>, dim3((unsigned)(n * lin->rows_in)), dim3(F::THREADS), 0, s, dg);
                  hipLaunchKernelGGL(trace_conversions_kernel<F>, dim3((unsigned)(n * lin->rows_out)), dim3(F::THREADS), 0, s, p));
  }
  return launched();
}

// The checks the compute calls share.  Null handles and scalar ranges come before any handle is read and before any HIP call; *run = false: nothing to do.
static int gswlinear_check(const char *who, mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t lin, const void *d_out, const void *d_in, int idx, bool extract, int count,
                           GswLinearPlan *plan, bool *run) {
  *run = false;
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!lin) return fail(MOSFHET_HIP_EINVAL, "%s: null lin", who);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (extract && idx < 0) return fail(MOSFHET_HIP_EINVAL, "%s: idx = %d (0 .. N - 1)", who, idx);
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_in) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  if (extract && idx >= lin->N) return fail(MOSFHET_HIP_EINVAL, "%s: idx = %d (0 .. N - 1 = %d)", who, idx, lin->N - 1);
  if (lin->ctx != ctx) return fail(MOSFHET_HIP_EINVAL, "%s: lin belongs to another context (device %d): mosfhet_hip_gswlinear_clone makes a copy for this one", who, lin->device);
  const int rc = gswlinear_plan(who, lin->N, lin->l, lin->rows_out, lin->rows_in, lin->nnz, count, extract, 256, 0, plan);
  if (rc) return rc;
  const size_t out_words = extract ? (size_t)lin->N + 1 : (size_t)2 * lin->N;
  if (linear_overlap(d_out, (size_t)count * lin->rows_out * out_words * sizeof(uint64_t), d_in, (size_t)count * lin->rows_in * 2 * lin->N * sizeof(uint64_t)))
    return fail(MOSFHET_HIP_EINVAL, "%s: d_out overlaps d_in", who);
  *run = true;
  return MOSFHET_HIP_OK;
}

// sums of src/trgsw.c:385-423 with one rounding, over a batch
extern "C" int mosfhet_hip_trlwe_gsw_linear_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t lin, uint64_t *d_out, const uint64_t *d_in, int count, void *stream) {
  GswLinearPlan plan;
  bool run;
  const int rc = gswlinear_check("trlwe_gsw_linear", ctx, lin, d_out, d_in, -1, false, count, &plan, &run);
  if (rc || !run) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return gswlinear_run(ctx, lin, plan, d_out, d_in, -1, count, pick(ctx, stream));
}

// ... followed by trlwe_extract_tlwe(., idx) (src/trlwe.c:540-552); the TRLWE result is never written
extern "C" int mosfhet_hip_trlwe_gsw_linear_extract_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gswlinear_t lin, uint64_t *d_out, const uint64_t *d_in, int idx, int count,
                                                          void *stream) {
  GswLinearPlan plan;
  bool run;
  const int rc = gswlinear_check("trlwe_gsw_linear_extract", ctx, lin, d_out, d_in, idx, true, count, &plan, &run);
  if (rc || !run) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return gswlinear_run(ctx, lin, plan, d_out, d_in, idx, count, pick(ctx, stream));
}
