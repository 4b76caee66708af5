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
// bounded by mosfhet_hip_set_tlwe_pack_workspace; a larger batch runs in rounds of whole batch elements, which changes no word.  One place decides the shape of a call
// (polylinear_plan: for the launcher and for mosfhet_hip_trlwe_linear_plan).
struct mosfhet_hip_polylinear {
  mosfhet_hip_ctx_t ctx = nullptr;   // compared, never read: the context may already be destroyed when the handle is freed or cloned
  int device = 0;
  int rows_out = 0, rows_in = 0, N = 0, sparse = 0, has_bias = 0;
  long long nnz = -1, entries = 0;
  size_t off[4] = {}, bytes = 0;     // offsets of the arrays in the one device image
  char *d = nullptr;
  ~mosfhet_hip_polylinear() {
    if (ctx) (void)hipSetDevice(device);
    if (d) (void)hipFree(d);
  }
  template <class T> const T *at(int k) const { return reinterpret_cast<const T *>(d + off[k]); }
};
enum { PLIN_W = 0, PLIN_BIAS, PLIN_PTR, PLIN_COL };

struct PolyLinearPlan { long long teams, round, rounds, pool_bytes, forwards, inverses, weight_bytes, input_bytes; };

// The one place that decides the shape of a call.  `cus` is RESERVED, as in linear_plan: checked, sizes nothing today (one team per output sample, a flat grid).
static int polylinear_plan(const char *who, int N, int rows_out, int rows_in, long long nnz, int count, int extract, int cus, long long workspace, PolyLinearPlan *r) {
  if (!ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (1024, 2048, 4096)", who, N);
  if (rows_out < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_out = %d", who, rows_out);
  if (rows_in < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_in = %d", who, rows_in);
  if (nnz < -1 || nnz > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: nnz = %lld (-1 dense, at most 2^31 - 1)", who, nnz);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (extract != 0 && extract != 1) return fail(MOSFHET_HIP_EINVAL, "%s: extract = %d (0 or 1)", who, extract);
  if (cus < 1) return fail(MOSFHET_HIP_EINVAL, "%s: cus = %d", who, cus);
  if (workspace < 0) return fail(MOSFHET_HIP_EINVAL, "%s: workspace_bytes = %lld (0: the current setting)", who, workspace);
  if (workspace == 0) workspace = g_pack_workspace.load(std::memory_order_relaxed);
  const long long entries = nnz < 0 ? (long long)rows_out * rows_in : nnz;
  if (entries > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: rows_out = %d x rows_in = %d weight polynomials do not fit 2^31 - 1", who, rows_out, rows_in);
  const long long one = (long long)rows_in * 2 * N * 8;   // the transformed inputs of one batch element
  if (one > workspace)
    return fail(MOSFHET_HIP_EINVAL, "%s: the workspace bound of %lld bytes does not hold the transformed inputs of one batch element (%lld): mosfhet_hip_set_tlwe_pack_workspace",
                who, workspace, one);
  const long long fit = workspace / one;
  r->round = count < fit ? count : fit;
  r->rounds = count ? (count + r->round - 1) / r->round : 0;
  r->teams = r->round * rows_out;
  if (r->teams > 0x7fffffffLL || r->round * rows_in * 2 > 0x7fffffffLL)
    return fail(MOSFHET_HIP_EINVAL, "%s: %lld batch elements x rows_out = %d (or x 2 rows_in = %d) teams do not fit one launch", who, r->round, rows_out, rows_in);
  r->pool_bytes = r->round * one;
  r->forwards = (long long)count * rows_in * 2;
  r->inverses = (long long)count * rows_out * 2;
  const long long per_team = (entries + rows_out - 1) / rows_out;   // dense: rows_in; sparse: the mean row, rounded up
  r->weight_bytes = per_team * N * 8;
  r->input_bytes = per_team * 2 * N * 8;
  return MOSFHET_HIP_OK;
}

// plan = { teams of the main launch, batch elements per round, rounds, pool bytes per round, forward transforms per call, inverse transforms per call, weight bytes one
//          team reads, input bytes one team reads }
extern "C" int mosfhet_hip_trlwe_linear_plan(int N, int rows_out, int rows_in, long long nnz, int count, int extract, int cus, long long workspace_bytes, long long plan[8]) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "trlwe_linear_plan: null plan");
  PolyLinearPlan r;
  const int rc = polylinear_plan("trlwe_linear_plan", N, rows_out, rows_in, nnz, count, extract, cus, workspace_bytes, &r);
  if (rc) return rc;
  plan[0] = r.teams; plan[1] = r.round; plan[2] = r.rounds; plan[3] = r.pool_bytes; plan[4] = r.forwards; plan[5] = r.inverses; plan[6] = r.weight_bytes;
  plan[7] = r.input_bytes;
  return MOSFHET_HIP_OK;
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
  std::vector<int> ptr((size_t)rows_out + 1, 0), col;
  long long entries;
  if (sparse) {
    if (!h_row_ptr) return fail(MOSFHET_HIP_EINVAL, "%s: null h_row_ptr", who);
    if (h_row_ptr[0] != 0) return fail(MOSFHET_HIP_EINVAL, "%s: row_ptr[0] = %d (must be 0)", who, h_row_ptr[0]);
    for (int j = 0; j < rows_out; j++)
      if (h_row_ptr[j + 1] < h_row_ptr[j]) return fail(MOSFHET_HIP_EINVAL, "%s: row_ptr[%d] = %d is below row_ptr[%d] = %d", who, j + 1, h_row_ptr[j + 1], j, h_row_ptr[j]);
    entries = h_row_ptr[rows_out];
    if (entries && (!h_col || !h_val)) return fail(MOSFHET_HIP_EINVAL, "%s: null h_col or h_val", who);
    for (long long q = 0; q < entries; q++)
      if (h_col[q] < 0 || h_col[q] >= rows_in) return fail(MOSFHET_HIP_EINVAL, "%s: col[%lld] = %d (rows_in = %d)", who, q, h_col[q], rows_in);
    ptr.assign(h_row_ptr, h_row_ptr + rows_out + 1);
    col.assign(h_col, h_col + entries);
  } else {
    if (!h_val) return fail(MOSFHET_HIP_EINVAL, "%s: null h_W", who);
    entries = (long long)rows_out * rows_in;
    if (entries > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: rows_out = %d x rows_in = %d weight polynomials do not fit 2^31 - 1", who, rows_out, rows_in);
    col.resize((size_t)entries);
    for (int j = 0; j < rows_out; j++) {
      ptr[j + 1] = (j + 1) * rows_in;
      for (int i = 0; i < rows_in; i++) col[(size_t)j * rows_in + i] = i;
    }
  }
  std::unique_ptr<mosfhet_hip_polylinear> h(new mosfhet_hip_polylinear());
  h->ctx = ctx; h->device = ctx->device; h->rows_out = rows_out; h->rows_in = rows_in; h->N = N; h->sparse = sparse; h->has_bias = h_bias != nullptr;
  h->nnz = sparse ? entries : -1; h->entries = entries;
  const size_t len[4] = {(size_t)entries * N * sizeof(double), h_bias ? (size_t)rows_out * N * sizeof(uint64_t) : 0, ptr.size() * sizeof(int), col.size() * sizeof(int)};
  const void *src[4] = {nullptr, h_bias, ptr.data(), col.data()};
  size_t total = 0;
  for (int k = 0; k < 4; k++) { h->off[k] = total; total += (len[k] + 15) & ~(size_t)15; }
  h->bytes = total;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMalloc((void **)&h->d, h->bytes));
  for (int k = 1; k < 4; k++)
    if (len[k]) HIP_TRY(hipMemcpy(h->d + h->off[k], src[k], len[k], hipMemcpyHostToDevice));
  if (entries) {
    DevBuf words;   // (double)(int64_t): a weight is converted exactly as a torus word is
    HIP_TRY(words.alloc(len[PLIN_W]));
    HIP_TRY(hipMemcpy(words.p, h_val, len[PLIN_W], hipMemcpyHostToDevice));
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
  info[0] = lin->rows_out; info[1] = lin->rows_in; info[2] = lin->nnz; info[3] = lin->N; info[4] = (long long)lin->bytes; info[5] = lin->sparse;
  return MOSFHET_HIP_OK;
}

// after the pattern of mosfhet_hip_linear_clone: a copy of the handle on the device of ctx_other, device to device
extern "C" int mosfhet_hip_polylinear_clone(mosfhet_hip_ctx_t ctx_other, mosfhet_hip_polylinear_t lin, mosfhet_hip_polylinear_t *out) {
  if (!ctx_other) return fail(MOSFHET_HIP_EINVAL, "polylinear_clone: null ctx_other");
  if (!lin) return fail(MOSFHET_HIP_EINVAL, "polylinear_clone: null lin");
  if (!out) return fail(MOSFHET_HIP_EINVAL, "polylinear_clone: null out");
  HIP_TRY(hipSetDevice(lin->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipSetDevice(ctx_other->device));
  std::unique_ptr<mosfhet_hip_polylinear> h(new mosfhet_hip_polylinear());
  h->ctx = ctx_other; h->device = ctx_other->device;
  h->rows_out = lin->rows_out; h->rows_in = lin->rows_in; h->N = lin->N; h->sparse = lin->sparse; h->has_bias = lin->has_bias; h->nnz = lin->nnz; h->entries = lin->entries;
  h->bytes = lin->bytes;
  memcpy(h->off, lin->off, sizeof(h->off));
  HIP_TRY(hipMalloc((void **)&h->d, h->bytes));
  const int rc = copy_across(h->d, ctx_other->device, lin->d, lin->device, h->bytes);
  if (rc) return rc;
  *out = h.release();
  return MOSFHET_HIP_OK;
}

// the body of the compute calls, after the argument checks: per round one forward launch over the inputs and one launch of trace_conversions_kernel kind 4.
// idx < 0: d_out [count][rows_out][2][N]; else [count][rows_out][N + 1]
static int polylinear_run(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t lin, const PolyLinearPlan &plan, uint64_t *d_out, const uint64_t *d_in, int idx, int count,
                          hipStream_t s) {
  const int N = lin->N;
  uint64_t *pool = nullptr;
  const int rc = pool_get(ctx->device, POOL_POLYLINEAR, (size_t)(plan.pool_bytes / (long long)sizeof(uint64_t)), &pool);
  if (rc) return rc;
  TraceParams p = {};
  p.kind = TRACE_KIND_POLYLINEAR;
  p.key = lin->at<d2>(PLIN_W); p.row_ptr = lin->at<int>(PLIN_PTR); p.col = lin->at<int>(PLIN_COL); p.bias = lin->has_bias ? lin->at<uint64_t>(PLIN_BIAS) : nullptr;
  p.xin = reinterpret_cast<const d2 *>(pool);
  p.rows_out = lin->rows_out; p.rows_in = lin->rows_in; p.idx = idx;
  const size_t out_words = idx < 0 ? (size_t)2 * N : (size_t)N + 1;
  for (long long b0 = 0; b0 < count; b0 += plan.round) {
    const long long n = count - b0 < plan.round ? count - b0 : plan.round;
    const uint64_t *src = d_in + (size_t)b0 * lin->rows_in * 2 * N;
    p.out = d_out + (size_t)b0 * lin->rows_out * out_words;
    RING_DISPATCH(ctx, N, p.tw = TW;
                  hipLaunchKernelGGL(torus_to_dft_kernel<F>, dim3((unsigned)(n * lin->rows_in * 2)), dim3(F::THREADS), 0, s, (const void *)src, (void *)pool, TW, 0);
                  hipLaunchKernelGGL(trace_conversions_kernel<F>, dim3((unsigned)(n * lin->rows_out)), dim3(F::THREADS), 0, s, p));
  }
  return launched();
}

// The checks the compute calls share.  Null handles and scalar ranges come before any handle is read and before any HIP call; *run = false: nothing to do.
static int polylinear_check(const char *who, mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t lin, const void *d_out, const void *d_in, int idx, bool extract, int count,
                            bool need_out, PolyLinearPlan *plan, bool *run) {
  *run = false;
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!lin) return fail(MOSFHET_HIP_EINVAL, "%s: null lin", who);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (extract && idx < 0) return fail(MOSFHET_HIP_EINVAL, "%s: idx = %d (0 .. N - 1)", who, idx);
  if (extract && idx >= lin->N) return fail(MOSFHET_HIP_EINVAL, "%s: idx = %d (0 .. N - 1 = %d)", who, idx, lin->N - 1);
  if (count == 0) return MOSFHET_HIP_OK;
  if ((need_out && !d_out) || !d_in) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  if (lin->ctx != ctx) return fail(MOSFHET_HIP_EINVAL, "%s: lin belongs to another context (device %d): mosfhet_hip_polylinear_clone makes a copy for this one", who, lin->device);
  const int rc = polylinear_plan(who, lin->N, lin->rows_out, lin->rows_in, lin->nnz, count, extract, 256, 0, plan);
  if (rc) return rc;
  if (need_out) {
    const size_t out_words = extract ? (size_t)lin->N + 1 : (size_t)2 * lin->N;
    if (linear_overlap(d_out, (size_t)count * lin->rows_out * out_words * sizeof(uint64_t), d_in, (size_t)count * lin->rows_in * 2 * lin->N * sizeof(uint64_t)))
      return fail(MOSFHET_HIP_EINVAL, "%s: d_out overlaps d_in", who);
  }
  *run = true;
  return MOSFHET_HIP_OK;
}

// src/trlwe.c:491-505 between trlwe_to_DFT and trlwe_from_DFT, over a batch
extern "C" int mosfhet_hip_trlwe_linear_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t lin, uint64_t *d_out, const uint64_t *d_in, int count, void *stream) {
  PolyLinearPlan plan;
  bool run;
  const int rc = polylinear_check("trlwe_linear", ctx, lin, d_out, d_in, -1, false, count, true, &plan, &run);
  if (rc || !run) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return polylinear_run(ctx, lin, plan, d_out, d_in, -1, count, pick(ctx, stream));
}

// ... followed by trlwe_extract_tlwe(., idx) (src/trlwe.c:540-552); the TRLWE result is never written
extern "C" int mosfhet_hip_trlwe_linear_extract_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_polylinear_t lin, uint64_t *d_out, const uint64_t *d_in, int idx, int count,
                                                      void *stream) {
  PolyLinearPlan plan;
  bool run;
  const int rc = polylinear_check("trlwe_linear_extract", ctx, lin, d_out, d_in, idx, true, count, true, &plan, &run);
  if (rc || !run) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return polylinear_run(ctx, lin, plan, d_out, d_in, idx, count, pick(ctx, stream));
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
  PolyLinearPlan plan;
  bool run;
  int rc = polylinear_check(who, ctx, lin, nullptr, d_in, idx, true, count, false, &plan, &run);
  if (rc || !run) return rc;
  if (!d_out || !d_tv) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  // the checks of the body below on the two keys, BEFORE anything is queued: the extracted samples are lin->N + 1 words
  if (ksk->n_in != bsk->k * bsk->N || ksk->n_out != bsk->n || ksk->b_word != ksk->n_out)
    return fail(MOSFHET_HIP_EINVAL, "%s: key-switch key is %d -> %d, expected %d -> %d", who, ksk->n_in, ksk->n_out, bsk->k * bsk->N, bsk->n);
  if (ksk->n_in != lin->N) return fail(MOSFHET_HIP_EINVAL, "%s: the handle's ring is N = %d, the key-switch key takes samples of %d words + 1", who, lin->N, ksk->n_in);
  const long long samples = (long long)count * lin->rows_out;
  if (samples > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d x rows_out = %d samples do not fit an int", who, count, lin->rows_out);
  if (tv_count != 1 && tv_count != samples) return fail(MOSFHET_HIP_EINVAL, "%s: tv_count = %d (1 or count * rows_out = %lld)", who, tv_count, samples);
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
  PolyLinearPlan plan;
  bool run;
  rc = polylinear_check(who, ctx, lin, nullptr, d_in, -1, false, count, false, &plan, &run);
  if (rc || !run) return rc;
  if (!d_out || !d_tv) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  // the checks of the body below on the two keys and the geometry, BEFORE anything is queued
  if (ksk->n_in != bsk->k * bsk->N || ksk->n_out != bsk->n || ksk->b_word != ksk->n_out)
    return fail(MOSFHET_HIP_EINVAL, "%s: key-switch key is %d -> %d, expected %d -> %d", who, ksk->n_in, ksk->n_out, bsk->k * bsk->N, bsk->n);
  if (bsk->k != 1) return fail(MOSFHET_HIP_EINVAL, "%s: packed inputs have one mask polynomial (k = 1), the bootstrap key has k = %d", who, bsk->k);
  if (ksk->n_in != lin->N) return fail(MOSFHET_HIP_EINVAL, "%s: the handle's ring is N = %d, the key-switch key opens samples of a ring of %d", who, lin->N, ksk->n_in);
  if (ksk->ctx != ctx) return fail(MOSFHET_HIP_EINVAL, "%s: ksk belongs to another context (device %d)", who, ksk->device);
  if (per > lin->N) return fail(MOSFHET_HIP_EINVAL, "%s: per = %d (1 .. N = %d)", who, per, lin->N);
  if ((rc = unpack_geometry(who, lin->N, per, first, stride))) return rc;
  const long long inputs = (long long)count * lin->rows_out, samples = inputs * per;
  if (samples > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d x rows_out = %d x per = %d samples do not fit an int", who, count, lin->rows_out, per);
  if (tv_count != 1 && tv_count != samples) return fail(MOSFHET_HIP_EINVAL, "%s: tv_count = %d (1 or count * rows_out * per = %lld)", who, tv_count, samples);
  HIP_TRY(hipSetDevice(ctx->device));
  uint64_t *y = nullptr;
  if ((rc = pool_get(ctx->device, POOL_POLYLINEAR_OUT, (size_t)inputs * 2 * (size_t)lin->N, &y))) return rc;
  if ((rc = polylinear_run(ctx, lin, plan, y, d_in, -1, count, pick(ctx, stream)))) return rc;
  return unpack_keyswitch_bootstrap_body(who, ctx, ksk, bsk, d_out, d_tv, tv_count, y, (int)samples, per, first, stride, torus_base, extract, stream);
}
