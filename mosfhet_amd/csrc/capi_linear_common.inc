// capi_linear_common.inc -- what the three families of linear layers share, each defined once: the CSR checks and the dense lists, the handles' one device image and
// its clone (capi_linear.inc, capi_polylinear.inc, capi_gswlinear.inc), and, for the two families on packed TRLWE samples, the handle's shape, the plan of a call, the
// checks of the compute calls and the loop over rounds.  Host code only; own code: nothing of the reference is compiled in.

// ---- lists ----
// The caller's CSR arrays, before anything is copied: *entries = row_ptr[rows_out].  `missing` names an array of the entries that the caller left null (or is null):
// it is refused only where there are entries, between the row pointers and the columns.
static int csr_check(const char *who, const int *h_row_ptr, const int *h_col, int rows_out, int rows_in, const char *missing, long long *entries) {
  if (!h_row_ptr) return fail(MOSFHET_HIP_EINVAL, "%s: null h_row_ptr", who);
  if (h_row_ptr[0] != 0) return fail(MOSFHET_HIP_EINVAL, "%s: row_ptr[0] = %d (must be 0)", who, h_row_ptr[0]);
  for (int j = 0; j < rows_out; j++)
    if (h_row_ptr[j + 1] < h_row_ptr[j]) return fail(MOSFHET_HIP_EINVAL, "%s: row_ptr[%d] = %d is below row_ptr[%d] = %d", who, j + 1, h_row_ptr[j + 1], j, h_row_ptr[j]);
  *entries = h_row_ptr[rows_out];
  if (*entries && missing) return fail(MOSFHET_HIP_EINVAL, "%s: null %s", who, missing);
  for (long long q = 0; q < *entries; q++)
    if (h_col[q] < 0 || h_col[q] >= rows_in) return fail(MOSFHET_HIP_EINVAL, "%s: col[%lld] = %d (rows_in = %d)", who, q, h_col[q], rows_in);
  return MOSFHET_HIP_OK;
}

// the lists of a dense map: every column, in order, for every row
static void dense_lists(int rows_out, int rows_in, std::vector<int> &ptr, std::vector<int> &col) {
  ptr.assign((size_t)rows_out + 1, 0);
  col.resize((size_t)rows_out * rows_in);
  for (int j = 0; j < rows_out; j++) {
    ptr[j + 1] = (j + 1) * rows_in;
    for (int i = 0; i < rows_in; i++) col[(size_t)j * rows_in + i] = i;
  }
}

// ---- the device image ----
// Every array of a handle lives in ONE device allocation, read-only after creation (any number of host threads may share the handle).  A handle is this base plus a
// plain struct of scalars, its `Shape`: clone_image copies the shape in one assignment, so a field added to a shape is cloned without anybody remembering it.
constexpr int LINEAR_IMAGE_SLOTS = 10;
struct LinearImage {
  mosfhet_hip_ctx_t ctx = nullptr;   // compared, never read: the context may already be destroyed when the handle is freed or cloned
  int device = 0;
  size_t off[LINEAR_IMAGE_SLOTS] = {}, bytes = 0;   // offsets of the arrays in the image, its size
  char *d = nullptr;
  LinearImage() = default;
  LinearImage(const LinearImage &) = delete;
  LinearImage &operator=(const LinearImage &) = delete;
  ~LinearImage() {
    if (ctx) (void)hipSetDevice(device);
    if (d) (void)hipFree(d);
  }
  template <class T> const T *at(int k) const { return reinterpret_cast<const T *>(d + off[k]); }
};

// lays len[0 .. slots) out (16-byte aligned each) and allocates the image on the device of ctx, which becomes the current one.  The floor of 16 bytes is the LWE
// family's, kept as it was: no handle reaches it (every image holds weights or a row-pointer list), so `bytes` is the plain total in all three families.  Slots
// past `slots` get the end of the image as offset and are never read.
static int image_alloc(LinearImage *h, mosfhet_hip_ctx_t ctx, const size_t *len, int slots) {
  size_t total = 0;
  for (int k = 0; k < LINEAR_IMAGE_SLOTS; k++) { h->off[k] = total; total += k < slots ? (len[k] + 15) & ~(size_t)15 : 0; }
  h->ctx = ctx; h->device = ctx->device; h->bytes = total ? total : 16;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMalloc((void **)&h->d, h->bytes));
  return MOSFHET_HIP_OK;
}

// after the pattern of mosfhet_hip_ksk_clone: a copy of the handle on the device of ctx_other, device to device
template <class H> static int clone_image(const char *who, mosfhet_hip_ctx_t ctx_other, const H *lin, H **out) {
  if (!ctx_other) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx_other", who);
  if (!lin) return fail(MOSFHET_HIP_EINVAL, "%s: null lin", who);
  if (!out) return fail(MOSFHET_HIP_EINVAL, "%s: null out", who);
  HIP_TRY(hipSetDevice(lin->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipSetDevice(ctx_other->device));
  std::unique_ptr<H> h(new H());
  static_cast<typename H::Shape &>(*h) = *lin;
  h->ctx = ctx_other; h->device = ctx_other->device; h->bytes = lin->bytes;
  memcpy(h->off, lin->off, sizeof(h->off));
  HIP_TRY(hipMalloc((void **)&h->d, h->bytes));
  const int rc = copy_across(h->d, ctx_other->device, lin->d, lin->device, h->bytes);
  if (rc) return rc;
  *out = h.release();
  return MOSFHET_HIP_OK;
}

// ---- the two families on packed TRLWE samples ----
// One handle layout for both: cleartext weights leave l = Bg_bit = 0 and know the forms dense and sparse only.
struct PackedShape {
  int rows_out = 0, rows_in = 0, N = 0, l = 0, Bg_bit = 0, form = 0, has_bias = 0;
  long long nnz = -1, entries = 0;
};
struct PackedLinear : LinearImage, PackedShape { using Shape = PackedShape; };
enum { PLIN_W = 0, PLIN_BIAS, PLIN_PTR, PLIN_COL };
enum { PLIN_DENSE = 0, PLIN_SPARSE = 1, PLIN_SELECTORS = 2 };

struct PackedPlan { long long teams, round, rounds, pool_bytes, forwards, inverses, weight_bytes, second_bytes; };

// What tells the families apart.
struct PackedFamily {
  bool gadget;                   // TRGSW weights: l polynomials staged per input component and 4 l per weight, instead of 1 and 1
  int first_teams;               // teams per input of a round's first launch: 2 (one per component) or 1
  int pool;                      // the slot of the calling thread's pool that stages a round
  const char *weights, *staged;  // the nouns of the messages
  const char *clone;             // the clone call that the refusal of a foreign handle names
};
// the body of a family's compute calls after their checks: it fills the launch parameters and goes through packed_linear_rounds
using PackedRun = int (*)(mosfhet_hip_ctx_t, const PackedLinear *, const PackedPlan &, uint64_t *, const uint64_t *, int idx, int count, hipStream_t);

// The one place that decides the shape of a call, for the launchers and for the two plan calls.  `cus` is RESERVED, as in linear_plan: checked, sizes nothing today
// (one team per output sample, a flat grid).  l is read for TRGSW weights only.
static int packed_linear_plan(const char *who, const PackedFamily &f, int N, int l, int rows_out, int rows_in, long long nnz, int count, int extract, int cus,
                              long long workspace, PackedPlan *r) {
  if (!ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (1024, 2048, 4096)", who, N);
  if (f.gadget && (l < 1 || l > 6)) return fail(MOSFHET_HIP_EINVAL, "%s: l = %d (1 .. 6)", who, l);
  if (rows_out < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_out = %d", who, rows_out);
  if (rows_in < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_in = %d", who, rows_in);
  if (nnz < -1 || nnz > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: nnz = %lld (-1 dense, at most 2^31 - 1)", who, nnz);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (extract != 0 && extract != 1) return fail(MOSFHET_HIP_EINVAL, "%s: extract = %d (0 or 1)", who, extract);
  if (cus < 1) return fail(MOSFHET_HIP_EINVAL, "%s: cus = %d", who, cus);
  if (workspace < 0) return fail(MOSFHET_HIP_EINVAL, "%s: workspace_bytes = %lld (0: the current setting)", who, workspace);
  if (workspace == 0) workspace = g_pack_workspace.load(std::memory_order_relaxed);
  const long long entries = nnz < 0 ? (long long)rows_out * rows_in : nnz;
  if (entries > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: rows_out = %d x rows_in = %d %s do not fit 2^31 - 1", who, rows_out, rows_in, f.weights);
  const long long m = f.gadget ? l : 1;                  // polynomials of N / 2 complex staged per input component: its transform, or those of its l digits
  const long long one = (long long)rows_in * 2 * m * N * 8;   // ... of one batch element
  if (one > workspace)
    return fail(MOSFHET_HIP_EINVAL, "%s: the workspace bound of %lld bytes does not hold the %s of one batch element (%lld): mosfhet_hip_set_tlwe_pack_workspace", who,
                workspace, f.staged, one);
  const long long fit = workspace / one;
  r->round = count < fit ? count : fit;
  r->rounds = count ? (count + r->round - 1) / r->round : 0;
  r->teams = r->round * rows_out;
  if (r->teams > 0x7fffffffLL || r->round * rows_in * f.first_teams > 0x7fffffffLL)
    return fail(MOSFHET_HIP_EINVAL, "%s: %lld batch elements x rows_out = %d (or x %srows_in = %d) teams do not fit one launch", who, r->round, rows_out,
                f.first_teams == 2 ? "2 " : "", rows_in);
  r->pool_bytes = r->round * one;
  r->forwards = (long long)count * rows_in * 2 * m;
  r->inverses = (long long)count * rows_out * 2;
  const long long per_team = (entries + rows_out - 1) / rows_out;   // dense: rows_in; sparse: the mean row, rounded up
  r->weight_bytes = per_team * (f.gadget ? 4 * l : 1) * N * 8;
  r->second_bytes = per_team * 2 * m * N * 8;                       // the staged polynomials one team reads: transformed inputs, or digit transforms
  return MOSFHET_HIP_OK;
}

// plan = { teams of the main launch, batch elements per round, rounds, pool bytes per round, forward transforms per call, inverse transforms per call, weight bytes one
//          team reads, input (cleartext weights) or digit (TRGSW weights) bytes one team reads }
static int packed_linear_plan_out(const char *who, const PackedFamily &f, int N, int l, int rows_out, int rows_in, long long nnz, int count, int extract, int cus,
                                  long long workspace, long long plan[8]) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "%s: null plan", who);
  PackedPlan r;
  const int rc = packed_linear_plan(who, f, N, l, rows_out, rows_in, nnz, count, extract, cus, workspace, &r);
  if (rc) return rc;
  plan[0] = r.teams; plan[1] = r.round; plan[2] = r.rounds; plan[3] = r.pool_bytes; plan[4] = r.forwards; plan[5] = r.inverses; plan[6] = r.weight_bytes;
  plan[7] = r.second_bytes;
  return MOSFHET_HIP_OK;
}

// The lists of a creation call: the caller's CSR, checked, or a dense map's.  `missing` as in csr_check (a dense map always has entries).
static int packed_linear_lists(const char *who, const PackedFamily &f, bool sparse, const int *h_row_ptr, const int *h_col, const char *missing, int rows_out, int rows_in,
                               std::vector<int> &ptr, std::vector<int> &col) {
  if (sparse) {
    long long entries;
    const int rc = csr_check(who, h_row_ptr, h_col, rows_out, rows_in, missing, &entries);
    if (rc) return rc;
    ptr.assign(h_row_ptr, h_row_ptr + rows_out + 1);
    col.assign(h_col, h_col + entries);
    return MOSFHET_HIP_OK;
  }
  if (missing) return fail(MOSFHET_HIP_EINVAL, "%s: null %s", who, missing);
  if ((long long)rows_out * rows_in > 0x7fffffffLL)
    return fail(MOSFHET_HIP_EINVAL, "%s: rows_out = %d x rows_in = %d %s do not fit 2^31 - 1", who, rows_out, rows_in, f.weights);
  dense_lists(rows_out, rows_in, ptr, col);
  return MOSFHET_HIP_OK;
}

// The image of a creation call: allocated, lists and bias uploaded; slot PLIN_W (weight_bytes) is left for the family to fill.
static int packed_linear_image(PackedLinear *h, mosfhet_hip_ctx_t ctx, size_t weight_bytes, const uint64_t *h_bias, const std::vector<int> &ptr, const std::vector<int> &col) {
  const size_t len[4] = {weight_bytes, h_bias ? (size_t)h->rows_out * h->N * sizeof(uint64_t) : 0, ptr.size() * sizeof(int), col.size() * sizeof(int)};
  const void *src[4] = {nullptr, h_bias, ptr.data(), col.data()};
  const int rc = image_alloc(h, ctx, len, 4);
  if (rc) return rc;
  for (int k = 1; k < 4; k++)
    if (len[k]) HIP_TRY(hipMemcpy(h->d + h->off[k], src[k], len[k], hipMemcpyHostToDevice));
  return MOSFHET_HIP_OK;
}

// The checks the compute calls share.  Null handles and scalar ranges come before any handle is read and before any HIP call, and so does count == 0 (*run = false:
// nothing to do).  need_out = false: the result goes to the pool, d_out is not this call's to check.
static int packed_linear_check(const char *who, const PackedFamily &f, mosfhet_hip_ctx_t ctx, const PackedLinear *lin, const void *d_out, const void *d_in, int idx,
                               bool extract, int count, bool need_out, PackedPlan *plan, bool *run) {
  *run = false;
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!lin) return fail(MOSFHET_HIP_EINVAL, "%s: null lin", who);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (extract && idx < 0) return fail(MOSFHET_HIP_EINVAL, "%s: idx = %d (0 .. N - 1)", who, idx);
  if (count == 0) return MOSFHET_HIP_OK;
  if ((need_out && !d_out) || !d_in) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  if (extract && idx >= lin->N) return fail(MOSFHET_HIP_EINVAL, "%s: idx = %d (0 .. N - 1 = %d)", who, idx, lin->N - 1);
  if (lin->ctx != ctx) return fail(MOSFHET_HIP_EINVAL, "%s: lin belongs to another context (device %d): %s makes a copy for this one", who, lin->device, f.clone);
  const int rc = packed_linear_plan(who, f, lin->N, lin->l, lin->rows_out, lin->rows_in, lin->nnz, count, extract, 256, 0, plan);
  if (rc) return rc;
  if (need_out) {
    const size_t out_words = extract ? (size_t)lin->N + 1 : (size_t)2 * lin->N;
    if (ranges_overlap(d_out, (size_t)count * lin->rows_out * out_words * sizeof(uint64_t), d_in, (size_t)count * lin->rows_in * 2 * lin->N * sizeof(uint64_t)))
      return fail(MOSFHET_HIP_EINVAL, "%s: d_out overlaps d_in", who);
  }
  *run = true;
  return MOSFHET_HIP_OK;
}

// The loop over the rounds of a call: the pool, then launch(pool, in, out, n) for every n batch elements that fit it -- the family's two launches.
// idx < 0: d_out [count][rows_out][2][N]; else [count][rows_out][N + 1]
template <class Launch>
static int packed_linear_rounds(mosfhet_hip_ctx_t ctx, const PackedFamily &f, const PackedLinear *lin, const PackedPlan &plan, uint64_t *d_out, const uint64_t *d_in, int idx,
                                int count, Launch launch) {
  uint64_t *pool = nullptr;
  const int rc = pool_get(ctx->device, f.pool, (size_t)(plan.pool_bytes / (long long)sizeof(uint64_t)), &pool);
  if (rc) return rc;
  const size_t out_words = idx < 0 ? (size_t)2 * lin->N : (size_t)lin->N + 1;
  for (long long b0 = 0; b0 < count; b0 += plan.round)
    launch(pool, d_in + (size_t)b0 * lin->rows_in * 2 * lin->N, d_out + (size_t)b0 * lin->rows_out * out_words, count - b0 < plan.round ? count - b0 : plan.round);
  return launched();
}

// a compute call that writes the caller's buffer: the TRLWE results (idx = -1), or with `extract` trlwe_extract_tlwe(., idx) of them (src/trlwe.c:540-552), the TRLWE
// results never written
static int packed_linear_call(const char *who, const PackedFamily &f, PackedRun run_rounds, mosfhet_hip_ctx_t ctx, const PackedLinear *lin, uint64_t *d_out, const uint64_t *d_in, int idx, bool extract,
                              int count, void *stream) {
  PackedPlan plan;
  bool run;
  const int rc = packed_linear_check(who, f, ctx, lin, d_out, d_in, idx, extract, count, true, &plan, &run);
  if (rc || !run) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return run_rounds(ctx, lin, plan, d_out, d_in, idx, count, pick(ctx, stream));
}
