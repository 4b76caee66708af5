// capi_linear.inc -- cleartext-weight linear layers on batches of LWE samples: y = W x + bias, the reference's tlwe_scale / tlwe_scale_addto / tlwe_scale_subto /
// tlwe_add / tlwe_sub (src/tlwe.c:143-191) with cleartext int64 weights, as ONE call over a batch of independent inferences or circuit instances; dense (a layer)
// and sparse (a netlist level, a convolution, a gather); alone or in front of key switch + bootstrap.  Own code: nothing of the reference is compiled in.
//
//   out[b][j][c] = (c == n ? bias[j] : 0) + sum_i W[j][i] in[b][i][c]   (mod 2^64);   d_in [count][rows_in][n + 1], d_out [count][rows_out][n + 1]
//
// The handle holds the weights on the device, read-only after creation (any number of host threads may share it).  One place decides the shape of a launch
// (linear_plan: for the launcher and for mosfhet_hip_tlwe_linear_plan).  Kernel: linear_kernels.h.
//
// Sparse rows longer than LINEAR_CHUNK entries are cut at creation: chunk q of such a row becomes a list of its own whose sum goes to staging row q, and a second
// list level (weights 1) adds a row's staging rows and its bias.  The second level is not cut again: a row of more than LINEAR_CHUNK^2 = 4096 entries has a
// second-level list of ceil(entries / LINEAR_CHUNK) > LINEAR_CHUNK staging rows, walked by one wavefront (1 / LINEAR_CHUNK of the row's work).  The staging rows [count][parts][n + 1] live in the calling thread's pool (slot POOL_LINEAR), as
// every temporary of this library: a call neither allocates per call nor synchronises, and is capturable on its one stream once a call of the same size has
// grown the pool.
struct LinearShape {
  int rows_out = 0, rows_in = 0, narrow = 0, sparse = 0, has_bias = 0;
  long long nnz = -1;
  int lists = 0, entries = 0;        // sparse, first level: lists (rows and chunks of cut rows) and their entries
  int parts = 0, lists2 = 0, entries2 = 0;   // second level: staging rows, cut rows, entries (= parts)
};
struct mosfhet_hip_linear : LinearImage, LinearShape { using Shape = LinearShape; };   // the image and its clone: capi_linear_common.inc
enum { LIN_W = 0, LIN_BIAS, LIN_PTR, LIN_COL, LIN_VAL, LIN_DST, LIN_PTR2, LIN_COL2, LIN_VAL2, LIN_DST2 };

struct LinearPlan { int sparse, wide; unsigned strips, tiles, units, workgroups, gx, gy; long long passes, bytes; };

// The one place that decides the shape of a launch.  `cus` is RESERVED: it sizes nothing today (every unit is one wavefront of a flat grid); it is checked and kept in
// the signature so that a persistent grid can be sized from it without another ABI.
static int linear_plan(const char *who, int rows_out, int rows_in, long long nnz, int narrow, int n, int count, int cus, LinearPlan *r) {
  if (rows_out < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_out = %d", who, rows_out);
  if (rows_in < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_in = %d", who, rows_in);
  if (nnz < -1 || nnz > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: nnz = %lld (-1 dense, at most 2^31 - 1)", who, nnz);
  if (narrow != 0 && narrow != 1) return fail(MOSFHET_HIP_EINVAL, "%s: narrow = %d (0 or 1)", who, narrow);
  if (n < 1 || n > 65535) return fail(MOSFHET_HIP_EINVAL, "%s: n = %d (1 .. 65535)", who, n);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (cus < 1) return fail(MOSFHET_HIP_EINVAL, "%s: cus = %d", who, cus);
  const long long w = (long long)n + 1, strips = (w + 63) / 64, tiles = ((long long)rows_out + LINEAR_TJ - 1) / LINEAR_TJ;
  const long long units = (long long)count * strips * tiles;
  if (units > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d: count x %lld word strips x %lld row tiles is more than 2^31 - 1 units", who, count, strips, tiles);
  r->sparse = nnz >= 0; r->wide = !narrow;
  r->strips = (unsigned)strips; r->tiles = (unsigned)tiles; r->units = (unsigned)units;
  r->workgroups = (unsigned)((units + 3) / 4);
  r->gy = (r->workgroups + 16383) / 16384;                       // <= 2^31 / 4 / 2^14 = 2^15: within gridDim.y's 65535
  r->gx = r->gy ? (r->workgroups + r->gy - 1) / r->gy : 0;       // <= 16384
  r->passes = tiles;
  // the byte model: count * tiles < 2^31 (above), rows_in < 2^31, w * 8 <= 2^19 -- up to 2^81; refuse what does not fit the plan's signed 64-bit field
  const unsigned __int128 bytes = (unsigned __int128)(tiles * count) * (unsigned __int128)((long long)rows_in * w * 8);
  if (bytes > (unsigned __int128)0x7fffffffffffffffLL)
    return fail(MOSFHET_HIP_EINVAL, "%s: rows_in = %d: %lld passes x count = %d x rows_in x %lld words x 8 bytes do not fit the plan's 64-bit byte count", who, rows_in, tiles, count, w);
  r->bytes = (long long)bytes;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_tlwe_linear_plan(int rows_out, int rows_in, long long nnz, int narrow, int n, int count, int cus, long long plan[8]) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "tlwe_linear_plan: null plan");
  LinearPlan r;
  const int rc = linear_plan("tlwe_linear_plan", rows_out, rows_in, nnz, narrow, n, count, cus, &r);
  if (rc) return rc;
  plan[0] = r.sparse; plan[1] = LINEAR_TJ; plan[2] = 1; plan[3] = r.workgroups; plan[4] = r.gy; plan[5] = r.passes; plan[6] = r.bytes; plan[7] = r.wide;
  return MOSFHET_HIP_OK;
}

static int linear_shape_checks(const char *who, mosfhet_hip_ctx_t ctx, mosfhet_hip_linear_t *out, int rows_out, int rows_in) {
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!out) return fail(MOSFHET_HIP_EINVAL, "%s: null out", who);
  if (rows_out < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_out = %d", who, rows_out);
  if (rows_in < 1) return fail(MOSFHET_HIP_EINVAL, "%s: rows_in = %d", who, rows_in);
  return MOSFHET_HIP_OK;
}

static bool linear_is_narrow(const int64_t *v, size_t count) {
  for (size_t i = 0; i < count; i++)
    if (v[i] < -(1ll << 31) || v[i] >= (1ll << 31)) return false;
  return true;
}

// the image, put together on the host (the padding zero) and uploaded in one copy
static int linear_upload(mosfhet_hip_linear *h, mosfhet_hip_ctx_t ctx, const void *const *src, const size_t *len) {
  const int rc = image_alloc(h, ctx, len, 10);
  if (rc) return rc;
  std::vector<char> image(h->bytes, 0);
  for (int k = 0; k < 10; k++)
    if (len[k]) memcpy(image.data() + h->off[k], src[k], len[k]);
  HIP_TRY(hipMemcpy(h->d, image.data(), h->bytes, hipMemcpyHostToDevice));
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_linear_create_dense(mosfhet_hip_ctx_t ctx, mosfhet_hip_linear_t *out, const int64_t *h_W, const uint64_t *h_bias, int rows_out, int rows_in) {
  int rc = linear_shape_checks("linear_create_dense", ctx, out, rows_out, rows_in);
  if (rc) return rc;
  if (!h_W) return fail(MOSFHET_HIP_EINVAL, "linear_create_dense: null h_W");
  const size_t tiles = ((size_t)rows_out + LINEAR_TJ - 1) / LINEAR_TJ;
  if (tiles * (size_t)rows_in > (size_t)0x7fffffff / LINEAR_TJ) return fail(MOSFHET_HIP_EINVAL, "linear_create_dense: rows_out = %d x rows_in = %d weights do not fit 2^31", rows_out, rows_in);
  std::unique_ptr<mosfhet_hip_linear> h(new mosfhet_hip_linear());
  h->rows_out = rows_out; h->rows_in = rows_in; h->has_bias = h_bias != nullptr;
  h->narrow = linear_is_narrow(h_W, (size_t)rows_out * rows_in);
  h->lists = rows_out;
  std::vector<int64_t> wt(tiles * rows_in * LINEAR_TJ, 0);                    // tile-major: [tile][i][TJ], rows past rows_out stay zero
  for (int j = 0; j < rows_out; j++)
    for (int i = 0; i < rows_in; i++) wt[((size_t)(j / LINEAR_TJ) * rows_in + i) * LINEAR_TJ + j % LINEAR_TJ] = h_W[(size_t)j * rows_in + i];
  const void *src[10] = {wt.data(), h_bias};
  size_t len[10] = {wt.size() * sizeof(int64_t), h_bias ? (size_t)rows_out * sizeof(uint64_t) : 0};
  if ((rc = linear_upload(h.get(), ctx, src, len))) return rc;
  *out = h.release();
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_linear_create_sparse(mosfhet_hip_ctx_t ctx, mosfhet_hip_linear_t *out, const int *h_row_ptr, const int *h_col, const int64_t *h_val,
                                                const uint64_t *h_bias, int rows_out, int rows_in) {
  int rc = linear_shape_checks("linear_create_sparse", ctx, out, rows_out, rows_in);
  if (rc) return rc;
  long long entries;
  if ((rc = csr_check("linear_create_sparse", h_row_ptr, h_col, rows_out, rows_in, !h_col || !h_val ? "h_col or h_val" : nullptr, &entries))) return rc;
  const int nnz = (int)entries;
  std::unique_ptr<mosfhet_hip_linear> h(new mosfhet_hip_linear());
  h->rows_out = rows_out; h->rows_in = rows_in; h->has_bias = h_bias != nullptr; h->sparse = 1; h->nnz = nnz;
  h->narrow = linear_is_narrow(h_val, (size_t)nnz);
  // first level: a row of at most LINEAR_CHUNK entries is one list written to its output row; a longer one is cut into chunks, one staging row each.  The
  // entries keep their order, so col / val are the caller's arrays as they are.
  std::vector<int> ptr{0}, dst, ptr2{0}, col2, dst2;
  for (int j = 0; j < rows_out; j++) {
    const int beg = h_row_ptr[j], end = h_row_ptr[j + 1];
    if (end - beg <= LINEAR_CHUNK) { ptr.push_back(end); dst.push_back(j); continue; }
    for (int q = beg; q < end; q += LINEAR_CHUNK) {
      ptr.push_back(q + LINEAR_CHUNK < end ? q + LINEAR_CHUNK : end);
      dst.push_back(~(int)col2.size());
      col2.push_back((int)col2.size());
    }
    ptr2.push_back((int)col2.size());
    dst2.push_back(j);
  }
  const std::vector<int64_t> val2(col2.size(), 1);
  h->lists = (int)dst.size(); h->entries = nnz; h->parts = (int)col2.size(); h->lists2 = (int)dst2.size(); h->entries2 = (int)col2.size();
  const void *src[10] = {nullptr, h_bias, ptr.data(), h_col, h_val, dst.data(), ptr2.data(), col2.data(), val2.data(), dst2.data()};
  size_t len[10] = {0, h_bias ? (size_t)rows_out * sizeof(uint64_t) : 0, ptr.size() * sizeof(int), (size_t)nnz * sizeof(int), (size_t)nnz * sizeof(int64_t), dst.size() * sizeof(int),
                    h->lists2 ? ptr2.size() * sizeof(int) : 0, col2.size() * sizeof(int), val2.size() * sizeof(int64_t), dst2.size() * sizeof(int)};
  if ((rc = linear_upload(h.get(), ctx, src, len))) return rc;
  *out = h.release();
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_linear_destroy(mosfhet_hip_linear_t lin) {
  delete lin;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_linear_info(mosfhet_hip_linear_t lin, long long info[6]) {
  if (!lin || !info) return fail(MOSFHET_HIP_EINVAL, "linear_info: null %s", lin ? "info" : "lin");
  info[0] = lin->rows_out; info[1] = lin->rows_in; info[2] = lin->nnz; info[3] = lin->narrow; info[4] = (long long)lin->bytes; info[5] = lin->sparse;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_linear_clone(mosfhet_hip_ctx_t ctx_other, mosfhet_hip_linear_t lin, mosfhet_hip_linear_t *out) {
  return clone_image("linear_clone", ctx_other, lin, out);
}

static int linear_launch(const char *who, const LinearParams &p, int n, int count, hipStream_t s) {
  LinearPlan plan;
  const int rc = linear_plan(who, p.lists, p.rows_in, p.sparse ? 0 : -1, p.narrow, n, count, 256, &plan);
  if (rc) return rc;
  LinearParams q = p;
  q.strips = plan.strips; q.tiles = plan.tiles; q.units = plan.units;
  hipLaunchKernelGGL(tlwe_linear_kernel<LINEAR_TJ>, dim3(plan.gx, plan.gy), dim3(256), 0, s, q);
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// the body of the compute call, after the argument checks: one launch, or two when the handle has cut rows
static int linear_run(const char *who, mosfhet_hip_ctx_t ctx, mosfhet_hip_linear_t lin, uint64_t *d_out, const uint64_t *d_in, int n, int count, hipStream_t s) {
  LinearParams p = {};
  p.in = d_in; p.out = d_out; p.bias = lin->has_bias ? lin->at<uint64_t>(LIN_BIAS) : nullptr;
  p.rows_in = lin->rows_in; p.w = n + 1; p.sparse = lin->sparse; p.narrow = lin->narrow; p.lists = lin->lists;
  p.in_rows = (size_t)lin->rows_in; p.out_rows = (size_t)lin->rows_out; p.part_rows = (size_t)lin->parts;
  if (!lin->sparse) {
    p.W = lin->at<int64_t>(LIN_W);
    return linear_launch(who, p, n, count, s);
  }
  p.row_ptr = lin->at<int>(LIN_PTR); p.col = lin->at<int>(LIN_COL); p.val = lin->at<int64_t>(LIN_VAL); p.dst = lin->at<int>(LIN_DST);
  if (!lin->lists2) return linear_launch(who, p, n, count, s);
  uint64_t *part = nullptr;
  int rc = pool_get(ctx->device, POOL_LINEAR, (size_t)count * lin->parts * ((size_t)n + 1), &part);
  if (rc) return rc;
  p.part = part;
  if ((rc = linear_launch(who, p, n, count, s))) return rc;
  // second level: every cut row = the sum of its staging rows (+ bias); narrow (the weights are 1)
  p.in = part; p.in_rows = (size_t)lin->parts; p.rows_in = lin->parts; p.part = nullptr; p.narrow = 1; p.lists = lin->lists2;
  p.row_ptr = lin->at<int>(LIN_PTR2); p.col = lin->at<int>(LIN_COL2); p.val = lin->at<int64_t>(LIN_VAL2); p.dst = lin->at<int>(LIN_DST2);
  return linear_launch(who, p, n, count, s);
}

// Null handles and scalar ranges come before any handle is read and before any HIP call.
extern "C" int mosfhet_hip_tlwe_linear_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_linear_t lin, uint64_t *d_out, const uint64_t *d_in, int n, int count, void *stream) {
  const char *who = "tlwe_linear";
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!lin) return fail(MOSFHET_HIP_EINVAL, "%s: null lin", who);
  if (n < 1 || n > 65535) return fail(MOSFHET_HIP_EINVAL, "%s: n = %d (1 .. 65535)", who, n);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_in) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  if (lin->ctx != ctx) return fail(MOSFHET_HIP_EINVAL, "%s: lin belongs to another context (device %d): mosfhet_hip_linear_clone makes a copy for this one", who, lin->device);
  LinearPlan plan;
  int rc = linear_plan(who, lin->rows_out, lin->rows_in, lin->nnz, lin->narrow, n, count, 256, &plan);   // the size limits, on the whole call
  if (rc) return rc;
  const size_t row = ((size_t)n + 1) * sizeof(uint64_t);
  if (ranges_overlap(d_out, (size_t)count * lin->rows_out * row, d_in, (size_t)count * lin->rows_in * row))
    return fail(MOSFHET_HIP_EINVAL, "%s: d_out overlaps d_in", who);
  HIP_TRY(hipSetDevice(ctx->device));
  return linear_run(who, ctx, lin, d_out, d_in, n, count, pick(ctx, stream));
}

// The linear map into the calling thread's pool (slot POOL_LINEAR_OUT: a slot of its own, so that it collides neither with the key switch's output, which the body
// below keeps in the bootstrap key's scratch, nor with the staging rows of cut sparse rows), then the body of mosfhet_hip_keyswitch_functional_bootstrap_batch on the
// count * rows_out samples.  No bootstrap or key-switch kernel, launcher or kernel choice differs from that call's; the key's product order governs as it does there.
// The pool belongs to the calling host thread and the launches are ordered by its one stream: one stream per host thread, as for every composition here.
extern "C" int mosfhet_hip_linear_keyswitch_functional_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_linear_t lin, mosfhet_hip_ksk_t ksk, mosfhet_hip_bsk_t bsk,
                                                                       uint64_t *d_out, const uint64_t *d_tv, int tv_count, const uint64_t *d_in, int count, int torus_base,
                                                                       int extract, void *stream) {
  const char *who = "linear_keyswitch_bootstrap";
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!lin) return fail(MOSFHET_HIP_EINVAL, "%s: null lin", who);
  if (!ksk) return fail(MOSFHET_HIP_EINVAL, "%s: null ksk", who);
  if (!bsk) return fail(MOSFHET_HIP_EINVAL, "%s: null bsk", who);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_tv || !d_in) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  if (lin->ctx != ctx) return fail(MOSFHET_HIP_EINVAL, "%s: lin belongs to another context (device %d): mosfhet_hip_linear_clone makes a copy for this one", who, lin->device);
  // the checks of the body below on the two keys, BEFORE the linear kernel is queued: it reads ksk->n_in + 1 words per input sample
  int rc = ks_bootstrap_keys_match(who, ksk, bsk);
  if (rc) return rc;
  const int n = ksk->n_in;
  long long samples;
  if ((rc = ks_bootstrap_samples(who, count, lin->rows_out, 0, tv_count, &samples))) return rc;
  LinearPlan plan;
  rc = linear_plan(who, lin->rows_out, lin->rows_in, lin->nnz, lin->narrow, n, count, 256, &plan);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  uint64_t *y = nullptr;
  if ((rc = pool_get(ctx->device, POOL_LINEAR_OUT, (size_t)samples * ((size_t)n + 1), &y))) return rc;
  if ((rc = linear_run(who, ctx, lin, y, d_in, n, count, pick(ctx, stream)))) return rc;
  return mosfhet_hip_keyswitch_functional_bootstrap_batch(ctx, ksk, bsk, d_out, d_tv, tv_count, y, (int)samples, torus_base, extract, stream);
}
