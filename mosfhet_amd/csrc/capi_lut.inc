// capi_lut.inc -- leveled look-up-table evaluation for a batch of independent TRGSW-encrypted inputs (leveled_lut_kernels.h): eval_LUT of
// applications/leveled_lut/vertical_packing.c:36-52 for `count` inputs against `tables` shared tables, an entry of a table holding m = 2^pack_log outputs.  Own
// code: the reference application is the specification (which selector halves which level, which mask the rotation takes), nothing of it is compiled in.
//
// Three entry points, one path (lut_plan, launch_leveled_lut, leveled_lut_run):
//   mosfhet_hip_leveled_lut_batch          one table, one output per entry; d_out [count][N + 1]; finishes through lut_cmux_kernel mode 1
//   mosfhet_hip_leveled_lut_tables_batch   `tables` tables, one output per entry; d_out [count][tables][N + 1]
//   mosfhet_hip_leveled_lut_packed_batch   `tables` tables of m adjacent coefficients per entry (CGGI's other packing; the reference's vertical_packing.c:4 points
//                                          at it); d_out [count][tables][m][N + 1]
// A table of 2^size entries is max(1, 2^(size + pack_log) / N) TRLWEs: the tree has max(0, size + pack_log - log2 N) levels over the TOP selectors, the finish
// rotates by m 2^i with selector i for min(size, log2 N - pack_log) steps and extracts coefficients 0 .. m-1.
//
// Launches of one chunk of inputs of one pass of tables: level 0 over (input, table, node) (no forward transform), one launch per deeper tree level over the same
// units, one finishing launch (rotation steps + extraction) over (input, group of tables); in front of a pass's first chunk the preparation of the pass's tables.
// Workspace of a pass of `pass` tables: the prepared rows [pass][nodes][2l][N/2] complex, then the intermediates [chunk][pass][nodes][2][N].  It lives in the
// calling thread's pool (slot POOL_LUT): no allocation and no synchronisation from the second call of a shape on, everything queues on the given stream.

// Workspace bound: the prepared rows and the intermediates of one chunk of inputs of one pass stay within it; a call that needs more is cut into passes of whole
// tables and chunks of whole inputs.  Results do not depend on it.
constexpr long long LUT_WORKSPACE_DEFAULT = 1ll << 30;
static std::atomic<long long> g_lut_workspace{LUT_WORKSPACE_DEFAULT};
constexpr int LUT_MAX_CHUNK = 32768;   // level 0 indexes the inputs of a chunk by gridDim.y

extern "C" int mosfhet_hip_set_leveled_lut_workspace(long long bytes) {
  if (bytes < 0) return fail(MOSFHET_HIP_EINVAL, "set_leveled_lut_workspace: bytes = %lld (0 restores the default)", bytes);
  g_lut_workspace = bytes ? bytes : LUT_WORKSPACE_DEFAULT;
  return MOSFHET_HIP_OK;
}

// Tables per finishing workgroup asked for (0: the default, LUT_GROUP_DEFAULT); what runs is min(that, what the LDS of a CU holds at this ring, the tables of a pass).
// Default 1: see DESIGN 4.11.1 for the measurement behind it.
constexpr int LUT_GROUP_DEFAULT = 1;
static std::atomic<int> g_lut_group{0};

extern "C" int mosfhet_hip_set_leveled_lut_tables_group(int group) {
  if (group < 0 || group > MOSFHET_HIP_LUT_MAX_TABLES) return fail(MOSFHET_HIP_EINVAL, "set_leveled_lut_tables_group: group = %d (0 .. %d, 0 restores the default)", group, MOSFHET_HIP_LUT_MAX_TABLES);
  g_lut_group = group;
  return MOSFHET_HIP_OK;
}

struct LutPlan {
  int levels, nodes, chunk, pass, group, steps, outputs;
  long long table_bytes, input_bytes, bytes;   // of one table's prepared rows, of one input's intermediates on one table, of the workspace
  size_t lut_stride;                           // words from one table to the next
};

// The one place that decides the shape of a call: for the launcher and for the three mosfhet_hip_leveled_lut*_plan functions.  All tables in one pass when one
// input fits beside them (a pass re-reads every selector, a chunk does not); else as many tables per pass as hold one input each, and then the largest chunk.
static int lut_plan(const char *who, int N, int l, int size, int tables, int pack_log, int count, int cus, LutPlan *r) {
  if (tables < 1 || tables > MOSFHET_HIP_LUT_MAX_TABLES) return fail(MOSFHET_HIP_EINVAL, "%s: tables = %d (1 .. %d)", who, tables, MOSFHET_HIP_LUT_MAX_TABLES);
  if (N != 1024 && N != 2048) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (1024, 2048)", who, N);
  if (l < 1 || l > 6) return fail(MOSFHET_HIP_EINVAL, "%s: l = %d (1 .. 6)", who, l);
  const int log_N = ilog2(N);
  if (pack_log < 0 || pack_log > log_N - 1) return fail(MOSFHET_HIP_EINVAL, "%s: pack_log = %d (0 .. log2 N - 1 = %d)", who, pack_log, log_N - 1);
  if (size < 1 || size + pack_log > log_N + MOSFHET_HIP_LUT_MAX_LEVELS)
    return fail(MOSFHET_HIP_EINVAL, "%s: size = %d with pack_log = %d (size >= 1, size + pack_log <= log2 N + %d = %d)", who, size, pack_log, MOSFHET_HIP_LUT_MAX_LEVELS,
                log_N + MOSFHET_HIP_LUT_MAX_LEVELS);
  if (count < 1) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (cus < 1) return fail(MOSFHET_HIP_EINVAL, "%s: cus = %d", who, cus);
  const int rot = log_N - pack_log;
  const long long bound = g_lut_workspace.load(std::memory_order_relaxed);
  r->steps = size < rot ? size : rot;
  r->outputs = tables << pack_log;
  r->levels = size > rot ? size - rot : 0;
  r->nodes = r->levels ? 1 << (r->levels - 1) : 0;
  r->lut_stride = ((size_t)1 << r->levels) * 2 * (size_t)N;
  r->table_bytes = (long long)r->nodes * 2 * l * (N / 2) * (long long)sizeof(d2);
  r->input_bytes = (long long)r->nodes * 2 * N * (long long)sizeof(uint64_t);
  r->chunk = count < LUT_MAX_CHUNK ? count : LUT_MAX_CHUNK;
  r->pass = tables;
  if (r->levels) {
    const long long unit = r->table_bytes + r->input_bytes;
    if (unit > bound)
      return fail(MOSFHET_HIP_EINVAL, "%s: the workspace bound of %lld bytes does not hold the prepared table (%lld) and one input's intermediates (%lld)", who, bound,
                  r->table_bytes, r->input_bytes);
    if ((long long)tables * unit > bound) r->pass = (int)(bound / unit);
    const long long fit = (bound / r->pass - r->table_bytes) / r->input_bytes;
    if (fit < r->chunk) r->chunk = (int)fit;
  }
  r->bytes = (long long)r->pass * (r->table_bytes + (long long)r->chunk * r->input_bytes);
  const int want = g_lut_group.load(std::memory_order_relaxed);
  const int fits = N == 1024 ? lut_tables_max_group<Fft1024>() : lut_tables_max_group<Fft2048>();
  r->group = want ? want : LUT_GROUP_DEFAULT;
  if (r->group > fits) r->group = fits;
  if (r->group > r->pass) r->group = r->pass;
  return MOSFHET_HIP_OK;
}

// plan[0 .. fields): 4 fields for the one-table call, 6 for several tables, 8 for packed tables
static int lut_plan_fields(const char *who, int N, int l, int size, int tables, int pack_log, int count, int cus, long long *plan, int fields) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "%s: null plan", who);
  LutPlan r;
  const int rc = lut_plan(who, N, l, size, tables, pack_log, count, cus, &r);
  if (rc) return rc;
  plan[0] = r.levels; plan[1] = r.nodes; plan[2] = r.chunk;
  if (fields == 4) { plan[3] = r.bytes; return MOSFHET_HIP_OK; }
  plan[3] = r.pass; plan[4] = r.bytes; plan[5] = r.group;
  if (fields == 8) { plan[6] = r.steps; plan[7] = r.outputs; }
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_leveled_lut_plan(int N, int l, int size, int count, int cus, long long *plan) {
  return lut_plan_fields("leveled_lut_plan", N, l, size, 1, 0, count, cus, plan, 4);
}

extern "C" int mosfhet_hip_leveled_lut_tables_plan(int N, int l, int size, int tables, int count, int cus, long long *plan) {
  return lut_plan_fields("leveled_lut_tables_plan", N, l, size, tables, 0, count, cus, plan, 6);
}

extern "C" int mosfhet_hip_leveled_lut_packed_plan(int N, int l, int size, int tables, int pack_log, int count, int cus, long long *plan) {
  return lut_plan_fields("leveled_lut_packed_plan", N, l, size, tables, pack_log, count, cus, plan, 8);
}

// `one`: the one-table call, whose finish is lut_cmux_kernel mode 1 (plan.pass = tables = 1 there); every other call finishes through lut_tables_finish_kernel
template <class F>
static int launch_leveled_lut(const LutPlan &plan, LutParams p, uint64_t *ws, int tables, bool one, int count, int cus, hipStream_t s) {
  const int teams = cus * 8 / (F::THREADS / 64);   // resident capacity at two wavefronts per SIMD: level 0's workgroups (one team each) ...
  const int pairs = teams / 2;                     // ... and the two-team workgroups of lut_cmux_kernel
  const uint64_t *luts = p.lut;
  uint64_t *out = p.out;
  int rc;
  for (int tb0 = 0; tb0 < tables; tb0 += plan.pass) {
    p.tables = tables - tb0 < plan.pass ? tables - tb0 : plan.pass;
    p.group = plan.group < p.tables ? plan.group : p.tables;
    p.lut = luts + (size_t)tb0 * p.lut_stride;
    p.out = out + ((size_t)tb0 << p.pack_log) * (size_t)(F::N + 1);
    p.dtab = reinterpret_cast<d2 *>(ws);
    p.work = ws ? ws + (size_t)p.tables * (size_t)(plan.table_bytes / (long long)sizeof(uint64_t)) : nullptr;
    const int nodes = p.tables * plan.nodes;
    if (plan.levels) {
      p.first = 0; p.inputs = 0;
      hipLaunchKernelGGL(lut_prepare_kernel<F>, dim3((unsigned)(plan.nodes * 2 * p.l), (unsigned)p.tables), dim3(F::THREADS), 0, s, p);
    }
    for (int first = 0; first < count; first += plan.chunk) {
      p.first = first;
      p.inputs = count - first < plan.chunk ? count - first : plan.chunk;
      if (plan.levels) {
        // level 0: a workgroup works for one input; the nodes of an input are cut over as many workgroups as it takes to fill the device
        int slices = (teams + p.inputs - 1) / p.inputs;
        slices = slices < 1 ? 1 : (slices > nodes ? nodes : slices);
        hipLaunchKernelGGL(lut_level0_kernel<F>, dim3((unsigned)slices, (unsigned)p.inputs), dim3(F::THREADS), 0, s, p);
        for (int i = 1; i < plan.levels; i++) {
          p.mode = 0;
          p.half = plan.nodes >> i;
          p.sel_index = p.size - i - 1;
          const size_t units = (size_t)p.inputs * p.tables * p.half;
          if ((rc = launch_dyn_lds(lut_cmux_kernel<F>, dim3((unsigned)(units < (size_t)pairs ? units : (size_t)pairs)), dim3(2 * F::THREADS), lut_cmux_lds<F>(), s, p))) return rc;
        }
      }
      p.mode = 1;
      if (one) {
        rc = launch_dyn_lds(lut_cmux_kernel<F>, dim3((unsigned)p.inputs), dim3(2 * F::THREADS), lut_cmux_lds<F>(), s, p);
      } else {
        const int groups = (p.tables + p.group - 1) / p.group;
        size_t grid = (size_t)p.inputs * groups;
        if (groups > 1) grid = (grid + 7) / 8 * 8;   // dealt over the eight dies' shares: see the kernel
        rc = launch_dyn_lds(lut_tables_finish_kernel<F>, dim3((unsigned)grid), dim3(2 * F::THREADS), lut_tables_finish_lds<F>(p.group), s, p);
      }
      if (rc) return rc;
    }
  }
  return launched();
}

// The body of the three calls (`one` as for the launcher).  Argument checks come before any HIP call.
static int leveled_lut_run(const char *who, mosfhet_hip_ctx_t ctx, uint64_t *d_out, const double *d_sel_dft, const uint64_t *d_luts, int size, int N, int l, int Bg_bit,
                           int tables, int pack_log, bool one, int count, void *stream) {
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (l < 1 || Bg_bit < 1 || Bg_bit > 31 || l * Bg_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "%s: bad gadget l=%d Bg_bit=%d (Bg_bit <= 31, l*Bg_bit < 64)", who, l, Bg_bit);
  LutPlan plan;
  int rc = lut_plan(who, N, l, size, tables, pack_log, count ? count : 1, 256, &plan);
  if (rc) return rc;
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_sel_dft || !d_luts) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  HIP_TRY(hipSetDevice(ctx->device));
  const int cus = device_cus() > 0 ? device_cus() : 256;
  uint64_t *ws = nullptr;
  if (plan.levels && (rc = pool_get(ctx->device, POOL_LUT, (size_t)(plan.bytes / (long long)sizeof(uint64_t)), &ws))) return rc;
  LutParams p;
  p.sel = reinterpret_cast<const d2 *>(d_sel_dft);
  p.lut = d_luts;
  p.dtab = nullptr; p.work = nullptr;   // (per pass: the launcher)
  p.out = d_out;
  p.size = size; p.l = l; p.Bg_bit = Bg_bit;
  p.half0 = plan.nodes;
  p.first = 0; p.inputs = 0; p.mode = 1; p.half = 0; p.sel_index = 0;
  p.steps = plan.steps;
  p.tables = tables; p.out_tables = tables; p.group = plan.group;
  p.lut_stride = plan.lut_stride;
  p.pack_log = pack_log;
  hipStream_t s = pick(ctx, stream);
  if (N == 1024) { p.tw = ctx->tw1024; return launch_leveled_lut<Fft1024>(plan, p, ws, tables, one, count, cus, s); }
  p.tw = ctx->tw2048;
  return launch_leveled_lut<Fft2048>(plan, p, ws, tables, one, count, cus, s);
}

extern "C" int mosfhet_hip_leveled_lut_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const double *d_sel_dft, const uint64_t *d_lut, int size, int N, int l, int Bg_bit,
                                             int count, void *stream) {
  return leveled_lut_run("leveled_lut", ctx, d_out, d_sel_dft, d_lut, size, N, l, Bg_bit, 1, 0, true, count, stream);
}

extern "C" int mosfhet_hip_leveled_lut_tables_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const double *d_sel_dft, const uint64_t *d_luts, int size, int N, int l,
                                                    int Bg_bit, int tables, int count, void *stream) {
  return leveled_lut_run("leveled_lut_tables", ctx, d_out, d_sel_dft, d_luts, size, N, l, Bg_bit, tables, 0, false, count, stream);
}

extern "C" int mosfhet_hip_leveled_lut_packed_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const double *d_sel_dft, const uint64_t *d_luts, int size, int N, int l,
                                                    int Bg_bit, int tables, int pack_log, int count, void *stream) {
  return leveled_lut_run("leveled_lut_packed", ctx, d_out, d_sel_dft, d_luts, size, N, l, Bg_bit, tables, pack_log, false, count, stream);
}
