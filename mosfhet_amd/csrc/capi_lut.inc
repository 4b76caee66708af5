// capi_lut.inc -- leveled look-up-table evaluation for a batch of independent TRGSW-encrypted inputs (leveled_lut_kernels.h): eval_LUT of
// applications/leveled_lut/vertical_packing.c:36-52 for `count` inputs against one shared table.  Own code: the reference application is the specification
// (which selector halves which level, which mask the rotation takes), nothing of it is compiled in.
//
// Launches of one chunk of inputs: level 0 (count x first-level nodes units, no forward transform), one launch per deeper tree level, one finishing launch (rotation
// steps + extraction); in front of the first chunk the table preparation, once per call.  The prepared rows and the intermediates live in the calling thread's
// pool (slot POOL_LUT): no allocation and no synchronisation from the second call of a shape on, everything queues on the given stream.

// Workspace bound: the prepared rows [half][2l][N/2] complex plus the intermediates [chunk][half][2][N] of one chunk of inputs stay within it; a batch that
// needs more is cut into chunks of whole inputs.  Results do not depend on it.
constexpr long long LUT_WORKSPACE_DEFAULT = 1ll << 30;
static std::atomic<long long> g_lut_workspace{LUT_WORKSPACE_DEFAULT};
constexpr int LUT_MAX_CHUNK = 32768;   // level 0 indexes the inputs of a chunk by gridDim.y

extern "C" int mosfhet_hip_set_leveled_lut_workspace(long long bytes) {
  if (bytes < 0) return fail(MOSFHET_HIP_EINVAL, "set_leveled_lut_workspace: bytes = %lld (0 restores the default)", bytes);
  g_lut_workspace = bytes ? bytes : LUT_WORKSPACE_DEFAULT;
  return MOSFHET_HIP_OK;
}

struct LutPlan { int levels, nodes, chunk; long long table_bytes, input_bytes, bytes; };

// The one place that decides the shape of a call: for the launcher and for mosfhet_hip_leveled_lut_plan.
static int lut_plan(const char *who, int N, int l, int size, int count, int cus, LutPlan *r) {
  if (N != 1024 && N != 2048) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (1024, 2048)", who, N);
  if (l < 1 || l > 6) return fail(MOSFHET_HIP_EINVAL, "%s: l = %d (1 .. 6)", who, l);
  const int log_N = ilog2(N);
  if (size < 1 || size > log_N + MOSFHET_HIP_LUT_MAX_LEVELS)
    return fail(MOSFHET_HIP_EINVAL, "%s: size = %d (1 .. log2 N + %d = %d selector bits)", who, size, MOSFHET_HIP_LUT_MAX_LEVELS, log_N + MOSFHET_HIP_LUT_MAX_LEVELS);
  if (count < 1) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (cus < 1) return fail(MOSFHET_HIP_EINVAL, "%s: cus = %d", who, cus);
  r->levels = size > log_N ? size - log_N : 0;
  r->nodes = r->levels ? 1 << (r->levels - 1) : 0;
  r->table_bytes = (long long)r->nodes * 2 * l * (N / 2) * (long long)sizeof(d2);
  r->input_bytes = (long long)r->nodes * 2 * N * (long long)sizeof(uint64_t);
  r->chunk = count < LUT_MAX_CHUNK ? count : LUT_MAX_CHUNK;
  if (r->levels) {
    const long long bound = g_lut_workspace.load(std::memory_order_relaxed);
    if (r->table_bytes + r->input_bytes > bound)
      return fail(MOSFHET_HIP_EINVAL, "%s: the workspace bound of %lld bytes does not hold the prepared table (%lld) and one input's intermediates (%lld)", who, bound,
                  r->table_bytes, r->input_bytes);
    const long long fit = (bound - r->table_bytes) / r->input_bytes;
    if (fit < r->chunk) r->chunk = (int)fit;
  }
  r->bytes = r->table_bytes + (long long)r->chunk * r->input_bytes;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_leveled_lut_plan(int N, int l, int size, int count, int cus, long long *plan) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "leveled_lut_plan: null plan");
  LutPlan r;
  const int rc = lut_plan("leveled_lut_plan", N, l, size, count, cus, &r);
  if (rc) return rc;
  plan[0] = r.levels; plan[1] = r.nodes; plan[2] = r.chunk; plan[3] = r.bytes;
  return MOSFHET_HIP_OK;
}

template <class F>
static int launch_leveled_lut(const LutPlan &plan, LutParams p, int count, int cus, hipStream_t s) {
  const int teams = cus * 8 / (F::THREADS / 64);   // resident capacity at two wavefronts per SIMD: level 0's workgroups (one team each) ...
  const int pairs = teams / 2;                     // ... and the two-team workgroups of lut_cmux_kernel
  int rc;
  if (plan.levels) {
    p.first = 0; p.inputs = 0;
    hipLaunchKernelGGL(lut_prepare_kernel<F>, dim3((unsigned)(plan.nodes * 2 * p.l), 1), dim3(F::THREADS), 0, s, p);
  }
  for (int first = 0; first < count; first += plan.chunk) {
    p.first = first;
    p.inputs = count - first < plan.chunk ? count - first : plan.chunk;
    if (plan.levels) {
      // level 0: a workgroup works for one input; the nodes of an input are cut over as many workgroups as it takes to fill the device
      int slices = (teams + p.inputs - 1) / p.inputs;
      slices = slices < 1 ? 1 : (slices > plan.nodes ? plan.nodes : slices);
      hipLaunchKernelGGL(lut_level0_kernel<F>, dim3((unsigned)slices, (unsigned)p.inputs), dim3(F::THREADS), 0, s, p);
      for (int i = 1; i < plan.levels; i++) {
        p.mode = 0;
        p.half = plan.nodes >> i;
        p.sel_index = p.size - i - 1;
        const size_t units = (size_t)p.inputs * p.half;
        if ((rc = launch_dyn_lds(lut_cmux_kernel<F>, dim3((unsigned)(units < (size_t)pairs ? units : (size_t)pairs)), dim3(2 * F::THREADS), lut_cmux_lds<F>(), s, p))) return rc;
      }
    }
    p.mode = 1;
    if ((rc = launch_dyn_lds(lut_cmux_kernel<F>, dim3((unsigned)p.inputs), dim3(2 * F::THREADS), lut_cmux_lds<F>(), s, p))) return rc;
  }
  return launched();
}

extern "C" int mosfhet_hip_leveled_lut_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const double *d_sel_dft, const uint64_t *d_lut, int size, int N, int l, int Bg_bit,
                                             int count, void *stream) {
  // (argument checks come before any HIP call)
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "leveled_lut: null ctx");
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "leveled_lut: count = %d", count);
  if (l < 1 || Bg_bit < 1 || Bg_bit > 31 || l * Bg_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "leveled_lut: bad gadget l=%d Bg_bit=%d (Bg_bit <= 31, l*Bg_bit < 64)", l, Bg_bit);
  LutPlan plan;
  int rc = lut_plan("leveled_lut", N, l, size, count ? count : 1, 256, &plan);
  if (rc) return rc;
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_sel_dft || !d_lut) return fail(MOSFHET_HIP_EINVAL, "leveled_lut: null buffer");
  HIP_TRY(hipSetDevice(ctx->device));
  const int cus = device_cus() > 0 ? device_cus() : 256;
  uint64_t *ws = nullptr;
  if (plan.levels && (rc = pool_get(ctx->device, POOL_LUT, (size_t)(plan.bytes / (long long)sizeof(uint64_t)), &ws))) return rc;
  LutParams p;
  p.sel = reinterpret_cast<const d2 *>(d_sel_dft);
  p.lut = d_lut;
  p.dtab = reinterpret_cast<d2 *>(ws);
  p.work = ws ? ws + plan.table_bytes / (long long)sizeof(uint64_t) : nullptr;
  p.out = d_out;
  p.size = size; p.l = l; p.Bg_bit = Bg_bit;
  p.half0 = plan.nodes;
  p.first = 0; p.inputs = 0; p.mode = 1; p.half = 0; p.sel_index = 0;
  p.steps = size < ilog2(N) ? size : ilog2(N);
  p.tables = 1; p.out_tables = 1; p.group = 1; p.lut_stride = 0; p.pack_log = 0;
  hipStream_t s = pick(ctx, stream);
  if (N == 1024) { p.tw = ctx->tw1024; return launch_leveled_lut<Fft1024>(plan, p, count, cus, s); }
  p.tw = ctx->tw2048;
  return launch_leveled_lut<Fft2048>(plan, p, count, cus, s);
}

// ---------------------------------------------------------------- several tables over the same selectors ----------------------------------------------------------------
// mosfhet_hip_leveled_lut_tables_batch: `tables` shared tables on every input, d_out [count][tables][N + 1].  Launches of one chunk of one pass: level 0 over
// (input, table, node), one launch per deeper level over the same units, lut_tables_finish_kernel over (input, group of tables); in front of a pass's first chunk
// the preparation of the pass's tables.  Workspace of a pass of `pass` tables: the prepared rows [pass][nodes][2l][N/2] complex, then the intermediates
// [chunk][pass][nodes][2][N] -- within the bound of the one-table call.

// Tables per finishing workgroup asked for (0: the default, LUT_GROUP_DEFAULT); what runs is min(that, what the LDS of a CU holds at this ring, the tables of a pass).
// Default 1: see DESIGN 4.11.1 for the measurement behind it.
constexpr int LUT_GROUP_DEFAULT = 1;
static std::atomic<int> g_lut_group{0};

extern "C" int mosfhet_hip_set_leveled_lut_tables_group(int group) {
  if (group < 0 || group > MOSFHET_HIP_LUT_MAX_TABLES) return fail(MOSFHET_HIP_EINVAL, "set_leveled_lut_tables_group: group = %d (0 .. %d, 0 restores the default)", group, MOSFHET_HIP_LUT_MAX_TABLES);
  g_lut_group = group;
  return MOSFHET_HIP_OK;
}

struct LutTablesPlan { int levels, nodes, chunk, pass, group; long long table_bytes, input_bytes, bytes; };

// The one place that decides the shape of a several-table call: for the launcher and for mosfhet_hip_leveled_lut_tables_plan.  All tables in one pass when one input
// fits beside them (a pass re-reads every selector, a chunk does not); else as many tables per pass as hold one input each, and then the largest chunk.
// The arithmetic of a several-table shape at a given number of tree levels (shared with the packed call, whose levels are not those of `size` alone).
// nodes, table_bytes, input_bytes and the refusal are lut_plan's formulas at `levels` and MUST stay equal to them: lut_tables_plan runs lut_plan first (its
// checks and its refusal, which therefore never fires here on that path) and then this with lut_plan's levels; test_tables_plan_sweep and test_packed_plan_sweep
// (pack_log = 0 against leveled_lut_tables_plan, tables = 1 against leveled_lut_plan) hold the two together.  The refusal here is the packed call's.
static int lut_tables_shape(const char *who, int N, int l, int levels, int tables, int count, LutTablesPlan *r) {
  const long long bound = g_lut_workspace.load(std::memory_order_relaxed);
  r->levels = levels;
  r->nodes = levels ? 1 << (levels - 1) : 0;
  r->table_bytes = (long long)r->nodes * 2 * l * (N / 2) * (long long)sizeof(d2);
  r->input_bytes = (long long)r->nodes * 2 * N * (long long)sizeof(uint64_t);
  if (levels && r->table_bytes + r->input_bytes > bound)
    return fail(MOSFHET_HIP_EINVAL, "%s: the workspace bound of %lld bytes does not hold the prepared table (%lld) and one input's intermediates (%lld)", who, bound,
                r->table_bytes, r->input_bytes);
  r->chunk = count < LUT_MAX_CHUNK ? count : LUT_MAX_CHUNK;
  r->pass = tables;
  if (r->levels) {
    const long long unit = r->table_bytes + r->input_bytes;
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

static int lut_tables_plan(const char *who, int N, int l, int size, int tables, int count, int cus, LutTablesPlan *r) {
  if (tables < 1 || tables > MOSFHET_HIP_LUT_MAX_TABLES) return fail(MOSFHET_HIP_EINVAL, "%s: tables = %d (1 .. %d)", who, tables, MOSFHET_HIP_LUT_MAX_TABLES);
  LutPlan one;
  int rc = lut_plan(who, N, l, size, count, cus, &one);   // the argument checks, and the refusal when one table with one input does not fit
  if (rc) return rc;
  return lut_tables_shape(who, N, l, one.levels, tables, count, r);
}

extern "C" int mosfhet_hip_leveled_lut_tables_plan(int N, int l, int size, int tables, int count, int cus, long long *plan) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "leveled_lut_tables_plan: null plan");
  LutTablesPlan r;
  const int rc = lut_tables_plan("leveled_lut_tables_plan", N, l, size, tables, count, cus, &r);
  if (rc) return rc;
  plan[0] = r.levels; plan[1] = r.nodes; plan[2] = r.chunk; plan[3] = r.pass; plan[4] = r.bytes; plan[5] = r.group;
  return MOSFHET_HIP_OK;
}

template <class F>
static int launch_leveled_lut_tables(const LutTablesPlan &plan, LutParams p, uint64_t *ws, int tables, int count, int cus, hipStream_t s) {
  const int teams = cus * 8 / (F::THREADS / 64), pairs = teams / 2;   // (as launch_leveled_lut)
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
      const int groups = (p.tables + p.group - 1) / p.group;
      size_t grid = (size_t)p.inputs * groups;
      if (groups > 1) grid = (grid + 7) / 8 * 8;   // dealt over the eight dies' shares: see the kernel
      if ((rc = launch_dyn_lds(lut_tables_finish_kernel<F>, dim3((unsigned)grid), dim3(2 * F::THREADS), lut_tables_finish_lds<F>(p.group), s, p))) return rc;
    }
  }
  return launched();
}

extern "C" int mosfhet_hip_leveled_lut_tables_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const double *d_sel_dft, const uint64_t *d_luts, int size, int N, int l,
                                                    int Bg_bit, int tables, int count, void *stream) {
  // (argument checks come before any HIP call)
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "leveled_lut_tables: null ctx");
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "leveled_lut_tables: count = %d", count);
  if (l < 1 || Bg_bit < 1 || Bg_bit > 31 || l * Bg_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "leveled_lut_tables: bad gadget l=%d Bg_bit=%d (Bg_bit <= 31, l*Bg_bit < 64)", l, Bg_bit);
  LutTablesPlan plan;
  int rc = lut_tables_plan("leveled_lut_tables", N, l, size, tables, count ? count : 1, 256, &plan);
  if (rc) return rc;
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_sel_dft || !d_luts) return fail(MOSFHET_HIP_EINVAL, "leveled_lut_tables: null buffer");
  HIP_TRY(hipSetDevice(ctx->device));
  const int cus = device_cus() > 0 ? device_cus() : 256;
  uint64_t *ws = nullptr;
  if (plan.levels && (rc = pool_get(ctx->device, POOL_LUT, (size_t)(plan.bytes / (long long)sizeof(uint64_t)), &ws))) return rc;
  const int log_N = ilog2(N);
  LutParams p;
  p.sel = reinterpret_cast<const d2 *>(d_sel_dft);
  p.lut = d_luts;
  p.dtab = nullptr; p.work = nullptr;
  p.out = d_out;
  p.size = size; p.l = l; p.Bg_bit = Bg_bit;
  p.half0 = plan.nodes;
  p.first = 0; p.inputs = 0; p.mode = 1; p.half = 0; p.sel_index = 0;
  p.steps = size < log_N ? size : log_N;
  p.tables = tables; p.out_tables = tables; p.group = plan.group;
  p.lut_stride = (size_t)(size > log_N ? 1 << (size - log_N) : 1) * 2 * (size_t)N;
  p.pack_log = 0;
  hipStream_t s = pick(ctx, stream);
  if (N == 1024) { p.tw = ctx->tw1024; return launch_leveled_lut_tables<Fft1024>(plan, p, ws, tables, count, cus, s); }
  p.tw = ctx->tw2048;
  return launch_leveled_lut_tables<Fft2048>(plan, p, ws, tables, count, cus, s);
}

// ---------------------------------------------------------------- several outputs packed into one table ----------------------------------------------------------------
// mosfhet_hip_leveled_lut_packed_batch: an entry of a table is m = 2^pack_log adjacent coefficients, the m output bits of that entry (CGGI's other packing;
// the reference's vertical_packing.c:4 points at it).  A table of 2^size entries is max(1, 2^(size + pack_log) / N) TRLWEs: the tree has
// max(0, size + pack_log - log2 N) levels over the TOP selectors, the finish rotates by m 2^i with selector i for min(size, log2 N - pack_log) steps and extracts
// coefficients 0 .. m-1.  The launches are those of the several-table call with this plan; d_out is [count][tables][m][N + 1].

struct LutPackedPlan { LutTablesPlan t; int steps, outputs; };

// The one place that decides the shape of a packed call: for the launcher and for mosfhet_hip_leveled_lut_packed_plan.
static int lut_packed_plan(const char *who, int N, int l, int size, int tables, int pack_log, int count, int cus, LutPackedPlan *r) {
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
  r->steps = size < rot ? size : rot;
  r->outputs = tables << pack_log;
  return lut_tables_shape(who, N, l, size > rot ? size - rot : 0, tables, count, &r->t);
}

extern "C" int mosfhet_hip_leveled_lut_packed_plan(int N, int l, int size, int tables, int pack_log, int count, int cus, long long *plan) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "leveled_lut_packed_plan: null plan");
  LutPackedPlan r;
  const int rc = lut_packed_plan("leveled_lut_packed_plan", N, l, size, tables, pack_log, count, cus, &r);
  if (rc) return rc;
  plan[0] = r.t.levels; plan[1] = r.t.nodes; plan[2] = r.t.chunk; plan[3] = r.t.pass; plan[4] = r.t.bytes; plan[5] = r.t.group;
  plan[6] = r.steps; plan[7] = r.outputs;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_leveled_lut_packed_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const double *d_sel_dft, const uint64_t *d_luts, int size, int N, int l,
                                                    int Bg_bit, int tables, int pack_log, int count, void *stream) {
  // (argument checks come before any HIP call)
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "leveled_lut_packed: null ctx");
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "leveled_lut_packed: count = %d", count);
  if (l < 1 || Bg_bit < 1 || Bg_bit > 31 || l * Bg_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "leveled_lut_packed: bad gadget l=%d Bg_bit=%d (Bg_bit <= 31, l*Bg_bit < 64)", l, Bg_bit);
  LutPackedPlan plan;
  int rc = lut_packed_plan("leveled_lut_packed", N, l, size, tables, pack_log, count ? count : 1, 256, &plan);
  if (rc) return rc;
  if (pack_log == 0) return mosfhet_hip_leveled_lut_tables_batch(ctx, d_out, d_sel_dft, d_luts, size, N, l, Bg_bit, tables, count, stream);   // one output per entry: that call
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_sel_dft || !d_luts) return fail(MOSFHET_HIP_EINVAL, "leveled_lut_packed: null buffer");
  HIP_TRY(hipSetDevice(ctx->device));
  const int cus = device_cus() > 0 ? device_cus() : 256;
  uint64_t *ws = nullptr;
  if (plan.t.levels && (rc = pool_get(ctx->device, POOL_LUT, (size_t)(plan.t.bytes / (long long)sizeof(uint64_t)), &ws))) return rc;
  LutParams p;
  p.sel = reinterpret_cast<const d2 *>(d_sel_dft);
  p.lut = d_luts;
  p.dtab = nullptr; p.work = nullptr;
  p.out = d_out;
  p.size = size; p.l = l; p.Bg_bit = Bg_bit;
  p.half0 = plan.t.nodes;
  p.first = 0; p.inputs = 0; p.mode = 1; p.half = 0; p.sel_index = 0;
  p.steps = plan.steps;
  p.tables = tables; p.out_tables = tables; p.group = plan.t.group;
  p.lut_stride = ((size_t)1 << plan.t.levels) * 2 * (size_t)N;
  p.pack_log = pack_log;
  hipStream_t s = pick(ctx, stream);
  if (N == 1024) { p.tw = ctx->tw1024; return launch_leveled_lut_tables<Fft1024>(plan.t, p, ws, tables, count, cus, s); }
  p.tw = ctx->tw2048;
  return launch_leveled_lut_tables<Fft2048>(plan.t, p, ws, tables, count, cus, s);
}
