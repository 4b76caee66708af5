// capi_ram.inc -- encrypted memory: cells = 2^size TRLWE samples PER INPUT, read and written at an address given bit by bit as TRGSW_DFT selectors (the leveled
// RAM of the TFHE papers).  Device code: lut_cmux_kernel modes 2 and 3 (leveled_lut_kernels.h).
//   mosfhet_hip_trlwe_ram_read_batch    out[b] = the CMUX tree over mem[b], top address bit first; `size` launches per chunk of inputs, the memory is read only:
//                                       the first level reads the memory and writes the workspace [chunk][cells / 2][2][N], the levels between work in place there,
//                                       the last one writes d_out (size = 1: the memory straight to d_out, no workspace)
//   mosfhet_hip_trlwe_ram_write_batch   every cell of every input: the chain of `size` CMUXes between the cell and val[b], one workgroup per (input, cell), in place;
//                                       one launch, no workspace
// The workspace lives in the calling thread's pool (slot POOL_RAM) under the bound of mosfhet_hip_set_leveled_lut_workspace: no allocation and no synchronisation
// from the second call of a shape on, everything queues on the given stream.

struct RamPlan {
  long long cells, launches, chunk, bytes, products;
};

// The one place that decides the shape of a call: for the launchers and for mosfhet_hip_trlwe_ram_plan.
static int ram_plan(const char *who, int N, int l, int size, int count, int write, int cus, RamPlan *r) {
  if (N != 1024 && N != 2048) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (1024, 2048)", who, N);
  if (l < 1 || l > 6) return fail(MOSFHET_HIP_EINVAL, "%s: l = %d (1 .. 6)", who, l);
  if (size < 1 || size > MOSFHET_HIP_LUT_MAX_LEVELS) return fail(MOSFHET_HIP_EINVAL, "%s: size = %d (1 .. %d)", who, size, MOSFHET_HIP_LUT_MAX_LEVELS);
  if (count < 1) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (cus < 1) return fail(MOSFHET_HIP_EINVAL, "%s: cus = %d", who, cus);
  r->cells = 1ll << size;
  if (write) {
    r->launches = 1; r->chunk = count; r->bytes = 0;
    r->products = (long long)count * r->cells * size;
    return MOSFHET_HIP_OK;
  }
  r->chunk = count;
  r->bytes = 0;
  if (size > 1) {
    const long long bound = g_lut_workspace.load(std::memory_order_relaxed);
    const long long input_bytes = (r->cells / 2) * 2 * N * (long long)sizeof(uint64_t);
    if (input_bytes > bound)
      return fail(MOSFHET_HIP_EINVAL, "%s: the workspace bound of %lld bytes does not hold one input's intermediates (%lld)", who, bound, input_bytes);
    if (bound / input_bytes < r->chunk) r->chunk = bound / input_bytes;
    r->bytes = r->chunk * input_bytes;
  }
  r->launches = (long long)size * ((count + r->chunk - 1) / r->chunk);
  r->products = (long long)count * (r->cells - 1);
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_trlwe_ram_plan(int N, int l, int size, int count, int write, int cus, long long *plan) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "trlwe_ram_plan: null plan");
  RamPlan r;
  const int rc = ram_plan("trlwe_ram_plan", N, l, size, count, write, cus, &r);
  if (rc) return rc;
  plan[0] = r.cells; plan[1] = r.launches; plan[2] = r.chunk; plan[3] = r.bytes; plan[4] = r.products;
  return MOSFHET_HIP_OK;
}

// Argument checks of both calls, before any HIP call.  `other` is d_out (read) or d_val (write): [count][2][N] words.
static int ram_check(const char *who, const char *other_name, mosfhet_hip_ctx_t ctx, const void *other, const double *d_sel_dft, const uint64_t *d_mem, int size, int N,
                     int l, int Bg_bit, int count, int write, RamPlan *plan) {
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (l < 1 || Bg_bit < 1 || Bg_bit > 31 || l * Bg_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "%s: bad gadget l=%d Bg_bit=%d (Bg_bit <= 31, l*Bg_bit < 64)", who, l, Bg_bit);
  const int rc = ram_plan(who, N, l, size, count ? count : 1, write, 256, plan);
  if (rc) return rc;
  if (count == 0) return MOSFHET_HIP_OK;
  if (!other) return fail(MOSFHET_HIP_EINVAL, "%s: null %s", who, other_name);
  if (!d_sel_dft) return fail(MOSFHET_HIP_EINVAL, "%s: null d_sel_dft", who);
  if (!d_mem) return fail(MOSFHET_HIP_EINVAL, "%s: null d_mem", who);
  const size_t sample = (size_t)2 * N * sizeof(uint64_t);
  if (ranges_overlap(other, (size_t)count * sample, d_mem, ((size_t)count << size) * sample))
    return fail(MOSFHET_HIP_EINVAL, "%s: %s overlaps d_mem", who, other_name);
  return MOSFHET_HIP_OK;
}

static LutParams ram_params(const double *d_sel_dft, int size, int l, int Bg_bit) {
  LutParams p = {};
  p.sel = reinterpret_cast<const d2 *>(d_sel_dft);
  p.size = size; p.l = l; p.Bg_bit = Bg_bit;
  p.tables = 1; p.out_tables = 1; p.group = 1;
  return p;
}

template <class F>
static int launch_ram_read(const RamPlan &plan, LutParams p, uint64_t *d_out, const uint64_t *d_mem, uint64_t *ws, int count, int cus, hipStream_t s) {
  const size_t pairs = (size_t)(cus * 8 / (F::THREADS / 64) / 2);   // resident two-team workgroups at two wavefronts per SIMD
  const size_t row = (size_t)2 * F::N, cells = (size_t)plan.cells;
  int rc;
  for (int first = 0; first < count; first += (int)plan.chunk) {
    p.first = first;
    p.inputs = count - first < plan.chunk ? count - first : (int)plan.chunk;
    for (int t = 0; t < p.size; t++) {
      p.mode = 2;
      p.half = 1 << (p.size - 1 - t);
      p.sel_index = p.size - 1 - t;
      if (t == 0) { p.lut = d_mem + (size_t)first * cells * row; p.lut_stride = cells * row; }
      else { p.lut = ws; p.lut_stride = cells / 2 * row; }
      if (t == p.size - 1) { p.out = d_out + (size_t)first * row; p.half0 = 1; }
      else { p.out = ws; p.half0 = (int)(cells / 2); }
      const size_t units = (size_t)p.inputs * p.half;
      if ((rc = launch_dyn_lds(lut_cmux_kernel<F>, dim3((unsigned)(units < pairs ? units : pairs)), dim3(2 * F::THREADS), lut_cmux_lds<F>(), s, p))) return rc;
    }
  }
  return MOSFHET_HIP_OK;
}

template <class F>
static int launch_ram_write(LutParams p, uint64_t *d_mem, const uint64_t *d_val, int count, int cus, hipStream_t s) {
  const size_t pairs = (size_t)(cus * 8 / (F::THREADS / 64) / 2);
  p.mode = 3;
  p.first = 0; p.inputs = count;
  p.lut = d_val;
  p.out = d_mem;
  const size_t units = (size_t)count << p.size;
  return launch_dyn_lds(lut_cmux_kernel<F>, dim3((unsigned)(units < pairs ? units : pairs)), dim3(2 * F::THREADS), lut_cmux_lds<F>(), s, p);
}

extern "C" int mosfhet_hip_trlwe_ram_read_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const double *d_sel_dft, const uint64_t *d_mem, int size, int N, int l, int Bg_bit,
                                                int count, void *stream) {
  RamPlan plan;
  int rc = ram_check("trlwe_ram_read", "d_out", ctx, d_out, d_sel_dft, d_mem, size, N, l, Bg_bit, count, 0, &plan);
  if (rc || count == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const int cus = device_cus() > 0 ? device_cus() : 256;
  uint64_t *ws = nullptr;
  if (plan.bytes && (rc = pool_get(ctx->device, POOL_RAM, (size_t)(plan.bytes / (long long)sizeof(uint64_t)), &ws))) return rc;
  LutParams p = ram_params(d_sel_dft, size, l, Bg_bit);
  hipStream_t s = pick(ctx, stream);
  if (N == 1024) { p.tw = ctx->tw1024; return launch_ram_read<Fft1024>(plan, p, d_out, d_mem, ws, count, cus, s); }
  p.tw = ctx->tw2048;
  return launch_ram_read<Fft2048>(plan, p, d_out, d_mem, ws, count, cus, s);
}

extern "C" int mosfhet_hip_trlwe_ram_write_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_mem, const double *d_sel_dft, const uint64_t *d_val, int size, int N, int l, int Bg_bit,
                                                 int count, void *stream) {
  RamPlan plan;
  const int rc = ram_check("trlwe_ram_write", "d_val", ctx, d_val, d_sel_dft, d_mem, size, N, l, Bg_bit, count, 1, &plan);
  if (rc || count == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const int cus = device_cus() > 0 ? device_cus() : 256;
  LutParams p = ram_params(d_sel_dft, size, l, Bg_bit);
  hipStream_t s = pick(ctx, stream);
  if (N == 1024) { p.tw = ctx->tw1024; return launch_ram_write<Fft1024>(p, d_mem, d_val, count, cus, s); }
  p.tw = ctx->tw2048;
  return launch_ram_write<Fft2048>(p, d_mem, d_val, count, cus, s);
}
