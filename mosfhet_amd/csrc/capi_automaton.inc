// capi_automaton.inc -- weighted deterministic automata (layered branching programs) over words whose symbols are TRGSW_DFT-encrypted bits: the third leveled
// primitive of the TFHE papers next to the look-up table (capi_lut.inc) and the memory (capi_ram.inc).  Device code: lut_cmux_kernel mode 4 (leveled_lut_kernels.h).
//   mosfhet_hip_automaton_create / _destroy / _info   the transition tables [layers][states] x {next0, next1, rot0, rot1} as a handle: checked and packed on the host at
//                                                     creation (no device needed), copied to a device the first time a call runs there
//   mosfhet_hip_trlwe_automaton_batch                 V_steps = init;  V_t[b][q] = R0 + sel[b][t] (.) (R1 - R0) for t = steps-1 .. 0; one launch per step and chunk of
//                                                     inputs: the first reads d_init, the last writes d_out, those between go to and fro between two buffers
//                                                     [chunk][states][2][N] (a step reads ANY row of its source, so it never works in place)
// The buffers live in the calling thread's pool (slot POOL_AUTOMATON) under the bound of mosfhet_hip_set_leveled_lut_workspace: no allocation and no synchronisation
// from the second call of a shape on, everything queues on the given stream.

struct mosfhet_hip_automaton {
  int N = 0, states = 0, layers = 0;
  std::vector<LutStep> table;               // [layers][states]
  std::mutex lock;
  std::map<int, LutStep *> images;          // device -> the table's copy there, made on first use
  ~mosfhet_hip_automaton() {
    for (auto &e : images)
      if (hipSetDevice(e.first) == hipSuccess) (void)hipFree(e.second);
  }
};

struct AutomatonPlan {
  long long launches, chunk, bytes, products, buffers;
};

// The one place that decides the shape of a call: for the launcher and for mosfhet_hip_trlwe_automaton_plan.
static int automaton_plan(const char *who, int N, int l, int states, int layers, int steps, int start, int count, int cus, AutomatonPlan *r) {
  if (N != 1024 && N != 2048) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (1024, 2048)", who, N);
  if (l < 1 || l > 6) return fail(MOSFHET_HIP_EINVAL, "%s: l = %d (1 .. 6)", who, l);
  if (states < 1 || states > MOSFHET_HIP_AUTOMATON_MAX_STATES) return fail(MOSFHET_HIP_EINVAL, "%s: states = %d (1 .. %d)", who, states, MOSFHET_HIP_AUTOMATON_MAX_STATES);
  if (layers < 1 || layers > MOSFHET_HIP_AUTOMATON_MAX_STEPS) return fail(MOSFHET_HIP_EINVAL, "%s: layers = %d (1 .. %d)", who, layers, MOSFHET_HIP_AUTOMATON_MAX_STEPS);
  if (steps < 1 || steps > MOSFHET_HIP_AUTOMATON_MAX_STEPS) return fail(MOSFHET_HIP_EINVAL, "%s: steps = %d (1 .. %d)", who, steps, MOSFHET_HIP_AUTOMATON_MAX_STEPS);
  if (start >= states) return fail(MOSFHET_HIP_EINVAL, "%s: start = %d (negative: every state; else below states = %d)", who, start, states);
  if (count < 1) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (cus < 1) return fail(MOSFHET_HIP_EINVAL, "%s: cus = %d", who, cus);
  r->buffers = steps == 1 ? 0 : steps == 2 ? 1 : 2;
  r->chunk = count;
  r->bytes = 0;
  if (r->buffers) {
    const long long bound = g_lut_workspace.load(std::memory_order_relaxed);
    const long long input_bytes = r->buffers * (long long)states * 2 * N * (long long)sizeof(uint64_t);
    if (input_bytes > bound)
      return fail(MOSFHET_HIP_EINVAL, "%s: the workspace bound of %lld bytes does not hold one input's state vectors (%lld)", who, bound, input_bytes);
    if (bound / input_bytes < r->chunk) r->chunk = bound / input_bytes;
    r->bytes = r->chunk * input_bytes;
  }
  r->launches = (long long)steps * ((count + r->chunk - 1) / r->chunk);
  r->products = (long long)count * ((long long)states * (steps - 1) + (start < 0 ? states : 1));
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_trlwe_automaton_plan(int N, int l, int states, int layers, int steps, int start, int count, int cus, long long *plan) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "trlwe_automaton_plan: null plan");
  AutomatonPlan r;
  const int rc = automaton_plan("trlwe_automaton_plan", N, l, states, layers, steps, start, count, cus, &r);
  if (rc) return rc;
  plan[0] = r.launches; plan[1] = r.chunk; plan[2] = r.bytes; plan[3] = r.products; plan[4] = r.buffers;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_automaton_create(mosfhet_hip_automaton_t *out, const int *h_next0, const int *h_next1, const int *h_rot0, const int *h_rot1, int states, int layers,
                                            int N) {
  const char *who = "automaton_create";
  if (!out) return fail(MOSFHET_HIP_EINVAL, "%s: null out", who);
  if (N != 1024 && N != 2048) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (1024, 2048)", who, N);
  if (states < 1 || states > MOSFHET_HIP_AUTOMATON_MAX_STATES) return fail(MOSFHET_HIP_EINVAL, "%s: states = %d (1 .. %d)", who, states, MOSFHET_HIP_AUTOMATON_MAX_STATES);
  if (layers < 1 || layers > MOSFHET_HIP_AUTOMATON_MAX_STEPS) return fail(MOSFHET_HIP_EINVAL, "%s: layers = %d (1 .. %d)", who, layers, MOSFHET_HIP_AUTOMATON_MAX_STEPS);
  const int *arrays[4] = {h_next0, h_next1, h_rot0, h_rot1};
  const char *names[4] = {"next0", "next1", "rot0", "rot1"};
  for (int k = 0; k < 4; k++)
    if (!arrays[k]) return fail(MOSFHET_HIP_EINVAL, "%s: null h_%s", who, names[k]);
  const size_t entries = (size_t)layers * states;
  for (int k = 0; k < 4; k++) {
    const int top = k < 2 ? states : 2 * N;
    for (size_t i = 0; i < entries; i++)
      if (arrays[k][i] < 0 || arrays[k][i] >= top)
        return fail(MOSFHET_HIP_EINVAL, "%s: %s[%zu][%zu] = %d (0 .. %d)", who, names[k], i / (size_t)states, i % (size_t)states, arrays[k][i], top - 1);
  }
  std::unique_ptr<mosfhet_hip_automaton> h(new mosfhet_hip_automaton());
  h->N = N; h->states = states; h->layers = layers;
  h->table.resize(entries);
  for (size_t i = 0; i < entries; i++) h->table[i] = LutStep{h_next0[i], h_next1[i], h_rot0[i], h_rot1[i]};
  *out = h.release();
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_automaton_destroy(mosfhet_hip_automaton_t automaton) {
  delete automaton;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_automaton_info(mosfhet_hip_automaton_t automaton, long long info[3]) {
  if (!automaton || !info) return fail(MOSFHET_HIP_EINVAL, "automaton_info: null %s", automaton ? "info" : "automaton");
  info[0] = automaton->N; info[1] = automaton->states; info[2] = automaton->layers;
  return MOSFHET_HIP_OK;
}

// a handle's packed table on `device` (the current one): the copy is made by the first call there, synchronously, under the handle's lock, and kept for the handle's
// life (the automaton's transition entries here, the gate records of capi_sellogic.inc)
template <class T>
static int table_image(std::mutex &lock, std::map<int, T *> &images, const std::vector<T> &table, int device, const T **out) {
  std::lock_guard<std::mutex> guard(lock);
  auto it = images.find(device);
  if (it == images.end()) {
    DevBuf image;
    const size_t bytes = table.size() * sizeof(T);
    HIP_TRY(image.alloc(bytes));
    HIP_TRY(hipMemcpy(image.p, table.data(), bytes, hipMemcpyHostToDevice));
    it = images.emplace(device, image.as<T>()).first;
    image.p = nullptr;
  }
  *out = it->second;
  return MOSFHET_HIP_OK;
}

static int automaton_image(mosfhet_hip_automaton_t a, int device, const LutStep **out) { return table_image(a->lock, a->images, a->table, device, out); }

template <class F>
static int launch_automaton(const AutomatonPlan &plan, LutParams p, uint64_t *d_out, const LutStep *image, const uint64_t *d_init, int init_shared, uint64_t *ws, int states,
                            int layers, int steps, int start, int count, int cus, hipStream_t s) {
  const size_t pairs = (size_t)(cus * 8 / (F::THREADS / 64) / 2);   // resident two-team workgroups at two wavefronts per SIMD
  const size_t vec = (size_t)states * 2 * F::N;                     // words of one input's state vector
  const int out_rows = start < 0 ? states : 1;
  int rc;
  p.mode = 4;
  for (int first = 0; first < count; first += (int)plan.chunk) {
    p.first = first;
    p.inputs = count - first < plan.chunk ? count - first : (int)plan.chunk;
    p.lut = init_shared ? d_init : d_init + (size_t)first * vec;
    p.lut_stride = init_shared ? 0 : vec;
    for (int t = steps - 1, k = 0; t >= 0; t--, k++) {
      p.sel_index = t;
      p.dtab = reinterpret_cast<d2 *>(const_cast<LutStep *>(image + (size_t)(t % layers) * states));
      if (t == 0) { p.out = d_out + (size_t)first * out_rows * 2 * F::N; p.half = p.half0 = out_rows; p.steps = start < 0 ? 0 : start; }
      else { p.out = ws + (size_t)(k & 1) * (size_t)plan.chunk * vec; p.half = p.half0 = states; p.steps = 0; }
      const size_t units = (size_t)p.inputs * p.half;
      if ((rc = launch_dyn_lds(lut_cmux_kernel<F>, dim3((unsigned)(units < pairs ? units : pairs)), dim3(2 * F::THREADS), lut_cmux_lds<F>(), s, p))) return rc;
      p.lut = p.out;
      p.lut_stride = vec;
    }
  }
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_trlwe_automaton_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, mosfhet_hip_automaton_t automaton, const double *d_sel_dft, const uint64_t *d_init,
                                                 int init_shared, int steps, int start, int l, int Bg_bit, int count, void *stream) {
  const char *who = "trlwe_automaton";
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!automaton) return fail(MOSFHET_HIP_EINVAL, "%s: null automaton", who);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (l < 1 || Bg_bit < 1 || Bg_bit > 31 || l * Bg_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "%s: bad gadget l=%d Bg_bit=%d (Bg_bit <= 31, l*Bg_bit < 64)", who, l, Bg_bit);
  const int N = automaton->N, states = automaton->states;
  AutomatonPlan plan;
  int rc = automaton_plan(who, N, l, states, automaton->layers, steps, start, count ? count : 1, 256, &plan);
  if (rc || count == 0) return rc;
  if (!d_out) return fail(MOSFHET_HIP_EINVAL, "%s: null d_out", who);
  if (!d_sel_dft) return fail(MOSFHET_HIP_EINVAL, "%s: null d_sel_dft", who);
  if (!d_init) return fail(MOSFHET_HIP_EINVAL, "%s: null d_init", who);
  const size_t sample = (size_t)2 * N * sizeof(uint64_t);
  if (ranges_overlap(d_out, (size_t)count * (start < 0 ? states : 1) * sample, d_init, (size_t)(init_shared ? 1 : count) * states * sample))
    return fail(MOSFHET_HIP_EINVAL, "%s: d_out overlaps d_init", who);
  HIP_TRY(hipSetDevice(ctx->device));
  const int cus = device_cus() > 0 ? device_cus() : 256;
  const LutStep *image = nullptr;
  if ((rc = automaton_image(automaton, ctx->device, &image))) return rc;
  uint64_t *ws = nullptr;
  if (plan.bytes && (rc = pool_get(ctx->device, POOL_AUTOMATON, (size_t)(plan.bytes / (long long)sizeof(uint64_t)), &ws))) return rc;
  LutParams p = ram_params(d_sel_dft, steps, l, Bg_bit);
  hipStream_t s = pick(ctx, stream);
  if (N == 1024) { p.tw = ctx->tw1024; return launch_automaton<Fft1024>(plan, p, d_out, image, d_init, init_shared, ws, states, automaton->layers, steps, start, count, cus, s); }
  p.tw = ctx->tw2048;
  return launch_automaton<Fft2048>(plan, p, d_out, image, d_init, init_shared, ws, states, automaton->layers, steps, start, count, cus, s);
}
