// capi_sellogic.inc -- selector logic: circuits of gates over TRGSW_DFT selectors, computed on the device from selectors (include/mosfhet_hip.h has the definition;
// the reference's trgsw_mul_DFT2, src/trgsw.c:425-442, is the AND gate).  Own code: nothing of the reference is compiled in.  Device code: sel_gate_body,
// trace_conversions_kernel kind 7 (trace_kernels.h).
//   mosfhet_hip_sellogic_create / _destroy / _info   the gate list [n_gates][4] = {op, x, y, z} as a handle: checked, levelled and packed on the host at creation (no
//                                                    device needed), copied to a device the first time a call runs there (table_image, capi_automaton.inc)
//   mosfhet_hip_trgsw_logic_batch                    one launch per level and chunk of batch elements, teams = chunk x gates of the level x 2l; every gate's output is a
//                                                    row of d_out_dft, which later levels read: no pool, no workspace, nothing but launches on the given stream
//   mosfhet_hip_trgsw_logic_plan                     the shape of a call as a pure function, shared with the launcher (sellogic_plan)

struct mosfhet_hip_sellogic {
  int N = 0, n_in = 0, n_gates = 0, levels = 0, widest = 0, product_gates = 0;
  std::vector<SelGate> table;               // the gates sorted by level, op_row = op | (gate index << 4)
  std::vector<int> first;                   // [levels + 1]: level v is table[first[v]] .. table[first[v + 1] - 1]
  std::mutex lock;
  std::map<int, SelGate *> images;          // device -> the table's copy there, made on first use
  ~mosfhet_hip_sellogic() {
    for (auto &e : images)
      if (hipSetDevice(e.first) == hipSuccess) (void)hipFree(e.second);
  }
};

// Teams of one launch at most: 2^24 teams of up to 256 threads stay below 2^32 threads, the limit of a launch.
static const long long SELLOGIC_GRID_TEAMS = 1LL << 24;

struct SelLogicPlan { long long launches, teams, products, inverses, forwards, chunk; };

// The one place that decides the shape of a call: for the launcher and for mosfhet_hip_trgsw_logic_plan.  Every level runs over the same chunks of whole batch
// elements, sized so that the widest level's launch fits one grid.  `cus` is RESERVED, as in gswlinear_plan: checked, sizes nothing today (one team per row, a flat grid).
static int sellogic_plan(const char *who, int N, int l, int n_in, int n_gates, int levels, int widest, int count, int cus, SelLogicPlan *r) {
  if (N != 1024 && N != 2048) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (1024, 2048)", who, N);
  if (l < 1 || l > 6) return fail(MOSFHET_HIP_EINVAL, "%s: l = %d (1 .. 6)", who, l);
  if (n_in < 1 || n_in > MOSFHET_HIP_SELLOGIC_MAX_WIRES) return fail(MOSFHET_HIP_EINVAL, "%s: n_in = %d (1 .. %d)", who, n_in, MOSFHET_HIP_SELLOGIC_MAX_WIRES);
  if (n_gates < 1 || n_gates > MOSFHET_HIP_SELLOGIC_MAX_WIRES) return fail(MOSFHET_HIP_EINVAL, "%s: n_gates = %d (1 .. %d)", who, n_gates, MOSFHET_HIP_SELLOGIC_MAX_WIRES);
  if (levels < 1 || levels > n_gates) return fail(MOSFHET_HIP_EINVAL, "%s: levels = %d (1 .. n_gates = %d)", who, levels, n_gates);
  if (widest < (n_gates + levels - 1) / levels || widest > n_gates - (levels - 1))
    return fail(MOSFHET_HIP_EINVAL, "%s: widest_level = %d (%d gates in %d levels: %d .. %d)", who, widest, n_gates, levels, (n_gates + levels - 1) / levels, n_gates - (levels - 1));
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (cus < 1) return fail(MOSFHET_HIP_EINVAL, "%s: cus = %d", who, cus);
  const long long per_element = (long long)widest * 2 * l, fit = SELLOGIC_GRID_TEAMS / per_element;   // >= 341
  r->chunk = count < fit ? count : fit;
  r->launches = count ? (long long)levels * ((count + r->chunk - 1) / r->chunk) : 0;
  r->teams = r->chunk * per_element;
  const long long rows = (long long)count * n_gates * 2 * l;   // teams of the whole call
  r->products = rows;
  r->inverses = rows * 4;
  r->forwards = rows * (2 * l + 2);
  return MOSFHET_HIP_OK;
}

// plan = { launches, teams of the widest launch, external products, inverse transforms, forward transforms }; the last three are those of a circuit whose n_gates gates
// are all AND gates (one product of 2l digit transforms, the row of x inverted, the product inverted, the result transformed): a handle's own product count is
// count x 2l x info[4]
extern "C" int mosfhet_hip_trgsw_logic_plan(int N, int l, int n_in, int n_gates, int levels, int widest_level, int count, int cus, long long *plan) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "trgsw_logic_plan: null plan");
  SelLogicPlan r;
  const int rc = sellogic_plan("trgsw_logic_plan", N, l, n_in, n_gates, levels, widest_level, count, cus, &r);
  if (rc) return rc;
  plan[0] = r.launches; plan[1] = r.teams; plan[2] = r.products; plan[3] = r.inverses; plan[4] = r.forwards;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_sellogic_create(mosfhet_hip_sellogic_t *out, const int *h_gates, int n_gates, int n_in, int N) {
  const char *who = "sellogic_create";
  static const char *const names[SEL_OPS] = {"NOT", "AND", "NAND", "OR", "NOR", "XOR", "XNOR", "ANDNOT", "MUX"};
  if (!out) return fail(MOSFHET_HIP_EINVAL, "%s: null out", who);
  if (!h_gates) return fail(MOSFHET_HIP_EINVAL, "%s: null h_gates", who);
  if (N != 1024 && N != 2048) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (1024, 2048)", who, N);
  if (n_in < 1 || n_in > MOSFHET_HIP_SELLOGIC_MAX_WIRES) return fail(MOSFHET_HIP_EINVAL, "%s: n_in = %d (1 .. %d)", who, n_in, MOSFHET_HIP_SELLOGIC_MAX_WIRES);
  if (n_gates < 1 || n_gates > MOSFHET_HIP_SELLOGIC_MAX_WIRES) return fail(MOSFHET_HIP_EINVAL, "%s: n_gates = %d (1 .. %d)", who, n_gates, MOSFHET_HIP_SELLOGIC_MAX_WIRES);
  std::vector<int> level((size_t)n_gates);
  int levels = 0, product_gates = 0;
  for (int g = 0; g < n_gates; g++) {
    const int *e = h_gates + (size_t)4 * g, op = e[0];
    if (op < 0 || op >= SEL_OPS) return fail(MOSFHET_HIP_EINVAL, "%s: gates[%d].op = %d (0 .. %d)", who, g, op, SEL_OPS - 1);
    const int used = op == SEL_NOT ? 1 : op == SEL_MUX ? 3 : 2;
    int lv = 0;
    for (int k = 1; k <= 3; k++) {
      const int w = e[k];
      const char field = "?xyz"[k];
      if (k > used) {
        if (w != -1) return fail(MOSFHET_HIP_EINVAL, "%s: gates[%d].%c = %d, a field %s does not use (must be -1)", who, g, field, w, names[op]);
        continue;
      }
      if (w < 0 || w >= n_in + g)
        return fail(MOSFHET_HIP_EINVAL, "%s: gates[%d].%c = %d (a wire below n_in + %d = %d: an input or an earlier gate)", who, g, field, w, g, n_in + g);
      const int wl = w < n_in ? 0 : level[(size_t)(w - n_in)];
      if (wl > lv) lv = wl;
    }
    level[(size_t)g] = lv + 1;
    if (lv + 1 > levels) levels = lv + 1;
    product_gates += op != SEL_NOT;
  }
  std::unique_ptr<mosfhet_hip_sellogic> h(new mosfhet_hip_sellogic());
  h->N = N; h->n_in = n_in; h->n_gates = n_gates; h->levels = levels; h->product_gates = product_gates;
  h->first.assign((size_t)levels + 1, 0);
  for (int g = 0; g < n_gates; g++) h->first[(size_t)level[(size_t)g]]++;   // first[v + 1] = gates of level v (levels count from 1 here)
  for (int v = 0; v < levels; v++) {
    if (h->first[(size_t)v + 1] > h->widest) h->widest = h->first[(size_t)v + 1];
    h->first[(size_t)v + 1] += h->first[(size_t)v];
  }
  h->table.resize((size_t)n_gates);
  std::vector<int> next(h->first.begin(), h->first.end() - 1);
  for (int g = 0; g < n_gates; g++) {
    const int *e = h_gates + (size_t)4 * g;
    h->table[(size_t)next[(size_t)level[(size_t)g] - 1]++] = SelGate{e[0] | (g << 4), e[1], e[2], e[3]};
  }
  *out = h.release();
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_sellogic_destroy(mosfhet_hip_sellogic_t c) {
  delete c;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_sellogic_info(mosfhet_hip_sellogic_t c, long long info[5]) {
  if (!c || !info) return fail(MOSFHET_HIP_EINVAL, "sellogic_info: null %s", c ? "info" : "circuit");
  info[0] = c->N; info[1] = c->n_in; info[2] = c->n_gates; info[3] = c->levels; info[4] = c->product_gates;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_trgsw_logic_batch(mosfhet_hip_ctx_t ctx, double *d_out_dft, mosfhet_hip_sellogic_t c, const double *d_in_dft, int l, int Bg_bit, int count,
                                             void *stream) {
  const char *who = "trgsw_logic";
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!c) return fail(MOSFHET_HIP_EINVAL, "%s: null circuit", who);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (l < 1 || Bg_bit < 1 || Bg_bit > 31 || l * Bg_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "%s: bad gadget l=%d Bg_bit=%d (Bg_bit <= 31, l*Bg_bit < 64)", who, l, Bg_bit);
  const int N = c->N;
  SelLogicPlan plan;
  int rc = sellogic_plan(who, N, l, c->n_in, c->n_gates, c->levels, c->widest, count, 256, &plan);
  if (rc || count == 0) return rc;
  if (!d_out_dft) return fail(MOSFHET_HIP_EINVAL, "%s: null d_out_dft", who);
  if (!d_in_dft) return fail(MOSFHET_HIP_EINVAL, "%s: null d_in_dft", who);
  const size_t sample = (size_t)2 * l * 2 * N * sizeof(double);   // bytes of one TRGSW_DFT sample
  if (ranges_overlap(d_out_dft, (size_t)count * c->n_gates * sample, d_in_dft, (size_t)count * c->n_in * sample))
    return fail(MOSFHET_HIP_EINVAL, "%s: d_out_dft overlaps d_in_dft", who);
  HIP_TRY(hipSetDevice(ctx->device));
  const SelGate *image = nullptr;
  if ((rc = table_image(c->lock, c->images, c->table, ctx->device, &image))) return rc;
  hipStream_t s = pick(ctx, stream);
  TraceParams p = {};
  p.kind = TRACE_KIND_SEL_GATE;
  p.l = l; p.base_bit = Bg_bit; p.rows_in = c->n_in; p.rows_out = c->n_gates;
  const size_t slots = sample / sizeof(d2);
  for (long long b0 = 0; b0 < count; b0 += plan.chunk) {
    const long long n = count - b0 < plan.chunk ? count - b0 : plan.chunk;
    p.xin = reinterpret_cast<const d2 *>(d_in_dft) + (size_t)b0 * c->n_in * slots;
    p.sel = reinterpret_cast<d2 *>(d_out_dft) + (size_t)b0 * c->n_gates * slots;
    for (int v = 0; v < c->levels; v++) {
      p.idx = c->first[(size_t)v + 1] - c->first[(size_t)v];
      p.row_ptr = reinterpret_cast<const int *>(image + c->first[(size_t)v]);
      const unsigned teams = (unsigned)(n * p.idx * 2 * l);
      if (N == 1024) { p.tw = ctx->tw1024; hipLaunchKernelGGL(trace_conversions_kernel<Fft1024>, dim3(teams), dim3(Fft1024::THREADS), 0, s, p); }
      else { p.tw = ctx->tw2048; hipLaunchKernelGGL(trace_conversions_kernel<Fft2048>, dim3(teams), dim3(Fft2048::THREADS), 0, s, p); }
    }
  }
  return launched();
}
