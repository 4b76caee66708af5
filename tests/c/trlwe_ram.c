/*
 * GPU test of mosfhet_trlwe_ram_write / mosfhet_trlwe_ram_read (include/mosfhet_compat.h): 3 inputs, each with its own memory of 2^SIZE TRLWE cells and its own
 * encrypted address, at SET_1's ring and gadget (N = 1024, l = 2, Bg = 2^8; 2-bit messages on every coefficient).
 *   - a write equals, word for word, the chain of CMUXes per cell written against include/mosfhet.h (trlwe_sub / trgsw_mul_trlwe_DFT / trlwe_from_DFT / trlwe_add),
 *     at SIZE = 2 and at size 1; a read equals the CMUX tree written the same way, and leaves the memory as it was;
 *   - after the write every cell decrypts: the value at the address, the old message elsewhere; a read at the address decrypts to the value, a read at another
 *     address to that cell's old message.
 * Run by tests/test_trlwe_ram.py; exit status = number of failed checks.
 */
#include <math.h>
#include <mosfhet.h>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __func__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

enum { N = 1024, k = 1, l = 2, Bg_bit = 8, SIZE = 2, CELLS = 1 << SIZE, PREC = 2, COUNT = 3 };

static uint64_t tdist(Torus a, Torus b) { int64_t d = (int64_t)(a - b); return (uint64_t)(d < 0 ? -d : d); }
static int same_trlwe(TRLWE a, TRLWE b) {
  const size_t bytes = sizeof(Torus) * (size_t)N;
  return !memcmp(a->a[0]->coeffs, b->a[0]->coeffs, bytes) && !memcmp(a->b->coeffs, b->b->coeffs, bytes);
}

/* out = in1 + selector (.) (in2 - in1); out may be in1 or in2 */
static void cmux(TRLWE out, TRLWE in1, TRLWE in2, TRGSW_DFT selector) {
  TRLWE_DFT tmp = trlwe_alloc_new_DFT_sample(k, N);
  TRLWE tmp2 = trlwe_alloc_new_sample(k, N);
  trlwe_sub(tmp2, in2, in1);
  trgsw_mul_trlwe_DFT(tmp, tmp2, selector);
  trlwe_from_DFT(tmp2, tmp);
  trlwe_add(out, tmp2, in1);
  free_trlwe(tmp);
  free_trlwe(tmp2);
}

/* cell <- the chain of `size` CMUXes between the cell and val */
static void write_cell(TRLWE cell, TRLWE val, TRGSW_DFT *addr, int size, int i) {
  TRLWE v = trlwe_alloc_new_sample(k, N);
  trlwe_copy(v, val);
  for (int j = 0; j < size; j++) {
    if ((i >> j) & 1) cmux(v, cell, v, addr[j]);
    else cmux(v, v, cell, addr[j]);
  }
  trlwe_copy(cell, v);
  free_trlwe(v);
}

/* out <- the CMUX tree over a copy of the 2^size cells */
static void read_cells(TRLWE out, TRLWE *cells, TRGSW_DFT *addr, int size) {
  TRLWE *T = trlwe_alloc_new_sample_array(1 << size, k, N);
  for (int i = 0; i < (1 << size); i++) trlwe_copy(T[i], cells[i]);
  for (int t = 0; t < size; t++) {
    const int half = 1 << (size - 1 - t);
    for (int j = 0; j < half; j++) cmux(T[j], T[j], T[j + half], addr[size - 1 - t]);
  }
  trlwe_copy(out, T[0]);
  free_trlwe_array(T, 1 << size);
}

static uint64_t worst = 0;
static void check_decrypts(TRLWE c, const Torus *msg, TRLWE_Key key, const char *what, int b, int i) {
  TorusPolynomial ph = polynomial_new_torus_polynomial(N);
  trlwe_phase(ph, c, key);
  uint64_t w = 0;
  for (int j = 0; j < N; j++) {
    const uint64_t d = tdist(ph->coeffs[j], msg[j]);
    if (d > w) w = d;
  }
  if (w > worst) worst = w;
  CHECK(w < (1ULL << (64 - PREC - 1)), "%s, input %d, cell %d: 2^%.1f from the message", what, b, i, log2((double)w + 1.0));
  free_polynomial(ph);
}

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  mosfhet_seed(0x52414D);
  TRLWE_Key rlwe_key = trlwe_new_binary_key(N, k, 2.9802322387695312e-08);   /* 2^-25 */
  TRGSW_Key key = trgsw_new_key(rlwe_key, l, Bg_bit);

  static Torus msg[COUNT][CELLS][N], vmsg[COUNT][N];
  uint64_t x = 0x9E3779B97F4A7C15ULL;
  TRLWE *mem[COUNT], *before[COUNT], *want[COUNT];
  TRLWE *val = trlwe_alloc_new_sample_array(COUNT, k, N), *out = trlwe_alloc_new_sample_array(COUNT, k, N), *ref = trlwe_alloc_new_sample_array(COUNT, k, N);
  TRGSW_DFT *addr[COUNT], *other[COUNT];
  const int address[COUNT] = {0, CELLS - 1, 1}, elsewhere[COUNT] = {CELLS - 1, 1, 2};
  TorusPolynomial m = polynomial_new_torus_polynomial(N);
  TRGSW tmp = trgsw_alloc_new_sample(l, Bg_bit, k, N);
  for (int b = 0; b < COUNT; b++) {
    mem[b] = trlwe_alloc_new_sample_array(CELLS, k, N);
    before[b] = trlwe_alloc_new_sample_array(CELLS, k, N);
    want[b] = trlwe_alloc_new_sample_array(CELLS, k, N);
    for (int i = 0; i <= CELLS; i++) {
      Torus *dst = i < CELLS ? msg[b][i] : vmsg[b];
      for (int j = 0; j < N; j++) {
        x = x * 6364136223846793005ULL + 1442695040888963407ULL;
        dst[j] = m->coeffs[j] = (Torus)((x >> 40) & ((1u << PREC) - 1)) << (64 - PREC);
      }
      trlwe_sample(i < CELLS ? mem[b][i] : val[b], m, rlwe_key);
    }
    addr[b] = trgsw_alloc_new_DFT_sample_array(SIZE, l, Bg_bit, k, N);
    other[b] = trgsw_alloc_new_DFT_sample_array(SIZE, l, Bg_bit, k, N);
    for (int j = 0; j < SIZE; j++) {
      trgsw_monomial_sample(tmp, (address[b] >> j) & 1, 0, key);
      trgsw_to_DFT(addr[b][j], tmp);
      trgsw_monomial_sample(tmp, (elsewhere[b] >> j) & 1, 0, key);
      trgsw_to_DFT(other[b][j], tmp);
    }
  }

  /* size 1 on the first two cells of every memory: a read is one CMUX, a write one CMUX per cell -- every word */
  for (int b = 0; b < COUNT; b++)
    for (int i = 0; i < 2; i++) { trlwe_copy(before[b][i], mem[b][i]); trlwe_copy(want[b][i], mem[b][i]); }
  mosfhet_trlwe_ram_read(out, addr, 1, mem, COUNT);
  for (int b = 0; b < COUNT; b++) {
    cmux(ref[b], mem[b][0], mem[b][1], addr[b][0]);
    CHECK(same_trlwe(out[b], ref[b]), "size 1: the read of input %d differs from trgsw_mul_trlwe_DFT + trlwe_from_DFT", b);
    CHECK(same_trlwe(mem[b][0], before[b][0]) && same_trlwe(mem[b][1], before[b][1]), "size 1: the read changed the memory of input %d", b);
  }
  mosfhet_trlwe_ram_write(mem, addr, 1, val, COUNT);
  for (int b = 0; b < COUNT; b++)
    for (int i = 0; i < 2; i++) {
      write_cell(want[b][i], val[b], addr[b], 1, i);
      CHECK(same_trlwe(mem[b][i], want[b][i]), "size 1: cell %d of input %d differs from the CMUX after the write", i, b);
      trlwe_copy(mem[b][i], before[b][i]);
    }

  /* SIZE: write, then read at the address and elsewhere */
  for (int b = 0; b < COUNT; b++)
    for (int i = 0; i < CELLS; i++) { trlwe_copy(before[b][i], mem[b][i]); trlwe_copy(want[b][i], mem[b][i]); }
  mosfhet_trlwe_ram_write(mem, addr, SIZE, val, COUNT);
  int differ = 0;
  for (int b = 0; b < COUNT; b++)
    for (int i = 0; i < CELLS; i++) {
      write_cell(want[b][i], val[b], addr[b], SIZE, i);
      differ += !same_trlwe(mem[b][i], want[b][i]);
      check_decrypts(mem[b][i], i == address[b] ? vmsg[b] : msg[b][i], rlwe_key, "after the write", b, i);
    }
  CHECK(differ == 0, "%d of %d cells differ from the CMUX chain after the write", differ, COUNT * CELLS);
  printf("write: %d of %d cells differ from the CMUX chain as words; worst distance from the message 2^%.1f (bound 2^%d)\n", differ, COUNT * CELLS,
         log2((double)worst + 1.0), 64 - PREC - 1);

  mosfhet_trlwe_ram_read(out, addr, SIZE, mem, COUNT);
  for (int b = 0; b < COUNT; b++) {
    read_cells(ref[b], mem[b], addr[b], SIZE);
    CHECK(same_trlwe(out[b], ref[b]), "the read of input %d at its address differs from the CMUX tree", b);
    check_decrypts(out[b], vmsg[b], rlwe_key, "read at the address", b, address[b]);
    for (int i = 0; i < CELLS; i++) CHECK(same_trlwe(mem[b][i], want[b][i]), "the read changed cell %d of input %d", i, b);
  }
  mosfhet_trlwe_ram_read(out, other, SIZE, mem, COUNT);
  for (int b = 0; b < COUNT; b++) {
    read_cells(ref[b], mem[b], other[b], SIZE);
    CHECK(same_trlwe(out[b], ref[b]), "the read of input %d at another address differs from the CMUX tree", b);
    check_decrypts(out[b], msg[b][elsewhere[b]], rlwe_key, "read at another address", b, elsewhere[b]);
  }
  /* one input alone: the same words */
  mosfhet_trlwe_ram_read(out, other + 1, SIZE, mem + 1, 1);
  CHECK(same_trlwe(out[0], ref[1]), "a batch of one differs");
  printf("read: worst distance from the message 2^%.1f (bound 2^%d)\n", log2((double)worst + 1.0), 64 - PREC - 1);

  for (int b = 0; b < COUNT; b++) {
    free_trgsw_array(addr[b], SIZE);
    free_trgsw_array(other[b], SIZE);
    free_trlwe_array(mem[b], CELLS);
    free_trlwe_array(before[b], CELLS);
    free_trlwe_array(want[b], CELLS);
  }
  free_trgsw(tmp);
  free_polynomial(m);
  free_trlwe_array(val, COUNT);
  free_trlwe_array(out, COUNT);
  free_trlwe_array(ref, COUNT);
  if (!failures) printf("trlwe_ram ok\n");
  return failures;
}
