"""The Galois-automorphism bootstrap kernels (mosfhet_amd/csrc/bootstrap_kernels.h: pbs_ga_kernel, pbs_ga_wide_kernel, pbs_ga_split_kernel paired / alone / SOLO, and
the stand-alone automorphism, mode == 1 of pbs_ga_kernel) at the VALUES and in the RUN CONTEXTS the plain bootstrap kernels are held to in tests/test_gpu_parity.py.
The family has three hand-written coefficient permutations, three copies of the generator bookkeeping (a_i | 1, Newton inverse mod 2N, gen = a_i a_{i+1}^-1, key entry
(gen - 1) >> 1) and a two-exchange-per-step pairing protocol; random words reach none of their corners.

  1. edge inputs (tests/ga_edges_reference.py: edge_rows; L = log2(2N), word(v) = v << (64 - L)), n = 8 mask words and a body word:
       a  every mask word 0                                  every exponent forced to 1, every generator 1 (entry 0)
       b  every mask word 2^64 - 1                           rounds up, wraps to 0, forced to 1
       c  alternately 2^(63-L) - 1 and 2^(63-L)              the last word that rounds to 0 and the first that rounds to 1
       d  word(2N - 1) + 2^(63-L)                            rounds to 2N, wraps, forced to 1
       e  every mask word word(2N - 1)                       first and last generator 2N - 1 (entry N - 1, the last one), every inner generator 1
       f  alternately word(1) and word(2N - 1)               every inner generator 2N - 1
       g  even exponents 2, 4, N, 2N - 2, N - 2, N + 2, 6, 8  forced odd to 3, 5, N + 1, 2N - 1, ...
       h  alternately word(N - 1) and word(N + 1)            generators N +- 1 (entries N/2 - 1 and N/2), self-inverse
       i  random words                                       control
     the body words make b + prec_offset round to 0, N, 2N - 1 and 2N (wraps), at torus_base 4 and at torus_base 1; keys of n = 1 and n = 2 mask words, where the
     loop's `i + 1 < n` branch is never or once taken
  2. these rows on every form of the family (FORMS), the form that ran asserted; accumulators, bootstrap-key rows and automorphism-key entries at +-2^63 and with
     every gadget digit at +-2^(Bg-1): sums past 2^83, which holds the kernels to the reduction mod 2^64 in front of the rounding (round_mod_2_64) that capi.hip
     claims for all of them
  3. the split kernel's pairing protocol: batch sizes, every bootstrap alone, any mix, two streams at once, more streams than a thread has slot sets
  4. graph capture, two host threads on their own streams, positions in the batch
  5. the refusals of the three entry points that index the key set by a data-dependent (gen - 1) >> 1: a key set with fewer entries is refused before any launch

Expected words are oracle.functional_bootstrap_ga / blind_rotate_ga / trlwe_eval_automorphism on the same words, under oracle.product_order("by_component") where the
split or solo kernels run.  Every device comparison is == on every word; there is no tolerance anywhere on the GPU side.  Key material is uniform random words except
where planted (bit-exactness needs no valid keys); only the automorphism-key entries an input uses are transformed for the oracle.  The oracle itself is held to
exact arithmetic on the same rows in test_oracle_on_the_edge_rows_against_exact_arithmetic (real keys; the code under test plays no part) and to the reference build in
tests/test_oracle_vs_reference.py.
"""
import contextlib
import threading

import numpy as np
import pytest

import ga_edges_reference as R
from test_leveled_lut import _assert_words, _map

U64 = np.uint64
SENTINEL = 0x5EA75EA75EA75EA7
_CACHE = {}
ROWS = len(R.ROW_NAMES)

# (N, l, Bg_bit) of section 2's table
SHAPES = {"N1024 2x8": (1024, 2, 8), "N1024 3x7": (1024, 3, 7), "N2048 2x11": (2048, 2, 11), "N2048 4x9": (2048, 4, 9), "N2048 4x7": (2048, 4, 7),
          "N4096 1x22": (4096, 1, 22)}

# form: (shape, the key's product order, team max batch, wide-team max batch, pairing wait, batch, the family bootstrap_plan must report, how the split launch is taken)
# batch "rows": the nine edge rows; "solo": the edge rows tiled to CUs / 2 + 1, one past the split kernel's batches
FORMS = {
    "wide, N1024 2x8":                      ("N1024 2x8", "auto", 512, 512, 200000, "rows", "latency", None),
    "wide, N1024 3x7":                      ("N1024 3x7", "auto", 512, 512, 200000, "rows", "latency", None),
    "one team, N1024 2x8 compile-time":     ("N1024 2x8", "auto", 0, 512, 200000, "rows", "throughput", None),
    "one team, N1024 3x7 run-time":         ("N1024 3x7", "auto", 0, 512, 200000, "rows", "throughput", None),
    "one team, N2048 2x11 run-time":        ("N2048 2x11", "auto", 512, 0, 200000, "rows", "throughput", None),
    "wide, N2048 2x11":                     ("N2048 2x11", "auto", 512, 512, 200000, "rows", "latency", None),
    "wide, N2048 4x9 reference key":        ("N2048 4x9", "reference", 512, 512, 200000, "rows", "latency", None),
    "one team Fft2048L, N2048 4x9 reference key": ("N2048 4x9", "reference", 512, 0, 200000, "rows", "throughput", None),
    "split paired, N2048 4x9":              ("N2048 4x9", "auto", 512, 512, 200000, "rows", "split", "paired"),
    "split paired, N2048 4x7 run-time":     ("N2048 4x7", "auto", 512, 512, 200000, "rows", "split", "paired"),
    "split alone, N2048 4x9":               ("N2048 4x9", "auto", 512, 512, 0, "rows", "split", "alone"),
    "split alone, N2048 4x7 run-time":      ("N2048 4x7", "auto", 512, 512, 0, "rows", "split", "alone"),
    "solo, N2048 4x9 by-component key":     ("N2048 4x9", "by_component", 512, 512, 200000, "solo", "latency_by_component", None),
    "one team, N4096 1x22":                 ("N4096 1x22", "auto", 512, 512, 200000, "rows", "throughput", None),
}


def _oracle_order(form):
    return "by_component" if FORMS[form][6] in ("split", "latency_by_component") else "reference"


def _rand(rng, *shape):
    return rng.integers(0, 2 ** 64, size=shape, dtype=U64)


def _log2(x):
    return float(np.log2(max(float(x), 1.0)))


# ---------------------------------------------------------------- keys and expected words ----------------------------------------------------------------
def _random_ak(N, l):
    """uniform random automorphism key set [N][l][2][N], one per (N, l): 4 x 2^9 and the run-time 4 x 2^7 share theirs"""
    key = ("ak", N, l)
    if key not in _CACHE:
        _CACHE[key] = _rand(np.random.default_rng(0xA6 + N + l), N, l, 2, N)
    return _CACHE[key]


def _planted_entries(N):
    """the entries the edge rows use at either torus_base (the mask words do not depend on it), and entry 1 for generator 3 of the stand-alone automorphism"""
    return sorted(R.entries_used(R.edge_rows(N, 4), N) | {1})


def _host_keys(oracle, shape, plant=None):
    """dict(bk [8][2l][2][N], bk_dft, ak [N][l][2][N], ak_dft with the entries transformed so far).  plant None: uniform random words.  plant "A": bootstrap-key
    entry i and the j-th automorphism-key entry the edge rows use hold every word 2^63 / every word 2^63 - 1 / the two alternating by coefficient, by i % 3 and
    j % 3 (entry 0: every word 2^63), every other automorphism-key entry zero.  plant "B": as A with automorphism-key entry 0 zero, so that row a's first key switch
    returns (0, b) and the first external product decomposes the caller's b alone."""
    key = ("host", shape, plant)
    if key in _CACHE:
        return _CACHE[key]
    N, l, Bg = SHAPES[shape]
    oracle.plan(N)
    if plant is None:
        bk, ak = _rand(np.random.default_rng(0xB6 + N + 16 * l + Bg), R.N_MASK, 2 * l, 2, N), _random_ak(N, l)
    else:
        bk, ak = np.empty((R.N_MASK, 2 * l, 2, N), dtype=U64), np.zeros((N, l, 2, N), dtype=U64)
        for i in range(R.N_MASK):
            bk[i] = R.extreme_poly(R.KEY_KINDS[i % 3], N, l, Bg)
        for j, e in enumerate(_planted_entries(N)):
            ak[e] = R.extreme_poly(R.KEY_KINDS[j % 3], N, l, Bg)
        if plant == "B":
            ak[0] = 0
    H = dict(shape=shape, plant=plant, N=N, l=l, Bg=Bg, bk=bk, bk_dft=oracle.bk_to_dft(bk, 1, l), ak=ak, ak_dft=np.zeros(ak.shape, dtype=np.float64), filled=set())
    _CACHE[key] = H
    return H


def _fill(oracle, H, entries):
    """transform the automorphism-key entries an input uses, once"""
    for j in sorted(set(entries) - H["filled"]):
        H["ak_dft"][j] = oracle.ks_to_dft(H["ak"][j])
        H["filled"].add(j)


def _dev_keys(eng, H, n=R.N_MASK):
    """(bootstrap key over the first n entries, automorphism key set) on the device, loaded once"""
    key = ("dev", H["shape"], H["plant"])
    if key not in _CACHE:
        _CACHE[key] = dict(gak=eng.load_automorphism_keys(H["ak"], H["Bg"]))
    D = _CACHE[key]
    if n not in D:
        D[n] = eng.load_bootstrap_key(H["bk"][:n], 1, H["l"], H["Bg"])
    return D[n], D["gak"]


def _inputs(shape):
    """dict(cts[torus_base] [9][9], tv [2][N], tvs [9][2][N], accs [9][2][N]) of a shape: the edge rows, one shared and nine per-ciphertext test vectors of random
    words, nine accumulators of random words"""
    key = ("inputs", shape)
    if key not in _CACHE:
        N = SHAPES[shape][0]
        rng = np.random.default_rng(0xC6 + N)
        _CACHE[key] = dict(cts={tb: R.edge_rows(N, tb) for tb in (4, 1)}, tv=_rand(rng, 2, N), tvs=_rand(rng, ROWS, 2, N), accs=_rand(rng, ROWS, 2, N))
    return _CACHE[key]


def _bootstrap_words(oracle, H, tvs, cts, torus_base, extract, order):
    """oracle.functional_bootstrap_ga over a batch; tvs [1 or count][2][N]"""
    n = cts.shape[1] - 1
    _fill(oracle, H, R.entries_used(cts, H["N"]))
    with oracle.product_order(order):
        return np.stack(_map(lambda b: oracle.functional_bootstrap_ga(tvs[b % len(tvs)], cts[b], H["bk_dft"][:n], H["ak_dft"], H["l"], H["Bg"], torus_base, extract=extract),
                             range(len(cts))))


def _rotate_words(oracle, H, accs, cts, order):
    """oracle.blind_rotate_ga over a batch of accumulators [count][2][N]"""
    n = cts.shape[1] - 1
    _fill(oracle, H, R.entries_used(cts, H["N"]))
    with oracle.product_order(order):
        return np.stack(_map(lambda b: oracle.blind_rotate_ga(accs[b], cts[b, :n].copy(), H["bk_dft"][:n], H["ak_dft"], H["l"], H["Bg"]), range(len(cts))))


def _expected(oracle, shape, order):
    """the oracle's words for the edge rows of a shape in a product order, computed once: (torus_base, extract, per-ciphertext test vectors) -> [9][..]; "rotate" ->
    blind_rotate_ga on the random accumulators; ("n", 1) and ("n", 2) -> the bootstrap with extraction at torus_base 4 over the first 1 and 2 key entries"""
    key = ("expected", shape, order)
    if key in _CACHE:
        return _CACHE[key]
    H, I = _host_keys(oracle, shape), _inputs(shape)
    W = {}
    for tb in (4, 1):
        for extract in (True, False):
            for per in (False, True):
                W[tb, extract, per] = _bootstrap_words(oracle, H, I["tvs"] if per else I["tv"][None], I["cts"][tb], tb, extract, order)
    W["rotate"] = _rotate_words(oracle, H, I["accs"], I["cts"][4], order)
    for n in (1, 2):
        W["n", n] = _bootstrap_words(oracle, H, I["tv"][None], R.shorten(I["cts"][4], n), 4, True, order)
    _CACHE[key] = W
    return W


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_edge_rows_reach_what_they_claim(N):
    """From Python integers (pow(x, -1, 2N)): per row the exponents and generators the table of the module docstring names; over the batch the key entries 0,
    N/2 - 1, N/2 and N - 1; the body words round to 0, N, 2N - 1 and 2N (wraps) at torus_base 4 and 1; keys of one and two mask words use entry N - 1 as well."""
    top = 2 * N - 1
    for tb in (4, 1):
        cts = R.edge_rows(N, tb)
        assert cts.shape == (ROWS, R.N_MASK + 1)
        a = {name: R.exponents(cts[r], N) for r, name in enumerate(R.ROW_NAMES)}
        g = {name: R.generators(cts[r], N) for r, name in enumerate(R.ROW_NAMES)}
        for name in "abd":
            assert a[name] == [1] * 8 and g[name] == [1] * 9, name
        assert a["c"] == [1] * 8                                                     # 0 | 1 and 1 | 1
        assert [R.modswitch(x, N) for x in cts[2, :8]] == [0, 1] * 4
        assert [R.modswitch(x, N) for x in cts[1, :8]] == [0] * 8 and [R.modswitch(x, N) for x in cts[3, :8]] == [0] * 8
        assert g["e"] == [top] + [1] * 7 + [top]
        assert g["f"] == [1] + [top] * 7 + [top]
        assert a["g"] == [3, 5, N + 1, top, N - 1, N + 3, 7, 9]
        assert a["h"] == [N - 1, N + 1] * 4 and g["h"][0] == N - 1 and g["h"][-1] == N + 1 and (N - 1) ** 2 % (2 * N) == 1 and (N + 1) ** 2 % (2 * N) == 1
        m = list(range(1, N + 1))
        assert R.permute(m, N + 1, N) == [x if i % 2 == 0 else 2 ** 64 - x for i, x in enumerate(m)]      # generator N + 1 flips the sign of the odd coefficients only
        assert R.permute(m, 1, N) == m and R.permute(m, top, N) == [m[0]] + [2 ** 64 - x for x in m[:0:-1]]
        for row in cts:
            for x, inv in zip(R.exponents(row, N), [pow(x, -1, 2 * N) for x in R.exponents(row, N)]):
                assert x * inv % (2 * N) == 1
        used = R.entries_used(cts, N)
        assert {0, N // 2 - 1, N // 2, N - 1} <= used, sorted(used)
        bbar = [R.body_exponent(row, N, tb) for row in cts]
        raw = [((int(row[-1]) + R.prec_offset(tb)) % 2 ** 64 + (1 << (63 - R.log2n2(N)))) >> (64 - R.log2n2(N)) for row in cts]
        assert {0, N, top} <= set(bbar) and 2 * N in raw, (bbar, raw)
        for n in (1, 2):
            short = R.shorten(cts, n)
            assert short.shape == (ROWS, n + 1) and {0, N - 1} <= R.entries_used(short, N)
            assert (short[:, -1] == cts[:, -1]).all()


def test_oracle_on_the_edge_rows_against_exact_arithmetic(oracle):
    """The oracle alone, at N = 1024, 2 x 2^8, n = 8 with a REAL Galois bootstrap key and a REAL automorphism key set (both at sigma 2^-50, binary keys): for every edge
    row, at torus_base 4 and 1, the phase of functional_bootstrap_ga without extraction is the exact negacyclic rotation X^e m of the test vector's message by
    e = (-bbar + sum_i (abar_i | 1) s_i) mod 2N, computed with Python integers.  Measured here: worst torus distance 2^54.52 over the 18 outputs (the decomposition's
    rounding, 2^47 per coefficient, over 17 products); asserted: 4 x that, 2^56.52 -- the factor is for the seed -- which stays 3.5 bits below 2^60, a sixteenth of the
    table's message spacing of 2^62.  A wrong exponent, generator, inverse, key entry or permutation sign moves a phase by a whole message (2^62) or
    scrambles it."""
    N, l, Bg, n, sigma = 1024, 2, 8, R.N_MASK, 2.0 ** -50
    rng = oracle.Rng(0x6AE)
    lwe_s, s = oracle.gen_binary_key(rng, n), oracle.gen_binary_key(rng, N)
    bk_dft = oracle.bk_to_dft(oracle.gen_bootstrap_key_ga(rng, lwe_s, s.reshape(1, N), l, Bg, sigma), 1, l)
    ak = oracle.gen_automorphism_keyset(rng, s, l, Bg, sigma)
    ak_dft = np.zeros(ak.shape, dtype=np.float64)
    for j in R.entries_used(R.edge_rows(N, 4), N):
        ak_dft[j] = oracle.ks_to_dft(ak[j])
    tv = oracle.trlwe_torus_packing(np.array([3 << 60, 7 << 60, 11 << 60, 15 << 60], dtype=U64), 1, N)
    assert (tv[0] == 0).all()
    msg = [int(x) for x in tv[1]]
    worst = 0.0
    for tb in (4, 1):
        for r, row in enumerate(R.edge_rows(N, tb)):
            out = oracle.functional_bootstrap_ga(tv, row, bk_dft, ak_dft, l, Bg, tb, extract=False)
            e = (-R.body_exponent(row, N, tb) + sum(a * int(si) for a, si in zip(R.exponents(row, N), lwe_s))) % (2 * N)
            want = np.array(R.rotate(msg, e, N), dtype=U64)
            dist = float(oracle.torus_dist(oracle.trlwe_phase(out, s), want).max())
            print("torus_base %d, row %s: e = %d, log2 distance %.1f" % (tb, R.ROW_NAMES[r], e, _log2(dist)))
            worst = max(worst, dist)
    bound = 4 * 2.0 ** 54.52
    print("worst log2 distance %.2f, bound %.2f" % (_log2(worst), _log2(bound)))
    assert bound < 2.0 ** 60
    assert worst < bound, _log2(worst)


def _first_step_sums(shape):
    """log2 of the largest exact integer sum of the first key switch (plant A: the digits of the accumulator's a against automorphism-key entry 0) and of the first
    external product (plant B: that key switch returns (0, b); the digits of (0, b) against bootstrap-key entry 0) of edge row a -- generator 1, the identity
    permutation -- per accumulator kind"""
    if ("sums", shape) in _CACHE:
        return _CACHE["sums", shape]
    N, l, Bg = SHAPES[shape]
    out = _CACHE["sums", shape] = {}
    for kind in R.ACC_KINDS:
        p = R.extreme_poly(kind, N, l, Bg)
        d = R.digits(p, l, Bg)
        key0 = R.extreme_poly(R.KEY_KINDS[0], N, l, Bg)
        out["key switch", kind] = R.largest_sum_log2(d, np.stack([key0] * l))
        both = np.concatenate([R.digits(np.zeros(N, dtype=U64), l, Bg), d])
        out["external product", kind] = R.largest_sum_log2(both, np.stack([key0] * (2 * l)))
    return out


def test_planted_magnitudes_pass_the_reduction_free_bound():
    """The condition on the inputs of the magnitude tests: with every digit of the accumulator at -2^(Bg-1) against key rows of -2^63 the exact sums of the first key
    switch and of the first external product reach l N 2^(Bg-1) 2^63 -- at N = 2048, 4 x 2^9: 2^84, past the 2^83 up to which rounding without the reduction
    mod 2^64 is exact.  exact_sums itself against a direct evaluation in Python integers at a small size."""
    rng = np.random.default_rng(7)
    d, key = rng.integers(-256, 256, size=(3, 16)), _rand(rng, 3, 16)
    signed = [[int(x) - (1 << 64 if int(x) >> 63 else 0) for x in row] for row in key]
    direct = [sum(int(d[r][j]) * signed[r][(k - j) % 16] * (1 if j <= k else -1) for r in range(3) for j in range(16)) for k in range(16)]
    assert R.exact_sums(d.astype(np.int64), key) == direct
    assert (R.digits(R.extreme_poly("digits_lo", 64, 4, 9), 4, 9) == -256).all() and (R.digits(R.extreme_poly("digits_hi", 64, 4, 9), 4, 9) == 255).all()
    assert (R.digits(np.zeros(8, dtype=U64), 4, 9) == 0).all()
    sums = _first_step_sums("N2048 4x9")
    for k, v in sums.items():
        print("N2048 4x9, %s, accumulator %s: largest exact sum 2^%.2f" % (k + (v,)))
    assert sums["key switch", "digits_lo"] > 83 and sums["external product", "digits_lo"] > 83, sums
    assert abs(sums["key switch", "digits_lo"] - (2 + 11 + 8 + 63)) < 0.01


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    for key in [k for k in _CACHE if k[0] == "dev"]:
        for h in _CACHE.pop(key).values():
            h.free()
    e.close()


def _cus(eng):
    import torch
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


@contextlib.contextmanager
def _settings(bsk, order="auto", team=512, wide=512, wait=200000):
    """the setters that choose the form, restored on every way out"""
    from mosfhet_amd import engine
    try:
        engine.set_split_max_batch(-1)
        engine.set_team_max_batch(team)
        engine.set_wide_team_max_batch(wide)
        engine.set_split_wait_limit(wait)
        bsk.set_product_order(order)
        yield
    finally:
        bsk.set_product_order("auto")
        engine.set_split_wait_limit(200000)
        engine.set_wide_team_max_batch(512)
        engine.set_team_max_batch(512)


def _assert_form(eng, bsk, form, B):
    """in front of the calls: the launchers' own decision for this key and batch at the current setters"""
    plan = eng.bootstrap_plan(bsk, B, galois=True)
    assert plan["family"] == FORMS[form][6], (form, B, plan)


def _assert_split(form, B):
    """behind a call: how the split launch was taken (the launcher's own account, per host thread)"""
    from mosfhet_amd import engine
    how = FORMS[form][7]
    if how:
        assert engine.split_last_launch() == ((B, B, 0) if how == "paired" else (B, 0, B)), (form, engine.split_last_launch())


def _guarded(eng, B, *row):
    """an output of B rows with a sentinel-filled guard row behind it"""
    import torch
    return torch.full((B + 1,) + row, SENTINEL, dtype=torch.int64, device=eng.device)


def _bootstrap(eng, bsk, gak, d_tv, d_ct, tb, extract, what):
    """functional_bootstrap_ga into a guarded buffer: the words, the guard row checked"""
    import mosfhet_amd as ma
    B, N = d_ct.shape[0], bsk.N
    buf = _guarded(eng, B, *((N + 1,) if extract else (2, N)))
    eng.functional_bootstrap_ga(bsk, gak, d_tv, d_ct, tb, extract=extract, out=buf[:B])
    got = ma.to_numpy(buf)
    assert (got[B] == U64(SENTINEL)).all(), "%s wrote past its last output" % what
    return got[:B]


def _rotate(eng, bsk, gak, accs, d_ct, what):
    """blind_rotate_ga in place on a copy of the accumulators with a guard row behind it"""
    import mosfhet_amd as ma
    B = d_ct.shape[0]
    buf = _guarded(eng, B, 2, bsk.N)
    buf[:B].copy_(ma.to_device(accs, eng.device))
    eng.blind_rotate_ga(bsk, gak, buf[:B], d_ct)
    got = ma.to_numpy(buf)
    assert (got[B] == U64(SENTINEL)).all(), "%s wrote past its last accumulator" % what
    return got[:B]


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_edge_rows_on_every_form(eng, oracle, form):
    """1 and 2.  The edge rows through one form of the family, the form asserted from the launchers' own plan (and, for the split kernel, from its pairing words):
    functional_bootstrap_ga with and without extraction, with one shared test vector and with one per ciphertext, at torus_base 4 and 1; blind_rotate_ga in place;
    keys of one and two mask words.  Every word equals the oracle's; the inputs on the device are unchanged and the guard row behind every output keeps its pattern."""
    import torch
    import mosfhet_amd as ma
    shape, order, team, wide, wait, batch, family, how = FORMS[form]
    H, I, W = _host_keys(oracle, shape), _inputs(shape), _expected(oracle, shape, _oracle_order(form))
    bsk, gak = _dev_keys(eng, H)
    B = ROWS if batch == "rows" else _cus(eng) // 2 + 1
    idx = np.arange(B) % ROWS
    d_tv, d_tvs, d_cts = ma.to_device(I["tv"][None], eng.device), ma.to_device(I["tvs"][idx], eng.device), {tb: ma.to_device(I["cts"][tb][idx], eng.device) for tb in (4, 1)}
    keep = [d_tv.clone(), d_tvs.clone(), d_cts[4].clone(), d_cts[1].clone()]
    with _settings(bsk, order, team, wide, wait):
        _assert_form(eng, bsk, form, B)
        for tb in (4, 1):
            for extract in (True, False):
                for per in (False, True):
                    what = "%s: torus_base %d, extract %s, %s" % (form, tb, extract, "a test vector per ciphertext" if per else "one test vector")
                    got = _bootstrap(eng, bsk, gak, d_tvs if per else d_tv, d_cts[tb], tb, extract, what)
                    _assert_split(form, B)
                    _assert_words(got, W[tb, extract, per][idx], what)
        got = _rotate(eng, bsk, gak, I["accs"][idx], d_cts[4], form)
        _assert_split(form, B)
        _assert_words(got, W["rotate"][idx], "%s: blind_rotate_ga in place" % form)
    for n in (1, 2):
        short, _ = _dev_keys(eng, H, n)
        with _settings(short, order, team, wide, wait):
            _assert_form(eng, short, form, B)
            got = _bootstrap(eng, short, gak, d_tv, ma.to_device(R.shorten(I["cts"][4], n)[idx], eng.device), 4, True, "%s: n = %d" % (form, n))
            _assert_split(form, B)
            _assert_words(got, W["n", n][idx], "%s: a key of %d mask words" % (form, n))
    for t, t0 in zip([d_tv, d_tvs, d_cts[4], d_cts[1]], keep):
        assert torch.equal(t, t0), "%s changed its inputs" % form


# the forms the magnitudes run on: every kernel of the family once at SET_1's gadget and at 4 x 2^9, the only form of N = 4096
MAGNITUDE_FORMS = ["wide, N1024 2x8", "one team, N1024 2x8 compile-time", "wide, N2048 4x9 reference key", "one team Fft2048L, N2048 4x9 reference key",
                   "split paired, N2048 4x9", "split alone, N2048 4x9", "solo, N2048 4x9 by-component key", "one team, N4096 1x22"]


def _extreme_accs(shape):
    """[6 kinds x 9 rows][2][N]: accumulator kind k (both components) for edge row r at index 9 k + r"""
    N, l, Bg = SHAPES[shape]
    return np.stack([np.stack([R.extreme_poly(kind, N, l, Bg)] * 2) for kind in R.ACC_KINDS for _ in range(ROWS)])


@pytest.mark.gpu
@pytest.mark.parametrize("form", MAGNITUDE_FORMS)
def test_extreme_accumulators_and_keys_through_blind_rotate_ga(eng, oracle, form):
    """2, magnitudes.  blind_rotate_ga on accumulators of every word 2^63, every word 2^63 - 1, the two alternating, zero, every digit -2^(Bg-1) and every digit
    2^(Bg-1) - 1, one of each per edge row, under keys with the same extremes planted in the bootstrap-key rows and in the automorphism-key entries the rows use
    (_host_keys: plant A; at 4 x 2^9 also plant B, whose first external product sees the caller's digits): every word equals the oracle's.  Prints the largest exact sum of the first step (test_planted_magnitudes_pass_the_reduction_free_bound holds it past 2^83 at
    N = 2048, 4 x 2^9): a kernel that rounded without the reduction would differ there."""
    import mosfhet_amd as ma
    shape, order, team, wide, wait, batch, family, how = FORMS[form]
    accs, cts = _extreme_accs(shape), np.concatenate([R.edge_rows(SHAPES[shape][0], 4)] * len(R.ACC_KINDS))
    B = len(accs) if batch == "rows" else max(len(accs), _cus(eng) // 2 + 1)
    idx = np.arange(B) % len(accs)
    sums = _first_step_sums(shape)
    for step in ("key switch", "external product"):
        print("%s, first %s: largest exact sum 2^%.2f" % (shape, step, max(v for k, v in sums.items() if k[0] == step)))
    plants = ("A", "B") if shape == "N2048 4x9" else ("A",)
    for plant in plants:
        H = _host_keys(oracle, shape, plant)
        key = ("extreme rotate", shape, plant, _oracle_order(form))
        if key not in _CACHE:
            _CACHE[key] = _rotate_words(oracle, H, accs, cts, _oracle_order(form))
        bsk, gak = _dev_keys(eng, H)
        with _settings(bsk, order, team, wide, wait):
            _assert_form(eng, bsk, form, B)
            got = _rotate(eng, bsk, gak, accs[idx], ma.to_device(cts[idx], eng.device), form)
            _assert_split(form, B)
            _assert_words(got, _CACHE[key][idx], "%s, plant %s: extreme accumulators" % (form, plant))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["N1024 2x8", "N1024 3x7", "N2048 2x11", "N2048 4x9", "N4096 1x22"])
def test_extreme_inputs_through_the_stand_alone_automorphism(eng, oracle, shape):
    """2, magnitudes, mode == 1 (pbs_ga_kernel alone, so at each N and at compile-time and run-time gadgets): trlwe_eval_automorphism and its _entry form at the
    generators 1, 3, N - 1, N + 1 and 2N - 1 on the six extreme accumulators, on their pre-images under the permutation (so that the PERMUTED polynomial has every
    digit at the extreme) and on random words, with key entries of +-2^63: every word equals oracle.trlwe_eval_automorphism.  The _entry form with the entry of the
    NEXT generator of the list: the permutation and the key are independent.  Prints the largest exact sum per generator."""
    import torch
    import mosfhet_amd as ma
    N, l, Bg = SHAPES[shape]
    H = _host_keys(oracle, shape, "A")
    _, gak = _dev_keys(eng, H)
    gens = [1, 3, N - 1, N + 1, 2 * N - 1]
    _fill(oracle, H, [(g - 1) // 2 for g in gens])
    rng = np.random.default_rng(0xD6 + N)
    plain = [np.stack([R.extreme_poly(kind, N, l, Bg)] * 2) for kind in R.ACC_KINDS]
    for i, gen in enumerate(gens):
        inv = pow(gen, -1, 2 * N)
        pre = [np.stack([oracle.poly_permute(p[0], inv)] * 2) for p in plain]
        assert all((oracle.poly_permute(q[0], gen) == p[0]).all() for p, q in zip(plain, pre))
        accs = np.stack(plain + pre + [_rand(rng, 2, N)])
        entry, other = (gen - 1) // 2, (gens[(i + 1) % len(gens)] - 1) // 2
        mag = max(R.largest_sum_log2(R.digits(oracle.poly_permute(a[0], gen), l, Bg), H["ak"][entry, :, 0]) for a in accs)
        print("%s, generator %d: largest exact sum 2^%.2f" % (shape, gen, mag))
        d = ma.to_device(accs, eng.device)
        d0 = d.clone()
        buf = _guarded(eng, len(accs), 2, N)
        eng.trlwe_eval_automorphism(gak, d, gen, out=buf[:len(accs)])
        got = ma.to_numpy(buf)
        assert (got[len(accs)] == U64(SENTINEL)).all(), (shape, gen)
        want = np.stack([oracle.trlwe_eval_automorphism(a, gen, H["ak_dft"][entry], l, Bg) for a in accs])
        _assert_words(got[:len(accs)], want, "%s: automorphism of generator %d" % (shape, gen))
        assert (ma.to_numpy(eng.trlwe_eval_automorphism_entry(gak, entry, d, gen)) == want).all(), (shape, gen, "entry form")
        want = np.stack([oracle.trlwe_eval_automorphism(a, gen, H["ak_dft"][other], l, Bg) for a in accs])
        _assert_words(ma.to_numpy(eng.trlwe_eval_automorphism_entry(gak, other, d, gen)), want, "%s: generator %d through entry %d" % (shape, gen, other))
        assert torch.equal(d, d0), "the automorphism changed its input"


# ---------------------------------------------------------------- 3: the split kernel's protocol ----------------------------------------------------------------
def _protocol_case(eng, oracle, B):
    """the edge rows of N = 2048, 4 x 2^9 tiled to B under an AUTO key: per entry point (extract, no extract, blind_rotate_ga) a function that runs it and the words
    the oracle gives by component"""
    import mosfhet_amd as ma
    shape = "N2048 4x9"
    H, I, W = _host_keys(oracle, shape), _inputs(shape), _expected(oracle, shape, "by_component")
    bsk, gak = _dev_keys(eng, H)
    idx = np.arange(B) % ROWS
    d_tv, d_ct = ma.to_device(I["tv"][None], eng.device), ma.to_device(I["cts"][4][idx], eng.device)
    return bsk, [("extract", lambda: _bootstrap(eng, bsk, gak, d_tv, d_ct, 4, True, "extract"), W[4, True, False][idx]),
                 ("no extract", lambda: _bootstrap(eng, bsk, gak, d_tv, d_ct, 4, False, "no extract"), W[4, False, False][idx]),
                 ("blind_rotate_ga", lambda: _rotate(eng, bsk, gak, I["accs"][idx], d_ct, "blind_rotate_ga"), W["rotate"][idx])]


@pytest.mark.gpu
def test_ga_split_kernel_batch_sizes_pairs_and_alone(eng, oracle):
    """3.  pbs_ga_split_kernel at N = 2048, 4 x 2^9, n = 8 on the edge rows: batches of 1, 7, 8, 9 and 33 (block pairs B / B + 8, ragged groups of eight) are all taken
    by PAIRS of workgroups and give the oracle's by-component words through all three entry points; with the pairing wait at 0 every bootstrap is taken ALONE and the
    bits are the same; with a wait of one tick (10 ns) some pairs form and some do not -- whatever the mix, the same bits.  Nothing here is meant to stall: the
    pairing wait is bounded and a paired workgroup's partner is resident."""
    from mosfhet_amd import engine
    by_component, reference = _expected(oracle, "N2048 4x9", "by_component"), _expected(oracle, "N2048 4x9", "reference")
    assert all((by_component[k] != reference[k]).any() for k in by_component), "the two summation orders give different words on these rows: the comparison tells them apart"
    for B in (1, 7, 8, 9, 33):
        bsk, calls = _protocol_case(eng, oracle, B)
        with _settings(bsk):
            assert eng.bootstrap_plan(bsk, B, galois=True)["family"] == "split"
            for name, run, want in calls:
                got = run()
                assert engine.split_last_launch() == (B, B, 0), (B, name, engine.split_last_launch())
                _assert_words(got, want, "%d Galois bootstraps on two CUs each, %s" % (B, name))
    bsk, calls = _protocol_case(eng, oracle, 33)
    with _settings(bsk, wait=0):
        for name, run, want in calls:
            got = run()
            assert engine.split_last_launch() == (33, 0, 33), (name, engine.split_last_launch())
            _assert_words(got, want, "33 Galois bootstraps, each alone, %s" % name)
    with _settings(bsk, wait=1):
        for name, run, want in calls:
            got = run()
            n, paired, alone = engine.split_last_launch()
            assert n == 33 and paired + alone == 33, (name, n, paired, alone)
            _assert_words(got, want, "33 Galois bootstraps, %d paired and %d alone, %s" % (paired, alone, name))


@pytest.mark.gpu
def test_ga_split_kernel_launches_on_two_streams_at_once(eng, oracle):
    """3.  Two streams with split launches of 33 in flight at the same time, three rounds of all three entry points: each stream has its own exchange slots -- both
    slot sets of the Galois kernel -- and pairing words (capi.hip: split_set), and every output equals the single-stream words.  Then ten fresh streams of 8: more
    streams than a host thread has slot sets, the least recently used set changes hands; still two CUs per bootstrap, still the same bits."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    shape = "N2048 4x9"
    H, I, W = _host_keys(oracle, shape), _inputs(shape), _expected(oracle, shape, "by_component")
    bsk, gak = _dev_keys(eng, H)
    B = 33
    idx = [np.arange(B) % ROWS, (np.arange(B) + 4) % ROWS]
    d_tv = ma.to_device(I["tv"][None], eng.device)
    d_cts = [ma.to_device(I["cts"][tb][ix], eng.device) for tb, ix in zip((4, 1), idx)]
    d_accs = [ma.to_device(I["accs"][ix], eng.device) for ix in idx]
    want = [[W[tb, True, False][ix], W[tb, False, False][ix]] for tb, ix in zip((4, 1), idx)]
    want_rot = [_rotate_words(oracle, H, I["accs"][ix], I["cts"][tb][ix], "by_component") for tb, ix in zip((4, 1), idx)]
    streams = [torch.cuda.Stream(device=eng.device) for _ in range(2)]
    outs = [[], []]
    with _settings(bsk):
        torch.cuda.synchronize()
        for rep in range(3):
            for i, st in enumerate(streams):
                with torch.cuda.stream(st):
                    acc = d_accs[i].clone()
                    eng.blind_rotate_ga(bsk, gak, acc, d_cts[i])
                    outs[i].append((eng.functional_bootstrap_ga(bsk, gak, d_tv, d_cts[i], (4, 1)[i]), eng.functional_bootstrap_ga(bsk, gak, d_tv, d_cts[i], (4, 1)[i], extract=False), acc))
        torch.cuda.synchronize()
        for i in range(2):
            for rep, (a, b, c) in enumerate(outs[i]):
                _assert_words(ma.to_numpy(a), want[i][0], "stream %d, round %d, extract" % (i, rep))
                _assert_words(ma.to_numpy(b), want[i][1], "stream %d, round %d, no extract" % (i, rep))
                _assert_words(ma.to_numpy(c), want_rot[i], "stream %d, round %d, blind_rotate_ga" % (i, rep))
        for k in range(10):
            st = torch.cuda.Stream(device=eng.device)
            with torch.cuda.stream(st):
                o = eng.functional_bootstrap_ga(bsk, gak, d_tv, d_cts[0][:8], 4, extract=bool(k % 2))
            st.synchronize()
            assert engine.split_last_launch() == (8, 8, 0), (k, engine.split_last_launch())
            _assert_words(ma.to_numpy(o), want[0][1 - k % 2][:8], "fresh stream %d" % k)


# ---------------------------------------------------------------- 4: run contexts ----------------------------------------------------------------
def _context_inputs(oracle, shape, B, sets, seed):
    """`sets` batches of B rows for a shape: the edge rows (torus_base 4) in a set-dependent rotation, random words behind them"""
    N = SHAPES[shape][0]
    rng = np.random.default_rng(seed)
    out = []
    for r in range(sets):
        cts = _rand(rng, B, R.N_MASK + 1)
        cts[:min(B, ROWS)] = np.roll(R.edge_rows(N, 4), r, axis=0)[:min(B, ROWS)]
        out.append(cts)
    return out


@pytest.mark.gpu
def test_ga_launches_are_captured_in_a_graph(eng, oracle):
    """4.  A Galois batch of 20 at N = 1024 on the one-team kernel and one of 70 at N = 2048, 4 x 2^9 under a REFERENCE key with the latency kernel off (pbs_ga_kernel
    on Fft2048L in one paced residency round, the memset of its rendezvous counters in front), captured into ONE graph on a side stream after eager calls of the same
    shapes and replayed three times on fresh inputs: every replay equals the eager call, whose words are the oracle's.  (The paired split kernel is not captured: it is
    covered eagerly above.)"""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    jobs = []
    for shape, order, B in (("N1024 2x8", "auto", 20), ("N2048 4x9", "reference", 70)):
        H, I = _host_keys(oracle, shape), _inputs(shape)
        bsk, gak = _dev_keys(eng, H)
        jobs.append(dict(shape=shape, H=H, bsk=bsk, gak=gak, B=B, order=order, tv=ma.to_device(I["tv"][None], eng.device), host_tv=I["tv"],
                         cts=_context_inputs(oracle, shape, B, 3, 0xE6 + B), d_in=eng.empty(B, R.N_MASK + 1), d_out=eng.empty(B, H["N"] + 1)))
    with contextlib.ExitStack() as stack:
        for J in jobs:
            stack.enter_context(_settings(J["bsk"], J["order"]))
        # both latency kernels off (the team threshold governs N = 1024, the wide-team threshold N = 2048); _settings restores them on the way out
        engine.set_team_max_batch(0)
        engine.set_wide_team_max_batch(0)
        for J in jobs:
            assert eng.bootstrap_plan(J["bsk"], J["B"], galois=True)["family"] == "throughput", J["shape"]
            J["eager"] = [ma.to_numpy(eng.functional_bootstrap_ga(J["bsk"], J["gak"], J["tv"], ma.to_device(c, eng.device), 4)) for c in J["cts"]]
            want = _bootstrap_words(oracle, J["H"], J["host_tv"][None], J["cts"][0], 4, True, "reference")
            _assert_words(J["eager"][0], want, "%s: eager batch of %d" % (J["shape"], J["B"]))
            J["d_in"].copy_(ma.to_device(J["cts"][0], eng.device))
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=eng.device)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            for J in jobs:
                eng.functional_bootstrap_ga(J["bsk"], J["gak"], J["tv"], J["d_in"], 4, out=J["d_out"])
        for r in (1, 2, 0):
            for J in jobs:
                J["d_in"].copy_(ma.to_device(J["cts"][r], eng.device))
                J["d_out"].zero_()
            g.replay()
            torch.cuda.synchronize()
            for J in jobs:
                assert (ma.to_numpy(J["d_out"]) == J["eager"][r]).all(), "%s: replay on inputs %d differs from the eager call" % (J["shape"], r)
        del g


@pytest.mark.gpu
def test_two_host_threads_run_ga_batches_on_their_own_streams(eng, oracle):
    """4.  Two host threads, each on a stream of its own, three times each: one runs the edge rows at N = 1024 (the two-team kernel), the other 8 of them at N = 2048,
    4 x 2^9 on the paired split kernel (exchange slots and pairing words belong to the calling thread and its stream): the words are the single-thread words, which
    are the oracle's."""
    import torch
    import mosfhet_amd as ma
    jobs = []
    for shape, B, order in (("N1024 2x8", ROWS, "reference"), ("N2048 4x9", 8, "by_component")):
        H, I, W = _host_keys(oracle, shape), _inputs(shape), _expected(oracle, shape, order)
        bsk, gak = _dev_keys(eng, H)
        jobs.append((bsk, gak, ma.to_device(I["tv"][None], eng.device), ma.to_device(I["cts"][4][:B], eng.device), W[4, True, False][:B]))
    with _settings(jobs[0][0]), _settings(jobs[1][0]):
        single = [ma.to_numpy(eng.functional_bootstrap_ga(bsk, gak, d_tv, d_ct, 4)) for bsk, gak, d_tv, d_ct, _ in jobs]
        for t in range(2):
            _assert_words(single[t], jobs[t][4], "single-threaded, job %d" % t)
        torch.cuda.synchronize()
        bad, errors = [0, 0], []

        def worker(t):
            try:
                bsk, gak, d_tv, d_ct, _ = jobs[t]
                stream = torch.cuda.Stream(device=eng.device)
                with torch.cuda.stream(stream):
                    for _ in range(3):
                        got = ma.to_numpy(eng.functional_bootstrap_ga(bsk, gak, d_tv, d_ct, 4))
                        bad[t] += int(not (got == single[t]).all())
            except Exception as e:  # noqa: BLE001
                errors.append(repr(e))

        threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
    assert not errors, errors
    assert bad == [0, 0], bad


@pytest.mark.gpu
@pytest.mark.parametrize("form,B", [("wide, N1024 2x8", 9), ("one team, N1024 2x8 compile-time", 9), ("split paired, N2048 4x9", 7), ("split paired, N2048 4x9", 15),
                                    ("one team Fft2048L, N2048 4x9 reference key", 9)])
def test_a_permuted_batch_gives_the_permuted_outputs(eng, oracle, form, B):
    """4.  Position in the batch: B rows (the edge rows, random words behind them) in a random order give the outputs in that order -- the split kernel's blocks B / B + 8
    at 7 and 15 rows, one short of one and of two full tiles of eight."""
    import mosfhet_amd as ma
    shape, order, team, wide, wait, batch, family, how = FORMS[form]
    H, I = _host_keys(oracle, shape), _inputs(shape)
    bsk, gak = _dev_keys(eng, H)
    cts = _context_inputs(oracle, shape, B, 1, 0xF6 + B)[0]
    key = ("permuted", shape, B, _oracle_order(form))
    if key not in _CACHE:
        _CACHE[key] = _bootstrap_words(oracle, H, I["tv"][None], cts, 4, False, _oracle_order(form))
    perm = np.random.default_rng(B).permutation(B)
    d_tv = ma.to_device(I["tv"][None], eng.device)
    with _settings(bsk, order, team, wide, wait):
        _assert_form(eng, bsk, form, B)
        for ix in (np.arange(B), perm):
            got = _bootstrap(eng, bsk, gak, d_tv, ma.to_device(cts[ix], eng.device), 4, False, form)
            _assert_split(form, B)
            _assert_words(got, _CACHE[key][ix], "%s: %d rows in the order %s" % (form, B, list(ix)))


# ---------------------------------------------------------------- 5: refusals ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["N1024 2x8", "N2048 4x9"])
def test_short_key_sets_and_bad_arguments_are_refused_before_any_launch(eng, oracle, shape):
    """5.  mosfhet_hip_gak_t is the handle of every FFT key-switch key set, and three entry points index it by a data-dependent (gen - 1) >> 1 that reaches N - 1.  A
    2-entry set with the bootstrap key's N, t and base_bit is refused by functional_bootstrap_ga and blind_rotate_ga, and by trlwe_eval_automorphism at generator 5,
    with a message that names `entries`; at generators 1 and 3 it is accepted and gives the words of the _entry call and of the oracle.  Pinned with them: an even
    generator, generators <= 0 and >= 2N, tv_count neither 1 nor count, a key set of another N, l or Bg_bit, an unfolded bootstrap key.  Every refused call leaves a
    pattern-filled output untouched: nothing was launched."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, l, Bg = SHAPES[shape]
    H, I = _host_keys(oracle, shape), _inputs(shape)
    bsk, gak = _dev_keys(eng, H)
    rows = H["ak"][:2]
    short = eng.load_trlwe_ks_keys(rows, Bg)
    others = [eng.load_trlwe_ks_keys(np.zeros((2, l, 2, 3072 - N), dtype=U64), Bg), eng.load_trlwe_ks_keys(np.zeros((2, l + 1, 2, N), dtype=U64), Bg),
              eng.load_trlwe_ks_keys(np.zeros((2, l, 2, N), dtype=U64), Bg + 1)]
    unfolded = eng.load_bootstrap_key_unfolded(np.zeros((4, 2 * l, 2, N), dtype=U64), l, Bg, 2)
    d_tv, d_ct, d_acc = ma.to_device(I["tv"][None], eng.device), ma.to_device(I["cts"][4][:3], eng.device), ma.to_device(I["accs"][:3], eng.device)
    out_t, out_r, acc = _guarded(eng, 2, N + 1), _guarded(eng, 2, 2, N), _guarded(eng, 2, 2, N)

    def refused(call, match):
        with pytest.raises(ma.MosfhetHipError, match=match):
            call()
        torch.cuda.synchronize()
        for buf in (out_t, out_r, acc):
            assert (ma.to_numpy(buf) == U64(SENTINEL)).all(), "a refused call wrote to its output"

    try:
        refused(lambda: eng.functional_bootstrap_ga(bsk, short, d_tv, d_ct, 4, out=out_t), "entries")
        refused(lambda: eng.functional_bootstrap_ga(bsk, short, d_tv, d_ct, 4, extract=False, out=out_r), "entries")
        refused(lambda: eng.blind_rotate_ga(bsk, short, acc, d_ct), "entries")
        refused(lambda: eng.trlwe_eval_automorphism(short, d_acc, 5, out=out_r), "entries")
        refused(lambda: eng.trlwe_eval_automorphism(short, d_acc, 2 * N - 1, out=out_r), "entries")
        refused(lambda: eng.trlwe_eval_automorphism_entry(short, 2, d_acc, 5, out=out_r), "bad argument")
        for k in (short, gak):
            for gen in (2, 0, -1, 2 * N, 2 * N + 1):
                refused(lambda: eng.trlwe_eval_automorphism(k, d_acc, gen, out=out_r), "must be odd and < 2N")
        for other in others:
            refused(lambda: eng.functional_bootstrap_ga(bsk, other, d_tv, d_ct, 4, out=out_t), "must use the bootstrap key's N, l, Bg_bit")
            refused(lambda: eng.blind_rotate_ga(bsk, other, acc, d_ct), "must use the bootstrap key's N, l, Bg_bit")
        refused(lambda: eng.functional_bootstrap_ga(unfolded, gak, d_tv, d_ct, 4, out=out_t), "without unfolding")
        refused(lambda: eng.blind_rotate_ga(unfolded, gak, acc, d_ct), "without unfolding")
        two_tvs = ma.to_device(I["tvs"][:2], eng.device)
        refused(lambda: engine._check(engine.lib().mosfhet_hip_functional_bootstrap_ga_batch(eng.h, bsk.h, gak.h, engine._ptr(out_t), engine._ptr(two_tvs), 2, engine._ptr(d_ct), 3,
                                                                                             4, 1, eng._stream())), "tv_count must be 1 or count")
        # ... and what the short set does hold is served: generators 1 and 3 read entries 0 and 1
        _fill(oracle, H, [0, 1])
        for gen in (1, 3):
            got = ma.to_numpy(eng.trlwe_eval_automorphism(short, d_acc, gen))
            assert (got == ma.to_numpy(eng.trlwe_eval_automorphism_entry(short, (gen - 1) // 2, d_acc, gen))).all(), gen
            want = np.stack([oracle.trlwe_eval_automorphism(a, gen, H["ak_dft"][(gen - 1) // 2], l, Bg) for a in I["accs"][:3]])
            _assert_words(got, want, "%s: generator %d through a 2-entry set" % (shape, gen))
    finally:
        for k in [short, unfolded] + others:
            k.free()
