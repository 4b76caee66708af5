"""The plain bootstrap and external-product kernels (mosfhet_amd/csrc/bootstrap_kernels.h, external_product_kernels.h, general_kernels.h, unfold_kernels.h) at the
VALUES SET_1's team kernel is held to in tests/test_gpu_parity.py (test_rounding_bound_worst_case, test_edge_cases_empty_ragged_and_degenerate_inputs) and the Galois
kernels in tests/test_ga_edges.py.  Each of these kernels has its own transposes, row pipelines, digit paths and hand-offs and carries add_rounded<kReduce> with kReduce
decided per instantiation; uniform random words reach none of the corners below.

  1a. the value table (tests/pbs_edges_reference.py: VALUE_KINDS, value_rows): accumulators (every component) of every word 2^63, every word 2^63 - 1, the two alternating,
      zero, every digit -2^(Bg-1), every digit 2^(Bg-1) - 1, and the two digit extremes halved (so that a step of abar = N, (X^N - 1) acc = -2 acc, decomposes exactly
      them); a key of n = 3 entries (unfolded keys: 4) with every word 2^63 / every word 2^63 - 1 / the two alternating; per key entry one mask word at 2^63 (abar = N)
      or at 1 << (64 - log2 2N) (abar = 1) and every other word 0: one entry and one step live at a time.  Through blind_rotate_ in place (unfolded keys have no such
      entry point: functional_bootstrap_wo_extract with the accumulator as test vector and a body word that rotates by 0).
  1b. the mask edge rows (mask_edge_rows; L = log2(2N), word(v) = v << (64 - L)), n = 8 mask words and a body word, under a key of uniform random words:
        a  every mask word 0                                  every step skipped
        b  every mask word 2^64 - 1                           rounds up, wraps to 0
        c  alternately 2^(63-L) - 1 and 2^(63-L)              the last word that rounds to 0 and the first that rounds to 1
        d  every mask word word(N)                            pure sign flips
        e  alternately word(1) and word(2N - 1)
        f  alternately word(N - 1) and word(N + 1)
        g  word(2N - 1) + 2^(63-L)                            rounds to 2N, wraps
        h  word(3), zeros, word(2N - 3)                       exactly one live step at each end
        i  random words                                       control
      the body words make the first rotation 0, N, 2N - 1 and the wrap at 2N.  Through functional_bootstrap_wo_extract with one random test vector per ciphertext and
      through programmable_bootstrap at (3, 0, 0), with extraction.
  2.  both on every form of FORMS, the form that ran asserted from the launchers' own plan, the split launch's pairing words and the process's switches.
  3.  external_product, cmux (out of place, in place) and external_product_dft with one selector per unit at the value table, on every form of EP_FORMS.
  4.  the oracle alone against exact integer arithmetic at the same values (CPU).

Expected words are the oracle's on the same words, under oracle.product_order("by_component") where a split or by-component form runs.  Every device comparison is == on
every word; there is no tolerance anywhere on the GPU side.  Key material is planted or uniform random words: bit-exactness needs no valid key.
"""
import contextlib
import os

import numpy as np
import pytest

import ga_edges_reference as R
import pbs_edges_reference as P
from ga_edges_reference import ACC_KINDS, KEY_KINDS, digits, digit_target, exact_sums, extreme_poly, gadget_offset, largest_sum_log2, modswitch, rotate
from test_leveled_lut import _assert_words, _map

U64 = np.uint64
SENTINEL = 0x5EA75EA75EA75EA7
_CACHE = {}
ROWS = len(P.ROW_NAMES)

# (N, k, l, Bg_bit)
SHAPES = {"N1024 2x8": (1024, 1, 2, 8), "N2048 4x9": (2048, 1, 4, 9), "N2048 4x7": (2048, 1, 4, 7), "N2048 2x15": (2048, 1, 2, 15), "N2048 6x7": (2048, 1, 6, 7),
          "N4096 1x22": (4096, 1, 1, 22), "N512 k2 2x8": (512, 2, 2, 8), "N256 k3 2x8": (256, 3, 2, 8)}

SWITCH_DEFAULTS = dict(team=512, wide=512, split_max=0, wait=200000, group=-1, unfold_split=-1)
BY_COMPONENT = ("split", "latency_by_component", "throughput_by_component")


def _form(shape, kernel, unfolding=1, order="auto", family=None, split=None, pairs=None, batches=(ROWS,), **switches):
    """One entry of FORMS.  kernel: what runs (for the reader and the messages); order: the key's product order; family: what bootstrap_plan must report (None: the
    key is not one it plans -- a general ring, an unfolded key); split: how split_last_launch must say the launch was taken; pairs: what MOSFHET_HIP_WIDE_PAIRS must
    be in this process ("0": the form runs in a child process started with it); batches: the mask edge rows tiled to these sizes; switches: the launch switches
    that differ from SWITCH_DEFAULTS."""
    assert set(switches) <= set(SWITCH_DEFAULTS), switches
    return dict(shape=shape, kernel=kernel, unfolding=unfolding, order=order, family=family, split=split, pairs=pairs, batches=batches, switches=dict(SWITCH_DEFAULTS, **switches))


FORMS = {
    # the control: what test_rounding_bound_worst_case already holds
    "team, N1024 2x8":                      _form("N1024 2x8", "pbs_team_kernel<2, 8>", family="latency"),
    # N = 2048, 4 x 2^9 (compile-time)
    "wide pair, N2048 4x9":                 _form("N2048 4x9", "pbs_wide_pair_kernel<Fft2048L, 4, 9>", family="latency", pairs="1"),
    "wide team, N2048 4x9":                 _form("N2048 4x9", "pbs_wide_team_kernel<Fft2048, 4, 9>", family="latency", pairs="0"),
    "throughput, N2048 4x9":                _form("N2048 4x9", "pbs_kernel<Fft2048, 4, 9>", family="throughput", wide=0),
    "split paired, N2048 4x9":              _form("N2048 4x9", "pbs_split_kernel<Fft2048L, 4, 9>", family="split", split="paired", batches=(9, 17), split_max=-1),
    "split alone, N2048 4x9":               _form("N2048 4x9", "pbs_split_kernel<Fft2048L, 4, 9>", family="split", split="alone", batches=(9, 17), split_max=-1, wait=0),
    "by-component latency, N2048 4x9":      _form("N2048 4x9", "pbs_split_kernel<Fft2048L, 4, 9, SOLO>", order="by_component", family="latency_by_component"),
    "by-component throughput, N2048 4x9":   _form("N2048 4x9", "pbs_kernel<Fft2048, 4, 9, BYC>", order="by_component", family="throughput_by_component", wide=0),
    # N = 2048, run-time and other gadgets
    "split paired, N2048 4x7 run-time":     _form("N2048 4x7", "pbs_split_kernel<Fft2048L, 4, 0>", family="split", split="paired", batches=(9, 17), split_max=-1),
    "wide pair, N2048 4x7 run-time":        _form("N2048 4x7", "pbs_wide_pair_kernel<Fft2048L, 4, 0>", family="latency", pairs="1"),
    "split paired, N2048 2x15 run-time":    _form("N2048 2x15", "pbs_split_kernel<Fft2048L, 2, 0> (TAIL only)", family="split", split="paired", batches=(9, 17), split_max=-1),
    "throughput, N2048 2x15 run-time":      _form("N2048 2x15", "pbs_kernel<Fft2048, 2, 0>", family="throughput", wide=0),
    "split paired, N2048 6x7":              _form("N2048 6x7", "pbs_split_kernel<Fft2048L, 6, 7> (QUADS + TAIL)", family="split", split="paired", batches=(9, 17), split_max=-1),
    "wide pair, N2048 6x7 run-time":        _form("N2048 6x7", "pbs_wide_pair_kernel<Fft2048L, 6, 0>", family="latency", pairs="1"),
    # N = 4096
    "latency, N4096 1x22":                  _form("N4096 1x22", "pbs_wide_team_kernel<Fft4096, 1, 0>", family="latency"),
    "throughput, N4096 1x22":               _form("N4096 1x22", "pbs_kernel<Fft4096, 1, 0>", family="throughput", wide=0),
    # general rings: the smallest k = 2 and k = 3 shapes of test_general_rings_and_k_bit_exact
    "general, N512 k2 2x8":                 _form("N512 k2 2x8", "pbs_general_kernel"),
    "general, N256 k3 2x8":                 _form("N256 k3 2x8", "pbs_general_kernel"),
    # unfolded keys
    "unfolding 2 selectors first, N1024":   _form("N1024 2x8", "unfold2_select_kernel + ubr_phase2_wide_kernel<Fft1024>", unfolding=2),
    "unfolding 2 one kernel, N1024":        _form("N1024 2x8", "pbs_unfold2_kernel", unfolding=2, unfold_split=0),
    "unfolding 4 selectors first, N1024":   _form("N1024 2x8", "ubr_phase1_kernel + ubr_phase2_kernel<Fft1024>", unfolding=4, team=0),
    "unfolding 4 one kernel, N1024":        _form("N1024 2x8", "pbs_unfolded_kernel", unfolding=4, unfold_split=0),
    "unfolding 2 selectors first, N2048":   _form("N2048 4x9", "unfold2_select_kernel + ubr_phase2_wide_kernel<Fft2048>", unfolding=2),
}
IN_PROCESS = [f for f in FORMS if FORMS[f]["pairs"] != "0"]


def _oracle_order(form):
    return "by_component" if FORMS[form]["family"] in BY_COMPONENT else "reference"


def _rand(rng, *shape):
    return rng.integers(0, 2 ** 64, size=shape, dtype=U64)


def _log2(x):
    return float(np.log2(max(float(x), 1.0)))


# ---------------------------------------------------------------- keys and expected words ----------------------------------------------------------------
def _host_key(oracle, shape, unfolding=1, planted=False):
    """dict(words, dft, n, ...): a bootstrap key [n][(k+1)l][k+1][N] (unfolded: its n 2^u / u samples [..][2l][2][N]) of uniform random words over n = 8 mask words,
    or planted: entry (sample) i holds every word 2^63 / every word 2^63 - 1 / the two alternating by coefficient, by i % 3, in every row and component, over
    n = 3 mask words (unfolded: 4)"""
    key = ("host", shape, unfolding, planted)
    if key in _CACHE:
        return _CACHE[key]
    N, k, l, Bg = SHAPES[shape]
    oracle.plan(N)
    n = (3 if unfolding == 1 else 4) if planted else P.N_MASK
    count = n if unfolding == 1 else n * (1 << unfolding) // unfolding
    if planted:
        words = np.empty((count, (k + 1) * l, k + 1, N), dtype=U64)
        for i in range(count):
            words[i] = extreme_poly(KEY_KINDS[i % 3], N, l, Bg)
    else:
        words = _rand(np.random.default_rng(0xB5 + N + 16 * l + Bg + 1000 * unfolding + k), count, (k + 1) * l, k + 1, N)
    H = dict(shape=shape, unfolding=unfolding, planted=planted, N=N, k=k, l=l, Bg=Bg, n=n, words=words)
    if unfolding == 1:
        H["dft"] = oracle.bk_to_dft(words, k, l)
    elif unfolding == 2:
        H["dft"] = oracle.su_to_dft(words, l)
    _CACHE[key] = H
    return H


def _want_bootstrap(oracle, H, tv, c, pre):
    """functional_bootstrap_wo_extract at torus_base 4 (pre False) / programmable_bootstrap at (3, 0, 0) (pre True) of one ciphertext"""
    N, l, Bg, u = H["N"], H["l"], H["Bg"], H["unfolding"]
    if u == 1:
        return oracle.programmable_bootstrap(tv, c, H["dft"], l, Bg, 3, 0, 0) if pre else oracle.functional_bootstrap_wo_extract(tv, c, H["dft"], l, Bg, 4)
    if pre:
        c = oracle.pbs_preprocess(c, N, 0, 0)                    # programmable_bootstrap = scaled input + functional_bootstrap (src/bootstrap.c:208-219)
    if u == 2:
        return oracle.functional_bootstrap_unfolded2_dft(tv, c, H["dft"], l, Bg, 4, extract=pre)
    return oracle.functional_bootstrap_unfolded(tv, c, H["words"], l, Bg, 4, u, extract=pre)


def _want_rotation(oracle, H, acc, row):
    """what the value table's call gives for one accumulator and one row"""
    if H["unfolding"] == 1:
        return oracle.blind_rotate(acc, row[:-1].copy(), H["dft"], H["l"], H["Bg"])
    return _want_bootstrap(oracle, H, acc, row, False)


def _value_inputs(H, which):
    """(accs [16][k+1][N], rows [16][n+1]) of the value table for key entry `which`: accumulator kind j under the abar = N row at 2 j, under the abar = 1 row at
    2 j + 1.  Unfolded keys go through the bootstrap: the body word makes its first rotation 0."""
    N, k, l, Bg, n = H["N"], H["k"], H["l"], H["Bg"], H["n"]
    two = P.value_rows(which, n, N)
    if H["unfolding"] > 1:
        two[:, -1] = U64((-R.prec_offset(4)) & R.MASK64)
    accs = np.stack([np.stack([P.value_poly(kind, N, l, Bg)] * (k + 1)) for kind in P.VALUE_KINDS for _ in range(2)])
    return accs, np.ascontiguousarray(np.concatenate([two] * len(P.VALUE_KINDS)))


def _value_expected(oracle, shape, unfolding, order):
    """[n][16][k+1][N], computed once per (shape, unfolding, order)"""
    key = ("value", shape, unfolding, order)
    if key not in _CACHE:
        H = _host_key(oracle, shape, unfolding, planted=True)
        out = []
        with oracle.product_order(order):
            for which in range(H["n"]):
                accs, rows = _value_inputs(H, which)
                out.append(np.stack(_map(lambda b: _want_rotation(oracle, H, accs[b], rows[b]), range(len(rows)))))
        _CACHE[key] = out
    return _CACHE[key]


def _row_inputs(shape):
    """dict(cts [9][9] at torus_base 4, tvs [9][k+1][N] random words)"""
    key = ("rows", shape)
    if key not in _CACHE:
        N, k, l, Bg = SHAPES[shape]
        _CACHE[key] = dict(cts=P.mask_edge_rows(N, 4), tvs=_rand(np.random.default_rng(0xC5 + N + k), ROWS, k + 1, N))
    return _CACHE[key]


def _row_expected(oracle, shape, unfolding, order):
    """dict(wo [9][k+1][N], pb [9][k N + 1]), computed once per (shape, unfolding, order)"""
    key = ("row words", shape, unfolding, order)
    if key not in _CACHE:
        H, I = _host_key(oracle, shape, unfolding), _row_inputs(shape)
        with oracle.product_order(order):
            _CACHE[key] = {name: np.stack(_map(lambda b: _want_bootstrap(oracle, H, I["tvs"][b], I["cts"][b], pre), range(ROWS))) for name, pre in (("wo", False), ("pb", True))}
    return _CACHE[key]


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_value_table_digits_are_at_the_extremes(shape):
    """From ga_edges_reference.digits: at every shape used, the two digits_* kinds have every digit at -2^(Bg-1) and at 2^(Bg-1) - 1, and so has -2 x their halved
    forms, which is what the step abar = N of the value table decomposes; the value rows round to N and to 1 at the live word and to 0 (skipped) elsewhere."""
    N, k, l, Bg = SHAPES[shape]
    lo, hi = -(1 << (Bg - 1)), (1 << (Bg - 1)) - 1
    assert (digits(extreme_poly("digits_lo", N, l, Bg), l, Bg) == lo).all() and (digits(extreme_poly("digits_hi", N, l, Bg), l, Bg) == hi).all()
    assert (digits(np.zeros(N, dtype=U64), l, Bg) == 0).all()
    assert digit_target(l, Bg, 0) == (-gadget_offset(l, Bg)) % 2 ** 64
    for kind, want in (("digits_lo halved", lo), ("digits_hi halved", hi)):
        c = P.value_poly(kind, N, l, Bg)
        stepped = np.array(rotate([int(x) for x in c], N, N), dtype=U64) - c          # (X^N - 1) c
        assert (stepped == U64(0) - c - c).all() and (digits(stepped, l, Bg) == want).all(), kind
    for n in (3, 4):
        for which in range(n):
            rows = P.value_rows(which, n, N)
            assert P.steps(rows[0], N) == [N if i == which else 0 for i in range(n)] and P.steps(rows[1], N) == [1 if i == which else 0 for i in range(n)]
            assert modswitch((int(rows[0, -1]) - R.prec_offset(4) + R.prec_offset(4)) & R.MASK64, N) == 0


@pytest.mark.parametrize("N", [256, 512, 1024, 2048, 4096])
def test_mask_edge_rows_reach_what_they_claim(N):
    """Per row the steps the table of the module docstring names, in Python integers; the body words round to 0, N, 2N - 1 and 2N (wraps) at torus_base 4."""
    top, L = 2 * N - 1, R.log2n2(N)
    cts = P.mask_edge_rows(N, 4)
    assert cts.shape == (ROWS, P.N_MASK + 1)
    s = {name: P.steps(cts[r], N) for r, name in enumerate(P.ROW_NAMES)}
    assert s["a"] == [0] * 8 and s["b"] == [0] * 8 and s["g"] == [0] * 8
    assert [((int(x) + (1 << (63 - L))) >> (64 - L)) for x in cts[6, :8]] == [2 * N] * 8           # ... row g by wrapping from 2N
    assert s["c"] == [0, 1] * 4 and s["d"] == [N] * 8 and s["e"] == [1, top] * 4 and s["f"] == [N - 1, N + 1] * 4
    assert s["h"] == [3] + [0] * 6 + [top - 2]
    assert sum(1 for x in s["i"] if x) >= 6
    bbar = [R.body_exponent(row, N, 4) for row in cts]
    raw = [((int(row[-1]) + R.prec_offset(4)) % 2 ** 64 + (1 << (63 - L))) >> (64 - L) for row in cts]
    assert bbar[:4] == [0, N, top, 0] and raw[3] == 2 * N and bbar[4:8] == [0, N, 1, N + 1], (bbar, raw)
    m = list(range(1, N + 1))
    assert rotate(m, N, N) == [2 ** 64 - x for x in m] and rotate(m, 1, N) == [2 ** 64 - m[-1]] + m[:-1] and rotate(m, 0, N) == m


# the gadgets of the issue's table and the general shape the device runs: (N, k, l, Bg)
ORACLE_SHAPES = ["N1024 2x8", "N2048 4x9", "N2048 4x7", "N2048 2x15", "N4096 1x22", "N2048 6x7", "N512 k2 2x8"]
ORACLE_FRACTION_LOG2 = -50.2          # the worst distance measured, as a fraction of the magnitude bound (test_oracle_external_product_against_exact_sums)


def _magnitude_bound_log2(shape):
    N, k, l, Bg = SHAPES[shape]
    return ((k + 1) * l - 1).bit_length() + (N.bit_length() - 1) + Bg - 1 + 63


@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_oracle_external_product_against_exact_sums(oracle, shape):
    """4.  The oracle alone: oracle.external_product on every unit of section 3's table (ACC_KINDS x KEY_KINDS), in both product orders, against exact_sums reduced
    mod 2^64.  Measured, as a fraction of the magnitude bound 2^(ceil log2 (k+1)l + log2 N + Bg - 1 + 63) of the exact sums, worst over units, components and both
    orders:
        N1024 2x8 2^-50.7 (bound 2^82)   N2048 4x9 2^-50.4 (2^85)   N2048 4x7 2^-50.4 (2^83)   N2048 2x15 2^-50.4 (2^90)   N4096 1x22 2^-50.2 (2^97)
        N2048 6x7 2^-50.4 (2^84)         N512 k2 2x8 2^-50.7 (2^82)
    asserted: four times the worst of these, 2^-48.2 -- the factor is for shapes and seeds not tried.  So the oracle is a sound expected value at these extremes.
    Per shape the largest exact sum reaches the bound: past 2^83, where rounding without the reduction mod 2^64 is no longer exact (cmux_steps.h:
    kProductNeedsReduce), at every tuned gadget but SET_1's, where it stays at 2^82."""
    N, k, l, Bg = SHAPES[shape]
    bound = _magnitude_bound_log2(shape)
    worst, largest = 0.0, 0.0
    for kk, key_kind in enumerate(KEY_KINDS):
        g = np.empty(((k + 1) * l, k + 1, N), dtype=U64)
        g[:] = extreme_poly(key_kind, N, l, Bg)
        g_dft = oracle.trgsw_to_dft(g, k, l)
        for acc_kind in ACC_KINDS:
            p = extreme_poly(acc_kind, N, l, Bg)
            c = np.stack([p] * (k + 1))
            d = np.concatenate([digits(p, l, Bg)] * (k + 1))
            sums = exact_sums(d, g[:, 0])                                                  # every component of the key holds the same rows: one sum serves all k + 1 outputs
            largest = max(largest, _log2(max(abs(x) for x in sums)))
            want = np.array([x % 2 ** 64 for x in sums], dtype=U64)
            for order in ("reference", "by_component"):
                with oracle.product_order(order):
                    got = oracle.external_product(c, g_dft, l, Bg)
                worst = max(worst, float(oracle.torus_dist(got, want[None]).max()))
    print("%s: bound 2^%d, largest exact sum 2^%.2f, worst torus distance 2^%.1f = 2^%.1f of the bound" % (shape, bound, largest, _log2(worst), _log2(worst) - bound))
    assert _log2(worst) - bound < ORACLE_FRACTION_LOG2 + 2, (shape, _log2(worst) - bound)
    reach = float(np.log2((k + 1) * l)) + (N.bit_length() - 1) + Bg - 1 + 63          # (k+1) l N products of a digit -2^(Bg-1) with a key word -2^63
    assert abs(largest - reach) < 0.01 and reach <= bound, (shape, largest, reach, bound)
    if shape == "N1024 2x8":
        assert largest <= 82
    elif k == 1:
        assert largest >= 83 and (shape == "N2048 4x7" or largest > 83), (shape, largest)          # (4 x 2^7: exactly 2^83, and a run-time gadget, which always reduces)
    assert largest_sum_log2(np.concatenate([digits(extreme_poly("digits_lo", N, l, Bg), l, Bg)] * (k + 1)), g[:, 0]) <= bound


def _real_key(oracle, shape):
    """a real key at n = 8, sigma 2^-50, binary keys"""
    key = ("real", shape)
    if key not in _CACHE:
        N, k, l, Bg = SHAPES[shape]
        rng = oracle.Rng(0x9B5 + N)
        lwe_s, s = oracle.gen_binary_key(rng, P.N_MASK), oracle.gen_binary_key(rng, N)
        bk = oracle.gen_bootstrap_key(rng, lwe_s, s.reshape(1, N), l, Bg, 2.0 ** -50)
        _CACHE[key] = dict(lwe_s=lwe_s, s=s, bk=bk, bk_dft=oracle.bk_to_dft(bk, 1, l))
    return _CACHE[key]


@pytest.mark.parametrize("shape,measured", [("N1024 2x8", 53.78), ("N2048 4x9", 34.98)])
def test_oracle_on_the_mask_edge_rows_against_exact_arithmetic(oracle, shape, measured):
    """4.  The oracle alone with a REAL key (n = 8, sigma 2^-50, binary keys): for every mask edge row the phase of functional_bootstrap_wo_extract is the exact
    negacyclic rotation X^e m of the test vector's message by e = (-bbar + sum_i abar_i s_i) mod 2N, computed with Python integers, in both product orders.  Measured:
    worst torus distance 2^53.78 at N = 1024, 2 x 2^8 (the decomposition's rounding, 2^47 per coefficient) and 2^34.98 at N = 2048, 4 x 2^9 (2^27 per coefficient); asserted: 4 x that -- the
    factor is for the seed -- which stays below 2^58, a sixteenth of the table's message spacing of 2^62.  A wrong rounding of a mask word, a skipped or extra step or
    a wrong rotation sign moves a phase by a whole message or scrambles it."""
    N, k, l, Bg = SHAPES[shape]
    K = _real_key(oracle, shape)
    tv = oracle.trlwe_torus_packing(np.array([3 << 60, 7 << 60, 11 << 60, 15 << 60], dtype=U64), 1, N)
    assert (tv[0] == 0).all()
    msg = [int(x) for x in tv[1]]
    worst = 0.0
    for order in ("reference", "by_component"):
        for r, row in enumerate(P.mask_edge_rows(N, 4)):
            with oracle.product_order(order):
                out = oracle.functional_bootstrap_wo_extract(tv, row, K["bk_dft"], l, Bg, 4)
            e = (-R.body_exponent(row, N, 4) + sum(a * int(si) for a, si in zip(P.steps(row, N), K["lwe_s"]))) % (2 * N)
            dist = float(oracle.torus_dist(oracle.trlwe_phase(out, K["s"].reshape(1, N)), np.array(rotate(msg, e, N), dtype=U64)).max())
            print("%s, %s order, row %s: e = %d, log2 distance %.1f" % (shape, order, P.ROW_NAMES[r], e, _log2(dist)))
            worst = max(worst, dist)
    bound = 4 * 2.0 ** measured
    print("%s: worst log2 distance %.2f, bound %.2f" % (shape, _log2(worst), _log2(bound)))
    assert bound < 2.0 ** 58
    assert worst < bound, _log2(worst)


def test_reference_build_on_the_mask_edge_rows(oracle):
    """4.  Where oracle/_ref is built: the mask edge rows through the reference's own programmable_bootstrap at N = 1024, 2 x 2^8 with the real key, against the
    oracle in both product orders under the criterion of test_by_component_product_order_is_held_to_the_reference_too (2^38 on the ciphertext)."""
    from oracle import reflib
    backends = [b for b in ("avx512", "ffnt") if reflib.available(b)]
    if not backends:
        pytest.skip("oracle/_ref not built")
    shape = "N1024 2x8"
    N, k, l, Bg = SHAPES[shape]
    K = _real_key(oracle, shape)
    tv = oracle.trlwe_torus_packing(np.array([3 << 60, 7 << 60, 11 << 60, 15 << 60], dtype=U64), 1, N)
    for backend in backends:
        ref = reflib.get(backend)
        ref.init(N)
        h = ref.bk_new(K["bk"], 1, l, Bg)
        try:
            for r, row in enumerate(P.mask_edge_rows(N, 4)):
                theirs = ref.programmable_bootstrap(tv, row, h, 3, 0, 0)
                for order in ("reference", "by_component"):
                    with oracle.product_order(order):
                        mine = oracle.programmable_bootstrap(tv, row, K["bk_dft"], l, Bg, 3, 0, 0)
                    dist = float(oracle.torus_dist(mine, theirs).max())
                    print("%s, %s order, row %s: log2 distance %.1f" % (backend, order, P.ROW_NAMES[r], _log2(dist)))
                    assert dist < 2.0 ** 38, (backend, order, P.ROW_NAMES[r], _log2(dist))
        finally:
            ref.bk_free(h)


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    _free_device_keys()
    e.close()


def _free_device_keys():
    for key in [k for k in _CACHE if k[0] == "dev"]:
        _CACHE.pop(key).free()


def _dev_key(eng, H):
    key = ("dev", H["shape"], H["unfolding"], H["planted"])
    if key not in _CACHE:
        if H["unfolding"] == 1:
            _CACHE[key] = eng.load_bootstrap_key(H["words"], H["k"], H["l"], H["Bg"])
        else:
            _CACHE[key] = eng.load_bootstrap_key_unfolded(H["words"], H["l"], H["Bg"], H["unfolding"])
    return _CACHE[key]


@contextlib.contextmanager
def _settings(bsk, form):
    """the switches that choose the form, restored on every way out"""
    from mosfhet_amd import engine
    F = FORMS[form]
    sw = F["switches"]
    try:
        engine.set_split_max_batch(sw["split_max"])
        engine.set_split_wait_limit(sw["wait"])
        engine.set_team_max_batch(sw["team"])
        engine.set_wide_team_max_batch(sw["wide"])
        engine.set_pbs_group(sw["group"])
        engine.set_unfold_split_max(sw["unfold_split"])
        engine.set_ep_plain_loop(0)
        if F["unfolding"] == 1:
            bsk.set_product_order(F["order"])
        yield
    finally:
        if F["unfolding"] == 1:
            bsk.set_product_order("auto")
        engine.set_ep_plain_loop(0)
        engine.set_unfold_split_max(-1)
        engine.set_pbs_group(-1)
        engine.set_wide_team_max_batch(512)
        engine.set_team_max_batch(512)
        engine.set_split_wait_limit(200000)
        engine.set_split_max_batch(-1)


def _assert_form(eng, bsk, form, B):
    """in front of the calls: the launchers' own decision for this key and batch at the current switches, and the process-wide switch between the two latency
    kernels of N = 2048.  A form whose kernel would not run fails here."""
    F = FORMS[form]
    if F["family"] is not None:
        plan = eng.bootstrap_plan(bsk, B)
        assert plan["family"] == F["family"] and plan["by_component"] == (F["family"] in BY_COMPONENT), (form, B, plan)
    else:
        info = eng.bootstrap_key_info(bsk)
        assert info[5] == F["unfolding"] and ((info[1] > 1 or info[2] not in (1024, 2048, 4096)) == F["kernel"].startswith("pbs_general")), (form, info)
    if F["pairs"] is not None:
        env = os.environ.get("MOSFHET_HIP_WIDE_PAIRS")
        on = True if env is None else (int(env) != 0)
        assert on == (F["pairs"] == "1"), "%s: MOSFHET_HIP_WIDE_PAIRS=%r in this process, %s would not run" % (form, env, F["kernel"])


def _assert_ran(form, B):
    """behind a call: how the split launch was taken (the launcher's own account, per host thread)"""
    from mosfhet_amd import engine
    how = FORMS[form]["split"]
    if how:
        assert engine.split_last_launch() == ((B, B, 0) if how == "paired" else (B, 0, B)), (form, engine.split_last_launch())


def _guarded(eng, B, *row):
    """an output of B rows with a sentinel-filled guard row on either side: (buffer, the B rows in the middle)"""
    import torch
    buf = torch.full((B + 2,) + row, SENTINEL, dtype=torch.int64, device=eng.device)
    return buf, buf[1:B + 1]


def _checked(buf, B, what):
    import mosfhet_amd as ma
    got = ma.to_numpy(buf)
    assert (got[0] == U64(SENTINEL)).all(), "%s wrote in front of its first output" % what
    assert (got[B + 1] == U64(SENTINEL)).all(), "%s wrote past its last output" % what
    return got[1:B + 1]


def _run_value_rows(eng, bsk, H, accs, rows, what):
    """the value table's call on the device: blind_rotate_ in place on a guarded copy of the accumulators (unfolded: functional_bootstrap_wo_extract, see _value_inputs)"""
    import mosfhet_amd as ma
    B = len(rows)
    buf, mid = _guarded(eng, B, H["k"] + 1, H["N"])
    d_ct = ma.to_device(rows, eng.device)
    if H["unfolding"] == 1:
        mid.copy_(ma.to_device(accs, eng.device))
        eng.blind_rotate_(bsk, mid, d_ct)
    else:
        eng.functional_bootstrap_wo_extract(bsk, ma.to_device(accs, eng.device), d_ct, 4, out=mid)
    return _checked(buf, B, what)


def _value_table_case(eng, oracle, form):
    """1a on one form.  Returns the number of outputs compared.  (Module level: the wide-team form runs it in a child process.)"""
    F = FORMS[form]
    H = _host_key(oracle, F["shape"], F["unfolding"], planted=True)
    W = _value_expected(oracle, F["shape"], F["unfolding"], _oracle_order(form))
    bsk = _dev_key(eng, H)
    compared = 0
    with _settings(bsk, form):
        for which in range(H["n"]):
            accs, rows = _value_inputs(H, which)
            what = "%s (%s): value table, key entry %d" % (form, F["kernel"], which)
            _assert_form(eng, bsk, form, len(rows))
            got = _run_value_rows(eng, bsk, H, accs, rows, what)
            _assert_ran(form, len(rows))
            bad = ["%s under abar = %s" % (P.VALUE_KINDS[b // 2], "1" if b % 2 else "N") for b in range(len(rows)) if not (got[b] == W[which][b]).all()]
            assert not bad, "%s: %d of %d outputs differ from the oracle: %s" % (what, len(bad), len(rows), bad)
            compared += len(rows)
    return compared


def _mask_rows_case(eng, oracle, form):
    """1b on one form.  Returns the number of outputs compared."""
    import torch
    import mosfhet_amd as ma
    F = FORMS[form]
    H, I = _host_key(oracle, F["shape"], F["unfolding"]), _row_inputs(F["shape"])
    W = _row_expected(oracle, F["shape"], F["unfolding"], _oracle_order(form))
    N, k = H["N"], H["k"]
    bsk = _dev_key(eng, H)
    once = F["family"] is None and F["unfolding"] == 1 or N == 4096                 # the general rings and N = 4096: the row set once
    orders = [np.arange(ROWS)] if once else [np.arange(ROWS), np.roll(np.arange(ROWS), 1), np.concatenate([np.arange(4), [8], np.arange(4, 8)])]
    orders += [np.arange(B) % ROWS for B in F["batches"] if B != ROWS]
    compared = 0
    with _settings(bsk, form):
        for j, idx in enumerate(orders):
            B = len(idx)
            d_tv, d_ct = ma.to_device(I["tvs"][idx], eng.device), ma.to_device(I["cts"][idx], eng.device)
            keep = [d_tv.clone(), d_ct.clone()]
            _assert_form(eng, bsk, form, B)
            for name in (("wo", "pb") if j == 0 or B != ROWS else ("wo",)):           # the permuted orders: position independence, one entry point
                what = "%s (%s): mask edge rows in the order %s, %s" % (form, F["kernel"], list(idx), "programmable_bootstrap" if name == "pb" else "functional_bootstrap_wo_extract")
                if name == "wo":
                    buf, mid = _guarded(eng, B, k + 1, N)
                    eng.functional_bootstrap_wo_extract(bsk, d_tv, d_ct, 4, out=mid)
                else:
                    buf, mid = _guarded(eng, B, k * N + 1)
                    eng.programmable_bootstrap(bsk, d_tv, d_ct, 3, 0, 0, out=mid)
                _assert_ran(form, B)
                got = _checked(buf, B, what)
                bad = [P.ROW_NAMES[idx[b]] + "@%d" % b for b in range(B) if not (got[b] == W[name][idx[b]]).all()]
                assert not bad, "%s: %d of %d outputs differ from the oracle: rows %s" % (what, len(bad), B, bad)
                compared += B
            assert torch.equal(d_tv, keep[0]) and torch.equal(d_ct, keep[1]), "%s changed its inputs" % form
    return compared


def _in_a_child_process(form, case):
    """pbs_wide_team_kernel at N = 2048, even l: a small batch takes pbs_wide_pair_kernel unless MOSFHET_HIP_WIDE_PAIRS=0, which is read once per process -- so in a
    fresh child process, as test_preprocessing_range_wide_team_kernel does"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = {k: v for k, v in os.environ.items() if not k.startswith(("MOSFHET_HIP_WIDE", "MOSFHET_HIP_SPLIT"))}
    e.update(MOSFHET_HIP_WIDE_PAIRS="0")
    e["PYTHONPATH"] = root + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _PROBE, form, case], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=e, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


_PROBE = r"""
import os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import mosfhet_amd as ma
from oracle import oracle as O
import test_pbs_value_edges as T
O.build()
eng = ma.Engine(0)
form = sys.argv[1]
for case in sys.argv[2].split(","):
    print("COMPARED", case, getattr(T, case)(eng, O, form))
T._free_device_keys()
eng.close()
"""


@pytest.mark.gpu
@pytest.mark.parametrize("form", IN_PROCESS)
def test_value_table_on_every_form(eng, oracle, form):
    """1a, 2.  The value table through one form, the form asserted: every word equals the oracle's, the guard rows either side of the accumulators keep their pattern.
    One key entry and one step are live per row, so a differing output names the accumulator kind, the rotation and the entry."""
    H = _host_key(oracle, FORMS[form]["shape"], FORMS[form]["unfolding"], planted=True)
    assert _value_table_case(eng, oracle, form) == H["n"] * 2 * len(P.VALUE_KINDS)


@pytest.mark.gpu
@pytest.mark.parametrize("form", IN_PROCESS)
def test_mask_edge_rows_on_every_form(eng, oracle, form):
    """1b, 2.  The mask edge rows through one form, the form asserted, with one test vector per ciphertext: functional_bootstrap_wo_extract and programmable_bootstrap
    at (3, 0, 0); the rows in three orders (the random row first, in the middle, last: position independence); on the split forms also tiled to 17 (block pairs
    B / B + 8, a ragged group of eight, row a -- every step skipped -- in both halves of a pairing).  Inputs unchanged, guard rows intact."""
    F = FORMS[form]
    once = F["family"] is None and F["unfolding"] == 1 or SHAPES[F["shape"]][0] == 4096
    assert _mask_rows_case(eng, oracle, form) == (2 * ROWS if once else 4 * ROWS) + sum(2 * B for B in F["batches"] if B != ROWS)


@pytest.mark.gpu
def test_both_tables_on_the_wide_team_kernel(native_lib):
    """1a, 1b, 2 on pbs_wide_team_kernel<Fft2048, 4, 9>, in a child process started with MOSFHET_HIP_WIDE_PAIRS=0 (the form asserts that it is)."""
    out = _in_a_child_process("wide team, N2048 4x9", "_value_table_case,_mask_rows_case")
    assert "COMPARED _value_table_case %d" % (3 * 2 * len(P.VALUE_KINDS)) in out and "COMPARED _mask_rows_case %d" % (4 * ROWS) in out, out[-2000:]


# ---------------------------------------------------------------- 3: external product and CMUX ----------------------------------------------------------------
# form: (shape, units per call: the six accumulator kinds tiled to this many, set_ep_plain_loop, the kernel that runs)
EP_FORMS = {
    "N1024 2x8, 6 units":             ("N1024 2x8", 6, 0, "external_product_kernel<Fft1024, 2, 8> (fewer than 64 units)"),
    "N1024 2x8, 70 units":            ("N1024 2x8", 70, 0, "external_product_ldskey_kernel<2, 8> (64 units and more, one key entry)"),
    "N2048 4x9, default loop":        ("N2048 4x9", 6, 0, "external_product_kernel<Fft2048L, 4, 9>: row pairs, the loop the launcher takes"),
    "N2048 4x9, plain loop":          ("N2048 4x9", 6, 1, "external_product_kernel<Fft2048L, 4, 9>: row pairs, the plain loop"),
    "N2048 4x7 run-time":             ("N2048 4x7", 6, 0, "external_product_kernel<Fft2048L, 4, 0>"),
    "N4096 1x22":                     ("N4096 1x22", 6, 0, "external_product_kernel<Fft4096, 1, 0>"),
    "N512 k2 2x8":                    ("N512 k2 2x8", 6, 0, "external_product_general_kernel"),
}


def _ep_expected(oracle, shape):
    """[3 key kinds][6 accumulator kinds][k+1][N]: oracle.external_product of the unit (every component the accumulator kind) with the planted entry"""
    key = ("ep", shape)
    if key not in _CACHE:
        N, k, l, Bg = SHAPES[shape]
        H = _host_key(oracle, shape, planted=True)
        cts = np.stack([np.stack([extreme_poly(kind, N, l, Bg)] * (k + 1)) for kind in ACC_KINDS])
        _CACHE[key] = cts, np.stack([np.stack([oracle.external_product(c, H["dft"][j], l, Bg) for c in cts]) for j in range(3)])
    return _CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(EP_FORMS))
def test_external_product_and_cmux_at_the_value_table(eng, oracle, form):
    """3.  Units ACC_KINDS x KEY_KINDS: external_product; cmux out of place and in place with in0 random words and in1 = in0 + the unit, so that the kernel's own
    subtraction yields the extreme digits; on the tuned rings external_product_dft with ONE SELECTOR PER UNIT (key_stride != 0; caller-held DFT content: the reducing
    instantiation), finished by dft_to_torus.  Every word equals the oracle's; inputs unchanged, guard rows intact."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    shape, units, plain, kernel = EP_FORMS[form]
    N, k, l, Bg = SHAPES[shape]
    H = _host_key(oracle, shape, planted=True)
    cts6, want6 = _ep_expected(oracle, shape)
    bsk = _dev_key(eng, H)
    idx = np.arange(units) % len(ACC_KINDS)
    cts = cts6[idx]
    in0 = _rand(np.random.default_rng(0xD5 + N), units, k + 1, N)
    d_ct, d_in0, d_in1 = ma.to_device(cts, eng.device), ma.to_device(in0, eng.device), ma.to_device(in0 + cts, eng.device)
    keep = [d_ct.clone(), d_in0.clone(), d_in1.clone()]
    try:
        engine.set_ep_plain_loop(plain)
        for j, key_kind in enumerate(KEY_KINDS):
            what = "%s (%s), key entry of kind %s" % (form, kernel, key_kind)
            buf, mid = _guarded(eng, units, k + 1, N)
            eng.external_product(bsk, j, d_ct, out=mid)
            _assert_words(_checked(buf, units, what), want6[j][idx], what + ": external_product")
            buf, mid = _guarded(eng, units, k + 1, N)
            eng.cmux(bsk, j, d_in0, d_in1, out=mid)
            _assert_words(_checked(buf, units, what), in0 + want6[j][idx], what + ": cmux")
            buf, mid = _guarded(eng, units, k + 1, N)
            mid.copy_(d_in0)
            eng.cmux(bsk, j, mid, d_in1, out=mid)
            _assert_words(_checked(buf, units, what), in0 + want6[j][idx], what + ": cmux in place")
        if k == 1 and units == len(ACC_KINDS):
            sel = eng.trgsw_to_dft(ma.to_device(H["words"][np.repeat(np.arange(3), units)], eng.device))          # [18][2l][2][N]: one selector per unit
            d_all = ma.to_device(np.concatenate([cts] * 3), eng.device)
            dft = eng.external_product_dft(sel, d_all, l, Bg)
            back = ma.to_numpy(eng.dft_to_torus(dft.reshape(-1, N))).reshape(3 * units, 2, N)
            _assert_words(back, want6.reshape(3 * units, 2, N), "%s: external_product_dft with a selector per unit" % form)
    finally:
        engine.set_ep_plain_loop(0)
    for t, t0 in zip([d_ct, d_in0, d_in1], keep):
        assert torch.equal(t, t0), "%s changed its inputs" % form
    if shape == "N2048 4x9":
        assert engine.ep_kernel_info(), "the multi-wavefront instantiation was not launched"


@pytest.mark.gpu
def test_key_view_over_the_planted_rows_gives_the_owned_keys_words(eng, oracle):
    """3.  At N = 1024, 2 x 2^8 an owned key takes the instantiation that rounds WITHOUT the reduction, a non-owning view (bootstrap_key_view) over the same rows the
    reducing one (gadget_dispatch: bounded): on the planted rows, where the sums stand at the 2^82 bound, both give the oracle's words -- external_product on few and
    on 70 units, and the value table through blind_rotate_ on the team kernel."""
    import mosfhet_amd as ma
    shape, form = "N1024 2x8", "team, N1024 2x8"
    N, k, l, Bg = SHAPES[shape]
    H = _host_key(oracle, shape, planted=True)
    cts6, want6 = _ep_expected(oracle, shape)
    owned = _dev_key(eng, H)
    view = eng.bootstrap_key_view(eng.trgsw_to_dft(ma.to_device(H["words"], eng.device)), 1, l, Bg)
    W = _value_expected(oracle, shape, 1, "reference")
    try:
        for units in (6, 70):
            idx = np.arange(units) % len(ACC_KINDS)
            d_ct = ma.to_device(cts6[idx], eng.device)
            for j in range(3):
                for name, key in (("owned", owned), ("view", view)):
                    _assert_words(ma.to_numpy(eng.external_product(key, j, d_ct)), want6[j][idx], "%s key, entry %d, %d units" % (name, j, units))
        for name, key in (("owned", owned), ("view", view)):
            with _settings(key, form):
                for which in range(H["n"]):
                    accs, rows = _value_inputs(H, which)
                    _assert_form(eng, key, form, len(rows))
                    _assert_words(_run_value_rows(eng, key, H, accs, rows, name), W[which], "%s key: value table, key entry %d" % (name, which))
    finally:
        view.free()
