"""The leveled-LUT kernels (mosfhet_amd/csrc/leveled_lut_kernels.h: lut_prepare_kernel, lut_level0_kernel, lut_cmux_kernel modes 0 and 1, lut_tables_finish_kernel)
at the VALUES that could break them, as tests/test_gpu_parity.py holds the bootstrap kernels (test_rounding_bound_worst_case,
test_unbounded_key_views_take_the_reducing_kernels), and in the run contexts the sibling calls are held to.

  a. every gadget digit at +-2^(Bg-1) against selector rows of +-2^63, stage by stage: the sums reach 2l N 2^(Bg-1) 2^63, which at l = 3, Bg_bit = 10, N = 1024 is
     2^84.6 -- past the 2^83 up to which rounding without the reduction mod 1 is exact (the kernels round with add_rounded<true>; this is what holds them to it)
  b. selectors that are sums a + 2^16 b of fresh selectors, built on the device (dft_lincomb): caller-held DFT content without a magnitude bound
  c. the corner indices: 0, 2^size - 1, the one-hot and the all-but-one indices, all tree bits with no rotation bit and the reverse; size 4 exhaustively
  d. no write past the output, inputs unchanged; a smaller call after a larger one in the same thread's workspace; graph capture; host threads on their own streams

Expected words are the composition of tests/test_leveled_lut.py (_composition; _packed_composition of tests/test_leveled_lut_packed.py for packed tables) on the
oracle's transform of the same selector words -- in b on the device's own doubles copied back.  Every device comparison is == on every word; there is no tolerance
anywhere.  The decryption bound 2^(64 - prec - 1) of c is a condition on the INPUTS, which the oracle composition alone meets on the CPU
(test_corner_indices_composition_decrypts prints the slack); it is no tolerance on the GPU side.
"""
import threading

import numpy as np
import pytest

from test_leveled_lut import _assert_words, _case, _composition, _map, _sel_dft
from test_leveled_lut_packed import _packed_composition
from test_leveled_lut_tables import _tcase

U64 = np.uint64
_CACHE = {}

# a: (N, l, Bg_bit, size).  The first: 4 tables, two tree levels, worst case 2^84.6.  The second: 2 tables, one level, worst case 2^82 -- AT the bound of the
# reduction-free rounding, which it must therefore survive.  The third: 4 tables at N = 2048 with l > 1 (the deeper level's first run there).
EDGE_SHAPES = {"N1024 l3 Bg10": (1024, 3, 10, 12), "N1024 l2 Bg8": (1024, 2, 8, 11), "N2048 l4 Bg9": (2048, 4, 9, 13)}
KINDS = ("min", "max", "alt", "zero")


def _log2(x):
    return float(np.log2(max(float(x), 1.0)))


def _structure(N, size, p):
    """(tree levels, TRLWEs of a table, rotation steps) of a table of 2^size entries of 2^p coefficients"""
    rot = (N.bit_length() - 1) - p
    levels = max(0, size - rot)
    return levels, 1 << levels, min(size, rot)


def _offset(l, Bg):
    """2^(63 - l Bg) + sum_i 2^(63 - i Bg): the rounding offset of the decomposition (leveled_lut_kernels.h: lut_gadget_offset; src/polynomial.c:74-89)"""
    return (1 << (63 - l * Bg)) + sum(1 << (63 - i * Bg) for i in range(l))


def _target(l, Bg, field):
    """the torus word whose l digits all come out of the Bg-bit slot value `field`: 0 -> every digit -2^(Bg-1), 2^Bg - 1 -> every digit 2^(Bg-1) - 1"""
    return (sum(field << (64 - (i + 1) * Bg) for i in range(l)) - _offset(l, Bg)) % 2 ** 64


def _targets(N, l, Bg):
    """the three difference polynomials of the three tables of a: digits all at the bottom, all at the top, alternating by coefficient"""
    lo, hi = _target(l, Bg, 0), _target(l, Bg, (1 << Bg) - 1)
    alt = np.full(N, lo, dtype=U64)
    alt[::2] = U64(hi)
    return [np.full(N, lo, dtype=U64), np.full(N, hi, dtype=U64), alt]


def _rows(kind, l, N):
    """one selector [2l][2][N] of torus words: every word -2^63, every word 2^63 - 1, the two alternating by coefficient, every word 0"""
    g = np.zeros((2 * l, 2, N), dtype=U64)
    if kind in ("min", "alt"):
        g[:] = U64(1 << 63)
    if kind == "max":
        g[:] = U64((1 << 63) - 1)
    if kind == "alt":
        g[..., ::2] = U64((1 << 63) - 1)
    return g


def _stage_tables(N, l, Bg, n_luts, half, seed):
    """three tables [3][n_luts][2][N]: rows 0 .. half-1 trivial (a = 0, b random words), row j + half = row j + target in BOTH components, so that all 2l digit
    rows of the difference sit at the extremes (table 0: bottom, 1: top, 2: alternating); the rows behind 2 half trivial and random"""
    rng = np.random.default_rng(seed)
    tabs = np.zeros((3, n_luts, 2, N), dtype=U64)
    tabs[:, :, 1, :] = rng.integers(0, 2 ** 64, size=(3, n_luts, N), dtype=U64)
    for tb, t in enumerate(_targets(N, l, Bg)):
        for j in range(half):
            tabs[tb, j + half] = tabs[tb, j] + t
    return tabs


def _rotation_preimage(t, m):
    """the polynomial acc with (X^(2N - m) - 1) acc = t, i.e. acc[j + m] - acc[j] = t[j] for j < N - m and -acc[j + m - N] - acc[j] = t[j] behind it: per residue r mod m
    a chain of partial sums from acc[r], and the wrap gives 2 acc[r] = -(the sum of t over the residue class), which is even for the targets used here"""
    N = len(t)
    acc = [0] * N
    for r in range(m):
        total = sum(int(t[j]) for j in range(r, N, m)) % 2 ** 64
        assert total % 2 == 0
        x = ((-total) % 2 ** 64) // 2
        for j in range(r, N, m):
            acc[j] = x
            x = (x + int(t[j])) % 2 ** 64
    return np.array(acc, dtype=U64)


def _extract(c, e):
    """SampleExtract at coefficient e of the TRLWE sample c [2][N], written out (src/trlwe.c:540-552): a[j] = c.a[e - j] for j <= e, -c.a[N + e - j] behind it; b = c.b[e]
    -- what a call gives when every selector is zero; (0, ..., 0, c.b[e]) for a trivial c"""
    N = c.shape[1]
    j = np.arange(N)
    with np.errstate(over="ignore"):
        a = np.where(j <= e, c[0][(e - j) % N], U64(0) - c[0][(e - j) % N])
    return np.concatenate([a, c[1][e:e + 1]]).astype(U64)


def _assert_extracted(out, tabs, p, what):
    """out [tables][2^p][N + 1] is the extraction of table[0] of every table at e < 2^p"""
    for tb in range(len(tabs)):
        for e in range(1 << p):
            assert (out[tb, e] == _extract(tabs[tb, 0], e)).all(), (what, tb, e)


def _expect(oracle, tabs, sel_dft, N, l, Bg, size, p):
    """[2^p][N + 1]: the composition of the sibling files on one table"""
    if p == 0:
        return _composition(oracle, tabs, sel_dft, N, l, Bg, size)[None]
    return _packed_composition(oracle, tabs, sel_dft, N, l, Bg, size, p)


def _want(oracle, tabs, sel_dft, N, l, Bg, size, p):
    """want[b][tb][t][N + 1] over all inputs (sel_dft: a list of [size][2l][2][N] doubles in the oracle's order) and all tables"""
    tables = len(tabs)
    out = _map(lambda u: _expect(oracle, tabs[u % tables], sel_dft[u // tables], N, l, Bg, size, p), range(len(sel_dft) * tables))
    return np.stack(out).reshape(len(sel_dft), tables, 1 << p, N + 1)


def _edge_case(oracle, shape, p):
    """The stages of a for one shape and one pack_log: a list of dict(name, tabs [3][n_luts][2][N], sel [count][size][2l][2][N] torus words, want, zero = the input
    whose selectors are all zero, level = the tree level the stage aims at or None for the finish, diff [3][nodes][2][N] = the polynomials the stage's step decomposes
    (None where they are whatever the tree left), mag = the largest |double| of the transformed selectors).
      tree level i   table[j + half_i] - table[j] = target for j < half_i; selectors size-1 .. size-i all zero (those levels leave their left operands as they are, so
                     level i decomposes exactly the target); selector size-1-i all -2^63 / all 2^63 - 1 / alternating / all zero; every other selector zero
      finish, step 0 table[0] = the polynomial whose first rotation difference (X^(2N - 2^p) - 1) table[0] is the target, in both components, every tree selector zero, so
                     that the finish's first step decomposes exactly the target; selector 0 as above, every other selector zero
      finish         selectors 0 .. steps-1 at the extremes on whatever the tree left: the tree selectors zero (three inputs), every selector of the input cycling
                     through the extremes, every selector -2^63, every selector zero"""
    key = ("edge", shape, p)
    if key in _CACHE:
        return _CACHE[key]
    N, l, Bg, size = EDGE_SHAPES[shape]
    oracle.plan(N)       # by one thread, in front of the workers of _map
    levels, n_luts, steps = _structure(N, size, p)
    stages = []
    for i in range(levels):
        sel = np.zeros((len(KINDS), size, 2 * l, 2, N), dtype=U64)
        for k, kind in enumerate(KINDS):
            sel[k, size - 1 - i] = _rows(kind, l, N)
        tabs, half = _stage_tables(N, l, Bg, n_luts, n_luts >> (i + 1), 0xED6E + i), n_luts >> (i + 1)
        stages.append(dict(name="tree level %d" % i, level=i, zero=KINDS.index("zero"), sel=sel, tabs=tabs, diff=tabs[:, half:2 * half] - tabs[:, :half]))
    # the finish's first step: (X^(2N - 2^p) - 1) table[0] = target in both components
    sel = np.zeros((len(KINDS), size, 2 * l, 2, N), dtype=U64)
    for k, kind in enumerate(KINDS):
        sel[k, 0] = _rows(kind, l, N)
    tabs = _stage_tables(N, l, Bg, n_luts, 0, 0x57E9)
    for tb, t in enumerate(_targets(N, l, Bg)):
        tabs[tb, 0] = _rotation_preimage(t, 1 << p)
    diff = np.stack([np.stack([oracle.poly_mul_by_xai_minus_1(np.ascontiguousarray(tabs[tb, 0, q]), 2 * N - (1 << p)) for q in range(2)]) for tb in range(3)])[:, None]
    stages.append(dict(name="finish, step 0", level=None, zero=KINDS.index("zero"), sel=sel, tabs=tabs, diff=diff))
    sel = np.zeros((6, size, 2 * l, 2, N), dtype=U64)
    for k, kind in enumerate(KINDS[:3]):
        sel[k, :steps] = _rows(kind, l, N)
    for i in range(size):
        sel[3, i] = _rows(KINDS[i % 3], l, N)
    sel[4, :] = _rows("min", l, N)
    stages.append(dict(name="finish", level=None, zero=5, sel=sel, tabs=_stage_tables(N, l, Bg, n_luts, n_luts >> 1, 0xF121), diff=None))
    for S in stages:
        dft = _map(lambda b: oracle.bk_to_dft(S["sel"][b], 1, l), range(len(S["sel"])))
        S["mag"] = max(float(np.abs(d).max()) for d in dft)
        S["want"] = _want(oracle, S["tabs"], dft, N, l, Bg, size, p)
    _CACHE[key] = stages
    return stages


def _fresh_selectors(oracle, r, s, m, size, l, Bg, sigma):
    """[len(m)][size][2l][2][N]: selector i of input b encrypts bit i of m[b], as tests/test_leveled_lut.py::_case makes them"""
    return np.stack([np.stack([oracle.trgsw_monomial_sample(r, (x >> i) & 1, 0, s, l, Bg, sigma) for i in range(size)]) for x in m])


def _trivial_tables(seed, N, n_luts, tables, prec):
    """(lut [tables][n_luts N] of values below 2^prec, tabs [tables][n_luts][2][N] trivial samples of them at the top of the word)"""
    rng = np.random.default_rng(seed)
    lut = rng.integers(0, 1 << prec, size=(tables, n_luts * N), dtype=U64)
    tabs = np.zeros((tables, n_luts, 2, N), dtype=U64)
    tabs[:, :, 1, :] = (lut << U64(64 - prec)).reshape(tables, n_luts, N)
    return lut, tabs


# c: name: (N, l, Bg_bit, sigma, size, prec) -- the gadgets, noises and precisions of sets E, F, A and C of tests/test_leveled_lut.py
CORNER_SETS = {"size 4": (1024, 3, 10, 2.0 ** -44, 4, 3), "size 10": (1024, 3, 10, 2.0 ** -44, 10, 6), "size 13": (1024, 3, 10, 2.0 ** -44, 13, 6),
               "N2048 size 12": (2048, 4, 9, 2.0 ** -44, 12, 4)}
CORNER_PACKS = (0, 1, 3)


def _corner_indices(N, size, p):
    """0, 2^size - 1, 1, 2^(size-1), 2^size - 2; with a tree (at this pack_log), the index whose tree bits are all one and whose rotation bits are all zero, and its
    complement.  Size 4 exhaustively."""
    if size == 4:
        return list(range(16))
    full = (1 << size) - 1
    m = [0, full, 1, 1 << (size - 1), full - 1]
    levels, _, steps = _structure(N, size, p)
    if levels:
        m += [full ^ ((1 << steps) - 1), (1 << steps) - 1]
    return m


def _corner_case(oracle, name):
    """dict(s, per pack_log p: m (the indices), sel, lut, tabs (one table), want [len(m)][1][2^p][N + 1]) -- one selector set per index, shared by the pack_logs"""
    key = ("corner", name)
    if key in _CACHE:
        return _CACHE[key]
    N, l, Bg, sigma, size, prec = CORNER_SETS[name]
    oracle.plan(N)
    r = oracle.Rng(0xC0E + size + N)
    s = oracle.gen_binary_key(r, N).reshape(1, N)
    union = sorted({x for p in CORNER_PACKS for x in _corner_indices(N, size, p)})
    sel = _fresh_selectors(oracle, r, s, union, size, l, Bg, sigma)
    dft = dict(zip(union, _map(lambda b: oracle.bk_to_dft(sel[b], 1, l), range(len(union)))))
    S = dict(N=N, l=l, Bg=Bg, size=size, prec=prec, s=s)
    for p in CORNER_PACKS:
        m = _corner_indices(N, size, p)
        assert len(m) <= 8 or size == 4
        lut, tabs = _trivial_tables(0xC0E + p, N, _structure(N, size, p)[1], 1, prec)
        S[p] = dict(m=m, sel=np.stack([sel[union.index(x)] for x in m]), lut=lut, tabs=tabs, want=_want(oracle, tabs, [dft[x] for x in m], N, l, Bg, size, p))
    _CACHE[key] = S
    return S


def _worst_corner_distance(oracle, S, p, outs):
    """largest torus distance of an output's phase from LUT[2^p m + t] over all (input, t) of the corner case at pack_log p"""
    worst, mm = 0.0, 1 << p
    for b, x in enumerate(S[p]["m"]):
        for t in range(mm):
            want = int(S[p]["lut"][0][mm * x + t]) << (64 - S["prec"])
            worst = max(worst, float(oracle.torus_dist(oracle.tlwe_phase(outs[b, 0, t], S["s"][0]), want)))
    return worst


# d: the run contexts, at N = 1024, l = 3, Bg_bit = 10
def _context_case(oracle, size, inputs, seed):
    """fresh selectors of `inputs` random indices, three trivial tables for pack_log 0 and for pack_log 1, and the composition's words for both"""
    key = ("context", size, inputs, seed)
    if key in _CACHE:
        return _CACHE[key]
    N, l, Bg, sigma = 1024, 3, 10, 2.0 ** -44
    oracle.plan(N)
    r = oracle.Rng(seed)
    s = oracle.gen_binary_key(r, N).reshape(1, N)
    rng = np.random.default_rng(seed)
    m = [int(rng.integers(0, 1 << size)) for _ in range(inputs)]
    sel = _fresh_selectors(oracle, r, s, m, size, l, Bg, sigma)
    dft = _map(lambda b: oracle.bk_to_dft(sel[b], 1, l), range(inputs))
    S = dict(N=N, l=l, Bg=Bg, size=size, sel=sel)
    for p in (0, 1):
        _, tabs = _trivial_tables(seed + p, N, _structure(N, size, p)[1], 3, 6)
        S[p] = dict(tabs=tabs, want=_want(oracle, tabs, dft, N, l, Bg, size, p))
    _CACHE[key] = S
    return S


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
@pytest.mark.parametrize("shape", list(EDGE_SHAPES))
def test_digit_constructions(oracle, shape):
    """oracle.poly_decompose_i on the constructions of a: target(0) gives every one of the l digits -2^(Bg-1), target(2^Bg - 1) gives 2^(Bg-1) - 1; in the tables of
    every stage both components of what the stage's step decomposes -- table[j + half] - table[j] of a tree level, (X^(2N - 2^p) - 1) table[0] of the finish's first
    step (oracle.poly_mul_by_xai_minus_1) -- decompose so (table 2: alternating by coefficient): all 2l digit rows.  Prints the largest magnitude
    of the transformed extreme selectors and the bound 2l N 2^(Bg-1) 2^63 the sums reach with them."""
    N, l, Bg, size = EDGE_SHAPES[shape]
    bottom, top = -(1 << (Bg - 1)), (1 << (Bg - 1)) - 1
    lo, hi, alt = _targets(N, l, Bg)
    for i in range(l):
        assert (oracle.poly_decompose_i(lo.copy(), Bg, l, i).view(np.int64) == bottom).all(), (shape, i)
        assert (oracle.poly_decompose_i(hi.copy(), Bg, l, i).view(np.int64) == top).all(), (shape, i)
    for p in (0, 1):
        for S in _edge_case(oracle, shape, p):
            print("%s, pack_log %d, %s: largest |selector double| 2^%.1f" % (shape, p, S["name"], _log2(S["mag"])))
            if S["diff"] is None:
                continue
            for tb in range(3):
                for j in range(S["diff"].shape[1]):
                    for q in range(2):
                        for i in range(l):
                            got = oracle.poly_decompose_i(np.ascontiguousarray(S["diff"][tb, j, q]), Bg, l, i).view(np.int64)
                            if tb == 2:
                                assert (got[::2] == top).all() and (got[1::2] == bottom).all(), (shape, p, S["name"], j, q, i)
                            else:
                                assert (got == (bottom if tb == 0 else top)).all(), (shape, p, S["name"], tb, j, q, i)
    print("%s: the sums reach 2l N 2^(Bg-1) 2^63 = 2^%.1f" % (shape, np.log2(2 * l * N) + Bg - 1 + 63))


@pytest.mark.parametrize("shape", list(EDGE_SHAPES))
def test_zero_selector_identity_in_the_oracle(oracle, shape):
    """What the stage construction of a rests on, in the oracle: the external product with a selector of all-zero words is zero on every word, whatever the sample,
    so a tree level with it leaves its left operands unchanged bit for bit; and the composition with every selector zero is the extraction of table[0]
    at e < 2^pack_log, written out in _extract: (0, ..., 0, table[0].b[e]) where table[0] is trivial."""
    N, l, Bg, size = EDGE_SHAPES[shape]
    zero = oracle.bk_to_dft(np.zeros((1, 2 * l, 2, N), dtype=U64), 1, l)[0]
    assert (zero == 0).all()
    rng = np.random.default_rng(5)
    for x in (rng.integers(0, 2 ** 64, size=(2, N), dtype=U64), np.stack([_targets(N, l, Bg)[0]] * 2), np.full((2, N), 2 ** 64 - 1, dtype=U64)):
        assert (oracle.external_product(x, zero, l, Bg) == 0).all()
    for p in (0, 1):
        for S in _edge_case(oracle, shape, p):
            _assert_extracted(S["want"][S["zero"]], S["tabs"], p, (shape, p, S["name"]))
            if S["level"] is not None:
                z = S["want"][S["zero"]]
                assert (z[:, :, :N] == 0).all() and all((z[:, e, N] == S["tabs"][:, 0, 1, e]).all() for e in range(1 << p))      # trivial table[0]: (0, ..., 0, b[e])


@pytest.mark.parametrize("name", list(CORNER_SETS))
def test_corner_indices_composition_decrypts(oracle, name):
    """The condition on the inputs of c, proven on the CPU: the oracle composition alone decrypts every corner index to LUT[2^p m + t] within 2^(64 - prec - 1), at
    pack_log 0, 1 and 3.  The slack is printed."""
    S = _corner_case(oracle, name)
    bound = 64 - S["prec"] - 1
    for p in CORNER_PACKS:
        worst = _worst_corner_distance(oracle, S, p, S[p]["want"])
        print("%s, pack_log %d, indices %s: worst log2 torus_dist(phase, LUT) = %.1f, bound %d, slack %.1f bits" % (name, p, S[p]["m"], _log2(worst), bound, bound - _log2(worst)))
        assert worst < 2.0 ** bound, (name, p, _log2(worst))


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


ENTRIES = {"one table": ("one", 0, 0), "3 tables, default group": ("tables", 0, 0), "3 tables, largest group": ("tables", 0, 64), "packed, pack_log 1": ("packed", 1, 0)}


def _call(eng, entry, sel, d_tabs, size, l, Bg, p, out=None):
    """one of the three entry points on device selectors [count][size][2l][2][N] and device tables [tables][n_luts][2][N] -> the device tensor(s) it wrote"""
    if entry == "one":
        return eng.leveled_lut(sel, d_tabs[0], size, l, Bg, out=out)
    if entry == "tables":
        return eng.leveled_lut_tables(sel, d_tabs, size, l, Bg, out=out)
    return eng.leveled_lut_packed(sel, d_tabs, size, l, Bg, p, out=out)


def _words(eng, entry, sel, d_tabs, size, l, Bg, p):
    """the words of an entry point as [count][tables][2^p][N + 1]; the one-table call runs once per table"""
    import mosfhet_amd as ma
    if entry == "one":
        return np.stack([ma.to_numpy(eng.leveled_lut(sel, d_tabs[tb], size, l, Bg)) for tb in range(d_tabs.shape[0])], axis=1)[:, :, None]
    got = ma.to_numpy(_call(eng, entry, sel, d_tabs, size, l, Bg, p))
    return got[:, :, None] if entry == "tables" else got


def _assert_all(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    _assert_words(got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1]), what)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("shape", list(EDGE_SHAPES))
def test_digit_extremes_against_extreme_selector_rows(eng, oracle, shape, entry):
    """a.  Per stage (every tree level, the finish's first step, then the whole finish) one call on the stage's three tables (digits all -2^(Bg-1), all 2^(Bg-1) - 1, alternating) and its inputs
    (selector rows all -2^63, all 2^63 - 1, alternating, zero): every word equals the composition on oracle.bk_to_dft of the same selector words.  Without an
    oracle: the all-zero input gives the extraction of table[0] written out in _extract -- (0, ..., 0, table[0].b[e]) where table[0] is trivial -- exactly.  In front of a deeper level the identity it rests on, on the device: a ONE-level call on
    the stage's first two rows with zero selectors returns table[0] extracted, exactly."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    which, p, group = ENTRIES[entry]
    N, l, Bg, size = EDGE_SHAPES[shape]
    rot = (N.bit_length() - 1) - p
    try:
        engine.set_leveled_lut_tables_group(group)
        for S in _edge_case(oracle, shape, p):
            d_tabs = ma.to_device(S["tabs"], eng.device)
            if S["level"]:
                first = d_tabs[:, :2].contiguous()
                none = _sel_dft(eng, np.zeros((1, rot + 1, 2 * l, 2, N), dtype=U64))
                one_level = _words(eng, which, none, first, rot + 1, l, Bg, p)
                _assert_extracted(one_level[0], S["tabs"], p, (shape, entry, S["name"], "one level, zero selectors"))
                assert (one_level[0, :, :, :N] == 0).all()
            got = _words(eng, which, _sel_dft(eng, S["sel"]), d_tabs, size, l, Bg, p)
            print("%s, %s, %s: largest |selector double| 2^%.1f" % (shape, entry, S["name"], _log2(S["mag"])))
            _assert_all(got, S["want"], "%s, %s, %s" % (shape, entry, S["name"]))
            _assert_extracted(got[S["zero"]], S["tabs"], p, (shape, entry, S["name"], "all selectors zero"))
            assert (ma.to_numpy(d_tabs) == S["tabs"]).all(), "the tables were modified"
    finally:
        engine.set_leveled_lut_tables_group(0)


# b: (N, l, Bg_bit, sigma, size)
UNBOUNDED_SHAPES = {"size 4": (1024, 3, 10, 2.0 ** -44, 4), "size 10": (1024, 3, 10, 2.0 ** -44, 10), "size 12": (1024, 3, 10, 2.0 ** -44, 12),
                    "N2048 l1 Bg23 size 12": (2048, 1, 23, 2.0 ** -52, 12)}


@pytest.mark.gpu
@pytest.mark.parametrize("content", ["a + 2^16 b", "a + b"])
@pytest.mark.parametrize("shape", list(UNBOUNDED_SHAPES))
def test_unbounded_selectors(eng, oracle, shape, content):
    """b.  Two fresh selector sets a, b of the same two indices, summed on the device (dft_lincomb) to a + 2^16 b -- beyond 2^78 in the DFT domain, which no
    transform of torus words reaches (below 2^73) -- and, as the control, to a plain a + b, which stays below 2^78.  The one-table call, three tables and packed tables
    (pack_log 1) equal the composition on the device's own doubles copied back (engine.slot_order_to_oracle), word for word.  Nothing is decrypted: the sums encrypt
    nothing meaningful."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, l, Bg, sigma, size = UNBOUNDED_SHAPES[shape]
    oracle.plan(N)
    key = ("unbounded", shape)
    if key not in _CACHE:
        r = oracle.Rng(0xB16 + size + N)
        s = oracle.gen_binary_key(r, N).reshape(1, N)
        m = [int(x) for x in np.random.default_rng(size + N).integers(0, 1 << size, size=2)]
        _CACHE[key] = [_fresh_selectors(oracle, r, s, m, size, l, Bg, sigma) for _ in range(2)]
    a, b = [_sel_dft(eng, x) for x in _CACHE[key]]
    big = content == "a + 2^16 b"
    sel = eng.dft_lincomb(a, b, 2.0 ** 16 if big else 1.0)
    host = engine.slot_order_to_oracle(sel.cpu().numpy().reshape(-1, N), N).reshape(2, size, 2 * l, 2, N)
    mag = float(np.abs(host).max())
    print("%s, %s: largest |selector double| 2^%.1f" % (shape, content, _log2(mag)))
    assert np.isfinite(host).all()
    assert (mag > 2.0 ** 78) == big, (shape, content, _log2(mag))
    dft = [np.ascontiguousarray(host[i]) for i in range(2)]
    for which, p in (("one", 0), ("tables", 0), ("packed", 1)):
        _, tabs = _trivial_tables(0xB16 + p, N, _structure(N, size, p)[1], 3, 4)
        want = _want(oracle, tabs, dft, N, l, Bg, size, p)
        got = _words(eng, which, sel, ma.to_device(tabs, eng.device), size, l, Bg, p)
        _assert_all(got, want, "%s, %s, %s" % (shape, content, which))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CORNER_SETS))
def test_corner_indices(eng, oracle, name):
    """c.  Fresh selectors of the indices 0, 2^size - 1, 1, 2^(size-1), 2^size - 2 and, with a tree, of the index with all tree bits and no rotation bit and of its
    complement (size 4: all 16 indices), through the one-table call and through packed tables at pack_log 1 and 3: every word equals the composition, and every
    output decrypts to LUT[2^p m + t] (test_corner_indices_composition_decrypts: the composition alone meets that bound)."""
    import mosfhet_amd as ma
    S = _corner_case(oracle, name)
    N, l, Bg, size = S["N"], S["l"], S["Bg"], S["size"]
    for which, p in (("one", 0), ("packed", 1), ("packed", 3)):
        C = S[p]
        got = _words(eng, which, _sel_dft(eng, C["sel"]), ma.to_device(C["tabs"], eng.device), size, l, Bg, p)
        _assert_all(got, C["want"], "%s, %s, pack_log %d, indices %s" % (name, which, p, C["m"]))
        worst = _worst_corner_distance(oracle, S, p, got)
        assert worst < 2.0 ** (64 - S["prec"] - 1), (name, which, p, _log2(worst))


SENTINEL = 0x5EA75EA75EA75EA7


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["one", "tables", "packed"])
def test_a_call_stays_inside_its_output_and_leaves_its_inputs(eng, oracle, entry):
    """d.  Size 12 (two tree levels; three with pack_log 1), 2 inputs: the output buffer is one row (one input's share) longer than needed and sentinel-filled; the
    tail keeps the sentinel, the rows in front equal the composition, and the selectors and tables on the device are unchanged afterwards."""
    import torch
    import mosfhet_amd as ma
    p = 1 if entry == "packed" else 0
    S = _context_case(oracle, 12, 2, 0xD1)
    N, l, Bg, size = S["N"], S["l"], S["Bg"], S["size"]
    tabs, want = (S[p]["tabs"][:1], S[p]["want"][:, :1]) if entry == "one" else (S[p]["tabs"], S[p]["want"])
    share = {"one": (N + 1,), "tables": (3, N + 1), "packed": (3, 2, N + 1)}[entry]
    sel, d_tabs = _sel_dft(eng, S["sel"]), ma.to_device(tabs, eng.device)
    sel0, tabs0 = sel.clone(), d_tabs.clone()
    buf = torch.full((3,) + share, SENTINEL, dtype=torch.int64, device=eng.device)
    _call(eng, entry, sel, d_tabs, size, l, Bg, p, out=buf[:2])
    torch.cuda.synchronize(eng.device)
    got = ma.to_numpy(buf)
    assert (got[2] == U64(SENTINEL)).all(), "%s wrote past its last input" % entry
    _assert_all(got[:2].reshape(want.shape), want, entry)
    assert torch.equal(sel, sel0), "%s changed its selectors" % entry
    assert torch.equal(d_tabs, tabs0), "%s changed its tables" % entry


@pytest.mark.gpu
@pytest.mark.parametrize("tables", [1, 3])
def test_a_smaller_call_after_a_larger_one(eng, oracle, tables):
    """d.  In one thread -- one workspace, the calling thread's pool slot -- set G of tests/test_leveled_lut.py (size 16, 32 first-level nodes, 5 inputs), then size 12
    with 2 inputs, then size 11 with 7 inputs: each equals its composition, which prepared rows or intermediates left over from the larger call would spoil."""
    import mosfhet_amd as ma
    G = _case(oracle, "G") if tables == 1 else _tcase(oracle, "G", tables=3)
    runs = [(G["sel"], G["tabs"][None] if tables == 1 else G["tabs"], G["want"].reshape(5, tables, 1, -1), 16)]
    for size, inputs in ((12, 2), (11, 7)):
        S = _context_case(oracle, size, inputs, 0xD1 if size == 12 else 0xD2)
        runs.append((S["sel"], S[0]["tabs"][:tables], S[0]["want"][:, :tables], size))
    for sel, tabs, want, size in runs:
        got = _words(eng, "one" if tables == 1 else "tables", _sel_dft(eng, sel), ma.to_device(tabs, eng.device), size, 3, 10, 0)
        _assert_all(got, want, "size %d, %d inputs, %d tables, behind the calls in front of it" % (size, len(sel), tables))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["one", "tables", "packed"])
def test_lut_calls_are_captured_in_a_graph(eng, oracle, entry):
    """d.  Each call at size 12, captured on one side stream after an eager call of that shape, replayed twice on different selectors copied into the captured
    buffer: each replay == the eager words (which equal the composition) -- no hidden allocation, synchronisation or state left between replays.  One stream, no
    parallel branches."""
    import torch
    import mosfhet_amd as ma
    p = 1 if entry == "packed" else 0
    S = _context_case(oracle, 12, 4, 0xD3)
    N, l, Bg, size = S["N"], S["l"], S["Bg"], S["size"]
    tabs, want = (S[p]["tabs"][:1], S[p]["want"][:, :1]) if entry == "one" else (S[p]["tabs"], S[p]["want"])
    d_tabs = ma.to_device(tabs, eng.device)
    all_sel = _sel_dft(eng, S["sel"])
    xs = [all_sel[:2].contiguous(), all_sel[2:].contiguous()]
    eager = [ma.to_numpy(_call(eng, entry, x, d_tabs, size, l, Bg, p)) for x in xs]
    for r in range(2):
        _assert_all(eager[r].reshape(want[2 * r:2 * r + 2].shape), want[2 * r:2 * r + 2], "%s, eager, inputs %d" % (entry, r))
    d_sel, d_out = xs[0].clone(), torch.empty(eager[0].shape, dtype=torch.int64, device=eng.device)
    side = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _call(eng, entry, d_sel, d_tabs, size, l, Bg, p, out=d_out)
    for r in (1, 0):
        d_sel.copy_(xs[r])
        d_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert (ma.to_numpy(d_out) == eager[r]).all(), "%s: replay on inputs %d differs from the plain call" % (entry, r)
    del g


@pytest.mark.gpu
def test_host_threads_run_lut_calls_on_their_own_streams(eng, oracle):
    """d.  Three host threads, each on a stream of its own, each five times its own shape -- size 12 through the one-table call, size 13 with three tables, size 16
    (set G) through the one-table call: every result equals the single-threaded words, which equal the composition.  The workspace of a call belongs to the calling
    thread's pool; a workspace shared between threads would mix the three shapes' intermediates."""
    import torch
    import mosfhet_amd as ma
    S12, S13, G = _context_case(oracle, 12, 2, 0xD1), _context_case(oracle, 13, 2, 0xD4), _case(oracle, "G")
    jobs = [("one", S12["sel"], S12[0]["tabs"][:1], 12, S12[0]["want"][:, :1]), ("tables", S13["sel"], S13[0]["tabs"], 13, S13[0]["want"]),
            ("one", G["sel"], G["tabs"][None], 16, G["want"].reshape(5, 1, 1, -1))]
    dev = [(_sel_dft(eng, sel), ma.to_device(tabs, eng.device)) for _, sel, tabs, _, _ in jobs]
    single = [_words(eng, jobs[t][0], dev[t][0], dev[t][1], jobs[t][3], 3, 10, 0) for t in range(3)]
    for t in range(3):
        _assert_all(single[t], jobs[t][4], "single-threaded, size %d" % jobs[t][3])
    torch.cuda.synchronize()
    bad, errors = [0, 0, 0], []

    def worker(t):
        try:
            stream = torch.cuda.Stream(device=eng.device)
            with torch.cuda.stream(stream):
                for _ in range(5):
                    got = _words(eng, jobs[t][0], dev[t][0], dev[t][1], jobs[t][3], 3, 10, 0)
                    bad[t] += int(not (got == single[t]).all())
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(3)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert bad == [0, 0, 0], bad
