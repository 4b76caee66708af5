"""Row builders for tests/test_pbs_value_edges.py: plain Python integers and numpy, no oracle and no device.  The arithmetic (digits, exact sums, rounding of a mask
word, rotation) is tests/ga_edges_reference.py's; only what the PLAIN blind rotation needs is added here.

The plain blind rotation (src/bootstrap.c:106-122) reads a mask word a_i as abar_i = round(a_i 2N / 2^64) mod 2N, skips the step where abar_i = 0 and otherwise
takes acc <- acc + bk_i (.) ((X^abar_i - 1) acc); the bootstrap rotates the test vector by X^(2N - bbar) first, bbar from the body word plus 2^64 / (4 torus_base)."""
import numpy as np

import ga_edges_reference as R

U64 = np.uint64
MASK64 = R.MASK64
N_MASK = 8
ROW_NAMES = "abcdefghi"


def mask_edge_rows(N, torus_base, seed=0x9B5ED6E, n=N_MASK):
    """[9][n + 1] LWE rows a .. i (the table of the test module's docstring; n even and >= 4); the body words make b + prec_offset round to 0, N, 2N - 1, 2N (wraps),
    0 from just below the first word that rounds to 1, N, 1, N + 1 and a random value"""
    L = R.log2n2(N)
    half = 1 << (63 - L)                                  # the first word that rounds to 1; half - 1 is the last that rounds to 0
    top = 2 * N - 1
    w = lambda v: R.word(v, N)
    masks = [[0] * n,
             [MASK64] * n,
             [half - 1, half] * (n // 2),
             [w(N)] * n,
             [w(1), w(top)] * (n // 2),
             [w(N - 1), w(N + 1)] * (n // 2),
             [w(top) + half] * n,
             [w(3)] + [0] * (n - 2) + [w(top - 2)]]
    rng = np.random.default_rng(seed + N)
    masks.append([int(x) for x in rng.integers(0, 2 ** 64, size=n, dtype=U64)])
    bodies = [0, w(N), w(top), w(top) + half, half - 1, w(N - 1) + half, w(1), w(N + 1), int(rng.integers(0, 2 ** 64, dtype=U64))]
    rows = [m + [(b - R.prec_offset(torus_base)) & MASK64] for m, b in zip(masks, bodies)]
    return np.array(rows, dtype=U64)


def steps(row, N):
    """abar_i of the mask words of one row (the body is the last word); 0 = the step is skipped"""
    return [R.modswitch(x, N) for x in row[:-1]]


def halved(p):
    """[N] uint64 c with -2 c = p mod 2^64 (p even everywhere): (X^N - 1) c = -2 c, so a step of abar = N decomposes p itself"""
    p = np.asarray(p, dtype=U64)
    assert not (p & U64(1)).any()
    return (U64(0) - p) >> U64(1)


# accumulators of the value table: ga_edges_reference.ACC_KINDS as they are, and the two digit extremes halved, so that the step abar = N decomposes exactly them
VALUE_KINDS = R.ACC_KINDS + ("digits_lo halved", "digits_hi halved")


def value_poly(kind, N, l, Bg):
    if kind.endswith(" halved"):
        return halved(R.extreme_poly(kind[:-len(" halved")], N, l, Bg))
    return R.extreme_poly(kind, N, l, Bg)


def value_rows(which, n, N):
    """[2][n + 1]: mask word `which` at 2^63 (abar = N) / at 1 << (64 - log2 2N) (abar = 1), every other word and the body 0"""
    rows = np.zeros((2, n + 1), dtype=U64)
    rows[0, which] = U64(1 << 63)
    rows[1, which] = U64(R.word(1, N))
    return rows


def magnitude_bound_log2(N, l, Bg):
    """log2 of 2^(ceil(log2 2l) + log2 N + Bg - 1 + 63), the magnitude bound of an external product's exact sums at k = 1"""
    return (2 * l - 1).bit_length() + (N.bit_length() - 1) + Bg - 1 + 63
