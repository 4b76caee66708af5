"""Row builders and exact integer arithmetic for tests/test_ga_edges.py: plain Python integers and numpy, no oracle and no device.

The Galois-automorphism blind rotation (src/bootstrap_ga.c:39-60) reads a mask word a_i as abar_i = round(a_i 2N / 2^64) mod 2N, forces it odd (abar_i | 1) and
walks the generators  inverse(abar_0 | 1),  (abar_i | 1) inverse(abar_{i+1} | 1) for i < n - 1,  abar_{n-1} | 1  (all mod 2N); the automorphism of generator g
switches with key-set entry (g - 1) / 2."""
import numpy as np

U64 = np.uint64
MASK64 = (1 << 64) - 1
N_MASK = 8                    # mask words of an edge row
ROW_NAMES = "abcdefghi"


def log2n2(N):
    return (2 * N).bit_length() - 1


def word(v, N):
    """the torus word that rounds to v exactly: v << (64 - L), L = log2(2N)"""
    return (v << (64 - log2n2(N))) & MASK64


def modswitch(x, N):
    """round(x 2N / 2^64) mod 2N of a torus word (src/misc.c: torus2int)"""
    L = log2n2(N)
    return ((int(x) + (1 << (63 - L))) >> (64 - L)) & (2 * N - 1)


def prec_offset(torus_base):
    """2^64 / (4 torus_base): what functional_bootstrap adds to the body word in front of the rounding (src/bootstrap_ga.c:64)"""
    return (1 << 64) // (4 * torus_base)


def edge_rows(N, torus_base, seed=0x6AED6E, n=N_MASK):
    """[9][n + 1] LWE rows a .. i (the table of this file's test module; n even, the patterns repeat beyond 8 mask words); the body words make b + prec_offset round
    to 0, N, 2N - 1, 2N (wraps), 0 from just below the first word that rounds to 1, N from the first word that rounds to it, 1, N + 1 and a random value"""
    L = log2n2(N)
    half = 1 << (63 - L)                                  # the first word that rounds to 1; half - 1 is the last that rounds to 0
    top = 2 * N - 1
    even = (2, 4, N, 2 * N - 2, N - 2, N + 2, 6, 8)
    masks = [[0] * n,
             [MASK64] * n,
             [half - 1, half] * (n // 2),
             [word(top, N) + half] * n,
             [word(top, N)] * n,
             [word(1, N), word(top, N)] * (n // 2),
             [word(even[i % 8], N) for i in range(n)],
             [word(N - 1, N), word(N + 1, N)] * (n // 2)]
    rng = np.random.default_rng(seed + N)
    masks.append([int(x) for x in rng.integers(0, 2 ** 64, size=n, dtype=U64)])
    bodies = [0, word(N, N), word(top, N), word(top, N) + half, half - 1, word(N - 1, N) + half, word(1, N), word(N + 1, N), int(rng.integers(0, 2 ** 64, dtype=U64))]
    rows = [m + [(b - prec_offset(torus_base)) & MASK64] for m, b in zip(masks, bodies)]
    return np.array(rows, dtype=U64)


def shorten(cts, n):
    """the rows for a key of n mask words: the first n mask words and the body"""
    return np.ascontiguousarray(np.concatenate([cts[:, :n], cts[:, -1:]], axis=1))


def exponents(row, N):
    """abar_i | 1 of the mask words of one row (the body is the last word)"""
    return [modswitch(x, N) | 1 for x in row[:-1]]


def generators(row, N):
    """the n + 1 generators a row walks, in order"""
    a = exponents(row, N)
    return [pow(a[0], -1, 2 * N)] + [(a[i] * pow(a[i + 1], -1, 2 * N)) % (2 * N) for i in range(len(a) - 1)] + [a[-1]]


def entries_used(cts, N):
    """the set of key-set entries (g - 1) / 2 a batch uses"""
    return {(g - 1) // 2 for row in cts for g in generators(row, N)}


def body_exponent(row, N, torus_base):
    """bbar: what the first rotation uses"""
    return modswitch((int(row[-1]) + prec_offset(torus_base)) & MASK64, N)


def rotate(m, e, N):
    """X^e m(X) mod X^N + 1 on a list of Python integers mod 2^64, e in [0, 2N)"""
    out = [0] * N
    for j in range(N):
        k = j + e
        out[k % N] = m[j] if (k // N) % 2 == 0 else (-m[j]) & MASK64
    return out


def permute(m, gen, N):
    """m(X^gen) mod X^N + 1 (src/polynomial.c:442-450): out[(i gen) mod N] = +-in[i]"""
    out = [0] * N
    for i in range(N):
        k = i * gen
        out[k % N] = m[i] if (k // N) % 2 == 0 else (-m[i]) & MASK64
    return out


def gadget_offset(l, Bg):
    """2^(63 - l Bg) + sum_i 2^(63 - i Bg): the rounding offset of the decomposition (src/polynomial.c:74-89)"""
    return (1 << (63 - l * Bg)) + sum(1 << (63 - i * Bg) for i in range(l))


def digit_target(l, Bg, field):
    """the torus word whose l digits all come out of the Bg-bit slot value `field`: 0 -> every digit -2^(Bg-1), 2^Bg - 1 -> every digit 2^(Bg-1) - 1"""
    return (sum(field << (64 - (i + 1) * Bg) for i in range(l)) - gadget_offset(l, Bg)) % 2 ** 64


def digits(p, l, Bg):
    """[l][N] int64: the signed digits of the polynomial p (uint64 [N]) as the kernels and src/polynomial.c:74-89 take them"""
    w = np.asarray(p, dtype=U64) + U64(gadget_offset(l, Bg))
    return np.stack([((w >> U64(64 - (i + 1) * Bg)) & U64((1 << Bg) - 1)).astype(np.int64) - (1 << (Bg - 1)) for i in range(l)])


ACC_KINDS = ("min", "max", "alt", "zero", "digits_lo", "digits_hi")
KEY_KINDS = ("min", "max", "alt")


def extreme_poly(kind, N, l, Bg):
    """[N] uint64: every word 2^63, every word 2^63 - 1, the two alternating by coefficient, zero, every digit -2^(Bg-1), every digit 2^(Bg-1) - 1"""
    p = np.zeros(N, dtype=U64)
    if kind in ("min", "alt"):
        p[:] = U64(1 << 63)
    if kind == "max":
        p[:] = U64((1 << 63) - 1)
    if kind == "alt":
        p[::2] = U64((1 << 63) - 1)
    if kind == "digits_lo":
        p[:] = U64(digit_target(l, Bg, 0))
    if kind == "digits_hi":
        p[:] = U64(digit_target(l, Bg, (1 << Bg) - 1))
    return p


def exact_sums(d, key):
    """The exact integers sum_r d[r] (*) key[r] of a product (negacyclic convolutions mod X^N + 1, the key words read as signed 64-bit integers, nothing reduced):
    d [rows][N] int64 digits, key [rows][N] uint64 -> a list of N Python integers.  The key words are cut into 22-bit limbs so that every partial convolution stays
    inside int64 (rows N 2^(Bg-1) 2^22 < 2^63 for every gadget here)."""
    rows, N = d.shape
    k = np.asarray(key, dtype=U64).view(np.int64)
    limbs = [(k >> np.int64(22 * j)) & np.int64((1 << 22) - 1) for j in range(2)] + [k >> np.int64(44)]      # the top limb keeps the sign
    acc = [np.zeros(N, dtype=np.int64) for _ in limbs]
    for r in range(rows):
        for j, limb in enumerate(limbs):
            full = np.convolve(d[r], limb[r])
            acc[j] += full[:N]
            acc[j][:N - 1] -= full[N:]
    return [int(acc[0][i]) + (int(acc[1][i]) << 22) + (int(acc[2][i]) << 44) for i in range(N)]


def largest_sum_log2(d, key):
    import math
    return math.log2(max(1, max(abs(x) for x in exact_sums(d, key))))
