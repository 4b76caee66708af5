"""Plain reference of the library's key-generation randomness, written from its specification (tests/test_keygen_known_answers.py).

  * chacha20_block: the ChaCha20 block function of RFC 8439 section 2.3 in the original parameterisation (64-bit block counter in state words 12 - 13,
    64-bit nonce in words 14 - 15);
  * mask_word: the public mask generator of the device key generators (csrc/keygen_kernels.h, keygen_mix: a splitmix64 finaliser over (seed, row, word,
    stream)) -- a FILE FORMAT: stored seed-compressed keys regenerate their masks with it;
  * noise_term: the secret Gaussian noise term of coefficient x of row `row` of one generate call: ChaCha20 under the installed secret, counter
    (row << 16) | x, nonce call_nonce(call index, kind), Box-Muller on the first two 64-bit words of the block, evaluated EXACTLY (mpmath, 50 digits);
  * HostStream: the host layer's generator after mosfhet_seed (csrc/host/csprng.c).

Pure Python / numpy, no GPU and no native code.
"""
import struct

import mpmath
import numpy as np

M64 = (1 << 64) - 1
TWO_PI = 6.283185307179586            # the double both generators multiply u1 by
KIND_TABLE, KIND_BSK, KIND_BSK_UNFOLDED, KIND_TRLWE_KSK, KIND_TLWE_KSK = 1, 2, 3, 4, 5
MP_DIGITS = 50

_SIGMA_WORDS = struct.unpack("<4I", b"expand 32-byte k")


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def _quarter_round(x, a, b, c, d):
    """RFC 8439 section 2.1"""
    x[a] = x[a] + x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = x[c] + x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = x[a] + x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = x[c] + x[d]; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_blocks(key_words, counters, nonce64):
    """The blocks of all `counters` (any array of 64-bit counters) under one key and nonce: uint32 [len(counters)][16]."""
    counters = np.atleast_1d(np.asarray(counters, dtype=np.uint64))
    n = counters.size
    init = [np.full(n, w, dtype=np.uint32) for w in _SIGMA_WORDS]
    init += [np.full(n, int(w) & 0xFFFFFFFF, dtype=np.uint32) for w in key_words]
    init += [(counters & np.uint64(0xFFFFFFFF)).astype(np.uint32), (counters >> np.uint64(32)).astype(np.uint32)]
    init += [np.full(n, nonce64 & 0xFFFFFFFF, dtype=np.uint32), np.full(n, (nonce64 >> 32) & 0xFFFFFFFF, dtype=np.uint32)]
    assert len(init) == 16
    x = [w.copy() for w in init]
    with np.errstate(over="ignore"):
        for _ in range(10):                  # 20 rounds: ten column rounds, ten diagonal rounds
            _quarter_round(x, 0, 4, 8, 12); _quarter_round(x, 1, 5, 9, 13); _quarter_round(x, 2, 6, 10, 14); _quarter_round(x, 3, 7, 11, 15)
            _quarter_round(x, 0, 5, 10, 15); _quarter_round(x, 1, 6, 11, 12); _quarter_round(x, 2, 7, 8, 13); _quarter_round(x, 3, 4, 9, 14)
        return np.stack([x[i] + init[i] for i in range(16)], axis=1)


def chacha20_block(key_words, counter64, nonce64):
    """One block: a list of 16 output words."""
    return [int(w) for w in chacha20_blocks(key_words, [counter64 & M64], nonce64 & M64)[0]]


def key_words(secret32):
    """the eight little-endian key words of a 32-byte secret"""
    assert len(secret32) == 32
    return list(struct.unpack("<8I", bytes(secret32)))


def mask_word(seed, row, idx, stream=0):
    """Mask word `idx` of row `row` under the public seed; mask polynomial m of a k > 1 row is stream m."""
    z = (seed + 0x9E3779B97F4A7C15 * (row * 0x100000001B3 + idx * 4 + stream + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mask_row(seed, row, words, stream=0):
    """mask_word for idx = 0 .. words - 1 (numpy, wrap-around uint64)."""
    idx = np.arange(words, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & M64) + np.uint64(0x9E3779B97F4A7C15) * (np.uint64((row * 0x100000001B3 + stream + 1) & M64) + idx * np.uint64(4))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def call_nonce(call_index, kind):
    """Nonce of the `call_index`-th generate call (1-based) after the secret was installed."""
    return ((call_index << 8) | kind) & M64


def _uniform(u):
    return (mpmath.mpf(u >> 11) + mpmath.mpf(0.5)) * mpmath.mpf(2) ** -53


def gaussian_exact(u1, u2, sigma):
    """Box-Muller of two 64-bit uniforms as an mpmath real: cos(2 pi u1) sqrt(-2 ln u2) sigma."""
    with mpmath.workdps(MP_DIGITS):
        return mpmath.cos(mpmath.mpf(TWO_PI) * _uniform(u1)) * mpmath.sqrt(-2 * mpmath.log(_uniform(u2))) * mpmath.mpf(sigma)


def torus_of_exact(z):
    """double2torus of an exact real: times 2^64, truncated towards zero (a Python int, negative for negative z)."""
    with mpmath.workdps(MP_DIGITS):
        v = z * mpmath.mpf(2) ** 64
        return int(mpmath.floor(v)) if v >= 0 else -int(mpmath.floor(-v))


def _uniform_words(key, nonce, row, xs):
    blk = chacha20_blocks(key, (np.uint64(row << 16) | np.asarray(xs, dtype=np.uint64)), nonce)
    u1 = blk[:, 0].astype(np.uint64) | (blk[:, 1].astype(np.uint64) << np.uint64(32))
    u2 = blk[:, 2].astype(np.uint64) | (blk[:, 3].astype(np.uint64) << np.uint64(32))
    return u1, u2


def noise_term(key, nonce, row, x, sigma):
    """The noise term of coefficient x of row `row` as a signed Python int (exact evaluation)."""
    u1, u2 = _uniform_words(key, nonce, row, [x])
    return torus_of_exact(gaussian_exact(int(u1[0]), int(u2[0]), sigma))


def noise_row(key, nonce, row, words, sigma, exact_words=64):
    """noise_term for x = 0 .. words - 1 as int64: the first `exact_words` evaluated exactly, the rest in double (within 2^-47 sigma of the exact value: inside the
    comparison's 2^-40 sigma with 7 bits to spare)."""
    u1, u2 = _uniform_words(key, nonce, row, np.arange(words))
    f1 = ((u1 >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    f2 = ((u2 >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    z = np.cos(TWO_PI * f1) * np.sqrt(-2.0 * np.log(f2)) * sigma
    out = np.trunc(18446744073709551616.0 * z).astype(np.int64)
    for x in range(min(exact_words, words)):
        out[x] = torus_of_exact(gaussian_exact(int(u1[x]), int(u2[x]), sigma))
    return out


def noise_tolerance(sigma):
    """|got - reference| <= 1 (the truncation) + sigma 2^64 2^-40 (the double evaluation of cos, log and sqrt, measured at 2^-47.6 sigma on the host)."""
    return 1 + sigma * 2.0 ** 64 * 2.0 ** -40


class HostStream:
    """The host layer's generator after mosfhet_seed(seed): process key = the first eight words of the block of key {seed lo, seed hi, "mosf", "het!", 0, 0, 0, 0}
    at counter 0, nonce 0; the seeding thread reads blocks at nonce 0, counters 0, 1, ..., two words per 64-bit draw; further threads take nonces 1, 2, ...."""

    def __init__(self, seed):
        self.key = chacha20_block([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, 0x6d6f7366, 0x68657421, 0, 0, 0, 0], 0, 0)[:8]
        self.pos = {}

    def draw64(self, nonce=0):
        p = self.pos.get(nonce, 0)
        self.pos[nonce] = p + 1
        blk = chacha20_block(self.key, p // 8, nonce)
        return blk[2 * (p % 8)] | (blk[2 * (p % 8) + 1] << 32)

    def bytes(self, count, nonce=0):
        """whole 64-bit draws, little-endian; a tail shorter than eight bytes still consumes a whole draw"""
        out = b""
        while len(out) < count:
            out += struct.pack("<Q", self.draw64(nonce))
        return out[:count]

    def normal_exact(self, sigma, nonce=0):
        u1 = self.draw64(nonce)
        u2 = self.draw64(nonce)
        return gaussian_exact(u1, u2, sigma)
