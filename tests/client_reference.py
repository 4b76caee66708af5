"""Plain reference of the client half's samples (include/mosfhet_hip.h "The client half on the device"; csrc/client_kernels.h), written from its specification on
tests/keygen_reference.py: the ChaCha20 block function, the noise terms (noise_row: Box-Muller evaluated exactly) and the comparison's tolerance.

  * mask_row: mask word x of row `row` = output words 4 - 5 (low word first) of the block whose words 0 - 3 give that coefficient's noise term: counter
    (row << 16) | x, nonce call_nonce(call index, kind) with kind 6 (TLWE), 7 (TRLWE), 8 (TRGSW);
  * tlwe_sample / trlwe_sample / trgsw_sample: the three sample formats, every word, with the noise terms of noise_row;
  * negacyclic_mul: the exact product a * s mod (X^N + 1, 2^64) as shifted adds over the key's nonzero coefficients;
  * tlwe_phase / trlwe_phase / decode: the opening rule.

Pure Python / numpy, no GPU and no native code.
"""
import numpy as np

import keygen_reference as R

M64 = R.M64
U64 = np.uint64
KIND_TLWE, KIND_TRLWE, KIND_TRGSW = 6, 7, 8


def mask_row(key, nonce, row, words):
    """mask words x = 0 .. words - 1 of row `row`"""
    blk = R.chacha20_blocks(key, (U64(row << 16) | np.arange(words, dtype=U64)), nonce)
    return blk[:, 4].astype(U64) | (blk[:, 5].astype(U64) << U64(32))


def noise_words(key, nonce, row, words, sigma, exact_words=64):
    """the noise terms of row `row` as torus words (two's complement)"""
    return R.noise_row(key, nonce, row, words, sigma, exact_words).view(U64)


def negacyclic_mul(a, s):
    """(a * s)[x] = sum over nonzero s_p of s_p * (a[x - p] for x >= p, -a[N + x - p] below), mod 2^64"""
    a, s = np.asarray(a, dtype=U64), np.asarray(s, dtype=U64)          # (negative key coefficients: two's complement words, the same product mod 2^64)
    N = a.size
    out = np.zeros(N, dtype=U64)
    with np.errstate(over="ignore"):
        ext = np.concatenate([U64(0) - a, a])                          # ext[i] = -a[i], ext[N + i] = a[i]
        for p in np.flatnonzero(s):
            out += ext[N - p:2 * N - p] * s[p]
    return out


def tlwe_sample(key, nonce, row, s, msg, sigma):
    """[n + 1]: out[i] = a_i (mask word i), out[n] = sum a_i s_i + e + msg with e the noise term of coefficient 0"""
    s = np.asarray(s, dtype=U64)
    a = mask_row(key, nonce, row, s.size)
    with np.errstate(over="ignore"):
        b = (a * s).sum(dtype=U64) + noise_words(key, nonce, row, 1, sigma)[0] + U64(int(msg) & M64)
    return np.concatenate([a, [b]]).astype(U64)


def trlwe_sample(key, nonce, row, s, msg, sigma, mul=negacyclic_mul):
    """[2][N]: a = the mask words, b = a * s + e + msg (msg None: zero)"""
    N = len(s)
    a = mask_row(key, nonce, row, N)
    with np.errstate(over="ignore"):
        b = mul(a.copy(), np.asarray(s, dtype=U64)) + noise_words(key, nonce, row, N, sigma)
        if msg is not None:
            b = b + np.asarray(msg, dtype=U64)
    return np.stack([a, b])


def gadget_rows(N, m, exp, l, Bg_bit):
    """[2l][2][N]: what trgsw_monomial_sample adds to the 2l fresh TRLWE(0) rows: m 2^(64 - (j+1) Bg_bit) X^exp on component c of row c l + j; exponent mod 2N, X^N = -1"""
    out = np.zeros((2 * l, 2, N), dtype=U64)
    e = int(exp) % (2 * N)
    for c in range(2):
        for j in range(l):
            h = (int(m) << (64 - (j + 1) * Bg_bit)) & M64
            out[c * l + j, c, e % N] = (-h if e >= N else h) & M64
    return out


def trgsw_sample(key, nonce, sample, s, m, exp, l, Bg_bit, sigma, mul=negacyclic_mul):
    """[2l][2][N]: row q of sample `sample` is row number sample * 2l + q of the call, a fresh TRLWE(0); the gadget is added AFTER b was formed from the plain mask"""
    rows = np.stack([trlwe_sample(key, nonce, sample * 2 * l + q, s, None, sigma, mul) for q in range(2 * l)])
    return rows + gadget_rows(len(s), m, exp, l, Bg_bit)


def tlwe_phase(c, s):
    c, s = np.asarray(c, dtype=U64), np.asarray(s, dtype=U64)
    with np.errstate(over="ignore"):
        return c[..., -1] - (c[..., :-1] * s).sum(axis=-1, dtype=U64)


def trlwe_phase(c, s, mul=negacyclic_mul):
    return np.asarray(c[1], dtype=U64) - mul(np.asarray(c[0], dtype=U64).copy(), np.asarray(s, dtype=U64))


def decode(phase, msg_bits):
    """msg_bits = 0: the phase; else (phase + 2^(63 - msg_bits)) >> (64 - msg_bits), mod 2^64 before the shift"""
    phase = np.asarray(phase, dtype=U64)
    if msg_bits == 0:
        return phase
    with np.errstate(over="ignore"):
        return (phase + U64(1 << (63 - msg_bits))) >> U64(64 - msg_bits)
