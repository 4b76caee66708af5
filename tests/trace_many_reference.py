"""Expected words of mosfhet_hip_tlwe_trace_pack_many_batch (include/mosfhet_hip.h has the definition): 2^L LWE samples packed into one TRLWE sample through a binary
tree of merges and the rest of the trace, composed of the oracle primitives tests/trace_reference.py composes -- poly_permute, trlwe_keyswitch -- and the exact negacyclic
shift.  Keys as there: keys_dft [log2 N][t][2][N], entry j switching from s(X^(N / 2^j + 1)).
"""
import numpy as np

import trace_reference as R


def shift(p, s):
    """X^s p for a TRLWE sample [2][N] (or one polynomial [N]), 0 <= s < N: the exact negacyclic shift"""
    out = np.roll(p, s, axis=-1)
    with np.errstate(over="ignore"):
        out[..., :s] = np.uint64(0) - out[..., :s]
    return out


def merge(oracle, E, P1, lvl, keys_dft, t, base_bit, N):
    """one merge of level lvl: O = X^(N / 2^lvl) P1, U = E + O, V = E - O, U + KeySwitch_(log2 N - lvl)(V(X^(2^lvl + 1)))  -> (result, U, V)"""
    O = shift(P1, N >> lvl)
    with np.errstate(over="ignore"):
        U, V = E + O, E - O
    gen = (1 << lvl) + 1
    tmp = np.stack([oracle.poly_permute(np.ascontiguousarray(V[0]), gen), oracle.poly_permute(np.ascontiguousarray(V[1]), gen)])
    with np.errstate(over="ignore"):
        return U + oracle.trlwe_keyswitch(tmp, np.ascontiguousarray(keys_dft[R.log2n(N) - lvl]), t, base_bit), U, V


def pack_one(oracle, cts, L, keys_dft, t, base_bit, N):
    """the samples of one output, at most 2^L of them [<= n][N + 1] (missing ones are all-zero samples) -> [2][N]"""
    n = 1 << L
    P = [R.embed(cts[j], N) if j < len(cts) else np.zeros((2, N), dtype=np.uint64) for j in range(n)]
    for lvl in range(1, L + 1):
        half = n >> lvl
        P = [merge(oracle, P[r], P[r + half], lvl, keys_dft, t, base_bit, N)[0] for r in range(half)]
    acc = P[0]
    for j in range(R.log2n(N) - L):
        acc = R.trace_step(oracle, acc, (N >> j) + 1, keys_dft[j], t, base_bit)
    return acc


def pack_many(oracle, cts, L, keys_dft, t, base_bit, N):
    """[total][N + 1] -> [ceil(total / 2^L)][2][N]"""
    n = 1 << L
    outs = [pack_one(oracle, cts[o:o + n], L, keys_dft, t, base_bit, N) for o in range(0, len(cts), n)]
    return np.stack(outs) if outs else np.zeros((0, 2, N), dtype=np.uint64)


def expected_phase(msgs, L, N):
    """N m_j at coefficient j N / 2^L of the output sample j belongs to: msgs [total] -> [outputs][N]"""
    n = 1 << L
    exp = np.zeros((-(-len(msgs) // n), N), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for j, m in enumerate(msgs):
            exp[j // n, (j % n) * (N // n)] = np.uint64(m) * np.uint64(N)
    return exp
