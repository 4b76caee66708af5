"""The encrypted automata of include/mosfhet_hip.h (mosfhet_hip_trlwe_automaton_batch) restated on the CPU from oracle.external_product, oracle.poly_mul_by_xai and word
arithmetic mod 2^64 alone.  A state vector is [states][2][N] uint64; the tables next0, next1, rot0, rot1 are integer arrays [layers][states]; sel_dft is
[steps][2l][2][N] doubles in the oracle's order (oracle.bk_to_dft of the selector words), selector t encrypting symbol t of the word.
"""
import numpy as np


def rotate(oracle, c, a):
    """X^a c for a in [0, 2N): the exact negacyclic rotation of both components"""
    return np.stack([oracle.poly_mul_by_xai(np.ascontiguousarray(c[0]), int(a)), oracle.poly_mul_by_xai(np.ascontiguousarray(c[1]), int(a))])


def step(oracle, V, tables, lam, sel_dft_t, l, Bg, states=None):
    """V_t from V = V_{t+1} with layer lam: V_t[q] = R0 + sel (.) (R1 - R0), R0 = X^rot0[q] V[next0[q]], R1 = X^rot1[q] V[next1[q]]; `states`: the q to compute"""
    next0, next1, rot0, rot1 = tables
    out = []
    for q in (range(V.shape[0]) if states is None else states):
        R0 = rotate(oracle, V[next0[lam][q]], rot0[lam][q])
        R1 = rotate(oracle, V[next1[lam][q]], rot1[lam][q])
        out.append(R0 + oracle.external_product(np.ascontiguousarray(R1 - R0), sel_dft_t, l, Bg))
    return np.stack(out)


def run(oracle, tables, sel_dft, init, l, Bg, start=-1):
    """V_0 ([states][2][N]) with start < 0, else V_0[start] ([2][N]); backwards from V_steps = init, position t using layer t mod layers"""
    tables = [np.atleast_2d(np.asarray(a)) for a in tables]
    layers, steps = tables[0].shape[0], sel_dft.shape[0]
    V = init
    for t in range(steps - 1, -1, -1):
        V = step(oracle, V, tables, t % layers, sel_dft[t], l, Bg, [start] if t == 0 and start >= 0 else None)
    return V if start < 0 else V[0]
