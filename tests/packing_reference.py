"""Expected words of mosfhet_hip_tlwe_pack_batch: the reference's trlwe_full_packing_keyswitch (src/keyswitch.c:195-227) composed from oracle primitives that are
each held to the reference (tests/test_oracle_vs_reference.py) -- poly_decompose_i, torus_to_dft, dft_mul_addto, dft_to_torus -- in the reference's order.
tests/test_tlwe_pack.py holds this composition to the reference's own function."""
import numpy as np

from oracle import oracle as O


def pack(cts, ks_dft, t, base_bit, N, split=1):
    """One output: cts u64 [samples <= N][n_in + 1] -> TRLWE u64 [2][N], sample j at coefficient j.  ks_dft float64 [n_in][t][2][N]: O.ks_to_dft of the torus rows,
    entry i switching from the constant polynomial s_in[i].  split = 1: one accumulator pair, entries ascending, rows j < t ascending, one dft_to_torus per
    component, out.a = -as.a, out.b[j] = in[j].b - as.b[j].  split = P: P consecutive parts of ceil(n_in / P) entries (the last shorter, possibly empty), an
    accumulator pair and a rounding per part, the rounded parts subtracted as 64-bit integers."""
    cts = np.ascontiguousarray(cts, dtype=np.uint64)
    samples, n_in = cts.shape[0], cts.shape[1] - 1
    assert 1 <= samples <= N and ks_dft.shape == (n_in, t, 2, N) and 1 <= split <= n_in
    out = np.zeros((2, N), dtype=np.uint64)
    out[1, :samples] = cts[:, n_in]
    step = -(-n_in // split)
    for part in range(split):
        acc = [np.zeros(N, dtype=np.float64), np.zeros(N, dtype=np.float64)]
        for i in range(part * step, min(n_in, (part + 1) * step)):
            a_i = np.zeros(N, dtype=np.uint64)
            a_i[:samples] = cts[:, i]
            for j in range(t):
                digits = O.torus_to_dft(O.poly_decompose_i(a_i, base_bit, t, j))
                for c in range(2):
                    acc[c] = O.dft_mul_addto(acc[c], digits, np.ascontiguousarray(ks_dft[i, j, c]))
        with np.errstate(over="ignore"):
            for c in range(2):
                out[c] -= O.dft_to_torus(acc[c])
    return out


def pack_batch(cts, ks_dft, t, base_bit, N, per, split=1):
    """The batch: [total][n_in + 1] -> [ceil(total / per)][2][N], each output by pack() alone."""
    return np.stack([pack(cts[lo:lo + per], ks_dft, t, base_bit, N, split) for lo in range(0, len(cts), per)])
