"""The contract of mosfhet_hip_trlwe_gsw_linear_batch / _extract_batch (include/mosfhet_hip.h) restated from the oracle's primitives -- poly_decompose_i, torus_to_dft,
dft_mul_addto, dft_to_torus, trlwe_extract_tlwe, trgsw_to_dft -- and the helpers that make TRGSW samples for its tests.  Nothing here goes through the library under
test."""
import numpy as np


def csr_of_dense(W):
    """W [rows_out][rows_in][2l][2][N] -> (row_ptr, col, W [nnz][2l][2][N]): every row lists col = 0 .. rows_in - 1 ascending"""
    rows_out, rows_in = W.shape[:2]
    return np.arange(rows_out + 1, dtype=np.int32) * rows_in, np.tile(np.arange(rows_in, dtype=np.int32), rows_out), W.reshape((-1,) + W.shape[2:])


def restatement(oracle, row_ptr, col, W, bias, x, l, Bg_bit, idx=None):
    """acc_a = acc_b = +0.0; for e in row j's entries in the stored order: for c in (a, b): for i < l: d = F(dec_i(x[b][col_e].c)); acc_a = mul_addto(acc_a, d,
    W_e[c l + i].a); acc_b = mul_addto(acc_b, d, W_e[c l + i].b); out[b][j] = (G(acc_a), G(acc_b) + bias[j]); idx given: trlwe_extract_tlwe(out[b][j], idx).
    x [count][rows_in][2][N] uint64, W [nnz][2l][2][N] uint64 torus words, bias [rows_out][N] uint64 or None."""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    count, rows_in, two, N = x.shape
    W = np.ascontiguousarray(np.asarray(W, dtype=np.uint64).reshape(-1, 2 * l, 2, N))
    rows_out = len(row_ptr) - 1
    fw = [oracle.trgsw_to_dft(w, 1, l) for w in W]
    used = sorted(set(int(c) for c in col))
    out = np.empty((count, rows_out, 2, N), dtype=np.uint64)
    for b in range(count):
        d = {i: [oracle.torus_to_dft(oracle.poly_decompose_i(np.ascontiguousarray(x[b, i, c]), Bg_bit, l, lev)) for c in range(2) for lev in range(l)] for i in used}
        for j in range(rows_out):
            acc = [np.zeros(N, dtype=np.float64), np.zeros(N, dtype=np.float64)]
            for e in range(int(row_ptr[j]), int(row_ptr[j + 1])):
                for r in range(2 * l):                      # r = c l + i: a first, then b
                    for o in range(2):
                        acc[o] = oracle.dft_mul_addto(acc[o], d[int(col[e])][r], np.ascontiguousarray(fw[e][r, o]))
            out[b, j, 0] = oracle.dft_to_torus(acc[0])
            out[b, j, 1] = oracle.dft_to_torus(acc[1])
            if bias is not None:
                out[b, j, 1] += np.asarray(bias, dtype=np.uint64)[j]
    if idx is None:
        return out
    return extracted(oracle, out, idx)


def extracted(oracle, trlwe, idx):
    count, rows_out, two, N = trlwe.shape
    return np.stack([oracle.trlwe_extract_tlwe(np.ascontiguousarray(s), int(idx)) for s in trlwe.reshape(-1, 2, N)]).reshape(count, rows_out, N + 1)


def trgsw_of_polynomial(oracle, rng, mu, s, l, Bg_bit, sigma):
    """A TRGSW sample of the polynomial mu [N] (signed coefficients) under the ring key s [1][N]: 2l zero trlwe_samples plus mu 2^(64 - (i + 1) Bg_bit) on the row's own
    component (rows 0 .. l - 1: a, rows l .. 2l - 1: b) -> [2l][2][N] uint64"""
    N = s.shape[1]
    mu = np.asarray(mu, dtype=np.int64).view(np.uint64)
    g = np.empty((2 * l, 2, N), dtype=np.uint64)
    for c in range(2):
        for i in range(l):
            g[c * l + i] = oracle.trlwe_sample(rng, None, s, sigma)
            g[c * l + i, c] += mu << np.uint64(64 - (i + 1) * Bg_bit)
    return g


def dot_layout(w, N, stride=1):
    """what mosfhet_polylinear_dot_layout writes: poly[0] = w[0], poly[N - c stride] = -w[c]"""
    poly = np.zeros(N, dtype=np.int64)
    poly[0] = w[0]
    for c in range(1, len(w)):
        poly[N - c * stride] = -int(w[c])
    return poly
