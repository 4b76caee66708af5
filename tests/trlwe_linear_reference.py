"""The contract of mosfhet_hip_trlwe_linear_batch / _extract_batch (include/mosfhet_hip.h) restated from the oracle's primitives -- torus_to_dft, dft_mul_addto,
dft_to_torus, trlwe_extract_tlwe -- and the exact negacyclic integer convolution it approximates.  Nothing here goes through the library under test."""
import numpy as np


def csr_of_dense(W):
    """W [rows_out][rows_in][N] -> (row_ptr, col, val [nnz][N]): every row lists col = 0 .. rows_in - 1 ascending, zero polynomials included"""
    rows_out, rows_in, N = W.shape
    return np.arange(rows_out + 1, dtype=np.int32) * rows_in, np.tile(np.arange(rows_in, dtype=np.int32), rows_out), W.reshape(-1, N)


def restatement(oracle, row_ptr, col, val, bias, x, idx=None):
    """acc_a = acc_b = +0.0; for e in row j's entries in the stored order: acc_c = mul_addto(acc_c, F(x[b][col_e].c), F(val_e)); out[b][j] = (G(acc_a), G(acc_b) + bias[j]);
    idx given: trlwe_extract_tlwe(out[b][j], idx).  x [count][rows_in][2][N] uint64, val [nnz][N] int64, bias [rows_out][N] uint64 or None."""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    count, rows_in, two, N = x.shape
    val = np.ascontiguousarray(np.asarray(val, dtype=np.int64).reshape(-1, N))
    rows_out = len(row_ptr) - 1
    fw = [oracle.torus_to_dft(np.ascontiguousarray(v.view(np.uint64))) for v in val]      # (double)(int64_t): a weight is converted exactly as a torus word is
    out = np.empty((count, rows_out, 2, N), dtype=np.uint64)
    for b in range(count):
        fx = [[oracle.torus_to_dft(np.ascontiguousarray(x[b, i, c])) for c in range(2)] for i in range(rows_in)]
        for j in range(rows_out):
            acc = [np.zeros(N, dtype=np.float64), np.zeros(N, dtype=np.float64)]
            for e in range(int(row_ptr[j]), int(row_ptr[j + 1])):
                for c in range(2):
                    acc[c] = oracle.dft_mul_addto(acc[c], fx[int(col[e])][c], fw[e])
            out[b, j, 0] = oracle.dft_to_torus(acc[0])
            out[b, j, 1] = oracle.dft_to_torus(acc[1])
            if bias is not None:
                out[b, j, 1] += np.asarray(bias, dtype=np.uint64)[j]
    if idx is None:
        return out
    ext = np.empty((count, rows_out, N + 1), dtype=np.uint64)
    for b in range(count):
        for j in range(rows_out):
            ext[b, j] = oracle.trlwe_extract_tlwe(np.ascontiguousarray(out[b, j]), int(idx))
    return ext


def negacyclic_exact(p, w):
    """p * w mod (X^N + 1, 2^64) in Python integers: p [N] torus words, w [N] signed weights -> [N] uint64"""
    N = len(p)
    pp = np.array([int(v) for v in p], dtype=object)
    acc = np.zeros(N, dtype=object)
    for k in range(N):
        wk = int(w[k])
        if wk:
            acc += np.concatenate((-pp[N - k:], pp[:N - k])) * wk       # X^k p: the top k coefficients wrap with a sign
    return np.array([int(v) % (1 << 64) for v in acc], dtype=np.uint64)


def exact(row_ptr, col, val, bias, x):
    """the map of `restatement` with every product exact (no bias rounding to speak of: integers mod 2^64)"""
    count, rows_in, two, N = x.shape
    rows_out = len(row_ptr) - 1
    out = np.zeros((count, rows_out, 2, N), dtype=np.uint64)
    for b in range(count):
        for j in range(rows_out):
            for e in range(int(row_ptr[j]), int(row_ptr[j + 1])):
                for c in range(2):
                    out[b, j, c] += negacyclic_exact(x[b, int(col[e]), c], val[e])
            if bias is not None:
                out[b, j, 1] += np.asarray(bias, dtype=np.uint64)[j]
    return out
