"""Expected words of mosfhet_hip_trlwe_unpack_batch: a numpy restatement of the reference's trlwe_extract_tlwe (src/trlwe.c:540-552, k = 1) over a batch.

    extract(c, j).a[i] = c.a[j - i] for i <= j,  -c.a[N + j - i] for i > j;      extract(c, j).b = c.b[j]

tests/test_trlwe_unpack.py holds it to oracle.trlwe_extract_tlwe, to the reference's own function and, column by column, to oracle.poly_mul_by_xai.
"""
import numpy as np


def unpack(c, count=None):
    """c [2][N] -> [count][N + 1]: samples 0 .. count - 1 of one packed input (count defaults to N)"""
    a, b = c
    N = a.size
    count = N if count is None else count
    j = np.arange(count)[:, None]
    i = np.arange(N)[None, :]
    idx = (j - i) % N
    with np.errstate(over="ignore"):
        mask = np.where(i <= j, a[idx], np.uint64(0) - a[idx])
    out = np.empty((count, N + 1), dtype=np.uint64)
    out[:, :N] = mask
    out[:, N] = b[:count]
    return out


def unpack_batch(trlwe, total, per):
    """trlwe [outputs][2][N] -> [total][N + 1]: sample o per + j = extract(trlwe[o], j); the last input may be opened in part"""
    trlwe = np.ascontiguousarray(trlwe, dtype=np.uint64)
    N = trlwe.shape[2]
    assert 1 <= per <= N and 0 <= total <= trlwe.shape[0] * per
    out = np.empty((total, N + 1), dtype=np.uint64)
    for o in range(-(-total // per)):
        lo, hi = o * per, min(total, (o + 1) * per)
        out[lo:hi] = unpack(trlwe[o], hi - lo)
    return out
