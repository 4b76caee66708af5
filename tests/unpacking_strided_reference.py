"""Expected words of mosfhet_hip_trlwe_unpack_strided_batch: sample j of an input is the reference's trlwe_extract_tlwe (src/trlwe.c:540-552, k = 1) at the coefficient
first + j stride -- rows first + stride * arange(.) of unpacking_reference.unpack, which restates that function for every coefficient of one input.

tests/test_trlwe_unpack_strided.py holds it to oracle.trlwe_extract_tlwe and to the reference's own function.
"""
import numpy as np

import unpacking_reference


def unpack(c, count, first, stride):
    """c [2][N] -> [count][N + 1]: the samples at the coefficients first, first + stride, ..., first + (count - 1) stride of one packed input; no index wraps"""
    N = c.shape[1]
    assert count >= 0 and 0 <= first < N and stride >= 1 and (count == 0 or first + (count - 1) * stride <= N - 1)
    return unpacking_reference.unpack(c)[first + stride * np.arange(count)]


def unpack_batch(trlwe, total, per, first, stride):
    """trlwe [outputs][2][N] -> [total][N + 1]: sample o per + j = extract(trlwe[o], first + j stride); the last input may be opened in part"""
    trlwe = np.ascontiguousarray(trlwe, dtype=np.uint64)
    N = trlwe.shape[2]
    assert 1 <= per and 0 <= first < N and stride >= 1 and first + (per - 1) * stride <= N - 1 and 0 <= total <= trlwe.shape[0] * per
    out = np.empty((total, N + 1), dtype=np.uint64)
    for o in range(-(-total // per)):
        lo, hi = o * per, min(total, (o + 1) * per)
        out[lo:hi] = unpack(trlwe[o], hi - lo, first, stride)
    return out
