"""Expected words of the trace switch and of the gadget -> TRGSW conversion (include/mosfhet_hip.h: mosfhet_hip_tlwe_trace_pack_batch,
mosfhet_hip_trlwe_rlwe_priv_keyswitch_batch, mosfhet_hip_trgsw_from_gadget_batch), composed of oracle primitives that are each held to the reference, in the order of
the reference's trlwe_packing1_keyswitch_CDKS21 (src/keyswitch.c:526-546), trlwe_RLWE_priv_keyswitch (:65-97) and trgsw_from_gadget (:559-572).

Keys are [entries][t][2][N]: torus words for the device (Engine.load_trlwe_ks_keys), their transforms in the oracle's order (oracle.ks_to_dft) for the helpers.
"""
import numpy as np


def log2n(N):
    return N.bit_length() - 1


def trace_gens(N):
    """the generators of the trace, step j: N / 2^j + 1"""
    return [(N >> j) + 1 for j in range(log2n(N))]


def gen_trace_keys(oracle, rng, s, t, base_bit, sigma):
    """trlwe_new_packing1_KS_key_CDKS21 (src/keyswitch.c:477-498): entry j switches from s(X^(2^(logN - j) + 1)) to s.  -> torus words [log2 N][t][2][N]"""
    N = s.size
    return np.stack([oracle.gen_trlwe_ks_key(rng, oracle.poly_permute(s, (1 << (log2n(N) - j)) + 1), s, t, base_bit, sigma) for j in range(log2n(N))])


def gen_gadget_keys(oracle, rng, s, t, base_bit, sigma):
    """trlwe_new_gadget_to_RGSW_KS (src/keyswitch.c:574-608, k = 1): v = -s; entry 0 switches from s v, entry 1 from v.  -> [2][t][2][N]"""
    with np.errstate(over="ignore"):
        v = np.uint64(0) - s
    return np.stack([oracle.gen_trlwe_ks_key(rng, oracle.poly_naive_mul(v, s), s, t, base_bit, sigma), oracle.gen_trlwe_ks_key(rng, v, s, t, base_bit, sigma)])


def embed(c, N):
    """the LWE sample as the TRLWE sample whose constant coefficient carries its phase: a[0] = in.a[0], a[N - i] = -in.a[i], b = in.b X^0"""
    out = np.zeros((2, N), dtype=np.uint64)
    with np.errstate(over="ignore"):
        out[0, 0] = c[0]
        out[0, 1:] = (np.uint64(0) - c[1:N])[::-1]
    out[1, 0] = c[N]
    return out


def trace_step(oracle, acc, gen, key_dft, t, base_bit):
    """acc + KeySwitch(acc(X^gen)): poly_permute on both components, trlwe_keyswitch, add"""
    tmp = np.stack([oracle.poly_permute(np.ascontiguousarray(acc[0]), gen), oracle.poly_permute(np.ascontiguousarray(acc[1]), gen)])
    with np.errstate(over="ignore"):
        return acc + oracle.trlwe_keyswitch(tmp, np.ascontiguousarray(key_dft), t, base_bit)


def trace_pack(oracle, c, keys_dft, t, base_bit, N):
    """one sample [N + 1] -> [2][N]; keys_dft [log2 N][t][2][N]"""
    acc = embed(c, N)
    for j, gen in enumerate(trace_gens(N)):
        acc = trace_step(oracle, acc, gen, keys_dft[j], t, base_bit)
    return acc


def trace_pack_batch(oracle, cts, keys_dft, t, base_bit, N):
    return np.stack([trace_pack(oracle, c, keys_dft, t, base_bit, N) for c in cts]) if len(cts) else np.zeros((0, 2, N), dtype=np.uint64)


def rlwe_priv_keyswitch(oracle, c, keys_dft, t, base_bit):
    """-(trlwe_keyswitch((in.b, 0), K1)) + trlwe_keyswitch((in.a, 0), K0); keys_dft [2][t][2][N]"""
    z = np.zeros(c.shape[1], dtype=np.uint64)
    as_ = oracle.trlwe_keyswitch(np.stack([c[0], z]), np.ascontiguousarray(keys_dft[0]), t, base_bit)
    bs_ = oracle.trlwe_keyswitch(np.stack([c[1], z]), np.ascontiguousarray(keys_dft[1]), t, base_bit)
    with np.errstate(over="ignore"):
        return (np.uint64(0) - bs_) + as_


def trgsw_from_gadget(oracle, gadget, keys_dft, t, base_bit):
    """gadget [l][2][N] -> the TRGSW in the torus domain [2l][2][N]: rows i < l the private switch of row i, rows l + i the rows themselves"""
    return np.stack([rlwe_priv_keyswitch(oracle, g, keys_dft, t, base_bit) for g in gadget] + [g for g in gadget])


def digit_boundary_words(t, base_bit):
    """mask words on both sides of where a digit of the (t, base_bit) decomposition changes: the rounding offset 2^(63 - t base_bit) carries at x = k 2^(64 - t base_bit)
    - 2^(63 - t base_bit); the words around the first such x of every digit position, and around the wrap of the top digit"""
    out = []
    half = 1 << (63 - t * base_bit)
    for j in range(1, t + 1):
        edge = ((1 << (64 - j * base_bit)) - half) % (1 << 64)
        out += [(edge - 1) % (1 << 64), edge, (edge + 1) % (1 << 64)]
    top = ((1 << 63) - half) % (1 << 64)
    out += [(top - 1) % (1 << 64), top, (top + 1) % (1 << 64)]
    return np.array(out, dtype=np.uint64)
