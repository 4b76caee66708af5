"""Expected words of the digit-parallel radix-integer callers (include/mosfhet_hip.h: mosfhet_hip_vec_*; mosfhet_amd/csrc/capi_vec.inc), composed of oracle primitives
that are each held to the reference -- tlwe_keyswitch, functional_bootstrap(_wo_extract), trlwe_lut_packing_keyswitch, trlwe_mv_extract, multivalue_bootstrap_phase1 /
phase2, trlwe_torus_packing, double2torus -- in the order of the reference application's gate sequences (applications/multi-ciphertext-arith: src/integer.c, src/ml.c,
src/lut.c; the constants of src/ufhe.c:44-94), ONE INTEGER AND ONE GATE AT A TIME: nothing here is batched, tiled, pooled or gathered.

An array of M integers of d digits is digit-major, [d][M][N + 1] uint64 (digit / (2 B) under the extracted TRLWE key).  Every function returns new arrays and leaves
its arguments unchanged; the two calls that consume a table in the real API (encrypted_lut, mux_array) return the consumed table next to the result.

Where the device call is documented to differ from the application, the documented behaviour is what stands here: vec_mul bootstraps ALL digits of b against every
digit of a (capi_vec.inc: "two bootstrap launches over all db x M digits of b"; the application leaves its loop early, src/integer.c:205, and keeps stale digits).
"""
import numpy as np


class Keys:
    """The evaluation keys as plain arrays: bk_dft float64 [n][2l][2][N] (oracle slot order), ks_rows uint64 [N][t][2^bb - 1][n + 1] (LWE key switch N -> n), pk_rows
    uint64 [N][B][pt][2^pbb - 1][2][N] (LUT-packing key, or None: then only add / sub / sl_add / extend)."""

    def __init__(self, oracle, bk_dft, l, Bg_bit, ks_rows, bb, pk_rows, pbb, B):
        self.O, self.bk_dft, self.l, self.Bg_bit, self.ks_rows, self.bb, self.pk_rows, self.pbb, self.B = oracle, bk_dft, l, Bg_bit, ks_rows, bb, pk_rows, pbb, B
        self.n, self.N, self.t, self.logB = bk_dft.shape[0], bk_dft.shape[-1], ks_rows.shape[1], B.bit_length() - 1
        assert B == 1 << self.logB and ks_rows.shape == (self.N, self.t, (1 << bb) - 1, self.n + 1)
        assert pk_rows is None or pk_rows.shape[:2] == (self.N, B)
        dt = lambda x: np.uint64(oracle.double2torus(x))
        self.dt = dt
        # src/ufhe.c:57-67
        self.addsub_lut = oracle.trlwe_torus_packing([dt(-1. / (4 * B))], 1, self.N)
        self.signextend_lut = oracle.trlwe_torus_packing([dt(0.)] * (B // 2) + [dt((B - 1.) / (2 * B))] * (B // 2), 1, self.N)
        # src/ml.c:15-19
        self.relu_top_lut = oracle.trlwe_torus_packing([dt(float(j) / (2 * B)) for j in range(B // 2)] + [dt(0.)] * (B // 2), 1, self.N)

    # ---- the gates ----
    def trivial(self, value):
        out = np.zeros(self.N + 1, dtype=np.uint64)
        out[self.N] = value
        return out

    def ks(self, c):
        return self.O.tlwe_keyswitch(np.ascontiguousarray(c), self.ks_rows, self.n, self.t, self.bb)

    def bs(self, tv, c_n):
        return self.O.functional_bootstrap(np.ascontiguousarray(tv), c_n, self.bk_dft, self.l, self.Bg_bit, self.B)

    def bs_wo(self, tv, c_n):
        return self.O.functional_bootstrap_wo_extract(np.ascontiguousarray(tv), c_n, self.bk_dft, self.l, self.Bg_bit, self.B)

    def pack(self, slots):
        assert len(slots) == self.B
        return self.O.trlwe_lut_packing_keyswitch(np.stack(slots), self.pk_rows, self.pbb)

    def mv1(self, c_n):
        return self.O.multivalue_bootstrap_phase1(c_n, self.bk_dft, self.l, self.Bg_bit, self.B)

    def mv2(self, lut, rot):
        return self.O.multivalue_bootstrap_phase2([int(x) for x in lut], rot, self.B, self.logB)

    def addto(self, acc, tv, scale):        # trlwe_mv_extract_tlwe_scaling_addto
        return self.O.trlwe_mv_extract(tv, 2, scale, acc=acc)

    def subto(self, acc, tv, scale):        # trlwe_mv_extract_tlwe_scaling_subto
        return self.O.trlwe_mv_extract(tv, 3, scale, acc=acc)


def _add_b(c, value):
    with np.errstate(over="ignore"):
        c[-1] += np.uint64(value)


def _sub_b(c, value):
    with np.errstate(over="ignore"):
        c[-1] -= np.uint64(value)


# ---- one integer: lists of digits [N + 1] ----
def _carry_step(K, c, i, last, fresh):
    """the body of ufhe_sl_add_integer's / ufhe_sl_addto_integer's loop (src/integer.c:94-101, 120-127) on digit i of the list c"""
    tv = K.bs_wo(K.addsub_lut, K.ks(c[i]))
    c[i] = K.subto(c[i], tv, K.B)
    _sub_b(c[i], K.dt(1. / 4))
    if not last:
        if fresh:
            c[i + 1] = K.trivial(K.dt(1. / (4 * K.B)))
        else:
            _add_b(c[i + 1], K.dt(1. / (4 * K.B)))
        c[i + 1] = K.addto(c[i + 1], tv, 1)


def _extend1(K, c, d_ini, signed):
    """ufhe_extend_integer (src/integer.c:62-76) on the list c"""
    if not signed:
        for i in range(d_ini, len(c)):
            c[i] = K.trivial(0)
    elif len(c) > d_ini:
        tv = K.bs_wo(K.signextend_lut, K.ks(c[d_ini - 1]))
        c[d_ini:] = list(K.O.trlwe_mv_extract(tv, 0, len(c) - d_ini))


def _sl_add1(K, a, g, b, h, dc, signed):
    """ufhe_sl_add_integer (src/integer.c:79-107)"""
    size = len(a) if signed else min(max(len(a) + g, len(b) + h) + 1, dc)
    c = [None] * max(dc, size)
    c[0] = K.trivial(0)
    with np.errstate(over="ignore"):
        for i in range(size):
            if 0 <= i - g < len(a):
                c[i] = c[i] + a[i - g]
            if 0 <= i - h < len(b):
                c[i] = c[i] + b[i - h]
            if i - g < 0 or i - h < 0:
                if i != size - 1:
                    c[i + 1] = K.trivial(0)
                continue
            _carry_step(K, c, i, i == size - 1, True)
    _extend1(K, c, size, signed)
    return c


def _sl_addto1(K, b, a, g, signed):
    """ufhe_sl_addto_integer (src/integer.c:110-132), on the list b"""
    size = len(a) if signed else min(len(a) + g + 1, len(b))
    with np.errstate(over="ignore"):
        for i in range(size):
            if 0 <= i - g < len(a):
                b[i] = b[i] + a[i - g]
            if i - g < 0:
                continue
            _carry_step(K, b, i, i == size - 1, False)


def _encrypted_lut1(K, sel, lut):
    """ufhe_encrypted_tlwe_lut (src/lut.c:6-20) on the list lut, in place: lut[0] = lut[selector]"""
    size, i = len(lut), 0
    while size > 1:
        assert size % K.B == 0, (size, K.B)
        tmp = K.ks(sel[i])
        for j in range(size // K.B):
            lut[j] = K.bs(K.pack(lut[j * K.B:(j + 1) * K.B]), tmp)
        size //= K.B
        i += 1


def _per_integer(fn, M, *arrays):
    """fn over the M integers of digit-major arrays: each array [d][M][row] -> a list of d digits"""
    return [fn(*[[x[i, m].copy() for i in range(x.shape[0])] for x in arrays]) for m in range(M)]


def _digit_major(results):
    """[M] lists of d digits -> [d][M][row]"""
    return np.ascontiguousarray(np.stack([np.stack(r) for r in results]).transpose(1, 0, 2))


# ---- the callers ----
def addsub(K, a, b, subtract=False):
    """ufhe_sl_add_integer with g = h = 0 at equal widths (src/integer.c:79-107) / ufhe_sub_integer (:135-155): the chain over all d digits, the last carry dropped"""
    d, M, _ = a.shape

    def one(x, y):
        if not subtract:
            return _sl_add1(K, x, 0, y, 0, d, True)
        c = [K.trivial(0)] + [None] * (d - 1)
        with np.errstate(over="ignore"):
            for i in range(d):
                c[i] = c[i] + x[i] - y[i]
                tv = K.bs_wo(K.addsub_lut, K.ks(c[i]))
                c[i] = K.addto(c[i], tv, K.B)
                _add_b(c[i], K.dt(1. / 4))
                if i != d - 1:
                    c[i + 1] = K.subto(K.trivial(K.dt(-1. / (4 * K.B))), tv, 1)
        return c
    return _digit_major(_per_integer(one, M, a, b))


def relu(K, a):
    """ufhe_relu_integer (src/ml.c:4-20)"""
    d, M, _ = a.shape

    def one(x):
        sel, zero = K.ks(x[d - 1]), K.trivial(0)
        out = [K.bs(K.pack([x[i]] * (K.B // 2) + [zero] * (K.B // 2)), sel) for i in range(d - 1)]
        return out + [K.bs(K.relu_top_lut, sel)]
    return _digit_major(_per_integer(one, M, a))


def encrypted_lut(K, table, sel):
    """ufhe_encrypted_tlwe_lut (src/lut.c:6-20) for M tables: table [size][M][row], sel [levels][M][row], least significant digit first -> (the selected entries
    [M][row], the consumed table [size][M][row] whose entry 0 they are)"""
    size, M, _ = table.shape

    def one(lut, s):
        _encrypted_lut1(K, s, lut)
        return lut
    consumed = _digit_major(_per_integer(one, M, table, sel))
    return consumed[0].copy(), consumed


def mux_array(K, tables, sel):
    """ufhe_mux_integer_array (src/lut.c:48-64): tables [size][d][M][row] -> (out [d][M][row], the consumed tables)"""
    size, d, M, _ = tables.shape
    consumed = np.stack([encrypted_lut(K, np.ascontiguousarray(tables[:, i]), sel)[1] for i in range(d)], axis=1)
    return consumed[0].copy(), consumed


def cmp(K, a, b, a_signed, b_signed):
    """ufhe_cmp_integer (src/integer.c:217-265) at equal widths -> [M][row]: 0 / 1 / 2 over 2 B for a < / = / > b"""
    d, M, _ = a.shape

    def one(x, y):
        c, one_ = K.trivial(0), K.trivial(K.dt(1. / (2 * K.B)))
        with np.errstate(over="ignore"):
            for i in range(d):
                c = K.bs(K.pack([c] + [one_] * (K.B - 1)), K.ks(x[i] - y[i]))
            for is_signed, top in ((a_signed, x[d - 1]), (b_signed, y[d - 1])):
                if is_signed:
                    c = K.bs(K.pack([c] * (K.B // 2) + [np.uint64(0) - c] * (K.B // 2)), K.ks(top))
        _add_b(c, K.dt(1. / (2 * K.B)))
        return [c]
    return _digit_major(_per_integer(one, M, a, b))[0]


def lut_cleartext(K, sel, lut, out_digits):
    """ufhe_lut_integer (src/lut.c:23-46): sel [levels][M][row], lut [size] cleartext words -> [out_digits][M][row]"""
    levels, M, _ = sel.shape
    lut = [int(x) for x in lut]
    groups = len(lut) // K.B
    assert groups * K.B == len(lut) and groups >= 1

    def one(s):
        rot = K.mv1(K.ks(s[0]))
        out = []
        for j in range(out_digits):
            enc = [K.mv2([(lut[i * K.B + q] >> (j * K.logB)) & (K.B - 1) for q in range(K.B)], rot) for i in range(groups)]
            _encrypted_lut1(K, s[1:], enc)
            out.append(enc[0])
        return out
    return _digit_major(_per_integer(one, M, sel))


def sl_add(K, a, g, b, h, dc, signed):
    """c = a B^g + b B^h (ufhe_sl_add_integer, src/integer.c:79-107): a [da][M][row], b [db][M][row] -> [dc][M][row]"""
    return _digit_major(_per_integer(lambda x, y: _sl_add1(K, x, g, y, h, dc, signed)[:dc], a.shape[1], a, b))


def sl_addto(K, b, a, g, signed):
    """b + a B^g (ufhe_sl_addto_integer, src/integer.c:110-132) -> the new b"""
    def one(y, x):
        _sl_addto1(K, y, x, g, signed)
        return y
    return _digit_major(_per_integer(one, b.shape[1], b, a))


def extend(K, c, d_ini, signed):
    """ufhe_extend_integer (src/integer.c:62-76): digits [d_ini, dc) <- 0 (unsigned) or the sign of digit d_ini - 1 -> the new c"""
    def one(x):
        _extend1(K, x, d_ini, signed)
        return x
    return _digit_major(_per_integer(one, c.shape[1], c))


def mul(K, a, b, dc, signed):
    """ufhe_mul_integer (src/integer.c:167-215): a [da][M][row], b [db][M][row] -> [dc][M][row]; all db digits of b go through both product tables at every digit of a"""
    da, db, B = a.shape[0], b.shape[0], K.B
    size = da if signed else min(da + db + 1, dc)

    def one(x, y):
        c = [K.trivial(0) for _ in range(dc)]
        sel_b = [K.ks(y[j]) for j in range(db)]
        for i in range(da):
            rot = K.mv1(K.ks(x[i]))
            mulmod = K.pack([K.trivial(0), x[i]] + [K.mv2([(j * q) % B for q in range(B)], rot) for j in range(2, B)])
            mulquo = K.pack([K.trivial(0), K.trivial(0)] + [K.mv2([(j * q) // B for q in range(B)], rot) for j in range(2, B)])
            prod = [K.bs(mulmod, s) for s in sel_b]
            carry = [K.bs(mulquo, s) for s in sel_b]
            res = _sl_add1(K, prod, 0, carry, 1, db + (0 if signed else 1), signed)
            _sl_addto1(K, c, res, i, signed)
        if signed:
            _extend1(K, c, size, True)
        return c
    return _digit_major(_per_integer(one, a.shape[1], a, b))


# ---- reading results ----
def phases(oracle, ct, s):
    """torus phases of an array [...][N + 1] under the LWE key s"""
    flat = np.ascontiguousarray(ct).reshape(-1, ct.shape[-1])
    return np.array([oracle.tlwe_phase(c, s) for c in flat], dtype=np.uint64).reshape(ct.shape[:-1])


def read(oracle, ct, s, B):
    """(the nearest position [...] of every phase in [0, 2 B), that position's digit in [0, B), the worst distance of a phase from its position in units of
    1 / (2 B)) of an array [...][N + 1]"""
    units = phases(oracle, ct, s).astype(np.float64) / 2.0 ** 64 * (2 * B)
    pos = np.round(units)
    return pos.astype(np.int64) % (2 * B), pos.astype(np.int64) % B, float(np.abs(units - pos).max())


def to_int(digits, B):
    """digit-major digits [d][M] -> the M unsigned values (Python ints)"""
    logB = B.bit_length() - 1
    return [sum(int(digits[i][m]) << (logB * i) for i in range(len(digits))) for m in range(len(digits[0]))]


def encrypt(oracle, rng, values, d, s, B, sigma):
    """ufhe_encrypt_integer (src/integer.c:29-35): the low d digits of every value -> [d][M][N + 1]"""
    logB = B.bit_length() - 1
    return np.stack([np.stack([oracle.tlwe_sample(rng, oracle.double2torus(float((int(v) >> (logB * i)) & (B - 1)) / (2 * B)), s, sigma) for v in values]) for i in range(d)])
