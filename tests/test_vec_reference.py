"""tests/vec_reference.py -- the radix-integer callers composed over the oracle, what tests/test_vec_callers_bits.py compares the device with bit for bit -- held to
the ARITHMETIC first, without a GPU: a reference that is wrong in the way the device code is wrong would prove nothing.

Keys come from the oracle's own generators at a ring small enough for the LUT-packing key to take about a second (N = 256, n = 12, l = 2, Bg = 2^8; key switch and
packing switch t = 7, base 2^2 -- at t = 6 the multiplication at B = 8 reached 0.065 of a digit position here, and four times that is past the 0.25 this file allows
itself; what is left at t = 7 is the 2 x 2^8 gadget's rounding through the multi-value bootstrap's second phase.  vec_reference.py does not depend on the ring).  One key set per digit base B, generated once per module.

Every caller must (a) decrypt to the integer arithmetic it stands for, (b) leave its arguments unchanged, (c) keep every output digit's phase within a bound of its
position.  Decryption needs 0.5 of a position (1 / (2 B) of the torus).  The bounds asserted are 4 x the worst error MEASURED with these keys and inputs (a noise
maximum over a few dozen samples: the factor covers other seeds), all below 0.25: WORST below lists the measurements, in positions.
"""
import numpy as np
import pytest

import vec_reference as V

N, n, l, Bg, T, BB = 256, 12, 2, 8, 7, 2
# worst |phase - position| per (caller, B), in units of 1 / (2 B), as measured on the CPU with the keys and inputs of this file; the tests assert 4 x these
WORST = {
    ("add", 4): 0.0084,
    ("cmp", 2): 0.0033,
    ("cmp", 4): 0.0079,
    ("cmp", 8): 0.0107,
    ("encrypted_lut", 4): 0.0028,
    ("extend", 4): 0.0018,
    ("lut_cleartext", 2): 0.0014,
    ("lut_cleartext", 4): 0.0101,
    ("lut_cleartext", 8): 0.0495,
    ("mul", 2): 0.0033,
    ("mul", 4): 0.0236,
    ("mul", 8): 0.0518,
    ("mux_array", 4): 0.0048,
    ("relu", 2): 0.0016,
    ("relu", 4): 0.0026,
    ("relu", 8): 0.0057,
    ("sl_add", 4): 0.0084,
    ("sl_addto", 4): 0.0065,
    ("sub", 4): 0.0077,
}


EVERY_BASE = pytest.mark.parametrize("keys", [4, 2, 8], indirect=True, ids=lambda B: "B%d" % B)
BASE_4 = pytest.mark.parametrize("keys", [4], indirect=True, ids=lambda B: "B%d" % B)


@pytest.fixture(scope="module")
def keys(request, oracle):
    B = request.param
    r = oracle.Rng(0x5EED00 + B)
    lwe_s, s = oracle.gen_binary_key(r, n), oracle.gen_binary_key(r, N)
    bk_dft = oracle.bk_to_dft(oracle.gen_bootstrap_key(r, lwe_s, s.reshape(1, N), l, Bg, 2.0 ** -45), 1, l)
    ks = oracle.gen_tlwe_ks_key(r, s, lwe_s, T, BB, 2.0 ** -25)
    pk = oracle.gen_lut_packing_ks_key(r, s, s, T, BB, B, 2.0 ** -45)
    K = V.Keys(oracle, bk_dft, l, Bg, ks, BB, pk, BB, B)
    return {"K": K, "s": s, "r": r, "B": B, "O": oracle}


def _enc(keys, values, d):
    return V.encrypt(keys["O"], keys["r"], values, d, keys["s"], keys["B"], 2.0 ** -30)


def _run(keys, fn, *args):
    """fn(K, *args) with the array arguments checked to come back unchanged"""
    before = [a.copy() if isinstance(a, np.ndarray) else a for a in args]
    out = fn(keys["K"], *args)
    for a, b in zip(args, before):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, b), "%s changed an argument" % fn.__name__
    return out


def _held(keys, name, ct, want, positions=False):
    """ct decrypts to want (integers; positions: the raw position mod 2 B of a single digit, as the comparison's 0 / 1 / 2) within the caller's bound"""
    B = keys["B"]
    pos, dig, err = V.read(keys["O"], ct, keys["s"], B)
    got = [int(x) for x in pos.reshape(-1)] if positions else V.to_int(dig, B)
    print("%s B = %d: worst error %.4f positions" % (name, B, err))
    assert got == [int(w) for w in want], (name, B, got, want)
    bound = 4 * WORST[(name, B)]
    assert bound <= 0.25, (name, B, bound)
    assert err <= bound, (name, B, err, bound)


def _signed(v, d, B):
    """the value of the low d digits read as two's complement"""
    m = B ** d
    v %= m
    return v - m if v >= m // 2 else v


@BASE_4
def test_addsub_decrypts(keys):
    """add and subtract over d = 3 and d = 1: carries and borrows through every digit, the last one dropped"""
    B = keys["B"]
    for d in (3, 1):
        m = B ** d
        a_v, b_v = [5 % m, m - 1, 0, 37 % m, m // 2], [11 % m, 1, 0, 27 % m, m // 2]
        a, b = _enc(keys, a_v, d), _enc(keys, b_v, d)
        _held(keys, "add", _run(keys, V.addsub, a, b), [(x + y) % m for x, y in zip(a_v, b_v)])
        _held(keys, "sub", _run(keys, V.addsub, a, b, True), [(x - y) % m for x, y in zip(a_v, b_v)])


@EVERY_BASE
def test_relu_decrypts(keys):
    """d = 3 and d = 1 (no lower digit: the top digit's cleartext table alone); the largest positive, the smallest negative, zero, -1"""
    B = keys["B"]
    for d in (3, 1) if B == 4 else (2,):
        m = B ** d
        a_v = [m // 2 - 1, m // 2, 0, m - 1, 1 % m, (m // 2 + 1) % m]
        _held(keys, "relu", _run(keys, V.relu, _enc(keys, a_v, d)), [v if v < m // 2 else 0 for v in a_v])


@BASE_4
def test_encrypted_lut_and_mux_array_decrypt(keys):
    """one and two levels of the tree; a selector per instance; the array form over d = 2 digits and the bare copy of size 1"""
    B, rng = keys["B"], np.random.default_rng(7)
    for size in (B, B * B):
        levels = 1 if size == B else 2
        table_v = rng.integers(0, B, (size, 3))
        sel_v = [0, size - 1, size // 2 + 1]
        table = np.stack([_enc(keys, table_v[j], 1)[0] for j in range(size)])
        out, consumed = _run(keys, V.encrypted_lut, table, _enc(keys, sel_v, levels))
        assert np.array_equal(consumed[0], out) and consumed.shape == table.shape
        _held(keys, "encrypted_lut", out[None], [table_v[sel_v[m], m] for m in range(3)])
    size, d = B * B, 2
    vec_v = rng.integers(0, B ** d, (size, 3))
    sel_v = [size - 1, 0, 6]
    tables = np.stack([_enc(keys, vec_v[j], d) for j in range(size)])
    out, _ = _run(keys, V.mux_array, tables, _enc(keys, sel_v, 2))
    _held(keys, "mux_array", out, [vec_v[sel_v[m], m] for m in range(3)])
    out, consumed = _run(keys, V.mux_array, tables[:1], _enc(keys, sel_v, 2)[:0])
    assert np.array_equal(out, tables[0]) and np.array_equal(consumed, tables[:1])


@EVERY_BASE
def test_cmp_decrypts(keys):
    """all four signedness pairs over equal operands and operands that differ in the top / in the bottom digit only, both ways.  What the gate sequence stands for
    (src/integer.c:217-265): the unsigned comparison, turned round once for every operand that is marked signed AND negative -- the true order for two signed or
    two unsigned operands"""
    B, d = keys["B"], 2
    m = B ** d
    top, bot = (B - 1) * B, B - 1
    a_v = [0, m - 1, 1, top + 1, 1, 1 + bot - 1, B, m - 1, top]
    b_v = [0, m - 1, top + 1, 1, 1 + bot - 1, 1, m - 1, B, 1][:len(a_v)]
    if B == 2:   # (bot - 1 == 0 would make the bottom-digit pair equal)
        a_v[4], b_v[4], a_v[5], b_v[5] = 0, 1, 1, 0
    a, b = _enc(keys, a_v, d), _enc(keys, b_v, d)
    for sa in (False, True):
        for sb in (False, True):
            want = []
            for x, y in zip(a_v, b_v):
                c = (x > y) - (x < y)
                if sa and x >= m // 2:
                    c = -c
                if sb and y >= m // 2:
                    c = -c
                if sa == sb:
                    vx, vy = (_signed(x, d, B), _signed(y, d, B)) if sa else (x, y)
                    assert c == (vx > vy) - (vx < vy)
                want.append(c + 1)
            _held(keys, "cmp", _run(keys, V.cmp, a, b, sa, sb)[None], want, positions=True)


@EVERY_BASE
def test_lut_cleartext_decrypts(keys):
    """size == B (no tree) and B^2; one output digit and the largest count with out_digits log2 B == 64 (at B = 8: 21 digits, 63 bits); entries that use all 64 bits"""
    B, K = keys["B"], keys["K"]
    rng = np.random.default_rng(11)
    for size, out_digits in ((B, 1), (B * B, 64 // K.logB), (B, 64 // K.logB)) if B == 4 else ((B * B, 64 // K.logB),):
        lut = rng.integers(0, 1 << 64, size, dtype=np.uint64)
        lut[0], lut[size - 1] = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0x8000000000000001)
        levels = 1 if size == B else 2
        sel_v = [0, size - 1, size // 2 + 1]
        out = _run(keys, V.lut_cleartext, _enc(keys, sel_v, levels), lut, out_digits)
        _held(keys, "lut_cleartext", out, [int(lut[v]) % B ** out_digits for v in sel_v])


@BASE_4
def test_sl_add_and_extend_decrypt(keys):
    """c = a B^g + b B^h: the shifts of the device tests, operands of different widths, signed (the low digits of a's width, sign-extended) and unsigned (exact, and cut
    at dc); the extension on its own, signed at d_ini < dc and d_ini == dc, unsigned"""
    B = keys["B"]
    da, db = 2, 1
    a_v, b_v = [B * B - 1, 0, 6, B * B // 2], [B - 1, 0, 3, 1]
    a, b = _enc(keys, a_v, da), _enc(keys, b_v, db)
    for g, h in ((0, 0), (1, 0), (0, 2), (2, 1)):
        natural = max(da + g, db + h) + 1
        for dc in (natural, natural + 1, natural - 1):
            exact = [x * B ** g + y * B ** h for x, y in zip(a_v, b_v)]
            _held(keys, "sl_add", _run(keys, V.sl_add, a, g, b, h, dc, False), [v % B ** dc for v in exact])
        dc = 4
        _held(keys, "sl_add", _run(keys, V.sl_add, a, g, b, h, dc, True), [_signed(v, da, B) % B ** dc for v in exact])
    c = np.concatenate([a, _enc(keys, [5, 6, 7, 1], 2)])          # digits 2, 3 hold something else
    _held(keys, "extend", _run(keys, V.extend, c, 2, True), [_signed(v, 2, B) % B ** 4 for v in a_v])
    _held(keys, "extend", _run(keys, V.extend, c, 2, False), a_v)
    assert np.array_equal(_run(keys, V.extend, c, 4, True), c) and np.array_equal(_run(keys, V.extend, c, 4, False), c)


@BASE_4
def test_sl_addto_decrypts(keys):
    """b += a B^g as the multiplication uses it: unsigned, onto a wider accumulator that already holds a value.  The chain ends at digit da + g (src/integer.c:115): a
    carry out of it is dropped and the digits above keep what they held -- the multiplication's accumulator is still zero there"""
    B = keys["B"]
    a_v, b_v = [B * B - 1, 0, 6], [B ** 4 - 1, 5, B ** 3 + B * B - 1]
    a, b = _enc(keys, a_v, 2), _enc(keys, b_v, 4)
    for g in (0, 1):
        low = B ** min(2 + g + 1, 4)
        _held(keys, "sl_addto", _run(keys, V.sl_addto, b, a, g, False), [y - y % low + (y % low + x * B ** g) % low for x, y in zip(a_v, b_v)])


@EVERY_BASE
def test_mul_decrypts(keys):
    """unsigned: the exact product, operands of different widths, and a result narrower than da + db + 1 (the product mod B^dc); signed: the low digits of a's width,
    sign-extended, as the reference application's test has it (8 x 8 -> 32 bits: the product's low byte)"""
    B = keys["B"]
    m = B * B
    a_v, b_v = [m - 1, 0, m // 2, 3 % m, m - 1], [m - 1, m - 1, m // 2, 2, 1]
    a, b = _enc(keys, a_v, 2), _enc(keys, b_v, 2)
    _held(keys, "mul", _run(keys, V.mul, a, b, 5, False), [x * y for x, y in zip(a_v, b_v)])
    _held(keys, "mul", _run(keys, V.mul, a, b, 4, True), [_signed(x * y, 2, B) % B ** 4 for x, y in zip(a_v, b_v)])
    if B == 4:
        _held(keys, "mul", _run(keys, V.mul, a, b[:1], 4, False), [x * (y % B) for x, y in zip(a_v, b_v)])
        _held(keys, "mul", _run(keys, V.mul, a[:1], b, 4, False), [(x % B) * y for x, y in zip(a_v, b_v)])
        _held(keys, "mul", _run(keys, V.mul, a, b, 3, False), [x * y % B ** 3 for x, y in zip(a_v, b_v)])
