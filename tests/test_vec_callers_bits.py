"""The digit-parallel radix-integer callers (include/mosfhet_hip.h: mosfhet_hip_vec_*; mosfhet_amd/csrc/capi_vec.inc; Engine.vector_ops) held to the CPU oracle's BITS at
every digit base, and mosfhet_hip_tlwe_keyswitch_no_precomp_batch held to exact integers.

Expected words of the callers: tests/vec_reference.py -- the reference application's gate sequences over oracle primitives, one integer and one gate at a time -- which
tests/test_vec_reference.py holds to the arithmetic without a GPU.  Here every output word must equal it (numpy.array_equal) and decrypt.  Keys are generated on the
device and exported for the oracle (a LUT-packing key of this ring takes the oracle's generator tens of seconds): N = 1024, n = 12, l = 2, Bg = 2^8 (the tuned
kernels), key switch and packing switch t = 7, base 2^2 as fixed in tests/test_vec_reference.py, one key set per digit base B in (4, 2, 8), M = 3 integers (M = 1 once
per caller), at most 3 digits.  A decryption test cannot see a constant off by 2^40, a trivial sample that is not exactly trivial, a selector from the wrong tile that
holds the same digit, or stale words of a reused pool slot that land in the noise; a comparison of bits sees each.

The refusals of capi_vec.inc run on a real handle and fake buffers: every one returns before a launch.
"""
import ctypes as C

import numpy as np
import pytest

import vec_reference as V

N, n, l, Bg, T, BB = 1024, 12, 2, 8, 7, 2
EINVAL = -1
ONES = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


EVERY_BASE = pytest.mark.parametrize("keys", [4, 2, 8], indirect=True, ids=lambda B: "B%d" % B)
BASE_4 = pytest.mark.parametrize("keys", [4], indirect=True, ids=lambda B: "B%d" % B)


@pytest.fixture(scope="module")
def keys(request, eng, oracle):
    """One key set per digit base, generated on the device, its rows exported for the oracle; the LWE key-switch key twice, seed-compressed and stored (each call draws
    its own noise: two keys, two sets of rows), one handle and one reference key set on each.  Freed before the next base's."""
    B = request.param
    r = oracle.Rng(0xB175 + B)
    lwe_s, s = oracle.gen_binary_key(r, n), oracle.gen_binary_key(r, N)        # (the extracted key of a k = 1 TRLWE key is the key's coefficients)
    bsk = eng.generate_bootstrap_key(s, lwe_s, l, Bg, 2.0 ** -45, seed=31)
    ksk = {c: eng.generate_keyswitch_key(lwe_s, s, T, BB, 2.0 ** -25, seed=32, compressed=c) for c in (True, False)}
    pksk = eng.generate_lut_packing_key(s, s, T, BB, B, 2.0 ** -45, seed=33)
    cands = (1 << BB) - 1
    pk_rows = eng.export_key_rows(pksk, 0, N * B * T * cands).reshape(N, B, T, cands, 2, N)
    bk_dft = bsk.export_dft()
    K = {c: V.Keys(oracle, bk_dft, l, Bg, eng.export_key_rows(ksk[c], 0, N * T * cands).reshape(N, T, cands, n + 1), BB, pk_rows, BB, B) for c in (True, False)}
    vec = {c: eng.vector_ops(bsk, ksk[c], pksk, B) for c in (True, False)}
    yield {"K": K[True], "K_stored": K[False], "s": s, "r": r, "B": B, "O": oracle, "vec": vec[True], "vec_stored": vec[False], "lwe_s": lwe_s, "bsk": bsk, "ksk": ksk[True], "pksk": pksk}
    for h in (vec[True], vec[False], pksk, ksk[True], ksk[False], bsk):
        h.free()


def _enc(keys, values, d):
    return V.encrypt(keys["O"], keys["r"], values, d, keys["s"], keys["B"], 2.0 ** -30)


def _dev(eng, x):
    import mosfhet_amd as ma
    return ma.to_device(x, eng.device)


def _same(keys, name, got, want, values=None, positions=False):
    """every word of the device's result equals the reference's, and the result decrypts (to `values`: integers, or the raw positions of single digits)"""
    import mosfhet_amd as ma
    got = ma.to_numpy(got) if not isinstance(got, np.ndarray) else got
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = np.nonzero((got != want).reshape(-1, got.shape[-1]).any(axis=1))[0]
    assert np.array_equal(got, want), "%s at B = %d: %d of %d samples differ from the oracle's composition, the first at flat index %d" % (
        name, keys["B"], bad.size, got.size // got.shape[-1], bad[0] if bad.size else -1)
    if values is not None:
        pos, dig, err = V.read(keys["O"], got if got.ndim == 3 else got[None], keys["s"], keys["B"])
        assert err < 0.5, (name, err)
        assert ([int(x) for x in pos.reshape(-1)] if positions else V.to_int(dig, keys["B"])) == [int(v) for v in values], (name, keys["B"])


def _signed(v, d, B):
    m = B ** d
    v %= m
    return v - m if v >= m // 2 else v


# ---------------------------------------------------------------- the callers, bits ----------------------------------------------------------------
@pytest.mark.gpu
@BASE_4
@pytest.mark.parametrize("stored", [False, True], ids=["compressed_ksk", "stored_ksk"])
def test_addsub_bits(eng, keys, stored):
    """add and subtract over d = 3 (M = 3) and d = 1 (M = 1: no next digit to carry into), with the seed-compressed and with the stored LWE key-switch key"""
    B, vec, K = keys["B"], keys["vec_stored" if stored else "vec"], keys["K_stored" if stored else "K"]
    for d, a_v, b_v in ((3, [B ** 3 - 1, 37, B ** 3 // 2], [1, 27, B ** 3 // 2]), (1, [B - 1], [B - 2])):
        m = B ** d
        a, b = _enc(keys, a_v, d), _enc(keys, b_v, d)
        da, db = _dev(eng, a), _dev(eng, b)
        _same(keys, "add d = %d" % d, vec.addsub(da, db), V.addsub(K, a, b), [(x + y) % m for x, y in zip(a_v, b_v)])
        _same(keys, "sub d = %d" % d, vec.addsub(da, db, subtract=True), V.addsub(K, a, b, True), [(x - y) % m for x, y in zip(a_v, b_v)])


@pytest.mark.gpu
@EVERY_BASE
def test_relu_bits(eng, keys):
    """B = 4: d = 3, d = 1 (no lower digit: no packing switch at all) and in place; B = 2 (the non-negative half is ONE slot) and B = 8: d = 2"""
    B, vec = keys["B"], keys["vec"]
    for d in (3, 1) if B == 4 else (2,):
        m = B ** d
        a_v = [m // 2 - 1, m // 2, m - 1] if d > 1 else [B // 2 - 1]
        a = _enc(keys, a_v, d)
        want = V.relu(keys["K"], a)
        _same(keys, "relu d = %d" % d, vec.relu(_dev(eng, a)), want, [v if v < m // 2 else 0 for v in a_v])
        da = _dev(eng, a)
        assert vec.relu(da, out=da) is da
        _same(keys, "relu in place d = %d" % d, da, want)


@pytest.mark.gpu
@BASE_4
def test_encrypted_lut_and_mux_array_bits(eng, keys):
    """the tree at size == B (one level) and B^2 (two): the selected entries AND the whole consumed table; the array form at size == 1 (no level: a bare copy, no
    selector read) and at size == B^2 over d = 2 digits (one tree over d M instances)"""
    import torch
    import mosfhet_amd as ma
    B, vec, K = keys["B"], keys["vec"], keys["K"]
    rng = np.random.default_rng(7)
    for size, M in ((B, 1), (B * B, 3)):
        levels = 1 if size == B else 2
        table_v = rng.integers(0, B, (size, M))
        sel_v = [size - 1, 0, size // 2 + 1][:M]
        table, sel = np.stack([_enc(keys, table_v[j], 1)[0] for j in range(size)]), _enc(keys, sel_v, levels)
        want, consumed = V.encrypted_lut(K, table, sel)
        d_table = _dev(eng, table)
        out = vec.encrypted_lut(d_table, _dev(eng, sel))
        _same(keys, "encrypted_lut size = %d" % size, out, want, None)
        _same(keys, "encrypted_lut size = %d, consumed table" % size, d_table, consumed)
        _same(keys, "encrypted_lut size = %d" % size, ma.to_numpy(out)[None], want[None], [table_v[sel_v[m], m] for m in range(M)])
    size, d, M = B * B, 2, 3
    vec_v = rng.integers(0, B ** d, (size, M))
    sel_v = [size - 1, 0, 6]
    tables, sel = np.stack([_enc(keys, vec_v[j], d) for j in range(size)]), _enc(keys, sel_v, 2)
    want, consumed = V.mux_array(K, tables, sel)
    d_tables = _dev(eng, tables)
    _same(keys, "mux_array", vec.mux_array(d_tables, _dev(eng, sel)), want, [vec_v[sel_v[m], m] for m in range(M)])
    _same(keys, "mux_array, consumed tables", d_tables, consumed)
    for M in (3, 1):
        one = _dev(eng, tables[:1, :, :M])
        out = vec.mux_array(one, torch.empty(0, M, N + 1, dtype=torch.int64, device=eng.device))
        _same(keys, "mux_array size = 1", out, np.ascontiguousarray(tables[0, :, :M]), vec_v[0, :M])
        _same(keys, "mux_array size = 1, table", one, np.ascontiguousarray(tables[:1, :, :M]))


@pytest.mark.gpu
@EVERY_BASE
def test_cmp_bits(eng, keys):
    """all four signedness pairs (the sign steps read the operands' top digits with slots [c .. c, -c .. -c]) over equal operands, operands that differ in the top digit
    only and in the bottom digit only; once more at M = 1.  At B = 4 with the seed-compressed and with the stored LWE key-switch key."""
    B, d, K = keys["B"], 2, keys["K"]
    m = B ** d
    a_v, b_v = [m - 1, 1, B + (B - 1)], [m - 1, (B - 1) * B + 1, B]
    a, b = _enc(keys, a_v, d), _enc(keys, b_v, d)
    da, db = _dev(eng, a), _dev(eng, b)
    for sa in (False, True):
        for sb in (False, True):
            want_v = []
            for x, y in zip(a_v, b_v):
                c = (x > y) - (x < y)
                c = -c if sa and x >= m // 2 else c
                c = -c if sb and y >= m // 2 else c
                want_v.append(c + 1)
            want = V.cmp(K, a, b, sa, sb)
            _same(keys, "cmp %s %s" % (sa, sb), keys["vec"].cmp(da, db, sa, sb), want, want_v, positions=True)
            if B == 4:
                _same(keys, "cmp %s %s, stored key" % (sa, sb), keys["vec_stored"].cmp(da, db, sa, sb), V.cmp(keys["K_stored"], a, b, sa, sb), want_v, positions=True)
    _same(keys, "cmp M = 1", keys["vec"].cmp(da[:, 1:2].contiguous(), db[:, 1:2].contiguous(), True, False), V.cmp(K, a[:, 1:2], b[:, 1:2], True, False), [0], positions=True)


@pytest.mark.gpu
@EVERY_BASE
def test_lut_cleartext_bits(eng, keys):
    """B = 4: size == B (no tree is run) and B^2, one output digit and the largest count (32 digits of 2 bits: shifts up to 62, at M = 1), a table whose entries use all 64
    bits; B = 2 and B = 8: size == B^2, two output digits"""
    B, vec, K = keys["B"], keys["vec"], keys["K"]
    rng = np.random.default_rng(11)
    for size, out_digits, M in ((B, 1, 3), (B * B, 64 // K.logB, 1), (B, 3, 1), (B * B, 2, 3)) if B == 4 else ((B * B, 2, 3),):
        lut = rng.integers(0, 1 << 64, size, dtype=np.uint64)
        lut[0], lut[size - 1] = np.uint64(ONES), np.uint64(0x8000000000000001)
        levels = 1 if size == B else 2
        sel_v = [size - 1, 0, size // 2 + 1][:M]
        sel = _enc(keys, sel_v, levels)
        before = lut.copy()
        got = vec.lut_cleartext(_dev(eng, sel), lut, out_digits)
        assert np.array_equal(lut, before)
        _same(keys, "lut_cleartext size = %d, %d digits" % (size, out_digits), got, V.lut_cleartext(K, sel, lut, out_digits), [int(lut[v]) % B ** out_digits for v in sel_v])


@pytest.mark.gpu
@BASE_4
def test_sl_add_bits(eng, keys):
    """c = a B^g + b B^h with da = 2, db = 1 over the shifts (0, 0), (1, 0), (0, 2), (2, 1): unsigned into the natural width max(da + g, db + h) + 1 and one digit more
    (the zero extension), signed into 4 digits (a's width, then the sign extension); (0, 0) once more at M = 1"""
    B, vec, K = keys["B"], keys["vec"], keys["K"]
    da_, db_ = 2, 1
    a_v, b_v = [B * B - 1, 6, B * B // 2], [B - 1, 3, 1]
    a, b = _enc(keys, a_v, da_), _enc(keys, b_v, db_)
    da, db = _dev(eng, a), _dev(eng, b)
    for g, h in ((0, 0), (1, 0), (0, 2), (2, 1)):
        exact = [x * B ** g + y * B ** h for x, y in zip(a_v, b_v)]
        natural = max(da_ + g, db_ + h) + 1
        for dc in (natural, natural + 1):
            _same(keys, "sl_add unsigned %s dc = %d" % ((g, h), dc), vec.sl_add(da, g, db, h, dc, signed=False), V.sl_add(K, a, g, b, h, dc, False), exact)
        _same(keys, "sl_add signed %s" % ((g, h),), vec.sl_add(da, g, db, h, 4, signed=True), V.sl_add(K, a, g, b, h, 4, True), [_signed(v, da_, B) % B ** 4 for v in exact])
    _same(keys, "sl_add M = 1", vec.sl_add(da[:, :1].contiguous(), 0, db[:, :1].contiguous(), 0, 3, signed=False), V.sl_add(K, a[:, :1], 0, b[:, :1], 0, 3, False), [a_v[0] + b_v[0]])


@pytest.mark.gpu
@BASE_4
def test_extend_bits(eng, keys):
    """signed with d_ini < dc (one bootstrap, dc - d_ini extractions, strided into the digit planes), signed with d_ini == dc (the buffer is not touched), unsigned
    (trivial zeros); the digits above d_ini hold other samples before the call"""
    B, vec, K = keys["B"], keys["vec"], keys["K"]
    a_v = [B * B - 1, 6, B * B // 2]
    c = np.concatenate([_enc(keys, a_v, 2), _enc(keys, [5, 6, 7], 2)])
    _same(keys, "extend signed", vec.extend(_dev(eng, c), 2, signed=True), V.extend(K, c, 2, True), [_signed(v, 2, B) % B ** 4 for v in a_v])
    _same(keys, "extend signed, d_ini == dc", vec.extend(_dev(eng, c), 4, signed=True), c)
    _same(keys, "extend unsigned", vec.extend(_dev(eng, c), 2, signed=False), V.extend(K, c, 2, False), a_v)
    _same(keys, "extend signed M = 1", vec.extend(_dev(eng, c[:, :1]), 1, signed=True), V.extend(K, c[:, :1], 1, True), None)


@pytest.mark.gpu
@EVERY_BASE
def test_mul_bits(eng, keys):
    """d = 2 x 2 digits, unsigned into 5 digits (the exact product) and signed into 4 (a's width, sign-extended): at B = 2 the loop over the multi-value tables is empty and
    the table slots are [0, a_i] / [0, 0]; B = 4 also: operands of different widths both ways, a result narrower than da + db + 1, and M = 1"""
    B, vec, K = keys["B"], keys["vec"], keys["K"]
    m = B * B
    a_v, b_v = [m - 1, m // 2, 3 % m], [m - 1, m // 2 + 1, 2]
    a, b = _enc(keys, a_v, 2), _enc(keys, b_v, 2)
    da, db = _dev(eng, a), _dev(eng, b)
    _same(keys, "mul unsigned", vec.mul(da, db, 5, signed=False), V.mul(K, a, b, 5, False), [x * y for x, y in zip(a_v, b_v)])
    _same(keys, "mul signed", vec.mul(da, db, 4, signed=True), V.mul(K, a, b, 4, True), [_signed(x * y, 2, B) % B ** 4 for x, y in zip(a_v, b_v)])
    if B == 4:
        _same(keys, "mul da > db", vec.mul(da, db[:1].contiguous(), 4, signed=False), V.mul(K, a, b[:1], 4, False), [x * (y % B) for x, y in zip(a_v, b_v)])
        _same(keys, "mul da < db", vec.mul(da[:1].contiguous(), db, 4, signed=False), V.mul(K, a[:1], b, 4, False), [(x % B) * y for x, y in zip(a_v, b_v)])
        _same(keys, "mul narrow result", vec.mul(da, db, 3, signed=False), V.mul(K, a, b, 3, False), [x * y % B ** 3 for x, y in zip(a_v, b_v)])
        _same(keys, "mul M = 1", vec.mul(da[:, :1].contiguous(), db[:, :1].contiguous(), 5, signed=False), V.mul(K, a[:, :1], b[:, :1], 5, False), [a_v[0] * b_v[0]])


@pytest.mark.gpu
@BASE_4
def test_same_bits_on_a_second_stream(eng, keys):
    """ReLU on a non-default stream of the engine right behind a comparison on the default stream: both take the thread's POOL_VEC slot, the comparison leaves its
    differences, selectors, slots and test vectors there.  The side stream waits for the default one (a pool slot serves one stream at a time) and nothing else
    synchronises: a kernel or copy of the call queued anywhere but on the given stream, or a word read before it is written, changes the bits."""
    import torch
    B, vec, K = keys["B"], keys["vec"], keys["K"]
    m = B ** 3
    a_v, b_v = [m // 2 - 1, m // 2, m - 1], [1, m - 1, 5]
    a, b = _enc(keys, a_v, 3), _enc(keys, b_v, 3)
    da, db = _dev(eng, a), _dev(eng, b)
    want = V.relu(K, a)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=eng.device)
    c = vec.cmp(da, db, True, True)
    side.wait_stream(torch.cuda.current_stream(eng.device))
    with torch.cuda.stream(side):
        assert eng._stream().value == side.cuda_stream
        out = vec.relu(da)
    side.synchronize()
    torch.cuda.synchronize()
    _same(keys, "relu on a second stream", out, want, [v if v < m // 2 else 0 for v in a_v])
    _same(keys, "cmp before it", c, V.cmp(K, a, b, True, True))


# ---------------------------------------------------------------- refusals ----------------------------------------------------------------
@pytest.mark.gpu
@BASE_4
def test_refusals_of_the_vector_callers(eng, keys, native_lib):
    """Every fail(...) of the nine entry points of capi_vec.inc and of vec_create: MOSFHET_HIP_EINVAL and the message, on a real handle and fake non-null buffers (no
    refusal comes after a launch); M == 0 returns OK with null buffers."""
    lib = native_lib
    err = lambda: lib.mosfhet_hip_last_error().decode()
    P, I = C.c_void_p, C.c_int
    fake, fake2 = P(8), P(16)
    v, bsk, ksk, pksk, B = keys["vec"].h, keys["bsk"], keys["ksk"], keys["pksk"], keys["B"]
    big = 65536

    def refused(rc, fragment):
        assert rc == EINVAL and fragment in err(), (rc, err(), fragment)

    create = lib.mosfhet_hip_vec_create
    create.argtypes = [P, P, P, P, P, I]
    out = P()
    refused(create(None, C.byref(out), bsk.h, ksk.h, pksk.h, B), "vec_create: bad argument")
    refused(create(eng.h, None, bsk.h, ksk.h, pksk.h, B), "vec_create: bad argument")
    refused(create(eng.h, C.byref(out), None, ksk.h, pksk.h, B), "vec_create: bad argument")
    refused(create(eng.h, C.byref(out), bsk.h, None, pksk.h, B), "vec_create: bad argument")
    for tb in (0, 1, 3, 6, 2 * N):
        refused(create(eng.h, C.byref(out), bsk.h, ksk.h, pksk.h, tb), "torus_base %d must be a power of two dividing N / 2" % tb)
    refused(create(eng.h, C.byref(out), bsk.h, pksk.h, pksk.h, B), "ksk must be the LWE key switch N -> n")
    refused(create(eng.h, C.byref(out), bsk.h, ksk.h, ksk.h, B), "pksk must be the LUT-packing key of %d slots" % B)
    refused(create(eng.h, C.byref(out), bsk.h, ksk.h, pksk.h, 2 * B), "pksk must be the LUT-packing key of %d slots" % (2 * B))
    general = eng.generate_bootstrap_key(np.stack([keys["s"], keys["s"]]), keys["lwe_s"], l, Bg, 2.0 ** -45, seed=34)       # k = 2: the general-ring path
    refused(create(eng.h, C.byref(out), general.h, ksk.h, pksk.h, B), "vec_create: keys of the general-ring path")
    general.free()
    assert out.value is None
    no_pk = eng.vector_ops(bsk, ksk, None, B)          # add / sub only

    f = lib.mosfhet_hip_vec_addsub
    f.argtypes = [P, P, P, P, I, I, I, P]
    refused(f(None, fake, fake, fake, 1, 1, 0, None), "vec_addsub: bad argument")
    refused(f(v, fake, fake, fake, -1, 1, 0, None), "vec_addsub: bad argument")
    refused(f(v, fake, fake, fake, 1, 0, 0, None), "vec_addsub: bad argument")
    assert f(v, None, None, None, 0, 1, 0, None) == 0
    for args in ((None, fake, fake), (fake2, None, fake), (fake2, fake, None), (fake, fake, fake2), (fake, fake2, fake)):
        refused(f(v, *args, 1, 1, 0, None), "vec_addsub: null or aliased buffer")
    refused(f(v, fake2, fake, fake, big, 1, 0, None), "vec_addsub: M = 65536")

    f = lib.mosfhet_hip_vec_relu
    f.argtypes = [P, P, P, I, I, P]
    refused(f(None, fake, fake, 1, 1, None), "vec_relu: bad argument")
    refused(f(v, fake, fake, -1, 1, None), "vec_relu: bad argument")
    refused(f(v, fake, fake, 1, 0, None), "vec_relu: bad argument")
    refused(f(no_pk.h, fake, fake, 1, 1, None), "vec_relu: the handle has no LUT-packing key")
    assert f(v, None, None, 0, 1, None) == 0
    refused(f(v, None, fake, 1, 1, None), "vec_relu: null buffer")
    refused(f(v, fake, None, 1, 1, None), "vec_relu: null buffer")
    refused(f(v, fake, fake, big, 1, None), "vec_relu: batch too large")
    refused(f(v, fake, fake, 65535, 2 ** 31 // (65535 * B) + 2, None), "vec_relu: batch too large")

    f = lib.mosfhet_hip_vec_encrypted_lut
    f.argtypes = [P, P, P, I, I, P]
    refused(f(None, fake, fake, B, 1, None), "vec_encrypted_lut: bad argument")
    refused(f(v, fake, fake, B, -1, None), "vec_encrypted_lut: bad argument")
    refused(f(v, fake, fake, 0, 1, None), "vec_encrypted_lut: bad argument")
    refused(f(no_pk.h, fake, fake, B, 1, None), "vec_encrypted_lut: the handle has no LUT-packing key")
    for size in (B + 1, 3 * B, 2 * B * B):
        refused(f(v, fake, fake, size, 1, None), "vec_encrypted_lut: size %d is not a power of torus_base %d" % (size, B))
    assert f(v, None, None, B, 0, None) == 0 and f(v, None, None, 1, 5, None) == 0       # nothing to do: no instance, or no level
    refused(f(v, None, fake, B, 1, None), "vec_encrypted_lut: null buffer")
    refused(f(v, fake, None, B, 1, None), "vec_encrypted_lut: null buffer")
    refused(f(v, fake, fake, B ** 8, 2 ** 31 // B ** 8 + 1, None), "vec_encrypted_lut: too many units")

    f = lib.mosfhet_hip_vec_mux_array
    f.argtypes = [P, P, P, P, I, I, I, P]
    refused(f(None, fake, fake, fake, B, 1, 1, None), "vec_mux_array: bad argument")
    refused(f(v, fake, fake, fake, B, 1, -1, None), "vec_mux_array: bad argument")
    refused(f(v, fake, fake, fake, 0, 1, 1, None), "vec_mux_array: bad argument")
    refused(f(v, fake, fake, fake, B, 0, 1, None), "vec_mux_array: bad argument")
    refused(f(v, fake, fake, fake, B + 1, 1, 1, None), "vec_mux_array: size %d is not a power of torus_base %d" % (B + 1, B))
    assert f(v, None, None, None, B, 1, 0, None) == 0
    refused(f(v, None, fake, fake, B, 1, 1, None), "vec_mux_array: null buffer")
    refused(f(v, fake, None, fake, B, 1, 1, None), "vec_mux_array: null buffer")
    refused(f(v, fake, fake, None, B, 1, 1, None), "vec_mux_array: null buffer")
    refused(f(v, fake, fake, fake, B ** 8, 2 ** 15, 2 ** 15, None), "vec_mux_array: too many units")

    f = lib.mosfhet_hip_vec_cmp
    f.argtypes = [P, P, P, P, I, I, I, I, P]
    refused(f(None, fake, fake, fake, 1, 1, 0, 0, None), "vec_cmp: bad argument")
    refused(f(v, fake, fake, fake, -1, 1, 0, 0, None), "vec_cmp: bad argument")
    refused(f(v, fake, fake, fake, 1, 0, 0, 0, None), "vec_cmp: bad argument")
    refused(f(no_pk.h, fake2, fake, fake, 1, 1, 0, 0, None), "vec_cmp: the handle has no LUT-packing key")
    assert f(v, None, None, None, 0, 1, 0, 0, None) == 0
    for args in ((None, fake, fake), (fake2, None, fake), (fake2, fake, None)):
        refused(f(v, *args, 1, 1, 0, 0, None), "vec_cmp: null buffer")
    refused(f(v, fake, fake, fake2, 1, 1, 0, 0, None), "vec_cmp: the result must not alias an operand")
    refused(f(v, fake, fake2, fake, 1, 1, 0, 0, None), "vec_cmp: the result must not alias an operand")
    refused(f(v, fake2, fake, fake, big, 1, 0, 0, None), "vec_cmp: M = 65536")

    f = lib.mosfhet_hip_vec_lut_cleartext
    f.argtypes = [P, P, P, P, I, I, I, P]
    lut = (C.c_uint64 * (B * B))()
    refused(f(None, fake, fake, lut, B, 1, 1, None), "vec_lut_cleartext: bad argument")
    refused(f(v, fake, fake, None, B, 1, 1, None), "vec_lut_cleartext: bad argument")
    refused(f(v, fake, fake, lut, B, 1, -1, None), "vec_lut_cleartext: bad argument")
    refused(f(v, fake, fake, lut, 0, 1, 1, None), "vec_lut_cleartext: bad argument")
    refused(f(v, fake, fake, lut, B, 0, 1, None), "vec_lut_cleartext: bad argument")
    refused(f(no_pk.h, fake, fake, lut, B, 1, 1, None), "vec_lut_cleartext: the handle has no LUT-packing key")
    refused(f(v, fake, fake, lut, B - 1, 1, 1, None), "vec_lut_cleartext: the table needs at least torus_base entries")
    refused(f(v, fake, fake, lut, B, 64 // keys["K"].logB + 1, 1, None), "digits of %d bits do not fit the 64-bit table entries" % keys["K"].logB)
    refused(f(v, fake, fake, lut, 2 * B, 1, 1, None), "vec_lut_cleartext: size %d is not a power of torus_base %d" % (2 * B, B))
    refused(f(v, fake, fake, lut, B ** 15, 1, 2 ** 31 // B ** 14 + 1, None), "vec_lut_cleartext: too many units")
    assert f(v, None, None, lut, B, 1, 0, None) == 0
    refused(f(v, None, fake, lut, B, 1, 1, None), "vec_lut_cleartext: null buffer")
    refused(f(v, fake, None, lut, B, 1, 1, None), "vec_lut_cleartext: null buffer")

    f = lib.mosfhet_hip_vec_sl_add
    f.argtypes = [P, P, I, P, I, I, P, I, I, I, I, P]
    refused(f(None, fake2, 2, fake, 1, 0, fake, 1, 0, 0, 1, None), "vec_sl_add: bad argument")
    for dc, da_, g, db_, h, M in ((2, 1, 0, 1, 0, -1), (2, 0, 0, 1, 0, 1), (2, 1, 0, 0, 0, 1), (0, 1, 0, 1, 0, 1), (2, 1, -1, 1, 0, 1), (2, 1, 0, 1, -1, 1)):
        refused(f(v, fake2, dc, fake, da_, g, fake, db_, h, 0, M, None), "vec_sl_add: bad argument")
    assert f(v, None, 2, None, 1, 0, None, 1, 0, 0, 0, None) == 0
    for c_, a_, b_ in ((None, fake, fake), (fake2, None, fake), (fake2, fake, None), (fake, fake, fake2), (fake, fake2, fake)):
        refused(f(v, c_, 2, a_, 1, 0, b_, 1, 0, 0, 1, None), "vec_sl_add: null or aliased buffer")
    refused(f(v, fake2, 2, fake, 3, 0, fake, 1, 0, 1, 1, None), "vec_sl_add: the result has fewer digits than the signed operand a")
    refused(f(v, fake2, 2, fake, 1, 0, fake, 1, 0, 0, big, None), "vec_sl_add: M = 65536")

    f = lib.mosfhet_hip_vec_extend
    f.argtypes = [P, P, I, I, I, I, P]
    refused(f(None, fake, 2, 1, 1, 1, None), "vec_extend: bad argument")
    for dc, d_ini, sg, M in ((2, 1, 1, -1), (0, 0, 0, 1), (2, 0, 1, 1), (2, -1, 0, 1), (2, 3, 0, 1)):
        refused(f(v, fake, dc, d_ini, sg, M, None), "vec_extend: bad argument")
    assert f(v, None, 2, 1, 1, 0, None) == 0
    refused(f(v, None, 2, 1, 1, 1, None), "vec_extend: null buffer")
    refused(f(v, fake, 2, 1, 1, big, None), "vec_extend: M = 65536")

    f = lib.mosfhet_hip_vec_mul
    f.argtypes = [P, P, I, P, I, P, I, I, I, P]
    refused(f(None, fake2, 2, fake, 1, fake, 1, 0, 1, None), "vec_mul: bad argument")
    for dc, da_, db_, M in ((2, 1, 1, -1), (2, 0, 1, 1), (2, 1, 0, 1), (0, 1, 1, 1)):
        refused(f(v, fake2, dc, fake, da_, fake, db_, 0, M, None), "vec_mul: bad argument")
    refused(f(no_pk.h, fake2, 2, fake, 1, fake, 1, 0, 1, None), "vec_mul: the handle has no LUT-packing key")
    refused(f(v, fake2, 2, fake, 3, fake, 1, 1, 1, None), "vec_mul: the result has fewer digits than a signed operand")
    refused(f(v, fake2, 2, fake, 1, fake, 3, 1, 1, None), "vec_mul: the result has fewer digits than a signed operand")
    assert f(v, None, 2, None, 1, None, 1, 0, 0, None) == 0
    for c_, a_, b_ in ((None, fake, fake), (fake2, None, fake), (fake2, fake, None), (fake, fake, fake2), (fake, fake2, fake)):
        refused(f(v, c_, 2, a_, 1, b_, 1, 0, 1, None), "vec_mul: null or aliased buffer")
    refused(f(v, fake2, 2, fake, 1, fake, 1, 0, big, None), "vec_mul: batch too large (M <= 65535")
    no_pk.free()


# ---------------------------------------------------------------- tlwe_keyswitch_no_precomp ----------------------------------------------------------------
def _no_precomp_expected(rows, cts, t, bb):
    """out = (0, .., 0, b) - sum_{i, j} digit_ij KS[i][j] mod 2^64, the digits cut from a_i + 2 * 2^(63 - t bb) (src/tlwe.c:305-320 adds the offset twice);
    rows [n_in][t][n_out + 1], cts [count][n_in + 1]"""
    n_in, _, row = rows.shape
    a = cts[:, :n_in] + np.uint64(2 << (63 - t * bb))
    digits = np.stack([(a >> np.uint64(64 - (j + 1) * bb)) & np.uint64((1 << bb) - 1) for j in range(t)], axis=2)          # [count][n_in][t]
    out = np.uint64(0) - digits.reshape(len(cts), n_in * t) @ rows.reshape(n_in * t, row)
    out[:, row - 1] += cts[:, n_in]
    return out


def _no_precomp(eng, native_lib, d_rows, d_out, d_in, count, n_in, n_out, t, bb):
    f = native_lib.mosfhet_hip_tlwe_keyswitch_no_precomp_batch
    f.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p]
    ptr = lambda x: x if x is None or isinstance(x, C.c_void_p) else C.c_void_p(x.data_ptr())
    return f(eng.h, ptr(d_rows), ptr(d_out), ptr(d_in), count, n_in, n_out, t, bb, eng._stream())


@pytest.mark.gpu
@pytest.mark.parametrize("t,bb", [(8, 2), (1, 1), (3, 16), (31, 2)], ids=lambda x: str(x))
def test_keyswitch_no_precomp_exact(eng, native_lib, t, bb):
    """mosfhet_hip_tlwe_keyswitch_no_precomp_batch (tlwe_keyswitch_scaled_kernel + the shared reduce kernel) against exact integers, every word: count in (1, 2, 17,
    300) -- both sides of where the split of the input words collapses to one -- n_in in (3, 8, 37) (n_in / 4 == 0; an uneven last split), n_out + 1 in (2, 256, 257,
    600) (one slice, a full one, one word into the second, three), digits of 1, 2 and 16 bits and t bb == 62.  The key is random words (the arithmetic is exact mod
    2^64); the inputs are random words with, sprinkled over rows and positions: zero, all ones, the first and last word whose digits are all zero after the doubled
    rounding offset (it carries out of the top digit) and their neighbours; and, at count <= 2, whole inputs of zeros and of ones."""
    import torch
    import mosfhet_amd as ma
    rng = np.random.default_rng(1000 * t + bb)
    edge = (1 << 64) - (1 << (64 - t * bb))                    # a + 2^(64 - t bb) wraps from here on: every digit is zero
    special = [0, ONES, edge, edge - 1, (edge + 1) & ONES, (1 << (64 - t * bb)) - 1, 1 << 63, (1 << 63) - (1 << (64 - t * bb))]
    widths = (2, 256, 257, 600)
    for ci, count in enumerate((1, 2, 17, 300)):
        for ni, n_in in enumerate((3, 8, 37)):
            for row in sorted({widths[(ci + ni) % 4], widths[(ci + 2 * ni + 1) % 4]} | (set(widths) if (count, n_in) == (17, 37) else set())):
                rows = rng.integers(0, 1 << 64, (n_in, t, row), dtype=np.uint64)
                kinds = ["sprinkled"] + (["zeros", "ones"] if count <= 2 else [])
                for kind in kinds:
                    cts = rng.integers(0, 1 << 64, (count, n_in + 1), dtype=np.uint64)
                    if kind == "sprinkled":
                        flat = cts.reshape(-1)
                        flat[::3] = np.array(special, dtype=np.uint64)[np.arange(flat[::3].size) % len(special)]
                    else:
                        cts[:] = np.uint64(0 if kind == "zeros" else ONES)
                    d_out = torch.full((count + 1, row), 0x5A5A5A5A, dtype=torch.int64, device=eng.device)      # one row more: it must stay as it is
                    assert _no_precomp(eng, native_lib, ma.to_device(rows, eng.device), d_out, ma.to_device(cts, eng.device), count, n_in, row - 1, t, bb) == 0
                    got = ma.to_numpy(d_out)
                    assert np.array_equal(got[:count], _no_precomp_expected(rows, cts, t, bb)), (count, n_in, row, kind)
                    assert (got[count] == 0x5A5A5A5A).all(), (count, n_in, row, kind)


@pytest.mark.gpu
def test_keyswitch_no_precomp_refusals(eng, native_lib):
    """count beyond 65535 (the batch index is gridDim.z of one kernel and gridDim.y of the other) is refused before any device call, as the vector callers refuse M;
    so are the scalar arguments out of range and null buffers; count == 0 returns OK with null buffers"""
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)
    call = lambda count=1, n_in=8, n_out=8, t=2, bb=2, bufs=(fake, fake, fake): _no_precomp(eng, native_lib, bufs[0], bufs[1], bufs[2], count, n_in, n_out, t, bb)
    assert call(count=65536) == EINVAL and "count = 65536" in err() and "65535" in err()
    assert call(count=2 ** 31 - 1) == EINVAL and "count = 2147483647" in err()
    for kw in ({"count": -1}, {"n_in": 0}, {"n_out": 0}, {"t": 0}, {"bb": 0}, {"bb": 17}, {"t": 21, "bb": 3}, {"t": 63, "bb": 1}):
        assert call(**kw) == EINVAL and "keyswitch_no_precomp: bad argument" in err(), kw
    for bufs in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert call(bufs=bufs) == EINVAL and "keyswitch_no_precomp: null buffer" in err()
    assert call(count=0, bufs=(None, None, None)) == 0
