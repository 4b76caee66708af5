"""The client half on the device: encrypting and opening sample batches under a secret-key handle (include/mosfhet_hip.h: mosfhet_hip_client_key_create,
mosfhet_hip_tlwe_encrypt_batch, _trlwe_, _trgsw_, mosfhet_hip_tlwe_phase_batch, _trlwe_, mosfhet_hip_trgsw_encrypt_plan; mosfhet_amd/csrc/capi_client.inc,
client_kernels.h).

Expected words come from tests/client_reference.py, the contract restated on tests/keygen_reference.py.  The encrypt calls are deterministic once the keygen secret is
installed, so every word is compared: masks ==, and the noise term recovered exactly as b - a * s - message (mod 2^64) within keygen_reference.noise_tolerance
(1 + sigma 2^64 2^-40: the truncation and the device's double evaluation of cos, log and sqrt; a wrong stream misses by about sigma 2^64).  Phases are == the oracle.
The decryption bound of the selector test is test_trgsw_from_gadget's 2^57 (half a slot of four-bit messages less two bits)."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import client_reference as ref
import keygen_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
U64 = np.uint64
M64 = R.M64
SECRET = bytes(range(32))
KEY = R.key_words(SECRET)
BOUND = 2.0 ** 57


def _u64(x):
    return np.asarray([int(v) & M64 for v in (x if isinstance(x, (list, tuple)) else np.atleast_1d(x))], dtype=U64)   # (a list of Python ints stays exact)


def _binary_key(rng, n):
    s = rng.integers(0, 2, size=n).astype(U64)
    s[0] = 1
    return s


def _small_key(rng, n):
    """small integers with negative coefficients (and zeros): the multiply path"""
    s = rng.integers(-3, 4, size=n).astype(np.int64)
    s[0] = -2
    if n > 2:
        s[1], s[n - 1] = 3, -1
    return s.astype(U64)


def _corner_key(N, which):
    """weight 0, only s[N - 1] set, all ones"""
    s = np.zeros(N, dtype=U64)
    if which == "last":
        s[N - 1] = 1
    elif which == "ones":
        s[:] = 1
    return s


def _noise_off(e, nonce, row, sigma, exact_words=64):
    """|e - the noise terms of (KEY, nonce, row)| per word, as floats"""
    want = R.noise_row(KEY, nonce, row, e.size, sigma, exact_words)
    return np.abs((np.asarray(e, dtype=U64).view(np.int64) - want).astype(np.float64))


def _check_noise(e, nonce, row, sigma, what):
    off = _noise_off(e, nonce, row, sigma)
    bad = np.flatnonzero(off > R.noise_tolerance(sigma))
    assert bad.size == 0, "%s row %d: %d of %d noise terms off, first at x = %d by %g (tolerance %.1f)" % (what, row, bad.size, e.size, bad[0], off[bad[0]],
                                                                                                          R.noise_tolerance(sigma))


def _mismatch(e, nonce, row, sigma):
    """median |e - noise of another stream| / (sigma 2^64): about 1 for an independent stream, below 2^-40 for the same one"""
    return float(np.median(_noise_off(e, nonce, row, sigma, exact_words=0))) / (sigma * 2.0 ** 64)


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_reference_against_the_oracle(oracle):
    """The reference itself; the code under test plays no part.  Its product is oracle.poly_naive_mul (binary, small and corner keys); its TRLWE sample has
    oracle.trlwe_phase = msg + its noise terms, word for word; its TLWE sample has oracle.tlwe_phase = msg + the noise term of coefficient 0; mask words are words 4 - 5 of
    the block whose words 0 - 3 the noise reads; decode against hand-worked words."""
    rng = np.random.default_rng(0xC11E)
    N, sigma, nonce = 256, 2.0 ** -15, R.call_nonce(3, ref.KIND_TRLWE)
    for s in (_binary_key(rng, N), _small_key(rng, N), _corner_key(N, "zero"), _corner_key(N, "last"), _corner_key(N, "ones")):
        a = rng.integers(0, 2 ** 64, size=N, dtype=U64)
        assert (ref.negacyclic_mul(a, s) == oracle.poly_naive_mul(a.copy(), s)).all()
        msg = rng.integers(0, 2 ** 64, size=N, dtype=U64)
        c = ref.trlwe_sample(KEY, nonce, 5, s, msg, sigma)
        assert (oracle.trlwe_phase(np.ascontiguousarray(c), s.reshape(1, N)) == msg + ref.noise_words(KEY, nonce, 5, N, sigma)).all()
        assert (ref.trlwe_phase(c, s) == oracle.trlwe_phase(np.ascontiguousarray(c), s.reshape(1, N))).all()
    s = _small_key(rng, 70)
    c = ref.tlwe_sample(KEY, R.call_nonce(1, ref.KIND_TLWE), 9, s, 0x1234 << 40, sigma)
    want = (int(ref.noise_words(KEY, R.call_nonce(1, ref.KIND_TLWE), 9, 1, sigma)[0]) + (0x1234 << 40)) & M64
    assert oracle.tlwe_phase(c, s) == want == int(ref.tlwe_phase(c, s))
    blk = R.chacha20_block(KEY, (5 << 16) | 7, nonce)
    assert int(ref.mask_row(KEY, nonce, 5, 8)[7]) == blk[4] | (blk[5] << 32)
    assert R.call_nonce(2, ref.KIND_TRGSW) == 0x208
    assert list(ref.decode(_u64([0, 1 << 59, (1 << 59) - 1, 15 << 60, (31 << 59), M64]), 4)) == [0, 1, 0, 15, 0, 0]
    assert list(ref.decode(_u64([1 << 62, (1 << 62) - 1, 3 << 62]), 1)) == [1, 0, 0]
    assert list(ref.decode(_u64([5, M64]), 63)) == [3, 0] and list(ref.decode(_u64([5, M64]), 0)) == [5, M64]
    g = ref.gadget_rows(256, -1, 256 + 3, 2, 8)
    assert int(g[0, 0, 3]) == 1 << 56 and int(g[3, 1, 3]) == 1 << 48 and np.count_nonzero(g) == 4         # -1 X^(N + 3) = + X^3
    assert int(ref.gadget_rows(256, 3, -3, 2, 8)[1, 0, 253]) == (-3 << 48) & M64                          # X^-3 = -X^(N - 3)


def test_reference_trgsw_selects(oracle):
    """The reference's TRGSW samples of 0 and 1 at (1024, 2, 8), sigma 2^-25, select under oracle.external_product: the product with a sample of four-bit messages opens to
    bit x message within test_trgsw_from_gadget's 2^57.  X^exp rotates: the sample of 1 X^(N + 2) gives -X^2 message."""
    N, l, Bg, sigma = 1024, 2, 8, 2.0 ** -25
    oracle.plan(N)
    rng = np.random.default_rng(0x7265)
    s = _binary_key(rng, N)
    msg = rng.integers(0, 16, size=N).astype(U64) << U64(60)
    probe = ref.trlwe_sample(KEY, R.call_nonce(1, ref.KIND_TRLWE), 0, s, msg, sigma, oracle.poly_naive_mul)
    nonce = R.call_nonce(2, ref.KIND_TRGSW)
    for u, (m, e) in enumerate(((0, 0), (1, 0), (1, N + 2))):
        g = ref.trgsw_sample(KEY, nonce, u, s, m, e, l, Bg, sigma, oracle.poly_naive_mul)
        out = oracle.external_product(np.ascontiguousarray(probe), oracle.trgsw_to_dft(np.ascontiguousarray(g), 1, l), l, Bg)
        want = np.zeros(N, dtype=U64) if m == 0 else (msg if e == 0 else oracle.poly_mul_by_xai(msg, e))
        worst = float(oracle.torus_dist(oracle.trlwe_phase(out, s.reshape(1, N)), want).max())
        print("TRGSW(%d X^%d): 2^%.1f from the selected message" % (m, e, np.log2(worst + 1)))
        assert worst < BOUND, (m, e, worst)


def _create(native_lib, s_rlwe, N, s_lwe, n):
    mk = native_lib.mosfhet_hip_client_key_create
    mk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    out = C.c_void_p()
    p = [None if s is None else np.ascontiguousarray(s, dtype=U64) for s in (s_rlwe, s_lwe)]
    rc = mk(C.byref(out), None if p[0] is None else p[0].ctypes.data_as(C.c_void_p), N, None if p[1] is None else p[1].ctypes.data_as(C.c_void_p), n)
    return rc, out


def test_client_key_info_and_refusals(native_lib):
    """info on hand-made keys (weight 0, only s[N - 1] set, all ones, small integers with negatives; with and without the other key) and creation's refusals: N not a
    power of two or outside 256 .. 4096, a coefficient beyond int16 either side, n = 0, both keys NULL, out NULL."""
    from mosfhet_amd import engine
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    rng = np.random.default_rng(1)
    N = 256
    small = _small_key(rng, N)
    lwe = _u64([1, 0, -2, 5, 0])
    for s, want in ((_corner_key(N, "zero"), (0, True)), (_corner_key(N, "last"), (1, True)), (_corner_key(N, "ones"), (N, True)),
                    (small, (int(np.count_nonzero(small)), False))):
        k = engine.client_key_create(s_rlwe=s)
        assert k.info() == dict(N=N, n=0, rlwe_weight=want[0], rlwe_binary=want[1], lwe_weight=0, lwe_binary=True), k.info()
        k.close()
    k = engine.client_key_create(s_rlwe=_corner_key(4096, "ones"), s_lwe=lwe)
    assert k.info() == dict(N=4096, n=5, rlwe_weight=4096, rlwe_binary=True, lwe_weight=3, lwe_binary=False), k.info()
    k.close()
    k = engine.client_key_create(s_lwe=_u64([1, 0, 1]))
    assert k.info() == dict(N=0, n=3, rlwe_weight=0, rlwe_binary=True, lwe_weight=2, lwe_binary=True), k.info()
    k.close()
    ones = np.ones(8192, dtype=U64)
    for bad in (0, 128, 255, 384, 1000, 8192, -256):
        rc, out = _create(native_lib, ones, bad, None, 0)
        assert rc == EINVAL and "N = %d" % bad in err() and out.value is None, (bad, err())
    for value, at in ((32768, 3), (-32769, 255), (1 << 40, 0)):
        s = np.zeros(N, dtype=U64)
        s[at] = U64(value & M64)
        rc, out = _create(native_lib, s, N, None, 0)
        assert rc == EINVAL and "h_s_rlwe[%d]" % at in err() and "16 bits" in err(), err()
        rc, out = _create(native_lib, None, 0, s, N)
        assert rc == EINVAL and "h_s_lwe[%d]" % at in err(), err()
    for value in (32767, -32768):
        s = np.zeros(N, dtype=U64)
        s[7] = U64(value & M64)
        rc, out = _create(native_lib, s, N, None, 0)
        assert rc == 0 and out.value
        assert native_lib.mosfhet_hip_client_key_destroy(out) == 0
    rc, out = _create(native_lib, None, 0, ones, 0)
    assert rc == EINVAL and "n = 0" in err()
    rc, out = _create(native_lib, None, 256, None, 3)
    assert rc == EINVAL and "h_s_rlwe" in err() and "h_s_lwe" in err() and out.value is None
    mk = native_lib.mosfhet_hip_client_key_create
    assert mk(None, ones.ctypes.data_as(C.c_void_p), 256, None, 0) == EINVAL and "out" in err()
    info = (C.c_int64 * 6)()
    gi = native_lib.mosfhet_hip_client_key_info
    gi.argtypes = [C.c_void_p, C.c_void_p]
    assert gi(None, info) == EINVAL and "key" in err()
    rc, out = _create(native_lib, ones, 256, None, 0)
    assert rc == 0 and gi(out, None) == EINVAL and "info" in err()
    assert gi(out, info) == 0 and list(info) == [256, 0, 256, 1, 0, 1]
    assert native_lib.mosfhet_hip_client_key_destroy(out) == 0
    assert native_lib.mosfhet_hip_client_key_destroy(None) == 0
    with pytest.raises(engine.MosfhetHipError, match="at least one key"):
        engine.client_key_create()


def test_trgsw_encrypt_plan_across_the_chunk_limit():
    """mosfhet_hip_trgsw_encrypt_plan swept across the limit of 2^20 rows per launch: rows = count x 2l; with a torus output chunks of 2^20 rows, one row launch each plus
    one transform each when the DFT output is asked for too (two workgroups per row); DFT only: the rows pass through the pool, at most 1 GiB of it."""
    from mosfhet_amd import engine
    lim = 1 << 20
    for N, l in ((1024, 2), (2048, 4), (4096, 1), (1024, 6), (256, 3)):
        for rows in (2 * l, lim - 2 * l, lim, lim + 2 * l, 3 * lim + 2 * l):
            count = rows // (2 * l)
            rows = count * 2 * l
            for outputs in engine.TRGSW_ENCRYPT_OUTPUTS:
                if N == 256 and outputs != "torus":
                    with pytest.raises(engine.MosfhetHipError, match="N = 256"):
                        engine.trgsw_encrypt_plan(N, l, count, outputs)
                    continue
                p = engine.trgsw_encrypt_plan(N, l, count, outputs)
                cap = min(lim, (1 << 30) // (16 * N)) if outputs == "dft" else lim
                chunk = min(rows, cap)
                chunks = -(-rows // chunk)
                assert p == dict(launches=chunks * (1 if outputs == "torus" else 2), workgroups=chunk * (1 if outputs == "torus" else 2),
                                 workspace_bytes=chunk * 16 * N if outputs == "dft" else 0, chunks=chunks), (N, l, count, outputs, p)
    assert engine.trgsw_encrypt_plan(1024, 2, lim // 4, "both")["chunks"] == 1 and engine.trgsw_encrypt_plan(1024, 2, lim // 4 + 1, "both")["chunks"] == 2
    assert engine.trgsw_encrypt_plan(2048, 4, 0) == dict(launches=0, workgroups=0, workspace_bytes=0, chunks=0)
    assert engine.trgsw_encrypt_plan(2048, 4, 632)["workspace_bytes"] == 632 * 8 * 2 * 2048 * 8
    for args, word in (((1000, 2, 1), "N = 1000"), ((1024, 0, 1), "l = 0"), ((1024, 7, 1), "l = 7"), ((1024, 2, -1), "count = -1")):
        with pytest.raises(engine.MosfhetHipError, match=word):
            engine.trgsw_encrypt_plan(*args)


def test_client_symbols_and_argument_checks(native_lib):
    """The library exports the entry points and the binding its functions; every refusal returns MOSFHET_HIP_EINVAL with a message naming the argument, on fake pointers
    and without a device: ctx missing; key missing, or the wrong key missing; count = -1; both TRGSW outputs NULL; the gadget (l Bg_bit >= 64, l < 1, l = 7); msg_bits 64
    and -1; null buffers; an input overlapping an output.  count == 0 does nothing."""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_client_key_create", "mosfhet_hip_client_key_destroy", "mosfhet_hip_client_key_info", "mosfhet_hip_tlwe_encrypt_batch",
                 "mosfhet_hip_trlwe_encrypt_batch", "mosfhet_hip_trgsw_encrypt_batch", "mosfhet_hip_trgsw_encrypt_plan", "mosfhet_hip_tlwe_phase_batch",
                 "mosfhet_hip_trlwe_phase_batch"):
        assert hasattr(native_lib, name), name
    for name in ("client_key_create", "trgsw_encrypt_plan", "ClientKey"):
        assert hasattr(engine, name), name
    for name in ("tlwe_encrypt", "trlwe_encrypt", "trgsw_encrypt", "tlwe_phase", "trlwe_phase"):
        assert hasattr(engine.Engine, name), name
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)     # never dereferenced
    N, n = 1024, 70
    both = engine.client_key_create(np.ones(N, dtype=U64), np.ones(n, dtype=U64))
    only_r = engine.client_key_create(s_rlwe=np.ones(N, dtype=U64))
    only_l = engine.client_key_create(s_lwe=np.ones(n, dtype=U64))
    base = 1 << 20
    at = lambda off: C.c_void_p(base + off)
    sig = C.c_double(2.0 ** -25)

    te = native_lib.mosfhet_hip_tlwe_encrypt_batch
    te.argtypes = [C.c_void_p] * 4 + [C.c_double, C.c_int, C.c_void_p]
    re_ = native_lib.mosfhet_hip_trlwe_encrypt_batch
    re_.argtypes = te.argtypes
    for f, key, wrong, word in ((te, both, only_r, "h_s_lwe"), (re_, both, only_l, "h_s_rlwe")):
        assert f(None, key.h, fake, fake, sig, 1, None) == EINVAL and "ctx" in err()
        assert f(fake, None, fake, fake, sig, 1, None) == EINVAL and "key" in err()
        assert f(fake, wrong.h, fake, fake, sig, 1, None) == EINVAL and word in err()
        assert f(fake, key.h, fake, fake, sig, -1, None) == EINVAL and "count = -1" in err()
        assert f(fake, key.h, fake, fake, C.c_double(-1.0), 1, None) == EINVAL and "sigma" in err()
        assert f(fake, key.h, None, fake, sig, 1, None) == EINVAL and "d_out" in err()
        assert f(fake, key.h, at(0), at(0), sig, 1, None) == EINVAL and "overlaps" in err()
        assert f(fake, key.h, None, None, sig, 0, None) == 0
    assert te(fake, both.h, fake, None, sig, 1, None) == EINVAL and "d_msg" in err()
    assert te(fake, both.h, at(0), at(3 * (n + 1) * 8 - 8), sig, 3, None) == EINVAL and "overlaps" in err()     # the last word of the samples

    ge = native_lib.mosfhet_hip_trgsw_encrypt_batch
    ge.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]
    assert ge(None, both.h, fake, fake, fake, None, 2, 8, sig, 1, None) == EINVAL and "ctx" in err()
    assert ge(fake, None, fake, fake, fake, None, 2, 8, sig, 1, None) == EINVAL and "key" in err()
    assert ge(fake, only_l.h, fake, fake, fake, None, 2, 8, sig, 1, None) == EINVAL and "h_s_rlwe" in err()
    assert ge(fake, both.h, fake, fake, fake, None, 2, 8, sig, -1, None) == EINVAL and "count = -1" in err()
    assert ge(fake, both.h, None, None, fake, None, 2, 8, sig, 1, None) == EINVAL and "d_out_dft" in err() and "d_out_torus" in err()
    for l, Bg in ((2, 33), (5, 13), (0, 8), (-1, 8), (7, 8), (2, 0), (4, 16), (1, 64), (2, 32)):
        assert ge(fake, both.h, fake, fake, fake, None, l, Bg, sig, 1, None) == EINVAL and ("gadget" in err() or "l = " in err()), (l, Bg, err())
    assert ge(fake, both.h, fake, None, None, None, 2, 8, sig, 1, None) == EINVAL and "d_m" in err()
    rows = 2 * 2 * 2 * N * 8        # bytes of one sample's rows, either domain
    assert ge(fake, both.h, at(0), at(rows - 8), at(1 << 30), None, 2, 8, sig, 1, None) == EINVAL and "d_out_dft overlaps d_out_torus" in err()
    assert ge(fake, both.h, at(0), None, at(rows - 4), None, 2, 8, sig, 1, None) == EINVAL and "d_out_dft overlaps d_m" in err()
    assert ge(fake, both.h, None, at(0), at(1 << 30), at(0), 2, 8, sig, 1, None) == EINVAL and "d_out_torus overlaps d_exp" in err()
    assert ge(fake, both.h, None, None, None, None, 2, 8, sig, 0, None) == EINVAL                               # no output stays refused at count 0
    assert ge(fake, both.h, fake, None, None, None, 2, 8, sig, 0, None) == 0
    small_ring = engine.client_key_create(s_rlwe=np.ones(512, dtype=U64))
    assert ge(fake, small_ring.h, fake, None, fake, None, 2, 8, sig, 1, None) == EINVAL and "N = 512" in err()  # no TRGSW_DFT form at this ring
    small_ring.close()

    tp = native_lib.mosfhet_hip_tlwe_phase_batch
    tp.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p]
    rp = native_lib.mosfhet_hip_trlwe_phase_batch
    rp.argtypes = tp.argtypes
    for f, wrong, word, in_bytes in ((tp, only_r, "h_s_lwe", (n + 1) * 8), (rp, only_l, "h_s_rlwe", 2 * N * 8)):
        assert f(None, both.h, fake, fake, 0, 1, None) == EINVAL and "ctx" in err()
        assert f(fake, None, fake, fake, 0, 1, None) == EINVAL and "key" in err()
        assert f(fake, wrong.h, fake, fake, 0, 1, None) == EINVAL and word in err()
        assert f(fake, both.h, fake, fake, 0, -1, None) == EINVAL and "count = -1" in err()
        assert f(fake, both.h, fake, fake, 64, 1, None) == EINVAL and "msg_bits = 64" in err()
        assert f(fake, both.h, fake, fake, -1, 1, None) == EINVAL and "msg_bits = -1" in err()
        assert f(fake, both.h, None, fake, 0, 1, None) == EINVAL and "d_out" in err()
        assert f(fake, both.h, fake, None, 0, 1, None) == EINVAL and "d_in" in err()
        assert f(fake, both.h, at(0), at(0), 4, 2, None) == EINVAL and "overlaps" in err()
        assert f(fake, both.h, at(2 * in_bytes - 8), at(0), 4, 2, None) == EINVAL and "overlaps" in err()       # the last word of the inputs
        assert f(fake, both.h, None, None, 63, 0, None) == 0
    p = native_lib.mosfhet_hip_trgsw_encrypt_plan
    p.argtypes = [C.c_int] * 4 + [C.c_void_p]
    info = (C.c_int64 * 4)()
    assert p(1024, 2, 1, 0, None) == EINVAL and "info" in err()
    assert p(1024, 2, 1, 3, info) == EINVAL and "with_torus_out = 3" in err()
    for k in (both, only_r, only_l):
        k.close()


def _compile_c(tmp_path):
    exe = str(tmp_path / "client_samples")
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "client_samples.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_client_c_program_compiles_and_links(native_lib, tmp_path):
    """tests/c/client_samples.c compiles with -Wall -Werror against include/mosfhet_hip.h alone and links against the built library (it runs in test_client_c_program)."""
    assert os.path.exists(_compile_c(tmp_path))


def test_client_kernels_of_the_build(native_lib):
    """The client half has no kernel of its own: its bodies are run-time kinds of trlwe_poly_keygen_kernel and tlwe_ksk_keygen_kernel, each still listed once and without
    scratch; the library holds exactly 329 kernels, none of them named client_*; tools/check_lds_barriers.py found nothing on the build."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    rows = kernel_table.table()
    for host in ("trlwe_poly_keygen_kernel", "tlwe_ksk_keygen_kernel"):
        mine = [r for r in rows if r["name"] == host]
        assert len(mine) == 1, (host, [r["name"] for r in mine])
        print("%-30s vgpr %3d  agpr %3d  sgpr %3d  lds %6d  scratch %4d" % (host, mine[0]["vgpr"], mine[0]["agpr"], mine[0]["sgpr"], mine[0]["lds"], mine[0]["scratch"]))
        assert mine[0]["scratch"] == 0, mine[0]
    assert not [r["name"] for r in rows if r["name"].startswith("client_")]
    assert len(rows) == 329, len(rows)
    with open(os.path.join(ROOT, "mosfhet_amd", "build", "lds_barrier_check.txt")) as fh:
        report = fh.read()
    assert ", 0 violations" in report, report


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


def _dev(eng, a):
    import mosfhet_amd as ma
    return ma.to_device(a, eng.device)


def _i32(eng, values):
    import torch
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device=eng.device)


def _guarded(eng, shape, dtype=None):
    """(the whole buffer, the view a call writes): sentinel words either side of every output"""
    import torch
    dtype = dtype or torch.int64
    n = int(np.prod(shape))
    buf = torch.full((n + 32,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=eng.device)
    return buf, buf[16:16 + n].view(dtype).view(*shape)


def _guards_intact(buf):
    import torch
    torch.cuda.synchronize()
    edge = torch.cat([buf[:16], buf[-16:]])
    return bool((edge == 0x5A5A5A5A5A5A5A5A).all())


def _check_tlwe(got, s, msg, nonce, first_row, sigma, what):
    n = s.size
    for q, row in enumerate(got.reshape(-1, n + 1)):
        r = first_row + q
        assert (row[:n] == ref.mask_row(KEY, nonce, r, n)).all(), (what, r)
        with np.errstate(over="ignore"):
            e = row[n:] - (row[:n] * s).sum(dtype=U64) - msg[q]
        _check_noise(e, nonce, r, sigma, what)


def _check_trlwe_rows(oracle, got, s, msgs, gadget, nonce, first_row, sigma, what):
    """got [rows][2][N]: the mask == the reference's mask (+ the gadget's words on it), and b - a * s - msg - gadget is the row's noise; a * s by oracle.poly_naive_mul
    on the PLAIN mask"""
    N = s.size
    for q, row in enumerate(got.reshape(-1, 2, N)):
        r = first_row + q
        a = ref.mask_row(KEY, nonce, r, N)
        g = gadget[q] if gadget is not None else np.zeros((2, N), dtype=U64)
        assert (row[0] == a + g[0]).all(), (what, r)
        e = row[1] - oracle.poly_naive_mul(a.copy(), s) - g[1] - (msgs[q] if msgs is not None else U64(0))
        _check_noise(e, nonce, r, sigma, what)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 70, 632])
def test_tlwe_known_answers(eng, n):
    """client_lwe_body, kind 3: one lane, exactly one pass of the 64-lane loop, a ragged second pass, SET lvl2's n; count 3, sigma 2^-15, a small-integer key with
    negatives; two calls under one secret: call 2 is on nonce 2.  Masks ==, noise within tolerance, sentinels either side of the output intact."""
    import mosfhet_amd as ma
    sigma = 2.0 ** -15
    rng = np.random.default_rng(600 + n)
    s = _small_key(rng, n)
    key = ma.engine.client_key_create(s_lwe=s)
    eng.set_keygen_secret(SECRET)
    seen = []
    for call in (1, 2):
        msg = rng.integers(0, 2 ** 64, size=3, dtype=U64)
        buf, out = _guarded(eng, (3, n + 1))
        eng.tlwe_encrypt(key, _dev(eng, msg), sigma, out=out)
        assert _guards_intact(buf)
        got = ma.to_numpy(out)
        _check_tlwe(got, s, msg, R.call_nonce(call, ref.KIND_TLWE), 0, sigma, "TLWE n %d call %d" % (n, call))
        seen.append(got[:, :n].copy())
    assert not (seen[0] == seen[1]).any()
    key.close()


TRLWE_KEYS = ["binary", "small", "zero", "last", "ones"]


def _trlwe_key(kind, N, rng):
    return _binary_key(rng, N) if kind == "binary" else _small_key(rng, N) if kind == "small" else _corner_key(N, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", TRLWE_KEYS)
@pytest.mark.parametrize("N", [256, 1024, 2048])
def test_trlwe_known_answers(eng, oracle, N, kind):
    """client_ring_body, kind 1, l = 0: count 3, binary and small keys and the three corner weights (0, only s[N - 1], N), msg NULL then msg random (call 2: nonce 2).
    Every word: the mask ==, b - a * s - msg (a * s by oracle.poly_naive_mul) within tolerance of the row's noise."""
    import mosfhet_amd as ma
    sigma = 2.0 ** -15
    rng = np.random.default_rng([700, N, TRLWE_KEYS.index(kind)])
    s = _trlwe_key(kind, N, rng)
    key = ma.engine.client_key_create(s_rlwe=s)
    assert key.rlwe_binary == (kind != "small")
    eng.set_keygen_secret(SECRET)
    msgs = rng.integers(0, 2 ** 64, size=(3, N), dtype=U64)
    for call, m in ((1, None), (2, msgs)):
        buf, out = _guarded(eng, (3, 2, N))
        eng.trlwe_encrypt(key, None if m is None else _dev(eng, m), sigma, count=3, out=out)
        assert _guards_intact(buf)
        _check_trlwe_rows(oracle, ma.to_numpy(out), s, m, None, R.call_nonce(call, ref.KIND_TRLWE), 0, sigma, "TRLWE N %d %s call %d" % (N, kind, call))
    key.close()


MS, EXPS = (0, 1, -1, 3), lambda N: (0, 1, N - 1, N, 2 * N - 1, -3)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 2, 5])
@pytest.mark.parametrize("N,l,Bg", [(1024, 2, 8), (1024, 3, 10), (2048, 4, 9)])
def test_trgsw_known_answers(eng, oracle, N, l, Bg, count):
    """client_ring_body, kind 1, l > 0, both outputs: m from {0, 1, -1, 3} and exponents from {0, 1, N - 1, N, 2N - 1, -3} (sign flips and wraps; the nine cases walk
    through all of both lists).  Torus rows: row q of sample u is row u 2l + q of the call -- plain mask + the gadget on component 0, body formed from the PLAIN mask +
    the gadget on component 1.  The doubles == eng.torus_to_dft of the torus rows, on every double; a DFT-only call after installing the secret again gives the same
    doubles; exp None = all zero."""
    import torch
    import mosfhet_amd as ma
    sigma = 2.0 ** -25
    rng = np.random.default_rng([800, N, l, count])
    s = _binary_key(rng, N) if l != 3 else _small_key(rng, N)
    key = ma.engine.client_key_create(s_rlwe=s)
    off = (l * 7 + count * 3) % 12
    ms = [MS[(off + u) % 4] for u in range(count)]
    es = [EXPS(N)[(off + u) % 6] for u in range(count)]
    eng.set_keygen_secret(SECRET)
    dft, torus = eng.trgsw_encrypt(key, _i32(eng, ms), l, Bg, sigma, exp=_i32(eng, es), torus=True)
    assert dft.shape == (count, 2 * l, 2, N) and dft.dtype == torch.float64 and torus.shape == (count, 2 * l, 2, N)
    gadget = np.concatenate([ref.gadget_rows(N, ms[u], es[u], l, Bg) for u in range(count)])
    assert np.count_nonzero(gadget) == 2 * l * sum(m != 0 for m in ms)
    _check_trlwe_rows(oracle, ma.to_numpy(torus), s, None, gadget, R.call_nonce(1, ref.KIND_TRGSW), 0, sigma, "TRGSW (%d, %d, %d) count %d" % (N, l, Bg, count))
    want = eng.torus_to_dft(torus.view(-1, N)).view(count, 2 * l, 2, N)
    torch.cuda.synchronize()
    assert torch.equal(dft.view(torch.int64), want.view(torch.int64)), "%d doubles differ from torus_to_dft of the torus rows" % int((dft != want).sum())
    eng.set_keygen_secret(SECRET)
    buf, only = _guarded(eng, (count, 2 * l, 2, N), torch.float64)
    d_m, d_e = _i32(eng, ms), _i32(eng, es)
    ma.engine._check(ma.engine.lib().mosfhet_hip_trgsw_encrypt_batch(eng.h, key.h, C.c_void_p(only.data_ptr()), None, C.c_void_p(d_m.data_ptr()), C.c_void_p(d_e.data_ptr()),
                                                                     l, Bg, C.c_double(sigma), count, eng._stream()))
    assert _guards_intact(buf)
    assert torch.equal(only.view(torch.int64), dft.view(torch.int64)), "the DFT-only call gives other doubles"
    if count == 2:
        eng.set_keygen_secret(SECRET)
        t0 = eng.trgsw_encrypt(key, _i32(eng, ms), l, Bg, sigma, torus=True, dft=False)
        g0 = np.concatenate([ref.gadget_rows(N, m, 0, l, Bg) for m in ms])
        _check_trlwe_rows(oracle, ma.to_numpy(t0), s, None, g0, R.call_nonce(1, ref.KIND_TRGSW), 0, sigma, "TRGSW exp None")
    key.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 70, 632, 2048])
def test_tlwe_phases_equal_the_oracle(eng, oracle, n):
    """client_lwe_body, kind 4 == oracle.tlwe_phase: counts 1, 2, 5, 130, an all-ones key against masks of
    2^64 - 1 and 2^63 so that the sums wrap, and a small key with negatives against random words; msg_bits 0, 1, 4, 63 against the reference's decode."""
    import mosfhet_amd as ma
    rng = np.random.default_rng(900 + n)
    for s in (np.ones(n, dtype=U64), _small_key(rng, n)):
        key = ma.engine.client_key_create(s_lwe=s)
        for count in (1, 2, 5, 130):
            ct = rng.integers(0, 2 ** 64, size=(count, n + 1), dtype=U64)
            ct[0, :n] = M64
            if count > 1:
                ct[1, :n] = 1 << 63
            want = _u64([oracle.tlwe_phase(c, s) for c in ct])
            buf, out = _guarded(eng, (count,))
            eng.tlwe_phase(key, _dev(eng, ct), 0, out=out)
            assert _guards_intact(buf)
            assert (ma.to_numpy(out) == want).all(), (n, count)
            for bits in (1, 4, 63):
                assert (ma.to_numpy(eng.tlwe_phase(key, _dev(eng, ct), bits)) == ref.decode(want, bits)).all(), (n, count, bits)
        key.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zero", "last", "ones", "small"])
@pytest.mark.parametrize("N", [256, 1024, 2048, 4096])
def test_trlwe_phases_equal_the_oracle(eng, oracle, N, kind):
    """client_ring_body, kind 2 == oracle.trlwe_phase on every word: keys of weight 0, 1 (only s[N - 1]) and N, and small integers with negatives; samples of all 0, all 1,
    all 2^63, all 2^64 - 1 and random words; msg_bits 1, 4, 63 against the reference's decode."""
    import mosfhet_amd as ma
    rng = np.random.default_rng([1000, N])
    s = _trlwe_key(kind, N, rng)
    key = ma.engine.client_key_create(s_rlwe=s)
    ct = rng.integers(0, 2 ** 64, size=(6, 2, N), dtype=U64)
    for i, w in enumerate((0, 1, 1 << 63, M64)):
        ct[i] = U64(w)
    ct[4, 0] = M64                                               # every term wraps, random body
    want = np.stack([oracle.trlwe_phase(np.ascontiguousarray(c), s.reshape(1, N)) for c in ct])
    buf, out = _guarded(eng, (6, N))
    eng.trlwe_phase(key, _dev(eng, ct), 0, out=out)
    assert _guards_intact(buf)
    assert (ma.to_numpy(out) == want).all(), "%d words differ" % int((ma.to_numpy(out) != want).sum())
    for bits in (1, 4, 63):
        assert (ma.to_numpy(eng.trlwe_phase(key, _dev(eng, ct), bits)) == ref.decode(want, bits)).all(), bits
    key.close()


@pytest.mark.gpu
def test_round_trip_decodes(eng):
    """phase(encrypt(m)) decodes m at four bits, sigma 2^-25, both sample types (n = 632, N = 2048, binary keys)."""
    import mosfhet_amd as ma
    rng = np.random.default_rng(1100)
    n, N, sigma = 632, 2048, 2.0 ** -25
    key = ma.engine.client_key_create(_binary_key(rng, N), _binary_key(rng, n))
    m_t, m_r = rng.integers(0, 16, size=40).astype(U64), rng.integers(0, 16, size=(3, N)).astype(U64)
    got = eng.tlwe_phase(key, eng.tlwe_encrypt(key, _dev(eng, m_t << U64(60)), sigma), 4)
    assert (ma.to_numpy(got) == m_t).all()
    got = eng.trlwe_phase(key, eng.trlwe_encrypt(key, _dev(eng, m_r << U64(60)), sigma), 4)
    assert (ma.to_numpy(got) == m_r).all()
    key.close()


@pytest.mark.gpu
def test_selectors_drive_the_encrypted_memory(eng, oracle):
    """Selectors from trgsw_encrypt at (2048, 4, 9), sigma 2^-44, drive Engine.trlwe_ram_read (size 2, count 2; cells made by trlwe_encrypt): the cell opened by
    trlwe_phase lies within 2^57 of the message stored at the address (selector i = bit i of the address, least significant first)."""
    import mosfhet_amd as ma
    N, l, Bg, sigma, size, count = 2048, 4, 9, 2.0 ** -44, 2, 2
    rng = np.random.default_rng(1200)
    s = _binary_key(rng, N)
    key = ma.engine.client_key_create(s_rlwe=s)
    msgs = rng.integers(0, 16, size=(count, 1 << size, N)).astype(U64) << U64(60)
    mem = eng.trlwe_encrypt(key, _dev(eng, msgs.reshape(-1, N)), sigma).view(count, 1 << size, 2, N)
    addrs = [2, 1]
    bits = [[(a >> i) & 1 for i in range(size)] for a in addrs]
    import torch
    sel = eng.trgsw_encrypt(key, torch.tensor(bits, dtype=torch.int32, device=eng.device), l, Bg, sigma)
    assert sel.shape == (count, size, 2 * l, 2, N)
    out = eng.trlwe_ram_read(sel, mem, size, l, Bg)
    ph = ma.to_numpy(eng.trlwe_phase(key, out))
    for b in range(count):
        d = float(oracle.torus_dist(ph[b], msgs[b, addrs[b]]).max())
        others = min(float(oracle.torus_dist(ph[b], msgs[b, a]).max()) for a in range(1 << size) if a != addrs[b])
        print("input %d, address %d: 2^%.1f from the stored message" % (b, addrs[b], np.log2(d + 1)))
        assert d < BOUND and others > 2.0 ** 59, (b, d, others)
    key.close()


@pytest.mark.gpu
def test_encrypted_inputs_go_through_a_bootstrap(eng):
    """tlwe_encrypt under an n = 16 key, generate_bootstrap_key from the same keys, one functional bootstrap at SET_1's ring and gadget (N = 1024, l = 2, Bg = 2^8, four
    slots), opened through tlwe_phase under the TRLWE key read as an LWE key (the extracted key): the table's entries come out."""
    import mosfhet_amd as ma
    from mosfhet_amd import host
    P = ma.PARAMS_SET1
    N, n = P["N"], 16
    rng = np.random.default_rng(1300)
    s_rlwe, s_lwe = _binary_key(rng, N), _binary_key(rng, n)
    key = ma.engine.client_key_create(s_rlwe, s_lwe)
    extracted = ma.engine.client_key_create(s_lwe=s_rlwe)
    eng.set_keygen_secret(SECRET)
    bsk = eng.generate_bootstrap_key(s_rlwe, s_lwe, P["l"], P["Bg_bit"], P["rlwe_sigma"], 0xB5)
    lut = _u64([v << 60 for v in (3, 9, 14, 6)])
    tv = _dev(eng, host.torus_packing(lut, 1, N)[None])
    slots = [b % 4 for b in range(8)]
    ct = eng.tlwe_encrypt(key, _dev(eng, _u64([host.double2torus(v / 8.0) for v in slots])), 2.0 ** -25)
    out = eng.functional_bootstrap(bsk, tv, ct, 4)
    got = ma.to_numpy(eng.tlwe_phase(extracted, out, 4))
    assert list(got) == [int(lut[v]) >> 60 for v in slots], got
    bsk.free()
    key.close()
    extracted.close()


@pytest.mark.gpu
def test_count_zero_batch_position_and_two_contexts(eng):
    """count = 0 writes nothing and draws no nonce; count 5, then the same secret again and count 2, gives the first two samples (all three sample types); one handle
    serves a second context with the same words."""
    import torch
    import mosfhet_amd as ma
    rng = np.random.default_rng(1400)
    N, n, l, Bg, sigma = 1024, 70, 2, 8, 2.0 ** -25
    key = ma.engine.client_key_create(_binary_key(rng, N), _small_key(rng, n))
    msg = _dev(eng, rng.integers(0, 2 ** 64, size=5, dtype=U64))
    polys = _dev(eng, rng.integers(0, 2 ** 64, size=(5, N), dtype=U64))
    m, e = _i32(eng, [1, 0, -1, 3, 1]), _i32(eng, [0, 5, N, -3, 1])
    empty = torch.empty(0, dtype=torch.int64, device=eng.device)
    eng2 = ma.Engine(0)

    def run(en, k):
        en.set_keygen_secret(SECRET)
        assert en.tlwe_encrypt(key, empty, sigma).shape == (0, n + 1)                       # no nonce drawn: the next call is call 1
        d, t = en.trgsw_encrypt(key, m[:k], l, Bg, sigma, exp=e[:k], torus=True)
        return en.tlwe_encrypt(key, msg[:k], sigma), en.trlwe_encrypt(key, polys[:k], sigma), d, t

    five, two, other = run(eng, 5), run(eng, 2), run(eng2, 5)
    torch.cuda.synchronize()
    for a, b, c in zip(five, two, other):
        assert torch.equal(a[:2].view(torch.int64), b.view(torch.int64)) and torch.equal(a.view(torch.int64), c.view(torch.int64))
    assert eng.trlwe_phase(key, five[1][:0]).shape == (0, N) and eng.tlwe_phase(key, five[0][:0], 4).shape == (0,)
    assert torch.equal(eng.trlwe_phase(key, five[1]), eng2.trlwe_phase(key, five[1]))
    eng2.close()
    key.close()


@pytest.mark.gpu
def test_two_host_threads_draw_distinct_nonces(eng):
    """Two host threads, six TLWE calls each on streams of their own under one secret: the twelve calls are on the nonces of calls 1 .. 12, each once (the first mask word
    of sample 0 tells which), and no mask word is shared between any two calls."""
    import torch
    import mosfhet_amd as ma
    n, sigma = 70, 2.0 ** -15
    key = ma.engine.client_key_create(s_lwe=np.ones(n, dtype=U64))
    msg = torch.zeros(2, dtype=torch.int64, device=eng.device)
    eng.tlwe_encrypt(key, msg, sigma)                             # the key image is on the device
    eng.set_keygen_secret(SECRET)
    torch.cuda.synchronize()
    outs, errors = [[], []], []

    def work(t):
        try:
            with torch.cuda.stream(torch.cuda.Stream(eng.device)):
                for _ in range(6):
                    outs[t].append(eng.tlwe_encrypt(key, msg, sigma))
                torch.cuda.current_stream().synchronize()
        except Exception as ex:       # noqa: BLE001
            errors.append(ex)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    got = [ma.to_numpy(o) for o in outs[0] + outs[1]]
    first = {int(ref.mask_row(KEY, R.call_nonce(c, ref.KIND_TLWE), 0, 1)[0]): c for c in range(1, 13)}
    calls = sorted(first[int(g[0, 0])] for g in got)
    assert calls == list(range(1, 13)), calls
    words = np.concatenate([g[:, :n].reshape(-1) for g in got])
    assert np.unique(words).size == words.size
    for g in got:
        c = first[int(g[0, 0])]
        assert (g[1, :n] == ref.mask_row(KEY, R.call_nonce(c, ref.KIND_TLWE), 1, n)).all()
    key.close()


@pytest.mark.gpu
def test_tlwe_rows_across_the_launch_chunks(eng):
    """The encrypt launchers work in chunks of 2^20 rows (first_row): TLWE at n = 1, 2^20 + 3 samples; the rows either side of the seam, the first and the last."""
    import torch
    import mosfhet_amd as ma
    sigma, count = 2.0 ** -15, (1 << 20) + 3
    s = _u64([-3])
    key = ma.engine.client_key_create(s_lwe=s)
    msg = torch.arange(count, dtype=torch.int64, device=eng.device) * 0x1E3779B97F4A7C15
    eng.set_keygen_secret(SECRET)
    out = eng.tlwe_encrypt(key, msg, sigma)
    for first, k in (((1 << 20) - 2, 4), (count - 1, 1), (0, 1)):
        _check_tlwe(ma.to_numpy(out[first:first + k]), s, ma.to_numpy(msg[first:first + k]), R.call_nonce(1, ref.KIND_TLWE), first, sigma, "TLWE chunks")
    key.close()


@pytest.mark.gpu
def test_phase_calls_are_captured_in_a_graph(eng):
    """Both phase calls captured on a side stream after an eager call of that shape, replayed on other inputs copied into the captured buffer: each replay == the eager
    words -- no hidden allocation, synchronisation or state.  One stream, no parallel branches."""
    import torch
    import mosfhet_amd as ma
    rng = np.random.default_rng(1500)
    N, n = 1024, 70
    key = ma.engine.client_key_create(_binary_key(rng, N), _small_key(rng, n))
    for run, shape in ((lambda x, out=None: eng.tlwe_phase(key, x, 4, out=out), (5, n + 1)), (lambda x, out=None: eng.trlwe_phase(key, x, 0, out=out), (3, 2, N))):
        xs = [_dev(eng, rng.integers(0, 2 ** 64, size=shape, dtype=U64)) for _ in range(2)]
        eager = [run(x).clone() for x in xs]
        torch.cuda.synchronize()
        assert not torch.equal(eager[0], eager[1])
        d_in, d_out = xs[0].clone(), torch.empty_like(eager[0])
        side = torch.cuda.Stream(eng.device)
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                run(d_in, out=d_out)
        for r in (1, 0, 1):
            d_in.copy_(xs[r])
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(d_out, eager[r]), "replay on inputs %d differs from the plain call" % r
        del g
    key.close()


@pytest.mark.gpu
def test_encryption_is_refused_on_a_capturing_stream(eng):
    """Each encrypt call on a capturing stream returns MOSFHET_HIP_EINVAL ("capture") with nothing launched: the graph -- which also holds one phase call, captured
    after the refusals, so the capture itself stayed valid -- replays to untouched encrypt outputs, and the refused calls drew no nonce: the next eager call is still
    call 1.  The capture is ended whatever happens (torch.cuda.graph ends it on the way out)."""
    import torch
    import mosfhet_amd as ma
    rng = np.random.default_rng(1600)
    N, n, sigma = 1024, 70, 2.0 ** -25
    s_lwe = _small_key(rng, n)
    key = ma.engine.client_key_create(_binary_key(rng, N), s_lwe)
    msg = _dev(eng, rng.integers(0, 2 ** 64, size=2, dtype=U64))
    m = _i32(eng, [1, 0])
    eng.tlwe_encrypt(key, msg, sigma)                             # the key image is on the device
    outs = [torch.full((2, n + 1), 7, dtype=torch.int64, device=eng.device), torch.full((2, 2, N), 7, dtype=torch.int64, device=eng.device),
            torch.full((2, 4, 2, N), 7, dtype=torch.int64, device=eng.device)]
    calls = [lambda: eng.tlwe_encrypt(key, msg, sigma, out=outs[0]), lambda: eng.trlwe_encrypt(key, None, sigma, count=2, out=outs[1]),
             lambda: ma.engine._check(ma.engine.lib().mosfhet_hip_trgsw_encrypt_batch(eng.h, key.h, None, C.c_void_p(outs[2].data_ptr()), C.c_void_p(m.data_ptr()), None, 2, 8,
                                                                                      C.c_double(sigma), 2, eng._stream()))]
    ct = eng.tlwe_encrypt(key, msg, sigma)
    opened, d_open = eng.tlwe_phase(key, ct, 0).clone(), torch.zeros(2, dtype=torch.int64, device=eng.device)
    eng.set_keygen_secret(SECRET)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(eng.device)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    refused = []
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for call in calls:
                try:
                    call()
                    refused.append(None)
                except ma.MosfhetHipError as ex:
                    refused.append(str(ex))
            eng.tlwe_phase(key, ct, 0, out=d_open)
    assert len(refused) == 3 and all(r is not None and "error -1" in r and "capture" in r for r in refused), refused
    g.replay()
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs) and torch.equal(d_open, opened)
    got = ma.to_numpy(eng.tlwe_encrypt(key, msg, sigma))
    _check_tlwe(got, s_lwe, ma.to_numpy(msg), R.call_nonce(1, ref.KIND_TLWE), 0, sigma, "the call after the refused ones")
    del g
    key.close()


@pytest.mark.gpu
def test_every_client_kind_has_its_own_nonce(eng, oracle):
    """One call of each kind under one secret with a generator call between them (TLWE, LWE table, TRLWE, TRGSW): the noise of call i matches call_nonce(i, kind) -- and
    not the nonce of the call before or after, nor another kind's tag (1 .. 8) at the same index."""
    import mosfhet_amd as ma
    N, n, sigma = 1024, 70, 2.0 ** -25
    rng = np.random.default_rng(1700)
    s, s_lwe = _binary_key(rng, N), _binary_key(rng, n)
    key = ma.engine.client_key_create(s, s_lwe)
    eng.set_keygen_secret(SECRET)
    zeros = _dev(eng, np.zeros(6, dtype=U64))
    t = ma.to_numpy(eng.tlwe_encrypt(key, zeros, sigma))                                        # call 1, kind 6
    ksk = eng.generate_keyswitch_key(s_lwe, _u64([1, 1]), 2, 2, sigma, 0x77)                    # call 2, kind 5
    rows = eng.export_key_rows(ksk, 0, 6)
    ksk.free()
    r = ma.to_numpy(eng.trlwe_encrypt(key, None, sigma, count=2))                               # call 3, kind 7
    g = ma.to_numpy(eng.trgsw_encrypt(key, _i32(eng, [0]), 2, 8, sigma, torus=True, dft=False))  # call 4, kind 8
    with np.errstate(over="ignore"):
        e_t = np.array([c[n] - (c[:n] * s_lwe).sum(dtype=U64) for c in t])
        e_k = np.array([rows[q, n] - (rows[q, :n] * s_lwe).sum(dtype=U64) - U64(((q % 3 + 1) << (64 - (q // 3 + 1) * 2)) & M64) for q in range(6)])
    noise = {ref.KIND_TRLWE: (3, 1, r[1, 1] - oracle.poly_naive_mul(r[1, 0].copy(), s)), ref.KIND_TRGSW: (4, 3, g[0, 3, 1] - oracle.poly_naive_mul(g[0, 3, 0].copy(), s))}
    for kind, (call, row, e) in noise.items():
        _check_noise(e, R.call_nonce(call, kind), row, sigma, "call %d (kind %d)" % (call, kind))
        others = [(call - 1, kind), (call + 1, kind)] + [(call, other) for other in range(1, 9) if other != kind] + [(kind, call), (0, kind)]
        for c2, k2 in others:
            assert _mismatch(e, R.call_nonce(c2, k2), row, sigma) > 2.0 ** -3, (call, kind, c2, k2)
    # the TLWE kinds have one noise word per row: six rows each, none within tolerance of a neighbouring stream
    for kind, call, e in ((ref.KIND_TLWE, 1, e_t), (R.KIND_TLWE_KSK, 2, e_k)):
        for q in range(6):
            _check_noise(e[q:q + 1], R.call_nonce(call, kind), q, sigma, "call %d (kind %d)" % (call, kind))
        for c2, k2 in [(call - 1, kind), (call + 1, kind)] + [(call, other) for other in range(1, 9) if other != kind]:
            off = [float(_noise_off(e[q:q + 1], R.call_nonce(c2, k2), q, sigma, 0)[0]) for q in range(6)]
            assert min(off) > R.noise_tolerance(sigma) and max(off) > 2.0 ** -3 * sigma * 2.0 ** 64, (kind, c2, k2, off)
    key.close()


@pytest.mark.gpu
def test_client_c_program(native_lib, tmp_path):
    """tests/c/client_samples.c on the plain C ABI: create, encrypt, phase, destroy; TLWE and TRLWE round trips at four bits, TRGSW rows open to their gadget terms."""
    r = subprocess.run([_compile_c(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "client_samples ok" in r.stdout, r.stdout[-3000:]
