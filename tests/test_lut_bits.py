"""Function evaluation on LWE-encrypted bits in one call (include/mosfhet_hip.h: mosfhet_hip_circuit_bootstrap_3_dft_batch, mosfhet_hip_lut_bits_batch,
mosfhet_hip_lut_bits_plan; mosfhet_amd/csrc/capi_bits.inc; bootstrap_kernels.h: trlwe_fft_keyswitch_kernel mode 3; include/mosfhet_compat.h: mosfhet_eval_LUTs_bits).

Expected words come from the oracle (oracle.circuit_bootstrap_3, oracle.bk_to_dft, tests/test_leveled_lut.py::_composition, oracle.tlwe_keyswitch) and, where the
oracle is too slow for the shape, from the entry points that existed before (circuit_bootstrap_3, trgsw_to_dft, leveled_lut_tables, tlwe_keyswitch).  Every comparison
is == on all words, doubles compared as their 64-bit patterns; there is no tolerance anywhere.  The one decryption bound (2^61, half the spacing of the one-bit
messages 0 and 1/4) is a condition on the inputs that the earlier four-call composition alone must meet.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_leveled_lut import _composition, _map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
_CACHE = {}


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_bits_symbols_and_argument_checks(native_lib):
    """The library exports the new entry points; mosfhet_hip_lut_bits_batch refuses null handles, size 0 and 22, tables 0 and 65 and count < 0 with MOSFHET_HIP_EINVAL
    and a message naming the argument -- on fake pointers, before any handle is read and before any HIP call (this runs without a GPU); count == 0 is OK."""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_circuit_bootstrap_3_dft_batch", "mosfhet_hip_lut_bits_batch", "mosfhet_hip_lut_bits_plan", "mosfhet_hip_set_lut_bits_workspace",
                 "mosfhet_eval_LUTs_bits"):
        assert hasattr(native_lib, name), name
    for name in ("lut_bits_plan", "set_lut_bits_workspace"):
        assert hasattr(engine, name), name
    for name in ("circuit_bootstrap_3_dft", "lut_bits", "lut_bits_plan"):
        assert hasattr(engine.Engine, name), name
    f = native_lib.mosfhet_hip_lut_bits_batch
    f.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_int, C.c_void_p]
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)     # never dereferenced: every call below ends on its scalar arguments
    assert f(None, fake, fake, fake, fake, fake, fake, fake, 8, 8, 2, None) == EINVAL and "ctx" in err()
    assert f(fake, None, fake, fake, fake, fake, fake, fake, 8, 8, 2, None) == EINVAL and "bsk" in err()
    assert f(fake, fake, None, fake, fake, fake, fake, fake, 8, 8, 2, None) == EINVAL and "kska" in err()
    assert f(fake, fake, fake, None, fake, fake, fake, fake, 8, 8, 2, None) == EINVAL and "kskb" in err()
    assert f(fake, fake, fake, fake, None, fake, fake, fake, 0, 8, 2, None) == EINVAL and "size = 0" in err()
    assert f(fake, fake, fake, fake, fake, fake, fake, fake, -3, 8, 2, None) == EINVAL and "size = -3" in err()
    assert f(fake, fake, fake, fake, fake, fake, fake, fake, 22, 8, 2, None) == EINVAL and "size = 22" in err()
    assert f(fake, fake, fake, fake, fake, fake, fake, fake, 8, 0, 2, None) == EINVAL and "tables = 0" in err()
    assert f(fake, fake, fake, fake, fake, fake, fake, fake, 8, 65, 2, None) == EINVAL and "tables = 65" in err()
    assert f(fake, fake, fake, fake, fake, fake, fake, fake, 8, 8, -1, None) == EINVAL and "count = -1" in err()
    assert f(fake, fake, fake, fake, fake, fake, fake, fake, 8, 8, 0, None) == 0                   # count == 0: nothing to do, no handle read
    assert f(fake, fake, fake, fake, None, fake, fake, fake, 21, 64, 0, None) == 0
    assert f(fake, fake, fake, fake, fake, fake, fake, fake, 0, 8, 0, None) == EINVAL and "size = 0" in err()      # ... after the scalar checks
    g = native_lib.mosfhet_hip_circuit_bootstrap_3_dft_batch
    g.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    assert g(None, None, None, None, None, None, 1, None) == EINVAL and "circuit_bootstrap_3_dft" in err()
    plan = (C.c_longlong * 10)()
    p = native_lib.mosfhet_hip_lut_bits_plan
    assert p(2048, 4, 8, 8, 2, 256, None) == EINVAL
    assert p(4096, 1, 8, 8, 2, 256, plan) == EINVAL and "N = 4096" in err()
    assert p(512, 1, 8, 8, 2, 256, plan) == EINVAL and "N = 512" in err()
    assert p(2048, 7, 8, 8, 2, 256, plan) == EINVAL and "l = 7" in err()
    assert p(2048, 4, 0, 8, 2, 256, plan) == EINVAL and "size = 0" in err()
    assert p(2048, 4, 22, 8, 2, 256, plan) == EINVAL and "size = 22" in err()
    assert p(1024, 2, 21, 8, 2, 256, plan) == EINVAL and "size = 21" in err()
    assert p(2048, 4, 8, 0, 2, 256, plan) == EINVAL and "tables = 0" in err()
    assert p(2048, 4, 8, 65, 2, 256, plan) == EINVAL and "tables = 65" in err()
    assert p(2048, 4, 8, 8, 0, 256, plan) == EINVAL and "count = 0" in err()
    assert p(2048, 4, 8, 8, 2, 0, plan) == EINVAL and "cus = 0" in err()
    assert p(2048, 4, 8, 8, 2, 256, plan) == 0
    native_lib.mosfhet_hip_set_lut_bits_workspace.argtypes = [C.c_longlong]
    assert native_lib.mosfhet_hip_set_lut_bits_workspace(-1) == EINVAL and "bytes = -1" in err()


def test_bits_plan_is_a_pure_function(native_lib):
    """mosfhet_hip_lut_bits_plan -- the function the launcher decides with -- over both rings, several gadgets, sizes, table counts, batches, CU counts and bounds:
    1 <= chunk <= count, the chunks cover the batch, selector bytes = chunk * size * 2l * 2 * N * 8 and within the bound unless chunk == 1, chunk as large as the
    bound allows and monotone in it, nothing depends on the CU count, the LUT fields are leveled_lut_tables_plan of one chunk; the setter's 0 restores the default."""
    from mosfhet_amd import engine
    GiB = 1 << 30

    def check(N, l, size, tables, count, cus, bound):
        p = engine.lut_bits_plan(N, l, size, tables, count, cus)
        what = (N, l, size, tables, count, cus, bound, p)
        per_input = size * 2 * l * 2 * N * 8
        chunk = p["chunk"]
        assert 1 <= chunk <= count and p["chunks"] == -(-count // chunk), what
        assert p["selector_bytes"] == chunk * per_input and p["cb_bits"] == chunk * size, what
        assert p["selector_bytes"] <= bound or chunk == 1, what
        assert chunk == count or (chunk + 1) * per_input > bound or (chunk + 1) * size > 1 << 20, what
        assert p == engine.lut_bits_plan(N, l, size, tables, count, 256), what
        assert p["lut"] == engine.leveled_lut_tables_plan(N, l, size, tables, chunk, cus), what
        return p

    default = engine.lut_bits_plan(2048, 4, 8, 8, 4096)
    assert (default["chunk"], default["chunks"], default["selector_bytes"], default["cb_bits"]) == (1024, 4, 2 * GiB, 8192), default     # 2 GiB: 8192 bits at lvl2
    for cus in (256, 64):
        for N in (1024, 2048):
            log_N = N.bit_length() - 1
            for l in (1, 2, 4, 6):
                for size in (1, 8, log_N, log_N + 1, log_N + 5, log_N + engine.LEVELED_LUT_MAX_LEVELS):
                    for tables in (1, 8, 64):
                        for count in (1, 3, 1024, 4096):
                            check(N, l, size, tables, count, cus, 2 * GiB)
    try:
        per_input = 12 * 2 * 4 * 2 * 2048 * 8
        last = 0
        for bound in (1, per_input - 1, per_input, 2 * per_input - 1, 2 * per_input, 3 * per_input, 5 * per_input - 1, 5 * per_input, GiB, 64 * GiB):
            engine.set_lut_bits_workspace(bound)
            p = check(2048, 4, 12, 2, 5, 256, bound)
            assert p["chunk"] == max(1, min(5, bound // per_input)) and p["chunk"] >= last, (bound, p)
            last = p["chunk"]
        assert last == 5
        engine.set_lut_bits_workspace(1 << 50)                        # whatever the bound: at most 2^20 bits per circuit-bootstrap launch
        p = check(1024, 1, 8, 1, 1 << 20, 256, 1 << 50)
        assert p["cb_bits"] == 1 << 20 and p["chunks"] == 8, p
        with pytest.raises(engine.MosfhetHipError, match="bytes = -5"):
            engine.set_lut_bits_workspace(-5)
    finally:
        engine.set_lut_bits_workspace(0)
    assert engine.lut_bits_plan(2048, 4, 8, 8, 4096) == default


def test_bits_kernels_of_the_build(native_lib):
    """The built library still holds fewer than 330 kernels, and trlwe_fft_keyswitch_kernel -- the kernel that gained the selector mode -- once per ring, without
    scratch and within the 512 registers of a wavefront at one wavefront per SIMD."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    rows = kernel_table.table()
    mine = sorted((r for r in rows if r["name"].startswith("trlwe_fft_keyswitch_kernel<")), key=lambda r: r["name"])
    for r in mine:
        print("%-55s vgpr %3d  agpr %3d  sgpr %3d  lds %6d  scratch %4d" % (r["name"], r["vgpr"], r["agpr"], r["sgpr"], r["lds"], r["scratch"]))
    names = [r["name"].replace("> >", ">>") for r in mine]
    assert names == ["trlwe_fft_keyswitch_kernel<Fft1024>", "trlwe_fft_keyswitch_kernel<Fft2048T<false, false>>", "trlwe_fft_keyswitch_kernel<Fft4096T<false>>"], names
    for r in mine:
        assert r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 512, r
    print("%d kernels in the library" % len(rows))
    assert len(rows) < 330, len(rows)


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


def _bits(t):
    """a float64 or int64 device tensor as its 64-bit patterns on the host"""
    import torch
    return t.contiguous().view(torch.int64).cpu().numpy().view(np.uint64)


def _pipeline(eng, oracle):
    """Exactly the data of tests/test_leveled_lut_tables.py::test_the_pipeline_closes (same generators in the same order): lvl2's ring and gadget, the cheap private and
    packing keys, 2 inputs x 8 bits, 8 one-bit tables -- with the oracle's words of both rounds, computed once for this module."""
    if "pipeline" in _CACHE:
        return _CACHE["pipeline"]
    import mosfhet_amd as ma
    from test_gpu_parity import _keyset, _ksk_for
    K = _keyset("lvl2", eng, oracle)
    P = K["P"]
    N, l, Bg, size, count, tables = P["N"], P["l"], P["Bg_bit"], 8, 2, 8
    oracle.plan(N)
    r = oracle.Rng(0xC105E)
    s = np.ascontiguousarray(K["rk"].s[0], dtype=np.uint64)
    lwe_s = np.ascontiguousarray(K["lk"].s, dtype=np.uint64)
    ks0, ks1 = oracle.gen_priv_ks_key(r, s, s, 20, 2, P["rlwe_sigma"])
    kskb = oracle.gen_packing1_ks_key(r, s, s, 1, 2, P["rlwe_sigma"])
    kska, pk = eng.load_trlwe_ks_keys(np.stack([ks0, ks1]), 2), eng.load_packing1_key(kskb, 2)
    ks0_dft, ks1_dft = oracle.ks_to_dft(ks0), oracle.ks_to_dft(ks1)
    ksk, _ = _ksk_for(K, eng)
    dksk = eng.load_keyswitch_key(ksk, P["base_bit"])      # (handles of this module's engine: the cached ones belong to the engine of whichever module made them first)
    rng = np.random.default_rng(0xC105E)
    m = [int(rng.integers(0, 1 << size)) for _ in range(count)]
    cts = np.stack([oracle.tlwe_sample(r, oracle.double2torus(0.25 * ((m[b] >> i) & 1)), lwe_s, P["lwe_sigma"]) for b in range(count) for i in range(size)])
    tabs = np.zeros((tables, 1, 2, N), dtype=np.uint64)
    tabs[:, 0, 1, :] = (oracle.u64(r.words(tables * N)) % np.uint64(2)).reshape(tables, N) << np.uint64(62)

    def cb(c):
        return np.stack(_map(lambda u: oracle.circuit_bootstrap_3(c[u], K["bk_dft"], ks0_dft, ks1_dft, 2, kskb, 2, l, Bg), range(len(c))))       # [bits][2l][2][N]

    def dfts(sel):
        return np.stack(_map(lambda u: oracle.bk_to_dft(sel[u].reshape(1, 2 * l, 2, N), 1, l).reshape(2 * l, 2, N), range(len(sel))))                # [bits][2l][2][N] doubles

    def luts(dft):
        d = dft.reshape(count, size, 2 * l, 2, N)
        return np.stack(_map(lambda u: _composition(oracle, tabs[u % tables], d[u // tables], N, l, Bg, size), range(count * tables))).reshape(count, tables, N + 1)

    def switch(out):
        return np.stack(_map(lambda u: oracle.tlwe_keyswitch(out.reshape(count * tables, N + 1)[u], ksk, P["n"], P["t"], P["base_bit"]), range(count * tables)))

    sel1 = cb(cts)
    dft1 = dfts(sel1)
    out1 = luts(dft1)
    ks1_ = switch(out1)
    out2 = luts(dfts(cb(ks1_)))
    ks2_ = switch(out2)
    keys = {}
    for order in ("reference", "by_component"):
        keys[order] = eng.load_bootstrap_key(K["bk"], 1, l, Bg)
        keys[order].set_product_order(order)
    D = dict(K=K, P=P, N=N, l=l, Bg=Bg, n=P["n"], size=size, count=count, tables=tables, kska=kska, pk=pk, dksk=dksk, keys=keys, ks0=ks0, cts=cts, tabs=tabs,
             d_cts=ma.to_device(cts, eng.device), d_luts=ma.to_device(tabs, eng.device), want_dft1=dft1, want_out1=out1, want_ks1=ks1_, want_out2=out2, want_ks2=ks2_)
    _CACHE["pipeline"] = D
    return D


def _two_calls(eng, key, kska, pk, d_cts):
    """the selectors as the two earlier calls make them: trgsw_to_dft(circuit_bootstrap_3(...)), [count][2l][2][N] doubles"""
    return eng.trgsw_to_dft(eng.circuit_bootstrap_3(key, kska, pk, d_cts))


def _assert_same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = [u for u in range(len(w)) if not (g[u] == w[u]).all()]
    assert not bad, "%s: %d of %d selectors differ (first: %s)" % (what, len(bad), len(w), bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 3])
def test_dft_circuit_bootstrap_matches_the_oracle_and_the_two_calls(eng, oracle, count):
    """lvl2's ring and gadget, the cheap key set of test_the_pipeline_closes, key order REFERENCE, 1 and 3 inputs (the levels switched together): every double of
    circuit_bootstrap_3_dft equals oracle.bk_to_dft(oracle.circuit_bootstrap_3(...)) and trgsw_to_dft(circuit_bootstrap_3(...)) as a 64-bit pattern."""
    import mosfhet_amd as ma
    D = _pipeline(eng, oracle)
    N, l = D["N"], D["l"]
    d_cts = D["d_cts"][:count].contiguous()
    got = eng.circuit_bootstrap_3_dft(D["keys"]["reference"], D["kska"], D["pk"], d_cts)
    assert tuple(got.shape) == (count, 2 * l, 2, N) and got.dtype == eng.torch.float64
    nat = ma.engine.slot_order_to_oracle(got.cpu().numpy().reshape(count * 2 * l * 2, N), N).reshape(count, 2 * l, 2, N)
    want = D["want_dft1"][:count]
    assert (np.ascontiguousarray(nat).view(np.uint64) == np.ascontiguousarray(want).view(np.uint64)).all(), "circuit_bootstrap_3_dft differs from the oracle"
    _assert_same_bits(got, _two_calls(eng, D["keys"]["reference"], D["kska"], D["pk"], d_cts), "%d inputs against the two calls" % count)


@pytest.mark.gpu
def test_dft_circuit_bootstrap_one_switch_per_level(eng, oracle):
    """512 inputs at lvl2's gadget -- the first count at which the levels are no longer switched together for l = 4, so the packing switch of every level lands in the
    staging block -- and 3 inputs at the N = 1024 key set, against the two earlier calls on the same inputs."""
    import mosfhet_amd as ma
    from test_gpu_parity import _keyset
    D = _pipeline(eng, oracle)
    rng = np.random.default_rng(0xB175)
    cts = rng.integers(0, 2 ** 64, size=(512, D["n"] + 1), dtype=np.uint64)
    cts[:16] = D["cts"]
    d_cts = ma.to_device(cts, eng.device)
    key = D["keys"]["reference"]
    got = eng.circuit_bootstrap_3_dft(key, D["kska"], D["pk"], d_cts)
    _assert_same_bits(got, _two_calls(eng, key, D["kska"], D["pk"], d_cts), "512 inputs at lvl2")
    del got
    K = _keyset("set1", eng, oracle)
    P = K["P"]
    r = oracle.Rng(0xB175)
    s = np.ascontiguousarray(K["rk"].s[0], dtype=np.uint64)
    ks0, ks1 = oracle.gen_priv_ks_key(r, s, s, 20, 2, P["rlwe_sigma"])
    kska, pk = eng.load_trlwe_ks_keys(np.stack([ks0, ks1]), 2), eng.load_packing1_key(oracle.gen_packing1_ks_key(r, s, s, 1, 2, P["rlwe_sigma"]), 2)
    key1 = eng.load_bootstrap_key(K["bk"], 1, P["l"], P["Bg_bit"])
    key1.set_product_order("reference")
    d_cts = ma.to_device(rng.integers(0, 2 ** 64, size=(3, P["n"] + 1), dtype=np.uint64), eng.device)
    got = eng.circuit_bootstrap_3_dft(key1, kska, pk, d_cts)
    assert tuple(got.shape) == (3, 2 * P["l"], 2, 1024)
    _assert_same_bits(got, _two_calls(eng, key1, kska, pk, d_cts), "3 inputs at N = 1024")
    for h in (kska, pk, key1):
        h.free()


@pytest.mark.gpu
def test_dft_circuit_bootstrap_by_component(eng, oracle):
    """The same key set with the product order BY_COMPONENT, 3 inputs, against the two earlier calls: the key's order governs the new call's bootstrap exactly as
    it governs circuit_bootstrap_3's -- and the words differ from the REFERENCE order's, so the comparison is not vacuous."""
    D = _pipeline(eng, oracle)
    d_cts = D["d_cts"][:3].contiguous()
    key = D["keys"]["by_component"]
    got = eng.circuit_bootstrap_3_dft(key, D["kska"], D["pk"], d_cts)
    _assert_same_bits(got, _two_calls(eng, key, D["kska"], D["pk"], d_cts), "3 inputs, BY_COMPONENT")
    assert not (_bits(got) == _bits(eng.circuit_bootstrap_3_dft(D["keys"]["reference"], D["kska"], D["pk"], d_cts))).all()


@pytest.mark.gpu
def test_lut_bits_is_the_pipeline(eng, oracle):
    """Exactly test_the_pipeline_closes' data (2 inputs x 8 bits, 8 one-bit tables, size 8): one call with the output key equals the oracle's key-switched words,
    without it the oracle's leveled_lut_tables words; a second call fed with the first call's output equals the oracle's second round; the tables are unchanged."""
    import mosfhet_amd as ma
    D = _pipeline(eng, oracle)
    key, count, size, tables, N, n = D["keys"]["reference"], D["count"], D["size"], D["tables"], D["N"], D["n"]
    d_in = D["d_cts"].view(count, size, n + 1)
    out1 = eng.lut_bits(key, D["kska"], D["pk"], D["d_luts"], d_in, ksk_out=D["dksk"])
    assert tuple(out1.shape) == (count, tables, n + 1)
    assert (ma.to_numpy(out1).reshape(count * tables, n + 1) == D["want_ks1"]).all(), "lut_bits with the output key differs from the oracle's pipeline"
    plain = eng.lut_bits(key, D["kska"], D["pk"], D["d_luts"], d_in)
    assert tuple(plain.shape) == (count, tables, N + 1)
    assert (ma.to_numpy(plain) == D["want_out1"]).all(), "lut_bits without an output key differs from the oracle's leveled_lut_tables words"
    out2 = eng.lut_bits(key, D["kska"], D["pk"], D["d_luts"], out1, ksk_out=D["dksk"])          # tables == size: the output IS the next input
    assert (ma.to_numpy(out2).reshape(count * tables, n + 1) == D["want_ks2"]).all(), "the second round differs from the oracle's"
    plain2 = eng.lut_bits(key, D["kska"], D["pk"], D["d_luts"], out1)
    assert (ma.to_numpy(plain2) == D["want_out2"]).all(), "the second round without an output key differs from the oracle's"
    assert (ma.to_numpy(D["d_luts"]) == D["tabs"]).all(), "the tables were modified"


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["reference", "by_component"])
def test_lut_bits_chunking_and_the_tree(eng, oracle, order):
    """size = 12 at N = 2048 (one tree level), 3 inputs, 2 tables: with the selector bound set so that a chunk holds 1 input, then 2 (a tail chunk of 1), then at
    the default (one chunk), the results are identical and equal the four earlier calls made one after the other on the whole batch; the plan reports the chunks."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    D = _pipeline(eng, oracle)
    key, N, l, Bg, n = D["keys"][order], D["N"], D["l"], D["Bg"], D["n"]
    size, count, tables = 12, 3, 2
    rng = np.random.default_rng(0xC4A2)
    cts = rng.integers(0, 2 ** 64, size=(count * size, n + 1), dtype=np.uint64)
    cts[:16] = D["cts"]
    tabs = rng.integers(0, 2 ** 64, size=(tables, 2, 2, N), dtype=np.uint64)                   # encrypted-looking tables: every word takes part
    d_cts, d_luts = ma.to_device(cts, eng.device), ma.to_device(tabs, eng.device)
    sel = _two_calls(eng, key, D["kska"], D["pk"], d_cts).reshape(count, size, 2 * l, 2, N)
    lut = eng.leveled_lut_tables(sel, d_luts, size, l, Bg)
    want_plain = ma.to_numpy(lut)
    want = ma.to_numpy(eng.tlwe_keyswitch(D["dksk"], lut.view(count * tables, N + 1))).reshape(count, tables, n + 1)
    per_input = size * 2 * l * 2 * N * 8
    try:
        for bound, chunk in ((per_input, 1), (2 * per_input + 5, 2), (0, 3)):
            engine.set_lut_bits_workspace(bound)
            p = eng.lut_bits_plan(N, l, size, tables, count)
            assert (p["chunk"], p["chunks"], p["cb_bits"]) == (chunk, -(-count // chunk), chunk * size), (bound, p)
            got = ma.to_numpy(eng.lut_bits(key, D["kska"], D["pk"], d_luts, d_cts.view(count, size, n + 1), ksk_out=D["dksk"]))
            assert (got == want).all(), "%s, %d inputs per chunk: differs from the four calls on the whole batch" % (order, chunk)
            got = ma.to_numpy(eng.lut_bits(key, D["kska"], D["pk"], d_luts, d_cts.view(count, size, n + 1)))
            assert (got == want_plain).all(), "%s, %d inputs per chunk, no output key: differs from the three calls on the whole batch" % (order, chunk)
    finally:
        engine.set_lut_bits_workspace(0)
    assert (ma.to_numpy(d_luts) == tabs).all(), "the tables were modified"


@pytest.mark.gpu
def test_lut_bits_key_shape_refusals(eng, oracle):
    """An output key that is a packing key, one that does not end in the bootstrap key's n, a one-entry kska and a bootstrap key at N = 4096 are refused with
    MOSFHET_HIP_EINVAL and nothing is written; at N = 4096 circuit_bootstrap_3_dft itself runs and equals the two earlier calls."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    D = _pipeline(eng, oracle)
    key, count, size, tables, N, n = D["keys"]["reference"], D["count"], D["size"], D["tables"], D["N"], D["n"]
    d_in = D["d_cts"].view(count, size, n + 1)
    out = torch.full((count, tables, N + 1), 0x5A5A5A5A, dtype=torch.int64, device=eng.device)

    with pytest.raises(engine.MosfhetHipError, match="ksk_out is a packing"):
        eng.lut_bits(key, D["kska"], D["pk"], D["d_luts"], d_in, ksk_out=D["pk"], out=out[:, :, :n + 1].contiguous())
    other = eng.load_keyswitch_key(np.zeros((N, 1, 3, n + 2), dtype=np.uint64), 2)          # N -> n + 1: not the bootstrap key's dimension
    with pytest.raises(engine.MosfhetHipError, match="ksk_out switches %d -> %d" % (N, n + 1)):
        eng.lut_bits(key, D["kska"], D["pk"], D["d_luts"], d_in, ksk_out=other, out=out[:, :, :n + 1].contiguous())
    wrong_in = eng.load_keyswitch_key(np.zeros((N // 2, 1, 3, n + 1), dtype=np.uint64), 2)  # N / 2 -> n: not from the ring's dimension
    with pytest.raises(engine.MosfhetHipError, match="ksk_out switches %d -> %d" % (N // 2, n)):
        eng.lut_bits(key, D["kska"], D["pk"], D["d_luts"], d_in, ksk_out=wrong_in, out=out[:, :, :n + 1].contiguous())
    one = eng.load_trlwe_ks_keys(D["ks0"][None], 2)
    with pytest.raises(engine.MosfhetHipError, match="kska must be the 2-entry"):
        eng.lut_bits(key, one, D["pk"], D["d_luts"], d_in, out=out)
    # a ring the LUT does not serve
    rng = np.random.default_rng(0x4096)
    N4, n4, l4, Bg4 = 4096, 4, 1, 22
    key4 = eng.load_bootstrap_key(rng.integers(0, 2 ** 64, size=(n4, 2 * l4, 2, N4), dtype=np.uint64), 1, l4, Bg4)
    key4.set_product_order("reference")
    s4 = rng.integers(0, 2, size=N4, dtype=np.uint64)
    kska4 = eng.load_trlwe_ks_keys(rng.integers(0, 2 ** 64, size=(2, 3, 2, N4), dtype=np.uint64), 4)
    pk4 = eng.generate_table_key(0, s4, s4, 1, 2, 2.0 ** -44, seed=4096, compressed=True)
    d_in4 = ma.to_device(rng.integers(0, 2 ** 64, size=(1, 3, n4 + 1), dtype=np.uint64), eng.device)
    luts4 = ma.to_device(np.zeros((1, 1, 2, N4), dtype=np.uint64), eng.device)
    with pytest.raises(engine.MosfhetHipError, match="N = 4096"):
        eng.lut_bits(key4, kska4, pk4, luts4, d_in4)
    torch.cuda.synchronize(eng.device)
    assert (out == 0x5A5A5A5A).all(), "a refused call wrote to its output"
    got = eng.circuit_bootstrap_3_dft(key4, kska4, pk4, d_in4[0])
    assert tuple(got.shape) == (3, 2 * l4, 2, N4)
    _assert_same_bits(got, _two_calls(eng, key4, kska4, pk4, d_in4[0]), "3 inputs at N = 4096")
    for h in (other, wrong_in, one, key4, kska4, pk4):
        h.free()


# Bits per input (= tables) of test_lut_bits_two_rounds_decrypt.  At 8 bits the four earlier calls themselves miss the bound in the second round: their first round
# leaves 2^59.1 of noise on an output bit, and the circuit bootstrap of the second round takes 2^59 at most (a slot of its 2l = 8-slot test vector is 1/16 of the torus
# wide).  7 is the largest size at which they meet it on this test's inputs (2^59.0 and 2^58.8): DESIGN 4.12.4 has the measured table.
DECRYPT_SIZE = 7


def _real_keys(eng):
    """BASELINE.json configs[3]'s keys: lvl2's ring and gadget, packing key t = 6, base_bit = 4 generated on the device and seed-compressed (under a fixed generator
    secret: the same key every run), private key t = 20, base_bit = 2, the LWE key of the lvl2 set"""
    if "real" not in _CACHE:
        import mosfhet_amd as ma
        from mosfhet_amd import host
        from test_gpu_parity import _ksk_for
        P = dict(ma.PARAMS_LVL2)
        N, l, Bg, n = P["N"], P["l"], P["Bg_bit"], P["n"]
        host.seed(0xB175B175)
        lk = host.LweKey(n, P["lwe_sigma"])
        rk = host.RlweKey(N, 1, P["rlwe_sigma"])
        key = eng.load_bootstrap_key(host.gen_bootstrap_key(rk, lk, l, Bg), 1, l, Bg)
        key.set_product_order("reference")
        kska = eng.load_trlwe_ks_keys(host.gen_priv_ks_key(rk, rk, 20, 2), 2)
        eng.set_keygen_secret(b"lut_bits: two rounds do decrypt!")
        pk = eng.generate_table_key(0, rk.s[0], rk.s[0], 6, 4, P["rlwe_sigma"], seed=99, compressed=True)
        _, dksk = _ksk_for(dict(P=P, lk=lk, out_key=rk.extracted_lwe_key()), eng)
        _CACHE["real"] = dict(P=P, lk=lk, key=key, kska=kska, pk=pk, dksk=dksk)
    return _CACHE["real"]


def _two_rounds(eng, oracle, size, count, new_call):
    """`count` inputs of `size` bits through `size` one-bit tables with entries in {0, 1/4}, twice: (outputs of round 1, of round 2, worst torus distance of an
    output bit's phase from f(m), from f(f(m))) -- by the four earlier calls, or by lut_bits when new_call"""
    import mosfhet_amd as ma
    from mosfhet_amd import host
    R = _real_keys(eng)
    P, key, kska, pk, dksk = R["P"], R["key"], R["kska"], R["pk"], R["dksk"]
    N, l, Bg, n, tables = P["N"], P["l"], P["Bg_bit"], P["n"], size
    rng = np.random.default_rng(0xB175B175)
    f = rng.integers(0, 2, size=(tables, N), dtype=np.uint64)                       # f(m) bit tb = f[tb][m]
    tabs = np.zeros((tables, 1, 2, N), dtype=np.uint64)
    tabs[:, 0, 1, :] = f << np.uint64(62)
    d_luts = ma.to_device(tabs, eng.device)
    m = [int(rng.integers(0, 1 << size)) for _ in range(count)]
    host.seed(0xB175 + size)
    cts = host.tlwe_samples([host.double2torus(0.25 * ((m[b] >> i) & 1)) for b in range(count) for i in range(size)], R["lk"])
    lwe_s = np.ascontiguousarray(R["lk"].s, dtype=np.uint64)

    def apply(x):
        return sum(int(f[tb][x]) << tb for tb in range(tables))

    def worst(outs, xs):
        w = 0.0
        for b in range(count):
            fx = apply(xs[b])
            for tb in range(tables):
                w = max(w, float(oracle.torus_dist(oracle.tlwe_phase(outs[b, tb], lwe_s), ((fx >> tb) & 1) << 62)))
        return w

    def four_calls(d_in):
        sel = eng.trgsw_to_dft(eng.circuit_bootstrap_3(key, kska, pk, d_in.view(count * size, n + 1))).reshape(count, size, 2 * l, 2, N)
        out = eng.leveled_lut_tables(sel, d_luts, size, l, Bg)
        return eng.tlwe_keyswitch(dksk, out.view(count * tables, N + 1)).view(count, tables, n + 1)

    def one_call(d_in):
        return eng.lut_bits(key, kska, pk, d_luts, d_in, ksk_out=dksk)

    step = one_call if new_call else four_calls
    out1 = step(ma.to_device(cts, eng.device).view(count, size, n + 1))
    out2 = step(out1)
    out1, out2 = ma.to_numpy(out1), ma.to_numpy(out2)
    return out1, out2, worst(out1, m), worst(out2, [apply(x) for x in m])


@pytest.mark.gpu
def test_lut_bits_two_rounds_decrypt(eng, oracle):
    """BASELINE.json configs[3]'s real keys (N = 2048, l = 4, Bg = 2^9, n = 632; packing key t = 6, base_bit = 4, generated on the device and seed-compressed; private
    key t = 20, base_bit = 2; the LWE key of the lvl2 set), 2 inputs x DECRYPT_SIZE bits, DECRYPT_SIZE one-bit tables with entries in {0, 1/4}.  The condition on
    the inputs, shown by the four earlier calls alone: two rounds of them decrypt to f(f(m)) within torus distance 2^61, half the message spacing of 1/4 (SURVEY
    section 4 puts one circuit-bootstrap product near 2^57.4; the rotation steps come on top).  Then lut_bits must equal that composition == at every round."""
    import torch
    free, _ = torch.cuda.mem_get_info(eng.device)
    if free < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory (3 GB packing key), %.1f GiB free" % (free / 2 ** 30))
    size, count = DECRYPT_SIZE, 2
    want1, want2, w1, w2 = _two_rounds(eng, oracle, size, count, False)
    print("four-call composition, %d bits: worst log2 torus distance from the message %.1f after one round, %.1f after two (bound 61)" % (
        size, np.log2(max(w1, 1.0)), np.log2(max(w2, 1.0))))
    assert max(w1, w2) < 2.0 ** 61, "the inputs are unfit: the four-call composition itself is 2^%.1f away from f(f(m)) (bound 2^61)" % np.log2(max(w1, w2))
    got1, got2, g1, g2 = _two_rounds(eng, oracle, size, count, True)
    print("lut_bits, %d bits: worst log2 torus distance %.1f after one round, %.1f after two" % (size, np.log2(max(g1, 1.0)), np.log2(max(g2, 1.0))))
    assert (got1 == want1).all(), "round 1 of lut_bits differs from the four-call composition"
    assert (got2 == want2).all(), "round 2 of lut_bits differs from the four-call composition"
    R = _CACHE.pop("real")
    for h in (R["key"], R["kska"], R["pk"], R["dksk"]):
        h.free()


@pytest.mark.gpu
def test_eval_LUTs_bits_through_the_host_structs(native_lib, tmp_path):
    """tests/c/lut_bits.c: mosfhet_eval_LUTs_bits on 2 inputs equals the same loop written against include/mosfhet.h (circuit_bootstrap_3, trgsw_to_DFT, the
    reference's eval_LUT on a copy of each table, tlwe_keyswitch), word for word, with and without the output key; the tables are left as they were.
    mosfhet_eval_LUTs_packed_bits gives the same words at pack_log = 0, and at pack_log = 1 on one packed table (two output bits per entry, no tree) the words of
    the same loop with the rotation masks of the packed entries and the extractions at 0 and 1."""
    exe = str(tmp_path / "lut_bits")
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "lut_bits.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and "lut_bits ok" in r.stdout, r.stdout[-3000:]
