"""Cleartext-weight linear layers on LWE batches, y = W x + bias, dense and sparse (include/mosfhet_hip.h: mosfhet_hip_linear_*, mosfhet_hip_tlwe_linear_batch,
mosfhet_hip_tlwe_linear_plan, mosfhet_hip_linear_keyswitch_functional_bootstrap_batch; mosfhet_amd/csrc/capi_linear.inc, linear_kernels.h; include/mosfhet_compat.h:
mosfhet_tlwe_linear_inputs, mosfhet_tlwe_linear_bootstrap_inputs).

Expected words come from numpy uint64 arithmetic written out here (_expected: exact mod 2^64, no matmul through the library); for the fused call from the entry
points that existed before (keyswitch_functional_bootstrap) and, on two samples, from the oracle.  Every comparison is == on all words.  The two decryption bounds
(test_a_gate_level_and_a_toy_layer_decrypt) are conditions on the inputs that the earlier entry points' composition must meet, shown with the oracle on the CPU.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NARROW_SPECIAL = [0, 1, -1, (1 << 31) - 1, -(1 << 31)]
WIDE_SPECIAL = NARROW_SPECIAL + [1 << 31, 1 << 32, (1 << 32) + 1, -(1 << 32), I64_MIN, I64_MAX]
_CACHE = {}


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_linear_symbols_and_argument_checks(native_lib):
    """The library exports the new entry points and the binding its functions; every scalar refusal of the creation calls, the compute call, the fused call and the
    plan returns MOSFHET_HIP_EINVAL with a message naming the argument and its value -- on fake pointers, before any handle is read and before any HIP call (this
    runs without a GPU); count == 0 is OK."""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_linear_create_dense", "mosfhet_hip_linear_create_sparse", "mosfhet_hip_linear_destroy", "mosfhet_hip_linear_info", "mosfhet_hip_linear_clone",
                 "mosfhet_hip_tlwe_linear_batch", "mosfhet_hip_tlwe_linear_plan", "mosfhet_hip_linear_keyswitch_functional_bootstrap_batch", "mosfhet_tlwe_linear_inputs",
                 "mosfhet_tlwe_linear_bootstrap_inputs"):
        assert hasattr(native_lib, name), name
    assert hasattr(engine, "tlwe_linear_plan")
    for name in ("linear_dense", "linear_sparse", "tlwe_linear", "linear_keyswitch_functional_bootstrap"):
        assert hasattr(engine.Engine, name), name
    for name in ("info", "close"):
        assert hasattr(engine.LinearMap, name), name
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)     # never dereferenced: every call below ends on its scalar arguments
    f = native_lib.mosfhet_hip_tlwe_linear_batch
    f.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p]
    assert f(None, fake, fake, fake, 585, 1, None) == EINVAL and "ctx" in err()
    assert f(fake, None, fake, fake, 585, 1, None) == EINVAL and "lin" in err()
    assert f(fake, fake, fake, fake, 0, 1, None) == EINVAL and "n = 0" in err()
    assert f(fake, fake, fake, fake, -7, 1, None) == EINVAL and "n = -7" in err()
    assert f(fake, fake, fake, fake, 65536, 1, None) == EINVAL and "n = 65536" in err()
    assert f(fake, fake, fake, fake, 585, -1, None) == EINVAL and "count = -1" in err()
    assert f(fake, fake, fake, fake, 585, 0, None) == 0                       # count == 0: nothing to do, no handle read
    assert f(fake, fake, None, None, 65535, 0, None) == 0
    assert f(fake, fake, fake, fake, 0, 0, None) == EINVAL and "n = 0" in err()    # ... after the scalar checks
    g = native_lib.mosfhet_hip_linear_keyswitch_functional_bootstrap_batch
    g.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    assert g(None, fake, fake, fake, fake, fake, 1, fake, 1, 4, 1, None) == EINVAL and "ctx" in err()
    assert g(fake, None, fake, fake, fake, fake, 1, fake, 1, 4, 1, None) == EINVAL and "lin" in err()
    assert g(fake, fake, None, fake, fake, fake, 1, fake, 1, 4, 1, None) == EINVAL and "ksk" in err()
    assert g(fake, fake, fake, None, fake, fake, 1, fake, 1, 4, 1, None) == EINVAL and "bsk" in err()
    assert g(fake, fake, fake, fake, fake, fake, 1, fake, -1, 4, 1, None) == EINVAL and "count = -1" in err()
    assert g(fake, fake, fake, fake, fake, fake, 1, fake, 0, 4, 1, None) == 0
    d = native_lib.mosfhet_hip_linear_create_dense
    d.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int]
    out = C.c_void_p()
    assert d(None, C.byref(out), fake, None, 2, 2) == EINVAL and "ctx" in err()
    assert d(fake, None, fake, None, 2, 2) == EINVAL and "out" in err()
    assert d(fake, C.byref(out), fake, None, 0, 2) == EINVAL and "rows_out = 0" in err()
    assert d(fake, C.byref(out), fake, None, 2, -1) == EINVAL and "rows_in = -1" in err()
    assert d(fake, C.byref(out), None, None, 2, 2) == EINVAL and "h_W" in err()
    s = native_lib.mosfhet_hip_linear_create_sparse
    s.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int]
    ints = lambda *v: (C.c_int * len(v))(*v)
    vals = (C.c_longlong * 4)(1, 1, 1, 1)
    assert s(None, C.byref(out), ints(0, 1), ints(0), vals, None, 1, 1) == EINVAL and "ctx" in err()
    assert s(fake, C.byref(out), ints(0, 1), ints(0), vals, None, 0, 1) == EINVAL and "rows_out = 0" in err()
    assert s(fake, C.byref(out), ints(0, 1), ints(0), vals, None, 1, 0) == EINVAL and "rows_in = 0" in err()
    assert s(fake, C.byref(out), None, ints(0), vals, None, 1, 1) == EINVAL and "h_row_ptr" in err()
    assert s(fake, C.byref(out), ints(1, 2), ints(0, 0), vals, None, 1, 1) == EINVAL and "row_ptr[0] = 1" in err()
    assert s(fake, C.byref(out), ints(0, 2, 1), ints(0, 0), vals, None, 2, 1) == EINVAL and "row_ptr[2] = 1" in err()      # not monotone
    assert s(fake, C.byref(out), ints(0, 2), ints(0, 3), vals, None, 1, 3) == EINVAL and "col[1] = 3" in err()           # out of range
    assert s(fake, C.byref(out), ints(0, 2), ints(0, -1), vals, None, 1, 3) == EINVAL and "col[1] = -1" in err()
    assert out.value is None                                                                                           # nothing was created
    i = native_lib.mosfhet_hip_linear_info
    i.argtypes = [C.c_void_p, C.c_void_p]
    assert i(None, (C.c_longlong * 6)()) == EINVAL and "lin" in err()
    p = native_lib.mosfhet_hip_tlwe_linear_plan
    p.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    plan = (C.c_longlong * 8)()
    assert p(8, 8, -1, 1, 585, 1, 256, None) == EINVAL and "plan" in err()
    assert p(0, 8, -1, 1, 585, 1, 256, plan) == EINVAL and "rows_out = 0" in err()
    assert p(8, 0, -1, 1, 585, 1, 256, plan) == EINVAL and "rows_in = 0" in err()
    assert p(8, 8, -2, 1, 585, 1, 256, plan) == EINVAL and "nnz = -2" in err()
    assert p(8, 8, -1, 2, 585, 1, 256, plan) == EINVAL and "narrow = 2" in err()
    assert p(8, 8, -1, 1, 0, 1, 256, plan) == EINVAL and "n = 0" in err()
    assert p(8, 8, -1, 1, 65536, 1, 256, plan) == EINVAL and "n = 65536" in err()
    assert p(8, 8, -1, 1, 585, -1, 256, plan) == EINVAL and "count = -1" in err()
    assert p(8, 8, -1, 1, 585, 1, 0, plan) == EINVAL and "cus = 0" in err()
    assert p(8, 8, -1, 1, 585, 0, 256, plan) == 0 and plan[3] == 0                # count == 0: an empty launch
    assert p(8, 2 ** 31 - 1, -1, 1, 65535, 70000, 256, plan) == EINVAL and "rows_in = 2147483647" in err()      # the byte model would pass 2^63
    c = native_lib.mosfhet_hip_linear_clone
    c.argtypes = [C.c_void_p] * 3
    assert c(None, fake, C.byref(out)) == EINVAL and "ctx_other" in err()
    assert c(fake, None, C.byref(out)) == EINVAL and "lin" in err()
    assert c(fake, fake, None) == EINVAL and "out" in err()
    assert p(8, 8, -1, 1, 585, 1, 256, plan) == 0


def test_linear_plan_is_a_pure_function(native_lib):
    """mosfhet_hip_tlwe_linear_plan -- the function the launcher decides with -- over the issue's sweep, both forms, both multiply sequences: a unit is one wavefront
    = 64 * words_per_lane word columns x TJ rows of one batch element, four units per workgroup; the strips cover the n + 1 words and the tiles the rows exactly once
    (no empty strip or tile, no empty workgroup, no empty grid row); gridDim.x <= 2^31 - 1 and gridDim.y <= 65535; passes == ceil(rows_out / TJ); the byte model;
    nothing but grid sizes depends on cus; the same arguments give the same plan.  A call of more than 2^31 - 1 units is refused naming count."""
    from mosfhet_amd import engine
    TJ = engine.tlwe_linear_plan(1, 1, 1, 1)["tj"]
    assert TJ >= 2
    checked = refused = 0
    for rows_out in (1, TJ - 1, TJ, TJ + 1, 128, 1000):
        for rows_in in (1, 3, 784):
            for n in (1, 585, 1024, 2048, 49152):
                for count in (1, 3, 4096, 70000):
                    for nnz in (-1, 2 * rows_out):
                        for narrow in (True, False):
                            args = (rows_out, rows_in, n, count)
                            w = n + 1
                            if count * -(-w // 64) * -(-rows_out // TJ) > 2 ** 31 - 1:
                                with pytest.raises(engine.MosfhetHipError, match="count = %d" % count):
                                    engine.tlwe_linear_plan(*args, nnz=nnz, narrow=narrow)
                                refused += 1
                                continue
                            p = engine.tlwe_linear_plan(*args, nnz=nnz, narrow=narrow, cus=256)
                            what = (args, nnz, narrow, p)
                            assert p["form"] == ("dense" if nnz < 0 else "sparse") and p["multiply"] == ("narrow" if narrow else "wide") and p["tj"] == TJ, what
                            lanes = 64 * p["words_per_lane"]
                            strips, tiles = -(-w // lanes), -(-rows_out // TJ)
                            assert (strips - 1) * lanes < w <= strips * lanes and (tiles - 1) * TJ < rows_out <= tiles * TJ, what
                            units = count * strips * tiles
                            assert (p["workgroups"] - 1) * 4 < units <= p["workgroups"] * 4, what
                            gy = p["grid_folds"]
                            gx = -(-p["workgroups"] // gy)
                            assert 1 <= gy <= 65535 and 1 <= gx <= 2 ** 31 - 1 and (gy - 1) * gx < p["workgroups"] <= gx * gy, what
                            assert p["passes"] == tiles and p["input_bytes"] == tiles * count * rows_in * w * 8, what
                            q = engine.tlwe_linear_plan(*args, nnz=nnz, narrow=narrow, cus=64)
                            assert {k: v for k, v in q.items() if k not in ("workgroups", "grid_folds")} == {k: v for k, v in p.items() if k not in ("workgroups", "grid_folds")}, what
                            assert p == engine.tlwe_linear_plan(*args, nnz=nnz, narrow=narrow, cus=256), what
                            checked += 1
    assert checked > 1000 and refused > 0, (checked, refused)
    assert engine.tlwe_linear_plan(1, 1, 1, 70000)["grid_folds"] > 1            # the batch of test_linear_folded_grid does fold


def test_linear_kernels_of_the_build(native_lib):
    """tools/kernel_table.py lists the new kernel -- one instantiation -- without scratch and within 256 registers (two wavefronts per SIMD at least); the library
    still holds fewer than 330 kernels (words_sub_kernel went: its one launch site runs words_add2_kernel); tools/check_lds_barriers.py found nothing on the build."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    rows = kernel_table.table()
    mine = [r for r in rows if r["name"].startswith("tlwe_linear_kernel")]
    for r in mine:
        print("%-40s vgpr %3d  agpr %3d  sgpr %3d  lds %6d  scratch %4d" % (r["name"], r["vgpr"], r["agpr"], r["sgpr"], r["lds"], r["scratch"]))
    assert len(mine) == 1, [r["name"] for r in mine]
    for r in mine:
        assert r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 256, r
    assert not [r["name"] for r in rows if r["name"].startswith("words_sub_kernel")]
    print("%d kernels in the library" % len(rows))
    assert len(rows) < 330, len(rows)
    with open(os.path.join(ROOT, "mosfhet_amd", "build", "lds_barrier_check.txt")) as fh:
        report = fh.read()
    print(report)
    assert ", 0 violations" in report, report


def _compile_c(tmp_path):
    exe = str(tmp_path / "tlwe_linear")
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "tlwe_linear.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_linear_c_program_compiles_and_links(native_lib, tmp_path):
    """tests/c/tlwe_linear.c compiles against include/mosfhet.h and links against the built library (its device part: test_linear_host_face)."""
    assert os.path.exists(_compile_c(tmp_path))


# ---------------------------------------------------------------- expected words ----------------------------------------------------------------
def _expected(row_ptr, col, val, bias, x):
    """out[b][j][c] = (c == n ? bias[j] : 0) + sum_q val[q] x[b][col[q]][c] over row j's entries, in numpy uint64 arithmetic (wraps mod 2^64)"""
    count, _, w = x.shape
    rows_out = len(row_ptr) - 1
    out = np.zeros((count, rows_out, w), dtype=np.uint64)
    col, valu = np.asarray(col, dtype=np.int64), np.asarray(val, dtype=np.int64).view(np.uint64)
    with np.errstate(over="ignore"):
        for j in range(rows_out):
            lo, hi = int(row_ptr[j]), int(row_ptr[j + 1])
            if hi > lo:
                out[:, j, :] = (x[:, col[lo:hi], :] * valu[None, lo:hi, None]).sum(axis=1, dtype=np.uint64)
        if bias is not None:
            out[:, :, w - 1] += np.asarray(bias, dtype=np.uint64)[None, :]
    return out


def _csr_of_dense(W):
    rows_out, rows_in = W.shape
    return np.arange(rows_out + 1, dtype=np.int32) * rows_in, np.tile(np.arange(rows_in, dtype=np.int32), rows_out), W.reshape(-1)


def _inputs(n, count, rows_in):
    """uniform random words, plus a row of all-ones, one of 2^32 - 1 and one of 2^32 (interleaved in the one row when rows_in == 1); made once per shape and left unchanged"""
    key = ("x", n, count, rows_in)
    if key not in _CACHE:
        rng = np.random.default_rng([0x11EA, n, count, rows_in])
        x = rng.integers(0, 2 ** 64, size=(count, rows_in, n + 1), dtype=np.uint64)
        special = [ONES, np.uint64((1 << 32) - 1), np.uint64(1 << 32)]
        if rows_in >= 3:
            for i, v in enumerate(special):
                x[0, i, :] = v
        else:
            for i, v in enumerate(special):
                x[0, 0, i::4] = v
        _CACHE[key] = x
    return _CACHE[key]


def _matrices(rows_out, rows_in):
    """three matrices per shape: narrow (0, +-1, 2^31 - 1, -2^31, random 32-bit), the same with one 2^31 (the first wide weight: the other sequence runs on the same
    numbers) and wide (+-2^32, 2^32 + 1, INT64_MIN, INT64_MAX, random 64-bit)"""
    rng = np.random.default_rng([0x3A7, rows_out, rows_in])
    size = rows_out * rows_in
    narrow = rng.integers(-(1 << 31), 1 << 31, size=size, dtype=np.int64)
    wide = rng.integers(I64_MIN, I64_MAX, size=size, dtype=np.int64, endpoint=True)
    for k, v in enumerate(NARROW_SPECIAL):
        narrow[(k * 7) % size] = v
    for k, v in enumerate(WIDE_SPECIAL):
        wide[(k * 7) % size] = v
    edge = narrow.copy()
    edge[size // 2] = 1 << 31
    return [("narrow", narrow.reshape(rows_out, rows_in), True), ("2^31", edge.reshape(rows_out, rows_in), False), ("wide", wide.reshape(rows_out, rows_in), False)]


def _bias(rows_out):
    b = np.random.default_rng([0xB1A5, rows_out]).integers(0, 2 ** 64, size=rows_out, dtype=np.uint64)
    b[0] = ONES
    return b


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


def _run(eng, lin, x):
    import mosfhet_amd as ma
    return ma.to_numpy(eng.tlwe_linear(lin, ma.to_device(x, eng.device)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 585, 1024, 2048])
def test_linear_dense_exact(eng, n):
    """Shapes (1, 1), (TJ - 1, 3), (TJ + 1, 5), (2 TJ + 3, 17) (one ragged tile, two, three), count 1 and 3, n + 1 words (a single lane, ragged last strips), the three
    matrices of _matrices, with and without bias: every word == numpy; the bias lands on word n only (the two results differ there and nowhere else)."""
    from mosfhet_amd import engine
    TJ = engine.tlwe_linear_plan(1, 1, 1, 1)["tj"]
    for rows_out, rows_in in ((1, 1), (TJ - 1, 3), (TJ + 1, 5), (2 * TJ + 3, 17)):
        bias = _bias(rows_out)
        for name, W, narrow in _matrices(rows_out, rows_in):
            plain, biased = eng.linear_dense(W), eng.linear_dense(W, bias)
            info = plain.info()
            assert (info["rows_out"], info["rows_in"], info["nnz"], info["narrow"], info["form"]) == (rows_out, rows_in, -1, narrow, "dense"), (name, info)
            assert info["nbytes"] >= W.size * 8
            for count in (1, 3):
                x = _inputs(n, count, rows_in)
                csr = _csr_of_dense(W)
                want, got = _expected(*csr, None, x), _run(eng, plain, x)
                assert got.shape == want.shape and (got == want).all(), "dense %s %dx%d n=%d count=%d: %d words differ" % (name, rows_out, rows_in, n, count, (got != want).sum())
                want_b, got_b = _expected(*csr, bias, x), _run(eng, biased, x)
                assert (got_b == want_b).all(), "dense %s %dx%d n=%d count=%d with bias: %d words differ" % (name, rows_out, rows_in, n, count, (got_b != want_b).sum())
                assert (got_b[:, :, :n] == got[:, :, :n]).all() and (got_b[:, :, n] - got[:, :, n] == bias[None, :]).all()
            plain.close()
            biased.close()


def _sparse_cases(TJ):
    """(name, row_ptr, col, val, rows_in): an empty row / a row listing every column / repeated and unsorted columns (one row of 5000 entries: more staging rows than a
    second-level list is cut at) / the skewed matrix (one row listing all 600 columns, the rest fan-in 2) / an all-empty matrix"""
    rng = np.random.default_rng(0x5BA25E)
    cases = []

    def build(rows, rows_in, name):
        ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
        col = np.array([c for r in rows for c, _ in r], dtype=np.int32)
        val = np.array([v for r in rows for _, v in r], dtype=np.int64)
        cases.append((name, ptr, col, val, rows_in))

    def weight(wide):
        return int(rng.integers(I64_MIN, I64_MAX, endpoint=True)) if wide else int(rng.integers(-(1 << 31), 1 << 31))

    for wide in (False, True):
        tag = "wide" if wide else "narrow"
        special = WIDE_SPECIAL if wide else NARROW_SPECIAL
        rows = [[], [(i, special[i % len(special)]) for i in range(17)], [(3, weight(wide)), (3, weight(wide)), (16, 1), (0, -1), (3, special[-1])], [],
                [(i, weight(wide)) for i in reversed(range(17))]] + [[(int(rng.integers(0, 17)), weight(wide)) for _ in range(k)] for k in range(2 * TJ)]
        build(rows, 17, "kinds " + tag)
        skew = [[(i, weight(wide)) for i in rng.permutation(600)]] + [[(int(rng.integers(0, 600)), 1), (int(rng.integers(0, 600)), -1)] for _ in range(2 * TJ + 2)]
        build(skew, 600, "skewed " + tag)
    build([[(int(rng.integers(0, 5)), weight(False)) for _ in range(5000)], [(1, 1)], [(c % 5, weight(True)) for c in range(65)], [(c % 5, 2) for c in range(64)]], 5, "long rows")
    build([[], [], []], 4, "all empty")
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 585, 1024, 2048])
def test_linear_sparse_exact(eng, n):
    """The row kinds of _sparse_cases on the inputs of the dense test, count 1 and 3, with and without bias: every word == numpy (an empty row is its bias alone);
    the sparse handle of a dense matrix gives the dense handle's words."""
    from mosfhet_amd import engine
    TJ = engine.tlwe_linear_plan(1, 1, 1, 1)["tj"]
    for name, ptr, col, val, rows_in in _sparse_cases(TJ):
        rows_out = len(ptr) - 1
        bias = _bias(rows_out)
        plain, biased = eng.linear_sparse(ptr, col, val, rows_in), eng.linear_sparse(ptr, col, val, rows_in, bias)
        info = plain.info()
        narrow = bool(len(val) == 0 or (val.min() >= -(1 << 31) and val.max() < (1 << 31)))
        assert (info["rows_out"], info["rows_in"], info["nnz"], info["narrow"], info["form"]) == (rows_out, rows_in, len(val), narrow, "sparse"), (name, info)
        for count in (1, 3):
            x = _inputs(n, count, rows_in)
            want, got = _expected(ptr, col, val, None, x), _run(eng, plain, x)
            assert (got == want).all(), "sparse %s n=%d count=%d: %d words differ, rows %s" % (name, n, count, (got != want).sum(), sorted(set(np.nonzero(got != want)[1]))[:8])
            want_b, got_b = _expected(ptr, col, val, bias, x), _run(eng, biased, x)
            assert (got_b == want_b).all(), "sparse %s n=%d count=%d with bias: %d words differ" % (name, n, count, (got_b != want_b).sum())
        plain.close()
        biased.close()
    for name, W, _ in _matrices(2 * TJ + 3, 17):
        dense, sparse = eng.linear_dense(W, _bias(2 * TJ + 3)), eng.linear_sparse(*_csr_of_dense(W), 17, _bias(2 * TJ + 3))
        x = _inputs(n, 3, 17)
        assert (_run(eng, sparse, x) == _run(eng, dense, x)).all(), "the sparse handle of the dense %s matrix differs from the dense handle" % name
        dense.close()
        sparse.close()


@pytest.mark.gpu
def test_linear_narrow_and_wide_agree(eng):
    """A narrow matrix, and the same matrix with one wide weight (2^40) in a column whose input row is zero: the handle turns wide (info), every word stays -- the
    two multiply sequences give the same low 64 bits on the same numbers; dense and sparse."""
    from mosfhet_amd import engine
    TJ = engine.tlwe_linear_plan(1, 1, 1, 1)["tj"]
    rows_out, rows_in, n = TJ + 1, 5, 585
    W = _matrices(rows_out, rows_in)[0][1].copy()
    W[:, 4] = 0
    W2 = W.copy()
    W2[1, 4] = 1 << 40
    x = _inputs(n, 3, rows_in).copy()
    x[:, 4, :] = 0
    want = _expected(*_csr_of_dense(W), None, x)
    for make in (eng.linear_dense, lambda M: eng.linear_sparse(*_csr_of_dense(M), rows_in)):
        a, b = make(W), make(W2)
        assert a.info()["narrow"] is True and b.info()["narrow"] is False
        got_a, got_b = _run(eng, a, x), _run(eng, b, x)
        assert (got_a == want).all() and (got_b == want).all()
        a.close()
        b.close()


@pytest.mark.gpu
def test_linear_folded_grid(eng):
    """count = 70000 at 1 x 1 and n = 1 (about 1 MB): the workgroup index is folded over two grid dimensions (the plan says so) and unfolded by the kernel; exact."""
    from mosfhet_amd import engine
    count, n = 70000, 1
    assert engine.tlwe_linear_plan(1, 1, n, count)["grid_folds"] > 1
    x = np.random.default_rng(70000).integers(0, 2 ** 64, size=(count, 1, n + 1), dtype=np.uint64)
    for wt in (-3, (1 << 40) + 1):
        W, bias = np.array([[wt]], dtype=np.int64), np.array([5], dtype=np.uint64)
        for lin in (eng.linear_dense(W, bias), eng.linear_sparse([0, 1], [0], [wt], 1, bias)):
            got = _run(eng, lin, x)
            assert (got == _expected([0, 1], [0], [wt], bias, x)).all(), "weight %d: %d of %d words differ" % (wt, (got != _expected([0, 1], [0], [wt], bias, x)).sum(), got.size)
            lin.close()


@pytest.mark.gpu
def test_linear_refusals_on_the_device(eng):
    """d_out overlapping d_in (byte ranges: the same buffer, and a partial overlap) and a handle made for another context are refused with MOSFHET_HIP_EINVAL, and
    nothing is written; the handle's clone for that context works there."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    W = np.array([[1, -1], [2, 3]], dtype=np.int64)
    lin = eng.linear_dense(W)
    x = _inputs(585, 1, 2)
    buf = torch.zeros(3 * 2 * 586, dtype=torch.int64, device=eng.device)
    buf[:2 * 586] = ma.to_device(x, eng.device).view(-1)
    before = buf.clone()
    d_in = buf[:2 * 586].view(1, 2, 586)
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.tlwe_linear(lin, d_in, out=d_in)
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.tlwe_linear(lin, d_in, out=buf[2 * 586 - 1:4 * 586 - 1].view(1, 2, 586))
    got = eng.tlwe_linear(lin, d_in, out=buf[2 * 586:4 * 586].view(1, 2, 586))              # adjacent: fine
    assert (ma.to_numpy(got) == _expected(*_csr_of_dense(W), None, x)).all()
    buf.copy_(before)
    other = ma.Engine(0)
    try:
        with pytest.raises(engine.MosfhetHipError, match="another context"):
            other.tlwe_linear(lin, d_in, out=buf[2 * 586:4 * 586].view(1, 2, 586))
        torch.cuda.synchronize(eng.device)
        assert (buf == before).all(), "a refused call wrote to its output"
        mine = other.clone_linear(lin)
        assert mine.info() == lin.info()
        assert (ma.to_numpy(other.tlwe_linear(mine, d_in)) == _expected(*_csr_of_dense(W), None, x)).all()
        mine.close()
    finally:
        other.close()
    lin.close()


def _keys(eng, oracle, name, order=None):
    """A key set of tests/test_gpu_parity.py (same generators, cached host keys) with device handles of THIS module's engine (the cached handles belong to the engine
    of whichever module made them first): dict(K, P, ksk, dksk, bsk)"""
    key = ("keys", name, order)
    if key not in _CACHE:
        from mosfhet_amd import host
        from test_gpu_parity import _keyset
        K = _keyset(name, eng, oracle)
        P = K["P"]
        if "ksk" not in K:
            K["ksk"] = host.gen_tlwe_ks_key(K["lk"], K["out_key"], P["t"], P["base_bit"])
        bsk = eng.load_bootstrap_key(K["bk"], 1, P["l"], P["Bg_bit"])
        if order:
            bsk.set_product_order(order)
        _CACHE[key] = dict(K=K, P=P, ksk=K["ksk"], dksk=eng.load_keyswitch_key(K["ksk"], P["base_bit"]), bsk=bsk)
    return _CACHE[key]


def _fused_case(eng, oracle, name, order):
    """rows_in = 3, rows_out = 2, count = 2 at key set `name`: both extract values, tv_count 1 and count * rows_out, against numpy-linear followed by the existing
    keyswitch_functional_bootstrap; two samples against the oracle's tlwe_keyswitch + functional_bootstrap"""
    import mosfhet_amd as ma
    from mosfhet_amd import host
    D = _keys(eng, oracle, name, order)
    K, P, ksk, dksk, bsk = D["K"], D["P"], D["ksk"], D["dksk"], D["bsk"]
    N = P["N"]
    rng = np.random.default_rng(0xF05ED)
    count, rows_in, rows_out = 2, 3, 2
    x = rng.integers(0, 2 ** 64, size=(count, rows_in, N + 1), dtype=np.uint64)
    W = np.array([[1, -1, 2], [-(1 << 31), 3, (1 << 33) + 1]], dtype=np.int64)
    bias = rng.integers(0, 2 ** 64, size=rows_out, dtype=np.uint64)
    y = _expected(*_csr_of_dense(W), bias, x).reshape(count * rows_out, N + 1)
    tvs = np.stack([host.torus_packing(rng.integers(0, 2 ** 64, size=4, dtype=np.uint64), 1, N) for _ in range(count * rows_out)])
    d_x, d_y = ma.to_device(x, eng.device), ma.to_device(y, eng.device)
    for make in (lambda: eng.linear_dense(W, bias), lambda: eng.linear_sparse(*_csr_of_dense(W), rows_in, bias)):
        lin = make()
        for tv in (tvs[:1], tvs):
            d_tv = ma.to_device(tv, eng.device)
            for extract in (True, False):
                want = ma.to_numpy(eng.keyswitch_functional_bootstrap(dksk, bsk, d_tv, d_y, 4, extract=extract))
                got = ma.to_numpy(eng.linear_keyswitch_functional_bootstrap(lin, dksk, bsk, d_tv, d_x, 4, extract=extract))
                assert got.shape[:2] == (count, rows_out) and (got.reshape(want.shape) == want).all(), (name, len(tv), extract)
            for u in (0, 3):          # (the last pass was extract = False: extraction at 0 of the oracle's accumulator is its functional_bootstrap)
                sw = oracle.tlwe_keyswitch(y[u], ksk, P["n"], P["t"], P["base_bit"])
                ref = oracle.functional_bootstrap(tv[u % len(tv)], sw, K["bk_dft"], P["l"], P["Bg_bit"], 4)
                full = ma.to_numpy(eng.linear_keyswitch_functional_bootstrap(lin, dksk, bsk, d_tv, d_x, 4)).reshape(count * rows_out, N + 1)
                assert (full[u] == ref).all(), (name, "oracle", u)
        lin.close()


@pytest.mark.gpu
def test_linear_fused_call_equals_the_composition(eng, oracle):
    """SET_1 keys as the gate tests make them, and once lvl2 with the key's product order set to REFERENCE (the oracle's order at every batch size)."""
    _fused_case(eng, oracle, "set1", None)
    _fused_case(eng, oracle, "lvl2", "reference")


# Half the spacing of the messages of both circuits below: slots of 1/8 at torus_base 4.  What the composition of the earlier entry points leaves of it at SET_1 is
# printed by the test: the key switch of SET_1 (t = 5, base_bit = 2: 10 bits of every mask word) alone leaves a rounding error of about 2^56.7.
HALF_SLOT = 2.0 ** 60


@pytest.mark.gpu
def test_a_gate_level_and_a_toy_layer_decrypt(eng, oracle):
    """SET_1.  Gate level: bits as 0 / 1/8, one LUT T = [0, 0, 1/8, 1/8] (x >= 2) at torus_base 4, four fan-in-2 gates as +-1 weights and a constant in the bias --
    AND = T(a + b), OR = T(a + b + 1), a AND NOT b = T(a - b + 1), NOR = T(-a - b + 2) -- over 4 instances of 3 bits (a sparse level).  Toy layer: 4 -> 3 dense,
    weights in [-2, 2] with an odd sum of magnitudes per row, inputs +-1/16, bias -1/16 (the LUT's slots are centred on m / 8, so the sign changes at -1/16), a
    constant LUT 1/16: out = sign(W x) / 16, the inputs' encoding.  The condition, shown on the CPU with the oracle first: numpy-linear + oracle.tlwe_keyswitch
    lands within HALF_SLOT of the slot centre it should (the margin left is printed), and oracle.functional_bootstrap of that decrypts to the cleartext evaluation.
    Then the fused call on the device decrypts to the same."""
    import mosfhet_amd as ma
    from mosfhet_amd import host
    D = _keys(eng, oracle, "set1")
    K, P, ksk, dksk, bsk = D["K"], D["P"], D["ksk"], D["dksk"], D["bsk"]
    N = P["N"]
    lwe_s, out_s = np.ascontiguousarray(K["lk"].s, dtype=np.uint64), np.ascontiguousarray(K["out_key"].s, dtype=np.uint64)
    t = lambda v: np.uint64(host.double2torus(v))
    eighth = 1 << 61
    rng = np.random.default_rng(0x6A7E)

    def check(what, lin, W_csr, bias, x, tv, slots, outs):
        """slots[b][j]: the slot (in eighths, possibly negative) the bootstrap input must fall into; outs[b][j]: the torus word the output decrypts to"""
        count, rows_out = slots.shape
        y = _expected(*W_csr, bias, x).reshape(count * rows_out, N + 1)
        worst_in = worst_out = 0.0
        for u in range(count * rows_out):
            sw = oracle.tlwe_keyswitch(y[u], ksk, P["n"], P["t"], P["base_bit"])
            centre = np.uint64((int(slots.reshape(-1)[u]) * eighth) % 2 ** 64)
            worst_in = max(worst_in, float(oracle.torus_dist(oracle.tlwe_phase(sw, lwe_s), centre)))
            ref = oracle.functional_bootstrap(tv, sw, K["bk_dft"], P["l"], P["Bg_bit"], 4)
            worst_out = max(worst_out, float(oracle.torus_dist(oracle.tlwe_phase(ref, out_s), outs.reshape(-1)[u])))
        print("%s: the earlier entry points' composition is 2^%.1f from the slot centre in front of the bootstrap (half a slot 2^60: margin 2^%.1f) and 2^%.1f from the "
              "result behind it" % (what, np.log2(max(worst_in, 1.0)), np.log2(max(HALF_SLOT - worst_in, 1.0)), np.log2(max(worst_out, 1.0))))
        assert worst_in < HALF_SLOT and worst_out < HALF_SLOT, "%s: the inputs are unfit, the composition of the earlier entry points itself does not decrypt" % what
        got = ma.to_numpy(eng.linear_keyswitch_functional_bootstrap(lin, dksk, bsk, ma.to_device(tv[None], eng.device), ma.to_device(x, eng.device), 4))
        ph = host.tlwe_phase(got.reshape(count * rows_out, N + 1), out_s)
        dist = oracle.torus_dist(ph, outs.reshape(-1))
        assert dist.max() < HALF_SLOT, "%s: %d of %d outputs of the fused call do not decrypt" % (what, (dist >= HALF_SLOT).sum(), dist.size)

    # the gate level
    gates = [("and", 0, 1, 1, 1, 0), ("or", 1, 2, 1, 1, 1), ("andnot", 0, 2, 1, -1, 1), ("nor", 2, 1, -1, -1, 2)]        # name, input a, input b, weight a, weight b, constant
    bits = rng.integers(0, 2, size=(4, 3))
    bits[0] = (0, 0, 0)
    bits[1] = (1, 1, 1)
    x = host.tlwe_samples([int(v) * eighth for v in bits.reshape(-1)], K["out_key"]).reshape(4, 3, N + 1)
    ptr, col, val = np.arange(5, dtype=np.int32) * 2, np.array([c for g in gates for c in g[1:3]], dtype=np.int32), np.array([w for g in gates for w in g[3:5]], dtype=np.int64)
    bias = np.array([g[5] * eighth for g in gates], dtype=np.uint64)
    sums = np.array([[g[3] * b[g[1]] + g[4] * b[g[2]] + g[5] for g in gates] for b in bits])
    assert sums.min() >= 0 and sums.max() <= 3
    tv = host.torus_packing(np.array([0, 0, eighth, eighth], dtype=np.uint64), 1, N)
    lin = eng.linear_sparse(ptr, col, val, 3, bias)
    check("gate level", lin, (ptr, col, val), bias, x, tv, sums, (sums >= 2).astype(np.uint64) * np.uint64(eighth))
    lin.close()

    # the toy layer
    W = np.array([[2, -1, 1, -1], [1, 1, -1, 0], [-2, 1, 0, 2]], dtype=np.int64)
    assert (np.abs(W).sum(axis=1) % 2 == 1).all() and np.abs(W).max() <= 2
    signs = rng.integers(0, 2, size=(4, 4)) * 2 - 1
    signs[0] = (1, 1, 1, 1)
    signs[1] = (-1, 1, -1, 1)
    x = host.tlwe_samples([int(t(v / 16.0)) for v in signs.reshape(-1)], K["out_key"]).reshape(4, 4, N + 1)
    bias = np.full(3, t(-1 / 16.0), dtype=np.uint64)
    s = signs @ W.T                                          # odd, |s| <= 5: s / 16 - 1 / 16 is the centre of slot (s - 1) / 2, slots 0 .. 2 for s > 0, -1 .. -3 for s < 0
    assert (s % 2 != 0).all() and np.abs(s).max() <= 5
    tv = host.torus_packing(np.full(4, t(1 / 16.0), dtype=np.uint64), 1, N)
    lin = eng.linear_dense(W, bias)
    check("toy layer", lin, _csr_of_dense(W), bias, x, tv, (s - 1) // 2, np.where(s > 0, t(1 / 16.0), t(-1 / 16.0)).astype(np.uint64))
    lin.close()


@pytest.mark.gpu
def test_linear_calls_are_captured_in_a_graph(eng, oracle):
    """The linear call (dense, and sparse with a cut row: two launches and the staging rows of the pool) and the fused call, each captured on one side stream after an
    eager call of the same size, replayed on fresh inputs: the replayed words == the plain call's -- no hidden allocation or synchronisation.  One stream, no parallel
    branches."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import host
    D = _keys(eng, oracle, "set1")
    P, dksk, bsk = D["P"], D["dksk"], D["bsk"]
    N = P["N"]
    rng = np.random.default_rng(0xCA97)
    W = rng.integers(-4, 5, size=(3, 70), dtype=np.int64)
    dense, sparse = eng.linear_dense(W), eng.linear_sparse(*_csr_of_dense(W), 70)          # rows of 70 entries: cut into two chunks each
    d_tv = ma.to_device(host.torus_packing(rng.integers(0, 2 ** 64, size=4, dtype=np.uint64), 1, N)[None], eng.device)
    xs = [ma.to_device(rng.integers(0, 2 ** 64, size=(2, 70, N + 1), dtype=np.uint64), eng.device) for _ in range(2)]
    calls = [("dense", lambda i, o: eng.tlwe_linear(dense, i, out=o), (2, 3, N + 1)), ("sparse", lambda i, o: eng.tlwe_linear(sparse, i, out=o), (2, 3, N + 1)),
             ("fused", lambda i, o: eng.linear_keyswitch_functional_bootstrap(dense, dksk, bsk, d_tv, i, 4, out=o), (2, 3, N + 1))]
    side = torch.cuda.Stream(device=eng.device)
    for name, call, shape in calls:
        eager = [ma.to_numpy(call(x, eng.empty(*shape))) for x in xs]
        d_in, d_out = xs[0].clone(), eng.empty(*shape)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call(d_in, d_out)
        for r in (1, 0):
            d_in.copy_(xs[r])
            d_out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert (ma.to_numpy(d_out) == eager[r]).all(), "%s: replay on inputs %d differs from the plain call" % (name, r)
        del g
    dense.close()
    sparse.close()


@pytest.mark.gpu
def test_linear_host_face(native_lib, tmp_path):
    """tests/c/tlwe_linear.c: mosfhet_tlwe_linear_inputs on host structs equals a loop of tlwe_scale_addto written in the program, word for word, with and without
    bias; mosfhet_tlwe_linear_bootstrap_inputs equals that loop followed by tlwe_keyswitch and functional_bootstrap, and decrypts."""
    r = subprocess.run([_compile_c(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "tlwe_linear ok" in r.stdout, r.stdout[-3000:]
