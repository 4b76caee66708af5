"""Cleartext polynomial-weight linear layers on packed TRLWE samples (include/mosfhet_hip.h: mosfhet_hip_polylinear_*, mosfhet_hip_trlwe_linear_batch,
mosfhet_hip_trlwe_linear_extract_batch, mosfhet_hip_trlwe_linear_keyswitch_functional_bootstrap_batch, mosfhet_hip_trlwe_linear_plan; mosfhet_amd/csrc/capi_polylinear.inc,
polylinear_body in trace_kernels.h; include/mosfhet_compat.h: mosfhet_trlwe_linear, mosfhet_trlwe_linear_extract, mosfhet_polylinear_dot_layout).

Expected words come from tests/trlwe_linear_reference.py: the contract restated from the oracle's primitives (torus_to_dft, dft_mul_addto, dft_to_torus,
trlwe_extract_tlwe).  Every device comparison is == on all words.  The one bound (test_restatement_against_the_exact_convolution) is the oracle's own figure."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from trlwe_linear_reference import csr_of_dense, exact, negacyclic_exact, restatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
_CACHE = {}


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_restatement_against_the_exact_convolution(oracle):
    """N = 1024, rows_in = 4, uniform torus inputs, weights uniform in [-128, 128): the restatement deviates from the exact negacyclic convolution mod 2^64 (Python
    integers) by the double arithmetic's error only.  The CPU oracle measured max 2^25.1, rms 2^23.3 at this shape (2^23.2 at N = 256, rows_in = 1; 2^33.1 with 16-bit
    weights: about 2^10 |w| sqrt(N rows_in)); the bound is that figure with 2^3 for the seed.  The code under test plays no part."""
    N, rows_in = 1024, 4
    rng = np.random.default_rng(0xC0471)
    x = rng.integers(0, 2 ** 64, size=(1, rows_in, 2, N), dtype=np.uint64)
    W = rng.integers(-128, 128, size=(1, rows_in, N), dtype=np.int64)
    csr = csr_of_dense(W)
    dev = oracle.torus_dist(restatement(oracle, *csr, None, x), exact(*csr, None, x))
    print("restatement against the exact convolution: max 2^%.1f, rms 2^%.1f" % (np.log2(max(dev.max(), 1.0)), np.log2(max(np.sqrt((dev ** 2).mean()), 1.0))))
    assert dev.max() < 2.0 ** 28, np.log2(dev.max())


def _dot_layout(native_lib, w, per, N, stride):
    f = native_lib.mosfhet_polylinear_dot_layout
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    f.restype = C.c_int
    poly = np.full(N, 77, dtype=np.int64)
    w = np.ascontiguousarray(w, dtype=np.int64)
    return f(poly.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), per, N, stride), poly


def test_dot_layout(native_lib):
    """poly[0] = w[0], poly[N - c stride] = -w[c], zero elsewhere; coefficient 0 of the exact convolution with a polynomial holding x[c] at coefficient c stride (and
    anything in between) is sum w[c] x[c] mod 2^64, for stride 1 and N / 16; per * stride > N, per < 1, stride < 1 and null pointers are refused, nothing written."""
    N, per = 1024, 16
    rng = np.random.default_rng(0xD07)
    w = rng.integers(-3, 4, size=per, dtype=np.int64)
    w[0], w[1] = 3, -3
    for stride in (1, N // 16):
        rc, poly = _dot_layout(native_lib, w, per, N, stride)
        assert rc == 0
        want = np.zeros(N, dtype=np.int64)
        want[0] = w[0]
        for c in range(1, per):
            want[N - c * stride] = -w[c]
        assert (poly == want).all(), stride
        p = rng.integers(0, 2 ** 64, size=N, dtype=np.uint64)
        dot = sum(int(w[c]) * int(p[c * stride]) for c in range(per)) % 2 ** 64
        assert int(negacyclic_exact(p, poly)[0]) == dot, stride
    for args in ((per, N, N // 16 + 1), (N + 1, N, 1), (0, N, 1), (per, N, 0), (per, 1000, 1)):
        rc, poly = _dot_layout(native_lib, w, *args)
        assert rc == -1 and (poly == 77).all(), args
    f = native_lib.mosfhet_polylinear_dot_layout
    assert f(None, w.ctypes.data_as(C.c_void_p), per, N, 1) == -1
    rc, poly = _dot_layout(native_lib, w, N // 64, N, 64)                      # per * stride == N: the last entry lands on coefficient stride
    assert rc == 0 and poly[64] == -w[N // 64 - 1]


def test_polylinear_symbols_and_argument_checks(native_lib):
    """The library exports the new entry points and the binding its functions; every refusal that needs no device returns MOSFHET_HIP_EINVAL with a message naming the
    argument -- on fake pointers, before any handle is read and before any HIP call (this runs without a GPU); count == 0 is OK."""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_polylinear_create_dense", "mosfhet_hip_polylinear_create_sparse", "mosfhet_hip_polylinear_destroy", "mosfhet_hip_polylinear_info",
                 "mosfhet_hip_polylinear_clone", "mosfhet_hip_trlwe_linear_batch", "mosfhet_hip_trlwe_linear_extract_batch",
                 "mosfhet_hip_trlwe_linear_keyswitch_functional_bootstrap_batch", "mosfhet_hip_trlwe_linear_plan", "mosfhet_trlwe_linear", "mosfhet_trlwe_linear_extract",
                 "mosfhet_polylinear_dot_layout"):
        assert hasattr(native_lib, name), name
    assert hasattr(engine, "trlwe_linear_plan")
    for name in ("polylinear_create_dense", "polylinear_create_sparse", "clone_polylinear", "trlwe_linear", "trlwe_linear_extract", "trlwe_linear_keyswitch_functional_bootstrap"):
        assert hasattr(engine.Engine, name), name
    for name in ("info", "close"):
        assert hasattr(engine.PolyLinearMap, name), name
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)     # never dereferenced: every call below ends on its scalar arguments
    f = native_lib.mosfhet_hip_trlwe_linear_batch
    f.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
    assert f(None, fake, fake, fake, 1, None) == EINVAL and "ctx" in err()
    assert f(fake, None, fake, fake, 1, None) == EINVAL and "lin" in err()
    assert f(fake, fake, fake, fake, -1, None) == EINVAL and "count = -1" in err()
    assert f(fake, fake, fake, fake, 0, None) == 0                              # count == 0: nothing to do, no handle read
    assert f(fake, fake, None, None, 0, None) == 0
    x = native_lib.mosfhet_hip_trlwe_linear_extract_batch
    x.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p]
    assert x(None, fake, fake, fake, 0, 1, None) == EINVAL and "ctx" in err()
    assert x(fake, None, fake, fake, 0, 1, None) == EINVAL and "lin" in err()
    assert x(fake, fake, fake, fake, 0, -2, None) == EINVAL and "count = -2" in err()
    assert x(fake, fake, fake, fake, -1, 1, None) == EINVAL and "idx = -1" in err()
    assert x(fake, fake, fake, fake, -1, 0, None) == EINVAL and "idx = -1" in err()       # ... before count == 0 returns
    assert x(fake, fake, fake, fake, 0, 0, None) == 0                             # count == 0: nothing to do, no handle read
    assert x(fake, fake, None, None, 5000, 0, None) == 0                          # ... not even for idx >= N
    g = native_lib.mosfhet_hip_trlwe_linear_keyswitch_functional_bootstrap_batch
    g.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    assert g(None, fake, fake, fake, fake, fake, 1, fake, 0, 1, 4, 1, None) == EINVAL and "ctx" in err()
    assert g(fake, None, fake, fake, fake, fake, 1, fake, 0, 1, 4, 1, None) == EINVAL and "lin" in err()
    assert g(fake, fake, None, fake, fake, fake, 1, fake, 0, 1, 4, 1, None) == EINVAL and "ksk" in err()
    assert g(fake, fake, fake, None, fake, fake, 1, fake, 0, 1, 4, 1, None) == EINVAL and "bsk" in err()
    assert g(fake, fake, fake, fake, fake, fake, 1, fake, 0, -1, 4, 1, None) == EINVAL and "count = -1" in err()
    assert g(fake, fake, fake, fake, fake, fake, 1, fake, -3, 1, 4, 1, None) == EINVAL and "idx = -3" in err()
    d = native_lib.mosfhet_hip_polylinear_create_dense
    d.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int]
    out = C.c_void_p()
    assert d(None, C.byref(out), fake, None, 2, 2, 1024) == EINVAL and "ctx" in err()
    assert d(fake, None, fake, None, 2, 2, 1024) == EINVAL and "out" in err()
    assert d(fake, C.byref(out), fake, None, 0, 2, 1024) == EINVAL and "rows_out = 0" in err()
    assert d(fake, C.byref(out), fake, None, 2, -1, 1024) == EINVAL and "rows_in = -1" in err()
    assert d(fake, C.byref(out), fake, None, 2, 2, 512) == EINVAL and "N = 512" in err()
    assert d(fake, C.byref(out), None, None, 2, 2, 1024) == EINVAL and "h_W" in err()
    s = native_lib.mosfhet_hip_polylinear_create_sparse
    s.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int]
    ints = lambda *v: (C.c_int * len(v))(*v)
    assert s(None, C.byref(out), ints(0, 1), ints(0), fake, None, 1, 1, 1024) == EINVAL and "ctx" in err()
    assert s(fake, C.byref(out), ints(0, 1), ints(0), fake, None, 0, 1, 1024) == EINVAL and "rows_out = 0" in err()
    assert s(fake, C.byref(out), ints(0, 1), ints(0), fake, None, 1, 0, 1024) == EINVAL and "rows_in = 0" in err()
    assert s(fake, C.byref(out), ints(0, 1), ints(0), fake, None, 1, 1, 3000) == EINVAL and "N = 3000" in err()
    assert s(fake, C.byref(out), None, ints(0), fake, None, 1, 1, 1024) == EINVAL and "h_row_ptr" in err()
    assert s(fake, C.byref(out), ints(1, 2), ints(0, 0), fake, None, 1, 1, 1024) == EINVAL and "row_ptr[0] = 1" in err()
    assert s(fake, C.byref(out), ints(0, 2, 1), ints(0, 0), fake, None, 2, 1, 1024) == EINVAL and "row_ptr[2] = 1" in err()     # not monotone
    assert s(fake, C.byref(out), ints(0, 2), ints(0, 3), fake, None, 1, 3, 1024) == EINVAL and "col[1] = 3" in err()          # out of range
    assert s(fake, C.byref(out), ints(0, 2), ints(0, -1), fake, None, 1, 3, 1024) == EINVAL and "col[1] = -1" in err()
    assert s(fake, C.byref(out), ints(0, 2), None, fake, None, 1, 3, 1024) == EINVAL and "h_col" in err()
    assert out.value is None                                                                                                # nothing was created
    i = native_lib.mosfhet_hip_polylinear_info
    i.argtypes = [C.c_void_p, C.c_void_p]
    assert i(None, (C.c_longlong * 6)()) == EINVAL and "lin" in err()
    c = native_lib.mosfhet_hip_polylinear_clone
    c.argtypes = [C.c_void_p] * 3
    assert c(None, fake, C.byref(out)) == EINVAL and "ctx_other" in err()
    assert c(fake, None, C.byref(out)) == EINVAL and "lin" in err()
    assert c(fake, fake, None) == EINVAL and "out" in err()
    p = native_lib.mosfhet_hip_trlwe_linear_plan
    p.argtypes = [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p]
    plan = (C.c_longlong * 8)()
    assert p(1024, 2, 2, -1, 1, 0, 256, 0, None) == EINVAL and "plan" in err()
    assert p(512, 2, 2, -1, 1, 0, 256, 0, plan) == EINVAL and "N = 512" in err()
    assert p(1024, 0, 2, -1, 1, 0, 256, 0, plan) == EINVAL and "rows_out = 0" in err()
    assert p(1024, 2, 0, -1, 1, 0, 256, 0, plan) == EINVAL and "rows_in = 0" in err()
    assert p(1024, 2, 2, -2, 1, 0, 256, 0, plan) == EINVAL and "nnz = -2" in err()
    assert p(1024, 2, 2, -1, -1, 0, 256, 0, plan) == EINVAL and "count = -1" in err()
    assert p(1024, 2, 2, -1, 1, 2, 256, 0, plan) == EINVAL and "extract = 2" in err()
    assert p(1024, 2, 2, -1, 1, 0, 0, 0, plan) == EINVAL and "cus = 0" in err()
    assert p(1024, 2, 2, -1, 1, 0, 256, -5, plan) == EINVAL and "workspace_bytes = -5" in err()
    assert p(1024, 2, 2, -1, 1, 0, 256, 2 * 2 * 1024 * 8 - 1, plan) == EINVAL and "workspace" in err()          # below one batch element
    assert p(1024, 2 ** 20, 1, 5, 2 ** 12, 0, 256, 2 ** 40, plan) == EINVAL and "do not fit one launch" in err()  # 2^32 teams in the one round
    assert p(1024, 2, 2, -1, 0, 0, 256, 0, plan) == 0 and plan[0] == 0 and plan[2] == 0                        # count == 0: no round
    assert p(1024, 2, 2, -1, 1, 1, 256, 0, plan) == 0


def test_polylinear_plan_values():
    """mosfhet_hip_trlwe_linear_plan at fixed shapes: one team per (batch element, output row); the pool holds rows_in * 2 transformed polynomials per batch element;
    a workspace of exactly one batch element gives count rounds of rows_out teams; dense against sparse differ in the bytes a team reads only; neither extract nor
    cus changes anything."""
    from mosfhet_amd import engine
    one = 4 * 2 * 1024 * 8
    p = engine.trlwe_linear_plan(1024, 16, 4, 64)
    assert p == dict(teams=1024, per_round=64, rounds=1, pool_bytes=64 * one, forwards=512, inverses=2048, weight_bytes=4 * 8192, input_bytes=4 * 16384), p
    assert engine.trlwe_linear_plan(1024, 16, 4, 64, extract=True, cus=64) == p
    q = engine.trlwe_linear_plan(1024, 16, 4, 64, workspace_bytes=one)
    assert q == dict(p, teams=16, per_round=1, rounds=64, pool_bytes=one), q
    q = engine.trlwe_linear_plan(1024, 16, 4, 64, workspace_bytes=5 * one + 17)
    assert (q["per_round"], q["rounds"], q["teams"], q["pool_bytes"]) == (5, 13, 80, 5 * one), q
    with pytest.raises(engine.MosfhetHipError, match="one batch element"):
        engine.trlwe_linear_plan(1024, 16, 4, 64, workspace_bytes=one - 1)
    s = engine.trlwe_linear_plan(1024, 16, 4, 64, nnz=24)           # 1.5 entries per row: the mean row, rounded up
    assert s == dict(p, weight_bytes=2 * 8192, input_bytes=2 * 16384), s
    assert engine.trlwe_linear_plan(1024, 16, 4, 64, nnz=64) == p     # the dense entries as a sparse handle
    e = engine.trlwe_linear_plan(1024, 3, 4, 7, nnz=0)
    assert (e["teams"], e["forwards"], e["weight_bytes"], e["input_bytes"]) == (21, 56, 0, 0), e
    big = engine.trlwe_linear_plan(4096, 2, 3, 5)
    assert big == dict(teams=10, per_round=5, rounds=1, pool_bytes=5 * 3 * 2 * 4096 * 8, forwards=30, inverses=20, weight_bytes=3 * 4096 * 8, input_bytes=3 * 2 * 4096 * 8), big


def test_polylinear_kernels_of_the_build(native_lib):
    """The new body is a run-time kind of trace_conversions_kernel: that kernel is still listed once per ring, without scratch; the library holds exactly 329 kernels;
    tools/check_lds_barriers.py found nothing on the build."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    rows = kernel_table.table()
    mine = [r for r in rows if r["name"].startswith("trace_conversions_kernel")]
    for r in mine:
        print("%-60s vgpr %3d  agpr %3d  sgpr %3d  lds %6d  scratch %4d" % (r["name"], r["vgpr"], r["agpr"], r["sgpr"], r["lds"], r["scratch"]))
    assert len(mine) == 3 and len({r["name"] for r in mine}) == 3, [r["name"] for r in mine]
    for r in mine:
        assert r["scratch"] == 0, r
    assert len(rows) == 329, len(rows)
    with open(os.path.join(ROOT, "mosfhet_amd", "build", "lds_barrier_check.txt")) as fh:
        report = fh.read()
    print(report)
    assert ", 0 violations" in report, report


def _compile_c(tmp_path):
    exe = str(tmp_path / "trlwe_linear")
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "trlwe_linear.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_polylinear_c_program_compiles_and_links(native_lib, tmp_path):
    """tests/c/trlwe_linear.c compiles against include/mosfhet.h and links against the built library (its device part: test_polylinear_host_face)."""
    assert os.path.exists(_compile_c(tmp_path))


# ---------------------------------------------------------------- cases ----------------------------------------------------------------
def _case(oracle, N, rows_out, rows_in, count):
    """uniform inputs, weights uniform in [-128, 128) with a zero polynomial among them (dense handles do not skip it), a uniform bias, and the restatement's words
    for the TRLWE mode with and without bias; made once per shape and left unchanged"""
    key = ("case", N, rows_out, rows_in, count)
    if key not in _CACHE:
        rng = np.random.default_rng([0x9011, N, rows_out, rows_in, count])
        x = rng.integers(0, 2 ** 64, size=(count, rows_in, 2, N), dtype=np.uint64)
        W = rng.integers(-128, 128, size=(rows_out, rows_in, N), dtype=np.int64)
        if rows_in > 1:
            W[rows_out - 1, 0] = 0
        bias = rng.integers(0, 2 ** 64, size=(rows_out, N), dtype=np.uint64)
        csr = csr_of_dense(W)
        _CACHE[key] = dict(x=x, W=W, bias=bias, csr=csr, plain=restatement(oracle, *csr, None, x), biased=restatement(oracle, *csr, bias, x))
    return _CACHE[key]


def _extracted(oracle, trlwe, idx):
    count, rows_out, two, N = trlwe.shape
    return np.stack([oracle.trlwe_extract_tlwe(np.ascontiguousarray(s), idx) for s in trlwe.reshape(-1, 2, N)]).reshape(count, rows_out, N + 1)


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


@pytest.mark.gpu
@pytest.mark.parametrize("N,rows_out,rows_in,count", [(1024, 1, 1, 1), (1024, 2, 3, 2), (1024, 3, 2, 5), (2048, 2, 2, 2), (4096, 1, 2, 1)])
def test_polylinear_dense_bit_exact(eng, oracle, N, rows_out, rows_in, count):
    """Dense handles, with and without bias: the TRLWE mode and the extract mode at idx 0, 1, N / 2, N - 1 == the restatement on every word; the bias lands on
    component b only."""
    import mosfhet_amd as ma
    D = _case(oracle, N, rows_out, rows_in, count)
    d_x = _dev(eng, D["x"])
    for bias, want in ((None, D["plain"]), (D["bias"], D["biased"])):
        lin = eng.polylinear_create_dense(D["W"], bias)
        info = lin.info()
        assert (info["rows_out"], info["rows_in"], info["nnz"], info["N"], info["form"]) == (rows_out, rows_in, -1, N, "dense"), info
        assert info["nbytes"] >= D["W"].size * 8
        got = ma.to_numpy(eng.trlwe_linear(lin, d_x))
        assert got.shape == want.shape and (got == want).all(), "TRLWE mode, bias %s: %d words differ" % (bias is not None, (got != want).sum())
        for idx in (0, 1, N // 2, N - 1):
            got = ma.to_numpy(eng.trlwe_linear_extract(lin, d_x, idx))
            ext = _extracted(oracle, want, idx)
            assert got.shape == ext.shape and (got == ext).all(), "extract at %d, bias %s: %d words differ" % (idx, bias is not None, (got != ext).sum())
        lin.close()
    assert (D["biased"][:, :, 0] == D["plain"][:, :, 0]).all() and (D["biased"][:, :, 1] - D["plain"][:, :, 1] == D["bias"][None]).all()


@pytest.mark.gpu
def test_polylinear_sparse(eng, oracle):
    """N = 1024, rows_in = 3, count = 2: an empty row gives (0, bias); a repeated column adds, in the stored order; unsorted columns; and the same ordered entries
    give the same words dense and sparse."""
    import mosfhet_amd as ma
    N, rows_in, count = 1024, 3, 2
    rng = np.random.default_rng(0x5BA25E)
    x = rng.integers(0, 2 ** 64, size=(count, rows_in, 2, N), dtype=np.uint64)
    rows = [[], [2, 2, 0, 2], [2, 0, 1], [1], []]
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    col = np.array([c for r in rows for c in r], dtype=np.int32)
    val = rng.integers(-128, 128, size=(len(col), N), dtype=np.int64)
    bias = rng.integers(0, 2 ** 64, size=(len(rows), N), dtype=np.uint64)
    d_x = _dev(eng, x)
    for b in (None, bias):
        lin = eng.polylinear_create_sparse(ptr, col, val, rows_in, N, b)
        info = lin.info()
        assert (info["rows_out"], info["rows_in"], info["nnz"], info["N"], info["form"]) == (len(rows), rows_in, len(col), N, "sparse"), info
        want = restatement(oracle, ptr, col, val, b, x)
        got = ma.to_numpy(eng.trlwe_linear(lin, d_x))
        assert (got == want).all(), "sparse, bias %s: %d words differ, rows %s" % (b is not None, (got != want).sum(), sorted(set(np.nonzero(got != want)[1])))
        for j in (0, 4):
            assert (got[:, j, 0] == 0).all() and (got[:, j, 1] == (0 if b is None else b[j][None])).all(), "an empty row is (0, bias)"
        got = ma.to_numpy(eng.trlwe_linear_extract(lin, d_x, 7))
        assert (got == _extracted(oracle, want, 7)).all()
        lin.close()
    empty = eng.polylinear_create_sparse([0, 0], [], np.zeros((0, N), dtype=np.int64), rows_in, N)     # no entry at all
    assert (ma.to_numpy(eng.trlwe_linear(empty, d_x)) == 0).all()
    empty.close()
    D = _case(oracle, 1024, 2, 3, 2)
    dense, sparse = eng.polylinear_create_dense(D["W"], D["bias"]), eng.polylinear_create_sparse(*D["csr"], 3, 1024, D["bias"])
    d_x = _dev(eng, D["x"])
    a, b = ma.to_numpy(eng.trlwe_linear(dense, d_x)), ma.to_numpy(eng.trlwe_linear(sparse, d_x))
    assert (a == D["biased"]).all() and (b == a).all(), "the sparse handle of the dense entries differs from the dense handle"
    dense.close()
    sparse.close()


@pytest.mark.gpu
def test_polylinear_value_edges(eng, oracle):
    """Input words drawn from {0, 1, 2^63 - 1, 2^63, 2^64 - 1}, weights from {0, +-1, 2^53 + 1, 2^62, -2^63}: the sums pass 2^130 and the general rounding still gives
    the restatement's words, TRLWE mode and extract mode; N = 1024 and 2048."""
    import mosfhet_amd as ma
    words = np.array([0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)
    weights = np.array([0, 1, -1, 2 ** 53 + 1, 2 ** 62, -2 ** 63], dtype=np.int64)
    for N in (1024, 2048):
        rng = np.random.default_rng([0xED6E, N])
        x = words[rng.integers(0, len(words), size=(2, 2, 2, N))]
        W = weights[rng.integers(0, len(weights), size=(2, 2, N))]
        W[1, 1] = -2 ** 63                                        # every coefficient at the edge
        x[1, 1] = np.uint64(2 ** 63)
        bias = words[rng.integers(0, len(words), size=(2, N))]
        want = restatement(oracle, *csr_of_dense(W), bias, x)
        lin = eng.polylinear_create_dense(W, bias)
        got = ma.to_numpy(eng.trlwe_linear(lin, _dev(eng, x)))
        assert (got == want).all(), "N = %d: %d words differ" % (N, (got != want).sum())
        got = ma.to_numpy(eng.trlwe_linear_extract(lin, _dev(eng, x), N - 1))
        assert (got == _extracted(oracle, want, N - 1)).all(), N
        lin.close()


@pytest.mark.gpu
def test_polylinear_run_contexts(eng, oracle):
    """(3, 2, 5) at N = 1024: a larger call on other inputs first (the pool holds its transforms: garbage for this one); sentinel words behind d_out stay, both modes;
    with the workspace set to one batch element the call runs count rounds and gives the same words; a position in the batch changes nothing."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, rows_out, rows_in, count = 1024, 3, 2, 5
    D = _case(oracle, N, rows_out, rows_in, count)
    lin = eng.polylinear_create_dense(D["W"], D["bias"])
    d_x = _dev(eng, D["x"])
    junk = _dev(eng, np.random.default_rng(1).integers(0, 2 ** 64, size=(count + 2, rows_in, 2, N), dtype=np.uint64))
    eng.trlwe_linear(lin, junk)
    SENT = -0x0123456789ABCDEF
    for idx, words, want in ((None, 2 * N, D["biased"]), (3, N + 1, _extracted(oracle, D["biased"], 3))):
        buf = torch.full((count * rows_out * words + 64,), SENT, dtype=torch.int64, device=eng.device)
        out = buf[:count * rows_out * words].view(count, rows_out, *((2, N) if idx is None else (N + 1,)))
        if idx is None:
            eng.trlwe_linear(lin, d_x, out=out)
        else:
            eng.trlwe_linear_extract(lin, d_x, idx, out=out)
        assert (ma.to_numpy(out) == want).all() and (buf[count * rows_out * words:] == SENT).all(), idx
    one = rows_in * 2 * N * 8
    assert engine.trlwe_linear_plan(N, rows_out, rows_in, count, workspace_bytes=one)["rounds"] == count
    engine.set_tlwe_pack_workspace(one)
    try:
        assert (ma.to_numpy(eng.trlwe_linear(lin, d_x)) == D["biased"]).all(), "one batch element per round"
        assert (ma.to_numpy(eng.trlwe_linear_extract(lin, d_x, N - 1)) == _extracted(oracle, D["biased"], N - 1)).all()
        engine.set_tlwe_pack_workspace(one - 8)
        with pytest.raises(engine.MosfhetHipError, match="one batch element"):
            eng.trlwe_linear(lin, d_x)
    finally:
        engine.set_tlwe_pack_workspace(0)
    back = np.ascontiguousarray(D["x"][::-1])
    assert (ma.to_numpy(eng.trlwe_linear(lin, _dev(eng, back))) == D["biased"][::-1]).all(), "a sample's position in the batch"
    assert (ma.to_numpy(eng.trlwe_linear(lin, d_x[:0])).size == 0)                 # count == 0
    lin.close()


@pytest.mark.gpu
def test_polylinear_calls_are_captured_in_a_graph(eng, oracle):
    """Both calls captured on one side stream after an eager call of the same size, replayed on fresh inputs: the replayed words == the plain call's -- no hidden
    allocation or synchronisation.  One stream, no parallel branches."""
    import torch
    import mosfhet_amd as ma
    N = 1024
    D = _case(oracle, N, 2, 3, 2)
    lin = eng.polylinear_create_dense(D["W"], D["bias"])
    xs = [_dev(eng, D["x"]), _dev(eng, np.ascontiguousarray(D["x"][::-1]))]
    calls = [("trlwe", lambda i, o: eng.trlwe_linear(lin, i, out=o), (2, 2, 2, N)), ("extract", lambda i, o: eng.trlwe_linear_extract(lin, i, 9, out=o), (2, 2, N + 1))]
    side = torch.cuda.Stream(device=eng.device)
    for name, call, shape in calls:
        eager = [ma.to_numpy(call(x, eng.empty(*shape))) for x in xs]
        assert (eager[0] == (D["biased"] if name == "trlwe" else _extracted(oracle, D["biased"], 9))).all()
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
    lin.close()


@pytest.mark.gpu
def test_two_host_threads_polylinear(eng, oracle):
    """Two host threads, each on a stream of its own and with a pool of its own, run the call five times concurrently on one shared handle per shape -- (3, 2, 5) at
    N = 1024 and (2, 2, 2) at N = 2048: every result equals the restatement."""
    import threading
    import torch
    import mosfhet_amd as ma
    jobs = []
    for shape in ((1024, 3, 2, 5), (2048, 2, 2, 2)):
        D = _case(oracle, *shape)
        jobs.append((eng.polylinear_create_dense(D["W"], D["bias"]), _dev(eng, D["x"]), D["biased"]))
    torch.cuda.synchronize()
    bad, errors = [0, 0], []

    def worker(k):
        try:
            lin, d_in, want = jobs[k]
            stream = torch.cuda.Stream(device=eng.device)
            with torch.cuda.stream(stream):
                for _ in range(5):
                    bad[k] += int(not (ma.to_numpy(eng.trlwe_linear(lin, d_in)) == want).all())
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert bad == [0, 0], bad
    for lin, _, _ in jobs:
        lin.close()


@pytest.mark.gpu
def test_polylinear_refusals_on_the_device(eng, oracle):
    """idx = N, d_out overlapping d_in (the same buffer, and a partial overlap) and a handle made for another context are refused with MOSFHET_HIP_EINVAL, and nothing
    is written; the handle's clone for that context works there."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N = 1024
    D = _case(oracle, N, 2, 3, 2)
    lin = eng.polylinear_create_dense(D["W"], D["bias"])
    in_w, out_w = 2 * 3 * 2 * N, 2 * 2 * 2 * N
    buf = torch.zeros(in_w + out_w, dtype=torch.int64, device=eng.device)
    buf[:in_w] = _dev(eng, D["x"]).view(-1)
    before = buf.clone()
    d_in = buf[:in_w].view(2, 3, 2, N)
    with pytest.raises(engine.MosfhetHipError, match="idx = 1024"):
        eng.trlwe_linear_extract(lin, d_in, N)
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.trlwe_linear(lin, d_in, out=buf[:out_w].view(2, 2, 2, N))
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.trlwe_linear(lin, d_in, out=buf[in_w - 1:in_w - 1 + out_w].view(2, 2, 2, N))
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.trlwe_linear_extract(lin, d_in, 0, out=buf[in_w - 1:in_w - 1 + 4 * (N + 1)].view(2, 2, N + 1))
    other = ma.Engine(0)
    try:
        with pytest.raises(engine.MosfhetHipError, match="another context"):
            other.trlwe_linear(lin, d_in, out=buf[in_w:].view(2, 2, 2, N))
        torch.cuda.synchronize(eng.device)
        assert (buf == before).all(), "a refused call wrote to its output"
        mine = other.clone_polylinear(lin)
        assert mine.info() == lin.info()
        assert (ma.to_numpy(other.trlwe_linear(mine, d_in)) == D["biased"]).all()
        mine.close()
    finally:
        other.close()
    got = eng.trlwe_linear(lin, d_in, out=buf[in_w:].view(2, 2, 2, N))              # adjacent: fine
    assert (ma.to_numpy(got) == D["biased"]).all()
    lin.close()


def _keys(eng, oracle, name):
    """The key fixtures tests/test_tlwe_linear.py builds (the key set of tests/test_gpu_parity.py with an N -> n key-switch key), with device handles of THIS module's
    engine"""
    key = ("keys", name)
    if key not in _CACHE:
        from mosfhet_amd import host
        from test_gpu_parity import _keyset
        K = _keyset(name, eng, oracle)
        P = K["P"]
        if "ksk" not in K:
            K["ksk"] = host.gen_tlwe_ks_key(K["lk"], K["out_key"], P["t"], P["base_bit"])
        _CACHE[key] = dict(K=K, P=P, dksk=eng.load_keyswitch_key(K["ksk"], P["base_bit"]), bsk=eng.load_bootstrap_key(K["bk"], 1, P["l"], P["Bg_bit"]))
    return _CACHE[key]


@pytest.mark.gpu
def test_polylinear_fused_call_equals_the_composition(eng, oracle):
    """count = 2, rows_out = 2, N = 1024, SET_1 keys: the fused call == trlwe_linear_extract followed by keyswitch_functional_bootstrap, word for word -- both extract
    values, one test vector and one per result, idx 0 and 5; a handle of another ring is refused."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine, host
    K = _keys(eng, oracle, "set1")
    P, dksk, bsk = K["P"], K["dksk"], K["bsk"]
    N = P["N"]
    assert N == 1024
    D = _case(oracle, N, 2, 3, 2)
    lin = eng.polylinear_create_dense(D["W"], D["bias"])
    d_x = _dev(eng, D["x"])
    rng = np.random.default_rng(0xF05ED)
    tvs = np.stack([host.torus_packing(rng.integers(0, 2 ** 64, size=4, dtype=np.uint64), 1, N) for _ in range(4)])
    for idx in (0, 5):
        d_y = eng.trlwe_linear_extract(lin, d_x, idx).view(4, N + 1)
        assert (ma.to_numpy(d_y) == _extracted(oracle, D["biased"], idx).reshape(4, N + 1)).all()
        for tv in (tvs[:1], tvs):
            d_tv = _dev(eng, tv)
            for extract in (True, False):
                want = ma.to_numpy(eng.keyswitch_functional_bootstrap(dksk, bsk, d_tv, d_y, 4, extract=extract))
                got = ma.to_numpy(eng.trlwe_linear_keyswitch_functional_bootstrap(lin, dksk, bsk, d_tv, d_x, 4, idx=idx, extract=extract))
                assert got.shape[:2] == (2, 2) and (got.reshape(want.shape) == want).all(), (idx, len(tv), extract)
    lin.close()
    D2 = _case(oracle, 2048, 2, 2, 2)
    lin2 = eng.polylinear_create_dense(D2["W"])
    with pytest.raises(engine.MosfhetHipError, match="ring"):
        eng.trlwe_linear_keyswitch_functional_bootstrap(lin2, dksk, bsk, _dev(eng, tvs[:1]), _dev(eng, D2["x"]), 4)
    lin2.close()


@pytest.mark.gpu
def test_packed_inner_products_decrypt(eng, oracle, native_lib):
    """16 four-bit values per sample, packed at stride 1 under a ring key (oracle.trlwe_sample, noise 2^-40), rows_in = 2, rows_out = 3, count = 2; weights in
    [-3, 3] through mosfhet_polylinear_dot_layout; extract at 0: the phase is sum w x mod 16 in slots of 2^60, within half a slot."""
    import mosfhet_amd as ma
    N, per, rows_in, rows_out, count = 1024, 16, 2, 3, 2
    rng = oracle.Rng(0xD0751)
    s_ring = oracle.gen_binary_key(rng, N)
    nrng = np.random.default_rng(0xD0752)
    vals = nrng.integers(0, 16, size=(count, rows_in, per))
    w = nrng.integers(-3, 4, size=(rows_out, rows_in, per), dtype=np.int64)
    x = np.empty((count, rows_in, 2, N), dtype=np.uint64)
    for b in range(count):
        for i in range(rows_in):
            m = np.zeros(N, dtype=np.uint64)
            m[:per] = vals[b, i].astype(np.uint64) << np.uint64(60)
            x[b, i] = oracle.trlwe_sample(rng, m, s_ring.reshape(1, N), 2.0 ** -40)
    W = np.stack([np.stack([_dot_layout(native_lib, w[j, i], per, N, 1)[1] for i in range(rows_in)]) for j in range(rows_out)])
    lin = eng.polylinear_create_dense(W)
    got = ma.to_numpy(eng.trlwe_linear_extract(lin, _dev(eng, x), 0))
    lin.close()
    want = np.einsum("jic,bic->bj", w, vals) % 16
    worst = 0.0
    for b in range(count):
        for j in range(rows_out):
            ph = oracle.tlwe_phase(np.ascontiguousarray(got[b, j]), s_ring)
            worst = max(worst, float(oracle.torus_dist(ph, np.uint64(int(want[b, j]) << 60))))
    print("inner products of 32 four-bit values with weights in [-3, 3]: worst distance from sum w x 2^%.1f (half a slot: 2^59)" % np.log2(max(worst, 1.0)))
    assert worst < 2.0 ** 59


@pytest.mark.gpu
def test_polylinear_host_face(native_lib, tmp_path):
    """tests/c/trlwe_linear.c: mosfhet_trlwe_linear on host structs equals the drop-in layer's loop of trlwe_DFT_mul_addto_by_polynomial word for word, with and without
    bias; mosfhet_trlwe_linear_extract equals trlwe_extract_tlwe of it and decrypts to the inner products."""
    r = subprocess.run([_compile_c(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "trlwe_linear ok" in r.stdout, r.stdout[-3000:]
