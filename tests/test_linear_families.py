"""What the three families of linear layers share on the host (mosfhet_amd/csrc/capi_linear_common.inc: the CSR checks, the handles' one device image and its clone,
the plan, checks and round loop of the two packed families; capi_linear.inc, capi_polylinear.inc, capi_gswlinear.inc): the families refuse a bad CSR in the same
words, and a dense handle, a sparse handle of the same ordered entries and the clones of both give the same words.  Every device comparison is == on all words; the
one reference (the LWE family's) is exact integer arithmetic mod 2^64."""
import ctypes as C

import numpy as np
import pytest

EINVAL = -1


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_linear_families_refuse_alike(native_lib):
    """One table of bad sparse inputs through the sparse creators of all three families (and the creator over selectors), on a fake context that is never read: null
    row_ptr, row_ptr[0] = 1, a row_ptr that falls, col = rows_in, col = -1.  Each refusal is MOSFHET_HIP_EINVAL, creates nothing, carries the creator's own name
    as prefix, and behind it the same text in every family."""
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)
    ints = lambda *v: (C.c_int * len(v))(*v)
    vals = (C.c_longlong * 4)(1, 1, 1, 1)
    out = C.c_void_p()
    lin = native_lib.mosfhet_hip_linear_create_sparse
    lin.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int]
    poly = native_lib.mosfhet_hip_polylinear_create_sparse
    poly.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int]
    gsw = native_lib.mosfhet_hip_gswlinear_create_sparse
    gsw.argtypes = [C.c_void_p] * 6 + [C.c_int] * 5
    sel = native_lib.mosfhet_hip_gswlinear_create_from_selectors
    sel.argtypes = [C.c_void_p] * 6 + [C.c_int] * 5
    creators = {
        "linear_create_sparse": lambda ptr, col, ro, ri: lin(fake, C.byref(out), ptr, col, vals, None, ro, ri),
        "polylinear_create_sparse": lambda ptr, col, ro, ri: poly(fake, C.byref(out), ptr, col, fake, None, ro, ri, 1024),
        "gswlinear_create_sparse": lambda ptr, col, ro, ri: gsw(fake, C.byref(out), ptr, col, fake, None, ro, ri, 1024, 2, 8),
        "gswlinear_create_from_selectors": lambda ptr, col, ro, ri: sel(fake, C.byref(out), fake, ptr, col, None, ro, ri, 1024, 2, 8),
    }
    table = [
        ((None, ints(0), 1, 1), "null h_row_ptr"),
        ((ints(1, 2), ints(0, 0), 1, 1), "row_ptr[0] = 1 (must be 0)"),
        ((ints(0, 2, 1), ints(0, 0), 2, 1), "row_ptr[2] = 1 is below row_ptr[1] = 2"),
        ((ints(0, 2), ints(0, 3), 1, 3), "col[1] = 3 (rows_in = 3)"),
        ((ints(0, 2), ints(0, -1), 1, 3), "col[1] = -1 (rows_in = 3)"),
    ]
    for args, text in table:
        said = {}
        for who, create in creators.items():
            assert create(*args) == EINVAL, (who, text)
            prefix, _, said[who] = err().partition(": ")
            assert prefix == who, err()
        assert set(said.values()) == {text}, said
    assert out.value is None                                                    # nothing was created


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


ROWS_OUT, ROWS_IN, COUNT = 2, 2, 3
CSR = (np.array([0, 2, 4], dtype=np.int32), np.array([0, 1, 0, 1], dtype=np.int32))      # the dense map's entries, in its order


def _lwe_family(eng, rng):
    """n = 16.  Besides the dense / sparse pair a sparse handle whose row 0 has 150 entries, more than LINEAR_CHUNK = 64: three chunks and a second list level."""
    import mosfhet_amd as ma
    n = 16
    x = rng.integers(0, 2 ** 64, size=(COUNT, ROWS_IN, n + 1), dtype=np.uint64)
    W = rng.integers(-2 ** 40, 2 ** 40, size=(ROWS_OUT, ROWS_IN), dtype=np.int64)
    bias = rng.integers(0, 2 ** 64, size=ROWS_OUT, dtype=np.uint64)
    long_col = rng.integers(0, ROWS_IN, size=150 + 1).astype(np.int32)
    long_val = rng.integers(-2 ** 40, 2 ** 40, size=150 + 1, dtype=np.int64)
    long_ptr = np.array([0, 150, 151], dtype=np.int32)
    handles = {"dense": eng.linear_dense(W, bias), "sparse": eng.linear_sparse(*CSR, W.reshape(-1), ROWS_IN, bias),
               "cut row": eng.linear_sparse(long_ptr, long_col, long_val, ROWS_IN, bias)}

    def exact(ptr, col, val):                                                  # mod 2^64: uint64 arithmetic wraps
        want = np.zeros((COUNT, ROWS_OUT, n + 1), dtype=np.uint64)
        want[:, :, n] = bias
        for j in range(ROWS_OUT):
            for q in range(ptr[j], ptr[j + 1]):
                want[:, j] += val.astype(np.uint64)[q] * x[:, col[q]]
        return want

    d_x = ma.to_device(x, eng.device)
    return dict(handles=handles, clone=eng.clone_linear, groups=[("dense", "sparse"), ("cut row",)], rounds=None,
                runs=[lambda lin: eng.tlwe_linear(lin, d_x)], want={"dense": exact(*CSR, W.reshape(-1)), "cut row": exact(long_ptr, long_col, long_val)})


def _poly_family(eng, rng):
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N = 1024
    x = rng.integers(0, 2 ** 64, size=(COUNT, ROWS_IN, 2, N), dtype=np.uint64)
    W = rng.integers(-128, 128, size=(ROWS_OUT, ROWS_IN, N), dtype=np.int64)
    bias = rng.integers(0, 2 ** 64, size=(ROWS_OUT, N), dtype=np.uint64)
    handles = {"dense": eng.polylinear_create_dense(W, bias), "sparse": eng.polylinear_create_sparse(*CSR, W.reshape(-1, N), ROWS_IN, N, bias)}
    one = ROWS_IN * 2 * N * 8
    d_x = ma.to_device(x, eng.device)
    return dict(handles=handles, clone=eng.clone_polylinear, groups=[("dense", "sparse")], workspace=one,
                rounds=engine.trlwe_linear_plan(N, ROWS_OUT, ROWS_IN, COUNT, workspace_bytes=one)["rounds"],
                runs=[lambda lin: eng.trlwe_linear(lin, d_x), lambda lin: eng.trlwe_linear_extract(lin, d_x, 5)], want={})


def _gsw_family(eng, rng):
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, l, Bg_bit = 1024, 2, 8
    x = rng.integers(0, 2 ** 64, size=(COUNT, ROWS_IN, 2, N), dtype=np.uint64)
    W = rng.integers(0, 2 ** 64, size=(ROWS_OUT, ROWS_IN, 2 * l, 2, N), dtype=np.uint64)
    bias = rng.integers(0, 2 ** 64, size=(ROWS_OUT, N), dtype=np.uint64)
    handles = {"dense": eng.gswlinear_create_dense(W, Bg_bit, bias),
               "sparse": eng.gswlinear_create_sparse(*CSR, W.reshape(-1, 2 * l, 2, N), ROWS_IN, N, l, Bg_bit, bias)}
    one = ROWS_IN * 2 * l * N * 8
    d_x = ma.to_device(x, eng.device)
    return dict(handles=handles, clone=eng.clone_gswlinear, groups=[("dense", "sparse")], workspace=one,
                rounds=engine.trlwe_gsw_linear_plan(N, l, ROWS_OUT, ROWS_IN, COUNT, workspace_bytes=one)["rounds"],
                runs=[lambda lin: eng.trlwe_gsw_linear(lin, d_x), lambda lin: eng.trlwe_gsw_linear_extract(lin, d_x, 5)], want={})


@pytest.mark.gpu
@pytest.mark.parametrize("family", [_lwe_family, _poly_family, _gsw_family], ids=["linear", "polylinear", "gswlinear"])
def test_linear_families_dense_sparse_clone_agree(eng, family):
    """rows_out = rows_in = 2, count = 3; N = 1024, l = 2, Bg_bit = 8 (n = 16 for the LWE family); the workspace bound at exactly one batch element, so the packed
    families run three rounds.  A clone on the same context reports the original's info(), and the dense handle, the sparse handle of the same ordered entries and
    both clones give the same words, in the TRLWE mode and the extract mode; the packed families give them again in one round.  The LWE family also has a row cut
    into chunks (the second-level lists pass through the shared image and its clone) and is held to exact arithmetic mod 2^64.  The packed families have no
    reference of their own here -- an error common to all four handles would pass: their words are held to the oracle in test_trlwe_linear.py and
    test_trlwe_gsw_linear.py."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    F = family(eng, np.random.default_rng(0xFA3117))
    handles = dict(F["handles"])
    for name, lin in F["handles"].items():
        handles[name + ", cloned"] = twin = F["clone"](lin)
        assert twin.h.value != lin.h.value and twin.info() == lin.info(), (name, twin.info(), lin.info())
    assert F["rounds"] in (None, COUNT), F["rounds"]
    try:
        for run in F["runs"]:
            if F["rounds"]:
                engine.set_tlwe_pack_workspace(F["workspace"])
            got = {name: ma.to_numpy(run(lin)) for name, lin in handles.items()}
            for group in F["groups"]:
                first = got[group[0]]
                if group[0] in F["want"]:
                    assert (first == F["want"][group[0]]).all(), "%s: %d words differ from the exact sums" % (group[0], (first != F["want"][group[0]]).sum())
                for name in [g + c for g in group for c in ("", ", cloned")][1:]:
                    assert got[name].shape == first.shape and (got[name] == first).all(), "%s against %s: %d words differ" % (name, group[0], (got[name] != first).sum())
            if F["rounds"]:
                engine.set_tlwe_pack_workspace(0)
                assert (ma.to_numpy(run(handles["dense"])) == got["dense"]).all(), "one round against three"
    finally:
        engine.set_tlwe_pack_workspace(0)
        for lin in handles.values():
            lin.close()
