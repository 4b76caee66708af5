"""Leveled look-up-table evaluation for a batch of INDEPENDENT TRGSW-encrypted inputs against one shared table (include/mosfhet_hip.h:
mosfhet_hip_leveled_lut_batch; mosfhet_amd/csrc/leveled_lut_kernels.h): eval_LUT of the reference's leveled application
(applications/leveled_lut/vertical_packing.c:36-52) per input.

The expected words of input b are the composition test_gpu_parity.py::test_leveled_lut_vertical_packing writes down -- the CMUX tree with oracle.external_product,
oracle.blind_rotate with a[i] = int2torus(2N - 2^i), oracle.trlwe_extract_tlwe -- with sel_dft = oracle.bk_to_dft(sel[b], 1, l).  Every GPU comparison is word for
word.  The decryption bound 2^(64 - prec - 1) is a condition on the INPUTS, which the oracle composition alone meets on the CPU with 6 bits or more to spare
(test_oracle_composition_decrypts); it is no tolerance on the GPU side.
"""
import ctypes as C
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (N, l, Bg_bit, sigma, size, prec, inputs, encrypted table, seed)
SETS = {
    "A": (1024, 3, 10, 2.0 ** -44, 13, 6, 33, False, 0x7E7),    # test_leveled_lut_vertical_packing's parameters
    "A'": (1024, 3, 10, 2.0 ** -44, 13, 6, 33, True, 0x7E8),    # ... with an encrypted table
    "B": (2048, 1, 23, 2.0 ** -52, 13, 4, 5, False, 1),         # the reference application's gadget
    "C": (2048, 4, 9, 2.0 ** -44, 12, 4, 5, False, 2),          # lvl2's gadget: a selector is 256 KiB
    "D": (1024, 2, 8, 2.0 ** -25, 12, 3, 5, False, 4),          # SET_1's gadget
    "E": (1024, 3, 10, 2.0 ** -44, 4, 3, 5, False, 5),          # no tree, fewer than log2 N rotation steps
    "F": (1024, 3, 10, 2.0 ** -44, 10, 6, 5, False, 6),         # no tree, all steps
    "G": (1024, 3, 10, 2.0 ** -44, 16, 6, 5, False, 7),         # 64 tables, 32 first-level nodes
}
_CACHE = {}


def _map(fn, items):
    with ThreadPoolExecutor(16) as ex:     # (the C oracle releases the GIL)
        return list(ex.map(fn, items))


def _composition(oracle, tabs, sel_dft, N, l, Bg, size):
    """eval_LUT restated with the oracle's pinned routines (tests/test_gpu_parity.py:3872-3881)"""
    log_N = N.bit_length() - 1
    T = tabs.copy()
    for i in range(max(0, size - log_N)):
        half = 1 << (size - log_N - i - 1)
        for j in range(half):
            T[j] = T[j] + oracle.external_product(T[j + half] - T[j], sel_dft[size - i - 1], l, Bg)
    steps = min(size, log_N)
    a = np.zeros(steps, dtype=np.uint64)
    for i in range(steps):
        a[i] = ((2 * N - (1 << i)) << (64 - (log_N + 1))) % 2 ** 64
    return oracle.trlwe_extract_tlwe(oracle.blind_rotate(T[0], a, sel_dft[:steps], l, Bg), 0)


def _case(oracle, name):
    """key, table, indices, selectors and the oracle's outputs of a parameter set (cached: the CPU test and the GPU tests of one run share them)"""
    if name in _CACHE:
        return _CACHE[name]
    N, l, Bg, sigma, size, prec, n_inputs, encrypted, seed = SETS[name]
    log_N = N.bit_length() - 1
    r = oracle.Rng(seed)
    s = oracle.gen_binary_key(r, N).reshape(1, N)
    lut = (oracle.u64(r.words(1 << max(size, log_N))) % np.uint64(1 << prec)).astype(np.uint64)
    n_luts = max(1, (1 << size) >> log_N)
    msg = (lut << np.uint64(64 - prec)).reshape(n_luts, N)
    tabs = np.zeros((n_luts, 2, N), dtype=np.uint64)
    if encrypted:
        for j in range(n_luts):
            tabs[j] = oracle.trlwe_sample(r, msg[j].copy(), s, sigma)
    else:
        tabs[:, 1, :] = msg
    rng = np.random.default_rng(seed)
    m = [int(rng.integers(0, 1 << size)) for _ in range(n_inputs)]
    sel = np.stack([np.stack([oracle.trgsw_monomial_sample(r, (m[b] >> i) & 1, 0, s, l, Bg, sigma) for i in range(size)]) for b in range(n_inputs)])
    want = np.stack(_map(lambda b: _composition(oracle, tabs, oracle.bk_to_dft(sel[b], 1, l), N, l, Bg, size), range(n_inputs)))
    _CACHE[name] = dict(N=N, l=l, Bg=Bg, size=size, prec=prec, s=s, lut=lut, tabs=tabs, m=m, sel=sel, want=want)
    return _CACHE[name]


def _assert_decrypts(oracle, S, outs, idx, what):
    for b, out in zip(idx, outs):
        d = float(oracle.torus_dist(oracle.tlwe_phase(out, S["s"][0]), int(S["lut"][S["m"][b]]) << (64 - S["prec"])))
        assert d < 2.0 ** (64 - S["prec"] - 1), "%s, input %d: 2^%.1f from LUT[m]" % (what, b, np.log2(max(d, 1.0)))


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_leveled_lut_symbols_and_argument_checks(native_lib):
    """The library exports the entry points, and mosfhet_hip_leveled_lut_batch refuses a null context, size 0 and past the bound, N = 512 and 4096 and
    l * Bg_bit >= 64 with MOSFHET_HIP_EINVAL and a message naming the argument -- before any HIP call (this runs without a GPU)."""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_leveled_lut_batch", "mosfhet_hip_leveled_lut_plan", "mosfhet_hip_set_leveled_lut_workspace", "mosfhet_eval_LUT_inputs"):
        assert hasattr(native_lib, name), name
    f = native_lib.mosfhet_hip_leveled_lut_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)     # never dereferenced: every call below fails on its arguments
    bound = 10 + engine.LEVELED_LUT_MAX_LEVELS
    assert f(None, fake, fake, fake, 13, 1024, 3, 10, 4, None) == -1 and "ctx" in err()
    assert f(fake, fake, fake, fake, 0, 1024, 3, 10, 4, None) == -1 and "size = 0" in err()
    assert f(fake, fake, fake, fake, bound + 1, 1024, 3, 10, 4, None) == -1 and "size = %d" % (bound + 1) in err()
    assert f(fake, fake, fake, fake, bound + 2, 2048, 3, 10, 4, None) == -1 and "size = %d" % (bound + 2) in err()
    assert f(fake, fake, fake, fake, 13, 512, 3, 10, 4, None) == -1 and "N = 512" in err()
    assert f(fake, fake, fake, fake, 13, 4096, 3, 10, 4, None) == -1 and "N = 4096" in err()
    assert f(fake, fake, fake, fake, 13, 1024, 4, 16, 4, None) == -1 and "l=4 Bg_bit=16" in err()
    assert f(fake, fake, fake, fake, 13, 1024, 3, 10, -1, None) == -1 and "count = -1" in err()
    plan = (C.c_longlong * 4)()
    assert native_lib.mosfhet_hip_leveled_lut_plan(1024, 3, 13, 4, 256, None) == -1
    assert native_lib.mosfhet_hip_leveled_lut_plan(4096, 1, 13, 4, 256, plan) == -1 and "N = 4096" in err()
    assert native_lib.mosfhet_hip_leveled_lut_plan(1024, 3, 13, 0, 256, plan) == -1 and "count = 0" in err()
    assert native_lib.mosfhet_hip_leveled_lut_plan(1024, 3, 13, 4, 0, plan) == -1 and "cus = 0" in err()
    assert native_lib.mosfhet_hip_set_leveled_lut_workspace(C.c_longlong(-1)) == -1


def test_leveled_lut_plan_sweep(native_lib):
    """mosfhet_hip_leveled_lut_plan -- the function the launcher decides with -- over both rings, every size up to the bound, small and large batches and a device of
    256 and of 64 CUs: levels = max(0, size - log2 N), first-level nodes = 2^(levels - 1) (0 without a tree), chunks of whole inputs that cover the batch, the
    workspace = prepared rows + one chunk's intermediates, within the bound (1 GiB by default; lowered: more chunks, never a larger workspace)."""
    from mosfhet_amd import engine
    GiB = 1 << 30
    for cus in (256, 64):
        for N in (1024, 2048):
            log_N = N.bit_length() - 1
            for l in (1, 3, 6):
                for size in range(1, log_N + engine.LEVELED_LUT_MAX_LEVELS + 1):
                    for count in (1, 3, 257, 1024, 4096):
                        p = engine.leveled_lut_plan(N, l, size, count, cus)
                        what = (cus, N, l, size, count, p)
                        levels = max(0, size - log_N)
                        nodes = (1 << (levels - 1)) if levels else 0
                        assert p["levels"] == levels and p["nodes"] == nodes, what
                        assert 1 <= p["chunk"] <= count, what
                        assert p["chunk"] * -(-count // p["chunk"]) >= count, what
                        table, per_input = nodes * 2 * l * (N // 2) * 16, nodes * 2 * N * 8
                        assert p["workspace_bytes"] == table + p["chunk"] * per_input, what
                        assert p["workspace_bytes"] <= GiB, what
                        # a chunk is as large as the bound allows: the whole batch, or one more input would not fit
                        assert p["chunk"] == count or table + (p["chunk"] + 1) * per_input > GiB, what
                        assert p == engine.leveled_lut_plan(N, l, size, count, 256), what     # the CU count sizes grids only
    try:
        p0 = engine.leveled_lut_plan(1024, 3, 16, 5)
        per_input, table = 32 * 2 * 1024 * 8, 32 * 6 * 512 * 16
        assert p0 == dict(levels=6, nodes=32, chunk=5, workspace_bytes=table + 5 * per_input)
        engine.set_leveled_lut_workspace(table + 2 * per_input)
        assert engine.leveled_lut_plan(1024, 3, 16, 5) == dict(levels=6, nodes=32, chunk=2, workspace_bytes=table + 2 * per_input)
        engine.set_leveled_lut_workspace(table)                 # not even one input: refused, not overrun
        with pytest.raises(engine.MosfhetHipError, match="workspace bound"):
            engine.leveled_lut_plan(1024, 3, 16, 5)
        assert engine.leveled_lut_plan(1024, 3, 10, 5)["workspace_bytes"] == 0      # no tree, no workspace
    finally:
        engine.set_leveled_lut_workspace(0)
    assert engine.leveled_lut_plan(1024, 3, 16, 5) == p0
    with pytest.raises(engine.MosfhetHipError):
        engine.leveled_lut_plan(1024, 3, 10 + engine.LEVELED_LUT_MAX_LEVELS + 1, 1)


@pytest.mark.parametrize("name", list(SETS))
def test_oracle_composition_decrypts(oracle, name):
    """The condition on the inputs, proven on the CPU: the oracle composition alone decrypts every input of every set to LUT[m] within 2^(64 - prec - 1)."""
    S = _case(oracle, name)
    worst = max(float(oracle.torus_dist(oracle.tlwe_phase(S["want"][b], S["s"][0]), int(S["lut"][S["m"][b]]) << (64 - S["prec"]))) for b in range(len(S["m"])))
    print("set %s: worst log2 torus_dist(phase, LUT[m]) = %.1f, bound %d" % (name, np.log2(max(worst, 1.0)), 64 - S["prec"] - 1))
    _assert_decrypts(oracle, S, S["want"], range(len(S["m"])), "oracle composition of set " + name)


def test_leveled_lut_kernels_of_the_build(native_lib):
    """tools/check_lds_barriers.py lists the leveled-LUT form and finds nothing; the built library's kernel table holds the six new kernels -- prepare, level 0 and
    CMUX / finish, per ring, run-time gadget -- and fewer than 330 kernels in all."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_lds_barriers as chk
    import kernel_table
    assert any("leveled LUT" in f[0] for f in chk.FORMS), [f[0] for f in chk.FORMS]
    assert chk.build_and_check([f for f in chk.FORMS if "leveled LUT" in f[0]]) == []
    rows = kernel_table.table()
    by_name = {r["name"].replace("> >", ">>"): r for r in rows}       # (the demangler's spelling of nested template arguments)
    kernels = ("lut_prepare_kernel", "lut_level0_kernel", "lut_cmux_kernel")
    for kernel in kernels:
        for ring in ("Fft1024", "Fft2048T<false, false>"):
            name = "%s<%s>" % (kernel, ring)
            assert name in by_name, (name, sorted(n for n in by_name if n.startswith(kernels)))
            r = by_name[name]
            print("%-50s vgpr %3d  agpr %3d  sgpr %3d  lds %6d  scratch %4d" % (name, r["vgpr"], r["agpr"], r["sgpr"], r["lds"], r["scratch"]))
            assert r["lds"] <= 64 * 1024 and r["vgpr"] <= 256, r
    assert sorted(n for n in by_name if n.startswith(kernels)) == sorted("%s<%s>" % (k, f) for k in kernels for f in ("Fft1024", "Fft2048T<false, false>"))
    print("%d kernels in the library" % len(rows))
    assert len(rows) < 330, len(rows)


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


def _sel_dft(eng, sel):
    """[count][size][2l][2][N] torus words -> the same shape in the DFT domain, on the device"""
    import mosfhet_amd as ma
    return eng.trgsw_to_dft(ma.to_device(sel, eng.device))


def _run(eng, S, idx=None):
    import mosfhet_amd as ma
    sel = S["sel"] if idx is None else S["sel"][idx]
    return ma.to_numpy(eng.leveled_lut(_sel_dft(eng, sel), ma.to_device(S["tabs"], eng.device), S["size"], S["l"], S["Bg"]))


def _assert_words(got, want, what):
    bad = [b for b in range(len(want)) if not (got[b] == want[b]).all()]
    assert not bad, "%s: %d of %d outputs differ from the oracle (first: %s)" % (what, len(bad), len(want), bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "A'"])
def test_leveled_lut_matches_the_oracle(eng, oracle, name):
    """33 independent inputs of set A against a trivial and against an encrypted table: every output word equals the oracle's, every output decrypts to
    LUT[m_b], and the table on the device is unchanged afterwards."""
    import mosfhet_amd as ma
    S = _case(oracle, name)
    d_lut = ma.to_device(S["tabs"], eng.device)
    got = ma.to_numpy(eng.leveled_lut(_sel_dft(eng, S["sel"]), d_lut, S["size"], S["l"], S["Bg"]))
    _assert_words(got, S["want"], "set " + name)
    _assert_decrypts(oracle, S, got, range(len(S["m"])), "set " + name)
    assert (ma.to_numpy(d_lut) == S["tabs"]).all(), "the table was modified"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B", "C", "D", "E", "F", "G"])
def test_leveled_lut_parameter_sets(eng, oracle, name):
    """Both rings, the gadgets of the reference application, lvl2 and SET_1, tables without a tree (with fewer than log2 N and with all rotation steps) and a
    64-table tree, bit for bit; the 64-table tree also with the workspace bound lowered so that 5 inputs take three chunks."""
    from mosfhet_amd import engine
    S = _case(oracle, name)
    got = _run(eng, S)
    _assert_words(got, S["want"], "set " + name)
    _assert_decrypts(oracle, S, got, range(len(S["m"])), "set " + name)
    if name == "G":
        p = eng.leveled_lut_plan(S["N"], S["l"], S["size"], 5)
        per_input = p["nodes"] * 2 * S["N"] * 8
        try:
            engine.set_leveled_lut_workspace(p["workspace_bytes"] - 3 * per_input)
            assert eng.leveled_lut_plan(S["N"], S["l"], S["size"], 5)["chunk"] == 2
            _assert_words(_run(eng, S), S["want"], "set G in chunks of two inputs")
        finally:
            engine.set_leveled_lut_workspace(0)


@pytest.mark.gpu
def test_leveled_lut_words_do_not_depend_on_the_batch_size(eng, oracle):
    """Set A at batch sizes 1, 3, CUs + 1 and 1024, tiled from 16 distinct inputs (the selectors are tiled on the device: 1.3 GB at 1024): the outputs are the 16
    expected rows tiled, so no word depends on the batch size, on the level-0 slicing or on the chunking."""
    import torch
    import mosfhet_amd as ma
    S = _case(oracle, "A")
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    sel16 = _sel_dft(eng, S["sel"][:16])
    d_lut = ma.to_device(S["tabs"], eng.device)
    for B in (1, 3, cus + 1, 1024):
        idx = np.arange(B) % 16
        sel = sel16[torch.from_numpy(idx).to(eng.device)].contiguous()
        got = ma.to_numpy(eng.leveled_lut(sel, d_lut, S["size"], S["l"], S["Bg"]))
        del sel
        _assert_words(got, S["want"][idx], "%d inputs tiled from 16" % B)


@pytest.mark.gpu
def test_leveled_lut_equals_the_existing_route(eng, oracle):
    """Four inputs of set A through the entry points that existed before -- a key view per input, one cmux launch per tree level, blind_rotate_,
    trlwe_extract_tlwe -- give the words of the new call: it computes nothing a caller could not already compute."""
    import mosfhet_amd as ma
    S = _case(oracle, "A")
    N, l, Bg, size = S["N"], S["l"], S["Bg"], S["size"]
    log_N = N.bit_length() - 1
    sel_dft = _sel_dft(eng, S["sel"][:4])
    new = ma.to_numpy(eng.leveled_lut(sel_dft, ma.to_device(S["tabs"], eng.device), size, l, Bg))
    a = np.zeros(size + 1, dtype=np.uint64)
    for i in range(log_N):
        a[i] = ((2 * N - (1 << i)) << (64 - (log_N + 1))) % 2 ** 64
    d_a = ma.to_device(a[None], eng.device)
    for b in range(4):
        key = eng.bootstrap_key_view(sel_dft[b], 1, l, Bg)
        d = ma.to_device(S["tabs"], eng.device)
        for i in range(size - log_N):
            half = 1 << (size - log_N - i - 1)
            eng.cmux(key, size - i - 1, d[:half], d[half:2 * half], out=d[:half])
        acc = d[:1].contiguous()
        eng.blind_rotate_(key, acc, d_a)
        old = ma.to_numpy(eng.trlwe_extract_tlwe(acc, 0))[0]
        key.free()
        assert (old == new[b]).all(), "input %d: the new call differs from cmux / blind_rotate_ / extract" % b
    _assert_words(new, S["want"][:4], "four inputs of set A")


@pytest.mark.gpu
def test_circuit_bootstrap_output_is_the_selector_layout(eng, oracle):
    """Plumbing from BASELINE configs[3] at set C's ring and gadget (lvl2): circuit_bootstrap_3 on 8 x size LWE encryptions of bits -> trgsw_to_dft
    (mosfhet_hip_torus_to_dft_batch) -> leveled_lut, with no repacking in between, against oracle.circuit_bootstrap_3 + bk_to_dft + the composition.  The cheap key
    set of test_by_component_circuit_bootstrap_3 (one-digit packing key): words are compared, nothing is decrypted."""
    import mosfhet_amd as ma
    from test_gpu_parity import _keyset
    K = _keyset("lvl2", eng, oracle)
    P = K["P"]
    N, l, Bg, size, count = P["N"], P["l"], P["Bg_bit"], 12, 8
    key, _ = eng.clone_key(K["bsk"])
    key.set_product_order("reference")
    r = oracle.Rng(0xCB3)
    s = np.ascontiguousarray(K["rk"].s[0], dtype=np.uint64)
    lwe_s = np.ascontiguousarray(K["lk"].s, dtype=np.uint64)
    ks0, ks1 = oracle.gen_priv_ks_key(r, s, s, 20, 2, P["rlwe_sigma"])
    kskb = oracle.gen_packing1_ks_key(r, s, s, 1, 2, P["rlwe_sigma"])
    kska, pk = eng.load_trlwe_ks_keys(np.stack([ks0, ks1]), 2), eng.load_packing1_key(kskb, 2)
    ks0_dft, ks1_dft = oracle.ks_to_dft(ks0), oracle.ks_to_dft(ks1)
    rng = np.random.default_rng(0xCB3)
    m = [int(rng.integers(0, 1 << size)) for _ in range(count)]
    cts = np.stack([oracle.tlwe_sample(r, oracle.double2torus(0.25 * ((m[b] >> i) & 1)), lwe_s, P["lwe_sigma"]) for b in range(count) for i in range(size)])
    tabs = np.zeros((max(1, (1 << size) // N), 2, N), dtype=np.uint64)
    tabs[:, 1, :] = (oracle.u64(r.words(tabs.shape[0] * N)) << np.uint64(60)).reshape(tabs.shape[0], N)
    want_sel = np.stack(_map(lambda u: oracle.circuit_bootstrap_3(cts[u], K["bk_dft"], ks0_dft, ks1_dft, 2, kskb, 2, l, Bg), range(count * size)))
    want_sel = want_sel.reshape(count, size, 2 * l, 2, N)
    want = np.stack(_map(lambda b: _composition(oracle, tabs, oracle.bk_to_dft(want_sel[b], 1, l), N, l, Bg, size), range(count)))
    trgsw = eng.circuit_bootstrap_3(key, kska, pk, ma.to_device(cts, eng.device))            # [count * size][2l][2][N]
    assert (ma.to_numpy(trgsw).reshape(want_sel.shape) == want_sel).all(), "circuit_bootstrap_3 differs from the oracle"
    sel_dft = eng.trgsw_to_dft(trgsw).reshape(count, size, 2 * l, 2, N)                      # a view: the circuit bootstrap's output IS the selector layout
    got = ma.to_numpy(eng.leveled_lut(sel_dft, ma.to_device(tabs, eng.device), size, l, Bg))
    _assert_words(got, want, "8 inputs from circuit_bootstrap_3")
    for h in (kska, pk, key):
        h.free()


@pytest.mark.gpu
def test_eval_LUT_inputs_through_the_host_structs(native_lib, tmp_path):
    """tests/c/leveled_lut_inputs.c: mosfhet_eval_LUT_inputs on 8 inputs of set B's parameters equals the reference's own eval_LUT loop written against
    include/mosfhet.h (trlwe_sub / trgsw_mul_trlwe_DFT / trlwe_from_DFT / trlwe_add, blind_rotate, trlwe_extract_tlwe) word for word, decrypts to the table entry,
    and leaves LUT as it was."""
    exe = str(tmp_path / "leveled_lut_inputs")
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "leveled_lut_inputs.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and "leveled_lut_inputs ok" in r.stdout, r.stdout[-3000:]
