"""Packed TRLWE samples opened into LWE batches on the device (include/mosfhet_hip.h: mosfhet_hip_trlwe_unpack_batch, mosfhet_hip_trlwe_unpack_keyswitch_batch,
mosfhet_hip_unpack_keyswitch_functional_bootstrap_batch, mosfhet_hip_trlwe_unpack_plan; mosfhet_amd/csrc/capi_unpack.inc, unpack_kernels.h;
include/mosfhet_compat.h: mosfhet_trlwe_unpack, mosfhet_trlwe_unpack_keyswitch).

Expected words come from tests/unpacking_reference.py, a numpy restatement of the reference's trlwe_extract_tlwe over a batch, held here to the project's oracle, to
the reference's own function and to oracle.poly_mul_by_xai; the key switch of its rows goes through oracle.tlwe_keyswitch.  Everything is integer work: every
comparison of device words is == on all words.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
_CACHE = {}
SENTINEL = np.uint64(0xA5A5A5A55A5A5A5A)


def _log2(x):
    return float(np.log2(max(float(x), 1.0)))


def _packed(oracle, N, outputs, seed=0):
    """`outputs` packed samples of random words [outputs][2][N], made once and left unchanged"""
    key = ("packed", N, outputs, seed)
    if key not in _CACHE:
        _CACHE[key] = oracle.Rng(0x0DDBA11 + 7 * N + outputs + 1000 * seed).words(outputs * 2 * N).reshape(outputs, 2, N)
    return _CACHE[key]


def _rows(oracle, N, total, per, seed=0):
    """the helper's batch for _packed(N, ceil(total / per)), cached"""
    import unpacking_reference
    key = ("rows", N, total, per, seed)
    if key not in _CACHE:
        _CACHE[key] = unpacking_reference.unpack_batch(_packed(oracle, N, -(-total // per), seed), total, per)
    return _CACHE[key]


def _switch_key(oracle, N, n_out, t, base_bit):
    """an oracle-made LWE -> LWE table key N -> n_out [N][t][2^base_bit - 1][n_out + 1] with its binary keys"""
    key = ("ksk", N, n_out, t, base_bit)
    if key not in _CACHE:
        rng = oracle.Rng(0x5EED + N + 31 * n_out + 7 * t + base_bit)
        s_in, s_out = oracle.gen_binary_key(rng, N), oracle.gen_binary_key(rng, n_out)
        _CACHE[key] = dict(s_in=s_in, s_out=s_out, rows=oracle.gen_tlwe_ks_key(rng, s_in, s_out, t, base_bit, 2.0 ** -40))
    return _CACHE[key]


def _switched(oracle, K, rows, n_out, t, base_bit):
    return np.stack([oracle.tlwe_keyswitch(r, K["rows"], n_out, t, base_bit) for r in rows])


# the composition of tests 7, 12 and 13: N = 1024, n = 24, l = 2, Bg_bit = 8, switch t = 4, base_bit = 4, all noises 2^-40, 16 slots, 70 values in two inputs of 40
BOOT = dict(N=1024, n=24, l=2, Bg_bit=8, t=4, base_bit=4, sigma=2.0 ** -40, slots=16, total=70, per=40)
HALF_SLOT_16 = 2.0 ** 59      # table entries on multiples of 1/16
MARGIN_BITS = 2


def _boot_case(oracle):
    """keys, table and encrypted inputs of the composition, made once by the oracle's generators (oracle.trlwe_sample for the inputs) and left unchanged"""
    if "boot" not in _CACHE:
        B = BOOT
        N, n, total, per = B["N"], B["n"], B["total"], B["per"]
        rng = oracle.Rng(0xB007CA5E)
        s_lwe, s_ring = oracle.gen_binary_key(rng, n), oracle.gen_binary_key(rng, N)
        bk = oracle.gen_bootstrap_key(rng, s_lwe, s_ring.reshape(1, N), B["l"], B["Bg_bit"], B["sigma"])
        ksk = oracle.gen_tlwe_ks_key(rng, s_ring, s_lwe, B["t"], B["base_bit"], B["sigma"])
        lut = (rng.words(16) % np.uint64(16)) << np.uint64(60)
        msgs = rng.words(total) % np.uint64(16)
        outputs = -(-total // per)
        packed = np.empty((outputs, 2, N), dtype=np.uint64)
        for o in range(outputs):
            m = (rng.words(N) % np.uint64(16)) << np.uint64(59)          # slot s of 16 is the phase s / 32; the coefficients past `per` carry values nobody opens
            have = min(per, total - o * per)
            m[:have] = msgs[o * per:o * per + have] << np.uint64(59)
            packed[o] = oracle.trlwe_sample(rng, m, s_ring.reshape(1, N), B["sigma"])
        _CACHE["boot"] = dict(s_lwe=s_lwe, s_ring=s_ring, bk=bk, bk_dft=oracle.bk_to_dft(bk, 1, B["l"]), ksk=ksk, lut=lut, tv=oracle.trlwe_torus_packing(lut, 1, N),
                              msgs=msgs, expect=lut[msgs.astype(np.int64)], packed=packed)
    return _CACHE["boot"]


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_helper_against_the_oracle_and_the_rotations(oracle):
    """unpacking_reference.unpack_batch == oracle.trlwe_extract_tlwe on every (input, j) of a ragged batch (N = 256, per = 67, the last input opened to 5), and column
    i of an input's full batch == oracle.poly_mul_by_xai(a, i) for every i: the orientation the key switch wants is the negacyclic rotations of the mask."""
    import unpacking_reference
    N, per, total = 256, 67, 3 * 67 + 5
    P, got = _packed(oracle, N, 4), _rows(oracle, N, total, per)
    assert got.shape == (total, N + 1)
    for c in range(total):
        assert (got[c] == oracle.trlwe_extract_tlwe(P[c // per], c % per)).all(), c
    full = unpacking_reference.unpack(P[1])
    for i in range(N):
        assert (full[:, i] == oracle.poly_mul_by_xai(P[1][0], i)).all(), i
    assert (full[:, N] == P[1][1]).all()
    assert (unpacking_reference.unpack_batch(P, 0, 5).shape == (0, N + 1))


@pytest.mark.parametrize("backend", ["avx512", "ffnt"])
def test_helper_against_the_reference(oracle, backend):
    """unpacking_reference.unpack_batch == the reference's own trlwe_extract_tlwe (both builds of oracle/_ref, through ctypes) on every (input, j) of the ragged batch
    of N = 256 and on inputs of N = 1024 at j in {0, 1, 511, 1023}: pure integer work, so == on all words."""
    from oracle import reflib
    if not reflib.available(backend):
        pytest.skip("oracle/_ref/libmosfhet_ref_%s.so is absent (or this CPU lacks AVX-512)" % backend)
    ref = reflib.get(backend)
    if not ref.has("ref_trlwe_extract_tlwe"):
        pytest.skip("the reference build does not export trlwe_extract_tlwe")
    N, per, total = 256, 67, 3 * 67 + 5
    P, got = _packed(oracle, N, 4), _rows(oracle, N, total, per)
    for c in range(total):
        assert (got[c] == ref.trlwe_extract_tlwe(P[c // per], c % per)).all(), (backend, c)
    N = 1024
    P, got = _packed(oracle, N, 2), _rows(oracle, N, 1025, N)
    for c in (0, 1, 511, 1023, 1024):
        assert (got[c] == ref.trlwe_extract_tlwe(P[c // N], c % N)).all(), (backend, c)


def test_unpack_symbols_and_argument_checks(native_lib):
    """The library exports the four entry points and the host face, the binding its functions; every scalar refusal returns MOSFHET_HIP_EINVAL with a message naming
    the argument and its value -- on fake pointers, before any handle is read and before any HIP call (this runs without a GPU); total == 0 is OK."""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_trlwe_unpack_batch", "mosfhet_hip_trlwe_unpack_keyswitch_batch", "mosfhet_hip_unpack_keyswitch_functional_bootstrap_batch",
                 "mosfhet_hip_trlwe_unpack_plan", "mosfhet_trlwe_unpack", "mosfhet_trlwe_unpack_keyswitch"):
        assert hasattr(native_lib, name), name
    assert hasattr(engine, "trlwe_unpack_plan")
    for name in ("trlwe_unpack", "trlwe_unpack_keyswitch", "unpack_keyswitch_functional_bootstrap"):
        assert hasattr(engine.Engine, name), name
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)     # never dereferenced: every call below ends on its scalar arguments
    f = native_lib.mosfhet_hip_trlwe_unpack_batch
    f.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_int, C.c_void_p]
    assert f(None, fake, fake, 1024, 1, 1, None) == EINVAL and "ctx" in err()
    assert f(fake, fake, fake, 1024, 1, 0, None) == EINVAL and "per = 0" in err()
    assert f(fake, fake, fake, 1024, 1, -3, None) == EINVAL and "per = -3" in err()
    assert f(fake, fake, fake, 1024, 1, 1025, None) == EINVAL and "per = 1025" in err()
    assert f(fake, fake, fake, 256, 1, 257, None) == EINVAL and "per = 257" in err()
    assert f(fake, fake, fake, 1024, -1, 1, None) == EINVAL and "total = -1" in err()
    for N in (128, 8192, 1000, 0, -256):
        assert f(fake, fake, fake, N, 1, 1, None) == EINVAL and "N = %d" % N in err(), N
    assert f(fake, None, fake, 1024, 1, 1, None) == EINVAL and "null buffer" in err()
    assert f(fake, fake, None, 1024, 1, 1, None) == EINVAL and "null buffer" in err()
    assert f(fake, fake, fake, 1024, 0, 1, None) == 0                      # total == 0: nothing to do
    assert f(fake, None, None, 4096, 0, 4096, None) == 0
    assert f(fake, fake, fake, 1024, 0, 0, None) == EINVAL and "per = 0" in err()      # ... after the scalar checks
    g = native_lib.mosfhet_hip_trlwe_unpack_keyswitch_batch
    g.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p]
    assert g(None, fake, fake, fake, 1, 1, None) == EINVAL and "ctx" in err()
    assert g(fake, None, fake, fake, 1, 1, None) == EINVAL and "ksk" in err()
    assert g(fake, fake, fake, fake, 1, 0, None) == EINVAL and "per = 0" in err()
    assert g(fake, fake, fake, fake, 1, 4097, None) == EINVAL and "per = 4097" in err()
    assert g(fake, fake, fake, fake, -1, 1, None) == EINVAL and "total = -1" in err()
    assert g(fake, fake, fake, fake, 0, 1, None) == 0
    h = native_lib.mosfhet_hip_unpack_keyswitch_functional_bootstrap_batch
    h.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    assert h(None, fake, fake, fake, fake, 1, fake, 1, 1, 4, 1, None) == EINVAL and "ctx" in err()
    assert h(fake, None, fake, fake, fake, 1, fake, 1, 1, 4, 1, None) == EINVAL and "null key" in err()
    assert h(fake, fake, None, fake, fake, 1, fake, 1, 1, 4, 1, None) == EINVAL and "null key" in err()
    assert h(fake, fake, fake, fake, fake, 1, fake, 1, 0, 4, 1, None) == EINVAL and "per = 0" in err()
    assert h(fake, fake, fake, fake, fake, 1, fake, -2, 1, 4, 1, None) == EINVAL and "total = -2" in err()
    p = native_lib.mosfhet_hip_trlwe_unpack_plan
    p.argtypes = [C.c_int] * 8 + [C.c_void_p]
    plan = (C.c_longlong * 8)()
    assert p(1024, 0, 0, 0, 0, 10, 5, 256, None) == EINVAL and "plan" in err()
    for N in (128, 8192, 1000):
        assert p(N, 0, 0, 0, 0, 10, 5, 256, plan) == EINVAL and "N = %d" % N in err()
    assert p(1024, -1, 0, 0, 0, 10, 5, 256, plan) == EINVAL and "n_out = -1" in err()
    assert p(1024, 16, 0, 2, 0, 10, 5, 256, plan) == EINVAL and "t = 0" in err()
    assert p(1024, 16, 2, 9, 0, 10, 5, 256, plan) == EINVAL and "base_bit = 9" in err()
    assert p(1024, 16, 2, 2, 0, -1, 5, 256, plan) == EINVAL and "total = -1" in err()
    assert p(1024, 16, 2, 2, 0, 10, 0, 256, plan) == EINVAL and "per = 0" in err()
    assert p(1024, 16, 2, 2, 0, 10, 1025, 256, plan) == EINVAL and "per = 1025" in err()
    assert p(1024, 16, 2, 2, 0, 10, 5, 0, plan) == EINVAL and "cus = 0" in err()
    # byte counts past 2^63: the switched batch of 2^31 - 1 samples of 2^31 words; the largest batch part 1 can be asked for (2^31 - 1 samples at N = 4096) fits
    assert p(4096, 2 ** 31 - 1, 2, 2, 0, 2 ** 31 - 1, 1, 256, plan) == EINVAL and "64-bit byte count" in err()
    assert p(4096, 0, 0, 0, 0, 2 ** 31 - 1, 1, 256, plan) == 0 and plan[4] == (2 ** 31 - 1) * 4097 * 8
    assert p(1024, 16, 2, 2, 0, 0, 5, 256, plan) == 0 and list(plan)[:7] == [0] * 7       # total == 0: no input, no launch


def test_unpack_plan_is_a_pure_function(native_lib):
    """mosfhet_hip_trlwe_unpack_plan -- the function the launchers decide with: fixed arguments give fixed plans and nothing is launched (no device here); the form
    follows launch_tlwe_keyswitch's limits -- up to 16 samples the direct kernels (unpacked first, into the pool), then mosfhet_hip_ks_words_plan's `applies`, else
    tiles of 512 for base_bit >= 3 and more than 256 samples or base_bit > 4, else tiles of 256 -- at the current set_ks_words; pieces = ceil(total / 8192) in the
    word-lane form; the byte counts are those of the layouts."""
    from mosfhet_amd import engine
    P = engine.trlwe_unpack_plan
    a = P(1024, 585, 5, 2, 4096, 1024)
    assert a == P(1024, 585, 5, 2, 4096, 1024), a
    assert a == dict(outputs=4, form="words", pieces=1, prepass_workgroups=64 * 16, prepass_bytes=1024 * 5 * 64 * 64 * 2 + 4096 * 8, saved_bytes=4096 * 1025 * 8,
                     pool_bytes=0, rows_per_workgroup=8), a
    assert P(1024, total=4096, per=1024) == dict(outputs=4, form="small", pieces=1, prepass_workgroups=4 * 128, prepass_bytes=4096 * 1025 * 8, saved_bytes=0, pool_bytes=0,
                                                 rows_per_workgroup=8)
    assert P(2048, total=2049, per=2048, cus=1)["rows_per_workgroup"] == 64 and P(2048, total=2049, per=2048, cus=1)["prepass_workgroups"] == 2 * 32
    assert P(256, 16, 2, 2, 9, 4) == dict(outputs=3, form="small", pieces=1, prepass_workgroups=3, prepass_bytes=9 * 257 * 8, saved_bytes=0, pool_bytes=9 * 257 * 8,
                                          rows_per_workgroup=8)
    kp = native_lib.mosfhet_hip_ks_words_plan
    kp.argtypes = [C.c_int] * 6 + [C.c_void_p]
    words = (C.c_longlong * 8)()

    def expected_form(N, n_out, t, bb, compressed, total):
        if total <= 16:
            return "small"
        assert kp(total, N, n_out + 1, t, bb, int(compressed), words) == 0
        if words[0]:
            return "words"
        return "tiles_512" if bb >= 3 and (total > 256 or bb > 4) else "tiles_256"

    checked = 0
    try:
        for setting in (-1, 0, 100):
            engine.set_ks_words(setting)
            for N, n_out in ((256, 16), (1024, 585), (2048, 632)):
                for t, bb in ((2, 2), (3, 4), (5, 3), (2, 6), (1, 8), (7, 1)):
                    for compressed in (False, True):
                        for total in (1, 16, 17, 70, 99, 100, 256, 257, 300, 8192, 8193, 8192 + 70, 3 * 8192):
                            per = min(N, 67)
                            p = P(N, n_out, t, bb, total, per, compressed)
                            what = (setting, N, n_out, t, bb, compressed, total, p)
                            assert p == P(N, n_out, t, bb, total, per, compressed), what
                            assert p["outputs"] == -(-total // per), what
                            assert p["form"] == expected_form(N, n_out, t, bb, compressed, total), what
                            batch = total * (N + 1) * 8
                            if p["form"] == "small":
                                assert (p["pieces"], p["prepass_bytes"], p["saved_bytes"], p["pool_bytes"]) == (1, batch, 0, batch), what
                            else:
                                assert (p["saved_bytes"], p["pool_bytes"]) == (batch, 0), what
                                assert p["pieces"] == (-(-total // 8192) if p["form"] == "words" else 1), what
                            if p["form"].startswith("tiles"):
                                assert p["prepass_bytes"] == batch and p["prepass_workgroups"] == -(-total // 256) * -(-(N + 1) // 16), what
                            if p["form"] == "words":
                                waves = sum(-(-min(8192, total - f) // 64) for f in range(0, total, 8192))
                                assert p["prepass_workgroups"] == waves * (N // 64) and p["prepass_bytes"] == N * t * waves * 64 * 2 + total * 8, what
                            checked += 1
    finally:
        engine.set_ks_words(-1)
    assert checked > 1000
    assert P(256, 16, 2, 2, 70, 67)["form"] == "words" and P(256, 16, 2, 2, 70, 67, compressed=True)["form"] == "tiles_256"      # (seed-compressed LWE rows stay with the tiles)


def test_unpack_kernels_of_the_build(native_lib):
    """tools/kernel_table.py lists trlwe_unpack_kernel once (one kernel for both orientations) and the packed entries kernel once, at most 256 VGPRs, without scratch;
    the library holds fewer than 330 kernels; tools/check_lds_barriers.py finds nothing on a build of its own."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    import check_lds_barriers
    rows = kernel_table.table()
    for name in ("trlwe_unpack_kernel", "ks_words_entries_packed_kernel"):
        mine = [r for r in rows if r["name"].startswith(name)]
        for r in mine:
            print("%-60s vgpr %3d  agpr %3d  sgpr %3d  lds %6d  scratch %4d" % (r["name"], r["vgpr"], r["agpr"], r["sgpr"], r["lds"], r["scratch"]))
        assert len(mine) == 1, (name, mine)
        assert mine[0]["vgpr"] <= 256 and mine[0]["scratch"] == 0, mine
    print("%d kernels" % len(rows))
    assert len(rows) < 330, len(rows)
    assert check_lds_barriers.build_and_check() == []


def _compile_c(tmp_path):
    exe = str(tmp_path / "trlwe_unpack")
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "trlwe_unpack.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_unpack_c_program_compiles_and_links(native_lib, tmp_path):
    """tests/c/trlwe_unpack.c compiles against include/mosfhet.h and links against the built library (its device part: test_unpack_host_face)."""
    assert os.path.exists(_compile_c(tmp_path))


def test_unpack_sharding_cuts_at_whole_inputs(oracle):
    """shard_bounds_whole with unit = per: every rank opens whole inputs (lo is a multiple of per), and the helper's batches of the ranks, concatenated, are the
    unsharded batch."""
    import unpacking_reference
    from mosfhet_amd.shard import shard_bounds_whole
    N, per, total = 256, 67, 3 * 67 + 5
    P, whole = _packed(oracle, N, 4), _rows(oracle, N, total, per)
    for world in (1, 2, 3, 4, 7):
        parts = []
        for r in range(world):
            lo, hi = shard_bounds_whole(total, per, r, world)
            assert lo % per == 0 or lo == total, (world, r, lo)
            parts.append(unpacking_reference.unpack_batch(P[lo // per:], hi - lo, per))
        assert (np.concatenate(parts) == whole).all(), world


def test_the_composition_decrypts_on_the_cpu(oracle):
    """The condition of test_unpack_bootstrap_decrypts, proven without the device: the helper, then oracle.tlwe_keyswitch, then oracle.functional_bootstrap on the 70
    values of BOOT (N = 1024, n = 24, l = 2, Bg_bit = 8, switch t = 4, base_bit = 4, all noises 2^-40, 16 slots) decrypts every value to its table entry; the phases lie
    within half a slot (2^59) with a margin of at least 2 bits.  Measured: 2^54.2 (printed again by every run)."""
    import unpacking_reference
    B, D = BOOT, _boot_case(oracle)
    rows = unpacking_reference.unpack_batch(D["packed"], B["total"], B["per"])
    worst_in = max(oracle.torus_dist(np.uint64(oracle.tlwe_phase(rows[c], D["s_ring"])), D["msgs"][c] << np.uint64(59)) for c in range(B["total"]))
    worst = 0.0
    for c in range(B["total"]):
        sw = oracle.tlwe_keyswitch(rows[c], D["ksk"], B["n"], B["t"], B["base_bit"])
        out = oracle.functional_bootstrap(D["tv"], sw, D["bk_dft"], B["l"], B["Bg_bit"], B["slots"])
        worst = max(worst, float(oracle.torus_dist(np.uint64(oracle.tlwe_phase(out, D["s_ring"])), D["expect"][c])))
    print("the extracted inputs: 2^%.1f from their slots; the composition: 2^%.1f from the table entries (half a slot: 2^59)" % (_log2(worst_in), _log2(worst)))
    assert worst < HALF_SLOT_16 / 2 ** MARGIN_BITS, _log2(worst)


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


def _unpack_into_sentinel(eng, packed, total, per):
    """the call into a buffer one row longer than total, pre-filled with a sentinel: (the batch, the row past it)"""
    import torch
    import mosfhet_amd as ma
    N = packed.shape[2]
    buf = torch.full((total + 1, N + 1), int(SENTINEL.view(np.int64)), dtype=torch.int64, device=eng.device)
    eng.trlwe_unpack(ma.to_device(packed, eng.device), total, per, out=buf[:total])
    got = ma.to_numpy(buf)
    return got[:total], got[total]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(256, 256, 256), (256, 67, 3 * 67 + 5), (1024, 1024, 1025), (2048, 2048, 2049), (4096, 1, 3)])
def test_unpack_bit_exact(eng, oracle, shape):
    """== the helper on every word: one full input at the smallest ring; a ragged batch with per off every tile size; two inputs at N = 1024 and N = 2048, the second
    opened to one sample; per = 1 at N = 4096.  The row past `total` keeps its sentinel."""
    N, per, total = shape
    got, past = _unpack_into_sentinel(eng, _packed(oracle, N, -(-total // per)), total, per)
    want = _rows(oracle, N, total, per)
    assert got.shape == want.shape and (got == want).all(), "%s: %d words differ, rows %s" % (shape, (got != want).sum(), sorted(set(np.nonzero(got != want)[0]))[:8])
    assert (past == SENTINEL).all(), "%s: the row past total was written" % (shape,)


@pytest.mark.gpu
def test_unpack_extreme_masks_and_stale_rows(eng, oracle):
    """Inputs whose mask words are all 0, all 2^63 and all 2^64 - 1, and a random one (N = 256, per = N): == the helper; the negated wrap of 0 and of 2^63 is itself, so
    those batches hold one value throughout.  A per = 5 call on two inputs into the buffer a per = N call filled leaves no stale word: rows 0 .. 9 == the helper, the
    rest keep the earlier call's words."""
    import torch
    import mosfhet_amd as ma
    import unpacking_reference
    N = 256
    P = _packed(oracle, N, 4, seed=1).copy()
    P[0, 0], P[1, 0], P[2, 0] = 0, np.uint64(1) << np.uint64(63), np.uint64(0xFFFFFFFFFFFFFFFF)
    got, past = _unpack_into_sentinel(eng, P, 4 * N, N)
    assert (got == unpacking_reference.unpack_batch(P, 4 * N, N)).all() and (past == SENTINEL).all()
    assert (got[:N, :N] == 0).all() and (got[N:2 * N, :N] == np.uint64(1) << np.uint64(63)).all()
    buf = torch.empty((4 * N, N + 1), dtype=torch.int64, device=eng.device)
    d_in = ma.to_device(P, eng.device)
    eng.trlwe_unpack(d_in, 4 * N, N, out=buf)
    eng.trlwe_unpack(d_in[2:], 10, 5, out=buf[:10])
    again = ma.to_numpy(buf)
    assert (again[:10] == unpacking_reference.unpack_batch(P[2:], 10, 5)).all() and (again[10:] == got[10:]).all()


def _device_key(eng, K, base_bit):
    if "dksk" not in K or K["dksk"].engine is not eng:
        K["dksk"] = eng.load_keyswitch_key(K["rows"], base_bit)
    return K["dksk"]


# (form the plan must report, set_ks_words setting, t, base_bit, total, per)
FUSED = [("small", -1, 2, 2, 9, 4), ("words", -1, 2, 2, 70, 67), ("words", -1, 3, 4, 300, 256), ("words", -1, 2, 2, 8192 + 70, 67), ("tiles_256", 0, 2, 2, 200, 67),
         ("tiles_512", 0, 3, 4, 300, 256)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", FUSED, ids=["small", "words-70", "words-300", "words-two-pieces", "tiles256", "tiles512"])
def test_unpack_keyswitch_equals_unpack_then_keyswitch(eng, oracle, case):
    """N = 256, n_out = 16: trlwe_unpack_keyswitch == trlwe_unpack followed by tlwe_keyswitch on the device, and == oracle.tlwe_keyswitch of the helper's rows (all rows;
    for the batch of 8192 + 70 the first 80 and the rows 8100 .. 8261 around the piece boundary, which lies inside input 122), for every form, each asserted through
    the plan: the direct kernels (9 samples, unpacked into the pool), the word-lane form with a last wavefront of 6 samples, with 15 candidates and with a second
    piece that begins in the middle of an input, and -- with set_ks_words(0) -- the tiles of 256 and of 512."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    form, setting, t, bb, total, per = case
    N, n_out = 256, 16
    K = _switch_key(oracle, N, n_out, t, bb)
    dksk = _device_key(eng, K, bb)
    packed = _packed(oracle, N, -(-total // per), seed=2)
    rows = _rows(oracle, N, total, per, seed=2)
    d_in = ma.to_device(packed, eng.device)
    try:
        engine.set_ks_words(setting)
        plan = engine.trlwe_unpack_plan(N, n_out, t, bb, total, per)
        assert plan["form"] == form and plan["pieces"] == -(-total // 8192), plan
        fused = ma.to_numpy(eng.trlwe_unpack_keyswitch(dksk, d_in, total, per))
        unpacked = eng.trlwe_unpack(d_in, total, per)
        assert (ma.to_numpy(unpacked) == rows).all()
        two_calls = ma.to_numpy(eng.tlwe_keyswitch(dksk, unpacked))
    finally:
        engine.set_ks_words(-1)
    assert fused.shape == (total, n_out + 1)
    bad = np.nonzero((fused != two_calls).any(axis=1))[0]
    assert bad.size == 0, "%s: %d samples differ from unpack + tlwe_keyswitch, first %s" % (form, bad.size, bad[:8])
    check = range(total) if total < 1000 else list(range(80)) + list(range(8100, total))
    want = _switched(oracle, K, rows[list(check)], n_out, t, bb)
    assert (fused[list(check)] == want).all(), "%s: differs from the oracle's key switch of the helper's rows" % form


@pytest.mark.gpu
def test_unpack_keyswitch_with_a_seed_compressed_key(eng, oracle):
    """A key from mosfhet_hip_tlwe_ksk_generate with compressed = 1 (every word but b regenerated in the kernel: the tiles, whatever set_ks_words says) and its stored
    twin made with the same seed and the same noise secret: the fused call gives the same words with both, at 200 samples (tiles of 256) and at 9 (the direct kernels), and they equal unpack
    followed by tlwe_keyswitch."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, n_out, t, bb, per = 256, 16, 2, 2, 67
    K = _switch_key(oracle, N, n_out, t, bb)
    eng.set_keygen_secret(b"the twins share one noise stream")   # (a fresh one per call otherwise)
    stored = eng.generate_keyswitch_key(K["s_out"], K["s_in"], t, bb, 2.0 ** -40, 0xC0FFEE)
    eng.set_keygen_secret(b"the twins share one noise stream")
    packed_key = eng.generate_keyswitch_key(K["s_out"], K["s_in"], t, bb, 2.0 ** -40, 0xC0FFEE, compressed=True)
    try:
        for total, form in ((200, "tiles_256"), (9, "small")):
            assert engine.trlwe_unpack_plan(N, n_out, t, bb, total, per, compressed=True)["form"] == form
            d_in = ma.to_device(_packed(oracle, N, -(-total // per), seed=2), eng.device)
            a = ma.to_numpy(eng.trlwe_unpack_keyswitch(packed_key, d_in, total, per))
            b = ma.to_numpy(eng.trlwe_unpack_keyswitch(stored, d_in, total, per))
            c = ma.to_numpy(eng.tlwe_keyswitch(stored, eng.trlwe_unpack(d_in, total, per)))
            assert (a == b).all() and (b == c).all(), total
    finally:
        stored.free()
        packed_key.free()


@pytest.mark.gpu
def test_unpack_refusals_on_the_device(eng, oracle):
    """A key whose n_in is no ring this call opens (300), a key whose n_in is not the packed samples' N (the binding's check: the C call takes N from the key), a TRLWE
    table key (b_word != n_out), a key of another context and d_out overlapping d_in are refused with MOSFHET_HIP_EINVAL, each leaving d_out untouched; total = 0
    returns OK and writes nothing."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, n_out, t, bb, total, per = 256, 16, 2, 2, 70, 67
    K = _switch_key(oracle, N, n_out, t, bb)
    dksk = _device_key(eng, K, bb)
    in_w, out_w = 2 * 2 * N, total * (n_out + 1)
    buf = torch.full((in_w + out_w,), 5, dtype=torch.int64, device=eng.device)
    buf[:in_w] = ma.to_device(_packed(oracle, N, 2, seed=2), eng.device).view(-1)
    before = buf.clone()
    d_in, d_out = buf[:in_w].view(2, 2, N), buf[in_w:].view(total, n_out + 1)
    odd = eng.load_keyswitch_key(np.zeros((300, t, 3, n_out + 1), dtype=np.uint64), bb)
    with pytest.raises(engine.MosfhetHipError, match="n_in = 300"):
        eng.trlwe_unpack_keyswitch(odd, buf[:2 * 2 * 300].view(2, 2, 300), 4, 2, out=d_out[:4])
    odd.free()
    with pytest.raises(engine.MosfhetHipError, match="n_in = 256"):
        eng.trlwe_unpack_keyswitch(dksk, buf[:1024].view(1, 2, 512), 2, 2, out=d_out[:2])
    table = eng.load_packing1_key(np.zeros((N, 1, 3, 2, 1024), dtype=np.uint64), bb)
    with pytest.raises(engine.MosfhetHipError, match="packing"):
        eng.trlwe_unpack_keyswitch(table, d_in, total, per, out=d_out)
    table.free()
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.trlwe_unpack_keyswitch(dksk, d_in, total, per, out=buf[:out_w].view(total, n_out + 1))
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.trlwe_unpack_keyswitch(dksk, d_in, total, per, out=buf[in_w - 1:in_w - 1 + out_w].view(total, n_out + 1))
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.trlwe_unpack(d_in, 2, 1, out=buf[2 * N - 1:2 * N - 1 + 2 * (N + 1)].view(2, N + 1))
    other = ma.Engine(0)
    try:
        with pytest.raises(engine.MosfhetHipError, match="another context"):
            other.trlwe_unpack_keyswitch(dksk, d_in, total, per, out=d_out)
    finally:
        other.close()
    assert eng.trlwe_unpack_keyswitch(dksk, d_in, 0, per, out=d_out[:0]).shape[0] == 0
    assert eng.trlwe_unpack(d_in, 0, per, out=d_out.view(-1)[:0].view(0, N + 1)).shape[0] == 0
    torch.cuda.synchronize(eng.device)
    assert (buf == before).all(), "a refused call (or total = 0) wrote to its output"
    got = ma.to_numpy(eng.trlwe_unpack_keyswitch(dksk, d_in, total, per, out=d_out))          # adjacent buffers: fine
    assert (got == _switched(oracle, K, _rows(oracle, N, total, per, seed=2), n_out, t, bb)).all()


def _boot_keys(eng, oracle):
    D = _boot_case(oracle)
    if "bsk" not in D or D["bsk"].engine is not eng:
        D["bsk"] = eng.load_bootstrap_key(D["bk"], 1, BOOT["l"], BOOT["Bg_bit"])
        D["dksk"] = eng.load_keyswitch_key(D["ksk"], BOOT["base_bit"])
    return D


@pytest.mark.gpu
def test_unpack_keyswitch_bootstrap_equals_the_two_calls(eng, oracle):
    """unpack_keyswitch_functional_bootstrap == trlwe_unpack_keyswitch followed by functional_bootstrap[_wo_extract] (BOOT: N = 1024, n = 24, 70 values, 40 per input),
    with extract 1 and 0 and with one test vector and one per value; the one-table result with extraction also == oracle.functional_bootstrap of
    oracle.tlwe_keyswitch of the helper's rows."""
    import mosfhet_amd as ma
    import unpacking_reference
    B, D = BOOT, _boot_keys(eng, oracle)
    N, total, per = B["N"], B["total"], B["per"]
    d_in = ma.to_device(D["packed"], eng.device)
    tvs = np.stack([oracle.trlwe_torus_packing(np.roll(D["lut"], c), 1, N) for c in range(total)])
    switched = eng.trlwe_unpack_keyswitch(D["dksk"], d_in, total, per)
    for d_tv in (ma.to_device(D["tv"][None], eng.device), ma.to_device(tvs, eng.device)):
        for extract in (True, False):
            one = ma.to_numpy(eng.unpack_keyswitch_functional_bootstrap(D["dksk"], D["bsk"], d_tv, d_in, total, per, B["slots"], extract))
            boot = eng.functional_bootstrap if extract else eng.functional_bootstrap_wo_extract
            two = ma.to_numpy(boot(D["bsk"], d_tv, switched, B["slots"]))
            assert one.shape == two.shape and (one == two).all(), (d_tv.shape[0], extract)
            if extract and d_tv.shape[0] == 1:
                rows = unpacking_reference.unpack_batch(D["packed"], total, per)
                for c in range(0, total, 9):
                    sw = oracle.tlwe_keyswitch(rows[c], D["ksk"], B["n"], B["t"], B["base_bit"])
                    assert (one[c] == oracle.functional_bootstrap(D["tv"], sw, D["bk_dft"], B["l"], B["Bg_bit"], B["slots"])).all(), c


@pytest.mark.gpu
def test_unpack_bootstrap_decrypts(eng, oracle):
    """The inputs of test_the_composition_decrypts_on_the_cpu (made by oracle.trlwe_sample) through unpack_keyswitch_functional_bootstrap: every value decrypts to its
    table entry within half a slot (2^59).  Then the round trip the feature is for: the results packed again with tlwe_pack (split 1, 40 per output, a device-made key
    of 1024 entries, t = 6, base_bit = 4, noise 2^-40) and opened with trlwe_unpack decrypt to the same entries."""
    import mosfhet_amd as ma
    B, D = BOOT, _boot_keys(eng, oracle)
    N, total, per = B["N"], B["total"], B["per"]
    out = eng.unpack_keyswitch_functional_bootstrap(D["dksk"], D["bsk"], ma.to_device(D["tv"][None], eng.device), ma.to_device(D["packed"], eng.device), total, per, B["slots"])
    words = ma.to_numpy(out)
    d = max(float(oracle.torus_dist(np.uint64(oracle.tlwe_phase(words[c], D["s_ring"])), D["expect"][c])) for c in range(total))
    print("packed inputs through the bootstrap: 2^%.1f from the table entries (half a slot: 2^59)" % _log2(d))
    assert d < HALF_SLOT_16, _log2(d)
    src = np.zeros((N, N), dtype=np.uint64)
    src[:, 0] = D["s_ring"]
    pk = eng.generate_trlwe_ks_keys(D["s_ring"], src, 6, 4, B["sigma"], 0x9AC4)
    try:
        repacked = eng.tlwe_pack(pk, out, per, 1)
        assert tuple(repacked.shape) == (2, 2, N)
        ph = oracle.trlwe_phase(ma.to_numpy(repacked)[0], D["s_ring"])
        d_packed = float(oracle.torus_dist(ph[:per], D["expect"][:per]).max())
        opened = ma.to_numpy(eng.trlwe_unpack(repacked, total, per))
        d2 = max(float(oracle.torus_dist(np.uint64(oracle.tlwe_phase(opened[c], D["s_ring"])), D["expect"][c])) for c in range(total))
        print("packed again: 2^%.1f; opened again: 2^%.1f from the table entries" % (_log2(d_packed), _log2(d2)))
        assert d_packed < HALF_SLOT_16 and d2 < HALF_SLOT_16, (_log2(d_packed), _log2(d2))
    finally:
        pk.free()


@pytest.mark.gpu
def test_unpack_keyswitch_is_captured_in_a_graph(eng, oracle):
    """trlwe_unpack (from its first call) and trlwe_unpack_keyswitch at 70 samples (after one eager call of that size), each captured on one side stream and replayed
    twice on different inputs: each replay == the eager words -- no hidden allocation, synchronisation or state left between replays.  One stream, no parallel
    branches."""
    import torch
    import mosfhet_amd as ma
    N, n_out, t, bb, total, per = 256, 16, 2, 2, 70, 67
    K = _switch_key(oracle, N, n_out, t, bb)
    dksk = _device_key(eng, K, bb)
    xs = [ma.to_device(_packed(oracle, N, 2, seed=s), eng.device) for s in (2, 3)]
    want_rows = [_rows(oracle, N, total, per, seed=s) for s in (2, 3)]
    eager = [ma.to_numpy(eng.trlwe_unpack_keyswitch(dksk, x, total, per)) for x in xs]
    assert (eager[0] == _switched(oracle, K, want_rows[0], n_out, t, bb)).all()
    side = torch.cuda.Stream(device=eng.device)
    d_in, d_rows, d_out = xs[0].clone(), eng.empty(total, N + 1), eng.empty(total, n_out + 1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        eng.trlwe_unpack(d_in, total, per, out=d_rows)
        eng.trlwe_unpack_keyswitch(dksk, d_in, total, per, out=d_out)
    for r in (1, 0):
        d_in.copy_(xs[r])
        d_rows.zero_()
        d_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert (ma.to_numpy(d_rows) == want_rows[r]).all(), "replay on inputs %d: the unpacked rows differ from the helper" % r
        assert (ma.to_numpy(d_out) == eager[r]).all(), "replay on inputs %d differs from the plain call" % r
    del g


@pytest.mark.gpu
def test_unpack_host_face(native_lib, tmp_path):
    """tests/c/trlwe_unpack.c: mosfhet_trlwe_unpack and mosfhet_trlwe_unpack_keyswitch on host structs equal the C-ABI calls and the drop-in layer's trlwe_extract_tlwe /
    tlwe_keyswitch loops word for word, and every sample decrypts (N = 1024, n = 24, 70 samples, 40 per input)."""
    r = subprocess.run([_compile_c(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "trlwe_unpack ok" in r.stdout, r.stdout
