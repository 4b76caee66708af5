"""SET_1's throughput bootstrap kernels cut their gadget digits in the sign-free form (pbs_body.inc: kSignFree; bootstrap_kernels.h: cmux_digits<.., SF>,
digit_source_hi, Digits<2, 8, RAW>): the rotation's sign and source index from one 11-bit subtraction, the sign applied by two XORs around the carry-free add of the
negated home word, and the high dword kept raw -- digit lv is (byte 3 - lv) - 128.  Same digits as before, so every test compares with the oracle bit for bit, on
pbs_kernel<Fft1024, 2, 8> (one ciphertext per workgroup) and on pbs_group_kernel<Fft1024, 2, 8, 4> (four, with a ragged last workgroup), at batches of 1, 4, 5 and 9
and an LWE side of 24 words.

  * blind_rotate_ on accumulators CRAFTED for the first executed step: in both components (a: registers, staged through the exchange buffer; b: LDS) the words the
    digits are cut from have their byte fields at 0x00 / 0x7f / 0x80 / 0xff in both levels, with the 48 bits below at zero and at all ones, where the rotation negates
    and where it does not; rotations by one, around a wavefront's 64 lanes, around N/2 (the pair j, j + N/2), around N (the flip), by 2N - 1, and a skipped step.
    That the targeted fields really occur is asserted on the CPU from the oracle's own digits;
  * the same rotation split over two launches;
  * programmable_bootstrap with and without pre-processing and functional_bootstrap_wo_extract on a random key;
  * the host program tests/c/pbs_sign_forms.cpp (both integer forms in plain C++ under the sanitizers) and the build's kernel table (no GPU).

Mutants tried once, uncommitted: the lane mask taken from bit 9 instead of bit 10 (pieces 1 + 2) and the field offset 127 instead of 128 (piece 3) -- every GPU
test of this file fails with either."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x4D4F5346
N_LWE = 24
COUNTS = [1, 4, 5, 9]
EDGES = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)
# mod-switched mask words (log2 2N = 11) in the order ciphertext 0 meets them: ciphertext b starts at position b.  513 first, so that a batch of ONE has a first
# step with many coefficients of either sign; the second ciphertext starts with a skipped step.
ABARS = [513, 0, 1, 63, 64, 65, 511, 512, 1023, 1024, 1025, 2047]
FIELDS = (0x00, 0x7F, 0x80, 0xFF)
OFF = 2 ** 63 + 2 ** 55 + 2 ** 47


@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def keys(eng, oracle):
    """one key of 24 entries on SET_1's ring and gadget, and its two halves as keys of their own"""
    import mosfhet_amd as ma
    from mosfhet_amd import host
    P = dict(ma.PARAMS_SET1)
    host.seed(SEED + 2600)
    lk = host.LweKey(N_LWE, P["lwe_sigma"])
    rk = host.RlweKey(P["N"], 1, P["rlwe_sigma"])
    bk = host.gen_bootstrap_key(rk, lk, P["l"], P["Bg_bit"])
    K = dict(N=P["N"], l=P["l"], Bg_bit=P["Bg_bit"], lk=lk, rk=rk, bk=bk, bk_dft=oracle.bk_to_dft(bk, 1, P["l"]))
    K["bsk"] = eng.load_bootstrap_key(bk, 1, P["l"], P["Bg_bit"])
    K["halves"] = [eng.load_bootstrap_key(np.ascontiguousarray(bk[h * 12:(h + 1) * 12]), 1, P["l"], P["Bg_bit"]) for h in range(2)]
    return K


@pytest.fixture(autouse=True)
def kernel_switches(request):
    """every GPU test of this file runs the THROUGHPUT kernels and leaves the library's switches at their defaults"""
    if "gpu" not in request.keywords:
        yield
        return
    request.getfixturevalue("native_lib")
    from mosfhet_amd import engine
    engine.set_team_max_batch(0)
    engine.set_wide_team_max_batch(0)
    engine.set_split_max_batch(0)
    yield
    engine.set_pbs_group(-1)
    engine.set_team_max_batch(512)
    engine.set_wide_team_max_batch(512)
    engine.set_split_max_batch(-1)


def _both(call):
    """call() -> numpy with one ciphertext per workgroup and with four forced; the launcher's own account of what it launched is checked"""
    from mosfhet_amd import engine
    outs = []
    for mode, group in ((0, 1), (4, 4)):
        engine.set_pbs_group(mode)
        outs.append(call())
        assert engine.last_pbs_group() == group, (mode, engine.last_pbs_group())
    return outs


def _mask_words(count):
    """[count][25]: ciphertext b takes ABARS from position b on, exactly on the grid in the first 12 steps and at the two ends of the rounding interval in the last
    12, in reverse order -- so the teams of a workgroup skip DIFFERENT steps"""
    cts = np.zeros((count, N_LWE + 1), dtype=np.uint64)
    for b in range(count):
        for i in range(12):
            cts[b, i] = np.uint64((ABARS[(i + b) % 12] << 53) % 2 ** 64)
            abar = ABARS[(11 - i + b) % 12]
            cts[b, 12 + i] = np.uint64(((abar << 53) + (2 ** 52 - 1 if i % 2 == 0 else -2 ** 52)) % 2 ** 64)
    return cts


def _modswitch(words):
    return ((words.astype(object) + 2 ** 52) % 2 ** 64) >> 53


def _first_rotation(ct):
    return next(int(a) for a in _modswitch(ct[:-1]) if int(a) != 0)


def _negated(j, abar, N):
    """does coefficient j of acc X^abar come with a minus sign (src/polynomial.c:184-199)"""
    return (j < (abar & (N - 1))) != bool(abar & N)


def _crafted_accumulators(count, N):
    """[count][2][N]: edge words, over which the FIRST executed rotation r of ciphertext b gets its targets: for chosen j, acc[src(j)] is set so that
    (acc X^r - acc)[j] + off has the byte fields (f0, f1) and the low 48 bits asked for.  Chosen greedily, so that no target's two words are another target's."""
    rng = np.random.default_rng(2600 + count)
    cts = _mask_words(count)
    accs = EDGES[rng.integers(0, len(EDGES), size=(count, 2, N))]
    targets = [(f0 << 56) | (f1 << 48) | low for low in (0, 2 ** 48 - 1) for f0 in FIELDS for f1 in FIELDS]
    for b in range(count):
        r = _first_rotation(cts[b])
        a_lo = r & (N - 1)
        for c in range(2):
            acc = [int(x) for x in accs[b, c]]
            used = set()
            left = {False: list(targets), True: list(targets)}
            # (from both ends of the polynomial and from the lanes around the rotation's own sign change)
            order = sorted(range(N), key=lambda j: min(j, N - 1 - j, abs(j - a_lo) + (c + 1)))
            for j in order:
                src, neg = (j - a_lo) % N, _negated(j, r, N)
                if not left[neg] or j in used or src in used or src == j:
                    continue
                used.update((j, src))
                want = (left[neg].pop(0) - OFF + acc[j]) % 2 ** 64        # rot(acc)[j]
                acc[src] = (-want) % 2 ** 64 if neg else want
            accs[b, c] = np.array(acc, dtype=np.uint64)
    return accs


def _fields_hit(oracle, accs, cts, N):
    """{(component, level, field value, negated)} over the batch's first executed steps, from the oracle's own rotation and digits"""
    hit = set()
    for b in range(accs.shape[0]):
        r = _first_rotation(cts[b])
        neg = np.array([_negated(j, r, N) for j in range(N)])
        for c in range(2):
            digits = oracle.poly_decompose(oracle.poly_mul_by_xai_minus_1(np.ascontiguousarray(accs[b, c]), r), 8, 2).astype(np.int64)
            for lv in range(2):
                fields = digits[lv] + 128
                assert fields.min() >= 0 and fields.max() <= 255
                for f in FIELDS:
                    for s in (False, True):
                        if ((fields == f) & (neg == s)).any():
                            hit.add((c, lv, f, s))
    return hit


@pytest.mark.parametrize("count", COUNTS)
def test_crafted_inputs_reach_every_field_value(oracle, count):
    """(no GPU) every batch's crafted accumulators put 0x00 / 0x7f / 0x80 / 0xff into both levels' fields of both components under both signs in the first executed
    step -- by the oracle's digits; every ciphertext meets every rotation twice; ciphertext 1 starts with a skipped step"""
    N = 1024
    cts, accs = _mask_words(count), _crafted_accumulators(count, N)
    for b in range(count):
        assert sorted(int(x) for x in _modswitch(cts[b, :-1])) == sorted(ABARS + ABARS), b
    assert int(_modswitch(cts[:, 0])[0]) == 513 and (count < 2 or int(_modswitch(cts[1, :1])[0]) == 0)
    want = {(c, lv, f, s) for c in range(2) for lv in range(2) for f in FIELDS for s in (False, True)}
    assert _fields_hit(oracle, accs, cts, N) == want, sorted(want - _fields_hit(oracle, accs, cts, N))


def test_integer_forms_agree_on_the_host(tmp_path):
    """(no GPU) tests/c/pbs_sign_forms.cpp, a program of its own under the address and undefined-behaviour sanitizers: the digits in the form as it was, in the
    sign-free form and by the reference's formula agree on all rotations x positions, on words at every boundary and on 4 * 10^6 random triples"""
    import subprocess
    exe = str(tmp_path / "pbs_sign_forms")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "c", "pbs_sign_forms.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:]
    assert run.stdout.strip().endswith(" checks, 0 failures"), run.stdout[-3000:]


def test_kernel_table_keeps_both_kernels(native_lib):
    """(no GPU) the build's kernel table shows SET_1's two throughput kernels once each, within 256 registers, without scratch and with their LDS unchanged"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    rows = kernel_table.table()
    one = [r for r in rows if r["name"].startswith("pbs_kernel<Fft1024, 2, 8")]
    four = [r for r in rows if r["name"].startswith("pbs_group_kernel<Fft1024, 2, 8, 4>")]
    assert len(one) == 1 and len(four) == 1, ([r["name"] for r in one], [r["name"] for r in four])
    for r in one + four:
        assert r["vgpr"] <= 256 and r["scratch"] == 0, r
    assert one[0]["lds"] == 17408 and four[0]["lds"] == 4 * 17408, (one[0], four[0])
    assert len(rows) == 329, len(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_blind_rotate_on_crafted_accumulators(eng, oracle, keys, count):
    import mosfhet_amd as ma
    K = keys
    accs, cts = _crafted_accumulators(count, K["N"]), _mask_words(count)
    want_fields = {(c, lv, f, s) for c in range(2) for lv in range(2) for f in FIELDS for s in (False, True)}
    assert _fields_hit(oracle, accs, cts, K["N"]) == want_fields
    d_ct = ma.to_device(cts, eng.device)
    plain, grouped = _both(lambda: ma.to_numpy(eng.blind_rotate_(K["bsk"], ma.to_device(accs, eng.device), d_ct)))
    for b in range(count):
        want = oracle.blind_rotate(accs[b], cts[b, :-1].copy(), K["bk_dft"], K["l"], K["Bg_bit"])
        for name, got in (("one per workgroup", plain), ("four per workgroup", grouped)):
            bad = np.nonzero(got[b] != want)
            assert len(bad[0]) == 0, "%s: accumulator %d of %d differs from the oracle in %d words, first at component %d coefficient %d" % (
                name, b, count, len(bad[0]), bad[0][0], bad[1][0])


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_rotation_in_two_calls_equals_one(eng, oracle, keys, count):
    """steps 0 - 11 and 12 - 23 as two launches on the halves of the key"""
    import mosfhet_amd as ma
    K = keys
    accs, cts = _crafted_accumulators(count, K["N"]), _mask_words(count)
    first = np.ascontiguousarray(np.concatenate([cts[:, :12], cts[:, -1:]], axis=1))
    second = np.ascontiguousarray(cts[:, 12:])
    d_ct, d_first, d_second = (ma.to_device(x, eng.device) for x in (cts, first, second))

    def two_calls():
        d_acc = ma.to_device(accs, eng.device)
        eng.blind_rotate_(K["halves"][0], d_acc, d_first)
        eng.blind_rotate_(K["halves"][1], d_acc, d_second)
        return ma.to_numpy(d_acc)

    halves = _both(two_calls)
    whole = _both(lambda: ma.to_numpy(eng.blind_rotate_(K["bsk"], ma.to_device(accs, eng.device), d_ct)))
    for b in range(count):
        want = oracle.blind_rotate(accs[b], cts[b, :-1].copy(), K["bk_dft"], K["l"], K["Bg_bit"])
        for got in halves + whole:
            assert (got[b] == want).all(), "accumulator %d of %d differs from the oracle" % (b, count)


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_bootstraps_with_and_without_extraction(eng, oracle, keys, count):
    import mosfhet_amd as ma
    from mosfhet_amd import host
    K = keys
    rng = np.random.default_rng(2700 + count)
    tv = host.torus_packing(rng.integers(0, 2 ** 64, size=4, dtype=np.uint64), 1, K["N"])
    cts = host.tlwe_samples([host.double2torus((b % 4) / 8.0) for b in range(count)], K["lk"])
    cts[count // 2, [1, 7]] = 0      # skipped steps in one team
    d_tv, d_ct = ma.to_device(tv[None], eng.device), ma.to_device(cts, eng.device)
    for kappa, theta in ((0, 0), (2, 1)):
        for got in _both(lambda: ma.to_numpy(eng.programmable_bootstrap(K["bsk"], d_tv, d_ct, 3, kappa, theta))):
            assert got.shape == (count, K["N"] + 1)
            for b in range(count):
                want = oracle.programmable_bootstrap(tv, cts[b], K["bk_dft"], K["l"], K["Bg_bit"], 3, kappa, theta)
                assert (got[b] == want).all(), "programmable_bootstrap(kappa %d, theta %d): ciphertext %d of %d differs from the oracle" % (kappa, theta, b, count)
    for got in _both(lambda: ma.to_numpy(eng.functional_bootstrap_wo_extract(K["bsk"], d_tv, d_ct, 4))):
        assert got.shape == (count, 2, K["N"])
        for b in range(count):
            want = oracle.functional_bootstrap_wo_extract(tv, cts[b], K["bk_dft"], K["l"], K["Bg_bit"], 4)
            assert (got[b] == want).all(), "functional_bootstrap_wo_extract: ciphertext %d of %d differs from the oracle" % (b, count)
