"""SET_1's throughput bootstrap kernels keep their accumulators NEGATED (pbs_body.inc: kNegAcc): -acc mod 2^64 in registers (component a) and in LDS
(component b) from the first load to the last store, so that the digits and the rounded increments are carry-free 64-bit adds and component b's add is done by the
LDS unit.  What a caller sees must be the parent's bits: every test compares with the oracle bit for bit, on pbs_kernel<Fft1024, 2, 8> (one ciphertext per
workgroup) and on pbs_group_kernel<Fft1024, 2, 8, 4> (four, with a ragged last workgroup), at batches of 1, 4, 5 and 9 and an LWE side of 24 words.

  * blind_rotate_ on crafted accumulators: the negating load and store of the caller's accumulator, words at the edges of both 32-bit halves, rotations by one,
    around a wavefront's 64 lanes, around N/2, around N (the sign flip) and by 2N - 1, a skipped step;
  * the same rotation in two calls of 12 steps: the store / load round trip of the negated form in the middle;
  * programmable_bootstrap (sample extraction: a[j] is the resident word for j > 0, a[0] and b are negated back) with and without pre-processing, and
    functional_bootstrap_wo_extract (the negating store of both components)."""
import numpy as np
import pytest

SEED = 0x4D4F5346
N_LWE = 24
COUNTS = [1, 4, 5, 9]
# accumulator words: zero, the carry into and out of the low half, the sign bit, -1
EDGES = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)
# mod-switched mask words (log2 2N = 11): a skipped step, one, around the 64 lanes of a wavefront, around N/2, around N, 2N - 1
ABARS = [0, 1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047]


@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def keys(eng, oracle):
    """one key of 24 entries on SET_1's ring and gadget, and its two halves as keys of their own (the same rows, transformed row by row: the same key words)"""
    import mosfhet_amd as ma
    from mosfhet_amd import host
    P = dict(ma.PARAMS_SET1)
    host.seed(SEED + 2400)
    lk = host.LweKey(N_LWE, P["lwe_sigma"])
    rk = host.RlweKey(P["N"], 1, P["rlwe_sigma"])
    bk = host.gen_bootstrap_key(rk, lk, P["l"], P["Bg_bit"])
    K = dict(N=P["N"], l=P["l"], Bg_bit=P["Bg_bit"], lk=lk, rk=rk, bk=bk, bk_dft=oracle.bk_to_dft(bk, 1, P["l"]))
    K["bsk"] = eng.load_bootstrap_key(bk, 1, P["l"], P["Bg_bit"])
    K["halves"] = [eng.load_bootstrap_key(np.ascontiguousarray(bk[h * 12:(h + 1) * 12]), 1, P["l"], P["Bg_bit"]) for h in range(2)]
    return K


@pytest.fixture(autouse=True)
def kernel_switches(native_lib):
    """every test of this file runs the THROUGHPUT kernels and leaves the library's switches at their defaults"""
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
    """[count][25]: ciphertext b takes ABARS from position b on, exactly on the grid in the first 12 steps and at the two ends of the rounding interval (half a
    grid step below, one word short of half a step above) in the last 12, in reverse order -- so the teams of a workgroup skip DIFFERENT steps"""
    cts = np.zeros((count, N_LWE + 1), dtype=np.uint64)
    for b in range(count):
        for i in range(12):
            cts[b, i] = np.uint64((ABARS[(i + b) % 12] << 53) % 2 ** 64)
            abar = ABARS[(11 - i + b) % 12]
            cts[b, 12 + i] = np.uint64(((abar << 53) + (2 ** 52 - 1 if i % 2 == 0 else -2 ** 52)) % 2 ** 64)
    return cts


def _modswitch(words):
    return ((words.astype(object) + 2 ** 52) % 2 ** 64) >> 53


def _crafted_accumulators(count, N):
    """[count][2][N], every word one of EDGES: drawn at random, in a period of six along the polynomial, or one word throughout"""
    rng = np.random.default_rng(2400 + count)
    accs = np.empty((count, 2, N), dtype=np.uint64)
    for b in range(count):
        if b % 3 == 0:
            accs[b] = EDGES[rng.integers(0, len(EDGES), size=(2, N))]
        elif b % 3 == 1:
            accs[b] = EDGES[(np.arange(N)[None, :] + np.arange(2)[:, None] + b) % len(EDGES)]
        else:
            accs[b] = EDGES[(b // 3 + np.arange(2)[:, None] * 3) % len(EDGES)]
    return accs


def test_mask_words_reach_every_rotation():
    """(no GPU) the crafted mask words mod-switch to ABARS, each ciphertext meets each of them twice"""
    cts = _mask_words(9)
    for b in range(9):
        got = [int(x) for x in _modswitch(cts[b, :-1])]
        assert sorted(got) == sorted(ABARS + ABARS), (b, got)
    assert set(int(w) for w in _crafted_accumulators(9, 1024).reshape(-1)) == set(int(e) for e in EDGES)


def test_integer_forms_agree_on_the_host(tmp_path):
    """(no GPU) tests/c/pbs_acc_forms.cpp, a program of its own under the address and undefined-behaviour sanitizers: the step's tail and the digit words in the
    parent's form and in the negated-accumulator form give the same words on products and accumulators at the edges and on 10^7 random ones"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "pbs_acc_forms")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(root, "tests", "c", "pbs_acc_forms.cpp"), "-o", exe, "-lm"])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:]
    assert run.stdout.strip().endswith(" checks, 0 failures"), run.stdout[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_blind_rotate_on_crafted_accumulators(eng, oracle, keys, count):
    import mosfhet_amd as ma
    K = keys
    accs, cts = _crafted_accumulators(count, K["N"]), _mask_words(count)
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
    """steps 0 - 11 and 12 - 23 as two launches on the halves of the key: the accumulator goes through memory in its caller's form in between"""
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
    for got in halves + whole[1:]:
        assert (got == whole[0]).all()
    b = count - 1
    assert (whole[0][b] == oracle.blind_rotate(accs[b], cts[b, :-1].copy(), K["bk_dft"], K["l"], K["Bg_bit"])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_bootstraps_with_and_without_extraction(eng, oracle, keys, count):
    import mosfhet_amd as ma
    from mosfhet_amd import host
    K = keys
    rng = np.random.default_rng(2500 + count)
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
