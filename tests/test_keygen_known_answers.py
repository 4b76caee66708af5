"""Known answers for the key generators' randomness: the ChaCha20 noise streams and the public masks of the device generators (csrc/keygen_kernels.h) and the
host layer's generator (csrc/host/csprng.c), against a plain restatement of their specification (tests/keygen_reference.py: RFC 8439 block function, the
mask formula, Box-Muller evaluated exactly in mpmath).

The generators are deterministic once their secret is installed, so every exported word is compared: masks word for word, noise terms -- recovered exactly as
e = b - a * s - message (mod 2^64) -- within
    |e - reference| <= 1 + sigma 2^64 2^-40
(1: the truncation of double2torus; 2^-40 sigma: the generators evaluate cos, log and sqrt in double with their own library -- the host's double evaluation
lies within 2^-47.6 sigma of the exact value, worst of 20,000 draws, which leaves 7 bits for the device library).  A wrong stream misses by about sigma 2^64
per coefficient.  Keys that can be exported in the DFT domain only come back through the oracle's inverse transform; their masks are known exactly, so the
round trip's error is MEASURED per row on the mask and bounds the body's (see _dft_body_tolerance).
"""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import keygen_reference as R

SECRET = bytes(range(32))
KEY = R.key_words(SECRET)
M64 = R.M64

# largest |e - reference| / (sigma 2^64) seen by the device tests of this process: [exactly evaluated reference words, words evaluated in double]
OBSERVED = {"exact": 0.0, "double": 0.0}


def _u64(x):
    return np.asarray([int(v) & M64 for v in np.atleast_1d(x)], dtype=np.uint64)


# ------------------------------------------------------------------ the reference itself
def test_reference_block_reproduces_rfc8439_vectors():
    """RFC 8439 section 2.3.2 (key 00 .. 1f, state words 12 - 15 = 00000001 09000000 4a000000 00000000) and appendix A.1 #1 (all zero)."""
    out = R.chacha20_block(KEY, 1 | (0x09000000 << 32), 0x4a000000)
    assert out == [0xe4e7f110, 0x15593bd1, 0x1fdd0f50, 0xc47120a3, 0xc7f4d1c7, 0x0368c033, 0x9aaa2204, 0x4e6cd4c3,
                   0x466482d2, 0x09aa9f07, 0x05d7c214, 0xa2028bd9, 0xd19c12b5, 0xb94e16de, 0xe883d0cb, 0x4e3c50a2]
    zero = struct.pack("<16I", *R.chacha20_block([0] * 8, 0, 0))
    assert zero[:16].hex() == "76b8e0ada0f13d90405d6ae55386bd28" and zero[-8:].hex() == "c387b669b2ee6586"
    rng = np.random.default_rng(5)
    for _ in range(20):
        seed, row, idx, stream = (int(v) for v in rng.integers(0, 2 ** 63, size=4))
        assert R.mask_word(seed, row % 2 ** 21, idx % 4096, stream % 3) == int(R.mask_row(seed, row % 2 ** 21, idx % 4096 + 1, stream % 3)[-1])
    assert R.call_nonce(1, R.KIND_TABLE) == 0x101 and R.call_nonce(3, R.KIND_TLWE_KSK) == 0x305
    assert R.torus_of_exact(R.mpmath.mpf("-1.5") / 2 ** 64) == -1 and R.torus_of_exact(R.mpmath.mpf("2.9") / 2 ** 64) == 2


# ------------------------------------------------------------------ host generator (no GPU)
class _HostProgram:
    """tests/c/csprng_known_answers.c: the host layer's sources in a process of their own (mc_chacha20_block is not exported by the library, and a fresh process
    has a fresh generator state: the engine is not running, no thread has drawn yet)."""

    def __init__(self, exe):
        self.exe = exe

    def run(self, *commands):
        import subprocess
        r = subprocess.run([self.exe], input="\n".join(commands) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        lines = r.stdout.splitlines()
        assert r.returncode == 0 and len(lines) == len(commands) and "OVERRUN" not in r.stdout, r.stdout[-2000:]
        return lines


@pytest.fixture(scope="module")
def host_program(native_lib, tmp_path_factory):
    """built the way tests/test_host_and_abi.py builds its host-helper program (without the sanitizers)"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "mosfhet_amd", "csrc", "host")
    srcs = [os.path.join(host, f) for f in ("mosfhet_compat.c", "mosfhet_compat_dft.c", "mosfhet_compat_multi.c", "mosfhet_compat_legacy.c", "mosfhet_compat_extra.c", "csprng.c")]
    exe = str(tmp_path_factory.mktemp("csprng") / "csprng_known_answers")
    subprocess.check_call(["gcc", "-O1", "-g", "-ffp-contract=off", "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "mosfhet_amd", "csrc"),
                           os.path.join(root, "tests", "c", "csprng_known_answers.c")] + srcs +
                          ["-o", exe, "-L" + os.path.join(root, "mosfhet_amd"), "-lmosfhet_hip", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-lpthread",
                           "-Wl,-rpath," + os.path.join(root, "mosfhet_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return _HostProgram(exe)


def _block_command(key, counter, nonce):
    return "block " + " ".join("%x" % w for w in key) + " %x %x" % (counter, nonce)


def _words(line):
    return [int(w, 16) for w in line.split()]


def test_host_block_function_known_answers(host_program):
    """mc_chacha20_block: the two RFC 8439 vectors as literal words, then 100 random (key, counter, nonce) triples -- counters and nonces above 2^32 included --
    against the Python block."""
    rng = np.random.default_rng(8439)
    triples = [(KEY, 1 | (0x09000000 << 32), 0x4a000000), ([0] * 8, 0, 0), (KEY, 7, 9), (KEY, 9, 7), (KEY, 1 << 32, 0), (KEY, 0, 1)]
    for i in range(100):
        key = [int(w) for w in rng.integers(0, 2 ** 32, size=8)]
        bits_c, bits_n = (64, 64) if i % 3 == 0 else ((20, 64) if i % 3 == 1 else (64, 8))
        triples.append((key, (int(rng.integers(0, 2 ** 63)) * 2 + 1) >> (64 - bits_c), (int(rng.integers(0, 2 ** 63)) * 2 + 1) >> (64 - bits_n)))
    assert sum(c >= 2 ** 32 for _, c, _ in triples) > 30 and sum(n >= 2 ** 32 for _, _, n in triples) > 30
    out = [_words(line) for line in host_program.run(*(_block_command(*tr) for tr in triples))]
    assert out[0] == [0xe4e7f110, 0x15593bd1, 0x1fdd0f50, 0xc47120a3, 0xc7f4d1c7, 0x0368c033, 0x9aaa2204, 0x4e6cd4c3,
                      0x466482d2, 0x09aa9f07, 0x05d7c214, 0xa2028bd9, 0xd19c12b5, 0xb94e16de, 0xe883d0cb, 0x4e3c50a2]
    zero = struct.pack("<16I", *out[1])
    assert zero[:16].hex() == "76b8e0ada0f13d90405d6ae55386bd28" and zero[-8:].hex() == "c387b669b2ee6586"
    for tr, got in zip(triples, out):
        assert got == R.chacha20_block(*tr), tr
    assert out[2] != out[3] and out[4] != out[5]             # counter and nonce are different words of the state


def test_host_stream_after_seed(host_program):
    """generate_random_bytes after mosfhet_seed(s): the restated stream across block boundaries, a ragged tail consuming a whole draw, the same stream after
    seeding again; threads started afterwards draw on nonces 1 and 2 in the order of their first draw, the seeding thread goes on at nonce 0."""
    seed = 0x0123456789ABCDEF
    out = host_program.run("seed %x" % seed, "bytes 200", "bytes 13 8 3", "bytes 64",
                           "seed %x" % seed, "bytes 64",
                           "seed %x" % (seed + 1), "bytes 64",
                           "seed %x" % seed, "thread 100 28", "thread 100 28", "bytes 64")
    ref = R.HostStream(seed)
    assert out[1] == ref.bytes(200).hex()                     # three blocks of 64 bytes and more
    assert out[2] == (ref.bytes(13) + ref.bytes(8) + ref.bytes(3)).hex()   # 13 = 8 + 5: the tail takes a whole 64-bit draw, the next request starts at the draw after it
    assert out[3] == ref.bytes(64).hex()
    first = R.HostStream(seed).bytes(64)
    assert out[5] == first.hex() == out[1][:128]
    assert out[7] == R.HostStream(seed + 1).bytes(64).hex() != out[5]
    ref = R.HostStream(seed)
    assert out[9] == (ref.bytes(100, nonce=1) + ref.bytes(28, nonce=1)).hex()
    assert out[10] == (ref.bytes(100, nonce=2) + ref.bytes(28, nonce=2)).hex()
    assert out[11] == ref.bytes(64).hex() == first.hex()
    assert len({out[9][:128], out[10][:128], out[11]}) == 3


def test_host_gaussians_and_seed_words(host_program):
    """generate_normal_random / generate_torus_normal_random_array: Box-Muller of the next two draws each, against the exact value; generate_rnd_seed: four words."""
    sigmas_n, sigmas_t = (1.0, 2.0 ** -15, 2.989040792967434e-8), (2.0 ** -15, 2.0 ** -25, 2.0 ** -44)
    out = host_program.run("seed feedface", *(["normal %s 200" % s.hex() for s in sigmas_n] + ["torus %s 300" % s.hex() for s in sigmas_t] + ["rndseed", "bytes 8"]))
    ref = R.HostStream(0xFEEDFACE)
    worst = 0.0
    for sigma, line in zip(sigmas_n, out[1:4]):
        got = [float.fromhex(w) for w in line.split()]
        assert len(got) == 200
        for g in got:
            err = abs(float(R.mpmath.mpf(g) - ref.normal_exact(sigma))) / sigma
            worst = max(worst, err)
            assert err <= 2.0 ** -40, (sigma, g)
    for sigma, line in zip(sigmas_t, out[4:7]):
        got = _words(line)
        assert len(got) == 300
        for i, g in enumerate(got):
            want = R.torus_of_exact(ref.normal_exact(sigma))
            diff = abs((g - (1 << 64) if g >> 63 else g) - want)
            worst = max(worst, diff / (sigma * 2.0 ** 64) if diff > 1 else 0.0)
            assert diff <= R.noise_tolerance(sigma), (sigma, i, g, want)
    print("host Box-Muller: largest |got - exact| / sigma = 2^%.1f" % np.log2(worst + 2.0 ** -80))
    assert struct.pack("<4Q", *_words(out[7])) == ref.bytes(32)
    assert out[8] == ref.bytes(8).hex()                       # ... and exactly four words were drawn


# ------------------------------------------------------------------ device generators
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


def _binary_key(rng, n):
    s = rng.integers(0, 2, size=n).astype(np.uint64)
    s[0] = 1
    return s


def _small_key(rng, n):
    """small integers with negative coefficients (and zeros): the generators' general-coefficient branch"""
    s = rng.integers(-3, 4, size=n).astype(np.int64)
    s[0], s[1], s[n - 1] = -2, 3, -1
    return s.astype(np.uint64)


def _check_noise(e, key, nonce, row, sigma, extra_tol=0.0, what=None, exact_words=64):
    """e (uint64 words of one row) against the noise terms of (key, nonce, row): every word, nothing skipped."""
    want = R.noise_row(key, nonce, row, e.size, sigma, exact_words)
    diff = np.abs((e.astype(np.int64) - want).astype(np.float64))   # |e|, |want| < 2^62: the difference does not wrap for a matching stream
    tol = R.noise_tolerance(sigma) + extra_tol
    if extra_tol == 0.0 and diff.max() <= tol:
        scale = sigma * 2.0 ** 64
        OBSERVED["exact"] = max(OBSERVED["exact"], diff[:exact_words].max() / scale)
        OBSERVED["double"] = max(OBSERVED["double"], diff[exact_words:].max() / scale if e.size > exact_words else 0.0)
    bad = np.flatnonzero(diff > tol)
    assert bad.size == 0, "%s row %d: %d of %d noise terms off, first at x = %d: got %d, want %d (tolerance %.1f)" % (
        what, row, bad.size, e.size, bad[0], int(e.astype(np.int64)[bad[0]]), int(want[bad[0]]), tol)


def _noise_mismatch(e, key, nonce, row, sigma):
    """median |e - noise of another stream| / (sigma 2^64): about 1 for an independent stream, below 2^-40 for the same one"""
    want = R.noise_row(key, nonce, row, e.size, sigma, exact_words=0)
    return float(np.median(np.abs((e.astype(np.int64) - want).astype(np.float64)))) / (sigma * 2.0 ** 64)


def _report(name):
    print("%s: largest |e - reference| / (sigma 2^64) so far: 2^%.1f on exactly evaluated words, 2^%.1f on words evaluated in double" % (
        name, np.log2(OBSERVED["exact"] + 2.0 ** -80), np.log2(OBSERVED["double"] + 2.0 ** -80)))


def _table_message(kind, r, s_out, s_in, n, t, bb, slots):
    """message polynomial of row r of a table key (trlwe_new_packing1_KS_key, trlwe_new_priv_SK_KS_key_N2, trlwe_new_packing_KS_key)"""
    N, cands = s_out.size, (1 << bb) - 1
    v, j, i = r % cands + 1, (r // cands) % t, r // (cands * t)
    h = 1 << (64 - (j + 1) * bb)
    msg = np.zeros(N, dtype=np.uint64)
    if kind == 0:
        msg[0] = (int(s_in[i]) * v * h) & M64
    elif kind == 1:
        s_i = int(s_in[i]) if i < n else M64                    # entry n: the key's own -1
        with np.errstate(over="ignore"):
            msg = (np.uint64(0) - s_out) * np.uint64((s_i * v * h) & M64)
    else:
        e, span = i % slots, N // slots
        msg[e * span:(e + 1) * span] = (int(s_in[i // slots]) * v * h) & M64
    return msg


def _check_table_rows(oracle, rows, first_row, kind, s_out, s_in, t, bb, slots, seed, nonce, sigma, what):
    N, n = s_out.size, s_in.size
    for q, row in enumerate(rows.reshape(-1, 2, N)):
        r = first_row + q
        assert (row[0] == R.mask_row(seed, r, N)).all(), (what, r)
        e = row[1] - oracle.poly_naive_mul(row[0].copy(), s_out) - _table_message(kind, r, s_out, s_in, n, t, bb, slots)
        _check_noise(e, KEY, nonce, r, sigma, what=what)


@pytest.mark.gpu
@pytest.mark.parametrize("key_kind", ["binary", "small"])
@pytest.mark.parametrize("kind,compressed", [(0, False), (0, True), (1, False), (1, True), (2, False)])
def test_table_key_known_answers(eng, oracle, kind, compressed, key_kind):
    """trlwe_table_keygen_kernel, N = 256, n = 3, t = 2, bb = 2: the packing key (kind 0), the private key (1) and the LUT-packing key (2, four slots; it has no
    compressed form), full and seed-compressed, under a binary key and under small integers with negative coefficients.  Two calls under one secret: call 2
    takes another seed and the next nonce."""
    N, n, t, bb, sigma, slots = 256, 3, 2, 2, 2.0 ** -15, 4 if kind == 2 else 1
    rng = np.random.default_rng(100 + kind)
    s_out = _binary_key(rng, N) if key_kind == "binary" else _small_key(rng, N)
    s_in = _u64([1, 0, 1]) if key_kind == "binary" else _u64([1, -2, 3])
    n_rows = (n * slots if kind == 2 else n + kind) * t * 3
    eng.set_keygen_secret(SECRET)
    for call, seed in ((1, 0x5EED0001), (2, 0xC0FFEE0000000002)):
        if kind == 2:
            key = eng.generate_lut_packing_key(s_out, s_in, t, bb, slots, sigma, seed)
        else:
            key = eng.generate_table_key(kind, s_out, s_in, t, bb, sigma, seed, compressed=compressed)
        rows = eng.export_key_rows(key, 0, n_rows)
        key.free()
        _check_table_rows(oracle, rows, 0, kind, s_out, s_in, t, bb, slots, seed, R.call_nonce(call, R.KIND_TABLE), sigma, "table key kind %d call %d" % (kind, call))
    _report("table key")


def _check_lwe_rows(rows, first_row, s_out, s_in, t, bb, seed, nonce, sigma, what):
    n_out, cands = s_out.size, (1 << bb) - 1
    for q, row in enumerate(rows.reshape(-1, n_out + 1)):
        r = first_row + q
        v, j, i = r % cands + 1, (r // cands) % t, r // (cands * t)
        assert (row[:n_out] == R.mask_row(seed, r, n_out)).all(), (what, r)
        with np.errstate(over="ignore"):
            dot = (row[:n_out] * s_out).sum(dtype=np.uint64)
            e = row[n_out:] - dot - np.uint64((int(s_in[i]) * v << (64 - (j + 1) * bb)) & M64)
        _check_noise(e, KEY, nonce, r, sigma, what=what)         # one noise term per row, at coefficient 0


@pytest.mark.gpu
@pytest.mark.parametrize("compressed", [False, True])
@pytest.mark.parametrize("n_out", [1, 64, 70])
def test_lwe_table_known_answers(eng, n_out, compressed):
    """tlwe_ksk_keygen_kernel, n_in = 3, t = 2, bb = 2: one lane, exactly one pass of the 64-lane loop, a ragged second pass; small-integer keys."""
    t, bb, sigma = 2, 2, 2.0 ** -15
    rng = np.random.default_rng(200 + n_out)
    s_out, s_in = _small_key(rng, max(n_out, 3))[:n_out], _u64([1, -1, 2])
    eng.set_keygen_secret(SECRET)
    for call, seed in ((1, 77), (2, 0xABCDEF0123456789)):
        key = eng.generate_keyswitch_key(s_out, s_in, t, bb, sigma, seed, compressed=compressed)
        rows = eng.export_key_rows(key, 0, 3 * t * 3)
        key.free()
        _check_lwe_rows(rows, 0, s_out, s_in, t, bb, seed, R.call_nonce(call, R.KIND_TLWE_KSK), sigma, "LWE table n_out %d call %d" % (n_out, call))
    _report("LWE table")


@pytest.mark.gpu
def test_lwe_table_rows_across_the_launch_chunks(eng):
    """The LWE table's launcher works in chunks of 2^20 rows (first_row): n_in = 1029, t = 4, bb = 8, n_out = 1 is 1,049,580 rows of two words; the rows either
    side of 2^20 and the last one."""
    n_in, t, bb, sigma, seed = 1029, 4, 8, 2.0 ** -15, 0x1234
    rng = np.random.default_rng(300)
    s_out, s_in = _u64([-3]), _binary_key(rng, n_in)
    n_rows = n_in * t * 255
    assert n_rows == 1049580
    eng.set_keygen_secret(SECRET)
    key = eng.generate_keyswitch_key(s_out, s_in, t, bb, sigma, seed)
    for first, count in ((2 ** 20 - 2, 4), (n_rows - 1, 1), (0, 1)):
        _check_lwe_rows(eng.export_key_rows(key, first, count), first, s_out, s_in, t, bb, seed, R.call_nonce(1, R.KIND_TLWE_KSK), sigma, "LWE table chunks")
    key.free()
    _report("LWE table chunks")


@pytest.mark.gpu
def test_table_key_rows_across_the_launch_chunks(eng, oracle):
    """The table keys' launcher works in chunks of 2^20 rows too: a seed-compressed packing key at N = 256 with n = 588, t = 7, bb = 8 is 1,049,580 rows (2.0 GiB);
    the rows either side of 2^20 and the last one.  (t bb must stay below 64: 8 digits of 8 bits are refused by the generator.)"""
    N, n, t, bb, sigma, seed = 256, 588, 7, 8, 2.0 ** -15, 0x4321
    rng = np.random.default_rng(301)
    s_out, s_in = _binary_key(rng, N), _binary_key(rng, n)
    n_rows = n * t * 255
    assert n_rows == 1049580
    eng.set_keygen_secret(SECRET)
    key = eng.generate_table_key(0, s_out, s_in, t, bb, sigma, seed, compressed=True)
    for first, count in ((2 ** 20 - 2, 4), (n_rows - 1, 1), (0, 1)):
        _check_table_rows(oracle, eng.export_key_rows(key, first, count), first, 0, s_out, s_in, t, bb, 1, seed, R.call_nonce(1, R.KIND_TABLE), sigma, "table key chunks")
    key.free()
    _report("table key chunks")


@pytest.mark.gpu
def test_unfolded_bootstrap_key_known_answers(eng, oracle):
    """trgsw_bk_keygen_kernel through generate_bootstrap_key_unfolded(unfolding = 2), whose image is torus-domain samples: N = 1024, l = 2, Bg = 2^8, n = 4.
    Entry g 4 + j is TRGSW(1 if the bits of group g spell j else 0): every row of every sample, the gadget term on coefficient 0 of the right component."""
    N, l, Bg, n, sigma, seed, u = 1024, 2, 8, 4, 2.0 ** -15, 0xB00F, 2
    rng = np.random.default_rng(400)
    s, s_lwe = _binary_key(rng, N), _u64([1, 0, 1, 1])
    eng.set_keygen_secret(SECRET)
    key = eng.generate_bootstrap_key_unfolded(s, s_lwe, l, Bg, sigma, seed, u)
    image = eng.export_bootstrap_key(key).view(np.uint64).reshape(n // u << u, 2 * l, 2, N)
    key.free()
    nonce = R.call_nonce(1, R.KIND_BSK_UNFOLDED)
    for entry in range(image.shape[0]):
        g, spelled = divmod(entry, 1 << u)
        msg = int(all(int(s_lwe[g * u + b]) == ((spelled >> b) & 1) for b in range(u)))
        for q in range(2 * l):
            r, (c, j) = entry * 2 * l + q, divmod(q, l)
            gadget = np.zeros((2, N), dtype=np.uint64)
            gadget[c, 0] = msg << (64 - (j + 1) * Bg)
            a = R.mask_row(seed, r, N)
            assert (image[entry, q, 0] == a + gadget[0]).all(), (entry, q)
            e = image[entry, q, 1] - oracle.poly_naive_mul(a, s) - gadget[1]      # the body is formed from the plain mask
            _check_noise(e, KEY, nonce, r, sigma, what="unfolded key")
    _report("unfolded bootstrap key")


def _dft_body_tolerance(mask_err, s, sigma):
    """A row that went through the forward transform on the device and the oracle's inverse on the host: `mask_err`, the largest deviation of the row's recovered
    mask words from their known exact values, is the round trip's error on that row.  The body's bound is that error once for every nonzero key coefficient (the
    a * s sum) and once for the body itself, on top of the noise tolerance.  It has to stay below 2^-12 sigma 2^64 for the comparison to tell streams apart."""
    extra = mask_err * (int(np.count_nonzero(s)) + 1)
    assert extra + R.noise_tolerance(sigma) < 2.0 ** -12 * sigma * 2.0 ** 64, (mask_err, sigma)
    return extra


def _check_dft_row(oracle, row_dft, masks, gadget, s_polys, nonce, r, sigma, what):
    """row_dft: [k+1][N] doubles in the oracle's slot order; masks: the k exact plain masks; gadget: [k+1][N] words added after the body was formed.
    Returns the round trip's measured error on this row."""
    k = len(masks)
    mask_err = 0.0
    for m in range(k):
        got = oracle.dft_to_torus(np.ascontiguousarray(row_dft[m]))
        mask_err = max(mask_err, float(oracle.torus_dist(got, masks[m] + gadget[m]).max()))
    body = oracle.dft_to_torus(np.ascontiguousarray(row_dft[k]))
    e = body - gadget[k]
    for m in range(k):
        e = e - oracle.poly_naive_mul(masks[m], s_polys[m])
    _check_noise(e, KEY, nonce, r, sigma, extra_tol=_dft_body_tolerance(mask_err, np.concatenate(s_polys), sigma), what=what)
    return mask_err


@pytest.mark.gpu
@pytest.mark.parametrize("ga", [False, True])
def test_bootstrap_key_known_answers(eng, oracle, ga):
    """trgsw_bk_keygen_kernel through generate_bootstrap_key, plain and Galois (TRGSW(X^{s_i})): N = 1024, l = 2, Bg = 2^8, n = 3, a bounded LWE key whose Galois
    exponents are negative (-3 = 2N - 3: coefficient N - 3, sign flipped) and beyond N (N + 5: coefficient 5, sign flipped).  Only the DFT image leaves the device:
    rows come back through the oracle's inverse transform, sigma = 2^-25.  Measured round-trip error (largest deviation of a recovered mask word, MI355X):
    2^12.88 plain, 2^13.05 Galois (2^12.89 at k = 2, N = 256 and 2^12.90 for the TRLWE key-switch keys below), i.e. a body bound of about 2^22 at this key's
    weight; _dft_body_tolerance asserts that it stays below 2^27 = 2^-12 sigma 2^64.  The exactly exported keys measure the device's Box-Muller at
    2^-48.0 sigma from the exact value (largest of all words the tests of this file compare at sigma = 2^-15)."""
    N, l, Bg, sigma, seed = 1024, 2, 8, 2.0 ** -25, 0xD1F7
    rng = np.random.default_rng(500)
    s, s_lwe = _binary_key(rng, N), _u64([2, -3, N + 5])
    eng.set_keygen_secret(SECRET)
    key = eng.generate_bootstrap_key(s, s_lwe, l, Bg, sigma, seed, ga=ga)
    dft = key.export_dft()
    key.free()
    worst = 0.0
    for i in range(3):
        for q in range(2 * l):
            r, (c, j) = i * 2 * l + q, divmod(q, l)
            h = 1 << (64 - (j + 1) * Bg)
            gadget = np.zeros((2, N), dtype=np.uint64)
            if ga:
                ex = int(np.int64(s_lwe[i])) % (2 * N)
                gadget[c, ex % N] = (-h if ex >= N else h) & M64
            else:
                gadget[c, 0] = (int(s_lwe[i]) * h) & M64
            worst = max(worst, _check_dft_row(oracle, dft[i, q], [R.mask_row(seed, r, N)], gadget, [s], R.call_nonce(1, R.KIND_BSK), r, sigma, "bootstrap key ga=%d" % ga))
    print("bootstrap key (ga = %d): round trip through the DFT image, largest deviation of a recovered mask word: 2^%.2f" % (ga, np.log2(worst + 1)))


@pytest.mark.gpu
def test_bootstrap_key_k2_known_answers(eng, oracle):
    """trgsw_bk_keygen_k_kernel: k = 2, N = 256, l = 2, Bg = 2^8, n = 3.  Mask m of a row comes from generator stream m, the noise is added once, on the body, and
    the gadget term sits on coefficient 0 of component c.  Rows come back through the DFT image as in test_bootstrap_key_known_answers."""
    N, k, l, Bg, sigma, seed = 256, 2, 2, 8, 2.0 ** -25, 0x2B2B
    rng = np.random.default_rng(600)
    s = np.stack([_binary_key(rng, N), _small_key(rng, N)])
    s_lwe = _u64([1, 0, -1])
    eng.set_keygen_secret(SECRET)
    key = eng.generate_bootstrap_key(s, s_lwe, l, Bg, sigma, seed)
    dft = key.export_dft()
    key.free()
    worst = 0.0
    for i in range(3):
        for q in range((k + 1) * l):
            r, (c, j) = i * (k + 1) * l + q, divmod(q, l)
            gadget = np.zeros((k + 1, N), dtype=np.uint64)
            gadget[c, 0] = (int(s_lwe[i]) << (64 - (j + 1) * Bg)) & M64
            masks = [R.mask_row(seed, r, N, stream=m) for m in range(k)]
            worst = max(worst, _check_dft_row(oracle, dft[i, q], masks, gadget, [s[0], s[1]], R.call_nonce(1, R.KIND_BSK), r, sigma, "k = 2 bootstrap key"))
    print("k = 2 bootstrap key: round trip through the DFT image, largest deviation of a recovered mask word: 2^%.2f" % np.log2(worst + 1))


@pytest.mark.gpu
def test_trlwe_key_switch_keys_known_answers(eng, oracle):
    """trlwe_poly_keygen_kernel: a key set of two entries (switching from a plain polynomial and from the key under X -> X^5), N = 1024, t = 3, bb = 8.  The image
    is in the DFT domain (the engine's slot order): rows come back as in test_bootstrap_key_known_answers."""
    from mosfhet_amd import engine
    N, t, bb, sigma, seed = 1024, 3, 8, 2.0 ** -25, 0x7715
    rng = np.random.default_rng(700)
    s = _binary_key(rng, N)
    msgs = np.stack([rng.integers(0, 2 ** 64, size=N, dtype=np.uint64), oracle.poly_permute(s, 5)])
    eng.set_keygen_secret(SECRET)
    keys = eng.generate_trlwe_ks_keys(s, msgs, t, bb, sigma, seed)
    image = eng.export_trlwe_ks_keys(keys)
    keys.free()
    assert image.shape == (2, t, 2, N)
    dft = engine.slot_order_to_oracle(image, N)
    worst = 0.0
    for entry in range(2):
        for j in range(t):
            r = entry * t + j
            gadget = np.zeros((2, N), dtype=np.uint64)
            gadget[1] = msgs[entry] << np.uint64(64 - (j + 1) * bb)
            worst = max(worst, _check_dft_row(oracle, dft[entry, j], [R.mask_row(seed, r, N)], gadget, [s], R.call_nonce(1, R.KIND_TRLWE_KSK), r, sigma, "TRLWE key-switch keys"))
    print("TRLWE key-switch keys: round trip through the DFT image, largest deviation of a recovered mask word: 2^%.2f" % np.log2(worst + 1))


@pytest.mark.gpu
def test_every_generator_kind_has_its_own_nonce(eng, oracle):
    """One call of each of the five generator kinds under one secret, in a fixed order: the noise of call i matches call_nonce(i, kind) -- and not the nonce of the
    call before or after, nor another kind's tag at the same index."""
    from mosfhet_amd import engine
    N, sigma, seed = 1024, 2.0 ** -25, 0x9999
    rng = np.random.default_rng(800)
    s, s256 = _binary_key(rng, N), _binary_key(rng, 256)
    s_lwe = _u64([1, 1])
    eng.set_keygen_secret(SECRET)
    noise = {}                                                  # kind -> (call index, row number, recovered noise words, extra tolerance)
    # call 1: LWE table (n_out = 70: row 0 has one noise word; take the first six rows)
    key = eng.generate_keyswitch_key(s[:70], s_lwe, 2, 2, sigma, seed)
    rows = eng.export_key_rows(key, 0, 6)
    key.free()
    with np.errstate(over="ignore"):
        e5 = np.array([rows[r, 70] - (rows[r, :70] * s[:70]).sum(dtype=np.uint64) - np.uint64((int(s_lwe[0]) * (r % 3 + 1) << (64 - (r // 3 + 1) * 2)) & M64) for r in range(6)])
    # call 2: table key
    key = eng.generate_table_key(0, s256, s_lwe, 2, 2, sigma, seed)
    row = eng.export_key_rows(key, 1, 1).reshape(2, 256)
    key.free()
    noise[R.KIND_TABLE] = (2, 1, row[1] - oracle.poly_naive_mul(row[0].copy(), s256) - _table_message(0, 1, s256, s_lwe, 2, 2, 2, 1), 0.0)
    # call 3: bootstrap key (DFT image)
    key = eng.generate_bootstrap_key(s, s_lwe, 2, 8, sigma, seed)
    dft = key.export_dft()
    key.free()
    a = R.mask_row(seed, 1, N)
    err = float(oracle.torus_dist(oracle.dft_to_torus(np.ascontiguousarray(dft[0, 1, 0])), a + _u64([1 << 48] + [0] * (N - 1))).max())
    noise[R.KIND_BSK] = (3, 1, oracle.dft_to_torus(np.ascontiguousarray(dft[0, 1, 1])) - oracle.poly_naive_mul(a, s), _dft_body_tolerance(err, s, sigma))
    # call 4: unfolded bootstrap key (torus-domain image); entry 3 = "both bits set" carries message 1: row 3 * 4 + 2 has it on the body
    key = eng.generate_bootstrap_key_unfolded(s, s_lwe, 2, 8, sigma, seed, 2)
    image = eng.export_bootstrap_key(key).view(np.uint64).reshape(4, 4, 2, N)
    key.free()
    assert (image[3, 2, 0] == R.mask_row(seed, 14, N)).all()
    noise[R.KIND_BSK_UNFOLDED] = (4, 14, image[3, 2, 1] - oracle.poly_naive_mul(image[3, 2, 0].copy(), s) - _u64([1 << 56] + [0] * (N - 1)), 0.0)
    # call 5: TRLWE key-switch keys (DFT image)
    keys = eng.generate_trlwe_ks_keys(s, s[None], 2, 8, sigma, seed)
    dft = engine.slot_order_to_oracle(eng.export_trlwe_ks_keys(keys), N)
    keys.free()
    err = float(oracle.torus_dist(oracle.dft_to_torus(np.ascontiguousarray(dft[0, 1, 0])), a).max())
    noise[R.KIND_TRLWE_KSK] = (5, 1, oracle.dft_to_torus(np.ascontiguousarray(dft[0, 1, 1])) - oracle.poly_naive_mul(a, s) - (s << np.uint64(48)), _dft_body_tolerance(err, s, sigma))

    for r in range(6):
        _check_noise(e5[r:r + 1], KEY, R.call_nonce(1, R.KIND_TLWE_KSK), r, sigma, what="call 1 (LWE table)")
    for kind, (call, r, e, extra) in noise.items():
        _check_noise(e, KEY, R.call_nonce(call, kind), r, sigma, extra_tol=extra, what="call %d (kind %d)" % (call, kind))
        others = [(call - 1, kind), (call + 1, kind)] + [(call, other) for other in range(1, 6) if other != kind] + [(kind, call), (0, kind)]
        for c2, k2 in others:
            assert _noise_mismatch(e, KEY, R.call_nonce(c2, k2), r, sigma) > 2.0 ** -3, (call, kind, c2, k2)
    # the LWE table has one noise word per row: six rows, none of them within tolerance of a neighbouring stream
    for c2, k2 in ((2, R.KIND_TLWE_KSK), (0, R.KIND_TLWE_KSK)) + tuple((1, other) for other in range(1, 5)):
        off = [abs(int(e5[r].astype(np.int64)) - int(R.noise_row(KEY, R.call_nonce(c2, k2), r, 1, sigma)[0])) for r in range(6)]
        assert min(off) > R.noise_tolerance(sigma) and max(off) > 2.0 ** -3 * sigma * 2.0 ** 64, (c2, k2, off)
    _report("generator kinds")


@pytest.mark.gpu
def test_seed_chain_reaches_the_device_generators(eng, oracle, native_lib):
    """mosfhet_seed with the host layer's engine running: the device generators' secret is the first 32 bytes of the seeded host stream (and the host stream goes on
    behind them), so the table key generated next is call 1 under that secret -- noise included."""
    L, seed = native_lib, 0x5EEDC4A1
    L.mosfhet_engine_ctx.restype = C.c_void_p
    L.mosfhet_seed.argtypes = [C.c_uint64]
    L.generate_random_bytes.argtypes = [C.c_uint64, C.c_void_p]
    L.generate_random_bytes.restype = None
    assert L.mosfhet_engine_ctx()                           # the host layer's engine is running from here on
    L.mosfhet_seed(seed)
    ref = R.HostStream(seed)
    secret = R.key_words(ref.bytes(32))
    N, n, t, bb, sigma, mask_seed = 256, 2, 2, 2, 2.0 ** -15, 0xFACE
    rng = np.random.default_rng(900)
    s_out, s_in = _binary_key(rng, N), _u64([1, 1])
    key = eng.generate_table_key(0, s_out, s_in, t, bb, sigma, mask_seed)
    rows = eng.export_key_rows(key, 0, n * t * 3).reshape(-1, 2, N)
    key.free()
    for r, row in enumerate(rows):
        assert (row[0] == R.mask_row(mask_seed, r, N)).all(), r
        e = row[1] - oracle.poly_naive_mul(row[0].copy(), s_out) - _table_message(0, r, s_out, s_in, n, t, bb, 1)
        want = R.noise_row(secret, R.call_nonce(1, R.KIND_TABLE), r, N, sigma)
        assert np.abs((e.astype(np.int64) - want).astype(np.float64)).max() <= R.noise_tolerance(sigma), r
        assert _noise_mismatch(e, KEY, R.call_nonce(1, R.KIND_TABLE), r, sigma) > 2.0 ** -3        # not the secret the other tests install
    buf = (C.c_uint8 * 72)()
    L.generate_random_bytes(72, buf)
    assert bytes(buf) == ref.bytes(72)                      # the host stream goes on behind the 32 bytes
    eng.set_keygen_secret(SECRET)
