"""The contract of mosfhet_hip_trgsw_logic_batch (include/mosfhet_hip.h) restated from the oracle's primitives -- dft_to_torus, external_product, trgsw_to_dft -- and the
circuits its tests use.  Nothing here goes through the library under test.

A wire is a TRGSW_DFT sample in the ORACLE's slot order (oracle.trgsw_to_dft of torus words); a gate's result is kept as the torus-domain rows "before F", which is
what the tests compare: the device's selector must equal eng.torus_to_dft of them, and eng.dft_to_torus of the device's selector must give them back."""
import numpy as np

NOT, AND, NAND, OR, NOR, XOR, XNOR, ANDNOT, MUX = range(9)
U64 = np.uint64


def trivial_one(N, l, Bg_bit, mu=1):
    """the trivial TRGSW sample of mu: row r = c l + i holds mu 2^(64 - (i + 1) Bg_bit) at coefficient 0 of component c -> [2l][2][N] uint64"""
    h = np.zeros((2 * l, 2, N), dtype=U64)
    for c in range(2):
        for i in range(l):
            h[c * l + i, c, 0] = U64((int(mu) << (64 - (i + 1) * Bg_bit)) % 2 ** 64)
    return h


def rows_of(oracle, S):
    """T(S): [2l][2][N] float64 (oracle slot order) -> [2l][2][N] uint64, polynomial by polynomial"""
    return np.stack([np.stack([oracle.dft_to_torus(np.ascontiguousarray(S[r, c])) for c in range(2)]) for r in range(S.shape[0])])


def product_rows(oracle, L, W, l, Bg_bit):
    """row r: E(L_r, W) -- the external product of the TRLWE sample L[r] [2][N] with the sample W, reference order"""
    with oracle.product_order("reference"):
        return np.stack([oracle.external_product(np.ascontiguousarray(L[r]), W, l, Bg_bit) for r in range(L.shape[0])])


def gate_rows(oracle, op, X, Y, Z, l, Bg_bit):
    """the rows of one gate before F (the table of include/mosfhet_hip.h), uint64 arithmetic mod 2^64; X, Y, Z: wires (float64 [2l][2][N]) or None"""
    N = X.shape[-1]
    H = trivial_one(N, l, Bg_bit)
    TX = rows_of(oracle, X)
    if op == NOT:
        return H - TX
    TY = rows_of(oracle, Y)
    if op == MUX:
        return TY + product_rows(oracle, TX - TY, Z, l, Bg_bit)
    P = product_rows(oracle, TX, Y, l, Bg_bit)
    two = U64(2)
    return {AND: lambda: P, NAND: lambda: H - P, OR: lambda: TX + TY - P, NOR: lambda: H - TX - TY + P, XOR: lambda: TX + TY - two * P,
            XNOR: lambda: H - TX - TY + two * P, ANDNOT: lambda: TX - P}[op]()


def circuit_rows(oracle, gates, inputs, l, Bg_bit, in_dft=None):
    """inputs: [n_in][2l][2][N] uint64 torus words of one batch element (or in_dft: the wires themselves, a list of float64 [2l][2][N]) -> the rows before F of every
    gate, [n_gates][2l][2][N] uint64.  A gate's wire is oracle.trgsw_to_dft of its rows: F polynomial by polynomial."""
    wires = list(in_dft) if in_dft is not None else [oracle.trgsw_to_dft(np.ascontiguousarray(w), 1, l) for w in inputs]
    out = []
    for op, x, y, z in gates:
        rows = gate_rows(oracle, int(op), wires[x], wires[y] if y >= 0 else None, wires[z] if z >= 0 else None, l, Bg_bit)
        out.append(rows)
        wires.append(oracle.trgsw_to_dft(np.ascontiguousarray(rows), 1, l))
    return np.stack(out)


def levels_of(gates, n_in):
    """level(g) = 1 + the highest level of g's operands, inputs at level 0"""
    lv = []
    for op, x, y, z in gates:
        lv.append(1 + max([0] + [lv[w - n_in] for w in (x, y, z) if w >= n_in]))
    return lv


def truth(op, x, y=0, z=0):
    return {NOT: 1 - x, AND: x & y, NAND: 1 - (x & y), OR: x | y, NOR: 1 - (x | y), XOR: x ^ y, XNOR: 1 - (x ^ y), ANDNOT: x & (1 - y), MUX: x if z else y}[op]


def evaluate(gates, bits):
    """the cleartext value on every gate's wire"""
    w = list(bits)
    for op, x, y, z in gates:
        w.append(truth(op, w[x], w[y] if y >= 0 else 0, w[z] if z >= 0 else 0))
    return w[len(bits):]


# ---------------------------------------------------------------- circuits ----------------------------------------------------------------
def every_op_circuit():
    """n_in = 3, 12 gates, three levels, every op; gate 4 has x = y, gate 10 (MUX) reads gates of levels 1 and 2 and another of level 1, input 0 is read by five gates"""
    return 3, [(NOT, 0, -1, -1),      # g0  w3   level 1
               (AND, 0, 1, -1),       # g1  w4   1
               (NAND, 1, 2, -1),      # g2  w5   1
               (OR, 0, 2, -1),        # g3  w6   1
               (XOR, 0, 0, -1),       # g4  w7   1, x = y
               (NOR, 4, 2, -1),       # g5  w8   2
               (XNOR, 5, 0, -1),      # g6  w9   2
               (ANDNOT, 6, 3, -1),    # g7  w10  2
               (MUX, 0, 1, 2),        # g8  w11  1, inputs only
               (AND, 8, 1, -1),       # g9  w12  3
               (MUX, 4, 8, 5),        # g10 w13  3: x of level 1, y of level 2, z of level 1
               (XOR, 9, 10, -1)]      # g11 w14  3


def incrementer(bits=4):
    """a + 1 on `bits` input wires (least significant first): s_0 = NOT a_0, c_1 = a_0; s_i = c_i XOR a_i, c_{i+1} = c_i AND a_i with the carry in x (the deeper wire).
    Returns (n_in, gates, the wires of the sum bits)."""
    gates, sums = [(NOT, 0, -1, -1)], [bits]
    carry = 0
    for i in range(1, bits):
        gates.append((XOR, carry, i, -1))
        sums.append(bits + len(gates) - 1)
        if i + 1 < bits:
            gates.append((AND, carry, i, -1))
            carry = bits + len(gates) - 1
    return bits, gates, sums


def demultiplexer(bits=3):
    """one-hot lines of a `bits`-bit address: the NOTs, then per line a chain of ANDs with the partial product in x.  Returns (n_in, gates, the wires of the 2^bits lines)."""
    gates = [(NOT, i, -1, -1) for i in range(bits)]
    lit = lambda i, v: i if v else bits + i
    lines = []
    for a in range(1 << bits):
        acc = lit(0, a & 1)
        for i in range(1, bits):
            gates.append((AND, acc, lit(i, (a >> i) & 1), -1))
            acc = bits + len(gates) - 1
        lines.append(acc)
    return bits, gates, lines


def chain(op, depth, accumulated_left=True):
    """n_in = depth + 1: w = in_0; w = op(w, in_k) (accumulated wire in x) or op(in_k, w) for k = 1 .. depth"""
    gates, acc = [], 0
    for k in range(1, depth + 1):
        gates.append((op, acc, k, -1) if accumulated_left else (op, k, acc, -1))
        acc = depth + 1 + len(gates) - 1
    return depth + 1, gates


# ---------------------------------------------------------------- samples and noise ----------------------------------------------------------------
def encrypted_bits(oracle, rng, bits, s, l, Bg_bit, sigma):
    """TRGSW samples of the given bits under the ring key s [1][N] -> [len(bits)][2l][2][N] uint64"""
    from trlwe_gsw_linear_reference import trgsw_of_polynomial
    N = s.shape[1]
    out = []
    for b in bits:
        mu = np.zeros(N, dtype=np.int64)
        mu[0] = int(b)
        out.append(trgsw_of_polynomial(oracle, rng, mu, s, l, Bg_bit, sigma))
    return np.stack(out)


def probe(oracle, rng, s, sigma):
    """a TRLWE sample of 4-bit messages in slots of 2^60 -> (sample [2][N], messages [N])"""
    N = s.shape[1]
    m = (rng.words(N) % U64(16)) << U64(60)
    return oracle.trlwe_sample(rng, m, s, sigma), m


def selector_error(oracle, rows, bit, d, m, s, l, Bg_bit):
    """the worst phase error of oracle.external_product(d, S) against bit * m, S the selector whose rows before F are `rows`"""
    S = oracle.trgsw_to_dft(np.ascontiguousarray(rows), 1, l)
    with oracle.product_order("reference"):
        out = oracle.external_product(d, S, l, Bg_bit)
    want = m if bit else np.zeros_like(m)
    return float(oracle.torus_dist(oracle.trlwe_phase(out, s), want).max())
