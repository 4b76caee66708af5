"""ctypes binding of the C ABI in include/mosfhet_hip.h.

Torus64 buffers are torch.int64 CUDA tensors (same bits as uint64; torch has no full uint64 support).
Every function launches on torch's current stream of the engine's device.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# parameter sets of the reference's benchmarks (test/benchmark.c:53-54 and :64-75)
PARAMS_SET1 = dict(n=585, N=1024, k=1, l=2, Bg_bit=8, t=5, base_bit=2,
                   lwe_sigma=9.141776004202573e-5, rlwe_sigma=2.989040792967434e-8)
PARAMS_LVL2 = dict(n=632, N=2048, k=1, l=4, Bg_bit=9, t=8, base_bit=4,
                   lwe_sigma=2.0 ** -15, rlwe_sigma=2.0 ** -44)
# the reference's SET_2 (its default, test/tests.c:43-45) and SET_3 (:47-49), eprint 2022/704 table 4
PARAMS_SET2 = dict(n=744, N=2048, k=1, l=1, Bg_bit=23, t=5, base_bit=3,
                   lwe_sigma=7.747831515176779e-6, rlwe_sigma=2.2148688116005568e-16)
PARAMS_SET3 = dict(n=807, N=4096, k=1, l=1, Bg_bit=22, t=5, base_bit=3,
                   lwe_sigma=1.0562341599676662e-6, rlwe_sigma=2.168404344971009e-19)


class MosfhetHipError(RuntimeError):
    pass


def lib_path():
    return os.path.join(_HERE, "libmosfhet_hip.so")


def lib():
    """Load the native library; fail loudly if it has not been built (no fallback path exists)."""
    global _LIB
    if _LIB is None:
        # torch bundles its own HIP runtime (torch/lib/libamdhip64.so, same SONAME as /opt/rocm's).  Import it
        # first so this process holds ONE runtime: loading ours first would bind torch to a second, mismatched
        # runtime/HSA pair and the device disappears ("no HIP device visible").
        import torch  # noqa: F401
        path = lib_path()
        if not os.path.exists(path):
            raise MosfhetHipError(
                "native library %s is missing: run `python -m mosfhet_amd.build` (or __graft_entry__.build())" % path)
        L = C.CDLL(path)
        L.mosfhet_hip_last_error.restype = C.c_char_p
        L.mosfhet_hip_version.restype = C.c_char_p
        L.mosfhet_hip_bsk_bytes.restype = C.c_size_t
        L.mosfhet_hip_bsk_bytes.argtypes = [C.c_void_p]
        _LIB = L
    return _LIB


def _check(rc):
    if rc != 0:
        raise MosfhetHipError("mosfhet_hip error %d: %s" % (rc, lib().mosfhet_hip_last_error().decode()))


def to_device(a, device):
    """numpy uint64 array -> torch.int64 CUDA tensor with the same bits."""
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(device)


def to_numpy(t):
    """torch.int64 tensor -> numpy uint64 array with the same bits."""
    return t.detach().cpu().numpy().view(np.uint64)


def _ptr(t):
    assert t.is_cuda and t.is_contiguous(), "expected a contiguous CUDA tensor"
    return C.c_void_p(t.data_ptr())


PRODUCT_ORDERS = ("auto", "reference", "by_component")                                                           # MOSFHET_HIP_ORDER_*
KERNEL_FAMILIES = ("throughput", "latency", "split", "latency_by_component", "throughput_by_component")         # MOSFHET_HIP_FAMILY_*


def bootstrap_plan(N, l, Bg_bit, count, order="auto", cus=256, rows=1, galois=False):
    """Which kernel family a bootstrap launch takes (no device needed; the launchers' own decision at the current batch-threshold setters, `cus` in place of the
    device's CU count): dict(family, by_component, rounds).  include/mosfhet_hip.h: mosfhet_hip_bootstrap_plan."""
    plan = (C.c_int * 4)()
    _check(lib().mosfhet_hip_bootstrap_plan(int(N), int(l), int(Bg_bit), int(count), int(rows), int(bool(galois)), PRODUCT_ORDERS.index(order), int(cus), plan))
    return dict(family=KERNEL_FAMILIES[plan[0]], by_component=bool(plan[1]), rounds=int(plan[2]))


LEVELED_LUT_MAX_LEVELS = 10                                                                                     # MOSFHET_HIP_LUT_MAX_LEVELS


def leveled_lut_plan(N, l, size, count, cus=256):
    """What a leveled_lut call will do (no device needed): dict(levels, nodes, chunk, workspace_bytes) -- tree levels, first-level nodes, inputs per chunk and the
    bytes of the prepared table rows plus one chunk's intermediates.  include/mosfhet_hip.h: mosfhet_hip_leveled_lut_plan."""
    plan = (C.c_longlong * 4)()
    _check(lib().mosfhet_hip_leveled_lut_plan(int(N), int(l), int(size), int(count), int(cus), plan))
    return dict(levels=int(plan[0]), nodes=int(plan[1]), chunk=int(plan[2]), workspace_bytes=int(plan[3]))


LEVELED_LUT_MAX_TABLES = 64                                                                                     # MOSFHET_HIP_LUT_MAX_TABLES


def leveled_lut_tables_plan(N, l, size, tables, count, cus=256):
    """What a leveled_lut_tables call will do (no device needed): dict(levels, nodes, chunk, tables_per_pass, workspace_bytes, group) -- tree levels, first-level
    nodes per table, inputs per chunk, tables per pass, tables_per_pass * (prepared rows + one chunk's intermediates) and the tables per finishing workgroup.
    include/mosfhet_hip.h: mosfhet_hip_leveled_lut_tables_plan."""
    plan = (C.c_longlong * 6)()
    _check(lib().mosfhet_hip_leveled_lut_tables_plan(int(N), int(l), int(size), int(tables), int(count), int(cus), plan))
    return dict(levels=int(plan[0]), nodes=int(plan[1]), chunk=int(plan[2]), tables_per_pass=int(plan[3]), workspace_bytes=int(plan[4]), group=int(plan[5]))


def set_leveled_lut_tables_group(group):
    """Tables per finishing workgroup of leveled_lut_tables (0 restores the default); capped by the LDS of a CU and by the tables of a pass.  Results do not
    depend on it."""
    _check(lib().mosfhet_hip_set_leveled_lut_tables_group(int(group)))


def set_leveled_lut_workspace(nbytes):
    """Workspace bound of leveled_lut (0 restores the default of 1 GiB): batches that need more run in chunks of whole inputs; results do not depend on it."""
    _check(lib().mosfhet_hip_set_leveled_lut_workspace(C.c_longlong(int(nbytes))))


def lut_bits_plan(N, l, size, tables, count, cus=256):
    """What a lut_bits call will do (no device needed): dict(chunk, chunks, selector_bytes, cb_bits, lut) -- inputs per chunk, chunks, bytes of one chunk's
    selectors, bits per circuit-bootstrap launch and leveled_lut_tables_plan's dict for one chunk.  include/mosfhet_hip.h: mosfhet_hip_lut_bits_plan."""
    plan = (C.c_longlong * 10)()
    _check(lib().mosfhet_hip_lut_bits_plan(int(N), int(l), int(size), int(tables), int(count), int(cus), plan))
    return dict(chunk=int(plan[0]), chunks=int(plan[1]), selector_bytes=int(plan[2]), cb_bits=int(plan[3]),
                lut=dict(levels=int(plan[4]), nodes=int(plan[5]), chunk=int(plan[6]), tables_per_pass=int(plan[7]), workspace_bytes=int(plan[8]), group=int(plan[9])))


def leveled_lut_packed_plan(N, l, size, tables, pack_log, count, cus=256):
    """What a leveled_lut_packed call will do (no device needed): leveled_lut_tables_plan's dict at the packed levels and nodes, plus steps (rotate steps of the
    finish) and outputs (per input, tables * 2^pack_log).  include/mosfhet_hip.h: mosfhet_hip_leveled_lut_packed_plan."""
    plan = (C.c_longlong * 8)()
    _check(lib().mosfhet_hip_leveled_lut_packed_plan(int(N), int(l), int(size), int(tables), int(pack_log), int(count), int(cus), plan))
    return dict(levels=int(plan[0]), nodes=int(plan[1]), chunk=int(plan[2]), tables_per_pass=int(plan[3]), workspace_bytes=int(plan[4]), group=int(plan[5]),
                steps=int(plan[6]), outputs=int(plan[7]))


def trlwe_ram_plan(N, l, size, count, write=False, cus=256):
    """What a trlwe_ram_read / trlwe_ram_write call will do (no device needed): dict(cells, launches, chunk, workspace_bytes, products) -- cells per input, kernel
    launches, inputs per chunk, bytes of one chunk's intermediates (0 for a write and for size 1) and external products of the call.
    include/mosfhet_hip.h: mosfhet_hip_trlwe_ram_plan."""
    plan = (C.c_longlong * 5)()
    _check(lib().mosfhet_hip_trlwe_ram_plan(int(N), int(l), int(size), int(count), int(bool(write)), int(cus), plan))
    return dict(cells=int(plan[0]), launches=int(plan[1]), chunk=int(plan[2]), workspace_bytes=int(plan[3]), products=int(plan[4]))


AUTOMATON_MAX_STATES = 4096    # MOSFHET_HIP_AUTOMATON_MAX_STATES
AUTOMATON_MAX_STEPS = 4096     # MOSFHET_HIP_AUTOMATON_MAX_STEPS


def trlwe_automaton_plan(N, l, states, layers, steps, count, start=-1, cus=256):
    """What a trlwe_automaton call will do (no device needed): dict(launches, chunk, workspace_bytes, products, buffers) -- kernel launches (one per step and chunk),
    inputs per chunk, bytes of one chunk's state-vector buffers (buffers * chunk * states * 2N * 8), external products of the call
    (count * (states * (steps - 1) + (states if start < 0 else 1))) and buffers (0 for one step, 1 for two, else 2).
    include/mosfhet_hip.h: mosfhet_hip_trlwe_automaton_plan."""
    plan = (C.c_longlong * 5)()
    _check(lib().mosfhet_hip_trlwe_automaton_plan(int(N), int(l), int(states), int(layers), int(steps), int(start), int(count), int(cus), plan))
    return dict(launches=int(plan[0]), chunk=int(plan[1]), workspace_bytes=int(plan[2]), products=int(plan[3]), buffers=int(plan[4]))


class _Handle:
    """What the handle classes share: self.h is the native handle, _destroy the symbol that gives it back."""
    _destroy = None

    def close(self):
        if self.h:
            getattr(lib(), self._destroy)(self.h)
            self.h = None

    free = close


class Automaton(_Handle):
    """The transition tables of a deterministic weighted automaton / layered branching program (mosfhet_hip_automaton_t): made by automaton_create or
    Engine.automaton_create, shared by every call and batch that runs it."""
    _destroy = "mosfhet_hip_automaton_destroy"

    def __init__(self, handle):
        self.h = handle
        v = (C.c_longlong * 3)()
        _check(lib().mosfhet_hip_automaton_info(self.h, v))
        self.N, self.states, self.layers = int(v[0]), int(v[1]), int(v[2])

    def info(self):
        return dict(N=self.N, states=self.states, layers=self.layers)


def automaton_create(next0, next1, rot0, rot1, N):
    """An Automaton from host tables (no device needed: the packed table is copied to a device by the first call that runs there).  next0, next1, rot0, rot1: integer
    arrays [layers][states] ([states]: one layer, a time-invariant automaton); in state q of layer t mod layers a symbol 0 leads to next0[q] and multiplies by
    X^rot0[q], a symbol 1 to next1[q] with X^rot1[q].  next in [0, states), rot in [0, 2N); N in {1024, 2048}."""
    tabs = [np.atleast_2d(np.ascontiguousarray(a, dtype=np.int32)) for a in (next0, next1, rot0, rot1)]
    assert all(a.ndim == 2 and a.shape == tabs[0].shape for a in tabs), [a.shape for a in tabs]
    h = C.c_void_p()
    _check(lib().mosfhet_hip_automaton_create(C.byref(h), *[a.ctypes.data_as(C.c_void_p) for a in tabs], int(tabs[0].shape[1]), int(tabs[0].shape[0]), int(N)))
    return Automaton(h)


SELLOGIC_MAX_WIRES = 4096      # MOSFHET_HIP_SELLOGIC_MAX_WIRES
SEL_NOT, SEL_AND, SEL_NAND, SEL_OR, SEL_NOR, SEL_XOR, SEL_XNOR, SEL_ANDNOT, SEL_MUX = range(9)   # MOSFHET_HIP_SEL_*


def trgsw_logic_plan(N, l, n_in, n_gates, levels, widest_level, count, cus=256):
    """What a trgsw_logic call will do (no device needed): dict(launches, teams, products, inverses, forwards) -- kernel launches (one per level and chunk of batch
    elements), teams of the widest launch, and the external products, inverse and forward transforms of n_gates AND gates (count * 2l * n_gates products; a circuit's
    own count is count * 2l * SelLogic.product_gates).  include/mosfhet_hip.h: mosfhet_hip_trgsw_logic_plan."""
    plan = (C.c_longlong * 5)()
    _check(lib().mosfhet_hip_trgsw_logic_plan(int(N), int(l), int(n_in), int(n_gates), int(levels), int(widest_level), int(count), int(cus), plan))
    return dict(launches=int(plan[0]), teams=int(plan[1]), products=int(plan[2]), inverses=int(plan[3]), forwards=int(plan[4]))


class SelLogic(_Handle):
    """A circuit of gates over TRGSW_DFT selectors (mosfhet_hip_sellogic_t): made by sellogic_create or Engine.sellogic_create, shared by every call and batch."""
    _destroy = "mosfhet_hip_sellogic_destroy"

    def __init__(self, handle):
        self.h = handle
        v = (C.c_longlong * 5)()
        _check(lib().mosfhet_hip_sellogic_info(self.h, v))
        self.N, self.n_in, self.n_gates, self.levels, self.product_gates = (int(x) for x in v)

    def info(self):
        return dict(N=self.N, n_in=self.n_in, n_gates=self.n_gates, levels=self.levels, product_gates=self.product_gates)


def sellogic_create(gates, n_in, N):
    """A SelLogic from a host gate list (no device needed: the packed table is copied to a device by the first call that runs there).  gates: integers [n_gates][4] =
    {op, x, y, z} with op one of SEL_NOT .. SEL_MUX; wires 0 .. n_in - 1 are the inputs, wire n_in + g the output of gate g; a gate reads inputs and EARLIER gates
    only, and the fields it does not use are -1 (NOT: y, z; MUX uses all three, z ? x : y; the others: z).  N in {1024, 2048}."""
    g = np.ascontiguousarray(gates, dtype=np.int32)
    assert g.ndim == 2 and g.shape[1] == 4, g.shape
    h = C.c_void_p()
    _check(lib().mosfhet_hip_sellogic_create(C.byref(h), g.ctypes.data_as(C.c_void_p), int(g.shape[0]), int(n_in), int(N)))
    return SelLogic(h)


TRGSW_ENCRYPT_OUTPUTS = ("dft", "both", "torus")    # with_torus_out of mosfhet_hip_trgsw_encrypt_plan


def trgsw_encrypt_plan(N, l, count, outputs="dft"):
    """What a trgsw_encrypt call will do (no device needed): dict(launches, workgroups, workspace_bytes, chunks) -- kernel launches (a row launch and, with a DFT
    output, a transform per chunk of at most 2^20 rows), workgroups of the widest launch, bytes of pooled torus rows (DFT-only calls) and chunks.  outputs: "dft",
    "both" or "torus".  include/mosfhet_hip.h: mosfhet_hip_trgsw_encrypt_plan."""
    info = (C.c_int64 * 4)()
    _check(lib().mosfhet_hip_trgsw_encrypt_plan(int(N), int(l), int(count), TRGSW_ENCRYPT_OUTPUTS.index(outputs), info))
    return dict(launches=int(info[0]), workgroups=int(info[1]), workspace_bytes=int(info[2]), chunks=int(info[3]))


class ClientKey(_Handle):
    """Secret keys for the encrypt and phase calls (mosfhet_hip_client_key_t): made by client_key_create, shared by every engine, call and host thread."""
    _destroy = "mosfhet_hip_client_key_destroy"

    def __init__(self, handle):
        self.h = handle
        v = (C.c_int64 * 6)()
        _check(lib().mosfhet_hip_client_key_info(self.h, v))
        self.N, self.n, self.rlwe_weight, self.lwe_weight = int(v[0]), int(v[1]), int(v[2]), int(v[4])
        self.rlwe_binary, self.lwe_binary = bool(v[3]), bool(v[5])

    def info(self):
        return dict(N=self.N, n=self.n, rlwe_weight=self.rlwe_weight, rlwe_binary=self.rlwe_binary, lwe_weight=self.lwe_weight, lwe_binary=self.lwe_binary)


def client_key_create(s_rlwe=None, s_lwe=None):
    """A ClientKey from host keys (no device needed: the packed key is copied to a device by the first call that runs there).  s_rlwe: [N] words, N a power of two in
    256 .. 4096; s_lwe: [n] words; either may be None; coefficients are binary or small signed integers (they must fit 16 bits)."""
    keys = [None if s is None else np.ascontiguousarray(s, dtype=np.uint64).reshape(-1) for s in (s_rlwe, s_lwe)]
    ptr = [None if s is None else s.ctypes.data_as(C.c_void_p) for s in keys]
    h = C.c_void_p()
    _check(lib().mosfhet_hip_client_key_create(C.byref(h), ptr[0], 0 if keys[0] is None else int(keys[0].size), ptr[1], 0 if keys[1] is None else int(keys[1].size)))
    return ClientKey(h)


def lut_bits_packed_plan(N, l, size, tables, pack_log, count, cus=256):
    """What a lut_bits_packed call will do (no device needed): lut_bits_plan's dict with leveled_lut_packed_plan's dict for one chunk as `lut`.
    include/mosfhet_hip.h: mosfhet_hip_lut_bits_packed_plan."""
    plan = (C.c_longlong * 12)()
    _check(lib().mosfhet_hip_lut_bits_packed_plan(int(N), int(l), int(size), int(tables), int(pack_log), int(count), int(cus), plan))
    return dict(chunk=int(plan[0]), chunks=int(plan[1]), selector_bytes=int(plan[2]), cb_bits=int(plan[3]),
                lut=dict(levels=int(plan[4]), nodes=int(plan[5]), chunk=int(plan[6]), tables_per_pass=int(plan[7]), workspace_bytes=int(plan[8]), group=int(plan[9]),
                         steps=int(plan[10]), outputs=int(plan[11])))


def set_lut_bits_workspace(nbytes):
    """Bound of lut_bits' selector workspace (0 restores the default of 2 GiB): batches whose selectors need more run in chunks of whole inputs; with a key whose
    product order is set, results do not depend on it."""
    _check(lib().mosfhet_hip_set_lut_bits_workspace(C.c_longlong(int(nbytes))))


def tlwe_linear_plan(rows_out, rows_in, n, count, nnz=-1, narrow=True, cus=256):
    """What a tlwe_linear call will do (no device needed; the launcher's own decision): dict(form, tj, words_per_lane, workgroups, grid_folds, passes,
    input_bytes, multiply) -- "dense" / "sparse", output rows per wavefront, words per lane, workgroups, gridDim.y (gridDim.x = ceil(workgroups / grid_folds)),
    passes over the input = ceil(rows_out / tj), passes * count * rows_in * (n + 1) * 8 and "narrow" / "wide".  include/mosfhet_hip.h: mosfhet_hip_tlwe_linear_plan."""
    plan = (C.c_longlong * 8)()
    _check(lib().mosfhet_hip_tlwe_linear_plan(int(rows_out), int(rows_in), C.c_longlong(int(nnz)), int(narrow), int(n), int(count), int(cus), plan))
    return dict(form=("dense", "sparse")[plan[0]], tj=int(plan[1]), words_per_lane=int(plan[2]), workgroups=int(plan[3]), grid_folds=int(plan[4]), passes=int(plan[5]),
                input_bytes=int(plan[6]), multiply=("narrow", "wide")[plan[7]])


def tlwe_pack_plan(N, n_in, t, total, per, split=0, cus=256, workspace_bytes=0):
    """What a tlwe_pack call will do (no device needed; the launcher's own decision): dict(outputs, split, part_entries, outputs_per_round, rounds, teams,
    staging_bytes, key_bytes) -- TRLWE samples written, parts the entries are cut into (split = 0 asks for a recommendation on `cus` CUs), entries per part,
    outputs per round of the transposed staging, rounds, teams of a round's main launch, bytes of a round's staging and key bytes one team reads.
    workspace_bytes = 0: the current setting.  include/mosfhet_hip.h: mosfhet_hip_tlwe_pack_plan."""
    plan = (C.c_longlong * 8)()
    _check(lib().mosfhet_hip_tlwe_pack_plan(int(N), int(n_in), int(t), int(total), int(per), int(split), int(cus), C.c_longlong(int(workspace_bytes)), plan))
    return dict(outputs=int(plan[0]), split=int(plan[1]), part_entries=int(plan[2]), outputs_per_round=int(plan[3]), rounds=int(plan[4]), teams=int(plan[5]),
                staging_bytes=int(plan[6]), key_bytes=int(plan[7]))


def set_tlwe_pack_workspace(nbytes):
    """Bound of tlwe_pack's transposed staging (0 restores the default of 256 MiB): batches that need more run in rounds of whole outputs; results do not depend
    on it."""
    _check(lib().mosfhet_hip_set_tlwe_pack_workspace(C.c_longlong(int(nbytes))))


def _c_int(x):
    """x as a C int, refused here when it does not fit one (ctypes would wrap it silently)"""
    x = int(x)
    if not -2 ** 31 <= x < 2 ** 31:
        raise MosfhetHipError("argument %d does not fit a C int" % x)
    return x


KS_FORMS = ("small", "words", "tiles_256", "tiles_512")


def trlwe_unpack_plan(N, n_out=0, t=0, base_bit=0, total=0, per=None, compressed=False, cus=256):
    """What a trlwe_unpack (n_out = 0) or trlwe_unpack_keyswitch call will do (no device needed; the launchers' own decision at the current set_ks_words):
    dict(outputs, form, pieces, prepass_workgroups, prepass_bytes, saved_bytes, pool_bytes, rows_per_workgroup) -- packed inputs read, form of the switch ("small":
    up to 16 samples, unpacked first; "words"; "tiles_256"; "tiles_512"), pieces (ceil(total / 8192) for "words"), workgroups and written bytes of the pre-pass that
    reads the packed samples, bytes of the [total][N + 1] batch that is never written, pool bytes and samples per workgroup of trlwe_unpack's kernel.
    include/mosfhet_hip.h: mosfhet_hip_trlwe_unpack_plan."""
    plan = (C.c_longlong * 8)()
    _check(lib().mosfhet_hip_trlwe_unpack_plan(int(N), int(n_out), int(t), int(base_bit), int(bool(compressed)), int(total), int(N if per is None else per), int(cus), plan))
    return dict(outputs=int(plan[0]), form=KS_FORMS[plan[1]], pieces=int(plan[2]), prepass_workgroups=int(plan[3]), prepass_bytes=int(plan[4]), saved_bytes=int(plan[5]),
                pool_bytes=int(plan[6]), rows_per_workgroup=int(plan[7]))


def trlwe_unpack_strided_plan(N, n_out=0, t=0, base_bit=0, total=0, per=None, first=0, stride=1, compressed=False, cus=256):
    """trlwe_unpack_plan for a call with a geometry: sample j of an input is the coefficient first + j stride.  The geometry is checked as the calls check it (first in
    0 .. N - 1, stride >= 1, first + (per - 1) stride <= N - 1) and changes no field.  include/mosfhet_hip.h: mosfhet_hip_trlwe_unpack_strided_plan."""
    plan = (C.c_longlong * 8)()
    _check(lib().mosfhet_hip_trlwe_unpack_strided_plan(int(N), int(n_out), int(t), int(base_bit), int(bool(compressed)), int(total), int(N if per is None else per),
                                                       C.c_int(_c_int(first)), C.c_int(_c_int(stride)), int(cus), plan))
    return dict(outputs=int(plan[0]), form=KS_FORMS[plan[1]], pieces=int(plan[2]), prepass_workgroups=int(plan[3]), prepass_bytes=int(plan[4]), saved_bytes=int(plan[5]),
                pool_bytes=int(plan[6]), rows_per_workgroup=int(plan[7]))


TRACE_KINDS = ("trace_pack", "rlwe_priv_keyswitch", "trgsw_from_gadget")


def trace_plan(kind, N, t, base_bit, entries, entry0=0, l=1, count=1):
    """The shape of a tlwe_trace_pack / trlwe_rlwe_priv_keyswitch / trgsw_from_gadget call, checked as the calls check it (no device needed): kind one of TRACE_KINDS,
    entries what the key set holds.  dict(entries_read, teams, threads, forwards, inverses, key_bytes) -- key entries a team reads, teams of the launch, threads per
    team, forward and inverse transforms per team, key bytes a team reads.  include/mosfhet_hip.h: mosfhet_hip_trace_plan."""
    plan = (C.c_longlong * 6)()
    _check(lib().mosfhet_hip_trace_plan(TRACE_KINDS.index(kind), int(N), int(t), int(base_bit), int(entries), int(entry0), int(l), int(count), plan))
    return dict(entries_read=int(plan[0]), teams=int(plan[1]), threads=int(plan[2]), forwards=int(plan[3]), inverses=int(plan[4]), key_bytes=int(plan[5]))


def tlwe_trace_pack_many_plan(N, t, base_bit, entries, total, log_per, entry0=0, workspace_bytes=0):
    """What a tlwe_trace_pack_many call will do (no device needed; the launcher's own decision): dict(outputs, launches_per_round, teams, merge_steps, tail_steps,
    outputs_per_round, rounds, pool_bytes) -- TRLWE samples written, launches of a round (one per level; one for log_per = 0), teams of a round's first launch, merges
    (2^log_per - 1) and trace steps (log2 N - log_per) per output, outputs per round of the pool, rounds, pool bytes of a round.  workspace_bytes = 0: the current
    set_tlwe_pack_workspace.  include/mosfhet_hip.h: mosfhet_hip_tlwe_trace_pack_many_plan."""
    plan = (C.c_longlong * 8)()
    _check(lib().mosfhet_hip_tlwe_trace_pack_many_plan(int(N), int(t), int(base_bit), int(entries), int(entry0), int(total), int(log_per), C.c_longlong(int(workspace_bytes)), plan))
    return dict(outputs=int(plan[0]), launches_per_round=int(plan[1]), teams=int(plan[2]), merge_steps=int(plan[3]), tail_steps=int(plan[4]), outputs_per_round=int(plan[5]),
                rounds=int(plan[6]), pool_bytes=int(plan[7]))


def trlwe_linear_plan(N, rows_out, rows_in, count, nnz=-1, extract=False, cus=256, workspace_bytes=0):
    """What a trlwe_linear / trlwe_linear_extract call will do (no device needed; the launcher's own decision): dict(teams, per_round, rounds, pool_bytes, forwards,
    inverses, weight_bytes, input_bytes) -- teams of a round's main launch (one per batch element and output row), batch elements per round of the pool, rounds, pool
    bytes of a round, forward (count * rows_in * 2) and inverse (count * rows_out * 2) transforms per call, weight and input bytes one team reads (sparse: of the mean
    row).  workspace_bytes = 0: the current set_tlwe_pack_workspace.  include/mosfhet_hip.h: mosfhet_hip_trlwe_linear_plan."""
    plan = (C.c_longlong * 8)()
    _check(lib().mosfhet_hip_trlwe_linear_plan(int(N), int(rows_out), int(rows_in), C.c_longlong(int(nnz)), int(count), int(bool(extract)), int(cus),
                                               C.c_longlong(int(workspace_bytes)), plan))
    return dict(teams=int(plan[0]), per_round=int(plan[1]), rounds=int(plan[2]), pool_bytes=int(plan[3]), forwards=int(plan[4]), inverses=int(plan[5]),
                weight_bytes=int(plan[6]), input_bytes=int(plan[7]))


class PolyLinearMap(_Handle):
    """The cleartext polynomial weights of y = W x + bias on packed TRLWE samples, transformed, on the device (mosfhet_hip_polylinear_t): made by
    Engine.polylinear_create_dense / Engine.polylinear_create_sparse."""
    _destroy = "mosfhet_hip_polylinear_destroy"

    def __init__(self, engine, handle):
        self.engine, self.h = engine, handle
        i = self.info()
        self.rows_out, self.rows_in, self.N = i["rows_out"], i["rows_in"], i["N"]

    def info(self):
        v = (C.c_longlong * 6)()
        _check(lib().mosfhet_hip_polylinear_info(self.h, v))
        return dict(rows_out=int(v[0]), rows_in=int(v[1]), nnz=int(v[2]), N=int(v[3]), nbytes=int(v[4]), form=("dense", "sparse")[v[5]])


def trlwe_gsw_linear_plan(N, l, rows_out, rows_in, count, nnz=-1, extract=False, cus=256, workspace_bytes=0):
    """What a trlwe_gsw_linear / trlwe_gsw_linear_extract call will do (no device needed; the launcher's own decision): dict(teams, per_round, rounds, pool_bytes,
    forwards, inverses, weight_bytes, digit_bytes) -- teams of a round's main launch (one per batch element and output row), batch elements per round of the pool, rounds,
    pool bytes of a round, forward (count * rows_in * 2l) and inverse (count * rows_out * 2) transforms per call, weight and digit bytes one team reads (sparse: of the
    mean row).  workspace_bytes = 0: the current set_tlwe_pack_workspace.  include/mosfhet_hip.h: mosfhet_hip_trlwe_gsw_linear_plan."""
    plan = (C.c_longlong * 8)()
    _check(lib().mosfhet_hip_trlwe_gsw_linear_plan(int(N), int(l), int(rows_out), int(rows_in), C.c_longlong(int(nnz)), int(count), int(bool(extract)), int(cus),
                                                   C.c_longlong(int(workspace_bytes)), plan))
    return dict(teams=int(plan[0]), per_round=int(plan[1]), rounds=int(plan[2]), pool_bytes=int(plan[3]), forwards=int(plan[4]), inverses=int(plan[5]),
                weight_bytes=int(plan[6]), digit_bytes=int(plan[7]))


class GswLinearMap(_Handle):
    """The encrypted polynomial weights (TRGSW_DFT samples) of y = W x + bias on packed TRLWE samples, on the device (mosfhet_hip_gswlinear_t): made by
    Engine.gswlinear_create_dense / _sparse / _from_selectors."""
    _destroy = "mosfhet_hip_gswlinear_destroy"

    def __init__(self, engine, handle):
        self.engine, self.h = engine, handle
        i = self.info()
        self.rows_out, self.rows_in, self.N, self.l, self.Bg_bit = i["rows_out"], i["rows_in"], i["N"], i["l"], i["Bg_bit"]

    def info(self):
        v = (C.c_longlong * 8)()
        _check(lib().mosfhet_hip_gswlinear_info(self.h, v))
        return dict(rows_out=int(v[0]), rows_in=int(v[1]), nnz=int(v[2]), N=int(v[3]), l=int(v[4]), Bg_bit=int(v[5]), nbytes=int(v[6]),
                    form=("dense", "sparse", "selectors")[v[7]])


class LinearMap(_Handle):
    """The cleartext weights of y = W x + bias on the device (mosfhet_hip_linear_t): made by Engine.linear_dense / Engine.linear_sparse."""
    _destroy = "mosfhet_hip_linear_destroy"

    def __init__(self, engine, handle):
        self.engine, self.h = engine, handle
        i = self.info()
        self.rows_out, self.rows_in = i["rows_out"], i["rows_in"]

    def info(self):
        v = (C.c_longlong * 6)()
        _check(lib().mosfhet_hip_linear_info(self.h, v))
        return dict(rows_out=int(v[0]), rows_in=int(v[1]), nnz=int(v[2]), narrow=bool(v[3]), nbytes=int(v[4]), form=("dense", "sparse")[v[5]])


class BootstrapKey:
    def __init__(self, engine, handle, n, k, N, l, Bg_bit):
        self.engine, self.h = engine, handle
        self.n, self.k, self.N, self.l, self.Bg_bit = n, k, N, l, Bg_bit

    @property
    def nbytes(self):
        return lib().mosfhet_hip_bsk_bytes(self.h)

    def set_product_order(self, order):
        """Summation order of this key's external products: "auto" (the kernel chosen for the batch size decides: the default), "reference" (one chain over all rows:
        never a split kernel) or "by_component" (the split kernels' order at every batch size).  include/mosfhet_hip.h: mosfhet_hip_bsk_set_product_order."""
        if order not in PRODUCT_ORDERS:
            raise MosfhetHipError("product order %r: one of %s" % (order, ", ".join(PRODUCT_ORDERS)))
        _check(lib().mosfhet_hip_bsk_set_product_order(self.h, PRODUCT_ORDERS.index(order)))

    @property
    def product_order(self):
        v = C.c_int(0)
        _check(lib().mosfhet_hip_bsk_get_product_order(self.h, C.byref(v)))
        return PRODUCT_ORDERS[v.value]

    def export_dft(self):
        out = np.empty((self.n, (self.k + 1) * self.l, self.k + 1, self.N), dtype=np.float64)
        _check(lib().mosfhet_hip_bsk_export_dft(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def free(self):
        if self.h:
            lib().mosfhet_hip_bsk_destroy(self.h)
            self.h = None


class KeySwitchKey:
    def __init__(self, engine, handle, n_in, n_out, t, base_bit):
        self.engine, self.h = engine, handle
        self.n_in, self.n_out, self.t, self.base_bit = n_in, n_out, t, base_bit

    @property
    def nbytes(self):
        lib().mosfhet_hip_ksk_bytes.restype = C.c_size_t
        lib().mosfhet_hip_ksk_bytes.argtypes = [C.c_void_p]
        return lib().mosfhet_hip_ksk_bytes(self.h)

    def free(self):
        if self.h:
            lib().mosfhet_hip_ksk_destroy(self.h)
            self.h = None


class AutomorphismKeys:
    def __init__(self, engine, handle, N, t, base_bit):
        self.engine, self.h, self.N, self.t, self.base_bit = engine, handle, N, t, base_bit

    def free(self):
        if self.h:
            lib().mosfhet_hip_gak_destroy(self.h)
            self.h = None


class Engine:
    """One engine per (process, GPU): wraps mosfhet_hip_ctx_t."""

    def __init__(self, device=0):
        import torch
        if not torch.cuda.is_available():
            raise MosfhetHipError("no GPU visible: mosfhet_amd has no CPU fallback")
        self.torch = torch
        self.device = torch.device("cuda", device)
        self.h = C.c_void_p()
        _check(lib().mosfhet_hip_ctx_create(C.byref(self.h), int(device)))

    def close(self):
        if self.h:
            lib().mosfhet_hip_ctx_destroy(self.h)
            self.h = None

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def pace_skip_credit(self):
        """paced launches of this device that will still skip the team rendezvous because an earlier launch's wait ran out (synchronises the device)"""
        v = C.c_int()
        _check(lib().mosfhet_hip_pace_skip_credit(self.h, C.byref(v)))
        return v.value

    def empty(self, *shape):
        return self.torch.empty(*shape, dtype=self.torch.int64, device=self.device)

    # ---- keys ----
    def load_bootstrap_key(self, bk_torus, k, l, Bg_bit):
        """bk_torus: numpy uint64 [n][(k+1)l][k+1][N] (torus domain) -> device DFT key."""
        bk_torus = np.ascontiguousarray(bk_torus, dtype=np.uint64)
        n, rows, k1, N = bk_torus.shape
        assert rows == (k + 1) * l and k1 == k + 1
        h = C.c_void_p()
        _check(lib().mosfhet_hip_bsk_create(self.h, C.byref(h), bk_torus.ctypes.data_as(C.c_void_p), n, k, N, l, Bg_bit))
        return BootstrapKey(self, h, n, k, N, l, Bg_bit)

    def load_bootstrap_key_unfolded(self, su, l, Bg_bit, unfolding):
        """su: numpy uint64 [n 2^u/u][2l][2][N] (torus domain) -> device key taking the unfolded blind rotation."""
        su = np.ascontiguousarray(su, dtype=np.uint64)
        cnt, rows, two, N = su.shape
        n = cnt * unfolding >> unfolding
        h = C.c_void_p()
        _check(lib().mosfhet_hip_bsk_unfolded_create(self.h, C.byref(h), su.ctypes.data_as(C.c_void_p), n, N, l, Bg_bit, unfolding))
        return BootstrapKey(self, h, n, 1, N, l, Bg_bit)

    def load_bootstrap_key_device(self, d_bk, k, l, Bg_bit):
        n, rows, k1, N = d_bk.shape
        h = C.c_void_p()
        _check(lib().mosfhet_hip_bsk_create_from_device(self.h, C.byref(h), _ptr(d_bk), n, k, N, l, Bg_bit, self._stream()))
        self.torch.cuda.current_stream(self.device).synchronize()
        return BootstrapKey(self, h, n, k, N, l, Bg_bit)

    def load_keyswitch_key(self, ksk, base_bit):
        ksk = np.ascontiguousarray(ksk, dtype=np.uint64)
        n_in, t, per_j, row = ksk.shape
        assert per_j == (1 << base_bit) - 1
        h = C.c_void_p()
        _check(lib().mosfhet_hip_ksk_create(self.h, C.byref(h), ksk.ctypes.data_as(C.c_void_p), n_in, row - 1, t, base_bit))
        return KeySwitchKey(self, h, n_in, row - 1, t, base_bit)

    def load_automorphism_keys(self, ak_torus, base_bit):
        """ak_torus: numpy uint64 [N][t][2][N] (torus domain, entry j for generator 2j+1)."""
        ak_torus = np.ascontiguousarray(ak_torus, dtype=np.uint64)
        N, t, two, N2 = ak_torus.shape
        assert two == 2 and N2 == N
        h = C.c_void_p()
        _check(lib().mosfhet_hip_gak_create(self.h, C.byref(h), ak_torus.ctypes.data_as(C.c_void_p), N, t, base_bit))
        return AutomorphismKeys(self, h, N, t, base_bit)

    def load_trlwe_ks_keys(self, rows, base_bit):
        """rows: numpy uint64 [entries][t][2][N] (torus domain) -> device FFT key-switch key set."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        entries, t, two, N = rows.shape
        h = C.c_void_p()
        _check(lib().mosfhet_hip_trlwe_ksk_create(self.h, C.byref(h), rows.ctypes.data_as(C.c_void_p), entries, N, t, base_bit))
        return AutomorphismKeys(self, h, N, t, base_bit)

    def generate_trlwe_ks_keys(self, s_out, msgs, t, base_bit, sigma, seed):
        """On-device FFT key-switch key set: entry e switches from the polynomial msgs[e] to the binary key s_out."""
        s_out = np.ascontiguousarray(s_out, dtype=np.uint64)
        msgs = np.ascontiguousarray(msgs, dtype=np.uint64).reshape(-1, s_out.size)
        h = C.c_void_p()
        _check(lib().mosfhet_hip_trlwe_ksk_generate(self.h, C.byref(h), s_out.ctypes.data_as(C.c_void_p), s_out.size, msgs.ctypes.data_as(C.c_void_p),
                                                    msgs.shape[0], t, base_bit, C.c_double(sigma), C.c_uint64(seed)))
        return AutomorphismKeys(self, h, s_out.size, t, base_bit)

    def export_trlwe_ks_keys(self, tks):
        """The engine's image of an FFT key-switch key set (mosfhet_hip_trlwe_ksk_export): float64 [entries][t][2][N], DFT domain, the engine's slot order
        (slot_order_to_oracle brings a polynomial into the oracle's)."""
        info = (C.c_int * 4)()
        _check(lib().mosfhet_hip_trlwe_ksk_info(tks.h, info))
        entries, N, t, _ = info
        out = np.empty((entries, t, 2, N), dtype=np.float64)
        lib().mosfhet_hip_trlwe_ksk_bytes.restype = C.c_size_t
        lib().mosfhet_hip_trlwe_ksk_bytes.argtypes = [C.c_void_p]
        if lib().mosfhet_hip_trlwe_ksk_bytes(tks.h) != out.nbytes:
            raise MosfhetHipError("key-switch key set of %d bytes, %d expected" % (lib().mosfhet_hip_trlwe_ksk_bytes(tks.h), out.nbytes))
        _check(lib().mosfhet_hip_trlwe_ksk_export(tks.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def load_packing1_key(self, rows, base_bit):
        """rows: numpy uint64 [n][t][2^bb-1][2][N] -> device LWE -> TRLWE packing key."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        n, t, per_j, two, N = rows.shape
        h = C.c_void_p()
        _check(lib().mosfhet_hip_packing1_ksk_create(self.h, C.byref(h), rows.ctypes.data_as(C.c_void_p), n, N, t, base_bit))
        return KeySwitchKey(self, h, n, 2 * N - 1, t, base_bit)

    def trlwe_keyswitch(self, tks, entry, ct, out=None):
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, 2, tks.N)
        _check(lib().mosfhet_hip_trlwe_keyswitch_batch(self.h, tks.h, int(entry), _ptr(out), _ptr(ct), count, self._stream()))
        return out

    def trlwe_priv_keyswitch_2(self, tks, ct, out=None):
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, 2, tks.N)
        _check(lib().mosfhet_hip_trlwe_priv_keyswitch_2_batch(self.h, tks.h, _ptr(out), _ptr(ct), count, self._stream()))
        return out

    def trlwe_packing1_keyswitch(self, ksk, ct, out=None):
        count = ct.shape[0]
        N = (ksk.n_out + 1) // 2
        if out is None:
            out = self.empty(count, 2, N)
        _check(lib().mosfhet_hip_trlwe_packing1_keyswitch_batch(self.h, ksk.h, _ptr(out), _ptr(ct), count, self._stream()))
        return out

    @staticmethod
    def _level_events(level_events, l):
        """l torch.cuda.Event objects (or None entries) -> the void*[l] the *_batch_ev entry points take; an event is recorded when its gadget level is final"""
        if level_events is None:
            return None
        if len(level_events) != l:
            raise MosfhetHipError("level_events: %d events for %d gadget levels" % (len(level_events), l))
        arr = (C.c_void_p * l)()
        for i, e in enumerate(level_events):
            if e is not None:
                e.record()   # (a torch event has no handle before its first record; the engine records it again where it belongs)
                arr[i] = e.cuda_event
        return arr

    def circuit_bootstrap_3(self, bsk, kska, kskb, ct, out=None, level_events=None):
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, 2 * bsk.l, 2, bsk.N)
        ev = self._level_events(level_events, bsk.l)
        _check(lib().mosfhet_hip_circuit_bootstrap_3_batch_ev(self.h, bsk.h, kska.h, kskb.h, _ptr(out), _ptr(ct), count, self._stream(), ev))
        return out

    def circuit_bootstrap_3_dft(self, bsk, kska, kskb, ct, out=None):
        """circuit_bootstrap_3 followed by trgsw_to_dft in one call, without the torus-domain TRGSWs in between: [count][2l][2][N] doubles, word for word
        trgsw_to_dft(circuit_bootstrap_3(...)); reshaped to [count / size][size][2l][2][N] it is leveled_lut's sel_dft."""
        count = ct.shape[0]
        if out is None:
            out = self.torch.empty((count, 2 * bsk.l, 2, bsk.N), dtype=self.torch.float64, device=self.device)
        assert tuple(out.shape) == (count, 2 * bsk.l, 2, bsk.N) and out.dtype == self.torch.float64, tuple(out.shape)
        _check(lib().mosfhet_hip_circuit_bootstrap_3_dft_batch(self.h, bsk.h, kska.h, kskb.h, _ptr(out), _ptr(ct), count, self._stream()))
        return out

    def lut_bits(self, bsk, kska, kskb, luts, ct, ksk_out=None, out=None):
        """A size-bit -> tables-bit function on a batch of inputs given as LWE-encrypted bits: circuit_bootstrap_3 -> trgsw_to_dft -> leveled_lut_tables
        (-> tlwe_keyswitch with ksk_out) in one call, the selectors a bounded internal workspace.  ct: [count][size][n + 1], bit i of input b at [b][i];
        luts: [tables][max(1, 2^size / N)][2][N], read only; returns [count][tables][n + 1] with ksk_out (the ct of the next call when tables == size), else
        [count][tables][N + 1]."""
        count, size, tables, N = ct.shape[0], ct.shape[1], luts.shape[0], bsk.N
        assert tuple(ct.shape) == (count, size, bsk.n + 1), tuple(ct.shape)
        assert tuple(luts.shape) == (tables, max(1, (1 << size) // N), 2, N), tuple(luts.shape)
        width = (bsk.n if ksk_out is not None else N) + 1
        if out is None:
            out = self.empty(count, tables, width)
        assert tuple(out.shape) == (count, tables, width)
        _check(lib().mosfhet_hip_lut_bits_batch(self.h, bsk.h, kska.h, kskb.h, ksk_out.h if ksk_out is not None else None, _ptr(out), _ptr(luts), _ptr(ct), int(size),
                                                int(tables), int(count), self._stream()))
        return out

    def lut_bits_plan(self, N, l, size, tables, count):
        """lut_bits_plan() at this device's CU count."""
        return lut_bits_plan(N, l, size, tables, count, self.torch.cuda.get_device_properties(self.device).multi_processor_count)

    def lut_bits_packed(self, bsk, kska, kskb, luts, ct, pack_log, ksk_out=None, out=None):
        """lut_bits with m = 2^pack_log output bits packed into every table entry (leveled_lut_packed in the middle).  ct: [count][size][n + 1];
        luts: [tables][max(1, 2^(size + pack_log) / N)][2][N], read only; returns [count][tables * m][n + 1] with ksk_out (the ct of the next call when
        tables * m == size), else [count][tables * m][N + 1]."""
        count, size, tables, N = ct.shape[0], ct.shape[1], luts.shape[0], bsk.N
        assert tuple(ct.shape) == (count, size, bsk.n + 1), tuple(ct.shape)
        assert tuple(luts.shape) == (tables, max(1, (1 << (size + pack_log)) // N), 2, N), tuple(luts.shape)
        width = (bsk.n if ksk_out is not None else N) + 1
        if out is None:
            out = self.empty(count, tables << pack_log, width)
        assert tuple(out.shape) == (count, tables << pack_log, width)
        _check(lib().mosfhet_hip_lut_bits_packed_batch(self.h, bsk.h, kska.h, kskb.h, ksk_out.h if ksk_out is not None else None, _ptr(out), _ptr(luts), _ptr(ct),
                                                       int(size), int(tables), int(pack_log), int(count), self._stream()))
        return out

    def lut_bits_packed_plan(self, N, l, size, tables, pack_log, count):
        """lut_bits_packed_plan() at this device's CU count."""
        return lut_bits_packed_plan(N, l, size, tables, pack_log, count, self.torch.cuda.get_device_properties(self.device).multi_processor_count)

    def public_mux(self, p0, p1, sel, Bg_bit, out=None):
        count, l, two, N = sel.shape
        if out is None:
            out = self.empty(count, 2, N)
        _check(lib().mosfhet_hip_public_mux_batch(self.h, _ptr(out), _ptr(p0), _ptr(p1), _ptr(sel), N, l, Bg_bit, count, self._stream()))
        return out

    def full_domain_functional_bootstrap_KS21(self, bsk, pksk, tv, ct, torus_base, variant=0, out=None):
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, bsk.N + 1)
        _check(lib().mosfhet_hip_full_domain_functional_bootstrap_KS21_batch(self.h, bsk.h, pksk.h, _ptr(out), _ptr(tv), _ptr(ct), count, torus_base,
                                                                             variant, self._stream()))
        return out

    def multivalue_bootstrap_phase1(self, bsk, ct, torus_base, out=None):
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, torus_base + 1, 2, bsk.N)
        _check(lib().mosfhet_hip_multivalue_bootstrap_phase1_batch(self.h, bsk.h, _ptr(out), _ptr(ct), count, torus_base, self._stream()))
        return out

    def multivalue_bootstrap_phase2(self, lut, rotated, torus_base, log_torus_base, out=None):
        count, _, _, N = rotated.shape
        if out is None:
            out = self.empty(count, N + 1)
        h_lut = (C.c_int * torus_base)(*[int(x) for x in lut])
        _check(lib().mosfhet_hip_multivalue_bootstrap_phase2_batch(self.h, _ptr(out), h_lut, _ptr(rotated), N, torus_base, log_torus_base, count,
                                                                   self._stream()))
        return out

    def load_priv_key(self, rows, base_bit):
        """rows: numpy uint64 [n+1][t][2^bb-1][2][N] -> device table-lookup private key-switch key."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        n1, t, per_j, two, N = rows.shape
        h = C.c_void_p()
        _check(lib().mosfhet_hip_priv_ksk_create(self.h, C.byref(h), rows.ctypes.data_as(C.c_void_p), n1 - 1, N, t, base_bit))
        return KeySwitchKey(self, h, n1, 2 * N - 1, t, base_bit)

    def trlwe_priv_keyswitch(self, ksk, ct, out=None):
        count = ct.shape[0]
        N = (ksk.n_out + 1) // 2
        if out is None:
            out = self.empty(count, 2, N)
        _check(lib().mosfhet_hip_trlwe_priv_keyswitch_batch(self.h, ksk.h, _ptr(out), _ptr(ct), count, self._stream()))
        return out

    def circuit_bootstrap(self, bsk, kska, kskb, ct, variant=0, out=None, level_events=None):
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, 2 * bsk.l, 2, bsk.N)
        ev = self._level_events(level_events, bsk.l)
        _check(lib().mosfhet_hip_circuit_bootstrap_batch_ev(self.h, bsk.h, kska.h, kskb.h, _ptr(out), _ptr(ct), count, variant, self._stream(), ev))
        return out

    def functional_bootstrap_trgsw_phase1(self, bsk, ct, torus_base, out=None):
        count = ct.shape[0]
        if out is None:
            out = self.torch.empty(count, 2 * bsk.l, 2, bsk.N, dtype=self.torch.float64, device=self.device)
        _check(lib().mosfhet_hip_functional_bootstrap_trgsw_phase1_batch(self.h, bsk.h, _ptr(out), _ptr(ct), count, torus_base, self._stream()))
        return out

    def functional_bootstrap_trgsw_phase2(self, bsk, g_dft, tv, out=None):
        count = g_dft.shape[0]
        if out is None:
            out = self.empty(count, bsk.N + 1)
        _check(lib().mosfhet_hip_functional_bootstrap_trgsw_phase2_batch(self.h, bsk.h, _ptr(out), _ptr(g_dft), _ptr(tv), tv.shape[0], count,
                                                                         self._stream()))
        return out

    def trlwe_tensor_prod_FFT(self, rlk, c1, c2, precision, out=None):
        count = c1.shape[0]
        if out is None:
            out = self.empty(count, 2, rlk.N)
        _check(lib().mosfhet_hip_trlwe_tensor_prod_FFT_batch(self.h, rlk.h, _ptr(out), _ptr(c1), _ptr(c2), precision, count, self._stream()))
        return out

    def tlwe_mul(self, pksk, rlk, c1, c2, precision, out=None):
        count = c1.shape[0]
        if out is None:
            out = self.empty(count, rlk.N + 1)
        _check(lib().mosfhet_hip_tlwe_mul_batch(self.h, pksk.h, rlk.h, _ptr(out), _ptr(c1), _ptr(c2), precision, count, self._stream()))
        return out

    def full_domain_functional_bootstrap_CLOT21(self, bsk, pksk, rlk, tv, ct, precision, variant=0, out=None):
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, bsk.N + 1)
        _check(lib().mosfhet_hip_full_domain_functional_bootstrap_CLOT21_batch(self.h, bsk.h, pksk.h, rlk.h, _ptr(out), _ptr(tv), _ptr(ct), count,
                                                                               precision, variant, self._stream()))
        return out

    def multivalue_bootstrap_UBR_phase1(self, bsk, ct, unfolding, out=None):
        count = ct.shape[0]
        if out is None:
            out = self.torch.empty(count, bsk.n // unfolding, 2 * bsk.l, 2, bsk.N, dtype=self.torch.float64, device=self.device)
        _check(lib().mosfhet_hip_multivalue_bootstrap_UBR_phase1_batch(self.h, bsk.h, _ptr(out), _ptr(ct), count, self._stream()))
        return out

    def multivalue_bootstrap_UBR_phase2(self, bsk, tvs, ct, sa, torus_base, out=None):
        count, tv_count = ct.shape[0], tvs.shape[0]
        if out is None:
            out = self.empty(count, tv_count, bsk.N + 1)
        _check(lib().mosfhet_hip_multivalue_bootstrap_UBR_phase2_batch(self.h, bsk.h, _ptr(out), _ptr(tvs), tv_count, _ptr(ct), _ptr(sa), count,
                                                                       torus_base, self._stream()))
        return out

    def trlwe_mv_extract(self, ct, mode, amount, out=None):
        count, _, N = ct.shape
        if out is None:
            out = self.empty(count, amount, N + 1) if mode == 0 else self.empty(count, N + 1)
        _check(lib().mosfhet_hip_trlwe_mv_extract_batch(self.h, _ptr(out), _ptr(ct), N, mode, amount, count, self._stream()))
        return out

    @staticmethod
    def set_keygen_secret(key32):
        """Install the 256-bit ChaCha20 key the on-device generators draw their NOISE under (process-wide; default: from the operating system) and
        restart its per-call nonce sequence: the same secret followed by the same generate calls reproduces the same keys (tests, mosfhet_seed)."""
        key32 = bytes(key32)
        assert len(key32) == 32
        _check(lib().mosfhet_hip_set_keygen_secret(key32))

    def ks_words_gave_up(self):
        """wavefronts of the word-lane key-switch kernel whose bounded counter wait ran out since the library was loaded (0 unless something is broken)"""
        n = C.c_uint()
        _check(lib().mosfhet_hip_ks_words_gave_up(self.h, C.byref(n)))
        return n.value

    def generate_table_key(self, kind, s_out, s_in, t, base_bit, sigma, seed, compressed=False):
        """On-device packing (kind 0) / private (kind 1) key-switch key; returns a KeySwitchKey.  compressed: keep only the b halves in HBM and
        regenerate the masks inside the key-switch kernels (same rows, same results)."""
        s_out = np.ascontiguousarray(s_out, dtype=np.uint64)
        s_in = np.ascontiguousarray(s_in, dtype=np.uint64)
        h = C.c_void_p()
        gen = lib().mosfhet_hip_trlwe_table_ksk_generate_compressed if compressed else lib().mosfhet_hip_trlwe_table_ksk_generate
        _check(gen(self.h, C.byref(h), kind, s_out.ctypes.data_as(C.c_void_p), s_out.size,
                                                          s_in.ctypes.data_as(C.c_void_p), s_in.size, t, base_bit, C.c_double(sigma), C.c_uint64(seed)))
        return KeySwitchKey(self, h, s_in.size + kind, 2 * s_out.size - 1, t, base_bit)

    def generate_lut_packing_key(self, s_out, s_in, t, base_bit, torus_base, sigma, seed):
        """On-device LUT-packing key (trlwe_new_packing_KS_key, src/keyswitch.c:214-241): rows (i, e, j, v), n * torus_base digit sources."""
        s_out = np.ascontiguousarray(s_out, dtype=np.uint64)
        s_in = np.ascontiguousarray(s_in, dtype=np.uint64)
        h = C.c_void_p()
        _check(lib().mosfhet_hip_trlwe_lut_packing_ksk_generate(self.h, C.byref(h), s_out.ctypes.data_as(C.c_void_p), s_out.size, s_in.ctypes.data_as(C.c_void_p),
                                                                s_in.size, t, base_bit, torus_base, C.c_double(sigma), C.c_uint64(seed)))
        return KeySwitchKey(self, h, s_in.size * torus_base, 2 * s_out.size - 1, t, base_bit)

    def trlwe_lut_packing_keyswitch(self, ksk, torus_base, cts, out=None):
        """trlwe_packing_keyswitch (src/keyswitch.c:346-366) for a batch: cts [count][torus_base][n + 1] -> [count][2][N]"""
        count = cts.shape[0]
        N = (ksk.n_out + 1) // 2
        if out is None:
            out = self.empty(count, 2, N)
        _check(lib().mosfhet_hip_trlwe_lut_packing_keyswitch_batch(self.h, ksk.h, int(torus_base), _ptr(out), _ptr(cts), count, self._stream()))
        return out

    def generate_bootstrap_key(self, s_rlwe, s_lwe, l, Bg_bit, sigma, seed, ga=False):
        """On-device bootstrap key BK_i = TRGSW(s_lwe[i]) (ga: TRGSW(X^{s_lwe[i]})) under the binary TRLWE key s_rlwe."""
        s_rlwe = np.ascontiguousarray(s_rlwe, dtype=np.uint64)
        s_lwe = np.ascontiguousarray(s_lwe, dtype=np.uint64)
        h = C.c_void_p()
        if s_rlwe.ndim == 2:   # [k][N]: any k <= 3 / any ring the engine serves (general-ring path included)
            k, N = s_rlwe.shape
            if ga:
                raise MosfhetHipError("generate_bootstrap_key: the Galois form exists for k = 1 only")
            _check(lib().mosfhet_hip_bsk_generate_k(self.h, C.byref(h), s_rlwe.ctypes.data_as(C.c_void_p), k, N, s_lwe.ctypes.data_as(C.c_void_p), s_lwe.size,
                                                    l, Bg_bit, C.c_double(sigma), C.c_uint64(seed)))
            return BootstrapKey(self, h, s_lwe.size, k, N, l, Bg_bit)
        _check(lib().mosfhet_hip_bsk_generate(self.h, C.byref(h), s_rlwe.ctypes.data_as(C.c_void_p), s_rlwe.size, s_lwe.ctypes.data_as(C.c_void_p), s_lwe.size,
                                              l, Bg_bit, C.c_double(sigma), C.c_uint64(seed), int(ga)))
        return BootstrapKey(self, h, s_lwe.size, 1, s_rlwe.size, l, Bg_bit)

    def generate_bootstrap_key_unfolded(self, s_rlwe, s_lwe, l, Bg_bit, sigma, seed, unfolding):
        """On-device key of new_bootstrap_key(.., unfolding > 1): per group of `unfolding` key bits the 2^unfolding samples TRGSW(group spells j)."""
        s_rlwe = np.ascontiguousarray(s_rlwe, dtype=np.uint64)
        s_lwe = np.ascontiguousarray(s_lwe, dtype=np.uint64)
        h = C.c_void_p()
        _check(lib().mosfhet_hip_bsk_unfolded_generate(self.h, C.byref(h), s_rlwe.ctypes.data_as(C.c_void_p), s_rlwe.size, s_lwe.ctypes.data_as(C.c_void_p), s_lwe.size,
                                                       l, Bg_bit, C.c_double(sigma), C.c_uint64(seed), int(unfolding)))
        return BootstrapKey(self, h, s_lwe.size, 1, s_rlwe.size, l, Bg_bit)

    def generate_keyswitch_key(self, s_out, s_in, t, base_bit, sigma, seed, compressed=False):
        """On-device LWE -> LWE key-switch table (tlwe_new_KS_key) from the binary keys s_in (switched from) and s_out (switched to)."""
        s_out = np.ascontiguousarray(s_out, dtype=np.uint64)
        s_in = np.ascontiguousarray(s_in, dtype=np.uint64)
        h = C.c_void_p()
        _check(lib().mosfhet_hip_tlwe_ksk_generate(self.h, C.byref(h), s_out.ctypes.data_as(C.c_void_p), s_out.size, s_in.ctypes.data_as(C.c_void_p), s_in.size,
                                                   t, base_bit, C.c_double(sigma), C.c_uint64(seed), int(compressed)))
        return KeySwitchKey(self, h, s_in.size, s_out.size, t, base_bit)

    # ---- key images (on-disk formats; include/mosfhet_hip.h "Key images") ----
    def export_bootstrap_key(self, bsk):
        """The engine's own image of a bootstrap key (DFT rows; torus-domain samples for an unfolded key) as raw bytes."""
        out = np.empty(bsk.nbytes, dtype=np.uint8)
        _check(lib().mosfhet_hip_bsk_export(bsk.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def import_bootstrap_key(self, image, n, k, N, l, Bg_bit, unfolding=1):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        # the C ABI takes a bare pointer: the length is checked here (an image is mosfhet_hip_bsk_bytes long: DFT entries, or the torus-domain samples of an unfolded key)
        want = n * (k + 1) * l * (k + 1) * N * 8 if unfolding == 1 else (n << unfolding) // unfolding * 2 * l * 2 * N * 8
        if image.nbytes != want:
            raise MosfhetHipError("bootstrap-key image of %d bytes, %d expected for n=%d k=%d N=%d l=%d unfolding=%d" % (image.nbytes, want, n, k, N, l, unfolding))
        h = C.c_void_p()
        _check(lib().mosfhet_hip_bsk_import(self.h, C.byref(h), image.ctypes.data_as(C.c_void_p), n, k, N, l, Bg_bit, unfolding))
        return BootstrapKey(self, h, n, k, N, l, Bg_bit)

    def clone_key(self, key):
        """A copy of a key handle of ANOTHER engine (or this one) on this engine's device, device to device (mosfhet_hip_*_clone: SURVEY 8(e), keys
        replicated per GPU).  Returns (handle of the same class, route: 0 same device, 1 peer to peer, 2 device to device without peer access, 3 host bounce)."""
        h = C.c_void_p()
        if isinstance(key, BootstrapKey):
            _check(lib().mosfhet_hip_bsk_clone(self.h, C.byref(h), key.h))
            out = BootstrapKey(self, h, key.n, key.k, key.N, key.l, key.Bg_bit)
        elif isinstance(key, KeySwitchKey):
            _check(lib().mosfhet_hip_ksk_clone(self.h, C.byref(h), key.h))
            out = KeySwitchKey(self, h, key.n_in, key.n_out, key.t, key.base_bit)
        else:
            _check(lib().mosfhet_hip_gak_clone(self.h, C.byref(h), key.h))
            out = AutomorphismKeys(self, h, key.N, key.t, key.base_bit)
        return out, int(lib().mosfhet_hip_last_clone_route())

    def bootstrap_plan(self, bsk, count, rows=1, galois=False):
        """bootstrap_plan() for a key of this engine at its product order and this device's CU count."""
        cus = self.torch.cuda.get_device_properties(self.device).multi_processor_count
        return bootstrap_plan(bsk.N, bsk.l, bsk.Bg_bit, count, bsk.product_order, cus, rows, galois)

    def bootstrap_key_info(self, bsk):
        v = (C.c_int * 6)()
        _check(lib().mosfhet_hip_bsk_info(bsk.h, v))
        return tuple(v)

    def alloc_keyswitch_key(self, kind, n, n_out_or_N, t, base_bit):
        """Empty table key to be filled by import_keyswitch_rows: kind 0 LWE -> LWE (n_out), 1 packing (N), 2 private (N)."""
        h = C.c_void_p()
        _check(lib().mosfhet_hip_ksk_alloc(self.h, C.byref(h), kind, n, n_out_or_N, t, base_bit))
        return KeySwitchKey(self, h, n + (kind == 2), n_out_or_N if kind == 0 else 2 * n_out_or_N - 1, t, base_bit)

    def import_keyswitch_rows(self, ksk, first_row, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        assert rows.shape[1] == ksk.n_out + 1
        _check(lib().mosfhet_hip_ksk_import_rows(ksk.h, C.c_size_t(first_row), C.c_size_t(rows.shape[0]), rows.ctypes.data_as(C.c_void_p)))

    def export_key_rows(self, ksk, first_row, count):
        out = np.empty((count, ksk.n_out + 1), dtype=np.uint64)
        _check(lib().mosfhet_hip_ksk_export_rows(ksk.h, C.c_size_t(first_row), C.c_size_t(count), out.ctypes.data_as(C.c_void_p)))
        return out

    def keyswitch_functional_bootstrap(self, ksk, bsk, tv, ct, torus_base, extract=True, out=None):
        """tlwe_keyswitch N -> n followed by functional_bootstrap[_wo_extract] in one call."""
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, bsk.N + 1) if extract else self.empty(count, 2, bsk.N)
        _check(lib().mosfhet_hip_keyswitch_functional_bootstrap_batch(self.h, ksk.h, bsk.h, _ptr(out), _ptr(tv), self._tv(tv, bsk, count), _ptr(ct), count,
                                                                      torus_base, int(extract), self._stream()))
        return out

    def cmux(self, bsk, key_index, in0, in1, out=None):
        """out[b] = in0[b] + key[key_index] (.) (in1[b] - in0[b]); out may be in0."""
        count = in0.shape[0]
        if out is None:
            out = self.empty(count, bsk.k + 1, bsk.N)
        _check(lib().mosfhet_hip_cmux_batch(self.h, bsk.h, int(key_index), _ptr(out), _ptr(in0), _ptr(in1), count, self._stream()))
        return out

    def leveled_lut(self, sel_dft, lut, size, l, Bg_bit, out=None):
        """A shared look-up table evaluated on a batch of independent inputs given bit by bit as TRGSW_DFT selectors (eval_LUT of the reference's leveled
        application per input).  sel_dft: [count][size][2l][2][N] doubles (trgsw_to_dft of [count][size] TRGSW samples, bit i of input b at [b][i]);
        lut: [max(1, 2^size / N)][2][N] torus words, read only; returns [count][N + 1]."""
        count, N = sel_dft.shape[0], lut.shape[-1]
        assert tuple(sel_dft.shape) == (count, size, 2 * l, 2, N) and sel_dft.dtype == self.torch.float64, tuple(sel_dft.shape)
        assert tuple(lut.shape) == (max(1, (1 << size) // N), 2, N), tuple(lut.shape)
        if out is None:
            out = self.empty(count, N + 1)
        assert tuple(out.shape) == (count, N + 1)
        _check(lib().mosfhet_hip_leveled_lut_batch(self.h, _ptr(out), _ptr(sel_dft), _ptr(lut), int(size), int(N), int(l), int(Bg_bit), int(count), self._stream()))
        return out

    def leveled_lut_tables(self, sel_dft, luts, size, l, Bg_bit, out=None):
        """Several shared look-up tables evaluated on a batch of independent inputs, the selectors fetched once for all of them.  sel_dft as for leveled_lut;
        luts: [tables][max(1, 2^size / N)][2][N] torus words, read only; returns [count][tables][N + 1] -- out[b][tb] is leveled_lut's out[b] for table tb, and
        out.view(count * tables, N + 1) is the batch tlwe_keyswitch / circuit_bootstrap_3 take."""
        count, tables, N = sel_dft.shape[0], luts.shape[0], luts.shape[-1]
        assert tuple(sel_dft.shape) == (count, size, 2 * l, 2, N) and sel_dft.dtype == self.torch.float64, tuple(sel_dft.shape)
        assert tuple(luts.shape) == (tables, max(1, (1 << size) // N), 2, N), tuple(luts.shape)
        if out is None:
            out = self.empty(count, tables, N + 1)
        assert tuple(out.shape) == (count, tables, N + 1)
        _check(lib().mosfhet_hip_leveled_lut_tables_batch(self.h, _ptr(out), _ptr(sel_dft), _ptr(luts), int(size), int(N), int(l), int(Bg_bit), int(tables),
                                                          int(count), self._stream()))
        return out

    def leveled_lut_packed(self, sel_dft, luts, size, l, Bg_bit, pack_log, out=None):
        """Shared tables whose entries hold m = 2^pack_log output bits in adjacent coefficients, evaluated on a batch of independent inputs: one rotation chain per
        table, m sample extractions.  sel_dft as for leveled_lut; luts: [tables][max(1, 2^(size + pack_log) / N)][2][N] torus words, output t of entry x at
        coefficient (x m + t) mod N of TRLWE (x m + t) / N, read only; returns [count][tables][m][N + 1] -- out.view(count * tables * m, N + 1) is the batch
        tlwe_keyswitch takes.  pack_log = 0 is leveled_lut_tables."""
        count, tables, N = sel_dft.shape[0], luts.shape[0], luts.shape[-1]
        m = 1 << pack_log
        assert tuple(sel_dft.shape) == (count, size, 2 * l, 2, N) and sel_dft.dtype == self.torch.float64, tuple(sel_dft.shape)
        assert tuple(luts.shape) == (tables, max(1, (1 << (size + pack_log)) // N), 2, N), tuple(luts.shape)
        if out is None:
            out = self.empty(count, tables, m, N + 1)
        assert tuple(out.shape) == (count, tables, m, N + 1)
        _check(lib().mosfhet_hip_leveled_lut_packed_batch(self.h, _ptr(out), _ptr(sel_dft), _ptr(luts), int(size), int(N), int(l), int(Bg_bit), int(tables),
                                                          int(pack_log), int(count), self._stream()))
        return out

    def trlwe_ram_read(self, sel_dft, mem, size, l, Bg_bit, out=None):
        """Encrypted memory, read: every input b owns mem[b], 2^size TRLWE cells, and out[b] is the cell at the address its selectors encrypt (the CMUX tree over the
        cells, top address bit first).  sel_dft: [count][size][2l][2][N] doubles as for leveled_lut (bit i of input b's address at [b][i]); mem:
        [count][2^size][2][N] torus words, read only; returns [count][2][N]."""
        count, N = mem.shape[0], mem.shape[-1]
        assert tuple(sel_dft.shape) == (count, size, 2 * l, 2, N) and sel_dft.dtype == self.torch.float64, tuple(sel_dft.shape)
        assert tuple(mem.shape) == (count, 1 << size, 2, N), tuple(mem.shape)
        if out is None:
            out = self.empty(count, 2, N)
        assert tuple(out.shape) == (count, 2, N)
        _check(lib().mosfhet_hip_trlwe_ram_read_batch(self.h, _ptr(out), _ptr(sel_dft), _ptr(mem), int(size), int(N), int(l), int(Bg_bit), int(count), self._stream()))
        return out

    def trlwe_ram_write(self, sel_dft, mem, val, size, l, Bg_bit):
        """Encrypted memory, write, IN PLACE: cell i of mem[b] becomes the chain of `size` CMUXes between the cell and val[b] -- val[b] where i is the address the
        selectors of input b encrypt, the old cell elsewhere.  sel_dft and mem as for trlwe_ram_read; val: [count][2][N].  Returns mem."""
        count, N = mem.shape[0], mem.shape[-1]
        assert tuple(sel_dft.shape) == (count, size, 2 * l, 2, N) and sel_dft.dtype == self.torch.float64, tuple(sel_dft.shape)
        assert tuple(mem.shape) == (count, 1 << size, 2, N), tuple(mem.shape)
        assert tuple(val.shape) == (count, 2, N), tuple(val.shape)
        _check(lib().mosfhet_hip_trlwe_ram_write_batch(self.h, _ptr(mem), _ptr(sel_dft), _ptr(val), int(size), int(N), int(l), int(Bg_bit), int(count), self._stream()))
        return mem

    def trlwe_ram_plan(self, N, l, size, count, write=False):
        """trlwe_ram_plan() at this device's CU count."""
        return trlwe_ram_plan(N, l, size, count, write, self.torch.cuda.get_device_properties(self.device).multi_processor_count)

    def automaton_create(self, next0, next1, rot0, rot1, N):
        """automaton_create(): the handle is not tied to this engine's device."""
        return automaton_create(next0, next1, rot0, rot1, N)

    def trlwe_automaton(self, automaton, sel_dft, init, l, Bg_bit, start=-1, out=None):
        """Encrypted automaton: runs `automaton` backwards over every input's word of encrypted bits.  V_steps = init; for t = steps-1 .. 0 and every state q:
        V_t[b][q] = R0 + sel[b][t] (.) (R1 - R0) with R0 = X^rot0[q] V_{t+1}[b][next0[q]], R1 = X^rot1[q] V_{t+1}[b][next1[q]] of layer t mod layers.
        sel_dft: [count][steps][2l][2][N] doubles as for leveled_lut (symbol t of input b's word at [b][t]); init: [count][states][2][N] torus words, or
        [states][2][N], one vector shared by the batch; returns V_0 [count][states][2][N] with start < 0, else [count][2][N] = V_0[:, start] (the last launch then
        computes that state only).  A long word is streamed last chunk first by passing the result as the next call's init."""
        count, steps, N, S = sel_dft.shape[0], sel_dft.shape[1], init.shape[-1], automaton.states
        if N != automaton.N:
            raise MosfhetHipError("mosfhet_hip error -1: trlwe_automaton: the automaton was made for N = %d, the state vectors have N = %d" % (automaton.N, N))
        assert tuple(sel_dft.shape) == (count, steps, 2 * l, 2, N) and sel_dft.dtype == self.torch.float64, tuple(sel_dft.shape)
        shared = init.dim() == 3
        assert tuple(init.shape) == ((S, 2, N) if shared else (count, S, 2, N)), tuple(init.shape)
        shape = (count, S, 2, N) if start < 0 else (count, 2, N)
        if out is None:
            out = self.empty(*shape)
        assert tuple(out.shape) == shape, tuple(out.shape)
        _check(lib().mosfhet_hip_trlwe_automaton_batch(self.h, _ptr(out), automaton.h, _ptr(sel_dft), _ptr(init), int(shared), int(steps), int(start), int(l), int(Bg_bit),
                                                       int(count), self._stream()))
        return out

    def trlwe_automaton_plan(self, N, l, states, layers, steps, count, start=-1):
        """trlwe_automaton_plan() at this device's CU count."""
        return trlwe_automaton_plan(N, l, states, layers, steps, count, start, self.torch.cuda.get_device_properties(self.device).multi_processor_count)

    def sellogic_create(self, gates, n_in, N):
        """sellogic_create(): the handle is not tied to this engine's device."""
        return sellogic_create(gates, n_in, N)

    def trgsw_logic(self, circuit, in_dft, l, Bg_bit, out=None):
        """Selector logic: evaluates `circuit` on every batch element's input selectors and returns EVERY gate's output selector, [count][n_gates][2l][2][N] float64
        (row g = wire n_in + g: a sel_dft of the leveled calls with size = n_gates; pick outputs by index).  in_dft: [count][n_in][2l][2][N] float64 as for leveled_lut.
        One launch per level.  AND-like gates are not commutative in their noise: THE DEEPER WIRE GOES IN x (the left operand's noise is added, the right operand's
        is amplified), and a gate's output is usable only at a fine gadget with lvl2-sized noise such as (2048, 4, 9), sigma 2^-44 -- include/mosfhet_hip.h."""
        count, N = in_dft.shape[0], in_dft.shape[-1]
        if N != circuit.N:
            raise MosfhetHipError("mosfhet_hip error -1: trgsw_logic: the circuit was made for N = %d, the selectors have N = %d" % (circuit.N, N))
        assert tuple(in_dft.shape) == (count, circuit.n_in, 2 * l, 2, N) and in_dft.dtype == self.torch.float64, tuple(in_dft.shape)
        shape = (count, circuit.n_gates, 2 * l, 2, N)
        if out is None:
            out = self.torch.empty(shape, dtype=self.torch.float64, device=self.device)
        assert tuple(out.shape) == shape and out.dtype == self.torch.float64, tuple(out.shape)
        _check(lib().mosfhet_hip_trgsw_logic_batch(self.h, _ptr(out) if count else None, circuit.h, _ptr(in_dft) if count else None, int(l), int(Bg_bit), int(count),
                                                   self._stream()))
        return out

    def trgsw_logic_plan(self, N, l, n_in, n_gates, levels, widest_level, count):
        """trgsw_logic_plan() at this device's CU count."""
        return trgsw_logic_plan(N, l, n_in, n_gates, levels, widest_level, count, self.torch.cuda.get_device_properties(self.device).multi_processor_count)

    # ---- the client half: encrypt and open samples under a ClientKey (include/mosfhet_hip.h "The client half on the device") ----
    def tlwe_encrypt(self, key, msg, sigma, out=None):
        """TLWE samples of the torus words msg [count] under key's LWE key: [count][n + 1], out[i] = a_i, out[n] = sum a_i s_i + e + msg.  Masks and noise from
        ChaCha20 under the keygen secret, one nonce per call; refused on a capturing stream."""
        count = msg.shape[0]
        assert tuple(msg.shape) == (count,) and msg.dtype == self.torch.int64, tuple(msg.shape)
        if out is None:
            out = self.empty(count, key.n + 1)
        assert tuple(out.shape) == (count, key.n + 1), tuple(out.shape)
        _check(lib().mosfhet_hip_tlwe_encrypt_batch(self.h, key.h, _ptr(out) if count else None, _ptr(msg) if count else None, C.c_double(sigma), int(count), self._stream()))
        return out

    def trlwe_encrypt(self, key, msg, sigma, count=None, out=None):
        """TRLWE samples of the polynomials msg [count][N] (None: `count` samples of zero) under key's TRLWE key: [count][2][N], b = a * s + e + msg, the product
        exact.  Randomness and capture rule as for tlwe_encrypt."""
        if msg is not None:
            count = msg.shape[0]
            assert tuple(msg.shape) == (count, key.N) and msg.dtype == self.torch.int64, tuple(msg.shape)
        if out is None:
            out = self.empty(count, 2, key.N)
        assert tuple(out.shape) == (count, 2, key.N), tuple(out.shape)
        _check(lib().mosfhet_hip_trlwe_encrypt_batch(self.h, key.h, _ptr(out) if count else None, _ptr(msg) if msg is not None and count else None, C.c_double(sigma),
                                                     int(count), self._stream()))
        return out

    def trgsw_encrypt(self, key, m, l, Bg_bit, sigma, exp=None, torus=False, dft=True):
        """TRGSW samples of m[u] X^exp[u] (trgsw_monomial_sample; exp None: X^0) under key's TRLWE key.  m, exp: int32 tensors of one shape, e.g. [count][size] for
        the leveled calls' selectors.  Returns the TRGSW_DFT samples, shape + [2l][2][N] float64 (the sel_dft layout); torus=True: (dft, torus rows shape + [2l][2][N]
        int64), the doubles being torus_to_dft of exactly those rows; dft=False (with torus=True): the torus rows only.  Randomness and capture rule as for
        tlwe_encrypt."""
        assert dft or torus
        assert m.dtype == self.torch.int32 and (exp is None or (exp.dtype == self.torch.int32 and exp.shape == m.shape)), (m.dtype, m.shape)
        shape, count, N = tuple(m.shape), m.numel(), key.N
        d = self.torch.empty(shape + (2 * l, 2, N), dtype=self.torch.float64, device=self.device) if dft else None
        t = self.empty(*(shape + (2 * l, 2, N))) if torus else None
        _check(lib().mosfhet_hip_trgsw_encrypt_batch(self.h, key.h, _ptr(d) if dft and count else None, _ptr(t) if torus and count else None, _ptr(m) if count else None,
                                                     _ptr(exp) if exp is not None and count else None, int(l), int(Bg_bit), C.c_double(sigma), int(count), self._stream()))
        return (d, t) if dft and torus else (d if dft else t)

    def tlwe_phase(self, key, ct, msg_bits=0, out=None):
        """Phases b - sum a_i s_i of the TLWE samples ct [count][n + 1], exact: [count] words; msg_bits in 1 .. 63: the messages of that many bits nearest to them,
        (phase + 2^(63 - msg_bits)) >> (64 - msg_bits)."""
        count = ct.shape[0]
        assert tuple(ct.shape) == (count, key.n + 1), tuple(ct.shape)
        if out is None:
            out = self.empty(count)
        assert tuple(out.shape) == (count,), tuple(out.shape)
        _check(lib().mosfhet_hip_tlwe_phase_batch(self.h, key.h, _ptr(out) if count else None, _ptr(ct) if count else None, int(msg_bits), int(count), self._stream()))
        return out

    def trlwe_phase(self, key, ct, msg_bits=0, out=None):
        """Phases b - a * s of the TRLWE samples ct [count][2][N], exact (no transform): [count][N] words; msg_bits as for tlwe_phase."""
        count = ct.shape[0]
        assert tuple(ct.shape) == (count, 2, key.N), tuple(ct.shape)
        if out is None:
            out = self.empty(count, key.N)
        assert tuple(out.shape) == (count, key.N), tuple(out.shape)
        _check(lib().mosfhet_hip_trlwe_phase_batch(self.h, key.h, _ptr(out) if count else None, _ptr(ct) if count else None, int(msg_bits), int(count), self._stream()))
        return out

    def leveled_lut_packed_plan(self, N, l, size, tables, pack_log, count):
        """leveled_lut_packed_plan() at this device's CU count."""
        return leveled_lut_packed_plan(N, l, size, tables, pack_log, count, self.torch.cuda.get_device_properties(self.device).multi_processor_count)

    def leveled_lut_tables_plan(self, N, l, size, tables, count):
        """leveled_lut_tables_plan() at this device's CU count."""
        return leveled_lut_tables_plan(N, l, size, tables, count, self.torch.cuda.get_device_properties(self.device).multi_processor_count)

    def leveled_lut_plan(self, N, l, size, count):
        """leveled_lut_plan() at this device's CU count."""
        return leveled_lut_plan(N, l, size, count, self.torch.cuda.get_device_properties(self.device).multi_processor_count)

    def trlwe_eval_automorphism(self, gak, ct, gen, out=None):
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, 2, gak.N)
        _check(lib().mosfhet_hip_trlwe_eval_automorphism_batch(self.h, gak.h, _ptr(out), _ptr(ct), int(gen), count, self._stream()))
        return out

    def functional_bootstrap_ga(self, bsk, gak, tv, ct, torus_base, extract=True, out=None):
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, bsk.N + 1) if extract else self.empty(count, 2, bsk.N)
        _check(lib().mosfhet_hip_functional_bootstrap_ga_batch(self.h, bsk.h, gak.h, _ptr(out), _ptr(tv), self._tv(tv, bsk, count),
                                                               _ptr(ct), count, torus_base, int(extract), self._stream()))
        return out

    # ---- bootstraps ----
    def _tv(self, tv, bsk, count):
        assert tv.dim() == 3 and tv.shape[1] == bsk.k + 1 and tv.shape[2] == bsk.N, tv.shape
        assert tv.shape[0] in (1, count)
        return tv.shape[0]

    def programmable_bootstrap(self, bsk, tv, ct, precision, kappa=0, theta=0, out=None):
        count = ct.shape[0]
        assert ct.shape[1] == bsk.n + 1
        if out is None:
            out = self.empty(count, bsk.k * bsk.N + 1)
        _check(lib().mosfhet_hip_programmable_bootstrap_batch(self.h, bsk.h, _ptr(out), _ptr(tv), self._tv(tv, bsk, count),
                                                              _ptr(ct), count, precision, kappa, theta, self._stream()))
        return out

    def functional_bootstrap(self, bsk, tv, ct, torus_base, out=None):
        count = ct.shape[0]
        assert ct.shape[1] == bsk.n + 1
        if out is None:
            out = self.empty(count, bsk.k * bsk.N + 1)
        _check(lib().mosfhet_hip_functional_bootstrap_batch(self.h, bsk.h, _ptr(out), _ptr(tv), self._tv(tv, bsk, count),
                                                            _ptr(ct), count, torus_base, self._stream()))
        return out

    def functional_bootstrap_wo_extract(self, bsk, tv, ct, torus_base, out=None):
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, bsk.k + 1, bsk.N)
        _check(lib().mosfhet_hip_functional_bootstrap_wo_extract_batch(
            self.h, bsk.h, _ptr(out), _ptr(tv), self._tv(tv, bsk, count), _ptr(ct), count, torus_base, self._stream()))
        return out

    def blind_rotate_(self, bsk, acc, ct):
        """In place: acc[b] <- blind_rotate(acc[b], ct[b].a, BK)."""
        count = ct.shape[0]
        assert acc.shape == (count, bsk.k + 1, bsk.N)
        _check(lib().mosfhet_hip_blind_rotate_batch(self.h, bsk.h, _ptr(acc), _ptr(ct), count, self._stream()))
        return acc

    def external_product(self, bsk, key_index, ct, out=None):
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, bsk.k + 1, bsk.N)
        _check(lib().mosfhet_hip_external_product_batch(self.h, bsk.h, key_index, _ptr(out), _ptr(ct), count, self._stream()))
        return out

    # ---- digit-parallel radix-integer callers (capi_vec.inc): integers are digit-major [d][M][N+1] ----
    def vector_ops(self, bsk, ksk, pksk, torus_base):
        h = C.c_void_p()
        _check(lib().mosfhet_hip_vec_create(self.h, C.byref(h), bsk.h, ksk.h, pksk.h if pksk is not None else None, int(torus_base)))
        return VectorOps(self, h, bsk, torus_base)

    # ---- DFT-level objects of the legacy API (include/mosfhet.h of the reference: TRGSW_DFT, TRLWE_DFT stay on the device in slot order) ----
    def trgsw_to_dft(self, trgsw):
        """trgsw_to_DFT (src/trgsw.c:359-366) for a batch: [count][(k+1)l][k+1][N] torus words -> the same shape in doubles (N/2 complex per polynomial)"""
        shape = tuple(trgsw.shape)
        return self.torus_to_dft(trgsw.reshape(-1, shape[-1])).reshape(shape)

    def external_product_dft(self, trgsw_dft, ct, l, Bg_bit):
        """trgsw_mul_trlwe_DFT (src/trgsw.c:385-423), result left in the DFT domain.  trgsw_dft: [2l][2][N] doubles (one TRGSW for the batch)
        or [count][2l][2][N] (one per unit); ct: [count][2][N]"""
        count, two, N = ct.shape
        per_unit = trgsw_dft.dim() == 4
        assert (trgsw_dft.shape[0] == count) if per_unit else True
        out = self.torch.empty(count, 2, N, dtype=self.torch.float64, device=self.device)
        stride = C.c_size_t(2 * l * 2 * N if per_unit else 0)
        _check(lib().mosfhet_hip_external_product_dft_batch(self.h, _ptr(trgsw_dft), stride, _ptr(out), _ptr(ct), N, l, Bg_bit, count, self._stream()))
        return out

    def bootstrap_key_view(self, trgsw_dft, k, l, Bg_bit):
        """non-owning key handle over n TRGSW_DFT entries already on the device ([n][(k+1)l][k+1][N] doubles): blind_rotate(tv, a, TRGSW_DFT *s, size)"""
        n, N = trgsw_dft.shape[0], trgsw_dft.shape[-1]
        h = C.c_void_p()
        _check(lib().mosfhet_hip_bsk_view_create(self.h, C.byref(h), _ptr(trgsw_dft), n, k, N, l, Bg_bit))
        key = BootstrapKey(self, h, n, k, N, l, Bg_bit)
        key._keep = trgsw_dft     # the view borrows the tensor's memory
        return key

    def public_mux_dft(self, p0, p1, sel_dft, Bg_bit, out=None):
        """public_mux (src/bootstrap.c:369-389) with the selector rows already in the DFT domain: sel_dft [count][l][2][N] doubles"""
        count, l, two, N = sel_dft.shape
        if out is None:
            out = self.empty(count, 2, N)
        _check(lib().mosfhet_hip_public_mux_dft_batch(self.h, _ptr(out), _ptr(p0), _ptr(p1), _ptr(sel_dft), N, l, Bg_bit, count, self._stream()))
        return out

    def blind_rotate_ga(self, bsk, gak, acc, ct):
        """blind_rotate_ga (src/bootstrap_ga.c:35-60) in place on acc [count][2][N]"""
        _check(lib().mosfhet_hip_blind_rotate_ga_batch(self.h, bsk.h, gak.h, _ptr(acc), _ptr(ct), ct.shape[0], self._stream()))
        return acc

    def trlwe_eval_automorphism_entry(self, gak, entry, ct, gen, out=None):
        """trlwe_eval_automorphism (src/trlwe.c:775-781) with the key-set entry the caller names"""
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, 2, gak.N)
        _check(lib().mosfhet_hip_trlwe_eval_automorphism_entry_batch(self.h, gak.h, int(entry), _ptr(out), _ptr(ct), int(gen), count, self._stream()))
        return out

    # ---- polynomial level ----
    def torus_to_dft(self, polys):
        count, N = polys.shape
        out = self.torch.empty(count, N, dtype=self.torch.float64, device=self.device)
        _check(lib().mosfhet_hip_torus_to_dft_batch(self.h, _ptr(out), _ptr(polys), N, count, self._stream()))
        return out

    def dft_to_torus(self, dfts):
        count, N = dfts.shape
        out = self.empty(count, N)
        _check(lib().mosfhet_hip_dft_to_torus_batch(self.h, _ptr(out), _ptr(dfts), N, count, self._stream()))
        return out

    def dft_lincomb(self, a, b, cb, out=None):
        """out = a + cb * b elementwise over DFT-domain doubles (a may be None: cb * b) -- trgsw_DFT_add / _sub and their kin (src/trgsw.c, src/polynomial.c:102-128)"""
        assert a is None or a.shape == b.shape
        if out is None:
            out = self.torch.empty_like(b)
        _check(lib().mosfhet_hip_dft_lincomb_batch(self.h, _ptr(out), None if a is None else _ptr(a), _ptr(b), C.c_double(cb), C.c_size_t(b.numel()),
                                                   self._stream()))
        return out

    def dft_mul(self, a, b, out=None, addto=False):
        count, N = a.shape
        if out is None:
            assert not addto
            out = self.torch.empty_like(a)
        _check(lib().mosfhet_hip_dft_mul_batch(self.h, _ptr(out), _ptr(a), _ptr(b), N, count, int(addto), self._stream()))
        return out

    # ---- cleartext-weight linear layers (include/mosfhet_hip.h: mosfhet_hip_linear_*, mosfhet_hip_tlwe_linear_batch) ----
    @staticmethod
    def _bias(bias, shape):
        """(the array to keep alive, its pointer) of a bias of `shape`: (rows_out,) torus words, or (rows_out, N) for the layers on packed samples"""
        if bias is None:
            return None, None
        b = np.ascontiguousarray(np.asarray(bias).astype(np.uint64, copy=False))
        assert b.shape == tuple(shape), "bias: one %s per output row" % ("torus word" if len(shape) == 1 else "polynomial of N torus words")
        return b, b.ctypes.data_as(C.c_void_p)

    @staticmethod
    def _csr(row_ptr, col, n_entries):
        """(row_ptr, col, rows_out) of a sparse creator: the lists as contiguous int32, one column per entry and no fewer entries than row_ptr names"""
        row_ptr, col = np.ascontiguousarray(row_ptr, dtype=np.int32), np.ascontiguousarray(col, dtype=np.int32)
        rows_out = len(row_ptr) - 1
        assert len(col) == n_entries and (rows_out < 0 or len(col) >= row_ptr[-1])
        return row_ptr, col, rows_out

    def _clone(self, symbol, cls, lin):
        h = C.c_void_p()
        _check(getattr(lib(), symbol)(self.h, lin.h, C.byref(h)))
        return cls(self, h)

    def linear_dense(self, W, bias=None):
        """Handle of a dense layer: W [rows_out][rows_in] int64 (the multipliers tlwe_scale takes), bias [rows_out] torus words or None."""
        W = np.ascontiguousarray(W, dtype=np.int64)
        assert W.ndim == 2
        keep, pb = self._bias(bias, (W.shape[0],))
        h = C.c_void_p()
        _check(lib().mosfhet_hip_linear_create_dense(self.h, C.byref(h), W.ctypes.data_as(C.c_void_p), pb, int(W.shape[0]), int(W.shape[1])))
        return LinearMap(self, h)

    def linear_sparse(self, row_ptr, col, val, rows_in, bias=None):
        """Handle of a sparse map in CSR: row_ptr [rows_out + 1], col / val [nnz] (columns may be unsorted or repeat within a row; rows may be empty)."""
        val = np.ascontiguousarray(val, dtype=np.int64)
        row_ptr, col, rows_out = self._csr(row_ptr, col, len(val))
        keep, pb = self._bias(bias, (rows_out,))
        h = C.c_void_p()
        _check(lib().mosfhet_hip_linear_create_sparse(self.h, C.byref(h), row_ptr.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p),
                                                      val.ctypes.data_as(C.c_void_p), pb, int(rows_out), int(rows_in)))
        return LinearMap(self, h)

    def clone_linear(self, lin):
        """A copy of a LinearMap of another engine for this one (mosfhet_hip_linear_clone)."""
        return self._clone("mosfhet_hip_linear_clone", LinearMap, lin)

    def tlwe_linear(self, lin, ct, out=None):
        """out[b][j] = (0, bias[j]) + sum_i W[j][i] ct[b][i]: ct [count][rows_in][n + 1] -> [count][rows_out][n + 1], exact mod 2^64."""
        count, rows_in, row = ct.shape
        if out is None:
            out = self.empty(count, lin.rows_out, row)
        _check(lib().mosfhet_hip_tlwe_linear_batch(self.h, lin.h, _ptr(out), _ptr(ct), row - 1, count, self._stream()))
        return out

    def linear_keyswitch_functional_bootstrap(self, lin, ksk, bsk, tv, ct, torus_base, extract=True, out=None):
        """tlwe_linear, then keyswitch_functional_bootstrap on the count * rows_out results, in one call: ct [count][rows_in][kN + 1] -> [count][rows_out][kN + 1]
        (extract) or [count][rows_out][k + 1][N]; tv one test vector or one per result."""
        count, samples = ct.shape[0], ct.shape[0] * lin.rows_out
        if out is None:
            out = self.empty(count, lin.rows_out, bsk.k * bsk.N + 1) if extract else self.empty(count, lin.rows_out, bsk.k + 1, bsk.N)
        _check(lib().mosfhet_hip_linear_keyswitch_functional_bootstrap_batch(self.h, lin.h, ksk.h, bsk.h, _ptr(out), _ptr(tv), self._tv(tv, bsk, samples), _ptr(ct), count,
                                                                             torus_base, int(extract), self._stream()))
        return out

    # ---- cleartext polynomial-weight linear layers on packed TRLWE samples (include/mosfhet_hip.h: mosfhet_hip_polylinear_*, mosfhet_hip_trlwe_linear_batch) ----
    def polylinear_create_dense(self, W, bias=None):
        """Handle of a dense layer: W [rows_out][rows_in][N] int64 coefficients of the cleartext weight polynomials, bias [rows_out][N] torus words or None."""
        W = np.ascontiguousarray(W, dtype=np.int64)
        assert W.ndim == 3
        keep, pb = self._bias(bias, (W.shape[0], W.shape[2]))
        h = C.c_void_p()
        _check(lib().mosfhet_hip_polylinear_create_dense(self.h, C.byref(h), W.ctypes.data_as(C.c_void_p), pb, int(W.shape[0]), int(W.shape[1]), int(W.shape[2])))
        return PolyLinearMap(self, h)

    def polylinear_create_sparse(self, row_ptr, col, val, rows_in, N, bias=None):
        """Handle of a sparse map in CSR over polynomial blocks: row_ptr [rows_out + 1], col [nnz], val [nnz][N] (columns may be unsorted or repeat within a row --
        they add in the stored order; rows may be empty)."""
        val = np.ascontiguousarray(val, dtype=np.int64).reshape(-1, int(N))
        row_ptr, col, rows_out = self._csr(row_ptr, col, len(val))
        keep, pb = self._bias(bias, (rows_out, int(N)))
        h = C.c_void_p()
        _check(lib().mosfhet_hip_polylinear_create_sparse(self.h, C.byref(h), row_ptr.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p),
                                                          val.ctypes.data_as(C.c_void_p), pb, int(rows_out), int(rows_in), int(N)))
        return PolyLinearMap(self, h)

    def clone_polylinear(self, lin):
        """A copy of a PolyLinearMap of another engine for this one (mosfhet_hip_polylinear_clone)."""
        return self._clone("mosfhet_hip_polylinear_clone", PolyLinearMap, lin)

    def trlwe_linear(self, lin, ct, out=None):
        """out[b][j] = (0, bias[j]) + sum_e ct[b][col_e] * val_e, negacyclic products through the transform in the stored order: ct [count][rows_in][2][N] ->
        [count][rows_out][2][N]."""
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, lin.rows_out, 2, lin.N)
        _check(lib().mosfhet_hip_trlwe_linear_batch(self.h, lin.h, _ptr(out) if count else None, _ptr(ct) if count else None, count, self._stream()))
        return out

    def trlwe_linear_extract(self, lin, ct, idx=0, out=None):
        """trlwe_linear followed by trlwe_extract_tlwe(., idx), the TRLWE result never written: ct [count][rows_in][2][N] -> [count][rows_out][N + 1]."""
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, lin.rows_out, lin.N + 1)
        _check(lib().mosfhet_hip_trlwe_linear_extract_batch(self.h, lin.h, _ptr(out) if count else None, _ptr(ct) if count else None, int(idx), count, self._stream()))
        return out

    def trlwe_linear_keyswitch_functional_bootstrap(self, lin, ksk, bsk, tv, ct, torus_base, idx=0, extract=True, out=None):
        """trlwe_linear_extract, then keyswitch_functional_bootstrap on the count * rows_out results, in one call: ct [count][rows_in][2][N] -> [count][rows_out][N + 1]
        (extract) or [count][rows_out][2][N]; tv one test vector or one per result."""
        count, samples = ct.shape[0], ct.shape[0] * lin.rows_out
        if out is None:
            out = self.empty(count, lin.rows_out, bsk.k * bsk.N + 1) if extract else self.empty(count, lin.rows_out, bsk.k + 1, bsk.N)
        _check(lib().mosfhet_hip_trlwe_linear_keyswitch_functional_bootstrap_batch(self.h, lin.h, ksk.h, bsk.h, _ptr(out), _ptr(tv), self._tv(tv, bsk, samples), _ptr(ct),
                                                                                   int(idx), count, torus_base, int(extract), self._stream()))
        return out

    # ---- encrypted polynomial-weight linear layers on packed TRLWE samples (include/mosfhet_hip.h: mosfhet_hip_gswlinear_*, mosfhet_hip_trlwe_gsw_linear_batch) ----
    def gswlinear_create_dense(self, W, Bg_bit, bias=None):
        """Handle of a dense layer: W [rows_out][rows_in][2l][2][N] torus words (TRGSW samples), bias [rows_out][N] torus words or None."""
        W = np.ascontiguousarray(np.asarray(W).astype(np.uint64, copy=False))
        assert W.ndim == 5 and W.shape[3] == 2 and W.shape[2] % 2 == 0
        keep, pb = self._bias(bias, (W.shape[0], W.shape[4]))
        h = C.c_void_p()
        _check(lib().mosfhet_hip_gswlinear_create_dense(self.h, C.byref(h), W.ctypes.data_as(C.c_void_p), pb, int(W.shape[0]), int(W.shape[1]), int(W.shape[4]),
                                                        int(W.shape[2] // 2), int(Bg_bit)))
        return GswLinearMap(self, h)

    def gswlinear_create_sparse(self, row_ptr, col, W, rows_in, N, l, Bg_bit, bias=None):
        """Handle of a sparse map in CSR over TRGSW blocks: row_ptr [rows_out + 1], col [nnz], W [nnz][2l][2][N] torus words (columns may be unsorted or repeat
        within a row -- they add in the stored order; rows may be empty)."""
        W = np.ascontiguousarray(np.asarray(W).astype(np.uint64, copy=False)).reshape(-1, 2 * int(l), 2, int(N))
        row_ptr, col, rows_out = self._csr(row_ptr, col, len(W))
        keep, pb = self._bias(bias, (rows_out, int(N)))
        h = C.c_void_p()
        _check(lib().mosfhet_hip_gswlinear_create_sparse(self.h, C.byref(h), row_ptr.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p),
                                                         W.ctypes.data_as(C.c_void_p), pb, int(rows_out), int(rows_in), int(N), int(l), int(Bg_bit)))
        return GswLinearMap(self, h)

    def gswlinear_create_from_selectors(self, sel_dft, row_ptr, col, rows_in, Bg_bit, bias=None):
        """The same map over weights already on the device: sel_dft [nnz][2l][2][N] float64 (TRGSW_DFT samples in the engine's slot order, as trgsw_from_gadget,
        circuit_bootstrap_3_dft or torus_to_dft wrote them), copied into the handle."""
        nnz, rows, two, N = sel_dft.shape
        assert two == 2 and rows % 2 == 0 and sel_dft.dtype == self.torch.float64 and sel_dft.is_contiguous()
        row_ptr, col, rows_out = self._csr(row_ptr, col, nnz)
        keep, pb = self._bias(bias, (rows_out, int(N)))
        h = C.c_void_p()
        _check(lib().mosfhet_hip_gswlinear_create_from_selectors(self.h, C.byref(h), _ptr(sel_dft) if nnz else None, row_ptr.ctypes.data_as(C.c_void_p),
                                                                 col.ctypes.data_as(C.c_void_p), pb, int(rows_out), int(rows_in), int(N), int(rows // 2), int(Bg_bit)))
        return GswLinearMap(self, h)

    def clone_gswlinear(self, lin):
        """A copy of a GswLinearMap of another engine for this one (mosfhet_hip_gswlinear_clone)."""
        return self._clone("mosfhet_hip_gswlinear_clone", GswLinearMap, lin)

    def trlwe_gsw_linear(self, lin, ct, out=None):
        """out[b][j] = (0, bias[j]) + sum_e W_e x ct[b][col_e], external products summed in the DFT domain in the stored order and rounded once: ct
        [count][rows_in][2][N] -> [count][rows_out][2][N]."""
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, lin.rows_out, 2, lin.N)
        _check(lib().mosfhet_hip_trlwe_gsw_linear_batch(self.h, lin.h, _ptr(out) if count else None, _ptr(ct) if count else None, count, self._stream()))
        return out

    def trlwe_gsw_linear_extract(self, lin, ct, idx=0, out=None):
        """trlwe_gsw_linear followed by trlwe_extract_tlwe(., idx), the TRLWE result never written: ct [count][rows_in][2][N] -> [count][rows_out][N + 1]."""
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, lin.rows_out, lin.N + 1)
        _check(lib().mosfhet_hip_trlwe_gsw_linear_extract_batch(self.h, lin.h, _ptr(out) if count else None, _ptr(ct) if count else None, int(idx), count,
                                                                self._stream()))
        return out

    # ---- LWE batches packed into TRLWE samples (include/mosfhet_hip.h: mosfhet_hip_tlwe_pack_batch) ----
    def tlwe_pack(self, pk, ct, per=None, split=1, out=None):
        """trlwe_full_packing_keyswitch over a batch: ct [total][n_in + 1] -> [ceil(total / per)][2][N]; pk an FFT key-switch key set of n_in entries
        (load_trlwe_ks_keys / generate_trlwe_ks_keys), per samples per output (default N), sample j of an output at coefficient j.  split = 1: the reference's
        words; split = P: P teams per output (tlwe_pack_plan recommends one)."""
        total = ct.shape[0]
        per = pk.N if per is None else int(per)
        if out is None:
            out = self.empty(-(-total // per) if per >= 1 else 0, 2, pk.N)
        _check(lib().mosfhet_hip_tlwe_pack_batch(self.h, pk.h, _ptr(out) if total else None, _ptr(ct) if total else None, int(total), per, int(split), self._stream()))
        return out

    # ---- the trace switch and the gadget -> TRGSW conversion (include/mosfhet_hip.h: mosfhet_hip_tlwe_trace_pack_batch) ----
    def tlwe_trace_pack(self, tks, ct, entry0=0, out=None):
        """trlwe_packing1_keyswitch_CDKS21 over a batch: ct [count][N + 1] under the extracted ring key -> [count][2][N], phase N m at coefficient 0; tks holds the
        log2 N trace keys from entry0 on (entry j switches from s(X^(N / 2^j + 1)))."""
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, 2, tks.N)
        _check(lib().mosfhet_hip_tlwe_trace_pack_batch(self.h, tks.h, int(entry0), _ptr(out) if count else None, _ptr(ct) if count else None, count, self._stream()))
        return out

    def tlwe_trace_pack_many(self, tks, ct, log_per, entry0=0, out=None):
        """2^log_per samples per output by the trace: ct [total][N + 1] under the extracted ring key -> [ceil(total / 2^log_per)][2][N], sample j of an output with
        phase N m_j at coefficient j N / 2^log_per; the same log2 N trace keys as tlwe_trace_pack, whose words log_per = 0 gives."""
        total, log_per = ct.shape[0], int(log_per)
        if out is None:
            out = self.empty(-(-total // (1 << log_per)) if 0 <= log_per < 31 else 0, 2, tks.N)
        _check(lib().mosfhet_hip_tlwe_trace_pack_many_batch(self.h, tks.h, int(entry0), _ptr(out) if total else None, _ptr(ct) if total else None, int(total), log_per,
                                                            self._stream()))
        return out

    def trlwe_rlwe_priv_keyswitch(self, tks, ct, entry0=0, out=None):
        """trlwe_RLWE_priv_keyswitch over a batch: ct [count][2][N] -> TRLWE(m v), entries entry0 (from s_in v) and entry0 + 1 (from v); out may be ct."""
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, 2, tks.N)
        _check(lib().mosfhet_hip_trlwe_rlwe_priv_keyswitch_batch(self.h, tks.h, int(entry0), _ptr(out) if count else None, _ptr(ct) if count else None, count, self._stream()))
        return out

    def trgsw_from_gadget(self, tks, gadget, entry0=0, out=None):
        """trgsw_from_gadget over a batch: gadget [count][l][2][N] -> selectors [count][2l][2][N] float64 (DFT domain, the engine's slot order: the d_sel_dft of the
        leveled-LUT calls); tks holds the gadget key (v = -s) at entry0, entry0 + 1."""
        count, l, two, N = gadget.shape
        assert two == 2
        if out is None:
            out = self.torch.empty(count, 2 * l, 2, N, dtype=self.torch.float64, device=self.device)
        _check(lib().mosfhet_hip_trgsw_from_gadget_batch(self.h, tks.h, int(entry0), _ptr(out) if count else None, _ptr(gadget) if count else None, int(l), count, self._stream()))
        return out

    # ---- packed TRLWE samples opened into LWE batches (include/mosfhet_hip.h: mosfhet_hip_trlwe_unpack_batch) ----
    def _unpack_shape(self, trlwe, total, per, ksk=None):
        outputs, two, N = trlwe.shape
        assert two == 2
        if ksk is not None and ksk.n_in != N:   # (the C call takes N from the key: it cannot see the tensor's)
            raise MosfhetHipError("trlwe_unpack_keyswitch: the key switches from n_in = %d words, the packed samples have N = %d" % (ksk.n_in, N))
        per = N if per is None else int(per)
        total = outputs * per if total is None else int(total)
        assert total <= outputs * per, "total = %d: %d packed samples of %d hold %d" % (total, outputs, per, outputs * per)
        return N, total, per

    def trlwe_unpack(self, trlwe, total=None, per=None, out=None):
        """trlwe_extract_tlwe over a batch, the inverse layout of tlwe_pack: trlwe [outputs][2][N] -> [total][N + 1], sample o per + j = extract(trlwe[o], j); per
        defaults to N, total to outputs * per."""
        N, total, per = self._unpack_shape(trlwe, total, per)
        if out is None:
            out = self.empty(max(total, 0), N + 1)
        _check(lib().mosfhet_hip_trlwe_unpack_batch(self.h, _ptr(out) if total else None, _ptr(trlwe) if total else None, N, total, per, self._stream()))
        return out

    def trlwe_unpack_keyswitch(self, ksk, trlwe, total, per, out=None):
        """tlwe_keyswitch of trlwe_unpack's samples without writing them: trlwe [outputs][2][N] -> [total][n_out + 1]; ksk an LWE -> LWE key with n_in == N."""
        N, total, per = self._unpack_shape(trlwe, total, per, ksk)
        if out is None:
            out = self.empty(max(total, 0), ksk.n_out + 1)
        _check(lib().mosfhet_hip_trlwe_unpack_keyswitch_batch(self.h, ksk.h, _ptr(out) if total else None, _ptr(trlwe) if total else None, total, per, self._stream()))
        return out

    def unpack_keyswitch_functional_bootstrap(self, ksk, bsk, tv, trlwe, total, per, torus_base, extract=True, out=None):
        """trlwe_unpack_keyswitch followed by functional_bootstrap[_wo_extract] in one call: trlwe [outputs][2][N] -> [total][N + 1] (extract) or [total][2][N]; tv one
        test vector or one per sample."""
        N, total, per = self._unpack_shape(trlwe, total, per, ksk)
        if out is None:
            out = self.empty(max(total, 0), bsk.N + 1) if extract else self.empty(max(total, 0), 2, bsk.N)
        _check(lib().mosfhet_hip_unpack_keyswitch_functional_bootstrap_batch(self.h, ksk.h, bsk.h, _ptr(out) if total else None, _ptr(tv), self._tv(tv, bsk, total),
                                                                             _ptr(trlwe) if total else None, total, per, torus_base, int(extract), self._stream()))
        return out

    # ---- ... at an offset and a stride: sample j of an input is the coefficient first + j stride (mosfhet_hip_trlwe_unpack_strided_batch) ----
    def _unpack_strided_shape(self, trlwe, total, per, ksk=None):
        outputs, two, N = trlwe.shape
        assert two == 2
        if ksk is not None and ksk.n_in != N:   # (the C call takes N from the key: it cannot see the tensor's)
            raise MosfhetHipError("trlwe_unpack_strided_keyswitch: the key switches from n_in = %d words, the packed samples have N = %d" % (ksk.n_in, N))
        per = int(per)
        total = outputs * per if total is None else int(total)
        assert total <= outputs * max(per, 0), "total = %d: %d packed samples of %d hold %d" % (total, outputs, per, outputs * per)
        return N, total, per

    def trlwe_unpack_strided(self, trlwe, total, per, first, stride, out=None):
        """trlwe_extract_tlwe at the coefficients first + j stride, j < per, of every input: trlwe [outputs][2][N] -> [total][N + 1], sample o per + j =
        extract(trlwe[o], first + j stride); first + (per - 1) stride <= N - 1.  total = None: outputs * per."""
        N, total, per = self._unpack_strided_shape(trlwe, total, per)
        if out is None:
            out = self.empty(max(total, 0), N + 1)
        _check(lib().mosfhet_hip_trlwe_unpack_strided_batch(self.h, _ptr(out) if total else None, _ptr(trlwe) if total else None, N, total, per, _c_int(first),
                                                            _c_int(stride), self._stream()))
        return out

    def trlwe_unpack_strided_keyswitch(self, ksk, trlwe, total, per, first, stride, out=None):
        """tlwe_keyswitch of trlwe_unpack_strided's samples without writing them: trlwe [outputs][2][N] -> [total][n_out + 1]; ksk an LWE -> LWE key with n_in == N."""
        N, total, per = self._unpack_strided_shape(trlwe, total, per, ksk)
        if out is None:
            out = self.empty(max(total, 0), ksk.n_out + 1)
        _check(lib().mosfhet_hip_trlwe_unpack_strided_keyswitch_batch(self.h, ksk.h, _ptr(out) if total else None, _ptr(trlwe) if total else None, total, per,
                                                                      _c_int(first), _c_int(stride), self._stream()))
        return out

    def unpack_strided_keyswitch_functional_bootstrap(self, ksk, bsk, tv, trlwe, total, per, first, stride, torus_base, extract=True, out=None):
        """trlwe_unpack_strided_keyswitch followed by functional_bootstrap[_wo_extract] in one call: trlwe [outputs][2][N] -> [total][N + 1] (extract) or [total][2][N];
        tv one test vector or one per sample."""
        N, total, per = self._unpack_strided_shape(trlwe, total, per, ksk)
        if out is None:
            out = self.empty(max(total, 0), bsk.N + 1) if extract else self.empty(max(total, 0), 2, bsk.N)
        _check(lib().mosfhet_hip_unpack_strided_keyswitch_functional_bootstrap_batch(self.h, ksk.h, bsk.h, _ptr(out) if total else None, _ptr(tv),
                                                                                     self._tv(tv, bsk, total), _ptr(trlwe) if total else None, total, per, _c_int(first),
                                                                                     _c_int(stride), torus_base, int(extract), self._stream()))
        return out

    def trlwe_linear_unpack_keyswitch_functional_bootstrap(self, lin, ksk, bsk, tv, ct, per, first, stride, torus_base, extract=True, out=None):
        """trlwe_linear, then unpack_strided_keyswitch_functional_bootstrap on its count * rows_out results, per samples of each, in one call: ct
        [count][rows_in][2][N] -> [count * rows_out * per][N + 1] (extract) or [count * rows_out * per][2][N]; tv one test vector or one per sample."""
        count, per = ct.shape[0], int(per)
        samples = count * lin.rows_out * max(per, 0)
        if out is None:
            out = self.empty(samples, bsk.N + 1) if extract else self.empty(samples, 2, bsk.N)
        _check(lib().mosfhet_hip_trlwe_linear_unpack_keyswitch_functional_bootstrap_batch(self.h, lin.h, ksk.h, bsk.h, _ptr(out), _ptr(tv), self._tv(tv, bsk, samples),
                                                                                          _ptr(ct), per, _c_int(first), _c_int(stride), count, torus_base, int(extract),
                                                                                          self._stream()))
        return out

    # ---- key switch ----
    def tlwe_keyswitch(self, ksk, ct, out=None):
        count = ct.shape[0]
        assert ct.shape[1] == ksk.n_in + 1
        if out is None:
            out = self.empty(count, ksk.n_out + 1)
        _check(lib().mosfhet_hip_tlwe_keyswitch_batch(self.h, ksk.h, _ptr(out), _ptr(ct), count, self._stream()))
        return out

    def trlwe_extract_tlwe(self, trlwe, idx, out=None):
        count, k1, N = trlwe.shape
        if out is None:
            out = self.empty(count, (k1 - 1) * N + 1)
        if k1 == 2:
            _check(lib().mosfhet_hip_trlwe_extract_tlwe_batch(self.h, _ptr(out), _ptr(trlwe), N, idx, count, self._stream()))
        else:
            _check(lib().mosfhet_hip_trlwe_extract_tlwe_k_batch(self.h, _ptr(out), _ptr(trlwe), k1 - 1, N, idx, count, self._stream()))
        return out

    def tlwe_addto_(self, out, ct):
        count, row = ct.shape
        assert out.shape == ct.shape
        _check(lib().mosfhet_hip_tlwe_addto_batch(self.h, _ptr(out), _ptr(ct), row - 1, count, self._stream()))
        return out

    def full_domain_functional_bootstrap(self, bsk, ksk, tv, ct, precision, out=None):
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, bsk.k * bsk.N + 1)
        _check(lib().mosfhet_hip_full_domain_functional_bootstrap_batch(
            self.h, bsk.h, ksk.h, _ptr(out), _ptr(tv), self._tv(tv, bsk, count), _ptr(ct), count, precision, self._stream()))
        return out

    def multivalue_bootstrap_CLOT21(self, bsk, tv, ct, torus_base, n_luts, out=None):
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, n_luts, bsk.k * bsk.N + 1)
        _check(lib().mosfhet_hip_multivalue_bootstrap_CLOT21_batch(
            self.h, bsk.h, _ptr(out), _ptr(tv), self._tv(tv, bsk, count), _ptr(ct), count, torus_base, n_luts, self._stream()))
        return out

    # ---- measurement ----
    def time_programmable_bootstrap(self, bsk, tv, ct, precision, reps, out=None):
        """Average milliseconds per kernel launch, hipEvents on the launch stream."""
        count = ct.shape[0]
        if out is None:
            out = self.empty(count, bsk.k * bsk.N + 1)
        ms = C.c_float()
        _check(lib().mosfhet_hip_time_programmable_bootstrap(self.h, bsk.h, _ptr(out), _ptr(tv), self._tv(tv, bsk, count),
                                                             _ptr(ct), count, precision, reps, self._stream(), C.byref(ms)))
        return ms.value

    def sync(self):
        self.torch.cuda.current_stream(self.device).synchronize()


def set_unfold_split_max(max_batch):
    """chunk size of the two-phase unfolded bootstrap (-1 default, 0 = always the fused kernel)"""
    _check(lib().mosfhet_hip_set_unfold_split_max(int(max_batch)))


def set_unfold2_dft(on):
    """unfolding-2 keys: DFT-domain assembly of the per-group TRGSW (default) or the torus-domain one of u = 4 and 8"""
    _check(lib().mosfhet_hip_set_unfold2_dft(int(bool(on))))


def set_team_max_batch(max_batch):
    """Batches up to this size use the latency-oriented bootstrap kernel at N = 1024 (0 disables it)."""
    _check(lib().mosfhet_hip_set_team_max_batch(int(max_batch)))


def set_pbs_group(mode):
    """SET_1's throughput bootstrap kernel with four ciphertexts per workgroup: 0 = never, 1 = from one residency round of the device on, 4 = at any batch size (same bits)."""
    _check(lib().mosfhet_hip_set_pbs_group(int(mode)))


def last_pbs_group():
    """ciphertexts per workgroup of the throughput-kernel launch of this thread's most recent bootstrap call (0: it launched none)"""
    return int(lib().mosfhet_hip_last_pbs_group())


def set_wide_team_max_batch(max_batch):
    """Batches up to this size use the latency-oriented bootstrap kernel at N = 2048 (0 disables it)."""
    _check(lib().mosfhet_hip_set_wide_team_max_batch(int(max_batch)))


def set_split_max_batch(max_batch):
    """N = 2048, l = 2, 4, 6: batches up to this size take two CUs per bootstrap (pbs_split_kernel; sums per accumulator component: FFT-level different bits). -1 = CUs / 2 (default), 0 = never."""
    _check(lib().mosfhet_hip_set_split_max_batch(int(max_batch)))


def set_ks_words(min_count):
    """Table key switches with 2 - 4 digit bits take the word-lane kernel (keyswitch_words_kernels.h) from this many ciphertexts on (default 17, 0 = never; same bits)."""
    _check(lib().mosfhet_hip_set_ks_words(int(min_count)))


def set_bycomp_parking(on):
    """0: a by-component key's large batches run the one-CU by-component kernel in residency rounds, as when the parking memory of the throughput form is refused
    (same bits, about 1.8 x the time); 1 = default"""
    _check(lib().mosfhet_hip_set_bycomp_parking(int(bool(on))))


def set_split_wait_limit(ticks):
    """bound (10 ns ticks) of the pairing wait of pbs_split_kernel; 0 = every bootstrap taken alone by one workgroup (same bits)"""
    _check(lib().mosfhet_hip_set_split_wait_limit(int(ticks)))


def split_last_launch():
    """(count, paired, alone) of this thread's last split launch"""
    c, p, a = C.c_int(), C.c_int(), C.c_int()
    _check(lib().mosfhet_hip_split_last_launch(C.byref(c), C.byref(p), C.byref(a)))
    return c.value, p.value, a.value


class VectorOps:
    """Handle of the digit-parallel integer callers (mosfhet_hip_vec_*): add / sub / ReLU / encrypted LUT over M independent radix-B integers"""
    def __init__(self, eng, h, bsk, torus_base):
        self.eng, self.h, self.bsk, self.torus_base = eng, h, bsk, torus_base

    def addsub(self, a, b, subtract=False, out=None):
        d, M, row = a.shape
        if out is None:
            out = self.eng.empty(d, M, row)
        _check(lib().mosfhet_hip_vec_addsub(self.h, _ptr(out), _ptr(a), _ptr(b), M, d, int(bool(subtract)), self.eng._stream()))
        return out

    def relu(self, a, out=None):
        d, M, row = a.shape
        if out is None:
            out = self.eng.empty(d, M, row)
        _check(lib().mosfhet_hip_vec_relu(self.h, _ptr(out), _ptr(a), M, d, self.eng._stream()))
        return out

    def encrypted_lut(self, table, sel):
        """table [size][M][N+1] is consumed; returns table[0] = the selected entries"""
        size, M, row = table.shape
        _check(lib().mosfhet_hip_vec_encrypted_lut(self.h, _ptr(table), _ptr(sel), size, M, self.eng._stream()))
        return table[0]

    def cmp(self, a, b, a_signed=True, b_signed=True):
        """[M][N+1]: digit 0 / 1 / 2 (over 2 B) for a < / = / > b"""
        d, M, row = a.shape
        out = self.eng.empty(M, row)
        _check(lib().mosfhet_hip_vec_cmp(self.h, _ptr(out), _ptr(a), _ptr(b), M, d, int(bool(a_signed)), int(bool(b_signed)), self.eng._stream()))
        return out

    def mux_array(self, tables, sel):
        """tables [size][d][M][N+1] (consumed), sel [log_B size][M][N+1] -> [d][M][N+1]"""
        size, d, M, row = tables.shape
        out = self.eng.empty(d, M, row)
        _check(lib().mosfhet_hip_vec_mux_array(self.h, _ptr(out), _ptr(tables), _ptr(sel), size, d, M, self.eng._stream()))
        return out

    def sl_add(self, a, g, b, h, out_digits, signed=True):
        da, M, row = a.shape
        out = self.eng.empty(out_digits, M, row)
        _check(lib().mosfhet_hip_vec_sl_add(self.h, _ptr(out), int(out_digits), _ptr(a), da, int(g), _ptr(b), b.shape[0], int(h), int(bool(signed)), M, self.eng._stream()))
        return out

    def extend(self, c, d_ini, signed=True):
        dc, M, _ = c.shape
        _check(lib().mosfhet_hip_vec_extend(self.h, _ptr(c), dc, int(d_ini), int(bool(signed)), M, self.eng._stream()))
        return c

    def mul(self, a, b, out_digits, signed=True):
        da, M, row = a.shape
        out = self.eng.empty(out_digits, M, row)
        _check(lib().mosfhet_hip_vec_mul(self.h, _ptr(out), int(out_digits), _ptr(a), da, _ptr(b), b.shape[0], int(bool(signed)), M, self.eng._stream()))
        return out

    def lut_cleartext(self, sel, lut, out_digits):
        """out[m] = lut[selector_m] for a cleartext table (numpy uint64 [size]); sel [levels][M][N+1] -> [out_digits][M][N+1]"""
        levels, M, row = sel.shape
        lut = np.ascontiguousarray(lut, dtype=np.uint64)
        out = self.eng.empty(out_digits, M, row)
        _check(lib().mosfhet_hip_vec_lut_cleartext(self.h, _ptr(out), _ptr(sel), lut.ctypes.data_as(C.c_void_p), int(lut.size), int(out_digits), M, self.eng._stream()))
        return out

    def free(self):
        if self.h:
            lib().mosfhet_hip_vec_destroy(self.h)
            self.h = None


def set_ep_plain_loop(on):
    """external products on two-wavefront teams (N = 2048, l = 4): the plain unit loop instead of the software-pipelined one (same bits)"""
    _check(lib().mosfhet_hip_set_ep_plain_loop(int(bool(on))))


def ep_kernel_info():
    """[(name, scratch bytes per lane of the pipelined build, launcher takes it)] of the multi-wavefront external-product instantiations launched so far"""
    out, i = [], 0
    name, scratch, takes = C.c_char_p(), C.c_int(), C.c_int()
    while lib().mosfhet_hip_ep_kernel_info(i, C.byref(name), C.byref(scratch), C.byref(takes)) == 0:
        out.append((name.value.decode(), scratch.value, bool(takes.value)))
        i += 1
    return out


def twiddles(N):
    out = np.empty(2 * (N // 2 - 1), dtype=np.float64)
    _check(lib().mosfhet_hip_twiddles(N, out.ctypes.data_as(C.c_void_p)))
    return out


def slot_order_to_oracle(dft, N):
    """Engine slot order (index m*T + thread, T = N/16 threads of 8 registers) -> oracle order (index thread*8 + m)."""
    assert N in (1024, 2048, 4096)
    M, T = N // 2, N // 16
    j = np.arange(M)
    dev = (j & 7) * T + (j >> 3)
    z = dft.reshape(-1, M, 2)
    return z[:, dev, :].reshape(dft.shape)
