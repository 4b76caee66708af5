"""The encrypted memory of include/mosfhet_hip.h (mosfhet_hip_trlwe_ram_read_batch / mosfhet_hip_trlwe_ram_write_batch) restated on the CPU from
oracle.external_product and word arithmetic mod 2^64 alone.  A memory is [cells][2][N] uint64 with cells = 2^size; sel_dft is [size][2l][2][N] doubles in the oracle's
order (oracle.bk_to_dft of the selector words), selector j encrypting bit j of the address, least significant first.
"""
import numpy as np


def cmux(oracle, sel_dft, c0, c1, l, Bg):
    """c0 + sel (.) (c1 - c0): c1 where sel encrypts 1, c0 where it encrypts 0"""
    return c0 + oracle.external_product(np.ascontiguousarray(c1 - c0), sel_dft, l, Bg)


def read(oracle, mem, sel_dft, l, Bg):
    """the CMUX tree over the cells, top address bit first; mem is left as it was"""
    size = sel_dft.shape[0]
    assert mem.shape[0] == 1 << size
    T = mem.copy()
    for t in range(size):
        half = 1 << (size - 1 - t)
        for j in range(half):
            T[j] = T[j] + oracle.external_product(np.ascontiguousarray(T[j + half] - T[j]), sel_dft[size - 1 - t], l, Bg)
    return T[0]


def write_cell(oracle, cell, val, sel_dft, i, l, Bg):
    """the CMUX form, which the tests pin: bit j of i set: v = cell + sel[j] (.) (v - cell); else v = v + sel[j] (.) (cell - v)"""
    v = val.copy()
    for j in range(sel_dft.shape[0]):
        if (i >> j) & 1:
            v = cell + oracle.external_product(np.ascontiguousarray(v - cell), sel_dft[j], l, Bg)
        else:
            v = v + oracle.external_product(np.ascontiguousarray(cell - v), sel_dft[j], l, Bg)
    return v


def write_cell_e(oracle, cell, val, sel_dft, i, l, Bg):
    """the form with one buffer, e = v - cell: bit 1: e = sel (.) e; bit 0: e = e + sel (.) (-e); then cell + e"""
    e = val - cell
    for j in range(sel_dft.shape[0]):
        if (i >> j) & 1:
            e = oracle.external_product(np.ascontiguousarray(e), sel_dft[j], l, Bg)
        else:
            e = e + oracle.external_product(np.ascontiguousarray(np.uint64(0) - e), sel_dft[j], l, Bg)
    return cell + e


def write(oracle, mem, val, sel_dft, l, Bg, cell_fn=write_cell):
    """the memory after a write of val at the address of sel_dft: every cell on its own"""
    return np.stack([cell_fn(oracle, mem[i], val, sel_dft, i, l, Bg) for i in range(mem.shape[0])])
