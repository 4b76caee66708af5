#!/usr/bin/env python3
"""Generates tests/golden/reference_prototypes.npz: for every function the REAL reference's include/mosfhet.h declares, its name and a digest of its
prototype (return type and argument types, parameter names and spacing removed: tests/test_host_and_abi.py's _prototypes) -- data only, no declaration
text.  tests/test_host_and_abi.py::test_header_matches_the_reference_prototypes holds include/mosfhet.h to it.  Run where the reference tree is present:
    python tests/golden/make_prototypes_golden.py <the reference's include/mosfhet.h>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from test_host_and_abi import _prototypes, prototype_digest  # noqa: E402


def main():
    protos = _prototypes(sys.argv[1])
    names = sorted(protos)
    np.savez_compressed(os.path.join(HERE, "reference_prototypes.npz"), names=np.array(names), digests=np.array([prototype_digest(protos[n]) for n in names]))
    print("%d prototypes" % len(names))


if __name__ == "__main__":
    main()
