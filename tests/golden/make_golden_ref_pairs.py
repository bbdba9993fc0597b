#!/usr/bin/env python3
"""tests/golden/ref_iou_pairs.npz: the reference's own polyiou.cpp (oracle/_ref, compiled by oracle/Makefile where the reference
tree is present) on the seeded quad pairs of tests/test_oracle_polyiou.py::test_against_compiled_reference_if_present, so that
the test checks the C restatement against the reference's answers on every machine.  The inputs are regenerated from the seed;
`*_sum` / `*_head` pin them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import oracle  # noqa: E402
from conftest import rrects  # noqa: E402


def pairs():
    """-> [(p, q)]: rotated rectangles, then arbitrary (self-intersecting) quads; the test's own generator."""
    rng = np.random.default_rng(5)
    p = rrects(20000, rng, extent=300.0).astype(np.float64)
    q = rrects(20000, rng, extent=300.0).astype(np.float64)
    p2 = rng.normal(0, 5, (20000, 8))
    q2 = rng.normal(0, 5, (20000, 8))
    return [(p, q), (p2, q2)]


if __name__ == "__main__":
    if oracle.ref_lib() is None:
        raise SystemExit("oracle/_ref/libpolyiou_ref.so is not built (needs the reference tree)")
    fx = {}
    for i, (p, q) in enumerate(pairs()):
        fx["iou_%d" % i] = oracle.ref_iou_poly_pairs(p, q)
        fx["p_sum_%d" % i], fx["q_sum_%d" % i] = p.sum(0), q.sum(0)
        fx["p_head_%d" % i], fx["q_head_%d" % i] = p[:4], q[:4]
    np.savez_compressed(os.path.join(HERE, "ref_iou_pairs.npz"), **fx)
    print("wrote ref_iou_pairs.npz")
