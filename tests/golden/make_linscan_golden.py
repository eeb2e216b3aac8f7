#!/usr/bin/env python
"""Generates tests/golden/linscan/reference_outputs.npz: the outputs of the reference's own ADC scan build (oracle/_ref, made by
`make -C oracle ref` from the reference's source) on the seeded inputs of tests/test_linscan.py -- data only, no source.
Needs oracle/_ref; re-run only when those test cases change:

    python tests/golden/make_linscan_golden.py

Per case (key = test_linscan.case_key): KEY_dists (nq, knn) f32, KEY_idx (nq, knn) int32 1-based, and KEY_inputs, the
sha256 of the inputs (codes, Q, K, dbnorms) the outputs belong to.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import oracle as O  # noqa: E402
import test_linscan as TL  # noqa: E402


def main():
    O.build()
    if O.ref_linscan_path() is None:
        raise SystemExit("oracle/_ref not built: the reference sources are needed to make this fixture")
    out = {}
    cases = [(c, c[0] + c[2]) for c in TL.REF_CASES] + [(TL.RECALL_CASE, 9)]
    for (n, nq, d, m, knn, ties), seed in cases:
        codes, Q, K, dbnorms = TL._case(np.random.default_rng(seed), n, nq, d, m, ties)
        key = TL.case_key(n, nq, d, m, knn, ties)
        dists, idx = O.ref_linscan(codes, Q, K, dbnorms, m, TL.H, knn)
        out[key + "_dists"], out[key + "_idx"] = dists, idx
        out[key + "_inputs"] = np.array(TL.inputs_digest(codes, Q, K, dbnorms))
    path = os.path.join(HERE, "linscan", "reference_outputs.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, len(cases), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
