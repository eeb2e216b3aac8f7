#!/usr/bin/env python
"""Generates tests/golden/linscan_pq/reference_outputs.npz: the outputs of the reference's own PQ / OPQ scan (linscan_aqd_query,
src/linscan/cpp/linscan_aqd.cpp) on the seeded inputs of tests/test_linscan_pq.py -- data only, no source.  The reference checkout is named by
$REFERENCE; its source is compiled in place with the flags of its src/linscan/cpp/compile.sh into a temporary directory that is deleted
afterwards.  Re-run only when those test cases change:

    REFERENCE=/path/to/local-search-quantization python tests/golden/make_linscan_pq_golden.py

Per case (key = the case's name in test_linscan_pq.FIXTURE_CASES): KEY_dists (nq, K) f32, KEY_res (nq, K) uint32 0-based, and KEY_inputs,
the sha256 of the inputs (codes, centers, queries) the outputs belong to.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_linscan_pq as TP  # noqa: E402


def main():
    ref = os.environ.get("REFERENCE")
    src = os.path.join(ref or "", "src", "linscan", "cpp", "linscan_aqd.cpp")
    if not ref or not os.path.isfile(src):
        raise SystemExit("set REFERENCE to a checkout of the reference: %s not found" % src)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "linscan_aqd.so")
        subprocess.check_call(["g++", "-shared", "-O3", "-fPIC", src, "-o", so, "-fopenmp"])
        lib = C.CDLL(so)
        lib.linscan_aqd_query.restype = None
        lib.linscan_aqd_query.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        for name, (n, nq, m, subdim, dc, dq, K, kind) in sorted(TP.FIXTURE_CASES.items()):
            codes, centers, Q = TP.fixture_inputs(name)
            dists = np.zeros((nq, K), np.float32)
            res = np.zeros((nq, K), np.uint32)
            lib.linscan_aqd_query(dists.ctypes.data, res.ctypes.data, codes.ctypes.data, centers.ctypes.data, Q.ctypes.data, n, nq, 8 * m, K, dc, dq,
                                  subdim)
            out[name + "_dists"], out[name + "_res"] = dists, res
            out[name + "_inputs"] = np.array(TP.inputs_digest(codes, centers, Q))
        del lib
    path = os.path.join(HERE, "linscan_pq", "reference_outputs.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, len(TP.FIXTURE_CASES), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
