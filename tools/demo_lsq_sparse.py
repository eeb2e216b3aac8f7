"""The reference's demos/demo_lsq_sparse.jl flow against this package (SLSQ1: sparse codebooks, S = d h, tau = 0.7 ||C_pq||_1):
PQ init -> train_lsq_sparse (SPGL1 codebook update on the device) -> encode the base set -> quantise norms -> ADC linear scan -> recall.

    LSQ_DATA_DIR=/data python tools/demo_lsq_sparse.py [nread_train] [nread_base] [nquery]

SIFT1M under $LSQ_DATA_DIR/sift as in tools/demo_lsq_gpu.py; without it the same flow runs on that script's seeded synthetic stand-in."""
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from demo_lsq_gpu import load, lsq  # noqa: E402

ini = importlib.import_module("local-search-quantization_amd.initializers")


def main():
    real = bool(os.environ.get("LSQ_DATA_DIR"))
    nt = int(sys.argv[1]) if len(sys.argv) > 1 else (10_000 if real else 3000)
    nb = int(sys.argv[2]) if len(sys.argv) > 2 else (1_000_000 if real else 6000)
    nq = int(sys.argv[3]) if len(sys.argv) > 3 else (10_000 if real else 64)
    name, x_train, x_base, x_query, gt = load(nt, nb, nq)
    d = x_train.shape[0]
    m, h, niter, knn = (7, 256, 10, 1000) if name == "SIFT1M" else (4, 256, 3, 50)     # demo_lsq_sparse.jl:10-16
    eng = lsq.Engine(0)
    C, B, err = ini.train_pq(x_train, m, h, True, engine=eng)
    print("Error after PQ is %e" % err)
    ilsiter, icmiter, randord, npert = 8, 4, True, min(4, m)
    S = d * h                                                                # SLSQ1; d h + d^2 for SLSQ2
    tau = 0.7 * sum(float(np.abs(Cj.astype(np.float64)).sum()) for Cj in C)  # 0.7 for SLSQ1, 0.9 for SLSQ2 (demo_lsq_sparse.jl:27-37)
    infos = []
    t0 = time.perf_counter()
    C, B, R, train_error, cbnorms, objs = lsq.train_lsq_sparse(x_train, m, h, niter, ilsiter, icmiter, randord, npert, S, tau, B, C,
                                                                np.eye(d, dtype=np.float32), None, True, engine=eng, infos=infos)
    print("train_lsq_sparse: %.2f s; SPGL1 iterations per update %s; objs %s" % (time.perf_counter() - t0, [i["iterations"] for i in infos], objs.tolist()))
    B_base = lsq.randinit(x_base.shape[1], m, h)
    for i in range(16):                                                      # LSQ-16 on the base set (demo_lsq_sparse.jl:50-55)
        B_base = lsq.encoding_icm(x_base, B_base, C, icmiter, randord, npert, False, engine=eng)
    print("Error in base is %e" % lsq.qerror(x_base, B_base, C, engine=eng))
    nidx = lsq.quantize_norms(B_base, C, cbnorms, engine=eng)
    db_norms = np.asarray(cbnorms, dtype=np.float32)[nidx.astype(np.int64) - 1]
    dists, idx = lsq.linscan_lsq((B_base - 1).astype(np.uint8), x_query, C, db_norms, np.eye(d, dtype=np.float32), knn, engine=eng)
    rec = lsq.eval_recall(gt, idx.astype(np.uint32), knn, True)
    print("%s: recall@1 = %.4f, recall@%d = %.4f" % (name, rec[0], knn, rec[knn - 1]))
    eng.close()


if __name__ == "__main__":
    main()
