"""What a beam start costs and what it buys, at the headline shape (default 10^6 x 128, m = 8) with codebooks trained as bench.py's `trained` workload trains
them (train_lsq_dev on the first 100 000 vectors, 8 iterations x 4 ILS, seed 42):

    python tools/beam_bench.py [--vectors N] [--dim D] [--codebooks M] [--reps R] [--out profiles/beam.jsonl]

appends JSON lines to --out:
  {"kind": "shape", ...}            the problem, the build, the training objective
  {"kind": "beam_ms", "L": ..}      device-event ms of Encoder.beam (device form: the unary GEMMs of its chunks + the beam kernel), per repetition, for
                                    L in --beams; "unaries_ms" / "kernel_ms": the same call's two parts from a separate pass under option "profile"
  {"kind": "ils_ms", ...}           in the same process and ALTERNATED with the beam calls: encode_icm_dev with ilsiters [1] and [16] from random codes;
                                    "per_iteration" = (t16 - t1) / 15, the cost of an ILS iteration without the call's set-up
  {"kind": "objective", ...}        qerror after {random, beam-L} + I ILS iterations, I in 0, 1, 2, 4, 8, 16, for the ascending and the energy order
  {"kind": "start_plus_ils_ms", ..} event ms of {beam-L, then encode_icm_dev with [I]} for the (L, I) pairs of --pairs, next to {random + 16}
Timing follows the usual rules: every shape warmed up once, R repetitions, the variants alternated inside a repetition, medians reported with all values."""
import argparse
import hashlib
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H = 256
ILS = [1, 2, 4, 8, 16]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--vectors", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--codebooks", type=int, default=8)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--beams", default="1,4,8,16,32")
    p.add_argument("--pairs", default="4:8,8:8,16:4,16:8,32:2,32:4,32:8", help="L:I pairs timed as beam-L + I iterations")
    p.add_argument("--icmiter", type=int, default=4)
    p.add_argument("--npert", type=int, default=4)
    p.add_argument("--train-vectors", type=int, default=100_000)
    p.add_argument("--timing-only", action="store_true", help="skip the objective table")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam.jsonl"))
    a = p.parse_args()
    import torch
    lsq = importlib.import_module("local-search-quantization_amd")
    if not torch.cuda.is_available():
        raise SystemExit("beam_bench needs a GPU: nothing here is measured on the host")
    n, d, m = a.vectors, a.dim, a.codebooks
    beams = [int(x) for x in a.beams.split(",")]
    pairs = [tuple(int(v) for v in x.split(":")) for x in a.pairs.split(",") if x]
    lines = []

    def emit(**rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    with lsq.Engine(0) as eng:
        dX = eng.synth_data_u8_dev(1234, n, d)
        dB0 = eng.randinit_dev(7, n, m)
        ns = min(n, a.train_vectors)
        t0 = time.perf_counter()
        with lsq.Engine(0) as e2:
            dK, _, _, _, obj = lsq.train_lsq_dev(dX[:ns].contiguous(), m, H, dB0[:ns].contiguous(), 8, 4, a.icmiter, True, a.npert, seed=42, engine=e2,
                                                 norm_codebook=False)
        torch.cuda.synchronize()
        K = np.ascontiguousarray(dK.cpu().numpy())
        lib = hashlib.sha256(open(lsq._lib.LIB_PATH, "rb").read()).hexdigest()[:12]
        emit(kind="shape", n=n, d=d, m=m, h=H, data="synth_data_u8 seed 1234", train_vectors=ns, train_objective_first_last=[float(obj[0]), float(obj[-1])],
             train_seconds=round(time.perf_counter() - t0, 2), icmiter=a.icmiter, npert=a.npert, lib=lib, device=torch.cuda.get_device_name(0))
        Cs = [np.ascontiguousarray(K[j * H:(j + 1) * H].T) for j in range(m)]
        orders = {"ascending": None, "energy": lsq.beam_order(Cs)}
        one, sixteen = np.array([1], np.int64), np.array([16], np.int64)

        def ils(dB, ilsiters):
            return eng.encode_icm_dev(dX, dB, dK, m, ilsiters, a.icmiter, a.npert, True, seed=42)

        with eng.encoder_dev(dK, m) as enc:
            # ---- warm-up: every shape the timed window uses ------------------------------------------------------------------------------------------
            for L in beams:
                enc.beam(dX, L)
            ils(dB0, one)
            ils(dB0, sixteen)
            torch.cuda.synchronize()
            # ---- timings, alternated ------------------------------------------------------------------------------------------------------------------
            t_beam = {L: [] for L in beams}
            t_ils = {1: [], 16: []}
            t_pair = {pr: [] for pr in pairs}
            for _ in range(a.reps):
                for L in beams:
                    t_beam[L].append(event_ms(lambda: enc.beam(dX, L, order=orders["energy"]))[0])
                    t_ils[1].append(event_ms(lambda: ils(dB0, one))[0])
                t_ils[16].append(event_ms(lambda: ils(dB0, sixteen))[0])
                for (L, I) in pairs:
                    t_pair[(L, I)].append(event_ms(lambda: ils(enc.beam(dX, L, order=orders["energy"]), np.array([I], np.int64)))[0])
            med = lambda v: float(np.median(v))      # noqa: E731
            per_it = (med(t_ils[16]) - med(t_ils[1])) / 15.0
            emit(kind="ils_ms", encode_1=med(t_ils[1]), encode_16=med(t_ils[16]), per_iteration=per_it, encode_1_all=t_ils[1], encode_16_all=t_ils[16],
                 note="encode_icm_dev from random codes, event-timed, alternated with the beam calls")
            eng.set_option("profile", 1)
            for L in beams:
                enc.beam(dX, L, order=orders["energy"])
                torch.cuda.synchronize()
                info = enc.info()
                emit(kind="beam_ms", L=L, order="energy", ms=med(t_beam[L]), ms_all=t_beam[L], unaries_ms=info["unaries_ms"], kernel_ms=info["beam_ms"],
                     chunks=info["chunks"], in_ils_iterations=med(t_beam[L]) / per_it)
            eng.set_option("profile", 0)
            for (L, I) in pairs:
                emit(kind="start_plus_ils_ms", L=L, I=I, order="energy", ms=med(t_pair[(L, I)]), ms_all=t_pair[(L, I)], random_plus_16_ms=med(t_ils[16]))
            if a.timing_only:
                orders = {}
            # ---- objectives ---------------------------------------------------------------------------------------------------------------------------
            X = dX.cpu().numpy() if orders else None

            def objectives(dB):
                o0 = eng.qerror(X, dB.cpu().numpy().astype(np.int16) + 1, K, m)
                _, sums, _ = ils(dB, np.array(ILS, np.int64))
                return dict(zip(["0"] + [str(i) for i in ILS], [float(o0)] + [float(s) / n for s in sums]))

            if orders:
                emit(kind="objective", start="random", order=None, objective=objectives(dB0))
            for oname, order in orders.items():
                for L in beams:
                    emit(kind="objective", start="beam", L=L, order=oname, objective=objectives(enc.beam(dX, L, order=order)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
