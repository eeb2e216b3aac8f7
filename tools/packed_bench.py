"""tools/packed_bench.py [n nq] -- the packed index (lsq_index_create_packed: rows of m code bytes and one norm byte) next to the plain index of the SAME
data (m code bytes and a float norm per row), one JSON line per grid point, written to profiles/packed.jsonl and printed.  Without arguments: 10^4 queries
x 10^6 codes x d = 128.

Data and codebooks as bench.py's `trained` workload builds them: synth_data_u8 rows (seed 1234), codebooks from train_lsq_dev on the first 100 000 rows
(8 iterations x 4 ILS x 4 ICM sweeps, seed 42), then one encode of the whole set (4 ILS iterations: the codes' quality does not enter the scan's time).
The norm table: 256 evenly ranked values of the reconstructions' squared norms, every row assigned by lsq_quantize_norms_dev (the reference trains the
table by k-means, LSQ.jl:67-84; which 256 values it holds does not enter the scan's time either).  The plain index gets dbnorms = cbnorms[byte]: both
indexes return the same bits, which is asserted on every pair of calls.

Grid: m in {7, 8, 15, 16}, nn in {100, 1000}; the exhaustive scan (lsq_index_search) and the inverted-list search at nlist = 1024, nprobe = 16
(train_coarse on 100 000 rows, every row assigned by ivf_assign).  One process; a warm-up of every call at full size; then plain and packed ALTERNATED,
device events around each call, option "profile" off, REPS repeats, medians; the phase times come from a pass of its own with "profile" on."""
import importlib, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lsq = importlib.import_module("local-search-quantization_amd")
REPS = 5
D, NLIST, NPROBE = 128, 1024, 16
PHASES = ("lut_ms", "sample_ms", "scan_ms", "select_ms")
IVF_PHASES = ("coarse_ms", "lut_ms", "scan_ms", "select_ms")


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def alternate(calls):
    """calls: name -> thunk; REPS rounds of every call in turn -> name -> (median ms, [min, max]), and the last results"""
    times, last = {k: [] for k in calls}, {}
    for _ in range(REPS):
        for k, f in calls.items():
            t, last[k] = timed(f)
            times[k].append(t)
    return {k: (round(statistics.median(v), 3), [round(min(v), 3), round(max(v), 3)]) for k, v in times.items()}, last


def main(n, nq):
    dev = torch.device("cuda:0")
    out = open(os.path.join(ROOT, "profiles", "packed.jsonl"), "w")

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    with lsq.Engine(0) as eng:
        X = eng.synth_data_u8_dev(1234, n, D)
        Q = eng.synth_data_u8_dev(777, nq, D)
        Xh = X.cpu().numpy()
        cent, _ = lsq.train_coarse(Xh[:min(n, 100_000)], NLIST, niter=5, seed=2, engine=eng)
        assign = torch.from_numpy(lsq.ivf_assign(Xh, cent, engine=eng)).to(dev)
        dcent = torch.from_numpy(cent).to(dev)
        del Xh
        for m in (7, 8, 15, 16):
            ns = min(n, 100_000)
            dK, _, _, _, _ = lsq.train_lsq_dev(X[:ns].contiguous(), m, 256, eng.randinit_dev(7, ns, m), 8, 4, 4, True, 4, seed=42, engine=eng,
                                               norm_codebook=False)
            dBs, _, _ = eng.encode_icm_dev(X, eng.randinit_dev(7, n, m), dK, m, [4], 4, 4, True, seed=42)
            codes = dBs[-1].contiguous()
            _, _, norms = eng.quantize_norms_dev(codes, dK, torch.zeros(1, dtype=torch.float32, device=dev), m)
            cb = torch.sort(norms)[0][torch.linspace(0, n - 1, 256, device=dev).round().long()].contiguous()
            nc, dbn, _ = eng.quantize_norms_dev(codes, dK, cb, m)
            with eng.index_dev(codes, dK, dbn.contiguous(), m) as plain, eng.index_packed_dev(codes, dK, nc, cb, m) as packed:
                plain.set_lists(dcent, assign)
                packed.set_lists(dcent, assign)
                pinfo = packed.packed_info()
                resident = dict(plain_bytes=n * (m + 4), packed_bytes=pinfo["resident_bytes"], plain_ivf_bytes=n * (m + 8),
                                packed_ivf_bytes=n * pinfo["ivf_row_bytes"], dword_rows=pinfo["dword_rows"], plain_dword_rows=int(m % 4 == 0))
                for nn in (100, 1000):
                    for kind, calls in (("scan", {"plain": lambda: plain.search(Q, nn), "packed": lambda: packed.search(Q, nn)}),
                                        ("ivf", {"plain": lambda: plain.search_ivf(Q, nn, NPROBE), "packed": lambda: packed.search_ivf(Q, nn, NPROBE)})):
                        for f in calls.values():                                 # warm-up at full size: code objects, work buffers
                            f()
                        torch.cuda.synchronize()
                        ms, last = alternate(calls)
                        assert torch.equal(last["plain"][1], last["packed"][1]) and torch.equal(last["plain"][0].view(torch.int32), last["packed"][0].view(torch.int32))
                        eng.set_option("profile", 1)
                        phases = {}
                        for k, f in calls.items():
                            f()
                            ix = plain if k == "plain" else packed
                            st = ix.scan_stats() if kind == "scan" else ix.ivf_info()
                            phases[k] = {p: round(st[p], 3) for p in (PHASES if kind == "scan" else IVF_PHASES)}
                            if kind == "scan":
                                phases[k].update(candidates_per_query=round(st["candidates"] / nq, 1), fallback_queries=st["fallback_queries"])
                        eng.set_option("profile", 0)
                        line = dict(bench="packed", kind=kind, n=n, d=D, m=m, nq=nq, nn=nn, reps=REPS,
                                    plain_ms=ms["plain"][0], plain_ms_min_max=ms["plain"][1], packed_ms=ms["packed"][0], packed_ms_min_max=ms["packed"][1],
                                    packed_over_plain=round(ms["packed"][0] / ms["plain"][0], 4), phases_plain_ms=phases["plain"],
                                    phases_packed_ms=phases["packed"], **resident)
                        if kind == "ivf":
                            line.update(nlist=NLIST, nprobe=NPROBE)
                        else:                                                    # the scan's LDS gathers: nq n m table reads of 4 bytes, over scan_ms
                            line.update(scan_gather_Gps_plain=round(nq * n * m / max(phases["plain"]["scan_ms"], 1e-6) / 1e6, 1),
                                        scan_gather_Gps_packed=round(nq * n * m / max(phases["packed"]["scan_ms"], 1e-6) / 1e6, 1))
                        emit(line)
            del codes, dBs, norms, dbn, nc
    out.close()


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:3]] + [1_000_000, 10_000][len(sys.argv) - 1:]
    main(*a)
