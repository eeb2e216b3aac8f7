"""tools/ivf_build_bench.py [n nlist] -- building a residual inverted-list index on the device (lsq_partition_*, csrc/lsq_partition.hip; train_coarse_dev,
build_ivf_residual_index) next to the numpy statement of the same build, and the index it gives next to the plain-code one.  One JSON line per item,
written to profiles/ivf_build.jsonl and printed.  Without arguments: 10^6 x 128, m = 8, nlist = 1024 -- tools/ivf_bench.py's mixture and codebook recipe.

  phase        assign, update, residuals, code_norms: the device call (device tensors in and out) against what a caller wrote before -- ivf_assign through
               host buffers, train_coarse's np.add.at means, X - centroids[assign] and its upload, the float64 ivf_residual_norms and its upload -- in one
               process, ALTERNATED, REPS repeats, medians.  Wall clock around calls that wait for their results.
  residuals    the kernel alone (option "profile": events around it inside the call), f32 and uint8 rows: bytes read and written over time, as a share of
               the 8.0 TB/s HBM peak and of the 6.29 TB/s a float4 copy reaches on this part.
  update       the kernel alone on the trained lists and on lists of which ONE holds half of the rows: the longest chain of dependent float64 adds.
  build        build_ivf_residual_index as a whole (assign, residuals, encode, code_norms, index, set_lists), f32 and uint8 rows.
  quality      mean squared error of the residual codes against the plain ones, and the share of the exact top-nn that search_ivf returns from either index at
               nprobe = 1, 4, 16, 64 (same m, same lists, same queries; residual: add_coarse=True)."""
import importlib, json, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lsq = importlib.import_module("local-search-quantization_amd")
REPS = 5
D, M, NN, NQ = 128, 8, 100, 1000
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
med = statistics.median


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def mixture(g, dev, centres, n):
    pick = torch.randint(0, centres.shape[0], (n,), device=dev, generator=g)
    return (centres[pick] + torch.randn((n, D), device=dev, generator=g)).contiguous()


def train_codebooks(eng, dXt, seed):
    B0 = eng.randinit_dev(seed, dXt.shape[0], M)
    return lsq.train_lsq_dev(dXt, M, 256, B0, 3, 2, 2, True, 4, seed=seed + 2, engine=eng, norm_codebook=False)[0]


def main(n, nlist):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    centres = 3.0 * torch.randn((2 * nlist, D), device=dev, generator=g)
    X, Q = mixture(g, dev, centres, n), mixture(g, dev, centres, NQ)
    out = open(os.path.join(ROOT, "profiles", "ivf_build.jsonl"), "w")

    def emit(**line):
        s = json.dumps(dict(bench="ivf_build", n=n, d=D, m=M, nlist=nlist, **line))
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    with lsq.Engine(0) as eng:
        ntrain, ncoarse = min(n, 20_000), min(n, 100_000)
        t_train, (part, _) = wall(lambda: lsq.train_coarse_dev(X[:ncoarse], nlist, 5, 2, engine=eng))
        dassign = part.assign(X)
        cent = part.centroids()
        sizes = torch.bincount(dassign.long(), minlength=nlist).cpu().numpy()
        emit(item="train_coarse_dev", rows=ncoarse, niter=5, ms=round(t_train, 1), list_rows_min_median_max=[int(sizes.min()), int(np.median(sizes)), int(sizes.max())])
        # codebooks: for the rows themselves and for the residuals of the same training prefix
        dKp = train_codebooks(eng, X[:ntrain].contiguous(), 3)
        dKr = train_codebooks(eng, part.residuals(X[:ntrain], dassign[:ntrain]), 3)
        # ---- the two indexes ----------------------------------------------------------------------------------------------------------------------
        enc = dict(engine=eng, ilsiters=[2], icmiter=2, npert=4, randord=True, seed=6)
        rep = {}
        t_build, ixr = wall(lambda: lsq.build_ivf_residual_index(X, part, dKr, M, report=rep, **enc))
        dBs, sums, _ = eng.encode_icm_dev(X, eng.randinit_dev(6, n, M), dKp, M, [2], 2, 4, True, seed=6)
        pcodes = dBs[-1].contiguous()
        _, _, pnorms = eng.quantize_norms_dev(pcodes, dKp, torch.zeros(1, dtype=torch.float32, device=dev), M)
        ixp = eng.index_dev(pcodes, dKp, pnorms.contiguous(), M)
        ixp.set_lists(cent, dassign)
        emit(item="build", rows="f32", ms=round(t_build, 1), mse_residual=rep["obj"], mse_plain=float(sums[-1]) / n)
        X8 = torch.clamp(torch.round(X * 6 + 128), 0, 255).to(torch.uint8)
        part8, _ = lsq.train_coarse_dev(X8[:ncoarse], nlist, 2, 2, engine=eng)
        t_build8, ix8 = wall(lambda: lsq.build_ivf_residual_index(X8, part8, dKr * 6, M, **enc))
        ix8.close()
        emit(item="build", rows="uint8", ms=round(t_build8, 1))
        # ---- quality: the share of the exact top-nn either index returns ------------------------------------------------------------------------------
        with eng.index_dev(None, None, None, 0, base=X) as truth_ix:
            truth = truth_ix.knn(Q, NN, id_base=1)[1].cpu().numpy()
        for nprobe in (1, 4, 16, 64):
            if nprobe > nlist:
                continue
            got = {"plain": ixp.search_ivf(Q, NN, nprobe)[1].cpu().numpy(), "residual": ixr.search_ivf(Q, NN, nprobe, add_coarse=True)[1].cpu().numpy()}
            emit(item="quality", nprobe=nprobe, nn=NN, nq=NQ,
                 **{"recall_top%d_%s" % (NN, k): round(float(np.mean([len(np.intersect1d(v[q], truth[q])) / NN for q in range(NQ)])), 4) for k, v in got.items()},
                 **{"nearest_found_%s" % k: round(float(np.mean([truth[q, 0] in v[q] for q in range(NQ)])), 4) for k, v in got.items()})
        rcodes = rep["codes"]
        # ---- phases: the device call against the numpy statement, alternated ---------------------------------------------------------------------------
        Xh, centh, assignh = X.cpu().numpy(), cent.cpu().numpy(), dassign.cpu().numpy()
        codesh, Kh = rcodes.cpu().numpy(), dKr.cpu().numpy()
        scratch = eng.partition_dev(cent)

        def np_update():
            sums = np.zeros((nlist, D), dtype=np.float64)
            np.add.at(sums, assignh, Xh)
            counts = np.bincount(assignh, minlength=nlist)
            return (sums / np.maximum(counts, 1)[:, None]).astype(np.float32)

        pairs = {"assign": (lambda: part.assign(X), lambda: lsq.ivf_assign(Xh, centh, engine=eng)),
                 "update": (lambda: scratch.update(X, dassign), np_update),
                 "residuals": (lambda: part.residuals(X, dassign), lambda: torch.from_numpy(Xh - centh[assignh]).to(dev)),
                 "code_norms": (lambda: part.code_norms(rcodes, dKr, dassign), lambda: torch.from_numpy(lsq.ivf_residual_norms(codesh, Kh, centh, assignh)).to(dev))}
        for name, (dev_call, np_call) in pairs.items():
            dev_call()                                                          # warm-up: code objects, work buffers
            td, th = [], []
            for _ in range(REPS):
                td.append(wall(dev_call)[0])
                th.append(wall(np_call)[0])
            emit(item="phase", phase=name, reps=REPS, device_ms=round(med(td), 3), device_ms_min_max=[round(min(td), 3), round(max(td), 3)],
                 numpy_ms=round(med(th), 1), numpy_ms_min_max=[round(min(th), 1), round(max(th), 1)], speedup=round(med(th) / med(td), 1))
        # ---- the kernels alone --------------------------------------------------------------------------------------------------------------------------
        eng.set_option("profile", 1)
        for rows, Xr, p in (("f32", X, part), ("uint8", X8, part8)):
            a = p.assign(Xr)
            ms = []
            for _ in range(REPS + 1):
                p.residuals(Xr, a)
                ms.append(p.info()["kernel_ms"])
            t = med(ms[1:])
            nbytes = n * D * (Xr.element_size() + 4) + 4 * n
            emit(item="residual_kernel", rows=rows, loader_bytes=p.info()["loader_bytes"], kernel_ms=round(t, 4), bytes=nbytes, TBps=round(nbytes / t / 1e9, 3),
                 share_of_hbm_peak=round(nbytes / (t * 1e-3) / HBM_PEAK, 3), share_of_float4_copy=round(nbytes / (t * 1e-3) / HBM_COPY, 3))
        giant = dassign.clone()
        giant[::2] = 0                                                          # one list holds (at least) half of the rows
        for name, lists in (("trained lists", dassign), ("one list of half the rows", giant)):
            gs, ks = [], []
            for _ in range(REPS + 1):
                scratch.update(X, lists)
                info = scratch.info()
                gs.append(info["group_ms"])
                ks.append(info["kernel_ms"])
            emit(item="update_kernel", lists=name, max_list_rows=info["max_list_rows"], empty_lists=info["empty_lists"], group_ms=round(med(gs[1:]), 3),
                 kernel_ms=round(med(ks[1:]), 3), ns_per_row_of_longest_list=round(med(ks[1:]) * 1e6 / max(info["max_list_rows"], 1), 2))
        eng.set_option("profile", 0)
    out.close()


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:3]] + [1_000_000, 1024][len(sys.argv) - 1:]
    main(*a)
