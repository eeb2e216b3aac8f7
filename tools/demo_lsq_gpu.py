"""The reference's demos/demo_lsq_gpu.jl flow against this package (BASELINE's secondary metric, recall@1 on SIFT1M):
OPQ init -> ChainQ init -> train_lsq -> encode the base set on the GPU -> quantise norms -> ADC linear scan -> recall.

    LSQ_DATA_DIR=/data python tools/demo_lsq_gpu.py [--resident] [--bvecs] [--rerank L [--base-format f16|bf16]] [--ivf NLIST:NPROBE [--residual] [--grow FRACTION]] [--delete FRACTION] [--radius R] [--reconstruct] [--save PATH] [--load PATH] [--init beam:L] [--norm-byte] [nread_train] [nread_base] [nquery]

--resident: the three trainers run on ONE device tensor (train_opq_dev -> train_chainq_dev -> train_lsq_dev): the training set is uploaded once and
the codes and codebooks stay in HBM between the stages; the rest of the flow is unchanged.

--bvecs: the base set stays 8-bit end to end -- read with bvecs_read from the first *base*.bvecs file under $LSQ_DATA_DIR (SIFT1B layout: learn, base and
query .bvecs files and an .ivecs ground truth side by side), else the synthetic stand-in quantised to bytes -- and is handed to encode_icm_cuda as
uint8 (lsq_encode_icm_u8: d bytes per vector over the bus and in HBM).  The ground truth is exact k-NN of the 8-bit queries over the un-widened 8-bit base
(lsq_index_knn: integer distances, the f32 chain's bits).  Training set and scan queries are widened: the trainers and the scan take f32.

--init beam:L: the base set's initial codes come from the beam-search encoder (encode_beam, width L, codebooks visited by descending energy: beam_order)
instead of randinit (demos/demo_lsq_gpu.jl:46); the rest of the flow is unchanged.  Default: randinit, as the reference.

--base-format f16|bf16 (with --rerank L): the same two-stage search once more over half-precision base rows (Engine.index(..., base_format=)), its recall
curve printed beside the float32 one: what the format costs.
--rerank L: after the ADC scan, the two-stage search on a resident index (Engine.index: the codes, norms, codebooks and the base rows uploaded once):
the scan's L nearest re-ordered by exact distance to the stored vectors -- f32 rows, or the un-widened 8-bit rows with --bvecs -- and the recall curve of the
re-ranked lists printed next to the ADC one.  The reference has no such stage: its recall is that of the ADC order.

--ivf NLIST:NPROBE: after the ADC scan, inverted lists over the same codes (train_coarse on the base rows, Index.set_lists) and the search that reads
each query's NPROBE nearest lists alone (Index.search_ivf); its recall curve is printed next to the exhaustive one.  The reference has no such search.

--residual (with --ivf): the form of IVF that encodes what the coarse quantiser leaves, built resident on the device at the same m and NPROBE: the same
centroids, codebooks from the three resident trainers run on the training set's residuals (Partition.assign / residuals), the base set -- f32, or un-widened
bytes with --bvecs -- through build_ivf_residual_index, searched with add_coarse; with --norm-byte the norm codebook is the scalar k-means of the training
residuals' code_norms and the index is packed.  Its recall curve is printed as a third column.

--norm-byte: the norm byte that quantize_norms computes stays a byte up to the search: a packed index (Engine.index_packed, rows of m code bytes and one
norm byte: the 64-bit code at m = 7) is searched through linscan_lsq_bytes, and its ids and distances are checked to equal the float-norm run's.  The
reference widens the byte to a float per vector one line before its scan (demo_lsq_gpu.jl:57-60).

--grow FRACTION (with --ivf): the index is built on the first 1 - FRACTION of the base and the rest is APPENDED (Index.add): the partition is fixed, so the
new rows' lists come from Partition.assign row by row -- with --residual their residuals, codes and code_norms too (Partition.residuals, encode_icm_dev at
global_offset = the rows already held, Partition.code_norms).  The recall curve of the grown index is printed next to that of the whole build; whether the
two coincide exactly depends on the encoder being deterministic per row under global_offset, and the demo says which it saw.

--filter FRACTION: a seeded random mask that allows about FRACTION of the base rows is laid over a resident index (Index.set_filter); the ADC search -- and,
where given, the --ivf and --rerank variants -- then answer over the allowed rows alone, and their recall is taken against Index.knn under the SAME mask on
the same resident base rows.  The reference has no such search.

--delete FRACTION (alone or beside --ivf, --residual, --grow, whose sections run as before): a seeded random FRACTION of the base rows is removed from a
resident index (Index.remove: tombstones) and the recall of the ADC search -- and of the --ivf search over the same codes -- is taken against Index.knn over
the rows that are left; then Index.compact makes the rows leave, the same searches run again, and their ids, taken back through old_of_new, must name the
same rows: the demo asserts it and prints the two recall curves side by side.

--save PATH / --load PATH: the index over the base codes written to a snapshot file (Index.save; the section table with its digests is printed) / an index read
back from a snapshot (Engine.load_index) and searched -- the same ids as the exhaustive scan when both name one file.

--reconstruct: the base prefix decoded from the resident codes (Index.reconstruct) with its mean squared error against the base rows, with --ivf ...
--residual also the residual index decoded with the coarse add, and one search whose queries are stored rows (Index.search_rows).

--radius R (alone or beside --ivf and --filter, whose sections run as before): range search on a resident index (Index.range_search) -- every base row
whose ADC distance to the query is <= R, R in the scan's own units (the distances linscan_lsq prints), or `auto`: the median over the queries of the 10th
neighbour's distance.  The mean, minimum and maximum result counts are printed; with --ivf also the share of the exhaustive range result that the search
over the probed lists returns (it can only miss rows: its distances are the same bits); with --filter the counts under the mask.  The reference has no such
search.

needs $LSQ_DATA_DIR/sift/{sift_learn,sift_base,sift_query}.fvecs and sift_groundtruth.ivecs (TEXMEX layout).  The file's ground truth
describes the full 10^6-vector base only: for a prefix of it (nread_base < 10^6) and for the stand-in, the ground truth is exact k-NN of the base
actually encoded, computed on the device (knn_exact).  The data is
not in the build image; without it the script says so and runs the same flow on a small synthetic stand-in, so that the
wiring stays exercised (tests/test_pipeline_gpu.py asserts on that flow)."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lsq = importlib.import_module("local-search-quantization_amd")


def ground_truth(xb, xq):
    """1-based id of each query's nearest base vector: exact k-NN on the device (lsq_knn_exact; uint8 matrices stay uint8: lsq_index_knn)"""
    t0 = time.perf_counter()
    with lsq.Engine(0) as eng:
        _, ids = lsq.knn_exact(xb, xq, 1, engine=eng)
    print("Ground truth of %d queries in %d base vectors: %.3f s (exact k-NN on the device, %s rows)" % (xq.shape[1], xb.shape[1], time.perf_counter() - t0,
                                                                                                       xb.dtype))
    return ids[0]


def find_bvecs():
    """-> (learn, base, query) .bvecs paths of the first directory under $LSQ_DATA_DIR that has all three, or None"""
    root = os.environ.get("LSQ_DATA_DIR")
    if not root:
        return None
    for dirpath, _, files in sorted(os.walk(root)):
        got = {}
        for f in sorted(files):
            if f.endswith(".bvecs"):
                for role in ("learn", "base", "query"):
                    if role in f:
                        got.setdefault(role, os.path.join(dirpath, f))
        if len(got) == 3:
            return got["learn"], got["base"], got["query"]
    return None


def load_bvecs(nt, nb, nq):
    """-> name, x_train f32, x_base UINT8, x_query f32, ground truth (exact k-NN of the base actually encoded)"""
    paths = find_bvecs()
    if paths:
        xt8, xb8, xq8 = lsq.bvecs_read(nt, paths[0]), lsq.bvecs_read(nb, paths[1]), lsq.bvecs_read(nq, paths[2])
        name = "bvecs"
    else:
        print("no learn / base / query .bvecs under $LSQ_DATA_DIR -- running the synthetic stand-in quantised to bytes")
        _, xt, xb, xq, _ = load(nt, nb, nq, want_gt=False, synthetic=True)
        lo, hi = min(xt.min(), xb.min(), xq.min()), max(xt.max(), xb.max(), xq.max())
        xt8, xb8, xq8 = (np.rint((x - lo) * (255.0 / (hi - lo))).astype(np.uint8) for x in (xt, xb, xq))
        name = "synthetic"
    xq = xq8.astype(np.float32)
    return name, xt8.astype(np.float32), xb8, xq, ground_truth(xb8, xq8)      # from the 8-bit base as it is: no widened copy


def load(nt, nb, nq, want_gt=True, synthetic=False):
    base = os.path.join(os.environ.get("LSQ_DATA_DIR", ""), "sift")
    names = ["sift_learn.fvecs", "sift_base.fvecs", "sift_query.fvecs", "sift_groundtruth.ivecs"]
    if not synthetic and os.environ.get("LSQ_DATA_DIR") and all(os.path.exists(os.path.join(base, f)) for f in names):
        xt = lsq.fvecs_read(nt, os.path.join(base, names[0]))
        xb = lsq.fvecs_read(nb, os.path.join(base, names[1]))
        xq = lsq.fvecs_read(nq, os.path.join(base, names[2]))
        if nb == 1_000_000:                                                   # the file describes the full base only
            gt = lsq.ivecs_read(nq, os.path.join(base, names[3]))[0] + 1      # 0-based in the file (demo_lsq_gpu.jl:62-64)
        else:                                                                 # a prefix: exact k-NN of the base actually encoded
            gt = ground_truth(xb, xq)
        return "SIFT1M", xt, xb, xq, gt.astype(np.uint32)
    print("SIFT1M not found under $LSQ_DATA_DIR/sift -- running the synthetic stand-in (clustered Gaussians, d = 32)")
    rng = np.random.default_rng(1)
    d, k = 32, 400
    cen = rng.standard_normal((d, k)).astype(np.float32) * 3.0
    allx = (cen[:, rng.integers(k, size=nt + nb + nq)] + 0.35 * rng.standard_normal((d, nt + nb + nq))).astype(np.float32)
    xt, xb, xq = allx[:, :nt], allx[:, nt:nt + nb], allx[:, nt + nb:]
    return "synthetic", xt, xb, xq, ground_truth(xb, xq) if want_gt else None


def train_resident_dev(eng, dX, m, h, niter, ilsiter, icmiter, randord, npert, what=""):
    """the three training stages on one device tensor -> train_lsq_dev's result"""
    dK, dB, R, err = lsq.train_opq_dev(dX, m, h, niter, "natural", engine=eng)
    print("Error after OPQ%s is %e" % (what, err[-1]))
    dK, dB, R, err = lsq.train_chainq_dev(dX, m, h, R, dB, niter, engine=eng)
    print("Error after ChainQ%s is %e" % (what, err[-1]))
    return lsq.train_lsq_dev(dX, m, h, dB, niter, ilsiter, icmiter, randord, npert, engine=eng, R=R)


def train_resident(x_train, m, h, niter, ilsiter, icmiter, randord, npert):
    """... uploaded once -> what train_lsq returns, in its host shapes"""
    import torch
    t0 = time.perf_counter()
    with lsq.Engine(0) as eng:
        dX = torch.from_numpy(np.ascontiguousarray(x_train.T)).cuda()
        dK, dB, cbnorms, B_norms, obj = train_resident_dev(eng, dX, m, h, niter, ilsiter, icmiter, randord, npert)
        torch.cuda.synchronize()
        K = dK.cpu().numpy()
        B = np.ascontiguousarray(dB.cpu().numpy().T.astype(np.int16) + 1)
    print("Error after LSQ is %e; the three resident trainers took %.3f s" % (obj[-1], time.perf_counter() - t0))
    return [np.ascontiguousarray(K[i * h:(i + 1) * h].T) for i in range(m)], B, cbnorms, B_norms, obj


def residual_ivf(eng, x_train, x_base, Q, gt, cent, assign, m, h, niter, ilsiter, icmiter, randord, npert, nprobe, knn, norm_byte, n0=None, recon=False):
    """the residual index over the SAME centroids and lists, resident on the device -> (recall curve, seconds of the build, error in base, and with n0 the
    recall curve of the index built on the first n0 rows and grown by the rest -- else None)"""
    import torch
    dXt = torch.from_numpy(np.ascontiguousarray(x_train.T)).cuda()
    dXb = torch.from_numpy(np.ascontiguousarray(x_base.T)).cuda()            # f32, or the un-widened bytes of --bvecs
    with eng.partition_dev(torch.from_numpy(cent).cuda()) as part:
        # codebooks for residuals: the three resident trainers, as for the rows themselves, on the training set's residuals
        ta = part.assign(dXt)
        dK, dBt, _, _, obj = train_resident_dev(eng, part.residuals(dXt, ta), m, h, niter, ilsiter, icmiter, randord, npert, " of the residuals")
        print("Error after LSQ of the residuals is %e" % obj[-1])
        cb = None
        if norm_byte:                                                       # the norm codebook: the host scalar k-means of train_lsq_dev, fed with code_norms
            nrm = part.code_norms(dBt, dK, ta).cpu().numpy()
            cb = lsq.initializers.kmeans(nrm.reshape(1, -1), min(h, nrm.shape[0]), niter=100, seed=0)[0].reshape(-1).astype(np.float32)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = {}
        ix = lsq.build_ivf_residual_index(dXb, part, dK, m, engine=eng, ilsiters=[16], icmiter=icmiter, npert=npert, randord=randord, cbnorms=cb, report=rep)
        torch.cuda.synchronize()
        t_build = time.perf_counter() - t0
        assert np.array_equal(rep["assign"].cpu().numpy(), assign), "the device assignment differs from ivf_assign's"
        with ix:
            _, ridx = ix.search_ivf(torch.from_numpy(Q).cuda(), knn, nprobe, add_coarse=True)
            ridx = ridx.cpu().numpy()
            if recon:                                                       # --reconstruct: the residual codes decoded with the centroid of each row's list
                pre = min(int(dXb.shape[0]), 100000)
                xh = ix.reconstruct(count=pre, add_coarse=True)
                mse = float(((dXb[:pre].float() - xh).double() ** 2).sum(dim=1).mean().item())
                print("Decoded %d rows of the residual index on the device (centroid + residual codes): mean squared error against the base rows %e; row -> list "
                      "map built once (%d)" % (pre, mse, ix.recon_info()["map_rebuilds"]))
        grec = None
        if n0 is not None:                                                  # --grow: the same build on the first n0 rows, the rest appended
            gx = lsq.build_ivf_residual_index(dXb[:n0], part, dK, m, engine=eng, ilsiters=[16], icmiter=icmiter, npert=npert, randord=randord, cbnorms=cb)
            with gx:
                dXn = dXb[n0:]
                ta = part.assign(dXn)
                nnew = int(dXn.shape[0])
                dBs, _, _ = eng.encode_icm_dev(part.residuals(dXn, ta), eng.randinit_dev(0, nnew, m, device=dXn.device, global_offset=n0), dK, m, [16], icmiter,
                                               npert, randord, seed=0, global_offset=n0)
                if cb is None:
                    gx.add(codes=dBs[-1], dbnorms=part.code_norms(dBs[-1], dK, ta), assign=ta)
                else:
                    _, dnc, _ = part.code_norms(dBs[-1], dK, ta, torch.from_numpy(cb).cuda())
                    gx.add(codes=dBs[-1], norm_codes=dnc, assign=ta)
                _, gidx = gx.search_ivf(torch.from_numpy(Q).cuda(), knn, nprobe, add_coarse=True)
                same = bool(torch.equal(gidx.cpu(), torch.from_numpy(ridx)))
                print("Residual IVF index grown from %d to %d rows (Index.add): %d rows held, results %s the whole build's"
                      % (n0, n0 + nnew, gx.n, "EQUAL" if same else "differ from"))
                grec = lsq.eval_recall(gt, np.ascontiguousarray(gidx.cpu().numpy().T).astype(np.uint32), knn)
    return lsq.eval_recall(gt, np.ascontiguousarray(ridx.T).astype(np.uint32), knn), t_build, rep["obj"], grec


BASE_FORMAT = None                               # --base-format f16 | bf16 (with --rerank): the recall curve of half-precision base rows beside the f32 one


def main():
    global BASE_FORMAT
    argv = sys.argv[1:]
    if "--base-format" in argv:
        at = argv.index("--base-format")
        BASE_FORMAT = argv[at + 1]
        del argv[at:at + 2]
        if BASE_FORMAT not in ("f16", "bf16"):
            raise SystemExit("--base-format takes f16 or bf16, got %r" % BASE_FORMAT)
        if "--rerank" not in argv:
            raise SystemExit("--base-format needs --rerank L")
    shortlist = 0
    if "--rerank" in argv:
        at = argv.index("--rerank")
        shortlist = int(argv[at + 1])
        del argv[at:at + 2]
    init = "random"
    if "--init" in argv:
        at = argv.index("--init")
        init = argv[at + 1]
        del argv[at:at + 2]
        if init != "random" and not (init.startswith("beam:") and init[5:].isdigit()):
            raise SystemExit("--init takes `random` or `beam:L`, got %r" % init)
    ivf = None
    if "--ivf" in argv:
        at = argv.index("--ivf")
        try:
            ivf = tuple(int(x) for x in argv[at + 1].split(":"))
            assert len(ivf) == 2 and 1 <= ivf[1] <= ivf[0]
        except (ValueError, AssertionError, IndexError):
            raise SystemExit("--ivf takes NLIST:NPROBE with 1 <= NPROBE <= NLIST")
        del argv[at:at + 2]
    fraction = None
    if "--filter" in argv:
        at = argv.index("--filter")
        try:
            fraction = float(argv[at + 1])
            assert 0.0 < fraction <= 1.0
        except (ValueError, AssertionError, IndexError):
            raise SystemExit("--filter takes a FRACTION in (0, 1]")
        del argv[at:at + 2]
    delete = None
    if "--delete" in argv:
        at = argv.index("--delete")
        try:
            delete = float(argv[at + 1])
            assert 0.0 < delete < 1.0
        except (ValueError, AssertionError, IndexError):
            raise SystemExit("--delete takes a FRACTION in (0, 1)")
        del argv[at:at + 2]
    radius = None
    if "--radius" in argv:
        at = argv.index("--radius")
        try:
            radius = argv[at + 1] if argv[at + 1] == "auto" else float(argv[at + 1])
        except (ValueError, IndexError):
            raise SystemExit("--radius takes a distance R or `auto`")
        del argv[at:at + 2]
    snap = {}
    for flag in ("--save", "--load"):
        if flag in argv:
            at = argv.index(flag)
            if at + 1 >= len(argv):
                raise SystemExit("%s takes a PATH" % flag)
            snap[flag] = argv[at + 1]
            del argv[at:at + 2]
    grow = None
    if "--grow" in argv:
        at = argv.index("--grow")
        try:
            grow = float(argv[at + 1])
            assert 0.0 < grow < 1.0
        except (ValueError, AssertionError, IndexError):
            raise SystemExit("--grow takes a FRACTION in (0, 1)")
        del argv[at:at + 2]
        if not ivf:
            raise SystemExit("--grow needs --ivf NLIST:NPROBE")
    args = [a for a in argv if a not in ("--resident", "--bvecs", "--norm-byte", "--residual", "--reconstruct")]
    resident, bvecs, norm_byte, residual, recon = "--resident" in argv, "--bvecs" in argv, "--norm-byte" in argv, "--residual" in argv, "--reconstruct" in argv
    if residual and not ivf:
        raise SystemExit("--residual needs --ivf NLIST:NPROBE")
    real = bool(os.environ.get("LSQ_DATA_DIR"))
    nt = int(args[0]) if len(args) > 0 else (10_000 if real else 3000)
    nb = int(args[1]) if len(args) > 1 else (1_000_000 if real else 6000)
    nq = int(args[2]) if len(args) > 2 else (10_000 if real else 64)
    name, x_train, x_base, x_query, gt = load_bvecs(nt, nb, nq) if bvecs else load(nt, nb, nq)
    d = x_train.shape[0]
    m, h, niter, knn = (7, 256, 10, 1000) if name in ("SIFT1M", "bvecs") else (4, 256, 3, 50)     # demo_lsq_gpu.jl:13-20
    ilsiter, icmiter, randord, npert = 8, 4, True, 4
    if resident:
        C, B, cbnorms, B_norms, obj = train_resident(x_train, m, h, niter, ilsiter, icmiter, randord, min(npert, m))
    else:
        C, B, R, err = lsq.train_opq(x_train, m, h, niter, "natural", True)
        print("Error after OPQ is %e" % err[-1])
        with lsq.Engine(0) as eng:                                          # ChainQ with its structured codebook update on the device as well
            C, B, R, err = lsq.train_chainq(x_train, m, h, R, B, C, niter, engine=eng, device_update=True)
        print("Error after ChainQ is %e" % err[-1])
        C, B, cbnorms, B_norms, obj = lsq.train_lsq(x_train, m, h, R, B, C, niter, ilsiter, icmiter, randord, min(npert, m), True)
    if init.startswith("beam:"):
        t0 = time.perf_counter()
        with lsq.Engine(0) as eng:
            B_base = lsq.encode_beam(x_base, C, int(init[5:]), order=lsq.beam_order(C), engine=eng)
        print("Initial codes of the base set by beam search of width %s: %.3f s (host buffers)" % (init[5:], time.perf_counter() - t0))
    else:
        B_base = lsq.randinit(x_base.shape[1], m, h)
    t0 = time.perf_counter()
    Bs, objs = lsq.encode_icm_cuda(x_base, B_base, C, [16], icmiter, min(npert, m), randord, 2, True)
    dt = time.perf_counter() - t0
    B_base = Bs[-1]
    print("Encoded %d base vectors in %.3f s (%.0f vectors/s, host buffers, %s rows); error in base is %e" % (x_base.shape[1], dt, x_base.shape[1] / dt,
                                                                                                       x_base.dtype, objs[-1]))
    assert x_base.dtype == (np.uint8 if bvecs else np.float32)
    with lsq.Engine(0) as eng:                                              # norm quantisation on the device (lsq_quantize_norms), checked against the mirror
        nidx = lsq.quantize_norms(B_base, C, cbnorms, engine=eng)
    assert np.array_equal(nidx, lsq.quantize_norms(B_base, C, cbnorms)), "device and host norm quantisation disagree"
    db_norms = np.asarray(cbnorms, dtype=np.float32)[nidx.astype(np.int64) - 1]
    t0 = time.perf_counter()
    with lsq.Engine(0) as eng:                                              # the ADC scan on the device (lsq_linscan) ...
        dists, idx = lsq.linscan_lsq((B_base - 1).astype(np.uint8), x_query, C, db_norms, np.eye(d, dtype=np.float32), knn, engine=eng)
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    dists_h, idx_h = lsq.linscan_lsq((B_base - 1).astype(np.uint8), x_query, C, db_norms, np.eye(d, dtype=np.float32), knn)   # ... and on the host cores
    t_host = time.perf_counter() - t0
    assert np.array_equal(idx, idx_h) and np.array_equal(dists, dists_h), "device and host scans disagree"
    print("Searched %d queries: device %.3f s (host buffers, incl. copies), host %.3f s; identical results" % (x_query.shape[1], t_dev, t_host))
    rec = lsq.eval_recall(gt, idx.astype(np.uint32), knn, True)
    print("%s: recall@1 = %.4f, recall@%d = %.4f" % (name, rec[0], knn, rec[knn - 1]))
    if norm_byte:
        t0 = time.perf_counter()
        with lsq.Engine(0) as eng:                                          # the same scan on rows of m + 1 bytes: the norm stays the byte quantize_norms made
            bd, bidx = lsq.linscan_lsq_bytes((B_base - 1).astype(np.uint8), x_query, C, np.asarray(cbnorms, dtype=np.float32), nidx,
                                             np.eye(d, dtype=np.float32), knn, engine=eng)
        t_byte = time.perf_counter() - t0
        assert np.array_equal(bidx, idx) and np.array_equal(bd.view(np.uint32), dists.view(np.uint32)), "the packed index and the float-norm scan disagree"
        print("Norm byte kept (%d bytes per vector resident instead of %d): %.3f s incl. the upload of the index; ids and distances equal the float-norm run's"
              % (m + 1, m + 4, t_byte))
    if shortlist:
        L = min(shortlist, x_base.shape[1])
        keep = min(knn, L)
        t0 = time.perf_counter()
        with lsq.Engine(0) as eng:                                          # stage two: the scan's L nearest re-ordered by exact distance, on a resident index
            rd, ridx = lsq.linscan_lsq_rerank((B_base - 1).astype(np.uint8), x_query, C, db_norms, np.eye(d, dtype=np.float32), x_base, L, keep, engine=eng)
        t_two = time.perf_counter() - t0
        rrec = lsq.eval_recall(gt, ridx.astype(np.uint32), keep)
        hrec = None
        if BASE_FORMAT:                                                      # --base-format: the same search over half-precision base rows (2 d bytes per row)
            with lsq.Engine(0) as eng:
                _, hidx = lsq.linscan_lsq_rerank((B_base - 1).astype(np.uint8), x_query, C, db_norms, np.eye(d, dtype=np.float32),
                                                 np.asarray(x_base, dtype=np.float32), L, keep, engine=eng, base_format=BASE_FORMAT)
            hrec = lsq.eval_recall(gt, hidx.astype(np.uint32), keep)
        print("Two-stage search (shortlist %d, %s rows resident): %.3f s incl. the upload of the index" % (L, x_base.dtype, t_two))
        print("     r@   ADC      re-ranked" + ("   re-ranked on %s rows" % BASE_FORMAT if BASE_FORMAT else ""))
        for i in (1, 2, 5, 10, 20, 50, 100, 200, 500, 1000):
            if i <= keep:
                print("%7d   %.4f   %.4f" % (i, rec[i - 1], rrec[i - 1]) + ("      %.4f" % hrec[i - 1] if BASE_FORMAT else ""))
        print("%s: recall@1 after re-ranking %d = %.4f (ADC: %.4f)" % (name, L, rrec[0], rec[0]))
    if ivf:
        nlist, nprobe = min(ivf[0], x_base.shape[1]), ivf[1]
        nprobe = min(nprobe, nlist)
        rows = np.ascontiguousarray(np.asarray(x_base, dtype=np.float32).T)
        Q = np.ascontiguousarray(x_query.T)
        with lsq.Engine(0) as eng:                                          # inverted lists over the same codes: the scan reads the probed lists alone
            cent, assign = lsq.train_coarse(rows, nlist, niter=10, seed=0, engine=eng)
            with eng.index((B_base - 1).astype(np.uint8).T, np.ascontiguousarray(np.hstack(C).T), db_norms, m) as ix:
                ix.set_lists(cent, assign)
                t0 = time.perf_counter()
                _, iidx = ix.search_ivf(Q, knn, nprobe)
                t_ivf = time.perf_counter() - t0
                info = ix.ivf_info()
            nb_all = x_base.shape[1]
            n0 = max(1, nb_all - max(1, int(round(grow * nb_all)))) if grow else None
            grec = gres = None
            if grow:                                                        # the index on the first n0 rows, the rest appended; lists of the new rows: Partition.assign
                codes_all = np.ascontiguousarray((B_base - 1).astype(np.uint8).T)
                with eng.index(codes_all[:n0], np.ascontiguousarray(np.hstack(C).T), db_norms[:n0], m) as gx, eng.partition(cent) as part:
                    gx.set_lists(cent, assign[:n0])
                    new_lists = np.asarray(part.assign(rows[n0:]), dtype=np.int32)
                    gx.add(codes=codes_all[n0:], dbnorms=db_norms[n0:], assign=new_lists)
                    _, gidx = gx.search_ivf(Q, knn, nprobe)
                    print("IVF index grown from %d to %d rows (Index.add); the new rows' lists %s ivf_assign's; results %s the whole build's"
                          % (n0, gx.n, "equal" if np.array_equal(new_lists, assign[n0:]) else "DIFFER from", "EQUAL" if np.array_equal(gidx, iidx) else "differ from"))
                grec = lsq.eval_recall(gt, np.ascontiguousarray(gidx.T).astype(np.uint32), knn)
            if residual:
                rrec_ivf, t_res, mse, gres = residual_ivf(eng, x_train, x_base, Q, gt, cent, assign, m, h, niter, ilsiter, icmiter, randord, min(npert, m),
                                                          nprobe, knn, norm_byte, n0, recon)
        irec = lsq.eval_recall(gt, np.ascontiguousarray(iidx.T).astype(np.uint32), knn)
        print("IVF search (nlist %d, nprobe %d): %.3f s on the resident index; %.0f of %d rows probed per query, %d of %d queries on the thresholded road"
              % (nlist, nprobe, t_ivf, info["probed_rows"] / Q.shape[0], x_base.shape[1], info["threshold_queries"], Q.shape[0]))
        if residual:
            print("Residual IVF index (%s rows, %s norms) built on the device in %.3f s; error in base is %e (plain codes: %e)"
                  % (x_base.dtype, "byte" if norm_byte else "float", t_res, mse, objs[-1]))
        print("     r@   exhaustive   IVF" + ("          residual IVF" if residual else "") + ("     grown IVF" if grow else "") + ("   grown residual IVF" if gres is not None else ""))
        for i in (1, 2, 5, 10, 20, 50, 100, 200, 500, 1000):
            if i <= knn:
                print("%7d   %.4f       %.4f" % (i, rec[i - 1], irec[i - 1]) + ("       %.4f" % rrec_ivf[i - 1] if residual else "")
                      + ("         %.4f" % grec[i - 1] if grow else "") + ("      %.4f" % gres[i - 1] if gres is not None else ""))
    if fraction is not None:
        filtered_recall(fraction, name, x_base, x_query, B_base, C, db_norms, m, knn, shortlist, ivf)
    if delete is not None:
        deleted_recall(delete, name, x_base, x_query, B_base, C, db_norms, m, knn, ivf)
    if radius is not None:
        if radius == "auto":
            radius = float(np.median(dists[min(10, knn) - 1]))
        range_counts(radius, name, x_base, x_query, B_base, C, db_norms, m, ivf, fraction)
    if recon:
        reconstruct_rows(name, x_base, B_base, C, db_norms, m, knn)
    if snap:
        snapshot_roundtrip(snap, name, x_query, B_base, C, db_norms, m, knn, gt, idx)


def snapshot_roundtrip(snap, name, x_query, B_base, C, db_norms, m, knn, gt, idx):
    """--save PATH: the index over the base codes written to a snapshot file (Index.save), its section table printed.  --load PATH: an index read back from
    a snapshot (Engine.load_index) and searched; its ids are compared with the exhaustive scan's when the file holds as many rows"""
    Q = np.ascontiguousarray(x_query.T)
    with lsq.Engine(0) as eng:
        if "--save" in snap:
            with eng.index((B_base - 1).astype(np.uint8).T, np.ascontiguousarray(np.hstack(C).T), db_norms, m) as ix:
                t0 = time.perf_counter()
                ix.save(snap["--save"])
                dt = time.perf_counter() - t0
                info, io = lsq.snapshot_info(snap["--save"], verify=True), ix.snapshot_info()
                print("Saved the index of %d rows to %s: %d bytes in %d sections and %d chunks, %.3f s; the file's table equals the index's digest: %s"
                      % (ix.n, snap["--save"], info["file_bytes"], info["nsections"], io["chunks"], dt, info["sections"] == ix.digest()["sections"]))
                for sec in info["sections"]:
                    print("   %-12s %12d bytes at %12d   digest %016x" % (sec["name"], sec["bytes"], sec["offset"], sec["digest"]))
        if "--load" in snap:
            t0 = time.perf_counter()
            with eng.load_index(snap["--load"]) as lx:
                dt = time.perf_counter() - t0
                _, lidx = lx.search(Q, min(knn, lx.n))
                print("Loaded an index of %d rows (d = %d, m = %d) from %s in %.3f s" % (lx.n, lx.d, lx.m, snap["--load"], dt))
                if lx.n == B_base.shape[1]:
                    lrec = lsq.eval_recall(gt, np.ascontiguousarray(lidx.T).astype(np.uint32), min(knn, lx.n))
                    print("%s: recall@1 of the loaded index = %.4f; ids %s the exhaustive scan's" % (name, lrec[0], "EQUAL" if np.array_equal(lidx.T, idx) else "differ from"))


def reconstruct_rows(name, x_base, B_base, C, db_norms, m, knn):
    """--reconstruct: the base prefix decoded from the resident codes (Index.reconstruct) and its mean squared error against the base rows -- the encode's
    objective, measured from the index alone -- then one search whose queries are stored rows (Index.search_rows)"""
    n = x_base.shape[1]
    pre, k = min(n, 100000), min(knn, 10)
    with lsq.Engine(0) as eng, eng.index((B_base - 1).astype(np.uint8).T, np.ascontiguousarray(np.hstack(C).T), db_norms, m) as ix:
        t0 = time.perf_counter()
        xh = ix.reconstruct(count=pre)
        dt = time.perf_counter() - t0
        assert np.array_equal(xh.view(np.uint32), np.ascontiguousarray(lsq.reconstruct(B_base[:, :pre], C).T).view(np.uint32)) or np.isnan(xh).any(), \
            "the device decode and the numpy mirror disagree"
        mse = float(((np.asarray(x_base[:, :pre], dtype=np.float32).T.astype(np.float64) - xh) ** 2).sum(axis=1).mean())
        rows = np.arange(0, n, max(1, n // 8), dtype=np.int32)[:8]
        dists, ids = ix.search_rows(rows, k)
        own = int(sum(int(rows[q]) + 1 == int(ids[q, 0]) for q in range(rows.shape[0])))
    print("Decoded %d base rows from the resident codes in %.3f s (host buffers, incl. the fetch), the numpy mirror's bits; mean squared error against the base "
          "rows %e" % (pre, dt, mse))
    print("%s: neighbours of %d stored rows (search_rows, k = %d): %d of them are their own nearest row (no self-exclusion; quantised norms)"
          % (name, rows.shape[0], k, own, ))


def range_counts(radius, name, x_base, x_query, B_base, C, db_norms, m, ivf, fraction):
    """--radius: every row within ADC distance `radius` of each query (Index.range_search): the result counts over all rows, over the probed lists of
    --ivf (and the share of the exhaustive result they hold), and under the mask of --filter"""
    n = x_base.shape[1]
    Q = np.ascontiguousarray(x_query.T.astype(np.float32))

    def line(label, lims):
        c = np.diff(lims)
        return "%-28s mean %10.2f   min %8d   max %8d" % (label, c.mean(), c.min(), c.max())

    out = []
    with lsq.Engine(0) as eng, eng.index((B_base - 1).astype(np.uint8).T, np.ascontiguousarray(np.hstack(C).T), db_norms, m) as ix:
        t0 = time.perf_counter()
        lims, rd, ri = ix.range_search(Q, radius)
        t_all = time.perf_counter() - t0
        info = ix.range_info()
        out.append(line("every row", lims))
        if ivf:
            nlist = min(ivf[0], n)
            nprobe = min(ivf[1], nlist)
            cent, assign = lsq.train_coarse(np.ascontiguousarray(np.asarray(x_base, dtype=np.float32).T), nlist, niter=10, seed=0, engine=eng)
            ix.set_lists(cent, assign)
            ilims, _, iids = ix.range_search(Q, radius, nprobe=nprobe)
            # the probed lists' result is a subset of the exhaustive one (the same distance bits): the share is a ratio of counts
            share = float(ilims[-1]) / max(float(lims[-1]), 1.0)
            assert all(np.isin(iids[ilims[q]:ilims[q + 1]], ri[lims[q]:lims[q + 1]]).all() for q in range(min(Q.shape[0], 16)))
            out.append(line("IVF %d:%d" % (nlist, nprobe), ilims) + "   share of the exhaustive result %.4f" % share)
        if fraction is not None:
            allowed = np.random.default_rng(0).random(n) < fraction
            ix.set_filter(mask=allowed)
            flims, _, fids = ix.range_search(Q, radius)
            assert allowed[fids - 1].all()
            out.append(line("filter %g (%s road)" % (fraction, {0: "unfiltered", 1: "dense", 2: "compact"}[ix.range_info()["road"]]), flims))
    print("Range search (radius %g, %d queries, %d rows): %.3f s on the resident index incl. the fetch; %d results held in %d bytes, %d fill batch(es)"
          % (radius, Q.shape[0], n, t_all, info["results"], info["held_bytes"], info["batches"]))
    for text in out:
        print("   " + text)
    print("%s: mean range result at radius %g = %.2f rows" % (name, radius, np.diff(lims).mean()))


def deleted_recall(fraction, name, x_base, x_query, B_base, C, db_norms, m, knn, ivf):
    """--delete: a seeded random fraction of the rows removed (Index.remove: tombstones), the recall of the searches over the rest against Index.knn over
    the rest; then Index.compact -- the rows leave --, the same searches again, and their ids, taken back through old_of_new, must be the same sets"""
    n = x_base.shape[1]
    gone = np.flatnonzero(np.random.default_rng(1).random(n) < fraction).astype(np.int32)
    gone = gone[: n - 1]                                                     # an index holds at least one row
    rows = np.ascontiguousarray(x_base.T)
    Q = np.ascontiguousarray(x_query.T.astype(np.float32))
    keep = max(1, min(knn, n - gone.shape[0]))
    with lsq.Engine(0) as eng, eng.index((B_base - 1).astype(np.uint8).T, np.ascontiguousarray(np.hstack(C).T), db_norms, m, base=rows) as ix:
        nprobe = 0
        if ivf:
            nlist = min(ivf[0], n)
            nprobe = min(ivf[1], nlist)
            cent, assign = lsq.train_coarse(np.asarray(rows, dtype=np.float32), nlist, niter=10, seed=0, engine=eng)
            ix.set_lists(cent, assign)

        def curves(back):
            """name -> (recall curve, ids 1-based in the numbering before the compact); back: None, or old_of_new"""
            to_old = (lambda ids: ids) if back is None else (lambda ids: np.where(ids > 0, back[np.maximum(ids, 1) - 1] + 1, 0))
            _, truth = ix.knn(Q, 1, id_base=1)                               # the ground truth: exact k-NN over the rows that are left
            gt = to_old(truth)[:, 0].astype(np.uint32)
            out = {}
            for label, ids in [("ADC", ix.search(Q, keep)[1])] + ([("IVF %d:%d" % (nlist, nprobe), ix.search_ivf(Q, keep, nprobe)[1])] if ivf else []):
                ids = to_old(ids)
                out[label] = (lsq.eval_recall(gt, np.ascontiguousarray(ids.T).astype(np.uint32), keep), ids)
            return out
        ix.remove(gone)
        under = curves(None)
        old_of_new = ix.compact()
        after = curves(old_of_new)
        info = ix.compact_info()
    print("Deleted %d of %d rows (Index.remove), then compacted to %d rows (Index.compact, %d bytes moved)" % (gone.shape[0], n, info["n_after"], info["moved_bytes"]))
    print("     r@   " + "   ".join("%-24s" % (k + " tombstones / compact") for k in under))
    for i in (1, 2, 5, 10, 20, 50, 100, 200, 500, 1000):
        if i <= keep:
            print("%7d   " % i + "   ".join("%-.4f / %-15.4f" % (under[k][0][i - 1], after[k][0][i - 1]) for k in under))
    for k in under:
        assert np.array_equal(np.sort(under[k][1], axis=1), np.sort(after[k][1], axis=1)), "%s: the ids after the compact are not the ids under the tombstones" % k
    print("%s: recall@1 after deleting a fraction of %g = %.4f; the answers under tombstones and after the compact name the same rows" % (name, fraction, under["ADC"][0][0]))


def filtered_recall(fraction, name, x_base, x_query, B_base, C, db_norms, m, knn, shortlist, ivf):
    """--filter: the searches over the allowed rows of a seeded random mask, their recall against Index.knn under the same mask"""
    n = x_base.shape[1]
    allowed = np.random.default_rng(0).random(n) < fraction
    rows = np.ascontiguousarray(x_base.T)                                    # f32, or the un-widened bytes of --bvecs
    Q = np.ascontiguousarray(x_query.T.astype(np.float32))
    with lsq.Engine(0) as eng, eng.index((B_base - 1).astype(np.uint8).T, np.ascontiguousarray(np.hstack(C).T), db_norms, m, base=rows) as ix:
        ix.set_filter(mask=allowed)
        info = ix.filter_info()
        keep = max(1, min(knn, info["allowed"]))
        _, truth = ix.knn(Q, 1, id_base=1)                                   # the ground truth: exact k-NN over the allowed rows
        gt = truth[:, 0].astype(np.uint32)
        curves = {}
        _, ids = ix.search(Q, keep)
        curves["ADC"] = lsq.eval_recall(gt, np.ascontiguousarray(ids.T).astype(np.uint32), keep)
        road = {0: "unfiltered", 1: "dense", 2: "compact"}[ix.filter_info()["road"]]
        if shortlist:
            L = min(max(shortlist, keep), n)
            _, ids = ix.search(Q, keep, shortlist=L, Q_exact=Q)
            curves["re-ranked %d" % L] = lsq.eval_recall(gt, np.ascontiguousarray(ids.T).astype(np.uint32), keep)
        if ivf:
            nlist = min(ivf[0], n)
            nprobe = min(ivf[1], nlist)
            cent, assign = lsq.train_coarse(np.asarray(rows, dtype=np.float32), nlist, niter=10, seed=0, engine=eng)
            ix.set_lists(cent, assign)
            _, ids = ix.search_ivf(Q, keep, nprobe)
            curves["IVF %d:%d" % (nlist, nprobe)] = lsq.eval_recall(gt, np.ascontiguousarray(ids.T).astype(np.uint32), keep)
    print("Filtered search (%d of %d rows allowed, %s road; ground truth: exact k-NN under the same mask)" % (info["allowed"], n, road))
    print("     r@   " + "   ".join("%-12s" % k for k in curves))
    for i in (1, 2, 5, 10, 20, 50, 100, 200, 500, 1000):
        if i <= keep:
            print("%7d   " % i + "   ".join("%-12.4f" % c[i - 1] for c in curves.values()))
    print("%s: filtered recall@1 = %.4f at fraction %g" % (name, curves["ADC"][0], fraction))


if __name__ == "__main__":
    main()
