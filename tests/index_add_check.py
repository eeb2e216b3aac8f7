"""Helpers of tests/test_index_add.py and tests/test_gpu_index_add.py: a problem (the shapes of ivf_check.py, filter_check.py and packed_check.py), its
split into an initial part and a sequence of additions, the builder of the FRESH index over a prefix of the rows -- the yardstick of Identity G: a grown
index answers every call as the fresh index over the same rows does, bit for bit -- and the calls that are compared.

A problem is a dict of numpy arrays over ALL rows: codes (n,m), K, dbn (n,), optionally nc / cb (norm bytes and their table: a packed index; dbn is then
cb[nc]), base (n, >= d) f32 or uint8, cent (nlist,d) / lor (n,) (inverted lists), and the queries Q (nq,d), Qc (coarse)."""
import numpy as np

import ivf_check as ic
import packed_check as PC

H = 256
STATS_SCAN = ("exhaustive", "threshold_rank", "list_capacity", "candidates", "fallback_queries")
STATS_IVF = ("probed_rows", "records", "threshold_queries", "fallback_queries")
STATS_FILTER = ("n", "allowed", "lists_without_allowed")


def t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to_np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def problem(n, m, d, nq, seed, nlist=0, packed=False, base=None, lists="skewed"):
    """base: None, "f32" or "u8" (rows of d elements; u8: the codes' reconstruction has nothing to do with them, the searches do not care)"""
    codes, K, dbn, cent, lor, Qs, Qc = ic.problem(n, d, m, max(nlist, 1), nq, seed, lists=lists)
    P = {"codes": codes, "K": K, "dbn": dbn, "Q": Qs, "Qc": Qc, "m": m, "d": d, "n": n}
    if nlist:
        P["cent"], P["lor"] = cent, lor
    if packed:
        cb, nc = PC.quantize(dbn)
        P["cb"], P["nc"], P["dbn"] = cb, nc, cb[nc]
    rng = np.random.default_rng(seed + 7)
    if base == "f32":
        P["base"] = rng.standard_normal((n, d)).astype(np.float32)
    elif base == "u8":
        P["base"] = rng.integers(0, 256, (n, d)).astype(np.uint8)
        P["Qb"] = rng.integers(0, 256, (nq, d)).astype(np.uint8)     # queries of the base's own type: the integer road of knn (d <= 258)
    return P


def cuts(n0, adds):
    """[(lo, hi)] of the additions after the first n0 rows"""
    out, lo = [], n0
    for a in adds:
        out.append((lo, lo + a))
        lo += a
    return out


def fresh(engine, P, n, dev=False, lists=True, codes=True, base=True):
    """the index a caller builds today over rows [0, n): created over the arrays, set_lists over the same centroids and the rows' lists"""
    conv = t if dev else (lambda a: np.ascontiguousarray(a))
    b = conv(P["base"][:n]) if base and "base" in P else None
    if not codes:
        ix = (engine.index_dev if dev else engine.index)(None, None, None, 0, base=b, d=P["d"])
    elif "nc" in P:
        ix = (engine.index_packed_dev if dev else engine.index_packed)(conv(P["codes"][:n]), conv(P["K"]), conv(P["nc"][:n]), conv(P["cb"]), P["m"], base=b)
    else:
        ix = (engine.index_dev if dev else engine.index)(conv(P["codes"][:n]), conv(P["K"]), conv(P["dbn"][:n]), P["m"], base=b)
    if lists and codes and "cent" in P:
        ix.set_lists(conv(P["cent"]), conv(P["lor"][:n]))
    return ix


def add_args(P, lo, hi, ix, dev=False, base_view=None):
    """Index.add's keyword arguments for rows [lo, hi) of the problem, as numpy arrays or device tensors; base_view: the base rows laid out otherwise"""
    conv = t if dev else (lambda a: np.ascontiguousarray(a))
    kw = {}
    if ix._has_codes:
        kw["codes"] = conv(P["codes"][lo:hi])
        if ix._packed:
            kw["norm_codes"] = conv(P["nc"][lo:hi])
        else:
            kw["dbnorms"] = conv(P["dbn"][lo:hi])
        if getattr(ix, "nlist", 0):
            kw["assign"] = conv(P["lor"][lo:hi])
    if ix._has_base:
        kw["base"] = base_view if base_view is not None else conv(P["base"][lo:hi])
    return kw


def grow(ix, P, lo, hi, dev=False, base_view=None):
    ix.add(**add_args(P, lo, hi, ix, dev, base_view))


def bits(a):
    a = np.ascontiguousarray(to_np(a))
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want):
    """(dists, ids) equal bit for bit: NaN payloads, signed zeros and padding records included"""
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def call(ix, method, Q, *args, **kw):
    """an Index search method with numpy arguments on either kind of index -> numpy (dists, ids)"""
    if ix._dev:
        Q = t(Q)
        kw = {k: (t(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    d, i = getattr(ix, method)(Q, *args, **kw)
    return to_np(d), to_np(i)


def pick(info, keys):
    return {k: info[k] for k in keys}


def answers(ix, P, nns=(10,), nprobes=(), shortlist=0, knn=False, flags=0):
    """every call of the comparison on one index -> {label: ((dists, ids), deterministic statistics)}"""
    out = {}
    if ix._has_codes:
        for nn in nns:
            if nn <= ix.n:
                out["search", nn] = (call(ix, "search", P["Q"], nn), pick(ix.scan_stats(), STATS_SCAN))
        if shortlist and ix._has_base:
            out["search-shortlist"] = (call(ix, "search", P["Q"], min(nns), shortlist=shortlist), None)
        for nprobe in nprobes:
            for every in (False, True):
                for add in (False, True):
                    nn = min(nns)
                    out["ivf", nprobe, every, add] = (call(ix, "search_ivf", P["Q"], nn, nprobe, Q_coarse=P["Qc"], every_record=every, add_coarse=add,
                                                           flags=flags), pick(ix.ivf_info(), STATS_IVF))
    if knn and ix._has_base:
        nn = min(min(nns), ix.n)
        out["knn-f32"] = (call(ix, "knn", P["Q"], nn), pick(ix.knn_info(), ("rows", "exhaustive", "int_road", "fallback_queries")))      # u8 rows: widened
        if "Qb" in P:
            out["knn-u8"] = (call(ix, "knn", P["Qb"], nn), pick(ix.knn_info(), ("rows", "exhaustive", "int_road", "fallback_queries")))
        cand = np.ascontiguousarray((np.arange(P["Q"].shape[0] * 2 * nn).reshape(-1, 2 * nn) * 7) % (ix.n + 3), dtype=np.int32)      # some ids outside the base
        out["rerank"] = (call(ix, "rerank", P["Q"], cand=cand, k=nn, id_base=0), None)
    out["filter"] = (((), ()), pick(ix.filter_info(), STATS_FILTER))
    return out


def equal_answers(got, want):
    """-> the labels at which two answers() differ (empty: Identity G holds on them)"""
    assert got.keys() == want.keys(), (sorted(map(str, got)), sorted(map(str, want)))
    return [k for k in got if not same(got[k][0], want[k][0]) or got[k][1] != want[k][1]]
