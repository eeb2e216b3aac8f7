"""The cases of tests/test_gpu_q16_bound.py and their driver: one encode through the shipped library on the route the case names (asserted through the
context's counters), the snapshot the encode left behind (Engine.q16_snapshot), assertion C of tests/q16_bound.py on EVERY row of the chunk and A, B, D
on a seeded sample of rows plus the tile edges.  Nothing here touches a GPU at import.

    python tests/q16_cases.py --run NAME [NAME ...]     the cases on the library LSQ_LIB_PATH names -> one JSON line (the mutants' child processes)
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import q16_bound as QB  # noqa: E402

H = 256
SAMPLED_ROWS = 256
FORCED = dict(schedule=6, q16_min=0, light=0, filter_probe_div=0, filter_fallback_div=0)          # conftest's s6_forced
FILTER = dict(schedule=6, q16_min=0, light=0, filter_probe_div=0)                                 # ... with the product's cap on flagged pairs in force
FALLBACK_DIV = 64                                                                                 # the product's default filter_fallback_div


def _case(name, n, d, m, kind="gauss", options=None, entry="dev", chunk=None, scale=None, device_data=None, plant=None, seed=None, K_scale=None):
    return dict(name=name, n=n, d=d, m=m, kind=kind, options=FORCED if options is None else options, entry=entry, chunk=chunk, scale=scale,
                device_data=device_data, plant=plant, seed=sum(map(ord, name)) if seed is None else seed, K_scale=K_scale)


CASES = [_case("forced_m%d" % m, 3000 + 7 * m, 32, m) for m in range(1, 17)] + [
    # default options, one resident chunk above q16_min: the flagship shape, long vectors (the d > 256 shift kernel, Kd = 960 in the epilogue), m = 16
    _case("default_d128_m8", 66_000, 128, 8, options={}, device_data=1.0),
    _case("default_d960_m8", 66_000, 960, 8, options={}, device_data=0.3 / 255.0),
    _case("default_d64_m16", 66_000, 64, 16, options={}, device_data=1.0),
    # the data kinds of test_gpu_icm_f64.problem
    _case("sift", 4000, 32, 8, kind="sift"), _case("gauss", 4000, 32, 8), _case("offset", 4000, 32, 8, kind="offset"), _case("dup", 4000, 32, 8, kind="dup"),
    # a common component 2000 x the data's scale (values near 10^6, ranges near 10^3): the f32 rounding terms of the slack (eps) outweigh its level terms
    _case("offset_far", 4000, 32, 8, kind="offset_far"),
    # the value scales of tools/fuzz_filter.py
    _case("scale_1e-6", 4000, 32, 8, scale=1e-6), _case("scale_1e6", 4000, 32, 8, scale=1e6),
    # planted outliers in panels the range sample does not read (tests/test_gpu_staged.py): far ones (x 6: beyond 16 bits) and mild ones (x 1.2 .. 1.8:
    # a level above hiq that still fits 16 bits), table ranges comparable to the unary's (K x 2.5) so that hiq sits well below 65535
    _case("outliers", 40_000, 16, 8, options=FILTER, plant=dict(far=40, mild=500), K_scale=2.5),
    # the host-buffer entry point through the panel pipeline: parameters from the uploaded sample, |sigma| bound checked panel by panel
    _case("host_sample", 40_000, 32, 8, kind="sift", options=dict(FILTER, upload_pipeline_min_bytes=1, upload_panel_bytes=4 * 32 * 128 * 37), entry="host",
          plant=dict(far=40, mild=0)),
    # several chunks: the last one partial, starting at a non-zero row
    _case("last_chunk", 10_000, 32, 8, chunk=4096),
]
BY_NAME = {c["name"]: c for c in CASES}
# what every mutant of tests/q16_mutants.py is run on
MUTANT_CASES = ["forced_m1", "forced_m2", "forced_m4", "forced_m6", "forced_m8", "forced_m16", "offset", "offset_far", "outliers"]
MUTANT_PAIR_SUBSET = 64                                                                           # a wider pair search than the suite's 16: the children are few


def _planted_rows(n, count, parity, seed):
    """`count` rows of the 128-row panels of one parity (the range sample of a 40 000-vector chunk reads every other panel)"""
    rng = np.random.default_rng(seed)
    pool = np.array([i for i in rng.choice(n, size=min(n, 8 * count + 64), replace=False) if (i // 128) % 2 == parity])
    assert pool.size >= count
    return np.sort(pool[:count])


def build(case):
    """-> dict(X, K, B0 (0-based u8), far, mild): host arrays, or device tensors when the case generates its data on the device"""
    from test_gpu_icm_f64 import problem
    n, d, m, seed = case["n"], case["d"], case["m"], case["seed"]
    if case["kind"] == "offset_far":
        X, K, B0 = problem("gauss", n, d, m, seed)
        u = np.random.default_rng(seed).standard_normal(d).astype(np.float32)
        u /= np.linalg.norm(u)
        X, K = X + np.float32(2000.0) * u, K + np.float32(2000.0 / m) * u
    else:
        X, K, B0 = problem(case["kind"], n, d, m, seed)
    if case["scale"]:
        X, K = X * np.float32(case["scale"]), K * np.float32(case["scale"])
    if case["K_scale"]:
        K = K * np.float32(case["K_scale"])
    far = mild = np.zeros(0, dtype=np.int64)
    if case["plant"]:
        X = X.copy()
        far = _planted_rows(n, case["plant"]["far"], 1, seed)
        X[far] *= np.float32(6.0)
        if case["plant"]["mild"]:
            rows = np.setdiff1d(_planted_rows(n, 3 * case["plant"]["mild"] + 40, 1, seed + 1), far)[:3 * case["plant"]["mild"]]
            for part, s in zip(np.array_split(rows, 3), (1.2, 1.45, 1.8)):
                X[part] *= np.float32(s)
            mild = rows
    return dict(X=np.ascontiguousarray(X, np.float32), K=np.ascontiguousarray(K, np.float32), B0=(B0 - 1).astype(np.uint8), far=far, mild=mild)


def sample_rows(cn, seed, count=SAMPLED_ROWS):
    """`count` seeded rows plus the edges of the GEMM's 128-row tiles (0, 127, 128, the last row)"""
    r = {0, cn - 1} | {i for i in (127, 128) if i < cn}
    r |= set(np.random.default_rng(seed).choice(cn, size=min(cn, count), replace=False).tolist())
    return np.array(sorted(r))


def run_case(lsq, case, sampled=SAMPLED_ROWS, pair_subset=16):
    """-> dict: the case's reports and figures (nothing asserted here but the route and the snapshot's own consistency; the caller judges `violations`)"""
    import torch
    from conftest import open_engine
    n, d, m = case["n"], case["d"], case["m"]
    t_all = time.time()
    with open_engine(lsq, case["options"], **({"chunk": case["chunk"]} if case["chunk"] else {})) as eng:
        far = mild = np.zeros(0, dtype=np.int64)
        if case["device_data"] is not None:
            dX = eng.synth_data_u8_dev(1000 + case["seed"], n, d)
            dK = eng.synth_codebooks_dev(2000 + case["seed"], m, d)
            if case["device_data"] != 1.0:
                dX.mul_(case["device_data"])
                dK.mul_(case["device_data"])
            dB0 = eng.randinit_dev(7, n, m)
        else:
            inp = build(case)
            far, mild = inp["far"], inp["mild"]
            if case["entry"] == "dev":
                dX, dK, dB0 = (torch.from_numpy(inp[k]).to("cuda:0") for k in ("X", "K", "B0"))
        eng.reset_timings()
        t_enc = time.time()
        if case["entry"] == "dev":
            dBs, _, _ = eng.encode_icm_dev(dX, dB0, dK, m, [1], 2, 4, True, seed=case["seed"])
            torch.cuda.synchronize()
            codes = dBs[0]
        else:
            Bs, _ = eng.encode_icm(inp["X"], inp["B0"].astype(np.int16) + 1, inp["K"], m, [1], 2, 4, True, seed=case["seed"])
            codes = torch.from_numpy((Bs[0] - 1).astype(np.uint8))
        t_enc = time.time() - t_enc
        t = eng.timings()
        # the route: the filtered walk produced the codes of this chunk, no chunk was handed to the f32 walk
        assert t["filtered_blocks"] > 0 and t["staged_blocks"] == 0 and t["filter_fallback_chunks"] == 0, (case["name"], t)
        if case["options"].get("light") == 0:
            assert t["light_blocks"] == 0, (case["name"], t)
        snap = eng.q16_snapshot()
        cn, row0, par = snap["rows"], snap["row0"], snap["params"]
        per = case["chunk"] or n
        assert snap["filtered"] and snap["m"] == m and (snap["slq"], snap["slf"]) == QB.slice_widths(m), snap
        assert row0 == (n - 1) // per * per and cn == n - row0, (case["name"], row0, cn)      # the LAST chunk of the call
        # C on every row: the whole u16 planes come to the host; A, B, D on the sampled rows, gathered on the device
        Uq, Tq, qflag = (snap[k].cpu().numpy().view(np.uint16) for k in ("Uq", "Tq", "qflag"))
        rows = sample_rows(cn, case["seed"], sampled)
        if far.size or mild.size:                                  # ... and some of the planted rows: where they are not flagged they are the widest unaries the filter keeps
            rows = np.unique(np.concatenate([rows, (mild - row0)[:64], (far - row0)[:8]]))
        idx = torch.from_numpy(rows).to(snap["U"].device)
        U_rows = snap["U"].index_select(2, idx).cpu().numpy()
        T = snap["T"].cpu().numpy()
        held = codes[row0:row0 + cn].to("cpu").numpy().astype(np.int64)
        after = eng.timings()
    assert all(after[k] == t[k] for k in t if not k.endswith("_ms")), "the getter moved a counter"
    t_chk = time.time()
    crep, nflag = QB.check_carry(m, par, Uq, Tq, qflag, snap["slq"])
    sn = QB.Snapshot(m, par, Uq[:, :, rows, :], Tq, qflag[rows], U_rows, T, rows=rows, slq=snap["slq"], slf=snap["slf"])
    rep = QB.check_rows(sn, held[rows], seed=case["seed"], pair_subset=pair_subset)
    rep.merge(crep)
    t_chk = time.time() - t_chk
    flags = qflag.astype(np.int64)
    sampled_flagged = int(sum(np.count_nonzero((flags[rows] >> j) & 1) for j in range(m)))
    out = dict(case=case["name"], n=n, d=d, m=m, rows=cn, row0=row0, sampled_rows=int(rows.size), sampled_flagged_pairs=sampled_flagged,
               pairs_checked=int(rep.pairs_checked),
               tuples_checked=int(rep.tuples_checked), flagged_pairs=int(nflag), flagged_share=nflag / float(cn * m), params_nflag=int(par["nflag"]),
               params_ok=int(par["ok"]), window=par["window"].tolist(), slack_over_D=(par["slack"] / par["D"].astype(np.float64)).tolist(),
               hiq=par["hiq"].tolist(), tight_random=rep.tight_random.tolist(), tight_adversarial=rep.tight_adversarial.tolist(),
               filter_refined=int(t["filter_refined"]), filter_f32=int(t["filter_f32"]), node_updates=int(t["icm_node_updates"]),
               far_rows=int(far.size), far_rows_flagged=int(np.count_nonzero(flags[far - row0] != 0)) if far.size else 0,
               mild_rows=int(mild.size), mild_rows_flagged=int(np.count_nonzero(flags[mild - row0] != 0)) if mild.size else 0,
               violations=[[v[0], int(v[1]), v[2][:300]] for v in rep.violations], encode_s=round(t_enc, 3), check_s=round(t_chk, 3),
               total_s=round(time.time() - t_all, 3))
    return out


def judge(res):
    """the assertions of one case on the shipped library"""
    what = res["case"]
    assert res["params_ok"] == 1, what
    assert res["flagged_pairs"] == res["params_nflag"], "%s: %d pairs carry a flag, the chunk's verdict counted %d" % (what, res["flagged_pairs"], res["params_nflag"])
    # a flagged pair is excluded from A-C: at most the share above which the product itself would not run the filter on the chunk
    assert res["flagged_pairs"] * FALLBACK_DIV <= res["rows"] * res["m"], "%s: %d of %d pairs are flagged" % (what, res["flagged_pairs"], res["rows"] * res["m"])
    assert res["far_rows_flagged"] == res["far_rows"], "%s: %d of the %d planted rows are flagged" % (what, res["far_rows_flagged"], res["far_rows"])
    # every unflagged pair of the sampled rows went through A and B
    assert res["pairs_checked"] == res["sampled_rows"] * res["m"] - res["sampled_flagged_pairs"] and res["sampled_rows"] >= min(res["rows"], SAMPLED_ROWS), what
    assert res["violations"] == [], "%s: %d violations of the filter's bound, the first: %r" % (what, len(res["violations"]), res["violations"][:4])
    assert max(res["tight_random"] + res["tight_adversarial"]) <= 1.0, what


def main(argv):
    if len(argv) < 2 or argv[0] != "--run":
        raise SystemExit(__doc__)
    import importlib
    lsq = importlib.import_module("local-search-quantization_amd")
    out = [run_case(lsq, BY_NAME[name], pair_subset=MUTANT_PAIR_SUBSET) for name in argv[1:]]
    print("Q16_CASES_RESULT " + json.dumps({"lib": lsq._lib.LIB_PATH, "cases": out}))


if __name__ == "__main__":
    main(sys.argv[1:])
