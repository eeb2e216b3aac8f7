"""The inequality the default encoder's exactness rests on, held directly on the device's own numbers.

The 16-bit filtered walk (csrc/lsq_icmq.hip) decides a node update on level sums alone when the runner-up lies outside a window, and the window is
rigorous only if  |C_i + D_j Q[a] - s_f32[a]| <= slack_j  for every vector, node and candidate.  Every other test of the filter checks OUTCOMES (codes
equal to the oracle, the float64 replay, the route counters), and an outcome cannot see an undersized bound: the true argmin would have to land outside
the window, which random data practically never does.  Here the inequality itself is evaluated (tests/q16_bound.py: assertions A-D) on the snapshot the
shipped library leaves behind (lsq_get_q16_snapshot), at the held codes, at random tuples and at adversarial tuples built from the device's own levels --
on every m through the forced filter, on default options above q16_min at d = 128 / 960 and m = 16, on the data kinds, value scales and planted outliers
of the other filter tests, through the host-buffer pipeline (parameters from the sample) and on a partial last chunk (tests/q16_cases.py).

Then the proof that these assertions can fail: one-slip, arithmetic-only copies of the kernel files (tests/q16_mutants.py), each loaded in a child
process of its own; the required ones must be reported by A-D on at least one case.

Set LSQ_Q16_BOUND_OUT to a file name to have the figures of every case (tightness = largest spread / (2 slack) per node, random and adversarial tuples)
and the mutants' table written there, one JSON line each (the place for such a run is profiles/q16_bound.jsonl)."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q16_cases as QC  # noqa: E402
import q16_mutants  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = QC.ROOT


def _record(line):
    print(json.dumps(line))
    path = os.environ.get("LSQ_Q16_BOUND_OUT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


@pytest.mark.parametrize("name", [c["name"] for c in QC.CASES])
def test_bound_holds(lsq, name):
    res = QC.run_case(lsq, QC.BY_NAME[name])
    _record(dict(res, kind="case"))
    QC.judge(res)
    if name == "outliers":
        assert res["filter_f32"] > 0 and res["mild_rows"] > 0                    # flagged pairs took the f32 routine; the unflagged rest was checked in full
    if name == "last_chunk":
        assert res["row0"] == 8192 and res["rows"] == 1808
    if name.startswith("default"):
        assert res["rows"] >= 65536


def test_snapshot_is_refused_without_a_resident_filtered_chunk(lsq):
    import numpy as np
    import torch
    from conftest import make_problem, open_engine
    X, K, B0 = make_problem(16, 600, 4, seed=3, kind="gauss")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    with lsq.Engine(0) as eng:
        with pytest.raises(lsq._lib.LsqError) as e:                            # no encode yet
            eng.q16_snapshot()
        assert e.value.code == lsq._lib.LSQ_EINVAL and "no filtered chunk" in str(e.value)
        eng.encode_icm(X, B0, K, 4, [1], 2, 2, True, seed=1)                     # below q16_min: the wave kernel
        with pytest.raises(lsq._lib.LsqError):
            eng.q16_snapshot()
    with open_engine(lsq, QC.FORCED) as eng:
        Bs, _ = eng.encode_icm(X, B0, K, 4, [1], 2, 2, True, seed=1)
        snap = eng.q16_snapshot()
        assert snap["rows"] == 600 and snap["row0"] == 0 and snap["m"] == 4 and snap["filtered"]
        L, h = eng._L, eng._h
        small = torch.empty(16, dtype=torch.int16, device="cuda:0")
        assert L.lsq_get_q16_snapshot(h, lsq._lib.SNAP_UQ, small.data_ptr(), 32, None) == lsq._lib.LSQ_EINVAL      # too small
        assert L.lsq_get_q16_snapshot(h, 6, small.data_ptr(), 32, None) == lsq._lib.LSQ_EINVAL                     # unknown item
        assert L.lsq_get_q16_snapshot(h, -1, small.data_ptr(), 32, None) == lsq._lib.LSQ_EINVAL
        # host destination, and the same bytes as the device copy
        host = np.empty(600, dtype=np.uint16)
        assert L.lsq_get_q16_snapshot(h, lsq._lib.SNAP_QFLAG, host.ctypes.data, host.nbytes, None) == 0
        eng.synchronize()
        assert np.array_equal(host, snap["qflag"].cpu().numpy().view(np.uint16))
        # the getter changes no result: the same call again gives the same codes, and the snapshot the same bytes
        Bs2, _ = eng.encode_icm(X, B0, K, 4, [1], 2, 2, True, seed=1)
        again = eng.q16_snapshot()
        assert np.array_equal(Bs, Bs2) and all(torch.equal(snap[k], again[k]) for k in ("Uq", "Tq", "qflag", "U", "T"))
        eng.get_unaries(X, K, 4)                                                 # rebuilds the unaries row-major: the snapshot is gone
        with pytest.raises(lsq._lib.LsqError):
            eng.q16_snapshot()
        eng.encode_icm_dev(dev(X), dev((B0 - 1).astype(np.uint8)), dev(K), 4, [1], 2, 2, True, seed=1, nonblocking=True)
        torch.cuda.synchronize()
        with pytest.raises(lsq._lib.LsqError):                                   # option "async": the verdict stayed on the device
            eng.q16_snapshot()


def _child(lib_path, cases, timeout=600):
    env = dict(os.environ, LSQ_LIB_PATH=lib_path)
    env.pop("LSQ_Q16_BOUND_OUT", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "q16_cases.py"), "--run"] + list(cases), env=env, capture_output=True, text=True,
                       timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("Q16_CASES_RESULT ")]
    if p.returncode != 0 or len(lines) != 1:
        pytest.fail("the child on %s ended abnormally (exit status %d); nothing is retried\n%s" % (lib_path, p.returncode, (p.stdout + p.stderr)[-3000:]), pytrace=False)
    return json.loads(lines[0][len("Q16_CASES_RESULT "):])


def test_every_required_mutant_is_reported(lsq):
    """Each one-slip copy of lsq_icmq.hip / lsq_gemm.hip in a child process of its own, one after another, each once."""
    mdir = os.path.join(os.path.dirname(lsq._lib.LIB_PATH), "csrc", "build", "mutants")
    missed = []
    for name, fname, _, _, required in q16_mutants.MUTANTS:
        path = os.path.join(mdir, "liblsq_%s.so" % name)
        assert os.path.exists(path), "%s is not built (make -C local-search-quantization_amd/csrc)" % path
        res = _child(path, QC.MUTANT_CASES)
        assert res["lib"] == path
        killed = {c["case"]: sorted({v[0] for v in c["violations"]}) for c in res["cases"] if c["violations"]}
        tight = {c["case"]: round(max(c["tight_random"] + c["tight_adversarial"]), 4) for c in res["cases"]}
        _record(dict(kind="mutant", mutant=name, file=fname, required=required, reported_by=killed, largest_tightness=tight))
        if required and not killed:
            missed.append((name, tight))
    assert not missed, "mutants that assertions A-D report on no case (largest spread / (2 slack) per case): %r" % missed
