"""One-slip copies of the kernel files behind the 16-bit filter's error bound: the proof that tests/test_gpu_q16_bound.py can fail.

Each mutant is ONE exact-string replacement in csrc/lsq_icmq.hip or csrc/lsq_gemm.hip that changes ARITHMETIC only -- a coefficient of the slack, a term of
it, the window taken from it, the level above which the GEMM epilogue flags a pair -- and leaves every pointer, size, bound, loop condition and launch
geometry as shipped: a mutant can publish an undersized bound or an unflagged level and nothing else.  The Makefile's `mutants` rule writes each copy under
csrc/build/mutants/, compiles that one file and links it with the shipped objects into build/mutants/liblsq_<name>.so; the GPU test loads each through
LSQ_LIB_PATH in a child process of its own (tests/q16_cases.py --run).

`required`: assertions A-D of tests/q16_bound.py must report the mutant on at least one case of MUTANT_CASES (tests/test_gpu_q16_bound.py); for the others
the test records which case reports it.

    python q16_mutants.py --names                  the names, one line
    python q16_mutants.py --names FILE             the names of the mutants of FILE
    python q16_mutants.py --emit NAME SRC DST      write the mutated copy of SRC to DST
"""
import sys

SLACK = "        const double slack = (double)m * (0.5 + 1.0 / 32.0) * D + eps + 65535.0 * D * 2.384185791015625e-7;"

# (name, file, old, new, required)
MUTANTS = [
    # the per-term level error (0.5 + 2^-5) D of the slack: halved ...
    ("q16_slack_coefficient_quarter", "lsq_icmq.hip", SLACK, SLACK.replace("(0.5 + 1.0 / 32.0)", "0.25"), True),
    # ... and just below the half step a rounded level really errs by
    ("q16_slack_coefficient_047", "lsq_icmq.hip", SLACK, SLACK.replace("(0.5 + 1.0 / 32.0)", "0.47"), True),
    # the window taken from the slack: half of it
    ("q16_window_halved", "lsq_icmq.hip",
     "        nd.window = (w < 30000.0) ? (int)w + 1 : 65535;\n",
     "        nd.window = (w < 30000.0) ? (int)(0.5 * w) + 1 : 65535;\n", True),
    # the GEMM epilogue flags a pair above level 65535 instead of above hiq: a level above hiq stays with the filter (the sum of the m levels may carry)
    ("q16_epilogue_flags_above_65535", "lsq_gemm.hip",
     "            qhi = qp->node[c / h].hiq;\n",
     "            qhi = 65535.0f;\n", True),
    # the f32 rounding terms dropped from the slack
    ("q16_slack_without_eps", "lsq_icmq.hip", SLACK, SLACK.replace(" * D + eps + ", " * D + "), False),
]

NAMES = [m[0] for m in MUTANTS]
FILES = sorted({m[1] for m in MUTANTS})


def mutate(src, name):
    for n, _, old, new, _ in MUTANTS:
        if n == name:
            if src.count(old) != 1:
                raise SystemExit("mutant %s: its `old` string occurs %d times in the source (must be exactly once)" % (name, src.count(old)))
            return src.replace(old, new)
    raise SystemExit("unknown mutant %r" % name)


def file_of(name):
    for n, f, _, _, _ in MUTANTS:
        if n == name:
            return f
    raise SystemExit("unknown mutant %r" % name)


if __name__ == "__main__":
    if sys.argv[1:] == ["--names"]:
        print(" ".join(NAMES))
    elif len(sys.argv) == 3 and sys.argv[1] == "--names":
        print(" ".join(m[0] for m in MUTANTS if m[1] == sys.argv[2]))
    elif len(sys.argv) == 5 and sys.argv[1] == "--emit":
        with open(sys.argv[3]) as f:
            out = mutate(f.read(), sys.argv[2])
        with open(sys.argv[4], "w") as f:
            f.write(out)
    else:
        raise SystemExit(__doc__)
