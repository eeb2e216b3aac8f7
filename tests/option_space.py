"""The option table of the encoder and a covering array over it (plain Python, no GPU).

README: "All schedules and option values give bit-identical codes."  The options interact in run_sweeps (csrc/lsq_api.hip): which kernel a chunk takes
depends on schedule x q16_min x chunk x wave_max x light, how its node sequence is cut on per_node and on the filter probe, which memoisation rules run on
skip x fallback, and the entry point decides who takes the chunk's verdict (the host, or -- async -- a one-thread kernel).  Testing every combination is
3 * 2 * 2 * 4 * 3 * 3 * 2 * 2 * 3 * 3 * 2 * 5 = 155 520 encodes; a PAIRWISE covering array (every value of every factor next to every value of every other
factor in at least one row) takes a few dozen, and is what tests/test_gpu_option_space.py runs.

FACTORS lists each factor's values, the library's default first.  Values that depend on the problem are symbols: resolve() turns a row into the
`set_option` calls of a problem with n vectors.  EXCLUSIONS lists the value pairs the library rejects: none -- lsq_set_option (csrc/lsq_api.hip) checks each
key's own range only (chunk >= 1, filter_*_div >= 0, schedule in {3, 4, 6}) and accepts every value of this table whatever the other options are; options that
do not apply to the road a chunk takes (per_node on the f32 walks, wave_max on the filtered walk, ...) are ignored there, not refused.  The generator honours
an exclusion list all the same (tests/test_option_space.py drives it with one), so that a future rejection is one line here.
"""
from collections import OrderedDict
from itertools import combinations

FACTORS = OrderedDict([
    ("schedule", (6, 4, 3)),
    ("skip", (1, 0)),
    ("fallback", (1, 0)),
    ("light", (-1, 0, 64, 280)),
    ("wave_max", (64, 0, 280)),
    ("q16_min", (65536, 0, "above_n")),                 # above_n: n + 1 -- schedule 6 never reaches the filtered walk
    ("chunk", ("default", "third")),                    # third: n // 3 + 1 -- three resident chunks, the last one short
    ("per_node", (0, 1)),
    ("filter_probe_div", (8, 0, 1)),
    ("filter_fallback_div", (64, 0, 1)),
    ("profile", (0, 1)),
    ("entry", ("host_f32", "dev_f32", "dev_async", "host_u8", "dev_u8")),
])

# ((factor, value), (factor, value)) pairs that must not meet in a row, each with the line that rejects it.  The library rejects none (see above).
EXCLUSIONS = ()

MAX_ROWS = 60


def _norm(pair):
    (fa, va), (fb, vb) = pair
    return ((fa, va), (fb, vb)) if fa <= fb else ((fb, vb), (fa, va))


def all_pairs(factors=FACTORS, exclusions=EXCLUSIONS):
    """every pair of values of every two factors, minus the excluded ones"""
    out = set()
    for fa, fb in combinations(factors, 2):
        for va in factors[fa]:
            for vb in factors[fb]:
                out.add(_norm(((fa, va), (fb, vb))))
    return out - {_norm(p) for p in exclusions}


def row_pairs(row):
    return {_norm(((fa, row[fa]), (fb, row[fb]))) for fa, fb in combinations(row, 2)}


def covering_array(factors=FACTORS, exclusions=EXCLUSIONS):
    """Deterministic greedy pairwise array -> list of rows (OrderedDict factor -> value).  Row 0 is the all-defaults row.  Every further row is seeded with
    the first pair still uncovered (in sorted order), then each remaining factor -- visited in an order rotated by the row number, so that no factor is always
    decided last -- takes the value that covers the most uncovered pairs against the factors already set; ties go to the earlier value (the default first).
    A value that would put an excluded pair into the row is never taken."""
    names = list(factors)
    banned = {_norm(p) for p in exclusions}
    key = lambda p: repr(p)
    uncovered = all_pairs(factors, exclusions)

    def allowed(row, f, v):
        return all(_norm(((f, v), (g, w))) not in banned for g, w in row.items())

    rows = []
    first = OrderedDict((f, factors[f][0]) for f in names)
    if not (row_pairs(first) & banned):
        rows.append(first)
        uncovered -= row_pairs(first)
    while uncovered:
        (fa, va), (fb, vb) = min(uncovered, key=key)
        row = {fa: va, fb: vb}
        k = len(rows) % len(names)
        for f in names[k:] + names[:k]:
            if f in row:
                continue
            best, gain = None, -1
            for v in factors[f]:
                if not allowed(row, f, v):
                    continue
                g = sum(1 for h, w in row.items() if _norm(((f, v), (h, w))) in uncovered)
                if g > gain:
                    best, gain = v, g
            if best is None:
                raise ValueError("no value of %r is allowed next to %r" % (f, row))
            row[f] = best
        row = OrderedDict((f, row[f]) for f in names)
        rows.append(row)
        uncovered -= row_pairs(row)
    return rows


def row_id(row):
    """a short, stable name of a row (the pytest id)"""
    short = {"schedule": "s", "skip": "k", "fallback": "f", "light": "l", "wave_max": "w", "q16_min": "q", "chunk": "c", "per_node": "p",
             "filter_probe_div": "pd", "filter_fallback_div": "fd", "profile": "t", "entry": ""}
    return "-".join("%s%s" % (short[f], v) for f, v in row.items())


def resolve(row, n, default_chunk=256 * 3968):
    """-> (the row's set_option calls for a problem of n vectors, in a fixed order; its entry point)"""
    opts = OrderedDict()
    for f, v in row.items():
        if f == "entry":
            continue
        if f == "q16_min" and v == "above_n":
            v = n + 1
        if f == "chunk":
            v = default_chunk if v == "default" else n // 3 + 1
        opts[f] = int(v)
    return opts, row["entry"]


def takes_filtered_walk(row, n):
    """does a chunk of this row reach the 16-bit filtered walk at all (use_q16 in csrc/lsq_api.hip: schedule 6 and a chunk of at least q16_min vectors)?"""
    opts, _ = resolve(row, n)
    return opts["schedule"] == 6 and min(opts["chunk"], n) >= opts["q16_min"]


def takes_wave_kernel(row, n, per_block):
    """does a chunk of this row run the wave-per-vector-pair kernel (run_sweeps: schedule >= 4, not the filtered walk, not the device-decided road, and at most
    min(light, wave_max) vectors per block; light < 0 stands for the f32 walk's default of 256)?  `per_block`: vectors per block of the chunk."""
    opts, entry = resolve(row, n)
    if opts["schedule"] < 4 or takes_filtered_walk(row, n):
        return False
    light = opts["light"] if opts["light"] >= 0 else 256
    return per_block <= light and per_block <= opts["wave_max"]
