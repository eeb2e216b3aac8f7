"""One-slip copies of csrc/lsq_api.hip: the proof that the context walk of tests/test_gpu_ctx_state.py can fail.

Each mutant is ONE exact-string replacement that leaves a stale value behind -- a flag not cleared, a counter not advanced or advanced twice, a cache
not invalidated -- and every pointer, size, bound and launch geometry as shipped: a mutant can return wrong numbers and nothing else.  The Makefile's
`mutants` rule writes each copy under csrc/build/mutants/, compiles that one file and links it with the shipped objects into
build/mutants/liblsq_<name>.so; the GPU test loads each through LSQ_LIB_PATH in a child process of its own.

`pair` is the consecutive (previous entry, entry) of the fixed-shape mutant sequence (ctx_ops.mutant_sequence) at which the walk must report a mismatch,
`profile` the option profile it happens under.

    python ctx_mutants.py --names                  the names, one line
    python ctx_mutants.py --emit NAME SRC DST      write the mutated copy of SRC to DST
"""
import sys

# (name, old, new, profile, pair)
MUTANTS = [
    # the host-table cache (hostK / tables_valid), site 1: claim_sK, the one place where a host-buffer call takes sK for other codebooks
    # (the name is that of the helper that held the line before claim_sK: the built copies and their reports are known by it)
    ("upload_xk_keeps_tables_valid",
     "    c->tables_valid = false;        // sK is about to hold other codebooks than the cached tables were built from\n",
     "    // (mutant) sK is about to hold other codebooks than the cached tables were built from\n",
     "default", ("veccost", "encoding_icm_it")),
    # the host-table cache, site 2: the device assignment overwrites ||c||^2 without touching sK.  Engine's _dev forms rebind the stream around every
    # call, which drops the cache by itself: only a _dev call made on the context's OWN stream (catalogue entry assign_codewords_dev_own) reaches this line
    ("init_codes_dev_keeps_tables_valid",
     "    else {\n        c->tables_valid = false;\n        LSQ_TRY(c->sci.ensure(sizeof(float) * (size_t)m * LSQ_H));\n",
     "    else {\n        LSQ_TRY(c->sci.ensure(sizeof(float) * (size_t)m * LSQ_H));\n",
     "default", ("assign_codewords_dev_own", "encoding_icm_it")),
    # the ILS counter of the CPU-shaped entry points: advanced twice by one call ...
    ("encoding_icm_advances_auto_it_twice",
     "    if (rc == LSQ_OK && autoit && c->auto_it < LSQ_IT_AUTO - 1u) ++c->auto_it;\n    return rc;\n",
     "    if (rc == LSQ_OK && autoit && c->auto_it < LSQ_IT_AUTO - 2u) c->auto_it += 2u;\n    return rc;\n",
     "default", ("encoding_icm_auto", "encoding_icm_auto")),
    # ... and not advanced by the other
    ("encode_icm_fully_keeps_auto_it",
     "    if (autoit && c->auto_it < LSQ_IT_AUTO - 1u) ++c->auto_it;\n    return LSQ_OK;\n",
     "    return LSQ_OK;\n",
     "default", ("encode_icm_fully_auto", "encoding_icm_auto")),
    # the road word of option "async": a blocking call still gated by the device word the async call before it used
    # (the ONE reset of the chunk state, where a chunk's unaries start to be built, carries the old `on_device` over)
    ("q16_verdict_keeps_chunk_road_dev",
     "    c->chunk_road = ChunkRoad{};\n",
     "    c->chunk_road = ChunkRoad{false, c->chunk_road.on_device};\n",
     "s6_forced", ("encode_icm_dev_nb", "encode_icm_dev")),
    # the statistics of option "async": never folded into timings(), wiped by the next call
    ("finish_call_keeps_pending_fold",
     "        c->pending_fold = true;\n        return LSQ_OK;\n",
     "        return LSQ_OK;\n",
     "default", ("encoding_icm_it", "encode_icm_dev_nb")),
    # the filtered walk's 16-bit slice tables: not rebuilt after the pair tables changed
    ("prepare_tables_keeps_tables_changed",
     "    Timer t(c, CAT_TABLES);\n    c->tables_changed = 1;\n",
     "    Timer t(c, CAT_TABLES);\n",
     "s6_forced", ("encoding_icm_it", "encode_icm_dev")),
]

NAMES = [m[0] for m in MUTANTS]


def mutate(src, name):
    for n, old, new, _, _ in MUTANTS:
        if n == name:
            if src.count(old) != 1:
                raise SystemExit("mutant %s: its `old` string occurs %d times in the source (must be exactly once)" % (name, src.count(old)))
            return src.replace(old, new)
    raise SystemExit("unknown mutant %r" % name)


if __name__ == "__main__":
    if sys.argv[1:] == ["--names"]:
        print(" ".join(NAMES))
    elif len(sys.argv) == 5 and sys.argv[1] == "--emit":
        with open(sys.argv[3]) as f:
            out = mutate(f.read(), sys.argv[2])
        with open(sys.argv[4], "w") as f:
            f.write(out)
    else:
        raise SystemExit(__doc__)
