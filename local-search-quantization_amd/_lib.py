"""ctypes binding of liblsq_mi355x.so -- every symbol include/lsq_mi355x.h declares.

There is deliberately NO fallback: if the shared library is missing or a call fails, an
exception is raised.  Build it with `python -c "import __graft_entry__ as g; g.build()"`
(or `make -C local-search-quantization_amd/csrc`).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LSQ_LIB_PATH") or os.path.join(_HERE, "liblsq_mi355x.so")      # override: A/B builds of the same ABI
# Same ABI built with -DLSQ_TUNING: + option "ablation", environment knobs, clock stamps.  Profiling tools and the tests
# that cross-check the earlier schedules load it explicitly (Engine(..., tuning=True)); the product path never does.
TUNING_LIB_PATH = os.environ.get("LSQ_TUNING_LIB_PATH") or os.path.join(_HERE, "liblsq_mi355x_tuning.so")

LSQ_OK, LSQ_EINVAL, LSQ_EHIP, LSQ_ENOMEM, LSQ_ECODE, LSQ_ENODEV = 0, -1, -2, -3, -4, -5
LSQ_EIO, LSQ_EFORMAT = -6, -7          # snapshots (since v2600): a file operation failed; not a (valid) snapshot


class LsqError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("liblsq_mi355x error %d: %s" % (code, msg))
        self.code = code


class _Struct(C.Structure):
    """a struct of the header; as_dict: its fields by name (the statistics and info structs are handed out that way)"""

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Timings(_Struct):
    _fields_ = [("tables_ms", C.c_double), ("unaries_ms", C.c_double), ("perturb_ms", C.c_double),
                ("icm_ms", C.c_double), ("cost_ms", C.c_double), ("other_ms", C.c_double),
                ("icm_launches", C.c_int64), ("icm_node_updates", C.c_int64),
                ("staged_blocks", C.c_int64), ("light_blocks", C.c_int64), ("filtered_blocks", C.c_int64),
                ("filter_refined", C.c_int64), ("filter_exact", C.c_int64), ("filter_f32", C.c_int64),
                ("filter_fallback_chunks", C.c_int64), ("xs_launches", C.c_int64), ("xs_fallback_launches", C.c_int64),
                ("table_reuses", C.c_int64)]


class LinscanStats(_Struct):
    _fields_ = [("queries", C.c_int64), ("codes", C.c_int64), ("candidates", C.c_int64), ("fallback_queries", C.c_int64),
                ("batches", C.c_int64), ("exhaustive", C.c_int64), ("threshold_rank", C.c_int64), ("list_capacity", C.c_int64),
                ("lut_ms", C.c_double), ("sample_ms", C.c_double), ("scan_ms", C.c_double), ("select_ms", C.c_double)]


class IndexDesc(_Struct):
    _fields_ = [("n", C.c_int64), ("d", C.c_int), ("m", C.c_int), ("h", C.c_int), ("codes", C.c_void_p), ("codebooks", C.c_void_p),
                ("dbnorms", C.c_void_p), ("base", C.c_void_p), ("base_u8", C.c_int), ("ldb", C.c_int), ("on_device", C.c_int)]


class IndexKnnInfo(_Struct):
    _fields_ = [("queries", C.c_int64), ("rows", C.c_int64), ("batches", C.c_int64), ("fallback_queries", C.c_int64), ("exhaustive", C.c_int64),
                ("int_road", C.c_int64), ("norms_ms", C.c_double), ("scan_ms", C.c_double), ("select_ms", C.c_double)]


class IndexStats(_Struct):
    _fields_ = [("queries", C.c_int64), ("rows", C.c_int64), ("invalid", C.c_int64), ("batches", C.c_int64),
                ("scan_ms", C.c_double), ("gather_ms", C.c_double), ("select_ms", C.c_double)]


class IvfDesc(_Struct):
    _fields_ = [("nlist", C.c_int), ("centroids", C.c_void_p), ("list_of_row", C.c_void_p), ("on_device", C.c_int)]


class IvfInfo(_Struct):
    _fields_ = [("queries", C.c_int64), ("probed_rows", C.c_int64), ("records", C.c_int64), ("threshold_queries", C.c_int64),
                ("fallback_queries", C.c_int64), ("batches", C.c_int64), ("batch_queries", C.c_int64), ("tail_capacity", C.c_int64),
                ("coarse_ms", C.c_double), ("lut_ms", C.c_double), ("scan_ms", C.c_double), ("select_ms", C.c_double)]


IVF_ADD_COARSE, IVF_EVERY_RECORD, IVF_TEST_BATCH = 1, 2, 4


class IndexPackedDesc(_Struct):
    _fields_ = [("n", C.c_int64), ("d", C.c_int), ("m", C.c_int), ("h", C.c_int), ("codes", C.c_void_p), ("norm_codes", C.c_void_p),
                ("cbnorms", C.c_void_p), ("ncb", C.c_int), ("codebooks", C.c_void_p), ("base", C.c_void_p), ("base_u8", C.c_int), ("ldb", C.c_int),
                ("on_device", C.c_int)]


class IndexPackedInfo(_Struct):
    _fields_ = [("row_bytes", C.c_int64), ("ivf_row_bytes", C.c_int64), ("ncb", C.c_int64), ("dword_rows", C.c_int64), ("resident_bytes", C.c_int64)]


class FilterDesc(_Struct):
    _fields_ = [("form", C.c_int), ("data", C.c_void_p), ("count", C.c_int64), ("id_base", C.c_int), ("flags", C.c_int), ("on_device", C.c_int)]


class FilterInfo(_Struct):
    _fields_ = [("active", C.c_int64), ("n", C.c_int64), ("allowed", C.c_int64), ("lists", C.c_int64), ("lists_without_allowed", C.c_int64),
                ("road", C.c_int64), ("crossover_rows", C.c_int64)]


class IndexAddDesc(_Struct):
    _fields_ = [("count", C.c_int64), ("codes", C.c_void_p), ("dbnorms", C.c_void_p), ("norm_codes", C.c_void_p), ("base", C.c_void_p), ("ldb", C.c_int),
                ("list_of_row", C.c_void_p), ("on_device", C.c_int)]


class IndexGrowthInfo(_Struct):
    _fields_ = [("n", C.c_int64), ("capacity_rows", C.c_int64), ("adds", C.c_int64), ("rows_added", C.c_int64), ("reallocations", C.c_int64),
                ("adopted", C.c_int64), ("merged_rows", C.c_int64), ("append_ms", C.c_double), ("merge_ms", C.c_double), ("filter_ms", C.c_double)]


class IndexCompactDesc(_Struct):
    _fields_ = [("old_of_new", C.c_void_p), ("new_of_old", C.c_void_p), ("id_base", C.c_int), ("flags", C.c_int), ("on_device", C.c_int)]


class IndexCompactInfo(_Struct):
    _fields_ = [("n_before", C.c_int64), ("n_after", C.c_int64), ("removes", C.c_int64), ("rows_tombstoned", C.c_int64), ("compactions", C.c_int64),
                ("rows_dropped", C.c_int64), ("moved_bytes", C.c_int64), ("shrunk", C.c_int64), ("tombstone_ms", C.c_double), ("gather_ms", C.c_double),
                ("layout_ms", C.c_double)]


class IndexReconInfo(_Struct):
    _fields_ = [("rows", C.c_int64), ("invalid", C.c_int64), ("map_rebuilt", C.c_int64), ("map_rebuilds", C.c_int64), ("road", C.c_int64),
                ("calls", C.c_int64), ("map_ms", C.c_double), ("decode_ms", C.c_double)]


class IndexBaseInfo(_Struct):
    _fields_ = [("format", C.c_int64), ("elem_bytes", C.c_int64), ("ldb", C.c_int64), ("owned", C.c_int64), ("resident_bytes", C.c_int64),
                ("to_inf", C.c_int64), ("to_zero", C.c_int64), ("nans", C.c_int64), ("narrow_ms", C.c_double)]


class SnapshotArrays(_Struct):
    _fields_ = [("n", C.c_int64), ("d", C.c_int), ("m", C.c_int), ("h", C.c_int), ("packed", C.c_int), ("ncb", C.c_int), ("base_format", C.c_int),
                ("nlist", C.c_int), ("filter_active", C.c_int), ("filter_force", C.c_int), ("reserved", C.c_int), ("allowed", C.c_int64),
                ("codebooks", C.c_void_p), ("codes", C.c_void_p), ("dbnorms", C.c_void_p), ("norm_codes", C.c_void_p), ("cbnorms", C.c_void_p),
                ("base", C.c_void_p), ("centroids", C.c_void_p), ("list_of_row", C.c_void_p), ("filter_bits", C.c_void_p)]


class SnapshotSection(_Struct):
    _fields_ = [("kind", C.c_int64), ("elem_bytes", C.c_int64), ("offset", C.c_int64), ("bytes", C.c_int64), ("digest", C.c_uint64)]


class SnapshotInfo(_Struct):
    _fields_ = [("format", C.c_int64), ("n", C.c_int64), ("d", C.c_int64), ("m", C.c_int64), ("h", C.c_int64), ("packed", C.c_int64), ("ncb", C.c_int64),
                ("base_format", C.c_int64), ("nlist", C.c_int64), ("has_codes", C.c_int64), ("has_base", C.c_int64), ("filter_active", C.c_int64),
                ("filter_force", C.c_int64), ("allowed", C.c_int64), ("file_bytes", C.c_int64), ("nsections", C.c_int64), ("header_digest", C.c_uint64),
                ("sections", SnapshotSection * 9)]

    def as_dict(self):
        out = {k: getattr(self, k) for k, _ in self._fields_ if k != "sections"}
        out["sections"] = [dict(self.sections[k].as_dict(), name=SNAP_NAMES[self.sections[k].kind]) for k in range(self.nsections)]
        return out


class SnapshotIoInfo(_Struct):
    _fields_ = [("op", C.c_int64), ("bytes", C.c_int64), ("chunks", C.c_int64), ("chunk_bytes", C.c_int64), ("sections", C.c_int64),
                ("host_staging_bytes", C.c_int64), ("derive_ms", C.c_double), ("digest_ms", C.c_double), ("copy_ms", C.c_double), ("file_ms", C.c_double),
                ("total_ms", C.c_double)]


# the sections of a snapshot in file order: LSQ_SNAP_* -> the key of the array in Index.export / snapshot_read / snapshot_write
SNAP_NAMES = {1: "codebooks", 2: "codes", 3: "dbnorms", 4: "norm_codes", 5: "cbnorms", 6: "base", 7: "centroids", 8: "list_of_row", 9: "filter_bits"}
SNAPSHOT_FORMAT = 1
BASE_F32, BASE_U8, BASE_F16, BASE_BF16 = 0, 1, 2, 3       # the format a base_u8 field / argument stands for (LSQ_BASE_F16, LSQ_BASE_BF16)
RECON_ADD_COARSE, RECON_PAD_NAN = 1, 2
RECON_ROAD_DWORD, RECON_ROAD_VEC16, RECON_ROAD_CODE_DWORDS = 1, 2, 4


class RangeInfo(_Struct):
    _fields_ = [("queries", C.c_int64), ("rows_walked", C.c_int64), ("results", C.c_int64), ("max_per_query", C.c_int64), ("batches", C.c_int64),
                ("road", C.c_int64), ("held_bytes", C.c_int64), ("coarse_ms", C.c_double), ("lut_ms", C.c_double), ("count_ms", C.c_double),
                ("fill_ms", C.c_double), ("sort_ms", C.c_double)]


COMPACT_SHRINK = 1
FILTER_BITS, FILTER_BYTES, FILTER_IDS = 0, 1, 2
FILTER_DENY, FILTER_FORCE_DENSE, FILTER_FORCE_COMPACT = 1, 2, 4


class EncoderDesc(_Struct):
    _fields_ = [("d", C.c_int), ("m", C.c_int), ("h", C.c_int), ("codebooks", C.c_void_p), ("on_device", C.c_int), ("chunk", C.c_int64)]


class EncoderInfo(_Struct):
    _fields_ = [("vectors", C.c_int64), ("chunks", C.c_int64), ("beam", C.c_int64), ("unaries_ms", C.c_double), ("beam_ms", C.c_double)]


class PartitionDesc(_Struct):
    _fields_ = [("nlist", C.c_int), ("d", C.c_int), ("centroids", C.c_void_p), ("on_device", C.c_int)]


class PartitionInfo(_Struct):
    _fields_ = [("call", C.c_int64), ("rows", C.c_int64), ("lists_touched", C.c_int64), ("empty_lists", C.c_int64), ("loader_bytes", C.c_int64),
                ("max_list_rows", C.c_int64), ("group_ms", C.c_double), ("kernel_ms", C.c_double)]


PARTITION_ASSIGN, PARTITION_UPDATE, PARTITION_RESIDUALS, PARTITION_CODE_NORMS = 1, 2, 3, 4


class Q16SnapshotNode(_Struct):
    _fields_ = [("loU", C.c_float), ("invD", C.c_float), ("D", C.c_float), ("hiq", C.c_float), ("window", C.c_int32), ("pad_", C.c_int32),
                ("slack", C.c_double)]


class Q16SnapshotParams(_Struct):
    _fields_ = [("ok", C.c_int32), ("oor", C.c_int32), ("nflag", C.c_int32), ("pad_", C.c_int32), ("node", Q16SnapshotNode * 16)]


SNAP_PARAMS, SNAP_UQ, SNAP_TQ, SNAP_QFLAG, SNAP_U, SNAP_T = 0, 1, 2, 3, 4, 5


class Spgl1Params(_Struct):
    _fields_ = [("opt_tol", C.c_double), ("max_iter", C.c_int64)]


class Spgl1Info(_Struct):
    _fields_ = [("status", C.c_int), ("iterations", C.c_int64), ("line_search_trials", C.c_int64), ("f", C.c_double), ("rel_gap", C.c_double),
                ("l1", C.c_double), ("tau", C.c_double), ("nnz_before_threshold", C.c_int64), ("nnz", C.c_int64)]


SPGL1_OPTIMAL, SPGL1_ITERATIONS, SPGL1_LINE_ERROR = 0, 1, 2

_vp, _i, _i64, _u64, _u32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_uint32

# name -> (restype, argtypes).  Pointers are passed as raw addresses (host or device).
SIGNATURES = {
    "lsq_last_error": (C.c_char_p, []),
    "lsq_version": (_i, []),
    "lsq_device_count": (_i, [C.POINTER(_i)]),
    "lsq_create": (_i, [C.POINTER(_vp), _i]),
    "lsq_destroy": (_i, [_vp]),
    "lsq_set_stream": (_i, [_vp, _vp]),
    "lsq_set_option": (_i, [_vp, C.c_char_p, _i64]),
    "lsq_get_timings": (_i, [_vp, C.POINTER(Timings)]),
    "lsq_get_timings_sized": (_i, [_vp, _vp, C.c_size_t]),
    "lsq_get_walk_trace": (_i, [_vp, _vp, _i]),
    "lsq_get_q16_snapshot": (_i, [_vp, _i, _vp, C.c_size_t, _vp]),
    "lsq_reset_timings": (_i, [_vp]),
    "lsq_synchronize": (_i, [_vp]),
    "lsq_multi_create": (_i, [C.POINTER(_vp), _vp, _i]),
    "lsq_multi_destroy": (_i, [_vp]),
    "lsq_multi_set_option": (_i, [_vp, C.c_char_p, _i64]),
    "lsq_multi_encode_icm": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, _i, _i, _i, _i, _u64, _u64, _i, _vp, _vp]),
    "lsq_encode_icm": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, _i, _i, _i, _i, _i, _u64, _u64, _i, _vp, _vp]),
    "lsq_encode_icm_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, _i, _i, _i, _i, _u64, _u64, _vp, _vp, _vp]),
    # 8-bit data rows (since v1300): the argument lists of the three calls above, X as uint8
    "lsq_encode_icm_u8": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, _i, _i, _i, _i, _i, _u64, _u64, _i, _vp, _vp]),
    "lsq_encode_icm_u8_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, _i, _i, _i, _i, _u64, _u64, _vp, _vp, _vp]),
    "lsq_multi_encode_icm_u8": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, _i, _i, _i, _i, _u64, _u64, _i, _vp, _vp]),
    "lsq_encoding_icm": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _i, _i, _i, _u64, _u32, _u64, _vp]),
    "lsq_encode_icm_fully": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _i, _i, _i, _i64, _u64, _u32]),
    "lsq_get_unaries": (_i, [_vp, _vp, _vp, _i, _i64, _i, _i, _vp]),
    "lsq_get_binaries": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "lsq_veccost": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp]),
    "lsq_qerror": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, C.POINTER(C.c_double)]),
    "lsq_perturb": (_i, [_vp, _vp, _i64, _i, _i, _i, _u64, _u32, _u64]),
    "lsq_randinit": (_i, [_u64, _u64, _i64, _i, _i, _vp]),
    "lsq_node_order": (_i, [_u64, _u32, _i, _i, _vp]),
    "lsq_splitarray": (_i, [_i64, _i, _i, C.POINTER(_i64), C.POINTER(_i64)]),
    "lsq_linscan_aqd_query_extra_byte": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i]),
    "lsq_linscan": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i]),
    "lsq_linscan_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i]),
    "lsq_multi_linscan": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i]),
    "lsq_get_linscan_stats": (_i, [_vp, C.POINTER(LinscanStats)]),
    "lsq_linscan_aqd_query": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _u32, _i, _i, _i, _i, _i]),
    "lsq_linscan_pq": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _u32, _i, _i, _i, _i, _i]),
    "lsq_linscan_pq_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _u32, _i, _i, _i, _i, _i]),
    "lsq_knn_exact_cpu": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i]),
    "lsq_knn_exact": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i]),
    "lsq_knn_exact_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i]),
    # two-stage search (since v1400): the host checker of the re-rank, and the resident index
    "lsq_rerank_cpu": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "lsq_index_create": (_i, [C.POINTER(_vp), _vp, C.POINTER(IndexDesc)]),
    "lsq_index_destroy": (_i, [_vp]),
    "lsq_index_search": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "lsq_index_rerank": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i]),
    "lsq_index_get_stats": (_i, [_vp, C.POINTER(IndexStats)]),
    "lsq_index_knn": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i]),
    "lsq_index_get_knn_info": (_i, [_vp, C.POINTER(IndexKnnInfo)]),
    "lsq_knn_exact_u8_cpu": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i]),
    # inverted lists on the index (since v1700), and their host checker
    "lsq_index_set_lists": (_i, [_vp, C.POINTER(IvfDesc)]),
    "lsq_index_search_ivf": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i]),
    "lsq_index_get_ivf_info": (_i, [_vp, C.POINTER(IvfInfo)]),
    "lsq_ivf_search_cpu": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i]),
    # the packed index: rows of m code bytes and one norm byte (since v1800), and the selection statistics of an index's last scan
    "lsq_index_create_packed": (_i, [C.POINTER(_vp), _vp, C.POINTER(IndexPackedDesc)]),
    "lsq_index_get_packed_info": (_i, [_vp, C.POINTER(IndexPackedInfo)]),
    "lsq_index_get_scan_stats": (_i, [_vp, C.POINTER(LinscanStats)]),
    "lsq_index_set_filter": (_i, [_vp, C.POINTER(FilterDesc)]),
    "lsq_index_get_filter_info": (_i, [_vp, C.POINTER(FilterInfo)]),
    # appending rows to the index (since v2100)
    "lsq_index_add": (_i, [_vp, C.POINTER(IndexAddDesc)]),
    "lsq_index_reserve": (_i, [_vp, _i64]),
    "lsq_index_get_growth_info": (_i, [_vp, C.POINTER(IndexGrowthInfo)]),
    # removing rows from the index (since v2200)
    "lsq_index_remove": (_i, [_vp, _vp, _i64, _i, _i]),
    "lsq_index_compact": (_i, [_vp, C.POINTER(IndexCompactDesc)]),
    "lsq_index_get_compact_info": (_i, [_vp, C.POINTER(IndexCompactInfo)]),
    # range search on the index: every row within a radius, and its host drop-in (since v2300)
    "lsq_index_range_search": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "lsq_index_range_fetch": (_i, [_vp, _vp, _vp, _i64, _i]),
    "lsq_index_get_range_info": (_i, [_vp, C.POINTER(RangeInfo)]),
    "lsq_range_search_cpu": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i]),
    # decode and search by stored row (since v2400)
    "lsq_reconstruct_cpu": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i, _i64, _i, _i, _i, _vp, _vp, _i, _i]),
    "lsq_index_reconstruct": (_i, [_vp, _vp, _i64, _vp, _i64, _i64, _i, _i, _i]),
    "lsq_index_search_rows": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i]),
    "lsq_index_get_recon_info": (_i, [_vp, C.POINTER(IndexReconInfo)]),
    # half-precision base rows (since v2500): the host narrowing, the device narrowing of a resident base, the stored rows read back
    "lsq_narrow_rows_cpu": (_i, [_vp, _vp, _i64, _i, _i64, _i64, _i, _i]),
    "lsq_index_narrow_base": (_i, [_vp, _i]),
    "lsq_index_get_base": (_i, [_vp, _vp, _i64, _i64, _i64, _i]),
    "lsq_index_get_base_info": (_i, [_vp, C.POINTER(IndexBaseInfo)]),
    # snapshots (since v2600): an index saved, loaded, exported and digested; the host-only writer, reader, inspector and digest
    "lsq_index_save": (_i, [_vp, C.c_char_p, _i]),
    "lsq_index_load": (_i, [C.POINTER(_vp), _vp, C.c_char_p, _i]),
    "lsq_index_export": (_i, [_vp, C.POINTER(SnapshotArrays), _i]),
    "lsq_index_digest": (_i, [_vp, C.POINTER(SnapshotInfo)]),
    "lsq_index_get_snapshot_info": (_i, [_vp, C.POINTER(SnapshotIoInfo)]),
    "lsq_snapshot_write_cpu": (_i, [C.c_char_p, C.POINTER(SnapshotArrays)]),
    "lsq_snapshot_read_cpu": (_i, [C.c_char_p, C.POINTER(SnapshotArrays)]),
    "lsq_snapshot_inspect_cpu": (_i, [C.c_char_p, C.POINTER(SnapshotInfo), _i]),
    "lsq_snapshot_digest_cpu": (_i, [_vp, _i64, _i64, C.POINTER(_u64)]),
    # the beam-search encoder on resident codebooks (since v1600)
    "lsq_encoder_create": (_i, [C.POINTER(_vp), _vp, C.POINTER(EncoderDesc)]),
    "lsq_encoder_destroy": (_i, [_vp]),
    "lsq_encoder_beam": (_i, [_vp, _vp, _i, _i64, _i, _vp, _vp, _vp, _i]),
    "lsq_encoder_get_info": (_i, [_vp, C.POINTER(EncoderInfo)]),
    # the coarse partition of a residual inverted-list index (since v1900), and its host checkers
    "lsq_partition_create": (_i, [C.POINTER(_vp), _vp, C.POINTER(PartitionDesc)]),
    "lsq_partition_destroy": (_i, [_vp]),
    "lsq_partition_get_centroids": (_i, [_vp, _vp, _i]),
    "lsq_partition_get_info": (_i, [_vp, C.POINTER(PartitionInfo)]),
    "lsq_partition_assign": (_i, [_vp, _vp, _i, _i64, _i, _vp, _vp, _i]),
    "lsq_partition_update": (_i, [_vp, _vp, _i, _i64, _i, _vp, _vp, _i]),
    "lsq_partition_residuals": (_i, [_vp, _vp, _i, _i64, _i, _vp, _vp, _i, _i]),
    "lsq_partition_code_norms": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i]),
    "lsq_partition_update_cpu": (_i, [_vp, _vp, _vp, _i, _i64, _i, _i, _vp, _i, _i]),
    "lsq_partition_residuals_cpu": (_i, [_vp, _i, _vp, _i, _i64, _i, _i, _vp, _vp, _i, _i]),
    "lsq_partition_code_norms_cpu": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _vp, _i, _i]),
    "lsq_quantize_norms": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i64, _i, _i, _vp, _vp, _vp]),
    "lsq_quantize_norms_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i64, _i, _i, _vp, _vp, _vp]),
    "lsq_update_codebooks": (_i, [_vp, _vp, _i, _i64, _i, _i, _i, _vp]),
    "lsq_update_codebooks_lsmr": (_i, [_vp, _vp, _i, _i64, _i, _i, _i, _vp]),
    "lsq_update_codebooks_gpu": (_i, [_vp, _vp, _vp, _i, _i64, _i, _i, _vp, C.POINTER(_i)]),
    "lsq_update_codebooks_dev": (_i, [_vp, _vp, _vp, _i, _i64, _i, _i, _vp, C.POINTER(_i)]),
    "lsq_update_codebooks_struct": (_i, [_vp, _vp, _vp, _i, _i64, _i, _i, _i, _vp]),
    "lsq_update_codebooks_struct_gpu": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, C.POINTER(_i)]),
    "lsq_update_codebooks_struct_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, C.POINTER(_i)]),
    "lsq_update_codebooks_spgl1": (_i, [_vp, _vp, _vp, _i, _i64, _i, _i, C.c_double, _vp, _i64, C.POINTER(Spgl1Params), _vp, C.POINTER(Spgl1Info)]),
    "lsq_update_codebooks_spgl1_dev": (_i, [_vp, _vp, _vp, _i, _i64, _i, _i, C.c_double, _vp, _i64, C.POINTER(Spgl1Params), _vp, C.POINTER(Spgl1Info)]),
    "lsq_encode_viterbi": (_i, [_vp, _vp, _vp, _i, _i64, _i, _i, _vp]),
    "lsq_encode_viterbi_dev": (_i, [_vp, _vp, _vp, _i, _i64, _i, _i, _vp]),
    "lsq_assign_codewords": (_i, [_vp, _vp, _vp, _i, _i64, _i, _i, _vp, _vp]),
    "lsq_assign_codewords_dev": (_i, [_vp, _vp, _vp, _i, _i64, _i, _i, _vp, _vp]),
    "lsq_update_centers": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, _vp]),
    "lsq_update_centers_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, _vp]),
    "lsq_kmeanspp_seed": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, _vp, _vp]),
    "lsq_kmeanspp_seed_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, _vp, _vp]),
    "lsq_synth_data_u8_dev": (_i, [_vp, _u64, _u64, _i64, _i, _vp]),
    "lsq_randinit_dev": (_i, [_vp, _u64, _u64, _i64, _i, _i, _vp]),
    "lsq_synth_codebooks_dev": (_i, [_vp, _u64, _i, _i, _i, _vp]),
}

MIN_VERSION = 2600     # the version floor: the oldest library that exports every symbol above with these structs

_libs = {}


def load(tuning=False):
    """Load the shared library (once per flavour).  Raises if it has not been built."""
    path = TUNING_LIB_PATH if tuning else LIB_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise RuntimeError(
                "%s not found: the HIP extension is not built. Run `python -c \"import __graft_entry__ as g; "
                "g.build()\"` -- there is no CPU fallback." % path)
        # torch bundles its own libamdhip64.so / libhsa-runtime64.so (SONAME libamdhip64.so.7).  Two HIP
        # runtimes in one process cannot both own the GPU ("No HIP GPUs are available" in whichever
        # initialises second), so when torch is installed it must be loaded FIRST: our DT_NEEDED
        # libamdhip64.so.7 then resolves to the copy already in the process.  A pure-C consumer (the
        # Julia ccall shim of INTEGRATION.md) simply gets /opt/rocm's runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)       # AttributeError if the symbol is missing: loud by design
            fn.restype = res
            fn.argtypes = args
        if lib.lsq_version() < MIN_VERSION:
            raise RuntimeError("%s is version %d, this binding needs %d or later: rebuild it" % (path, lib.lsq_version(), MIN_VERSION))
        _libs[path] = lib
    return _libs[path]


def check(rc, lib=None):
    if rc != LSQ_OK:
        msg = (lib or load()).lsq_last_error()      # thread-local inside the library that failed
        raise LsqError(rc, msg.decode("utf-8", "replace") if msg else "")
    return rc
